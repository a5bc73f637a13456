"""GPU tests of acgpu_spans_utf8 / acgpu_spans_utf8_lossy (include/acgpu.h; csrc/acgpu_spans.hip): the spans of a UTF-8 text in byte
offsets of the caller's buffer.  Every expected value is tests/spans_ref.py's merge of the byte records that the tests of
find_all_utf8 expect (tests/test_gpu_utf8.py, tests/test_gpu_utf8_lossy.py: the CPU oracle on the decoded text, mapped to bytes)."""
import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.spans import spans_utf8
from ahocorasick_amd.strings import AhoCorasickSet, Utf8Error
from tests.spans_ref import merge
from tests.test_gpu_utf8 import expected, keywords_from, mixed_text, pair
from tests.test_gpu_utf8_lossy import every_unit
from tests.test_gpu_utf8_lossy import expected as expected_lossy

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20)]


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def pieces(p):
    if p:
        N.set_tunable("cursor_first_piece", p)
        N.set_tunable("cursor_max_piece", p)


def same(got, want):
    assert got.dtype == np.int32 and got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.fixture(scope="module")
def mixed():
    """a text of a few thousand bytes with sequences of 1, 2, 3 and 4 bytes, and per family a dictionary drawn from it"""
    rng = np.random.default_rng(77)
    text = mixed_text(rng, 1500)
    data = text.encode()
    assert 2000 < len(data) < 6000 and {len(ch.encode()) for ch in text} == {1, 2, 3, 4}
    cases = {}
    for mode in (N.MODE_ALL, N.MODE_LONGEST):
        kws = keywords_from(np.random.default_rng(78 + mode), text, mode, True)
        assert sum(1 for k in kws if ord(max(k)) >= 0x80) >= 3  # non-ASCII keywords
        a, orc = pair(mode, kws)
        recs_b = expected(orc, data)[1]
        cases[mode] = (a, recs_b, merge(recs_b[:, :2], len(data)))
    return data, cases


@pytest.mark.parametrize("p", [None, 3, 16])
@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_LONGEST])
def test_strict_mixed_text(mixed, mode, p):
    data, cases = mixed
    a, recs_b, want = cases[mode]
    assert len(want) >= 10 and len(want) < len(recs_b)  # (some records overlap or touch)
    pieces(p)
    st, ust = N.SpansStats(), None
    same(spans_utf8(a, data, stats=st), want)
    assert (st.n_records, st.n_spans) == (len(recs_b), len(want))
    if p:
        assert st.pieces >= len(data.decode()) // p


def test_ill_formed_text_raises_where_find_all_utf8_does(mixed):
    data, cases = mixed
    a = cases[N.MODE_ALL][0]
    for bad in (data[:1000] + b"\xff" + data[1000:], data + b"\xe2\x82", b"\x80" + data):
        with pytest.raises(Utf8Error) as want:
            a.match_utf8(bad, with_ids=False)
        with pytest.raises(Utf8Error) as got:
            spans_utf8(a, bad)
        assert (got.value.start, got.value.haystack) == (want.value.start, want.value.haystack)
    same(spans_utf8(a, data), cases[N.MODE_ALL][2])  # the pool is as usable as before


@pytest.mark.parametrize("p", [None, 3])
def test_lossy_stray_bytes_a_truncated_tail_and_a_replacement_keyword(p):
    text = "aé€😀kw".encode()
    data = (b"\x80" + text + b"\xbf\xbf" + text * 3 + b"\xc3(" + b"\xe2\x82" + b"x" + b"\xf0\x9f\x98" + text) * 40 + b"ab" + b"\xf0\x9f\x98"
    assert 2000 < len(data) < 6000
    a, orc = every_unit([b"k\x80w", "é😀".encode()])  # "k", "w", "é", both halves of the pair, U+FFFD and U+FFFD U+FFFD
    recs_b = expected_lossy(orc, data)[0]
    want = merge(recs_b[:, :2], len(data))
    assert len(want) >= 10 and want[-1].tolist()[1] == len(data)  # (the truncated tail is one U+FFFD, the last span ends at the buffer's end)
    pieces(p)
    st = N.SpansStats()
    same(spans_utf8(a, data, errors="replace", stats=st), want)
    assert (st.n_records, st.n_spans) == (len(recs_b), len(want))
    with pytest.raises(Utf8Error):
        spans_utf8(a, data)


@pytest.mark.parametrize("p", [None, 3, 16])
def test_a_lone_surrogate_keyword_on_supplementary_characters(p):
    s = AhoCorasickSet(["\ud83d", "\ude00", "ab", "b😀"], True)
    data = ("a😀b😀😀 ab😀.𝒜b " * 120).encode()
    assert 2000 < len(data) < 6000
    recs_b = s.find_all_utf8(data)
    assert len(recs_b) > 500
    want = merge(recs_b, len(data))
    pieces(p)
    same(spans_utf8(s, data), want)
