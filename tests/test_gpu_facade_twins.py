"""GPU tests of StringSet against StringMap (ahocorasick_amd/strings.py): the two flavours share their public methods through one
base, so for each of the five families a Set and the Map built with values = keywords must report the same matches -- the Map's rows
without their last column -- through every find_all* form, hand every match* listener exactly those rows (the Map the value as
well), stop a listener where it says so, and rewrite a text identically.  The text is small on purpose: a 2-, a 3- and a 4-byte
sequence, keywords that overlap ("ab", "abc", "bc"), one 0xFF byte that errors="replace" scans as U+FFFD, and the empty text."""
import io

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import (AhoCorasickMap, AhoCorasickSet, LongestMatchMap, LongestMatchSet, ShortestMatchMap, ShortestMatchSet,
                                     WholeWordLongestMatchMap, WholeWordLongestMatchSet, WholeWordMatchMap, WholeWordMatchSet)

pytestmark = pytest.mark.gpu

KEYWORDS = ["ab", "abc", "bc", "é", "日本", "x"]
WELL_FORMED = "x abc é 日本 😀 ab bc zabcab, 日本 x abc".encode()
DAMAGED = WELL_FORMED.replace(b"ab bc", b"ab\xffbc")
FAMILIES = {"AhoCorasick": (AhoCorasickSet, AhoCorasickMap), "LongestMatch": (LongestMatchSet, LongestMatchMap),
            "ShortestMatch": (ShortestMatchSet, ShortestMatchMap), "WholeWordMatch": (WholeWordMatchSet, WholeWordMatchMap),
            "WholeWordLongestMatch": (WholeWordLongestMatchSet, WholeWordLongestMatchMap)}
TEXTS = [pytest.param(DAMAGED, "replace", id="damaged-replace"), pytest.param(WELL_FORMED, "strict", id="well-formed-strict"),
         pytest.param(b"", "replace", id="empty-replace"), pytest.param(b"", "strict", id="empty-strict")]
_built = {}


@pytest.fixture(params=list(FAMILIES))
def twins(request):
    """(the family's Set, its Map with values = keywords), built once"""
    if request.param not in _built:
        set_cls, map_cls = FAMILIES[request.param]
        _built[request.param] = (set_cls(KEYWORDS, True), map_cls(KEYWORDS, KEYWORDS, True))
    return _built[request.param]


def batch_of(data):
    """haystacks for the batch forms, the empty one among them -> (list, the same as one buffer, its offsets)"""
    datas = [data, b"abc", b"", b"bc abc x", b"x ab"]  # (no object twice: a listener is told its haystack by identity)
    return datas, b"".join(datas), np.cumsum([0] + [len(d) for d in datas]).astype(np.uint64)


def test_the_text_is_what_the_docstring_says():
    assert len(DAMAGED) <= 200 and DAMAGED.count(b"\xff") == 1 and len(DAMAGED) == len(WELL_FORMED)
    assert {len(c.encode()) for c in WELL_FORMED.decode()} == {1, 2, 3, 4}
    with pytest.raises(UnicodeDecodeError):
        DAMAGED.decode()


@pytest.mark.parametrize("data,errors", TEXTS)
def test_set_rows_are_map_rows_without_the_last_column(twins, data, errors):
    s, m = twins
    datas, buf, offsets = batch_of(data)
    forms = {"find_all": lambda f: f.find_all(data.decode("utf-8", errors)),
             "find_all_utf8": lambda f: f.find_all_utf8(data, errors=errors),
             "find_all_utf8_readable": lambda f: f.find_all_utf8_readable(io.BytesIO(data), chunk_bytes=7, errors=errors),
             "find_all_batch_utf8": lambda f: f.find_all_batch_utf8(datas, errors=errors),
             "find_all_batch_utf8(offsets=)": lambda f: f.find_all_batch_utf8(buf, offsets=offsets, errors=errors)}
    got = {name: (form(s), form(m)) for name, form in forms.items()}
    for name, (rs, rm) in got.items():
        cols = 3 if "batch" in name else 2
        assert rs.shape == (len(rm), cols) and rm.shape == (len(rm), cols + 1) and rs.dtype == rm.dtype, name
        assert (rs == rm[:, :-1]).all(), name
        assert bool(len(rm)) == bool(data) or "batch" in name, name
        if len(rm):
            assert 0 <= rm[:, -1].min() and rm[:, -1].max() < len(KEYWORDS), name
    assert got["find_all_utf8_readable"][1].dtype == np.int64 and (got["find_all_utf8_readable"][1] == got["find_all_utf8"][1]).all()
    assert (got["find_all_batch_utf8"][1] == got["find_all_batch_utf8(offsets=)"][1]).all()
    if errors == "strict" and data:  # every row names its keyword: the Map's last column is the keyword's index, not something else
        assert [data[b:e].decode() for b, e, _ in got["find_all_utf8"][1].tolist()] == [KEYWORDS[k] for k in got["find_all_utf8"][1][:, 2].tolist()]


def listener_forms(data, errors):
    """name -> (call(facade, listener), rows(facade) of the find_all* form, the haystacks the listener may be handed | None)"""
    text = data.decode("utf-8", errors)
    texts = [text, "abc", "", "bc abc x", "x ab"]
    datas = batch_of(data)[0]
    with_ids = lambda f: hasattr(f, "_values")
    return {
        "match": (lambda f, fn: f.match(text, fn), lambda f: f.find_all(text).tolist(), [text]),
        "match_utf8": (lambda f, fn: f.match_utf8(data, fn, errors=errors), lambda f: f.find_all_utf8(data, errors=errors).tolist(), [data]),
        "match_utf8_readable": (lambda f, fn: f.match_utf8_readable(io.BytesIO(data), fn, chunk_bytes=7, errors=errors),
                                lambda f: f.find_all_utf8_readable(io.BytesIO(data), chunk_bytes=7, errors=errors).tolist(), None),
        "match_batch": (lambda f, fn: f.match_batch(texts, fn), lambda f: f.automaton.match_batch(texts, with_ids(f)).tolist(), texts),
        "match_batch_utf8": (lambda f, fn: f.match_batch_utf8(datas, fn, errors=errors),
                             lambda f: f.find_all_batch_utf8(datas, errors=errors).tolist(), datas),
    }


@pytest.mark.parametrize("data,errors", TEXTS[:2])
def test_listeners_get_the_rows_of_find_all_and_stop_where_they_say(twins, data, errors):
    for name, (call, rows, haystacks) in listener_forms(data, errors).items():
        batch = "batch" in name
        for f in twins:
            is_map = hasattr(f, "_values")
            want = rows(f)
            assert len(want) >= 4, name
            seen = []

            def listener(*args, stop_at=None):
                seen.append(args)
                return stop_at is None or sum(1 for a in seen if not batch or a[0] is args[0]) < stop_at
            call(f, listener)
            # what the listener got, as the rows of the find_all* form: the haystack (its index, for a batch) is its first argument
            got = []
            for args in seen:
                head, rest = (args[:1], args[1:]) if haystacks is not None else ((), args)
                if is_map:
                    assert rest[-1] in KEYWORDS
                    rest = rest[:-1] + (KEYWORDS.index(rest[-1]),)
                if haystacks is not None:
                    assert any(head[0] is h for h in haystacks), name  # the object itself, not a copy
                got.append(list(rest))
            strip = (lambda r: r[1:]) if batch else (lambda r: r)
            assert got == [strip(r) for r in want], (name, type(f).__name__)
            if batch:  # and each row with its own haystack
                assert [a[0] for a in seen] == [haystacks[r[0]] for r in want], name

            del seen[:]
            call(f, lambda *args: listener(*args, stop_at=2))
            if batch:
                per_haystack = np.bincount([r[0] for r in want], minlength=len(haystacks))
                assert max(per_haystack) >= 2 and len(seen) == int(np.minimum(per_haystack, 2).sum()), (name, type(f).__name__)
            else:
                assert len(seen) == 2, (name, type(f).__name__)
                assert [list(a[1:] if haystacks is not None else a)[:2] for a in seen] == [r[:2] for r in want[:2]], name


def replace_forms(data, errors):
    text = data.decode("utf-8", errors)
    datas, buf, offsets = batch_of(data)
    return {"replace": lambda f, r: f.replace(text, r),
            "replace_batch": lambda f, r: f.replace_batch([text, "abc", "", "x ab"], r),
            "replace_utf8": lambda f, r: f.replace_utf8(data, r, errors=errors),
            "replace_batch_utf8": lambda f, r: f.replace_batch_utf8(datas, r, errors=errors),
            "replace_batch_utf8(offsets=)": lambda f, r: f.replace_batch_utf8(buf, r, offsets=offsets, errors=errors),
            "replace_readable": lambda f, r: "".join(f.replace_readable(io.StringIO(text), r, chunk_chars=5)),
            "replace_utf8_readable": lambda f, r: b"".join(f.replace_utf8_readable(io.BytesIO(data), r, chunk_bytes=7, errors=errors))}


@pytest.mark.parametrize("data,errors", TEXTS)
def test_set_and_map_rewrite_a_text_identically(twins, data, errors):
    s, m = twins
    got = {}
    for name, form in replace_forms(data, errors).items():
        if isinstance(s, AhoCorasickSet):  # overlapping matches: the library refuses, for both flavours alike
            with pytest.raises(N.AcgpuError) as es:
                form(s, "<>")
            with pytest.raises(N.AcgpuError) as em:
                form(m, ["<>"] * len(KEYWORDS))
            assert es.value.code == em.value.code == N.E_UNSUPPORTED, name
            continue
        got[name] = out = form(s, "<>")
        assert out == form(m, ["<>"] * len(KEYWORDS)) == form(m, "<>"), name
        if name == "replace_utf8":  # replacements=None: every match by its value, here its own keyword -- the text itself
            assert form(m, None) == data
    if got:
        as_bytes = lambda t: t.encode("utf-8", "surrogatepass")
        if errors == "strict":
            assert as_bytes(got["replace"]) == as_bytes(got["replace_readable"]) == got["replace_utf8"] == got["replace_utf8_readable"]
        else:
            assert got["replace"] == got["replace_readable"] and got["replace_utf8"] == got["replace_utf8_readable"]
        assert got["replace_batch_utf8"] == got["replace_batch_utf8(offsets=)"] and got["replace_batch_utf8"][0] == got["replace_utf8"]
        assert got["replace_batch"][0] == got["replace"] and got["replace_batch"][2] == ""
        assert (b"<>" in got["replace_utf8"]) == bool(data) and (b"\xff" in got["replace_utf8"]) == (b"\xff" in data)
