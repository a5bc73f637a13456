"""The cover entries without a GPU (include/acgpu.h: acgpu_cover_u16 / _device / _utf8 / _utf8_lossy; ahocorasick_amd/cover.py): the
tests' own reference against str.replace and re.sub, the symbols and the two structs, every argument decision that is made before
a device is touched, and the wrappers' argument checks and capacity rule against the stub of tests/test_binding_calls_cpu.py."""
import ctypes
import importlib
import re

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickSet, Automaton, Utf8Error, utf16
from tests.cover_ref import byte_records, cover_ref
from tests.test_binding_calls_cpu import FIRST_BAD, OVF, automaton, stub  # noqa: F401 (stub: the fixture)

C = importlib.import_module("ahocorasick_amd.cover")  # (the package's name `cover` is the function)
ENTRIES = ["acgpu_cover_u16", "acgpu_cover_device", "acgpu_cover_utf8", "acgpu_cover_utf8_lossy"]
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
to_str = lambda u: np.asarray(u, np.uint16).tobytes().decode("utf-16-le")


# ---- the reference -----------------------------------------------------------------------------------------------------------
def _finditer(pattern, text):
    return np.array([m.span() for m in re.finditer(pattern, text)], np.int32).reshape(-1, 2)


@pytest.mark.parametrize("text,kw", [("xx ab yy ab", "ab"), ("ab", "ab"), ("abxab", "ab"), ("nothing here", "ab"), ("", "ab")])
def test_reference_drop_is_str_replace_where_no_two_matches_touch(text, kw):
    recs = _finditer(re.escape(kw), text)
    assert to_str(cover_ref(utf16(text), recs, utf16("#-#"), (), "drop")) == text.replace(kw, "#-#")
    assert to_str(cover_ref(utf16(text), recs, (), (), "drop")) == text.replace(kw, "")
    assert to_str(cover_ref(utf16(text), recs, utf16("<"), utf16(">"), "keep")) == text.replace(kw, "<" + kw + ">")
    assert to_str(cover_ref(utf16(text), recs, (), (), "fill", ord("*"))) == text.replace(kw, "*" * len(kw))


def test_reference_touching_matches_give_one_replacement():
    text = "zababz ab abab"
    recs = _finditer("ab", text)
    assert recs.tolist()[:2] == [[1, 3], [3, 5]]
    assert to_str(cover_ref(utf16(text), recs, utf16("R"), (), "drop")) == re.sub("(?:ab)+", "R", text) == "zRz R R"
    assert text.replace("ab", "R") == "zRRz R RR"  # ... which is not what replace gives
    assert to_str(cover_ref(utf16(text), recs, utf16("["), utf16("]"), "keep")) == re.sub("((?:ab)+)", r"[\1]", text)
    assert to_str(cover_ref(utf16(text), recs, (), (), "fill", ord("#"))) == re.sub("ab", "##", text)


def test_reference_overlapping_and_nested_records():
    text = "xabcdex"
    recs = np.array([[1, 4], [2, 3], [3, 6]], np.int32)  # abc, b, cde: one span [1, 6)
    assert to_str(cover_ref(utf16(text), recs, utf16("("), utf16(")"), "keep")) == "x(abcde)x"
    assert to_str(cover_ref(utf16(text), recs, (), (), "fill", ord("*"))) == "x*****x"
    assert to_str(cover_ref(utf16(text), recs, (), (), "drop")) == "xx"


def test_reference_in_bytes():
    text = "aé€😀b"
    data = text.encode()
    units = utf16(text)
    recs = np.array([[1, 2], [3, 5]], np.int32)  # é, and the pair of 😀, in units
    rb = byte_records(recs, data)
    assert rb.tolist() == [[1, 3], [6, 10]]
    assert cover_ref(np.frombuffer(data, np.uint8), rb, (), (), "fill", ord("*")).tobytes() == b"a**\xe2\x82\xac****b"
    assert len(units) == 6


# ---- symbols and layout ------------------------------------------------------------------------------------------------------
def test_the_four_symbols_are_declared_and_exported():
    L = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert name in N.SYMBOLS and hasattr(L, name), name
    assert N.UTF8_STATS["acgpu_cover_utf8"] is N.Utf8Stats and N.UTF8_STATS["acgpu_cover_utf8_lossy"] is N.Utf8LossyStats
    assert N.lib().acgpu_abi_version() == N.ABI_VERSION == 5
    u64, vp_, P = ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER
    assert N.SIGNATURES["acgpu_cover_u16"][1] == [vp_, vp_, u64, P(N.CoverSpec), vp_, u64, P(u64), P(N.CoverStats)]
    assert N.SIGNATURES["acgpu_cover_device"][1] == [vp_, P(N.Shard), P(N.CoverSpec), vp_, u64, P(u64), vp_, P(N.CoverStats)]
    assert N.SIGNATURES["acgpu_cover_utf8_lossy"][1] == [vp_, vp_, u64, P(N.CoverSpec), vp_, u64, P(u64), P(N.CoverStats), P(N.Utf8LossyStats)]


def test_layout_of_the_structs():
    S = N.CoverSpec
    assert ctypes.sizeof(S) == 40
    assert [(f, getattr(S, f).offset, getattr(S, f).size) for f, _ in S._fields_] == [
        ("open", 0, 8), ("open_len", 8, 4), ("close", 16, 8), ("close_len", 24, 4), ("body", 28, 4), ("fill", 32, 4)]
    S = N.CoverStats
    assert ctypes.sizeof(S) == 40
    assert [(f, getattr(S, f).offset, getattr(S, f).size) for f, _ in S._fields_] == [
        ("n_records", 0, 8), ("n_spans", 8, 8), ("units_out", 16, 8), ("pieces", 24, 4), ("rescans", 28, 4), ("max_carry", 32, 4), ("reserved", 36, 4)]
    assert (N.COVER_KEEP, N.COVER_FILL, N.COVER_DROP) == (0, 1, 2)


# ---- decisions made before a device is touched -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def auto():
    return Automaton(N.MODE_ALL, ["ab", "b"], True)


def spec_of(dtype, open_=b"", close=b"", body=0, fill=ord("*"), open_len=None, close_len=None):
    o, c = np.frombuffer(open_, np.uint8).astype(dtype), np.frombuffer(close, np.uint8).astype(dtype)
    s = N.CoverSpec(o.ctypes.data if o.size else None, o.size if open_len is None else open_len, c.ctypes.data if c.size else None,
                    c.size if close_len is None else close_len, body, fill)
    s._keep = (o, c)
    return s


def _host(auto, name, hay, n, spec, out, cap, n_out=True):
    no, st = ctypes.c_uint64(77), N.CoverStats()
    tail = (None,) if "utf8" in name else ()
    rc = getattr(N.lib(), name)(auto.handle if auto is not None else None, hay, n, ctypes.byref(spec) if spec is not None else None, out, cap,
                                ctypes.byref(no) if n_out else None, ctypes.byref(st), *tail)
    return rc


@pytest.mark.parametrize("name,dtype", [("acgpu_cover_u16", np.uint16), ("acgpu_cover_utf8", np.uint8), ("acgpu_cover_utf8_lossy", np.uint8)])
def test_host_entries_refuse_bad_arguments_without_a_device(auto, name, dtype):
    hay, out = np.zeros(16, dtype), np.zeros(64, dtype)
    ok = spec_of(dtype, b"<", b">")
    assert _host(None, name, vp(hay), 16, ok, vp(out), 64) == N.E_INVALID                    # no automaton
    assert _host(auto, name, vp(hay), 16, None, vp(out), 64) == N.E_INVALID                  # no spec
    assert _host(auto, name, vp(hay), 16, ok, vp(out), 64, n_out=False) == N.E_INVALID       # no n_out
    assert _host(auto, name, None, 16, ok, vp(out), 64) == N.E_INVALID                       # a text without a pointer
    assert _host(auto, name, vp(hay), 16, ok, None, 64) == N.E_INVALID                       # a capacity without a buffer
    assert _host(auto, name, vp(hay), 1 << 31, ok, vp(out), 64) == N.E_INVALID               # n >= 2^31
    assert _host(auto, name, vp(hay), (1 << 40) + 3, ok, vp(out), 64) == N.E_INVALID
    assert _host(auto, name, vp(hay), 16, spec_of(dtype, body=3), vp(out), 64) == N.E_INVALID           # body > 2
    assert _host(auto, name, vp(hay), 16, spec_of(dtype, body=0xFFFFFFFF), vp(out), 64) == N.E_INVALID
    assert _host(auto, name, vp(hay), 16, spec_of(dtype, open_len=2), vp(out), 64) == N.E_INVALID       # open: a length without a pointer
    assert _host(auto, name, vp(hay), 16, spec_of(dtype, close_len=1), vp(out), 64) == N.E_INVALID      # close likewise
    assert _host(auto, name, vp(hay), 16, spec_of(dtype, b"<", open_len=1 << 31), vp(out), 64) == N.E_INVALID   # 2^31 elements of open
    assert _host(auto, name, vp(hay), 16, spec_of(dtype, b"", b">", close_len=1 << 31), vp(out), 64) == N.E_INVALID


def test_fill_must_fit_the_element(auto):
    hay8, out8 = np.zeros(16, np.uint8), np.zeros(64, np.uint8)
    for name in ("acgpu_cover_utf8", "acgpu_cover_utf8_lossy"):
        for fill in (0x80, 0xFF, 0x2022):
            assert _host(auto, name, vp(hay8), 16, spec_of(np.uint8, body=N.COVER_FILL, fill=fill), vp(out8), 64) == N.E_INVALID
    hay, out = np.zeros(16, np.uint16), np.zeros(64, np.uint16)
    assert _host(auto, "acgpu_cover_u16", vp(hay), 16, spec_of(np.uint16, body=N.COVER_FILL, fill=0x10000), vp(out), 64) == N.E_INVALID


def _shard(d_hay=0x10000, n=64, own=None, text_begin=True, text_end=True):
    sh = N.Shard()
    sh.d_hay, sh.n_units = d_hay, n
    sh.own_begin, sh.own_end = (0, n) if own is None else own
    sh.text_begin, sh.text_end = int(text_begin), int(text_end)
    sh.chain_entry, sh.chain_exit = sh.own_begin, -1
    return sh


def _device(auto, sh, spec="ok", d_out=0x20000, cap=8, n_out=True):
    no, st = ctypes.c_uint64(0), N.CoverStats()
    if spec == "ok":
        spec = spec_of(np.uint16, b"<", b">")
    return N.lib().acgpu_cover_device(auto.handle if auto is not None else None, ctypes.byref(sh) if sh is not None else None,
                                      ctypes.byref(spec) if spec is not None else None, d_out, cap, ctypes.byref(no) if n_out else None, None,
                                      ctypes.byref(st))


def test_device_entry_refuses_bad_arguments_without_a_device(auto):
    # (the pointers are never read: every decision here falls before a device is touched)
    assert _device(None, _shard()) == N.E_INVALID
    assert _device(auto, None) == N.E_INVALID
    assert _device(auto, _shard(), spec=None) == N.E_INVALID
    assert _device(auto, _shard(), n_out=False) == N.E_INVALID
    assert _device(auto, _shard(), d_out=None, cap=8) == N.E_INVALID
    assert _device(auto, _shard(), d_out=0x20001) == N.E_INVALID          # d_out not aligned to a unit
    assert _device(auto, _shard(d_hay=0x10002)) == N.E_INVALID            # d_hay not 16-byte aligned
    assert _device(auto, _shard(d_hay=None)) == N.E_INVALID               # units without a pointer
    assert _device(auto, _shard(n=1 << 31)) == N.E_INVALID                # n >= 2^31
    assert _device(auto, _shard(), spec=spec_of(np.uint16, body=3)) == N.E_INVALID
    assert _device(auto, _shard(), spec=spec_of(np.uint16, open_len=4)) == N.E_INVALID


@pytest.mark.parametrize("kw", [dict(own=(1, 64)), dict(own=(0, 63)), dict(text_begin=False), dict(text_end=False), dict(own=(16, 32))])
def test_device_entry_serves_a_whole_text_only(auto, kw):
    assert _device(auto, _shard(**kw)) == N.E_UNSUPPORTED
    for mode in (N.MODE_LONGEST, N.MODE_SHORTEST):
        assert _device(Automaton(mode, ["ab", "b"], True), _shard(**kw)) == N.E_UNSUPPORTED


@pytest.mark.parametrize("errors", ["strict", "replace"])
def test_the_empty_utf8_text_needs_no_device(auto, errors):
    name = "acgpu_cover_utf8" + ("_lossy" if errors == "replace" else "")
    no, st = ctypes.c_uint64(77), N.CoverStats(9, 9, 9, 9, 9, 9, 9)
    ust = N.UTF8_STATS[name]()
    spec = spec_of(np.uint8, b"<", b">")
    assert getattr(N.lib(), name)(auto.handle, None, 0, ctypes.byref(spec), None, 0, ctypes.byref(no), ctypes.byref(st), ctypes.byref(ust)) == N.OK
    assert no.value == 0 and (st.n_records, st.n_spans, st.units_out, st.pieces, st.rescans, st.max_carry) == (0, 0, 0, 0, 0, 0)
    assert ust.n_units == 0 and ust.ascii == 1
    for data in (b"", bytearray(), np.zeros(0, np.uint8)):
        assert C.cover_utf8(auto, data, open=b"<", close=b">", errors=errors) == b""
        assert C.mask_utf8(auto, data, errors=errors) == b""


# ---- the wrappers, against the stub ------------------------------------------------------------------------------------------
def test_wrappers_refuse_bad_arguments_before_a_native_call(stub):
    a = automaton(stub)
    for call in (lambda: C.cover(a, "xabx", body="mask"), lambda: C.cover_utf8(a, b"xabx", body=1), lambda: C.cover(a, "xabx", body=None),
                 lambda: C.cover_utf8(a, b"xabx", errors="ignore"), lambda: C.cover_utf8(a, b"xabx", fill="é"), lambda: C.mask_utf8(a, b"xabx", fill=b"\x80"),
                 lambda: C.mask_utf8(a, b"xabx", fill=b"**"), lambda: C.mask(a, "xabx", fill="**"), lambda: C.mask(a, "xabx", fill="😀"),
                 lambda: C.mask(a, "xabx", fill="")):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: C.cover(a, None), lambda: C.cover_utf8(a, None), lambda: C.cover(a, "x", open=None), lambda: C.cover(a, "x", close=None),
                 lambda: C.cover_utf8(a, b"x", open=None), lambda: C.cover_utf8(a, b"x", close=None), lambda: C.mask(a, "x", fill=None),
                 lambda: C.mask_utf8(a, b"x", fill=None), lambda: C.redact(a, "x", None), lambda: C.highlight(a, "x", "<", None),
                 lambda: C.redact_utf8(a, b"x", None), lambda: C.highlight_utf8(a, b"x", None, b">")):
        with pytest.raises(TypeError):
            call()
    assert not [n for n, _ in stub.calls if "cover" in n]


CALLS = [("acgpu_cover_u16", lambda a, n, **kw: C.cover(a, np.arange(n, dtype=np.uint16) + 1, **kw), "<b>", "</b>"),
         ("acgpu_cover_utf8", lambda a, n, **kw: C.cover_utf8(a, b"x" * n, **kw), b"<b>", "</b>"),
         ("acgpu_cover_utf8_lossy", lambda a, n, **kw: C.cover_utf8(a, b"x" * n, errors="replace", **kw), "<b>", b"</b>")]


def _caps(stub, name):
    return [args[5] for n, args in stub.calls if n == name]


@pytest.mark.parametrize("name,call,o,c", CALLS)
def test_wrappers_retry_once_with_the_exact_size(stub, name, call, o, c):
    a = automaton(stub)
    stub.plan[name] = iter([(OVF, 9001), (N.OK, 9001)])
    got = call(a, 100, open=o, close=c)
    assert len(got) == 9001
    assert _caps(stub, name) == [100 + 25 + 3 + 4, 9001]            # n + n // 4 + len(open) + len(close), then the reported size
    spec = [args[3]._obj for n, args in stub.calls if n == name][0]
    assert (spec.open_len, spec.close_len, spec.body) == (3, 4, N.COVER_KEEP)
    stub.calls.clear()
    stub.plan[name] = iter([(N.OK, 3)])
    assert len(call(a, 80000)) == 3 and _caps(stub, name) == [100000]
    stub.calls.clear()
    stub.plan[name] = iter([(OVF, 5000), (OVF, 5001), (N.OK, 5001)])
    with pytest.raises(N.AcgpuError) as e:
        call(a, 100)
    assert e.value.code == OVF and _caps(stub, name) == [125, 5000]  # a second overflow is an error, not a third call


def test_thin_wrappers_pass_the_spec_of_their_use(stub):
    s = AhoCorasickSet(["ab", "b"], True)
    stub.objects.append(s.automaton)

    def last_spec(name):
        args = [args for n, args in stub.calls if n == name][-1]
        assert args[0] == s.automaton.handle
        sp = args[3]._obj
        return sp.open_len, sp.close_len, sp.body, sp.fill

    C.mask(s, "xabx", fill="#")
    assert last_spec("acgpu_cover_u16") == (0, 0, N.COVER_FILL, ord("#"))
    C.highlight(s, "xabx", "<b>", "</b>")
    assert last_spec("acgpu_cover_u16")[:3] == (3, 4, N.COVER_KEEP)
    C.redact(s, "xabx", "é😀")
    assert last_spec("acgpu_cover_u16")[:3] == (3, 0, N.COVER_DROP)       # in UTF-16 units
    C.mask_utf8(s, b"xabx")
    assert last_spec("acgpu_cover_utf8") == (0, 0, N.COVER_FILL, ord("*"))
    C.highlight_utf8(s, b"xabx", "«", b">>", errors="replace")
    assert last_spec("acgpu_cover_utf8_lossy")[:3] == (2, 2, N.COVER_KEEP)  # a str is encoded as UTF-8
    C.redact_utf8(s, b"xabx", "é😀")
    assert last_spec("acgpu_cover_utf8")[:3] == (6, 0, N.COVER_DROP)


def test_utf8_wrapper_raises_utf8error_as_find_all_utf8_does(stub):
    a = automaton(stub)
    stub.plan["acgpu_cover_utf8"] = iter([(N.E_ENCODING, 0)])
    with pytest.raises(Utf8Error) as e:
        C.cover_utf8(a, b"ab\xffcd")
    assert e.value.start == FIRST_BAD and e.value.haystack is None


def test_device_wrapper_hands_over_a_whole_text_shard(stub):
    a = automaton(stub)
    stub.plan["acgpu_cover_device"] = iter([(OVF, 12)])
    n_out, rc, st = C.cover_device(a, 0x7000, 99, 0x9002, 5, open="<", body="drop", stream=0x33)
    assert (n_out, rc) == (12, OVF) and set(st) == {f for f, _ in N.CoverStats._fields_}
    sh = stub.shards[-1]
    assert (sh["d_hay"], sh["n_units"], sh["own_begin"], sh["own_end"], sh["text_begin"], sh["text_end"]) == (0x7000, 99, 0, 99, 1, 1)
    (name, args), = [c for c in stub.calls if c[0] == "acgpu_cover_device"]
    assert args[3] == 0x9002 and args[4] == 5 and args[6].value == 0x33
    assert (args[2]._obj.open_len, args[2]._obj.body) == (1, N.COVER_DROP)
