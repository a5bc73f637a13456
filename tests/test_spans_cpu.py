"""The spans entries without a GPU (include/acgpu.h: acgpu_spans_u16 / _device / _utf8 / _utf8_lossy; ahocorasick_amd/spans.py): the
tests' own reference against hand-written cases, the symbols and the stats struct, every argument decision that is made before a
device is touched, and the capacity rule of the Python wrappers against the stub of tests/test_binding_calls_cpu.py."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.spans import spans, spans_device, spans_utf8
from ahocorasick_amd.strings import AhoCorasickSet, Automaton, Utf8Error
from tests.spans_ref import merge
from tests.test_binding_calls_cpu import FIRST_BAD, OVF, automaton, stub  # noqa: F401 (stub: the fixture)

ENTRIES = ["acgpu_spans_u16", "acgpu_spans_device", "acgpu_spans_utf8", "acgpu_spans_utf8_lossy"]
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None


# ---- the reference -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recs,n,want", [
    ([], 5, []),                                   # empty
    ([], 0, []),
    ([(2, 4)], 9, [(2, 4)]),                       # one record
    ([(1, 5), (5, 8)], 9, [(1, 8)]),               # touching
    ([(1, 3), (0, 5)], 9, [(0, 5)]),               # nested, the longer record later
    ([(0, 2), (4, 5)], 9, [(0, 2), (4, 5)]),       # a record at unit 0
    ([(1, 2), (7, 9)], 9, [(1, 2), (7, 9)]),       # a record that ends at n
    ([(0, 9)], 9, [(0, 9)]),
    ([(1, 3), (2, 4), (5, 6), (6, 7), (9, 10)], 10, [(1, 4), (5, 7), (9, 10)]),
    ([(3, 4, 7), (1, 2, 0)], 5, [(1, 2), (3, 4)]),  # Map records, any order
])
def test_merge_against_hand_written_cases(recs, n, want):
    got = merge(np.array(recs, np.int32), n)
    assert got.dtype == np.int32 and got.shape == (len(want), 2) and got.tolist() == [list(w) for w in want]


# ---- symbols and layout ------------------------------------------------------------------------------------------------------
def test_the_four_symbols_are_declared_and_exported():
    L = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert name in N.SYMBOLS and hasattr(L, name), name
    assert N.UTF8_STATS["acgpu_spans_utf8"] is N.Utf8Stats and N.UTF8_STATS["acgpu_spans_utf8_lossy"] is N.Utf8LossyStats
    assert N.lib().acgpu_abi_version() == N.ABI_VERSION == 5


def test_layout_of_the_stats_struct():
    S = N.SpansStats
    assert ctypes.sizeof(S) == 32
    assert [(f, getattr(S, f).offset, getattr(S, f).size) for f, _ in S._fields_] == [
        ("n_records", 0, 8), ("n_spans", 8, 8), ("pieces", 16, 4), ("rescans", 20, 4), ("max_carry", 24, 4), ("reserved", 28, 4)]


# ---- decisions made before a device is touched -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def auto():
    return Automaton(N.MODE_ALL, ["ab", "b"], True)


def _host(auto, name, hay, n, out, cap, n_out=True, ust=False):
    no, st = ctypes.c_uint64(77), N.SpansStats()
    tail = (None,) if "utf8" in name else ()
    return getattr(N.lib(), name)(auto.handle, hay, n, out, cap, ctypes.byref(no) if n_out else None, ctypes.byref(st), *tail), no.value


@pytest.mark.parametrize("name,dtype", [("acgpu_spans_u16", np.uint16), ("acgpu_spans_utf8", np.uint8), ("acgpu_spans_utf8_lossy", np.uint8)])
def test_host_entries_refuse_bad_arguments_without_a_device(auto, name, dtype):
    hay, out = np.zeros(16, dtype), np.zeros((4, 2), np.int32)
    fn = getattr(N.lib(), name)
    tail = (None,) if "utf8" in name else ()
    no = ctypes.c_uint64(0)
    assert fn(None, vp(hay), 16, vp(out), 4, ctypes.byref(no), None, *tail) == N.E_INVALID       # no automaton
    assert _host(auto, name, vp(hay), 16, vp(out), 4, n_out=False)[0] == N.E_INVALID             # no n_out
    assert _host(auto, name, None, 16, vp(out), 4)[0] == N.E_INVALID                              # a text without a pointer
    assert _host(auto, name, vp(hay), 16, None, 4)[0] == N.E_INVALID                              # a capacity without a buffer
    assert _host(auto, name, vp(hay), 1 << 31, vp(out), 4)[0] == N.E_INVALID                      # n >= 2^31
    assert _host(auto, name, vp(hay), (1 << 40) + 3, vp(out), 4)[0] == N.E_INVALID


def _shard(d_hay=0x10000, n=64, own=None, text_begin=True, text_end=True):
    sh = N.Shard()
    sh.d_hay, sh.n_units = d_hay, n
    sh.own_begin, sh.own_end = (0, n) if own is None else own
    sh.text_begin, sh.text_end = int(text_begin), int(text_end)
    sh.chain_entry, sh.chain_exit = sh.own_begin, -1
    return sh


def _device(auto, sh, d_out=0x20000, cap=8, n_out=True):
    no, st = ctypes.c_uint64(0), N.SpansStats()
    return N.lib().acgpu_spans_device(auto.handle if auto is not None else None, ctypes.byref(sh) if sh is not None else None, d_out, cap,
                                      ctypes.byref(no) if n_out else None, None, ctypes.byref(st))


def test_device_entry_refuses_bad_arguments_without_a_device(auto):
    # (the pointers are never read: every decision here falls before a device is touched)
    assert _device(None, _shard()) == N.E_INVALID
    assert _device(auto, None) == N.E_INVALID
    assert _device(auto, _shard(), n_out=False) == N.E_INVALID
    assert _device(auto, _shard(), d_out=None, cap=8) == N.E_INVALID
    assert _device(auto, _shard(), d_out=0x20008) == N.E_INVALID          # d_out not 16-byte aligned
    assert _device(auto, _shard(d_hay=0x10002)) == N.E_INVALID            # d_hay not 16-byte aligned
    assert _device(auto, _shard(d_hay=None)) == N.E_INVALID               # units without a pointer
    assert _device(auto, _shard(n=1 << 31)) == N.E_INVALID                # n >= 2^31


@pytest.mark.parametrize("kw", [dict(own=(1, 64)), dict(own=(0, 63)), dict(text_begin=False), dict(text_end=False), dict(own=(16, 32))])
def test_device_entry_serves_a_whole_text_only(auto, kw):
    assert _device(auto, _shard(**kw)) == N.E_UNSUPPORTED
    for mode in (N.MODE_LONGEST, N.MODE_SHORTEST):
        assert _device(Automaton(mode, ["ab", "b"], True), _shard(**kw)) == N.E_UNSUPPORTED


@pytest.mark.parametrize("errors", ["strict", "replace"])
def test_the_empty_utf8_text_needs_no_device(auto, errors):
    name = "acgpu_spans_utf8" + ("_lossy" if errors == "replace" else "")
    no, st = ctypes.c_uint64(77), N.SpansStats(9, 9, 9, 9, 9, 9)
    ust = N.UTF8_STATS[name]()
    assert getattr(N.lib(), name)(auto.handle, None, 0, None, 0, ctypes.byref(no), ctypes.byref(st), ctypes.byref(ust)) == N.OK
    assert no.value == 0 and (st.n_records, st.n_spans, st.pieces, st.rescans, st.max_carry) == (0, 0, 0, 0, 0)
    assert ust.n_units == 0 and ust.ascii == 1
    for data in (b"", bytearray(), np.zeros(0, np.uint8)):
        got = spans_utf8(auto, data, errors=errors)
        assert got.shape == (0, 2) and got.dtype == np.int32


# ---- the wrappers' capacity rule, against the stub ---------------------------------------------------------------------------
def _caps(stub, name):
    return [args[4] for n, args in stub.calls if n == name]


CALLS = [("acgpu_spans_u16", lambda a, n: spans(a, np.arange(n, dtype=np.uint16) + 1), 2),
         ("acgpu_spans_utf8", lambda a, n: spans_utf8(a, b"x" * n), 1),
         ("acgpu_spans_utf8_lossy", lambda a, n: spans_utf8(a, b"x" * n, errors="replace"), 1)]


@pytest.mark.parametrize("name,call,_", CALLS)
def test_wrappers_retry_once_with_the_exact_count(stub, name, call, _):
    a = automaton(stub)
    stub.plan[name] = iter([(OVF, 9001), (N.OK, 9001)])
    got = call(a, 100)
    assert got.shape == (9001, 2) and got.dtype == np.int32
    assert _caps(stub, name) == [4096, 9001]                      # the guess: at least 4096 spans
    stub.calls.clear()
    stub.plan[name] = iter([(N.OK, 3)])
    assert call(a, 80000).shape == (3, 2) and _caps(stub, name) == [20000]   # ... a span per 4 elements of the text
    stub.calls.clear()
    stub.plan[name] = iter([(OVF, 5000), (OVF, 5001), (N.OK, 5001)])
    with pytest.raises(N.AcgpuError) as e:
        call(a, 100)
    assert e.value.code == OVF and _caps(stub, name) == [4096, 5000]  # a second overflow is an error, not a third call


def test_wrappers_take_a_set_or_a_map_and_pass_the_text(stub):
    s = AhoCorasickSet(["ab", "b"], True)
    stub.objects.append(s.automaton)
    assert spans(s, "xabx").shape == (0, 2)
    (name, args), = [c for c in stub.calls if c[0] == "acgpu_spans_u16"]
    assert args[0] == s.automaton.handle and args[2] == 4
    with pytest.raises(TypeError):
        spans(s, None)
    with pytest.raises(TypeError):
        spans_utf8(s, None)
    with pytest.raises(ValueError):
        spans_utf8(s, b"ab", errors="ignore")


def test_utf8_wrapper_raises_utf8error_as_find_all_utf8_does(stub):
    a = automaton(stub)
    stub.plan["acgpu_spans_utf8"] = iter([(N.E_ENCODING, 0)])
    with pytest.raises(Utf8Error) as e:
        spans_utf8(a, b"ab\xffcd")
    assert e.value.start == FIRST_BAD and e.value.haystack is None
    stub.plan["acgpu_match_utf8"] = iter([(N.E_ENCODING, 0)])
    with pytest.raises(Utf8Error) as e2:
        a.match_utf8(b"ab\xffcd", with_ids=False)
    assert (e2.value.start, e2.value.haystack) == (e.value.start, e.value.haystack)


def test_device_wrapper_hands_over_a_whole_text_shard(stub):
    a = automaton(stub)
    stub.plan["acgpu_spans_device"] = iter([(OVF, 12)])
    n_out, rc, st = spans_device(a, 0x7000, 99, 0x9000, 5, stream=0x33)
    assert (n_out, rc) == (12, OVF) and set(st) == {f for f, _ in N.SpansStats._fields_}
    sh = stub.shards[-1]
    assert (sh["d_hay"], sh["n_units"], sh["own_begin"], sh["own_end"], sh["text_begin"], sh["text_end"]) == (0x7000, 99, 0, 99, 1, 1)
    (name, args), = [c for c in stub.calls if c[0] == "acgpu_spans_device"]
    assert args[2] == 0x9000 and args[3] == 5 and args[5].value == 0x33
