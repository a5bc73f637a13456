"""The batch spans and batch cover entries without a GPU (include/acgpu.h: acgpu_spans_batch_u16, acgpu_cover_batch_u16;
ahocorasick_amd/spans.py, cover.py): the symbols, every argument decision that is made before a device is touched, the wrappers'
argument checks and capacity rule against the stub of tests/test_binding_calls_cpu.py, and the tests' own reference at a seam."""
import ctypes
import importlib

import numpy as np
import pytest

import ahocorasick_amd
from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import AhoCorasickSet, Automaton, utf16
from tests.cover_batch_ref import cover_batch_ref, spans_batch_ref
from tests.cover_ref import cover_ref
from tests.test_binding_calls_cpu import OVF, automaton, stub  # noqa: F401 (stub: the fixture)
from tests.test_cover_cpu import spec_of

C = importlib.import_module("ahocorasick_amd.cover")  # (the package's names `cover` and `spans` are the functions)
S = importlib.import_module("ahocorasick_amd.spans")
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
to_str = lambda u: np.asarray(u, np.uint16).tobytes().decode("utf-16-le")


# ---- the reference -----------------------------------------------------------------------------------------------------------
def _find(text, kw):
    out, at = [], text.find(kw)
    while at >= 0:
        out.append((at, at + len(kw)))
        at = text.find(kw, at + 1)
    return np.array(out, np.int32).reshape(-1, 2)


def test_reference_a_seam_keeps_two_spans_where_the_joined_text_has_one():
    hays = [utf16("xab"), utf16("abx")]
    recs = [_find("xab", "ab"), _find("abx", "ab")]
    units, off = cover_batch_ref(hays, recs, utf16("R"), (), "drop")
    assert to_str(units) == "xRRx" and off.tolist() == [0, 2, 4]
    joined = "xababx"
    assert to_str(cover_ref(utf16(joined), _find(joined, "ab"), utf16("R"), (), "drop")) == "xRx"
    assert spans_batch_ref(hays, recs).tolist() == [[0, 1, 3], [1, 0, 2]]
    units, off = cover_batch_ref(hays, recs, utf16("<"), utf16(">"), "keep")
    assert to_str(units) == "x<ab><ab>x" and off.tolist() == [0, 5, 10]
    units, off = cover_batch_ref([utf16(""), utf16("ab"), utf16("")], [_find("", "ab"), _find("ab", "ab"), _find("", "ab")], (), (), "fill")
    assert to_str(units) == "**" and off.tolist() == [0, 0, 2, 2]


# ---- symbols -----------------------------------------------------------------------------------------------------------------
def test_the_two_symbols_are_declared_and_exported():
    L = ctypes.CDLL(N.LIB_PATH)
    for name in ("acgpu_spans_batch_u16", "acgpu_cover_batch_u16"):
        assert name in N.SYMBOLS and hasattr(L, name), name
    assert N.lib().acgpu_abi_version() == N.ABI_VERSION == 5
    u64, u32, vp_, P = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER
    assert N.SIGNATURES["acgpu_spans_batch_u16"][1] == [vp_, vp_, vp_, u32, vp_, u64, P(u64), P(N.SpansStats)]
    assert N.SIGNATURES["acgpu_cover_batch_u16"][1] == [vp_, vp_, vp_, u32, P(N.CoverSpec), vp_, u64, vp_, P(u64), P(N.CoverStats)]
    for name in ("spans_batch", "cover_batch", "cover_batch_units", "mask_batch", "highlight_batch", "redact_batch"):
        assert name in ahocorasick_amd.__all__ and callable(getattr(ahocorasick_amd, name)), name


# ---- decisions made before a device is touched -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def auto():
    return Automaton(N.MODE_ALL, ["ab", "b"], True)


def _cover(auto, units, off, n, spec, out, cap, out_off, n_out=True):
    no, st = ctypes.c_uint64(77), N.CoverStats()
    rc = N.lib().acgpu_cover_batch_u16(auto.handle if auto is not None else None, units, off, n, ctypes.byref(spec) if spec is not None else None, out,
                                       cap, out_off, ctypes.byref(no) if n_out else None, ctypes.byref(st))
    return rc, no.value


def _spans(auto, units, off, n, out, cap, n_out=True):
    no, st = ctypes.c_uint64(77), N.SpansStats()
    rc = N.lib().acgpu_spans_batch_u16(auto.handle if auto is not None else None, units, off, n, out, cap, ctypes.byref(no) if n_out else None,
                                       ctypes.byref(st))
    return rc, no.value


def test_cover_batch_refuses_bad_arguments_without_a_device(auto):
    units, out = np.zeros(16, np.uint16), np.zeros(64, np.uint16)
    off, oo = np.array([0, 4, 4, 16], np.uint64), np.zeros(4, np.uint64)
    ok = spec_of(np.uint16, b"<", b">")
    E = N.E_INVALID
    assert _cover(None, vp(units), vp(off), 3, ok, vp(out), 64, vp(oo))[0] == E                    # no automaton
    assert _cover(auto, vp(units), None, 3, ok, vp(out), 64, vp(oo))[0] == E                       # no offsets
    assert _cover(auto, vp(units), vp(off), 3, ok, vp(out), 64, vp(oo), n_out=False)[0] == E       # no n_out
    assert _cover(auto, vp(units), vp(off), 3, None, vp(out), 64, vp(oo))[0] == E                  # no spec
    assert _cover(auto, vp(units), vp(off), 3, ok, vp(out), 64, None)[0] == E                      # no out_offsets
    assert _cover(auto, vp(units), vp(off), 3, ok, None, 64, vp(oo))[0] == E                       # a capacity without a buffer
    assert _cover(auto, None, vp(off), 3, ok, vp(out), 64, vp(oo))[0] == E                         # units without a pointer
    assert _cover(auto, vp(units), vp(np.array([0, 5, 4, 16], np.uint64)), 3, ok, vp(out), 64, vp(oo))[0] == E  # descending offsets
    assert _cover(auto, vp(units), vp(np.array([0, (1 << 31) - 1], np.uint64)), 1, ok, vp(out), 64, vp(oo))[0] == E  # 2^31 with the separator
    assert _cover(auto, vp(units), vp(np.array([0, 1 << 40], np.uint64)), 1, ok, vp(out), 64, vp(oo))[0] == E
    # everything check_spec refuses
    assert _cover(auto, vp(units), vp(off), 3, spec_of(np.uint16, body=3), vp(out), 64, vp(oo))[0] == E
    assert _cover(auto, vp(units), vp(off), 3, spec_of(np.uint16, open_len=2), vp(out), 64, vp(oo))[0] == E
    assert _cover(auto, vp(units), vp(off), 3, spec_of(np.uint16, close_len=1), vp(out), 64, vp(oo))[0] == E
    assert _cover(auto, vp(units), vp(off), 3, spec_of(np.uint16, b"<", open_len=1 << 31), vp(out), 64, vp(oo))[0] == E
    assert _cover(auto, vp(units), vp(off), 3, spec_of(np.uint16, body=N.COVER_FILL, fill=0x10000), vp(out), 64, vp(oo))[0] == E
    assert _cover(auto, vp(units), vp(off), 0, spec_of(np.uint16, body=3), vp(out), 64, vp(oo))[0] == E  # ... also for no haystacks


def test_spans_batch_refuses_bad_arguments_without_a_device(auto):
    units, out = np.zeros(16, np.uint16), np.zeros((64, 3), np.int32)
    off = np.array([0, 4, 4, 16], np.uint64)
    E = N.E_INVALID
    assert _spans(None, vp(units), vp(off), 3, vp(out), 64)[0] == E
    assert _spans(auto, vp(units), None, 3, vp(out), 64)[0] == E
    assert _spans(auto, vp(units), vp(off), 3, vp(out), 64, n_out=False)[0] == E
    assert _spans(auto, vp(units), vp(off), 3, None, 64)[0] == E
    assert _spans(auto, None, vp(off), 3, vp(out), 64)[0] == E
    assert _spans(auto, vp(units), vp(np.array([0, 5, 4, 16], np.uint64)), 3, vp(out), 64)[0] == E
    assert _spans(auto, vp(units), vp(np.array([0, (1 << 31) - 1], np.uint64)), 1, vp(out), 64)[0] == E


def test_no_haystacks_need_no_device(auto):
    off, oo = np.array([7], np.uint64), np.array([99], np.uint64)
    assert _cover(auto, None, vp(off), 0, spec_of(np.uint16, b"<", b">"), None, 0, vp(oo)) == (N.OK, 0)
    assert oo.tolist() == [0]
    assert _spans(auto, None, vp(off), 0, None, 0) == (N.OK, 0)
    assert S.spans_batch(auto, []).shape == (0, 3)
    assert C.cover_batch(auto, [], open="<") == [] and C.mask_batch(auto, []) == []
    units, out_off, st = C.cover_batch_units(auto, [])
    assert units.size == 0 and out_off.tolist() == [0] and st["units_out"] == 0


# ---- the wrappers, against the stub ------------------------------------------------------------------------------------------
def test_wrappers_refuse_bad_arguments_before_a_native_call(stub):
    a = automaton(stub)
    for call in (lambda: C.cover_batch(a, ["xabx"], body="mask"), lambda: C.cover_batch_units(a, ["xabx"], body=None),
                 lambda: C.mask_batch(a, ["xabx"], fill="**"), lambda: C.mask_batch(a, ["xabx"], fill="")):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: C.cover_batch(a, ["x", None]), lambda: S.spans_batch(a, [None]), lambda: C.cover_batch(a, ["x"], open=None),
                 lambda: C.cover_batch(a, ["x"], close=None), lambda: C.mask_batch(a, ["x"], fill=None), lambda: C.redact_batch(a, ["x"], None),
                 lambda: C.highlight_batch(a, ["x"], "<", None)):
        with pytest.raises(TypeError):
            call()
    assert not [n for n, _ in stub.calls if "cover" in n or "spans" in n]


def _caps(stub, name, at):
    return [args[at] for n, args in stub.calls if n == name]


def test_cover_batch_retries_once_with_the_exact_size(stub):
    a = automaton(stub)
    name = "acgpu_cover_batch_u16"
    hays = [np.arange(60, dtype=np.uint16) + 1, "", np.arange(40, dtype=np.uint16) + 1]
    stub.plan[name] = iter([(OVF, 9001), (N.OK, 9001)])
    units, out_off, st = C.cover_batch_units(a, hays, open="<b>", close="</b>")
    assert len(units) == 9001 and len(out_off) == 4 and set(st) == {f for f, _ in N.CoverStats._fields_}
    assert _caps(stub, name, 6) == [100 + 25 + 3 + 4, 9001]  # the batch's units n: n + n // 4 + len(open) + len(close), then the reported size
    args = [args for n, args in stub.calls if n == name][0]
    assert args[0] == a.handle and args[3] == 3 and (args[4]._obj.open_len, args[4]._obj.close_len, args[4]._obj.body) == (3, 4, N.COVER_KEEP)
    stub.calls.clear()
    stub.plan[name] = iter([(OVF, 5000), (OVF, 5001), (N.OK, 5001)])
    with pytest.raises(N.AcgpuError) as e:
        C.cover_batch_units(a, hays)
    assert e.value.code == OVF and _caps(stub, name, 6) == [125, 5000]  # a second overflow is an error, not a third call
    stub.calls.clear()
    stub.plan[name] = iter([(OVF, 700), (N.OK, 700)])
    assert len(C.cover_batch_units(a, hays, cap=16)[0]) == 700 and _caps(stub, name, 6) == [16, 700]


def test_spans_batch_retries_once_with_the_exact_size(stub):
    a = automaton(stub)
    name = "acgpu_spans_batch_u16"
    stub.plan[name] = iter([(OVF, 9001), (N.OK, 9001)])
    got = S.spans_batch(a, ["xab", "", "cd"])
    assert got.shape == (9001, 3) and got.dtype == np.int32 and _caps(stub, name, 5) == [4096, 9001]
    stub.calls.clear()
    stub.plan[name] = iter([(OVF, 5000), (OVF, 5001)])
    with pytest.raises(N.AcgpuError) as e:
        S.spans_batch(a, ["xab"])
    assert e.value.code == OVF and _caps(stub, name, 5) == [4096, 5000]


def test_thin_wrappers_pass_the_spec_of_their_use(stub):
    s = AhoCorasickSet(["ab", "b"], True)
    stub.objects.append(s.automaton)

    def last_spec():
        args = [args for n, args in stub.calls if n == "acgpu_cover_batch_u16"][-1]
        assert args[0] == s.automaton.handle and args[3] == 2
        sp = args[4]._obj
        return sp.open_len, sp.close_len, sp.body, sp.fill

    assert C.mask_batch(s, ["xabx", ""], fill="#") == ["", ""]  # (the stub writes nothing: every result is empty)
    assert last_spec() == (0, 0, N.COVER_FILL, ord("#"))
    C.highlight_batch(s, ["xabx", ""], "<b>", "</b>")
    assert last_spec()[:3] == (3, 4, N.COVER_KEEP)
    C.redact_batch(s, ["xabx", ""], "é😀")
    assert last_spec()[:3] == (3, 0, N.COVER_DROP)  # in UTF-16 units
