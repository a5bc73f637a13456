"""CPU-side checks of the count-batch entries (include/acgpu.h: acgpu_count_batch_u16, acgpu_count_batch_utf8,
acgpu_count_batch_utf8_lossy): the layout of the stats, everything the entries decide before a device is touched, the host's
finishing pass (csrc/acgpu_terms_finish.h) through acgpu_debug_count_batch_finish and as a stand-alone program under the
sanitizers, and the one retry of ahocorasick_amd/terms.py against a stub in place of the library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ahocorasick_amd
from ahocorasick_amd import _native as N
from ahocorasick_amd import terms
from ahocorasick_amd.strings import AhoCorasickSet, Automaton, Utf8Error, _pack, _pack_utf8
from tests.helpers import WORD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
KWS = ["abc", "", "b", "abc"]  # an empty keyword and a duplicate
HAYS = ["zabcz", "", "b", "zz"]
ENTRIES = ("acgpu_count_batch_u16", "acgpu_count_batch_utf8", "acgpu_count_batch_utf8_lossy")
C64, C32 = 0x1122334455667788, 0x5A5A5A5A


class Out:
    """canaried output arrays of a call with room for `cap` entries of `n_hay` haystacks"""

    def __init__(self, n_hay, cap):
        self.row_ptr = np.full(n_hay + 3, C64, np.uint64)
        self.ids = np.full(cap + 2, C32, np.uint32)
        self.counts = np.full(cap + 2, C32, np.uint32)
        self.n_out = ctypes.c_uint64(99)

    def untouched(self):
        return bool((self.row_ptr == C64).all() and (self.ids == C32).all() and (self.counts == C32).all())


def call(entry, a, text, off, n_hay, out, cap, row_ptr=True, arrays=True, n_out=True, stats=True):
    """one native call -> (rc, count-batch stats); text: units for acgpu_count_batch_u16, bytes for the UTF-8 entries"""
    st = N.CountBatchStats(7, 7, 7, 7, 7, 7, 7)
    args = [a.handle if a else None, vp(text), vp(off), n_hay, vp(out.row_ptr) if row_ptr else None, vp(out.ids) if arrays else None,
            vp(out.counts) if arrays else None, cap, ctypes.byref(out.n_out) if n_out else None, ctypes.byref(st) if stats else None]
    if entry != "acgpu_count_batch_u16":
        args.append(None)
    return getattr(N.lib(), entry)(*args), st


def packed(entry, hays):
    return _pack(hays) if entry == "acgpu_count_batch_u16" else _pack_utf8([h.encode() for h in hays], None)


def test_layout_and_symbols():
    assert ctypes.sizeof(N.CountBatchStats) == 40
    want = (("n_records", 0, 8), ("n_entries", 8, 8), ("n_terms", 16, 8), ("pieces", 24, 4), ("rescans", 28, 4), ("rows_cut", 32, 4), ("reserved", 36, 4))
    assert [(f, getattr(N.CountBatchStats, f).offset, getattr(N.CountBatchStats, f).size) for f, _ in N.CountBatchStats._fields_] == list(want)
    L = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRIES + ("acgpu_debug_count_batch_finish",):
        assert name in N.SYMBOLS and hasattr(L, name), name
    assert N.lib().acgpu_count_batch_utf8.argtypes[-1] == ctypes.POINTER(N.Utf8BatchStats)
    assert N.lib().acgpu_count_batch_utf8_lossy.argtypes[-1] == ctypes.POINTER(N.Utf8LossyStats)
    assert N.TERMS_BLOCK == 2048
    assert ahocorasick_amd.count_batch is terms.count_batch and ahocorasick_amd.count_batch_utf8 is terms.count_batch_utf8


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_checks_leave_the_arrays_untouched(entry):
    a = Automaton(N.MODE_ALL, KWS, True)
    text, off = packed(entry, HAYS)
    n = len(HAYS)
    out = Out(n, 16)
    bad = lambda *args, **kw: call(entry, *args, **kw)[0] == N.E_INVALID
    assert bad(None, text, off, n, out, 16)
    assert bad(None, text, np.zeros(1, np.uint64), 0, out, 16)
    assert bad(a, text, None, n, out, 16)
    assert bad(a, text, None, 0, out, 16)
    assert bad(a, text, off, n, out, 16, row_ptr=False)  # NULL row_ptr
    assert bad(a, text, off, n, out, 16, arrays=False)   # NULL ids and counts with a capacity
    assert bad(a, text, off, n, out, 16, n_out=False)    # NULL n_out
    assert bad(a, text, off, 0, out, 0, n_out=False)
    assert bad(a, None, off, n, out, 16)                 # units to read, and no array
    assert bad(a, text, np.array([0, 5, 4, 6, 8], np.uint64), 4, out, 16)  # descending offsets
    assert bad(a, text, np.array([3, 0], np.uint64), 1, out, 16)
    # units (bytes) + haystacks of 2^31 or more: the concatenation would not fit a call (nothing is read before the check)
    for total, n_hay in (((1 << 31) - 1, 1), ((1 << 31) - 2, 2), (1 << 31, 1), (1 << 40, 1)):
        big = np.zeros(n_hay + 1, np.uint64)
        big[-1] = total
        assert bad(a, text, big, n_hay, out, 16), (total, n_hay)
    assert out.untouched() and out.n_out.value == 99


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("mode", [N.MODE_ALL, N.MODE_LONGEST, N.MODE_WHOLEWORD, N.MODE_SHORTEST, N.MODE_WWLONGEST])
def test_a_batch_with_nothing_to_scan_needs_no_device(entry, mode):
    a = Automaton(mode, ["ab", "b"], True, word_chars=WORD if mode in (N.MODE_WHOLEWORD, N.MODE_WWLONGEST) else None)
    # the empty batch: row_ptr[0] alone; cap == 0 with NULL arrays is a valid call
    for arrays, cap in ((True, 5), (False, 0)):
        out = Out(0, 5)
        rc, st = call(entry, a, None, np.zeros(1, np.uint64), 0, out, cap, arrays=arrays)
        assert rc == N.OK and out.n_out.value == 0 and out.row_ptr.tolist() == [0, C64, C64]
        assert (st.n_records, st.n_entries, st.n_terms, st.pieces, st.rescans, st.rows_cut, st.reserved) == (0,) * 7
        assert (out.ids == C32).all() and (out.counts == C32).all()
    out = Out(0, 5)
    assert call(entry, a, None, np.full(1, 12, np.uint64), 0, out, 0, arrays=False, stats=False)[0] == N.OK  # (a first offset that is not 0)
    # only empty haystacks, anywhere in a buffer
    out = Out(3, 5)
    rc, st = call(entry, a, None, np.full(4, 6, np.uint64), 3, out, 0, arrays=False)
    assert rc == N.OK and out.n_out.value == 0 and out.row_ptr.tolist() == [0, 0, 0, 0, C64, C64] and st.n_terms == 0
    indptr, indices, data = terms.count_batch(a, [])
    assert (indptr.dtype, indices.dtype, data.dtype) == (np.int64, np.int32, np.uint32)
    assert indptr.tolist() == [0] and indices.shape == data.shape == (0,)
    indptr, indices, data = terms.count_batch_utf8(a, [b"", b""], errors="replace" if entry.endswith("lossy") else "strict")
    assert indptr.tolist() == [0, 0, 0] and indices.shape == data.shape == (0,)


def test_without_a_device_the_call_fails_as_the_batch_match_call_does():
    a = Automaton(N.MODE_ALL, KWS, True)
    units, off = _pack(HAYS)
    recs = np.zeros((16, 4), np.int32)
    n_recs = ctypes.c_uint64(0)
    rc_match = N.lib().acgpu_match_batch_u16(a.handle, vp(units), vp(off), len(HAYS), N.REC_MAP, vp(recs), 16, ctypes.byref(n_recs))
    for entry in ENTRIES:
        text, toff = packed(entry, HAYS)
        out = Out(len(HAYS), 16)
        rc, st = call(entry, a, text, toff, len(HAYS), out, 16)
        assert rc == rc_match, entry
        if rc != N.OK:  # no device: nothing was written, and the wrappers raise the library's error
            assert rc in (N.E_NODEVICE, N.E_HIP) and out.untouched()
        else:  # "zabcz": b (2) and abc (the duplicate's last index, 3); "b": b
            assert out.row_ptr[:5].tolist() == [0, 2, 2, 3, 3] and out.ids[:3].tolist() == [2, 3, 2] and out.counts[:3].tolist() == [1, 1, 1]
            assert out.n_out.value == 3 and (st.n_records, st.n_entries, st.n_terms, st.rows_cut) == (3, 3, 3, 0)
    if rc_match != N.OK:
        with pytest.raises(N.AcgpuError):
            terms.count_batch(a, HAYS)
        with pytest.raises(N.AcgpuError):
            terms.count_batch(AhoCorasickSet(KWS, True), HAYS)
        with pytest.raises(N.AcgpuError):
            terms.count_batch_utf8(a, [h.encode() for h in HAYS])


# ---- the finishing pass ------------------------------------------------------------------------------------------------------------
def finish(entries, n_hay):
    """acgpu_debug_count_batch_finish on a list of (h, id, count) -> (rc, row_ptr, ids, counts, rows_cut); the outputs have exactly
    the promised sizes and canaries behind them"""
    e = np.array(entries, dtype=np.uint32).reshape(-1, 3)
    n = len(e)
    row_ptr, ids, counts = np.full(n_hay + 2, C64, np.uint64), np.full(n + 1, C32, np.uint32), np.full(n + 1, C32, np.uint32)
    n_terms, cut = ctypes.c_uint64(77), ctypes.c_uint32(77)
    rc = N.lib().acgpu_debug_count_batch_finish(vp(e) if n else None, n, n_hay, vp(row_ptr), vp(ids), vp(counts), ctypes.byref(n_terms),
                                                ctypes.byref(cut))
    assert row_ptr[-1] == C64 and ids[-1] == C32 and counts[-1] == C32
    if rc != N.OK:
        assert (row_ptr == C64).all() and (ids == C32).all() and (counts == C32).all() and (n_terms.value, cut.value) == (77, 77)
        return rc, None, None, None, None
    assert row_ptr[n_hay] == n_terms.value
    return rc, row_ptr[:n_hay + 1].tolist(), ids[:n_terms.value].tolist(), counts[:n_terms.value].tolist(), cut.value


def test_finishing_pass_on_hand_made_lists():
    # no cut
    assert finish([(0, 1, 2), (0, 5, 1), (1, 0, 3), (2, 4, 1), (2, 9, 7)], 3) == (N.OK, [0, 2, 3, 5], [1, 5, 0, 4, 9], [2, 1, 3, 1, 7], 0)
    # a row cut once, id 2 on both sides
    assert finish([(0, 3, 1), (1, 2, 4), (1, 7, 1), (1, 2, 5), (1, 8, 2), (2, 0, 1)], 3) == (N.OK, [0, 1, 4, 5], [3, 2, 7, 8, 0], [1, 9, 1, 2, 1], 1)
    # a row cut where the id only repeats
    assert finish([(0, 4, 1), (0, 4, 1)], 1) == (N.OK, [0, 1], [4], [2], 1)
    # five sub-rows: (5, 9) (5) (5, 6) (0, 9) (5)
    five = [(1, 5, 1), (1, 9, 1), (1, 5, 2), (1, 5, 3), (1, 6, 1), (1, 0, 4), (1, 9, 1), (1, 5, 10)]
    assert finish(five, 2) == (N.OK, [0, 0, 4], [0, 5, 6, 9], [4, 16, 1, 2], 1)
    # empty haystacks at the front, in the middle and at the end
    assert finish([(2, 1, 1), (5, 0, 2), (5, 3, 1)], 9) == (N.OK, [0, 0, 0, 1, 1, 1, 3, 3, 3, 3], [1, 0, 3], [1, 2, 1], 0)
    # two cut rows with an uncut one between them
    assert finish([(0, 1, 1), (0, 0, 1), (1, 2, 2), (3, 7, 1), (3, 8, 1), (3, 7, 1)], 4) == (N.OK, [0, 2, 3, 3, 5], [0, 1, 2, 7, 8], [1, 1, 2, 2, 1], 2)
    # zero entries
    assert finish([], 4) == (N.OK, [0, 0, 0, 0, 0], [], [], 0)
    assert finish([], 0) == (N.OK, [0], [], [], 0)
    # a haystack index that descends, or is not below n_haystacks: refused, nothing written
    assert finish([(0, 1, 1), (2, 1, 1), (1, 1, 1)], 3)[0] == N.E_HIP
    assert finish([(0, 1, 1), (3, 1, 1)], 3)[0] == N.E_HIP
    n_terms, cut = ctypes.c_uint64(0), ctypes.c_uint32(0)
    assert N.lib().acgpu_debug_count_batch_finish(None, 0, 1, None, None, None, ctypes.byref(n_terms), ctypes.byref(cut)) == N.E_INVALID


@pytest.mark.parametrize("seed", range(200))
def test_finishing_pass_on_random_splits_of_known_rows(seed):
    """rows drawn at random (np.unique of random ids), every row split into sub-rows at random points the way blocks and pieces cut
    a haystack's run of records: each sub-row is np.unique of a slice of the row's records"""
    rng = np.random.default_rng(seed)
    n_hay = int(rng.integers(1, 12))
    entries, want_ptr, want_ids, want_counts, want_cut = [], [0], [], [], 0
    for h in range(n_hay):
        recs = rng.integers(0, int(rng.integers(1, 30)), int(rng.integers(0, 40))) if rng.integers(4) else np.zeros(0, np.int64)
        u, c = np.unique(recs, return_counts=True)
        want_ids += u.tolist()
        want_counts += c.tolist()
        want_ptr.append(len(want_ids))
        cuts = np.sort(rng.integers(0, len(recs) + 1, int(rng.integers(0, 4)))) if len(recs) and rng.integers(2) else []
        parts = [p for p in np.split(recs, cuts) if len(p)]
        subs = [np.unique(p, return_counts=True) for p in parts]
        flat = [int(i) for su, _ in subs for i in su]
        want_cut += any(b <= a for a, b in zip(flat, flat[1:]))
        entries += [(h, int(i), int(k)) for su, sc in subs for i, k in zip(su, sc)]
    assert finish(entries, n_hay) == (N.OK, want_ptr, want_ids, want_counts, want_cut)


def test_finishing_pass_stand_alone_under_asan_ubsan(tmp_path):
    """tests/san_terms_finish.cpp: the host-only header with output arrays of exactly the promised sizes, as a program of its own"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    clang = os.path.join(rocm, "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        pytest.skip("no ROCm clang++")
    exe = tmp_path / "san_terms_finish"
    subprocess.check_call([clang, "-x", "c++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "ahocorasick_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "san_terms_finish.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "san_terms_finish: done" in out and "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]


# ---- the wrapper's one retry, against a stub in place of the library ------------------------------------------------------------------
class StubLib:
    """Stands where _native.lib() keeps the loaded library.  plan[name]: the (return code, n_out) answers of entry `name`, (OK, 0)
    once used up; caps[name]: the capacity of each of its calls (argument 7 of the three count-batch entries).  A successful
    answer fills row_ptr with n_out at its end and the first n_out ids and counts with 0, 1, 2, ..."""

    def __init__(self):
        self.plan, self.caps = {}, {}

    def __getattr__(self, name):
        if not name.startswith("acgpu_"):
            raise AttributeError(name)

        def entry(*args):
            if name == "acgpu_strerror":
                return b"stub error"
            if name == "acgpu_build":
                args[7]._obj.value = 0x1000
                return N.OK
            if name not in ENTRIES:  # (acgpu_free, acgpu_last_hip_error for an error's text)
                return None if name == "acgpu_free" else 0
            rc, n_out = next(self.plan.get(name, iter(())), (N.OK, 0))
            n_hay, cap = args[3], args[7]
            self.caps.setdefault(name, []).append(cap)
            args[8]._obj.value = n_out
            if rc == N.OK:
                assert n_out <= cap
                ctypes.cast(args[4], ctypes.POINTER(ctypes.c_uint64))[n_hay] = n_out
                for i in range(n_out):
                    ctypes.cast(args[5], ctypes.POINTER(ctypes.c_uint32))[i] = i
                    ctypes.cast(args[6], ctypes.POINTER(ctypes.c_uint32))[i] = i + 1
            if rc == N.E_ENCODING:
                args[10]._obj.first_bad, args[10]._obj.bad_haystack = 7, 2
            return rc
        entry.__name__ = name
        self.__dict__[name] = entry
        return entry


@pytest.fixture
def stub():
    saved, s = N._lib, StubLib()
    N._lib = s
    made = []
    s.made = made
    try:
        yield s
    finally:
        for a in made:  # their handles are the stub's: nothing of theirs may reach the library
            a._h = None
        N._lib = saved


CALLS = [("acgpu_count_batch_u16", lambda a: terms.count_batch(a, ["xab", "", "cd"])),
         ("acgpu_count_batch_utf8", lambda a: terms.count_batch_utf8(a, [b"xab", b"", b"cd"])),
         ("acgpu_count_batch_utf8_lossy", lambda a: terms.count_batch_utf8(a, b"xab\xffcd", offsets=[0, 3, 4, 6], errors="replace"))]


@pytest.mark.parametrize("name,run", CALLS, ids=[c[0] for c in CALLS])
def test_wrapper_retries_once_with_the_reported_capacity_and_no_more(stub, name, run):
    a = Automaton(N.MODE_LONGEST, ["ab", "cd"], True)
    stub.made.append(a)
    indptr, indices, data = run(a)  # no overflow: one call with the first capacity
    assert stub.caps[name] == [4096] and indptr.tolist() == [0, 0, 0, 0] and len(indices) == len(data) == 0
    stub.caps.clear()
    stub.plan[name] = iter([(N.E_OVERFLOW, 5000), (N.OK, 4999)])  # (the host merged one entry away)
    indptr, indices, data = run(a)
    assert stub.caps[name] == [4096, 5000]
    assert indptr.tolist() == [0, 0, 0, 4999] and indices.tolist() == list(range(4999)) and data.tolist() == list(range(1, 5000))
    assert (indptr.dtype, indices.dtype, data.dtype) == (np.int64, np.int32, np.uint32)
    stub.caps.clear()
    stub.plan[name] = iter([(N.E_OVERFLOW, 5000), (N.E_OVERFLOW, 6000), (N.OK, 10)])  # a second overflow is an error
    with pytest.raises(N.AcgpuError) as ei:
        run(a)
    assert ei.value.code == N.E_OVERFLOW and stub.caps[name] == [4096, 5000] and str(ei.value).startswith(name + ":")
    for code in (N.E_INVALID, N.E_HIP, N.E_NODEVICE):
        stub.caps.clear()
        stub.plan[name] = iter([(code, 0)])
        with pytest.raises(N.AcgpuError) as ei:
            run(a)
        assert ei.value.code == code and stub.caps[name] == [4096]


def test_wrapper_raises_utf8_error_for_an_ill_formed_haystack(stub):
    a = Automaton(N.MODE_LONGEST, ["ab", "cd"], True)
    stub.made.append(a)
    stub.plan["acgpu_count_batch_utf8"] = iter([(N.E_ENCODING, 0)])
    with pytest.raises(Utf8Error) as ei:
        terms.count_batch_utf8(a, [b"ab", b"", b"\xff"])
    assert ei.value.start == 7 and ei.value.haystack == 2
    with pytest.raises(ValueError):
        terms.count_batch_utf8(a, [b"ab"], errors="ignore")
    with pytest.raises(TypeError):
        terms.count_batch(a, ["ab", None])
