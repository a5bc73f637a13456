"""The call shapes of ahocorasick_amd/strings.py against a stub in place of libacgpu.so (no GPU, no library): how often and with what
capacity an entry is called again after ACGPU_E_OVERFLOW, which exception a return code becomes, what an empty input passes, every
field of the acgpu_shard a device call hands over, and that a stream refuses the other errors= policy without a native call.

The stub stands where _native.lib() keeps the loaded library.  Every entry is a Python function named like the symbol; what
ctypes.byref(x) passes exposes x as arg._obj, so the stub fills n_out, base, first_bad and the handles as the library would."""
import ctypes
import itertools

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, Comm, Stream, Utf8Error

BASE, FIRST_BAD, BAD_HAYSTACK = 1000, 7, 2
OVF = N.E_OVERFLOW

# the position of `cap` in the argument list of every entry that has one (include/acgpu.h); its twin with _lossy has the same
CAP_AT = {"acgpu_match_u16": 5, "acgpu_match_u16_multi": 7, "acgpu_match_utf8": 5, "acgpu_match_batch_u16": 6, "acgpu_match_batch_utf8": 6,
          "acgpu_stream_feed": 6, "acgpu_stream_feed_utf8": 6, "acgpu_replace_u16": 7, "acgpu_replace_utf8": 7, "acgpu_replace_batch_u16": 8,
          "acgpu_replace_batch_utf8": 8, "acgpu_stream_replace_u16": 8, "acgpu_stream_replace_utf8": 8, "acgpu_match_device": 4,
          "acgpu_match_device_begin": 4, "acgpu_replace_device": 6}


def shard_fields(s):
    return {f: getattr(s, f) for f, _ in N.Shard._fields_}


class StubLib:
    """plan[name]: an iterator of (return code, n_out) answers, n_out an int or a function of the call's cap; (OK, 0) once it is
    used up.  calls: (name, args) of every call; caps[name]: the cap of each of its calls; shards: the acgpu_shard fields seen."""

    def __init__(self):
        self.plan, self.calls, self.caps, self.shards, self.objects = {}, [], {}, [], []

    def count(self, name):
        return sum(1 for n, _ in self.calls if n == name)

    def __getattr__(self, name):
        if not name.startswith("acgpu_"):
            raise AttributeError(name)

        def entry(*args):
            if name == "acgpu_strerror":
                return b"stub error"
            rc, n_out = next(self.plan.get(name, iter(())), (N.OK, 0))
            self.calls.append((name, args))
            cap_at = CAP_AT.get(name[:-6] if name.endswith("_lossy") else name)
            if cap_at is not None:
                cap = args[cap_at]
                self.caps.setdefault(name, []).append(cap)
                n_out = n_out(cap) if callable(n_out) else n_out
                if name.startswith("acgpu_stream_feed") and rc == N.OK:
                    ctypes.memset(args[5], 0, cap * args[4])  # zeroed records: the caller's "+ base" shows
            for a in args:
                if isinstance(a, ctypes.Array) and a._type_ is N.Shard:
                    self.shards += [shard_fields(s) for s in a]
                    for i, s in enumerate(a):
                        s.chain_exit = 70 + i
                o = getattr(a, "_obj", None)
                if isinstance(o, ctypes.c_uint64):
                    o.value = n_out
                elif isinstance(o, ctypes.c_int64):
                    o.value = BASE
                elif isinstance(o, ctypes.c_void_p):
                    o.value = 0x1000 + len(self.calls)  # a handle
                elif isinstance(o, N.Shard):
                    self.shards.append(shard_fields(o))
                    o.chain_exit = 70
                elif rc == N.E_ENCODING and hasattr(o, "first_bad"):
                    o.first_bad = FIRST_BAD
                    if hasattr(o, "bad_haystack"):
                        o.bad_haystack = BAD_HAYSTACK
            return None if name.endswith(("_free", "_close")) else rc
        entry.__name__ = name
        self.__dict__[name] = entry
        return entry


@pytest.fixture
def stub():
    saved, s = N._lib, StubLib()
    N._lib = s
    try:
        yield s
    finally:
        for o in s.objects:  # their handles are the stub's: nothing of theirs may reach the library
            o._h = None
        N._lib = saved


def automaton(stub, keywords=("ab", "cd", "e")):
    a = Automaton(N.MODE_LONGEST, list(keywords), True)
    stub.objects.append(a)
    return a


def stream(stub, with_ids=True):
    s = Stream(automaton(stub), with_ids=with_ids)
    stub.objects.append(s)
    return s


def lossy(name, errors):
    return name + "_lossy" if errors == "replace" else name


# ---- records calls ----------------------------------------------------------------------------------------------------------------
# (id, the entry's strict name, errors or None, columns, (src, n) positions, call(stub, input, cap), the empty input, an input)
def _rec(name, errors, cols, at, call, empty, some):
    return pytest.param(lossy(name, errors), cols, at, call, empty, some, id=lossy(name, errors))


def _kw(errors):
    return {} if errors is None else {"errors": errors}


RECORDS = [
    _rec("acgpu_match_u16", None, 3, (1, 2), lambda st, x, cap: automaton(st).match_host(x, True, cap=cap), np.zeros(0, np.uint16),
         np.arange(9, dtype=np.uint16)),
    _rec("acgpu_match_u16_multi", None, 2, (1, 2), lambda st, x, cap: automaton(st).match_host(x, False, cap=cap, devices=[0, 1]),
         np.zeros(0, np.uint16), np.arange(9, dtype=np.uint16)),
    _rec("acgpu_match_batch_u16", None, 4, (1, 3), lambda st, x, cap: automaton(st).match_batch(x, True, cap=cap), [], ["xab", "", "cd"]),
    _rec("acgpu_stream_feed", None, 3, (1, 2), lambda st, x, cap: stream(st).feed(x, cap=cap), np.zeros(0, np.uint16),
         np.arange(9, dtype=np.uint16)),
]
for _e in ("strict", "replace"):
    RECORDS += [
        _rec("acgpu_match_utf8", _e, 2, (1, 2), lambda st, x, cap, e=_e: automaton(st).match_utf8(x, False, cap=cap, errors=e), b"", b"xxabxx"),
        _rec("acgpu_match_batch_utf8", _e, 3, (1, 3), lambda st, x, cap, e=_e: automaton(st).match_batch_utf8(x, False, cap=cap, errors=e), [],
             [b"ab", b"", b"xcd"]),
        _rec("acgpu_stream_feed_utf8", _e, 3, (1, 2), lambda st, x, cap, e=_e: stream(st).feed_utf8(x, cap=cap, errors=e), b"", b"xxabxx"),
    ]


@pytest.mark.parametrize("name,cols,at,call,empty,some", RECORDS)
def test_records_call_follows_every_overflow_with_exactly_the_reported_capacity(stub, name, cols, at, call, empty, some):
    stub.plan[name] = iter([(OVF, 5), (OVF, 9), (OVF, 33), (N.OK, 4)])
    r = call(stub, some, 1)
    assert stub.caps[name] == [1, 5, 9, 33] and stub.count(name) == 4
    assert r.shape == (4, cols)
    if "stream" in name:
        assert r.dtype == np.int64 and (r[:, :2] == BASE).all() and (r[:, 2:] == 0).all()
    else:
        assert r.dtype == np.int32


@pytest.mark.parametrize("name,cols,at,call,empty,some", RECORDS)
def test_records_call_maps_the_return_code(stub, name, cols, at, call, empty, some):
    for code in (N.E_INVALID, N.E_HIP, N.E_UNSUPPORTED):
        stub.plan[name] = iter([(code, 0)])
        with pytest.raises(N.AcgpuError) as ei:
            call(stub, some, None)
        assert ei.value.code == code and str(ei.value).startswith(name + ":")
    if "utf8" in name and not name.endswith("_lossy"):
        stub.plan[name] = iter([(OVF, 6), (N.E_ENCODING, 0)])  # (after a retry as well)
        with pytest.raises(Utf8Error) as ei:
            call(stub, some, 2)
        assert ei.value.start == FIRST_BAD and ei.value.haystack == (BAD_HAYSTACK if "batch" in name else None)
        assert stub.caps[name][-2:] == [2, 6]


@pytest.mark.parametrize("name,cols,at,call,empty,some", RECORDS)
def test_records_call_of_an_empty_input_passes_a_buffer_and_no_units(stub, name, cols, at, call, empty, some):
    r = call(stub, empty, None)
    (_, args), = [c for c in stub.calls if c[0] == name]
    assert args[at[0]].value and args[at[1]] == 0  # (non-null: the library refuses a null text even for n = 0)
    assert ctypes.cast(args[at[0]], ctypes.POINTER(ctypes.c_uint8))[0] == 0  # one readable element
    assert r.shape == (0, cols) and stub.caps[name] == [4096]


# ---- rewrite calls ----------------------------------------------------------------------------------------------------------------
def _rw(name, errors, call):
    return pytest.param(lossy(name, errors), call, id=lossy(name, errors))


REWRITES = [_rw("acgpu_replace_u16", None, lambda st, cap: automaton(st).replace_host(np.arange(9, dtype=np.uint16), "<>", cap=cap)),
            _rw("acgpu_replace_batch_u16", None, lambda st, cap: automaton(st).replace_batch(["xab", "", "cd"], ["1", "2", "3"], cap=cap))]
STREAM_REWRITES = [_rw("acgpu_stream_replace_u16", None, lambda st, cap: stream(st).replace_feed("xxabxx", "<>", cap=cap))]
for _e in ("strict", "replace"):
    REWRITES += [_rw("acgpu_replace_utf8", _e, lambda st, cap, e=_e: automaton(st).replace_utf8(b"xxabxx", "<>", cap=cap, errors=e)),
                 _rw("acgpu_replace_batch_utf8", _e,
                     lambda st, cap, e=_e: automaton(st).replace_batch_utf8([b"ab", b"", b"xcd"], [b"1", "2", b"3"], cap=cap, errors=e))]
    STREAM_REWRITES += [_rw("acgpu_stream_replace_utf8", _e, lambda st, cap, e=_e: stream(st).replace_feed_utf8(b"xxabxx", "<>", cap=cap, errors=e))]


@pytest.mark.parametrize("name,call", REWRITES)
def test_automaton_rewrite_call_retries_exactly_once(stub, name, call):
    stub.plan[name] = iter([(OVF, 50), (N.OK, 42)])
    r = call(stub, 3)
    assert stub.caps[name] == [3, 50] and len(r[0]) == 42 and r[0].dtype == (np.uint8 if "utf8" in name else np.uint16)
    assert set(r[-1]) == {f for f, _ in N.ReplaceStats._fields_}
    if "batch" in name:
        assert r[1].dtype == np.uint64 and len(r[1]) == 4

    stub.caps.clear()
    stub.plan[name] = itertools.repeat((OVF, 50))  # a second overflow is an error, however much it asks for
    with pytest.raises(N.AcgpuError) as ei:
        call(stub, 3)
    assert ei.value.code == OVF and stub.caps[name] == [3, 50] and str(ei.value).startswith(name + ":")

    stub.caps.clear()
    stub.plan[name] = iter([(OVF, lambda cap: cap + 1), (OVF, lambda cap: cap + 1)])
    with pytest.raises(N.AcgpuError) as ei:
        call(stub, None)
    assert ei.value.code == OVF and len(stub.caps[name]) == 2 and stub.caps[name][1] == stub.caps[name][0] + 1


@pytest.mark.parametrize("name,call", STREAM_REWRITES)
def test_stream_rewrite_call_retries_while_the_entry_asks_for_more(stub, name, call):
    stub.plan[name] = iter([(OVF, 10), (OVF, 20), (OVF, 40), (N.OK, 3)])
    r = call(stub, 1)
    assert stub.caps[name] == [1, 10, 20, 40] and len(r) == 3

    for asked in (lambda cap: cap, lambda cap: cap - 1, lambda cap: 0):  # overflow that asks for no more than it was given
        stub.caps.clear()
        stub.plan[name] = iter([(OVF, 10), (OVF, asked), (N.OK, 0)])
        with pytest.raises(N.AcgpuError) as ei:
            call(stub, 1)
        assert ei.value.code == OVF and stub.caps[name] == [1, 10] and str(ei.value).startswith(name + ":")


@pytest.mark.parametrize("name,call", REWRITES + STREAM_REWRITES)
def test_rewrite_call_maps_the_return_code(stub, name, call):
    stub.plan[name] = iter([(N.E_UNSUPPORTED, 0)])
    with pytest.raises(N.AcgpuError) as ei:
        call(stub, None)
    assert ei.value.code == N.E_UNSUPPORTED and stub.count(name) == 1 and str(ei.value).startswith(name + ":")
    if "utf8" in name and not name.endswith("_lossy"):
        stub.plan[name] = iter([(OVF, 60), (N.E_ENCODING, 0)])
        with pytest.raises(Utf8Error) as ei:
            call(stub, 2)
        assert ei.value.start == FIRST_BAD and ei.value.haystack == (BAD_HAYSTACK if "batch" in name else None)


# ---- the acgpu_shard of the device calls ----------------------------------------------------------------------------------------------
def shard(d_hay, n_units, own, text_begin, text_end, chain_entry, d_result=None):
    return dict(d_hay=d_hay, n_units=n_units, own_begin=own[0], own_end=own[1], text_begin=text_begin, text_end=text_end,
                chain_entry=chain_entry, chain_exit=-1, d_result=d_result)


EXPLICIT = dict(own=(8, 40), text_begin=False, text_end=True, chain_entry=5)


def test_shard_of_match_device(stub):
    a = automaton(stub)
    assert a.match_device(0x100, 64, True, 0x200, 8) == (0, N.OK, None, 70)
    assert a.match_device(0x100, 64, False, 0x200, 8, own=(8, 40), text_begin=True, text_end=False)[3] == 70
    a.match_device(0x100, 64, False, 0x200, 8, d_result=0x300, **EXPLICIT)
    assert stub.shards == [shard(0x100, 64, (0, 64), 1, 1, 0), shard(0x100, 64, (8, 40), 1, 0, 8), shard(0x100, 64, (8, 40), 0, 1, 5, 0x300)]
    assert [args[2] for _, args in stub.calls[-3:]] == [N.REC_MAP, N.REC_SET, N.REC_SET]


def test_shard_of_count_device_and_replace_device(stub):
    a = automaton(stub)
    rc, stats, chain_exit = a.count_device(0x100, 64, 0x200)
    assert (rc, chain_exit) == (N.OK, 70) and set(stats) == {f for f, _ in N.CountStats._fields_}
    a.count_device(0x100, 64, 0x200, **EXPLICIT)
    assert stub.shards == [shard(0x100, 64, (0, 64), 1, 1, 0), shard(0x100, 64, (8, 40), 0, 1, 5)]
    del stub.shards[:]
    n_out, rc, stats = a.replace_device(0x100, 64, "<>", 0x200, 80)
    assert (n_out, rc) == (0, N.OK) and set(stats) == {f for f, _ in N.ReplaceStats._fields_}
    assert stub.shards == [shard(0x100, 64, (0, 64), 1, 1, 0)] and stub.caps["acgpu_replace_device"] == [80]


def test_shard_of_match_device_begin_stays_with_the_ticket(stub):
    a = automaton(stub)
    tk, rc = a.match_device_begin(0x100, 64, True, 0x200, 8)
    assert rc == N.OK and tk.handle.value and tk.chain_exit == 70
    tk2, _ = a.match_device_begin(0x100, 64, True, 0x200, 8, d_result=0x300, **EXPLICIT)
    assert stub.shards == [shard(0x100, 64, (0, 64), 1, 1, 0), shard(0x100, 64, (8, 40), 0, 1, 5, 0x300)]
    assert dict(shard_fields(tk2.shard), chain_exit=-1) == stub.shards[1]  # the one the library was given, not a copy of it
    tk2.shard.chain_exit = 99
    assert tk2.chain_exit == 99
    assert a.match_device_end(tk) == (0, N.OK, None) and stub.calls[-1][1][1] is tk.handle


def test_shards_of_match_device_allgather(stub):
    a = automaton(stub)
    comm = Comm([0, 1, 2])
    stub.objects.append(comm)
    rc, counts, exits, profs = comm.match_device_allgather(a, [dict(d_hay=0x100 * (i + 1), n_units=64 + i) for i in range(3)], True,
                                                           [0x10, 0x20, 0x30], 16)
    assert (rc, counts, exits, profs) == (N.OK, [0, 0, 0], [70, 71, 72], None)
    assert stub.shards == [shard(0x100, 64, (0, 64), 1, 0, 0), shard(0x200, 65, (0, 65), 0, 0, 0), shard(0x300, 66, (0, 66), 0, 1, 0)]
    del stub.shards[:]
    comm.match_device_allgather(a, [dict(d_hay=0x100, n_units=64, own=(8, 40), text_begin=False, text_end=True, chain_entry=5),
                                    dict(d_hay=0x200, n_units=64, own=(4, 60), text_begin=True, text_end=False),
                                    dict(d_hay=0x300, n_units=64, own=(0, 64), text_begin=True, text_end=True, chain_entry=-1)], False,
                                [0x10, 0x20, 0x30], 16, profile=True)
    assert stub.shards == [shard(0x100, 64, (8, 40), 0, 1, 5), shard(0x200, 64, (4, 60), 1, 0, 4), shard(0x300, 64, (0, 64), 1, 1, -1)]


def test_profile_dict_of_the_device_calls(stub):
    a = automaton(stub)
    keys = {"scan_ms", "finalize_ms", "total_ms", "scan_units", "n_matches", "scan_kernel"}
    pd = a.match_device(0x100, 64, True, 0x200, 8, profile=True)[2]
    assert set(pd) == keys and pd["scan_kernel"] == "" and pd["scan_units"] == 0
    tk, _ = a.match_device_begin(0x100, 64, True, 0x200, 8, profile=True)
    assert set(a.match_device_end(tk, profile=True)[2]) == keys


# ---- a stream's policy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,second", [("strict", "replace"), ("replace", "strict")])
def test_stream_refuses_the_other_policy_before_any_native_call(stub, first, second):
    feeds = (lambda s, e: s.feed_utf8(b"ab", errors=e), lambda s, e: s.replace_feed_utf8(b"ab", "x", errors=e))
    for mk1 in feeds:
        for mk2 in feeds:
            s = stream(stub)
            mk1(s, first)
            n_calls = len(stub.calls)
            with pytest.raises(ValueError, match="errors"):
                mk2(s, second)
            assert len(stub.calls) == n_calls
            mk1(s, first)
            assert len(stub.calls) == n_calls + 1 and stub.calls[-1][0].endswith("_lossy") == (first == "replace")
