"""GPU tests of what the replace entries (include/acgpu.h: acgpu_replace_u16 / acgpu_replace_device / acgpu_replace_batch_u16;
csrc/acgpu_replace.hip) claim beyond the cases of test_gpu_replace.py and test_gpu_replace_batch.py: output positions, n_out and
out_offsets at and past 2^32 (counted only, and written: 8.6 GB on the device), a replacement table that is a slice of a larger
array, Longest and Shortest over a fold table, an empty dictionary and a dictionary of one keyword."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, _pack, utf16
from oracle.oracle import FAM_LONGEST, Oracle
from tests.helpers import splice
from tests.test_gpu_replace import check_both, on_device, pair
from tests.test_gpu_replace_batch import check as check_batch, oracle_records

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("replace_slab_units", 1 << 25)]
CANARY = 0x5A5A
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


# ---- the three entries on a raw replacement table (units, offsets, n_repl), a canary behind cap ----------------------------------
def raw_host(a, hay, table, cap):
    """-> (rc, n_out, the units written, stats)"""
    hay = utf16(hay)
    out = np.full(cap + 64, CANARY, np.uint16)
    n_out, st = ctypes.c_uint64(0), N.ReplaceStats()
    rc = N.lib().acgpu_replace_u16(a.handle, vp(hay if hay.size else np.zeros(1, np.uint16)), hay.size, vp(table[0]), vp(table[1]), table[2],
                                   vp(out), cap, ctypes.byref(n_out), ctypes.byref(st))
    assert (out[cap:] == CANARY).all(), "written at or beyond cap"
    return rc, n_out.value, out[:min(cap, n_out.value)], st


def raw_device(a, hay, table, cap):
    import torch
    hay = utf16(hay)
    d_hay = on_device(hay if hay.size else np.zeros(8, np.uint16))
    d_out = torch.full((cap + 64,), CANARY, dtype=torch.int16, device="cuda")
    sh = N.Shard()
    sh.d_hay, sh.n_units, sh.own_begin, sh.own_end = d_hay.data_ptr(), hay.size, 0, hay.size
    sh.text_begin = sh.text_end = 1
    sh.chain_entry, sh.chain_exit, sh.d_result = 0, -1, None
    n_out, st = ctypes.c_uint64(0), N.ReplaceStats()
    rc = N.lib().acgpu_replace_device(a.handle, ctypes.byref(sh), vp(table[0]), vp(table[1]), table[2], d_out.data_ptr(), cap,
                                      ctypes.byref(n_out), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(st))
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint16)
    assert (out[cap:] == CANARY).all(), "written at or beyond cap"
    return rc, n_out.value, out[:min(cap, n_out.value)], st


def raw_batch(a, units, offsets, table, cap):
    """-> (rc, n_out, the units written, stats, out_offsets)"""
    out = np.full(cap + 64, CANARY, np.uint16)
    oo = np.full(len(offsets), 99, np.uint64)
    n_out, st = ctypes.c_uint64(0), N.ReplaceStats()
    rc = N.lib().acgpu_replace_batch_u16(a.handle, vp(units), vp(offsets), len(offsets) - 1, vp(table[0]), vp(table[1]), table[2], vp(out), cap,
                                         vp(oo), ctypes.byref(n_out), ctypes.byref(st))
    assert (out[cap:] == CANARY).all(), "written at or beyond cap"
    return rc, n_out.value, out[:min(cap, n_out.value)], st, oo


# ---- 1. past 2^32 ---------------------------------------------------------------------------------------------------------------
N_A = (1 << 20) + 5                                  # matches of the keyword "a"
RAMP = (np.arange(4099) + 0x0100).astype(np.uint16)  # its replacement: 4099 ascending units
TAIL = "zqz"
TOTAL = 4099 * N_A + 3                               # units of the rewritten text
assert TOTAL > 1 << 32 and 4099 * (N_A - 3) > 1 << 32


def big_text():
    return np.concatenate([np.full(N_A, ord("a"), np.uint16), utf16(TAIL)])


def test_counted_not_written_past_2_32():
    """cap = 10000: the plan runs over every record, the emit over the first 10000 units only"""
    a = Automaton(N.MODE_LONGEST, ["a"], True)
    table = (RAMP, np.array([0, 4099], np.uint64), 1)
    cap = 10000
    head = np.tile(RAMP, 3)[:cap]
    rc, n_out, got, st = raw_host(a, big_text(), table, cap)
    assert rc == N.E_OVERFLOW and n_out == TOTAL and st.units_out == TOTAL and st.n_records == N_A, (rc, n_out, st.units_out)
    assert (got == head).all()
    # N_A haystacks "a": result i begins at 4099 * i, the last ones past 2^32
    units, offsets = np.full(N_A, ord("a"), np.uint16), np.arange(N_A + 1, dtype=np.uint64)
    rc, n_out, got, st, oo = raw_batch(a, units, offsets, table, cap)
    assert rc == N.E_OVERFLOW and n_out == 4099 * N_A and st.units_out == 4099 * N_A and st.n_records == N_A, (rc, n_out, st.units_out)
    assert oo.dtype == np.uint64 and (oo == np.uint64(4099) * np.arange(N_A + 1, dtype=np.uint64)).all() and int(oo[-1]) > 1 << 32
    assert (got == head).all()


def test_written_past_2_32():
    """the same text through acgpu_replace_device into 8.6 GB: every row, the tail and the canary checked on the device"""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 12 << 30:
        pytest.skip("less than 12 GiB of device memory free")
    a = Automaton(N.MODE_LONGEST, ["a"], True)
    d_hay = on_device(big_text())
    d_out = torch.full((TOTAL + 64,), CANARY, dtype=torch.int16, device="cuda")
    n_out, rc, st = a.replace_device(d_hay.data_ptr(), N_A + 3, [RAMP], d_out.data_ptr(), TOTAL, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == N.OK and n_out == TOTAL and st["units_out"] == TOTAL and st["n_records"] == N_A and st["pieces"] >= 2, (rc, n_out, st)
    ramp = on_device(RAMP)
    rows = d_out[:4099 * N_A].view(N_A, 4099)
    step = 1 << 15  # (rows per comparison: a quarter of a gigabyte at a time)
    for r0 in range(0, N_A, step):
        assert bool((rows[r0:r0 + step] == ramp).all()), r0
    assert d_out[4099 * N_A:TOTAL].cpu().numpy().view(np.uint16).tolist() == utf16(TAIL).tolist()
    assert bool((d_out[TOTAL:] == CANARY).all())


# ---- 2. a table that is a slice ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("single", [False, True])
def test_replacement_table_that_is_a_slice(single):
    """repl_off[0] == 37, other units in front of and behind the table's: the same result as with the table rebased to 0"""
    rng = np.random.default_rng(12)
    kws = ["ab", "abc", "c", "bcd", "dd", "abcdab", "ab"]
    a, orc = pair(N.MODE_LONGEST, kws)
    repls = "<*=*>" if single else ["<12345678>", "", "Q", "0123456789ABCDEFG", "xy", "#", "ab"]
    units, off, n_repl = a._replacements(repls)
    units = units[:int(off[-1])]
    rebased = (units, off, n_repl)
    sliced = (np.concatenate([np.full(37, 0xDEAD, np.uint16), units, np.full(50, 0xBEEF, np.uint16)]), off + np.uint64(37), n_repl)
    assert sliced[1][0] == 37 and n_repl == (1 if single else len(kws))
    hay = utf16("abcdz")[rng.integers(0, 5, 3001)]
    want = splice(hay, orc.match(hay, cap=hay.size), repls)
    assert 0xDEAD not in want and want.size > hay.size
    cap = int(want.size)
    for table in (rebased, sliced):
        for entry in (raw_host, raw_device):
            rc, n_out, got, st = entry(a, hay, table, cap)
            assert rc == N.OK and n_out == cap and (got == want).all(), entry.__name__
    hays = [hay[i:j] for i, j in zip(range(0, 3000, 30), range(30, 3001, 30))] + [hay[:0], hay[3000:]]
    b_want = [splice(h, r, repls) for h, r in zip(hays, oracle_records(orc, hays))]
    b_off = np.concatenate([[0], np.cumsum([w.size for w in b_want])]).astype(np.uint64)
    h_units, h_off = _pack(hays)
    for table in (rebased, sliced):
        rc, n_out, got, st, oo = raw_batch(a, h_units, h_off, table, int(b_off[-1]))
        assert rc == N.OK and n_out == b_off[-1] and oo.tolist() == b_off.tolist() and (got == np.concatenate(b_want)).all()


# ---- 3. Longest and Shortest over a fold table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [N.MODE_LONGEST, N.MODE_SHORTEST])
def test_case_insensitive_longest_and_shortest(mode):
    """U+0130 folds to i and U+212A to k (one unit each, as Character.toLowerCase folds them); U+FFFF is the table's last entry"""
    rng = np.random.default_rng(40 + mode)
    kws = ["Kelvin", "kiK", "IK", "nil", "\u212ae", "v\uffff", "liv\u0130", "EVIL", "kelvin"]
    table = utf16("kKiIeElLvVnN\u0130\u212a\uffff z")
    hay = table[rng.integers(0, len(table), 4001)]
    for at in range(50, 3900, 211):  # Kelvin in every mix of cases, the k and the i also as U+212A and U+0130
        word = utf16("".join(ch.upper() if rng.integers(2) else ch for ch in "kelvin"))
        if rng.integers(2):
            word[0] = 0x212A
        if rng.integers(2):
            word[4] = 0x0130
        hay[at:at + 6] = word
    a, orc = pair(mode, kws, cs=False)
    recs = orc.match(hay, cap=hay.size * 2)
    inside = np.zeros(hay.size, bool)
    for s, e, _ in recs.tolist():
        inside[s:e] = True
    for unit in (0x0130, 0x212A, 0xFFFF):  # in matches and outside of them
        assert (inside & (hay == unit)).sum() >= 5 and (~inside & (hay == unit)).sum() >= 5, hex(unit)
    assert (inside & (hay >= ord("A")) & (hay <= ord("Z"))).sum() >= 50 and len(recs) > 200
    repls = ["<%d\uffff>" % i if i % 3 else "" for i in range(len(kws))]
    want, _ = check_both(a, orc, hay, repls, recs)
    N.set_tunable("cursor_first_piece", 64)
    N.set_tunable("cursor_max_piece", 256)
    N.set_tunable("replace_slab_units", 1000)
    _, st = check_both(a, orc, hay, repls, recs, want)
    assert st["pieces"] > 10
    cuts = np.concatenate([[0], np.sort(rng.integers(0, hay.size, 149)), [hay.size]])
    hays = [hay[cuts[i]:cuts[i + 1]] for i in range(150)]
    _, _, st = check_batch(a, hays, oracle_records(orc, hays), repls)
    assert st["pieces"] > 10


# ---- 4. an empty dictionary, a dictionary of one keyword ---------------------------------------------------------------------------
TEXTS = ["", "a", "abzabzab", "zabzabzab"]  # 0, 1, 8 and 9 units


def test_empty_dictionary():
    """n_repl == 0 and no table entry; a batch call's table is the separators' empty slot alone"""
    a = Automaton(N.MODE_LONGEST, [], True)
    assert a.info()["n_keywords"] == 0
    orc = Oracle(FAM_LONGEST, [])
    for text in TEXTS:
        want, st = check_both(a, orc, text, [])
        assert (want == utf16(text)).all() and st["n_records"] == 0
    check_batch(a, TEXTS, oracle_records(orc, TEXTS), [])
    check_batch(a, [""], oracle_records(orc, [""]), [])


def test_dictionary_of_one_keyword():
    a, orc = pair(N.MODE_LONGEST, ["ab"])
    assert [len(t) for t in TEXTS] == [0, 1, 8, 9]
    for repl in ("<12345678>", ""):
        for text in TEXTS:
            _, st = check_both(a, orc, text, repl)  # n_repl == 1
            assert st["n_records"] == text.count("ab")
        check_batch(a, TEXTS, oracle_records(orc, TEXTS), repl)
