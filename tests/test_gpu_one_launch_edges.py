"""GPU tests of the one-launch form of acgpu_match_u16 (k_small<MODE>, csrc/acgpu_small.hip; the gate in match_host_text,
csrc/acgpu_hosttext.hip) at the edges of its lists, every record against the CPU oracle, bit for bit.  The inputs and the proof that each
reaches its edge are tests/small_edges.py (checked without a device by tests/test_one_launch_inputs_cpu.py):

  a. `m > kSmallMaxRecs` at 4095, 4096 and 4097 occurrences, ALL and SHORTEST; the counting sort with `recs` and `sorted` full;
     the rank loop with 90 occurrences in one end;
  b. `t.max_len > kSmallMaxLen` at 256 and 257; walks of 256 steps from unit 0, over the lane seams 1024, 2048, 3072, onto unit n;
  c. 20 000 keywords: the probe sequences of a hashed goto table of that size, ALL and LONGEST;
  d. the last round of the Longest pointer doubling (`span < n`) at n = 1, 2, 3, 1023 .. 1025, 4095, 4096; a last jump clamped to n;
  e. WholeWord runs that start at 0, 1023, 1024, 1025, end at 1024, 2048, 3072 and n (`wordf[min(pos, kSmallMaxUnits)]`), a keyword
     and one letter more, a keyword less its last letter, both case rules; what the gate refuses: a fold-inconsistent table,
     WholeWordLongest, 4097 units;
  f. U+0000 in keywords at the end of the text, units from 0x8000 on through edge_key, duplicates after folding;
  g. two automata in turn on one pinned block, a 5-unit text behind a 4096-unit one;
  and `c.cap = min(cap, kSmallMaxRecs)`, `*n_out > cap` and the memcpy of `*n_out` records at the C entry, with a canary.

WHO answered is certain: with tile_debug bit 2^44 (kSelOnlySmallCall) a call that k_small does not answer itself is
ACGPU_E_UNSUPPORTED instead of the general path's answer."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton
from tests import small_edges as E

pytestmark = pytest.mark.gpu

ONLY_ONE_LAUNCH, NO_ONE_LAUNCH = 1 << 44, 1 << 41  # tile_debug: kSelOnlySmallCall, kSelNoSmallCall
MODE = {"all": N.MODE_ALL, "longest": N.MODE_LONGEST, "wholeword": N.MODE_WHOLEWORD, "shortest": N.MODE_SHORTEST, "wwlongest": N.MODE_WWLONGEST}


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k in ("tile_debug", "force_kernel"):
        N.set_tunable(k, 0)


class Automata:
    """one automaton per dictionary and family"""

    def __init__(self):
        self.built = {}

    def of(self, c):
        key = (id(c.d), c.mode)
        if key not in self.built:
            a = Automaton(MODE[c.mode], c.d.kws, c.d.cs, word_chars=c.d.word, lower=c.d.lower)
            info = a.info()
            assert info["max_keyword_len"] == c.d.max_len()
            if c.why == "fold":
                assert info["fold_consistent"] == 0
            self.built[key] = a
        return self.built[key]


def same(got, want):
    return got.shape == want.shape and bool((got == want).all())


def check_three_ways(a, c):
    """Set and Map records: from k_small alone (or its refusal), from the call as it ships, from the general path"""
    for ids in (True, False):
        want = c.recs if ids else c.recs[:, :2]
        N.set_tunable("tile_debug", ONLY_ONE_LAUNCH)
        if c.one_launch:
            assert same(a.match_host(c.hay, ids), want), (c, ids, "k_small's own answer")
        else:
            with pytest.raises(N.AcgpuError) as err:
                a.match_host(c.hay, ids)
            assert err.value.code == N.E_UNSUPPORTED, (c, ids, c.why, "k_small answered a call that is not its own")
        N.set_tunable("tile_debug", 0)
        assert same(a.match_host(c.hay, ids), want), (c, ids, c.why or "the shipped call")
        N.set_tunable("tile_debug", NO_ONE_LAUNCH)
        assert same(a.match_host(c.hay, ids), want), (c, ids, "the general path")
        N.set_tunable("tile_debug", 0)


@pytest.mark.parametrize("group", [g for g in E.GROUPS if g != "g_alternating"])
def test_one_launch_answers_its_edges_and_refuses_the_rest(group):
    """Every case of the group, three calls per record kind: tile_debug 2^44 -- the oracle's records from k_small itself, or
    ACGPU_E_UNSUPPORTED where the case is not the one launch's (4097 occurrences, a keyword of 257 units, a fold-inconsistent word
    table, WholeWordLongest, 4097 units); 0 -- the oracle's records, through the hand-over where there is one; 2^41 -- the
    general path on the same short input."""
    automata = Automata()
    for c in E.GROUPS[group]():
        check_three_ways(automata.of(c), c)


def test_two_automata_in_turn_on_one_pinned_block():
    """An ALL automaton with 4096 records and a WholeWord automaton with one, on 4096 units and then on 5, three rounds, each call
    answered by k_small: the 5-unit texts lie in front of the stale units of the 4096-unit ones (the run "ab" ends on the text's
    last unit, the letters behind it are not the text's), their records in front of 4095 stale ones."""
    automata = Automata()
    cases = E.case_g()
    N.set_tunable("tile_debug", ONLY_ONE_LAUNCH)
    for rnd in range(3):
        for ids in (True, False):
            for c in cases:
                got = automata.of(c).match_host(c.hay, ids)
                assert same(got, c.recs if ids else c.recs[:, :2]), (rnd, c, ids)


def c_entry(a, hay, kind, cap, with_out=True):
    """acgpu_match_u16 itself into cap + 1 rows of -7 -> (rc, n_out, the rows)"""
    out = np.full((cap + 1, kind // 4), -7, dtype=np.int32)
    n_out = ctypes.c_uint64(0)
    rc = N.lib().acgpu_match_u16(a.handle, hay.ctypes.data_as(ctypes.c_void_p), hay.size, kind,
                                 out.ctypes.data_as(ctypes.c_void_p) if with_out else None, cap, ctypes.byref(n_out))
    return rc, int(n_out.value), out


@pytest.mark.parametrize("group", ["a_record_lists", "e_wholeword_cs", "e_wholeword_ci"])
def test_capacity_protocol_at_the_c_entry(group):
    """k_small's `n_out <= C.cap` with C.cap = min(cap, 4096), match_small's `*n_out > cap` and its memcpy of `*n_out` records,
    with tile_debug 2^44: a capacity below the count is ACGPU_E_OVERFLOW with the exact count; otherwise the oracle's records, and
    not one row behind them -- nor the row at `cap` -- is touched.  A capacity of 0 without a buffer is a counting call."""
    automata = Automata()
    N.set_tunable("tile_debug", ONLY_ONE_LAUNCH)
    for c in E.GROUPS[group]():
        if not c.one_launch:
            continue
        a, m = automata.of(c), len(c.recs)
        hay = np.array(c.hay, dtype=np.uint16)
        for kind in (N.REC_MAP, N.REC_SET):
            want = c.recs if kind == N.REC_MAP else c.recs[:, :2]
            for cap in sorted({0, max(m - 1, 0), m, m + 1, 5000}):
                rc, n_out, out = c_entry(a, hay, kind, cap)
                assert n_out == m, (c, kind, cap, n_out)
                assert (out[cap] == -7).all(), (c, kind, cap, "a row behind the capacity was written")
                if cap < m:
                    assert rc == N.E_OVERFLOW, (c, kind, cap, rc)
                else:
                    assert rc == N.OK and (out[:m] == want).all() and (out[m:] == -7).all(), (c, kind, cap, rc)
            rc, n_out, _ = c_entry(a, hay, kind, 0, with_out=False)
            assert (rc, n_out) == (N.E_OVERFLOW if m else N.OK, m), (c, kind, "counting call", rc, n_out)
