"""GPU test of what the batch entries leave behind on their scratch pool (csrc/acgpu_batch.hip: BatchText holds
DeviceState::start_behind, the separator unit, for the duration of a batch scan): batch calls that end early -- no room for a
single record, no room for a single output unit -- and one that completes are followed by a plain acgpu_match_u16 call on a text
that holds the separator unit between word characters.  Its records must be the CPU oracle's: a separator left behind would make
WholeWordLongest start a walk behind every U+FFFF of that text."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, _pack, utf16
from oracle.oracle import FAM_WHOLEWORD, FAM_WWLONGEST, Oracle
from tests.helpers import WORD

pytestmark = pytest.mark.gpu

vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
FAMILIES = {N.MODE_WWLONGEST: FAM_WWLONGEST, N.MODE_WHOLEWORD: FAM_WHOLEWORD}
# " " and ", " have no word character: WholeWordLongest keeps them as they are (WholeWord refuses such keywords)
KEYWORDS = {N.MODE_WWLONGEST: ["ab", "ab cd", " ", "c", ", ", "cd"], N.MODE_WHOLEWORD: ["ab", "abc", "c", "cd"]}
BATCH = ["ab cd, c", "zz ab", "c ab cd ab, c"]  # three haystacks of under 32 units, each with matches
# 64 units; U+FFFF between word characters, and in front of the keywords that begin with a non-word unit
TEXT = "ab\uffffcd ab\uffffab cd\uffff, c\uffff c ab\uffffc\uffff\uffffab cd, zz\uffffzz ab cd\uffffcd,\uffffab c ab cd ab"


@pytest.mark.parametrize("mode", sorted(FAMILIES))
def test_batch_calls_that_end_early_leave_the_pool_as_they_found_it(mode):
    kws = KEYWORDS[mode]
    a = Automaton(mode, kws, True, word_chars=WORD)  # case sensitive over the default table: fold-consistent
    orc = Oracle(FAMILIES[mode], kws, True, None, WORD, map_flavour=True)
    assert a.info()["fold_consistent"] == 1
    assert len(BATCH) == 3 and all(len(h) < 32 for h in BATCH) and len(TEXT) == 64
    want = orc.match(TEXT, cap=8 * len(TEXT))
    assert len(want) >= 8 and all(len(orc.match(h, cap=64)) for h in BATCH)
    lib, h = N.lib(), a.handle
    units, off = _pack(BATCH)
    n_out = ctypes.c_uint64(0)
    # 1. batch match without room for a record
    rc = lib.acgpu_match_batch_u16(h, vp(units), vp(off), len(BATCH), N.REC_MAP, None, 0, ctypes.byref(n_out))
    assert rc == N.E_OVERFLOW and n_out.value > 0
    # 2. batch replace without room for a unit
    r_units, r_off = _pack(["#"])
    out_off = np.zeros(len(off), dtype=np.uint64)
    st = N.ReplaceStats()
    rc = lib.acgpu_replace_batch_u16(h, vp(units), vp(off), len(BATCH), vp(r_units), vp(r_off), 1, None, 0, vp(out_off), ctypes.byref(n_out),
                                     ctypes.byref(st))
    assert rc == N.E_OVERFLOW and n_out.value > 0
    # 3. batch summary
    got, _ = a.summary_batch(BATCH)
    assert [int(x) for x in got["n_matches"]] == [len(orc.match(x, cap=64)) for x in BATCH]
    # 4. one plain call on the text with separators in it
    recs = a.match_host(utf16(TEXT), True)
    assert recs.tolist() == want.tolist()
