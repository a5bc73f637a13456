"""GPU test of case folding under caller-supplied fold tables (tests/fold_tables.py): all five families over tables that cross the
limits of the structures the builder derives from lower[] -- more fold pages than k_wwl_walk (24) or k_ww_pp / k_ww_tile<1> (64) keep
in LDS, byte pages that cannot be built, class tables with 200 distinct pages (no dfa_pages, cls_pages beyond the tile kernel's LDS),
folded range classes accepted and refused, merged stretches with partner bases, a sparse automaton, a table that is not idempotent and
a word table that is not fold-consistent.  Map records against the CPU oracle built with the same table, exact in shape and content,
and the form acgpu_profile::scan_kernel names.  The texts hold one copy of the whole plane and every preimage of the dictionary's
units; tests/test_fold_tables_cpu.py checks these inputs (coverage floors, sensitivity to one unit of the table) with the oracle alone."""
import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton
from oracle.oracle import FAM_AC, Oracle
from tests import fold_tables as F

pytestmark = pytest.mark.gpu


def _kernel_ok(spec, k):
    if spec is None:
        return True
    if callable(spec):
        return spec(k)
    return {"=": k == spec[1:], "^": k.startswith(spec[1:]), "!": not k.startswith(spec[1:])}[spec[0]]


@pytest.mark.parametrize("name", list(F.CASES))
def test_records_and_form_under_a_custom_fold_table(name):
    import torch
    fam, mode, table, kind, build, call, kernel = F.CASES[name]
    kws, hay, spans, T, word = F.case_inputs(name)
    want = F.case_records(name)
    try:
        for k, v in build.items():
            N.set_tunable(k, v)
        a = Automaton(mode, kws, False, word_chars=word, lower=T)
        for k, v in call.items():
            N.set_tunable(k, v)
        d_hay = torch.from_numpy(hay.view(np.int16).copy()).cuda()
        cap = len(want) + 16
        d_out = torch.full((cap, 3), -7, dtype=torch.int32, device="cuda")
        n_out, rc, prof, _ = a.match_device(d_hay.data_ptr(), hay.size, True, d_out.data_ptr(), cap,
                                            stream=torch.cuda.current_stream().cuda_stream, profile=True)
    finally:
        for k, v in F.KNOBS:
            N.set_tunable(k, v)
    print(name, prof["scan_kernel"], n_out)
    assert rc == N.OK, rc
    got = d_out[:n_out].cpu().numpy()
    assert got.shape == want.shape and (got == want).all(), (name, got.shape, want.shape, prof["scan_kernel"])
    assert _kernel_ok(kernel, prof["scan_kernel"]), (name, prof["scan_kernel"])


# the one-launch form of a short haystack (acgpu_match_u16 on up to 4096 units; csrc/acgpu_small.hip folds by T.lower itself): the
# beginning of a case's text, where the planted keywords start, under "wide"; WholeWordLongest has no such form and takes the general path
SHORT = {"all": "tile_sparse_wide", "longest": "longest_sparse_wide", "shortest": "shortest_sparse_wide", "wholeword": "ww_short_wide",
         "wwlongest": "wwl_wide"}


@pytest.mark.parametrize("family", list(SHORT))
def test_short_haystacks_under_a_custom_fold_table(family):
    fam, mode = F.CASES[SHORT[family]][:2]
    kws, hay, spans, T, word = F.case_inputs(SHORT[family])
    a = Automaton(mode, kws, False, word_chars=word, lower=T)
    orc = F.case_oracle(SHORT[family])
    for n in (4096, 4095, 777):
        want = orc.match(hay[:n])
        assert len(want) >= n // 40
        # the one launch orders at most 4096 occurrences and hands a text with more to the general path without a word: these
        # texts stay below it (Shortest and Longest select among the occurrences AhoCorasick reports), so the one launch answers
        if family in ("all", "longest", "shortest"):
            assert len(Oracle(FAM_AC, kws, case_sensitive=False, lower=T).match(hay[:n])) <= 4096
        assert len(want) <= 4096
        got = a.match_host(hay[:n], True)
        assert got.shape == want.shape and (got == want).all(), (family, n, got.shape, want.shape)


# Found by the soak under "rotate" (where e folds to U+0000) and independent of the table: the tile kernel's verification reads the
# K units in front of a candidate from a window that is zero in front of the buffer, and, where keywords shorter than K let the
# first K - 1 positions through, took a keyword that BEGINS with U+0000 for one that ends there -- {0, 0, b, b} over {0, b, b, ..}
# as the record (-1, 3).
@pytest.mark.parametrize("classes", ["packed", "bucketed"])
@pytest.mark.parametrize("table", [None, "java", "rotate"])
def test_keywords_that_begin_with_nul_do_not_match_in_front_of_the_text(classes, table):
    import torch
    cs = table is None
    T = None if cs else F.fold_table(table)[0]
    b, a_ = ord("b"), ord("a")
    extra = list(range(0x4E00, 0x4E00 + 300)) if classes == "bucketed" else []
    rng = np.random.default_rng(len(classes) + 3 * len(str(table)))
    lead = [[0, 0, b, b], [0, 0, 0, 0], [0, b, b, b, a_], [0, 0, 0, b, a_, b], [0, b, a_]]
    kws = [np.array(k, np.uint16) for k in lead + [[b], [a_, b], [0], [0, b], [b, b, a_]]]
    kws += [np.array(rng.choice([0, a_, b] + extra, int(rng.integers(1, 7))), dtype=np.uint16) for _ in range(40 if not extra else 400)]
    try:
        N.set_tunable("force_kernel", 2)
        N.set_tunable("all_form", 1)
        auto = Automaton(N.MODE_ALL, kws, cs, lower=T)
        orc = Oracle(FAM_AC, kws, case_sensitive=cs, lower=T)
        for k in lead + [[0, 0, 0, 0, 0, 0]]:
            for drop in range(1, len(k)):
                hay = np.concatenate([np.array(k[drop:], np.uint16), np.array(rng.choice([0, a_, b] + extra[:3], 3000), dtype=np.uint16)])
                want = orc.match(hay, cap=1 << 16)
                d_hay = torch.from_numpy(hay.view(np.int16).copy()).cuda()
                cap = len(want) + 16
                d_out = torch.full((cap, 3), -7, dtype=torch.int32, device="cuda")
                n_out, rc, prof, _ = auto.match_device(d_hay.data_ptr(), hay.size, True, d_out.data_ptr(), cap,
                                                       stream=torch.cuda.current_stream().cuda_stream, profile=True)
                got = d_out[:min(n_out, cap)].cpu().numpy()
                assert rc == N.OK and prof["scan_kernel"].startswith("k_ac_tile<"), (rc, prof["scan_kernel"])
                assert (got[:, 0] >= 0).all(), got[got[:, 0] < 0][:4]
                assert got.shape == want.shape and (got == want).all(), (classes, table, k, drop, got.shape, want.shape)
    finally:
        N.set_tunable("force_kernel", 0)
        N.set_tunable("all_form", 0)
