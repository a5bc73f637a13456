"""GPU test of the kernel forms the host chooses (csrc/acgpu_forms.h: choose_tile_form, choose_ww_form, choose_dfa_form): one
dictionary per reachable family, one text of 2^16 + 777 units with keywords planted across a lane, a tile and a region boundary,
Map records against the CPU oracle, and the exact name acgpu_profile::scan_kernel reports.  The names are literals: they were
taken from a run of this test's body at the commit before the forms moved into one table, and must not change with the host
code that picks and launches the kernels.  (The large second level, BIG, stays with the 70 k-keyword test of
tests/test_gpu_parity.py.)"""
import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd import synth
from ahocorasick_amd.strings import Automaton
from oracle.oracle import FAM_AC, FAM_WHOLEWORD, Oracle
from tests.helpers import LOWER, WORD

pytestmark = pytest.mark.gpu

N_UNITS = (1 << 16) + 777
KNOBS = [("force_kernel", 0), ("tile_debug", 0), ("all_form", 0), ("no_merged_ranges", 0)]
# a lane (16 or 32 units per lane), a tile (1024; the second-level forms: 2048), a region (16384 here) and the seam at 2^16
BOUNDARIES = [160, 1024, 2048, 3 * 2048, 16384, 32768, 65536]
SPACE = ord(" ")


def _u(s):
    return np.array([ord(c) for c in s], dtype=np.uint16)


def _words(rng, alpha, n, lo, hi):
    alpha = np.asarray(alpha, dtype=np.uint16)
    return list({k.tobytes(): k for k in (alpha[rng.integers(0, len(alpha), int(rng.integers(lo, hi + 1)))] for _ in range(n))}.values())


def _lower(rng):
    return synth.random_keywords(synth.CONFIGS["C2"]["dict_seed"], 300, 4, 12), synth.ALPHA_LOWER


def _lower_short(rng):
    kws, alpha = _lower(rng)
    return kws + [_u("q")], alpha


def _class_table(rng):  # 50 units over 300 code points: more stretches than the range arithmetic merges, fewer than 64 classes
    alpha = list(range(0x4E00, 0x4E00 + 300, 6))
    return _words(rng, alpha, 300, 4, 9), alpha


def _bucketed(rng):  # 300 distinct units: bucketed classes
    alpha = list(range(0x4E00, 0x4E00 + 300))
    return _words(rng, alpha, 2000, 3, 8), alpha


def _merged2(rng):  # mixed case, case-sensitive: two stretches
    alpha = [ord(c) for c in "bcdefghijklmBCDEFGHIJKLM"]
    return _words(rng, alpha, 300, 4, 11), alpha


def _merged4(rng):  # mixed case with spaces and digits: four stretches
    alpha = [ord(c) for c in "abcdefghABCDEFGH 0129-"]
    return [k for k in _words(rng, alpha, 300, 4, 11) if k[0] != SPACE and k[-1] != SPACE], alpha


def _ww_short(rng):
    return _words(rng, _u("abcdefgh"), 300, 1, 16), _u("abcdefgh")


def _ww_long(rng):  # a keyword of more than 32 units: k_ww_tile
    kws, alpha = _ww_short(rng)
    return kws + [alpha[rng.integers(0, len(alpha), 40)]], alpha


# family -> (dictionary, mode, case-sensitive, tunables of the call, the kernel)
CASES = {
    "packed_l2": (_lower, N.MODE_ALL, True, {"force_kernel": 2}, "k_ac_tile<4, true, false, false, false, true, true>"),
    "packed_l2_short": (_lower_short, N.MODE_ALL, True, {"force_kernel": 2}, "k_ac_tile<4, true, false, false, false, true, true>"),
    "packed": (_lower, N.MODE_ALL, True, {"force_kernel": 2, "tile_debug": 2048}, "k_ac_tile<4, true, false, false, false, true>"),
    "generic_range": (_lower, N.MODE_ALL, True, {"force_kernel": 2, "tile_debug": 1024}, "k_ac_tile<4, true, false, false>"),
    "class_table": (_class_table, N.MODE_ALL, True, {"force_kernel": 2}, "k_ac_tile<3, false, true, false>"),
    "bucketed": (_bucketed, N.MODE_ALL, True, {"force_kernel": 2}, "k_ac_tile<3, false, true, false, true>"),
    "merged_2": (_merged2, N.MODE_ALL, True, {"force_kernel": 2}, "k_ac_tile<4, false, false, false, true, true, true, false>"),
    "merged_4": (_merged4, N.MODE_ALL, True, {"force_kernel": 2}, "k_ac_tile<4, false, false, false, true, true, true, true>"),
    "split": (_lower, N.MODE_ALL, True, {"force_kernel": 3}, "k_ac_tile<4, true, false, true>"),
    "ww_pp": (_ww_short, N.MODE_WHOLEWORD, False, {}, "k_ww_pp<3, false, true>"),
    "ww_tile": (_ww_long, N.MODE_WHOLEWORD, False, {}, "k_ww_tile<1>"),
    "dfa": (_lower, N.MODE_ALL, True, {"force_kernel": 1}, "k_ac_dfa<unsigned short, true, false>"),
}


def _text(rng, kws, alpha, ww):
    """random text over the dictionary's alphabet and a few other units, a keyword across every boundary (WholeWord: between
    spaces) and ending at the text's last unit"""
    pool = np.concatenate([np.asarray(alpha, dtype=np.uint16), np.array([SPACE, ord("!"), 0x00E9, 0xFFFF], dtype=np.uint16)])
    hay = pool[rng.integers(0, len(pool), N_UNITS)].copy()
    spans = []
    for i, b in enumerate(BOUNDARIES + [N_UNITS]):
        k = kws[(7 * i) % len(kws)]
        s = b - k.size if b == N_UNITS else b - (k.size + 1) // 2
        if k.size == 1:
            s = b - 1
        hay[s:s + k.size] = k
        if ww:
            hay[s - 1] = SPACE
            if s + k.size < N_UNITS:
                hay[s + k.size] = SPACE
        spans.append((s, s + k.size))
    return hay, spans


@pytest.mark.parametrize("family", list(CASES))
def test_the_form_each_family_takes_and_its_records(family):
    import torch
    make, mode, cs, knobs, kernel = CASES[family]
    rng = np.random.default_rng(len(family) * 131 + 7)
    kws, alpha = make(rng)
    ww = mode == N.MODE_WHOLEWORD
    hay, spans = _text(rng, kws, alpha, ww)
    if ww:
        orc = Oracle(FAM_WHOLEWORD, kws, case_sensitive=cs, lower=LOWER, word_chars=WORD)
    else:
        orc = Oracle(FAM_AC, kws, case_sensitive=cs, lower=None if cs else LOWER)
    want = orc.match(hay, cap=1 << 20)
    have = set(map(tuple, want[:, :2].tolist()))
    assert all(sp in have for sp in spans), family
    try:
        N.set_tunable("all_form", 1)
        for k, v in knobs.items():
            N.set_tunable(k, v)
        a = Automaton(mode, kws, cs, word_chars=WORD, lower=None if cs else LOWER) if ww else Automaton(mode, kws, cs)
        d_hay = torch.from_numpy(hay.view(np.int16)).cuda()
        cap = len(want) + 16
        d_out = torch.full((cap, 3), -7, dtype=torch.int32, device="cuda")
        n_out, rc, prof, _ = a.match_device(d_hay.data_ptr(), hay.size, True, d_out.data_ptr(), cap,
                                            stream=torch.cuda.current_stream().cuda_stream, profile=True)
    finally:
        for k, v in KNOBS:
            N.set_tunable(k, v)
    assert rc == N.OK, rc
    got = d_out[:n_out].cpu().numpy()
    assert got.shape == want.shape and (got == want).all(), (family, got.shape, want.shape)
    assert prof["scan_kernel"] == kernel, (family, prof["scan_kernel"])
