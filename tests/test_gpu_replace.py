"""GPU tests of the replace entries (include/acgpu.h: acgpu_replace_u16 / acgpu_replace_device; csrc/acgpu_replace.hip: the plan's
prefix sum and k_replace_emit).  Every expected text is the Python splice of the CPU oracle's records,
hay[e_{-1}:s_0] + repl[id_0] + hay[e_0:s_1] + ... + hay[e_{k-1}:n]; host and device entry in every case."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton, WholeWordMatchMap, WholeWordMatchSet, utf16
from ahocorasick_amd.unicode_tables import word_chars_from_list
from oracle.oracle import FAM_LONGEST, FAM_SHORTEST, FAM_WHOLEWORD, FAM_WWLONGEST, Oracle
from tests.helpers import LOWER, WORD, fixture_inputs, rand_case, splice

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20),
            ("replace_slab_units", 1 << 25)]
MODES = {N.MODE_LONGEST: FAM_LONGEST, N.MODE_WHOLEWORD: FAM_WHOLEWORD, N.MODE_SHORTEST: FAM_SHORTEST, N.MODE_WWLONGEST: FAM_WWLONGEST}
WORDY = (N.MODE_WHOLEWORD, N.MODE_WWLONGEST)


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def on_device(hay):
    import torch
    return torch.from_numpy(np.ascontiguousarray(hay).view(np.int16)).cuda()


def replace_device(a, hay, repls, cap=None, need=None):
    """acgpu_replace_device on the current torch stream, into a buffer with a canary behind cap -> (units, rc, n_out, stats)"""
    import torch
    hay = utf16(hay)
    d_hay = on_device(hay if hay.size else np.zeros(8, np.uint16))
    if cap is None:
        cap = need
    d_out = torch.full((cap + 64,), 0x5A5A, dtype=torch.int16, device="cuda")
    n_out, rc, st = a.replace_device(d_hay.data_ptr(), int(hay.size), repls, d_out.data_ptr(), cap,
                                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint16)
    assert (got[cap:] == 0x5A5A).all(), "written at or beyond cap"
    return got[:min(cap, n_out)], rc, n_out, st


def check_both(a, orc, hay, repls, recs=None, want=None):
    """host and device entry against the oracle splice -> (the text, the host entry's stats)"""
    hay = utf16(hay)
    if recs is None:
        recs = orc.match(hay, cap=max(1024, hay.size * 2))
    if want is None:
        want = splice(hay, recs, repls)
    got, st = a.replace_host(hay, repls)
    assert got.shape == want.shape and (got == want).all(), "host"
    assert st["n_records"] == len(recs) and st["units_out"] == want.size, st
    got, rc, n_out, st = replace_device(a, hay, repls, need=int(want.size))
    assert rc == N.OK and n_out == want.size and (got == want).all(), "device"
    assert st["n_records"] == len(recs) and st["units_out"] == want.size, st
    return want, st


def pair(mode, kws, cs=True, wc=None, map_flavour=False):
    if wc is None and mode in WORDY:
        wc = WORD
    return (Automaton(mode, kws, cs, word_chars=wc),
            Oracle(MODES[mode], kws, case_sensitive=cs, lower=None if cs else LOWER, word_chars=wc, map_flavour=map_flavour))


def four_sets(kws):
    kws = [utf16(k) if k is not None else np.zeros(0, np.uint16) for k in kws]
    return {"longer": [np.concatenate([k, utf16("<+>")]) for k in kws], "shorter": [k[:len(k) // 2] for k in kws],
            "empty": ["" for _ in kws], "same": [np.full(len(k), ord("#"), np.uint16) for k in kws]}


# ---- 1. fixtures ------------------------------------------------------------------------------------------------------------
FIXTURES = [("literal", N.MODE_LONGEST), ("literal", N.MODE_WHOLEWORD), ("overlap2", N.MODE_LONGEST), ("wwl4", N.MODE_WWLONGEST),
            ("shortest2", N.MODE_SHORTEST), ("readmeWholeWord", N.MODE_WHOLEWORD)]


@pytest.mark.parametrize("name,mode", FIXTURES)
def test_fixtures_with_four_replacement_sets(fixtures, name, mode):
    fx = [f for f in fixtures if f["name"] == name][0]
    hay, kws = fixture_inputs(fx)
    kws = fx.get({N.MODE_SHORTEST: "S_keywords", N.MODE_WWLONGEST: "WWL_keywords"}.get(mode, "keywords"), kws)
    a, orc = pair(mode, kws)
    recs = orc.match(hay)
    if name == "overlap2":
        assert [r[:2] for r in recs.tolist()[:2]] == [[1, 5], [5, 8]]  # the run of seven a's: two adjacent records
    for label, repls in four_sets(kws).items():
        check_both(a, orc, hay, repls, recs)


# ---- 2. edges ---------------------------------------------------------------------------------------------------------------
def test_edges():
    kws = ["ab", "abc", "c"]
    repls = ["<12345678>", "", "Q"]
    a, orc = pair(N.MODE_LONGEST, kws)
    base = "abzcabczzab"
    for n in (0, 1, 2, 7, 8, 9, len(base)):  # (length 2: the text is one match; 7: a match ends at n; all: one at unit 0)
        check_both(a, orc, base[:n], repls)
    check_both(a, orc, "abc", repls)          # one match, deleted: the empty text
    check_both(a, orc, "zabczabz", "*")       # n_repl == 1
    want, st = check_both(a, orc, "zzzz zzzz zzzz zzzz z", repls)  # no match
    assert st["n_records"] == 0 and (want == utf16("zzzz zzzz zzzz zzzz z")).all()


# ---- 3. every source alignment ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def align_case():
    rng = np.random.default_rng(31)
    kws, seen = [], set()
    while len(kws) < 18:
        k = "".join(rng.choice(list("ab"), int(rng.integers(2, 7))))
        if k not in seen:
            seen.add(k)
            kws.append(k)
    kws += ["bbbbbbbb", "dd"]
    repls = [("0123456789ABCDEFG" * 2)[i:i + i] for i in range(18)] + ["L" * 10000, ""]  # lengths 0 .. 17, one of 10 000, one deleted
    assert [len(r) for r in repls[:18]] == list(range(18))
    hay = np.array([ord(c) for c in "abcd"], np.uint16)[rng.choice(4, 200003, p=[0.3, 0.3, 0.3, 0.1])]
    for at in (5000, 77777, 150001):
        hay[at:at + 100] = ord("d")  # 50 deleted matches in a row
        hay[at - 1] = hay[at + 100] = ord("c")
    hay[100000:100008] = ord("b")
    hay[99999] = hay[100008] = ord("c")
    return kws, repls, hay


def test_every_source_alignment(align_case):
    kws, repls, hay = align_case
    a, orc = pair(N.MODE_LONGEST, kws)
    recs = orc.match(hay, cap=hay.size)
    ids = recs[:, 2]
    assert set(range(len(kws))) - set(ids.tolist()) <= {0}, "every replacement length is used"
    assert (ids == 18).sum() >= 1 and (ids == 19).sum() >= 150
    want, _ = check_both(a, orc, hay, repls, recs)
    assert want.size > hay.size // 2 + 10000


# ---- 4. density 1 -----------------------------------------------------------------------------------------------------------
def test_density_one():
    n = (1 << 20) + 3
    hay = np.full(n, ord("a"), np.uint16)
    hay[4098::4099] = ord("b")
    n_b = int((hay == ord("b")).sum())
    a, orc = pair(N.MODE_LONGEST, ["a"])
    recs = orc.match(hay, cap=n)
    assert len(recs) == n - n_b
    want, st = check_both(a, orc, hay, ["xyz"], recs)
    assert st["units_out"] == 3 * (n - n_b) + n_b
    want, st = check_both(a, orc, hay, [""], recs)
    assert want.size == n_b and (want == ord("b")).all()


# ---- 5. piece seams ---------------------------------------------------------------------------------------------------------
def _seam_case(mode):
    rng = np.random.default_rng(500 + mode)
    word = mode in WORDY
    kw_alpha = [ord(c) for c in "abAB"] if word else [ord(c) for c in "abc"]
    hay_alpha = kw_alpha + [32, 32, 32, 45] if word else kw_alpha + [ord("d")]
    _, kws = rand_case(rng, kw_alpha, 300 if word else 50, 4 if word else 9, 0)  # (dense enough to overflow 341 records per piece)
    kws += [kws[3].copy(), np.zeros(0, np.uint16)]
    hay = np.asarray(hay_alpha, np.uint16)[rng.integers(0, len(hay_alpha), 200003)]
    if mode == N.MODE_LONGEST:  # keywords of up to 40 units, in the text where pieces of 64 .. 4096 units end
        longs = [np.asarray(kw_alpha, np.uint16)[rng.integers(0, 3, ln)] for ln in (25, 33, 40, 40)]
        kws += longs
        for i, at in enumerate(range(40, 200003 - 50, 1009)):
            k = longs[i % 4]
            hay[at:at + k.size] = k
    if mode == N.MODE_WWLONGEST:
        kws += [np.concatenate([kws[i], np.array([32], np.uint16), kws[i + 1]]) for i in range(0, 20, 2)]
    hay[:1500] = ord("z")  # (the ramp reaches its largest piece before it knows a density)
    repls = [utf16("<" + "=" * (i % 6) + ">") if i % 3 else np.zeros(0, np.uint16) for i in range(len(kws))]
    return kws, hay, repls


@pytest.mark.parametrize("mode", sorted(MODES))
def test_piece_halo_and_slab_seams(mode):
    kws, hay, repls = _seam_case(mode)
    a, orc = pair(mode, kws)
    recs = orc.match(hay, cap=hay.size * 2)
    want, st = check_both(a, orc, hay, repls, recs)
    assert len(recs) > 0.1 * hay.size and st["pieces"] == 1
    for first in (64, 257):
        N.set_tunable("cursor_first_piece", first)
        N.set_tunable("cursor_max_piece", 4096)
        N.set_tunable("replace_slab_units", 1000)
        _, st = check_both(a, orc, hay, repls, recs, want)
        assert st["pieces"] > 10, st
    N.set_tunable("cursor_reservoir_bytes", 4096)  # 341 records
    a = Automaton(mode, kws, True, word_chars=WORD if mode in WORDY else None)  # (a pool whose reservoir has not grown yet)
    _, st = check_both(a, orc, hay, repls, recs, want)
    assert st["pieces"] > 10 and st["rescans"] > 0, st


# ---- 6. case folding --------------------------------------------------------------------------------------------------------
def test_case_folding_through_the_facade():
    rng = np.random.default_rng(6)
    words = ["straße", "naïve", "Zürich", "λόγος", "ΑΘΗΝΑ", "σοφία", "москва", "Привет", "мир", "data", "GPU"]
    values = ["[%d:%s]" % (i, w.upper()) for i, w in enumerate(words)]
    filler = ["und", "και", "или", "the", "x1"]

    def flip(w):
        return "".join(c.upper() if rng.integers(2) else c.lower() for c in w)
    toks = [flip(words[int(rng.integers(len(words)))]) if rng.integers(3) else filler[int(rng.integers(len(filler)))] for _ in range(4000)]
    # ('-' is a word character: a word with one on either side, 5 in 9 of them, is no whole word and stays as it is)
    text = "".join(t + (" ", ", ", "-")[int(rng.integers(3))] for t in toks)
    orc = Oracle(FAM_WHOLEWORD, words, case_sensitive=False, lower=LOWER, word_chars=WORD)
    recs = orc.match(text)
    assert len(recs) > 1000
    m = WholeWordMatchMap(words, values, False)
    want = splice(text, recs, values)
    assert utf16(m.replace(text)).tolist() == want.tolist()
    assert utf16(m.replace(text, "")).tolist() == splice(text, recs, "").tolist()
    assert utf16(WholeWordMatchSet(words, False).replace(text, "***")).tolist() == splice(text, recs, "***").tolist()
    with pytest.raises(TypeError):
        WholeWordMatchMap(words, list(range(len(words))), False).replace(text)


def test_word_table_that_is_not_fold_consistent():
    """the sequential whole-text kernel: one piece, whatever the tunables say"""
    rng = np.random.default_rng(9)
    alpha = np.array([ord(ch) for ch in "abxyABXY ,"], dtype=np.uint16)
    wc = word_chars_from_list("abcdxyABCD")  # X, Y are not word characters although x, y are
    hay = alpha[rng.integers(0, len(alpha), 20000)]
    kws = [alpha[rng.integers(0, 4, int(rng.integers(1, 5)))] for _ in range(12)]
    kws += [kws[2].copy()]
    a, orc = pair(N.MODE_WHOLEWORD, kws, cs=False, wc=wc, map_flavour=True)
    assert a.info()["fold_consistent"] == 0
    recs = orc.match(hay, cap=hay.size)
    assert len(recs) > 100
    N.set_tunable("cursor_first_piece", 64)
    N.set_tunable("replace_slab_units", 1000)
    _, st = check_both(a, orc, hay, ["<%d>" % i for i in range(len(kws))], recs)
    assert st["pieces"] == 1


# ---- 7. capacity protocol, 8. stats and the pool ----------------------------------------------------------------------------
def test_capacity_protocol_and_the_pool_afterwards(align_case):
    kws, repls, hay = align_case
    hay = hay[:50001]
    a, orc = pair(N.MODE_LONGEST, kws)
    recs = orc.match(hay, cap=hay.size)
    before = a.match_host(hay, with_ids=True)
    counts_before, _ = a.count_host(hay)
    assert (before == recs).all()
    want = splice(hay, recs, repls)
    need = int(want.size)
    N.set_tunable("cursor_first_piece", 4096)
    N.set_tunable("cursor_max_piece", 4096)
    N.set_tunable("replace_slab_units", 3000)
    units, off, n_repl = a._replacements(repls)
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    for cap, rc_want in ((0, N.E_OVERFLOW), (need - 1, N.E_OVERFLOW), (need // 3, N.E_OVERFLOW), (need, N.OK)):
        out = np.full(need + 64, 0x5A5A, np.uint16)
        n_out, st = ctypes.c_uint64(0), N.ReplaceStats()
        rc = N.lib().acgpu_replace_u16(a.handle, vp(hay), hay.size, vp(units), vp(off), n_repl, vp(out) if cap else None, cap,
                                       ctypes.byref(n_out), ctypes.byref(st))
        assert rc == rc_want and n_out.value == need and st.units_out == need and st.n_records == len(recs), (cap, rc)
        assert (out[cap:] == 0x5A5A).all(), cap
        if rc == N.OK:
            assert (out[:need] == want).all()
        got, rc, n_dev, dst = replace_device(a, hay, repls, cap=cap)  # (asserts its own canary behind cap)
        assert rc == rc_want and n_dev == need and dst["units_out"] == need and dst["n_records"] == len(recs), (cap, rc)
        if rc == N.OK:
            assert (got == want).all()
    got, st = a.replace_host(hay, repls, cap=16)  # the wrapper's one retry
    assert (got == want).all()
    for k, v in DEFAULTS:
        N.set_tunable(k, v)
    assert (a.match_host(hay, with_ids=True) == before).all()
    assert (a.count_host(hay)[0] == counts_before).all()
