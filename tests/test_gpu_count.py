"""GPU tests of the counting entries (include/acgpu.h: acgpu_count_u16 / acgpu_count_device; csrc/acgpu_count.hip, k_states_hist /
k_states_spread / k_count_ids in csrc/acgpu_states.hip): per-keyword counts without records.  Expected values come from the CPU
oracle -- bincount of the keyword_id column of its records -- for the direct form (states -> visits -> counts) at every seam of
its passes, for the records form of every family, and for the mix of both a default call makes on a word list."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd import synth
from ahocorasick_amd.strings import AhoCorasickMap, Automaton, LongestMatchSet, utf16
from ahocorasick_amd.unicode_tables import word_chars_from_list
from oracle.oracle import FAM_AC, FAM_LONGEST, FAM_SHORTEST, FAM_WHOLEWORD, FAM_WWLONGEST, Oracle
from tests.helpers import LOWER, WORD, rand_case

pytestmark = pytest.mark.gpu

DEFAULTS = [("cursor_first_piece", 1 << 20), ("cursor_max_piece", 1 << 26), ("cursor_reservoir_bytes", 256 << 20), ("all_form", 0),
            ("tile_debug", 0), ("states_chunk_log2", 0), ("count_form", 0)]
MODES = {N.MODE_ALL: FAM_AC, N.MODE_LONGEST: FAM_LONGEST, N.MODE_WHOLEWORD: FAM_WHOLEWORD, N.MODE_SHORTEST: FAM_SHORTEST,
         N.MODE_WWLONGEST: FAM_WWLONGEST}
STATES_ALWAYS = 6  # all_form: the states form whatever the pool's last call found, for short texts too
SEAM_SIZES = (1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, 32769, 200003)


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    for k, v in DEFAULTS:
        N.set_tunable(k, v)


def expected(orc, hay, n_kw):
    return np.bincount(orc.match(hay, cap=max(1024, hay.size * 2))[:, 2], minlength=n_kw).astype(np.uint64)


def on_device(hay):
    import torch
    return torch.from_numpy(np.ascontiguousarray(hay).view(np.int16)).cuda()


def count_device(a, d_hay, n, d_counts=None, **kw):
    """acgpu_count_device on the current torch stream -> (counts as numpy, stats, chain_exit, the device array)"""
    import torch
    if d_counts is None:
        d_counts = torch.zeros(max(len(a.keywords), 1), dtype=torch.int64, device="cuda")
    rc, st, chain_exit = a.count_device(d_hay.data_ptr(), n, d_counts.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, **kw)
    assert rc == N.OK, rc
    return d_counts.cpu().numpy().astype(np.uint64)[:len(a.keywords)], st, chain_exit, d_counts


@pytest.fixture(scope="module")
def words():
    return synth.readme_dictionary(n=30000)


@pytest.fixture(scope="module")
def seam_case(words):
    """the word list's automaton and oracle, a text of the largest seam size, the oracle's records of it (computed once)"""
    text = synth.readme_text(4, SEAM_SIZES[-1], words)
    orc = Oracle(FAM_AC, words)
    recs = orc.match(text, cap=text.size * 2)
    return Automaton(N.MODE_ALL, words, True), text, recs


@pytest.mark.parametrize("chunk_log2", [0, 9, 10])
def test_direct_form_at_every_seam_of_its_passes(seam_case, words, chunk_log2):
    """k_ac_states + k_states_hist + k_states_spread on 1 .. 200003 units, with a lane's chunk left to the text's length (256 units
    at these sizes: one step per chunk) and forced to 512 and 1024 (2 and 4 steps), host and device entry: no record is written."""
    a, text, recs = seam_case
    N.set_tunable("all_form", STATES_ALWAYS)
    N.set_tunable("states_chunk_log2", chunk_log2)
    d_text = on_device(text)
    for n in SEAM_SIZES:
        # (AhoCorasick: the records of a prefix are the records that end inside it)
        want = np.bincount(recs[recs[:, 1] <= n][:, 2], minlength=len(words)).astype(np.uint64)
        got, st = a.count_host(text[:n])
        assert (got == want).all(), (n, "host")
        assert st["units_records"] == 0 and st["units_direct"] == n and st["n_records"] == int(want.sum()), (n, st)
        got, st, _, _ = count_device(a, d_text[:n], n)
        assert (got == want).all(), (n, "device")
        assert st["units_records"] == 0 and st["units_direct"] == n and st["n_records"] == int(want.sum()), (n, st)


def test_direct_form_over_owned_ranges_accumulates(seam_case, words):
    """Three shards of one buffer, the ALL left halo in place, own_begin no multiple of 4: one d_counts takes them all."""
    a, text, recs = seam_case
    n = 70001
    N.set_tunable("all_form", STATES_ALWAYS)
    want = np.bincount(recs[recs[:, 1] <= n][:, 2], minlength=len(words)).astype(np.uint64)
    d_text = on_device(text[:n])
    halo = a.info()["max_keyword_len"] - 1
    cuts = [0, 4099, 33334, n]
    assert all(c % 4 for c in cuts[1:3])
    d_counts = None
    for rounds in (1, 2):
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            b0 = max(0, lo - halo)  # the shard's buffer: its left halo and its owned units (16-byte aligned start)
            b0 -= b0 % 8
            got, st, _, d_counts = count_device(a, d_text[b0:], hi - b0, d_counts, own=(lo - b0, hi - b0), text_begin=b0 == 0, text_end=hi == n)
            assert st["units_direct"] == hi - lo and st["units_records"] == 0
        assert (got == want * rounds).all(), rounds


def test_direct_form_id_lists_hot_state_and_duplicates():
    """a, aa, ..., a x 32 (+ b, ab, a duplicate of aa, an empty keyword) in a text of a's: one hot state that lists 32 ids, states
    with one id inline, the last duplicate's slot counts and the first one's stays 0."""
    kws = ["a" * k for k in range(1, 33)] + ["b", "ab", "aa", ""]
    n = 1 << 20
    hay = np.full(n, ord("a"), np.uint16)
    hay[4098::4099] = ord("b")
    want = expected(Oracle(FAM_AC, kws), hay, len(kws))
    assert want[1] == 0 and want[34] > 0 and want[35] == 0 and want[33] == n // 4099
    a = Automaton(N.MODE_ALL, kws, True)
    N.set_tunable("all_form", STATES_ALWAYS)
    for form in (0, 2, 4):  # (count_form: with and without the LDS counters and the same-key peel -- the same counts)
        N.set_tunable("count_form", form)
        got, st = a.count_host(hay)
        assert (got == want).all(), form
        assert st["units_direct"] == n and st["units_records"] == 0 and st["n_records"] == int(want.sum())


def _family_case(mode, cs, seed, n, wc=WORD):
    rng = np.random.default_rng(seed)
    word = mode in (N.MODE_WHOLEWORD, N.MODE_WWLONGEST)
    kw_alpha = [ord(c) for c in "abAB"] if word else [ord(c) for c in "abcA"]
    hay_alpha = kw_alpha + [32, 32, 45] if word else kw_alpha
    _, kws = rand_case(rng, kw_alpha, 60, 7 if word else 12, 0)
    kws += [kws[3].copy(), kws[10].copy(), np.zeros(0, np.uint16)]  # duplicates and an empty keyword
    if mode == N.MODE_WWLONGEST:
        kws += [np.concatenate([kws[i], np.array([32], np.uint16), kws[i + 1]]) for i in range(0, 20, 2)]
    hay = np.asarray(hay_alpha, np.uint16)[rng.integers(0, len(hay_alpha), n)]
    # a beginning without any match: the ramp reaches its largest piece before it knows a density, so the first piece of the dense
    # part does not fit the reservoir and is scanned again, smaller
    hay[:1500] = ord("z")
    return kws, hay


def _small_pieces():
    N.set_tunable("cursor_first_piece", 64)
    N.set_tunable("cursor_max_piece", 4096)
    N.set_tunable("cursor_reservoir_bytes", 6000)  # 500 Map records


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("cs", [True, False])
def test_records_form_of_every_family(mode, cs):
    """Pieces of 64 .. 4096 units through a reservoir of 500 records: many pieces, the chains handed on, pieces scanned again."""
    kws, hay = _family_case(mode, cs, 300 + mode * 2 + cs, 20000)
    wc = WORD if mode in (N.MODE_WHOLEWORD, N.MODE_WWLONGEST) else None
    a = Automaton(mode, kws, cs, word_chars=wc)
    want = expected(Oracle(MODES[mode], kws, case_sensitive=cs, lower=None if cs else LOWER, word_chars=wc), hay, len(kws))
    ref = np.bincount(a.match_host(hay, with_ids=True)[:, 2], minlength=len(kws)).astype(np.uint64)
    assert want.sum() > 500 and (ref == want).all()
    _small_pieces()
    got, st = a.count_host(hay)
    assert (got == want).all()
    assert st["units_direct"] == 0 and st["units_records"] == hay.size and st["n_records"] == int(want.sum())
    if mode == N.MODE_ALL:
        assert st["pieces"] > 4 and st["rescans"] >= 1, st
    got, st, _, _ = count_device(a, on_device(hay), hay.size)
    assert (got == want).all() and st["n_records"] == int(want.sum())


@pytest.mark.parametrize("mode", [N.MODE_WHOLEWORD, N.MODE_WWLONGEST])
def test_records_form_of_the_word_matchers_over_a_table_that_is_not_fold_consistent(mode):
    rng = np.random.default_rng(9)
    alpha = np.array([ord(ch) for ch in "abxyABXY ,"], dtype=np.uint16)
    wc = word_chars_from_list("abcdxyABCD")  # X, Y are not word characters although x, y are
    hay = alpha[rng.integers(0, len(alpha), 20000)]
    kws = [alpha[rng.integers(0, 4, int(rng.integers(1, 5)))] for _ in range(12)]
    kws += [kws[2].copy()]
    if mode == N.MODE_WWLONGEST:
        kws += [np.concatenate([kws[0], [32], kws[1]]).astype(np.uint16)]
    a = Automaton(mode, kws, False, word_chars=wc)
    assert a.info()["fold_consistent"] == 0
    # (the Map class's loop: what the Map records of a match call restate)
    want = expected(Oracle(MODES[mode], kws, case_sensitive=False, lower=LOWER, word_chars=wc, map_flavour=True), hay, len(kws))
    ref = np.bincount(a.match_host(hay, with_ids=True)[:, 2], minlength=len(kws)).astype(np.uint64)
    assert want.sum() > 100 and (ref == want).all()
    _small_pieces()
    got, st = a.count_host(hay)
    assert (got == want).all() and st["n_records"] == int(want.sum()) and st["units_direct"] == 0
    got, st, _, _ = count_device(a, on_device(hay), hay.size)
    assert (got == want).all()


def test_records_form_with_one_hot_id():
    n = 1 << 20
    hay = np.full(n, ord("a"), np.uint16)
    a = Automaton(N.MODE_ALL, ["a"], True)
    N.set_tunable("all_form", 1)
    for form in (0, 4):
        N.set_tunable("count_form", form)
        got, st = a.count_host(hay)
        assert got.tolist() == [n] and st["units_direct"] == 0 and st["units_records"] == n


def test_default_call_on_a_word_list_mixes_both_forms(words):
    """A fresh automaton, default tunables: the first piece goes through records and teaches the pool its density, the next is
    counted directly, the short tail through records again."""
    n = 5 * (1 << 20) + 77
    hay = synth.readme_text(12, n, words)
    want = expected(Oracle(FAM_AC, words), hay, len(words))
    a = Automaton(N.MODE_ALL, words, True)
    got, st = a.count_host(hay)
    assert (got == want).all()
    assert st["units_records"] > 0 and st["units_direct"] > 0 and st["units_direct"] + st["units_records"] == n, st
    assert st["n_records"] == int(want.sum())


def test_fall_backs_of_the_direct_form(seam_case, words):
    a, text, recs = seam_case
    n = 70001
    want = np.bincount(recs[recs[:, 1] <= n][:, 2], minlength=len(words)).astype(np.uint64)
    N.set_tunable("all_form", STATES_ALWAYS)
    N.set_tunable("tile_debug", 1 << 40)  # no room for the state words
    got, st = a.count_host(text[:n])
    assert (got == want).all() and st["units_direct"] == 0 and st["units_records"] == n
    N.set_tunable("tile_debug", 0)
    N.set_tunable("count_form", 1)  # never direct
    got, st = a.count_host(text[:n])
    assert (got == want).all() and st["units_direct"] == 0
    N.set_tunable("count_form", 0)
    # a keyword of more than 32 units: no compact automaton
    kws = list(words[:2000]) + [np.concatenate(sorted(words[:2000], key=len)[-6:])]
    assert len(kws[-1]) > 32
    hay = np.concatenate([text[:30000], kws[-1], text[30000:60000]])
    want = expected(Oracle(FAM_AC, kws), hay, len(kws))
    assert want[-1] >= 1
    got, st = Automaton(N.MODE_ALL, kws, True).count_host(hay)
    assert (got == want).all() and st["units_direct"] == 0


def test_stream_rule():
    import torch
    kws = ["ab", "b"]
    hay = synth.haystack(3, 1 << 16, table=np.array([97, 98, 99], np.uint16))
    want = expected(Oracle(FAM_AC, kws), hay, 2)
    a = Automaton(N.MODE_ALL, kws, True)
    d_hay = on_device(hay)
    cap = int(want.sum()) + 8
    out = torch.empty((cap, 3), dtype=torch.int32, device="cuda")
    d_counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    tk, rc = a.match_device_begin(d_hay.data_ptr(), hay.size, True, out.data_ptr(), cap, stream=s1.cuda_stream)
    assert rc == N.OK
    rc, _, _ = a.count_device(d_hay.data_ptr(), hay.size, d_counts.data_ptr(), stream=s2.cuda_stream)
    assert rc == N.E_INVALID
    m, rc, _ = a.match_device_end(tk)
    assert rc == N.OK and m == int(want.sum())
    torch.cuda.synchronize()
    assert d_counts.cpu().tolist() == [0, 0]
    rc, _, _ = a.count_device(d_hay.data_ptr(), hay.size, d_counts.data_ptr(), stream=s2.cuda_stream)
    assert rc == N.OK and d_counts.cpu().numpy().astype(np.uint64).tolist() == want.tolist()


def test_facade_count_equals_a_counting_listener():
    text = "she sells sea shells by the sea shore; he sees her shells"
    kws = ["he", "she", "sea", "shells", "s", "he", "hers"]
    for cls, args in ((AhoCorasickMap, (kws, list(range(len(kws))), True)), (LongestMatchSet, (kws, True))):
        m = cls(*args)
        held = np.zeros(len(kws), np.uint64)
        if cls is AhoCorasickMap:
            def listener(h, s, e, v):
                held[v] += 1
                return True
        else:
            def listener(h, s, e):
                held[len(kws) - 1 - kws[::-1].index(h[s:e])] += 1  # (the last keyword equal to the match)
                return True
        m.match(text, listener)
        got = m.count(text)
        assert held.sum() > 5 and got.dtype == np.uint64 and (got == held).all()
