"""CPU check of WholeWordLongest's first-word table (csrc/acgpu_build.cpp step 5b, what k_wwl_walk probes ONCE for a first word
of at most 12 units): the table acgpu_debug_wordhash exports against a plain Python trie of the folded, trimmed keywords.  The set
of word strings found in it is exactly the set of all-word paths of depth 12 or less that are a keyword or go on with a non-word
unit; bit 31 of the payload says which; the id is the last duplicate's; nothing deeper is in it.  Strings are looked up the way
the kernel does: the two hashes of tests/test_native_cpu.py::_simulate_wholeword, restated for one string."""
import ctypes

import numpy as np
import pytest

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import Automaton
from tests import wwl_edges as E
from tests.helpers import WORD
from tests.test_native_cpu import _wordhash_tables

DEFAULT_SEED = 0x811C9DC5


@pytest.fixture(autouse=True)
def _reset_tunables():
    yield
    N.set_tunable("ww_first_seed", 0)


def lookup(tables, units):
    """the payload of the folded word `units` in the two-choice table, None if neither of its two slots holds it"""
    slots, _, _, _, seed = tables
    mask = len(slots) - 1
    f = list(units)
    packed = [f[k] | ((f[k + 1] if k + 1 < len(f) else 0) << 16) for k in range(0, len(f), 2)]
    packed += [0] * (8 - len(packed))
    h = g = seed
    for d in packed:
        h = (h * 33 + d) & 0xffffffff
        g = (((g << 5) | (g >> 27)) & 0xffffffff) ^ d
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xffffffff
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xffffffff
    h ^= h >> 16
    tag = (h & 0xffffff00) | min(len(f), 255)
    s1 = h & mask
    s2 = ((((g ^ (h >> 16) ^ (g >> 13)) * 0x2C1B3C6D) & 0xffffffff) >> 11) & mask
    if s2 == s1:
        s2 ^= 1
    for s in (s1, s2):
        e = [int(x) for x in slots[s]]
        if e[0] == tag and e[2:8] == packed[:6]:
            return e[1]
    return None


def slot_words(tables):
    """{units: payload} of every used slot, decoded from the slot itself (tag: the length, units 0..11 inline)"""
    out = {}
    for e in tables[0].tolist():
        if e[0] == 0:
            continue
        ln = e[0] & 255
        assert 1 <= ln <= E.INLINE, ln  # nothing of 13 units or more, whose slot would hold a record offset
        units = tuple((e[2 + (k >> 1)] >> (16 * (k & 1))) & 0xffff for k in range(ln))
        assert all(e[2 + (k >> 1)] >> (16 * (k & 1)) & 0xffff == 0 for k in range(ln, 12)), e
        assert units not in out
        out[units] = e[1]
    return out


def node_depths(a):
    depth = np.zeros(a.info()["n_states"], np.uint32)
    N.check(N.lib().acgpu_debug_tables(a.handle, None, None, None, None, None, depth.ctypes.data_as(ctypes.c_void_p), None), "depth")
    return depth


def check_table(kws, cs, first_seed=0):
    N.set_tunable("ww_first_seed", first_seed)
    a = Automaton(N.MODE_WWLONGEST, kws, cs, word_chars=WORD)
    N.set_tunable("ww_first_seed", 0)
    tables = _wordhash_tables(a)
    assert (tables[4] == DEFAULT_SEED) == (first_seed == 0)
    trie = E.Trie(kws, cs)
    paths = trie.word_paths()
    expected = {p: v for p, v in paths.items() if len(p) <= E.INLINE and (v[1] or v[2])}
    assert len(expected) >= 10
    depth = node_depths(a)
    found, nodes = {}, set()
    for p, (node, is_kw, goes_on) in paths.items():
        payload = lookup(tables, p)
        if p not in expected:
            assert payload is None, p  # deeper than 12 units, or a path a walk cannot stand on when its first word ends
            continue
        assert payload is not None, p
        found[p] = payload
        assert (payload >> 31 == 1) == goes_on, (p, payload)
        if goes_on:  # the number of the trie node the walk goes on from: one per path, at the path's depth
            n = payload & 0x7fffffff
            assert n < len(depth) and depth[n] == len(p) and n not in nodes, (p, n)
            nodes.add(n)
        else:  # the id of the keyword -- among duplicates, the last one
            assert payload == trie.kw[node] and is_kw, (p, payload, trie.kw[node])
    assert slot_words(tables) == found  # and the table holds nothing else
    assert any(len(p) > E.INLINE and (v[1] or v[2]) for p, v in paths.items())  # there WERE deeper candidates to leave out
    return found, tables[4], trie


def duplicates_reach_the_payload(kws, cs, found, trie):
    """some keyword id in the table belongs to a keyword that was given more than once: the id is the last one's"""
    folded = [tuple(E.fold_units(E.trim(k, WORD), cs).tolist()) for k in kws]
    n = 0
    for p, payload in found.items():
        ids = [i for i, f in enumerate(folded) if f == p]
        if len(ids) > 1 and not payload >> 31:
            assert payload == ids[-1]
            n += 1
    return n


@pytest.mark.parametrize("cs", [True, False])
def test_first_word_table_of_the_edge_dictionary(cs):
    c = E.edge_case(cs)
    E.regime(c)  # the committed seeds reach every class of the GPU suite: asserted here on the CPU too
    found, seed, trie = check_table(c.kws, cs)
    assert {len(p) for p in found} >= {1, 2, 5, 11, 12}
    assert any(v >> 31 for v in found.values()) and any(not v >> 31 for v in found.values())
    # a first word that stands ONLY inside phrases: bit 31 without a keyword
    assert any(v[2] and not v[1] for p, v in trie.word_paths().items() if p in found)
    assert duplicates_reach_the_payload(c.kws, cs, found, trie) >= 1
    found5, seed5, _ = check_table(c.kws, cs, first_seed=5)
    assert seed5 != seed and found5 == found


@pytest.mark.parametrize("cs", [True, False])
def test_first_word_table_of_random_phrases(cs):
    rng = np.random.default_rng(4200 + cs)
    kws = []
    for _ in range(400):
        words = [E.ALPHA[rng.integers(0, len(E.ALPHA), int(rng.choice([1, 2, 3, 6, 11, 12, 13, 14, 20])))] for _ in range(int(rng.integers(1, 4)))]
        seps = [E.SP, E.COMMA_SP, E.cat([44])]
        k = words[0]
        for w in words[1:]:
            k = E.cat(k, seps[int(rng.integers(3))], w)
        if rng.integers(8) == 0:
            k = E.cat(E.SP, k, [46])  # trimmed by the builder
        kws.append(k)
    kws += [kws[int(i)].copy() for i in rng.integers(0, 400, 20)] + [E.cat([44, 32]), E.cat([32])]  # duplicates; no word character at all
    found, seed, trie = check_table(kws, cs)
    assert len(found) >= 100
    duplicates_reach_the_payload(kws, cs, found, trie)
    found5, seed5, _ = check_table(kws, cs, first_seed=5)
    assert seed5 != seed and found5 == found
