"""Keyword counts per haystack of a batch -- the document-term matrix, what CountVectorizer(vocabulary=...) computes -- from ONE
device call (include/acgpu.h: acgpu_count_batch_u16, acgpu_count_batch_utf8, acgpu_count_batch_utf8_lossy).

Both functions return (indptr int64[n + 1], indices int32[nnz], data uint32[nnz]): row i is indices[indptr[i]:indptr[i + 1]] --
the distinct keyword indices found in haystack i, ascending -- with their counts in data; numpy's unique(ids, return_counts=True)
of the records find_all_batch returns for that haystack.  The triple is what scipy.sparse.csr_matrix((data, indices, indptr),
shape=(n, number of keywords)) takes.  Indices index the constructor's keyword list; a duplicate keyword reports the index that
wins in a match call.

    indptr, indices, data = count_batch(AhoCorasickSet(vocabulary, False), lines)
    X = scipy.sparse.csr_matrix((data, indices, indptr), shape=(len(lines), len(vocabulary)))
"""
import ctypes

import numpy as np

from . import _native as N
from .strings import Automaton, _checked, _pack, _pack_utf8, _raise_for, _readable, _utf8_entry, _vp

__all__ = ["count_batch", "count_batch_utf8"]


def _automaton(matcher):
    """an Automaton, or the one behind a StringSet / StringMap"""
    return matcher if isinstance(matcher, Automaton) else matcher.automaton


def _csr_call(entry, head, n, units, stats, tail=()):
    """entry(*head, row_ptr, ids, counts, cap, &n_out, &stats, *tail) -> (indptr, indices, data).  The first capacity is a
    guess from the text's size; ACGPU_E_OVERFLOW wrote nothing and reports the entries the device produced, and the same call
    with exactly that capacity succeeds (include/acgpu.h, CAPACITY): ONE retry, a second overflow is an error."""
    st = stats if stats is not None else N.CountBatchStats()
    row_ptr = np.zeros(n + 1, dtype=np.uint64)
    cap = max(4096, units // 4)
    for attempt in range(2):
        ids, counts = np.empty(cap, dtype=np.uint32), np.empty(cap, dtype=np.uint32)
        n_out = ctypes.c_uint64(0)
        rc = entry(*head, _vp(row_ptr), _vp(ids), _vp(counts), cap, ctypes.byref(n_out), ctypes.byref(st), *tail)
        if rc != N.E_OVERFLOW:
            break
        cap = int(n_out.value)
    _raise_for(rc, entry, [t._obj for t in tail])
    nnz = int(n_out.value)
    return row_ptr.view(np.int64), ids[:nnz].view(np.int32), counts[:nnz]


def count_batch(matcher, haystacks, stats=None):
    """Keyword counts of many short haystacks (str or uint16 arrays) in one device call -> (indptr, indices, data), see the
    module's text.  matcher: an Automaton or any StringSet / StringMap, all five families.  stats: an N.CountBatchStats to fill
    in, if wanted."""
    units, off = _pack(_checked(haystacks))
    n = len(off) - 1
    return _csr_call(N.lib().acgpu_count_batch_u16, (_automaton(matcher).handle, _vp(units), _vp(off), n), n, int(off[-1]), stats)


def count_batch_utf8(matcher, datas, offsets=None, errors="strict", stats=None):
    """count_batch for UTF-8 haystacks: a sequence of bytes-like objects, or with offsets= ONE buffer used in place (a log file:
    offsets=utf8_line_offsets(buf)) -- the counts of count_batch on every haystack decoded alone.  An ill-formed haystack raises
    Utf8Error (.haystack, and .start inside it) -- unless errors="replace": every haystack as its .decode("utf-8", "replace")."""
    entry, stats_type = _utf8_entry("acgpu_count_batch_utf8", errors)
    if offsets is None:
        datas = _checked(datas)
    elif datas is None:
        raise TypeError("haystack is None")
    buf, off = _pack_utf8(datas, offsets)
    n = len(off) - 1
    return _csr_call(entry, (_automaton(matcher).handle, _vp(_readable(buf)), _vp(off), n), n, int(off[-1] - off[0]), stats,
                     tail=(ctypes.byref(stats_type()),))
