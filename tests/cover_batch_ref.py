"""The reference of the batch spans and batch cover tests (include/acgpu.h: acgpu_spans_batch_u16, acgpu_cover_batch_u16):
tests/spans_ref.merge and tests/cover_ref.cover_ref over the oracle's records, haystack by haystack, and the layout of the result
that the tests about tiles, slabs and segments reason with.  A helper, not collected."""
import ctypes
import importlib

import numpy as np

from ahocorasick_amd import _native as N
from ahocorasick_amd.strings import _pack, utf16
from tests.cover_ref import cover_ref
from tests.spans_ref import merge


def spans_batch_ref(hays, recs):
    """-> the (n, 3) int32 triples (haystack, start, end)"""
    rows = [np.concatenate([np.full((len(sp), 1), i, np.int32), sp], axis=1)
            for i, (h, r) in enumerate(zip(hays, recs)) for sp in [merge(r, len(h))]]
    return np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 3), np.int32)


def cover_batch_ref(hays, recs, open=(), close=(), body="keep", fill=ord("*")):
    """-> (units, out_offsets): every haystack's cover_ref, back to back"""
    parts = [cover_ref(np.asarray(h, np.uint16), r, open, close, body, fill) for h, r in zip(hays, recs)]
    off = np.zeros(len(parts) + 1, np.uint64)
    if parts:
        off[1:] = np.cumsum([p.size for p in parts], dtype=np.uint64)
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint16)).astype(np.uint16), off


def layout(hays, recs, n_open, n_close, body):
    """What every unit of the result is, from the reference's spans alone -> (kinds, stretch, item_at): kinds[o] is one of "open",
    "body", "close", "text" for output unit o and stretch[o] numbers the stretch of one kind it belongs to; item_at = the ascending
    output positions at which an ITEM of the batch begins -- a span's open, or a separator (which has no unit of its own: its
    position is that of the next unit)."""
    kinds, stretch, item_at, n_stretch = [], [], [], 0

    def put(kind, length):
        nonlocal n_stretch
        kinds.extend([kind] * length)
        stretch.extend([n_stretch] * length)
        n_stretch += 1

    for h, r in zip(hays, recs):
        last = 0
        for s, e in merge(r, len(h)).tolist():
            put("text", s - last)
            item_at.append(len(kinds))
            put("open", n_open)
            put("body", 0 if body == "drop" else e - s)
            put("close", n_close)
            last = e
        put("text", len(h) - last)
        item_at.append(len(kinds))  # the separator behind the haystack
    return kinds, np.array(stretch, np.int64), np.array(item_at, np.int64)


# ---- the two entries called raw, with a sentinel behind cap (the GPU tests) -------------------------------------------------
SENTINEL = 0x5A5A
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None


def cover_batch_raw(a, hays, cap, open="", close="", body="keep", fill="*"):
    """acgpu_cover_batch_u16 into a buffer with a sentinel behind cap -> (the units written, out_offsets, rc, n_out, stats)"""
    C = importlib.import_module("ahocorasick_amd.cover")
    units, off = _pack(hays)
    spec, keep = C._spec(utf16(open), utf16(close), C.BODIES[body], int(utf16(fill)[0]))
    out = np.full(cap + 64, SENTINEL, np.uint16)
    oo = np.full(len(hays) + 1, 99, np.uint64)
    n_out, st = ctypes.c_uint64(0), N.CoverStats()
    rc = N.lib().acgpu_cover_batch_u16(a.handle, vp(units), vp(off), len(hays), ctypes.byref(spec), vp(out), cap, vp(oo), ctypes.byref(n_out),
                                       ctypes.byref(st))
    assert (out[cap:] == SENTINEL).all(), "written at or beyond cap"
    return out[:min(cap, n_out.value)], oo, rc, int(n_out.value), st


def spans_batch_raw(a, hays, cap):
    """acgpu_spans_batch_u16 into a buffer with a sentinel behind cap (in spans) -> (the triples written, rc, n_out, stats)"""
    units, off = _pack(hays)
    out = np.full((cap + 16, 3), SENTINEL, np.int32)
    n_out, st = ctypes.c_uint64(0), N.SpansStats()
    rc = N.lib().acgpu_spans_batch_u16(a.handle, vp(units), vp(off), len(hays), vp(out), cap, ctypes.byref(n_out), ctypes.byref(st))
    assert (out[cap:] == SENTINEL).all(), "written at or beyond cap"
    return out[:min(cap, n_out.value)], rc, int(n_out.value), st
