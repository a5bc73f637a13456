"""The reference of the cover tests (include/acgpu.h: acgpu_cover_*): the spans of tests/spans_ref.merge over the oracle's records,
spliced with Python slices.  Works on any numpy array of elements -- UTF-16 units or UTF-8 bytes.  A helper, not collected."""
import numpy as np

from ahocorasick_amd.strings import utf8_unit_offsets
from tests.spans_ref import merge


def cover_ref(text, recs, open=(), close=(), body="keep", fill=ord("*")):
    """text: 1-d array of elements; recs: (k, >= 2) records in elements -> the covered text, same dtype"""
    text = np.asarray(text)
    open, close = np.asarray(open, text.dtype), np.asarray(close, text.dtype)
    parts, last = [], 0
    for s, e in merge(recs, text.size).tolist():
        inner = {"keep": text[s:e], "fill": np.full(e - s, fill, text.dtype), "drop": text[:0]}[body]
        parts += [text[last:s], open, inner, close]
        last = e
    return np.concatenate(parts + [text[last:]]).astype(text.dtype)


def byte_records(recs, data):
    """records of the DECODED text (UTF-16 units) -> byte offsets into the well-formed UTF-8 `data`: a start is the first byte of
    the code point that holds the unit, an end one past the last byte of the code point that holds unit end - 1"""
    recs = np.asarray(recs, np.int64).reshape(len(recs), -1)
    b = np.frombuffer(bytes(data), np.uint8)
    off = utf8_unit_offsets(b)
    if not len(recs):
        return np.zeros((0, 2), np.int32)
    lead = b[off[recs[:, 1] - 1]]
    seq = 1 + (lead >= 0xC0) + (lead >= 0xE0) + (lead >= 0xF0)
    return np.stack([off[recs[:, 0]], off[recs[:, 1] - 1] + seq], axis=1).astype(np.int32)
