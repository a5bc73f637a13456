"""ahocorasick_amd -- MI355X-native drop-in for the match() hot path of RokLenarcic/AhoCorasick.

The product is ahocorasick_amd/lib/libacgpu.so (C ABI: include/acgpu.h; HIP kernels: ahocorasick_amd/csrc/).
This package is the host-side mirror of the reference's API on top of it.  No CPU fallback exists.
"""
from .strings import (AhoCorasickMap, AhoCorasickSet, Automaton, IllegalArgumentException, LongestMatchMap,
                      LongestMatchSet, MapMatchListener, ReadableMatchListener, SetMatchListener, ShortestMatchMap, ShortestMatchSet, Stream, StringMap,
                      StringSet, WholeWordLongestMatchMap, WholeWordLongestMatchSet, WholeWordMatchMap, WholeWordMatchSet,
                      Utf8Error, utf8_line_offsets, utf8_unit_offsets, utf16)
from . import terms
from .terms import count_batch, count_batch_utf8
from .spans import spans, spans_batch, spans_batch_utf8, spans_device, spans_utf8  # (the name `spans` of this package is the function; the module: ahocorasick_amd.spans in sys.modules)
from .cover import (cover, cover_batch, cover_batch_units, cover_device, cover_utf8, highlight, highlight_batch, highlight_utf8, mask, mask_batch,
                    mask_utf8, redact, redact_batch, redact_utf8, cover_batch_bytes, cover_batch_utf8, highlight_batch_utf8, mask_batch_utf8,
                    redact_batch_utf8, CoverStream, cover_readable, cover_utf8_readable, mask_readable, mask_utf8_readable, highlight_readable,
                    highlight_utf8_readable, redact_readable, redact_utf8_readable)  # (as for spans: the name `cover` is the function)

__all__ = ["AhoCorasickSet", "AhoCorasickMap", "LongestMatchSet", "LongestMatchMap", "WholeWordMatchSet",
           "WholeWordMatchMap", "ShortestMatchSet", "ShortestMatchMap", "WholeWordLongestMatchSet", "WholeWordLongestMatchMap", "StringSet", "StringMap", "SetMatchListener", "MapMatchListener", "ReadableMatchListener", "Stream", "Automaton",
           "IllegalArgumentException", "utf16", "Utf8Error", "utf8_unit_offsets", "utf8_line_offsets",
           "terms", "count_batch", "count_batch_utf8", "spans", "spans_batch", "spans_utf8", "spans_device",
           "cover", "cover_utf8", "cover_device", "mask", "mask_utf8", "highlight", "highlight_utf8", "redact", "redact_utf8",
           "cover_batch", "cover_batch_units", "mask_batch", "highlight_batch", "redact_batch",
           "spans_batch_utf8", "cover_batch_utf8", "cover_batch_bytes", "mask_batch_utf8", "highlight_batch_utf8", "redact_batch_utf8",
           "CoverStream", "cover_readable", "cover_utf8_readable", "mask_readable", "mask_utf8_readable", "highlight_readable",
           "highlight_utf8_readable", "redact_readable", "redact_utf8_readable"]
