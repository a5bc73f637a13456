"""ctypes binding of include/acgpu.h (libacgpu.so).  There is no Python/CPU fallback: if the HIP library is
missing or no device is usable, every match call fails loudly."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ACGPU_LIB") or os.path.join(_HERE, "lib", "libacgpu.so")  # ACGPU_LIB: A/B builds

OK, E_INVALID, E_NONWORD, E_NOMEM, E_OVERFLOW, E_HIP, E_NODEVICE, E_UNSUPPORTED, E_ENCODING = 0, -1, -2, -3, -4, -5, -6, -7, -8
MODE_ALL, MODE_LONGEST, MODE_WHOLEWORD, MODE_SHORTEST, MODE_WWLONGEST = 0, 1, 2, 3, 4
REC_SET, REC_MAP = 8, 12
TRANSPORT_AUTO, TRANSPORT_RCCL, TRANSPORT_PEER = 0, 1, 2


def gather_slot_bytes(gcap, record_kind):
    """acgpu_gather_slot_bytes (include/acgpu.h): [16-byte acgpu_device_result | gcap records], padded to 16 bytes."""
    return (16 + int(gcap) * int(record_kind) + 15) & ~15


class AcgpuError(RuntimeError):
    def __init__(self, code, where=""):
        self.code = code
        msg = lib().acgpu_strerror(code).decode() if _lib is not None else str(code)
        if code == E_HIP:
            msg += " (hipError_t=%d)" % lib().acgpu_last_hip_error()
        super().__init__("%s: %s [%d]" % (where, msg, code))


class Utf8Error(ValueError):
    """ACGPU_E_ENCODING of acgpu_match_utf8: the haystack is not well-formed UTF-8.  start: the byte offset at which a strict
    decoder stops -- UnicodeDecodeError.start of bytes.decode("utf-8") on the same buffer.  haystack: None, or for the batch
    entries the index of the first ill-formed haystack; start is then an offset inside THAT haystack."""

    def __init__(self, start, haystack=None):
        self.start = int(start)
        self.haystack = None if haystack is None else int(haystack)
        if haystack is None:
            super().__init__("haystack is not well-formed UTF-8 at byte %d" % self.start)
        else:
            super().__init__("haystack %d is not well-formed UTF-8 at byte %d" % (self.haystack, self.start))


class Info(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_uint32), ("mode", ctypes.c_uint32), ("case_sensitive", ctypes.c_uint32),
                ("n_states", ctypes.c_uint32), ("n_classes", ctypes.c_uint32), ("n_keywords", ctypes.c_uint32),
                ("min_keyword_len", ctypes.c_uint32), ("max_keyword_len", ctypes.c_uint32), ("dense", ctypes.c_uint32),
                ("entry_bytes", ctypes.c_uint32), ("table_bytes", ctypes.c_uint64), ("lds_states", ctypes.c_uint32),
                ("fold_consistent", ctypes.c_uint32), ("filter_k", ctypes.c_uint32), ("filter_bits", ctypes.c_uint32),
                ("tile_kernel", ctypes.c_uint32), ("filter_density", ctypes.c_float), ("fold_clean", ctypes.c_uint32)]


class Shard(ctypes.Structure):
    _fields_ = [("d_hay", ctypes.c_void_p), ("n_units", ctypes.c_uint64), ("own_begin", ctypes.c_uint64),
                ("own_end", ctypes.c_uint64), ("text_begin", ctypes.c_int32), ("text_end", ctypes.c_int32),
                ("chain_entry", ctypes.c_int64), ("chain_exit", ctypes.c_int64), ("d_result", ctypes.c_void_p)]


class DeviceResult(ctypes.Structure):  # acgpu_device_result: what Shard.d_result receives, in stream order
    _fields_ = [("n_records", ctypes.c_uint64), ("redone", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


ABI_VERSION = 5


class Profile(ctypes.Structure):
    _fields_ = [("scan_ms", ctypes.c_float), ("finalize_ms", ctypes.c_float), ("total_ms", ctypes.c_float),
                ("scan_units", ctypes.c_uint64), ("n_matches", ctypes.c_uint64), ("scan_kernel", ctypes.c_char * 64)]


class CursorStats(ctypes.Structure):  # acgpu_cursor_stats
    _fields_ = [("records_delivered", ctypes.c_uint64), ("records_buffered", ctypes.c_uint64), ("units_scanned", ctypes.c_uint64),
                ("scan_end", ctypes.c_uint64), ("pieces", ctypes.c_uint32), ("rescans", ctypes.c_uint32), ("done", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class CountStats(ctypes.Structure):  # acgpu_count_stats
    _fields_ = [("n_records", ctypes.c_uint64), ("units_direct", ctypes.c_uint64), ("units_records", ctypes.c_uint64),
                ("pieces", ctypes.c_uint32), ("rescans", ctypes.c_uint32)]


class ReplaceStats(ctypes.Structure):  # acgpu_replace_stats
    _fields_ = [("n_records", ctypes.c_uint64), ("units_out", ctypes.c_uint64), ("pieces", ctypes.c_uint32), ("rescans", ctypes.c_uint32)]


class BatchSummary(ctypes.Structure):  # acgpu_batch_summary
    _fields_ = [("n_matches", ctypes.c_uint64), ("start", ctypes.c_int32), ("end", ctypes.c_int32), ("keyword_id", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class SummaryStats(ctypes.Structure):  # acgpu_summary_stats
    _fields_ = [("n_records", ctypes.c_uint64), ("n_matched", ctypes.c_uint64), ("pieces", ctypes.c_uint32), ("rescans", ctypes.c_uint32)]


class CountBatchStats(ctypes.Structure):  # acgpu_count_batch_stats
    _fields_ = [("n_records", ctypes.c_uint64), ("n_entries", ctypes.c_uint64), ("n_terms", ctypes.c_uint64), ("pieces", ctypes.c_uint32),
                ("rescans", ctypes.c_uint32), ("rows_cut", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class SpansStats(ctypes.Structure):  # acgpu_spans_stats
    _fields_ = [("n_records", ctypes.c_uint64), ("n_spans", ctypes.c_uint64), ("pieces", ctypes.c_uint32), ("rescans", ctypes.c_uint32),
                ("max_carry", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class CoverSpec(ctypes.Structure):  # acgpu_cover_spec
    _fields_ = [("open", ctypes.c_void_p), ("open_len", ctypes.c_uint32), ("close", ctypes.c_void_p), ("close_len", ctypes.c_uint32),
                ("body", ctypes.c_uint32), ("fill", ctypes.c_uint32)]


class CoverStats(ctypes.Structure):  # acgpu_cover_stats
    _fields_ = [("n_records", ctypes.c_uint64), ("n_spans", ctypes.c_uint64), ("units_out", ctypes.c_uint64), ("pieces", ctypes.c_uint32),
                ("rescans", ctypes.c_uint32), ("max_carry", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


COVER_KEEP, COVER_FILL, COVER_DROP = 0, 1, 2
COVER_TILE_UNITS, COVER_TILE_BYTES = 2048, 4096  # kEmitTile (csrc/acgpu_emit.h): the output elements a workgroup of k_cover_emit writes
COVER_LDS_SEGMENTS = 1536  # kCoverLds (csrc/acgpu_cover.hip): the segments of a tile k_cover_emit stages in LDS at most; tunable "cover_lds_segments"
SPAN_TILE = 2048  # kSpanTile (csrc/acgpu_spans.hip): the intervals a workgroup of the merge's scans takes
SPAN_BLOCK = 256  # kSpanBlock (csrc/acgpu_spans.hip): the tiles one step of the merge's level-2 scans (k_span_scan_mins, k_span_offsets) takes
SPAN_CHUNK = SPAN_BLOCK * SPAN_TILE  # the intervals behind one such step: kSpanBlock * kSpanTile, beyond which the level-2 scans carry
PLAN_TILE = 2048  # kPlanTile (csrc/acgpu_emit.h): the spans a workgroup of a DROP call's plan takes; k_cover_offsets scans kPlanBlock = 256 of their sums per step
TERMS_BLOCK = 2048  # kTermsBlock (csrc/acgpu_terms.hip): the records a workgroup of k_terms_block sorts and reduces


class Utf8Stats(ctypes.Structure):  # acgpu_utf8_stats
    _fields_ = [("n_units", ctypes.c_uint64), ("first_bad", ctypes.c_int64), ("ascii", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class Utf8BatchStats(ctypes.Structure):  # acgpu_utf8_batch_stats
    _fields_ = [("n_units", ctypes.c_uint64), ("first_bad", ctypes.c_int64), ("bad_haystack", ctypes.c_uint32), ("ascii", ctypes.c_uint32)]


class Utf8LossyStats(ctypes.Structure):  # acgpu_utf8_lossy_stats
    _fields_ = [("n_units", ctypes.c_uint64), ("n_replaced", ctypes.c_uint64), ("first_replaced", ctypes.c_int64),
                ("first_haystack", ctypes.c_uint32), ("ascii", ctypes.c_uint32)]


class Utf8StreamStats(ctypes.Structure):  # acgpu_utf8_stream_stats
    _fields_ = [("n_units", ctypes.c_uint64), ("first_bad", ctypes.c_int64), ("ascii", ctypes.c_uint32), ("held", ctypes.c_uint32)]


class Utf8LossyStreamStats(ctypes.Structure):  # acgpu_utf8_lossy_stream_stats
    _fields_ = [("n_units", ctypes.c_uint64), ("n_replaced", ctypes.c_uint64), ("ascii", ctypes.c_uint32), ("held", ctypes.c_uint32)]


def _summary_dtype():
    import numpy as np
    return np.dtype({"names": ["n_matches", "start", "end", "keyword_id", "reserved"],
                     "formats": [np.uint64, np.int32, np.int32, np.int32, np.int32],
                     "offsets": [0, 8, 12, 16, 20], "itemsize": 24})


SUMMARY_DTYPE = _summary_dtype()  # one acgpu_batch_summary as a numpy record


# the struct a strict UTF-8 entry reports in -> the one its _lossy twin fills instead
_LOSSY_STATS = {Utf8Stats: Utf8LossyStats, Utf8BatchStats: Utf8LossyStats, Utf8StreamStats: Utf8LossyStreamStats}
_UTF8_STATS = set(_LOSSY_STATS) | set(_LOSSY_STATS.values())


def _signatures():
    """The C ABI of include/acgpu.h, once: symbol -> (restype, argtypes); argtypes None: ctypes is told nothing about them.  The
    _lossy entries are their strict twins with another stats struct (_LOSSY_STATS) and are derived, not written out."""
    vp, u64, i64, u32, ci, P = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER
    sig = {
        "acgpu_build": (ci, [ci, vp, vp, u32, ci, vp, vp, P(vp), P(i64)]),
        "acgpu_free": (None, [vp]),
        "acgpu_get_info": (ci, [vp, P(Info)]),
        "acgpu_match_u16": (ci, [vp, vp, u64, ci, vp, u64, P(u64)]),
        "acgpu_match_batch_u16": (ci, [vp, vp, vp, u32, ci, vp, u64, P(u64)]),
        "acgpu_match_device": (ci, [vp, P(Shard), ci, vp, u64, P(u64), vp, P(Profile)]),
        "acgpu_match_device_begin": (ci, [vp, P(Shard), ci, vp, u64, vp, ci, P(vp)]),
        "acgpu_match_device_end": (ci, [vp, vp, P(u64), P(Profile)]),
        "acgpu_match_device_abandon": (ci, [vp, vp]),
        "acgpu_synth_fill": (ci, [vp, u64, u64, u64, vp, u32, vp]),
        "acgpu_synth_tokens": (ci, [vp, u64, u64, vp, vp, u32, vp, vp]),
        "acgpu_stream_probe": (ci, [vp, u64, vp, ci, ci, P(ctypes.c_float)]),
        "acgpu_set_tunable": (i64, [ctypes.c_char_p, i64]),
        "acgpu_strerror": (ctypes.c_char_p, [ci]),
        "acgpu_last_hip_error": (ci, None),
        "acgpu_abi_version": (u32, None),
        "acgpu_debug_states": (ci, [vp, vp, vp, vp, vp, vp, vp]),
        "acgpu_debug_tables": (ci, [vp, vp, vp, vp, vp, vp, vp, P(u32)]),
        "acgpu_debug_wordhash_perfect": (ci, [vp, vp, vp, vp, vp, vp, vp]),
        "acgpu_debug_wordhash": (ci, [vp, P(u32), vp, P(u64), vp, vp, P(u32), vp, P(u32)]),
        "acgpu_stream_open": (ci, [vp, P(vp)]),
        "acgpu_stream_feed": (ci, [vp, vp, u64, ci, ci, vp, u64, P(u64), P(i64)]),
        "acgpu_stream_feed_utf8": (ci, [vp, vp, u64, ci, ci, vp, u64, P(u64), P(i64), P(Utf8StreamStats)]),
        "acgpu_stream_replace_u16": (ci, [vp, vp, u64, ci, vp, vp, u32, vp, u64, P(u64), P(ReplaceStats)]),
        "acgpu_stream_replace_utf8": (ci, [vp, vp, u64, ci, vp, vp, u32, vp, u64, P(u64), P(Utf8StreamStats), P(ReplaceStats)]),
        "acgpu_stream_cover_u16": (ci, [vp, vp, u64, ci, P(CoverSpec), vp, u64, P(u64), P(CoverStats)]),
        "acgpu_stream_cover_utf8": (ci, [vp, vp, u64, ci, P(CoverSpec), vp, u64, P(u64), P(Utf8StreamStats), P(CoverStats)]),
        "acgpu_stream_close": (None, [vp]),
        "acgpu_stream_set_pipelined": (ci, [vp, ci]),
        "acgpu_stream_reserve": (ci, [vp, u64, P(vp)]),
        "acgpu_cursor_open": (ci, [vp, vp, u64, ci, P(vp)]),
        "acgpu_cursor_next": (ci, [vp, vp, u64, P(u64)]),
        "acgpu_cursor_get_stats": (ci, [vp, P(CursorStats)]),
        "acgpu_cursor_close": (None, [vp]),
        "acgpu_count_u16": (ci, [vp, vp, u64, vp, u32, P(CountStats)]),
        "acgpu_count_device": (ci, [vp, P(Shard), vp, u32, vp, P(CountStats)]),
        "acgpu_replace_u16": (ci, [vp, vp, u64, vp, vp, u32, vp, u64, P(u64), P(ReplaceStats)]),
        "acgpu_replace_device": (ci, [vp, P(Shard), vp, vp, u32, vp, u64, P(u64), vp, P(ReplaceStats)]),
        "acgpu_replace_batch_u16": (ci, [vp, vp, vp, u32, vp, vp, u32, vp, u64, vp, P(u64), P(ReplaceStats)]),
        "acgpu_summary_batch_u16": (ci, [vp, vp, vp, u32, vp, P(SummaryStats)]),
        "acgpu_match_utf8": (ci, [vp, vp, u64, ci, vp, u64, P(u64), P(Utf8Stats)]),
        "acgpu_match_batch_utf8": (ci, [vp, vp, vp, u32, ci, vp, u64, P(u64), P(Utf8BatchStats)]),
        "acgpu_summary_batch_utf8": (ci, [vp, vp, vp, u32, vp, P(SummaryStats), P(Utf8BatchStats)]),
        "acgpu_count_batch_u16": (ci, [vp, vp, vp, u32, vp, vp, vp, u64, P(u64), P(CountBatchStats)]),
        "acgpu_count_batch_utf8": (ci, [vp, vp, vp, u32, vp, vp, vp, u64, P(u64), P(CountBatchStats), P(Utf8BatchStats)]),
        "acgpu_debug_count_batch_finish": (ci, [vp, u64, u32, vp, vp, vp, P(u64), P(u32)]),
        "acgpu_replace_utf8": (ci, [vp, vp, u64, vp, vp, u32, vp, u64, P(u64), P(ReplaceStats), P(Utf8Stats)]),
        "acgpu_replace_batch_utf8": (ci, [vp, vp, vp, u32, vp, vp, u32, vp, u64, vp, P(u64), P(ReplaceStats), P(Utf8BatchStats)]),
        "acgpu_spans_u16": (ci, [vp, vp, u64, vp, u64, P(u64), P(SpansStats)]),
        "acgpu_spans_device": (ci, [vp, P(Shard), vp, u64, P(u64), vp, P(SpansStats)]),
        "acgpu_spans_batch_u16": (ci, [vp, vp, vp, u32, vp, u64, P(u64), P(SpansStats)]),
        "acgpu_spans_utf8": (ci, [vp, vp, u64, vp, u64, P(u64), P(SpansStats), P(Utf8Stats)]),
        "acgpu_cover_u16": (ci, [vp, vp, u64, P(CoverSpec), vp, u64, P(u64), P(CoverStats)]),
        "acgpu_cover_device": (ci, [vp, P(Shard), P(CoverSpec), vp, u64, P(u64), vp, P(CoverStats)]),
        "acgpu_cover_batch_u16": (ci, [vp, vp, vp, u32, P(CoverSpec), vp, u64, vp, P(u64), P(CoverStats)]),
        "acgpu_cover_utf8": (ci, [vp, vp, u64, P(CoverSpec), vp, u64, P(u64), P(CoverStats), P(Utf8Stats)]),
        "acgpu_spans_batch_utf8": (ci, [vp, vp, vp, u32, vp, u64, P(u64), P(SpansStats), P(Utf8BatchStats)]),
        "acgpu_cover_batch_utf8": (ci, [vp, vp, vp, u32, P(CoverSpec), vp, u64, vp, P(u64), P(CoverStats), P(Utf8BatchStats)]),
        "acgpu_match_u16_multi": (ci, [vp, vp, u64, P(ci), ci, ci, vp, u64, P(u64)]),
        "acgpu_comm_open": (ci, [P(ci), ci, ci, P(vp)]),
        "acgpu_comm_close": (None, [vp]),
        "acgpu_comm_transport": (ci, [vp]),
        "acgpu_comm_stream": (vp, [vp, ci]),
        "acgpu_match_device_allgather": (ci, [vp, vp, P(Shard), ci, P(vp), u64, P(u64), P(Profile)]),
        "acgpu_last_rccl_error": (ci, None),
        "acgpu_gather_slot_bytes": (u64, [u64, ci]),
    }
    for name, (restype, argtypes) in list(sig.items()):
        twin = [P(_LOSSY_STATS[t._type_]) if getattr(t, "_type_", None) in _LOSSY_STATS else t for t in argtypes or ()]
        if twin != (argtypes or []):
            sig[name + "_lossy"] = (restype, twin)
    return sig


SIGNATURES = _signatures()
SYMBOLS = list(SIGNATURES)  # every symbol include/acgpu.h declares


# entry -> the UTF-8 stats struct it fills, for the entries that have one: a key of _LOSSY_STATS for a strict entry, a value for its twin
UTF8_STATS = {name: t._type_ for name, (_, argtypes) in SIGNATURES.items() for t in argtypes or () if getattr(t, "_type_", None) in _UTF8_STATS}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "ahocorasick_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C ahocorasick_amd/csrc`).  There is no CPU fallback." % LIB_PATH)
        try:
            # PyTorch-ROCm bundles its own libamdhip64.so (same SONAME, libamdhip64.so.7).  Loading torch first makes
            # libacgpu.so bind to that copy; the other order would put two HIP/HSA runtimes in one process and the
            # second one finds no GPU.  Without torch (JNI / plain C callers) libacgpu.so uses /opt/rocm's runtime.
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = restype
            if argtypes is not None:
                fn.argtypes = argtypes
        if L.acgpu_abi_version() != ABI_VERSION:
            raise ImportError("ahocorasick_amd: %s has ABI version %d, this package binds version %d -- rebuild it"
                              % (LIB_PATH, L.acgpu_abi_version(), ABI_VERSION))
        _lib = L
    return _lib


def _code_only(text):
    """C / C++ / HIP source without comments and with runs of white space collapsed: what the compiler sees of it.  (String and
    character literals are kept as they are; a comment marker inside one is left alone.)"""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if c == '"' and i > 0 and text[i - 1] == "R" and not (i > 1 and (text[i - 2].isalnum() or text[i - 2] == "_")):
            # raw string literal R"delim( ... )delim": copied whole
            k = text.find("(", i)
            end = text.find(")" + text[i + 1:k] + '"', k) if k >= 0 else -1
            j = n - 1 if end < 0 else end + (k - i)
            out.append(text[i:j + 1])
            i = j + 1
        elif c == "'" and i > 0 and text[i - 1].isalnum():  # a digit separator (1'000'000), not a character literal
            out.append(c)
            i += 1
        elif c in "\"'":  # literal: copy to its closing quote
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            out.append(text[i:j + 1])
            i = j + 1
        elif text.startswith("//", i):
            j = text.find("\n", i)
            i = n if j < 0 else j
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            i = n if j < 0 else j + 2
            out.append(" ")
        else:
            out.append(c)
            i += 1
    return " ".join("".join(out).split())


def source_hash():
    """SHA-256 (first 16 hex digits) over the CODE of the kernel and builder sources -- comments and white space are not part of
    it: what measured evidence (profiles/latest_traffic.json) is keyed by, so that a counter figure is never attached to a kernel
    that has been edited since, while an edit of a comment does not ask for a new collection."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.h")) +
                   glob.glob(os.path.join(_HERE, "csrc", "*.cpp")) + [os.path.join(os.path.dirname(_HERE), "include", "acgpu.h")])
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "r", encoding="utf-8", errors="replace") as fh:
            h.update(_code_only(fh.read()).encode())
    return h.hexdigest()[:16]


def check(rc, where):
    if rc != OK:
        raise AcgpuError(rc, where)


def set_tunable(name, value):
    return lib().acgpu_set_tunable(name.encode(), int(value))
