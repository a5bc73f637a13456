// acgpu_replace.hip -- acgpu_replace_u16 / acgpu_replace_device (include/acgpu.h): the text with every match of a non-overlapping
// family replaced, written on the device.
//
// A replace call is the third consumer of the piece driver (scan_next_piece, acgpu_pieces.hip): the Map records of a piece stay
// in the pool's reservoir, the piece's text is on the device already (d.stage_hay, or the caller's buffer), and behind every piece
//  * the PLAN (acgpu_emit.h; k_replace_sums, k_replace_offsets, k_replace_plan), whose items are the records' deltas, turns record
//    i into the output position of its replacement, pos_i = (s_i - done) + sum over j < i of (rlen[id_j] - (e_j - s_j)), 64-bit.
//    The positions ascend weakly: deleted matches that touch each other share one;
//  * the EMIT (acgpu_emit.h; k_replace_emit) writes a window of the piece's output from its SOURCE (EmitArgs): segments of two
//    sources, a record's replacement and the text behind the record up to the next one.
// The host keeps `done`, the text position up to which output exists, and `out_pos`, the units written so far; what a piece may
// emit, [done, limit), is decided by replace_limit below.
//
// acgpu_replace_batch_u16 rewrites many short texts as ONE such text: the haystacks with a separator unit behind each (the batch
// match call's concatenation), where a separator is a match that is deleted.  Behind every piece k_replace_merge merges the piece's
// records with the pseudo-records of its separators; plan and emit run over the merged list as they are, so the results come out
// back to back, and k_replace_batch_offsets reads every result's first output unit off the plan.  The separators' descriptor, the
// two searches of the merge and the host's range of them (separators_in) are acgpu_emit.h's, shared with the cover entries.
//
// acgpu_replace_utf8 rewrites a UTF-8 text in BYTES: the text is staged by stage_utf8_text (acgpu_utf8.hip) and scanned in UTF-16
// units as a device shard; behind every piece its records become byte offsets (utf8_map_records) and its boundary a byte position
// (utf8_map_position), and from there on the driver's bookkeeping, the plan and the emit count bytes: the emit is a template over
// the element, k_replace_emit<uint16_t> for the entries above and k_replace_emit<uint8_t> for this one.
//
// acgpu_replace_batch_utf8 rewrites many UTF-8 texts as ONE span of bytes: stage_utf8_batch stages them as the device shard the
// batch match call scans (a separator unit behind every haystack), and behind every piece its records become bytes of the span
// (utf8_map_records with the batch) and its boundary a byte of it (utf8_map_position with the batch).  The span itself has NO separators, so nothing
// is merged and nothing deleted: plan and emit run over the records alone, and the results lie back to back because the
// haystacks do.  Where each result begins is computed behind the plan by k_replace_span_offsets, a lane per haystack boundary.
// Its front (staging, stats, what an encoding error leaves) and its route haystack by haystack are utf8_batch_front and
// utf8_each_haystack of acgpu_host.h, shared with the spans and cover entries.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "acgpu_device.h"
#include "acgpu_emit.h"
#include "acgpu_host.h"
#include "acgpu_internal.h"

using namespace acgpu;

namespace {

constexpr int kEmitLds = 3072; // segments a workgroup stages (16 bytes each)
constexpr int kPlanHead = 4;   // words in front of the plan's sums: {sum of the deltas, last end, the piece's boundary in bytes (UTF-8), unused}

// (Records, the table's entries, the plan and the windows count elements; "unit" below means element.)

// The replacement table on the device: n_repl entries {first unit in `units`, length}, then the units.
struct ReplTable {
    const uint2 *ent;
    const void *units; // uint16_t or uint8_t: the emit's element
    uint32_t n_repl;   // 1: that replacement stands for every keyword
};

__device__ __forceinline__ uint2 repl_of(const ReplTable &rt, int32_t id) {
    return rt.ent[rt.n_repl == 1 ? 0u : std::min<uint32_t>((uint32_t)id, rt.n_repl - 1)];
}

// The plan's item: what record i adds to the output's length, its replacement's units minus the match's
__device__ __forceinline__ int64_t repl_delta(const int32_t *recs, uint64_t i, const ReplTable &rt) {
    const int32_t s = recs[3 * i], e = recs[3 * i + 1], id = recs[3 * i + 2];
    return (int64_t)repl_of(rt, id).y - (int64_t)(e - s);
}

// the plan (acgpu_emit.h) over a piece's n records
__global__ __launch_bounds__(kPlanBlock) void k_replace_sums(const int32_t *__restrict__ recs, uint64_t n, ReplTable rt, int64_t *__restrict__ bsum) {
    plan_sums([=](uint64_t i) { return repl_delta(recs, i, rt); }, n, bsum);
}

// slot[0] = the sum of all deltas, slot[1] = the end of the last record
__global__ __launch_bounds__(kPlanBlock) void k_replace_offsets(int64_t *__restrict__ bsum, uint32_t n_blocks, const int32_t *__restrict__ recs, uint64_t n,
                                                                int64_t *__restrict__ slot) {
    const int64_t sum = plan_offsets(bsum, n_blocks);
    if (threadIdx.x == 0) {
        slot[0] = sum;
        slot[1] = n ? (int64_t)recs[3 * (n - 1) + 1] : 0;
    }
}

// pos[i] = (s_i - done) + the deltas in front of record i (done: buffer relative, as the records are)
__global__ __launch_bounds__(kPlanBlock) void k_replace_plan(const int32_t *__restrict__ recs, uint64_t n, ReplTable rt, const int64_t *__restrict__ bsum,
                                                             int64_t done, int64_t *__restrict__ pos) {
    plan_positions([=](uint64_t i) { return repl_delta(recs, i, rt); }, n, bsum,
                   [&](uint64_t i, int64_t front) { pos[i] = (int64_t)recs[3 * i] - done + front; });
}

// A segment of two sources: from u = rel on, the units below rend are units rsrc + u of the replacement table, the others units
// tsrc + u of the text.
struct Seg {
    int32_t rel, rend;
    uint32_t rsrc, tsrc;
};

// The emit's source (acgpu_emit.h): the text with a piece's records replaced.
template <class T>
struct EmitArgs {
    using Elem = T;
    using Seg = ::Seg;
    static constexpr int kLds = kEmitLds;
    const T *hay;         // the piece's buffer
    const int32_t *recs;  // its Map records, buffer relative
    const int64_t *pos;   // the plan
    int64_t n_recs;
    ReplTable rt;
    int64_t done;         // buffer relative: output unit 0 of the piece is text unit `done` (if no record starts there)
    int64_t w0, w1;
    T *dst;
    __device__ __forceinline__ const T *repl() const { return static_cast<const T *>(rt.units); }
    __device__ __forceinline__ int32_t lds_cap() const { return kLds; }
    __device__ __forceinline__ int64_t n() const { return n_recs; }
    __device__ __forceinline__ int64_t pos_at(int64_t i) const { return pos[i]; }
    __device__ __forceinline__ Seg make_seg(int64_t i, int64_t t0) const {
        Seg s;
        if (i < 0) {
            s.rel = -1;
            s.rend = 0;
            s.rsrc = 0;
            s.tsrc = (uint32_t)(done + t0);
            return s;
        }
        const int64_t P = pos[i] - t0; // < kEmitTile<T>
        const uint2 r = repl_of(rt, recs[3 * i + 2]);
        const int64_t rend = P + (int64_t)r.y;
        s.rel = (int32_t)std::max<int64_t>(P, -1);
        s.rend = (int32_t)std::min<int64_t>(std::max<int64_t>(rend, 0), kEmitTile<T>);
        s.rsrc = r.x - (uint32_t)P;
        s.tsrc = (uint32_t)recs[3 * i + 1] - (uint32_t)rend;
        return s;
    }
    __device__ __forceinline__ bool whole(const Seg &s, int32_t u0, rp_v4u *v) const {
        if (u0 >= s.rend) *v = load16(hay + (uint32_t)(s.tsrc + (uint32_t)u0));
        else if (u0 + kEmitPer<T> <= s.rend) *v = load16(repl() + (uint32_t)(s.rsrc + (uint32_t)u0));
        else return false;
        return true;
    }
    __device__ __forceinline__ uint32_t element(const Seg &s, int32_t u) const {
        return u < s.rend ? repl()[(uint32_t)(s.rsrc + (uint32_t)u)] : hay[(uint32_t)(s.tsrc + (uint32_t)u)];
    }
};

template <class T>
__global__ __launch_bounds__(kEmitBlock) void k_replace_emit(EmitArgs<T> A) {
    emit_block(A);
}

constexpr int kMergeBlock = 256;

// a piece's records: three words each, ascending starts
__device__ __forceinline__ uint64_t records_before(const int32_t *__restrict__ recs, uint64_t cnt, int64_t p) {
    return starts_before([=](uint64_t i) { return recs[3 * i]; }, cnt, p);
}

// A batch call's piece (THE SEPARATORS, acgpu_emit.h): its cnt records and the pseudo-records {p, p + 1, id} of its separators as
// one list in position order -- a record neither contains nor starts at a separator.  id: the keyword id of a pseudo-record, the
// empty slot behind the replacement table.
__global__ __launch_bounds__(kMergeBlock) void k_replace_merge(const int32_t *__restrict__ recs, uint64_t cnt, BatchSeps S, int32_t id, int32_t *__restrict__ merged) {
    const uint64_t t = (uint64_t)blockIdx.x * kMergeBlock + threadIdx.x;
    if (t < cnt) {
        const int32_t s = recs[3 * t];
        int32_t *o = merged + 3 * (t + seps_before(S, S.n_sep, s));
        o[0] = s;
        o[1] = recs[3 * t + 1];
        o[2] = recs[3 * t + 2];
    } else if (t < cnt + S.n_sep) {
        const int64_t p = sep_at(S, (uint32_t)(t - cnt));
        int32_t *o = merged + 3 * (t - cnt + records_before(recs, cnt, p));
        o[0] = (int32_t)p;
        o[1] = (int32_t)p + 1;
        o[2] = id;
    }
}

// Behind the plan of such a merged list: separator i0 + j ends haystack i0 + j, so the result of haystack i0 + j + 1 begins where
// the separator's (empty) replacement stands -- out_pos, the output in front of the piece, plus the plan's position of its record.
__global__ __launch_bounds__(kMergeBlock) void k_replace_batch_offsets(const int32_t *__restrict__ recs, uint64_t cnt, BatchSeps S,
                                                                       const int64_t *__restrict__ pos, uint64_t out_pos,
                                                                       uint64_t *__restrict__ out_off) {
    const uint32_t j = blockIdx.x * kMergeBlock + threadIdx.x;
    if (j >= S.n_sep) return;
    out_off[(uint64_t)S.i0 + j + 1] = out_pos + (uint64_t)pos[j + records_before(recs, cnt, sep_at(S, j))];
}

// A UTF-8 batch call, behind a piece's plan: the output offset of the n_b haystack boundaries j0 .. j0 + n_b - 1 that the piece
// emits (span_boundaries, acgpu_host.h), a lane per boundary.  b = boff[j] is a byte of the span with done <= b <= limit, and with
// k = the piece's records that start before b (records and `done` in bytes of the span):
//   k == 0 : out_off[j] = out_pos + (b - done)                                       -- text only in front of b
//   k  > 0 : out_off[j] = out_pos + pos[k - 1] + rlen[id_{k-1}] + (b - e_{k-1})      -- record k - 1's replacement, then text
// No record crosses a haystack boundary (in the scan's text a separator stands there), so e_{k-1} <= b; and the records in
// front of b are the first k of the list because starts ascend.  A run of empty haystacks is several lanes with the same b.
__global__ __launch_bounds__(kMergeBlock) void k_replace_span_offsets(const int32_t *__restrict__ recs, uint64_t cnt, ReplTable rt,
                                                                      const int64_t *__restrict__ pos, const uint32_t *__restrict__ boff, uint32_t j0,
                                                                      uint32_t n_b, int64_t done, uint64_t out_pos, uint64_t *__restrict__ out_off) {
    const uint32_t t = blockIdx.x * kMergeBlock + threadIdx.x;
    if (t >= n_b) return;
    const int64_t b = (int64_t)boff[j0 + t];
    const uint64_t k = records_before(recs, cnt, b);
    int64_t at = b - done;
    if (k) at = pos[k - 1] + (int64_t)repl_of(rt, recs[3 * (k - 1) + 2]).y + (b - (int64_t)recs[3 * (k - 1) + 1]);
    out_off[j0 + t] = out_pos + (uint64_t)at;
}

// What one call holds while it runs (the caller holds d.mu).
struct ReplaceCall {
    acgpu_automaton *a;
    DeviceState &d;
    hipStream_t stream;
    ReplTable rt{};
    uint32_t esz = 2;          // bytes of an element: 2, a UTF-16 unit; 1, a byte of a UTF-8 text (acgpu_replace_utf8).  What follows counts elements
    const Utf8Text *u8 = nullptr; // esz == 1: the staged text -- the scan runs over its units, everything below counts its bytes
    const Utf8Batch *ub = nullptr; // ... a batch of them staged as one shard (u8 == &ub->text): n, done and the records count bytes of the SPAN;
                                   // n_hay haystacks, d_out_off as below
    uint8_t *h_out = nullptr;  // the host entry's result (through the slabs) ...
    uint8_t *d_out = nullptr;  // ... or the device entry's
    uint64_t cap = 0;
    uint64_t n = 0;            // units of the text
    uint64_t done = 0;         // output exists for the text's units [0, done)
    uint64_t out_pos = 0;      // units of it (beyond cap: counted, not written)
    acgpu_replace_stats st{};
    // a batch call: the concatenation's offsets on the host (n_hay + 1 words), what the current piece merges (seps.cat_off: the
    // offsets on the device, set for the whole call), the result's offsets on the device (n_hay + 1 words of 64 bits)
    const uint32_t *h_cat_off = nullptr;
    uint32_t n_hay = 0;
    BatchSeps seps{};
    int32_t sep_id = 0; // the keyword id of a separator's pseudo-record
    uint64_t *d_out_off = nullptr;
};

// full: the table in its full form, whatever n_repl is -- an entry per keyword given to acgpu_build (a single replacement: they
// share its units) and behind them an empty one, the slot of a batch call's separators; repl_of then never sees n_repl == 1 where
// there is a keyword.
// repl_units: c.esz bytes each; the entries are {first, length} in those.  Behind the units the blob is padded so that an aligned
// 16-byte load around any of them stays inside it.
int upload_table(ReplaceCall &c, const void *repl_units, const uint64_t *repl_off, uint32_t n_repl, bool full = false) {
    const uint64_t r0 = n_repl ? repl_off[0] : 0, total = n_repl ? repl_off[n_repl] - r0 : 0;
    const uint32_t n_ent = full ? c.a->n_given + 1 : n_repl;
    const size_t ent_bytes = ((size_t)n_ent * 8 + 15) & ~(size_t)15;
    std::vector<uint64_t> blob;
    try {
        blob.assign((ent_bytes + (size_t)total * c.esz + 16 + 7) / 8, 0);
    } catch (...) {
        return ACGPU_E_NOMEM;
    }
    uint32_t *ent = reinterpret_cast<uint32_t *>(blob.data());
    for (uint32_t i = 0; i < n_ent; ++i) {
        const uint32_t from = n_repl == 1 ? 0 : i; // (the blob is zeroed: the entries behind the caller's stay empty)
        if (from >= n_repl || (full && i + 1 == n_ent)) continue;
        ent[2 * i] = (uint32_t)(repl_off[from] - r0);
        ent[2 * i + 1] = (uint32_t)(repl_off[from + 1] - repl_off[from]);
    }
    if (total) std::copy_n(static_cast<const char *>(repl_units) + r0 * c.esz, total * c.esz, reinterpret_cast<char *>(blob.data()) + ent_bytes);
    const int rc = c.d.replace_tab.ensure(blob.size() * 8);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(c.d.replace_tab.p, blob.data(), blob.size() * 8, hipMemcpyHostToDevice)); // (blocking: the blob dies here)
    c.rt.ent = reinterpret_cast<const uint2 *>(c.d.replace_tab.p);
    c.rt.units = reinterpret_cast<const char *>(c.d.replace_tab.p) + ent_bytes;
    c.rt.n_repl = n_ent;
    return ACGPU_OK;
}

// The text position up to which a piece that owned [.., own_hi) and reported records up to last_end (0: none) may emit.
//  * last piece, or the text as one piece: the text's end.
//  * LONGEST, WHOLEWORD, WWLONGEST -- a match belongs to the piece that owns its FIRST unit: every later piece's records start at
//    or behind own_hi, and, as the records of a text do not overlap and come in position order, at or behind last_end.  So nothing
//    starts before max(own_hi, last_end).  That lies inside the buffer: a record starts before own_hi and has at most max_len
//    units, which the right halo (max_len - 1 units and more) holds; and `done`, where the next piece's emit starts, is at least
//    its own_lo, the buffer's first unit but for the one unit of left context of the word matchers.
//  * SHORTEST -- a match belongs to the piece that owns its LAST unit: a later record ends behind own_hi, so it starts at or
//    behind own_hi - (max_len - 1), and at or behind every earlier record's end, which `done` and last_end bound.  The units
//    withheld, at most max_len - 1 in front of own_hi, are the next piece's left halo: it emits them from there.  The limit never
//    exceeds own_hi, the buffer's end.
//  * A BATCH call's piece merges the separators in [done, own_hi), every family, and last_end is the end of the last element of
//    the merged list, record or separator.  A first-unit family's record that starts before own_hi cannot reach across a separator
//    at or behind own_hi, so no separator lies in [own_hi, last_end).  For SHORTEST a later record ends behind own_hi and holds no
//    separator, so it starts behind the last merged separator: max(last_end, done, own_hi - (max_len - 1)) is still a position no
//    later record starts before.  And every separator below the limit has been merged: the limit is at most own_hi, or, for the
//    first-unit families, at most the end of a record that holds no separator.  So the plan's sum holds exactly the elements below
//    the limit, and every separator is merged by exactly one piece: the one that emits it.
//  * A UTF-8 call scans in units and keeps n, done, last_end and the limit in BYTES.  Its keywords are well-formed UTF-16
//    (HostTables::lone_surrogate is refused), so every record begins and ends on a code-point boundary of the text, and the map
//    from such unit positions to byte positions is exact and monotone: records that neither overlap nor are out of order in units
//    are neither in bytes.  The piece's boundary (piece_bound, in units) is the one position that need not be a code-point
//    boundary -- a piece may end between the two units of a surrogate pair -- so it is mapped to the first byte of the code point
//    that HOLDS it, i.e. rounded down (utf8_map_position).  A later record starts on a code-point boundary at or behind that
//    unit, therefore at or behind the rounded byte; rounding down only withholds more, and the limit still takes the maximum
//    with done and last_end, so it never falls behind what has been emitted or inside a record of this piece.  The text is on
//    the device as a whole, so "inside the buffer" holds trivially.
//  * A UTF-8 BATCH call scans the haystacks' units with a separator behind each and keeps n, done, last_end and the limit in bytes
//    of the caller's SPAN, which has no separators.  The map unit -> span byte (k_utf8_batch_map for records, k_utf8_batch_pos
//    for the boundary) drops the h separators in front of haystack h and is monotone; a boundary that IS a separator maps to the
//    byte where the next haystack begins.  A later record starts at or behind the boundary's unit x (first-unit families: at or
//    behind own_hi; SHORTEST: at or behind own_hi - (max_len - 1), as above, and no record holds a separator): if x is a unit of
//    a haystack, on a code-point boundary at or behind it, so at or behind the rounded byte; if x is haystack h's separator, in a
//    haystack behind h, so at or behind boff[h + 1].  The rest is the UTF-8 argument.  Two facts that k_replace_span_offsets
//    rests on follow.  (1) Every record of a piece's list lies below the piece's limit: the limit is at least last_end, the end
//    of the list's last record, and the records ascend without overlapping -- so for a boundary b < limit, or any b on the last
//    piece, the records counted in front of b are all planned by THIS piece, and the plan's sum is over exactly the list.
//    (2) `done` never exceeds the first record's start: done is the previous piece's limit, a position no later record starts
//    before -- for the first-unit families because such a record starts at or behind that piece's own_hi and last_end, for
//    SHORTEST because it ends behind that piece's own_hi, hence starts at or behind own_hi - (max_len - 1), and behind every
//    earlier record's end.  So b - done and pos[] (which are relative to done) are not negative for the boundaries a piece takes.
//  * A LOSSY UTF-8 call (text, batch or a stream's feed) scans the units of the text decoded with errors="replace" and keeps n,
//    done, last_end and the limit in bytes of the caller's buffer as it is.  The units tile the bytes in order: a unit is a
//    START of the bitmap -- a well-formed sequence (two units where it has four bytes) or a maximal ill-formed subpart of one
//    to three bytes, which is ONE unit, U+FFFD.  The decoded text is well-formed UTF-16 and so are the keywords, so every
//    record begins and ends between two starts; the map from such unit positions to bytes (locate's lossy form, over the
//    bitmap) is exact and monotone, and a record that holds a subpart's U+FFFD covers all the subpart's bytes and nothing
//    else of it -- records that do not overlap in units do not overlap in bytes.  The piece's boundary is rounded down to the
//    first byte of the START that holds it: for a subpart that IS the unit's own first byte -- a boundary never falls inside
//    a subpart, which has one unit -- and only between the two units of a surrogate pair does rounding withhold anything.  A
//    boundary on, directly before or directly behind a subpart is therefore a byte between two starts, and a later record
//    starts at a start at or behind it.  In a batch the haystack boundaries are starts of the bitmap (a byte at a cut is never
//    claimed), so the separator rule above holds as it stands.  A text with as many units as bytes has no checkpoints and no
//    bitmap: every start is one byte and one unit, and the unit is the byte, as in an ASCII text.
// piece_bound: the family's part of the rule, in the scan's coordinates; replace_limit: the maximum, in the driver's.
uint64_t piece_bound(const HostTables &t, uint64_t own_hi) {
    if (t.mode != ACGPU_MODE_SHORTEST) return own_hi;
    const uint64_t back = t.max_len ? t.max_len - 1 : 0;
    return own_hi > back ? own_hi - back : 0;
}

uint64_t replace_limit(bool last_or_whole, uint64_t n, uint64_t bound, uint64_t last_end, uint64_t done) {
    return last_or_whole ? n : std::max({bound, last_end, done});
}

template <class T>
int launch_emit_as(ReplaceCall &c, const void *hay, const int32_t *recs, uint64_t cnt, int64_t done_rel, uint64_t w0, uint64_t w1, void *dst) {
    EmitArgs<T> A;
    A.hay = static_cast<const T *>(hay);
    A.recs = recs;
    A.pos = reinterpret_cast<const int64_t *>(c.d.replace_plan.p) + kPlanHead + (cnt + kPlanTile - 1) / kPlanTile;
    A.n_recs = (int64_t)cnt;
    A.rt = c.rt;
    A.done = done_rel;
    return launch_emit_kernel(k_replace_emit<T>, A, w0, w1, dst, c.stream);
}

// A batch call's piece: its cnt records (d.count_res) merged with the separators in [done, own_hi) into d.replace_merged.  Which
// separators those are the host knows from its copy of the offsets, so the plan still gets its n by value.
int merge_separators(ReplaceCall &c, uint64_t base, uint64_t own_hi, const int32_t **recs, uint64_t *cnt) {
    uint32_t i1;
    separators_in(c.h_cat_off, c.n_hay, c.done, own_hi, &c.seps.i0, &i1);
    c.seps.n_sep = i1 - c.seps.i0;
    c.seps.base = (int64_t)base;
    if (!c.seps.n_sep) return ACGPU_OK;
    const uint64_t n = *cnt + c.seps.n_sep;
    const int rc = c.d.replace_merged.ensure(n * ACGPU_REC_MAP);
    if (rc) return rc;
    hipLaunchKernelGGL(k_replace_merge, dim3((unsigned)((n + kMergeBlock - 1) / kMergeBlock)), dim3(kMergeBlock), 0, c.stream, *recs, *cnt, c.seps,
                       c.sep_id, reinterpret_cast<int32_t *>(c.d.replace_merged.p));
    HIP_TRY(hipGetLastError());
    *recs = reinterpret_cast<const int32_t *>(c.d.replace_merged.p);
    *cnt = n;
    return ACGPU_OK;
}

// Behind a piece: plan its cnt records `recs` (relative to `base`; a batch call's: n_found records and the piece's separators),
// then emit [done, limit) of the text `hay` (the piece's buffer, whose unit 0 is the text's unit `base`).  A UTF-8 call: recs
// and hay are in bytes (base == 0), own_hi is in units still.
int replace_piece(ReplaceCall &c, const void *hay, uint64_t base, const int32_t *recs, uint64_t cnt, uint64_t n_found, uint64_t own_hi,
                  bool last_or_whole) {
    DeviceState &d = c.d;
    const int64_t done_rel = (int64_t)(c.done - base);
    int64_t delta = 0;
    uint64_t last_end = 0, bound = piece_bound(c.a->t, own_hi);
    // UTF-8: the boundary goes from units to bytes through the checkpoints (the last piece's limit is the text's end, and in an
    // all-ASCII text a unit is a byte); the byte rides with what the host reads behind the plan anyway
    // a batch's boundary always goes through the kernel: also in an all-ASCII batch a unit stands h separators behind its byte
    bool map_bound = !last_or_whole && (c.ub || (c.u8 && c.u8->d_ckpt));
    // a stream's feed whose right halo is empty (SHORTEST; LONGEST over one-unit keywords) ends its last piece at the buffer's
    // end, which is no unit of the text (utf8_map_position wants unit < n_units): its byte is the end of the decoded bytes
    if (map_bound && !c.ub && bound >= c.u8->n_units) {
        bound = c.u8->n_bytes;
        map_bound = false;
    }
    if (cnt || map_bound) {
        const uint32_t n_blocks = (uint32_t)((cnt + kPlanTile - 1) / kPlanTile);
        int rc = d.replace_plan.ensure((kPlanHead + (size_t)n_blocks + cnt) * 8); // {sum of the deltas, last end, boundary, -} | workgroup sums | pos
        if (rc) return rc;
        int64_t *slot = reinterpret_cast<int64_t *>(d.replace_plan.p), *bsum = slot + kPlanHead, *pos = bsum + n_blocks;
        if (cnt) {
            hipLaunchKernelGGL(k_replace_sums, dim3(n_blocks), dim3(kPlanBlock), 0, c.stream, recs, cnt, c.rt, bsum);
            hipLaunchKernelGGL(k_replace_offsets, dim3(1), dim3(kPlanBlock), 0, c.stream, bsum, n_blocks, recs, cnt, slot);
            hipLaunchKernelGGL(k_replace_plan, dim3(n_blocks), dim3(kPlanBlock), 0, c.stream, recs, cnt, c.rt, (const int64_t *)bsum, done_rel, pos);
            if (c.seps.n_sep) // (over the piece's own records: the same search that placed the separators)
                hipLaunchKernelGGL(k_replace_batch_offsets, dim3((c.seps.n_sep + kMergeBlock - 1) / kMergeBlock), dim3(kMergeBlock), 0, c.stream,
                                   reinterpret_cast<const int32_t *>(d.count_res.p), n_found, c.seps, (const int64_t *)pos, c.out_pos, c.d_out_off);
            HIP_TRY(hipGetLastError());
        }
        if (map_bound && (rc = utf8_map_position(*c.u8, c.ub, bound, slot + 2, c.stream))) return rc;
        // (a piece without records reads the boundary alone)
        const size_t first = cnt ? 0 : 2, words = (map_bound ? 3 : 2) - first;
        HIP_TRY(hipMemcpyAsync(static_cast<int64_t *>(d.replace_pin.h) + first, slot + first, words * 8, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream)); // the piece's output length decides the windows and the next piece's `done`
        const int64_t *h = static_cast<const int64_t *>(d.replace_pin.h);
        if (cnt) {
            delta = h[0];
            last_end = base + (uint64_t)h[1];
        }
        if (map_bound) bound = (uint64_t)h[2];
    }
    const uint64_t limit = std::min(c.n, replace_limit(last_or_whole, c.n, bound, last_end, c.done));
    const int64_t total_s = (int64_t)(limit - c.done) + delta;
    if (limit < c.done || total_s < 0) return ACGPU_E_HIP; // (records that overlap or are out of order: not a family this call serves)
    const uint64_t total = (uint64_t)total_s;
    if (c.ub) { // where the results of the haystacks that begin in [done, limit) begin: behind the plan, before the emit, no wait
        uint32_t j0, j1;
        span_boundaries(c.ub->h_boff.data(), c.n_hay, c.done, limit, last_or_whole, &j0, &j1);
        if (j1 > j0) {
            const int64_t *pos = cnt ? reinterpret_cast<const int64_t *>(d.replace_plan.p) + kPlanHead + (cnt + kPlanTile - 1) / kPlanTile : nullptr;
            hipLaunchKernelGGL(k_replace_span_offsets, dim3((j1 - j0 + kMergeBlock - 1) / kMergeBlock), dim3(kMergeBlock), 0, c.stream, recs, cnt, c.rt,
                               pos, c.ub->d_boff, j0, j1 - j0, done_rel, c.out_pos, c.d_out_off);
            HIP_TRY(hipGetLastError());
        }
    }
    // (hay, dst: elements of c.esz bytes)
    const int rc = emit_piece(d, c.stream, c.esz, c.d_out, c.h_out, c.cap, c.out_pos, total, [&](uint64_t w0, uint64_t w1, void *dst) {
        return c.esz == 1 ? launch_emit_as<uint8_t>(c, hay, recs, cnt, done_rel, w0, w1, dst)
                          : launch_emit_as<uint16_t>(c, hay, recs, cnt, done_rel, w0, w1, dst);
    });
    if (rc) return rc;
    c.done = limit;
    c.out_pos += total;
    c.st.n_records += n_found;
    return ACGPU_OK;
}

// The pieces of the owned units [own_begin, own_end) of the scan's text, behind c.done (set by the caller: the position up to
// which output exists).  last: the range's end is the text's end, so its last piece emits everything; else every piece emits
// up to replace_limit and c.done is where the next range's emit starts (a stream's feed, acgpu_stream.hip).  A whole text is
// (0, n, c.done = 0, last = true).  chain: the chain's entry; *chain_exit: its exit, if a piece was scanned.
int replace_pieces(ReplaceCall &c, int64_t chain, bool whole, const PieceScan &scan, uint64_t own_begin, uint64_t own_end, bool last = true,
                   int64_t *chain_exit = nullptr) {
    DeviceState &d = c.d;
    if (!d.replace_pin) HIP_TRY(hipHostMalloc(&d.replace_pin.h, 64, hipHostMallocDefault));
    int rc = emit_slabs_ready(d);
    if (rc) return rc;
    // (driven over the units the scan sees: a UTF-8 text's units, a UTF-8 batch's units and separators)
    PieceDriver p(own_begin, own_end, chain, whole, ACGPU_REC_MAP, &d.count_res); // the pool's reservoir of Map records (a counting call's too: one call at a time holds the pool)
    const void *hay = c.u8 ? (const void *)c.u8->d_bytes : scan.shard ? (const void *)scan.shard->d_hay : d.stage_hay.p;
    while (rc == ACGPU_OK && p.pos < p.end) {
        uint64_t cnt = 0, base = 0;
        if ((rc = scan_next_piece(p, scan, &cnt, &base))) break;
        if (!c.u8 && !scan.shard) hay = d.stage_hay.p; // (a host text's buffer may have grown under the piece)
        const int32_t *recs = reinterpret_cast<const int32_t *>(d.count_res.p);
        // UTF-8: the piece's records go from units to bytes where they lie (text relative: the shard is the whole text)
        // (a batch: span relative, and an all-ASCII one is mapped too)
        int32_t *own = reinterpret_cast<int32_t *>(d.count_res.p);
        if (c.u8 && (rc = utf8_map_records(*c.u8, c.ub, own, cnt, ACGPU_REC_MAP / 4, c.stream))) break;
        uint64_t n_list = cnt;
        if (c.h_cat_off && (rc = merge_separators(c, base, p.pos, &recs, &n_list))) break;
        rc = replace_piece(c, hay, base, recs, n_list, cnt, p.pos, last && p.pos >= p.end); // (a whole text's one piece ends at p.end)
    }
    // a stream's last feed that owns nothing new: what the feeds before it withheld, text without a record
    if (rc == ACGPU_OK && last && scan.shard && c.done < c.n) rc = replace_piece(c, hay, 0, reinterpret_cast<const int32_t *>(d.count_res.p), 0, 0, p.end, true);
    if (chain_exit && p.pieces) *chain_exit = p.chain;
    c.st.pieces += (uint32_t)p.pieces; // (added: a batch call haystack by haystack drives one text after the other)
    c.st.rescans += (uint32_t)p.rescans;
    c.st.units_out = c.out_pos;
    return rc;
}

// One host text through the pieces to its end: the body of acgpu_replace_u16, and of every haystack of a batch call that goes
// haystack by haystack -- c.cap, c.out_pos and the stats carry on from text to text, the table is uploaded once.
int replace_host_text(ReplaceCall &c, const uint16_t *hay, uint64_t n_units) {
    c.n = n_units;
    c.done = 0;
    const int rc = replace_pieces(c, 0, host_one_piece(c.a->t, ACGPU_REC_MAP), PieceScan{c.a, c.d, hay, n_units, nullptr, c.stream}, 0, n_units);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c.stream));
    return ACGPU_OK;
}

// what every entry returns behind its last piece
int replace_result(const ReplaceCall &c, uint64_t *n_out, acgpu_replace_stats *st) {
    if (st) *st = c.st;
    *n_out = c.out_pos;
    return c.out_pos > c.cap ? ACGPU_E_OVERFLOW : ACGPU_OK;
}

// the checks both entries share, none of which needs a device
int check_table(const acgpu_automaton *a, const void *repl_units, const uint64_t *repl_off, uint32_t n_repl) {
    if (n_repl != a->n_given && n_repl != 1) return ACGPU_E_INVALID;
    if (n_repl && !repl_off) return ACGPU_E_INVALID;
    for (uint32_t i = 0; i < n_repl; ++i)
        if (repl_off[i] > repl_off[i + 1]) return ACGPU_E_INVALID;
    const uint64_t total = n_repl ? repl_off[n_repl] - repl_off[0] : 0;
    if (total > (1ull << 31) || (total && !repl_units)) return ACGPU_E_INVALID;
    return a->t.mode == ACGPU_MODE_ALL ? ACGPU_E_UNSUPPORTED : ACGPU_OK; // (its records overlap)
}

} // namespace

namespace acgpu {

int replace_check_table(const acgpu_automaton *a, const void *repl, const uint64_t *repl_off, uint32_t n_repl) {
    return check_table(a, repl, repl_off, n_repl);
}

// One feed of a replace stream: the pieces of the buffer's owned range behind f->done, as a text's pieces are driven -- the
// table is uploaded per feed, so nothing of the stream stays on the device between two feeds.
int replace_feed(acgpu_automaton *a, DeviceState &d, ReplaceFeed *f, const void *repl, const uint64_t *repl_off, uint32_t n_repl, void *out,
                 uint64_t cap, uint64_t *n_out) {
    ReplaceCall c{a, d, d.call_stream};
    c.esz = f->u8 ? 1 : 2;
    c.u8 = f->u8;
    c.h_out = static_cast<uint8_t *>(out);
    c.cap = cap;
    c.n = f->u8 ? f->u8->n_bytes : f->shard.n_units;
    c.done = f->done;
    if (c.done > c.n) return ACGPU_E_HIP; // (never: the carry reaches back to `done`, the stream checks it)
    int rc = upload_table(c, repl, repl_off, n_repl);
    if (rc) return rc;
    const ShardRule rule = shard_rule(a->t, ACGPU_REC_MAP, /*readable=*/true);
    const int64_t entry = piece_entry(rule, f->chain, 0, f->shard.own_begin);
    int64_t chain_exit = piece_exit(rule, entry, f->shard.own_end, nullptr, 0); // (nothing owned: nothing scanned)
    acgpu_shard sh = f->shard;
    sh.chain_entry = entry;
    rc = replace_pieces(c, f->chain, rule.sequential, PieceScan{a, d, nullptr, 0, &sh, c.stream, /*readable=*/true}, sh.own_begin, sh.own_end, f->final,
                        &chain_exit);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c.stream));
    f->done = c.done;
    f->chain = chain_exit;
    f->st = c.st;
    *n_out = c.out_pos;
    return c.out_pos > c.cap ? ACGPU_E_OVERFLOW : ACGPU_OK;
}

} // namespace acgpu

extern "C" {

int acgpu_replace_u16(const acgpu_automaton *ca, const uint16_t *haystack, uint64_t n_units, const uint16_t *repl_units,
                      const uint64_t *repl_off, uint32_t n_repl, uint16_t *out, uint64_t cap, uint64_t *n_out, acgpu_replace_stats *st) {
    if (!ca || !n_out || (n_units && !haystack) || (cap && !out)) return ACGPU_E_INVALID;
    if (n_units >= (1ull << 31)) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    int rc = check_table(a, repl_units, repl_off, n_repl);
    if (rc) return rc;
    PoolCall call(a); // (no device: fails here, as acgpu_match_u16 does, and out is untouched)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    if ((rc = call.on(d.call_stream))) return rc;
    ReplaceCall c{a, d, d.call_stream};
    c.h_out = reinterpret_cast<uint8_t *>(out);
    c.cap = cap;
    if ((rc = upload_table(c, repl_units, repl_off, n_repl))) return rc;
    if ((rc = replace_host_text(c, haystack, n_units))) return call.fail(rc);
    return replace_result(c, n_out, st);
}

int acgpu_replace_device(const acgpu_automaton *ca, acgpu_shard *shard, const uint16_t *repl_units, const uint64_t *repl_off,
                         uint32_t n_repl, uint16_t *d_out, uint64_t cap, uint64_t *n_out, void *stream_, acgpu_replace_stats *st) {
    if (!ca || !shard || !n_out || (cap && !d_out) || ((uintptr_t)d_out & 15)) return ACGPU_E_INVALID;
    if (shard->n_units >= (1ull << 31) || (shard->n_units && !shard->d_hay) || ((uintptr_t)shard->d_hay & 15)) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    int rc = check_table(a, repl_units, repl_off, n_repl);
    if (rc) return rc;
    // one shard of a sharded text: its rewrite starts at the position up to which the rank before it has emitted -- not built
    if (!shard_is_whole_text(*shard)) return ACGPU_E_UNSUPPORTED;
    PoolCall call(a);
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    const hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if ((rc = call.on(stream))) return rc;
    ReplaceCall c{a, d, stream};
    c.d_out = reinterpret_cast<uint8_t *>(d_out);
    c.cap = cap;
    c.n = shard->n_units;
    if ((rc = upload_table(c, repl_units, repl_off, n_repl))) return rc;
    const bool whole = shard_rule(a->t, ACGPU_REC_MAP, false).sequential;
    rc = replace_pieces(c, shard->chain_entry, whole, PieceScan{a, d, nullptr, 0, shard, stream}, 0, shard->n_units);
    const hipError_t e = hipStreamSynchronize(stream); // the final wait
    if (rc) return rc;
    HIP_TRY(e);
    return replace_result(c, n_out, st);
}

} // extern "C"

namespace {

// The body of acgpu_replace_utf8 and acgpu_replace_utf8_lossy.  P (acgpu_host.h): how the text is staged, and the entry's stats.
// Lossy: the scan runs over the units of the text decoded with errors="replace", the records are mapped to bytes through the
// start bitmap, and plan and emit work on the caller's bytes as they lie on the device -- outside the matches the result is a
// copy of them, ill-formed ones included; a record that covers a replaced subpart removes the subpart's bytes.
template <class P>
int replace_utf8(const acgpu_automaton *ca, const uint8_t *bytes, uint64_t n_bytes, const uint8_t *repl_bytes, const uint64_t *repl_off,
                 uint32_t n_repl, uint8_t *out, uint64_t cap, uint64_t *n_out, acgpu_replace_stats *st, typename P::Stats *ust) {
    if (!ca || !n_out || (n_bytes && !bytes) || (cap && !out)) return ACGPU_E_INVALID;
    if (n_bytes >= (1ull << 31)) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    int rc = check_table(a, repl_bytes, repl_off, n_repl);
    if (rc) return rc;
    if (a->t.lone_surrogate) return ACGPU_E_UNSUPPORTED; // (a match inside a surrogate pair: records that overlap in bytes, see replace_limit)
    *n_out = 0;
    if (st) *st = acgpu_replace_stats{};
    if (ust) *ust = P::stats();
    if (n_bytes == 0) return ACGPU_OK; // (nothing to decode and nothing to rewrite: no device needed)
    PoolCall call(a); // (no device: fails here, as acgpu_match_utf8 does, and out is untouched)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    if ((rc = call.idle())) return rc; // (the NULL stream: see the stream rule)
    Utf8Text text;
    rc = stage_utf8_text(d, bytes, n_bytes, d.call_stream, &text, P::errors);
    if (ust) *ust = P::stats(&text, rc);
    if (rc == ACGPU_E_ENCODING) return rc; // (the stream is idle: the pool is as usable as before the call)
    if (rc) return call.fail(rc);
    ReplaceCall c{a, d, d.call_stream};
    c.esz = 1;
    c.u8 = &text;
    c.h_out = out;
    c.cap = cap;
    c.n = n_bytes;
    if ((rc = upload_table(c, repl_bytes, repl_off, n_repl))) return call.fail(rc);
    const bool whole = shard_rule(a->t, ACGPU_REC_MAP, false).sequential;
    if ((rc = replace_pieces(c, 0, whole, PieceScan{a, d, nullptr, 0, &text.shard, c.stream}, 0, text.shard.n_units))) return call.fail(rc);
    HIP_TRY(hipStreamSynchronize(c.stream));
    return replace_result(c, n_out, st);
}

// The body of acgpu_replace_batch_utf8 and acgpu_replace_batch_utf8_lossy
template <class P>
int replace_batch_utf8(const acgpu_automaton *ca, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                       const uint8_t *repl_bytes, const uint64_t *repl_off, uint32_t n_repl, uint8_t *out, uint64_t cap,
                       uint64_t *out_offsets, uint64_t *n_out, acgpu_replace_stats *st, typename P::Stats *ust) {
    if (!ca || !offsets || !n_out || !out_offsets || (cap && !out)) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    const HostTables &t = a->t;
    int rc = check_table(a, repl_bytes, repl_off, n_repl);
    if (rc) return rc;
    if (t.lone_surrogate) return ACGPU_E_UNSUPPORTED; // (as acgpu_replace_utf8)
    BatchPlan plan; // (in bytes: bytes >= units, so bytes + haystacks < 2^31 bounds the text the scan sees)
    if ((rc = check_batch(t, reinterpret_cast<const uint16_t *>(bytes), offsets, n_haystacks, &plan))) return rc;
    *n_out = 0;
    out_offsets[0] = 0;
    if (st) *st = acgpu_replace_stats{};
    if (ust) *ust = P::stats();
    if (plan.total == 0) { // (nothing to decode and nothing to rewrite: no device needed)
        for (uint32_t i = 0; i < n_haystacks; i++) out_offsets[i + 1] = 0;
        return ACGPU_OK;
    }
    PoolCall call(a); // (no device: fails here, and out is untouched)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    Utf8Batch b;
    if ((rc = utf8_batch_front<P>(call, t, bytes, offsets, n_haystacks, plan, &b, ust))) return rc; // (ACGPU_E_ENCODING: out_offsets[1..] untouched)
    ReplaceCall c{a, d, d.call_stream};
    c.esz = 1;
    c.h_out = out;
    c.cap = cap;
    if ((rc = upload_table(c, repl_bytes, repl_off, n_repl))) return call.fail(rc);
    const bool whole = shard_rule(t, ACGPU_REC_MAP, false).sequential; // (a device shard: as acgpu_replace_utf8 drives its pieces)
    if (plan.per_haystack) { // every haystack by the route acgpu_replace_utf8 takes, the results back to back
        rc = utf8_each_haystack<P>(
            d, bytes, offsets, n_haystacks, c.stream,
            [&](uint32_t i, const Utf8Text &text) {
                c.u8 = &text;
                c.n = offsets[i + 1] - offsets[i];
                c.done = 0;
                const int prc = replace_pieces(c, 0, whole, PieceScan{a, d, nullptr, 0, &text.shard, c.stream}, 0, text.shard.n_units);
                if (prc) return prc;
                return hipStreamSynchronize(c.stream) != hipSuccess ? (int)ACGPU_E_HIP : (int)ACGPU_OK; // (the next haystack is staged over this one)
            },
            [&](uint32_t i) { out_offsets[i + 1] = c.out_pos; });
        if (rc) return call.fail(rc);
        return replace_result(c, n_out, st);
    }
    if ((rc = d.replace_off.ensure(((size_t)n_haystacks + 1) * 8))) return call.fail(rc);
    c.u8 = &b.text;
    c.ub = &b;
    c.n = plan.total;
    c.n_hay = n_haystacks;
    c.d_out_off = reinterpret_cast<uint64_t *>(d.replace_off.p);
    {
        SeparatorScan sep(d, t);
        rc = replace_pieces(c, 0, whole, PieceScan{a, d, nullptr, 0, &b.text.shard, c.stream}, 0, b.text.shard.n_units);
    }
    if (rc) return call.fail(rc);
    // (every boundary was written by exactly one piece, boundary 0 -- offset 0 -- included)
    if (hipMemcpyAsync(out_offsets, c.d_out_off, ((size_t)n_haystacks + 1) * 8, hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
        hipStreamSynchronize(c.stream) != hipSuccess)
        return call.fail(ACGPU_E_HIP);
    return replace_result(c, n_out, st);
}

} // namespace

extern "C" {

int acgpu_replace_utf8(const acgpu_automaton *a, const uint8_t *bytes, uint64_t n_bytes, const uint8_t *repl_bytes, const uint64_t *repl_off,
                       uint32_t n_repl, uint8_t *out, uint64_t cap, uint64_t *n_out, acgpu_replace_stats *st, acgpu_utf8_stats *ust) {
    return replace_utf8<Utf8StrictText>(a, bytes, n_bytes, repl_bytes, repl_off, n_repl, out, cap, n_out, st, ust);
}

int acgpu_replace_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, uint64_t n_bytes, const uint8_t *repl_bytes, const uint64_t *repl_off,
                             uint32_t n_repl, uint8_t *out, uint64_t cap, uint64_t *n_out, acgpu_replace_stats *st, acgpu_utf8_lossy_stats *ust) {
    return replace_utf8<Utf8LossyText>(a, bytes, n_bytes, repl_bytes, repl_off, n_repl, out, cap, n_out, st, ust);
}

int acgpu_replace_batch_utf8(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                             const uint8_t *repl_bytes, const uint64_t *repl_off, uint32_t n_repl, uint8_t *out, uint64_t cap,
                             uint64_t *out_offsets, uint64_t *n_out, acgpu_replace_stats *st, acgpu_utf8_batch_stats *ust) {
    return replace_batch_utf8<Utf8StrictBatch>(a, bytes, offsets, n_haystacks, repl_bytes, repl_off, n_repl, out, cap, out_offsets, n_out, st, ust);
}

int acgpu_replace_batch_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                                   const uint8_t *repl_bytes, const uint64_t *repl_off, uint32_t n_repl, uint8_t *out, uint64_t cap,
                                   uint64_t *out_offsets, uint64_t *n_out, acgpu_replace_stats *st, acgpu_utf8_lossy_stats *ust) {
    return replace_batch_utf8<Utf8LossyBatch>(a, bytes, offsets, n_haystacks, repl_bytes, repl_off, n_repl, out, cap, out_offsets, n_out, st, ust);
}

int acgpu_replace_batch_u16(const acgpu_automaton *ca, const uint16_t *units, const uint64_t *offsets, uint32_t n_haystacks,
                            const uint16_t *repl_units, const uint64_t *repl_off, uint32_t n_repl, uint16_t *out, uint64_t cap,
                            uint64_t *out_offsets, uint64_t *n_out, acgpu_replace_stats *st) {
    if (!ca || !offsets || !n_out || !out_offsets || (cap && !out)) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    int rc = check_table(a, repl_units, repl_off, n_repl);
    if (rc) return rc;
    *n_out = 0;
    out_offsets[0] = 0;
    if (st) *st = acgpu_replace_stats{};
    if (n_haystacks == 0) return ACGPU_OK;
    const HostTables &t = a->t;
    BatchPlan plan;
    if ((rc = check_batch(t, units, offsets, n_haystacks, &plan))) return rc;
    PoolCall call(a); // (no device: fails here, and out is untouched)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    ReplaceCall c{a, d, d.call_stream};
    c.h_out = reinterpret_cast<uint8_t *>(out);
    c.cap = cap;
    if (plan.per_haystack) { // every haystack as a text of its own, the results back to back
        if ((rc = call.on(c.stream))) return rc; // (what acgpu_replace_u16 asks)
        if ((rc = upload_table(c, repl_units, repl_off, n_repl))) return rc;
        for (uint32_t i = 0; i < n_haystacks; i++) {
            const uint64_t len = offsets[i + 1] - offsets[i];
            if ((rc = replace_host_text(c, len ? units + offsets[i] : nullptr, len))) return call.fail(rc);
            out_offsets[i + 1] = c.out_pos;
        }
        return replace_result(c, n_out, st);
    }
    if ((rc = call.idle())) return rc; // (the NULL stream: see the stream rule)
    BatchText text(d, t);
    if ((rc = text.stage(units, offsets, n_haystacks, c.stream))) return rc;
    if ((rc = d.replace_off.ensure(((size_t)n_haystacks + 1) * 8))) return rc;
    c.n = text.cat;
    c.h_cat_off = text.h_off;
    c.n_hay = n_haystacks;
    c.seps.cat_off = text.d_off();
    c.sep_id = (int32_t)a->n_given;
    c.d_out_off = reinterpret_cast<uint64_t *>(d.replace_off.p);
    if ((rc = upload_table(c, repl_units, repl_off, n_repl, /*full=*/true))) return rc;
    rc = replace_pieces(c, 0, host_one_piece(t, ACGPU_REC_MAP), PieceScan{a, d, text.h_cat, text.cat, nullptr, c.stream}, 0, text.cat);
    if (rc) return call.fail(rc);
    HIP_TRY(hipMemcpyAsync(out_offsets + 1, c.d_out_off + 1, (size_t)n_haystacks * 8, hipMemcpyDeviceToHost, d.call_stream)); // (every separator was merged once)
    HIP_TRY(hipStreamSynchronize(d.call_stream));
    return replace_result(c, n_out, st);
}

} // extern "C"
