// acgpu_spans.hip -- acgpu_spans_u16 / acgpu_spans_batch_u16 / acgpu_spans_device / acgpu_spans_utf8 / acgpu_spans_utf8_lossy /
// acgpu_spans_batch_utf8 / acgpu_spans_batch_utf8_lossy (include/acgpu.h): the
// records of a text merged into its covered runs, on the device, for all five families.
//
// A spans call is the sixth consumer of the piece driver (scan_next_piece, acgpu_pieces.hip): the Set records of a piece stay in
// the pool's reservoir, and behind every piece the MERGE reduces a list of m intervals -- the spans the piece before withheld (the
// carry, text coordinates) and then the piece's records (relative to the piece's `base`, which interval() adds) -- to spans.
//
// The list is sorted by end, not descending (ALL: end ascending, longest first; the other families: disjoint, in position order;
// the carry ends at or before the owned range of the piece, the piece's records behind it).  With
//   X_i = min(start_j : j > i)         the exclusive suffix minimum of the starts (nothing behind i: +infinity)
//   M_i = min(start_i, X_i)
// interval i CLOSES a span iff i == m - 1 or X_i > end_i, and it is the HEAD of one iff i == 0 or interval i - 1 closes, i.e.
// M_i > end_{i-1}.  The span of head i starts at M_i: a later interval of the same run has start < end <= end_b < M_{b+1}, b the
// run's last interval, so M_i is the minimum over the run alone.  It ends at the end of the interval that closes it, the largest
// of the run because the ends ascend.  Touching intervals (start == an earlier end) do not close: X_i > end_i is strict.
// The span's index is the number of closing intervals in front of its head -- which is also the number in front of its closing
// interval -- so one exclusive prefix count serves both writes.  Five launches on the call's stream, no atomics, no flags:
//   k_span_mins      a workgroup per tile of kSpanTile intervals: the tile's smallest start
//   k_span_scan_mins ONE workgroup: the tiles' minima become exclusive suffix minima, in place
//   k_span_counts    per tile: its closing intervals, and those of them whose span is final
//   k_span_offsets   ONE workgroup: the tiles' counts become exclusive prefix counts, in place; {n_final, n_carry} for the host
//   k_span_scatter   per tile again: recomputes X_i and the closing flags, the head writes start, the closing interval writes end
//
// THE CARRY.  Behind a piece that owned [.., own_hi) the host knows `bound`, a position no record of a later piece starts before:
// own_hi for the families whose match belongs to the piece that owns its FIRST unit (LONGEST, WHOLEWORD, WWLONGEST), and
// own_hi + 1 - max_len for those where it belongs to the piece that owns its LAST unit (ALL, SHORTEST: a later record ends behind
// own_hi and has at most max_len units).  For the first-unit families a later record also starts at or behind every earlier
// record's end, so the kernels take B = max(bound, end of the list's last interval); for the others B = bound.  A span is FINAL iff
// end < B: no later record overlaps or touches it.  The ends of the spans ascend, so the final spans are a prefix of the piece's
// spans: span k < n_final goes to the output, span k >= n_final to the carry buffer (two of them, read and written in turn), in
// text coordinates.  Carried spans are disjoint, do not touch and end in [B, own_hi], so there are at most max_len / 2 + 2 of
// them (one for the first-unit families); the buffer has that size and a count beyond it is ACGPU_E_HIP.  The last piece, and a
// text scanned as one piece, finalise everything.  The host reads 16 bytes per piece, {n_final, n_carry}: one wait beside the
// scan's own.
//
// A SECOND CALLER.  The cover entries (acgpu_cover.hip) run the same piece loop and merge through acgpu_spans.h (spans_pieces):
// SpansCall::to_pool sends a piece's spans to d.cover_spans instead of the caller, k_span_settled adds the position up to which the
// text is settled, SpansCall::planned enqueues the caller's plan in front of the wait -- which then reads the whole head, 56 bytes,
// still once -- and SpansCall::merged is the caller's step behind it, the piece's emit.  What the spans entries compute, read back
// and return is untouched by that.
//
// A RANGE (SpansRange, acgpu_spans.h; the feed of a cover stream): the same loop over the owned units of a buffer [carry | chunk].
// The first piece's carry is uploaded from the host, the range's last piece finalises everything only if the caller says the
// range ends the text -- otherwise it is a piece like any other, after which the caller reads B and the first withheld span from
// the head (kSpanBelow, kSpanCarry0) -- and what it withholds goes back to the host.  Carried spans may start in front of the
// buffer: starts are only compared.
//
// A BATCH (acgpu_spans_batch_u16): the haystacks are merged as one text, a separator unit behind each.  No record holds a
// separator, so a separator's position is never covered, and a span that ends at it and one that starts behind it do not touch:
// the merge is unchanged and its spans are the haystacks' spans, shifted.  Behind the piece's wait k_span_tag turns the piece's final
// spans into {haystack, start, end} relative to the haystack, and 12 bytes per span leave for the caller.
//
// UTF-8: the text is staged by stage_utf8_text and scanned in units; a piece's records become byte offsets where they lie
// (utf8_map_records, two words per record) BEFORE the merge -- the map is monotone, so the order by end survives -- and `bound`
// goes through utf8_map_position, rounded down, into the slot the kernels read it from.  Keywords with an unpaired surrogate are
// served: their widened records may overlap in bytes, which a merge does not mind.
//
// A BATCH OF UTF-8 TEXTS (acgpu_spans_batch_utf8): the scan's text has a separator unit behind every haystack, the caller's bytes
// have none, and the records of a lone-surrogate keyword may touch in bytes only -- so the merge runs over VIRTUAL COORDINATES,
// v = byte of the buffer + index of the haystack: the bytes with one phantom element behind every haystack, which no record
// covers.  A piece's records become v where they lie (utf8_vmap_records), `bound` becomes a v (utf8_vmap_position), and with
// voff in the place of cat_off merge, carry and k_span_tag run as for a UTF-16 batch.  The entry's front and its
// route haystack by haystack are utf8_batch_front and utf8_each_haystack (acgpu_host.h), shared with the cover and replace entries.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "acgpu_device.h"
#include "acgpu_host.h"
#include "acgpu_internal.h"
#include "acgpu_spans.h"

using namespace acgpu;

namespace {

constexpr int kSpanBlock = 256, kSpanPer = 8, kSpanTile = kSpanBlock * kSpanPer; // intervals per workgroup: a thread takes kSpanPer consecutive ones
constexpr int32_t kNoStart = INT_MAX;

// The list a piece merges: n_carry spans in text coordinates, then the piece's records, relative to `base`.
struct SpanList {
    const int2 *carry;
    const int2 *recs;
    uint64_t m; // intervals in all
    uint32_t n_carry;
    int32_t base;
};

__device__ __forceinline__ int2 interval(const SpanList &L, uint64_t i) {
    if (i < L.n_carry) return L.carry[i];
    int2 r = L.recs[i - L.n_carry];
    r.x += L.base;
    r.y += L.base;
    return r;
}

// What decides which spans are final (see THE CARRY)
struct SpanBound {
    const int64_t *d_bound; // the bound where the device has it (a UTF-8 text's, in bytes), or nullptr: `bound`
    int64_t bound;
    int32_t first_unit; // a match belongs to the piece that owns its first unit
    int32_t last;       // the last piece, or the text as one piece: every span is final
};

__device__ __forceinline__ int64_t final_below(const SpanList &L, const SpanBound &Bd) {
    if (Bd.last) return LLONG_MAX;
    int64_t b = Bd.d_bound ? *Bd.d_bound : Bd.bound;
    if (Bd.first_unit && L.m) b = std::max<int64_t>(b, interval(L, L.m - 1).y);
    return b;
}

// the minimum of v over the threads BEHIND this one (none: kNoStart), *total = over all; kSpanBlock threads
__device__ __forceinline__ int32_t block_suffix_min(int32_t v, int32_t *total) {
    __shared__ int32_t wmin[kSpanBlock / kWave];
    int32_t inc = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int32_t o = __shfl_down(inc, d);
        if ((int)lane_id() + d < kWave) inc = std::min(inc, o);
    }
    const int32_t behind = __shfl_down(inc, 1);
    const int w = threadIdx.x / kWave;
    if (lane_id() == 0) wmin[w] = inc;
    __syncthreads();
    int32_t ex = lane_id() == kWave - 1 ? kNoStart : behind, all = kNoStart;
    for (int i = 0; i < kSpanBlock / kWave; ++i) {
        if (i > w) ex = std::min(ex, wmin[i]);
        all = std::min(all, wmin[i]);
    }
    *total = all;
    __syncthreads();
    return ex;
}

// the sum of v over the threads IN FRONT of this one, *total = over all; kSpanBlock threads
__device__ __forceinline__ uint32_t block_prefix_sum(uint32_t v, uint32_t *total) {
    __shared__ uint32_t wsum[kSpanBlock / kWave];
    const uint32_t inc = wave_inclusive_scan(v);
    const int w = threadIdx.x / kWave;
    if (lane_id() == kWave - 1) wsum[w] = inc;
    __syncthreads();
    uint32_t base = 0, all = 0;
    for (int i = 0; i < kSpanBlock / kWave; ++i) {
        if (i < w) base += wsum[i];
        all += wsum[i];
    }
    *total = all;
    __syncthreads();
    return base + inc - v;
}

// A thread's kSpanPer intervals (s = kNoStart behind the list's end) and, from the tile's scan, x[k] = X_i of each.
struct SpanLane {
    int32_t s[kSpanPer], e[kSpanPer], x[kSpanPer];
};

// tile_behind: the smallest start of the tiles behind this one
__device__ __forceinline__ void load_lane(const SpanList &L, uint64_t first, int32_t tile_behind, SpanLane &t) {
    int32_t v = kNoStart;
#pragma unroll
    for (int k = 0; k < kSpanPer; ++k) {
        t.s[k] = kNoStart;
        t.e[k] = 0;
        if (first + k < L.m) {
            const int2 r = interval(L, first + k);
            t.s[k] = r.x;
            t.e[k] = r.y;
        }
        v = std::min(v, t.s[k]);
    }
    int32_t total;
    int32_t run = std::min(block_suffix_min(v, &total), tile_behind);
#pragma unroll
    for (int k = kSpanPer - 1; k >= 0; --k) {
        t.x[k] = run;
        run = std::min(run, t.s[k]);
    }
}

__device__ __forceinline__ bool closes(const SpanList &L, const SpanLane &t, uint64_t first, int k) {
    return first + k < L.m && (first + k == L.m - 1 || t.x[k] > t.e[k]);
}

// merge, level 1 of the suffix minimum: every tile's smallest start
__global__ __launch_bounds__(kSpanBlock) void k_span_mins(SpanList L, int32_t *__restrict__ tmin) {
    const uint64_t first = (uint64_t)blockIdx.x * kSpanTile + (uint64_t)threadIdx.x * kSpanPer;
    int32_t v = kNoStart;
    for (int k = 0; k < kSpanPer; ++k)
        if (first + k < L.m) v = std::min(v, interval(L, first + k).x);
    int32_t total;
    block_suffix_min(v, &total);
    if (threadIdx.x == 0) tmin[blockIdx.x] = total;
}

// level 2: ONE workgroup turns the tiles' minima into exclusive suffix minima in place, kSpanBlock per step from the back with a
// running carry
__global__ __launch_bounds__(kSpanBlock) void k_span_scan_mins(int32_t *__restrict__ tmin, uint32_t n_tiles) {
    int32_t carry = kNoStart;
    for (uint32_t c = (n_tiles + kSpanBlock - 1) / kSpanBlock; c-- > 0;) {
        const uint32_t b = c * kSpanBlock + threadIdx.x;
        const int32_t v = b < n_tiles ? tmin[b] : kNoStart;
        int32_t total;
        const int32_t ex = block_suffix_min(v, &total);
        if (b < n_tiles) tmin[b] = std::min(carry, ex);
        carry = std::min(carry, total);
    }
}

// level 1 of the count: every tile's closing intervals, and those whose span is final
__global__ __launch_bounds__(kSpanBlock) void k_span_counts(SpanList L, SpanBound Bd, const int32_t *__restrict__ tmin, uint32_t *__restrict__ tcnt,
                                                            uint32_t *__restrict__ tfin) {
    const uint64_t first = (uint64_t)blockIdx.x * kSpanTile + (uint64_t)threadIdx.x * kSpanPer;
    const int64_t B = final_below(L, Bd);
    SpanLane t;
    load_lane(L, first, tmin[blockIdx.x], t);
    uint32_t n = 0, nf = 0;
#pragma unroll
    for (int k = 0; k < kSpanPer; ++k)
        if (closes(L, t, first, k)) {
            n++;
            nf += (int64_t)t.e[k] < B;
        }
    uint32_t total, total_f;
    block_prefix_sum(n, &total);
    block_prefix_sum(nf, &total_f);
    if (threadIdx.x == 0) {
        tcnt[blockIdx.x] = total;
        tfin[blockIdx.x] = total_f;
    }
}

// level 2: ONE workgroup turns the tiles' counts into exclusive prefix counts in place and adds the final ones up;
// slot[0] = the final spans, slot[1] = the spans to carry
__global__ __launch_bounds__(kSpanBlock) void k_span_offsets(uint32_t *__restrict__ tcnt, const uint32_t *__restrict__ tfin, uint32_t n_tiles,
                                                             uint64_t *__restrict__ slot) {
    uint64_t carry = 0, fin = 0;
    for (uint32_t b0 = 0; b0 < n_tiles; b0 += kSpanBlock) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < n_tiles ? tcnt[b] : 0, f = b < n_tiles ? tfin[b] : 0;
        uint32_t total, total_f;
        const uint32_t ex = block_prefix_sum(v, &total);
        block_prefix_sum(f, &total_f);
        if (b < n_tiles) tcnt[b] = (uint32_t)carry + ex; // (a piece has fewer than 2^32 records)
        carry += total;
        fin += total_f;
    }
    if (threadIdx.x == 0) {
        slot[0] = fin;
        slot[1] = carry - fin;
    }
}

// Where the spans go: span k < n_final to out[out_first + k] if k < room, span k >= n_final to carry[k - n_final] if that is below
// carry_cap (the host refuses the call if it was not).
struct SpanOut {
    int2 *out;
    uint64_t out_first, room;
    int2 *carry;
    uint32_t carry_cap;
};

__device__ __forceinline__ int32_t *span_slot(const SpanOut &O, uint64_t k, uint64_t n_final) {
    if (k < n_final) return k < O.room ? reinterpret_cast<int32_t *>(O.out + O.out_first + k) : nullptr;
    return k - n_final < O.carry_cap ? reinterpret_cast<int32_t *>(O.carry + (k - n_final)) : nullptr;
}

// level 3: per interval again -- the head of span k writes its start, the interval that closes it its end
__global__ __launch_bounds__(kSpanBlock) void k_span_scatter(SpanList L, const int32_t *__restrict__ tmin, const uint32_t *__restrict__ toff,
                                                             const uint64_t *__restrict__ slot, SpanOut O) {
    const uint64_t first = (uint64_t)blockIdx.x * kSpanTile + (uint64_t)threadIdx.x * kSpanPer;
    const uint64_t n_final = slot[0];
    SpanLane t;
    load_lane(L, first, tmin[blockIdx.x], t);
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < kSpanPer; ++k) n += closes(L, t, first, k);
    uint32_t total;
    uint64_t idx = (uint64_t)toff[blockIdx.x] + block_prefix_sum(n, &total);
    if (first >= L.m) return;
    int32_t prev_end = first ? interval(L, first - 1).y : 0;
#pragma unroll
    for (int k = 0; k < kSpanPer; ++k) {
        if (first + k >= L.m) break;
        const int32_t M = std::min(t.s[k], t.x[k]);
        if (first + k == 0 || M > prev_end) { // the head: interval i - 1 closed
            int32_t *p = span_slot(O, idx, n_final);
            if (p) p[0] = M;
        }
        if (closes(L, t, first, k)) {
            int32_t *p = span_slot(O, idx, n_final);
            if (p) p[1] = t.e[k];
            ++idx;
        }
        prev_end = t.e[k];
    }
}

// A cover call (acgpu_cover.hip), behind the scatter: the settled position L = min(B, start of the first carried span) -- every
// position below it is inside a final span or will never be covered -- into slot[kSpanSettled]; one thread.  empty: a piece
// without intervals, whose other launches did not run.
// slot[kSpanBelow] = B itself and slot[kSpanCarry0] = the first carried span, {start, end}: what the last piece of a RANGE (a cover
// stream's feed, acgpu_spans.h) settles at instead, and the span it cuts there.
__global__ void k_span_settled(SpanList L, SpanBound Bd, const int2 *__restrict__ carry_out, uint64_t *__restrict__ slot, int empty) {
    if (empty) slot[0] = slot[1] = slot[kSpanDropped] = 0;
    const int64_t below = final_below(L, Bd);
    int64_t at = below;
    int2 first = make_int2(0, 0);
    if (slot[1]) {
        first = carry_out[0];
        at = std::min<int64_t>(at, first.x);
    }
    slot[kSpanSettled] = (uint64_t)at;
    slot[kSpanBelow] = (uint64_t)below;
    slot[kSpanCarry0] = (uint64_t)(uint32_t)first.x | ((uint64_t)(uint32_t)first.y << 32);
}

// A batch call's final spans of a piece -> {haystack, start, end} relative to the haystack: the layout of k_batch_tag's Set
// records.  cat_off == nullptr: the text is haystack `tag`, whose spans are relative to it already.
__global__ __launch_bounds__(kSpanBlock) void k_span_tag(const int2 *__restrict__ spans, uint64_t n, const uint32_t *__restrict__ cat_off, uint32_t n_hay,
                                                         int32_t tag, int32_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kSpanBlock + threadIdx.x;
    if (i >= n) return;
    const int2 sp = spans[i];
    int32_t h = tag, base = 0;
    if (cat_off) {
        uint32_t lo = 0, hi = n_hay; // the last haystack that begins at or before the span's start
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (cat_off[mid] <= (uint32_t)sp.x) lo = mid;
            else hi = mid;
        }
        h = (int32_t)lo;
        base = (int32_t)cat_off[lo];
    }
    out[3 * i] = h;
    out[3 * i + 1] = sp.x - base;
    out[3 * i + 2] = sp.y - base;
}

bool first_unit_family(const HostTables &t) { return t.mode != ACGPU_MODE_ALL && t.mode != ACGPU_MODE_SHORTEST; }

// `bound` of THE CARRY, in the scan's units: piece_bound of the replace entries, with ALL on SHORTEST's side
uint64_t spans_bound(const HostTables &t, uint64_t own_hi) {
    if (first_unit_family(t)) return own_hi;
    const uint64_t back = t.max_len ? t.max_len - 1 : 0;
    return own_hi > back ? own_hi - back : 0;
}

// before the first piece: the pinned words and the two carry buffers
// (a range: the spans an earlier range withheld are the first piece's carry)
int spans_begin(SpansCall &c, const SpansRange *range) {
    DeviceState &d = c.d;
    static_assert(kSpanHead * 8 <= 64, "the head fits the pinned words");
    if (!d.spans_pin) HIP_TRY(hipHostMalloc(&d.spans_pin.h, 64, hipHostMallocDefault));
    c.carry_cap = c.a->t.max_len / 2 + 2;
    const int rc = d.spans_carry.ensure((size_t)c.carry_cap * 2 * 8);
    if (rc || !range || !range->n_carry_in) return rc;
    if (range->n_carry_in > c.carry_cap) return ACGPU_E_HIP; // (never: what a range hands back fits)
    HIP_TRY(hipMemcpyAsync(reinterpret_cast<int2 *>(d.spans_carry.p) + (size_t)c.cur * c.carry_cap, range->carry_in, (size_t)range->n_carry_in * 8,
                           hipMemcpyHostToDevice, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream)); // (the caller's memory is pageable)
    c.n_carry = range->n_carry_in;
    return ACGPU_OK;
}

// Behind a piece: merge the carry and the piece's cnt records (in d.count_res, relative to `base`; a UTF-8 call's: in bytes).
// range_last: the last piece of a range whose end is not the text's (acgpu_spans.h).
int spans_piece(SpansCall &c, uint64_t base, uint64_t cnt, uint64_t own_hi, bool last_or_whole, bool range_last = false) {
    DeviceState &d = c.d;
    c.st.n_records += cnt;
    const uint64_t m = c.n_carry + cnt;
    c.piece_final = c.piece_dropped = 0;
    c.piece_own_hi = own_hi;
    c.piece_last = last_or_whole;
    c.piece_range_last = range_last;
    c.piece_carried = 0;
    if (!m && !c.to_pool) return ACGPU_OK;
    const uint32_t n_tiles = (uint32_t)((m + kSpanTile - 1) / kSpanTile);
    int rc = d.spans_work.ensure(kSpanHead * 8 + (size_t)n_tiles * 12); // the head (acgpu_spans.h) | tile minima | tile counts | tile final counts
    if (rc) return rc;
    uint64_t *slot = reinterpret_cast<uint64_t *>(d.spans_work.p);
    int32_t *tmin = reinterpret_cast<int32_t *>(slot + kSpanHead);
    uint32_t *tcnt = reinterpret_cast<uint32_t *>(tmin + n_tiles), *tfin = tcnt + n_tiles;
    int2 *carry = reinterpret_cast<int2 *>(d.spans_carry.p);

    SpanList L;
    L.carry = carry + (size_t)c.cur * c.carry_cap;
    L.recs = reinterpret_cast<const int2 *>(d.count_res.p);
    L.m = m;
    L.n_carry = c.n_carry;
    L.base = (int32_t)base;

    SpanBound Bd;
    Bd.d_bound = nullptr;
    Bd.first_unit = first_unit_family(c.a->t);
    Bd.last = last_or_whole;
    uint64_t bound = spans_bound(c.a->t, own_hi);
    // UTF-8: the bound goes from units to bytes through the checkpoints, rounded down, and stays on the device (an all-ASCII
    // text: a unit is a byte; a bound at the text's end: the text's bytes)
    if (c.ub) { // a batch in virtual coordinates: a unit of an all-ASCII batch's shard is its v; else the device maps it, a separator to its phantom
        if (!last_or_whole && c.u8->d_ckpt) {
            if ((rc = utf8_vmap_position(*c.ub, bound, reinterpret_cast<int64_t *>(slot + 2), c.stream))) return rc;
            Bd.d_bound = reinterpret_cast<const int64_t *>(slot + 2);
        }
    } else if (!last_or_whole && c.u8 && c.u8->d_ckpt) {
        if (bound >= c.u8->n_units) {
            bound = c.u8->n_bytes;
        } else {
            if ((rc = utf8_map_position(*c.u8, nullptr, bound, reinterpret_cast<int64_t *>(slot + 2), c.stream))) return rc;
            Bd.d_bound = reinterpret_cast<const int64_t *>(slot + 2);
        }
    }
    Bd.bound = (int64_t)bound;

    SpanOut O;
    const uint64_t room = c.cap > c.out_pos ? c.cap - c.out_pos : 0;
    if (c.to_pool) { // every span of the piece has a slot: the plan and the emit read the final ones from there
        if ((rc = d.cover_spans.ensure((size_t)m * 8 + 16))) return rc;
        O.out = reinterpret_cast<int2 *>(d.cover_spans.p);
        O.out_first = 0;
        O.room = m;
    } else if (c.d_out) {
        O.out = reinterpret_cast<int2 *>(c.d_out);
        O.out_first = c.out_pos;
        O.room = room;
    } else {
        if ((rc = d.spans_out.ensure((size_t)std::min(m, room) * 8 + 8))) return rc;
        O.out = reinterpret_cast<int2 *>(d.spans_out.p);
        O.out_first = 0;
        O.room = std::min(m, room);
    }
    O.carry = carry + (size_t)(c.cur ^ 1) * c.carry_cap;
    O.carry_cap = c.carry_cap;
    if (!m) { // (a cover call's piece without intervals: its settled position is the bound)
        c.piece_settled = c.piece_below = (int64_t)bound;
        if (!Bd.d_bound) return ACGPU_OK;
        hipLaunchKernelGGL(k_span_settled, dim3(1), dim3(1), 0, c.stream, L, Bd, (const int2 *)O.carry, slot, 1);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(d.spans_pin.h, slot, kSpanHead * 8, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        c.piece_settled = c.piece_below = (int64_t) static_cast<const uint64_t *>(d.spans_pin.h)[kSpanSettled];
        return ACGPU_OK;
    }

    hipLaunchKernelGGL(k_span_mins, dim3(n_tiles), dim3(kSpanBlock), 0, c.stream, L, tmin);
    hipLaunchKernelGGL(k_span_scan_mins, dim3(1), dim3(kSpanBlock), 0, c.stream, tmin, n_tiles);
    hipLaunchKernelGGL(k_span_counts, dim3(n_tiles), dim3(kSpanBlock), 0, c.stream, L, Bd, (const int32_t *)tmin, tcnt, tfin);
    hipLaunchKernelGGL(k_span_offsets, dim3(1), dim3(kSpanBlock), 0, c.stream, tcnt, (const uint32_t *)tfin, n_tiles, slot);
    hipLaunchKernelGGL(k_span_scatter, dim3(n_tiles), dim3(kSpanBlock), 0, c.stream, L, (const int32_t *)tmin, (const uint32_t *)tcnt,
                       (const uint64_t *)slot, O);
    if (c.to_pool && !last_or_whole)
        hipLaunchKernelGGL(k_span_settled, dim3(1), dim3(1), 0, c.stream, L, Bd, (const int2 *)O.carry, slot, 0);
    HIP_TRY(hipGetLastError());
    if (c.planned && (rc = c.planned(c.ctx, slot, O.out, m))) return rc;
    HIP_TRY(hipMemcpyAsync(d.spans_pin.h, slot, c.to_pool ? kSpanHead * 8 : 16, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream)); // how many spans left for the output decides out_pos and the next piece's list
    const uint64_t *h = static_cast<const uint64_t *>(d.spans_pin.h);
    const uint64_t n_final = h[0], n_carry = h[1];
    if (n_carry > c.carry_cap || (last_or_whole && n_carry)) return ACGPU_E_HIP; // (never: see THE CARRY)
    if (c.h_out && n_final && room) { // (the next piece's scatter follows it on the stream; the call waits for the stream at its end)
        const uint64_t n_put = std::min(n_final, room);
        if (c.cat_off || c.tag_all) { // a batch call: tagged and rebased in the pool, then 12 bytes per span
            if ((rc = d.batch_out.ensure((size_t)n_put * 12 + 16))) return rc;
            hipLaunchKernelGGL(k_span_tag, dim3((unsigned)((n_put + kSpanBlock - 1) / kSpanBlock)), dim3(kSpanBlock), 0, c.stream, (const int2 *)O.out, n_put,
                               c.cat_off, c.n_hay, c.tag, reinterpret_cast<int32_t *>(d.batch_out.p));
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(c.h_out + 3 * c.out_pos, d.batch_out.p, (size_t)n_put * 12, hipMemcpyDeviceToHost, c.stream));
        } else {
            HIP_TRY(hipMemcpyAsync(c.h_out + 2 * c.out_pos, O.out, (size_t)n_put * 8, hipMemcpyDeviceToHost, c.stream));
        }
    }
    c.out_pos += n_final;
    c.n_carry = (uint32_t)n_carry;
    c.cur ^= 1;
    c.st.max_carry = std::max(c.st.max_carry, (uint32_t)n_carry);
    c.piece_final = n_final;
    c.piece_settled = (int64_t)h[kSpanSettled];
    c.piece_dropped = h[kSpanDropped];
    c.piece_below = (int64_t)h[kSpanBelow];
    c.piece_carry0 = make_int2((int32_t)(uint32_t)h[kSpanCarry0], (int32_t)(uint32_t)(h[kSpanCarry0] >> 32));
    c.piece_carried = (uint32_t)n_carry;
    return ACGPU_OK;
}

} // namespace

namespace acgpu {

int spans_pieces(SpansCall &c, int64_t chain, bool whole, const PieceScan &scan, uint64_t n_units, SpansRange *range) {
    DeviceState &d = c.d;
    int rc = spans_begin(c, range);
    if (rc) return rc;
    const bool text_end = !range || range->text_end;
    // the pool's reservoir, here of Set records: one call at a time holds the pool
    PieceDriver p(range ? range->own_begin : 0, range ? range->own_end : n_units, chain, whole, ACGPU_REC_SET, &d.count_res);
    while (p.pos < p.end) {
        uint64_t cnt = 0, base = 0;
        if ((rc = scan_next_piece(p, scan, &cnt, &base))) return rc;
        // UTF-8: the piece's records go from units to bytes where they lie (text relative: the shard is the whole text)
        // (a batch of them: to virtual coordinates, the haystack's index added)
        int32_t *recs = reinterpret_cast<int32_t *>(d.count_res.p);
        if (c.ub) rc = utf8_vmap_records(*c.ub, recs, cnt, c.stream);
        else if (c.u8) rc = utf8_map_records(*c.u8, nullptr, recs, cnt, ACGPU_REC_SET / 4, c.stream);
        if (rc) return rc;
        const bool at_end = p.pos >= p.end, last = at_end && text_end; // (a whole text's one piece ends at p.end)
        const uint64_t m = c.n_carry + cnt;
        if ((rc = spans_piece(c, base, cnt, p.pos, last, at_end && !text_end))) return rc;
        if (c.merged && (rc = c.merged(c.ctx, m, last))) return rc;
    }
    if (range) {
        // a text's last range that owns nothing new: what the ranges before it withheld is finalised by a piece without records
        if (!p.pieces && text_end) {
            const uint64_t m = c.n_carry;
            if ((rc = spans_piece(c, 0, 0, p.end, true))) return rc;
            if (c.merged && (rc = c.merged(c.ctx, m, true))) return rc;
        }
        range->scanned = p.pieces != 0;
        range->chain_exit = p.chain;
        // what the range withheld, for the next one: the carry buffer the last piece wrote (c.cur names it now)
        try {
            range->carry_out.resize(c.n_carry);
        } catch (...) {
            return ACGPU_E_NOMEM;
        }
        if (c.n_carry == 1 && c.piece_carried == 1) {
            range->carry_out[0] = c.piece_carry0;
        } else if (c.n_carry) {
            HIP_TRY(hipMemcpyAsync(range->carry_out.data(), reinterpret_cast<const int2 *>(d.spans_carry.p) + (size_t)c.cur * c.carry_cap, (size_t)c.n_carry * 8,
                                   hipMemcpyDeviceToHost, c.stream));
            HIP_TRY(hipStreamSynchronize(c.stream));
        }
    }
    c.st.pieces += (uint32_t)p.pieces; // (added: a batch call haystack by haystack drives one text after the other)
    c.st.rescans += (uint32_t)p.rescans;
    return ACGPU_OK;
}

} // namespace acgpu

namespace {

// what every entry returns behind its last piece
int spans_result(SpansCall &c, uint64_t *n_out, acgpu_spans_stats *st) {
    c.st.n_spans = c.out_pos;
    if (st) *st = c.st;
    *n_out = c.out_pos;
    return c.out_pos > c.cap ? ACGPU_E_OVERFLOW : ACGPU_OK;
}

// The body of acgpu_spans_utf8 and acgpu_spans_utf8_lossy.  P (acgpu_host.h): how the text is staged, and the entry's stats.
template <class P>
int spans_utf8(const acgpu_automaton *ca, const uint8_t *bytes, uint64_t n_bytes, int32_t *out, uint64_t cap, uint64_t *n_out,
               acgpu_spans_stats *st, typename P::Stats *ust) {
    if (!ca || !n_out || (n_bytes && !bytes) || (cap && !out)) return ACGPU_E_INVALID;
    if (n_bytes >= (1ull << 31)) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    *n_out = 0;
    if (st) *st = acgpu_spans_stats{};
    if (ust) *ust = P::stats();
    if (n_bytes == 0) return ACGPU_OK; // (nothing to decode and nothing to merge: no device needed)
    PoolCall call(a); // (no device: fails here, as acgpu_match_utf8 does, and out is untouched)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    int rc = call.idle(); // (the NULL stream: see the stream rule)
    if (rc) return rc;
    Utf8Text text;
    rc = stage_utf8_text(d, bytes, n_bytes, d.call_stream, &text, P::errors);
    if (ust) *ust = P::stats(&text, rc);
    if (rc == ACGPU_E_ENCODING) return rc; // (the stream is idle: the pool is as usable as before the call)
    if (rc) return call.fail(rc);
    SpansCall c{a, d, d.call_stream};
    c.u8 = &text;
    c.h_out = out;
    c.cap = cap;
    const bool whole = shard_rule(a->t, ACGPU_REC_SET, false).sequential;
    if ((rc = spans_pieces(c, 0, whole, PieceScan{a, d, nullptr, 0, &text.shard, c.stream}, text.shard.n_units))) return call.fail(rc);
    if (hipStreamSynchronize(c.stream) != hipSuccess) return call.fail(ACGPU_E_HIP);
    return spans_result(c, n_out, st);
}

// The body of acgpu_spans_batch_utf8 and acgpu_spans_batch_utf8_lossy.  The batch is staged as acgpu_match_batch_utf8 stages it
// and scanned as ONE device shard; a piece's records become VIRTUAL COORDINATES where they lie -- v = byte of the span + index of
// the haystack, the caller's bytes with a phantom element behind every haystack -- and the merge, the carry and
// k_span_tag run over v as they run over a UTF-16 batch's units: no record covers a phantom, so no span reaches across two
// haystacks, and a span minus voff[haystack] is in bytes of its haystack.
template <class P>
int spans_batch_utf8(const acgpu_automaton *ca, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks, int32_t *out, uint64_t cap,
                     uint64_t *n_out, acgpu_spans_stats *st, typename P::Stats *ust) {
    if (!ca || !offsets || !n_out || (cap && !out)) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    const HostTables &t = a->t;
    BatchPlan plan; // (in bytes: bytes >= units, so bytes + haystacks < 2^31 bounds the text the scan sees, and the virtual text)
    int rc = check_batch(t, reinterpret_cast<const uint16_t *>(bytes), offsets, n_haystacks, &plan);
    if (rc) return rc;
    *n_out = 0;
    if (st) *st = acgpu_spans_stats{};
    if (ust) *ust = P::stats();
    if (plan.total == 0) return ACGPU_OK; // (nothing to decode and nothing to merge: no device needed)
    PoolCall call(a); // (no device: fails here, and out is untouched)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    Utf8Batch b;
    if ((rc = utf8_batch_front<P>(call, t, bytes, offsets, n_haystacks, plan, &b, ust))) return rc;
    SpansCall c{a, d, d.call_stream};
    c.h_out = out;
    c.cap = cap;
    const bool whole = shard_rule(t, ACGPU_REC_SET, false).sequential; // (a device shard: as acgpu_spans_utf8 drives its pieces)
    if (plan.per_haystack) { // every haystack as a text of its own, by the route acgpu_spans_utf8 takes
        c.tag_all = true;
        rc = utf8_each_haystack<P>(
            d, bytes, offsets, n_haystacks, c.stream,
            [&](uint32_t i, const Utf8Text &text) { // (staged on the call's stream, behind the copies of the haystack before: no wait)
                c.u8 = &text;
                c.tag = (int32_t)i;
                const int prc = spans_pieces(c, 0, whole, PieceScan{a, d, nullptr, 0, &text.shard, c.stream}, text.shard.n_units);
                c.u8 = nullptr;
                return prc;
            },
            [](uint32_t) {});
        if (rc) return call.fail(rc);
    } else {
        std::vector<uint32_t> h_voff;
        if ((rc = utf8_virtual_offsets(d, b, c.stream, &h_voff, &c.cat_off))) return call.fail(rc);
        c.u8 = &b.text;
        c.ub = &b;
        c.n_hay = n_haystacks;
        {
            SeparatorScan sep(d, t);
            rc = spans_pieces(c, 0, whole, PieceScan{a, d, nullptr, 0, &b.text.shard, c.stream}, b.text.shard.n_units);
        }
        if (rc) return call.fail(rc);
    }
    if (hipStreamSynchronize(c.stream) != hipSuccess) return call.fail(ACGPU_E_HIP);
    return spans_result(c, n_out, st);
}

} // namespace

extern "C" {

int acgpu_spans_u16(const acgpu_automaton *ca, const uint16_t *haystack, uint64_t n_units, int32_t *out, uint64_t cap, uint64_t *n_out,
                    acgpu_spans_stats *st) {
    if (!ca || !n_out || (n_units && !haystack) || (cap && !out)) return ACGPU_E_INVALID;
    if (n_units >= (1ull << 31)) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    PoolCall call(a); // (no device: fails here, as acgpu_match_u16 does, and out is untouched)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    int rc = call.on(d.call_stream);
    if (rc) return rc;
    SpansCall c{a, d, d.call_stream};
    c.h_out = out;
    c.cap = cap;
    if ((rc = spans_pieces(c, 0, host_one_piece(a->t, ACGPU_REC_SET), PieceScan{a, d, haystack, n_units, nullptr, c.stream}, n_units))) return call.fail(rc);
    if (hipStreamSynchronize(c.stream) != hipSuccess) return call.fail(ACGPU_E_HIP);
    return spans_result(c, n_out, st);
}

int acgpu_spans_device(const acgpu_automaton *ca, acgpu_shard *shard, int32_t *d_out, uint64_t cap, uint64_t *n_out, void *stream_,
                       acgpu_spans_stats *st) {
    if (!ca || !shard || !n_out || (cap && !d_out) || ((uintptr_t)d_out & 15)) return ACGPU_E_INVALID;
    if (shard->n_units >= (1ull << 31) || (shard->n_units && !shard->d_hay) || ((uintptr_t)shard->d_hay & 15)) return ACGPU_E_INVALID;
    // one shard of a sharded text: the spans it withholds would have to travel to the rank behind it -- not built
    if (!shard_is_whole_text(*shard)) return ACGPU_E_UNSUPPORTED;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    PoolCall call(a);
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    const hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    int rc = call.on(stream);
    if (rc) return rc;
    SpansCall c{a, d, stream};
    c.d_out = d_out;
    c.cap = cap;
    const bool whole = shard_rule(a->t, ACGPU_REC_SET, false).sequential;
    rc = spans_pieces(c, shard->chain_entry, whole, PieceScan{a, d, nullptr, 0, shard, stream}, shard->n_units);
    const hipError_t e = hipStreamSynchronize(stream); // the final wait
    if (rc) return rc;
    HIP_TRY(e);
    return spans_result(c, n_out, st);
}

int acgpu_spans_batch_u16(const acgpu_automaton *ca, const uint16_t *units, const uint64_t *offsets, uint32_t n_haystacks, int32_t *out, uint64_t cap,
                          uint64_t *n_out, acgpu_spans_stats *st) {
    if (!ca || !offsets || !n_out || (cap && !out)) return ACGPU_E_INVALID;
    *n_out = 0;
    if (st) *st = acgpu_spans_stats{};
    if (n_haystacks == 0) return ACGPU_OK;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    const HostTables &t = a->t;
    BatchPlan plan;
    int rc = check_batch(t, units, offsets, n_haystacks, &plan);
    if (rc) return rc;
    PoolCall call(a); // (no device: fails here, and out is untouched)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    SpansCall c{a, d, d.call_stream};
    c.h_out = out;
    c.cap = cap;
    if (plan.per_haystack) { // every haystack as a text of its own, by the route acgpu_spans_u16 takes
        if ((rc = call.on(c.stream))) return rc;
        c.tag_all = true;
        for (uint32_t i = 0; i < n_haystacks; i++) {
            const uint64_t len = offsets[i + 1] - offsets[i];
            if (!len) continue;
            c.tag = (int32_t)i;
            const uint16_t *hay = units + offsets[i];
            if ((rc = spans_pieces(c, 0, host_one_piece(t, ACGPU_REC_SET), PieceScan{a, d, hay, len, nullptr, c.stream}, len))) return call.fail(rc);
        }
    } else {
        if ((rc = call.idle())) return rc; // (the NULL stream: see the stream rule)
        BatchText text(d, t);
        if ((rc = text.stage(units, offsets, n_haystacks, c.stream))) return call.fail(rc);
        c.cat_off = text.d_off();
        c.n_hay = n_haystacks;
        if ((rc = spans_pieces(c, 0, host_one_piece(t, ACGPU_REC_SET), PieceScan{a, d, text.h_cat, text.cat, nullptr, c.stream}, text.cat))) return call.fail(rc);
    } // (every scan has been waited for: what is left on the stream are the copies of the last piece's spans)
    if (hipStreamSynchronize(c.stream) != hipSuccess) return call.fail(ACGPU_E_HIP);
    return spans_result(c, n_out, st);
}

int acgpu_spans_utf8(const acgpu_automaton *a, const uint8_t *bytes, uint64_t n_bytes, int32_t *out, uint64_t cap, uint64_t *n_out,
                     acgpu_spans_stats *st, acgpu_utf8_stats *ust) {
    return spans_utf8<Utf8StrictText>(a, bytes, n_bytes, out, cap, n_out, st, ust);
}

int acgpu_spans_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, uint64_t n_bytes, int32_t *out, uint64_t cap, uint64_t *n_out,
                           acgpu_spans_stats *st, acgpu_utf8_lossy_stats *ust) {
    return spans_utf8<Utf8LossyText>(a, bytes, n_bytes, out, cap, n_out, st, ust);
}

int acgpu_spans_batch_utf8(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks, int32_t *out, uint64_t cap,
                           uint64_t *n_out, acgpu_spans_stats *st, acgpu_utf8_batch_stats *ust) {
    return spans_batch_utf8<Utf8StrictBatch>(a, bytes, offsets, n_haystacks, out, cap, n_out, st, ust);
}

int acgpu_spans_batch_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks, int32_t *out,
                                 uint64_t cap, uint64_t *n_out, acgpu_spans_stats *st, acgpu_utf8_lossy_stats *ust) {
    return spans_batch_utf8<Utf8LossyBatch>(a, bytes, offsets, n_haystacks, out, cap, n_out, st, ust);
}

} // extern "C"
