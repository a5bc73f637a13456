// acgpu_cover.hip -- acgpu_cover_u16 / acgpu_cover_batch_u16 / acgpu_cover_device / acgpu_cover_utf8 / acgpu_cover_utf8_lossy /
// acgpu_cover_batch_utf8 / acgpu_cover_batch_utf8_lossy (include/acgpu.h): the text
// with every span [s, e) -- the spans of acgpu_spans_* -- rewritten as open ++ body ++ close, on the device, for all five families.
// body is the covered text itself (KEEP: highlight, tagging), one fill element per covered element (FILL: mask) or nothing (DROP:
// redaction, deletion); everything outside the spans is copied.
//
// A cover call is a consumer of the spans piece loop (spans_pieces, acgpu_spans.h): behind every piece the five launches of the
// merge run as they do for the spans entries, but the piece's final spans stay in the pool (d.cover_spans), and with {n_final, n_carry}
// the host reads in the same wait
//   L, the SETTLED POSITION: the text's end on the last piece, else min(B, start of the first carried span), B as final_below has
//      it (k_span_settled).  Every position below L is inside a final span or will never be covered: a later record starts at or
//      behind B, and what the carry holds starts at or behind its first span.  L never moves backwards: B does not, and a carried
//      span's start is the smallest start of a run of intervals each of which is a span carried before (start >= the L of then)
//      or a record of a later piece (start >= the B of then >= the L of then).  So `done`, the L of the piece before, is at or in
//      front of every span this piece finalises, and the final spans of a piece lie in [done, L): they end before B and before
//      the first carried span.
//   and for DROP the elements the piece's final spans hold (the plan's sum).
// The piece then emits the text's elements [done, L) with its final spans rewritten (cover_piece, the loop's step behind the
// merge), by the plan and the emit of acgpu_emit.h:
//  * the plan's ITEMS are the piece's final spans.  With w = open_len + close_len, span k begins at output position
//    pos_k = (s_k - done) + k w - D_k of the piece's output, D_k = 0 for KEEP and FILL -- closed form, no scan, no array -- and the
//    elements of the piece's spans in front of k for DROP: THE PLAN below (k_cover_sums, k_cover_plan_offsets, k_cover_plan) over
//    what a span adds, w minus its elements, which takes its n from the merge's slot on the device, so it runs BEFORE the piece's
//    one wait.  The positions ascend strictly: two spans do not touch, so pos_{k+1} - pos_k >= 1 + w.
//  * the emit's SOURCE (CoverArgs, k_cover_emit<T, BODY, BATCH>) has up to four sources per segment: open, the body, close, and
//    the text behind the span up to the next one.
// The running output position and the running span count travel from piece to piece on the host (CoverCall).
//
// The text stays on the device for the whole call: a carried span can be as long as the text (keyword "aa" on "aaaa..."), and
// KEEP copies its body long after the piece that first saw it.  The UTF-8 entries hold the caller's bytes anyway; acgpu_cover_u16
// stages the whole text once (stage_whole_text: one blocking copy in front, not hidden behind the scan) and drives the pieces
// over it as a device shard.
//
// acgpu_cover_batch_u16 rewrites many short texts as ONE such text: the haystacks with a separator unit behind each (BatchText),
// staged whole like acgpu_cover_u16's text.  No record holds a separator, so the spans of that text are the haystacks' spans; a
// separator is an item of the same plan that emits nothing and skips one element, so the results come out back to back (see "a
// batch call" below, and DESIGN.md 4.24).  acgpu_cover_batch_utf8 does the same for bytes over virtual coordinates, the caller's
// bytes with a phantom element behind every haystack in the separator's place (cover_batch_utf8 below).
//
// acgpu_stream_cover_* (acgpu_stream.hip) cover a text that arrives in chunks: cover_feed below drives the same pieces over the owned
// range of a feed's buffer, and there the text does NOT stay -- a feed may end inside a span, which the emit's source serves with
// two kinds of item that no whole text has (A FEED below, CoverArgs::cut and ::head).
//
// One plan, one emit launch (launch_emit<T, BODY, BATCH>, twelve kernels) and one piece step (cover_piece) serve all of them; the
// separators' descriptor and searches are acgpu_emit.h's, shared with the replace entries; the entries' bodies share
// cover_staged_text (one staged text to its end), cover_batch_result and the UTF-8 batch front and loop of acgpu_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "acgpu_device.h"
#include "acgpu_emit.h"
#include "acgpu_host.h"
#include "acgpu_internal.h"
#include "acgpu_spans.h"

using namespace acgpu;

namespace {

constexpr int kCoverLds = 1536; // segments a workgroup stages (32 bytes each)

// A segment of four sources: from u = rel on, the elements below a_end are elements osrc + u of open, those below b_end the body
// (elements bsrc + u of the text, or the fill element), those below c_end elements csrc + u of close, the others elements
// tsrc + u of the text.
struct CSeg {
    int32_t rel, a_end, b_end, c_end;
    uint32_t osrc, bsrc, csrc, tsrc;
};

// The emit's source (acgpu_emit.h): the text with a piece's final spans (text coordinates, elements) rewritten.
// BATCH (acgpu_cover_batch_u16): `spans` is the piece's ITEM list -- its final spans and, as {p, p}, the separators at p -- and
// `pos` the plan over it, whatever the body.  A separator has neither open nor body nor close, and the text behind it begins at
// p + 1: it emits nothing and skips one element.  Its segment is empty where the next item touches it, and so is a DROP span's
// with an empty open and close: positions ascend WEAKLY, which is all the emit asks (emit_block takes the last of equal ones).
// make_seg assumes nothing about the next item: P may lie anywhere at or below the tile's last element, and what it adds to P is
// clamped to the tile.
// A byte batch (acgpu_cover_batch_utf8) works in VIRTUAL COORDINATES, the caller's bytes with a phantom element behind every
// haystack (voff[j] = haystack j's first element): items and `done` are v, and an element v of haystack h is byte
// v - h of `hay`.  An item is a segment and every phantom is an item, so h is constant within a segment: make_seg finds it once
// per segment (haystack_of over voff) and the segment's text sources carry the shift; whole() and element() read them as ever.
template <bool VIRT>
struct CoverShift {
    __device__ __forceinline__ uint32_t hay_of(int64_t) const { return 0; }
};
template <>
struct CoverShift<true> {
    const uint32_t *voff;
    uint32_t n_hay;
    __device__ __forceinline__ uint32_t hay_of(int64_t v) const { return haystack_of(voff, n_hay, (uint32_t)v); }
};

template <class T, int BODY, bool BATCH = false>
struct CoverArgs : CoverShift<BATCH && sizeof(T) == 1> {
    static constexpr bool VIRT = BATCH && sizeof(T) == 1;
    using Elem = T;
    using Seg = CSeg;
    static constexpr int kLds = kCoverLds;
    const T *hay;        // the whole text
    const int2 *spans;
    const int64_t *pos;  // DROP, and every BATCH call: the plan; else nullptr, the positions are closed form
    int64_t n_spans;
    const T *open, *close;
    uint32_t ol, cl;
    uint32_t fill;
    int64_t done;        // output element 0 of the piece is text element `done` (if no span starts there)
    // A FEED of a cover stream (cover_feed below; no batch call) has two kinds of item that a whole text has not:
    //  * item 0 is HEADLESS iff spans[0].x < done -- a span that an earlier feed opened and cut at `done`: no open, and its body
    //    begins at `done` (its true start, in front of the buffer if need be, is kept so that the item is never empty: where its
    //    end equals `done` it is close alone).  head = ol then, else 0: what the closed form takes off every later position;
    //  * the last item is TAILLESS iff its end is at or behind `cut`, where the feed's output ends: no close, the body ends at cut.
    //    cut = INT64_MAX: no feed, or a piece that cuts nothing.
    // Both are clipped here and nowhere else: text in front of `done` or behind `cut` is never read for a body.
    int64_t cut, head;
    int64_t w0, w1;
    T *dst;
    int32_t cap;         // segments to stage at most (tunable "cover_lds_segments")
    __device__ __forceinline__ int32_t lds_cap() const { return cap; }
    __device__ __forceinline__ int64_t n() const { return n_spans; }
    __device__ __forceinline__ int64_t pos_at(int64_t i) const {
        if (BODY == ACGPU_COVER_DROP || BATCH) return pos[i];
        return std::max<int64_t>(spans[i].x, done) - done + i * ((int64_t)ol + (int64_t)cl) - (i ? head : 0);
    }
    __device__ __forceinline__ CSeg make_seg(int64_t i, int64_t t0) const {
        CSeg s;
        if (i < 0) {
            s.rel = -1;
            s.a_end = s.b_end = s.c_end = 0;
            s.osrc = s.bsrc = s.csrc = 0;
            s.tsrc = (uint32_t)(done + t0) - this->hay_of(done); // (VIRT: up to the first item the text is the haystack's that holds `done`)
            return s;
        }
        const int2 sp = spans[i];
        const int64_t P = pos_at(i) - t0; // < kEmitTile<T>
        const bool sep = BATCH && sp.y == sp.x;
        // VIRT: the item's haystack.  A span's body and the text behind it are bytes v - h; the text behind haystack h's phantom p
        // begins at p + 1 in haystack h + 1, which is byte p - h.
        const uint32_t h = this->hay_of(sp.x);
        if constexpr (!BATCH) { // (a feed's items: see `cut` above; for every other call s0 = sp.x, e0 = sp.y and both flags are false)
            const bool headless = (int64_t)sp.x < done, tailless = (int64_t)sp.y >= cut;
            const int64_t s0 = headless ? done : (int64_t)sp.x, e0 = tailless ? cut : (int64_t)sp.y;
            const int64_t a = P + (headless ? 0 : (int64_t)ol), b = a + (BODY == ACGPU_COVER_DROP ? 0 : e0 - s0), c = b + (tailless ? 0 : (int64_t)cl);
            auto in_tile = [](int64_t x) { return (int32_t)std::min<int64_t>(std::max<int64_t>(x, 0), kEmitTile<T>); };
            s.rel = (int32_t)std::max<int64_t>(P, -1);
            s.a_end = in_tile(a);
            s.b_end = in_tile(b);
            s.c_end = in_tile(c);
            s.osrc = (uint32_t)0 - (uint32_t)P;
            s.bsrc = (uint32_t)s0 - (uint32_t)a;
            s.csrc = (uint32_t)0 - (uint32_t)b;
            s.tsrc = (uint32_t)e0 - (uint32_t)c;
            return s;
        }
        const int64_t a = P + (sep ? 0 : (int64_t)ol), b = a + (BODY == ACGPU_COVER_DROP ? 0 : (int64_t)(sp.y - sp.x)), c = b + (sep ? 0 : (int64_t)cl);
        auto in_tile = [](int64_t x) { return (int32_t)std::min<int64_t>(std::max<int64_t>(x, 0), kEmitTile<T>); };
        s.rel = (int32_t)std::max<int64_t>(P, -1);
        s.a_end = in_tile(a);
        s.b_end = in_tile(b);
        s.c_end = in_tile(c);
        s.osrc = (uint32_t)0 - (uint32_t)P;
        s.bsrc = (uint32_t)sp.x - h - (uint32_t)a;
        s.csrc = (uint32_t)0 - (uint32_t)b;
        s.tsrc = (uint32_t)sp.y + (VIRT ? 0u : (uint32_t)sep) - h - (uint32_t)c;
        return s;
    }
    // (inside a FILL body the vector is a constant and needs no load)
    __device__ __forceinline__ bool whole(const CSeg &s, int32_t u0, rp_v4u *v) const {
        constexpr int kPer = kEmitPer<T>;
        if (u0 >= s.c_end) *v = load16(hay + (uint32_t)(s.tsrc + (uint32_t)u0));
        else if (u0 >= s.a_end && u0 + kPer <= s.b_end) {
            if (BODY == ACGPU_COVER_FILL) v->x = v->y = v->z = v->w = sizeof(T) == 2 ? (fill | (fill << 16)) : fill * 0x01010101u;
            else *v = load16(hay + (uint32_t)(s.bsrc + (uint32_t)u0));
        } else if (u0 + kPer <= s.a_end) *v = load16(open + (uint32_t)(s.osrc + (uint32_t)u0));
        else if (u0 >= s.b_end && u0 + kPer <= s.c_end) *v = load16(close + (uint32_t)(s.csrc + (uint32_t)u0));
        else return false;
        return true;
    }
    __device__ __forceinline__ uint32_t element(const CSeg &s, int32_t u) const {
        if constexpr (VIRT) {
            // (the sources read up front, by value: left in the branches, the compiler made a choice between the body's, close's and
            // the text's source a choice between the ADDRESSES of s.bsrc, s.csrc and s.tsrc in k_cover_emit<uint8_t, KEEP, true> and
            // <.., DROP, true>, and kept the segment in 36 bytes of private memory for it)
            const uint32_t bs = s.bsrc + (uint32_t)u, cs = s.csrc + (uint32_t)u, ts = s.tsrc + (uint32_t)u;
            if (u < s.a_end) return open[(uint32_t)(s.osrc + (uint32_t)u)];
            if (u < s.b_end) return BODY == ACGPU_COVER_FILL ? fill : (uint32_t)hay[bs];
            if (u < s.c_end) return close[cs];
            return hay[ts];
        }
        if (u < s.a_end) return open[(uint32_t)(s.osrc + (uint32_t)u)];
        if (u < s.b_end) return BODY == ACGPU_COVER_FILL ? fill : (uint32_t)hay[(uint32_t)(s.bsrc + (uint32_t)u)];
        if (u < s.c_end) return close[(uint32_t)(s.csrc + (uint32_t)u)];
        return hay[(uint32_t)(s.tsrc + (uint32_t)u)];
    }
};

template <class T, int BODY, bool BATCH>
__global__ __launch_bounds__(kEmitBlock) void k_cover_emit(CoverArgs<T, BODY, BATCH> A) {
    emit_block(A);
}

// ---- THE PLAN (acgpu_emit.h) of a piece whose positions have no closed form: a DROP call's, over the piece's final spans, and
// every batch call's, over its items -- final spans and, as {p, p}, separators.  Their number is on the device only, the plan runs
// in front of the piece's wait: n_final[0] final spans and, n_sep given, n_sep[0] separators; the grids are sized by what the host
// does know, M >= that number.  d.cover_plan holds {n_final, n_sep} of a batch call | the workgroups' sums | the positions. ----

constexpr int kPlanHead = 2; // words in front of the plan's sums: a batch call's {n_final, n_sep}

__device__ __forceinline__ uint64_t plan_items(const uint64_t *n_final, const uint64_t *n_sep) { return n_final[0] + (n_sep ? n_sep[0] : 0); }

// The plan's item: what item i adds to the output's length beyond the text it stands for -- -1 for a separator (the one item
// without elements), else w = open + close minus, for DROP, the span's elements.  A feed's HEADLESS item (CoverArgs: it starts in
// front of `done`) has no open and only its elements from `done` on; no other call has an item in front of its `done`.
__device__ __forceinline__ int64_t item_delta(const int2 *items, uint64_t i, int64_t w, int drop, int64_t done, int64_t ol) {
    const int2 it = items[i];
    if (it.y == it.x) return -1;
    const bool headless = (int64_t)it.x < done;
    return w - (headless ? ol : 0) - (drop ? (int64_t)it.y - (headless ? done : (int64_t)it.x) : 0);
}

__global__ __launch_bounds__(kPlanBlock) void k_cover_sums(const int2 *__restrict__ items, const uint64_t *__restrict__ n_final, const uint64_t *__restrict__ n_sep,
                                                           int64_t w, int drop, int64_t done, int64_t ol, int64_t *__restrict__ bsum) {
    plan_sums([=](uint64_t i) { return item_delta(items, i, w, drop, done, ol); }, plan_items(n_final, n_sep), bsum);
}

// *dropped (the merge's slot[kSpanDropped], or nullptr) = the elements of the text in [done, L) that have no output of their own:
// the separators, and a DROP call's covered elements -- n_final w minus the sum of the deltas (a feed with a headless item: plus
// open's length, which the host takes off again)
__global__ __launch_bounds__(kPlanBlock) void k_cover_plan_offsets(int64_t *__restrict__ bsum, uint32_t n_blocks, const uint64_t *__restrict__ n_final, int64_t w,
                                                                   uint64_t *__restrict__ dropped) {
    const int64_t sum = plan_offsets(bsum, n_blocks);
    if (threadIdx.x == 0 && dropped) *dropped = (uint64_t)((int64_t)n_final[0] * w - sum);
}

// pos[k] = (s_k - done) + the deltas in front of item k (a headless item: at 0)
__global__ __launch_bounds__(kPlanBlock) void k_cover_plan(const int2 *__restrict__ items, const uint64_t *__restrict__ n_final, const uint64_t *__restrict__ n_sep,
                                                           const int64_t *__restrict__ bsum, int64_t done, int64_t w, int64_t ol, int drop, int64_t *__restrict__ pos) {
    plan_positions([=](uint64_t i) { return item_delta(items, i, w, drop, done, ol); }, plan_items(n_final, n_sep), bsum,
                   [&](uint64_t k, int64_t front) { pos[k] = std::max<int64_t>(items[k].x, done) - done + front; });
}

// A feed's TAILLESS item (CoverArgs), which the merge withheld and the feed's last piece emits all the same up to `cut`: item `at`
// of the piece's list, behind its final spans, and for DROP its position behind their plan.  One thread.
__global__ void k_cover_tail_item(int2 *__restrict__ items, int64_t *__restrict__ pos, uint64_t at, int2 span, int64_t p) {
    items[at] = span;
    if (pos) pos[at] = p;
}

// What one call holds while it runs (the caller holds d.mu).  Positions and lengths are ELEMENTS: units, or bytes of a UTF-8 text.
struct CoverCall {
    SpansCall sc;
    uint32_t esz = 2;         // bytes of an element
    const void *hay = nullptr; // the whole text on the device
    uint64_t n = 0;           // its elements
    uint32_t body = 0, fill = 0, ol = 0, cl = 0;
    const void *d_open = nullptr, *d_close = nullptr;
    uint8_t *h_out = nullptr; // the host entry's result (through the slabs) ...
    uint8_t *d_out = nullptr; // ... or the device entry's
    uint64_t cap = 0;
    uint64_t done = 0;        // output exists for the text's elements [0, done)
    uint64_t out_pos = 0;     // elements of it (beyond cap: counted, not written)
    // a batch call over the concatenation: its offsets on the host and on the device (n_hay + 1 words), the result's offsets on the
    // device (n_hay + 1 words of 64 bits), and what the current piece's plan was sized for
    const uint32_t *h_cat_off = nullptr, *d_cat_off = nullptr;
    uint32_t n_hay = 0;
    uint64_t *d_out_off = nullptr;
    uint64_t piece_items = 0;   // m + piece_max_sep: the items the plan has room for
    uint32_t piece_max_sep = 0; // the separators in [done, own_hi)
    // a FEED of a cover stream (cover_feed): hay is the feed's buffer, and `done` may stand inside a span
    bool feed = false;
    bool in_span = false;       // element done - 1 is covered by a span that has not been closed: the list's first span is HEADLESS
    uint64_t opens = 0;         // the spans whose open the feed has emitted
    int64_t piece_cut = INT64_MAX, piece_head = 0; // CoverArgs::cut and ::head of the piece being emitted
};

// open and close on the device, each padded so that an aligned 16-byte load around any of their elements stays inside the blob
int upload_spec(CoverCall &c, const acgpu_cover_spec &spec) {
    const size_t ob = (((size_t)spec.open_len * c.esz + 15) & ~(size_t)15) + 16, cb = (((size_t)spec.close_len * c.esz + 15) & ~(size_t)15) + 16;
    std::vector<uint8_t> blob;
    try {
        blob.assign(ob + cb, 0);
    } catch (...) {
        return ACGPU_E_NOMEM;
    }
    if (spec.open_len) std::copy_n(static_cast<const uint8_t *>(spec.open), (size_t)spec.open_len * c.esz, blob.data());
    if (spec.close_len) std::copy_n(static_cast<const uint8_t *>(spec.close), (size_t)spec.close_len * c.esz, blob.data() + ob);
    DeviceState &d = c.sc.d;
    const int rc = d.cover_tab.ensure(blob.size());
    if (rc) return rc;
    HIP_TRY(hipMemcpy(d.cover_tab.p, blob.data(), blob.size(), hipMemcpyHostToDevice)); // (blocking: the blob dies here)
    c.d_open = d.cover_tab.p;
    c.d_close = static_cast<const uint8_t *>(d.cover_tab.p) + ob;
    c.ol = spec.open_len;
    c.cl = spec.close_len;
    c.body = spec.body;
    c.fill = spec.fill;
    return ACGPU_OK;
}

// d.cover_plan with room for a plan over M items
int plan_room(DeviceState &d, uint64_t M) { return d.cover_plan.ensure((kPlanHead + (size_t)((M + kPlanTile - 1) / kPlanTile) + M) * 8); }
uint64_t *plan_head(DeviceState &d) { return reinterpret_cast<uint64_t *>(d.cover_plan.p); }
int64_t *plan_pos(DeviceState &d, uint64_t M) { return reinterpret_cast<int64_t *>(plan_head(d) + kPlanHead) + (M + kPlanTile - 1) / kPlanTile; }

// the plan's three launches over `items`, sized for M of them (plan_room has made the room)
void launch_plan(CoverCall &c, const int2 *items, uint64_t M, const uint64_t *n_final, const uint64_t *n_sep, uint64_t *d_dropped) {
    const uint32_t n_blocks = (uint32_t)((M + kPlanTile - 1) / kPlanTile);
    int64_t *bsum = reinterpret_cast<int64_t *>(plan_head(c.sc.d) + kPlanHead);
    const hipStream_t stream = c.sc.stream;
    const int64_t w = (int64_t)c.ol + (int64_t)c.cl;
    const int drop = c.body == ACGPU_COVER_DROP;
    hipLaunchKernelGGL(k_cover_sums, dim3(n_blocks), dim3(kPlanBlock), 0, stream, items, n_final, n_sep, w, drop, (int64_t)c.done, (int64_t)c.ol, bsum);
    hipLaunchKernelGGL(k_cover_plan_offsets, dim3(1), dim3(kPlanBlock), 0, stream, bsum, n_blocks, n_final, w, d_dropped);
    hipLaunchKernelGGL(k_cover_plan, dim3(n_blocks), dim3(kPlanBlock), 0, stream, items, n_final, n_sep, (const int64_t *)bsum, (int64_t)c.done, w, (int64_t)c.ol,
                       drop, plan_pos(c.sc.d, M));
}

// SpansCall::planned of a DROP call that is no batch: the plan over the piece's final spans, whose number is the merge's slot[0],
// enqueued in front of the piece's wait.  A span is never empty, so no item passes for a separator: pos[k] = (s_k - done) + k w -
// the elements of the spans in front of k, and slot[kSpanDropped] = the elements of all final spans.
int plan_dropped(void *ctx, uint64_t *d_slot, const int2 *d_spans, uint64_t m) {
    CoverCall &c = *static_cast<CoverCall *>(ctx);
    const int rc = plan_room(c.sc.d, m);
    if (rc) return rc;
    launch_plan(c, d_spans, m, d_slot, nullptr, d_slot + kSpanDropped);
    HIP_TRY(hipGetLastError());
    return ACGPU_OK;
}

// ---- a batch call (acgpu_cover_batch_u16): the text is the haystacks' concatenation, a separator behind each, and a separator is
// an ITEM of the plan that emits nothing and skips one element.  Behind a piece's merge its final spans and the separators in
// [done, L) become one ascending list (k_cover_batch_merge: a rank merge, one binary search per element -- the two lists cannot
// tie, a separator is never covered), the plan runs over that list for every body (an item's delta: -1 for a separator, else
// w minus, for DROP, the span's elements), and k_cover_batch_offsets reads every result's first output element off the plan.
// All of it is enqueued BEFORE the piece's wait, where n_final and L are on the device only: k_cover_batch_head reads them from
// the merge's head, counts the separators below L in cat_off and leaves {n_final, n_sep} for the other kernels; the grids are
// sized by what the host does know, m and the separators in [done, own_hi) -- L <= own_hi, see DESIGN.md 4.24. ----

constexpr int kBatchBlock = 256; // lanes of the merge's and the offsets' workgroups

// (The separators a piece may emit are a BatchSeps of acgpu_emit.h in text coordinates, base = 0; its n_sep is the host's bound,
// the separators in [done, own_hi), and what the kernels take for the count is head[1].)

// Where a piece's n_final and L come from: the merge's head on the device (acgpu_spans.h); slot == nullptr: a piece without
// intervals, which has no final span and whose L the host knows.
struct CoverPieceIn {
    const uint64_t *slot;
    uint64_t m;      // the intervals the piece merged: n_final is at most that
    int64_t L;       // L where the head does not hold it: without a slot, and on the last piece
    int32_t slot_L;  // L is slot[kSpanSettled]
};

// a piece's spans: ascending starts
__device__ __forceinline__ uint64_t spans_before(const int2 *__restrict__ spans, uint64_t n, int64_t p) {
    return starts_before([=](uint64_t i) { return spans[i].x; }, n, p);
}

// one thread: head = {n_final, the separators in [done, L)}, both counts clamped to what the grids and buffers are sized for
__global__ void k_cover_batch_head(CoverPieceIn in, BatchSeps S, uint32_t n_hay, uint64_t *__restrict__ head) {
    const uint64_t n_final = in.slot ? std::min<uint64_t>(in.slot[0], in.m) : 0;
    const int64_t L = in.slot && in.slot_L ? (int64_t)in.slot[kSpanSettled] : in.L;
    uint32_t lo = S.i0, hi = n_hay; // the first separator at or behind L: cat_off[j + 1] - 1 >= L
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((int64_t)S.cat_off[mid + 1] <= L) lo = mid + 1;
        else hi = mid;
    }
    head[0] = n_final;
    head[1] = std::min(lo - S.i0, S.n_sep);
}

// items = the piece's final spans and, as {p, p}, its separators, in position order (THE SEPARATORS, acgpu_emit.h: a separator
// is never covered); a thread per span (t < m) or separator
__global__ __launch_bounds__(kBatchBlock) void k_cover_batch_merge(const int2 *__restrict__ spans, const uint64_t *__restrict__ head, BatchSeps S, uint64_t m,
                                                                   int2 *__restrict__ items) {
    S.base = 0; // (text coordinates, as plan_batch sets it: said here, the subtraction is compiled away)
    const uint64_t t = (uint64_t)blockIdx.x * kBatchBlock + threadIdx.x;
    const uint64_t n_final = head[0];
    const uint32_t n_sep = (uint32_t)head[1];
    if (t < m) {
        if (t >= n_final) return;
        const int2 sp = spans[t];
        items[t + seps_before(S, n_sep, sp.x)] = sp;
    } else if (t - m < n_sep) {
        const int32_t p = (int32_t)sep_at(S, (uint32_t)(t - m));
        items[(t - m) + spans_before(spans, n_final, p)] = make_int2(p, p);
    }
}

// Separator i0 + j ends haystack i0 + j: the result of haystack i0 + j + 1 begins where the separator's item stands
__global__ __launch_bounds__(kBatchBlock) void k_cover_batch_offsets(const int2 *__restrict__ spans, const uint64_t *__restrict__ head, BatchSeps S,
                                                                     const int64_t *__restrict__ pos, uint64_t out_pos, uint64_t *__restrict__ out_off) {
    S.base = 0; // (as in k_cover_batch_merge)
    const uint32_t j = blockIdx.x * kBatchBlock + threadIdx.x;
    if (j >= (uint32_t)head[1]) return;
    out_off[(uint64_t)S.i0 + j + 1] = out_pos + (uint64_t)pos[j + spans_before(spans, head[0], sep_at(S, j))];
}

// The item list and the plan of a batch call's piece that merged m intervals and owned [.., own_hi): enqueued, no wait.
int plan_batch(CoverCall &c, const CoverPieceIn &in, const int2 *d_spans, uint64_t own_hi, uint64_t *d_dropped) {
    DeviceState &d = c.sc.d;
    BatchSeps S;
    uint32_t i1;
    separators_in(c.h_cat_off, c.n_hay, c.done, own_hi, &S.i0, &i1);
    S.cat_off = c.d_cat_off;
    S.n_sep = i1 - S.i0;
    const uint64_t M = in.m + S.n_sep;
    c.piece_items = M;
    c.piece_max_sep = S.n_sep;
    if (!M) return ACGPU_OK;
    int rc = d.cover_items.ensure((size_t)M * 8 + 16);
    if (rc || (rc = plan_room(d, M))) return rc;
    uint64_t *head = plan_head(d);
    int2 *items = reinterpret_cast<int2 *>(d.cover_items.p);
    const hipStream_t stream = c.sc.stream;
    hipLaunchKernelGGL(k_cover_batch_head, dim3(1), dim3(1), 0, stream, in, S, c.n_hay, head);
    hipLaunchKernelGGL(k_cover_batch_merge, dim3((unsigned)((M + kBatchBlock - 1) / kBatchBlock)), dim3(kBatchBlock), 0, stream, d_spans, head, S, in.m, items);
    launch_plan(c, items, M, head, head + 1, d_dropped);
    if (S.n_sep)
        hipLaunchKernelGGL(k_cover_batch_offsets, dim3((S.n_sep + kBatchBlock - 1) / kBatchBlock), dim3(kBatchBlock), 0, stream, d_spans, head, S,
                           (const int64_t *)plan_pos(d, M), c.out_pos, c.d_out_off);
    HIP_TRY(hipGetLastError());
    return ACGPU_OK;
}

// SpansCall::planned of a batch call: in front of the piece's wait, n_final and L read from the merge's head
int plan_batch_piece(void *ctx, uint64_t *d_slot, const int2 *d_spans, uint64_t m) {
    CoverCall &c = *static_cast<CoverCall *>(ctx);
    const CoverPieceIn in{d_slot, m, (int64_t)c.n, !c.sc.piece_last};
    // A byte batch that is not all ASCII: own_hi is a unit of the shard, and the host has no map from units to v.  The plan is sized
    // by ALL phantoms not yet emitted -- L never exceeds the text's end -- at the price of at most 8 n_hay bytes of items and idle
    // lanes, and no wait.  (All ASCII: a unit is its v, and 4.24's bound holds as it stands.)
    const uint64_t own_hi = c.sc.ub && c.sc.u8->d_ckpt ? c.n : c.sc.piece_own_hi;
    return plan_batch(c, in, d_spans, own_hi, d_slot + kSpanDropped);
}

// The emit of a window of a piece's output over n_items items: the piece's final spans in d.cover_spans, or, BATCH, its item list
// in d.cover_items.  M: the items the piece's plan was sized for (where its positions begin in d.cover_plan), 0: there is none.
template <class T, int BODY, bool BATCH>
int launch_emit(CoverCall &c, uint64_t n_items, uint64_t M, uint64_t w0, uint64_t w1, void *dst) {
    DeviceState &d = c.sc.d;
    CoverArgs<T, BODY, BATCH> A;
    if constexpr (BATCH && sizeof(T) == 1) { // a byte batch: cat_off is voff
        A.voff = c.d_cat_off;
        A.n_hay = c.n_hay;
    }
    A.hay = static_cast<const T *>(c.hay);
    A.spans = reinterpret_cast<const int2 *>(BATCH ? d.cover_items.p : d.cover_spans.p);
    A.pos = (BATCH || BODY == ACGPU_COVER_DROP) && M ? plan_pos(d, M) : nullptr;
    A.n_spans = (int64_t)n_items;
    A.open = static_cast<const T *>(c.d_open);
    A.close = static_cast<const T *>(c.d_close);
    A.ol = c.ol;
    A.cl = c.cl;
    A.fill = c.fill;
    A.done = (int64_t)c.done;
    A.cut = c.piece_cut;
    A.head = c.piece_head;
    A.cap = (int32_t)std::min<int64_t>(std::max<int64_t>(tunables().cover_lds_segments.load(std::memory_order_relaxed), 0), kCoverLds);
    return launch_emit_kernel(k_cover_emit<T, BODY, BATCH>, A, w0, w1, dst, c.sc.stream);
}

// ... as the call's element, body and kind have it: one of the twelve
int launch_emit_for(CoverCall &c, uint64_t n_items, uint64_t M, uint64_t w0, uint64_t w1, void *dst) {
    auto as = [&](auto elem, auto batch) {
        using T = decltype(elem);
        constexpr bool B = decltype(batch)::value;
        return c.body == ACGPU_COVER_KEEP   ? launch_emit<T, ACGPU_COVER_KEEP, B>(c, n_items, M, w0, w1, dst)
               : c.body == ACGPU_COVER_FILL ? launch_emit<T, ACGPU_COVER_FILL, B>(c, n_items, M, w0, w1, dst)
                                            : launch_emit<T, ACGPU_COVER_DROP, B>(c, n_items, M, w0, w1, dst);
    };
    if (c.h_cat_off) return c.esz == 1 ? as(uint8_t{}, std::true_type{}) : as(uint16_t{}, std::true_type{});
    return c.esz == 1 ? as(uint8_t{}, std::false_type{}) : as(uint16_t{}, std::false_type{});
}

// ---- A FEED of a cover stream (cover_feed; acgpu_stream_cover_*, acgpu_stream.hip).  The text is the feed's buffer [carry | chunk],
// the pieces run over its owned range, and the stream cannot withhold a span that is still open at the feed's end -- the carry would
// have to reach back to its start.  So the feed's last piece, unless it is the text's, settles at B itself, L = max(done, B), and
// the first span it withheld is CUT there if it starts in front of L: it becomes the piece's last item, TAILLESS, emitted as open
// ++ body up to L.  The span stays in the carry with its true start, so the next feed's merge sees it whole; `done` then stands
// inside it (in_span), the merge's first span starts in front of `done`, and the piece that finalises it -- or cuts it again --
// emits it HEADLESS: no second open, the body from `done` on.  A carried span whose end EQUALS done (nothing touched it after
// all) is a headless item of close alone: never an empty one.  Inside a feed the pieces keep their L rule, min(B, first carried
// start), clamped to `done` while `done` stands in that very span.  What the items cost the emit: CoverArgs::cut and ::head. ----

// the emit of a feed's piece that merged m intervals and settles at L
int cover_feed_piece(CoverCall &c, uint64_t m, uint64_t L, bool cutting) {
    DeviceState &d = c.sc.d;
    const uint64_t n_final = c.sc.piece_final;
    const int2 first = c.sc.piece_carry0;
    const bool tail = cutting && c.sc.piece_carried && (int64_t)first.x < (int64_t)L;
    if (tail && (int64_t)first.y < (int64_t)L) return ACGPU_E_HIP; // (never: a withheld span ends at or behind B, and behind the `done` that cut it)
    const uint64_t n_items = n_final + (tail ? 1 : 0);
    const bool headless = c.in_span && n_items;
    if (n_items > m) return ACGPU_E_HIP; // (never: m intervals merge to at most m spans)
    const uint64_t opens = n_items - (headless ? 1 : 0), closes = n_final;
    uint64_t dropped = 0;
    if (c.body == ACGPU_COVER_DROP) {
        const uint64_t raw = m ? c.sc.piece_dropped : 0; // the plan's: the final spans' elements from `done` on, plus open's length for a headless one
        const uint64_t off = headless && n_final ? c.ol : 0;
        if (raw < off) return ACGPU_E_HIP;
        dropped = raw - off;
        if (tail) dropped += L - (uint64_t)std::max<int64_t>(first.x, (int64_t)c.done);
    }
    if (dropped > L - c.done) return ACGPU_E_HIP; // (never: the items lie in [done, L))
    const uint64_t total = (L - c.done) + opens * c.ol + closes * c.cl - dropped;
    if (tail) { // behind the final spans: their deltas sum to n_final w - raw
        int64_t *pos = c.body == ACGPU_COVER_DROP ? plan_pos(d, m) : nullptr;
        const int64_t at = std::max<int64_t>(first.x, (int64_t)c.done) - (int64_t)c.done + (int64_t)(n_final * ((uint64_t)c.ol + c.cl)) - (int64_t)c.sc.piece_dropped;
        hipLaunchKernelGGL(k_cover_tail_item, dim3(1), dim3(1), 0, c.sc.stream, reinterpret_cast<int2 *>(d.cover_spans.p), pos, n_final, first, at);
        HIP_TRY(hipGetLastError());
    }
    c.piece_cut = tail ? (int64_t)L : INT64_MAX;
    c.piece_head = headless ? (int64_t)c.ol : 0;
    const int rc = emit_piece(d, c.sc.stream, c.esz, c.d_out, c.h_out, c.cap, c.out_pos, total,
                              [&](uint64_t w0, uint64_t w1, void *dst) { return launch_emit_for(c, n_items, m, w0, w1, dst); });
    if (rc) return rc;
    c.done = L;
    c.out_pos += total;
    c.opens += opens;
    if (n_items) c.in_span = tail;
    return ACGPU_OK;
}

// SpansCall::merged: behind a piece's merge of m intervals, emit the text's elements [done, L) with the piece's final spans rewritten
int cover_piece(void *ctx, uint64_t m, bool last) {
    CoverCall &c = *static_cast<CoverCall *>(ctx);
    // (a feed's last piece that is not the text's settles at B itself and cuts the span that reaches it: A FEED below)
    const bool cutting = c.feed && c.sc.piece_range_last;
    const uint64_t n_final = c.sc.piece_final;
    uint64_t L = last ? c.n : std::min((uint64_t)std::max<int64_t>(cutting ? c.sc.piece_below : c.sc.piece_settled, 0), c.n);
    if (c.feed) L = std::max(L, c.done); // (the first carried span may be the one `done` stands in: nothing is settled then)
    if (L < c.done) return ACGPU_E_HIP; // (never: the settled position does not move backwards)
    uint64_t dropped = c.body == ACGPU_COVER_DROP ? c.sc.piece_dropped : 0;
    uint64_t n_items = n_final;
    int rc;
    if (c.feed) return cover_feed_piece(c, m, L, cutting);
    if (c.h_cat_off) { // a batch call: the separators in [done, L) are items, and none of them has output
        uint32_t i0, i1;
        separators_in(c.h_cat_off, c.n_hay, c.done, L, &i0, &i1);
        n_items += i1 - i0;
        if (m) { // planned in front of the wait (plan_batch_piece)
            if (i1 - i0 > c.piece_max_sep) return ACGPU_E_HIP; // (never: L <= own_hi)
            dropped = c.sc.piece_dropped;
        } else { // a piece without intervals has no launches of its own: its separators are planned here, n_final and L by value
            if ((rc = plan_batch(c, CoverPieceIn{nullptr, 0, (int64_t)L, 0}, nullptr, L, nullptr))) return rc;
            dropped = i1 - i0;
        }
    }
    const uint64_t added = n_final * ((uint64_t)c.ol + c.cl);
    if (dropped > L - c.done) return ACGPU_E_HIP; // (never: the final spans lie in [done, L))
    const uint64_t total = (L - c.done) + added - dropped;
    const uint64_t M = c.h_cat_off ? c.piece_items : m; // what the piece's plan, if it has one, was sized for
    rc = emit_piece(c.sc.d, c.sc.stream, c.esz, c.d_out, c.h_out, c.cap, c.out_pos, total,
                    [&](uint64_t w0, uint64_t w1, void *dst) { return launch_emit_for(c, n_items, M, w0, w1, dst); });
    if (rc) return rc;
    c.done = L;
    c.out_pos += total;
    return ACGPU_OK;
}

// The pieces of the whole text on the device, c.hay, scanned as the device shard `shard`, its units (spans_pieces, acgpu_spans.h),
// each merged, planned and emitted: what follows the last piece's wait is enqueued, not waited for.
int cover_text(CoverCall &c, const acgpu_shard &shard) {
    SpansCall &sc = c.sc;
    int rc;
    if (c.h_out && (rc = emit_slabs_ready(sc.d))) return rc;
    sc.to_pool = true;
    sc.ctx = &c;
    sc.merged = cover_piece;
    sc.planned = c.h_cat_off ? plan_batch_piece : c.body == ACGPU_COVER_DROP ? plan_dropped : nullptr;
    const bool whole = shard_rule(sc.a->t, ACGPU_REC_SET, false).sequential;
    return spans_pieces(sc, shard.chain_entry, whole, PieceScan{sc.a, sc.d, nullptr, 0, &shard, sc.stream}, shard.n_units);
}

// One text that a host entry has staged -- `hay`, n elements, on the device; `shard`, its units -- through its pieces to its end.
// c.cap, c.out_pos and the stats carry on from text to text (a batch call haystack by haystack: the next text is staged over
// this one, hence the wait).
int cover_staged_text(CoverCall &c, const void *hay, uint64_t n, const acgpu_shard &shard) {
    c.hay = hay;
    c.n = n;
    c.done = 0;
    const int rc = cover_text(c, shard);
    if (rc) return rc;
    return hipStreamSynchronize(c.sc.stream) != hipSuccess ? ACGPU_E_HIP : ACGPU_OK;
}

// what every entry returns behind its last piece
int cover_result(const CoverCall &c, uint64_t *n_out, acgpu_cover_stats *st) {
    if (st) {
        *st = acgpu_cover_stats{};
        st->n_records = c.sc.st.n_records;
        st->n_spans = c.sc.out_pos;
        st->units_out = c.out_pos;
        st->pieces = c.sc.st.pieces;
        st->rescans = c.sc.st.rescans;
        st->max_carry = c.sc.st.max_carry;
    }
    *n_out = c.out_pos;
    return c.out_pos > c.cap ? ACGPU_E_OVERFLOW : ACGPU_OK;
}

// ... and a batch call over one text behind its cover_text: the results' offsets come back, with the call's one final wait.
// (Every separator, or phantom, was an item of exactly one piece: the pieces' [done, L) tile the text.)
int cover_batch_result(const PoolCall &call, const CoverCall &c, uint64_t *out_offsets, uint64_t *n_out, acgpu_cover_stats *st) {
    if (hipMemcpyAsync(out_offsets + 1, c.d_out_off + 1, (size_t)c.n_hay * 8, hipMemcpyDeviceToHost, c.sc.stream) != hipSuccess ||
        hipStreamSynchronize(c.sc.stream) != hipSuccess)
        return call.fail(ACGPU_E_HIP);
    return cover_result(c, n_out, st);
}

// the checks all entries share, none of which needs a device; esz: bytes of an element
int check_spec(const acgpu_cover_spec *spec, uint32_t esz) {
    if (!spec || spec->body > ACGPU_COVER_DROP) return ACGPU_E_INVALID;
    if ((spec->open_len && !spec->open) || (spec->close_len && !spec->close)) return ACGPU_E_INVALID;
    if (spec->open_len >= (1u << 31) || spec->close_len >= (1u << 31)) return ACGPU_E_INVALID;
    if (spec->body == ACGPU_COVER_FILL && spec->fill >= (esz == 1 ? 0x80u : 0x10000u)) return ACGPU_E_INVALID;
    return ACGPU_OK;
}

// The body of acgpu_cover_utf8 and acgpu_cover_utf8_lossy.  P (acgpu_host.h): how the text is staged, and the entry's stats.
template <class P>
int cover_utf8(const acgpu_automaton *ca, const uint8_t *bytes, uint64_t n_bytes, const acgpu_cover_spec *spec, uint8_t *out, uint64_t cap,
               uint64_t *n_out, acgpu_cover_stats *st, typename P::Stats *ust) {
    if (!ca || !n_out || (n_bytes && !bytes) || (cap && !out)) return ACGPU_E_INVALID;
    if (n_bytes >= (1ull << 31)) return ACGPU_E_INVALID;
    int rc = check_spec(spec, 1);
    if (rc) return rc;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    *n_out = 0;
    if (st) *st = acgpu_cover_stats{};
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
    CoverCall c{SpansCall{a, d, d.call_stream}};
    c.sc.u8 = &text;
    c.esz = 1;
    c.h_out = out;
    c.cap = cap;
    if ((rc = upload_spec(c, *spec))) return call.fail(rc);
    if ((rc = cover_staged_text(c, text.d_bytes, n_bytes, text.shard))) return call.fail(rc);
    return cover_result(c, n_out, st);
}

// The body of acgpu_cover_batch_utf8 and acgpu_cover_batch_utf8_lossy.  The batch is staged as acgpu_replace_batch_utf8 stages it
// and scanned as ONE device shard, whose units have a separator behind every haystack; the caller's bytes have none.  Merge, plan
// and emit therefore run over VIRTUAL COORDINATES -- v = byte of the span + index of the haystack: the bytes with a phantom
// element behind every haystack.  With voff in the place of cat_off everything of "a batch call" above runs
// unchanged: a phantom is an item {p, p} with delta -1 that emits nothing and skips one element, and a result's first output
// byte is read off the plan at its phantom.  Only the emit's source knows that the phantoms are not there (CoverShift).
template <class P>
int cover_batch_utf8(const acgpu_automaton *ca, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks, const acgpu_cover_spec *spec,
                     uint8_t *out, uint64_t cap, uint64_t *out_offsets, uint64_t *n_out, acgpu_cover_stats *st, typename P::Stats *ust) {
    if (!ca || !offsets || !n_out || !out_offsets || (cap && !out)) return ACGPU_E_INVALID;
    int rc = check_spec(spec, 1);
    if (rc) return rc;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    const HostTables &t = a->t;
    BatchPlan plan; // (in bytes: bytes >= units, so bytes + haystacks < 2^31 bounds the text the scan sees, and the virtual text)
    if ((rc = check_batch(t, reinterpret_cast<const uint16_t *>(bytes), offsets, n_haystacks, &plan))) return rc;
    *n_out = 0;
    out_offsets[0] = 0;
    if (st) *st = acgpu_cover_stats{};
    if (ust) *ust = P::stats();
    if (plan.total == 0) { // (nothing to decode and nothing to rewrite: no device needed)
        for (uint32_t i = 0; i < n_haystacks; i++) out_offsets[i + 1] = 0;
        return ACGPU_OK;
    }
    PoolCall call(a); // (no device: fails here, and out is untouched)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    Utf8Batch b;
    if ((rc = utf8_batch_front<P>(call, t, bytes, offsets, n_haystacks, plan, &b, ust))) return rc; // (ACGPU_E_ENCODING: out and out_offsets[1..] untouched)
    CoverCall c{SpansCall{a, d, d.call_stream}};
    c.esz = 1;
    c.h_out = out;
    c.cap = cap;
    if ((rc = upload_spec(c, *spec))) return call.fail(rc);
    if (plan.per_haystack) { // every haystack by the route acgpu_cover_utf8 takes, the results back to back
        rc = utf8_each_haystack<P>(
            d, bytes, offsets, n_haystacks, c.sc.stream,
            [&](uint32_t i, const Utf8Text &text) {
                c.sc.u8 = &text;
                const int prc = cover_staged_text(c, text.d_bytes, offsets[i + 1] - offsets[i], text.shard);
                c.sc.u8 = nullptr;
                return prc;
            },
            [&](uint32_t i) { out_offsets[i + 1] = c.out_pos; });
        if (rc) return call.fail(rc);
        return cover_result(c, n_out, st);
    }
    std::vector<uint32_t> h_voff;
    if ((rc = utf8_virtual_offsets(d, b, c.sc.stream, &h_voff, &c.d_cat_off))) return call.fail(rc);
    if ((rc = d.replace_off.ensure(((size_t)n_haystacks + 1) * 8))) return call.fail(rc);
    c.sc.u8 = &b.text;
    c.sc.ub = &b;
    c.hay = b.text.d_bytes;
    c.n = plan.total + n_haystacks;
    c.h_cat_off = h_voff.data();
    c.n_hay = n_haystacks;
    c.d_out_off = reinterpret_cast<uint64_t *>(d.replace_off.p);
    {
        SeparatorScan sep(d, t);
        rc = cover_text(c, b.text.shard);
    }
    if (rc) return call.fail(rc);
    return cover_batch_result(call, c, out_offsets, n_out, st);
}

} // namespace

namespace acgpu {

int cover_check_spec(const acgpu_cover_spec *spec, uint32_t esz) { return check_spec(spec, esz); }

// One feed of a cover stream (A FEED above): the pieces of the buffer's owned range behind f->done, as a text's pieces are driven
// -- the spec is uploaded per feed and the carried spans come from and go back to the host, so nothing of the stream stays on the
// device between two feeds.
int cover_feed(acgpu_automaton *a, DeviceState &d, CoverFeed *f, const acgpu_cover_spec *spec, void *out, uint64_t cap, uint64_t *n_out) {
    CoverCall c{SpansCall{a, d, d.call_stream}};
    c.esz = f->u8 ? 1 : 2;
    c.sc.u8 = f->u8;
    c.hay = f->u8 ? static_cast<const void *>(f->u8->d_bytes) : static_cast<const void *>(f->shard.d_hay);
    c.n = f->u8 ? f->u8->n_bytes : f->shard.n_units;
    c.h_out = static_cast<uint8_t *>(out);
    c.cap = cap;
    c.done = f->done;
    c.feed = true;
    c.in_span = f->in_span;
    if (c.done > c.n) return ACGPU_E_HIP; // (never: the carry reaches back to `done`, the stream checks it)
    int rc = upload_spec(c, *spec);
    if (rc || (rc = emit_slabs_ready(d))) return rc;
    // the carried spans, buffer relative.  A start far in front of the buffer is clamped: all that a span which began in an
    // earlier feed is asked for is that it starts in front of `done`, and its end.
    constexpr int64_t kFarFront = -(1ll << 30);
    std::vector<int2> carry_in;
    try {
        carry_in.resize(f->carried.size() / 2);
    } catch (...) {
        return ACGPU_E_NOMEM;
    }
    for (size_t i = 0; i < carry_in.size(); ++i) {
        const int64_t s = f->carried[2 * i] - (int64_t)f->origin, e = f->carried[2 * i + 1] - (int64_t)f->origin;
        if (e < 0 || e > (int64_t)c.n || s >= e) return ACGPU_E_HIP; // (never: a carried span ends inside the carried text)
        carry_in[i] = make_int2((int32_t)std::max(s, kFarFront), (int32_t)e);
    }
    const ShardRule rule = shard_rule(a->t, ACGPU_REC_SET, /*readable=*/true);
    const int64_t entry = piece_entry(rule, f->chain, 0, f->shard.own_begin);
    const int64_t idle_exit = piece_exit(rule, entry, f->shard.own_end, nullptr, 0); // (nothing owned: nothing scanned)
    acgpu_shard sh = f->shard;
    sh.chain_entry = entry;
    SpansRange range;
    range.own_begin = sh.own_begin;
    range.own_end = sh.own_end;
    range.text_end = f->final;
    range.carry_in = carry_in.data();
    range.n_carry_in = (uint32_t)carry_in.size();
    SpansCall &sc = c.sc;
    sc.to_pool = true;
    sc.ctx = &c;
    sc.merged = cover_piece;
    sc.planned = c.body == ACGPU_COVER_DROP ? plan_dropped : nullptr;
    rc = spans_pieces(sc, f->chain, rule.sequential, PieceScan{a, d, nullptr, 0, &sh, sc.stream, /*readable=*/true}, sh.n_units, &range);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(sc.stream));
    std::vector<int64_t> carried;
    try {
        carried.reserve(range.carry_out.size() * 2);
    } catch (...) {
        return ACGPU_E_NOMEM;
    }
    for (const int2 &sp : range.carry_out) {
        carried.push_back((int64_t)sp.x + (int64_t)f->origin);
        carried.push_back((int64_t)sp.y + (int64_t)f->origin);
    }
    f->carried.swap(carried);
    f->done = c.done;
    f->in_span = c.in_span;
    f->chain = range.scanned ? range.chain_exit : idle_exit;
    f->st = acgpu_cover_stats{};
    f->st.n_records = sc.st.n_records;
    f->st.n_spans = c.opens;
    f->st.units_out = c.out_pos;
    f->st.pieces = sc.st.pieces;
    f->st.rescans = sc.st.rescans;
    f->st.max_carry = sc.st.max_carry;
    *n_out = c.out_pos;
    return c.out_pos > c.cap ? ACGPU_E_OVERFLOW : ACGPU_OK;
}

} // namespace acgpu

extern "C" {

int acgpu_cover_u16(const acgpu_automaton *ca, const uint16_t *haystack, uint64_t n_units, const acgpu_cover_spec *spec, uint16_t *out, uint64_t cap,
                    uint64_t *n_out, acgpu_cover_stats *st) {
    if (!ca || !n_out || (n_units && !haystack) || (cap && !out)) return ACGPU_E_INVALID;
    if (n_units >= (1ull << 31)) return ACGPU_E_INVALID;
    int rc = check_spec(spec, 2);
    if (rc) return rc;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    PoolCall call(a); // (no device: fails here, as acgpu_match_u16 does, and out is untouched)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    if ((rc = call.idle())) return rc; // (the text is staged by a blocking copy: the NULL stream, see the stream rule)
    acgpu_shard sh;
    if ((rc = stage_whole_text(d, haystack, n_units, &sh))) return call.fail(rc); // the whole text, once: see the head of this file
    CoverCall c{SpansCall{a, d, d.call_stream}};
    c.h_out = reinterpret_cast<uint8_t *>(out);
    c.cap = cap;
    if ((rc = upload_spec(c, *spec))) return call.fail(rc);
    if ((rc = cover_staged_text(c, sh.d_hay, n_units, sh))) return call.fail(rc);
    return cover_result(c, n_out, st);
}

int acgpu_cover_device(const acgpu_automaton *ca, acgpu_shard *shard, const acgpu_cover_spec *spec, uint16_t *d_out, uint64_t cap, uint64_t *n_out,
                       void *stream_, acgpu_cover_stats *st) {
    if (!ca || !shard || !n_out || (cap && !d_out) || ((uintptr_t)d_out & 1)) return ACGPU_E_INVALID;
    if (shard->n_units >= (1ull << 31) || (shard->n_units && !shard->d_hay) || ((uintptr_t)shard->d_hay & 15)) return ACGPU_E_INVALID;
    int rc = check_spec(spec, 2);
    if (rc) return rc;
    // one shard of a sharded text: the spans it withholds would have to travel to the rank behind it -- not built
    if (!shard_is_whole_text(*shard)) return ACGPU_E_UNSUPPORTED;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    PoolCall call(a);
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    const hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if ((rc = call.on(stream))) return rc;
    CoverCall c{SpansCall{a, d, stream}};
    c.hay = shard->d_hay;
    c.n = shard->n_units;
    c.d_out = reinterpret_cast<uint8_t *>(d_out);
    c.cap = cap;
    if ((rc = upload_spec(c, *spec))) return rc;
    rc = cover_text(c, *shard);
    const hipError_t e = hipStreamSynchronize(stream); // the final wait
    if (rc) return rc;
    HIP_TRY(e);
    return cover_result(c, n_out, st);
}

int acgpu_cover_batch_u16(const acgpu_automaton *ca, const uint16_t *units, const uint64_t *offsets, uint32_t n_haystacks, const acgpu_cover_spec *spec,
                          uint16_t *out, uint64_t cap, uint64_t *out_offsets, uint64_t *n_out, acgpu_cover_stats *st) {
    if (!ca || !offsets || !n_out || !out_offsets || (cap && !out)) return ACGPU_E_INVALID;
    int rc = check_spec(spec, 2);
    if (rc) return rc;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    const HostTables &t = a->t;
    BatchPlan plan;
    if ((rc = check_batch(t, units, offsets, n_haystacks, &plan))) return rc;
    *n_out = 0;
    out_offsets[0] = 0;
    if (st) *st = acgpu_cover_stats{};
    if (n_haystacks == 0) return ACGPU_OK;
    PoolCall call(a); // (no device: fails here, and out is untouched)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    if ((rc = call.idle())) return rc; // (the text is staged by a blocking copy: the NULL stream, see the stream rule)
    CoverCall c{SpansCall{a, d, d.call_stream}};
    c.h_out = reinterpret_cast<uint8_t *>(out);
    c.cap = cap;
    if ((rc = upload_spec(c, *spec))) return call.fail(rc);
    acgpu_shard sh;
    if (plan.per_haystack) { // every haystack by the route acgpu_cover_u16 takes, the results back to back
        for (uint32_t i = 0; i < n_haystacks; i++) {
            const uint64_t len = offsets[i + 1] - offsets[i];
            if (len) {
                if ((rc = stage_whole_text(d, units + offsets[i], len, &sh))) return call.fail(rc);
                if ((rc = cover_staged_text(c, sh.d_hay, len, sh))) return call.fail(rc);
            }
            out_offsets[i + 1] = c.out_pos;
        }
        return cover_result(c, n_out, st);
    }
    BatchText text(d, t); // (d.start_behind is the separator until this returns, whichever way)
    if ((rc = text.stage(units, offsets, n_haystacks, c.sc.stream))) return call.fail(rc);
    if ((rc = stage_whole_text(d, text.h_cat, text.cat, &sh))) return call.fail(rc); // the whole concatenation, once: as acgpu_cover_u16
    if ((rc = d.replace_off.ensure(((size_t)n_haystacks + 1) * 8))) return call.fail(rc);
    c.hay = sh.d_hay;
    c.n = text.cat;
    c.h_cat_off = text.h_off;
    c.d_cat_off = text.d_off();
    c.n_hay = n_haystacks;
    c.d_out_off = reinterpret_cast<uint64_t *>(d.replace_off.p);
    if ((rc = cover_text(c, sh))) return call.fail(rc);
    return cover_batch_result(call, c, out_offsets, n_out, st);
}

int acgpu_cover_utf8(const acgpu_automaton *a, const uint8_t *bytes, uint64_t n_bytes, const acgpu_cover_spec *spec, uint8_t *out, uint64_t cap,
                     uint64_t *n_out, acgpu_cover_stats *st, acgpu_utf8_stats *ust) {
    return cover_utf8<Utf8StrictText>(a, bytes, n_bytes, spec, out, cap, n_out, st, ust);
}

int acgpu_cover_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, uint64_t n_bytes, const acgpu_cover_spec *spec, uint8_t *out, uint64_t cap,
                           uint64_t *n_out, acgpu_cover_stats *st, acgpu_utf8_lossy_stats *ust) {
    return cover_utf8<Utf8LossyText>(a, bytes, n_bytes, spec, out, cap, n_out, st, ust);
}

int acgpu_cover_batch_utf8(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks, const acgpu_cover_spec *spec,
                           uint8_t *out, uint64_t cap, uint64_t *out_offsets, uint64_t *n_out, acgpu_cover_stats *st, acgpu_utf8_batch_stats *ust) {
    return cover_batch_utf8<Utf8StrictBatch>(a, bytes, offsets, n_haystacks, spec, out, cap, out_offsets, n_out, st, ust);
}

int acgpu_cover_batch_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                                 const acgpu_cover_spec *spec, uint8_t *out, uint64_t cap, uint64_t *out_offsets, uint64_t *n_out, acgpu_cover_stats *st,
                                 acgpu_utf8_lossy_stats *ust) {
    return cover_batch_utf8<Utf8LossyBatch>(a, bytes, offsets, n_haystacks, spec, out, cap, out_offsets, n_out, st, ust);
}

} // extern "C"
