// acgpu_emit.h -- the rewrite family's device and host code that does not depend on what an output is made of: the 64-bit plan
// over a piece's items, the emit of a window of a piece's output from a SOURCE, and a piece's way out, straight to the caller's
// device memory or to the host through two slabs.  k_replace_emit (acgpu_replace.hip) and k_cover_emit (acgpu_cover.hip) are this
// emit over their sources; the six plan kernels are the three levels below over their items.  And the separators of a batch call,
// which both merge into a piece's list: their descriptor, the two searches of the rank merge, the host's range of them.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "acgpu_device.h"
#include "acgpu_host.h"

namespace acgpu {

typedef uint32_t rp_v4u __attribute__((ext_vector_type(4)));

constexpr int kPlanBlock = 256, kPlanPer = 8, kPlanTile = kPlanBlock * kPlanPer; // records per workgroup of a plan
constexpr int kEmitBlock = 256;                                                  // lanes of a workgroup of an emit: one 16-byte store each

// An output ELEMENT is what the text is made of as the caller sees it: a UTF-16 unit (T = uint16_t), or a byte of a UTF-8 text
// (T = uint8_t).
template <class T>
constexpr int kEmitPer = 16 / (int)sizeof(T); // elements of a lane's store: 8 units or 16 bytes
template <class T>
constexpr int kEmitTile = kEmitBlock * kEmitPer<T>; // ... of a workgroup: 2048 units or 4096 bytes

__device__ __forceinline__ int64_t plan_block_scan(int64_t v, int64_t *total) { // exclusive, kPlanBlock threads
    __shared__ int64_t wsum[kPlanBlock / kWave];
    const int64_t inc = wave_inclusive_scan(v);
    const int w = threadIdx.x / kWave;
    if (lane_id() == kWave - 1) wsum[w] = inc;
    __syncthreads();
    int64_t base = 0, all = 0;
    for (int i = 0; i < kPlanBlock / kWave; ++i) {
        if (i < w) base += wsum[i];
        all += wsum[i];
    }
    *total = all;
    __syncthreads();
    return base + inc - v;
}

// THE PLAN: the exclusive 64-bit prefix sums of item(i), i < n, in two levels -- a workgroup per kPlanTile items, a thread per
// kPlanPer consecutive ones.  A kernel of a level says what an item adds, where n comes from and what is written.
// level 1: bsum[workgroup] = the sum of the workgroup's items
template <class Item>
__device__ __forceinline__ void plan_sums(Item item, uint64_t n, int64_t *__restrict__ bsum) {
    const uint64_t first = (uint64_t)blockIdx.x * kPlanTile + (uint64_t)threadIdx.x * kPlanPer;
    int64_t v = 0;
    for (int k = 0; k < kPlanPer; ++k)
        if (first + k < n) v += item(first + k);
    int64_t total;
    plan_block_scan(v, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// level 2: ONE workgroup scans the workgroups' sums in place (exclusive), kPlanBlock per step with a running carry; returns the
// sum of all items
__device__ __forceinline__ int64_t plan_offsets(int64_t *__restrict__ bsum, uint32_t n_blocks) {
    int64_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += kPlanBlock) {
        const uint32_t b = b0 + threadIdx.x;
        const int64_t v = b < n_blocks ? bsum[b] : 0;
        int64_t total;
        const int64_t ex = plan_block_scan(v, &total);
        if (b < n_blocks) bsum[b] = carry + ex;
        carry += total;
    }
    return carry;
}

// level 3: put(i, the sum of the items in front of i) for every i < n -- the items again, behind the workgroup's base
template <class Item, class Put>
__device__ __forceinline__ void plan_positions(Item item, uint64_t n, const int64_t *__restrict__ bsum, Put put) {
    const uint64_t first = (uint64_t)blockIdx.x * kPlanTile + (uint64_t)threadIdx.x * kPlanPer;
    int64_t it[kPlanPer], v = 0;
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        it[k] = first + k < n ? item(first + k) : 0;
        v += it[k];
    }
    int64_t total;
    int64_t run = plan_block_scan(v, &total) + bsum[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
        if (first + k < n) put(first + k, run);
        run += it[k];
    }
}

// THE SEPARATORS of a batch call, whose text is the haystacks' concatenation with a separator element behind each (cat_off[i] =
// the first element of haystack i in it; a byte batch: the phantoms, voff).  A piece merges those in a range of the text with its
// own list -- replace: records, the separator a match that is deleted (k_replace_merge); cover: final spans, the separator an item
// that emits nothing (k_cover_batch_merge) -- by rank: both lists ascend and cannot tie, so an element's place is its index plus
// the elements of the other list in front of it, one binary search per element.
// Separator j of a piece is separator i0 + j of the text and stands at text position cat_off[i0 + j + 1] - 1; `base` = the text
// position of element 0 of the buffer the piece's list is relative to.
struct BatchSeps {
    const uint32_t *cat_off = nullptr;
    uint32_t i0 = 0, n_sep = 0;
    int64_t base = 0;
};

__device__ __forceinline__ int64_t sep_at(const BatchSeps &S, uint32_t j) { return (int64_t)S.cat_off[S.i0 + j + 1] - 1 - S.base; } // buffer relative

// the first n separators of S that stand in front of buffer position x
__device__ __forceinline__ uint32_t seps_before(const BatchSeps &S, uint32_t n, int64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (sep_at(S, mid) < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the first n elements of a list of ascending starts -- start(i) -- that start in front of p
template <class Start>
__device__ __forceinline__ uint64_t starts_before(Start start, uint64_t n, int64_t p) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)start(mid) < p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// on the host: separator i stands at h_cat_off[i + 1] - 1, and the separators in the text's [lo, hi) are [*i0, *i1)
inline void separators_in(const uint32_t *h_cat_off, uint32_t n_hay, uint64_t lo, uint64_t hi, uint32_t *i0, uint32_t *i1) {
    const uint32_t *sep_end = h_cat_off + 1; // at or behind x <=> sep_end[i] > x
    *i0 = (uint32_t)(std::upper_bound(sep_end, sep_end + n_hay, lo) - sep_end);
    *i1 = std::max(*i0, (uint32_t)(std::upper_bound(sep_end, sep_end + n_hay, hi) - sep_end));
}

// The 16 consecutive bytes from p -- 8 units at any 2-byte alignment, or 16 bytes at any address -- as one 16-byte value: the two
// aligned 16-byte words around them and a funnel shift by sh = p's offset into the first, in bytes (units: even).  Only 16-byte
// words that hold one of the wanted bytes are read, so nothing beyond the page of a valid element.
template <class T>
__device__ __forceinline__ rp_v4u load16(const T *p) {
    const uintptr_t a = (uintptr_t)p;
    const uint32_t sh = (uint32_t)a & 15u;
    const rp_v4u *q = reinterpret_cast<const rp_v4u *>(a & ~(uintptr_t)15);
    const rp_v4u lo = q[0];
    if (sh == 0) return lo;
    const rp_v4u hi = q[1];
    uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    if (sh & 8u) {
#pragma unroll
        for (int j = 0; j < 6; ++j) w[j] = w[j + 2];
    }
    if (sh & 4u) {
#pragma unroll
        for (int j = 0; j < 7; ++j) w[j] = w[j + 1];
    }
    if (sizeof(T) == 2) {
        if (sh & 2u) {
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = (w[j] >> 16) | (w[j + 1] << 16);
        }
    } else { // the low bytes of the shift: each word from itself and its neighbour, {w[j + 1], w[j]} >> 8 (sh & 3)
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], sh & 3u);
    }
    rp_v4u r;
    r.x = w[0]; r.y = w[1]; r.z = w[2]; r.w = w[3];
    return r;
}

// THE EMIT writes the window [w0, w1) of a piece's output to dst.  The output is the text with n() ITEMS spliced in -- replace: a
// record's replacement; cover: a span's open ++ body ++ close -- and item i begins at output position pos_at(i), which ascends with
// i (weakly will do: items without output between them share a position).  A SEGMENT is the stretch of the output from one item's
// position to the next one's, tile relative: u = an output element minus t0, the tile's first; segment -1 is the text in front of
// item 0.  A source S -- the kernel's argument struct -- provides
//   S::Elem               the output's element: a UTF-16 unit, or a byte of a UTF-8 text
//   S::Seg                a segment: `int32_t rel`, where it begins (-1: at or in front of the tile's first element), and where each
//                         of its sources ends and is read from, as offsets to add to u (modulo 2^32; what they are used for
//                         lies below 2^31)
//   S::kLds, lds_cap()    the segments a workgroup has room for in LDS, and stages at most
//   w0, w1, dst           the window, and where output element w0 goes
//   n(), pos_at(i)        the items
//   make_seg(i, t0)       the segment of item i, i = -1 included
//   whole(seg, u0, &v)    if ONE source of seg holds the elements u0 .. u0 + kEmitPer - 1, that vector (a load16, or a constant)
//   element(seg, u)       element u of seg
//
// Tiles are laid over the DESTINATION's 16-byte grid: v = o - w0 + (dst's misalignment in elements), tile b = the v in
// [b * kEmitTile, + kEmitTile), lane l of it the kEmitPer elements -- 8 units, or 16 bytes -- of one aligned 16-byte store, wherever
// dst points (a source is read at any alignment: load16).  A vector that the window covers only in part (the window's first and
// last) is written element by element, so nothing outside [w0, w1) -- nothing at or beyond the caller's capacity -- is touched.
// The items that touch a tile are found by two binary searches over pos_at; their segments go to LDS when they fit (they do unless
// thousands of items without output between them fall into one tile), else every lane takes them from global memory: the same code
// over another view.  A lane finds the segment of its first element by binary search and walks on from there (a few steps, then a
// search again).

// The last item i with pos_at(i) <= x, -1 if there is none.
template <class S>
__device__ __forceinline__ int64_t last_at_or_before(const S &A, int64_t x) {
    int64_t lo = 0, hi = A.n();
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (A.pos_at(mid) <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// a lane's vector of the tile at t0, whose segments are the n_seg from item i0 on: lseg (kLds), or made as they are read
template <class S, bool kLds>
__device__ __forceinline__ void emit_tile(const S &A, const typename S::Seg *lseg, int64_t t0, int64_t i0, int64_t cnt) {
    const int64_t n_seg = kLds ? (int64_t)(int32_t)cnt : cnt; // (what LDS holds is counted in 32 bits, and the searches know it)
    using T = typename S::Elem;
    using Seg = typename S::Seg;
    auto rel_at = [&](int64_t j) -> int64_t {
        if (kLds) return lseg[j].rel;
        const int64_t i = i0 + j;
        return i < 0 ? -1 : std::max<int64_t>(A.pos_at(i) - t0, -1);
    };
    auto seg_at = [&](int64_t j) -> Seg { return kLds ? lseg[j] : A.make_seg(i0 + j, t0); };
    auto find = [&](int64_t from, int32_t u) -> int64_t { // the last segment j >= from with rel <= u (segment `from` has)
        int64_t lo = from + 1, hi = n_seg;
        for (int step = 0; step < 4 && lo < hi; ++step) {
            if (rel_at(lo) > u) return lo - 1;
            ++lo;
        }
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (rel_at(mid) <= u) lo = mid + 1;
            else hi = mid;
        }
        return lo - 1;
    };
    constexpr int kPer = kEmitPer<T>, kPerWord = 4 / (int)sizeof(T);
    const int32_t u0 = (int32_t)threadIdx.x * kPer;
    const int64_t o_first = t0 + u0;
    if (o_first >= A.w1 || o_first + kPer <= A.w0) return;
    const int32_t ua = (int32_t)std::max<int64_t>(A.w0 - o_first, 0), ub = (int32_t)std::min<int64_t>(A.w1 - o_first, kPer); // the lane's valid elements [ua, ub)
    T *out = A.dst + (o_first - A.w0);
    int64_t j = find(0, u0 + ua);
    Seg s = seg_at(j);
    const bool full = ua == 0 && ub == kPer;
    rp_v4u v;
    if (full && (j + 1 >= n_seg || rel_at(j + 1) > u0 + kPer - 1) && A.whole(s, u0, &v)) { // one source of one segment holds the vector
        __builtin_nontemporal_store(v, reinterpret_cast<rp_v4u *>(out));
        return;
    }
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        if (k >= ua && k < ub) {
            const int32_t u = u0 + k;
            if (k > ua) {
                const int64_t jn = find(j, u);
                if (jn != j) {
                    j = jn;
                    s = seg_at(j);
                }
            }
            const uint32_t x = A.element(s, u);
            if (full) w[k / kPerWord] |= x << (8 * (int)sizeof(T) * (k % kPerWord));
            else out[k] = (T)x;
        }
    }
    if (full) {
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        __builtin_nontemporal_store(v, reinterpret_cast<rp_v4u *>(out));
    }
}

// a workgroup's tile: the body of an emit kernel
template <class S>
__device__ __forceinline__ void emit_block(const S &src) {
    // a copy, so that the source's pointers are values in registers: read through the reference to the kernel's argument, a choice
    // between two of them (element(): open, text or close) compiles to a choice between their ADDRESSES and a load of the pointer
    // from the argument segment for every element written
    const S A = src;
    using T = typename S::Elem;
    __shared__ typename S::Seg lseg[S::kLds];
    __shared__ int64_t bounds[2];
    const int64_t mis = (int64_t)(((uintptr_t)A.dst & 15u) / sizeof(T));
    const int64_t t0 = A.w0 - mis + (int64_t)blockIdx.x * kEmitTile<T>;
    const int64_t ov0 = std::max(t0, A.w0), ov1 = std::min(t0 + kEmitTile<T>, A.w1); // the tile's elements of the window
    if (ov0 >= ov1) return;
    if (threadIdx.x == 0) bounds[0] = last_at_or_before(A, ov0);
    if (threadIdx.x == kWave) bounds[1] = last_at_or_before(A, ov1 - 1);
    __syncthreads();
    const int64_t i0 = bounds[0], cnt = bounds[1] - i0 + 1; // segments i0 .. bounds[1]
    if (cnt <= (int64_t)A.lds_cap()) {
        for (int32_t j = (int32_t)threadIdx.x; j < (int32_t)cnt; j += kEmitBlock) lseg[j] = A.make_seg(i0 + j, t0);
        __syncthreads();
        emit_tile<S, true>(A, lseg, t0, i0, cnt);
    } else {
        emit_tile<S, false>(A, lseg, t0, i0, cnt);
    }
}

// The launch of an emit kernel `k` over source A for the window [w0, w1) to the device address dst: a workgroup per tile of dst's grid.
template <class S>
int launch_emit_kernel(void (*k)(S), S &A, uint64_t w0, uint64_t w1, void *dst, hipStream_t stream) {
    using T = typename S::Elem;
    A.w0 = (int64_t)w0;
    A.w1 = (int64_t)w1;
    A.dst = static_cast<T *>(dst);
    const uint64_t mis = ((uintptr_t)dst & 15u) / sizeof(T);
    const uint64_t tiles = (w1 - w0 + mis + kEmitTile<T> - 1) / kEmitTile<T>;
    hipLaunchKernelGGL(k, dim3((unsigned)tiles), dim3(kEmitBlock), 0, stream, A);
    HIP_TRY(hipGetLastError());
    return ACGPU_OK;
}

// what emit_through_slabs needs of the pool: the copy stream and the four events
inline int emit_slabs_ready(DeviceState &d) {
    if (!d.copy_stream) HIP_TRY(hipStreamCreateWithFlags(&d.copy_stream.h, hipStreamNonBlocking));
    for (auto &e : d.replace_ev)
        if (!e) HIP_TRY(hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
    return ACGPU_OK;
}

// A host entry's way out: emit_total elements of esz bytes to h_dst through two slabs of the pool -- slab k is copied to the
// caller's memory (on the copy stream) while slab k + 1 is emitted.  launch(w0, w1, dst) enqueues on `stream` the emit of the
// window [w0, w1) of the piece's output to the device address dst.  A slab is a whole number of 16-byte vectors -- 8 units, or 16
// bytes -- so that both slabs start 16-byte aligned.  Returns with both streams idle.
template <class Launch>
int emit_through_slabs(DeviceState &d, hipStream_t stream, uint32_t esz, uint8_t *h_dst, uint64_t emit_total, Launch launch) {
    const uint64_t vec = 16 / esz;
    const uint64_t slab = (std::min<uint64_t>((uint64_t)std::max<int64_t>(8, tunables().replace_slab_units.load(std::memory_order_relaxed)), emit_total) + vec - 1) & ~(vec - 1);
    int rc = d.replace_slab.ensure(slab * 2 * esz + 32);
    if (rc) return rc;
    uint8_t *buf[2] = {reinterpret_cast<uint8_t *>(d.replace_slab.p), reinterpret_cast<uint8_t *>(d.replace_slab.p) + slab * esz};
    bool copied[2] = {false, false};
    auto copy_out = [&](int b, uint64_t w0, uint64_t w1) -> int {
        HIP_TRY(hipStreamWaitEvent(d.copy_stream, d.replace_ev[b], 0));
        HIP_TRY(hipMemcpyAsync(h_dst + w0 * esz, buf[b], (w1 - w0) * esz, hipMemcpyDeviceToHost, d.copy_stream));
        HIP_TRY(hipEventRecord(d.replace_ev[2 + b], d.copy_stream));
        copied[b] = true;
        return ACGPU_OK;
    };
    uint64_t prev0 = 0, prev1 = 0;
    int k = 0;
    for (uint64_t w0 = 0; w0 < emit_total; w0 += slab, ++k) {
        const uint64_t w1 = std::min(emit_total, w0 + slab);
        const int b = k & 1;
        if (copied[b]) HIP_TRY(hipStreamWaitEvent(stream, d.replace_ev[2 + b], 0)); // (the slab has left for the host)
        if ((rc = launch(w0, w1, static_cast<void *>(buf[b])))) return rc;
        HIP_TRY(hipEventRecord(d.replace_ev[b], stream));
        if (k > 0 && (rc = copy_out(b ^ 1, prev0, prev1))) return rc;
        prev0 = w0;
        prev1 = w1;
    }
    if ((rc = copy_out((k - 1) & 1, prev0, prev1))) return rc;
    HIP_TRY(hipStreamSynchronize(d.copy_stream));
    HIP_TRY(hipStreamSynchronize(stream)); // (the next piece's text overwrites d.stage_hay from the copy stream)
    return ACGPU_OK;
}

// A piece's way out: its output is `total` elements of esz bytes behind the out_pos the call has counted so far, and what of them
// lies below cap is written -- beyond cap: planned, not written -- straight to d_out, or, d_out == nullptr, to h_out through the
// slabs.  launch as emit_through_slabs has it.
template <class Launch>
int emit_piece(DeviceState &d, hipStream_t stream, uint32_t esz, uint8_t *d_out, uint8_t *h_out, uint64_t cap, uint64_t out_pos, uint64_t total,
               Launch launch) {
    const uint64_t room = cap > out_pos ? cap - out_pos : 0, emit_total = std::min(total, room);
    if (!emit_total) return ACGPU_OK;
    if (d_out) return launch(0, emit_total, static_cast<void *>(d_out + out_pos * esz));
    return emit_through_slabs(d, stream, esz, h_out + out_pos * esz, emit_total, launch);
}

} // namespace acgpu
