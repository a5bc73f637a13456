// acgpu_emit.h -- what the two emit kernels (k_replace_emit, acgpu_replace.hip; k_cover_emit, acgpu_cover.hip) and the plans in
// front of them share: the tile shape, the 16-byte load at any alignment, the search over ascending output positions, the 64-bit
// block scan, and the host entries' way out through two slabs.
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

// The last index i in [lo, hi) with pos[i] <= x, lo - 1 if there is none (pos ascends; equal positions: deleted matches that
// touch each other).
__device__ __forceinline__ int64_t last_at_or_before(const int64_t *__restrict__ pos, int64_t lo, int64_t hi, int64_t x) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (pos[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
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

} // namespace acgpu
