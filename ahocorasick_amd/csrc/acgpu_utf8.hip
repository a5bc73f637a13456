// acgpu_utf8.hip -- acgpu_match_utf8 (include/acgpu.h): a UTF-8 haystack validated and transcoded on the device, scanned as the
// one shard acgpu_match_u16 would scan, its records rewritten to byte offsets of the caller's buffer.
//
// Four kernels around the unchanged scan (match_shard):
//   k_utf8_count : a lane per 16 bytes: validates them strictly and counts the UTF-16 units they decode to; one sum per block of
//                  4096 bytes, the smallest offending offset into one 64-bit atomicMin;
//   k_utf8_scan  : one workgroup: the block sums become block bases, their total n_units;
//   k_utf8_write : the same lanes again (after the host has seen n_units and that nothing offends): every lead byte decodes its
//                  code point and stores one or two units, and the lane of a unit whose index is a multiple of 32 stores where
//                  that unit's sequence begins -- the checkpoint table, 4 bytes per 32 units;
//   k_utf8_map   : a lane per record: start and end - 1 go from units to bytes through the nearest checkpoint at or below them
//                  and a walk of at most 31 units over the lead bytes.
// For acgpu_replace_utf8 (acgpu_replace.hip) the front end and k_utf8_map are host functions of their own (stage_utf8_text,
// utf8_map_records), and k_utf8_pos maps one unit position -- a piece's boundary -- the same way (utf8_map_position).
// What a lane knows about its 16 bytes is eleven bit masks over a window of 24 bytes (the 4 before, its own, the 4 behind), built
// by one function that both passes over the text share, so they cannot disagree about a count.
#include <hip/hip_runtime.h>

#include "acgpu_device.h"
#include "acgpu_host.h"
#include "acgpu_internal.h"

using namespace acgpu;

namespace {

constexpr int kU8Threads = 256;
constexpr uint32_t kU8Lane = 16;                     // bytes per lane
constexpr uint32_t kU8Block = kU8Threads * kU8Lane;  // bytes per workgroup: 4096
constexpr uint32_t kU8Own = 0x000ffff0u;             // the window's bits of a lane's own bytes
constexpr uint32_t kCkptLow = 0x80000000u;           // checkpoint flag: the unit is the low surrogate of the sequence named

static_assert(sizeof(acgpu_utf8_stats) == 24, "the layout include/acgpu.h promises");

// What a lane knows about its bytes.  Bit k of a mask stands for the byte at offset o - 4 + k of the text, o the lane's first.
struct LaneView {
    uint32_t w[6];   // the window's bytes, zero where the text has none (before its begin, at and behind its end)
    uint32_t lead;   // own bytes inside the text that are no continuation bytes: every one begins a sequence
    uint32_t four;   // ... of those, the leads of 4-byte sequences (two units)
    uint32_t bad;    // own bytes at which a strict decoder stops: leads of ill-formed sequences, unclaimed continuation bytes
    __device__ __forceinline__ uint32_t byte(int k) const { return (w[k >> 2] >> (8 * (k & 3))) & 0xffu; }
    __device__ __forceinline__ uint32_t units() const { return __popc(lead) + __popc(four); }
};

// Every lane of the wave takes part (the neighbours' bytes come through cross-lane moves; a wave's first and last lane load
// theirs).  in: 16-byte aligned, readable up to n rounded up to 16 and 4 bytes more.
__device__ __forceinline__ LaneView lane_view(const uint8_t *__restrict__ in, uint32_t n, uint32_t o) {
    LaneView v;
    uint4 own = make_uint4(0, 0, 0, 0);
    if (o < n) own = *reinterpret_cast<const uint4 *>(in + o);
    uint32_t prev = __shfl_up(own.w, 1), next = __shfl_down(own.x, 1);
    const uint32_t lane = lane_id();
    if (lane == 0) prev = (o != 0 && o < n) ? *reinterpret_cast<const uint32_t *>(in + o - 4) : 0u;
    if (lane == kWave - 1) next = (o + kU8Lane < n) ? *reinterpret_cast<const uint32_t *>(in + o + kU8Lane) : 0u;
    v.w[0] = prev;
    v.w[1] = own.x;
    v.w[2] = own.y;
    v.w[3] = own.z;
    v.w[4] = own.w;
    v.w[5] = next;
    // the window's bytes [0, k_end) lie inside the text; what a load brought from behind its end reads as zero -- no
    // continuation byte, so a sequence that the end of the text truncates fails at its lead
    const int k_end = o >= n ? 4 : (n - o >= 20u ? 24 : (int)(n - o) + 4);
#pragma unroll
    for (int j = 1; j < 6; ++j) {
        const int r = k_end - 4 * j;
        v.w[j] = r >= 4 ? v.w[j] : (r <= 0 ? 0u : v.w[j] & ((1u << (8 * r)) - 1u));
    }
    uint32_t cont = 0, l2 = 0, l3 = 0, l4 = 0, inv = 0, ge90 = 0, gea0 = 0, e0 = 0, ed = 0, f0 = 0, f4 = 0;
#pragma unroll
    for (int k = 0; k < 24; ++k) {
        const uint32_t b = v.byte(k);
        const uint32_t c = (b & 0xc0u) == 0x80u;
        cont |= c << k;
        l2 |= (uint32_t)(b >= 0xc0u) << k;
        l3 |= (uint32_t)(b >= 0xe0u) << k;
        l4 |= (uint32_t)(b >= 0xf0u) << k;
        inv |= (uint32_t)(b == 0xc0u || b == 0xc1u || b >= 0xf5u) << k;
        ge90 |= (uint32_t)(c && b >= 0x90u) << k;
        gea0 |= (uint32_t)(c && b >= 0xa0u) << k;
        e0 |= (uint32_t)(b == 0xe0u) << k;
        ed |= (uint32_t)(b == 0xedu) << k;
        f0 |= (uint32_t)(b == 0xf0u) << k;
        f4 |= (uint32_t)(b == 0xf4u) << k;
    }
    const uint32_t own_bits = k_end >= 20 ? kU8Own : (((1u << k_end) - 1u) & kU8Own);
    // a lead validates its own sequence: the bytes it needs are continuation bytes, the second one in the range its lead allows
    // (E0: A0..BF, no overlong form; ED: 80..9F, no surrogate; F0: 90..BF; F4: 80..8F, nothing above U+10FFFF)
    const uint32_t bad_lead = inv | (l2 & ~(cont >> 1)) | (l3 & ~(cont >> 2)) | (l4 & ~(cont >> 3)) | (e0 & ~(gea0 >> 1)) | (ed & (gea0 >> 1)) |
                              (f0 & ~(ge90 >> 1)) | (f4 & (ge90 >> 1));
    // a continuation byte is claimed when the nearest byte before it that is none is a lead long enough to reach it
    const uint32_t claimed = (l2 << 1) | ((l3 << 2) & (cont << 1)) | ((l4 << 3) & (cont << 2) & (cont << 1));
    v.lead = ~cont & own_bits;
    v.four = l4 & own_bits;
    v.bad = (bad_lead | (cont & ~claimed)) & own_bits;
    return v;
}

// exclusive scan over the workgroup's 256 threads; *total = the sum
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *total) {
    __shared__ uint32_t wave_sum[kU8Threads / kWave];
    const uint32_t inc = wave_inclusive_scan(v);
    const uint32_t wave = threadIdx.x / kWave;
    __syncthreads(); // (the sums of a scan before this one have been read)
    if (lane_id() == kWave - 1) wave_sum[wave] = inc;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < kU8Threads / kWave; ++i) {
        base += i < wave ? wave_sum[i] : 0u;
        sum += wave_sum[i];
    }
    *total = sum;
    return base + inc - v;
}

// res[1]: the smallest offending offset (preset to ~0); block_sums[b] = the units of block b's bytes
__global__ __launch_bounds__(kU8Threads) void k_utf8_count(const uint8_t *__restrict__ in, uint32_t n, uint32_t *__restrict__ block_sums,
                                                           unsigned long long *__restrict__ res) {
    const uint32_t o = (blockIdx.x * kU8Threads + threadIdx.x) * kU8Lane;
    const LaneView v = lane_view(in, n, o);
    // lanes are contiguous: the first lane of a wave that saw something holds the wave's smallest offset
    const unsigned long long offenders = __ballot(v.bad != 0);
    if (offenders && lane_id() == (uint32_t)__ffsll((long long)offenders) - 1)
        atomicMin(res + 1, (unsigned long long)(o - 4 + (uint32_t)__ffs((int)v.bad) - 1));
    uint32_t total;
    (void)block_scan(v.units(), &total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// one workgroup, 256 block sums a round with a running carry (at most 2^19 blocks: 2048 rounds): block_sums become exclusive
// -- the blocks' first unit indices -- and res[0] = their total
__global__ __launch_bounds__(kU8Threads) void k_utf8_scan(uint32_t *__restrict__ block_sums, uint32_t n_blocks, unsigned long long *__restrict__ res) {
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += kU8Threads) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t c = i < n_blocks ? block_sums[i] : 0u;
        uint32_t total;
        const uint32_t ex = carry + block_scan(c, &total);
        if (i < n_blocks) block_sums[i] = ex;
        carry += total;
    }
    if (threadIdx.x == 0) res[0] = carry;
}

// The text is known to be well-formed.  out: n_units units; ckpt: one word per 32 units, or nullptr (an all-ASCII text needs none).
__global__ __launch_bounds__(kU8Threads) void k_utf8_write(const uint8_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ block_base,
                                                           uint16_t *__restrict__ out, uint32_t n_units, uint32_t *__restrict__ ckpt) {
    const uint32_t o = (blockIdx.x * kU8Threads + threadIdx.x) * kU8Lane;
    const LaneView v = lane_view(in, n, o);
    const uint32_t cnt = v.units();
    uint32_t total;
    uint32_t u = block_base[blockIdx.x] + block_scan(cnt, &total);
    if (!cnt || u + cnt > n_units) return; // (the second: never, the counts are those of k_utf8_count)
    if (v.lead == kU8Own && !v.four && cnt == kU8Lane && ((v.w[1] | v.w[2] | v.w[3] | v.w[4]) & 0x80808080u) == 0 && (u & 7u) == 0) {
        // 16 ASCII bytes whose units begin on a 16-byte boundary of the output: two vector stores
        uint32_t p[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t x = v.w[1 + j];
            p[2 * j] = (x & 0xffu) | ((x & 0xff00u) << 8);
            p[2 * j + 1] = ((x >> 16) & 0xffu) | ((x >> 8) & 0xff0000u);
        }
        uint4 *dst = reinterpret_cast<uint4 *>(out + u);
        dst[0] = make_uint4(p[0], p[1], p[2], p[3]);
        dst[1] = make_uint4(p[4], p[5], p[6], p[7]);
        const uint32_t m = (0u - u) & 31u; // the first of the lane's units whose index is a multiple of 32
        if (ckpt && m < kU8Lane) ckpt[(u + m) >> 5] = o + m;
        return;
    }
#pragma unroll
    for (int k = 4; k < 20; ++k) {
        if (!((v.lead >> k) & 1u)) continue;
        const uint32_t pos = o + (uint32_t)(k - 4);
        const uint32_t b0 = v.byte(k), b1 = v.byte(k + 1) & 0x3fu, b2 = v.byte(k + 2) & 0x3fu, b3 = v.byte(k + 3) & 0x3fu;
        if (ckpt && (u & 31u) == 0) ckpt[u >> 5] = pos;
        if (b0 < 0xf0u) {
            const uint32_t cp = b0 < 0x80u ? b0 : (b0 < 0xe0u ? ((b0 & 0x1fu) << 6) | b1 : ((b0 & 0x0fu) << 12) | (b1 << 6) | b2);
            out[u] = (uint16_t)cp;
            u += 1;
        } else {
            const uint32_t cp = (((b0 & 0x07u) << 18) | (b1 << 12) | (b2 << 6) | b3) - 0x10000u;
            out[u] = (uint16_t)(0xd800u + (cp >> 10));
            out[u + 1] = (uint16_t)(0xdc00u + (cp & 0x3ffu));
            if (ckpt && ((u + 1) & 31u) == 0) ckpt[(u + 1) >> 5] = pos | kCkptLow;
            u += 2;
        }
    }
}

__device__ __forceinline__ uint32_t seq_len(uint32_t lead) { return lead < 0x80u ? 1u : (lead < 0xe0u ? 2u : (lead < 0xf0u ? 3u : 4u)); }

// a position of the walk over the sequences: p = the byte offset of a lead, u = the index of its first unit
struct SeqPos {
    uint32_t p, u;
};

__device__ __forceinline__ SeqPos seek(const uint32_t *__restrict__ ckpt, uint32_t unit) {
    const uint32_t c = ckpt[unit >> 5];
    SeqPos s;
    s.p = c & ~kCkptLow;
    s.u = (unit & ~31u) - (c >> 31);
    return s;
}

// moves s (s.u <= unit) to the sequence that holds `unit`; returns that sequence's length in bytes
__device__ __forceinline__ uint32_t advance(const uint8_t *__restrict__ in, uint32_t n, SeqPos &s, uint32_t unit) {
    uint32_t len = 1;
    while (s.p < n) {
        len = seq_len(in[s.p]);
        const uint32_t nu = len == 4 ? 2u : 1u;
        if (unit < s.u + nu) break;
        s.u += nu;
        s.p += len;
    }
    return len;
}

// recs: cnt records of `cols` words in place: start -> the first byte of the code point that holds unit start, end -> one past the
// last byte of the code point that holds unit end - 1 (a match has at least one unit)
__global__ __launch_bounds__(kU8Threads) void k_utf8_map(int32_t *__restrict__ recs, uint64_t cnt, uint32_t cols, const uint8_t *__restrict__ in,
                                                         uint32_t n, uint32_t n_units, const uint32_t *__restrict__ ckpt) {
    const uint64_t i = (uint64_t)blockIdx.x * kU8Threads + threadIdx.x;
    if (i >= cnt) return;
    int32_t *r = recs + i * cols;
    const uint32_t first = (uint32_t)r[0], last = (uint32_t)r[1] - 1u;
    if (first > last || last >= n_units) return; // (never: the scan's records lie inside the text)
    SeqPos s = seek(ckpt, first);
    (void)advance(in, n, s, first);
    r[0] = (int32_t)s.p;
    if ((last >> 5) != (first >> 5)) s = seek(ckpt, last);
    const uint32_t len = advance(in, n, s, last);
    r[1] = (int32_t)(s.p + len);
}

// one lane: *out = the first byte of the code point that holds unit `unit` < n_units -- of a low surrogate, its pair's
__global__ void k_utf8_pos(uint32_t unit, const uint8_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ ckpt, int64_t *__restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    SeqPos s = seek(ckpt, unit);
    (void)advance(in, n, s, unit);
    *out = (int64_t)s.p;
}

} // namespace

namespace acgpu {

int utf8_map_records(const Utf8Text &text, int32_t *d_recs, uint64_t cnt, uint32_t cols, hipStream_t stream) {
    if (!text.d_ckpt || !cnt) return ACGPU_OK;
    hipLaunchKernelGGL(k_utf8_map, dim3((unsigned)((cnt + kU8Threads - 1) / kU8Threads)), dim3(kU8Threads), 0, stream, d_recs, cnt, cols,
                       text.d_bytes, (uint32_t)text.n_bytes, (uint32_t)text.n_units, text.d_ckpt);
    HIP_TRY(hipGetLastError());
    return ACGPU_OK;
}

int utf8_map_position(const Utf8Text &text, uint64_t unit, int64_t *d_out, hipStream_t stream) {
    if (!text.d_ckpt || unit >= text.n_units) return ACGPU_E_INVALID; // (a checkpoint is written for the text's units only)
    hipLaunchKernelGGL(k_utf8_pos, dim3(1), dim3(1), 0, stream, (uint32_t)unit, text.d_bytes, (uint32_t)text.n_bytes, text.d_ckpt, d_out);
    HIP_TRY(hipGetLastError());
    return ACGPU_OK;
}

int stage_utf8_text(DeviceState &d, const uint8_t *bytes, uint64_t n_bytes, hipStream_t stream, Utf8Text *out) {
    *out = Utf8Text{};
    out->n_bytes = n_bytes;
    const uint32_t n = (uint32_t)n_bytes, n_blocks = (n + kU8Block - 1) / kU8Block;
    // aux: [n_units, first_bad | block sums | checkpoints, one per 32 units of a text that has at most n units]
    const size_t sums_off = 64, ckpt_off = sums_off + (((size_t)n_blocks * 4 + 63) & ~(size_t)63);
    int rc;
    if ((rc = d.utf8_in.ensure((size_t)n + 64))) return rc; // (a lane's 16-byte load, and 4 bytes behind it)
    if ((rc = d.utf8_aux.ensure(ckpt_off + ((size_t)n / 32 + 1) * 4))) return rc;
    const uint8_t *d_in = reinterpret_cast<const uint8_t *>(d.utf8_in.p);
    unsigned long long *d_res = reinterpret_cast<unsigned long long *>(d.utf8_aux.p);
    uint32_t *d_sums = reinterpret_cast<uint32_t *>((char *)d.utf8_aux.p + sums_off);
    uint32_t *d_ckpt = reinterpret_cast<uint32_t *>((char *)d.utf8_aux.p + ckpt_off);
    HIP_TRY(hipMemcpyAsync(d.utf8_in.p, bytes, n, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(d_res, 0xff, 16, stream));
    hipLaunchKernelGGL(k_utf8_count, dim3(n_blocks), dim3(kU8Threads), 0, stream, d_in, n, d_sums, d_res);
    hipLaunchKernelGGL(k_utf8_scan, dim3(1), dim3(kU8Threads), 0, stream, d_sums, n_blocks, d_res);
    HIP_TRY(hipGetLastError());
    // the one wait this front end adds: the shard cannot be sized, nor the scan begun, before the text is known to be well-formed
    unsigned long long h_res[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(h_res, d_res, 16, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    out->n_units = h_res[0];
    out->first_bad = (int64_t)h_res[1];
    if (out->first_bad >= 0) return ACGPU_E_ENCODING;
    if (out->n_units > n) return ACGPU_E_HIP; // (never: a sequence has no more units than bytes)
    const bool ascii = out->n_units == n;
    if ((rc = d.stage_hay.ensure(out->n_units * 2 + 16))) return rc;
    hipLaunchKernelGGL(k_utf8_write, dim3(n_blocks), dim3(kU8Threads), 0, stream, d_in, n, (const uint32_t *)d_sums,
                       reinterpret_cast<uint16_t *>(d.stage_hay.p), (uint32_t)out->n_units, ascii ? nullptr : d_ckpt);
    HIP_TRY(hipGetLastError());
    out->shard.d_hay = (const uint16_t *)d.stage_hay.p;
    out->shard.n_units = out->shard.own_end = out->n_units;
    out->shard.text_begin = out->shard.text_end = 1;
    out->d_bytes = d_in;
    out->d_ckpt = ascii ? nullptr : d_ckpt;
    return ACGPU_OK;
}

} // namespace acgpu

extern "C" {

int acgpu_match_utf8(const acgpu_automaton *ca, const uint8_t *bytes, uint64_t n_bytes, int record_kind, void *out, uint64_t cap,
                     uint64_t *n_out, acgpu_utf8_stats *stats) {
    if (!ca || !n_out || (n_bytes && !bytes) || (cap && !out)) return ACGPU_E_INVALID;
    if (record_kind != ACGPU_REC_SET && record_kind != ACGPU_REC_MAP) return ACGPU_E_INVALID;
    if (n_bytes >= (1ull << 31)) return ACGPU_E_INVALID;
    *n_out = 0;
    acgpu_utf8_stats st{};
    st.first_bad = -1;
    st.ascii = 1;
    if (stats) *stats = st;
    if (n_bytes == 0) return ACGPU_OK; // (nothing to decode and nothing to find: no device needed)
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    PoolCall call(a);
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    int rc;
    if ((rc = call.idle())) return rc; // (the NULL stream: see the stream rule)
    const hipStream_t stream = d.call_stream;
    Utf8Text text;
    rc = stage_utf8_text(d, bytes, n_bytes, stream, &text);
    st.n_units = text.n_units;
    st.first_bad = text.first_bad;
    st.ascii = text.n_units == n_bytes;
    if (rc == ACGPU_E_ENCODING) { // (the stream is idle: the pool is as usable as before the call)
        st.n_units = 0;
        st.ascii = 0;
        if (stats) *stats = st;
        return rc;
    }
    if (rc) return call.fail(rc);
    if (stats) *stats = st;
    if ((rc = d.stage_out.ensure(cap * (uint64_t)record_kind + 16))) return call.fail(rc);
    rc = match_shard(a, d, &text.shard, record_kind, d.stage_out.p, cap, n_out, stream, nullptr);
    if (rc != ACGPU_OK) return rc; // (ACGPU_E_OVERFLOW: *n_out is the capacity to call again with)
    if (!*n_out) return ACGPU_OK;
    if ((rc = utf8_map_records(text, reinterpret_cast<int32_t *>(d.stage_out.p), *n_out, (uint32_t)record_kind / 4, stream))) return call.fail(rc);
    HIP_TRY(hipMemcpyAsync(out, d.stage_out.p, *n_out * (uint64_t)record_kind, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return ACGPU_OK;
}

} // extern "C"
