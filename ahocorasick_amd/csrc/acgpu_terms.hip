// acgpu_terms.hip -- acgpu_count_batch_u16 / _utf8 / _utf8_lossy (include/acgpu.h): for every haystack of a batch its distinct
// keywords and how often each occurs -- the document-term matrix of the batch in CSR form -- reduced on the device.
//
// A count-batch call is the fifth consumer of the piece driver (scan_next_piece, acgpu_pieces.hip), and up to the records it is
// the batch summary (acgpu_summary.hip): the haystacks are one text with a separator unit behind each, the Map records of a piece
// stay in the pool's reservoir, and the kernels here run behind every piece that completed.  The run argument of the summary
// holds: a family's records come in listener order, no match crosses a separator, so the haystack index of the records never
// descends, within a piece and from piece to piece.
//
// Per piece of cnt records, three kernels on the call's stream, no host wait between them or behind them:
//   k_terms_block   a workgroup per block of kTermsBlock consecutive records: the keys (h << 32) | id sorted in LDS, the heads of
//                   the runs of equal keys counted, and the block's d distinct {h, id, count} written to ITS region of the staging
//                   buffer, d to n_distinct[block].  Sorting the keys of a block keeps h ascending across blocks, because the
//                   blocks are consecutive slices of a list whose h never descends.
//   k_terms_place   one workgroup: the exclusive scan of n_distinct[] behind the call's running entry count (a u64 in device
//                   memory that lives across the pieces) -> block_base[]; the running count moves on.
//   k_terms_gather  block b copies its entries to entries[block_base[b] + j] where that is below the capacity; counting goes on
//                   where writes are dropped, so the running count at the end of the call is exact.
// (Place and gather are two kernels: the gather of a block needs nothing but block_base[b], and a launch boundary is the cheapest
// order between the scan and its readers.)  The reservoir is only read: the staging buffer holds what the blocks produce.
//
// The entry list the device leaves: h never descends; the entries of one block and one h have ascending, distinct ids; a haystack
// whose run a block or piece boundary cuts (or that has more than kTermsBlock records) has several such sub-rows in a row.  The
// host merges those and only those: terms_finish (acgpu_terms_finish.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <new>

#include "acgpu_device.h"
#include "acgpu_host.h"
#include "acgpu_internal.h"
#include "acgpu_terms_finish.h"

using namespace acgpu;

namespace {

constexpr int kTermsLanes = 256;
constexpr int kTermsPerLane = 8;
constexpr uint32_t kTermsBlock = kTermsLanes * kTermsPerLane; // B: records per workgroup (ahocorasick_amd/_native.py: TERMS_BLOCK)
static_assert(kTermsBlock == 2048 && (kTermsBlock & (kTermsBlock - 1)) == 0, "the bitonic network needs a power of two; _native.py mirrors 2048");
static_assert(sizeof(acgpu_count_batch_stats) == 40, "the layout include/acgpu.h promises");

// exclusive scan of v over the workgroup's kTermsLanes lanes; *total = the sum.  wsum: kTermsLanes / kWave words of LDS, free
// again behind the call (the barrier at its end)
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *wsum, uint32_t *total) {
    const uint32_t incl = wave_inclusive_scan(v), wave = threadIdx.x / kWave;
    if (lane_id() == kWave - 1) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kTermsLanes / kWave; w++) {
        const uint32_t s = wsum[w];
        before += w < wave ? s : 0;
        all += s;
    }
    __syncthreads();
    *total = all;
    return before + incl - v;
}

// Block blockIdx.x of a piece's cnt Map records (buffer relative; base = the text position of the buffer's unit 0 in cat_off's
// coordinates): records [blockIdx.x * B, + m), m = min(B, what is left).  h of a record = h_add + haystack_of(its start).
//  1. keys[p] = (h << 32) | id for p < m, all ones behind (they sort to the end, and no key is all ones: h < 2^31);
//  2. a bitonic network over the B keys in LDS: 66 steps of B / 2 compare-exchanges, 4 per lane;
//  3. lane t owns the sorted positions [8 t, 8 t + 8): a head is a position below m whose key differs from the one before it; the
//     exclusive scan of the lanes' head counts gives every head its slot; the head stores its key and its position there, the
//     number of heads d is the block's distinct keys, first[d] = m;
//  4. entry s < d = {key >> 32, key, first[s + 1] - first[s]} into stage[blockIdx.x * B + s], d into n_distinct[blockIdx.x].
// Every global index is bounded by m <= B: reads of recs below 3 (block * B + m) <= 3 cnt, writes of stage inside the block's own region.
__global__ __launch_bounds__(kTermsLanes) void k_terms_block(const int32_t *__restrict__ recs, uint64_t cnt, const uint32_t *__restrict__ cat_off,
                                                             uint32_t n_hay, int64_t base, uint32_t h_add, uint32_t *__restrict__ stage,
                                                             uint32_t *__restrict__ n_distinct) {
    __shared__ uint64_t keys[kTermsBlock];
    __shared__ uint32_t first[kTermsBlock + 1];
    __shared__ uint32_t wsum[kTermsLanes / kWave];
    const uint32_t tid = threadIdx.x;
    const uint64_t rec0 = (uint64_t)blockIdx.x * kTermsBlock;
    const uint32_t m = cnt - rec0 < kTermsBlock ? (uint32_t)(cnt - rec0) : kTermsBlock;
#pragma unroll
    for (int r = 0; r < kTermsPerLane; r++) {
        const uint32_t p = tid + r * kTermsLanes;
        uint64_t key = ~0ull;
        if (p < m) {
            const int32_t *rec = recs + 3 * (rec0 + p);
            const uint32_t h = h_add + haystack_of(cat_off, n_hay, (uint32_t)((int64_t)rec[0] + base));
            key = (uint64_t)h << 32 | (uint32_t)rec[2];
        }
        keys[p] = key;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= kTermsBlock; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int r = 0; r < kTermsPerLane / 2; r++) {
                const uint32_t t = tid + r * kTermsLanes;               // the t-th pair of this step
                const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const uint64_t a = keys[lo], b = keys[hi];
                if ((a > b) == ((lo & k) == 0)) { // (k == B: every pair ascending)
                    keys[lo] = b;
                    keys[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    const uint32_t p0 = tid * kTermsPerLane;
    uint64_t mine[kTermsPerLane];
    uint64_t prev = tid ? keys[p0 - 1] : ~0ull;
    uint32_t heads = 0, n_heads = 0;
#pragma unroll
    for (int r = 0; r < kTermsPerLane; r++) {
        mine[r] = keys[p0 + r];
        const bool head = p0 + r < m && (p0 + r == 0 || mine[r] != prev);
        prev = mine[r];
        heads |= (uint32_t)head << r;
        n_heads += head;
    }
    uint32_t d;
    uint32_t slot = block_exclusive_scan(n_heads, wsum, &d); // (its barriers: every lane has read its keys before a slot is written)
#pragma unroll
    for (int r = 0; r < kTermsPerLane; r++) {
        if (heads >> r & 1) {
            keys[slot] = mine[r]; // (slot <= p0 + r)
            first[slot] = p0 + r;
            slot++;
        }
    }
    if (tid == 0) {
        first[d] = m;
        n_distinct[blockIdx.x] = d;
    }
    __syncthreads();
    uint32_t *out = stage + 3 * rec0;
    for (uint32_t s = tid; s < d; s += kTermsLanes) {
        const uint64_t key = keys[s];
        out[3 * s] = (uint32_t)(key >> 32);
        out[3 * s + 1] = (uint32_t)key;
        out[3 * s + 2] = first[s + 1] - first[s];
    }
}

// block_base[b] = *running + the distinct keys of the blocks in front of b; *running += those of all n_blocks.  One workgroup.
__global__ __launch_bounds__(kTermsLanes) void k_terms_place(const uint32_t *__restrict__ n_distinct, uint32_t n_blocks,
                                                             unsigned long long *__restrict__ running, unsigned long long *__restrict__ block_base) {
    __shared__ uint32_t wsum[kTermsLanes / kWave];
    unsigned long long run = *running;
    __syncthreads(); // (lane 0 writes *running at the end: behind every lane's read, also where the loop below runs once)
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += kTermsLanes) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < n_blocks ? n_distinct[b] : 0;
        uint32_t total;
        const uint32_t before = block_exclusive_scan(v, wsum, &total);
        if (b < n_blocks) block_base[b] = run + before;
        run += total;
    }
    if (threadIdx.x == 0) *running = run;
}

// Block b's n_distinct[b] entries (3 words each, at stage + 3 b B) to entries + 3 block_base[b], word by word; a word is written
// only where its entry index is below cap.
__global__ __launch_bounds__(kTermsLanes) void k_terms_gather(const uint32_t *__restrict__ stage, const uint32_t *__restrict__ n_distinct,
                                                              const unsigned long long *__restrict__ block_base, uint32_t *__restrict__ entries,
                                                              uint64_t cap) {
    const uint32_t words = 3 * n_distinct[blockIdx.x];
    const uint64_t to = 3 * (uint64_t)block_base[blockIdx.x], limit = 3 * cap;
    const uint32_t *from = stage + 3 * (uint64_t)blockIdx.x * kTermsBlock;
    for (uint32_t w = threadIdx.x; w < words; w += kTermsLanes)
        if (to + w < limit) entries[to + w] = from[w];
}

// One count-batch call on a pool: the device's entry list as it grows over the pieces of the texts the call drives.
struct TermsCall {
    DeviceState &d;
    hipStream_t stream;
    uint64_t cap;          // the caller's capacity, in entries
    uint64_t room = 0;     // entries the device list has room for: min(cap, every record seen so far)
    uint64_t records = 0;  // records of the pieces reduced so far (an upper bound of the entries)
    acgpu_count_batch_stats st{};

    unsigned long long *running() const { return reinterpret_cast<unsigned long long *>(d.terms_count.p); }

    int begin(uint64_t units) {
        int rc = d.terms_count.ensure(16);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(d.terms_count.p, 0, 16, stream));
        return grow(std::max<uint64_t>(4096, units / 4));
    }

    // The entry list with room for min(cap, want) entries.  A list that has to move keeps what it holds: the one place where the
    // host waits between pieces, and with the list growing by half at least it does so a logarithmic number of times.
    int grow(uint64_t want) {
        want = std::min(cap, want);
        const uint64_t have = d.terms_entries.bytes / 12;
        int rc = ACGPU_OK;
        if (want > have) {
            want = std::max(want, std::min(cap, have + have / 2));
            const size_t keep = (size_t)std::min(room, records) * 12; // (what the list holds: at most every record so far)
            DevBuf &list = d.terms_entries, old = list; // (a PoolBuf is a DevBuf that releases itself: `old` is the plain buffer)
            list = DevBuf{};
            rc = list.ensure((size_t)want * 12);
            if (rc == ACGPU_OK && keep && hipMemcpyAsync(list.p, old.p, keep, hipMemcpyDeviceToDevice, stream) != hipSuccess) rc = ACGPU_E_HIP;
            if (hipStreamSynchronize(stream) != hipSuccess) rc = rc ? rc : ACGPU_E_HIP; // (nothing reads or writes the old list when it is freed)
            old.release();
        }
        room = std::min<uint64_t>(cap, d.terms_entries.bytes / 12);
        return rc;
    }

    // the three kernels behind a piece of cnt records in the reservoir
    int reduce(uint64_t cnt, const uint32_t *cat_off, uint32_t n_hay, int64_t base, uint32_t h_add) {
        const uint64_t n_blocks = (cnt + kTermsBlock - 1) / kTermsBlock;
        int rc = grow(records + cnt);
        if (rc) return rc;
        if ((rc = d.terms_stage.ensure((size_t)n_blocks * kTermsBlock * 12))) return rc;
        if ((rc = d.terms_aux.ensure((size_t)n_blocks * 12))) return rc;
        unsigned long long *block_base = reinterpret_cast<unsigned long long *>(d.terms_aux.p);
        uint32_t *n_distinct = reinterpret_cast<uint32_t *>(block_base + n_blocks);
        uint32_t *stage = reinterpret_cast<uint32_t *>(d.terms_stage.p);
        hipLaunchKernelGGL(k_terms_block, dim3((unsigned)n_blocks), dim3(kTermsLanes), 0, stream, reinterpret_cast<const int32_t *>(d.count_res.p),
                           cnt, cat_off, n_hay, base, h_add, stage, n_distinct);
        hipLaunchKernelGGL(k_terms_place, dim3(1), dim3(kTermsLanes), 0, stream, n_distinct, (uint32_t)n_blocks, running(), block_base);
        hipLaunchKernelGGL(k_terms_gather, dim3((unsigned)n_blocks), dim3(kTermsLanes), 0, stream, stage, n_distinct, block_base,
                           reinterpret_cast<uint32_t *>(d.terms_entries.p), room);
        HIP_TRY(hipGetLastError());
        records += cnt;
        st.n_records += cnt;
        return ACGPU_OK;
    }

    // One text through the pieces, as summary_pieces drives it.  The haystacks that begin at cat_off[0 .. n_hay) of a text whose
    // unit 0 stands at `origin` in cat_off's coordinates are haystacks h_add .. of the batch; one haystack alone: n_hay = 1,
    // h_add = its index, and cat_off is not read.
    int pieces(acgpu_automaton *a, const PieceScan &scan, bool whole, const uint32_t *cat_off, uint32_t n_hay, uint64_t origin, uint32_t h_add) {
        PieceDriver p(0, scan.shard ? scan.shard->own_end : scan.n, 0, whole, ACGPU_REC_MAP, &d.count_res);
        int rc = ACGPU_OK;
        while (rc == ACGPU_OK && p.pos < p.end) {
            uint64_t cnt = 0, base = 0;
            if ((rc = scan_next_piece(p, scan, &cnt, &base))) break;
            if (cnt) rc = reduce(cnt, cat_off, n_hay, (int64_t)(base + origin), h_add);
        }
        st.pieces += (uint32_t)p.pieces;
        st.rescans += (uint32_t)p.rescans;
        return rc;
    }

    // Behind the last piece: the running count, then -- where it fits the caller's capacity -- the entries, finished into the
    // caller's arrays.  ACGPU_E_OVERFLOW: *n_out = the entries, nothing else is written.
    int finish(uint32_t n_haystacks, uint64_t *row_ptr, uint32_t *ids, uint32_t *counts, uint64_t *n_out) {
        unsigned long long n_entries = 0;
        HIP_TRY(hipMemcpyAsync(&n_entries, running(), 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        st.n_entries = n_entries;
        if (n_entries > cap) {
            *n_out = n_entries;
            return ACGPU_E_OVERFLOW;
        }
        if (n_entries > records || n_entries > room) return ACGPU_E_HIP; // (never)
        std::unique_ptr<uint32_t[]> entries(new (std::nothrow) uint32_t[(size_t)n_entries * 3 + 1]); // (not zeroed: the copy fills it)
        if (!entries) return ACGPU_E_NOMEM;
        if (n_entries) {
            HIP_TRY(hipMemcpyAsync(entries.get(), d.terms_entries.p, (size_t)n_entries * 12, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
        if (terms_finish(entries.get(), n_entries, n_haystacks, row_ptr, ids, counts, &st.n_terms, &st.rows_cut)) return ACGPU_E_HIP; // (never)
        *n_out = st.n_terms;
        return ACGPU_OK;
    }
};

// what the three entries check before anything else
bool bad_arguments(const void *a, const void *offsets, const uint64_t *row_ptr, const uint32_t *ids, const uint32_t *counts, uint64_t cap,
                   const uint64_t *n_out) {
    return !a || !offsets || !row_ptr || !n_out || (cap && (!ids || !counts));
}

// a batch with nothing to scan: an empty matrix, no device
int empty_matrix(uint32_t n_haystacks, uint64_t *row_ptr, uint64_t *n_out, acgpu_count_batch_stats *st) {
    for (uint32_t i = 0; i <= n_haystacks; i++) row_ptr[i] = 0;
    *n_out = 0;
    if (st) *st = acgpu_count_batch_stats{};
    return ACGPU_OK;
}

// The body of acgpu_count_batch_utf8 and acgpu_count_batch_utf8_lossy.  P (acgpu_host.h): how the batch is staged, and the entry's stats.
template <class P>
int count_batch_utf8(const acgpu_automaton *ca, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks, uint64_t *row_ptr,
                     uint32_t *ids, uint32_t *counts, uint64_t cap, uint64_t *n_out, acgpu_count_batch_stats *st, typename P::Stats *stats) {
    if (bad_arguments(ca, offsets, row_ptr, ids, counts, cap, n_out)) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    const HostTables &t = a->t;
    BatchPlan plan; // (in bytes: bytes >= units, so bytes + haystacks < 2^31 bounds the text the scan sees)
    int rc = check_batch(t, reinterpret_cast<const uint16_t *>(bytes), offsets, n_haystacks, &plan);
    if (rc) return rc;
    if (plan.total == 0) {
        if (stats) *stats = P::stats();
        return empty_matrix(n_haystacks, row_ptr, n_out, st);
    }
    PoolCall call(a); // (no device: fails here and the arrays are untouched)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    if ((rc = call.idle())) return rc; // (the NULL stream: see the stream rule)
    const hipStream_t stream = d.call_stream;
    Utf8Batch b;
    rc = stage_utf8_batch(d, t, bytes, offsets, n_haystacks, stream, &b, plan.per_haystack, P::errors);
    if (rc == ACGPU_E_ENCODING) { // (the stream is idle: the pool is as usable as before the call)
        if (stats) *stats = P::stats(&b, rc);
        *n_out = 0;
        return rc;
    }
    if (rc) return call.fail(rc);
    TermsCall terms{d, stream, cap};
    if ((rc = terms.begin(plan.cat))) return call.fail(rc);
    const bool whole = shard_rule(t, ACGPU_REC_MAP, false).sequential; // (a device shard: as acgpu_summary_batch_utf8 drives its pieces)
    if (plan.per_haystack) { // every haystack staged and driven as a text of its own
        for (uint32_t i = 0; i < n_haystacks && rc == ACGPU_OK; i++) {
            const uint64_t len = offsets[i + 1] - offsets[i];
            if (!len) continue;
            Utf8Text text;
            if ((rc = stage_utf8_text(d, bytes + offsets[i], len, stream, &text, P::errors))) break;
            rc = terms.pieces(a, PieceScan{a, d, nullptr, 0, &text.shard, stream}, whole, nullptr, 1, 0, i);
        }
        if (rc == ACGPU_E_ENCODING) rc = ACGPU_E_HIP; // (never: the batch has been validated)
    } else {
        SeparatorScan sep(d, t);
        rc = terms.pieces(a, PieceScan{a, d, nullptr, 0, &b.text.shard, stream}, whole, b.d_cat_off, n_haystacks, 0, 0);
    }
    if (rc == ACGPU_OK) rc = terms.finish(n_haystacks, row_ptr, ids, counts, n_out);
    if (rc != ACGPU_OK && rc != ACGPU_E_OVERFLOW) return call.fail(rc);
    if (st) *st = terms.st;
    if (stats) *stats = P::stats(&b);
    return rc;
}

} // namespace

extern "C" {

int acgpu_count_batch_u16(const acgpu_automaton *ca, const uint16_t *units, const uint64_t *offsets, uint32_t n_haystacks, uint64_t *row_ptr,
                          uint32_t *keyword_ids, uint32_t *counts, uint64_t cap, uint64_t *n_out, acgpu_count_batch_stats *st) {
    if (bad_arguments(ca, offsets, row_ptr, keyword_ids, counts, cap, n_out)) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    const HostTables &t = a->t;
    BatchPlan plan;
    int rc = check_batch(t, units, offsets, n_haystacks, &plan);
    if (rc) return rc;
    if (plan.total == 0) return empty_matrix(n_haystacks, row_ptr, n_out, st);
    PoolCall call(a); // (no device: fails here, as acgpu_match_batch_u16 does, and the arrays are untouched)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    if ((rc = call.idle())) return rc; // (the NULL stream: see the stream rule)
    const hipStream_t stream = d.call_stream;
    TermsCall terms{d, stream, cap};
    if ((rc = terms.begin(plan.cat))) return call.fail(rc);
    const bool whole = host_one_piece(t, ACGPU_REC_MAP);
    if (plan.per_haystack) { // every haystack goes through the pieces as a text of its own
        for (uint32_t i = 0; i < n_haystacks && rc == ACGPU_OK; i++) {
            const uint64_t len = offsets[i + 1] - offsets[i];
            if (len) rc = terms.pieces(a, PieceScan{a, d, units + offsets[i], len, nullptr, stream}, whole, nullptr, 1, 0, i);
        }
    } else {
        BatchText text(d, t);
        if ((rc = text.stage(units, offsets, n_haystacks, stream))) return call.fail(rc);
        rc = terms.pieces(a, PieceScan{a, d, text.h_cat, text.cat, nullptr, stream}, whole, text.d_off(), n_haystacks, 0, 0);
    }
    if (rc == ACGPU_OK) rc = terms.finish(n_haystacks, row_ptr, keyword_ids, counts, n_out);
    if (rc != ACGPU_OK && rc != ACGPU_E_OVERFLOW) return call.fail(rc);
    if (st) *st = terms.st;
    return rc;
}

int acgpu_count_batch_utf8(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks, uint64_t *row_ptr,
                           uint32_t *keyword_ids, uint32_t *counts, uint64_t cap, uint64_t *n_out, acgpu_count_batch_stats *st,
                           acgpu_utf8_batch_stats *stats) {
    return count_batch_utf8<Utf8StrictBatch>(a, bytes, offsets, n_haystacks, row_ptr, keyword_ids, counts, cap, n_out, st, stats);
}

int acgpu_count_batch_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks, uint64_t *row_ptr,
                                 uint32_t *keyword_ids, uint32_t *counts, uint64_t cap, uint64_t *n_out, acgpu_count_batch_stats *st,
                                 acgpu_utf8_lossy_stats *stats) {
    return count_batch_utf8<Utf8LossyBatch>(a, bytes, offsets, n_haystacks, row_ptr, keyword_ids, counts, cap, n_out, st, stats);
}

int acgpu_debug_count_batch_finish(const uint32_t *entries, uint64_t n_entries, uint32_t n_haystacks, uint64_t *row_ptr, uint32_t *ids,
                                   uint32_t *counts, uint64_t *n_terms, uint32_t *rows_cut) {
    if ((n_entries && (!entries || !ids || !counts)) || !row_ptr || !n_terms || !rows_cut) return ACGPU_E_INVALID;
    return terms_finish(entries, n_entries, n_haystacks, row_ptr, ids, counts, n_terms, rows_cut) ? ACGPU_E_HIP : ACGPU_OK;
}

} // extern "C"
