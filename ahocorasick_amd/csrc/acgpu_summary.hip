// acgpu_summary.hip -- acgpu_summary_batch_u16 (include/acgpu.h): for every haystack of a batch how many records it has and the
// first of them, reduced on the device.
//
// A summary call is the fourth consumer of the piece driver (scan_next_piece, acgpu_pieces.hip): the haystacks are concatenated
// with a separator unit behind each (BatchText, as acgpu_replace_batch_u16 does), that text goes through the pieces, the Map
// records of a piece stay in the pool's reservoir, and behind every piece that completed ONE kernel, k_batch_summary, reduces them
// into the pool's summaries -- 24 bytes per haystack, the only thing that leaves the device, once, at the end of the call.
//
// Why a run-wise reduction is enough: no match, word or walk crosses a separator, and a family's records come in listener order,
// which within a text is a position order (ALL and SHORTEST: by last unit, the others: by first unit) -- so the records of one
// haystack are CONTIGUOUS, within a piece and from piece to piece, and a piece's record list is a sequence of runs, one per
// haystack that has records in it, haystacks ascending.  A piece therefore holds at most one run per haystack; a run that a piece
// boundary cuts continues as the first run of the next piece.
//
// acgpu_summary_batch_utf8 is the same call for UTF-8 haystacks: the text comes from stage_utf8_batch (acgpu_utf8.hip) as a device
// shard, the pieces and k_batch_summary run unchanged, and k_summary_utf8_bytes maps the first records to bytes at the end.
// acgpu_summary_batch_utf8_lossy is that body with the lossy policy (summary_batch_utf8<P>): ill-formed bytes are staged as U+FFFD.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "acgpu_device.h"
#include "acgpu_host.h"
#include "acgpu_internal.h"

using namespace acgpu;

namespace {

constexpr int kSummaryBlock = 256;

static_assert(sizeof(acgpu_batch_summary) == 24, "the layout include/acgpu.h promises");

// every entry {0, -1, -1, -1, 0}
__global__ __launch_bounds__(kSummaryBlock) void k_summary_fill(acgpu_batch_summary *__restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * kSummaryBlock + threadIdx.x;
    if (i >= n) return;
    acgpu_batch_summary s;
    s.n_matches = 0;
    s.start = s.end = s.keyword_id = -1;
    s.reserved = 0;
    out[i] = s;
}

// A piece's cnt Map records (buffer relative; `base` = the text position of the buffer's unit 0) into the summaries: a lane per
// record.  The lane's haystack h comes from its record's start; its neighbours' come from the lanes beside it, and only a wave's
// first and last lane search for a record of another wave (i - 1, i + 1).
//  * count: the HEAD of a run (i == 0 or h(i - 1) != h(i)) adds -i to n_matches[h], its TAIL (i == cnt - 1 or h(i + 1) != h(i))
//    adds i + 1 (modulo 2^64; a run of one record adds 1 at once).  A run cut by a piece boundary has its tail in one piece and
//    its head in the next, and the sums still add up to the run's length.
//  * first: a head writes its record where the entry's start is still -1.  Only the head at i == 0 can find an entry that an
//    earlier piece wrote -- an earlier kernel on the same stream; within the kernel one lane at most touches the first-record
//    words of an entry (one run per haystack), so plain stores do.
__global__ __launch_bounds__(kSummaryBlock) void k_batch_summary(const int32_t *__restrict__ recs, uint64_t cnt, const uint32_t *__restrict__ cat_off,
                                                                 uint32_t n_hay, int64_t base, acgpu_batch_summary *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kSummaryBlock + threadIdx.x;
    const bool live = i < cnt;
    int32_t s = 0, e = 0, id = 0;
    uint32_t h = 0xffffffffu;
    if (live) {
        s = recs[3 * i];
        e = recs[3 * i + 1];
        id = recs[3 * i + 2];
        h = haystack_of(cat_off, n_hay, (uint32_t)((int64_t)s + base));
    }
    const uint32_t lane = lane_id();
    uint32_t hp = __shfl_up(h, 1), hn = __shfl_down(h, 1); // (every lane of the wave takes part; a live lane's neighbour inside [0, cnt) is live)
    if (!live) return;
    bool head = i == 0, tail = i == cnt - 1;
    if (!head) {
        if (lane == 0) hp = haystack_of(cat_off, n_hay, (uint32_t)((int64_t)recs[3 * (i - 1)] + base));
        head = hp != h;
    }
    if (!tail) {
        if (lane == kWave - 1) hn = haystack_of(cat_off, n_hay, (uint32_t)((int64_t)recs[3 * (i + 1)] + base));
        tail = hn != h;
    }
    if (!head && !tail) return;
    acgpu_batch_summary *o = out + h;
    unsigned long long *n_matches = reinterpret_cast<unsigned long long *>(&o->n_matches);
    if (head && tail) atomicAdd(n_matches, 1ull);
    else if (head) atomicAdd(n_matches, 0ull - (unsigned long long)i);
    else atomicAdd(n_matches, (unsigned long long)i + 1);
    if (head && o->start == -1) {
        const int64_t rel = base - (int64_t)cat_off[h];
        o->start = (int32_t)((int64_t)s + rel);
        o->end = (int32_t)((int64_t)e + rel);
        o->keyword_id = id;
    }
}

// Where the records of one driven text go: the entries of the haystacks that begin at cat_off[0 .. n_hay) of a text whose unit 0
// stands at `origin` in cat_off's coordinates.  The batch as one text: all the offsets, origin 0.  One haystack alone (the calls
// per haystack): its own offset, n_hay = 1 and origin = that offset, so that every record is its haystack's and positions stay
// what they are.
struct SummaryTarget {
    const uint32_t *cat_off;
    uint32_t n_hay;
    uint64_t origin;
    acgpu_batch_summary *out;
};

// One text through the pieces; behind every piece that scan_next_piece completed (a piece scanned again for want of room comes
// back once) the summary kernel on its records.  The host waits for nothing here: the next scan follows on the same stream.
int summary_pieces(acgpu_automaton *a, DeviceState &d, const PieceScan &scan, bool whole, const SummaryTarget &tg, acgpu_summary_stats *st) {
    // the pool's reservoir of Map records (one call at a time holds the pool); a device shard is driven over the units it owns
    PieceDriver p(0, scan.shard ? scan.shard->own_end : scan.n, 0, whole, ACGPU_REC_MAP, &d.count_res);
    int rc = ACGPU_OK;
    while (rc == ACGPU_OK && p.pos < p.end) {
        uint64_t cnt = 0, base = 0;
        if ((rc = scan_next_piece(p, scan, &cnt, &base))) break;
        if (!cnt) continue;
        hipLaunchKernelGGL(k_batch_summary, dim3((unsigned)((cnt + kSummaryBlock - 1) / kSummaryBlock)), dim3(kSummaryBlock), 0, scan.stream,
                           reinterpret_cast<const int32_t *>(d.count_res.p), cnt, tg.cat_off, tg.n_hay, (int64_t)(base + tg.origin), tg.out);
        HIP_TRY(hipGetLastError());
        st->n_records += cnt;
    }
    st->pieces += (uint32_t)p.pieces;
    st->rescans += (uint32_t)p.rescans;
    return rc;
}

// The body of acgpu_summary_batch_utf8 and acgpu_summary_batch_utf8_lossy.  P (acgpu_host.h): how the batch is staged, and the entry's stats.
template <class P>
int summary_batch_utf8(const acgpu_automaton *ca, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks, acgpu_batch_summary *out,
                       acgpu_summary_stats *st, typename P::Stats *stats) {
    if (!ca || !offsets || (n_haystacks && !out)) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    const HostTables &t = a->t;
    BatchPlan plan; // (in bytes: bytes >= units, so bytes + haystacks < 2^31 bounds the text the scan sees)
    int rc = check_batch(t, reinterpret_cast<const uint16_t *>(bytes), offsets, n_haystacks, &plan);
    if (rc) return rc;
    if (plan.total == 0) { // (nothing to decode and nothing to find: no device needed)
        for (uint32_t i = 0; i < n_haystacks; i++) out[i] = acgpu_batch_summary{0, -1, -1, -1, 0};
        if (st) *st = acgpu_summary_stats{};
        if (stats) *stats = P::stats();
        return ACGPU_OK;
    }
    PoolCall call(a); // (no device: fails here and out is untouched)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    if ((rc = call.idle())) return rc; // (the NULL stream: see the stream rule)
    const hipStream_t stream = d.call_stream;
    Utf8Batch b;
    rc = stage_utf8_batch(d, t, bytes, offsets, n_haystacks, stream, &b, plan.per_haystack, P::errors);
    if (rc == ACGPU_E_ENCODING) { // (the stream is idle: the pool is as usable as before the call)
        if (stats) *stats = P::stats(&b, rc);
        return rc;
    }
    if (rc) return call.fail(rc);
    const size_t sum_bytes = (size_t)n_haystacks * sizeof(acgpu_batch_summary);
    if ((rc = d.summary.ensure(sum_bytes))) return call.fail(rc);
    acgpu_batch_summary *d_sum = reinterpret_cast<acgpu_batch_summary *>(d.summary.p);
    hipLaunchKernelGGL(k_summary_fill, dim3((n_haystacks + kSummaryBlock - 1) / kSummaryBlock), dim3(kSummaryBlock), 0, stream, d_sum, n_haystacks);
    if (hipGetLastError() != hipSuccess) return call.fail(ACGPU_E_HIP);
    acgpu_summary_stats sum{};
    const bool whole = shard_rule(t, ACGPU_REC_MAP, false).sequential; // (a device shard: as acgpu_replace_utf8 drives its pieces)
    if (plan.per_haystack) { // every haystack staged and driven as a text of its own, into its own entry, mapped before the next is staged
        // the target of one haystack alone: one offset that is the text's origin as well -- its value does not matter, word 0 of
        // the batch's offsets table (stage_utf8_batch has made room for it) holds it
        uint32_t *d_zero = reinterpret_cast<uint32_t *>(d.batch_off.p);
        if (hipMemsetAsync(d_zero, 0, 4, stream) != hipSuccess) return call.fail(ACGPU_E_HIP);
        for (uint32_t i = 0; i < n_haystacks && rc == ACGPU_OK; i++) {
            const uint64_t len = offsets[i + 1] - offsets[i];
            if (!len) continue;
            Utf8Text text;
            if ((rc = stage_utf8_text(d, bytes + offsets[i], len, stream, &text, P::errors))) break;
            if ((rc = summary_pieces(a, d, PieceScan{a, d, nullptr, 0, &text.shard, stream}, whole, SummaryTarget{d_zero, 1, 0, d_sum + i}, &sum))) break;
            rc = utf8_summary_bytes(nullptr, text, d_sum + i, 1, stream);
        }
        if (rc == ACGPU_E_ENCODING) rc = ACGPU_E_HIP; // (never: the batch has been validated)
    } else {
        SeparatorScan sep(d, t);
        rc = summary_pieces(a, d, PieceScan{a, d, nullptr, 0, &b.text.shard, stream}, whole, SummaryTarget{b.d_cat_off, n_haystacks, 0, d_sum}, &sum);
        if (rc == ACGPU_OK) rc = utf8_summary_bytes(&b, b.text, d_sum, n_haystacks, stream);
    }
    if (rc) return call.fail(rc);
    if (hipMemcpyAsync(out, d_sum, sum_bytes, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
        return call.fail(ACGPU_E_HIP);
    for (uint32_t i = 0; i < n_haystacks; i++) sum.n_matched += out[i].n_matches != 0;
    if (st) *st = sum;
    if (stats) *stats = P::stats(&b);
    return ACGPU_OK;
}

} // namespace

extern "C" {

int acgpu_summary_batch_u16(const acgpu_automaton *ca, const uint16_t *units, const uint64_t *offsets, uint32_t n_haystacks,
                            acgpu_batch_summary *out, acgpu_summary_stats *st) {
    if (!ca || !offsets || (n_haystacks && !out)) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    const HostTables &t = a->t;
    BatchPlan plan;
    int rc = check_batch(t, units, offsets, n_haystacks, &plan);
    if (rc) return rc;
    if (n_haystacks == 0) {
        if (st) *st = acgpu_summary_stats{};
        return ACGPU_OK;
    }
    PoolCall call(a); // (no device: fails here, as acgpu_match_batch_u16 does, and out is untouched)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    if ((rc = call.idle())) return rc; // (the NULL stream: see the stream rule)
    const hipStream_t stream = d.call_stream;
    const size_t off_bytes = ((size_t)n_haystacks + 1) * 4, sum_bytes = (size_t)n_haystacks * sizeof(acgpu_batch_summary);
    if ((rc = d.summary.ensure(sum_bytes))) return rc;
    acgpu_batch_summary *d_sum = reinterpret_cast<acgpu_batch_summary *>(d.summary.p);
    hipLaunchKernelGGL(k_summary_fill, dim3((n_haystacks + kSummaryBlock - 1) / kSummaryBlock), dim3(kSummaryBlock), 0, stream, d_sum, n_haystacks);
    HIP_TRY(hipGetLastError());
    acgpu_summary_stats sum{};
    const bool whole = host_one_piece(t, ACGPU_REC_MAP);
    if (plan.per_haystack) { // every haystack goes through the pieces as a text of its own, into its own entry
        std::vector<uint32_t> h_off;
        try {
            h_off.resize((size_t)n_haystacks + 1);
        } catch (...) {
            return ACGPU_E_NOMEM;
        }
        for (uint32_t i = 0; i <= n_haystacks; i++) h_off[i] = (uint32_t)(offsets[i] - offsets[0] + i); // (the concatenation's offsets)
        if ((rc = d.batch_off.ensure(off_bytes + 16))) return rc;
        const uint32_t *d_off = reinterpret_cast<const uint32_t *>(d.batch_off.p);
        HIP_TRY(hipMemcpy(d.batch_off.p, h_off.data(), off_bytes, hipMemcpyHostToDevice));
        for (uint32_t i = 0; i < n_haystacks && rc == ACGPU_OK; i++) {
            const uint64_t len = offsets[i + 1] - offsets[i];
            if (!len) continue;
            rc = summary_pieces(a, d, PieceScan{a, d, units + offsets[i], len, nullptr, stream}, whole,
                                SummaryTarget{d_off + i, 1, h_off[i], d_sum + i}, &sum);
        }
    } else {
        BatchText text(d, t);
        if ((rc = text.stage(units, offsets, n_haystacks, stream))) return rc;
        rc = summary_pieces(a, d, PieceScan{a, d, text.h_cat, text.cat, nullptr, stream}, whole, SummaryTarget{text.d_off(), n_haystacks, 0, d_sum},
                            &sum);
    }
    if (rc) return call.fail(rc);
    HIP_TRY(hipMemcpyAsync(out, d_sum, sum_bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (uint32_t i = 0; i < n_haystacks; i++) sum.n_matched += out[i].n_matches != 0;
    if (st) *st = sum;
    return ACGPU_OK;
}

int acgpu_summary_batch_utf8(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                             acgpu_batch_summary *out, acgpu_summary_stats *st, acgpu_utf8_batch_stats *stats) {
    return summary_batch_utf8<Utf8StrictBatch>(a, bytes, offsets, n_haystacks, out, st, stats);
}

int acgpu_summary_batch_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                                   acgpu_batch_summary *out, acgpu_summary_stats *st, acgpu_utf8_lossy_stats *stats) {
    return summary_batch_utf8<Utf8LossyBatch>(a, bytes, offsets, n_haystacks, out, st, stats);
}

} // extern "C"
