// acgpu_count.hip -- acgpu_count_u16 / acgpu_count_device (include/acgpu.h): how often every keyword occurs, without records.
//
// A counting call drives the text in pieces through the cursor's driver (scan_next_piece, acgpu_pieces.hip), every piece as
// ordinary shard calls whose results collect() hands to count_collected below instead of to a caller:
//  * direct form -- ALL mode where the shard takes the states form (choose_states_form): k_ac_states, then k_states_hist adds
//    the owned positions' states to the pool's visit words (acgpu_states.hip).  No record exists; after the last piece
//    k_states_spread turns the visits into counts.
//  * records form -- any family, any scan form: Map records into the pool's reservoir, whose keyword_id column k_count_ids adds
//    to the counts.  Records that do not fit: nothing of that shard is counted, and it is scanned again in a larger reservoir
//    or as a smaller piece.
// Nothing but a shard's record count reaches the host.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "acgpu_host.h"
#include "acgpu_internal.h"

using namespace acgpu;

namespace acgpu {

int count_collected(DeviceState &d, const CallRecord &r, uint64_t n) {
    CountCall &c = *d.count;
    const uint64_t own = r.shard.own_end - r.shard.own_begin;
    if (r.form == CallForm::StatesCount) {
        c.st.units_direct += own;
        c.st.n_records += n;
        return ACGPU_OK;
    }
    if (n > r.cap) return ACGPU_E_OVERFLOW;
    HIP_TRY(launch_count_ids(r.d_out, n, c.d_counts, c.n_counts, !(tunables().count_form & 4), r.stream));
    c.st.units_records += own;
    c.st.n_records += n;
    c.through_reservoir += n;
    return ACGPU_OK;
}

} // namespace acgpu

namespace {

struct CountGuard { // DeviceState::count for the duration of a call (the caller holds d.mu)
    DeviceState &d;
    CountGuard(DeviceState &d_, CountCall *c) : d(d_) { d.count = c; }
    ~CountGuard() { d.count = nullptr; }
};

// What both entries do around their pieces: [begin, end) of the text that `scan` reads, piece by piece, the chain from *chain on.
int count_pieces(acgpu_automaton *a, DeviceState &d, CountCall &c, uint64_t begin, uint64_t end, int64_t *chain, bool whole,
                 const PieceScan &scan) {
    const HostTables &t = a->t;
    c.direct_ok = false;
    if (t.mode == ACGPU_MODE_ALL && t.hy_n_states && !(tunables().count_form & 1))
        c.direct_ok = d.visits.ensure((size_t)t.hy_n_states * 4) == ACGPU_OK; // (no room: every piece takes the records form)
    PieceDriver p(begin, end, *chain, whole, ACGPU_REC_MAP, &d.count_res, &c.through_reservoir); // (the reservoir with what the pool holds from earlier calls)
    int rc = ACGPU_OK;
    for (uint64_t cnt, base; rc == ACGPU_OK && p.pos < p.end;) rc = scan_next_piece(p, scan, &cnt, &base);
    c.st.pieces = (uint32_t)p.pieces;
    c.st.rescans = (uint32_t)p.rescans;
    *chain = p.chain;
    if (rc) return rc;
    if (c.st.units_direct) HIP_TRY(launch_states_spread(d.T, (const uint32_t *)d.visits.p, c.d_counts, c.n_counts, scan.stream));
    return ACGPU_OK;
}

} // namespace

extern "C" {

int acgpu_count_u16(const acgpu_automaton *ca, const uint16_t *haystack, uint64_t n_units, uint64_t *counts, uint32_t n_counts,
                    acgpu_count_stats *st) {
    if (!ca || (n_units && !haystack) || (n_counts && !counts)) return ACGPU_E_INVALID;
    if (n_units >= (1ull << 31)) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    if (n_counts != a->n_given) return ACGPU_E_INVALID;
    PoolCall call(a); // (no device: fails here, as acgpu_match_u16 does, and counts is untouched)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    const hipStream_t stream = d.call_stream;
    int rc = call.on(stream);
    if (rc) return rc;
    if ((rc = d.count_out.ensure((size_t)n_counts * 8 + 8))) return rc;
    HIP_TRY(hipMemsetAsync(d.count_out.p, 0, (size_t)n_counts * 8 + 8, stream));
    CountCall c;
    c.d_counts = (unsigned long long *)d.count_out.p;
    c.n_counts = n_counts;
    CountGuard guard(d, &c);
    int64_t chain = 0;
    rc = count_pieces(a, d, c, 0, n_units, &chain, host_one_piece(a->t, ACGPU_REC_MAP), PieceScan{a, d, haystack, n_units, nullptr, stream});
    if (rc) return call.fail(rc); // (nothing of the call stays in flight behind its CountCall)
    if (n_counts) HIP_TRY(hipMemcpyAsync(counts, d.count_out.p, (size_t)n_counts * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (st) *st = c.st;
    return ACGPU_OK;
}

int acgpu_count_device(const acgpu_automaton *ca, acgpu_shard *shard, uint64_t *d_counts, uint32_t n_counts, void *stream_,
                       acgpu_count_stats *st) {
    if (!ca || !shard || (n_counts && !d_counts) || ((uintptr_t)d_counts & 7)) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    if (n_counts != a->n_given) return ACGPU_E_INVALID;
    if (shard->n_units >= (1ull << 31) || shard->own_begin > shard->own_end || shard->own_end > shard->n_units) return ACGPU_E_INVALID;
    PoolCall call(a);
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    const hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    int rc = call.on(stream);
    if (rc) return rc;
    CountCall c;
    c.d_counts = reinterpret_cast<unsigned long long *>(d_counts);
    c.n_counts = n_counts;
    CountGuard guard(d, &c);
    const ShardRule rule = shard_rule(a->t, ACGPU_REC_MAP, false);
    const bool whole = rule.sequential;
    int64_t chain = shard->chain_entry;
    rc = count_pieces(a, d, c, shard->own_begin, shard->own_end, &chain, whole, PieceScan{a, d, nullptr, 0, shard, stream});
    const hipError_t e = hipStreamSynchronize(stream); // the final wait (every shard call, direct or not, has waited for its own record count in collect())
    if (rc) return rc;
    HIP_TRY(e);
    if (rule.chain != Chain::None) shard->chain_exit = chain;
    if (st) *st = c.st;
    return ACGPU_OK;
}

} // extern "C"
