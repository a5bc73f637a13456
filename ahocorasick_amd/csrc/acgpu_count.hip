// acgpu_count.hip -- acgpu_count_u16 / acgpu_count_device (include/acgpu.h): how often every keyword occurs, without records.
//
// A counting call drives the text in pieces, as the cursor does (the same ramp and reservoir rules: PieceRamp), every piece as
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
#include <mutex>

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

// the pool's reservoir with room for `recs` Map records
int reservoir_for(DeviceState &d, uint64_t recs, uint64_t *have) {
    if (recs > *have) {
        const int rc = d.count_res.ensure(recs * ACGPU_REC_MAP + 64);
        if (rc) return rc;
        *have = recs;
    }
    return ACGPU_OK;
}

// What both entries do around their pieces.  scan(own_lo, size, chain, room, &cnt, &done): scans the owned units
// [own_lo, own_lo + size) with the chain's entry `*chain` (the entry's coordinates) into the reservoir of `room` records; on
// ACGPU_OK *chain is the exit; on ACGPU_E_OVERFLOW *cnt is what did not fit and *done the position up to which the piece has
// been counted all the same (*chain: the entry into the rest).
template <typename Scan>
int count_pieces(acgpu_automaton *a, DeviceState &d, CountCall &c, uint64_t begin, uint64_t end, int64_t *chain, bool whole,
                 hipStream_t stream, Scan scan) {
    const HostTables &t = a->t;
    c.direct_ok = false;
    if (t.mode == ACGPU_MODE_ALL && t.hy_n_states && !(tunables().count_form & 1))
        c.direct_ok = d.visits.ensure((size_t)t.hy_n_states * 4) == ACGPU_OK; // (no room: every piece takes the records form)
    const uint64_t budget_recs = std::max<uint64_t>(reservoir_budget_bytes() / ACGPU_REC_MAP, 1);
    uint64_t have = d.count_res.bytes > 64 ? (d.count_res.bytes - 64) / ACGPU_REC_MAP : 0; // (what the pool holds from earlier calls)
    PieceRamp ramp;
    ramp.start();
    uint64_t pos = begin;
    int rc;
    // The ramp's density is what the reservoir has to hold per unit of text: the units of a direct piece count, its records --
    // there are none to hold -- do not, so a text that has gone over to the direct form soon takes the largest pieces.
    while (pos < end) {
        uint64_t size = whole ? end - pos : ramp.next_size(end - pos, budget_recs);
        for (;;) {
            uint64_t room = ramp.predicted_room(size, budget_recs);
            if (whole || !room) room = std::min<uint64_t>(budget_recs, std::max<uint64_t>(whole ? size / 16 : size, 4096));
            if ((rc = reservoir_for(d, room, &have))) return rc;
            const uint64_t before = c.through_reservoir;
            uint64_t cnt = 0, done = pos;
            rc = scan(pos, size, chain, have, &cnt, &done);
            c.st.pieces++;
            if (rc == ACGPU_E_OVERFLOW) {
                c.st.rescans++;
                if (done > pos) ramp.advance(done - pos, c.through_reservoir - before); // (the shards in front of the one that did not fit)
                size -= done - pos;
                pos = done;
                uint64_t want = 0;
                if (whole) want = cnt; // (the one sequential scan: the exact count, past the budget if device memory allows)
                else if (!ramp.on_overflow(&size, cnt, budget_recs, &want)) return ACGPU_E_NOMEM;
                if ((rc = reservoir_for(d, want, &have))) return rc;
                continue;
            }
            if (rc) return rc;
            ramp.advance(size, c.through_reservoir - before);
            pos += size;
            break;
        }
    }
    if (c.st.units_direct) HIP_TRY(launch_states_spread(d.T, (const uint32_t *)d.visits.p, c.d_counts, c.n_counts, stream));
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
    DeviceState *dp = nullptr;
    int rc = device_for_call(a, &dp); // (no device: fails here, as acgpu_match_u16 does, and counts is untouched)
    if (rc) return rc;
    DeviceState &d = *dp;
    std::lock_guard<std::mutex> lock(d.mu);
    if (d.inflight > 0 && d.call_stream != d.inflight_stream) return ACGPU_E_INVALID; // stream rule (include/acgpu.h)
    const hipStream_t stream = d.call_stream;
    if ((rc = d.count_out.ensure((size_t)n_counts * 8 + 8))) return rc;
    HIP_TRY(hipMemsetAsync(d.count_out.p, 0, (size_t)n_counts * 8 + 8, stream));
    CountCall c;
    c.d_counts = (unsigned long long *)d.count_out.p;
    c.n_counts = n_counts;
    CountGuard guard(d, &c);
    const ShardRule rule = shard_rule(a->t, ACGPU_REC_MAP, false);
    const bool whole = one_piece(rule, a->t);
    int64_t chain = 0;
    rc = count_pieces(a, d, c, 0, n_units, &chain, whole, stream,
                      [&](uint64_t own_lo, uint64_t size, int64_t *ch, uint64_t room, uint64_t *cnt, uint64_t *done) -> int {
        const uint64_t own_hi = own_lo + size;
        if (whole) { // the text as one shard (the loops that exist only as one sequential kernel)
            int r2;
            if ((r2 = d.stage_hay.ensure(n_units * 2 + 16))) return r2;
            HIP_TRY(hipMemcpy(d.stage_hay.p, haystack, n_units * 2, hipMemcpyHostToDevice));
            acgpu_shard sh{};
            sh.d_hay = (const uint16_t *)d.stage_hay.p;
            sh.n_units = sh.own_end = n_units;
            sh.text_begin = sh.text_end = 1;
            return match_shard(a, d, &sh, ACGPU_REC_MAP, d.count_res.p, room, cnt, stream, nullptr);
        }
        const uint64_t lo = own_lo - std::min(rule.left, own_lo), hi = std::min<uint64_t>(n_units, own_hi + rule.right);
        int64_t rel = *ch - (int64_t)lo; // (buffer relative: scan_host_range takes each shard's entry from it)
        uint64_t done_rel = own_lo - lo;
        const int r2 = scan_host_range(a, d, haystack, n_units, lo, hi, own_lo, own_hi, ACGPU_REC_MAP, room, cnt, &rel, d.count_res.p, &done_rel);
        if (r2 == ACGPU_OK || r2 == ACGPU_E_OVERFLOW) {
            *ch = rel + (int64_t)lo;
            *done = lo + done_rel;
        }
        return r2;
    });
    if (rc) {
        (void)hipStreamSynchronize(stream); // (nothing of the call stays in flight behind its CountCall)
        return rc;
    }
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
    DeviceState *dp = nullptr;
    int rc = device_for_call(a, &dp);
    if (rc) return rc;
    DeviceState &d = *dp;
    std::lock_guard<std::mutex> lock(d.mu);
    const hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (d.inflight > 0 && stream != d.inflight_stream) return ACGPU_E_INVALID; // stream rule (include/acgpu.h)
    CountCall c;
    c.d_counts = reinterpret_cast<unsigned long long *>(d_counts);
    c.n_counts = n_counts;
    CountGuard guard(d, &c);
    const ShardRule rule = shard_rule(a->t, ACGPU_REC_MAP, false);
    const bool whole = rule.sequential;
    int64_t chain = shard->chain_entry;
    rc = count_pieces(a, d, c, shard->own_begin, shard->own_end, &chain, whole, stream,
                      [&](uint64_t own_lo, uint64_t size, int64_t *ch, uint64_t room, uint64_t *cnt, uint64_t *) -> int {
        acgpu_shard sh = *shard; // the caller's buffer, a moving owned range
        sh.own_begin = own_lo;
        sh.own_end = own_lo + size;
        sh.d_result = nullptr;
        const int64_t entry = rule.chain == Chain::None ? shard->chain_entry : piece_entry(rule, *ch, 0, own_lo);
        sh.chain_entry = entry;
        const int r2 = match_shard(a, d, &sh, ACGPU_REC_MAP, d.count_res.p, room, cnt, stream, nullptr);
        if (r2 == ACGPU_OK) *ch = piece_exit(rule, entry, sh.own_end, &sh, *cnt);
        return r2;
    });
    const hipError_t e = hipStreamSynchronize(stream); // the final wait (every shard call, direct or not, has waited for its own record count in collect())
    if (rc) return rc;
    HIP_TRY(e);
    if (rule.chain != Chain::None) shard->chain_exit = chain;
    if (st) *st = c.st;
    return ACGPU_OK;
}

} // extern "C"
