// acgpu_hostrun.hip -- the families that need the host between their launches (CallForm::HostRun): the selection over the
// all-matches list (SHORTEST, sparse LONGEST), the two sequential word kernels, and the WholeWordLongest walk.
#include <algorithm>

#include "acgpu_calls.h"

using namespace acgpu;

namespace {

// Marks the chain k0, nxt[k0], nxt[nxt[k0]], ... (nxt[k] in (k, M], nxt[M] = M; d_mark[k0] = 1 on entry, every other mark 0):
// afterwards d_mark[k] = 1 exactly for the chain's elements.  One pass when the jumps are short: with nxt[k] - k as the
// "length" this is the greedy chain of LongestMatchSet, and the Longest chain kernels mark it (tiles of indices with
// synchronisation points, one lane per tile, a bit per visited index; acgpu_longest.hip, acgpu_wwlongest.hip: k_wwl_jumps);
// pointer doubling -- ceil(log2 M) rounds over all M elements -- otherwise (tiny inputs, jumps beyond 16 bits, tunable
// tile_debug bit kSelMarkDoubling).  The doubling squares the jump table: *d_nxt_kept is where the successors survive
// (d_nxt itself, or d_nxt_copy -- M + 1 words, may be null if the caller does not need them).
// jump_bound: what the caller knows nxt[k] - k cannot exceed (0: unknown -- the largest jump is measured).  The one pass has a
// fixed cost (a read-back, four small launches) that 21 doubling rounds over a million elements do not reach: it is taken
// from 4 M elements on.
int mark_chain(DeviceState &d, uint32_t *d_nxt, uint32_t *d_tmp, uint32_t *d_mark, uint32_t M, hipStream_t stream,
               uint32_t *d_nxt_copy, const uint32_t **d_nxt_kept, uint32_t jump_bound) {
    int rc;
    if (d_nxt_kept) *d_nxt_kept = d_nxt;
    // (tunable tile_debug: kSelMarkDoubling = always the doubling, kSelMarkOnePassEarly = the one pass from 64 elements on -- tests)
    const uint32_t one_pass_from = (tunables().tile_debug & kSelMarkOnePassEarly) ? 64u : (1u << 22);
    bool one_pass = M >= one_pass_from && jump_bound <= 60000 && !(tunables().tile_debug & kSelMarkDoubling);
    uint64_t head = ~0ull, max_jump = 0;
    if (one_pass) {
        // counter words used here: [2] chain head, [3] largest jump (bytes 16..32) of the line the caller has borrowed
        // (borrow_counter_line)
        static_assert(kCounterStride >= 4, "mark_chain keeps its head and largest jump in words 2 and 3 of the first counter line");
        if ((rc = d.lenbuf.ensure((size_t)M * 2 + 128))) return rc;
        if ((rc = d.blockmax.ensure(((size_t)M / 64 + 2) * 4))) return rc;
        HIP_TRY(hipMemsetAsync((char *)d.counter.p + 16, 0xff, 8, stream)); // the chain head's index (none: all ones)
        HIP_TRY(hipMemsetAsync((char *)d.counter.p + 24, 0, 8, stream));    // the largest jump
        HIP_TRY(launch_wwl_jumps(d_nxt, d_mark, M, (uint16_t *)d.lenbuf.p, (uint32_t *)d.blockmax.p,
                                 (unsigned long long *)d.counter.p + 2, jump_bound == 0, stream));
        HIP_TRY(hipMemcpyAsync(d.h_counter + kPoolChainHead, (const char *)d.counter.p + 16, 16, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        head = d.h_counter[kPoolChainHead];
        max_jump = jump_bound ? jump_bound : d.h_counter[kPoolChainHead + 1];
        if (head >= M) return ACGPU_OK; // no head: nothing is marked, nothing to mark
        if (max_jump > 60000) one_pass = false;
    }
    if (!one_pass) {
        if (d_nxt_copy) {
            HIP_TRY(hipMemcpyAsync(d_nxt_copy, d_nxt, ((size_t)M + 1) * 4, hipMemcpyDeviceToDevice, stream));
            if (d_nxt_kept) *d_nxt_kept = d_nxt_copy;
        }
        HIP_TRY(launch_chain_mark(d_nxt, d_tmp, d_mark, M, stream));
        return ACGPU_OK;
    }
    // (jumps are ~1, so a lane makes about one step per index: short tiles, i.e. many lanes)
    const uint32_t tile_units = 512;
    const size_t bit_bytes = ((size_t)M / 128 + 2) * 16;
    if ((rc = d.chainbits.ensure(bit_bytes))) return rc;
    HIP_TRY(hipMemsetAsync(d.chainbits.p, 0, bit_bytes, stream));
    LongestChainLaunch Cn{};
    Cn.d_len = d.lenbuf.p;
    Cn.len_bytes = 2;
    Cn.own_begin = 0;
    Cn.own_end = M;
    Cn.d_blockmax = (const uint32_t *)d.blockmax.p;
    Cn.entry = (uint32_t)head;
    Cn.tile_units = tile_units;
    Cn.n_tiles = (uint32_t)(((uint64_t)M - head + tile_units - 1) / tile_units);
    Cn.max_len = (uint32_t)std::max<uint64_t>(max_jump, 1);
    if ((rc = d.chunk_counts.ensure((size_t)Cn.n_tiles * 4))) return rc;
    Cn.d_counts = (uint32_t *)d.chunk_counts.p; // (per-tile counts nobody reads)
    Cn.d_exit = (unsigned long long *)d.counter.p + 3;
    Cn.len_units = M;
    Cn.d_bits = (uint32_t *)d.chainbits.p;
    Cn.record_kind = ACGPU_REC_SET;
    if ((rc = d.chain.ensure((size_t)Cn.n_tiles * 4 + 64))) return rc;
    HIP_TRY(launch_longest_sync(Cn, (uint32_t *)d.chain.p, stream));
    HIP_TRY(launch_longest_chain_lds(Cn, (const uint32_t *)d.chain.p, stream));
    HIP_TRY(launch_wwl_bits_to_mark((const uint32_t *)d.chainbits.p, M, d_mark, stream));
    return ACGPU_OK;
}

// SHORTEST, and LONGEST where matches are sparse, as a selection over the all-matches list: the ALL pipeline over `all` into an
// internal buffer (all matches, end ascending, longest first, with keyword ids; retried once with the exact capacity), every
// record's successor (k_short_next; leftmost_longest: k_long_next), the chain from `entry` marked, its records written out.
// More than dense_limit matches: ACGPU_E_UNSUPPORTED.  r.shard.chain_exit: the exit the caller has preset.
int run_selection(acgpu_automaton *a, DeviceState &d, CallRecord &r, acgpu_shard all, int64_t entry, uint64_t dense_limit,
                  bool leftmost_longest) {
    const hipStream_t stream = r.stream;
    const uint64_t own_len = r.shard.own_end - r.shard.own_begin;
    int rc;
    uint64_t m = 0;
    // what the buffer already holds (its size includes 16 spare bytes), or a first guess
    uint64_t acap = std::max<uint64_t>(d.short_recs.bytes > 16 ? (d.short_recs.bytes - 16) / ACGPU_REC_MAP : 0, own_len / 32 + (1 << 16));
    for (;;) {
        if ((rc = d.short_recs.ensure(acap * ACGPU_REC_MAP + 16))) return rc;
        rc = run_inside(enqueue_all, a, d, r, &all, ACGPU_REC_MAP, d.short_recs.p, acap, &m);
        if (m > dense_limit && (rc == ACGPU_OK || rc == ACGPU_E_OVERFLOW)) return ACGPU_E_UNSUPPORTED;
        if (rc == ACGPU_OK) break;
        if (rc != ACGPU_E_OVERFLOW) return rc;
        acap = m;
    }
    if (m == 0) return close_as_inside(r, 0, r.shard.chain_exit); // (nothing to select from)
    if (m >= 0xfffffff0ull) return ACGPU_E_UNSUPPORTED; // (the selection's indices are 32 bits wide)
    const uint32_t M = (uint32_t)m;
    if ((rc = d.short_nxt.ensure(((size_t)M + 1) * 4))) return rc;
    if ((rc = d.short_tmp.ensure(((size_t)M + 1) * 4))) return rc;
    if ((rc = d.short_mark.ensure(((size_t)M + 1) * 4))) return rc;
    if ((rc = d.offsets.ensure((size_t)M * 8))) return rc;
    if ((rc = ensure_scan_tmp(d, M))) return rc;
    if ((rc = borrow_counter_line(d, stream, /*clear=*/false))) return rc; // (the exit position; mark_chain's words)
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[0], stream));
    if (leftmost_longest)
        HIP_TRY(launch_longest_select((const int32_t *)d.short_recs.p, M, entry, (int64_t)r.shard.own_end, a->t.max_len,
                                      (uint32_t *)d.short_nxt.p, (uint32_t *)d.short_mark.p, stream));
    else
        HIP_TRY(launch_shortest_select((const int32_t *)d.short_recs.p, M, entry, (uint32_t *)d.short_nxt.p, (uint32_t *)d.short_mark.p, stream));
    if ((rc = mark_chain(d, (uint32_t *)d.short_nxt.p, (uint32_t *)d.short_tmp.p, (uint32_t *)d.short_mark.p, M, stream, nullptr,
                         nullptr, 0)))
        return rc;
    HIP_TRY(launch_exclusive_scan((const uint32_t *)d.short_mark.p, M, (uint64_t *)d.offsets.p, (uint64_t *)d.scan_tmp.p, stream));
    const uint64_t *d_total = scan_total(d, M);
    HIP_TRY(launch_shortest_emit((const int32_t *)d.short_recs.p, M, (const uint32_t *)d.short_mark.p, (const uint64_t *)d.offsets.p,
                                 d_total, r.record_kind, r.d_out, r.cap, entry, (unsigned long long *)d.counter.p, stream));
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[1], stream));
    r.behind_pass = true; // (the ordering of the all-matches list + the selection)
    if ((rc = close_host_run(r, d_total, d.counter.p, r.inside.scan_kernel, leftmost_longest ? own_len : r.inside.scan_units))) return rc;
    // LONGEST: the chain leaves the owned range at the end of its last match, or walks out of it one unit at a time
    if (leftmost_longest)
        r.h_slot[kSlotExit] = r.h_slot[kSlotCount] ? std::max<unsigned long long>(r.h_slot[kSlotExit], r.shard.own_end)
                                                   : (unsigned long long)r.shard.chain_exit;
    return ACGPU_OK;
}

} // namespace

namespace acgpu { // (what acgpu_calls.h and acgpu_host.h declare: described there)

int run_shortest(acgpu_automaton *a, DeviceState &d, CallRecord &r) {
    const int64_t entry = r.shard.chain_entry > 0 ? r.shard.chain_entry : 0;
    r.user_shard->chain_exit = r.shard.chain_exit = entry;
    return run_selection(a, d, r, r.shard, entry, ~0ull, false);
}

int run_longest_sparse(acgpu_automaton *a, DeviceState &d, CallRecord &r) {
    const HostTables &t = a->t;
    int rc;
    if ((rc = check_longest_shard(t, &r.shard))) return rc;
    r.user_shard->chain_exit = r.shard.chain_exit;
    const acgpu_shard &sh = r.shard;
    if ((uint64_t)sh.chain_entry >= sh.own_end || t.n_states <= 1) return enqueue_empty(r, sh.chain_exit);
    acgpu_shard all = sh; // every occurrence that ENDS in the owned range or its right halo
    all.own_end = std::min<uint64_t>(sh.n_units, sh.own_end + (t.max_len > 0 ? t.max_len - 1 : 0));
    all.text_begin = 1; // occurrences that begin before the buffer begin before own_begin: not ours anyway
    return run_selection(a, d, r, all, sh.chain_entry, (sh.own_end - sh.own_begin) / 4 + 4096, true);
}

int run_wholeword_sequential(acgpu_automaton *, DeviceState &d, CallRecord &r) {
    const acgpu_shard &sh = r.shard;
    const uint64_t own_len = sh.own_end - sh.own_begin;
    if (own_len == 0) return enqueue_empty(r, sh.chain_exit);
    int rc;
    if ((rc = borrow_counter_line(d, r.stream, /*clear=*/true))) return rc;
    if (!sh.text_begin || !sh.text_end || sh.own_begin != 0 || sh.own_end != sh.n_units) return ACGPU_E_UNSUPPORTED;
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[0], r.stream));
    HIP_TRY(launch_ww_sequential(d.T, sh.d_hay, (uint32_t)sh.n_units, r.d_out, r.cap, r.record_kind, (unsigned long long *)d.counter.p,
                                 r.stream));
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[2], r.stream));
    r.one_kernel = true;
    r.h_slot[kSlotExit] = (unsigned long long)sh.chain_exit; // (no chain: the caller's word stays what it is)
    return close_host_run(r, d.counter.p, nullptr, "k_ww_sequential", own_len);
}

int run_wwlongest_sequential(acgpu_automaton *a, DeviceState &d, CallRecord &r) {
    const acgpu_shard &sh = r.shard;
    const uint32_t n = (uint32_t)sh.n_units;
    const int64_t entry = std::max<int64_t>(sh.chain_entry, (int64_t)sh.own_begin);
    r.user_shard->chain_exit = entry;
    int rc;
    if (!sh.text_begin || !sh.text_end || sh.own_begin != 0 || sh.own_end != sh.n_units) return ACGPU_E_UNSUPPORTED;
    if (n == 0 || a->t.n_states <= 1) return enqueue_empty(r, entry);
    if ((rc = borrow_counter_line(d, r.stream, /*clear=*/false))) return rc;
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[0], r.stream));
    HIP_TRY(launch_wwl_sequential(d.T, sh.d_hay, n, r.d_out, r.cap, r.record_kind, (unsigned long long *)d.counter.p, r.stream));
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[2], r.stream));
    r.one_kernel = true;
    r.h_slot[kSlotExit] = n;
    return close_host_run(r, d.counter.p, nullptr, "k_wwl_sequential", n);
}

int run_wwlongest(acgpu_automaton *a, DeviceState &d, CallRecord &r, const DevTables &T, bool plain_words) {
    const HostTables &t = a->t;
    const acgpu_shard *sh = &r.shard;
    const hipStream_t stream = r.stream;
    const uint32_t n = (uint32_t)sh->n_units;
    const uint64_t entry = (uint64_t)std::max<int64_t>(sh->chain_entry, (int64_t)sh->own_begin);
    r.user_shard->chain_exit = (int64_t)entry;
    int rc;
    if (!sh->text_begin && sh->own_begin < 1) return ACGPU_E_INVALID;                              // left context: 1 unit
    if (!sh->text_end && sh->n_units - sh->own_end < (uint64_t)t.max_len + 1) return ACGPU_E_INVALID; // right halo
    if (n == 0 || t.n_states <= 1 || sh->own_end == sh->own_begin || entry >= sh->own_end) return enqueue_empty(r, (int64_t)entry);
    const uint32_t n_tiles = wwl_tiles(n);
    if ((rc = ensure_scan_buffers(d, n_tiles))) return rc;
    if ((rc = borrow_counter_line(d, stream, /*clear=*/false))) return rc; // (the exit position; mark_chain's words)
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[0], stream));
    HIP_TRY(launch_wwl_starts(T, sh->d_hay, n, d.n_cu, false, (uint32_t *)d.chunk_counts.p, nullptr, nullptr, sh->text_begin, d.start_behind, stream));
    HIP_TRY(launch_exclusive_scan((const uint32_t *)d.chunk_counts.p, n_tiles, (uint64_t *)d.offsets.p, (uint64_t *)d.scan_tmp.p,
                                  stream));
    HIP_TRY(hipMemcpyAsync(r.h_slot + kSlotCount, scan_total(d, n_tiles), 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint32_t M = (uint32_t)r.h_slot[kSlotCount]; // walk starts of the buffer (halos included)
    if (M == 0) return enqueue_empty(r, (int64_t)entry);
    if ((rc = d.wwl_rs.ensure(((size_t)M + 1) * 4))) return rc;
    if ((rc = d.wwl_mend.ensure(((size_t)M + 1) * 4))) return rc;
    if ((rc = d.wwl_mid.ensure(((size_t)M + 1) * 4))) return rc;
    if ((rc = d.wwl_sel.ensure(((size_t)M + 1) * 4))) return rc;
    if ((rc = d.wwl_stop.ensure(((size_t)M + 1) * 4))) return rc;
    if ((rc = d.short_nxt.ensure(((size_t)M + 1) * 4))) return rc;
    if ((rc = d.short_tmp.ensure(((size_t)M + 1) * 4))) return rc;
    if ((rc = d.short_mark.ensure(((size_t)M + 1) * 4))) return rc;
    { // the exit position, preset to the entry (no visited walk start: nothing changes hands)
        r.h_slot[kSlotExit] = entry;
        HIP_TRY(hipMemcpyAsync(d.counter.p, r.h_slot + kSlotExit, 8, hipMemcpyHostToDevice, stream));
    }
    HIP_TRY(launch_wwl_starts(T, sh->d_hay, n, d.n_cu, true, nullptr, (const uint64_t *)d.offsets.p, (uint32_t *)d.wwl_rs.p,
                              sh->text_begin, d.start_behind, stream));
    HIP_TRY(launch_wwl_walk(T, plain_words, sh->d_hay, n, (const uint32_t *)d.wwl_rs.p, M, (uint32_t *)d.short_nxt.p,
                            (uint32_t *)d.short_mark.p, (int32_t *)d.wwl_mend.p, (int32_t *)d.wwl_mid.p, (uint32_t *)d.wwl_stop.p,
                            (uint32_t)entry, d.n_cu, stream));
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[1], stream));
    // Which starts does the scan visit?  The chain k0, NXT[k0], ... over the start indices: mark_chain (one pass -- a walk
    // runs over few later starts; pointer doubling took 2.5 ms of 8.4 on config 5's text).  The select pass needs the
    // successors afterwards.
    const uint32_t *nxt_for_select = nullptr;
    if ((rc = d.wwl_nxt0.ensure(((size_t)M + 1) * 4))) return rc;
    if ((rc = mark_chain(d, (uint32_t *)d.short_nxt.p, (uint32_t *)d.short_tmp.p, (uint32_t *)d.short_mark.p, M, stream,
                         (uint32_t *)d.wwl_nxt0.p, &nxt_for_select, t.max_len / 2 + 2)))
        return rc;
    HIP_TRY(launch_wwl_select((const uint32_t *)d.short_mark.p, (const int32_t *)d.wwl_mend.p, (const uint32_t *)d.wwl_rs.p,
                              nxt_for_select, (const uint32_t *)d.wwl_stop.p, (uint32_t *)d.wwl_sel.p, M,
                              (uint32_t)sh->own_begin, (uint32_t)sh->own_end, (unsigned long long *)d.counter.p, stream));
    if (scan_tile_elems() != 2048) return ACGPU_E_INVALID; // (k_wwl_emit ranks one prefix-sum tile per workgroup)
    if ((rc = ensure_scan_tmp(d, M))) return rc;
    HIP_TRY(launch_scan_tile_offsets((const uint32_t *)d.wwl_sel.p, M, (uint64_t *)d.scan_tmp.p, stream));
    HIP_TRY(launch_wwl_emit((const uint32_t *)d.wwl_rs.p, (const uint32_t *)d.wwl_sel.p, (const int32_t *)d.wwl_mend.p,
                            (const int32_t *)d.wwl_mid.p, (const uint64_t *)d.scan_tmp.p, M, r.record_kind, r.d_out, r.cap, stream));
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[2], stream));
    return close_host_run(r, scan_total(d, M), d.counter.p, "k_wwl_walk", n);
}

} // namespace acgpu
