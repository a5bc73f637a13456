// acgpu_call.hip -- a shard call's life below the ABI: the call record is opened, a pipeline of the automaton's family is
// enqueued into it (or runs to its end on the host), and collect() completes it -- for the pool's own synchronous calls and for
// tickets alike; the acgpu_match_device* entries.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>

#include "acgpu_calls.h"

using namespace acgpu;

namespace {

// ---- the call record: enqueue, then collect() ----

// Starts a call in `r`: the call's arguments, the record's events and pinned slot (done: a ticket's completion marker, null for a
// synchronous call).  Until a form fills it in, the record is complete with nothing found.
void open_call(CallRecord &r, const PoolEvent *ev, hipEvent_t done, unsigned long long *slot, const acgpu_shard &sh, acgpu_shard *user,
               int record_kind, void *d_out, uint64_t cap, hipStream_t stream, bool profiled, bool folded) {
    r = CallRecord{};
    r.shard = sh; r.user_shard = user; r.record_kind = record_kind; r.d_out = d_out; r.cap = cap; r.stream = stream;
    r.ev = ev; r.done = done; r.h_slot = slot; r.profiled = profiled; r.folded = folded;
}

// what a ticket's call is complete with: its marker, or the last kernel's own end
hipEvent_t completion(const CallRecord &r) { return r.done_is_ev2 ? r.ev[2] : r.done; }

// The level a call has to be redone at, or -1.  ALL: an overflow word raised by the scan (a candidate slice of the split form
// or a scratch slice was too small) -> 1, the fused kernel with one scratch slice.  LONGEST: the bail flag of k_longest_bits /
// k_longest_follow (1: a chain that did not merge inside the run-up, 2: a unit outside the alphabet) -> the next run-up level,
// or 2, the walk pipeline.  A redo is always at a higher level, and the forms of the last levels never ask for one.
int redo_level(const CallRecord &r) {
    const unsigned long long flag = r.h_slot[kSlotFlag];
    if (r.form == CallForm::Ordered || r.form == CallForm::FusedTail) return r.level == 0 && (uint32_t)flag != 0 ? 1 : -1;
    if (r.form == CallForm::LongestBits || r.form == CallForm::LongestFollow) return flag == 0 ? -1 : flag == 1 ? r.level + 1 : 2;
    return -1;
}

} // namespace

namespace acgpu { // (what acgpu_calls.h and acgpu_host.h declare: described there)

int slot_on_device(const CallRecord &r, unsigned long long **d_slot) {
    HIP_TRY(hipHostGetDevicePointer((void **)d_slot, r.h_slot, 0));
    return ACGPU_OK;
}

int close_call(CallRecord &r, CallForm form, const char *kname, uint64_t scanned, bool done_is_ev2) {
    r.form = form;
    r.scanned = scanned;
    std::snprintf(r.kname, sizeof(r.kname), "%.*s", (int)sizeof(r.kname) - 1, kname); // (the one cut: acgpu_profile::scan_kernel holds 63 characters)
    r.done_is_ev2 = done_is_ev2;
    if (r.done && !done_is_ev2) HIP_TRY(hipEventRecord(r.done, r.stream));
    return ACGPU_OK;
}

int enqueue_empty(CallRecord &r, int64_t chain_exit) {
    r.h_slot[kSlotCount] = r.h_slot[kSlotFlag] = 0;
    r.h_slot[kSlotExit] = (unsigned long long)chain_exit;
    if (r.shard.d_result) HIP_TRY(hipMemsetAsync(r.shard.d_result, 0, sizeof(acgpu_device_result), r.stream));
    return close_call(r, CallForm::Complete, "", 0);
}

int close_host_run(CallRecord &r, const void *d_count, const void *d_exit, const char *kname, uint64_t scanned) {
    HIP_TRY(hipMemcpyAsync(r.h_slot + kSlotCount, d_count, 8, hipMemcpyDeviceToHost, r.stream));
    if (d_exit) HIP_TRY(hipMemcpyAsync(r.h_slot + kSlotExit, d_exit, 8, hipMemcpyDeviceToHost, r.stream));
    HIP_TRY(hipStreamSynchronize(r.stream));
    return close_call(r, CallForm::HostRun, kname, scanned);
}

int borrow_counter_line(DeviceState &d, hipStream_t stream, bool clear) {
    int rc;
    if ((rc = d.counter.ensure(64))) return rc;
    if (clear) HIP_TRY(hipMemsetAsync(d.counter.p, 0, 64, stream));
    d.cclean[0] = false;
    return ACGPU_OK;
}

int run_inside(EnqueueFn enqueue, acgpu_automaton *a, DeviceState &d, CallRecord &r, acgpu_shard *sh, int record_kind, void *d_out,
               uint64_t cap, uint64_t *n_out) {
    const CallRecord outer = r;
    acgpu_profile inside{};
    open_call(d.call, d.ev, nullptr, d.h_counter, *sh, sh, record_kind, d_out, cap, outer.stream, outer.profiled, false);
    int rc = enqueue(a, d, d.call, 0);
    if (rc == ACGPU_OK) rc = collect(a, d, &d.call, n_out, outer.profiled ? &inside : nullptr, nullptr);
    r = outer;
    r.inside = inside;
    return rc;
}

int close_as_inside(CallRecord &r, uint64_t n, int64_t chain_exit) {
    r.profiled = false; // (no events of its own)
    r.h_slot[kSlotCount] = n;
    r.h_slot[kSlotExit] = (unsigned long long)chain_exit;
    return close_call(r, CallForm::HostRun, r.inside.scan_kernel, r.inside.scan_units);
}

int collect(acgpu_automaton *a, DeviceState &d, CallRecord *r, uint64_t *n_out, acgpu_profile *prof, bool *redone) {
    for (;;) {
        if (!r->done && r->form != CallForm::Complete && r->form != CallForm::HostRun) HIP_TRY(hipStreamSynchronize(r->stream));
        const int level = redo_level(*r);
        if (level < 0) break;
        const bool longest = r->form != CallForm::Ordered && r->form != CallForm::FusedTail;
        if (r->form == CallForm::LongestFollow) d.fol_level = std::max(d.fol_level, r->level + 1); // (the pool's later calls start there)
        // (the redo shares the scratch with the tickets still in flight: same stream, so stream order keeps them apart)
        acgpu_shard sh = r->shard;
        const bool counting = r->counting;
        if (longest && r->done) sh.d_result = nullptr; // (a ticket's Longest redo leaves the device result to the first attempt, which says "redone")
        open_call(d.call, d.ev, nullptr, d.h_counter, sh, r->user_shard, r->record_kind, r->d_out, r->cap, r->stream, prof != nullptr,
                  r->folded);
        d.call.counting = counting;
        if (redone) *redone = true;
        const int rc = longest ? enqueue_longest(a, d, d.call, level) : enqueue_all(a, d, d.call, level);
        if (rc) return rc;
        r = &d.call;
    }
    *n_out = r->h_slot[kSlotCount];
    if (r->form == CallForm::LongestBits || r->form == CallForm::LongestFollow || r->form == CallForm::LongestWalk || r->form == CallForm::HostRun)
        r->user_shard->chain_exit = (int64_t)r->h_slot[kSlotExit];
    else if (r->form != CallForm::Complete && a->t.mode != ACGPU_MODE_WHOLEWORD) // (what the states form's choice goes by)
        d.all_density = (double)*n_out / (double)(r->shard.own_end - r->shard.own_begin);
    if (prof) *prof = r->inside; // (zero, but for a host-run call with a pass inside)
    if (prof && r->form != CallForm::Complete) {
        if (r->profiled && r->behind_pass) {
            float behind_ms = 0;
            HIP_TRY(hipEventElapsedTime(&behind_ms, r->ev[0], r->ev[1]));
            prof->finalize_ms += behind_ms;
            prof->total_ms += behind_ms;
        } else if (r->profiled && r->one_kernel) {
            HIP_TRY(hipEventElapsedTime(&prof->scan_ms, r->ev[0], r->ev[2]));
            prof->total_ms = prof->scan_ms;
        } else if (r->profiled) {
            HIP_TRY(hipEventElapsedTime(&prof->scan_ms, r->ev[0], r->ev[1]));
            HIP_TRY(hipEventElapsedTime(&prof->finalize_ms, r->ev[1], r->ev[2]));
            HIP_TRY(hipEventElapsedTime(&prof->total_ms, r->ev[0], r->ev[2]));
        }
        prof->scan_units = r->scanned;
        prof->n_matches = *n_out;
        std::snprintf(prof->scan_kernel, sizeof(prof->scan_kernel), "%s", r->kname);
    }
    if (r->counting) return count_collected(d, *r, *n_out);
    return *n_out > r->cap ? ACGPU_E_OVERFLOW : ACGPU_OK;
}

// ---- cutting a text into shards ------------------------------------------------------------------------------
// ALL / SHORTEST: a match belongs to the piece that owns its last unit; LONGEST: to the piece that owns its first unit; the word
// matchers: a word belongs to the piece that owns its first unit, whose left neighbour decides whether it starts a word.
ShardRule shard_rule(const HostTables &t, int record_kind, bool readable) {
    const uint64_t m = t.max_len, h = m ? m - 1 : 0;
    switch (t.mode) { // ShardRule{left, right, chain, sequential, all_pipeline}
    case ACGPU_MODE_ALL: return ShardRule{h, 0, Chain::None, false, true};
    case ACGPU_MODE_SHORTEST: return ShardRule{h, 0, Chain::Restart, false, false};
    case ACGPU_MODE_LONGEST: return ShardRule{0, h, Chain::Position, false, false};
    case ACGPU_MODE_WHOLEWORD:
        // not fold-consistent: the String loop mixes folded and raw lookups (sequential); the Readable loop folds in every
        // lookup: the pipeline over the folded tables, or the WholeWordLongest walk where folded keywords hold non-word units
        if (t.fold_consistent || (readable && t.fold_clean)) return ShardRule{1, m + 1, Chain::None, false, true};
        return readable ? ShardRule{1, m + 1, Chain::Position, false, false} : ShardRule{1, m + 1, Chain::None, true, false};
    case ACGPU_MODE_WWLONGEST: // (not fold-consistent: only the Set class's String loop mixes folded and raw lookups)
        return ShardRule{1, m + 1, Chain::Position, !t.fold_consistent && record_kind == ACGPU_REC_SET && !readable, false};
    default: return ShardRule{};
    }
}

// the checks of match_shard and begin_shard (include/acgpu.h), after the call's view of the tunables is refreshed
int check_shard(acgpu_automaton *a, DeviceState &d, const acgpu_shard *sh, int record_kind, const void *d_out, uint64_t cap,
                hipStream_t stream) {
    refresh_call_state(a, d);
    if (record_kind != ACGPU_REC_SET && record_kind != ACGPU_REC_MAP) return ACGPU_E_INVALID;
    if (sh->n_units >= (1ull << 31) || sh->own_begin > sh->own_end || sh->own_end > sh->n_units) return ACGPU_E_INVALID;
    if (sh->n_units && (!sh->d_hay || ((uintptr_t)sh->d_hay & 15))) return ACGPU_E_INVALID;
    if (cap && (!d_out || ((uintptr_t)d_out & 3))) return ACGPU_E_INVALID;
    if (sh->d_result && ((uintptr_t)sh->d_result & 15)) return ACGPU_E_INVALID;
    if (d.inflight > 0 && stream != d.inflight_stream) return ACGPU_E_INVALID; // stream rule (include/acgpu.h)
    return ACGPU_OK;
}

// One call on a checked shard into its record -- the pool's own (tk null: a synchronous call, which the caller collects at once)
// or a ticket's -- by the pipeline of the automaton's family.  Enqueued without waiting: the AhoCorasick / WholeWord pipeline
// (one scan + ordering pass) and the LongestMatch pipelines (nothing of them needs the host).  The other families -- and
// LongestMatch over a dictionary with a selective suffix filter, whose sparse form falls back to the walk after looking at the
// match count -- need the host between their launches and run to their end here (CallForm::HostRun): such a ticket is complete
// when _begin returns (no completion marker: nothing in flight, the stream rule does not apply to it); only its bookkeeping
// waits for collect().
// readable: the call stands for match(Readable, ...) (acgpu_stream_feed) -- the word matchers' Readable loops fold in every
// lookup where their String loops mix folded and raw ones, which only matters for tables that are not fold-consistent.
static int start_call(acgpu_automaton *a, DeviceState &d, Ticket *tk, acgpu_shard *sh, int record_kind, void *d_out, uint64_t cap,
                      hipStream_t stream, bool profiled, bool readable) {
    const HostTables &t = a->t;
    const ShardRule rule = shard_rule(t, record_kind, readable);
    const bool enqueued = rule.all_pipeline || (t.mode == ACGPU_MODE_LONGEST && !(filter_is_selective(t) && tunables().force_kernel != 1));
    CallRecord &r = tk ? tk->rec : d.call;
    // (all_pipeline over tables that are not fold-consistent: the Readable loop of WholeWord, an ordinary scan over w' = word o lower)
    open_call(r, tk ? tk->ev : d.ev, tk && enqueued ? tk->done.h : nullptr, tk ? tk->h_count : d.h_counter, *sh, sh, record_kind, d_out, cap,
              stream, profiled, rule.all_pipeline && !t.fold_consistent);
    r.counting = d.count != nullptr;
    if (rule.all_pipeline) return enqueue_all(a, d, r, 0);
    if (enqueued) return enqueue_longest(a, d, r, 0);
    // a host-run call ends with its count on the host (and some run the ALL pipeline inside): the device copy of the result is
    // written behind the pipeline
    r.shard.d_result = nullptr;
    int rc;
    switch (t.mode) {
    case ACGPU_MODE_LONGEST:
        // a selective suffix filter: a selection over all matches, unless the text turns out to be dense in them -- then the
        // walk after all, as a pass inside
        rc = run_longest_sparse(a, d, r);
        if (rc == ACGPU_E_UNSUPPORTED) {
            acgpu_shard walk = r.shard;
            uint64_t n = 0;
            rc = run_inside(enqueue_longest, a, d, r, &walk, record_kind, d_out, cap, &n);
            if (rc == ACGPU_OK || rc == ACGPU_E_OVERFLOW) rc = close_as_inside(r, n, walk.chain_exit);
        }
        break;
    case ACGPU_MODE_WHOLEWORD:
        if (rule.sequential) {
            rc = run_wholeword_sequential(a, d, r);
        } else { // Readable, folded keywords with non-word units: the WholeWordLongest walk without fail matches, unit by unit
            DevTables Tf = folded_tables(d);
            Tf.ww_fat = nullptr;
            rc = run_wwlongest(a, d, r, Tf, true);
        }
        break;
    case ACGPU_MODE_SHORTEST: rc = run_shortest(a, d, r); break;
    case ACGPU_MODE_WWLONGEST:
        // not fold-consistent: the Map class's String loop and both Readable loops fold in every lookup
        // (S/WholeWordLongestMatchMap.java:252-288, :404) -- position parallel over w'; the Set class's String loop mixes
        // raw and folded lookups (S/WholeWordLongestMatchSet.java:126,151,156) -- sequential
        if (rule.sequential) rc = run_wwlongest_sequential(a, d, r);
        else rc = run_wwlongest(a, d, r, t.fold_consistent ? d.T : folded_tables(d), false);
        break;
    default: rc = ACGPU_E_UNSUPPORTED;
    }
    if (rc == ACGPU_OK && sh->d_result)
        HIP_TRY(launch_write_result(reinterpret_cast<acgpu_device_result *>(sh->d_result), r.h_slot[kSlotCount], stream));
    return rc;
}

// validates a shard and runs the pipeline of the automaton's family; caller holds d.mu.
int match_shard(acgpu_automaton *a, DeviceState &d, acgpu_shard *sh, int record_kind, void *d_out, uint64_t cap,
                uint64_t *n_out, hipStream_t stream, acgpu_profile *prof, bool readable) {
    int rc;
    if ((rc = check_shard(a, d, sh, record_kind, d_out, cap, stream))) return rc;
    *n_out = 0;
    if (prof) std::memset(prof, 0, sizeof(*prof));
    if ((rc = start_call(a, d, nullptr, sh, record_kind, d_out, cap, stream, prof != nullptr, readable))) return rc;
    return collect(a, d, &d.call, n_out, prof, nullptr);
}

// acgpu_match_device_begin on a given scratch pool (the caller holds d.mu and has made d's device current)
int begin_shard(acgpu_automaton *a, DeviceState &d, acgpu_shard *sh, int record_kind, void *d_out, uint64_t cap, hipStream_t stream,
                int want_profile, acgpu_ticket **ticket) {
    *ticket = nullptr;
    int rc;
    if ((rc = check_shard(a, d, sh, record_kind, d_out, cap, stream))) return rc;
    Ticket *tk = nullptr;
    for (auto &cand : d.tickets)
        if (!cand.busy) { tk = &cand; break; }
    if (!tk) return ACGPU_E_INVALID; // too many calls in flight: collect one first
    if ((rc = start_call(a, d, tk, sh, record_kind, d_out, cap, stream, want_profile != 0, false))) return rc;
    if (tk->rec.done) { // enqueued: in flight until _end or _abandon
        d.inflight++;
        d.inflight_stream = stream;
    }
    tk->busy = true;
    *ticket = reinterpret_cast<acgpu_ticket *>(tk);
    return ACGPU_OK;
}

int end_ticket(const acgpu_automaton *ca, acgpu_ticket *ticket, uint64_t *n_out, acgpu_profile *prof, bool *redone) {
    if (redone) *redone = false;
    if (!ca || !ticket || !n_out) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    Ticket *tk = reinterpret_cast<Ticket *>(ticket);
    DeviceState *d = reinterpret_cast<DeviceState *>(tk->owner); // (set when the pool was created)
    hipEvent_t done = nullptr;
    {
        std::lock_guard<std::mutex> lock(d->mu);
        if (!tk->busy) return ACGPU_E_INVALID;
        if (tk->rec.done) done = completion(tk->rec);
    }
    if (done) HIP_TRY(hipEventSynchronize(done)); // outside the lock: other calls may be enqueued meanwhile
    std::lock_guard<std::mutex> lock(d->mu);
    if (!tk->busy) return ACGPU_E_INVALID; // (collected by another thread meanwhile)
    tk->busy = false; // (whatever happens below, the ticket is collected)
    if (tk->rec.done) d->inflight--;
    return collect(a, *d, &tk->rec, n_out, prof, redone);
}

} // namespace acgpu

extern "C" {

int acgpu_match_device(const acgpu_automaton *ca, acgpu_shard *sh, int record_kind, void *d_out, uint64_t cap,
                       uint64_t *n_out, void *stream_, acgpu_profile *prof) {
    if (!ca || !sh || !n_out) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    PoolCall call(a);
    if (call.rc) return call.rc;
    return match_shard(a, *call.d, sh, record_kind, d_out, cap, n_out, reinterpret_cast<hipStream_t>(stream_), prof);
}

int acgpu_match_device_begin(const acgpu_automaton *ca, acgpu_shard *sh, int record_kind, void *d_out, uint64_t cap,
                             void *stream_, int want_profile, acgpu_ticket **ticket) {
    if (!ca || !sh || !ticket) return ACGPU_E_INVALID;
    *ticket = nullptr;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    PoolCall call(a);
    if (call.rc) return call.rc;
    return begin_shard(a, *call.d, sh, record_kind, d_out, cap, reinterpret_cast<hipStream_t>(stream_), want_profile, ticket);
}

int acgpu_match_device_abandon(const acgpu_automaton *ca, acgpu_ticket *ticket) {
    if (!ca || !ticket) return ACGPU_E_INVALID;
    Ticket *tk = reinterpret_cast<Ticket *>(ticket);
    DeviceState *own = reinterpret_cast<DeviceState *>(tk->owner); // (set when the pool was created)
    hipEvent_t done = nullptr;
    {
        std::lock_guard<std::mutex> lock(own->mu);
        if (!tk->busy) return ACGPU_E_INVALID;
        if (!tk->rec.done) { // (ran to its end inside _begin)
            tk->busy = false;
            return ACGPU_OK;
        }
        done = completion(tk->rec);
    }
    HIP_TRY(hipEventSynchronize(done)); // (its kernels still write the caller's buffers until then)
    std::lock_guard<std::mutex> lock(own->mu);
    if (!tk->busy) return ACGPU_E_INVALID;
    tk->busy = false;
    own->inflight--;
    return ACGPU_OK;
}

int acgpu_match_device_end(const acgpu_automaton *ca, acgpu_ticket *ticket, uint64_t *n_out, acgpu_profile *prof) {
    return end_ticket(ca, ticket, n_out, prof, nullptr);
}

} // extern "C"
