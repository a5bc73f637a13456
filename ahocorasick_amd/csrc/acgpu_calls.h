// acgpu_calls.h -- what the units behind a shard call ask of one another: the tables as a call sees them (acgpu_tables.hip), the
// call record's steps (acgpu_call.hip), the planners (acgpu_all.hip, acgpu_longest_calls.hip), the host-run families
// (acgpu_hostrun.hip), and the prefix sum's scratch.  Everything else of those units is local to its file.
#pragma once
#include "acgpu_host.h"

namespace acgpu {
// (these were local to one file while the units were one: they stay out of the library's dynamic symbols)
#pragma GCC visibility push(hidden)

// ---- the prefix sum's scratch (launch_exclusive_scan, launch_scan_tile_offsets: acgpu_kernels.hip) ----
// d.scan_tmp for n elements: a word per tile of scan_tile_elems() elements, the grand total behind them
inline int ensure_scan_tmp(DeviceState &d, size_t n) { return d.scan_tmp.ensure((n / scan_tile_elems() + 2) * 8); }
// ... and with it the n counts the sum runs over and their offsets
inline int ensure_scan_buffers(DeviceState &d, size_t n) {
    int rc;
    if ((rc = d.chunk_counts.ensure(n * 4))) return rc;
    if ((rc = d.offsets.ensure(n * 8))) return rc;
    return ensure_scan_tmp(d, n);
}
// where the prefix sum over n elements has left their grand total
inline const uint64_t *scan_total(const DeviceState &d, uint32_t n) { return (const uint64_t *)d.scan_tmp.p + scan_tiles_for(n); }

// ---- acgpu_tables.hip ----
// the leading states of the dense table that the tunable lds_table_bytes lets k_ac_dfa keep in LDS
uint32_t lds_states_for(const HostTables &t);
// The device tables as a scan that folds in EVERY lookup sees them (word-character tables that are not fold-consistent):
// w'[c] = word[lower[c]] in place of both word-character tables.
DevTables folded_tables(const DeviceState &d);

// ---- acgpu_call.hip ----
using EnqueueFn = int (*)(acgpu_automaton *, DeviceState &, CallRecord &, int);
// the device address of the record's pinned slot
int slot_on_device(const CallRecord &r, unsigned long long **d_slot);
// The end of an enqueue: the form, what the profile reports, and a ticket's completion marker -- unless the call's last kernel
// delivers its own end to ev[2] (done_is_ev2: no marker packet behind the call).
int close_call(CallRecord &r, CallForm form, const char *kname, uint64_t scanned, bool done_is_ev2 = false);
// A call with nothing to scan: the device result says so, the slot is written here (no kernel will write it).
int enqueue_empty(CallRecord &r, int64_t chain_exit);
// The end of a call that ran on the host: the count and the chain exit from their device words into the record's slot (no
// d_exit: the pipeline has put the exit there), and the wait.
int close_host_run(CallRecord &r, const void *d_count, const void *d_exit, const char *kname, uint64_t scanned);
// This call keeps words of its own (an exit position, a count, mark_chain's head and largest jump) in the first 64 bytes of
// d.counter -- the first slot-counter line of enqueue_all's first set (word 0 = slot counter, word 1 = workgroup sum, the rest
// of the 128-byte line is padding): the next ALL call must clear that set itself.  clear: the words are zeroed on the stream.
int borrow_counter_line(DeviceState &d, hipStream_t stream, bool clear);
// A pass that a host-run call runs inside itself: a synchronous call of an enqueued pipeline on the pool's own record (events
// d.ev, slot d.h_counter), enqueued and collected -- that record may be `r`, so r is put back afterwards, with the pass's profile
// in r.inside.
int run_inside(EnqueueFn enqueue, acgpu_automaton *a, DeviceState &d, CallRecord &r, acgpu_shard *sh, int record_kind, void *d_out,
               uint64_t cap, uint64_t *n_out);
// A host-run call whose pass inside was the whole call: what that pass found, and the chain's exit.
int close_as_inside(CallRecord &r, uint64_t n, int64_t chain_exit);
// Completes the call in *r, for every family: the wait (a synchronous call's; end_ticket waits for a ticket's outside the pool's
// lock; a host-run call has waited itself), the redo if the kernels ask for one -- a synchronous call on the pool's own record --,
// then the count, the chain exit, what the pool learns (the ALL density), the profile and the overflow status.  The caller
// holds d.mu.
int collect(acgpu_automaton *a, DeviceState &d, CallRecord *r, uint64_t *n_out, acgpu_profile *prof, bool *redone);

// ---- acgpu_all.hip ----
// Which ALL-mode kernel serves this dictionary: the position-parallel K-gram tile kernel when the suffix filter
// exists and is selective, otherwise the general DFA chunk scan (any alphabet, any keyword lengths).
// force_kernel: 0 = automatic, 1 = DFA chunk scan, 2 = fused tile kernel, 3 = split tile kernels (filter + verification)
// The tile kernel serves every dictionary that has a suffix filter: measured on 0.5 GiB it beats the DFA chunk scan
// 3x even when the filter passes every position (10 k keywords: 0.22 ms; 100 k keywords, density 0.20: 0.72 against
// 1.78 ms; 300 k, density 0.48: 1.6 against 4.4 ms; 200 two-to-four-unit keywords over {a,b,c,d}, density 1.0: 25
// against 76 ms, both bound by emitting 647 M records).
bool use_tile_kernel(const HostTables &t);
// ALL-mode pipeline on one shard (and WHOLEWORD over fold-consistent tables, or folded ones: r.folded): the empty call, the
// states form, or a scan form (WholeWord tile kernels, the AhoCorasick tile kernel, the DFA chunk scan) and the ordering stage.
// level 1: the redo after an overflow of the split form's candidate slices or of a scratch slice -- the fused kernel, one
// scratch slice.
int enqueue_all(acgpu_automaton *a, DeviceState &d, CallRecord &r, int level);

// ---- acgpu_longest_calls.hip ----
// A LONGEST shard's own checks (the right halo, a chain entry inside the owned range or behind it); presets sh->chain_exit.
int check_longest_shard(const HostTables &t, acgpu_shard *sh);
// LONGEST takes the all-matches pipeline only when matches are expected to be sparse
bool filter_is_selective(const HostTables &t);
// LONGEST-mode pipeline on one shard: the checks, the chain's preset exit, the empty call; then the form of this run-up level
// (bits_level 0: short, 1: a whole segment, 2: the walk pipeline).  The sparse form of a selective suffix filter runs before
// this, on the host (start_call).  Tunable longest_form, bits: 1 = never k_longest_bits, 2 = never k_longest_follow,
// 4 = also for short texts (tests), 8 = k_longest_follow where the walk pipeline has its root table too.
int enqueue_longest(acgpu_automaton *a, DeviceState &d, CallRecord &r, int bits_level);

// ---- acgpu_hostrun.hip ----
// SHORTEST-mode pipeline on one shard: the restart position that came in restricts where the first match may start.
int run_shortest(acgpu_automaton *a, DeviceState &d, CallRecord &r);
// LONGEST over a dictionary whose suffix filter is selective: matches are sparse, so leftmost-longest is a selection over the
// all-matches list instead of a trie walk from every position.  Returns ACGPU_E_UNSUPPORTED when the haystack turns out to be
// dense in matches (the caller then takes the walk).
int run_longest_sparse(acgpu_automaton *a, DeviceState &d, CallRecord &r);
// WHOLEWORD with a word-character table that is not fold-consistent: the reference's mixed folded/raw lookups make
// token boundaries history dependent -- whole text, one lane (k_ww_sequential).  (Fold-consistent tables: enqueue_all.)
int run_wholeword_sequential(acgpu_automaton *, DeviceState &d, CallRecord &r);
// WholeWordLongestMatchSet.match(String) with a word-character table that is not fold-consistent: the reference mixes folded
// and raw lookups (S/WholeWordLongestMatchSet.java:126 against :151,:156), which makes token boundaries history dependent --
// whole text, one lane (k_wwl_sequential).
int run_wwlongest_sequential(acgpu_automaton *a, DeviceState &d, CallRecord &r);
// WWLONGEST-mode pipeline on one shard.  A walk belongs to the shard that owns its first unit; the scan visits the first walk
// start at or after chain_entry and leaves chain_exit = the position behind the stop of its last visited walk.
// T: the device tables the scan sees (d.T, or folded_tables(d) for the loops that fold in every lookup).
// plain_words: the walk reports only a whole path that is a keyword and ends at a word boundary -- no carried fail match --
// and does without the first-word table: WholeWordMatchMap's loop (S/WholeWordMatchMap.java:55-153), which is this walk
// without fail matches, over a WHOLEWORD automaton whose folded keywords hold non-word units (HostTables::fold_clean).
int run_wwlongest(acgpu_automaton *a, DeviceState &d, CallRecord &r, const DevTables &T, bool plain_words);

#pragma GCC visibility pop

// what the tunables decide per call: the LDS residency of the DFA rows, and the CUs the scan kernels size their grids for --
// "reserve_cus" leaves that many CUs without a scan workgroup (the scans hold a whole CU's LDS per workgroup, so a grid of
// n_cu - k workgroups keeps k CUs free: room for the workgroups of a collective that runs under the scan)
void refresh_call_state(acgpu_automaton *a, DeviceState &d); // acgpu_tables.hip

} // namespace acgpu
