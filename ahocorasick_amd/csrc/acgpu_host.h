// acgpu_host.h -- host-side state shared by the units of the C ABI (acgpu_call.hip and the entries around it; acgpu_multi.hip):
// grow-only device buffers, tickets, the per-automaton per-device scratch pool, the automaton handle.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <set>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "acgpu_internal.h"
#include "acgpu_kernels.h"

namespace acgpu {

extern thread_local int g_last_hip_error;

#define HIP_TRY(expr)                                  \
    do {                                               \
        hipError_t _e = (expr);                        \
        if (_e != hipSuccess) {                        \
            g_last_hip_error = (int)_e;                \
            (void)hipGetLastError();                   \
            return _e == hipErrorOutOfMemory ? ACGPU_E_NOMEM : (_e == hipErrorNoDevice ? ACGPU_E_NODEVICE : ACGPU_E_HIP); \
        }                                              \
    } while (0)

// grow-only device buffer
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return ACGPU_OK;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        size_t want = need + need / 4 + 256;
        HIP_TRY(hipMalloc(&p, want));
        bytes = want;
        return ACGPU_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// A device buffer whose capacity is kept in records (the cursor's and the counting calls' reservoir): grow-only, and exactly
// what was asked for plus 64 bytes of slack -- the tunable "cursor_reservoir_bytes" bounds what the callers ask for.
// The capacity is in records of the kind it was last asked for (kind = the record's bytes): the pool's reservoir holds Map records
// for one call and Set records for the next (acgpu_spans.hip), and what is there is counted anew in the kind that is asked for.
struct Reservoir {
    void *p = nullptr;
    uint64_t recs = 0;
    uint64_t kind = 0; // bytes of the records `recs` counts
    int ensure(uint64_t need, uint64_t record_bytes) {
        if (kind && kind != record_bytes) recs = recs * kind / record_bytes;
        kind = record_bytes;
        if (need <= recs) return ACGPU_OK;
        release();
        HIP_TRY(hipMalloc(&p, need * record_bytes + 64));
        recs = need;
        return ACGPU_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        recs = 0;
    }
};

// What a scratch pool (DeviceState) owns: released when the pool dies, neither copied nor assigned.  DevBuf and Reservoir
// themselves stay plain -- StreamBufs is moved by member copy, g_timing is a global, locals release by hand.
template <class Buf>
struct Owned : Buf {
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { this->release(); }
};
using PoolBuf = Owned<DevBuf>;

// ... and its pinned blocks, events and streams: reads as the handle, the runtime creates it through &x.h.
template <class H, auto Free>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle &&o) noexcept : h(o.h) { o.h = nullptr; } // (no copies: a handle has one owner)
    ~Handle() { reset(); }
    void reset() {
        if (h) (void)Free(h);
        h = nullptr;
    }
    operator H() const { return h; }
};
template <class T = void>
using Pinned = Handle<T *, hipHostFree>;
using PoolEvent = Handle<hipEvent_t, hipEventDestroy>;
using PoolStream = Handle<hipStream_t, hipStreamDestroy>;

// How a call's result is collected (collect(), acgpu_call.hip): the pipeline that was enqueued.
enum class CallForm : uint8_t {
    Complete,      // the empty call: nothing found, nothing to report
    HostRun,       // ran to its end on the host (the families that need the host between their launches): count and chain exit in the slot
    States,        // k_ac_states + k_ac_states_out
    StatesCount,   // k_ac_states + k_states_hist: a counting call's direct form, no records (acgpu_count.hip)
    Ordered,       // a scan kernel and its ordering pass (k_permute, k_permute_wg, k_ww_compact), which reports into the slot
    FusedTail,     // the tile kernel or k_ww_pp with the fused tail: one kernel
    LongestBits,   // k_longest_bits
    LongestFollow, // k_longest_follow
    LongestWalk,   // the LONGEST walk pipeline
};

// The words of a record's pinned slot (CallRecord::h_slot), and the further words of the pool's own slot (DeviceState::h_counter)
// that a call borrows while it runs.
enum : int {
    kSlotCount = 0,     // records found
    kSlotFlag = 1,      // ALL: the overflow word; LONGEST: the bail flag
    kSlotExit = 2,      // the chain's exit
    kPoolChainHead = 3, // mark_chain: the chain head's index, behind it (kPoolChainHead + 1) the largest jump
    kPoolBound = 5,     // the multi-device driver: record_bound's index
};

// One call on a scratch pool: what enqueueing it decided and what completing it needs.  A ticket carries one; the pool owns one
// for its synchronous calls (DeviceState::call, on DeviceState::ev and h_counter).
struct CallRecord {
    acgpu_shard shard{};               // the shard as it was enqueued: a redo runs on this copy
    acgpu_shard *user_shard = nullptr; // the caller's: receives chain_exit
    int record_kind = 0;
    void *d_out = nullptr;
    uint64_t cap = 0;
    hipStream_t stream = nullptr;
    const PoolEvent *ev = nullptr;     // ev[0] .. ev[2]: the profile's events
    hipEvent_t done = nullptr;         // a ticket's completion marker; null: a synchronous call (or one that ran to its end inside _begin)
    bool done_is_ev2 = false;          // the completion to wait for is ev[2] (the call's last kernel's own end), not `done`
    bool one_kernel = false;           // the call was one kernel (the fused tail, a sequential kernel): ev[0] .. ev[2] is all of it, ev[1] is not recorded
    bool profiled = false;             // the events are recorded
    bool behind_pass = false;          // HostRun: ev[0] .. ev[1] is what ran behind the pass inside the call, accounted as finalizing
    acgpu_profile inside{};            // HostRun: the profile of a pass that ran inside the call on the pool's own record (run_inside)
    unsigned long long *h_slot = nullptr; // pinned, 64 bytes: kSlotCount, kSlotFlag, kSlotExit
    CallForm form = CallForm::Complete;
    int level = 0;                     // ALL: 1 = the redo's form (the fused kernel, one scratch slice); LONGEST: the run-up level
    bool folded = false;               // WHOLEWORD: the scan saw the folded tables (folded_tables, acgpu_tables.hip)
    bool counting = false;             // a shard call of acgpu_count_*: collect() hands its result to the pool's CountCall
    uint64_t scanned = 0;
    char kname[64] = {0};
};

// One asynchronous call in flight (acgpu_match_device_begin/_end): its own events and pinned count slot.
struct Ticket {
    PoolEvent ev[3];
    PoolEvent done;
    Pinned<unsigned long long> h_count; // 64 bytes
    bool busy = false;
    CallRecord rec;
    void *owner = nullptr; // the DeviceState it belongs to
};

// One acgpu_count_u16 / acgpu_count_device call (acgpu_count.hip), set in DeviceState::count while it runs: every shard call
// it makes is a counting call (CallRecord::counting) whose result collect() turns into counts -- the visit words of a direct
// piece, or the keyword_id column of the records in the call's reservoir -- instead of handing records on.
struct CountCall {
    unsigned long long *d_counts = nullptr; // device, n_counts words: added to
    uint32_t n_counts = 0;
    bool direct_ok = false;      // the visit words are there (and the tunable count_form allows the direct form)
    bool visits_zeroed = false;  // ... and zeroed on the call's stream (before the first direct piece)
    uint64_t through_reservoir = 0; // records counted in the records form
    acgpu_count_stats st{};
};

// The sizes of the pieces a text is scanned in when its records go through a reservoir of bounded size (the cursor, the counting
// calls): a ramp -- "cursor_first_piece", then four times the piece before, up to "cursor_max_piece" -- capped so that the records
// seen per unit so far fill at most half of the reservoir's budget.
struct PieceRamp {
    uint64_t piece = 0;                        // owned units of the next piece (before the density cap)
    uint64_t seen_records = 0, seen_units = 0; // what the pieces scanned so far yielded (the density estimate)
    void start();
    uint64_t next_size(uint64_t left, uint64_t budget_recs) const; // the next piece's owned units
    // records to have room for before a piece of `size` units is scanned (0: nothing is known yet)
    uint64_t predicted_room(uint64_t size, uint64_t budget_recs) const;
    // A piece of `size` units yielded cnt records, more than the reservoir held: *room = the records to make room for, and
    // `size` shrinks if even the budget does not hold them.  false: one unit's records do not fit the budget.
    bool on_overflow(uint64_t *size, uint64_t cnt, uint64_t budget_recs, uint64_t *room) const;
    void advance(uint64_t size, uint64_t cnt);
};
uint64_t reservoir_budget_bytes(); // tunable "cursor_reservoir_bytes"

struct DeviceState {
    std::mutex mu;   // one call at a time on this scratch pool (the automaton's own mutex only guards its map of these)
    int device = -1;
    int lane = 0;    // 0: what the single-device entries use; > 0: further shards of a multi-device call on the SAME device
    hipStream_t call_stream = nullptr; // the stream the host-haystack entries work on: the NULL stream for lane 0, lane_stream otherwise
    PoolStream lane_stream;            // (acgpu_match_u16_multi points call_stream at multi_stream for the duration of a call)
    int n_cu = 256;      // CUs the scan kernels size their grids for: n_cu_phys minus the tunable reserve_cus
    int n_cu_phys = 256; // multiProcessorCount of the device
    DevTables T{};
    const uint8_t *wflags_f = nullptr; // word-character tables of the loops that fold in every lookup (HostTables::wflags_f)
    const uint32_t *wbits_f = nullptr;
    int start_behind = -1; // set for the duration of a batch call: the separator unit (k_wwl_starts: a haystack's first unit is a walk start)
    std::vector<Handle<void *, hipFree>> table_allocs;
    // scratch pool (one in-flight match per automaton and device)
    PoolBuf counter, chunk_counts, offsets, scan_tmp, scratch, chain, lenbuf, statebuf;
    PoolBuf stage_hay, stage_out; // acgpu_match_u16 staging
    // the one-launch form for short haystacks (acgpu_small.hip): host-mapped pinned block [status | haystack | records], its stream
    Pinned<> small_pin;
    void *small_pin_dev = nullptr;
    PoolStream small_stream;
    PoolBuf multi_win, multi_tail; // multi-device calls, chain families: records of a repair window, the kept tail of the speculation
    // batch entry: pinned concatenation + offsets, device offsets, tagged records
    Pinned<> batch_pin;
    size_t batch_pin_bytes = 0;
    PoolBuf batch_off, batch_out;
    // pipelined host entry: pinned staging ring (one slot per chunk in flight), its copy stream, one event per chunk
    static constexpr int kPinSlots = 8;
    Pinned<> pin[kPinSlots];
    size_t pin_bytes = 0; // bytes per slot
    int pin_n = 0;        // slots allocated
    PoolStream multi_stream; // acgpu_match_u16_multi: this pool's stream for the duration of such a call (kept between calls)
    PoolStream copy_stream;
    std::vector<PoolEvent> chunk_ev;
    PoolBuf short_recs, short_nxt, short_tmp, short_mark; // SHORTEST: all-matches list + selection scratch
    PoolBuf ww_recs;                                      // WHOLEWORD: region-local record slots (TileLaunch::d_region_recs)
    PoolBuf blockmax;                                     // LONGEST: farthest landing per 64 positions
    PoolBuf lenbig, todo;                                 // LONGEST: escaped lengths; root-table form: flagged chunks
    PoolBuf chainbits;                                    // LONGEST: one bit per position, set where the chain reports a match
    PoolBuf bits_state;                                   // k_longest_bits: exit / flag / count, look-back words, region counter -- zero between calls
    PoolBuf visits, count_out;                            // acgpu_count_*: visit words (4 bytes per state of the compact automaton), the host entry's counts
    Owned<Reservoir> count_res;                           // ... and their reservoir of Map records (a replace call's too: acgpu_replace.hip)
    PoolBuf replace_tab, replace_plan, replace_slab;      // acgpu_replace_*: the replacement table, the plan {sums, output positions}, the host entry's two slabs
    Pinned<> replace_pin;                                 // ... 64 bytes: a piece's output length and last end
    PoolEvent replace_ev[4];                              // ... slab b emitted (b), slab b copied out (2 + b)
    PoolBuf replace_merged, replace_off;                  // acgpu_replace_batch_u16: a piece's records merged with its separators, the result's offsets (acgpu_replace_batch_utf8's and acgpu_cover_batch_u16's too)
    PoolBuf summary;                                      // acgpu_summary_batch_u16: 24 bytes per haystack, {records, the first of them}
    PoolBuf terms_entries, terms_stage, terms_aux, terms_count; // acgpu_count_batch_*: the call's entry list {h, id, count}, a piece's entries block by block, {block_base, n_distinct} per block, the running entry count (acgpu_terms.hip)
    PoolBuf spans_work, spans_carry, spans_out;        // acgpu_spans_*: {n_final, n_carry, bound} and the tiles' minima and counts, the two carry buffers, the host entry's final spans of a piece (acgpu_spans.hip)
    Pinned<> spans_pin;                                   // ... 64 bytes: a piece's {n_final, n_carry} and, for a cover call, the rest of the head (acgpu_spans.h)
    PoolBuf cover_spans, cover_tab, cover_plan;           // acgpu_cover_*: a piece's spans, the call's open and close elements, a DROP call's plan {sums, output positions} (acgpu_cover.hip)
    PoolBuf cover_items;                                  // acgpu_cover_batch_u16: a piece's final spans merged with its separators (its result's offsets: replace_off)
    PoolBuf utf8_in, utf8_aux;                          // the UTF-8 entries: the caller's bytes; {n_units, first_bad, tail, n_replaced}, block sums, checkpoints, a batch's byte offsets, a lossy text's start bitmap (Utf8Aux, acgpu_utf8.hip)
    PoolBuf utf8_voff;                                   // acgpu_spans_batch_utf8, acgpu_cover_batch_utf8: a batch's offsets in virtual coordinates (utf8_virtual_offsets)
    CountCall *count = nullptr;                          // the counting call that runs on this pool (it holds mu), or nullptr
    double all_density = -1.0;                           // ALL: records per unit of this pool's last call (-1: none yet): k_ac_states or the tile kernel
    int fol_level = 0;                                   // k_longest_follow: 0 = run-up of 128 positions, 1 = of a whole segment (a call's chains had not merged), 2 = not for this pool's texts
    void *bits_state_seen = nullptr;                     // (a re-allocated buffer, or a call that failed half way, is zeroed by a memset)
    PoolBuf cands, region_cands;                          // ALL, split form: candidate positions, {first, count} per region
    PoolBuf wwl_rs, wwl_mend, wwl_mid, wwl_sel, wwl_stop, wwl_nxt0; // WWLONGEST: walk starts, what each would report, where it stops
    Pinned<unsigned long long> h_counter;    // 64 bytes: the slot of the pool's own record, and the kPool words
    // match_all: two sets of slot counters alternate; the permute pass of a call zeroes the set the next call uses
    int cset = 0;
    bool cclean[2] = {false, false};
    void *counter_seen = nullptr; // (a re-allocated counter buffer is not clean)
    PoolEvent ev[4];
    CallRecord call; // the synchronous calls' record
    Ticket tickets[4];
    // stream rule (include/acgpu.h): while tickets are in flight every call on this automaton and device uses their stream
    int inflight = 0;
    hipStream_t inflight_stream = nullptr;
}; // (no destructor: every member releases itself -- acgpu_free has made the pool's device current)

} // namespace acgpu

namespace acgpu {
// what a pipelined stream (acgpu_stream.hip) works in: two chunks in pinned host memory and on the device, one scan's records on
// the device and in host-mapped pinned memory.  Pinning 30 MB takes longer than streaming 100 MB, and a stream is single-use:
// a closed stream leaves its buffers to the automaton, the next one on the same device takes them over.
struct StreamBufs {
    int device = -1;
    void *pin[2] = {nullptr, nullptr};
    size_t pin_bytes[2] = {0, 0};
    DevBuf dev[2];
    DevBuf out_dev;
    void *out_pin = nullptr, *out_pin_dev = nullptr;
    size_t out_pin_bytes = 0;
    hipStream_t copy_stream = nullptr;          // the chunk transfers' stream (creating one per stream object cost milliseconds)
    hipEvent_t arrived[2] = {nullptr, nullptr}; // chunk i has arrived on the device
    void release() { // (the caller has made `device` current)
        if (copy_stream) {
            (void)hipStreamSynchronize(copy_stream);
            (void)hipStreamDestroy(copy_stream);
            copy_stream = nullptr;
        }
        for (auto &e : arrived) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        for (int i = 0; i < 2; ++i) {
            if (pin[i]) (void)hipHostFree(pin[i]);
            pin[i] = nullptr;
            pin_bytes[i] = 0;
            dev[i].release();
        }
        out_dev.release();
        if (out_pin) (void)hipHostFree(out_pin);
        out_pin = out_pin_dev = nullptr;
        out_pin_bytes = 0;
    }
};
} // namespace acgpu

// what acgpu_free does with the streams and cursors still open on an automaton (open_streams, open_cursors below)
extern "C" void acgpu_stream_detach(acgpu_stream *s); // acgpu_stream.hip
extern "C" void acgpu_cursor_detach(acgpu_cursor *c); // acgpu_cursor.hip

struct acgpu_automaton {
    acgpu::HostTables t;
    std::vector<acgpu::StreamBufs> stream_cache;                                 // guarded by mu
    std::set<struct acgpu_stream *> open_streams;                                // guarded by mu: acgpu_free detaches them (acgpu_stream::a = nullptr)
    std::set<struct acgpu_cursor *> open_cursors;                                // guarded by mu: the same for cursors (acgpu_cursor.hip)
    std::mutex mu;                                                               // guards `dev`, `stream_cache` and `open_streams`
    std::map<std::pair<int, int>, std::unique_ptr<acgpu::DeviceState>> dev;      // (HIP device, lane) -> scratch pool + tables
    uint32_t n_given = 0;                                                        // keywords handed to acgpu_build (empty and duplicate ones included)
};

namespace acgpu {

// How a text is cut into shards for one call (shard_rule, acgpu_call.hip): the facts of the automaton's family that every host
// entry which scans a text piece by piece needs.
enum class Chain : uint8_t {
    None,     // ALL, WHOLEWORD: nothing passes from piece to piece
    Position, // LONGEST, WWLONGEST, the WholeWord walk: the position the scan goes on from, at least the piece's own_begin
    Restart,  // SHORTEST: where matching last restarted -- it passes through a piece that reports nothing
};

struct ShardRule {
    uint64_t left = 0, right = 0; // units of left context and of right halo a piece needs
    Chain chain = Chain::None;
    bool sequential = false;      // only the sequential kernel over the whole text exists
    bool all_pipeline = false;    // the ALL / WholeWord enqueued pipeline (enqueue_all; over the folded tables if not fold-consistent)
};

// readable: the call stands for match(Readable, ...) (acgpu_stream_feed)
ShardRule shard_rule(const HostTables &t, int record_kind, bool readable);
// The chain's entry into a piece, buffer relative: `chain` and `origin` (the buffer's first unit) in the caller's coordinates.
int64_t piece_entry(const ShardRule &r, int64_t chain, int64_t origin, uint64_t own_begin);
// The chain's exit from a piece that was entered at `entry`, buffer relative: sh = the shard as scanned, which reported n
// records; nullptr = nothing was scanned.
int64_t piece_exit(const ShardRule &r, int64_t entry, uint64_t own_end, const acgpu_shard *sh, uint64_t n);
// A host haystack is scanned as one piece: only the whole-text kernel exists, or the halos would not fit a host chunk.
bool one_piece(const ShardRule &r, const HostTables &t);
// ... what the host entries that scan piece by piece ask: the rule of the String loop
bool host_one_piece(const HostTables &t, int record_kind);

// The scratch pool of `a` on the CURRENT HIP device (created and the tables uploaded on first use).  lane > 0: a further,
// independent pool on the same device (its own stream), for multi-device calls that list a device more than once.
int device_for_call(acgpu_automaton *a, DeviceState **d, int lane = 0);

// The prologue of a call on the current device's pool: device_for_call, then d->mu for the call's lifetime.  rc != 0: no pool,
// nothing is locked.  The stream rule (include/acgpu.h) in its two forms, for the entry to apply where its checks have it.
struct PoolCall {
    DeviceState *d = nullptr;
    int rc;
    std::unique_lock<std::mutex> lock;
    explicit PoolCall(acgpu_automaton *a) : rc(device_for_call(a, &d)) {
        if (!rc) lock = std::unique_lock<std::mutex>(d->mu);
    }
    // a call that enqueues on `stream`: tickets in flight must be on that stream
    int on(hipStream_t stream) const { return d->inflight > 0 && stream != d->inflight_stream ? ACGPU_E_INVALID : ACGPU_OK; }
    // a call that uses the NULL stream or waits on the host: no ticket may be in flight
    int idle() const { return d->inflight > 0 ? ACGPU_E_INVALID : ACGPU_OK; }
    int fail(int code) const { // the call failed: nothing of it stays in flight
        (void)hipStreamSynchronize(d->call_stream);
        if (d->copy_stream) (void)hipStreamSynchronize(d->copy_stream);
        return code;
    }
};

// Validates a shard and runs the pipeline of the automaton's family on `stream`; the caller holds d.mu.
// readable: the call stands for match(Readable, ...) (acgpu_stream_feed).
int match_shard(acgpu_automaton *a, DeviceState &d, acgpu_shard *sh, int record_kind, void *d_out, uint64_t cap, uint64_t *n_out,
                hipStream_t stream, acgpu_profile *prof, bool readable = false);

// acgpu_match_device_begin on a given scratch pool: the caller holds d.mu and has made d's device current.  The ticket is
// collected with acgpu_match_device_end / _abandon (which take d.mu themselves).
int begin_shard(acgpu_automaton *a, DeviceState &d, acgpu_shard *sh, int record_kind, void *d_out, uint64_t cap, hipStream_t stream,
                int want_profile, acgpu_ticket **ticket);

// acgpu_match_device_end; *redone: the call had to be redone inside (a scratch slice had filled up) -- the records and the device
// result were written a second time, AFTER whatever the caller had enqueued behind the first attempt.
int end_ticket(const acgpu_automaton *a, acgpu_ticket *ticket, uint64_t *n_out, acgpu_profile *prof, bool *redone);

// acgpu_match_u16 on a long haystack, pipelined over chunks (acgpu_hosttext.hip): the units [lo, hi) of `haystack` become the
// device buffer d.stage_hay (buffer unit 0 = unit lo), the owned range [own_lo, own_hi) is scanned as shards of it on
// d.call_stream, the records (buffer relative) land in d.stage_out -- or in d_out, a device buffer of cap records, when it is
// given.  chain: in = entry, out = exit (buffer relative).
// own_done given -- a counting call's scan (d.count is set; acgpu_count.hip is the only such caller): every shard's records are consumed when it is collected, so each shard writes to the start of
// d_out; the scan stops at the first shard whose records do not fit -- *own_done = the buffer position up to which the owned
// units have been counted (own_hi - lo when all were), *n_out = that shard's records, *chain = the entry into it.
int scan_host_range(acgpu_automaton *a, DeviceState &d, const uint16_t *haystack, uint64_t n_units, uint64_t lo, uint64_t hi,
                    uint64_t own_lo, uint64_t own_hi, int record_kind, uint64_t cap, uint64_t *n_out, int64_t *chain,
                    void *d_out = nullptr, uint64_t *own_done = nullptr);

// The whole host text as one shard: copied (blocking) into d.stage_hay; *out = that buffer, all of it owned, the text's begin and
// end, no chain.  The caller holds d.mu.
int stage_whole_text(DeviceState &d, const uint16_t *haystack, uint64_t n_units, acgpu_shard *out);

// the shard is one whole text: all of it owned, the text's begin and end (what the device entries of spans, cover and replace serve)
inline bool shard_is_whole_text(const acgpu_shard &sh) {
    return sh.own_begin == 0 && sh.own_end == sh.n_units && sh.text_begin == 1 && sh.text_end == 1;
}

// What a UTF-8 entry does with ill-formed bytes: refuse the text (ACGPU_E_ENCODING), or scan every maximal ill-formed subpart as
// one U+FFFD, as bytes.decode("utf-8", "replace") does (the *_lossy entries).
enum class Utf8Errors { strict, replace };

// A UTF-8 host text staged as one shard (acgpu_utf8.hip): validated and transcoded on the device.
struct Utf8Text {
    acgpu_shard shard{};              // as stage_whole_text builds it: d.stage_hay, all of it owned, the text's begin and end, no chain
    const uint8_t *d_bytes = nullptr; // the bytes on the device (d.utf8_in)
    const uint32_t *d_ckpt = nullptr; // checkpoint table, one word per 32 units: the byte offset of the sequence that holds unit 32 i, bit 31
                                      // set where that unit is its low surrogate; nullptr: an all-ASCII text, unit offsets are byte offsets
    uint64_t n_units = 0;             // UTF-16 units of the text
    uint64_t n_bytes = 0;             // ... and its bytes (the open form: without the held prefix)
    uint32_t tail = 0;                // the open form: bytes at the buffer's end that begin a sequence the next buffer completes, 0..3
    int64_t first_bad = -1;           // ACGPU_E_ENCODING: where a strict decoder stops; lossy: -1, or the first replaced subpart's first byte
    bool lossy = false;               // staged with Utf8Errors::replace: the maps walk d_starts, not the bytes
    const uint32_t *d_starts = nullptr; // lossy, with d_ckpt: the start bitmap, a bit per byte set where a sequence or a subpart begins (d.utf8_aux)
    uint64_t n_replaced = 0;          // lossy: the U+FFFD units that stand for ill-formed subparts
};
// bytes -> {device shard, checkpoint table, n_units} on `stream`, which it waits for once (the transcoder's 16-byte result sizes
// the shard).  ACGPU_E_ENCODING: the text is ill-formed, out->first_bad says where, nothing was transcoded and the stream is
// idle.  The caller holds d.mu; n_bytes < 2^31.
// errors == replace: never ACGPU_E_ENCODING; out->n_replaced and out->first_bad say what was replaced.
int stage_utf8_text(DeviceState &d, const uint8_t *bytes, uint64_t n_bytes, hipStream_t stream, Utf8Text *out, Utf8Errors errors = Utf8Errors::strict);
// The same for a buffer that lies in two parts on the host, head | bytes (acgpu_stream_feed_utf8: the carried bytes and the
// caller's chunk; n_head + n_rest < 2^31, not 0), each copied from where it is.  open: the text goes on behind the buffer -- a
// sequence that the buffer's end cuts and that is well-formed so far is held back: out->tail bytes, and the shard, the
// checkpoints, n_units and n_bytes are those of the bytes before them (k_utf8_open_count).  open and replace
// (acgpu_stream_feed_utf8_lossy): held is a lead with what it has claimed so far, where that reaches the buffer's end
// (k_utf8_lossy_open_count); n_replaced and first_bad are those of the bytes before it, too.
int stage_utf8_parts(DeviceState &d, const uint8_t *head, uint64_t n_head, const uint8_t *bytes, uint64_t n_rest, bool open, hipStream_t stream,
                     Utf8Text *out, Utf8Errors errors = Utf8Errors::strict);
// A batch of UTF-8 haystacks staged as ONE shard (acgpu_utf8.hip): the caller's span copied once, every haystack validated on its
// own, and transcoded into the text a batch call scans -- the haystacks' units with the separator unit behind every haystack.
struct Utf8Batch {
    Utf8Text text;                       // shard: d.stage_hay, n_units + n_haystacks units, all owned; n_units: WITHOUT separators; d_ckpt:
                                         // indexed by the unit without separators (text unit - haystack), nullptr for an all-ASCII batch
    const uint32_t *d_boff = nullptr;    // n_haystacks + 1 byte offsets relative to the span's first byte (d.utf8_aux)
    const uint32_t *d_cat_off = nullptr; // n_haystacks + 1: the first unit of every haystack in the shard (d.batch_off), what k_batch_tag,
                                         // k_batch_summary and haystack_of take
    std::vector<uint32_t> h_boff;        // ... and on the host (what d_boff was uploaded from)
    uint32_t n_haystacks = 0;
    uint32_t bad_haystack = 0;           // ACGPU_E_ENCODING: the first ill-formed haystack; text.first_bad is relative to ITS first byte
                                         // (lossy: the haystack of the first replaced subpart, likewise)
};
// bytes[offsets[0] .. offsets[n]) -> Utf8Batch on `stream`, which it waits for once, as stage_utf8_text does.  offsets: checked
// (check_batch), the span not empty.  validate_only: no shard is built (the calls that go haystack by haystack stage every
// haystack with stage_utf8_text afterwards); out->text.n_units is set all the same.  ACGPU_E_ENCODING: nothing was transcoded
// and the stream is idle.  errors == replace: every haystack decoded on its own, never ACGPU_E_ENCODING.  The caller holds d.mu.
int stage_utf8_batch(DeviceState &d, const HostTables &t, const uint8_t *bytes, const uint64_t *offsets, uint32_t n, hipStream_t stream,
                     Utf8Batch *out, bool validate_only = false, Utf8Errors errors = Utf8Errors::strict);
// cnt records of the scan over b's shard in d_recs -> records tagged with their haystack in d_out, positions in bytes relative to
// the haystack (k_utf8_batch_tag; an all-ASCII batch: k_batch_tag, there a relative unit is a relative byte)
int utf8_batch_tag(const Utf8Batch &b, const void *d_recs, uint64_t cnt, int record_kind, void *d_out, hipStream_t stream);
// cnt records of `cols` words of the scan over text's shard, in place in d_recs, enqueued on `stream` (k_utf8_batch_map): start ->
// the first byte of the code point that holds unit start, end -> one past the last byte of the one that holds unit end - 1.
// b == nullptr: the shard is the text's own units, bytes of the text; an all-ASCII text (no checkpoints) needs no map, nothing is
// launched.  b given (text is b->text): units of the batch's shard -> bytes relative to the SPAN; an all-ASCII batch is mapped
// too, a record of haystack h stands h separators behind its byte.
int utf8_map_records(const Utf8Text &text, const Utf8Batch *b, int32_t *d_recs, uint64_t cnt, uint32_t cols, hipStream_t stream);
// *d_out = the byte for unit `unit` of the shard, enqueued on `stream` (k_utf8_batch_pos).  b == nullptr: the first byte of the
// code point that holds unit `unit` < n_units -- a position between the two units of a surrogate pair is rounded DOWN; not for
// an all-ASCII text (there the unit is the byte).  A lossy text: the first byte of the START that holds the unit -- a replaced
// subpart is one unit, so it is never entered, and only a surrogate pair rounds down; not for a text without checkpoints.  b given: a byte of the span -- a separator, the last one included, maps to the
// byte where the next haystack begins (n_bytes behind the last), as does a unit at or behind the shard's end; any other unit as
// above.
int utf8_map_position(const Utf8Text &text, const Utf8Batch *b, uint64_t unit, int64_t *d_out, hipStream_t stream);
// A batch in VIRTUAL COORDINATES (acgpu_spans_batch_utf8, acgpu_cover_batch_utf8): v = (byte of the span) + (index of the
// haystack), the caller's bytes with one phantom element behind every haystack; n_bytes + n_haystacks elements in all.
// voff[j] = boff[j] + j, n_haystacks + 1 words: on the host from b.h_boff, on the device (d.utf8_voff, enqueued) from b.d_boff.
int utf8_virtual_offsets(DeviceState &d, const Utf8Batch &b, hipStream_t stream, std::vector<uint32_t> *h_voff, const uint32_t **d_voff);
// cnt Set records of the scan over b's shard, in place in d_recs, enqueued (k_utf8_batch_vmap): units of the shard -> v.  An
// all-ASCII batch needs no map: there a unit of the shard is its v.
int utf8_vmap_records(const Utf8Batch &b, int32_t *d_recs, uint64_t cnt, hipStream_t stream);
// *d_out = a v that no record starting at or behind unit `unit` of b's shard starts before, enqueued (k_utf8_batch_vpos): a
// separator maps to its phantom, a unit at or behind the shard's end to the text's end; not for an all-ASCII batch (the unit itself).
int utf8_vmap_position(const Utf8Batch &b, uint64_t unit, int64_t *d_out, hipStream_t stream);
// The first records of n_entries summaries from units to bytes (k_summary_utf8_bytes): b given, the entries of b's haystacks;
// else the entries -- one -- of `text` scanned as a text of its own.  Nothing is launched where there are no checkpoints.
int utf8_summary_bytes(const Utf8Batch *b, const Utf8Text &text, acgpu_batch_summary *d_sum, uint32_t n_entries, hipStream_t stream);

// The stats of the UTF-8 entries.  No argument: the preset, what an entry writes before it touches a device.  With the staged
// text and the front end's rc: ACGPU_E_ENCODING -> where the decoder stops, no units, not ASCII; any other rc -> what was decoded.
inline acgpu_utf8_stats utf8_stats(const Utf8Text *text = nullptr, int rc = ACGPU_OK) {
    acgpu_utf8_stats st{};
    st.first_bad = text ? text->first_bad : -1;
    st.n_units = text && rc != ACGPU_E_ENCODING ? text->n_units : 0;
    st.ascii = text ? rc != ACGPU_E_ENCODING && text->n_units == text->n_bytes : 1;
    return st;
}
inline acgpu_utf8_batch_stats utf8_batch_stats(const Utf8Batch *b = nullptr, int rc = ACGPU_OK) {
    acgpu_utf8_batch_stats st{};
    const bool bad = b && rc == ACGPU_E_ENCODING;
    st.first_bad = bad ? b->text.first_bad : -1;
    st.bad_haystack = bad ? b->bad_haystack : 0;
    st.n_units = b && !bad ? b->text.n_units : 0;
    st.ascii = b ? !bad && b->text.n_units == b->text.n_bytes : 1;
    return st;
}

inline acgpu_utf8_lossy_stats utf8_lossy_stats(const Utf8Text *text = nullptr, uint32_t first_haystack = 0) {
    acgpu_utf8_lossy_stats st{};
    st.n_units = text ? text->n_units : 0;
    st.n_replaced = text ? text->n_replaced : 0;
    st.first_replaced = text ? text->first_bad : -1;
    st.first_haystack = first_haystack;
    st.ascii = text ? text->n_units == text->n_bytes && !text->n_replaced : 1;
    return st;
}

// The policy of an entry's body: how its texts are staged and what its stats argument is.  One body serves the strict entry and
// the lossy one (acgpu_utf8.hip, acgpu_summary.hip, acgpu_replace.hip).
struct Utf8StrictText {
    using Stats = acgpu_utf8_stats;
    static constexpr Utf8Errors errors = Utf8Errors::strict;
    static Stats stats(const Utf8Text *text = nullptr, int rc = ACGPU_OK) { return utf8_stats(text, rc); }
};
struct Utf8LossyText {
    using Stats = acgpu_utf8_lossy_stats;
    static constexpr Utf8Errors errors = Utf8Errors::replace;
    static Stats stats(const Utf8Text *text = nullptr, int = ACGPU_OK) { return utf8_lossy_stats(text); }
};
struct Utf8StrictBatch {
    using Stats = acgpu_utf8_batch_stats;
    static constexpr Utf8Errors errors = Utf8Errors::strict;
    static Stats stats(const Utf8Batch *b = nullptr, int rc = ACGPU_OK) { return utf8_batch_stats(b, rc); }
};
struct Utf8LossyBatch {
    using Stats = acgpu_utf8_lossy_stats;
    static constexpr Utf8Errors errors = Utf8Errors::replace;
    static Stats stats(const Utf8Batch *b = nullptr, int = ACGPU_OK) { return utf8_lossy_stats(b ? &b->text : nullptr, b ? b->bad_haystack : 0); }
};

// acgpu_replace_batch_utf8, behind a piece that emits the span's bytes [done, limit): the haystack boundaries whose output offset
// that piece writes are [*j0, *j1) of boff (n_hay + 1 ascending byte offsets, boff[n_hay] = the span's bytes) -- those with
// done <= boff[j] < limit, and behind the LAST piece (limit = the span's end) those at the end as well.  The pieces' [done, limit)
// tile the span, so every boundary is taken by exactly one piece; a run of empty haystacks is a run of equal offsets, taken whole.
inline void span_boundaries(const uint32_t *boff, uint32_t n_hay, uint64_t done, uint64_t limit, bool last, uint32_t *j0, uint32_t *j1) {
    const uint32_t *end = boff + n_hay + 1;
    auto below = [](uint32_t b, uint64_t x) { return (uint64_t)b < x; };
    *j0 = (uint32_t)(std::lower_bound(boff, end, done, below) - boff);
    *j1 = last ? n_hay + 1 : std::max(*j0, (uint32_t)(std::lower_bound(boff, end, limit, below) - boff));
}

// For as long as a batch's text is scanned: d.start_behind is the separator unit (WholeWordLongest: every haystack's first unit
// is a walk start).  BatchText does the same for the texts it stages.  The caller holds d.mu.
struct SeparatorScan {
    DeviceState &d;
    SeparatorScan(DeviceState &d_, const HostTables &t) : d(d_) { d.start_behind = t.sep_unit; }
    SeparatorScan(const SeparatorScan &) = delete;
    ~SeparatorScan() { d.start_behind = -1; }
};

// acgpu_match_u16 behind its argument checks; the caller holds d.mu (acgpu_match_batch_u16 calls it per haystack).
int match_host_text(acgpu_automaton *a, DeviceState &d, const uint16_t *haystack, uint64_t n_units, int record_kind, void *out,
                    uint64_t cap, uint64_t *n_out);

// What the batch entries check before they touch a device (check_batch, acgpu_batch.hip).
struct BatchPlan {
    uint64_t total = 0, cat = 0; // units of all haystacks; of their concatenation, a separator behind every haystack
    bool per_haystack = false; // they cannot be concatenated: every haystack is scanned as a text of its own
};
int check_batch(const HostTables &t, const uint16_t *units, const uint64_t *offsets, uint32_t n_haystacks, BatchPlan *plan);

// The front of the UTF-8 batch entries of spans, cover and replace, behind their checks, preset outputs and PoolCall; P =
// Utf8StrictBatch or Utf8LossyBatch.  The stream rule (idle: the NULL stream), then the whole batch is staged -- validated
// whichever way it is scanned (plan.per_haystack: validated only), so that what is refused does not depend on the route -- and
// *ust says what was decoded.  ACGPU_OK: go on.  Any other code is the entry's to return as it is: ACGPU_E_ENCODING (and the stream
// rule's ACGPU_E_INVALID) with the stream idle and the pool as usable as before the call; the rest behind call.fail.
// (The summary, count-batch and match entries could follow; what they write on an encoding error differs in ways that tests pin.)
template <class P>
int utf8_batch_front(const PoolCall &call, const HostTables &t, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks, const BatchPlan &plan,
                     Utf8Batch *b, typename P::Stats *ust) {
    int rc = call.idle();
    if (rc) return rc;
    rc = stage_utf8_batch(*call.d, t, bytes, offsets, n_haystacks, call.d->call_stream, b, plan.per_haystack, P::errors);
    if (rc && rc != ACGPU_E_ENCODING) return call.fail(rc);
    if (ust) *ust = P::stats(b, rc);
    return rc;
}

// ... and the route haystack by haystack of those entries: every non-empty haystack staged as a text of its own on `stream`
// (never ill-formed: the front has validated it) and handed to text(i, staged); after(i) behind every haystack, the empty ones too.
// Whether the stream is waited for before the next haystack is staged over this one is text's business.
template <class P, class Text, class After>
int utf8_each_haystack(DeviceState &d, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks, hipStream_t stream, Text text, After after) {
    for (uint32_t i = 0; i < n_haystacks; i++) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        if (len) {
            Utf8Text staged;
            int rc = stage_utf8_text(d, bytes + offsets[i], len, stream, &staged, P::errors);
            if (rc) return rc == ACGPU_E_ENCODING ? ACGPU_E_HIP : rc;
            if ((rc = text(i, staged))) return rc;
        }
        after(i);
    }
    return ACGPU_OK;
}

// The haystacks of a batch call staged as ONE text, for as long as the call scans it: the text and its offsets in d.batch_pin
// (h_off[i] = the first unit of haystack i, separator i stands at h_off[i + 1] - 1; n_haystacks + 1 words), the offsets in
// d.batch_off as well, and d.start_behind set to the separator.  The caller holds d.mu.
struct BatchText {
    DeviceState &d;
    const uint16_t sep;
    uint16_t *h_cat = nullptr;
    uint32_t *h_off = nullptr;
    uint64_t cat = 0;
    uint32_t n_haystacks = 0;
    // (WholeWordLongest: every haystack's first unit is a walk start, also where a piece's left halo is the separator)
    BatchText(DeviceState &d_, const HostTables &t) : d(d_), sep((uint16_t)t.sep_unit) { d.start_behind = t.sep_unit; }
    BatchText(const BatchText &) = delete;
    ~BatchText() { d.start_behind = -1; }
    const uint32_t *d_off() const { return reinterpret_cast<const uint32_t *>(d.batch_off.p); }
    // concatenates, and uploads the offsets on `stream` (asynchronously: the scan follows on it)
    int stage(const uint16_t *units, const uint64_t *offsets, uint32_t n, hipStream_t stream);
};

// A text on its way through a reservoir, piece by piece (scan_next_piece, acgpu_pieces.hip).  Six consumers: the cursor keeps
// one from page call to page call; a counting, a replace, a batch summary, a count-batch and a spans call have one for each text
// they drive -- a spans call being every call through spans_pieces (acgpu_spans.h): the spans and the cover entries, their batch
// entries over the concatenation, and, haystack by haystack, a batch that cannot be concatenated.
struct PieceDriver {
    uint64_t pos = 0, end = 0;         // the owned units [pos, end) have not been scanned yet
    int64_t chain = 0;                 // the chain's entry into the next piece (the text's coordinates)
    bool whole = false;                // the text is scanned as ONE piece (one_piece, or a sequential rule)
    int record_kind = 0;
    PieceRamp ramp;                    // the sizes of the pieces
    Reservoir *res = nullptr;          // where a piece's records go
    const uint64_t *through = nullptr; // a counting call: CountCall::through_reservoir (its shards' records are counted as they are collected)
    uint64_t pieces = 0, rescans = 0;  // scan attempts; of those, attempts whose records did not fit
    uint64_t units_scanned = 0, scan_end = 0; // owned units scanned, rescans included; the host text's units [0, scan_end) have been scanned
    PieceDriver() = default;
    PieceDriver(uint64_t pos_, uint64_t end_, int64_t chain_, bool whole_, int record_kind_, Reservoir *res_, const uint64_t *through_ = nullptr)
        : pos(pos_), end(end_), chain(chain_), whole(whole_), record_kind(record_kind_), res(res_), through(through_) { ramp.start(); }
};

// The scan of one piece.  Exactly three kinds: a caller's device shard with a moving owned range (`shard`, on `stream`); else a
// host text (hay, n) -- whole as one staged shard (stage_whole_text + match_shard), or a range of it through scan_host_range.
struct PieceScan {
    acgpu_automaton *a;
    DeviceState &d;
    const uint16_t *hay;
    uint64_t n;
    const acgpu_shard *shard;
    hipStream_t stream;
    bool readable = false; // a shard scanned as match(Readable, ...) scans it (shard_rule, match_shard): a stream's buffer
    int operator()(PieceDriver &p, uint64_t size, uint64_t *cnt, uint64_t *done, uint64_t *base) const;
};

// Scans the next piece to its completion: sizes it, makes room, scans, and on overflow scans again -- in a larger reservoir, as a
// smaller piece, or not at all (ACGPU_E_NOMEM: one unit's records do not fit the budget; a whole text instead grows the reservoir
// to the exact count, past the budget).  *n_out = the piece's records, *base = the text position of their buffer's unit 0.
int scan_next_piece(PieceDriver &p, const PieceScan &scan, uint64_t *n_out, uint64_t *base);

// ---- a replace stream's feed (acgpu_replace.hip, for acgpu_stream.hip) ----
// check_table of the replace entries: ACGPU_E_INVALID for a bad table, ACGPU_E_UNSUPPORTED for ACGPU_MODE_ALL; no device.
int replace_check_table(const acgpu_automaton *a, const void *repl, const uint64_t *repl_off, uint32_t n_repl);
// The buffer [carry | chunk] of one feed, on the device.  Positions are buffer relative; done counts ELEMENTS -- units, or
// bytes of u8 -- and chain units.
struct ReplaceFeed {
    acgpu_shard shard{};         // the buffer's units with the feed's owned range, text_begin and text_end set
    const Utf8Text *u8 = nullptr; // a stream of bytes: the staged buffer `shard` is the units of
    bool final = false;          // the buffer's end is the text's end
    uint64_t done = 0;           // in: output exists for the elements in front of it; out: the same behind this feed
    int64_t chain = 0;           // in: the chain's entry; out: its exit
    acgpu_replace_stats st{};    // out: this feed alone
};
// Rewrites [f->done, new done) of the buffer into out (host, cap elements) through the pieces of the replace entries, scanned by
// the Readable rule.  ACGPU_E_OVERFLOW: *n_out and f->st are exact, nothing at or beyond out[cap] was written.  The caller holds
// d.mu, no ticket is in flight, and on an error it waits for the streams (PoolCall::fail).
int replace_feed(acgpu_automaton *a, DeviceState &d, ReplaceFeed *f, const void *repl, const uint64_t *repl_off, uint32_t n_repl, void *out,
                 uint64_t cap, uint64_t *n_out);

// ---- a cover stream's feed (acgpu_cover.hip, for acgpu_stream.hip) ----
// check_spec of the cover entries (esz: bytes of an element): ACGPU_E_INVALID for a bad spec; no device.
int cover_check_spec(const acgpu_cover_spec *spec, uint32_t esz);
// The buffer [carry | chunk] of one feed, on the device.  done counts ELEMENTS of the buffer -- units, or bytes of u8 -- and chain
// units; the carried spans are GLOBAL, in elements since the first feed: `origin` is the global position of the buffer's element 0.
struct CoverFeed {
    acgpu_shard shard{};           // the buffer's units with the feed's owned range, text_begin and text_end set
    const Utf8Text *u8 = nullptr;  // a stream of bytes: the staged buffer `shard` is the units of
    bool final = false;            // the buffer's end is the text's end
    uint64_t done = 0;             // in: output exists for the elements in front of it; out: the same behind this feed
    bool in_span = false;          // in / out: element done - 1 is covered by a span whose close has not been delivered
    uint64_t origin = 0;
    std::vector<int64_t> carried;  // in / out: {start, end} of the spans the merge withheld, ascending (at most max_len / 2 + 2)
    int64_t chain = 0;             // in: the chain's entry; out: its exit
    acgpu_cover_stats st{};        // out: this feed alone
};
// Rewrites [f->done, new done) of the buffer into out (host, cap elements) through the pieces of the cover entries over the owned
// range, scanned by the Readable rule.  ACGPU_E_OVERFLOW: *n_out and f->st are exact, nothing at or beyond out[cap] was written.
// The caller holds d.mu, no ticket is in flight, and on an error it waits for the streams (PoolCall::fail).
int cover_feed(acgpu_automaton *a, DeviceState &d, CoverFeed *f, const acgpu_cover_spec *spec, void *out, uint64_t cap, uint64_t *n_out);

// collect() of a counting shard call that found n records: counts them (acgpu_count.hip).  ACGPU_E_OVERFLOW: they did not fit
// the reservoir, nothing was counted.
int count_collected(DeviceState &d, const CallRecord &r, uint64_t n);

} // namespace acgpu
