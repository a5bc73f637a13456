// acgpu_longest_calls.hip -- the LONGEST planners: k_longest_bits, k_longest_follow and the walk pipeline as enqueued calls, the
// chain stage they share, and the choice among them by run-up level.
#include <algorithm>
#include <cstdio>

#include "acgpu_calls.h"

using namespace acgpu;

namespace {

// A two-letter alphabet in which every letter is a keyword: the text as one bit per unit, the chain's own positions only
// (k_longest_bits, acgpu_longest_bits.hip) -- no length array, no synchronisation pass; Map records look their keyword ids up
// by the matched text's own bits when they are written (keywords of up to 32 units; the rare longer ones by a walk).  The kernel checks
// its own result (every segment's exit against the next one's entry) and raises the bail flag -- also for a unit outside
// the alphabet --: collect() then redoes the call once more with a run-up of a whole segment (level 1), or by the walk pipeline
// (level 2).
int enqueue_longest_bits(acgpu_automaton *a, DeviceState &d, CallRecord &r, uint64_t entry, int bits_level) {
    const HostTables &t = a->t;
    const acgpu_shard *sh = &r.shard;
    const hipStream_t stream = r.stream;
    int rc;
    LongestBitsLaunch Bl{};
    Bl.d_hay = sh->d_hay;
    Bl.n_units = (uint32_t)sh->n_units;
    Bl.own_end = (uint32_t)sh->own_end;
    Bl.entry = (uint32_t)entry;
    Bl.g0 = (uint32_t)entry & ~127u; // (bitmap words in groups of four: 16-byte stores)
    const uint32_t region_units = longest_bits_region_units();
    Bl.n_regions = (uint32_t)((sh->own_end - Bl.g0 + region_units - 1) / region_units);
    Bl.runup = bits_level == 0 ? longest_bits_seg_units() / 2 : longest_bits_seg_units();
    Bl.max_len = t.max_len;
    Bl.d_out = r.d_out;
    Bl.cap = r.cap;
    const size_t n_blk = ((size_t)Bl.n_regions + 63) / 64, state_words = 8 + (size_t)Bl.n_regions + n_blk + 2;
    // exit / flag / count, a word per region, a word per block of 64 regions, the region counter: zero at the start of a call --
    // the call's last kernel leaves them so; a memset only for a fresh (or larger) buffer and after a call that failed half way
    const size_t state_had = d.bits_state.bytes;
    if ((rc = d.bits_state.ensure(state_words * 8))) return rc;
    if (d.bits_state.p != d.bits_state_seen || d.bits_state.bytes != state_had) {
        HIP_TRY(hipMemsetAsync(d.bits_state.p, 0, d.bits_state.bytes, stream));
        d.bits_state_seen = d.bits_state.p;
    }
    if ((rc = d.blockmax.ensure((size_t)Bl.n_regions * 8 + 64))) return rc;
    if ((rc = d.chainbits.ensure((size_t)Bl.n_regions * longest_bits_region_scratch_bytes() + 64))) return rc;
    Bl.d_exit = (unsigned long long *)d.bits_state.p;
    Bl.d_agg = Bl.d_exit + 8;
    Bl.d_blk = Bl.d_agg + Bl.n_regions;
    Bl.d_next = (uint32_t *)(Bl.d_blk + n_blk);
    Bl.d_marks = (uint32_t *)d.chainbits.p;
    Bl.d_xout = Bl.d_marks + (size_t)Bl.n_regions * (region_units / 32);
    Bl.d_text = nullptr;
    if (r.record_kind == ACGPU_REC_MAP) { // the regions' text bits, parked for the keyword ids (acgpu_longest_bits.hip)
        if ((rc = d.lenbuf.ensure((size_t)Bl.n_regions * longest_bits_region_text_bytes() + 64))) return rc;
        Bl.d_text = (uint32_t *)d.lenbuf.p;
    }
    Bl.d_pred = (uint32_t *)d.blockmax.p;
    Bl.d_true = Bl.d_pred + Bl.n_regions;
    Bl.grid = (int)std::min<uint64_t>((uint64_t)d.n_cu, (Bl.n_regions + 15) / 16);
    Bl.debug = (uint32_t)(tunables().tile_debug >> 32);
    unsigned long long *d_slot = nullptr;
    if ((rc = slot_on_device(r, &d_slot))) return rc;
    void *const seen = d.bits_state_seen;
    d.bits_state_seen = nullptr; // (until both kernels are enqueued: an error below leaves the words in an unknown state)
    // the whole pipeline in two launches: text in, records out; then the seams, the result and the state for the next call.
    // (Profiled calls take the dispatches' own start / stop timestamps: marker packets between the steps cost more than the
    // second kernel does.)
    const bool timed = r.profiled;
    HIP_TRY(launch_longest_bits(d.T, Bl, d_slot, reinterpret_cast<acgpu_device_result *>(sh->d_result),
                                (unsigned long long *)d.bits_state.p, (uint32_t)state_words, stream, timed ? r.ev[0] : nullptr,
                                timed ? r.ev[1] : nullptr, timed ? r.ev[2] : nullptr));
    d.bits_state_seen = seen;
#ifdef ACGPU_ABLATION
    if (Bl.debug && !r.done) {
        HIP_TRY(hipStreamSynchronize(stream));
        unsigned long long mism = 0;
        (void)hipMemcpy(&mism, (const char *)d.bits_state.p + 24, 8, hipMemcpyDeviceToHost); // (the finish kernel has zeroed it: kept for builds that skip it)
        fprintf(stderr, "[k_longest_bits debug %u] segments whose assumed entry was not the exit before them: %llu\n", Bl.debug, mism);
    }
#endif
    return close_call(r, CallForm::LongestBits, "k_longest_bits", sh->own_end - sh->own_begin, /*done_is_ev2=*/timed); // (the finish kernel's own end)
}

// What the chain stage of a LONGEST call is told whichever pipeline runs in front of it: the shard's bounds and the chain's entry,
// the per-tile counts and their offsets, the records' place, the chain's exit.  (Called with those buffers allocated; the
// tiles, the lengths and the bitmaps are the pipeline's own.)
LongestChainLaunch longest_chain_launch(const HostTables &t, const DeviceState &d, const CallRecord &r, uint64_t entry) {
    LongestChainLaunch Cn{};
    Cn.d_out_id = d.T.term_id; // state[] holds the trie node of the longest keyword starting at a position
    Cn.own_begin = (uint32_t)r.shard.own_begin;
    Cn.own_end = (uint32_t)r.shard.own_end;
    Cn.entry = (uint32_t)entry;
    Cn.max_len = t.max_len;
    Cn.d_counts = (uint32_t *)d.chunk_counts.p;
    Cn.d_offsets = (const uint64_t *)d.offsets.p;
    Cn.d_out = r.d_out;
    Cn.cap = r.cap;
    Cn.record_kind = r.record_kind;
    Cn.d_exit = (unsigned long long *)d.counter.p;
    Cn.len_units = (uint32_t)r.shard.n_units;
    return Cn;
}

// {count, 0, exit} into the call's pinned host slot (and the device result) by the pipeline's last kernel: the count is the
// grand total the prefix sum over n_tiles counts left, the exit what the count pass wrote into the counter line
int publish_chain_result(const DeviceState &d, CallRecord &r, uint32_t n_tiles) {
    int rc;
    unsigned long long *d_slot = nullptr;
    if ((rc = slot_on_device(r, &d_slot))) return rc;
    HIP_TRY(launch_publish_result((const unsigned long long *)scan_total(d, n_tiles), (const unsigned long long *)d.counter.p,
                                  d_slot, reinterpret_cast<acgpu_device_result *>(r.shard.d_result), r.stream));
    return ACGPU_OK;
}

// Any other dense dictionary with range classes or small class pages, long texts, Set and Map records: the walks of the chain's own
// positions only (k_longest_follow, acgpu_longest_follow.hip) in place of the length array, the synchronisation points and the chain
// pass; the bitmaps, counts and first positions it leaves are what the prefix sum and k_longest_emit_ends below read.  It checks its
// own result like k_longest_bits and is redone the same way.
int enqueue_longest_follow(acgpu_automaton *a, DeviceState &d, CallRecord &r, uint64_t entry, int bits_level, uint32_t fol_hot) {
    const HostTables &t = a->t;
    const acgpu_shard *sh = &r.shard;
    const hipStream_t stream = r.stream;
    int rc;
    LongestFollowLaunch F{};
    F.d_hay = sh->d_hay;
    F.n_units = (uint32_t)sh->n_units;
    F.own_end = (uint32_t)sh->own_end;
    F.entry = (uint32_t)entry;
    F.g0 = (uint32_t)entry & ~31u;
    // a lane walks a segment of 1024 positions behind a run-up.  (Segments of 512 for texts that leave half the chip's lanes
    // without one were measured: 4.95 against 3.30 ms per 2^28 units of the README word list -- the kernel is bound by the
    // number of gathers, and a run-up of a whole segment is a third more of them.)  Tunable region_units (64 .. 1024): the first
    // try's run-up, for A/B.
    const uint32_t seg_units = longest_follow_seg_units();
    F.seg_log2 = 10;
    const uint32_t region_units = 64 * seg_units;
    F.n_regions = (uint32_t)((sh->own_end - F.g0 + region_units - 1) / region_units);
    // The first try's run-up is 128 positions: on a text with separators every chain lands on each of them (no keyword goes
    // across), so chains merge within a word, and the run-up is a fifth of the gathers at 512 (measured on the README word
    // list: 3.27 ms per 2^28 units at 512, 2.85 at 256, 2.65 at 128).  A text on which that fails -- the kernel notices --
    // is redone with a whole segment, and this pool remembers it (d.fol_level): the next call starts there, or, if chains
    // do not merge within 1024 positions either, with the walk pipeline.
    const int64_t ru = tunables().region_units;
    F.runup = bits_level == 0 ? (ru >= 64 && ru <= 1024 ? (uint32_t)ru : 128u) : seg_units;
    F.tile_log2 = 2; // (emit tiles of 4096 positions)
    F.hot_rows = fol_hot;
    const uint32_t n_tiles = (F.n_regions * (region_units / seg_units)) >> F.tile_log2;
    if ((rc = borrow_counter_line(d, stream, /*clear=*/true))) return rc;
    if ((rc = ensure_scan_buffers(d, n_tiles))) return rc;
    if ((rc = d.chain.ensure((size_t)n_tiles * 4 + 64))) return rc;
    if ((rc = d.blockmax.ensure((size_t)F.n_regions * 8 + 64))) return rc;
    const size_t bit_bytes = ((size_t)sh->n_units / 128 + 2) * 16;
    if ((rc = d.chainbits.ensure(bit_bytes * 2))) return rc;
    F.d_bits = (uint32_t *)d.chainbits.p;
    F.d_ebits = F.d_bits + bit_bytes / 4;
    F.d_state = nullptr;
    if (r.record_kind == ACGPU_REC_MAP) {
        if ((rc = d.statebuf.ensure((size_t)sh->n_units * 4 + 64))) return rc;
        F.d_state = (uint32_t *)d.statebuf.p;
    }
    F.d_sync = (uint32_t *)d.chain.p;
    F.d_counts = (uint32_t *)d.chunk_counts.p;
    F.d_exit = (unsigned long long *)d.counter.p;
    F.d_pred = (uint32_t *)d.blockmax.p;
    F.d_true = F.d_pred + F.n_regions;
    F.grid = (int)std::min<uint64_t>(2ull * d.n_cu, (F.n_regions + 15) / 16);
    { // the end bits are merged with atomicOr: zeros from the first word the chain can touch to where its last match can end
        const size_t first = F.g0 >> 5, last = std::min<size_t>(bit_bytes / 4, (((size_t)sh->own_end + t.max_len) >> 5) + 2);
        if (last > first) HIP_TRY(hipMemsetAsync(F.d_ebits + first, 0, (last - first) * 4, stream));
    }
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[0], stream));
    HIP_TRY(launch_longest_follow(d.T, F, t.range_cls, r.record_kind == ACGPU_REC_MAP, stream));
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[1], stream));
    LongestChainLaunch Cn = longest_chain_launch(t, d, r, entry); // (its counts and exit: what F.d_counts and F.d_exit point to)
    Cn.d_state = F.d_state;
    Cn.len_bytes = 1; // (no lengths: the emit pass reads the two bitmaps)
    Cn.tile_units = seg_units << F.tile_log2;
    Cn.n_tiles = n_tiles;
    Cn.d_bits = F.d_bits;
    Cn.d_ebits = F.d_ebits;
    HIP_TRY(launch_exclusive_scan(Cn.d_counts, Cn.n_tiles, (uint64_t *)d.offsets.p, (uint64_t *)d.scan_tmp.p, stream));
    HIP_TRY(launch_longest_emit(Cn, F.d_sync, stream));
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[2], stream));
    if ((rc = publish_chain_result(d, r, Cn.n_tiles))) return rc;
    return close_call(r, CallForm::LongestFollow, "k_longest_follow", sh->own_end - sh->own_begin);
}

// The walk pipeline: a length for every position (the walk), then the chain: synchronisation points -> count pass -> prefix sum -> emit pass.
int enqueue_longest_walk(acgpu_automaton *a, DeviceState &d, CallRecord &r, uint64_t entry) {
    const HostTables &t = a->t;
    const acgpu_shard *sh = &r.shard;
    const hipStream_t stream = r.stream;
    const int record_kind = r.record_kind;
    const uint64_t own_len = sh->own_end - sh->own_begin;
    LongestScanLaunch S{};
    S.block = 1024;
    // two workgroups per CU share the LDS (hot trie rows: at most 72 KB each); a short haystack gets fewer (every
    // workgroup stages the rows before it starts)
    S.grid = (int)std::min<uint64_t>(2ull * d.n_cu, (own_len + S.block - 1) / S.block);
    S.chunk_units = 0;
    S.n_chunks = 0;
    S.d_hay = sh->d_hay;
    S.n_units = (uint32_t)sh->n_units;
    S.own_begin = (uint32_t)sh->own_begin;
    S.own_end = (uint32_t)sh->own_end;
    S.len_bytes = t.max_len < 65536 ? 2 : 4;
    uint32_t lds_rows = 0;
    // (table classes: the general walk keeps the class pages behind its rows -- acgpu_build.cpp 7c -- when they are small)
    // (measured, tools/longest_shapes.py: the README word list case-insensitive, 27 classes: 8.13 -> 6.08 ms per 2^28 units; 3000 CJK
    // units, where a row is 12 KB and the walk waits for the table in global memory anyway: 4.74 -> 5.05 -- so: small alphabets only)
    const size_t walk_pages = (t.dense && !t.range_cls && !t.dfa_pages.empty() && t.dfa_pages.size() * 2 <= 16 * 1024 && t.n_cls <= 512) ? t.dfa_pages.size() * 2 + 16 : 0;
    if (t.dense && t.n_cls) lds_rows = (uint32_t)std::min<uint64_t>(t.n_states, (72 * 1024 - walk_pages) / ((uint64_t)t.n_cls * 4));
    // range classes (case sensitive, keyword units within a span of 63) take the lean walk; tunable force_kernel=1
    // keeps the general one
    const bool range = t.dense && t.range_cls && t.n_cls == t.cls_span + 1 && tunables().force_kernel != 1 &&
                       (uint64_t)t.n_states * t.n_cls * 4 < (1ull << 31);
    S.form = range ? LongestWalkForm::Range : LongestWalkForm::General;
    if (range) lds_rows = (uint32_t)std::min<uint64_t>(t.n_states, (72 * 1024) / ((uint64_t)t.n_cls * 4) - 2);
    S.lds_rows = lds_rows;
    S.lds_bytes = std::max<size_t>((size_t)(lds_rows + (range ? 2 : 0)) * t.n_cls * 4, 16) + (range ? 0 : walk_pages);
    S.pages_bytes = range ? 0u : (uint32_t)walk_pages; // (0: classes from the table in global memory)
    int rc;
    // the work-list form of the range-class walk (tunable force_kernel=4 keeps the lock-step form): keywords below 64000 units,
    // LDS rows below 64 KiB (the row offset is the low word of an entry), two workgroups per CU.  It stores ONE byte per length,
    // 255 = "255 or more: see the 16-bit side array" -- half the bytes written by the walk and read back by the chain passes
    if (range && t.max_len < 64000 && tunables().force_kernel != 4) {
        S.form = LongestWalkForm::RangeList;
        S.lds_rows = lds_rows = std::min<uint32_t>(t.n_states, longest_list_max_rows(t.n_cls, record_kind == ACGPU_REC_MAP));
        S.lds_bytes = longest_list_lds_bytes(record_kind == ACGPU_REC_MAP);
        // two workgroups per CU (Set records: 60 KiB of rows + 17 KiB of lists each; Map: 52 + 26)
        S.grid = (int)std::min<uint64_t>(2ull * d.n_cu, (own_len + 16 * 1024 - 1) / (16 * 1024));
        S.len_bytes = 1;
        if ((rc = d.lenbig.ensure((size_t)sh->n_units * 2 + 64))) return rc;
        S.d_len_big = (uint16_t *)d.lenbig.p;
    }
    if ((rc = d.lenbuf.ensure((size_t)sh->n_units * S.len_bytes + 64))) return rc;
    S.d_len = d.lenbuf.p;
    if ((rc = d.blockmax.ensure((own_len / 64 + 2) * 4))) return rc;
    S.d_blockmax = (uint32_t *)d.blockmax.p;
    S.d_state = nullptr;
    if (record_kind == ACGPU_REC_MAP) {
        if ((rc = d.statebuf.ensure((size_t)sh->n_units * 4 + 64))) return rc;
        S.d_state = (uint32_t *)d.statebuf.p;
    }
    // Set records over a small alphabet: k_longest_block (first round through the root table, the live walks through its own
    // work list), then the general kernel for the chunks it flagged.  A wave's span must fit the 16-bit lane positions of its
    // queue.
    const uint64_t blk_waves = (uint64_t)S.grid * (S.block / 64), blk_chunks = (own_len + 1023) / 1024;
    const uint64_t blk_span = (blk_chunks + blk_waves - 1) / std::max<uint64_t>(blk_waves, 1);
    const bool root_form = S.form == LongestWalkForm::RangeList && record_kind == ACGPU_REC_SET && d.T.root_b != 0 &&
                           blk_span * 1024 <= (1u << 19) && sh->n_units >= 4096 && (sh->own_begin & 7) == 0;
    if (root_form) {
        S.span_chunks = (uint32_t)blk_span;
        if ((rc = d.todo.ensure(blk_chunks + 64))) return rc;
        S.d_todo_w = (uint8_t *)d.todo.p;
    }
    // positions per chain lane: the synchronisation scan skips 64-position blocks that cannot reach the tile, so tiles
    // can stay small (more lanes, shorter dependent chains) even when keywords are long
    // (measured at config 4: 6144 positions per lane are best with 256-position chunks of one-byte lengths -- 4096: +15 %,
    // 8192: +3 %, 12288: +22 % for the chain passes; small inputs get more, shorter lanes)
    const uint64_t T_units = tunables().region_units > 0 ? (uint64_t)tunables().region_units : (own_len >= (1ull << 24) ? 6144 : 1024);
    const uint32_t n_tiles = (uint32_t)((sh->own_end - entry + T_units - 1) / T_units);
    if ((rc = borrow_counter_line(d, stream, /*clear=*/true))) return rc;
    if ((rc = ensure_scan_buffers(d, n_tiles))) return rc;
    LongestChainLaunch Cn = longest_chain_launch(t, d, r, entry);
    Cn.tile_units = (uint32_t)T_units;
    Cn.n_tiles = n_tiles;
    Cn.d_len = d.lenbuf.p;
    Cn.d_len_big = S.d_len_big;
    Cn.d_state = S.d_state;
    Cn.len_bytes = S.len_bytes;
    Cn.d_blockmax = S.d_blockmax;
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[0], stream));
    const char *kname = "";
    if (root_form) {
        LongestScanLaunch Sb = S;
        Sb.debug = (uint32_t)(tunables().tile_debug >> 32);
        Sb.lds_rows = std::min<uint32_t>(t.n_states, longest_block_max_rows(t.n_cls));
        HIP_TRY(launch_longest_block(d.T, Sb, stream, &kname));
        S.d_todo = S.d_todo_w;
        HIP_TRY(launch_longest_scan(d.T, S, stream, nullptr));
    } else {
        HIP_TRY(launch_longest_scan(d.T, S, stream, &kname));
    }
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[1], stream));
    if ((rc = d.chain.ensure((size_t)Cn.n_tiles * 4 + 64))) return rc;
    uint32_t *d_sync = (uint32_t *)d.chain.p;
    // Chain: synchronisation points; the count pass, which marks the chain's matches in a bitmap -- through LDS for 1- and 2-byte
    // lengths (k_longest_chain_lds), which also marks their ends in a second bitmap, from global memory for 4-byte lengths
    // (k_longest_chain); prefix sum; the records written position-parallel from the bitmaps.
    const bool lds_pass = Cn.len_bytes <= 2;
    const size_t bit_bytes = ((size_t)sh->n_units / 128 + 2) * 16; // whole groups of four words (16-byte stores)
    if ((rc = d.chainbits.ensure(bit_bytes * (lds_pass ? 2 : 1)))) return rc;
    Cn.d_bits = (uint32_t *)d.chainbits.p;
    Cn.d_ebits = lds_pass ? Cn.d_bits + bit_bytes / 4 : nullptr;
    HIP_TRY(hipMemsetAsync(d.chainbits.p, 0, bit_bytes * (lds_pass ? 2 : 1), stream));
    HIP_TRY(launch_longest_sync(Cn, d_sync, stream));
    if (lds_pass) HIP_TRY(launch_longest_chain_lds(Cn, d_sync, stream));
    else HIP_TRY(launch_longest_chain(Cn, d_sync, stream));
    HIP_TRY(launch_exclusive_scan(Cn.d_counts, Cn.n_tiles, (uint64_t *)d.offsets.p, (uint64_t *)d.scan_tmp.p, stream));
    HIP_TRY(launch_longest_emit(Cn, d_sync, stream));
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[2], stream));
    if ((rc = publish_chain_result(d, r, Cn.n_tiles))) return rc;
    return close_call(r, CallForm::LongestWalk, kname, own_len);
}

} // namespace

namespace acgpu { // (what acgpu_calls.h and acgpu_host.h declare: described there)

int check_longest_shard(const HostTables &t, acgpu_shard *sh) {
    const uint32_t halo = t.max_len > 0 ? t.max_len - 1 : 0;
    if (!sh->text_end && sh->n_units - sh->own_end < halo) return ACGPU_E_INVALID; // right halo too short
    if (sh->chain_entry < (int64_t)sh->own_begin) return ACGPU_E_INVALID;
    sh->chain_exit = (int64_t)std::max<uint64_t>((uint64_t)sh->chain_entry, sh->own_end);
    return ACGPU_OK;
}

bool filter_is_selective(const HostTables &t) { return t.filt_k != 0 && t.filt_density <= 0.08; }

int enqueue_longest(acgpu_automaton *a, DeviceState &d, CallRecord &r, int bits_level) {
    const HostTables &t = a->t;
    int rc;
    if ((rc = check_longest_shard(t, &r.shard))) return rc;
    r.user_shard->chain_exit = r.shard.chain_exit;
    const acgpu_shard *sh = &r.shard;
    const uint64_t entry = (uint64_t)sh->chain_entry;
    if (entry >= sh->own_end || t.n_states <= 1) return enqueue_empty(r, sh->chain_exit);
    const uint64_t own_len = sh->own_end - sh->own_begin;
    const int64_t lform = tunables().longest_form;
    const bool bits_form = bits_level < 2 && (r.record_kind == ACGPU_REC_SET || d.T.bits_idkeys != nullptr) && d.T.bits_rk != 0 && !(lform & 1) &&
                           (own_len >= (1ull << 21) || (lform & 4)) && tunables().force_kernel == 0;
    if (bits_form) {
        r.level = bits_level;
        return enqueue_longest_bits(a, d, r, entry, bits_level);
    }
    const size_t fol_pages = (!t.range_cls && !t.dfa_pages.empty()) ? t.dfa_pages.size() * 2 : 0;
    const bool fol_classes = t.dense && ((t.range_cls && t.n_cls == t.cls_span + 1) || fol_pages > 0);
    const uint32_t fol_hot = fol_classes ? longest_follow_hot_rows(t.n_cls, t.n_states, (uint32_t)fol_pages) : 0;
    if (bits_level < d.fol_level) bits_level = d.fol_level; // (what earlier calls on this pool have learnt about its texts)
    r.level = bits_level;
    // (Not where the walk pipeline has its root table -- dictionaries over up to four letters whose first 14 or 7 units one lookup
    // decides: config 4's dictionary with Map records 3.71 against 5.79 ms per 2^29 units, tools/longest_shapes.py.  Tunable
    // longest_form bit 8: there too, for A/B.)
    const bool follow_form = bits_level < 2 && fol_hot > 0 && !(lform & 2) && (own_len >= (1ull << 20) || (lform & 4)) && tunables().force_kernel == 0 &&
                             (t.root_b == 0 || (lform & 8));
    if (follow_form) return enqueue_longest_follow(a, d, r, entry, bits_level, fol_hot);
    return enqueue_longest_walk(a, d, r, entry);
}

} // namespace acgpu
