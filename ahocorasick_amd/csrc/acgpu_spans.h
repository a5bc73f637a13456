// acgpu_spans.h -- the piece loop with the merge behind every piece (acgpu_spans.hip) as its two callers see it: the spans entries,
// whose final spans go to the caller, and the cover entries (acgpu_cover.hip), whose final spans stay in the pool for the plan and
// the emit.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "acgpu_host.h"

namespace acgpu {

// 64-bit words in front of the tiles' values in d.spans_work: {n_final, n_carry, the piece's bound in bytes (UTF-8), and for a
// cover call: the settled position L, the elements of the piece's final spans (written by the plan of a DROP call), and B itself
// (final_below), which the last piece of a RANGE settles at, the first span the piece withheld as {start, end}}
constexpr int kSpanHead = 7;
constexpr int kSpanSettled = 3, kSpanDropped = 4, kSpanBelow = 5, kSpanCarry0 = 6;

// A RANGE of a buffer instead of a whole text (a cover stream's feed, acgpu_stream.hip): the pieces run over the owned units
// [own_begin, own_end) of the scan's shard, the first piece's list begins with the spans an earlier range withheld, whether the
// range's end is the text's end comes from outside, and what the range's last piece withholds goes back to the host.  Spans are
// in elements of the buffer; a carried span may begin in front of it (start < 0: only its end and "it began earlier" matter).
struct SpansRange {
    uint64_t own_begin = 0, own_end = 0;
    bool text_end = true;           // the range's last piece finalises everything, as a whole text's
    const int2 *carry_in = nullptr; // host
    uint32_t n_carry_in = 0;
    std::vector<int2> carry_out;    // out: the spans the range's last piece withheld
    int64_t chain_exit = 0;         // out, if scanned: where the chain leaves the range
    bool scanned = false;           // out: a piece was scanned
};

// What one call holds while it runs (the caller holds d.mu).  Positions are ELEMENTS of the text as the caller sees it: units, or
// bytes of a UTF-8 text.
struct SpansCall {
    acgpu_automaton *a;
    DeviceState &d;
    hipStream_t stream;
    const Utf8Text *u8 = nullptr; // a UTF-8 text: the scan runs over its units, the merge over bytes
    // a batch of UTF-8 texts staged as one shard (u8 == &ub->text): the merge runs over VIRTUAL COORDINATES, the span's bytes with
    // one phantom element behind every haystack (utf8_virtual_offsets, acgpu_host.h), and cat_off below is voff
    const Utf8Batch *ub = nullptr;
    int32_t *h_out = nullptr;     // the host entry's result (through d.spans_out) ...
    int32_t *d_out = nullptr;     // ... or the device entry's
    uint64_t cap = 0;
    uint64_t out_pos = 0;         // final spans so far (beyond cap: counted, not written)
    uint32_t n_carry = 0;         // spans the piece before withheld, in carry buffer `cur`
    uint32_t carry_cap = 0;
    int cur = 0;
    acgpu_spans_stats st{};
    // A cover call: a piece's final spans go to d.cover_spans (all of them, text coordinates), and the piece's settled position
    // and whatever `planned` adds ride with {n_final, n_carry} in the piece's one wait.
    bool to_pool = false;
    // ... called behind the scatter and before that wait, with the head of d.spans_work (device), the piece's spans (device; the
    // first slot[0] of them are final) and m, the intervals merged, which bounds their number
    int (*planned)(void *ctx, uint64_t *d_slot, const int2 *d_spans, uint64_t m) = nullptr;
    // ... called behind the piece's wait, with m again and whether the piece was the last: the caller's step behind the merge
    int (*merged)(void *ctx, uint64_t m, bool last) = nullptr;
    void *ctx = nullptr;
    // A batch call (acgpu_spans_batch_u16): the text is the haystacks' concatenation, a separator behind each; cat_off (device,
    // n_hay + 1 words) = every haystack's first unit in it.  A piece's final spans are tagged with their haystack and rebased to
    // it in d.batch_out, and 12 bytes per span leave for h_out.  cat_off == nullptr with tag_all: a batch that goes haystack by
    // haystack -- the text is haystack `tag`.
    const uint32_t *cat_off = nullptr;
    uint32_t n_hay = 0;
    bool tag_all = false;
    int32_t tag = 0;
    uint64_t piece_own_hi = 0;    // in, for `planned`: the piece owned [.., piece_own_hi) ...
    bool piece_last = false;      // ... and was the last, or the text as one piece
    uint64_t piece_final = 0;     // out: the piece's final spans
    int64_t piece_settled = 0;    // out, not on the last piece: L = min(B, start of the first carried span)
    uint64_t piece_dropped = 0;   // out: slot[kSpanDropped] if `planned` is set
    // a RANGE whose end is not the text's: the piece was the range's last, which nothing finalises but which SETTLES at
    // piece_below = B itself -- a carried span may begin in front of it (the caller cuts it there)
    bool piece_range_last = false; // in, for `merged`
    int64_t piece_below = 0;      // out, with piece_range_last
    int2 piece_carry0{0, 0};      // out, with piece_range_last: the first span the piece withheld, if piece_carried
    uint32_t piece_carried = 0;   // out: the spans the piece withheld
};

// The pieces of a whole text, each merged behind its scan: chain = the chain's entry, whole = the text is scanned as one piece.
// range given: the pieces of that range of the scan's shard instead (SpansRange above).
int spans_pieces(SpansCall &c, int64_t chain, bool whole, const PieceScan &scan, uint64_t n_units, SpansRange *range = nullptr);

} // namespace acgpu
