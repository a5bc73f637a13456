// acgpu_utf8.hip -- acgpu_match_utf8 (include/acgpu.h): a UTF-8 haystack validated and transcoded on the device, scanned as the
// one shard acgpu_match_u16 would scan, its records rewritten to byte offsets of the caller's buffer.
//
// Four kernels around the unchanged scan (match_shard):
//   k_utf8_count : a lane per 16 bytes: validates them strictly and counts the UTF-16 units they decode to; one sum per block of
//                  4096 bytes, the smallest offending offset into one 64-bit atomicMin;
//   k_utf8_scan  : one workgroup: the block sums become block bases, their total n_units;
//   k_utf8_write : the same lanes again (after the host has seen n_units and that nothing offends): every lead byte decodes its
//                  code point and stores one or two units, and the lane of a unit whose index is a multiple of 32 stores where
//                  that unit's sequence begins -- the checkpoint table, 4 bytes per 32 units;
//   k_utf8_batch_map : a lane per record: start and end - 1 go from units to bytes through the nearest checkpoint at or below
//                  them and a walk of at most 31 units over the lead bytes (locate, batch_bytes).
// Every form of the entry is these four with one more argument, and each piece of logic stands once:
//  * count: count_units<BATCH, OPEN> is the body of k_utf8_count, k_utf8_batch_count (acgpu_match_batch_utf8 here,
//    acgpu_summary_batch_utf8 in acgpu_summary.hip: every haystack validated on its own -- lane_view's twelfth mask, the cuts) and
//    k_utf8_open_count (acgpu_stream_feed_utf8, acgpu_stream.hip: unless the feed is the last, a sequence that the buffer's end
//    cuts is held back, not refused);
//  * write: k_utf8_write and k_utf8_batch_write store through store_ascii16 and store_lead; the batch's writer also stores the
//    separator unit behind every haystack and every haystack's first unit (cat_off), the checkpoints stay those of the buffer read
//    as one text;
//  * map: locate is the rule from a unit to its byte, batch_bytes a record's.  k_utf8_batch_map rewrites records in place -- a
//    text's (utf8_map_records without a batch) or, for acgpu_replace_batch_utf8 (acgpu_replace.hip), a batch's to bytes of the
//    SPAN; k_utf8_batch_pos maps one unit position, a piece's boundary, of either (utf8_map_position); k_utf8_batch_tag is
//    k_batch_tag and the map in one, k_summary_utf8_bytes maps the summaries' first records;
//  * staging: Utf8Aux lays out the device buffers and utf8_validate runs count, scan and the one wait for stage_utf8_parts (a
//    text in two host parts: acgpu_stream_feed_utf8's carried bytes and chunk; stage_utf8_text is its one-part, closed case) and
//    for stage_utf8_batch;
//  * lossy: acgpu_match_utf8_lossy and acgpu_match_batch_utf8_lossy (acgpu_summary_batch_utf8_lossy in acgpu_summary.hip) are the
//    same bodies with another policy (match_utf8<P>, match_batch_utf8<P>; Utf8Errors::replace down to utf8_validate) over the LOSSY
//    instantiations of lane_view, count_units, the writers and locate: nothing is refused, a maximal ill-formed subpart is one
//    U+FFFD, and the maps walk a start bitmap that the lossy writers store beside the checkpoints.  The lossy replace entries
//    (acgpu_replace.hip) and the lossy feeds (acgpu_stream.hip) stage through the same two functions with that policy; the feeds'
//    validator is k_utf8_lossy_open_count, lane_view's LOSSY and OPEN form.
// What a lane knows about its 16 bytes is eleven bit masks over a window of 24 bytes (the 4 before, its own, the 4 behind), built
// by one function that both passes over the text share, so they cannot disagree about a count; the two writers share the
// decoder, so they cannot disagree about a unit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "acgpu_device.h"
#include "acgpu_host.h"
#include "acgpu_internal.h"
#include "acgpu_kernels.h"

using namespace acgpu;

namespace {

constexpr int kU8Threads = 256;
constexpr uint32_t kU8Lane = 16;                     // bytes per lane
constexpr uint32_t kU8Block = kU8Threads * kU8Lane;  // bytes per workgroup: 4096
constexpr uint32_t kU8Own = 0x000ffff0u;             // the window's bits of a lane's own bytes
constexpr uint32_t kCkptLow = 0x80000000u;           // checkpoint flag: the unit is the low surrogate of the sequence named

static_assert(sizeof(acgpu_utf8_stats) == 24, "the layout include/acgpu.h promises");
static_assert(sizeof(acgpu_utf8_batch_stats) == 24, "the layout include/acgpu.h promises");
static_assert(sizeof(acgpu_utf8_lossy_stats) == 32, "the layout include/acgpu.h promises");

// What a lane knows about its bytes.  Bit k of a mask stands for the byte at offset o - 4 + k of the text, o the lane's first.
struct LaneView {
    uint32_t w[6];   // the window's bytes, zero where the text has none (before its begin, at and behind its end)
    uint32_t lead;   // own bytes inside the text that are no continuation bytes: every one begins a sequence
    uint32_t four;   // ... of those, the leads of 4-byte sequences (two units)
    uint32_t bad;    // own bytes at which a strict decoder stops: leads of ill-formed sequences, unclaimed continuation bytes
    uint32_t cut;    // the batch form: bytes of the window's bits 4..23 that begin a haystack (or are the buffer's end)
    uint32_t next;   // the batch form: the first boundary j with boff[j] >= o -- until the lane meets it, its bytes are haystack j - 1's
    uint32_t tail;   // the open form: the own byte (at most one) that begins a sequence which the buffer's end cuts, so far well-formed
    __device__ __forceinline__ uint32_t byte(int k) const { return (w[k >> 2] >> (8 * (k & 3))) & 0xffu; }
    __device__ __forceinline__ uint32_t units() const { return __popc(lead) + __popc(four); }
};

// Every lane of the wave takes part (the neighbours' bytes come through cross-lane moves; a wave's first and last lane load
// theirs).  in: 16-byte aligned, readable up to n rounded up to 16 and 4 bytes more.
//
// BATCH: the buffer is n_hay haystacks, haystack j the bytes [boff[j], boff[j + 1]), boff[0] = 0, boff[n_hay] = n; every haystack
// has to be well-formed ON ITS OWN.  The twelfth mask, cut, has a bit where a byte begins a haystack, and
//  * a lead is bad when a byte it needs lies at or behind a cut (the haystack's end truncates its sequence);
//  * a continuation byte that stands at a cut is unclaimed (nothing of its own haystack can claim it).
// Why the buffer's smallest flagged offset p is then the first ill-formed haystack's own error position: let h be the first
// haystack that is ill-formed and e the byte at which a strict decoder of h alone stops.  Every byte before e -- the haystacks
// before h, and h's bytes before e -- belongs to a sequence that lies whole inside its own haystack; no cut falls behind its lead
// and no continuation byte of it stands at a cut, so these bytes are judged as the one-text rules judge them, by bytes of their own
// haystack alone: none is flagged.  At e the decoder stops for one of three reasons.  A lead whose sequence is ill-formed in its
// bytes: the one-text rules flag it.  A lead whose sequence the end of h truncates: the cut rule flags it, AT THE LEAD, and a
// lead lies before every byte its sequence could claim in the next haystack, so no flag of a mis-claimed byte comes first.
// A continuation byte that no sequence of h reaches: if it is h's first byte, it stands at a cut; if not, the byte before it is
// h's, decoded, and did not claim it -- as in one text.  So p = e.  The cuts come from the offsets themselves: a search for the
// first boundary at or behind the lane's first byte, then a walk over the boundaries of the window -- haystacks that are empty
// are several boundaries at one byte, one bit.
//
// OPEN: the buffer is a text that GOES ON behind byte n (a feed of acgpu_stream_feed_utf8 that is not the last).  A lead in the
// last three bytes whose sequence reaches behind the buffer's end is judged by the bytes that are there alone -- the lead byte
// itself, the second byte against the range its lead allows, a third byte as a continuation byte: what
// codecs.getincrementaldecoder("utf-8") holds back.  If they pass, the lead is neither bad nor counted (lead, four): it is the
// `tail`, and the units are those of the n - tail bytes before it, which end on a sequence's end and are well-formed as a text
// of their own.  Its continuation bytes are claimed as ever.  If they do not pass, the lead is bad NOW, as for a decoder that no
// later byte can satisfy.  One prefix is held although it is none: ED A0..BF as the last two bytes (bad_open).
// At most one tail exists in a buffer: let p < q be two leads of the last three bytes that both reach behind the end.  Then q
// is one of the bytes p + 1 .. n - 1 that p's sequence needs and that are there, and q is a lead, no continuation byte: p does
// not pass.  So of such leads only the last can pass, and the one lane that owns it stores n - position without a race.
//
// LOSSY: nothing is refused.  The masks are those of a decoder that puts one U+FFFD for every MAXIMAL ILL-FORMED SUBPART, as
// bytes.decode("utf-8", "replace") does: a lead claims the byte behind it only if that is a continuation byte in the range the
// lead allows, the one behind that only if it claimed the first and it is a continuation byte, a third likewise (4-byte leads
// only); it never claims a byte at or behind a cut, and C0, C1, F5..FF claim nothing (claimed_lossy).  Then
//  * lead: every byte that is no claimed continuation byte begins a unit -- a sequence, or a subpart of one to three bytes;
//  * bad:  of those, the REPLACED ones: a lead that did not claim all it needs, an unclaimed continuation byte;
//  * four: the 4-byte leads that are not replaced.
// On well-formed input each equals its strict counterpart (a lead claims all it needs, which is what the strict rules ask).
// A continuation byte looks at most 3 bytes back for the lead that claims it, and whether that lead does depends on the cuts
// BETWEEN them: the batch form's cut mask reaches down to bit 1 here, `next` stays the first boundary at or behind o.
//
// LOSSY and OPEN (a feed of acgpu_stream_feed_utf8_lossy that is not the last): the last 1..3 bytes are held back exactly when
// they are a lead with everything it has claimed so far under claimed_lossy, and that claim reaches the buffer's end while the
// lead still needs more.  Everything else is decided now -- a lead whose PRESENT bytes fail is a subpart now, whatever follows
// (so ED A0 at the end is two U+FFFD now: the strict form's exception is not mirrored, only chunking invariance is promised).
// The held lead is the `tail`: neither a start (lead) nor replaced (bad) in this buffer, the bytes it claimed are claimed as ever.
// At most one tail exists in a buffer: let p < q be two leads of the last three bytes.  For p to be a tail its claim reaches the
// end, so it claimed q -- but a claimed byte is a continuation byte and q is a lead.  So only the last such lead can pass, and the
// one lane that owns it stores n - position without a race.
// The bytes before the tail p decode as a CLOSED text of p bytes exactly as they do here: a claim is a run of continuation bytes
// directly behind its lead, and p is none, so no lead before p claims p or anything behind it -- which bytes before p are claimed,
// and which leads before p claimed all they need, is decided by bytes before p alone, and in the closed text the window reads
// zero from p on, no continuation byte either.  So the sums are those of the n - tail bytes, and k_utf8_lossy_write runs
// unchanged over them.
template <bool BATCH, bool OPEN = false, bool LOSSY = false>
__device__ __forceinline__ LaneView lane_view(const uint8_t *__restrict__ in, uint32_t n, uint32_t o, const uint32_t *__restrict__ boff = nullptr,
                                              uint32_t n_hay = 0) {
    static_assert(!(BATCH && OPEN), "a batch's haystacks end where they end");
    LaneView v;
    uint4 own = make_uint4(0, 0, 0, 0);
    if (o < n) own = *reinterpret_cast<const uint4 *>(in + o);
    uint32_t prev = __shfl_up(own.w, 1), next = __shfl_down(own.x, 1);
    const uint32_t lane = lane_id();
    if (lane == 0) prev = (o != 0 && o < n) ? *reinterpret_cast<const uint32_t *>(in + o - 4) : 0u;
    if (lane == kWave - 1) next = (o + kU8Lane < n) ? *reinterpret_cast<const uint32_t *>(in + o + kU8Lane) : 0u;
    v.w[0] = prev;
    v.w[1] = own.x;
    v.w[2] = own.y;
    v.w[3] = own.z;
    v.w[4] = own.w;
    v.w[5] = next;
    // the window's bytes [0, k_end) lie inside the text; what a load brought from behind its end reads as zero -- no
    // continuation byte, so a sequence that the end of the text truncates fails at its lead
    const int k_end = o >= n ? 4 : (n - o >= 20u ? 24 : (int)(n - o) + 4);
#pragma unroll
    for (int j = 1; j < 6; ++j) {
        const int r = k_end - 4 * j;
        v.w[j] = r >= 4 ? v.w[j] : (r <= 0 ? 0u : v.w[j] & ((1u << (8 * r)) - 1u));
    }
    uint32_t cont = 0, l2 = 0, l3 = 0, l4 = 0, inv = 0, ge90 = 0, gea0 = 0, e0 = 0, ed = 0, f0 = 0, f4 = 0;
#pragma unroll
    for (int k = 0; k < 24; ++k) {
        const uint32_t b = v.byte(k);
        const uint32_t c = (b & 0xc0u) == 0x80u;
        cont |= c << k;
        l2 |= (uint32_t)(b >= 0xc0u) << k;
        l3 |= (uint32_t)(b >= 0xe0u) << k;
        l4 |= (uint32_t)(b >= 0xf0u) << k;
        inv |= (uint32_t)(b == 0xc0u || b == 0xc1u || b >= 0xf5u) << k;
        ge90 |= (uint32_t)(c && b >= 0x90u) << k;
        gea0 |= (uint32_t)(c && b >= 0xa0u) << k;
        e0 |= (uint32_t)(b == 0xe0u) << k;
        ed |= (uint32_t)(b == 0xedu) << k;
        f0 |= (uint32_t)(b == 0xf0u) << k;
        f4 |= (uint32_t)(b == 0xf4u) << k;
    }
    const uint32_t own_bits = k_end >= 20 ? kU8Own : (((1u << k_end) - 1u) & kU8Own);
    uint32_t cut = 0, first = 0;
    if constexpr (BATCH) {
        if (o < n) { // (boff[n_hay] = n > o: the search ends inside the table)
            uint32_t hi = n_hay;
            const uint32_t from = LOSSY && o ? o - 3u : o;
            while (first < hi) {
                const uint32_t mid = first + ((hi - first) >> 1);
                if (boff[mid] < from) first = mid + 1;
                else hi = mid;
            }
            if constexpr (LOSSY)
                for (; boff[first] < o; ++first) cut |= 1u << (boff[first] + 4u - o); // (bits 1..3; ends: boff[n_hay] = n > o)
            for (uint32_t j = first; j <= n_hay; ++j) {
                const uint32_t q = boff[j] - o;
                if (q >= 20u) break;
                cut |= 1u << (q + 4u);
            }
        }
    }
    v.cut = cut;
    v.next = first;
    // a lead validates its own sequence: the bytes it needs are continuation bytes, the second one in the range its lead allows
    // (E0: A0..BF, no overlong form; ED: 80..9F, no surrogate; F0: 90..BF; F4: 80..8F, nothing above U+10FFFF)
    const uint32_t bad_lead = inv | (l2 & ~(cont >> 1)) | (l3 & ~(cont >> 2)) | (l4 & ~(cont >> 3)) | (e0 & ~(gea0 >> 1)) | (ed & (gea0 >> 1)) |
                              (f0 & ~(ge90 >> 1)) | (f4 & (ge90 >> 1)) | (l2 & (cut >> 1)) | (l3 & (cut >> 2)) | (l4 & (cut >> 3));
    // a continuation byte is claimed when the nearest byte before it that is none is a lead long enough to reach it
    const uint32_t claimed = (l2 << 1) | ((l3 << 2) & (cont << 1)) | ((l4 << 3) & (cont << 2) & (cont << 1));
    v.lead = ~cont & own_bits;
    v.four = l4 & own_bits;
    v.bad = (bad_lead | (cont & (~claimed | cut))) & own_bits;
    v.tail = 0;
    if constexpr (LOSSY) {
        const uint32_t second = (cont >> 1) & ~(e0 & ~(gea0 >> 1)) & ~(ed & (gea0 >> 1)) & ~(f0 & ~(ge90 >> 1)) & ~(f4 & (ge90 >> 1));
        const uint32_t c1 = l2 & ~inv & second & ~(cut >> 1);  // leads that claim the byte behind them
        const uint32_t c2 = c1 & l3 & (cont >> 2) & ~(cut >> 2); // ... and the second
        const uint32_t c3 = c2 & l4 & (cont >> 3) & ~(cut >> 3); // ... and the third
        const uint32_t claimed_lossy = (c1 << 1) | (c2 << 2) | (c3 << 3);
        const uint32_t whole = (c1 & ~l3) | (c2 & ~l4) | c3; // leads that claimed all they need
        const uint32_t bad_lossy = l2 & ~whole;
        v.lead = (~cont | (cont & ~claimed_lossy)) & own_bits;
        v.four = l4 & ~bad_lossy & own_bits;
        v.bad = (bad_lossy | (cont & ~claimed_lossy)) & own_bits;
        if constexpr (OPEN) {
            // the lead whose claim reaches the buffer's end while it still needs more: a 2..4-byte lead as the last byte, a 3- or
            // 4-byte lead that claimed the last byte, a 4-byte lead that claimed the last two (behind the end the window reads as
            // zero, which nobody claims: c1 of the last byte and c2 of the last two are 0, so the three terms exclude each other)
            const uint32_t behind = k_end >= 24 ? 0u : ~((1u << k_end) - 1u);
            v.tail = ((l2 & ~inv & (behind >> 1)) | (c1 & l3 & (behind >> 2)) | (c2 & l4 & (behind >> 3))) & own_bits;
            v.lead &= ~v.tail; // the held prefix's lead begins no unit of THIS buffer ...
            v.bad &= ~v.tail;  // ... and is no replaced one: it did not claim all it needs YET (four: clear already, it is in bad_lossy)
        }
    }
    if constexpr (OPEN && !LOSSY) {
        // `behind`: the window's bytes at and behind the buffer's end -- they are not there YET, so whatever a lead asks of them holds
        // (what a lead forbids, ED A0.. and F4 90.., is asked of bytes that are there: the plain masks, zero behind the end)
        const uint32_t behind = k_end >= 24 ? 0u : ~((1u << k_end) - 1u);
        const uint32_t cont_o = cont | behind, gea0_o = gea0 | behind, ge90_o = ge90 | behind;
        // (ED A0..BF as the buffer's LAST two bytes is held all the same, as CPython's incremental decoder holds it -- "a truncated
        // surrogate" -- although no third byte can complete it: the next buffer, or the end, reports it, at the same lead)
        const uint32_t bad_open = inv | (l2 & ~(cont_o >> 1)) | (l3 & ~(cont_o >> 2)) | (l4 & ~(cont_o >> 3)) | (e0 & ~(gea0_o >> 1)) |
                                  (ed & (gea0 >> 1) & ~(behind >> 2)) | (f0 & ~(ge90_o >> 1)) | (f4 & (ge90 >> 1));
        v.tail = ((l2 & (behind >> 1)) | (l3 & (behind >> 2)) | (l4 & (behind >> 3))) & ~bad_open & own_bits;
        v.lead &= ~v.tail; // the held prefix's lead begins no unit of THIS buffer
        v.four &= ~v.tail;
        v.bad = (bad_open | (cont & ~claimed)) & own_bits;
    }
    return v;
}

// exclusive scan over the workgroup's 256 threads; *total = the sum
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *total) {
    __shared__ uint32_t wave_sum[kU8Threads / kWave];
    const uint32_t inc = wave_inclusive_scan(v);
    const uint32_t wave = threadIdx.x / kWave;
    __syncthreads(); // (the sums of a scan before this one have been read)
    if (lane_id() == kWave - 1) wave_sum[wave] = inc;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < kU8Threads / kWave; ++i) {
        base += i < wave ? wave_sum[i] : 0u;
        sum += wave_sum[i];
    }
    *total = sum;
    return base + inc - v;
}

// The body of the three count kernels, one per form of lane_view.  res[1]: the smallest offending offset (preset to ~0);
// block_sums[b] = the units of block b's bytes.  OPEN: res[2] (preset to 0) = the bytes at the buffer's end that begin a sequence
// a later buffer has to complete, 1 .. 3, and the sums are those of the n - res[2] bytes before them.
// LOSSY: res[1] is the first REPLACED offset, and res[3] (preset to 0) the number of replaced units: one 64-bit add per wave that
// has any.  LOSSY and OPEN: all four -- res[0] the units, res[1] the first replaced offset and res[3] the replaced units of the
// n - res[2] bytes before the held prefix (its lead is in neither v.bad nor v.lead), res[2] the held bytes.
template <bool BATCH, bool OPEN, bool LOSSY = false>
__device__ __forceinline__ void count_units(const uint8_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ boff, uint32_t n_hay,
                                            uint32_t *__restrict__ block_sums, unsigned long long *__restrict__ res) {
    const uint32_t o = (blockIdx.x * kU8Threads + threadIdx.x) * kU8Lane;
    const LaneView v = lane_view<BATCH, OPEN, LOSSY>(in, n, o, boff, n_hay);
    // lanes are contiguous: the first lane of a wave that saw something holds the wave's smallest offset
    const unsigned long long offenders = __ballot(v.bad != 0);
    if (offenders && lane_id() == (uint32_t)__ffsll((long long)offenders) - 1)
        atomicMin(res + 1, (unsigned long long)(o - 4 + (uint32_t)__ffs((int)v.bad) - 1));
    if constexpr (LOSSY)
        if (offenders) { // (wave-uniform)
            const uint32_t replaced = wave_inclusive_scan((uint32_t)__popc(v.bad));
            if (lane_id() == kWave - 1) atomicAdd(res + 3, (unsigned long long)replaced);
        }
    if constexpr (OPEN)
        if (v.tail) res[2] = (unsigned long long)(n - (o - 4 + (uint32_t)__ffs((int)v.tail) - 1));
    uint32_t total;
    (void)block_scan(v.units(), &total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kU8Threads) void k_utf8_count(const uint8_t *__restrict__ in, uint32_t n, uint32_t *__restrict__ block_sums,
                                                           unsigned long long *__restrict__ res) {
    count_units<false, false>(in, n, nullptr, 0, block_sums, res);
}

// ... over a buffer whose text goes on behind it (lane_view's OPEN form)
__global__ __launch_bounds__(kU8Threads) void k_utf8_open_count(const uint8_t *__restrict__ in, uint32_t n, uint32_t *__restrict__ block_sums,
                                                                unsigned long long *__restrict__ res) {
    count_units<false, true>(in, n, nullptr, 0, block_sums, res);
}

// ... over a batch: the same sums (units of the buffer read as one text, separators not counted), the cut-aware validation
__global__ __launch_bounds__(kU8Threads) void k_utf8_batch_count(const uint8_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ boff,
                                                                 uint32_t n_hay, uint32_t *__restrict__ block_sums, unsigned long long *__restrict__ res) {
    count_units<true, false>(in, n, boff, n_hay, block_sums, res);
}

// ... that refuse nothing (lane_view's LOSSY form): a text's, a batch's
__global__ __launch_bounds__(kU8Threads) void k_utf8_lossy_count(const uint8_t *__restrict__ in, uint32_t n, uint32_t *__restrict__ block_sums,
                                                                 unsigned long long *__restrict__ res) {
    count_units<false, false, true>(in, n, nullptr, 0, block_sums, res);
}
// ... of a text that goes on behind the buffer (lane_view's LOSSY and OPEN form): the held prefix is neither counted nor replaced
__global__ __launch_bounds__(kU8Threads) void k_utf8_lossy_open_count(const uint8_t *__restrict__ in, uint32_t n, uint32_t *__restrict__ block_sums,
                                                                      unsigned long long *__restrict__ res) {
    count_units<false, true, true>(in, n, nullptr, 0, block_sums, res);
}
__global__ __launch_bounds__(kU8Threads) void k_utf8_lossy_batch_count(const uint8_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ boff,
                                                                       uint32_t n_hay, uint32_t *__restrict__ block_sums,
                                                                       unsigned long long *__restrict__ res) {
    count_units<true, false, true>(in, n, boff, n_hay, block_sums, res);
}

// one workgroup, 256 block sums a round with a running carry (at most 2^19 blocks: 2048 rounds): block_sums become exclusive
// -- the blocks' first unit indices -- and res[0] = their total
__global__ __launch_bounds__(kU8Threads) void k_utf8_scan(uint32_t *__restrict__ block_sums, uint32_t n_blocks, unsigned long long *__restrict__ res) {
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += kU8Threads) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t c = i < n_blocks ? block_sums[i] : 0u;
        uint32_t total;
        const uint32_t ex = carry + block_scan(c, &total);
        if (i < n_blocks) block_sums[i] = ex;
        carry += total;
    }
    if (threadIdx.x == 0) res[0] = carry;
}

// The lane's 16 bytes are ASCII and `dst`, where their units go, is 16-byte aligned: two vector stores.  u: the index of the
// first of them among the units that the checkpoints count, o: the lane's first byte.
__device__ __forceinline__ void store_ascii16(const LaneView &v, uint16_t *__restrict__ dst, uint32_t u, uint32_t o, uint32_t *__restrict__ ckpt) {
    uint32_t p[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t x = v.w[1 + j];
        p[2 * j] = (x & 0xffu) | ((x & 0xff00u) << 8);
        p[2 * j + 1] = ((x >> 16) & 0xffu) | ((x >> 8) & 0xff0000u);
    }
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    d4[0] = make_uint4(p[0], p[1], p[2], p[3]);
    d4[1] = make_uint4(p[4], p[5], p[6], p[7]);
    const uint32_t m = (0u - u) & 31u; // the first of the lane's units whose index is a multiple of 32
    if (ckpt && m < kU8Lane) ckpt[(u + m) >> 5] = o + m;
}

// The lead at bit k of the lane's window, byte `pos` of the buffer: decodes its code point, stores its one or two units at dst,
// and the checkpoint of whichever of them has an index that is a multiple of 32 -- u is the index of the first, among the units
// that the checkpoints count.  Returns the number of units.  LOSSY: a replaced start (v.bad) is one unit, U+FFFD.
template <bool LOSSY = false>
__device__ __forceinline__ uint32_t store_lead(const LaneView &v, int k, uint32_t pos, uint16_t *__restrict__ dst, uint32_t u, uint32_t *__restrict__ ckpt) {
    const uint32_t b0 = v.byte(k), b1 = v.byte(k + 1) & 0x3fu, b2 = v.byte(k + 2) & 0x3fu, b3 = v.byte(k + 3) & 0x3fu;
    if (ckpt && (u & 31u) == 0) ckpt[u >> 5] = pos;
    if constexpr (LOSSY)
        if ((v.bad >> k) & 1u) {
            dst[0] = (uint16_t)0xfffdu;
            return 1;
        }
    if (b0 < 0xf0u) {
        const uint32_t cp = b0 < 0x80u ? b0 : (b0 < 0xe0u ? ((b0 & 0x1fu) << 6) | b1 : ((b0 & 0x0fu) << 12) | (b1 << 6) | b2);
        dst[0] = (uint16_t)cp;
        return 1;
    }
    const uint32_t cp = (((b0 & 0x07u) << 18) | (b1 << 12) | (b2 << 6) | b3) - 0x10000u;
    dst[0] = (uint16_t)(0xd800u + (cp >> 10));
    dst[1] = (uint16_t)(0xdc00u + (cp & 0x3ffu));
    if (ckpt && ((u + 1) & 31u) == 0) ckpt[(u + 1) >> 5] = pos | kCkptLow;
    return 2;
}

// The text is known to be well-formed.  out: n_units units; ckpt: one word per 32 units, or nullptr (an all-ASCII text needs none).
//
// LOSSY (nothing is known about the text; `starts` given): the START BITMAP as well, one bit per byte, set where a sequence or a
// subpart begins -- what locate's lossy form walks.  Every lane of the grid stores the 16 bits of its own bytes with one 2-byte
// store, lanes behind the text zeros: the bitmap has 512 bytes per block, and no bit at or behind n is set.
template <bool LOSSY>
__device__ __forceinline__ void write_units(const uint8_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ block_base, uint16_t *__restrict__ out,
                                            uint32_t n_units, uint32_t *__restrict__ ckpt, uint16_t *__restrict__ starts) {
    const uint32_t o = (blockIdx.x * kU8Threads + threadIdx.x) * kU8Lane;
    const LaneView v = lane_view<false, false, LOSSY>(in, n, o);
    const uint32_t cnt = v.units();
    uint32_t total;
    uint32_t u = block_base[blockIdx.x] + block_scan(cnt, &total);
    if constexpr (LOSSY)
        if (starts) starts[o / kU8Lane] = (uint16_t)(v.lead >> 4);
    if (!cnt || u + cnt > n_units) return; // (the second: never, the counts are those of k_utf8_count)
    if (v.lead == kU8Own && !v.four && cnt == kU8Lane && ((v.w[1] | v.w[2] | v.w[3] | v.w[4]) & 0x80808080u) == 0 && (u & 7u) == 0) {
        store_ascii16(v, out + u, u, o, ckpt); // (their units begin on a 16-byte boundary of the output)
        return;
    }
#pragma unroll
    for (int k = 4; k < 20; ++k)
        if ((v.lead >> k) & 1u) u += store_lead<LOSSY>(v, k, o + (uint32_t)(k - 4), out + u, u, ckpt);
}

__global__ __launch_bounds__(kU8Threads) void k_utf8_write(const uint8_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ block_base,
                                                           uint16_t *__restrict__ out, uint32_t n_units, uint32_t *__restrict__ ckpt) {
    write_units<false>(in, n, block_base, out, n_units, ckpt, nullptr);
}
__global__ __launch_bounds__(kU8Threads) void k_utf8_lossy_write(const uint8_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ block_base,
                                                                 uint16_t *__restrict__ out, uint32_t n_units, uint32_t *__restrict__ ckpt,
                                                                 uint16_t *__restrict__ starts) {
    write_units<true>(in, n, block_base, out, n_units, ckpt, starts);
}

// k_utf8_write over a batch that is known to be well-formed, haystack by haystack.  out: the text the scan sees, n_units + n_hay
// units: the haystacks' units with `sep` behind every haystack, empty ones included -- the unit of a lead at byte p of haystack h
// goes to (units of bytes[0, p)) + h.  cat_off[j] = (units of bytes[0, boff[j])) + j, the first unit of haystack j in that text;
// the lane that owns byte boff[j] stores it and the separator in front of it, and the lane of the buffer's last byte those of
// the boundaries at the buffer's end (j = n_hay, and the empty haystacks at the end).  Checkpoints are indexed by the unit WITHOUT
// separators -- the table of the buffer read as one text, which is well-formed because every haystack is: the two helpers store
// to out + u + j - 1 and count checkpoints by u.
// LOSSY: as write_units, the start bitmap of the buffer -- the cuts are in it: a byte at a cut is no claimed byte, so it is a start.
template <bool LOSSY>
__device__ __forceinline__ void batch_write_units(const uint8_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ block_base,
                                                  uint16_t *__restrict__ out, uint32_t n_units, uint32_t *__restrict__ ckpt,
                                                  const uint32_t *__restrict__ boff, uint32_t n_hay, uint32_t *__restrict__ cat_off, uint32_t sep,
                                                  uint16_t *__restrict__ starts) {
    const uint32_t o = (blockIdx.x * kU8Threads + threadIdx.x) * kU8Lane;
    const LaneView v = lane_view<true, false, LOSSY>(in, n, o, boff, n_hay);
    const uint32_t cnt = v.units();
    uint32_t total;
    uint32_t u = block_base[blockIdx.x] + block_scan(cnt, &total);
    if constexpr (LOSSY)
        if (starts) starts[o / kU8Lane] = (uint16_t)(v.lead >> 4);
    if (o >= n || u + cnt > n_units) return; // (the second: never, the counts are those of k_utf8_batch_count)
    uint32_t j = v.next;                      // the boundaries [0, j) lie before the byte the lane is at: it is haystack j - 1's
    if (!(v.cut & kU8Own) && o + kU8Lane < n && v.lead == kU8Own && ((v.w[1] | v.w[2] | v.w[3] | v.w[4]) & 0x80808080u) == 0 &&
        ((u + j - 1u) & 7u) == 0) {
        // 16 ASCII bytes of one haystack (j >= 1: byte 0 is a cut) whose units begin on a 16-byte boundary of the output
        store_ascii16(v, out + u + j - 1u, u, o, ckpt);
        return;
    }
#pragma unroll
    for (int k = 4; k < 20; ++k) {
        const uint32_t pos = o + (uint32_t)(k - 4);
        if ((v.cut >> k) & 1u) {
            while (j <= n_hay && boff[j] == pos) { // (several: empty haystacks)
                cat_off[j] = u + j;
                if (j) out[u + j - 1u] = (uint16_t)sep;
                ++j;
            }
        }
        // (j >= 1: a lead is a byte of a haystack, whose boundary has been met)
        if ((v.lead >> k) & 1u) u += store_lead<LOSSY>(v, k, pos, out + u + j - 1u, u, ckpt);
    }
    if (o + kU8Lane >= n) { // the buffer's last lane: u = n_units, what is left are the boundaries at the buffer's end
        while (j <= n_hay) {
            cat_off[j] = u + j;
            if (j) out[u + j - 1u] = (uint16_t)sep;
            ++j;
        }
    }
}

__global__ __launch_bounds__(kU8Threads) void k_utf8_batch_write(const uint8_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ block_base,
                                                                 uint16_t *__restrict__ out, uint32_t n_units, uint32_t *__restrict__ ckpt,
                                                                 const uint32_t *__restrict__ boff, uint32_t n_hay, uint32_t *__restrict__ cat_off,
                                                                 uint32_t sep) {
    batch_write_units<false>(in, n, block_base, out, n_units, ckpt, boff, n_hay, cat_off, sep, nullptr);
}
__global__ __launch_bounds__(kU8Threads) void k_utf8_lossy_batch_write(const uint8_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ block_base,
                                                                       uint16_t *__restrict__ out, uint32_t n_units, uint32_t *__restrict__ ckpt,
                                                                       const uint32_t *__restrict__ boff, uint32_t n_hay, uint32_t *__restrict__ cat_off,
                                                                       uint32_t sep, uint16_t *__restrict__ starts) {
    batch_write_units<true>(in, n, block_base, out, n_units, ckpt, boff, n_hay, cat_off, sep, starts);
}

__device__ __forceinline__ uint32_t seq_len(uint32_t lead) { return lead < 0x80u ? 1u : (lead < 0xe0u ? 2u : (lead < 0xf0u ? 3u : 4u)); }

// a position of the walk over the sequences: p = the byte offset of a lead, u = the index of its first unit
struct SeqPos {
    uint32_t p, u;
};

// THE rule from a unit to its byte: s = the sequence that holds `unit` -- s.p the first byte of its code point; of a low
// surrogate, its pair's -- reached from the checkpoint at or below `unit` by a walk of at most 31 units over the lead bytes.
// resume: s stands at a unit of the same 32 that is not behind `unit`, the walk goes on from there.  Returns the sequence's
// length in bytes.
//
// LOSSY: `in` is the START BITMAP of the buffer instead (k_utf8_lossy_write), no byte is read.  The length of the start at p is
// the distance to the next set bit, clamped to n: 4 for a well-formed 4-byte sequence and for nothing else (a subpart has at most
// 3 bytes), so that is where a start has two units.  Cuts need no thought here: a walk that begins in an earlier haystack passes
// them as starts like any other -- "E2 82 | AC" is two starts, never a euro sign.
__device__ __forceinline__ uint32_t start_len(const uint32_t *__restrict__ starts, uint32_t n, uint32_t p) {
    if (p + 1u >= n) return n - p;
    const uint32_t w = (p + 1u) >> 5, sh = (p + 1u) & 31u;
    const uint32_t lo = starts[w], hi = (sh > 29u && ((w + 1u) << 5) < n) ? starts[w + 1u] : 0u; // (a word behind the text's bits is not read)
    const uint32_t bits = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh) & 7u;                    // the starts at p + 1 .. p + 3
    const uint32_t len = bits ? (uint32_t)__ffs((int)bits) : 4u;
    return len < n - p ? len : n - p;
}

template <bool LOSSY = false>
__device__ __forceinline__ uint32_t locate(const uint8_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ ckpt, uint32_t unit, SeqPos &s,
                                           bool resume = false) {
    if (!resume) {
        const uint32_t c = ckpt[unit >> 5];
        s.p = c & ~kCkptLow;
        s.u = (unit & ~31u) - (c >> 31);
    }
    uint32_t len = 1;
    while (s.p < n) {
        if constexpr (LOSSY) len = start_len(reinterpret_cast<const uint32_t *>(in), n, s.p);
        else len = seq_len(in[s.p]);
        const uint32_t nu = len == 4 ? 2u : 1u;
        if (unit < s.u + nu) break;
        s.u += nu;
        s.p += len;
    }
    return len;
}

// A record's units first .. last of the buffer read as one text (n_units of them, WITHOUT separators) -> *start, the first byte
// of the code point that holds unit first, and *end, one past the last byte of the one that holds unit last (a match has at
// least one unit), both minus `base`: a haystack's first byte, or 0.  A range that is none is left alone (never: the scan's
// records lie inside the text).  ckpt == nullptr: an all-ASCII buffer, where a unit is its byte.  LOSSY: locate's, `in` the bitmap.
template <bool LOSSY = false>
__device__ __forceinline__ void batch_bytes(uint32_t first, uint32_t last, uint32_t base, const uint8_t *__restrict__ in, uint32_t n, uint32_t n_units,
                                            const uint32_t *__restrict__ ckpt, int32_t *start, int32_t *end) {
    if (first > last || last >= n_units) return;
    if (!ckpt) {
        *start = (int32_t)(first - base);
        *end = (int32_t)(last + 1u - base);
        return;
    }
    SeqPos s;
    (void)locate<LOSSY>(in, n, ckpt, first, s);
    *start = (int32_t)(s.p - base);
    const uint32_t len = locate<LOSSY>(in, n, ckpt, last, s, (last >> 5) == (first >> 5));
    *end = (int32_t)(s.p + len - base);
}

// k_batch_tag and the map in one, a lane per record: {start, end[, id]} in units of the batch's text -> {haystack, start, end[, id]}
// in bytes of the haystack
template <int REC, bool LOSSY = false>
__global__ __launch_bounds__(kU8Threads) void k_utf8_batch_tag(const int32_t *__restrict__ recs, uint64_t cnt, const uint32_t *__restrict__ cat_off,
                                                               uint32_t n_hay, const uint32_t *__restrict__ boff, const uint8_t *__restrict__ in, uint32_t n,
                                                               uint32_t n_units, const uint32_t *__restrict__ ckpt, int32_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kU8Threads + threadIdx.x;
    if (i >= cnt) return;
    constexpr int W = REC / 4;
    const uint32_t start = (uint32_t)recs[i * W], end = (uint32_t)recs[i * W + 1];
    const uint32_t h = haystack_of(cat_off, n_hay, start);
    int32_t *o = out + i * (W + 1);
    o[0] = (int32_t)h;
    if (W == 3) o[3] = recs[i * W + 2];
    // (no match holds a separator: both ends are units of haystack h)
    batch_bytes<LOSSY>(start - h, end - 1u - h, boff[h], in, n, n_units, ckpt, o + 1, o + 2);
}

// A lane per record of `cols` words, in place: {start, end} in units of the scan's text -> bytes of the buffer.  The text is a
// batch's (acgpu_replace_batch_utf8) or, n_hay == 0, the buffer's own units (acgpu_match_utf8 and what shares its map): the
// record's haystack h -- 0 then -- is also the number of separators in front of it, so its units in the buffer read as one text
// are start - h .. end - 1 - h.  The bytes are relative to the SPAN's first byte, not the haystack's -- plan and emit work on the
// span, which has no separators.  In an all-ASCII batch the shift is all there is to do -- but it is still to do.
template <bool LOSSY = false>
__global__ __launch_bounds__(kU8Threads) void k_utf8_batch_map(int32_t *__restrict__ recs, uint64_t cnt, uint32_t cols, const uint32_t *__restrict__ cat_off,
                                                               uint32_t n_hay, const uint8_t *__restrict__ in, uint32_t n, uint32_t n_units,
                                                               const uint32_t *__restrict__ ckpt) {
    const uint64_t i = (uint64_t)blockIdx.x * kU8Threads + threadIdx.x;
    if (i >= cnt) return;
    int32_t *r = recs + i * cols;
    const uint32_t start = (uint32_t)r[0], end = (uint32_t)r[1];
    const uint32_t h = haystack_of(cat_off, n_hay, start); // (n_hay == 0: 0, and cat_off is not read)
    batch_bytes<LOSSY>(start - h, end - 1u - h, 0u, in, n, n_units, ckpt, r, r + 1);
}

// One lane: unit x of the scan's text -> *out, a byte of the buffer (a piece's boundary, see replace_limit in acgpu_replace.hip).
// cat_off == nullptr: the text is the buffer's own units, x < n_units, and *out is the first byte of the code point that holds
// unit x -- between the two units of a surrogate pair that rounds down.  Else the text is a batch's, and with h the haystack
// that holds x (cat_off[h] <= x < cat_off[h + 1]):
//  * x is haystack h's separator, the last unit before cat_off[h + 1]: the byte where haystack h + 1 begins, boff[h + 1] -- for
//    the batch's last separator that is n, the span's end.  (The checkpoint table has no entry for a separator: x - h would be
//    the first unit of the next haystack, or n_units.)  A unit at or behind the text's end maps to n as well;
//  * any other unit: as above for unit x - h of the buffer read as one text; all-ASCII (ckpt == nullptr): the byte x - h itself.
// LOSSY: locate's, `in` the start bitmap -- the unit of a replaced subpart is the whole subpart, so *out is its first byte, and
// only a surrogate pair rounds down.
template <bool LOSSY = false>
__global__ void k_utf8_batch_pos(uint32_t x, const uint32_t *__restrict__ cat_off, uint32_t n_hay, const uint32_t *__restrict__ boff,
                                 const uint8_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ ckpt, int64_t *__restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t u = x;
    if (cat_off) {
        if (x >= cat_off[n_hay]) {
            *out = (int64_t)n;
            return;
        }
        const uint32_t h = haystack_of(cat_off, n_hay, x);
        if (x + 1u == cat_off[h + 1u]) {
            *out = (int64_t)boff[h + 1u];
            return;
        }
        u = x - h;
    }
    if (!ckpt) {
        *out = (int64_t)u;
        return;
    }
    SeqPos s;
    (void)locate<LOSSY>(in, n, ckpt, u, s);
    *out = (int64_t)s.p;
}

// ---- VIRTUAL COORDINATES of a batch (acgpu_spans_batch_utf8, acgpu_cover_batch_utf8): v = (byte of the span) +
// (index of the haystack), the caller's bytes with one PHANTOM element behind every haystack.  voff[j] = boff[j] + j is haystack j's
// first element, its phantom stands at voff[j + 1] - 1, and the text has n + n_hay elements.  The map unit -> v is monotone. ----

// A lane per word: voff[j] = boff[j] + j, j <= n_hay
__global__ __launch_bounds__(kU8Threads) void k_utf8_batch_voff(const uint32_t *__restrict__ boff, uint32_t n_words, uint32_t *__restrict__ voff) {
    const uint32_t j = blockIdx.x * kU8Threads + threadIdx.x;
    if (j < n_words) voff[j] = boff[j] + j;
}

// The Set-record form of k_utf8_batch_map for virtual coordinates, a lane per record, in place: {start, end} in units of the
// batch's text -> v.  Both ends are units of the record's haystack h (no match holds a separator), so its bytes are those of
// units start - h .. end - 1 - h of the buffer read as one text, and h is added to both.  (An all-ASCII batch needs no launch:
// there a unit without separators is its byte, and unit - h + h is the unit itself -- utf8_vmap_records.)
template <bool LOSSY = false>
__global__ __launch_bounds__(kU8Threads) void k_utf8_batch_vmap(int32_t *__restrict__ recs, uint64_t cnt, const uint32_t *__restrict__ cat_off, uint32_t n_hay,
                                                                const uint8_t *__restrict__ in, uint32_t n, uint32_t n_units,
                                                                const uint32_t *__restrict__ ckpt) {
    const uint64_t i = (uint64_t)blockIdx.x * kU8Threads + threadIdx.x;
    if (i >= cnt) return;
    int32_t *r = recs + i * 2;
    const uint32_t start = (uint32_t)r[0], end = (uint32_t)r[1];
    const uint32_t h = haystack_of(cat_off, n_hay, start);
    int32_t s = (int32_t)(start - h), e = (int32_t)(end - h); // (what a range that is none keeps: the record as it was)
    batch_bytes<LOSSY>(start - h, end - 1u - h, 0u, in, n, n_units, ckpt, &s, &e);
    r[0] = s + (int32_t)h;
    r[1] = e + (int32_t)h;
}

// The form of k_utf8_batch_pos for virtual coordinates, one lane: unit x of the batch's text -> *out, a v no record that starts at
// or behind unit x starts before (a piece's bound, acgpu_spans.hip).  With h the haystack that holds x:
//  * x is haystack h's separator: ITS OWN PHANTOM, boff[h + 1] + h.  The position behind it, voff[h + 1], would do as well -- a
//    record at or behind unit x starts in haystack h + 1 or later, at or behind voff[h + 1], and nothing starts at a phantom.  The
//    phantom is chosen because it is what the all-ASCII branch computes without a launch (there cat_off == voff and v is the unit,
//    so a separator IS its phantom): both branches then cut a batch's pieces at the same places, and what is tested on the one
//    holds on the other.  The price: a span that ends at the haystack's last byte is carried into the next piece (end < B fails).
//  * a unit at or behind the shard's end: n + n_hay, the text's end;
//  * any other unit: the first byte of the code point (lossy: of the start) that holds unit x - h of the buffer read as one text --
//    between the two units of a surrogate pair that rounds down, as utf8_map_position does -- plus h.
template <bool LOSSY = false>
__global__ void k_utf8_batch_vpos(uint32_t x, const uint32_t *__restrict__ cat_off, uint32_t n_hay, const uint32_t *__restrict__ boff,
                                  const uint8_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ ckpt, int64_t *__restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (x >= cat_off[n_hay]) {
        *out = (int64_t)n + (int64_t)n_hay;
        return;
    }
    const uint32_t h = haystack_of(cat_off, n_hay, x);
    if (x + 1u == cat_off[h + 1u]) {
        *out = (int64_t)boff[h + 1u] + (int64_t)h;
        return;
    }
    SeqPos s;
    (void)locate<LOSSY>(in, n, ckpt, x - h, s);
    *out = (int64_t)s.p + (int64_t)h;
}

// A lane per haystack, behind the last piece of a summary call: the first record of every entry that has one, from units
// relative to its haystack to bytes relative to it.  cat_off given: entry i is haystack i of a batch's text (its first unit
// without separators is cat_off[i] - i, its first byte boff[i]); not given: the entries' one text is `in` itself.
template <bool LOSSY = false>
__global__ __launch_bounds__(kU8Threads) void k_summary_utf8_bytes(acgpu_batch_summary *__restrict__ sum, uint32_t n_entries, const uint32_t *__restrict__ cat_off,
                                                                   const uint32_t *__restrict__ boff, const uint8_t *__restrict__ in, uint32_t n,
                                                                   uint32_t n_units, const uint32_t *__restrict__ ckpt) {
    const uint32_t i = blockIdx.x * kU8Threads + threadIdx.x;
    if (i >= n_entries) return;
    acgpu_batch_summary *e = sum + i;
    if (!e->n_matches || e->start < 0 || e->end <= e->start) return;
    const uint32_t unit0 = cat_off ? cat_off[i] - i : 0u, byte0 = cat_off ? boff[i] : 0u;
    batch_bytes<LOSSY>(unit0 + (uint32_t)e->start, unit0 + (uint32_t)e->end - 1u, byte0, in, n, n_units, ckpt, &e->start, &e->end);
}

} // namespace

namespace acgpu {

// what locate walks from a checkpoint: the bytes, or a lossy text's start bitmap
static const uint8_t *walked(const Utf8Text &text) { return text.lossy ? reinterpret_cast<const uint8_t *>(text.d_starts) : text.d_bytes; }

int utf8_map_records(const Utf8Text &text, const Utf8Batch *b, int32_t *d_recs, uint64_t cnt, uint32_t cols, hipStream_t stream) {
    if (!cnt || (!b && !text.d_ckpt)) return ACGPU_OK; // (a batch is mapped also when it is all ASCII: its records stand behind separators)
    // (lossy: the walk reads the start bitmap where the strict one reads the bytes)
    hipLaunchKernelGGL(text.lossy ? k_utf8_batch_map<true> : k_utf8_batch_map<false>, dim3((unsigned)((cnt + kU8Threads - 1) / kU8Threads)),
                       dim3(kU8Threads), 0, stream, d_recs, cnt, cols, b ? b->d_cat_off : nullptr, b ? b->n_haystacks : 0u, walked(text),
                       (uint32_t)text.n_bytes, (uint32_t)text.n_units, text.d_ckpt);
    HIP_TRY(hipGetLastError());
    return ACGPU_OK;
}

int utf8_map_position(const Utf8Text &text, const Utf8Batch *b, uint64_t unit, int64_t *d_out, hipStream_t stream) {
    if (b ? !b->d_cat_off || !b->n_haystacks || unit >= (1ull << 32)
          : !text.d_ckpt || unit >= text.n_units) // (a checkpoint is written for the text's units only)
        return ACGPU_E_INVALID;
    // (lossy: the walk reads the start bitmap; without checkpoints -- an all-ASCII batch, or one with as many units as bytes --
    // neither is read)
    hipLaunchKernelGGL(text.lossy ? k_utf8_batch_pos<true> : k_utf8_batch_pos<false>, dim3(1), dim3(1), 0, stream, (uint32_t)unit,
                       b ? b->d_cat_off : nullptr, b ? b->n_haystacks : 0u, b ? b->d_boff : nullptr, walked(text), (uint32_t)text.n_bytes, text.d_ckpt,
                       d_out);
    HIP_TRY(hipGetLastError());
    return ACGPU_OK;
}

int utf8_virtual_offsets(DeviceState &d, const Utf8Batch &b, hipStream_t stream, std::vector<uint32_t> *h_voff, const uint32_t **d_voff) {
    const uint32_t n_words = b.n_haystacks + 1u;
    try {
        h_voff->resize(n_words);
    } catch (...) {
        return ACGPU_E_NOMEM;
    }
    for (uint32_t j = 0; j < n_words; j++) (*h_voff)[j] = b.h_boff[j] + j;
    const int rc = d.utf8_voff.ensure((size_t)n_words * 4 + 16);
    if (rc) return rc;
    uint32_t *voff = reinterpret_cast<uint32_t *>(d.utf8_voff.p);
    hipLaunchKernelGGL(k_utf8_batch_voff, dim3((n_words + kU8Threads - 1) / kU8Threads), dim3(kU8Threads), 0, stream, b.d_boff, n_words, voff);
    HIP_TRY(hipGetLastError());
    *d_voff = voff;
    return ACGPU_OK;
}

int utf8_vmap_records(const Utf8Batch &b, int32_t *d_recs, uint64_t cnt, hipStream_t stream) {
    // an all-ASCII batch: a record's start and end are v as they are -- a unit of haystack h stands h separators behind its byte,
    // and v adds those h back.  Nothing is to do, so nothing is launched.
    if (!cnt || !b.text.d_ckpt) return ACGPU_OK;
    hipLaunchKernelGGL(b.text.lossy ? k_utf8_batch_vmap<true> : k_utf8_batch_vmap<false>, dim3((unsigned)((cnt + kU8Threads - 1) / kU8Threads)),
                       dim3(kU8Threads), 0, stream, d_recs, cnt, b.d_cat_off, b.n_haystacks, walked(b.text), (uint32_t)b.text.n_bytes,
                       (uint32_t)b.text.n_units, b.text.d_ckpt);
    HIP_TRY(hipGetLastError());
    return ACGPU_OK;
}

int utf8_vmap_position(const Utf8Batch &b, uint64_t unit, int64_t *d_out, hipStream_t stream) {
    if (!b.d_cat_off || !b.n_haystacks || !b.text.d_ckpt || unit >= (1ull << 32)) return ACGPU_E_INVALID;
    hipLaunchKernelGGL(b.text.lossy ? k_utf8_batch_vpos<true> : k_utf8_batch_vpos<false>, dim3(1), dim3(1), 0, stream, (uint32_t)unit, b.d_cat_off,
                       b.n_haystacks, b.d_boff, walked(b.text), (uint32_t)b.text.n_bytes, b.text.d_ckpt, d_out);
    HIP_TRY(hipGetLastError());
    return ACGPU_OK;
}

namespace {

// What the front ends keep on the device around the scan's text: the caller's bytes in d.utf8_in, with room for a lane's 16-byte
// load and the 4 bytes behind it, and in d.utf8_aux, each part 64-byte aligned,
//   [n_units, first_bad, tail, n_replaced | block sums | checkpoints, one per 32 units of a text that has at most n units |
//    a batch's byte offsets | lossy: the start bitmap, 512 bytes per block]
struct Utf8Aux {
    uint32_t n = 0, n_blocks = 0; // the buffer's bytes, and its blocks of 4096
    const uint8_t *in = nullptr;
    unsigned long long *res = nullptr;
    uint32_t *sums = nullptr, *ckpt = nullptr, *boff = nullptr; // boff: n_off words
    uint16_t *starts = nullptr;                                  // lossy: 16 bits per lane of the write kernel's grid
    int ensure(DeviceState &d, uint32_t n_bytes, size_t n_off = 0, bool lossy = false) {
        auto up64 = [](size_t x) { return (x + 63) & ~(size_t)63; };
        n = n_bytes;
        n_blocks = (n + kU8Block - 1) / kU8Block;
        const size_t sums_off = 64, ckpt_off = sums_off + up64((size_t)n_blocks * 4), boff_off = ckpt_off + up64(((size_t)n / 32 + 1) * 4);
        int rc;
        if ((rc = d.utf8_in.ensure((size_t)n + 64))) return rc;
        const size_t starts_off = boff_off + up64(n_off * 4);
        if ((rc = d.utf8_aux.ensure(lossy ? starts_off + (size_t)n_blocks * (kU8Block / 8) : boff_off + n_off * 4))) return rc;
        char *aux = (char *)d.utf8_aux.p;
        in = reinterpret_cast<const uint8_t *>(d.utf8_in.p);
        res = reinterpret_cast<unsigned long long *>(aux);
        sums = reinterpret_cast<uint32_t *>(aux + sums_off);
        ckpt = reinterpret_cast<uint32_t *>(aux + ckpt_off);
        boff = reinterpret_cast<uint32_t *>(aux + boff_off);
        starts = lossy ? reinterpret_cast<uint16_t *>(aux + starts_off) : nullptr;
        return ACGPU_OK;
    }
};

// The validate phase of both front ends, behind the copies: the result words preset, the count kernel of the buffer's form
// (n_hay != 0: a batch with its offsets in x.boff; open: a text that goes on), the scan of the block sums, and the one wait this
// front end adds -- the shard cannot be sized, nor the scan begun, before the text is known to be well-formed.  Fills in
// n_units, first_bad, tail, n_bytes (the bytes before the held prefix), d_bytes and d_ckpt, the table the write kernel is to fill.
// errors == replace: the lossy count kernels, n_replaced with the rest in the one wait, and the call goes on whatever they saw;
// d_starts with d_ckpt, the bitmap the write kernel is to fill.  Open as well: the held prefix comes in the same 32 bytes.
int utf8_validate(const Utf8Aux &x, uint32_t n_hay, bool open, Utf8Errors errors, hipStream_t stream, Utf8Text *text) {
    const dim3 grid(x.n_blocks), block(kU8Threads);
    const bool lossy = errors == Utf8Errors::replace;
    HIP_TRY(hipMemsetAsync(x.res, 0xff, 16, stream));
    if (lossy) {
        HIP_TRY(hipMemsetAsync(x.res + 3, 0, 8, stream));
        if (n_hay)
            hipLaunchKernelGGL(k_utf8_lossy_batch_count, grid, block, 0, stream, x.in, x.n, (const uint32_t *)x.boff, n_hay, x.sums, x.res);
        else if (open) {
            HIP_TRY(hipMemsetAsync(x.res + 2, 0, 8, stream));
            hipLaunchKernelGGL(k_utf8_lossy_open_count, grid, block, 0, stream, x.in, x.n, x.sums, x.res);
        } else
            hipLaunchKernelGGL(k_utf8_lossy_count, grid, block, 0, stream, x.in, x.n, x.sums, x.res);
    } else if (n_hay) {
        hipLaunchKernelGGL(k_utf8_batch_count, grid, block, 0, stream, x.in, x.n, (const uint32_t *)x.boff, n_hay, x.sums, x.res);
    } else if (open) {
        HIP_TRY(hipMemsetAsync(x.res + 2, 0, 8, stream));
        hipLaunchKernelGGL(k_utf8_open_count, grid, block, 0, stream, x.in, x.n, x.sums, x.res);
    } else {
        hipLaunchKernelGGL(k_utf8_count, grid, block, 0, stream, x.in, x.n, x.sums, x.res);
    }
    hipLaunchKernelGGL(k_utf8_scan, dim3(1), block, 0, stream, x.sums, x.n_blocks, x.res);
    HIP_TRY(hipGetLastError());
    unsigned long long h_res[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h_res, x.res, lossy ? 32 : (open ? 24 : 16), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream)); // (what the copies in front read on the host has been read by now, too)
    text->n_units = h_res[0];
    text->first_bad = (int64_t)h_res[1];
    text->lossy = lossy;
    if (lossy) {
        if (!open) h_res[2] = 0; // (no held prefix; the word was not preset)
        text->n_replaced = h_res[3];
        if ((text->first_bad >= 0) != (text->n_replaced != 0) || text->n_replaced > x.n) return ACGPU_E_HIP; // (never)
    } else if (text->first_bad >= 0) {
        return ACGPU_E_ENCODING;
    }
    if (h_res[2] > 3 || h_res[2] > x.n) return ACGPU_E_HIP; // (never: a held prefix is one to three bytes of the buffer)
    text->tail = (uint32_t)h_res[2];
    // the text that is transcoded: the bytes before the held prefix -- they end where a sequence ends, well-formed on their own
    text->n_bytes = x.n - text->tail;
    if (text->n_units > text->n_bytes) return ACGPU_E_HIP; // (never: a sequence has no more units than bytes)
    text->d_bytes = x.in;
    // an all-ASCII text needs none -- nor does a lossy text with as many units as bytes: then every start is one byte and one unit
    // ("a\x80b"), the map is the identity, and no bitmap is written either
    text->d_ckpt = text->n_units == text->n_bytes ? nullptr : x.ckpt;
    text->d_starts = lossy && text->d_ckpt ? reinterpret_cast<const uint32_t *>(x.starts) : nullptr;
    return ACGPU_OK;
}

// the scan's text behind the write kernel: d.stage_hay as one shard, all of it owned, the text's begin and end, no chain
void whole_shard(const DeviceState &d, uint64_t n_units, acgpu_shard *sh) {
    sh->d_hay = (const uint16_t *)d.stage_hay.p;
    sh->n_units = sh->own_end = n_units;
    sh->text_begin = sh->text_end = 1;
}

} // namespace

int stage_utf8_text(DeviceState &d, const uint8_t *bytes, uint64_t n_bytes, hipStream_t stream, Utf8Text *out, Utf8Errors errors) {
    return stage_utf8_parts(d, nullptr, 0, bytes, n_bytes, /*open=*/false, stream, out, errors);
}

int stage_utf8_parts(DeviceState &d, const uint8_t *head, uint64_t n_head, const uint8_t *bytes, uint64_t n_rest, bool open, hipStream_t stream,
                     Utf8Text *out, Utf8Errors errors) {
    *out = Utf8Text{};
    out->n_bytes = n_head + n_rest;
    const bool lossy = errors == Utf8Errors::replace;
    Utf8Aux x;
    int rc;
    if ((rc = x.ensure(d, (uint32_t)(n_head + n_rest), 0, lossy))) return rc;
    if (n_head) HIP_TRY(hipMemcpyAsync(d.utf8_in.p, head, n_head, hipMemcpyHostToDevice, stream));
    if (n_rest) HIP_TRY(hipMemcpyAsync((char *)d.utf8_in.p + n_head, bytes, n_rest, hipMemcpyHostToDevice, stream));
    if ((rc = utf8_validate(x, 0, open, errors, stream, out))) return rc;
    if ((rc = d.stage_hay.ensure(out->n_units * 2 + 16))) return rc;
    const uint32_t n_text = (uint32_t)out->n_bytes, n_text_blocks = (n_text + kU8Block - 1) / kU8Block;
    if (lossy && n_text_blocks) // (n_text <= n: the grid is at most the one the bitmap was sized for, and no word behind n_text's is read)
        hipLaunchKernelGGL(k_utf8_lossy_write, dim3(n_text_blocks), dim3(kU8Threads), 0, stream, x.in, n_text, (const uint32_t *)x.sums,
                           reinterpret_cast<uint16_t *>(d.stage_hay.p), (uint32_t)out->n_units, out->d_ckpt ? x.ckpt : nullptr,
                           out->d_starts ? x.starts : nullptr);
    else if (!lossy && n_text_blocks) // (a buffer that is a held prefix and nothing else has no unit to write)
        hipLaunchKernelGGL(k_utf8_write, dim3(n_text_blocks), dim3(kU8Threads), 0, stream, x.in, n_text, (const uint32_t *)x.sums,
                           reinterpret_cast<uint16_t *>(d.stage_hay.p), (uint32_t)out->n_units, out->d_ckpt ? x.ckpt : nullptr);
    HIP_TRY(hipGetLastError());
    whole_shard(d, out->n_units, &out->shard);
    return ACGPU_OK;
}

int stage_utf8_batch(DeviceState &d, const HostTables &t, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_hay, hipStream_t stream,
                     Utf8Batch *out, bool validate_only, Utf8Errors errors) {
    *out = Utf8Batch{};
    out->n_haystacks = n_hay;
    const uint32_t n = (uint32_t)(offsets[n_hay] - offsets[0]);
    out->text.n_bytes = n;
    const size_t off_bytes = ((size_t)n_hay + 1) * 4;
    Utf8Aux x;
    int rc;
    const bool lossy = errors == Utf8Errors::replace;
    if ((rc = x.ensure(d, n, (size_t)n_hay + 1, lossy))) return rc;
    if ((rc = d.batch_off.ensure(off_bytes + 16))) return rc;
    std::vector<uint32_t> &h_boff = out->h_boff;
    try {
        h_boff.resize((size_t)n_hay + 1);
    } catch (...) {
        return ACGPU_E_NOMEM;
    }
    for (uint32_t i = 0; i <= n_hay; i++) h_boff[i] = (uint32_t)(offsets[i] - offsets[0]);
    HIP_TRY(hipMemcpyAsync(d.utf8_in.p, bytes + offsets[0], n, hipMemcpyHostToDevice, stream)); // the caller's span as it lies: one copy
    HIP_TRY(hipMemcpyAsync(x.boff, h_boff.data(), off_bytes, hipMemcpyHostToDevice, stream));
    rc = utf8_validate(x, n_hay, /*open=*/false, errors, stream, &out->text);
    if (rc == ACGPU_E_ENCODING || (rc == ACGPU_OK && out->text.first_bad >= 0)) { // (the second: a lossy batch that had something replaced)
        // the haystack that holds byte p: the LAST j < n_hay with offset <= p (of several at one byte all but the last are empty)
        const uint32_t p = (uint32_t)out->text.first_bad;
        const uint32_t j = (uint32_t)(std::upper_bound(h_boff.begin(), h_boff.begin() + n_hay, p) - h_boff.begin()) - 1u;
        out->bad_haystack = j;
        out->text.first_bad = (int64_t)(p - h_boff[j]);
    }
    if (rc) return rc;
    out->d_boff = x.boff;
    if (validate_only) {
        out->text.d_ckpt = nullptr; // (no table is written)
        out->text.d_starts = nullptr;
        return ACGPU_OK;
    }
    const uint64_t cat = out->text.n_units + n_hay;
    uint32_t *d_cat_off = reinterpret_cast<uint32_t *>(d.batch_off.p);
    if ((rc = d.stage_hay.ensure(cat * 2 + 16))) return rc;
    if (lossy)
        hipLaunchKernelGGL(k_utf8_lossy_batch_write, dim3(x.n_blocks), dim3(kU8Threads), 0, stream, x.in, n, (const uint32_t *)x.sums,
                           reinterpret_cast<uint16_t *>(d.stage_hay.p), (uint32_t)out->text.n_units, out->text.d_ckpt ? x.ckpt : nullptr,
                           (const uint32_t *)x.boff, n_hay, d_cat_off, (uint32_t)(uint16_t)t.sep_unit, out->text.d_starts ? x.starts : nullptr);
    else
        hipLaunchKernelGGL(k_utf8_batch_write, dim3(x.n_blocks), dim3(kU8Threads), 0, stream, x.in, n, (const uint32_t *)x.sums,
                           reinterpret_cast<uint16_t *>(d.stage_hay.p), (uint32_t)out->text.n_units, out->text.d_ckpt ? x.ckpt : nullptr,
                           (const uint32_t *)x.boff, n_hay, d_cat_off, (uint32_t)(uint16_t)t.sep_unit);
    HIP_TRY(hipGetLastError());
    whole_shard(d, cat, &out->text.shard);
    out->d_cat_off = d_cat_off;
    return ACGPU_OK;
}

int utf8_batch_tag(const Utf8Batch &b, const void *d_recs, uint64_t cnt, int record_kind, void *d_out, hipStream_t stream) {
    if (!cnt) return ACGPU_OK;
    if (!b.text.d_ckpt) {
        HIP_TRY(launch_batch_tag(d_recs, cnt, record_kind, b.d_cat_off, b.n_haystacks, d_out, stream));
        return ACGPU_OK;
    }
    const dim3 grid((unsigned)((cnt + kU8Threads - 1) / kU8Threads)), block(kU8Threads);
    const uint32_t n = (uint32_t)b.text.n_bytes, n_units = (uint32_t)b.text.n_units;
    const bool set = record_kind == ACGPU_REC_SET;
    const auto kernel = b.text.lossy ? (set ? k_utf8_batch_tag<ACGPU_REC_SET, true> : k_utf8_batch_tag<ACGPU_REC_MAP, true>)
                                     : (set ? k_utf8_batch_tag<ACGPU_REC_SET, false> : k_utf8_batch_tag<ACGPU_REC_MAP, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, (const int32_t *)d_recs, cnt, b.d_cat_off, b.n_haystacks, b.d_boff, walked(b.text), n, n_units,
                       b.text.d_ckpt, (int32_t *)d_out);
    HIP_TRY(hipGetLastError());
    return ACGPU_OK;
}

int utf8_summary_bytes(const Utf8Batch *b, const Utf8Text &text, acgpu_batch_summary *d_sum, uint32_t n_entries, hipStream_t stream) {
    if (!text.d_ckpt || !n_entries) return ACGPU_OK;
    hipLaunchKernelGGL(text.lossy ? k_summary_utf8_bytes<true> : k_summary_utf8_bytes<false>, dim3((n_entries + kU8Threads - 1) / kU8Threads),
                       dim3(kU8Threads), 0, stream, d_sum, n_entries, b ? b->d_cat_off : nullptr, b ? b->d_boff : nullptr, walked(text),
                       (uint32_t)text.n_bytes, (uint32_t)text.n_units, text.d_ckpt);
    HIP_TRY(hipGetLastError());
    return ACGPU_OK;
}

} // namespace acgpu

namespace {

// The body of acgpu_match_utf8 and acgpu_match_utf8_lossy.  P (acgpu_host.h): how the text is staged, and the entry's stats.
template <class P>
int match_utf8(const acgpu_automaton *ca, const uint8_t *bytes, uint64_t n_bytes, int record_kind, void *out, uint64_t cap, uint64_t *n_out,
               typename P::Stats *stats) {
    if (!ca || !n_out || (n_bytes && !bytes) || (cap && !out)) return ACGPU_E_INVALID;
    if (record_kind != ACGPU_REC_SET && record_kind != ACGPU_REC_MAP) return ACGPU_E_INVALID;
    if (n_bytes >= (1ull << 31)) return ACGPU_E_INVALID;
    *n_out = 0;
    if (stats) *stats = P::stats();
    if (n_bytes == 0) return ACGPU_OK; // (nothing to decode and nothing to find: no device needed)
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    PoolCall call(a);
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    int rc;
    if ((rc = call.idle())) return rc; // (the NULL stream: see the stream rule)
    const hipStream_t stream = d.call_stream;
    Utf8Text text;
    rc = stage_utf8_text(d, bytes, n_bytes, stream, &text, P::errors);
    if (rc && rc != ACGPU_E_ENCODING) return call.fail(rc);
    if (stats) *stats = P::stats(&text, rc);
    if (rc) return rc; // (ACGPU_E_ENCODING.  The stream is idle: the pool is as usable as before the call)
    if ((rc = d.stage_out.ensure(cap * (uint64_t)record_kind + 16))) return call.fail(rc);
    rc = match_shard(a, d, &text.shard, record_kind, d.stage_out.p, cap, n_out, stream, nullptr);
    if (rc != ACGPU_OK) return rc; // (ACGPU_E_OVERFLOW: *n_out is the capacity to call again with)
    if (!*n_out) return ACGPU_OK;
    if ((rc = utf8_map_records(text, nullptr, reinterpret_cast<int32_t *>(d.stage_out.p), *n_out, (uint32_t)record_kind / 4, stream))) return call.fail(rc);
    HIP_TRY(hipMemcpyAsync(out, d.stage_out.p, *n_out * (uint64_t)record_kind, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return ACGPU_OK;
}

// The body of acgpu_match_batch_utf8 and acgpu_match_batch_utf8_lossy
template <class P>
int match_batch_utf8(const acgpu_automaton *ca, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks, int record_kind, void *out,
                     uint64_t cap, uint64_t *n_out, typename P::Stats *stats) {
    if (!ca || !n_out || !offsets || (cap && !out)) return ACGPU_E_INVALID;
    if (record_kind != ACGPU_REC_SET && record_kind != ACGPU_REC_MAP) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    const HostTables &t = a->t;
    BatchPlan plan; // (in bytes: bytes >= units, so bytes + haystacks < 2^31 bounds the text the scan sees)
    int rc = check_batch(t, reinterpret_cast<const uint16_t *>(bytes), offsets, n_haystacks, &plan);
    if (rc) return rc;
    *n_out = 0;
    if (stats) *stats = P::stats();
    if (plan.total == 0) return ACGPU_OK; // (nothing to decode and nothing to find: no device needed)
    PoolCall call(a);
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    if ((rc = call.idle())) return rc; // (the NULL stream: see the stream rule)
    const hipStream_t stream = d.call_stream;
    Utf8Batch b;
    rc = stage_utf8_batch(d, t, bytes, offsets, n_haystacks, stream, &b, plan.per_haystack, P::errors);
    if (rc && rc != ACGPU_E_ENCODING) return call.fail(rc);
    if (stats) *stats = P::stats(&b, rc);
    if (rc) return rc; // (ACGPU_E_ENCODING.  The stream is idle: the pool is as usable as before the call)
    const uint64_t W = (uint64_t)record_kind / 4, out_rec = (uint64_t)record_kind + 4;
    if (plan.per_haystack) { // every haystack by the route acgpu_match_utf8 takes, tagged on the host
        std::vector<int32_t> tmp;
        uint64_t n = 0;
        for (uint32_t i = 0; i < n_haystacks; i++) {
            const uint64_t len = offsets[i + 1] - offsets[i];
            if (!len) continue;
            uint64_t got = 0;
            const uint64_t room = cap > n ? cap - n : 0;
            Utf8Text text;
            if ((rc = stage_utf8_text(d, bytes + offsets[i], len, stream, &text, P::errors))) return call.fail(rc == ACGPU_E_ENCODING ? ACGPU_E_HIP : rc);
            if ((rc = d.stage_out.ensure(room * (uint64_t)record_kind + 16))) return call.fail(rc);
            rc = match_shard(a, d, &text.shard, record_kind, d.stage_out.p, room, &got, stream, nullptr);
            if (rc != ACGPU_OK && rc != ACGPU_E_OVERFLOW) return call.fail(rc);
            if (rc == ACGPU_OK && got) {
                if ((rc = utf8_map_records(text, nullptr, reinterpret_cast<int32_t *>(d.stage_out.p), got, (uint32_t)W, stream))) return call.fail(rc);
                try {
                    tmp.resize(got * W);
                } catch (...) {
                    return call.fail(ACGPU_E_NOMEM);
                }
                if (hipMemcpyAsync(tmp.data(), d.stage_out.p, got * (uint64_t)record_kind, hipMemcpyDeviceToHost, stream) != hipSuccess ||
                    hipStreamSynchronize(stream) != hipSuccess)
                    return call.fail(ACGPU_E_HIP);
                for (uint64_t r = 0; r < got; r++) {
                    int32_t *o = (int32_t *)((char *)out + (n + r) * out_rec);
                    o[0] = (int32_t)i;
                    for (uint64_t w = 0; w < W; w++) o[1 + w] = tmp[r * W + w];
                }
            }
            n += got;
        }
        *n_out = n;
        return n > cap ? call.fail(ACGPU_E_OVERFLOW) : ACGPU_OK;
    }
    if ((rc = d.stage_out.ensure(cap * (uint64_t)record_kind + 16))) return call.fail(rc);
    if ((rc = d.batch_out.ensure(cap * out_rec + 16))) return call.fail(rc);
    {
        SeparatorScan sep(d, t);
        rc = match_shard(a, d, &b.text.shard, record_kind, d.stage_out.p, cap, n_out, stream, nullptr);
    }
    if (rc != ACGPU_OK) return call.fail(rc); // (ACGPU_E_OVERFLOW: *n_out is the capacity to call again with)
    if (!*n_out) return ACGPU_OK;
    if ((rc = utf8_batch_tag(b, d.stage_out.p, *n_out, record_kind, d.batch_out.p, stream))) return call.fail(rc);
    if (hipMemcpyAsync(out, d.batch_out.p, *n_out * out_rec, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
        return call.fail(ACGPU_E_HIP);
    return ACGPU_OK;
}

} // namespace

extern "C" {

int acgpu_match_utf8(const acgpu_automaton *a, const uint8_t *bytes, uint64_t n_bytes, int record_kind, void *out, uint64_t cap, uint64_t *n_out,
                     acgpu_utf8_stats *stats) {
    return match_utf8<Utf8StrictText>(a, bytes, n_bytes, record_kind, out, cap, n_out, stats);
}

int acgpu_match_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, uint64_t n_bytes, int record_kind, void *out, uint64_t cap,
                           uint64_t *n_out, acgpu_utf8_lossy_stats *stats) {
    return match_utf8<Utf8LossyText>(a, bytes, n_bytes, record_kind, out, cap, n_out, stats);
}

int acgpu_match_batch_utf8(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks, int record_kind, void *out,
                           uint64_t cap, uint64_t *n_out, acgpu_utf8_batch_stats *stats) {
    return match_batch_utf8<Utf8StrictBatch>(a, bytes, offsets, n_haystacks, record_kind, out, cap, n_out, stats);
}

int acgpu_match_batch_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks, int record_kind,
                                 void *out, uint64_t cap, uint64_t *n_out, acgpu_utf8_lossy_stats *stats) {
    return match_batch_utf8<Utf8LossyBatch>(a, bytes, offsets, n_haystacks, record_kind, out, cap, n_out, stats);
}

} // extern "C"
