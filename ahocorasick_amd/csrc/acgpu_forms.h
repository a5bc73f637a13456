// acgpu_forms.h -- which instantiation of a scan kernel serves a dictionary: k_ac_tile / k_ac_verify (acgpu_tile.hip), k_ww_pp /
// k_ww_tile (acgpu_wholeword.hip) and k_ac_dfa / k_ac_scan_* (acgpu_kernels.hip).  Host code only -- no kernel, nothing that
// needs a device: tests/tile_forms.cpp compiles it into a stand-alone program.  For every family there is
//   a form    : the kernel's template arguments, the dynamic LDS it is launched with, and its name;
//   a chooser : ONE pure function that holds every predicate of the choice, once;
//   a table   : the forms that are compiled, written as the rules that generate them.  The .hip file instantiates exactly the
//               table's entries (launch_form<I>) and looks the chosen form up in it: a form that is not there is an error.
#pragma once
#include <array>
#include <cstdio>
#include <optional>
#include <string_view>

#include "acgpu_kernels.h"

namespace acgpu {

// ---- geometry the predicates and the LDS sizes need (the kernels read the same constants) -------------------------------------
constexpr int kTileBlock = 1024;               // 16 waves share one LDS copy of the filter rows
constexpr int kTileUnits = 512;                // units per wave tile (64 lanes x 8 units)
#ifndef ACGPU_NB
#define ACGPU_NB 2
#endif
constexpr int kVerifyBatches = ACGPU_NB;              // candidates verified per lane and call (independent load chains in flight)
#ifndef ACGPU_VEC
#define ACGPU_VEC 2
#endif
// AhoCorasick tile geometry: a lane holds kAcVec 16-byte vectors = 8*kAcVec consecutive units of a tile, so the per-tile
// fixed work (prefix sum, cross-lane carry, queue append) is shared by 16 positions per lane instead of 8
constexpr int kAcVec = ACGPU_VEC;
constexpr int kAcLaneUnits = 8 * kAcVec;
constexpr int kAcTileUnits = kWave * kAcLaneUnits;
constexpr int kAcCandCap = kAcTileUnits + kVerifyBatches * kWave;
constexpr int kFilterWordsSplit = 20224; // the filter-only kernel: 79 KiB, so that two workgroups fit one CU's 160 KiB
// L2 form (second-level filter in LDS, see l2_gram in acgpu_internal.h): smaller static array for the rows, and per wave a
// queue of SURVIVORS (kL2Cap), a copy of the current tile as packed classes behind an 8-unit halo (kTbBytes) and the list
// of the tile's first-level candidates (kL2Fresh tile-relative positions); the Bloom words follow
constexpr int kFilterWordsL2 = 19712;  // 78848 bytes: 27 classes, K = 4
constexpr int kL2Cap = 256;            // a drain leaves fewer than 128; a tile adds at most 128 through the second level
constexpr int kL2Fresh = 128;
constexpr int kL2Vec = 4;              // the L2 form takes 32 units per lane: every per-tile cost is shared by 2048 positions
constexpr int kL2TileUnits = kWave * 8 * kL2Vec;
constexpr int kTbBytes = 16 + kL2TileUnits; // one BYTE per class: [8 spare][8 classes before the tile][the tile]
constexpr size_t kL2WaveBytes = kL2Cap * 4 + kL2Cap * 2 + kTbBytes + kL2Fresh * 2; // queue (info + pos16), tile copy, list
constexpr uint32_t kFtWords = 2 + kTileBlock / kWave; // fused tail, LDS: [0] the workgroup's number (later: the records below it), [1] the slice's fill mark, [2 + w] wave w's records

// ---- k_ac_tile ----------------------------------------------------------------------------------------------------------------
struct TileForm {
    int k;                                                        // k_ac_tile's ten template arguments, in their order
    bool range, wide, split, hashk, pk, l2, nr4, shorts, big;
    size_t lds;    // dynamic LDS at the launch's block size (the filter-only form has none)
    int name_args; // how many of the arguments the name prints
    bool filter_only() const { return split; }
    bool same_kernel(const TileForm &o) const {
        return k == o.k && range == o.range && wide == o.wide && split == o.split && hashk == o.hashk && pk == o.pk && l2 == o.l2 &&
               nr4 == o.nr4 && shorts == o.shorts && big == o.big;
    }
};

inline bool tile_split_supported(const DevTables &t) {
    return t.filt_k >= 1 && t.filt_words <= (uint32_t)kFilterWordsSplit && !(t.hashk && t.fold_range); // (merged ranges: fused only)
}

// the packed 16-bit filter: range classes, 4-byte rows, row index below 2^16 (kSelScalarFilter keeps the scalar filter: A/B)
inline bool tile_pk_usable(const DevTables &t, const TileLaunch &l) {
    if (!(t.range_cls || t.fold_range) || t.filt_row_bytes != 4 || t.filt_k < 2 || (t.hashk && !t.fold_range) || (l.debug & kSelScalarFilter)) return false;
    uint64_t rows = 1;
    for (uint32_t i = 0; i + 1 < t.filt_k; ++i) rows *= t.filt_n;
    if (rows > 65536) return false;
    if (t.fold_range) return t.fr_base + t.fr_span <= 65536 && t.fr_base2 + t.fr_span <= 65536 &&
                             (t.fr_nr <= 2 || (t.fr_base3 + t.fr_span <= 65536 && t.fr_base4 + t.fr_span <= 65536));
    return t.cls_base + t.cls_span <= 65536;
}

// The form of k_ac_tile that scans with these tables and this launch (its region_units and debug set), or none: tables no
// compiled form serves (the caller reports hipErrorInvalidValue; the builder makes no such tables).  `split`: the filter-only
// form, in front of k_ac_verify.  Fused, in this order: merged ranges, bucketed classes, the second level (with the large second
// level BIG, and SHORTS), the packed filter, the generic form.
inline std::optional<TileForm> choose_tile_form(const DevTables &t, const TileLaunch &l, bool split) {
    const int K = (int)t.filt_k;
    const bool range = t.range_cls != 0, wide = t.filt_row_bytes == 8;
    if (split) {
        if (!tile_split_supported(t) || K > 8 || (t.hashk && K > 3)) return std::nullopt;
        if (t.hashk) return TileForm{K, false, true, true, true, false, false, false, true, false, 0, 5}; // bucketed classes: LUT classes, 8-byte rows, K <= 3
        return TileForm{K, range, wide, true, false, false, false, false, true, false, 0, 4};
    }
    if (K < 1 || K > 8) return std::nullopt;
    const size_t waves = (size_t)(l.block / kWave);
    const size_t lds_queues = waves * kAcCandCap * sizeof(uint32_t);       // the candidate queues
    const size_t lds_l2 = waves * kL2WaveBytes + kL2Words * 4;             // the second-level forms, BIG among them
    const bool pk = tile_pk_usable(t, l);
    // the second-level filter behind the packed one (kSelNoSecondLevel keeps the one-level form: A/B): queue entries hold the
    // K-gram index in 20 bits and the position in its region in 16
    uint64_t grams = 1;
    for (uint32_t i = 0; i < t.filt_k; ++i) grams *= t.filt_n;
    const bool l2 = pk && t.l2_bloom != nullptr && t.l2_depth != 0 && K <= 5 && grams <= (1u << 20) && l.region_units <= 65536u &&
                    t.filt_words <= (uint32_t)kFilterWordsL2 && !(l.debug & kSelNoSecondLevel);
    // the large second level (K = 4, DevTables::l2_big): kSelNoBigL2 keeps the LDS form for A/B
    const bool big = l2 && t.l2_big != nullptr && K == 4 && !(l.debug & kSelNoBigL2);
    if (t.hashk && t.fold_range) { // merged ranges: the packed filter over up to four ranges, the verification by units; K <= 4
        if (!pk || K > 4) return std::nullopt; // (the builder chooses this form only where it is usable)
        return TileForm{K, false, false, false, true, true, l2, t.fr_nr > 2, true, big, l2 ? lds_l2 : lds_queues, big ? 10 : 8};
    }
    if (t.hashk) { // bucketed classes: LUT classes, 8-byte rows, K <= 3
        if (K > 3) return std::nullopt;
        return TileForm{K, false, true, false, true, false, false, false, true, false, lds_queues, 5};
    }
    // (short keywords imply K <= 4: the K = 5 form needs no SHORTS instantiation)
    if (l2) return TileForm{K, range, false, false, false, true, true, false, K <= 4 && t.has_short != 0, big, lds_l2, big ? 10 : 7};
    if (pk) return TileForm{K, range, false, false, false, true, false, false, true, false, lds_queues, 6};
    return TileForm{K, range, wide, false, false, false, false, false, true, false, lds_queues, 4};
}

// "k_ac_tile<" and the form's first name_args arguments: what acgpu_profile::scan_kernel has always shown for the family (4
// generic and filter-only, 5 bucketed, 6 packed, 7 second level, 8 merged, 10 BIG).  Known limit: the 7-argument names do not
// show SHORTS, the ninth argument.  The BIG names are longer than the 64-byte field of the ABI: the one cut is where the name is
// copied into it (close_call).
constexpr size_t kFormNameBytes = 96;
inline const char *tile_form_name(const TileForm &f, char (&buf)[kFormNameBytes]) { // (the longest name: 70 characters)
    const bool a[9] = {f.range, f.wide, f.split, f.hashk, f.pk, f.l2, f.nr4, f.shorts, f.big};
    size_t n = (size_t)std::snprintf(buf, sizeof(buf), "k_ac_tile<%d", f.k);
    for (int i = 0; i + 1 < f.name_args; ++i) n += std::string_view(a[i] ? ", true" : ", false").copy(buf + n, sizeof(buf) - 2 - n);
    buf[n++] = '>';
    buf[n] = 0;
    return buf;
}

// The compiled forms of k_ac_tile, as the rules that generate them (116).  lds and name_args belong to a chosen form: 0 here.
constexpr size_t kTileFormCount = 116;
constexpr std::array<TileForm, kTileFormCount> make_tile_forms() {
    std::array<TileForm, kTileFormCount> f{};
    size_t n = 0;
    for (int k = 1; k <= 8; ++k)      // generic and filter-only: every K, range or table classes, 4- or 8-byte rows
        for (int m = 0; m < 8; ++m) f[n++] = TileForm{k, (m & 1) != 0, (m & 2) != 0, (m & 4) != 0, false, false, false, false, true, false, 0, 0};
    for (int k = 1; k <= 3; ++k)      // bucketed classes, fused and filter-only
        for (int s = 0; s < 2; ++s) f[n++] = TileForm{k, false, true, s != 0, true, false, false, false, true, false, 0, 0};
    for (int k = 2; k <= 4; ++k)      // merged ranges: one or two levels, two or four ranges
        for (int m = 0; m < 4; ++m) f[n++] = TileForm{k, false, false, false, true, true, (m & 1) != 0, (m & 2) != 0, true, false, 0, 0};
    for (int k = 2; k <= 8; ++k)      // packed, one level
        for (int r = 0; r < 2; ++r) f[n++] = TileForm{k, r != 0, false, false, false, true, false, false, true, false, 0, 0};
    for (int k = 2; k <= 5; ++k)      // packed, second level: with SHORTS up to K = 4
        for (int m = 0; m < (k <= 4 ? 4 : 2); ++m) f[n++] = TileForm{k, (m & 1) != 0, false, false, false, true, true, false, (m & 2) != 0, false, 0, 0};
    for (int m = 0; m < 4; ++m)       // BIG (K = 4): range or folded-range classes x SHORTS ...
        f[n++] = TileForm{4, (m & 1) != 0, false, false, false, true, true, false, (m & 2) != 0, true, 0, 0};
    for (int r = 0; r < 2; ++r)       // ... and merged ranges, two or four
        f[n++] = TileForm{4, false, false, false, true, true, true, r != 0, true, true, 0, 0};
    return f; // (a count that is not kTileFormCount does not compile: an index past the array, or the check below)
}
constexpr std::array<TileForm, kTileFormCount> kTileForms = make_tile_forms();
static_assert(kTileForms[kTileFormCount - 1].k == 4 && kTileForms[kTileFormCount - 1].big, "the rules generate kTileFormCount forms");

template <class Table, class Form>
inline int form_index(const Table &table, const Form &f) { // -1: not compiled
    for (size_t i = 0; i < table.size(); ++i)
        if (table[i].same_kernel(f)) return (int)i;
    return -1;
}

// k_ac_verify<K, RANGE, HASHK>, the verification half of the split form: every K x range or table classes, and bucketed K <= 3
struct VerifyForm {
    int k;
    bool range, hashk;
    bool same_kernel(const VerifyForm &o) const { return k == o.k && range == o.range && hashk == o.hashk; }
};
inline std::optional<VerifyForm> choose_verify_form(const DevTables &t) {
    const int K = (int)t.filt_k;
    if (K < 1 || K > (t.hashk ? 3 : 8)) return std::nullopt;
    return VerifyForm{K, !t.hashk && t.range_cls != 0, t.hashk != 0};
}
constexpr size_t kVerifyFormCount = 19;
constexpr std::array<VerifyForm, kVerifyFormCount> make_verify_forms() {
    std::array<VerifyForm, kVerifyFormCount> f{};
    size_t n = 0;
    for (int k = 1; k <= 8; ++k)
        for (int r = 0; r < 2; ++r) f[n++] = VerifyForm{k, r != 0, false};
    for (int k = 1; k <= 3; ++k) f[n++] = VerifyForm{k, false, true};
    return f;
}
constexpr std::array<VerifyForm, kVerifyFormCount> kVerifyForms = make_verify_forms();
static_assert(kVerifyForms[kVerifyFormCount - 1].hashk, "the rules generate kVerifyFormCount forms");

// ---- k_ww_pp / k_ww_tile ------------------------------------------------------------------------------------------------------
#ifndef ACGPU_WW_NB
#define ACGPU_WW_NB 3
#endif
constexpr int kWwBatches = ACGPU_WW_NB;   // run starts verified per lane and call (independent lookup chains in flight)
// run starts per tile <= 256 (a start needs a non-word unit before it); the queue holds one verification call's worth
// (kept until the next call) plus one tile
constexpr int kWwCandCap = kWwBatches * 64 + 256 + 64;
#ifndef ACGPU_FOLD_PAGES_MAX
#define ACGPU_FOLD_PAGES_MAX 64
#endif
constexpr uint32_t kFoldPagesMax = ACGPU_FOLD_PAGES_MAX; // 32 KB of LDS; Unicode 13 simple lower-casing needs 18 pages
constexpr uint32_t kBytePagesMax = 64;                    // k_ww_pp, FOLD 3: 16 KB (acgpu_build.cpp caps HostTables::ww_bp_n at this)
// k_ww_pp, per wave: ring = 2 tile slots of 512 folded units + a copy of slot 0's first 32 units behind slot 1; bits = the same
// for the word-character bits, one byte per lane and tile; list = the run starts of the tile being verified
constexpr int kPpRingUnits = 2 * kTileUnits + 32;
constexpr int kPpBitBytes = 2 * (kTileUnits / 8) + 8;
constexpr int kPpListCap = kTileUnits / 2; // a run start needs a unit that is no word character before it
constexpr int kPpWaveBytes = (kPpRingUnits * 2 + kPpBitBytes + kPpListCap * 2 + 15) & ~15;
constexpr uint32_t kPpMaxLen = 32; // longer keywords: k_ww_tile (up to 16 units: the LONG = false form, one 32-byte ring read per run)

// k_ww_pp<fold, lng, ph> (pp) or k_ww_tile<fold>.  fold: 0 = case-sensitive, 1 = the fold table's pages in LDS, 2 = the fold
// table in global memory (k_ww_tile only), 3 = word bit and fold delta in one byte page (k_ww_pp only).
struct WwForm {
    bool pp;
    int fold;
    bool lng, ph; // k_ww_pp: keywords of more than 16 units; the perfect hash (its displacements take the Bloom filter's place in LDS)
    size_t lds;   // dynamic LDS at the given block size
    bool same_kernel(const WwForm &o) const { return pp == o.pp && fold == o.fold && lng == o.lng && ph == o.ph; }
};
inline uint32_t ww_fold_pages_in_lds(const DevTables &t) { return (!t.cs && t.fold_n_pages <= kFoldPagesMax) ? t.fold_n_pages : 0u; }
inline size_t ww_bloom_bytes(const DevTables &t) { return ((size_t)t.ww_bloom_mask + 1) / 8; }
inline size_t ww_pp_static_lds(int fold) { // k_ww_pp's static LDS
    return (fold == 3 ? 16 + 256 + 16 + kBytePagesMax * 256 + 256 : fold == 1 ? 8192 + 256 + kFoldPagesMax * 512 + 32 : 8192 + 64) + kFtWords * 4;
}
// The position-parallel form serves keywords of at most 32 units whose fold table (if any) fits LDS, when its LDS fits next to
// the Bloom filter or the displacements (kSelWwTile keeps k_ww_tile: A/B; kSelWwTrieWalk, the trie-walk verification, exists
// only there).  The byte pages serve the scan they were built for (case-insensitive, the automaton's own word bits).
inline WwForm choose_ww_form(const DevTables &t, const TileLaunch &l, int block_threads) {
    const size_t waves = (size_t)(block_threads / kWave);
    const bool byte_pages = !t.cs && t.ww_bp_n != 0 && t.ww_bp_n <= kBytePagesMax && t.wbits == t.ww_bp_wbits;
    const int fold_tile = t.cs ? 0 : ww_fold_pages_in_lds(t) ? 1 : 2;
    const int fold = byte_pages ? 3 : fold_tile;
    const bool ph = t.ww_ph != nullptr && !(l.debug & kSelWwNoPerfectHash);
    const size_t pp_lds = (ph ? ((size_t)t.ww_ph_buckets + 7) / 8 * 16 : ww_bloom_bytes(t)) + waves * kPpWaveBytes;
    if (fold != 2 && t.max_len <= kPpMaxLen && !(l.debug & (kSelWwTrieWalk | kSelWwTile)) && pp_lds + ww_pp_static_lds(fold) <= 160 * 1024)
        return WwForm{true, fold, t.max_len > 16, ph, pp_lds};
    // k_ww_tile: [Bloom words | candidate queues]; the word-character bits, the page index and the pages are static LDS
    return WwForm{false, fold_tile, false, false, ww_bloom_bytes(t) + waves * kWwCandCap * sizeof(uint32_t)};
}
inline const char *ww_form_name(const WwForm &f, char (&buf)[kFormNameBytes]) {
    if (f.pp) std::snprintf(buf, sizeof(buf), "k_ww_pp<%d, %s, %s>", f.fold, f.lng ? "true" : "false", f.ph ? "true" : "false");
    else std::snprintf(buf, sizeof(buf), "k_ww_tile<%d>", f.fold);
    return buf;
}
constexpr size_t kWwFormCount = 15;
constexpr std::array<WwForm, kWwFormCount> make_ww_forms() {
    std::array<WwForm, kWwFormCount> f{};
    size_t n = 0;
    for (int fold : {0, 3, 1})        // k_ww_pp: the fold table in LDS or none
        for (int m = 3; m >= 0; --m) f[n++] = WwForm{true, fold, (m & 2) != 0, (m & 1) != 0, 0};
    for (int fold = 0; fold < 3; ++fold) f[n++] = WwForm{false, fold, false, false, 0}; // k_ww_tile
    return f;
}
constexpr std::array<WwForm, kWwFormCount> kWwForms = make_ww_forms();
static_assert(!kWwForms[kWwFormCount - 1].pp && kWwForms[kWwFormCount - 1].fold == 2, "the rules generate kWwFormCount forms");

// ---- k_ac_dfa / k_ac_scan_dense / k_ac_scan_sparse ------------------------------------------------------------------------------
struct DfaForm {
    enum Kernel { Dfa, Dense, Sparse } kernel; // k_ac_dfa<E, range, glob>, k_ac_scan_dense<E>, k_ac_scan_sparse
    bool u16, range, glob;                     // E: 16- or 32-bit entries; glob: rows beyond the LDS copy exist
    bool same_kernel(const DfaForm &o) const { return kernel == o.kernel && u16 == o.u16 && range == o.range && glob == o.glob; }
};
// k_ac_dfa's packed state words hold the table's size
inline bool dfa_chains_usable(const DevTables &t) {
    return t.dense && t.n_states < (1u << 24) && t.n_cls < (1u << 22) && (uint64_t)t.n_states * t.n_cls < (1ull << 30);
}
// (kScanOneChain: the one-chain kernel, k_ac_scan_dense, where k_ac_dfa would run: A/B.)  None: more leading entries than
// k_ac_dfa's static LDS holds (lds_states_for keeps below it).
inline std::optional<DfaForm> choose_dfa_form(const DevTables &t, const ScanLaunch &l) {
    const bool u16 = t.entry_bytes == 2;
    if (!t.dense) return DfaForm{DfaForm::Sparse, false, false, false};
    if (!dfa_chains_usable(t) || (l.debug & kScanOneChain)) return DfaForm{DfaForm::Dense, u16, false, false};
    if ((uint64_t)t.lds_entries * (u16 ? 2u : 4u) > (uint64_t)kDfaLdsBytes) return std::nullopt;
    return DfaForm{DfaForm::Dfa, u16, t.range_cls != 0, (uint64_t)t.lds_entries < (uint64_t)t.n_states * t.n_cls};
}
inline const char *dfa_form_name(const DfaForm &f, char (&buf)[kFormNameBytes]) {
    const char *e = f.u16 ? "unsigned short" : "unsigned int";
    if (f.kernel == DfaForm::Dfa) std::snprintf(buf, sizeof(buf), "k_ac_dfa<%s, %s, %s>", e, f.range ? "true" : "false", f.glob ? "true" : "false");
    else if (f.kernel == DfaForm::Dense) std::snprintf(buf, sizeof(buf), "k_ac_scan_dense<%s>", e);
    else std::snprintf(buf, sizeof(buf), "k_ac_scan_sparse");
    return buf;
}
constexpr size_t kDfaFormCount = 11;
constexpr std::array<DfaForm, kDfaFormCount> make_dfa_forms() {
    std::array<DfaForm, kDfaFormCount> f{};
    size_t n = 0;
    for (int m = 7; m >= 0; --m) f[n++] = DfaForm{DfaForm::Dfa, (m & 4) != 0, (m & 2) != 0, (m & 1) != 0};
    for (int u = 1; u >= 0; --u) f[n++] = DfaForm{DfaForm::Dense, u != 0, false, false};
    f[n++] = DfaForm{DfaForm::Sparse, false, false, false};
    return f;
}
constexpr std::array<DfaForm, kDfaFormCount> kDfaForms = make_dfa_forms();
static_assert(kDfaForms[kDfaFormCount - 1].kernel == DfaForm::Sparse, "the rules generate kDfaFormCount forms");

} // namespace acgpu
