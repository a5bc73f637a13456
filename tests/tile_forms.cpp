// tile_forms.cpp -- a stand-alone host program (tests/test_tile_forms_cpu.py builds it with ROCm's clang++, no device code, no HIP
// runtime) over csrc/acgpu_forms.h: it sweeps a grid of tables and launches through choose_tile_form, choose_ww_form and
// choose_dfa_form and prints one line per input, `input -> name, dynamic LDS bytes, template arguments` or `input -> none`.
// The test compares the lines with tests/tile_forms_expected.txt, which the dispatch code these choosers replaced printed
// for the same sweep.  Here: every chosen form is in its table of compiled forms (else "NOT COMPILED" and exit status 1), and
// the table entries the sweep never chose are listed at the end ("unreached ...").
#include <cstdio>
#include <string>
#include <vector>

#include "acgpu_forms.h"

using namespace acgpu;

static const uint32_t g_words[4] = {0, 0, 0, 0}; // what the table pointers of the sweep point at (never read)

// ---- the sweeps: the inputs and their labels ----------------------------------------------------------------------------------
// The grid is crossed where the answer depends on the crossing and walked one step from a base point elsewhere: every table kind
// at every filt_k under the base conditions, then every other condition on the four kinds that read it.
struct TileCond {
    int l2; // 0: no second level, 1: l2_bloom + l2_depth, 2: both and l2_big, 3: l2_bloom without l2_depth, 4: l2_big + l2_depth without l2_bloom
    int has_short;
    uint32_t filt_words, filt_n, region_units, bits;
};
static const TileCond kTileConds[] = { // [0]: the base; [5] and [12] take the packed forms away, at every filt_k
    {1, 0, 19712, 4, 65536, 0},          {1, 1, 19712, 4, 65536, 0},        {2, 0, 19712, 4, 65536, 0},       {2, 1, 19712, 4, 65536, 0},
    {2, 1, 19712, 4, 65536, 1u << 30},   {0, 1, 19712, 4, 65536, 0},        {3, 0, 19712, 4, 65536, 0},       {4, 0, 19712, 4, 65536, 0},
    {1, 0, 19713, 4, 65536, 0},          {2, 1, 19712, 33, 65536, 0},       {2, 1, 19712, 300, 65536, 0},     {1, 1, 19712, 4, 65536 + 2048, 0},
    {2, 1, 19712, 4, 65536, 1024},       {1, 0, 19712, 4, 65536, 2048},     {2, 1, 19712, 4, 65536, 2048},    {2, 1, 19712, 4, 65536 + 2048, 1u << 30},
};
struct TileKind {
    int range;
    uint32_t row;
    int hashk;
    uint32_t nr; // fold_range: 0 = off, or the ranges in use
};
static const TileKind kPackedKinds[] = {{1, 4, 0, 0}, {0, 4, 0, 2}, {0, 4, 1, 2}, {0, 4, 1, 4}}; // range, folded range, merged stretches (2, 4)
static const TileKind kSplitKinds[] = {{1, 4, 0, 0}, {0, 8, 0, 0}, {0, 8, 1, 0}};               // range, class table, bucketed

template <class Emit>
static void tile_input(Emit &&emit, bool split, uint32_t k, const TileKind &kind, const TileCond &z) {
    char in[160];
    DevTables t{};
    TileLaunch l{};
    t.filt_k = k;
    t.range_cls = kind.range;
    t.filt_row_bytes = kind.row;
    t.hashk = kind.hashk;
    t.fold_range = kind.nr != 0;
    t.fr_nr = kind.nr ? kind.nr : 2;
    t.fr_base = 97, t.fr_span = 26, t.fr_base2 = 65, t.fr_base3 = 48, t.fr_base4 = 32;
    t.cls_base = 97, t.cls_span = 26;
    t.l2_bloom = (z.l2 >= 1 && z.l2 <= 3) ? g_words : nullptr;
    t.l2_big = (z.l2 == 2 || z.l2 == 4) ? g_words : nullptr;
    t.l2_depth = (z.l2 == 1 || z.l2 == 2 || z.l2 == 4) ? 6 : 0;
    t.has_short = (uint32_t)z.has_short;
    t.filt_words = z.filt_words;
    t.filt_n = z.filt_n;
    l.block = kTileBlock;
    l.region_units = z.region_units;
    l.debug = z.bits;
    std::snprintf(in, sizeof(in), "T split=%d k=%u range=%d row=%u hashk=%d fr=%u l2=%d short=%d words=%u n=%u region=%u bits=%u", (int)split, k,
                  kind.range, kind.row, kind.hashk, kind.nr, z.l2, z.has_short, z.filt_words, z.filt_n, z.region_units, z.bits);
    emit(in, t, l, split);
}

template <class Emit>
static void sweep_tile(Emit &&emit) {
    for (int split = 0; split < 2; ++split) // every kind of table at every filt_k (the split form does not read fr_nr)
        for (uint32_t k = 0; k <= 9; ++k)
            for (int range = 0; range < 2; ++range)
                for (uint32_t row = 4; row <= 8; row += 4)
                    for (int hashk = 0; hashk < 2; ++hashk)
                        for (uint32_t nr = 0; nr <= (split ? 2u : 4u); nr += 2) tile_input(emit, split != 0, k, TileKind{range, row, hashk, nr}, kTileConds[0]);
    for (size_t c = 1; c < sizeof(kTileConds) / sizeof(kTileConds[0]); ++c) {
        const bool every_k = c == 5 || c == 12;
        for (uint32_t k = every_k ? 1 : 2; k <= (every_k ? 8u : 5u); ++k) // (the second level: K = 2 .. 5)
            for (const TileKind &kind : kPackedKinds) tile_input(emit, false, k, kind, kTileConds[c]);
    }
    for (uint32_t words : {20224u, 20225u}) // the split form: the rows around the filter-only kernel's LDS array
        for (uint32_t k : {1u, 4u})
            for (const TileKind &kind : kSplitKinds) {
                TileCond z = kTileConds[0];
                z.filt_words = words;
                tile_input(emit, true, k, kind, z);
            }
}

template <class Emit>
static void ww_input(Emit &&emit, int cs, int bp, uint32_t pages, uint32_t max_len, uint32_t buckets, uint32_t bits) {
    char in[160];
    DevTables t{};
    TileLaunch l{};
    t.cs = cs;
    t.wbits = g_words;
    t.ww_bp_n = bp ? 10 : 0;
    t.ww_bp_wbits = bp == 1 ? g_words : bp == 2 ? g_words + 1 : nullptr;
    t.fold_n_pages = pages;
    t.max_len = max_len;
    t.ww_ph = buckets ? g_words : nullptr;
    t.ww_ph_buckets = buckets;
    t.ww_bloom_mask = 64 * 1024 * 8 - 1;
    l.block = kTileBlock;
    l.debug = bits;
    std::snprintf(in, sizeof(in), "W cs=%d byte_pages=%d fold_pages=%u max_len=%u ph_buckets=%u bits=%u", cs, bp, pages, max_len, buckets, bits);
    emit(in, t, l);
}

template <class Emit>
static void sweep_ww(Emit &&emit) {
    for (int cs = 0; cs < 2; ++cs)
        for (int bp = 0; bp < 3; ++bp) // byte pages: none, the scan's own, built for other word bits
            for (uint32_t pages : {18u, 65u})
                for (uint32_t max_len : {16u, 17u, 32u, 33u})
                    for (uint32_t buckets : {0u, 20000u}) ww_input(emit, cs, bp, pages, max_len, buckets, 0);
    for (int cs = 0; cs < 2; ++cs) // the selection bits, and displacements that do not fit LDS
        for (int bp = 0; bp < 2; ++bp)
            for (uint32_t max_len : {16u, 32u}) {
                for (uint32_t bits : {256u, 1u << 28, 1u << 29}) ww_input(emit, cs, bp, 18, max_len, 20000, bits);
                ww_input(emit, cs, bp, 18, max_len, 70000, 0);
            }
}

template <class Emit>
static void sweep_dfa(Emit &&emit) {
    char in[160];
    for (int dense = 0; dense < 2; ++dense)
        for (int entry = 2; entry <= 4; entry += 2)
            for (int range = 0; range < 2; ++range)
                for (uint32_t lds_entries : {100u, 20000u, 40000u, 70000u, 0u}) // 40 classes x 500 states: a part of the table, all of it, more than the LDS holds; 0: more states than k_ac_dfa's words hold
                    for (uint32_t bits : {0u, 1u}) {
                        DevTables t{};
                        ScanLaunch l{};
                        t.dense = dense;
                        t.entry_bytes = entry;
                        t.range_cls = range;
                        t.n_states = lds_entries ? 500u : 1u << 24;
                        t.n_cls = 40;
                        t.lds_entries = lds_entries ? lds_entries : 100u;
                        l.debug = bits;
                        std::snprintf(in, sizeof(in), "D dense=%d entry=%d range=%d states=%u lds_entries=%u bits=%u", dense, entry, range, t.n_states, t.lds_entries, bits);
                        emit(in, t, l);
                    }
}

// ---- what the choosers answer ---------------------------------------------------------------------------------------------------
static bool g_ok = true;
static std::vector<int> g_tile_hits(kTileFormCount, 0), g_ww_hits(kWwFormCount, 0), g_dfa_hits(kDfaFormCount, 0);

template <class Table, class Form>
static void hit(const Table &table, const Form &f, std::vector<int> &hits, const char *in) {
    const int i = form_index(table, f);
    if (i < 0) {
        std::printf("NOT COMPILED: %s\n", in);
        g_ok = false;
    } else {
        ++hits[(size_t)i];
    }
}

static std::string tile_args(const TileForm &f) {
    char b[64];
    std::snprintf(b, sizeof(b), "%d %d %d %d %d %d %d %d %d %d", f.k, f.range, f.wide, f.split, f.hashk, f.pk, f.l2, f.nr4, f.shorts, f.big);
    return b;
}

int main() {
    char name[kFormNameBytes], line[256];
    sweep_tile([&](const char *in, const DevTables &t, const TileLaunch &l, bool split) {
        const std::optional<TileForm> f = choose_tile_form(t, l, split);
        if (!f) {
            std::printf("%s -> none\n", in);
            return;
        }
        hit(kTileForms, *f, g_tile_hits, in);
        if (f->filter_only() != split) g_ok = false;
        // (the name as acgpu_profile::scan_kernel shows it: the field holds 63 characters)
        std::snprintf(line, sizeof(line), "%s -> %.63s, %zu, %s", in, tile_form_name(*f, name), f->lds, tile_args(*f).c_str());
        std::puts(line);
    });
    sweep_ww([&](const char *in, const DevTables &t, const TileLaunch &l) {
        const WwForm f = choose_ww_form(t, l, l.block);
        hit(kWwForms, f, g_ww_hits, in);
        std::printf("%s -> %s, %zu\n", in, ww_form_name(f, name), f.lds);
    });
    sweep_dfa([&](const char *in, const DevTables &t, const ScanLaunch &l) {
        const std::optional<DfaForm> f = choose_dfa_form(t, l);
        if (!f) {
            std::printf("%s -> none\n", in);
            return;
        }
        hit(kDfaForms, *f, g_dfa_hits, in);
        std::printf("%s -> %s\n", in, dfa_form_name(*f, name));
    });
    for (size_t i = 0; i < kTileFormCount; ++i)
        if (!g_tile_hits[i]) std::printf("unreached k_ac_tile %s\n", tile_args(kTileForms[i]).c_str());
    for (size_t i = 0; i < kWwFormCount; ++i)
        if (!g_ww_hits[i]) std::printf("unreached %s\n", ww_form_name(kWwForms[i], name));
    for (size_t i = 0; i < kDfaFormCount; ++i)
        if (!g_dfa_hits[i]) std::printf("unreached %s\n", dfa_form_name(kDfaForms[i], name));
    std::printf("tile_forms: %s\n", g_ok ? "done" : "FAILED");
    return g_ok ? 0 : 1;
}
