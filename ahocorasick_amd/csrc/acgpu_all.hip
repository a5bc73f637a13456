// acgpu_all.hip -- the ALL / WHOLEWORD planners: which form serves a call (the states form, the WholeWord tile kernels, the
// AhoCorasick tile kernel, the DFA chunk scan), its lay-out and launches, and the ordering stage behind a scan.
#include <algorithm>
#include <cstdio>
#include <initializer_list>
#include <optional>
#include <vector>

#include "acgpu_calls.h"
#include "acgpu_forms.h"

using namespace acgpu;

namespace {

uint32_t round_up8(uint64_t v) { return (uint32_t)((v + 7) & ~7ull); }

// Region size of the tile kernels for a long shard: every wave scans r regions of R units one after the other, so the scan
// lasts as long as r * R units of one wave -- with a fixed R the step from "r regions fill the waves exactly" to one region
// more costs a whole region per wave (2^29 units in 32768-unit regions on 4096 waves: r = 4; one unit more, or four CUs
// fewer (tunable reserve_cus): r = 5, a quarter slower).  Chosen here: whole tile groups, between r_lo and r_hi regions per
// wave, the smallest r * R that covers the shard; among equals the R nearest `prefer`.
uint64_t balanced_region_units(uint64_t len, uint64_t waves, uint64_t g, uint64_t r_min, uint64_t r_hi, uint64_t prefer) {
    uint64_t best_R = 0, best_cost = ~0ull, best_dist = ~0ull;
    for (uint64_t r = 1; r <= r_hi; ++r) {
        const uint64_t m = (len + waves * r * g - 1) / (waves * r * g);
        const uint64_t R = std::max<uint64_t>(m, 1) * g;
        if (R < r_min || R > 65536) continue;
        const uint64_t cost = r * R, dist = R > prefer ? R - prefer : prefer - R;
        if (cost < best_cost || (cost == best_cost && dist < best_dist)) {
            best_cost = cost;
            best_dist = dist;
            best_R = R;
        }
    }
    return best_R;
}

// the split form needs the filter rows to fit the smaller static LDS array of the filter-only kernel
// (measured at config 2: filter 0.27 ms + verification 0.33 ms against 0.39 ms fused -- the fused kernel verifies a
// candidate while its text is still in the L2 of the XCD that streamed it; the split form gathers it from HBM again --
// so the split form is only taken on request)
bool use_split_form(const DevTables &T) { return tunables().force_kernel == 3 && tile_split_supported(T); }

// ALL-mode pipeline on one shard, the form for texts with dense matches: see enqueue_all.
constexpr double kStatesFormDensity = 0.05; // records per unit of the pool's last call from which k_ac_states is taken
// counting: the direct form of a counting call (acgpu_count.hip) -- k_states_hist adds the owned positions' states to the pool's
// visit words in place of the prefix sum's consumer, the record pass; the count still comes from the chunks' counts.
int enqueue_states(acgpu_automaton *a, DeviceState &d, CallRecord &r, uint32_t hot_rows, bool counting = false) {
    const HostTables &t = a->t;
    const acgpu_shard *sh = &r.shard;
    const PoolEvent *ev = r.ev;
    const hipStream_t stream = r.stream;
    int rc;
    AcStatesLaunch S{};
    S.d_hay = sh->d_hay;
    S.n_units = (uint32_t)sh->n_units;
    S.own_begin = (uint32_t)sh->own_begin;
    S.own_end = (uint32_t)sh->own_end;
    S.g0 = S.own_begin & ~3u;
    S.halo = t.max_len - 1;
    S.hot_rows = hot_rows;
    const uint64_t span = sh->own_end - S.g0;
    // a lane's chunk: 1024 units, shorter (down to 256) when the text would leave lanes of the chip without one
    // (development tunable states_chunk_log2: 8 .. 10 forces it -- 1 to 4 steps per chunk of the passes behind the walk on short texts)
    S.chunk_log2 = 10;
    const int64_t forced_log2 = tunables().states_chunk_log2;
    if (forced_log2 >= 8 && forced_log2 <= 10) S.chunk_log2 = (uint32_t)forced_log2;
    else while (S.chunk_log2 > 8 && (span >> S.chunk_log2) < (uint64_t)ac_states_lanes_per_cu() * d.n_cu) --S.chunk_log2;
    const uint64_t chunks = (span + (1ull << S.chunk_log2) - 1) >> S.chunk_log2;
    S.n_waves = (uint32_t)((chunks + 63) / 64);
    S.n_chunks = (uint32_t)chunks;
    if (tunables().tile_debug & kSelAllocFails) return ACGPU_E_NOMEM; // (tests: the allocation "fails", the caller falls back)
    if ((rc = d.statebuf.ensure((((size_t)S.n_waves * 64) << S.chunk_log2) * 4 + 64))) return rc;
    if ((rc = ensure_scan_buffers(d, S.n_chunks))) return rc;
    S.d_state = (uint32_t *)d.statebuf.p;
    S.d_counts = (uint32_t *)d.chunk_counts.p;
    S.d_offsets = (const uint64_t *)d.offsets.p;
    S.d_out = r.d_out;
    S.cap = r.cap;
    S.grid = (int)std::min<uint64_t>((uint64_t)d.n_cu * (ac_states_lanes_per_cu() / 1024u), (S.n_waves + 15) / 16);
    if ((rc = borrow_counter_line(d, stream, /*clear=*/true))) return rc; // (word 1: the "redo" flag of the result -- never raised here)
    if (counting) {
        CountCall &c = *d.count;
        S.d_visits = (uint32_t *)d.visits.p;
        S.n_states = t.hy_n_states;
        const int64_t cform = tunables().count_form;
        S.hist_hot = (cform & 2) ? 0u : std::min(t.hy_n_states, states_hist_max_hot());
        S.hist_peel = (cform & 4) ? 0u : 1u;
        if (!c.visits_zeroed) HIP_TRY(hipMemsetAsync(d.visits.p, 0, (size_t)t.hy_n_states * 4, stream));
        c.visits_zeroed = true;
    }
    if (r.profiled) HIP_TRY(hipEventRecord(ev[0], stream));
    HIP_TRY(launch_ac_states(d.T, S, t.range_cls, stream));
    if (r.profiled) HIP_TRY(hipEventRecord(ev[1], stream));
    HIP_TRY(launch_exclusive_scan(S.d_counts, S.n_chunks, (uint64_t *)d.offsets.p, (uint64_t *)d.scan_tmp.p, stream));
    if (counting) HIP_TRY(launch_states_hist(S, d.n_cu, stream));
    else HIP_TRY(launch_ac_states_out(d.T, S, r.record_kind == ACGPU_REC_MAP, stream));
    if (r.profiled) HIP_TRY(hipEventRecord(ev[2], stream));
    unsigned long long *d_slot = nullptr;
    if ((rc = slot_on_device(r, &d_slot))) return rc;
    HIP_TRY(launch_publish_result((const unsigned long long *)scan_total(d, S.n_chunks), (const unsigned long long *)d.counter.p, d_slot,
                                  reinterpret_cast<acgpu_device_result *>(sh->d_result), stream));
    return close_call(r, counting ? CallForm::StatesCount : CallForm::States, "k_ac_states", sh->own_end - sh->own_begin);
}

// Texts in which this dictionary matches densely (natural words in natural text: every filter passes, every verification walk
// is long): the automaton's state behind every unit (k_ac_states over the compact automaton of acgpu_build.cpp 6d), then the
// records from the states (acgpu_states.hip).  Its cost does not depend on the text (~ one gather per unit), the tile kernel's
// does: what this pool's last call found decides (records per unit; a pool's first call looks at the beginning of a long text,
// and takes the tile kernel for a short one or when it may not wait).
// Tunable all_form, bits: 1 = never, 2 = whatever the last call found, 4 = also for short texts.
// *hot: k_ac_states' hot rows when the call takes this form, 0 otherwise.
int choose_states_form(acgpu_automaton *a, DeviceState &d, const CallRecord &r, uint32_t *hot) {
    const HostTables &t = a->t;
    const uint64_t own_len = r.shard.own_end - r.shard.own_begin;
    *hot = 0;
    const int64_t aform = tunables().all_form;
    const size_t st_pages = (!t.range_cls && !t.dfa_pages.empty()) ? t.dfa_pages.size() * 2 : 0;
    const uint32_t st_hot = (t.mode != ACGPU_MODE_WHOLEWORD && t.hy_n_states && (t.range_cls || st_pages > 0))
                                ? ac_states_hot_rows(t.n_cls, t.hy_n_dense, (uint32_t)st_pages) : 0;
    const bool usable = st_hot > 0 && !(aform & 1) && tunables().force_kernel == 0 && r.level == 0 && (own_len >= (1ull << 20) || (aform & 4));
    // a pool that knows nothing yet and a long text (a synchronous call): the first 2^20 units of the shard are counted first (a
    // synchronous call of this form on the pool's record, no records written: 60 us) -- the whole text then takes the form its
    // beginning suggests
    if (usable && !r.done && d.all_density < 0.0 && !(aform & 2) && own_len >= (1ull << 23)) {
        CallRecord head = r;
        head.shard.own_end = head.shard.own_begin + (1ull << 20);
        head.shard.d_result = nullptr;
        head.cap = 0;
        head.profiled = false;
        head.counting = false;
        uint64_t n_head = 0;
        int prc = enqueue_states(a, d, head, st_hot);
        if (prc == ACGPU_OK) prc = collect(a, d, &head, &n_head, nullptr, nullptr);
        // (no room for the probe's state words: like the call itself below, the tile kernel it is -- the pool stays without a
        // density, so a later call asks again)
        if (prc != ACGPU_OK && prc != ACGPU_E_OVERFLOW && prc != ACGPU_E_NOMEM) return prc;
    }
    if (usable && ((aform & 2) || d.all_density >= kStatesFormDensity)) *hot = st_hot;
    return ACGPU_OK;
}

// An ALL / WHOLEWORD scan into the scratch slices: what a scan form's setup is given, and what it leaves for the ordering stage.
struct AllScan {
    const DevTables *T = nullptr; // the scan's tables (WHOLEWORD: folded_tables for a scan that folds in every lookup)
    unsigned long long *counters = nullptr, *counters_next = nullptr; // this call's set of slot counters, the next call's
    uint32_t *overflow_word = nullptr;
    uint64_t scratch_cap = 0;
    bool fused_only = false; // the redo: the fused kernel, one scratch slice
    // left by the setup
    enum class Order { Permute, PermuteWg, WwCompact, FusedTail } order = Order::Permute;
    uint32_t n_slices = 1, n_chunks = 0, chunk_units = 0, perm_base = 0, regions_per_wg = 0, ww_region_cap = 0;
    uint64_t slice_slots = 0;
    const uint32_t *id_map = nullptr;
    int by_start = 0;
    char kname[kFormNameBytes] = ""; // the whole name (close_call cuts it to the ABI's field)
    uint64_t scanned = 0;
};

// The fused tail's part of a tile launch (TileLaunch::fused_tail): the records' final place and where the call's result goes.
int set_fused_tail(TileLaunch &L, const CallRecord &r, AllScan &A, const uint32_t *id_map) {
    int rc;
    A.order = AllScan::Order::FusedTail;
    L.fused_tail = 1;
    L.d_out = r.d_out;
    L.out_cap = r.cap;
    L.out_map = r.record_kind == ACGPU_REC_MAP ? 1 : 0;
    L.d_id_map = id_map;
    if ((rc = slot_on_device(r, &L.tail_result))) return rc;
    L.tail_d_result = reinterpret_cast<acgpu_device_result *>(r.shard.d_result);
    L.tail_zero_counters = A.counters_next;
    return ACGPU_OK;
}

#ifdef ACGPU_TIMING
// ACGPU_TIMING builds: the scan kernels' s_memtime counters (8 words per wave, 16 waves per workgroup), read back after a
// synchronous call
DevBuf g_timing;
int timing_arm(TileLaunch &L, hipStream_t stream) {
    int rc;
    if ((rc = g_timing.ensure((size_t)L.grid * 16 * 8 * 8))) return rc;
    HIP_TRY(hipMemsetAsync(g_timing.p, 0, (size_t)L.grid * 16 * 8 * 8, stream));
    L.d_timing = (unsigned long long *)g_timing.p;
    return ACGPU_OK;
}

int timing_read(const TileLaunch &L, hipStream_t stream, std::vector<unsigned long long> &h) {
    HIP_TRY(hipStreamSynchronize(stream));
    h.assign((size_t)L.grid * 16 * 8, 0);
    HIP_TRY(hipMemcpy(h.data(), g_timing.p, h.size() * 8, hipMemcpyDeviceToHost));
    return ACGPU_OK;
}

// where a WholeWord wave's time goes (s_memtime ticks, 100 MHz), averaged over the waves
int timing_report_ww(const TileLaunch &L, bool fused_tail, hipStream_t stream) {
    std::vector<unsigned long long> h;
    if (int rc = timing_read(L, stream, h)) return rc;
    double sum[8] = {0}; size_t nw = 0;
    for (size_t w = 0; w < h.size() / 8; ++w) {
        if (!h[w * 8]) continue;
        nw++;
        for (int i = 0; i < 8; ++i) sum[i] += (double)h[w * 8 + i];
    }
    if (fused_tail) { // the workgroups in the order of their numbers: scan end, counts there, copy done (s_memtime ticks from the first scan end)
        unsigned long long t0 = ~0ull;
        for (size_t w = 0; w < h.size() / 8; ++w) if (h[w * 8]) t0 = std::min(t0, h[w * 8]);
        const size_t G = (size_t)L.grid;
        for (size_t b0 = 0; b0 < G; b0 += std::max<size_t>(G / 16, 1)) {
            double se = 0, be = 0, ce = 0; size_t k = 0;
            for (size_t b = b0; b < std::min(G, b0 + std::max<size_t>(G / 16, 1)); ++b)
                for (size_t w = b * 16; w < b * 16 + 16; ++w) if (h[w * 8]) { se = std::max(se, (double)(h[w * 8] - t0)); be = std::max(be, (double)(h[w * 8 + 1] - t0)); ce = std::max(ce, (double)(h[w * 8 + 2] - t0)); k++; }
            fprintf(stderr, "[ww fused tail] workgroups %3zu..: last scan end %8.0f | counts below there %8.0f | last copy done %8.0f\n", b0, se, be, ce);
        }
    } else
    if (nw) fprintf(stderr, "[ww timing] waves %zu total %.0f | windows %.0f | chunk1 %.0f | chunk2 %.0f | hash+bloom %.0f | probes %.0f | emission %.0f | calls %.1f\n",
                    nw, sum[0] / nw, sum[1] / nw, sum[2] / nw, sum[3] / nw, sum[4] / nw, sum[5] / nw, sum[6] / nw, sum[7] / nw);
    return ACGPU_OK;
}

// where an AhoCorasick tile wave's time goes, and the spread of the waves' durations
int timing_report_tile(const TileLaunch &L, hipStream_t stream) {
    std::vector<unsigned long long> h;
    if (int rc = timing_read(L, stream, h)) return rc;
    double sum[8] = {0}, mx0 = 0, vt[4] = {0, 0, 0, 0}, su = 0, su_min = 1e30, su_max = 0; size_t nw = 0;
    for (size_t w = 0; w < h.size() / 8; ++w) {
        if (!h[w * 8]) continue;
        nw++;
        { // word 4: passes, and above them the start-up (kernel entry to the first filtered tile)
            const double s = (double)(h[w * 8 + 4] >> 32);
            h[w * 8 + 4] &= 0xffffffffull;
            su += s; su_min = std::min(su_min, s); su_max = std::max(su_max, s);
        }
        for (int i = 0; i < 6; ++i) sum[i] += (double)h[w * 8 + i];
        vt[0] += (double)(h[w * 8 + 6] & 0xffffffffu); vt[1] += (double)(h[w * 8 + 6] >> 32);
        vt[2] += (double)(h[w * 8 + 7] & 0xffffffffu); vt[3] += (double)(h[w * 8 + 7] >> 32);
        mx0 = std::max(mx0, (double)h[w * 8]);
    }
    { // spread of the waves' durations: per XCD (workgroup modulo 8) and per workgroup
        double xs[8] = {0}, xm[8] = {0}; size_t xn[8] = {0}; double bmin = 1e30, bmax = 0, wmin = 1e30;
        for (size_t b = 0; b < (size_t)L.grid; ++b) {
            double bs = 0; size_t bn = 0;
            for (size_t w = b * 16; w < b * 16 + 16; ++w) if (h[w * 8]) { bs += (double)h[w * 8]; bn++; xm[b % 8] = std::max(xm[b % 8], (double)h[w * 8]); wmin = std::min(wmin, (double)h[w * 8]); }
            if (!bn) continue;
            xs[b % 8] += bs; xn[b % 8] += bn;
            bmin = std::min(bmin, bs / bn); bmax = std::max(bmax, bs / bn);
        }
        fprintf(stderr, "[timing] wave min %.0f; workgroup averages %.0f .. %.0f; per XCD avg/max:", wmin, bmin, bmax);
        for (int x = 0; x < 8; ++x) if (xn[x]) fprintf(stderr, " %.0f/%.0f", xs[x] / xn[x], xm[x]);
        fprintf(stderr, "\n[timing] by wave slot in the workgroup:");
        for (size_t sl = 0; sl < 16; ++sl) {
            double a = 0; size_t n2 = 0;
            for (size_t b = 0; b < (size_t)L.grid; ++b) if (h[(b * 16 + sl) * 8]) { a += (double)h[(b * 16 + sl) * 8]; n2++; }
            fprintf(stderr, " %.0f", n2 ? a / n2 : 0.0);
        }
        fprintf(stderr, "\n");
    }
    if (nw) fprintf(stderr, "[timing] start-up (entry to first filtered tile): avg %.0f min %.0f max %.0f\n", su / nw, su_min, su_max);
    if (nw) fprintf(stderr, "[timing] verification: windows %.0f | K-gram nodes %.0f | walks %.0f | emission %.0f\n", vt[0] / nw, vt[1] / nw, vt[2] / nw, vt[3] / nw);
    if (nw) fprintf(stderr, "[timing] waves %zu  total avg %.0f max %.0f | stream wait %.0f | drain %.0f (%.1f calls) | filter+L2 %.0f | passes %.1f  (s_memtime ticks, 100 MHz)\n",
                    nw, sum[0] / nw, mx0, sum[1] / nw, sum[2] / nw, sum[5] / nw, sum[3] / nw, sum[4] / nw);
    return ACGPU_OK;
}
#endif

// The region lay-out of a tile scan (setup_ww_scan, setup_tile_scan; L.block and L.debug are set): regions of sizes[i].units
// when the shard has at least sizes[i].per_wave units for each of `waves` waves (the last entry: any shard), on long shards
// (balance_from units per wave) the size that fills the waves evenly (balanced_region_units: r_min, prefer) -- or the tunable
// region_units -- rounded to whole tile groups and laid out from the shard's 16-byte aligned start; a wave scans regions_per_wave
// consecutive regions, the grid holds the waves that own one; one scratch slice and slot counter per workgroup (a slice that
// fills up: the redo takes one slice; kSelOneCounter: A/B); the region counts, their offsets and the prefix sum's words.
struct RegionSize {
    uint64_t units, per_wave;
};
int lay_out_regions(DeviceState &d, const CallRecord &r, AllScan &A, TileLaunch &L, uint64_t waves, std::initializer_list<RegionSize> sizes,
                    uint64_t balance_from, uint64_t r_min, uint64_t prefer) {
    const acgpu_shard *sh = &r.shard;
    const uint64_t own_len = sh->own_end - sh->own_begin, g = tile_group_units(), waves_per_block = (uint64_t)L.block / 64;
    const uint64_t base8 = sh->own_begin & ~7ull;
    int rc;
    uint64_t R = (uint64_t)tunables().region_units;
    if (tunables().region_units <= 0) {
        for (const RegionSize &z : sizes)
            if (own_len >= z.per_wave * waves) { R = z.units; break; }
        const uint64_t Rb = own_len >= balance_from * waves ? balanced_region_units(sh->own_end - base8, waves, g, r_min, 16, prefer) : 0;
        if (Rb) R = Rb;
    }
    R = std::max<uint64_t>(g, (R + g - 1) / g * g);
    L.region_units = (uint32_t)R;
    L.n_regions = (uint32_t)((sh->own_end - base8 + R - 1) / R);
    L.regions_per_wave = (uint32_t)((L.n_regions + waves - 1) / waves);
    const uint64_t waves_used = ((uint64_t)L.n_regions + L.regions_per_wave - 1) / L.regions_per_wave;
    L.grid = (int)((waves_used + waves_per_block - 1) / waves_per_block);
    A.perm_base = (uint32_t)base8;
    L.d_hay = sh->d_hay;
    L.n_units = (uint32_t)sh->n_units;
    L.own_begin = (uint32_t)sh->own_begin;
    L.own_end = (uint32_t)sh->own_end;
    L.cap = A.scratch_cap;
    L.d_overflow = A.overflow_word;
    if (!A.fused_only && L.grid > 1 && !(L.debug & kSelOneCounter)) {
        A.n_slices = (uint32_t)std::min<int>(L.grid, kMaxSlices);
        A.slice_slots = A.scratch_cap / A.n_slices;
    }
    L.n_slices = A.n_slices;
    L.slice_slots = (uint32_t)A.slice_slots;
    if ((rc = ensure_scan_buffers(d, L.n_regions))) return rc;
    L.d_scratch = (ScratchRec *)d.scratch.p;
    L.d_counter = A.counters;
    L.d_region_counts = (uint32_t *)d.chunk_counts.p;
    return ACGPU_OK;
}

// The launch of a tile scan and what it leaves for the ordering stage.  own_events: one kernel scans, and a profiled call takes
// that kernel's own dispatch timestamps (no marker packets around it); fused: the scan is the call's only kernel, its end the call's.
template <class Launch>
int launch_regions(TileLaunch &L, CallRecord &r, AllScan &A, bool own_events, bool fused, bool ww, Launch &&launch) {
    int rc;
#ifdef ACGPU_TIMING
    if ((rc = timing_arm(L, r.stream))) return rc;
#endif
    if (own_events && r.profiled) {
        L.ev_start = r.ev[0];
        L.ev_stop = r.ev[1];
    }
    if (own_events && fused) L.ev_stop = (r.profiled || r.done) ? r.ev[2] : nullptr;
    if ((rc = launch())) return rc;
#ifdef ACGPU_TIMING
    if (!r.done && own_events && (rc = ww ? timing_report_ww(L, fused, r.stream) : timing_report_tile(L, r.stream))) return rc;
#else
    (void)ww;
#endif
    A.n_chunks = L.n_regions;
    A.chunk_units = L.region_units;
    A.scanned = r.shard.own_end - r.shard.own_begin;
    return ACGPU_OK;
}

// WHOLEWORD (fold-consistent tables): the WholeWord tile kernels over regions -- run starts instead of K-gram candidates, ranks
// by match start, halos of 1 unit on the left and max_len + 1 on the right.
int setup_ww_scan(acgpu_automaton *a, DeviceState &d, CallRecord &r, AllScan &A) {
    const HostTables &t = a->t;
    const acgpu_shard *sh = &r.shard;
    const DevTables &T = *A.T;
    int rc;
    TileLaunch L{};
    L.block = tile_block_threads();
    L.debug = (uint32_t)tunables().tile_debug | (tunables().force_kernel == 1 ? (uint32_t)kSelWwTrieWalk : 0u);
    // regions as large as still gives every wave one (fewer forced drains: 65536 against 16384 units -2 % at config 5's share);
    // one scratch slice per workgroup: config 5 emits 15 M records per shard, 60 k reservations that one counter would serve at
    // under 100 per microsecond
    const uint64_t ww_waves = (uint64_t)d.n_cu * ww_blocks_per_cu() * (L.block / 64);
    if ((rc = lay_out_regions(d, r, A, L, ww_waves, {{65536, 65536}, {32768, 32768}, {16384, 0}}, 32768, 16384, 65536))) return rc;
    A.by_start = 1;
    const uint64_t R = L.region_units, base8 = A.perm_base;
    // region-local record slots (a region of R units holds at most R/2 + 1 words): no slot reservations in the scan, and a
    // coalesced copy instead of the permutation (kSelWwPermute: the scratch slices + k_permute, for A/B)
    L.d_region_recs = nullptr;
    L.region_cap = (uint32_t)(R / 2 + 1);
    const uint64_t ww_rec_bytes = (uint64_t)L.n_regions * L.region_cap * 12;
    bool direct = !(tunables().tile_debug & kSelWwPermute) && ww_rec_bytes <= (24ull << 30);
    // The fused tail of k_ww_pp (TileLaunch::fused_tail, ft_total16): no counts, prefix sums or copy pass behind the scan -- a
    // wave's records go to its own area and, when the workgroups with lower numbers are done, from there to their final
    // place.  (Tunable ww_ramp_pm: spans that grow with the workgroup's number, so that copies would run while later
    // workgroups still scan -- measured slower at every slope, 0 by default: EXPERIMENTS.md, round 6.)
    // Tunable tile_form bit 2: never (the region-local slots + k_ww_compact: A/B, tests).
    // Its areas take the place of the region-local slots: which of the two is decided before the one allocation below.
    bool fused = false;
    int block_ft = L.block;
    uint64_t total16 = 0, G = 0, area_recs = 0;
    const WwForm whole = choose_ww_form(T, L, L.block); // (k_ww_pp is the kernel that has the fused tail)
    if (direct && !A.fused_only && !(tunables().tile_form & 2) && whole.pp) {
        // (tunable ww_block: workgroups of fewer waves, two to a CU when their LDS allows -- A/B)
        const int64_t wb = tunables().ww_block;
        block_ft = (wb >= 64 && wb <= 1024 && wb % 64 == 0) ? (int)wb : L.block;
        const uint64_t wpb = (uint64_t)block_ft / 64;
        // (two workgroups: when each needs at most half the LDS, and for the 16-unit form only -- the 32-unit form's registers allow four waves per SIMD)
        // (block_ft <= L.block: k_ww_pp serves there as well, and the form's LDS is k_ww_pp's)
        const uint64_t per_cu = wb > 0 && t.max_len <= 16 && choose_ww_form(T, L, block_ft).lds + ww_pp_static_lds(whole.fold) <= 80 * 1024 ? 2 : 1;
        const uint64_t tiles = (sh->own_end - base8 + 511) / 512;
        total16 = (tiles + wpb - 1) / wpb;
        G = std::min<uint64_t>((uint64_t)d.n_cu * per_cu, total16);
        area_recs = total16 * wpb * 512 / 2 + G * wpb + 8;
        fused = G >= 1 && G <= (uint64_t)kMaxSlices && area_recs < (1ull << 32);
    }
    if (direct) {
        // (about 6 bytes per haystack unit: on a device that cannot spare them the call falls back to the scratch slices +
        // k_permute instead of failing; kSelAllocFails: the allocation "fails", for the test of that path)
        rc = (tunables().tile_debug & kSelAllocFails) ? ACGPU_E_NOMEM : d.ww_recs.ensure((fused ? area_recs * 12 : ww_rec_bytes) + 64);
        if (rc == ACGPU_E_NOMEM) direct = fused = false;
        else if (rc != ACGPU_OK) return rc;
    }
    if (direct) {
        L.d_region_recs = (int32_t *)d.ww_recs.p;
        A.order = AllScan::Order::WwCompact;
        A.ww_region_cap = L.region_cap;
    }
    if (fused) {
        L.grid = (int)G;
        L.block = block_ft;
        L.ft_total16 = (uint32_t)total16;
        const int64_t ramp = tunables().ww_ramp_pm;
        L.ft_ramp_pm = (uint32_t)(ramp < 0 ? 0 : std::min<int64_t>(ramp, 1000));
        if ((rc = set_fused_tail(L, r, A, nullptr))) return rc;
    } else {
        HIP_TRY(hipMemsetAsync(d.chunk_counts.p, 0, (size_t)L.n_regions * 4, r.stream));
    }
    const WwForm form = choose_ww_form(T, L, L.block);
    L.lds_bytes = form.lds;
    ww_form_name(form, A.kname);
    return launch_regions(L, r, A, true, fused, true, [&]() -> int {
        HIP_TRY(launch_ww_tile(T, L, form, r.stream));
        return ACGPU_OK;
    });
}

// ALL: the position-parallel K-gram tile kernel (fused, or the split form: filter + verification) over regions.
int setup_tile_scan(acgpu_automaton *a, DeviceState &d, CallRecord &r, AllScan &A) {
    int rc;
    TileLaunch L{};
    L.block = tile_block_threads();
    L.debug = (uint32_t)tunables().tile_debug;
    const int waves_per_block = L.block / 64;
    // regions of 16384 units, or 32768 when that still leaves every wave two of them (fewer forced drains: -1.1 % at
    // config 2 in interleaved A/B; 65536 was no better)
    if ((rc = lay_out_regions(d, r, A, L, (uint64_t)d.n_cu * waves_per_block, {{32768, 2 * 32768}, {16384, 0}}, 2 * 16384, 12288, 32768))) return rc;
    const uint64_t R = L.region_units;
    const uint64_t waves_used = ((uint64_t)L.n_regions + L.regions_per_wave - 1) / L.regions_per_wave;
    A.id_map = d.T.rterm;
    L.wg_sums = 0;
    // (every region's count is written by the wave that owns the region: no memset)
    bool split = !A.fused_only && use_split_form(d.T);
    if (split) {
        L.n_slices = A.n_slices = 1; // (the verification kernel's grid is not the filter's)
        L.slice_slots = (uint32_t)(A.slice_slots = A.scratch_cap);
        // a wave's slice holds one candidate per 8 units of its span (the filter passes ~2 % on selective
        // dictionaries); a haystack that needs more is redone with the fused kernel
        const uint64_t per_wave = (uint64_t)L.regions_per_wave * R / (uint64_t)std::max<int64_t>(1, tunables().split_cand_div) + 2 * 1024;
        if (per_wave * waves_used >= (1ull << 32)) split = false;
        else {
            L.cands_per_wave = (uint32_t)per_wave;
            if ((rc = d.cands.ensure(per_wave * waves_used * 4 + 64))) return rc;
            if ((rc = d.region_cands.ensure((size_t)L.n_regions * 8))) return rc;
            L.d_cands = (uint32_t *)d.cands.p;
            L.d_region_cands = (uint2 *)d.region_cands.p;
            HIP_TRY(hipMemsetAsync(d.region_cands.p, 0, (size_t)L.n_regions * 8, r.stream)); // unwritten = no candidates
            L.verify_grid = (int)std::min<uint64_t>(((uint64_t)L.n_regions + 3) / 4, (uint64_t)d.n_cu * 8);
            // every verification wave may hold one partly used reservation of scratch slots
            const uint64_t need = std::min<uint64_t>(std::max<uint64_t>(r.cap, 1) + (uint64_t)L.verify_grid * 4 * tile_reserve_slots(),
                                                     0xffffffe0ull);
            if (need > L.cap) {
                if ((rc = d.scratch.ensure(need * sizeof(ScratchRec)))) return rc;
                L.cap = A.scratch_cap = need;
                L.slice_slots = (uint32_t)(A.slice_slots = A.scratch_cap);
                L.d_scratch = (ScratchRec *)d.scratch.p;
            }
        }
    }
    // one finalize launch instead of three (prefix-sum kernels + permute) when a scratch slice is a workgroup: the scan
    // kernel leaves every workgroup's record count next to its slot counter and the permute pass (k_permute_wg) derives
    // its offsets from those and the region counts of its own workgroup.  (kSelFinalizeLaunches: the old way)
    const bool fused_finalize = !split && A.n_slices == (uint32_t)L.grid && L.grid <= kMaxSlices &&
                                (uint64_t)waves_per_block * L.regions_per_wave <= kPermuteWgRegions && !(L.debug & kSelFinalizeLaunches);
    if (fused_finalize) A.order = AllScan::Order::PermuteWg;
    L.wg_sums = fused_finalize ? 1u : 0u;
    A.regions_per_wg = (uint32_t)waves_per_block * L.regions_per_wave;
    // The fused tail (TileLaunch::fused_tail): no finalize launch at all -- the scan's workgroups put their own slices in order
    // when their spans are scanned, each behind the counts of the workgroups that started before it, and the last one
    // reports the call's result.  Same conditions as the one-launch finalize.  Tunable tile_form bit 1: never (A/B, tests).
    const bool fused = fused_finalize && !(tunables().tile_form & 1);
    if (fused) {
        L.wg_sums = 0; // (the workgroups' sums go through their own LDS)
        if ((rc = set_fused_tail(L, r, A, A.id_map))) return rc;
    }
    // the kernel's form, once: its dynamic LDS and its name (the second level's predicate reads L.region_units and L.debug)
    const std::optional<TileForm> form = choose_tile_form(d.T, L, split);
    if (!form) HIP_TRY(hipErrorInvalidValue);
    L.lds_bytes = form->lds;
    tile_form_name(*form, A.kname);
    return launch_regions(L, r, A, !split, fused, false, [&]() -> int {
        if (split) {
            if (r.profiled) HIP_TRY(hipEventRecord(r.ev[0], r.stream));
            HIP_TRY(launch_ac_filter(d.T, L, *form, r.stream));
            if (r.profiled) HIP_TRY(hipEventRecord(r.ev[1], r.stream)); // the verification is accounted with the ordering
            HIP_TRY(launch_ac_verify(d.T, L, r.stream));
        } else {
            HIP_TRY(launch_ac_tile(d.T, L, *form, r.stream));
        }
        return ACGPU_OK;
    });
}

// ALL: the general DFA chunk scan (any alphabet, any keyword lengths).
int setup_dfa_scan(acgpu_automaton *a, DeviceState &d, CallRecord &r, AllScan &A) {
    const HostTables &t = a->t;
    const acgpu_shard *sh = &r.shard;
    const uint64_t own_len = sh->own_end - sh->own_begin;
    const uint32_t halo = t.max_len > 0 ? t.max_len - 1 : 0;
    int rc;
    ScanLaunch L{};
    L.block = scan_block_threads();
    L.grid = d.n_cu * (int)std::max<int64_t>(1, tunables().blocks_per_cu);
    // kSelDfaOneChain: the one-chain kernel of rounds 1-3 (A/B); kSelDfaNoGlobal (ablation build): no lookups in global memory
    L.debug = ((tunables().tile_debug & kSelDfaOneChain) ? kScanOneChain : 0u) | ((tunables().tile_debug & kSelDfaNoGlobal) ? 4u : 0u);
    if (sh->n_units < 64) L.debug |= kScanOneChain; // (k_ac_dfa takes the buffer's last vector whole: the old kernel reads unit by unit)
    const uint64_t lanes = (uint64_t)L.grid * L.block * (uint64_t)((L.debug & kScanOneChain) ? 1 : std::max(1, scan_chains(d.T)));
    uint64_t C = tunables().chunk_units > 0 ? (uint64_t)tunables().chunk_units
                                            : std::max<uint64_t>({(own_len + lanes - 1) / lanes, 256, 16ull * halo});
    C = std::max<uint32_t>(8, round_up8(C));
    L.chunk_units = (uint32_t)C;
    L.n_chunks = (uint32_t)((own_len + C - 1) / C);
    // do not launch more workgroups than there are chunks
    L.grid = (int)std::min<uint64_t>((uint64_t)L.grid, ((uint64_t)L.n_chunks + L.block - 1) / L.block);
    L.d_hay = sh->d_hay;
    L.n_units = (uint32_t)sh->n_units;
    L.own_begin = (uint32_t)sh->own_begin;
    L.own_end = (uint32_t)sh->own_end;
    L.cap = A.scratch_cap; // every slot below min(counter, scratch_cap) must be written: the permute pass reads them all
    L.lds_bytes = scan_queue_bytes(L.block) + (size_t)d.T.lds_entries * t.entry_bytes + 16;
    if ((rc = ensure_scan_buffers(d, L.n_chunks))) return rc;
    L.d_scratch = (ScratchRec *)d.scratch.p;
    L.d_counter = A.counters;
    L.d_chunk_counts = (uint32_t *)d.chunk_counts.p;
    const std::optional<DfaForm> form = choose_dfa_form(d.T, L);
    if (!form) HIP_TRY(hipErrorInvalidValue);
    dfa_form_name(*form, A.kname);
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[0], r.stream));
    HIP_TRY(launch_ac_scan(d.T, L, *form, r.stream));
    if (r.profiled) HIP_TRY(hipEventRecord(r.ev[1], r.stream));
    A.n_chunks = L.n_chunks;
    A.chunk_units = L.chunk_units;
    A.scanned = own_len + (uint64_t)L.n_chunks * halo;
    return ACGPU_OK;
}

// The ordering stage behind a scan form: the fused tail has done it inside the scan; otherwise the prefix sum of the chunk
// counts (k_permute_wg derives its own) and the pass that puts the records in order, which reports {record count, overflow
// word} into the record's pinned slot, clears the word and zeroes the other set of slot counters for the next call: no copy or
// memset operations on the stream.
int order_records(DeviceState &d, CallRecord &r, const AllScan &A) {
    const int cs = d.cset;
    if (A.order == AllScan::Order::FusedTail) { // nothing behind the scan kernel: it has ordered its records, reports the count and has zeroed the other counter set
        d.cclean[1 - cs] = true;
        d.cset = 1 - cs;
        r.one_kernel = true;
        return close_call(r, CallForm::FusedTail, A.kname, A.scanned, /*done_is_ev2=*/true);
    }
    int rc;
    const hipStream_t stream = r.stream;
    if (A.order != AllScan::Order::PermuteWg)
        HIP_TRY(launch_exclusive_scan((const uint32_t *)d.chunk_counts.p, A.n_chunks, (uint64_t *)d.offsets.p,
                                      (uint64_t *)d.scan_tmp.p, stream));
    unsigned long long *d_slot = nullptr;
    if ((rc = slot_on_device(r, &d_slot))) return rc;
    const PermuteTail tail{d_slot, scan_total(d, A.n_chunks), A.overflow_word, A.counters_next,
                           reinterpret_cast<acgpu_device_result *>(r.shard.d_result)};
    // (k_ww_compact and k_permute_wg are one kernel that ends the call: profiled, it delivers its own end timestamp; a ticket's
    // completion is that timestamp too, profiled or not -- no marker packet behind the call)
    const bool ext_stop = (A.order == AllScan::Order::WwCompact || A.order == AllScan::Order::PermuteWg) && (r.profiled || r.done);
    if (A.order == AllScan::Order::WwCompact)
        HIP_TRY(launch_ww_compact((const int32_t *)d.ww_recs.p, A.ww_region_cap, (const uint32_t *)d.chunk_counts.p, (const uint64_t *)d.offsets.p,
                                  A.n_chunks, r.record_kind, r.d_out, r.cap, stream, &tail, ext_stop ? r.ev[2] : nullptr));
    else if (A.order == AllScan::Order::PermuteWg)
        HIP_TRY(launch_permute_wg((const ScratchRec *)d.scratch.p, A.counters, A.n_slices, A.slice_slots, (const uint32_t *)d.chunk_counts.p,
                                  A.n_chunks, A.regions_per_wg, A.perm_base, A.chunk_units, r.record_kind, r.d_out, r.cap, A.id_map, stream, &tail,
                                  ext_stop ? r.ev[2] : nullptr));
    else
        HIP_TRY(launch_permute((const ScratchRec *)d.scratch.p, A.counters, A.n_slices, A.slice_slots,
                               (const uint64_t *)d.offsets.p, A.perm_base, A.chunk_units, A.by_start, r.record_kind, r.d_out, r.cap, A.id_map,
                               stream, &tail));
    d.cclean[1 - cs] = true; // zeroed by the pass just launched
    d.cset = 1 - cs;
    if (r.profiled && !ext_stop) HIP_TRY(hipEventRecord(r.ev[2], stream));
    return close_call(r, CallForm::Ordered, A.kname, A.scanned, ext_stop);
}

} // namespace

namespace acgpu { // (what acgpu_calls.h and acgpu_host.h declare: described there)

bool use_tile_kernel(const HostTables &t) {
    if (t.filt_k == 0) return false;
    const int64_t f = tunables().force_kernel;
    if (f == 1) return false;
    if (f == 2 || f == 3) return true;
    // The packed forms (range classes, folded or merged ranges) always win: with K = 4 even where the filter passes everything --
    // the 235 886-word list of the reference's README (52 letters in two ranges, the single letters among the keywords: every
    // position ends a keyword) 23.5 against 62.9 ms per 2^28 units, both bound by 412 M records (tools/readme_shapes.py).
    if (t.range_cls || t.fold_range) return true;
    // The class-table forms (bucketed classes: more than 63 distinct units; or up to 63 classes that no range arithmetic
    // gives) run the scalar filter -- three LDS reads per unit and, bucketed, a hash probe of its K units per candidate.
    // Against them (tools/wide_alphabets.py, 2^28 units, round 4): a DFA table that stays in the L2 cache makes k_ac_dfa the
    // faster kernel as soon as the filter passes more than a tenth of the positions (300 CJK units, 2 k keywords of 2-4
    // units, a 3.6 MB table, density 0.17: 0.65 against 1.06 ms; config 2's phrases case-insensitive, density 0.24: 0.60
    // against 1.04 ms; density 0.08: 0.39 ms for the tile kernel), while a table far beyond the cache (3000 CJK units) loses
    // to the tile kernel whatever the filter passes (20 k keywords of 2-8 units, density 0.54: 2.97 against 5.19 ms; of 1-4
    // units, 1.03: 10.6 against 25.8 ms, 218 M records; 20 k of 2 units, K = 2: 2.63 against 3.92 ms; only 100 k keywords of
    // 2-3 units went the other way, 6.8 against 5.35 ms), as does the sparse form (4.7 ms and more).
    const uint64_t table_bytes = t.dense ? (uint64_t)t.n_states * t.n_cls * (uint64_t)t.entry_bytes : ~0ull;
    if (table_bytes <= (6ull << 20)) return t.filt_density <= 0.1;
    return true;
}

int enqueue_all(acgpu_automaton *a, DeviceState &d, CallRecord &r, int level) {
    const HostTables &t = a->t;
    const acgpu_shard *sh = &r.shard;
    const uint64_t own_len = sh->own_end - sh->own_begin;
    const bool ww = t.mode == ACGPU_MODE_WHOLEWORD;
    const uint32_t halo = ww ? 1u : (t.max_len > 0 ? t.max_len - 1 : 0);
    if (!sh->text_begin && sh->own_begin < halo) return ACGPU_E_INVALID; // left halo too short
    if (ww && !sh->text_end && sh->n_units - sh->own_end < (uint64_t)t.max_len + 1) return ACGPU_E_INVALID; // right halo
    r.level = level;
    if (own_len == 0 || t.n_states <= 1) return enqueue_empty(r, 0);
    int rc;
    uint32_t st_hot = 0;
    if ((rc = choose_states_form(a, d, r, &st_hot))) return rc;
    if (st_hot) {
        // (a counting call: its direct form; without room for the visit words, or with the tunable count_form against it, the records form)
        rc = enqueue_states(a, d, r, st_hot, r.counting && d.count->direct_ok);
        if (rc != ACGPU_E_NOMEM) return rc; // (no room for 4 bytes of state per unit -- before anything was launched: the tile kernel it is)
    }
    AllScan A;
    const DevTables Tf = r.folded ? folded_tables(d) : DevTables{};
    A.T = r.folded ? &Tf : &d.T;
    A.fused_only = level > 0;
    const size_t counter_bytes = (size_t)kMaxSlices * kCounterStride * 8; // one set; layout: [set 0][set 1][overflow word]
    if ((rc = d.counter.ensure(2 * counter_bytes + 64))) return rc;
    if (d.counter.p != d.counter_seen) {
        d.counter_seen = d.counter.p;
        d.cclean[0] = d.cclean[1] = false;
        HIP_TRY(hipMemsetAsync((char *)d.counter.p + 2 * counter_bytes, 0, 64, r.stream));
    }
    const int cs = d.cset;
    A.counters = (unsigned long long *)((char *)d.counter.p + (size_t)cs * counter_bytes);
    A.counters_next = (unsigned long long *)((char *)d.counter.p + (size_t)(1 - cs) * counter_bytes);
    A.overflow_word = (uint32_t *)((char *)d.counter.p + 2 * counter_bytes);
    // the tile kernel reserves scratch slots 256 at a time per wave: head-room for the unused tails; a quarter more than
    // the caller's capacity so that the scratch slices (one per workgroup) tolerate unevenly spread matches
    A.scratch_cap = std::min<uint64_t>(
        std::max<uint64_t>(r.cap, 1) + r.cap / 4 +
            (uint64_t)d.n_cu * (ww ? ww_blocks_per_cu() : 1) * (tile_block_threads() / 64) * tile_reserve_slots(),
        0xffffffe0ull);
    if ((rc = d.scratch.ensure(A.scratch_cap * sizeof(ScratchRec)))) return rc;
    if (!d.cclean[cs]) HIP_TRY(hipMemsetAsync(A.counters, 0, counter_bytes, r.stream)); // (normally zeroed by the previous call's permute pass)
    // from here on this set is in use; the other set only counts as clean once the permute pass that zeroes it has been
    // launched (order_records) -- an early error return leaves both marked dirty and the next call clears its set itself
    d.cclean[0] = d.cclean[1] = false;
    A.slice_slots = A.scratch_cap;
    A.perm_base = (uint32_t)sh->own_begin;
    if (ww) rc = setup_ww_scan(a, d, r, A);
    else if (use_tile_kernel(t)) rc = setup_tile_scan(a, d, r, A);
    else rc = setup_dfa_scan(a, d, r, A);
    if (rc) return rc;
    return order_records(d, r, A);
}

} // namespace acgpu
