// acgpu_api.hip -- what is left of the C ABI of include/acgpu.h once every feature has its own unit: automaton lifetime, errors,
// the tunables, the readers of the built tables, and the benchmark's probe and text generators.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "acgpu_calls.h"

using namespace acgpu;

namespace acgpu {
thread_local int g_last_hip_error = 0;
}

extern "C" {

uint32_t acgpu_abi_version(void) { return ACGPU_ABI_VERSION; }

int acgpu_last_hip_error(void) { return g_last_hip_error; }

const char *acgpu_strerror(int code) {
    switch (code) {
    case ACGPU_OK: return "ok";
    case ACGPU_E_INVALID: return "invalid argument";
    case ACGPU_E_NONWORD: return "keyword contains non-word characters";
    case ACGPU_E_NOMEM: return "out of memory";
    case ACGPU_E_OVERFLOW: return "output capacity too small";
    case ACGPU_E_HIP: return "HIP runtime error";
    case ACGPU_E_NODEVICE: return "no HIP device";
    case ACGPU_E_UNSUPPORTED: return "unsupported";
    case ACGPU_E_ENCODING: return "haystack is not well-formed UTF-8";
    default: return "unknown error";
    }
}

int64_t acgpu_set_tunable(const char *name, int64_t value) {
    if (!name) return -1;
    if (!std::strcmp(name, "ablation_build")) { // (read only) 1: built with -DACGPU_ABLATION, the ablation bits of tile_debug work
#ifdef ACGPU_ABLATION
        return 1;
#else
        return 0;
#endif
    }
    Tunables &t = tunables();
    std::atomic<int64_t> *slot = nullptr;
#define ACGPU_TUNABLE_LOOKUP(knob, dflt) if (!slot && !std::strcmp(name, #knob)) slot = &t.knob;
    ACGPU_TUNABLES(ACGPU_TUNABLE_LOOKUP)
#undef ACGPU_TUNABLE_LOOKUP
    if (!slot) return -1;
    return slot->exchange(value, std::memory_order_relaxed);
}

int acgpu_build(int mode, const uint16_t *kw_units, const uint64_t *kw_off, uint32_t n_kw, int case_sensitive,
                const uint16_t *lower_tbl, const uint8_t *wordchar_tbl, acgpu_automaton **out, int64_t *bad_keyword) {
    if (!out) return ACGPU_E_INVALID;
    *out = nullptr;
    acgpu_automaton *a = new (std::nothrow) acgpu_automaton();
    if (!a) return ACGPU_E_NOMEM;
    int rc;
    try {
        rc = build_tables(mode, kw_units, kw_off, n_kw, case_sensitive, lower_tbl, wordchar_tbl, a->t, bad_keyword);
    } catch (const std::bad_alloc &) {
        rc = ACGPU_E_NOMEM;
    } catch (...) {
        rc = ACGPU_E_INVALID;
    }
    if (rc != ACGPU_OK) {
        delete a;
        return rc;
    }
    a->n_given = n_kw;
    *out = a;
    return ACGPU_OK;
}

void acgpu_free(acgpu_automaton *a) {
    if (!a) return;
    { // streams still open on it (include/acgpu.h asks for them to be closed first): detached -- their feeds return
      // ACGPU_E_INVALID from now on and acgpu_stream_close touches nothing of the automaton
        std::lock_guard<std::mutex> l(a->mu);
        for (acgpu_stream *s : a->open_streams) acgpu_stream_detach(s);
        a->open_streams.clear();
        for (acgpu_cursor *c : a->open_cursors) acgpu_cursor_detach(c); // (the same for cursors)
        a->open_cursors.clear();
    }
    int cur = -1;
    bool have = hipGetDevice(&cur) == hipSuccess;
    for (auto &kv : a->dev) {
        if (have) (void)hipSetDevice(kv.first.first);
        kv.second.reset();
    }
    for (auto &b : a->stream_cache) {
        if (have) (void)hipSetDevice(b.device);
        b.release();
    }
    if (have) (void)hipSetDevice(cur);
    delete a;
}

int acgpu_get_info(const acgpu_automaton *a, acgpu_info *info) {
    if (!a || !info) return ACGPU_E_INVALID;
    const HostTables &t = a->t;
    std::memset(info, 0, sizeof(*info));
    info->abi_version = ACGPU_ABI_VERSION;
    info->mode = (uint32_t)t.mode;
    info->case_sensitive = t.cs;
    info->n_states = t.n_states;
    info->n_classes = t.n_cls;
    info->n_keywords = t.n_kw;
    info->min_keyword_len = t.min_len;
    info->max_keyword_len = t.max_len;
    info->dense = t.dense;
    info->entry_bytes = t.entry_bytes;
    info->table_bytes = t.dense ? (uint64_t)t.dfa.size() * t.entry_bytes : (uint64_t)t.hkeys.size() * 12 + (uint64_t)t.n_states * 4;
    info->lds_states = lds_states_for(t);
    info->fold_consistent = t.fold_consistent;
    info->filter_k = t.filt_k;
    info->filter_bits = (uint32_t)(t.filt_bits.size() * 32);
    info->tile_kernel = t.mode == ACGPU_MODE_LONGEST ? (filter_is_selective(t) && tunables().force_kernel != 1) : use_tile_kernel(t);
    info->filter_density = (float)t.filt_density;
    info->fold_clean = t.fold_clean;
    return ACGPU_OK;
}

int acgpu_debug_tables(const acgpu_automaton *a, uint16_t *cls_lut, uint32_t *dfa, uint32_t *out_len, uint32_t *out_link,
                       uint32_t *out_id, uint32_t *depth, uint32_t *first_out_state) {
    if (!a) return ACGPU_E_INVALID;
    const HostTables &t = a->t;
    if (cls_lut) std::memcpy(cls_lut, t.cls_lut.data(), 65536 * sizeof(uint16_t));
    if (dfa) {
        if (!t.dense) return ACGPU_E_UNSUPPORTED;
        std::memcpy(dfa, t.dfa.data(), t.dfa.size() * sizeof(uint32_t));
    }
    if (out_len) std::memcpy(out_len, t.out_len.data(), t.n_states * sizeof(uint32_t));
    if (out_link) std::memcpy(out_link, t.out_link.data(), t.n_states * sizeof(uint32_t));
    if (out_id) std::memcpy(out_id, t.out_id.data(), t.n_states * sizeof(uint32_t));
    if (depth) std::memcpy(depth, t.depth.data(), t.n_states * sizeof(uint32_t));
    if (first_out_state) *first_out_state = t.first_out;
    return ACGPU_OK;
}

int acgpu_debug_states(const acgpu_automaton *a, uint64_t sizes[6], uint32_t *rows, uint32_t *nodes, uint32_t *mask, uint32_t *out,
                       uint32_t *ids) {
    if (!a || !sizes) return ACGPU_E_INVALID;
    const HostTables &t = a->t;
    const bool have = t.hy_n_states != 0 && (t.mode == ACGPU_MODE_ALL || t.mode == ACGPU_MODE_SHORTEST);
    sizes[0] = have ? t.hy_n_states : 0;
    sizes[1] = have ? t.hy_n_dense : 0;
    sizes[2] = t.n_cls;
    sizes[3] = have ? t.hy_dense.size() : 0;
    sizes[4] = have ? t.hy_nodes.size() : 0;
    sizes[5] = have ? t.hy_ids.size() : 0;
    if (!have) return ACGPU_OK;
    if (rows) std::memcpy(rows, t.hy_dense.data(), t.hy_dense.size() * sizeof(uint32_t));
    if (nodes) std::memcpy(nodes, t.hy_nodes.data(), t.hy_nodes.size() * sizeof(uint32_t));
    if (mask) std::memcpy(mask, t.hy_mask.data(), t.hy_mask.size() * sizeof(uint32_t));
    if (out) std::memcpy(out, t.hy_out.data(), t.hy_out.size() * sizeof(uint32_t));
    if (ids) std::memcpy(ids, t.hy_ids.data(), t.hy_ids.size() * sizeof(uint32_t));
    return ACGPU_OK;
}

int acgpu_debug_wordhash_perfect(const acgpu_automaton *a, uint32_t sizes[3], uint32_t *slots, uint16_t *disp, uint8_t *bp_idx,
                                 uint8_t *bp_pages, uint16_t *bp_delta) {
    if (!a || !sizes) return ACGPU_E_INVALID;
    const HostTables &t = a->t;
    if (t.mode != ACGPU_MODE_WHOLEWORD) return ACGPU_E_UNSUPPORTED;
    sizes[0] = t.ww_ph_n;
    sizes[1] = t.ww_ph_buckets;
    sizes[2] = t.ww_bp_n;
    if (slots && !t.ww_ph.empty()) std::memcpy(slots, t.ww_ph.data(), t.ww_ph.size() * sizeof(uint32_t));
    if (disp && !t.ww_ph_disp.empty()) std::memcpy(disp, t.ww_ph_disp.data(), (size_t)t.ww_ph_buckets * sizeof(uint16_t));
    if (bp_idx && t.ww_bp_n) std::memcpy(bp_idx, t.ww_bp_idx.data(), 256);
    if (bp_pages && t.ww_bp_n) std::memcpy(bp_pages, t.ww_bp_pages.data(), t.ww_bp_pages.size());
    if (bp_delta && t.ww_bp_n) std::memcpy(bp_delta, t.ww_bp_delta.data(), 128 * sizeof(uint16_t));
    return ACGPU_OK;
}

int acgpu_debug_wordhash(const acgpu_automaton *a, uint32_t *n_slots, uint32_t *slots, uint64_t *n_rec_words, uint32_t *recs,
                         uint8_t *fold_pgidx, uint32_t *n_pages, uint16_t *fold_pages, uint32_t *seed) {
    if (!a) return ACGPU_E_INVALID;
    const HostTables &t = a->t;
    if (t.mode != ACGPU_MODE_WHOLEWORD && t.mode != ACGPU_MODE_WWLONGEST) return ACGPU_E_UNSUPPORTED;
    if (n_slots) *n_slots = (uint32_t)(t.ww_fat.size() / 8);
    if (slots) std::memcpy(slots, t.ww_fat.data(), t.ww_fat.size() * sizeof(uint32_t));
    if (n_rec_words) *n_rec_words = t.ww_recs.size();
    if (recs) std::memcpy(recs, t.ww_recs.data(), t.ww_recs.size() * sizeof(uint32_t));
    if (fold_pgidx) std::memcpy(fold_pgidx, t.fold_pgidx.data(), 256);
    if (n_pages) *n_pages = t.fold_n_pages;
    if (fold_pages) std::memcpy(fold_pages, t.fold_pages.data(), t.fold_pages.size() * sizeof(uint16_t));
    if (seed) *seed = t.ww_seed;
    return ACGPU_OK;
}

int acgpu_stream_probe(const void *d_buf, uint64_t n_bytes, void *stream_, int repeats, int pattern, float *ms_median) {
    if (pattern != 0 && pattern != 1) return ACGPU_E_INVALID;
    if (!d_buf || !ms_median || ((uintptr_t)d_buf & 15) || n_bytes < (1ull << 20) || repeats < 1 || repeats > 64) return ACGPU_E_INVALID;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return ACGPU_E_HIP; }
    unsigned *d_sink = nullptr;
    int rc = ACGPU_OK;
    std::vector<float> ms;
    int dev = 0, n_cu = 256;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        n_cu = prop.multiProcessorCount;
    if (hipMalloc((void **)&d_sink, 64) != hipSuccess) rc = ACGPU_E_NOMEM;
    for (int r = 0; rc == ACGPU_OK && r <= repeats; ++r) { // (the first run is a warm-up)
        float t = 0;
        if (hipEventRecord(e0, stream) != hipSuccess || launch_stream_probe(d_buf, n_bytes, n_cu, d_sink, pattern, stream) != hipSuccess ||
            hipEventRecord(e1, stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
            hipEventElapsedTime(&t, e0, e1) != hipSuccess) {
            g_last_hip_error = (int)hipGetLastError();
            rc = ACGPU_E_HIP;
        } else if (r) ms.push_back(t);
    }
    if (d_sink) (void)hipFree(d_sink);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc != ACGPU_OK) return rc;
    std::sort(ms.begin(), ms.end());
    *ms_median = ms[ms.size() / 2];
    return ACGPU_OK;
}

int acgpu_synth_fill(uint16_t *d_dst, uint64_t n_units, uint64_t start_index, uint64_t seed, const uint16_t *table,
                     uint32_t table_len, void *stream) {
    if ((n_units && !d_dst) || !table || table_len == 0 || table_len > 64) return ACGPU_E_INVALID;
    HIP_TRY(launch_synth_fill(d_dst, n_units, start_index, seed, table, table_len, reinterpret_cast<hipStream_t>(stream)));
    return ACGPU_OK;
}

int acgpu_synth_tokens(uint16_t *d_dst, uint64_t n_units, uint64_t seed, const uint16_t *kw_units, const uint64_t *kw_off,
                       uint32_t n_kw, const uint16_t *swapcase_tbl, void *stream_) {
    if ((n_units && !d_dst) || (n_kw && (!kw_units || !kw_off))) return ACGPU_E_INVALID;
    if (n_units == 0) return ACGPU_OK;
    // a token is a word -- of the dictionary, or a random one of 2..12 units -- plus 1..3 separators: its shortest form bounds
    // the number of tokens that cover the haystack (a dictionary with a 1-unit or empty word makes 2- and 1-unit tokens)
    uint64_t min_word = 2;
    for (uint32_t i = 0; i < n_kw; ++i) min_word = std::min<uint64_t>(min_word, kw_off[i + 1] - kw_off[i]);
    const uint64_t n_tokens64 = n_units / (min_word + 1) + 2;
    if (n_tokens64 >= (1ull << 32)) return ACGPU_E_INVALID;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    // the benchmark's scripts and separators (ahocorasick_amd/synth.py: _SCRIPTS, _SEPARATORS)
    static const uint16_t ranges[][2] = {{0x41, 0x5A}, {0x61, 0x7A}, {0xC0, 0xD6}, {0xD8, 0xF6}, {0xF8, 0xFF}, // latin
                                         {0x0391, 0x03A1}, {0x03A3, 0x03A9}, {0x03B1, 0x03C9},                // greek
                                         {0x0410, 0x044F},                                                    // cyrillic
                                         {0x4E00, 0x9FA5},                                                    // cjk
                                         {0xAC00, 0xD7A3},                                                    // hangul
                                         {0x0621, 0x063A}, {0x0641, 0x064A}};                                 // arabic
    static const int script_first[7] = {0, 5, 8, 9, 10, 11, 13};
    static const uint16_t seps[6] = {0x20, ',', '.', 0x0A, 0x3002, 0x2014};
    std::vector<uint16_t> scripts;
    uint32_t script_off[7];
    std::vector<uint32_t> off32;
    try {
        for (int sc = 0; sc < 6; ++sc) {
            script_off[sc] = (uint32_t)scripts.size();
            for (int r = script_first[sc]; r < script_first[sc + 1]; ++r)
                for (uint32_t u = ranges[r][0]; u <= ranges[r][1]; ++u) scripts.push_back((uint16_t)u);
        }
        script_off[6] = (uint32_t)scripts.size();
        off32.resize((size_t)n_kw + 1);
        for (uint32_t i = 0; i <= n_kw; ++i) {
            const uint64_t o = n_kw ? kw_off[i] - kw_off[0] : 0;
            if (o >= (1ull << 32)) return ACGPU_E_INVALID;
            off32[i] = (uint32_t)o;
        }
    } catch (...) {
        return ACGPU_E_NOMEM;
    }
    const uint32_t n_tokens = (uint32_t)n_tokens64; // these cover the haystack
    const size_t kw_bytes = n_kw ? (size_t)off32[n_kw] * 2 : 0;
    DevBuf b_kw, b_off, b_sw, b_sc, b_len, b_start, b_tmp;
    auto release = [&]() { b_kw.release(); b_off.release(); b_sw.release(); b_sc.release(); b_len.release(); b_start.release(); b_tmp.release(); };
    int rc = ACGPU_OK;
    if ((rc = b_kw.ensure(kw_bytes + 16)) || (rc = b_off.ensure(off32.size() * 4 + 16)) || (rc = b_sc.ensure(scripts.size() * 2 + 16)) ||
        (rc = b_len.ensure((size_t)n_tokens * 4 + 16)) || (rc = b_start.ensure((size_t)n_tokens * 8 + 16)) ||
        (rc = b_tmp.ensure(((size_t)n_tokens / 2048 + 2) * 8 + 16)) || (swapcase_tbl && (rc = b_sw.ensure(65536 * 2)))) {
        release();
        return rc;
    }
    hipError_t e = hipSuccess;
    if (kw_bytes) e = hipMemcpy(b_kw.p, kw_units + kw_off[0], kw_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(b_off.p, off32.data(), off32.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(b_sc.p, scripts.data(), scripts.size() * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess && swapcase_tbl) e = hipMemcpy(b_sw.p, swapcase_tbl, 65536 * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = launch_token_stream(d_dst, n_units, seed, (const uint16_t *)b_kw.p, (const uint32_t *)b_off.p, n_kw,
                                swapcase_tbl ? (const uint16_t *)b_sw.p : nullptr, (const uint16_t *)b_sc.p, script_off, seps, n_tokens,
                                (uint32_t *)b_len.p, (uint64_t *)b_start.p, (uint64_t *)b_tmp.p, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream); // (the scratch is released below)
    release();
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? ACGPU_E_NOMEM : ACGPU_E_HIP;
    }
    return ACGPU_OK;
}

} // extern "C"
