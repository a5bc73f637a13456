// acgpu_tables.hip -- residency: the upload of an automaton's tables to a device on the first call there, the scratch pool that
// is created with them, and the tables as a call sees them (the tunables' part, the folded word-character tables).
#include <algorithm>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "acgpu_calls.h"

using namespace acgpu;

namespace {

template <typename T>
int upload(DeviceState &d, const std::vector<T> &v, const T **out) {
    d.table_allocs.emplace_back();
    void *&p = d.table_allocs.back().h;
    size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    HIP_TRY(hipMalloc(&p, bytes));
    if (!v.empty()) HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = reinterpret_cast<const T *>(p);
    return ACGPU_OK;
}

// caller holds a->mu
int ensure_device(acgpu_automaton *a, DeviceState **out, int lane) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    auto it = a->dev.find({dev, lane});
    if (it != a->dev.end()) {
        *out = it->second.get();
        return ACGPU_OK;
    }
    std::unique_ptr<DeviceState> d(new (std::nothrow) DeviceState());
    if (!d) return ACGPU_E_NOMEM;
    d->device = dev;
    d->lane = lane;
    if (lane > 0) {
        HIP_TRY(hipStreamCreateWithFlags(&d->lane_stream.h, hipStreamNonBlocking));
        d->call_stream = d->lane_stream;
    }
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    d->n_cu = d->n_cu_phys = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const HostTables &t = a->t;
    DevTables &T = d->T;
    int rc;
    if ((rc = upload(*d, t.cls_lut, &T.cls_lut))) return rc;
    if ((rc = upload(*d, t.lower, &T.lower))) return rc;
    if ((rc = upload(*d, t.wflags, &T.wflags))) return rc;
    if ((rc = upload(*d, t.wbits, &T.wbits))) return rc;
    if (!t.fold_consistent) {
        if ((rc = upload(*d, t.wflags_f, &d->wflags_f))) return rc;
        if ((rc = upload(*d, t.wbits_f, &d->wbits_f))) return rc;
    }
    if ((rc = upload(*d, t.out_len, &T.out_len))) return rc;
    if ((rc = upload(*d, t.out_link, &T.out_link))) return rc;
    if ((rc = upload(*d, t.out_id, &T.out_id))) return rc;
    if ((rc = upload(*d, t.fail, &T.fail))) return rc;
    if ((rc = upload(*d, t.depth, &T.depth))) return rc;
    if ((rc = upload(*d, t.term_id, &T.term_id))) return rc;
    if ((rc = upload(*d, t.hkeys, &T.hkeys))) return rc;
    if ((rc = upload(*d, t.hvals, &T.hvals))) return rc;
    T.dfa = nullptr;
    if (t.dense) {
        if (t.entry_bytes == 2) {
            std::vector<uint16_t> narrow(t.dfa.size());
            for (size_t i = 0; i < t.dfa.size(); i++) narrow[i] = (uint16_t)t.dfa[i];
            const uint16_t *p;
            if ((rc = upload(*d, narrow, &p))) return rc;
            T.dfa = p;
        } else {
            const uint32_t *p;
            if ((rc = upload(*d, t.dfa, &p))) return rc;
            T.dfa = p;
        }
    }
    T.root_tab = nullptr; T.root_b = t.root_b; T.root_rk = t.root_rk;
    if (t.root_b && (rc = upload(*d, t.root_tab, &T.root_tab))) return rc;
    T.bits_tab = nullptr; T.bits_rk = t.bits_rk;
    if (t.bits_rk && (rc = upload(*d, t.bits_tab, &T.bits_tab))) return rc;
    T.bits_idkeys = nullptr; T.bits_idmask = t.bits_idmask;
    if (t.bits_rk && !t.bits_idkeys.empty() && (rc = upload(*d, t.bits_idkeys, &T.bits_idkeys))) return rc;
    T.hy_dense = T.hy_nodes = T.hy_mask = T.hy_out = T.hy_ids = nullptr;
    T.hy_n_dense = t.hy_n_dense; T.hy_n_states = t.hy_n_states;
    if (t.hy_n_states) {
        { // one allocation, rows first (padded to 16 bytes), nodes behind them: k_ac_states reads either with ONE 16-byte gather
            std::vector<uint32_t> all(t.hy_dense);
            all.resize((all.size() + 3) & ~(size_t)3, 0u);
            const size_t node_at = all.size();
            all.insert(all.end(), t.hy_nodes.begin(), t.hy_nodes.end());
            all.resize(all.size() + 4, 0u);
            if ((rc = upload(*d, all, &T.hy_dense))) return rc;
            T.hy_nodes = T.hy_dense + node_at;
        }
        if ((rc = upload(*d, t.hy_mask, &T.hy_mask))) return rc;
        if ((rc = upload(*d, t.hy_out, &T.hy_out))) return rc;
        if ((rc = upload(*d, t.hy_ids, &T.hy_ids))) return rc;
    }
    if ((rc = upload(*d, t.filt_bits, &T.filt_bits))) return rc;
    if ((rc = upload(*d, t.kgram_node, &T.kgram_node))) return rc;
    T.fold_range = t.fold_range; T.fr_base = t.fr_base; T.fr_span = t.fr_span; T.fr_base2 = t.fr_base2; T.fr_himask = t.fr_himask;
    T.fr_base3 = t.fr_base3; T.fr_base4 = t.fr_base4; T.fr_nr = t.fr_nr;
    T.l2_bloom = nullptr; T.l2_big = nullptr; T.l2_depth = 0;
    if (t.l2_depth) {
        if ((rc = upload(*d, t.l2_bloom, &T.l2_bloom))) return rc;
        if (!t.l2_big.empty() && (rc = upload(*d, t.l2_big, &T.l2_big))) return rc;
        T.l2_depth = t.l2_depth;
    }
    if ((rc = upload(*d, t.rterm, &T.rterm))) return rc;
    if ((rc = upload(*d, t.rtab, &T.rtab))) return rc;
    T.kshort = nullptr; T.ks_keys = nullptr; T.ks_vals = nullptr; T.ks_mask = t.ks_mask; T.has_short = t.has_short ? 1u : 0u;
    if (t.has_short && !t.kshort.empty() && (rc = upload(*d, t.kshort, &T.kshort))) return rc;
    if (t.has_short && !t.ks_keys.empty()) {
        if ((rc = upload(*d, t.ks_keys, &T.ks_keys))) return rc;
        if ((rc = upload(*d, t.ks_vals, &T.ks_vals))) return rc;
    }
    T.rdense = t.rdense;
    if ((rc = upload(*d, t.rhkeys, &T.rhkeys))) return rc;
    if ((rc = upload(*d, t.rhvals, &T.rhvals))) return rc;
    if ((rc = upload(*d, t.tile_lut, &T.tile_lut))) return rc;
    T.cls_pages = nullptr; T.cls_pages_bytes = (uint32_t)t.cls_pages.size();
    if (!t.cls_pages.empty() && (rc = upload(*d, t.cls_pages, &T.cls_pages))) return rc;
    T.dfa_pages = nullptr; T.dfa_pages_bytes = (uint32_t)t.dfa_pages.size() * 2;
    if (!t.dfa_pages.empty() && (rc = upload(*d, t.dfa_pages, &T.dfa_pages))) return rc;
    if ((rc = upload(*d, t.kg_keys, &T.kg_keys))) return rc;
    if ((rc = upload(*d, t.kg_vals, &T.kg_vals))) return rc;
    T.kg_mask = t.kg_mask; T.hashk = t.hashk;
    if ((rc = upload(*d, t.ww_fat, &T.ww_fat))) return rc;
    if ((rc = upload(*d, t.ww_recs, &T.ww_recs))) return rc;
    T.ww_bp_idx = nullptr; T.ww_bp_pages = nullptr; T.ww_bp_delta = nullptr; T.ww_bp_n = t.ww_bp_n; T.ww_bp_wbits = T.wbits;
    if (t.ww_bp_n && ((rc = upload(*d, t.ww_bp_idx, &T.ww_bp_idx)) || (rc = upload(*d, t.ww_bp_pages, &T.ww_bp_pages)) ||
                      (rc = upload(*d, t.ww_bp_delta, &T.ww_bp_delta)))) return rc;
    T.ww_ph = nullptr; T.ww_ph_disp = nullptr; T.ww_ph_n = t.ww_ph_n; T.ww_ph_buckets = t.ww_ph_buckets;
    if (!t.ww_ph.empty() && ((rc = upload(*d, t.ww_ph, &T.ww_ph)) || (rc = upload(*d, t.ww_ph_disp, &T.ww_ph_disp)))) return rc;
    if ((rc = upload(*d, t.fold_pgidx, &T.fold_pgidx))) return rc;
    if ((rc = upload(*d, t.fold_pages, &T.fold_pages))) return rc;
    if ((rc = upload(*d, t.ww_bloom, &T.ww_bloom))) return rc;
    T.ww_fat_mask = t.ww_fat_mask; T.ww_seed = t.ww_seed; T.fold_n_pages = t.fold_n_pages; T.fold_direct_n = t.fold_direct_n; T.ww_bloom_mask = t.ww_bloom_mask;
    T.rhmask = t.rhmask; T.filt_k = t.filt_k; T.filt_n = t.filt_n; T.filt_other = t.filt_other;
    T.filt_words = (uint32_t)t.filt_bits.size(); T.filt_row_bytes = t.filt_row_bytes;
    T.hmask = t.hmask;
    T.n_states = t.n_states; T.n_cls = t.n_cls; T.first_out = t.first_out; T.max_len = t.max_len; T.min_len = t.min_len;
    T.cls_base = t.cls_base; T.cls_span = t.cls_span; T.range_cls = t.range_cls; T.cs = t.cs; T.dense = t.dense;
    T.entry_bytes = (int32_t)t.entry_bytes;
    T.lds_entries = lds_states_for(t) * t.n_cls;
    HIP_TRY(hipHostMalloc((void **)&d->h_counter.h, 64, hipHostMallocDefault));
    for (auto &e : d->ev) HIP_TRY(hipEventCreate(&e.h));
    for (auto &tk : d->tickets) {
        for (auto &e : tk.ev) HIP_TRY(hipEventCreate(&e.h));
        HIP_TRY(hipEventCreateWithFlags(&tk.done.h, hipEventDisableTiming));
        HIP_TRY(hipHostMalloc((void **)&tk.h_count.h, 64, hipHostMallocDefault));
        tk.owner = d.get();
    }
    *out = d.get();
    a->dev[{dev, lane}] = std::move(d);
    return ACGPU_OK;
}

} // namespace

namespace acgpu { // (what acgpu_calls.h and acgpu_host.h declare: described there)

uint32_t lds_states_for(const HostTables &t) {
    if (!t.dense) return 0;
    int64_t budget = tunables().lds_table_bytes;
    const int64_t max_budget = 160 * 1024 - (int64_t)scan_queue_bytes(scan_block_threads()) - 1024;
    budget = std::max<int64_t>(0, std::min(budget, max_budget));
    // table classes: k_ac_dfa keeps the class pages behind the rows when they are small next to them (at most a quarter of the
    // budget: 3000 CJK units are 3.5 KB of pages)
    if (!t.range_cls && !t.dfa_pages.empty() && (int64_t)t.dfa_pages.size() * 2 + 16 <= budget / 4)
        budget -= (int64_t)t.dfa_pages.size() * 2 + 16;
    uint64_t row = (uint64_t)t.n_cls * t.entry_bytes;
    uint64_t s = row ? (uint64_t)budget / row : 0;
    return (uint32_t)std::min<uint64_t>(s, t.n_states);
}

DevTables folded_tables(const DeviceState &d) {
    DevTables T = d.T;
    if (d.wflags_f) {
        T.wflags = d.wflags_f;
        T.wbits = d.wbits_f;
    }
    return T;
}

void refresh_call_state(acgpu_automaton *a, DeviceState &d) {
    d.T.lds_entries = lds_states_for(a->t) * a->t.n_cls;
    const int64_t k = std::max<int64_t>(0, tunables().reserve_cus);
    d.n_cu = (int)std::max<int64_t>(8, (int64_t)d.n_cu_phys - k);
}

int device_for_call(acgpu_automaton *a, DeviceState **d, int lane) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        return ACGPU_E_NODEVICE;
    }
    std::lock_guard<std::mutex> lock(a->mu); // (the map; a new pool uploads its tables under it)
    return ensure_device(a, d, lane);
}

} // namespace acgpu
