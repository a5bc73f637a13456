// acgpu_batch.hip -- the front end of the batch entries (acgpu_match_batch_u16 here, acgpu_replace_batch_u16 in
// acgpu_replace.hip, acgpu_summary_batch_u16 in acgpu_summary.hip, acgpu_spans_batch_u16 in acgpu_spans.hip, acgpu_cover_batch_u16
// in acgpu_cover.hip): the checks they share and the decision how the batch is
// scanned (check_batch), the haystacks staged as one text (BatchText), and acgpu_match_batch_u16 itself.
//
// A batch is scanned as ONE text, the haystacks with a separator unit behind each, or, where that cannot be done, haystack by
// haystack: every haystack as a text of its own through the entry's own consumer, under the one lock the entry holds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "acgpu_host.h"
#include "acgpu_internal.h"
#include "acgpu_kernels.h"

namespace acgpu {

int check_batch(const HostTables &t, const uint16_t *units, const uint64_t *offsets, uint32_t n_haystacks, BatchPlan *plan) {
    for (uint32_t i = 0; i < n_haystacks; i++)
        if (offsets[i] > offsets[i + 1]) return ACGPU_E_INVALID;
    plan->total = offsets[n_haystacks] - offsets[0];
    if (plan->total && !units) return ACGPU_E_INVALID;
    plan->cat = plan->total + n_haystacks; // one separator behind every haystack
    if (plan->cat >= (1ull << 31)) return ACGPU_E_INVALID;
    // no unit can stand between two haystacks (every one of the 65536 is in use), or a word matcher over a table that is not
    // fold-consistent: haystack by haystack.  (Such a table makes some loops sequential kernels over one whole text; and in
    // the folding scans a keyword's FOLDED first unit need not be a word character, so a walk that begins at position 0 of a
    // text -- where the scan starts whatever stands there -- is not a walk that begins behind a separator.)
    plan->per_haystack = t.sep_unit < 0 || ((t.mode == ACGPU_MODE_WHOLEWORD || t.mode == ACGPU_MODE_WWLONGEST) && !t.fold_consistent);
    return ACGPU_OK;
}

namespace {

// The haystacks as one text in d.batch_pin, b.sep behind every haystack; the offsets stand 64-byte aligned behind the text.  The
// offsets have been checked.
int batch_concat(BatchText &b, const uint16_t *units, const uint64_t *offsets, uint32_t n_haystacks) {
    DeviceState &d = b.d;
    const uint64_t cat = offsets[n_haystacks] - offsets[0] + n_haystacks;
    const size_t off_bytes = ((size_t)n_haystacks + 1) * 4, pin_need = cat * 2 + 64 + off_bytes;
    if (d.batch_pin_bytes < pin_need) {
        d.batch_pin.reset();
        d.batch_pin_bytes = 0;
        HIP_TRY(hipHostMalloc(&d.batch_pin.h, pin_need + pin_need / 4, hipHostMallocDefault));
        d.batch_pin_bytes = pin_need + pin_need / 4;
    }
    uint16_t *h_cat = (uint16_t *)d.batch_pin.h;
    uint32_t *h_off = (uint32_t *)((char *)d.batch_pin.h + ((cat * 2 + 63) & ~(size_t)63));
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_haystacks; i++) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        h_off[i] = (uint32_t)at;
        if (len) std::memcpy(h_cat + at, units + offsets[i], len * 2);
        at += len;
        h_cat[at++] = b.sep;
    }
    h_off[n_haystacks] = (uint32_t)at;
    b.h_cat = h_cat;
    b.h_off = h_off;
    b.cat = cat;
    b.n_haystacks = n_haystacks;
    return ACGPU_OK;
}

} // namespace

int BatchText::stage(const uint16_t *units, const uint64_t *offsets, uint32_t n, hipStream_t stream) {
    int rc = batch_concat(*this, units, offsets, n);
    if (rc) return rc;
    const size_t off_bytes = ((size_t)n + 1) * 4;
    if ((rc = d.batch_off.ensure(off_bytes + 16))) return rc;
    HIP_TRY(hipMemcpyAsync(d.batch_off.p, h_off, off_bytes, hipMemcpyHostToDevice, stream));
    return ACGPU_OK;
}

} // namespace acgpu

using namespace acgpu;

extern "C" {

int acgpu_match_batch_u16(const acgpu_automaton *ca, const uint16_t *units, const uint64_t *offsets, uint32_t n_haystacks,
                          int record_kind, void *out, uint64_t cap, uint64_t *n_out) {
    if (!ca || !n_out || !offsets || (cap && !out)) return ACGPU_E_INVALID;
    if (record_kind != ACGPU_REC_SET && record_kind != ACGPU_REC_MAP) return ACGPU_E_INVALID;
    *n_out = 0;
    if (n_haystacks == 0) return ACGPU_OK;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    const HostTables &t = a->t;
    BatchPlan plan;
    int rc = check_batch(t, units, offsets, n_haystacks, &plan);
    if (rc) return rc;
    const size_t out_rec = (size_t)record_kind + 4;
    PoolCall call(a); // (the staging buffers are part of the per-device scratch pool)
    if (call.rc) return call.rc;
    DeviceState &d = *call.d;
    if (plan.per_haystack) { // every haystack by the route acgpu_match_u16 takes, tagged on the host
        const int W = record_kind / 4;
        std::vector<int32_t> tmp;
        uint64_t n = 0;
        for (uint32_t i = 0; i < n_haystacks; i++) {
            const uint64_t len = offsets[i + 1] - offsets[i];
            uint64_t got = 0, room = cap > n ? cap - n : 0;
            try {
                tmp.resize(std::max<size_t>(room * W, 4));
            } catch (...) {
                return ACGPU_E_NOMEM;
            }
            rc = match_host_text(a, d, units + offsets[i], len, record_kind, tmp.data(), room, &got);
            if (rc != ACGPU_OK && rc != ACGPU_E_OVERFLOW) return rc;
            for (uint64_t r = 0; rc == ACGPU_OK && r < got; r++) {
                int32_t *o = (int32_t *)((char *)out + (n + r) * out_rec);
                o[0] = (int32_t)i;
                for (int w = 0; w < W; w++) o[1 + w] = tmp[r * W + w];
            }
            n += got;
        }
        *n_out = n;
        return n > cap ? ACGPU_E_OVERFLOW : ACGPU_OK;
    }
    if ((rc = call.idle())) return rc; // (the NULL stream: see the stream rule)
    BatchText text(d, t);
    if ((rc = text.stage(units, offsets, n_haystacks, nullptr))) return rc;
    if ((rc = d.stage_hay.ensure(text.cat * 2 + 16))) return rc;
    if ((rc = d.stage_out.ensure(cap * (uint64_t)record_kind + 16))) return rc;
    if ((rc = d.batch_out.ensure(cap * out_rec + 16))) return rc;
    HIP_TRY(hipMemcpyAsync(d.stage_hay.p, text.h_cat, text.cat * 2, hipMemcpyHostToDevice, nullptr));
    acgpu_shard sh{};
    sh.d_hay = (const uint16_t *)d.stage_hay.p;
    sh.n_units = sh.own_end = text.cat;
    sh.text_begin = sh.text_end = 1;
    rc = match_shard(a, d, &sh, record_kind, d.stage_out.p, cap, n_out, nullptr, nullptr);
    if (rc != ACGPU_OK) return rc; // ACGPU_E_OVERFLOW: *n_out is the capacity to retry with
    if (*n_out) {
        HIP_TRY(launch_batch_tag(d.stage_out.p, *n_out, record_kind, text.d_off(), n_haystacks, d.batch_out.p, nullptr));
        HIP_TRY(hipMemcpy(out, d.batch_out.p, *n_out * out_rec, hipMemcpyDeviceToHost));
    }
    return ACGPU_OK;
}

} // extern "C"
