// acgpu_cursor.hip -- acgpu_cursor_* (include/acgpu.h): one match(String, listener) call handed out in pages, scanned piece by
// piece only as far as the pages taken so far require.
//
// A piece is one scan_host_range call (acgpu_api.hip) over an owned range of the haystack plus the halo its family needs, into
// the cursor's own device reservoir; the chain of LONGEST / SHORTEST / WWLONGEST is handed from piece to piece in haystack
// coordinates.  Pages leave the reservoir through k_cursor_page, which shifts the positions from the piece's buffer coordinates
// to haystack coordinates on the way into pinned, device-mapped staging memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>

#include "acgpu_host.h"
#include "acgpu_internal.h"

using namespace acgpu;

namespace {

// Reservoir records [r, r + k) -> page staging, start / end + base.  The page is n_dw = k * cols dwords (cols = 2 or 3); a
// thread writes one 16-byte quad of it (the staging is 16-byte aligned) with one dwordx4 store -- the page's last, partial quad
// dword by dword.  src = the reservoir's dword r * cols: its alignment mod 16 bytes (`mis` dwords) is the same for every
// thread of a launch, so the loads are one dwordx4 (aligned), two dwordx2 (mis 2) or four dwords (mis 1, 3) -- coalesced across
// the wave either way.
__global__ void k_cursor_page(const int32_t *__restrict__ src, int32_t *__restrict__ dst, uint64_t n_dw, int cols, int32_t base) {
    const uint32_t mis = (uint32_t)(((uintptr_t)src >> 2) & 3u);
    const uint64_t n_q = (n_dw + 3) / 4;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_q; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = 4 * q;
        const uint32_t c0 = cols == 2 ? 0u : (uint32_t)(q % 3u); // column of dword i: (4 q) mod 3 == q mod 3
        int32_t v[4];
        if (i + 4 <= n_dw) {
            if (mis == 0) {
                const int4 x = *reinterpret_cast<const int4 *>(src + i);
                v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
            } else if (mis == 2) {
                const int2 x = *reinterpret_cast<const int2 *>(src + i), y = *reinterpret_cast<const int2 *>(src + i + 2);
                v[0] = x.x; v[1] = x.y; v[2] = y.x; v[3] = y.y;
            } else {
                for (int j = 0; j < 4; ++j) v[j] = src[i + j];
            }
            for (uint32_t j = 0; j < 4; ++j)
                if ((c0 + j) % (uint32_t)cols < 2u) v[j] += base; // start, end; keyword_id passes through
            *reinterpret_cast<int4 *>(dst + i) = make_int4(v[0], v[1], v[2], v[3]);
        } else {
            for (uint32_t j = 0; i + j < n_dw; ++j) {
                const int32_t x = src[i + j];
                dst[i + j] = (c0 + j) % (uint32_t)cols < 2u ? x + base : x;
            }
        }
    }
}

} // namespace

namespace acgpu {

uint64_t reservoir_budget_bytes() { return (uint64_t)std::max<int64_t>(tunables().cursor_reservoir_bytes.load(std::memory_order_relaxed), 16); }

void PieceRamp::start() {
    piece = (uint64_t)std::max<int64_t>(1, tunables().cursor_first_piece.load(std::memory_order_relaxed));
    seen_records = seen_units = 0;
}

// the next step of the ramp, capped so that the density seen so far fills at most half the reservoir budget
uint64_t PieceRamp::next_size(uint64_t left, uint64_t budget_recs) const {
    uint64_t size = std::min<uint64_t>(piece, left);
    if (seen_records && seen_units) {
        const double per_unit = (double)seen_records / (double)seen_units;
        const double fit = (double)(budget_recs / 2) / per_unit;
        if (fit < (double)size) size = std::max<uint64_t>(1, (uint64_t)fit);
    }
    return size;
}

uint64_t PieceRamp::predicted_room(uint64_t size, uint64_t budget_recs) const {
    if (!seen_units) return 0;
    const double pred = (double)seen_records / (double)seen_units * (double)size;
    return std::min<uint64_t>(budget_recs, (uint64_t)(pred * 1.25) + 1024);
}

bool PieceRamp::on_overflow(uint64_t *size, uint64_t cnt, uint64_t budget_recs, uint64_t *room) const {
    if (cnt <= budget_recs) { // a larger reservoir
        *room = std::min<uint64_t>(budget_recs, cnt + cnt / 8);
    } else if (*size > 1) { // a smaller piece: half the budget by this piece's density
        *size = std::max<uint64_t>(1, (uint64_t)((double)*size * (double)(budget_recs / 2) / (double)cnt));
        *room = budget_recs;
    } else {
        return false;
    }
    return true;
}

void PieceRamp::advance(uint64_t size, uint64_t cnt) {
    seen_records += cnt;
    seen_units += size;
    const uint64_t max_piece = (uint64_t)std::max<int64_t>(1, tunables().cursor_max_piece.load(std::memory_order_relaxed));
    piece = std::min<uint64_t>(max_piece, std::max<uint64_t>(size, 1) * 4);
}

} // namespace acgpu

struct acgpu_cursor {
    acgpu_automaton *a = nullptr; // nullptr: detached by acgpu_free
    int device = -1;
    const uint16_t *hay = nullptr;
    uint64_t n = 0;
    int record_kind = 0;
    bool whole = false;  // the text is scanned as ONE piece (one_piece)
    bool failed = false; // a next failed: only close is valid
    // the scan
    uint64_t pos = 0;      // owned units [0, pos) have been scanned
    int64_t chain = 0;     // the chain's entry into the next piece (haystack coordinates)
    PieceRamp ramp;        // the sizes of the pieces
    // the reservoir: records [res_r, res_n) of the current piece are not handed out yet; positions relative to res_base
    void *res = nullptr;
    uint64_t res_bytes = 0;
    uint64_t res_n = 0, res_r = 0;
    int32_t res_base = 0;
    // page staging: pinned, device-mapped
    void *pin = nullptr, *pin_dev = nullptr;
    uint64_t pin_bytes = 0;
    acgpu_cursor_stats st{};
    ~acgpu_cursor() {
        if (a) {
            std::lock_guard<std::mutex> l(a->mu);
            a->open_cursors.erase(this);
        }
        if (device >= 0 && (res || pin)) {
            int cur = -1;
            const bool have = hipGetDevice(&cur) == hipSuccess;
            (void)hipSetDevice(device);
            if (res) (void)hipFree(res);
            if (pin) (void)hipHostFree(pin);
            if (have) (void)hipSetDevice(cur);
        }
    }
};

namespace {

int grow_reservoir(acgpu_cursor *c, uint64_t bytes) {
    if (bytes <= c->res_bytes) return ACGPU_OK;
    if (c->res) (void)hipFree(c->res);
    c->res = nullptr;
    c->res_bytes = 0;
    HIP_TRY(hipMalloc(&c->res, bytes + 64));
    c->res_bytes = bytes;
    return ACGPU_OK;
}

uint64_t budget_bytes() { return reservoir_budget_bytes(); }

// The whole text as one shard (the loops that exist only as one sequential kernel): copied to the pool's staging buffer and
// scanned into the reservoir, which grows to the exact count -- past the budget if device memory allows.
int scan_whole(acgpu_cursor *c, DeviceState &d) {
    acgpu_automaton *a = c->a;
    const uint64_t rk = (uint64_t)c->record_kind;
    int rc;
    if ((rc = d.stage_hay.ensure(c->n * 2 + 16))) return rc;
    if (c->n) HIP_TRY(hipMemcpy(d.stage_hay.p, c->hay, c->n * 2, hipMemcpyHostToDevice));
    if ((rc = grow_reservoir(c, std::min<uint64_t>(budget_bytes(), std::max<uint64_t>(c->n / 16, 4096) * rk)))) return rc;
    for (;;) {
        acgpu_shard sh{};
        sh.d_hay = (const uint16_t *)d.stage_hay.p;
        sh.n_units = c->n;
        sh.own_begin = 0;
        sh.own_end = c->n;
        sh.text_begin = 1;
        sh.text_end = 1;
        sh.chain_entry = 0;
        uint64_t cnt = 0;
        rc = match_shard(a, d, &sh, c->record_kind, c->res, c->res_bytes / rk, &cnt, d.call_stream, nullptr);
        c->st.pieces++;
        c->st.units_scanned += c->n;
        if (rc == ACGPU_E_OVERFLOW) {
            c->st.rescans++;
            if ((rc = grow_reservoir(c, cnt * rk))) return rc;
            continue;
        }
        if (rc) return rc;
        c->res_n = cnt;
        c->res_r = 0;
        c->res_base = 0;
        c->pos = c->n;
        c->st.scan_end = c->n;
        return ACGPU_OK;
    }
}

// Scans the next piece into the reservoir (which is empty): its owned range starts at c->pos.  Overflow: a larger reservoir
// within the budget, else a smaller piece, and the same piece scanned again.
int scan_piece(acgpu_cursor *c, DeviceState &d) {
    if (c->whole) return scan_whole(c, d);
    acgpu_automaton *a = c->a;
    const ShardRule rule = shard_rule(a->t, c->record_kind, false);
    const uint64_t rk = (uint64_t)c->record_kind;
    const uint64_t budget_recs = std::max<uint64_t>(budget_bytes() / rk, 1);
    uint64_t size = c->ramp.next_size(c->n - c->pos, budget_recs);
    for (;;) {
        const uint64_t own_lo = c->pos, own_hi = own_lo + size;
        const uint64_t lo = own_lo - std::min(rule.left, own_lo), hi = std::min<uint64_t>(c->n, own_hi + rule.right);
        // predicted records: room for them (within the budget) before the scan, so that a steady text is not scanned twice
        if (const uint64_t want = c->ramp.predicted_room(size, budget_recs)) {
            int rc = grow_reservoir(c, want * rk);
            if (rc) return rc;
        } else if (!c->res) { // (a record per unit: natural text against a word list has 0.8)
            int rc = grow_reservoir(c, std::min<uint64_t>(budget_recs, std::max<uint64_t>(size, 4096)) * rk);
            if (rc) return rc;
        }
        int64_t chain = c->chain - (int64_t)lo; // (buffer relative: scan_host_range takes each shard's entry from it)
        uint64_t cnt = 0;
        int rc = scan_host_range(a, d, c->hay, c->n, lo, hi, own_lo, own_hi, c->record_kind, c->res_bytes / rk, &cnt, &chain, c->res);
        c->st.pieces++;
        c->st.units_scanned += size;
        c->st.scan_end = std::max<uint64_t>(c->st.scan_end, hi);
        if (rc == ACGPU_E_OVERFLOW) {
            c->st.rescans++;
            uint64_t room = 0;
            if (!c->ramp.on_overflow(&size, cnt, budget_recs, &room)) return ACGPU_E_NOMEM; // one unit's records do not fit the budget
            if ((rc = grow_reservoir(c, room * rk))) return rc;
            continue;
        }
        if (rc) return rc;
        c->chain = chain + (int64_t)lo;
        c->res_n = cnt;
        c->res_r = 0;
        c->res_base = (int32_t)lo;
        c->pos = own_hi;
        c->ramp.advance(size, cnt);
        return ACGPU_OK;
    }
}

int page_out(acgpu_cursor *c, DeviceState &d, void *out, uint64_t k) {
    const uint64_t rk = (uint64_t)c->record_kind, bytes = k * rk;
    if (c->pin_bytes < bytes) {
        if (c->pin) (void)hipHostFree(c->pin);
        c->pin = c->pin_dev = nullptr;
        c->pin_bytes = 0;
        const uint64_t want = bytes + bytes / 4 + 4096;
        HIP_TRY(hipHostMalloc(&c->pin, want, hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer(&c->pin_dev, c->pin, 0));
        c->pin_bytes = want;
    }
    const uint64_t n_dw = k * (rk / 4), n_q = (n_dw + 3) / 4;
    const unsigned blocks = (unsigned)std::min<uint64_t>((n_q + 255) / 256, 8192);
    hipLaunchKernelGGL(k_cursor_page, dim3(blocks), dim3(256), 0, d.call_stream,
                       (const int32_t *)((const char *)c->res + c->res_r * rk), (int32_t *)c->pin_dev, n_dw, (int)(rk / 4), c->res_base);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(d.call_stream));
    std::memcpy(out, c->pin, bytes);
    return ACGPU_OK;
}

int cursor_next(acgpu_cursor *c, void *out, uint64_t cap, uint64_t *n_out) {
    int cur = -1;
    HIP_TRY(hipGetDevice(&cur));
    if (cur != c->device) return ACGPU_E_INVALID;
    DeviceState *d = nullptr;
    int rc = device_for_call(c->a, &d);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(d->mu);
    if (d->inflight > 0) return ACGPU_E_INVALID; // (stream rule: tickets of the asynchronous entry are in flight)
    while (c->res_r == c->res_n) { // (an empty reservoir: scan until a piece yields a record or the text ends)
        if (c->pos >= c->n) {
            c->st.done = 1;
            return ACGPU_OK;
        }
        if ((rc = scan_piece(c, *d))) return rc;
    }
    const uint64_t k = std::min<uint64_t>(cap, c->res_n - c->res_r);
    if ((rc = page_out(c, *d, out, k))) return rc;
    c->res_r += k;
    c->st.records_delivered += k;
    *n_out = k;
    return ACGPU_OK;
}

} // namespace

extern "C" {

// acgpu_free with this cursor still open (the caller holds the automaton's mutex): nothing of the cursor refers to it any more
void acgpu_cursor_detach(acgpu_cursor *c) { c->a = nullptr; }

int acgpu_cursor_open(const acgpu_automaton *ca, const uint16_t *haystack, uint64_t n_units, int record_kind, acgpu_cursor **out) {
    if (!out) return ACGPU_E_INVALID;
    *out = nullptr;
    if (!ca || !haystack) return ACGPU_E_INVALID;
    if (record_kind != ACGPU_REC_SET && record_kind != ACGPU_REC_MAP) return ACGPU_E_INVALID;
    if (n_units >= (1ull << 31)) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    DeviceState *d = nullptr;
    int rc = device_for_call(a, &d); // (no device: fails here, as acgpu_match_u16 does; else the tables are uploaded now)
    if (rc) return rc;
    acgpu_cursor *c = new (std::nothrow) acgpu_cursor();
    if (!c) return ACGPU_E_NOMEM;
    c->device = d->device;
    c->hay = haystack;
    c->n = n_units;
    c->record_kind = record_kind;
    const HostTables &t = a->t;
    c->whole = one_piece(shard_rule(t, record_kind, false), t);
    c->ramp.start();
    try {
        std::lock_guard<std::mutex> l(a->mu);
        a->open_cursors.insert(c);
    } catch (...) {
        delete c;
        return ACGPU_E_NOMEM;
    }
    c->a = a;
    *out = c;
    return ACGPU_OK;
}

int acgpu_cursor_next(acgpu_cursor *c, void *out, uint64_t cap, uint64_t *n_out) {
    if (!c || !out || !n_out || cap == 0) return ACGPU_E_INVALID;
    *n_out = 0;
    if (!c->a || c->failed) return ACGPU_E_INVALID; // (detached by acgpu_free, or a next failed before)
    const int rc = cursor_next(c, out, cap, n_out);
    if (rc) {
        c->failed = true;
        *n_out = 0;
    }
    return rc;
}

int acgpu_cursor_get_stats(const acgpu_cursor *c, acgpu_cursor_stats *st) {
    if (!c || !st) return ACGPU_E_INVALID;
    *st = c->st;
    st->records_buffered = c->res_n - c->res_r;
    return ACGPU_OK;
}

void acgpu_cursor_close(acgpu_cursor *c) { delete c; }

} // extern "C"
