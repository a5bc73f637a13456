// acgpu_cursor.hip -- acgpu_cursor_* (include/acgpu.h): one match(String, listener) call handed out in pages, scanned piece by
// piece (scan_next_piece, acgpu_pieces.hip) only as far as the pages taken so far require.
//
// Pages leave the cursor's own device reservoir through k_cursor_page, which shifts the positions from the piece's buffer
// coordinates to haystack coordinates on the way into pinned, device-mapped staging memory.
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

struct acgpu_cursor {
    acgpu_automaton *a = nullptr; // nullptr: detached by acgpu_free
    int device = -1;
    const uint16_t *hay = nullptr;
    bool failed = false; // a next failed: only close is valid
    PieceDriver p;       // the scan: the text's units [0, p.pos) have been scanned
    // the reservoir: records [res_r, res_n) of the current piece are not handed out yet; positions relative to res_base
    Reservoir res;
    uint64_t res_n = 0, res_r = 0;
    int32_t res_base = 0;
    // page staging: pinned, device-mapped
    void *pin = nullptr, *pin_dev = nullptr;
    uint64_t pin_bytes = 0;
    acgpu_cursor_stats st{}; // done, records_delivered: the rest is the driver's
    ~acgpu_cursor() {
        if (a) {
            std::lock_guard<std::mutex> l(a->mu);
            a->open_cursors.erase(this);
        }
        if (device >= 0 && (res.p || pin)) {
            int cur = -1;
            const bool have = hipGetDevice(&cur) == hipSuccess;
            (void)hipSetDevice(device);
            res.release();
            if (pin) (void)hipHostFree(pin);
            if (have) (void)hipSetDevice(cur);
        }
    }
};

namespace {

int page_out(acgpu_cursor *c, DeviceState &d, void *out, uint64_t k) {
    const uint64_t rk = (uint64_t)c->p.record_kind, bytes = k * rk;
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
                       (const int32_t *)((const char *)c->res.p + c->res_r * rk), (int32_t *)c->pin_dev, n_dw, (int)(rk / 4), c->res_base);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(d.call_stream));
    std::memcpy(out, c->pin, bytes);
    return ACGPU_OK;
}

int cursor_next(acgpu_cursor *c, void *out, uint64_t cap, uint64_t *n_out) {
    int cur = -1;
    HIP_TRY(hipGetDevice(&cur));
    if (cur != c->device) return ACGPU_E_INVALID;
    PoolCall call(c->a);
    if (call.rc) return call.rc;
    DeviceState *d = call.d;
    int rc = call.idle(); // (tickets of the asynchronous entry are in flight)
    if (rc) return rc;
    while (c->res_r == c->res_n) { // (an empty reservoir: scan until a piece yields a record or the text ends)
        if (c->p.pos >= c->p.end) {
            c->st.done = 1;
            return ACGPU_OK;
        }
        uint64_t base = 0;
        if ((rc = scan_next_piece(c->p, PieceScan{c->a, *d, c->hay, c->p.end, nullptr, nullptr}, &c->res_n, &base))) return rc;
        c->res_r = 0;
        c->res_base = (int32_t)base;
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
    c->p = PieceDriver(0, n_units, 0, host_one_piece(a->t, record_kind), record_kind, &c->res);
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
    st->units_scanned = c->p.units_scanned;
    st->scan_end = c->p.scan_end;
    st->pieces = (uint32_t)c->p.pieces;
    st->rescans = (uint32_t)c->p.rescans;
    return ACGPU_OK;
}

void acgpu_cursor_close(acgpu_cursor *c) { delete c; }

} // extern "C"
