// san_owners.cpp -- a stand-alone host program (tests/test_sanitizers.py builds it with -fsanitize=address,undefined) over the
// owning types of csrc/acgpu_host.h: Owned<DevBuf>, Owned<Reservoir>, the Handle owners, a whole DeviceState, and the BatchText
// guard.  The HIP runtime is the stub below: there is no device -- every hipMalloc fails with hipErrorNoDevice -- while pinned
// blocks, events and streams are host allocations the stub keeps a ledger of.  Freeing a null or a handle twice aborts.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "acgpu_host.h"

static std::set<void *> g_live;
static int g_device_frees = 0;

static void *stub_new() {
    void *p = std::malloc(64);
    g_live.insert(p);
    return p;
}
static hipError_t stub_delete(void *p, const char *what) {
    if (!p || !g_live.erase(p)) {
        std::fprintf(stderr, "san_owners: %s of %s\n", what, p ? "a handle that is not live" : "null");
        std::abort();
    }
    std::free(p);
    return hipSuccess;
}

extern "C" {
hipError_t hipMalloc(void **p, size_t) { *p = nullptr; return hipErrorNoDevice; }
hipError_t hipFree(void *p) { ++g_device_frees; return stub_delete(p, "hipFree"); }
hipError_t hipHostMalloc(void **p, size_t, unsigned) { *p = stub_new(); return hipSuccess; }
hipError_t hipHostFree(void *p) { return stub_delete(p, "hipHostFree"); }
hipError_t hipEventCreate(hipEvent_t *e) { *e = (hipEvent_t)stub_new(); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { return stub_delete(e, "hipEventDestroy"); }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = (hipStream_t)stub_new(); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { return stub_delete(s, "hipStreamDestroy"); }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
}

namespace acgpu {
thread_local int g_last_hip_error = 0;
int device_for_call(acgpu_automaton *, DeviceState **, int) { return ACGPU_E_NODEVICE; }
void PieceRamp::start() {}
} // namespace acgpu

using namespace acgpu;

#define CHECK(x)                                                          \
    do {                                                                  \
        if (!(x)) {                                                       \
            std::fprintf(stderr, "san_owners: line %d: %s\n", __LINE__, #x); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

int main() {
    { // buffers: a failed ensure leaves nothing to free, and the owner frees nothing
        PoolBuf b;
        Owned<Reservoir> r;
        CHECK(b.ensure(1000) == ACGPU_E_NODEVICE && !b.p && b.bytes == 0);
        CHECK(r.ensure(10, 12) == ACGPU_E_NODEVICE && !r.p && r.recs == 0);
        CHECK(g_last_hip_error == (int)hipErrorNoDevice);
        b.release(); // (by hand, then by the owner: still nothing)
    }
    CHECK(g_device_frees == 0);
    { // handles: empty, created, moved into a vector, reset by hand
        PoolEvent none, e;
        PoolStream s;
        Pinned<unsigned long long> words;
        CHECK(hipEventCreate(&e.h) == hipSuccess && hipStreamCreateWithFlags(&s.h, 0) == hipSuccess);
        CHECK(hipHostMalloc((void **)&words.h, 64, 0) == hipSuccess && g_live.size() == 3);
        words[1] = 7;
        CHECK(!none && e && (words + 1)[0] == 7);
        std::vector<PoolEvent> v;
        for (int i = 0; i < 9; ++i) { // (the vector grows: every handle moves, none is destroyed on the way)
            PoolEvent x;
            CHECK(hipEventCreate(&x.h) == hipSuccess);
            v.push_back(std::move(x));
            CHECK(!x);
        }
        CHECK(g_live.size() == 12);
        e.reset();
        e.reset();
        CHECK(!e && g_live.size() == 11);
    }
    CHECK(g_live.empty());
    { // a pool as ensure_device leaves it when the device goes away half way: what exists is released once
        DeviceState d;
        d.table_allocs.emplace_back();
        CHECK(hipMalloc(&d.table_allocs.back().h, 16) == hipErrorNoDevice);
        CHECK(hipStreamCreateWithFlags(&d.lane_stream.h, 0) == hipSuccess);
        d.call_stream = d.lane_stream;
        CHECK(hipHostMalloc((void **)&d.h_counter.h, 64, 0) == hipSuccess);
        for (auto &e : d.ev) CHECK(hipEventCreate(&e.h) == hipSuccess);
        CHECK(hipEventCreate(&d.tickets[0].ev[0].h) == hipSuccess && hipHostMalloc((void **)&d.tickets[0].h_count.h, 64, 0) == hipSuccess);
        CHECK(hipHostMalloc(&d.pin[2].h, 64, 0) == hipSuccess && hipEventCreate(&d.replace_ev[3].h) == hipSuccess);
        CHECK(d.stage_hay.ensure(64) == ACGPU_E_NODEVICE && d.count_res.ensure(4, 12) == ACGPU_E_NODEVICE);
        CHECK(g_live.size() == 10);
        HostTables t;
        t.sep_unit = 0xffff;
        auto ends_early = [&]() -> int { // a batch call that fails behind its staged text
            BatchText text(d, t);
            if (d.start_behind != 0xffff || text.sep != 0xffff) return ACGPU_E_INVALID;
            const int rc = d.batch_off.ensure(16);
            if (rc) return rc;
            return ACGPU_OK;
        };
        CHECK(ends_early() == ACGPU_E_NODEVICE && d.start_behind == -1);
        PoolCall call(nullptr);
        CHECK(call.rc == ACGPU_E_NODEVICE && !call.d && !call.lock.owns_lock());
    }
    CHECK(g_live.empty() && g_device_frees == 0);
    std::puts("san_owners: done");
    return 0;
}
