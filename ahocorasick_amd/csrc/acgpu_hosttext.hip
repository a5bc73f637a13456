// acgpu_hosttext.hip -- acgpu_match_u16: a host text on its way through the device -- the one-launch call for a short one, the
// whole text staged as one shard, or chunks through a ring of pinned buffers, copied by threads on the device's NUMA node, while
// the chunks that have arrived are scanned.
#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "acgpu_host.h"
#include "acgpu_small.h"

using namespace acgpu;

namespace acgpu {

int64_t piece_entry(const ShardRule &r, int64_t chain, int64_t origin, uint64_t own_begin) {
    const int64_t rel = std::max<int64_t>(0, chain - origin); // (a restart left of the buffer restricts nothing more than its start)
    return r.chain == Chain::Restart ? rel : std::max<int64_t>(rel, (int64_t)own_begin);
}

int64_t piece_exit(const ShardRule &r, int64_t entry, uint64_t own_end, const acgpu_shard *sh, uint64_t n) {
    if (r.chain == Chain::Restart) return sh && n ? sh->chain_exit : entry; // (no record: the restart that came in)
    if (r.chain == Chain::Position && sh) return sh->chain_exit;
    return std::max<int64_t>(entry, (int64_t)own_end);
}

// acgpu_match_u16 on a long haystack, pipelined: the text goes to the device in chunks -- worker threads copy the caller's
// (pageable) memory into a ring of pinned staging buffers and enqueue the DMA on a copy stream -- while the chunks that have
// arrived are scanned as shards of the device buffer (own range = the chunk, halos = its neighbours already / also there;
// the chain families hand their entry on from shard to shard).  The scans are a fraction of the transfer time, so the call
// runs at the rate of the slower of the host copy and the link instead of copy + scan + copy back in sequence.
// The general form serves one device's share of a multi-device call as well: the device buffer holds the units [lo, hi) of
// the text (the share plus its halos), of which [own_lo, own_hi) is owned; positions in the records and in *chain are
// relative to the buffer.
constexpr uint64_t kHostChunkUnits = 1ull << 24; // 32 MiB per chunk

bool one_piece(const ShardRule &r, const HostTables &t) { return r.sequential || (uint64_t)t.max_len + 2 >= kHostChunkUnits; }
bool host_one_piece(const HostTables &t, int record_kind) { return one_piece(shard_rule(t, record_kind, false), t); }

// The CPUs of the NUMA node a device hangs on (/sys/bus/pci/devices/<bdf>/numa_node, /sys/devices/system/node/node<N>/cpulist):
// the threads that copy a share's text into pinned memory run there, so that on a two-socket host eight devices are fed by both
// sockets' memory controllers, each from its own side.  false: unknown (node -1, a container without /sys, ...): no affinity is set.
static bool device_numa_cpus(int dev, cpu_set_t *set) {
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), dev) != hipSuccess) return false;
    for (char *p = bdf; *p; ++p) *p = (char)std::tolower((unsigned char)*p);
    char path[160];
    std::snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bdf);
    FILE *f = std::fopen(path, "r");
    if (!f) return false;
    int node = -1;
    const int got = std::fscanf(f, "%d", &node);
    std::fclose(f);
    if (got != 1 || node < 0) return false;
    std::snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    f = std::fopen(path, "r");
    if (!f) return false;
    char list[4096] = {0};
    const bool have = std::fgets(list, (int)sizeof(list), f) != nullptr;
    std::fclose(f);
    if (!have) return false;
    CPU_ZERO(set);
    int n_set = 0;
    for (char *p = list; *p;) { // "0-63,128-191"
        char *end = nullptr;
        const long a = std::strtol(p, &end, 10);
        if (end == p) break;
        long b = a;
        p = end;
        if (*p == '-') {
            b = std::strtol(p + 1, &end, 10);
            p = end;
        }
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c) {
            CPU_SET((int)c, set);
            ++n_set;
        }
        if (*p == ',') ++p;
    }
    return n_set > 0;
}

int stage_whole_text(DeviceState &d, const uint16_t *haystack, uint64_t n_units, acgpu_shard *out) {
    const int rc = d.stage_hay.ensure(n_units * 2 + 16);
    if (rc) return rc;
    if (n_units) HIP_TRY(hipMemcpy(d.stage_hay.p, haystack, n_units * 2, hipMemcpyHostToDevice));
    *out = acgpu_shard{};
    out->d_hay = (const uint16_t *)d.stage_hay.p;
    out->n_units = out->own_end = n_units;
    out->text_begin = out->text_end = 1;
    return ACGPU_OK;
}

int scan_host_range(acgpu_automaton *a, DeviceState &d, const uint16_t *haystack, uint64_t n_units, uint64_t lo, uint64_t hi,
                    uint64_t own_lo, uint64_t own_hi, int record_kind, uint64_t cap, uint64_t *n_out, int64_t *chain_io,
                    void *d_out, uint64_t *own_done) {
    const ShardRule rule = shard_rule(a->t, record_kind, false);
    const uint64_t C = kHostChunkUnits;
    const uint64_t nb = hi - lo; // units in the device buffer
    const uint32_t n_chunks = (uint32_t)((nb + C - 1) / C);
    const uint64_t ob = own_lo - lo, oe = own_hi - lo; // the owned range in the buffer
    hipStream_t stream = d.call_stream;
    const bool counting = own_done != nullptr; // (a counting call's scan: a shard's records are consumed when it is collected, see acgpu_host.h)
    *n_out = 0;
    if (own_done) *own_done = ob;
    int rc;
    if ((rc = d.stage_hay.ensure(nb * 2 + 16))) return rc;
    if (!d_out) {
        if ((rc = d.stage_out.ensure(cap * (uint64_t)record_kind + 16))) return rc;
        d_out = d.stage_out.p;
    }
    if (!d.copy_stream) HIP_TRY(hipStreamCreateWithFlags(&d.copy_stream.h, hipStreamNonBlocking));
    // the ring: as many slots as this buffer has chunks (at most kPinSlots), each as large as its largest chunk -- a share of a
    // few megabytes of a multi-device call, or a 40 MiB haystack, does not pin 8 x 32 MiB
    const size_t slot_bytes = (((size_t)std::min<uint64_t>(nb, C) * 2 + (1u << 20) - 1) >> 20) << 20;
    const int slots_needed = (int)std::min<uint32_t>(n_chunks, (uint32_t)DeviceState::kPinSlots);
    if (d.pin_bytes < slot_bytes) {
        for (auto &q : d.pin) q.reset();
        d.pin_n = 0;
        d.pin_bytes = slot_bytes;
    }
    while (d.pin_n < slots_needed) {
        HIP_TRY(hipHostMalloc(&d.pin[d.pin_n].h, d.pin_bytes, hipHostMallocDefault));
        d.pin_n++;
    }
    while (d.chunk_ev.size() < n_chunks) {
        PoolEvent e;
        HIP_TRY(hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
        d.chunk_ev.push_back(std::move(e));
    }
    // producers: chunk k -> pinned slot k % kPinSlots (free once chunk k - kPinSlots has been copied to the device) -> DMA
    const int n_workers = (int)std::min<uint32_t>({(uint32_t)DeviceState::kPinSlots - 2, n_chunks, std::max(2u, std::thread::hardware_concurrency() / 2)});
    std::atomic<uint32_t> next_chunk{0};
    std::atomic<int> worker_rc{ACGPU_OK};
    std::vector<std::atomic<int>> ready(n_chunks); // 1: the chunk's DMA and event are enqueued
    for (auto &r : ready) r.store(0, std::memory_order_relaxed);
    const int dev = d.device;
    cpu_set_t node_cpus;
    const bool have_node = device_numa_cpus(dev, &node_cpus);
    auto worker = [&]() {
        if (have_node) (void)pthread_setaffinity_np(pthread_self(), sizeof(node_cpus), &node_cpus); // (best effort)
        if (hipSetDevice(dev) != hipSuccess) {
            worker_rc.store(ACGPU_E_HIP);
            return;
        }
        for (;;) {
            const uint32_t k = next_chunk.fetch_add(1);
            if (k >= n_chunks || worker_rc.load() != ACGPU_OK) return;
            const uint64_t b0 = (uint64_t)k * C, len = std::min<uint64_t>(C, nb - b0);
            const int slot = (int)(k % DeviceState::kPinSlots);
            if (k >= (uint32_t)DeviceState::kPinSlots) { // the slot's previous chunk must have left it
                while (!ready[k - DeviceState::kPinSlots].load(std::memory_order_acquire)) {
                    if (worker_rc.load() != ACGPU_OK) return;
                    std::this_thread::yield();
                }
                if (hipEventSynchronize(d.chunk_ev[k - DeviceState::kPinSlots]) != hipSuccess) {
                    worker_rc.store(ACGPU_E_HIP);
                    return;
                }
            }
            std::memcpy(d.pin[slot], haystack + lo + b0, len * 2);
            if (hipMemcpyAsync((char *)d.stage_hay.p + b0 * 2, d.pin[slot], len * 2, hipMemcpyHostToDevice, d.copy_stream) != hipSuccess ||
                hipEventRecord(d.chunk_ev[k], d.copy_stream) != hipSuccess) {
                worker_rc.store(ACGPU_E_HIP);
                return;
            }
            ready[k].store(1, std::memory_order_release);
        }
    };
    std::vector<std::thread> pool;
    try {
        for (int i = 0; i < n_workers; ++i) pool.emplace_back(worker);
    } catch (...) {
        worker_rc.store(ACGPU_E_NOMEM);
    }
    auto join_all = [&]() {
        for (auto &th : pool) if (th.joinable()) th.join();
    };
    // consumer: shard k once the chunks its right halo reaches into have arrived (the chunks before a shard always have)
    uint64_t total = 0;
    int64_t chain = chain_io ? *chain_io : 0;
    uint32_t waited = 0; // chunks whose arrival the compute stream already waits for
    int result = ACGPU_OK;
    for (uint32_t k = 0; k < n_chunks && result == ACGPU_OK; ++k) {
        const uint64_t c0 = std::max<uint64_t>((uint64_t)k * C, ob), c1 = std::min<uint64_t>({nb, (uint64_t)(k + 1) * C, oe});
        if (c0 >= c1) continue; // a chunk of halo units only
        const uint32_t need = (uint32_t)std::min<uint64_t>(n_chunks, (std::min<uint64_t>(nb, c1 + rule.right) + C - 1) / C); // chunks [0, need)
        for (; waited < need && result == ACGPU_OK; ++waited) {
            while (!ready[waited].load(std::memory_order_acquire)) {
                if (worker_rc.load() != ACGPU_OK) { result = worker_rc.load(); break; }
                std::this_thread::yield();
            }
            if (result == ACGPU_OK && hipStreamWaitEvent(stream, d.chunk_ev[waited], 0) != hipSuccess) result = ACGPU_E_HIP;
        }
        if (result != ACGPU_OK) break;
        acgpu_shard sh{};
        sh.d_hay = (const uint16_t *)d.stage_hay.p;
        sh.n_units = std::min<uint64_t>(nb, (uint64_t)need * C); // what has arrived
        sh.own_begin = c0;
        sh.own_end = c1;
        sh.text_begin = lo == 0 ? 1 : 0;
        sh.text_end = (sh.n_units == nb && hi == n_units) ? 1 : 0;
        const int64_t entry = piece_entry(rule, chain, 0, c0);
        sh.chain_entry = entry;
        uint64_t n_k = 0;
        const uint64_t room = total < cap ? cap - total : 0;
        rc = match_shard(a, d, &sh, record_kind, (char *)d_out + std::min(total, cap) * (uint64_t)record_kind, room, &n_k, stream, nullptr);
        if (rc != ACGPU_OK && !(rc == ACGPU_E_OVERFLOW && !counting)) {
            if (rc == ACGPU_E_OVERFLOW) total = n_k; // (a counting call: this shard's records did not fit, what lies before it is counted)
            result = rc;
            break;
        }
        if (!counting) total += n_k; // (beyond cap: the remaining shards only count)
        chain = piece_exit(rule, entry, c1, &sh, n_k);
        if (own_done) *own_done = c1;
    }
    if (result != ACGPU_OK) worker_rc.store(result); // (stops the producers)
    join_all();
    if (result == ACGPU_OK && worker_rc.load() != ACGPU_OK) result = worker_rc.load();
    (void)hipStreamSynchronize(d.copy_stream); // nothing of this call stays in flight
    if (result != ACGPU_OK && !(result == ACGPU_E_OVERFLOW && counting)) {
        if (result == ACGPU_E_HIP) g_last_hip_error = (int)hipGetLastError();
        return result;
    }
    *n_out = total;
    if (chain_io) *chain_io = chain;
    if (counting) return result;
    return total > cap ? ACGPU_E_OVERFLOW : ACGPU_OK;
}

// acgpu_match_u16 on a short haystack: ONE launch of one workgroup (acgpu_small.hip) that reads the haystack from, and writes
// the records to, host-mapped pinned memory; the host waits on a flag in that memory.  *handled = false: the kernel could not
// hold the call (too many occurrences) -- the general path takes it.
static int match_small(acgpu_automaton *a, DeviceState &d, const uint16_t *haystack, uint64_t n_units, int record_kind, void *out,
                uint64_t cap, uint64_t *n_out, bool *handled) {
    *handled = false;
    constexpr size_t kHayBytes = (size_t)kSmallMaxUnits * 2 + 64, kOutBytes = (size_t)kSmallMaxRecs * ACGPU_REC_MAP + 64;
    if (!d.small_pin) {
        // fine-grained (coherent) host memory: the device's writes are visible to the host while the kernel is still running
        HIP_TRY(hipHostMalloc(&d.small_pin.h, 64 + kHayBytes + kOutBytes, hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipHostGetDevicePointer(&d.small_pin_dev, d.small_pin, 0));
        HIP_TRY(hipStreamCreateWithFlags(&d.small_stream.h, hipStreamNonBlocking));
    }
    volatile unsigned long long *status = static_cast<volatile unsigned long long *>(d.small_pin.h);
    char *h_hay = (char *)d.small_pin.h + 64, *h_out = h_hay + kHayBytes;
    char *dev = (char *)d.small_pin_dev;
    std::memcpy(h_hay, haystack, n_units * 2);
    std::memset(h_hay + n_units * 2, 0, 8); // (the kernel reads whole 8-byte groups)
    status[0] = 0;
    status[1] = 0;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    SmallCall c{};
    c.hay = reinterpret_cast<const uint16_t *>(dev + 64);
    c.n_units = (uint32_t)n_units;
    c.record_kind = record_kind;
    c.out = dev + 64 + kHayBytes;
    c.cap = (uint32_t)std::min<uint64_t>(cap, kSmallMaxRecs);
    c.status = reinterpret_cast<unsigned long long *>(dev);
    HIP_TRY(launch_small(d.T, a->t.mode, c, d.small_stream));
    // the flag; every so often the stream itself, so that a launch that failed behind the call cannot hang the host
    for (uint64_t spins = 1;; ++spins) {
        if (status[0] != 0) break;
        if ((spins & 0xfffffu) == 0) {
            const hipError_t q = hipStreamQuery(d.small_stream);
            if (q != hipErrorNotReady && status[0] == 0) {
                if (q == hipSuccess) continue; // (finished: the flag is on its way)
                g_last_hip_error = (int)q;
                (void)hipGetLastError();
                return ACGPU_E_HIP;
            }
        }
    }
    std::atomic_thread_fence(std::memory_order_seq_cst);
    if (status[0] != 1) return ACGPU_OK; // not handled
    *handled = true;
    *n_out = status[1];
    if (*n_out > cap) return ACGPU_E_OVERFLOW;
    if (*n_out) std::memcpy(out, h_out, *n_out * (uint64_t)record_kind);
    return ACGPU_OK;
}

int match_host_text(acgpu_automaton *a, DeviceState &d, const uint16_t *haystack, uint64_t n_units, int record_kind, void *out,
                    uint64_t cap, uint64_t *n_out) {
    const HostTables &t = a->t;
    int rc;
    // short haystacks: one launch, no copies (tunable tile_debug bit kSelNoSmallCall, or a kernel form forced by "force_kernel": the
    // general path -- for A/B, and for the tests that run the scan kernels on the short edge-case inputs; bit kSelOnlySmallCall:
    // no general path -- a call the one launch does not answer itself is ACGPU_E_UNSUPPORTED, which tells a test who answered)
    if (n_units > 0 && n_units <= kSmallMaxUnits && d.inflight == 0 && small_call_supported(t) && !(tunables().tile_debug & kSelNoSmallCall) &&
        tunables().force_kernel == 0) {
        bool handled = false;
        rc = match_small(a, d, haystack, n_units, record_kind, out, cap, n_out, &handled);
        if (rc != ACGPU_OK || handled) return rc;
    }
    if (tunables().tile_debug & kSelOnlySmallCall) return ACGPU_E_UNSUPPORTED;
    // long haystacks: the pipelined form, unless the text is one piece (the loops that only exist as a sequential kernel over
    // the whole text -- WholeWord / WholeWordLongestSet with a fold-inconsistent table -- take the plain one)
    if (n_units >= 2 * kHostChunkUnits && !host_one_piece(t, record_kind) && d.inflight == 0 && !(tunables().tile_debug & kSelNoHostChunks)) {
        int64_t chain = 0;
        if ((rc = scan_host_range(a, d, haystack, n_units, 0, n_units, 0, n_units, record_kind, cap, n_out, &chain)) || !*n_out) return rc;
        HIP_TRY(hipMemcpyAsync(out, d.stage_out.p, *n_out * (uint64_t)record_kind, hipMemcpyDeviceToHost, d.call_stream));
        HIP_TRY(hipStreamSynchronize(d.call_stream));
        return ACGPU_OK;
    }
    acgpu_shard sh;
    if ((rc = d.stage_out.ensure(cap * (uint64_t)record_kind + 16))) return rc;
    if ((rc = stage_whole_text(d, haystack, n_units, &sh))) return rc;
    rc = match_shard(a, d, &sh, record_kind, d.stage_out.p, cap, n_out, nullptr, nullptr);
    if (rc != ACGPU_OK) return rc;
    if (*n_out) HIP_TRY(hipMemcpy(out, d.stage_out.p, *n_out * (uint64_t)record_kind, hipMemcpyDeviceToHost));
    return ACGPU_OK;
}

} // namespace acgpu

extern "C" {

int acgpu_match_u16(const acgpu_automaton *ca, const uint16_t *haystack, uint64_t n_units, int record_kind, void *out,
                    uint64_t cap, uint64_t *n_out) {
    if (!ca || !n_out || (n_units && !haystack) || (cap && !out)) return ACGPU_E_INVALID;
    if (record_kind != ACGPU_REC_SET && record_kind != ACGPU_REC_MAP) return ACGPU_E_INVALID;
    if (n_units >= (1ull << 31)) return ACGPU_E_INVALID;
    acgpu_automaton *a = const_cast<acgpu_automaton *>(ca);
    PoolCall call(a); // (the staging buffers are part of the per-device scratch pool)
    if (call.rc) return call.rc;
    return match_host_text(a, *call.d, haystack, n_units, record_kind, out, cap, n_out);
}

} // extern "C"
