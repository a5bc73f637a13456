// acgpu_stream.hip -- match(Readable, ReadableMatchListener<T>) (S/StringMap.java:6; S/AhoCorasickMap.java:208-275,
// S/LongestMatchMap.java:203-286, S/WholeWordMatchMap.java:55-153, S/ShortestMatchMap.java:199-291,
// S/WholeWordLongestMatchMap.java:54-181): the haystack arrives in chunks, the stream keeps what a later chunk can still change.
//
// Two forms of acgpu_stream_feed:
//  * synchronous (default): copy in, scan, copy out -- a feed returns the records ITS chunk made decidable;
//  * pipelined (acgpu_stream_set_pipelined): the chunk is copied into a pinned staging buffer by several host threads while the
//    calling thread scans the PREVIOUS chunk (whose transfer the previous feed enqueued) and returns ITS records; when the
//    copy is done the calling thread enqueues ONE transfer of the whole chunk (transfers enqueued piece by piece from
//    several threads made the launches of the scan slow): copy, transfer and scan of neighbouring chunks overlap, a feed
//    costs the slowest of them instead of their sum.  The last feed (final != 0) returns the records
//    of both the previous and its own chunk.  The concatenation over all feeds is the same in both forms.
// acgpu_stream_feed_utf8 is the synchronous form for a text that arrives as UTF-8 bytes: the stream carries BYTES, whole code points
// and behind them the prefix of a sequence that a chunk's end has cut; every feed transcodes [carried bytes | chunk] on the
// device (stage_utf8_parts, open at the end unless the feed is the last), scans it by the same plan in units and maps the
// records to bytes of that buffer.
// acgpu_stream_replace_u16 / acgpu_stream_replace_utf8 rewrite the text instead of reporting its records: the same buffers and the
// same plan, and over a feed's owned range the pieces of the replace entries (replace_feed, acgpu_replace.hip); the stream keeps
// `done`, the global position up to which output has been delivered.
// acgpu_stream_cover_u16 / acgpu_stream_cover_utf8 / acgpu_stream_cover_utf8_lossy cover the text instead (mask, highlight, redact):
// the same buffers and plan again, and over a feed's owned range the pieces of the cover entries (cover_feed, acgpu_cover.hip); the
// stream keeps `done`, whether it stands inside a span, and the few spans the merge withheld.
// acgpu_stream_feed_utf8_lossy / acgpu_stream_replace_utf8_lossy are the two byte entries' bodies with the other error policy
// (feed_utf8, stream_replace_utf8): nothing is refused, the buffer is staged through the validator that is both lossy and open,
// the carry is cut at a START found by the claim rule restated on the host (lossy_start, lossy_span), and the stream keeps the
// replaced count of what it carries.  The policy is part of the stream's kind.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <functional>
#include <new>
#include <optional>
#include <thread>
#include <vector>

#include "acgpu_host.h"

using namespace acgpu;

namespace {

// records device -> host-mapped pinned memory, coalesced 16-byte pieces (a hipMemcpy of the same 100 KB queues behind the
// chunk transfers that are in flight and takes as long as the scan)
__global__ void k_copy_out(const uint4 *src, uint4 *dst, uint64_t n16) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n16) dst[i] = src[i];
}

// what one feed scans, from lengths alone: the buffer is [carry | chunk] = `total` units, of which [own_begin, own_end) become
// decidable now, and the units from keep_from on are carried to the next feed
struct FeedPlan {
    uint64_t total, own_begin, own_end, keep_from;
};

FeedPlan plan_feed(const ShardRule &rule, uint64_t n_carry, uint64_t n_units, uint64_t own_from, uint64_t carry_pos, bool final) {
    FeedPlan p{};
    p.total = n_carry + n_units;
    p.own_begin = own_from - carry_pos;
    // the right halo is held back until a later chunk (or the end) brings it; the left context is carried
    p.own_end = final ? p.total : std::max<uint64_t>(p.own_begin, p.total > rule.right ? p.total - rule.right : 0);
    p.keep_from = p.own_end - std::min<uint64_t>(rule.left, p.own_end);
    return p;
}

// a feed's shard: sh names the buffer (d_hay, n_units); its owned range, the text's ends -- carry_pos is the global position of
// buffer unit 0 -- and where the chain enters it (a replace feed enters the chain itself: replace_feed)
void plan_shard(acgpu_shard *sh, const FeedPlan &p, uint64_t carry_pos, bool final, int64_t chain_entry = 0) {
    sh->own_begin = p.own_begin;
    sh->own_end = p.own_end;
    sh->text_begin = carry_pos == 0 ? 1 : 0;
    sh->text_end = final ? 1 : 0;
    sh->chain_entry = chain_entry;
}

// a few persistent host threads that copy pieces of a chunk (thread start-up costs as much as copying a megabyte)
class CopyPool {
  public:
    explicit CopyPool(int n) {
        for (int i = 0; i < n; ++i) workers_.emplace_back([this] { loop(); });
    }
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> l(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &w : workers_) w.join();
    }
    // runs job(i) for i in [0, n) on the workers and the calling thread; returns when all are done
    void run(int n, const std::function<void(int)> &job) {
        {
            std::lock_guard<std::mutex> l(mu_);
            job_ = &job;
            next_ = 0;
            n_ = n;
            left_ = n;
        }
        cv_.notify_all();
        work();
        std::unique_lock<std::mutex> l(mu_);
        done_.wait(l, [this] { return left_ == 0; });
        job_ = nullptr;
    }
    // the same, but the calling thread does something else meanwhile: start(), ..., wait()
    void start(int n, const std::function<void(int)> &job) {
        {
            std::lock_guard<std::mutex> l(mu_);
            job_ = &job;
            next_ = 0;
            n_ = n;
            left_ = n;
        }
        cv_.notify_all();
    }
    void wait() {
        work(); // (whatever is left)
        std::unique_lock<std::mutex> l(mu_);
        done_.wait(l, [this] { return left_ == 0; });
        job_ = nullptr;
    }

  private:
    void work() {
        for (;;) {
            int i;
            const std::function<void(int)> *job;
            {
                std::lock_guard<std::mutex> l(mu_);
                if (!job_ || next_ >= n_) return;
                i = next_++;
                job = job_;
            }
            (*job)(i);
            {
                std::lock_guard<std::mutex> l(mu_);
                if (--left_ == 0) done_.notify_all();
            }
        }
    }
    void loop() {
        for (;;) {
            {
                std::unique_lock<std::mutex> l(mu_);
                cv_.wait(l, [this] { return stop_ || (job_ && next_ < n_); });
                if (stop_) return;
            }
            work();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_, done_;
    std::vector<std::thread> workers_;
    const std::function<void(int)> *job_ = nullptr;
    int next_ = 0, n_ = 0, left_ = 0;
    bool stop_ = false;
};

// one chunk on its way: its units in pinned host memory and (soon) in device memory, and what its scan will be
struct Slot {
    bool pending = false; // transferred (or on its way), not yet scanned
    FeedPlan plan{};
    uint64_t carry_pos = 0; // global position of buffer unit 0
    bool final = false;
};

} // namespace

struct acgpu_stream {
    acgpu_automaton *a = nullptr;
    std::vector<uint16_t> carry; // units a later chunk can still change the answer for (context + held back)
    uint64_t carry_pos = 0;      // global position of carry[0]
    uint64_t own_from = 0;       // global position of the first unit no earlier feed has owned
    int64_t chain_entry = 0;     // the chain families: where the chain enters the next feed (global; piece_entry)
    bool finished = false;
    std::vector<uint16_t> buf;
    // ---- a stream of UTF-8 bytes (acgpu_stream_feed_utf8): carry_pos, own_from and chain_entry stay in units ----
    enum Fed : uint8_t {
        kFedNone, kFedUnits, kFedBytes, kFedReplaceUnits, kFedReplaceBytes, kFedBytesLossy, kFedReplaceBytesLossy,
        kFedCoverUnits, kFedCoverBytes, kFedCoverBytesLossy
    };
    Fed fed = kFedNone;          // what the first feed, of whatever length, made of the stream: every other entry refuses it
                                 // (the error policy of a stream of bytes is part of its kind: a strict feed on a lossy stream, and the reverse)
    uint64_t done = 0;           // a replace or cover stream: output has been delivered for the text in front of this global position,
                                 // in units (kFedReplaceUnits, kFedCoverUnits) or bytes; never in front of the carry's first
    bool in_span = false;        // a cover stream: `done` stands inside a span whose close has not been delivered
    std::vector<int64_t> spans;  // ... and the spans the merge withheld, {start, end} in the coordinates of `done` (CoverFeed::carried)
    std::vector<uint8_t> carry8; // the carried text's bytes, whole code points, then the held prefix
    uint32_t held = 0;           // bytes at carry8's end that begin a sequence the next feed must complete, 0..3
    uint64_t carry_units = 0;    // units that carry8 without the held prefix decodes to
    uint64_t carry_replaced = 0; // a lossy stream: of those, the U+FFFD that stand for ill-formed subparts (an earlier feed has reported them)
    uint64_t carry_byte = 0;     // global byte position of carry8[0]
    // ---- pipelined form ----
    bool pipelined = false, started = false;
    int device = -1;
    Slot slot[2];
    int cur = 0; // the slot the NEXT feed fills
    CopyPool *pool = nullptr;
    // the chunks' staging memory, and the records of one scan: a device buffer, and pinned host memory they are copied back to (a
    // hipMemcpy straight into the caller's pageable memory cost more than the scan of a chunk; kernels writing records into
    // host-mapped memory: 50x more).  Taken from / left to the automaton's cache (StreamBufs, acgpu_host.h).
    StreamBufs b;
    std::vector<char> undelivered;   // records a feed could not hand over (capacity too small): the same feed, called again, gets them
    uint64_t undelivered_n = 0;
    int64_t undelivered_base = 0;
    bool redeliver = false;
    ~acgpu_stream() {
        delete pool;
        if (a) { // (acgpu_free on an automaton with open streams detaches them: a == nullptr, nothing of it is touched here)
            std::lock_guard<std::mutex> l(a->mu);
            a->open_streams.erase(this);
        }
        if (device >= 0) {
            int cur_dev = -1;
            const bool have = hipGetDevice(&cur_dev) == hipSuccess;
            (void)hipSetDevice(device);
            if (b.copy_stream) (void)hipStreamSynchronize(b.copy_stream); // (nothing of this stream stays in flight)
            if (b.device >= 0 && a) { // (the buffers outlive the stream: the next one on this device takes them over)
                std::lock_guard<std::mutex> l(a->mu);
                try {
                    a->stream_cache.push_back(std::move(b));
                    b = StreamBufs();
                } catch (...) {
                }
            }
            if (b.device >= 0) b.release();
            if (have) (void)hipSetDevice(cur_dev);
        }
    }
};

namespace {

// scans the chunk in slot `sl` (its transfer has been enqueued) on the NULL stream and appends its records, relative to
// `base`, to out[n_done ..); *n_out = records so far (beyond cap: a count only)
int scan_slot(acgpu_stream *s, Slot &sl, int record_kind, void *out, uint64_t cap, uint64_t n_done, int64_t base, uint64_t *n_out) {
    acgpu_automaton *a = s->a;
    const ShardRule rule = shard_rule(a->t, record_kind, /*readable=*/true);
    const FeedPlan &p = sl.plan;
    const int si = (int)(&sl - s->slot);
    *n_out = n_done;
    const int64_t entry = piece_entry(rule, s->chain_entry, (int64_t)sl.carry_pos, p.own_begin);
    int64_t chain_exit = piece_exit(rule, entry, p.own_end, nullptr, 0);
    if (p.own_end > p.own_begin) {
        PoolCall call(a);
        if (call.rc) return call.rc;
        DeviceState *d = call.d;
        int rc;
        const bool trace = (tunables().tile_debug & kSelStreamTrace) != 0;
        const auto t0 = std::chrono::steady_clock::now();
        auto since = [&]() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); };
        if (trace) {
            HIP_TRY(hipEventSynchronize(s->b.arrived[si]));
            fprintf(stderr, "[scan] chunk arrived after %.0f us", since());
        }
        HIP_TRY(hipStreamWaitEvent(nullptr, s->b.arrived[si], 0));
        // (what the buffer holds already -- NOT a record more, or the buffer would grow by a quarter with every feed)
        uint64_t n = 0, scap = std::max<uint64_t>((s->b.out_dev.bytes > 16 ? s->b.out_dev.bytes - 16 : 0) / (uint64_t)record_kind, 1 << 16);
        acgpu_shard sh{};
        for (;;) { // (the scan keeps ALL its records: the caller's capacity only decides what this feed can hand over)
            if ((rc = s->b.out_dev.ensure(scap * (uint64_t)record_kind + 16))) return rc;
            sh = acgpu_shard{};
            sh.d_hay = (const uint16_t *)s->b.dev[si].p;
            sh.n_units = p.total;
            plan_shard(&sh, p, sl.carry_pos, sl.final, entry);
            rc = match_shard(a, *d, &sh, record_kind, s->b.out_dev.p, scap, &n, nullptr, nullptr, /*readable=*/true);
            if (rc == ACGPU_E_OVERFLOW) {
                scap = n + n / 8 + 16;
                continue;
            }
            if (rc) return rc;
            break;
        }
        if (trace) fprintf(stderr, ", scanned after %.0f us (%llu records)\n", since(), (unsigned long long)n);
        chain_exit = piece_exit(rule, entry, p.own_end, &sh, n);
        if (n) {
            // positions relative to `base` (the final feed hands over two chunks' records under one base)
            const int64_t delta = (int64_t)sl.carry_pos - base;
            const size_t bytes = n * (size_t)record_kind;
            char *dst;
            if (n_done + n <= cap) {
                dst = (char *)out + n_done * (size_t)record_kind;
            } else { // does not fit: kept for the call that comes back with the capacity
                try {
                    s->undelivered.resize((n_done + n) * (size_t)record_kind);
                } catch (...) {
                    return ACGPU_E_NOMEM;
                }
                if (n_done && n_done <= cap) std::memcpy(s->undelivered.data(), out, n_done * (size_t)record_kind);
                dst = s->undelivered.data() + n_done * (size_t)record_kind;
            }
            if (s->b.out_pin_bytes < bytes) {
                if (s->b.out_pin) (void)hipHostFree(s->b.out_pin);
                s->b.out_pin = nullptr;
                s->b.out_pin_bytes = 0;
                HIP_TRY(hipHostMalloc(&s->b.out_pin, bytes + bytes / 4 + 4096, hipHostMallocMapped));
                HIP_TRY(hipHostGetDevicePointer(&s->b.out_pin_dev, s->b.out_pin, 0));
                s->b.out_pin_bytes = bytes + bytes / 4 + 4096;
            }
            {
                const uint64_t n16 = (bytes + 15) / 16;
                hipLaunchKernelGGL(k_copy_out, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, nullptr, (const uint4 *)s->b.out_dev.p,
                                   (uint4 *)s->b.out_pin_dev, n16);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipStreamSynchronize(nullptr));
            }
            if (!delta) {
                std::memcpy(dst, s->b.out_pin, bytes);
            } else {
                const int32_t *src = reinterpret_cast<const int32_t *>(s->b.out_pin);
                int32_t *r = reinterpret_cast<int32_t *>(dst);
                const int cols = record_kind / 4;
                for (uint64_t i = 0; i < n; ++i) {
                    r[i * cols] = src[i * cols] + (int32_t)delta;
                    r[i * cols + 1] = src[i * cols + 1] + (int32_t)delta;
                    if (cols == 3) r[i * cols + 2] = src[i * cols + 2];
                }
            }
            *n_out = n_done + n;
        }
    }
    s->chain_entry = (int64_t)sl.carry_pos + chain_exit;
    sl.pending = false;
    return ACGPU_OK;
}

// The staging buffers, the copy stream and the events belong to the device of the FIRST feed (include/acgpu.h: every feed comes
// from a thread whose current device is that one).  A feed from another device -- a worker thread that another call left on a
// different device -- would scan device-A pointers with device-B tables: an error code instead.
int check_feed_device(const acgpu_stream *s) {
    if (s->device < 0) return ACGPU_OK;
    int cur = -1;
    HIP_TRY(hipGetDevice(&cur));
    return cur == s->device ? ACGPU_OK : ACGPU_E_INVALID;
}

// the stream's buffers: those a closed stream on this device left to the automaton, or none yet (they grow on demand)
int adopt_bufs(acgpu_stream *s) {
    if (s->b.device >= 0) return ACGPU_OK;
    if (s->device < 0) HIP_TRY(hipGetDevice(&s->device));
    std::lock_guard<std::mutex> l(s->a->mu);
    for (size_t i = 0; i < s->a->stream_cache.size(); ++i) {
        if (s->a->stream_cache[i].device != s->device) continue;
        s->b = std::move(s->a->stream_cache[i]);
        s->a->stream_cache.erase(s->a->stream_cache.begin() + (ptrdiff_t)i);
        return ACGPU_OK;
    }
    s->b.device = s->device;
    return ACGPU_OK;
}

int feed_pipelined(acgpu_stream *s, const uint16_t *units, uint64_t n_units, int final, int record_kind, void *out, uint64_t cap,
                   uint64_t *n_out, int64_t *base) {
    acgpu_automaton *a = s->a;
    if (!a) return ACGPU_E_INVALID; // (its automaton has been freed)
    *n_out = 0;
    { const int drc = check_feed_device(s); if (drc) return drc; }
    if (s->redeliver) { // the same feed again, with the capacity the first call reported: its chunk was consumed then
        *base = s->undelivered_base;
        *n_out = s->undelivered_n;
        if (s->undelivered_n > cap) return ACGPU_E_OVERFLOW;
        if (s->undelivered_n) std::memcpy(out, s->undelivered.data(), s->undelivered_n * (size_t)record_kind);
        s->redeliver = false;
        s->undelivered.clear();
        s->undelivered_n = 0;
        s->finished = final != 0;
        return ACGPU_OK;
    }
    if (!s->started) {
        if (s->device < 0) HIP_TRY(hipGetDevice(&s->device));
        { const int arc = adopt_bufs(s); if (arc) return arc; }
        if (!s->b.copy_stream) { // the transfers at the LOWEST priority: where they run as copy kernels they must not hold the scan's CUs
            int lo = 0, hi = 0;
            HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
            HIP_TRY(hipStreamCreateWithPriority(&s->b.copy_stream, hipStreamNonBlocking, lo));
        }
        for (auto &e : s->b.arrived)
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        const int workers = (int)std::min<unsigned>(5, std::max(1u, std::thread::hardware_concurrency() / 2));
        s->pool = new (std::nothrow) CopyPool(workers);
        if (!s->pool) return ACGPU_E_NOMEM;
        s->started = true;
    }
    const uint64_t n_carry = s->carry.size();
    // (half the synchronous form's limit: the final feed hands two chunks' records over under one base)
    if (n_carry + n_units >= (1ull << 30)) return ACGPU_E_INVALID;
    Slot &sl = s->slot[s->cur];
    Slot &prev = s->slot[1 - s->cur];
    const int si = s->cur;
    const FeedPlan p = plan_feed(shard_rule(a->t, record_kind, /*readable=*/true), n_carry, n_units, s->own_from, s->carry_pos, final != 0);
    int rc;
    if (s->b.pin_bytes[si] < p.total * 2 + 64) {
        if (s->b.pin[si]) (void)hipHostFree(s->b.pin[si]);
        s->b.pin[si] = nullptr;
        s->b.pin_bytes[si] = 0;
        const size_t want = p.total * 2 + p.total / 2 + 4096;
        HIP_TRY(hipHostMalloc(&s->b.pin[si], want, hipHostMallocNumaUser)); // (pages where the copying threads run, not on the device's node: 3x the copy rate)
        s->b.pin_bytes[si] = want;
    }
    if ((rc = s->b.dev[si].ensure(p.total * 2 + 64))) return rc;
    uint16_t *h = reinterpret_cast<uint16_t *>(s->b.pin[si]);
    if (n_carry) std::memcpy(h, s->carry.data(), n_carry * 2);
    // the chunk: pieces of 1 MiB copied by the pool's threads (units == our own staging memory: acgpu_stream_reserve --
    // nothing to copy).  The threads only copy; the ONE transfer of the whole buffer is enqueued by the calling thread behind
    // the previous chunk's scan (transfers enqueued from several threads while the scan's launches go out from this one made
    // every launch wait for the runtime: the scan took 310 us instead of 75)
    const bool in_place = units == h + n_carry;
    const uint64_t piece = 1ull << 19; // units
    const int n_pieces = in_place ? 0 : (int)((n_units + piece - 1) / piece);
    std::atomic<int> copy_rc{ACGPU_OK};
    std::function<void(int)> job = [&](int i) {
        const uint64_t o = (uint64_t)i * piece, len = std::min<uint64_t>(piece, n_units - o);
        std::memcpy(h + n_carry + o, units + o, len * 2);
    };
    const bool trace = (tunables().tile_debug & kSelStreamTrace) != 0; // development: where a feed's time goes (stderr)
    const auto t_start = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count(); };
    if (n_pieces) s->pool->start(n_pieces, job);
    const double t_started = since();
    // meanwhile: the previous chunk's scan, whose records this feed returns
    *base = prev.pending ? (int64_t)prev.carry_pos : (int64_t)s->carry_pos;
    int scan_rc = ACGPU_OK;
    uint64_t n_done = 0;
    if (prev.pending) scan_rc = scan_slot(s, prev, record_kind, out, cap, 0, *base, &n_done);
    const double t_scanned = since();
    if (n_pieces) s->pool->wait();
    if (trace) fprintf(stderr, "[feed] %llu units: copies started %.0f us, previous chunk scanned %.0f us, copies done %.0f us\n",
                       (unsigned long long)n_units, t_started, t_scanned, since());
    if (scan_rc == ACGPU_OK && copy_rc.load() != ACGPU_OK) scan_rc = copy_rc.load();
    if (scan_rc != ACGPU_OK) {
        (void)hipStreamSynchronize(s->b.copy_stream);
        s->finished = true; // (a stream that failed half way cannot go on)
        return scan_rc;
    }
    if (p.total) HIP_TRY(hipMemcpyAsync(s->b.dev[si].p, s->b.pin[si], p.total * 2, hipMemcpyHostToDevice, s->b.copy_stream));
    HIP_TRY(hipEventRecord(s->b.arrived[si], s->b.copy_stream));
    // commit this chunk
    sl.plan = p;
    sl.carry_pos = s->carry_pos;
    sl.final = final != 0;
    sl.pending = true;
    s->own_from = s->carry_pos + p.own_end;
    try {
        s->carry.assign(h + p.keep_from, h + p.total);
    } catch (...) {
        return ACGPU_E_NOMEM;
    }
    s->carry_pos += p.keep_from;
    s->cur = 1 - s->cur;
    if (final) { // nothing comes after it: its own records as well
        rc = scan_slot(s, sl, record_kind, out, cap, n_done, *base, &n_done);
        if (rc) {
            s->finished = true;
            return rc;
        }
    }
    *n_out = n_done;
    if (n_done > cap) { // the chunk HAS been consumed: the same feed, called again with this capacity, receives the records
        s->undelivered_n = n_done;
        s->undelivered_base = *base;
        s->redeliver = true;
        return ACGPU_E_OVERFLOW;
    }
    s->finished = final != 0;
    return ACGPU_OK;
}

// ---- what the synchronous feeds share (each entry keeps its argument checks and its middle) ----

// s->buf = [carry | chunk], p.total units
int join_units(acgpu_stream *s, const uint16_t *units, uint64_t n_units, const FeedPlan &p) {
    try {
        s->buf.resize(p.total);
    } catch (...) {
        return ACGPU_E_NOMEM;
    }
    if (!s->carry.empty()) std::memcpy(s->buf.data(), s->carry.data(), s->carry.size() * 2);
    if (n_units) std::memcpy(s->buf.data() + s->carry.size(), units, n_units * 2);
    return ACGPU_OK;
}

// the commit of a feed of units; chain_exit: buffer relative
void commit_units(acgpu_stream *s, const FeedPlan &p, int64_t chain_exit, bool final) {
    s->own_from = s->carry_pos + p.own_end;
    s->chain_entry = (int64_t)s->carry_pos + chain_exit;
    s->carry.assign(s->buf.begin() + (ptrdiff_t)p.keep_from, s->buf.end());
    s->carry_pos += p.keep_from;
    s->finished = final;
}

// A feed of bytes between its entry's argument checks and its commit.
struct ByteFeed {
    const uint8_t *bytes;
    uint64_t n_bytes;
    bool final;
    acgpu_utf8_stream_stats *stats; // the caller's, may be NULL
    acgpu_utf8_lossy_stream_stats *lossy_stats = nullptr; // a lossy feed's instead (lossy), may be NULL
    bool lossy = false;             // the stream's error policy: Utf8Errors::replace
    uint64_t n_c8 = 0, total_bytes = 0;
    bool go = false;                // begin: there is something to decode, the pool is held and the buffer staged
    std::optional<PoolCall> call;   // ... from begin to the entry's return
    Utf8Text text;                  // [carried bytes | chunk] on the device
    ShardRule rule{};
    FeedPlan p{};
    uint8_t at(const acgpu_stream *s, uint64_t i) const { return i < n_c8 ? s->carry8[i] : bytes[i - n_c8]; }
};

// The claim rule of lane_view's LOSSY form (acgpu_utf8.hip) restated on the host, for the few bytes byte_feed_commit walks.
// at(i): byte i of a text of `end` bytes; p: a START of it.  Returns the bytes of that start -- a lead with what it claims (the
// second byte in the range the lead allows, the later ones continuation bytes, never a byte at or behind `end`), or one byte that
// claims nothing (ASCII, a continuation byte, C0, C1, F5..FF) -- and *replaced: it is an ill-formed subpart, one U+FFFD.  4 bytes
// are a well-formed 4-byte sequence and nothing else: two units.
template <class At>
uint32_t lossy_span(const At &at, uint64_t p, uint64_t end, bool *replaced) {
    const uint32_t b0 = at(p);
    *replaced = b0 >= 0x80u;
    if (b0 < 0xc2u || b0 > 0xf4u) return 1;
    const uint32_t need = b0 < 0xe0u ? 1u : (b0 < 0xf0u ? 2u : 3u);
    const uint32_t lo = b0 == 0xe0u ? 0xa0u : (b0 == 0xf0u ? 0x90u : 0x80u), hi = b0 == 0xedu ? 0x9fu : (b0 == 0xf4u ? 0x8fu : 0xbfu);
    uint32_t got = 0;
    if (p + 1 < end && at(p + 1) >= lo && at(p + 1) <= hi) {
        got = 1;
        while (got < need && p + 1 + got < end && (at(p + 1 + got) & 0xc0u) == 0x80u) ++got;
    }
    *replaced = got < need;
    return 1 + got;
}

// ... byte i of that text is a start: no continuation byte, or one that the nearest byte before it that is none -- it looks at
// most 3 bytes back -- does not claim.  The text begins at a start (a stream's carry does, see byte_feed_commit): bytes before
// byte 0 claim nothing.
template <class At>
bool lossy_start(const At &at, uint64_t i, uint64_t end) {
    if ((at(i) & 0xc0u) != 0x80u) return true;
    for (uint64_t k = 1; k <= 3 && k <= i; ++k) {
        if ((at(i - k) & 0xc0u) == 0x80u) continue;
        bool replaced;
        return lossy_span(at, i - k, end, &replaced) <= k;
    }
    return true;
}

// The prologue of the byte feeds, from the stats' preset through plan_feed: returns what the entry returns where !f->go -- an
// empty feed, a failure, or ill-formed bytes (ACGPU_E_ENCODING, which finishes the stream; never on a lossy stream).
int byte_feed_begin(acgpu_stream *s, int record_kind, ByteFeed *f) {
    static_assert(sizeof(acgpu_utf8_stream_stats) == 24, "the layout include/acgpu.h promises");
    static_assert(sizeof(acgpu_utf8_lossy_stream_stats) == 24, "the layout include/acgpu.h promises");
    // the caller's stats, whichever the entry has: a lossy feed has n_replaced where a strict one has first_bad
    auto put = [f](const acgpu_utf8_stream_stats &st, uint64_t n_replaced) {
        if (f->stats) *f->stats = st;
        if (f->lossy_stats) *f->lossy_stats = acgpu_utf8_lossy_stream_stats{st.n_units, n_replaced, st.ascii, st.held};
    };
    f->n_c8 = s->carry8.size();
    f->total_bytes = f->n_c8 + f->n_bytes;
    acgpu_utf8_stream_stats st{};
    st.first_bad = -1;
    st.held = s->held;
    st.ascii = 1;
    for (uint8_t b : s->carry8) st.ascii &= b < 0x80u ? 1u : 0u;
    put(st, 0);
    if (f->n_bytes == 0 && !f->final) return ACGPU_OK; // (nothing new to decode or to decide: no device needed)
    if (f->total_bytes == 0) {                         // (the end of a stream that holds nothing: neither)
        s->finished = true;
        return ACGPU_OK;
    }
    PoolCall &call = f->call.emplace(s->a);
    if (call.rc) return call.rc;
    int rc;
    if ((rc = call.idle())) return rc; // (the call stream, waited for: see the stream rule)
    rc = stage_utf8_parts(*call.d, s->carry8.data(), f->n_c8, f->bytes, f->n_bytes, /*open=*/!f->final, call.d->call_stream, &f->text,
                          f->lossy ? Utf8Errors::replace : Utf8Errors::strict);
    if (rc == ACGPU_E_ENCODING) { // (the stream is idle: the pool is as usable as before the call; what a replace stream withheld stays undelivered)
        st.first_bad = (int64_t)s->carry_byte + f->text.first_bad; // (in an earlier feed's bytes: the lead of the held prefix)
        st.ascii = 0;
        st.held = 0;
        put(st, 0);
        s->finished = true;
        return rc;
    }
    if (rc) return call.fail(rc);
    if (f->text.n_units < s->carry_units) return call.fail(ACGPU_E_HIP); // (never: the carried code points decode as they did)
    // (lossy: nor were they replaced otherwise -- byte_feed_commit shows both; the carry's count makes the feeds' n_replaced sum
    // to the whole text's)
    if (f->text.n_replaced < s->carry_replaced) return call.fail(ACGPU_E_HIP);
    st.n_units = f->text.n_units - s->carry_units;
    st.ascii = f->text.n_units == f->total_bytes && !f->text.n_replaced; // ("a\x80b" has as many units as bytes)
    st.held = f->text.tail;
    put(st, f->text.n_replaced - s->carry_replaced);
    f->rule = shard_rule(s->a->t, record_kind, /*readable=*/true);
    f->p = plan_feed(f->rule, s->carry_units, f->text.n_units - s->carry_units, s->own_from, s->carry_pos, f->final);
    f->go = true;
    return ACGPU_OK;
}

// The epilogue of the byte feeds: the byte to cut the carry at, the next carry, the commit.  chain_exit: buffer relative.
// done: a replace stream's -- output exists for the buffer's bytes in front of *done, and the carry must reach back to it.
int byte_feed_commit(acgpu_stream *s, const ByteFeed &f, int64_t chain_exit, const uint64_t *done = nullptr) {
    // The cut is found on the host: back from the end of the decoded bytes over the leads -- every byte that is no continuation
    // byte begins a code point of one unit, of two from F0 up -- until at least total - keep_from units are covered.  That is a
    // code-point boundary; where keep_from names a low surrogate, one unit more is carried than the plan asks.
    //
    // A LOSSY stream cuts at a START: a lead, or a continuation byte nobody claimed -- a byte that is no continuation byte is not
    // enough to look for, "a 80 80" has three starts.  The walk restates the claim rule (lossy_start, lossy_span) over the bytes
    // it passes, at most 3 more behind each: back to the nearest start, which is one unit, or two where it is a well-formed
    // 4-byte sequence, and replaced where lossy_span says so.  These are the units the device counted: the decoded bytes
    // [0, n_bytes) were judged as a closed text of n_bytes bytes (lane_view, LOSSY and OPEN), which is what `end` says here.
    // Why a carry that begins at a start c decodes, with nothing before it, to the units it decoded to before -- the "never"
    // checks of byte_feed_begin: a claim is a run of continuation bytes directly behind its lead, so a lead before c that claimed
    // a byte at or behind c would have claimed c, and c is a start.  Which bytes from c on are claimed, by which lead, and
    // whether that lead got all it needs is therefore decided by bytes from c on alone.  And the units of the carried bytes
    // BEFORE the held prefix do not depend on what the next feed brings: those bytes were decoded as a text that ends where
    // the held lead stands, or at the buffer's end where nothing was held, and a lead among them whose claim reached that end
    // while it needed more IS the held lead -- every other start was decided by bytes that were there.
    const uint64_t need = f.p.total - f.p.keep_from;
    uint64_t cut = f.text.n_bytes, kept = 0, kept_replaced = 0;
    if (f.lossy) {
        auto at = [&](uint64_t i) { return (uint32_t)f.at(s, i); };
        while (kept < need && cut > 0) {
            --cut;
            while (cut > 0 && !lossy_start(at, cut, f.text.n_bytes)) --cut; // (byte 0 is a start)
            bool replaced;
            kept += lossy_span(at, cut, f.text.n_bytes, &replaced) == 4 ? 2u : 1u;
            kept_replaced += replaced ? 1u : 0u;
        }
    } else {
        while (kept < need && cut > 0) {
            const uint8_t b = f.at(s, --cut);
            if ((b & 0xc0u) != 0x80u) kept += b >= 0xf0u ? 2u : 1u;
        }
    }
    // the cut is the first byte of the code point that holds unit keep_from, or of the one before it, and `done` is at least the
    // byte that keep_from <= own_end - left rounds down to
    if (done && !f.final && *done < cut) return ACGPU_E_HIP;
    std::vector<uint8_t> next;
    try {
        next.resize(f.total_bytes - cut);
    } catch (...) {
        return ACGPU_E_NOMEM;
    }
    for (uint64_t i = cut; i < f.total_bytes; ++i) next[i - cut] = f.at(s, i);
    if (done) s->done = s->carry_byte + *done;
    s->own_from = s->carry_pos + f.p.own_end;
    s->chain_entry = (int64_t)s->carry_pos + chain_exit;
    s->carry8.swap(next);
    s->held = f.text.tail;
    s->carry_pos += f.p.total - kept;
    s->carry_units = kept;
    s->carry_replaced = kept_replaced;
    s->carry_byte += cut;
    s->finished = f.final;
    return ACGPU_OK;
}

} // namespace

extern "C" {

int acgpu_stream_open(const acgpu_automaton *a, acgpu_stream **out) {
    if (!a || !out) return ACGPU_E_INVALID;
    *out = nullptr;
    // (word-character tables that are not fold-consistent: the reference's Readable loops fold in EVERY lookup,
    // S/WholeWordMatchMap.java:112,117,328, S/WholeWordLongestMatchMap.java:404 -- ordinary scans over word o lower,
    // match_shard(..., readable))
    acgpu_stream *s = new (std::nothrow) acgpu_stream();
    if (!s) return ACGPU_E_NOMEM;
    s->a = const_cast<acgpu_automaton *>(a);
    try {
        std::lock_guard<std::mutex> l(s->a->mu);
        s->a->open_streams.insert(s);
    } catch (...) {
        s->a = nullptr;
        delete s;
        return ACGPU_E_NOMEM;
    }
    *out = s;
    return ACGPU_OK;
}

void acgpu_stream_close(acgpu_stream *s) { delete s; }

// acgpu_free with this stream still open (the caller holds the automaton's mutex): nothing of the stream refers to it any more;
// the staging buffers stay the stream's own and go when it is closed
void acgpu_stream_detach(acgpu_stream *s) { s->a = nullptr; }

int acgpu_stream_set_pipelined(acgpu_stream *s, int on) {
    if (!s || s->started || s->carry_pos != 0 || !s->carry.empty() || s->own_from != 0) return ACGPU_E_INVALID; // before the first feed
    if (s->fed != acgpu_stream::kFedNone && s->fed != acgpu_stream::kFedUnits) return ACGPU_E_INVALID;          // (of bytes or a replace stream as well)
    s->pipelined = on != 0;
    return ACGPU_OK;
}

int acgpu_stream_reserve(acgpu_stream *s, uint64_t n_units, uint16_t **buf) {
    if (!s || !buf || !s->pipelined || s->finished || s->redeliver) return ACGPU_E_INVALID;
    *buf = nullptr;
    const uint64_t n_carry = s->carry.size();
    if (n_carry + n_units >= (1ull << 30) || !s->a) return ACGPU_E_INVALID;
    { const int drc = check_feed_device(s); if (drc) return drc; }
    const int si = s->cur;
    { const int arc = adopt_bufs(s); if (arc) return arc; }
    if (s->b.pin_bytes[si] < (n_carry + n_units) * 2 + 64) {
        if (s->b.pin[si]) (void)hipHostFree(s->b.pin[si]);
        s->b.pin[si] = nullptr;
        s->b.pin_bytes[si] = 0;
        const size_t want = (n_carry + n_units) * 2 + (n_carry + n_units) / 2 + 4096;
        HIP_TRY(hipHostMalloc(&s->b.pin[si], want, hipHostMallocNumaUser)); // (pages where the copying threads run, not on the device's node: 3x the copy rate)
        s->b.pin_bytes[si] = want;
    }
    *buf = reinterpret_cast<uint16_t *>(s->b.pin[si]) + n_carry;
    return ACGPU_OK;
}

int acgpu_stream_feed(acgpu_stream *s, const uint16_t *units, uint64_t n_units, int final, int record_kind, void *out,
                      uint64_t cap, uint64_t *n_out, int64_t *base) {
    if (!s || !n_out || !base || (n_units && !units) || (cap && !out) || s->finished) return ACGPU_E_INVALID;
    if (record_kind != ACGPU_REC_SET && record_kind != ACGPU_REC_MAP) return ACGPU_E_INVALID;
    if (!s->a) return ACGPU_E_INVALID; // (its automaton has been freed)
    if (s->fed != acgpu_stream::kFedNone && s->fed != acgpu_stream::kFedUnits) return ACGPU_E_INVALID; // (a stream of another kind: bytes, or a replace stream)
    s->fed = acgpu_stream::kFedUnits;
    if (s->pipelined) return feed_pipelined(s, units, n_units, final, record_kind, out, cap, n_out, base);
    acgpu_automaton *a = s->a;
    const ShardRule rule = shard_rule(a->t, record_kind, /*readable=*/true);
    const FeedPlan p = plan_feed(rule, s->carry.size(), n_units, s->own_from, s->carry_pos, final != 0);
    if (p.total >= (1ull << 31)) return ACGPU_E_INVALID;
    *n_out = 0;
    *base = (int64_t)s->carry_pos;
    int rc;
    if ((rc = join_units(s, units, n_units, p))) return rc;
    const int64_t entry = piece_entry(rule, s->chain_entry, (int64_t)s->carry_pos, p.own_begin);
    int64_t chain_exit = piece_exit(rule, entry, p.own_end, nullptr, 0);
    if (p.own_end > p.own_begin) {
        PoolCall call(a); // (the staging buffers are part of the per-device scratch pool)
        if (call.rc) return call.rc;
        DeviceState *d = call.d;
        acgpu_shard sh;
        if ((rc = d->stage_out.ensure(cap * (uint64_t)record_kind + 16))) return rc;
        if ((rc = stage_whole_text(*d, s->buf.data(), p.total, &sh))) return rc; // (the carry and the fed units: then the owned range, the ends and the chain)
        plan_shard(&sh, p, s->carry_pos, final != 0, entry);
        rc = match_shard(a, *d, &sh, record_kind, d->stage_out.p, cap, n_out, nullptr, nullptr, /*readable=*/true);
        if (rc != ACGPU_OK) return rc; // ACGPU_E_OVERFLOW: nothing consumed, *n_out = capacity to retry with
        if (*n_out) HIP_TRY(hipMemcpy(out, d->stage_out.p, *n_out * (uint64_t)record_kind, hipMemcpyDeviceToHost));
        chain_exit = piece_exit(rule, entry, p.own_end, &sh, *n_out);
    }
    commit_units(s, p, chain_exit, final != 0);
    return ACGPU_OK;
}

} // extern "C"

namespace {

// The body of acgpu_stream_feed_utf8 and acgpu_stream_feed_utf8_lossy: exactly one of stats and lossy_stats is the entry's (either
// may be NULL).  The policy is part of the stream's kind.
int feed_utf8(acgpu_stream *s, const uint8_t *bytes, uint64_t n_bytes, int final, int record_kind, void *out, uint64_t cap, uint64_t *n_out,
              int64_t *base, bool lossy, acgpu_utf8_stream_stats *stats, acgpu_utf8_lossy_stream_stats *lossy_stats) {
    if (!s || !n_out || !base || (n_bytes && !bytes) || (cap && !out) || s->finished) return ACGPU_E_INVALID;
    if (record_kind != ACGPU_REC_SET && record_kind != ACGPU_REC_MAP) return ACGPU_E_INVALID;
    if (!s->a) return ACGPU_E_INVALID; // (its automaton has been freed)
    if (s->pipelined) return ACGPU_E_UNSUPPORTED;
    const acgpu_stream::Fed kind = lossy ? acgpu_stream::kFedBytesLossy : acgpu_stream::kFedBytes;
    if (s->fed != acgpu_stream::kFedNone && s->fed != kind) return ACGPU_E_INVALID; // (a stream of another kind: units, a replace stream, bytes under the other policy)
    if (n_bytes >= (1ull << 31) || s->carry8.size() + n_bytes >= (1ull << 31)) return ACGPU_E_INVALID;
    s->fed = kind;
    *n_out = 0;
    *base = (int64_t)s->carry_byte;
    ByteFeed f{bytes, n_bytes, final != 0, stats, lossy_stats, lossy};
    int rc = byte_feed_begin(s, record_kind, &f);
    if (!f.go) return rc;
    acgpu_automaton *a = s->a;
    const PoolCall &call = *f.call;
    DeviceState &d = *call.d;
    const hipStream_t stream = d.call_stream;
    const FeedPlan &p = f.p;
    const int64_t entry = piece_entry(f.rule, s->chain_entry, (int64_t)s->carry_pos, p.own_begin);
    int64_t chain_exit = piece_exit(f.rule, entry, p.own_end, nullptr, 0);
    if (p.own_end > p.own_begin) {
        if ((rc = d.stage_out.ensure(cap * (uint64_t)record_kind + 16))) return call.fail(rc);
        acgpu_shard &sh = f.text.shard; // (all the buffer's units: then the owned range, the ends and the chain)
        plan_shard(&sh, p, s->carry_pos, f.final, entry);
        rc = match_shard(a, d, &sh, record_kind, d.stage_out.p, cap, n_out, stream, nullptr, /*readable=*/true);
        if (rc != ACGPU_OK) return rc; // ACGPU_E_OVERFLOW: nothing consumed, *n_out = capacity to retry with
        if (*n_out) {
            if ((rc = utf8_map_records(f.text, nullptr, reinterpret_cast<int32_t *>(d.stage_out.p), *n_out, (uint32_t)record_kind / 4, stream))) return call.fail(rc);
            if (hipMemcpyAsync(out, d.stage_out.p, *n_out * (uint64_t)record_kind, hipMemcpyDeviceToHost, stream) != hipSuccess ||
                hipStreamSynchronize(stream) != hipSuccess)
                return call.fail(ACGPU_E_HIP);
        }
        chain_exit = piece_exit(f.rule, entry, p.own_end, &sh, *n_out);
    }
    return byte_feed_commit(s, f, chain_exit);
}

} // namespace

extern "C" {

int acgpu_stream_feed_utf8(acgpu_stream *s, const uint8_t *bytes, uint64_t n_bytes, int final, int record_kind, void *out, uint64_t cap,
                           uint64_t *n_out, int64_t *base, acgpu_utf8_stream_stats *stats) {
    return feed_utf8(s, bytes, n_bytes, final, record_kind, out, cap, n_out, base, /*lossy=*/false, stats, nullptr);
}

int acgpu_stream_feed_utf8_lossy(acgpu_stream *s, const uint8_t *bytes, uint64_t n_bytes, int final, int record_kind, void *out, uint64_t cap,
                                 uint64_t *n_out, int64_t *base, acgpu_utf8_lossy_stream_stats *stats) {
    return feed_utf8(s, bytes, n_bytes, final, record_kind, out, cap, n_out, base, /*lossy=*/true, nullptr, stats);
}

int acgpu_stream_replace_u16(acgpu_stream *s, const uint16_t *units, uint64_t n_units, int final, const uint16_t *repl_units,
                             const uint64_t *repl_off, uint32_t n_repl, uint16_t *out, uint64_t cap, uint64_t *n_out, acgpu_replace_stats *st) {
    if (!s || !n_out || (n_units && !units) || (cap && !out) || s->finished) return ACGPU_E_INVALID;
    if (!s->a) return ACGPU_E_INVALID; // (its automaton has been freed)
    if (s->fed != acgpu_stream::kFedNone && s->fed != acgpu_stream::kFedReplaceUnits) return ACGPU_E_INVALID; // (a stream of another kind)
    acgpu_automaton *a = s->a;
    int rc = replace_check_table(a, repl_units, repl_off, n_repl);
    if (rc) return rc;
    if (s->pipelined) return ACGPU_E_UNSUPPORTED;
    const ShardRule rule = shard_rule(a->t, ACGPU_REC_MAP, /*readable=*/true);
    const FeedPlan p = plan_feed(rule, s->carry.size(), n_units, s->own_from, s->carry_pos, final != 0);
    if (n_units >= (1ull << 31) || p.total >= (1ull << 31)) return ACGPU_E_INVALID;
    s->fed = acgpu_stream::kFedReplaceUnits;
    *n_out = 0;
    if (st) *st = acgpu_replace_stats{};
    if (n_units == 0 && !final) return ACGPU_OK; // (nothing new to decide: no device needed)
    if (p.total == 0) {                          // (the end of a stream that holds nothing: neither)
        s->finished = true;
        return ACGPU_OK;
    }
    if (s->done < s->carry_pos) return ACGPU_E_HIP; // (never: the carry invariant, checked at every commit)
    if ((rc = join_units(s, units, n_units, p))) return rc;
    ReplaceFeed f;
    f.final = final != 0;
    f.done = s->done - s->carry_pos;
    f.chain = s->chain_entry - (int64_t)s->carry_pos;
    if (p.own_end > p.own_begin || (final && f.done < p.total)) {
        PoolCall call(a);
        if (call.rc) return call.rc;
        DeviceState &d = *call.d;
        if ((rc = call.idle())) return rc; // (the call stream, waited for: see the stream rule)
        if ((rc = stage_whole_text(d, s->buf.data(), p.total, &f.shard))) return rc; // (the carry and the fed units: then the owned range and the ends)
        plan_shard(&f.shard, p, s->carry_pos, f.final);
        rc = replace_feed(a, d, &f, repl_units, repl_off, n_repl, out, cap, n_out);
        if (rc == ACGPU_OK || rc == ACGPU_E_OVERFLOW) {
            if (st) *st = f.st;
        }
        if (rc == ACGPU_E_OVERFLOW) return rc; // nothing committed: the same feed again, with *n_out units of room
        if (rc) return call.fail(rc);
    } else { // (nothing owned yet: the chain passes through)
        f.chain = piece_exit(rule, piece_entry(rule, f.chain, 0, p.own_begin), p.own_end, nullptr, 0);
    }
    // the carry must reach back to `done`: keep_from <= own_end - left <= done by the limit rule
    if (!final && f.done < p.keep_from) return ACGPU_E_HIP;
    s->done = s->carry_pos + f.done;
    commit_units(s, p, f.chain, f.final);
    return ACGPU_OK;
}

} // extern "C"

namespace {

// The body of acgpu_stream_replace_utf8 and acgpu_stream_replace_utf8_lossy (ust or lossy_ust: as feed_utf8's stats).  Lossy: the
// feed's buffer is staged with the other policy and that is all -- the pieces map records and boundaries through the start
// bitmap, and the emit copies the caller's bytes as they are, so a held prefix (the bytes behind text.n_bytes) stays undelivered
// until the bytes that complete it, or fail to, or the final feed decide what it is.
int stream_replace_utf8(acgpu_stream *s, const uint8_t *bytes, uint64_t n_bytes, int final, const uint8_t *repl_bytes, const uint64_t *repl_off,
                        uint32_t n_repl, uint8_t *out, uint64_t cap, uint64_t *n_out, bool lossy, acgpu_utf8_stream_stats *ust,
                        acgpu_utf8_lossy_stream_stats *lossy_ust, acgpu_replace_stats *rst) {
    if (!s || !n_out || (n_bytes && !bytes) || (cap && !out) || s->finished) return ACGPU_E_INVALID;
    if (!s->a) return ACGPU_E_INVALID; // (its automaton has been freed)
    const acgpu_stream::Fed kind = lossy ? acgpu_stream::kFedReplaceBytesLossy : acgpu_stream::kFedReplaceBytes;
    if (s->fed != acgpu_stream::kFedNone && s->fed != kind) return ACGPU_E_INVALID; // (a stream of another kind)
    acgpu_automaton *a = s->a;
    int rc = replace_check_table(a, repl_bytes, repl_off, n_repl);
    if (rc) return rc;
    if (s->pipelined || a->t.lone_surrogate) return ACGPU_E_UNSUPPORTED; // (the latter: as acgpu_replace_utf8)
    if (n_bytes >= (1ull << 31) || s->carry8.size() + n_bytes >= (1ull << 31)) return ACGPU_E_INVALID;
    s->fed = kind;
    *n_out = 0;
    if (rst) *rst = acgpu_replace_stats{};
    ByteFeed bf{bytes, n_bytes, final != 0, ust, lossy_ust, lossy};
    rc = byte_feed_begin(s, ACGPU_REC_MAP, &bf);
    if (!bf.go) return rc;
    const PoolCall &call = *bf.call;
    const FeedPlan &p = bf.p;
    if (s->done < s->carry_byte) return call.fail(ACGPU_E_HIP); // (never: the carry invariant, checked at every commit)
    ReplaceFeed f;
    f.u8 = &bf.text;
    f.final = bf.final;
    f.done = s->done - s->carry_byte; // (bytes of the buffer)
    f.chain = s->chain_entry - (int64_t)s->carry_pos;
    if (p.own_end > p.own_begin || (final && f.done < bf.text.n_bytes)) {
        f.shard = bf.text.shard; // (all the buffer's units: then the owned range and the ends)
        plan_shard(&f.shard, p, s->carry_pos, f.final);
        rc = replace_feed(a, *call.d, &f, repl_bytes, repl_off, n_repl, out, cap, n_out);
        if (rc == ACGPU_OK || rc == ACGPU_E_OVERFLOW) {
            if (rst) *rst = f.st;
        }
        if (rc == ACGPU_E_OVERFLOW) return rc; // nothing committed: the same feed again, with *n_out bytes of room
        if (rc) return call.fail(rc);
    } else { // (nothing owned yet: the chain passes through)
        f.chain = piece_exit(bf.rule, piece_entry(bf.rule, f.chain, 0, p.own_begin), p.own_end, nullptr, 0);
    }
    return byte_feed_commit(s, bf, f.chain, &f.done);
}

} // namespace

extern "C" {

int acgpu_stream_replace_utf8(acgpu_stream *s, const uint8_t *bytes, uint64_t n_bytes, int final, const uint8_t *repl_bytes,
                              const uint64_t *repl_off, uint32_t n_repl, uint8_t *out, uint64_t cap, uint64_t *n_out,
                              acgpu_utf8_stream_stats *ust, acgpu_replace_stats *rst) {
    return stream_replace_utf8(s, bytes, n_bytes, final, repl_bytes, repl_off, n_repl, out, cap, n_out, /*lossy=*/false, ust, nullptr, rst);
}

int acgpu_stream_replace_utf8_lossy(acgpu_stream *s, const uint8_t *bytes, uint64_t n_bytes, int final, const uint8_t *repl_bytes,
                                    const uint64_t *repl_off, uint32_t n_repl, uint8_t *out, uint64_t cap, uint64_t *n_out,
                                    acgpu_utf8_lossy_stream_stats *ust, acgpu_replace_stats *rst) {
    return stream_replace_utf8(s, bytes, n_bytes, final, repl_bytes, repl_off, n_repl, out, cap, n_out, /*lossy=*/true, nullptr, ust, rst);
}

} // extern "C"

namespace {

// An empty final feed on a cover stream whose text is delivered to its end: all that is left is the close of the span `done`
// stands in, if it stands in one.  No device: close is the caller's, in host memory.
int cover_close_on_host(acgpu_stream *s, const acgpu_cover_spec *spec, uint32_t esz, void *out, uint64_t cap, uint64_t *n_out, acgpu_cover_stats *st) {
    const uint64_t n = s->in_span ? spec->close_len : 0;
    *n_out = n;
    if (st) st->units_out = n;
    if (n > cap) return ACGPU_E_OVERFLOW; // (nothing committed: the same feed again)
    if (n) std::memcpy(out, spec->close, (size_t)n * esz);
    s->in_span = false;
    s->spans.clear();
    s->finished = true;
    return ACGPU_OK;
}

// the stream's state in front of a feed -> f (positions relative to the buffer, whose element 0 is global `origin`)
void cover_feed_in(const acgpu_stream *s, uint64_t origin, bool final, CoverFeed *f) {
    f->final = final;
    f->done = s->done - origin;
    f->in_span = s->in_span;
    f->origin = origin;
    f->carried = s->spans;
    f->chain = s->chain_entry - (int64_t)s->carry_pos;
}

// The body of acgpu_stream_cover_utf8 and acgpu_stream_cover_utf8_lossy (ust or lossy_ust: as feed_utf8's stats).
int stream_cover_utf8(acgpu_stream *s, const uint8_t *bytes, uint64_t n_bytes, int final, const acgpu_cover_spec *spec, uint8_t *out, uint64_t cap,
                      uint64_t *n_out, bool lossy, acgpu_utf8_stream_stats *ust, acgpu_utf8_lossy_stream_stats *lossy_ust, acgpu_cover_stats *st) {
    if (!s || !n_out || (n_bytes && !bytes) || (cap && !out) || s->finished) return ACGPU_E_INVALID;
    if (!s->a) return ACGPU_E_INVALID; // (its automaton has been freed)
    const acgpu_stream::Fed kind = lossy ? acgpu_stream::kFedCoverBytesLossy : acgpu_stream::kFedCoverBytes;
    if (s->fed != acgpu_stream::kFedNone && s->fed != kind) return ACGPU_E_INVALID; // (a stream of another kind)
    acgpu_automaton *a = s->a;
    int rc = cover_check_spec(spec, 1);
    if (rc) return rc;
    if (s->pipelined) return ACGPU_E_UNSUPPORTED;
    if (n_bytes >= (1ull << 31) || s->carry8.size() + n_bytes >= (1ull << 31)) return ACGPU_E_INVALID;
    s->fed = kind;
    *n_out = 0;
    if (st) *st = acgpu_cover_stats{};
    ByteFeed bf{bytes, n_bytes, final != 0, ust, lossy_ust, lossy};
    rc = byte_feed_begin(s, ACGPU_REC_SET, &bf);
    if (!bf.go) {
        // (the end of a stream that holds nothing, inside a span: its close; an overflow leaves the stream open for the same feed)
        if (rc == ACGPU_OK && final && (rc = cover_close_on_host(s, spec, 1, out, cap, n_out, st)) == ACGPU_E_OVERFLOW) s->finished = false;
        return rc;
    }
    const PoolCall &call = *bf.call;
    const FeedPlan &p = bf.p;
    if (s->done < s->carry_byte) return call.fail(ACGPU_E_HIP); // (never: the carry invariant, checked at every commit)
    CoverFeed f;
    cover_feed_in(s, s->carry_byte, bf.final, &f); // (bytes of the buffer)
    f.u8 = &bf.text;
    if (p.own_end > p.own_begin || final) {
        f.shard = bf.text.shard; // (all the buffer's units: then the owned range and the ends)
        plan_shard(&f.shard, p, s->carry_pos, f.final);
        rc = cover_feed(a, *call.d, &f, spec, out, cap, n_out);
        if (rc == ACGPU_OK || rc == ACGPU_E_OVERFLOW) {
            if (st) *st = f.st;
        }
        if (rc == ACGPU_E_OVERFLOW) return rc; // nothing committed: the same feed again, with *n_out bytes of room
        if (rc) return call.fail(rc);
    } else { // (nothing owned yet: the chain passes through)
        f.chain = piece_exit(bf.rule, piece_entry(bf.rule, f.chain, 0, p.own_begin), p.own_end, nullptr, 0);
    }
    if ((rc = byte_feed_commit(s, bf, f.chain, &f.done))) return rc; // (s->done: global again)
    s->in_span = f.in_span;
    s->spans.swap(f.carried);
    return ACGPU_OK;
}

} // namespace

extern "C" {

int acgpu_stream_cover_u16(acgpu_stream *s, const uint16_t *units, uint64_t n_units, int final, const acgpu_cover_spec *spec, uint16_t *out, uint64_t cap,
                           uint64_t *n_out, acgpu_cover_stats *st) {
    if (!s || !n_out || (n_units && !units) || (cap && !out) || s->finished) return ACGPU_E_INVALID;
    if (!s->a) return ACGPU_E_INVALID; // (its automaton has been freed)
    if (s->fed != acgpu_stream::kFedNone && s->fed != acgpu_stream::kFedCoverUnits) return ACGPU_E_INVALID; // (a stream of another kind)
    acgpu_automaton *a = s->a;
    int rc = cover_check_spec(spec, 2);
    if (rc) return rc;
    if (s->pipelined) return ACGPU_E_UNSUPPORTED;
    const ShardRule rule = shard_rule(a->t, ACGPU_REC_SET, /*readable=*/true);
    const FeedPlan p = plan_feed(rule, s->carry.size(), n_units, s->own_from, s->carry_pos, final != 0);
    if (n_units >= (1ull << 31) || p.total >= (1ull << 31)) return ACGPU_E_INVALID;
    s->fed = acgpu_stream::kFedCoverUnits;
    *n_out = 0;
    if (st) *st = acgpu_cover_stats{};
    if (n_units == 0 && !final) return ACGPU_OK; // (nothing new to decide: no device needed)
    if (s->done < s->carry_pos) return ACGPU_E_HIP; // (never: the carry invariant, checked at every commit)
    // (the end of a text that has been delivered to its end -- a stream that holds nothing included: no device needed either)
    if (final && p.own_end == p.own_begin && s->done - s->carry_pos == p.total) return cover_close_on_host(s, spec, 2, out, cap, n_out, st);
    if ((rc = join_units(s, units, n_units, p))) return rc;
    CoverFeed f;
    cover_feed_in(s, s->carry_pos, final != 0, &f);
    if (p.own_end > p.own_begin || final) {
        PoolCall call(a);
        if (call.rc) return call.rc;
        DeviceState &d = *call.d;
        if ((rc = call.idle())) return rc; // (the call stream, waited for: see the stream rule)
        if ((rc = stage_whole_text(d, s->buf.data(), p.total, &f.shard))) return rc; // (the carry and the fed units: then the owned range and the ends)
        plan_shard(&f.shard, p, s->carry_pos, f.final);
        rc = cover_feed(a, d, &f, spec, out, cap, n_out);
        if (rc == ACGPU_OK || rc == ACGPU_E_OVERFLOW) {
            if (st) *st = f.st;
        }
        if (rc == ACGPU_E_OVERFLOW) return rc; // nothing committed: the same feed again, with *n_out units of room
        if (rc) return call.fail(rc);
    } else { // (nothing owned yet: the chain passes through)
        f.chain = piece_exit(rule, piece_entry(rule, f.chain, 0, p.own_begin), p.own_end, nullptr, 0);
    }
    // the carry must reach back to `done`: keep_from = own_end - left never lies behind B
    if (!final && f.done < p.keep_from) return ACGPU_E_HIP;
    s->done = s->carry_pos + f.done;
    s->in_span = f.in_span;
    s->spans.swap(f.carried);
    commit_units(s, p, f.chain, f.final);
    return ACGPU_OK;
}

int acgpu_stream_cover_utf8(acgpu_stream *s, const uint8_t *bytes, uint64_t n_bytes, int final, const acgpu_cover_spec *spec, uint8_t *out, uint64_t cap,
                            uint64_t *n_out, acgpu_utf8_stream_stats *ust, acgpu_cover_stats *st) {
    return stream_cover_utf8(s, bytes, n_bytes, final, spec, out, cap, n_out, /*lossy=*/false, ust, nullptr, st);
}

int acgpu_stream_cover_utf8_lossy(acgpu_stream *s, const uint8_t *bytes, uint64_t n_bytes, int final, const acgpu_cover_spec *spec, uint8_t *out,
                                  uint64_t cap, uint64_t *n_out, acgpu_utf8_lossy_stream_stats *ust, acgpu_cover_stats *st) {
    return stream_cover_utf8(s, bytes, n_bytes, final, spec, out, cap, n_out, /*lossy=*/true, nullptr, ust, st);
}

} // extern "C"
