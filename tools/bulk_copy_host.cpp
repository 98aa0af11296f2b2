// The chunk protocol of the staged host <-> device copies (figaroh_plus_amd/csrc/figh_bulk_copy.h) on the CPU, driven
// through a fake transport: no device, no library.  tests/test_bulk_copy_host.py compiles this file twice and runs it.
// Build, from the repository root (build/ is git-ignored):
//   c++ -std=c++17 -O2 -pthread -Ifigaroh_plus_amd/csrc tools/bulk_copy_host.cpp -o build/bulk_copy_host
//   c++ -std=c++17 -O1 -g -fsanitize=thread -pthread -Ifigaroh_plus_amd/csrc tools/bulk_copy_host.cpp -o build/bulk_copy_host_tsan
// Run:  bulk_copy_host [all | slices | cases | errors | plant-early-wait | plant-misroute | plant-drop-byte]
// Exit status 0: every run passed; 1: some run failed (its first violation is printed); 2: usage.
//
// The fake transport.  One engine thread executes the enqueued operations strictly in order, as a stream does; device memory
// is a host array; an event completes when the engine reaches its record, and wait() blocks on a mutex and a condition
// variable until then -- the happens-before edge of an event synchronisation, and the only one the fake offers between the
// engine and the copy threads.  Seeded jitter (sleeps and yields chosen from the seed) sits in the engine, between taking
// an operation and carrying it out, and in the slice copy, so that runs cover the DMA far ahead of the copy threads, far
// behind them, and mixtures.  The transport's own checks use relaxed atomics only, which order nothing: they neither hide
// a race of the protocol from ThreadSanitizer nor depend on it.  Checked:
//   device -> host: when the engine starts to write a staging buffer no slice copy on it is in flight, and the slices taken
//     from the chunk it last held tile that chunk exactly (every byte consumed once); a slice is read only from a buffer
//     that holds all of its chunk and that the engine is not writing; at the staging offset of its host offset.
//   host -> device: the engine reads a staging buffer only when the slices written tile all n bytes of the chunk and nobody
//     is writing it; a slice is written only into a buffer whose previous chunk the engine has finished reading; each
//     chunk goes to its own device offset with its own length.
//   after the copy: destination == source byte for byte; the guard bytes behind `bytes` keep their sentinel.
// Error runs make operation number j of a copy fail (every j in turn): bulk_copy returns that code, returns at all (its
// threads are joined before it does), and issues no operation after the failing one but drain().  Slice copies of threads
// that were already released may still finish.  The path "the copy threads could not be started" (kBulkNotStarted) is not
// exercised: it needs std::thread's constructor to throw.
// Planted transports show that the checks detect: wait() that returns at once (plain build: a check fires; ThreadSanitizer:
// a data race between the engine's staging write and a worker's read), one chunk routed to the other staging buffer, the
// last byte of one slice dropped.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#if defined(__linux__)
#include <pthread.h>
#endif

#include "figh_bulk_copy.h"

namespace {

constexpr size_t kGuard = 64;
constexpr unsigned char kSentinel = 0xA5, kStageFill = 0x5A;
constexpr int kSlots = 64;

enum Plant { kNoPlant, kEarlyWait, kMisroute, kDropByte };

// the first violation of the current run (the failure path alone takes this mutex)
std::mutex g_vmutex;
std::atomic<int> g_violations{0};
std::string g_first;

void violation(const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lock(g_vmutex);
    if (g_violations.fetch_add(1, std::memory_order_relaxed) == 0) g_first = buf;
}

void name_thread(const char *name) {
#if defined(__linux__)
    pthread_setname_np(pthread_self(), name);
#else
    (void)name;
#endif
}

struct Rng {
    uint64_t s;
    uint64_t next() {
        s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
        return s * 0x2545F4914F6CDD1DULL;
    }
};

void sleep_us(unsigned us) { std::this_thread::sleep_for(std::chrono::microseconds(us)); }

// mode 0: slow engine (the threads wait for the DMA), 1: slow threads (the DMA runs ahead), 2: mixture, 3: yields only,
// 4: an engine that is always late (the early-wait plant)
void jitter(Rng &r, bool engine, int mode) {
    switch (mode) {
    case 0: if (engine) sleep_us(20 + r.next() % 100); break;
    case 1: if (!engine) sleep_us(20 + r.next() % 100); break;
    case 2: {
        const uint64_t x = r.next() % 3;
        if (x == 1) for (int i = 1 + (int)(r.next() % 8); i > 0; --i) std::this_thread::yield();
        if (x == 2) sleep_us(5 + r.next() % 60);
        break;
    }
    case 4: if (engine) sleep_us(400); break;
    default: if (r.next() & 1) std::this_thread::yield();
    }
}

// position-dependent content that never holds the sentinel: a table made once, read at an offset the seed chooses
const char *pattern(size_t bytes, unsigned seed) {
    static std::vector<char> table;
    const size_t shift = seed % 251;
    if (table.size() < bytes + 251) {
        table.resize(bytes + 251);
        for (size_t p = 0; p < table.size(); ++p) {
            uint64_t x = (p + 1) * 0x9E3779B97F4A7C15ULL;
            x ^= x >> 29;
            const unsigned char v = (unsigned char)(x % 255);
            table[p] = (char)(v >= kSentinel ? v + 1 : v);
        }
    }
    return table.data() + shift;
}

struct Case {
    size_t chunk;
    int nt;
    bool to_host;
    size_t bytes;
    unsigned seed;
    int fail_at;  // the operation that fails, -1: none
    Plant plant;
};

class FakeTransport {
public:
    explicit FakeTransport(const Case &c)
        : c_(c), mode_(c.plant == kEarlyWait ? 4 : (int)(c.seed % 4)), device_(c.bytes + kGuard), engine_rng_{c.seed * 2654435761ULL + 17} {
        nch_ = (long)((c.bytes + c.chunk - 1) / c.chunk);
        for (int i = 0; i < 2; ++i) {
            stage_[i].assign(c.chunk, (char)kStageFill);
            inflight_[i].store(0), engine_on_[i].store(0), holds_[i].store(-1), released_[i].store(i - 2), nslots_[i].store(0);
        }
        engine_ = std::thread([this] { run(); });
    }
    ~FakeTransport() {
        {
            std::lock_guard<std::mutex> lock(m_);
            stop_ = true;
        }
        cv_.notify_all();
        engine_.join();
    }

    std::vector<char> &device() { return device_; }
    void set_host(const char *h) { h_ = h; }
    int ops() const { return ops_; }
    int drains() const { return drains_; }  // at or after the failing operation

    // ---- the transport interface of figh::bulk_copy
    char *stage(int i) { return stage_[i].data(); }
    int device_to_stage(int i, size_t off, size_t n) { return enqueue({kD2S, i, off, n, 0}); }
    int stage_to_device(int i, size_t off, size_t n) { return enqueue({kS2D, i, off, n, 0}); }
    int record(int i) { return enqueue({kRecord, i, 0, 0, 0}); }
    int wait(int i) {
        if (int e = count_op(false)) return e;
        if (c_.plant == kEarlyWait) return 0;  // (planted: no lock, no wait -- nothing orders the engine before the caller)
        std::unique_lock<std::mutex> lock(m_);
        const long target = recorded_[i];
        cv_.wait(lock, [&] { return reached_[i] >= target; });
        return 0;
    }
    int drain() {
        if (int e = count_op(true)) return e;
        std::unique_lock<std::mutex> lock(m_);
        cv_.wait(lock, [&] { return q_.empty() && !busy_; });
        return 0;
    }
    void copy(void *dst, const void *src, size_t n) {
        thread_local bool named = false;
        thread_local Rng rng{0};
        if (!named) {
            name_thread("copy_worker");
            named = true;
            rng.s = c_.seed * 0x9E3779B97F4A7C15ULL + 1 + 2 * (uint64_t)worker_ids_.fetch_add(1, std::memory_order_relaxed);
        }
        const char *hp = static_cast<const char *>(c_.to_host ? dst : src);
        const char *sp = static_cast<const char *>(c_.to_host ? src : dst);
        int i = -1;
        for (int b = 0; b < 2; ++b)
            if (sp >= stage_[b].data() && sp + n <= stage_[b].data() + c_.chunk) i = b;
        if (i < 0 || hp < h_ || hp + n > h_ + c_.bytes || n == 0) {
            violation("slice copy outside the staging buffers or the host array (%zu bytes)", n);
            return;
        }
        const size_t hoff = (size_t)(hp - h_);
        const long k = (long)(hoff / c_.chunk);
        const size_t a = hoff - (size_t)k * c_.chunk;
        if (sp != stage_[i].data() + a) violation("chunk %ld: host offset %zu in the chunk copied at staging offset %zu", k, a, (size_t)(sp - stage_[i].data()));
        if (c_.to_host) {
            if (holds_[i].load(std::memory_order_relaxed) != k)
                violation("chunk %ld: slice read from staging buffer %d, which holds %ld (-1 nothing, -2 being written)", k, i, holds_[i].load(std::memory_order_relaxed));
        } else if (released_[i].load(std::memory_order_relaxed) != k - 2) {
            violation("chunk %ld: slice written into staging buffer %d before the engine has read chunk %ld from it", k, i, k - 2);
        }
        if (engine_on_[i].load(std::memory_order_relaxed)) violation("chunk %ld: slice copy on staging buffer %d while the engine uses it", k, i);
        inflight_[i].fetch_add(1, std::memory_order_relaxed);
        size_t ncopy = n;
        if (c_.plant == kDropByte && k == 1 && a == 0 && n > 1) ncopy = n - 1;  // (planted)
        const int slot = nslots_[i].fetch_add(1, std::memory_order_relaxed);
        if (slot < kSlots) {
            slots_[i][slot].k.store(k, std::memory_order_relaxed);
            slots_[i][slot].a.store(a, std::memory_order_relaxed);
            slots_[i][slot].b.store(a + ncopy, std::memory_order_relaxed);
        }
        jitter(rng, false, mode_);
        std::memcpy(dst, src, ncopy);
        if (engine_on_[i].load(std::memory_order_relaxed)) violation("chunk %ld: the engine took staging buffer %d during a slice copy", k, i);
        inflight_[i].fetch_sub(1, std::memory_order_relaxed);
    }

    // after a copy that returned 0: what the staging buffers still hold has been consumed as well
    void final_checks() {
        for (int i = 0; i < 2; ++i) {
            if (inflight_[i].load()) violation("slice copies in flight on staging buffer %d after the copy", i);
            if (c_.to_host && holds_[i].load() >= 0) check_tiled(i, holds_[i].load(), "at the end");
            if (!c_.to_host && nslots_[i].load()) violation("staging buffer %d was filled and never sent", i);
        }
        if (!c_.to_host)
            for (long k = 0; k < nch_; ++k)
                if (!sent_[k]) violation("chunk %ld was never sent", k);
    }

private:
    enum Kind { kD2S, kS2D, kRecord };
    struct Op {
        Kind kind;
        int i;
        size_t off, n;
        long seq;
    };
    struct Slot {
        std::atomic<long> k;
        std::atomic<size_t> a, b;
    };

    // every call of the interface but copy() comes from the thread that called bulk_copy
    int count_op(bool is_drain) {
        const int id = ops_++;
        if (failed_ && !is_drain) violation("operation %d issued after operation %d had failed", id, c_.fail_at);
        if (is_drain && (failed_ || id == c_.fail_at)) ++drains_;  // (the failing operation may be drain() itself)
        if (id == c_.fail_at) {
            failed_ = true;
            return 1000 + id;
        }
        return 0;
    }
    int enqueue(Op op) {
        if (int e = count_op(false)) return e;
        {
            std::lock_guard<std::mutex> lock(m_);
            if (op.kind == kRecord) op.seq = ++recorded_[op.i];
            q_.push_back(op);
        }
        cv_.notify_all();
        return 0;
    }
    size_t span(long k) const { return std::min(c_.chunk, c_.bytes - (size_t)k * c_.chunk); }

    // the slices recorded on buffer i are of chunk k and tile [0, span(k)) exactly
    void check_tiled(int i, long k, const char *when) {
        const int ns = nslots_[i].load(std::memory_order_relaxed);
        if (ns > kSlots) { violation("chunk %ld: %d slice copies on staging buffer %d", k, ns, i); return; }
        std::vector<std::pair<size_t, size_t>> iv;
        for (int s = 0; s < ns; ++s) {
            if (slots_[i][s].k.load(std::memory_order_relaxed) != k) { violation("chunk %ld %s: staging buffer %d has a slice of chunk %ld", k, when, i, slots_[i][s].k.load(std::memory_order_relaxed)); return; }
            iv.emplace_back(slots_[i][s].a.load(std::memory_order_relaxed), slots_[i][s].b.load(std::memory_order_relaxed));
        }
        std::sort(iv.begin(), iv.end());
        size_t at = 0;
        for (const auto &p : iv) {
            if (p.first != at) { violation("chunk %ld %s: bytes [%zu, %zu) of staging buffer %d copied %s", k, when, std::min(at, p.first), std::max(at, p.first), i, p.first > at ? "by nobody" : "twice"); return; }
            at = p.second;
        }
        if (at != span(k)) violation("chunk %ld %s: bytes [%zu, %zu) of staging buffer %d copied by nobody", k, when, at, span(k), i);
    }

    void transfer(const Op &op) {
        const long k = (long)(op.off / c_.chunk);
        if (op.off % c_.chunk || k >= nch_ || op.n != span(k)) {
            violation("transfer of %zu bytes at device offset %zu is not a chunk of the copy", op.n, op.off);
            return;  // (never touch memory on the word of a broken protocol)
        }
        const int i = (c_.plant == kMisroute && k == 2) ? op.i ^ 1 : op.i;  // (planted)
        if (inflight_[i].load(std::memory_order_relaxed)) violation("chunk %ld: the engine takes staging buffer %d with slice copies in flight", k, i);
        if (op.kind == kD2S) {
            const long prev = holds_[i].load(std::memory_order_relaxed);
            if (prev >= 0) check_tiled(i, prev, "when its buffer is written again");
            nslots_[i].store(0, std::memory_order_relaxed);
            holds_[i].store(-2, std::memory_order_relaxed);
        } else {
            check_tiled(i, k, "when the engine reads it");
            if (sent_[k]) violation("chunk %ld sent twice", k);
        }
        engine_on_[i].store(1, std::memory_order_relaxed);
        jitter(engine_rng_, true, mode_);
        if (op.kind == kD2S) std::memcpy(stage_[i].data(), device_.data() + op.off, op.n);
        else std::memcpy(device_.data() + op.off, stage_[i].data(), op.n);
        if (inflight_[i].load(std::memory_order_relaxed)) violation("chunk %ld: slice copies on staging buffer %d while the engine used it", k, i);
        engine_on_[i].store(0, std::memory_order_relaxed);
        if (op.kind == kD2S) {
            holds_[i].store(k, std::memory_order_relaxed);
        } else {
            sent_[k] = true;
            nslots_[i].store(0, std::memory_order_relaxed);
            released_[i].store(k, std::memory_order_relaxed);
        }
    }

    void run() {
        name_thread("dma_engine");
        sent_.assign((size_t)nch_, false);
        for (;;) {
            Op op;
            {
                std::unique_lock<std::mutex> lock(m_);
                cv_.wait(lock, [&] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;
                op = q_.front();
                q_.pop_front();
                busy_ = true;
            }
            if (op.kind != kRecord) transfer(op);
            {
                std::lock_guard<std::mutex> lock(m_);
                if (op.kind == kRecord) reached_[op.i] = op.seq;
                busy_ = false;
            }
            cv_.notify_all();
        }
    }

    const Case c_;
    const int mode_;
    long nch_ = 0;
    const char *h_ = nullptr;
    std::vector<char> stage_[2], device_;
    std::vector<bool> sent_;  // engine thread; read after drain()
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<Op> q_;
    bool stop_ = false, busy_ = false;
    long recorded_[2] = {0, 0}, reached_[2] = {0, 0};
    std::atomic<int> inflight_[2], engine_on_[2], nslots_[2], worker_ids_{0};
    std::atomic<long> holds_[2];     // device -> host: the chunk buffer i holds, -1 none yet, -2 being written
    std::atomic<long> released_[2];  // host -> device: the last chunk the engine has read from buffer i
    Slot slots_[2][kSlots];
    Rng engine_rng_;
    int ops_ = 0, drains_ = 0;
    bool failed_ = false;
    std::thread engine_;
};

std::string case_name(const Case &c) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s chunk=%zu nt=%d bytes=%zu (last chunk %zu) seed=%u", c.to_host ? "d2h" : "h2d", c.chunk, c.nt, c.bytes,
                  c.bytes ? c.bytes - (c.bytes - 1) / c.chunk * c.chunk : 0, c.seed);
    std::string s = buf;
    if (c.fail_at >= 0) s += " fail_at=" + std::to_string(c.fail_at);
    return s;
}

int g_runs = 0, g_failed = 0;

// One copy.  Returns the number of transport operations it issued.
int run_case(const Case &c) {
    g_violations.store(0);
    g_first.clear();
    int ops = 0;
    {
        FakeTransport tr(c);
        std::vector<char> host(c.bytes + kGuard);
        std::vector<char> &dev = tr.device();
        std::vector<char> &src = c.to_host ? dev : host, &dst = c.to_host ? host : dev;
        std::memcpy(src.data(), pattern(c.bytes, c.seed), c.bytes);
        std::memset(src.data() + c.bytes, kSentinel, kGuard);
        std::memset(dst.data(), kSentinel, dst.size());
        tr.set_host(host.data());
        const int rc = figh::bulk_copy(tr, host.data(), c.bytes, c.to_host, c.chunk, c.nt);
        ops = tr.ops();
        if (c.fail_at < 0) {
            if (rc != 0) violation("bulk_copy returned %d", rc);
            tr.final_checks();
            const bool same = std::memcmp(dst.data(), src.data(), c.bytes) == 0;
            for (size_t p = 0; p < c.bytes && !same; ++p)
                if (dst[p] != src[p]) {
                    size_t q = p;
                    while (q < c.bytes && dst[q] != src[q]) ++q;
                    violation("destination differs from the source in bytes [%zu, %zu) (0x%02x for 0x%02x)", p, q, (unsigned char)dst[p], (unsigned char)src[p]);
                    break;
                }
            for (size_t p = c.bytes; p < c.bytes + kGuard; ++p)
                if ((unsigned char)dst[p] != kSentinel) { violation("guard byte %zu behind the destination overwritten", p - c.bytes); break; }
        } else {
            if (rc != 1000 + c.fail_at) violation("bulk_copy returned %d, operation %d failed with %d", rc, c.fail_at, 1000 + c.fail_at);
            if (tr.drains() != 1) violation("%d calls of drain() at or after the failure", tr.drains());
        }
    }
    ++g_runs;
    if (g_violations.load()) {
        ++g_failed;
        std::printf("FAIL %s: %s%s\n", case_name(c).c_str(), g_first.c_str(), g_violations.load() > 1 ? " (and more)" : "");
        std::fflush(stdout);
    }
    return ops;
}

int check_slices() {
    long bad = 0;
    for (int nt = 1; nt <= 8; ++nt)
        for (size_t n = 0; n <= size_t(3) * 8 * 4096 + 8; ++n) {
            size_t at = 0;
            bool ok = true;
            for (int t = 0; t < nt; ++t) {
                size_t a, b;
                figh::bulk_slice(n, nt, t, a, b);
                ok = ok && a == at && b >= a && b <= n && (a % 4096 == 0 || a == n);  // consecutive, disjoint, page-aligned starts
                at = b;
            }
            ok = ok && at == n;
            if (!ok && bad++ < 10) std::printf("FAIL slices nt=%d n=%zu: the shares end at %zu\n", nt, n, at);
        }
    ++g_runs;
    if (bad) {
        ++g_failed;
        std::printf("FAIL slices: %ld of the (nt, n) pairs are not partitioned\n", bad);
    }
    return bad != 0;
}

constexpr size_t kPage = 4096;

void run_cases() {
    for (const size_t chunk : {size_t(16) * kPage, size_t(3) * kPage})
        for (int nt = 1; nt <= 8; ++nt) {
            const size_t sizes[] = {1, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 3 * chunk, 5 * chunk + 12345 % chunk};
            // two seeds per case, jitter modes 0 and 2 or 1 and 3 (seed % 4), the other pair for the neighbouring size and nt
            unsigned j = (unsigned)nt;
            for (const size_t bytes : sizes) {
                for (const bool to_host : {true, false})
                    for (const unsigned seed : {j % 4, (j + 2) % 4}) run_case({chunk, nt, to_host, bytes, 4 * (unsigned)nt + seed, -1, kNoPlant});
                ++j;
            }
        }
    // last chunks of nt * 4096 * m + r bytes, 0 < r < nt, m = 1, 2 behind one full chunk: the sizes at which the share
    // floor(n / nt) rounded up to a page left r bytes to nobody.  A last chunk is at most a chunk: of the issue's two chunk
    // sizes, 16 pages takes all of them but nt = 8, m = 2, which run with 32 pages; 3 pages takes nt = 2, m = 1.
    for (int nt = 2; nt <= 8; ++nt)
        for (int m = 1; m <= 2; ++m)
            for (int r = 1; r < nt; ++r) {
                const size_t last = (size_t)nt * kPage * m + r;
                for (const size_t chunk : {size_t(3) * kPage, size_t(16) * kPage, size_t(32) * kPage}) {
                    if (last > chunk || (chunk == 32 * kPage && last <= 16 * kPage)) continue;
                    for (const bool to_host : {true, false})
                        for (unsigned seed = 0; seed < 2; ++seed) run_case({chunk, nt, to_host, chunk + last, 100 + seed, -1, kNoPlant});
                }
            }
}

void run_errors() {
    const size_t chunk = 3 * kPage;
    for (const bool to_host : {true, false})
        for (const int nt : {1, 3, 8}) {
            Case c{chunk, nt, to_host, 5 * chunk, 7, -1, kNoPlant};
            const int ops = run_case(c);
            if (ops != (to_host ? 16 : 15)) {  // 5 transfers + 5 records + 5 (4: host -> device) waits + drain
                ++g_failed;
                std::printf("FAIL %s: %d transport operations\n", case_name(c).c_str(), ops);
            }
            for (c.fail_at = 0; c.fail_at < ops; ++c.fail_at)
                for (const unsigned seed : {(unsigned)c.fail_at % 4, (unsigned)(c.fail_at + 2) % 4}) c.seed = seed, run_case(c);
        }
}

int run_plant(Plant plant) {
    int total = 0;
    for (const size_t chunk : {size_t(16) * kPage, size_t(3) * kPage})
        for (const bool to_host : {true, false})
            for (unsigned seed = 0; seed < 3; ++seed) {
                const int before = g_failed;
                run_case({chunk, 4, to_host, 5 * chunk + 777, seed, -1, plant});
                std::printf("%s %s chunk=%zu seed=%u\n", g_failed > before ? "detected" : "NOT DETECTED", to_host ? "d2h" : "h2d", chunk, seed);
                ++total;
            }
    std::printf("bulk_copy_host: planted transport detected in %d of %d runs\n", g_failed, total);
    return g_failed ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "all";
    if (what == "plant-early-wait") return run_plant(kEarlyWait);
    if (what == "plant-misroute") return run_plant(kMisroute);
    if (what == "plant-drop-byte") return run_plant(kDropByte);
    if (what != "all" && what != "slices" && what != "cases" && what != "errors") {
        std::fprintf(stderr, "usage: bulk_copy_host [all | slices | cases | errors | plant-early-wait | plant-misroute | plant-drop-byte]\n");
        return 2;
    }
    if (what == "all" || what == "slices") check_slices();
    if (what == "all" || what == "cases") run_cases();
    if (what == "all" || what == "errors") run_errors();
    std::printf("bulk_copy_host: %d runs, %d failed\n", g_runs, g_failed);
    return g_failed ? 1 : 0;
}
