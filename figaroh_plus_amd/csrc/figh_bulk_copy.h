// The chunk protocol of the staged host <-> device copies (figh_memcpy_h2d / figh_memcpy_d2h on pageable memory of 24 MB
// and more: figh_api.hip) without a device: chunks go through two staging buffers, the DMA of chunk k + 1 beside the
// host-side copy of chunk k, which `nt` threads share.  Plain C++17 with threads; what touches the device is a transport
// object, so tools/bulk_copy_host.cpp drives the same code with a fake transport (one engine thread as the stream, a host
// array as device memory, seeded jitter) and tests/test_bulk_copy_host.py runs that program plainly and under
// ThreadSanitizer.
//
// A transport T supplies (every int is an error code of the transport's own, 0 = success):
//   char *stage(int i)                                  staging buffer i = 0, 1, each of at least `chunk` bytes
//   int   device_to_stage(int i, size_t off, size_t n)  enqueue device[off, off + n) -> stage(i)[0, n)
//   int   stage_to_device(int i, size_t off, size_t n)  enqueue stage(i)[0, n) -> device[off, off + n)
//   int   record(int i)                                 record event i behind what has been enqueued
//   int   wait(int i)                                   block until the last record of event i has been reached
//   int   drain()                                       block until everything enqueued has run
//   void  copy(void *dst, const void *src, size_t n)    the host-side copy of one slice (std::memcpy), from any thread
// Enqueued operations run in order, as on one stream.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <memory>
#include <thread>
#include <vector>

namespace figh {

constexpr int kBulkNotStarted = -1;  // bulk_copy: the copy threads could not be started -- nothing was copied

// chunk k of a copy of `bytes` bytes in chunks of `chunk`: [lo, lo + n)
inline void bulk_span(long k, size_t bytes, size_t chunk, size_t &lo, size_t &n) {
    lo = (size_t)k * chunk;
    n = std::min(chunk, bytes - lo);
}

// Thread t's share [a, b) of a chunk of n bytes among nt threads: the shares are consecutive and cover [0, n) for every n
// (the share is ceil(n / nt) rounded up to a page, so nt shares reach n; all but the last non-empty one are whole pages).
// The rule before -- floor(n / nt) rounded up -- left the last n mod nt bytes to nobody whenever floor(n / nt) was a multiple
// of 4096 (tests/test_bulk_copy_host.py, profiles/bulk_copy_host_old_slice_rule.txt).
inline void bulk_slice(size_t n, int nt, int t, size_t &a, size_t &b) {
    const size_t per = (((n + (size_t)nt - 1) / (size_t)nt) + 4095) & ~size_t(4095);
    a = std::min(n, per * (size_t)t);
    b = std::min(n, a + per);
}

// host h[0, bytes) <-> device[0, bytes) in staged chunks; to_host: device -> host, else host -> device.  Returns the first
// error of the transport (after it only drain() is called), 0, or kBulkNotStarted.  All threads are joined on return.
template <class T>
int bulk_copy(T &tr, char *h, const size_t bytes, const bool to_host, const size_t chunk, const int nt) {
    const long nch = (long)((bytes + chunk - 1) / chunk);
    std::atomic<long> go{to_host ? 0 : 2};  // to_host: chunks < go sit in staging; else: chunks < go may be filled
    std::unique_ptr<std::atomic<int>[]> done(new std::atomic<int>[nch]);  // per chunk: threads that have copied their slice
    for (long k = 0; k < nch; ++k) done[k].store(0, std::memory_order_relaxed);
    std::atomic<bool> abort{false};
    auto worker = [&](int t) {
        for (long k = 0; k < nch; ++k) {
            while (go.load(std::memory_order_acquire) <= k) {
                if (abort.load(std::memory_order_relaxed)) return;
                std::this_thread::yield();
            }
            size_t lo, n, a, b;
            bulk_span(k, bytes, chunk, lo, n);
            bulk_slice(n, nt, t, a, b);
            if (b > a) {
                if (to_host) tr.copy(h + lo + a, tr.stage(k & 1) + a, b - a);
                else tr.copy(tr.stage(k & 1) + a, h + lo + a, b - a);
            }
            done[k].fetch_add(1, std::memory_order_release);
        }
    };
    std::vector<std::thread> pool;
    try {
        for (int t = 0; t < nt; ++t) pool.emplace_back(worker, t);
    } catch (...) {  // (thread limit of the container: the caller takes the one-piece copy instead)
        abort.store(true);
        for (auto &t : pool) t.join();
        return kBulkNotStarted;
    }
    // (per CHUNK: a global count of thread-chunks would let a fast thread's next chunk stand in for a slow thread's current one)
    auto wait_chunk = [&](long k) { while (done[k].load(std::memory_order_acquire) < nt) std::this_thread::yield(); };
    int err = 0;
    auto fail = [&](int e) { if (e != 0 && err == 0) { err = e; abort.store(true); } return e != 0; };
    size_t lo, n;
    if (to_host) {
        bulk_span(0, bytes, chunk, lo, n);
        if (!fail(tr.device_to_stage(0, 0, n))) fail(tr.record(0));
        for (long k = 0; k < nch && err == 0; ++k) {
            if (k + 1 < nch) {
                if (k >= 1) wait_chunk(k - 1);  // chunk k - 1 has left the buffer chunk k + 1 lands in
                bulk_span(k + 1, bytes, chunk, lo, n);
                if (fail(tr.device_to_stage((int)((k + 1) & 1), lo, n))) break;
                if (fail(tr.record((int)((k + 1) & 1)))) break;
            }
            if (fail(tr.wait((int)(k & 1)))) break;
            go.store(k + 1, std::memory_order_release);
        }
    } else {
        for (long k = 0; k < nch && err == 0; ++k) {
            wait_chunk(k);  // chunk k is in its staging buffer
            bulk_span(k, bytes, chunk, lo, n);
            if (fail(tr.stage_to_device((int)(k & 1), lo, n))) break;
            if (fail(tr.record((int)(k & 1)))) break;
            if (k >= 1) {
                if (fail(tr.wait((int)((k - 1) & 1)))) break;  // chunk k - 1 has left its buffer: chunk k + 1 may be filled
                go.store(k + 2, std::memory_order_release);
            }
        }
    }
    if (err != 0) abort.store(true);
    for (auto &t : pool) t.join();
    const int e2 = tr.drain();
    return err != 0 ? err : e2;
}

}  // namespace figh
