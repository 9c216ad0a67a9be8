// utf8_host_walk.cpp -- tools/utf8_bench.py's host leg: the UTF-8 check of a
// tick's messages with cfws_utf8_check_messages on `threads` threads
// (messages dealt out in contiguous ranges of about equal payload bytes, each
// thread writing its rows of `result` and a BAD list of its own; the lists
// are not stitched together, which favours the host). Native so the time is
// the walk's and not an interpreter's. Built by
// `make build/libutf8hostwalk.so`, linked to libcfws.so.
#include <chrono>
#include <cstdint>
#include <thread>
#include <vector>

#include "cfws.h"

extern "C" uint64_t utf8_host_walk(const void* payload, uint64_t payload_bytes, const cfws_message_t* msgs,
                                   uint64_t n_msgs, uint32_t threads, cfws_utf8_result_t* result, uint64_t* counts)
{
    // the ranges' ends, found before the clock starts
    std::vector<uint64_t> end(threads, n_msgs);
    uint64_t total = 0, run = 0;
    for (uint64_t m = 0; m < n_msgs; ++m) total += msgs[m].payload_size;
    for (uint64_t m = 0, t = 0; m < n_msgs && t + 1 < threads; ++m) {
        run += msgs[m].payload_size;
        while (t + 1 < threads && run >= total / threads * (t + 1)) end[t++] = m + 1;
    }
    std::vector<std::vector<uint32_t>> bad(threads);
    std::vector<uint64_t> c(2 * threads, 0);
    for (uint32_t t = 0; t < threads; ++t) bad[t].assign(end[t] - (t ? end[t - 1] : 0) + 1, 0);
    std::vector<std::thread> pool;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t t = 0; t < threads; ++t)
        pool.emplace_back([&, t] {
            const uint64_t a = t ? end[t - 1] : 0, b = end[t];
            cfws_utf8_check_messages(payload, payload_bytes, msgs + a, b - a, nullptr, result + a, bad[t].data(),
                                     bad[t].size(), &c[2 * t]);
        });
    for (auto& th : pool) th.join();
    const auto t1 = std::chrono::steady_clock::now();
    counts[0] = counts[1] = 0;
    for (uint32_t t = 0; t < threads; ++t) {
        counts[0] += c[2 * t];
        counts[1] += c[2 * t + 1];
    }
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
}
