// h2_streams_host_walk.cpp -- tools/h2_streams_bench.py's host leg: the
// stream grouping of a tick's records with cfws_h2_streams_from_frames, one
// call per connection, on `threads` threads (connections dealt out in
// contiguous ranges, each thread writing into buffers of its own; the
// per-thread tables are not stitched together, which favours the host).
// Native so the time is the call's and not an interpreter's. Built by
// `make build/libh2streamshostwalk.so`, linked to libcfws.so.
#include <chrono>
#include <cstdint>
#include <thread>
#include <vector>

#include "cfws.h"

extern "C" uint64_t h2_streams_host_walk(const uint64_t* starts, const cfws_h2_frame_info_t* info, uint64_t n_frames,
                                         const uint64_t* conn_first, uint64_t conns, uint32_t threads,
                                         uint64_t* messages)
{
    std::vector<uint64_t> found(threads, 0);
    std::vector<std::vector<uint64_t>> order(threads);
    std::vector<std::vector<cfws_h2_stream_msg_t>> msgs(threads);
    auto first = [&](uint64_t c) { return c < conns ? conn_first[c] : n_frames; };
    for (uint32_t t = 0; t < threads; ++t) {              // allocated (and touched) before the clock starts
        const uint64_t f0 = first(conns * t / threads), f1 = first(conns * (t + 1) / threads);
        order[t].assign(f1 - f0 + 1, 0);
        msgs[t].assign(f1 - f0 + 1, cfws_h2_stream_msg_t{});
    }
    std::vector<std::thread> pool;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t t = 0; t < threads; ++t)
        pool.emplace_back([&, t] {
            uint64_t m = 0, at = 0;
            for (uint64_t c = conns * t / threads; c < conns * (t + 1) / threads; ++c) {
                const uint64_t a = first(c), b = first(c + 1);
                uint64_t counts[5];
                cfws_h2_streams_from_frames(starts + a, info + a, b - a, nullptr, 0, order[t].data() + at, nullptr,
                                            msgs[t].data() + at, nullptr, nullptr, counts);
                m += counts[0];
                at += b - a;
            }
            found[t] = m;
        });
    for (auto& th : pool) th.join();
    const auto t1 = std::chrono::steady_clock::now();
    *messages = 0;
    for (uint64_t k : found) *messages += k;
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
}
