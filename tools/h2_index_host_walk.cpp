// h2_index_host_walk.cpp -- tools/h2_index_bench.py's host leg: a tick of
// equal-size connection buffers walked with cfws_h2_index_frames, one call
// per connection, on `threads` threads (connections dealt out in contiguous
// ranges). Native so the time is the walk's and not an interpreter's.
// Built by `make build/libh2hostwalk.so`, linked to libcfws.so.
#include <chrono>
#include <cstdint>
#include <thread>
#include <vector>

#include "cfws.h"

extern "C" uint64_t h2_host_walk(const void* buf, uint64_t conns, uint64_t conn_bytes, uint32_t select,
                                 uint32_t threads, uint64_t* frames)
{
    std::vector<uint64_t> found(threads, 0);
    std::vector<std::thread> pool;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t t = 0; t < threads; ++t)
        pool.emplace_back([&, t] {
            std::vector<uint64_t> starts(conn_bytes / 9 + 1);
            std::vector<cfws_h2_frame_info_t> info(starts.size());
            uint64_t k = 0, consumed = 0;
            int32_t stop = 0;
            for (uint64_t c = conns * t / threads; c < conns * (t + 1) / threads; ++c)
                k += cfws_h2_index_frames(buf, c * conn_bytes, (c + 1) * conn_bytes, 0, select, 0, starts.data(),
                                          info.data(), starts.size(), &consumed, &stop);
            found[t] = k;
        });
    for (auto& th : pool) th.join();
    const auto t1 = std::chrono::steady_clock::now();
    *frames = 0;
    for (uint64_t k : found) *frames += k;
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
}
