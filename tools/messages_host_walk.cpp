// messages_host_walk.cpp -- tools/messages_bench.py's host leg: the message
// tables of a tick's frames with cfws_messages_from_frames, one call per
// connection, on `threads` threads (connections dealt out in contiguous
// ranges, each thread writing records and control indices into buffers of
// its own; the per-thread tables are not stitched together, which favours
// the host). Native so the time is the walk's and not an interpreter's.
// Built by `make build/libmsghostwalk.so`, linked to libcfws.so.
#include <chrono>
#include <cstdint>
#include <thread>
#include <vector>

#include "cfws.h"

extern "C" uint64_t messages_host_walk(const cfws_frame_desc_t* desc, const int32_t* status, uint64_t n_frames,
                                       const uint64_t* conn_first, uint64_t conns, uint32_t threads,
                                       uint64_t* messages)
{
    std::vector<uint64_t> found(threads, 0);
    std::vector<std::vector<cfws_message_t>> msgs(threads);
    std::vector<std::vector<uint32_t>> control(threads);
    auto first = [&](uint64_t c) { return c < conns ? conn_first[c] : n_frames; };
    for (uint32_t t = 0; t < threads; ++t) {              // allocated (and touched) before the clock starts
        const uint64_t f0 = first(conns * t / threads), f1 = first(conns * (t + 1) / threads);
        msgs[t].assign(f1 - f0 + 1, cfws_message_t{});
        control[t].assign(f1 - f0 + 1, 0);
    }
    std::vector<std::thread> pool;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t t = 0; t < threads; ++t)
        pool.emplace_back([&, t] {
            uint64_t m = 0, c_at = 0;
            for (uint64_t c = conns * t / threads; c < conns * (t + 1) / threads; ++c) {
                const uint64_t a = first(c), b = first(c + 1);
                uint64_t nc = 0;
                m += cfws_messages_from_frames(desc + a, status ? status + a : nullptr, b - a, nullptr, 0,
                                               msgs[t].data() + m, msgs[t].size() - m, nullptr,
                                               control[t].data() + c_at, control[t].size() - c_at, &nc);
                c_at += nc;
            }
            found[t] = m;
        });
    for (auto& th : pool) th.join();
    const auto t1 = std::chrono::steady_clock::now();
    *messages = 0;
    for (uint64_t k : found) *messages += k;
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
}
