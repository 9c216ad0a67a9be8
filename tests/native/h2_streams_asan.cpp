// h2_streams_asan.cpp -- the host stream grouping
// (cfws_h2_streams_from_frames, cfws_index.cpp) over exact-size heap arrays,
// for a build with -fsanitize=address,undefined (make build/h2_streams_asan):
// a read outside the records or a write past a count is a
// heap-buffer-overflow report. A stand-alone program: it links cfws_index.cpp
// alone and touches no GPU.
//
//   h2_streams_asan <cases.bin>
//
// cases.bin: u32 count; per case: u32 n_frames, u32 n_conns (0xffffffff: no
// conn_first), then starts (u64), the records (16 bytes each) and conn_first
// (u64), as tests/test_h2_streams.py writes them. Each case runs once with
// every output NULL but the counts, then with every output a malloc of
// exactly what the counts say (nothing when that is 0). One line per case:
//   case counts[0..4] fnv1a(order, order_frame, msgs, conn_first_msg, stream_first)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cfws.h"

static uint64_t fnv(uint64_t h, const void* p, size_t n)
{
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

template <typename T>
static T* exact(size_t count)
{
    return count ? static_cast<T*>(malloc(count * sizeof(T))) : nullptr;
}

template <typename T>
static T* read_exact(FILE* f, size_t count)
{
    T* p = exact<T>(count);
    if (count && fread(p, sizeof(T), count, f) != count) exit(2);
    return p;
}

int main(int argc, char** argv)
{
    static_assert(sizeof(cfws_h2_stream_msg_t) == 32, "cfws_h2_stream_msg_t is 32 bytes");
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t b = 0; b < count; ++b) {
        uint32_t n = 0, nc = 0;
        if (fread(&n, 4, 1, f) != 1 || fread(&nc, 4, 1, f) != 1) return 2;
        const bool has_cf = nc != 0xffffffffu;
        const size_t conns = has_cf ? nc : 0;
        uint64_t* starts = read_exact<uint64_t>(f, n);
        cfws_h2_frame_info_t* info = read_exact<cfws_h2_frame_info_t>(f, n);
        uint64_t* conn_first = read_exact<uint64_t>(f, conns);
        // conn_first of no entries is still "given": a non-null pointer to nothing
        uint64_t* cf = has_cf ? (conns ? conn_first : reinterpret_cast<uint64_t*>(sizeof(uint64_t))) : nullptr;
        uint64_t want[5] = {9, 9, 9, 9, 9};
        const size_t m0 = cfws_h2_streams_from_frames(starts, info, n, cf, conns, nullptr, nullptr, nullptr, nullptr,
                                                      nullptr, want);
        const size_t frames = (size_t)(want[1] + want[3]), rows = (size_t)(want[0] + want[2]);
        uint64_t* order = exact<uint64_t>(frames);
        uint32_t* order_frame = exact<uint32_t>(frames);
        cfws_h2_stream_msg_t* msgs = exact<cfws_h2_stream_msg_t>(rows);
        const size_t n_cfm = has_cf ? conns : 1;
        uint64_t* cfm = exact<uint64_t>(n_cfm);
        uint64_t* sf = exact<uint64_t>((size_t)want[4]);
        uint64_t got[5] = {9, 9, 9, 9, 9};
        const size_t m = cfws_h2_streams_from_frames(starts, info, n, cf, conns, order, order_frame, msgs, cfm, sf,
                                                     got);
        if (m != m0 || m != got[0] || memcmp(want, got, sizeof got) != 0) {
            fprintf(stderr, "case %u: the counts change with the outputs\n", b);
            return 3;
        }
        uint64_t h = 0xcbf29ce484222325ull;
        h = fnv(h, order, frames * 8);
        h = fnv(h, order_frame, frames * 4);
        h = fnv(h, msgs, rows * sizeof(cfws_h2_stream_msg_t));
        h = fnv(h, cfm, n_cfm * 8);
        h = fnv(h, sf, (size_t)want[4] * 8);
        printf("%u %llu %llu %llu %llu %llu %016llx\n", b, (unsigned long long)got[0], (unsigned long long)got[1],
               (unsigned long long)got[2], (unsigned long long)got[3], (unsigned long long)got[4],
               (unsigned long long)h);
        free(order);
        free(order_frame);
        free(msgs);
        free(cfm);
        free(sf);
        free(starts);
        free(info);
        free(conn_first);
    }
    fclose(f);
    return 0;
}
