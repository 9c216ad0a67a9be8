// messages_asan.cpp -- the host message walk (cfws_messages_from_frames,
// cfws_index.cpp) over exact-size heap arrays, for a build with
// -fsanitize=address,undefined (make build/messages_asan): a read outside
// the tables or a write at or past a capacity is a heap-buffer-overflow
// report. A stand-alone program: it links cfws_index.cpp alone and touches
// no GPU.
//
//   messages_asan <cases.bin>
//
// cases.bin: u32 count; per case: u32 n_frames, u32 has_status, u32 n_conns
// (0xffffffff: no conn_first), then the descriptors (32 bytes each), the
// statuses (i32) and conn_first (u64), as tests/test_messages_host.py writes
// them from tests/messages_util.py's fixed cases. Each case runs with the
// message and control capacities 0, total - 1 and total, every array a
// malloc of exactly its size (nothing when the size is 0). One line per run:
//   case msg_capacity control_capacity n_messages n_control fnv1a(msgs, conn_first_msg, control)
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
    static_assert(sizeof(cfws_message_t) == 32, "cfws_message_t is 32 bytes");
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t b = 0; b < count; ++b) {
        uint32_t n = 0, has_status = 0, nc = 0;
        if (fread(&n, 4, 1, f) != 1 || fread(&has_status, 4, 1, f) != 1 || fread(&nc, 4, 1, f) != 1) return 2;
        const size_t conns = nc != 0xffffffffu ? nc : 0;
        cfws_frame_desc_t* desc = read_exact<cfws_frame_desc_t>(f, n);
        int32_t* status = read_exact<int32_t>(f, has_status ? n : 0);
        uint64_t* conn_first = read_exact<uint64_t>(f, conns);
        uint64_t total_c = 0;
        const size_t total_m =
            cfws_messages_from_frames(desc, status, n, conn_first, conns, nullptr, 0, nullptr, nullptr, 0, &total_c);
        const size_t mcaps[3] = {0, total_m ? total_m - 1 : 0, total_m};
        const size_t ccaps[3] = {0, total_c ? (size_t)total_c - 1 : 0, (size_t)total_c};
        for (int k = 0; k < 3; ++k) {
            if (k && mcaps[k] == mcaps[k - 1] && ccaps[k] == ccaps[k - 1]) continue;
            cfws_message_t* msgs = exact<cfws_message_t>(mcaps[k]);
            uint32_t* control = exact<uint32_t>(ccaps[k]);
            uint64_t* cfm = exact<uint64_t>(conns ? conns : 1);
            uint64_t got_c = 99;
            const size_t m = cfws_messages_from_frames(desc, status, n, conn_first, conns, msgs, mcaps[k], cfm, control,
                                                       ccaps[k], k == 0 ? nullptr : &got_c);
            if (m != total_m || (k && got_c != total_c)) {
                fprintf(stderr, "case %u: totals change with the capacity\n", b);
                return 3;
            }
            uint64_t h = 0xcbf29ce484222325ull;
            h = fnv(h, msgs, (m < mcaps[k] ? m : mcaps[k]) * sizeof(cfws_message_t));
            h = fnv(h, cfm, (conns ? conns : 1) * 8);
            h = fnv(h, control, (total_c < ccaps[k] ? (size_t)total_c : ccaps[k]) * 4);
            printf("%u %zu %zu %zu %llu %016llx\n", b, mcaps[k], ccaps[k], m, (unsigned long long)total_c,
                   (unsigned long long)h);
            free(msgs);
            free(control);
            free(cfm);
        }
        free(desc);
        free(status);
        free(conn_first);
    }
    fclose(f);
    return 0;
}
