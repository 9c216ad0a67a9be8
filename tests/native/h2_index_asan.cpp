// h2_index_asan.cpp -- the host HTTP/2 walk (cfws_h2_index_frames,
// cfws_index.cpp) over exact-size heap buffers, for a build with
// -fsanitize=address,undefined (make build/h2_index_asan): a read one byte
// outside [0, end) is a heap-buffer-overflow report. A stand-alone program:
// it links cfws_index.cpp alone and touches no GPU.
//
//   h2_index_asan <blobs.bin>
//
// blobs.bin: u32 count; per blob: u32 max_frame, u32 begin, u64 size, bytes
// (tests/test_h2_index.py writes it from tests/golden/h2_index_cases.json).
// Every blob is walked cut at each length 0..24 and whole, each cut copied
// into a malloc of exactly that many bytes, with select ALL / DATA / DATA +
// stream 1, once in one call and once resumed through a 2-entry `starts`
// (both must agree). One line per walk:
//   blob cut select stream_id k consumed stop fnv1a(starts, info)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cfws.h"

static uint64_t fnv(uint64_t h, const void* p, size_t n)
{
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

struct Walk {
    std::vector<uint64_t> starts;
    std::vector<cfws_h2_frame_info_t> info;
    uint64_t consumed;
    int32_t stop;
};

static Walk walk(const uint8_t* buf, uint64_t begin, uint64_t end, uint32_t mf, uint32_t sel, uint32_t sid,
                 size_t step)
{
    Walk w;
    uint64_t pos = begin;
    for (;;) {
        std::vector<uint64_t> s(step ? step : 1);
        std::vector<cfws_h2_frame_info_t> f(step ? step : 1);
        int32_t stop = 99;
        const size_t k = cfws_h2_index_frames(buf, pos, end, mf, sel, sid, s.data(), f.data(), step, &pos, &stop);
        w.starts.insert(w.starts.end(), s.begin(), s.begin() + k);
        w.info.insert(w.info.end(), f.begin(), f.begin() + k);
        w.stop = stop;
        if (stop != CFWS_INDEX_FULL) break;
        if (k != step) { fprintf(stderr, "INDEX_FULL with %zu of %zu starts\n", k, step); exit(2); }
    }
    w.consumed = pos;
    return w;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t b = 0; b < count; ++b) {
        uint32_t mf = 0, begin = 0;
        uint64_t size = 0;
        if (fread(&mf, 4, 1, f) != 1 || fread(&begin, 4, 1, f) != 1 || fread(&size, 8, 1, f) != 1) return 2;
        std::vector<uint8_t> blob(size);
        if (size && fread(blob.data(), 1, size, f) != size) return 2;
        for (uint64_t c = 0; c <= 25; ++c) {
            const uint64_t cut = c == 25 ? size : c;
            if (cut > size || (c < 25 && cut == size)) continue;
            uint8_t* exact = static_cast<uint8_t*>(malloc(cut ? cut : 1));
            if (cut) memcpy(exact, blob.data(), cut);
            const uint64_t bg = begin < cut ? begin : cut;
            const uint32_t sel[3][2] = {{CFWS_H2_INDEX_ALL, 0}, {CFWS_H2_INDEX_DATA, 0}, {CFWS_H2_INDEX_DATA, 1}};
            for (const auto& s : sel) {
                // cut == 0: the 1-byte allocation must not be read either, so pass its end
                const uint8_t* base = cut ? exact : exact + 1;
                const Walk one = walk(base, bg, cut, mf, s[0], s[1], (size_t)(cut / 9 + 1));
                const Walk res = walk(base, bg, cut, mf, s[0], s[1], 2);
                if (one.starts != res.starts || one.consumed != res.consumed || one.stop != res.stop ||
                    (one.info.size() &&
                     memcmp(one.info.data(), res.info.data(), one.info.size() * sizeof(cfws_h2_frame_info_t)))) {
                    fprintf(stderr, "resumed walk differs: blob %u cut %llu\n", b, (unsigned long long)cut);
                    return 3;
                }
                uint64_t h = 0xcbf29ce484222325ull;
                h = fnv(h, one.starts.data(), one.starts.size() * 8);
                h = fnv(h, one.info.data(), one.info.size() * sizeof(cfws_h2_frame_info_t));
                printf("%u %llu %u %u %zu %llu %d %016llx\n", b, (unsigned long long)cut, s[0], s[1],
                       one.starts.size(), (unsigned long long)one.consumed, one.stop, (unsigned long long)h);
            }
            free(exact);
        }
    }
    fclose(f);
    return 0;
}
