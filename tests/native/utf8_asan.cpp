// utf8_asan.cpp -- the host UTF-8 check (cfws_utf8_check_messages,
// cfws_index.cpp) over exact-size heap arrays, for a build with
// -fsanitize=address,undefined (make build/utf8_asan): a read outside the
// payload or the tables, or a write at or past a capacity, is a
// heap-buffer-overflow report. A stand-alone program: it links cfws_index.cpp
// alone and touches no GPU.
//
//   utf8_asan <cases.bin> <out.bin>
//
// cases.bin: u32 count; per case: u64 heap bytes of the payload, u64
// payload_bytes as passed, u32 n_msgs, u32 has_carry, then the payload, the
// message rows (32 bytes each) and carry_in (u32 each), as
// tests/test_utf8_host.py writes them. Every array is a malloc of exactly its
// size (nothing when the size is 0). Each case runs with the BAD capacity 0
// (bad == NULL), then with the exact total. out.bin, per case: u64 checked,
// u64 BAD, the result rows, the BAD list.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cfws.h"

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
    static_assert(sizeof(cfws_utf8_result_t) == 16, "cfws_utf8_result_t is 16 bytes");
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t b = 0; b < count; ++b) {
        uint64_t heap = 0, claimed = 0;
        uint32_t n = 0, has_carry = 0;
        if (fread(&heap, 8, 1, f) != 1 || fread(&claimed, 8, 1, f) != 1 || fread(&n, 4, 1, f) != 1 ||
            fread(&has_carry, 4, 1, f) != 1)
            return 2;
        uint8_t* payload = read_exact<uint8_t>(f, heap);
        cfws_message_t* msgs = read_exact<cfws_message_t>(f, n);
        uint32_t* carry = read_exact<uint32_t>(f, has_carry ? n : 0);
        cfws_utf8_result_t* first = exact<cfws_utf8_result_t>(n);
        uint64_t c0[2] = {99, 99};
        const size_t total = cfws_utf8_check_messages(payload, claimed, msgs, n, carry, first, nullptr, 0, c0);
        cfws_utf8_result_t* result = exact<cfws_utf8_result_t>(n);
        uint32_t* bad = exact<uint32_t>(total);
        uint64_t c1[2] = {99, 99};
        const size_t again = cfws_utf8_check_messages(payload, claimed, msgs, n, carry, result, bad, total, c1);
        if (again != total || c0[1] != total || c1[1] != total || c0[0] != c1[0] ||
            (n && memcmp(first, result, n * sizeof(cfws_utf8_result_t)) != 0)) {
            fprintf(stderr, "case %u: the result changes with the capacity\n", b);
            return 3;
        }
        fwrite(c1, 8, 2, o);
        if (n) fwrite(result, sizeof(cfws_utf8_result_t), n, o);
        if (total) fwrite(bad, 4, total, o);
        free(payload);
        free(msgs);
        free(carry);
        free(first);
        free(result);
        free(bad);
    }
    fclose(f);
    fclose(o);
    return 0;
}
