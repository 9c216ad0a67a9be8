// cfws_handshake.hip -- the upgrade's key handling for a connection storm
// (co_ws_http_extension.c), one rule each:
//   ws_accept_kernel     Sec-WebSocket-Accept of n keys
//                        (co_ws_create_base64_accept_key, :26-57);
//   client_keys_kernel   n clients' Sec-WebSocket-Key values, drawn from the
//                        reference's random() stream (:280-290), with the
//                        accept values their answers must carry;
//   upgrade_keys_kernel  the server's decision on each key (:156-170:
//                        co_base64_decode and nonce_length == 16) with the
//                        accept value in the same pass;
//   check_accept_kernel  the client's strcmp of each answer (:247).
#include "cfws_kernels.h"
#include "cfws_keydev.h"

namespace {

// ---------------------------------------------------------------------------
// SHA-1, base64 and the accept value's message (co_sha1.c, co_base64.c)
// ---------------------------------------------------------------------------
__constant__ char kWsGuid[37] = "258EAFA5-E914-47DA-95CA-C5AB0DC85B11";
__constant__ char kB64[65] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";

// A base64 character (RFC 4648 4, co_base64.c's table). The table lookup
// measured 10 % faster than computing the character by compares.
__device__ __forceinline__ uint32_t b64_char(uint32_t x) { return (uint8_t)kB64[x]; }

// Four characters of a 24-bit group, as a little-endian word of text.
__device__ __forceinline__ uint32_t b64_group(uint32_t v)
{
    return b64_char((v >> 18) & 63) | b64_char((v >> 12) & 63) << 8 | b64_char((v >> 6) & 63) << 16 |
           b64_char(v & 63) << 24;
}

// How co_base64_decode (co_base64.c:94-167) treats a byte of its input.
//   data     A-Z a-z 0-9 + / and ! - : _ (the table's second spellings of 62
//            and 63); every byte >= 0x80 too: the table spells out 128
//            entries, the rest are zero and decode as value 0;
//   skipped  \n \r = (0x80 in the table): dropped wherever they stand, each
//            lowering the reported length by 1;
//   failing  any other byte below 0x80, NUL included: the decode returns false.
enum : uint8_t { kB64Data = 0, kB64Skipped = 1, kB64Failing = 2 };

constexpr uint8_t b64_decode_class(uint32_t b)
{
    if (b >= 0x80u) return kB64Data;
    if (b == '\n' || b == '\r' || b == '=') return kB64Skipped;
    if ((b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || (b >= '0' && b <= '9')) return kB64Data;
    if (b == '+' || b == '/' || b == '!' || b == '-' || b == ':' || b == '_') return kB64Data;
    return kB64Failing;
}

struct B64Classes {
    uint8_t c[256];
};
constexpr B64Classes b64_classes()
{
    B64Classes T = {};
    for (uint32_t b = 0; b < 256; ++b) T.c[b] = b64_decode_class(b);
    return T;
}
__constant__ const B64Classes kB64Class = b64_classes();

// The decode walk's state over a key: the bytes skipped and whether one failed.
struct DecodeWalk {
    uint32_t skipped = 0, failed = 0;
    __device__ __forceinline__ void byte(uint32_t b)
    {
        const uint32_t k = kB64Class.c[b & 0xffu];
        skipped += k == kB64Skipped ? 1u : 0u;
        failed |= k == kB64Failing ? 1u : 0u;
    }
    __device__ __forceinline__ void be_word(uint32_t w)
    {
        byte(w >> 24);
        byte(w >> 16);
        byte(w >> 8);
        byte(w);
    }
    // co_http_request_validate_ws_upgrade's decision (:159-170) on a key of L
    // bytes: the decode succeeded and nonce_length, (size_t)(L / 4.0 * 3)
    // less the skipped bytes, is 16. The length comes from L, not from the
    // bytes decoded.
    __device__ __forceinline__ bool valid(uint64_t L) const { return !failed && 3 * L / 4 == 16u + uint64_t(skipped); }
};

// Byte i of the SHA-1 input key || GUID || 0x80 || 0... || bit length (BE64)
// over `blocks` 64-byte blocks.
__device__ __forceinline__ uint32_t accept_msg_byte(const uint8_t* __restrict__ key, uint64_t L,
                                                    uint64_t blocks, uint64_t i)
{
    const uint64_t m = L + 36;
    if (i < L) return key[i];
    if (i < m) return (uint8_t)kWsGuid[i - L];
    if (i == m) return 0x80u;
    const uint64_t end = blocks * 64;
    if (i >= end - 8) return (uint32_t)((m * 8) >> (8 * (end - 1 - i))) & 0xffu;
    return 0;
}

__device__ __forceinline__ uint32_t rol32(uint32_t v, int b) { return (v << b) | (v >> (32 - b)); }

// One SHA-1 block (80 rounds over a 16-word schedule kept in registers).
// When w is a compile-time constant (the second block of a 24-byte key's
// message), the whole schedule folds into constants.
__device__ __forceinline__ void sha1_block(uint32_t (&st)[5], uint32_t (&w)[16])
{
    uint32_t a = st[0], bb = st[1], cc = st[2], d = st[3], e = st[4];
#pragma unroll
    for (int r = 0; r < 80; ++r) {
        if (r >= 16)
            w[r & 15] = rol32(w[(r + 13) & 15] ^ w[(r + 8) & 15] ^ w[(r + 2) & 15] ^ w[r & 15], 1);
        const uint32_t f = r < 20 ? ((bb & cc) | (~bb & d))
                         : r < 40 ? (bb ^ cc ^ d)
                         : r < 60 ? ((bb & cc) | (bb & d) | (cc & d)) : (bb ^ cc ^ d);
        const uint32_t k = r < 20 ? 0x5a827999u : r < 40 ? 0x6ed9eba1u : r < 60 ? 0x8f1bbcdcu : 0xca62c1d6u;
        const uint32_t t = rol32(a, 5) + f + e + k + w[r & 15];
        e = d; d = cc; cc = rol32(bb, 30); bb = a; a = t;
    }
    st[0] += a; st[1] += bb; st[2] += cc; st[3] += d; st[4] += e;
}

// The GUID's bytes as big-endian words (it follows a 24-byte key at word 6).
__device__ __forceinline__ uint32_t guid_word(int j)
{
    constexpr char g[] = "258EAFA5-E914-47DA-95CA-C5AB0DC85B11";
    return (uint32_t)(uint8_t)g[4 * j] << 24 | (uint32_t)(uint8_t)g[4 * j + 1] << 16 |
           (uint32_t)(uint8_t)g[4 * j + 2] << 8 | (uint32_t)(uint8_t)g[4 * j + 3];
}

__device__ __forceinline__ void sha1_init(uint32_t (&st)[5])
{
    st[0] = 0x67452301u; st[1] = 0xefcdab89u; st[2] = 0x98badcfeu; st[3] = 0x10325476u; st[4] = 0xc3d2e1f0u;
}

// SHA-1(key || GUID) of a 24-byte key (every RFC 6455 client key: base64 of
// 16 bytes), w[0..5] holding the key as big-endian words: 6 key words + 9
// GUID words + the 0x80 pad in block 0, and a constant block 1 (zeros and
// the 480-bit length).
__device__ __forceinline__ void accept_hash24(uint32_t (&w)[16], uint32_t (&st)[5])
{
    sha1_init(st);
#pragma unroll
    for (int t = 6; t < 15; ++t) w[t] = guid_word(t - 6);
    w[15] = 0x80000000u;
    sha1_block(st, w);
    uint32_t w2[16];
#pragma unroll
    for (int t = 0; t < 15; ++t) w2[t] = 0;
    w2[15] = 60u * 8u;
    sha1_block(st, w2);
}

// SHA-1(key || GUID) of key[0, L), with the decode walk over the key's bytes
// in the same pass when kWalk. A key of 24 bytes takes accept_hash24, read
// as three 8-byte loads where it is 8-byte aligned (keys packed 24 bytes
// apart stay aligned); any other length builds the message byte by byte.
template <bool kWalk>
__device__ __forceinline__ void accept_hash(const uint8_t* __restrict__ key, uint64_t L, uint32_t (&st)[5],
                                            DecodeWalk& walk)
{
    if (L == 24) {
        uint32_t w[16];
        if ((reinterpret_cast<uintptr_t>(key) & 7u) == 0) {
            const uint2* k8 = reinterpret_cast<const uint2*>(key);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const uint2 v = k8[t];
                w[2 * t] = __builtin_bswap32(v.x);
                w[2 * t + 1] = __builtin_bswap32(v.y);
            }
        } else {
#pragma unroll
            for (int t = 0; t < 6; ++t)
                w[t] = (uint32_t)key[4 * t] << 24 | (uint32_t)key[4 * t + 1] << 16 |
                       (uint32_t)key[4 * t + 2] << 8 | (uint32_t)key[4 * t + 3];
        }
        if (kWalk) {
#pragma unroll
            for (int t = 0; t < 6; ++t) walk.be_word(w[t]);
        }
        accept_hash24(w, st);
    } else {
        sha1_init(st);
        const uint64_t blocks = (L + 36 + 9 + 63) / 64;
        for (uint64_t b = 0; b < blocks; ++b) {
            uint32_t w[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const uint64_t i = b * 64 + 4 * t;
                w[t] = accept_msg_byte(key, L, blocks, i) << 24 | accept_msg_byte(key, L, blocks, i + 1) << 16 |
                       accept_msg_byte(key, L, blocks, i + 2) << 8 | accept_msg_byte(key, L, blocks, i + 3);
                if (kWalk) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (i + k < L) walk.byte(w[t] >> (8 * (3 - k)));
                }
            }
            sha1_block(st, w);
        }
    }
}

// base64 of the 20 hash bytes: 6 full groups + 2 bytes -> 3 chars + '='; the
// 32-byte slot as words: 28 characters, the NUL, 3 zeros
__device__ __forceinline__ void accept_words(const uint32_t (&st)[5], uint32_t (&ow)[8])
{
    ow[7] = 0u;
#pragma unroll
    for (int g = 0; g < 7; ++g) {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int idx = 3 * g + j;
            const uint32_t byte = idx < 20 ? (st[idx >> 2] >> (8 * (3 - (idx & 3)))) & 0xffu : 0u;
            v = v << 8 | byte;
        }
        const uint32_t c3 = g < 6 ? b64_char(v & 63) : (uint32_t)'=';
        ow[g] = b64_char((v >> 18) & 63) | b64_char((v >> 12) & 63) << 8 | b64_char((v >> 6) & 63) << 16 |
                c3 << 24;
    }
}

// A 32-byte slot of text from its words: two 16-byte stores where the slot is
// 16-byte aligned; otherwise its first `bytes` bytes one by one, the rest of
// the slot left alone.
__device__ __forceinline__ void store_slot(char* o, const uint32_t (&ow)[8], int bytes)
{
    if ((reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
        uint4* o16 = reinterpret_cast<uint4*>(o);
        o16[0] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        o16[1] = make_uint4(ow[4], ow[5], ow[6], ow[7]);
    } else {
        for (int b = 0; b < bytes; ++b) o[b] = (char)(ow[b >> 2] >> (8 * (b & 3)));
    }
}

// offsets out of order: no key, an empty slot (a wrapped length would walk
// ~2^58 SHA-1 blocks)
__device__ __forceinline__ void zero_slot(char* o)
{
    for (int b = 0; b < CFWS_WS_ACCEPT_SLOT; ++b) o[b] = 0;
}

// One thread per connection: a connection storm's accept keys at once.
#ifndef CFWS_ACCEPT_MIN_BLOCKS
#define CFWS_ACCEPT_MIN_BLOCKS 1
#endif
__global__ void __launch_bounds__(kThreads, CFWS_ACCEPT_MIN_BLOCKS)
ws_accept_kernel(const uint8_t* __restrict__ keys, const uint64_t* __restrict__ key_off, uint64_t n,
                 char* __restrict__ out)
{
    const uint64_t c = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (c >= n) return;
    const uint8_t* key = keys + key_off[c];
    char* o = out + CFWS_WS_ACCEPT_SLOT * c;
    if (key_off[c + 1] < key_off[c]) {
        zero_slot(o);
        return;
    }
    uint32_t st[5], ow[8];
    DecodeWalk walk;
    accept_hash<false>(key, key_off[c + 1] - key_off[c], st, walk);
    accept_words(st, ow);
    store_slot(o, ow, 29);
}

// ---------------------------------------------------------------------------
// client keys (co_http_request_create_ws_upgrade, co_ws_http_extension.c:280-290)
// ---------------------------------------------------------------------------
// A lane's run of kLaneDraws draws is kLaneConns nonces of 16 draws: the run
// draw_keys_kernel has, so the generator's tables serve both kernels.
constexpr uint32_t kNonceDraws = 16;
constexpr uint32_t kLaneConns = uint32_t(kLaneDraws / kNonceDraws);   // r: 8
constexpr uint32_t kWaveConns = 64 * kLaneConns;                     // w: 512
constexpr uint32_t kGroupConns = kWaves * kWaveConns;                // G: 2,048
constexpr uint64_t kMaxClientConns = kKeyMaxDraws / kNonceDraws;     // 2^30
static_assert(kLaneDraws % kNonceDraws == 0, "a lane's run is whole nonces");
static_assert(kNonceDraws < kKeyDeg, "a nonce's draws touch each ring word once");

// Connections [0, n) of the stream whose 31 words at its first draw are
// `base`, kGroupConns per workgroup. Connection c's nonce is draws
// [16 c, 16 c + 16); its key, co_base64_encode(nonce, padding) -- 22
// characters and "==" -- goes to ws_keys + 32 c as 24 characters, the NUL
// and 7 zeros, and its accept value (when expect is given) to expect + 32 c
// as ws_accept_kernel writes it. Both outputs 16-byte aligned; each slot is
// two 16-byte stores, and nothing outside [0, 32 n) of either is written.
// The nonce never goes to memory. Waves leave whole before the shuffles of
// key_wave_window; lanes leave individually only after them.
__global__ void __launch_bounds__(kThreads)
client_keys_kernel(KeyState base, uint64_t n, char* __restrict__ ws_keys, char* __restrict__ expect,
                   uint64_t* __restrict__ next_draw, uint64_t next_value)
{
    if (next_draw && blockIdx.x == 0 && threadIdx.x == 0) *next_draw = next_value;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    const uint64_t wave_first = uint64_t(g) * kWaveConns;
    if (wave_first >= n) return;                          // whole waves only
    uint32_t W[kKeyWindow];
    key_wave_window(base, g, lane, W);

    const uint64_t c0 = wave_first + uint64_t(lane) * kLaneConns;
    if (c0 >= n) return;
    uint32_t ring[kKeyDeg];
    key_lane_ring(W, lane, ring);
    // One nonce per turn, not unrolled (a turn is two SHA-1 blocks): the ring
    // is turned by 16 words after each, so every turn draws at indices 0..15.
#pragma unroll 1
    for (uint32_t i = 0; i < kLaneConns; ++i) {
        const uint64_t c = c0 + i;
        if (c >= n) return;
        uint32_t b[kNonceDraws];
#pragma unroll
        for (uint32_t j = 0; j < kNonceDraws; ++j) b[j] = key_draw(ring, (int)j);
        uint32_t turned[kKeyDeg];
#pragma unroll
        for (int k = 0; k < kKeyDeg; ++k) turned[k] = ring[(k + (int)kNonceDraws) % kKeyDeg];
#pragma unroll
        for (int k = 0; k < kKeyDeg; ++k) ring[k] = turned[k];

        // the key as text: five whole groups, then one byte -> 2 characters + "=="
        uint32_t kw[8];
#pragma unroll
        for (int q = 0; q < 5; ++q) kw[q] = b64_group(b[3 * q] << 16 | b[3 * q + 1] << 8 | b[3 * q + 2]);
        kw[5] = b64_char(b[15] >> 2) | b64_char((b[15] & 3u) << 4) << 8 | (uint32_t)'=' << 16 | (uint32_t)'=' << 24;
        kw[6] = 0u;
        kw[7] = 0u;
        store_slot(ws_keys + 32 * c, kw, 32);
        if (expect) {
            uint32_t w[16], st[5], ow[8];
#pragma unroll
            for (int t = 0; t < 6; ++t) w[t] = __builtin_bswap32(kw[t]);
            accept_hash24(w, st);
            accept_words(st, ow);
            store_slot(expect + CFWS_WS_ACCEPT_SLOT * c, ow, 32);
        }
    }
}

// ---------------------------------------------------------------------------
// the server's key decision and the client's check of the answer
// ---------------------------------------------------------------------------
// `flag` summed over the workgroup's threads into *count: one atomic per
// wave. Every thread of the workgroup calls it.
__device__ __forceinline__ void count_flags(bool flag, uint32_t* __restrict__ count)
{
    const uint32_t k = (uint32_t)__popcll(__ballot(flag));
    if (count && k != 0 && (threadIdx.x & 63u) == 0) atomicAdd(count, k);
}

// One thread per connection: ws_accept_kernel's hash with the decode walk in
// the same pass. valid[c] = the reference's decision; accept (optional) as
// ws_accept_kernel writes it, for every key; *invalid (optional, zeroed
// before the launch) += the keys with valid 0.
__global__ void __launch_bounds__(kThreads, CFWS_ACCEPT_MIN_BLOCKS)
upgrade_keys_kernel(const uint8_t* __restrict__ keys, const uint64_t* __restrict__ key_off, uint64_t n,
                    uint8_t* __restrict__ valid, char* __restrict__ accept, uint32_t* __restrict__ invalid)
{
    const uint64_t c = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    bool bad = false;
    if (c < n) {
        const uint64_t lo = key_off[c], hi = key_off[c + 1];
        char* o = accept ? accept + CFWS_WS_ACCEPT_SLOT * c : nullptr;
        if (hi < lo) {
            bad = true;
            if (o) zero_slot(o);
        } else {
            uint32_t st[5];
            DecodeWalk walk;
            accept_hash<true>(keys + lo, hi - lo, st, walk);
            bad = !walk.valid(hi - lo);
            if (o) {
                uint32_t ow[8];
                accept_words(st, ow);
                store_slot(o, ow, 29);
            }
        }
        valid[c] = bad ? 0u : 1u;
    }
    count_flags(bad, invalid);
}

// One thread per connection: strcmp(answer, expected) == 0 (:247), the
// expected value a string in its 32-byte slot, the answer ending at its first
// NUL or at its end. ok[c]; *fail (optional, zeroed before the launch) += the
// answers that differ.
__global__ void __launch_bounds__(kThreads)
check_accept_kernel(const char* __restrict__ expect, const uint8_t* __restrict__ resp,
                    const uint64_t* __restrict__ resp_off, uint64_t n, uint8_t* __restrict__ ok,
                    uint32_t* __restrict__ fail)
{
    const uint64_t c = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    bool differs = false;
    if (c < n) {
        const uint64_t lo = resp_off[c], hi = resp_off[c + 1];
        differs = hi < lo;
        if (!differs) {
            const uint8_t* e = reinterpret_cast<const uint8_t*>(expect) + CFWS_WS_ACCEPT_SLOT * c;
            const uint8_t* a = resp + lo;
            const uint64_t L = hi - lo;
            for (uint32_t i = 0; i <= CFWS_WS_ACCEPT_SLOT; ++i) {
                const uint32_t eb = i < CFWS_WS_ACCEPT_SLOT ? e[i] : 0u;   // a slot holds at most 32 characters
                const uint32_t ab = i < L ? a[i] : 0u;
                if (eb != ab) differs = true;
                if (eb != ab || eb == 0) break;
            }
        }
        ok[c] = differs ? 0u : 1u;
    }
    count_flags(differs, fail);
}

int zero_count(uint32_t* d_count, hipStream_t st)
{
    if (!d_count) return CFWS_OK;
    const hipError_t e = hipMemsetAsync(d_count, 0, sizeof(uint32_t), st);
    return e == hipSuccess ? CFWS_OK : set_err(CFWS_ERROR_HIP, "hipMemsetAsync", e);
}

}  // namespace

extern "C" {

int cfws_ws_accept_keys_batch(const void* d_keys, const uint64_t* d_key_off, size_t n,
                              char* d_accept, void* stream)
{
    const CfwsPassScope pass_scope;
    if (int rc = check_init()) return rc;
    if (n == 0) return CFWS_OK;
    if (!d_keys || !d_key_off || !d_accept)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "accept keys: null pointer", hipSuccess);
    ws_accept_kernel<<<grid_for(n, kThreads), kThreads, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const uint8_t*>(d_keys), d_key_off, n, d_accept);
    return launch_check("ws_accept_keys");
}

size_t cfws_ws_client_keys_group_conns(void) { return kGroupConns; }

int cfws_ws_client_keys_batch(uint32_t seed, uint64_t first_draw, size_t n_conns, char* d_ws_keys,
                              char* d_expect_accept, uint64_t* d_next_draw, void* stream)
{
    const CfwsPassScope pass_scope;                       // not a timed pass: a pending pair is dropped
    if (int rc = check_init()) return rc;
    if (first_draw > kCfwsKeyMaxFirstDraw)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "first_draw above 2^62", hipSuccess);
    if (uint64_t(n_conns) >= kMaxClientConns)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "2^30 connections or more", hipSuccess);
    if (n_conns != 0 && !d_ws_keys) return set_err(CFWS_ERROR_INVALID_ARGUMENT, "null pointer", hipSuccess);
    if (n_conns != 0 && misaligned(d_ws_keys, d_expect_accept))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "client keys: outputs must be 16-byte aligned", hipSuccess);
    KeyState base;
    if (cfws_internal_key_state(seed, first_draw, base.h))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "seed", hipSuccess);
    if (n_conns == 0 && !d_next_draw) return CFWS_OK;
    client_keys_kernel<<<grid_for(n_conns, kGroupConns), kThreads, 0, static_cast<hipStream_t>(stream)>>>(
        base, n_conns, d_ws_keys, d_expect_accept, d_next_draw, first_draw + kNonceDraws * uint64_t(n_conns));
    return launch_check("ws_client_keys");
}

int cfws_ws_upgrade_keys_batch(const void* d_keys, const uint64_t* d_key_off, size_t n, uint8_t* d_valid,
                               char* d_accept, uint32_t* d_invalid_count, void* stream)
{
    const CfwsPassScope pass_scope;
    if (int rc = check_init()) return rc;
    if (n != 0 && (!d_keys || !d_key_off || !d_valid))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "upgrade keys: null pointer", hipSuccess);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = zero_count(d_invalid_count, st)) return rc;
    if (n == 0) return CFWS_OK;
    upgrade_keys_kernel<<<grid_for(n, kThreads), kThreads, 0, st>>>(static_cast<const uint8_t*>(d_keys), d_key_off, n,
                                                                    d_valid, d_accept, d_invalid_count);
    return launch_check("ws_upgrade_keys");
}

int cfws_ws_check_accept_batch(const char* d_expect_accept, const void* d_resp, const uint64_t* d_resp_off,
                               size_t n, uint8_t* d_ok, uint32_t* d_fail_count, void* stream)
{
    const CfwsPassScope pass_scope;
    if (int rc = check_init()) return rc;
    if (n != 0 && (!d_expect_accept || !d_resp || !d_resp_off || !d_ok))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "check accept: null pointer", hipSuccess);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = zero_count(d_fail_count, st)) return rc;
    if (n == 0) return CFWS_OK;
    check_accept_kernel<<<grid_for(n, kThreads), kThreads, 0, st>>>(
        d_expect_accept, static_cast<const uint8_t*>(d_resp), d_resp_off, n, d_ok, d_fail_count);
    return launch_check("ws_check_accept");
}

}  // extern "C"
