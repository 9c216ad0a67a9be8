// cfws_keyrules.h -- the mask-key generator's rules, written once for the
// host form (cfws_frame.cpp: cfws_draw_mask_keys_seeded_at), the device form
// (cfws_keydev.h: the entry cfws_keys.hip and cfws_handshake.hip draw from)
// and its compile-time tables.
//
// The reference draws a key as four random() % 256 (co_ws_frame.c:84 ->
// co_random.c:32-35). With h[0..30] the 31 words of the seeded table in draw
// order (from the generator's front pointer, wrapping round), the t-th
// random() since srandom is h[t + 31] >> 1, where
//     h[t + 31] = h[t + 28] + h[t]          (mod 2^32).
// The recurrence is linear with characteristic polynomial
//     p(x) = x^31 - x^28 - 1,
// so with q = x^k mod p:   h[k + j] = sum_c q[c] h[c + j],  c = 0..30.
// A key byte is bits 1-8 of h and carries only move upward, so everything
// here is kept mod 2^9 (kKeyMask): products of two words fit 24-bit
// multiplies and a polynomial's coefficients fit 16 bits. The seeded table
// itself is glibc's (initstate_r) and is not restated.
#ifndef CFWS_KEYRULES_H
#define CFWS_KEYRULES_H

#include <hip/hip_runtime.h>

#include <stdint.h>

constexpr int kKeyDeg = 31;                    // words of state, degree of p
constexpr int kKeyTap = 28;                    // h[t + 31] = h[t + kKeyTap] + h[t]
constexpr int kKeyWindow = 2 * kKeyDeg - 1;    // words a polynomial is applied to
constexpr uint32_t kKeyMask = 0x1ffu;

// The recurrence step: h[t + 31] from h[t] and h[t + 28].
__host__ __device__ constexpr uint32_t key_next(uint32_t h_t, uint32_t h_t28) { return h_t + h_t28; }

// The key byte of one draw: (h >> 1) % 256.
__host__ __device__ constexpr uint32_t key_byte(uint32_t h) { return (h >> 1) & 0xffu; }

// One draw on a ring of 31 words, ring[i] = h[t + (i - t % 31) mod 31]; i = t % 31.
__host__ __device__ constexpr uint32_t key_draw(uint32_t (&ring)[kKeyDeg], int i)
{
    ring[i] = key_next(ring[i], ring[(i + kKeyTap) % kKeyDeg]);
    return key_byte(ring[i]);
}

// W[31..60] from W[0..30].
__host__ __device__ constexpr void key_window_extend(uint32_t (&W)[kKeyWindow])
{
#pragma unroll
    for (int t = 0; t + kKeyDeg < kKeyWindow; ++t) W[t + kKeyDeg] = key_next(W[t], W[t + kKeyTap]) & kKeyMask;
}

// out = a b mod p (out may be a or b). x^k = x^(k - 3) + x^(k - 31) for k >= 31.
__host__ __device__ constexpr void key_poly_mul(const uint32_t (&a)[kKeyDeg], const uint32_t (&b)[kKeyDeg],
                                                uint32_t (&out)[kKeyDeg])
{
    uint32_t r[kKeyWindow] = {};
    for (int i = 0; i < kKeyDeg; ++i)
        for (int j = 0; j < kKeyDeg; ++j) r[i + j] += a[i] * b[j];
    for (int k = kKeyWindow - 1; k >= kKeyDeg; --k) {
        r[k - (kKeyDeg - kKeyTap)] += r[k];
        r[k - kKeyDeg] += r[k];
    }
    for (int i = 0; i < kKeyDeg; ++i) out[i] = r[i] & kKeyMask;
}

// q = x^k mod p, by square-and-multiply from k's top bit (a multiply by x is a shift).
__host__ __device__ constexpr void key_poly_xpow(uint64_t k, uint32_t (&q)[kKeyDeg])
{
    for (int i = 0; i < kKeyDeg; ++i) q[i] = i == 0 ? 1u : 0u;
    int bit = 63;
    while (bit >= 0 && !((k >> bit) & 1u)) --bit;
    for (; bit >= 0; --bit) {
        key_poly_mul(q, q, q);
        if ((k >> bit) & 1u) {
            const uint32_t top = q[kKeyDeg - 1];
            for (int i = kKeyDeg - 1; i > 0; --i) q[i] = q[i - 1];
            q[0] = top;
            q[kKeyTap] = (q[kKeyTap] + top) & kKeyMask;
        }
    }
}

// a b for a, b below 2^24 (a coefficient and a word are below 2^9): on the
// device the full-rate 24-bit multiply-add. key_sum closes a sum of such
// products: the empty statement makes all 32 bits of it count. Without it
// the compiler, seeing that only 9 bits are used, turns the 24-bit
// multiplies back into 32-bit ones, whose operands it then cannot bound,
// and emits the quarter-rate v_mul_lo_u32.
__host__ __device__ __forceinline__ uint32_t key_mul(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return a * b;
#endif
}

__host__ __device__ __forceinline__ uint32_t key_sum(uint32_t s)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(s));
#endif
    return s & kKeyMask;
}

// out[j] = sum_c q[c] W[c + j]: with W[i] = h[t + i] and q = x^k mod p,
// out[j] = h[t + k + j]. q and W hold values below 2^9.
__host__ __device__ __forceinline__ void key_poly_apply(const uint32_t (&q)[kKeyDeg],
                                                        const uint32_t (&W)[kKeyWindow], uint32_t (&out)[kKeyDeg])
{
#pragma unroll
    for (int j = 0; j < kKeyDeg; ++j) {
        uint32_t s = 0;
#pragma unroll
        for (int c = 0; c < kKeyDeg; ++c) s += key_mul(q[c], W[c + j]);
        out[j] = key_sum(s);
    }
}

#endif
