// cfws_keydev.h -- the mask-key generator's device entry,
// written once for the kernels that draw from the stream: draw_keys_kernel
// (cfws_keys.hip: mask keys) and client_keys_kernel (cfws_handshake.hip: the
// upgrade keys, 16 draws each). The generator is sequential, but linear
// (cfws_keyrules.h): a position k draws ahead is x^k mod p applied to a
// 61-word window, so every lane enters the stream at the start of its own run.
//   host    the 31 words at first_draw (cfws_internal_key_state), by value;
//   wave g  jumps by g * kWaveDraws: one application of x^(kWaveDraws 2^j)
//           per set bit j of g, the window spread over the wave's lanes
//           (key_wave_window: every lane of the wave takes part);
//   lane l  jumps by l * kLaneDraws from the wave's window: x^(kLaneDraws l)
//           applied with the window in scalar registers (key_lane_ring: a
//           lane on its own);
//   then    kLaneDraws draws on a ring of 31 registers, every index static.
// Both tables of polynomials are built at compile time (one copy per unit
// that includes this header).
#ifndef CFWS_KEYDEV_H
#define CFWS_KEYDEV_H

#include "cfws_keyrules.h"

namespace {

constexpr uint64_t kLaneDraws = 128;                          // one lane's run: 32 mask keys, 8 upgrade keys
constexpr uint64_t kWaveDraws = 64 * kLaneDraws;              // one wave's run
constexpr int kWaveBits = 21;                                 // waves of a batch: below 2^34 draws
constexpr uint64_t kKeyMaxDraws = kWaveDraws << kWaveBits;    // a batch draws fewer than this

// A polynomial mod p over Z/2^9: 31 coefficients, padded to four 16-byte loads.
struct alignas(16) KeyPoly {
    uint16_t c[32];
};
template <int N>
struct KeyPolys {
    KeyPoly p[N];
};

constexpr void put_poly(KeyPoly& d, const uint32_t (&q)[kKeyDeg])
{
    for (int i = 0; i < kKeyDeg; ++i) d.c[i] = (uint16_t)q[i];
}

// x^(kWaveDraws 2^j), j < kWaveBits
constexpr KeyPolys<kWaveBits> wave_pows()
{
    KeyPolys<kWaveBits> T = {};
    uint32_t q[kKeyDeg] = {};
    key_poly_xpow(kWaveDraws, q);
    for (int j = 0; j < kWaveBits; ++j) {
        put_poly(T.p[j], q);
        key_poly_mul(q, q, q);
    }
    return T;
}

// x^(kLaneDraws l), l < 64
constexpr KeyPolys<64> lane_pows()
{
    KeyPolys<64> T = {};
    uint32_t q[kKeyDeg] = {}, step[kKeyDeg] = {};
    key_poly_xpow(0, q);
    key_poly_xpow(kLaneDraws, step);
    for (int l = 0; l < 64; ++l) {
        put_poly(T.p[l], q);
        key_poly_mul(q, step, q);
    }
    return T;
}

__device__ const KeyPolys<kWaveBits> kWavePow = wave_pows();
__device__ const KeyPolys<64> kLanePow = lane_pows();

struct KeyState {
    uint32_t h[kKeyDeg];
};

// key_window_extend over lanes: lane i < 31 holds W[i]; afterwards lane
// i < 61 holds W[i]. W[t + 31] needs W[t + 28], so three words per round.
__device__ __forceinline__ uint32_t wave_window_extend(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (uint32_t t = kKeyDeg; t < (uint32_t)kKeyWindow; t += kKeyDeg - kKeyTap) {
        const uint32_t a = __shfl(v, (int)((lane - kKeyDeg) & 63u), 64);
        const uint32_t b = __shfl(v, (int)((lane - (kKeyDeg - kKeyTap)) & 63u), 64);
        if (lane >= t && lane < t + (kKeyDeg - kKeyTap)) v = key_next(a, b) & kKeyMask;
    }
    return v;
}

// key_poly_apply over lanes: lane j < 31 gets sum_c q[c] W[c + j] from the
// window wave_window_extend left; q is the same for the whole wave.
__device__ __forceinline__ uint32_t wave_poly_apply(const KeyPoly& q, uint32_t v, uint32_t lane)
{
    uint32_t s = 0;
#pragma unroll
    for (int c = 0; c < kKeyDeg; ++c) s += key_mul(q.c[c], (uint32_t)__shfl(v, (int)((lane + c) & 63u), 64));
    return key_sum(s);
}

// W = the 61 words from draw g * kWaveDraws of the stream whose 31 words at
// its first draw are `base`. g is wave-uniform (below 2^kWaveBits) and all 64
// lanes of the wave call this together: it shuffles. No lane may have left.
__device__ __forceinline__ void key_wave_window(const KeyState& base, uint32_t g, uint32_t lane,
                                                uint32_t (&W)[kKeyWindow])
{
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < kKeyDeg; ++i)
        if (lane == (uint32_t)i) v = base.h[i];
    for (uint32_t j = 0; (g >> j) != 0; ++j) {
        if (!((g >> j) & 1u)) continue;
        v = wave_poly_apply(kWavePow.p[j], wave_window_extend(v, lane), lane);
    }
    v = wave_window_extend(v, lane);
#pragma unroll
    for (int i = 0; i < kKeyWindow; ++i) W[i] = (uint32_t)__builtin_amdgcn_readlane((int)v, i);
}

// ring = the 31 words at draw lane * kLaneDraws of the wave's window: the
// lane's own work, no shuffles (lanes past the batch have left by now).
__device__ __forceinline__ void key_lane_ring(const uint32_t (&W)[kKeyWindow], uint32_t lane,
                                              uint32_t (&ring)[kKeyDeg])
{
    uint32_t q[kKeyDeg];
    const uint4* qp = reinterpret_cast<const uint4*>(kLanePow.p[lane].c);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint4 w = qp[i];
        const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            q[8 * i + 2 * k] = d[k] & 0xffffu;
            if (8 * i + 2 * k + 1 < kKeyDeg) q[8 * i + 2 * k + 1] = d[k] >> 16;
        }
    }
    key_poly_apply(q, W, ring);
}

}  // namespace

#endif
