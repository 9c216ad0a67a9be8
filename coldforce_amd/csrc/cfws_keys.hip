// cfws_keys.hip -- cfws_draw_mask_keys_device: the keys
// cfws_draw_mask_keys_seeded_at gives, drawn on the device. The generator is
// sequential, but linear (cfws_keyrules.h): a position k draws ahead is
// x^k mod p applied to a 61-word window, so every lane enters the stream at
// the start of its own run.
//   host    the 31 words at first_draw (cfws_internal_key_state), by value;
//   wave g  jumps by g * kWaveDraws: one application of x^(kWaveDraws 2^j)
//           per set bit j of g, the window spread over the wave's lanes;
//   lane l  jumps by l * kLaneDraws from the wave's window: x^(kLaneDraws l)
//           applied with the window in scalar registers;
//   then    kLaneDraws draws on a ring of 31 registers, every index static,
//           stored as kLaneFrames / 4 chunks of 16 bytes: one 128-byte line.
// Both tables of polynomials are built at compile time. With mask flags the
// draw goes packed into the workspace (n keys: an upper bound) and a second
// pass ranks the masked frames and writes keys[i] = flag ? packed[rank] : 0.
#include "cfws_kernels.h"
#include "cfws_keyrules.h"

namespace {

constexpr uint32_t kLaneFrames = 32;                          // r: one lane's run
constexpr uint32_t kWaveFrames = 64 * kLaneFrames;            // w: one wave's run
constexpr uint32_t kGroupFrames = kWaves * kWaveFrames;       // G: one workgroup's
constexpr uint64_t kLaneDraws = 4 * uint64_t(kLaneFrames);
constexpr uint64_t kWaveDraws = 4 * uint64_t(kWaveFrames);
constexpr int kWaveBits = 21;                                 // waves of a batch: n < 2^32 frames
static_assert((uint64_t(1) << 32) / kWaveFrames <= (uint64_t(1) << kWaveBits), "wave index bits");
static_assert(kLaneFrames % 4 == 0, "a lane's run is whole 16-byte chunks");

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

// Keys [0, n) of the stream whose 31 words at its first draw are `base`,
// kGroupFrames per workgroup. keys: 16-byte aligned, written in [0, 4 n).
// next_draw (optional) gets next_value.
__global__ void __launch_bounds__(kThreads)
draw_keys_kernel(KeyState base, uint64_t n, uint32_t* __restrict__ keys, uint64_t* __restrict__ next_draw,
                 uint64_t next_value)
{
    if (next_draw && blockIdx.x == 0 && threadIdx.x == 0) *next_draw = next_value;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    const uint64_t wave_first = uint64_t(g) * kWaveFrames;
    if (wave_first >= n) return;                          // whole waves only: the shuffles below need all lanes
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < kKeyDeg; ++i)
        if (lane == (uint32_t)i) v = base.h[i];
    for (uint32_t j = 0; (g >> j) != 0; ++j) {
        if (!((g >> j) & 1u)) continue;
        v = wave_poly_apply(kWavePow.p[j], wave_window_extend(v, lane), lane);
    }
    v = wave_window_extend(v, lane);
    uint32_t W[kKeyWindow];
#pragma unroll
    for (int i = 0; i < kKeyWindow; ++i) W[i] = (uint32_t)__builtin_amdgcn_readlane((int)v, i);

    const uint64_t k0 = wave_first + uint64_t(lane) * kLaneFrames;
    if (k0 >= n) return;
    uint32_t q[kKeyDeg], ring[kKeyDeg];
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
#pragma unroll
    for (uint32_t c = 0; c < kLaneFrames / 4; ++c) {
        const uint64_t kf = k0 + 4 * c;
        if (kf >= n) return;
        uint32_t k[4];
#pragma unroll
        for (uint32_t f = 0; f < 4; ++f) {
            k[f] = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) k[f] |= key_draw(ring, (int)((16 * c + 4 * f + j) % kKeyDeg)) << (8 * j);
        }
        if (kf + 4 <= n) {
            *reinterpret_cast<uint4*>(keys + kf) = make_uint4(k[0], k[1], k[2], k[3]);
        } else {                                          // the batch's tail chunk
#pragma unroll
            for (uint32_t f = 0; f < 4; ++f)
                if (kf + f < n) keys[kf + f] = k[f];
        }
    }
}

// ---- with mask flags: rank the masked frames, 16 flags per thread ----------
constexpr uint32_t kFlagItems = 16;
constexpr uint64_t kFlagBlock = uint64_t(kThreads) * kFlagItems;

// This thread's 16 flags as set bits (frames at or past n: clear); the load
// stays below round16(n).
__device__ __forceinline__ uint32_t flag_bits(const uint8_t* __restrict__ flags, uint64_t i0, uint64_t n)
{
    if (i0 >= n) return 0;
    const uint4 w = ld16u(flags + i0);
    const uint32_t d[4] = {w.x, w.y, w.z, w.w};
    uint32_t m = 0;
#pragma unroll
    for (uint32_t k = 0; k < kFlagItems; ++k)
        if (i0 + k < n && ((d[k / 4] >> (8 * (k % 4))) & 0xffu)) m |= 1u << k;
    return m;
}

__global__ void __launch_bounds__(kThreads)
keys_count_kernel(const uint8_t* __restrict__ flags, uint64_t n, uint64_t* __restrict__ partials)
{
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t i0 = (uint64_t(blockIdx.x) * kThreads + threadIdx.x) * kFlagItems;
    uint64_t total;
    block_exclusive_scan(__popc(flag_bits(flags, i0, n)), s_wave, &total);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// keys[i] = flag[i] ? packed[rank(i)] : 0, and the next position.
__global__ void __launch_bounds__(kThreads)
keys_select_kernel(const uint8_t* __restrict__ flags, uint64_t n, const uint32_t* __restrict__ packed,
                   const uint64_t* __restrict__ partials, uint64_t nb, uint32_t self_scan,
                   const uint64_t* __restrict__ grand, uint32_t* __restrict__ keys, uint64_t* __restrict__ next_draw,
                   uint64_t first_draw)
{
    __shared__ uint64_t s_wave[kWaves];
    uint64_t prefix, masked;
    plan_prefix(partials, nb, self_scan, grand, s_wave, prefix, masked);
    const uint64_t i0 = (uint64_t(blockIdx.x) * kThreads + threadIdx.x) * kFlagItems;
    const uint32_t m = flag_bits(flags, i0, n);
    uint64_t total;
    uint64_t rank = block_exclusive_scan(__popc(m), s_wave, &total) + prefix;
    if (next_draw && blockIdx.x == nb - 1 && threadIdx.x == 0) *next_draw = first_draw + 4 * masked;
    if (i0 >= n) return;
    uint32_t k[kFlagItems];
#pragma unroll
    for (uint32_t j = 0; j < kFlagItems; ++j) {
        const bool on = (m >> j) & 1u;
        k[j] = on ? packed[rank] : 0u;
        rank += on ? 1u : 0u;
    }
    if (i0 + kFlagItems <= n) {
#pragma unroll
        for (uint32_t j = 0; j < kFlagItems; j += 4)
            *reinterpret_cast<uint4*>(keys + i0 + j) = make_uint4(k[j], k[j + 1], k[j + 2], k[j + 3]);
    } else {
#pragma unroll
        for (uint32_t j = 0; j < kFlagItems; ++j)
            if (i0 + j < n) keys[i0 + j] = k[j];
    }
}

// The workspace of a call with flags: n packed keys, the total's slot, one
// sum per block of kFlagBlock frames.
struct KeysLayout {
    uint64_t grand, partials, bytes;
};
inline KeysLayout keys_layout(uint64_t n)
{
    KeysLayout L;
    L.grand = align_up(4 * n, 16);
    L.partials = L.grand + 16;
    L.bytes = L.partials + 8 * uint64_t(grid_for(n, kFlagBlock));
    return L;
}

}  // namespace

extern "C" {

size_t cfws_draw_keys_workspace_size(size_t n_frames) { return (size_t)keys_layout(n_frames).bytes; }

size_t cfws_draw_keys_group_frames(void) { return kGroupFrames; }

int cfws_draw_mask_keys_device(uint32_t seed, uint64_t first_draw, size_t n, const uint8_t* d_mask_flags,
                               uint32_t* d_keys, uint64_t* d_next_draw, void* ws, size_t ws_size, void* stream)
{
    const CfwsPassScope pass_scope;                       // not a timed pass: a pending pair is dropped
    if (int rc = check_init()) return rc;
    if (first_draw > kCfwsKeyMaxFirstDraw)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "first_draw above 2^62", hipSuccess);
    if (uint64_t(n) >> 32) return set_err(CFWS_ERROR_INVALID_ARGUMENT, "2^32 frames or more", hipSuccess);
    if (n != 0 && !d_keys) return set_err(CFWS_ERROR_INVALID_ARGUMENT, "null pointer", hipSuccess);
    if (n != 0 && misaligned(d_keys, nullptr))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "d_keys must be 16-byte aligned", hipSuccess);
    const bool flags = n != 0 && d_mask_flags;
    const KeysLayout L = keys_layout(n);
    if (flags && (!ws || ws_size < L.bytes)) return set_err(CFWS_ERROR_WORKSPACE, "workspace too small", hipSuccess);
    if (flags && misaligned(ws, nullptr))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "workspace must be 16-byte aligned", hipSuccess);
    KeyState base;
    if (cfws_internal_key_state(seed, first_draw, base.h))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "seed", hipSuccess);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0 && !d_next_draw) return CFWS_OK;
    if (!flags) {                                         // n == 0: the next position only
        draw_keys_kernel<<<grid_for(n, kGroupFrames), kThreads, 0, st>>>(base, n, d_keys, d_next_draw,
                                                                         first_draw + 4 * uint64_t(n));
        return launch_check("draw_mask_keys_device");
    }
    uint32_t* packed = ws_ptr<uint32_t>(ws, 0);
    uint64_t* partials = ws_ptr<uint64_t>(ws, L.partials);
    uint64_t* grand = ws_ptr<uint64_t>(ws, L.grand);
    const uint32_t nb = grid_for(n, kFlagBlock);
    const uint32_t self_scan = nb <= kSelfScanBlocks ? 1u : 0u;
    draw_keys_kernel<<<grid_for(n, kGroupFrames), kThreads, 0, st>>>(base, n, packed, nullptr, 0);
    keys_count_kernel<<<nb, kThreads, 0, st>>>(d_mask_flags, n, partials);
    if (!self_scan) scan_partials_kernel<<<1, kThreads, 0, st>>>(partials, nb, grand);
    keys_select_kernel<<<nb, kThreads, 0, st>>>(d_mask_flags, n, packed, partials, nb, self_scan, grand, d_keys,
                                                d_next_draw, first_draw);
    return launch_check("draw_mask_keys_device(flags)");
}

}  // extern "C"
