// cfws_keys.hip -- cfws_draw_mask_keys_device: the keys
// cfws_draw_mask_keys_seeded_at gives, drawn on the device. Every lane enters
// the stream at the start of its own run (cfws_keydev.h: a wave jump, a lane
// jump, then a ring of 31 registers) and draws kLaneDraws times, stored as
// kLaneFrames / 4 chunks of 16 bytes: one 128-byte line. With mask flags the
// draw goes packed into the workspace (n keys: an upper bound) and a second
// pass ranks the masked frames and writes keys[i] = flag ? packed[rank] : 0.
#include "cfws_kernels.h"
#include "cfws_keydev.h"

namespace {

constexpr uint32_t kLaneFrames = uint32_t(kLaneDraws / 4);    // r: one lane's run
constexpr uint32_t kWaveFrames = 64 * kLaneFrames;            // w: one wave's run
constexpr uint32_t kGroupFrames = kWaves * kWaveFrames;       // G: one workgroup's
static_assert((uint64_t(1) << 32) / kWaveFrames <= (uint64_t(1) << kWaveBits), "wave index bits");
static_assert(kLaneFrames % 4 == 0, "a lane's run is whole 16-byte chunks");

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
    uint32_t W[kKeyWindow];
    key_wave_window(base, g, lane, W);

    const uint64_t k0 = wave_first + uint64_t(lane) * kLaneFrames;
    if (k0 >= n) return;
    uint32_t ring[kKeyDeg];
    key_lane_ring(W, lane, ring);
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
