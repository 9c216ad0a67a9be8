// cfws_slots.hip -- the receive into fixed payload slots
// (cfws_deserialize_slots, _scatter, _slots_info, _scatter_info and
// _slots_uniform, include/cfws.h).
//
// Frame i's payload goes to slot i (payload_off = i * slot), or to the
// caller's dst[i] (the scatter form): no prefix, so no look-back, and the
// pass reads each wire line once. The packed receive cannot: a frame's
// destination needs every earlier header, so its header line is fetched by
// the parse and again by the copy (§9: 6.86 GB per 16 M x 256 B launch
// against 4.43 GB of wire).
//
// One argument block (SlotsArgs) and one per-frame prologue (slot_frame:
// start, destination, parse, slot rule, the frame's record, the total) serve
// three kernels, picked by slots_route from the slot size and the batch's
// average frame:
//  * deserialize_slots_window_kernel, slots up to kSlotWindow8Max bytes:
//    every block of a frame's window loaded once, frames packed into shared
//    wave-rounds (window_shape);
//  * deserialize_slots_piece_kernel, larger slots (and full ones from 2 KiB
//    on whose pieces pay, piece_pays): one wave per 2 KiB piece of a frame;
//  * deserialize_slots_kernel, short frames in large slots: one frame per
//    thread parsed, the wave's 64 frames copied by fused_item.
#include "cfws_kernels.h"

#include <type_traits>

namespace {

// A slot receive's arguments, in the order of the kernels' parameters. The
// entry points fill them in and slots_impl launches through launch_slots.
// The kernels take them one by one (`__restrict__` holds on parameters, not
// on a struct's members: passed as a struct by value, the eight-sub-window
// kernels spilled SGPRs and lost a wave per SIMD) and bundle them again,
// brace-initialised, for the prologue -- the window kernel only where it
// calls it: a block whose address a call takes ahead of the kernel's loops
// cost those same kernels their registers too.
struct SlotsArgs {
    const uint8_t* wire;
    uint64_t wire_size;
    const uint64_t* index;       // frame starts; null: frame i starts at i * stride
    uint64_t n;
    uint64_t max_payload;
    uint64_t slot;
    cfws_frame_desc_t* desc;     // a frame's record: descriptor + status, or (kInfo) ...
    int32_t* status;
    uint8_t* out;
    uint64_t capacity;
    uint64_t* user_total;        // may be null
    const uint64_t* dst;         // kScatter: frame i's payload offset
    cfws_frame_info_t* info;     // ... an 8-byte info entry
    uint64_t stride;
    uint32_t* mismatch;          // may be null: counts the frames that are not uniform frames
};

__device__ __forceinline__ uint4 shfl16(uint4 v, int src)
{
    return make_uint4((uint32_t)__shfl((int)v.x, src, 64), (uint32_t)__shfl((int)v.y, src, 64),
                      (uint32_t)__shfl((int)v.z, src, 64), (uint32_t)__shfl((int)v.w, src, 64));
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src)
{
    return (uint64_t)__shfl((long long)v, src, 64);
}

// The slot rule: a COMPLETE frame whose non-empty payload is longer than the
// slot, or ends past the capacity, gets CFWS_ERROR_OUT_OF_MEMORY (the
// reference's failed allocation, co_ws_frame.c:216-223); its slot is not
// written.
__device__ __forceinline__ int32_t slot_rule(int32_t st, uint64_t run, uint64_t ps, uint64_t slot, uint64_t cap)
{
    return st == CFWS_PARSE_COMPLETE && ps > 0 && (ps > slot || run > cap || ps > cap - run)
               ? CFWS_ERROR_OUT_OF_MEMORY : st;
}

// The scatter form (cfws_deserialize_scatter): frame i's payload at the
// caller's dst[i] instead of i * slot, which must be a multiple of 16 (the
// copy stores whole aligned blocks); a frame whose offset is not does not
// fit either.
__device__ __forceinline__ int32_t scatter_rule(int32_t st, uint64_t run, uint64_t ps, uint64_t slot, uint64_t cap)
{
    st = slot_rule(st, run, ps, slot, cap);
    return st == CFWS_PARSE_COMPLETE && ps > 0 && (run & 15u) ? CFWS_ERROR_OUT_OF_MEMORY : st;
}

__device__ __forceinline__ void slot_desc(cfws_frame_desc_t* desc, int32_t* status, uint64_t f, uint64_t run,
                                          const cfws_frame_desc_t& d, int32_t st)
{
    uint4* q = reinterpret_cast<uint4*>(desc + f);
    const uint64_t w3 = (uint64_t)d.mask_key | (uint64_t)d.fin << 32 | (uint64_t)d.opcode << 40 |
                        (uint64_t)d.mask << 48 | (uint64_t)d.header_size << 56;
    q[0] = make_uint4((uint32_t)run, (uint32_t)(run >> 32), (uint32_t)d.wire_off, (uint32_t)(d.wire_off >> 32));
    q[1] = make_uint4((uint32_t)d.payload_size, (uint32_t)(d.payload_size >> 32), (uint32_t)w3,
                      (uint32_t)(w3 >> 32));
    status[f] = st;
}

// The compact per-frame output (cfws_deserialize_slots_info /
// _scatter_info): the reference frame's header fields and the status in 8
// bytes, one u64 store per frame (consecutive lanes, consecutive entries).
__device__ __forceinline__ void slot_info(cfws_frame_info_t* info, uint64_t f, const cfws_frame_desc_t& d, int32_t st)
{
    const uint32_t ps = d.payload_size > 0xffffffffull ? 0xffffffffu : (uint32_t)d.payload_size;
    const uint32_t w1 = (uint32_t)d.fin | (uint32_t)d.opcode << 8 | ((uint32_t)st & 0xffffu) << 16;
    reinterpret_cast<uint2*>(info)[f] = make_uint2(ps, w1);
}

// the uniform receive's check: lanes whose frame is not a COMPLETE frame of
// exactly `stride` wire bytes, one atomic per wave that has any
__device__ __forceinline__ void count_mismatch(uint32_t* mismatch, bool odd, uint32_t lane)
{
    const uint64_t b = __ballot(odd);
    if (b && lane == 0) atomicAdd(mismatch, (uint32_t)__popcll(b));
}

// ---- the per-frame prologue -----------------------------------------------------
// the frame's start: the index, or frame i at i * stride (the uniform
// receive: no index load ahead of the frame's own loads)
__device__ __forceinline__ uint64_t slot_start(const uint64_t* index, uint64_t stride, uint64_t f)
{
    return index ? index[f] : f * stride;
}

// the frame's payload offset: its slot, or the caller's (scatter)
template <bool kScatter>
__device__ __forceinline__ uint64_t slot_dest(const uint64_t* dst, uint64_t slot, uint64_t f)
{
    return kScatter ? dst[f] : f * slot;
}

// What the copy needs of a frame.
struct SlotFrame {
    int32_t st;      // the parse's status after the slot (scatter) rule: the payload is copied when COMPLETE
    uint64_t len;    // payload bytes
    uint32_t hs;     // header bytes: the payload starts at s0 + hs
    uint32_t key;    // zero when unmasked
    uint64_t run;    // destination
    bool odd;        // not a COMPLETE frame of exactly `stride` wire bytes (the mismatch count)
};

// Frame f of the pass, starting at wire byte s0 and going to payload offset
// `run`: parsed -- from its first 16 bytes in hw when `regs`, from the wire
// otherwise -- and put to the slot (scatter) rule. `write`: also writes the
// frame's record (descriptor + status, or the info entry: kInfo) and, for
// the last frame, the pass total.
template <bool kScatter, bool kInfo>
__device__ __forceinline__ SlotFrame slot_frame(const SlotsArgs& a, uint64_t f, uint64_t s0, uint64_t run, bool regs,
                                                uint4 hw, bool write)
{
    cfws_frame_desc_t d;
    int32_t st;
    if (regs) {
        const uint32_t w[4] = {hw.x, hw.y, hw.z, hw.w};
        st = parse_ws_header_regs(w, a.wire_size - s0, a.max_payload, d);
        d.wire_off = s0;
    } else {
        st = parse_ws_header(a.wire, a.wire_size, s0, a.max_payload, d);
    }
    st = kScatter ? scatter_rule(st, run, d.payload_size, a.slot, a.capacity)
                  : slot_rule(st, run, d.payload_size, a.slot, a.capacity);
    if (write) {
        if constexpr (kInfo)
            slot_info(a.info, f, d, st);
        else
            slot_desc(a.desc, a.status, f, run, d, st);
        if (f == a.n - 1 && a.user_total) {
            const uint64_t t = a.n * a.slot;
            *a.user_total = t < a.capacity ? t : a.capacity;
        }
    }
    SlotFrame F;
    F.st = st;
    F.len = d.payload_size;
    F.hs = d.header_size;
    F.key = d.mask ? d.mask_key : 0u;
    F.run = run;
    F.odd = st != CFWS_PARSE_COMPLETE || d.header_size + d.payload_size != a.stride;
    return F;
}

// ---- slots up to kSlotWindow8Max bytes: windows ---------------------------------
// A frame's window is the 16-byte block holding its first byte and the G - 1
// after it, G = slot / 16 + 2 (block phase <= 15 plus header <= 14 plus
// payload <= slot bytes), one block per virtual lane. S sub-windows of 64
// lanes give 64 S virtual lanes, so P = 64 S / G frames share a wave-round
// (window_shape). A wave takes R rounds (R P <= 64 frames) per iteration:
// lane l loads frame l's index, every round's window blocks are issued at
// once together with each frame's 16 header bytes (one unaligned load, lane =
// frame: the same lines as the windows, in flight together, so HBM sees them
// once), each lane parses its frame and writes its descriptor and status
// (consecutive lanes, consecutive entries), and each round then takes its
// frames' (length, phase + header, key) from the parsing lanes. A virtual
// lane's 16 payload bytes start (phase + header) bytes into its own block:
// blocks c and c + 1, or c + 1 and c + 2 past 16 (DPP shifts by one lane, no
// LDS; a sub-window's last two lanes take the next sub-window's first two
// blocks), funnelled and unmasked (each chunk starts at a payload index that
// is a multiple of 16: no key rotation). Blocks at or past the wire's end are
// not loaded. The first form parsed in every lane of every round (480
// instructions per 3 frames at 256 B) and ran at 5.2 TB/s.
constexpr uint64_t kSlotWindow8Max = 512 * 16 - 32;   // eight blocks per lane up to 8,160 B
// Rounds per iteration (their loads in flight together): 8 for one frame per
// round (slots over 480 B), 4 for more (16 M x 256 B receive 1.686 -> 1.620
// ms; 12 or 16 rounds: 3.3 ms; 8 M x 512 B at 4 rounds 1.59 -> 1.76 ms).
#ifndef CFWS_SLOT_ROUNDS
#define CFWS_SLOT_ROUNDS 8
#endif
#ifndef CFWS_SLOT_ROUNDS_MULTI
#define CFWS_SLOT_ROUNDS_MULTI 4
#endif
#ifndef CFWS_SLOT_ROUNDS2
#define CFWS_SLOT_ROUNDS2 4      // two blocks per lane (1,008-2,016 B): 2,016 B 2 / 4 / 6 -> 1.61-1.62 / 1.61 / 1.63 ms
#endif
#ifndef CFWS_SLOT_ROUNDS8
#define CFWS_SLOT_ROUNDS8 1      // eight blocks per lane (4,080-8,160 B)
#endif
#ifndef CFWS_SLOT_ROUNDS4
#define CFWS_SLOT_ROUNDS4 1      // four blocks per lane (2,032-4,064 B): 3 KiB 1 / 2 / 4 -> 1.48 / 1.55 / 1.59 ms
#endif

// Sub-window packing. Closed A/Bs, once the knobs CFWS_SLOT_SUB2_G,
// CFWS_SLOT_SUB2_G_IMPLICIT and CFWS_SLOT_SUB4_G; what each measured:
//  * indexed, 33-42 lanes (496-640 B) three to a pair: 512 B 1.535 -> 1.498 ms (profiles/r05/slots/sub2_ab/)
//  * index-free, the same: off, 8 M x 512 B 1.50 -> 1.62 ms (profiles/r06/compact/implicit/)
//  * 65-85 lanes three to four sub-windows: off, 1 KiB 1.523 -> 1.589-1.593 ms (profiles/r05/slots/sub4_ab/)
constexpr uint32_t kSlotSub2MinG = 33, kSlotSub2MaxG = 128 / 3;

// A window launch's shape: S sub-windows of 64 lanes, P frames per
// wave-round, `rounds` rounds of loads in flight (S and rounds: the kernel's
// template values), of which a wave-iteration takes R (R P <= 64: lane =
// frame in the parse). The host takes all four from window_shape; the kernel,
// which has S and rounds, takes P and R from the same two functions.
struct WindowShape {
    uint32_t S, P, rounds, R;
};

// P: frames of G lanes in S sub-windows
__host__ __device__ constexpr uint32_t window_frames(uint32_t G, uint32_t S)
{
    return 64 * S / G;
}

// R: of `rounds` rounds, those that P frames each keep within 64 frames
__host__ __device__ constexpr uint32_t window_rounds(uint32_t P, uint32_t rounds)
{
    return P * rounds <= 64 ? rounds : 64 / P;
}

// The shape of a receive of G-lane frames (G = slot / 16 + 2 <= 512), with
// (`indexed`) or without an index.
__host__ __device__ constexpr WindowShape window_shape(uint32_t G, bool indexed)
{
    const uint32_t S = G > 256 ? 8 : G > 128 ? 4
                       : G > 64 || (indexed && G >= kSlotSub2MinG && G <= kSlotSub2MaxG) ? 2 : 1;
    const uint32_t rounds = S == 8 ? CFWS_SLOT_ROUNDS8 : S == 4 ? CFWS_SLOT_ROUNDS4 : S == 2 ? CFWS_SLOT_ROUNDS2
                            : window_frames(G, 1) > 1 ? CFWS_SLOT_ROUNDS_MULTI : CFWS_SLOT_ROUNDS;
    const uint32_t P = window_frames(G, S);
    return {S, P, rounds, window_rounds(P, rounds)};
}

// the class edges: G = slot / 16 + 2
constexpr bool shape_is(uint32_t G, bool indexed, uint32_t S, uint32_t P)
{
    return window_shape(G, indexed).S == S && window_shape(G, indexed).P == P;
}
static_assert(shape_is(3, true, 1, 21) && shape_is(3, false, 1, 21), "16 B slots");
#if CFWS_SLOT_ROUNDS_MULTI == 4
static_assert(window_shape(3, true).R == 3, "16 B slots: 4 rounds of 21 frames would exceed 64 frames");
static_assert(window_shape(18, true).R == 4 && window_shape(18, false).R == 4, "256 B slots");
#endif
static_assert(shape_is(18, true, 1, 3) && shape_is(18, false, 1, 3), "256 B slots");
static_assert(shape_is(32, true, 1, 2) && shape_is(32, false, 1, 2), "480 B slots");
static_assert(shape_is(33, true, 2, 3) && shape_is(33, false, 1, 1), "496 B slots");
static_assert(shape_is(42, true, 2, 3) && shape_is(42, false, 1, 1), "640 B slots");
static_assert(shape_is(43, true, 1, 1) && shape_is(43, false, 1, 1), "656 B slots");
static_assert(shape_is(64, true, 1, 1) && shape_is(64, false, 1, 1), "992 B slots");
static_assert(shape_is(65, true, 2, 1) && shape_is(65, false, 2, 1), "1,008 B slots");
static_assert(shape_is(128, true, 2, 1) && shape_is(128, false, 2, 1), "2,016 B slots");
static_assert(shape_is(129, true, 4, 1) && shape_is(129, false, 4, 1), "2,032 B slots");
static_assert(shape_is(256, true, 4, 1) && shape_is(256, false, 4, 1), "4,064 B slots");
static_assert(shape_is(257, true, 8, 1) && shape_is(257, false, 8, 1), "4,080 B slots");
static_assert(shape_is(512, true, 8, 1) && shape_is(512, false, 8, 1), "8,160 B slots");
static_assert(kSlotWindow8Max / 16 + 2 == 512, "the largest window is eight sub-windows");

// kSlotRounds, kSub: the launch's window_shape (rounds, S); G its frames' lanes
template <int kSlotRounds, int kSub, bool kScatter, bool kInfo>
__global__ void __launch_bounds__(kThreads)
deserialize_slots_window_kernel(const uint8_t* __restrict__ wire, uint64_t wire_size,
                                const uint64_t* __restrict__ index, uint64_t n, uint64_t max_payload,
                                uint64_t slot, cfws_frame_desc_t* __restrict__ desc,
                                int32_t* __restrict__ status, uint8_t* __restrict__ out, uint64_t capacity,
                                uint64_t* __restrict__ user_total, const uint64_t* __restrict__ dst,
                                cfws_frame_info_t* __restrict__ infos, uint64_t stride,
                                uint32_t* __restrict__ mismatch, uint32_t G)
{
    const uint32_t lane = threadIdx.x & 63u;
    // kSub sub-windows of 64 lanes make 64 kSub virtual lanes, v = 64 sw +
    // lane; frame g of a round takes virtual lanes [g G, g G + G), P = 64 kSub
    // / G frames, so lane `lane` of sub-window sw holds block c[sw] of the
    // round's frame g[sw]
    const uint32_t P = window_frames(G, kSub);
    uint32_t g[kSub], c[kSub];
#pragma unroll
    for (int sw = 0; sw < kSub; ++sw) {
        g[sw] = (64u * sw + lane) / G;
        c[sw] = 64u * sw + lane - g[sw] * G;
    }
    const uint32_t R = window_rounds(P, kSlotRounds);
    const uint64_t FI = uint64_t(R) * P;                 // frames per wave-iteration
    const uint64_t grid_frames = uint64_t(gridDim.x) * kWaves * FI;
    const uint4 z = make_uint4(0, 0, 0, 0);
    const bool b16 = wire_size >= 16;
    const uint64_t lastu = wire_size - 16;
    for (uint64_t f0 = (uint64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6)) * FI; f0 < n; f0 += grid_frames) {
        const uint64_t fl = f0 + lane;
        const bool mine = lane < FI && fl < n;
        // the frame's start: the index, or frame i at i * stride (the uniform
        // receive: its window loads need no index load before them)
        const uint64_t wl = !mine ? ~uint64_t(0) : slot_start(index, stride, fl);
        // the frame's payload offset: its slot, or the caller's (scatter)
        const uint64_t runl = !mine ? 0 : slot_dest<kScatter>(dst, slot, fl);
        // every round's window block, then each frame's header bytes
        uint4 A[kSlotRounds][kSub];
#pragma unroll
        for (int u = 0; u < kSlotRounds; ++u) {
#pragma unroll
            for (int sw = 0; sw < kSub; ++sw) {
                const uint32_t src = (uint32_t)u * P + g[sw];
                const uint64_t wo = shfl64(wl, (int)(src < 64 ? src : 63));
                const uint64_t blk = (wo & ~uint64_t(15)) + 16ull * c[sw];   // block c of the window
                A[u][sw] = (uint32_t)u < R && g[sw] < P && wo < wire_size && blk < wire_size
                               ? ld16(wire + blk) : z;
            }
        }
        const uint4 hw = mine && b16 && wl <= lastu ? ld16u(wire + wl) : z;
        // lane l parses frame f0 + l; its round info: payload length (<= slot
        // < 2^16) | (phase + header size) << 16, zero when not copied
        uint32_t info = 0, key = 0;
        bool odd = false;
        if (mine) {
            const SlotsArgs a = {wire, wire_size, index, n, max_payload, slot, desc, status, out, capacity, user_total,
                                 dst, infos, stride, mismatch};
            const SlotFrame F = slot_frame<kScatter, kInfo>(a, fl, wl, runl, b16 && wl <= lastu, hw, true);
            if (F.st == CFWS_PARSE_COMPLETE && F.len > 0)
                info = (uint32_t)F.len | ((uint32_t)(wl & 15u) + F.hs) << 16;
            key = F.key;
            odd = F.odd;
        }
        if (mismatch) count_mismatch(mismatch, odd, lane);
#pragma unroll
        for (int u = 0; u < kSlotRounds; ++u) {
            if ((uint32_t)u >= R) break;   // wave-uniform
#pragma unroll
            for (int sw = 0; sw < kSub; ++sw) {
                const uint32_t src = (uint32_t)u * P + g[sw];
                const int s = (int)(src < 64 ? src : 63);
                const uint32_t inf = (uint32_t)__shfl((int)info, s, 64);
                const uint32_t k = (uint32_t)__shfl((int)key, s, 64);
                const uint32_t len = inf & 0xffffu, off = inf >> 16;
                const uint64_t runf = kScatter ? shfl64(runl, s) : (f0 + src) * slot;
                // blocks c + 1 and c + 2 of this sub-window, by DPP (every
                // lane); lanes 62 and 63 of a sub-window take the next one's
                // first two blocks
                const uint4 l0 = sw + 1 < kSub ? shfl16(A[u][sw + 1 < kSub ? sw + 1 : sw], 0) : z;
                const uint4 l1 = sw + 1 < kSub ? shfl16(A[u][sw + 1 < kSub ? sw + 1 : sw], 1) : z;
                const uint4 n1 = from_next_lane(A[u][sw], l0);
                const uint4 n2 = from_next_lane(n1, l1);
                const uint32_t q = c[sw];          // payload chunk
                if (g[sw] < P && 16u * q < len) {
                    const bool k1 = off >= 16;
                    const uint4 B0 = k1 ? n1 : A[u][sw], B1 = k1 ? n2 : n1;
                    const uint32_t sh = off & 15u;
                    uint4 o = sh ? funnel16(B0, B1, sh) : B0;
                    xor4(o, k);
                    if (len - 16u * q < 16u) o = and4(o, byte_range(0, len - 16u * q));
                    fused_store(out, runf + 16ull * q, capacity, o);
                }
            }
        }
    }
}

// ---- short frames in large slots: one frame per thread ---------------------------
#ifndef CFWS_SLOT_UNROLL
#define CFWS_SLOT_UNROLL 16      // slots over 8,160 B: 64 K x 64 KiB receive 2.04 / 1.76 / 1.71 ms at 4 / 8 / 16 rounds, 8 KiB 1.72 at each
#endif
constexpr int kSlotUnroll = CFWS_SLOT_UNROLL;   // deserialize_slots_kernel: rounds of loads in flight

// One frame per thread parsed (its header line fetched twice), the wave's 64
// payloads copied by fused_item, which packs short frames into shared
// wave-instructions.
template <bool kScatter, bool kInfo>
__global__ void __launch_bounds__(kThreads)
deserialize_slots_kernel(const uint8_t* __restrict__ wire, uint64_t wire_size, const uint64_t* __restrict__ index,
                         uint64_t n, uint64_t max_payload, uint64_t slot, cfws_frame_desc_t* __restrict__ desc,
                         int32_t* __restrict__ status, uint8_t* __restrict__ out, uint64_t capacity,
                         uint64_t* __restrict__ user_total, const uint64_t* __restrict__ dst,
                         cfws_frame_info_t* __restrict__ info, uint64_t stride, uint32_t* __restrict__ mismatch)
{
    const SlotsArgs a = {wire, wire_size, index, n, max_payload, slot, desc, status, out, capacity, user_total,
                         dst, info, stride, mismatch};
    const uint64_t f = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    uint64_t run = 0, src = 0;
    uint32_t len = 0, nb = 0, key = 0;
    bool odd = false;
    if (f < a.n) {
        const uint64_t s0 = slot_start(a.index, a.stride, f);
        run = slot_dest<kScatter>(a.dst, a.slot, f);
        const SlotFrame F = slot_frame<kScatter, kInfo>(a, f, s0, run, false, make_uint4(0, 0, 0, 0), true);
        if (F.st == CFWS_PARSE_COMPLETE) {
            len = (uint32_t)F.len;   // <= slot < 2^31
            nb = (len + 15u) & ~15u;
            src = s0 + F.hs;
            key = F.key;
        }
        odd = F.odd;
    }
    if (a.mismatch) count_mismatch(a.mismatch, odd, threadIdx.x & 63u);
    fused_item<kSlotUnroll>(a.wire, a.out, a.capacity, run, src, len, nb, key, threadIdx.x & 63u);
}

// ---- large slots, piece by piece --------------------------------------------------
// Wave w copies piece w % P of frame w / P (kSlotPiece bytes of slot), so a
// 64 KiB frame is 32 waves' work and a launch has n x P waves. P is the
// slot's piece count; when the batch's frames are shorter on average (wire
// bytes / frames) P is that average's piece count and each wave takes pieces
// w % P, w % P + P, ... (kLoop), so a large slot holding short payloads does
// not cost a wave per piece of the slot. Batches averaging under one piece
// per frame take the per-frame kernel, which packs short frames into shared
// wave-instructions (slots_route; tools/slot_sparse_probe.py: 1 M x 256 B in
// 16 KiB slots 0.13 ms there against 0.59 one wave per frame). The per-frame
// kernel above gives each wave the 64 frames its lanes parsed, one after
// another: 1,024 waves for 64 K frames, one per SIMD. Every wave of a frame
// parses its header (one line, the same address in every lane); piece 0's
// lane 0 writes the frame's descriptor + status or info entry and counts a
// mismatch. 64 K x 64 KiB receive (profiles/r06/compact/slot_pieces/):
// per-frame kernel 1.59-1.64 ms; pieces of 8 / 4 / 2 / 1 KiB 1.51-1.60 /
// 1.42-1.49 / 1.35-1.36 / 2.13 ms; 2 KiB with write-through stores 1.31-1.32
// (8 KiB frames 1.38, against 1.51-1.64).
#ifndef CFWS_SLOT_PIECE_AUX
#define CFWS_SLOT_PIECE_AUX 19        // write-through (sc0 sc1 nt), as the WS receive; 0: the global nt store
#endif
#ifndef CFWS_SLOT_PIECE_UNROLL
#define CFWS_SLOT_PIECE_UNROLL 2
#endif
constexpr int kSlotPieceUnroll = CFWS_SLOT_PIECE_UNROLL;            // rounds of loads in flight per wave
constexpr uint64_t kSlotPiece = 64ull * 16 * kSlotPieceUnroll;     // 2 KiB
template <bool kScatter, bool kInfo, bool kLoop>
__global__ void __launch_bounds__(kThreads)
deserialize_slots_piece_kernel(const uint8_t* __restrict__ wire, uint64_t wire_size, const uint64_t* __restrict__ index,
                               uint64_t n, uint64_t max_payload, uint64_t slot, cfws_frame_desc_t* __restrict__ desc,
                               int32_t* __restrict__ status, uint8_t* __restrict__ out, uint64_t capacity,
                               uint64_t* __restrict__ user_total, const uint64_t* __restrict__ dst,
                               cfws_frame_info_t* __restrict__ info, uint64_t stride, uint32_t* __restrict__ mismatch,
                               uint64_t pieces)
{
    const SlotsArgs a = {wire, wire_size, index, n, max_payload, slot, desc, status, out, capacity, user_total,
                         dst, info, stride, mismatch};
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t waves = a.n * pieces;
    for (uint64_t w = uint64_t(blockIdx.x) * kWaves + wv; w < waves; w += uint64_t(gridDim.x) * kWaves) {
        const uint64_t f = w / pieces, piece = w - f * pieces;
        const uint64_t s0 = slot_start(a.index, a.stride, f);
        const bool write = piece == 0 && lane == 0;
        const SlotFrame F = slot_frame<kScatter, kInfo>(a, f, s0, slot_dest<kScatter>(a.dst, a.slot, f), false,
                                                        make_uint4(0, 0, 0, 0), write);
        if (write && a.mismatch && F.odd) atomicAdd(a.mismatch, 1u);
        if (F.st != CFWS_PARSE_COMPLETE) continue;           // wave-uniform: every lane parsed the same frame
        const uint64_t len = F.len;                          // <= slot <= 2^31
        const uint64_t nb = (len + 15) & ~uint64_t(15);
        const uint64_t src = s0 + F.hs, run = F.run;
        const uint32_t ph = (uint32_t)(src & 15u);
        // this wave's piece of the frame (kLoop: pieces piece, piece + P, ...;
        // without, the loop body once: the straight-line form measured 7 %
        // faster when every frame fills its slot)
        for (uint64_t c0 = piece * kSlotPiece; c0 < nb; c0 += pieces * kSlotPiece) {
            const auto prs = __builtin_amdgcn_make_buffer_rsrc(a.out + run + c0, 0, (int)kSlotPiece, 0x00020000);
            uint4 A[kSlotPieceUnroll], E[kSlotPieceUnroll];
            uint32_t need[kSlotPieceUnroll];
            bool nl[kSlotPieceUnroll];
#pragma unroll
            for (int u = 0; u < kSlotPieceUnroll; ++u)
                frame_chunk_load(a.wire, src, len, c0 + (uint64_t)u * 1024 + 16 * lane, ph, lane, A[u], E[u], need[u],
                                 nl[u]);
#pragma unroll
            for (int u = 0; u < kSlotPieceUnroll; ++u) {
                const uint64_t k0 = c0 + (uint64_t)u * 1024 + 16 * lane;
                frame_chunk_value(A[u], E[u], need[u], nl[u], ph, F.key, k0 < nb, [&](uint4 o) {
                    if (CFWS_SLOT_PIECE_AUX != 0 && run + k0 + 16 <= a.capacity) {
                        // a buffer store over the wave's piece (cache policy CFWS_SLOT_PIECE_AUX)
                        const u32x4 v = {o.x, o.y, o.z, o.w};
                        __builtin_amdgcn_raw_buffer_store_b128(v, prs, (int)(k0 - c0), 0, CFWS_SLOT_PIECE_AUX);
                    } else {
                        fused_store(a.out, run + k0, a.capacity, o);
                    }
                });
            }
            if (!kLoop) break;
        }
    }
}

// ---- the route ----------------------------------------------------------------------
bool slots_window()
{
    static const bool v = env_knob("CFWS_SLOTS_WINDOW", 1) != 0;
    return v;
}

// the kernel a slot / scatter receive takes (slots_impl and
// cfws_deserialize_slots_pass_kernel): windows up to kSlotWindow8Max-byte
// slots, pieces past that (A/B knob: CFWS_SLOTS_WINDOW=0 falls back to the
// piece and per-frame kernels)
enum SlotsRoute { kSlotsWindow, kSlotsPiece, kSlotsPerFrame };
// Closed A/Bs, once the knobs CFWS_SLOTS_PIECE and CFWS_SLOTS_PIECE_MIN:
//  * pieces on: 64 K x 64 KiB 1.31-1.32 ms against the per-frame kernel's 1.59-1.64
//  * from 2 KiB slots: 2 KiB 1.47 ms against the windows' 1.84 (piece_pays, below)
constexpr uint64_t kSlotPieceMin = 2048;
// Slots of 2 KiB up to kSlotWindow8Max take pieces too where the pieces'
// lanes are at least 85 % used and every piece starts on a 128-byte line.
// Receive without / with an index (profiles/r06/compact/slot_pieces/):
// 2 / 4 / 6 / 7.5 KiB 1.41 / 1.38 / 1.36 / 1.45 and 1.47 / 1.43 / 1.40 /
// 1.47 ms against the windows' 1.59 / 1.58 / 1.54 / 1.57 and 1.84 / 1.62 /
// 1.52 / 1.51; 5 KiB (83 % used) 1.47 / 1.56 against 1.52 / 1.53; 2.5 / 3 KiB
// (63 / 75 %) 1.90 / 1.62 against 1.52 / 1.48; 8,160 B (off the 128-byte
// lines) 1.86 against 1.69.
bool piece_pays(uint64_t slot)
{
    const uint64_t pieces = (slot + kSlotPiece - 1) / kSlotPiece;
    return slot % 128 == 0 && 20 * slot >= 17 * pieces * kSlotPiece;
}

SlotsRoute slots_route(uint64_t slot, uint64_t n, uint64_t wire_size)
{
    // the batch's average frame (wire bytes): pieces pay for frames that
    // fill them, not for short frames in large slots
    const uint64_t avg = n ? wire_size / n : 0;
    const bool piece = slot >= kSlotPieceMin &&
                       (slot > kSlotWindow8Max ? avg > 1040 : piece_pays(slot) && 20 * avg >= 17 * slot);
    // a window spans the whole slot, whatever the frame: frames of up to
    // 1 KiB filling under half their slot (under 80 % of a slot of 1 KiB or
    // more) take the per-frame kernel, which packs them into shared
    // wave-instructions (tools/slot_sparse_probe.py: 256 B frames in 4 KiB
    // slots 0.14 against 1.15 ms, 512 B in 1 KiB 0.91 against 1.25, 768 B in
    // 1 KiB 1.30 against 1.41; 128 B in 256 B slots stay on the windows,
    // 0.67 against 0.71)
    const bool sparse = avg <= 1040 && (2 * avg < slot || (slot >= 1024 && 5 * avg < 4 * slot));
    if (slot <= kSlotWindow8Max && slots_window() && !piece && !sparse) return kSlotsWindow;
    return piece ? kSlotsPiece : kSlotsPerFrame;
}

// ---- the launch ---------------------------------------------------------------------
// f(scatter, info) with the two run-time forms as compile-time ones
// (std::true_type / std::false_type): every kernel is instantiated per form
// -- the scatter form's per-round offset shuffle, as a run-time branch in one
// kernel, cost the 1 KiB slot receive 11 % (1.525 -> 1.70 ms)
template <typename F>
void with_forms(bool scatter, bool info, F&& f)
{
    if (scatter && info)
        f(std::true_type{}, std::true_type{});
    else if (scatter)
        f(std::true_type{}, std::false_type{});
    else if (info)
        f(std::false_type{}, std::true_type{});
    else
        f(std::false_type{}, std::false_type{});
}

// a slot kernel's launch: the argument block, then the kernel's own
template <typename K, typename... X>
void launch_slots(K kernel, uint32_t grid, hipStream_t st, const SlotsArgs& a, X... own)
{
    kernel<<<grid, kThreads, 0, st>>>(a.wire, a.wire_size, a.index, a.n, a.max_payload, a.slot, a.desc, a.status, a.out,
                                      a.capacity, a.user_total, a.dst, a.info, a.stride, a.mismatch, own...);
}

// The five entry points. scatter: frame i at a.dst[i], a.slot the largest
// payload a frame may have; otherwise at i * a.slot. a.info not null: info
// entries instead of descriptors and statuses.
int slots_impl(const SlotsArgs& a, bool scatter, void* stream, const char* what)
{
    if (int rc = check_init()) return rc;
    if (a.slot < 16 || (a.slot & 15) || a.slot > (1ull << 31))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "slot bytes must be a multiple of 16 in [16, 2^31]",
                       hipSuccess);
    if (a.n > 0xffffffffull) return set_err(CFWS_ERROR_INVALID_ARGUMENT, "too many frames", hipSuccess);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a.n == 0) {
        if (a.user_total && hipMemsetAsync(a.user_total, 0, sizeof(uint64_t), st) != hipSuccess)
            return launch_check(what);
        return CFWS_OK;
    }
    const bool info = a.info != nullptr;
    if (!a.wire || (!a.index && !a.stride) || (!info && (!a.desc || !a.status)) || (a.capacity && !a.out) ||
        (scatter && !a.dst))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "null pointer", hipSuccess);
    if (misaligned(a.out, a.wire))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "arenas must be 16-byte aligned", hipSuccess);
    if (reinterpret_cast<uintptr_t>(a.info) & 7u)          // slot_info stores each entry as one uint2
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "info entries must be 8-byte aligned", hipSuccess);
    const CfwsPassTimer timer(st);
    const SlotsRoute route = slots_route(a.slot, a.n, a.wire_size);
    if (route == kSlotsWindow) {
        // one wave-iteration of R P frames per wave (CFWS_SLOT_GRID caps the
        // workgroups: a grid-stride loop; A/B knob)
        const uint32_t G = (uint32_t)(a.slot / 16 + 2);
        const WindowShape w = window_shape(G, a.index != nullptr);
        const uint64_t per_block = uint64_t(kWaves) * w.R * w.P;
        static const uint64_t cap_blocks = [] {
            const int64_t v = env_knob("CFWS_SLOT_GRID", 0);   // 0: one iteration per wave
            return v > 0 ? (uint64_t)v : 0x7fffffffull;
        }();
        const uint64_t want = (a.n + per_block - 1) / per_block;
        const uint32_t grid = (uint32_t)(want < cap_blocks ? want : cap_blocks);
        with_forms(scatter, info, [&](auto sc, auto in) {
            constexpr bool kSc = decltype(sc)::value, kIn = decltype(in)::value;
            if (w.S == 8)
                launch_slots(deserialize_slots_window_kernel<CFWS_SLOT_ROUNDS8, 8, kSc, kIn>, grid, st, a, G);
            else if (w.S == 4)
                launch_slots(deserialize_slots_window_kernel<CFWS_SLOT_ROUNDS4, 4, kSc, kIn>, grid, st, a, G);
            else if (w.S == 2)
                launch_slots(deserialize_slots_window_kernel<CFWS_SLOT_ROUNDS2, 2, kSc, kIn>, grid, st, a, G);
            else if (w.P > 1)
                launch_slots(deserialize_slots_window_kernel<CFWS_SLOT_ROUNDS_MULTI, 1, kSc, kIn>, grid, st, a, G);
            else
                launch_slots(deserialize_slots_window_kernel<CFWS_SLOT_ROUNDS, 1, kSc, kIn>, grid, st, a, G);
        });
    } else if (route == kSlotsPiece) {
        // waves per frame: the slot's pieces, at most the pieces of the
        // batch's average frame (its wire bytes; at least one)
        const uint64_t slot_pieces = (a.slot + kSlotPiece - 1) / kSlotPiece;
        const uint64_t avg_pieces = (a.wire_size / a.n + kSlotPiece - 1) / kSlotPiece;
        const uint64_t pieces = avg_pieces < 1 ? 1 : avg_pieces < slot_pieces ? avg_pieces : slot_pieces;
        const uint64_t want = (a.n * pieces + kWaves - 1) / kWaves;
        const uint32_t grid = (uint32_t)(want < (1u << 22) ? want : (1u << 22));   // a grid-stride loop past that
        with_forms(scatter, info, [&](auto sc, auto in) {
            constexpr bool kSc = decltype(sc)::value, kIn = decltype(in)::value;
            if (pieces < slot_pieces)
                launch_slots(deserialize_slots_piece_kernel<kSc, kIn, true>, grid, st, a, pieces);
            else
                launch_slots(deserialize_slots_piece_kernel<kSc, kIn, false>, grid, st, a, pieces);
        });
    } else {
        with_forms(scatter, info, [&](auto sc, auto in) {
            launch_slots(deserialize_slots_kernel<decltype(sc)::value, decltype(in)::value>, grid_for(a.n, kThreads),
                         st, a);
        });
    }
    return launch_check(what);
}

// the arguments every entry point passes alike
SlotsArgs receive_args(const void* d_wire, uint64_t wire_size, const uint64_t* d_index, size_t n, uint64_t max_payload,
                       uint64_t slot, void* d_payload, uint64_t cap, uint64_t* d_total)
{
    SlotsArgs a = {};
    a.wire = static_cast<const uint8_t*>(d_wire);
    a.wire_size = wire_size;
    a.index = d_index;
    a.n = n;
    a.max_payload = max_payload;
    a.slot = slot;
    a.capacity = cap;
    a.out = static_cast<uint8_t*>(d_payload);
    a.user_total = d_total;
    return a;
}

}  // namespace

extern "C" {

int cfws_deserialize_slots(const void* d_wire, uint64_t wire_size, const uint64_t* d_index, size_t n,
                           uint64_t max_payload, uint64_t slot, cfws_frame_desc_t* d_desc, int32_t* d_status,
                           void* d_payload, uint64_t cap, uint64_t* d_total, void* stream)
{
    const CfwsPassScope pass_scope;
    SlotsArgs a = receive_args(d_wire, wire_size, d_index, n, max_payload, slot, d_payload, cap, d_total);
    a.desc = d_desc;
    a.status = d_status;
    return slots_impl(a, false, stream, "deserialize_slots");
}

int cfws_deserialize_scatter(const void* d_wire, uint64_t wire_size, const uint64_t* d_index,
                             const uint64_t* d_payload_off, size_t n, uint64_t max_payload, uint64_t max_slot,
                             cfws_frame_desc_t* d_desc, int32_t* d_status, void* d_payload, uint64_t cap,
                             void* stream)
{
    const CfwsPassScope pass_scope;
    SlotsArgs a = receive_args(d_wire, wire_size, d_index, n, max_payload, max_slot, d_payload, cap, nullptr);
    a.desc = d_desc;
    a.status = d_status;
    a.dst = d_payload_off;
    return slots_impl(a, true, stream, "deserialize_scatter");
}

int cfws_deserialize_slots_info(const void* d_wire, uint64_t wire_size, const uint64_t* d_index, size_t n,
                                uint64_t max_payload, uint64_t slot, cfws_frame_info_t* d_info, void* d_payload,
                                uint64_t cap, uint64_t* d_total, void* stream)
{
    const CfwsPassScope pass_scope;
    if (!d_info && n) return set_err(CFWS_ERROR_INVALID_ARGUMENT, "null pointer", hipSuccess);
    SlotsArgs a = receive_args(d_wire, wire_size, d_index, n, max_payload, slot, d_payload, cap, d_total);
    a.info = d_info;
    return slots_impl(a, false, stream, "deserialize_slots_info");
}

int cfws_deserialize_scatter_info(const void* d_wire, uint64_t wire_size, const uint64_t* d_index,
                                  const uint64_t* d_payload_off, size_t n, uint64_t max_payload, uint64_t max_slot,
                                  cfws_frame_info_t* d_info, void* d_payload, uint64_t cap, void* stream)
{
    const CfwsPassScope pass_scope;
    if (!d_info && n) return set_err(CFWS_ERROR_INVALID_ARGUMENT, "null pointer", hipSuccess);
    SlotsArgs a = receive_args(d_wire, wire_size, d_index, n, max_payload, max_slot, d_payload, cap, nullptr);
    a.info = d_info;
    a.dst = d_payload_off;
    return slots_impl(a, true, stream, "deserialize_scatter_info");
}

int cfws_deserialize_slots_uniform(const void* d_wire, uint64_t wire_size, size_t n, uint64_t stride,
                                   uint64_t max_payload, uint64_t slot, cfws_frame_info_t* d_info, void* d_payload,
                                   uint64_t cap, uint64_t* d_total, uint32_t* d_mismatch, void* stream)
{
    const CfwsPassScope pass_scope;
    if (int rc = check_init()) return rc;
    if (stride < 2 || (n && stride > (1ull << 63) / n))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "frame stride must be >= 2 and n * stride < 2^63", hipSuccess);
    if (!d_info && n) return set_err(CFWS_ERROR_INVALID_ARGUMENT, "null pointer", hipSuccess);
    if (d_mismatch && hipMemsetAsync(d_mismatch, 0, sizeof(uint32_t), static_cast<hipStream_t>(stream)) != hipSuccess)
        return launch_check("deserialize_slots_uniform");
    SlotsArgs a = receive_args(d_wire, wire_size, nullptr, n, max_payload, slot, d_payload, cap, d_total);
    a.info = d_info;
    a.stride = stride;
    a.mismatch = d_mismatch;
    return slots_impl(a, false, stream, "deserialize_slots_uniform");
}

const char* cfws_deserialize_slots_pass_kernel(size_t n, uint64_t wire_size, uint64_t slot)
{
    switch (slots_route(slot, n, wire_size)) {
    case kSlotsWindow: return "deserialize_slots_window_kernel";
    case kSlotsPiece: return "deserialize_slots_piece_kernel";
    default: return "deserialize_slots_kernel";
    }
}

}  // extern "C"
