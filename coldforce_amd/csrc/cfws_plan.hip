// cfws_plan.hip -- the WebSocket plans (cfws_serialize_plan,
// cfws_deserialize_plan): reduce / (scan) / apply launches,
// above kSelfScanBlocks blocks one single-pass kernel with a decoupled
// look-back, and that kernel's fused form, which also copies its frames
// (cfws_deserialize_batch). The layout rows are in cfws_kernels.h. The scan
// kernels and deserialize_plan_apply_kernel, which HTTP/2 and the indexing
// launch too, are defined here (namespace cfws_rt) and declared there.
#include "cfws_kernels.h"

namespace {

// A/B knob: dynamic LDS the WS plan kernels reserve (CFWS_PLAN_LDS; default 0)
uint32_t plan_lds_bytes()
{
    static const int64_t v = env_knob("CFWS_PLAN_LDS", 0);
    return (uint32_t)(v > 65536 ? 65536 : v);
}

// WS serialize's in-region edge chunks (general_region_ser_edges) need every
// frame's payload at 80..CFWS_SER_INREG_MAX bytes and 16-aligned in the payload
// arena (3,584: 2 to 3.5 KiB frames 1.5-8 % faster in-region, 4 KiB 5 % slower;
// profiles/r04/inreg_bound_ab/).
#ifndef CFWS_SER_INREG_MAX
#define CFWS_SER_INREG_MAX 3584
#endif
// general_region_ser_edges carries a header as two words: 16-bit lengths
static_assert(CFWS_SER_INREG_MAX <= 65535, "in-region headers are at most 8 bytes");
__device__ __forceinline__ bool ser_inreg_frame_ok(uint64_t len, uint32_t payload_off_lo)
{
    return len >= 80 && len <= CFWS_SER_INREG_MAX && (payload_off_lo & 15u) == 0;
}

__global__ void __launch_bounds__(kThreads)
serialize_plan_reduce_kernel(cfws_frame_desc_t* __restrict__ desc, uint64_t* __restrict__ vals,
                             uint64_t n, uint64_t* __restrict__ partials, uint32_t* __restrict__ inreg_flag)
{
    __shared__ uint64_t s_wave[kWaves];
    if (blockIdx.x == 0 && threadIdx.x == 0) *inreg_flag = 0u;    // the apply kernel ORs into it
    const uint64_t b0 = uint64_t(blockIdx.x) * kPlanBlock;
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kPlanItems; ++k) {
        const uint64_t f = b0 + uint64_t(k) * kThreads + threadIdx.x;
        if (f < n) {
            const uint64_t len = desc[f].payload_size;
            const uint32_t hs = header_size_of(len, desc[f].mask != 0);
            desc[f].header_size = (uint8_t)hs;
            vals[f] = ser_wire_bytes(hs, len);
            sum += ser_wire_bytes(hs, len);
        }
    }
    uint64_t total;
    block_exclusive_scan(sum, s_wave, &total);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kThreads)
serialize_plan_apply_kernel(cfws_frame_desc_t* __restrict__ desc, uint64_t* __restrict__ vals,
                            uint64_t n, const uint64_t* __restrict__ partials, uint64_t nb,
                            uint32_t self_scan, uint64_t* __restrict__ hdr, uint64_t capacity,
                            uint32_t* __restrict__ map, uint64_t* __restrict__ user_total,
                            uint32_t* __restrict__ inreg_flag)
{
    __shared__ uint64_t s_wave[kWaves];
    uint64_t prefix, g;
    plan_prefix(partials, nb, self_scan, hdr + 3, s_wave, prefix, g);
    const uint64_t total = g < capacity ? g : capacity;
    const uint64_t i0 = uint64_t(blockIdx.x) * kPlanBlock + uint64_t(threadIdx.x) * kPlanItems;
    uint64_t v[kPlanItems];
    uint64_t sum = 0;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < kPlanItems; ++k) {
        v[k] = (i0 + k < n) ? vals[i0 + k] : 0;
        sum += v[k];
    }
    uint64_t tot;
    uint64_t run = block_exclusive_scan(sum, s_wave, &tot) + prefix;
#pragma unroll
    for (int k = 0; k < kPlanItems; ++k) {
        const uint64_t f = i0 + k;
        if (f < n) {
            vals[f] = run;
            bad |= !ser_inreg_frame_ok(desc[f].payload_size, (uint32_t)desc[f].payload_off);
            desc[f].wire_off = run;
            map_range(run, run + v[k], f, total, map);
            if (f == n - 1) {
                map[(total + kRegion - 1) / kRegion] = (uint32_t)f;
                ser_epilogue(hdr, user_total, total, g, self_scan);
            }
        }
        run += v[k];
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(inreg_flag, 1u);
}

// Header decode at index[f] against its data size (the whole buffer, or the
// frame's own message: co_http2_stream_receive_ws_frame passes the pooled
// DATA, co_ws_http2_extension.c:144-146). Layout sizes: vals0 = data (or
// every frame without reassembly), vals1 = control frames when reassembling.
__global__ void __launch_bounds__(kThreads)
deserialize_plan_reduce_kernel(const uint8_t* __restrict__ wire, uint64_t wire_size_all,
                               const uint64_t* __restrict__ index, const uint64_t* __restrict__ ends,
                               uint64_t n, uint64_t max_payload, uint64_t align, uint32_t reassemble,
                               cfws_frame_desc_t* __restrict__ desc, int32_t* __restrict__ status,
                               uint64_t* __restrict__ vals0, uint64_t* __restrict__ vals1,
                               uint64_t* __restrict__ partials0, uint64_t* __restrict__ partials1)
{
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t b0 = uint64_t(blockIdx.x) * kPlanBlock;
    uint64_t sum0 = 0, sum1 = 0;
#pragma unroll
    for (int k = 0; k < kPlanItems; ++k) {
        const uint64_t f = b0 + uint64_t(k) * kThreads + threadIdx.x;
        if (f >= n) continue;
        const uint64_t wire_size = ends && ends[f] < wire_size_all ? ends[f] : wire_size_all;
        cfws_frame_desc_t d;
        const int32_t st = parse_ws_header(wire, wire_size, index[f], max_payload, d);
        desc[f] = d;
        status[f] = st;
        if (reassemble) {
            const uint64_t len = de_slot_bytes(st, d.payload_size, 1);      // packed
            const bool ctl = is_control(d.opcode);
            vals0[f] = ctl ? 0 : len;
            vals1[f] = ctl ? len : 0;
            sum0 += ctl ? 0 : len;
            sum1 += ctl ? len : 0;
        } else {
            const uint64_t v = de_slot_bytes(st, d.payload_size, align);
            vals0[f] = v;
            sum0 += v;
        }
    }
    uint64_t total;
    block_exclusive_scan(sum0, s_wave, &total);
    if (threadIdx.x == 0) partials0[blockIdx.x] = total;
    if (reassemble) {
        block_exclusive_scan(sum1, s_wave, &total);
        if (threadIdx.x == 0) partials1[blockIdx.x] = total;
    }
}

// Single-pass plans (plan_lookback): the reduce and apply kernels above in
// one launch, for plans of more than kSelfScanBlocks blocks (no scan launch,
// no second read of the sizes). A block takes kThreads x kSingleItems frames,
// each wave a contiguous kSingleItems x 64 of them (item k, lane l: frame k * 64 + l of
// the wave's run, so every load is coalesced): the look-back's cost is a
// device-scope round trip per 64 blocks, and 16 K blocks of 256 frames spent
// 232 us on it for 4 M frames. With a capacity cut the region map clips at
// the capacity itself: a frame's range ends at or below the grand total, so
// that is the same clip as at min(total, capacity).
// The serialize plan reads every descriptor whole and writes it back whole
// (8 frames per thread for the registers): a descriptor line then leaves L2
// fully written, and the payload offset is not fetched a second time. The
// round-4 A/B against reading the sizes first and writing two fields after
// the look-back (16 frames per thread): at 16 M x 256 B 0.54 GB read per plan
// instead of 1.08, the same 0.68 GB written, the same time (328 against
// 331 us; profiles/r04/plan_ab.json); with the packed look-back, the two-field
// form at 4, 8 or 16 frames per thread (down to 122 VGPRs, 4 waves per SIMD)
// was 0.2-1.9 % slower per step at 256 B and 1 KiB (profiles/r04/plan_lite_ab.json).
// (CFWS_SINGLE_ITEMS_SER, CFWS_SER_PLAN_THREADS: cfws_kernels.h, with ser_inreg_flag)
#ifndef CFWS_SINGLE_ITEMS_DESER
#define CFWS_SINGLE_ITEMS_DESER 8
#endif
constexpr int kSingleItemsDeser = CFWS_SINGLE_ITEMS_DESER;
// Threads per block of the single-pass plans (serialize, deserialize) and
// of the fused deserialize. A block's look-back waits on the inclusive
// frontier, which advances 64 blocks per poll round trip (about 2.3 us
// under load: tools/plan_trace.py timed the serialize plan's blocks at
// 5.2 us of loads, 6.6 us of look-back, 4.0 us of stores, 465 resident),
// so a block of more frames moves the frontier further per round trip. On
// 16 M x 256 B: serialize plan 305 -> 274 us at 512 threads (1,024: 128
// VGPRs, spills); fused receive 1.95 -> 1.79 ms at 1,024 threads (512:
// 1.87); step 3.84-3.87 -> 3.65-3.66 ms. 1 KiB and 3 KiB unchanged, and the
// receive plan at 512 / 1,024 threads too (profiles/r05/plan_blocks_ab/).
#ifndef CFWS_DE_PLAN_THREADS
#define CFWS_DE_PLAN_THREADS 256
#endif
#ifndef CFWS_FUSED_THREADS
#define CFWS_FUSED_THREADS 1024
#endif
constexpr int kDePlanThreads = CFWS_DE_PLAN_THREADS;
constexpr int kFusedThreads = CFWS_FUSED_THREADS;

// ---- single-pass plans (more than kSelfScanBlocks blocks) --------------------
// A plan of many blocks scans its block sums with a decoupled look-back
// instead of a scan launch and a second pass over the frames: each block
// takes a ticket (so every lower ticket is already running), publishes its
// sum (flag 1), finds its exclusive prefix from the words of the blocks
// below it, 64 at a time, and publishes the inclusive prefix (flag 2). A
// block's flag and value are one 64-bit word (value << 2 | flag: sums below
// 2^62 bytes, far above any arena), stored and
// loaded whole by device-scope atomics (coherent across the XCDs' L2s by
// themselves), so a reader never sees a flag without its value and nothing
// has to be ordered: a publish is one store the block does not wait for, a
// poll one load. (The first form kept flags and values apart: each publish
// waited for its value's store before the flag's, and each poll loaded the
// value after the flag -- two more round trips per block, which under a
// saturated memory system bound the plans by look-back latency. Release /
// acquire fences would write back and invalidate the whole L2 at each
// publish and each poll: measured 2 ms per plan on 16 K blocks.)
//
// The words live in the workspace's look area after the u32 ticket (word
// 0), the u32 flag words 1..sb + 1 that some plans leave for their execute,
// and padding to 8 bytes (look_state_index, look_bytes); all of it is zeroed
// before the launch.

__device__ __forceinline__ uint64_t* look_states(uint32_t* look)
{
    return reinterpret_cast<uint64_t*>(look + look_state_index(gridDim.x));
}

__device__ __forceinline__ uint32_t plan_ticket(uint32_t* look, uint32_t* s_bid)
{
    if (threadIdx.x == 0) *s_bid = __hip_atomic_fetch_add(look, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    return *s_bid;
}

// Wave 0 of block b (every lane): b's exclusive prefix, after publishing
// `total` as b's sum; then b's inclusive prefix is published. Blocks below
// b that have not published yet (flag 0) hold a lower ticket, so they are
// running and publish without waiting on anyone.
__device__ __forceinline__ uint64_t plan_lookback(uint32_t b, uint64_t total, uint64_t* state)
{
    const uint32_t lane = threadIdx.x & 63u;
    if (b == 0) {
        if (lane == 0) __hip_atomic_store(&state[0], total << 2 | 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return 0;
    }
    if (lane == 0) __hip_atomic_store(&state[b], total << 2 | 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint64_t excl = 0;
    int64_t hi = (int64_t)b - 1;                      // window [hi - 63, hi], lane l: hi - l
    while (true) {
        const int64_t i = hi - (int64_t)lane;
        uint64_t w = 2u;                              // below block 0: an inclusive 0
        if (i >= 0) {
            do {
                w = __hip_atomic_load(&state[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((w & 3u) == 0u) __builtin_amdgcn_s_sleep(2);
            } while ((w & 3u) == 0u);
        }
        // the nearest inclusive prefix (lowest lane) ends the walk
        const uint64_t pm = __ballot((w & 3u) == 2u);
        const uint32_t stop = pm ? (uint32_t)__builtin_ctzll(pm) : 64u;
        uint64_t c = lane <= stop ? w >> 2 : 0;
#pragma unroll
        for (uint32_t o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
        excl += c;
        if (pm) break;
        hi -= 64;
    }
    if (lane == 0) __hip_atomic_store(&state[b], (excl + total) << 2 | 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return excl;
}

// The wave-exclusive prefixes of v[k] in frame order (k-major), and the
// wave's total.
template <int kSingleItems>
__device__ __forceinline__ uint64_t wave_scan_items(const uint64_t (&v)[kSingleItems], uint64_t (&ex)[kSingleItems])
{
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t run = 0;
#pragma unroll
    for (int k = 0; k < kSingleItems; ++k) {
        uint64_t inc = v[k];
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint64_t y = __shfl_up(inc, o, 64);
            if (lane >= o) inc += y;
        }
        ex[k] = run + inc - v[k];
        run += __shfl(inc, 63, 64);
    }
    return run;
}

// This block's exclusive prefix from the look-back, plus each wave's offset
// within the block (s_wave: the waves' totals).
template <int kNW = kWaves>
__device__ __forceinline__ uint64_t single_block_prefix(uint32_t b, uint64_t wave_total, uint64_t* s_wave,
                                                        uint64_t* s_prefix, uint32_t* look)
{
    const uint32_t wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) s_wave[wid] = wave_total;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)kNW; ++w) {
        if (w < wid) before += s_wave[w];
        all += s_wave[w];
    }
    if (wid == 0) {
        const uint64_t pre = plan_lookback(b, all, look_states(look));
        if (threadIdx.x == 0) *s_prefix = pre;
    }
    __syncthreads();
    return *s_prefix + before;
}

// CFWS_PLAN_TRACE builds (tools/plan_trace.py; never the shipped library):
// per block ticket, wall-clock stamps at the ticket, after the loads and
// the block scan, after the look-back, at the end.
#ifndef CFWS_PLAN_TRACE
#define CFWS_PLAN_TRACE 0
#endif
#if CFWS_PLAN_TRACE
constexpr uint32_t kTraceBlocks = 1u << 16;
__device__ uint64_t g_plan_trace[kTraceBlocks][4];
#define PLAN_STAMP(b, i)                                                                       \
    do {                                                                                       \
        if (threadIdx.x == 0 && (b) < kTraceBlocks) g_plan_trace[(b)][(i)] = wall_clock64();   \
    } while (0)
#else
#define PLAN_STAMP(b, i) do {} while (0)
#endif

template <int kBT>
__global__ void __launch_bounds__(kBT)
serialize_plan_single_kernel(cfws_frame_desc_t* __restrict__ desc, uint64_t* __restrict__ offs, uint64_t n,
                             uint32_t* __restrict__ look, uint64_t* __restrict__ hdr, uint64_t capacity,
                             uint32_t* __restrict__ map, uint64_t* __restrict__ user_total)
{
    __shared__ uint64_t s_wave[kBT / 64];
    __shared__ uint64_t s_prefix;
    __shared__ uint32_t s_bid;
    constexpr int kSingleItems = kSingleItemsSer;
    static_assert(kSingleItems <= 16, "4-bit header sizes in one word");
    constexpr uint64_t kSingleFrames = uint64_t(kBT) * kSingleItems;
    const uint32_t b = plan_ticket(look, &s_bid);
    PLAN_STAMP(b, 0);
    const uint64_t f0 = uint64_t(b) * kSingleFrames + uint64_t(threadIdx.x >> 6) * (64 * kSingleItems) +
                        (threadIdx.x & 63u);
    uint64_t v[kSingleItems], ex[kSingleItems];
    uint64_t hsp = 0;                                  // 4 bits per item: header sizes (2..14)
    // every item's loads in one round (frames past n read frame n - 1's:
    // a branch per item made it a round trip per item)
    uint64_t len[kSingleItems];
    uint32_t msk[kSingleItems];
    bool bad = false;                                  // a frame outside ser_inreg_frame_ok
    uint64_t poff[kSingleItems], w3[kSingleItems];
#pragma unroll
    for (int k = 0; k < kSingleItems; ++k) {
        const uint64_t f = f0 + uint64_t(k) * 64, fc = f < n ? f : n - 1;
        const DescWords d = load_desc(desc, (uint32_t)fc);
        poff[k] = d.payload_off;
        len[k] = d.payload_size;
        w3[k] = d.w3;
        msk[k] = d.mask();
    }
#pragma unroll
    for (int k = 0; k < kSingleItems; ++k)
        bad |= f0 + uint64_t(k) * 64 < n && !ser_inreg_frame_ok(len[k], (uint32_t)poff[k]);
#pragma unroll
    for (int k = 0; k < kSingleItems; ++k) {
        const uint64_t f = f0 + uint64_t(k) * 64;
        const uint32_t hs = header_size_of(len[k], msk[k] != 0);
        hsp |= uint64_t(hs) << (4 * k);
        v[k] = f < n ? ser_wire_bytes(hs, len[k]) : 0;
    }
    const uint64_t wt = wave_scan_items(v, ex);
    PLAN_STAMP(b, 1);
    const uint64_t pre = single_block_prefix<kBT / 64>(b, wt, s_wave, &s_prefix, look);
    PLAN_STAMP(b, 2);
#pragma unroll
    for (int k = 0; k < kSingleItems; ++k) {
        const uint64_t f = f0 + uint64_t(k) * 64;
        if (f >= n) continue;
        const uint64_t run = pre + ex[k];
        offs[f] = run;
        const uint32_t hs = (uint32_t)((hsp >> (4 * k)) & 15u);
        // the whole descriptor: the line leaves L2 fully written
        uint64_t* q = reinterpret_cast<uint64_t*>(desc) + 4 * f;
        q[0] = poff[k];
        q[1] = run;
        q[2] = len[k];
        q[3] = (w3[k] & ~(uint64_t(0xff) << 56)) | uint64_t(hs) << 56;
        map_range(run, run + v[k], f, capacity, map);
        if (f == n - 1) {
            const uint64_t g = run + v[k], t = g < capacity ? g : capacity;
            map[(t + kRegion - 1) / kRegion] = (uint32_t)f;
            ser_epilogue(hdr, user_total, t, g);
        }
    }
    // in-region edges only when every frame qualifies (look[gridDim.x + 1],
    // zeroed with the tickets)
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(look + gridDim.x + 1, 1u);
    PLAN_STAMP(b, 3);
}

// ---- the fused deserialize: plan and copy in one pass ------------------------
// For batches of small frames at 16-byte slots (cfws_deserialize_batch),
// each block of the single-pass plan copies its own frames once their
// offsets are known, so the header lines the plan reads are the lines the
// copy streams next (one pass over the wire instead of two: the plan alone
// re-read 0.5 GB of 128-byte lines for 4 M x 1 KiB frames, 2.2 GB for
// 16 M x 256 B). Wave w copies the frames it parsed (item k, lane l: frame
// k * 64 + l of its run) with fused_item (cfws_kernels.h, shared with the
// slot receive): every slot byte below the pass total is written once,
// payload or zero, as the plan + execute write it.
//
// The fused kernel's occupancy hint, stated as what it is: workgroups of
// kFusedThreads per CU (__launch_bounds__' second argument). 1 at 1024
// threads = 16 waves per CU, 4 per SIMD: the register budget every fused
// measurement in DESIGN.md ran with (the hint used to be written as
// 5 * 256 / kBT, which truncated to this same 1).
#ifndef CFWS_FUSED_MIN_BLOCKS_PER_CU
#define CFWS_FUSED_MIN_BLOCKS_PER_CU 1
#endif
constexpr int kFusedMinBlocksPerCU = CFWS_FUSED_MIN_BLOCKS_PER_CU;
static_assert(kFusedMinBlocksPerCU >= 1, "the fused kernel's occupancy hint must be at least 1");

// deserialize_plan_reduce_kernel + deserialize_plan_apply_kernel in one
// launch, without reassembly (its control-frame pass starts at the data
// pass's grand total, which no block knows before the last one). The
// descriptors are written as parsed, their payload offsets (and the
// capacity rule's status) once the offsets are known. kCopy: the fused
// deserialize (above): each block then copies its frames into `out`; no
// offsets or region map are written (no execute follows).
#ifndef CFWS_FUSED_ITEMS
#define CFWS_FUSED_ITEMS 2
#endif
constexpr int kFusedItems = CFWS_FUSED_ITEMS;   // frames per thread in the fused form (registers)

template <bool kCopy, int kBT>
__global__ void __launch_bounds__(kBT, kCopy ? kFusedMinBlocksPerCU : 1)
deserialize_plan_single_kernel(const uint8_t* __restrict__ wire, uint64_t wire_size_all,
                               const uint64_t* __restrict__ index, const uint64_t* __restrict__ ends,
                               uint64_t n, uint64_t max_payload, uint64_t align,
                               cfws_frame_desc_t* __restrict__ desc, int32_t* __restrict__ status,
                               uint64_t* __restrict__ offs, uint32_t* __restrict__ look,
                               uint64_t* __restrict__ hdr, uint64_t capacity, uint32_t* __restrict__ map,
                               uint64_t* __restrict__ user_total, uint8_t* __restrict__ out = nullptr)
{
    __shared__ uint64_t s_wave[kBT / 64];
    __shared__ uint64_t s_prefix;
    __shared__ uint32_t s_bid;
    constexpr int kSingleItems = kCopy ? kFusedItems : kSingleItemsDeser;
    constexpr uint64_t kSingleFrames = uint64_t(kBT) * kSingleItems;
    const uint32_t b = plan_ticket(look, &s_bid);
    PLAN_STAMP(b, 0);
    const uint64_t f0 = uint64_t(b) * kSingleFrames + uint64_t(threadIdx.x >> 6) * (64 * kSingleItems) +
                        (threadIdx.x & 63u);
    // each descriptor is written once, whole, with its offset: the parsed
    // fields wait in registers (wire_off, payload_size, the last word)
    uint64_t v[kSingleItems], ex[kSingleItems], wo[kSingleItems], ps[kSingleItems], w3[kSingleItems];
    int32_t sts[kSingleItems];
    // the loads of all items first, in two rounds (starts and ends, then
    // every header's 16 bytes, below), then the parses: a
    // header per round trip serialized the wave (24 round trips for 8
    // items). Frames past n load frame n - 1's entries: no branch in a round.
    uint64_t sx[kSingleItems], sz[kSingleItems];
#pragma unroll
    for (int k = 0; k < kSingleItems; ++k) {
        const uint64_t f = f0 + uint64_t(k) * 64, fc = f < n ? f : n - 1;
        sx[k] = index[fc];
        sz[k] = wire_size_all;
    }
    if (ends) {
#pragma unroll
        for (int k = 0; k < kSingleItems; ++k) {
            const uint64_t f = f0 + uint64_t(k) * 64, fc = f < n ? f : n - 1;
            const uint64_t e = ends[fc];
            sz[k] = e < wire_size_all ? e : wire_size_all;
        }
    }
    // every header from one 16-byte load at its first byte (unaligned: the
    // part's unaligned access mode; one request, or two when the 16 bytes
    // cross a line), clamped to the buffer's last 16 bytes instead of
    // branching on the bytes available; a header with fewer than 16 bytes
    // after it in the buffer is parsed by the loads of parse_ws_header
    const bool b16 = wire_size_all >= 16;
    const uint64_t lastu = wire_size_all - 16;
    uint4 hw[kSingleItems];
    if (b16) {
#pragma unroll
        for (int k = 0; k < kSingleItems; ++k) hw[k] = ld16u(wire + (sx[k] < lastu ? sx[k] : lastu));
    }
#pragma unroll
    for (int k = 0; k < kSingleItems; ++k) {
        const uint64_t f = f0 + uint64_t(k) * 64;
        v[k] = 0;
        if (f < n) {
            const uint64_t wire_size = sz[k];
            cfws_frame_desc_t d;
            const uint64_t s0 = sx[k];
            if (b16 && s0 <= lastu) {
                const uint64_t avail = s0 <= wire_size ? wire_size - s0 : 0;
                const uint4 W = hw[k];
                const uint32_t w[4] = {W.x, W.y, W.z, W.w};
                sts[k] = parse_ws_header_regs(w, avail, max_payload, d);
                d.wire_off = s0;
            } else {
                sts[k] = parse_ws_header(wire, wire_size, s0, max_payload, d);
            }
            wo[k] = d.wire_off;
            ps[k] = d.payload_size;
            w3[k] = (uint64_t)d.mask_key | (uint64_t)d.fin << 32 | (uint64_t)d.opcode << 40 |
                    (uint64_t)d.mask << 48 | (uint64_t)d.header_size << 56;
            v[k] = de_slot_bytes(sts[k], d.payload_size, align);
        }
    }
    const uint64_t wt = wave_scan_items(v, ex);
    PLAN_STAMP(b, 1);
    const uint64_t pre = single_block_prefix<kBT / 64>(b, wt, s_wave, &s_prefix, look);
    PLAN_STAMP(b, 2);
    // kCopy: what the copy needs per item, compact (the parse's arrays die here)
    uint64_t c_run[kSingleItems], c_src[kSingleItems];
    uint32_t c_len[kSingleItems], c_nb[kSingleItems], c_key[kSingleItems];
#pragma unroll
    for (int k = 0; k < kSingleItems; ++k) {
        const uint64_t f = f0 + uint64_t(k) * 64;
        c_run[k] = c_src[k] = 0;
        c_len[k] = c_nb[k] = c_key[k] = 0;
        if (f >= n) continue;
        const uint64_t run = pre + ex[k];
        if (!kCopy) offs[f] = run;
        uint64_t* q = reinterpret_cast<uint64_t*>(desc) + 4 * f;
        q[0] = run;
        q[1] = wo[k];
        q[2] = ps[k];
        q[3] = w3[k];
        const int32_t st = de_capacity_rule(sts[k], ps[k], run, capacity);
        status[f] = st;
        if (kCopy) {
            // slot bytes below the capacity (every slot ends at or below the
            // grand total, so that is the pass total's cut); the payload
            // only for a frame still COMPLETE, zeros otherwise
            const uint64_t end = run + v[k] < capacity ? run + v[k] : capacity;
            const uint64_t nbk = end > run ? end - run : 0;
            c_run[k] = run;
            c_src[k] = wo[k] + (w3[k] >> 56);
            c_nb[k] = nbk < 0xffffffffull ? (uint32_t)nbk : 0xffffffffu;
            c_len[k] = st == CFWS_PARSE_COMPLETE ? (uint32_t)(ps[k] < nbk ? ps[k] : nbk) : 0u;
            c_key[k] = (w3[k] >> 48) & 0xffu ? (uint32_t)w3[k] : 0u;
        } else {
            map_range(run, run + v[k], f, capacity, map);
        }
        if (f == n - 1) {
            const uint64_t g = run + v[k], t = g < capacity ? g : capacity;
            if (!kCopy) map[(t + kRegion - 1) / kRegion] = (uint32_t)f;
            de_epilogue(hdr, user_total, t, g);
        }
    }
    if (!kCopy) {
#if CFWS_PLAN_TRACE
        __syncthreads();
        PLAN_STAMP(b, 3);
#endif
        return;
    }
    // the copy: every slot byte below the pass total min(grand total,
    // capacity), cut at the capacity itself (above)
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int k = 0; k < kSingleItems; ++k)
        fused_item(wire, out, capacity, c_run[k], c_src[k], c_len[k], c_nb[k], c_key[k], lane);
#if CFWS_PLAN_TRACE
    __syncthreads();
    PLAN_STAMP(b, 3);
#endif
}

// Single-pass plans above kSelfScanBlocks blocks (CFWS_PLAN_SINGLE=0: the
// reduce / scan / apply launches everywhere; A/B knob).
bool plan_single()
{
    static const bool v = env_knob("CFWS_PLAN_SINGLE", 1) != 0;
    return v;
}

// Zero the look area, then launch(look, sb): a single-pass kernel over sb
// blocks of kBT threads x kItems frames.
template <int kBT, int kItems, typename Launch>
int launch_single_pass(const char* what, const WsLayout& L, void* ws, uint64_t n, hipStream_t st, Launch launch)
{
    uint32_t* look = ws_ptr<uint32_t>(ws, L.look);
    const uint32_t sb = grid_for(n, uint64_t(kBT) * kItems);
    if (hipMemsetAsync(look, 0, look_bytes(sb), st) != hipSuccess) return launch_check(what);
    launch(look, sb);
    return launch_check(what);
}

}  // namespace

namespace cfws_rt {

// ---- the kernels other units launch too (declared in cfws_kernels.h) --------

__global__ void __launch_bounds__(kThreads)
scan_reduce_kernel(const uint64_t* __restrict__ vals, uint64_t n, uint64_t* __restrict__ partials)
{
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t b0 = uint64_t(blockIdx.x) * kScanBlock;
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        const uint64_t i = b0 + uint64_t(k) * kThreads + threadIdx.x;
        if (i < n) sum += vals[i];
    }
    uint64_t total;
    block_exclusive_scan(sum, s_wave, &total);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// One workgroup's exclusive scan of nb block sums, in place; *grand gets the
// total. A step takes kThreads x kPartialItems sums, kPartialItems
// consecutive ones per thread with all their loads in flight: the 16,384
// sums of a 4 M-frame plan in one step, 19 us (one sum per thread per step:
// 64 dependent steps, 46 us; 16 per thread through LDS with coalesced loads
// and stores: 4 steps, 29-35 us -- each step's round trip costs more than
// the strided access).
constexpr int kPartialItems = 64;

__device__ __forceinline__ void scan_partials_block(uint64_t* __restrict__ partials, uint64_t nb,
                                                    uint64_t* __restrict__ grand, uint64_t* s_wave)
{
    uint64_t carry = 0;
    for (uint64_t b = 0; b < nb; b += uint64_t(kThreads) * kPartialItems) {
        const uint64_t i0 = b + uint64_t(threadIdx.x) * kPartialItems;
        uint64_t v[kPartialItems];
        uint64_t sum = 0;
#pragma unroll
        for (int k = 0; k < kPartialItems; ++k) {
            v[k] = i0 + k < nb ? partials[i0 + k] : 0;
            sum += v[k];
        }
        uint64_t tot;
        uint64_t run = block_exclusive_scan(sum, s_wave, &tot) + carry;
#pragma unroll
        for (int k = 0; k < kPartialItems; ++k) {
            if (i0 + k < nb) partials[i0 + k] = run;
            run += v[k];
        }
        carry += tot;
    }
    if (threadIdx.x == 0) *grand = carry;
}

__global__ void __launch_bounds__(kThreads)
scan_partials_kernel(uint64_t* __restrict__ partials, uint64_t nb, uint64_t* __restrict__ grand)
{
    __shared__ uint64_t s_wave[kWaves];
    scan_partials_block(partials, nb, grand, s_wave);
}

__global__ void __launch_bounds__(kThreads)
scan_partials2_kernel(uint64_t* __restrict__ partials0, uint64_t* __restrict__ partials1, uint64_t nb,
                      uint64_t* __restrict__ grand0, uint64_t* __restrict__ grand1)
{
    __shared__ uint64_t s_wave[kWaves];
    scan_partials_block(blockIdx.x ? partials1 : partials0, nb, blockIdx.x ? grand1 : grand0, s_wave);
}

__global__ void __launch_bounds__(kThreads)
scan_apply_kernel(uint64_t* __restrict__ vals, uint64_t n, const uint64_t* __restrict__ partials)
{
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t i0 = uint64_t(blockIdx.x) * kScanBlock + uint64_t(threadIdx.x) * kScanItems;
    uint64_t v[kScanItems];
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        v[k] = (i0 + k < n) ? vals[i0 + k] : 0;
        sum += v[k];
    }
    uint64_t tot;
    uint64_t run = block_exclusive_scan(sum, s_wave, &tot) + partials[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        if (i0 + k < n) vals[i0 + k] = run;
        run += v[k];
    }
}

int run_scan(uint64_t* vals, uint64_t n, uint64_t* partials, uint64_t* grand, hipStream_t st)
{
    const uint32_t nb = grid_for(n, kScanBlock);
    scan_reduce_kernel<<<nb, kThreads, 0, st>>>(vals, n, partials);
    scan_partials_kernel<<<1, kThreads, 0, st>>>(partials, nb, grand);
    scan_apply_kernel<<<nb, kThreads, 0, st>>>(vals, n, partials);
    return launch_check("scan");
}

__global__ void __launch_bounds__(kThreads)
deserialize_plan_apply_kernel(cfws_frame_desc_t* __restrict__ desc, int32_t* __restrict__ status,
                              uint64_t* __restrict__ vals0, uint64_t* __restrict__ vals1, uint64_t n,
                              const uint64_t* __restrict__ partials0,
                              const uint64_t* __restrict__ partials1, uint64_t nb,
                              uint32_t self_scan, uint64_t* __restrict__ hdr,
                              uint64_t capacity, uint32_t reassemble, uint32_t* __restrict__ map0,
                              uint32_t* __restrict__ map1, uint64_t* __restrict__ user_total)
{
    __shared__ uint64_t s_wave[kWaves];
    uint64_t pre0, pre1 = 0, g0, g1 = 0;
    plan_prefix(partials0, partials1, nb, self_scan, hdr + 3, hdr + 4, reassemble, s_wave, pre0, g0, pre1, g1);
    const uint64_t t0 = g0 < capacity ? g0 : capacity;
    const uint64_t room1 = capacity - t0;
    const uint64_t t1 = g1 < room1 ? g1 : room1;
    const uint64_t i0 = uint64_t(blockIdx.x) * kPlanBlock + uint64_t(threadIdx.x) * kPlanItems;
    uint64_t v0[kPlanItems], v1[kPlanItems];
    uint64_t s0 = 0, s1 = 0;
#pragma unroll
    for (int k = 0; k < kPlanItems; ++k) {
        v0[k] = (i0 + k < n) ? vals0[i0 + k] : 0;
        v1[k] = (reassemble && i0 + k < n) ? vals1[i0 + k] : 0;
        s0 += v0[k];
        s1 += v1[k];
    }
    uint64_t tot;
    uint64_t run0 = block_exclusive_scan(s0, s_wave, &tot) + pre0;
    uint64_t run1 = 0;
    if (reassemble) run1 = block_exclusive_scan(s1, s_wave, &tot) + pre1;
#pragma unroll
    for (int k = 0; k < kPlanItems; ++k) {
        const uint64_t f = i0 + k;
        if (f < n) {
            vals0[f] = run0;
            const bool ctl = reassemble && is_control(desc[f].opcode);
            const uint64_t off = ctl ? g0 + run1 : run0;
            desc[f].payload_off = off;
            const int32_t st = status[f];
            if (de_capacity_rule(st, desc[f].payload_size, off, capacity) != st)
                status[f] = CFWS_ERROR_OUT_OF_MEMORY;
            map_range(run0, run0 + v0[k], f, t0, map0);
            if (reassemble) {
                vals1[f] = run1;
                map_range(run1, run1 + v1[k], f, t1, map1);
            }
            if (f == n - 1) {
                map0[(t0 + kRegion - 1) / kRegion] = (uint32_t)f;
                if (reassemble) map1[(t1 + kRegion - 1) / kRegion] = (uint32_t)f;
                hdr[0] = t0;
                hdr[1] = t1;
                hdr[2] = t0;
                if (self_scan) {
                    hdr[3] = g0;
                    if (reassemble) hdr[4] = g1;
                }
                if (user_total) *user_total = t0 + t1;
            }
        }
        run0 += v0[k];
        run1 += v1[k];
    }
}

// ---- the deserialize plan and the fused deserialize --------------------------

int deserialize_plan_impl(const void* d_wire, uint64_t wire_size, const uint64_t* d_index,
                          const uint64_t* d_ends, size_t n, uint64_t max_payload, uint32_t align,
                          uint32_t flags, cfws_frame_desc_t* d_desc, int32_t* d_status, uint64_t cap,
                          uint64_t* d_total, void* ws, size_t ws_size, void* stream)
{
    if (int rc = check_init()) return rc;
    const ArgCheck c = check_de_plan(d_wire, d_index, n, align, flags, d_desc, d_status, cap, ws, ws_size);
    if (c.code) return set_err(c.code, c.what, hipSuccess);
    const WsLayout L = ws_layout(n, cap);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) return zero_totals(L, ws, d_total, st);
    const uint8_t* wire = static_cast<const uint8_t*>(d_wire);
    const uint32_t reasm = (flags & CFWS_DESERIALIZE_REASSEMBLE) ? 1u : 0u;
    uint64_t* hdr = ws_ptr<uint64_t>(ws, L.hdr);
    uint64_t* offs0 = ws_ptr<uint64_t>(ws, L.offs[0]);
    uint64_t* offs1 = ws_ptr<uint64_t>(ws, L.offs[1]);
    uint64_t* part0 = ws_ptr<uint64_t>(ws, L.partials[0]);
    uint64_t* part1 = ws_ptr<uint64_t>(ws, L.partials[1]);
    const uint32_t nb = grid_for(n, kPlanBlock);
    if (!reasm && nb > kSelfScanBlocks && plan_single())
        return launch_single_pass<kDePlanThreads, kSingleItemsDeser>(
            "deserialize_plan", L, ws, n, st, [&](uint32_t* look, uint32_t sb) {
                deserialize_plan_single_kernel<false, kDePlanThreads><<<sb, kDePlanThreads, 0, st>>>(
                    wire, wire_size, d_index, d_ends, n, max_payload, align, d_desc, d_status, offs0, look, hdr,
                    cap, ws_ptr<uint32_t>(ws, L.map[0]), d_total);
            });
    deserialize_plan_reduce_kernel<<<nb, kThreads, plan_lds_bytes(), st>>>(
        wire, wire_size, d_index, d_ends, n, max_payload, align, reasm, d_desc, d_status, offs0, offs1, part0,
        part1);
    const uint32_t self_scan = nb <= kSelfScanBlocks ? 1u : 0u;
    if (!self_scan)
        scan_partials2_kernel<<<reasm ? 2 : 1, kThreads, 0, st>>>(part0, part1, nb, hdr + 3, hdr + 4);
    deserialize_plan_apply_kernel<<<nb, kThreads, plan_lds_bytes(), st>>>(
        d_desc, d_status, offs0, offs1, n, part0, part1, nb, self_scan, hdr, cap, reasm,
        ws_ptr<uint32_t>(ws, L.map[0]), ws_ptr<uint32_t>(ws, L.map[1]), d_total);
    return launch_check("deserialize_plan");
}

// The timed span starts after the look area's memset: the kernel alone.
int deserialize_fused_impl(const void* d_wire, uint64_t wire_size, const uint64_t* d_index, size_t n,
                           uint64_t max_payload, uint32_t align, cfws_frame_desc_t* d_desc, int32_t* d_status,
                           void* d_payload, uint64_t cap, uint64_t* d_total, void* ws, void* stream)
{
    const WsLayout L = ws_layout(n, cap);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return launch_single_pass<kFusedThreads, kFusedItems>(
        "deserialize_batch(fused)", L, ws, n, st, [&](uint32_t* look, uint32_t sb) {
            const CfwsPassTimer timer(st);
            deserialize_plan_single_kernel<true, kFusedThreads><<<sb, kFusedThreads, 0, st>>>(
                static_cast<const uint8_t*>(d_wire), wire_size, d_index, nullptr, n, max_payload, align, d_desc,
                d_status, nullptr, look, ws_ptr<uint64_t>(ws, L.hdr), cap, nullptr, d_total,
                static_cast<uint8_t*>(d_payload));
        });
}

}  // namespace cfws_rt

extern "C" {

int cfws_serialize_plan(cfws_frame_desc_t* d_desc, size_t n, uint64_t cap, uint64_t* d_total,
                        void* ws, size_t ws_size, void* stream)
{
    const CfwsPassScope pass_scope;
    if (int rc = check_init()) return rc;
    const ArgCheck c = check_ser_plan(d_desc, n, cap, ws, ws_size);
    if (c.code) return set_err(c.code, c.what, hipSuccess);
    const WsLayout L = ws_layout(n, cap);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) return zero_totals(L, ws, d_total, st);
    uint64_t* hdr = ws_ptr<uint64_t>(ws, L.hdr);
    uint64_t* offs = ws_ptr<uint64_t>(ws, L.offs[0]);
    uint64_t* partials = ws_ptr<uint64_t>(ws, L.partials[0]);
    uint32_t* map = ws_ptr<uint32_t>(ws, L.map[0]);
    const uint32_t nb = grid_for(n, kPlanBlock);
    const uint32_t self_scan = nb <= kSelfScanBlocks ? 1u : 0u;
    if (!self_scan && plan_single())
        return launch_single_pass<kSerPlanThreads, kSingleItemsSer>(
            "serialize_plan", L, ws, n, st, [&](uint32_t* look, uint32_t sb) {
                serialize_plan_single_kernel<kSerPlanThreads><<<sb, kSerPlanThreads, 0, st>>>(
                    d_desc, offs, n, look, hdr, cap, map, d_total);
            });
    serialize_plan_reduce_kernel<<<nb, kThreads, plan_lds_bytes(), st>>>(d_desc, offs, n, partials,
                                                                         ser_inreg_flag(L, ws, n));
    if (!self_scan) scan_partials_kernel<<<1, kThreads, 0, st>>>(partials, nb, hdr + 3);
    serialize_plan_apply_kernel<<<nb, kThreads, plan_lds_bytes(), st>>>(
        d_desc, offs, n, partials, nb, self_scan, hdr, cap, map, d_total, ser_inreg_flag(L, ws, n));
    return launch_check("serialize_plan");
}

int cfws_deserialize_plan(const void* d_wire, uint64_t wire_size, const uint64_t* d_index,
                          size_t n, uint64_t max_payload, uint32_t align, uint32_t flags,
                          cfws_frame_desc_t* d_desc, int32_t* d_status, uint64_t cap,
                          uint64_t* d_total, void* ws, size_t ws_size, void* stream)
{
    const CfwsPassScope pass_scope;
    return deserialize_plan_impl(d_wire, wire_size, d_index, nullptr, n, max_payload, align, flags,
                                 d_desc, d_status, cap, d_total, ws, ws_size, stream);
}

#if CFWS_PLAN_TRACE
// tools/plan_trace.py: the last traced launch's stamps, blocks [0, n)
int cfws_debug_plan_trace(void* out, size_t n)
{
    if (n > kTraceBlocks) n = kTraceBlocks;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_plan_trace), n * 4 * sizeof(uint64_t)) == hipSuccess ? 0 : -1;
}
#endif

}  // extern "C"

