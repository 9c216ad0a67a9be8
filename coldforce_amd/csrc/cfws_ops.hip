// cfws_ops.hip -- the codec's smaller device operations and their C ABI
// (include/cfws.h): the multi-connection receive walk, the D2H copy into mapped host memory, the single-buffer XOR of the
// per-frame drop-in and its frame service, the bench's plain device copy,
// and the synthetic fill. (The split header / payload ops: cfws_split.hip.)
#include "cfws_kernels.h"

namespace cfws_rt {

// The kept starts to their places: thread (c, j) copies connection c's j-th
// start (j < kIndexSlots), after the scan turned the counts into firsts.
__global__ void __launch_bounds__(kThreads)
index_place_kernel(const uint64_t* __restrict__ first, const uint64_t* __restrict__ slots,
                   const uint64_t* __restrict__ total, uint64_t n, uint64_t* __restrict__ starts,
                   uint64_t cap)
{
    const uint64_t t = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t c = t / kIndexSlots, j = t % kIndexSlots;
    if (c >= n) return;
    const uint64_t next = c + 1 < n ? first[c + 1] : *total;
    const uint64_t k = next - first[c];
    if (j < k && first[c] + j < cap) starts[first[c] + j] = slots[t];
}

}  // namespace cfws_rt

namespace {

using cfws_rt::index_place_kernel;

// Device -> host copy by a kernel (cfws_copy_to_host): 16-byte stores into
// device-mapped pinned host memory, any alignment on either side. Running the
// D2H leg this way beside an SDMA H2D measured 43 GB/s each way against 28
// for two SDMA copies (tools/pcie_probe2.hip). Each lane writes whole
// destination-aligned 16-byte chunks (source funnel-shifted into place); the
// first and last chunk, which the destination may share with other data,
// byte by byte. The chunk grid starts on a kCopyOutAlign boundary of the
// destination, so each wave's 64 x 16 B of stores is one aligned 1 KiB span
// of PCIe writes wherever the caller's destination starts.
#ifndef CFWS_COPY_OUT_ALIGN
#define CFWS_COPY_OUT_ALIGN 1024
#endif
constexpr uintptr_t kCopyOutAlign = CFWS_COPY_OUT_ALIGN;

__global__ void __launch_bounds__(kThreads)
copy_out_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint64_t n)
{
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst);
    const uintptr_t c0 = d0 & ~(kCopyOutAlign - 1);
    const uint64_t nchunks = (d0 + n - c0 + 15) >> 4;
    const uint32_t ph = (uint32_t)((reinterpret_cast<uintptr_t>(src) - d0) & 15u);
    const uint64_t stride = uint64_t(gridDim.x) * kThreads;
    for (uint64_t c = uint64_t(blockIdx.x) * kThreads + threadIdx.x; c < nchunks; c += stride) {
        const uintptr_t A = c0 + 16 * c;
        if (A >= d0 && A + 16 <= d0 + n) {
            const uint8_t* sp = reinterpret_cast<const uint8_t*>(
                (reinterpret_cast<uintptr_t>(src) + (A - d0)) & ~uintptr_t(15));
            uint4 o = ld16(sp);
            if (ph) o = funnel16(o, ld16(sp + 16), ph);    // holds the chunk's last source byte
            *reinterpret_cast<u32x4*>(A) = u32x4{o.x, o.y, o.z, o.w};
        } else {
            for (uint32_t j = 0; j < 16; ++j) {
                const uintptr_t x = A + j;
                if (x >= d0 && x < d0 + n) *reinterpret_cast<uint8_t*>(x) = src[x - d0];
            }
        }
    }
}

__global__ void __launch_bounds__(kThreads)
xor_mask_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint64_t n,
                uint32_t key, uint32_t phase)
{
    const uint64_t stride = uint64_t(gridDim.x) * kThreads;
    const uint64_t nv = n / 16;
    const uint32_t kr = rotr8(key, phase);
    const bool aligned = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
    const uint64_t tid = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (aligned) {
        for (uint64_t i = tid; i < nv; i += stride) {
            uint4 v = reinterpret_cast<const uint4*>(src)[i];
            xor4(v, kr);
            reinterpret_cast<uint4*>(dst)[i] = v;
        }
        for (uint64_t i = nv * 16 + tid; i < n; i += stride)
            dst[i] = src[i] ^ (uint8_t)(kr >> (8 * (i & 3)));
    } else {
        for (uint64_t i = tid; i < n; i += stride)
            dst[i] = src[i] ^ (uint8_t)(kr >> (8 * (i & 3)));
    }
}

// A plain streaming device-to-device copy: the practical HBM ceiling the
// bench reports the codec against (copy_ceiling). The best bare-copy shape of
// tools/copy_probe.hip (profiles/r01_copy_probe.jsonl): `nt` loads and
// stores, 2 KiB per wave (2 x 16 B per lane), 4 workgroups per CU (an LDS
// reservation of 40,000 B), one chunk per lane per slot, no grid-stride.
constexpr uint32_t kCopyU = 2;

__global__ void __launch_bounds__(kThreads)
stream_copy_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, uint64_t n16)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t base = (uint64_t(blockIdx.x) * kWaves + wave) * (kCopyU * 64) + (threadIdx.x & 63u);
    u32x4 a[kCopyU];
#pragma unroll
    for (uint32_t u = 0; u < kCopyU; ++u)
        if (base + u * 64 < n16) a[u] = __builtin_nontemporal_load(src + base + u * 64);
#pragma unroll
    for (uint32_t u = 0; u < kCopyU; ++u)
        if (base + u * 64 < n16) __builtin_nontemporal_store(a[u], dst + base + u * 64);
}

// The drop-in's frame service (cfws_internal.h): the XOR of a masked frame
// (co_ws_frame.c:93-97 / :234-242) without a launch per frame, for every
// calling thread of a process on one device. One workgroup of 16 waves:
//   * wave 0 dispatches: lane s polls slot s's request word with one
//     coalesced system-scope load per round (all 64 slots' words in 512
//     contiguous bytes of mapped host memory, s_sleep between rounds),
//     cuts each new frame into 4 KiB pieces and hands the pieces to idle
//     worker waves through LDS;
//   * waves 1-15 serve: a worker XORs its piece of its slot's buffer in
//     place (4 chunks per lane, all loads in flight at once, each a PCIe
//     round trip) and releases its stores at system scope; the worker that
//     finishes a frame's last piece writes the slot's done word. A 64 KiB
//     frame is 16 pieces on 15 workers; frames of several threads share
//     them.
// The kernel ends (a) when the stop word is set, (b) after idle_ticks of the
// wall clock without a request, or (c) after life_ticks in all, so that a
// stream sharing its hardware queue never waits behind it for longer
// (GPU_MAX_HW_QUEUES = 4: streams share queues); requests not yet taken stay
// posted for the next launch. After every wave has left the loop, thread 0
// writes the launch's generation to the exit word: from then on this kernel
// touches no slot, and the host may launch the next one.
constexpr uint32_t kServiceThreads = 1024;
constexpr uint32_t kServiceWorkers = kServiceThreads / 64 - 1;     // 15
constexpr uint32_t kServicePiece = 4096;           // bytes per piece: 4 chunks per lane
static_assert(kCfwsServiceSlots == 64, "wave 0's lanes poll the slots");

__device__ __forceinline__ uint64_t sys_load(const uint64_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ void sys_store(uint64_t* p, uint64_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Piece p of a frame of n bytes at buf, XORed in place by one wave (chunk c
// at 16c: key phase 0 for every chunk); the frame's 0-15 tail bytes by the
// wave of its last piece.
__device__ __forceinline__ void service_xor_piece(uint8_t* buf, uint32_t n, uint32_t key, uint32_t p, uint32_t lane)
{
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");      // the frame's bytes, written by the host
    constexpr uint32_t kPer = kServicePiece / 16 / 64;
    const uint32_t nv = n / 16, c0 = p * (kServicePiece / 16);
    u32x4* b = reinterpret_cast<u32x4*>(buf);
    u32x4 v[kPer];
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t c = c0 + k * 64 + lane;
        if (c < nv) v[k] = b[c];
    }
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t c = c0 + k * 64 + lane;
        if (c < nv) b[c] = v[k] ^ key;
    }
    if ((n - 1) / kServicePiece == p && lane < n - nv * 16) {
        const uint32_t i = nv * 16 + lane;
        buf[i] = (uint8_t)(buf[i] ^ (key >> (8 * (i & 3u))));
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");      // the stores, before the piece counts as done
}

__global__ void __launch_bounds__(kServiceThreads)
dropin_service_kernel(uint64_t* ctl, uint8_t* bufs, uint64_t gen, uint64_t idle_ticks, uint64_t life_ticks)
{
    // per worker: its job (slot + 1 | piece << 8; 0 = idle), written by the
    // dispatcher, cleared by the worker; per slot: its request word and the
    // pieces not yet finished (the worker that takes it to 0 writes done)
    __shared__ uint32_t s_job[kServiceWorkers];
    __shared__ uint64_t s_word[kCfwsServiceSlots];
    __shared__ uint32_t s_left[kCfwsServiceSlots];
    __shared__ uint32_t s_exit;
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (threadIdx.x < kServiceWorkers) s_job[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_exit = 0;
    __syncthreads();
    uint64_t* req = ctl + kCfwsServiceReqWord;
    uint64_t* done = ctl + kCfwsServiceDoneWord;
    if (wv == 0) {
        // lane s: the seq last taken for slot s (its done word at launch:
        // every earlier request of the slot was finished), and the pieces of
        // the slot's current frame still to hand out: [next, npieces)
        uint32_t handed = (uint32_t)(sys_load(&done[lane]) >> 48);
        uint32_t next = 0, npieces = 0;
        const uint64_t t_start = (uint64_t)wall_clock64();
        uint64_t t_last = t_start;
        for (;;) {
            const uint64_t now = (uint64_t)wall_clock64();
            const bool retiring = sys_load(&ctl[kCfwsServiceStopWord]) != 0 || now - t_start > life_ticks;
            // a slot takes a new request only when its frame is all handed
            // out; a retiring kernel takes none
            if (!retiring && next == npieces) {
                const uint64_t w = sys_load(&req[lane]);
                if ((uint32_t)(w >> 48) != handed) {
                    // its previous frame is finished: the host posts the next
                    // request only after that frame's done word
                    const uint32_t n = (uint32_t)((w >> 32) & 0xffffu) + 1u;
                    handed = (uint32_t)(w >> 48);
                    next = 0;
                    npieces = (n + kServicePiece - 1) / kServicePiece;
                    s_word[lane] = w;
                    s_left[lane] = npieces;
                    t_last = now;
                }
            }
            // hand out pieces, lowest slot first, to idle workers
            for (uint32_t k = 0; k < kServiceWorkers; ++k) {
                uint64_t want = __ballot(next < npieces);
                if (!want) break;
                if (__hip_atomic_load(&s_job[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0) continue;
                const uint32_t s = (uint32_t)__builtin_ctzll(want);
                const uint32_t p = (uint32_t)__shfl((int)next, (int)s);
                if (lane == 0)
                    __hip_atomic_store(&s_job[k], (s + 1) | p << 8, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (lane == s) ++next;
            }
            bool busy = __ballot(next < npieces) != 0;
            for (uint32_t k = 0; k < kServiceWorkers; ++k)
                busy |= __hip_atomic_load(&s_job[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0;
            // the workers finish the pieces they hold, and every handed-out
            // frame is completed, before the kernel ends
            if (!busy && (retiring || now - t_last > idle_ticks)) break;
            __builtin_amdgcn_s_sleep(2);
        }
        if (lane == 0) __hip_atomic_store(&s_exit, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
        const uint32_t me = wv - 1;
        for (;;) {
            const uint32_t j = __hip_atomic_load(&s_job[me], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (j == 0) {
                if (__hip_atomic_load(&s_exit, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
                __builtin_amdgcn_s_sleep(1);
                continue;
            }
            const uint32_t s = (j & 0xffu) - 1, p = j >> 8;
            const uint64_t w = s_word[s];
            const uint32_t n = (uint32_t)((w >> 32) & 0xffffu) + 1u;
            service_xor_piece(bufs + (uint64_t)s * kCfwsServiceMax, n, (uint32_t)w, p, lane);
            if (lane == 0) {
                // the last piece of the frame: its done word
                if (__hip_atomic_fetch_sub(&s_left[s], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP) == 1u)
                    sys_store(&done[s], w & 0xffff000000000000ull);
                __hip_atomic_store(&s_job[me], 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) sys_store(&ctl[kCfwsServiceExitWord], gen);
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t seed, uint64_t i)
{
    uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void __launch_bounds__(kThreads)
fill_splitmix_kernel(uint8_t* __restrict__ dst, uint64_t n, uint64_t seed, uint64_t word_base)
{
    const uint64_t stride = uint64_t(gridDim.x) * kThreads;
    const uint64_t nv = n / 16;
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < nv; i += stride) {
        const uint64_t a = splitmix64(seed, word_base + 2 * i);
        const uint64_t b = splitmix64(seed, word_base + 2 * i + 1);
        reinterpret_cast<uint4*>(dst)[i] =
            make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
    }
    const uint64_t t = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (t < (n & 15u)) {
        const uint64_t o = nv * 16 + t;
        dst[o] = (uint8_t)(splitmix64(seed, word_base + o / 8) >> (8 * (o & 7)));
    }
}

// ---------------------------------------------------------------------------
// receive-buffer frame indexing (co_ws_server.c:107-169)
// ---------------------------------------------------------------------------

// One connection per thread: the receive loop's walk over buf[begin, end).
// The walk is a chain of dependent header reads (one memory round trip per
// frame), so a connection is one thread and the parallelism is across
// connections (a server's event loop tick holds the receive buffers of
// many). The walk runs once: it counts, records consumed / stop, and keeps
// the first kIndexSlots starts in the connection's workspace slots (where
// they wait for the scan that places them) and where frame kIndexSlots
// starts. After the scan, index_place_kernel copies the kept starts to
// their places, and only connections with more frames than slots walk on
// from there (index_rest_kernel). kIndexSlots, the workspace layout and the
// place pass are shared with the HTTP/2 indexer (cfws_kernels.h).

// One hop of the walk: the header at buf + p of a buffer ending at e, parsed
// into d (header and payload size: p + both is the next start). The
// header's bytes (up to 14) come in one round of independent loads and are
// parsed from registers: one memory round trip per hop, where a
// byte-by-byte parse takes two (the length code, then the rest).
__device__ __forceinline__ int32_t index_hop(const uint8_t* __restrict__ buf, uint64_t p, uint64_t e,
                                             uint64_t max_payload, cfws_frame_desc_t& d)
{
    uint32_t w[4];
    load_span16(buf + p, e - p < 14 ? (uint32_t)(e - p) : 14u, w);
    return parse_ws_header_regs(w, e - p, max_payload, d);
}

__global__ void __launch_bounds__(kThreads)
index_walk_kernel(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ begin,
                  const uint64_t* __restrict__ end, uint64_t n, uint64_t max_payload,
                  uint64_t* __restrict__ first, uint64_t* __restrict__ consumed,
                  int32_t* __restrict__ stop, uint64_t* __restrict__ slots, uint64_t* __restrict__ resume)
{
    const uint64_t c = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (c >= n) return;
    const uint64_t e = end[c];
    uint64_t p = begin[c];
    uint64_t k = 0, r = e;
    uint64_t* my = slots + c * kIndexSlots;
    int32_t st = CFWS_PARSE_COMPLETE;
    while (e > p) {
        if (e - p < 2) { st = CFWS_PARSE_MORE_DATA; break; }
        cfws_frame_desc_t d;
        st = index_hop(buf, p, e, max_payload, d);
        if (st != CFWS_PARSE_COMPLETE) break;
        if (k < kIndexSlots) my[k] = p;
        else if (k == kIndexSlots) r = p;
        ++k;
        p += d.header_size + d.payload_size;
    }
    first[c] = k;
    consumed[c] = p;
    stop[c] = st;
    resume[c] = r;
}

// Connections with more than kIndexSlots frames: the walk on from frame
// kIndexSlots, writing the rest of their starts in place.
__global__ void __launch_bounds__(kThreads)
index_rest_kernel(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ end, uint64_t n,
                  uint64_t max_payload, const uint64_t* __restrict__ first,
                  const uint64_t* __restrict__ total, const uint64_t* __restrict__ resume,
                  uint64_t* __restrict__ starts, uint64_t cap)
{
    const uint64_t c = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (c >= n) return;
    const uint64_t next = c + 1 < n ? first[c + 1] : *total;
    if (next - first[c] <= kIndexSlots) return;
    const uint64_t e = end[c];
    uint64_t p = resume[c];
    for (uint64_t k = first[c] + kIndexSlots; k < next; ++k) {
        cfws_frame_desc_t d;
        (void)index_hop(buf, p, e, max_payload, d);             // COMPLETE: the first walk's frames
        if (k < cap) starts[k] = p;
        p += d.header_size + d.payload_size;
    }
}

// The grid of a grid-stride kernel over n bytes, a 16-byte chunk per thread
// per round: one block per kThreads chunks, at least one, at most `cap`.
uint32_t capped_grid(uint64_t n, uint64_t cap)
{
    const uint64_t blocks = (n / 16 + kThreads - 1) / kThreads;
    return (uint32_t)(blocks == 0 ? 1 : (blocks < cap ? blocks : cap));
}

}  // namespace

int cfws_internal_copy_out(const void* d_src, void* dev_dst, uint64_t n, void* stream)
{
    if (n == 0) return CFWS_OK;
    const uint64_t chunks = (n + kCopyOutAlign) / 16 + 1;
    const uint64_t blocks = (chunks + kThreads - 1) / kThreads;
    copy_out_kernel<<<(uint32_t)(blocks < 1024 ? blocks : 1024), kThreads, 0,
                      static_cast<hipStream_t>(stream)>>>(static_cast<const uint8_t*>(d_src),
                                                          static_cast<uint8_t*>(dev_dst), n);
    return launch_check("copy_to_host");
}

extern "C" {

size_t cfws_index_workspace_size(size_t n_conns)
{
    return (size_t)index_layout(n_conns).bytes;
}

int cfws_index_frames_batch(const void* d_buf, const uint64_t* d_begin, const uint64_t* d_end,
                            size_t n, uint64_t max_payload, uint64_t* d_starts, uint64_t cap,
                            uint64_t* d_first, uint64_t* d_consumed, int32_t* d_stop,
                            uint64_t* d_total, void* ws, size_t ws_size, void* stream)
{
    const CfwsPassScope pass_scope;
    if (int rc = check_init()) return rc;
    if (ws_size < cfws_index_workspace_size(n))
        return set_err(CFWS_ERROR_WORKSPACE, "index workspace too small", hipSuccess);
    if ((n && (!d_buf || !d_begin || !d_end || !d_first || !d_consumed || !d_stop)) ||
        (cap && !d_starts) || !d_total || !ws)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "index: null pointer", hipSuccess);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) {
        (void)hipMemsetAsync(d_total, 0, 8, st);
        return launch_check("index");
    }
    const uint8_t* buf = static_cast<const uint8_t*>(d_buf);
    const IndexLayout L = index_layout(n);
    uint64_t* slots = ws_ptr<uint64_t>(ws, L.slots);
    uint64_t* resume = ws_ptr<uint64_t>(ws, L.resume);
    const uint32_t g = grid_for(n, kThreads);
    index_walk_kernel<<<g, kThreads, 0, st>>>(buf, d_begin, d_end, n, max_payload, d_first, d_consumed,
                                              d_stop, slots, resume);
    if (int rc = run_scan(d_first, n, ws_ptr<uint64_t>(ws, L.partials), d_total, st)) return rc;
    if (cap) {
        index_place_kernel<<<grid_for(n * kIndexSlots, kThreads), kThreads, 0, st>>>(
            d_first, slots, d_total, n, d_starts, cap);
        index_rest_kernel<<<g, kThreads, 0, st>>>(buf, d_end, n, max_payload, d_first, d_total, resume,
                                                  d_starts, cap);
    }
    return launch_check("index");
}

void* cfws_mapped_device_pointer(const void* h_ptr)
{
    if (check_init() != CFWS_OK || !h_ptr) return nullptr;
    unsigned flags = 0;
    void* d = nullptr;
    if (hipHostGetFlags(&flags, const_cast<void*>(h_ptr)) != hipSuccess || !(flags & hipHostMallocMapped) ||
        hipHostGetDevicePointer(&d, const_cast<void*>(h_ptr), 0) != hipSuccess) {
        (void)hipGetLastError();     // not a mapped HIP host allocation: no sticky error
        return nullptr;
    }
    return d;
}

int cfws_copy_to_host(const void* d_src, void* h_dst, uint64_t n, void* stream)
{
    const CfwsPassScope pass_scope;
    if (int rc = check_init()) return rc;
    if (n == 0) return CFWS_OK;
    if (!d_src || !h_dst) return set_err(CFWS_ERROR_INVALID_ARGUMENT, "null pointer", hipSuccess);
    void* d = cfws_mapped_device_pointer(h_dst);
    if (!d) return set_err(CFWS_ERROR_INVALID_ARGUMENT, "destination is not mapped pinned host memory",
                           hipSuccess);
    return cfws_internal_copy_out(d_src, d, n, stream);
}

int cfws_xor_mask(const void* d_src, void* d_dst, uint64_t n, uint32_t key, uint32_t phase,
                  void* stream)
{
    const CfwsPassScope pass_scope;
    if (int rc = check_init()) return rc;
    if (n == 0) return CFWS_OK;
    xor_mask_kernel<<<capped_grid(n, 4096), kThreads, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const uint8_t*>(d_src), static_cast<uint8_t*>(d_dst), n, key, phase & 3u);
    return launch_check("xor_mask");
}

int cfws_internal_service_launch(uint64_t* dev_ctl, uint8_t* dev_bufs, uint64_t gen, uint64_t idle_ticks,
                                 uint64_t life_ticks, void* stream)
{
    dropin_service_kernel<<<1, kServiceThreads, 0, static_cast<hipStream_t>(stream)>>>(dev_ctl, dev_bufs, gen,
                                                                                     idle_ticks, life_ticks);
    return launch_check("dropin_service");
}

int cfws_device_copy(const void* d_src, void* d_dst, uint64_t n, void* stream)
{
    const CfwsPassScope pass_scope;
    if (int rc = check_init()) return rc;
    if (n == 0) return CFWS_OK;
    if (misaligned(d_src, d_dst) || (n & 15u))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "copy needs 16-byte aligned pointers and size",
                       hipSuccess);
    const uint64_t n16 = n / 16;
    const uint64_t per_block = uint64_t(kWaves) * kCopyU * 64;
    const uint64_t blocks = (n16 + per_block - 1) / per_block;
    if (blocks > 0x7fffffffull) return set_err(CFWS_ERROR_INVALID_ARGUMENT, "copy too large", hipSuccess);
    stream_copy_kernel<<<(uint32_t)blocks, kThreads, 40000, static_cast<hipStream_t>(stream)>>>(
        static_cast<const u32x4*>(d_src), static_cast<u32x4*>(d_dst), n16);
    return launch_check("device_copy");
}

int cfws_fill_splitmix(void* d_dst, uint64_t n, uint64_t seed, uint64_t byte_base, void* stream)
{
    const CfwsPassScope pass_scope;
    if (int rc = check_init()) return rc;
    if (byte_base & 7u) return set_err(CFWS_ERROR_INVALID_ARGUMENT, "byte_base % 8 != 0", hipSuccess);
    if (reinterpret_cast<uintptr_t>(d_dst) & 15u)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "destination must be 16-byte aligned", hipSuccess);
    if (n == 0) return CFWS_OK;
    fill_splitmix_kernel<<<capped_grid(n, 8192), kThreads, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<uint8_t*>(d_dst), n, seed, byte_base / 8);
    return launch_check("fill_splitmix");
}

}  // extern "C"
