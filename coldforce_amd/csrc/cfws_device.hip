// cfws_device.hip -- MI355X (gfx950) WebSocket frame codec: the batch C ABI
// (include/cfws.h: serialize / deserialize execute and batch, and the route
// a batch takes), the single-launch small-batch kernels, and the library's
// runtime: error state, device probe and pass timing. The plans and the
// fused deserialize are in cfws_plan.hip; the streaming kernel and the
// device code the units share in cfws_kernels.h; the receive into fixed
// slots in cfws_slots.hip; HTTP/2 in cfws_h2.hip; the split ops in
// cfws_split.hip; the smaller ops in cfws_ops.hip.
//
// Reference behaviour restated on the device:
//   header encode        co_ws_frame.c:34-68, :70-91
//   payload mask         co_ws_frame.c:93-97    out[i] = in[i] ^ key[i % 4]
//   header decode        co_ws_frame.c:131-213 (MORE_DATA before TOO_BIG)
//   payload copy+unmask  co_ws_frame.c:214-242
//
// An execute is one streaming pass (launch_pass, cfws_kernels.h; DESIGN.md
// §3.1) over the output bytes [base, base + total), from the plan's
// per-frame offsets and region map. Deserialize with
// CFWS_DESERIALIZE_REASSEMBLE runs two passes: data frames packed (messages
// contiguous), then control frames after them.
#include "cfws_kernels.h"

#include <mutex>

namespace cfws_rt {

thread_local char g_err[512] = "";

int set_err(int code, const char* what, hipError_t e)
{
    snprintf(g_err, sizeof g_err, "%s%s%s", what, e == hipSuccess ? "" : ": ",
             e == hipSuccess ? "" : hipGetErrorString(e));
    fprintf(stderr, "cfws: %s\n", g_err);
    return code;
}

// Every visible device is probed once, by whichever thread gets here first
// (std::call_once); afterwards the checks only read what the probe wrote.
// A call runs on the caller's current device, which must be a gfx950.
namespace {
std::once_flag g_probe_once;
int g_probe_rc = CFWS_OK;
int g_dev_count = 0;
uint64_t g_gfx950_mask = 0;        // bit d: device d is a gfx950 (d < 64)
char g_probe_msg[256] = "";

void probe_devices()
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        g_probe_rc = set_err(CFWS_ERROR_NO_DEVICE, "no HIP device", e);
        snprintf(g_probe_msg, sizeof g_probe_msg, "%s", g_err);
        return;
    }
    g_dev_count = count;
    char first_arch[64] = "";
    for (int d = 0; d < count && d < 64; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) != hipSuccess) continue;
        if (d == 0) snprintf(first_arch, sizeof first_arch, "%s", prop.gcnArchName);
        if (strncmp(prop.gcnArchName, "gfx950", 6) == 0) g_gfx950_mask |= uint64_t(1) << d;
    }
    if (g_gfx950_mask == 0) {
        snprintf(g_probe_msg, sizeof g_probe_msg, "no gfx950 device (device 0 is %s)", first_arch);
        g_probe_rc = set_err(CFWS_ERROR_NO_DEVICE, g_probe_msg, hipSuccess);
    }
}
}  // namespace

int check_device(int dev)
{
    std::call_once(g_probe_once, probe_devices);
    if (g_probe_rc != CFWS_OK) {
        snprintf(g_err, sizeof g_err, "%s", g_probe_msg);
        return g_probe_rc;
    }
    if (dev < 0 || dev >= g_dev_count || dev >= 64 || !((g_gfx950_mask >> dev) & 1)) {
        snprintf(g_err, sizeof g_err, "device %d is not a usable gfx950 device (%d visible)", dev, g_dev_count);
        return CFWS_ERROR_NO_DEVICE;
    }
    return CFWS_OK;
}

int check_init()
{
    std::call_once(g_probe_once, probe_devices);
    if (g_probe_rc != CFWS_OK) return check_device(0);
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return set_err(CFWS_ERROR_NO_DEVICE, "hipGetDevice", e);
    return check_device(dev);
}

int launch_check(const char* what)
{
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? CFWS_OK : set_err(CFWS_ERROR_HIP, what, e);
}

}  // namespace cfws_rt

// Pass timing (cfws_internal.h): the calling thread's pending event pair and
// the open public call's.
CfwsPassEvents& cfws_internal_pass_events()
{
    thread_local CfwsPassEvents e = {nullptr, nullptr};
    return e;
}

namespace {
thread_local CfwsPassEvents t_call_pass = {nullptr, nullptr};   // the open call's pair
thread_local int t_pass_depth = 0;                               // open public calls
}  // namespace

CfwsPassScope::CfwsPassScope()
{
    if (t_pass_depth++ == 0) {
        CfwsPassEvents& pe = cfws_internal_pass_events();
        t_call_pass = pe;
        pe = {nullptr, nullptr};
    }
}

CfwsPassScope::~CfwsPassScope()
{
    if (--t_pass_depth == 0) t_call_pass = {nullptr, nullptr};
}

CfwsPassEvents cfws_internal_take_pass()
{
    const CfwsPassEvents e = t_call_pass;
    t_call_pass = {nullptr, nullptr};
    return e;
}

CfwsPassTimer::CfwsPassTimer(void* s) : e(cfws_internal_take_pass()), stream(s)
{
    if (e.start) (void)hipEventRecord(static_cast<hipEvent_t>(e.start), static_cast<hipStream_t>(stream));
}

CfwsPassTimer::~CfwsPassTimer()
{
    if (e.stop) (void)hipEventRecord(static_cast<hipEvent_t>(e.stop), static_cast<hipStream_t>(stream));
}

namespace {

using cfws_rt::g_err;

// Both reassembly passes' edge chunks in one launch of their own (the
// CFWS_EDGE_SPLIT=1 form; by default pass 0's streaming launch carries them).
__global__ void __launch_bounds__(kEdgeThreads)
edge_reasm_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                  const cfws_frame_desc_t* __restrict__ desc, const int32_t* __restrict__ status,
                  const uint64_t* __restrict__ offs0, const uint64_t* __restrict__ offs1,
                  const uint64_t* __restrict__ hdr, uint64_t capacity, uint32_t n_frames)
{
    const uint64_t t = uint64_t(blockIdx.x) * kEdgeThreads + threadIdx.x;
    if (edge_thread_frame(t) >= n_frames) return;
    reasm_edge_frame(src, dst, desc, status, offs0, offs1, hdr, capacity, n_frames, edge_thread_frame(t),
                     edge_thread_part(t));
}

// CFWS_SER_INREG=0: the edge workgroups write every serialize edge chunk
// (A/B knob).
bool ser_inreg()
{
    static const bool v = env_knob("CFWS_SER_INREG", 1) != 0;
    return v;
}

// The fused deserialize (deserialize_plan_single_kernel<true>, cfws_plan.hip)
// for batches of more than kSmallFrames frames averaging at most
// kFusedAvgMax wire bytes (CFWS_FUSED_DESER=0: plan + execute; A/B knob). A
// block copies its own frames, so a batch mixing a few huge frames into
// small ones would leave those to single waves: the average keeps such
// batches on the region stream (at 1 KiB frames the fused form lost: step
// 3.04 -> 3.35 ms).
constexpr uint64_t kFusedAvgMax = 512;

bool fused_deser()
{
    static const bool v = env_knob("CFWS_FUSED_DESER", 1) != 0;
    return v;
}

// ---------------------------------------------------------------------------
// small batches: plan and stream in one launch per direction
// ---------------------------------------------------------------------------
// A batch of up to kSmallFrames frames into at most kSmallBytes of output is
// bound by launch latency, not HBM: plan (two launches) + execute (one) per
// direction. Here every workgroup computes the batch's layout itself into
// LDS (a 1,024-entry scan: a few microseconds, all reads from L2 after the
// first workgroup), workgroup 0 writes the descriptors, statuses and totals
// the plan would, and all workgroups then write their 16-byte output chunks:
// a chunk inside one body takes body_chunk (two aligned loads + funnel), any
// other chunk (headers, frame boundaries, padding) is assembled byte by byte.
// Outputs are the normal path's, byte for byte, including the zeros the last
// chunk writes past the total within the capacity.
constexpr uint32_t kSmallFrames = 1024;
constexpr uint64_t kSmallBytes = 4ull << 20;
constexpr int kSmallItems = kSmallFrames / kThreads;
#ifndef CFWS_SMALL_CPT
#define CFWS_SMALL_CPT 1
#endif
constexpr uint32_t kSmallChunksPerThread = CFWS_SMALL_CPT;   // output chunks per thread

// Frame k * kThreads + tid of a small batch is thread tid's k-th: every
// thread loads (and parses) at most kSmallItems frames, all independent, and
// a batch of up to kThreads frames keeps every thread busy.
__device__ __forceinline__ uint32_t small_frame(int k) { return k * kThreads + threadIdx.x; }

// s_off[f] = exclusive prefix of w over the frames (w[k]: frame
// small_frame(k)), one block scan per slice of kThreads frames; s_off[n] =
// the grand total (returned). Ends with a barrier.
__device__ __forceinline__ uint64_t small_scan(const uint64_t (&w)[kSmallItems], uint32_t n,
                                               uint64_t* s_off, uint64_t* s_wave)
{
    uint64_t carry = 0;
#pragma unroll
    for (int k = 0; k < kSmallItems; ++k) {
        if (uint32_t(k) * kThreads >= n) break;          // uniform: the slice is empty
        uint64_t tot;
        const uint64_t ex = block_exclusive_scan(w[k], s_wave, &tot);
        const uint32_t f = small_frame(k);
        if (f < n) s_off[f] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) s_off[n] = carry;
    __syncthreads();
    return carry;
}

// Largest f < n with s_off[f] <= D (s_off[0] = 0 <= D).
__device__ __forceinline__ uint32_t small_frame_of(const uint64_t* s_off, uint32_t n, uint64_t D)
{
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (s_off[mid] <= D) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void small_store(uint8_t* dst, uint64_t cap, uint64_t D, uint4 o)
{
    if (D + 16 <= cap) {
        st16(dst + D, o);
    } else {
        for (uint32_t j = 0; D + j < cap; ++j) dst[D + j] = (uint8_t)(u4_byte(o, (int)j));
    }
}

// This workgroup's 16-byte chunks of the output bytes [0, total), frames at
// s_off[0..n]; view(f): frame f's FrameView from LDS (small_ser_view /
// small_de_view: no header and zero padding after the body on the receive,
// no padding on the send).
template <int kMode, typename View>
__device__ __forceinline__ void small_chunks(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                             uint64_t cap, uint64_t total, const uint64_t* s_off, uint32_t n,
                                             View view)
{
    const uint64_t n_chunks = (total + 15) / 16;
    for (uint64_t c = uint64_t(blockIdx.x) * kThreads + threadIdx.x; c < n_chunks;
         c += uint64_t(gridDim.x) * kThreads) {
        const uint64_t D = c * 16;
        uint32_t f = small_frame_of(s_off, n, D);
        FrameView v = view(f);
        uint4 o;
        const uint64_t lim = D + 16 < total ? D + 16 : total;
        const uint64_t o1 = f + 1 < n ? s_off[f + 1] : ~uint64_t(0);
        const uint64_t o2 = f + 2 < n ? s_off[f + 2] : ~uint64_t(0);
        if (D >= v.body_start && D + 16 <= v.body_start + v.body_len) {
            o = body_chunk(src, v, D);
        } else if (o2 >= lim) {
            // at most two frames in the chunk: their body bytes lined up in
            // registers (edge_chunk), headers generated, padding zero
            const FrameView vb = f + 1 < n ? view(f + 1) : v;
            Pass P = {};
            P.src = src;
            P.total = total;
            o = edge_chunk<kMode>(P, f, D, v, vb, o1, o2);
        } else {
            uint32_t b[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint64_t pos = D + j;
                b[j] = 0;
                if (pos >= total) continue;
                while (pos >= s_off[f + 1]) v = view(++f);
                const uint64_t r = pos - v.out_off;
                if (r < v.pre) {
                    b[j] = view_header_byte(v, (uint32_t)r);
                } else if (r - v.pre < v.body_len) {
                    const uint64_t k = r - v.pre;
                    b[j] = (src[v.src_off + k] ^ (v.key >> (8 * (k & 3u)))) & 0xffu;
                }
            }
            o = make_uint4(b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24,
                           b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24,
                           b[8] | b[9] << 8 | b[10] << 16 | b[11] << 24,
                           b[12] | b[13] << 8 | b[14] << 16 | b[15] << 24);
        }
        small_store(dst, cap, D, o);
    }
}

// A serialize frame's view from the LDS copy of its descriptor.
__device__ __forceinline__ FrameView small_ser_view(const uint64_t* s_off, const uint64_t* s_src,
                                                    const uint64_t* s_len, const uint32_t* s_key,
                                                    const uint32_t* s_hb, uint32_t f)
{
    FrameView v = {};
    v.out_off = s_off[f];
    v.pre = s_hb[f] >> 16;
    v.body_start = v.out_off + v.pre;
    v.body_len = s_len[f];
    v.src_off = s_src[f];
    v.key = s_key[f];
    v.hb = s_hb[f] & 0xffffu;
    return v;
}

// co_ws_frame_serialize for every frame (co_ws_frame.c:34-97), frames back
// to back from wire offset 0; as cfws_serialize_plan + cfws_serialize_execute.
__global__ void __launch_bounds__(kThreads)
serialize_small_kernel(const uint8_t* __restrict__ src, cfws_frame_desc_t* __restrict__ desc,
                       uint32_t n, uint8_t* __restrict__ dst, uint64_t cap,
                       uint64_t* __restrict__ ws_hdr, uint64_t* __restrict__ user_total)
{
    __shared__ uint64_t s_off[kSmallFrames + 1];
    __shared__ uint64_t s_src[kSmallFrames];        // payload offset
    __shared__ uint64_t s_len[kSmallFrames];        // payload size
    __shared__ uint32_t s_key[kSmallFrames];        // mask key (0: unmasked)
    __shared__ uint32_t s_hb[kSmallFrames];         // header byte 0 | mask bit << 8 | header size << 16
    __shared__ uint64_t s_wave[kWaves];
    uint64_t w[kSmallItems];
#pragma unroll
    for (int k = 0; k < kSmallItems; ++k) {
        const uint32_t f = small_frame(k);
        w[k] = 0;
        if (f < n) {
            const DescWords d = load_desc(desc, f);
            const uint32_t hs = header_size_of(d.payload_size, d.mask() != 0);
            w[k] = ser_wire_bytes(hs, d.payload_size);
            s_src[f] = d.payload_off;
            s_len[f] = d.payload_size;
            s_key[f] = d.mask() ? d.key() : 0u;
            s_hb[f] = d.header_word0() | hs << 16;
        }
    }
    const uint64_t g = small_scan(w, n, s_off, s_wave);      // (its barrier publishes the views)
    const uint64_t total = g < cap ? g : cap;
    if (blockIdx.x == 0) {
        // the plan's outputs
        for (uint32_t f = threadIdx.x; f < n; f += kThreads) {
            desc[f].header_size = (uint8_t)(s_hb[f] >> 16);
            desc[f].wire_off = s_off[f];
        }
        if (threadIdx.x == 0) ser_epilogue(ws_hdr, user_total, total, g);
    }
    small_chunks<kModeSer>(src, dst, cap, total, s_off, n,
                           [&](uint32_t f) { return small_ser_view(s_off, s_src, s_len, s_key, s_hb, f); });
}

// A deserialize frame's view from LDS: no header in the output, the body
// copied + unmasked, then zeros to the next frame (alignment padding).
__device__ __forceinline__ FrameView small_de_view(const uint64_t* s_off, const uint64_t* s_src,
                                                   const uint64_t* s_len, const uint32_t* s_key,
                                                   uint32_t f)
{
    FrameView v = {};
    v.out_off = s_off[f];
    v.body_start = v.out_off;
    v.body_len = s_len[f];
    v.src_off = s_src[f];
    v.key = s_key[f];
    return v;
}

// co_ws_frame_deserialize at every index (co_ws_frame.c:121-247), payloads
// laid out as cfws_deserialize_plan lays them out without reassembly;
// as cfws_deserialize_plan + cfws_deserialize_execute (flags 0).
__global__ void __launch_bounds__(kThreads)
deserialize_small_kernel(const uint8_t* __restrict__ wire, uint64_t wire_size,
                         const uint64_t* __restrict__ index, uint32_t n, uint64_t max_payload,
                         uint64_t align, cfws_frame_desc_t* __restrict__ desc,
                         int32_t* __restrict__ status, uint8_t* __restrict__ dst, uint64_t cap,
                         uint64_t* __restrict__ ws_hdr, uint64_t* __restrict__ user_total)
{
    __shared__ uint64_t s_off[kSmallFrames + 1];
    __shared__ uint64_t s_src[kSmallFrames];        // body source: wire offset + header size
    __shared__ uint64_t s_len[kSmallFrames];        // body bytes copied (COMPLETE, fits)
    __shared__ uint32_t s_key[kSmallFrames];
    __shared__ uint64_t s_wave[kWaves];
    cfws_frame_desc_t d[kSmallItems];
    int32_t st[kSmallItems];
    uint64_t w[kSmallItems];
#pragma unroll
    for (int k = 0; k < kSmallItems; ++k) {
        const uint32_t f = small_frame(k);
        w[k] = 0;
        st[k] = CFWS_PARSE_COMPLETE;
        if (f < n) {
            st[k] = parse_ws_header(wire, wire_size, index[f], max_payload, d[k]);
            w[k] = de_slot_bytes(st[k], d[k].payload_size, align);
        }
    }
    const uint64_t g = small_scan(w, n, s_off, s_wave);
    const uint64_t total = g < cap ? g : cap;
#pragma unroll
    for (int k = 0; k < kSmallItems; ++k) {
        const uint32_t f = small_frame(k);
        if (f >= n) continue;
        d[k].payload_off = s_off[f];
        st[k] = de_capacity_rule(st[k], d[k].payload_size, s_off[f], cap);
        s_src[f] = d[k].wire_off + d[k].header_size;
        s_len[f] = st[k] == CFWS_PARSE_COMPLETE ? d[k].payload_size : 0;
        s_key[f] = d[k].mask ? d[k].mask_key : 0u;
        if (blockIdx.x == 0) {
            desc[f] = d[k];
            status[f] = st[k];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) de_epilogue(ws_hdr, user_total, total, g);
    __syncthreads();
    small_chunks<kModeDeser>(wire, dst, cap, total, s_off, n,
                             [&](uint32_t f) { return small_de_view(s_off, s_src, s_len, s_key, f); });
}

// The single-launch small-batch path (CFWS_SMALL=0 turns it off: plan +
// execute for every batch, for A/B and for tests of both paths).
bool small_path()
{
    static const bool v = env_knob("CFWS_SMALL", 1) != 0;
    return v;
}

// Workgroups of a small-batch launch: kSmallChunksPerThread output chunks
// per thread at the capacity's size.
uint32_t small_grid(uint64_t cap)
{
    const uint64_t per = uint64_t(kThreads) * kSmallChunksPerThread * 16;
    return grid_for(cap, per);
}

// Which form of cfws_deserialize_batch a call with these sizes takes, its
// other arguments valid (cfws_deserialize_pass_kernel reports the same
// choice): the one-launch small batch, the fused plan + copy of batches of
// small frames, or plan + execute.
enum DeserRoute { kDeserSmall, kDeserFused, kDeserPlanExecute };

DeserRoute deser_route(size_t n, uint64_t wire_size, uint32_t align, uint32_t flags, uint64_t cap)
{
    const bool align_ok = align != 0 && (align & (align - 1)) == 0 && align <= 4096;
    if (small_path() && n > 0 && n <= kSmallFrames && cap <= kSmallBytes && flags == 0 && align_ok)
        return kDeserSmall;
    if (fused_deser() && flags == 0 && align >= 16 && align_ok && n > kSmallFrames && n <= 0xffffffffull &&
        wire_size / n <= kFusedAvgMax)
        return kDeserFused;
    return kDeserPlanExecute;
}

}  // namespace

uint64_t cfws_internal_grand_total_offset() { return ws_layout(0, 0).hdr + 3 * sizeof(uint64_t); }

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

int cfws_init(void) { return check_init(); }
int cfws_init_device(int device) { return cfws_rt::check_device(device); }
const char* cfws_last_error(void) { return g_err; }
const char* cfws_version(void) { return "cfws 0.2 gfx950"; }

int cfws_time_next_pass(void* start, void* stop)
{
    if ((start == nullptr) != (stop == nullptr))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "start and stop events go together", hipSuccess);
    cfws_internal_pass_events() = {start, stop};
    return CFWS_OK;
}

size_t cfws_workspace_size(size_t n_frames, uint64_t out_capacity)
{
    return (size_t)ws_layout(n_frames, out_capacity).bytes;
}

int cfws_serialize_execute(const void* d_payload, const cfws_frame_desc_t* d_desc, size_t n,
                           void* d_wire, uint64_t cap, const void* ws, void* stream)
{
    const CfwsPassScope pass_scope;
    if (int rc = check_init()) return rc;
    const ArgCheck c = check_execute(n, cap, d_payload, d_wire, d_desc, ws);
    if (c.code) return set_err(c.code, c.what, hipSuccess);
    if (n == 0 || cap == 0) return CFWS_OK;
    const WsLayout L = ws_layout(n, cap);
    launch_pass<kModeSer>(L, 0, d_payload, d_wire, d_desc, nullptr, ws, cap, n, kClassAll,
                          static_cast<hipStream_t>(stream), 0, true, false,
                          ser_inreg() ? ser_inreg_flag(L, ws, n) : nullptr);
    return launch_check("serialize_execute");
}

int cfws_serialize_batch(const void* d_payload, cfws_frame_desc_t* d_desc, size_t n, void* d_wire,
                         uint64_t cap, uint64_t* d_total, void* ws, size_t ws_size, void* stream)
{
    const CfwsPassScope pass_scope;
    // small batch that both stages would accept: one launch (serialize_small_kernel)
    if (small_path() && n > 0 && n <= kSmallFrames && cap <= kSmallBytes && check_init() == CFWS_OK &&
        !check_ser_plan(d_desc, n, cap, ws, ws_size).code &&
        !check_execute(n, cap, d_payload, d_wire, d_desc, ws).code) {
        const CfwsPassTimer timer(stream);
        serialize_small_kernel<<<small_grid(cap), kThreads, 0, static_cast<hipStream_t>(stream)>>>(
            static_cast<const uint8_t*>(d_payload), d_desc, (uint32_t)n, static_cast<uint8_t*>(d_wire),
            cap, ws_ptr<uint64_t>(ws, ws_layout(n, cap).hdr), d_total);
        return launch_check("serialize_batch(small)");
    }
    if (int rc = cfws_serialize_plan(d_desc, n, cap, d_total, ws, ws_size, stream)) return rc;
    return cfws_serialize_execute(d_payload, d_desc, n, d_wire, cap, ws, stream);
}

int cfws_deserialize_execute(const void* d_wire, const cfws_frame_desc_t* d_desc,
                             const int32_t* d_status, size_t n, uint32_t flags, void* d_payload,
                             uint64_t cap, const void* ws, void* stream)
{
    const CfwsPassScope pass_scope;
    if (int rc = check_init()) return rc;
    const ArgCheck c = check_execute(n, cap, d_payload, d_wire, d_desc, d_status, ws);
    if (c.code) return set_err(c.code, c.what, hipSuccess);
    if (n == 0 || cap == 0) return CFWS_OK;
    const WsLayout L = ws_layout(n, cap);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (flags & CFWS_DESERIALIZE_REASSEMBLE) {
        // every edge chunk of both passes is disjoint from the body chunks
        // either streaming pass writes, so pass 0's launch carries them all
        const bool split = edge_split();
        const CfwsPassTimer timer(st);      // both passes: one timed span
        launch_pass<kModeDeser>(L, 0, d_wire, d_payload, d_desc, d_status, ws, cap, n, kClassData, st,
                                0, !split, !split);
        launch_pass<kModeDeser>(L, 1, d_wire, d_payload, d_desc, d_status, ws, cap, n, kClassControl,
                                st, 0, false);
        if (split)
            edge_reasm_kernel<<<grid_for(edge_threads(n), kEdgeThreads), kEdgeThreads, 0, st>>>(
                static_cast<const uint8_t*>(d_wire), static_cast<uint8_t*>(d_payload), d_desc,
                d_status, ws_ptr<const uint64_t>(ws, L.offs[0]), ws_ptr<const uint64_t>(ws, L.offs[1]),
                ws_ptr<const uint64_t>(ws, L.hdr), cap, (uint32_t)n);
    } else {
        launch_pass<kModeDeser>(L, 0, d_wire, d_payload, d_desc, d_status, ws, cap, n, kClassAll, st);
    }
    return launch_check("deserialize_execute");
}

const char* cfws_deserialize_pass_kernel(size_t n, uint64_t wire_size, uint32_t align, uint32_t flags,
                                         uint64_t payload_capacity)
{
    switch (deser_route(n, wire_size, align, flags, payload_capacity)) {
    case kDeserSmall: return "deserialize_small_kernel";
    case kDeserFused: return "deserialize_plan_single_kernel<true>";
    default: return "xform_kernel<1>";
    }
}

int cfws_deserialize_batch(const void* d_wire, uint64_t wire_size, const uint64_t* d_index,
                           size_t n, uint64_t max_payload, uint32_t align, uint32_t flags,
                           cfws_frame_desc_t* d_desc, int32_t* d_status, void* d_payload,
                           uint64_t cap, uint64_t* d_total, void* ws, size_t ws_size,
                           void* stream)
{
    const CfwsPassScope pass_scope;
    const DeserRoute route = deser_route(n, wire_size, align, flags, cap);
    // a single-launch form only for a call both stages would accept
    const bool single =
        route != kDeserPlanExecute && check_init() == CFWS_OK &&
        !check_de_plan(d_wire, d_index, n, align, flags, d_desc, d_status, cap, ws, ws_size).code &&
        !check_execute(n, cap, d_payload, d_wire, d_desc, d_status, ws).code;
    // small batch without reassembly
    if (single && route == kDeserSmall) {
        const CfwsPassTimer timer(stream);
        deserialize_small_kernel<<<small_grid(cap), kThreads, 0, static_cast<hipStream_t>(stream)>>>(
            static_cast<const uint8_t*>(d_wire), wire_size, d_index, (uint32_t)n, max_payload, align,
            d_desc, d_status, static_cast<uint8_t*>(d_payload), cap,
            ws_ptr<uint64_t>(ws, ws_layout(n, cap).hdr), d_total);
        return launch_check("deserialize_batch(small)");
    }
    // small frames at 16-byte (or wider) slots: the fused plan + copy
    if (single)
        return cfws_rt::deserialize_fused_impl(d_wire, wire_size, d_index, n, max_payload, align, d_desc,
                                               d_status, d_payload, cap, d_total, ws, stream);
    if (int rc = cfws_deserialize_plan(d_wire, wire_size, d_index, n, max_payload, align, flags,
                                       d_desc, d_status, cap, d_total, ws, ws_size, stream))
        return rc;
    return cfws_deserialize_execute(d_wire, d_desc, d_status, n, flags, d_payload, cap, ws, stream);
}

}  // extern "C"

