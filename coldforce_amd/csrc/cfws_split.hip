// cfws_split.hip -- the split ops and their C ABI (include/cfws.h; DESIGN.md
// §3.8): header and payload passes over caller-laid-out frames
// (cfws_encode_headers, cfws_parse_headers, cfws_mask_batch,
// cfws_mask_batch_packed, cfws_unmask_batch).
#include "cfws_kernels.h"

namespace {

// co_ws_frame.c:34-91 for every frame: its 2-14 header bytes at wire_off,
// one thread per frame; bytes at or past cap are not written.
__global__ void __launch_bounds__(kThreads)
encode_headers_kernel(cfws_frame_desc_t* __restrict__ desc, uint64_t n, uint8_t* __restrict__ wire,
                      uint64_t cap)
{
    const uint64_t f = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (f >= n) return;
    const DescWords d = load_desc(desc, (uint32_t)f);
    const uint32_t hs = header_size_of(d.payload_size, d.mask() != 0);
    FrameView v;
    v.body_len = d.payload_size;
    v.key = d.mask() ? d.key() : 0u;
    v.hb = d.header_word0();
#pragma unroll
    for (uint32_t r = 0; r < 14; ++r)
        if (r < hs && d.wire_off + r < cap) wire[d.wire_off + r] = (uint8_t)view_header_byte(v, r);
    desc[f].header_size = (uint8_t)hs;
}

// co_ws_frame.c:131-213 (+ the callers' 2-byte precheck) at every frame
// start, one thread per frame: cfws_deserialize_plan's decode without the
// payload layout.
__global__ void __launch_bounds__(kThreads)
parse_headers_kernel(const uint8_t* __restrict__ wire, uint64_t size, const uint64_t* __restrict__ index,
                     uint64_t n, uint64_t max_payload, cfws_frame_desc_t* __restrict__ desc,
                     int32_t* __restrict__ status)
{
    const uint64_t f = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (f >= n) return;
    cfws_frame_desc_t d;
    status[f] = parse_ws_header(wire, size, index[f], max_payload, d);
    desc[f] = d;
}

// The payload loops (mask: co_ws_frame.c:93-97, unmask: :232-242) of every
// frame, each frame from its own source to its own destination. A wave
// writes one 1 KiB-aligned span of the destination per store instruction
// (64 lanes x 16 B), as the streaming kernel's regions do, so interior
// 64-byte segments are always written whole by one instruction (a span
// grid starting at the frame's first chunk left every instruction's first
// and last segment half-written: 5.6 / 5.9 TB/s against the streaming
// kernel's 6.5). Work unit (frame, piece): the frame's spans are split
// evenly over the fewest pieces of at most 20 spans, each wave taking a
// contiguous run of up to 5 (every load in flight before the first store),
// so a 64 KiB frame is 4 equal workgroups at any alignment. Stores are
// write-through (+0.6 % over `nt` stores and interleaved spans,
// tools/split_ab.sh) and both run at 4 workgroups per CU (the unmask ran
// at 5 until the round-3 rewrite; at 4 since, 1.377 -> 1.349 ms). A run is
// straight-line buffer loads and stores over descriptors clipped to it
// (xor_run); the frame's first and last chunk, which it may share with its
// neighbours, are written byte by byte by payload_edge_kernel after the
// stream. Round 3 took the per-lane bounds and per-store descriptor work out
// of the slots: 1.59 / 1.42 ms -> 1.47 / 1.38 ms (mask / unmask, config 2
// layout, profiles/r03_split_ab/).
#ifndef CFWS_MASK_LDS
#define CFWS_MASK_LDS 40000
#endif
#ifndef CFWS_UNMASK_LDS
#define CFWS_UNMASK_LDS 40000
#endif
constexpr uint32_t kPieceK = 5;
constexpr uint32_t kSpanChunks = 64;
constexpr uint32_t kPieceSpans = kPieceK * kWaves;

// A packed mask's boundary chunks (cfws_mask_batch_packed): the chunks from
// the one holding frame f's header start up to its first whole payload
// chunk, [c0, c0 + 16 nbc), hold frame f - 1's payload tail, f's header,
// then f's payload head. The tail and the header are wave-uniform words
// (T.lo, T.hi: bytes [0, 32) from c0; zero from pre = dof - c0 on); the
// payload head is the lane's own chunk, which is right from dof on.
struct PackedHead {
    uint64_t c0 = 0, dof = 0;
    uint4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
};

// One wave's run of up to kPieceK 1 KiB spans of a frame: every lane of every
// slot loads and stores; buffer descriptors clipped to the run and to the
// frame's whole chunks make the loads outside them return zeros and the
// stores outside them drop, so there is no branch. Lane l of slot k reads
// the aligned source block at offset sd + 1024 k + 16 l of rs
// (funnel-shifted with the next lane's block over DPP; the block after slot
// k < 4 is lane 0 of slot k + 1, rotated into lane 63) and writes the chunk
// at offset dd + 1024 k + 16 l of rd. kEdge: the run holds the frame's first
// span and starts below a descriptor's base (sd or dd negative), so offsets
// go out of range explicitly, never by 32-bit wrap-around. Without it
// (every other run) the offsets are plain: a per-slot edge test cost the
// unmask 7 % (1.46 against 1.37 ms). kPacked: the run also writes the
// frame's boundary chunks (ph_).
template <bool kEdge, bool kPacked = false>
__device__ __forceinline__ void xor_run(__amdgpu_buffer_rsrc_t rs, __amdgpu_buffer_rsrc_t rd, int32_t sd, int32_t dd,
                                        uint32_t ph, uint32_t kr, uint64_t wbase = 0, const PackedHead* ph_ = nullptr)
{
    constexpr uint64_t kSpan = kSpanChunks * 16;
    const uint32_t lane = threadIdx.x & 63u;
    auto off = [](int32_t o) { return kEdge ? (o < 0 ? 0x7fffffff : o) : o; };
    u32x4 a[kPieceK], ex = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < (int)kPieceK; ++k)
        a[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, off(sd + (int32_t)(lane * 16 + k * kSpan)), 0, 0);
    if (ph && lane == 63) ex = __builtin_amdgcn_raw_buffer_load_b128(rs, off(sd + (int32_t)(kPieceK * kSpan)), 0, 0);
    auto slot = [&](const int k) {
        const uint4 A4 = make_uint4(a[k][0], a[k][1], a[k][2], a[k][3]);
        uint4 o = A4;
        if (ph) {
            const uint4 L = k + 1 < (int)kPieceK
                                ? from_next_lane_wrap(make_uint4(a[k + 1][0], a[k + 1][1], a[k + 1][2], a[k + 1][3]))
                                : make_uint4(ex[0], ex[1], ex[2], ex[3]);
            o = funnel16(A4, from_next_lane(A4, L), ph);
        }
        xor4(o, kr);
        if (kPacked) {
            const uint64_t D = wbase + (uint64_t)k * kSpan + lane * 16;
            if (D >= ph_->c0 && D < ph_->dof) {
                const uint32_t q = (uint32_t)(ph_->dof - D < 16 ? ph_->dof - D : 16);   // bytes before the payload
                const uint4 T = D == ph_->c0 ? ph_->lo : ph_->hi;
                o = or4(and4(o, byte_range(q, 16)), and4(T, byte_range(0, q)));
            }
        }
        // write-through, as the streaming kernel's regions (sc0 sc1 nt)
        const u32x4 v = {o.x, o.y, o.z, o.w};
        __builtin_amdgcn_raw_buffer_store_b128(v, rd, off(dd + (int32_t)(lane * 16 + k * kSpan)), 0, 19);
    };
#pragma unroll
    for (int k = 0; k < (int)kPieceK; ++k) slot(k);
}

// cfws_mask_batch_packed: frame g's boundary chunks (PackedHead) are written
// whole by g's first run when g - 1's payload ends exactly where g's header
// starts (checked here, not trusted), g's payload has at least 16 bytes and
// g - 1's at least 16 (so a boundary chunk holds one tail and one header),
// and the chunks end inside the capacity; otherwise payload_edge_kernel
// writes g's head bytes and g - 1's tail bytes one by one, as unpacked.
__device__ __forceinline__ bool packed_inrun(const cfws_frame_desc_t* __restrict__ desc, uint64_t g, uint64_t n,
                                             uint64_t cap)
{
    if (g == 0 || g >= n) return false;
    const DescWords a = load_desc(desc, (uint32_t)(g - 1)), b = load_desc(desc, (uint32_t)g);
    const uint64_t aend = a.wire_off + header_size_of(a.payload_size, a.mask() != 0) + a.payload_size;
    const uint64_t bdof = b.wire_off + header_size_of(b.payload_size, b.mask() != 0);
    return aend == b.wire_off && a.payload_size >= 16 && b.payload_size >= 16 &&
           ((bdof + 15) & ~uint64_t(15)) <= cap;
}

// The per-frame prologue below and payload_edge_kernel's, and the packed
// head, are written out in their kernels: as shared functions (split_frame,
// packed_head) they compile to a differently ordered prologue, which cost the
// split bench 0.1-0.2 % (profiles/r07/ops_refactor/).
template <bool kUnmask>
__global__ void __launch_bounds__(kThreads)
payload_xor_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                   const cfws_frame_desc_t* __restrict__ desc, const int32_t* __restrict__ status,
                   uint64_t n, uint32_t pieces, uint64_t cap, uint32_t packed)
{
    const uint64_t f = blockIdx.x / pieces;
    const uint32_t p = blockIdx.x % pieces;
    if (f >= n) return;
    if (kUnmask && status && status[f] != CFWS_PARSE_COMPLETE) return;
    const DescWords d = load_desc(desc, (uint32_t)f);
    const uint64_t len = d.payload_size;
    const uint64_t so = kUnmask ? d.wire_off + d.header_size() : d.payload_off;
    const uint64_t dof = kUnmask ? d.payload_off : d.wire_off + header_size_of(len, d.mask() != 0);
    const uint32_t key = d.mask() ? d.key() : 0u;
    if (len == 0 || dof >= cap) return;
    // the packed mask: this frame's boundary chunks in its first run
    PackedHead H;
    const bool inrun = !kUnmask && packed && packed_inrun(desc, f, n, cap);
    if (inrun) {
        const DescWords a = load_desc(desc, (uint32_t)(f - 1));
        H.c0 = d.wire_off & ~uint64_t(15);
        H.dof = dof;
        const uint32_t t = (uint32_t)(d.wire_off - H.c0);             // f - 1's tail bytes
        const uint4 z = make_uint4(0, 0, 0, 0);
        // the header (co_ws_frame.c:34-91) at byte t of the 32-byte window
        const uint4 Hd = ws_header_words(len, d.header_word0(), key);
        H.lo = t ? funnel16(z, Hd, 16u - t) : Hd;
        H.hi = t ? funnel16(Hd, z, 16u - t) : z;
        if (t) {
            // f - 1's last t payload bytes, masked with its key
            const uint64_t ts = a.payload_off + a.payload_size - t;       // their source
            uint64_t addr = reinterpret_cast<uint64_t>(src) + (ts & ~uint64_t(15));
            asm volatile("" : "+v"(addr));
            const uint8_t* sp = reinterpret_cast<const uint8_t*>(addr);
            const uint32_t tph = (uint32_t)(ts & 15u);
            uint4 T = ld16(sp);
            if (tph + t > 16) T = funnel16(T, ld16(sp + 16), tph);
            else if (tph) T = funnel16(T, z, tph);
            xor4(T, a.mask() ? rotr8(a.key(), (uint32_t)((a.payload_size - t) & 3u)) : 0u);
            H.lo = or4(H.lo, and4(T, byte_range(0, t)));
        }
    }
    const uint64_t dend = len < cap - dof ? dof + len : cap;
    // 1 KiB spans of the destination arena (dst is 16-byte aligned; spans
    // count from it) holding the frame
    const uint64_t s0 = (inrun ? H.c0 : dof) / (16 * kSpanChunks), s1 = (dend - 1) / (16 * kSpanChunks) + 1;
    const uint64_t ns = s1 - s0;
    const uint64_t used = (ns + kPieceSpans - 1) / kPieceSpans;
    // source phase against the 16-byte destination chunks: one per frame
    const uint32_t ph = (uint32_t)((so - dof) & 15u);
    // wave-uniform, so the span bases and buffer descriptors stay scalar (a
    // descriptor the compiler cannot prove uniform costs a readfirstlane loop
    // per store)
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the key rotation of every 16-byte destination chunk: A - dof = -dof mod 4
    const uint32_t kr = rotr8(key, (uint32_t)((0u - (uint32_t)dof) & 3u));
    constexpr uint64_t kSpan = kSpanChunks * 16;
    // the aligned source blocks holding the frame's bytes, [xs0, xs1), and
    // the destination chunks the frame fills whole, [xd0, xd1)
    const int64_t xs0 = (int64_t)(so & ~uint64_t(15)), xs1 = (int64_t)((so + (dend - dof) + 15) & ~uint64_t(15));
    const uint64_t xd0 = inrun ? H.c0 : (dof + 15) & ~uint64_t(15), xd1 = dend & ~uint64_t(15);
    // virtual pieces p, p + pieces, ...: a frame larger than the caller's
    // max_payload_size (or a grid capped below 2^31 blocks) still gets every
    // chunk written
    for (uint64_t vp = p; vp < used; vp += pieces) {
        const uint64_t sb = s0 + ns * vp / used, se_piece = s0 + ns * (vp + 1) / used;
        // wave w streams a contiguous run of the piece's spans, [wb, se)
        const uint64_t m = se_piece - sb;
        const uint64_t wb = sb + m * wave / kWaves, se = sb + m * (wave + 1) / kWaves;
        const uint32_t cnt = (uint32_t)(se - wb);
        // descriptors over the run's source blocks and whole destination
        // chunks, clipped to the frame's (xor_run); lane l of span wb + k
        // reads the aligned source block at vb + 1024 k + 16 l
        const int64_t vb = (int64_t)so + (int64_t)(wb * kSpan) - (int64_t)dof - (int64_t)ph;
        const int64_t ve = vb + (int64_t)(cnt * kSpan) + 16;
        const int64_t ls = vb > xs0 ? vb : xs0, le = ve < xs1 ? ve : xs1;
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(src) + (le > ls ? ls : 0), 0,
                                                          le > ls ? (int)(le - ls) : 0, 0x00020000);
        const int32_t sd = (int32_t)(vb - ls);
        const uint64_t ds = wb * kSpan > xd0 ? wb * kSpan : xd0, de = se * kSpan < xd1 ? se * kSpan : xd1;
        const auto rd = __builtin_amdgcn_make_buffer_rsrc(dst + (de > ds ? ds : 0), 0,
                                                          de > ds ? (int)(de - ds) : 0, 0x00020000);
        const int32_t ddl = (int32_t)((int64_t)(wb * kSpan) - (int64_t)ds);
        if (inrun && wb * kSpan < ((dof + 15) & ~uint64_t(15)))
            xor_run<true, true>(rs, rd, sd, ddl, ph, kr, wb * kSpan, &H);
        else if (sd < 0 || ddl < 0)
            xor_run<true>(rs, rd, sd, ddl, ph, kr);
        else
            xor_run<false>(rs, rd, sd, ddl, ph, kr);
    }
}

// The frames' partial first and last chunks: one thread per frame writes
// the frame's bytes of the (at most two) 16-byte destination chunks it
// shares with its neighbours, byte by byte, in a launch after the stream.
// (In the stream, the edge runs' byte stores held their workgroups' slots:
// mask 1.482 ms there against 1.404 + 0.012 here, profiles/r03_split_ab/
// edge_kernel/.)
template <bool kUnmask>
__global__ void __launch_bounds__(kThreads)
payload_edge_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                    const cfws_frame_desc_t* __restrict__ desc, const int32_t* __restrict__ status,
                    uint64_t n, uint64_t cap, uint32_t packed)
{
    const uint64_t f = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (f >= n) return;
    if (kUnmask && status && status[f] != CFWS_PARSE_COMPLETE) return;
    // the packed mask: bytes a boundary chunk written in-run carries are done
    const bool head_done = !kUnmask && packed && packed_inrun(desc, f, n, cap);
    const bool tail_done = !kUnmask && packed && packed_inrun(desc, f + 1, n, cap);
    const DescWords d = load_desc(desc, (uint32_t)f);
    const uint64_t len = d.payload_size;
    const uint64_t so = kUnmask ? d.wire_off + d.header_size() : d.payload_off;
    const uint64_t dof = kUnmask ? d.payload_off : d.wire_off + header_size_of(len, d.mask() != 0);
    const uint32_t key = d.mask() ? d.key() : 0u;
    if (len == 0 || dof >= cap) return;
    const uint64_t dend = len < cap - dof ? dof + len : cap;
    // [dof, first whole chunk) and [last whole chunk's end, dend)
    const uint64_t h1 = (dof + 15) & ~uint64_t(15), t0 = dend & ~uint64_t(15);
    const uint64_t ha = dof, hb = h1 < dend ? h1 : dend;
    const uint64_t ta = t0 > hb ? t0 : hb, tb = dend;
    if (!head_done)
        for (uint64_t x = ha; x < hb; ++x)
            dst[x] = src[so + (x - dof)] ^ (uint8_t)(key >> (8 * ((x - dof) & 3u)));
    if (!tail_done)
        for (uint64_t x = ta; x < tb; ++x)
            dst[x] = src[so + (x - dof)] ^ (uint8_t)(key >> (8 * ((x - dof) & 3u)));
}

// Pieces per frame for the split payload ops: enough workgroups to cover the
// largest frame (max_payload_size, at any alignment) in pieces of at most
// kPieceSpans 1 KiB spans, capped so the grid stays under 2^31 blocks (the
// kernel then strides over a frame's pieces).
uint32_t payload_pieces(size_t n, uint64_t max_payload_size)
{
    const uint64_t spans = max_payload_size / (16 * kSpanChunks) + 2;
    uint64_t pieces = (spans + kPieceSpans - 1) / kPieceSpans;
    if (pieces > 65536) pieces = 65536;
    while (pieces > 1 && pieces * n > 0x7fffffffull) pieces >>= 1;
    return (uint32_t)pieces;
}

template <bool kUnmask>
int launch_payload_xor(const void* src, void* dst, const cfws_frame_desc_t* d_desc,
                       const int32_t* d_status, size_t n, uint64_t max_payload_size, uint64_t cap,
                       void* stream, const char* what, uint32_t packed = 0)
{
    if (int rc = check_init()) return rc;
    if (n == 0 || cap == 0) return CFWS_OK;
    if (!src || !dst || !d_desc) return set_err(CFWS_ERROR_INVALID_ARGUMENT, "null pointer", hipSuccess);
    if (misaligned(src, dst))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "arenas must be 16-byte aligned", hipSuccess);
    if (n > 0x7fffffffull) return set_err(CFWS_ERROR_INVALID_ARGUMENT, "too many frames", hipSuccess);
    const uint32_t pieces = payload_pieces(n, max_payload_size);
    payload_xor_kernel<kUnmask><<<(uint32_t)(n * pieces), kThreads, kUnmask ? CFWS_UNMASK_LDS : CFWS_MASK_LDS,
                                  static_cast<hipStream_t>(stream)>>>(
        static_cast<const uint8_t*>(src), static_cast<uint8_t*>(dst), d_desc, d_status, n, pieces, cap, packed);
    payload_edge_kernel<kUnmask><<<grid_for(n, kThreads), kThreads, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const uint8_t*>(src), static_cast<uint8_t*>(dst), d_desc, d_status, n, cap, packed);
    return launch_check(what);
}

}  // namespace

extern "C" {

int cfws_encode_headers(cfws_frame_desc_t* d_desc, size_t n, void* d_wire, uint64_t wire_capacity,
                        void* stream)
{
    const CfwsPassScope pass_scope;
    if (int rc = check_init()) return rc;
    if (n == 0) return CFWS_OK;
    if (!d_desc || !d_wire) return set_err(CFWS_ERROR_INVALID_ARGUMENT, "null pointer", hipSuccess);
    if (n > 0xffffffffull) return set_err(CFWS_ERROR_INVALID_ARGUMENT, "too many frames", hipSuccess);
    encode_headers_kernel<<<grid_for(n, kThreads), kThreads, 0, static_cast<hipStream_t>(stream)>>>(
        d_desc, n, static_cast<uint8_t*>(d_wire), wire_capacity);
    return launch_check("encode_headers");
}

int cfws_parse_headers(const void* d_wire, uint64_t wire_size, const uint64_t* d_frame_index, size_t n,
                       uint64_t max_payload, cfws_frame_desc_t* d_desc, int32_t* d_status,
                       void* stream)
{
    const CfwsPassScope pass_scope;
    if (int rc = check_init()) return rc;
    if (n == 0) return CFWS_OK;
    if (!d_wire || !d_frame_index || !d_desc || !d_status)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "null pointer", hipSuccess);
    parse_headers_kernel<<<grid_for(n, kThreads), kThreads, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const uint8_t*>(d_wire), wire_size, d_frame_index, n, max_payload, d_desc,
        d_status);
    return launch_check("parse_headers");
}

int cfws_mask_batch(const void* d_payload, const cfws_frame_desc_t* d_desc, size_t n,
                    uint64_t max_payload_size, void* d_wire, uint64_t wire_capacity, void* stream)
{
    const CfwsPassScope pass_scope;
    return launch_payload_xor<false>(d_payload, d_wire, d_desc, nullptr, n, max_payload_size,
                                     wire_capacity, stream, "mask_batch");
}

int cfws_mask_batch_packed(const void* d_payload, const cfws_frame_desc_t* d_desc, size_t n,
                           uint64_t max_payload_size, void* d_wire, uint64_t wire_capacity, void* stream)
{
    const CfwsPassScope pass_scope;
    return launch_payload_xor<false>(d_payload, d_wire, d_desc, nullptr, n, max_payload_size,
                                     wire_capacity, stream, "mask_batch_packed", 1u);
}

int cfws_unmask_batch(const void* d_wire, const cfws_frame_desc_t* d_desc, const int32_t* d_status,
                      size_t n, uint64_t max_payload_size, void* d_payload,
                      uint64_t payload_capacity, void* stream)
{
    const CfwsPassScope pass_scope;
    return launch_payload_xor<true>(d_wire, d_payload, d_desc, d_status, n, max_payload_size,
                                    payload_capacity, stream, "unmask_batch");
}

}  // extern "C"
