// cfws_h2index.hip -- HTTP/2 receive-buffer frame indexing on the device
// (cfws_h2_index_frames_batch, include/cfws.h): the walk of
// co_http2_client_on_tcp_receive_ready (co_http2_client.c:462-541) over many
// connections' receive buffers at once. The hop rule is h2_hop_by
// (cfws_rules.h), shared with the host walk (cfws_index.cpp). A unit of its
// own: the HTTP/2 rules stay out of cfws_ops.hip, whose WS indexer keeps its
// kernels as they were; what the two indexers share (the workspace layout,
// index_place_kernel, the scan) is defined once.
#include "cfws_kernels.h"

namespace {

using cfws_rt::index_place_kernel;

// One hop: the 9 header bytes and the possible pad length byte at buf + p of
// a buffer ending at e, in one round of independent loads (load_span16,
// clipped to e - p so nothing past e's dword is touched), then the rule from
// registers: one memory round trip per hop. Byte i is a constant at every
// use, so the selects below fold to a shift of one register. The caller has
// checked e - p >= 9 (the rule's first decision): with that check after the
// loads, one path left the loop with the loads never waited for, and the
// compiler then waited at the loop's head for everything outstanding, the
// previous hop's slot store included, before it issued the next loads.
__device__ __forceinline__ H2Hop h2_index_hop(const uint8_t* __restrict__ buf, uint64_t p, uint64_t e,
                                              uint32_t max_frame)
{
    __builtin_assume(e - p >= 9);
    uint32_t w[4];
    load_span16(buf + p, e - p < 10 ? (uint32_t)(e - p) : 10u, w);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    return h2_hop_by(
        [=](uint32_t i) -> uint32_t {
            const uint32_t x = i < 4 ? w0 : (i < 8 ? w1 : w2);
            return (x >> (8u * (i & 3u))) & 0xffu;
        },
        e - p, max_frame);
}

// A frame's record, one 16-byte store (d_info is 16-byte aligned).
__device__ __forceinline__ void store_info(cfws_h2_frame_info_t* __restrict__ info, uint64_t k, const H2Hop& h)
{
    *reinterpret_cast<u32x4*>(info + k) =
        u32x4{h.stream_id, h.length, h.advance, (uint32_t)h.type | (uint32_t)h.flags << 8};
}

// One connection per thread, as the WS indexer (cfws_ops.hip): the walk runs
// once over every COMPLETE frame, counts the SELECTED ones, records consumed
// / stop, keeps the first kIndexSlots selected starts in the connection's
// workspace slots and the position of selected frame kIndexSlots (where
// h2_index_rest_kernel walks on; with a filter that is not frame
// kIndexSlots of the buffer).
__global__ void __launch_bounds__(kThreads)
h2_index_walk_kernel(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ begin,
                     const uint64_t* __restrict__ end, uint64_t n, uint32_t max_frame, uint32_t select,
                     uint32_t stream_id, uint64_t* __restrict__ first, uint64_t* __restrict__ consumed,
                     int32_t* __restrict__ stop, uint64_t* __restrict__ slots, uint64_t* __restrict__ resume)
{
    const uint64_t c = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (c >= n) return;
    const uint64_t e = end[c];
    uint64_t p = begin[c];
    uint64_t k = 0, r = e;
    uint64_t* my = slots + c * kIndexSlots;
    int32_t st = CFWS_H2_PARSE_COMPLETE;
    while (e > p) {
        if (e - p < 9) { st = CFWS_H2_PARSE_MORE_DATA; break; }
        const H2Hop h = h2_index_hop(buf, p, e, max_frame);
        st = h.status;
        if (st != CFWS_H2_PARSE_COMPLETE) break;
        if (h2_selected(h, select, stream_id)) {
            if (k < kIndexSlots) my[k] = p;
            else if (k == kIndexSlots) r = p;
            ++k;
        }
        p += h.advance;
    }
    first[c] = k;
    consumed[c] = p;
    stop[c] = st;
    resume[c] = r;
}

// The records of the kept starts: thread (c, j) re-derives connection c's
// j-th selected frame from the bytes at its kept start (one round of
// independent loads per thread; the walk found the frame COMPLETE, so the
// same rule gives the same answer) and stores it at the start's place.
__global__ void __launch_bounds__(kThreads)
h2_index_info_kernel(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ end,
                     const uint64_t* __restrict__ first, const uint64_t* __restrict__ slots,
                     const uint64_t* __restrict__ total, uint64_t n, uint32_t max_frame,
                     cfws_h2_frame_info_t* __restrict__ info, uint64_t cap)
{
    const uint64_t t = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t c = t / kIndexSlots, j = t % kIndexSlots;
    if (c >= n) return;
    const uint64_t next = c + 1 < n ? first[c + 1] : *total;
    const uint64_t k = next - first[c];
    if (j < k && first[c] + j < cap) store_info(info, first[c] + j, h2_index_hop(buf, slots[t], end[c], max_frame));
}

// Connections with more than kIndexSlots selected frames: the walk on from
// selected frame kIndexSlots, writing the rest of their starts and records
// in place. Every frame on the way is one the first walk found COMPLETE.
__global__ void __launch_bounds__(kThreads)
h2_index_rest_kernel(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ end, uint64_t n,
                     uint32_t max_frame, uint32_t select, uint32_t stream_id,
                     const uint64_t* __restrict__ first, const uint64_t* __restrict__ total,
                     const uint64_t* __restrict__ resume, uint64_t* __restrict__ starts,
                     cfws_h2_frame_info_t* __restrict__ info, uint64_t cap)
{
    const uint64_t c = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (c >= n) return;
    uint64_t next = c + 1 < n ? first[c + 1] : *total;
    if (next - first[c] <= kIndexSlots) return;
    if (next > cap) next = cap;                                  // places past the capacity are not written
    const uint64_t e = end[c];
    uint64_t p = resume[c];
    if (p >= e) return;                 // never (a selected frame starts at p); settles both loads before the loop
    for (uint64_t k = first[c] + kIndexSlots; k < next;) {
        const H2Hop h = h2_index_hop(buf, p, e, max_frame);
        if (h2_selected(h, select, stream_id)) {
            starts[k] = p;
            if (info) store_info(info, k, h);
            ++k;
        }
        p += h.advance;
    }
}

}  // namespace

extern "C" {

size_t cfws_h2_index_workspace_size(size_t n_conns)
{
    return (size_t)index_layout(n_conns).bytes;
}

int cfws_h2_index_frames_batch(const void* d_buf, const uint64_t* d_begin, const uint64_t* d_end, size_t n,
                               uint32_t max_frame_size, uint32_t select, uint32_t stream_id,
                               uint64_t* d_starts, cfws_h2_frame_info_t* d_info, uint64_t cap,
                               uint64_t* d_first, uint64_t* d_consumed, int32_t* d_stop,
                               uint64_t* d_total, void* ws, size_t ws_size, void* stream)
{
    const CfwsPassScope pass_scope;     // not a timed pass: a pending pair is dropped
    if (int rc = check_init()) return rc;
    if ((n && (!d_buf || !d_begin || !d_end || !d_first || !d_consumed || !d_stop)) ||
        (cap && !d_starts) || !d_total || !ws)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "h2 index: null pointer", hipSuccess);
    if (select > CFWS_H2_INDEX_DATA)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "h2 index: select must be CFWS_H2_INDEX_ALL or _DATA",
                       hipSuccess);
    if (reinterpret_cast<uintptr_t>(d_info) & 15u)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "h2 index: d_info must be 16-byte aligned", hipSuccess);
    if (ws_size < cfws_h2_index_workspace_size(n))
        return set_err(CFWS_ERROR_WORKSPACE, "h2 index workspace too small", hipSuccess);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) {
        (void)hipMemsetAsync(d_total, 0, 8, st);
        return launch_check("h2 index");
    }
    const uint8_t* buf = static_cast<const uint8_t*>(d_buf);
    const uint32_t mfs = max_frame_size ? max_frame_size : CFWS_H2_DEFAULT_MAX_FRAME_SIZE;
    const IndexLayout L = index_layout(n);
    uint64_t* slots = ws_ptr<uint64_t>(ws, L.slots);
    uint64_t* resume = ws_ptr<uint64_t>(ws, L.resume);
    const uint32_t g = grid_for(n, kThreads);
    h2_index_walk_kernel<<<g, kThreads, 0, st>>>(buf, d_begin, d_end, n, mfs, select, stream_id, d_first,
                                                 d_consumed, d_stop, slots, resume);
    if (int rc = run_scan(d_first, n, ws_ptr<uint64_t>(ws, L.partials), d_total, st)) return rc;
    if (cap) {
        const uint32_t gs = grid_for(n * kIndexSlots, kThreads);
        index_place_kernel<<<gs, kThreads, 0, st>>>(d_first, slots, d_total, n, d_starts, cap);
        if (d_info)
            h2_index_info_kernel<<<gs, kThreads, 0, st>>>(buf, d_end, d_first, slots, d_total, n, mfs, d_info,
                                                          cap);
        h2_index_rest_kernel<<<g, kThreads, 0, st>>>(buf, d_end, n, mfs, select, stream_id, d_first, d_total,
                                                     resume, d_starts, d_info, cap);
    }
    return launch_check("h2 index");
}

}  // extern "C"
