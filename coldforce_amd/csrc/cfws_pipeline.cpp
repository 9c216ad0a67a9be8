// cfws_pipeline.cpp -- host-memory batch codec (include/cfws.h, cfws_pipeline_*).
//
// coldforce's frames start and end in host memory: socket receive buffers
// (co_tcp_receive_all, src/net/co_tcp_client.c:695-721) and send buffers
// (co_ws_send -> module.send, src/ws/co_ws_client.c:427-460). This pipeline
// runs the device batch codec over host buffers: the batch is cut into
// chunks of frames, and `depth` slots, each with its own stream and device
// staging, overlap H2D copies, the plan + streaming kernels and D2H copies of
// consecutive chunks (the two DMA directions run concurrently). H2D copies go
// in chunk order on one copy stream of the pipeline's, each waiting only for
// its slot's previous execute (the input staging free), never for a D2H: on a
// slot's own stream the next chunk's H2D would queue behind the slot's D2H,
// and all slots then alternate between an H2D burst and a D2H burst (half
// duplex). D2H copies stay on the slot streams (one shared
// in-order D2H stream measured no faster). The host
// buffers should be pinned (hipHostMalloc / hipHostRegister) for full PCIe
// rate. All codec decisions (header encode/decode, layout, status codes) are
// the device plan's; the host only cuts chunks (cfws_chunks.h) and rebases
// offsets.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "cfws.h"
#include "cfws_chunks.h"
#include "cfws_internal.h"

namespace {

constexpr int kMaxDepth = 4;

// One chunk in flight. The slot protocol, which event guards which buffer:
//   ev_in    (st_in) the chunk's H2D copies landed: the slot's stream may
//            start the chunk's kernels (take_in), and the H2D has read
//            h_stage. The send loop waits for it on the host before it fills
//            h_stage again. A receive's h_stage is also where its metadata
//            lands, so it is refilled only after ev_done, which implies ev_in
//            (no host wait of its own: that loop's host time is not hidden).
//   ev_exec  (st)    the chunk's kernels finished: d_in and d_desc / d_index
//            are free, so st_in may copy the slot's next chunk in.
//   ev_total (st)    h_total holds the chunk's unclamped layout total
//            (receive: the next chunk's payload base).
//   ev_done  (st)    the chunk's last D2H finished: the caller's output bytes
//            and, on receive, the metadata in h_stage have landed; d_out is
//            free. The receive's landing queue waits for it before it
//            rebases out of h_stage, and so before the staging is refilled.
// Every call leaves through the Call guard below, which drains st_in and all
// slot streams: between calls every event is complete.
struct Slot {
    hipStream_t st = nullptr;
    void* d_in = nullptr;              // chunk source (payload or wire)
    void* d_out = nullptr;             // chunk output
    cfws_frame_desc_t* d_desc = nullptr;
    int32_t* d_status = nullptr;
    uint64_t *d_index = nullptr, *d_total = nullptr;
    void* d_ws = nullptr;
    size_t ws_size = 0;
    void* h_stage = nullptr;           // pinned: descriptors / index / status staging
    // where in h_stage a receive's metadata lands, max_frames entries each:
    // descriptors, statuses, HTTP/2 message statuses
    cfws_frame_desc_t* h_desc = nullptr;
    int32_t *h_status = nullptr, *h_status2 = nullptr;
    uint64_t* h_total = nullptr;       // pinned
    hipEvent_t ev_in = nullptr, ev_exec = nullptr, ev_total = nullptr, ev_done = nullptr;
    // HTTP/2 (cfws_pipeline_h2_*), allocated at first use: WS wire / pool
    // scratch, message statuses and the HTTP/2 workspace
    void *d_aux = nullptr, *d_ws2 = nullptr;
    int32_t* d_status2 = nullptr;
    size_t ws2_size = 0;
};

int fail(const char* what, hipError_t e = hipSuccess)
{
    fprintf(stderr, "cfws pipeline: %s%s%s\n", what, e == hipSuccess ? "" : ": ",
            e == hipSuccess ? "" : hipGetErrorString(e));
    return e == hipSuccess ? CFWS_ERROR_INVALID_ARGUMENT : CFWS_ERROR_HIP;
}

// A call's output arena in host memory. dev: its device address when the D2H
// leg is a kernel (copy_out_kernel storing into mapped pinned memory), NULL
// for an SDMA copy (and for an empty batch, which copies nothing).
// Measured per direction with the H2D copies on their own stream (config 2,
// host to host): serialize 40 GiB/s with the kernel against 22
// with SDMA; deserialize 44 GiB/s with SDMA against 35 with the kernel. So
// CFWS_PIPELINE_D2H_AUTO takes the kernel for serialize when its wire arena
// is mapped and always copies for deserialize.
struct HostOut {
    uint8_t *host, *dev;
    uint64_t capacity;
};

HostOut host_out(int mode, void* h_out, uint64_t capacity, bool serialize, bool any_frames)
{
    const bool sdma = !any_frames || mode == CFWS_PIPELINE_D2H_DMA || (mode == CFWS_PIPELINE_D2H_AUTO && !serialize);
    return {static_cast<uint8_t*>(h_out), sdma ? nullptr : static_cast<uint8_t*>(cfws_mapped_device_pointer(h_out)),
            capacity};
}

// The default mode: CFWS_PIPELINE_D2H=dma | kernel | auto (unset: auto).
int default_d2h_mode()
{
    const char* s = getenv("CFWS_PIPELINE_D2H");
    if (s && strcmp(s, "dma") == 0) return CFWS_PIPELINE_D2H_DMA;
    if (s && strcmp(s, "kernel") == 0) return CFWS_PIPELINE_D2H_KERNEL;
    return CFWS_PIPELINE_D2H_AUTO;
}

#define CFWS_HIP(call)                                   \
    do {                                                 \
        hipError_t e_ = (call);                          \
        if (e_ != hipSuccess) return fail(#call, e_);    \
    } while (0)

}  // namespace

struct cfws_pipeline {
    hipStream_t st_in = nullptr;       // every H2D copy, in chunk order
    int d2h_mode = CFWS_PIPELINE_D2H_AUTO;
    int depth = 0;
    uint64_t chunk = 0;        // staging bytes per slot and direction
    size_t max_frames = 0;     // frames per chunk
    Slot slot[kMaxDepth];
};

// Waits for everything the pipeline has queued: st_in and every slot stream,
// whatever the earlier ones report. The first error, if any.
static hipError_t sync_all(const cfws_pipeline* p)
{
    hipError_t first = p->st_in ? hipStreamSynchronize(p->st_in) : hipSuccess;
    for (const Slot& S : p->slot)
        if (S.st) {
            const hipError_t e = hipStreamSynchronize(S.st);
            if (first == hipSuccess) first = e;
        }
    return first;
}

extern "C" {

int cfws_pipeline_create(uint64_t chunk_bytes, size_t max_frames, int depth, cfws_pipeline_t** out)
{
    if (int rc = cfws_init()) return rc;
    if (!out || depth < 1 || depth > kMaxDepth || chunk_bytes < 4096 || max_frames == 0)
        return fail("bad pipeline parameters");
    auto* p = new cfws_pipeline;
    p->depth = depth;
    p->chunk = (chunk_bytes + 255) & ~uint64_t(255);
    p->max_frames = max_frames;
    p->d2h_mode = default_d2h_mode();
    // The deserialize output of a chunk can exceed its wire bytes only by
    // the alignment padding; reserve one 4 KiB pad per frame at most.
    const uint64_t out_bytes = p->chunk + 64;
    if (hipStreamCreateWithFlags(&p->st_in, hipStreamNonBlocking) != hipSuccess) {
        cfws_pipeline_destroy(p);
        return fail("pipeline allocation failed");
    }
    for (int s = 0; s < depth; ++s) {
        Slot& S = p->slot[s];
        S.ws_size = cfws_workspace_size(max_frames, out_bytes);
        if (hipStreamCreateWithFlags(&S.st, hipStreamNonBlocking) != hipSuccess ||
            hipMalloc(&S.d_in, p->chunk + 64) != hipSuccess ||
            hipMalloc(&S.d_out, out_bytes) != hipSuccess ||
            hipMalloc(&S.d_desc, max_frames * sizeof(cfws_frame_desc_t)) != hipSuccess ||
            hipMalloc(&S.d_status, max_frames * sizeof(int32_t)) != hipSuccess ||
            hipMalloc(&S.d_index, max_frames * sizeof(uint64_t)) != hipSuccess ||
            hipMalloc(&S.d_total, 64) != hipSuccess ||
            hipMalloc(&S.d_ws, S.ws_size) != hipSuccess ||
            hipHostMalloc(&S.h_stage, max_frames * (sizeof(cfws_frame_desc_t) + 2 * sizeof(int32_t))) != hipSuccess ||
            hipHostMalloc(reinterpret_cast<void**>(&S.h_total), 64) != hipSuccess ||
            hipEventCreateWithFlags(&S.ev_done, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&S.ev_total, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&S.ev_in, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&S.ev_exec, hipEventDisableTiming) != hipSuccess) {
            cfws_pipeline_destroy(p);
            return fail("pipeline allocation failed");
        }
        S.h_desc = static_cast<cfws_frame_desc_t*>(S.h_stage);
        S.h_status = reinterpret_cast<int32_t*>(S.h_desc + max_frames);
        S.h_status2 = S.h_status + max_frames;
        (void)hipEventRecord(S.ev_done, S.st);
        (void)hipEventRecord(S.ev_exec, S.st);
        (void)hipEventRecord(S.ev_in, p->st_in);
    }
    *out = p;
    return CFWS_OK;
}

void cfws_pipeline_destroy(cfws_pipeline_t* p)
{
    if (!p) return;
    (void)sync_all(p);
    for (Slot& S : p->slot) {
        for (void* d : {S.d_in, S.d_out, (void*)S.d_desc, (void*)S.d_status, (void*)S.d_index, (void*)S.d_total,
                        S.d_ws, S.d_aux, (void*)S.d_status2, S.d_ws2})
            if (d) (void)hipFree(d);
        for (void* h : {S.h_stage, (void*)S.h_total})
            if (h) (void)hipHostFree(h);
        for (hipEvent_t e : {S.ev_in, S.ev_exec, S.ev_total, S.ev_done})
            if (e) (void)hipEventDestroy(e);
        if (S.st) (void)hipStreamDestroy(S.st);
    }
    if (p->st_in) (void)hipStreamDestroy(p->st_in);
    delete p;
}

int cfws_pipeline_set_d2h(cfws_pipeline_t* p, int mode)
{
    if (!p || mode < CFWS_PIPELINE_D2H_AUTO || mode > CFWS_PIPELINE_D2H_KERNEL) return fail("bad D2H mode");
    p->d2h_mode = mode;
    return CFWS_OK;
}

}  // extern "C"

// ---- the pieces every call is built from -----------------------------------

namespace {

using namespace cfws_chunks;

// The prologue of every pipeline call: the pass scope with its pair dropped
// (a pipeline call is not timed, cfws_time_next_pass), and the drain. On every
// return, success or error, nothing of the pipeline is in flight: no H2D is
// still reading the caller's input, no D2H still writing its output or a
// slot's h_stage. (After a receive's last finish all work is complete and the
// synchronisations return at once.)
struct Call {
    const CfwsPassScope pass_scope;
    cfws_pipeline* const p;
    explicit Call(cfws_pipeline* pipeline) : p(pipeline) { (void)cfws_internal_take_pass(); }
    ~Call() { if (p) (void)sync_all(p); }
    // the same wait, reported: how a call whose last step is not a wait ends
    int drain() const
    {
        CFWS_HIP(sync_all(p));
        return CFWS_OK;
    }
};

int check_align(uint32_t align)
{
    if (align == 0 || (align & (align - 1)) || align > 4096) return fail("bad align");
    return CFWS_OK;
}

int check_increasing(const uint64_t* h_index, size_t n)
{
    for (size_t i = 1; i < n; ++i)
        if (h_index[i] < h_index[i - 1]) return fail("frame index must be increasing");
    return CFWS_OK;
}

// H2D of a chunk on st_in: `bytes` input bytes from h_src into d_in, and the
// per-frame staging (descriptors or index) the caller wrote into h_stage into
// d_frames.
int stage_in(cfws_pipeline* p, Slot& S, const uint8_t* h_src, uint64_t bytes, void* d_frames, size_t frames_bytes)
{
    CFWS_HIP(hipStreamWaitEvent(p->st_in, S.ev_exec, 0));   // d_in, d_desc / d_index free
    CFWS_HIP(hipMemcpyAsync(S.d_in, h_src, bytes, hipMemcpyHostToDevice, p->st_in));
    CFWS_HIP(hipMemcpyAsync(d_frames, S.h_stage, frames_bytes, hipMemcpyHostToDevice, p->st_in));
    CFWS_HIP(hipEventRecord(S.ev_in, p->st_in));
    return CFWS_OK;
}

// The slot's stream waits for the staged chunk. Queued when the chunk is
// about to be launched, not when it is staged ahead (the HTTP/2 receive): a
// wait on a copy that has not finished is a barrier in the stream's hardware
// queue, which streams share, and queued a chunk early it held up the
// running chunk's kernels (config 5 deserialize 42.4 -> 34.9 GiB/s).
int take_in(Slot& S)
{
    CFWS_HIP(hipStreamWaitEvent(S.st, S.ev_in, 0));
    return CFWS_OK;
}

// The D2H leg on the slot's stream: d_out[0, bytes) to the output arena at
// `off`, clamped to its capacity.
int copy_back(Slot& S, const HostOut& out, uint64_t off, uint64_t bytes)
{
    if (off >= out.capacity || bytes == 0) return CFWS_OK;
    const uint64_t m = std::min(bytes, out.capacity - off);
    if (out.dev) return cfws_internal_copy_out(S.d_out, out.dev + off, m, S.st);
    CFWS_HIP(hipMemcpyAsync(out.host + off, S.d_out, m, hipMemcpyDeviceToHost, S.st));
    return CFWS_OK;
}

// A slot's HTTP/2 resources, allocated at first use: WS wire / pool scratch,
// message statuses, and an HTTP/2 workspace of at least ws_bytes.
int h2_slot(cfws_pipeline* p, Slot& S, size_t ws_bytes)
{
    if ((!S.d_aux && hipMalloc(&S.d_aux, p->chunk + 64) != hipSuccess) ||
        (!S.d_status2 && hipMalloc(&S.d_status2, p->max_frames * sizeof(int32_t)) != hipSuccess))
        return fail("pipeline allocation failed");
    if (S.ws2_size < ws_bytes) {
        if (S.d_ws2) {
            (void)hipStreamSynchronize(S.st);
            (void)hipFree(S.d_ws2);
            S.d_ws2 = nullptr;
            S.ws2_size = 0;
        }
        if (hipMalloc(&S.d_ws2, ws_bytes) != hipSuccess) return fail("pipeline allocation failed");
        S.ws2_size = ws_bytes;
    }
    return CFWS_OK;
}

// ---- send ------------------------------------------------------------------

// What a send codec is: bytes(), a frame's byte sums for the cut
// (cfws_chunks.h); prepare(), the slot resources it needs beyond the common
// ones; launch(), its batch call over the slot's staged chunk.
struct WsSend {
    cfws_pipeline* p;
    FrameBytes bytes(const cfws_frame_desc_t& d) const { return ws_frame_bytes(d); }
    int prepare(Slot&) const { return CFWS_OK; }
    int launch(Slot& S, size_t nf) const
    {
        return cfws_serialize_batch(S.d_in, S.d_desc, nf, S.d_out, p->chunk + 64, S.d_total, S.d_ws, S.ws_size,
                                    S.st);
    }
};

struct H2Send {
    cfws_pipeline* p;
    uint32_t stream_id;
    uint64_t mfs, ws_bytes;
    FrameBytes bytes(const cfws_frame_desc_t& d) const { return h2_frame_bytes(d, mfs); }
    int prepare(Slot& S) const { return h2_slot(p, S, ws_bytes); }
    int launch(Slot& S, size_t nf) const
    {
        return cfws_h2_serialize_batch(S.d_in, S.d_desc, nf, stream_id, (uint32_t)mfs, S.d_aux, p->chunk + 64,
                                       S.d_out, p->chunk + 64, S.d_total, S.d_ws2, S.ws2_size, S.st);
    }
};

// The send loop: host payload arena -> host output stream. h_desc gets
// header_size / wire_off as cfws_serialize_plan writes them (the same rule on
// the host, so that chunks can be cut by bytes); *total the output's bytes,
// unclamped.
template <typename Codec>
int pipeline_send(const Call& call, const Codec& codec, const void* h_payload, cfws_frame_desc_t* h_desc,
                  size_t n, void* h_out, uint64_t capacity, uint64_t* total)
{
    cfws_pipeline* p = call.p;
    uint64_t wire_off = 0, out_bytes = 0;
    for (size_t f = 0; f < n; ++f) {
        const FrameBytes b = codec.bytes(h_desc[f]);
        h_desc[f].header_size = (uint8_t)header_size_of(h_desc[f].payload_size, h_desc[f].mask != 0);
        h_desc[f].wire_off = wire_off;
        wire_off += b.wire;
        out_bytes += b.out;
    }
    if (total) *total = out_bytes;
    const uint8_t* src = static_cast<const uint8_t*>(h_payload);
    const HostOut out = host_out(p->d2h_mode, h_out, capacity, true, n != 0);
    uint64_t out_lo = 0;
    size_t i = 0;
    for (int c = 0; i < n; ++c) {
        const SendCut cut = send_cut(h_desc, n, i, p->chunk, p->max_frames, codec);
        if (!cut.fits) return fail("a frame is larger than the pipeline chunk");
        Slot& S = p->slot[c % p->depth];
        if (int rc = codec.prepare(S)) return rc;
        CFWS_HIP(hipEventSynchronize(S.ev_in));       // the slot's last H2D read the staging
        auto* stage = static_cast<cfws_frame_desc_t*>(S.h_stage);
        for (size_t k = i; k < cut.j; ++k) {
            stage[k - i] = h_desc[k];
            stage[k - i].payload_off -= cut.src_lo;
        }
        if (int rc = stage_in(p, S, src + cut.src_lo, cut.src_hi - cut.src_lo, S.d_desc,
                              (cut.j - i) * sizeof(cfws_frame_desc_t)))
            return rc;
        if (int rc = take_in(S)) return rc;
        if (int rc = codec.launch(S, cut.j - i)) return rc;
        CFWS_HIP(hipEventRecord(S.ev_exec, S.st));
        if (int rc = copy_back(S, out, out_lo, cut.out)) return rc;
        CFWS_HIP(hipEventRecord(S.ev_done, S.st));
        out_lo += cut.out;
        i = cut.j;
    }
    return call.drain();
}

// ---- receive ---------------------------------------------------------------

// The frame starts a chunked receive consumes: a caller's index, or a receive
// loop's walk (cfws_index_frames, co_ws_server.c:107-169; cfws_h2_index_frames,
// co_http2_client.c:462-541) run in steps of kStep frames, so the index grows
// with the frames found and not with the caller's capacity. Asked for a start
// it does not have yet, it walks on: cfws_pipeline_receive's walk so runs just
// ahead of its chunks, and the host walks chunk c + 1's frames while the
// device copies and decodes chunk c (the walk is a chain of dependent reads
// through host memory, ~100 ns per frame).
struct StartSource {
    // one step of the walk from pos: up to `room` starts; *used, *why as the
    // index call reports them
    using Walk = std::function<size_t(uint64_t pos, uint64_t* starts, size_t room, uint64_t* used, int32_t* why)>;

    const uint64_t* fixed = nullptr;     // a caller's index of n_fixed starts
    size_t n_fixed = 0;
    Walk walk;                           // or the walk from pos
    uint64_t pos = 0;
    size_t cap = 0;                      // at most this many starts
    std::vector<uint64_t> walked;
    int32_t stop = CFWS_PARSE_COMPLETE;
    bool done = true;
    static constexpr size_t kStep = 2048;

    StartSource(const uint64_t* h_index, size_t n) : fixed(h_index), n_fixed(n) {}
    StartSource(Walk w, uint64_t begin, size_t max_starts) : walk(std::move(w)), pos(begin), cap(max_starts), done(false)
    {
        walked.reserve(std::min(cap, size_t(1) << 20));
    }

    // Does start k exist? (walks on until it is known)
    bool has(size_t k)
    {
        if (fixed) return k < n_fixed;
        while (k >= walked.size() && !done) step();
        return k < walked.size();
    }
    uint64_t at(size_t k) const { return fixed ? fixed[k] : walked[k]; }
    // Where the last frame's bytes end (has() said there is no next start):
    // the walk's stop, so trailing incomplete bytes are never staged.
    uint64_t last_end(uint64_t wire_size) const { return fixed ? wire_size : std::min(pos, wire_size); }
    // Stepwise walks end as one walk over the whole buffer would:
    // CFWS_INDEX_FULL only when another selected frame follows.
    void step()
    {
        const size_t at0 = walked.size();
        const size_t room = std::min(kStep, cap - at0);
        walked.resize(at0 + room);
        uint64_t used = pos;
        int32_t why = CFWS_PARSE_COMPLETE;
        const size_t got = walk(pos, walked.data() + at0, room, &used, &why);
        walked.resize(at0 + got);
        pos = used;
        stop = why;
        if (why != CFWS_INDEX_FULL || walked.size() == cap) done = true;
    }
    void walk_to_end() { while (!done) step(); }
};

// One receive chunk, from its cut (frames [i, j) of the index) to its rebase.
struct Chunk : RecvCut {
    size_t i;
    int slot;
    size_t nd = 0;                      // descriptors it produced (launch)
    // known once settled:
    size_t m0 = 0;                      // its first descriptor's place in the caller's
    uint64_t base = 0, pool_base = 0;   // payload / pool bytes laid out by earlier chunks
};

// What a receive form is: kMessages, whether descriptors are per pooled
// message (with statuses of their own) and not per frame; prepare(), the
// slot resources beyond the common ones; launch(), its batch call under
// output capacity cap, which sets k.nd and says where on the device the
// unclamped layout total is; rebase(), a landed chunk's h_stage into the
// caller's arrays.
struct WsRecv {
    static constexpr bool kMessages = false;
    cfws_pipeline* p;
    uint64_t max_payload;
    uint32_t align;
    cfws_frame_desc_t* h_desc;           // the caller's arrays
    int32_t* h_status;
    int prepare(Slot&) const { return CFWS_OK; }
    // cap == 0 (capacity exhausted): the plan marks every non-empty COMPLETE
    // frame OUT_OF_MEMORY, exactly the batch rule.
    int launch(Slot& S, Chunk& k, uint64_t cap, const void** d_total) const
    {
        k.nd = k.j - k.i;
        *d_total = static_cast<char*>(S.d_ws) + cfws_internal_grand_total_offset();
        return cfws_deserialize_batch(S.d_in, k.hi - k.wire_lo, S.d_index, k.j - k.i, max_payload, align, 0,
                                      S.d_desc, S.d_status, S.d_out, cap, S.d_total, S.d_ws, S.ws_size, S.st);
    }
    void rebase(const Slot& S, const Chunk& k) const
    {
        for (size_t f = k.i; f < k.j; ++f) {
            h_desc[f] = S.h_desc[f - k.i];
            h_desc[f].wire_off += k.wire_lo;
            h_desc[f].payload_off += k.base;
            h_status[f] = S.h_status[f - k.i];
        }
    }
};

struct H2Recv {
    static constexpr bool kMessages = true;
    cfws_pipeline* p;
    uint64_t mfs, max_payload;
    uint32_t align;
    int32_t* h_h2_status;
    cfws_frame_desc_t* h_msg_desc;
    int32_t* h_msg_status;
    size_t ws_bytes;
    uint64_t pool_cap() const { return p->chunk + 64; }
    int prepare(Slot& S) const { return h2_slot(p, S, ws_bytes); }
    // synchronises for the chunk's message count
    int launch(Slot& S, Chunk& k, uint64_t cap, const void** d_total) const
    {
        *d_total = static_cast<char*>(S.d_ws2) + cfws_internal_h2_grand_total_offset(k.j - k.i, pool_cap(), cap);
        return cfws_h2_deserialize_batch(S.d_in, k.hi - k.wire_lo, S.d_index, k.j - k.i, (uint32_t)mfs, S.d_status,
                                         S.d_aux, pool_cap(), max_payload, align, S.d_desc, S.d_status2, S.d_out,
                                         cap, S.d_total, &k.nd, S.d_ws2, S.ws2_size, S.st);
    }
    void rebase(const Slot& S, const Chunk& k) const
    {
        for (size_t f = k.i; f < k.j; ++f) h_h2_status[f] = S.h_status[f - k.i];
        for (size_t m = 0; m < k.nd; ++m) {
            h_msg_desc[k.m0 + m] = S.h_desc[m];
            h_msg_desc[k.m0 + m].payload_off += k.base;
            h_msg_desc[k.m0 + m].wire_off += k.pool_base;
            h_msg_status[k.m0 + m] = S.h_status2[m];
        }
    }
};

// The receive core: a chunk goes through stage (H2D), launch (the batch call
// and the read of its layout total), settle (the total is on the host: D2H of
// payload and metadata, the bases move on) and finish (the copies landed:
// rebase into the caller's arrays). The two forms below differ in when they
// call these, not in what they do.
template <typename Form, typename Index>
struct Receive {
    cfws_pipeline* p;
    const Form& form;
    Index& idx;
    const uint8_t* src;
    HostOut out;
    std::vector<Chunk> landing;      // settled; not finished yet
    uint64_t base = 0, pool_base = 0;   // payload / pool bytes laid out by settled chunks
    size_t m0 = 0;                      // descriptors produced by settled chunks

    // A slot's staging is free once its last chunk is finished (and every
    // chunk before it, in order).
    int free_slot(int s)
    {
        for (size_t q = 0; q < landing.size(); ++q)
            if (landing[q].slot == s) {
                for (size_t r = 0; r <= q; ++r)
                    if (int rc = finish(landing[r])) return rc;
                landing.erase(landing.begin(), landing.begin() + q + 1);
                break;
            }
        return CFWS_OK;
    }
    int stage(const Chunk& k)
    {
        Slot& S = p->slot[k.slot];
        if (int rc = free_slot(k.slot)) return rc;
        if (int rc = form.prepare(S)) return rc;
        // the staging's last reader and writer, the slot's previous chunk, was finished above
        auto* sidx = static_cast<uint64_t*>(S.h_stage);
        for (size_t f = k.i; f < k.j; ++f) sidx[f - k.i] = idx.at(f) - k.wire_lo;
        return stage_in(p, S, src + k.wire_lo, k.hi - k.wire_lo, S.d_index, (k.j - k.i) * sizeof(uint64_t));
    }
    // The capacity rule needs the chunk's payload base: every earlier chunk
    // must be settled.
    int launch(Chunk& k)
    {
        Slot& S = p->slot[k.slot];
        const uint64_t cap = base >= out.capacity ? 0 : std::min(p->chunk + 64, out.capacity - base);
        const void* d_total = nullptr;
        if (int rc = form.launch(S, k, cap, &d_total)) return rc;
        CFWS_HIP(hipEventRecord(S.ev_exec, S.st));
        // the unclamped layout total: offsets keep counting past the capacity
        CFWS_HIP(hipMemcpyAsync(S.h_total, d_total, 8, hipMemcpyDeviceToHost, S.st));
        CFWS_HIP(hipEventRecord(S.ev_total, S.st));
        return CFWS_OK;
    }
    // Does not wait for the copies it enqueues, so the next chunk's kernels
    // overlap them.
    int settle(Chunk k)
    {
        Slot& S = p->slot[k.slot];
        CFWS_HIP(hipEventSynchronize(S.ev_total));
        const uint64_t tot = k.nd ? *S.h_total : 0;
        if (int rc = copy_back(S, out, base, tot)) return rc;
        if (k.nd)
            CFWS_HIP(hipMemcpyAsync(S.h_desc, S.d_desc, k.nd * sizeof(cfws_frame_desc_t), hipMemcpyDeviceToHost, S.st));
        CFWS_HIP(hipMemcpyAsync(S.h_status, S.d_status, (k.j - k.i) * sizeof(int32_t), hipMemcpyDeviceToHost, S.st));
        if (Form::kMessages && k.nd)
            CFWS_HIP(hipMemcpyAsync(S.h_status2, S.d_status2, k.nd * sizeof(int32_t), hipMemcpyDeviceToHost, S.st));
        CFWS_HIP(hipEventRecord(S.ev_done, S.st));
        k.base = base;
        k.m0 = m0;
        k.pool_base = pool_base;
        landing.push_back(k);
        base += tot;
        m0 += k.nd;
        pool_base += k.pooled;
        return CFWS_OK;
    }
    int finish(const Chunk& k)
    {
        const Slot& S = p->slot[k.slot];
        CFWS_HIP(hipEventSynchronize(S.ev_done));
        form.rebase(S, k);
        return CFWS_OK;
    }
    // The call's end: every settled chunk lands and is rebased.
    int end(uint64_t* payload_total)
    {
        for (const Chunk& k : landing)
            if (int rc = finish(k)) return rc;
        if (payload_total) *payload_total = std::min(base, out.capacity);
        return CFWS_OK;
    }
};

// co_ws_frame_deserialize at every start of a host wire buffer: header decode,
// status, copy + unmask into the host payload arena laid out as
// cfws_deserialize_plan lays it out (flags = 0: the reassembly layout puts
// control frames after ALL data, which a chunked pass cannot know). A chunk's
// total is read only when the next chunk's capacity rule needs it (or its slot
// is staged again), so its kernels overlap the previous chunk's copies.
int pipeline_deserialize(const Call& call, const void* h_wire, uint64_t wire_size, StartSource& idx,
                         uint64_t max_payload, uint32_t align, cfws_frame_desc_t* h_desc, int32_t* h_status,
                         void* h_payload, uint64_t payload_capacity, uint64_t* payload_total)
{
    cfws_pipeline* p = call.p;
    const WsRecv form{p, max_payload, align, h_desc, h_status};
    Receive<WsRecv, StartSource> R{p, form, idx, static_cast<const uint8_t*>(h_wire),
                      host_out(p->d2h_mode, h_payload, payload_capacity, false, idx.has(0))};
    Chunk pend;                      // launched; layout total not read yet
    bool pending = false;
    auto settle_pending = [&]() -> int {
        if (!pending) return CFWS_OK;
        pending = false;
        return R.settle(pend);
    };
    size_t i = 0;
    for (int c = 0; idx.has(i); ++c) {
        const RecvCut cut = recv_cut(idx, wire_size, i, p->chunk, p->max_frames, align);
        if (!cut.fits) return fail("a frame is larger than the pipeline chunk");
        Chunk k{cut, i, c % p->depth};
        if (pending && pend.slot == k.slot)      // its staging is about to be reused
            if (int rc = settle_pending()) return rc;
        if (int rc = R.stage(k)) return rc;
        if (int rc = take_in(p->slot[k.slot])) return rc;
        if (int rc = settle_pending()) return rc;
        if (int rc = R.launch(k)) return rc;
        pend = k;
        pending = true;
        i = cut.j;
    }
    if (int rc = settle_pending()) return rc;
    return R.end(payload_total);
}

// co_http2_stream_receive_ws_frame over a host DATA-frame stream
// (cfws_h2_deserialize_batch per chunk): the DATA frames at the index ->
// HTTP/2 statuses, pooled messages -> co_ws_frame_deserialize -> payloads in
// the host arena, laid out as the batch call lays them out. Chunks end where
// no message is open (h2_recv_cut), so every message is decoded whole. The
// batch call synchronises for its message count, so each chunk is settled at
// once, and the next chunk's H2D is queued before the call (after it with one
// slot, which the chunk still occupies).
int pipeline_h2_deserialize(const Call& call, const void* h_h2, uint64_t h2_size, ArrayIndex idx,
                            uint32_t max_frame_size, uint64_t max_payload, uint32_t align, int32_t* h_h2_status,
                            cfws_frame_desc_t* h_msg_desc, int32_t* h_msg_status, size_t* n_messages,
                            void* h_payload, uint64_t payload_capacity, uint64_t* payload_total)
{
    cfws_pipeline* p = call.p;
    *n_messages = 0;
    if (payload_total) *payload_total = 0;
    if (!idx.has(0)) return CFWS_OK;
    const uint64_t mfs = max_frame_size ? max_frame_size : CFWS_H2_DEFAULT_MAX_FRAME_SIZE;
    const uint8_t* h2 = static_cast<const uint8_t*>(h_h2);
    const H2Recv form{p, mfs, max_payload, align, h_h2_status, h_msg_desc, h_msg_status,
                      cfws_h2_deserialize_workspace_size(p->max_frames, p->chunk + 64, p->chunk + 64)};
    Receive<H2Recv, ArrayIndex> R{p, form, idx, h2, host_out(p->d2h_mode, h_payload, payload_capacity, false, true)};
    auto next = [&](size_t i, int c, Chunk& k) -> int {
        const RecvCut cut = h2_recv_cut(idx, h2, h2_size, i, p->chunk, p->max_frames, align, mfs);
        if (!cut.fits) return fail("a message spans more bytes or DATA frames than a pipeline chunk holds");
        k = Chunk{cut, i, c % p->depth};
        return CFWS_OK;
    };
    Chunk cur, nxt;
    if (int rc = next(0, 0, cur)) return rc;
    if (int rc = R.stage(cur)) return rc;
    for (int c = 0;; ++c) {
        const bool more = idx.has(cur.j);
        if (more) {
            if (int rc = next(cur.j, c + 1, nxt)) return rc;
            if (p->depth > 1)
                if (int rc = R.stage(nxt)) return rc;
        }
        if (int rc = take_in(p->slot[cur.slot])) return rc;
        if (int rc = R.launch(cur)) return rc;
        if (int rc = R.settle(cur)) return rc;
        if (!more) break;
        if (p->depth == 1)
            if (int rc = R.stage(nxt)) return rc;
        cur = nxt;
    }
    if (int rc = R.end(payload_total)) return rc;
    *n_messages = R.m0;
    return CFWS_OK;
}

}  // namespace

// ---- the public calls ------------------------------------------------------

extern "C" {

// co_ws_frame_serialize over a host batch: host payload arena -> host wire.
int cfws_pipeline_serialize(cfws_pipeline_t* p, const void* h_payload, cfws_frame_desc_t* h_desc,
                            size_t n, void* h_wire, uint64_t wire_capacity, uint64_t* wire_total)
{
    const Call call(p);
    if (!p || (n && (!h_payload || !h_desc || !h_wire))) return fail("null argument");
    return pipeline_send(call, WsSend{p}, h_payload, h_desc, n, h_wire, wire_capacity, wire_total);
}

// co_http2_stream_send_ws_frame over a host batch (cfws_h2_serialize_batch
// per chunk of WS frames): host payload arena -> host DATA-frame stream.
int cfws_pipeline_h2_serialize(cfws_pipeline_t* p, const void* h_payload, cfws_frame_desc_t* h_desc,
                               size_t n, uint32_t stream_id, uint32_t max_frame_size, void* h_h2,
                               uint64_t h2_capacity, uint64_t* h2_total)
{
    const Call call(p);
    if (!p || (n && (!h_payload || !h_desc || !h_h2))) return fail("null argument");
    const uint64_t mfs = max_frame_size ? max_frame_size : CFWS_H2_DEFAULT_MAX_FRAME_SIZE;
    const size_t ws_bytes = cfws_h2_serialize_workspace_size(p->max_frames, p->chunk + 64, p->chunk + 64,
                                                             (uint32_t)mfs);
    return pipeline_send(call, H2Send{p, stream_id, mfs, ws_bytes}, h_payload, h_desc, n, h_h2, h2_capacity,
                         h2_total);
}

// Precondition (what a receive loop's index satisfies): h_index increasing
// and every frame ending at or before the next frame's start.
int cfws_pipeline_deserialize(cfws_pipeline_t* p, const void* h_wire, uint64_t wire_size,
                              const uint64_t* h_index, size_t n, uint64_t max_payload,
                              uint32_t align, uint32_t flags, cfws_frame_desc_t* h_desc,
                              int32_t* h_status, void* h_payload, uint64_t payload_capacity,
                              uint64_t* payload_total)
{
    const Call call(p);
    if (!p || (n && (!h_wire || !h_index || !h_desc || !h_status || !h_payload)))
        return fail("null argument");
    if (flags != 0) return fail("the pipeline supports flags = 0 only");
    if (int rc = check_align(align)) return rc;
    if (int rc = check_increasing(h_index, n)) return rc;
    StartSource idx(h_index, n);
    return pipeline_deserialize(call, h_wire, wire_size, idx, max_payload, align, h_desc, h_status, h_payload,
                                payload_capacity, payload_total);
}

// The receive loop's walk on the host, where the bytes are, a step ahead of
// the chunked device deserialize it drives. Every walked frame is COMPLETE
// inside [begin, consumed): the walk stops before an incomplete or invalid
// frame, whose bytes are never staged.
int cfws_pipeline_receive(cfws_pipeline_t* p, const void* h_wire, uint64_t begin, uint64_t end,
                          uint64_t max_payload, uint32_t align, cfws_frame_desc_t* h_desc,
                          int32_t* h_status, size_t* n_frames, uint64_t* consumed, int32_t* stop,
                          void* h_payload, uint64_t payload_capacity, uint64_t* payload_total)
{
    const Call call(p);
    if (!p || !n_frames || (end > begin && !h_wire)) return fail("null argument");
    if (*n_frames && (!h_desc || !h_status || !h_payload)) return fail("null argument");
    if (int rc = check_align(align)) return rc;
    StartSource idx(
        [=](uint64_t pos, uint64_t* starts, size_t room, uint64_t* used, int32_t* why) {
            return cfws_index_frames(h_wire, pos, end, max_payload, starts, room, used, why);
        },
        begin, *n_frames);
    const int rc = pipeline_deserialize(call, h_wire, end, idx, max_payload, align, h_desc, h_status, h_payload,
                                        payload_capacity, payload_total);
    idx.walk_to_end();                  // an error above may leave the walk short
    *n_frames = idx.walked.size();
    if (consumed) *consumed = idx.pos;
    if (stop) *stop = idx.stop;
    return rc;
}

// Same index precondition as cfws_pipeline_deserialize.
int cfws_pipeline_h2_deserialize(cfws_pipeline_t* p, const void* h_h2, uint64_t h2_size,
                                 const uint64_t* h_index, size_t n, uint32_t max_frame_size,
                                 uint64_t max_payload, uint32_t align, int32_t* h_h2_status,
                                 cfws_frame_desc_t* h_msg_desc, int32_t* h_msg_status,
                                 size_t* n_messages, void* h_payload, uint64_t payload_capacity,
                                 uint64_t* payload_total)
{
    const Call call(p);
    if (!p || !n_messages ||
        (n && (!h_h2 || !h_index || !h_h2_status || !h_msg_desc || !h_msg_status || !h_payload)))
        return fail("null argument");
    if (int rc = check_align(align)) return rc;
    if (int rc = check_increasing(h_index, n)) return rc;
    return pipeline_h2_deserialize(call, h_h2, h2_size, ArrayIndex{h_index, n}, max_frame_size, max_payload, align,
                                   h_h2_status, h_msg_desc, h_msg_status, n_messages, h_payload, payload_capacity,
                                   payload_total);
}

// The HTTP/2 receive loop over one connection's host buffer, for one stream:
// the walk (select = DATA + stream id) on the calling thread, then the chunked
// deserialize of the DATA frames found, over h_h2[0, *consumed). The plain
// composition: the walk finishes before the first chunk is staged
// (cfws_pipeline_receive's walk runs a step ahead of its chunks; this one does
// not).
int cfws_pipeline_h2_receive(cfws_pipeline_t* p, const void* h_h2, uint64_t begin, uint64_t end,
                             uint32_t stream_id, uint32_t max_frame_size, uint64_t max_payload,
                             uint32_t align, int32_t* h_h2_status, cfws_frame_desc_t* h_msg_desc,
                             int32_t* h_msg_status, size_t* n_frames, size_t* n_messages,
                             uint64_t* consumed, int32_t* stop, void* h_payload,
                             uint64_t payload_capacity, uint64_t* payload_total)
{
    const Call call(p);
    if (!p || !n_frames || !n_messages || (end > begin && !h_h2)) return fail("null argument");
    if (*n_frames && (!h_h2_status || !h_msg_desc || !h_msg_status || !h_payload)) return fail("null argument");
    if (int rc = check_align(align)) return rc;
    StartSource idx(
        [=](uint64_t pos, uint64_t* starts, size_t room, uint64_t* used, int32_t* why) {
            return cfws_h2_index_frames(h_h2, pos, end, max_frame_size, CFWS_H2_INDEX_DATA, stream_id, starts,
                                        nullptr, room, used, why);
        },
        begin, *n_frames);
    idx.walk_to_end();
    *n_frames = idx.walked.size();
    if (consumed) *consumed = idx.pos;
    if (stop) *stop = idx.stop;
    // the whole index is in hand: the chunks are cut over the plain array
    return pipeline_h2_deserialize(call, h_h2, idx.pos, ArrayIndex{idx.walked.data(), idx.walked.size()},
                                   max_frame_size, max_payload, align, h_h2_status, h_msg_desc, h_msg_status,
                                   n_messages, h_payload, payload_capacity, payload_total);
}

}  // extern "C"
