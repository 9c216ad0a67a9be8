// cfws_relay.hip -- cfws_relay_batch: received frames sent
// on in one payload pass. A server that echoes, a proxy that re-masks and a
// fan-out all run co_ws_frame_deserialize and then co_ws_frame_serialize on
// the same payload (examples/ws_server/main.c:54-71, co_ws_client.c:428-460,
// :563-600); here one plan parses every frame and lays out its outgoing
// frame, and one streaming pass (xform_kernel<kModeRelay>, cfws_kernels.h)
// writes the new header and out[k] = in[k] ^ key_in[k % 4] ^ key_out[k % 4]
// straight from the incoming wire: no payload arena in between.
//
// Layout: every input frame keeps its index -- a frame that emits nothing is
// a zero-size entry (pre = 0, body_len = 0), as a frame that is not COMPLETE
// is in the receive. The user's d_desc / d_status / d_out_keys, the offsets,
// the region map and the internal descriptors are then all indexed by the
// input frame, and the plan needs one scan (a compacted layout needs a second
// one, of the emitted count, and an indirection from entry to frame).
#include "cfws_kernels.h"

namespace {

// What frame (st, fin, opcode) sends under `policy`: false = nothing; else
// the outgoing fin and opcode.
//   CFWS_RELAY_VERBATIM:    every COMPLETE frame as it came;
//   CFWS_RELAY_ECHO_SERVER: CONTINUATION / TEXT / BINARY as they came
//     (examples/ws_server/main.c:56-62), PING as a final PONG on the same
//     payload (co_ws_client.c:586-591, :552-560), nothing else.
__device__ __forceinline__ bool relay_decision(uint32_t policy, int32_t st, uint32_t fin, uint32_t opcode,
                                               uint32_t& out_fin, uint32_t& out_opcode)
{
    out_fin = fin;
    out_opcode = opcode;
    if (st != CFWS_PARSE_COMPLETE) return false;
    if (policy == CFWS_RELAY_VERBATIM || opcode <= 0x2u) return true;
    if (opcode != 0x9u) return false;
    out_fin = 1u;
    out_opcode = 0xAu;
    return true;
}

// Step 1, one thread per frame: the header decode of cfws_parse_headers into
// the user's tables, the policy decision, the outgoing bytes (vals) and the
// block's sum.
__global__ void __launch_bounds__(kThreads)
relay_plan_reduce_kernel(const uint8_t* __restrict__ wire, uint64_t wire_size, const uint64_t* __restrict__ index,
                         uint64_t n, uint64_t max_payload, uint32_t policy, uint32_t out_mask,
                         cfws_frame_desc_t* __restrict__ desc, int32_t* __restrict__ status,
                         uint64_t* __restrict__ vals, uint64_t* __restrict__ partials)
{
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t b0 = uint64_t(blockIdx.x) * kPlanBlock;
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kPlanItems; ++k) {
        const uint64_t f = b0 + uint64_t(k) * kThreads + threadIdx.x;
        if (f >= n) continue;
        cfws_frame_desc_t d;
        const int32_t st = parse_ws_header(wire, wire_size, index[f], max_payload, d);
        desc[f] = d;
        status[f] = st;
        uint32_t of, oo;
        const bool emit = relay_decision(policy, st, d.fin, d.opcode, of, oo);
        const uint64_t v = emit ? ser_wire_bytes(header_size_of(d.payload_size, out_mask != 0), d.payload_size) : 0;
        vals[f] = v;
        sum += v;
    }
    uint64_t total;
    block_exclusive_scan(sum, s_wave, &total);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// Step 2: each frame's offset in the outgoing wire (into vals, and the
// user's payload_off: written for frames that emit nothing too), the region
// map, the totals (the send's: the caller gets the unclamped one) and the
// frame's internal descriptor for the streaming pass (frame_view<kModeRelay>):
//   payload_off   the body's offset in the incoming wire (start + h_in)
//   wire_off      the outgoing header's key (0 when out_mask == 0)
//   payload_size  the body's length (0: nothing emitted)
//   mask_key      the body key: incoming ^ outgoing, an unmasked side 0
//   fin, opcode   the outgoing header's byte 0;  mask: out_mask
//   header_size   the outgoing header's size (0: nothing emitted)
__global__ void __launch_bounds__(kThreads)
relay_plan_apply_kernel(cfws_frame_desc_t* __restrict__ desc, const int32_t* __restrict__ status,
                        uint64_t* __restrict__ vals, uint64_t n, const uint64_t* __restrict__ partials,
                        uint64_t nb, uint32_t self_scan, uint64_t* __restrict__ hdr, uint64_t capacity,
                        uint32_t* __restrict__ map, uint64_t* __restrict__ user_total, uint32_t policy,
                        uint32_t out_mask, const uint32_t* __restrict__ out_keys,
                        cfws_frame_desc_t* __restrict__ send)
{
    __shared__ uint64_t s_wave[kWaves];
    uint64_t prefix, g;
    plan_prefix(partials, nb, self_scan, hdr + 3, s_wave, prefix, g);
    const uint64_t total = g < capacity ? g : capacity;
    const uint64_t i0 = uint64_t(blockIdx.x) * kPlanBlock + uint64_t(threadIdx.x) * kPlanItems;
    uint64_t v[kPlanItems];
    uint64_t sum = 0;
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
            const DescWords d = load_desc(desc, (uint32_t)f);
            desc[f].payload_off = run;
            uint32_t of, oo;
            const bool emit = relay_decision(policy, status[f], d.fin(), d.opcode(), of, oo);
            const uint32_t hs = emit ? header_size_of(d.payload_size, out_mask != 0) : 0u;
            const uint32_t kin = d.mask() ? d.key() : 0u;
            const uint32_t kout = out_mask ? out_keys[f] : 0u;
            uint64_t* q = reinterpret_cast<uint64_t*>(send) + 4 * f;
            q[0] = d.wire_off + d.header_size();
            q[1] = kout;
            q[2] = emit ? d.payload_size : 0;
            q[3] = (uint64_t)(kin ^ kout) | (uint64_t)of << 32 | (uint64_t)oo << 40 |
                   (uint64_t)(out_mask ? 1u : 0u) << 48 | (uint64_t)hs << 56;
            map_range(run, run + v[k], f, total, map);
            if (f == n - 1) {
                map[(total + kRegion - 1) / kRegion] = (uint32_t)f;
                ser_epilogue(hdr, user_total, total, g, self_scan);
            }
        }
        run += v[k];
    }
}

inline uint64_t relay_ws_bytes(size_t n, uint64_t cap) { return ws_layout(n, cap).bytes + 32 * uint64_t(n); }

}  // namespace

extern "C" {

size_t cfws_relay_workspace_size(size_t n_frames, uint64_t out_capacity)
{
    return (size_t)relay_ws_bytes(n_frames, out_capacity);
}

int cfws_relay_batch(const void* d_wire_in, uint64_t wire_in_size, const uint64_t* d_index, size_t n,
                     uint64_t max_payload, uint32_t policy, uint8_t out_mask, const uint32_t* d_out_keys,
                     cfws_frame_desc_t* d_desc, int32_t* d_status, void* d_wire_out, uint64_t cap,
                     uint64_t* d_out_total, void* ws, size_t ws_size, void* stream)
{
    const CfwsPassScope pass_scope;
    if (int rc = check_init()) return rc;
    if (policy != CFWS_RELAY_VERBATIM && policy != CFWS_RELAY_ECHO_SERVER)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "unknown relay policy", hipSuccess);
    if (!ws || ws_size < relay_ws_bytes(n, cap)) return set_err(CFWS_ERROR_WORKSPACE, "workspace too small", hipSuccess);
    // the receive plan's and the send plan's limits (packed, no flags)
    ArgCheck c = check_de_plan(d_wire_in, d_index, n, 1, 0, d_desc, d_status, cap, ws, ws_size);
    if (!c.code) c = check_ser_plan(d_desc, n, cap, ws, ws_size);
    if (c.code) return set_err(c.code, c.what, hipSuccess);
    if (n != 0 && out_mask && !d_out_keys)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "out_mask needs d_out_keys", hipSuccess);
    if (n != 0 && misaligned(d_wire_in, nullptr))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "arenas must be 16-byte aligned", hipSuccess);
    if (n != 0 && cap != 0) {
        if (!d_wire_out) return set_err(CFWS_ERROR_INVALID_ARGUMENT, "null pointer", hipSuccess);
        if (misaligned(d_wire_out, nullptr))
            return set_err(CFWS_ERROR_INVALID_ARGUMENT, "arenas must be 16-byte aligned", hipSuccess);
        // the input is read up to round16(wire_in_size)
        const uintptr_t in0 = reinterpret_cast<uintptr_t>(d_wire_in), out0 = reinterpret_cast<uintptr_t>(d_wire_out);
        const uint64_t in_len = align_up(wire_in_size, 16);
        if (in0 < out0 + cap && out0 < in0 + in_len)
            return set_err(CFWS_ERROR_INVALID_ARGUMENT, "input and output ranges overlap", hipSuccess);
    }
    const WsLayout L = ws_layout(n, cap);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) return zero_totals(L, ws, d_out_total, st);
    uint64_t* hdr = ws_ptr<uint64_t>(ws, L.hdr);
    uint64_t* offs = ws_ptr<uint64_t>(ws, L.offs[0]);
    uint64_t* partials = ws_ptr<uint64_t>(ws, L.partials[0]);
    cfws_frame_desc_t* send = ws_ptr<cfws_frame_desc_t>(ws, L.bytes);
    const uint32_t nb = grid_for(n, kPlanBlock);
    const uint32_t self_scan = nb <= kSelfScanBlocks ? 1u : 0u;
    relay_plan_reduce_kernel<<<nb, kThreads, 0, st>>>(static_cast<const uint8_t*>(d_wire_in), wire_in_size, d_index,
                                                      n, max_payload, policy, out_mask, d_desc, d_status, offs,
                                                      partials);
    if (!self_scan) scan_partials_kernel<<<1, kThreads, 0, st>>>(partials, nb, hdr + 3);
    relay_plan_apply_kernel<<<nb, kThreads, 0, st>>>(d_desc, d_status, offs, n, partials, nb, self_scan, hdr, cap,
                                                     ws_ptr<uint32_t>(ws, L.map[0]), d_out_total, policy, out_mask,
                                                     d_out_keys, send);
    if (int rc = launch_check("relay_batch(plan)")) return rc;
    if (cap == 0) return CFWS_OK;
    // the timed pass; no in-region send edges: they assume a 16-aligned source
    launch_pass<kModeRelay>(L, 0, d_wire_in, d_wire_out, send, nullptr, ws, cap, n, kClassAll, st);
    return launch_check("relay_batch");
}

}  // extern "C"
