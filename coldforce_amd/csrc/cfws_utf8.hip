// cfws_utf8.hip -- UTF-8 check of received text messages on the device
// (cfws_utf8_messages_batch, include/cfws.h). The rule is
// this library's own (cfws_rules.h: utf8_at and what it is made of,
// utf8_selected, utf8_carried, utf8_row), shared with the host walk
// (cfws_index.cpp). It is position-local: a byte is judged from the 3 bytes
// before and the 3 after it, so nothing scans over the bytes.
//
// Work is cut by message, then by piece: kPiece bytes on 16 lanes, a 16-byte
// chunk per lane, aligned to the arena's chunks (not to the message).
//   Utf8Pieces  table pass over the messages: each checked message's pieces,
//      scanned; the apply leaves a 16-byte row per message, the first piece
//      and the minimum (none yet).
//   check  the total is on the device, so the grid is sized from
//      payload_bytes and n_msgs and strides over the pieces, four per wave.
//      A piece's 16 lanes find its message by a 16-way search over the rows'
//      firsts. Every chunk is loaded once; the 3 bytes before and after it
//      come from the neighbouring lanes (DPP inside the row of 16), for a
//      piece's edge lanes from one aligned 4-byte load of the neighbouring
//      chunk when the message has one. Bytes outside the message are absent,
//      or the carried bytes in front of a HEADLESS message. A wave whose
//      chunks are all ASCII does nothing more (an ASCII byte is fine whatever
//      surrounds it). Else each lane takes the first position of its chunk
//      that is not fine, the wave reduces them by message and issues one
//      64-bit atomicMin per (wave, message) that found one.
//   Utf8Finish  table pass over the messages: the carried bytes' own
//      positions (they look into the message's first bytes), the row from
//      the minimum as one 16-byte store, the BAD list and the counts.
#include "cfws_tables.h"

namespace {

constexpr uint64_t kPieceLanes = 16;
constexpr uint64_t kPiece = kPieceLanes * kChunk;                   // 256 bytes
constexpr uint64_t kWavePieces = 64 / kPieceLanes;
constexpr uint64_t kWaveBytes = kWavePieces * kPiece;               // 1 KiB
constexpr uint64_t kGroupBytes = kWaves * kWaveBytes;               // a workgroup per stride: 4 KiB
constexpr uint64_t kNone = ~uint64_t(0);                            // no position found
constexpr uint32_t kMaxGrid = 16384;

enum : int { kHdrPieces = 0, kHdrChecked = 1, kHdrBad = 2 };

struct Utf8Msg {
    uint64_t lo, size;
    uint32_t flags, cin, k;
    bool checked;
};

__device__ __forceinline__ Utf8Msg utf8_msg(const cfws_message_t* __restrict__ msgs,
                                            const uint32_t* __restrict__ carry_in, uint64_t payload_bytes, uint64_t m)
{
    const uint64_t* q = reinterpret_cast<const uint64_t*>(msgs) + 4 * m;
    const uint64_t w3 = q[3];
    Utf8Msg M;
    M.lo = q[0];
    M.size = q[1];
    M.flags = (uint32_t)(w3 >> 40) & 0xffu;
    M.cin = carry_in ? carry_in[m] : 0u;
    M.checked = utf8_selected((uint32_t)(w3 >> 32) & 0xffu, M.flags, M.lo, M.size, payload_bytes, M.cin);
    M.k = utf8_carried(M.flags, M.cin);
    return M;
}

// The pieces of a message: its chunks, 16 per piece.
__device__ __forceinline__ uint64_t utf8_pieces(const Utf8Msg& M)
{
    if (!M.checked || M.size == 0) return 0;
    return (((M.lo + M.size - 1) >> 4) - (M.lo >> 4) + kPieceLanes) / kPieceLanes;
}

// Over the messages: the row {first piece, minimum} of each.
struct Utf8Pieces {
    const cfws_message_t* msgs;
    const uint32_t* carry_in;
    uint64_t payload_bytes, n;
    uint64_t* part[1];
    u32x4* rows;

    __device__ TableRows counts() const { return {n}; }
    __device__ uint64_t load(TableRows, uint64_t m) const { return utf8_pieces(utf8_msg(msgs, carry_in, payload_bytes, m)); }
    __device__ TableSums<1> weigh(const uint64_t& pieces) const { return {{pieces}}; }
    __device__ void emit(TableRows, uint64_t m, const uint64_t&, const uint64_t* run) const
    {
        rows[m] = u32x4{(uint32_t)run[0], (uint32_t)(run[0] >> 32), ~0u, ~0u};
    }
};

// The number of rows m < n whose first piece is <= p (a prefix of the rows),
// found by the piece's 16 lanes together: each round probes 16 evenly spaced
// rows and keeps the gap after the last that holds. gl: the lane in its row
// of 16; shift: that row's first lane in the wave.
__device__ __forceinline__ uint64_t utf8_rows_upto(const uint64_t* __restrict__ rows, uint64_t n, uint64_t p,
                                                   uint32_t gl, uint32_t shift)
{
    uint64_t lo = 0, hi = n;                                        // the answer lies in [lo, hi]
    while (lo < hi) {
        const uint64_t step = (hi - lo + kPieceLanes - 1) / kPieceLanes;
        const uint64_t q = lo + gl * step;
        const bool holds = q < hi && rows[2 * q] <= p;
        const uint32_t t = __popcll((__ballot(holds) >> shift) & 0xffffull);
        if (t == 0) {
            hi = lo;
        } else {
            const uint64_t top = lo + t * step;
            lo = lo + (t - 1) * step + 1;
            hi = top < hi ? top : hi;
        }
    }
    return lo;
}

// Lane i of a row of 16 receives lane i - 1's v (DPP row_shr:1) or lane
// i + 1's (row_shl:1); the row's edge lane keeps `edge`.
__device__ __forceinline__ uint32_t from_prev_in_row(uint32_t v, uint32_t edge)
{
    return __builtin_amdgcn_update_dpp(edge, v, 0x111, 0xf, 0xf, false);
}

__device__ __forceinline__ uint32_t from_next_in_row(uint32_t v, uint32_t edge)
{
    return __builtin_amdgcn_update_dpp(edge, v, 0x101, 0xf, 0xf, false);
}

// The first position of the chunk at arena offset a0 that is not fine, as a
// key (position in S << 1 | truncated), or kNone. A: the chunk; prevw: the 4
// bytes before it; nextw: the 4 after it.
__device__ __forceinline__ uint64_t utf8_chunk_key(const Utf8Msg& M, uint64_t a0, const uint4& A, uint32_t prevw,
                                                   uint32_t nextw)
{
    const uint64_t hi = M.lo + M.size;
    uint32_t w[22];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        w[j] = (prevw >> (8 * (j + 1))) & 0xffu;
        w[19 + j] = (nextw >> (8 * j)) & 0xffu;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) w[3 + j] = u4_byte(A, j);
    // window byte j is arena byte a0 - 3 + j
    if (a0 < M.lo + 3 || a0 + 19 > hi) {
#pragma unroll
        for (int j = 0; j < 22; ++j) {
            const uint64_t t = a0 + j;                              // the byte's offset + 3
            if (t < M.lo + 3) {
                const uint64_t d = M.lo + 3 - t;                    // bytes before the message: 1..
                w[j] = d <= M.k ? (M.cin >> (8u * (M.k - (uint32_t)d))) & 0xffu : kUtf8Absent;
            } else if (t >= hi + 3) {
                w[j] = kUtf8Absent;
            }
        }
    }
    const uint32_t i_lo = M.lo > a0 ? (uint32_t)(M.lo - a0) : 0u;
    const uint32_t i_hi = hi - a0 < 16 ? (uint32_t)(hi - a0) : 16u;
    uint64_t key = kNone;
#pragma unroll
    for (int i = 15; i >= 0; --i) {
        const uint32_t b = w[3 + i];
        if ((b & 0x80u) && (uint32_t)i >= i_lo && (uint32_t)i < i_hi) {
            const uint32_t cls = utf8_at(b, w[2 + i], w[1 + i], w[i], w[4 + i], w[5 + i], w[6 + i]);
            if (cls != kUtf8Fine) key = ((a0 + i - M.lo + M.k) << 1) | (cls == kUtf8Truncated ? 1u : 0u);
        }
    }
    return key;
}

__global__ void __launch_bounds__(kThreads)
utf8_check_kernel(const uint8_t* __restrict__ payload, uint64_t payload_bytes, const cfws_message_t* __restrict__ msgs,
                  const uint32_t* __restrict__ carry_in, uint64_t n, uint64_t* __restrict__ rows,
                  const uint64_t* __restrict__ hdr)
{
    const uint64_t total = hdr[kHdrPieces];
    const uint32_t lane = threadIdx.x & 63u, gl = lane & 15u, shift = lane & 48u;
    const uint64_t wave = uint64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6);
    const uint64_t stride = uint64_t(gridDim.x) * kWaves * kWavePieces;
    for (uint64_t pb = wave * kWavePieces; pb < total; pb += stride) {       // wave-uniform
        const uint64_t p = pb + (lane >> 4);
        uint32_t m = ~0u;
        Utf8Msg M = {};
        uint64_t c = 0, c0 = 0, c1 = 0;
        bool act = false;
        uint4 A = make_uint4(0, 0, 0, 0);
        if (p < total) {
            const uint64_t upto = utf8_rows_upto(rows, n, p, gl, shift);
            if (upto > 0) {
                m = (uint32_t)(upto - 1);
                M = utf8_msg(msgs, carry_in, payload_bytes, m);
                const uint64_t k = p - rows[2 * uint64_t(m)];
                // the message is checked again here, with the bounds: whatever
                // the rows hold, the chunk lies inside the arena
                if (M.checked && M.size > 0) {
                    c0 = M.lo >> 4;
                    c1 = (M.lo + M.size - 1) >> 4;
                    act = k <= (c1 - c0) / kPieceLanes && c0 + k * kPieceLanes + gl <= c1;
                    c = c0 + k * kPieceLanes + gl;
                }
                if (act) A = ld16(payload + kChunk * c);
            }
        }
        const bool high = ((A.x | A.y | A.z | A.w) & 0x80808080u) != 0;
        if (!__any(high)) continue;
        uint32_t prevw = from_prev_in_row(A.w, 0u), nextw = from_next_in_row(A.x, 0u);
        uint64_t key = kNone;
        if (high) {
            // the neighbouring chunk of a piece's edge lane, where the message has one
            if (gl == 0 && c > c0) prevw = *reinterpret_cast<const uint32_t*>(payload + kChunk * c - 4);
            if (gl == kPieceLanes - 1 && c < c1) nextw = *reinterpret_cast<const uint32_t*>(payload + kChunk * c + kChunk);
            key = utf8_chunk_key(M, kChunk * c, A, prevw, nextw);
        }
        if (!__any(key != kNone)) continue;
        // the smallest key of each message in the wave; a message's lanes are adjacent
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint64_t y = __shfl_down(key, o, 64);
            const uint32_t ym = (uint32_t)__shfl_down((int)m, o, 64);
            if (lane + o < 64 && ym == m && y < key) key = y;
        }
        const uint32_t pm = (uint32_t)__shfl_up((int)m, 1, 64);
        if ((lane == 0 || pm != m) && key != kNone)
            atomicMin(reinterpret_cast<unsigned long long*>(rows + 2 * uint64_t(m) + 1), (unsigned long long)key);
    }
}

// Over the messages: the result rows, the BAD list, the counts.
struct Utf8Finish {
    struct Counts { uint64_t n, checked, bad; };
    struct Item { u32x4 row; };
    const uint8_t* payload;
    const cfws_message_t* msgs;
    const uint32_t* carry_in;
    uint64_t payload_bytes, n;
    const uint64_t* rows;
    const uint64_t* hdr;
    uint64_t* part[2];
    u32x4* result;
    uint32_t* bad;
    uint64_t bad_cap;
    uint64_t* out_counts;

    __device__ Counts counts() const { return {n, hdr[kHdrChecked], hdr[kHdrBad]}; }
    __device__ Item load(const Counts&, uint64_t m) const
    {
        const Utf8Msg M = utf8_msg(msgs, carry_in, payload_bytes, m);
        if (!M.checked) return {u32x4{0u, 0u, 0u, 0u}};
        const uint8_t* body = payload + M.lo;
        const uint32_t k = M.k, cin = M.cin;
        const uint64_t len = k + M.size;
        auto S = [&](uint64_t j) -> uint32_t { return j < k ? (cin >> (8u * (uint32_t)j)) & 0xffu : body[j - k]; };
        uint64_t key = rows[2 * m + 1];
        for (uint32_t i = k; i-- > 0;) {                            // the carried bytes' own positions
            const uint32_t cls = utf8_at_by(S, len, i);
            if (cls != kUtf8Fine) key = (uint64_t(i) << 1) | (cls == kUtf8Truncated ? 1u : 0u);
        }
        const Utf8Row r = utf8_row(S, len, k, M.flags, key == kNone ? len : key >> 1, (key & 1u) != 0);
        return {u32x4{(uint32_t)r.prefix, (uint32_t)(r.prefix >> 32), r.carry, r.flags}};
    }
    __device__ TableSums<1, true> weigh(const Item& it) const      // checked | BAD
    {
        return {{pack2(it.row.w & CFWS_UTF8_CHECKED ? 1u : 0u, it.row.w & CFWS_UTF8_BAD ? 1u : 0u)}};
    }
    __device__ void emit(const Counts&, uint64_t m, const Item& it, const uint64_t* run) const
    {
        result[m] = it.row;
        const uint64_t j = run[0] >> 32;
        if ((it.row.w & CFWS_UTF8_BAD) && j < bad_cap) bad[j] = (uint32_t)m;
    }
    __device__ void first_thread(const Counts& c) const
    {
        out_counts[0] = c.checked;
        out_counts[1] = c.bad;
    }
};

}  // namespace

extern "C" {

size_t cfws_utf8_workspace_size(size_t n_msgs)
{
    return (size_t)table_head(n_msgs).end;
}

size_t cfws_utf8_piece_bytes(void) { return (size_t)kPiece; }
size_t cfws_utf8_wave_bytes(void) { return (size_t)kWaveBytes; }
size_t cfws_utf8_workgroup_bytes(void) { return (size_t)kGroupBytes; }

int cfws_utf8_messages_batch(const void* d_payload, uint64_t payload_bytes, const cfws_message_t* d_msgs, size_t n,
                             const uint32_t* d_carry_in, cfws_utf8_result_t* d_result, uint32_t* d_bad,
                             uint64_t bad_cap, uint64_t* d_counts, void* ws, size_t ws_size, void* stream)
{
    const CfwsPassScope pass_scope;     // not a timed pass: a pending pair is dropped
    if (int rc = check_init()) return rc;
    if ((n && (!d_msgs || !d_result)) || (payload_bytes && !d_payload) || (bad_cap && !d_bad) || !d_counts || !ws)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "utf8: null pointer", hipSuccess);
    if (misaligned(d_result, d_payload))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "utf8: d_result and d_payload must be 16-byte aligned", hipSuccess);
    if (n > 0xffffffffull)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "utf8: n_msgs above 2^32 - 1", hipSuccess);
    if (ws_size < cfws_utf8_workspace_size(n))
        return set_err(CFWS_ERROR_WORKSPACE, "utf8 workspace too small", hipSuccess);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) {
        (void)hipMemsetAsync(d_counts, 0, 16, st);
        return launch_check("utf8");
    }
    const TableHead L = table_head(n);
    uint64_t* hdr = ws_ptr<uint64_t>(ws, L.hdr);
    uint64_t* part[3];
    for (int p = 0; p < 3; ++p) part[p] = ws_ptr<uint64_t>(ws, L.part[p]);
    u32x4* rows = ws_ptr<u32x4>(ws, L.dense);
    const uint8_t* payload = static_cast<const uint8_t*>(d_payload);
    const Utf8Pieces pieces = {d_msgs, d_carry_in, payload_bytes, n, {part[0]}, rows};
    const Utf8Finish finish = {payload, d_msgs, d_carry_in, payload_bytes, n, reinterpret_cast<const uint64_t*>(rows),
                               hdr, {part[1], part[2]}, reinterpret_cast<u32x4*>(d_result), d_bad, bad_cap, d_counts};
    const uint32_t nb = grid_for(n, kTableGroup);
    table_pass_kernel<kTableReduce><<<nb, kThreads, 0, st>>>(pieces);
    scan_partials_kernel<<<1, kThreads, 0, st>>>(part[0], nb, hdr + kHdrPieces);
    table_pass_kernel<kTableApply><<<nb, kThreads, 0, st>>>(pieces);
    // the number of pieces is on the device: rows that do not overlap have at
    // most this many; the kernel strides up to the total
    const uint64_t most = payload_bytes / kPiece + 2 * uint64_t(n);
    const uint64_t blocks = (most + kWaves * kWavePieces - 1) / (kWaves * kWavePieces);
    utf8_check_kernel<<<(uint32_t)(blocks < kMaxGrid ? blocks : kMaxGrid), kThreads, 0, st>>>(
        payload, payload_bytes, d_msgs, d_carry_in, n, reinterpret_cast<uint64_t*>(rows), hdr);
    table_pass_kernel<kTableReduce><<<nb, kThreads, 0, st>>>(finish);
    scan_partials2_kernel<<<2, kThreads, 0, st>>>(part[1], part[2], nb, hdr + kHdrChecked, hdr + kHdrBad);
    table_pass_kernel<kTableApply><<<nb, kThreads, 0, st>>>(finish);
    return launch_check("utf8");
}

}  // extern "C"
