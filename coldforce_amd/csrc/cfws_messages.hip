// cfws_messages.hip -- message and control tables of received frames on the
// device (cfws_messages_batch, include/cfws.h). The rule is
// this library's own (cfws_rules.h: message_frame_class, message_starts,
// message_start_flags, message_end_flags), shared with the host walk
// (cfws_index.cpp). A unit of its own: no existing path changes.
//
// The walk's one bit of state, `open`, is "the connection's previous DATA
// frame's fin", which has to look across control frames, workgroups and
// messages of any length. Two rounds of reduce -> scan_partials2_kernel ->
// apply (plain launches; no look-back between workgroups) make it local:
//   A  classify; per-group counts of data and control frames; the apply
//      compacts the data frames into a dense list of 16-byte rows (payload
//      size, frame index, opcode | fin | out-of-memory) and writes the
//      control indices straight into d_control.
//   B  over the dense list, where data frame k's predecessor is row k - 1:
//      "starts a message" needs the row's opcode, row k - 1's fin and whether
//      k is the first data frame of its connection (a search in conn_first).
//      The sums are message starts, payload bytes and out-of-memory rows; the
//      apply gives each start its message index and leaves the running sums
//      at the start in a 32-byte row per message.
//   finish  one thread per message: the differences to the next start are
//      payload_size and n_fragments, the last fragment's fin and the next
//      message's connection decide FINAL / CUT / OPEN; the record goes out as
//      two 16-byte stores.
//   conn    one thread per connection: its first message, by a search over
//      the messages' connections (non-decreasing).
#include "cfws_kernels.h"

namespace {

constexpr int kMsgItems = 4;                                     // consecutive frames per thread
constexpr uint64_t kMsgGroup = uint64_t(kThreads) * kMsgItems;   // frames per workgroup

// A dense row's meta word.
constexpr uint32_t kRowFin = 0x100u, kRowOom = 0x200u;

// ws header words (u64): the scans' grand totals
enum : int { kHdrData = 0, kHdrControl = 1, kHdrStarts = 2, kHdrBytes = 3 };

// B's first sum packs two counts, each at most n_frames <= 2^32 - 1:
// message starts (low half) and out-of-memory rows (high half).
__host__ __device__ inline uint64_t pack_counts(uint32_t starts, uint32_t oom) { return starts | uint64_t(oom) << 32; }

struct MsgLayout {
    uint64_t hdr, part[4], dense, rows, bytes;
};

inline MsgLayout msg_layout(uint64_t n)
{
    MsgLayout L;
    const uint64_t nb = grid_for(n, kMsgGroup);
    uint64_t at = 0;
    L.hdr = at; at += 256;
    for (int p = 0; p < 4; ++p) { L.part[p] = at; at = align_up(at + 8 * (nb + 1), 256); }
    L.dense = at; at = align_up(at + 16 * n, 256);
    L.rows = at; at = align_up(at + 32 * n, 256);
    L.bytes = at;
    return L;
}

// The 32-byte row a message start leaves for the finish pass.
struct MsgRow {
    uint64_t bytes_before;     // payload bytes of the data rows before the start
    uint32_t k;                // the start's dense row
    uint32_t oom_before;       // out-of-memory rows before the start
    uint64_t payload_off;
    uint32_t conn, zero;
};
static_assert(sizeof(MsgRow) == 32 && sizeof(cfws_message_t) == 32, "two 16-byte words each");

// Frame f's class and, for a data frame, its dense row.
__device__ __forceinline__ uint32_t classify(const cfws_frame_desc_t* __restrict__ desc,
                                             const int32_t* __restrict__ status, uint64_t f, u32x4* row)
{
    const uint64_t* q = reinterpret_cast<const uint64_t*>(desc) + 4 * f;
    const uint64_t size = q[2], w3 = q[3];
    const int32_t st = status ? status[f] : CFWS_PARSE_COMPLETE;
    const uint32_t opcode = (uint32_t)(w3 >> 40) & 0xffu, fin = (uint32_t)(w3 >> 32) & 0xffu;
    if (row)
        *row = u32x4{(uint32_t)size, (uint32_t)(size >> 32), (uint32_t)f,
                     opcode | (fin ? kRowFin : 0u) | (st == CFWS_ERROR_OUT_OF_MEMORY ? kRowOom : 0u)};
    return message_frame_class(st, opcode);
}

// A: per-group counts (data in the low half, control in the high half of one
// word inside the group; two block sums out).
__global__ void __launch_bounds__(kThreads)
messages_count_kernel(const cfws_frame_desc_t* __restrict__ desc, const int32_t* __restrict__ status, uint64_t n,
                      uint64_t* __restrict__ part_data, uint64_t* __restrict__ part_control)
{
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t f0 = uint64_t(blockIdx.x) * kMsgGroup + uint64_t(threadIdx.x) * kMsgItems;
    uint64_t x = 0;
#pragma unroll
    for (int i = 0; i < kMsgItems; ++i) {
        if (f0 + i < n) {
            const uint32_t cls = classify(desc, status, f0 + i, nullptr);
            x += cls == kMessageFrameData ? 1u : (cls == kMessageFrameControl ? uint64_t(1) << 32 : 0u);
        }
    }
    uint64_t total;
    block_exclusive_scan(x, s_wave, &total);
    if (threadIdx.x == 0) {
        part_data[blockIdx.x] = total & 0xffffffffu;
        part_control[blockIdx.x] = total >> 32;
    }
}

// A's apply: the dense rows of the data frames, the control list.
__global__ void __launch_bounds__(kThreads)
messages_compact_kernel(const cfws_frame_desc_t* __restrict__ desc, const int32_t* __restrict__ status, uint64_t n,
                        const uint64_t* __restrict__ part_data, const uint64_t* __restrict__ part_control,
                        u32x4* __restrict__ dense, uint32_t* __restrict__ control, uint64_t control_cap)
{
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t f0 = uint64_t(blockIdx.x) * kMsgGroup + uint64_t(threadIdx.x) * kMsgItems;
    uint32_t cls[kMsgItems];
    u32x4 row[kMsgItems];
    uint64_t x = 0;
#pragma unroll
    for (int i = 0; i < kMsgItems; ++i) {
        cls[i] = kMessageFrameIgnored;
        if (f0 + i < n) cls[i] = classify(desc, status, f0 + i, &row[i]);
        x += cls[i] == kMessageFrameData ? 1u : (cls[i] == kMessageFrameControl ? uint64_t(1) << 32 : 0u);
    }
    uint64_t total;
    const uint64_t before = block_exclusive_scan(x, s_wave, &total);
    uint64_t k = part_data[blockIdx.x] + (before & 0xffffffffu);
    uint64_t j = part_control[blockIdx.x] + (before >> 32);
#pragma unroll
    for (int i = 0; i < kMsgItems; ++i) {
        if (cls[i] == kMessageFrameData) {
            dense[k++] = row[i];
        } else if (cls[i] == kMessageFrameControl) {
            if (j < control_cap) control[j] = (uint32_t)(f0 + i);
            ++j;
        }
    }
}

// The connection of frame f: the last c with conn_first[c] <= f (values above
// n_frames compare as n_frames, since f < n_frames); 0 without conn_first.
// *first gets conn_first[c].
__device__ __forceinline__ uint32_t conn_of(const uint64_t* __restrict__ conn_first, uint64_t n_conns, uint32_t f,
                                            uint64_t* first)
{
    *first = 0;
    if (!conn_first) return 0;
    uint64_t lo = 0, hi = n_conns;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (conn_first[mid] <= f) lo = mid + 1; else hi = mid;
    }
    if (lo <= 1) return 0;                      // connection 0 starts at frame 0
    *first = conn_first[lo - 1];
    return (uint32_t)(lo - 1);
}

// Does dense row k (meta `meta`, frame `frame`) start a message? `open` is
// the previous data frame's !fin when that frame is of the same connection.
struct RowStart {
    bool starts;
    uint32_t conn;
};

__device__ __forceinline__ RowStart row_start(const u32x4* __restrict__ dense, uint64_t k, const u32x4& row,
                                              const uint64_t* __restrict__ conn_first, uint64_t n_conns)
{
    uint64_t first;
    RowStart r;
    r.conn = conn_of(conn_first, n_conns, row.z, &first);
    bool open = false;
    if (k > 0) {
        const u32x4 prev = dense[k - 1];
        open = prev.z >= first && !(prev.w & kRowFin);
    }
    r.starts = message_starts(row.w & 0xffu, open);
    return r;
}

// B: per-group sums over the dense rows: starts | out-of-memory rows, bytes.
__global__ void __launch_bounds__(kThreads)
messages_starts_kernel(const u32x4* __restrict__ dense, const uint64_t* __restrict__ hdr,
                       const uint64_t* __restrict__ conn_first, uint64_t n_conns,
                       uint64_t* __restrict__ part_counts, uint64_t* __restrict__ part_bytes)
{
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t nd = hdr[kHdrData];
    const uint64_t k0 = uint64_t(blockIdx.x) * kMsgGroup + uint64_t(threadIdx.x) * kMsgItems;
    uint64_t counts = 0, bytes = 0;
#pragma unroll
    for (int i = 0; i < kMsgItems; ++i) {
        if (k0 + i < nd) {
            const u32x4 row = dense[k0 + i];
            const RowStart s = row_start(dense, k0 + i, row, conn_first, n_conns);
            counts += pack_counts(s.starts ? 1u : 0u, (row.w & kRowOom) ? 1u : 0u);
            bytes += row.x | uint64_t(row.y) << 32;
        }
    }
    uint64_t total_counts, total_bytes;
    block_exclusive_scan(counts, s_wave, &total_counts);
    block_exclusive_scan(bytes, s_wave, &total_bytes);
    if (threadIdx.x == 0) {
        part_counts[blockIdx.x] = total_counts;
        part_bytes[blockIdx.x] = total_bytes;
    }
}

// B's apply: each start's message index and its row of running sums.
__global__ void __launch_bounds__(kThreads)
messages_rows_kernel(const cfws_frame_desc_t* __restrict__ desc, const u32x4* __restrict__ dense,
                     const uint64_t* __restrict__ hdr, const uint64_t* __restrict__ conn_first, uint64_t n_conns,
                     const uint64_t* __restrict__ part_counts, const uint64_t* __restrict__ part_bytes,
                     MsgRow* __restrict__ rows)
{
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t nd = hdr[kHdrData];
    const uint64_t k0 = uint64_t(blockIdx.x) * kMsgGroup + uint64_t(threadIdx.x) * kMsgItems;
    u32x4 row[kMsgItems];
    RowStart s[kMsgItems];
    uint64_t counts = 0, bytes = 0;
#pragma unroll
    for (int i = 0; i < kMsgItems; ++i) {
        row[i] = u32x4{0, 0, 0, 0};
        s[i] = RowStart{false, 0};
        if (k0 + i < nd) {
            row[i] = dense[k0 + i];
            s[i] = row_start(dense, k0 + i, row[i], conn_first, n_conns);
            counts += pack_counts(s[i].starts ? 1u : 0u, (row[i].w & kRowOom) ? 1u : 0u);
            bytes += row[i].x | uint64_t(row[i].y) << 32;
        }
    }
    uint64_t total;
    uint64_t c = part_counts[blockIdx.x] + block_exclusive_scan(counts, s_wave, &total);
    uint64_t b = part_bytes[blockIdx.x] + block_exclusive_scan(bytes, s_wave, &total);
#pragma unroll
    for (int i = 0; i < kMsgItems; ++i) {
        if (s[i].starts) {
            const uint64_t off = desc[row[i].z].payload_off;
            u32x4* out = reinterpret_cast<u32x4*>(rows + (c & 0xffffffffu));
            out[0] = u32x4{(uint32_t)b, (uint32_t)(b >> 32), (uint32_t)(k0 + i), (uint32_t)(c >> 32)};
            out[1] = u32x4{(uint32_t)off, (uint32_t)(off >> 32), s[i].conn, 0u};
        }
        c += pack_counts(s[i].starts ? 1u : 0u, (row[i].w & kRowOom) ? 1u : 0u);
        b += row[i].x | uint64_t(row[i].y) << 32;
    }
}

// One thread per message: the record, from its row, the next message's row
// (or the grand totals) and the dense rows of its first and last fragment.
// Thread 0 also writes the totals.
__global__ void __launch_bounds__(kThreads)
messages_finish_kernel(const u32x4* __restrict__ dense, const MsgRow* __restrict__ rows,
                       const uint64_t* __restrict__ hdr, cfws_message_t* __restrict__ msgs, uint64_t cap,
                       uint64_t* __restrict__ n_messages, uint64_t* __restrict__ n_control)
{
    const uint64_t m = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t n_msg = hdr[kHdrStarts] & 0xffffffffu;
    if (m == 0) {
        *n_messages = n_msg;
        if (n_control) *n_control = hdr[kHdrControl];
    }
    if (m >= n_msg || m >= cap) return;
    const u32x4* r = reinterpret_cast<const u32x4*>(rows + m);
    const u32x4 a = r[0], b = r[1];
    uint64_t next_bytes = hdr[kHdrBytes], next_k = hdr[kHdrData], next_oom = hdr[kHdrStarts] >> 32;
    bool followed = false;
    if (m + 1 < n_msg) {
        const u32x4 na = r[2], nb = r[3];
        next_bytes = na.x | uint64_t(na.y) << 32;
        next_k = na.z;
        next_oom = na.w;
        followed = nb.z == b.z;
    }
    const u32x4 head = dense[a.z], tail = dense[next_k - 1];
    const uint64_t size = next_bytes - (a.x | uint64_t(a.y) << 32);
    const uint32_t opcode = head.w & 0xffu;
    const uint32_t flags = message_start_flags(opcode) |
                           message_end_flags((tail.w & kRowFin) != 0, followed, (uint32_t)next_oom != a.w);
    u32x4* out = reinterpret_cast<u32x4*>(msgs + m);
    out[0] = u32x4{b.x, b.y, (uint32_t)size, (uint32_t)(size >> 32)};
    out[1] = u32x4{head.z, (uint32_t)(next_k - a.z), b.z, opcode | flags << 8};
}

// One thread per connection: the messages of the connections before it.
__global__ void __launch_bounds__(kThreads)
messages_conn_kernel(const MsgRow* __restrict__ rows, const uint64_t* __restrict__ hdr, uint64_t n_conns,
                     uint64_t* __restrict__ conn_first_msg)
{
    const uint64_t c = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (c >= n_conns) return;
    uint64_t lo = 0, hi = hdr[kHdrStarts] & 0xffffffffu;
    while (lo < hi) {                           // the first message whose connection is >= c
        const uint64_t mid = (lo + hi) >> 1;
        if (rows[mid].conn < c) lo = mid + 1; else hi = mid;
    }
    conn_first_msg[c] = lo;
}

}  // namespace

extern "C" {

size_t cfws_messages_workspace_size(size_t n_frames, size_t n_conns)
{
    (void)n_conns;                              // the connections take no workspace
    return (size_t)msg_layout(n_frames).bytes;
}

size_t cfws_messages_group_frames(void)
{
    return (size_t)kMsgGroup;
}

int cfws_messages_batch(const cfws_frame_desc_t* d_desc, const int32_t* d_status, size_t n, const uint64_t* d_conn_first,
                        size_t n_conns, cfws_message_t* d_msgs, uint64_t msg_cap, uint64_t* d_conn_first_msg,
                        uint64_t* d_n_messages, uint32_t* d_control, uint64_t control_cap, uint64_t* d_n_control,
                        void* ws, size_t ws_size, void* stream)
{
    const CfwsPassScope pass_scope;     // not a timed pass: a pending pair is dropped
    if (int rc = check_init()) return rc;
    const uint64_t conns = d_conn_first ? n_conns : (d_conn_first_msg ? 1 : 0);
    if ((n && !d_desc) || (msg_cap && !d_msgs) || (control_cap && !d_control) ||
        (d_conn_first && n_conns && !d_conn_first_msg) || !d_n_messages || !ws)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "messages: null pointer", hipSuccess);
    if (reinterpret_cast<uintptr_t>(d_msgs) & 15u)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "messages: d_msgs must be 16-byte aligned", hipSuccess);
    if (n > 0xffffffffull)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "messages: n_frames above 2^32 - 1", hipSuccess);
    if (ws_size < cfws_messages_workspace_size(n, n_conns))
        return set_err(CFWS_ERROR_WORKSPACE, "messages workspace too small", hipSuccess);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0 || (d_conn_first && n_conns == 0)) {     // no frame belongs to a connection
        (void)hipMemsetAsync(d_n_messages, 0, 8, st);
        if (d_n_control) (void)hipMemsetAsync(d_n_control, 0, 8, st);
        if (conns) (void)hipMemsetAsync(d_conn_first_msg, 0, 8 * conns, st);
        return launch_check("messages");
    }
    const MsgLayout L = msg_layout(n);
    uint64_t* hdr = ws_ptr<uint64_t>(ws, L.hdr);
    uint64_t* pa0 = ws_ptr<uint64_t>(ws, L.part[0]);
    uint64_t* pa1 = ws_ptr<uint64_t>(ws, L.part[1]);
    uint64_t* pb0 = ws_ptr<uint64_t>(ws, L.part[2]);
    uint64_t* pb1 = ws_ptr<uint64_t>(ws, L.part[3]);
    u32x4* dense = ws_ptr<u32x4>(ws, L.dense);
    MsgRow* rows = ws_ptr<MsgRow>(ws, L.rows);
    const uint32_t nb = grid_for(n, kMsgGroup);
    messages_count_kernel<<<nb, kThreads, 0, st>>>(d_desc, d_status, n, pa0, pa1);
    scan_partials2_kernel<<<2, kThreads, 0, st>>>(pa0, pa1, nb, hdr + kHdrData, hdr + kHdrControl);
    messages_compact_kernel<<<nb, kThreads, 0, st>>>(d_desc, d_status, n, pa0, pa1, dense, d_control, control_cap);
    // the dense list's length is on the device: the grids cover n_frames rows
    messages_starts_kernel<<<nb, kThreads, 0, st>>>(dense, hdr, d_conn_first, n_conns, pb0, pb1);
    scan_partials2_kernel<<<2, kThreads, 0, st>>>(pb0, pb1, nb, hdr + kHdrStarts, hdr + kHdrBytes);
    messages_rows_kernel<<<nb, kThreads, 0, st>>>(d_desc, dense, hdr, d_conn_first, n_conns, pb0, pb1, rows);
    messages_finish_kernel<<<grid_for(n, kThreads), kThreads, 0, st>>>(dense, rows, hdr, d_msgs, msg_cap,
                                                                       d_n_messages, d_n_control);
    if (conns)
        messages_conn_kernel<<<grid_for(conns, kThreads), kThreads, 0, st>>>(rows, hdr, conns, d_conn_first_msg);
    return launch_check("messages");
}

}  // extern "C"
