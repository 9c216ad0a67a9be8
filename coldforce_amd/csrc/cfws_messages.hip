// cfws_messages.hip -- message and control tables of received frames on the
// device (cfws_messages_batch, include/cfws.h). The rule is
// this library's own (cfws_rules.h: message_frame_class, message_starts,
// message_start_flags, message_end_flags), shared with the host walk
// (cfws_index.cpp). The unit is two table passes (cfws_tables.h: each pass is
// one struct, its reduce and its apply kernel one template over it) and two
// plain kernels.
//
// The walk's one bit of state, `open`, is "the connection's previous DATA
// frame's fin", which has to look across control frames, workgroups and
// messages of any length. Two rounds of reduce -> scan_partials2_kernel ->
// apply (plain launches; no look-back between workgroups) make it local:
//   MsgFrames  classify; the sums are the data and the control frames; the
//      apply compacts the data frames into a dense list of 16-byte rows
//      (payload size, frame index, opcode | fin | out-of-memory) and writes
//      the control indices straight into d_control.
//   MsgStarts  over the dense list, where data frame k's predecessor is row
//      k - 1: "starts a message" needs the row's opcode, row k - 1's fin and
//      whether k is the first data frame of its connection (a search in
//      conn_first). The sums are message starts, out-of-memory rows and
//      payload bytes; the apply gives each start its message index and leaves
//      the running sums at the start in a 32-byte row per message.
//   finish  one thread per message: the differences to the next start are
//      payload_size and n_fragments, the last fragment's fin and the next
//      message's connection decide FINAL / CUT / OPEN; the record goes out as
//      two 16-byte stores.
//   conn    one thread per connection: its first message, by a search over
//      the messages' connections (non-decreasing).
#include "cfws_tables.h"

namespace {

// A dense row's meta word.
constexpr uint32_t kRowFin = 0x100u, kRowOom = 0x200u;

// ws header words (u64): the scans' grand totals. kHdrStarts: message starts
// (low half) and out-of-memory rows (high half).
enum : int { kHdrData = 0, kHdrControl = 1, kHdrStarts = 2, kHdrBytes = 3 };

struct MsgLayout {
    TableHead t;
    uint64_t rows, bytes;
};

inline MsgLayout msg_layout(uint64_t n)
{
    MsgLayout L;
    L.t = table_head(n);
    L.rows = L.t.end;
    L.bytes = align_up(L.rows + 32 * n, 256);
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

// Frame f's class and the dense row it has as a data frame.
struct FrameClass {
    uint32_t cls;
    u32x4 row;
};

__device__ __forceinline__ FrameClass classify(const cfws_frame_desc_t* __restrict__ desc,
                                               const int32_t* __restrict__ status, uint64_t f)
{
    const uint64_t* q = reinterpret_cast<const uint64_t*>(desc) + 4 * f;
    const uint64_t size = q[2], w3 = q[3];
    const int32_t st = status ? status[f] : CFWS_PARSE_COMPLETE;
    const uint32_t opcode = (uint32_t)(w3 >> 40) & 0xffu, fin = (uint32_t)(w3 >> 32) & 0xffu;
    return {message_frame_class(st, opcode),
            u32x4{(uint32_t)size, (uint32_t)(size >> 32), (uint32_t)f,
                  opcode | (fin ? kRowFin : 0u) | (st == CFWS_ERROR_OUT_OF_MEMORY ? kRowOom : 0u)}};
}

// Over the frames: the dense rows of the data frames, the control list.
struct MsgFrames {
    const cfws_frame_desc_t* desc;
    const int32_t* status;
    uint64_t n;
    uint64_t* part[2];
    u32x4* dense;
    uint32_t* control;
    uint64_t control_cap;

    __device__ TableRows counts() const { return {n}; }
    __device__ FrameClass load(TableRows, uint64_t f) const { return classify(desc, status, f); }
    __device__ TableSums<1, true> weigh(const FrameClass& it) const     // data frames | control frames
    {
        return {{pack2(it.cls == kMessageFrameData ? 1u : 0u, it.cls == kMessageFrameControl ? 1u : 0u)}};
    }
    __device__ void emit(TableRows, uint64_t f, const FrameClass& it, const uint64_t* run) const
    {
        const uint64_t k = run[0] & 0xffffffffu, j = run[0] >> 32;
        if (it.cls == kMessageFrameData) dense[k] = it.row;
        else if (it.cls == kMessageFrameControl && j < control_cap) control[j] = (uint32_t)f;
    }
};

// The connection of frame f: the last c with conn_first[c] <= f (values above
// n_frames compare as n_frames, since f < n_frames); 0 without conn_first.
// *first gets conn_first[c].
__device__ __forceinline__ uint32_t conn_of(const uint64_t* __restrict__ conn_first, uint64_t n_conns, uint32_t f,
                                            uint64_t* first)
{
    *first = 0;
    if (!conn_first) return 0;
    const uint64_t after = lower_bound(0, n_conns, [&](uint64_t c) { return conn_first[c] <= f; });
    if (after <= 1) return 0;                   // connection 0 starts at frame 0
    *first = conn_first[after - 1];
    return (uint32_t)(after - 1);
}

// Does dense row k (`row`) start a message? `open` is the previous data
// frame's !fin when that frame is of the same connection.
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

// Over the dense rows: each start's message index and its row of running sums.
struct MsgStarts {
    struct Item { u32x4 row; RowStart s; };
    const cfws_frame_desc_t* desc;
    const u32x4* dense;
    const uint64_t* hdr;
    const uint64_t* conn_first;
    uint64_t n_conns;
    uint64_t* part[2];
    MsgRow* msg_rows;

    __device__ TableRows counts() const { return {hdr[kHdrData]}; }
    __device__ Item load(TableRows, uint64_t k) const
    {
        const u32x4 row = dense[k];
        return {row, row_start(dense, k, row, conn_first, n_conns)};
    }
    __device__ TableSums<2> weigh(const Item& it) const     // starts | out-of-memory rows, payload bytes
    {
        return {{pack2(it.s.starts ? 1u : 0u, (it.row.w & kRowOom) ? 1u : 0u), it.row.x | uint64_t(it.row.y) << 32}};
    }
    __device__ void emit(TableRows, uint64_t k, const Item& it, const uint64_t* run) const
    {
        if (!it.s.starts) return;
        const uint64_t off = desc[it.row.z].payload_off;
        u32x4* out = reinterpret_cast<u32x4*>(msg_rows + (run[0] & 0xffffffffu));
        out[0] = u32x4{(uint32_t)run[1], (uint32_t)(run[1] >> 32), (uint32_t)k, (uint32_t)(run[0] >> 32)};
        out[1] = u32x4{(uint32_t)off, (uint32_t)(off >> 32), it.s.conn, 0u};
    }
};

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

// One thread per connection: the messages of the connections before it (the
// first message whose connection is >= c).
__global__ void __launch_bounds__(kThreads)
messages_conn_kernel(const MsgRow* __restrict__ rows, const uint64_t* __restrict__ hdr, uint64_t n_conns,
                     uint64_t* __restrict__ conn_first_msg)
{
    const uint64_t c = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (c >= n_conns) return;
    conn_first_msg[c] = lower_bound(0, hdr[kHdrStarts] & 0xffffffffu, [&](uint64_t m) { return rows[m].conn < c; });
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
    return (size_t)kTableGroup;
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
    uint64_t* hdr = ws_ptr<uint64_t>(ws, L.t.hdr);
    uint64_t* part[4];
    for (int p = 0; p < 4; ++p) part[p] = ws_ptr<uint64_t>(ws, L.t.part[p]);
    u32x4* dense = ws_ptr<u32x4>(ws, L.t.dense);
    MsgRow* rows = ws_ptr<MsgRow>(ws, L.rows);
    const MsgFrames frames = {d_desc, d_status, n, {part[0], part[1]}, dense, d_control, control_cap};
    const MsgStarts starts = {d_desc, dense, hdr, d_conn_first, n_conns, {part[2], part[3]}, rows};
    const uint32_t nb = grid_for(n, kTableGroup);
    table_pass_kernel<kTableReduce><<<nb, kThreads, 0, st>>>(frames);
    scan_partials2_kernel<<<2, kThreads, 0, st>>>(part[0], part[1], nb, hdr + kHdrData, hdr + kHdrControl);
    table_pass_kernel<kTableApply><<<nb, kThreads, 0, st>>>(frames);
    // the dense list's length is on the device: the grids cover n_frames rows
    table_pass_kernel<kTableReduce><<<nb, kThreads, 0, st>>>(starts);
    scan_partials2_kernel<<<2, kThreads, 0, st>>>(part[2], part[3], nb, hdr + kHdrStarts, hdr + kHdrBytes);
    table_pass_kernel<kTableApply><<<nb, kThreads, 0, st>>>(starts);
    messages_finish_kernel<<<grid_for(n, kThreads), kThreads, 0, st>>>(dense, rows, hdr, d_msgs, msg_cap,
                                                                       d_n_messages, d_n_control);
    if (conns)
        messages_conn_kernel<<<grid_for(conns, kThreads), kThreads, 0, st>>>(rows, hdr, conns, d_conn_first_msg);
    return launch_check("messages");
}

}  // extern "C"
