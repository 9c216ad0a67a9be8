// cfws_h2streams.hip -- HTTP/2 DATA frames of many streams, by message, on
// the device (cfws_h2_streams_batch, include/cfws.h). The
// rule is written once (cfws_rules.h: h2_stream_pooled, h2_stream_starts,
// h2_stream_closes, h2_stream_msg_flags) and shared with the host form
// (cfws_index.cpp). The three table passes (StRecords, StRuns, StClosed) are
// one struct each, their reduce and apply kernels one template over it
// (cfws_tables.h); the rest are plain kernels.
//
// Every launch is a plain kernel; their number depends on n_frames alone.
//   StRecords  pooled records (DATA, stream != 0) compacted into a dense list
//          of 16-byte rows (stream id, record index, length, flags): reduce
//          -> scan_partials_kernel -> apply. Connections stay contiguous; one
//          thread per connection finds its first dense row (a search over the
//          rows' record indices).
//   group  a stable sort of each connection's rows by stream id. The keys are
//          unique (stream id << 32 | dense row), so any sorting network is
//          stable. Every aligned tile of kSortTile rows is sorted in LDS by
//          (connection, stream id, row): a bitonic network over the tile's
//          power-of-two padding, which finishes every connection inside one
//          tile; small connections share the workgroup. A connection that
//          crosses a tile boundary has sorted pieces; merge pass p joins the
//          pieces in aligned windows of kSortTile << p rows pairwise, each
//          key finding its place by a binary search in the sibling run: at
//          most log2(n / kSortTile) passes of n log2 n comparisons for a
//          connection of n rows. A connection takes part in its first P
//          passes (P: the smallest window that holds it whole), ping-pongs
//          between two key arrays and lands in a third, so connections that
//          are finished are not copied again; a tile none of whose
//          connections takes part in a pass leaves it at once.
//   StRuns  over the grouped keys, where a frame's predecessor is the row
//          before it: run starts, running length and PADDED sums (reduce ->
//          scan_partials2_kernel -> apply); a 32-byte row per run and each
//          grouped row's run.
//   StClosed  over the runs: closed (the last frame has END_STREAM) or tail;
//          closed runs, their frames and FIRST flags summed the same way; the
//          apply writes the records (closed first, tails after), stream_first
//          and the counts, and leaves each run's place in d_order.
//   order  one thread per grouped row: d_order, d_order_frame.
//   conn   one thread per connection: its first closed message.
#include "cfws_tables.h"

namespace {

constexpr uint32_t kSortBits = 11;
constexpr uint32_t kSortTile = 1u << kSortBits;                 // rows one workgroup sorts in LDS
constexpr int kSortPer = kSortTile / kThreads;                  // rows per thread of the sort

// ws header words (u64): the scans' grand totals
enum : int { kHdrData = 0, kHdrRuns = 1, kHdrBytes = 2, kHdrClosed = 3, kHdrClosedFrames = 4 };

struct StLayout {
    TableHead t;
    uint64_t keys[3], run_of, runs, tile_passes, dfirst, bytes;
    uint32_t passes;       // merge passes: tiles of kSortTile -> one run of n rows
};

inline StLayout st_layout(uint64_t n, uint64_t conns)
{
    StLayout L;
    const uint64_t tiles = grid_for(n, kSortTile);
    L.t = table_head(n);
    uint64_t at = L.t.end;
    for (int p = 0; p < 3; ++p) { L.keys[p] = at; at = align_up(at + 8 * n, 256); }
    L.run_of = at; at = align_up(at + 4 * n, 256);
    L.runs = at; at = align_up(at + 32 * n, 256);
    L.tile_passes = at; at = align_up(at + 4 * tiles, 256);
    L.dfirst = at; at = align_up(at + 4 * (conns + 1), 256);
    L.bytes = at;
    L.passes = 0;
    while ((uint64_t(1) << L.passes) < tiles) ++L.passes;
    return L;
}

// The 32-byte row a run start leaves. Other runs' threads read the first half
// only; the second half is its own thread's.
struct RunRow {
    uint64_t bytes_before;     // lengths of the grouped rows before the start
    uint32_t r;                // the start's grouped row
    uint32_t padded_before;    // PADDED rows before the start
    uint32_t conn;
    uint32_t stream_start;     // the run is the first of its (connection, stream)
    uint32_t base;             // its first frame's position in d_order (C's apply)
    uint32_t closed_before;    // closed runs before it (C's apply)
};
static_assert(sizeof(RunRow) == 32 && sizeof(cfws_h2_stream_msg_t) == 32 && sizeof(cfws_h2_frame_info_t) == 16,
              "two 16-byte words each; one");

// Record f's dense row; is it pooled?
struct PooledRow {
    bool pooled;
    u32x4 row;
};

__device__ __forceinline__ PooledRow pooled_row(const cfws_h2_frame_info_t* __restrict__ info, uint64_t f)
{
    const cfws_h2_frame_info_t i = info[f];
    return {h2_stream_pooled(i.type, i.stream_id), u32x4{i.stream_id, (uint32_t)f, i.length, i.flags}};
}

// Over the records: the dense rows of the pooled ones.
struct StRecords {
    const cfws_h2_frame_info_t* info;
    uint64_t n;
    uint64_t* part[1];
    u32x4* dense;

    __device__ TableRows counts() const { return {n}; }
    __device__ PooledRow load(TableRows, uint64_t f) const { return pooled_row(info, f); }
    __device__ TableSums<1> weigh(const PooledRow& it) const { return {{it.pooled ? 1u : 0u}}; }
    __device__ void emit(TableRows, uint64_t, const PooledRow& it, const uint64_t* run) const
    {
        if (it.pooled) dense[run[0]] = it.row;
    }
};

// One thread per connection boundary c <= conns: dfirst[c], the dense rows of
// the connections before c (the first row whose record is at or past
// conn_first[c], a value above n read as n); dfirst[0] = 0, dfirst[conns] =
// all rows.
__global__ void __launch_bounds__(kThreads)
h2streams_conn_rows_kernel(const u32x4* __restrict__ dense, const uint64_t* __restrict__ hdr,
                           const uint64_t* __restrict__ conn_first, uint64_t conns, uint64_t n,
                           uint32_t* __restrict__ dfirst)
{
    const uint64_t c = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (c > conns) return;
    uint64_t at = c == 0 ? 0 : hdr[kHdrData];
    if (c != 0 && c != conns) {
        const uint64_t v = conn_first[c], b = v < n ? v : n;
        at = lower_bound(0, at, [&](uint64_t k) { return dense[k].y < b; });
    }
    dfirst[c] = (uint32_t)at;
}

// The connection of dense position i < nd: the last c with dfirst[c] <= i, its
// rows [*lo, *hi). Connections are contiguous and the grouping permutes rows
// inside a connection only, so a position's connection never changes. With a
// conn_first that breaks its precondition the position stands alone.
__device__ __forceinline__ uint32_t conn_range(const uint32_t* __restrict__ dfirst, uint64_t conns, uint32_t i,
                                               uint32_t* lo, uint32_t* hi)
{
    const uint64_t after = lower_bound(0, conns, [&](uint64_t k) { return dfirst[k] <= i; });
    const uint64_t c = after ? after - 1 : 0;
    *lo = dfirst[c];
    *hi = dfirst[c + 1];
    if (!(*lo <= i && i < *hi)) {
        *lo = i;
        *hi = i + 1;
    }
    return (uint32_t)c;
}

// The merge passes rows [lo, hi) take part in: the smallest p whose aligned
// window of kSortTile << p rows holds them all.
__device__ __forceinline__ uint32_t passes_of(uint32_t lo, uint32_t hi)
{
    const uint32_t x = (lo ^ (hi - 1u)) >> kSortBits;
    return x ? 32u - (uint32_t)__clz(x) : 0u;
}

// group, level 0: tile blockIdx.x's rows sorted in LDS by (connection, stream
// id, row). The LDS key is the connection's first row in the tile << 48 |
// stream id << 16 | row in the tile; what goes out is stream id << 32 | dense
// row, to `done` for a connection that lies inside the tile and to `next` for
// one that goes on to the merge passes. tile_passes: the most passes any of
// the tile's rows takes part in.
__global__ void __launch_bounds__(kThreads)
h2streams_sort_kernel(const u32x4* __restrict__ dense, const uint64_t* __restrict__ hdr,
                      const uint32_t* __restrict__ dfirst, uint64_t conns, uint64_t* __restrict__ next,
                      uint64_t* __restrict__ done, uint32_t* __restrict__ tile_passes)
{
    __shared__ uint64_t s_key[kSortTile];
    __shared__ uint32_t s_passes;
    const uint64_t nd = hdr[kHdrData];
    const uint64_t base = uint64_t(blockIdx.x) * kSortTile;
    if (base >= nd) {
        if (threadIdx.x == 0) tile_passes[blockIdx.x] = 0;
        return;
    }
    const uint32_t count = nd - base < kSortTile ? (uint32_t)(nd - base) : kSortTile;
    uint32_t width = 2;                                  // the network's size
    while (width < count) width <<= 1;
    if (threadIdx.x == 0) s_passes = 0;
    __syncthreads();
    uint32_t passes[kSortPer];
#pragma unroll
    for (int k = 0; k < kSortPer; ++k) {
        const uint32_t j = threadIdx.x + k * kThreads;
        passes[k] = 0;
        if (j < count) {
            uint32_t lo, hi;
            conn_range(dfirst, conns, (uint32_t)(base + j), &lo, &hi);
            passes[k] = passes_of(lo, hi);
            const uint64_t lo_tile = lo > base ? lo - base : 0;
            s_key[j] = lo_tile << 48 | uint64_t(dense[base + j].x) << 16 | j;
        } else if (j < width) {
            s_key[j] = ~uint64_t(0);
        }
    }
    uint32_t most = 0;
#pragma unroll
    for (int k = 0; k < kSortPer; ++k) most = passes[k] > most ? passes[k] : most;
    if (most) atomicMax(&s_passes, most);
    for (uint32_t k = 2; k <= width; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (uint32_t p = threadIdx.x; p < width / 2; p += kThreads) {
                const uint32_t i = ((p & ~(j - 1u)) << 1) | (p & (j - 1u)), l = i | j;
                const uint64_t a = s_key[i], b = s_key[l];
                if ((a > b) == ((i & k) == 0)) {
                    s_key[i] = b;
                    s_key[l] = a;
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) tile_passes[blockIdx.x] = s_passes;
#pragma unroll
    for (int k = 0; k < kSortPer; ++k) {
        const uint32_t j = threadIdx.x + k * kThreads;
        if (j < count) {
            const uint64_t key = s_key[j];
            const uint64_t out = (key >> 16 & 0xffffffffu) << 32 | (base + (key & 0xffffu));
            (passes[k] ? next : done)[base + j] = out;
        }
    }
}

// The keys of src[lo, hi) below `key`.
__device__ __forceinline__ uint64_t keys_below(const uint64_t* __restrict__ src, uint64_t lo, uint64_t hi,
                                               uint64_t key)
{
    const uint64_t at = lower_bound(lo, hi, [&](uint64_t k) { return src[k] < key; });
    return at > lo ? at - lo : 0;
}

// group, merge pass `pass`: one thread per dense position. In the aligned
// window of 2 * (kSortTile << pass) rows the position's connection has a
// sorted run in each half; the key's place in their merge is its place in its
// own run plus the sibling run's keys below it (the keys are unique). A
// connection's last pass writes to `done`.
__global__ void __launch_bounds__(kThreads)
h2streams_merge_kernel(const uint64_t* __restrict__ hdr, const uint32_t* __restrict__ dfirst, uint64_t conns,
                       const uint32_t* __restrict__ tile_passes, uint32_t pass, const uint64_t* __restrict__ src,
                       uint64_t* __restrict__ next, uint64_t* __restrict__ done)
{
    const uint64_t at = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (at >= hdr[kHdrData]) return;
    if (tile_passes[at >> kSortBits] <= pass) return;            // the whole workgroup: kThreads divides the tile
    const uint32_t i = (uint32_t)at;
    uint32_t lo, hi;
    conn_range(dfirst, conns, i, &lo, &hi);
    const uint32_t mine = passes_of(lo, hi);
    if (mine <= pass) return;
    const uint64_t run = uint64_t(kSortTile) << pass;
    const uint64_t w = at & ~(2 * run - 1), mid = w + run, end = w + 2 * run;
    // the runs [a_lo, a_hi) and [b_lo, b_hi); an empty one may have lo > hi
    const uint64_t a_lo = lo > w ? lo : w, a_hi = hi < mid ? hi : mid;
    const uint64_t b_lo = lo > mid ? lo : mid, b_hi = hi < end ? hi : end;
    const uint64_t key = src[i];
    uint64_t out = at;
    if (at < mid) out = at + keys_below(src, b_lo, b_hi, key);
    else if (a_lo < a_hi) out = a_lo + (at - b_lo) + keys_below(src, a_lo, a_hi, key);
    (mine == pass + 1 ? done : next)[out] = key;
}

// Grouped row r's dense row (a key's low half, kept inside the list whatever
// the connections held).
__device__ __forceinline__ u32x4 grouped_row(const u32x4* __restrict__ dense, const uint64_t* __restrict__ keys,
                                             uint64_t nd, uint64_t r)
{
    const uint64_t d = keys[r] & 0xffffffffu;
    return dense[d < nd ? d : nd - 1];
}

// Does grouped row r start a run?
struct RunStart {
    bool starts, stream_start;
    uint32_t conn;
};

__device__ __forceinline__ RunStart run_start(const u32x4* __restrict__ dense, const uint64_t* __restrict__ keys,
                                              uint64_t nd, uint64_t r, const u32x4& row,
                                              const uint32_t* __restrict__ dfirst, uint64_t conns)
{
    uint32_t lo, hi;
    RunStart s;
    s.conn = conn_range(dfirst, conns, (uint32_t)r, &lo, &hi);
    const bool first = r == lo;
    bool same = false, prev_closes = false;
    if (!first) {
        const u32x4 prev = grouped_row(dense, keys, nd, r - 1);
        same = prev.x == row.x;
        prev_closes = h2_stream_closes(prev.w);
    }
    s.stream_start = first || !same;
    s.starts = h2_stream_starts(first, same, prev_closes);
    return s;
}

// Over the grouped rows: each start's run index and row of running sums; each
// row's run.
struct StRuns {
    struct Item { u32x4 row; RunStart s; };
    const u32x4* dense;
    const uint64_t* keys;
    const uint64_t* hdr;
    const uint32_t* dfirst;
    uint64_t conns;
    uint64_t* part[2];
    RunRow* runs;
    uint32_t* run_of;

    __device__ TableRows counts() const { return {hdr[kHdrData]}; }
    __device__ Item load(TableRows c, uint64_t r) const
    {
        const u32x4 row = grouped_row(dense, keys, c.n, r);
        return {row, run_start(dense, keys, c.n, r, row, dfirst, conns)};
    }
    __device__ TableSums<2> weigh(const Item& it) const     // run starts | PADDED rows, lengths
    {
        return {{pack2(it.s.starts ? 1u : 0u, (it.row.w & kH2FlagPadded) ? 1u : 0u), it.row.z}};
    }
    __device__ void emit(TableRows, uint64_t r, const Item& it, const uint64_t* run) const
    {
        if (it.s.starts) {
            u32x4* out = reinterpret_cast<u32x4*>(runs + (run[0] & 0xffffffffu));
            out[0] = u32x4{(uint32_t)run[1], (uint32_t)(run[1] >> 32), (uint32_t)r, (uint32_t)(run[0] >> 32)};
            out[1] = u32x4{it.s.conn, it.s.stream_start ? 1u : 0u, 0u, 0u};
        }
        // every row, by the starts up to and including it (row 0 starts a run: >= 1)
        run_of[r] = (uint32_t)(run[0] + weigh(it).v[0]) - 1u;
    }
};

// Run u from its row and the next run's (or the grand totals).
struct RunView {
    uint64_t length_sum;
    uint32_t r, n_data, conn, stream_id, end_frame, flags;
    __device__ bool closed() const { return (flags & CFWS_H2_STREAM_CLOSED) != 0; }
    __device__ bool first() const { return (flags & CFWS_H2_STREAM_FIRST) != 0; }
};

__device__ __forceinline__ RunView run_view(const u32x4* __restrict__ dense, const uint64_t* __restrict__ keys,
                                            const RunRow* __restrict__ runs, const uint64_t* __restrict__ hdr,
                                            uint64_t u, uint64_t n_runs)
{
    const uint64_t nd = hdr[kHdrData];
    const u32x4* q = reinterpret_cast<const u32x4*>(runs + u);
    const u32x4 a = q[0], b = q[1];
    uint64_t next_bytes = hdr[kHdrBytes], next_r = nd;
    uint32_t next_padded = (uint32_t)(hdr[kHdrRuns] >> 32);
    if (u + 1 < n_runs) {
        const u32x4 na = q[2];
        next_bytes = na.x | uint64_t(na.y) << 32;
        next_r = na.z;
        next_padded = na.w;
    }
    const u32x4 last = grouped_row(dense, keys, nd, next_r - 1);
    RunView v;
    v.length_sum = next_bytes - (a.x | uint64_t(a.y) << 32);
    v.r = a.z;
    v.n_data = (uint32_t)(next_r - a.z);
    v.conn = b.x;
    v.stream_id = last.x;
    v.end_frame = last.y;
    v.flags = h2_stream_msg_flags(h2_stream_closes(last.w), b.y != 0, next_padded != a.w);
    return v;
}

// Over the runs: the records (closed runs from msgs[0], tails from msgs[M]),
// stream_first, each run's place in d_order and the closed runs before it.
struct StClosed {
    struct Counts { uint64_t n, data, closed, first, closed_frames; };  // n: the runs
    const u32x4* dense;
    const uint64_t* keys;
    RunRow* runs;
    const uint64_t* hdr;
    uint64_t* part[2];
    cfws_h2_stream_msg_t* msgs;
    uint64_t* stream_first;
    uint64_t* out_counts;

    __device__ Counts counts() const
    {
        return {hdr[kHdrRuns] & 0xffffffffu, hdr[kHdrData], hdr[kHdrClosed] & 0xffffffffu, hdr[kHdrClosed] >> 32,
                hdr[kHdrClosedFrames]};
    }
    __device__ RunView load(const Counts& c, uint64_t u) const { return run_view(dense, keys, runs, hdr, u, c.n); }
    __device__ TableSums<2> weigh(const RunView& v) const   // closed runs | FIRST runs, closed frames
    {
        return {{pack2(v.closed() ? 1u : 0u, v.first() ? 1u : 0u), v.closed() ? v.n_data : 0u}};
    }
    __device__ void emit(const Counts& c, uint64_t u, const RunView& v, const uint64_t* run) const
    {
        const uint64_t closed_before = run[0] & 0xffffffffu;
        // closed: after the closed frames before it; a tail: after all
        // closed frames and the tail frames before it
        const uint64_t m = v.closed() ? closed_before : c.closed + (u - closed_before);
        const uint64_t base = v.closed() ? run[1] : c.closed_frames + (v.r - run[1]);
        u32x4* out = reinterpret_cast<u32x4*>(msgs + m);
        out[0] = u32x4{(uint32_t)v.length_sum, (uint32_t)(v.length_sum >> 32), (uint32_t)base, v.n_data};
        out[1] = u32x4{v.conn, v.stream_id, v.end_frame, v.flags};
        if (v.first() && stream_first) stream_first[run[0] >> 32] = closed_before;
        runs[u].base = (uint32_t)base;
        runs[u].closed_before = (uint32_t)closed_before;
    }
    // the counts, also when nothing is pooled and no run exists
    __device__ void first_thread(const Counts& c) const
    {
        out_counts[0] = c.closed;
        out_counts[1] = c.closed_frames;
        out_counts[2] = c.n - c.closed;
        out_counts[3] = c.data - c.closed_frames;
        out_counts[4] = c.first;
    }
};

// One thread per grouped row: its frame's place in d_order.
__global__ void __launch_bounds__(kThreads)
h2streams_order_kernel(const uint64_t* __restrict__ starts, const u32x4* __restrict__ dense,
                       const uint64_t* __restrict__ keys, const RunRow* __restrict__ runs,
                       const uint32_t* __restrict__ run_of, const uint64_t* __restrict__ hdr,
                       uint64_t* __restrict__ order, uint32_t* __restrict__ order_frame)
{
    const uint64_t r = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t nd = hdr[kHdrData];
    if (r >= nd) return;
    const RunRow& run = runs[run_of[r]];
    const uint64_t at = run.base + (r - run.r);
    const uint32_t f = grouped_row(dense, keys, nd, r).y;
    order[at] = starts[f];
    if (order_frame) order_frame[at] = f;
}

// One thread per connection: the closed messages of the connections before it
// (those before the first run whose connection is >= c).
__global__ void __launch_bounds__(kThreads)
h2streams_conn_kernel(const RunRow* __restrict__ runs, const uint64_t* __restrict__ hdr, uint64_t conns,
                      uint64_t* __restrict__ conn_first_msg)
{
    const uint64_t c = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (c >= conns) return;
    const uint64_t n_runs = hdr[kHdrRuns] & 0xffffffffu;
    const uint64_t u = lower_bound(0, n_runs, [&](uint64_t k) { return runs[k].conn < c; });
    conn_first_msg[c] = u < n_runs ? runs[u].closed_before : hdr[kHdrClosed] & 0xffffffffu;
}

}  // namespace

extern "C" {

size_t cfws_h2_streams_workspace_size(size_t n_frames, size_t n_conns)
{
    return (size_t)st_layout(n_frames, n_conns ? n_conns : 1).bytes;
}

size_t cfws_h2_streams_group_frames(void)
{
    return (size_t)kSortTile;
}

int cfws_h2_streams_batch(const uint64_t* d_starts, const cfws_h2_frame_info_t* d_info, size_t n,
                          const uint64_t* d_conn_first, size_t n_conns, uint64_t* d_order, uint32_t* d_order_frame,
                          cfws_h2_stream_msg_t* d_msgs, uint64_t* d_conn_first_msg, uint64_t* d_stream_first,
                          uint64_t* d_counts, void* ws, size_t ws_size, void* stream)
{
    const CfwsPassScope pass_scope;     // not a timed pass: a pending pair is dropped
    if (int rc = check_init()) return rc;
    const uint64_t conns = d_conn_first ? n_conns : 1;
    if ((n && (!d_starts || !d_info || !d_order || !d_msgs)) || !d_counts || !ws ||
        (d_conn_first && n_conns && !d_conn_first_msg))
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "h2 streams: null pointer", hipSuccess);
    if (reinterpret_cast<uintptr_t>(d_msgs) & 15u)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "h2 streams: d_msgs must be 16-byte aligned", hipSuccess);
    if (n > 0xffffffffull)
        return set_err(CFWS_ERROR_INVALID_ARGUMENT, "h2 streams: n_frames above 2^32 - 1", hipSuccess);
    if (ws_size < cfws_h2_streams_workspace_size(n, n_conns))
        return set_err(CFWS_ERROR_WORKSPACE, "h2 streams workspace too small", hipSuccess);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0 || conns == 0) {                         // no record belongs to a connection
        (void)hipMemsetAsync(d_counts, 0, 5 * 8, st);
        if (conns && d_conn_first_msg) (void)hipMemsetAsync(d_conn_first_msg, 0, 8 * conns, st);
        return launch_check("h2 streams");
    }
    const StLayout L = st_layout(n, conns);
    uint64_t* hdr = ws_ptr<uint64_t>(ws, L.t.hdr);
    uint64_t* part[4];
    for (int p = 0; p < 4; ++p) part[p] = ws_ptr<uint64_t>(ws, L.t.part[p]);
    u32x4* dense = ws_ptr<u32x4>(ws, L.t.dense);
    uint64_t* ping = ws_ptr<uint64_t>(ws, L.keys[0]);
    uint64_t* pong = ws_ptr<uint64_t>(ws, L.keys[1]);
    uint64_t* keys = ws_ptr<uint64_t>(ws, L.keys[2]);
    uint32_t* run_of = ws_ptr<uint32_t>(ws, L.run_of);
    RunRow* runs = ws_ptr<RunRow>(ws, L.runs);
    uint32_t* tile_passes = ws_ptr<uint32_t>(ws, L.tile_passes);
    uint32_t* dfirst = ws_ptr<uint32_t>(ws, L.dfirst);
    // the block sums of StRecords are free again when StClosed needs a pair
    const StRecords records = {d_info, n, {part[0]}, dense};
    const StRuns group_runs = {dense, keys, hdr, dfirst, conns, {part[1], part[2]}, runs, run_of};
    const StClosed closed = {dense, keys, runs, hdr, {part[0], part[3]}, d_msgs, d_stream_first, d_counts};
    const uint32_t nb = grid_for(n, kTableGroup), rows = grid_for(n, kThreads);
    // the dense list's length is on the device: the grids cover n_frames rows
    table_pass_kernel<kTableReduce><<<nb, kThreads, 0, st>>>(records);
    scan_partials_kernel<<<1, kThreads, 0, st>>>(part[0], nb, hdr + kHdrData);
    table_pass_kernel<kTableApply><<<nb, kThreads, 0, st>>>(records);
    h2streams_conn_rows_kernel<<<grid_for(conns + 1, kThreads), kThreads, 0, st>>>(dense, hdr, d_conn_first, conns, n,
                                                                                  dfirst);
    h2streams_sort_kernel<<<grid_for(n, kSortTile), kThreads, 0, st>>>(dense, hdr, dfirst, conns, ping, keys,
                                                                       tile_passes);
    for (uint32_t p = 0; p < L.passes; ++p)
        h2streams_merge_kernel<<<rows, kThreads, 0, st>>>(hdr, dfirst, conns, tile_passes, p, (p & 1) ? pong : ping,
                                                          (p & 1) ? ping : pong, keys);
    table_pass_kernel<kTableReduce><<<nb, kThreads, 0, st>>>(group_runs);
    scan_partials2_kernel<<<2, kThreads, 0, st>>>(part[1], part[2], nb, hdr + kHdrRuns, hdr + kHdrBytes);
    table_pass_kernel<kTableApply><<<nb, kThreads, 0, st>>>(group_runs);
    table_pass_kernel<kTableReduce><<<nb, kThreads, 0, st>>>(closed);
    scan_partials2_kernel<<<2, kThreads, 0, st>>>(part[0], part[3], nb, hdr + kHdrClosed, hdr + kHdrClosedFrames);
    table_pass_kernel<kTableApply><<<nb, kThreads, 0, st>>>(closed);
    h2streams_order_kernel<<<rows, kThreads, 0, st>>>(d_starts, dense, keys, runs, run_of, hdr, d_order,
                                                      d_order_frame);
    if (d_conn_first_msg)
        h2streams_conn_kernel<<<grid_for(conns, kThreads), kThreads, 0, st>>>(runs, hdr, conns, d_conn_first_msg);
    return launch_check("h2 streams");
}

}  // extern "C"
