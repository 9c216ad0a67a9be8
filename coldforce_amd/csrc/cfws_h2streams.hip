// cfws_h2streams.hip -- HTTP/2 DATA frames of many streams, by message, on
// the device (cfws_h2_streams_batch, include/cfws.h). The
// rule is written once (cfws_rules.h: h2_stream_pooled, h2_stream_starts,
// h2_stream_closes, h2_stream_msg_flags) and shared with the host form
// (cfws_index.cpp). A unit of its own: no existing path changes.
//
// Every launch is a plain kernel; their number depends on n_frames alone.
//   A      pooled records (DATA, stream != 0) compacted into a dense list of
//          16-byte rows (stream id, record index, length, flags): reduce ->
//          scan_partials_kernel -> apply, as cfws_messages.hip. Connections
//          stay contiguous; one thread per connection finds its first dense
//          row (a search over the rows' record indices).
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
//   B      over the grouped keys, where a frame's predecessor is the row
//          before it: run starts, running length and PADDED sums (reduce ->
//          scan_partials2_kernel -> apply); a 32-byte row per run and each
//          grouped row's run.
//   C      over the runs: closed (the last frame has END_STREAM) or tail;
//          closed runs, their frames and FIRST flags summed the same way; the
//          apply writes the records (closed first, tails after), stream_first
//          and the counts, and leaves each run's place in d_order.
//   order  one thread per grouped row: d_order, d_order_frame.
//   conn   one thread per connection: its first closed message.
#include "cfws_kernels.h"

namespace {

constexpr int kStItems = 4;                                     // consecutive rows per thread
constexpr uint64_t kStGroup = uint64_t(kThreads) * kStItems;    // rows per workgroup of the table passes
constexpr uint32_t kSortBits = 11;
constexpr uint32_t kSortTile = 1u << kSortBits;                 // rows one workgroup sorts in LDS
constexpr int kSortPer = kSortTile / kThreads;                  // rows per thread of the sort

// ws header words (u64): the scans' grand totals
enum : int { kHdrData = 0, kHdrRuns = 1, kHdrBytes = 2, kHdrClosed = 3, kHdrClosedFrames = 4 };

// Two counts of at most n_frames <= 2^32 - 1 each in one sum.
__host__ __device__ inline uint64_t pack2(uint32_t lo, uint32_t hi) { return lo | uint64_t(hi) << 32; }

struct StLayout {
    uint64_t hdr, part[4], dense, keys[3], run_of, runs, tile_passes, dfirst, bytes;
    uint32_t passes;       // merge passes: tiles of kSortTile -> one run of n rows
};

inline StLayout st_layout(uint64_t n, uint64_t conns)
{
    StLayout L;
    const uint64_t nb = grid_for(n, kStGroup), tiles = grid_for(n, kSortTile);
    uint64_t at = 0;
    L.hdr = at; at += 256;
    for (int p = 0; p < 4; ++p) { L.part[p] = at; at = align_up(at + 8 * (nb + 1), 256); }
    L.dense = at; at = align_up(at + 16 * n, 256);
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
__device__ __forceinline__ bool pooled_row(const cfws_h2_frame_info_t* __restrict__ info, uint64_t f, u32x4* row)
{
    const cfws_h2_frame_info_t i = info[f];
    *row = u32x4{i.stream_id, (uint32_t)f, i.length, i.flags};
    return h2_stream_pooled(i.type, i.stream_id);
}

// A: per-group counts of pooled records.
__global__ void __launch_bounds__(kThreads)
h2streams_count_kernel(const cfws_h2_frame_info_t* __restrict__ info, uint64_t n, uint64_t* __restrict__ part)
{
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t f0 = uint64_t(blockIdx.x) * kStGroup + uint64_t(threadIdx.x) * kStItems;
    uint64_t x = 0;
    u32x4 row;
#pragma unroll
    for (int i = 0; i < kStItems; ++i)
        if (f0 + i < n && pooled_row(info, f0 + i, &row)) ++x;
    uint64_t total;
    block_exclusive_scan(x, s_wave, &total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// A's apply: the dense rows.
__global__ void __launch_bounds__(kThreads)
h2streams_compact_kernel(const cfws_h2_frame_info_t* __restrict__ info, uint64_t n,
                         const uint64_t* __restrict__ part, u32x4* __restrict__ dense)
{
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t f0 = uint64_t(blockIdx.x) * kStGroup + uint64_t(threadIdx.x) * kStItems;
    u32x4 row[kStItems];
    bool keep[kStItems];
    uint64_t x = 0;
#pragma unroll
    for (int i = 0; i < kStItems; ++i) {
        keep[i] = f0 + i < n && pooled_row(info, f0 + i, &row[i]);
        x += keep[i] ? 1u : 0u;
    }
    uint64_t total;
    uint64_t k = part[blockIdx.x] + block_exclusive_scan(x, s_wave, &total);
#pragma unroll
    for (int i = 0; i < kStItems; ++i)
        if (keep[i]) dense[k++] = row[i];
}

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
    const uint64_t nd = hdr[kHdrData];
    uint64_t lo = 0, hi = nd;
    if (c == 0) hi = 0;
    else if (c == conns) lo = nd;
    else {
        const uint64_t v = conn_first[c], b = v < n ? v : n;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (dense[mid].y < b) lo = mid + 1; else hi = mid;
        }
    }
    dfirst[c] = (uint32_t)lo;
}

// The connection of dense position i < nd: the last c with dfirst[c] <= i, its
// rows [*lo, *hi). Connections are contiguous and the grouping permutes rows
// inside a connection only, so a position's connection never changes. With a
// conn_first that breaks its precondition the position stands alone.
__device__ __forceinline__ uint32_t conn_range(const uint32_t* __restrict__ dfirst, uint64_t conns, uint32_t i,
                                               uint32_t* lo, uint32_t* hi)
{
    uint64_t a = 0, b = conns;
    while (a < b) {
        const uint64_t mid = (a + b) >> 1;
        if (dfirst[mid] <= i) a = mid + 1; else b = mid;
    }
    const uint64_t c = a ? a - 1 : 0;
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
    uint64_t a = lo, b = hi;
    while (a < b) {
        const uint64_t mid = (a + b) >> 1;
        if (src[mid] < key) a = mid + 1; else b = mid;
    }
    return a > lo ? a - lo : 0;
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

// B: per-group sums over the grouped rows: run starts | PADDED rows, lengths.
__global__ void __launch_bounds__(kThreads)
h2streams_starts_kernel(const u32x4* __restrict__ dense, const uint64_t* __restrict__ keys,
                        const uint64_t* __restrict__ hdr, const uint32_t* __restrict__ dfirst, uint64_t conns,
                        uint64_t* __restrict__ part_counts, uint64_t* __restrict__ part_bytes)
{
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t nd = hdr[kHdrData];
    const uint64_t r0 = uint64_t(blockIdx.x) * kStGroup + uint64_t(threadIdx.x) * kStItems;
    uint64_t counts = 0, bytes = 0;
#pragma unroll
    for (int i = 0; i < kStItems; ++i) {
        if (r0 + i < nd) {
            const u32x4 row = grouped_row(dense, keys, nd, r0 + i);
            const RunStart s = run_start(dense, keys, nd, r0 + i, row, dfirst, conns);
            counts += pack2(s.starts ? 1u : 0u, (row.w & kH2FlagPadded) ? 1u : 0u);
            bytes += row.z;
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

// B's apply: each start's run index and row of running sums; each row's run.
__global__ void __launch_bounds__(kThreads)
h2streams_runs_kernel(const u32x4* __restrict__ dense, const uint64_t* __restrict__ keys,
                      const uint64_t* __restrict__ hdr, const uint32_t* __restrict__ dfirst, uint64_t conns,
                      const uint64_t* __restrict__ part_counts, const uint64_t* __restrict__ part_bytes,
                      RunRow* __restrict__ runs, uint32_t* __restrict__ run_of)
{
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t nd = hdr[kHdrData];
    const uint64_t r0 = uint64_t(blockIdx.x) * kStGroup + uint64_t(threadIdx.x) * kStItems;
    u32x4 row[kStItems];
    RunStart s[kStItems];
    uint64_t counts = 0, bytes = 0;
#pragma unroll
    for (int i = 0; i < kStItems; ++i) {
        row[i] = u32x4{0, 0, 0, 0};
        s[i] = RunStart{false, false, 0};
        if (r0 + i < nd) {
            row[i] = grouped_row(dense, keys, nd, r0 + i);
            s[i] = run_start(dense, keys, nd, r0 + i, row[i], dfirst, conns);
            counts += pack2(s[i].starts ? 1u : 0u, (row[i].w & kH2FlagPadded) ? 1u : 0u);
            bytes += row[i].z;
        }
    }
    uint64_t total;
    uint64_t c = part_counts[blockIdx.x] + block_exclusive_scan(counts, s_wave, &total);
    uint64_t b = part_bytes[blockIdx.x] + block_exclusive_scan(bytes, s_wave, &total);
#pragma unroll
    for (int i = 0; i < kStItems; ++i) {
        if (r0 + i < nd) {
            if (s[i].starts) {
                u32x4* out = reinterpret_cast<u32x4*>(runs + (c & 0xffffffffu));
                out[0] = u32x4{(uint32_t)b, (uint32_t)(b >> 32), (uint32_t)(r0 + i), (uint32_t)(c >> 32)};
                out[1] = u32x4{s[i].conn, s[i].stream_start ? 1u : 0u, 0u, 0u};
            }
            c += pack2(s[i].starts ? 1u : 0u, (row[i].w & kH2FlagPadded) ? 1u : 0u);
            b += row[i].z;
            run_of[r0 + i] = (uint32_t)c - 1u;          // row 0 starts a run: c >= 1 here
        }
    }
}

// Run u from its row and the next run's (or the grand totals).
struct RunView {
    uint64_t length_sum;
    uint32_t r, n_data, conn, stream_id, end_frame, flags;
    bool closed, first;
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
    v.closed = h2_stream_closes(last.w);
    v.flags = h2_stream_msg_flags(v.closed, b.y != 0, next_padded != a.w);
    v.first = (v.flags & CFWS_H2_STREAM_FIRST) != 0;
    return v;
}

// C: per-group sums over the runs: closed runs | FIRST runs, closed frames.
__global__ void __launch_bounds__(kThreads)
h2streams_closed_kernel(const u32x4* __restrict__ dense, const uint64_t* __restrict__ keys,
                        const RunRow* __restrict__ runs, const uint64_t* __restrict__ hdr,
                        uint64_t* __restrict__ part_counts, uint64_t* __restrict__ part_frames)
{
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t n_runs = hdr[kHdrRuns] & 0xffffffffu;
    const uint64_t u0 = uint64_t(blockIdx.x) * kStGroup + uint64_t(threadIdx.x) * kStItems;
    uint64_t counts = 0, frames = 0;
#pragma unroll
    for (int i = 0; i < kStItems; ++i) {
        if (u0 + i < n_runs) {
            const RunView v = run_view(dense, keys, runs, hdr, u0 + i, n_runs);
            counts += pack2(v.closed ? 1u : 0u, v.first ? 1u : 0u);
            frames += v.closed ? v.n_data : 0u;
        }
    }
    uint64_t total_counts, total_frames;
    block_exclusive_scan(counts, s_wave, &total_counts);
    block_exclusive_scan(frames, s_wave, &total_frames);
    if (threadIdx.x == 0) {
        part_counts[blockIdx.x] = total_counts;
        part_frames[blockIdx.x] = total_frames;
    }
}

// C's apply: the records (closed runs from msgs[0], tails from msgs[M]),
// stream_first, each run's place in d_order and the closed runs before it;
// thread 0 writes the counts.
__global__ void __launch_bounds__(kThreads)
h2streams_records_kernel(const u32x4* __restrict__ dense, const uint64_t* __restrict__ keys,
                         RunRow* __restrict__ runs, const uint64_t* __restrict__ hdr,
                         const uint64_t* __restrict__ part_counts, const uint64_t* __restrict__ part_frames,
                         cfws_h2_stream_msg_t* __restrict__ msgs, uint64_t* __restrict__ stream_first,
                         uint64_t* __restrict__ out_counts)
{
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t nd = hdr[kHdrData], n_runs = hdr[kHdrRuns] & 0xffffffffu;
    const uint64_t n_closed = hdr[kHdrClosed] & 0xffffffffu, closed_frames = hdr[kHdrClosedFrames];
    const uint64_t u0 = uint64_t(blockIdx.x) * kStGroup + uint64_t(threadIdx.x) * kStItems;
    if (u0 == 0) {
        out_counts[0] = n_closed;
        out_counts[1] = closed_frames;
        out_counts[2] = n_runs - n_closed;
        out_counts[3] = nd - closed_frames;
        out_counts[4] = hdr[kHdrClosed] >> 32;
    }
    RunView v[kStItems];
    uint64_t counts = 0, frames = 0;
#pragma unroll
    for (int i = 0; i < kStItems; ++i) {
        v[i] = RunView{};
        if (u0 + i < n_runs) {
            v[i] = run_view(dense, keys, runs, hdr, u0 + i, n_runs);
            counts += pack2(v[i].closed ? 1u : 0u, v[i].first ? 1u : 0u);
            frames += v[i].closed ? v[i].n_data : 0u;
        }
    }
    uint64_t total;
    uint64_t c = part_counts[blockIdx.x] + block_exclusive_scan(counts, s_wave, &total);
    uint64_t fr = part_frames[blockIdx.x] + block_exclusive_scan(frames, s_wave, &total);
#pragma unroll
    for (int i = 0; i < kStItems; ++i) {
        if (u0 + i < n_runs) {
            const uint64_t closed_before = c & 0xffffffffu;
            // closed: after the closed frames before it; a tail: after all
            // closed frames and the tail frames before it
            const uint64_t m = v[i].closed ? closed_before : n_closed + (u0 + i - closed_before);
            const uint64_t base = v[i].closed ? fr : closed_frames + (v[i].r - fr);
            u32x4* out = reinterpret_cast<u32x4*>(msgs + m);
            out[0] = u32x4{(uint32_t)v[i].length_sum, (uint32_t)(v[i].length_sum >> 32), (uint32_t)base, v[i].n_data};
            out[1] = u32x4{v[i].conn, v[i].stream_id, v[i].end_frame, v[i].flags};
            if (v[i].first && stream_first) stream_first[c >> 32] = closed_before;
            runs[u0 + i].base = (uint32_t)base;
            runs[u0 + i].closed_before = (uint32_t)closed_before;
            c += pack2(v[i].closed ? 1u : 0u, v[i].first ? 1u : 0u);
            fr += v[i].closed ? v[i].n_data : 0u;
        }
    }
}

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

// One thread per connection: the closed messages of the connections before it.
__global__ void __launch_bounds__(kThreads)
h2streams_conn_kernel(const RunRow* __restrict__ runs, const uint64_t* __restrict__ hdr, uint64_t conns,
                      uint64_t* __restrict__ conn_first_msg)
{
    const uint64_t c = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (c >= conns) return;
    const uint64_t n_runs = hdr[kHdrRuns] & 0xffffffffu;
    uint64_t lo = 0, hi = n_runs;
    while (lo < hi) {                           // the first run whose connection is >= c
        const uint64_t mid = (lo + hi) >> 1;
        if (runs[mid].conn < c) lo = mid + 1; else hi = mid;
    }
    conn_first_msg[c] = lo < n_runs ? runs[lo].closed_before : hdr[kHdrClosed] & 0xffffffffu;
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
    uint64_t* hdr = ws_ptr<uint64_t>(ws, L.hdr);
    uint64_t* p0 = ws_ptr<uint64_t>(ws, L.part[0]);
    uint64_t* p1 = ws_ptr<uint64_t>(ws, L.part[1]);
    uint64_t* p2 = ws_ptr<uint64_t>(ws, L.part[2]);
    uint64_t* p3 = ws_ptr<uint64_t>(ws, L.part[3]);
    u32x4* dense = ws_ptr<u32x4>(ws, L.dense);
    uint64_t* ping = ws_ptr<uint64_t>(ws, L.keys[0]);
    uint64_t* pong = ws_ptr<uint64_t>(ws, L.keys[1]);
    uint64_t* keys = ws_ptr<uint64_t>(ws, L.keys[2]);
    uint32_t* run_of = ws_ptr<uint32_t>(ws, L.run_of);
    RunRow* runs = ws_ptr<RunRow>(ws, L.runs);
    uint32_t* tile_passes = ws_ptr<uint32_t>(ws, L.tile_passes);
    uint32_t* dfirst = ws_ptr<uint32_t>(ws, L.dfirst);
    const uint32_t nb = grid_for(n, kStGroup), rows = grid_for(n, kThreads);
    // the dense list's length is on the device: the grids cover n_frames rows
    h2streams_count_kernel<<<nb, kThreads, 0, st>>>(d_info, n, p0);
    scan_partials_kernel<<<1, kThreads, 0, st>>>(p0, nb, hdr + kHdrData);
    h2streams_compact_kernel<<<nb, kThreads, 0, st>>>(d_info, n, p0, dense);
    h2streams_conn_rows_kernel<<<grid_for(conns + 1, kThreads), kThreads, 0, st>>>(dense, hdr, d_conn_first, conns, n,
                                                                                  dfirst);
    h2streams_sort_kernel<<<grid_for(n, kSortTile), kThreads, 0, st>>>(dense, hdr, dfirst, conns, ping, keys,
                                                                       tile_passes);
    for (uint32_t p = 0; p < L.passes; ++p)
        h2streams_merge_kernel<<<rows, kThreads, 0, st>>>(hdr, dfirst, conns, tile_passes, p, (p & 1) ? pong : ping,
                                                          (p & 1) ? ping : pong, keys);
    h2streams_starts_kernel<<<nb, kThreads, 0, st>>>(dense, keys, hdr, dfirst, conns, p1, p2);
    scan_partials2_kernel<<<2, kThreads, 0, st>>>(p1, p2, nb, hdr + kHdrRuns, hdr + kHdrBytes);
    h2streams_runs_kernel<<<nb, kThreads, 0, st>>>(dense, keys, hdr, dfirst, conns, p1, p2, runs, run_of);
    h2streams_closed_kernel<<<nb, kThreads, 0, st>>>(dense, keys, runs, hdr, p0, p3);
    scan_partials2_kernel<<<2, kThreads, 0, st>>>(p0, p3, nb, hdr + kHdrClosed, hdr + kHdrClosedFrames);
    h2streams_records_kernel<<<nb, kThreads, 0, st>>>(dense, keys, runs, hdr, p0, p3, d_msgs, d_stream_first,
                                                      d_counts);
    h2streams_order_kernel<<<rows, kThreads, 0, st>>>(d_starts, dense, keys, runs, run_of, hdr, d_order,
                                                      d_order_frame);
    if (d_conn_first_msg)
        h2streams_conn_kernel<<<grid_for(conns, kThreads), kThreads, 0, st>>>(runs, hdr, conns, d_conn_first_msg);
    return launch_check("h2 streams");
}

}  // extern "C"
