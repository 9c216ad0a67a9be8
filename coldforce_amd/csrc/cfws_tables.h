// cfws_tables.h -- table passes: what cfws_messages.hip, cfws_h2streams.hip
// and cfws_utf8.hip are built from, written
// once. Only those three units include it.
//
// A table pass goes over the rows of a table, kTableItems consecutive rows per
// thread. Each row is weighed into one or two 64-bit sums, and the sums are
// scanned: inside the workgroup here, between the workgroups by
// scan_partials_kernel / scan_partials2_kernel, launched between the pass's
// two kernels. Both kernels are table_pass_kernel over the same pass, so they
// cannot disagree about a row's weights:
//   reduce  stores the workgroup's totals into the pass's block-sum arrays;
//   apply   adds the scanned block sums in front and hands every row, with the
//           running sums before it, to the pass.
// A pass is a trivially copyable struct, passed to the kernel by value:
//   part[]          the block-sum arrays;
//   counts()        the words of the workspace header the pass needs, read
//                   once, before any store: a struct whose n is the table's
//                   length (TableRows where a host value is all there is);
//   load(c, i)      row i's item: what is kept of it until the emit;
//   weigh(item)     its weights: TableSums<1>, TableSums<2>, or TableSums<1,
//                   true> for two 32-bit counts in one sum (pack2) whose
//                   halves have a block-sum array each, so that two counts
//                   cost one block scan;
//   emit(c, i, item, run)   the apply's work for row i; run[] holds the sums
//                   over the rows before i;
//   first_thread(c) optional: called by the apply grid's first thread, also
//                   when the table is empty.
#ifndef CFWS_TABLES_H
#define CFWS_TABLES_H

#include "cfws_kernels.h"

namespace {

constexpr int kTableItems = 4;                                      // consecutive rows per thread
constexpr uint64_t kTableGroup = uint64_t(kThreads) * kTableItems;  // rows per workgroup
constexpr bool kTableReduce = false, kTableApply = true;

// Two counts of at most n_frames <= 2^32 - 1 each in one sum.
__host__ __device__ inline uint64_t pack2(uint32_t lo, uint32_t hi) { return lo | uint64_t(hi) << 32; }

template <int kN, bool kSplitHalves = false>
struct TableSums {
    static constexpr int kSums = kN;
    static constexpr bool kSplit = kSplitHalves;
    static_assert(kN == 1 || (kN == 2 && !kSplitHalves), "one sum, one split sum or two sums");
    uint64_t v[kN];
};

struct TableRows {
    uint64_t n;
};

// The first index in [lo, hi) for which `below` fails; `below` holds for a
// prefix of the range. hi when it never fails, lo when lo >= hi.
template <class Below>
__device__ __forceinline__ uint64_t lower_bound(uint64_t lo, uint64_t hi, Below below)
{
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (below(mid)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <class Pass, class Counts>
__device__ __forceinline__ auto table_first_thread(const Pass& p, const Counts& c, int) -> decltype(p.first_thread(c))
{
    p.first_thread(c);
}
template <class Pass, class Counts>
__device__ __forceinline__ void table_first_thread(const Pass&, const Counts&, long) {}

template <bool kApply, class Pass>
__global__ void __launch_bounds__(kThreads) table_pass_kernel(const Pass p)
{
    __shared__ uint64_t s_wave[kWaves];
    const auto c = p.counts();
    const uint64_t i0 = uint64_t(blockIdx.x) * kTableGroup + uint64_t(threadIdx.x) * kTableItems;
    decltype(p.load(c, i0)) item[kTableItems];
    using Sums = decltype(p.weigh(item[0]));
    constexpr int kSums = Sums::kSums;
    uint64_t run[kSums] = {};
#pragma unroll
    for (int i = 0; i < kTableItems; ++i) {
        if (i0 + i < c.n) {
            item[i] = p.load(c, i0 + i);
            const Sums w = p.weigh(item[i]);
            for (int s = 0; s < kSums; ++s) run[s] += w.v[s];
        }
    }
    uint64_t total[kSums];
    for (int s = 0; s < kSums; ++s) run[s] = block_exclusive_scan(run[s], s_wave, &total[s]);
    if constexpr (!kApply) {
        if (threadIdx.x != 0) return;
        if constexpr (Sums::kSplit) {
            p.part[0][blockIdx.x] = total[0] & 0xffffffffu;
            p.part[1][blockIdx.x] = total[0] >> 32;
        } else {
            for (int s = 0; s < kSums; ++s) p.part[s][blockIdx.x] = total[s];
        }
    } else {
        // a split sum stays packed: neither half exceeds the table's length
        if constexpr (Sums::kSplit) run[0] += pack2((uint32_t)p.part[0][blockIdx.x], (uint32_t)p.part[1][blockIdx.x]);
        else for (int s = 0; s < kSums; ++s) run[s] += p.part[s][blockIdx.x];
#pragma unroll
        for (int i = 0; i < kTableItems; ++i) {
            if (i0 + i < c.n) {
                p.emit(c, i0 + i, item[i], run);
                const Sums w = p.weigh(item[i]);
                for (int s = 0; s < kSums; ++s) run[s] += w.v[s];
            }
        }
        // last, so that its stores do not stand between the loads above and their uses
        if (i0 == 0) table_first_thread(p, c, 0);
    }
}

// The head both workspaces share: 256 bytes of totals, four block-sum arrays,
// 16-byte dense rows; `end` is where the unit's own arrays begin.
struct TableHead {
    uint64_t hdr, part[4], dense, end;
};

inline TableHead table_head(uint64_t n)
{
    TableHead L;
    const uint64_t nb = grid_for(n, kTableGroup);
    uint64_t at = 0;
    L.hdr = at; at += 256;
    for (int p = 0; p < 4; ++p) { L.part[p] = at; at = align_up(at + 8 * (nb + 1), 256); }
    L.dense = at; at = align_up(at + 16 * n, 256);
    L.end = at;
    return L;
}

}  // namespace

#endif  // CFWS_TABLES_H
