// l5dh_le.hip -- exact cumulative `le` buckets (l5dh_le, l5dh_le_dense).
//
// What leaves the process as quantiles cannot be combined again; cumulative bucket
// counters can (`sum by (le)`, histogram_quantile).  A cut c in [1, 1797] stands for
// buckets 0..c-1 of a row -- the samples with (long)value <= L[c-1] - 1 -- so the count
// at a cut is an exact prefix sum of the row's integer buckets, carried in 64 bits.
//
//   k_le   one wave per row (four per workgroup, as k_rows): lane l loads its groups
//          (bins 28 l .. 28 l + 27, lane 63 also 1792..1797; 16-B loads) into WideSums,
//          the lane totals go through the 64-bit wave scan, and lane k < K resolves cut
//          k the way lanes 0..7 of wave_summary resolve their targets: the owner lane
//          min(c / 28, 63), its exclusive prefix by shuffle, its whole groups below the
//          cut (a statically unrolled loop of 9 shuffles), one get4 of the group the cut
//          falls in when c % 4 != 0.  Lanes 0..K-1 write the K counts as consecutive u64
//          words, then the row's count (word K) follows.
#include "l5dh_lanerow.hpp"
#include "l5dh_le.hpp"

namespace l5dh {
namespace {

// The count at this lane's cut c (mine: the lane holds a cut; the other lanes only take
// part in the shuffles) and the row's count, from the loaded groups.  Whole waves.
template <class Src>
__device__ __forceinline__ void le_resolve(const uint4 (&v)[9], const Src& src, uint32_t c, bool mine, uint64_t& at_cut,
                                           uint64_t& num) {
  WideSums g;
  g.clear();
#pragma unroll
  for (int q = 0; q < 9; ++q) g.set(q, v[q]);  // (groups the lane does not own: zeros)
  uint64_t ls = 0ull;
#pragma unroll
  for (int q = 0; q < 9; ++q) ls += sums_get(g, q);
  const uint64_t incl = wave_incl_scan(ls);
  const uint64_t excl = incl - ls;
  num = readlane64(incl, 63);
  const int owner = min((int)(c / 28u), 63);
  const int below = (int)c - 28 * owner;  // the owner's bins under the cut: 0..27 (lane 63: 0..33)
  const int nq = below >> 2, rem = below & 3;
  at_cut = __shfl(excl, owner, 64);
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const uint64_t gq = sums_get(g, q, owner);
    if (q < nq) at_cut += gq;
  }
  if (mine && rem != 0) {  // (nq <= 6, lane 63: <= 8: a group of the owner)
    const uint4 x = src.get4(28 * owner + 4 * nq);
    at_cut += x.x;
    if (rem >= 2) at_cut += x.y;
    if (rem == 3) at_cut += x.z;
  }
}

// dirty: the tiles' live flags (state rows: a row of a clean tile is never read and
// contributes zeros, as in k_rows), or nullptr (external rows: every row is read).
// (Two rows per wave with their loads in flight together, as k_ru_accum has them, was
// measured and is slower here: DESIGN 6f.)
template <class Rows>
__global__ __launch_bounds__(256) void k_le(Rows rows, const uint8_t* __restrict__ dirty, uint32_t first,
                                            uint32_t count, LeCuts cuts, uint32_t K, uint64_t* __restrict__ le_out,
                                            int64_t* __restrict__ sums_out, int accumulate) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= count) return;  // (whole waves)
  const int lane = lane_id();
  const bool mine = (uint32_t)lane < K;
  // lane k < K: cut k (the other lanes go through the shuffles with cut 0's owner)
  const uint32_t c = cuts.c[mine ? lane : 0];
  uint64_t at_cut = 0ull, num = 0ull, sum = 0ull;
  if (dirty == nullptr || dirty[(first + i) >> TILE_SHIFT] != 0) {  // (wave-uniform)
    const auto src = rows.row(i);
    sum = rows.sum(i);  // (with the row's loads, not after the cut's)
    uint4 v[9];
    lane_row_load(src, v);
    le_resolve(v, src, c, mine, at_cut, num);
  }
  uint64_t* __restrict__ orow = le_out + (size_t)i * (K + 1);
  if (mine) orow[lane] = accumulate ? orow[lane] + at_cut : at_cut;
  // the row's count: lane K (K = 64: lane 0 once more)
  if ((uint32_t)lane == (K & 63u)) orow[K] = accumulate ? orow[K] + num : num;
  if (sums_out && lane == 0) sums_out[i] = (int64_t)(accumulate ? (uint64_t)sums_out[i] + sum : sum);
}

}  // namespace

hipError_t launch_le(State state, uint32_t first, uint32_t count, const int32_t* ext, const int64_t* ext_total,
                     const LeCuts& cuts, uint32_t K, uint64_t* le_out, int64_t* sums_out, int accumulate,
                     hipStream_t st) {
  if (K == 0 || K > LE_MAX || !le_out) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  const dim3 grid = waves4(count), block(256);
  if (ext)
    hipLaunchKernelGGL(k_le<ExtRows>, grid, block, 0, st, ExtRows{ext, ext_total}, (const uint8_t*)nullptr, 0u, count,
                       cuts, K, le_out, sums_out, accumulate);
  else
    hipLaunchKernelGGL(k_le<LiveRows>, grid, block, 0, st, LiveRows{state.counts, state.total, state.sumfix, first},
                       (const uint8_t*)state.dirty, first, count, cuts, K, le_out, sums_out, accumulate);
  return hipGetLastError();
}

}  // namespace l5dh
