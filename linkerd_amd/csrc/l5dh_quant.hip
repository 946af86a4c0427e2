// l5dh_quant.hip -- exact configurable quantiles (l5dh_quantiles, l5dh_quantiles_dense).
//
// The inverse of the cumulative `le` buckets: not "how many samples lie at or below this
// value" but "which value is the q-quantile", for any q in [0, 1] -- upstream
// BucketedHistogram.percentile(p), of which the summary only ever asks six.
//
//   k_quant  one wave per row (four per workgroup, as k_le): lane l loads its groups (bins
//            28 l .. 28 l + 27, lane 63 also 1792..1797; 16-B loads, all in flight together)
//            into WideSums, the lane totals go through the 64-bit wave scan, and lane k < K
//            computes its own target Math.round(q[k] * num).  Each lane then finds the owner
//            lane of its target -- the first lane whose inclusive prefix reaches it -- by a
//            binary search over the non-decreasing prefixes: six rounds of 64-bit shuffles,
//            whatever K is.  The value is resolved as lanes 0..7 of wave_summary resolve
//            theirs: the owner's exclusive prefix by shuffle, its nine group sums (a
//            statically unrolled loop of shuffles), one get4 of the group the target falls
//            in, the bin, mid[bin].  Lanes 0..K-1 write the K values as consecutive i64 words.
#include "l5dh_lanerow.hpp"
#include "l5dh_quant.hpp"

namespace l5dh {
namespace {

// The value of this lane's quantile p (mine: the lane holds one; the other lanes only take
// part in the shuffles, with target 0) from the loaded groups.  Whole waves.
template <class Src>
__device__ __forceinline__ int64_t quant_resolve(const uint4 (&v)[9], const Src& src, double p, bool mine,
                                                 const int32_t* __restrict__ mid) {
  WideSums g;
  g.clear();
#pragma unroll
  for (int k = 0; k < 9; ++k) g.set(k, v[k]);  // (groups the lane does not own: zeros)
  uint64_t ls = 0ull;
#pragma unroll
  for (int k = 0; k < 9; ++k) ls += sums_get(g, k);
  const uint64_t incl = wave_incl_scan(ls);
  const uint64_t excl = incl - ls;
  const uint64_t num = readlane64(incl, 63);
  // 0 <= p <= 1 and num < 2^42: the product is below 2^52 and the target at most num
  const uint64_t t = mine ? (uint64_t)java_round_nonneg(__dmul_rn(p, (double)num)) : 0ull;
  // the owner: the number of lanes whose inclusive prefix is below t (t <= num = lane 63's: <= 63)
  int owner = 0;
#pragma unroll
  for (int step = 32; step > 0; step >>= 1)
    if (__shfl(incl, owner + step - 1, 64) < t) owner += step;
  uint64_t acc = __shfl(excl, owner, 64);
  int gsel = 0;
  bool done = false;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const uint64_t gk = sums_get(g, k, owner);
    if (!done) {
      if (acc + gk >= t) {
        gsel = k;
        done = true;
      } else {
        acc += gk;
      }
    }
  }
  int64_t res = 0;
  if (mine && t != 0ull) {  // (excl < t <= incl of the owner: gsel is one of its groups)
    const int b0 = 28 * owner + 4 * gsel;
    const uint4 x = src.get4(b0);
    int b = b0 + 3;
    if (acc + x.x >= t)
      b = b0;
    else if (acc + x.x + x.y >= t)
      b = b0 + 1;
    else if (acc + x.x + x.y + x.z >= t)
      b = b0 + 2;
    res = mid[min(b, NB - 1)];
  }
  return res;
}

// dirty: the tiles' live flags (state rows: a row of a clean tile is never read and gives
// K zeros, as in k_le), or nullptr (external rows: every row is read).
template <class Rows>
__global__ __launch_bounds__(256) void k_quant(Rows rows, const uint8_t* __restrict__ dirty, uint32_t first,
                                               uint32_t count, QuantQ qs, uint32_t K,
                                               const int32_t* __restrict__ mid, int64_t* __restrict__ q_out) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= count) return;  // (whole waves)
  const int lane = lane_id();
  const bool mine = (uint32_t)lane < K;
  // lane k < K: quantile k, one load from the argument segment
  const double p = qs.q[mine ? lane : 0];
  int64_t res = 0;
  if (dirty == nullptr || dirty[(first + i) >> TILE_SHIFT] != 0) {  // (wave-uniform)
    const auto src = rows.row(i);
    uint4 v[9];
    lane_row_load(src, v);
    res = quant_resolve(v, src, p, mine, mid);
  }
  if (mine) q_out[(size_t)i * K + lane] = res;
}

}  // namespace

hipError_t launch_quant(State state, uint32_t first, uint32_t count, const int32_t* ext, const QuantQ& qs, uint32_t K,
                        const int32_t* mid, int64_t* q_out, hipStream_t st) {
  if (K == 0 || K > Q_MAX || !q_out || !mid) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  const dim3 grid = waves4(count), block(256);
  if (ext)
    hipLaunchKernelGGL(k_quant<ExtRows>, grid, block, 0, st, ExtRows{ext, nullptr}, (const uint8_t*)nullptr, 0u, count, qs,
                       K, mid, q_out);
  else
    hipLaunchKernelGGL(k_quant<LiveRows>, grid, block, 0, st, LiveRows{state.counts, state.total, state.sumfix, first},
                       (const uint8_t*)state.dirty, first, count, qs, K, mid, q_out);
  return hipGetLastError();
}

}  // namespace l5dh
