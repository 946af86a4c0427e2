// l5dh_lanerow.hpp -- a wave's view of one row, for the per-row query kernels (k_le,
// k_quant, k_imp_dense, k_exp_count, k_exp_write): one wave per row, four per workgroup;
// lane l owns bins 28 l .. 28 l + 27 as groups 0..6, lane 63 also 1792..1797 as groups 7, 8.
#pragma once

#include "l5dh_device.hpp"

namespace l5dh {

// The grid of a one-wave-per-row launch of n rows with 256 threads per workgroup.
inline dim3 waves4(uint32_t n) { return dim3(n / 4 + (n % 4 != 0)); }

// Lane 63's groups 7 and 8 without a branch: every lane issues the two loads -- the other
// lanes at their own first bins, lines their groups 0 and 1 already bring -- and keeps
// zeros.  A load under `if (lane == 63)` makes the wave wait for everything in flight at
// the branch's join, one memory round trip per group.
__device__ __forceinline__ void lane_row_tail(const SrcRow32& s, bool tail, int own, uint4& t7, uint4& t8) {
  const uint4 a = *reinterpret_cast<const uint4*>(s.row + (tail ? 1792 : own));
  const uint4 b = *reinterpret_cast<const uint4*>(s.row + (tail ? 1796 : own));  // (rows are padded to ROW words)
  t7 = tail ? a : make_uint4(0u, 0u, 0u, 0u);
  t8 = tail ? make_uint4(b.x, b.y, 0u, 0u) : make_uint4(0u, 0u, 0u, 0u);
}
__device__ __forceinline__ void lane_row_tail(const SrcExt& s, bool tail, int own, uint4& t7, uint4& t8) {
  const int32_t* p = s.row + (tail ? 1792 : own);  // own <= 28 * 62: p + 5 stays inside the row
  const uint2 a0 = *reinterpret_cast<const uint2*>(p), a1 = *reinterpret_cast<const uint2*>(p + 2);
  const uint2 b0 = *reinterpret_cast<const uint2*>(p + 4);  // (lane 63: bins 1796, 1797, the row's last)
  t7 = tail ? make_uint4(a0.x, a0.y, a1.x, a1.y) : make_uint4(0u, 0u, 0u, 0u);
  t8 = tail ? make_uint4(b0.x, b0.y, 0u, 0u) : make_uint4(0u, 0u, 0u, 0u);
}

// One row's groups: lane l's 7 (lane 63: 9) 16-B loads, all in flight together; the groups
// a lane does not own are zeros.
template <class Src>
__device__ __forceinline__ void lane_row_load(const Src& src, uint4 (&v)[9]) {
  const int lane = lane_id();
#pragma unroll
  for (int q = 0; q < 7; ++q) v[q] = src.get4(28 * lane + 4 * q);
  lane_row_tail(src, lane == 63, 28 * lane, v[7], v[8]);
}

__device__ __forceinline__ uint64_t readlane64(uint64_t x, int k) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)(x >> 32), k) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((uint32_t)x, k);
}

}  // namespace l5dh
