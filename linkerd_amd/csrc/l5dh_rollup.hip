// l5dh_rollup.hip -- label rollups (l5dh_rollup, l5dh_rollup_dense).
//
// The histogram of a union of series is the element-wise integer sum of their bucket
// rows, so a group's summary is exact: what ONE Stat would report had it received
// every member's samples.  A call sums the rows of series [first, first + count) per
// group of a caller map (group[i] < G, or RU_NO_GROUP) in these steps:
//
//   k_ru_init    zero the per-group counters and the status words
//   k_ru_count   members per group; map entries validated (RH_BADIDX); a live series
//                of a clean tile is no member (its row is never read, as in k_rows)
//   k_ru_items   items per group by the work-item rule (ru_items)
//   k_scan_*     member and item offsets (the fleet merge's scan)
//   k_ru_plan    item -> group; groups of several items get partial rows
//   k_ru_fill    the members of each group (a CSR; the order inside a group is
//                arbitrary -- integer sums do not depend on it)
//   k_ru_accum   one wave per item: the members' rows summed in lane-owned u64
//                registers (lane l: bins 28 l .. 28 l + 27, lane 63 also 1792..1797;
//                16-B loads).  The only item of a group finishes it (range check,
//                dense row, total, wave_summary over an LDS copy of the row); an item
//                of a larger group stores its exact u64 partial row
//   k_ru_finish  one workgroup per group of several items: its waves stride over the
//                partial rows, add into one u64 LDS row, and wave 0 finishes the group
//
// Sums are u64 from the first add to the range check, so a bucket sum is known exactly
// however a group is cut (also beyond 2^32); any above 2^31 - 1 is reported (RH_RANGE:
// the least such group), never wrapped.  The totals wrap like a Java long.
#include <algorithm>

#include "l5dh_device.hpp"
#include "l5dh_merge.hpp"
#include "l5dh_rollup.hpp"

namespace l5dh {
namespace {

// (the row sources of the accumulate kernel, member i of the map: LiveRows / ExtRows of
// l5dh_device.hpp)

// The group series first + i is a member of, or RU_NO_GROUP.  An invalid entry counts
// as no group (bad != nullptr: its index is reported).
template <bool LIVE>
__device__ __forceinline__ uint32_t member_group(const RollupWork& w, const uint8_t* __restrict__ dirty, uint32_t i,
                                                 uint32_t* bad) {
  if (i >= w.count) return RU_NO_GROUP;
  const uint32_t gid = w.group[i];
  if (gid == RU_NO_GROUP) return RU_NO_GROUP;
  if (gid >= w.G) {
    if (bad) atomicMin(bad, i);
    return RU_NO_GROUP;
  }
  if (LIVE && dirty[(w.first + i) >> TILE_SHIFT] == 0) return RU_NO_GROUP;
  return gid;
}

__global__ __launch_bounds__(256) void k_ru_init(RollupWork w) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i <= w.G) w.cnt[i] = 0u;
  if (i < w.G) w.cursor[i] = 0u;
  if (i < RH_WORDS) w.hdr[i] = (i == RH_BADIDX || i == RH_RANGE) ? 0xFFFFFFFFu : 0u;
}

template <bool LIVE>
__global__ __launch_bounds__(256) void k_ru_count(RollupWork w, const uint8_t* __restrict__ dirty) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t gid = member_group<LIVE>(w, dirty, i, w.hdr + RH_BADIDX);
  // (whole waves: lanes past the map take part with no group)
  wave_atomic_inc<2>(w.cnt, gid, gid != RU_NO_GROUP);
}

__global__ __launch_bounds__(256) void k_ru_items(RollupWork w) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g <= w.G) w.nitems[g] = g < w.G ? ru_items(w.cnt[g], w.item) : 0u;
}

__global__ __launch_bounds__(256) void k_ru_plan(RollupWork w) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= w.G) return;
  const uint32_t ni = w.nitems[g];
  const uint64_t io = w.ioff[g];
  if (io + ni > (uint64_t)w.caps.items) {
    atomicOr(w.hdr + RH_BOUNDS, 1u);
    return;
  }
  for (uint32_t j = 0; j < ni; ++j) w.igroup[io + j] = g;
  uint32_t base = 0xFFFFFFFFu;
  if (ni > 1) {
    const uint32_t b = atomicAdd(w.hdr + RH_SLOTS, ni);
    const uint32_t k = atomicAdd(w.hdr + RH_NMULTI, 1u);
    if ((uint64_t)b + ni <= (uint64_t)w.caps.slots && k < w.caps.multi) {
      base = b;
      w.mlist[k] = g;
    } else {
      atomicOr(w.hdr + RH_BOUNDS, 2u);
    }
  }
  w.pbase[g] = base;
}

template <bool LIVE>
__global__ __launch_bounds__(256) void k_ru_fill(RollupWork w, const uint8_t* __restrict__ dirty) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t gid = member_group<LIVE>(w, dirty, i, nullptr);
  const bool valid = gid != RU_NO_GROUP;
  const uint32_t pos = wave_atomic_rank<2>(w.cursor, gid, valid);
  if (valid) {
    const uint64_t at = w.moff[gid] + pos;
    if (pos < w.cnt[gid] && at < (uint64_t)w.count)
      w.members[at] = i;
    else
      atomicOr(w.hdr + RH_BOUNDS, 4u);
  }
}

// ---- lane-owned u64 bins ----
struct Acc {
  uint64_t a[9][4];  // group q of this lane: bins 28 lane + 4 q .. + 3 (q >= 7: lane 63 only)
};

__device__ __forceinline__ void acc_zero(Acc& x) {
#pragma unroll
  for (int q = 0; q < 9; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j) x.a[q][j] = 0ull;
}

template <class Src>
__device__ __forceinline__ void row_load(const Src& src, uint4 (&v)[9]) {
  const int lane = lane_id();
  const int ng = lane_groups(lane);
#pragma unroll
  for (int q = 0; q < 9; ++q) v[q] = q < ng ? src.get4(28 * lane + 4 * q) : make_uint4(0u, 0u, 0u, 0u);
}

__device__ __forceinline__ void acc_add(Acc& x, const uint4 (&v)[9]) {
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    x.a[q][0] += v[q].x;
    x.a[q][1] += v[q].y;
    x.a[q][2] += v[q].z;
    x.a[q][3] += v[q].w;
  }
}

// The end of group g (one wave): range check, the dense row, the total, the summary.
// lrow: this wave's u32 LDS row (wave_summary locates its bins there).
__device__ __forceinline__ void finish_group(const Acc& x, uint64_t total, uint32_t g, uint32_t* lrow, const Tables& tb,
                                             const RollupOut& out, uint32_t* hdr) {
  const int lane = lane_id();
  const int ng = lane_groups(lane);
  uint64_t mx = 0ull;
#pragma unroll
  for (int q = 0; q < 9; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j) mx = x.a[q][j] > mx ? x.a[q][j] : mx;
  if (__ballot(mx > (uint64_t)INT_MAXV) != 0ull && lane == 0) atomicMin(hdr + RH_RANGE, g);
  WideSums gs;  // (four bucket sums of 2^31 - 1 each pass 2^32)
  gs.clear();
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const uint4 v = make_uint4((uint32_t)x.a[q][0], (uint32_t)x.a[q][1], (uint32_t)x.a[q][2], (uint32_t)x.a[q][3]);
    if (q < ng) {
      gs.set(q, v);
      store4_state(lrow, 28 * lane + 4 * q, v);  // (bins 1798, 1799: zero sums)
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  const SrcLds32 lds{lrow};
  if (out.counts) {
    int32_t* orow = out.counts + (size_t)g * NB;
    for (int q = lane; q < NB4; q += 64) store4_1798(orow, 4 * q, lds.get4(4 * q));
  }
  if (out.totals && lane == 0) out.totals[g] = (int64_t)total;
  if (out.summ) wave_summary(gs, lds, (int64_t)total, tb.mid, out.summ + g);
}

// One wave per item.
template <class Rows>
__global__ __launch_bounds__(64) void k_ru_accum(RollupWork w, Rows rows, Tables tb, RollupOut out) {
  __shared__ __attribute__((aligned(16))) uint32_t lrow[ROW];
  const uint32_t item = blockIdx.x;
  if ((uint64_t)item >= w.ioff[w.G] || item >= w.caps.items) return;
  const uint32_t g = w.igroup[item];
  const uint32_t c = w.cnt[g], per = ru_per_item(c, w.item), ni = w.nitems[g];
  const uint32_t j = item - (uint32_t)w.ioff[g];
  const uint32_t a = min(j * per, c), b = min(a + per, c);  // (j < 1024, per <= 2^20)
  const uint32_t* __restrict__ mem = w.members + w.moff[g];
  Acc x;
  acc_zero(x);
  uint64_t total = 0ull;
  uint32_t k = a;
  for (; k + 1 < b; k += 2) {  // two rows' loads in flight
    const uint32_t i0 = mem[k], i1 = mem[k + 1];
    uint4 v0[9], v1[9];
    row_load(rows.row(i0), v0);
    row_load(rows.row(i1), v1);
    total += rows.sum(i0) + rows.sum(i1);
    acc_add(x, v0);
    acc_add(x, v1);
  }
  if (k < b) {
    const uint32_t i0 = mem[k];
    uint4 v0[9];
    row_load(rows.row(i0), v0);
    total += rows.sum(i0);
    acc_add(x, v0);
  }
  if (ni == 1) {
    finish_group(x, total, g, lrow, tb, out, w.hdr);
    return;
  }
  const uint32_t base = w.pbase[g];
  if (base == 0xFFFFFFFFu) return;  // (RH_BOUNDS is set)
  const int lane = lane_id();
  const int ng = lane_groups(lane);
  uint64_t* __restrict__ p = w.partial + (size_t)(base + j) * RU_PROW;
  if (lane == 63) x.a[8][2] = total;  // word NB of the partial row
#pragma unroll
  for (int q = 0; q < 9; ++q)
    if (q < ng) {
      ulonglong2* d = reinterpret_cast<ulonglong2*>(p + 28 * lane + 4 * q);
      d[0] = make_ulonglong2(x.a[q][0], x.a[q][1]);
      d[1] = make_ulonglong2(x.a[q][2], x.a[q][3]);
    }
}

// One workgroup per group of several items.
constexpr int RU_FIN_WAVES = 8;
__global__ __launch_bounds__(64 * RU_FIN_WAVES) void k_ru_finish(RollupWork w, Tables tb, RollupOut out) {
  __shared__ __attribute__((aligned(16))) unsigned long long lsum[RU_PROW];
  __shared__ __attribute__((aligned(16))) uint32_t lrow[ROW];
  if (blockIdx.x >= w.hdr[RH_NMULTI] || blockIdx.x >= w.caps.multi) return;  // (workgroup-uniform)
  const uint32_t g = w.mlist[blockIdx.x];
  const uint32_t ni = w.nitems[g], base = w.pbase[g];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const int ng = lane_groups(lane);
  for (int b = threadIdx.x; b < RU_PROW; b += 64 * RU_FIN_WAVES) lsum[b] = 0ull;
  __syncthreads();
  if ((uint32_t)wv < ni) {
    Acc x;
    acc_zero(x);
    for (uint32_t j = wv; j < ni; j += RU_FIN_WAVES) {
      const uint64_t* __restrict__ p = w.partial + (size_t)(base + j) * RU_PROW;
#pragma unroll
      for (int q = 0; q < 9; ++q)
        if (q < ng) {
          const ulonglong2* s = reinterpret_cast<const ulonglong2*>(p + 28 * lane + 4 * q);
          const ulonglong2 lo = s[0], hi = s[1];
          x.a[q][0] += lo.x;
          x.a[q][1] += lo.y;
          x.a[q][2] += hi.x;
          x.a[q][3] += hi.y;
        }
    }
#pragma unroll
    for (int q = 0; q < 9; ++q)
      if (q < ng) {
#pragma unroll
        for (int e = 0; e < 4; ++e) atomicAdd(&lsum[28 * lane + 4 * q + e], (unsigned long long)x.a[q][e]);
      }
  }
  __syncthreads();
  if (wv != 0) return;
  Acc x;
  acc_zero(x);
#pragma unroll
  for (int q = 0; q < 9; ++q)
    if (q < ng) {
#pragma unroll
      for (int e = 0; e < 4; ++e) x.a[q][e] = lsum[28 * lane + 4 * q + e];
    }
  const uint64_t total = lsum[NB];
  if (lane == 63) x.a[8][2] = 0ull;  // (word NB held the items' totals)
  finish_group(x, total, g, lrow, tb, out, w.hdr);
}

}  // namespace

size_t rollup_tmp_bytes(uint32_t G) {
  size_t bytes = 0;
  merge_count(G + 1, nullptr, nullptr, nullptr, &bytes, nullptr);
  return bytes;
}

hipError_t launch_rollup(const RollupWork& w, State state, const int32_t* ext, const int64_t* ext_total, Tables tb,
                         RollupOut out, hipStream_t st) {
  if (w.G == 0 || w.item == 0) return hipErrorInvalidValue;
  const dim3 gg((w.G + 256) / 256), gc((w.count + 255) / 256);  // G + 1 entries; the map
  hipLaunchKernelGGL(k_ru_init, gg, dim3(256), 0, st, w);
  if (w.count) {
    if (ext)
      hipLaunchKernelGGL(k_ru_count<false>, gc, dim3(256), 0, st, w, (const uint8_t*)nullptr);
    else
      hipLaunchKernelGGL(k_ru_count<true>, gc, dim3(256), 0, st, w, (const uint8_t*)state.dirty);
  }
  hipLaunchKernelGGL(k_ru_items, gg, dim3(256), 0, st, w);
  hipError_t e = merge_offsets(w.cnt, w.G + 1, w.moff, w.tmp, w.tmp_bytes, st);
  if (e != hipSuccess) return e;
  e = merge_offsets(w.nitems, w.G + 1, w.ioff, w.tmp, w.tmp_bytes, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_ru_plan, gg, dim3(256), 0, st, w);
  if (w.count) {
    if (ext)
      hipLaunchKernelGGL(k_ru_fill<false>, gc, dim3(256), 0, st, w, (const uint8_t*)nullptr);
    else
      hipLaunchKernelGGL(k_ru_fill<true>, gc, dim3(256), 0, st, w, (const uint8_t*)state.dirty);
  }
  // (upper bounds of the item and group counts: the kernels read the exact ones on the device)
  const uint32_t items = (uint32_t)std::min<size_t>(w.caps.items, (size_t)w.count / w.item + (size_t)w.G + 1);
  if (ext)
    hipLaunchKernelGGL(k_ru_accum<ExtRows>, dim3(items), dim3(64), 0, st, w, ExtRows{ext, ext_total}, tb, out);
  else
    hipLaunchKernelGGL(k_ru_accum<LiveRows>, dim3(items), dim3(64), 0, st, w,
                       LiveRows{state.counts, state.total, state.sumfix, w.first}, tb, out);
  if (w.caps.multi)
    hipLaunchKernelGGL(k_ru_finish, dim3((uint32_t)w.caps.multi), dim3(64 * RU_FIN_WAVES), 0, st, w, tb, out);
  return hipGetLastError();
}

}  // namespace l5dh
