// l5dh_window.hip -- the sliding window's sum (l5dh_window_query): per series, the rows of
// the last W ended intervals added up, and what one Stat fed all their samples would report.
//
// A slot of the ring holds one ended interval as the sparse export wrote it: row_off
// [count + 1], 8-byte entries {bucket, count} in ascending bucket order per row, totals
// [count].  The histogram of a union of intervals is the element-wise integer sum of their
// rows, so the window of a series is a sum of at most 64 short entry lists into one dense row.
//
//   k_win_sum   k_mdecode's shape over CSR entries: persistent waves take one series at a
//               time, each of a workgroup's four waves owns a 1800-word u32 LDS row (28.8 KB
//               per workgroup, no barriers).  Lane s holds slot s's descriptor (loaded once
//               from the kernel arguments) and loads that slot's row_off[r], row_off[r + 1]
//               and totals[r] -- the next series' while this one is summed.  A slot counts
//               only if it was pushed after born[r] and covers r.  The first 64 entries of
//               WIN_BATCH slots are loaded together (one coalesced 8-byte load per lane),
//               longer rows four chunks at a time.  A lane adds its entry's count to
//               row[bucket] with an LDS add: within one slot's row the buckets are distinct
//               and the slots go one after another through the wave, so the add's return
//               value is the exact partial sum -- old + count > 2^31 - 1 lowers the status
//               word to the least such series, and no u32 wraps before that.  With
//               include_open the lane adds its own bins of the live row of a dirty tile.
//               Then the dense row, the total, the summary; the row is cleared for the next
//               series.
//   k_win_born  born[first .. first + count) = seq (l5dh_window_forget).
#include <algorithm>

#include "l5dh_lanerow.hpp"
#include "l5dh_window.hpp"

namespace l5dh {
namespace {

constexpr uint32_t CMAX = (uint32_t)INT_MAXV;  // 2^31 - 1: the largest count of an int32 row
constexpr int WIN_WAVES = 4, WIN_BATCH = 8, WIN_GRID = 1280;  // (5 workgroups per CU: 28.8 KB of LDS each)
static_assert(WIN_MAX == 64 && WIN_MAX % WIN_BATCH == 0, "a slot per lane, whole batches");

__device__ __forceinline__ uint2 load_entry(const BucketEntry* __restrict__ p, uint64_t i) {
  return *reinterpret_cast<const uint2*>(p + i);
}

__global__ __launch_bounds__(64 * WIN_WAVES) void k_win_sum(WinSlots ws, const uint64_t* __restrict__ born, State st,
                                                            uint32_t first, uint32_t count, int include_open,
                                                            Tables tb, int32_t* __restrict__ out_rows,
                                                            int64_t* __restrict__ out_totals,
                                                            Summary88* __restrict__ out_summ,
                                                            uint32_t* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) uint32_t lrow[WIN_WAVES][ROW];
  const int w = threadIdx.x >> 6;
  const int lane = lane_id();
  // persistent waves: rows i, i + GW, ... of the range (no barriers: a wave owns its LDS row)
  const uint32_t GW = gridDim.x * WIN_WAVES;
  uint32_t i = blockIdx.x * WIN_WAVES + w;
  uint32_t* row = lrow[w];
  for (int b = lane; b < ROW / 4; b += 64) reinterpret_cast<uint4*>(row)[b] = make_uint4(0u, 0u, 0u, 0u);
  // lane s: slot s's descriptor (slots >= ws.n: count 0, nothing of them is ever read)
  const uint64_t* __restrict__ my_off = ws.row_off[lane];
  const int64_t* __restrict__ my_tot = ws.totals[lane];
  const uint64_t my_ent = (uint64_t)(uintptr_t)ws.entries[lane];
  const uint64_t my_seq = ws.seq[lane];
  const uint32_t my_cnt = ws.count[lane];
  const int nslots = (int)ws.n;
  // lane s: the entries of series first + ii in slot s, and the row's exact sum there
  auto meta = [&](uint32_t ii, uint32_t& n, uint64_t& o, uint64_t& t) {
    const uint32_t r = first + (ii < count ? ii : 0u);
    const bool ok = ii < count && r < my_cnt && my_seq > born[r];
    const uint64_t a = ok ? my_off[r] : 0ull, b = ok ? my_off[r + 1] : 0ull;
    t = ok ? (uint64_t)my_tot[r] : 0ull;
    o = a;
    n = min((uint32_t)(b - a), (uint32_t)NB);  // (a row holds each bucket once)
  };
  bool over = false;
  auto add = [&](uint2 e, bool valid) {
    if (valid && e.x < (uint32_t)NB) {
      const uint32_t old = atomicAdd(&row[e.x], e.y);  // (an LDS add; its return value: the partial sum)
      over |= (uint64_t)old + e.y > CMAX;
    }
  };
  // one slot's row: its first chunk comes loaded, the others four at a time
  auto add_row = [&](uint2 x0, uint32_t n, const BucketEntry* __restrict__ p) {
    add(x0, (uint32_t)lane < n);
    for (uint32_t base = 64; base < n; base += 256) {
      const uint32_t k = base + (uint32_t)lane;
      const uint2 z = make_uint2(0u, 0u);
      const uint2 a0 = k < n ? load_entry(p, k) : z;
      const uint2 a1 = k + 64u < n ? load_entry(p, k + 64u) : z;
      const uint2 a2 = k + 128u < n ? load_entry(p, k + 128u) : z;
      const uint2 a3 = k + 192u < n ? load_entry(p, k + 192u) : z;
      add(a0, k < n);
      add(a1, k + 64u < n);
      add(a2, k + 128u < n);
      add(a3, k + 192u < n);
    }
  };
  uint32_t nl;
  uint64_t ol, tl;
  meta(i, nl, ol, tl);
  for (; i < count; i += GW) {
    const uint32_t r = first + i;
    const uint32_t cn = nl;
    const uint64_t co = ol;
    uint64_t total = wave_sum(tl);  // (an int64 that wraps like a Java long)
    meta(i + GW, nl, ol, tl);
    over = false;
    for (int s0 = 0; s0 < nslots; s0 += WIN_BATCH) {  // (s0 <= 56: every lane index below is < 64)
      uint2 xs[WIN_BATCH];
      uint32_t ns[WIN_BATCH];
      const BucketEntry* ps[WIN_BATCH];
#pragma unroll
      for (int k = 0; k < WIN_BATCH; ++k) {
        ns[k] = (uint32_t)__builtin_amdgcn_readlane((int)cn, s0 + k);
        ps[k] = reinterpret_cast<const BucketEntry*>((uintptr_t)readlane64(my_ent, s0 + k)) + readlane64(co, s0 + k);
        xs[k] = (uint32_t)lane < ns[k] ? load_entry(ps[k], (uint64_t)lane) : make_uint2(0u, 0u);
      }
#pragma unroll
      for (int k = 0; k < WIN_BATCH; ++k) add_row(xs[k], ns[k], ps[k]);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (include_open && st.dirty[r >> TILE_SHIFT] != 0) {  // (wave-uniform; a clean tile's row is never read)
      const LiveRows live{st.counts, st.total, st.sumfix, 0u};
      uint4 v[9];
      lane_row_load(live.row(r), v);
      total += live.sum(r);
      const int ng = lane_groups(lane);
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        if (q < ng) {  // the lane's own bins: plain LDS read, add, write
          uint4* p = reinterpret_cast<uint4*>(row + 28 * lane + 4 * q);
          const uint4 a = *p;
          over |= (uint64_t)a.x + v[q].x > CMAX || (uint64_t)a.y + v[q].y > CMAX ||
                  (uint64_t)a.z + v[q].z > CMAX || (uint64_t)a.w + v[q].w > CMAX;
          *p = make_uint4(a.x + v[q].x, a.y + v[q].y, a.z + v[q].z, a.w + v[q].w);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    if (__ballot(over) != 0ull && lane == 0) atomicMin(status, r);
    const SrcLds32 lds{row};
    if (out_rows) {
      int32_t* orow = out_rows + (size_t)i * NB;
      for (int q = lane; q < NB4; q += 64) store4_1798(orow, 4 * q, lds.get4(4 * q));
    }
    if (out_totals && lane == 0) out_totals[i] = (int64_t)total;
    WideSums g;  // (four summed buckets of a group can reach 2^32 and more)
    g.clear();
    const int ng = lane_groups(lane);
#pragma unroll
    for (int q = 0; q < 9; ++q)
      if (q < ng) g.set(q, lds.get4(28 * lane + 4 * q));
    wave_summary(g, lds, (int64_t)total, tb.mid, out_summ ? out_summ + i : nullptr);
    // cleared for the next row (this wave's LDS operations stay in order: the reads come first)
    for (int b = lane; b < ROW / 4; b += 64) reinterpret_cast<uint4*>(row)[b] = make_uint4(0u, 0u, 0u, 0u);
  }
}

__global__ __launch_bounds__(256) void k_win_born(uint64_t* __restrict__ born, uint32_t first, uint32_t count,
                                                  uint64_t seq) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k < count) born[first + k] = seq;
}

}  // namespace

hipError_t launch_win_sum(const WinSlots& slots, const uint64_t* born, State state, uint32_t first, uint32_t count,
                          int include_open, Tables tb, int32_t* out_rows, int64_t* out_totals, Summary88* out_summ,
                          uint32_t* status, hipStream_t st) {
  if (slots.n > (uint32_t)WIN_MAX || !born || !status || (uint64_t)first + count > state.S) return hipErrorInvalidValue;
  for (uint32_t k = 0; k < slots.n; ++k)  // (a slot never covers more series than born[] holds)
    if (slots.count[k] > state.S || (slots.count[k] && (!slots.row_off[k] || !slots.totals[k])))
      return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  const uint32_t grid = std::min<uint32_t>((count + WIN_WAVES - 1) / WIN_WAVES, (uint32_t)WIN_GRID);
  hipLaunchKernelGGL(k_win_sum, dim3(grid), dim3(64 * WIN_WAVES), 0, st, slots, born, state, first, count, include_open,
                     tb, out_rows, out_totals, out_summ, status);
  return hipGetLastError();
}

hipError_t launch_win_born(uint64_t* born, uint32_t first, uint32_t count, uint64_t seq, hipStream_t st) {
  if (!born) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_win_born, dim3((count + 255) / 256), dim3(256), 0, st, born, first, count, seq);
  return hipGetLastError();
}

}  // namespace l5dh
