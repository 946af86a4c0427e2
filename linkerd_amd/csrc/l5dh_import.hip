// l5dh_import.hip -- state import and the public sparse export (l5dh_import_state,
// l5dh_import_sparse, l5dh_export_sparse).
//
// The way into the bucket rows.  An import makes the target series report what they would
// had they also received the samples behind the imported rows: counts[b] += row[b], the
// exact sum += the row's total (an int64 that wraps like a Java long).  Nothing else moves:
// sumfix, the staging ring and the pending segments keep what they hold, and the next
// snapshot sums them onto the rows as it always does (its plan reads dirty[] then).
//
// The clean-tile rule.  The state rows and total[] of a tile are live only while dirty[tile]
// is set; a clean tile's hold stale values that nothing reads.  An import that touches a
// clean tile therefore leaves all its 32 rows valid -- imported rows stored (not added),
// every other row and total zeroed -- and sets dirty[tile] in a LATER launch, because the
// other waves of the tile read the flag to decide between storing and adding.
//
//   k_imp_dense     one wave per series of the range widened to tile boundaries; lane l owns
//                   bins 28 l .. 28 l + 27 (lane 63 also 1792..1797), the external row's and
//                   (dirty tile) the state row's 16-B groups all in flight together; add,
//                   compare in 64 bits, store.  A row of a clean tile is written once.
//   k_imp_check     sparse rows, read only: a wave per row over its offsets, id and entries.
//   k_imp_touch     a thread per row lists the clean tiles the rows touch (each once).
//   k_imp_zero      a wave per series of the listed tiles: zero row, zero total.
//   k_imp_sparse    a wave per row, a lane per entry: read-add-write of the entry's bucket.
//   k_imp_mark_*    dirty[tile] = 1 for the touched tiles.
//   k_exp_count /   a wave per row: the lanes' non-zero bins, summed (count) or scanned
//   k_exp_write     (write: each lane's entries in ascending bucket order, 8-B stores).
//
// Errors without a second read in the good case: both addends of a valid import are at most
// 2^31 - 1, so the u32 sum never wraps; the one pass adds, compares the 64-bit sum with
// 2^31 - 1 and lowers a status word to the least offending series (atomicMin).  On that
// status the host runs the undo kernel: the modular subtraction of the same rows, exact
// whatever the counts were.  A tile the failed call dirtied keeps zero rows and zero totals,
// which reads exactly as a clean tile does.
#include <algorithm>

#include "l5dh_lanerow.hpp"
#include "l5dh_import.hpp"

namespace l5dh {
namespace {

constexpr uint32_t CMAX = (uint32_t)INT_MAXV;  // 2^31 - 1: the largest count of an int32 row

// The lane's groups to a state row (lane 63: also groups 7 and 8, the padding bins zero).
__device__ __forceinline__ void store_state(uint32_t* __restrict__ row, const uint4 (&v)[9]) {
  const int lane = lane_id();
#pragma unroll
  for (int q = 0; q < 7; ++q) store4_state(row, 28 * lane + 4 * q, v[q]);
  if (lane == 63) {
    store4_state(row, 1792, v[7]);
    store4_state(row, 1796, make_uint4(v[8].x, v[8].y, 0u, 0u));
  }
}

__device__ __forceinline__ uint32_t max4(uint4 v) { return max(max(v.x, v.y), max(v.z, v.w)); }
__device__ __forceinline__ uint4 add4(uint4 a, uint4 b) { return make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ uint4 sub4(uint4 a, uint4 b) { return make_uint4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
// a component of a + b (in 64 bits) above 2^31 - 1
__device__ __forceinline__ bool over4(uint4 a, uint4 b) {
  return (uint64_t)a.x + b.x > CMAX || (uint64_t)a.y + b.y > CMAX || (uint64_t)a.z + b.z > CMAX ||
         (uint64_t)a.w + b.w > CMAX;
}
// A wave's finding: one atomicMin of the wave's key when any lane has it.
__device__ __forceinline__ void report(bool found, uint32_t* word, uint32_t key) {
  if (__ballot(found) != 0ull && lane_id() == 0) atomicMin(word, key);
}

// Series lo + w of the widened range [lo, lo + nser); in: the series is in [first, first + count).
template <bool UNDO>
__global__ __launch_bounds__(256) void k_imp_dense(State st, uint32_t first, uint32_t count, uint32_t lo, uint32_t nser,
                                                   const int32_t* __restrict__ ext,
                                                   const int64_t* __restrict__ ext_total, uint32_t* __restrict__ status) {
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= nser) return;  // (whole waves)
  const uint32_t s = lo + w;
  const int lane = lane_id();
  const bool in = s - first < count;  // (unsigned: s < first wraps)
  uint32_t* __restrict__ row = st.counts + (size_t)s * ROW;
  // (the undo runs after the range's tiles were marked: every one is dirty)
  const bool dirty = UNDO || st.dirty[s >> TILE_SHIFT] != 0;  // (wave-uniform)
  if (!in) {
    if (!dirty) {  // the tile's other rows: valid zeros
      uint4 z[9];
#pragma unroll
      for (int q = 0; q < 9; ++q) z[q] = make_uint4(0u, 0u, 0u, 0u);
      store_state(row, z);
      if (lane == 0) st.total[s] = 0;
    }
    return;
  }
  const size_t i = s - first;
  uint4 v[9], a[9];
  lane_row_load(SrcExt{ext + i * NB}, v);
  const uint64_t t = ext_total ? (uint64_t)ext_total[i] : 0ull;
  if (dirty) {
    lane_row_load(SrcRow32{row}, a);
  } else {
#pragma unroll
    for (int q = 0; q < 9; ++q) a[q] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (UNDO) {
#pragma unroll
    for (int q = 0; q < 9; ++q) a[q] = sub4(a[q], v[q]);
    store_state(row, a);
    if (lane == 0) st.total[s] = (int64_t)((uint64_t)st.total[s] - t);
    return;
  }
  bool bad = false, over = false;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    bad |= max4(v[q]) > CMAX;
    over |= over4(a[q], v[q]);
    a[q] = add4(a[q], v[q]);
  }
  store_state(row, a);
  if (lane == 0) st.total[s] = (int64_t)((dirty ? (uint64_t)st.total[s] : 0ull) + t);
  report(bad, status + IS_BAD, s);
  report(over && !bad, status + IS_RANGE, s);
}

__global__ __launch_bounds__(256) void k_imp_mark_range(uint8_t* __restrict__ dirty, uint32_t t0, uint32_t nt) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k < nt) dirty[t0 + k] = 1;
}

__device__ __forceinline__ uint32_t row_series(const SparseRows& r, uint32_t i) {
  return r.series ? r.series[i] : r.first + i;
}

__global__ __launch_bounds__(256) void k_imp_check(SparseRows r, uint32_t S, uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= r.n) return;  // (whole waves)
  const int lane = lane_id();
  bool bad = false;
  if (r.series) {
    const uint32_t s = r.series[i];
    bad = s >= S || (i > 0 && r.series[i - 1] >= s);
  }
  const uint64_t a = r.row_off[i], b = r.row_off[i + 1];
  if ((i == 0 && a != 0ull) || a > b || b > r.n_entries || b - a > (uint64_t)NB) {
    bad = true;  // (none of the row's entries is read)
  } else if (r.entries) {
    for (uint64_t k = a + lane; k < b; k += 64) {
      const BucketEntry e = r.entries[k];
      bad |= e.bucket >= (uint32_t)NB || e.count > CMAX;
      if (k > a) bad |= r.entries[k - 1].bucket >= e.bucket;
    }
  }
  report(bad, status + IS_BAD, i);
}

__global__ __launch_bounds__(256) void k_imp_touch(SparseRows r, const uint8_t* __restrict__ dirty,
                                                   uint32_t* __restrict__ tflag, uint32_t* __restrict__ list,
                                                   uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= r.n) return;
  const uint32_t t = row_series(r, i) >> TILE_SHIFT;
  if (dirty[t] == 0 && atomicExch(tflag + t, 1u) == 0u) list[atomicAdd(status + IS_NCLEAN, 1u)] = t;
}

// Eight workgroups (32 waves) per listed tile; launched for an upper bound of the list.
__global__ __launch_bounds__(256) void k_imp_zero(State st, const uint32_t* __restrict__ list,
                                                  const uint32_t* __restrict__ status) {
  const uint32_t j = blockIdx.x >> 3;
  if (j >= status[IS_NCLEAN]) return;
  const uint32_t s = list[j] * TILE + (blockIdx.x & 7u) * 4 + (threadIdx.x >> 6);
  if (s >= st.S) return;  // (whole waves)
  uint4 z[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) z[q] = make_uint4(0u, 0u, 0u, 0u);
  store_state(st.counts + (size_t)s * ROW, z);
  if (lane_id() == 0) st.total[s] = 0;
}

template <bool UNDO>
__global__ __launch_bounds__(256) void k_imp_sparse(State st, SparseRows r, uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= r.n) return;  // (whole waves)
  const int lane = lane_id();
  const uint32_t s = row_series(r, i);
  uint32_t* __restrict__ row = st.counts + (size_t)s * ROW;
  const uint64_t a = r.row_off[i], b = r.row_off[i + 1];
  bool over = false;
  for (uint64_t k = a + lane; k < b; k += 64) {  // (checked: b - a <= 1798, buckets < 1798 and distinct)
    const BucketEntry e = r.entries[k];
    const uint32_t old = row[e.bucket];
    over |= (uint64_t)old + e.count > CMAX;
    row[e.bucket] = UNDO ? old - e.count : old + e.count;
  }
  if (lane == 0 && r.totals) {
    const uint64_t t = (uint64_t)r.totals[i];
    st.total[s] = (int64_t)(UNDO ? (uint64_t)st.total[s] - t : (uint64_t)st.total[s] + t);
  }
  if (!UNDO) report(over, status + IS_RANGE, s);
}

__global__ __launch_bounds__(256) void k_imp_mark_rows(SparseRows r, uint8_t* __restrict__ dirty) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < r.n) dirty[row_series(r, i) >> TILE_SHIFT] = 1;
}

__device__ __forceinline__ uint32_t nz4(uint4 v) { return (v.x != 0u) + (v.y != 0u) + (v.z != 0u) + (v.w != 0u); }
__device__ __forceinline__ uint32_t nz_lane(const uint4 (&v)[9]) {
  uint32_t c = 0;
#pragma unroll
  for (int q = 0; q < 9; ++q) c += nz4(v[q]);  // (groups the lane does not own: zeros)
  return c;
}

__global__ __launch_bounds__(256) void k_exp_count(State st, uint32_t first, uint32_t count,
                                                   uint32_t* __restrict__ rowcnt) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= count) return;  // (whole waves)
  const uint32_t s = first + i;
  uint32_t c = 0;
  if (st.dirty[s >> TILE_SHIFT] != 0) {  // (wave-uniform; a clean tile's rows are never read)
    uint4 v[9];
    lane_row_load(SrcRow32{st.counts + (size_t)s * ROW}, v);
    c = (uint32_t)wave_sum((uint64_t)nz_lane(v));
  }
  if (lane_id() == 0) rowcnt[i] = c;
}

__device__ __forceinline__ void put_entry(BucketEntry* __restrict__ entries, uint64_t& at, uint32_t bucket, uint32_t c) {
  if (c != 0u) {
    *reinterpret_cast<uint2*>(entries + at) = make_uint2(bucket, c);
    ++at;
  }
}

__global__ __launch_bounds__(256) void k_exp_write(State st, uint32_t first, uint32_t count,
                                                   const uint64_t* __restrict__ offs, BucketEntry* __restrict__ entries,
                                                   int64_t* __restrict__ totals) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= count) return;  // (whole waves)
  const uint32_t s = first + i;
  const int lane = lane_id();
  if (st.dirty[s >> TILE_SHIFT] == 0) {  // (wave-uniform)
    if (totals && lane == 0) totals[i] = 0;
    return;
  }
  uint4 v[9];
  lane_row_load(SrcRow32{st.counts + (size_t)s * ROW}, v);
  // (+ sumfix as in k_rows: a one-tile space's fold leaves its escaped samples' sums there)
  if (totals && lane == 0) totals[i] = (int64_t)((uint64_t)st.total[s] + (uint64_t)st.sumfix[s]);
  const uint32_t c = nz_lane(v);
  uint64_t at = offs[i] + (wave_incl_scan32(c) - c);
  // the lane's bins in ascending order (lane 63: groups 7 and 8 are bins 1792..1797)
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const uint32_t b0 = 28u * lane + 4u * q;
    put_entry(entries, at, b0, v[q].x);
    put_entry(entries, at, b0 + 1, v[q].y);
    put_entry(entries, at, b0 + 2, v[q].z);
    put_entry(entries, at, b0 + 3, v[q].w);
  }
}

inline dim3 threads256(uint32_t n) { return dim3(n / 256 + (n % 256 != 0)); }

template <bool UNDO>
hipError_t launch_dense(State state, uint32_t first, uint32_t count, const int32_t* ext, const int64_t* ext_total,
                        uint32_t* status, hipStream_t st) {
  if (!ext || (uint64_t)first + count > state.S) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  // the undo touches the imported rows only; the import widens the range to whole tiles
  const uint32_t lo = UNDO ? first : first & ~(uint32_t)(TILE - 1);
  const uint32_t end = first + count;
  const uint32_t hi = UNDO ? end : (uint32_t)std::min<uint64_t>(state.S, ((uint64_t)end + TILE - 1) & ~(uint64_t)(TILE - 1));
  hipLaunchKernelGGL(k_imp_dense<UNDO>, waves4(hi - lo), dim3(256), 0, st, state, first, count, lo, hi - lo, ext,
                     ext_total, status);
  if (!UNDO) {
    const uint32_t t0 = first >> TILE_SHIFT, nt = ((end - 1) >> TILE_SHIFT) - t0 + 1;
    hipLaunchKernelGGL(k_imp_mark_range, threads256(nt), dim3(256), 0, st, state.dirty, t0, nt);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t import_status_init(uint32_t* status, hipStream_t st) {
  hipError_t e = hipMemsetAsync(status, 0xFF, 2 * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  return hipMemsetAsync(status + IS_NCLEAN, 0, (IS_WORDS - IS_NCLEAN) * sizeof(uint32_t), st);
}

hipError_t import_dense(State state, uint32_t first, uint32_t count, const int32_t* ext, const int64_t* ext_total,
                        uint32_t* status, hipStream_t st) {
  return launch_dense<false>(state, first, count, ext, ext_total, status, st);
}

hipError_t import_dense_undo(State state, uint32_t first, uint32_t count, const int32_t* ext,
                             const int64_t* ext_total, hipStream_t st) {
  return launch_dense<true>(state, first, count, ext, ext_total, nullptr, st);
}

hipError_t import_sparse_check(SparseRows rows, uint32_t S, uint32_t* status, hipStream_t st) {
  if (!rows.row_off || rows.n > S) return hipErrorInvalidValue;
  if (rows.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_imp_check, waves4(rows.n), dim3(256), 0, st, rows, S, status);
  return hipGetLastError();
}

hipError_t import_sparse(State state, SparseRows rows, uint32_t* tflag, uint32_t* list, uint32_t* status,
                         hipStream_t st) {
  if (!rows.row_off || rows.n > state.S || (rows.n_entries && !rows.entries)) return hipErrorInvalidValue;
  if (rows.n == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(tflag, 0, (size_t)state.F * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_imp_touch, threads256(rows.n), dim3(256), 0, st, rows, (const uint8_t*)state.dirty, tflag, list,
                     status);
  // (n ascending ids touch at most min(n, F) tiles; the kernel reads the list's length)
  hipLaunchKernelGGL(k_imp_zero, dim3(8u * std::min(rows.n, state.F)), dim3(256), 0, st, state, (const uint32_t*)list,
                     (const uint32_t*)status);
  hipLaunchKernelGGL(k_imp_sparse<false>, waves4(rows.n), dim3(256), 0, st, state, rows, status);
  hipLaunchKernelGGL(k_imp_mark_rows, threads256(rows.n), dim3(256), 0, st, rows, state.dirty);
  return hipGetLastError();
}

hipError_t import_sparse_undo(State state, SparseRows rows, hipStream_t st) {
  if (rows.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_imp_sparse<true>, waves4(rows.n), dim3(256), 0, st, state, rows, (uint32_t*)nullptr);
  return hipGetLastError();
}

hipError_t export_sparse_count(State state, uint32_t first, uint32_t count, uint32_t* rowcnt, hipStream_t st) {
  if ((uint64_t)first + count > state.S) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_exp_count, waves4(count), dim3(256), 0, st, state, first, count, rowcnt);
  return hipGetLastError();
}

hipError_t export_sparse_write(State state, uint32_t first, uint32_t count, const uint64_t* offs,
                               BucketEntry* entries, int64_t* totals, hipStream_t st) {
  if ((uint64_t)first + count > state.S) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_exp_write, waves4(count), dim3(256), 0, st, state, first, count, offs, entries, totals);
  return hipGetLastError();
}

}  // namespace l5dh
