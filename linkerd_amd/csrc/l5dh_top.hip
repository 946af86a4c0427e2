// l5dh_top.hip -- exact top-k series by a summary field or a quantile (l5dh_top,
// l5dh_top_summaries): a deterministic tournament, no atomics.
//
//   k_top_build   one workgroup (512 threads) per chunk of TOP_CHUNK rows.  Each thread reads
//                 its rows' count and key field (8 B each at the rows' 88-B stride; BY_QUANTILE:
//                 the contiguous int64 array), forms the item {key, id, valid} -- the key as an
//                 order-preserving u64, complemented for SMALLEST -- and the workgroup sorts the
//                 chunk in LDS with a bitonic network over the lexicographic compare (valid
//                 first, key descending, id ascending).  The first kp items (kp: the power of
//                 two >= k) go to the level's list buffer; rows that are no candidates, and the
//                 slots past the last row, carry valid = 0 and sink.
//   k_top_merge   a workgroup loads TOP_CHUNK / kp lists of kp items, sorts them the same way
//                 (from the stage that merges pairs of sorted lists on) and writes the first kp.  The host repeats it until one list remains; the
//                 level sizes are known there.
//   k_top_gather  lane j < min(k, candidates) copies winner j's id, its whole summary and its
//                 quantile value; the lane at the end of the valid run writes that minimum.
//
// Equal keys are told apart by the id, so the compare is a total order of distinct items:
// the network's result is one fixed permutation whatever the launch geometry.
#include <utility>

#include "l5dh_top.hpp"

namespace l5dh {
namespace {

// The LDS of k_top_build and k_top_merge: the items being sorted.
struct TopSortLds {
  TopItem item[TOP_CHUNK];
  static constexpr size_t bytes = (size_t)TOP_CHUNK * sizeof(TopItem);
};
static_assert(sizeof(TopSortLds) == TopSortLds::bytes, "no padding");
static_assert(TopSortLds::bytes == 64 * 1024, "two sorting workgroups fit a CU's 160 KB");
static_assert((TOP_CHUNK & (TOP_CHUNK - 1)) == 0 && TOP_CHUNK % (2 * TOP_THREADS) == 0, "whole pairs per thread");
static_assert(TOP_LIMIT <= TOP_CHUNK / 2 && (TOP_LIMIT & (TOP_LIMIT - 1)) == 0, "a merge takes >= 2 lists");

constexpr uint32_t TOP_ITEMS_PER_THREAD = TOP_CHUNK / TOP_THREADS;        // 8
constexpr uint32_t TOP_PAIRS_PER_THREAD = TOP_CHUNK / (2 * TOP_THREADS);  // 4

// a sorts before b: valid first, then key descending, then id ascending.
__device__ __forceinline__ bool top_before(const TopItem& a, const TopItem& b) {
  if (a.valid != b.valid) return a.valid > b.valid;
  if (a.key != b.key) return a.key > b.key;
  return a.id < b.id;
}

__device__ __forceinline__ TopItem top_invalid() { return TopItem{0ull, 0xFFFFFFFFu, 0u}; }

// Bitonic sort of lds.item[0 .. TOP_CHUNK), best first.  Whole workgroup of TOP_THREADS; the
// items are in place and visible (the caller's barrier), and sorted and visible on return.
// first_size: the network's first stage -- 2 for unsorted items; 2 m when every run of m
// items (m a power of two) is sorted already, best first in the even runs and worst first in
// the odd ones, which is the state the network itself is in when it reaches that stage.
__device__ __forceinline__ void top_sort(TopSortLds& lds, uint32_t first_size) {
  for (uint32_t size = first_size; size <= TOP_CHUNK; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
      for (uint32_t t = 0; t < TOP_PAIRS_PER_THREAD; ++t) {
        const uint32_t p = threadIdx.x + t * TOP_THREADS;       // pair index < TOP_CHUNK / 2
        const uint32_t i = 2 * p - (p & (stride - 1));          // the pair's lower slot
        const uint32_t j = i + stride;                          // < TOP_CHUNK
        const bool best_first = (i & size) == 0;                // (size == TOP_CHUNK: always)
        const TopItem a = lds.item[i], b = lds.item[j];
        if (top_before(b, a) == best_first) {
          lds.item[i] = b;
          lds.item[j] = a;
        }
      }
      __syncthreads();
    }
  }
}

// The first kp sorted items to list `w` of the level's buffer.
__device__ __forceinline__ void top_emit(const TopSortLds& lds, TopItem* __restrict__ out, uint32_t kp) {
  TopItem* dst = out + (size_t)blockIdx.x * kp;
  for (uint32_t s = threadIdx.x; s < kp; s += TOP_THREADS) dst[s] = lds.item[s];
}

// The order-preserving u64 image of a key: signed int64 (fields 0..9, quantile values), or
// the IEEE total order of a double's bits (avg): -NaN < -Inf < ... < -0.0 < +0.0 < ... < +NaN.
__device__ __forceinline__ uint64_t top_ordered(uint64_t bits, bool is_double) {
  const uint64_t sign = 1ull << 63;
  return (is_double && (bits & sign)) ? ~bits : bits ^ sign;
}

__global__ __launch_bounds__(TOP_THREADS) void k_top_build(const uint64_t* __restrict__ summ /* [n][11] */,
                                                           const int64_t* __restrict__ qv,
                                                           const uint32_t* __restrict__ group, uint32_t g, uint32_t n,
                                                           uint32_t first, uint32_t by, uint32_t smallest,
                                                           int64_t min_count, uint32_t kp, TopItem* __restrict__ out) {
  __shared__ TopSortLds lds;
  const uint32_t base = blockIdx.x * TOP_CHUNK;
  const bool is_double = by == TOP_BY_FIELDS - 1;
#pragma unroll
  for (uint32_t t = 0; t < TOP_ITEMS_PER_THREAD; ++t) {
    const uint32_t s = threadIdx.x + t * TOP_THREADS;
    const uint32_t i = base + s;  // (< 2^24 + TOP_CHUNK)
    TopItem it = top_invalid();
    if (i < n) {
      const uint64_t* row = summ + (size_t)i * TOP_BY_FIELDS;
      const int64_t cnt = (int64_t)row[0];
      const uint64_t bits = by == TOP_BY_QUANTILE ? (uint64_t)qv[i] : row[by];
      const bool member = group == nullptr || group[i] == g;
      if (cnt >= min_count && member) {
        const uint64_t key = top_ordered(bits, is_double);
        it = TopItem{smallest ? ~key : key, first + i, 1u};
      }
    }
    lds.item[s] = it;
  }
  __syncthreads();
  top_sort(lds, 2u);
  top_emit(lds, out, kp);
}

// lists: the `nlists` lists of the level below, kp items each; this workgroup takes lists
// [blockIdx.x * fanin, + fanin) of them (fanin * kp == TOP_CHUNK; the slots of lists past
// the last one are filled with invalid items).  Every list is sorted, so the odd ones are
// loaded back to front and the network starts at the stage that merges pairs of lists.
__global__ __launch_bounds__(TOP_THREADS) void k_top_merge(const TopItem* __restrict__ lists, uint32_t nlists,
                                                           uint32_t kp, uint32_t kp_shift, TopItem* __restrict__ out) {
  __shared__ TopSortLds lds;
  const uint32_t fanin = TOP_CHUNK >> kp_shift;
  const uint32_t l0 = blockIdx.x * fanin;
#pragma unroll
  for (uint32_t t = 0; t < TOP_ITEMS_PER_THREAD; ++t) {
    const uint32_t s = threadIdx.x + t * TOP_THREADS;
    const uint32_t l = l0 + (s >> kp_shift);
    TopItem it = top_invalid();
    const uint32_t w = s & (kp - 1);
    if (l < nlists) it = lists[(size_t)l * kp + ((l & 1u) ? kp - 1 - w : w)];  // (l0 is even: l's parity is the slot's)
    lds.item[s] = it;
  }
  __syncthreads();
  top_sort(lds, 2u * kp);
  top_emit(lds, out, kp);
}

// list: the final kp >= k items, best first.  One workgroup of TOP_LIMIT threads.
__global__ __launch_bounds__(TOP_LIMIT) void k_top_gather(const TopItem* __restrict__ list, uint32_t k, uint32_t first,
                                                          const uint64_t* __restrict__ summ, const int64_t* __restrict__ qv,
                                                          uint32_t* __restrict__ ids_out, uint64_t* __restrict__ top_out,
                                                          int64_t* __restrict__ q_out, uint32_t* __restrict__ n_out,
                                                          uint32_t* __restrict__ n_out2) {
  const uint32_t j = threadIdx.x;
  if (j >= k) return;
  const TopItem it = list[j];
  if (!it.valid) {
    if (j == 0) {  // no candidate at all
      *n_out = 0u;
      if (n_out2) *n_out2 = 0u;
    }
    return;
  }
  // the valid items are a prefix: the last of them (within k) knows the count
  if (j + 1 == k || !list[j + 1].valid) {
    *n_out = j + 1;
    if (n_out2) *n_out2 = j + 1;
  }
  const uint32_t i = it.id - first;  // the winner's row
  ids_out[j] = it.id;
  if (top_out) {
    const uint64_t* src = summ + (size_t)i * TOP_BY_FIELDS;
    uint64_t* dst = top_out + (size_t)j * TOP_BY_FIELDS;
#pragma unroll
    for (uint32_t f = 0; f < TOP_BY_FIELDS; ++f) dst[f] = src[f];
  }
  if (q_out) q_out[j] = qv[i];
}

}  // namespace

hipError_t launch_top(const TopArgs& a, hipStream_t st) {
  if (a.n == 0 || a.n > TOP_MAX_ROWS || a.k < 1 || a.k > TOP_LIMIT || a.by > TOP_BY_QUANTILE || !a.summ ||
      (a.by == TOP_BY_QUANTILE && !a.qv) || (a.q_out && !a.qv) || !a.list_a || !a.list_b || !a.ids_out || !a.n_out ||
      a.min_count < 0 || (uint64_t)a.first + a.n > ((uint64_t)1 << 32))
    return hipErrorInvalidValue;
  const uint32_t kp = top_kp(a.k);
  uint32_t kp_shift = 0;
  while ((1u << kp_shift) < kp) ++kp_shift;
  size_t lists = top_chunks(a.n);
  const uint64_t* summ = reinterpret_cast<const uint64_t*>(a.summ);
  hipLaunchKernelGGL(k_top_build, dim3((uint32_t)lists), dim3(TOP_THREADS), 0, st, summ, a.qv, a.group, a.g, a.n, a.first,
                     a.by, a.smallest, a.min_count, kp, a.list_a);
  TopItem* cur = a.list_a;
  TopItem* nxt = a.list_b;
  while (lists > 1) {
    const size_t up = top_next(lists, kp);
    hipLaunchKernelGGL(k_top_merge, dim3((uint32_t)up), dim3(TOP_THREADS), 0, st, cur, (uint32_t)lists, kp, kp_shift, nxt);
    std::swap(cur, nxt);
    lists = up;
  }
  hipLaunchKernelGGL(k_top_gather, dim3(1), dim3(TOP_LIMIT), 0, st, cur, a.k, a.first, summ, a.qv, a.ids_out,
                     reinterpret_cast<uint64_t*>(a.top_out), a.q_out, a.n_out, a.n_out2);
  return hipGetLastError();
}

}  // namespace l5dh
