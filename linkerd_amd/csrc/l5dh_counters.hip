// l5dh_counters.hip -- the counter space's kernels: k_cnt_add, the batched Metric.Counter.incr
// (values[id] += delta, wrapping like a Java long), and k_cnt_rollup, per-group sums of a
// range of counters.
//
// k_cnt_add.  A skewed id stream must not reach global memory add by add: the hottest id of a
// Zipf load takes percents of a batch, and adds to one address serialize at the memory side.
// Persistent workgroups take contiguous slabs of the batch; each keeps a private claim table
// in LDS (CntLds: tag[C] u32, sum[C] u64).  An id's home slot is id mod C (counter ids are
// dense, so the hot ids of a registry spread over the slots as they are); a slot is claimed
// by a compare-and-swap of its tag, a hit adds with a return-less 64-bit LDS add, and an id
// whose PROBE slots are all taken by others adds with a return-less agent-scope global atomic
// of its own.  At the slab's end every claimed slot with a non-zero sum issues one global
// atomic and the table is cleared.  All sums are two's-complement, so neither the order nor
// the path of an add shows in the result.
#include "l5dh_counters.hpp"

namespace l5dh {

namespace {

// The claim table of one workgroup, in the dynamic LDS.
struct CntLds {
  static constexpr int LOG_C = 13;
  static constexpr uint32_t C = 1u << LOG_C;  // slots (not tuned)
  static constexpr int PROBE = 4;              // slots an id may take: home .. home + PROBE - 1 (mod C)
  static constexpr uint32_t EMPTY = 0xFFFFFFFFu;  // (no valid id: ids are < 2^24)
  static constexpr size_t o_tag = 0;                // u32 [C] the id that owns the slot, or EMPTY
  static constexpr size_t o_sum = o_tag + C * 4;    // u64 [C] the slab's sum of that id's deltas
  static constexpr size_t bytes = o_sum + C * 8;
  static constexpr size_t static_bytes = 4 * 8;     // s_stat
  __device__ static uint32_t* tag(uint32_t* smem) { return smem + o_tag / 4; }
  __device__ static unsigned long long* sum(uint32_t* smem) {
    return reinterpret_cast<unsigned long long*>(smem + o_sum / 4);
  }
};
static_assert(CntLds::o_sum % 8 == 0, "the sums are 8-byte aligned");
static_assert(CntLds::bytes == 96 * 1024, "tag[8192] u32 + sum[8192] u64");
static_assert(CntLds::bytes + CntLds::static_bytes <= 160 * 1024, "fits a CU's LDS");
static_assert(CntLds::C % CNT_NT == 0, "the flush gives every thread the same number of slots");
static_assert(CNT_MAX <= CntLds::EMPTY, "EMPTY is no counter id");

struct CntArgs {
  const uint32_t* ids;
  const int32_t* deltas;  // nullable: 1 each
  size_t n;
  uint32_t head;       // leading elements before ids is 16-byte aligned (< 4, <= n)
  uint32_t dvec;       // deltas + head is 16-byte aligned too
  size_t nvec;         // 4-element vectors after the head
  uint32_t slab_vecs;  // vectors per slab
  uint32_t nslabs;
  int64_t* values;
  uint32_t maxc;
  uint64_t* stats;
};

enum : uint32_t { PATH_DROP = 0, PATH_LDS = 1, PATH_GLOBAL = 2 };  // what became of one add

__device__ __forceinline__ void global_add(int64_t* values, uint32_t id, unsigned long long v) {
  (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(values) + id, v, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}

template <bool TABLE>
__device__ __forceinline__ uint32_t cnt_apply(uint32_t id, int32_t d, const CntArgs& a, uint32_t* tag,
                                              unsigned long long* sum) {
  if (id >= a.maxc) return PATH_DROP;  // never applied, never an address
  const unsigned long long v = (unsigned long long)(long long)d;
  if (TABLE) {
    const uint32_t home = id & (CntLds::C - 1);
#pragma unroll
    for (int p = 0; p < CntLds::PROBE; ++p) {
      const uint32_t slot = (home + p) & (CntLds::C - 1);
      uint32_t owner = __hip_atomic_load(tag + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (owner == CntLds::EMPTY) {
        uint32_t expect = CntLds::EMPTY;
        if (__hip_atomic_compare_exchange_strong(tag + slot, &expect, id, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_WORKGROUP))
          owner = id;
        else
          owner = expect;  // (another wave's claim: possibly of this id)
      }
      if (owner == id) {
        (void)__hip_atomic_fetch_add(sum + slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return PATH_LDS;
      }
    }
  }
  global_add(a.values, id, v);
  return PATH_GLOBAL;
}

// The slab's end: one global atomic per claimed slot with a non-zero sum; the table is empty after.
__device__ __forceinline__ void cnt_flush(const CntArgs& a, uint32_t* tag, unsigned long long* sum) {
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < CntLds::C; s += CNT_NT) {
    const uint32_t owner = tag[s];
    if (owner != CntLds::EMPTY) {
      const unsigned long long v = sum[s];
      if (v) global_add(a.values, owner, v);
      tag[s] = CntLds::EMPTY;
      sum[s] = 0;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ unsigned long long wave_total(unsigned long long x) {
  for (int d = 32; d; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

template <bool TABLE>
__global__ __launch_bounds__(CNT_NT) void k_cnt_add(const CntArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  __shared__ unsigned long long s_stat[4];
  static_assert(sizeof(s_stat) == CntLds::static_bytes, "CntLds counts the static LDS");
  uint32_t* const tag = CntLds::tag(smem);
  unsigned long long* const sum = CntLds::sum(smem);
  const uint32_t tid = threadIdx.x;
  if (tid < 4) s_stat[tid] = 0;
  if (TABLE)
    for (uint32_t s = tid; s < CntLds::C; s += CNT_NT) {
      tag[s] = CntLds::EMPTY;
      sum[s] = 0;
    }
  __syncthreads();
  uint32_t n_path[3] = {0, 0, 0};  // this thread's adds by path
#define CNT_APPLY(id, d) ++n_path[cnt_apply<TABLE>((id), (d), a, tag, sum)]
  if (blockIdx.x == 0) {
    // the element-wise head (before the first aligned vector) and tail (after the last)
    const size_t body_end = (size_t)a.head + a.nvec * 4;
    const uint32_t ntail = (uint32_t)(a.n - body_end);
    if (tid < a.head + ntail) {
      const size_t i = tid < a.head ? tid : body_end + (tid - a.head);
      CNT_APPLY(a.ids[i], a.deltas ? a.deltas[i] : 1);
    }
    if (TABLE) cnt_flush(a, tag, sum);
  }
  const uint4* const iv = reinterpret_cast<const uint4*>(a.ids + a.head);
  const int32_t* const dp = a.deltas ? a.deltas + a.head : nullptr;
  auto load_d = [&](size_t v) -> int4 {
    if (!dp) return make_int4(1, 1, 1, 1);
    if (a.dvec) return reinterpret_cast<const int4*>(dp)[v];
    return make_int4(dp[4 * v], dp[4 * v + 1], dp[4 * v + 2], dp[4 * v + 3]);
  };
  for (uint32_t s = blockIdx.x; s < a.nslabs; s += gridDim.x) {
    const size_t v0 = (size_t)s * a.slab_vecs;
    const size_t v1 = v0 + a.slab_vecs < a.nvec ? v0 + a.slab_vecs : a.nvec;
    size_t v = v0 + tid;
    uint4 id4 = make_uint4(0, 0, 0, 0);
    int4 d4 = make_int4(0, 0, 0, 0);
    if (v < v1) {
      id4 = iv[v];
      d4 = load_d(v);
    }
    while (v < v1) {
      // the next iteration's loads are in flight while this one's adds run
      const size_t vn = v + CNT_NT;
      uint4 idn = id4;
      int4 dn = d4;
      if (vn < v1) {
        idn = iv[vn];
        dn = load_d(vn);
      }
      CNT_APPLY(id4.x, d4.x);
      CNT_APPLY(id4.y, d4.y);
      CNT_APPLY(id4.z, d4.z);
      CNT_APPLY(id4.w, d4.w);
      id4 = idn;
      d4 = dn;
      v = vn;
    }
    if (TABLE) cnt_flush(a, tag, sum);
  }
  // the statistics: one wave-aggregated LDS add per wave, one global add per word per workgroup
#undef CNT_APPLY
  const unsigned long long wl = wave_total(n_path[PATH_LDS]), wg = wave_total(n_path[PATH_GLOBAL]),
                           wd = wave_total(n_path[PATH_DROP]);
  if ((tid & 63) == 0) {
    if (wl) (void)__hip_atomic_fetch_add(&s_stat[CS_LDS], wl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (wg) (void)__hip_atomic_fetch_add(&s_stat[CS_GLOBAL], wg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (wd) (void)__hip_atomic_fetch_add(&s_stat[CS_DROPPED], wd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  if (tid == 0) s_stat[CS_ADDS] = s_stat[CS_LDS] + s_stat[CS_GLOBAL];
  __syncthreads();
  if (tid < CS_WORDS && s_stat[tid])
    (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(a.stats) + tid, s_stat[tid], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
}

// Per-group sums of values[0 .. count).  LDS: partial sums of the workgroup's share, flushed
// with one global atomic per non-zero group (lds_groups = ngroups), or none (lds_groups = 0:
// every member adds to g_out directly).
__global__ __launch_bounds__(CNT_NT) void k_cnt_rollup(const int64_t* values, uint32_t count, const uint32_t* group,
                                                       uint32_t ngroups, uint32_t lds_groups, int64_t* g_out,
                                                       uint32_t* status) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  unsigned long long* const part = reinterpret_cast<unsigned long long*>(smem);  // [lds_groups]
  unsigned long long* const out = reinterpret_cast<unsigned long long*>(g_out);
  const uint32_t tid = threadIdx.x;
  for (uint32_t g = tid; g < lds_groups; g += CNT_NT) part[g] = 0;
  __syncthreads();
  uint32_t bad = 0xFFFFFFFFu;
  for (size_t i = (size_t)blockIdx.x * CNT_NT + tid; i < count; i += (size_t)gridDim.x * CNT_NT) {
    const uint32_t g = group[i];
    if (g < ngroups) {
      const unsigned long long v = (unsigned long long)values[i];
      if (!v) continue;
      if (lds_groups)
        (void)__hip_atomic_fetch_add(part + g, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      else
        (void)__hip_atomic_fetch_add(out + g, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (g != CNT_NO_GROUP) {
      bad = bad < (uint32_t)i ? bad : (uint32_t)i;  // (no group)
    }
  }
  if (bad != 0xFFFFFFFFu) atomicMin(status, bad);
  __syncthreads();
  for (uint32_t g = tid; g < lds_groups; g += CNT_NT) {
    const unsigned long long v = part[g];
    if (v) (void)__hip_atomic_fetch_add(out + g, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace

hipError_t set_counters_attributes() {
  hipError_t e;
  if ((e = hipFuncSetAttribute((const void*)k_cnt_add<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)CntLds::bytes)))
    return e;
  return hipFuncSetAttribute((const void*)k_cnt_rollup, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)(CNT_RU_LDS_GROUPS * 8));
}

hipError_t launch_cnt_add(const uint32_t* ids, const int32_t* deltas, size_t n, int64_t* values, uint32_t max_counters,
                          uint64_t* stats, int max_wg, bool plain, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (max_wg < 1) max_wg = 1;
  CntArgs a{};
  a.ids = ids;
  a.deltas = deltas;
  a.n = n;
  a.head = (uint32_t)(((16 - (uintptr_t)ids % 16) % 16) / 4);
  if (a.head > n) a.head = (uint32_t)n;
  a.dvec = deltas && (uintptr_t)(deltas + a.head) % 16 == 0;
  a.nvec = (n - a.head) / 4;
  // contiguous slabs: n / workgroups elements each, within [CNT_SLAB_MIN, CNT_SLAB_MAX]
  size_t per = (n + (size_t)max_wg - 1) / (size_t)max_wg;
  per = per < CNT_SLAB_MIN ? CNT_SLAB_MIN : per > CNT_SLAB_MAX ? CNT_SLAB_MAX : per;
  a.slab_vecs = (uint32_t)((per + 3) / 4);
  a.nslabs = (uint32_t)((a.nvec + a.slab_vecs - 1) / a.slab_vecs);
  a.values = values;
  a.maxc = max_counters;
  a.stats = stats;
  const uint32_t grid = a.nslabs < (uint32_t)max_wg ? (a.nslabs ? a.nslabs : 1u) : (uint32_t)max_wg;
  if (plain)
    hipLaunchKernelGGL(k_cnt_add<false>, dim3(grid), dim3(CNT_NT), 0, st, a);
  else
    hipLaunchKernelGGL(k_cnt_add<true>, dim3(grid), dim3(CNT_NT), CntLds::bytes, st, a);
  return hipGetLastError();
}

hipError_t launch_cnt_rollup(const int64_t* values, uint32_t count, const uint32_t* group, uint32_t ngroups,
                             int64_t* g_out, uint32_t* status, int max_wg, hipStream_t st) {
  hipError_t e;
  if ((e = hipMemsetAsync(g_out, 0, (size_t)ngroups * 8, st))) return e;
  if ((e = hipMemsetAsync(status, 0xFF, 4, st))) return e;
  if (count == 0) return hipSuccess;
  if (max_wg < 1) max_wg = 1;
  const uint32_t lds_groups = ngroups <= CNT_RU_LDS_GROUPS ? ngroups : 0;
  // a workgroup clears and flushes lds_groups sums: give it at least as many members
  const size_t per = (size_t)CNT_NT * 4 > lds_groups ? (size_t)CNT_NT * 4 : lds_groups;
  size_t grid = ((size_t)count + per - 1) / per;
  if (grid > (size_t)max_wg) grid = (size_t)max_wg;
  hipLaunchKernelGGL(k_cnt_rollup, dim3((uint32_t)grid), dim3(CNT_NT), (size_t)lds_groups * 8, st, values, count, group,
                     ngroups, lds_groups, g_out, status);
  return hipGetLastError();
}

}  // namespace l5dh
