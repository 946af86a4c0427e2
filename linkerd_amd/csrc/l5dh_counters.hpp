// l5dh_counters.hpp -- the counter space's kernels (l5dh_counters.hip): batched adds into
// int64 values[max_counters] (Metric.Counter.incr, Metric.scala:14-20) and per-group sums of
// a range of them.  Every sum is a two's-complement sum that wraps like a Java long.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace l5dh {

constexpr uint32_t CNT_MAX = 1u << 24;          // = L5DH_MAX_COUNTERS
constexpr uint32_t CNT_NO_GROUP = 0xFFFFFFFFu;  // = L5DH_NO_GROUP
constexpr int CNT_NT = 1024;                    // threads of a workgroup (one workgroup per CU: the table is 96 KB)
constexpr uint32_t CNT_SLAB_MIN = 1u << 12;     // elements of a slab: n / workgroups, within these bounds;
constexpr uint32_t CNT_SLAB_MAX = 1u << 18;     // a workgroup flushes its claim table at each slab's end
constexpr uint32_t CNT_RU_LDS_GROUPS = 8192;    // rollup: LDS-private partial sums up to this many groups

// statistics words of a counter space (u64 each; only ever added to)
enum : uint32_t {
  CS_ADDS = 0,     // adds applied (CS_LDS + CS_GLOBAL)
  CS_LDS = 1,      // ... through a claim-table slot
  CS_GLOBAL = 2,   // ... by a global atomic of their own
  CS_DROPPED = 3,  // ids >= max_counters: never applied
  CS_WORDS = 4
};

// values[ids[i]] += deltas[i] (deltas == nullptr: 1) for i < n; ids and deltas are device
// memory at any 4-byte alignment.  At most max_wg workgroups.  plain: no claim table, one global
// atomic per add (L5DH_PARAM_VARIANT bit 3).  n == 0 launches nothing.
hipError_t launch_cnt_add(const uint32_t* ids, const int32_t* deltas, size_t n, int64_t* values, uint32_t max_counters,
                          uint64_t* stats, int max_wg, bool plain, hipStream_t st);

// g_out[g] = the sum of values[i] over i < count with group[i] == g, for g < ngroups (g_out is
// zeroed here).  A map value that is neither < ngroups nor CNT_NO_GROUP lowers *status (preset
// to 0xFFFFFFFF here) to the least such i and counts as no group.
hipError_t launch_cnt_rollup(const int64_t* values, uint32_t count, const uint32_t* group, uint32_t ngroups,
                             int64_t* g_out, uint32_t* status, int max_wg, hipStream_t st);

// Once per process before the first launch (dynamic LDS above 64 KB).
hipError_t set_counters_attributes();

}  // namespace l5dh
