// l5dh_top.hpp -- exact top-k selection over summary rows (l5dh_top.hip).
#pragma once

#include "l5dh_kernels.hpp"

namespace l5dh {

constexpr uint32_t TOP_LIMIT = 1024;     // = L5DH_TOP_LIMIT: k per call
constexpr uint32_t TOP_CHUNK = 4096;     // rows (items) one workgroup sorts: 4096 x 16 B = 64 KB of LDS
constexpr uint32_t TOP_THREADS = 512;    // threads of the sorting workgroups
constexpr uint32_t TOP_BY_FIELDS = 11;   // by < 11: the field's index in Summary88
constexpr uint32_t TOP_BY_QUANTILE = 11; // = L5DH_BY_QUANTILE: the key is qv[i]
constexpr size_t TOP_MAX_ROWS = (size_t)1 << 24;  // rows of one selection (bounds the workspace)

// One candidate: 16 B.  The lists are sorted "best first": valid before invalid, then key
// descending, then id ascending.  key is the order-preserving u64 image of the row's key
// (complemented for SMALLEST, so "descending" serves both orders).
struct alignas(16) TopItem {
  uint64_t key;
  uint32_t id;
  uint32_t valid;
};
static_assert(sizeof(TopItem) == 16, "TopItem is one 16-B LDS slot");

// The power of two >= k (k in [1, TOP_LIMIT]): the length of every list.
constexpr uint32_t top_kp(uint32_t k) {
  uint32_t p = 1;
  while (p < k) p <<= 1;
  return p;
}
// Lists one merge workgroup takes.
constexpr uint32_t top_fanin(uint32_t kp) { return TOP_CHUNK / kp; }
// Lists of level 0 (one per chunk) and of the level after one of `lists`.
inline size_t top_chunks(size_t n) { return (n + TOP_CHUNK - 1) / TOP_CHUNK; }
inline size_t top_next(size_t lists, uint32_t kp) { return (lists + top_fanin(kp) - 1) / top_fanin(kp); }
// Bytes of the two list buffers of a selection over n rows: level 0 in `a`, the merge
// levels alternate b, a, b, ...
inline size_t top_bytes_a(size_t n, uint32_t kp) { return top_chunks(n) * kp * sizeof(TopItem); }
inline size_t top_bytes_b(size_t n, uint32_t kp) { return top_next(top_chunks(n), kp) * kp * sizeof(TopItem); }

struct TopArgs {
  const Summary88* summ;   // [n] the rows (device)
  const int64_t* qv;       // [n] the quantile values (by == TOP_BY_QUANTILE), else unused
  const uint32_t* group;   // [n], nullable: row i is a candidate only if group[i] == g
  uint32_t g;
  uint32_t n;              // 1 .. TOP_MAX_ROWS
  uint32_t first;          // id of row 0
  uint32_t by;             // 0 .. 11
  uint32_t smallest;       // 0: LARGEST, 1: SMALLEST
  int64_t min_count;       // >= 0
  uint32_t k;              // 1 .. TOP_LIMIT
  TopItem* list_a;         // >= top_bytes_a(n, top_kp(k))
  TopItem* list_b;         // >= top_bytes_b(n, top_kp(k))
  // outputs (device): m = min(k, candidates) entries of each are written, nothing beyond
  uint32_t* ids_out;       // [k]
  Summary88* top_out;      // [k], nullable
  int64_t* q_out;          // [k], nullable (by == TOP_BY_QUANTILE)
  uint32_t* n_out;         // m
  uint32_t* n_out2;        // nullable: m once more (the caller's device word)
};

// Enqueues the tournament: k_top_build (one workgroup per chunk), the k_top_merge levels
// (sizes known here: no device counter, no host wait) and k_top_gather.
hipError_t launch_top(const TopArgs& a, hipStream_t st);

}  // namespace l5dh
