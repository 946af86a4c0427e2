// l5dh_rollup.hpp -- label rollups: per-group sums of series rows (l5dh_rollup.hip).
#pragma once

#include <algorithm>

#include "l5dh_kernels.hpp"

namespace l5dh {

constexpr uint32_t RU_NO_GROUP = 0xFFFFFFFFu;  // = L5DH_NO_GROUP
constexpr uint32_t RU_ITEM_DEFAULT = 64;       // members per work item (L5DH_PARAM_ROLLUP_ITEM)
constexpr uint32_t RU_MAX_ITEMS = 1024;        // items per group: larger groups take longer items
constexpr int RU_PROW = ROW;                   // u64 words of a partial row

// The work-item rule: a group of c members is cut into items of
// max(item, ceil(c / RU_MAX_ITEMS)) members, so it has at most RU_MAX_ITEMS items;
// an empty group has one (empty) item, which writes its zero results.
__host__ __device__ constexpr uint32_t ru_per_item(uint32_t c, uint32_t item) {
  const uint32_t m = (c + RU_MAX_ITEMS - 1) / RU_MAX_ITEMS;
  return m > item ? m : item;
}
__host__ __device__ constexpr uint32_t ru_items(uint32_t c, uint32_t item) {
  return c ? (c + ru_per_item(c, item) - 1) / ru_per_item(c, item) : 1u;
}

// status words of one call (RollupWork::hdr)
enum : uint32_t {
  RH_BADIDX = 0,  // least map index whose entry is neither < G nor RU_NO_GROUP (0xFFFFFFFF: none)
  RH_RANGE = 1,   // least group with a bucket sum above 2^31 - 1 (0xFFFFFFFF: none)
  RH_SLOTS = 2,   // partial rows handed out
  RH_NMULTI = 3,  // groups of more than one item
  RH_BOUNDS = 4,  // a workspace bound was hit (internal error; the outputs are incomplete)
  RH_WORDS = 8
};

// Capacities of the workspace for `count` map entries, G groups, `item` members per item.
struct RollupCaps {
  size_t items, multi, slots;
};
inline RollupCaps rollup_caps(size_t count, size_t G, uint32_t item) {
  RollupCaps c;
  // sum over groups of max(1, ceil(c_g / m_g)), m_g >= item
  c.items = count / item + G + 2;
  // groups of more than one item hold more than `item` members each; their items number
  // ceil(c_g / m_g) <= c_g / item + 1 < 2 c_g / item, and no item is empty
  c.multi = std::min<size_t>(G, count / ((size_t)item + 1));
  c.slots = std::min<size_t>(count, 2 * count / item + 1);
  return c;
}

struct RollupWork {       // device workspace of one call
  const uint32_t* group;  // [count] group of series first + i
  uint32_t count, G, first, item;
  uint32_t* cnt;          // [G + 1] members per group (a clean tile's series are no members); [G] = 0
  uint32_t* nitems;       // [G + 1] items per group; [G] = 0
  uint32_t* cursor;       // [G] members filled
  uint32_t* pbase;        // [G] first partial row of a group of several items
  uint64_t* moff;         // [G + 1] exclusive prefix of cnt
  uint64_t* ioff;         // [G + 1] exclusive prefix of nitems
  uint32_t* members;      // [count] map indices, group by group
  uint32_t* igroup;       // [caps.items] item -> group
  uint32_t* mlist;        // [caps.multi] groups of several items
  uint64_t* partial;      // [caps.slots][RU_PROW] exact partial rows, then the item's total at word NB
  uint32_t* hdr;          // [RH_WORDS]
  void* tmp;              // the scans' temporary storage
  size_t tmp_bytes;
  RollupCaps caps;
};

struct RollupOut {  // per group, each nullable
  Summary88* summ;
  int32_t* counts;  // [G][1798]
  int64_t* totals;  // [G]
};

// Bytes of the scans' temporary storage for G groups.
size_t rollup_tmp_bytes(uint32_t G);
// Enqueues the whole rollup: ext == nullptr sums the live state rows of series
// [w.first, w.first + w.count) (clean tiles contribute nothing and are not read),
// otherwise the external dense rows ext[w.count][1798] (+ ext_total, nullable).
hipError_t launch_rollup(const RollupWork& w, State state, const int32_t* ext, const int64_t* ext_total, Tables tb,
                         RollupOut out, hipStream_t st);

}  // namespace l5dh
