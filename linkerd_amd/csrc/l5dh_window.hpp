// l5dh_window.hpp -- the sliding window's kernels (l5dh_window.hip): per series, the sum of
// the sparse rows that the ring's slots hold (the CSR of the sparse export), and optionally
// the open interval's live row.
#pragma once

#include "l5dh_import.hpp"
#include "l5dh_kernels.hpp"

namespace l5dh {

constexpr int WIN_MAX = 64;  // = L5DH_WINDOW_MAX: slots of a ring, one lane of a wave each

// The slots a query sums, by value in the kernel arguments: slot k's CSR (row_off [count + 1],
// entries, totals [count]), the series it covers and its push number.  Entries k >= n are
// zero: count 0 admits no series.
struct WinSlots {
  const uint64_t* row_off[WIN_MAX];
  const BucketEntry* entries[WIN_MAX];
  const int64_t* totals[WIN_MAX];
  uint64_t seq[WIN_MAX];
  uint32_t count[WIN_MAX];
  uint32_t n;
};

// Per series r of [first, first + count): the sum of its rows in the slots with seq > born[r]
// and count > r, plus (include_open) its state row and total + sumfix when its tile is dirty.
// out_rows [count][1798], out_totals [count], out_summ [count]: each nullable.  A bucket sum
// above 2^31 - 1 lowers *status (preset to 0xFFFFFFFF) to the least such series.
hipError_t launch_win_sum(const WinSlots& slots, const uint64_t* born, State state, uint32_t first, uint32_t count,
                          int include_open, Tables tb, int32_t* out_rows, int64_t* out_totals, Summary88* out_summ,
                          uint32_t* status, hipStream_t st);
// born[first .. first + count) = seq
hipError_t launch_win_born(uint64_t* born, uint32_t first, uint32_t count, uint64_t seq, hipStream_t st);

}  // namespace l5dh
