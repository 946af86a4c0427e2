// l5dh_le.hpp -- exact cumulative `le` buckets of series rows (l5dh_le.hip).
#pragma once

#include "l5dh_kernels.hpp"

namespace l5dh {

constexpr uint32_t LE_MAX = 64;  // = L5DH_LE_MAX: cuts per call (one lane each; lane K carries the row count)

// The cuts of one call, by value in the kernel arguments: c[k] in [1, NL], strictly
// ascending for k < K (checked on the host); cut c stands for buckets 0..c-1.
struct LeCuts {
  uint32_t c[LE_MAX];
};

// Enqueues k_le over `count` rows: ext == nullptr reads the live state rows of series
// [first, first + count) (a row of a clean tile contributes zeros and is not read;
// a row's sum is total + sumfix), otherwise the external dense rows ext[count][1798]
// (+ ext_total, nullable: 0).  Per row i: le_out[i][k] = counts[0] + ... + counts[c[k] - 1]
// for k < K and le_out[i][K] = the row's count (u64 words), sums_out[i] (nullable) = the
// row's sum; accumulate != 0 adds to what the outputs hold (the sums wrap like a Java long).
hipError_t launch_le(State state, uint32_t first, uint32_t count, const int32_t* ext, const int64_t* ext_total,
                     const LeCuts& cuts, uint32_t K, uint64_t* le_out, int64_t* sums_out, int accumulate,
                     hipStream_t st);

}  // namespace l5dh
