// l5dh_quant.hpp -- exact configurable quantiles of series rows (l5dh_quant.hip).
#pragma once

#include "l5dh_kernels.hpp"

namespace l5dh {

constexpr uint32_t Q_MAX = 64;  // = L5DH_Q_MAX: quantiles per call (one lane each)

// The quantiles of one call, by value in the kernel arguments: q[k] in [0, 1] for k < K
// (checked on the host), in any order, duplicates included.
struct QuantQ {
  double q[Q_MAX];
};

// Enqueues k_quant over `count` rows: ext == nullptr reads the live state rows of series
// [first, first + count) (a row of a clean tile gives K zeros and is not read), otherwise
// the external dense rows ext[count][1798].  Per row i and k < K:
//   t = Math.round(q[k] * (double)num);  q_out[i][k] = t == 0 ? 0 : mid[first bucket whose
//   running count >= t]                                    (BucketedHistogram.percentile)
// with num the row's 64-bit count: q_out is [count][K] int64.
hipError_t launch_quant(State state, uint32_t first, uint32_t count, const int32_t* ext, const QuantQ& qs, uint32_t K,
                        const int32_t* mid, int64_t* q_out, hipStream_t st);

}  // namespace l5dh
