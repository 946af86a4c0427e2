// l5dh_tables.hpp -- the bucket limits and the constant lookup tables built from
// them on the host.  Plain C++17, no HIP: l5dh_tables.cpp builds with g++ alone
// (tests/c/tables_check.cpp runs it under ASan + UBSan against the oracle).
#pragma once

#include <cstddef>
#include <cstdint>

namespace l5dh {

constexpr int NL = 1797;            // BucketedHistogram.scala:42
constexpr int NB = 1798;            // counts = limits + overflow bucket
constexpr int INT_MAXV = 2147483647;
constexpr int LIM_PAD = 2048;       // limits padded with Int.MaxValue for an 11-step search
constexpr int ROW = 1800;           // state row stride in u32 (16-B aligned rows)
constexpr int LUT_N = 1664;         // bucket bracket LUT: 64 direct + 25 octaves x 64
constexpr int LUT2_N = 1024;        // exact bucket + offset LUT for keys < 2^21 (64 direct + 15 octaves x 64)
// (the level-1 record's escape threshold: l5dh_kernels.hpp)
constexpr uint32_t V_ESC = (1u << 21) - 2048u;

// BucketedHistogram.scala:25-40 (makeLimitsFor), error 0.005.  Host copy used
// to build the device tables; the oracle's independent restatement checks it.
struct HostLimits {
  int32_t L[NL];
  bool ok = false;
  HostLimits();
};
const HostLimits& host_limits();

// bucket(v) = number of limits <= v (upper bound), for the LUT builders.
int host_bucket(const int32_t* L, int64_t v);

// Cumulative `le` buckets.  A cut c in [1, NL] stands for buckets 0..c-1, i.e. the samples
// with (long)value <= L[c-1] - 1, so its exact label is le = L[c-1] - 1.  Each bound B is
// snapped DOWN to the largest such le <= floor(B): cuts[i] = #{ j : L[j] - 1 <= floor(B) }
// clipped to [1, NL] (B < 1 gives cut 1, le 0; +Inf and anything >= L[NL-1] - 1 give NL),
// le[i] = L[cuts[i] - 1] - 1.  No deduplication: bounds that snap to one cut yield equal
// cuts.  NaN or B < 0: -EINVAL (nothing is written then).  cuts / le: each nullable.
int le_cuts(const double* bounds, size_t n, uint32_t* cuts, int64_t* le);

// LUT for bucket_lut: builds lut[LUT_N] from the limits; returns the largest
// number of limits inside one LUT interval (the device search assumes <= 2).
int build_bucket_lut(const int32_t* limits, uint32_t* lut);
// LUT for bucket_lut2 (keys < 2^21), verified exhaustively; 0 on success.
int build_bucket_lut2(const int32_t* limits, uint32_t* lut2);
int build_bucket_lut3(const int32_t* limits, uint32_t* lut3);

// Every constant table of a context, as uploaded by l5dh_open.
struct HostTables {
  int32_t lim_pad[LIM_PAD];   // limits padded with Int.MaxValue
  int32_t mid[NB];            // value reported for bucket b
  int32_t base[ROW];          // lower limit of bucket b (0 for b == 0), zero padded
  uint32_t lut[LUT_N];        // bucket_lut
  uint32_t lut2[4 * LUT2_N];  // lut2, then lut3 (one device array holds both)
};
// Builds the tables once per process; 0 and *out on success, -EIO when the limits
// or a table's self-check failed.
int host_tables(const HostTables** out);

}  // namespace l5dh
