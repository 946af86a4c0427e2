// tables_check.cpp -- the engine's host tables (linkerd_amd/csrc/l5dh_tables.cpp) against
// the CPU oracle, as a plain executable (tests/test_sanitizers.py builds it with ASan +
// UBSan): the limits, the three LUT builders, and the decode of `lut` -- a host
// restatement of bucket_lut (l5dh_device.hpp) -- over every key below 2^21, around every
// limit and at both ends of every LUT interval.  Prints "ok".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hist_oracle.h"
#include "l5dh_tables.hpp"

using namespace l5dh;

// bucket_lut of l5dh_device.hpp, statement for statement (lim: the padded limits).
static uint32_t bucket_lut(uint32_t v, const uint32_t* lut, const int32_t* lim) {
  uint32_t idx, start;
  if (v < 64u) {
    idx = v;
    start = v;
  } else {
    const int sh = 25 - __builtin_clz(v);  // exponent - 6
    idx = 64u + (uint32_t)sh * 64u + ((v >> sh) & 63u);
    start = (v >> sh) << sh;
  }
  const uint32_t x = lut[idx];
  uint32_t b = x & 0x7FFu;
  const uint32_t o1 = (x >> 11) & 0x3FFu;
  const uint32_t o2 = x >> 21;
  if (o1 == 0x3FFu) {
    b += (lim[b] <= (int32_t)v) ? 1u : 0u;
    b += (lim[b] <= (int32_t)v) ? 1u : 0u;
  } else {
    const uint32_t d = v - start;
    b += (o1 != 0u && d >= o1) ? 1u : 0u;
    b += (o2 != 0u && d >= o2) ? 1u : 0u;
  }
  return b;
}

static int fail(const char* what, long long a, long long b, long long c) {
  std::printf("FAIL %s: %lld %lld %lld\n", what, a, b, c);
  return 1;
}

int main() {
  const HostLimits& hl = host_limits();
  if (!hl.ok) return fail("host_limits", 0, 0, 0);
  const int32_t* ref = l5do_default_limits();
  static_assert(NL == L5DO_NLIMITS && NB == L5DO_NBUCKETS, "table sizes");
  for (int i = 0; i < NL; ++i)
    if (hl.L[i] != ref[i]) return fail("limit", i, hl.L[i], ref[i]);

  std::vector<uint32_t> lut(LUT_N), lut2(2 * LUT2_N), lut3(2 * LUT2_N);
  const int maxin = build_bucket_lut(hl.L, lut.data());
  if (maxin > 2) return fail("build_bucket_lut: limits per interval", maxin, 0, 0);
  if (int rc = build_bucket_lut2(hl.L, lut2.data())) return fail("build_bucket_lut2", rc, 0, 0);
  if (int rc = build_bucket_lut3(hl.L, lut3.data())) return fail("build_bucket_lut3", rc, 0, 0);

  // the process-wide tables: built, and the same LUTs as the builders give
  const HostTables* ht = nullptr;
  if (int rc = host_tables(&ht)) return fail("host_tables", rc, 0, 0);
  for (int i = 0; i < LUT_N; ++i)
    if (ht->lut[i] != lut[i]) return fail("host_tables lut", i, ht->lut[i], lut[i]);
  for (int i = 0; i < 2 * LUT2_N; ++i)
    if (ht->lut2[i] != lut2[i] || ht->lut2[2 * LUT2_N + i] != lut3[i]) return fail("host_tables lut2/lut3", i, 0, 0);
  for (int i = 0; i < LIM_PAD; ++i)
    if (ht->lim_pad[i] != (i < NL ? ref[i] : INT_MAXV)) return fail("lim_pad", i, ht->lim_pad[i], 0);

  // bucket_lut's domain is 0 <= v < Int.MaxValue
  const int64_t vmax = 2147483646;
  long long checked = 0;
  auto check = [&](int64_t v) {
    if (v < 0) v = 0;
    if (v > vmax) v = vmax;
    ++checked;
    return (int)bucket_lut((uint32_t)v, ht->lut, ht->lim_pad) == l5do_bucket_of(v);
  };
  for (int64_t v = 0; v < ((int64_t)1 << 21); ++v)
    if (!check(v)) return fail("bucket_lut", v, bucket_lut((uint32_t)v, ht->lut, ht->lim_pad), l5do_bucket_of(v));
  for (int i = 0; i < NL; ++i)
    for (int64_t v = (int64_t)hl.L[i] - 1; v <= (int64_t)hl.L[i] + 1; ++v)
      if (!check(v)) return fail("bucket_lut at limit", i, v, l5do_bucket_of(v));
  for (int e = 6; e <= 30; ++e)  // (the 64 direct entries, v < 64, are covered above)
    for (int m = 0; m < 64; ++m) {
      const int64_t start = (int64_t)(64 + m) << (e - 6), end = ((int64_t)(64 + m + 1) << (e - 6)) - 1;
      if (!check(start)) return fail("bucket_lut at interval start", e, m, start);
      if (!check(end)) return fail("bucket_lut at interval end", e, m, end);
    }
  if (checked != ((long long)1 << 21) + 3LL * NL + 2LL * 25 * 64) return fail("cases", checked, 0, 0);
  std::printf("ok\n");
  return 0;
}
