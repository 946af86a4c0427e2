// l5dh_tables.cpp -- the bucket limits and the host builders of the device's
// constant tables (lim_pad, mid, base, lut, lut2, lut3).  No HIP in this file.
#include "l5dh_tables.hpp"

#include <algorithm>
#include <cerrno>
#include <cmath>

namespace l5dh {

HostLimits::HostLimits() {
  const double maxValue = 2147483647.0;
  const double factor = 1.0 + (0.005 * 2);
  int n = 0;
  L[n++] = 1;
  int32_t last = -1;
  volatile double cur = 1.0;  // volatile: no contraction / excess precision
  for (;;) {
    volatile double next = cur * factor;
    if (next >= maxValue) break;
    const int32_t v = (int32_t)next + 1;
    if (v != last) {
      if (n >= NL) return;
      L[n++] = v;
      last = v;
    }
    cur = next;
  }
  ok = (n == NL);
}

const HostLimits& host_limits() {
  static HostLimits h;
  return h;
}

int host_bucket(const int32_t* L, int64_t v) {
  int lo = 0, hi = NL;
  while (lo < hi) {
    const int m = (lo + hi) / 2;
    if ((int64_t)L[m] <= v) lo = m + 1; else hi = m;
  }
  return lo;
}

int le_cuts(const double* bounds, size_t n, uint32_t* cuts, int64_t* le) {
  const HostLimits& hl = host_limits();
  if (!hl.ok) return -EIO;
  if (n && !bounds) return -EINVAL;
  for (size_t i = 0; i < n; ++i)
    if (!(bounds[i] >= 0.0)) return -EINVAL;  // (NaN compares false)
  for (size_t i = 0; i < n; ++i) {
    const double f = std::floor(bounds[i]);
    // (int32 limits are exact doubles; f may be +Inf)
    int lo = 0, hi = NL;  // c = #{ j : L[j] - 1 <= f }
    while (lo < hi) {
      const int m = (lo + hi) / 2;
      if ((double)hl.L[m] - 1.0 <= f) lo = m + 1; else hi = m;
    }
    const int c = lo < 1 ? 1 : lo;
    if (cuts) cuts[i] = (uint32_t)c;
    if (le) le[i] = (int64_t)hl.L[c - 1] - 1;
  }
  return 0;
}

int build_bucket_lut(const int32_t* L, uint32_t* lut) {
  // entry = b0 | off1 << 11 | off2 << 21 (offsets of the limits inside the
  // interval from its start, 0 = none) or off1 = 0x3FF for intervals wider
  // than 1024 (the device then compares against the limits).
  int maxin = 0, k = 0;
  for (int v = 0; v < 64; ++v) lut[k++] = (uint32_t)host_bucket(L, v);
  for (int e = 6; e <= 30; ++e)
    for (int m = 0; m < 64; ++m) {
      const int64_t start = (int64_t)(64 + m) << (e - 6);
      int64_t end = ((int64_t)(64 + m + 1) << (e - 6)) - 1;
      if (end > 2147483646) end = 2147483646;
      const int b0 = host_bucket(L, start);
      const int nin = host_bucket(L, end) - b0;
      maxin = std::max(maxin, nin);
      uint32_t x = (uint32_t)b0;
      if (end - start + 1 <= 1024) {
        for (int i = 0; i < nin && i < 2; ++i) {
          const int64_t off = (int64_t)L[b0 + i] - start;  // >= 1: L[b0] > start
          if (off < 1 || off > 1023) return 99;
          x |= (uint32_t)off << (11 + 10 * i);
        }
      } else {
        x |= 0x3FFu << 11;
      }
      lut[k++] = x;
    }
  return k == LUT_N ? maxin : 99;
}

int build_bucket_lut2(const int32_t* L, uint32_t* lut2) {
  int k = 0;
  auto entry = [&](int64_t start, int64_t end) {
    const int b0 = host_bucket(L, start);
    uint32_t o[2] = {0xFFFFu, 0xFFFFu};
    for (int i = 0; i < 2 && b0 + i < NL && L[b0 + i] <= end; ++i) {
      const int64_t off = (int64_t)L[b0 + i] - start;
      if (off < 1 || off >= 0xFFFF) return false;
      o[i] = (uint32_t)off;
    }
    if (b0 + 2 < NL && L[b0 + 2] <= end) return false;  // at most two limits per interval
    const int64_t p = start - (b0 ? (int64_t)L[b0 - 1] : 0);
    if (p < 0 || p > 0xFFFF) return false;
    lut2[2 * k] = o[0] | o[1] << 16;
    lut2[2 * k + 1] = (uint32_t)b0 | (uint32_t)p << 16;
    ++k;
    return true;
  };
  for (int v = 0; v < 64; ++v)
    if (!entry(v, v)) return 1;
  for (int e = 6; e <= 20; ++e)
    for (int m = 0; m < 64; ++m)
      if (!entry((int64_t)(64 + m) << (e - 6), ((int64_t)(64 + m + 1) << (e - 6)) - 1)) return 1;
  if (k != LUT2_N) return 1;
  // exhaustive check of the device decode (bucket_lut2) against upper_bound
  for (uint32_t v = 0; v < (1u << 21); ++v) {
    const uint32_t sh = v < 64 ? 0u : (uint32_t)(25 - __builtin_clz(v));
    const uint32_t idx = v < 64 ? v : 64u + sh * 64u + ((v >> sh) & 63u);
    const uint32_t start = (v >> sh) << sh;
    const uint32_t d = v - start, x0 = lut2[2 * idx], x1 = lut2[2 * idx + 1];
    const uint32_t o1 = x0 & 0xFFFFu, o2 = x0 >> 16;
    const bool k1 = d >= o1, k2 = d >= o2;
    const uint32_t off = k2 ? d - o2 : (k1 ? d - o1 : d + (x1 >> 16));
    const uint32_t b = (x1 & 0xFFFFu) + k1 + k2;
    const int hb = host_bucket(L, v);
    if ((int)b != hb || off != v - (hb ? (uint32_t)L[hb - 1] : 0u)) return 2;
  }
  return 0;
}

// Level 1's LUT (same intervals and index as lut2): entry {b0 | lim1 << 11, lim2}, the
// absolute limits inside the interval (lim1 = 0x1FFFFF, lim2 = 0xFFFFFFFF: none), so
// bucket = b0 + (v << 11 | 0x7FF >= x0) + (v >= x1) for v < V_ESC -- no interval start
// or offset arithmetic on the device.  Verified exhaustively against upper_bound.
int build_bucket_lut3(const int32_t* L, uint32_t* lut3) {
  int k = 0;
  auto entry = [&](int64_t start, int64_t end) {
    const int b0 = host_bucket(L, start);
    uint32_t lim[2] = {0x1FFFFFu, 0xFFFFFFFFu};
    for (int i = 0; i < 2 && b0 + i < NL && L[b0 + i] <= end; ++i) {
      if (L[b0 + i] <= start || L[b0 + i] >= 0x1FFFFF) return false;
      lim[i] = (uint32_t)L[b0 + i];
    }
    if (b0 + 2 < NL && L[b0 + 2] <= end) return false;  // at most two limits per interval
    if (b0 > 0x7FF) return false;
    lut3[2 * k] = (uint32_t)b0 | lim[0] << 11;
    lut3[2 * k + 1] = lim[1];
    ++k;
    return true;
  };
  for (int v = 0; v < 64; ++v)
    if (!entry(v, v)) return 1;
  for (int e = 6; e <= 20; ++e)
    for (int m = 0; m < 64; ++m)
      if (!entry((int64_t)(64 + m) << (e - 6), ((int64_t)(64 + m + 1) << (e - 6)) - 1)) return 1;
  if (k != LUT2_N) return 1;
  for (uint32_t v = 0; v < V_ESC; ++v) {  // the device index (lut3_index) and decode
    const uint32_t sh = (uint32_t)(25 - __builtin_clz(v | 64u));
    const uint32_t idx = (v >> sh) + (sh << 6);
    const uint32_t x0 = lut3[2 * idx], x1 = lut3[2 * idx + 1];
    const uint32_t b = (x0 & 0x7FFu) + ((v << 11 | 0x7FFu) >= x0 ? 1u : 0u) + (v >= x1 ? 1u : 0u);
    if ((int)b != host_bucket(L, v)) return 2;
  }
  return 0;
}

namespace {
struct BuiltTables {
  HostTables t{};
  int rc = -EIO;
  BuiltTables() {
    const HostLimits& hl = host_limits();
    if (!hl.ok) return;
    for (int i = 0; i < LIM_PAD; ++i) t.lim_pad[i] = i < NL ? hl.L[i] : INT_MAXV;
    for (int b = 0; b < NB; ++b) {
      t.mid[b] = b == 0 ? 0 : (b >= NL ? INT_MAXV : (int32_t)(((int64_t)hl.L[b - 1] + hl.L[b]) / 2));
      t.base[b] = b == 0 ? 0 : hl.L[b - 1];
    }
    if (build_bucket_lut(hl.L, t.lut) > 2) return;
    if (build_bucket_lut2(hl.L, t.lut2) | build_bucket_lut3(hl.L, t.lut2 + 2 * LUT2_N)) return;
    rc = 0;
  }
};
}  // namespace

int host_tables(const HostTables** out) {
  static const BuiltTables b;  // once per process
  *out = &b.t;
  return b.rc;
}

}  // namespace l5dh
