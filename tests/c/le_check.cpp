// le_check.cpp -- le_cuts (linkerd_amd/csrc/l5dh_tables.cpp) against the CPU oracle, as a
// plain executable (tests/test_le_host.py builds it with ASan + UBSan).  A bound B is
// snapped down to the cut c = #{ j : L[j] - 1 <= floor(B) } clipped to [1, 1797] with the
// exact label le = L[c-1] - 1.  Checked: the cut against a brute-force count over the
// oracle's limits for every integer bound 0..70000, L[i]-2 .. L[i]+1 of every limit, x.5
// values, +Inf and 1e300; NaN and negative bounds are rejected and write nothing; and,
// for integer v around every limit, v <= le <=> the oracle's bucket of v is below the cut
// (so the count at the cut IS the number of samples <= le).  Prints "ok".
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "hist_oracle.h"
#include "l5dh_tables.hpp"

using namespace l5dh;

static int fail(const char* what, double a, long long b, long long c) {
  std::printf("FAIL %s: %.17g %lld %lld\n", what, a, b, c);
  return 1;
}

int main() {
  const int32_t* L = l5do_default_limits();
  static_assert(NL == L5DO_NLIMITS, "table sizes");
  std::vector<double> bounds;
  for (int v = 0; v <= 70000; ++v) bounds.push_back((double)v);
  for (int i = 0; i < NL; ++i)
    for (int d = -2; d <= 1; ++d)
      if ((int64_t)L[i] + d >= 0) bounds.push_back((double)((int64_t)L[i] + d));
  for (int v = 0; v <= 2000; ++v) bounds.push_back(v + 0.5);
  for (int i = 0; i < NL; i += 7) bounds.push_back((double)L[i] - 0.5);
  bounds.push_back(0.25);
  bounds.push_back(2147483646.0);
  bounds.push_back(2147483647.0);
  bounds.push_back(4294967296.5);
  bounds.push_back(1e300);
  bounds.push_back(std::numeric_limits<double>::infinity());

  const size_t n = bounds.size();
  std::vector<uint32_t> cuts(n, 0xDEADBEEFu);
  std::vector<int64_t> le(n, -7);
  if (int rc = le_cuts(bounds.data(), n, cuts.data(), le.data())) return fail("le_cuts", 0, rc, 0);
  for (size_t k = 0; k < n; ++k) {
    const double f = std::floor(bounds[k]);
    long long c = 0;  // brute force
    for (int j = 0; j < NL; ++j) c += ((double)L[j] - 1.0 <= f) ? 1 : 0;
    if (c < 1) c = 1;
    if ((long long)cuts[k] != c) return fail("cut", bounds[k], cuts[k], c);
    if (le[k] != (int64_t)L[c - 1] - 1) return fail("le", bounds[k], le[k], (int64_t)L[c - 1] - 1);
    if ((double)le[k] > f && c > 1) return fail("le above the bound", bounds[k], le[k], c);
    // the next label up would pass the bound: le is the largest one <= floor(B)
    if (c < NL && (double)L[c] - 1.0 <= f) return fail("a larger label fits", bounds[k], le[k], c);
    // samples: v <= le  <=>  bucket(v) < c, around the cut's limit and the bound
    for (int64_t v = le[k] - 2; v <= le[k] + 2; ++v)
      if ((v <= le[k]) != (l5do_bucket_of(v) < (int)c)) return fail("bucket vs le", bounds[k], v, c);
  }
  // +Inf, 1e300 and everything from L[1796] - 1 up: the last cut
  for (size_t k = n - 5; k < n; ++k)
    if (cuts[k] != (uint32_t)NL) return fail("last cut", bounds[k], cuts[k], NL);
  // around every limit, for the cut that ends at that limit
  for (int c = 1; c <= NL; ++c)
    for (int64_t v = (int64_t)L[c - 1] - 2; v <= (int64_t)L[c - 1] + 1; ++v)
      if ((v <= (int64_t)L[c - 1] - 1) != (l5do_bucket_of(v) < c)) return fail("bucket at limit", 0, v, c);
  // the issue's worked examples
  const double ex[] = {1, 2, 5, 10, 25, 50, 100, 250, 500, 1000, 60000};
  const uint32_t ex_cut[] = {2, 3, 6, 11, 26, 51, 101, 193, 262, 332, 743};
  const int64_t ex_le[] = {1, 2, 5, 10, 25, 50, 100, 250, 497, 997, 59582};
  uint32_t ec[11];
  int64_t el[11];
  if (le_cuts(ex, 11, ec, el) != 0) return fail("examples", 0, 0, 0);
  for (int k = 0; k < 11; ++k)
    if (ec[k] != ex_cut[k] || el[k] != ex_le[k]) return fail("example", ex[k], ec[k], el[k]);
  // rejected bounds write nothing, wherever they stand
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double bad[][3] = {{10.0, nan, 20.0}, {10.0, 20.0, -1.0}, {-0.5, 1.0, 2.0},
                           {1.0, -std::numeric_limits<double>::infinity(), 2.0}};
  for (const auto& b : bad) {
    uint32_t bc[3] = {77u, 77u, 77u};
    int64_t bl[3] = {-7, -7, -7};
    if (le_cuts(b, 3, bc, bl) != -EINVAL) return fail("not rejected", b[0], 0, 0);
    for (int k = 0; k < 3; ++k)
      if (bc[k] != 77u || bl[k] != -7) return fail("written on rejection", b[k], bc[k], bl[k]);
  }
  if (le_cuts(nullptr, 0, nullptr, nullptr) != 0) return fail("empty", 0, 0, 0);
  uint32_t only_cut = 0;
  const double one = 250.0;
  if (le_cuts(&one, 1, &only_cut, nullptr) != 0 || only_cut != 193u) return fail("null le", one, only_cut, 0);
  std::printf("ok\n");
  return 0;
}
