// fmt_check.cpp -- linkerd_amd/csrc/l5dh_fmt.hpp as plain C++ with its own main, for a
// host build under -fsanitize=address,undefined:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o fmt_check tests/c/fmt_check.cpp && ./fmt_check < inputs > texts
// Input lines: `d <16 hex digits of the double's bits>`, `l <int64>`, `u <uint64>`.
// Output: one text per line (`ERANGE` outside the domain), written into a buffer of
// exactly the documented size so the sanitizer sees any overrun.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>

#include "../../linkerd_amd/csrc/l5dh_fmt.hpp"

int main() {
  char line[128];
  while (fgets(line, sizeof(line), stdin)) {
    if (line[0] == 'd') {
      uint64_t bits = 0;
      if (sscanf(line + 1, "%" SCNx64, &bits) != 1) return 2;
      double x;
      memcpy(&x, &bits, 8);
      std::unique_ptr<char[]> out(new char[l5dh::fmt::DOUBLE_CHARS]);
      const int n = l5dh::fmt::format_double(x, out.get());
      if (n < 0)
        puts("ERANGE");
      else
        printf("%.*s\n", n, out.get());
    } else if (line[0] == 'l' || line[0] == 'u') {
      std::unique_ptr<char[]> out(new char[l5dh::fmt::LONG_CHARS]);
      int n;
      if (line[0] == 'l') {
        int64_t v = 0;
        if (sscanf(line + 1, "%" SCNd64, &v) != 1) return 2;
        n = l5dh::fmt::format_long(v, out.get());
        if (n != l5dh::fmt::long_digits(v)) return 3;
      } else {
        uint64_t v = 0;
        if (sscanf(line + 1, "%" SCNu64, &v) != 1) return 2;
        n = l5dh::fmt::format_ulong(v, out.get());
        if (n != l5dh::fmt::ulong_digits(v)) return 3;
      }
      printf("%.*s\n", n, out.get());
    }
  }
  return 0;
}
