// fmt_float_check.cpp -- linkerd_amd/csrc/l5dh_fmt.hpp as plain C++ with its own main, for a
// host build under -fsanitize=address,undefined (tests/test_fmt_float_host.py):
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o fmt_float_check tests/c/fmt_float_check.cpp && ./fmt_float_check < inputs > texts
// Input lines: `f <8 hex digits of the float's bits>`, `d <16 hex digits of the double's
// bits>`.  Output: format_float's / format_double's text per line (`ERANGE` outside the
// domain), written into a heap buffer of exactly the documented size so the sanitizer
// sees any overrun.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>

#include "../../linkerd_amd/csrc/l5dh_fmt.hpp"

static void print(int n, const char* text) {
  if (n < 0)
    puts("ERANGE");
  else
    printf("%.*s\n", n, text);
}

int main() {
  char line[128];
  while (fgets(line, sizeof(line), stdin)) {
    if (line[0] == 'f') {
      uint32_t bits = 0;
      if (sscanf(line + 1, "%" SCNx32, &bits) != 1) return 2;
      float x;
      memcpy(&x, &bits, 4);
      std::unique_ptr<char[]> out(new char[l5dh::fmt::FLOAT_CHARS]);
      print(l5dh::fmt::format_float(x, out.get()), out.get());
    } else if (line[0] == 'd') {
      uint64_t bits = 0;
      if (sscanf(line + 1, "%" SCNx64, &bits) != 1) return 2;
      double x;
      memcpy(&x, &bits, 8);
      std::unique_ptr<char[]> out(new char[l5dh::fmt::DOUBLE_CHARS]);
      print(l5dh::fmt::format_double(x, out.get()), out.get());
    } else if (line[0] != '\n') {
      return 2;
    }
  }
  return 0;
}
