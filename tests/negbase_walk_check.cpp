// The device's negabase recurrence (csrc/negbase.cuh) compiled for the host: the statements k_negbase_digits runs,
// driven from stdin.  tests/test_host_logic.py builds this with -fsanitize=address,undefined and compares every line
// with oracle/pyref.py.
//   in : words(4|8) base d negative(0|1) scalar(hex, at most 64 digits)
//   out: the d digits, then 1 if a non-zero magnitude is left after them, else 0
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../halo2_liam_eagen_msm_amd/csrc/negbase.cuh"

using namespace lemsm;

template <int NW>
static bool walk(const u32* s, bool negative, u32 base, u32 d, std::vector<u32>& digits) {
  const NegConsts nc = neg_consts(base);
  NegWalk<NW> w;
  w.init(s, negative);
  for (u32 i = 0; i < d; i++) digits.push_back(w.step(nc));
  return !w.zero();
}

int main() {
  unsigned words, base, d, negative;
  char hex[80];
  std::vector<u32> digits;
  while (scanf("%u %u %u %u %79s", &words, &base, &d, &negative, hex) == 5) {
    const size_t len = strlen(hex);
    if ((words != 4 && words != 8) || base < 2 || base > 255 || len > 8 * words) { fprintf(stderr, "bad line\n"); return 2; }
    u32 s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < len; i++) {
      const char c = hex[len - 1 - i];
      const u32 v = c >= '0' && c <= '9' ? (u32)(c - '0') : c >= 'a' && c <= 'f' ? (u32)(c - 'a' + 10) : 16u;
      if (v > 15) { fprintf(stderr, "bad digit\n"); return 2; }
      s[i / 8] |= v << (4 * (i % 8));
    }
    digits.clear();
    const bool left = words == 4 ? walk<4>(s, negative != 0, base, d, digits) : walk<8>(s, negative != 0, base, d, digits);
    for (u32 dg : digits) printf("%u ", dg);
    printf("%d\n", left ? 1 : 0);
  }
  return 0;
}
