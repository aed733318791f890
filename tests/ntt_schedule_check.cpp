// The pass schedule of a transform (csrc/ntt_schedule.hpp) for every logN from 0 to 28 and both directions: the passes cover
// every stage exactly once, one contiguous pass of min(logN, 10) stages and strided passes of at most 8, the forward list
// is the inverse list reversed, and the count is the closed form the plans have always reported.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/ntt_schedule_check.cpp -o ntt_schedule_check && ./ntt_schedule_check
#include <cstdio>
#include <cstdlib>

#include "../halo2_liam_eagen_msm_amd/csrc/ntt_schedule.hpp"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s (logN %u)\n", __FILE__, __LINE__, #c, logN); exit(1); } } while (0)

using lemsm::ntt::Pass;
using lemsm::ntt::Schedule;

// what the plans and the *_last figures counted before the schedule had a header of its own
static unsigned closed_form(unsigned logN) { return 1 + (logN > 10 ? (logN - 10 + 7) / 8 : 0); }

int main() {
  for (unsigned logN = 0; logN <= 28; logN++) {
    const Schedule inv = lemsm::ntt::schedule(logN, true), fwd = lemsm::ntt::schedule(logN, false);
    REQUIRE(inv.count == closed_form(logN) && fwd.count == inv.count && lemsm::ntt::passes(logN) == inv.count);
    REQUIRE(inv.count <= sizeof inv.pass / sizeof inv.pass[0]);
    unsigned seen[32] = {0}, contiguous = 0;
    for (unsigned i = 0; i < inv.count; i++) {
      const Pass& p = inv.pass[i];
      const Pass& q = fwd.pass[fwd.count - 1 - i];                     // forward: the same list reversed
      REQUIRE(p.lo == q.lo && p.S == q.S && p.strided == q.strided);
      REQUIRE(p.lo + p.S <= logN);
      for (unsigned s = p.lo; s < p.lo + p.S; s++) seen[s]++;
      if (!p.strided) { contiguous++; REQUIRE(p.lo == 0 && p.S == (logN < 10 ? logN : 10)); }
      else REQUIRE(p.S >= 1 && p.S <= 8 && p.lo >= 10);               // (a strided block owns 1024 elements: never below stage 10)
      if (i) REQUIRE(p.lo == inv.pass[i - 1].lo + inv.pass[i - 1].S);  // inverse: ascending, no gap
    }
    REQUIRE(contiguous == 1 && !inv.pass[0].strided);                  // inverse: the contiguous pass first
    for (unsigned s = 0; s < 32; s++) REQUIRE(seen[s] == (s < logN ? 1u : 0u));
  }
  // the smallest sizes: one contiguous pass over no stage (logN 0: priced, never launched) and over stage 0 alone
  for (int inverse = 0; inverse < 2; inverse++) {
    unsigned logN = 0;
    Schedule s = lemsm::ntt::schedule(logN, inverse != 0);
    REQUIRE(s.count == 1 && s.pass[0].lo == 0 && s.pass[0].S == 0 && !s.pass[0].strided);
    logN = 1;
    s = lemsm::ntt::schedule(logN, inverse != 0);
    REQUIRE(s.count == 1 && s.pass[0].lo == 0 && s.pass[0].S == 1 && !s.pass[0].strided);
  }
  printf("ntt schedule ok\n");
  return 0;
}
