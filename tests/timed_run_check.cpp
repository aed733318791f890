// The timed section of the witness entries (csrc/timed_run.hpp) on a fake stream: whichever call fails, the stream has been
// synchronised when the helper returns, the first error is the one returned, and the order of the calls is
// record 0, launch, last_error, record 1, read_back, sync, elapsed.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/timed_run_check.cpp -o timed_run_check && ./timed_run_check
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../halo2_liam_eagen_msm_amd/csrc/timed_run.hpp"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

// Every stream-facing call takes a number (from 1); call `fail_at` returns its own number as the status.
struct FakeQueue {
  int fail_at, calls = 0;
  std::string log;
  bool synced = true;        // nothing is in flight
  bool kept_last = true;     // the last sync was asked to keep its status
  int step(char what) { log += what; return ++calls == fail_at ? calls : 0; }
  int record(int i) { synced = false; return step(i ? 'R' : 'r'); }
  int last_error() { return step('e'); }
  int sync(bool keep) { synced = true; kept_last = keep; return step('s'); }
  int elapsed(double& ms) { const int rc = step('t'); if (!rc) ms = 1.5; return rc; }
};

int main() {
  const std::string full = "rLeRBst";
  for (int fail_at = 0; fail_at <= 7; fail_at++) {   // 0 and 7: nothing fails (six numbered calls)
    FakeQueue q{fail_at};
    double ms = -1;
    auto launch = [&] { q.synced = false; q.log += 'L'; };
    auto read_back = [&] { q.synced = false; return q.step('B'); };   // (the read-back is call 4: it can fail too)
    const int rc = lemsm::timed_run(q, ms, launch, read_back);
    const bool fails = fail_at >= 1 && fail_at <= 6;
    REQUIRE(rc == (fails ? fail_at : 0));                              // the first error stands
    REQUIRE(q.synced);                                                 // never work in flight on return
    REQUIRE(q.log.find('s') != std::string::npos);
    if (!fails) { REQUIRE(q.log == full);   /* the order of the success path */ REQUIRE(ms == 1.5); REQUIRE(q.kept_last); }
    else REQUIRE(ms == -1);
    if (fails && fail_at <= 4) REQUIRE(!q.kept_last);                  // an error was standing: the sync's status is dropped
    // nothing runs behind a failed call but the synchronise (and nothing behind a failed synchronise)
    const std::string want[7] = {"", "rs", "rLes", "rLeRs", "rLeRBs", "rLeRBs", "rLeRBst"};
    if (fails) REQUIRE(q.log == want[fail_at]);
  }
  printf("timed_run ok\n");
  return 0;
}
