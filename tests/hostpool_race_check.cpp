// CPU-only check of the host worker pool (halo2_liam_eagen_msm_amd/csrc/hostpool.hpp) used the way contexts use it: several
// host threads, each the only caller of a Pool of its own, all running at once.  Built with -fsanitize=thread by
// tests/test_host_logic.py.  No GPU, no HIP.  Every run() is checked for "each index exactly once" and for the visibility of
// the jobs' PLAIN (non-atomic) writes after run() returns -- the happens-before edge that the done_ release / acquire pair
// gives and that ThreadSanitizer reports as a data race when it is missing.  One leg drives the per-window fold of
// hosttail.hpp (window_sum, as lemsm.hip's window_sums_par does) through the pools of two such threads on synthetic records
// and compares with the serial fold.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <thread>
#include <vector>

#include "../halo2_liam_eagen_msm_amd/csrc/hostpool.hpp"
#include "../halo2_liam_eagen_msm_amd/csrc/hosttail.hpp"

using namespace lemsm;

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); exit(1); } \
  } while (0)

// ---- each host thread its own pool: indices once, plain writes visible ------------------------------------
void pool_owner(int id, int workers, int runs) {
  std::mt19937_64 rng(1000 + id);
  host::Pool pool(workers);
  CHECK(pool.workers() == workers);
  // job counts: 0, 1, fewer than / as many as / more than the workers + caller, and random ones up to 64
  const int fixed[] = {0, 1, 2, workers, workers + 1, workers + 2, 4 * workers + 3, 64};
  std::vector<int> hits;            // plain ints, written by whichever thread takes the index
  std::vector<unsigned long long> val;
  for (int r = 0; r < runs; r++) {
    const int n = r < 8 ? fixed[r] : (int)(rng() % 65);
    hits.assign(n, 0); val.assign(n, 0);
    const unsigned long long salt = rng();
    pool.run(n, [&](int i) { hits[i]++; val[i] = salt ^ (unsigned long long)i * 0x9e3779b97f4a7c15ULL; });
    for (int i = 0; i < n; i++) {
      CHECK(hits[i] == 1);
      CHECK(val[i] == (salt ^ (unsigned long long)i * 0x9e3779b97f4a7c15ULL));
    }
  }
}

// ---- the per-window fold through the pool, from two host threads at once ----------------------------------
// a point with known discrete log: k * G, G = (1, 2) on y^2 = x^3 + 3 (BN254 G1)
host::pt generator() {
  typedef host::HF<host::FqParams64> F;
  host::pt g; g.x = F::one();
  host::fe y = {{2, 0, 0, 0}}, r2; memcpy(r2.l, host::FqParams64::R2, 32);
  g.y = F::mul(y, r2);              // canonical -> Montgomery
  g.zz = F::one(); g.zzz = F::one();
  return g;
}

void fold_owner(int id, int workers, int rounds, int* mismatches) {
  typedef host::FqParams64 P;
  typedef host::HG<P> G;
  std::mt19937_64 rng(2000 + id);
  const host::pt g = generator();
  host::Pool pool(workers);
  int bad = 0;
  for (int r = 0; r < rounds; r++) {
    const u32 L = 1 + (u32)(rng() % 8), nw = 1 + (u32)(rng() % 24);    // windows: below, at and above the pool's size
    std::vector<host::pt> recs((size_t)nw * (L + 1));
    for (auto& p : recs) { u32 k = (u32)(rng() % 1000); p = k ? G::mul_small(g, k) : G::identity(); }
    std::vector<host::pt> serial(nw), par(nw);
    for (u32 w = 0; w < nw; w++) serial[w] = window_sum<P>(recs.data() + (size_t)w * (L + 1), L);
    pool.run((int)nw, [&](int w) { par[w] = window_sum<P>(recs.data() + (size_t)w * (L + 1), L); });
    for (u32 w = 0; w < nw; w++) {
      u64 a[8], b[8]; G::to_affine(serial[w], a); G::to_affine(par[w], b);
      if (memcmp(a, b, 64) != 0) bad++;
    }
    // and the serial Horner over them, as the call's last step
    u64 o1[12], o2[12];
    msm_combine_windows<P>(3, nw, serial.data(), o1); msm_combine_windows<P>(3, nw, par.data(), o2);
    if (memcmp(o1, o2, 96) != 0) bad++;
  }
  *mismatches = bad;
}

int main(int argc, char** argv) {
  const int runs = argc > 1 ? atoi(argv[1]) : 2000;
  {
    const int workers[] = {3, 3, 0, 1, 7, 3};
    std::vector<std::thread> th;
    for (int t = 0; t < 6; t++) th.emplace_back(pool_owner, t, workers[t], runs);
    for (auto& t : th) t.join();
  }
  {
    int bad[2] = {-1, -1};
    std::thread a(fold_owner, 0, 3, 40, &bad[0]), b(fold_owner, 1, 2, 40, &bad[1]);
    a.join(); b.join();
    CHECK(bad[0] == 0 && bad[1] == 0);
  }
  // pools created and destroyed beside running ones (a context created / closed while another is mid-call)
  {
    std::thread a(pool_owner, 10, 3, runs / 4);
    for (int k = 0; k < 20; k++) pool_owner(20 + k, 2, 10);
    a.join();
  }
  printf("hostpool race check ok\n");
  return 0;
}
