// The workspace arena helper (csrc/arena.hpp) driven on a host buffer: no GPU, no Python.
//   1. with guards off the offsets and the total equal the plain align_up chain the helper replaced;
//   2. with guards on every sub-buffer is followed by at least 256 bytes that fill() patterns and nothing else owns;
//   3. one flipped byte in zone i is reported with sub-buffer i's name and the byte's offset, an intact arena as clean.
// Built by tests/test_host_logic.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../halo2_liam_eagen_msm_amd/csrc/arena.hpp"

using namespace lemsm::arena;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "arena check failed at line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

struct Req { const char* name; size_t bytes, slack; };

static size_t au(size_t x, size_t a) { return (x + a - 1) / a * a; }

static void run(const std::vector<Req>& reqs, size_t align) {
  // 1. guards off: the plain chain
  {
    Arena a("plain", false, align);
    size_t off = 0, end = 0;
    for (const Req& r : reqs) {
      CHECK(a.take(r.name, r.bytes, r.slack) == off);
      end = off + r.bytes + r.slack; off = au(end, align);
    }
    CHECK(a.total() == off && a.end() == end && a.zones().empty());
    ArenaHostMem m; std::string msg;
    CHECK(a.fill(m, nullptr) && a.check(m, nullptr, msg) == 0);
  }
  // 2. guards on
  Arena a("host", true, align);
  std::vector<size_t> offs;
  for (const Req& r : reqs) offs.push_back(a.take(r.name, r.bytes, r.slack));
  CHECK(a.zones().size() == reqs.size());
  CHECK(a.total() % align == 0 && a.end() <= a.total());
  for (size_t i = 0; i < reqs.size(); i++) {
    const size_t g = a.zones()[i].off, next = i + 1 < reqs.size() ? offs[i + 1] : a.total();
    CHECK(offs[i] % align == 0);
    CHECK(a.zones()[i].name == reqs[i].name);
    CHECK(g == au(offs[i] + reqs[i].bytes, 16));              // directly behind the bytes, as carve() places it
    CHECK(g + WS_GUARD_BYTES <= next);                         // at least 256 bytes before anything else starts
  }
  std::vector<char> buf(a.total() + 1, 0x11);                  // (+ 1: a zero-size arena still has an address)
  ArenaHostMem m; std::string msg;
  CHECK(a.fill(m, buf.data()));
  for (size_t i = 0; i < reqs.size(); i++) {
    for (size_t k = 0; k < reqs[i].bytes; k++) CHECK(buf[offs[i] + k] == 0x11);                        // fill leaves the payload alone
    for (size_t k = 0; k < WS_GUARD_BYTES; k++) CHECK((unsigned char)buf[a.zones()[i].off + k] == WS_GUARD_PATTERN);
  }
  CHECK(a.check(m, buf.data(), msg) == 0 && msg.empty());
  // writing every payload byte damages no zone
  for (size_t i = 0; i < reqs.size(); i++) for (size_t k = 0; k < reqs[i].bytes; k++) buf[offs[i] + k] = 0x22;
  CHECK(a.check(m, buf.data(), msg) == 0);
  // 3. one flipped byte
  const size_t ks[] = {0, 1, 100, WS_GUARD_BYTES - 1};
  for (size_t i = 0; i < reqs.size(); i++)
    for (size_t k : ks) {
      char& c = buf[a.zones()[i].off + k];
      c ^= 0x40;
      msg.clear();
      CHECK(a.check(m, buf.data(), msg) == 1);
      const std::string want = std::string("workspace guard host/") + reqs[i].name + " overwritten at byte " + std::to_string(k) + " (option ws_canary)";
      if (msg != want) { fprintf(stderr, "got  '%s'\nwant '%s'\n", msg.c_str(), want.c_str()); exit(1); }
      c ^= 0x40;
      CHECK(a.check(m, buf.data(), msg) == 0);
    }
  // two damaged zones: the first is the one reported
  if (reqs.size() >= 2) {
    buf[a.zones()[1].off + 7] = 0; buf[a.zones()[0].off + 9] = 0;
    CHECK(a.check(m, buf.data(), msg) == 1);
    CHECK(msg == std::string("workspace guard host/") + reqs[0].name + " overwritten at byte 9 (option ws_canary)");
  }
}

int main() {
  run({{"a", 1, 0}}, 256);
  run({{"a", 0, 0}, {"b", 0, 16}, {"c", 5, 0}}, 256);
  run({{"coef", 4096, 0}, {"lens", 8, 0}, {"fbuf", 32 * 1024, 256}, {"stats", 256, 0}, {"exc", 4 * 14, 256}}, 256);
  run({{"jac", 37 * 96, 16}, {"table", 37 * 15 * 64, 16}, {"scratch", 37 * 15 * 160, 256}}, 256);
  run({{"x", 255, 0}, {"y", 256, 0}, {"z", 257, 1}, {"w", 241, 15}, {"v", 17, 512}, {"u", 3, 4096}}, 256);
  run({{"p", 100, 0}, {"q", 33, 16}, {"r", 1, 0}}, 64);
  printf("arena ok\n");
  return 0;
}
