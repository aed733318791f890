// Carving one device workspace into named sub-buffers, with optional guard zones (option ws_canary).
//
// A carve is a list of takes: take(name, bytes, slack) returns the sub-buffer's offset.  `bytes` is what the kernels are
// meant to touch; `slack` is room a request has always carried without a reader anybody can name.  With guards off a take
// advances by align_up(bytes + slack, align): the hand-written align_up chains this replaces, offset for offset.  With
// guards on a WS_GUARD-byte zone sits at align_up(off + bytes, 16), directly behind the bytes (the slack's place), and the
// next sub-buffer starts at the next multiple of `align` behind the zone.  fill() writes the pattern into every zone,
// check() reads the zones back and names the first damaged byte.
//
// Host-only: the memory behind the offsets is reached through a small `Mem` policy (set / get / sync), so the same code
// runs on a stream (ArenaHipMem in lemsm.hip) and on a plain host buffer (ArenaHostMem: tests/arena_check.cpp).
#pragma once
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

namespace lemsm {
namespace arena {

const size_t WS_GUARD_BYTES = 256;
const unsigned char WS_GUARD_PATTERN = 0xA5;

inline size_t align_up_sz(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct Zone { std::string name; size_t off; };   // the guard behind sub-buffer `name`

class Arena {
 public:
  Arena() {}
  Arena(const std::string& name, bool guards, size_t align = 256) : name_(name), guards_(guards), align_(align) {}

  size_t take(const char* name, size_t bytes, size_t slack = 0) {
    const size_t o = off_;
    if (guards_) {
      const size_t g = align_up_sz(off_ + bytes, 16);
      zones_.push_back(Zone{name, g});
      end_ = g + WS_GUARD_BYTES;
    } else end_ = off_ + bytes + slack;
    off_ = align_up_sz(end_, align_);
    return o;
  }
  size_t total() const { return off_; }   // the arena's size: the last take's end rounded up to `align`
  size_t end() const { return end_; }     // ... not rounded (for the requests that were never rounded)
  bool guards() const { return guards_; }
  const std::string& name() const { return name_; }
  const std::vector<Zone>& zones() const { return zones_; }

  template <class Mem>
  bool fill(Mem& m, char* base) const {
    for (const Zone& z : zones_) if (!m.set(base + z.off, WS_GUARD_PATTERN, WS_GUARD_BYTES)) return false;
    return true;
  }
  // 0: every zone intact; 1: damaged, `msg` names the first damaged byte; -1: the transport failed (its own error stands)
  template <class Mem>
  int check(Mem& m, const char* base, std::string& msg) const {
    if (zones_.empty()) return 0;
    std::vector<unsigned char> host(zones_.size() * WS_GUARD_BYTES);
    for (size_t i = 0; i < zones_.size(); i++) if (!m.get(host.data() + i * WS_GUARD_BYTES, base + zones_[i].off, WS_GUARD_BYTES)) return -1;
    if (!m.sync()) return -1;
    for (size_t i = 0; i < host.size(); i++)
      if (host[i] != WS_GUARD_PATTERN) {
        msg = "workspace guard " + name_ + "/" + zones_[i / WS_GUARD_BYTES].name + " overwritten at byte " + std::to_string(i % WS_GUARD_BYTES) + " (option ws_canary)";
        return 1;
      }
    return 0;
  }

 private:
  std::string name_;
  bool guards_ = false;
  size_t align_ = 256, off_ = 0, end_ = 0;
  std::vector<Zone> zones_;
};

struct ArenaHostMem {   // a host buffer stands in for the device
  bool set(void* p, unsigned char v, size_t n) { memset(p, v, n); return true; }
  bool get(void* dst, const void* src, size_t n) { memcpy(dst, src, n); return true; }
  bool sync() { return true; }
};

}  // namespace arena
}  // namespace lemsm
