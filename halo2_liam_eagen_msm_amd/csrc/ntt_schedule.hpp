// The passes over HBM of one batched transform of 2^logN elements, in launch order.  Stage s is the butterfly of span 2^s.
// One contiguous pass covers stages 0 .. min(logN, 10) - 1 in LDS tiles of 1024 consecutive elements; the stages above go
// in strided passes of at most 8.  An inverse transform (decimation in time) runs the contiguous pass, then the strided
// ones upwards; a forward transform (decimation in frequency) the same list reversed.  logN = 0 gives the contiguous pass
// alone, over no stage: a transform of one element is priced, and laid out, as one pass.
//
// Host-only: dw_ntt and poly_ntt launch k_ntt_tile from this list, the plans and the *_last figures count it
// (tests/ntt_schedule_check.cpp).
#pragma once

namespace lemsm { namespace ntt {

struct Pass { unsigned lo, S; bool strided; };       // stages lo .. lo + S - 1
struct Schedule { Pass pass[8]; unsigned count; };   // (8 passes: logN < 64)

inline Schedule schedule(unsigned logN, bool inverse) {
  Schedule s;
  s.pass[0] = Pass{0, logN < 10 ? logN : 10, false};
  s.count = 1;
  for (unsigned lo = s.pass[0].S; lo < logN; lo += 8) s.pass[s.count++] = Pass{lo, logN - lo < 8 ? logN - lo : 8, true};
  if (!inverse) for (unsigned i = 0, j = s.count - 1; i < j; i++, j--) { const Pass t = s.pass[i]; s.pass[i] = s.pass[j]; s.pass[j] = t; }
  return s;
}
inline unsigned passes(unsigned logN) { return schedule(logN, true).count; }

}}  // namespace lemsm::ntt
