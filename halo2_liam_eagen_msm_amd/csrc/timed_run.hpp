// One timed section of a stream: event 0, the launches, event 1, the read-back copies, synchronise, elapsed time.
//
// The guarantee: every exit synchronises the stream before it returns, the error exits too -- what the section (or the
// caller before it) enqueued reads and writes host objects that die when the caller returns.  On an error exit the first
// error stands and the status of that synchronisation is dropped.
//
// Host-only: the stream is reached through a small `Q` policy (record / last_error / sync / elapsed, each returning a
// status, 0 = ok), so the same code runs on a HIP stream (HipTimedQueue in lemsm.hip) and on a fake that fails its n-th
// call (tests/timed_run_check.cpp).
#pragma once

namespace lemsm {

template <class Q, class Launch, class ReadBack>
int timed_run(Q& q, double& ms, Launch&& launch, ReadBack&& read_back) {
  int rc = q.record(0);
  if (!rc) { launch(); rc = q.last_error(); }
  if (!rc) rc = q.record(1);
  if (!rc) rc = read_back();          // enqueues the device-to-host copies of results and error words (may do nothing)
  const int s = q.sync(rc == 0);      // (false: an error is standing already, this status and its message are dropped)
  if (!rc) rc = s;
  if (!rc) rc = q.elapsed(ms);
  return rc;
}

}  // namespace lemsm
