// mbd_ring.h — the arithmetic of a ring log (a pick record's ticks, an adapt and an elite record's steps): entry j lies at
// j % cap, so the log holds the most recent cap entries.  Pure integer code that includes nothing: mbd_internal.h builds the
// device reader on it (ring_read), tests/ring_host.cpp compiles it for the host alone and checks it over every small case.
#pragma once

// The most recent n entries of a ring of `cap` slots that has seen `count` entries, oldest first: n = min(wanted, count, cap)
// of them, as at most two runs of slots — first[0] .. first[0] + len[0] - 1, then, where the ring wraps between two of them,
// first[1] = 0 .. len[1] - 1.  A run that is not needed has len 0; cap < 1 or a negative argument: nothing.
struct RingRuns {
  long long n, first[2], len[2];
};
inline RingRuns ring_recent(long long count, long long cap, long long wanted) {
  long long n = wanted < count ? wanted : count;
  if (n > cap) n = cap;
  if (n <= 0) return RingRuns{0, {0, 0}, {0, 0}};
  const long long first = (count - n) % cap, len0 = n < cap - first ? n : cap - first;
  return RingRuns{n, {first, 0}, {len0, n - len0}};
}
