// The ring log's arithmetic (csrc/mbd_ring.h, included as it is) over every combination of cap in 1..5, count in 0..3 cap + 1 and
// n in 0..cap + 2: empty, unwrapped, exactly full, wrapped once, wrapped twice, n beyond both bounds.  Entry j = j is written at
// j % cap for j < count; what the runs read must be count - n' .. count - 1 with n' = min(n, count, cap), stated naively.
#include <cstdio>
#include <vector>

#include "mbd_ring.h"

int main() {
  long long cases = 0, bad = 0;
  for (long long cap = 1; cap <= 5; ++cap)
    for (long long count = 0; count <= 3 * cap + 1; ++count)
      for (long long n = 0; n <= cap + 2; ++n) {
        std::vector<long long> ring((size_t)cap, -1), want, got;
        for (long long j = 0; j < count; ++j) ring[(size_t)(j % cap)] = j;
        long long np = n;
        if (np > count) np = count;
        if (np > cap) np = cap;
        for (long long j = count - np; j < count; ++j) want.push_back(j);
        const RingRuns r = ring_recent(count, cap, n);
        bool ok = r.n == np && r.len[0] + r.len[1] == r.n;
        for (int i = 0; i < 2 && ok; ++i) {
          ok = r.len[i] >= 0 && r.first[i] >= 0 && r.first[i] + r.len[i] <= cap;  // (a run stays inside the ring)
          for (long long e = 0; e < r.len[i] && ok; ++e) got.push_back(ring[(size_t)(r.first[i] + e)]);
        }
        ok = ok && got == want;
        ++cases;
        if (!ok) {
          ++bad;
          printf("MISMATCH cap=%lld count=%lld n=%lld: n'=%lld runs (%lld,%lld) (%lld,%lld)\n", cap, count, n, r.n, r.first[0], r.len[0],
                 r.first[1], r.len[1]);
        }
      }
  printf("%lld combinations, %lld mismatches\n", cases, bad);
  return bad ? 1 : 0;
}
