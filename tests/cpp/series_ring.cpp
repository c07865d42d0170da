// The ring arithmetic of the time-series record (aither_amd/csrc/agx_series_ring.hpp) under
// the address and undefined-behaviour sanitizers: a record of `capacity` slots is sampled,
// collected and dropped at random beside a std::deque that holds the truth; the slot of every
// sample lies inside the ring and is not in use, and the chronological unroll -- row by row
// and as the two runs a collect copies -- is the deque, oldest first.
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>

#include "../../aither_amd/csrc/agx_series_ring.hpp"

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("series_ring: %s failed at line %d\n", #cond, __LINE__);   \
      return 1;                                                              \
    }                                                                        \
  } while (0)

static unsigned long long g_seed = 0x9e3779b97f4a7c15ULL;
static unsigned rnd(unsigned n) {
  g_seed = g_seed * 6364136223846793005ULL + 1442695040888963407ULL;
  return (unsigned)((g_seed >> 33) % n);
}

static int check(const agx::SeriesRing& ring, const std::vector<double>& store,
                 const std::deque<double>& truth) {
  REQUIRE(ring.count == (long)truth.size());
  REQUIRE(ring.head >= 0 && ring.head < ring.capacity);
  for (long r = 0; r < ring.count; ++r) REQUIRE(store[(size_t)ring.slot(r)] == truth[(size_t)r]);
  long n0, n1;
  ring.runs(&n0, &n1);
  REQUIRE(n0 >= 0 && n1 >= 0 && n0 + n1 == ring.count);
  REQUIRE(ring.head + n0 <= ring.capacity && n1 <= ring.head);
  std::vector<double> unrolled;
  for (long r = 0; r < n0; ++r) unrolled.push_back(store[(size_t)(ring.head + r)]);
  for (long r = 0; r < n1; ++r) unrolled.push_back(store[(size_t)r]);
  for (size_t r = 0; r < truth.size(); ++r) REQUIRE(unrolled[r] == truth[r]);
  return 0;
}

int main() {
  // the sequence of the device test: capacity 3, three samples, full, drop 2, two more
  {
    agx::SeriesRing ring;
    ring.reset(3);
    std::vector<double> store(3, -1.0);
    std::deque<double> truth;
    for (int t = 0; t < 3; ++t) {
      REQUIRE(!ring.full());
      store[(size_t)ring.next()] = t; ring.push(); truth.push_back(t);
    }
    REQUIRE(ring.full());
    REQUIRE(!ring.drop(4) && !ring.drop(-1) && ring.count == 3);
    REQUIRE(ring.drop(2));
    truth.pop_front(); truth.pop_front();
    for (int t = 3; t < 5; ++t) {
      REQUIRE(!ring.full());
      store[(size_t)ring.next()] = t; ring.push(); truth.push_back(t);
    }
    REQUIRE(ring.full() && ring.head == 2);       // wrapped: rows 2, 3, 4 in slots 2, 0, 1
    if (check(ring, store, truth)) return 1;
    REQUIRE(ring.drop(3) && ring.count == 0 && ring.head == 0);
  }
  // random histories at many capacities
  for (long cap = 1; cap <= 17; ++cap) {
    agx::SeriesRing ring;
    ring.reset(cap);
    std::vector<double> store((size_t)cap, -1.0);
    std::vector<char> used((size_t)cap, 0);
    std::deque<double> truth;
    double t = 0.0;
    for (int step = 0; step < 4000; ++step) {
      if (rnd(3) != 0) {
        if (ring.full()) {
          REQUIRE((long)truth.size() == cap);
        } else {
          const long s = ring.next();
          REQUIRE(s >= 0 && s < cap && !used[(size_t)s]);
          store[(size_t)s] = t; used[(size_t)s] = 1;
          ring.push(); truth.push_back(t);
          t += 1.0;
        }
      } else {
        const long n = (long)rnd((unsigned)cap + 2);
        const bool ok = n <= (long)truth.size();
        std::vector<long> slots;
        for (long r = 0; r < n && ok; ++r) slots.push_back(ring.slot(r));
        REQUIRE(ring.drop(n) == ok);
        if (ok) {
          for (long s : slots) used[(size_t)s] = 0;
          truth.erase(truth.begin(), truth.begin() + n);
        }
      }
      if (check(ring, store, truth)) return 1;
    }
  }
  std::printf("series_ring OK\n");
  return 0;
}
