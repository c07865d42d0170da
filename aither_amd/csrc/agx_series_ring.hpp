// agx_series_ring.hpp -- the arithmetic of the time-series record (agx_series.hpp): a ring of
// `capacity` row slots of which `count` are in use, the oldest in slot `head`.  A sample takes
// slot (head + count) % capacity, a drop of n rows moves head on by n; so a run samples,
// collects and drops for ever in the memory the plan allocated, and the rows recorded after a
// drop wrap around.  Chronological order is head, head + 1 ... modulo capacity: at most two
// contiguous runs of slots.  Nothing here names HIP (tests/cpp/series_ring.cpp runs it under
// the host sanitizers).
#pragma once

namespace agx {

struct SeriesRing {
  long capacity = 0, head = 0, count = 0;

  void reset(long cap) { capacity = cap; head = count = 0; }
  bool full() const { return count == capacity; }
  // the slot the next sample writes; the caller has seen !full()
  long next() const {
    const long s = head + count;
    return s >= capacity ? s - capacity : s;
  }
  void push() { ++count; }
  // the slot of row r in chronological order, 0 <= r < count
  long slot(long r) const {
    const long s = head + r;
    return s >= capacity ? s - capacity : s;
  }
  // drops the oldest n rows; false (and nothing changed) unless 0 <= n <= count
  bool drop(long n) {
    if (n < 0 || n > count) return false;
    head = slot(n);
    count -= n;
    if (count == 0) head = 0;     // (an empty ring starts over at slot 0)
    return true;
  }
  // the rows oldest first as two runs of slots: n0 from slot head, then n1 from slot 0
  void runs(long* n0, long* n1) const {
    const long to_end = capacity - head;
    *n0 = count < to_end ? count : to_end;
    *n1 = count - *n0;
  }
};

}  // namespace agx
