// key_range.h — the number of keys in a closed int64 interval (host only).
//
// Dense arrays and bitmaps over a key column's [min, max] are sized by
// max - min + 1.  In int64 the subtraction overflows once the interval is wider
// than 2^63 - 1, and the + 1 wraps to 0 for [INT64_MIN, INT64_MAX]: a width
// of 0 then passes every "small enough" test.  The width is formed in uint64_t
// and the one interval it cannot hold is reported as `wide`.
#pragma once
#include <cstdint>

namespace capf {

struct KeyRange {
  uint64_t n;  // keys in [lo, hi]; 0 when lo > hi (no key); UINT64_MAX when wide
  bool wide;   // [lo, hi] holds 2^64 keys (n saturates)
};

inline KeyRange key_range(int64_t lo, int64_t hi) {
  if (lo > hi) return KeyRange{0, false};
  const uint64_t d = (uint64_t)hi - (uint64_t)lo;  // exact: 0 ≤ hi − lo < 2^64
  if (d == UINT64_MAX) return KeyRange{UINT64_MAX, true};
  return KeyRange{d + 1, false};
}

// Do the keys of [lo, hi] number at most `limit` (and at least one)?
inline bool key_range_fits(int64_t lo, int64_t hi, uint64_t limit) {
  const KeyRange r = key_range(lo, hi);
  return !r.wide && r.n > 0 && r.n <= limit;
}

}  // namespace capf
