// civil_date.h — proleptic Gregorian calendar arithmetic shared by the temporal
// opcodes (kernels_basic.hip) and the typed CSV parser (edge_list.hip).
//
// 32-bit arithmetic with divisions by constants only: no loop over years or
// months and no table.  Values outside years 0001-9999 give unspecified
// results (never an access: nothing here reads memory).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace capf {

constexpr int64_t MICROS_PER_DAY = 86400000000ll;

struct Civil {
  int32_t y, m, d;
};

__device__ inline int32_t floor_div(int32_t a, int32_t b) { return (a >= 0 ? a : a - (b - 1)) / b; }
__device__ inline bool leap_year(int32_t y) { return (y & 3) == 0 && (y % 100 != 0 || y % 400 == 0); }

// Day number → civil date by the era / day-of-era method: eras of 400 years
// (146 097 days) from 0000-03-01, the year beginning in March so the leap day
// is its last.
__device__ inline Civil civil_from_days(int32_t z) {
  z += 719468;  // days from 0000-03-01 to 1970-01-01
  const int32_t era = floor_div(z, 146097);
  const uint32_t doe = (uint32_t)(z - era * 146097);                           // [0, 146096]
  const uint32_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;  // [0, 399]
  const uint32_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);                // [0, 365], from March 1
  const uint32_t mp = (5 * doy + 2) / 153;                                     // [0, 11], March = 0
  Civil c;
  c.d = (int32_t)(doy - (153 * mp + 2) / 5 + 1);
  c.m = (int32_t)(mp < 10 ? mp + 3 : mp - 9);
  c.y = (int32_t)yoe + era * 400 + (c.m <= 2 ? 1 : 0);
  return c;
}

__device__ inline int32_t days_from_civil(int32_t y, int32_t m, int32_t d) {
  y -= m <= 2 ? 1 : 0;
  const int32_t era = floor_div(y, 400);
  const uint32_t yoe = (uint32_t)(y - era * 400);
  const uint32_t doy = (153u * (uint32_t)(m > 2 ? m - 3 : m + 9) + 2) / 5 + (uint32_t)d - 1;
  const uint32_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + (int32_t)doe - 719468;
}

}  // namespace capf
