// The row of an element of a CSR-shaped LIST column, and the typed copy of one
// element: shared by the list-function fill (lists.hip::k_lfn_fill) and the
// lambda kernels (kernels_basic.hip::k_lam_pred / k_lam_map), which divide
// their work by element and find each tile's row window with one wave-wide
// search.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "capf_internal.h"

namespace capf {

// element i of source view c as the result's element type into slot d
__device__ inline void lfn_store(const ColView &c, int64_t i, int32_t elem, void *child, uint8_t *cvalid, int64_t d) {
  const bool ok = c.type != CAPF_TYPE_NULL && c.data && !(c.valid && !c.valid[i]);
  if (elem == CAPF_TYPE_BOOL) {
    ((uint8_t *)child)[d] = ok && ((const uint8_t *)c.data)[i] ? 1 : 0;
  } else if (elem == CAPF_TYPE_FLOAT64) {
    ((double *)child)[d] = !ok ? 0.0 : c.type == CAPF_TYPE_FLOAT64 ? ((const double *)c.data)[i] : (double)ld_int(c, i);
  } else {
    ((int64_t *)child)[d] = ok ? ld_int(c, i) : 0;
  }
  if (cvalid) cvalid[d] = ok ? 1 : 0;
}

// the last r in [lo, hi] with off[r] <= o (off[lo] <= o holds)
__device__ inline int64_t lfn_row_of(const int64_t *off, int64_t lo, int64_t hi, int64_t o) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= o) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The same over [0, n - 1] by one whole wave, 64 probes per round (lane = the
// caller's lane; every lane returns the row): a tile's first and last rows
// cost log64(n) dependent loads instead of log2(n).  The offsets ascend, so
// the probes that hold are a prefix of the lanes and their count is the answer.
__device__ inline int64_t lfn_row_of_wave(const int64_t *off, int64_t n, int64_t o, int lane) {
  int64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const int64_t step = (hi - lo + 63) / 64;  // the candidates lo + 1 .. hi in 64 runs of `step`
    const int64_t idx = lo + 1 + (int64_t)lane * step;
    const bool le = idx <= hi && off[idx] <= o;
    const int c = __popcll(__ballot(le));
    if (c == 0) {
      hi = lo;
    } else {
      lo += 1 + (int64_t)(c - 1) * step;
      hi = lo + step - 1 < hi ? lo + step - 1 : hi;
    }
  }
  return lo;
}

}  // namespace capf
