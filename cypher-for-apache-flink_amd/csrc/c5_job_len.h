// Job lengths of the indexed 2-hop count's units (k_c5_gather<…, IDX>): how an
// out-run of `nt` tiles holding T pieces is cut into jobs, given the mean run's
// pieces M, the jobs J a mean run is cut into (W = M / J pieces per job), the
// excess split X and the shortest job min_tiles.  Host and device: the kernel
// and the host-side check (capf_c5_job_len) run the same arithmetic.
//
// The plain rule: k = round(T / W) equal ranges of ⌈nt / k⌉ tiles.
// The two-zone rule (X > 0 and T − M ≥ W / X, one crumb's weight): the first
// B = ⌈nt · M / T⌉ tiles — those holding a mean run's work, work per tile taken
// as uniform within a run — are cut into J base jobs like any mean run's; the
// rest, the part of the run ABOVE the mean, into round((T − M) / (W / X))
// crumbs, X to the weight of a base job.  Only a heavy run pays for fine jobs,
// and only on its excess: the units that end early take the crumbs while the
// owner is still on its base jobs' successors.
// No length is 0, and none is below min_tiles unless the run itself is shorter.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define C5_JOB_LEN_FN __host__ __device__ inline
#else
#define C5_JOB_LEN_FN inline
#endif

namespace capf {

struct C5JobLens {
  uint32_t base;   // length of a job that starts in [0, zone)
  uint32_t crumb;  // length of a job that starts in [zone, nt); 0: one zone, every job is `base` long
  uint32_t zone;   // J · base (≥ B) when crumb > 0
};

// W = 0: the rule is off, every job is min_tiles long.
C5_JOB_LEN_FN C5JobLens c5_job_lens(uint32_t T, uint32_t W, uint32_t J, uint32_t X, uint32_t nt, uint32_t min_tiles) {
  const uint32_t lo = min_tiles ? min_tiles : 1u;
  const uint32_t cap = nt ? nt : 1u;
  C5JobLens l{lo < cap ? lo : cap, 0u, 0u};
  if (!W) return l;
  const uint64_t M = (uint64_t)W * (J ? J : 1u);
  if (X && J && T > M && (uint64_t)(T - M) * X >= W) {
    const uint64_t B = ((uint64_t)nt * M + T - 1) / T;  // ≤ nt
    uint32_t base = (uint32_t)((B + J - 1) / J);
    base = base < lo ? lo : base;
    const uint64_t zone = (uint64_t)J * base;
    if (zone < nt) {
      const uint32_t rest = nt - (uint32_t)zone;
      const uint64_t nc64 = ((uint64_t)(T - M) * X + W / 2) / W;
      const uint32_t nc = nc64 < 1 ? 1u : nc64 > rest ? rest : (uint32_t)nc64;
      uint32_t crumb = (rest + nc - 1) / nc;
      crumb = crumb < lo ? lo : crumb;
      l.base = base;
      l.crumb = crumb;
      l.zone = (uint32_t)zone;
      return l;
    }
  }
  const uint64_t k64 = ((uint64_t)T + W / 2) / W;
  const uint32_t k = k64 < 1 ? 1u : k64 > nt ? (nt ? nt : 1u) : (uint32_t)k64;
  const uint32_t jt = (nt + k - 1) / k;
  l.base = jt < lo ? lo : jt;
  l.base = l.base < cap ? l.base : cap;
  return l;
}

// What a taker does with the two stored lengths and a (possibly stale) cursor
// position: any choice gives disjoint covering ranges, the position only steers
// the sizes.  base = 0 (the owner has not stored it yet): min_tiles.
C5_JOB_LEN_FN uint32_t c5_job_pick(uint32_t base, uint32_t crumb, uint32_t J, uint32_t min_tiles, uint32_t pos) {
  if (!base) return min_tiles ? min_tiles : 1u;
  return crumb && (uint64_t)pos >= (uint64_t)J * base ? crumb : base;
}

// The length of the job a taker claims that read the cursor at `pos`.
C5_JOB_LEN_FN uint32_t c5_job_len(uint32_t T, uint32_t M, uint32_t J, uint32_t X, uint32_t nt, uint32_t min_tiles,
                                  uint32_t pos) {
  const uint32_t W = J ? (M / J ? M / J : 1u) : 0u;
  const C5JobLens l = c5_job_lens(T, W, J, X, nt, min_tiles);
  return c5_job_pick(l.base, l.crumb, J, min_tiles, pos);
}

}  // namespace capf
