// var_length_reach.hip — fused VarLengthExpand → DISTINCT (a, b) → GROUP BY a
// count(*) (config 5: MATCH (a:Person)-[:KNOWS*1..3]->(b:Person)
//                     WITH DISTINCT a, b WITH a, count(*) AS reach ...).
//
// The relational plan (VarLengthExpandPlanner.scala:82-259: one join per hop,
// isomorphism filter e_i ∉ {e_1..e_{i-1}} (:178-179), target join (:218-229),
// null padding + UNION ALL (:145-170)) materialises every path — ≈1e10 rows
// of 40 B at LDBC SF10 — and DISTINCT / GROUP BY (FlinkTable.scala:123-150,
// 189-196) then reduce them to one count per source.  With lower bound 1 and a
// directed pattern the DISTINCT pairs are exactly the pairs joined by a WALK
// of length 1..u (a walk repeating rel e contains the closed sub-walk between
// the two uses; cutting it keeps e once, so a walk of length ≥ 1 with the same
// endpoints and no repeated rel exists — isomorphism never changes the DISTINCT
// pairs).  So reach(a) = |{b ∈ targets : min walk length a→b ∈ [1, u]}|, the
// classic level-synchronous BFS from a with a itself NOT pre-visited.
//
// Bit-parallel multi-source BFS (MS-BFS), pull form, no atomics:
//   dict   all ids (rel endpoints, sources, targets) → sorted distinct keys
//          (rocprim radix sort + run-length encode); dense index = rank
//   CSR    in-edges by target (count, scan, fill)
//   state  visited / frontier / next: D nodes × K words of 64 source bits,
//          node-major (a node's K words are contiguous) in HBM
//   push1  level 1: rels of the batch's sources set their bits (M atomics)
//   level  levels 2..u, thread per (node y, word k): next = OR_{x ∈ in(y)} frontier[x][k]
//          & ~visited[y][k]; visited |= next  — K consecutive threads share
//          y's CSR row and read x's frontier words as one coalesced run
//   count  block per word k: wave ballots of (visited bit j ∧ target(y)),
//          popcount → reach of source 64k + j
// Sources are processed in batches of 64·K so the three state arrays stay
// within a fixed HBM budget.  Bytes per level ≈ 8·K·(M + 3·D).
//
// Lower bound ≥ 2 (≤ upper ≤ 4) is answered by trail enumeration instead:
// k_vt_trails below ("trails"); the undirected pattern (0 ≤ lower ≤ upper ≤ 4)
// by enumeration of its lowering's (node, mode) steps: k_vu_steps ("undirected
// steps").
#include <algorithm>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "capf_internal.h"
#include "device_common.h"

namespace capf {

template <class F>
static void vr_rocprim(Session *s, F &&f) {
  size_t tmp = 0;
  HIP_CHECK(f(nullptr, tmp));
  BufPtr t = s->alloc(std::max<size_t>(tmp, 16));
  HIP_CHECK(f(t->p, tmp));
}

// order-preserving uint64 key of an int64 id
__device__ inline uint64_t vr_key(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ull; }

__global__ void k_vr_keys(ColView c, int64_t n, uint64_t *out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = vr_key(ld_int(c, i));
}

// dense index of each id: lower_bound in the sorted distinct keys
__global__ void k_vr_map(ColView c, int64_t n, const uint64_t *dict, uint32_t nd, uint32_t *out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t k = vr_key(ld_int(c, i));
    uint32_t lo = 0, hi = nd;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (dict[mid] < k) lo = mid + 1;
      else hi = mid;
    }
    out[i] = lo;
  }
}

__global__ void k_vr_flag(const uint32_t *idx, int64_t n, uint8_t *flag) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    flag[idx[i]] = 1;
}

__global__ void k_vr_indeg(const uint32_t *dst, int64_t m, uint32_t *deg) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x)
    atomicAdd(&deg[dst[i]], 1u);
}

__global__ void k_vr_fill(const uint32_t *src, const uint32_t *dst, int64_t m, uint32_t *cursor,
                          uint32_t *cols) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x)
    cols[atomicAdd(&cursor[dst[i]], 1u)] = src[i];
}

// Level 1 by push (the frontier is only the batch's sources): every rel
// (x → y) whose x is source j of the batch sets bit j of y in visited and in
// the level-2 frontier — M atomics instead of a pull over M·K words.
__global__ void k_vr_srcpos(const int64_t *src_nodes, int64_t ns, int32_t *srcpos) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < ns;
       j += (int64_t)gridDim.x * blockDim.x)
    srcpos[src_nodes[j]] = (int32_t)j;
}

__global__ void k_vr_push1(const uint32_t *si, const uint32_t *di, int64_t m, const int32_t *srcpos,
                           int64_t s0, int64_t nb, int64_t K, unsigned long long *visited,
                           unsigned long long *frontier) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = (int64_t)srcpos[si[i]] - s0;
    if (j < 0 || j >= nb) continue;
    const int64_t w = (int64_t)di[i] * K + (j >> 6);
    const unsigned long long bit = 1ull << (j & 63);
    atomicOr(&visited[w], bit);
    atomicOr(&frontier[w], bit);
  }
}

constexpr int VR_ILP = 16;

// rows by decreasing in-degree: the hub rows (long dependent load chains)
// start first and overlap with the bulk instead of forming the tail
__global__ void k_vr_degkey(const uint32_t *rowptr, uint32_t D, uint64_t *key) {
  for (uint32_t y = blockIdx.x * blockDim.x + threadIdx.x; y < D; y += gridDim.x * blockDim.x)
    key[y] = ((uint64_t)(0xFFFFFFFFu - (rowptr[y + 1] - rowptr[y])) << 32) | y;
}

__global__ __launch_bounds__(256) void k_vr_level(const uint32_t *rowptr, const uint32_t *cols,
                                                  const uint64_t *order,
                                                  const unsigned long long *frontier,
                                                  unsigned long long *next,
                                                  unsigned long long *visited, int64_t D,
                                                  int64_t K, int last) {
  const int64_t total = D * K;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = t / K, k = t - r * K;
    const int64_t y = (int64_t)(uint32_t)order[r];
    const int64_t ty = y * K + k;
    unsigned long long acc = 0;
    const uint32_t e1 = rowptr[y + 1];
    uint32_t e = rowptr[y];
    // VR_ILP independent (col, frontier) load pairs in flight per lane: a
    // row is a chain of dependent loads otherwise, and hub rows (in-degree
    // 10^4+) would run at one HBM latency per rel
    for (; e + VR_ILP <= e1; e += VR_ILP) {
      uint32_t c[VR_ILP];
#pragma unroll
      for (int i = 0; i < VR_ILP; ++i) c[i] = cols[e + i];
      unsigned long long f[VR_ILP];
#pragma unroll
      for (int i = 0; i < VR_ILP; ++i) f[i] = frontier[(int64_t)c[i] * K + k];
#pragma unroll
      for (int i = 0; i < VR_ILP; ++i) acc |= f[i];
    }
    for (; e < e1; ++e) acc |= frontier[(int64_t)cols[e] * K + k];
    const unsigned long long v = visited[ty];
    const unsigned long long nv = acc & ~v;
    if (!last) next[ty] = nv;
    if (nv) visited[ty] = v | nv;
  }
}

// reach[s0 + 64k + j] = #{y : target(y) ∧ bit j of visited[y][k]}
__global__ __launch_bounds__(256) void k_vr_count(const unsigned long long *visited,
                                                  const uint8_t *target, int64_t D, int64_t K,
                                                  int64_t s0, int64_t ns, int64_t *reach) {
  __shared__ uint32_t part[4][WAVE];
  const int64_t k = blockIdx.x;
  const int lane = lane_id(), w = threadIdx.x / WAVE;
  uint32_t cnt = 0;
  for (int64_t y0 = (int64_t)w * WAVE; y0 < D; y0 += 4 * WAVE) {
    const int64_t y = y0 + lane;
    const unsigned long long v = (y < D && target[y]) ? visited[y * K + k] : 0ull;
#pragma unroll 8
    for (int j = 0; j < WAVE; ++j) {
      const uint32_t c = (uint32_t)__popcll(__ballot((v >> j) & 1ull));
      cnt += lane == j ? c : 0u;
    }
  }
  part[w][lane] = cnt;
  __syncthreads();
  if (threadIdx.x < WAVE) {
    const int64_t j = k * WAVE + threadIdx.x;
    if (j < ns)
      reach[s0 + j] = (int64_t)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] +
                      part[3][threadIdx.x];
  }
}

// The same counts from coalesced loads (CAPF_VR_COUNT=0 keeps k_vr_count):
// block (kc, cg) = source words [64·kc, 64·kc + 64) × row chunks cg·16 + w
// of VR_CR rows, one per wave; lane = source word, reading visited[y][k] as
// 512-B rows.  Each lane adds its words into a bit-sliced counter (level i
// holds bit i of the 64 per-source counts), the wave then hands out the
// counts (lane j: bit j of every level of lane l's counter) into an LDS
// table, and the block adds that table to reach[] with one coalesced atomic
// pass.  Zero reach[s0, s0 + ns) first.
constexpr int VR_CR = 256;   // rows per wave (< 2^VR_CL)
constexpr int VR_CL = 9;

__global__ __launch_bounds__(1024) void k_vr_count_bs(const unsigned long long *visited,
                                                      const uint8_t *target, int64_t D, int64_t K,
                                                      int64_t s0, int64_t ns, unsigned long long *reach) {
  __shared__ uint32_t tab[WAVE * WAVE];
  for (int i = threadIdx.x; i < WAVE * WAVE; i += 1024) tab[i] = 0;
  __syncthreads();
  const int lane = lane_id(), w = threadIdx.x / WAVE;
  const int64_t kc = blockIdx.x, k = kc * WAVE + lane;
  const int64_t y0 = ((int64_t)blockIdx.y * (1024 / WAVE) + w) * VR_CR, y1 = min(y0 + (int64_t)VR_CR, D);
  unsigned long long c[VR_CL];
#pragma unroll
  for (int i = 0; i < VR_CL; ++i) c[i] = 0ull;
  if (y0 < D) {
    const bool kin = k < K;
#pragma unroll 4
    for (int64_t y = y0; y < y1; ++y) {
      const unsigned long long v = (kin && target[y]) ? visited[y * K + k] : 0ull;
      unsigned long long carry = v;
#pragma unroll
      for (int i = 0; i < VR_CL; ++i) {
        const unsigned long long t = c[i] & carry;
        c[i] ^= carry;
        carry = t;
      }
    }
    for (int l = 0; l < WAVE; ++l) {
      uint32_t cnt = 0;
#pragma unroll
      for (int i = 0; i < VR_CL; ++i) {
        const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)c[i], l);
        const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(c[i] >> 32), l);
        const uint32_t word = lane < 32 ? lo : hi;
        cnt += ((word >> (lane & 31)) & 1u) << i;
      }
      if (cnt) atomicAdd(&tab[l * WAVE + lane], cnt);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < WAVE * WAVE; i += 1024) {
    const int64_t src = kc * WAVE * WAVE + i;  // word kc·64 + i/64, bit i%64
    if (tab[i] && src < ns) atomicAdd(&reach[s0 + src], (unsigned long long)tab[i]);
  }
}

__global__ void k_vr_out(const int64_t *rows, int64_t n, const int64_t *src_nodes,
                         const uint64_t *dict, const int64_t *reach, int64_t *a, int64_t *r) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = rows[i];
    a[i] = (int64_t)(dict[src_nodes[j]] ^ 0x8000000000000000ull);
    r[i] = reach[j];
  }
}

// lower bound 0 (the copyElement branch, VarLengthExpandPlanner.scala:180-205):
// every source also pairs with itself — once, so +1 unless a walk of the
// batch already reached the source as a target
__global__ void k_vr_self(const unsigned long long *vis, const uint8_t *tflag, const int64_t *src_nodes,
                          int64_t K, int64_t s0, int64_t nb, int64_t *reach) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nb;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = src_nodes[s0 + i];
    const bool hit = tflag[p] && ((vis[p * K + (i >> 6)] >> (i & 63)) & 1ull);
    if (!hit) reach[s0 + i] += 1;
  }
}

__global__ void k_vr_ones(int64_t *r, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    r[i] = 1;
}

__global__ void k_vr_pos(const int64_t *reach, int64_t n, uint8_t *flag) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    flag[i] = reach[i] > 0;
}

// ------------------------------------------------------------------ trails
// Lower bound ≥ 2 (directed, upper ≤ 4): the DISTINCT (a, b) pairs are those
// joined by a TRAIL (pairwise distinct rels) of length lower..upper — a walk
// no longer shortens into the range (a→b, b→a: *2..3 has the walk a→b→a→b and
// no trail to b), so the BFS above cannot answer it.  One workgroup per source
// enumerates the source's trails over an out-CSR whose positions are the rel
// identities (one position per rel row: parallel rels differ, a self-loop is
// one) and marks their end nodes in a D-bit LDS bitmap; reach = popcount of
// bitmap ∧ target mask.
constexpr int VT_BLOCK = 512;
constexpr uint32_t VT_NONE = 0xFFFFFFFFu;          // an empty stack entry (no rel position: m < 2^31)
constexpr int64_t VT_MAX_NODES = int64_t(1) << 20;  // a 128 KiB bitmap of the CU's 160 KiB LDS
constexpr size_t VT_LDS_MAX = 160 * 1024;
constexpr int VT_ILP = 4;            // independent row loads per lane
constexpr uint32_t VT_SHORT = 32;    // last-level rows up to this length are walked by one lane each

__global__ void k_vt_tmask(const uint8_t *tflag, uint32_t D, uint32_t *tmask) {
  const uint32_t W = (D + 31) / 32;
  for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < W; w += gridDim.x * blockDim.x) {
    uint32_t v = 0;
    for (uint32_t b = 0; b < 32 && w * 32 + b < D; ++b) v |= (tflag[w * 32 + b] ? 1u : 0u) << b;
    tmask[w] = v;
  }
}

// sources by decreasing degree: a hub source's workgroup starts first.  The
// degree is the out-degree, plus the in-degree where irow is given (the
// undirected steps; out + in ≤ 2m < 2^32)
__global__ void k_vt_srckey(const int64_t *src_nodes, int64_t ns, const uint32_t *orow, const uint32_t *irow,
                            uint64_t *key) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < ns;
       j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = src_nodes[j];
    uint32_t deg = orow[a + 1] - orow[a];
    if (irow) deg += irow[a + 1] - irow[a];
    key[j] = ((uint64_t)(0xFFFFFFFFu - deg) << 32) | (uint64_t)j;
  }
}

__device__ inline void vt_mark(uint32_t *bm, uint32_t y) { atomicOr(&bm[y >> 5], 1u << (y & 31)); }

// Prologue of an enumeration block: zeroes its n bitmap words and the two
// control words behind them (ctl[0] the first-hop cursor, ctl[1] the count).
__device__ __forceinline__ void vt_clear(uint32_t *lds, uint32_t n, uint32_t *ctl) {
  for (uint32_t w = threadIdx.x; w < n; w += VT_BLOCK) lds[w] = 0;
  if (threadIdx.x < 2) ctl[threadIdx.x] = 0;
  __syncthreads();
}

// Epilogue: once every wave's marks are in, reach[j] = popcount(bitmap ∧ tmask).
__device__ __forceinline__ void vt_count(const uint32_t *bm, const uint32_t *__restrict__ tmask, uint32_t W,
                                         uint32_t *ctl, int lane, int64_t j, int64_t *reach) {
  __syncthreads();
  uint32_t c = 0;
  for (uint32_t w = threadIdx.x; w < W; w += VT_BLOCK) c += (uint32_t)__popc(bm[w] & tmask[w]);
  c = wave_reduce_sum(c);
  if (lane == 0 && c) atomicAdd(&ctl[1], c);
  __syncthreads();
  if (threadIdx.x == 0) reach[j] = (int64_t)ctl[1];
}

// The wave stands at node d_S with out-row [b, e) after a trail of S rels whose
// positions are s1..s3 (VT_NONE beyond S) and whose start nodes are d0..d_{S-1}
// (VT_NONE beyond d_S); everything but `lane` is wave-uniform.  Last level
// (S + 1 = U): lanes stride over the row, skip the stack's positions and mark
// the end nodes.  Before it: each lane takes one position of the row, loads
// its end node y and y's row bounds, marks y when the trail is long enough,
// and the wave descends into the lanes' rows one after the other (bounds
// handed out by readlane).
// Expanded rows (ex, a second bitmap): when y's row is the last level and y is
// none of d0..d_S, no rel of the stack lies in y's row, so what the last level
// marks from y is y's whole row, whatever trail led there: the lane that sets
// y's bit in ex first descends, every later visit of y from this source is
// dropped.  A hub source reaches the same nodes over 10^7 trail prefixes; its
// last level shrinks from one row per prefix to one row per node.
template <int S, int U>
__device__ inline void vt_walk(const uint32_t *__restrict__ orow, const uint32_t *__restrict__ ocol,
                               uint32_t *bm, uint32_t *ex, int lower, uint32_t b, uint32_t e,
                               uint32_t s1, uint32_t s2, uint32_t s3, uint32_t d0, uint32_t d1,
                               uint32_t d2, uint32_t d3, int lane) {
  if constexpr (S + 1 >= U) {
    // VT_ILP loads in flight per lane: a long row is a chain of load → LDS or otherwise
    for (uint32_t p0 = b + lane; p0 < e; p0 += VT_ILP * WAVE) {
      uint32_t v[VT_ILP];
      bool on[VT_ILP];
#pragma unroll
      for (int i = 0; i < VT_ILP; ++i) {
        const uint32_t p = p0 + i * WAVE;
        on[i] = p < e && p != s1 && p != s2 && p != s3;
        v[i] = on[i] ? ocol[p] : 0u;
      }
#pragma unroll
      for (int i = 0; i < VT_ILP; ++i)
        if (on[i]) vt_mark(bm, v[i]);
    }
  } else {
    for (uint32_t p0 = b; p0 < e; p0 += WAVE) {
      const uint32_t p = p0 + lane;
      const bool ok = p < e && p != s1 && p != s2 && p != s3;
      uint32_t y = 0, yb = 0, ye = 0;
      if (ok) {
        y = ocol[p];
        yb = orow[y];
        ye = orow[y + 1];
        if (S + 1 >= lower) vt_mark(bm, y);
        if constexpr (S + 2 == U) {
          if (ex && ye > yb && y != d0 && y != d1 && y != d2 && y != d3) {
            const uint32_t bit = 1u << (y & 31);
            if (atomicOr(&ex[y >> 5], bit) & bit) ye = yb;  // y's row is already in the bitmap
          }
        }
      }
      if constexpr (S + 2 == U) {
        // short last-level rows: every lane walks its own y's row (stack: s1..s3
        // and p, the rel that led to y) — 64 rows at a time, instead of the
        // wave descending into one row of a few entries after the other
        const uint32_t len = ok ? ye - yb : 0u;
        const bool mine = len > 0 && len <= VT_SHORT;
        for (uint32_t k = 0; __ballot(mine && k < len); k += VT_ILP) {
          uint32_t v[VT_ILP];
          bool on[VT_ILP];
#pragma unroll
          for (int i = 0; i < VT_ILP; ++i) {
            const uint32_t pp = yb + k + i;
            on[i] = mine && k + i < len && pp != s1 && pp != s2 && pp != s3 && pp != p;
            v[i] = on[i] ? ocol[pp] : 0u;
          }
#pragma unroll
          for (int i = 0; i < VT_ILP; ++i)
            if (on[i]) vt_mark(bm, v[i]);
        }
        if (mine) ye = yb;
      }
      unsigned long long todo = __ballot(ok && ye > yb);
      while (todo) {
        const int i = __builtin_amdgcn_readfirstlane(__ffsll(todo) - 1);
        todo &= todo - 1;
        const uint32_t nb = __builtin_amdgcn_readlane(yb, i), ne = __builtin_amdgcn_readlane(ye, i);
        const uint32_t ny = __builtin_amdgcn_readlane(y, i);
        const uint32_t q = p0 + (uint32_t)i;
        if constexpr (S == 1) vt_walk<2, U>(orow, ocol, bm, ex, lower, nb, ne, s1, q, VT_NONE, d0, d1, ny, VT_NONE, lane);
        else vt_walk<3, U>(orow, ocol, bm, ex, lower, nb, ne, s1, s2, q, d0, d1, d2, ny, lane);
      }
    }
  }
}

// Block blockIdx.x = the source sorder[blockIdx.x] (low word: its position j
// in src_nodes).  Dynamic LDS: the bitmap (⌈D/32⌉ words, padded to 16 B), the
// expanded-rows bitmap of the same size when use_ex, then the first-hop cursor
// and the count.  The waves take first hops from the cursor (wave-uniform
// loads), so a hub source's rows spread over all waves.
template <int U>
__global__ __launch_bounds__(VT_BLOCK) void k_vt_trails(const uint32_t *__restrict__ orow,
                                                        const uint32_t *__restrict__ ocol,
                                                        const uint64_t *__restrict__ sorder,
                                                        const int64_t *__restrict__ src_nodes,
                                                        const uint32_t *__restrict__ tmask, uint32_t D,
                                                        int lower, int use_ex, int64_t *reach) {
  extern __shared__ __attribute__((aligned(16))) uint32_t vt_lds[];
  const uint32_t W = (D + 31) / 32, Wp = (W + 3) & ~3u;
  uint32_t *bm = vt_lds, *ex = use_ex ? vt_lds + Wp : nullptr;
  uint32_t *ctl = vt_lds + (use_ex ? 2 * Wp : Wp);
  vt_clear(vt_lds, use_ex ? 2 * Wp : Wp, ctl);
  const int64_t j = (int64_t)(uint32_t)sorder[blockIdx.x];
  const uint32_t a = (uint32_t)src_nodes[j];
  const uint32_t r0 = orow[a], r1 = orow[a + 1];
  const int lane = lane_id();
  for (;;) {
    uint32_t t = 0;
    if (lane == 0) t = atomicAdd(&ctl[0], 1u);
    const uint32_t p = r0 + __builtin_amdgcn_readfirstlane(t);
    if (p >= r1) break;
    const uint32_t y = ocol[p];
    const uint32_t yb = orow[y], ye = orow[y + 1];
    if (lower <= 1 && lane == 0) vt_mark(bm, y);
    if (ye == yb) continue;
    if constexpr (U == 2) {  // y's row is the last level
      if (ex && y != a) {
        uint32_t old = 0;
        if (lane == 0) old = atomicOr(&ex[y >> 5], 1u << (y & 31));
        if ((__builtin_amdgcn_readfirstlane(old) >> (y & 31)) & 1u) continue;
      }
    }
    vt_walk<1, U>(orow, ocol, bm, ex, lower, yb, ye, p, VT_NONE, VT_NONE, a, y, VT_NONE, VT_NONE, lane);
  }
  vt_count(bm, tmask, W, ctl, lane, j, reach);
}

// ------------------------------------------------------------------ undirected steps
// The undirected lowering (VarLengthExpandPlanner.scala:277-307) is an automaton
// over states (node x, mode out | in), from (a, out): a rel e not yet on the
// path leads
//   (x, out), start(e) = x → (end(e), out)      (x, in), start(e) = x → (x, in)
//   (x, out), end(e) = x → (start(e), in)       (x, in), end(e) = x → (x, out)
// (after an inbound step the next step does not move), and a state of depth
// max(lower, 1)..upper pairs a with its node.  One workgroup per source
// enumerates these steps as k_vt_trails enumerates trails; a rel's identity
// is its position in the out-CSR, which every in-CSR entry carries beside the
// other endpoint (iadj: x = start node, y = out position), so the rels of a
// path compare as out positions whichever row they were taken from.  A state's
// two rows are walked as one range: [0, od) the out-row, [od, tot) the in-row.
constexpr uint32_t VU_OUT = 0, VU_IN = 1;

struct VuCsr {
  const uint32_t *__restrict__ orow, *__restrict__ ocol, *__restrict__ irow;
  const uint2 *__restrict__ iadj;
};

// The in-rows, filled from the out-CSR itself: out position p lies in the row
// of x, the one row with orow[x] ≤ p < orow[x + 1] (binary search over the
// D + 1 bounds, orow[0] = 0 ≤ p < m = orow[D]; empty rows on either side of x
// share a bound with it and fail the test), and leads to y = ocol[p], so
// (x, p) goes into y's in-row through the cursor (a copy of irow).
__global__ void k_vu_fill_in(const uint32_t *orow, const uint32_t *ocol, uint32_t D, int64_t m, uint32_t *cursor,
                             uint2 *iadj) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t p = (uint32_t)i;
    uint32_t lo = 0, hi = D;  // orow[lo] ≤ p < orow[hi]
    while (hi - lo > 1) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (orow[mid] <= p) lo = mid;
      else hi = mid;
    }
    iadj[atomicAdd(&cursor[ocol[p]], 1u)] = make_uint2(lo, p);
  }
}

__device__ inline bool vu_free(uint32_t r, uint32_t s1, uint32_t s2, uint32_t s3) {
  return r != s1 && r != s2 && r != s3;
}

// The last level from (x, in): every remaining rel leads back to x, so x is an
// end node iff one of x's row entries is not on the stack.  A stack rel takes
// one entry off the out-row when its position lies there and one off the
// in-row when it ends at x (a self-loop on the stack: both).
__device__ inline bool vu_in_last(const VuCsr &g, uint32_t x, uint32_t s1, uint32_t s2, uint32_t s3) {
  const uint32_t ob = g.orow[x], oe = g.orow[x + 1];
  uint32_t left = (oe - ob) + (g.irow[x + 1] - g.irow[x]);
  if (s1 != VT_NONE) left -= (uint32_t)(s1 >= ob && s1 < oe) + (uint32_t)(g.ocol[s1] == x);
  if (s2 != VT_NONE) left -= (uint32_t)(s2 >= ob && s2 < oe) + (uint32_t)(g.ocol[s2] == x);
  if (s3 != VT_NONE) left -= (uint32_t)(s3 >= ob && s3 < oe) + (uint32_t)(g.ocol[s3] == x);
  return left > 0;
}

// The wave stands at state (x, mode) after S rels at out positions s1..s3
// (VT_NONE beyond S); everything but `lane` is wave-uniform.  Last level
// (S + 1 = U): from mode in the degree test above, from mode out the lanes
// stride over both rows, skip the stack and mark the other endpoints.  Before
// it: each lane takes one entry, marks the next state's node when the path is
// long enough, and the wave descends into the lanes' states one after the
// other (handed out by readlane).  One level above the last, the lanes settle
// their own mode-in states by the degree test instead of a descent.
template <int S, int U>
__device__ inline void vu_walk(const VuCsr &g, uint32_t *bm, int lower, uint32_t x, uint32_t mode,
                               uint32_t s1, uint32_t s2, uint32_t s3, int lane) {
  const uint32_t ob = g.orow[x], od = g.orow[x + 1] - ob;
  const uint32_t ib = g.irow[x], tot = od + (g.irow[x + 1] - ib);
  if constexpr (S + 1 >= U) {
    if (mode == VU_IN) {
      if (vu_in_last(g, x, s1, s2, s3)) vt_mark(bm, x);  // wave-uniform: see k_vu_steps
    }
    // VT_ILP loads in flight per lane; a wave-uniform trip count
    for (uint32_t t0 = 0; mode == VU_OUT && t0 < tot; t0 += VT_ILP * WAVE) {
      uint32_t v[VT_ILP];
      bool on[VT_ILP];
#pragma unroll
      for (int i = 0; i < VT_ILP; ++i) {
        const uint32_t t = t0 + lane + i * WAVE;
        on[i] = false;
        v[i] = 0u;
        if (t < od) {
          on[i] = vu_free(ob + t, s1, s2, s3);
          v[i] = g.ocol[ob + t];
        } else if (t < tot) {
          const uint2 e = g.iadj[ib + (t - od)];
          on[i] = vu_free(e.y, s1, s2, s3);
          v[i] = e.x;
        }
      }
#pragma unroll
      for (int i = 0; i < VT_ILP; ++i)
        if (on[i]) vt_mark(bm, v[i]);
    }
  } else {
    for (uint32_t t0 = 0; t0 < tot; t0 += WAVE) {
      const uint32_t t = t0 + lane;
      uint32_t r = VT_NONE, oth = 0, isin = 0;
      if (t < od) {
        r = ob + t;
        oth = g.ocol[r];
      } else if (t < tot) {
        const uint2 e = g.iadj[ib + (t - od)];
        oth = e.x;
        r = e.y;
        isin = 1;
      }
      bool ok = t < tot && vu_free(r, s1, s2, s3);
      const uint32_t ny = mode == VU_IN ? x : oth, nm = mode ^ isin;
      if (S + 1 >= lower) {
        if (mode == VU_IN) {  // every lane's next state sits on x
          if (__ballot(ok)) vt_mark(bm, x);
        } else if (ok) {
          vt_mark(bm, ny);
        }
      }
      if constexpr (S + 2 == U) {
        const bool mine = ok && nm == VU_IN;
        const bool hit = mine && (S == 1 ? vu_in_last(g, ny, s1, r, VT_NONE) : vu_in_last(g, ny, s1, s2, r));
        if (mode == VU_IN) {
          if (__ballot(hit)) vt_mark(bm, x);
        } else if (hit) {
          vt_mark(bm, ny);
        }
        if (mine) ok = false;
      }
      unsigned long long todo = __ballot(ok);
      while (todo) {
        const int i = __builtin_amdgcn_readfirstlane(__ffsll(todo) - 1);
        todo &= todo - 1;
        const uint32_t qy = __builtin_amdgcn_readlane(ny, i), qm = __builtin_amdgcn_readlane(nm, i);
        const uint32_t qr = __builtin_amdgcn_readlane(r, i);
        if constexpr (S == 1) vu_walk<2, U>(g, bm, lower, qy, qm, s1, qr, VT_NONE, lane);
        else vu_walk<3, U>(g, bm, lower, qy, qm, s1, s2, qr, lane);
      }
    }
  }
}

// Block blockIdx.x = the source sorder[blockIdx.x], as in k_vt_trails.  Dynamic
// LDS: the bitmap (⌈D/32⌉ words, padded to 16 B), then the first-hop cursor and
// the count.  The first hops are a's out-row (to (end, out)) and in-row (to
// (start, in)); the waves take them from the cursor.
// No statement of the cursor loop, or of vu_walk's wave-uniform parts, is
// guarded by `lane == 0`: every lane issues the cursor's atomicAdd (lane 0
// adds 1, the others 0) and the marks of a wave-uniform node (the same bit;
// the compiler folds either into one LDS atomic per wave).  With `if (lane ==
// 0)` guards the compiler threaded the lanes that skip one guard past the
// next one, across the loop's back edge: those lanes then read the cursor as
// the constant 0 under a partial exec mask and never left the loop when the
// source's first hop was an inbound one (an empty out-row).
template <int U>
__global__ __launch_bounds__(VT_BLOCK) void k_vu_steps(const uint32_t *__restrict__ orow,
                                                       const uint32_t *__restrict__ ocol,
                                                       const uint32_t *__restrict__ irow,
                                                       const uint2 *__restrict__ iadj,
                                                       const uint64_t *__restrict__ sorder,
                                                       const int64_t *__restrict__ src_nodes,
                                                       const uint32_t *__restrict__ tmask, uint32_t D,
                                                       int lower, int64_t *reach) {
  extern __shared__ __attribute__((aligned(16))) uint32_t vu_lds[];
  const uint32_t W = (D + 31) / 32, Wp = (W + 3) & ~3u;
  uint32_t *bm = vu_lds, *ctl = vu_lds + Wp;
  vt_clear(bm, Wp, ctl);
  const int64_t j = (int64_t)(uint32_t)sorder[blockIdx.x];
  const uint32_t a = (uint32_t)src_nodes[j];
  const int lane = lane_id();
  if (lower == 0 && threadIdx.x == 0) vt_mark(bm, a);  // the zero-length path
  if constexpr (U >= 1) {
    const VuCsr g{orow, ocol, irow, iadj};
    const uint32_t ob = orow[a], od = orow[a + 1] - ob;
    const uint32_t ib = irow[a], tot = od + (irow[a + 1] - ib);
    for (;;) {
      const uint32_t t = __builtin_amdgcn_readfirstlane(atomicAdd(&ctl[0], lane == 0 ? 1u : 0u));
      if (t >= tot) break;
      uint32_t r, y, nm;
      if (t < od) {
        r = ob + t;
        y = ocol[r];
        nm = VU_OUT;
      } else {
        const uint2 e = iadj[ib + (t - od)];
        y = e.x;
        r = e.y;
        nm = VU_IN;
      }
      if (lower <= 1) vt_mark(bm, y);
      if constexpr (U >= 2) vu_walk<1, U>(g, bm, lower, y, nm, r, VT_NONE, VT_NONE, lane);
    }
  }
  vt_count(bm, tmask, W, ctl, lane, j, reach);
}

// HBM budget of the three MS-BFS state arrays (sources are batched to fit)
constexpr double VR_STATE_BUDGET = 24e9;

// The environment knobs, read once per query and never kept: the tests change
// them between queries of one process.
struct VrKnobs {
  double budget;      // CAPF_VR_BUDGET (tests): a smaller state budget in bytes → more source batches
  bool count_bs;      // CAPF_VR_COUNT=0 (tuning): the ballot-transpose count
  bool expand;        // CAPF_VT_EXPAND=0 (tests, tuning): never the expanded-rows bitmap
  int64_t max_nodes;  // CAPF_VT_MAX_NODES (tests): a lower node limit of the enumeration kernels
};

static VrKnobs vr_knobs() {
  const char *vb = getenv("CAPF_VR_BUDGET"), *vc = getenv("CAPF_VR_COUNT");
  const char *ve = getenv("CAPF_VT_EXPAND"), *vm = getenv("CAPF_VT_MAX_NODES");
  VrKnobs k;
  k.budget = vb && atof(vb) > 0 ? atof(vb) : VR_STATE_BUDGET;
  k.count_bs = !(vc && atoi(vc) == 0);
  k.expand = !(ve && atoi(ve) == 0);
  k.max_nodes = vm && atoll(vm) > 0 ? std::min<int64_t>(atoll(vm), VT_MAX_NODES) : VT_MAX_NODES;
  return k;
}

// The reach index of (rels, sources, targets): id dictionary, dense endpoint
// indices, in-CSR by target, the degree order of its rows, source positions
// and target flags.  Everything here is a function of four immutable columns,
// so it is built by the first query and cached on the rel source column (an
// ingest-time adjacency index, like the triangle's oriented CSR) together with
// the other three columns and their lengths, its key; a query with other node
// columns (e.g. a filtered scan) builds its own.
struct VrIndex {
  std::weak_ptr<Column> rdst, sid, tid;
  int64_t m = 0, ns_in = 0, nt = 0;
  uint32_t D = 0;
  int64_t ns = 0;
  BufPtr dict, si, di, tflag, src_nodes, rowptr, cols, order, srcpos;
  // The enumeration part (trails, undirected steps), built on first use under
  // en_mu.  By the first enumeration query of either kind: the out-CSR by
  // source, whose positions are the rel identities of both kernels, the target
  // bitmask of ⌈D/32⌉ words, the sources by decreasing out-degree.  By the
  // first undirected query, on top: in-adjacency entries (start node, out
  // position) in the in-CSR's rows (rowptr), the sources by decreasing out + in
  // degree.
  std::mutex en_mu;
  BufPtr orow, ocol, tmask, sorder;
  BufPtr uiadj, usorder;
};

// CSR of m (row, value) pairs over D rows: degree count, exclusive scan into
// the D + 1 row bounds, fill through a cursor copy of them.
static void vr_csr(Session *s, const uint32_t *row, const uint32_t *val, int64_t m, uint32_t D, BufPtr &rowptr,
                   BufPtr &cols) {
  const size_t nb = 4 * ((size_t)D + 1);
  const unsigned g = grid_for(m, 256, 256 * 64);
  BufPtr deg = s->alloc(nb), cursor = s->alloc(nb), tot = s->alloc(16);
  rowptr = s->alloc(nb);
  cols = s->alloc(4 * m);
  HIP_CHECK(hipMemsetAsync(deg->p, 0, nb, s->stream));
  hipLaunchKernelGGL(k_vr_indeg, dim3(g), dim3(256), 0, s->stream, row, m, (uint32_t *)deg->p);
  exclusive_scan_u32_async(s, (const uint32_t *)deg->p, (uint32_t *)rowptr->p, (int64_t)D + 1, (uint32_t *)tot->p);
  HIP_CHECK(hipMemcpyAsync(cursor->p, rowptr->p, nb, hipMemcpyDeviceToDevice, s->stream));
  hipLaunchKernelGGL(k_vr_fill, dim3(g), dim3(256), 0, s->stream, val, row, m, (uint32_t *)cursor->p,
                     (uint32_t *)cols->p);
  KERNEL_CHECK();
}

// The degree order of the sources (k_vt_srckey): keys sorted ascending, the
// low word of each the source's position in src_nodes.
static BufPtr vt_source_order(Session *s, const VrIndex &ix, const uint32_t *irow) {
  BufPtr skey = s->alloc(8 * ix.ns), sorder = s->alloc(8 * ix.ns);
  hipLaunchKernelGGL(k_vt_srckey, dim3(grid_for(ix.ns, 256)), dim3(256), 0, s->stream,
                     (const int64_t *)ix.src_nodes->p, ix.ns, (const uint32_t *)ix.orow->p, irow,
                     (uint64_t *)skey->p);
  KERNEL_CHECK();
  vr_rocprim(s, [&](void *t, size_t &n) {
    return rocprim::radix_sort_keys(t, n, (const uint64_t *)skey->p, (uint64_t *)sorder->p, (size_t)ix.ns, 0, 64,
                                    s->stream);
  });
  return sorder;
}

// Builds what of the enumeration part the query needs and the index lacks.
// Each half is synchronised before the index shows it: another session may
// read it from its own stream.
static void vt_build(Session *s, VrIndex &ix, bool undirected) {
  std::lock_guard<std::mutex> lk(ix.en_mu);
  const uint32_t D = ix.D;
  const int64_t m = ix.m;
  if (!ix.sorder) {
    const int64_t W = ((int64_t)D + 31) / 32;
    {
      KernelTimer kt(s, "vt_index", 16.0 * m);
      // rows keyed by the rel's source, holding its target
      vr_csr(s, (const uint32_t *)ix.si->p, (const uint32_t *)ix.di->p, m, D, ix.orow, ix.ocol);
      ix.tmask = s->alloc(4 * W);
      hipLaunchKernelGGL(k_vt_tmask, dim3(grid_for(W, 256)), dim3(256), 0, s->stream,
                         (const uint8_t *)ix.tflag->p, D, (uint32_t *)ix.tmask->p);
      KERNEL_CHECK();
      ix.sorder = vt_source_order(s, ix, nullptr);
    }
    s->sync();
  }
  if (undirected && !ix.usorder) {
    const size_t nb = 4 * ((size_t)D + 1);
    BufPtr cursor = s->alloc(nb);
    {
      KernelTimer kt(s, "vu_index", 24.0 * m);
      ix.uiadj = s->alloc(8 * m);
      HIP_CHECK(hipMemcpyAsync(cursor->p, ix.rowptr->p, nb, hipMemcpyDeviceToDevice, s->stream));
      hipLaunchKernelGGL(k_vu_fill_in, dim3(grid_for(m, 256, 256 * 64)), dim3(256), 0, s->stream,
                         (const uint32_t *)ix.orow->p, (const uint32_t *)ix.ocol->p, D, m, (uint32_t *)cursor->p,
                         (uint2 *)ix.uiadj->p);
      KERNEL_CHECK();
      ix.usorder = vt_source_order(s, ix, (const uint32_t *)ix.rowptr->p);
    }
    s->sync();
  }
}

// reach[j] of every source j by enumeration: trails (directed, 2 ≤ lower ≤
// upper ≤ 4) or the undirected steps (0 ≤ lower ≤ upper ≤ 4)
static void vt_enumerate(Session *s, VrIndex &ix, bool undirected, int lower, int upper, bool expand,
                         int64_t *reach) {
  vt_build(s, ix, undirected);
  // the kernels by upper bound
  static const decltype(&k_vt_trails<2>) trails[5] = {nullptr, nullptr, k_vt_trails<2>, k_vt_trails<3>,
                                                      k_vt_trails<4>};
  static const decltype(&k_vu_steps<0>) steps[5] = {k_vu_steps<0>, k_vu_steps<1>, k_vu_steps<2>, k_vu_steps<3>,
                                                    k_vu_steps<4>};
  static std::once_flag attr_once;
  std::call_once(attr_once, [] {
    for (int u = 0; u <= 4; ++u)
      for (const void *k : {(const void *)trails[u], (const void *)steps[u]})
        if (k) HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)VT_LDS_MAX));
  });
  const uint32_t D = ix.D;
  // LDS: the bitmap, the trails' expanded-rows bitmap while two fit (D up to
  // about 655 k), the two control words (padded to 16 B)
  const size_t wp = (size_t)(((D + 31) / 32 + 3) & ~3u);
  const int use_ex = !undirected && expand && 4 * (2 * wp + 4) <= VT_LDS_MAX;
  const size_t lds = 4 * ((use_ex ? 2 * wp : wp) + 4);
  const uint32_t *orow = (const uint32_t *)ix.orow->p, *ocol = (const uint32_t *)ix.ocol->p;
  const int64_t *src_nodes = (const int64_t *)ix.src_nodes->p;
  const uint32_t *tmask = (const uint32_t *)ix.tmask->p;
  KernelTimer kt(s, undirected ? "vu_steps" : "vt_trails", (undirected ? 12.0 : 4.0) * ix.m);
  if (undirected)
    hipLaunchKernelGGL(steps[upper], dim3((unsigned)ix.ns), dim3(VT_BLOCK), lds, s->stream, orow, ocol,
                       (const uint32_t *)ix.rowptr->p, (const uint2 *)ix.uiadj->p, (const uint64_t *)ix.usorder->p,
                       src_nodes, tmask, D, lower, reach);
  else
    hipLaunchKernelGGL(trails[upper], dim3((unsigned)ix.ns), dim3(VT_BLOCK), lds, s->stream, orow, ocol,
                       (const uint64_t *)ix.sorder->p, src_nodes, tmask, D, lower, use_ex, reach);
  KERNEL_CHECK();
}

static std::shared_ptr<VrIndex> vr_build(Session *s, const ColPtr &rsrc, const ColPtr &rdst, int64_t m,
                                         const ColPtr &sid, int64_t ns_in, const ColPtr &tid, int64_t nt) {
  auto ix = std::make_shared<VrIndex>();
  const int64_t nk = 2 * m + ns_in + nt;
  if (nk >= (int64_t(1) << 32)) not_impl("var-length reach: more than 2^32 ids");
  const unsigned g = grid_for(nk, 256, 256 * 64);
  // 1. dictionary of every id
  BufPtr keys = s->alloc(8 * nk), sorted = s->alloc(8 * nk);
  {
    KernelTimer kt(s, "vr_dict", 24.0 * nk);
    uint64_t *k = (uint64_t *)keys->p;
    hipLaunchKernelGGL(k_vr_keys, dim3(g), dim3(256), 0, s->stream, view_of(rsrc), m, k);
    hipLaunchKernelGGL(k_vr_keys, dim3(g), dim3(256), 0, s->stream, view_of(rdst), m, k + m);
    hipLaunchKernelGGL(k_vr_keys, dim3(g), dim3(256), 0, s->stream, view_of(sid), ns_in, k + 2 * m);
    hipLaunchKernelGGL(k_vr_keys, dim3(g), dim3(256), 0, s->stream, view_of(tid), nt,
                       k + 2 * m + ns_in);
    KERNEL_CHECK();
    vr_rocprim(s, [&](void *t, size_t &n) {
      return rocprim::radix_sort_keys(t, n, (const uint64_t *)keys->p, (uint64_t *)sorted->p,
                                      (size_t)nk, 0, 64, s->stream);
    });
  }
  BufPtr dict = s->alloc(8 * nk), runs = s->alloc(4 * nk), nruns = s->alloc(16);
  vr_rocprim(s, [&](void *t, size_t &n) {
    return rocprim::run_length_encode(t, n, (const uint64_t *)sorted->p, (unsigned int)nk,
                                      (uint64_t *)dict->p, (uint32_t *)runs->p,
                                      (uint32_t *)nruns->p, s->stream);
  });
  uint32_t D = 0;
  HIP_CHECK(hipMemcpyAsync(&D, nruns->p, 4, hipMemcpyDeviceToHost, s->stream));
  s->sync();
  keys.reset();
  sorted.reset();
  runs.reset();
  const uint64_t *dk = (const uint64_t *)dict->p;
  // 2. dense indices
  BufPtr si = s->alloc(4 * m), di = s->alloc(4 * m), xi = s->alloc(4 * std::max(ns_in, nt));
  BufPtr tflag = s->alloc(D), sflag = s->alloc(D);
  HIP_CHECK(hipMemsetAsync(tflag->p, 0, D, s->stream));
  HIP_CHECK(hipMemsetAsync(sflag->p, 0, D, s->stream));
  hipLaunchKernelGGL(k_vr_map, dim3(g), dim3(256), 0, s->stream, view_of(rsrc), m, dk, D,
                     (uint32_t *)si->p);
  hipLaunchKernelGGL(k_vr_map, dim3(g), dim3(256), 0, s->stream, view_of(rdst), m, dk, D,
                     (uint32_t *)di->p);
  hipLaunchKernelGGL(k_vr_map, dim3(g), dim3(256), 0, s->stream, view_of(tid), nt, dk, D,
                     (uint32_t *)xi->p);
  hipLaunchKernelGGL(k_vr_flag, dim3(g), dim3(256), 0, s->stream, (const uint32_t *)xi->p, nt,
                     (uint8_t *)tflag->p);
  hipLaunchKernelGGL(k_vr_map, dim3(g), dim3(256), 0, s->stream, view_of(sid), ns_in, dk, D,
                     (uint32_t *)xi->p);
  hipLaunchKernelGGL(k_vr_flag, dim3(g), dim3(256), 0, s->stream, (const uint32_t *)xi->p, ns_in,
                     (uint8_t *)sflag->p);
  KERNEL_CHECK();
  // distinct sources in dictionary order (a node scan holds each node once;
  // duplicates would be merged by the DISTINCT anyway)
  int64_t ns = 0;
  BufPtr src_nodes = compact_flags(s, (const uint8_t *)sflag->p, D, &ns);
  // 3. in-CSR by target: rows keyed by the rel's target, holding its source
  {
    KernelTimer kt(s, "vr_csr", 16.0 * m);
    vr_csr(s, (const uint32_t *)di->p, (const uint32_t *)si->p, m, D, ix->rowptr, ix->cols);
  }
  {
    BufPtr dkey = s->alloc(8 * (int64_t)D);
    ix->order = s->alloc(8 * (int64_t)D);
    hipLaunchKernelGGL(k_vr_degkey, dim3(grid_for(D, 256)), dim3(256), 0, s->stream,
                       (const uint32_t *)ix->rowptr->p, D, (uint64_t *)dkey->p);
    KERNEL_CHECK();
    vr_rocprim(s, [&](void *t, size_t &n) {
      return rocprim::radix_sort_keys(t, n, (const uint64_t *)dkey->p, (uint64_t *)ix->order->p,
                                      (size_t)D, 0, 64, s->stream);
    });
  }
  ix->srcpos = s->alloc(4 * (int64_t)D);
  HIP_CHECK(hipMemsetAsync(ix->srcpos->p, 0xFF, 4 * (size_t)D, s->stream));
  hipLaunchKernelGGL(k_vr_srcpos, dim3(grid_for(ns, 256)), dim3(256), 0, s->stream,
                     (const int64_t *)src_nodes->p, ns, (int32_t *)ix->srcpos->p);
  KERNEL_CHECK();
  ix->rdst = rdst;
  ix->sid = sid;
  ix->tid = tid;
  ix->m = m;
  ix->ns_in = ns_in;
  ix->nt = nt;
  ix->D = D;
  ix->ns = ns;
  ix->dict = dict;
  ix->si = si;
  ix->di = di;
  ix->tflag = tflag;
  ix->src_nodes = src_nodes;
  return ix;
}

// 4. MS-BFS in batches of 64·K sources: reach[j] of every source j
static void vr_bfs(Session *s, const VrIndex &ix, const VrKnobs &kn, int upper, bool include_self,
                   const BufPtr &reach) {
  const uint32_t D = ix.D;
  const int64_t m = ix.m, ns = ix.ns;
  const unsigned g = grid_for(m, 256, 256 * 64);
  const int64_t kmax = std::max<int64_t>(1, (int64_t)(kn.budget / (24.0 * D)));
  const int64_t K = std::min<int64_t>((ns + 63) / 64, kmax);
  BufPtr fa = s->alloc(8 * (int64_t)D * K), fb = s->alloc(8 * (int64_t)D * K);
  BufPtr vis = s->alloc(8 * (int64_t)D * K);
  const unsigned glev = grid_for((int64_t)D * K, 256, (int64_t)s->num_cus * 32);
  // the bit-sliced count takes row chunks on gridDim.y (≤ 65535): beyond that
  // (D > 2^26 nodes) the ballot-transpose count, whose grid is 1-D over sources
  const bool bs_count = kn.count_bs && (int64_t)D <= (int64_t)65535 * (1024 / WAVE) * VR_CR;
  for (int64_t s0 = 0; s0 < ns; s0 += 64 * K) {
    const int64_t nb = std::min<int64_t>(64 * K, ns - s0);
    HIP_CHECK(hipMemsetAsync(fb->p, 0, 8 * (size_t)D * K, s->stream));
    HIP_CHECK(hipMemsetAsync(vis->p, 0, 8 * (size_t)D * K, s->stream));
    {
      KernelTimer kt(s, "vr_push1", 12.0 * m);
      hipLaunchKernelGGL(k_vr_push1, dim3(g), dim3(256), 0, s->stream, (const uint32_t *)ix.si->p,
                         (const uint32_t *)ix.di->p, m, (const int32_t *)ix.srcpos->p, s0, nb, K,
                         (unsigned long long *)vis->p, (unsigned long long *)fb->p);
      KERNEL_CHECK();
    }
    unsigned long long *cur = (unsigned long long *)fb->p, *nxt = (unsigned long long *)fa->p;
    for (int l = 2; l <= upper; ++l) {
      KernelTimer kt(s, "vr_level", 8.0 * K * ((double)m + 3.0 * D));
      hipLaunchKernelGGL(k_vr_level, dim3(glev), dim3(256), 0, s->stream,
                         (const uint32_t *)ix.rowptr->p, (const uint32_t *)ix.cols->p,
                         (const uint64_t *)ix.order->p, cur, nxt,
                         (unsigned long long *)vis->p, (int64_t)D, K, l == upper ? 1 : 0);
      KERNEL_CHECK();
      std::swap(cur, nxt);
    }
    {
      KernelTimer kt(s, "vr_count", 8.0 * K * D);
      if (bs_count) {
        HIP_CHECK(hipMemsetAsync((int64_t *)reach->p + s0, 0, 8 * (size_t)nb, s->stream));
        const int64_t kw = (nb + 63) / 64;  // source words of this batch
        const int64_t cg = (D + (int64_t)(1024 / WAVE) * VR_CR - 1) / ((int64_t)(1024 / WAVE) * VR_CR);
        hipLaunchKernelGGL(k_vr_count_bs, dim3((unsigned)((kw + 63) / 64), (unsigned)cg), dim3(1024), 0,
                           s->stream, (const unsigned long long *)vis->p, (const uint8_t *)ix.tflag->p,
                           (int64_t)D, K, s0, nb, (unsigned long long *)reach->p);
      } else {
        hipLaunchKernelGGL(k_vr_count, dim3((unsigned)((nb + 63) / 64)), dim3(256), 0, s->stream,
                           (const unsigned long long *)vis->p, (const uint8_t *)ix.tflag->p, (int64_t)D,
                           K, s0, nb, (int64_t *)reach->p);
      }
      KERNEL_CHECK();
      if (include_self) {
        hipLaunchKernelGGL(k_vr_self, dim3(grid_for(nb, 256)), dim3(256), 0, s->stream,
                           (const unsigned long long *)vis->p, (const uint8_t *)ix.tflag->p,
                           (const int64_t *)ix.src_nodes->p, K, s0, nb, (int64_t *)reach->p);
        KERNEL_CHECK();
      }
    }
  }
}

ReachMethod reach_method(bool undirected, int lower, int upper) {
  if (undirected) return 0 <= lower && lower <= upper && upper <= 4 ? ReachMethod::STEPS : ReachMethod::NONE;
  if (lower >= 2) return lower <= upper && upper <= 4 ? ReachMethod::TRAILS : ReachMethod::NONE;
  return lower >= 0 && 1 <= upper && upper <= 64 ? ReachMethod::BFS : ReachMethod::NONE;
}

DataPtr var_length_reach_rows(Session *s, const ColPtr &rsrc, const ColPtr &rdst, int64_t m, const ColPtr &sid,
                              int64_t ns_in, const ColPtr &tid, int64_t nt, int lower, int upper,
                              bool undirected) {
  const ReachMethod rm = reach_method(undirected, lower, upper);
  if (rm == ReachMethod::NONE) return nullptr;
  const bool include_self = lower == 0;
  auto out = std::make_shared<Data>();
  out->cols = {make_column(s, Type::Int64, 0, false), make_column(s, Type::Int64, 0, false)};
  if (include_self && ns_in > 0 && (m == 0 || nt == 0)) {  // no walks: every (a, a) alone (unique ids: the caller's)
    ColPtr a = decode_column(s, sid), r = make_column(s, Type::Int64, ns_in, false);
    hipLaunchKernelGGL(k_vr_ones, dim3(grid_for(ns_in, 256)), dim3(256), 0, s->stream, (int64_t *)r->data->p,
                       ns_in);
    KERNEL_CHECK();
    out->nrows = ns_in;
    out->cols = {a, r};
    return out;
  }
  if (m == 0 || ns_in == 0 || nt == 0) return out;
  if (m >= (int64_t(1) << 32)) not_impl("var-length reach: more than 2^32 rels");
  std::shared_ptr<VrIndex> ix;
  {
    std::lock_guard<std::mutex> lk(rsrc->mu);
    ix = rsrc->vr_index;
  }
  if (!ix || ix->rdst.lock() != rdst || ix->sid.lock() != sid || ix->tid.lock() != tid || ix->m != m ||
      ix->ns_in != ns_in || ix->nt != nt) {
    ix = vr_build(s, rsrc, rdst, m, sid, ns_in, tid, nt);
    std::lock_guard<std::mutex> lk(rsrc->mu);
    rsrc->vr_index = ix;
  }
  const uint32_t D = ix->D;
  const int64_t ns = ix->ns;
  const VrKnobs kn = vr_knobs();
  // the enumeration kernels hold a D-bit bitmap in LDS and rel positions below 2^31
  if (rm != ReachMethod::BFS && ((int64_t)D > kn.max_nodes || m >= (int64_t(1) << 31))) return nullptr;
  BufPtr reach = s->alloc(8 * std::max<int64_t>(ns, 1));
  if (rm == ReachMethod::BFS) vr_bfs(s, *ix, kn, upper, include_self, reach);
  else vt_enumerate(s, *ix, rm == ReachMethod::STEPS, lower, upper, kn.expand, (int64_t *)reach->p);
  // 5. rows (a, reach) for the sources that reach at least one target (every
  // source from lower bound 0)
  BufPtr pos = s->alloc(std::max<int64_t>(ns, 1));
  hipLaunchKernelGGL(k_vr_pos, dim3(grid_for(ns, 256)), dim3(256), 0, s->stream,
                     (const int64_t *)reach->p, ns, (uint8_t *)pos->p);
  KERNEL_CHECK();
  int64_t nr = 0;
  BufPtr rows = compact_flags(s, (const uint8_t *)pos->p, ns, &nr);
  ColPtr a = make_column(s, Type::Int64, nr, false), r = make_column(s, Type::Int64, nr, false);
  if (nr > 0) {
    hipLaunchKernelGGL(k_vr_out, dim3(grid_for(nr, 256)), dim3(256), 0, s->stream,
                       (const int64_t *)rows->p, nr, (const int64_t *)ix->src_nodes->p, (const uint64_t *)ix->dict->p,
                       (const int64_t *)reach->p, (int64_t *)a->data->p, (int64_t *)r->data->p);
    KERNEL_CHECK();
  }
  s->sync();
  out->nrows = nr;
  out->cols = {a, r};
  return out;
}

static ColPtr int_column_of(const NodePtr &nd, const DataPtr &d, const char *name) {
  const ColPtr &c = d->cols[nd->col_index_or_throw(name)];
  force(c);
  if (c->type != Type::Int64) illegal(std::string("column ") + name + " is not INTEGER");
  if (c->valid) not_impl(std::string("var-length reach: nullable id column ") + name);
  return c;
}

}  // namespace capf

using namespace capf;

static capf_status vr_entry(capf_session *cs, capf_table *rels, const char *src_col, const char *dst_col,
                            capf_table *sources, const char *source_id_col, capf_table *targets,
                            const char *target_id_col, int32_t lower, int32_t upper, const char *out_source_col,
                            const char *out_reach_col, capf_table **out, bool undirected) {
  try {
    if (!cs || !rels || !src_col || !dst_col || !sources || !source_id_col || !targets ||
        !target_id_col || !out_source_col || !out_reach_col || !out)
      illegal("null argument");
    if (reach_method(undirected, lower, upper) == ReachMethod::NONE) {  // say which side of the domain
      if (undirected) not_impl("undirected var-length reach is fused for 0 <= lower <= upper <= 4 only");
      if (lower < 0) not_impl("var-length reach: negative lower bound");
      if (lower >= 2) not_impl("var-length reach: lower bounds from 2 are fused for 2 <= lower <= upper <= 4 only");
      illegal("var-length reach: upper bound out of range");
    }
    if (!strcmp(out_source_col, out_reach_col)) illegal("output column names must differ");
    Session *s = &cs->impl;
    DataPtr dr = materialize(rels->node), ds = materialize(sources->node),
            dt = materialize(targets->node);
    ColPtr rs = int_column_of(rels->node, dr, src_col), rd = int_column_of(rels->node, dr, dst_col);
    ColPtr si = int_column_of(sources->node, ds, source_id_col);
    ColPtr ti = int_column_of(targets->node, dt, target_id_col);
    DataPtr d = var_length_reach_rows(s, rs, rd, dr->nrows, si, ds->nrows, ti, dt->nrows, lower, upper, undirected);
    if (!d)
      not_impl(undirected ? "undirected var-length reach: more nodes than the step kernel's LDS bitmap holds (2^20)"
                          : "var-length reach: more nodes than the trail kernel's LDS bitmap holds (2^20)");
    auto n = std::make_shared<Node>();
    n->s = s;
    n->kind = Kind::Source;
    n->names = {out_source_col, out_reach_col};
    n->types = {Type::Int64, Type::Int64};
    n->result = d;
    auto *t = new capf_table;
    t->node = n;
    *out = t;
    return CAPF_OK;
  } catch (const capf::Error &e) {
    return record_error(e.code, e.what());
  }
}

extern "C" capf_status capf_var_length_reach(capf_session *cs, capf_table *rels, const char *src_col,
                                             const char *dst_col, capf_table *sources,
                                             const char *source_id_col, capf_table *targets,
                                             const char *target_id_col, int32_t lower, int32_t upper,
                                             const char *out_source_col, const char *out_reach_col,
                                             capf_table **out) {
  return vr_entry(cs, rels, src_col, dst_col, sources, source_id_col, targets, target_id_col, lower, upper,
                  out_source_col, out_reach_col, out, false);
}

extern "C" capf_status capf_var_length_reach_undirected(capf_session *cs, capf_table *rels, const char *src_col,
                                                        const char *dst_col, capf_table *sources,
                                                        const char *source_id_col, capf_table *targets,
                                                        const char *target_id_col, int32_t lower,
                                                        int32_t upper, const char *out_source_col,
                                                        const char *out_reach_col, capf_table **out) {
  return vr_entry(cs, rels, src_col, dst_col, sources, source_id_col, targets, target_id_col, lower, upper,
                  out_source_col, out_reach_col, out, true);
}
