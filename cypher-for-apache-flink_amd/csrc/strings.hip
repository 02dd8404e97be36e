// strings.hip — STARTS WITH / ENDS WITH / CONTAINS with a literal pattern,
// answered once per dictionary string (CAPF_OP_STR_MATCH's dictionary path).
//
// All rows holding the same subject code share one answer, so a literal
// pattern is matched against the session's device string heap (string_dict.h
// heap()) — one uint8 per dictionary code, 0 false / 1 true — and the
// prepared program looks the answer up by subject code.  The table is cached
// per (kind, pattern code) and, the dictionary being append-only, extended
// over the codes interned since (at most STR_MATCH_TABLES tables are kept,
// the oldest dropped first).
//
// Thread tier (k_str_match): one thread per dictionary string, the pattern
// staged once per block in LDS as words (a pattern longer than PAT_LDS_BYTES
// is read from the heap instead).  STARTS WITH and ENDS WITH compare at most
// the pattern's length, so this tier is all they need.
// Wave tier (k_str_contains_long): a CONTAINS thread that meets a subject of
// at least L bytes (CAPF_STR_LONG, default 256) does not scan it — one lane
// walking kilobytes while 63 idle — but appends its code to a worklist (one
// atomic counter; the compiler folds a wave's adds into one).  The second
// launch gives each listed string to one wave: lanes take the start positions
// lane, lane + 64, … (consecutive bytes across the wave, LONG_ILP strides in
// flight at a time), and the wave's answer is a ballot.  The counter is read
// back, and the launch skipped when the list is empty.
#include <algorithm>
#include <cstring>

#include "capf_internal.h"
#include "device_common.h"
#include "str_match.h"

namespace capf {

constexpr int SM_BLOCK = 256;
constexpr int64_t STR_LONG_DEFAULT = 256;
constexpr int LONG_ILP = 4;  // strides of 64 start positions a wave tests per ballot

__global__ __launch_bounds__(SM_BLOCK) void k_str_match(const int64_t *off, const uint8_t *bytes, int64_t c0,
                                                         int64_t c1, int kind, int64_t pcode, int64_t long_len,
                                                         uint8_t *table, int64_t *work, unsigned long long *nwork) {
  __shared__ uint32_t s_pat[PAT_LDS_BYTES / 4];
  const PatRef p = stage_pattern(off, bytes, pcode, s_pat);
  for (int64_t c = c0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < c1;
       c += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = off[c], slen = off[c + 1] - q;
    if (kind == 2 && p.len > 0 && slen >= p.len && slen >= long_len) {
      work[atomicAdd(nwork, 1ull)] = c;  // the wave tier's
      continue;
    }
    table[c] = str_match(kind, bytes, q, slen, p) ? 1 : 0;
  }
}

// One wave per listed string (each of at least the pattern's length ≥ 1).
__global__ __launch_bounds__(SM_BLOCK) void k_str_contains_long(const int64_t *off, const uint8_t *bytes, int64_t pcode,
                                                                 const int64_t *work, int64_t nwork, uint8_t *table) {
  __shared__ uint32_t s_pat[PAT_LDS_BYTES / 4];
  const PatRef p = stage_pattern(off, bytes, pcode, s_pat);
  const uint32_t first = pat_u32(bytes, p, 0), m0 = low_bytes(p.len);
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int64_t nwaves = (int64_t)gridDim.x * blockDim.x / WAVE;
  for (int64_t w = wave; w < nwork; w += nwaves) {
    const int64_t c = work[w], q = off[c], last = off[c + 1] - q - p.len;
    bool found = false;
    for (int64_t base = 0; base <= last && !found; base += WAVE * LONG_ILP) {
      // LONG_ILP strides of start positions per ballot: their first words are
      // loaded together (one stride per ballot left the wave waiting on one
      // load at a time); a position past the last reads nothing and mismatches
      uint32_t fw[LONG_ILP];
#pragma unroll
      for (int j = 0; j < LONG_ILP; ++j) {
        const int64_t k = base + j * WAVE + lane;
        fw[j] = k <= last ? heap_u32(bytes, q + k) : ~first;
      }
      bool hit = false;
#pragma unroll
      for (int j = 0; j < LONG_ILP; ++j)
        if (((fw[j] ^ first) & m0) == 0) hit |= match_at(bytes, q + base + j * WAVE + lane, p, 4);
      found = __ballot(hit) != 0ull;
    }
    if (lane == 0) table[c] = found ? 1 : 0;
  }
}

int64_t string_long_threshold() {
  const char *e = getenv("CAPF_STR_LONG");  // bytes from which a string is given to a wave
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? (int64_t)v : STR_LONG_DEFAULT;
}

// table[c] for the codes c0 ≤ c < c1
static void fill_match_table(Session *s, const StringHeap &h, int kind, int64_t pcode, int64_t c0, int64_t c1,
                             uint8_t *table) {
  const int64_t m = c1 - c0;
  const int64_t *off = (const int64_t *)h.off->p;
  const uint8_t *bytes = (const uint8_t *)h.bytes->p;
  BufPtr work, cnt;
  if (kind == 2) {
    work = s->alloc(8 * (size_t)m);
    cnt = s->alloc(8);
    HIP_CHECK(hipMemsetAsync(cnt->p, 0, 8, s->stream));
  }
  // profiled bytes: the strings' bytes, one offset and one answer per string
  double heap_bytes = 9.0 * (double)m;
  if (s->profiling) heap_bytes += s->dict.bytes_of(nullptr, c0, m, c1);
  {
    KernelTimer kt(s, "str_match", heap_bytes);
    hipLaunchKernelGGL(k_str_match, dim3(grid_for(m, SM_BLOCK)), dim3(SM_BLOCK), 0, s->stream, off, bytes, c0, c1,
                       kind, pcode, string_long_threshold(), table, work ? (int64_t *)work->p : nullptr,
                       cnt ? (unsigned long long *)cnt->p : nullptr);
    KERNEL_CHECK();
  }
  if (kind != 2) return;
  HIP_CHECK(hipMemcpyAsync(s->h_scalars, cnt->p, 8, hipMemcpyDeviceToHost, s->stream));
  s->sync();
  const int64_t nwork = s->h_scalars[0];
  if (nwork <= 0) return;
  KernelTimer kt(s, "str_contains_long", 8.0 * (double)nwork);
  const int waves_per_block = SM_BLOCK / WAVE;
  hipLaunchKernelGGL(k_str_contains_long, dim3(grid_for(nwork, waves_per_block)), dim3(SM_BLOCK), 0, s->stream, off,
                     bytes, pcode, (const int64_t *)work->p, nwork, table);
  KERNEL_CHECK();
}

// (match_mu held)
static StringDict::MatchTable *find_table(Session *s, int kind, int64_t pcode) {
  for (auto &t : s->dict.match_tables)
    if (t.kind == kind && t.pattern == pcode) return &t;
  return nullptr;
}

bool string_match_by_table(Session *s, int kind, int64_t pattern_code, int64_t nrows) {
  const char *mode = getenv("CAPF_STR_MATCH");
  if (mode && strcmp(mode, "rows") == 0) return false;
  if (mode && strcmp(mode, "dict") == 0) return true;
  const size_t n = s->dict.size();
  size_t covered = 0;
  {
    std::lock_guard<std::mutex> lk(s->dict.match_mu);
    if (const auto *t = find_table(s, kind, pattern_code)) covered = t->n;
  }
  return (int64_t)(n - std::min(n, covered)) <= nrows;
}

BufPtr string_match_table(Session *s, int kind, int64_t pattern_code, size_t *n_out) {
  const StringHeap h = s->dict.heap();
  const size_t n = h.n;
  if (kind < 0 || kind > 2) illegal("string predicate kind out of range");
  if (pattern_code < 0 || (size_t)pattern_code >= n) illegal("unknown string code");
  std::lock_guard<std::mutex> lk(s->dict.match_mu);
  auto &tables = s->dict.match_tables;
  if (!find_table(s, kind, pattern_code)) {
    if (tables.size() >= STR_MATCH_TABLES) tables.erase(tables.begin());
    tables.push_back(StringDict::MatchTable{kind, pattern_code, nullptr, 0, 0});
  }
  StringDict::MatchTable &t = *find_table(s, kind, pattern_code);
  if (n > t.n) {
    s->dict.reserve(t.buf, t.cap, n, 4096, 1, t.n);  // the answers so far move with it
    fill_match_table(s, h, kind, pattern_code, (int64_t)t.n, (int64_t)n, (uint8_t *)t.buf->p);
    t.n = n;
  }
  *n_out = t.n;
  return t.buf;
}

}  // namespace capf
