// string_fn.hip — toUpper / toLower / trim / lTrim / rTrim / substring /
// replace / s + 'lit' / 'lit' + s with literal arguments, evaluated on the
// device string heap (string_dict.h heap()) and interned there
// (capf_string_fn_codes).
//
// The input is a worklist of n source codes: a range of the dictionary or a
// device array.  Two passes with an exclusive prefix sum in between:
//   length pass  each source gets a status (bytes / identity / host / NULL),
//                a result length and the source byte its result starts at;
//   write pass   the bytes of every result that has some go to a scratch heap
//                of the string heap's layout (offsets + padded bytes).
// Identity (the result equals the source) answers with the source's code;
// host (non-ASCII case mapping, substring over a supplementary character,
// replace in a long subject) is left to the caller, −2.
//
// Tiers, as in strings.hip.  Thread tier: one thread per source.  Wave tier: a
// source of at least L bytes (CAPF_STR_LONG, default 256) is appended to a
// worklist (one atomic counter, read back; the second launch is skipped when
// it is empty) and measured by one wave — lanes take consecutive words or
// bytes, trim's bounds and substring's unit positions come from ballots; a
// result of at least L bytes is copied by one wave likewise.  replace walks
// its subject sequentially, so a long subject is the host's.
//
// Interning: a hash index of the dictionary (StringDict::Index: open-addressed
// table of codes keyed by a 64-bit hash of the bytes, at most half full) is
// probed with each result, a hit confirmed by comparing bytes.  Results not
// found are grouped among themselves in a scratch table of worklist
// positions; once a result's slot is settled it lowers the slot's
// representative with an atomicMin of its position, and a prefix sum over the
// representatives ranks them: new codes ascend in the order of the smallest
// position producing each string, whatever the order the threads ran in.
// The interning is one function (intern_results) with three callers: the string
// functions above, split(subject, delimiter) per table row
// (capf_table_str_split), whose kernels and byte formulas are at the end, and
// the STRING fields of the typed CSV parser (edge_list.hip).
#include <algorithm>
#include <cstring>

#include "capf_internal.h"
#include "device_common.h"
#include "str_match.h"

namespace capf {

constexpr int SF_BLOCK = 256;
constexpr int64_t SF_EMPTY = -1;
constexpr int64_t SF_NEW = -3;  // out[i] between the probe and the assignment: not in the dictionary
// (the result statuses ST_* are capf_internal.h's: intern_results is called from edge_list.hip too)

struct FnArgs {
  int32_t fn;
  int64_t from, len;   // substring
  int64_t lit0, lit1;  // dictionary codes
};

__device__ inline int64_t item_code(const int64_t *src, int64_t c0, int64_t i) { return src ? src[i] : c0 + i; }

// ------------------------------------------------------------ bytes and words
// ASCII words (every byte < 0x80): 0x80 in each byte that is a lower-case /
// upper-case letter.  A byte >= 0x80 past the string's end may carry into the
// bytes above it — also past the end, and masked off by the caller.
__device__ inline uint32_t lower_mask(uint32_t w) { return (w + 0x1F1F1F1Fu) & ~(w + 0x05050505u) & 0x80808080u; }
__device__ inline uint32_t upper_mask(uint32_t w) { return (w + 0x3F3F3F3Fu) & ~(w + 0x25252525u) & 0x80808080u; }
// xf: 0 copy, 1 to upper, 2 to lower
__device__ inline uint32_t xform_word(uint32_t w, int xf) {
  if (xf == 1) return w - (lower_mask(w) >> 2);
  if (xf == 2) return w + (upper_mask(w) >> 2);
  return w;
}
__device__ inline uint8_t xform_byte(uint8_t b, int xf) {
  if (xf == 1 && b >= 'a' && b <= 'z') return b - 32;
  if (xf == 2 && b >= 'A' && b <= 'Z') return b + 32;
  return b;
}
// 0x01 in each byte that is not a UTF-8 continuation byte (10xxxxxx)
__device__ inline uint32_t unit_starts(uint32_t w) { return ~((w >> 7) & ~(w >> 6)) & 0x01010101u; }
// 0x80 in each byte >= 0xF0 (the lead of a 4-byte sequence: a surrogate pair)
__device__ inline uint32_t lead4(uint32_t w) { return w & (w << 1) & (w << 2) & (w << 3) & 0x80808080u; }

// n bytes src[sp ..) → dst[d ..), one thread: bytes up to dst's next word, whole words, bytes
__device__ inline void copy_thread(uint8_t *dst, int64_t d, const uint8_t *src, int64_t sp, int64_t n, int xf) {
  while (n > 0 && (d & 3)) {
    dst[d++] = xform_byte(src[sp++], xf);
    --n;
  }
  for (; n >= 4; n -= 4, d += 4, sp += 4) *(uint32_t *)(dst + d) = xform_word(heap_u32(src, sp), xf);
  for (; n > 0; --n) dst[d++] = xform_byte(src[sp++], xf);
}

// The same by one wave: lanes take consecutive words of dst.
__device__ inline void copy_wave(uint8_t *dst, int64_t d, const uint8_t *src, int64_t sp, int64_t n, int xf,
                                 int lane) {
  const int64_t head = min(n, (int64_t)((4 - (d & 3)) & 3));
  if (lane < head) dst[d + lane] = xform_byte(src[sp + lane], xf);
  const int64_t nw = (n - head) >> 2, tail = (n - head) & 3;
  for (int64_t j = lane; j < nw; j += WAVE)
    *(uint32_t *)(dst + d + head + 4 * j) = xform_word(heap_u32(src, sp + head + 4 * j), xf);
  if (lane < tail) dst[d + head + 4 * nw + lane] = xform_byte(src[sp + head + 4 * nw + lane], xf);
}

// a[qa, qa + n) == b[qb, qb + n)
__device__ inline bool bytes_equal(const uint8_t *a, int64_t qa, const uint8_t *b, int64_t qb, int64_t n) {
  for (int64_t i = 0; i < n; i += 4)
    if ((heap_u32(a, qa + i) ^ heap_u32(b, qb + i)) & low_bytes(n - i)) return false;
  return true;
}

// 64-bit hash of bytes[q, q + n): a sum of mixed (word, position) pairs, so
// the words may be taken in any order
__device__ inline uint64_t hash_bytes(const uint8_t *bytes, int64_t q, int64_t n) {
  uint64_t h = fmix64((uint64_t)n + 0x9E3779B97F4A7C15ull);
  for (int64_t i = 0; i < n; i += 4)
    h += fmix64((uint64_t)(heap_u32(bytes, q + i) & low_bytes(n - i)) | (uint64_t)((i >> 2) + 1) << 32);
  return h;
}

// substring's unit range [u0, u1) of a string of lc UTF-16 units (Calcite's
// SUBSTRING(s, from, for), 1-based from, negative from the end): false = empty
__device__ inline bool substring_units(int64_t from, int64_t len, int64_t lc, int64_t *u0, int64_t *u1) {
  if (from < 0) from += lc + 1;
  const int64_t e = from + len;
  if (from > lc || e < 1) return false;
  const int64_t s1 = max(from, (int64_t)1), e1 = min(e, lc + 1);
  if (e1 <= s1) return false;
  *u0 = s1 - 1;
  *u1 = e1 - 1;
  return true;
}

// ------------------------------------------------------------ length pass
// Thread tier: status, result length and start of item i; a long source goes
// on the worklist (replace: to the host).
__global__ __launch_bounds__(SF_BLOCK) void k_fn_len(const int64_t *off, const uint8_t *bytes, const int64_t *src,
                                                      int64_t c0, int64_t n, FnArgs a, int64_t long_len, uint8_t *st,
                                                      int64_t *len, int64_t *start, int64_t *work,
                                                      unsigned long long *nwork) {
  __shared__ uint32_t s_pat[PAT_LDS_BYTES / 4];
  PatRef p{nullptr, 0, 0};
  int64_t l0 = 0, l1 = 0;
  if (a.fn == CAPF_STR_FN_REPLACE) {
    p = stage_pattern(off, bytes, a.lit0, s_pat);
    l1 = off[a.lit1 + 1] - off[a.lit1];
  } else if (a.fn == CAPF_STR_FN_CONCAT_L || a.fn == CAPF_STR_FN_CONCAT_R) {
    l0 = off[a.lit0 + 1] - off[a.lit0];
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = item_code(src, c0, i);
    uint8_t status = ST_BYTES;
    int64_t rlen = 0, rstart = 0;
    if (c < 0) {
      status = ST_NULL;
    } else {
      const int64_t q = off[c], slen = off[c + 1] - q;
      if (a.fn == CAPF_STR_FN_CONCAT_L || a.fn == CAPF_STR_FN_CONCAT_R) {
        rlen = slen + l0;
        if (l0 == 0) status = ST_IDENT;
      } else if (slen >= long_len) {
        if (a.fn == CAPF_STR_FN_REPLACE) {
          status = ST_HOST;
        } else {
          status = ST_LONG;
          work[atomicAdd(nwork, 1ull)] = i;
        }
      } else if (a.fn == CAPF_STR_FN_UPPER || a.fn == CAPF_STR_FN_LOWER) {
        uint32_t high = 0, changed = 0;
        for (int64_t k = 0; k < slen; k += 4) {
          const uint32_t w = heap_u32(bytes, q + k), m = low_bytes(slen - k);
          high |= w & m & 0x80808080u;
          changed |= (a.fn == CAPF_STR_FN_UPPER ? lower_mask(w) : upper_mask(w)) & m;
        }
        rlen = slen;
        status = high ? ST_HOST : changed ? ST_BYTES : ST_IDENT;
      } else if (a.fn <= CAPF_STR_FN_RTRIM) {  // TRIM / LTRIM / RTRIM
        int64_t b = 0, e = slen;
        if (a.fn != CAPF_STR_FN_RTRIM)
          while (b < e && bytes[q + b] == 0x20) ++b;
        if (a.fn != CAPF_STR_FN_LTRIM)
          while (e > b && bytes[q + e - 1] == 0x20) --e;
        rlen = e - b;
        rstart = rlen ? b : 0;
        if (rlen == slen) status = ST_IDENT;
      } else if (a.fn == CAPF_STR_FN_SUBSTRING) {
        int64_t lc = 0;
        uint32_t four = 0;
        for (int64_t k = 0; k < slen; k += 4) {
          const uint32_t w = heap_u32(bytes, q + k), m = low_bytes(slen - k);
          four |= lead4(w) & m;
          lc += __popc(unit_starts(w) & m);
        }
        int64_t u0 = 0, u1 = 0;
        if (four) {
          status = ST_HOST;
        } else if (substring_units(a.from, a.len, lc, &u0, &u1)) {
          // the bytes at which units u0 and u1 start (u1 = lc: the end)
          int64_t b0 = slen, b1 = slen, u = 0;
          for (int64_t k = 0; k < slen; ++k) {
            if ((bytes[q + k] & 0xC0) == 0x80) continue;
            if (u == u0) b0 = k;
            if (u == u1) {
              b1 = k;
              break;
            }
            ++u;
          }
          rstart = b0;
          rlen = b1 - b0;
          if (rlen == slen) status = ST_IDENT;
        }
      } else {  // REPLACE: leftmost non-overlapping occurrences
        int64_t hits = 0;
        for (int64_t k = 0; k + p.len <= slen;) {
          if (match_at(bytes, q + k, p)) {
            ++hits;
            k += p.len;
          } else {
            ++k;
          }
        }
        rlen = slen + hits * (l1 - p.len);
        if (hits == 0) status = ST_IDENT;
      }
    }
    st[i] = status;
    len[i] = status == ST_BYTES ? rlen : 0;
    start[i] = rstart;
  }
}

// The byte at which unit u of bytes[q, q + slen) starts (slen when it has no
// more than u units), by one wave: 64 bytes per ballot.
__device__ inline int64_t wave_unit_pos(const uint8_t *bytes, int64_t q, int64_t slen, int64_t u, int lane) {
  int64_t seen = 0;
  for (int64_t base = 0; base < slen; base += WAVE) {
    const bool is_start = base + lane < slen && (bytes[q + base + lane] & 0xC0) != 0x80;
    const uint64_t m = __ballot(is_start);
    const int cnt = __popcll(m);
    if (seen + cnt > u) {
      const uint64_t at = __ballot(is_start && __popcll(m & ((1ull << lane) - 1ull)) == u - seen);
      return base + (__ffsll((unsigned long long)at) - 1);
    }
    seen += cnt;
  }
  return slen;
}

// Wave tier of the length pass: one wave per listed item (a source of at
// least long_len bytes; UPPER / LOWER / the TRIMs / SUBSTRING).
__global__ __launch_bounds__(SF_BLOCK) void k_fn_long_len(const int64_t *off, const uint8_t *bytes,
                                                           const int64_t *src, int64_t c0, FnArgs a,
                                                           const int64_t *work, int64_t nwork, uint8_t *st,
                                                           int64_t *len, int64_t *start) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int64_t nwaves = (int64_t)gridDim.x * blockDim.x / WAVE;
  for (int64_t wi = wave; wi < nwork; wi += nwaves) {
    const int64_t i = work[wi], c = item_code(src, c0, i), q = off[c], slen = off[c + 1] - q;
    uint8_t status = ST_BYTES;
    int64_t rlen = 0, rstart = 0;
    if (a.fn == CAPF_STR_FN_UPPER || a.fn == CAPF_STR_FN_LOWER) {
      uint32_t high = 0, changed = 0;
      for (int64_t k = 4 * (int64_t)lane; k < slen; k += 4 * WAVE) {
        const uint32_t w = heap_u32(bytes, q + k), m = low_bytes(slen - k);
        high |= w & m & 0x80808080u;
        changed |= (a.fn == CAPF_STR_FN_UPPER ? lower_mask(w) : upper_mask(w)) & m;
      }
      rlen = slen;
      status = __ballot(high != 0) ? ST_HOST : __ballot(changed != 0) ? ST_BYTES : ST_IDENT;
    } else if (a.fn <= CAPF_STR_FN_RTRIM) {
      int64_t b = 0, e = slen;
      if (a.fn != CAPF_STR_FN_RTRIM) {  // the first byte that is no space
        b = slen;
        for (int64_t base = 0; base < slen; base += WAVE) {
          const uint64_t m = __ballot(base + lane < slen && bytes[q + base + lane] != 0x20);
          if (m) {
            b = base + (__ffsll((unsigned long long)m) - 1);
            break;
          }
        }
      }
      if (a.fn != CAPF_STR_FN_LTRIM) {  // the last one, from the end
        e = b;
        for (int64_t base = 0; base < slen - b; base += WAVE) {
          const int64_t k = slen - 1 - base - lane;
          const uint64_t m = __ballot(k >= b && bytes[q + k] != 0x20);
          if (m) {
            e = slen - base - (__ffsll((unsigned long long)m) - 1);
            break;
          }
        }
      }
      rlen = e - b;
      rstart = rlen ? b : 0;
      if (rlen == slen) status = ST_IDENT;
    } else {  // SUBSTRING
      int64_t lc = 0;
      uint32_t four = 0;
      for (int64_t k = 4 * (int64_t)lane; k < slen; k += 4 * WAVE) {
        const uint32_t w = heap_u32(bytes, q + k), m = low_bytes(slen - k);
        four |= lead4(w) & m;
        lc += __popc(unit_starts(w) & m);
      }
      lc = wave_reduce_sum((int)lc);
      int64_t u0 = 0, u1 = 0;
      if (__ballot(four != 0)) {
        status = ST_HOST;
      } else if (substring_units(a.from, a.len, lc, &u0, &u1)) {
        const int64_t b0 = wave_unit_pos(bytes, q, slen, u0, lane);
        const int64_t b1 = u1 >= lc ? slen : wave_unit_pos(bytes, q, slen, u1, lane);
        rstart = b0;
        rlen = b1 - b0;
        if (rlen == slen) status = ST_IDENT;
      }
    }
    if (lane == 0) {
      st[i] = status;
      len[i] = status == ST_BYTES ? rlen : 0;
      start[i] = rstart;
    }
  }
}

// ------------------------------------------------------------ write pass
// The result of item i as two pieces of the heap: (p0, n0, transformed) then (p1, n1).
struct Pieces {
  int64_t p0, n0, p1, n1;
  int xf;
};
__device__ inline Pieces result_pieces(const int64_t *off, const FnArgs &a, int64_t c, int64_t rlen, int64_t rstart) {
  const int64_t q = off[c];
  if (a.fn == CAPF_STR_FN_CONCAT_L) return Pieces{off[a.lit0], off[a.lit0 + 1] - off[a.lit0], q, off[c + 1] - q, 0};
  if (a.fn == CAPF_STR_FN_CONCAT_R) return Pieces{q, off[c + 1] - q, off[a.lit0], off[a.lit0 + 1] - off[a.lit0], 0};
  return Pieces{q + rstart, rlen, 0, 0, a.fn == CAPF_STR_FN_UPPER ? 1 : a.fn == CAPF_STR_FN_LOWER ? 2 : 0};
}

// Thread tier: the bytes of every result that has some, to rbytes[roff[i] ..);
// a result of at least long_len bytes goes on the worklist (not replace's,
// whose subject is short).
__global__ __launch_bounds__(SF_BLOCK) void k_fn_write(const int64_t *off, const uint8_t *bytes, const int64_t *src,
                                                        int64_t c0, int64_t n, FnArgs a, int64_t long_len,
                                                        const uint8_t *st, const int64_t *roff, const int64_t *start,
                                                        uint8_t *rbytes, int64_t *work, unsigned long long *nwork) {
  __shared__ uint32_t s_pat[PAT_LDS_BYTES / 4];
  PatRef p{nullptr, 0, 0};
  int64_t r0 = 0, l1 = 0;
  if (a.fn == CAPF_STR_FN_REPLACE) {
    p = stage_pattern(off, bytes, a.lit0, s_pat);
    r0 = off[a.lit1];
    l1 = off[a.lit1 + 1] - r0;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t d = roff[i], rlen = roff[i + 1] - d;
    if (st[i] != ST_BYTES || rlen == 0) continue;
    const int64_t c = item_code(src, c0, i);
    if (a.fn == CAPF_STR_FN_REPLACE) {
      const int64_t q = off[c], slen = off[c + 1] - q;
      int64_t w = d;
      for (int64_t k = 0; k < slen;) {
        if (k + p.len <= slen && match_at(bytes, q + k, p)) {
          for (int64_t j = 0; j < l1; ++j) rbytes[w++] = bytes[r0 + j];
          k += p.len;
        } else {
          rbytes[w++] = bytes[q + k++];
        }
      }
      continue;
    }
    if (rlen >= long_len) {
      work[atomicAdd(nwork, 1ull)] = i;
      continue;
    }
    const Pieces pc = result_pieces(off, a, c, rlen, start[i]);
    copy_thread(rbytes, d, bytes, pc.p0, pc.n0, pc.xf);
    copy_thread(rbytes, d + pc.n0, bytes, pc.p1, pc.n1, 0);
  }
}

// Wave tier: one wave copies (and transforms) each listed result.
__global__ __launch_bounds__(SF_BLOCK) void k_fn_long(const int64_t *off, const uint8_t *bytes, const int64_t *src,
                                                       int64_t c0, FnArgs a, const int64_t *work, int64_t nwork,
                                                       const int64_t *roff, const int64_t *start, uint8_t *rbytes) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int64_t nwaves = (int64_t)gridDim.x * blockDim.x / WAVE;
  for (int64_t wi = wave; wi < nwork; wi += nwaves) {
    const int64_t i = work[wi], d = roff[i];
    const Pieces pc = result_pieces(off, a, item_code(src, c0, i), roff[i + 1] - d, start[i]);
    copy_wave(rbytes, d, bytes, pc.p0, pc.n0, pc.xf, lane);
    copy_wave(rbytes, d + pc.n0, bytes, pc.p1, pc.n1, 0, lane);
  }
}

// ------------------------------------------------------------ index
// hashes[i] of the strings i0 ≤ i < i1 of a heap
__global__ __launch_bounds__(SF_BLOCK) void k_str_hash(const int64_t *off, const uint8_t *bytes, int64_t i0,
                                                        int64_t i1, uint64_t *hashes) {
  for (int64_t i = i0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < i1;
       i += (int64_t)gridDim.x * blockDim.x)
    hashes[i] = hash_bytes(bytes, off[i], off[i + 1] - off[i]);
}

// The (distinct) dictionary codes c0 ≤ c < c1 into the table.
__global__ __launch_bounds__(SF_BLOCK) void k_idx_insert(int64_t *tab, uint64_t mask, const uint64_t *hashes,
                                                          int64_t c0, int64_t c1) {
  for (int64_t c = c0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < c1;
       c += (int64_t)gridDim.x * blockDim.x) {
    uint64_t slot = hashes[c] & mask;
    while (atomicCAS((unsigned long long *)&tab[slot], (unsigned long long)SF_EMPTY, (unsigned long long)c) !=
           (unsigned long long)SF_EMPTY)
      slot = (slot + 1) & mask;
  }
}

// out[i]: NULL, host and identity answered; a result with bytes looked up in
// the dictionary's index (its code, or SF_NEW).
__global__ __launch_bounds__(SF_BLOCK) void k_fn_probe(const int64_t *tab, uint64_t mask, const uint64_t *dhash,
                                                        const int64_t *off, const uint8_t *bytes, const int64_t *src,
                                                        int64_t c0, int64_t n, const uint8_t *st,
                                                        const uint64_t *rhash, const int64_t *roff,
                                                        const uint8_t *rbytes, int64_t *out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint8_t status = st[i];
    if (status != ST_BYTES) {
      out[i] = status == ST_NULL ? -1 : status == ST_IDENT ? item_code(src, c0, i) : -2;
      continue;
    }
    const uint64_t h = rhash[i];
    const int64_t d = roff[i], rlen = roff[i + 1] - d;
    int64_t found = SF_NEW;
    for (uint64_t slot = h & mask;; slot = (slot + 1) & mask) {
      const int64_t c = tab[slot];
      if (c == SF_EMPTY) break;
      if (dhash[c] == h && off[c + 1] - off[c] == rlen && bytes_equal(bytes, off[c], rbytes, d, rlen)) {
        found = c;
        break;
      }
    }
    out[i] = found;
  }
}

// The results not in the dictionary, grouped by their bytes: grp[i] = the slot
// of i's string in the scratch table tab2 (of positions), rep[slot] lowered to
// the smallest position of the group once the slot is settled.
__global__ __launch_bounds__(SF_BLOCK) void k_fn_group(int64_t *tab2, uint64_t mask2, unsigned long long *rep,
                                                        int64_t n, const int64_t *out, const uint64_t *rhash,
                                                        const int64_t *roff, const uint8_t *rbytes, int64_t *grp) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (out[i] != SF_NEW) continue;
    const uint64_t h = rhash[i];
    const int64_t d = roff[i], rlen = roff[i + 1] - d;
    uint64_t slot = h & mask2;
    for (;; slot = (slot + 1) & mask2) {
      const int64_t cur = (int64_t)atomicCAS((unsigned long long *)&tab2[slot], (unsigned long long)SF_EMPTY,
                                             (unsigned long long)i);
      if (cur == SF_EMPTY) break;  // the slot is this string's from now on
      if (rhash[cur] == h && roff[cur + 1] - roff[cur] == rlen && bytes_equal(rbytes, roff[cur], rbytes, d, rlen))
        break;
    }
    grp[i] = (int64_t)slot;
    atomicMin(&rep[slot], (unsigned long long)i);
  }
}

// flag[i] = 1 where i is its group's representative
__global__ __launch_bounds__(SF_BLOCK) void k_fn_rep_flags(int64_t n, const int64_t *out, const int64_t *grp,
                                                            const unsigned long long *rep, int64_t *flag) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    flag[i] = out[i] == SF_NEW && rep[grp[i]] == (unsigned long long)i ? 1 : 0;
}

// out[i] = code0 + the rank of i's representative; the representatives'
// positions and lengths listed by rank
__global__ __launch_bounds__(SF_BLOCK) void k_fn_assign(int64_t n, int64_t code0, const int64_t *grp,
                                                         const unsigned long long *rep, const int64_t *rank,
                                                         const int64_t *roff, int64_t *out, int64_t *items,
                                                         int64_t *nlen) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (out[i] != SF_NEW) continue;
    const int64_t r = (int64_t)rep[grp[i]], k = rank[r];
    out[i] = code0 + k;
    if (r == i) {
      items[k] = i;
      nlen[k] = roff[i + 1] - roff[i];
    }
  }
}

// The new strings back to back, as the heap will hold them: word j of the
// staged bytes (its strings found by bisection of the new offsets noff), and
// the absolute end offset of new string j.
__global__ __launch_bounds__(SF_BLOCK) void k_fn_stage(int64_t n_new, int64_t nb, int64_t base, const int64_t *noff,
                                                        const int64_t *items, const int64_t *roff,
                                                        const uint8_t *rbytes, int64_t *soffs, uint8_t *sbytes) {
  const int64_t nwords = (nb + 3) >> 2, total = max(nwords, n_new);
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
    if (j < n_new) soffs[j] = base + noff[j + 1];
    if (j >= nwords) continue;
    int64_t lo = 0, hi = n_new - 1;  // the last string starting at or before byte 4 j
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (noff[mid] <= 4 * j) lo = mid; else hi = mid - 1;
    }
    uint32_t w = 0;
    for (int b = 0; b < 4; ++b) {
      const int64_t pos = 4 * j + b;
      if (pos >= nb) break;
      while (pos >= noff[lo + 1]) ++lo;
      w |= (uint32_t)rbytes[roff[items[lo]] + pos - noff[lo]] << (8 * b);
    }
    *(uint32_t *)(sbytes + 4 * j) = w;
  }
}

// ------------------------------------------------------------ host
static uint64_t pow2_at_least(uint64_t x) {
  uint64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

constexpr size_t IDX_MIN_SLOTS = 1 << 12;

// The index over the heap's n strings (index_mu held).
static void ensure_index(Session *s, const StringHeap &h, size_t n) {
  StringDict::Index &ix = s->dict.index;
  if (n <= ix.n && ix.tab) return;
  const int64_t *off = (const int64_t *)h.off->p;
  const uint8_t *bytes = (const uint8_t *)h.bytes->p;
  // the hashes so far move with it; an empty dictionary (the typed CSV parser may be the first to
  // intern anything) still gets a buffer: the probe takes its address
  s->dict.reserve(ix.hashes, ix.hash_cap, std::max<size_t>(n, 1), 4096, 8, ix.n);
  const int64_t m = (int64_t)(n - ix.n);
  if (m > 0) {
    double by = 16.0 * (double)m;  // the strings' bytes, one offset and one hash per string
    if (s->profiling) by += s->dict.bytes_of(nullptr, (int64_t)ix.n, m, (int64_t)n);
    KernelTimer kt(s, "str_idx_hash", by);
    hipLaunchKernelGGL(k_str_hash, dim3(grid_for(m, SF_BLOCK)), dim3(SF_BLOCK), 0, s->stream, off, bytes,
                       (int64_t)ix.n, (int64_t)n, (uint64_t *)ix.hashes->p);
    KERNEL_CHECK();
  }
  int64_t first = (int64_t)ix.n;
  const bool rebuild = !ix.tab || 2 * n > ix.slots;
  if (rebuild) {  // past half full: a table of four slots per string, every code again
    ix.slots = std::max<size_t>((size_t)pow2_at_least(4 * (uint64_t)n), IDX_MIN_SLOTS);
    ix.tab = s->alloc(8 * ix.slots);
    HIP_CHECK(hipMemsetAsync(ix.tab->p, 0xFF, 8 * ix.slots, s->stream));
    first = 0;
  }
  if ((int64_t)n > first) {
    KernelTimer kt(s, rebuild ? "str_idx_build" : "str_idx_extend", 16.0 * (double)((int64_t)n - first));
    hipLaunchKernelGGL(k_idx_insert, dim3(grid_for((int64_t)n - first, SF_BLOCK)), dim3(SF_BLOCK), 0, s->stream,
                       (int64_t *)ix.tab->p, (uint64_t)ix.slots - 1, (const uint64_t *)ix.hashes->p, first,
                       (int64_t)n);
    KERNEL_CHECK();
  }
  ix.n = n;
}

static int64_t read_counter(Session *s, const BufPtr &cnt) {
  HIP_CHECK(hipMemcpyAsync(s->h_scalars, cnt->p, 8, hipMemcpyDeviceToHost, s->stream));
  s->sync();
  return s->h_scalars[0];
}

// ------------------------------------------------------------ interning
// The n results of a device step — statuses st, the bytes rbytes[roff[i],
// roff[i + 1]) of a scratch heap of `total` bytes — interned against the n0
// strings of the heap snapshot h (index_mu held).  Returns the device codes:
// −1 NULL, −2 host, the source's code (dsrc / c0) for an identity, else the
// code of the result's bytes.  New strings are appended to the heap and the
// dictionary, their codes ascending by the smallest position producing each.
// `out` non-null: the codes go to the host too, in the step's one
// synchronisation; null: they stay on the device (split's element column).
BufPtr intern_results(Session *s, const StringHeap &h, size_t n0, const int64_t *dsrc, int64_t c0, int64_t n,
                             const BufPtr &st, const BufPtr &roff, const BufPtr &rbytes, int64_t total,
                             int64_t *out) {
  const int64_t *off = (const int64_t *)h.off->p;
  const uint8_t *bytes = (const uint8_t *)h.bytes->p;
  const dim3 grid(grid_for(n, SF_BLOCK)), block(SF_BLOCK);
  ensure_index(s, h, n0);
  const StringDict::Index &ix = s->dict.index;
  BufPtr rhash = s->alloc(8 * (size_t)n), d_out = s->alloc(8 * (size_t)n), grp = s->alloc(8 * (size_t)n);
  {
    KernelTimer kt(s, "str_fn_hash", (double)total + 16.0 * (double)n);
    hipLaunchKernelGGL(k_str_hash, grid, block, 0, s->stream, (const int64_t *)roff->p, (const uint8_t *)rbytes->p,
                       (int64_t)0, n, (uint64_t *)rhash->p);
    KERNEL_CHECK();
  }
  {
    KernelTimer kt(s, "str_fn_probe", (double)total + 33.0 * (double)n);
    hipLaunchKernelGGL(k_fn_probe, grid, block, 0, s->stream, (const int64_t *)ix.tab->p, (uint64_t)ix.slots - 1,
                       (const uint64_t *)ix.hashes->p, off, bytes, dsrc, c0, n, (const uint8_t *)st->p,
                       (const uint64_t *)rhash->p, (const int64_t *)roff->p, (const uint8_t *)rbytes->p,
                       (int64_t *)d_out->p);
    KERNEL_CHECK();
  }
  const size_t slots2 = (size_t)pow2_at_least(2 * (uint64_t)n);
  BufPtr tab2 = s->alloc(8 * slots2), rep = s->alloc(8 * slots2), flag = s->alloc(8 * (size_t)n),
         rank = s->alloc(8 * (size_t)n);
  HIP_CHECK(hipMemsetAsync(tab2->p, 0xFF, 8 * slots2, s->stream));
  HIP_CHECK(hipMemsetAsync(rep->p, 0xFF, 8 * slots2, s->stream));
  {
    KernelTimer kt(s, "str_fn_group", (double)total + 40.0 * (double)n);
    hipLaunchKernelGGL(k_fn_group, grid, block, 0, s->stream, (int64_t *)tab2->p, (uint64_t)slots2 - 1,
                       (unsigned long long *)rep->p, n, (const int64_t *)d_out->p, (const uint64_t *)rhash->p,
                       (const int64_t *)roff->p, (const uint8_t *)rbytes->p, (int64_t *)grp->p);
    KERNEL_CHECK();
    hipLaunchKernelGGL(k_fn_rep_flags, grid, block, 0, s->stream, n, (const int64_t *)d_out->p,
                       (const int64_t *)grp->p, (const unsigned long long *)rep->p, (int64_t *)flag->p);
    KERNEL_CHECK();
  }
  const int64_t n_new = exclusive_scan_i64(s, (const int64_t *)flag->p, (int64_t *)rank->p, n);
  std::vector<int64_t> codes;
  if (n_new > 0) {
    BufPtr items = s->alloc(8 * (size_t)n_new), nlen = s->alloc(8 * (size_t)(n_new + 1)),
           noff = s->alloc(8 * (size_t)(n_new + 1));
    HIP_CHECK(hipMemsetAsync((int64_t *)nlen->p + n_new, 0, 8, s->stream));
    hipLaunchKernelGGL(k_fn_assign, grid, block, 0, s->stream, n, (int64_t)n0, (const int64_t *)grp->p,
                       (const unsigned long long *)rep->p, (const int64_t *)rank->p, (const int64_t *)roff->p,
                       (int64_t *)d_out->p, (int64_t *)items->p, (int64_t *)nlen->p);
    KERNEL_CHECK();
    const int64_t nb = exclusive_scan_i64(s, (const int64_t *)nlen->p, (int64_t *)noff->p, n_new + 1);
    // staged as the heap will hold them: [n_new end offsets][nb bytes], one copy to the host
    const size_t sbytes_at = 8 * (size_t)n_new, stage_size = sbytes_at + (((size_t)nb + 3) & ~(size_t)3);
    BufPtr stage = s->alloc(stage_size + 8);
    {
      KernelTimer kt(s, "str_fn_append", 2.0 * (double)nb + 24.0 * (double)n_new);
      hipLaunchKernelGGL(k_fn_stage, dim3(grid_for(std::max<int64_t>((nb + 3) / 4, n_new), SF_BLOCK)), block, 0,
                         s->stream, n_new, nb, h.nbytes, (const int64_t *)noff->p, (const int64_t *)items->p,
                         (const int64_t *)roff->p, (const uint8_t *)rbytes->p, (int64_t *)stage->p,
                         (uint8_t *)stage->p + sbytes_at);
      KERNEL_CHECK();
    }
    std::vector<char> host(stage_size);
    HIP_CHECK(hipMemcpyAsync(host.data(), stage->p, stage_size, hipMemcpyDeviceToHost, s->stream));
    if (out) HIP_CHECK(hipMemcpyAsync(out, d_out->p, 8 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    s->sync();
    s->dict.heap_append(h, (const int64_t *)stage->p, (const uint8_t *)stage->p + sbytes_at,
                        (const int64_t *)host.data(), host.data() + sbytes_at, n_new, nb, codes);
    // codes other than n0 + rank: another thread interned meanwhile (the host map resolved them)
    bool moved = false;
    for (int64_t r = 0; r < n_new; ++r) moved |= codes[(size_t)r] != (int64_t)n0 + r;
    if (moved) {
      std::vector<int64_t> tmp;
      int64_t *o = out;
      if (!o) {  // the device codes take the same correction, through the host
        tmp.resize((size_t)n);
        o = tmp.data();
        HIP_CHECK(hipMemcpyAsync(o, d_out->p, 8 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
        s->sync();
      }
      for (int64_t i = 0; i < n; ++i)
        if (o[i] >= (int64_t)n0) o[i] = codes[(size_t)(o[i] - (int64_t)n0)];
      if (!out) {
        HIP_CHECK(hipMemcpyAsync(d_out->p, o, 8 * (size_t)n, hipMemcpyHostToDevice, s->stream));
        s->sync();  // (pageable source)
      }
    }
    return d_out;
  }
  if (out) {
    HIP_CHECK(hipMemcpyAsync(out, d_out->p, 8 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    s->sync();
  }
  return d_out;
}

void string_fn_codes(Session *s, int32_t fn, int64_t iarg0, int64_t iarg1, int64_t lit0, int64_t lit1,
                     const int64_t *src, int64_t c0, int64_t n, int64_t *out) {
  if (fn < CAPF_STR_FN_UPPER || fn > CAPF_STR_FN_REPLACE) illegal("unknown string function");
  if (fn == CAPF_STR_FN_SUBSTRING && iarg1 < 0) illegal("negative substring length");
  std::lock_guard<std::mutex> index_lock(s->dict.index_mu);
  const StringHeap h = s->dict.heap();  // the snapshot the whole step works against
  const size_t n0 = h.n;
  const bool concat = fn == CAPF_STR_FN_CONCAT_L || fn == CAPF_STR_FN_CONCAT_R;
  if ((concat || fn == CAPF_STR_FN_REPLACE) && (lit0 < 0 || (size_t)lit0 >= n0)) illegal("unknown string code");
  if (fn == CAPF_STR_FN_REPLACE && (lit1 < 0 || (size_t)lit1 >= n0)) illegal("unknown string code");
  if (src) {
    for (int64_t i = 0; i < n; ++i)
      if (src[i] < -1 || src[i] >= (int64_t)n0) illegal("unknown string code");
  } else if (n > 0 && (c0 < 0 || c0 > (int64_t)n0 || n > (int64_t)n0 - c0)) {
    illegal("unknown string code");
  }
  if (fn == CAPF_STR_FN_REPLACE && s->dict.empty(lit0)) illegal("empty search literal");
  const double src_bytes = s->profiling ? s->dict.bytes_of(src, c0, n, (int64_t)n0) : 0;
  if (n == 0) return;
  // substring's arguments brought within ±2^41 (no string has that many units)
  // without changing the range they select, so the kernels' sums cannot overflow
  FnArgs a{fn, iarg0, iarg1, lit0, lit1};
  if (fn == CAPF_STR_FN_SUBSTRING) {
    const int64_t B = (int64_t)1 << 41;
    if (a.from < -B) {  // the end moves with the start
      const uint64_t delta = (uint64_t)(-B) - (uint64_t)a.from;
      a.len = (uint64_t)a.len > delta ? (int64_t)((uint64_t)a.len - delta) : 0;
      a.from = -B;
    }
    a.from = std::min(a.from, B);
    a.len = std::min(a.len, 2 * B);
  }
  const int64_t long_len = string_long_threshold();
  const int64_t *off = (const int64_t *)h.off->p;
  const uint8_t *bytes = (const uint8_t *)h.bytes->p;
  const int waves_per_block = SF_BLOCK / WAVE;
  const dim3 grid(grid_for(n, SF_BLOCK)), block(SF_BLOCK);

  BufPtr d_src;
  if (src) {
    d_src = s->alloc(8 * (size_t)n);
    HIP_CHECK(hipMemcpyAsync(d_src->p, src, 8 * (size_t)n, hipMemcpyHostToDevice, s->stream));
    s->sync();  // (pageable source)
  }
  const int64_t *dsrc = d_src ? (const int64_t *)d_src->p : nullptr;
  BufPtr st = s->alloc((size_t)n), len = s->alloc(8 * (size_t)(n + 1)), roff = s->alloc(8 * (size_t)(n + 1)),
         start = s->alloc(8 * (size_t)n), work = s->alloc(8 * (size_t)n), cnt = s->alloc(8);
  HIP_CHECK(hipMemsetAsync(cnt->p, 0, 8, s->stream));
  HIP_CHECK(hipMemsetAsync((int64_t *)len->p + n, 0, 8, s->stream));
  {  // profiled bytes: the sources' bytes, one offset per source, status + length + start out
    KernelTimer kt(s, "str_fn_len", src_bytes + 25.0 * (double)n);
    hipLaunchKernelGGL(k_fn_len, grid, block, 0, s->stream, off, bytes, dsrc, c0, n, a, long_len, (uint8_t *)st->p,
                       (int64_t *)len->p, (int64_t *)start->p, (int64_t *)work->p, (unsigned long long *)cnt->p);
    KERNEL_CHECK();
  }
  if (!concat && fn != CAPF_STR_FN_REPLACE) {
    const int64_t nwork = read_counter(s, cnt);
    if (nwork > 0) {
      KernelTimer kt(s, "str_fn_long_len", 25.0 * (double)nwork);
      hipLaunchKernelGGL(k_fn_long_len, dim3(grid_for(nwork, waves_per_block)), block, 0, s->stream, off, bytes, dsrc,
                         c0, a, (const int64_t *)work->p, nwork, (uint8_t *)st->p, (int64_t *)len->p,
                         (int64_t *)start->p);
      KERNEL_CHECK();
      HIP_CHECK(hipMemsetAsync(cnt->p, 0, 8, s->stream));
    }
  }
  const int64_t total = exclusive_scan_i64(s, (const int64_t *)len->p, (int64_t *)roff->p, n + 1);
  // the scratch result heap, padded like the string heap (words covering a string are read)
  BufPtr rbytes = s->alloc((size_t)total + 16);
  {
    KernelTimer kt(s, "str_fn_write", 2.0 * (double)total + 17.0 * (double)n);
    hipLaunchKernelGGL(k_fn_write, grid, block, 0, s->stream, off, bytes, dsrc, c0, n, a, long_len,
                       (const uint8_t *)st->p, (const int64_t *)roff->p, (const int64_t *)start->p,
                       (uint8_t *)rbytes->p, (int64_t *)work->p, (unsigned long long *)cnt->p);
    KERNEL_CHECK();
  }
  if (fn != CAPF_STR_FN_REPLACE) {
    const int64_t nwork = read_counter(s, cnt);
    if (nwork > 0) {
      KernelTimer kt(s, "str_fn_long", 24.0 * (double)nwork);
      hipLaunchKernelGGL(k_fn_long, dim3(grid_for(nwork, waves_per_block)), block, 0, s->stream, off, bytes, dsrc, c0,
                         a, (const int64_t *)work->p, nwork, (const int64_t *)roff->p, (const int64_t *)start->p,
                         (uint8_t *)rbytes->p);
      KERNEL_CHECK();
    }
  }

  intern_results(s, h, n0, dsrc, c0, n, st, roff, rbytes, total, out);
}

// ------------------------------------------------------------ split
// split(subject, delimiter) per ROW of a table (capf_table_str_split): the
// subject's bytes between the leftmost non-overlapping occurrences of a plain
// (non-empty, literal) delimiter, as a LIST<STRING> column.
//   count pass  per row: NULL or not, pieces = matches + 1, piece bytes =
//               subject bytes − matches · delimiter bytes;
//   two scans   the list offsets and each row's byte base in a scratch heap;
//   write pass  the row's pieces back to back from its base (its subject with
//               the delimiters removed) and one start offset per piece;
//   interning   of the pieces (intern_results): the codes are the child column.
// Thread tier: one thread walks the row with match_at.  Wave tier (a subject of
// at least L bytes, on a worklist filled by the count pass and used by both
// passes): lanes test one start position each over a 64-byte window, a ballot
// gives the candidates, and the leftmost non-overlapping ones are picked from
// the mask in wave-uniform code — the next free position carried across
// windows, since a delimiter such as "aa" overlaps itself and a match may end
// in the next window.
// Profiled bytes, S = the bytes of the subjects of non-NULL rows, T = the piece
// bytes, P = the pieces, n = the rows, w = the worklist's rows:
//   str_split_count       S + 41 n   (two codes, one offset in; count, bytes, validity out)
//   str_split_long_count  41 w
//   str_split_write       S + T + 8 P + 40 n   (codes, offset, list offset, byte base in)
//   str_split_long_write  40 w
struct SplitArgs {
  ColView s, d;  // subject and delimiter (STRING codes)
  int64_t n0;    // dictionary strings of the heap snapshot
};
constexpr uint32_t SPLIT_ERR_EMPTY = 1;

// Row r's subject bytes[q, q + slen) and delimiter; false: a NULL row.
__device__ inline bool split_row(const SplitArgs &g, const int64_t *off, int64_t r, int64_t &q, int64_t &slen,
                                 PatRef &p) {
  if ((g.s.valid && !g.s.valid[r]) || (g.d.valid && !g.d.valid[r])) return false;
  const int64_t cs = ld_int(g.s, r), cd = ld_int(g.d, r);
  if (cs < 0 || cs >= g.n0 || cd < 0 || cd >= g.n0) return false;
  q = off[cs];
  slen = off[cs + 1] - q;
  p = PatRef{nullptr, off[cd], off[cd + 1] - off[cd]};
  return true;
}

__global__ __launch_bounds__(SF_BLOCK) void k_split_count(const int64_t *off, const uint8_t *bytes, SplitArgs g,
                                                           int64_t n, int64_t long_len, int64_t *cnt, int64_t *blen,
                                                           uint8_t *valid, uint32_t *err, int64_t *work,
                                                           unsigned long long *nwork) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    int64_t q = 0, slen = 0, pieces = 0, nb = 0;
    PatRef p{nullptr, 0, 0};
    const bool ok = split_row(g, off, r, q, slen, p);
    if (ok && p.len == 0) {
      atomicOr(err, SPLIT_ERR_EMPTY);
    } else if (ok && slen >= long_len) {
      work[atomicAdd(nwork, 1ull)] = r;  // (counted by k_split_long_count)
    } else if (ok) {
      int64_t hits = 0;
      for (int64_t k = 0; k + p.len <= slen;) {
        if (match_at(bytes, q + k, p)) {
          ++hits;
          k += p.len;
        } else {
          ++k;
        }
      }
      pieces = hits + 1;
      nb = slen - hits * p.len;
    }
    cnt[r] = pieces;
    blen[r] = nb;
    if (valid) valid[r] = ok ? 1 : 0;
  }
}

// One wave over a subject: the matches picked window by window.  WRITE: the
// pieces go to rbytes from w on, piece e + j's start to poff[e + j].
template <bool WRITE>
__device__ inline int64_t split_wave(const uint8_t *bytes, int64_t q, int64_t slen, const PatRef &p, int lane,
                                     uint8_t *rbytes, int64_t w, int64_t *poff, int64_t e) {
  int64_t hits = 0, next_free = 0, ps = 0;  // ps: where the open piece starts
  if (WRITE && lane == 0) poff[e] = w;
  for (int64_t base = 0; base + p.len <= slen; base += WAVE) {
    const int64_t pos = base + lane;
    uint64_t m = __ballot(pos + p.len <= slen && match_at(bytes, q + pos, p));
    if (next_free > base) m = next_free - base >= WAVE ? 0 : m & ~((1ull << (next_free - base)) - 1ull);
    while (m) {  // (wave-uniform)
      const int64_t at = base + (__ffsll((unsigned long long)m) - 1);
      ++hits;
      if (WRITE) {
        copy_wave(rbytes, w, bytes, q + ps, at - ps, 0, lane);
        w += at - ps;
        ps = at + p.len;
        if (lane == 0) poff[e + hits] = w;
      }
      next_free = at + p.len;
      m = next_free - base >= WAVE ? 0 : m & ~((1ull << (next_free - base)) - 1ull);
    }
  }
  if (WRITE) copy_wave(rbytes, w, bytes, q + ps, slen - ps, 0, lane);
  return hits;
}

__global__ __launch_bounds__(SF_BLOCK) void k_split_long_count(const int64_t *off, const uint8_t *bytes, SplitArgs g,
                                                                const int64_t *work, int64_t nwork, int64_t *cnt,
                                                                int64_t *blen) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int64_t nwaves = (int64_t)gridDim.x * blockDim.x / WAVE;
  for (int64_t wi = wave; wi < nwork; wi += nwaves) {
    const int64_t r = work[wi];
    int64_t q = 0, slen = 0;
    PatRef p{nullptr, 0, 0};
    split_row(g, off, r, q, slen, p);
    const int64_t hits = split_wave<false>(bytes, q, slen, p, lane, nullptr, 0, nullptr, 0);
    if (lane == 0) {
      cnt[r] = hits + 1;
      blen[r] = slen - hits * p.len;
    }
  }
}

// loff: the list offsets [n + 1]; rbase: the rows' byte bases in rbytes; poff: the pieces' start offsets
__global__ __launch_bounds__(SF_BLOCK) void k_split_write(const int64_t *off, const uint8_t *bytes, SplitArgs g,
                                                           int64_t n, int64_t long_len, const int64_t *loff,
                                                           const int64_t *rbase, uint8_t *rbytes, int64_t *poff) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    int64_t e = loff[r], q = 0, slen = 0;
    if (loff[r + 1] == e) continue;  // a NULL row
    PatRef p{nullptr, 0, 0};
    split_row(g, off, r, q, slen, p);
    if (slen >= long_len) continue;  // k_split_long_write's
    int64_t w = rbase[r], ps = 0;
    poff[e] = w;
    for (int64_t k = 0; k + p.len <= slen;) {
      if (match_at(bytes, q + k, p)) {
        copy_thread(rbytes, w, bytes, q + ps, k - ps, 0);
        w += k - ps;
        k += p.len;
        ps = k;
        poff[++e] = w;
      } else {
        ++k;
      }
    }
    copy_thread(rbytes, w, bytes, q + ps, slen - ps, 0);
  }
}

__global__ __launch_bounds__(SF_BLOCK) void k_split_long_write(const int64_t *off, const uint8_t *bytes, SplitArgs g,
                                                                const int64_t *work, int64_t nwork,
                                                                const int64_t *loff, const int64_t *rbase,
                                                                uint8_t *rbytes, int64_t *poff) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int64_t nwaves = (int64_t)gridDim.x * blockDim.x / WAVE;
  for (int64_t wi = wave; wi < nwork; wi += nwaves) {
    const int64_t r = work[wi];
    int64_t q = 0, slen = 0;
    PatRef p{nullptr, 0, 0};
    split_row(g, off, r, q, slen, p);
    split_wave<true>(bytes, q, slen, p, lane, rbytes, rbase[r], poff, loff[r]);
  }
}

// S of the header: the subjects' bytes over the rows neither operand makes NULL (profiling only)
static double split_source_bytes(Session *s, const SplitArgs &g, int64_t n) {
  auto host_view = [&](const ColView &v, std::vector<uint8_t> &data, std::vector<uint8_t> &valid) {
    const size_t w = v.enc == ENC_FOR32 ? 4 : v.enc == ENC_FOR24 ? 3 : 8;
    data.resize(w * (size_t)n);
    HIP_CHECK(hipMemcpyAsync(data.data(), v.data, data.size(), hipMemcpyDeviceToHost, s->stream));
    if (v.valid) {
      valid.resize((size_t)n);
      HIP_CHECK(hipMemcpyAsync(valid.data(), v.valid, (size_t)n, hipMemcpyDeviceToHost, s->stream));
    }
    s->sync();
    ColView hv = v;
    hv.data = data.data();
    hv.valid = v.valid ? valid.data() : nullptr;
    return hv;
  };
  std::vector<uint8_t> b0, b1, b2, b3;
  const ColView hs = host_view(g.s, b0, b1), hd = host_view(g.d, b2, b3);
  std::vector<int64_t> codes;
  for (int64_t r = 0; r < n; ++r)
    if (!(hs.valid && !hs.valid[r]) && !(hd.valid && !hd.valid[r])) codes.push_back(ld_int(hs, r));
  return s->dict.bytes_of(codes.data(), 0, (int64_t)codes.size(), g.n0);
}

ColPtr str_split_column(Session *s, const Data &d, int subject_col, int delim_col) {
  const int64_t n = d.nrows;
  const ColPtr &sc = d.cols[(size_t)subject_col], &dc = d.cols[(size_t)delim_col];
  auto o = std::make_shared<Column>();
  o->type = Type::List;
  o->n = n;
  o->data = s->alloc(8 * (size_t)(n + 1));
  HIP_CHECK(hipMemsetAsync(o->data->p, 0, 8 * (size_t)(n + 1), s->stream));
  o->child = make_column(s, Type::String, 0, false);
  if (n == 0) return o;
  SplitArgs g{view_of(sc), view_of(dc), 0};
  std::lock_guard<std::mutex> index_lock(s->dict.index_mu);
  const StringHeap h = s->dict.heap();  // the snapshot the whole step works against
  const size_t n0 = h.n;
  g.n0 = (int64_t)n0;
  const double src_bytes = s->profiling ? split_source_bytes(s, g, n) : 0;
  const int64_t long_len = string_long_threshold();
  const int64_t *off = (const int64_t *)h.off->p;
  const uint8_t *bytes = (const uint8_t *)h.bytes->p;
  const int waves_per_block = SF_BLOCK / WAVE;
  const dim3 grid(grid_for(n, SF_BLOCK)), block(SF_BLOCK);
  int64_t *loff = (int64_t *)o->data->p;

  BufPtr cnt = s->alloc(8 * (size_t)(n + 1)), blen = s->alloc(8 * (size_t)(n + 1)),
         rbase = s->alloc(8 * (size_t)(n + 1)), work = s->alloc(8 * (size_t)n), ctr = s->alloc(16);
  BufPtr valid = g.s.valid || g.d.valid ? s->alloc((size_t)n) : nullptr;
  HIP_CHECK(hipMemsetAsync(ctr->p, 0, 16, s->stream));  // [0] the worklist's length, [1] the error flags
  HIP_CHECK(hipMemsetAsync((int64_t *)cnt->p + n, 0, 8, s->stream));
  HIP_CHECK(hipMemsetAsync((int64_t *)blen->p + n, 0, 8, s->stream));
  {
    KernelTimer kt(s, "str_split_count", src_bytes + 41.0 * (double)n);
    hipLaunchKernelGGL(k_split_count, grid, block, 0, s->stream, off, bytes, g, n, long_len, (int64_t *)cnt->p,
                       (int64_t *)blen->p, valid ? (uint8_t *)valid->p : nullptr, (uint32_t *)((int64_t *)ctr->p + 1),
                       (int64_t *)work->p, (unsigned long long *)ctr->p);
    KERNEL_CHECK();
  }
  HIP_CHECK(hipMemcpyAsync(s->h_scalars, ctr->p, 16, hipMemcpyDeviceToHost, s->stream));
  s->sync();
  const int64_t nwork = s->h_scalars[0];
  if (s->h_scalars[1] & SPLIT_ERR_EMPTY) illegal("split() with an empty delimiter");
  if (nwork > 0) {
    KernelTimer kt(s, "str_split_long_count", 41.0 * (double)nwork);
    hipLaunchKernelGGL(k_split_long_count, dim3(grid_for(nwork, waves_per_block)), block, 0, s->stream, off, bytes, g,
                       (const int64_t *)work->p, nwork, (int64_t *)cnt->p, (int64_t *)blen->p);
    KERNEL_CHECK();
  }
  const int64_t npieces = exclusive_scan_i64(s, (const int64_t *)cnt->p, loff, n + 1);
  const int64_t total = exclusive_scan_i64(s, (const int64_t *)blen->p, (int64_t *)rbase->p, n + 1);
  o->valid = valid;
  if (npieces == 0) return o;  // NULL rows only
  // the scratch result heap, padded like the string heap (words covering a string are read)
  BufPtr rbytes = s->alloc((size_t)total + 16), poff = s->alloc(8 * (size_t)(npieces + 1));
  {
    KernelTimer kt(s, "str_split_write",
                   src_bytes + (double)total + 8.0 * (double)npieces + 40.0 * (double)n);
    hipLaunchKernelGGL(k_split_write, grid, block, 0, s->stream, off, bytes, g, n, long_len, (const int64_t *)loff,
                       (const int64_t *)rbase->p, (uint8_t *)rbytes->p, (int64_t *)poff->p);
    KERNEL_CHECK();
  }
  if (nwork > 0) {
    KernelTimer kt(s, "str_split_long_write", 40.0 * (double)nwork);
    hipLaunchKernelGGL(k_split_long_write, dim3(grid_for(nwork, waves_per_block)), block, 0, s->stream, off, bytes, g,
                       (const int64_t *)work->p, nwork, (const int64_t *)loff, (const int64_t *)rbase->p,
                       (uint8_t *)rbytes->p, (int64_t *)poff->p);
    KERNEL_CHECK();
  }
  HIP_CHECK(hipMemcpyAsync((int64_t *)poff->p + npieces, (const int64_t *)rbase->p + n, 8, hipMemcpyDeviceToDevice,
                           s->stream));
  // every piece has bytes (ST_BYTES = 0): none is NULL, an identity or the host's
  BufPtr st = s->alloc((size_t)npieces);
  HIP_CHECK(hipMemsetAsync(st->p, ST_BYTES, (size_t)npieces, s->stream));
  auto child = std::make_shared<Column>();
  child->type = Type::String;
  child->n = npieces;
  child->data = intern_results(s, h, n0, nullptr, 0, npieces, st, poff, rbytes, total, nullptr);
  o->child = child;
  return o;
}

}  // namespace capf
