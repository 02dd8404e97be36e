// str_match.h — byte matching over the device string heap (CAPF_OP_STR_MATCH):
// shared by the interpreter's per-row path (kernels_basic.hip) and the
// per-dictionary-string kernels (strings.hip).
//
// Strings start at any byte, so nothing here loads a string's bytes one by
// one or through an unaligned pointer: a string is read as the aligned 4-byte
// words that cover it, shifted into place.  The heap's buffer is 16-byte
// aligned and padded past its last string (string_dict.h StringHeap), so the
// covering words — and CONTAINS's one word of look-ahead — are always inside
// it; bytes past a string's end are masked off before they are compared.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace capf {

// The 4 bytes at heap position pos (little-endian).
__device__ inline uint32_t heap_u32(const uint8_t *bytes, int64_t pos) {
  const uint32_t *w = (const uint32_t *)(bytes + (pos & ~(int64_t)3));
  const unsigned sh = ((unsigned)pos & 3u) * 8u;
  const uint32_t lo = w[0];
  return sh ? (lo >> sh) | (w[1] << (32u - sh)) : lo;
}

// A pattern of len bytes: staged as words in LDS (lds != null), else read from
// the heap at off.
struct PatRef {
  const uint32_t *lds;
  int64_t off, len;
};

constexpr int PAT_LDS_BYTES = 256;  // the pattern staging area

// The block's pattern (dictionary code pcode): staged into s_pat (PAT_LDS_BYTES
// / 4 words) when it fits.  Every thread of the block calls this.
__device__ inline PatRef stage_pattern(const int64_t *off, const uint8_t *bytes, int64_t pcode, uint32_t *s_pat) {
  const int64_t poff = off[pcode], plen = off[pcode + 1] - poff;
  const bool staged = plen <= PAT_LDS_BYTES;
  if (staged)
    for (int i = threadIdx.x; 4 * (int64_t)i < plen; i += blockDim.x) s_pat[i] = heap_u32(bytes, poff + 4 * (int64_t)i);
  __syncthreads();
  return PatRef{staged ? s_pat : nullptr, poff, plen};
}

// Pattern bytes [i, i + 4), i a multiple of 4.
__device__ inline uint32_t pat_u32(const uint8_t *bytes, const PatRef &p, int64_t i) {
  return p.lds ? p.lds[i >> 2] : heap_u32(bytes, p.off + i);
}

// Mask of the low min(rem, 4) bytes (rem ≥ 1).
__device__ inline uint32_t low_bytes(int64_t rem) {
  return rem >= 4 ? 0xFFFFFFFFu : (1u << (8u * (unsigned)rem)) - 1u;
}

// bytes[q + i0, q + len) equal the pattern from its byte i0 (a multiple of 4) on.
__device__ inline bool match_at(const uint8_t *bytes, int64_t q, const PatRef &p, int64_t i0 = 0) {
  for (int64_t i = i0; i < p.len; i += 4)
    if ((heap_u32(bytes, q + i) ^ pat_u32(bytes, p, i)) & low_bytes(p.len - i)) return false;
  return true;
}

// The pattern (1 ≤ len ≤ slen) occurs in bytes[q, q + slen): one thread walks
// the start positions over a 64-bit window refilled a word at a time, and
// compares the pattern's first word before anything else.
__device__ inline bool contains_scan(const uint8_t *bytes, int64_t q, int64_t slen, const PatRef &p) {
  const uint32_t first = pat_u32(bytes, p, 0), m0 = low_bytes(p.len);
  const int64_t last = slen - p.len;
  const uint32_t *w = (const uint32_t *)(bytes + (q & ~(int64_t)3));
  const unsigned sh = (unsigned)q & 3u;
  uint64_t win = ((uint64_t)w[0] | (uint64_t)w[1] << 32) >> (8u * sh);
  int avail = 8 - (int)sh;  // bytes of the subject (or past it) in the window
  int64_t wi = 2;
  for (int64_t k = 0; k <= last; ++k) {
    if (avail < 4) {
      win |= (uint64_t)w[wi++] << (8 * avail);
      avail += 4;
    }
    if ((((uint32_t)win ^ first) & m0) == 0 && match_at(bytes, q + k, p, 4)) return true;
    win >>= 8;
    --avail;
  }
  return false;
}

// subject bytes[q, q + slen) <kind> pattern; kind 0 STARTS WITH, 1 ENDS WITH,
// 2 CONTAINS.  The empty pattern matches every subject.
__device__ inline bool str_match(int kind, const uint8_t *bytes, int64_t q, int64_t slen, const PatRef &p) {
  if (slen < p.len) return false;
  if (p.len == 0) return true;
  if (kind == 0) return match_at(bytes, q, p);
  if (kind == 1) return match_at(bytes, q + slen - p.len, p);
  return contains_scan(bytes, q, slen, p);
}

}  // namespace capf
