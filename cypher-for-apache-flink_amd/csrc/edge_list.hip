// edge_list.hip — CSV edge-list ingest straight into HBM.
//
// EdgeListDataSource.graph (flink-cypher/.../api/io/edgelist/EdgeListDataSource.scala:61-81)
// reads a CSV through Flink's CsvTableSource with two LONG fields
// (sourceStartNodeKey, sourceEndNodeKey), a field delimiter and a comment
// prefix (:62-68), then gives every row a unique LONG id with
// `safeAddIdColumn` = DataSet.zipWithUniqueId (flink-cypher/.../impl/TableOps.scala:217-238).
// Here the raw bytes are copied to the device once and parsed there:
//
//   K1 k_el_count  per 16 KiB chunk (1024 threads × 16 B): '\n' count
//   (scan)         chunk → first line index (int64 exclusive scan)
//   K2 k_el_parse  per chunk: the chunk staged in LDS, its newline offsets
//                  found by a block scan, then one thread per line ending in
//                  the chunk parses (start, end) into the line's slot
//   compaction     only when comment lines were skipped
//
// Row semantics follow Flink 1.7's CsvInputFormat / LongParser: a trailing
// '\r' is stripped (line delimiter '\n'); a line starting with the comment
// prefix is skipped; each LONG field is an optional '-' and decimal digits
// up to the (possibly multi-byte) field delimiter; an empty field, any other
// byte (whitespace included), an orphan sign, an int64 overflow or a line
// with fewer than two fields fails the whole read (Flink raises a
// ParseException in the job); text after the second field is not read
// (only two fields are declared).  Rel ids are the data-line ordinals
// 0..M-1: one valid zipWithUniqueId assignment (Flink's ids are unique but
// depend on the task parallelism, so only uniqueness is specified).
#include <fcntl.h>
#include <locale.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cstdio>
#include <system_error>
#include <thread>
#include <vector>

#include "capf_internal.h"
#include "civil_date.h"
#include "device_common.h"

namespace capf {

constexpr int EL_BLOCK = 1024;
constexpr int EL_CHUNK = 16 * EL_BLOCK;  // bytes per workgroup
constexpr int EL_MAX_DELIM = 8;          // field delimiter / comment prefix bytes

enum : uint32_t {
  EL_OK = 0, EL_TOO_SHORT = 1, EL_EMPTY = 2, EL_ILLEGAL_CHAR = 3, EL_OVERFLOW = 4, EL_ORPHAN_SIGN = 5,
  // the typed parser (k_csv_typed)
  EL_BAD_BOOL = 6, EL_BAD_DATE = 7, EL_BAD_DATETIME = 8, EL_BAD_FLOAT = 9, EL_BAD_UTF8 = 10, EL_NUL_BYTE = 11,
  EL_LONE_CR = 12, EL_HIGH_BYTE = 13
};

struct ElSpec {
  uint8_t sep[EL_MAX_DELIM];
  uint8_t comment[EL_MAX_DELIM];
  int sep_len, comment_len;
};

// 16-bit mask of the '\n' bytes of a 16-B piece (bit i = byte i).
__device__ inline uint32_t el_newlines(uint4 q) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t x = w[k] ^ 0x0A0A0A0Au;
    // exact zero-byte detector (no borrow between bytes): 0x80 per zero byte
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
#pragma unroll
    for (int b = 0; b < 4; ++b) m |= ((z >> (8 * b + 7)) & 1u) << (4 * k + b);
  }
  return m;
}

__global__ __launch_bounds__(EL_BLOCK) void k_el_count(const uint4 *text, int64_t *chunk_nl) {
  __shared__ int64_t lds[17];
  const uint4 q = text[(int64_t)blockIdx.x * EL_BLOCK + threadIdx.x];
  const int64_t c = __popc(el_newlines(q));
  const int64_t tot = block_reduce_sum(c, lds);
  if (threadIdx.x == 0) chunk_nl[blockIdx.x] = tot;
}

// Byte at absolute position p.  ElLds: lines inside the staged chunk (the
// common case — the accessor indexes the __shared__ stage directly, so the
// loads are ds_read_u8, not flat loads); ElAny: the first line of a chunk,
// which may start in an earlier chunk (HBM below c0).
struct ElLds {
  const uint8_t *lds;
  int64_t c0;
  __device__ uint8_t operator[](int64_t p) const { return lds[p - c0]; }
};
struct ElAny {
  const uint8_t *g;
  const uint8_t *lds;
  int64_t c0;
  __device__ uint8_t operator[](int64_t p) const { return p >= c0 ? lds[p - c0] : g[p]; }
};

template <int SEP1, class B>
__device__ inline bool el_delim_at(const B &b, int64_t p, int64_t end, const ElSpec &sp) {
  if (SEP1) return p < end && b[p] == sp.sep[0];
  if (p + sp.sep_len > end) return false;
  for (int i = 0; i < sp.sep_len; ++i)
    if (b[p + i] != sp.sep[i]) return false;
  return true;
}

// LongParser.parseField: [p, end) up to the delimiter → value; *p advances
// to the delimiter (or end).  Returns an EL_* code.
template <int SEP1, class B>
__device__ inline uint32_t el_parse_long(const B &b, int64_t &p, int64_t end, const ElSpec &sp,
                                         int64_t &out) {
  if (p >= end || el_delim_at<SEP1>(b, p, end, sp)) return EL_EMPTY;
  bool neg = false;
  if (b[p] == '-') {
    neg = true;
    ++p;
    if (p >= end || el_delim_at<SEP1>(b, p, end, sp)) return EL_ORPHAN_SIGN;
  }
  const uint64_t limit = neg ? 9223372036854775808ull : 9223372036854775807ull;
  uint64_t mag = 0;
  for (; p < end; ++p) {
    const uint8_t ch = b[p];
    if (SEP1 ? ch == sp.sep[0] : el_delim_at<SEP1>(b, p, end, sp)) break;
    const uint32_t d = (uint32_t)ch - '0';
    if (d > 9) return EL_ILLEGAL_CHAR;
    if (mag > (limit - d) / 10) return EL_OVERFLOW;
    mag = mag * 10 + d;
  }
  out = neg ? (int64_t)(0ull - mag) : (int64_t)mag;
  return EL_OK;
}

// One line [start, end): comment test, two LONG fields.
template <int SEP1, class B>
__device__ inline uint32_t el_line(const B &by, int64_t start, int64_t end, const ElSpec &sp,
                                   bool &comment, int64_t &s, int64_t &d) {
  if (end > start && by[end - 1] == '\r') --end;
  comment = sp.comment_len > 0 && end - start >= sp.comment_len;
  for (int i = 0; comment && i < sp.comment_len; ++i) comment = by[start + i] == sp.comment[i];
  s = d = 0;
  if (comment) return EL_OK;
  int64_t p = start;
  uint32_t code = el_parse_long<SEP1>(by, p, end, sp, s);
  if (code != EL_OK) return code;
  if (p >= end) return EL_TOO_SHORT;  // no delimiter before the end of the line
  p += sp.sep_len;
  return p >= end ? EL_TOO_SHORT : el_parse_long<SEP1>(by, p, end, sp, d);
}

template <int SEP1>
__global__ __launch_bounds__(EL_BLOCK) void k_el_parse(const uint4 *text, int64_t n,
                                                       const int64_t *chunk_off, int64_t nchunks,
                                                       int64_t nlines, ElSpec sp, int64_t *src,
                                                       int64_t *dst, uint8_t *keep,
                                                       unsigned long long *err,
                                                       unsigned long long *kept) {
  __shared__ uint4 stage[EL_BLOCK];
  __shared__ uint16_t nlp[EL_CHUNK];
  __shared__ uint32_t lds_scan[17];
  __shared__ unsigned long long lds_kept[17];
  const int64_t b = blockIdx.x, c0 = b * EL_CHUNK;
  const uint4 q = text[b * EL_BLOCK + threadIdx.x];
  stage[threadIdx.x] = q;
  uint32_t m = el_newlines(q), cnt;
  uint32_t idx = block_exclusive_scan((uint32_t)__popc(m), lds_scan, cnt);
  while (m) {
    const int i = __ffs(m) - 1;
    m &= m - 1;
    nlp[idx++] = (uint16_t)(16 * threadIdx.x + i);
  }
  __syncthreads();
  const ElLds fast{(const uint8_t *)stage, c0};
  const int64_t l0 = chunk_off[b];
  // lines ending in this chunk: k < cnt end at a '\n'; the last chunk also
  // owns the unterminated last line (its slot is nlines − 1)
  const bool tail = b == nchunks - 1 && l0 + cnt < nlines;
  const uint32_t items = cnt + (tail ? 1u : 0u);
  unsigned long long mine = 0;
  for (uint32_t k = threadIdx.x; k < items; k += EL_BLOCK) {
    const int64_t gl = l0 + k;
    const int64_t end = k < cnt ? c0 + nlp[k] : n;
    bool comment;
    int64_t s, d;
    uint32_t code;
    if (k > 0) {
      code = el_line<SEP1>(fast, c0 + nlp[k - 1] + 1, end, sp, comment, s, d);
    } else {  // walk back to the previous '\n' (in an earlier chunk)
      const ElAny any{(const uint8_t *)text, (const uint8_t *)stage, c0};
      int64_t start = c0;
      while (start > 0 && any[start - 1] != '\n') --start;
      code = el_line<SEP1>(any, start, end, sp, comment, s, d);
    }
    if (code != EL_OK) atomicMin(err, ((unsigned long long)gl << 8) | code);
    mine += comment ? 0 : 1;
    src[gl] = s;
    dst[gl] = d;
    keep[gl] = comment ? 0 : 1;
  }
  const unsigned long long tot = block_reduce_sum(mine, lds_kept);
  if (threadIdx.x == 0 && tot) atomicAdd(kept, tot);
}

// ------------------------------------------------ K LONG fields per line
// The node / relationship tables of an FS graph source whose declared fields
// are all LONG (FSGraphSource.readFromCsv, FSGraphSource.scala:80-84: a
// CsvTableSource with the canonical field list — id, source, target and
// INTEGER properties, CAPFGraphExport.scala canonical*FieldReference) parse
// with the same row rules, one output column per declared field.
constexpr int CSV_MAXK = 16;
struct CsvOut {
  int64_t *col[CSV_MAXK];
  int k;
};

template <int SEP1, class B>
__device__ inline uint32_t csv_line(const B &by, int64_t start, int64_t end, const ElSpec &sp,
                                    bool &comment, const CsvOut &o, int64_t gl) {
  if (end > start && by[end - 1] == '\r') --end;
  comment = sp.comment_len > 0 && end - start >= sp.comment_len;
  for (int i = 0; comment && i < sp.comment_len; ++i) comment = by[start + i] == sp.comment[i];
  if (comment) {
    for (int f = 0; f < o.k; ++f) o.col[f][gl] = 0;
    return EL_OK;
  }
  int64_t p = start;
  for (int f = 0; f < o.k; ++f) {
    if (f > 0) {
      if (p >= end) return EL_TOO_SHORT;  // no delimiter before the end of the line
      p += sp.sep_len;
      if (p >= end) return EL_TOO_SHORT;
    }
    int64_t v = 0;
    const uint32_t code = el_parse_long<SEP1>(by, p, end, sp, v);
    if (code != EL_OK) return code;
    o.col[f][gl] = v;
  }
  return EL_OK;
}

template <int SEP1>
__global__ __launch_bounds__(EL_BLOCK) void k_csv_parse(const uint4 *text, int64_t n,
                                                        const int64_t *chunk_off, int64_t nchunks,
                                                        int64_t nlines, ElSpec sp, CsvOut o,
                                                        uint8_t *keep, unsigned long long *err,
                                                        unsigned long long *kept) {
  __shared__ uint4 stage[EL_BLOCK];
  __shared__ uint16_t nlp[EL_CHUNK];
  __shared__ uint32_t lds_scan[17];
  __shared__ unsigned long long lds_kept[17];
  const int64_t b = blockIdx.x, c0 = b * EL_CHUNK;
  const uint4 q = text[b * EL_BLOCK + threadIdx.x];
  stage[threadIdx.x] = q;
  uint32_t m = el_newlines(q), cnt;
  uint32_t idx = block_exclusive_scan((uint32_t)__popc(m), lds_scan, cnt);
  while (m) {
    const int i = __ffs(m) - 1;
    m &= m - 1;
    nlp[idx++] = (uint16_t)(16 * threadIdx.x + i);
  }
  __syncthreads();
  const ElLds fast{(const uint8_t *)stage, c0};
  const int64_t l0 = chunk_off[b];
  const bool tail = b == nchunks - 1 && l0 + cnt < nlines;
  const uint32_t items = cnt + (tail ? 1u : 0u);
  unsigned long long mine = 0;
  for (uint32_t k = threadIdx.x; k < items; k += EL_BLOCK) {
    const int64_t gl = l0 + k;
    const int64_t end = k < cnt ? c0 + nlp[k] : n;
    bool comment;
    uint32_t code;
    if (k > 0) {
      code = csv_line<SEP1>(fast, c0 + nlp[k - 1] + 1, end, sp, comment, o, gl);
    } else {
      const ElAny any{(const uint8_t *)text, (const uint8_t *)stage, c0};
      int64_t start = c0;
      while (start > 0 && any[start - 1] != '\n') --start;
      code = csv_line<SEP1>(any, start, end, sp, comment, o, gl);
    }
    if (code != EL_OK) atomicMin(err, ((unsigned long long)gl << 8) | code);
    mine += comment ? 0 : 1;
    keep[gl] = comment ? 0 : 1;
  }
  const unsigned long long tot = block_reduce_sum(mine, lds_kept);
  if (threadIdx.x == 0 && tot) atomicAdd(kept, tot);
}

// ------------------------------------------------ K typed fields per line
// The tables of an FS graph source with STRING / FLOAT / BOOLEAN / DATE /
// LOCALDATETIME or nullable fields (capf_csv_parse_typed; DESIGN.md "Typed CSV
// ingest").  Same pipeline as above — k_el_count, the scan, one pass per chunk
// staged in LDS, one thread per line ending — with a field grammar per declared
// type.  An empty field is NULL for every type (valid byte 0, and the column's
// bit in *nullmask); a column without NULL drops its mask on the host.
//   INT64          el_parse_long
//   BOOL           true | false, ASCII case-insensitive → uint8
//   DATE           YYYY-MM-DD, years 0001-9999 → days since 1970-01-01
//   LOCALDATETIME  YYYY-MM-DDTHH:MM:SS[.f{1,6}] → microseconds since the epoch
//   FLOAT64        [+-]?(\d+(\.\d*)?|\.\d+)([eE][+-]?\d+)?; converted here only on
//                  the exact path (mantissa ≤ 2^53, |power of ten| ≤ 22: one
//                  int → double conversion and one IEEE multiply or divide by
//                  an exact power of ten); any other field of the grammar goes
//                  on the slow list and is converted on the host
//   STRING         strict UTF-8 (no overlong form, surrogate or code point above
//                  U+10FFFF), no 0x00: (position, length, status) per field,
//                  item = string column ordinal · nlines + line, interned after
//                  the kernel (intern_results)
// A '\r' other than the one stripped before the line end, or a byte ≥ 0x80
// outside a STRING field — the ignored text after the last declared field
// included — rejects the line: the host reader (text mode, universal newlines,
// UTF-8) would split the line or count characters differently there.
struct SlowFloat {  // a FLOAT field left to the host: bytes [start, start + len) of the file
  int64_t row, start;
  int32_t len, col;
};
struct TypedOut {
  void *col[CSV_MAXK];       // int64 / double / uint8 rows (STRING: the codes arrive after the interning)
  uint8_t *valid[CSV_MAXK];  // 1 = present
  int32_t type[CSV_MAXK];
  int32_t sidx[CSV_MAXK];    // ordinal among the STRING columns
  int k;
  int64_t nlines;
  int64_t *spos, *slen;      // per STRING item
  uint8_t *sst;              // ST_BYTES | ST_NULL
  SlowFloat *slow;
  unsigned long long *nslow;
  uint32_t *nullmask;        // bit f: column f holds a NULL
};

template <class B>
__device__ inline bool typed_digits(const B &by, int64_t p, int n, int32_t &v) {
  v = 0;
  for (int i = 0; i < n; ++i) {
    const uint32_t d = (uint32_t)by[p + i] - '0';
    if (d > 9) return false;
    v = v * 10 + (int32_t)d;
  }
  return true;
}

// YYYY-MM-DD at [p, p + 10) → day number
template <class B>
__device__ inline bool typed_date(const B &by, int64_t p, int32_t &days) {
  int32_t y, m, d;
  if (!typed_digits(by, p, 4, y) || by[p + 4] != '-' || !typed_digits(by, p + 5, 2, m) || by[p + 7] != '-' ||
      !typed_digits(by, p + 8, 2, d))
    return false;
  if (y < 1 || m < 1 || m > 12 || d < 1) return false;
  const int32_t len = m == 2 ? (leap_year(y) ? 29 : 28) : 30 + ((m + (m >> 3)) & 1);
  if (d > len) return false;
  days = days_from_civil(y, m, d);
  return true;
}

// YYYY-MM-DDTHH:MM:SS[.f{1,6}] at [p, e)
template <class B>
__device__ inline bool typed_datetime(const B &by, int64_t p, int64_t e, int64_t &micros) {
  const int64_t len = e - p;
  if (len != 19 && (len < 21 || len > 26)) return false;
  int32_t days, hh, mm, ss, frac = 0;
  if (!typed_date(by, p, days) || by[p + 10] != 'T' || !typed_digits(by, p + 11, 2, hh) || by[p + 13] != ':' ||
      !typed_digits(by, p + 14, 2, mm) || by[p + 16] != ':' || !typed_digits(by, p + 17, 2, ss))
    return false;
  if (hh > 23 || mm > 59 || ss > 59) return false;
  if (len > 19) {
    const int nd = (int)(len - 20);
    if (by[p + 19] != '.' || !typed_digits(by, p + 20, nd, frac)) return false;
    for (int i = nd; i < 6; ++i) frac *= 10;
  }
  micros = (int64_t)days * MICROS_PER_DAY + (int64_t)((hh * 60 + mm) * 60 + ss) * 1000000 + frac;
  return true;
}

// [p, e) non-empty.  slow: inside the grammar, outside the exact path (out unset).
template <class B>
__device__ inline bool typed_float(const B &by, int64_t p, int64_t e, double &out, bool &slow) {
  static constexpr double P10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                     1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  bool neg = false;
  if (by[p] == '+' || by[p] == '-') neg = by[p++] == '-';
  uint64_t w = 0;
  bool big = false;
  int64_t nd = 0, nfrac = 0;
  for (; p < e; ++p, ++nd) {
    const uint32_t d = (uint32_t)by[p] - '0';
    if (d > 9) break;
    if (!big) {
      w = w * 10 + d;
      big = w > (1ull << 53);
    }
  }
  if (p < e && by[p] == '.') {
    for (++p; p < e; ++p, ++nd, ++nfrac) {
      const uint32_t d = (uint32_t)by[p] - '0';
      if (d > 9) break;
      if (!big) {
        w = w * 10 + d;
        big = w > (1ull << 53);
      }
    }
  }
  if (nd == 0) return false;
  int64_t ex = 0;
  if (p < e && (by[p] | 0x20) == 'e') {
    ++p;
    bool eneg = false;
    if (p < e && (by[p] == '+' || by[p] == '-')) eneg = by[p++] == '-';
    int ne = 0;
    for (; p < e; ++p, ne = 1) {
      const uint32_t d = (uint32_t)by[p] - '0';
      if (d > 9) break;
      if (ex < 100000) ex = ex * 10 + d;  // saturates far outside the exact path
    }
    if (ne == 0) return false;
    if (eneg) ex = -ex;
  }
  if (p != e) return false;
  const int64_t e10 = ex - nfrac;
  slow = big || e10 > 22 || e10 < -22;
  if (!slow) {
    const double v = e10 >= 0 ? (double)w * P10[e10] : (double)w / P10[-e10];
    out = neg ? -v : v;  // the sign last: -0.0 stays -0.0
  }
  return true;
}

template <class B>
__device__ inline uint32_t typed_utf8(const B &by, int64_t p, int64_t e) {
  while (p < e) {
    const uint32_t c = by[p++];
    if (c < 0x80) {
      if (c == 0) return EL_NUL_BYTE;
      if (c == '\r') return EL_LONE_CR;
      continue;
    }
    uint32_t lo = 0x80, hi = 0xBF;  // the range of the first continuation byte
    int more;
    if (c >= 0xC2 && c <= 0xDF) {
      more = 1;
    } else if (c >= 0xE0 && c <= 0xEF) {
      more = 2;
      if (c == 0xE0) lo = 0xA0;  // overlong
      if (c == 0xED) hi = 0x9F;  // surrogates
    } else if (c >= 0xF0 && c <= 0xF4) {
      more = 3;
      if (c == 0xF0) lo = 0x90;  // overlong
      if (c == 0xF4) hi = 0x8F;  // above U+10FFFF
    } else {
      return EL_BAD_UTF8;
    }
    for (int i = 0; i < more; ++i) {
      if (p >= e) return EL_BAD_UTF8;
      const uint32_t d = by[p++];
      if (d < lo || d > hi) return EL_BAD_UTF8;
      lo = 0x80;
      hi = 0xBF;
    }
  }
  return EL_OK;
}

// One line [start, end) into row gl.  nulls: bit f set where field f is empty.
template <int SEP1, class B>
__device__ inline uint32_t typed_line(const B &by, int64_t start, int64_t end, const ElSpec &sp,
                                      const TypedOut &o, int64_t gl, uint32_t &nulls) {
  if (end > start && by[end - 1] == '\r') --end;
  int64_t p = start;
  for (int f = 0; f < o.k; ++f) {
    if (f > 0) {
      if (p >= end) return EL_TOO_SHORT;  // no delimiter before the end of the line
      p += sp.sep_len;
    }
    int64_t fe = p;
    while (fe < end && !(SEP1 ? by[fe] == sp.sep[0] : el_delim_at<SEP1>(by, fe, end, sp))) ++fe;
    const int32_t t = o.type[f];
    const bool null = fe == p;
    if (null) nulls |= 1u << f;
    o.valid[f][gl] = null ? 0 : 1;
    if (t == CAPF_TYPE_STRING) {
      const int64_t item = (int64_t)o.sidx[f] * o.nlines + gl;
      if (!null) {
        const uint32_t code = typed_utf8(by, p, fe);
        if (code != EL_OK) return code;
      }
      o.spos[item] = p;
      o.slen[item] = fe - p;
      o.sst[item] = null ? ST_NULL : ST_BYTES;
    } else if (t == CAPF_TYPE_FLOAT64) {
      double v = 0;
      bool slow = false;
      if (!null && !typed_float(by, p, fe, v, slow)) return EL_BAD_FLOAT;
      if (slow) {
        const unsigned long long at = atomicAdd(o.nslow, 1ull);
        o.slow[at] = SlowFloat{gl, p, (int32_t)(fe - p), f};
      }
      ((double *)o.col[f])[gl] = v;
    } else if (t == CAPF_TYPE_BOOL) {
      uint8_t v = 0;
      if (!null) {
        const int64_t len = fe - p;
        const char *word = len == 4 ? "true" : "false";
        if (len != 4 && len != 5) return EL_BAD_BOOL;
        for (int i = 0; i < (int)len; ++i)
          if ((by[p + i] | 0x20) != (uint8_t)word[i]) return EL_BAD_BOOL;
        v = len == 4;
      }
      ((uint8_t *)o.col[f])[gl] = v;
    } else {
      int64_t v = 0;
      if (!null) {
        if (t == CAPF_TYPE_INT64) {
          int64_t q = p;
          const uint32_t code = el_parse_long<SEP1>(by, q, fe, sp, v);
          if (code != EL_OK) return code;
        } else if (t == CAPF_TYPE_DATE) {
          int32_t days;
          if (fe - p != 10 || !typed_date(by, p, days)) return EL_BAD_DATE;
          v = days;
        } else {
          if (!typed_datetime(by, p, fe, v)) return EL_BAD_DATETIME;
        }
      }
      ((int64_t *)o.col[f])[gl] = v;
    }
    p = fe;
  }
  for (; p < end; ++p) {  // the text that is not parsed
    const uint8_t c = by[p];
    if (c == '\r') return EL_LONE_CR;
    if (c >= 0x80) return EL_HIGH_BYTE;
  }
  return EL_OK;
}

template <int SEP1>
__global__ __launch_bounds__(EL_BLOCK) void k_csv_typed(const uint4 *text, int64_t n, const int64_t *chunk_off,
                                                        int64_t nchunks, int64_t nlines, ElSpec sp, TypedOut o,
                                                        unsigned long long *err) {
  __shared__ uint4 stage[EL_BLOCK];
  __shared__ uint16_t nlp[EL_CHUNK];
  __shared__ uint32_t lds_scan[17];
  __shared__ uint32_t lds_nulls;
  const int64_t b = blockIdx.x, c0 = b * EL_CHUNK;
  const uint4 q = text[b * EL_BLOCK + threadIdx.x];
  stage[threadIdx.x] = q;
  if (threadIdx.x == 0) lds_nulls = 0;
  uint32_t m = el_newlines(q), cnt;
  uint32_t idx = block_exclusive_scan((uint32_t)__popc(m), lds_scan, cnt);
  while (m) {
    const int i = __ffs(m) - 1;
    m &= m - 1;
    nlp[idx++] = (uint16_t)(16 * threadIdx.x + i);
  }
  __syncthreads();
  const ElLds fast{(const uint8_t *)stage, c0};
  const int64_t l0 = chunk_off[b];
  const bool tail = b == nchunks - 1 && l0 + cnt < nlines;
  const uint32_t items = cnt + (tail ? 1u : 0u);
  uint32_t nulls = 0;
  for (uint32_t k = threadIdx.x; k < items; k += EL_BLOCK) {
    const int64_t gl = l0 + k;
    const int64_t end = k < cnt ? c0 + nlp[k] : n;
    uint32_t code;
    if (k > 0) {
      code = typed_line<SEP1>(fast, c0 + nlp[k - 1] + 1, end, sp, o, gl, nulls);
    } else {  // walk back to the previous '\n' (in an earlier chunk)
      const ElAny any{(const uint8_t *)text, (const uint8_t *)stage, c0};
      int64_t start = c0;
      while (start > 0 && any[start - 1] != '\n') --start;
      code = typed_line<SEP1>(any, start, end, sp, o, gl, nulls);
    }
    if (code != EL_OK) atomicMin(err, ((unsigned long long)gl << 8) | code);
  }
  if (nulls) atomicOr(&lds_nulls, nulls);
  __syncthreads();
  if (threadIdx.x == 0 && lds_nulls) atomicOr(o.nullmask, lds_nulls);
}

// The bytes of the STRING items into the scratch heap the interning reads.
__global__ __launch_bounds__(256) void k_typed_strings(const uint8_t *text, const int64_t *spos,
                                                       const int64_t *roff, int64_t n, uint8_t *rbytes) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t d = roff[i], len = roff[i + 1] - d, p = spos[i];
    for (int64_t j = 0; j < len; ++j) rbytes[d + j] = text[p + j];
  }
}

// A STRING column from its items' codes (−1 = NULL: code 0 under a cleared valid byte, as an upload has it).
__global__ __launch_bounds__(256) void k_typed_codes(const int64_t *codes, int64_t n, int64_t *out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = codes[i] < 0 ? 0 : codes[i];
}

// The host's conversions of the slow FLOAT fields into their rows.
__global__ __launch_bounds__(256) void k_typed_patch(const SlowFloat *slow, const double *vals, int64_t n,
                                                     TypedOut o) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    ((double *)o.col[slow[i].col])[slow[i].row] = vals[i];
}

static const char *el_reason(uint32_t code) {
  switch (code) {
    case EL_TOO_SHORT: return "Row too short (fewer fields than declared)";
    case EL_EMPTY: return "empty LONG field";
    case EL_ILLEGAL_CHAR: return "illegal character in a LONG field";
    case EL_OVERFLOW: return "LONG value out of range";
    case EL_ORPHAN_SIGN: return "orphan sign in a LONG field";
    case EL_BAD_BOOL: return "a BOOLEAN field is neither true nor false";
    case EL_BAD_DATE: return "a DATE field is not a valid YYYY-MM-DD";
    case EL_BAD_DATETIME: return "a LOCALDATETIME field is not a valid YYYY-MM-DDTHH:MM:SS[.ffffff]";
    case EL_BAD_FLOAT: return "a FLOAT field is not a decimal number";
    case EL_BAD_UTF8: return "a STRING field is not well-formed UTF-8";
    case EL_NUL_BYTE: return "0x00 byte in a STRING field";
    case EL_LONE_CR: return "'\\r' not followed by the line end";
    case EL_HIGH_BYTE: return "byte >= 0x80 outside a STRING field";
    default: return "unknown parse error";
  }
}

// Parses `nbytes` host bytes into (id, source, target) INT64 columns.
// Parses the device copy `text` (nbytes, zero-padded to whole chunks) into
// (id, source, target) INT64 columns.  last = the file's last byte.
static DataPtr edge_list_parse_device(Session *s, const BufPtr &text, int64_t nbytes, char last,
                                      const ElSpec &sp) {
  auto d = std::make_shared<Data>();
  for (int i = 0; i < 3; ++i) d->cols.push_back(make_column(s, Type::Int64, 0, false));
  if (nbytes == 0) return d;
  const int64_t nchunks = (nbytes + EL_CHUNK - 1) / EL_CHUNK;
  BufPtr cnt = s->alloc(8 * nchunks), off = s->alloc(8 * nchunks);
  {
    KernelTimer kt(s, "el_count", (double)nchunks * EL_CHUNK);
    hipLaunchKernelGGL(k_el_count, dim3((unsigned)nchunks), dim3(EL_BLOCK), 0, s->stream,
                       (const uint4 *)text->p, (int64_t *)cnt->p);
    KERNEL_CHECK();
  }
  const int64_t nl = exclusive_scan_i64(s, (const int64_t *)cnt->p, (int64_t *)off->p, nchunks);
  const int64_t nlines = nl + (last != '\n' ? 1 : 0);
  ColPtr src = make_column(s, Type::Int64, nlines, false);
  ColPtr dst = make_column(s, Type::Int64, nlines, false);
  BufPtr keep = s->alloc(std::max<int64_t>(nlines, 1));
  BufPtr flags = s->alloc(16);
  unsigned long long *d_err = (unsigned long long *)flags->p, *d_kept = d_err + 1;
  const unsigned long long init[2] = {~0ull, 0ull};
  HIP_CHECK(hipMemcpyAsync(d_err, init, 16, hipMemcpyHostToDevice, s->stream));
  if (nlines > 0) {
    KernelTimer kt(s, "el_parse", (double)nchunks * EL_CHUNK + 17.0 * nlines);
    hipLaunchKernelGGL(sp.sep_len == 1 ? k_el_parse<1> : k_el_parse<0>, dim3((unsigned)nchunks),
                       dim3(EL_BLOCK), 0, s->stream,
                       (const uint4 *)text->p, nbytes, (const int64_t *)off->p, nchunks, nlines, sp,
                       (int64_t *)src->data->p, (int64_t *)dst->data->p, (uint8_t *)keep->p, d_err,
                       d_kept);
    KERNEL_CHECK();
  }
  unsigned long long h[2];
  HIP_CHECK(hipMemcpyAsync(h, d_err, 16, hipMemcpyDeviceToHost, s->stream));
  s->sync();
  if (h[0] != ~0ull) {
    const int64_t line = (int64_t)(h[0] >> 8);
    char msg[160];
    snprintf(msg, sizeof msg, "edge list line %lld could not be parsed: %s",
             (long long)line + 1, el_reason((uint32_t)(h[0] & 0xFF)));
    illegal(msg);
  }
  const int64_t m = (int64_t)h[1];
  if (m != nlines) {  // comment lines: compact the data lines
    int64_t got = 0;
    BufPtr idx = compact_flags(s, (const uint8_t *)keep->p, nlines, &got);
    if (got != m) fail(CAPF_ERR_INTERNAL, "edge list: kept-line count mismatch");
    src = gather_column(s, src, (const int64_t *)idx->p, m);
    dst = gather_column(s, dst, (const int64_t *)idx->p, m);
  }
  auto id = std::make_shared<Column>();
  id->type = Type::Int64;
  id->n = m;
  if (m > 0) id->data = iota_index(s, 0, m);
  d->nrows = m;
  d->cols = {id, src, dst};
  s->sync();
  return d;
}

// Parses the device copy `text` into K INT64 columns (one per declared field).
static DataPtr csv_longs_parse_device(Session *s, const BufPtr &text, int64_t nbytes, char last,
                                      const ElSpec &sp, int k) {
  auto d = std::make_shared<Data>();
  for (int i = 0; i < k; ++i) d->cols.push_back(make_column(s, Type::Int64, 0, false));
  if (nbytes == 0) return d;
  const int64_t nchunks = (nbytes + EL_CHUNK - 1) / EL_CHUNK;
  BufPtr cnt = s->alloc(8 * nchunks), off = s->alloc(8 * nchunks);
  {
    KernelTimer kt(s, "el_count", (double)nchunks * EL_CHUNK);
    hipLaunchKernelGGL(k_el_count, dim3((unsigned)nchunks), dim3(EL_BLOCK), 0, s->stream,
                       (const uint4 *)text->p, (int64_t *)cnt->p);
    KERNEL_CHECK();
  }
  const int64_t nl = exclusive_scan_i64(s, (const int64_t *)cnt->p, (int64_t *)off->p, nchunks);
  const int64_t nlines = nl + (last != '\n' ? 1 : 0);
  std::vector<ColPtr> cols;
  CsvOut o{};
  o.k = k;
  for (int i = 0; i < k; ++i) {
    cols.push_back(make_column(s, Type::Int64, nlines, false));
    o.col[i] = nlines > 0 ? (int64_t *)cols[i]->data->p : nullptr;
  }
  BufPtr keep = s->alloc(std::max<int64_t>(nlines, 1));
  BufPtr flags = s->alloc(16);
  unsigned long long *d_err = (unsigned long long *)flags->p, *d_kept = d_err + 1;
  const unsigned long long init[2] = {~0ull, 0ull};
  HIP_CHECK(hipMemcpyAsync(d_err, init, 16, hipMemcpyHostToDevice, s->stream));
  if (nlines > 0) {
    KernelTimer kt(s, "csv_parse", (double)nchunks * EL_CHUNK + 8.0 * k * nlines);
    hipLaunchKernelGGL(sp.sep_len == 1 ? k_csv_parse<1> : k_csv_parse<0>, dim3((unsigned)nchunks),
                       dim3(EL_BLOCK), 0, s->stream, (const uint4 *)text->p, nbytes, (const int64_t *)off->p,
                       nchunks, nlines, sp, o, (uint8_t *)keep->p, d_err, d_kept);
    KERNEL_CHECK();
  }
  unsigned long long h[2];
  HIP_CHECK(hipMemcpyAsync(h, d_err, 16, hipMemcpyDeviceToHost, s->stream));
  s->sync();
  if (h[0] != ~0ull) {
    char msg[160];
    snprintf(msg, sizeof msg, "CSV line %lld could not be parsed: %s", (long long)(h[0] >> 8) + 1,
             el_reason((uint32_t)(h[0] & 0xFF)));
    illegal(msg);
  }
  const int64_t m = (int64_t)h[1];
  if (m != nlines) {  // comment lines
    int64_t got = 0;
    BufPtr idx = compact_flags(s, (const uint8_t *)keep->p, nlines, &got);
    if (got != m) fail(CAPF_ERR_INTERNAL, "csv: kept-line count mismatch");
    for (auto &c : cols) c = gather_column(s, c, (const int64_t *)idx->p, m);
  }
  d->nrows = m;
  d->cols = cols;
  s->sync();
  return d;
}

static BufPtr el_text_buffer(Session *s, int64_t nbytes) {
  const int64_t nchunks = (nbytes + EL_CHUNK - 1) / EL_CHUNK;
  BufPtr text = s->alloc(std::max<int64_t>(nchunks, 1) * EL_CHUNK);
  if (nchunks * EL_CHUNK > nbytes)  // zero padding: never a '\n'
    HIP_CHECK(hipMemsetAsync((char *)text->p + nbytes, 0, nchunks * EL_CHUNK - nbytes, s->stream));
  return text;
}

static DataPtr edge_list_parse(Session *s, const char *bytes, int64_t nbytes, const ElSpec &sp) {
  BufPtr text = el_text_buffer(s, nbytes);
  if (nbytes > 0)
    HIP_CHECK(hipMemcpyAsync(text->p, bytes, nbytes, hipMemcpyHostToDevice, s->stream));
  return edge_list_parse_device(s, text, nbytes, nbytes > 0 ? bytes[nbytes - 1] : '\n', sp);
}

// File → HBM: 64 MiB pieces read by parallel pread()s into two pinned staging
// buffers, each DMA'd while the next piece is read (no whole-file pinning).
constexpr int64_t EL_PIECE = 64ll << 20;
constexpr int EL_READERS = 8;

// File → device text buffer (zero-padded to whole chunks); *len_out / *last_out
// = the file's size and last byte.
static BufPtr read_text_file(Session *s, const char *path, int64_t *len_out, char *last_out) {
  const int fd = open(path, O_RDONLY);
  if (fd < 0) illegal(std::string("cannot open ") + path);
  struct stat st;
  if (fstat(fd, &st) != 0) {
    close(fd);
    illegal(std::string("cannot stat ") + path);
  }
  const int64_t len = (int64_t)st.st_size;
  char *stage[2] = {nullptr, nullptr};
  hipEvent_t done[2] = {nullptr, nullptr};
  auto cleanup = [&]() {
    for (int b = 0; b < 2; ++b) {
      if (done[b]) (void)hipEventDestroy(done[b]);
      if (stage[b]) (void)hipHostFree(stage[b]);
    }
    close(fd);
  };
  try {
    BufPtr text = el_text_buffer(s, len);
    const int64_t piece = std::min<int64_t>(EL_PIECE, std::max<int64_t>(len, 1));
    for (int b = 0; b < 2; ++b) {
      HIP_CHECK(hipHostMalloc((void **)&stage[b], (size_t)piece, hipHostMallocDefault));
      HIP_CHECK(hipEventCreateWithFlags(&done[b], hipEventDisableTiming));
    }
    char last = '\n';
    for (int64_t off = 0, i = 0; off < len; off += piece, ++i) {
      const int b = (int)(i & 1);
      const int64_t n = std::min(piece, len - off);
      HIP_CHECK(hipEventSynchronize(done[b]));  // the DMA that last used this buffer
      std::atomic<bool> bad{false};
      std::vector<std::thread> rd;
      const int64_t part = (n + EL_READERS - 1) / EL_READERS;
      auto read_range = [&, b, off](int64_t lo, int64_t hi) {
        for (int64_t p = lo; p < hi;) {
          const ssize_t r = pread(fd, stage[b] + p, (size_t)(hi - p), (off_t)(off + p));
          if (r <= 0) {
            bad = true;
            return;
          }
          p += r;
        }
      };
      try {
        for (int t = 0; t < EL_READERS; ++t) {
          const int64_t lo = t * part, hi = std::min(n, lo + part);
          if (lo >= hi) break;
          rd.emplace_back(read_range, lo, hi);
        }
      } catch (const std::system_error &) {
        // a reader thread could not be started: the ones that were started
        // are joined below; the remaining ranges are read on this thread
        const int64_t done_to = (int64_t)rd.size() * part;
        read_range(done_to, n);
      }
      for (auto &th : rd) th.join();
      if (bad) illegal(std::string("short read of ") + path);
      last = stage[b][n - 1];
      HIP_CHECK(hipMemcpyAsync((char *)text->p + off, stage[b], (size_t)n, hipMemcpyHostToDevice,
                               s->stream));
      HIP_CHECK(hipEventRecord(done[b], s->stream));
    }
    s->sync();
    cleanup();
    *len_out = len;
    *last_out = last;
    return text;
  } catch (...) {
    s->sync();
    cleanup();
    throw;
  }
}

// float(s) of a field of the FLOAT grammar: glibc's strtod is correctly
// rounded, and the "C" locale is passed explicitly (the process's is not read).
static double slow_float(const char *p, int32_t len) {
  static const locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
  const std::string field(p, (size_t)len);
  return strtod_l(field.c_str(), nullptr, c_locale);
}

// Parses the device copy `text` (nbytes, zero-padded to whole chunks) into one
// column per declared type.  host(start, len) = those bytes of the file in host
// memory (asked only for slow FLOAT fields).
template <class HostBytes>
static DataPtr csv_typed_parse_device(Session *s, const BufPtr &text, int64_t nbytes, char last, const ElSpec &sp,
                                      int k, const int32_t *types, HostBytes host) {
  auto d = std::make_shared<Data>();
  s->csv_slow_floats = 0;
  if (nbytes == 0) {
    for (int i = 0; i < k; ++i) d->cols.push_back(make_column(s, (Type)types[i], 0, false));
    return d;
  }
  const int64_t nchunks = (nbytes + EL_CHUNK - 1) / EL_CHUNK;
  BufPtr cnt = s->alloc(8 * nchunks), off = s->alloc(8 * nchunks);
  {
    KernelTimer kt(s, "el_count", (double)nchunks * EL_CHUNK);
    hipLaunchKernelGGL(k_el_count, dim3((unsigned)nchunks), dim3(EL_BLOCK), 0, s->stream,
                       (const uint4 *)text->p, (int64_t *)cnt->p);
    KERNEL_CHECK();
  }
  const int64_t nl = exclusive_scan_i64(s, (const int64_t *)cnt->p, (int64_t *)off->p, nchunks);
  const int64_t nlines = nl + (last != '\n' ? 1 : 0);  // ≥ 1: the file is not empty
  std::vector<ColPtr> cols;
  TypedOut o{};
  o.k = k;
  o.nlines = nlines;
  int nstr = 0, nflt = 0;
  double row_bytes = 0;  // written per line: the value and its valid byte; a STRING's position, length and status
  for (int i = 0; i < k; ++i) {
    const Type t = (Type)types[i];
    cols.push_back(make_column(s, t, nlines, true));
    o.col[i] = cols[i]->data->p;
    o.valid[i] = (uint8_t *)cols[i]->valid->p;
    o.type[i] = types[i];
    o.sidx[i] = t == Type::String ? nstr++ : 0;
    nflt += t == Type::Float64;
    row_bytes += t == Type::String ? 18.0 : (double)type_width(t) + 1.0;
  }
  const int64_t nitems = (int64_t)nstr * nlines;
  BufPtr spos, slen, sst, slow;
  if (nstr) {
    spos = s->alloc(8 * (size_t)nitems);
    slen = s->alloc(8 * (size_t)(nitems + 1));
    sst = s->alloc((size_t)nitems);
    HIP_CHECK(hipMemsetAsync((int64_t *)slen->p + nitems, 0, 8, s->stream));
    o.spos = (int64_t *)spos->p;
    o.slen = (int64_t *)slen->p;
    o.sst = (uint8_t *)sst->p;
  }
  if (nflt) {  // every FLOAT field may be slow
    slow = s->alloc(sizeof(SlowFloat) * (size_t)nflt * (size_t)nlines);
    o.slow = (SlowFloat *)slow->p;
  }
  BufPtr flags = s->alloc(24);  // [0] first error, [1] slow fields, [2] columns holding a NULL
  unsigned long long *d_flags = (unsigned long long *)flags->p;
  const unsigned long long init[3] = {~0ull, 0ull, 0ull};
  HIP_CHECK(hipMemcpyAsync(d_flags, init, 24, hipMemcpyHostToDevice, s->stream));
  o.nslow = d_flags + 1;
  o.nullmask = (uint32_t *)(d_flags + 2);
  {
    KernelTimer kt(s, "csv_typed_parse", (double)nchunks * EL_CHUNK + row_bytes * (double)nlines);
    hipLaunchKernelGGL(sp.sep_len == 1 ? k_csv_typed<1> : k_csv_typed<0>, dim3((unsigned)nchunks),
                       dim3(EL_BLOCK), 0, s->stream, (const uint4 *)text->p, nbytes, (const int64_t *)off->p,
                       nchunks, nlines, sp, o, d_flags);
    KERNEL_CHECK();
  }
  unsigned long long h[3];
  HIP_CHECK(hipMemcpyAsync(h, d_flags, 24, hipMemcpyDeviceToHost, s->stream));
  s->sync();
  if (h[0] != ~0ull) {
    char msg[200];
    snprintf(msg, sizeof msg, "CSV line %lld could not be parsed: %s", (long long)(h[0] >> 8) + 1,
             el_reason((uint32_t)(h[0] & 0xFF)));
    illegal(msg);
  }
  const int64_t nslow = (int64_t)h[1];
  if (nslow > 0) {
    std::vector<SlowFloat> list((size_t)nslow);
    HIP_CHECK(hipMemcpyAsync(list.data(), slow->p, sizeof(SlowFloat) * (size_t)nslow, hipMemcpyDeviceToHost,
                             s->stream));
    s->sync();
    std::vector<double> vals((size_t)nslow);
    for (int64_t i = 0; i < nslow; ++i) vals[(size_t)i] = slow_float(host(list[(size_t)i].start), list[(size_t)i].len);
    BufPtr d_vals = s->alloc(8 * (size_t)nslow);
    HIP_CHECK(hipMemcpyAsync(d_vals->p, vals.data(), 8 * (size_t)nslow, hipMemcpyHostToDevice, s->stream));
    {
      KernelTimer kt(s, "csv_typed_patch", 40.0 * (double)nslow);
      hipLaunchKernelGGL(k_typed_patch, dim3(grid_for(nslow, 256)), dim3(256), 0, s->stream,
                         (const SlowFloat *)slow->p, (const double *)d_vals->p, nslow, o);
      KERNEL_CHECK();
    }
    s->sync();  // (pageable source)
  }
  s->csv_slow_floats = nslow;
  if (nstr) {
    std::lock_guard<std::mutex> index_lock(s->dict.index_mu);
    const StringHeap heap = s->dict.heap();  // the snapshot the interning works against
    BufPtr roff = s->alloc(8 * (size_t)(nitems + 1));
    const int64_t total = exclusive_scan_i64(s, (const int64_t *)slen->p, (int64_t *)roff->p, nitems + 1);
    BufPtr rbytes = s->alloc((size_t)total + 16);  // padded like the string heap
    {
      KernelTimer kt(s, "csv_typed_strings", 2.0 * (double)total + 24.0 * (double)nitems);
      hipLaunchKernelGGL(k_typed_strings, dim3(grid_for(nitems, 256)), dim3(256), 0, s->stream,
                         (const uint8_t *)text->p, (const int64_t *)spos->p, (const int64_t *)roff->p, nitems,
                         (uint8_t *)rbytes->p);
      KERNEL_CHECK();
    }
    BufPtr codes = intern_results(s, heap, heap.n, nullptr, 0, nitems, sst, roff, rbytes, total, nullptr);
    KernelTimer kt(s, "csv_typed_codes", 16.0 * (double)nitems);
    for (int i = 0; i < k; ++i)
      if ((Type)types[i] == Type::String) {
        hipLaunchKernelGGL(k_typed_codes, dim3(grid_for(nlines, 256)), dim3(256), 0, s->stream,
                           (const int64_t *)codes->p + (int64_t)o.sidx[i] * nlines, nlines, (int64_t *)o.col[i]);
        KERNEL_CHECK();
      }
  }
  for (int i = 0; i < k; ++i)
    if (!((uint32_t)h[2] >> i & 1u)) cols[i]->valid = nullptr;  // no NULL: no mask (the no-null fast paths)
  d->nrows = nlines;
  d->cols = cols;
  s->sync();
  return d;
}

static DataPtr edge_list_read_file(Session *s, const char *path, const ElSpec &sp) {
  int64_t len = 0;
  char last = '\n';
  BufPtr text = read_text_file(s, path, &len, &last);
  return edge_list_parse_device(s, text, len, last, sp);  // syncs the stream
}

static ElSpec el_spec(const char *sep, const char *comment) {
  ElSpec sp{};
  if (!sep || !*sep) illegal("edge list: the field delimiter (option `sep`) must be non-empty");
  sp.sep_len = (int)strlen(sep);
  sp.comment_len = comment ? (int)strlen(comment) : 0;
  if (sp.sep_len > EL_MAX_DELIM || sp.comment_len > EL_MAX_DELIM)
    illegal("edge list: delimiter / comment prefix longer than 8 bytes");
  if (strchr(sep, '\n') || (comment && strchr(comment, '\n')))
    illegal("edge list: delimiter / comment prefix must not contain the line delimiter");
  memcpy(sp.sep, sep, sp.sep_len);
  if (sp.comment_len) memcpy(sp.comment, comment, sp.comment_len);
  return sp;
}

static capf_table *edge_list_table(Session *s, DataPtr d, const char *id_col, const char *src_col,
                                   const char *dst_col) {
  auto n = std::make_shared<Node>();
  n->s = s;
  n->kind = Kind::Source;
  n->names = {id_col, src_col, dst_col};
  n->types = {Type::Int64, Type::Int64, Type::Int64};
  n->result = d;
  auto *t = new capf_table;
  t->node = n;
  return t;
}

}  // namespace capf

using namespace capf;

extern "C" capf_status capf_edge_list_parse(capf_session *cs, const char *bytes, int64_t nbytes,
                                            const char *sep, const char *comment,
                                            const char *id_col, const char *src_col,
                                            const char *dst_col, capf_table **out) {
  try {
    if (!cs || !out || !id_col || !src_col || !dst_col || (nbytes > 0 && !bytes))
      illegal("null argument");
    if (nbytes < 0) illegal("negative byte count");
    const ElSpec sp = el_spec(sep, comment);
    Session *s = &cs->impl;
    *out = edge_list_table(s, edge_list_parse(s, bytes, nbytes, sp), id_col, src_col, dst_col);
    return CAPF_OK;
  } catch (const capf::Error &e) {
    return record_error(e.code, e.what());
  } catch (const std::exception &e) {  // bad_alloc, system_error, … never cross the C-ABI
    return record_error(CAPF_ERR_INTERNAL, e.what());
  }
}

extern "C" capf_status capf_edge_list_read(capf_session *cs, const char *path, const char *sep,
                                           const char *comment, const char *id_col,
                                           const char *src_col, const char *dst_col,
                                           capf_table **out) {
  try {
    if (!cs || !out || !path || !id_col || !src_col || !dst_col) illegal("null argument");
    const ElSpec sp = el_spec(sep, comment);
    Session *s = &cs->impl;
    DataPtr d = edge_list_read_file(s, path, sp);
    *out = edge_list_table(s, d, id_col, src_col, dst_col);
    return CAPF_OK;
  } catch (const capf::Error &e) {
    return record_error(e.code, e.what());
  } catch (const std::exception &e) {  // bad_alloc, system_error, … never cross the C-ABI
    return record_error(CAPF_ERR_INTERNAL, e.what());
  }
}

static capf_table *csv_table(Session *s, DataPtr d, int32_t ncols, const char *const *names) {
  auto n = std::make_shared<Node>();
  n->s = s;
  n->kind = Kind::Source;
  for (int i = 0; i < ncols; ++i) {
    n->names.emplace_back(names[i]);
    n->types.push_back(Type::Int64);
  }
  n->result = d;
  auto *t = new capf_table;
  t->node = n;
  return t;
}

static void csv_args(capf_session *cs, int32_t ncols, const char *const *names, capf_table **out) {
  if (!cs || !out || !names) illegal("null argument");
  if (ncols < 1 || ncols > CSV_MAXK) illegal("CSV: 1..16 LONG fields");
  for (int i = 0; i < ncols; ++i)
    if (!names[i]) illegal("null column name");
}

extern "C" capf_status capf_csv_parse_longs(capf_session *cs, const char *bytes, int64_t nbytes,
                                            const char *sep, int32_t ncols, const char *const *names,
                                            capf_table **out) {
  try {
    csv_args(cs, ncols, names, out);
    if (nbytes < 0 || (nbytes > 0 && !bytes)) illegal("bad byte buffer");
    const ElSpec sp = el_spec(sep, nullptr);
    Session *s = &cs->impl;
    BufPtr text = el_text_buffer(s, nbytes);
    if (nbytes > 0) HIP_CHECK(hipMemcpyAsync(text->p, bytes, nbytes, hipMemcpyHostToDevice, s->stream));
    DataPtr d = csv_longs_parse_device(s, text, nbytes, nbytes > 0 ? bytes[nbytes - 1] : '\n', sp, ncols);
    *out = csv_table(s, d, ncols, names);
    return CAPF_OK;
  } catch (const capf::Error &e) {
    return record_error(e.code, e.what());
  } catch (const std::exception &e) {
    return record_error(CAPF_ERR_INTERNAL, e.what());
  }
}

extern "C" capf_status capf_csv_read_longs(capf_session *cs, const char *path, const char *sep,
                                           int32_t ncols, const char *const *names, capf_table **out) {
  try {
    csv_args(cs, ncols, names, out);
    if (!path) illegal("null argument");
    const ElSpec sp = el_spec(sep, nullptr);
    Session *s = &cs->impl;
    int64_t len = 0;
    char last = '\n';
    BufPtr text = read_text_file(s, path, &len, &last);
    DataPtr d = csv_longs_parse_device(s, text, len, last, sp, ncols);
    *out = csv_table(s, d, ncols, names);
    return CAPF_OK;
  } catch (const capf::Error &e) {
    return record_error(e.code, e.what());
  } catch (const std::exception &e) {
    return record_error(CAPF_ERR_INTERNAL, e.what());
  }
}

// ---- typed tables (DESIGN.md "Typed CSV ingest")
static capf_table *csv_typed_table(Session *s, DataPtr d, int32_t ncols, const char *const *names,
                                   const int32_t *types) {
  auto n = std::make_shared<Node>();
  n->s = s;
  n->kind = Kind::Source;
  for (int i = 0; i < ncols; ++i) {
    n->names.emplace_back(names[i]);
    n->types.push_back((Type)types[i]);
  }
  n->result = d;
  auto *t = new capf_table;
  t->node = n;
  return t;
}

static ElSpec csv_typed_args(capf_session *cs, const char *sep, int32_t ncols, const char *const *names,
                             const int32_t *types, capf_table **out) {
  if (!cs || !out || !names || !types) illegal("null argument");
  if (ncols < 1 || ncols > CSV_MAXK) illegal("CSV: 1..16 fields");
  for (int i = 0; i < ncols; ++i) {
    if (!names[i]) illegal("null column name");
    const int32_t t = types[i];
    if (t != CAPF_TYPE_INT64 && t != CAPF_TYPE_FLOAT64 && t != CAPF_TYPE_BOOL && t != CAPF_TYPE_STRING &&
        t != CAPF_TYPE_DATE && t != CAPF_TYPE_LOCALDATETIME)
      illegal("CSV: a field is INT64, FLOAT64, BOOL, STRING, DATE or LOCALDATETIME");
  }
  const ElSpec sp = el_spec(sep, nullptr);
  for (int i = 0; i < sp.sep_len; ++i)  // a delimiter byte may not fall inside a UTF-8 sequence or a line end
    if (sp.sep[i] >= 0x80 || sp.sep[i] == '\r') illegal("CSV: the typed parser takes an ASCII delimiter without '\\r'");
  return sp;
}

extern "C" capf_status capf_csv_parse_typed(capf_session *cs, const char *bytes, int64_t nbytes,
                                            const char *sep, int32_t ncols, const char *const *names,
                                            const int32_t *types, capf_table **out) {
  try {
    const ElSpec sp = csv_typed_args(cs, sep, ncols, names, types, out);
    if (nbytes < 0 || (nbytes > 0 && !bytes)) illegal("bad byte buffer");
    Session *s = &cs->impl;
    BufPtr text = el_text_buffer(s, nbytes);
    if (nbytes > 0) HIP_CHECK(hipMemcpyAsync(text->p, bytes, nbytes, hipMemcpyHostToDevice, s->stream));
    DataPtr d = csv_typed_parse_device(s, text, nbytes, nbytes > 0 ? bytes[nbytes - 1] : '\n', sp, ncols, types,
                                       [bytes](int64_t start) { return bytes + start; });
    *out = csv_typed_table(s, d, ncols, names, types);
    return CAPF_OK;
  } catch (const capf::Error &e) {
    return record_error(e.code, e.what());
  } catch (const std::exception &e) {
    return record_error(CAPF_ERR_INTERNAL, e.what());
  }
}

extern "C" capf_status capf_csv_read_typed(capf_session *cs, const char *path, const char *sep,
                                           int32_t ncols, const char *const *names, const int32_t *types,
                                           capf_table **out) {
  try {
    const ElSpec sp = csv_typed_args(cs, sep, ncols, names, types, out);
    if (!path) illegal("null argument");
    Session *s = &cs->impl;
    int64_t len = 0;
    char last = '\n';
    BufPtr text = read_text_file(s, path, &len, &last);
    // the file mapped on the first slow FLOAT field only (its pages are in the cache: it was just read)
    const char *map = nullptr;
    auto host = [&](int64_t start) {
      if (!map) {
        const int fd = open(path, O_RDONLY);
        void *m = fd < 0 ? MAP_FAILED : mmap(nullptr, (size_t)len, PROT_READ, MAP_PRIVATE, fd, 0);
        if (fd >= 0) close(fd);
        if (m == MAP_FAILED) illegal(std::string("cannot map ") + path);
        map = (const char *)m;
      }
      return map + start;
    };
    DataPtr d;
    try {
      d = csv_typed_parse_device(s, text, len, last, sp, ncols, types, host);
    } catch (...) {
      if (map) munmap((void *)map, (size_t)len);
      throw;
    }
    if (map) munmap((void *)map, (size_t)len);
    *out = csv_typed_table(s, d, ncols, names, types);
    return CAPF_OK;
  } catch (const capf::Error &e) {
    return record_error(e.code, e.what());
  } catch (const std::exception &e) {
    return record_error(CAPF_ERR_INTERNAL, e.what());
  }
}

extern "C" capf_status capf_session_csv_slow_floats(capf_session *cs, int64_t *out) {
  try {
    if (!cs || !out) illegal("null argument");
    *out = cs->impl.csv_slow_floats;
    return CAPF_OK;
  } catch (const capf::Error &e) {
    return record_error(e.code, e.what());
  }
}
