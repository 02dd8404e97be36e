// shuffle.hip — hash routing of table rows to ranks: the exchange step of
// the distributed Table layer (dist_table.py, SURVEY §8(e): "each hop's
// frontier rows are shuffled by join key"; GROUP BY / DISTINCT rows by
// h(key)).  Flink does the same inside its DataSet join / groupBy: a hash
// repartition of both inputs before the local hash join / group-reduce
// (FlinkTable.scala:171-187, 123-150 lower onto those operators).
//
//   k_route       dest(row) = owner of h(key values): splitmix64 of each key
//                 (decoded int64 / canonical fp64 bits / bool byte / NULL
//                 sentinel), combined; owner = (h >> 32) · parts >> 32.  Equal
//                 key tuples get equal owners (collisions only co-locate more
//                 rows), all NULLs of a key go to one owner, −0.0 routes like
//                 0.0 and every NaN alike.
//   radix sort    (dest, row) pairs, rocprim, only the ⌈log2 parts⌉ dest bits:
//                 a stable counting sort of the rows by owner
//   k_bounds      first row of every owner in the sorted keys (binary search)
//
// The caller gathers every column by the permutation (gather_column), so the
// rows for rank p are the contiguous slice [off[p], off[p+1]) of each column:
// one all-to-all per column moves them (RCCL, dist_table.py).
// Bytes per row: keys read once, 8 B dest + 8 B row written and sorted.
#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "capf_internal.h"
#include "device_common.h"

namespace capf {

constexpr int ROUTE_MAXK = 8;

struct RouteKeys {
  ColView k[ROUTE_MAXK];
  int nk;
};

__device__ inline uint64_t route_mix(uint64_t x) {  // splitmix64 finaliser
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// 64-bit routing image of row i of key column c (type-specific canonical form).
__device__ inline uint64_t route_bits(const ColView &c, int64_t i) {
  if (c.valid && !c.valid[i]) return 0x6E756C6C6E756C6Cull;  // NULL sentinel
  switch (c.type) {
    case CAPF_TYPE_BOOL:
      return ((const uint8_t *)c.data)[i] ? 1ull : 0ull;
    case CAPF_TYPE_FLOAT64: {
      double v = ((const double *)c.data)[i];
      if (v == 0.0) v = 0.0;                           // −0.0 → 0.0
      if (v != v) return 0x7FF8000000000000ull;        // one NaN
      return (uint64_t)__double_as_longlong(v);
    }
    case CAPF_TYPE_NULL:
      return 0x6E756C6C6E756C6Cull;
    default:  // INT64 / STRING codes, any encoding
      return (uint64_t)ld_int(c, i);
  }
}

__global__ void k_route(RouteKeys rk, int64_t n, uint32_t parts, uint32_t *dest, int64_t *row) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t h = 0x243F6A8885A308D3ull;
    for (int j = 0; j < rk.nk; ++j) h = route_mix(h ^ route_bits(rk.k[j], i)) + 0x9E3779B97F4A7C15ull;
    dest[i] = (uint32_t)(((h >> 32) * (uint64_t)parts) >> 32);
    row[i] = i;
  }
}

// off[p] = first index of the sorted dest array holding a value ≥ p (p ≤ parts).
__global__ void k_bounds(const uint32_t *sorted, int64_t n, int parts, int64_t *off) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > parts) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sorted[mid] < (uint32_t)p) lo = mid + 1;
    else hi = mid;
  }
  off[p] = lo;
}

template <class F>
static void route_rocprim(Session *s, F &&f) {
  size_t tmp = 0;
  HIP_CHECK(f(nullptr, tmp));
  BufPtr t = s->alloc(std::max<size_t>(tmp, 16));
  HIP_CHECK(f(t->p, tmp));
}

// Permutation (int64 row indexes, rows grouped by owner in owner order, stable
// within an owner) and per-owner counts of the rows of `keys` over `parts`.
BufPtr route_permutation(Session *s, const std::vector<ColView> &keys, int64_t n, int parts,
                         std::vector<int64_t> &counts) {
  if (keys.empty() || keys.size() > (size_t)ROUTE_MAXK) illegal("1..8 routing keys");
  if (parts <= 0 || parts > (1 << 20)) illegal("parts out of range");
  counts.assign(parts, 0);
  const int64_t n1 = std::max<int64_t>(n, 1);
  BufPtr perm = s->alloc(8 * n1);
  if (n == 0) return perm;
  RouteKeys rk;
  rk.nk = (int)keys.size();
  for (int j = 0; j < rk.nk; ++j) rk.k[j] = keys[j];
  BufPtr dest = s->alloc(4 * n1), dsort = s->alloc(4 * n1), rows = s->alloc(8 * n1);
  {
    KernelTimer kt(s, "route", (8.0 * rk.nk + 12.0) * n);
    hipLaunchKernelGGL(k_route, dim3(grid_for(n, 256)), dim3(256), 0, s->stream, rk, n, (uint32_t)parts,
                       (uint32_t *)dest->p, (int64_t *)rows->p);
    KERNEL_CHECK();
  }
  int bits = 0;
  while ((1 << bits) < parts) ++bits;
  if (bits == 0) {
    HIP_CHECK(hipMemcpyAsync(perm->p, rows->p, 8 * n, hipMemcpyDeviceToDevice, s->stream));
    counts[0] = n;
    return perm;
  }
  {
    KernelTimer kt(s, "route_sort", 24.0 * n);
    route_rocprim(s, [&](void *t, size_t &sz) {
      return rocprim::radix_sort_pairs(t, sz, (const uint32_t *)dest->p, (uint32_t *)dsort->p,
                                       (const int64_t *)rows->p, (int64_t *)perm->p, (size_t)n, 0, bits,
                                       s->stream);
    });
  }
  BufPtr off = s->alloc(8 * (parts + 1));
  hipLaunchKernelGGL(k_bounds, dim3((parts + 256) / 256), dim3(256), 0, s->stream, (const uint32_t *)dsort->p,
                     n, parts, (int64_t *)off->p);
  KERNEL_CHECK();
  std::vector<int64_t> h(parts + 1);
  HIP_CHECK(hipMemcpyAsync(h.data(), off->p, 8 * (parts + 1), hipMemcpyDeviceToHost, s->stream));
  s->sync();
  for (int p = 0; p < parts; ++p) counts[p] = h[p + 1] - h[p];
  return perm;
}

// ------------------------------------------------------------ row packing
// The exchange's wire format (dist_table.py GpuExchange.send): each row is W
// bytes, row-major — per column `width` bytes of (value − base) little-endian
// (width 3 / 4 for INTEGER / STRING-code columns whose range over ALL ranks
// fits 24 / 32 bits, the FOR24 / FOR32 encodings; 8 otherwise and for floats;
// 1 for BOOL), then one validity byte when the column is nullable on some
// rank.  One all_to_all_single moves the packed rows; the receiver's columns
// keep the narrow encodings (no re-encode).  One thread per row, the row
// assembled in registers and written as whole dwords when W is a multiple of 4.
//
// A LIST column puts a length field into the row — the list's element count,
// 4 bytes (8 when some list on some rank has 2^31 elements or more), 0 for a
// NULL list — then the usual validity byte.  Its elements travel apart, as
// the packed rows of the child column taken as a one-column table (the same
// record: `width` bytes of (value − base), then a validity byte when an
// element is NULL on some rank): see "list elements" below.
struct PackCol {
  ColView v;
  int32_t width, off, voff;  // voff < 0: no validity byte
  int64_t base;
};

__device__ inline uint64_t pack_value(const PackCol &c, int64_t r, bool valid) {
  if (!valid || c.v.type == CAPF_TYPE_NULL) return 0;
  if (c.v.type == CAPF_TYPE_LIST) {  // the length field: v.data = the offsets [n + 1]
    const int64_t *off = (const int64_t *)c.v.data;
    return (uint64_t)(off[r + 1] - off[r]);
  }
  if (c.v.type == CAPF_TYPE_BOOL) return ((const uint8_t *)c.v.data)[r] ? 1u : 0u;
  if (c.v.type == CAPF_TYPE_FLOAT64) return ((const uint64_t *)c.v.data)[r];
  return (uint64_t)(ld_int(c.v, r) - c.base);
}

__global__ void k_pack_rows(const PackCol *cols, int nc, int W, int64_t n, uint8_t *out) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    uint8_t *row = out + r * W;
    for (int j = 0; j < nc; ++j) {
      const PackCol c = cols[j];
      const bool valid = !c.v.valid || c.v.valid[r];
      const uint64_t x = pack_value(c, r, valid);
      for (int b = 0; b < c.width; ++b) row[c.off + b] = (uint8_t)(x >> (8 * b));
      if (c.voff >= 0) row[c.voff] = valid ? 1 : 0;
    }
  }
}

// One column out of packed rows: width 3 → FOR24 buffer, 4 → FOR32 words,
// 8 → int64 / float64 bits, 1 → bool bytes; validity bytes when voff ≥ 0.
__global__ void k_unpack_col(const uint8_t *rows, int64_t n, int W, int off, int width, int voff,
                             uint8_t *data, uint8_t *valid) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const uint8_t *row = rows + r * W;
    for (int b = 0; b < width; ++b) data[r * width + b] = row[off + b];
    if (voff >= 0) valid[r] = row[voff];
  }
}

void pack_rows(Session *s, const std::vector<ColPtr> &cols, const int32_t *width, const int64_t *base,
               const int32_t *nullable, int64_t n, int *W_out, void *d_out) {
  std::vector<PackCol> pc(cols.size());
  int W = 0;
  for (size_t j = 0; j < cols.size(); ++j) {
    if (cols[j]->type == Type::List) {  // (view_of refuses lists: no row kernel reads their values)
      const ColPtr &c = cols[j];
      pc[j].v = ColView{c->data ? c->data->p : nullptr, c->valid ? (const uint8_t *)c->valid->p : nullptr,
                        CAPF_TYPE_LIST, ENC_PLAIN, 0};
    } else {
      pc[j].v = view_of(cols[j]);
    }
    pc[j].width = width[j];
    pc[j].off = W;
    pc[j].base = base[j];
    W += width[j];
    pc[j].voff = nullable[j] ? W++ : -1;
  }
  *W_out = W;
  if (!d_out || n == 0 || W == 0) return;
  BufPtr dc = s->alloc(sizeof(PackCol) * std::max<size_t>(pc.size(), 1));
  HIP_CHECK(hipMemcpyAsync(dc->p, pc.data(), sizeof(PackCol) * pc.size(), hipMemcpyHostToDevice, s->stream));
  {
    KernelTimer kt(s, "pack_rows", (double)W * n);
    hipLaunchKernelGGL(k_pack_rows, dim3(grid_for(n, 256)), dim3(256), 0, s->stream, (const PackCol *)dc->p,
                       (int)pc.size(), W, n, (uint8_t *)d_out);
    KERNEL_CHECK();
  }
  s->sync();  // the host copy of the column table is released on return
}

ColPtr unpack_column(Session *s, const void *rows, int64_t n, int W, int off, int width, int voff, int64_t base,
                     Type t) {
  auto c = std::make_shared<Column>();
  c->type = t;
  c->n = n;
  if (t == Type::Null) return c;
  c->enc = width == 3 ? ENC_FOR24 : width == 4 ? ENC_FOR32 : ENC_PLAIN;
  c->base = width == 3 || width == 4 ? base : 0;
  // FOR24 buffers carry 16 zero bytes past 3·n (4-B / 12-B loads at any row)
  const int64_t bytes = (int64_t)width * n + (width == 3 ? 16 : 0);
  c->data = s->alloc(std::max<int64_t>(bytes, 16));
  if (width == 3) HIP_CHECK(hipMemsetAsync((uint8_t *)c->data->p + 3 * n, 0, 16, s->stream));
  if (voff >= 0) c->valid = s->alloc(std::max<int64_t>(n, 1));
  if (n > 0) {
    hipLaunchKernelGGL(k_unpack_col, dim3(grid_for(n, 256)), dim3(256), 0, s->stream, (const uint8_t *)rows, n,
                       W, off, width, voff, (uint8_t *)c->data->p, voff >= 0 ? (uint8_t *)c->valid->p : nullptr);
    KERNEL_CHECK();
  }
  return c;
}

// ------------------------------------------------------------ list elements
// The element stream of a LIST column: element e of the stream is child row
// first + e (first = offsets[0]: a list column's offsets need not start at 0),
// one record of REC = width + (validity byte ? 1 : 0) bytes each, the records
// of the rows for rank p one contiguous slice (element counts = differences of
// the offsets at the slice bounds).  Lists hold many more elements than the
// table has rows, so both kernels divide the work by element, never by row or
// list, and store whole dwords: a thread takes four consecutive records (their
// 4 · REC bytes are REC dwords at a dword boundary); REC = 8 stores one 8-byte
// value per thread.  Only the last, partial group is stored byte by byte.
struct ElemSrc {
  ColView v;      // the child column (type NULL: every element is NULL)
  int64_t first;  // child row of stream element 0
  int64_t base;
};

// value bits and validity of stream element e
__device__ inline uint64_t elem_value(const ElemSrc &c, int64_t e, bool &valid) {
  const int64_t r = c.first + e;
  valid = c.v.type != CAPF_TYPE_NULL && (!c.v.valid || c.v.valid[r]);
  if (!valid) return 0;
  if (c.v.type == CAPF_TYPE_BOOL) return ((const uint8_t *)c.v.data)[r] ? 1u : 0u;
  if (c.v.type == CAPF_TYPE_FLOAT64) return ((const uint64_t *)c.v.data)[r];
  return (uint64_t)(ld_int(c.v, r) - c.base);
}

// Four records per thread: 4 · REC bytes are REC whole dwords, assembled in
// registers (every shift and index is a compile-time constant once unrolled)
// and stored as dwords.  The last, partial group is stored byte by byte.
template <int WIDTH, bool VALID>
__global__ void k_pack_elems(ElemSrc c, int64_t total, uint8_t *out) {
  constexpr int REC = WIDTH + (VALID ? 1 : 0);
  const int64_t ng = (total + 3) >> 2;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ng; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e0 = g << 2;
    if (e0 + 4 <= total) {
      uint32_t w[REC] = {};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        bool valid;
        const uint64_t x = elem_value(c, e0 + q, valid);
#pragma unroll
        for (int k = 0; k < REC; ++k) {
          const uint32_t byte = k < WIDTH ? (uint32_t)(x >> (8 * k)) & 0xFFu : (valid ? 1u : 0u);
          const int pos = q * REC + k;
          w[pos >> 2] |= byte << (8 * (pos & 3));
        }
      }
      uint32_t *o = (uint32_t *)out + g * REC;
#pragma unroll
      for (int j = 0; j < REC; ++j) o[j] = w[j];
    } else {
      for (int64_t e = e0; e < total; ++e) {
        bool valid;
        const uint64_t x = elem_value(c, e, valid);
        for (int k = 0; k < REC; ++k)
          out[e * REC + k] = k < WIDTH ? (uint8_t)(x >> (8 * k)) : (uint8_t)(valid ? 1 : 0);
      }
    }
  }
}

// 8-byte records without a validity byte: one value per thread
__global__ void k_pack_elems8(ElemSrc c, int64_t total, uint64_t *out) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    bool valid;
    out[e] = elem_value(c, e, valid);
  }
}

// The receiver's side, records with a validity byte → the child's data (WIDTH
// bytes per element, contiguous: the FOR24 / FOR32 / plain buffer itself) and
// validity bytes.  Four records per thread again: REC dwords in, WIDTH dwords
// of data and one dword of validity out.  (Without a validity byte the records
// are the buffer: a device-to-device copy, no kernel.)
template <int WIDTH>
__global__ void k_unpack_elems(const uint8_t *rec, int64_t total, uint8_t *data, uint8_t *valid) {
  constexpr int REC = WIDTH + 1;
  const int64_t ng = (total + 3) >> 2;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ng; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e0 = g << 2;
    if (e0 + 4 <= total) {
      uint32_t r[REC], d[WIDTH] = {}, v = 0;
      const uint32_t *src = (const uint32_t *)rec + g * REC;
#pragma unroll
      for (int j = 0; j < REC; ++j) r[j] = src[j];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int k = 0; k < WIDTH; ++k) {
          const int pos = q * REC + k, dpos = q * WIDTH + k;
          d[dpos >> 2] |= ((r[pos >> 2] >> (8 * (pos & 3))) & 0xFFu) << (8 * (dpos & 3));
        }
        const int vpos = q * REC + WIDTH;
        v |= (((r[vpos >> 2] >> (8 * (vpos & 3))) & 0xFFu) ? 1u : 0u) << (8 * q);
      }
      uint32_t *o = (uint32_t *)data + g * WIDTH;
#pragma unroll
      for (int j = 0; j < WIDTH; ++j) o[j] = d[j];
      ((uint32_t *)valid)[g] = v;
    } else {
      for (int64_t e = e0; e < total; ++e) {
        for (int k = 0; k < WIDTH; ++k) data[e * WIDTH + k] = rec[e * REC + k];
        valid[e] = rec[e * REC + WIDTH] ? 1 : 0;
      }
    }
  }
}

// lengths (and validity) of a LIST column out of packed rows: len[r] = the
// length field, len[n] = 0 (the scan's last entry is then the element total)
// A length above the stream's element count is stored as n_elems + 1: the
// total then differs from n_elems (refused), and equal totals mean offsets
// that ascend within the stream.
__global__ void k_unpack_list_len(const uint8_t *rows, int64_t n, int W, int off, int width, int voff,
                                  int64_t n_elems, int64_t *len, uint8_t *valid) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n; r += (int64_t)gridDim.x * blockDim.x) {
    if (r == n) {
      len[r] = 0;
      continue;
    }
    const uint8_t *row = rows + r * W;
    uint64_t x = 0;
    for (int b = 0; b < width; ++b) x |= (uint64_t)row[off + b] << (8 * b);
    const bool v = voff < 0 || row[voff];
    len[r] = !v ? 0 : x > (uint64_t)n_elems ? n_elems + 1 : (int64_t)x;
    if (valid) valid[r] = v ? 1 : 0;
  }
}

// out[i] = off[pos[i]] (the offsets at the bounds of the per-destination row slices)
__global__ void k_pick_offsets(const int64_t *off, const int64_t *pos, int np, int64_t *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < np) out[i] = off[pos[i]];
}

__global__ void k_list_max_len(const int64_t *off, const uint8_t *valid, int64_t n, unsigned long long *mx) {
  unsigned long long m = 0;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long l = valid && !valid[r] ? 0ull : (unsigned long long)(off[r + 1] - off[r]);
    m = l > m ? l : m;
  }
  if (m) atomicMax(mx, m);
}

// A NULL list may own a non-empty extent of the offsets (capf_table_add_list
// accepts it, gathers keep it); on the wire a NULL list has length 0, so its
// elements must not enter the stream.  The three kernels below find that state
// and rebuild the column without those elements.
__global__ void k_null_list_extent(const int64_t *off, const uint8_t *valid, int64_t n, int32_t *found) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
    if (!valid[r] && off[r + 1] > off[r]) *found = 1;
}

// len[r] = elements of list r on the wire (0 for a NULL list), len[n] = 0
__global__ void k_wire_lengths(const int64_t *off, const uint8_t *valid, int64_t n, int64_t *len) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n; r += (int64_t)gridDim.x * blockDim.x)
    len[r] = r < n && valid[r] ? off[r + 1] - off[r] : 0;
}

// keep[q] = child row q belongs to a non-NULL list (rows outside [off[0], off[n]) do not)
__global__ void k_in_stream(int64_t lo, int64_t hi, int64_t m, uint8_t *keep) {
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < m; q += (int64_t)gridDim.x * blockDim.x)
    keep[q] = q >= lo && q < hi ? 1 : 0;
}
__global__ void k_drop_null_extents(const int64_t *off, const uint8_t *valid, int64_t n, int64_t m, uint8_t *keep) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    if (valid[r]) continue;
    for (int64_t q = off[r]; q < off[r + 1] && q < m; ++q) keep[q] = 0;  // (a rare state: serial per NULL list)
  }
}

ColPtr list_without_null_extents(Session *s, const ColPtr &c) {
  if (!c->valid || !c->data || c->n == 0) return c;
  const int64_t n = c->n;
  const int64_t *off = (const int64_t *)c->data->p;
  const uint8_t *valid = (const uint8_t *)c->valid->p;
  BufPtr flag = s->alloc(4);
  HIP_CHECK(hipMemsetAsync(flag->p, 0, 4, s->stream));
  hipLaunchKernelGGL(k_null_list_extent, dim3(grid_for(n, 256)), dim3(256), 0, s->stream, off, valid, n,
                     (int32_t *)flag->p);
  KERNEL_CHECK();
  int32_t found = 0;
  HIP_CHECK(hipMemcpyAsync(&found, flag->p, 4, hipMemcpyDeviceToHost, s->stream));
  s->sync();
  if (!found) return c;
  const std::vector<int64_t> o = list_offsets_at(s, c, {0, n});
  const int64_t m = c->child->n;
  if (o[0] < 0 || o[1] < o[0] || o[1] > m) fail(CAPF_ERR_INTERNAL, "list offsets outside the element column");
  auto out = std::make_shared<Column>();
  out->type = Type::List;
  out->n = n;
  out->valid = c->valid;
  out->data = s->alloc(8 * (n + 1));
  BufPtr len = s->alloc(8 * (n + 1));
  hipLaunchKernelGGL(k_wire_lengths, dim3(grid_for(n + 1, 256)), dim3(256), 0, s->stream, off, valid, n,
                     (int64_t *)len->p);
  KERNEL_CHECK();
  const int64_t total = exclusive_scan_i64(s, (const int64_t *)len->p, (int64_t *)out->data->p, n + 1);
  if (c->child->type == Type::Null || total == 0) {
    out->child = c->child->type == Type::Null ? null_column(s, Type::Null, total)
                                              : make_column(s, c->child->type, 0, false);
    return out;
  }
  BufPtr keep = s->alloc(std::max<int64_t>(m, 1));
  hipLaunchKernelGGL(k_in_stream, dim3(grid_for(m, 256)), dim3(256), 0, s->stream, o[0], o[1], m, (uint8_t *)keep->p);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k_drop_null_extents, dim3(grid_for(n, 256)), dim3(256), 0, s->stream, off, valid, n, m,
                     (uint8_t *)keep->p);
  KERNEL_CHECK();
  int64_t kept = 0;
  BufPtr idx = compact_flags(s, (const uint8_t *)keep->p, m, &kept);
  if (kept != total) fail(CAPF_ERR_INTERNAL, "list offsets overlap");
  out->child = gather_column(s, c->child, (const int64_t *)idx->p, kept);
  return out;
}

std::vector<int64_t> list_offsets_at(Session *s, const ColPtr &c, const std::vector<int64_t> &pos) {
  std::vector<int64_t> out(pos.size(), 0);
  if (pos.empty() || !c->data) return out;
  const int np = (int)pos.size();
  BufPtr dp = s->alloc(8 * np), dv = s->alloc(8 * np);
  HIP_CHECK(hipMemcpyAsync(dp->p, pos.data(), 8 * np, hipMemcpyHostToDevice, s->stream));
  hipLaunchKernelGGL(k_pick_offsets, dim3((np + 255) / 256), dim3(256), 0, s->stream, (const int64_t *)c->data->p,
                     (const int64_t *)dp->p, np, (int64_t *)dv->p);
  KERNEL_CHECK();
  HIP_CHECK(hipMemcpyAsync(out.data(), dv->p, 8 * np, hipMemcpyDeviceToHost, s->stream));
  s->sync();
  return out;
}

int64_t list_max_len(Session *s, const ColPtr &c) {
  if (c->n == 0 || !c->data) return 0;
  BufPtr mx = s->alloc(8);
  HIP_CHECK(hipMemsetAsync(mx->p, 0, 8, s->stream));
  hipLaunchKernelGGL(k_list_max_len, dim3(grid_for(c->n, 256)), dim3(256), 0, s->stream, (const int64_t *)c->data->p,
                     c->valid ? (const uint8_t *)c->valid->p : nullptr, c->n, (unsigned long long *)mx->p);
  KERNEL_CHECK();
  int64_t h = 0;
  HIP_CHECK(hipMemcpyAsync(&h, mx->p, 8, hipMemcpyDeviceToHost, s->stream));
  s->sync();
  return h;
}

void pack_list_elems(Session *s, const ColPtr &child, int64_t first, int64_t total, int width, int64_t base,
                     bool with_valid, void *d_out) {
  const int rec = width + (with_valid ? 1 : 0);
  if (total == 0 || rec == 0) return;
  ElemSrc c;
  c.v = child->type == Type::Null ? ColView{nullptr, nullptr, CAPF_TYPE_NULL, ENC_PLAIN, 0} : view_of(child);
  c.first = first;
  c.base = base;
  KernelTimer kt(s, "pack_elems", (double)rec * total);
  const dim3 g(grid_for((total + 3) >> 2, 256)), b(256);
  uint8_t *out = (uint8_t *)d_out;
#define CAPF_PACK_ELEMS(W, V) hipLaunchKernelGGL((k_pack_elems<W, V>), g, b, 0, s->stream, c, total, out)
  switch (rec) {
    case 1: CAPF_PACK_ELEMS(1, false); break;
    case 2: CAPF_PACK_ELEMS(1, true); break;
    case 3: CAPF_PACK_ELEMS(3, false); break;
    case 4:
      if (with_valid) CAPF_PACK_ELEMS(3, true);
      else CAPF_PACK_ELEMS(4, false);
      break;
    case 5: CAPF_PACK_ELEMS(4, true); break;
    case 8:
      hipLaunchKernelGGL(k_pack_elems8, dim3(grid_for(total, 256)), b, 0, s->stream, c, total, (uint64_t *)d_out);
      break;
    case 9: CAPF_PACK_ELEMS(8, true); break;
    default: illegal("packed elements: bad record size");
  }
#undef CAPF_PACK_ELEMS
  KERNEL_CHECK();
}

// The child column of a received LIST column from its `total` records.
static ColPtr unpack_list_elems(Session *s, const void *rec, int64_t total, int width, int64_t base, bool with_valid,
                                Type t) {
  if (t == Type::Null) return null_column(s, Type::Null, total);
  auto c = std::make_shared<Column>();
  c->type = t;
  c->n = total;
  c->enc = width == 3 ? ENC_FOR24 : width == 4 ? ENC_FOR32 : ENC_PLAIN;
  c->base = width == 3 || width == 4 ? base : 0;
  // FOR24 buffers carry 16 zero bytes past 3·n (4-B / 12-B loads at any row)
  const int64_t bytes = (int64_t)width * total + (width == 3 ? 16 : 0);
  c->data = s->alloc(std::max<int64_t>(bytes, 16));
  if (width == 3) HIP_CHECK(hipMemsetAsync((uint8_t *)c->data->p + 3 * total, 0, 16, s->stream));
  if (with_valid) c->valid = s->alloc(std::max<int64_t>(total, 1));
  if (total == 0) return c;
  const int R = width + (with_valid ? 1 : 0);
  KernelTimer kt(s, "unpack_elems", (double)R * total);
  if (!with_valid) {  // the records are the buffer
    HIP_CHECK(hipMemcpyAsync(c->data->p, rec, (size_t)width * total, hipMemcpyDeviceToDevice, s->stream));
    return c;
  }
  const dim3 g(grid_for((total + 3) >> 2, 256)), b(256);
  const uint8_t *r8 = (const uint8_t *)rec;
  uint8_t *d = (uint8_t *)c->data->p, *v = (uint8_t *)c->valid->p;
  switch (width) {
    case 1: hipLaunchKernelGGL(k_unpack_elems<1>, g, b, 0, s->stream, r8, total, d, v); break;
    case 3: hipLaunchKernelGGL(k_unpack_elems<3>, g, b, 0, s->stream, r8, total, d, v); break;
    case 4: hipLaunchKernelGGL(k_unpack_elems<4>, g, b, 0, s->stream, r8, total, d, v); break;
    default: hipLaunchKernelGGL(k_unpack_elems<8>, g, b, 0, s->stream, r8, total, d, v); break;
  }
  KERNEL_CHECK();
  return c;
}

ColPtr unpack_list_column(Session *s, const void *rows, int64_t n, int W, int off, int width, int voff,
                          const void *d_elems, int64_t n_elems, int ewidth, int64_t ebase, bool evalid, Type et) {
  auto c = std::make_shared<Column>();
  c->type = Type::List;
  c->n = n;
  c->data = s->alloc(8 * (n + 1));
  BufPtr len = s->alloc(8 * (n + 1));
  if (voff >= 0) c->valid = s->alloc(std::max<int64_t>(n, 1));
  hipLaunchKernelGGL(k_unpack_list_len, dim3(grid_for(n + 1, 256)), dim3(256), 0, s->stream, (const uint8_t *)rows,
                     n, W, off, width, voff, n_elems, (int64_t *)len->p,
                     voff >= 0 ? (uint8_t *)c->valid->p : nullptr);
  KERNEL_CHECK();
  const int64_t total = exclusive_scan_i64(s, (const int64_t *)len->p, (int64_t *)c->data->p, n + 1);
  if (total != n_elems)
    illegal("packed lists: the rows' lengths sum to " + std::to_string(total) + " elements, the stream holds " +
            std::to_string(n_elems));
  c->child = unpack_list_elems(s, d_elems, total, ewidth, ebase, evalid, et);
  return c;
}

}  // namespace capf
