// lists.hip — LIST columns: collect(e) per group and gathers of list rows.
//
// collect is the list-valued aggregator of the reference's Table SPI group
// (Expr.scala Collect, lowered by FlinkSQLExprMapper.scala:283 to Flink's
// COLLECT, a MULTISET).  A LIST column is CSR-shaped: int64 offsets [n + 1] in
// `data` and the elements in `child` (a plain column; its validity marks
// NULL elements and is absent when none can occur).
//   collect: keep the rows whose argument is non-NULL (compact_flags), drop
//   duplicate (group, value) pairs for DISTINCT (group_rows), stable radix sort
//   by (group, value) — elements ascend within a list —, per-group counts with
//   atomics, one exclusive scan over ng + 1 counters → offsets.
//   gather: new lengths, exclusive scan → offsets, one thread per output list
//   writes its child indexes, then the element column is gathered.
#include <algorithm>

#include "capf_internal.h"
#include "device_common.h"
#include "list_search.h"

namespace capf {

__global__ void k_valid_flags(const uint8_t *valid, int64_t n, uint8_t *flags) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    flags[i] = valid[i] ? 1 : 0;
}

__global__ void k_group_counts(const int64_t *gid, int64_t n, unsigned long long *counts) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    atomicAdd(&counts[gid[i]], 1ull);
}

static ColPtr list_column(Session *s, int64_t n, const BufPtr &offsets, const ColPtr &child) {
  auto o = std::make_shared<Column>();
  o->type = Type::List;
  o->n = n;
  o->data = offsets;
  o->child = child;
  (void)s;
  return o;
}

static ColPtr empty_elements(Session *s, Type elem) {
  return elem == Type::Null ? null_column(s, Type::Null, 0) : make_column(s, elem, 0, false);
}

ColPtr collect_lists(Session *s, const Grouping &g, int64_t nrows, const ColPtr &arg,
                     bool distinct) {
  const int64_t ng = g.ngroups;
  BufPtr offsets = s->alloc(8 * (ng + 1));
  HIP_CHECK(hipMemsetAsync(offsets->p, 0, 8 * (ng + 1), s->stream));
  force(arg);
  if (nrows == 0 || ng == 0 || arg->type == Type::Null)
    return list_column(s, ng, offsets, empty_elements(s, arg->type));
  auto gid = std::make_shared<Column>();
  gid->type = Type::Int64;
  gid->n = nrows;
  gid->data = g.group_of_row;
  // rows with a non-NULL argument
  ColPtr gk = gid, vk = arg;
  int64_t k = nrows;
  if (arg->valid) {
    BufPtr flags = s->alloc(nrows);
    hipLaunchKernelGGL(k_valid_flags, dim3(grid_for(nrows, 256)), dim3(256), 0, s->stream,
                       (const uint8_t *)arg->valid->p, nrows, (uint8_t *)flags->p);
    KERNEL_CHECK();
    BufPtr idx = compact_flags(s, (const uint8_t *)flags->p, nrows, &k);
    gk = gather_column(s, gid, (const int64_t *)idx->p, k);
    vk = gather_column(s, arg, (const int64_t *)idx->p, k);
  }
  if (k == 0) return list_column(s, ng, offsets, empty_elements(s, arg->type));
  if (distinct) {  // one row per distinct (group, value)
    Data pairs;
    pairs.nrows = k;
    pairs.cols = {gk, vk};
    Grouping dg = group_rows(s, pairs, {0, 1});
    const int64_t *reps = (const int64_t *)dg.rep_row->p;
    gk = gather_column(s, gk, reps, dg.ngroups);
    vk = gather_column(s, vk, reps, dg.ngroups);
    k = dg.ngroups;
  }
  BufPtr perm = sort_permutation(s, {gk, vk}, {0, 0}, k);
  ColPtr gs = gather_column(s, gk, (const int64_t *)perm->p, k);
  ColPtr vs = decode_column(s, gather_column(s, vk, (const int64_t *)perm->p, k));
  BufPtr counts = s->alloc(8 * (ng + 1));
  HIP_CHECK(hipMemsetAsync(counts->p, 0, 8 * (ng + 1), s->stream));
  hipLaunchKernelGGL(k_group_counts, dim3(grid_for(k, 256)), dim3(256), 0, s->stream,
                     (const int64_t *)gs->data->p, k, (unsigned long long *)counts->p);
  KERNEL_CHECK();
  // counts[ng] = 0, so the exclusive scan's last entry is the element total
  exclusive_scan_i64(s, (const int64_t *)counts->p, (int64_t *)offsets->p, ng + 1);
  auto child = std::make_shared<Column>();
  child->type = vs->type;
  child->n = k;
  child->data = vs->data;  // collect keeps no NULLs: no element validity
  return list_column(s, ng, offsets, child);
}

__global__ void k_list_lengths(const int64_t *off, const int64_t *idx, int64_t m, int64_t *len) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = idx[i];
    len[i] = j < 0 ? 0 : off[j + 1] - off[j];
  }
}

__global__ void k_list_child_idx(const int64_t *off, const int64_t *idx, const int64_t *noff,
                                 int64_t m, int64_t *cidx) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = idx[i];
    if (j < 0) continue;
    const int64_t a = off[j], len = off[j + 1] - a, o = noff[i];
    for (int64_t q = 0; q < len; ++q) cidx[o + q] = a + q;
  }
}

__global__ void k_list_valid(const uint8_t *sval, const int64_t *idx, int64_t m, uint8_t *dval) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = idx[i];
    dval[i] = j < 0 ? 0 : (sval ? sval[j] : 1);
  }
}

ColPtr gather_list(Session *s, const ColPtr &c, const int64_t *d_idx, int64_t m) {
  BufPtr noff = s->alloc(8 * (m + 1));
  HIP_CHECK(hipMemsetAsync(noff->p, 0, 8 * (m + 1), s->stream));
  if (m == 0) return list_column(s, 0, noff, empty_elements(s, c->child->type));
  BufPtr len = s->alloc(8 * (m + 1));
  HIP_CHECK(hipMemsetAsync(len->p, 0, 8 * (m + 1), s->stream));
  const int64_t *off = (const int64_t *)c->data->p;
  hipLaunchKernelGGL(k_list_lengths, dim3(grid_for(m, 256)), dim3(256), 0, s->stream, off, d_idx, m,
                     (int64_t *)len->p);
  KERNEL_CHECK();
  const int64_t total = exclusive_scan_i64(s, (const int64_t *)len->p, (int64_t *)noff->p, m + 1);
  ColPtr child;
  if (total == 0) {
    child = empty_elements(s, c->child->type);
  } else if (c->child->type == Type::Null) {  // NULL-typed elements: only their count
    child = null_column(s, Type::Null, total);
  } else {
    BufPtr cidx = s->alloc(8 * total);
    hipLaunchKernelGGL(k_list_child_idx, dim3(grid_for(m, 256)), dim3(256), 0, s->stream, off, d_idx,
                       (const int64_t *)noff->p, m, (int64_t *)cidx->p);
    KERNEL_CHECK();
    child = gather_column(s, c->child, (const int64_t *)cidx->p, total);
  }
  ColPtr o = list_column(s, m, noff, child);
  o->valid = s->alloc(m);
  hipLaunchKernelGGL(k_list_valid, dim3(grid_for(m, 256)), dim3(256), 0, s->stream,
                     c->valid ? (const uint8_t *)c->valid->p : nullptr, d_idx, m,
                     (uint8_t *)o->valid->p);
  KERNEL_CHECK();
  return o;
}

// ---------------------------------------------------------------- UNWIND
// withColumns(Explode(list) AS item) (RelationalPlanner.scala:99-101): row i of
// the output is input row i / k with element i % k of the constant list
// (k elements): two index columns, every input column a lazy gather of the
// first, the element column a gather of the second.
__global__ void k_explode_idx(int64_t m, int64_t k, int64_t *row, int64_t *elem) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / k;
    row[i] = r;
    elem[i] = i - r * k;
  }
}

DataPtr explode_values(Session *s, const Data &d, const ColPtr &values) {
  const int64_t k = values->n, m = d.nrows * k;
  auto out = std::make_shared<Data>();
  out->nrows = m;
  BufPtr row = s->alloc(8 * std::max<int64_t>(m, 1)), elem = s->alloc(8 * std::max<int64_t>(m, 1));
  if (m > 0) {
    hipLaunchKernelGGL(k_explode_idx, dim3(grid_for(m, 256)), dim3(256), 0, s->stream, m, k,
                       (int64_t *)row->p, (int64_t *)elem->p);
    KERNEL_CHECK();
  }
  IdxCache cache;
  for (auto &c : d.cols) out->cols.push_back(gather_lazy(s, c, row, m, false, &cache));
  out->cols.push_back(m > 0 ? gather_column(s, values, (const int64_t *)elem->p, m)
                            : (values->type == Type::Null ? null_column(s, Type::Null, 0)
                                                          : make_column(s, values->type, 0, false)));
  return out;
}

// a LIST column: output rows [off[r], off[r+1]) come from input row r and
// hold its elements in order (the element column is the list's child, as is)
__global__ void k_explode_list_rows(const int64_t *off, const uint8_t *valid, int64_t n, int64_t *row) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n;
       r += (int64_t)gridDim.x * blockDim.x) {
    if (valid && !valid[r]) continue;
    for (int64_t q = off[r]; q < off[r + 1]; ++q) row[q] = r;
  }
}
// drop the elements of NULL lists: their element rows keep row = -1
__global__ void k_row_flags(const int64_t *row, int64_t n, uint8_t *flags) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    flags[i] = row[i] >= 0 ? 1 : 0;
}

DataPtr explode_list(Session *s, const Data &d, int list_col) {
  const ColPtr &lc = d.cols[(size_t)list_col];
  auto out = std::make_shared<Data>();
  if (lc->type == Type::Null || d.nrows == 0) {  // nothing to unwind
    out->nrows = 0;
    BufPtr none = s->alloc(8);
    for (auto &c : d.cols) out->cols.push_back(gather_column(s, c, (const int64_t *)none->p, 0, false));
    out->cols.push_back(null_column(s, lc->type == Type::Null ? Type::Null : lc->child->type, 0));
    return out;
  }
  force(lc);
  int64_t total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, (const int64_t *)lc->data->p + d.nrows, 8, hipMemcpyDeviceToHost, s->stream));
  s->sync();
  BufPtr row = s->alloc(8 * std::max<int64_t>(total, 1));
  ColPtr elems = lc->child;
  int64_t m = total;
  if (total > 0) {
    HIP_CHECK(hipMemsetAsync(row->p, 0xFF, 8 * total, s->stream));
    hipLaunchKernelGGL(k_explode_list_rows, dim3(grid_for(d.nrows, 256)), dim3(256), 0, s->stream,
                       (const int64_t *)lc->data->p, lc->valid ? (const uint8_t *)lc->valid->p : nullptr, d.nrows,
                       (int64_t *)row->p);
    KERNEL_CHECK();
    if (lc->valid) {  // elements of NULL lists (if any were stored) are dropped
      BufPtr flags = s->alloc(total);
      hipLaunchKernelGGL(k_row_flags, dim3(grid_for(total, 256)), dim3(256), 0, s->stream,
                         (const int64_t *)row->p, total, (uint8_t *)flags->p);
      KERNEL_CHECK();
      BufPtr keep = compact_flags(s, (const uint8_t *)flags->p, total, &m);
      if (m != total) {
        ColPtr r64 = std::make_shared<Column>();
        r64->type = Type::Int64;
        r64->n = total;
        r64->data = row;
        row = gather_column(s, r64, (const int64_t *)keep->p, m)->data;
        elems = gather_column(s, elems, (const int64_t *)keep->p, m);
      }
    }
  }
  out->nrows = m;
  IdxCache cache;
  for (auto &c : d.cols) out->cols.push_back(gather_lazy(s, c, row, m, false, &cache));
  out->cols.push_back(elems);
  return out;
}

// ---------------------------------------------------------- labels / keys
// labels(n) / keys(n) (FlinkSQLExprMapper.scala:136-153, the GetLabels /
// GetKeys UDFs at :310-329): per row the names (STRING codes, caller-sorted)
// of the label columns holding TRUE (kind 0) or of the property columns
// holding a value (kind 1).  A row with none gets the empty list (the UDFs
// return an empty array, never NULL).  Two passes: per-row counts → offsets
// (exclusive scan) → the codes written in column order.
constexpr int NL_MAX = 64;
struct NameCols {
  ColView c[NL_MAX];
  int32_t kind[NL_MAX];
  int64_t code[NL_MAX];
  int32_t n;
};

__device__ inline bool nl_hit(const NameCols &nc, int j, int64_t r) {
  const ColView &v = nc.c[j];
  if (v.type == CAPF_TYPE_NULL || !v.data || (v.valid && !v.valid[r])) return false;
  return nc.kind[j] ? true : ((const uint8_t *)v.data)[r] != 0;
}

__global__ void k_name_counts(NameCols nc, int64_t n, int64_t *cnt) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    int64_t k = 0;
    for (int j = 0; j < nc.n; ++j) k += nl_hit(nc, j, r) ? 1 : 0;
    cnt[r] = k;
  }
}

__global__ void k_name_fill(NameCols nc, int64_t n, const int64_t *off, int64_t *codes) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    int64_t o = off[r];
    for (int j = 0; j < nc.n; ++j)
      if (nl_hit(nc, j, r)) codes[o++] = nc.code[j];
  }
}

ColPtr name_list_column(Session *s, const Data &d, const std::vector<int> &cols, const std::vector<int32_t> &kinds,
                        const std::vector<int64_t> &codes) {
  if (cols.size() > (size_t)NL_MAX) not_impl("labels / keys over more than 64 columns");
  NameCols nc{};
  nc.n = (int32_t)cols.size();
  for (size_t j = 0; j < cols.size(); ++j) {
    const ColPtr &c = d.cols[(size_t)cols[j]];
    if (kinds[j] == 0 && c->type != Type::Bool && c->type != Type::Null) illegal("label column is not BOOLEAN");
    if (c->type == Type::List) not_impl("keys() over a LIST property");
    nc.c[j] = c->type == Type::Null ? ColView{nullptr, nullptr, CAPF_TYPE_NULL, ENC_PLAIN, 0} : view_of(c);
    nc.kind[j] = kinds[j];
    nc.code[j] = codes[j];
  }
  const int64_t n = d.nrows;
  BufPtr off = s->alloc(8 * (n + 1));
  int64_t total = 0;
  if (n > 0) {
    BufPtr cnt = s->alloc(8 * n);
    hipLaunchKernelGGL(k_name_counts, dim3(grid_for(n, 256)), dim3(256), 0, s->stream, nc, n, (int64_t *)cnt->p);
    KERNEL_CHECK();
    total = exclusive_scan_i64(s, (const int64_t *)cnt->p, (int64_t *)off->p, n);
  }
  HIP_CHECK(hipMemcpyAsync((int64_t *)off->p + n, &total, 8, hipMemcpyHostToDevice, s->stream));
  ColPtr child = make_column(s, Type::String, total, false);
  if (total > 0) {
    hipLaunchKernelGGL(k_name_fill, dim3(grid_for(n, 256)), dim3(256), 0, s->stream, nc, n, (const int64_t *)off->p,
                       (int64_t *)child->data->p);
    KERNEL_CHECK();
  }
  s->sync();  // (the pageable total)
  return list_column(s, n, off, child);
}

// ------------------------------------------------- list literals per row
// Row i's list = (item 0's value, ..., item k-1's value): element o = i·k + j
// of the child is item j at row i (an INTEGER widened to FLOAT when the
// list's element type is FLOAT).  One launch, one thread per output element,
// the item views passed by value: lane l stores child[o + l] (contiguous
// 8-B / 1-B stores) and reads item j's rows in runs of ⌈64 / k⌉.  A NULL item
// value stores 0 and validity 0; the validity bytes are written only when
// some item can be NULL (cvalid non-null).  Literals longer than LI_MAX items
// run in batches of items [j0, j0 + nb).  o / nb is taken once per thread:
// the grid-stride step advances (i, j) by (stride / nb, stride % nb).
constexpr int LI_MAX = 64;
struct ListItems {
  ColView c[LI_MAX];
  int32_t nb;    // items of this batch
  int32_t j0;    // first item of this batch
  int32_t k;     // items of the literal (the row stride of the child)
  int32_t elem;  // the list's element type
};

__global__ void k_list_fill(ListItems it, int64_t n, void *child, uint8_t *cvalid) {
  const int64_t total = n * it.nb, stride = (int64_t)gridDim.x * blockDim.x;
  int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= total) return;
  int64_t i = o / it.nb;
  int32_t j = (int32_t)(o - i * it.nb);
  const int64_t di = stride / it.nb;
  const int32_t dj = (int32_t)(stride - di * it.nb);
  for (; o < total; o += stride) {
    const ColView &c = it.c[j];
    const bool ok = c.type != CAPF_TYPE_NULL && c.data && !(c.valid && !c.valid[i]);
    const int64_t d = i * it.k + it.j0 + j;
    if (it.elem == CAPF_TYPE_BOOL) {
      ((uint8_t *)child)[d] = ok && ((const uint8_t *)c.data)[i] ? 1 : 0;
    } else if (it.elem == CAPF_TYPE_FLOAT64) {
      ((double *)child)[d] = !ok ? 0.0 : c.type == CAPF_TYPE_FLOAT64 ? ((const double *)c.data)[i] : (double)ld_int(c, i);
    } else {
      ((int64_t *)child)[d] = ok ? ld_int(c, i) : 0;
    }
    if (cvalid) cvalid[d] = ok ? 1 : 0;
    i += di;
    j += dj;
    if (j >= it.nb) {
      j -= it.nb;
      ++i;
    }
  }
}

__global__ void k_list_offsets_stride(int64_t *off, int64_t n, int32_t k) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x)
    off[i] = i * k;
}

ColPtr list_from_columns(Session *s, const Data &d, const std::vector<int> &cols, Type elem) {
  const int64_t n = d.nrows;
  const int32_t k = (int32_t)cols.size();
  BufPtr off = s->alloc(8 * (n + 1));
  hipLaunchKernelGGL(k_list_offsets_stride, dim3(grid_for(n + 1, 256)), dim3(256), 0, s->stream,
                     (int64_t *)off->p, n, k);
  KERNEL_CHECK();
  if (k == 0) return list_column(s, n, off, empty_elements(s, elem));
  // every item NULL-typed: n·k NULL elements, no buffers
  if (elem == Type::Null) return list_column(s, n, off, null_column(s, Type::Null, n * k));
  std::vector<ColView> views;
  bool nullable = false;
  for (int32_t j = 0; j < k; ++j) {
    const ColPtr &c = d.cols[(size_t)cols[(size_t)j]];
    views.push_back(c->type == Type::Null ? ColView{nullptr, nullptr, CAPF_TYPE_NULL, ENC_PLAIN, 0} : view_of(c));
    nullable = nullable || c->type == Type::Null || c->valid;  // (view_of forced c)
  }
  ColPtr child = make_column(s, elem, n * k, nullable);
  if (n > 0) {
    for (int32_t j0 = 0; j0 < k; j0 += LI_MAX) {
      ListItems it{};
      it.nb = std::min<int32_t>(LI_MAX, k - j0);
      it.j0 = j0;
      it.k = k;
      it.elem = (int32_t)elem;
      for (int32_t j = 0; j < it.nb; ++j) it.c[j] = views[(size_t)(j0 + j)];
      hipLaunchKernelGGL(k_list_fill, dim3(grid_for(n * it.nb, 256)), dim3(256), 0, s->stream, it, n,
                         child->data->p, child->valid ? (uint8_t *)child->valid->p : nullptr);
      KERNEL_CHECK();
    }
  }
  return list_column(s, n, off, child);
}

// ----------------------------------------------------------- list functions
// slice / reverse / concat / range (capf_table_list_fn; okapi Expr.scala
// :640-653, 859-880, 1166-1176; the Morpheus lowering SparkSQLExprMapper.scala
// :171-182, 265, 269, 336-338).  Two launches around one exclusive scan:
//   k_lfn_lengths: one thread per row → the row's result length (and, for a
//     slice, its first source element), the row validity when some input can
//     make the row NULL, the two range errors ORed into a flag word;
//   k_lfn_fill: one thread per OUTPUT ELEMENT, so a list of any length is
//     spread over lanes and blocks.  A block owns 256 consecutive output
//     elements per grid-stride step; waves 0 and 1 find the rows of the tile's
//     first and last element (the last r with off[r] <= o, an upper bound over
//     the new offsets, which steps over runs of empty rows; 64 probes per
//     round) and leave that row window in LDS; every thread then searches only
//     inside the window.
// Sources are read through ColView (ld_int), so an encoded column stays
// correct; stores are contiguous, 8 B per lane (1 B for BOOLEAN).
struct ListSide {
  const int64_t *off;    // LIST side: its offsets [n + 1]; null: a scalar side (or absent)
  const uint8_t *valid;  // LIST side: the list validity (may be null)
  ColView e;             // LIST side: the element column; scalar side: the column itself
};
struct ListFnArgs {
  int32_t fn;
  int32_t elem;  // the result's element type
  ListSide a, b;
  ColView p[3];  // SLICE: p[0] from, p[1] to; RANGE: from, to, step
  int32_t has[3];
};

constexpr uint32_t LFN_ERR_STEP0 = 1, LFN_ERR_LONG = 2;
constexpr int64_t LFN_MAX_LEN = 2147483647;  // Spark's sequence / array limit

// INTEGER argument at row r (false: NULL)
__device__ inline bool lfn_arg(const ColView &c, int64_t r, int64_t &v) {
  if (c.type == CAPF_TYPE_NULL || !c.data || (c.valid && !c.valid[r])) return false;
  v = ld_int(c, r);
  return true;
}

// a slice bound against a list of len elements: from the end when negative, clamped
__device__ inline int64_t lfn_bound(int64_t x, int64_t len) {
  if (x < 0) return x < -len ? 0 : x + len;
  return x > len ? len : x;
}

__global__ void k_lfn_lengths(ListFnArgs g, int64_t n, int64_t *len, int64_t *first, uint8_t *valid,
                              uint32_t *err) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    bool ok = true;
    int64_t k = 0;
    if (g.fn == CAPF_LIST_FN_RANGE) {
      int64_t a = 0, b = 0, st = 1;
      ok = lfn_arg(g.p[0], r, a) && lfn_arg(g.p[1], r, b) && (!g.has[2] || lfn_arg(g.p[2], r, st));
      if (ok && st == 0) {
        atomicOr(err, LFN_ERR_STEP0);
      } else if (ok && (st > 0 ? b >= a : b <= a)) {
        // the distance and the step as unsigned 64-bit values: neither wraps
        const uint64_t dist = st > 0 ? (uint64_t)b - (uint64_t)a : (uint64_t)a - (uint64_t)b;
        const uint64_t us = st > 0 ? (uint64_t)st : 0 - (uint64_t)st;
        const uint64_t q = dist / us;  // the index of the last element
        if (q >= (uint64_t)LFN_MAX_LEN) atomicOr(err, LFN_ERR_LONG);
        else k = (int64_t)q + 1;
      }
    } else {
      const bool al = g.a.off != nullptr, bl = g.b.off != nullptr;
      if (al && g.a.valid && !g.a.valid[r]) ok = false;
      if (bl && g.b.valid && !g.b.valid[r]) ok = false;
      const int64_t la = al ? g.a.off[r + 1] - g.a.off[r] : 1;
      if (g.fn == CAPF_LIST_FN_REVERSE) {
        k = la;
      } else if (g.fn == CAPF_LIST_FN_CONCAT) {
        k = la + (bl ? g.b.off[r + 1] - g.b.off[r] : 1);
      } else {  // SLICE: an empty list, like a NULL bound, gives NULL
        int64_t lo = 0, hi = la;
        if (la == 0 || (g.has[0] && !lfn_arg(g.p[0], r, lo)) || (g.has[1] && !lfn_arg(g.p[1], r, hi))) ok = false;
        lo = lfn_bound(lo, la);
        hi = lfn_bound(hi, la);
        k = hi > lo ? hi - lo : 0;
        first[r] = lo;
      }
    }
    len[r] = ok ? k : 0;
    if (valid) valid[r] = ok ? 1 : 0;
  }
}

// (lfn_store, lfn_row_of and lfn_row_of_wave: list_search.h, shared with the lambda kernels)
constexpr int LFN_BLOCK = 256;

// off: the result's offsets [n + 1], off[n] = total > 0
__global__ __launch_bounds__(LFN_BLOCK) void k_lfn_fill(ListFnArgs g, int64_t n, const int64_t *off, int64_t total,
                                                        const int64_t *first, void *child, uint8_t *cvalid) {
  __shared__ int64_t s_win[2];
  for (int64_t o0 = (int64_t)blockIdx.x * LFN_BLOCK; o0 < total; o0 += (int64_t)gridDim.x * LFN_BLOCK) {
    if (threadIdx.x < 128) {  // waves 0 and 1: the rows of the tile's first and last element
      const int64_t last = o0 + LFN_BLOCK - 1 < total ? o0 + LFN_BLOCK - 1 : total - 1;
      const int w = threadIdx.x >> 6;
      const int64_t r = lfn_row_of_wave(off, n, w ? last : o0, threadIdx.x & 63);
      if ((threadIdx.x & 63) == 0) s_win[w] = r;
    }
    __syncthreads();
    const int64_t o = o0 + threadIdx.x;
    if (o < total) {
      const int64_t r = lfn_row_of(off, s_win[0], s_win[1], o);
      const int64_t q = o - off[r];
      if (g.fn == CAPF_LIST_FN_RANGE) {
        int64_t a = 0, st = 1;
        lfn_arg(g.p[0], r, a);
        if (g.has[2]) lfn_arg(g.p[2], r, st);
        // a + q·st lies between from and to: the unsigned sum is that value
        ((int64_t *)child)[o] = (int64_t)((uint64_t)a + (uint64_t)q * (uint64_t)st);
      } else if (g.fn == CAPF_LIST_FN_SLICE) {
        lfn_store(g.a.e, g.a.off[r] + first[r] + q, g.elem, child, cvalid, o);
      } else if (g.fn == CAPF_LIST_FN_REVERSE) {
        lfn_store(g.a.e, g.a.off[r] + (off[r + 1] - off[r]) - 1 - q, g.elem, child, cvalid, o);
      } else {  // CONCAT: side A's elements, then side B's; a scalar side reads the row's value
        const int64_t la = g.a.off ? g.a.off[r + 1] - g.a.off[r] : 1;
        if (q < la) lfn_store(g.a.e, g.a.off ? g.a.off[r] + q : r, g.elem, child, cvalid, o);
        else lfn_store(g.b.e, g.b.off ? g.b.off[r] + (q - la) : r, g.elem, child, cvalid, o);
      }
    }
    __syncthreads();  // (the window is rewritten by the next step)
  }
}

static const ColView LFN_NO_COL{nullptr, nullptr, CAPF_TYPE_NULL, ENC_PLAIN, 0};

// One side of SLICE / REVERSE / CONCAT as kernel arguments; `nullable`: the
// side can give a NULL element, `row_null`: it can make the row NULL.
static ListSide list_side(const ColPtr &c, bool &nullable, bool &row_null) {
  ListSide sd{nullptr, nullptr, LFN_NO_COL};
  if (c->type == Type::List) {
    force(c);
    sd.off = c->data ? (const int64_t *)c->data->p : nullptr;  // (null only without rows: nothing launches)
    sd.valid = c->valid ? (const uint8_t *)c->valid->p : nullptr;
    row_null = row_null || c->valid;
    if (c->child && c->child->type != Type::Null) {
      sd.e = view_of(c->child);
      nullable = nullable || c->child->valid;
    } else {
      nullable = true;  // NULL-typed elements
    }
  } else if (c->type == Type::Null) {  // a NULL scalar: one NULL element
    nullable = true;
  } else {
    sd.e = view_of(c);
    nullable = nullable || c->valid;
  }
  return sd;
}

ColPtr list_fn_column(Session *s, const Data &d, int32_t fn, const std::vector<int> &cols, Type elem) {
  const int64_t n = d.nrows;
  auto arg = [&](size_t j) -> ColPtr { return j < cols.size() && cols[j] >= 0 ? d.cols[(size_t)cols[j]] : nullptr; };
  ListFnArgs g{};
  g.fn = fn;
  g.elem = (int32_t)elem;
  g.a = g.b = ListSide{nullptr, nullptr, LFN_NO_COL};
  for (auto &v : g.p) v = LFN_NO_COL;
  bool nullable = false, row_null = false;
  if (fn == CAPF_LIST_FN_RANGE) {
    for (size_t j = 0; j < 3; ++j)
      if (ColPtr c = arg(j)) {
        g.has[j] = 1;
        if (c->type != Type::Null) g.p[j] = view_of(c);
        row_null = row_null || c->type == Type::Null || c->valid;
      }
  } else {
    g.a = list_side(arg(0), nullable, row_null);
    if (fn == CAPF_LIST_FN_CONCAT) g.b = list_side(arg(1), nullable, row_null);
    if (fn == CAPF_LIST_FN_SLICE) {
      row_null = true;  // an empty list gives NULL
      for (size_t j = 1; j < 3; ++j)
        if (ColPtr c = arg(j)) {
          g.has[j - 1] = 1;
          if (c->type != Type::Null) g.p[j - 1] = view_of(c);
        }
    }
  }
  BufPtr off = s->alloc(8 * (n + 1));
  HIP_CHECK(hipMemsetAsync(off->p, 0, 8 * (n + 1), s->stream));
  if (n == 0) return list_column(s, 0, off, empty_elements(s, elem));
  BufPtr len = s->alloc(8 * (n + 1));  // len[n] = 0: the scan's last entry is the element total
  HIP_CHECK(hipMemsetAsync(len->p, 0, 8 * (n + 1), s->stream));
  BufPtr first = fn == CAPF_LIST_FN_SLICE ? s->alloc(8 * n) : nullptr;
  BufPtr valid = row_null ? s->alloc(n) : nullptr;
  BufPtr err = fn == CAPF_LIST_FN_RANGE ? s->alloc(8) : nullptr;
  if (err) HIP_CHECK(hipMemsetAsync(err->p, 0, 8, s->stream));
  hipLaunchKernelGGL(k_lfn_lengths, dim3(grid_for(n, 256)), dim3(256), 0, s->stream, g, n, (int64_t *)len->p,
                     first ? (int64_t *)first->p : nullptr, valid ? (uint8_t *)valid->p : nullptr,
                     err ? (uint32_t *)err->p : nullptr);
  KERNEL_CHECK();
  const int64_t total = exclusive_scan_i64(s, (const int64_t *)len->p, (int64_t *)off->p, n + 1);
  if (err) {  // (the scan has synchronised the stream)
    uint32_t e = 0;
    HIP_CHECK(hipMemcpyAsync(&e, err->p, 4, hipMemcpyDeviceToHost, s->stream));
    s->sync();
    if (e & LFN_ERR_STEP0) illegal("range() with a step of 0");
    if (e & LFN_ERR_LONG) illegal("range() of more than 2147483647 elements");
  }
  ColPtr child;
  if (total == 0) {
    child = empty_elements(s, elem);
  } else if (elem == Type::Null) {  // NULL-typed elements move no bytes
    child = null_column(s, Type::Null, total);
  } else {
    child = make_column(s, elem, total, nullable);
    hipLaunchKernelGGL(k_lfn_fill, dim3(grid_for(total, LFN_BLOCK)), dim3(LFN_BLOCK), 0, s->stream, g, n,
                       (const int64_t *)off->p, total, first ? (const int64_t *)first->p : nullptr,
                       child->data->p, child->valid ? (uint8_t *)child->valid->p : nullptr);
    KERNEL_CHECK();
  }
  ColPtr o = list_column(s, n, off, child);
  o->valid = valid;
  return o;
}

}  // namespace capf
