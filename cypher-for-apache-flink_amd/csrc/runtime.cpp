// runtime.cpp — session, column store, lazy plan DAG and the C-ABI entry points.
//
// Each capf_table_* function mirrors one method of the okapi Table SPI
// (okapi-relational/.../api/table/Table.scala:43-178) as implemented by
// FlinkTable (flink-cypher/.../impl/table/FlinkTable.scala:49-199).  Like the
// Flink Table API, operations only build a plan; materialisation happens on
// size / download (FlinkTable.scala:57-61).
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <sstream>

#include "capf_internal.h"

namespace capf {

bool debug_sync_enabled() {
  static const bool on = [] {
    const char *e = getenv("CAPF_DEBUG_SYNC");
    return e && e[0] == '1';
  }();
  return on;
}

const char *type_name(Type t) {
  switch (t) {
    case Type::Null: return "NULL";
    case Type::Int64: return "INTEGER";
    case Type::Float64: return "FLOAT";
    case Type::Bool: return "BOOLEAN";
    case Type::String: return "STRING";
    case Type::List: return "LIST";
    case Type::Date: return "DATE";
    case Type::LocalDateTime: return "LOCALDATETIME";
  }
  return "?";
}

static int alloc_mode() {  // CAPF_ALLOC=sync → hipMalloc/hipFree per buffer (diagnostics)
  static const int m = [] {
    const char *e = getenv("CAPF_ALLOC");
    return (e && strcmp(e, "sync") == 0) ? 1 : 0;
  }();
  return m;
}

static size_t round_block(size_t bytes) {
  // 256 B granule below 1 MiB, 2 MiB granule above: big buffers of similar
  // size (per-query histograms, gathers) are reused across queries
  if (bytes < (size_t(1) << 20)) return (bytes + 255) & ~size_t(255);
  const size_t g = size_t(2) << 20;
  return (bytes + g - 1) / g * g;
}

void *BlockCache::get(size_t rounded) {
  auto it = free_blocks.lower_bound(rounded);
  // reuse a cached block up to 25 % larger than needed
  if (it != free_blocks.end() && it->first <= rounded + rounded / 4) {
    void *p = it->second;
    cached -= it->first;
    free_blocks.erase(it);
    return p;
  }
  return nullptr;
}

void BlockCache::put(void *p) {
  auto it = sizes.find(p);
  if (it == sizes.end()) return;
  free_blocks.emplace(it->second, p);
  cached += it->second;
}

void BlockCache::release_all() {
  for (auto &kv : free_blocks) {
    sizes.erase(kv.second);
    (void)hipFree(kv.second);
  }
  free_blocks.clear();
  cached = 0;
}

DevBuf::~DevBuf() {
  if (owned && p) {
    if (alloc_mode() == 1) {
      if (s && s->stream) (void)hipStreamSynchronize(s->stream);
      (void)hipFree(p);
    } else if (s) {
      s->cache.put(p);  // stream-ordered reuse, no synchronisation
    } else {
      (void)hipFree(p);
    }
  }
}

BufPtr Session::alloc(size_t bytes) {
  auto b = std::make_shared<DevBuf>();
  b->s = this;
  b->bytes = bytes;
  if (bytes == 0) return b;
  const size_t rounded = round_block(bytes);  // keeps every column 16-B aligned
  if (alloc_mode() == 1) {
    HIP_CHECK(hipMalloc(&b->p, rounded));
  } else {
    b->p = cache.get(rounded);
    if (!b->p) {
      hipError_t e = hipMalloc(&b->p, rounded);
      if (e == hipErrorOutOfMemory) {  // give cached blocks back and retry once
        (void)hipGetLastError();
        HIP_CHECK(hipStreamSynchronize(stream));
        cache.release_all();
        e = hipMalloc(&b->p, rounded);
      }
      HIP_CHECK(e);
      cache.sizes[b->p] = rounded;
    }
  }
  if (getenv("CAPF_POISON")) HIP_CHECK(hipMemsetAsync(b->p, 0xA5, rounded, stream));
  return b;
}

void Session::sync() { HIP_CHECK(hipStreamSynchronize(stream)); }

hipEvent_t Session::get_event() {
  if (!event_pool.empty()) {
    hipEvent_t e = event_pool.back();
    event_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  HIP_CHECK(hipEventCreate(&e));
  return e;
}

// Resolve recorded kernel timings (synchronises on the recorded events only
// when the profile is read, so timing never perturbs the timed region).
void Session::resolve_profile() {
  for (auto &p : pending) {
    (void)hipEventSynchronize(p.b);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, p.a, p.b);
    auto &e = profile[p.name];
    e.launches++;
    e.total_ms += ms;
    e.bytes += p.bytes;
    event_pool.push_back(p.a);
    event_pool.push_back(p.b);
  }
  pending.clear();
}

KernelTimer::KernelTimer(Session *s_, const char *n, double by) : s(s_), name(n), bytes(by) {
  if (!s->profiling) return;
  a = s->get_event();
  b = s->get_event();
  HIP_CHECK(hipEventRecord(a, s->stream));
}

KernelTimer::~KernelTimer() {
  if (!a) return;
  (void)hipEventRecord(b, s->stream);
  s->pending.push_back(PendingTiming{name, bytes, a, b});
}

int Node::col_index(const std::string &name) const {
  for (size_t i = 0; i < names.size(); ++i)
    if (names[i] == name) return (int)i;
  return -1;
}

int Node::col_index_or_throw(const std::string &name) const {
  int i = col_index(name);
  if (i < 0) {
    std::ostringstream os;
    os << "column '" << name << "' not found; available: [";
    for (size_t k = 0; k < names.size(); ++k) os << (k ? ", " : "") << names[k];
    os << "]";
    illegal(os.str());
  }
  return i;
}

Program Program::from_c(const capf_expr *e) {
  Program p;
  if (!e) illegal("null expression program");
  if (e->n <= 0) illegal("empty expression program");
  p.code.resize(e->n);
  for (int i = 0; i < e->n; ++i) {
    p.code[i].op = e->ops[i];
    p.code[i].pad = 0;
    p.code[i].i = e->iargs ? e->iargs[i] : 0;
    p.code[i].f = e->fargs ? e->fargs[i] : 0.0;
  }
  for (int i = 0; i < e->n_names; ++i) p.names.emplace_back(e->names[i]);
  for (auto &in : p.code)
    if (in.op == OP_COL && (in.i < 0 || in.i >= (int64_t)p.names.size()))
      illegal("column reference out of range in expression program");
  return p;
}

std::vector<std::string> Program::referenced() const {
  std::vector<std::string> r;
  for (auto &in : code)
    if (in.op == OP_COL || in.op == OP_LIST_SIZE || in.op == OP_LIST_INDEX || in.op == OP_IN_LIST)
      r.push_back(names[in.i]);
  return r;
}

static bool is_numeric(Type t) { return t == Type::Int64 || t == Type::Float64; }

Type infer_type(const Program &p, const std::vector<std::string> &names,
                const std::vector<Type> &types, const std::vector<Type> *lambda) {
  std::vector<Type> st;
  bool list_ref = false;
  auto pop = [&]() {
    if (st.empty()) illegal("malformed expression program (stack underflow)");
    Type t = st.back();
    st.pop_back();
    return t;
  };
  // a DATE / LOCALDATETIME takes comparison with its own type, IS [NOT] NULL,
  // COALESCE, IF, IN, its accessors and + duration: nothing numeric
  auto no_temporal = [&](Type t, const char *what) {
    if (is_temporal(t)) illegal(std::string(what) + " of a " + type_name(t) + " value");
  };
  for (auto &in : p.code) {
    switch (in.op) {
      case OP_COL: {
        const std::string &nm = p.names[in.i];
        int idx = -1;
        for (size_t k = 0; k < names.size(); ++k)
          if (names[k] == nm) idx = (int)k;
        if (idx < 0) illegal("expression references unknown column '" + nm + "'");
        list_ref |= types[idx] == Type::List;
        st.push_back(types[idx]);
        break;
      }
      case OP_LAMBDA:  // a lambda slot: only inside a lambda body (capf_table_list_lambda)
        if (!lambda || in.i < 0 || (size_t)in.i >= lambda->size())
          illegal("a lambda variable outside the expression that binds it");
        st.push_back((*lambda)[(size_t)in.i]);
        break;
      case OP_LIT_INT: st.push_back(Type::Int64); break;
      case OP_LIT_FLOAT: st.push_back(Type::Float64); break;
      case OP_LIT_BOOL: st.push_back(Type::Bool); break;
      case OP_LIT_STRING: st.push_back(Type::String); break;
      case OP_LIT_TEMPORAL: {
        const Type t = in.f == (double)CAPF_TYPE_DATE            ? Type::Date
                       : in.f == (double)CAPF_TYPE_LOCALDATETIME ? Type::LocalDateTime
                                                                 : Type::Null;
        if (t == Type::Null) illegal("a temporal literal must be typed DATE or LOCALDATETIME");
        st.push_back(t);
        break;
      }
      case OP_TEMPORAL_FIELD: {
        Type a = pop();
        if (a != Type::Null && !is_temporal(a))
          illegal(std::string("a temporal accessor on ") + type_name(a));
        if (in.i < CAPF_TEMPORAL_YEAR || in.i > CAPF_TEMPORAL_MICROSECOND) illegal("temporal field out of range");
        if (a == Type::Date && in.i >= CAPF_TEMPORAL_HOUR) illegal("a time accessor on a DATE");
        st.push_back(Type::Int64);
        break;
      }
      case OP_TEMPORAL_ADD: {
        Type a = pop();
        if (a != Type::Null && !is_temporal(a))
          illegal(std::string("a duration added to ") + type_name(a));
        // (the kernel adds the months to 12 · year in 32 bits)
        if (!(in.f >= -1073741824.0 && in.f <= 1073741824.0) || in.f != (double)(int64_t)in.f)
          illegal("duration months out of range");
        st.push_back(a);
        break;
      }
      case OP_LIT_NULL: {
        Type t = (Type)in.i;
        if (in.i < 0 || (in.i > 4 && !is_temporal(t))) t = Type::Null;
        st.push_back(t);
        break;
      }
      case OP_EQ: case OP_NEQ: case OP_LT: case OP_LE: case OP_GT: case OP_GE: {
        Type b = pop(), a = pop();
        bool ordered = in.op != OP_EQ && in.op != OP_NEQ;
        if (a != Type::Null && b != Type::Null) {
          if (ordered && (a == Type::String || b == Type::String))
            not_impl("ordering comparison on strings");
          if (!(a == b || (is_numeric(a) && is_numeric(b))))
            illegal(std::string("cannot compare ") + type_name(a) + " with " + type_name(b));
        }
        st.push_back(Type::Bool);
        break;
      }
      case OP_NOT: pop(); st.push_back(Type::Bool); break;
      case OP_AND: case OP_OR: {
        if (in.i < 0) illegal("negative arity");
        for (int64_t k = 0; k < in.i; ++k) pop();
        st.push_back(Type::Bool);
        break;
      }
      case OP_IS_NULL: case OP_IS_NOT_NULL: pop(); st.push_back(Type::Bool); break;
      case OP_ADD: case OP_SUB: case OP_MUL: case OP_DIV: case OP_MOD: {
        Type b = pop(), a = pop();
        no_temporal(a, "arithmetic");
        no_temporal(b, "arithmetic");
        if ((a != Type::Null && !is_numeric(a)) || (b != Type::Null && !is_numeric(b)))
          not_impl(std::string("arithmetic on ") + type_name(a) + " and " + type_name(b));
        if (a == Type::Float64 || b == Type::Float64)
          st.push_back(Type::Float64);
        else if (a == Type::Null && b == Type::Null)
          st.push_back(Type::Null);
        else
          st.push_back(Type::Int64);
        break;
      }
      case OP_NEG: {
        Type a = pop();
        no_temporal(a, "negation");
        if (a != Type::Null && !is_numeric(a)) not_impl("negation of non-numeric");
        st.push_back(a);
        break;
      }
      case OP_TO_FLOAT: {
        Type a = pop();
        no_temporal(a, "toFloat");
        if (a == Type::String) not_impl("toFloat on strings");
        st.push_back(Type::Float64);
        break;
      }
      case OP_TO_INTEGER: {
        Type a = pop();
        no_temporal(a, "toInteger");
        if (a == Type::String) not_impl("toInteger on strings");
        st.push_back(Type::Int64);
        break;
      }
      case OP_COALESCE: {
        if (in.i <= 0) illegal("coalesce arity");
        Type r = Type::Null;
        for (int64_t k = 0; k < in.i; ++k) {
          Type t = pop();
          if (t == Type::Null) continue;
          if (r == Type::Null)
            r = t;
          else if (r != t) {
            if (is_numeric(r) && is_numeric(t))
              r = Type::Float64;
            else
              illegal("coalesce over incompatible types");
          }
        }
        st.push_back(r);
        break;
      }
      case OP_IN_SET: {
        if (in.i < 0 || (size_t)in.i >= p.names.size() || !is_literal_set_name(p.names[in.i]))
          illegal("malformed expression program (literal set)");
        Type a = pop();
        if (!is_int_payload(a) && a != Type::String && a != Type::Null) illegal("IN set over a non-integer value");
        st.push_back(Type::Bool);
        break;
      }
      case OP_STR_LEN: {
        Type a = pop();
        if (a != Type::String && a != Type::Null) illegal("size() of a non-string value");
        st.push_back(Type::Int64);
        break;
      }
      case OP_STR_RANK: {
        Type a = pop();
        if (a != Type::String && a != Type::Null) illegal("string rank of a non-string value");
        st.push_back(Type::Int64);
        break;
      }
      case OP_STR_MATCH: {
        if (in.i < 0 || in.i > 2) illegal("string predicate kind out of range");
        Type b = pop(), a = pop();
        if ((a != Type::String && a != Type::Null) || (b != Type::String && b != Type::Null))
          illegal("STARTS WITH / ENDS WITH / CONTAINS of a non-string value");
        st.push_back(Type::Bool);
        break;
      }
      case OP_VALUE_MAP: {
        if (in.i < 0 || (size_t)in.i >= p.names.size() || !is_value_map_name(p.names[in.i]))
          illegal("malformed expression program (value map)");
        pop();
        if (in.f != 0.0) pop();
        st.push_back(Type::String);
        break;
      }
      case OP_STR_MAP: {
        if (in.i < 0 || (size_t)in.i >= p.names.size() || !is_code_map_name(p.names[in.i]))
          illegal("malformed expression program (code map)");
        Type a = pop();
        if (a != Type::String && a != Type::Null) illegal("string function of a non-string value");
        st.push_back(Type::String);
        break;
      }
      case OP_LIST_SIZE: {
        if (in.i < 0 || (size_t)in.i >= p.names.size()) illegal("malformed expression program (column)");
        const std::string &nm = p.names[in.i];
        int idx = -1;
        for (size_t k = 0; k < names.size(); ++k)
          if (names[k] == nm) idx = (int)k;
        if (idx < 0) illegal("expression references unknown column '" + nm + "'");
        if (types[idx] != Type::List && types[idx] != Type::Null) illegal("size() of a non-list column");
        st.push_back(Type::Int64);
        break;
      }
      case OP_IF: {
        Type v = pop(), c = pop(), e = pop();
        if (c != Type::Bool && c != Type::Null) illegal("condition is not boolean");
        if (v != Type::Null && e != Type::Null && v != e) {
          if (!(is_numeric(v) && is_numeric(e))) illegal("branches of different types");
          v = Type::Float64;  // numeric branches widen (Calcite's CASE type)
        }
        st.push_back(v != Type::Null ? v : e);
        break;
      }
      case OP_ROUND: case OP_ABS: case OP_CEIL: case OP_FLOOR: case OP_SIGN: case OP_SQRT:
      case OP_LOG: case OP_LOG10: case OP_EXP: case OP_SIN: case OP_COS: case OP_TAN:
      case OP_ASIN: case OP_ACOS: case OP_ATAN: case OP_DEGREES: case OP_RADIANS: {
        Type a = pop();
        no_temporal(a, "a math function");
        if (a != Type::Null && !is_numeric(a)) not_impl(std::string("math function on ") + type_name(a));
        const bool keeps = in.op == OP_ABS || in.op == OP_CEIL || in.op == OP_FLOOR || in.op == OP_SIGN;
        st.push_back(keeps && a == Type::Int64 ? Type::Int64 : Type::Float64);
        break;
      }
      case OP_ATAN2: {
        Type b = pop(), a = pop();
        no_temporal(a, "atan2");
        no_temporal(b, "atan2");
        if ((a != Type::Null && !is_numeric(a)) || (b != Type::Null && !is_numeric(b)))
          not_impl("atan2 of non-numeric values");
        st.push_back(Type::Float64);
        break;
      }
      case OP_TO_BOOLEAN: {
        Type a = pop();
        no_temporal(a, "toBoolean");
        if (a != Type::Null && a != Type::Bool && a != Type::String)
          not_impl(std::string("toBoolean on ") + type_name(a));
        st.push_back(Type::Bool);
        break;
      }
      case OP_STR_TO_NUM: {
        Type a = pop();
        if (a != Type::Null && a != Type::String) illegal("toFloat / toInteger of a string: operand is not a STRING");
        st.push_back(in.i == 1 ? Type::Float64 : Type::Int64);
        break;
      }
      case OP_RAND: st.push_back(Type::Float64); break;
      case OP_LIST_INDEX: {
        if (in.i < 0 || (size_t)in.i >= p.names.size()) illegal("malformed expression program (column)");
        const std::string &nm = p.names[in.i];
        int idx = -1;
        for (size_t k = 0; k < names.size(); ++k)
          if (names[k] == nm) idx = (int)k;
        if (idx < 0) illegal("expression references unknown column '" + nm + "'");
        if (types[idx] != Type::List && types[idx] != Type::Null) illegal("index into a non-list column");
        Type ix = pop();
        if (ix != Type::Null && ix != Type::Int64) illegal("a list index must be an INTEGER");
        const int et = (int)in.f;
        if (et < 0 || et > 4) illegal("list element type out of range");
        st.push_back((Type)et);
        break;
      }
      case OP_IN_LIST: {
        if (in.i < 0 || (size_t)in.i >= p.names.size()) illegal("malformed expression program (column)");
        const std::string &nm = p.names[in.i];
        int idx = -1;
        for (size_t k = 0; k < names.size(); ++k)
          if (names[k] == nm) idx = (int)k;
        if (idx < 0) illegal("expression references unknown column '" + nm + "'");
        if (types[idx] != Type::List && types[idx] != Type::Null) illegal("IN over a non-list column");
        const int et = (int)in.f;
        if (et < 0 || et > 4) illegal("list element type out of range");
        pop();
        st.push_back(Type::Bool);
        break;
      }
      default: not_impl("expression opcode " + std::to_string(in.op));
    }
  }
  if (st.size() != 1) illegal("malformed expression program (stack not singular)");
  // a list column can be projected (a bare reference), not computed on
  if (list_ref && p.code.size() != 1) not_impl("expressions over list values");
  return st.back();
}

ColPtr make_column(Session *s, Type t, int64_t n, bool with_valid) {
  auto c = std::make_shared<Column>();
  c->type = t;
  c->n = n;
  if (t != Type::Null && n > 0) c->data = s->alloc(type_width(t) * n);
  if (with_valid && n > 0) c->valid = s->alloc(n);
  return c;
}

ColPtr null_column(Session *s, Type t, int64_t n) {
  (void)s;
  auto c = std::make_shared<Column>();
  c->type = Type::Null;
  c->n = n;
  (void)t;
  return c;
}

ColView view_of(const ColPtr &c) {
  // LIST columns (collect results) are projected, gathered and downloaded,
  // never read by a row kernel: keys, predicates and sort items over lists
  // are not supported (Flink: no comparison on MULTISET either)
  if (c->type == Type::List) not_impl("list values as keys, predicates or sort items");
  force(c);
  ColView v;
  v.data = c->data ? c->data->p : nullptr;
  v.valid = c->valid ? (const uint8_t *)c->valid->p : nullptr;
  v.type = (int32_t)c->type;
  v.enc = c->enc;
  v.base = c->base;
  return v;
}

const ColStats &column_stats(Session *s, const ColPtr &c) {
  if (c->type == Type::List) not_impl("statistics of a list column");
  force(c);
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->stats) c->stats = compute_stats(s, *c);
  return *c->stats;
}

// ------------------------------------------------------------- materialise
static DataPtr materialize_impl(const NodePtr &n);

DataPtr materialize(const NodePtr &n) {
  std::lock_guard<std::mutex> g(n->mu);
  if (!n->result) n->result = materialize_impl(n);
  return n->result;
}

static DataPtr gather_all(Session *s, const Data &d, const BufPtr &idx, int64_t m) {
  IdxCache cache;
  auto out = std::make_shared<Data>();
  out->nrows = m;
  for (auto &c : d.cols) out->cols.push_back(gather_lazy(s, c, idx, m, false, &cache));
  return out;
}


// The output of a join node n from its inputs' row indexes (lazy gathers).
static DataPtr join_output(Session *s, const NodePtr &n, const Data &l, const Data &r, const BufPtr &li,
                           const BufPtr &ri, int64_t m, int key_alias, int build_unread = 0, int iw = 8) {
  auto out = std::make_shared<Data>();
  out->nrows = m;
  bool lnull = n->join_type == CAPF_JOIN_RIGHT_OUTER || n->join_type == CAPF_JOIN_FULL_OUTER;
  bool rnull = n->join_type == CAPF_JOIN_LEFT_OUTER || n->join_type == CAPF_JOIN_FULL_OUTER;
  IdxCache cache;  // the columns of one side share one (composed) index
  // a build side without a row index: constants fill, the key is aliased below
  auto unread = [&](const ColPtr &c, bool key) -> ColPtr {
    if (key) return c;
    return const_column(s, c->is_const ? *c : *c->lazy->src, m);
  };
  for (size_t i = 0; i < l.cols.size(); ++i)
    out->cols.push_back(build_unread == 1 ? unread(l.cols[i], (int)i == n->join_keys[0].first)
                                          : gather_lazy(s, l.cols[i], li, m, lnull, &cache, iw));
  for (size_t i = 0; i < r.cols.size(); ++i)
    out->cols.push_back(build_unread == 2 ? unread(r.cols[i], (int)i == n->join_keys[0].second)
                                          : gather_lazy(s, r.cols[i], ri, m, rnull, &cache, iw));
  if (key_alias) {
    // the build key column of an inner dense join IS the probe key column
    // (equal values on every row): no gather of it
    const size_t kl = (size_t)n->join_keys[0].first, kr = l.cols.size() + (size_t)n->join_keys[0].second;
    if (key_alias == 1) out->cols[kl] = out->cols[kr];
    else out->cols[kr] = out->cols[kl];
  }
  return out;
}

static DataPtr materialize_impl(const NodePtr &n) {
  Session *s = n->s;
  switch (n->kind) {
    case Kind::Source: illegal("source table without data");
    case Kind::Select: {
      DataPtr c = materialize(n->kids[0]);
      auto out = std::make_shared<Data>();
      out->nrows = c->nrows;
      for (int i : n->sel_index) out->cols.push_back(c->cols[i]);
      return out;
    }
    case Kind::Filter: {
      const NodePtr &k = n->kids[0];
      if (k->kind == Kind::Join && k->join_type == CAPF_JOIN_INNER) {
        // WHERE over an inner radix join not materialised yet: the join's EMIT
        // filters its pairs (radix_join_filtered); the join node itself stays
        // unmaterialised (another parent would run it unfiltered)
        bool done;
        {
          std::lock_guard<std::mutex> g(k->mu);
          done = k->result != nullptr;
        }
        if (!done) {
          DataPtr l = materialize(k->kids[0]);
          DataPtr r = materialize(k->kids[1]);
          JoinPairs jp;
          if (radix_join_filtered(s, n->pred, k->names, *l, *r, k->join_keys, k->join_type, jp)) {
            const Data &lb = jp.build_sorted && jp.build_is_left ? *jp.build_sorted : *l;
            const Data &rb = jp.build_sorted && !jp.build_is_left ? *jp.build_sorted : *r;
            return join_output(s, k, lb, rb, jp.left, jp.right, jp.n, 0, 0, jp.iw);
          }
        }
      }
      DataPtr c = materialize(k);
      return filter_select(s, n->pred, k->names, *c);
    }
    case Kind::Join: {
      DataPtr l = materialize(n->kids[0]);
      DataPtr r = materialize(n->kids[1]);
      BufPtr li, ri;
      int64_t m = 0;
      int key_alias = 0, build_unread = 0, iw = 8;
      DataPtr sorted_l, sorted_r;  // a radix join's build side in sorted order
      if (n->join_type == CAPF_JOIN_CROSS) {
        m = l->nrows * r->nrows;
        cross_index(s, l->nrows, r->nrows, li, ri);
      } else {
        JoinPairs jp;
        if (!dense_join(s, *l, *r, n->join_keys, n->join_type, jp))
          jp = radix_join_applies(*l, *r, n->join_keys, n->join_type)
                   ? radix_join(s, *l, *r, n->join_keys, n->join_type)
                   : hash_join(s, *l, *r, n->join_keys, n->join_type);
        li = jp.left;
        ri = jp.right;
        m = jp.n;
        key_alias = jp.key_alias;
        build_unread = jp.build_unread;
        iw = jp.iw;
        (jp.build_is_left ? sorted_l : sorted_r) = jp.build_sorted;
      }
      return join_output(s, n, sorted_l ? *sorted_l : *l, sorted_r ? *sorted_r : *r, li, ri, m, key_alias,
                         build_unread, iw);
    }
    case Kind::Union: {
      DataPtr l = materialize(n->kids[0]);
      DataPtr r = materialize(n->kids[1]);
      auto out = std::make_shared<Data>();
      out->nrows = l->nrows + r->nrows;
      for (size_t i = 0; i < n->names.size(); ++i) {
        int ri = n->kids[1]->col_index(n->names[i]);
        out->cols.push_back(concat_columns(s, l->cols[i], r->cols[ri], n->types[i]));
      }
      return out;
    }
    case Kind::Distinct: {
      DataPtr c = materialize(n->kids[0]);
      Grouping g = group_rows(s, *c, n->key_index);
      return gather_all(s, *c, g.rep_row, g.ngroups);
    }
    case Kind::Group: {
      // config 5: group(a; count(*)) over DISTINCT (a, b) of var-length paths
      if (!n->key_index.empty()) {
        DataPtr fused;
        if (try_fused_reach(n, fused)) return fused;
        // group(keys of one leaf; count(*)) over an inner-join tree: per-row weights
        if (try_fused_group_count(n, fused)) return fused;
      }
      // fused factorised count: group(∅, count(*)) over an inner-join tree
      bool all_count_star = n->key_index.empty() && !n->aggs.empty();
      for (auto &a : n->aggs) all_count_star &= a.kind == CAPF_AGG_COUNT_STAR;
      if (all_count_star) {
        int64_t cnt = 0;
        if (try_fused_count(n->kids[0], &cnt)) {
          auto out = std::make_shared<Data>();
          out->nrows = 1;
          for (size_t k = 0; k < n->aggs.size(); ++k) out->cols.push_back(scalar_i64_column(s, cnt));
          return out;
        }
      }
      DataPtr c = materialize(n->kids[0]);
      Grouping g = group_rows(s, *c, n->key_index);
      if (n->key_index.empty() && g.ngroups == 0) {
        // global aggregation over an empty input still yields one row
        g.ngroups = 1;
      }
      auto out = std::make_shared<Data>();
      out->nrows = g.ngroups;
      for (int k : n->key_index)
        out->cols.push_back(gather_column(s, c->cols[k], (const int64_t *)g.rep_row->p, g.ngroups));
      for (auto &a : n->aggs) {
        ColPtr arg;
        if (a.kind != CAPF_AGG_COUNT_STAR) {
          Type at = infer_type(a.arg, n->kids[0]->names, n->kids[0]->types);
          arg = eval_program(s, a.arg, n->kids[0]->names, *c, at);
        }
        if (a.kind == CAPF_AGG_COLLECT) {
          out->cols.push_back(collect_lists(s, g, c->nrows, arg, a.distinct));
          continue;
        }
        if (a.distinct && c->nrows > 0) {
          // agg(DISTINCT e) over the distinct (group, value) pairs: Spark semantics
          // (SparkSQLExprMapper.scala:427-429); Flink ignores the flag
          // (FlinkSQLExprMapper.scala:281-287), see DESIGN.md.
          auto gid = std::make_shared<Column>();
          gid->type = Type::Int64;
          gid->n = c->nrows;
          gid->data = g.group_of_row;
          Data pairs;
          pairs.nrows = c->nrows;
          pairs.cols = {gid, arg};
          Grouping dg = group_rows(s, pairs, {0, 1});
          const int64_t *reps = (const int64_t *)dg.rep_row->p;
          Grouping g2;
          g2.ngroups = g.ngroups;
          g2.group_of_row = gather_column(s, gid, reps, dg.ngroups)->data;
          ColPtr darg = gather_column(s, arg, reps, dg.ngroups);
          if (a.rank_to_code)
            out->cols.push_back(ranks_to_codes(s, aggregate(s, g2, *c, dg.ngroups, a.kind, darg, Type::Int64)));
          else
            out->cols.push_back(aggregate(s, g2, *c, dg.ngroups, a.kind, darg, a.out_type, a.param));
          continue;
        }
        if (a.rank_to_code) {  // min / max of STRINGs: over their ranks, back to codes
          out->cols.push_back(ranks_to_codes(s, aggregate(s, g, *c, c->nrows, a.kind, arg, Type::Int64)));
          continue;
        }
        out->cols.push_back(aggregate(s, g, *c, c->nrows, a.kind, arg, a.out_type, a.param));
      }
      return out;
    }
    case Kind::Explode: {
      DataPtr c = materialize(n->kids[0]);
      return n->explode_list_col >= 0 ? explode_list(s, *c, n->explode_list_col)
                                      : explode_values(s, *c, n->explode_values);
    }
    case Kind::NameList: {
      DataPtr c = materialize(n->kids[0]);
      auto out = std::make_shared<Data>();
      out->nrows = c->nrows;
      out->cols = c->cols;
      out->cols.push_back(name_list_column(s, *c, n->name_cols, n->name_kinds, n->name_codes));
      return out;
    }
    case Kind::ListColumns: {
      DataPtr c = materialize(n->kids[0]);
      auto out = std::make_shared<Data>();
      out->nrows = c->nrows;
      out->cols = c->cols;
      out->cols.push_back(list_from_columns(s, *c, n->name_cols, n->list_elem));
      return out;
    }
    case Kind::ListFn: {
      DataPtr c = materialize(n->kids[0]);
      auto out = std::make_shared<Data>();
      out->nrows = c->nrows;
      out->cols = c->cols;
      out->cols.push_back(n->types.back() == Type::Null
                              ? null_column(s, Type::Null, c->nrows)
                              : list_fn_column(s, *c, n->list_fn, n->name_cols, n->list_elem));
      return out;
    }
    case Kind::StrSplit: {
      DataPtr c = materialize(n->kids[0]);
      auto out = std::make_shared<Data>();
      out->nrows = c->nrows;
      out->cols = c->cols;
      out->cols.push_back(n->types.back() == Type::Null
                              ? null_column(s, Type::Null, c->nrows)
                              : str_split_column(s, *c, n->name_cols[0], n->name_cols[1]));
      return out;
    }
    case Kind::ListLambda: {
      DataPtr c = materialize(n->kids[0]);
      auto out = std::make_shared<Data>();
      out->nrows = c->nrows;
      out->cols = c->cols;
      out->cols.push_back(n->types.back() == Type::Null
                              ? null_column(s, Type::Null, c->nrows)
                              : list_lambda_column(s, *c, n->kids[0]->names, n->list_fn, n->name_cols[0], n->exprs[0],
                                                   n->exprs[1], n->name_cols[1], n->list_elem));
      return out;
    }
    case Kind::WithColumns: {
      DataPtr c = materialize(n->kids[0]);
      auto out = std::make_shared<Data>();
      out->nrows = c->nrows;
      out->cols = c->cols;
      out->cols.resize(n->names.size());
      for (size_t k = 0; k < n->exprs.size(); ++k) {
        Type t = n->types[n->target_index[k]];
        out->cols[n->target_index[k]] = eval_program(s, n->exprs[k], n->kids[0]->names, *c, t);
      }
      return out;
    }
    case Kind::OrderBy: {
      DataPtr c = materialize(n->kids[0]);
      std::vector<ColPtr> keys;
      for (auto &p : n->exprs) {
        Type t = infer_type(p, n->kids[0]->names, n->kids[0]->types);
        keys.push_back(eval_program(s, p, n->kids[0]->names, *c, t));
      }
      BufPtr perm = sort_permutation(s, keys, n->desc, c->nrows);
      return gather_all(s, *c, perm, c->nrows);
    }
    case Kind::Skip:
    case Kind::Limit: {
      DataPtr c = materialize(n->kids[0]);
      int64_t start, m;
      if (n->kind == Kind::Skip) {
        start = std::min(n->count, c->nrows);
        m = c->nrows - start;
      } else {
        start = 0;
        m = std::min(n->count, c->nrows);
      }
      BufPtr idx = iota_index(s, start, m);
      return gather_all(s, *c, idx, m);
    }
  }
  fail(CAPF_ERR_INTERNAL, "unknown plan node");
}

int64_t node_size(const NodePtr &n) {
  {
    std::lock_guard<std::mutex> g(n->mu);
    if (n->result) return n->result->nrows;
  }
  int64_t cnt = 0;
  if (n->kind == Kind::Union) return node_size(n->kids[0]) + node_size(n->kids[1]);
  if (try_fused_count(n, &cnt)) return cnt;
  return materialize(n)->nrows;
}
}  // namespace capf

// ===================================================================== C-ABI
using namespace capf;

static thread_local std::string g_err;
static thread_local int32_t g_err_kind = 0;

namespace capf {
int32_t record_error(int32_t code, const char *msg) {
  g_err = msg;
  g_err_kind = code;
  return code;
}
}  // namespace capf

#define CAPF_API_BEGIN try {
#define CAPF_API_END                                   \
  return CAPF_OK;                                      \
  }                                                    \
  catch (const capf::Error &e) {                       \
    g_err = e.what();                                  \
    g_err_kind = e.code;                               \
    return e.code;                                     \
  }                                                    \
  catch (const std::exception &e) {                    \
    g_err = e.what();                                  \
    g_err_kind = CAPF_ERR_INTERNAL;                    \
    return CAPF_ERR_INTERNAL;                          \
  }

static capf_table *wrap(NodePtr n) {
  auto *t = new capf_table;
  t->node = std::move(n);
  return t;
}

static void need(const void *p, const char *what) {
  if (!p) illegal(std::string("null argument: ") + what);
}

static NodePtr new_node(Session *s, Kind k) {
  auto n = std::make_shared<Node>();
  n->s = s;
  n->kind = k;
  return n;
}

extern "C" {

const char *capf_last_error(void) { return g_err.c_str(); }
int32_t capf_last_error_kind(void) { return g_err_kind; }
int32_t capf_abi_version(void) { return CAPF_ABI_VERSION; }

capf_status capf_session_create(int32_t device, void *hip_stream, capf_session **out) {
  CAPF_API_BEGIN
  need(out, "out");
  auto *cs = new capf_session;
  Session &s = cs->impl;
  s.device = device;
  HIP_CHECK(hipSetDevice(device));
  {
    int cus = 0;
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    if (cus > 0) s.num_cus = cus;
  }
  if (hip_stream) {
    s.stream = (hipStream_t)hip_stream;
    s.own_stream = false;
  } else {
    HIP_CHECK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    s.own_stream = true;
  }
  // freed blocks go back to the session's caching allocator (BlockCache):
  // no hipMalloc on the hot path after warm-up.
  HIP_CHECK(hipMalloc(&s.d_scalars, 64 * sizeof(int64_t)));
  HIP_CHECK(hipHostMalloc(&s.h_scalars, 64 * sizeof(int64_t), hipHostMallocDefault));
  *out = cs;
  CAPF_API_END
}

capf_status capf_session_destroy(capf_session *cs) {
  CAPF_API_BEGIN
  if (!cs) return CAPF_OK;
  Session &s = cs->impl;
  (void)hipStreamSynchronize(s.stream);
  s.resolve_profile();
  for (auto e : s.event_pool) (void)hipEventDestroy(e);
  s.cache.release_all();
  (void)hipFree(s.d_scalars);
  (void)hipHostFree(s.h_scalars);
  if (s.own_stream) (void)hipStreamDestroy(s.stream);
  delete cs;
  CAPF_API_END
}

capf_status capf_session_sync(capf_session *cs) {
  CAPF_API_BEGIN
  need(cs, "session");
  cs->impl.sync();
  CAPF_API_END
}

capf_status capf_session_alloc(capf_session *cs, int64_t bytes, void **d_out) {
  CAPF_API_BEGIN
  need(cs, "session");
  need(d_out, "d_out");
  if (bytes < 0) illegal("negative size");
  BufPtr b = cs->impl.alloc((size_t)std::max<int64_t>(bytes, 16));
  std::lock_guard<std::mutex> g(cs->impl.user_mu);
  cs->impl.user_bufs[b->p] = b;
  *d_out = b->p;
  CAPF_API_END
}

capf_status capf_session_free(capf_session *cs, void *d) {
  CAPF_API_BEGIN
  need(cs, "session");
  std::lock_guard<std::mutex> g(cs->impl.user_mu);
  if (!cs->impl.user_bufs.erase(d)) illegal("not a buffer of capf_session_alloc");
  CAPF_API_END
}

capf_status capf_session_copy(capf_session *cs, void *dst, const void *src, int64_t bytes, int32_t kind) {
  CAPF_API_BEGIN
  need(cs, "session");
  if (bytes < 0 || kind < 1 || kind > 3) illegal("bad copy");
  if (bytes == 0) return CAPF_OK;
  need(dst, "dst");
  need(src, "src");
  const hipMemcpyKind k = kind == 1 ? hipMemcpyHostToDevice : kind == 2 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)bytes, k, cs->impl.stream));
  cs->impl.sync();
  CAPF_API_END
}

capf_status capf_session_value_map(capf_session *cs, const int64_t *keys, const int64_t *keys2,
                                   const int64_t *codes, int64_t n, int32_t *map_id) {
  CAPF_API_BEGIN
  need(cs, "session");
  need(map_id, "map_id");
  if (n < 0 || (n > 0 && (!keys || !codes))) illegal("bad value map");
  for (int64_t i = 1; i < n; ++i)
    if (keys[i - 1] > keys[i] || (keys[i - 1] == keys[i] && (!keys2 || keys2[i - 1] >= keys2[i])))
      illegal("value map keys must be sorted and unique");
  const int64_t k = keys2 ? 3 : 2;
  std::vector<int64_t> h((size_t)(k * std::max<int64_t>(n, 1)), 0);
  std::copy(keys, keys + n, h.begin());
  if (keys2) std::copy(keys2, keys2 + n, h.begin() + n);
  std::copy(codes, codes + n, h.begin() + (k - 1) * n);
  Session &s = cs->impl;
  std::vector<int64_t> key(h);
  key.push_back(keys2 ? 1 : 0);
  key.push_back(n);
  {
    std::lock_guard<std::mutex> g(s.user_mu);
    auto it = s.value_map_ids.find(key);
    if (it != s.value_map_ids.end()) {
      *map_id = it->second;
      return CAPF_OK;
    }
  }
  BufPtr b = s.alloc(8 * h.size());
  HIP_CHECK(hipMemcpyAsync(b->p, h.data(), 8 * h.size(), hipMemcpyHostToDevice, s.stream));
  s.sync();  // (pageable source)
  std::lock_guard<std::mutex> g(s.user_mu);
  *map_id = (int32_t)s.value_maps.size();
  s.value_maps.push_back(Session::ValueMap{b, n, keys2 != nullptr});
  s.value_map_ids.emplace(std::move(key), *map_id);
  CAPF_API_END
}

capf_status capf_session_code_map(capf_session *cs, const int64_t *codes, int64_t n, int32_t *map_id) {
  CAPF_API_BEGIN
  need(cs, "session");
  need(map_id, "map_id");
  if (n < 0 || (n > 0 && !codes)) illegal("bad code map");
  Session &s = cs->impl;
  std::vector<int64_t> key(codes, codes + n);
  {
    std::lock_guard<std::mutex> g(s.user_mu);
    auto it = s.code_map_ids.find(key);
    if (it != s.code_map_ids.end()) {
      *map_id = it->second;
      ++s.code_map_refs[(size_t)it->second];
      return CAPF_OK;
    }
  }
  BufPtr b = s.alloc(8 * std::max<int64_t>(n, 1));
  if (n > 0) HIP_CHECK(hipMemcpyAsync(b->p, codes, 8 * n, hipMemcpyHostToDevice, s.stream));
  s.sync();  // (pageable source)
  std::lock_guard<std::mutex> g(s.user_mu);
  auto it = s.code_map_ids.find(key);  // registered meanwhile by another thread
  if (it != s.code_map_ids.end()) {
    *map_id = it->second;
    ++s.code_map_refs[(size_t)it->second];
    return CAPF_OK;
  }
  *map_id = (int32_t)s.code_maps.size();
  s.code_maps.emplace_back(b, n);
  s.code_map_refs.push_back(1);
  s.code_map_ids.emplace(std::move(key), *map_id);
  CAPF_API_END
}

capf_status capf_session_code_map_extend(capf_session *cs, int32_t map_id, const int64_t *codes, int64_t n,
                                         int32_t *new_id) {
  CAPF_API_BEGIN
  need(cs, "session");
  need(new_id, "new_id");
  if (n < 0 || (n > 0 && !codes)) illegal("bad code map");
  Session &s = cs->impl;
  std::vector<int64_t> key(codes, codes + n);
  bool in_place;
  {
    std::lock_guard<std::mutex> g(s.user_mu);
    if (map_id < 0 || (size_t)map_id >= s.code_maps.size()) illegal("unknown code map");
    const int64_t old_n = s.code_maps[(size_t)map_id].second;
    if (n < old_n) illegal("a code map only grows");
    auto old = std::find_if(s.code_map_ids.begin(), s.code_map_ids.end(),
                            [&](const std::pair<const std::vector<int64_t>, int32_t> &e) { return e.second == map_id; });
    if (old == s.code_map_ids.end() || !std::equal(old->first.begin(), old->first.end(), key.begin()))
      illegal("the extended code map must start with the map's codes");
    // shared by several registrations (equal maps of different functions), or
    // the longer map exists already: a map of its own, the old one untouched
    in_place = s.code_map_refs[(size_t)map_id] == 1 && !s.code_map_ids.count(key);
    if (!in_place) --s.code_map_refs[(size_t)map_id];
  }
  if (!in_place) return capf_session_code_map(cs, codes, n, new_id);
  BufPtr b = s.alloc(8 * std::max<int64_t>(n, 1));
  if (n > 0) HIP_CHECK(hipMemcpyAsync(b->p, codes, 8 * n, hipMemcpyHostToDevice, s.stream));
  s.sync();  // (pageable source)
  std::lock_guard<std::mutex> g(s.user_mu);
  for (auto it = s.code_map_ids.begin(); it != s.code_map_ids.end(); ++it)
    if (it->second == map_id) {
      s.code_map_ids.erase(it);
      break;
    }
  // the old table returns to the stream-ordered cache: launches already
  // enqueued keep reading it; programs naming map_id read the superset from now on
  s.code_maps[(size_t)map_id] = std::make_pair(b, n);
  s.code_map_ids.emplace(std::move(key), map_id);
  *new_id = map_id;
  CAPF_API_END
}

capf_status capf_session_literal_set(capf_session *cs, const int64_t *values, int64_t n, int32_t *set_id) {
  CAPF_API_BEGIN
  need(cs, "session");
  need(set_id, "set_id");
  if (n < 0 || (n > 0 && !values)) illegal("bad literal set");
  std::vector<int64_t> v(values, values + n);
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  Session &s = cs->impl;
  std::lock_guard<std::mutex> g(s.user_mu);
  auto it = s.literal_set_ids.find(v);
  if (it != s.literal_set_ids.end()) {
    *set_id = it->second;
    return CAPF_OK;
  }
  BufPtr b = s.alloc(8 * std::max<int64_t>((int64_t)v.size(), 1));
  if (!v.empty()) HIP_CHECK(hipMemcpyAsync(b->p, v.data(), 8 * v.size(), hipMemcpyHostToDevice, s.stream));
  s.sync();  // (pageable source)
  const int32_t id = (int32_t)s.literal_sets.size();
  s.literal_sets.emplace_back(b, (int64_t)v.size());
  s.literal_set_ids.emplace(std::move(v), id);
  *set_id = id;
  CAPF_API_END
}

capf_status capf_session_set_profiling(capf_session *cs, int32_t enabled) {
  CAPF_API_BEGIN
  need(cs, "session");
  cs->impl.profiling = enabled != 0;
  CAPF_API_END
}

capf_status capf_session_reset_profile(capf_session *cs) {
  CAPF_API_BEGIN
  need(cs, "session");
  cs->impl.resolve_profile();
  cs->impl.profile.clear();
  cs->impl.last_plan = "none";
  cs->impl.last_plan_detail.clear();
  CAPF_API_END
}

capf_status capf_session_profile_count(capf_session *cs, int32_t *n) {
  CAPF_API_BEGIN
  need(cs, "session");
  need(n, "n");
  cs->impl.resolve_profile();
  *n = (int32_t)cs->impl.profile.size();
  CAPF_API_END
}

capf_status capf_session_profile_entry(capf_session *cs, int32_t i, const char **kernel,
                                       int64_t *launches, double *total_ms, double *bytes) {
  CAPF_API_BEGIN
  need(cs, "session");
  if (i < 0 || i >= (int32_t)cs->impl.profile.size()) illegal("profile index out of range");
  auto it = cs->impl.profile.begin();
  std::advance(it, i);
  if (kernel) *kernel = it->first.c_str();
  if (launches) *launches = it->second.launches;
  if (total_ms) *total_ms = it->second.total_ms;
  if (bytes) *bytes = it->second.bytes;
  CAPF_API_END
}

const char *capf_session_last_plan(capf_session *cs) {
  return cs ? cs->impl.last_plan.c_str() : "";
}

const char *capf_session_last_plan_detail(capf_session *cs) {
  return cs ? cs->impl.last_plan_detail.c_str() : "";
}

capf_status capf_string_intern(capf_session *cs, const char *str, int64_t *code) {
  CAPF_API_BEGIN
  need(cs, "session");
  need(str, "str");
  need(code, "code");
  *code = cs->impl.dict.intern(str);
  CAPF_API_END
}

capf_status capf_string_lookup(capf_session *cs, int64_t code, const char **str) {
  CAPF_API_BEGIN
  need(cs, "session");
  need(str, "str");
  *str = cs->impl.dict.lookup(code);
  CAPF_API_END
}

capf_status capf_string_digest(capf_session *cs, int64_t *count, uint64_t *digest) {
  CAPF_API_BEGIN
  need(cs, "session");
  need(count, "count");
  need(digest, "digest");
  cs->impl.dict.digest(count, digest);
  CAPF_API_END
}

capf_status capf_string_fn_codes(capf_session *cs, int32_t fn, int64_t iarg0, int64_t iarg1, int64_t lit0,
                                 int64_t lit1, const int64_t *src, int64_t c0, int64_t n, int64_t *out) {
  CAPF_API_BEGIN
  need(cs, "session");
  if (n < 0) illegal("negative count");
  if (n > 0) need(out, "out");
  string_fn_codes(&cs->impl, fn, iarg0, iarg1, lit0, lit1, src, c0, n, out);
  CAPF_API_END
}

static void check_unique_names(const std::vector<std::string> &names) {
  for (size_t i = 0; i < names.size(); ++i)
    for (size_t j = i + 1; j < names.size(); ++j)
      if (names[i] == names[j]) illegal("duplicate column name '" + names[i] + "'");
}

static capf_status table_from(capf_session *cs, int32_t ncols, const char *const *names,
                              const int32_t *types, const void *const *data,
                              const uint8_t *const *valid, int64_t nrows, bool device,
                              bool copy, capf_table **out) {
  CAPF_API_BEGIN
  need(cs, "session");
  need(out, "out");
  if (ncols < 0 || nrows < 0) illegal("negative table dimensions");
  Session *s = &cs->impl;
  auto n = new_node(s, Kind::Source);
  auto d = std::make_shared<Data>();
  d->nrows = nrows;
  for (int i = 0; i < ncols; ++i) {
    Type t = (Type)types[i];
    if (types[i] < 0 || (types[i] > 4 && !is_temporal((Type)types[i]))) illegal("bad column type");
    n->names.emplace_back(names[i]);
    n->types.push_back(t);
    auto c = std::make_shared<Column>();
    c->type = t;
    c->n = nrows;
    size_t w = type_width(t);
    if (t != Type::Null && nrows > 0) {
      need(data[i], "column data");
      if (device && !copy) {
        c->data = std::make_shared<DevBuf>();
        c->data->p = const_cast<void *>(data[i]);
        c->data->bytes = w * nrows;
        c->data->owned = false;
        c->data->s = s;
      } else {
        c->data = s->alloc(w * nrows);
        HIP_CHECK(hipMemcpyAsync(c->data->p, data[i], w * nrows,
                                 device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                 s->stream));
      }
    }
    if (valid && valid[i] && nrows > 0) {
      if (device && !copy) {
        c->valid = std::make_shared<DevBuf>();
        c->valid->p = const_cast<uint8_t *>(valid[i]);
        c->valid->bytes = nrows;
        c->valid->owned = false;
        c->valid->s = s;
      } else {
        c->valid = s->alloc(nrows);
        HIP_CHECK(hipMemcpyAsync(c->valid->p, valid[i], nrows,
                                 device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                 s->stream));
      }
    }
    d->cols.push_back(c);
  }
  check_unique_names(n->names);
  s->sync();
  n->result = d;
  *out = wrap(n);
  CAPF_API_END
}

capf_status capf_table_from_host(capf_session *s, int32_t ncols, const char *const *names,
                                 const int32_t *types, const void *const *data,
                                 const uint8_t *const *valid, int64_t nrows, capf_table **out) {
  return table_from(s, ncols, names, types, data, valid, nrows, false, true, out);
}

capf_status capf_table_from_device(capf_session *s, int32_t ncols, const char *const *names,
                                   const int32_t *types, void *const *data,
                                   uint8_t *const *valid, int64_t nrows, int32_t copy,
                                   capf_table **out) {
  return table_from(s, ncols, names, types, (const void *const *)data,
                    (const uint8_t *const *)valid, nrows, true, copy != 0, out);
}

capf_status capf_table_unit(capf_session *cs, capf_table **out) {
  CAPF_API_BEGIN
  need(cs, "session");
  need(out, "out");
  auto n = new_node(&cs->impl, Kind::Source);
  auto d = std::make_shared<Data>();
  d->nrows = 1;
  n->result = d;
  *out = wrap(n);
  CAPF_API_END
}

capf_status capf_table_empty(capf_session *cs, int32_t ncols, const char *const *names,
                             const int32_t *types, capf_table **out) {
  std::vector<const void *> data(ncols > 0 ? ncols : 1, nullptr);
  return table_from(cs, ncols, names, types, data.data(), nullptr, 0, false, true, out);
}

capf_status capf_table_compact(capf_table *t, capf_table **out) {
  return capf_table_compact_width(t, 4, out);
}

capf_status capf_table_compact_width(capf_table *t, int32_t width, capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(out, "out");
  if (width != 3 && width != 4) illegal("compact width must be 3 (FOR24) or 4 (FOR32) bytes");
  DataPtr d = materialize(t->node);
  Session *s = t->node->s;
  auto n = new_node(s, Kind::Source);
  n->names = t->node->names;
  n->types = t->node->types;
  auto e = std::make_shared<Data>();
  e->nrows = d->nrows;
  for (const ColPtr &c : d->cols) e->cols.push_back(encode_column(s, c, width));
  s->sync();
  n->result = e;
  *out = wrap(n);
  CAPF_API_END
}

// The key column of a node-partitioned copy: a fresh (unshared) column gets the
// owner tag; a shared one (an identity gather handed back as is) does not.
static void tag_owner(ColPtr &c, int64_t lo, int64_t n_nodes, int parts, int part) {
  if (c.use_count() != 1 || c->lazy) return;
  c->owner[0] = lo;
  c->owner[1] = n_nodes;
  c->owner[2] = parts;
  c->owner[3] = part;
}

capf_status capf_table_node_partition(capf_table *t, const char *key_col, int64_t node_base,
                                      int64_t n_nodes, int32_t parts, int32_t part,
                                      capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(key_col, "key_col");
  need(out, "out");
  if (n_nodes <= 0 || n_nodes > (int64_t(1) << 31)) illegal("node count out of range");
  if (parts <= 0 || part < 0 || part >= parts) illegal("part out of range");
  const int ki = t->node->col_index_or_throw(key_col);
  if (t->node->types[ki] != Type::Int64) illegal("partition key must be an INTEGER column");
  DataPtr d = materialize(t->node);
  Session *s = t->node->s;
  const ColPtr &kc = d->cols[ki];
  force(kc);
  if (kc->valid) illegal("partition key must be non-null");
  BufPtr flags;
  const uint8_t *f = node_owner_flags(s, view_of(kc), d->nrows, node_base, n_nodes, parts, part, flags);
  int64_t m = 0;
  BufPtr idx = compact_flags(s, f, d->nrows, &m);
  auto n = new_node(s, Kind::Source);
  n->names = t->node->names;
  n->types = t->node->types;
  auto e = std::make_shared<Data>();
  e->nrows = m;
  for (const ColPtr &c : d->cols)
    e->cols.push_back(gather_column(s, decode_column(s, c), (const int64_t *)idx->p, m));
  tag_owner(e->cols[ki], node_base, n_nodes, parts, part);
  s->sync();
  n->result = e;
  *out = wrap(n);
  CAPF_API_END
}

capf_status capf_table_node_partition_diag(capf_table *t, const char *src_col, const char *dst_col,
                                           int64_t node_base, int64_t n_nodes, int32_t parts,
                                           int32_t part, capf_table **out, int64_t *n_diag) {
  CAPF_API_BEGIN
  need(t, "table");
  need(src_col, "src_col");
  need(dst_col, "dst_col");
  need(out, "out");
  need(n_diag, "n_diag");
  if (n_nodes <= 0 || n_nodes > (int64_t(1) << 31)) illegal("node count out of range");
  if (parts <= 0 || part < 0 || part >= parts) illegal("part out of range");
  const int si = t->node->col_index_or_throw(src_col), di = t->node->col_index_or_throw(dst_col);
  if (t->node->types[si] != Type::Int64 || t->node->types[di] != Type::Int64)
    illegal("partition keys must be INTEGER columns");
  DataPtr d = materialize(t->node);
  Session *s = t->node->s;
  for (int i : {si, di}) {
    force(d->cols[i]);
    if (d->cols[i]->valid) illegal("partition keys must be non-null");
  }
  int64_t m = 0;
  BufPtr idx = node_partition_diag_index(s, view_of(d->cols[si]), view_of(d->cols[di]), d->nrows, node_base,
                                         n_nodes, parts, part, &m, n_diag);
  auto n = new_node(s, Kind::Source);
  n->names = t->node->names;
  n->types = t->node->types;
  auto e = std::make_shared<Data>();
  e->nrows = m;
  for (const ColPtr &c : d->cols)
    e->cols.push_back(gather_column(s, decode_column(s, c), (const int64_t *)idx->p, m));
  tag_owner(e->cols[si], node_base, n_nodes, parts, part);
  s->sync();
  n->result = e;
  *out = wrap(n);
  CAPF_API_END
}

capf_status capf_table_hash_route(capf_table *t, int32_t nkeys, const char *const *keys,
                                  int32_t parts, int64_t *counts, capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(out, "out");
  need(counts, "counts");
  if (nkeys <= 0) illegal("at least one routing key");
  need(keys, "keys");
  DataPtr d = materialize(t->node);
  Session *s = t->node->s;
  std::vector<ColView> kv;
  for (int j = 0; j < nkeys; ++j) {
    need(keys[j], "key");
    const int ki = t->node->col_index_or_throw(keys[j]);
    const ColPtr &kc = d->cols[ki];
    if (kc->type == Type::List) illegal("a LIST column cannot be a routing key");
    force(kc);
    kv.push_back(view_of(kc));
  }
  std::vector<int64_t> cnt;
  BufPtr perm = route_permutation(s, kv, d->nrows, parts, cnt);
  auto n = new_node(s, Kind::Source);
  n->names = t->node->names;
  n->types = t->node->types;
  auto e = std::make_shared<Data>();
  e->nrows = d->nrows;
  for (const ColPtr &c : d->cols) e->cols.push_back(gather_column(s, c, (const int64_t *)perm->p, d->nrows));
  s->sync();
  n->result = e;
  for (int p = 0; p < parts; ++p) counts[p] = cnt[p];
  *out = wrap(n);
  CAPF_API_END
}

capf_status capf_table_download_device(capf_table *t, const char *col, void *d_values,
                                       uint8_t *d_valid) {
  CAPF_API_BEGIN
  need(t, "table");
  need(col, "col");
  int i = t->node->col_index_or_throw(col);
  DataPtr d = materialize(t->node);
  Session *s = t->node->s;
  if (d->cols[i]->type == Type::List)
    illegal("column '" + std::string(col) + "' is a LIST: use capf_table_download_list");
  force(d->cols[i]);
  const ColPtr c = decode_column(s, d->cols[i]);
  const size_t w = type_width(c->type);
  if (d->nrows > 0) {
    if (c->type != Type::Null && d_values)
      HIP_CHECK(hipMemcpyAsync(d_values, c->data->p, w * d->nrows, hipMemcpyDeviceToDevice, s->stream));
    if (d_valid) {
      if (c->type == Type::Null)
        HIP_CHECK(hipMemsetAsync(d_valid, 0, d->nrows, s->stream));
      else if (c->valid)
        HIP_CHECK(hipMemcpyAsync(d_valid, c->valid->p, d->nrows, hipMemcpyDeviceToDevice, s->stream));
      else
        HIP_CHECK(hipMemsetAsync(d_valid, 1, d->nrows, s->stream));
    }
    s->sync();
  }
  CAPF_API_END
}

capf_status capf_table_column_range(capf_table *t, const char *col, int64_t *mn, int64_t *mx,
                                    int64_t *non_null) {
  CAPF_API_BEGIN
  need(t, "table");
  need(col, "col");
  need(mn, "min");
  need(mx, "max");
  need(non_null, "non_null");
  int i = t->node->col_index_or_throw(col);
  if (!is_int_payload(t->node->types[i]) && t->node->types[i] != Type::String)
    illegal("column range: INTEGER or STRING columns only");
  DataPtr d = materialize(t->node);
  force(d->cols[i]);
  const ColStats &st = column_stats(t->node->s, d->cols[i]);
  *mn = st.min;
  *mx = st.max;
  *non_null = st.non_null;
  CAPF_API_END
}

// lists: a LIST column's length field (4 or 8 bytes) is allowed
static void check_wire(Type t, int32_t width, int64_t base, bool lists = false) {
  const bool ok = t == Type::List     ? lists && (width == 4 || width == 8) && base == 0
                  : t == Type::Null   ? width == 0
                  : t == Type::Bool   ? width == 1
                  : t == Type::Float64 ? width == 8 && base == 0
                  : (is_int_payload(t) || t == Type::String) ? (width == 3 || width == 4 || (width == 8 && base == 0))
                                                           : false;
  if (!ok) illegal(std::string("packed rows: width ") + std::to_string(width) + " does not fit a " + type_name(t) +
                   " column");
}

capf_status capf_table_pack_rows(capf_table *t, int32_t ncols, const char *const *cols, const int32_t *width,
                                 const int64_t *base, const int32_t *nullable, int32_t *row_bytes, void *d_out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(row_bytes, "row_bytes");
  if (ncols < 0) illegal("negative column count");
  if (ncols > 0) {
    need(cols, "cols");
    need(width, "width");
    need(base, "base");
    need(nullable, "nullable");
  }
  DataPtr d = materialize(t->node);
  Session *s = t->node->s;
  std::vector<ColPtr> cs;
  for (int j = 0; j < ncols; ++j) {
    need(cols[j], "col");
    const int i = t->node->col_index_or_throw(cols[j]);
    check_wire(t->node->types[i], width[j], base[j], true);
    force(d->cols[i]);
    if (!nullable[j] && d->cols[i]->valid && d->cols[i]->type != Type::Null)
      illegal("packed rows: a column with NULLs needs its validity byte");
    cs.push_back(d->cols[i]);
  }
  int W = 0;
  pack_rows(s, cs, width, base, nullable, d->nrows, &W, d_out);
  *row_bytes = W;
  CAPF_API_END
}

capf_status capf_table_from_packed_rows(capf_session *cs, int32_t ncols, const char *const *names,
                                        const int32_t *types, const int32_t *width, const int64_t *base,
                                        const int32_t *nullable, const void *d_rows, int64_t nrows,
                                        capf_table **out) {
  CAPF_API_BEGIN
  need(cs, "session");
  need(out, "out");
  if (ncols < 0 || nrows < 0) illegal("negative size");
  if (ncols > 0) {
    need(names, "names");
    need(types, "types");
    need(width, "width");
    need(base, "base");
    need(nullable, "nullable");
  }
  Session *s = &cs->impl;
  int W = 0;
  std::vector<int> off(ncols), voff(ncols);
  std::vector<std::string> nm;
  for (int j = 0; j < ncols; ++j) {
    need(names[j], "name");
    nm.emplace_back(names[j]);
    check_wire((Type)types[j], width[j], base[j]);
    off[j] = W;
    W += width[j];
    voff[j] = nullable[j] ? W++ : -1;
  }
  check_unique_names(nm);
  if (nrows > 0 && W > 0) need(d_rows, "rows");
  auto n = new_node(s, Kind::Source);
  auto e = std::make_shared<Data>();
  e->nrows = nrows;
  for (int j = 0; j < ncols; ++j) {
    n->names.push_back(nm[j]);
    n->types.push_back((Type)types[j]);
    e->cols.push_back(unpack_column(s, d_rows, nrows, W, off[j], width[j], voff[j], base[j], (Type)types[j]));
  }
  s->sync();
  n->result = e;
  *out = wrap(n);
  CAPF_API_END
}

// ---- LIST columns on the wire (shuffle.hip "list elements")
static const ColPtr &list_col_or_throw(capf_table *t, const DataPtr &d, const char *col) {
  const int i = t->node->col_index_or_throw(col);
  if (t->node->types[i] != Type::List) illegal("column '" + std::string(col) + "' is not a LIST");
  force(d->cols[i]);
  return d->cols[i];
}

static void check_elem_type(int32_t et) {
  if (et < CAPF_TYPE_NULL || et > CAPF_TYPE_STRING) illegal("bad list element type");
}

capf_status capf_table_list_stats(capf_table *t, const char *col, int32_t *elem_type, int64_t *longest,
                                  int64_t *n_elems, int32_t *elem_nulls, int32_t *elem_enc, int64_t *mn,
                                  int64_t *mx, int64_t *non_null) {
  CAPF_API_BEGIN
  need(t, "table");
  need(col, "col");
  need(elem_type, "elem_type");
  need(longest, "longest");
  need(n_elems, "n_elems");
  need(elem_nulls, "elem_nulls");
  need(elem_enc, "elem_enc");
  need(mn, "min");
  need(mx, "max");
  need(non_null, "non_null");
  DataPtr d = materialize(t->node);
  Session *s = t->node->s;
  const ColPtr c = list_without_null_extents(s, list_col_or_throw(t, d, col));
  const ColPtr &ch = c->child;
  const std::vector<int64_t> o = list_offsets_at(s, c, {0, c->n});
  *elem_type = (int32_t)ch->type;
  *n_elems = o[1] - o[0];
  *longest = list_max_len(s, c);
  *elem_nulls = ch->type == Type::Null ? (*n_elems > 0) : (ch->valid != nullptr);
  *elem_enc = ch->enc;
  *mn = 0;
  *mx = -1;
  *non_null = 0;
  if ((ch->type == Type::Int64 || ch->type == Type::String) && ch->n > 0) {
    // (over the whole child: a superset of the listed elements only widens the range)
    const ColStats &st = column_stats(s, ch);
    *mn = st.min;
    *mx = st.max;
    *non_null = st.non_null;
  }
  CAPF_API_END
}

capf_status capf_table_pack_list_elems(capf_table *t, const char *col, int32_t nparts, const int64_t *row_counts,
                                       int32_t elem_type, int32_t width, int64_t base, int32_t elem_nullable,
                                       int64_t *elem_counts, int32_t *rec_bytes, void *d_out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(col, "col");
  need(row_counts, "row_counts");
  need(elem_counts, "elem_counts");
  need(rec_bytes, "rec_bytes");
  if (nparts <= 0 || nparts > (1 << 20)) illegal("parts out of range");
  check_elem_type(elem_type);
  check_wire((Type)elem_type, width, base);
  if (elem_type == CAPF_TYPE_NULL && elem_nullable) illegal("packed elements: NULL-typed elements carry no validity byte");
  DataPtr d = materialize(t->node);
  Session *s = t->node->s;
  // (elements of NULL lists, where any are stored, stay behind: the row's length field is 0)
  const ColPtr c = list_without_null_extents(s, list_col_or_throw(t, d, col));
  const ColPtr &ch = c->child;
  std::vector<int64_t> pos(nparts + 1, 0);
  for (int p = 0; p < nparts; ++p) {
    if (row_counts[p] < 0 || row_counts[p] > d->nrows - pos[p]) illegal("packed elements: row counts do not sum to the table's rows");
    pos[p + 1] = pos[p] + row_counts[p];
  }
  if (pos[nparts] != d->nrows) illegal("packed elements: row counts do not sum to the table's rows");
  if (ch->type != Type::Null && (int32_t)ch->type != elem_type)
    illegal(std::string("packed elements: the column holds LIST<") + type_name(ch->type) + ">, not LIST<" +
            type_name((Type)elem_type) + ">");
  const std::vector<int64_t> o = list_offsets_at(s, c, pos);
  const int64_t first = o[0], total = o[nparts] - o[0];
  for (int p = 0; p < nparts; ++p) {
    if (o[p + 1] < o[p]) fail(CAPF_ERR_INTERNAL, "list offsets decrease");
    elem_counts[p] = o[p + 1] - o[p];
  }
  if (first < 0 || first + total > ch->n) fail(CAPF_ERR_INTERNAL, "list offsets outside the element column");
  const bool child_nulls = ch->type == Type::Null ? (elem_type != CAPF_TYPE_NULL && total > 0) : ch->valid != nullptr;
  if (child_nulls && !elem_nullable) illegal("packed elements: a list with NULL elements needs its validity byte");
  const int rec = width + (elem_nullable ? 1 : 0);
  *rec_bytes = rec;
  if (d_out && total > 0 && rec > 0) {
    if ((uintptr_t)d_out % (rec == 8 ? 8 : 4))
      illegal("packed elements: the output buffer must be 4-byte aligned (8-byte for 8-byte records)");
    pack_list_elems(s, ch, first, total, width, base, elem_nullable != 0, d_out);
    s->sync();
  }
  CAPF_API_END
}

capf_status capf_table_from_packed_lists(capf_session *cs, int32_t ncols, const char *const *names,
                                         const int32_t *types, const int32_t *width, const int64_t *base,
                                         const int32_t *nullable, const void *d_rows, int64_t nrows, int32_t nlists,
                                         const int32_t *elem_types, const int32_t *elem_width,
                                         const int64_t *elem_base, const int32_t *elem_nullable,
                                         const void *const *d_elems, const int64_t *n_elems, capf_table **out) {
  CAPF_API_BEGIN
  need(cs, "session");
  need(out, "out");
  if (ncols < 0 || nrows < 0 || nlists < 0) illegal("negative size");
  if (ncols > 0) {
    need(names, "names");
    need(types, "types");
    need(width, "width");
    need(base, "base");
    need(nullable, "nullable");
  }
  if (nlists > 0) {
    need(elem_types, "elem_types");
    need(elem_width, "elem_width");
    need(elem_base, "elem_base");
    need(elem_nullable, "elem_nullable");
    need(d_elems, "elems");
    need(n_elems, "n_elems");
  }
  Session *s = &cs->impl;
  int W = 0, nl = 0;
  std::vector<int> off(ncols), voff(ncols);
  std::vector<std::string> nm;
  for (int j = 0; j < ncols; ++j) {
    need(names[j], "name");
    nm.emplace_back(names[j]);
    check_wire((Type)types[j], width[j], base[j], true);
    nl += types[j] == CAPF_TYPE_LIST;
    off[j] = W;
    W += width[j];
    voff[j] = nullable[j] ? W++ : -1;
  }
  if (nl != nlists) illegal("packed lists: one element stream per LIST column");
  for (int l = 0; l < nlists; ++l) {
    check_elem_type(elem_types[l]);
    check_wire((Type)elem_types[l], elem_width[l], elem_base[l]);
    if (elem_types[l] == CAPF_TYPE_NULL && elem_nullable[l])
      illegal("packed elements: NULL-typed elements carry no validity byte");
    if (n_elems[l] < 0) illegal("negative size");
    const int rec = elem_width[l] + (elem_nullable[l] ? 1 : 0);
    if (n_elems[l] > 0 && rec > 0) {
      need(d_elems[l], "elems");
      if ((uintptr_t)d_elems[l] % 4) illegal("packed elements: the stream must be 4-byte aligned");
    }
  }
  check_unique_names(nm);
  if (nrows > 0 && W > 0) need(d_rows, "rows");
  auto n = new_node(s, Kind::Source);
  auto e = std::make_shared<Data>();
  e->nrows = nrows;
  int l = 0;
  for (int j = 0; j < ncols; ++j) {
    n->names.push_back(nm[j]);
    n->types.push_back((Type)types[j]);
    if (types[j] == CAPF_TYPE_LIST) {
      e->cols.push_back(unpack_list_column(s, d_rows, nrows, W, off[j], width[j], voff[j], d_elems[l], n_elems[l],
                                           elem_width[l], elem_base[l], elem_nullable[l] != 0, (Type)elem_types[l]));
      ++l;
    } else {
      e->cols.push_back(unpack_column(s, d_rows, nrows, W, off[j], width[j], voff[j], base[j], (Type)types[j]));
    }
  }
  s->sync();
  n->result = e;
  *out = wrap(n);
  CAPF_API_END
}

capf_status capf_table_has_nulls(capf_table *t, const char *col, int32_t *has) {
  CAPF_API_BEGIN
  need(t, "table");
  need(col, "col");
  need(has, "has");
  int i = t->node->col_index_or_throw(col);
  DataPtr d = materialize(t->node);
  force(d->cols[i]);
  *has = d->cols[i]->type == Type::Null ? (d->nrows > 0) : (d->cols[i]->valid != nullptr);
  CAPF_API_END
}

capf_status capf_table_column_encoding(capf_table *t, const char *col, int32_t *enc,
                                       int64_t *base) {
  CAPF_API_BEGIN
  need(t, "table");
  need(col, "col");
  int i = t->node->col_index_or_throw(col);
  DataPtr d = materialize(t->node);
  const ColPtr &c = d->cols[i];
  force(c);
  if (enc) *enc = c->enc;
  if (base) *base = c->base;
  CAPF_API_END
}

capf_status capf_table_retain(capf_table *t) {
  CAPF_API_BEGIN
  need(t, "table");
  // handles are values: retaining creates no new handle in this ABI; use
  // capf_table_cache to obtain a second owning handle.
  CAPF_API_END
}

capf_status capf_table_release(capf_table *t) {
  CAPF_API_BEGIN
  delete t;
  CAPF_API_END
}

capf_status capf_table_num_columns(capf_table *t, int32_t *n) {
  CAPF_API_BEGIN
  need(t, "table");
  need(n, "n");
  *n = (int32_t)t->node->names.size();
  CAPF_API_END
}

capf_status capf_table_column_name(capf_table *t, int32_t i, const char **name) {
  CAPF_API_BEGIN
  need(t, "table");
  need(name, "name");
  if (i < 0 || i >= (int32_t)t->node->names.size()) illegal("column index out of range");
  *name = t->node->names[i].c_str();
  CAPF_API_END
}

capf_status capf_table_columns(capf_table *t, const char **joined, int64_t *bytes, int32_t *n) {
  CAPF_API_BEGIN
  need(t, "table");
  need(joined, "joined");
  need(bytes, "bytes");
  need(n, "n");
  Node &nd = *t->node;
  {
    std::lock_guard<std::mutex> lk(nd.mu);
    if (nd.joined_names.empty() && !nd.names.empty()) {
      for (const auto &c : nd.names) {
        nd.joined_names += c;
        nd.joined_names.push_back('\0');
      }
    }
  }
  *joined = nd.joined_names.data();
  *bytes = (int64_t)nd.joined_names.size();
  *n = (int32_t)nd.names.size();
  CAPF_API_END
}

capf_status capf_table_column_type(capf_table *t, const char *col, int32_t *type) {
  CAPF_API_BEGIN
  need(t, "table");
  need(col, "col");
  need(type, "type");
  *type = (int32_t)t->node->types[t->node->col_index_or_throw(col)];
  CAPF_API_END
}

capf_status capf_table_size(capf_table *t, int64_t *n) {
  CAPF_API_BEGIN
  need(t, "table");
  need(n, "n");
  *n = node_size(t->node);
  CAPF_API_END
}

capf_status capf_table_count_async(capf_table *t, int64_t *d_count) {
  CAPF_API_BEGIN
  need(t, "table");
  need(d_count, "d_count");
  NodePtr n = t->node;
  Session *s = n->s;
  // group(∅, count(*)) → the count of its input (also under projections of
  // its one column: RETURN count(*) AS c); anything else → its row count
  NodePtr g = n;
  while (g->kind == Kind::Select && !g->names.empty()) g = g->kids[0];
  if (g->kind == Kind::Group && g->key_index.empty() && g->aggs.size() == 1 &&
      g->aggs[0].kind == CAPF_AGG_COUNT_STAR)
    n = g->kids[0];
  struct Reset {
    Session *s;
    ~Reset() { s->async_out = nullptr; }
  } reset{s};
  s->async_out = d_count;
  int64_t unused = 0;
  if (!try_fused_count(n, &unused)) {
    // not a fused shape (or already materialised): count on the host path
    s->async_out = nullptr;
    s->h_scalars[0] = node_size(n);
    HIP_CHECK(hipMemcpyAsync(d_count, s->h_scalars, 8, hipMemcpyHostToDevice, s->stream));
    s->sync();  // the pinned slot is reused by the next call
  }
  CAPF_API_END
}

capf_status capf_table_download(capf_table *t, const char *col, void *values_out,
                                uint8_t *valid_out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(col, "col");
  int i = t->node->col_index_or_throw(col);
  DataPtr d = materialize(t->node);
  Session *s = t->node->s;
  const ColPtr &hc = d->cols[i];
  if (!hc->host_i64.empty() && (int64_t)hc->host_i64.size() == d->nrows && !hc->valid) {
    if (values_out) memcpy(values_out, hc->host_i64.data(), 8 * d->nrows);
    if (valid_out) memset(valid_out, 1, d->nrows);
    return CAPF_OK;
  }
  if (d->cols[i]->type == Type::List)
    illegal("column '" + std::string(col) + "' is a LIST: use capf_table_download_list");
  const ColPtr c = decode_column(s, d->cols[i]);
  size_t w = type_width(c->type);
  if (d->nrows > 0) {
    if (c->type != Type::Null && values_out)
      HIP_CHECK(hipMemcpyAsync(values_out, c->data->p, w * d->nrows, hipMemcpyDeviceToHost, s->stream));
    if (valid_out) {
      if (c->type == Type::Null)
        memset(valid_out, 0, d->nrows);
      else if (c->valid)
        HIP_CHECK(hipMemcpyAsync(valid_out, c->valid->p, d->nrows, hipMemcpyDeviceToHost, s->stream));
      else
        memset(valid_out, 1, d->nrows);
    }
    s->sync();
  }
  CAPF_API_END
}

// Element type of LIST column i of plan node n, read off the plan without
// running it (UNWIND and list_info used to materialise the child
// while the plan was being built).  False when the plan does not say — a
// computed list expression or a source without data — and the caller then
// materialises.  Mirrors what materialize_impl produces column by column.
static bool static_list_elem(const NodePtr &n, int i, Type &et, int depth = 0) {
  if (depth > 256 || i < 0 || i >= (int)n->types.size()) return false;
  if (n->types[(size_t)i] == Type::Null) {  // a NULL column concatenated with a list adds no elements
    et = Type::Null;
    return true;
  }
  if (n->types[(size_t)i] != Type::List) return false;
  {
    std::lock_guard<std::mutex> g(n->mu);
    if (n->result) {
      const ColPtr &c = n->result->cols[(size_t)i];
      et = c->child ? c->child->type : Type::Null;
      return true;
    }
  }
  const int nk = n->kids.empty() ? 0 : (int)n->kids[0]->names.size();
  switch (n->kind) {
    case Kind::Source: return false;
    case Kind::Select: return static_list_elem(n->kids[0], n->sel_index[(size_t)i], et, depth + 1);
    case Kind::Filter:
    case Kind::Distinct:
    case Kind::OrderBy:
    case Kind::Skip:
    case Kind::Limit: return static_list_elem(n->kids[0], i, et, depth + 1);
    case Kind::Join:
      return i < nk ? static_list_elem(n->kids[0], i, et, depth + 1)
                    : static_list_elem(n->kids[1], i - nk, et, depth + 1);
    case Kind::Union: {  // concat_lists: the non-NULL side's element type, equal types otherwise
      Type a, b;
      if (!static_list_elem(n->kids[0], i, a, depth + 1) ||
          !static_list_elem(n->kids[1], n->kids[1]->col_index(n->names[(size_t)i]), b, depth + 1))
        return false;
      if (a != Type::Null && b != Type::Null && a != b) return false;  // the union reports the mismatch
      et = a == Type::Null ? b : a;
      return true;
    }
    case Kind::Group: {
      const int nkey = (int)n->key_index.size();
      if (i < nkey) return static_list_elem(n->kids[0], n->key_index[(size_t)i], et, depth + 1);
      const AggSpec &a = n->aggs[(size_t)(i - nkey)];
      if (a.kind != CAPF_AGG_COLLECT) return false;
      et = infer_type(a.arg, n->kids[0]->names, n->kids[0]->types);  // collect_lists: the argument's type
      return true;
    }
    case Kind::NameList:
      if (i < nk) return static_list_elem(n->kids[0], i, et, depth + 1);
      et = Type::String;
      return true;
    case Kind::ListColumns:
    case Kind::ListFn:
    case Kind::ListLambda:
    case Kind::StrSplit:
      if (i < nk) return static_list_elem(n->kids[0], i, et, depth + 1);
      et = n->list_elem;
      return true;
    case Kind::Explode: return i < nk && static_list_elem(n->kids[0], i, et, depth + 1);
    case Kind::WithColumns:
      for (int t : n->target_index)
        if (t == i) return false;  // a computed list
      return i < nk && static_list_elem(n->kids[0], i, et, depth + 1);
  }
  return false;
}

capf_status capf_table_list_info(capf_table *t, const char *col, int32_t *elem_type,
                                 int64_t *n_values) {
  CAPF_API_BEGIN
  need(t, "table");
  need(col, "col");
  int i = t->node->col_index_or_throw(col);
  if (t->node->types[i] != Type::List) illegal("column '" + std::string(col) + "' is not a LIST");
  Type st;
  if (!n_values && elem_type && static_list_elem(t->node, i, st)) {  // the type alone: no evaluation
    *elem_type = (int32_t)st;
    return CAPF_OK;
  }
  DataPtr d = materialize(t->node);
  const ColPtr &c = d->cols[i];
  Session *s = t->node->s;
  int64_t total = 0;
  if (c->n > 0) {
    HIP_CHECK(hipMemcpyAsync(&total, (const int64_t *)c->data->p + c->n, 8, hipMemcpyDeviceToHost,
                             s->stream));
    s->sync();
  }
  if (elem_type) *elem_type = (int32_t)c->child->type;
  if (n_values) *n_values = total;
  CAPF_API_END
}

capf_status capf_table_download_list(capf_table *t, const char *col, int64_t *offsets_out,
                                     void *values_out, uint8_t *valid_out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(col, "col");
  int i = t->node->col_index_or_throw(col);
  if (t->node->types[i] != Type::List) illegal("column '" + std::string(col) + "' is not a LIST");
  DataPtr d = materialize(t->node);
  const ColPtr &c = d->cols[i];
  Session *s = t->node->s;
  const int64_t n = c->n;
  int64_t total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, (const int64_t *)c->data->p + n, 8, hipMemcpyDeviceToHost,
                           s->stream));
  s->sync();
  if (offsets_out)
    HIP_CHECK(hipMemcpyAsync(offsets_out, c->data->p, 8 * (n + 1), hipMemcpyDeviceToHost, s->stream));
  if (values_out && total > 0 && c->child->type != Type::Null) {
    // (a list that came over the exchange keeps a FOR24 / FOR32 element column)
    const ColPtr ch = decode_column(s, c->child);
    HIP_CHECK(hipMemcpyAsync(values_out, ch->data->p, type_width(ch->type) * total, hipMemcpyDeviceToHost,
                             s->stream));
    s->sync();  // ch may be a temporary
  }
  if (valid_out && n > 0) {
    if (c->valid)
      HIP_CHECK(hipMemcpyAsync(valid_out, c->valid->p, n, hipMemcpyDeviceToHost, s->stream));
    else
      memset(valid_out, 1, n);
  }
  s->sync();
  CAPF_API_END
}

capf_status capf_table_download_list_nulls(capf_table *t, const char *col, uint8_t *elem_valid_out,
                                           int32_t *has_nulls) {
  CAPF_API_BEGIN
  need(t, "table");
  need(col, "col");
  need(has_nulls, "has_nulls");
  int i = t->node->col_index_or_throw(col);
  if (t->node->types[i] != Type::List) illegal("column '" + std::string(col) + "' is not a LIST");
  DataPtr d = materialize(t->node);
  const ColPtr &c = d->cols[i];
  Session *s = t->node->s;
  const ColPtr &ch = c->child;
  *has_nulls = ch->type == Type::Null || ch->valid ? 1 : 0;
  if (*has_nulls && elem_valid_out && ch->n > 0) {
    if (ch->type == Type::Null) {
      memset(elem_valid_out, 0, (size_t)ch->n);
    } else {
      HIP_CHECK(hipMemcpyAsync(elem_valid_out, ch->valid->p, (size_t)ch->n, hipMemcpyDeviceToHost, s->stream));
      s->sync();
    }
  }
  CAPF_API_END
}

capf_status capf_table_device_column(capf_table *t, const char *col, void **values,
                                     uint8_t **valid, int64_t *nrows) {
  CAPF_API_BEGIN
  need(t, "table");
  need(col, "col");
  int i = t->node->col_index_or_throw(col);
  DataPtr d = materialize(t->node);
  force(d->cols[i]);
  if (d->cols[i]->enc != ENC_PLAIN) {
    // the handle's storage becomes the plain column (same values), so the
    // returned pointer lives as long as the table
    Session *s = t->node->s;
    std::lock_guard<std::mutex> g(t->node->mu);
    d->cols[i] = decode_column(s, d->cols[i]);
    s->sync();
  }
  const ColPtr &c = d->cols[i];
  if (values) *values = c->data ? c->data->p : nullptr;
  if (valid) *valid = c->valid ? (uint8_t *)c->valid->p : nullptr;
  if (nrows) *nrows = d->nrows;
  CAPF_API_END
}

capf_status capf_table_materialize(capf_table *t) {
  CAPF_API_BEGIN
  need(t, "table");
  DataPtr d = materialize(t->node);
  for (const ColPtr &c : d->cols) force(c);  // every result column lands in HBM
  CAPF_API_END
}

capf_status capf_table_cache(capf_table *t, capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(out, "out");
  *out = wrap(t->node);  // Table.cache default: identity (Table.scala:52)
  CAPF_API_END
}

capf_status capf_table_select(capf_table *t, int32_t n, const char *const *cols,
                              const char *const *aliases, capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(out, "out");
  const NodePtr &c = t->node;
  auto nn = new_node(c->s, Kind::Select);
  nn->kids.push_back(c);
  for (int i = 0; i < n; ++i) {
    int idx = c->col_index_or_throw(cols[i]);
    nn->sel_index.push_back(idx);
    nn->names.emplace_back(aliases && aliases[i] ? aliases[i] : cols[i]);
    nn->types.push_back(c->types[idx]);
  }
  check_unique_names(nn->names);
  *out = wrap(nn);
  CAPF_API_END
}

capf_status capf_table_drop(capf_table *t, int32_t n, const char *const *cols, capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(out, "out");
  const NodePtr &c = t->node;
  // FlinkTable.drop = select(physicalColumns diff cols) (FlinkTable.scala:100-103)
  auto nn = new_node(c->s, Kind::Select);
  nn->kids.push_back(c);
  for (size_t i = 0; i < c->names.size(); ++i) {
    bool dropped = false;
    for (int k = 0; k < n; ++k) dropped |= c->names[i] == cols[k];
    if (dropped) continue;
    nn->sel_index.push_back((int)i);
    nn->names.push_back(c->names[i]);
    nn->types.push_back(c->types[i]);
  }
  *out = wrap(nn);
  CAPF_API_END
}

capf_status capf_table_filter(capf_table *t, const capf_expr *pred, capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(out, "out");
  const NodePtr &c = t->node;
  Program p = Program::from_c(pred);
  Type ty = infer_type(p, c->names, c->types);
  if (ty != Type::Bool && ty != Type::Null) illegal("filter predicate is not boolean");
  auto nn = new_node(c->s, Kind::Filter);
  nn->kids.push_back(c);
  nn->pred = std::move(p);
  nn->names = c->names;
  nn->types = c->types;
  *out = wrap(nn);
  CAPF_API_END
}

capf_status capf_table_join(capf_table *l, capf_table *r, int32_t join_type, int32_t npairs,
                            const char *const *lcols, const char *const *rcols,
                            capf_table **out) {
  CAPF_API_BEGIN
  need(l, "left");
  need(r, "right");
  need(out, "out");
  const NodePtr &a = l->node;
  const NodePtr &b = r->node;
  // FlinkTable.join asserts disjoint columns (FlinkTable.scala:173-174)
  for (auto &x : a->names)
    for (auto &y : b->names)
      if (x == y) illegal("overlapping columns: " + x);
  if (join_type < CAPF_JOIN_INNER || join_type > CAPF_JOIN_CROSS) illegal("bad join type");
  auto nn = new_node(a->s, Kind::Join);
  nn->kids = {a, b};
  nn->join_type = join_type;
  if (join_type != CAPF_JOIN_CROSS) {
    for (int i = 0; i < npairs; ++i) {
      int li = a->col_index_or_throw(lcols[i]);
      int ri = b->col_index_or_throw(rcols[i]);
      Type lt = a->types[li], rt = b->types[ri];
      if (lt != rt && lt != Type::Null && rt != Type::Null &&
          !(is_numeric(lt) && is_numeric(rt)))
        illegal(std::string("join on incompatible types ") + type_name(lt) + " / " + type_name(rt));
      if (lt != rt && lt != Type::Null && rt != Type::Null)
        not_impl("join between INTEGER and FLOAT columns");
      nn->join_keys.emplace_back(li, ri);
    }
  }
  nn->names = a->names;
  nn->names.insert(nn->names.end(), b->names.begin(), b->names.end());
  nn->types = a->types;
  nn->types.insert(nn->types.end(), b->types.begin(), b->types.end());
  *out = wrap(nn);
  CAPF_API_END
}

capf_status capf_table_union_all(capf_table *l, capf_table *r, capf_table **out) {
  CAPF_API_BEGIN
  need(l, "left");
  need(r, "right");
  need(out, "out");
  const NodePtr &a = l->node;
  const NodePtr &b = r->node;
  if (a->names.size() != b->names.size()) illegal("unionAll: column sets differ");
  auto nn = new_node(a->s, Kind::Union);
  nn->kids = {a, b};
  nn->names = a->names;
  for (size_t i = 0; i < a->names.size(); ++i) {
    int j = b->col_index(a->names[i]);
    if (j < 0) illegal("unionAll: right side lacks column '" + a->names[i] + "'");
    Type x = a->types[i], y = b->types[j];
    // Equal column types for union all, differing nullability OK
    // (FlinkTable.scala:152-169)
    if (x != y && x != Type::Null && y != Type::Null)
      illegal(std::string("Equal column types for union all: ") + a->names[i] + " " +
              type_name(x) + " vs " + type_name(y));
    nn->types.push_back(x == Type::Null ? y : x);
  }
  *out = wrap(nn);
  CAPF_API_END
}

capf_status capf_table_order_by(capf_table *t, int32_t n, const capf_expr *keys,
                                const int32_t *descending, capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(out, "out");
  const NodePtr &c = t->node;
  auto nn = new_node(c->s, Kind::OrderBy);
  nn->kids.push_back(c);
  for (int i = 0; i < n; ++i) {
    Program p = Program::from_c(&keys[i]);
    Type ty = infer_type(p, c->names, c->types);
    if (ty == Type::String) p.code.push_back(Instr{OP_STR_RANK, 0, 0, 0.0});  // sort on the ranks
    nn->exprs.push_back(std::move(p));
    nn->desc.push_back(descending ? descending[i] : 0);
  }
  nn->names = c->names;
  nn->types = c->types;
  *out = wrap(nn);
  CAPF_API_END
}

static capf_status skip_limit(capf_table *t, int64_t n, Kind k, capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(out, "out");
  if (n < 0) illegal("negative skip/limit");
  const NodePtr &c = t->node;
  auto nn = new_node(c->s, k);
  nn->kids.push_back(c);
  nn->count = n;
  nn->names = c->names;
  nn->types = c->types;
  *out = wrap(nn);
  CAPF_API_END
}

capf_status capf_table_skip(capf_table *t, int64_t n, capf_table **out) {
  return skip_limit(t, n, Kind::Skip, out);
}
capf_status capf_table_limit(capf_table *t, int64_t n, capf_table **out) {
  return skip_limit(t, n, Kind::Limit, out);
}

capf_status capf_table_distinct_cols(capf_table *t, int32_t n, const char *const *cols,
                                     capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(out, "out");
  const NodePtr &c = t->node;
  auto nn = new_node(c->s, Kind::Distinct);
  nn->kids.push_back(c);
  for (int i = 0; i < n; ++i) nn->key_index.push_back(c->col_index_or_throw(cols[i]));
  nn->names = c->names;
  nn->types = c->types;
  *out = wrap(nn);
  CAPF_API_END
}

capf_status capf_table_distinct(capf_table *t, capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  std::vector<const char *> cols;
  for (auto &nm : t->node->names) cols.push_back(nm.c_str());
  capf_status st = capf_table_distinct_cols(t, (int32_t)cols.size(), cols.data(), out);
  if (st != CAPF_OK) return st;
  CAPF_API_END
}

capf_status capf_table_group(capf_table *t, int32_t n_by, const char *const *by_cols,
                             int32_t n_aggs, const int32_t *agg_kinds,
                             const capf_expr *agg_args, const int32_t *agg_distinct,
                             const char *const *agg_names, capf_table **out) {
  return capf_table_group_ex(t, n_by, by_cols, n_aggs, agg_kinds, agg_args, agg_distinct, nullptr, agg_names,
                             out);
}

capf_status capf_table_group_ex(capf_table *t, int32_t n_by, const char *const *by_cols,
                                int32_t n_aggs, const int32_t *agg_kinds,
                                const capf_expr *agg_args, const int32_t *agg_distinct,
                                const double *agg_params, const char *const *agg_names,
                                capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(out, "out");
  const NodePtr &c = t->node;
  auto nn = new_node(c->s, Kind::Group);
  nn->kids.push_back(c);
  for (int i = 0; i < n_by; ++i) {
    int idx = c->col_index_or_throw(by_cols[i]);
    nn->key_index.push_back(idx);
    nn->names.push_back(c->names[idx]);
    nn->types.push_back(c->types[idx]);
  }
  for (int i = 0; i < n_aggs; ++i) {
    AggSpec a;
    a.kind = agg_kinds[i];
    a.distinct = agg_distinct && agg_distinct[i];
    a.name = agg_names[i];
    if (a.kind < CAPF_AGG_COUNT_STAR || a.kind > CAPF_AGG_PERCENTILE_DISC) illegal("bad aggregator kind");
    if (a.kind == CAPF_AGG_PERCENTILE_CONT || a.kind == CAPF_AGG_PERCENTILE_DISC) {
      if (!agg_params) illegal("percentile aggregator without its fraction (capf_table_group_ex)");
      a.param = agg_params[i];
      // Neo4j / openCypher: the percentile must lie in [0, 1]
      if (!(a.param >= 0.0 && a.param <= 1.0)) illegal("percentile must be between 0.0 and 1.0");
    }
    if (a.kind == CAPF_AGG_COUNT_STAR) {
      a.out_type = Type::Int64;
    } else {
      a.arg = Program::from_c(&agg_args[i]);
      Type at = infer_type(a.arg, c->names, c->types);
      if (at == Type::List) not_impl("aggregation of list values");
      if (is_temporal(at)) {  // ordered and countable, nothing else (no duration type to hold a sum)
        if (a.kind == CAPF_AGG_COLLECT) not_impl(std::string("collect of ") + type_name(at) + " values");
        if (a.kind != CAPF_AGG_COUNT && a.kind != CAPF_AGG_MIN && a.kind != CAPF_AGG_MAX)
          illegal(std::string("sum / avg / stDev / percentile of ") + type_name(at) + " values");
      }
      switch (a.kind) {
        case CAPF_AGG_COUNT: a.out_type = Type::Int64; break;
        case CAPF_AGG_SUM:
        case CAPF_AGG_AVG:
          if (at == Type::String || at == Type::Bool) not_impl("sum/avg of non-numeric");
          // avg is a FLOAT also over INTEGER values: the reference's acceptance
          // tests expect CypherFloat(49.666666666666664) for avg(42, 23, 84) and
          // 32.5 for avg(42, 23) (flink-cypher-testing/.../AggregationTests.scala:
          // 852, 876, 921); avg(2, 4, 6) = 4.0 equals their CypherMap("res" -> 4)
          // (:40-57) under Scala's numeric Map equality.  See DESIGN.md.
          a.out_type = a.kind == CAPF_AGG_AVG && at == Type::Int64 ? Type::Float64 : at;
          break;
        case CAPF_AGG_MIN:
        case CAPF_AGG_MAX:
          if (at == Type::String) {  // String.compareTo order: aggregate the ranks
            a.arg.code.push_back(Instr{OP_STR_RANK, 0, 0, 0.0});
            a.rank_to_code = true;
          }
          a.out_type = at;
          break;
        case CAPF_AGG_COLLECT: a.out_type = Type::List; break;
        case CAPF_AGG_STDEV:
        case CAPF_AGG_STDEV_POP:
        case CAPF_AGG_PERCENTILE_CONT:
          if (at != Type::Null && !is_numeric(at)) not_impl("stDev / percentile of non-numeric values");
          a.out_type = Type::Float64;
          break;
        case CAPF_AGG_PERCENTILE_DISC:
          if (at != Type::Null && !is_numeric(at)) not_impl("percentileDisc of non-numeric values");
          a.out_type = at == Type::Null ? Type::Float64 : at;
          break;
      }
    }
    nn->names.push_back(a.name);
    nn->types.push_back(a.out_type);
    nn->aggs.push_back(std::move(a));
  }
  check_unique_names(nn->names);
  *out = wrap(nn);
  CAPF_API_END
}

capf_status capf_table_with_columns(capf_table *t, int32_t n, const capf_expr *exprs,
                                    const char *const *names, capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(out, "out");
  const NodePtr &c = t->node;
  auto nn = new_node(c->s, Kind::WithColumns);
  nn->kids.push_back(c);
  nn->names = c->names;
  nn->types = c->types;
  for (int i = 0; i < n; ++i) {
    Program p = Program::from_c(&exprs[i]);
    Type ty = infer_type(p, c->names, c->types);
    int idx = nn->col_index(names[i]);
    if (idx < 0) {
      nn->names.emplace_back(names[i]);
      nn->types.push_back(ty);
      idx = (int)nn->names.size() - 1;
    } else {
      nn->types[idx] = ty;
    }
    nn->exprs.push_back(std::move(p));
    nn->target_index.push_back(idx);
  }
  *out = wrap(nn);
  CAPF_API_END
}

capf_status capf_table_explode_values(capf_table *t, const char *name, int32_t type, int64_t n,
                                      const void *values, const uint8_t *valid, capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(name, "name");
  need(out, "out");
  if (n < 0) illegal("negative list length");
  if (type < CAPF_TYPE_NULL || (type > CAPF_TYPE_STRING && !is_temporal((Type)type))) illegal("bad list element type");
  const NodePtr &c = t->node;
  if (c->col_index(name) >= 0) illegal(std::string("column '") + name + "' already exists");
  Type ty = (Type)type;
  if (n > 0 && ty != Type::Null && !values) illegal("list values missing");
  auto nn = new_node(c->s, Kind::Explode);
  nn->kids.push_back(c);
  nn->names = c->names;
  nn->types = c->types;
  nn->names.emplace_back(name);
  nn->types.push_back(ty);
  Session *s = c->s;
  ColPtr v = make_column(s, ty, n, valid != nullptr);
  if (n > 0 && ty != Type::Null)
    HIP_CHECK(hipMemcpyAsync(v->data->p, values, type_width(ty) * n, hipMemcpyHostToDevice, s->stream));
  if (n > 0 && valid) HIP_CHECK(hipMemcpyAsync(v->valid->p, valid, n, hipMemcpyHostToDevice, s->stream));
  s->sync();  // pageable host sources
  nn->explode_values = v;
  *out = wrap(nn);
  CAPF_API_END
}

// capf_table_add_list / _nulls: elem_valid (nv bytes) marks NULL elements; a
// NULL-typed element column holds only its count
static void add_list_column(capf_table *t, const char *name, int32_t elem_type, const int64_t *offsets,
                            const void *values, const uint8_t *valid, const uint8_t *elem_valid, bool null_elems,
                            capf_table **out) {
  need(t, "table");
  need(name, "name");
  need(offsets, "offsets");
  need(out, "out");
  if (elem_type < (null_elems ? CAPF_TYPE_NULL : CAPF_TYPE_INT64) || elem_type > CAPF_TYPE_STRING)
    illegal("bad list element type");
  const NodePtr &c = t->node;
  if (c->col_index(name) >= 0) illegal(std::string("column '") + name + "' already exists");
  DataPtr d = materialize(c);
  Session *s = c->s;
  const int64_t n = d->nrows;
  if (offsets[0] != 0) illegal("list offsets must start at 0");
  for (int64_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) illegal("list offsets must not decrease");
  const int64_t nv = offsets[n];
  const Type et = (Type)elem_type;
  if (nv > 0 && !values && et != Type::Null) illegal("list values missing");
  auto child = et == Type::Null ? null_column(s, Type::Null, nv) : make_column(s, et, nv, elem_valid != nullptr);
  if (nv > 0 && et != Type::Null) {
    HIP_CHECK(hipMemcpyAsync(child->data->p, values, type_width(et) * nv, hipMemcpyHostToDevice, s->stream));
    if (elem_valid) HIP_CHECK(hipMemcpyAsync(child->valid->p, elem_valid, (size_t)nv, hipMemcpyHostToDevice, s->stream));
  }
  auto lc = std::make_shared<Column>();
  lc->type = Type::List;
  lc->n = n;
  lc->child = child;
  lc->data = s->alloc(8 * (size_t)(n + 1));
  HIP_CHECK(hipMemcpyAsync(lc->data->p, offsets, 8 * (size_t)(n + 1), hipMemcpyHostToDevice, s->stream));
  if (valid && n > 0) {
    lc->valid = s->alloc((size_t)n);
    HIP_CHECK(hipMemcpyAsync(lc->valid->p, valid, (size_t)n, hipMemcpyHostToDevice, s->stream));
  }
  s->sync();  // pageable host sources
  auto nn = new_node(s, Kind::Source);
  nn->names = c->names;
  nn->types = c->types;
  nn->names.emplace_back(name);
  nn->types.push_back(Type::List);
  auto e = std::make_shared<Data>();
  e->nrows = n;
  e->cols = d->cols;
  e->cols.push_back(lc);
  nn->result = e;
  *out = wrap(nn);
}

capf_status capf_table_add_list(capf_table *t, const char *name, int32_t elem_type, const int64_t *offsets,
                                const void *values, const uint8_t *valid, capf_table **out) {
  CAPF_API_BEGIN
  add_list_column(t, name, elem_type, offsets, values, valid, nullptr, false, out);
  CAPF_API_END
}

capf_status capf_table_add_list_nulls(capf_table *t, const char *name, int32_t elem_type, const int64_t *offsets,
                                      const void *values, const uint8_t *valid, const uint8_t *elem_valid,
                                      capf_table **out) {
  CAPF_API_BEGIN
  add_list_column(t, name, elem_type, offsets, values, valid, elem_valid, true, out);
  CAPF_API_END
}

capf_status capf_table_name_list(capf_table *t, int32_t n, const char *const *cols, const int32_t *kinds,
                                 const int64_t *codes, const char *name, capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(name, "name");
  need(out, "out");
  if (n < 0 || (n > 0 && (!cols || !kinds || !codes))) illegal("bad name list");
  const NodePtr &c = t->node;
  if (c->col_index(name) >= 0) illegal(std::string("column '") + name + "' already exists");
  auto nn = new_node(c->s, Kind::NameList);
  nn->kids.push_back(c);
  nn->names = c->names;
  nn->types = c->types;
  for (int32_t j = 0; j < n; ++j) {
    nn->name_cols.push_back(c->col_index_or_throw(cols[j]));
    if (kinds[j] != 0 && kinds[j] != 1) illegal("bad name list kind");
    nn->name_kinds.push_back(kinds[j]);
    nn->name_codes.push_back(codes[j]);
  }
  nn->names.emplace_back(name);
  nn->types.push_back(Type::List);
  *out = wrap(nn);
  CAPF_API_END
}

capf_status capf_table_list_columns(capf_table *t, int32_t n, const char *const *cols, const char *name,
                                    capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(name, "name");
  need(out, "out");
  if (n < 0 || (n > 0 && !cols)) illegal("bad list element columns");
  const NodePtr &c = t->node;
  if (c->col_index(name) >= 0) illegal(std::string("column '") + name + "' already exists");
  auto nn = new_node(c->s, Kind::ListColumns);
  nn->kids.push_back(c);
  nn->names = c->names;
  nn->types = c->types;
  Type et = Type::Null;
  for (int32_t j = 0; j < n; ++j) {
    const int idx = c->col_index_or_throw(cols[j]);
    const Type ct = c->types[(size_t)idx];
    if (ct == Type::List) not_impl("nested lists");
    if (is_temporal(ct)) not_impl(std::string("a list of ") + type_name(ct) + " elements");
    // a NULL-typed item is a NULL element: the element type is that of the
    // other items (Type::Null when there are none)
    if (ct == Type::Null || et == Type::Null || et == ct) et = ct == Type::Null ? et : ct;
    else if ((et == Type::Int64 || et == Type::Float64) && (ct == Type::Int64 || ct == Type::Float64))
      et = Type::Float64;  // INTEGER and FLOAT elements widen together
    else
      not_impl(std::string("a list of mixed element types ") + type_name(et) + " / " + type_name(ct));
    nn->name_cols.push_back(idx);
  }
  nn->list_elem = et;
  nn->names.emplace_back(name);
  nn->types.push_back(Type::List);
  *out = wrap(nn);
  CAPF_API_END
}

// Element type of LIST column i of node c: off the plan, else by evaluating it.
static Type list_elem_of(const NodePtr &c, int i) {
  Type et;
  if (static_list_elem(c, i, et)) return et;
  DataPtr d = materialize(c);
  const ColPtr &lc = d->cols[(size_t)i];
  return lc->child ? lc->child->type : Type::Null;
}

capf_status capf_table_list_fn(capf_table *t, int32_t fn, int32_t nargs, const char *const *args,
                               const char *name, capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(name, "name");
  need(out, "out");
  static const int32_t want[4] = {3, 1, 2, 3};
  if (fn < CAPF_LIST_FN_SLICE || fn > CAPF_LIST_FN_RANGE) illegal("unknown list function");
  if (nargs != want[fn] || !args) illegal("wrong number of list function arguments");
  const NodePtr &c = t->node;
  if (c->col_index(name) >= 0) illegal(std::string("column '") + name + "' already exists");
  auto nn = new_node(c->s, Kind::ListFn);
  nn->kids.push_back(c);
  nn->names = c->names;
  nn->types = c->types;
  nn->list_fn = fn;
  for (int32_t j = 0; j < nargs; ++j) {
    need(args[j], "args[j]");
    const bool optional = (fn == CAPF_LIST_FN_SLICE && j > 0) || (fn == CAPF_LIST_FN_RANGE && j == 2);
    if (!args[j][0] && !optional) illegal("a list function argument is missing");
    nn->name_cols.push_back(args[j][0] ? c->col_index_or_throw(args[j]) : -1);
  }
  auto type_of = [&](int j) { return c->types[(size_t)nn->name_cols[(size_t)j]]; };
  auto integer_arg = [&](int j, const char *what) {
    if (nn->name_cols[(size_t)j] >= 0 && type_of(j) != Type::Int64 && type_of(j) != Type::Null)
      illegal(std::string(what) + " must be an INTEGER, got " + type_name(type_of(j)));
  };
  Type out_type = Type::List;
  if (fn == CAPF_LIST_FN_RANGE) {
    for (int j = 0; j < 3; ++j) integer_arg(j, "a range() argument");
    nn->list_elem = Type::Int64;
  } else if (fn == CAPF_LIST_FN_CONCAT) {
    if (type_of(0) != Type::List && type_of(1) != Type::List) illegal("list concatenation without a list side");
    Type et = Type::Null;
    for (int j = 0; j < 2; ++j) {
      const Type ct = type_of(j) == Type::List ? list_elem_of(c, nn->name_cols[(size_t)j]) : type_of(j);
      if (ct == Type::List) not_impl("nested lists");
      if (is_temporal(ct)) not_impl(std::string("a list of ") + type_name(ct) + " elements");
      if (ct == Type::Null || et == Type::Null || et == ct) et = ct == Type::Null ? et : ct;
      else if ((et == Type::Int64 || et == Type::Float64) && (ct == Type::Int64 || ct == Type::Float64))
        et = Type::Float64;  // INTEGER and FLOAT elements widen together
      else
        not_impl(std::string("Lists of different inner types are not supported (") + type_name(et) + ", " +
                 type_name(ct) + ")");
    }
    nn->list_elem = et;
  } else {  // SLICE / REVERSE
    if (type_of(0) == Type::Null) {
      out_type = Type::Null;  // a NULL list
    } else if (type_of(0) != Type::List) {
      not_impl(std::string(fn == CAPF_LIST_FN_SLICE ? "a slice" : "reverse()") + " of a " + type_name(type_of(0)));
    } else {
      nn->list_elem = list_elem_of(c, nn->name_cols[0]);
    }
    if (fn == CAPF_LIST_FN_SLICE) {
      integer_arg(1, "a slice bound");
      integer_arg(2, "a slice bound");
    }
  }
  nn->names.emplace_back(name);
  nn->types.push_back(out_type);
  *out = wrap(nn);
  CAPF_API_END
}

capf_status capf_table_str_split(capf_table *t, const char *str_col, const char *delim_col, const char *name,
                                 capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(str_col, "str_col");
  need(delim_col, "delim_col");
  need(name, "name");
  need(out, "out");
  const NodePtr &c = t->node;
  if (c->col_index(name) >= 0) illegal(std::string("column '") + name + "' already exists");
  auto nn = new_node(c->s, Kind::StrSplit);
  nn->kids.push_back(c);
  nn->names = c->names;
  nn->types = c->types;
  nn->name_cols = {c->col_index_or_throw(str_col), c->col_index_or_throw(delim_col)};
  Type out_type = Type::List;
  for (int j : nn->name_cols) {
    const Type ct = c->types[(size_t)j];
    if (ct == Type::Null) out_type = Type::Null;  // a NULL operand: a NULL list
    else if (ct != Type::String) illegal(std::string("split() of a ") + type_name(ct) + " column, not a STRING");
  }
  nn->list_elem = Type::String;
  nn->names.emplace_back(name);
  nn->types.push_back(out_type);
  *out = wrap(nn);
  CAPF_API_END
}

capf_status capf_table_list_lambda(capf_table *t, int32_t kind, const char *list, const capf_expr *pred,
                                   const capf_expr *body, const char *init, int32_t out_type, const char *name,
                                   capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(list, "list");
  need(name, "name");
  need(out, "out");
  if (kind < CAPF_LAMBDA_COMPREHENSION || kind > CAPF_LAMBDA_REDUCE) illegal("unknown lambda expression kind");
  if (is_temporal((Type)out_type)) not_impl(std::string("a lambda expression that gives ") + type_name((Type)out_type) + " values");
  if (out_type < 0 || out_type > 4) illegal("lambda expression result type out of range");
  const bool quant = kind >= CAPF_LAMBDA_ANY && kind <= CAPF_LAMBDA_SINGLE, reduce = kind == CAPF_LAMBDA_REDUCE;
  if (quant && !pred) illegal("any / all / none / single need a predicate");
  if (reduce && (!body || !init || !init[0])) illegal("reduce needs a body and an init column");
  if (reduce && pred) illegal("reduce takes no predicate");
  const NodePtr &c = t->node;
  if (c->col_index(name) >= 0) illegal(std::string("column '") + name + "' already exists");
  auto nn = new_node(c->s, Kind::ListLambda);
  nn->kids.push_back(c);
  nn->names = c->names;
  nn->types = c->types;
  nn->list_fn = kind;
  const int li = c->col_index_or_throw(list);
  const Type lt = c->types[(size_t)li];
  if (lt != Type::List && lt != Type::Null)
    illegal(std::string("a lambda expression over a ") + type_name(lt) + " column, not a LIST");
  nn->name_cols = {li, reduce ? c->col_index_or_throw(init) : -1};
  const Type et = lt == Type::List ? list_elem_of(c, li) : Type::Null;
  if (et == Type::List) not_impl("nested lists");
  const Type ot = (Type)out_type;
  nn->exprs.resize(2);
  if (pred) nn->exprs[0] = Program::from_c(pred);
  if (body) nn->exprs[1] = Program::from_c(body);
  auto fits = [](Type got, Type want) {  // a value of type `got` stored as `want`
    return got == want || got == Type::Null || (got == Type::Int64 && want == Type::Float64);
  };
  if (reduce) {
    const Type it = c->types[(size_t)nn->name_cols[1]];
    if (it == Type::List) not_impl("reduce with a list accumulator (nested lists)");
    // the accumulator is typed as the result: init's type, widened or taken from the body
    nn->lambda_types = {ot, et};
    const Type bt = infer_type(nn->exprs[1], c->names, c->types, &nn->lambda_types);
    if (!fits(it, ot) || !fits(bt, ot) || (it != Type::Null && it != ot && !(it == Type::Int64 && bt == Type::Float64)))
      illegal(std::string("reduce: init is ") + type_name(it) + ", the body " + type_name(bt));
  } else {
    nn->lambda_types = {et};
    if (pred) {
      const Type pt = infer_type(nn->exprs[0], c->names, c->types, &nn->lambda_types);
      if (pt != Type::Bool && pt != Type::Null) illegal(std::string("a lambda predicate of type ") + type_name(pt));
    }
    if (body) {
      if (quant) illegal("any / all / none / single take no extract expression");
      const Type bt = infer_type(nn->exprs[1], c->names, c->types, &nn->lambda_types);
      if (bt == Type::List) not_impl("nested lists");
      if (!fits(bt, ot)) illegal(std::string("an extract expression of type ") + type_name(bt) + " declared " + type_name(ot));
    } else if (!quant && et != ot) {
      illegal(std::string("a filter over ") + type_name(et) + " elements declared " + type_name(ot));
    }
  }
  nn->list_elem = quant ? Type::Bool : ot;
  nn->names.emplace_back(name);
  nn->types.push_back(lt == Type::Null ? Type::Null : quant ? Type::Bool : reduce ? ot : Type::List);
  *out = wrap(nn);
  CAPF_API_END
}

capf_status capf_table_explode_list(capf_table *t, const char *list_col, const char *name, capf_table **out) {
  CAPF_API_BEGIN
  need(t, "table");
  need(list_col, "list_col");
  need(name, "name");
  need(out, "out");
  const NodePtr &c = t->node;
  int li = c->col_index_or_throw(list_col);
  if (c->types[li] != Type::List && c->types[li] != Type::Null) illegal("UNWIND of a non-list column");
  if (c->col_index(name) >= 0) illegal(std::string("column '") + name + "' already exists");
  auto nn = new_node(c->s, Kind::Explode);
  nn->kids.push_back(c);
  nn->names = c->names;
  nn->types = c->types;
  nn->names.emplace_back(name);
  // the element type is known once the list column exists; a NULL-typed
  // column explodes to nothing
  nn->types.push_back(Type::Null);
  nn->explode_list_col = li;
  if (c->types[li] == Type::List) {
    Type et;
    if (static_list_elem(c, li, et)) {
      nn->types.back() = et;
    } else {  // a computed list: its element type is known once it exists
      DataPtr d = materialize(c);
      const ColPtr &lc = d->cols[li];
      nn->types.back() = lc->child ? lc->child->type : Type::Null;
    }
  }
  *out = wrap(nn);
  CAPF_API_END
}

capf_status capf_table_show(capf_table *t, int32_t rows) {
  CAPF_API_BEGIN
  need(t, "table");
  DataPtr d = materialize(t->node);
  Session *s = t->node->s;
  int64_t m = std::min<int64_t>(rows, d->nrows);
  std::vector<std::vector<int64_t>> vals(d->cols.size(), std::vector<int64_t>(m));
  std::vector<std::vector<uint8_t>> valid(d->cols.size(), std::vector<uint8_t>(m, 1));
  for (size_t i = 0; i < d->cols.size(); ++i) {
    const ColPtr c = decode_column(s, d->cols[i]);
    s->sync();
    if (m == 0) continue;
    if (c->type == Type::Null) {
      std::fill(valid[i].begin(), valid[i].end(), 0);
      continue;
    }
    if (c->type == Type::List) {  // shown as its length
      std::vector<int64_t> off(m + 1);
      HIP_CHECK(hipMemcpy(off.data(), c->data->p, 8 * (m + 1), hipMemcpyDeviceToHost));
      for (int64_t r = 0; r < m; ++r) vals[i][r] = off[r + 1] - off[r];
      if (c->valid) HIP_CHECK(hipMemcpy(valid[i].data(), c->valid->p, m, hipMemcpyDeviceToHost));
      continue;
    }
    std::vector<uint8_t> raw(type_width(c->type) * m);
    HIP_CHECK(hipMemcpy(raw.data(), c->data->p, raw.size(), hipMemcpyDeviceToHost));
    for (int64_t r = 0; r < m; ++r)
      vals[i][r] = c->type == Type::Bool ? raw[r] : ((int64_t *)raw.data())[r];
    if (c->valid) HIP_CHECK(hipMemcpy(valid[i].data(), c->valid->p, m, hipMemcpyDeviceToHost));
  }
  for (size_t i = 0; i < d->cols.size(); ++i) printf("%s%s", i ? " | " : "", t->node->names[i].c_str());
  printf("\n");
  for (int64_t r = 0; r < m; ++r) {
    for (size_t i = 0; i < d->cols.size(); ++i) {
      if (i) printf(" | ");
      auto ty = d->cols[i]->type;
      if (!valid[i][r]) {
        printf("null");
      } else if (ty == Type::Float64) {
        double f;
        memcpy(&f, &vals[i][r], 8);
        printf("%g", f);
      } else if (ty == Type::Bool) {
        printf("%s", vals[i][r] ? "true" : "false");
      } else if (ty == Type::List) {
        printf("[%lld values]", (long long)vals[i][r]);
      } else if (ty == Type::String) {
        printf("'%s'", s->dict.lookup(vals[i][r], "?"));
      } else {
        printf("%lld", (long long)vals[i][r]);
      }
    }
    printf("\n");
  }
  fflush(stdout);
  CAPF_API_END
}

}  // extern "C"
