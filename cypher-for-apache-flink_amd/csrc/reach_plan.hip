// reach_plan.hip — the plan matcher of the fused var-length reach: recognises the
// lowered DISTINCT / GROUP BY over var-length join chains in the lazy plan DAG
// and hands it to var_length_reach.hip.  Host code only.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>

#include "capf_internal.h"
#include "join_graph.h"

namespace capf {

// ============================================================ fused reach
// Config 5 below the Table SPI.  The unchanged okapi front end lowers
//   MATCH (a)-[:T*1..u]->(b) WITH DISTINCT a, b WITH a, count(*) AS reach
// into (DirectedVarLengthExpandPlanner, VarLengthExpandPlanner.scala:82-259;
// Distinct RelationalOperator.scala:325-332; Aggregate :334-346)
//   Group(a-columns; count(*))
//     ← [column copies] ← Distinct(a-columns, b-columns) ← [column copies]
//     ← UNION ALL over k = 1..u of
//         S_a ⋈[a = start(e1)] E ⋈[end(e1) = start(e2)] E … E ⋈[end(ek) = b] S_b
//         → Filter(NOT(e_i = e_j)) → withColumns(NULL padding)
// which would materialise every path (~1e10 rows at SF10).  When the DAG has
// exactly this shape, the Group is evaluated by the multi-source BFS of
// var_length_reach.hip instead — CAPF's Calcite rule set plays the same
// physical-choice role (flink-cypher/.../api/CAPFSession.scala:83-91).
// Exact for lower bound 1 (directed): the DISTINCT (a, b) pairs of
// relationship-isomorphic paths of length 1..u are exactly the pairs joined by
// a walk of length 1..u (cutting the closed sub-walk between two uses of a rel
// leaves a shorter walk with the same endpoints), so the isomorphism filters
// do not change the answer.  Group keys other than a's id must be columns of
// S_a (functions of the unique id) or literals; DISTINCT columns columns of
// S_a / S_b or literals.  Any other shape returns false (relational path).

static bool prog_eq(const Program &a, const Program &b) {
  if (a.code.size() != b.code.size() || a.names != b.names) return false;
  for (size_t i = 0; i < a.code.size(); ++i)
    if (a.code[i].op != b.code[i].op || a.code[i].i != b.code[i].i ||
        __builtin_bit_cast(uint64_t, a.code[i].f) != __builtin_bit_cast(uint64_t, b.code[i].f))
      return false;
  return true;
}

static bool progs_eq(const std::vector<Program> &a, const std::vector<Program> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (!prog_eq(a[i], b[i])) return false;
  return true;
}

static bool reach_reject(const char *why) {
  static const bool trace = getenv("CAPF_TRACE_FUSE") && atoi(getenv("CAPF_TRACE_FUSE")) == 1;
  if (trace) fprintf(stderr, "[capf] fused reach not applied: %s\n", why);
  return false;
}

// last_plan of a fused reach, by the method that answers it
static const char *reach_plan_name(ReachMethod rm) {
  return rm == ReachMethod::STEPS ? "fused_var_length_undirected"
         : rm == ReachMethod::TRAILS ? "fused_var_length_trails" : "fused_var_length_reach";
}

static bool is_literal_program(const Program &p) { return p.code.size() == 1 && p.code[0].op != OP_COL; }

// Descends through column-mapping operators (Select; withColumns whose
// expressions are column copies or literals), re-expressing the tracked
// columns; returns the first other node.
NodePtr through_mappings(NodePtr n, std::vector<TCol> &cols) {
  for (;;) {
    if (n->kind == Kind::Select) {
      for (auto &c : cols)
        if (!c.lit) c.col = n->sel_index[c.col];
      n = n->kids[0];
      continue;
    }
    if (n->kind == Kind::WithColumns) {
      for (auto &p : n->exprs)
        if (p.code.size() != 1) return n;
      const NodePtr &kid = n->kids[0];
      for (auto &c : cols) {
        if (c.lit) continue;
        int k = -1;
        for (size_t t = 0; t < n->target_index.size(); ++t)
          if (n->target_index[t] == c.col) k = (int)t;
        if (k < 0) continue;  // passes through at the same index
        const Program &p = n->exprs[k];
        if (is_literal_program(p)) {
          c.lit = &p;
          c.col = -1;
        } else {
          const int64_t ni = p.code[0].i;
          if (ni < 0 || (size_t)ni >= p.names.size()) return n;
          c.col = kid->col_index(p.names[(size_t)ni]);
          if (c.col < 0) return n;
        }
      }
      n = kid;
      continue;
    }
    return n;
  }
}

struct ReachBranch {
  NodePtr base;
  std::vector<TCol> cols;
};

static bool union_branches(NodePtr n, std::vector<TCol> cols, std::vector<ReachBranch> &out) {
  n = through_mappings(n, cols);
  if (n->kind != Kind::Union) {
    out.push_back(ReachBranch{n, cols});
    return out.size() <= 64;
  }
  std::vector<TCol> rc = cols;
  for (auto &c : rc)
    if (!c.lit) {
      c.col = n->kids[1]->col_index(n->names[c.col]);
      if (c.col < 0) return false;
    }
  return union_branches(n->kids[0], cols, out) && union_branches(n->kids[1], rc, out);
}

// One branch's role of a tracked column.
struct RCol {
  int role = -1;  // 0: S_a column, 1: S_b column, 2: literal
  int col = -1;
  Program lit;     // role 2 (a copy: the branch's join graph is temporary)
};

struct ReachShape {
  Leaf sa, sb, rel;
  int x = -1, y = -1, cs = -1, cd = -1;  // S_a / S_b id columns, rel start / end columns
  int k = 0;                              // rel leaves in the chain
  bool all_neq = false;                   // every pair of them carries NOT(e_i = e_j), on one column
  std::vector<RCol> roles;                // per tracked column
};

static bool leaf_eq(const Leaf &a, const Leaf &b) {
  return a.node == b.node && progs_eq(a.filters, b.filters) && a.col_eqs == b.col_eqs;
}

// The chain S_a ⋈ E ⋈ … ⋈ E ⋈ S_b of one branch; `a_cols` are tracked columns
// that must lie on S_a (the group keys).  With `links` (the undirected
// lowering) every rel leaf may be entered and left by either endpoint column,
// or by one column twice: the (entry, exit) column pairs are recorded for the
// caller to judge, and sh.cs / sh.cd stay unset.
static bool reach_branch(const ReachBranch &br, const std::vector<int> &a_cols, ReachShape &sh,
                         std::vector<std::pair<int, int>> *links = nullptr) {
  JoinGraph g;
  std::vector<ColRef> refs;
  if (br.base->kind != Kind::Join && br.base->kind != Kind::Filter) return reach_reject("branch check 1");
  if (!collect(br.base, g, refs)) return reach_reject("branch check 2");
  const int L = (int)g.leaves.size();
  if (L < 3 || (int)g.eqs.size() != L - 1) return reach_reject("branch check 3");
  // tracked column → (leaf, col) or literal
  std::vector<ColRef> tr(br.cols.size());
  std::vector<const Program *> tl(br.cols.size(), nullptr);
  for (size_t i = 0; i < br.cols.size(); ++i) {
    if (br.cols[i].lit) {
      tl[i] = br.cols[i].lit;
      continue;
    }
    tr[i] = refs[br.cols[i].col];
    if (tr[i].leaf == -2 && tr[i].col >= 0) tl[i] = &g.lits[tr[i].col];  // copied into the roles
    else if (tr[i].leaf < 0) return reach_reject("branch check 4");
  }
  int la = -1;
  for (int i : a_cols)
    if (!tl[i]) {
      if (la >= 0 && tr[i].leaf != la) return reach_reject("branch check 5");
      la = tr[i].leaf;
    }
  if (la < 0) return reach_reject("branch check 6");
  auto edges_of = [&](int leaf) {
    std::vector<std::pair<int, ColRef>> r;  // (my col, other)
    for (auto &e : g.eqs) {
      if (e.first.leaf == leaf) r.emplace_back(e.first.col, e.second);
      if (e.second.leaf == leaf) r.emplace_back(e.second.col, e.first);
    }
    return r;
  };
  auto ea = edges_of(la);
  if (ea.size() != 1) return reach_reject("branch check 7");
  sh.sa = g.leaves[la];
  sh.x = ea[0].first;
  int cur = ea[0].second.leaf, entry = ea[0].second.col, prev = la, lb = -1;
  std::vector<char> seen(L, 0);
  seen[la] = 1;
  sh.k = 0;
  sh.cs = entry;
  std::vector<int> pos(L, -1);  // leaf → its place among the chain's rel leaves
  for (;;) {
    if (cur < 0 || seen[cur]) return reach_reject("branch check 8");
    seen[cur] = 1;
    auto e = edges_of(cur);
    if (e.size() == 1) {  // the far end: S_b
      lb = cur;
      sh.y = entry;
      break;
    }
    if (e.size() != 2) return reach_reject("branch check 9");
    const Leaf &lr = g.leaves[cur];
    if (sh.k == 0) sh.rel = lr;
    else if (!leaf_eq(lr, sh.rel)) return reach_reject("branch check 10");
    if (!links && entry != sh.cs) return reach_reject("branch check 11");
    const auto &out = e[0].second.leaf == prev && e[0].first == entry ? e[1] : e[0];
    if (links) {
      links->emplace_back(entry, out.first);
    } else {
      if (out.first == entry) return reach_reject("branch check 12");
      if (sh.k == 0) sh.cd = out.first;
      else if (out.first != sh.cd) return reach_reject("branch check 13");
    }
    pos[cur] = sh.k;
    ++sh.k;
    prev = cur;
    cur = out.second.leaf;
    entry = out.second.col;
  }
  for (int i = 0; i < L; ++i)
    if (!seen[i]) return reach_reject("branch check 14");
  if (sh.k < 1 || lb < 0) return reach_reject("branch check 15");
  sh.sb = g.leaves[lb];
  if (sh.sa.node == sh.rel.node || sh.sb.node == sh.rel.node) return reach_reject("branch check 16");
  if (!sh.rel.col_eqs.empty() || !sh.sa.col_eqs.empty() || !sh.sb.col_eqs.empty()) return reach_reject("branch check 17");
  // isomorphism filters: NOT(e_i = e_j) on one unique rel column.  Walks
  // (lower bound ≤ 1) need none of them; for trails they are the semantics,
  // so all_neq records whether all k(k−1)/2 pairs are there, on one column.
  std::vector<char> pair_seen((size_t)sh.k * sh.k, 0);
  int npairs = 0, neq_col = -1;
  bool one_col = true;
  for (auto &ne : g.neqs) {
    if (ne.first.leaf == ne.second.leaf || ne.first.col != ne.second.col) return reach_reject("branch check 18");
    if (ne.first.leaf == la || ne.first.leaf == lb || ne.second.leaf == la || ne.second.leaf == lb)
      return reach_reject("branch check 19");
    if (!column_unique(sh.rel.node, ne.first.col)) return reach_reject("branch check 20");
    if (neq_col < 0) neq_col = ne.first.col;
    one_col &= ne.first.col == neq_col;
    if (ne.first.leaf < 0 || ne.second.leaf < 0 || pos[ne.first.leaf] < 0 || pos[ne.second.leaf] < 0) {
      one_col = false;
      continue;
    }
    const int i = std::min(pos[ne.first.leaf], pos[ne.second.leaf]);
    const int j = std::max(pos[ne.first.leaf], pos[ne.second.leaf]);
    if (!pair_seen[(size_t)i * sh.k + j]) {
      pair_seen[(size_t)i * sh.k + j] = 1;
      ++npairs;
    }
  }
  sh.all_neq = one_col && npairs == sh.k * (sh.k - 1) / 2;
  // roles of the tracked columns
  sh.roles.assign(br.cols.size(), RCol{});
  for (size_t i = 0; i < br.cols.size(); ++i) {
    RCol &r = sh.roles[i];
    if (tl[i]) {
      r.role = 2;
      r.lit = *tl[i];
    } else if (tr[i].leaf == la) {
      r.role = 0;
      r.col = tr[i].col;
    } else if (tr[i].leaf == lb) {
      r.role = 1;
      r.col = tr[i].col;
    } else {
      return reach_reject("branch check 21");
    }
  }
  return true;
}

// The directed lowering: one chain per length l..u, all on the same leaves and
// columns.
static bool directed_shapes(const std::vector<ReachBranch> &brs, const std::vector<int> &a_cols, size_t ntracked,
                            bool zero, std::vector<ReachShape> &shapes, int &lower_out, int &upper_out) {
  shapes.assign(brs.size(), ReachShape{});
  uint64_t lengths = 0;
  for (size_t b = 0; b < brs.size(); ++b) {
    if (!reach_branch(brs[b], a_cols, shapes[b])) return reach_reject("a branch is not a var-length chain");
    const ReachShape &sh = shapes[b], &s0 = shapes[0];
    if (sh.k > 64 || (lengths >> (sh.k - 1) & 1)) return reach_reject("branch lengths");
    lengths |= uint64_t(1) << (sh.k - 1);
    if (!leaf_eq(sh.sa, s0.sa) || !leaf_eq(sh.sb, s0.sb) || !leaf_eq(sh.rel, s0.rel))
      return reach_reject("branches scan different tables");
    if (sh.x != s0.x || sh.y != s0.y || sh.cs != s0.cs || sh.cd != s0.cd)
      return reach_reject("branches join different columns");
    for (size_t i = 0; i < ntracked; ++i) {
      const RCol &r = sh.roles[i], &r0 = s0.roles[i];
      if (r.role != r0.role || r.col != r0.col) return reach_reject("column roles differ across branches");
      if (r.role == 2 && !prog_eq(r.lit, r0.lit)) return reach_reject("literals differ across branches");
    }
  }
  const int upper = 64 - __builtin_clzll(lengths), lower = __builtin_ctzll(lengths) + 1;
  if ((lengths >> (lower - 1)) != (upper - lower == 63 ? ~uint64_t(0) : (uint64_t(1) << (upper - lower + 1)) - 1))
    return reach_reject("lengths are not l..u");
  if (lower >= 2) {  // trails (var_length_reach.hip::k_vt_trails)
    if (zero) return reach_reject("a zero-length branch beside lengths from 2");
    if (reach_method(false, lower, upper) != ReachMethod::TRAILS) return reach_reject("trail lengths above 4");
    for (auto &sh : shapes)
      if (!sh.all_neq) return reach_reject("a branch lacks some NOT(e_i = e_j) filters: not a trail");
  }
  lower_out = lower;
  upper_out = upper;
  return true;
}

// ---- the undirected lowering (VarLengthExpandPlanner.scala:277-307)
// Each step joins the (out, in) tables of the step before four ways and
// unions them pairwise, so its DAG has Union nodes BELOW joins.  hoist_unions
// rewrites a node into union-free alternatives whose UNION ALL it is: a Union
// over joins contributes the alternatives of both inputs (the second one's
// columns realigned by name, as union_branches does), and Join / Filter /
// Select / literal-only WithColumns above it are copied once per combination
// of their inputs' alternatives.  The copies are temporary plan nodes (as
// filter_node builds them) that only `collect` reads; leaves are never copied,
// so leaf identity holds across alternatives.  A Union with no join beneath (a
// node scan over several label tables) stays the opaque leaf it is to `collect`.
constexpr size_t HOIST_MAX = 64;  // alternatives of one node

struct Hoist {
  std::map<const Node *, std::vector<NodePtr>> memo;
  std::map<const Node *, bool> joins;
  bool failed = false;
};

static bool is_materialised(const NodePtr &n) {
  std::lock_guard<std::mutex> lk(n->mu);
  return n->result != nullptr;
}

static bool has_join(const NodePtr &n, Hoist &h) {
  auto it = h.joins.find(n.get());
  if (it != h.joins.end()) return it->second;
  bool j = false;
  if (!is_materialised(n)) {
    j = n->kind == Kind::Join;
    for (auto &k : n->kids) j = j || has_join(k, h);
  }
  h.joins[n.get()] = j;
  return j;
}

static NodePtr with_kids(const NodePtr &n, std::vector<NodePtr> kids) {
  auto c = std::make_shared<Node>();
  c->s = n->s;
  c->kind = n->kind;
  c->names = n->names;
  c->types = n->types;
  c->kids = std::move(kids);
  c->sel_index = n->sel_index;
  c->pred = n->pred;
  c->join_type = n->join_type;
  c->join_keys = n->join_keys;
  c->exprs = n->exprs;
  c->target_index = n->target_index;
  return c;
}

static std::vector<NodePtr> hoist_unions(const NodePtr &n, Hoist &h) {
  if (h.failed) return {};
  auto it = h.memo.find(n.get());
  if (it != h.memo.end()) return it->second;
  std::vector<NodePtr> out;
  bool through = false;  // an operator `collect` looks through
  if (!is_materialised(n)) {
    switch (n->kind) {
      case Kind::Select:
      case Kind::Filter: through = true; break;
      case Kind::Join: through = n->join_type == CAPF_JOIN_INNER; break;
      case Kind::WithColumns:
        through = true;
        for (auto &p : n->exprs) through = through && is_literal_program(p);
        break;
      default: break;
    }
  }
  if (!is_materialised(n) && n->kind == Kind::Union && n->kids.size() == 2 && has_join(n, h)) {
    out = hoist_unions(n->kids[0], h);
    std::vector<int> idx;
    for (auto &nm : n->names) {
      idx.push_back(n->kids[1]->col_index(nm));
      if (idx.back() < 0) h.failed = true;
    }
    for (auto &r : hoist_unions(n->kids[1], h)) {
      auto sel = std::make_shared<Node>();
      sel->s = n->s;
      sel->kind = Kind::Select;
      sel->names = n->names;
      sel->types = n->types;
      sel->kids = {r};
      sel->sel_index = idx;
      out.push_back(sel);
    }
  } else if (through && n->kids.size() == 1) {
    for (auto &k : hoist_unions(n->kids[0], h)) out.push_back(k == n->kids[0] ? n : with_kids(n, {k}));
  } else if (through && n->kids.size() == 2) {
    const std::vector<NodePtr> l = hoist_unions(n->kids[0], h), r = hoist_unions(n->kids[1], h);
    if (l.size() * r.size() > HOIST_MAX) h.failed = true;
    else
      for (auto &a : l)
        for (auto &b : r) out.push_back(a == n->kids[0] && b == n->kids[1] ? n : with_kids(n, {a, b}));
  } else {
    out = {n};
  }
  if (out.size() > HOIST_MAX) h.failed = true;
  if (h.failed) return {};
  h.memo[n.get()] = out;
  return out;
}

// Every hoisted alternative of length k must be one mode vector m ∈ {out, in}^k
// of the automaton (var_length_reach.hip, "undirected steps"), link by link,
// with cs / cd the rel's start / end column:
//   S_a.id = e_1.(m_1 = out ? cs : cd)
//   e_i leaves by (m_i = out ? cd : cs); e_{i+1} is entered by cs when
//   m_i = m_{i+1} and by cd otherwise; the last exit joins S_b.id
// and the alternatives must be all 2^k vectors of every length l..u ≤ 4, each
// with all its NOT(e_i = e_j) filters, on the same three leaves and columns.
// Which of the two columns is the start follows from the links (the two
// readings agree only where no alternative has a link, u = 1, and there they
// give the same pairs).
static bool undirected_shapes(const std::vector<ReachBranch> &brs, const std::vector<int> &a_cols, size_t ntracked,
                              bool zero, std::vector<ReachShape> &shapes, int &lower_out, int &upper_out) {
  Hoist hz;
  std::vector<ReachBranch> hb;
  for (auto &br : brs) {
    for (auto &alt : hoist_unions(br.base, hz)) hb.push_back(ReachBranch{alt, br.cols});
    if (hz.failed || hb.size() > HOIST_MAX) return reach_reject("undirected: too many union alternatives");
  }
  if (hb.empty()) return reach_reject("undirected: no alternatives");
  shapes.assign(hb.size(), ReachShape{});
  std::vector<std::vector<std::pair<int, int>>> links(hb.size());
  int c0 = -1, c1 = -1;  // the two rel columns the links use
  for (size_t b = 0; b < hb.size(); ++b) {
    if (!reach_branch(hb[b], a_cols, shapes[b], &links[b])) return reach_reject("undirected: an alternative is not a chain");
    const ReachShape &sh = shapes[b], &s0 = shapes[0];
    if (reach_method(true, sh.k, sh.k) == ReachMethod::NONE) return reach_reject("undirected lengths above 4");
    if (!sh.all_neq) return reach_reject("undirected: an alternative lacks some NOT(e_i = e_j) filters");
    if (!leaf_eq(sh.sa, s0.sa) || !leaf_eq(sh.sb, s0.sb) || !leaf_eq(sh.rel, s0.rel))
      return reach_reject("undirected: alternatives scan different tables");
    if (sh.x != s0.x || sh.y != s0.y) return reach_reject("undirected: alternatives join different id columns");
    for (size_t i = 0; i < ntracked; ++i) {
      const RCol &r = sh.roles[i], &r0 = s0.roles[i];
      if (r.role != r0.role || r.col != r0.col) return reach_reject("undirected: column roles differ");
      if (r.role == 2 && !prog_eq(r.lit, r0.lit)) return reach_reject("undirected: literals differ");
    }
    for (auto &lk : links[b])
      for (int c : {lk.first, lk.second}) {
        if (c == c0 || c == c1) continue;
        if (c0 < 0) c0 = c;
        else if (c1 < 0) c1 = c;
        else return reach_reject("undirected: more than two rel columns joined");
      }
  }
  if (c1 < 0) return reach_reject("undirected: one rel column joined");
  for (int turn = 0; turn < 2; ++turn) {
    const int cs = turn ? c1 : c0, cd = turn ? c0 : c1;
    uint32_t seen[5] = {0, 0, 0, 0, 0};  // per length: the mode vectors met (bit = vector, in = 1)
    bool ok = true;
    for (size_t b = 0; b < hb.size() && ok; ++b) {
      const auto &lk = links[b];
      uint32_t vec = 0;
      for (size_t i = 0; i < lk.size() && ok; ++i) {
        const bool in = lk[i].second == cs;
        const bool same = i == 0 ? !in : in == (bool)((vec >> (i - 1)) & 1u);  // the start state is (a, out)
        ok = lk[i].first == (same ? cs : cd);
        vec |= (in ? 1u : 0u) << i;
      }
      seen[lk.size()] |= 1u << vec;
    }
    int lower = 0, upper = 0;
    for (int k = 1; k <= 4 && ok; ++k) {
      if (!seen[k]) continue;
      ok = seen[k] == (k == 4 ? 0xFFFFu : (1u << (1u << k)) - 1u);  // all 2^k vectors
      if (!lower) lower = k;
      else if (upper != k - 1) ok = false;  // contiguous
      upper = k;
    }
    if (!ok) continue;
    if (zero && lower >= 2) return reach_reject("a zero-length branch beside lengths from 2");
    for (auto &sh : shapes) {
      sh.cs = cs;
      sh.cd = cd;
    }
    lower_out = lower;
    upper_out = upper;
    return true;
  }
  return reach_reject("undirected: the alternatives are not all mode vectors of lengths l..u");
}

bool try_fused_reach(const NodePtr &grp, DataPtr &result) {
  const char *fe = getenv("CAPF_FUSED_REACH");  // 0: always the relational plan
  if (fe && atoi(fe) == 0) return false;
  if (grp->kind != Kind::Group || grp->key_index.empty() || grp->aggs.empty()) return false;
  for (auto &a : grp->aggs)
    if (a.kind != CAPF_AGG_COUNT_STAR) return false;
  Session *s = grp->s;
  // group keys → columns of the Distinct
  std::vector<TCol> gk;
  for (int k : grp->key_index) gk.push_back(TCol{k, nullptr});
  NodePtr d = through_mappings(grp->kids[0], gk);
  if (d->kind != Kind::Distinct || d->key_index.empty()) return reach_reject("group input is not a DISTINCT");
  {
    std::lock_guard<std::mutex> lk(d->mu);
    if (d->result) return false;  // already materialised: the plain group is cheap
  }
  // tracked columns below the Distinct: its keys, then the group keys
  std::vector<TCol> tracked;
  for (int k : d->key_index) tracked.push_back(TCol{k, nullptr});
  const size_t nd = tracked.size();
  std::vector<int> gk_at(gk.size(), -1);  // group key → tracked index (−1: literal)
  for (size_t i = 0; i < gk.size(); ++i) {
    if (gk[i].lit) continue;
    gk_at[i] = (int)tracked.size();
    tracked.push_back(TCol{gk[i].col, nullptr});
  }
  std::vector<int> a_cols;
  for (int t : gk_at)
    if (t >= 0) a_cols.push_back(t);
  if (a_cols.empty()) return reach_reject("no group key column");
  std::vector<ReachBranch> brs;
  if (!union_branches(d->kids[0], tracked, brs)) return reach_reject("union branches");
  // lower bound 0: one branch is the copyElement branch (VarLengthExpandPlanner.scala:180-205),
  // S_a itself with b's columns copied from a's — no join below the mappings
  int zero = -1;
  for (size_t b = 0; b < brs.size(); ++b)
    if (brs[b].base->kind != Kind::Join) {
      JoinGraph g0;
      std::vector<ColRef> r0;
      if (collect(brs[b].base, g0, r0) && g0.leaves.size() == 1 && g0.eqs.empty()) {
        if (zero >= 0) return reach_reject("two zero-length branches");
        zero = (int)b;
      }
    }
  const ReachBranch zbr = zero >= 0 ? brs[(size_t)zero] : ReachBranch{};
  if (zero >= 0) brs.erase(brs.begin() + zero);
  if (brs.empty()) return reach_reject("no var-length chain");
  std::vector<ReachShape> shapes;
  int lower = 0, upper = 0;
  bool undirected = false;
  if (!directed_shapes(brs, a_cols, tracked.size(), zero >= 0, shapes, lower, upper)) {
    if (!undirected_shapes(brs, a_cols, tracked.size(), zero >= 0, shapes, lower, upper)) return false;
    undirected = true;
  }
  const ReachShape &sh = shapes[0];
  // DISTINCT over (a, b): both ids among its keys, every key a column of S_a /
  // S_b or a literal; group keys: S_a columns (with the id) or literals
  bool has_x = false, has_y = false;
  for (size_t i = 0; i < nd; ++i) {
    const RCol &r = sh.roles[i];
    has_x |= r.role == 0 && r.col == sh.x;
    has_y |= r.role == 1 && r.col == sh.y;
  }
  bool gx = false;
  for (int t : a_cols) {
    if (sh.roles[t].role == 1) return reach_reject("a group key is a target column");
    gx |= sh.roles[t].role == 0 && sh.roles[t].col == sh.x;
  }
  if (!has_x || !has_y || !gx) return reach_reject("DISTINCT / group keys lack the endpoint ids");
  if (zero >= 0) {  // the copy branch: S_a's leaf, a's columns where the chains have a's / b's
    JoinGraph g0;
    std::vector<ColRef> r0;
    if (!collect(zbr.base, g0, r0) || g0.leaves.size() != 1 || !g0.neqs.empty() || !leaf_eq(g0.leaves[0], sh.sa))
      return reach_reject("the zero-length branch is not the source scan");
    const bool same_scan = leaf_eq(sh.sa, sh.sb);
    for (size_t i = 0; i < tracked.size(); ++i) {
      const RCol &r = sh.roles[i];
      const TCol &z = zbr.cols[i];
      const Program *zl = z.lit;
      ColRef zr{-1, -1};
      if (!zl) {
        zr = r0[(size_t)z.col];
        if (zr.leaf == -2 && zr.col >= 0) zl = &g0.lits[(size_t)zr.col];
      }
      if (r.role == 2) {
        if (!zl || !prog_eq(*zl, r.lit)) return reach_reject("zero-length branch: a literal differs");
        continue;
      }
      if (zl || zr.leaf != 0) return reach_reject("zero-length branch: a column is not the source's");
      const int want = r.role == 0 ? r.col : r.col == sh.y ? sh.x : same_scan ? r.col : -1;
      if (want < 0 || zr.col != want) return reach_reject("zero-length branch: b's column is not a's");
    }
  }
  if (!column_unique(sh.sa.node, sh.x) || !column_unique(sh.sb.node, sh.y))
    return reach_reject("endpoint ids not unique");
  // rel endpoint columns: non-null INTEGER
  LeafData lr = leaf_data(sh.rel), la = leaf_data(sh.sa), lb = leaf_data(sh.sb);
  const ColPtr &rs = lr.data->cols[sh.cs], &rd = lr.data->cols[sh.cd];
  const ColPtr &xa = la.data->cols[sh.x], &yb = lb.data->cols[sh.y];
  for (const ColPtr *c : {&rs, &rd, &xa, &yb}) {
    force(*c);
    if ((*c)->type != Type::Int64 || (*c)->valid) return reach_reject("nullable or non-INTEGER ids");
  }
  if (lr.data->nrows >= (int64_t(1) << 32)) return reach_reject("more than 2^32 rels");
  if (zero >= 0) lower = 0;
  DataPtr res = var_length_reach_rows(s, rs, rd, lr.data->nrows, xa, la.data->nrows, yb, lb.data->nrows, lower, upper,
                                      undirected);
  if (!res) return reach_reject("more nodes than the enumeration kernel's LDS bitmap holds");
  s->last_plan = reach_plan_name(reach_method(undirected, lower, upper));
  // output: group keys (a's id, other S_a columns gathered by a's row, literals)
  // then one reach column per count(*)
  const int64_t nr = res->nrows;
  auto out = std::make_shared<Data>();
  out->nrows = nr;
  bool need_rows = false;
  for (int t : a_cols) need_rows |= sh.roles[t].role == 0 && sh.roles[t].col != sh.x;
  DataPtr a_rows;  // S_a's columns at each result row
  std::vector<ColPtr> rcols = res->cols;
  if (need_rows && nr > 0) {
    Data l;
    l.nrows = nr;
    l.cols = {res->cols[0]};
    JoinPairs jp;
    const std::vector<std::pair<int, int>> keys = {{0, sh.x}};
    if (!dense_join(s, l, *la.data, keys, CAPF_JOIN_INNER, jp))
      jp = hash_join(s, l, *la.data, keys, CAPF_JOIN_INNER);
    if (jp.n != nr) fail(CAPF_ERR_INTERNAL, "fused reach: source rows lost");
    IdxCache cache;
    if (jp.left)
      for (auto &c : rcols) c = gather_lazy(s, c, jp.left, nr, false, &cache, jp.iw);
    a_rows = std::make_shared<Data>();
    a_rows->nrows = nr;
    for (size_t j = 0; j < la.data->cols.size(); ++j) {
      const ColPtr &c = la.data->cols[j];
      if (jp.build_unread == 2)  // S_a holds its key and constants only: no row index
        a_rows->cols.push_back((int)j == sh.x ? rcols[0] : const_column(s, c->is_const ? *c : *c->lazy->src, nr));
      else
        a_rows->cols.push_back(jp.right ? gather_lazy(s, c, jp.right, nr, false, &cache, jp.iw) : c);
    }
  }
  for (size_t i = 0; i < gk.size(); ++i) {
    const Type t = grp->types[i];
    if (gk_at[i] < 0) {
      Data e;
      e.nrows = nr;
      out->cols.push_back(eval_program(s, *gk[i].lit, {}, e, t));
      continue;
    }
    const RCol &r = sh.roles[gk_at[i]];
    if (r.role == 2) {  // a literal in every branch (a constant label column)
      Data e;
      e.nrows = nr;
      out->cols.push_back(eval_program(s, r.lit, {}, e, t));
      continue;
    }
    out->cols.push_back(r.col == sh.x ? rcols[0] : a_rows->cols[r.col]);
  }
  for (size_t k = 0; k < grp->aggs.size(); ++k) out->cols.push_back(rcols[1]);
  result = out;
  return true;
}
}  // namespace capf
