// join_graph.h — the plan analysis shared by the fused count (fused_count.hip,
// which defines it) and the fused reach's plan matcher (reach_plan.hip): a lazy
// plan sub-DAG read as leaves joined by column equalities.
#pragma once
#include <utility>
#include <vector>

#include "capf_internal.h"

namespace capf {

struct ColRef {
  int leaf = -1;
  int col = -1;
  bool operator==(const ColRef &o) const { return leaf == o.leaf && col == o.col; }
};

struct Leaf {
  NodePtr node;                   // base plan node (materialisable)
  std::vector<Program> filters;   // single-leaf predicates pushed down (leaf column names)
  std::vector<std::pair<int, int>> col_eqs;  // intra-row equalities (after merges)
};

struct JoinGraph {
  std::vector<Leaf> leaves;
  std::vector<std::pair<ColRef, ColRef>> eqs;
  std::vector<std::pair<ColRef, ColRef>> neqs;
  // literal columns met on the way (withColumns of literals): ColRef{-2, k}
  // refers to lits[k]
  std::vector<Program> lits;
  // pairs of leaves joined on several keys, replaced by one leaf each: their
  // materialised inner join (fused_count.hip contract_pair)
  int pair_joins = 0;
};

struct LeafData {
  DataPtr data;
  bool plain = false;  // unfiltered base data (eligible for column stats / merges)
};

// A tracked column of a plan node: its index, or the literal it was set to.
struct TCol {
  int col = -1;
  const Program *lit = nullptr;
};

// Descends through column-mapping operators (Select; withColumns whose
// expressions are column copies or literals), re-expressing the tracked
// columns; returns the first other node (reach_plan.hip).
NodePtr through_mappings(NodePtr n, std::vector<TCol> &cols);

// The join graph below n and, per column of n, where it comes from; false: an
// operator or key type the fused paths do not read.
bool collect(const NodePtr &n, JoinGraph &g, std::vector<ColRef> &out);
// A leaf's rows: its base node under its pushed-down filters, materialised.
LeafData leaf_data(const Leaf &lf);
// Are the values of column `col` of a (materialisable) base node non-null and
// pairwise distinct?
bool column_unique(const NodePtr &node, int col);

}  // namespace capf
