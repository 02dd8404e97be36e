"""Fused undirected var-length reach, (a)-[:KNOWS*l..u]-(b), 0 ≤ l ≤ u ≤ 4.

The undirected lowering (planner.py::var_length_expand, VarLengthExpandPlanner
.scala:277-307) is an automaton over states (node x, mode out | in) that
starts at (a, out); a rel e not yet on the path leads

    (x, out), start(e) = x → (end(e), out)      (x, in), start(e) = x → (x, in)
    (x, out), end(e) = x → (start(e), in)       (x, in), end(e) = x → (x, out)

and a state of depth max(l, 1)..u pairs a with its node.  That is neither the
trails of the symmetrised graph nor any walk, so the expected values come
from `steps_reach`, a plain-Python enumerator of the automaton that the CPU
tests tie to the relational lowering on the oracle.  The runtime recognises
the shape (reach_plan.hip::try_fused_reach, unions hoisted over the joins)
and enumerates the steps per source (var_length_reach.hip::k_vu_steps)."""
import functools

import numpy as np
import pytest

from capf_amd.graph import GraphData, ScanGraph
from capf_amd.planner import run

from test_var_length_trails import HAND, enumerate_reach, hand_graph, reach_query, sparse_case

BOUNDS = [(1, 1), (1, 2), (1, 3), (0, 2), (0, 3), (2, 2), (2, 3), (3, 3), (1, 4), (2, 4), (4, 4)]
HAND_BOUNDS = [(1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3), (0, 1), (2, 4)]
# the relational lowering's answers on the oracle, written out
HAND_EXPECTED = {
    ("two_cycle", (1, 2)): {10: 2, 20: 2},
    ("two_cycle", (3, 3)): {},
    ("one_loop", (1, 1)): {10: 2, 20: 1},
    ("one_loop", (0, 1)): {10: 2, 20: 2},
    ("two_loops", (2, 3)): {10: 1},
    ("two_loops", (3, 3)): {},
    ("parallel", (3, 3)): {10: 2, 20: 2},
}


def steps_reach(src, dst, sources, targets, lower, upper, distinct_rels=True):
    """{a: #targets on a state of depth max(lower, 1)..upper of the automaton
    from (a, out)} (+ a itself from lower bound 0), sources without one left
    out.  Rel k is (src[k], dst[k])."""
    outs, ins = {}, {}
    for k, (s, d) in enumerate(zip(src, dst)):
        outs.setdefault(s, []).append((k, d))
        ins.setdefault(d, []).append((k, s))
    tset = set(targets)
    res = {}
    for a in sources:
        ends = set()
        if lower == 0 and a in tset:
            ends.add(a)

        def step(x, mode, depth, used):
            for k, y in outs.get(x, ()):          # start(e) = x
                if not (distinct_rels and k in used):
                    visit((y, "out") if mode == "out" else (x, "in"), depth + 1, used | {k})
            for k, y in ins.get(x, ()):           # end(e) = x
                if not (distinct_rels and k in used):
                    visit((y, "in") if mode == "out" else (x, "out"), depth + 1, used | {k})

        def visit(state, depth, used):
            if depth >= max(lower, 1) and state[0] in tset:
                ends.add(state[0])
            if depth < upper:
                step(state[0], state[1], depth, used)

        step(a, "out", 0, frozenset())
        if ends:
            res[a] = len(ends)
    return res


def true_trails(src, dst, sources, targets, lower, upper):
    """Textbook undirected trails: symmetrised adjacency, pairwise distinct rels."""
    adj = {}
    for k, (s, d) in enumerate(zip(src, dst)):
        adj.setdefault(s, []).append((k, d))
        if s != d:
            adj.setdefault(d, []).append((k, s))
    tset = set(targets)
    out = {}
    for a in sources:
        ends = set()
        if lower == 0 and a in tset:
            ends.add(a)

        def dfs(x, depth, used):
            for k, y in adj.get(x, ()):
                if k in used:
                    continue
                if depth + 1 >= max(lower, 1) and y in tset:
                    ends.add(y)
                if depth + 1 < upper:
                    dfs(y, depth + 1, used | {k})

        dfs(a, 0, frozenset())
        if ends:
            out[a] = len(ends)
    return out


@functools.lru_cache(maxsize=None)
def expected(n, m, seed, lower, upper):
    _, ks, kd, persons = sparse_case(n, m, seed)
    return steps_reach(ks, kd, persons, persons, lower, upper)


def hand_expected(name, bounds):
    ids, rels, _ = HAND[name]
    got = steps_reach([s for s, _ in rels], [d for _, d in rels], ids, ids, *bounds)
    if (name, bounds) in HAND_EXPECTED:
        assert got == HAND_EXPECTED[(name, bounds)]
    return got


def reach_of(graph, lower, upper):
    return {r["a"]: r["reach"] for r in run(graph, reach_query(lower, upper, direction="both"))}


def differing(p, q):
    return sum(1 for a in set(p) | set(q) if p.get(a) != q.get(a))


@functools.lru_cache(maxsize=None)
def hub_case():
    """A hub with 66 out-rels and 66 in-rels to distinct leaves, 2 self-loops,
    3 parallel rels to one leaf and one rel back: an out-row of 71 and an
    in-row of 69 entries (each longer than a wave), 140 first hops (more than
    the workgroup's waves)."""
    hub, leaf = 0, 1
    src, dst = [], []
    for i in range(66):
        src.append(hub), dst.append(1000 + i)
    for i in range(66):
        src.append(2000 + i), dst.append(hub)
    for _ in range(2):
        src.append(hub), dst.append(hub)
    for _ in range(3):
        src.append(hub), dst.append(leaf)
    src.append(leaf), dst.append(hub)
    ids = sorted(set(src) | set(dst))
    data = GraphData([(i, frozenset(["Person"]), {}) for i in ids],
                     [(10 ** 6 + k, s, d, "KNOWS", {}) for k, (s, d) in enumerate(zip(src, dst))])
    return data, tuple(src), tuple(dst), tuple(ids)


# ------------------------------------------------------------------- CPU
@pytest.mark.parametrize("lower,upper", BOUNDS)
def test_enumerator_equals_relational_on_oracle(lower, upper):
    from oracle.table_np import OracleSession
    data, *_ = sparse_case(24, 30, 1)
    got = reach_of(ScanGraph.from_data(OracleSession(), data), lower, upper)
    assert got == expected(24, 30, 1, lower, upper) and len(got) > 0


@pytest.mark.parametrize("bounds", HAND_BOUNDS)
@pytest.mark.parametrize("name", list(HAND))
def test_hand_cases_on_oracle(name, bounds):
    from oracle.table_np import OracleSession
    got = reach_of(ScanGraph.from_data(OracleSession(), hand_graph(name)), *bounds)
    assert got == hand_expected(name, bounds)


def test_written_out_hand_values_are_all_checked():
    for name, bounds in HAND_EXPECTED:
        assert name in HAND and bounds in HAND_BOUNDS


# sources of sparse(96, 140, 1) whose answer differs from (true undirected
# trails, the automaton without the distinct-rel filter, directed trails)
DIFFER = {
    (1, 2): (45, 47, 60), (1, 3): (60, 54, 63), (0, 2): (45, 0, 71), (0, 3): (60, 20, 72),
    (2, 2): (45, 47, 60), (2, 3): (61, 58, 63), (3, 3): (60, 62, 63),
    (1, 4): (63, 52, 64), (2, 4): (63, 55, 63), (4, 4): (63, 62, 62),
}
# *0..2 is the one bound where dropping the distinct-rel filter changes nothing:
# all it adds at length 2 is a itself (a rel taken there and back), which lower
# bound 0 pairs with a anyway.  The other two comparisons still differ there.
SAME_WITHOUT_FILTER = {(0, 2)}


@pytest.mark.parametrize("lower,upper", [b for b in BOUNDS if b[1] >= 2])
def test_sparse_graph_tells_the_lowering_from_its_neighbours(lower, upper):
    """sparse(96, 140, 1) discriminates: an implementation that symmetrises the
    CSR and walks trails, one that drops the distinct-rel filter (a BFS), and
    the directed enumeration each give other answers at every bound."""
    _, ks, kd, persons = sparse_case(96, 140, 1)
    e = expected(96, 140, 1, lower, upper)
    t = true_trails(ks, kd, persons, persons, lower, upper)
    w = steps_reach(ks, kd, persons, persons, lower, upper, distinct_rels=False)
    d = enumerate_reach(ks, kd, persons, persons, max(lower, 1), upper)
    got = (differing(e, t), differing(e, w), differing(e, d))
    print(lower, upper, got)
    assert got == DIFFER[(lower, upper)]
    assert got[0] > 0 and got[2] > 0 and (got[1] > 0) == ((lower, upper) not in SAME_WITHOUT_FILTER)


# ------------------------------------------------------------------- GPU
def fused(session, graph, lower, upper):
    session.reset_profile()
    got = reach_of(graph, lower, upper)
    assert session.last_plan() == "fused_var_length_undirected"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("bounds", HAND_BOUNDS)
@pytest.mark.parametrize("name", list(HAND))
def test_hand_cases(gpu_session, name, bounds):
    g = ScanGraph.from_data(gpu_session, hand_graph(name))
    assert fused(gpu_session, g, *bounds) == hand_expected(name, bounds)


@pytest.mark.gpu
@pytest.mark.parametrize("lower,upper", BOUNDS)
@pytest.mark.parametrize("compact", [False, True], ids=["int64", "for32"])
def test_steps_vs_enumerator(gpu_session, lower, upper, compact):
    data, *_ = sparse_case(96, 140, 1, likes=40)
    g = ScanGraph.from_data(gpu_session, data, compact=compact)
    assert fused(gpu_session, g, lower, upper) == expected(96, 140, 1, lower, upper)


@pytest.mark.gpu
@pytest.mark.parametrize("lower,upper", [(1, 3), (2, 4), (0, 2)])
def test_steps_many_workgroups(gpu_session, lower, upper):
    """5003 nodes: thousands of workgroups and a bitmap whose last word is partial."""
    data, *_ = sparse_case(5003, 7000, 2)
    g = ScanGraph.from_data(gpu_session, data)
    assert fused(gpu_session, g, lower, upper) == expected(5003, 7000, 2, lower, upper)


@pytest.mark.gpu
@pytest.mark.parametrize("lower,upper", [(1, 2), (1, 3), (2, 3)])
def test_steps_hub_rows(gpu_session, lower, upper):
    data, src, dst, ids = hub_case()
    g = ScanGraph.from_data(gpu_session, data)
    assert fused(gpu_session, g, lower, upper) == steps_reach(src, dst, ids, ids, lower, upper)


@pytest.mark.gpu
@pytest.mark.parametrize("scale,lower,upper", [(6, 1, 3), (6, 2, 3), (4, 2, 4)])
def test_fused_equals_relational_plan(gpu_session, monkeypatch, scale, lower, upper):
    """Row for row against the join chain on the GPU, on the dense graphs."""
    from test_var_length_reach import synthetic
    data, *_ = synthetic(scale)
    g = ScanGraph.from_data(gpu_session, data)
    got = fused(gpu_session, g, lower, upper)
    monkeypatch.setenv("CAPF_FUSED_REACH", "0")
    gpu_session.reset_profile()
    plain = reach_of(g, lower, upper)
    assert gpu_session.last_plan() == "none"
    assert got == plain and len(plain) > 0


@pytest.mark.gpu
def test_fallback_upper_above_four(gpu_session):
    data, ks, kd, persons = sparse_case(24, 30, 1)
    g = ScanGraph.from_data(gpu_session, data)
    gpu_session.reset_profile()
    got = reach_of(g, 2, 5)
    assert gpu_session.last_plan() == "none"
    assert got == steps_reach(ks, kd, persons, persons, 2, 5)


@pytest.mark.gpu
def test_fallback_above_node_limit(gpu_session, monkeypatch):
    """A dictionary above the kernel's node limit runs the relational plan."""
    data, *_ = sparse_case(24, 30, 1)
    g = ScanGraph.from_data(gpu_session, data)
    monkeypatch.setenv("CAPF_VT_MAX_NODES", "16")
    gpu_session.reset_profile()
    got = reach_of(g, 1, 3)
    assert gpu_session.last_plan() == "none"
    assert got == expected(24, 30, 1, 1, 3)


def _abi_tables(session):
    from capf_amd.expr import T_INT
    _, ks, kd, persons = sparse_case(96, 140, 1)
    rels = session.table([("s", T_INT, np.array(ks, dtype=np.int64), None),
                          ("t", T_INT, np.array(kd, dtype=np.int64), None)])
    nodes = session.table([("id", T_INT, np.array(persons, dtype=np.int64), None)])
    return rels, nodes


@pytest.mark.gpu
def test_c_abi_undirected(gpu_session):
    rels, nodes = _abi_tables(gpu_session)
    t = gpu_session.var_length_reach_undirected(rels, "s", "t", nodes, "id", nodes, "id", 1, 3, "a", "reach")
    assert {r["a"]: r["reach"] for r in t.rows} == expected(96, 140, 1, 1, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("lower,upper", [(2, 5), (3, 2)])
def test_c_abi_other_bounds_raise(gpu_session, lower, upper):
    from capf_amd._lib import NotImplementedException
    rels, nodes = _abi_tables(gpu_session)
    with pytest.raises(NotImplementedException):
        gpu_session.var_length_reach_undirected(rels, "s", "t", nodes, "id", nodes, "id", lower, upper, "a", "reach")


@pytest.mark.gpu
@pytest.mark.parametrize("lower,plan", [(1, "fused_var_length_reach"), (2, "fused_var_length_trails")])
def test_directed_plans_unchanged(gpu_session, lower, plan):
    """Directed *1..3 and *2..3 keep their plans and run no undirected kernel."""
    data, *_ = sparse_case(96, 140, 1, likes=40)
    g = ScanGraph.from_data(gpu_session, data)
    gpu_session.reset_profile()
    gpu_session.set_profiling(True)
    try:
        got = {r["a"]: r["reach"] for r in run(g, reach_query(lower, 3))}
    finally:
        gpu_session.set_profiling(False)
    assert gpu_session.last_plan() == plan
    _, ks, kd, persons = sparse_case(96, 140, 1)
    assert got == enumerate_reach(ks, kd, persons, persons, lower, 3, trail=lower >= 2)
    assert not any(k.startswith("vu_") for k in gpu_session.profile())
