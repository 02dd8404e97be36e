"""Fused var-length reach with lower bound ≥ 2 (directed, 2 ≤ l ≤ u ≤ 4).

From lower bound 2 on the DISTINCT (a, b) pairs of the relational lowering
(join chain with all NOT(e_i = e_j) filters, UNION ALL, DISTINCT, GROUP BY)
are the pairs joined by a TRAIL — a path whose relationships are pairwise
distinct — not by a walk.  The runtime recognises the shape
(reach_plan.hip::try_fused_reach) and enumerates the trails per source
(var_length_reach.hip::k_vt_trails).  Expected values: a plain-Python trail
enumerator, itself checked against the relational lowering on the CPU oracle.
The graphs are sparse, with self-loops and parallel rels: on the dense R-MAT
graphs of test_var_length_reach.py trail pairs and walk pairs coincide, so
they could not tell this feature from a walk-based one."""
import functools

import numpy as np
import pytest

from capf_amd.expr import CountStar, Var
from capf_amd.graph import GraphData, ScanGraph
from capf_amd.planner import Match, NodeP, Query, RelP, Stage, run

BOUNDS = [(2, 2), (2, 3), (3, 3), (2, 4), (4, 4)]


def sparse(n, m, seed, loops=2, dups=2, person_frac=0.75):
    rng = np.random.default_rng(seed)
    ids = (np.arange(n, dtype=np.int64) - n // 2) * 1000003 + 65
    src = rng.integers(0, n, m)
    dst = rng.integers(0, n, m)
    src[:loops] = dst[:loops]                                   # self-loops
    src[loops:loops + dups] = src[-dups:]                       # parallel rels
    dst[loops:loops + dups] = dst[-dups:]
    person = rng.random(n) < person_frac
    return ids, src, dst, person


def enumerate_reach(src, dst, sources, targets, lower, upper, trail=True):
    """{a: #targets ending a trail (trail=False: a walk) of length lower..upper
    from a}, sources without one left out.  Rel k is (src[k], dst[k])."""
    adj = {}
    for k, (s, d) in enumerate(zip(src, dst)):
        adj.setdefault(s, []).append((k, d))
    tset = set(targets)
    out = {}
    for a in sources:
        ends = set()

        def dfs(x, depth, used):
            for k, y in adj.get(x, ()):
                if trail and k in used:
                    continue
                if depth + 1 >= lower and y in tset:
                    ends.add(y)
                if depth + 1 < upper:
                    dfs(y, depth + 1, used | {k})

        dfs(a, 0, frozenset())
        if ends:
            out[a] = len(ends)
    return out


@functools.lru_cache(maxsize=None)
def sparse_case(n, m, seed, likes=0):
    """(GraphData, KNOWS src ids, KNOWS dst ids, Person ids) of sparse(n, m,
    seed): Person / Other labels, KNOWS rels and `likes` rels of a second type
    that the pattern must ignore."""
    ids, src, dst, person = sparse(n, m, seed)
    nodes = [(int(ids[i]), frozenset(["Person" if person[i] else "Other"]), {}) for i in range(n)]
    ks, kd = [int(v) for v in ids[src]], [int(v) for v in ids[dst]]
    rels = [(10 ** 12 + k, s, d, "KNOWS", {}) for k, (s, d) in enumerate(zip(ks, kd))]
    rng = np.random.default_rng(seed + 100)
    for k in range(likes):
        rels.append((2 * 10 ** 12 + k, int(ids[rng.integers(0, n)]), int(ids[rng.integers(0, n)]), "LIKES", {}))
    return GraphData(nodes, rels), tuple(ks), tuple(kd), tuple(int(v) for v in ids[person])


@functools.lru_cache(maxsize=None)
def expected(n, m, seed, lower, upper, trail=True):
    _, ks, kd, persons = sparse_case(n, m, seed)
    return enumerate_reach(ks, kd, persons, persons, lower, upper, trail)


def reach_query(lower, upper, direction="out", by="a"):
    return Query([Match([NodeP("a", ("Person",)), NodeP("b", ("Person",))],
                        [RelP("k", "a", "b", ("KNOWS",), direction=direction, length=(lower, upper))])],
                 [Stage([("a", Var("a")), ("b", Var("b"))], distinct=True),
                  Stage([(by, Var(by)), ("reach", CountStar())])])


def reach_of(graph, lower, upper, direction="out", by="a"):
    return {r[by]: r["reach"] for r in run(graph, reach_query(lower, upper, direction, by))}


# hand-made graphs, every node :Person; a = 10, b = 20; the answers of the
# relational lowering per (lower, upper), written out
A, B = 10, 20
HAND = {
    # a→b, b→a: the walk a→b→a→b is no trail, so *3..3 is empty and (a, b) never appears
    "two_cycle": ([A, B], [(A, B), (B, A)],
                  {(2, 2): {A: 1, B: 1}, (2, 3): {A: 1, B: 1}, (3, 3): {}}),
    # one self-loop on a, and a→b: loop then a→b is the only 2-trail
    "one_loop": ([A, B], [(A, A), (A, B)],
                 {(2, 2): {A: 1}, (2, 3): {A: 1}, (3, 3): {}}),
    # two self-loops on a: one after the other, never one twice
    "two_loops": ([A], [(A, A), (A, A)],
                  {(2, 2): {A: 1}, (2, 3): {A: 1}, (3, 3): {}, (2, 4): {A: 1}}),
    # a⇒b twice and b→a: a→b→a→b over the two parallel rels is a trail
    "parallel": ([A, B], [(A, B), (A, B), (B, A)],
                 {(2, 2): {A: 1, B: 1}, (3, 3): {A: 1}, (2, 3): {A: 2, B: 1}, (2, 4): {A: 2, B: 1}}),
}
HAND_CASES = [(name, b) for name, (_, _, exp) in HAND.items() for b in exp]


def hand_graph(name):
    ids, rels, _ = HAND[name]
    return GraphData([(i, frozenset(["Person"]), {}) for i in ids],
                     [(100 + k, s, d, "KNOWS", {}) for k, (s, d) in enumerate(rels)])


def hub_case():
    """A hub with rows longer than a wave and more first hops than waves: 150
    out-rels and 150 in-rels to distinct leaves, three self-loops, 70 parallel
    rels to one leaf that has one rel back.  (Its trail and walk COUNTS agree:
    this graph is about the kernel's loops over long rows, not the semantics.)"""
    hub, leaf = 0, 1
    src, dst = [], []
    for i in range(150):
        src.append(hub), dst.append(1000 + i)
    for i in range(150):
        src.append(2000 + i), dst.append(hub)
    for _ in range(3):
        src.append(hub), dst.append(hub)
    for _ in range(70):
        src.append(hub), dst.append(leaf)
    src.append(leaf), dst.append(hub)
    ids = sorted(set(src) | set(dst))
    data = GraphData([(i, frozenset(["Person"]), {}) for i in ids],
                     [(10 ** 6 + k, s, d, "KNOWS", {}) for k, (s, d) in enumerate(zip(src, dst))])
    return data, src, dst, ids


# ------------------------------------------------------------------- CPU
@pytest.mark.parametrize("lower,upper", BOUNDS)
def test_enumerator_equals_relational_on_oracle(lower, upper):
    from oracle.table_np import OracleSession
    data, *_ = sparse_case(24, 30, 1)
    got = reach_of(ScanGraph.from_data(OracleSession(), data), lower, upper)
    assert got == expected(24, 30, 1, lower, upper)


@pytest.mark.parametrize("name,bounds", HAND_CASES)
def test_hand_cases_on_oracle(name, bounds):
    from oracle.table_np import OracleSession
    ids, rels, exp = HAND[name]
    got = reach_of(ScanGraph.from_data(OracleSession(), hand_graph(name)), *bounds)
    assert got == exp[bounds]
    src, dst = [s for s, _ in rels], [d for _, d in rels]
    assert enumerate_reach(src, dst, ids, ids, *bounds) == exp[bounds]


@pytest.mark.parametrize("lower,upper", BOUNDS)
def test_sparse_graph_tells_trails_from_walks(lower, upper):
    """sparse(96, 140, 1) discriminates: number of sources whose trail answer
    differs from the walk answer, per bounds."""
    t = expected(96, 140, 1, lower, upper)
    w = expected(96, 140, 1, lower, upper, trail=False)
    differ = sum(1 for a in set(t) | set(w) if t.get(a) != w.get(a))
    assert differ == {(2, 2): 3, (2, 3): 5, (3, 3): 9, (2, 4): 7, (4, 4): 16}[(lower, upper)]


# ------------------------------------------------------------------- GPU
def fused(session, graph, lower, upper, **kw):
    session.reset_profile()
    got = reach_of(graph, lower, upper, **kw)
    assert session.last_plan() == "fused_var_length_trails"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name,bounds", HAND_CASES)
def test_hand_cases(gpu_session, name, bounds):
    g = ScanGraph.from_data(gpu_session, hand_graph(name))
    assert fused(gpu_session, g, *bounds) == HAND[name][2][bounds]


@pytest.mark.gpu
@pytest.mark.parametrize("lower,upper", BOUNDS)
@pytest.mark.parametrize("compact", [False, True], ids=["int64", "for32"])
def test_trails_vs_enumerator(gpu_session, lower, upper, compact):
    exp = expected(96, 140, 1, lower, upper)
    assert exp != expected(96, 140, 1, lower, upper, trail=False)
    data, *_ = sparse_case(96, 140, 1, likes=40)
    g = ScanGraph.from_data(gpu_session, data, compact=compact)
    assert fused(gpu_session, g, lower, upper) == exp


@pytest.mark.gpu
def test_trails_incoming_direction(gpu_session):
    """(a)<-[:KNOWS*2..3]-(b) grouped by b: trails from b along the rels."""
    exp = expected(96, 140, 1, 2, 3)
    assert exp != expected(96, 140, 1, 2, 3, trail=False)
    data, *_ = sparse_case(96, 140, 1, likes=40)
    g = ScanGraph.from_data(gpu_session, data)
    assert fused(gpu_session, g, 2, 3, direction="in", by="b") == exp


@pytest.mark.gpu
@pytest.mark.parametrize("lower,upper", [(2, 3), (2, 4)])
def test_trails_many_workgroups(gpu_session, lower, upper):
    """5003 nodes: thousands of workgroups and a bitmap whose last word is partial."""
    exp = expected(5003, 7000, 2, lower, upper)
    assert exp != expected(5003, 7000, 2, lower, upper, trail=False)
    data, *_ = sparse_case(5003, 7000, 2)
    g = ScanGraph.from_data(gpu_session, data)
    assert fused(gpu_session, g, lower, upper) == exp


@pytest.mark.gpu
@pytest.mark.parametrize("lower,upper", [(2, 2), (2, 3), (3, 3)])
def test_trails_hub_rows(gpu_session, lower, upper):
    data, src, dst, ids = hub_case()
    exp = enumerate_reach(src, dst, ids, ids, lower, upper)
    g = ScanGraph.from_data(gpu_session, data)
    assert fused(gpu_session, g, lower, upper) == exp


@pytest.mark.gpu
@pytest.mark.parametrize("lower,upper", BOUNDS)
def test_trails_without_expanded_rows(gpu_session, monkeypatch, lower, upper):
    """CAPF_VT_EXPAND=0: the kernel as it runs when two bitmaps do not fit the
    LDS (every last-level row per trail, no expanded-rows bitmap)."""
    monkeypatch.setenv("CAPF_VT_EXPAND", "0")
    data, *_ = sparse_case(96, 140, 1, likes=40)
    g = ScanGraph.from_data(gpu_session, data)
    assert fused(gpu_session, g, lower, upper) == expected(96, 140, 1, lower, upper)
    if upper <= 3:
        data, src, dst, ids = hub_case()
        g = ScanGraph.from_data(gpu_session, data)
        assert fused(gpu_session, g, lower, upper) == enumerate_reach(src, dst, ids, ids, lower, upper)


@pytest.mark.gpu
@pytest.mark.parametrize("scale,lower,upper", [(8, 2, 3), (8, 3, 3), (6, 2, 4)])
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
def test_fallback_above_node_limit(gpu_session, monkeypatch):
    """A dictionary above the kernel's node limit runs the relational plan."""
    data, *_ = sparse_case(96, 140, 1, likes=40)
    g = ScanGraph.from_data(gpu_session, data)
    monkeypatch.setenv("CAPF_VT_MAX_NODES", "16")
    gpu_session.reset_profile()
    got = reach_of(g, 2, 3)
    assert gpu_session.last_plan() == "none"
    assert got == expected(96, 140, 1, 2, 3)


@pytest.mark.gpu
def test_fallback_upper_above_four(gpu_session):
    data, ks, kd, persons = sparse_case(24, 30, 1)
    g = ScanGraph.from_data(gpu_session, data)
    gpu_session.reset_profile()
    got = reach_of(g, 2, 5)
    assert gpu_session.last_plan() == "none"
    assert got == enumerate_reach(ks, kd, persons, persons, 2, 5)


def _abi_tables(session):
    from capf_amd.expr import T_INT
    _, ks, kd, persons = sparse_case(96, 140, 1)
    rels = session.table([("s", T_INT, np.array(ks, dtype=np.int64), None),
                          ("t", T_INT, np.array(kd, dtype=np.int64), None)])
    nodes = session.table([("id", T_INT, np.array(persons, dtype=np.int64), None)])
    return rels, nodes


@pytest.mark.gpu
def test_c_abi_trails(gpu_session):
    rels, nodes = _abi_tables(gpu_session)
    t = gpu_session.var_length_reach(rels, "s", "t", nodes, "id", nodes, "id", 2, 3, "a", "reach")
    assert {r["a"]: r["reach"] for r in t.rows} == expected(96, 140, 1, 2, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("lower,upper", [(2, 5), (3, 2)])
def test_c_abi_other_bounds_raise(gpu_session, lower, upper):
    from capf_amd._lib import NotImplementedException
    rels, nodes = _abi_tables(gpu_session)
    with pytest.raises(NotImplementedException):
        gpu_session.var_length_reach(rels, "s", "t", nodes, "id", nodes, "id", lower, upper, "a", "reach")


@pytest.mark.gpu
@pytest.mark.parametrize("lower", [1, 0])
def test_walk_bounds_keep_their_plan(gpu_session, lower):
    """*1..3 and *0..3 stay on the BFS and neither build nor run the trail part."""
    from test_var_length_reach import synthetic
    data, *_ = synthetic(6)
    g = ScanGraph.from_data(gpu_session, data)
    gpu_session.reset_profile()
    gpu_session.set_profiling(True)
    try:
        got = reach_of(g, lower, 3)
    finally:
        gpu_session.set_profiling(False)
    assert gpu_session.last_plan() == "fused_var_length_reach"
    assert len(got) > 0
    prof = gpu_session.profile()
    assert any(k.startswith("vr_") for k in prof)
    assert not any(k.startswith("vt_") for k in prof)
