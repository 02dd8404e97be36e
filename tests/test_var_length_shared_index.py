"""The three fused var-length reach methods on ONE index.

BFS (directed *0|1..u), trails (directed *2..u) and the undirected steps share
the reach index cached on a graph's rel table: the enumeration part (out-CSR,
target mask, source order) is built by whichever of the two enumerations runs
first, the undirected in-adjacency on top of it from that same out-CSR.  A
rel's identity is its out position for both kernels.  These tests run the
methods one after the other on the same graph, in both build orders, and the
undirected steps on a graph whose empty out-rows sit where the search for a
position's row can slip.  Expected values: the host enumerators of
test_var_length_trails.py / test_var_length_undirected.py."""
import functools
import json
import os

import numpy as np
import pytest

from capf_amd.graph import GraphData, ScanGraph

from test_var_length_trails import enumerate_reach, reach_of, sparse_case
from test_var_length_undirected import hub_case, steps_reach

PLAN = {"bfs": "fused_var_length_reach", "trails": "fused_var_length_trails",
        "steps": "fused_var_length_undirected"}
# (method, lower, upper)
FORWARD = [("bfs", 1, 3), ("trails", 2, 3), ("steps", 1, 3), ("steps", 2, 4), ("trails", 2, 3)]
BACKWARD = [("steps", 1, 3), ("steps", 2, 4), ("trails", 2, 3), ("bfs", 1, 3)]


# steps_reach takes a minute on the hub graph at *2..4 (the hub's (x, in) states
# permute its 140 rels), so its answer there is a recorded one; the CPU test
# below recomputes three of its sources.
HUB_STEPS_2_4 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hub_case_steps_2_4.json")


@functools.lru_cache(maxsize=None)
def host_reach(case, method, lower, upper):
    _, src, dst, ids = case()
    if (case, method, lower, upper) == (hub_case, "steps", 2, 4):
        with open(HUB_STEPS_2_4) as f:
            return {int(a): r for a, r in json.load(f)["reach"].items()}
    if method == "steps":
        return steps_reach(src, dst, ids, ids, lower, upper)
    return enumerate_reach(src, dst, ids, ids, lower, upper, trail=method == "trails")


def sparse_96():
    return sparse_case(96, 140, 1, likes=40)


def run_sequence(session, case, sequence):
    g = ScanGraph.from_data(session, case()[0])
    for method, lower, upper in sequence:
        session.reset_profile()
        got = reach_of(g, lower, upper, direction="both" if method == "steps" else "out")
        assert session.last_plan() == PLAN[method], (method, lower, upper)
        assert got == host_reach(case, method, lower, upper), (method, lower, upper)
        assert len(got) > 0


@functools.lru_cache(maxsize=None)
def gap_case():
    """40 nodes (all :Person), 300 rels.  No outgoing rel: the three lowest ids,
    three consecutive ids in the middle, and the highest id — which, like the
    others, has incoming ones.  A sparse skeleton of single rels (where the
    distinct-rel filter bites), three self-loops, and twelve pairs repeated as
    parallel rels up to 300 rows: more than one 256-thread block of out
    positions, rows of 1 to 20-odd entries."""
    n = 40
    ids = [7 * i - 90 for i in range(n)]
    no_out = {0, 1, 2, 18, 19, 20, n - 1}
    outs = [i for i in range(n) if i not in no_out]
    rng = np.random.default_rng(5)
    pairs = []
    for x in outs:
        for _ in range(int(rng.integers(1, 3))):
            pairs.append((x, int(rng.integers(0, n))))
    for y in sorted(no_out):
        pairs.append((outs[int(rng.integers(len(outs)))], y))
    pairs.append((outs[3], n - 1))
    for x in (outs[0], outs[10], outs[-1]):
        pairs.append((x, x))
    rels = list(pairs)
    heavy = [pairs[int(i)] for i in rng.choice(len(pairs), 12, replace=False)]
    k = 0
    while len(rels) < 300:
        rels.append(heavy[k % len(heavy)])
        k += 1
    rels = [rels[int(i)] for i in rng.permutation(len(rels))]
    src, dst = tuple(ids[s] for s, _ in rels), tuple(ids[d] for _, d in rels)
    data = GraphData([(i, frozenset(["Person"]), {}) for i in ids],
                     [(10 ** 6 + k, s, d, "KNOWS", {}) for k, (s, d) in enumerate(zip(src, dst))])
    return data, src, dst, tuple(ids)


GAP_BOUNDS = [(1, 2), (1, 3), (2, 3)]


# ------------------------------------------------------------------- CPU
def test_gap_case_shape_and_answers_are_non_trivial():
    _, src, dst, ids = gap_case()
    assert len(ids) == 40 and len(src) == 300 > 256
    has_out, has_in = set(src), set(dst)
    empty = [i for i, x in enumerate(ids) if x not in has_out]
    assert empty == [0, 1, 2, 18, 19, 20, 39]
    assert all(ids[i] in has_in for i in empty)
    assert any(s == d for s, d in zip(src, dst))                      # self-loops
    assert len(set(zip(src, dst))) < len(src)                         # parallel rels
    for lower, upper in GAP_BOUNDS:
        e = host_reach(gap_case, "steps", lower, upper)
        w = steps_reach(src, dst, ids, ids, lower, upper, distinct_rels=False)
        changed = [a for a in ids if e.get(a) != w.get(a)]
        print(lower, upper, sorted(set(e.values())), len(changed))
        assert len(set(e.values())) > 3 and max(e.values()) < len(ids)
        assert changed
        # the nodes without outgoing rels are sources too: their first hop is inbound
        assert all(ids[i] in e for i in empty)
    assert host_reach(gap_case, "steps", 1, 2) != host_reach(gap_case, "steps", 1, 3)


def test_recorded_hub_answer_is_the_enumerators():
    _, src, dst, ids = hub_case()
    rec = host_reach(hub_case, "steps", 2, 4)
    assert set(rec) <= set(ids) and len(rec) == 134
    some = [0, 1000, 2065]  # the hub, an out-leaf, an in-leaf
    assert steps_reach(src, dst, some, ids, 2, 4) == {a: rec[a] for a in some}


# ------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", [sparse_96, hub_case], ids=["sparse", "hub"])
@pytest.mark.parametrize("sequence", [FORWARD, BACKWARD], ids=["bfs_first", "undirected_first"])
def test_every_method_on_one_index(gpu_session, case, sequence):
    """BFS, trails and undirected steps on one graph's index, the enumeration
    part built by the trails first or by the undirected steps first; the hub
    graph adds rows spread over the waves of a workgroup."""
    run_sequence(gpu_session, case, sequence)


@pytest.mark.gpu
@pytest.mark.parametrize("lower,upper", GAP_BOUNDS)
@pytest.mark.parametrize("compact", [False, True], ids=["int64", "for32"])
def test_steps_with_empty_out_rows(gpu_session, lower, upper, compact):
    g = ScanGraph.from_data(gpu_session, gap_case()[0], compact=compact)
    gpu_session.reset_profile()
    got = reach_of(g, lower, upper, direction="both")
    assert gpu_session.last_plan() == PLAN["steps"]
    assert got == host_reach(gap_case, "steps", lower, upper)
