"""group(keys; count(*)) over an inner-join tree answered without the join
(fused_count.hip try_fused_group_count, DESIGN.md "Grouped count").

Every "answers" case resets the profile, runs the query and asserts
`last_plan() == "message_passing_grouped"`; the rows are compared as multisets
with the oracle (the same planner over numpy tables) and, where stated, with
brute-force enumeration in plain Python that knows nothing of either.  Every
"declines" case asserts the opposite and the oracle's rows.
"""
import functools
import random

import numpy as np
import pytest

from capf_amd.expr import Count, CountStar, ElementProperty, Equals, GreaterThan, IntegerLit, Not, Sum, Var, T_INT
from capf_amd.graph import GraphData, ScanGraph
from capf_amd.header import RecordHeader
from capf_amd.planner import Match, NodeP, Query, RelP, Stage, run
from conftest import bag
from oracle.table_np import OracleSession
from test_message_passing import K, gpu_tables, hub_graph, join_tree, nrows

PLAN = "message_passing_grouped"
C = {"n": CountStar()}


def hdr(*cols):
    return RecordHeader({Var(c): c for c in cols})


def answered(session, make):
    """make()'s rows, answered by the grouped message passing; (rows, detail)."""
    session.reset_profile()
    assert session.last_plan() == "none"
    rows = make().rows
    assert session.last_plan() == PLAN, (session.last_plan(), session.last_plan_detail())
    return rows, session.last_plan_detail()


def declined(session, make):
    session.reset_profile()
    rows = make().rows
    assert session.last_plan() != PLAN, session.last_plan_detail()
    return rows


def oracle_tables(tables):
    o = OracleSession()
    return [o.table([(c, T_INT, [x if ok is None or ok[i] else None for i, x in enumerate(v.tolist())], None)
                     for c, (v, ok) in t.items()], nrows=nrows(t)) for t in tables]


# ------------------------------------------------------------------ 1. shapes
ISOLATED = [100, 205]


@functools.lru_cache(maxsize=None)
def hub_data(seed=31):
    """hub_graph's rels (multi-edges, self-loops — one on the hub, which has 70
    other predecessors — in- and out-degree above 64) over nodes 0..29 and two
    isolated nodes."""
    ids, src, dst = hub_graph(seed)
    nodes = [(int(i), frozenset(["V"]), {}) for i in list(range(30)) + ISOLATED]
    rels = [(int(r), int(s), int(t), "E", {}) for r, s, t in zip(ids, src, dst)]
    return GraphData(nodes, rels), src.tolist(), dst.tolist()


def brute_grouped(src, dst, hops, pos):
    """{node at position `pos` of the path: #paths r1..r_hops of pairwise
    different rels with target(r_i) = source(r_{i+1})}."""
    out_of = {}
    for r, s in enumerate(src):
        out_of.setdefault(s, []).append(r)
    counts = {}

    def extend(path):
        if len(path) == hops:
            nodes = [src[path[0]]] + [dst[r] for r in path]
            counts[nodes[pos]] = counts.get(nodes[pos], 0) + 1
            return
        for r in out_of.get(dst[path[-1]], ()):
            if r not in path:
                extend(path + [r])

    for r in range(len(src)):
        extend([r])
    return counts


def path_query(hops, by, extra_items=()):
    names = "abcd"[:hops + 1]
    return Query([Match([NodeP(v) for v in names], [RelP(f"r{i + 1}", names[i], names[i + 1]) for i in range(hops)])],
                 [Stage([(by, Var(by, "NODE"))] + list(extra_items) + [("n", CountStar())])])


@pytest.mark.gpu
@pytest.mark.parametrize("hops,by", [(1, "a"), (1, "b"), (2, "a"), (2, "b"), (2, "c")])
@pytest.mark.parametrize("compact", [False, True], ids=["int64", "for32"])
def test_paths_grouped_by_a_node(gpu_session, hops, by, compact):
    data, src, dst = hub_data()
    g = ScanGraph.from_data(gpu_session, data, compact=compact)
    q = path_query(hops, by)
    gpu_session.reset_profile()
    rows = run(g, q)
    plan, detail = gpu_session.last_plan(), gpu_session.last_plan_detail()
    print(f"{hops}-hop by {by}: plan {plan} detail {detail!r}")
    assert plan == PLAN, (plan, detail)
    assert detail.endswith(" group:unique") and detail.count("|") == hops - 1
    want = brute_grouped(src, dst, hops, "abcd".index(by))
    assert {r[by].id: r["n"] for r in rows} == want and len(rows) == len(want)
    assert not set(ISOLATED) & set(want)
    assert bag(rows) == bag(run(ScanGraph.from_data(OracleSession(), data), q))
    if hops == 2 and by == "a":
        # the r1 = r2 term (the hub's self-loop) subtracts from the hub's row alone
        walks = brute_walks2(src, dst)
        assert want[0] == walks[0] - sum(1 for s, t in zip(src, dst) if s == t == 0) and walks[0] != want[0]


@pytest.mark.gpu
@pytest.mark.parametrize("enc", [None, 4], ids=["int64", "for32"])
def test_three_hops_grouped_by_a(gpu_session, enc):
    """a ⋈ r1 ⋈ r2 ⋈ r3 ⋈ d with 3 uniqueness filters: 8 terms, the r1 = r3
    term a pair_join (the 2-cycles), every term rooted at a's scan."""
    from test_message_passing import rel_chain
    ids, src, dst = hub_graph(31)
    tables = [{"id": K(ids), "s": K(src), "t": K(dst)}, {"id": K(np.concatenate([np.arange(30), ISOLATED]))}]
    joins = [("t", "s"), ("t", "s")]

    def make(tabs):
        return rel_chain(tabs[0], joins, 3, tabs[1]).group([Var("na")], C, header=hdr("na"))

    rows, detail = answered(gpu_session, lambda: make(gpu_tables(gpu_session, tables, enc)))
    print(f"3-hop by a: detail {detail!r}")
    terms = detail.split("|")
    assert len(terms) == 8 and ["pair_join" in t.split() for t in terms] == [m == 2 for m in range(8)]
    assert detail.endswith(" group:unique") and all("rows" in t for t in terms)
    want = brute_grouped(src.tolist(), dst.tolist(), 3, 0)
    assert {r["na"]: r["n"] for r in rows} == want and len(rows) == len(want) > 3
    assert bag(rows) == bag(make(oracle_tables(tables)).rows)


def brute_walks2(src, dst):
    outdeg = {}
    for s in src:
        outdeg[s] = outdeg.get(s, 0) + 1
    w = {}
    for s, t in zip(src, dst):
        w[s] = w.get(s, 0) + outdeg.get(t, 0)
    return w


# ------------------------------------------------------------------ 2. kernel edges
def one_child(session, root, child, enc=None, by=("tag",)):
    """root(rk, tag) ⋈ child(sk) grouped by root columns: (gpu rows, detail,
    expected {tag: weight}) — tag is the root's row number."""
    tables = [{"rk": root, "tag": K(np.arange(len(root[0])))}, {"sk": child}]
    tabs = gpu_tables(session, tables, enc)
    rows, detail = answered(session, lambda: tabs[0].join(tabs[1], "inner", ("rk", "sk")).group(
        [Var(c) for c in by], C, header=hdr("rk", "tag", "sk")))
    cnt = {}
    cv, cok = child
    for i, x in enumerate(cv.tolist()):
        if cok is None or cok[i]:
            cnt[x] = cnt.get(x, 0) + 1
    rv, rok = root
    want = {i: cnt.get(x, 0) for i, x in enumerate(rv.tolist()) if (rok is None or rok[i]) and cnt.get(x, 0)}
    return rows, detail, want


@pytest.mark.gpu
@pytest.mark.parametrize("enc", [None, 4, 3], ids=["int64", "for32", "for24"])
@pytest.mark.parametrize("child", ["bits", "dense"])
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 257])
def test_root_sizes_and_key_widths(gpu_session, n, child, enc):
    """Root leaves around the wave size and the 4-row vector width, keys as
    int64 / FOR32 / FOR24; a 0/1 child (rows1) and a counted child (rows:1)."""
    rng = np.random.default_rng(1000 * n + (enc or 0))
    send = 3 * np.arange(400, dtype=np.int64) + 7
    if child == "dense":
        send = np.concatenate([send[:150], send[100:150], send[140:150]])
    hit = 3 * 145 + 7  # in the child three times over when it is `dense`
    root = rng.integers(0, 1300, n).astype(np.int64)
    root[max(0, n - 7):] = hit  # the ragged tail hits; every size > 0 holds the repeated key
    if n > 1:
        root[0] = 1299  # outside the child's keys
    rows, detail, want = one_child(gpu_session, K(root), K(rng.permutation(send)), enc)
    w = {None: 8, 4: 4, 3: 3}[enc]
    # no root row: the empty map, dropped over no rows (test_message_passing.test_empty_message)
    expect = "empty rows_all" if n == 0 else f"bits rows1:bits:w{w}" if child == "bits" else "dense rows:1"
    assert detail.replace("bits_cached", "bits") == expect + " group:unique", detail
    assert n == 0 or want[n - 1] == (3 if child == "dense" else 1)
    assert {r["tag"]: r["n"] for r in rows} == want and len(rows) == len(want)
    assert [r["tag"] for r in rows] == sorted(want)  # G's row order


@pytest.mark.gpu
def test_every_weight_zero(gpu_session, monkeypatch):
    """An empty rel table: no group at all, with the generic path's columns and types."""
    tables = [{"id": K(np.arange(40))}, {"s": K([]), "t": K([])}]
    tabs = gpu_tables(gpu_session, tables)
    make = lambda: tabs[0].join(tabs[1], "inner", ("id", "s")).group([Var("id")], C, header=hdr("id", "s", "t"))  # noqa: E731
    t = make()
    rows, detail = answered(gpu_session, lambda: t)
    assert rows == [] and t.size == 0
    cols, types = t.physicalColumns, t.columnType
    monkeypatch.setenv("CAPF_FUSED_GROUP", "0")
    u = make()
    assert declined(gpu_session, lambda: u) == []
    assert (u.physicalColumns, u.columnType) == (cols, types)
    assert cols == ["id", "n"]


@pytest.mark.gpu
def test_nullable_root_join_key(gpu_session):
    rng = np.random.default_rng(7)
    root = rng.integers(0, 60, 300).astype(np.int64)
    nulls = rng.random(300) < 0.25
    nulls[[0, 63, 64, 299]] = True
    send = rng.integers(0, 50, 200).astype(np.int64)
    rows, detail, want = one_child(gpu_session, K(root, nulls), K(send, rng.random(200) < 0.1))
    assert detail == "dense rows:1 group:unique", detail
    assert {r["tag"]: r["n"] for r in rows} == want and 0 < len(want) < 300 - nulls.sum() + 1


@pytest.mark.gpu
@pytest.mark.parametrize("child", ["bits", "dense"])
def test_root_above_the_grid_cap(gpu_session, child):
    """2^20 + 257 root rows against one child: more rows than the capped grid
    of the row-per-thread kernel has threads (rows:1), and the vector kernel's
    two groups in flight (rows1)."""
    n = (1 << 20) + 257
    rng = np.random.default_rng(11)
    root = rng.integers(0, 3000, n).astype(np.int64)
    send = 3 * np.arange(700, dtype=np.int64) + 5
    if child == "dense":
        send = np.concatenate([send, send[::2]])
    tabs = gpu_tables(gpu_session, [{"rk": K(root), "tag": K(np.arange(n))}, {"sk": K(rng.permutation(send))}], 4)
    t = tabs[0].join(tabs[1], "inner", ("rk", "sk")).group([Var("tag")], C, header=hdr("rk", "tag", "sk"))
    gpu_session.reset_profile()
    tags = np.array(t.column_values("tag"), dtype=np.int64)
    ns = np.array(t.column_values("n"), dtype=np.int64)
    assert gpu_session.last_plan() == PLAN
    assert gpu_session.last_plan_detail().replace("bits_cached", "bits") == \
        ("bits rows1:bits:w4" if child == "bits" else "dense rows:1") + " group:unique"
    hit = (root % 3 == 2) & (root >= 5) & (root <= 3 * 699 + 5)
    assert np.array_equal(tags, np.flatnonzero(hit))
    assert np.array_equal(ns, np.where((root[hit] - 5) % 6 == 0, 2, 1) if child == "dense" else np.ones(hit.sum()))
    assert hit[-257:].any() and hit[: 1 << 20].any()


@pytest.mark.gpu
def test_group_count_above_two_to_the_32(gpu_session):
    """65 537 parallel rels a→h and 65 537 rels h→x_i: 65 537² 2-paths from a."""
    k = 65537
    a, h = 1, 2
    src = np.concatenate([np.full(k, a), np.full(k, h)]).astype(np.int64)
    dst = np.concatenate([np.full(k, h), 10 + np.arange(k)]).astype(np.int64)
    rels, nodes = gpu_tables(gpu_session, [{"id": K(np.arange(2 * k)), "s": K(src), "t": K(dst)},
                                           {"id": K(np.concatenate([[a, h], 10 + np.arange(k)]))}])

    def make():
        r0, r1 = (rels.select(("id", f"i{j}"), ("s", f"s{j}"), ("t", f"t{j}")) for j in range(2))
        na = nodes.select(("id", "a"))
        cur = na.join(r0, "inner", ("a", "s0")).join(r1, "inner", ("t0", "s1"))
        cur = cur.filter(Not(Equals(Var("i0"), Var("i1"))), hdr("i0", "i1"), {})
        return cur.group([Var("a")], C, header=hdr("a"))

    rows, detail = answered(gpu_session, make)
    assert rows == [{"a": a, "n": k * k}] and k * k > 1 << 32, (rows, detail)


# ------------------------------------------------------------------ 3. keys
CITIES = ["Ulm", "Graz", None, "Bern"]


@functools.lru_cache(maxsize=None)
def people_data():
    """hub_graph(34) over 30 :P nodes with a unique STRING name, a repeated
    nullable STRING city and a repeated nullable FLOAT score (−0.0 and 0.0 among
    its values)."""
    ids, src, dst = hub_graph(34)
    scores = [0.0, -0.0, 1.5, None, 2.25]
    nodes = []
    for i in range(30):
        p = {"name": f"p{i}", "city": CITIES[i % 4], "score": scores[i % 5]}
        nodes.append((i, frozenset(["P"]), {k: v for k, v in p.items() if v is not None}))
    rels = [(int(r), int(s), int(t), "E", {}) for r, s, t in zip(ids, src, dst)]
    return GraphData(nodes, rels), src.tolist(), dst.tolist(), nodes


def two_hop(items, where=()):
    return Query([Match([NodeP("a", ("P",)), NodeP("b"), NodeP("c")], [RelP("r1", "a", "b"), RelP("r2", "b", "c")],
                        where=list(where))], [Stage(list(items))])


def run_both(session, q, data, plan=PLAN):
    g = ScanGraph.from_data(session, data)
    session.reset_profile()
    rows = run(g, q)
    if plan is not None:
        assert session.last_plan() == plan, (session.last_plan(), session.last_plan_detail())
    else:
        assert session.last_plan() != PLAN, session.last_plan_detail()
    assert bag(rows) == bag(run(ScanGraph.from_data(OracleSession(), data), q))
    return rows, session.last_plan_detail()


A = Var("a", "NODE")


def prop(key, owner=A):
    return ElementProperty(owner, key)


@pytest.mark.gpu
def test_node_with_label_flag_and_string_property(gpu_session):
    """RETURN a, count(*): a's id, its constant label column and its properties — the unique route."""
    data, src, dst, _ = people_data()
    rows, detail = run_both(gpu_session, two_hop([("a", A), ("n", CountStar())]), data)
    assert detail.endswith(" group:unique")
    want = brute_grouped(src, dst, 2, 0)
    assert {r["a"].id: r["n"] for r in rows} == want
    assert all(r["a"].labels == frozenset(["P"]) and r["a"].props()["name"] == f"p{r['a'].id}" for r in rows)
    rows, detail = run_both(gpu_session, two_hop([("name", prop("name")), ("n", CountStar())]), data)
    assert detail.endswith(" group:unique") and {r["name"]: r["n"] for r in rows} == {f"p{k}": v for k, v in want.items()}


@pytest.mark.gpu
def test_non_unique_keys_take_the_hash_route(gpu_session):
    """A nullable repeated FLOAT alone (NULL one group, −0.0 = 0.0), and two properties together."""
    data, src, dst, nodes = people_data()
    per_a = brute_grouped(src, dst, 2, 0)
    rows, detail = run_both(gpu_session, two_hop([("score", prop("score")), ("n", CountStar())]), data)
    assert detail.endswith(" group:hash")
    want = {}
    for i, _, p in nodes:
        if per_a.get(i):
            k = p.get("score")
            k = 0.0 if k == 0 else k
            want[k] = want.get(k, 0) + per_a[i]
    assert {(0.0 if r["score"] == 0 else r["score"]): r["n"] for r in rows} == want and len(rows) == len(want) == 4
    rows, detail = run_both(gpu_session, two_hop([("city", prop("city")), ("score", prop("score")),
                                                  ("n", CountStar())]), data)
    assert detail.endswith(" group:hash") and sum(r["n"] for r in rows) == sum(per_a.values())


@pytest.mark.gpu
def test_two_count_star_aggregates(gpu_session):
    data, src, dst, _ = people_data()
    rows, _ = run_both(gpu_session, two_hop([("a", A), ("n", CountStar()), ("m", CountStar())]), data)
    want = brute_grouped(src, dst, 2, 0)
    assert {r["a"].id: (r["n"], r["m"]) for r in rows} == {k: (v, v) for k, v in want.items()}


@pytest.mark.gpu
def test_select_with_aliases_between_group_and_joins(gpu_session):
    ids, src, dst = hub_graph(35)
    tables = [{"id": K(ids), "s": K(src), "t": K(dst)}, {"id": K(np.arange(30)), "w": K(np.arange(30) % 4)}]

    def make(tabs):
        rels, nodes = tabs
        cur = nodes.select(("id", "a"), ("w", "aw")).join(rels.select(("s", "s0"), ("t", "t0")), "inner", ("a", "s0"))
        cur = cur.join(nodes.select(("id", "b")), "inner", ("t0", "b"))
        cur = cur.select(("aw", "weight"), ("a", "node"), ("b", "other"))
        return cur.group([Var("node"), Var("weight")], {"n": CountStar()}, header=hdr("node", "weight", "other"))

    rows, detail = answered(gpu_session, lambda: make(gpu_tables(gpu_session, tables)))
    assert detail.endswith(" group:unique")
    assert bag(rows) == bag(make(oracle_tables(tables)).rows)
    assert {r["node"]: r["n"] for r in rows} == brute_grouped(src.tolist(), dst.tolist(), 1, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("on", ["G", "other"])
def test_pushed_single_leaf_filter(gpu_session, on):
    ids, src, dst = hub_graph(36)
    tables = [{"id": K(ids), "s": K(src), "t": K(dst)}, {"id": K(np.arange(30))}]
    col = "a" if on == "G" else "t0"

    def make(tabs):
        rels, nodes = tabs
        cur = nodes.select(("id", "a")).join(rels.select(("s", "s0"), ("t", "t0")), "inner", ("a", "s0"))
        cur = cur.filter(GreaterThan(Var(col), IntegerLit(4)), hdr("a", "s0", "t0"), {})
        return cur.group([Var("a")], C, header=hdr("a"))

    rows, detail = answered(gpu_session, lambda: make(gpu_tables(gpu_session, tables)))
    want = {}
    for s, t in zip(src.tolist(), dst.tolist()):
        if (s if on == "G" else t) > 4:
            want[s] = want.get(s, 0) + 1
    assert {r["a"]: r["n"] for r in rows} == want and detail.endswith(" group:unique")
    assert bag(rows) == bag(make(oracle_tables(tables)).rows)


# ------------------------------------------------------------------ 4. declines
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["two_leaves", "rel_key", "count_b", "sum", "four_hops", "triangle", "switch"])
def test_declines(gpu_session, monkeypatch, case):
    data, src, dst, _ = people_data()
    n = ("n", CountStar())
    if case == "two_leaves":
        q = two_hop([("a", A), ("c", Var("c", "NODE")), n])
    elif case == "rel_key":
        q = two_hop([("r1", Var("r1", "RELATIONSHIP")), n])
    elif case == "count_b":
        q = two_hop([("a", A), n, ("k", Count(Var("b", "NODE")))])
    elif case == "sum":
        q = two_hop([("a", A), n, ("k", Sum(prop("score", Var("c", "NODE"))))])
    elif case == "four_hops":
        ids, s4, d4 = hub_graph(33, n_nodes=12, hub=0, extra=40)
        data = GraphData([(i, frozenset(["V"]), {}) for i in range(12)],
                         [(int(r), int(s), int(t), "E", {}) for r, s, t in zip(ids, s4, d4)])
        q = Query([Match([NodeP(v) for v in "abcde"], [RelP(f"r{i}", "abcde"[i], "abcde"[i + 1]) for i in range(4)])],
                  [Stage([("a", A), n])])
    elif case == "triangle":
        q = Query([Match([NodeP("a"), NodeP("b"), NodeP("c")],
                         [RelP("r1", "a", "b"), RelP("r2", "b", "c"), RelP("r3", "c", "a")])], [Stage([("a", A), n])])
    else:
        monkeypatch.setenv("CAPF_FUSED_GROUP", "0")
        q = two_hop([("a", A), n])
    rows, _ = run_both(gpu_session, q, data, plan=None)
    assert len(rows) > 0


@pytest.mark.gpu
def test_left_outer_join_declines(gpu_session):
    ids, src, dst = hub_graph(37)
    tables = [{"id": K(ids), "s": K(src), "t": K(dst)}, {"id": K(np.arange(34))}]

    def make(tabs):
        rels, nodes = tabs
        cur = nodes.select(("id", "a")).join(rels.select(("s", "s0"), ("t", "t0")), "left_outer", ("a", "s0"))
        return cur.group([Var("a")], C, header=hdr("a"))

    rows = declined(gpu_session, lambda: make(gpu_tables(gpu_session, tables)))
    assert bag(rows) == bag(make(oracle_tables(tables)).rows) and len(rows) == 34


# ------------------------------------------------------------------ 5. seeded random trees
def random_tree(seed):
    """(tables, edges, group leaf, key columns): 2–6 leaves, acyclic, at most 6
    children at any root, small integer keys with duplicates and NULLs; every
    leaf has payload columns p0, p1 (duplicates, NULLs) to group by."""
    r = random.Random(seed)
    nt = r.randint(2, 6)
    tables = [dict() for _ in range(nt)]
    rows = [r.choice([1, r.randint(2, 40), r.randint(41, 130)]) for _ in range(nt)]
    edges = []
    for b in range(1, nt):
        a = r.randrange(b)
        hi = r.choice([4, 12, 40])
        for t, name in ((a, f"e{b}a"), (b, f"e{b}b")):
            vals = [r.randrange(hi) for _ in range(rows[t])]
            nulls = [r.random() < 0.15 for _ in range(rows[t])] if r.random() < 0.4 else None
            tables[t][name] = K(vals, nulls)
        edges.append((a, f"e{b}a", b, f"e{b}b"))
    for t in range(nt):
        for j in range(2):
            tables[t][f"p{t}_{j}"] = K([r.randrange(5) for _ in range(rows[t])],
                                       [r.random() < 0.2 for _ in range(rows[t])] if j else None)
    gl = r.randrange(nt)
    cand = list(tables[gl])
    keys = r.sample(cand, r.randint(1, min(3, len(cand))))
    return tables, edges, gl, keys


def dict_grouped(tables, edges, gl, keys):
    """{key tuple (None for NULL): Σ weight} by message passing in Python dicts, rooted at the group leaf."""
    adj = {i: [] for i in range(len(tables))}
    for a, ca, b, cb in edges:
        adj[a].append((b, ca, cb))
        adj[b].append((a, cb, ca))

    def col(t, c):
        v, ok = tables[t][c]
        v = v.tolist()
        return v if ok is None else [x if o else None for x, o in zip(v, ok.tolist())]

    def weights(v, parent):
        w = [1] * nrows(tables[v])
        for u, mine, theirs in adj[v]:
            if u == parent:
                continue
            m = {}
            for wi, k in zip(weights(u, v), col(u, theirs)):
                if k is not None and wi:
                    m[k] = m.get(k, 0) + wi
            w = [wi * m.get(k, 0) if k is not None else 0 for wi, k in zip(w, col(v, mine))]
        return w

    out = {}
    kc = [col(gl, c) for c in keys]
    for i, w in enumerate(weights(gl, -1)):
        if w:
            k = tuple(c[i] for c in kc)
            out[k] = out.get(k, 0) + w
    return out


SEEDS = list(range(40))


def test_random_trees_are_trees():
    shapes = set()
    for seed in SEEDS:
        tables, edges, gl, keys = random_tree(seed)
        assert 2 <= len(tables) <= 6 and len(edges) == len(tables) - 1 and all(a < b for a, _, b, _ in edges)
        assert all(k in tables[gl] for k in keys) and keys
        shapes.add(len(tables))
        assert sum(dict_grouped(tables, edges, gl, keys).values()) == \
            sum(dict_grouped(tables, edges, 0, [next(iter(tables[0]))]).values())
    assert shapes == {2, 3, 4, 5, 6}


@pytest.mark.gpu
def test_random_trees_vs_dictionaries(gpu_session):
    bad = []
    for seed in SEEDS:
        tables, edges, gl, keys = random_tree(seed)
        want = dict_grouped(tables, edges, gl, keys)
        tabs = gpu_tables(gpu_session, tables, [random.Random(seed).choice([None, 4, 3])] * len(tables))
        names = [c for t in tables for c in t]
        gpu_session.reset_profile()
        rows = join_tree(tabs, edges, seed % len(tables)).group([Var(k) for k in keys], C, header=hdr(*names)).rows
        got = {tuple(r[k] for k in keys): r["n"] for r in rows}
        if gpu_session.last_plan() != PLAN or got != want or len(rows) != len(want):
            bad.append((seed, gpu_session.last_plan(), gpu_session.last_plan_detail(), len(rows), len(want)))
    assert not bad, bad[:5]


# ------------------------------------------------------------------ 6. against the relational plan
TWO_HOP_BY_A = path_query(2, "a")


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [8, 10])
def test_fused_equals_relational_plan(gpu_session, monkeypatch, scale):
    from capf_amd.synthetic import rmat_graph
    g = rmat_graph(gpu_session, scale)
    gpu_session.reset_profile()
    got = run(g, TWO_HOP_BY_A)
    assert gpu_session.last_plan() == PLAN
    monkeypatch.setenv("CAPF_FUSED_GROUP", "0")
    gpu_session.reset_profile()
    plain = run(g, TWO_HOP_BY_A)
    assert gpu_session.last_plan() != PLAN
    assert bag(got) == bag(plain) and len(got) > 0


@pytest.mark.gpu
def test_s14_equals_closed_form(gpu_session):
    """1.2e8 joined rows never built: per a, Σ_{r: start = a} out(end(r)) − selfloops(a)."""
    from capf_amd.synthetic import rmat_graph
    scale = 14
    g = rmat_graph(gpu_session, scale, compact=True)
    gpu_session.reset_profile()
    op_rows = run(g, TWO_HOP_BY_A)
    assert gpu_session.last_plan() == PLAN and gpu_session.last_plan_detail().endswith(" group:unique")
    rels = g.rel_tables[0].table
    src = np.array(rels.column_values("source"), dtype=np.int64)
    dst = np.array(rels.column_values("target"), dtype=np.int64)
    n = 1 << scale
    out = np.bincount(src, minlength=n).astype(np.int64)
    want = np.zeros(n, dtype=np.int64)
    np.add.at(want, src, out[dst])
    want -= np.bincount(src[src == dst], minlength=n)
    got = np.zeros(n, dtype=np.int64)
    for r in op_rows:
        got[r["a"].id] = r["n"]
    assert len(op_rows) == int((want != 0).sum()) and np.array_equal(got, want)
    assert int(want.sum()) > 10 ** 8
