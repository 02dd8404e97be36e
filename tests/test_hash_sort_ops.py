"""ORDER BY, GROUP BY, DISTINCT and the hash join (csrc/kernels_hash.hip) at
edge values and at size, against plain Python / numpy expectations written
here from the rules of DESIGN.md ("Ordering and equality of values"):

  −∞ < … < −0.0 = 0.0 < … < +∞ < NaN < NULL     (every NaN one value)

ascending; descending is the exact reverse; ties keep input order.  Grouping,
DISTINCT and join keys use the same equality (all NaNs one key, ±0.0 one key,
NULL one key per column for grouping and no match in a join); FLOAT min / max
use the same order.  All comparisons are exact: integers and row indexes by
==, floats by value after mapping every NaN to one token and −0.0 to 0.0.

The tests marked gpu run the HIP backend; the unmarked ones hold the numpy
oracle (oracle/table_np.py) to the same expectations on the small cases, and
pin oracle/rowhash.py.  No expectation calls an OracleTable method."""
import functools
from collections import defaultdict
from dataclasses import dataclass

import numpy as np
import pytest

from capf_amd.expr import (Avg, Count, CountStar, FloatLit, Max, Min, PercentileDisc, Sum, Var, T_BOOL, T_FLOAT,
                           T_INT, T_STRING)
from capf_amd.header import RecordHeader
from oracle import rowhash
from oracle.table_np import OracleSession

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
NAN_POS, NAN_NEG, NAN_PAYLOAD = 0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001
# +NaN, −NaN, a payload NaN, ±∞, ±0.0, ±5e-324, ±DBL_MAX, 1.0 — and NULL (None)
SPECIAL_BITS = [NAN_POS, NAN_NEG, NAN_PAYLOAD, 0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000000,
                0x8000000000000000, 0x0000000000000001, 0x8000000000000001, 0x7FEFFFFFFFFFFFFF,
                0xFFEFFFFFFFFFFFFF, 0x3FF0000000000000]
SPECIALS = SPECIAL_BITS + [None]
INT_EDGES = [I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX, None]
SMALL_N = [0, 1, 2, 255, 256, 257, 4097]  # block edges, either side of rocprim's single-block sort
BIG = 2 ** 20 + 257  # the smallest count at which every grid-stride loop takes a second trip
WORDS = ["", "a", "ab", "B", "\uE000", "\U0001F600", None]  # (U+1F600 sorts below U+E000 in UTF-16)


def H(*names):
    return RecordHeader({Var(c): c for c in names})


def distinct_agg(cls):
    @dataclass(frozen=True)
    class D(cls):
        distinct = True
    return D


# ------------------------------------------------------------------ backends
class Gpu:
    def __init__(self, session):
        self.s = session

    def table(self, cols, compact=None):
        t = self.s.table(cols)
        return t.compact(compact) if compact else t


class Oracle:
    def table(self, cols, compact=None):
        return OracleSession().table(cols)


# -------------------------------------------------------------- value helpers
def f64(bits, nulls_as=0):
    """(float64 array, valid) from uint64 bit patterns (None = NULL): built
    with .view so that every NaN pattern reaches the device unchanged."""
    b = np.array([nulls_as if x is None else x for x in bits], dtype=np.uint64)
    return b.view(np.float64), np.array([x is not None for x in bits], dtype=np.uint8)


def i64(vals):
    return (np.array([0 if x is None else x for x in vals], dtype=np.int64),
            np.array([x is not None for x in vals], dtype=np.uint8))


def py(col):
    """Python values (None = NULL) of a column spec (name, type, values, valid)."""
    _, t, v, valid = col
    if isinstance(v, list):
        return list(v)
    out = v.tolist()
    if t == T_BOOL:
        out = [bool(x) for x in out]
    if valid is not None:
        out = [x if ok else None for x, ok in zip(out, valid.tolist())]
    return out


def sk(v):
    """Sort key (is_null, is_nan, value); strings in String.compareTo order."""
    if v is None:
        return (1, 0, 0)
    if isinstance(v, float) and v != v:
        return (0, 1, 0)
    if isinstance(v, str):
        return (0, 0, v.encode("utf-16-be", "surrogatepass"))
    return (0, 0, v)


def gk(v):
    """Canonical key of one value: all NaNs one key (−0.0 == 0.0 hash alike)."""
    return "NaN" if isinstance(v, float) and v != v else v


def cv(v):
    """Canonical result value: typed; floats by value with one NaN and one zero."""
    if isinstance(v, float):
        return ("f", "NaN") if v != v else ("f", v + 0.0)
    return v


def cvs(xs):
    return [cv(x) for x in xs]


def expect_order(n, *keys):
    """keys: (python values, desc); applied last key first, each stable."""
    idx = list(range(n))
    for vals, desc in reversed(keys):
        idx = sorted(idx, key=lambda i: sk(vals[i]), reverse=desc)
    return idx


# ================================================================= A. ORDER BY
def order_key_column(kind, n):
    """(column spec, compact width or None, expected (encoding, base) or None)."""
    rng = np.random.default_rng(1000 + n)
    if kind == "float":
        bits = [SPECIALS[(i // 2) % len(SPECIALS)] if i % 2 == 0 else
                int(np.float64(rng.normal() * 10.0 ** int(rng.integers(-3, 4))).view(np.uint64)) for i in range(n)]
        v, ok = f64(bits)
        return ("k", T_FLOAT, v, ok), None, None
    if kind == "int":
        v, ok = i64([INT_EDGES[i % len(INT_EDGES)] for i in range(n)])
        return ("k", T_INT, v, ok), None, None
    if kind.startswith("for"):
        width, span = (4, 2 ** 32) if kind.startswith("for32") else (3, 2 ** 24)
        base = 2 ** 62 if kind.endswith("pos") else -2 ** 62
        vals = [base + int(x) if i % 6 != 5 else None for i, x in enumerate(rng.integers(0, span, n))]
        if n > 0:
            vals[0] = base  # the column's minimum: the FOR base
        if n > 1:
            vals[1] = base + span - 1  # the widest offset
        for i in range(7, n, 7):  # ties
            vals[i] = vals[i - 3]
        v, ok = i64(vals)
        return ("k", T_INT, v, ok), width, (1 if width == 4 else 2, base)
    if kind == "bool":
        vals = [[True, False, None, False, True][(i * 7 + i // 5) % 5] for i in range(n)]
        return ("k", T_BOOL, np.array([bool(x) for x in vals], dtype=np.uint8),
                np.array([x is not None for x in vals], dtype=np.uint8)), None, None
    assert kind == "string"
    return ("k", T_STRING, [WORDS[(i * 5 + i // 7) % len(WORDS)] for i in range(n)], None), None, None


ORDER_KINDS = ["float", "int", "for32_pos", "for32_neg", "for24_pos", "for24_neg", "bool", "string"]


def run_order_single(be, kind, n):
    col, width, enc = order_key_column(kind, n)
    t = be.table([col, ("i", T_INT, np.arange(n, dtype=np.int64), None)], compact=width)
    if enc and n > 0 and hasattr(t, "encoding"):
        assert t.encoding("k") == enc
    vals = py(col)
    for desc in (False, True):
        got = t.orderBy((Var("k"), "desc" if desc else "asc"), header=H("k", "i"), params={})
        assert got.column_values("i") == expect_order(n, (vals, desc)), (kind, n, desc)
        assert cvs(got.column_values("k")) == cvs([vals[i] for i in expect_order(n, (vals, desc))])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("kind", ORDER_KINDS)
def test_order_single_key(gpu_session, kind, n):
    run_order_single(Gpu(gpu_session), kind, n)


@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("kind", ORDER_KINDS)
def test_order_single_key_oracle(kind, n):
    run_order_single(Oracle(), kind, n)


def multi_cols(n, seed=7):
    """(k INT, f FLOAT, b BOOL, s STRING, i): every key column from a small
    domain of edge values (heavy ties), NULLs placed independently."""
    rng = np.random.default_rng(seed)
    kd = np.array(INT_EDGES[:-1], dtype=np.int64)
    fb = np.array(SPECIAL_BITS, dtype=np.uint64)
    words = WORDS[:-1]
    sv = rng.random(n) > 0.15
    return [("k", T_INT, kd[rng.integers(0, len(kd), n)], (rng.random(n) > 0.15).astype(np.uint8)),
            ("f", T_FLOAT, fb[rng.integers(0, len(fb), n)].view(np.float64), (rng.random(n) > 0.15).astype(np.uint8)),
            ("b", T_BOOL, rng.integers(0, 2, n).astype(np.uint8), (rng.random(n) > 0.15).astype(np.uint8)),
            ("s", T_STRING, [words[j] if ok else None for j, ok in zip(rng.integers(0, len(words), n), sv)], None),
            ("i", T_INT, np.arange(n, dtype=np.int64), None)]


MULTI_ORDERS = {"s_asc_f_desc_k_asc": [("s", False), ("f", True), ("k", False)],
                "b_desc_k_desc": [("b", True), ("k", True)]}


def run_order_multi(be, case):
    n = 4097
    cols = multi_cols(n)
    vals = {c[0]: py(c) for c in cols}
    t = be.table(cols)
    items = MULTI_ORDERS[case]
    got = t.orderBy(*[(Var(c), "desc" if d else "asc") for c, d in items], header=H("k", "f", "b", "s", "i"), params={})
    assert got.column_values("i") == expect_order(n, *[(vals[c], d) for c, d in items])


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(MULTI_ORDERS))
def test_order_multi_key(gpu_session, case):
    run_order_multi(Gpu(gpu_session), case)


@pytest.mark.parametrize("case", list(MULTI_ORDERS))
def test_order_multi_key_oracle(case):
    run_order_multi(Oracle(), case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["int_1000_values_asc", "float_finite_desc"])
def test_order_big(gpu_session, case):
    """BIG rows: the second trip of k_sort_key / k_gather_u64 and rocprim's
    multi-block radix sort; with 1000 distinct keys stability decides almost
    every position."""
    rng = np.random.default_rng(5)
    if case == "int_1000_values_asc":
        k = rng.integers(-500, 500, BIG).astype(np.int64) * 1_000_003
        want = np.argsort(k, kind="stable")
        col, o = ("k", T_INT, k, None), "asc"
    else:
        f = rng.integers(-5000, 5000, BIG).astype(np.float64) / 8.0  # finite, with ties and a zero
        want = np.argsort(-f, kind="stable")  # finite values: the negation reverses the order exactly
        col, o = ("k", T_FLOAT, f, None), "desc"
    t = gpu_session.table([col, ("i", T_INT, np.arange(BIG, dtype=np.int64), None)])
    got, ok = t.orderBy((Var("k"), o), header=H("k", "i"), params={}).column_arrays("i")
    assert ok.all() and np.array_equal(got, want)


SKIP_LIMIT = {"skip0": [("skip", 0)], "skip255": [("skip", 255)], "skip256": [("skip", 256)],
              "skip1000": [("skip", 1000)], "skip1005": [("skip", 1005)], "limit0": [("limit", 0)],
              "limit1": [("limit", 1)], "limit257": [("limit", 257)], "limit1000": [("limit", 1000)],
              "limit1005": [("limit", 1005)], "skip250_limit10": [("skip", 250), ("limit", 10)],
              "limit300_skip256": [("limit", 300), ("skip", 256)]}


def run_skip_limit(be, ops):
    n = 1000
    k = [(i * 7919) % 37 if i % 11 else None for i in range(n)]
    t = be.table([("k", T_INT, *i64(k)), ("i", T_INT, np.arange(n, dtype=np.int64), None)])
    t = t.orderBy((Var("k"), "desc"), header=H("k", "i"), params={})
    want = expect_order(n, (k, True))
    for op, m in SKIP_LIMIT[ops]:
        t = getattr(t, op)(m)
        want = want[m:] if op == "skip" else want[:m]
    assert t.size == len(want)
    assert t.column_values("i") == want
    assert t.column_values("k") == [k[i] for i in want]


@pytest.mark.gpu
@pytest.mark.parametrize("ops", list(SKIP_LIMIT))
def test_skip_limit_edges(gpu_session, ops):
    run_skip_limit(Gpu(gpu_session), ops)


@pytest.mark.parametrize("ops", list(SKIP_LIMIT))
def test_skip_limit_edges_oracle(ops):
    run_skip_limit(Oracle(), ops)


# ================================================================= B. GROUP BY
def unique_keys(n, seed=0):
    """n distinct sparse int64 keys of both signs, INT64_MIN and INT64_MAX among them."""
    with np.errstate(over="ignore"):
        k = ((np.arange(n, dtype=np.uint64) + np.uint64(seed + 1)) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)
    k = k.copy()
    k[n // 3], k[(2 * n) // 3] = I64_MIN, I64_MAX
    assert len(np.unique(k)) == n
    return k


def run_group_unique(be, n, arrays=False):
    k = unique_keys(n, seed=n)
    t = be.table([("k", T_INT, k, None), ("x", T_INT, k.copy(), None)])
    out = t.group([Var("k")], {"c": CountStar(), "mn": Min(Var("x")), "mx": Max(Var("x")), "sm": Sum(Var("x"))},
                  header=H("k", "x"), params={})
    assert out.size == n
    for c in ("k", "mn", "mx", "sm"):  # groups come ordered by their smallest row: the input order
        if arrays:
            v, ok = out.column_arrays(c)
            assert ok.all() and np.array_equal(v, k), c
        else:
            assert out.column_values(c) == k.tolist(), c
    if arrays:
        assert np.array_equal(out.column_arrays("c")[0], np.ones(n, dtype=np.int64))
    else:
        assert out.column_values("c") == [1] * n


CAPACITY_STEPS = [511, 512, 513, 65536, 65537]  # load exactly 0.5 at 512 and 65536


@pytest.mark.gpu
@pytest.mark.parametrize("n", CAPACITY_STEPS + [BIG])
def test_group_all_unique(gpu_session, n):
    run_group_unique(Gpu(gpu_session), n, arrays=True)


@pytest.mark.parametrize("n", CAPACITY_STEPS)
def test_group_all_unique_oracle(n):
    run_group_unique(Oracle(), n)


def np_groups(keys):
    """(dense group id per row, representative row per group), groups ordered
    by their smallest row."""
    _, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    remap = np.empty_like(order)
    remap[order] = np.arange(len(order))
    return remap[np.asarray(inv).reshape(-1)], first[order]


def np_int_aggs(gid, ng, x, valid):
    """count(x), wrapped sum, min, max per group over the non-NULL x (numpy)."""
    sel = valid.astype(bool)
    g, xv = gid[sel], x[sel]
    o = np.argsort(g, kind="stable")
    gs, xs = g[o], xv[o]
    cnt = np.bincount(gs, minlength=ng).astype(np.int64)
    sm, mn, mx = (np.zeros(ng, dtype=np.int64) for _ in range(3))
    if len(gs):
        starts = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]])
        present = gs[starts]
        sm[present] = np.add.reduceat(xs.view(np.uint64), starts).view(np.int64)  # modulo 2^64
        mn[present] = np.minimum.reduceat(xs, starts)
        mx[present] = np.maximum.reduceat(xs, starts)
    return cnt, sm, mn, mx


@functools.lru_cache(maxsize=None)
def skewed_data():
    """BIG rows, about 300 000 groups: one key on 20 % of the rows, the rest
    Zipf-like; x near ±2^62 (hot groups wrap) with INT_EDGES sprinkled in, 5 % NULL."""
    rng = np.random.default_rng(99)
    g = (rng.random(BIG) ** 3 * 470_000).astype(np.int64)
    g[rng.random(BIG) < 0.2] = 77
    k = g * 1_000_003 - 2 ** 40
    x = np.where(rng.random(BIG) < 0.5, 1, -1) * (2 ** 62 + rng.integers(0, 1 << 20, BIG))
    edges = np.array(INT_EDGES[:-1], dtype=np.int64)
    at = rng.random(BIG) < 0.01
    x[at] = edges[rng.integers(0, len(edges), int(at.sum()))]
    xv = (rng.random(BIG) > 0.05).astype(np.uint8)
    f = rng.normal(size=BIG)
    f[::1000] = np.array([NAN_NEG], dtype=np.uint64).view(np.float64)[0]
    for a in (k, x, xv, f):
        a.setflags(write=False)
    return k, x, xv, f


def check_int_aggs(out, ng, cnt_star, cnt, sm, mn, mx):
    assert out.size == ng
    v, ok = out.column_arrays("c")
    assert ok.all() and np.array_equal(v, cnt_star)
    v, ok = out.column_arrays("cx")
    assert ok.all() and np.array_equal(v, cnt)
    has = cnt > 0
    for name, want in (("sm", sm), ("mn", mn), ("mx", mx)):
        v, ok = out.column_arrays(name)
        assert np.array_equal(ok, has), name
        assert np.array_equal(v[has], want[has]), name
    v, ok = out.column_arrays("av")  # the wrapped int64 sum as a double over the count
    assert np.array_equal(ok, has)
    want = sm[has].astype(np.float64) / cnt[has].astype(np.float64)
    assert np.array_equal(v[has].view(np.uint64), want.view(np.uint64))


INT_AGGS = {"c": CountStar(), "cx": Count(Var("x")), "sm": Sum(Var("x")), "av": Avg(Var("x")),
            "mn": Min(Var("x")), "mx": Max(Var("x"))}


@pytest.mark.gpu
def test_group_big_skewed(gpu_session):
    k, x, xv, _ = skewed_data()
    gid, reps = np_groups(k)
    ng = len(reps)
    assert 250_000 < ng < 350_000
    t = gpu_session.table([("k", T_INT, k, None), ("x", T_INT, x, xv)])
    out = t.group([Var("k")], INT_AGGS, header=H("k", "x"), params={})
    kv, ok = out.column_arrays("k")
    assert ok.all() and np.array_equal(kv, k[reps])
    check_int_aggs(out, ng, np.bincount(gid, minlength=ng), *np_int_aggs(gid, ng, x, xv))


def expect_groups(keys_per_col, n):
    """dict canonical key tuple → rows, in order of first appearance."""
    groups = {}
    for i, key in enumerate(zip(*[[gk(v) for v in col] for col in keys_per_col])):
        groups.setdefault(key, []).append(i)
    return groups


N_MULTI = 70_001


def run_group_multi(be):
    cols = multi_cols(N_MULTI)
    vals = {c[0]: py(c) for c in cols}
    keys = ["k", "f", "b", "s"]
    groups = expect_groups([vals[c] for c in keys], N_MULTI)
    t = be.table(cols)
    aggs = {"c": CountStar(), "lo": Min(Var("i")), "hi": Max(Var("i"))}
    hdr = H("k", "f", "b", "s", "i")
    out = t.group([Var(c) for c in keys], aggs, header=hdr, params={})
    res = {c: out.column_values(c) for c in keys + list(aggs)}
    assert out.size == len(groups)
    # groups ordered by their smallest row; the key columns hold that row's key:
    # the NaN group's key comes back as a NaN, the ±0.0 group's as a zero
    assert res["lo"] == [rows[0] for rows in groups.values()]
    assert res["hi"] == [rows[-1] for rows in groups.values()]
    assert res["c"] == [len(rows) for rows in groups.values()]
    for c in keys:
        assert cvs(res[c]) == cvs([vals[c][rows[0]] for rows in groups.values()]), c
    assert any(isinstance(v, float) and v != v for v in res["f"])
    # identical rows in identical order on a second run
    again = t.group([Var(c) for c in keys], aggs, header=hdr, params={})
    assert all(cvs(again.column_values(c)) == cvs(res[c]) for c in res)


@pytest.mark.gpu
def test_group_multi_column_keys(gpu_session):
    run_group_multi(Gpu(gpu_session))


def test_group_multi_column_keys_oracle():
    run_group_multi(Oracle())


def float_min(xs):
    """min / max of non-NULL floats under the total order (NaN largest)."""
    return min(xs, key=sk) if xs else None


def float_max(xs):
    return max(xs, key=sk) if xs else None


def minmax_table(n=4097):
    """Groups 0 all NaN, 1 NaN + finite, 2 NaN + ±∞, 3 only ±0.0, 4 only NULL,
    5 finite with NULLs, 6 one row."""
    rng = np.random.default_rng(3)
    nans = [NAN_POS, NAN_NEG, NAN_PAYLOAD]
    g, bits = [], []
    for i in range(n):
        grp = 6 if i == 2000 else i % 6
        r = int(rng.integers(0, 1 << 30))
        fin = int(np.float64(rng.normal() * 1e3).view(np.uint64))
        bits.append({0: nans[r % 3], 1: nans[r % 3] if r % 4 == 0 else fin,
                     2: [NAN_NEG, 0x7FF0000000000000, 0xFFF0000000000000][r % 3],
                     3: [0x8000000000000000, 0][r % 2], 4: None, 5: None if r % 3 == 0 else fin,
                     6: 0xFFF0000000000000}[grp])
        g.append(grp)
    return g, bits


def run_float_minmax(be):
    g, bits = minmax_table()
    f, ok = f64(bits)
    vals = py(("f", T_FLOAT, f, ok))
    t = be.table([("g", T_INT, np.array(g, dtype=np.int64), None), ("f", T_FLOAT, f, ok)])
    out = t.group([Var("g")], {"mn": Min(Var("f")), "mx": Max(Var("f")), "c": Count(Var("f"))},
                  header=H("g", "f"), params={})
    by = defaultdict(list)
    for grp, v in zip(g, vals):
        if v is not None:
            by[grp].append(v)
    got = {r["g"]: r for r in out.rows}
    assert sorted(got) == list(range(7))
    for grp in range(7):
        assert got[grp]["c"] == len(by[grp])
        assert cv(got[grp]["mn"]) == cv(float_min(by[grp])), ("min", grp)
        assert cv(got[grp]["mx"]) == cv(float_max(by[grp])), ("max", grp)
    assert cv(got[0]["mn"]) == cv(got[0]["mx"]) == ("f", "NaN")       # all NaN
    assert cv(got[1]["mx"]) == ("f", "NaN") and got[1]["mn"] == got[1]["mn"]  # NaN + finite: min is finite
    assert cv(got[2]["mn"]) == ("f", float("-inf"))
    assert got[3]["mn"] == 0.0 and got[3]["mx"] == 0.0            # zeros compare numerically
    assert got[4]["mn"] is None and got[4]["mx"] is None


@pytest.mark.gpu
def test_float_min_max_total_order(gpu_session):
    run_float_minmax(Gpu(gpu_session))


def test_float_min_max_total_order_oracle():
    run_float_minmax(Oracle())


def run_distinct_aggs(be):
    """count(DISTINCT f), min(DISTINCT f), count(DISTINCT k) per (b, s) group:
    both NaNs and the payload NaN count once, ±0.0 counts once."""
    cols = multi_cols(N_MULTI)
    vals = {c[0]: py(c) for c in cols}
    groups = expect_groups([vals["b"], vals["s"]], N_MULTI)
    t = be.table(cols)
    aggs = {"cdf": Count(Var("f"), True), "mdf": distinct_agg(Min)(Var("f")), "cdk": Count(Var("k"), True),
            "mxf": Max(Var("f")), "lo": Min(Var("i"))}
    out = t.group([Var("b"), Var("s")], aggs, header=H("k", "f", "b", "s", "i"), params={})
    res = {c: out.column_values(c) for c in aggs}
    assert res["lo"] == [rows[0] for rows in groups.values()]
    for j, rows in enumerate(groups.values()):
        fs = [vals["f"][i] for i in rows if vals["f"][i] is not None]
        ks = [vals["k"][i] for i in rows if vals["k"][i] is not None]
        assert res["cdf"][j] == len({gk(v) for v in fs}), j
        assert res["cdk"][j] == len(set(ks)), j
        assert cv(res["mdf"][j]) == cv(float_min(fs)), j
        assert cv(res["mxf"][j]) == cv(float_max(fs)), j
    assert max(res["cdf"]) == 9  # 12 special values: the three NaNs count once, the two zeros once


@pytest.mark.gpu
def test_distinct_aggregates_float_keys(gpu_session):
    run_distinct_aggs(Gpu(gpu_session))


def test_distinct_aggregates_float_keys_oracle():
    run_distinct_aggs(Oracle())


GLOBAL_AGGS = dict(INT_AGGS, fmn=Min(Var("f")), fmx=Max(Var("f")), cdf=Count(Var("f"), True))


def run_global_small(be, n):
    x, xv = i64([I64_MAX][:n])
    f, fv = f64([NAN_NEG][:n])
    t = be.table([("x", T_INT, x, xv), ("f", T_FLOAT, f, fv)])
    rows = t.group([], GLOBAL_AGGS, header=H("x", "f"), params={}).rows
    assert len(rows) == 1
    r = {c: cv(v) for c, v in rows[0].items()}
    if n == 0:
        assert r == dict(c=0, cx=0, sm=None, av=None, mn=None, mx=None, fmn=None, fmx=None, cdf=0)
    else:
        nan = ("f", "NaN")
        assert r == dict(c=1, cx=1, sm=I64_MAX, av=("f", float(I64_MAX)), mn=I64_MAX, mx=I64_MAX, fmn=nan, fmx=nan,
                         cdf=1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1])
def test_global_aggregation_small(gpu_session, n):
    run_global_small(Gpu(gpu_session), n)


@pytest.mark.parametrize("n", [0, 1])
def test_global_aggregation_small_oracle(n):
    run_global_small(Oracle(), n)


@pytest.mark.gpu
def test_global_aggregation_big(gpu_session):
    _, x, xv, f = skewed_data()
    t = gpu_session.table([("x", T_INT, x, xv), ("f", T_FLOAT, f, None)])
    out = t.group([], GLOBAL_AGGS, header=H("x", "f"), params={})
    check_int_aggs(out, 1, np.array([BIG]), *np_int_aggs(np.zeros(BIG, dtype=np.int64), 1, x, xv))
    r = out.rows[0]
    finite = f[~np.isnan(f)]
    assert r["fmn"] == float(finite.min()) and cv(r["fmx"]) == ("f", "NaN")  # max of a group with a NaN is NaN
    assert r["cdf"] == len(np.unique(finite + 0.0)) + 1


def run_percentile_nan(be):
    f, ok = f64([0x3FF0000000000000, NAN_NEG, 0x4008000000000000])  # 1.0, −NaN, 3.0
    t = be.table([("f", T_FLOAT, f, ok)])
    rows = t.group([], {"q": PercentileDisc(Var("f"), FloatLit(1.0))}, header=H("f"), params={}).rows
    assert [cv(r["q"]) for r in rows] == [("f", "NaN")]  # Scala's Double ordering sorts NaN last


@pytest.mark.gpu
def test_percentile_disc_sorts_nan_last(gpu_session):
    run_percentile_nan(Gpu(gpu_session))


def test_percentile_disc_sorts_nan_last_oracle():
    run_percentile_nan(Oracle())


# ================================================================= C. DISTINCT
def run_distinct_multi(be):
    cols = multi_cols(N_MULTI)
    vals = {c[0]: py(c) for c in cols}
    keys = ["k", "f", "b", "s"]
    first = [rows[0] for rows in expect_groups([vals[c] for c in keys], N_MULTI).values()]
    t = be.table(cols)
    d = t.distinct(*keys)  # one row per key: the one with the smallest i, in ascending i
    assert d.column_values("i") == first
    d = t.select(*keys).distinct()
    assert d.size == len(first)
    for c in keys:
        assert cvs(d.column_values(c)) == cvs([vals[c][i] for i in first]), c
    assert t.distinct().column_values("i") == list(range(N_MULTI))  # i makes every row its own key
    first_f = [rows[0] for rows in expect_groups([vals["f"]], N_MULTI).values()]
    assert len(first_f) == 10  # 9 distinct special values + NULL: the NaNs one row, the zeros one row
    assert t.distinct("f").column_values("i") == first_f


@pytest.mark.gpu
def test_distinct_multi_column(gpu_session):
    run_distinct_multi(Gpu(gpu_session))


def test_distinct_multi_column_oracle():
    run_distinct_multi(Oracle())


def run_distinct_specials(be):
    f, ok = f64(SPECIALS * 3)
    n = len(f)
    t = be.table([("f", T_FLOAT, f, ok), ("i", T_INT, np.arange(n, dtype=np.int64), None)])
    d = t.distinct("f")
    # NaN (rows 0-2) once, ±∞, the zeros (rows 5, 6) once, ±5e-324, ±DBL_MAX, 1.0, NULL
    assert d.column_values("i") == [0, 3, 4, 5, 7, 8, 9, 10, 11, 12]
    assert cvs(d.column_values("f")) == cvs([py(("f", T_FLOAT, f, ok))[i] for i in [0, 3, 4, 5, 7, 8, 9, 10, 11, 12]])


@pytest.mark.gpu
def test_distinct_specials(gpu_session):
    run_distinct_specials(Gpu(gpu_session))


def test_distinct_specials_oracle():
    run_distinct_specials(Oracle())


@pytest.mark.gpu
@pytest.mark.parametrize("data", ["all_unique", "skewed"])
def test_distinct_big(gpu_session, data):
    k = unique_keys(BIG, seed=BIG) if data == "all_unique" else skewed_data()[0]
    t = gpu_session.table([("k", T_INT, k, None), ("i", T_INT, np.arange(BIG, dtype=np.int64), None)])
    want = np_groups(k)[1]
    got, ok = t.distinct("k").column_arrays("i")
    assert ok.all() and np.array_equal(got, want)
    got, ok = t.select("k").distinct().column_arrays("k")
    assert ok.all() and np.array_equal(got, k[want])


# ================================================================ D. hash join
JOIN_TYPES = ["inner", "left_outer", "right_outer", "full_outer"]
FLOAT_KEY_BITS = [0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                  0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF, 0x7FEFFFFFFFFFFFFF]  # no NaN
FOR24_BASE = 2 ** 62


def with_nulls(rng, n, every):
    ok = (rng.random(n) > 1.0 / every).astype(np.uint8)
    if n:
        ok[0] = 1
    return ok


def join_side(rng, n, shape, dom, prefix, hot_rows):
    """Key columns of one side (names prefix+"0", prefix+"1") plus its row index;
    the first hot_rows rows carry one hot key."""
    d = rng.integers(0, dom, n)
    d[:hot_rows] = 5
    cols = []
    if shape == "float":
        bits = np.array(FLOAT_KEY_BITS, dtype=np.uint64)
        f = np.where(d < len(bits), bits[np.minimum(d, len(bits) - 1)].view(np.float64), d * 0.5 + 0.25)
        cols.append((prefix + "0", T_FLOAT, np.ascontiguousarray(f, dtype=np.float64), with_nulls(rng, n, 14)))
    elif shape == "for24":
        k = FOR24_BASE + d.astype(np.int64) * 3
        if n:
            k[0] = FOR24_BASE
        cols.append((prefix + "0", T_INT, k, with_nulls(rng, n, 14)))
    else:
        cols.append((prefix + "0", T_INT, d.astype(np.int64) * 1_000_003 - 2 ** 50, with_nulls(rng, n, 14)))
        e = rng.integers(0, 3, n)
        e[:hot_rows] = 1
        if shape == "int_string":
            ok = with_nulls(rng, n, 17)
            cols.append((prefix + "1", T_STRING, [["x", "", "\U0001F600"][j] if o else None for j, o in zip(e, ok)], None))
        elif shape == "int_bool":
            cols.append((prefix + "1", T_BOOL, (e > 0).astype(np.uint8), with_nulls(rng, n, 17)))
        else:
            cols.append((prefix + "1", T_INT, np.array([I64_MIN, 0, I64_MAX], dtype=np.int64)[e], with_nulls(rng, n, 17)))
    return cols, cols + [(prefix + "i", T_INT, np.arange(n, dtype=np.int64), None)]


def join_keys_py(key_cols):
    """Per row the canonical key tuple, or None when any key column is NULL."""
    return [None if any(v is None for v in key) else tuple(gk(v) for v in key)
            for key in zip(*[py(c) for c in key_cols])]


def expected_pairs(lkeys, rkeys):
    """jt → sorted (li, ri) array with −1 for the outer side; a NULL in any key
    column matches nothing and the row survives on an outer side."""
    byk = defaultdict(list)
    for j, key in enumerate(rkeys):
        if key is not None:
            byk[key].append(j)
    inner = [(i, j) for i, key in enumerate(lkeys) if key is not None for j in byk.get(key, ())]
    lm = {i for i, _ in inner}
    rm = {j for _, j in inner}
    lo = [(i, -1) for i in range(len(lkeys)) if i not in lm]
    ro = [(-1, j) for j in range(len(rkeys)) if j not in rm]
    return {"inner": inner, "left_outer": inner + lo, "right_outer": inner + ro, "full_outer": inner + lo + ro}


def sorted_pairs(a, b):
    p = np.stack([np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)], axis=1)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def check_hash_join(session, lt, rt, lkeys, rkeys, key_pairs, jts):
    want = expected_pairs(lkeys, rkeys)
    nl, nr = len(lkeys), len(rkeys)
    for jt in jts:
        session.reset_profile()
        session.set_profiling(True)
        out = lt.join(rt, jt, *key_pairs)
        li, lok = out.column_arrays("li")
        ri, rok = out.column_arrays("ri")
        session.set_profiling(False)
        prof = session.profile()
        assert ("hash_build" in prof) == (nr > 0) and ("hash_probe" in prof) == (nl > 0 and nr > 0), (jt, prof)
        assert not any(name.startswith("rj_") for name in prof)
        got = sorted_pairs(np.where(lok, li, -1), np.where(rok, ri, -1))
        exp = sorted_pairs(*zip(*want[jt])) if want[jt] else np.zeros((0, 2), dtype=np.int64)
        assert got.shape == exp.shape and np.array_equal(got, exp), jt


JOIN_SIZES = [(0, 0), (0, 500), (500, 0), (1, 1000), (1000, 1), (50_000, 200_003)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["int_string", "int_bool", "int_int", "float", "for24"])
@pytest.mark.parametrize("sizes", JOIN_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_hash_join(gpu_session, monkeypatch, sizes, shape):
    """CAPF_JOIN=hash over multi-column keys with NULLs placed independently,
    a FLOAT key with ±0.0 / ±∞ / subnormals, and a FOR24 left key against a
    plain right key; one hot key on 5 % of the build (right) side and on a few
    probe rows."""
    monkeypatch.setenv("CAPF_JOIN", "hash")
    nl, nr = sizes
    rng = np.random.default_rng(nl * 7 + nr)
    dom = max(max(nl, nr) // 3, 1) + 7
    lkc, lcols = join_side(rng, nl, shape, dom, "l", min(nl, 10) if nl > 1 else 0)
    rkc, rcols = join_side(rng, nr, shape, dom, "r", nr // 20)
    lt, rt = gpu_session.table(lcols), gpu_session.table(rcols)
    if shape == "for24":
        lt = lt.compact(3)
        if nl > 0:
            assert lt.encoding("l0") == (2, FOR24_BASE)
        assert rt.encoding("r0")[0] == 0
    pairs = [(a[0], b[0]) for a, b in zip(lkc, rkc)]
    check_hash_join(gpu_session, lt, rt, join_keys_py(lkc), join_keys_py(rkc), pairs, JOIN_TYPES)


@pytest.mark.gpu
def test_hash_join_probe_above_grid_cap(gpu_session, monkeypatch):
    """BIG probe rows against 3000 build rows: the second trip of k_probe and k_join_emit."""
    monkeypatch.setenv("CAPF_JOIN", "hash")
    rng = np.random.default_rng(8)
    lkc, lcols = join_side(rng, BIG, "int_int", 9000, "l", 0)
    rkc, rcols = join_side(rng, 3000, "int_int", 9000, "r", 0)
    check_hash_join(gpu_session, gpu_session.table(lcols), gpu_session.table(rcols), join_keys_py(lkc),
                    join_keys_py(rkc), [("l0", "r0"), ("l1", "r1")], ["inner", "left_outer"])


WRAP_ROWS, WRAP_CAP = 3000, 8192


@functools.lru_cache(maxsize=None)
def wrap_keys():
    """600 present + 200 absent INTEGER keys whose home slot in the 8192-slot
    table (3000 build rows) is one of the last two: their chain runs past the
    last slot and goes on at slot 0."""
    assert rowhash.table_capacity(WRAP_ROWS) == WRAP_CAP
    found, start, step = [], 1, 1 << 21
    while len(found) < 800:
        w = np.arange(start, start + step, dtype=np.int64)
        found += w[rowhash.home_slot(w, WRAP_ROWS) >= WRAP_CAP - 2].tolist()
        start += step
    return np.array(found[:600], dtype=np.int64), np.array(found[600:800], dtype=np.int64)


@pytest.mark.gpu
def test_hash_join_wrapping_probe_chains(gpu_session, monkeypatch):
    monkeypatch.setenv("CAPF_JOIN", "hash")
    present, absent = wrap_keys()
    rk = np.tile(present, 5)  # 3000 build rows: capacity 8192, at most half full
    lk = np.concatenate([present, absent, np.zeros(50, dtype=np.int64)])
    lv = np.r_[np.ones(800, dtype=np.uint8), np.zeros(50, dtype=np.uint8)]
    lkc = [("l0", T_INT, lk, lv)]
    rkc = [("r0", T_INT, rk, None)]
    lt = gpu_session.table(lkc + [("li", T_INT, np.arange(len(lk), dtype=np.int64), None)])
    rt = gpu_session.table(rkc + [("ri", T_INT, np.arange(len(rk), dtype=np.int64), None)])
    check_hash_join(gpu_session, lt, rt, join_keys_py(lkc), join_keys_py(rkc), [("l0", "r0")], JOIN_TYPES)


def run_wrap_group_distinct(be):
    present, _ = wrap_keys()
    k = np.tile(present, 5)
    t = be.table([("k", T_INT, k, None), ("i", T_INT, np.arange(len(k), dtype=np.int64), None)])
    out = t.group([Var("k")], {"c": CountStar(), "lo": Min(Var("i")), "hi": Max(Var("i"))}, header=H("k", "i"),
                  params={})
    assert out.column_values("k") == present.tolist()
    assert out.column_values("c") == [5] * 600
    assert out.column_values("lo") == list(range(600))
    assert out.column_values("hi") == list(range(2400, 3000))
    assert t.distinct("k").column_values("i") == list(range(600))


@pytest.mark.gpu
def test_wrapping_chains_group_distinct(gpu_session):
    run_wrap_group_distinct(Gpu(gpu_session))


def test_wrapping_chains_group_distinct_oracle():
    run_wrap_group_distinct(Oracle())


# ================================================ E. oracle/rowhash.py pinned
def _fmix64_py(k):
    m = (1 << 64) - 1
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & m
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & m
    return k ^ (k >> 33)


def test_rowhash_wrap_keys_and_bijection():
    present, absent = wrap_keys()
    keys = np.concatenate([present, absent])
    assert len(np.unique(keys)) == 800
    for w in keys.tolist():  # plain-integer restatement: home slot among the last two
        assert (_fmix64_py(rowhash.SEED ^ w) & (WRAP_CAP - 1)) >= WRAP_CAP - 2
    assert [rowhash.table_capacity(n) for n in (0, 512, 513, 65536, 65537)] == [1024, 1024, 2048, 131072, 262144]
    sample = np.concatenate([np.arange(1 << 16, dtype=np.uint64),
                             np.random.default_rng(1).integers(0, 2 ** 63, 1 << 16).astype(np.uint64) << np.uint64(1)])
    sample = np.unique(sample)
    h = rowhash.fmix64(sample)
    assert len(np.unique(h)) == len(sample)  # inputs distinct → outputs distinct
    assert [int(x) for x in h[:4]] == [_fmix64_py(int(x)) for x in sample[:4]]
    assert int(rowhash.hash_row(np.array([I64_MIN]))[0]) == _fmix64_py(rowhash.SEED ^ (1 << 63))
