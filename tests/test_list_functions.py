"""LIST functions on the device: range, slices, head / last, reverse, list
concatenation and IN over a LIST column (capf_table_list_fn, CAPF_OP_IN_LIST).

The CPU oracle does not know these expressions, so the expectations come from
the small Python model below — the definitions in expr.py's docstrings (the
Morpheus lowering, SparkSQLExprMapper.scala:161-182, 265, 269, 336-338) written
with Python lists — and from the 20 reference cases transcribed in
tests/golden/list_function_cases.py.  Lists are compared with ==, element
order and value types included (`typed`: 5.0 is not 5); conftest.bag sorts
lists and would hide a wrong order.
"""
import random

import numpy as np
import pytest

from conftest import case_parts
from list_function_cases import CASES

from capf_amd import _lib
from capf_amd.expr import (OP_COL, OP_EQ, OP_IN_LIST, OP_LIST_INDEX, OP_LIT_INT, OP_OR, Add, Collect, ContainerIndex,
                           ElementProperty, Equals, Explode, Head, In, IntegerLit, Last, ListLit, ListSliceFrom,
                           ListSliceFromTo, ListSliceTo, Modulo, NullLit, Range, Reverse, Size, StringLit, Var,
                           BoolLit, FloatLit, T_BOOL, T_FLOAT, T_INT, T_LIST, T_NULL, T_STRING, compile_program)
from capf_amd.header import RecordHeader

COLS = ["k", "g", "x", "y", "s", "f", "b", "xs", "ys", "fs", "z", "z0", "lo", "hi", "a", "st", "e"]
H = RecordHeader({Var(c): c for c in COLS})
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
ABSENT = "absent"


def I(v):  # noqa: E743
    return IntegerLit(v)


def typed(v):
    """A value with its type spelled out, lists in order: typed(5.0) != typed(5)."""
    if isinstance(v, (list, tuple)):
        return ("list", tuple(typed(x) for x in v))
    return (type(v).__name__, v)


def same(got, want):
    return typed(got) == typed(want)


# ------------------------------------------------------------------ the model
def m_slice(xs, lo=ABSENT, hi=ABSENT):
    if xs is None or not xs or lo is None or hi is None:
        return None  # a NULL list, an EMPTY list or a NULL bound
    return xs[(None if lo is ABSENT else lo):(None if hi is ABSENT else hi)]


def m_reverse(xs):
    return None if xs is None else xs[::-1]


def m_range(a, b, s=1):
    if a is None or b is None or s is None:
        return None
    if s == 0:
        raise ValueError("step 0")
    out = range(a, b + 1, s) if s > 0 else range(a, b - 1, s)
    if len(out) > 2 ** 31 - 1:
        raise ValueError("too long")
    return list(out)


def m_concat(a, b, a_list=True, b_list=True):
    a = a if a_list else [a]
    b = b if b_list else [b]
    return None if a is None or b is None else a + b


def m_in(x, xs, comparable=True):
    if xs is None:
        return None
    if not xs:
        return False
    if x is None or not comparable:
        return None
    if any(e is not None and e == x for e in xs):
        return True
    return None if any(e is None for e in xs) else False


def m_index(xs, i):
    if xs is None or i is None or not -len(xs) <= i < len(xs):
        return None
    return xs[i]


def m_size(xs):
    return None if xs is None else len(xs)


def m_eval(e, env):
    """The model over an expression tree (the classes the reference cases use)."""
    cls = type(e).__name__
    if cls in ("IntegerLit", "StringLit", "FloatLit", "BoolLit"):
        return e.v
    if cls == "NullLit":
        return None
    if cls == "Var":
        return env[e.vname]
    if cls == "ElementProperty":
        return env[e.key]
    if cls == "ListLit":
        return [m_eval(x, env) for x in e.items]
    if cls == "Head":
        return m_index(m_eval(e.expr, env), 0)
    if cls == "Last":
        return m_index(m_eval(e.expr, env), -1)
    if cls == "Reverse":
        return m_reverse(m_eval(e.expr, env))
    if cls == "Range":
        return m_range(m_eval(e.frm, env), m_eval(e.to, env), 1 if e.step is None else m_eval(e.step, env))
    if cls == "ListSliceFromTo":
        return m_slice(m_eval(e.list, env), m_eval(e.frm, env), m_eval(e.to, env))
    if cls == "ListSliceFrom":
        return m_slice(m_eval(e.list, env), m_eval(e.frm, env))
    if cls == "ListSliceTo":
        return m_slice(m_eval(e.list, env), hi=m_eval(e.to, env))
    raise NotImplementedError(cls)


CASE_ROWS = {"range_columns": [{"from": 1, "to": 2}, {"from": 1, "to": 3}, {"from": 1, "to": 4}],
             "range_varying_step": [{"step": 2}, {"step": 3}]}


def m_query(cid, q):
    rows = CASE_ROWS.get(cid, [{}])
    for m in q.matches:
        if type(m).__name__ == "Unwind":
            rows = [{**r, m.alias: v} for r in rows for v in (m_eval(m.list, r) or [])]
    for st in q.stages:
        rows = [{a: m_eval(e, r) for a, e in st.items} for r in rows]
    return rows


def rows_key(rows):
    return sorted(repr(sorted((k, typed(v)) for k, v in r.items())) for r in rows)


# ------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_model_agrees_with_reference_case(case):
    cid, src, create, query, expected, opts = case_parts(case)
    assert rows_key(m_query(cid, query)) == rows_key(expected), (cid, src)


def test_model_slices_are_python_slices():
    xs = [1, 2, 3, 4, 5]
    assert m_slice(xs, 1, -1) == [2, 3, 4] and m_slice(xs, -9, 9) == xs and m_slice(xs, 3, 1) == []
    assert m_slice([], 0, 1) is None and m_slice(None, 0, 1) is None and m_slice(xs, None, 1) is None
    assert m_range(INT64_MIN, INT64_MAX, INT64_MAX) == [INT64_MIN, -1, INT64_MAX - 1]
    assert m_range(3, 1) == [] and m_range(3, 1, -1) == [3, 2, 1] and m_range(1, 3, -1) == []


TYPES = {"xs": T_LIST, ("elem", "xs"): T_INT, "k": T_INT, "x": T_INT, "s": T_STRING}


def _compile(e, types=None, params=None):
    types = types or TYPES
    codes = {}
    return compile_program(e, H, {c for c in types if isinstance(c, str)}, params or {},
                           lambda x: codes.setdefault(x, 100 + len(codes)), lambda c: types[c])


def test_head_last_lower_onto_list_index():
    for e, ix in ((Head(Var("xs")), 0), (Last(Var("xs")), -1)):
        ops, ia, fa, names = _compile(e)
        assert list(ops) == [OP_LIT_INT, OP_LIST_INDEX] and ia[0] == ix
        assert names[ia[1]] == "xs" and fa[1] == float(T_INT)
        assert tuple(map(list, _compile(e)[:3])) == tuple(map(list, _compile(ContainerIndex(Var("xs"), I(ix)))[:3]))
    # a literal list folds; an empty or NULL list gives NULL
    assert (list(_compile(Head(ListLit(I(4), I(5))))[0]), list(_compile(Last(ListLit(I(4), I(5))))[1])) == \
        ([OP_LIT_INT], [5])
    for e in (Head(ListLit()), Last(ListLit()), Head(NullLit()), Last(NullLit())):
        assert list(_compile(e)[0]) == [6], str(e)  # OP_LIT_NULL


def test_in_over_a_list_column_lowers_onto_in_list():
    ops, ia, fa, names = _compile(In(Var("k"), Var("xs")))
    assert list(ops) == [OP_COL, OP_IN_LIST]
    assert names[ia[0]] == "k" and names[ia[1]] == "xs" and fa[1] == float(T_INT)
    # a NULL-typed column on the right: NULL
    ops, ia, _, _ = _compile(In(Var("k"), Var("xs")), types={"xs": T_NULL, "k": T_INT})
    assert (list(ops), list(ia)) == ([6], [T_BOOL])
    # a per-row list expression is no column yet: the table operations project it first
    with pytest.raises(_lib.NotImplementedException):
        _compile(In(Var("k"), Reverse(Var("xs"))))


def test_literal_list_in_keeps_its_program():
    """A literal-list IN gives exactly the program it gave before CAPF_OP_IN_LIST
    existed: the left-folded OR of equalities (written out here)."""
    ops, ia, fa, names = _compile(In(Var("k"), ListLit(I(1), I(2), I(3))))
    assert list(ops) == [OP_COL, OP_LIT_INT, OP_EQ, OP_COL, OP_LIT_INT, OP_EQ, OP_OR, OP_COL, OP_LIT_INT, OP_EQ, OP_OR]
    assert list(ia) == [0, 1, 0, 0, 2, 0, 2, 0, 3, 0, 2] and list(names) == ["k"] and not any(fa)
    assert list(_compile(In(Var("k"), ListLit()))[0]) == [4]  # OP_LIT_BOOL FALSE
    assert OP_IN_LIST not in _compile(In(Var("s"), ListLit(StringLit("a"), NullLit())))[0]


def test_scala_twin_names_the_classes_and_the_entry_point():
    import okapi_scala_scan as sc
    srcs = sc.integration_sources()
    mapper, table, native = (sc.strip_comments(srcs[f]) for f in
                             ("GpuExprMapper.scala", "GpuTable.scala", "Native.scala"))
    assert "OpInList = 97" in native and "Native.OpInList" in mapper
    for k, name in enumerate(("ListFnSlice", "ListFnReverse", "ListFnConcat", "ListFnRange")):
        assert f"{name} = {k}" in native and f"Native.{name}" in table
    for cls in ("Head", "Last"):
        assert f": {cls} =>" in mapper
    for cls in ("Reverse", "Range", "ListSliceFromTo", "ListSliceFrom", "ListSliceTo", "Add"):
        assert f": {cls}" in table
    assert "Native.tableListFn(" in table


# ------------------------------------------------------- GPU: reference cases
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_case_on_gpu(gpu_session, case):
    from capf_amd.graph import ScanGraph
    from capf_amd.planner import run
    from oracle.create_parser import parse_create
    cid, src, create, query, expected, opts = case_parts(case)
    got = run(ScanGraph.from_data(gpu_session, parse_create(create)), query, opts.get("params"))
    assert rows_key(got) == rows_key(expected), f"{cid} ({src}): {got}"


# ------------------------------------------------------ GPU: fixed edge table
def with_col(t, e, name="z"):
    return t.withColumns((e, name), header=H, params={})


def values(t, e):
    out = with_col(t, e, "z")
    assert [c for c in out.physicalColumns if c.startswith("\x03")] == [], out.physicalColumns
    return out.column_values("z")


ELEMS = {  # four values per element type
    T_INT: [1, 2, 3, 4], T_FLOAT: [0.5, 1.5, -2.0, 4.25], T_BOOL: [True, False, True, True],
    T_STRING: ["a", "bb", "", "d"],
}


def edge_lists(et):
    """A NULL list, [], [e], [None], NULLs first / in the middle / last, a longer list."""
    if et == T_NULL:
        return [None, [], [None], [None, None, None]]
    a, b, c, d = ELEMS[et]
    return [None, [], [a], [None], [None, a, b], [a, None, b], [a, b, None], [c, a, b, d, a], [None, None]]


def edge_table(sess, et, extra=()):
    xs = edge_lists(et)
    n = len(xs)
    return sess.table([("k", T_INT, list(range(n)), None), ("xs", T_LIST, xs, None)] + list(extra), nrows=n), xs


ALL_TYPES = [T_INT, T_FLOAT, T_BOOL, T_STRING, T_NULL]
TYPE_IDS = ["int", "float", "bool", "string", "nulltyped"]
BOUNDS = [ABSENT, None, -9, -2, -1, 0, 1, 2, 9]


def slice_expr(xs, lo, hi):
    le = NullLit() if lo is None else lo if not isinstance(lo, int) else I(lo)
    he = NullLit() if hi is None else hi if not isinstance(hi, int) else I(hi)
    if lo is ABSENT and hi is ABSENT:
        return None
    if hi is ABSENT:
        return ListSliceFrom(xs, le)
    if lo is ABSENT:
        return ListSliceTo(xs, he)
    return ListSliceFromTo(xs, le, he)


@pytest.mark.gpu
@pytest.mark.parametrize("et", ALL_TYPES, ids=TYPE_IDS)
def test_slices_with_literal_bounds(gpu_session, et):
    t, xs = edge_table(gpu_session, et)
    combos = [(lo, hi) for lo in BOUNDS for hi in BOUNDS if (lo, hi) != (ABSENT, ABSENT)]
    items = [(slice_expr(Var("xs"), lo, hi), f"c{i}") for i, (lo, hi) in enumerate(combos)]
    out = t.withColumns(*items, header=H, params={})
    assert out.physicalColumns == ["k", "xs"] + [c for _, c in items]
    for (lo, hi), (_, c) in zip(combos, items):
        got = out.column_values(c)
        assert same(got, [m_slice(x, lo, hi) for x in xs]), (lo, hi, got)
        if out.capf_type(c) == T_LIST:
            assert out.list_elem_type(c) == et


@pytest.mark.gpu
@pytest.mark.parametrize("et", ALL_TYPES, ids=TYPE_IDS)
def test_slices_with_column_bounds(gpu_session, et):
    xs0 = edge_lists(et)
    bs = [b for b in BOUNDS if b is not ABSENT]
    rows = [(x, lo, hi) for x in xs0 for lo in bs for hi in bs]
    n = len(rows)
    t = gpu_session.table([("k", T_INT, list(range(n)), None), ("xs", T_LIST, [r[0] for r in rows], None),
                           ("lo", T_INT, [r[1] for r in rows], None), ("hi", T_INT, [r[2] for r in rows], None)],
                          nrows=n)
    assert same(values(t, ListSliceFromTo(Var("xs"), Var("lo"), Var("hi"))), [m_slice(*r) for r in rows])
    assert same(values(t, ListSliceFrom(Var("xs"), Var("lo"))), [m_slice(r[0], r[1]) for r in rows])
    assert same(values(t, ListSliceTo(Var("xs"), Var("hi"))), [m_slice(r[0], hi=r[2]) for r in rows])
    # a column on one side, a literal on the other
    assert same(values(t, ListSliceFromTo(Var("xs"), I(1), Var("hi"))), [m_slice(r[0], 1, r[2]) for r in rows])


@pytest.mark.gpu
@pytest.mark.parametrize("et", ALL_TYPES, ids=TYPE_IDS)
def test_reverse_head_last_over_the_edge_table(gpu_session, et):
    t, xs = edge_table(gpu_session, et)
    out = with_col(t, Reverse(Var("xs")), "z")
    assert same(out.column_values("z"), [m_reverse(x) for x in xs])
    assert out.list_elem_type("z") == et
    assert same(values(t, Head(Var("xs"))), [m_index(x, 0) for x in xs])
    assert same(values(t, Last(Var("xs"))), [m_index(x, -1) for x in xs])
    assert same(values(t, Head(Reverse(Var("xs")))), [m_index(x, -1) for x in xs])


@pytest.mark.gpu
def test_reverse_of_a_string_stays_not_implemented(gpu_session):
    t = gpu_session.table([("s", T_STRING, ["ab", "c"], None)])
    with pytest.raises(_lib.NotImplementedException):
        with_col(t, Reverse(Var("s"))).column_values("z")


RANGE_ROWS = [  # (from, to, step)
    (1, 4, 1), (1, 4, 2), (1, 4, 3), (4, 1, -1), (4, 1, -2), (4, 1, 1), (1, 4, -1), (0, 0, 5), (0, 0, -5),
    (-3, 3, 2), (3, -3, -4), (None, 4, 1), (1, None, 1), (1, 4, None), (7, 7, 1), (5, 4, 1),
    (INT64_MIN, INT64_MAX, INT64_MAX), (INT64_MAX, INT64_MIN, INT64_MIN), (INT64_MAX - 2, INT64_MAX, 1),
    (INT64_MIN + 2, INT64_MIN, -1), (INT64_MAX, INT64_MAX, INT64_MAX), (INT64_MIN, INT64_MIN, INT64_MIN),
]


def range_table(sess, rows):
    n = len(rows)
    return sess.table([("k", T_INT, list(range(n)), None), ("a", T_INT, [r[0] for r in rows], None),
                       ("b", T_INT, [r[1] for r in rows], None), ("st", T_INT, [r[2] for r in rows], None)], nrows=n)


@pytest.mark.gpu
def test_range_over_columns(gpu_session):
    t = range_table(gpu_session, RANGE_ROWS)
    out = with_col(t, Range(Var("a"), Var("b"), Var("st")))
    assert same(out.column_values("z"), [m_range(*r) for r in RANGE_ROWS])
    assert out.list_elem_type("z") == T_INT and out.list_arrays("z")[4] is None
    small = [r for r in RANGE_ROWS if r[0] is None or r[1] is None or abs(r[0]) < 100]
    t = range_table(gpu_session, small)
    assert same(values(t, Range(Var("a"), Var("b"))), [m_range(r[0], r[1]) for r in small])
    assert same(values(t, Range(Var("a"), Var("b"), I(-2))), [m_range(r[0], r[1], -2) for r in small])
    assert same(values(t, Range(I(2), Var("b"), Var("st"))), [m_range(2, r[1], r[2]) for r in small])
    assert same(values(t, Range(Var("a"), Var("b"), NullLit())), [None] * len(small))
    assert same(values(t, Range(NullLit(), Var("b"))), [None] * len(small))


@pytest.mark.gpu
def test_range_does_not_wrap(gpu_session):
    t = range_table(gpu_session, [(INT64_MIN, INT64_MAX, INT64_MAX)])
    assert same(values(t, Range(Var("a"), Var("b"), Var("st"))), [[INT64_MIN, -1, INT64_MAX - 1]])
    assert same(values(t, Range(I(INT64_MIN), I(INT64_MAX), I(INT64_MAX))), [[INT64_MIN, -1, INT64_MAX - 1]])


@pytest.mark.gpu
@pytest.mark.parametrize("bad,row", [("step0", (1, 4, 0)), ("long", (0, 2 ** 31 - 1, 1)),
                                      ("long_full", (INT64_MIN, INT64_MAX, 1)), ("long_down", (0, -2 ** 31 + 1, -1))])
def test_range_errors_when_the_plan_executes(gpu_session, bad, row):
    """Only one row offends; the error comes when the plan executes, not when it is built."""
    rows = [(1, 3, 1), (5, 1, -2), row, (2, 2, 1)]
    out = with_col(range_table(gpu_session, rows), Range(Var("a"), Var("b"), Var("st")))  # built: no error
    with pytest.raises(_lib.IllegalArgumentException):
        out.column_values("z")
    ok = [r for r in rows if r != row] + [(0, 2 ** 31 - 2, 2 ** 30)]
    assert same(values(range_table(gpu_session, ok), Range(Var("a"), Var("b"), Var("st"))), [m_range(*r) for r in ok])


def concat_table(sess):
    xs = [None, [], [1], [None], [1, None, 2], [3, 4], [5], [None, 6]]
    ys = [[1], None, [], [2, None], [None], [7, 8, 9], [], [None]]
    fs = [[0.5], [1.5, None], None, [], [2.5], [None], [3.5, 4.5], []]
    ns = [[None], [], None, [None, None], [], [None], [], [None]]
    ss = [["a"], [], None, ["b", None], [], ["c"], [], [None]]
    n = len(xs)
    t = sess.table([("k", T_INT, list(range(n)), None), ("x", T_INT, [None, 1, 2, None, 4, 5, None, 7], None),
                    ("f", T_FLOAT, [0.5, None, 2.5, None, 4.5, 5.5, 6.5, None], None),
                    ("s", T_STRING, ["p", None, "q", "r", None, "s", "t", "u"], None),
                    ("xs", T_LIST, xs, None), ("ys", T_LIST, ys, None), ("fs", T_LIST, fs, None),
                    ("e", T_LIST, ns, None), ("z0", T_LIST, ss, None)], nrows=n)
    return t, dict(xs=xs, ys=ys, fs=fs, ns=ns, ss=ss, x=[None, 1, 2, None, 4, 5, None, 7],
                   f=[0.5, None, 2.5, None, 4.5, 5.5, 6.5, None], s=["p", None, "q", "r", None, "s", "t", "u"])


def widen(xs):
    return None if xs is None else [None if v is None else float(v) for v in xs]


@pytest.mark.gpu
def test_concat(gpu_session):
    t, d = concat_table(gpu_session)
    n = len(d["xs"])
    X, Y, F, E = Var("xs"), Var("ys"), Var("fs"), Var("e")
    # list + list, list + scalar, scalar + list (a NULL scalar appends a NULL element)
    assert same(values(t, Add(X, Y)), [m_concat(a, b) for a, b in zip(d["xs"], d["ys"])])
    assert same(values(t, Add(X, X)), [m_concat(a, a) for a in d["xs"]])
    assert same(values(t, Add(X, Var("x"))), [m_concat(a, b, b_list=False) for a, b in zip(d["xs"], d["x"])])
    assert same(values(t, Add(Var("x"), X)), [m_concat(a, b, a_list=False) for a, b in zip(d["x"], d["xs"])])
    assert same(values(t, Add(X, I(9))), [m_concat(a, 9, b_list=False) for a in d["xs"]])
    assert same(values(t, Add(X, NullLit())), [m_concat(a, None, b_list=False) for a in d["xs"]])
    assert same(values(t, Add(X, ListLit(I(8), NullLit()))), [m_concat(a, [8, None]) for a in d["xs"]])
    assert same(values(t, Add(ListLit(Var("x"), I(3)), X)), [m_concat([v, 3], a) for v, a in zip(d["x"], d["xs"])])
    # INTEGER with FLOAT widens to FLOAT per column
    out = with_col(t, Add(X, F))
    assert out.list_elem_type("z") == T_FLOAT
    assert same(out.column_values("z"), [m_concat(widen(a), b) for a, b in zip(d["xs"], d["fs"])])
    assert same(values(t, Add(F, X)), [m_concat(a, widen(b)) for a, b in zip(d["fs"], d["xs"])])
    assert same(values(t, Add(X, Var("f"))), [m_concat(widen(a), b, b_list=False) for a, b in zip(d["xs"], d["f"])])
    assert same(values(t, Add(Var("x"), F)),
                [m_concat(None if a is None else float(a), b, a_list=False) for a, b in zip(d["x"], d["fs"])])
    # a NULL-typed side takes the other side's type
    out = with_col(t, Add(E, X))
    assert out.list_elem_type("z") == T_INT
    assert same(out.column_values("z"), [m_concat(a, b) for a, b in zip(d["ns"], d["xs"])])
    assert same(values(t, Add(Var("z0"), E)), [m_concat(a, b) for a, b in zip(d["ss"], d["ns"])])
    out = with_col(t, Add(E, E))
    assert out.list_elem_type("z") == T_NULL
    assert same(out.column_values("z"), [m_concat(a, a) for a in d["ns"]])
    assert same(values(t, Add(Var("z0"), Var("s"))), [m_concat(a, b, b_list=False) for a, b in zip(d["ss"], d["s"])])
    # strings and booleans
    b = gpu_session.table([("xs", T_LIST, [[True], [False, None], None], None), ("b", T_BOOL, [False, None, True], None)],
                          nrows=3)
    hb = RecordHeader({Var("xs"): "xs", Var("b"): "b"})
    got = b.withColumns((Add(Var("b"), Var("xs")), "z"), header=hb, params={}).column_values("z")
    assert same(got, [[False, True], [None, False, None], None])
    # lists of different inner types are not supported
    for e in (Add(X, Var("s")), Add(X, Var("z0")), Add(Var("s"), F), Add(X, StringLit("a")), Add(X, BoolLit(True))):
        with pytest.raises(_lib.NotImplementedException):
            with_col(t, e).column_values("z")
    assert n == 8


@pytest.mark.gpu
def test_in_over_list_columns(gpu_session):
    t, d = concat_table(gpu_session)
    X = Var("xs")
    assert same(values(t, In(Var("x"), X)), [m_in(a, b) for a, b in zip(d["x"], d["xs"])])
    assert same(values(t, In(Var("k"), X)), [m_in(a, b) for a, b in zip(range(8), d["xs"])])
    for lit in (1, 2, 6, 99):
        assert same(values(t, In(I(lit), X)), [m_in(lit, b) for b in d["xs"]]), lit
    assert same(values(t, In(NullLit(), X)), [m_in(None, b) for b in d["xs"]])
    # INTEGER x against a FLOAT list (numeric equality), FLOAT x against an INTEGER list
    fl = [[1.0, 2.5], [1.5, None], None, [], [4.0], [None], [6.0, 4.5], []]
    t2 = gpu_session.table([("x", T_INT, d["x"], None), ("f", T_FLOAT, d["f"], None), ("fs", T_LIST, fl, None),
                            ("xs", T_LIST, d["xs"], None)], nrows=8)
    assert same(values(t2, In(Var("x"), Var("fs"))), [m_in(a, b) for a, b in zip(d["x"], fl)])
    assert same(values(t2, In(FloatLit(4.0), Var("fs"))), [m_in(4.0, b) for b in fl])
    assert same(values(t2, In(FloatLit(1.0), Var("xs"))), [m_in(1.0, b) for b in d["xs"]])
    # STRING and BOOLEAN
    assert same(values(t, In(Var("s"), Var("z0"))), [m_in(a, b) for a, b in zip(d["s"], d["ss"])])
    assert same(values(t, In(StringLit("b"), Var("z0"))), [m_in("b", b) for b in d["ss"]])
    bl = [[True], [False, None], None, [], [None], [False], [True, False], [None, True]]
    bx = [True, True, False, None, True, False, None, False]
    t3 = gpu_session.table([("b", T_BOOL, bx, None), ("xs", T_LIST, bl, None)], nrows=8)
    h3 = RecordHeader({Var("xs"): "xs", Var("b"): "b"})
    got = t3.withColumns((In(Var("b"), Var("xs")), "z"), header=h3, params={}).column_values("z")
    assert same(got, [m_in(a, b) for a, b in zip(bx, bl)])
    # incomparable types: NULL — after the NULL-list and empty-list answers
    assert same(values(t, In(Var("x"), Var("z0"))), [m_in(a, b, False) for a, b in zip(d["x"], d["ss"])])
    assert same(values(t, In(Var("s"), X)), [m_in(a, b, False) for a, b in zip(d["s"], d["xs"])])
    assert same(values(t, In(BoolLit(True), X)), [m_in(True, b, False) for b in d["xs"]])
    # NULL-typed elements
    assert same(values(t, In(Var("x"), Var("e"))), [m_in(a, b) for a, b in zip(d["x"], d["ns"])])


# --------------------------------------------------------- GPU: composition
@pytest.mark.gpu
def test_composition(gpu_session):
    t, d = concat_table(gpu_session)
    X, x, k = Var("xs"), Var("x"), Var("k")
    tail = ListSliceFrom(X, I(1))
    assert same(values(t, Size(tail)), [m_size(m_slice(a, 1)) for a in d["xs"]])
    assert same(values(t, Head(Reverse(X))), [m_index(m_reverse(a), 0) for a in d["xs"]])
    assert same(values(t, Last(Add(X, x))), [m_index(m_concat(a, b, b_list=False), -1) for a, b in zip(d["xs"], d["x"])])
    assert same(values(t, In(x, Range(I(1), k))), [m_in(a, m_range(1, b)) for a, b in zip(d["x"], range(8))])
    assert same(values(t, In(x, Range(k, I(5)))), [m_in(a, m_range(b, 5)) for a, b in zip(d["x"], range(8))])
    assert same(values(t, In(x, ListLit(k, I(3)))), [m_in(a, [b, 3]) for a, b in zip(d["x"], range(8))])
    assert same(values(t, In(I(3), ListLit(k, x))), [m_in(3, [b, a]) for a, b in zip(d["x"], range(8))])
    assert same(values(t, Reverse(Reverse(tail))), [m_slice(a, 1) for a in d["xs"]])
    assert same(values(t, Size(Add(Reverse(X), ListSliceTo(X, I(-1))))),
                [m_size(m_concat(m_reverse(a), m_slice(a, hi=-1))) for a in d["xs"]])
    # WHERE x IN xs[1..]
    f = t.filter(In(x, tail), header=H, params={})
    assert f.physicalColumns == t.physicalColumns
    keep = [i for i in range(8) if m_in(d["x"][i], m_slice(d["xs"][i], 1)) is True]
    assert f.column_values("k") == keep
    # two list items and a scalar one in one call; nothing temporary survives
    out = t.withColumns((Reverse(X), "r"), (Add(k, I(1)), "k1"), (tail, "tl"), header=H, params={})
    assert out.physicalColumns == t.physicalColumns + ["r", "k1", "tl"]
    assert same(out.column_values("r"), [m_reverse(a) for a in d["xs"]])
    assert same(out.column_values("tl"), [m_slice(a, 1) for a in d["xs"]]) and out.column_values("k1") == list(range(1, 9))
    # UNWIND range(1, 7, 3)
    u = gpu_session.table([("k", T_INT, [10, 20], None)]).withColumns((Explode(Range(I(1), I(7), I(3))), "e"),
                                                                      header=H, params={})
    assert u.physicalColumns == ["k", "e"]
    assert same([(r["k"], r["e"]) for r in u.rows], [(10, 1), (10, 4), (10, 7), (20, 1), (20, 4), (20, 7)])
    # orderBy arguments are not hoisted: they keep raising
    with pytest.raises(_lib.NotImplementedException):
        t.orderBy((Reverse(X), "asc"), header=H, params={}).size


# ---------------------------------------------------- GPU: seeded random chains
def _chain(sess, seed):
    rnd = random.Random(seed)
    n = 60
    ks = list(range(n))
    xv = [rnd.choice([None, 0, 1, 2, 3, 4]) for _ in ks]
    yv = [rnd.choice([None, 1, 2, 5]) for _ in ks]
    t = sess.table([("k", T_INT, ks, None), ("x", T_INT, xv, None), ("y", T_INT, yv, None)], nrows=n)
    if seed % 2:  # a literal over nullable items
        t = t.withColumns((ListLit(Var("x"), Var("y"), Var("k"), Var("x")), "xs"), header=H, params={})
        rows = [dict(k=k, x=x, xs=[x, y, k, x]) for k, x, y in zip(ks, xv, yv)]
        t = t.select("k", "x", "xs")
    else:  # collect(y) per x: ascending, no NULLs, a NULL key is its own group
        g = t.group([Var("x")], {"xs": Collect(Var("y"))}, header=H, params={})
        g = g.withColumns((Var("x"), "k"), header=H, params={}).select("k", "x", "xs")
        groups = {}
        for x, y in zip(xv, yv):
            groups.setdefault(x, []).extend([] if y is None else [y])
        rows = [dict(k=x, x=x, xs=sorted(v)) for x, v in groups.items()]
        t = g
    for _ in range(rnd.randint(1, 3)):
        op = rnd.choice(["slice", "reverse", "concat", "select", "filter", "orderBy", "union"])
        X = Var("xs")
        if op == "slice":
            lo, hi = rnd.choice([ABSENT, -2, 0, 1, 2]), rnd.choice([ABSENT, -1, 1, 3, 9])
            e = slice_expr(X, lo, hi) or ListSliceFrom(X, I(0))
            if lo is ABSENT and hi is ABSENT:
                lo = 0
            rows = [{**r, "xs": m_slice(r["xs"], lo, hi)} for r in rows]
        elif op == "reverse":
            e = Reverse(X)
            rows = [{**r, "xs": m_reverse(r["xs"])} for r in rows]
        elif op == "concat":
            how = rnd.choice(["self", "scalar", "front"])
            e = Add(X, X) if how == "self" else Add(X, Var("x")) if how == "scalar" else Add(Var("x"), X)
            rows = [{**r, "xs": m_concat(r["xs"], r["xs"]) if how == "self" else
                     m_concat(r["xs"], r["x"], b_list=False) if how == "scalar" else
                     m_concat(r["x"], r["xs"], a_list=False)} for r in rows]
        if op in ("slice", "reverse", "concat"):
            t = t.withColumns((e, "ys"), header=H, params={}).select(("k", "k"), ("x", "x"), ("ys", "xs"))
        elif op == "select":
            t = t.select("xs", "x", "k")
        elif op == "filter":
            t = t.filter(Equals(Modulo(Var("k"), I(3)), I(1)), header=H, params={})
            rows = [r for r in rows if r["k"] is not None and r["k"] % 3 == 1]
        elif op == "orderBy":
            t = t.orderBy((Var("k"), "desc"), header=H, params={})  # (rows are compared sorted below)
        else:
            t = t.unionAll(t)
            rows = rows + rows
    return t, rows


@pytest.mark.gpu
@pytest.mark.parametrize("group", range(8))
def test_random_chains(gpu_session, group):
    for seed in range(group * 10, group * 10 + 10):
        t, rows = _chain(gpu_session, seed)
        X, x = Var("xs"), Var("x")
        obs = [("size", Size(X), lambda r: m_size(r["xs"])), ("head", Head(X), lambda r: m_index(r["xs"], 0)),
               ("last", Last(X), lambda r: m_index(r["xs"], -1)), ("in", In(x, X), lambda r: m_in(r["x"], r["xs"]))]
        obs += [(f"ix{i}", ContainerIndex(X, I(i)), (lambda r, i=i: m_index(r["xs"], i))) for i in (-2, 0, 1)]
        out = t.withColumns(*[(e, nm) for nm, e, _ in obs], header=H, params={})
        cols = {c: out.column_values(c) for c in ["k", "xs"] + [nm for nm, _, _ in obs]}
        got = sorted(repr([typed(cols[c][i]) for c in cols]) for i in range(len(cols["k"])))
        want = sorted(repr([typed(r["k"]), typed(r["xs"])] + [typed(f(r)) for _, _, f in obs]) for r in rows)
        assert got == want, seed


# ------------------------------------- GPU: shapes where the fill can go wrong
def _list_table(sess, lists):
    n = len(lists)
    return sess.table([("k", T_INT, np.arange(n, dtype=np.int64), None), ("xs", T_LIST, lists, None)], nrows=n)


def _arrays(lists, conv=np.int64):
    """(offsets, values, list validity) numpy arrays of python lists (None: a NULL list)."""
    lens = np.array([0 if x is None else len(x) for x in lists], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    vals = np.array([v for x in lists if x for v in x], dtype=conv) if lens.sum() else np.zeros(0, dtype=conv)
    return offs, vals, np.array([x is not None for x in lists], dtype=np.uint8)


def _check_buffers(out, col, want, elem_valid_absent=True):
    et, offs, vals, valid, ev = out.list_arrays(col)
    wo, wv, wok = _arrays(want)
    assert et == T_INT
    assert np.array_equal(offs, wo) and np.array_equal(vals, wv), col
    assert np.array_equal(valid.astype(np.uint8), wok), col
    if elem_valid_absent:
        assert ev is None, col


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_row_counts_around_a_block(gpu_session, n):
    lists = [list(range(r, r + r % 5)) for r in range(n)]
    t = _list_table(gpu_session, lists)
    out = t.withColumns((Reverse(Var("xs")), "r"), (ListSliceFrom(Var("xs"), I(1)), "s"), (Add(Var("xs"), Var("k")), "c"),
                        (Range(Var("k"), Add(Var("k"), I(2))), "g"), header=H, params={})
    assert out.size == n
    _check_buffers(out, "r", [m_reverse(x) for x in lists])
    _check_buffers(out, "s", [m_slice(x, 1) for x in lists])
    _check_buffers(out, "c", [x + [r] for r, x in enumerate(lists)])
    _check_buffers(out, "g", [[r, r + 1, r + 2] for r in range(n)])


@pytest.mark.gpu
def test_runs_of_empty_rows(gpu_session):
    lists = [[] for _ in range(1000)]
    lists[0], lists[499], lists[999] = [1, 2, 3], [4, 5], [6, 7, 8, 9]
    t = _list_table(gpu_session, lists)
    out = t.withColumns((Reverse(Var("xs")), "r"), (ListSliceFromTo(Var("xs"), I(1), I(9)), "s"),
                        (Add(Var("xs"), Var("xs")), "c"), header=H, params={})
    _check_buffers(out, "r", [m_reverse(x) for x in lists])
    _check_buffers(out, "s", [m_slice(x, 1, 9) for x in lists])
    _check_buffers(out, "c", [x + x for x in lists])


@pytest.mark.gpu
def test_one_list_longer_than_a_block_span(gpu_session):
    big = list(range(70000))
    lists = [[] for _ in range(40)]
    lists[17] = big
    t = _list_table(gpu_session, lists)
    out = t.withColumns((Reverse(Var("xs")), "r"), (ListSliceFromTo(Var("xs"), I(1), I(-1)), "s"),
                        (Add(Var("xs"), Var("xs")), "c"), header=H, params={})
    _check_buffers(out, "r", [m_reverse(x) for x in lists])
    _check_buffers(out, "s", [m_slice(x, 1, -1) for x in lists])
    _check_buffers(out, "c", [x + x for x in lists])


@pytest.mark.gpu
def test_range_past_the_grid_cap(gpu_session):
    """2^20 + 3 elements: more than the 4096 x 256 elements one sweep of the fill
    grid covers, so its grid-stride step runs twice."""
    ks = np.full(1025, 1023, dtype=np.int64)
    ks[700] = 2
    t = gpu_session.table([("k", T_INT, ks, None)], nrows=len(ks))
    out = t.withColumns((Range(I(0), Var("k")), "g"), header=H, params={})
    et, offs, vals, valid, ev = out.list_arrays("g")
    lens = ks + 1
    assert lens.sum() == 2 ** 20 + 3 and et == T_INT and ev is None and valid.all()
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum(lens)]))
    assert np.array_equal(vals, np.concatenate([np.arange(m, dtype=np.int64) for m in lens]))


@pytest.mark.gpu
def test_list_fn_binding_type_checks(gpu_session):
    """capf_table_list_fn rejects a malformed call when the node is built."""
    t = gpu_session.table([("k", T_INT, [1, 2], None), ("s", T_STRING, ["a", "b"], None)])
    for fn, args in ((0, ["k", "", ""]), (3, ["k", "s", ""]), (3, ["k", "", ""]), (2, ["k", "k"]), (9, ["k"])):
        with pytest.raises((_lib.IllegalArgumentException, _lib.NotImplementedException)):
            t._new("capf_table_list_fn", t._h, fn, len(args), _lib.strs(args), b"z")
