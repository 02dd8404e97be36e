"""Lambda expressions over lists on the device: [x IN xs WHERE p | e], filter,
any / all / none / single and reduce (capf_table_list_lambda, CAPF_OP_LAMBDA).

The CPU oracle does not know these expressions, so the expectations come from
the small Python model below — the table in expr.py's docstrings (the Morpheus
lowering, SparkSQLExprMapper.scala:340-395, on Spark 2.4) written with Python
lists — and from the 11 reference cases transcribed in
tests/golden/list_lambda_cases.py.  Lists are compared with == on typed values:
order and 5 vs 5.0 matter (floats by repr, so NaN equals NaN and -0.0 is not 0.0).
"""
import random

import numpy as np
import pytest

from conftest import case_parts
from list_lambda_cases import CASES, NESTED

from capf_amd import _lib
from capf_amd.expr import (LAMBDA_EXPRS, OP_ADD, OP_COL, OP_GT, OP_LAMBDA, OP_LIT_INT, T_BOOL, T_FLOAT, T_INT,
                           T_LIST, T_NULL, T_STRING, Add, Ands, BoolLit, CaseExpr, Collect, ContainerIndex, CountStar,
                           ElementProperty, Equals, Explode, FloatLit, GreaterThan, Head, In, IntegerLit, IsNull,
                           LambdaVar, LessThan, ListAll, ListAny, ListComprehension, ListFilter, ListLit, ListNone,
                           ListReduction, ListSingle, ListSliceFrom, Modulo, Multiply, Not, NullLit, Ors, Rand_,
                           Range, Reverse, Size, StringLit, Subtract, ToInteger, ToUpper, Var, compile_program,
                           lambda_parts, reduce_type, static_type_in_lambda)
from capf_amd.header import RecordHeader

COLS = ["k", "g", "xs", "ys", "z", "x", "s", "f"]
H = RecordHeader({Var(c): c for c in COLS})
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
x, a = LambdaVar("x"), LambdaVar("a")
XS, K, G = Var("xs"), Var("k"), Var("g")


def I(v):  # noqa: E743
    return IntegerLit(v)


def typed(v):
    """A value with its type spelled out, lists in order: typed(5.0) != typed(5)."""
    if isinstance(v, (list, tuple)):
        return ("list", tuple(typed(e) for e in v))
    return (type(v).__name__, repr(v) if isinstance(v, float) else v)


def same(got, want):
    return typed(got) == typed(want)


# ------------------------------------------------------------------ the model
def wrap(v):
    return (v + 2 ** 63) % 2 ** 64 - 2 ** 63


def m_and(vals):
    return False if any(v is False for v in vals) else None if any(v is None for v in vals) else True


def m_or(vals):
    return True if any(v is True for v in vals) else None if any(v is None for v in vals) else False


def m_in(v, xs):
    if xs is None:
        return None
    if not xs:
        return False
    if v is None:
        return None
    if any(e is not None and e == v for e in xs):
        return True
    return None if any(e is None for e in xs) else False


def m_arith(op, p, q):
    if p is None or q is None:
        return None
    if isinstance(p, float) or isinstance(q, float):
        p, q = float(p), float(q)
        return {"Add": p + q, "Subtract": p - q, "Multiply": p * q}[op]
    if op in ("Divide", "Modulo"):
        if q == 0:
            return None
        t = abs(p) // abs(q) * (1 if (p < 0) == (q < 0) else -1)  # truncated, as Java
        return wrap(t) if op == "Divide" else p - t * q
    return wrap({"Add": p + q, "Subtract": p - q, "Multiply": p * q}[op])


def m_comprehension(xs, env, var, pred, body):
    if xs is None:
        return None
    kept = [e for e in xs if pred is None or m_eval(pred, {**env, var: e}) is True]
    return [e if body is None else m_eval(body, {**env, var: e}) for e in kept]


def m_quantifier(kind, xs, env, var, pred):
    if xs is None:
        return None
    t = sum(1 for e in xs if m_eval(pred, {**env, var: e}) is True)
    return {"ListAny": t > 0, "ListNone": t == 0, "ListAll": t == len(xs), "ListSingle": t == 1}[kind]


def m_reduce(xs, env, acc, var, body, init, widen=False):
    if xs is None:
        return None
    v = float(init) if widen and init is not None else init
    for e in xs:
        v = m_eval(body, {**env, acc: v, var: e})
    return float(v) if widen and v is not None else v


def m_eval(e, env):
    """The model over an expression tree: the interpreter's rules for the
    classes the tests use, lambda expressions by the table above."""
    cls = type(e).__name__
    if cls in ("IntegerLit", "StringLit", "FloatLit", "BoolLit"):
        return e.v
    if cls == "NullLit":
        return None
    if cls in ("Var", "LambdaVar"):
        return env[e.vname]
    if cls == "ElementProperty":
        return env[e.key]
    if cls == "ListLit":
        return [m_eval(i, env) for i in e.items]
    if cls in ("Add", "Subtract", "Multiply", "Divide", "Modulo"):
        return m_arith(cls, m_eval(e.lhs, env), m_eval(e.rhs, env))
    if cls in ("Equals", "LessThan", "LessThanOrEqual", "GreaterThan", "GreaterThanOrEqual"):
        p, q = m_eval(e.lhs, env), m_eval(e.rhs, env)
        if p is None or q is None:
            return None
        return {"Equals": p == q, "LessThan": p < q, "LessThanOrEqual": p <= q, "GreaterThan": p > q,
                "GreaterThanOrEqual": p >= q}[cls]
    if cls == "Not":
        v = m_eval(e.expr, env)
        return None if v is None else not v
    if cls == "Ands":
        return m_and([m_eval(i, env) for i in e.exprs])
    if cls == "Ors":
        return m_or([m_eval(i, env) for i in e.exprs])
    if cls == "IsNull":
        return m_eval(e.expr, env) is None
    if cls == "CaseExpr":
        for p, v in e.alternatives:
            if m_eval(p, env) is True:
                return m_eval(v, env)
        return None if e.default is None else m_eval(e.default, env)
    if cls == "In":
        return m_in(m_eval(e.lhs, env), m_eval(e.rhs, env))
    if cls == "Size":
        v = m_eval(e.expr, env)
        return None if v is None else len(v)
    if cls == "ToInteger":
        v = m_eval(e.expr, env)
        return None if v is None else int(v)
    if cls == "ToUpper":
        v = m_eval(e.expr, env)
        return None if v is None else v.upper()
    if cls == "Reverse":
        v = m_eval(e.expr, env)
        return None if v is None else v[::-1]
    if cls == "Head":
        v = m_eval(e.expr, env)
        return v[0] if v else None
    if cls == "ContainerIndex":
        v, i = m_eval(e.container, env), m_eval(e.index, env)
        return None if v is None or i is None or not -len(v) <= i < len(v) else v[i]
    if cls == "ListSliceFrom":
        v, lo = m_eval(e.list, env), m_eval(e.frm, env)
        return None if not v or lo is None else v[lo:]  # an EMPTY list gives NULL too
    if cls == "Range":
        lo, hi = m_eval(e.frm, env), m_eval(e.to, env)
        return None if lo is None or hi is None else list(range(lo, hi + 1))
    if isinstance(e, LAMBDA_EXPRS):
        _, lst, pred, body, init, vs = lambda_parts(e)
        xs = m_eval(lst, env)
        if cls == "ListReduction":
            return m_reduce(xs, env, vs[0].vname, vs[1].vname, body, m_eval(init, env))
        if cls in ("ListComprehension", "ListFilter"):
            return m_comprehension(xs, env, vs[0].vname, pred, body)
        return m_quantifier(cls, xs, env, vs[0].vname, pred)
    raise NotImplementedError(cls)


def m_query(q):
    rows = [{}]
    for st in q.stages:
        rows = [{al: m_eval(e, r) for al, e in st.items} for r in rows]
    return rows


def rows_key(rows):
    return sorted(repr(sorted((k, typed(v)) for k, v in r.items())) for r in rows)


def seven(pred, val, lst=XS, init=None):
    """The seven forms over one predicate and one extract / fold expression."""
    init = I(0) if init is None else init
    return [("comprehension", ListComprehension(x, pred, val, lst)), ("filter", ListFilter(x, pred, lst)),
            ("any", ListAny(x, pred, lst)), ("all", ListAll(x, pred, lst)), ("none", ListNone(x, pred, lst)),
            ("single", ListSingle(x, pred, lst)),
            ("reduce", ListReduction(a, x, CaseExpr([(pred, Add(a, val))], a), init, lst))]


# ------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_model_agrees_with_reference_case(case):
    cid, src, create, query, expected, opts = case_parts(case)
    assert rows_key(m_query(query)) == rows_key(expected), (cid, src)


def test_model_pins():
    env = {}
    gt0 = GreaterThan(x, I(0))
    assert m_eval(ListAll(x, gt0, ListLit(I(1), NullLit(), I(2))), env) is False
    assert m_eval(ListAny(x, gt0, ListLit(NullLit(), I(0))), env) is False
    assert m_eval(ListNone(x, gt0, ListLit()), env) is True and m_eval(ListAll(x, gt0, ListLit()), env) is True
    assert m_eval(ListSingle(x, gt0, ListLit(I(1), I(2))), env) is False
    assert m_eval(ListAny(x, gt0, NullLit()), env) is None and m_eval(ListAll(x, gt0, NullLit()), env) is None
    assert m_eval(ListReduction(a, x, Add(a, x), I(INT64_MAX), ListLit(I(1))), env) == INT64_MIN
    assert m_eval(ListComprehension(x, None, None, ListLit(I(1), NullLit())), env) == [1, None]
    assert m_arith("Divide", -7, 2) == -3 and m_arith("Modulo", -7, 2) == -1 and m_arith("Modulo", 7, 0) is None


def test_nested_comprehension_is_not_implemented():
    """ExpressionTests.scala:1562-1572 wants [[1], [], []]: nested lists and a
    lambda expression inside a lambda body, both NotImplemented.  (Raised when
    the expression is hoisted, before any device work.)"""
    from capf_amd.expr import check_lambda_body
    cid, src, create, query, expected, opts = case_parts(NESTED)
    outer = query.stages[1].items[0][1]
    with pytest.raises(_lib.NotImplementedException, match="lambda expression inside a lambda body"):
        check_lambda_body(outer.extractExpression, outer)


TYPES = {"xs": T_LIST, ("elem", "xs"): T_INT, "ys": T_LIST, ("elem", "ys"): T_INT, "k": T_INT, "x": T_INT,
         "s": T_STRING, "f": T_FLOAT}


def _compile(e, lambdas=None, types=None):
    types = types or TYPES
    codes = {}
    return compile_program(e, H, {c for c in types if isinstance(c, str)}, {},
                           lambda v: codes.setdefault(v, 100 + len(codes)), lambda c: types[c], lambdas=lambdas)


def test_body_compiles_to_lambda_slots():
    ops, ia, fa, names = _compile(GreaterThan(x, K), {"x": (0, T_INT)})
    assert list(ops) == [OP_LAMBDA, OP_COL, OP_GT] and ia[0] == 0 and names[ia[1]] == "k"
    # reduce: slot 0 the accumulator, slot 1 the element
    ops, ia, _, _ = _compile(Add(a, x), {"a": (0, T_INT), "x": (1, T_INT)})
    assert (list(ops), list(ia)) == ([OP_LAMBDA, OP_LAMBDA, OP_ADD], [0, 1, 0])
    # the lambda variable shadows column x, as a LambdaVar and as a plain Var of its name
    for v in (x, Var("x")):
        ops, ia, _, names = _compile(Add(v, I(1)), {"x": (0, T_INT)})
        assert list(ops) == [OP_LAMBDA, OP_LIT_INT, OP_ADD] and "x" not in names
    assert list(_compile(Add(Var("x"), I(1)))[0]) == [OP_COL, OP_LIT_INT, OP_ADD]  # no binder: the column
    # row columns, another LIST column of the row
    ops, _, _, names = _compile(Ands(In(x, Var("ys")), GreaterThan(Size(Var("ys")), ContainerIndex(Var("ys"), x))),
                                {"x": (0, T_INT)})
    assert OP_LAMBDA in ops and list(names) == ["ys"]
    # the static type follows the slot's type
    assert static_type_in_lambda(Multiply(x, I(3)), H, set(COLS), {}, TYPES.get, {"x": (0, T_INT)}) == T_INT
    assert static_type_in_lambda(Multiply(x, I(3)), H, set(COLS), {}, TYPES.get, {"x": (0, T_FLOAT)}) == T_FLOAT
    assert static_type_in_lambda(ToUpper(x), H, set(COLS), {}, TYPES.get, {"x": (0, T_STRING)}) == T_STRING


def test_free_lambda_var_is_illegal():
    with pytest.raises(_lib.IllegalArgumentException):
        _compile(Add(x, I(1)))
    with pytest.raises(_lib.IllegalArgumentException):
        _compile(Add(a, x), {"x": (0, T_INT)})


def test_lambda_expressions_are_table_operations():
    for _, e in seven(GreaterThan(x, I(0)), x):
        with pytest.raises(_lib.NotImplementedException):
            _compile(e)  # orderBy / group arguments are lowered so: they stay NotImplemented


def test_disallowed_bodies():
    from capf_amd.expr import check_lambda_body
    bad = [Size(Reverse(XS)), In(x, Range(I(1), x)), Head(ListSliceFrom(XS, I(1))), In(x, ListLit(K, I(3))),
           ListAny(x, GreaterThan(x, I(0)), XS), Add(x, CountStar()), GreaterThan(Rand_(), FloatLit(0.5)),
           ListLit(x, I(1)), Add(x, Size(ListComprehension(x, None, None, XS)))]
    for b in bad:
        with pytest.raises(_lib.NotImplementedException) as err:
            check_lambda_body(b, ListComprehension(x, None, b, XS))
        assert "lambda body" in str(err.value), b
    for ok in (Add(x, K), In(x, Var("ys")), In(x, ListLit(I(1), NullLit())), Size(Var("ys"))):
        check_lambda_body(ok, ListAny(x, ok, XS))


def test_reduce_type_rules():
    def typer(body):
        return lambda at: static_type_in_lambda(body, H, set(COLS), {}, TYPES.get, {"a": (0, at), "x": (1, T_INT)})
    assert reduce_type(T_INT, typer(Add(a, x))) == T_INT
    assert reduce_type(T_FLOAT, typer(Add(a, x))) == T_FLOAT
    assert reduce_type(T_INT, typer(Add(a, Multiply(x, FloatLit(0.5))))) == T_FLOAT  # INTEGER init widened
    assert reduce_type(T_NULL, typer(Add(a, x))) == T_INT  # a NULL-typed init takes the body's type
    assert reduce_type(T_NULL, typer(Multiply(x, FloatLit(2.0)))) == T_FLOAT
    assert reduce_type(T_BOOL, typer(Ors(a, GreaterThan(x, I(1))))) == T_BOOL
    for it, body in ((T_FLOAT, GreaterThan(x, I(1))), (T_BOOL, Add(x, I(1))), (T_STRING, Add(x, I(1))),
                     (T_INT, GreaterThan(x, a))):
        with pytest.raises(_lib.IllegalArgumentException):
            reduce_type(it, typer(body))


def test_str_is_okapi_without_type():
    n = LambdaVar("n")
    t = Var("things")
    assert str(ListComprehension(n, GreaterThan(n, I(2)), Multiply(n, I(3)), t)) == \
        "[n IN things WHERE (n > 2) | (n * 3)]"
    assert str(ListComprehension(n, None, None, t)) == "[n IN things]"
    assert str(ListFilter(n, GreaterThan(n, I(2)), t)) == "filter(n IN things WHERE (n > 2))"
    assert str(ListAny(n, GreaterThan(n, I(2)), t)) == "any((n IN things WHERE (n > 2)))"
    assert str(ListReduction(a, n, Add(a, n), I(0), t)) == "reduce(a = 0, n IN things | (a + n))"
    assert ListAny(n, BoolLit(True), t) != ListAll(n, BoolLit(True), t) and LambdaVar("n") != Var("n")


def test_scala_twin_names_the_classes_and_the_entry_point():
    import okapi_scala_scan as sc
    srcs = sc.integration_sources()
    mapper, table, native = (sc.strip_comments(srcs[f]) for f in
                             ("GpuExprMapper.scala", "GpuTable.scala", "Native.scala"))
    assert "OpLambda = 98" in native and "Native.OpLambda" in mapper
    for k, name in enumerate(("LambdaComprehension", "LambdaAny", "LambdaAll", "LambdaNone", "LambdaSingle",
                              "LambdaReduce")):
        assert f"{name} = {k}" in native and f"Native.{name}" in table
    assert "LambdaVar" in mapper
    for cls in ("ListComprehension", "ListReduction", "ListFilter", "ListAny", "ListAll", "ListNone", "ListSingle"):
        assert f": {cls}" in table, cls
    assert "Native.tableListLambda(" in table and "def tableListLambda(" in native
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "integration", "jni", "capf_jni.cpp")) as f:
        assert "capf_table_list_lambda(" in f.read()


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


@pytest.mark.gpu
def test_nested_reference_case_raises_on_gpu(gpu_session):
    from capf_amd.graph import ScanGraph
    from capf_amd.planner import run
    from oracle.create_parser import parse_create
    cid, src, create, query, expected, opts = case_parts(NESTED)
    with pytest.raises(_lib.NotImplementedException):
        run(ScanGraph.from_data(gpu_session, parse_create(create)), query, None)


# ------------------------------------------------------ GPU: fixed edge table
def values(t, e, h=H):
    out = t.withColumns((e, "z"), header=h, params={})
    assert [c for c in out.physicalColumns if c.startswith("\x03")] == [], out.physicalColumns
    return out.column_values("z")


def check(t, rows, e, h=H):
    got = values(t, e, h)
    want = [m_eval(e, r) for r in rows]
    assert same(got, want), f"{e}: got {got}, want {want}"


NAN = float("nan")
EDGE = {  # a NULL list, [], one element, NULL elements, all NULL, the type's edge values
    T_INT: [None, [], [2], [1, None, 2], [None, 0], [None, None], [INT64_MIN, INT64_MAX, 1], [3, 4], [0, 5, 7, -1]],
    T_FLOAT: [None, [], [1.5], [0.5, None, 2.0], [None, -1.0], [None, None], [NAN, 0.0, -0.0], [NAN], [2.5, -0.0, 3.0]],
    T_BOOL: [None, [], [True], [True, None, False], [None, False], [None, None], [True, True], [False], [False, True]],
    T_STRING: [None, [], ["a"], ["a", None, "bb"], [None, ""], [None, None], ["bb", "a", "a"], ["c"], ["", "bb"]],
}
EDGE_K = [0, 1, None, 1, 0, 2, 1, 3, None]
# (predicates, an extract, a reduce body over (a, x), its init) per element type; the predicates
# are TRUE, FALSE and NULL on different elements
EDGE_BODIES = {
    T_INT: ([GreaterThan(x, I(0)), IsNull(x), GreaterThan(x, K), Equals(Modulo(x, I(2)), I(0)), BoolLit(True),
             NullLit("BOOLEAN")], Add(x, I(1)), Add(a, x), I(0)),
    T_FLOAT: ([GreaterThan(x, FloatLit(0.0)), Equals(x, x), IsNull(x), LessThan(x, K)], Multiply(x, FloatLit(2.0)),
              Add(a, x), FloatLit(0.0)),
    T_BOOL: ([x, Not(x), IsNull(x), Ors(x, Equals(K, I(1)))], Not(x), Ors(a, x), BoolLit(False)),
    T_STRING: ([Equals(x, StringLit("a")), IsNull(x), GreaterThan(Size(x), K)], Size(x), Add(a, Size(x)), I(0)),
}


def edge_table(sess, et):
    xs = EDGE[et]
    n = len(xs)
    t = sess.table([("k", T_INT, EDGE_K, None), ("xs", T_LIST, xs, None)], nrows=n)
    return t, [dict(k=k, xs=v) for k, v in zip(EDGE_K, xs)]


@pytest.mark.gpu
@pytest.mark.parametrize("et", [T_INT, T_FLOAT, T_BOOL, T_STRING], ids=["int", "float", "bool", "string"])
def test_seven_forms_over_the_edge_table(gpu_session, et):
    t, rows = edge_table(gpu_session, et)
    preds, val, fold, init = EDGE_BODIES[et]
    check(t, rows, ListComprehension(x, None, val, XS))
    check(t, rows, ListComprehension(x, None, None, XS))
    check(t, rows, ListReduction(a, x, fold, init, XS))
    for p in preds:
        check(t, rows, ListComprehension(x, p, val, XS))
        check(t, rows, ListComprehension(x, p, None, XS))
        check(t, rows, ListFilter(x, p, XS))
        for q in (ListAny, ListAll, ListNone, ListSingle):
            check(t, rows, q(x, p, XS))
        check(t, rows, ListReduction(a, x, CaseExpr([(p, fold)], a), init, XS))
    out = t.withColumns((ListComprehension(x, preds[0], val, XS), "z"), header=H, params={})
    assert out.list_elem_type("z") == (T_BOOL if et == T_BOOL else T_INT if et in (T_INT, T_STRING) else T_FLOAT)


@pytest.mark.gpu
def test_pinned_quantifier_results(gpu_session):
    xs = [[1, None, 2], [None, 0], [], [1, 2], None, [None], [5]]
    t = gpu_session.table([("xs", T_LIST, xs, None)], nrows=len(xs))
    p = GreaterThan(x, I(0))
    assert same(values(t, ListAll(x, p, XS)), [False, False, True, True, None, False, True])  # a NULL result: FALSE
    assert same(values(t, ListAny(x, p, XS)), [True, False, False, True, None, False, True])  # only NULLs: FALSE
    assert same(values(t, ListNone(x, p, XS)), [False, True, True, False, None, True, False])  # none([]) is TRUE
    assert same(values(t, ListSingle(x, p, XS)), [False, False, False, False, None, False, True])  # two hits: FALSE
    # elements whose validity is not needed carry none
    z = t.withColumns((ListComprehension(x, IsNull(x), I(7), XS), "z"), header=H, params={})
    assert z.list_arrays("z")[4] is None and same(z.column_values("z"), [[7], [7], [], [], None, [7], []])


@pytest.mark.gpu
def test_null_typed_lists_and_elements(gpu_session):
    xs = [None, [], [None], [None, None, None]]
    t = gpu_session.table([("k", T_INT, [1, 2, 3, 4], None), ("xs", T_LIST, xs, None)], nrows=4)
    rows = [dict(k=k, xs=v) for k, v in zip([1, 2, 3, 4], xs)]
    assert t.list_elem_type("xs") == T_NULL
    for _, e in seven(IsNull(x), K):
        check(t, rows, e)
    check(t, rows, ListComprehension(x, None, x, XS))
    check(t, rows, ListComprehension(x, None, Add(K, I(1)), XS))
    # a NULL-typed list: a NULL-typed column
    for _, e in seven(IsNull(x), K, lst=NullLit()):
        out = t.withColumns((e, "z"), header=H, params={})
        assert out.capf_type("z") == T_NULL and out.column_values("z") == [None] * 4


# ------------------------------------------------ GPU: bodies that read the row
@pytest.mark.gpu
def test_bodies_that_read_the_row(gpu_session):
    """(A session of its own: a string function over the element goes through a
    code map, which exists only while the session's dictionary is small — the
    suite's shared session outgrows it.)"""
    from capf_amd.table import GpuSession
    sess = GpuSession(0)
    xs = [[1, 5, 9], [2, None, 4], None, [], [7], [3, 3]]
    ys = [[5], [None, 4], [1], [2], None, []]
    ks = [4, 2, 1, None, 7, 0]
    ss = [["ab", "c"], [None, "Dd"], [], None, ["12", "x7", "-3"], [""]]
    n = len(xs)
    t = sess.table([("k", T_INT, ks, None), ("xs", T_LIST, xs, None), ("ys", T_LIST, ys, None),
                    ("s", T_LIST, ss, None)], nrows=n)
    nk = ElementProperty(Var("n", "NODE"), "k", "INTEGER")
    h = RecordHeader({XS: "xs", Var("ys"): "ys", Var("s"): "s", nk: "k", K: "k"})
    rows = [dict(k=k, xs=p, ys=q, s=r) for k, p, q, r in zip(ks, xs, ys, ss)]
    check(t, rows, ListComprehension(x, GreaterThan(x, nk), Add(x, nk), XS), h)
    check(t, rows, ListAny(x, In(x, Var("ys")), XS), h)
    check(t, rows, ListComprehension(x, None, Add(Size(Var("ys")), ContainerIndex(Var("ys"), I(0))), XS), h)
    # STRING elements through a code map and through the string → number table
    check(t, rows, ListComprehension(x, None, ToUpper(x), Var("s")), h)
    check(t, rows, ListComprehension(x, Equals(ToUpper(x), StringLit("DD")), ToUpper(x), Var("s")), h)
    # once the dictionary has outgrown a code map the function would need a value map over the
    # lambda variable: NotImplemented (forced here by hiding the code maps)
    sess.string_map = lambda key: None
    try:
        with pytest.raises(_lib.NotImplementedException, match="value map over the lambda variable"):
            values(t, ListComprehension(x, None, ToUpper(x), Var("s")), h)
    finally:
        del sess.string_map
    got = values(t, ListComprehension(x, None, ToInteger(x), Var("s")), h)
    assert same(got, [[None, None], [None, None], [], None, [12, None, -3], [None]])
    # an extract whose static type is NULL
    out = t.withColumns((ListComprehension(x, GreaterThan(x, I(2)), NullLit(), XS), "z"), header=h, params={})
    assert out.list_elem_type("z") == T_NULL
    assert same(out.column_values("z"), [[None, None], [None], None, [], [None], [None, None]])
    # the lambda variable shadows a column of its name
    kk = LambdaVar("k")
    assert same(values(t, ListComprehension(kk, None, Add(kk, K), XS), h),
                [None if p is None else [None if v is None else 2 * v for v in p] for p in xs])


# ------------------------------------------- GPU: composition through hoisting
@pytest.mark.gpu
def test_composition(gpu_session):
    xs = [[1, 5, 9], [2, None, 4], None, [], [7], [3, 3], [0, 2]]
    ks = [4, 2, 1, None, 7, 0, 3]
    n = len(xs)
    t = gpu_session.table([("k", T_INT, ks, None), ("xs", T_LIST, xs, None)], nrows=n)
    rows = [dict(k=k, xs=v) for k, v in zip(ks, xs)]
    p = GreaterThan(x, I(2))
    check(t, rows, Size(ListComprehension(x, p, None, XS)))
    check(t, rows, ListComprehension(x, None, Multiply(x, x), Range(I(1), K)))
    check(t, rows, Head(ListComprehension(x, p, None, Reverse(XS))))
    check(t, rows, ListComprehension(x, None, Add(x, I(1)), ListLit(I(1), I(2), I(3))))
    check(t, rows, Add(ListReduction(a, x, Add(a, x), K, XS), Size(ListFilter(x, p, XS))))
    check(t, rows, ListAny(x, Equals(x, I(10)), ListComprehension(x, None, Add(x, I(1)), XS)))
    # WHERE any(x IN xs[1..] WHERE p) inside filter
    cond = ListAny(x, p, ListSliceFrom(XS, I(1)))
    f = t.filter(cond, header=H, params={})
    assert f.physicalColumns == t.physicalColumns
    assert f.column_values("k") == [r["k"] for r in rows if m_eval(cond, r) is True]
    # UNWIND [x IN xs | e]
    e = ListComprehension(x, None, Add(x, K), XS)
    u = t.withColumns((Explode(e), "e"), header=H, params={})
    assert u.physicalColumns == ["k", "xs", "e"]
    assert same([(r["k"], r["e"]) for r in u.rows], [(r["k"], v) for r in rows for v in (m_eval(e, r) or [])])
    # reduce with an INTEGER init and a FLOAT body: a FLOAT, the init widened
    body = Add(a, Multiply(x, FloatLit(0.5)))
    out = t.withColumns((ListReduction(a, x, body, I(1), XS), "z"), header=H, params={})
    assert out.capf_type("z") == T_FLOAT
    assert same(out.column_values("z"), [m_reduce(r["xs"], r, "a", "x", body, 1, widen=True) for r in rows])
    assert out.column_values("z")[3] == 1.0 and isinstance(out.column_values("z")[3], float)
    # two lambda items and a scalar one in one call; nothing temporary survives
    out = t.withColumns((ListFilter(x, p, XS), "f"), (Add(K, I(1)), "k1"), (ListAll(x, p, XS), "q"), header=H, params={})
    assert out.physicalColumns == ["k", "xs", "f", "k1", "q"]
    # orderBy arguments are not hoisted: they keep raising
    with pytest.raises(_lib.NotImplementedException):
        t.orderBy((ListAny(x, p, XS), "asc"), header=H, params={}).size
    with pytest.raises(_lib.IllegalArgumentException):
        values(t, ListReduction(a, x, GreaterThan(x, a), I(0), XS))
    with pytest.raises(_lib.NotImplementedException):
        values(t, ListAny(x, In(x, Reverse(XS)), XS))


@pytest.mark.gpu
def test_collected_ids_as_elements(gpu_session):
    """Lists built by collect over a FOR-encoded id column.  This path cannot
    hand the lambda kernels an encoded child: lists.hip::collect_lists passes
    the gathered, sorted values through decode_column before they become the
    element column, so the child is plain int64 (gather_list gathers an
    existing child, and the host constructors upload plain arrays: no operation
    encodes an element column).  The kernels read elements through load_col /
    ld_int all the same; the values over the collected ids are checked."""
    ids = np.arange(1000, 1400, dtype=np.int64)
    t = gpu_session.table([("k", T_INT, ids % 7, None), ("x", T_INT, ids, None)], nrows=len(ids)).compact(4)
    g = t.group([K], {"xs": Collect(Var("x"))}, header=H, params={})
    rows = [dict(k=k, xs=sorted(int(v) for v in ids[ids % 7 == k])) for k in g.column_values("k")]
    p = Equals(Modulo(x, I(3)), I(0))
    check(g, rows, ListComprehension(x, p, Subtract(x, K), XS))
    check(g, rows, ListReduction(a, x, Add(a, x), I(0), XS))
    check(g, rows, ListSingle(x, Equals(x, I(1001)), XS))


# ----------------------------------- GPU: shapes where the kernels can go wrong
def _list_table(sess, lists, valid=None):
    n = len(lists)
    t = sess.table([("k", T_INT, np.arange(n, dtype=np.int64), None)], nrows=n)
    return t.add_list("xs", lists, valid)


EVEN = Equals(Modulo(x, I(2)), I(0))


def _check_shapes(t, lists, pred=EVEN, keep=lambda v: v % 2 == 0):
    rows = [dict(k=r, xs=v) for r, v in enumerate(lists)]
    items = [(ListComprehension(x, pred, Add(x, K), XS), "c"), (ListFilter(x, pred, XS), "f"),
             (ListComprehension(x, None, Multiply(x, I(3)), XS), "m"), (ListAny(x, pred, XS), "any"),
             (ListAll(x, pred, XS), "all"), (ListNone(x, pred, XS), "none"), (ListSingle(x, pred, XS), "single"),
             (ListReduction(a, x, Add(a, x), I(0), XS), "r")]
    out = t.withColumns(*items, header=H, params={})
    assert out.size == len(lists)
    for e, c in items:
        got = out.column_values(c)
        assert same(got, [m_eval(e, r) for r in rows]), c
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_row_counts_around_a_block(gpu_session, n):
    lists = [list(range(r, r + r % 4)) for r in range(n)]
    _check_shapes(_list_table(gpu_session, lists), lists)


@pytest.mark.gpu
def test_long_list_between_runs_of_empty_rows(gpu_session):
    """600 elements between 70 and 130 empty rows: the tile windows cross the
    long list and step over more than 64 empty offsets."""
    lists = [[] for _ in range(70)] + [list(range(600))] + [[] for _ in range(130)] + [[1, 2, 3]]
    out = _check_shapes(_list_table(gpu_session, lists), lists)
    # without WHERE the offsets and the list validity are the source's own
    assert np.array_equal(out.list_arrays("m")[1], out.list_arrays("xs")[1])


@pytest.mark.gpu
def test_kept_totals(gpu_session):
    lists = [[1, 3], [5], [], [7, 9, 11]] * 80 + [[13] * 300]  # 780 elements, four tiles
    t = _list_table(gpu_session, lists)
    _check_shapes(t, lists)                                          # keeps nothing: the kept total is 0
    _check_shapes(t, lists, GreaterThan(x, I(0)))                    # keeps everything
    last = lists[:-1] + [[13] * 298 + [2, 4]]                        # kept elements only in the last tile
    _check_shapes(_list_table(gpu_session, last), last)
    _check_shapes(_list_table(gpu_session, [[], [], []]), [[], [], []])  # no element at all
    _check_shapes(_list_table(gpu_session, [None, None]), [None, None])  # all-NULL lists


@pytest.mark.gpu
def test_null_lists_that_own_stored_elements(gpu_session):
    """NULL lists that own stored elements.  No table operation CREATES such a
    column: lists.hip::gather_list gives an index of -1 the length 0, and
    kernels_basic.hip::concat_lists (unionAll) copies offsets and elements as
    they are; only the host constructor capf_table_add_list, which takes the
    validity as given, does.  Both operations carry stored elements ALONG,
    though (gather_list copies off[j + 1] - off[j] elements of a NULL source
    row j), so the column is built from the host and then also pushed through
    a filter (a gather) and a unionAll: the elements under NULL rows get flag
    0 and never reach a result."""
    stored = [[2, 4], [6, 1], [8], [], [3, 10, 12]]
    valid = [1, 0, 0, 1, 1]
    lists = [v if ok else None for v, ok in zip(stored, valid)]
    t = _list_table(gpu_session, stored, valid)
    assert same(t.column_values("xs"), lists)
    out = _check_shapes(t, lists)
    assert out.list_arrays("f")[2].tolist() == [2, 4, 10, 12]
    g = t.filter(GreaterThan(K, I(0)), header=H, params={})  # rows 1..4, gathered
    assert g.list_arrays("xs")[1].tolist() == [0, 2, 3, 3, 6]  # the NULL rows kept their elements
    rows = [dict(k=r, xs=lists[r]) for r in range(1, 5)]
    u = t.unionAll(g)
    urows = [dict(k=r, xs=v) for r, v in enumerate(lists)] + rows
    for tab, rr in ((g, rows), (u, urows)):
        for e in (ListFilter(x, EVEN, XS), ListComprehension(x, None, Add(x, K), XS), ListAll(x, EVEN, XS),
                  ListReduction(a, x, Add(a, x), I(0), XS)):
            check(tab, rr, e)


@pytest.mark.gpu
def test_lazy_row_columns_keep_their_nulls(gpu_session):
    """A body that reads a row column still held as a lazy gather — the output
    of a filter, the null-extended side of an optional join — with NULLs in
    it: the extract gives NULL elements there, not 0 (the element validity is
    decided after the column is forced), and so does the fold."""
    xs = [[1, 2], [3], [], [4, 5, 6], None, [7]]
    ks = [10, None, 3, None, 5, 20]
    n = len(xs)
    t = gpu_session.table([("id", T_INT, list(range(n)), None), ("k", T_INT, ks, None), ("xs", T_LIST, xs, None)],
                          nrows=n)
    h = RecordHeader({Var(c): c for c in ("id", "k", "xs", "rid")})
    exprs = [ListComprehension(x, None, Add(x, K), XS), ListComprehension(x, None, GreaterThan(x, K), XS),
             ListReduction(a, x, Add(Add(a, x), K), I(0), XS), ListComprehension(x, GreaterThan(x, I(1)), Add(x, K), XS)]
    f = t.filter(GreaterThan(Var("id"), I(-1)), header=h, params={})
    rows = [dict(id=i, k=k, xs=v) for i, (k, v) in enumerate(zip(ks, xs))]
    for e in exprs:
        check(f, rows, e, h)
    # optional join: k comes from the right side, absent for ids 1, 3 and 5
    left = gpu_session.table([("id", T_INT, list(range(n)), None), ("xs", T_LIST, xs, None)], nrows=n)
    right = gpu_session.table([("rid", T_INT, [0, 2, 4], None), ("k", T_INT, [10, 3, 5], None)], nrows=3)
    j = left.join(right, "left_outer", ("id", "rid"))
    jk = {0: 10, 2: 3, 4: 5}
    ids = j.column_values("id")
    assert sorted(ids) == list(range(n))
    for e in exprs:
        vals = values(j, e, h)
        want = [m_eval(e, dict(id=i, k=jk.get(i), xs=xs[i])) for i in ids]
        assert same(vals, want), f"{e}: got {vals}, want {want}"


@pytest.mark.gpu
def test_rows_past_the_grid_cap(gpu_session):
    """256·16·256 + 1 single-element rows: the grid-stride loops of the
    per-element and per-row kernels take a second step.  Against numpy."""
    n = 256 * 16 * 256 + 1
    v = (np.arange(n, dtype=np.int64) * 7919) % 1000
    t = gpu_session.table([("k", T_INT, v, None)], nrows=n).withColumns((ListLit(K), "xs"), header=H, params={})
    p = LessThan(x, I(500))
    out = t.withColumns((ListFilter(x, p, XS), "f"), (ListAll(x, p, XS), "q"), header=H, params={})
    et, offs, vals, valid, ev = out.list_arrays("f")
    keep = v < 500
    assert et == T_INT and np.array_equal(offs, np.concatenate([[0], np.cumsum(keep)]))
    assert np.array_equal(vals, v[keep]) and valid.all()
    q = np.asarray(out.column_values("q"), dtype=bool)
    assert np.array_equal(q, keep)


# ----------------------------------------------------- GPU: seeded random trees
def _int_expr(rnd, depth):
    if depth == 0 or rnd.random() < 0.3:
        return rnd.choice([x, x, K, G, I(rnd.randint(-3, 6)), I(rnd.randint(-3, 6))])
    c = rnd.random()
    if c < 0.6:
        return rnd.choice([Add, Subtract, Multiply, Modulo])(_int_expr(rnd, depth - 1), _int_expr(rnd, depth - 1))
    return CaseExpr([(_bool_expr(rnd, depth - 1), _int_expr(rnd, depth - 1))],
                    _int_expr(rnd, depth - 1) if rnd.random() < 0.7 else None)


def _bool_expr(rnd, depth):
    c = rnd.random()
    if depth == 0 or c < 0.4:
        cmp = rnd.choice([Equals, LessThan, GreaterThan])
        return cmp(_int_expr(rnd, max(depth - 1, 0)), _int_expr(rnd, max(depth - 1, 0)))
    if c < 0.5:
        return IsNull(_int_expr(rnd, depth - 1))
    if c < 0.6:
        return In(_int_expr(rnd, depth - 1), ListLit(*[rnd.choice([I(rnd.randint(0, 6)), NullLit()]) for _ in range(3)]))
    if c < 0.7:
        return Not(_bool_expr(rnd, depth - 1))
    return rnd.choice([Ands, Ors])(_bool_expr(rnd, depth - 1), _bool_expr(rnd, depth - 1))


def _random_cases(group):
    """16 (predicate, value) bodies; one the model cannot evaluate is redrawn."""
    rnd = random.Random(1000 + group)
    probe = [dict(k=1, g=None, x=2, a=0), dict(k=None, g=3, x=None, a=5)]
    out = []
    while len(out) < 16:
        p, v = _bool_expr(rnd, 3), _int_expr(rnd, 3)
        try:
            for env in probe:
                m_eval(p, env), m_eval(v, env)
        except NotImplementedError:
            continue
        out.append((p, v))
    return out


def _random_table(sess, seed):
    rnd = random.Random(seed)
    n = 300
    lists = [None if rnd.random() < 0.1 else
             [None if rnd.random() < 0.15 else rnd.randint(-4, 8) for _ in range(rnd.randint(0, 40))] for _ in range(n)]
    ks = [None if rnd.random() < 0.1 else rnd.randint(-2, 5) for _ in range(n)]
    gs = [None if rnd.random() < 0.2 else rnd.randint(0, 3) for _ in range(n)]
    t = sess.table([("k", T_INT, ks, None), ("g", T_INT, gs, None), ("xs", T_LIST, lists, None)], nrows=n)
    return t, [dict(k=k, g=g, xs=v) for k, g, v in zip(ks, gs, lists)]


@pytest.mark.gpu
@pytest.mark.parametrize("group", range(8))
def test_random_trees(gpu_session, group):
    t, rows = _random_table(gpu_session, group)
    ran = 0
    for p, v in _random_cases(group):
        items = [(e, f"c{j}") for j, (_, e) in enumerate(seven(p, v))]
        out = t.withColumns(*items, header=H, params={})
        for e, c in items:
            got = out.column_values(c)
            assert same(got, [m_eval(e, r) for r in rows]), (group, str(e))
            ran += 1
    assert ran == 16 * 7


# ------------------------------------------------------ GPU: binding type checks
@pytest.mark.gpu
def test_list_lambda_binding_type_checks(gpu_session):
    """capf_table_list_lambda rejects a malformed call when the node is built."""
    from ctypes import byref
    t = gpu_session.table([("k", T_INT, [1, 2], None), ("xs", T_LIST, [[1], [2, 3]], None)], nrows=2)
    pe, keep1 = _lib._keepalive_expr(_compile(GreaterThan(x, I(0)), {"x": (0, T_INT)}))
    be, keep2 = _lib._keepalive_expr(_compile(Add(a, x), {"a": (0, T_INT), "x": (1, T_INT)}))
    free, keep3 = _lib._keepalive_expr(_compile(Add(a, x), {"a": (1, T_INT), "x": (0, T_INT)}))
    bad = [(1, b"xs", None, None, b"", T_BOOL),          # a quantifier without pred
           (5, b"xs", None, byref(be), b"", T_INT),      # REDUCE without init
           (5, b"xs", None, None, b"k", T_INT),          # REDUCE without body
           (1, b"k", byref(pe), None, b"", T_BOOL),      # a non-LIST list
           (9, b"xs", byref(pe), None, b"", T_BOOL),     # an unknown kind
           (-1, b"xs", byref(pe), None, b"", T_BOOL),
           (0, b"xs", byref(free), None, b"", T_INT),    # slot 1 outside reduce
           (0, b"xs", byref(pe), None, b"", T_STRING),   # a filter declared with another element type
           (5, b"xs", None, byref(be), b"xs", T_INT)]    # a LIST init
    for kind, lst, p, b, init, ot in bad:
        with pytest.raises((_lib.IllegalArgumentException, _lib.NotImplementedException)):
            t._new("capf_table_list_lambda", t._h, kind, lst, p, b, init, ot, b"z")
    ok = t._new("capf_table_list_lambda", t._h, 5, b"xs", None, byref(be), b"k", T_INT, b"z")
    assert ok.column_values("z") == [2, 7]
    # CAPF_OP_LAMBDA outside a lambda program
    with pytest.raises(_lib.IllegalArgumentException):
        t._new("capf_table_filter", t._h, byref(pe))
