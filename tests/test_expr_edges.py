"""The expression interpreter (csrc/kernels_basic.hip run_program / k_eval, and
the filter_terms fast path) at numeric edges and at its program-shape limits.

Everything is compared with an exact scalar model written here in plain
Python `int` and `float` — Java `long` / `double` semantics, which is what
Flink's generated code computes (JLS 15.17, 15.18, 15.20, 15.21, 5.1.3) — and
not with oracle/table_np.py, which is itself checked against the model on the
CPU (test_oracle_matches_the_model).

  * INTEGER and BOOLEAN results compare exactly, FLOAT results by bit pattern
    (any NaN equals any NaN).  There is no tolerance: IEEE fixes + − × /,
    fmod is exact, the rest are selections and casts.
  * Every expression runs as a projection (withColumns) and as a predicate
    (filter).  A BOOLEAN expression is its own predicate — a row passes iff
    the value is TRUE; any other expression e runs as the predicate `e <= 0`.
  * Round is half away from zero with the operand's sign on a zero result
    (C99 round; the interpreter and the oracle both compute trunc(x) ± 1).
  * `<>` is Not(Equals(..)), as expr.py has no other spelling; CAPF_OP_NEQ —
    what the JVM mapper emits for it — is driven through raw programs.

Row counts: no table's is a multiple of 4 and the pair tables hold more than
256 rows, so that column/literal integer comparisons cover the quad kernel
and the tail kernel of filter_terms.
"""
import math
import struct
from ctypes import byref
from fractions import Fraction

import pytest

from capf_amd import _lib
from capf_amd.expr import (OP_AND, OP_COALESCE, OP_COL, OP_LIT_INT, OP_NEG, OP_NEQ, OP_OR, Abs, Add, Ands, Ceil,
                           Coalesce, Divide, Equals, FloatLit, Floor, GreaterThan, GreaterThanOrEqual, In, IntegerLit,
                           IsNotNull, IsNull, LessThan, LessThanOrEqual, Modulo, Multiply, Negate, Not, Ors, Round, Sign, Sqrt,
                           Subtract, ToFloat, ToInteger, Var, compile_program, T_BOOL, T_FLOAT, T_INT, T_LIST)
from capf_amd.header import RecordHeader
from oracle.table_np import OracleSession

MIN, MAX = -(1 << 63), (1 << 63) - 1
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------ the model
def is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def wrap64(x):
    """The low 64 bits of x as a Java long."""
    return ((x + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


def m_arith(op, a, b):
    """a op b.  Two longs: + − × wrap, / truncates toward zero, % takes the
    dividend's sign, x / 0 and x % 0 are NULL (the kernel's and the oracle's
    answer, where Java throws).  Otherwise doubles — a long operand widens by
    (double), round to nearest even — and % is fmod."""
    if a is None or b is None:
        return None
    if is_int(a) and is_int(b):
        if op == "+":
            return wrap64(a + b)
        if op == "-":
            return wrap64(a - b)
        if op == "*":
            return wrap64(a * b)
        if b == 0:
            return None
        q = abs(a) // abs(b)
        if (a < 0) != (b < 0):
            q = -q
        return wrap64(q) if op == "/" else a - q * b
    x, y = float(a), float(b)
    if op == "+":
        return x + y
    if op == "-":
        return x - y
    if op == "*":
        return x * y
    if op == "/":
        if y == 0.0:  # (Python raises where IEEE answers)
            if x == 0.0 or x != x:
                return NAN
            return math.copysign(INF, x) * math.copysign(1.0, y)
        return x / y
    if x != x or y != y or math.isinf(x) or y == 0.0:
        return NAN
    return math.fmod(x, y)


def m_cmp(op, a, b):
    """Java primitive comparison: two longs exactly; otherwise as doubles
    ((double) of a long operand), IEEE — with a NaN only <> holds."""
    if a is None or b is None:
        return None
    if not (is_int(a) and is_int(b)):
        a, b = float(a), float(b)
    return {"=": a == b, "<>": a != b, "<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b}[op]


def _zero_of(r, x):
    """r, a zero result carrying x's sign."""
    return math.copysign(0.0, x) if r == 0.0 else r


def m_unary(name, v):
    if v is None:
        return None
    if isinstance(v, bool):  # toInteger / toFloat of a BOOLEAN: NULL
        assert name in ("ToInteger", "ToFloat"), name
        return None
    if name == "ToFloat":
        return float(v)
    if name == "ToInteger":  # Flink casts to INT: Java (int)
        if is_int(v):
            return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
        if v != v:
            return 0
        if v >= 2147483647.0:
            return 2147483647
        if v <= -2147483648.0:
            return -2147483648
        return int(v)
    if name == "Round":  # half away from zero, a FLOAT also for an INTEGER
        if is_int(v):
            return float(v)
        if v != v or math.isinf(v):
            return v
        n = int(v)
        f = Fraction(v) - n
        if f >= Fraction(1, 2):
            n += 1
        elif f <= Fraction(-1, 2):
            n -= 1
        return _zero_of(float(n), v)
    if is_int(v):  # these keep an INTEGER operand's type
        return {"Abs": wrap64(abs(v)), "Negate": wrap64(-v), "Sign": (v > 0) - (v < 0), "Ceil": v, "Floor": v}[name]
    if name == "Abs":
        return abs(v)
    if name == "Negate":
        return -v
    if name == "Sign":
        return 1.0 if v > 0 else -1.0 if v < 0 else v  # ±0.0 and NaN as they are
    if name in ("Ceil", "Floor"):
        if v != v or math.isinf(v):
            return v
        return _zero_of(float(math.ceil(v) if name == "Ceil" else math.floor(v)), v)
    if name == "Sqrt":
        return NAN if v != v or v < 0 else math.sqrt(v)
    raise AssertionError(name)


def m_nary(name, vals):
    if name == "Coalesce":
        return next((v for v in vals if v is not None), None)
    dom = name == "Ors"  # the dominant value: FALSE for AND, TRUE for OR
    if any(v is dom for v in vals):
        return dom
    return None if any(v is None for v in vals) else not dom


def m_in(x, xs):
    """x IN xs, in CAPF_OP_IN_LIST's order: a NULL list NULL, an empty list
    FALSE, a NULL x NULL, an equal element TRUE, else NULL when the list holds
    a NULL element, else FALSE.  Equality is `=`: a NaN equals nothing."""
    if xs is None:
        return None
    if not xs:
        return False
    if x is None:
        return None
    if any(e is not None and m_cmp("=", e, x) for e in xs):
        return True
    return None if any(e is None for e in xs) else False


_ARITH = {"Add": "+", "Subtract": "-", "Multiply": "*", "Divide": "/", "Modulo": "%"}
_CMP = {"Equals": "=", "LessThan": "<", "LessThanOrEqual": "<=", "GreaterThan": ">", "GreaterThanOrEqual": ">="}
_BOOLEAN = set(_CMP) | {"Not", "IsNull", "IsNotNull", "Ands", "Ors", "In"}


def model(e, row):
    n = type(e).__name__
    if n == "Var":
        return row[e.vname]
    if n in ("IntegerLit", "FloatLit"):
        return e.v
    if n in _ARITH:
        return m_arith(_ARITH[n], model(e.lhs, row), model(e.rhs, row))
    if n in _CMP:
        return m_cmp(_CMP[n], model(e.lhs, row), model(e.rhs, row))
    if n == "Not":
        v = model(e.expr, row)
        return None if v is None else not v
    if n in ("IsNull", "IsNotNull"):
        return (model(e.expr, row) is None) == (n == "IsNull")
    if n in ("Ands", "Ors", "Coalesce"):
        return m_nary(n, [model(x, row) for x in e.exprs])
    if n == "In":
        return m_in(model(e.lhs, row), model(e.rhs, row))
    return m_unary(n, model(e.expr, row))


def same(x, y):
    """Typed equality: NULL, BOOLEAN and INTEGER exactly, FLOAT by bit pattern
    with any NaN equal to any NaN."""
    if x is None or y is None:
        return x is None and y is None
    if isinstance(x, bool) or isinstance(y, bool):
        return isinstance(x, bool) and isinstance(y, bool) and x == y
    if isinstance(x, float) or isinstance(y, float):
        if not (isinstance(x, float) and isinstance(y, float)):
            return False
        if x != x or y != y:
            return x != x and y != y
        return struct.pack("<d", x) == struct.pack("<d", y)
    return is_int(x) and is_int(y) and x == y


# ----------------------------------------------------------------- the tables
E_VALS = [MIN, MIN + 1, -2 ** 31 - 1, -2 ** 31, -3, -1, 0, 1, 2, 3, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 53, 2 ** 53 + 1,
          MAX - 1, MAX, None]


def _pm(*xs):
    return [s * x for x in xs for s in (1.0, -1.0)]


F_VALS = ([NAN] + _pm(INF, 0.0, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 0.49999999999999994, 0.5, 1.5,
                      2.5, 4503599627370495.5, 2.0 ** 53) +
          [2147483647.0, 2147483647.5, 2147483648.0, -2147483648.0, -2147483648.5, -2147483649.0] + _pm(1e19) + [None])


class Tab:
    """Host columns [(name, capf type, values)] plus a row id; the rows as
    dicts for the model; one upload per session."""

    def __init__(self, cols):
        n = len(cols[0][2])
        assert all(len(v) == n for _, _, v in cols) and n % 4 != 0, n
        self.cols = [("id", T_INT, list(range(n)))] + [(c, t, list(v)) for c, t, v in cols]
        self.n = n
        self.rows = [{c: v[i] for c, _, v in self.cols} for i in range(n)]
        self.header = RecordHeader({Var(c): c for c, _, _ in self.cols})
        self._on = {}

    def on(self, session, compact=None):
        key = (id(session), compact)
        if key not in self._on:
            t = session.table([(c, ty, v, None) for c, ty, v in self.cols])
            self._on[key] = t if compact is None else t.compact(compact)
        return self._on[key]


def _pairs(xs, ys, pad):
    return [x for x in xs for _ in ys] + [pad[0]], [y for _ in xs for y in ys] + [pad[1]]


def _bools(n):
    return [(True, False, None)[i % 3] for i in range(n)]


_TABS = {}


def tab(name):
    """The tables, built once: 'ii' E × E (325 rows), 'ff' F × F (1025),
    'fe' F × E (577), 'in' a FLOAT x against FLOAT lists (57)."""
    if name not in _TABS:
        if name == "ii":
            a, b = _pairs(E_VALS, E_VALS, (7, -5))
            _TABS[name] = Tab([("a", T_INT, a), ("b", T_INT, b), ("p", T_BOOL, _bools(len(a)))])
        elif name == "ff":
            f, g = _pairs(F_VALS, F_VALS, (0.25, -8.0))
            _TABS[name] = Tab([("f", T_FLOAT, f), ("g", T_FLOAT, g)])
        elif name == "fe":
            f, a = _pairs(F_VALS, E_VALS, (0.25, 9))
            _TABS[name] = Tab([("f", T_FLOAT, f), ("a", T_INT, a)])
        elif name == "in":
            xs = [NAN, 1.0, -0.0, 0.0, INF, None, 2.5]
            ls = [[NAN], [NAN, 1.0], [None, NAN], [0.0], [-0.0, None], [], None, [INF, NAN, 2.5]]
            x, l = _pairs(xs, ls, (1.0, [1.0]))
            _TABS[name] = Tab([("x", T_FLOAT, x), ("xs", T_LIST, l)])
        else:
            raise KeyError(name)
    return _TABS[name]


def neq(a, b):
    return Not(Equals(a, b))


ARITH = [Add, Subtract, Multiply, Divide, Modulo]
CMPS = [Equals, neq, LessThan, LessThanOrEqual, GreaterThan, GreaterThanOrEqual]
UNARY = [Abs, Negate, Sign, Ceil, Floor, Round, ToFloat, ToInteger]
INT_LITS = [MIN, -1, 0, 3, MAX]


def group(name):
    """(table, expressions) of one named group of the issue's cases."""
    a, b, f, g, p = Var("a"), Var("b"), Var("f"), Var("g"), Var("p")
    if name == "int_pairs":  # col ∘ col
        return tab("ii"), [op(a, b) for op in ARITH + CMPS]
    if name == "int_literals":  # col ∘ lit and lit ∘ col
        return tab("ii"), [x for v in INT_LITS for op in ARITH + CMPS
                           for x in (op(a, IntegerLit(v)), op(IntegerLit(v), b))]
    if name == "int_unary":
        return tab("ii"), [op(a) for op in UNARY] + [ToInteger(p), ToFloat(p)]
    if name == "float_pairs":
        return tab("ff"), [op(f, g) for op in ARITH + CMPS]
    if name == "mixed":  # F × E: the comparisons and + / with (double)long
        return tab("fe"), [x for op in CMPS + [Add, Divide] for x in (op(f, a), op(a, f))]
    if name == "float_unary":
        return tab("ff"), [op(f) for op in UNARY]
    if name == "nan_logic":  # NOT / IS NULL / AND / OR around comparisons that hold a NaN
        one = FloatLit(1.0)
        return tab("ff"), [Not(LessThanOrEqual(f, g)), Not(GreaterThan(f, g)), IsNull(Equals(f, g)),
                           IsNotNull(LessThan(f, g)), Ands(LessThanOrEqual(f, g), GreaterThanOrEqual(f, g)),
                           Ands(neq(f, g), IsNotNull(f), IsNotNull(g)), Ors(LessThan(f, g), Equals(f, g)),
                           Ors(Equals(f, g), GreaterThan(f, g), LessThan(f, g)), Ors(neq(f, f), IsNull(g)),
                           Ands(Not(LessThan(f, one)), Not(GreaterThanOrEqual(f, one))),
                           LessThanOrEqual(f, one), Not(Equals(f, one)), Equals(f, FloatLit(NAN)),
                           neq(f, FloatLit(NAN)), GreaterThanOrEqual(FloatLit(NAN), g),
                           LessThanOrEqual(Sqrt(f), FloatLit(2.0)), Equals(f, f), GreaterThanOrEqual(f, f)]
    if name == "in_list":
        x, xs = Var("x"), Var("xs")
        return tab("in"), [In(x, xs), In(FloatLit(NAN), xs), In(FloatLit(1.0), xs), In(FloatLit(0.0), xs),
                           Not(In(x, xs)), IsNull(In(x, xs))]
    raise KeyError(name)


ORACLE_GROUPS = ["int_pairs", "int_literals", "int_unary", "float_pairs", "mixed", "float_unary", "nan_logic"]
# (oracle/table_np.py evaluates no IN over a LIST column: "in_list" has the model alone)


# ------------------------------------------------------------------ checking
def project(t, header, exprs, batch=16):
    """The value columns of `exprs` over table t, `batch` programs per call."""
    out = []
    for k in range(0, len(exprs), batch):
        part = exprs[k:k + batch]
        names = [f"x{j}" for j in range(len(part))]
        r = t.withColumns(*zip(part, names), header=header, params={})
        out += [r.column_values(c) for c in names]
    return out


def projection_diffs(t, tb, exprs):
    bad = []
    wants = [[model(e, row) for row in tb.rows] for e in exprs]
    for e, got, want in zip(exprs, project(t, tb.header, exprs), wants):
        rows = [i for i in range(tb.n) if len(got) != tb.n or not same(got[i], want[i])]
        if rows:
            i = rows[0]
            bad.append((str(e), len(rows), {k: v for k, v in tb.rows[i].items() if k != "id"},
                        got[i] if len(got) == tb.n else len(got), want[i]))
    return bad


def predicate_of(e):
    return e if type(e).__name__ in _BOOLEAN else LessThanOrEqual(e, IntegerLit(0))


def predicate_diffs(t, tb, exprs):
    bad = []
    for e in exprs:
        p = predicate_of(e)
        want = [row["id"] for row in tb.rows if model(p, row) is True]
        got = t.filter(p, tb.header, {}).column_values("id")
        if got != want:
            odd = sorted(set(got) ^ set(want))
            bad.append((str(p), len(odd), [{k: v for k, v in tb.rows[i].items() if k != "id"} for i in odd[:2]]))
    return bad


def check(t, tb, exprs):
    bad = projection_diffs(t, tb, exprs)
    assert not bad, f"{len(bad)} of {len(exprs)} projections differ (expr, rows, first row, got, want): {bad[:6]}"
    bad = predicate_diffs(t, tb, exprs)
    assert not bad, f"{len(bad)} of {len(exprs)} predicates differ (predicate, rows, first rows): {bad[:6]}"


# ------------------------------------------------------------------ CPU tests
def test_model_states_the_jls_facts():
    assert m_arith("/", -7, 2) == -3 and m_arith("%", -7, 2) == -1
    assert m_arith("/", 7, -2) == -3 and m_arith("%", 7, -2) == 1
    assert m_arith("/", MIN, -1) == MIN and m_arith("%", MIN, -1) == 0
    assert m_arith("/", MIN, 3) == -3074457345618258602 and m_arith("%", MIN, 3) == -2
    assert m_arith("/", MIN, MIN) == 1 and m_arith("/", MAX, MIN) == 0 and m_arith("%", MAX, MIN) == MAX
    assert m_arith("+", MAX, 1) == MIN and m_arith("-", MIN, 1) == MAX and m_arith("*", MIN, -1) == MIN
    assert m_arith("*", 2 ** 32, 2 ** 32) == 0 and m_arith("*", MAX, MAX) == 1
    assert m_arith("/", 5, 0) is None and m_arith("%", 5, 0) is None and m_arith("+", None, 1) is None
    assert m_unary("ToInteger", 3e9) == 2147483647 and m_unary("ToInteger", -3e9) == -2147483648
    assert m_unary("ToInteger", NAN) == 0 and m_unary("ToInteger", -1.9) == -1 and m_unary("ToInteger", 2147483647.5) == 2147483647
    assert m_unary("ToInteger", 2 ** 32 + 5) == 5 and m_unary("ToInteger", 2 ** 31) == -2 ** 31 and m_unary("ToInteger", MIN) == 0
    assert m_unary("ToInteger", True) is None and m_unary("ToFloat", False) is None
    assert m_unary("ToFloat", 2 ** 53 + 1) == 9007199254740992.0 and m_unary("ToFloat", MAX) == 2.0 ** 63
    assert m_unary("ToFloat", MAX - 1) == 2.0 ** 63 and m_unary("ToFloat", MIN) == -2.0 ** 63
    assert [m_unary("Round", v) for v in (0.5, -0.5, 1.5, 2.5, -2.5, 0.49999999999999994, 4503599627370495.5)] == \
        [1.0, -1.0, 2.0, 3.0, -3.0, 0.0, 4503599627370496.0]
    assert same(m_unary("Round", 7), 7.0) and same(m_unary("Round", -0.0), -0.0) and same(m_unary("Round", -0.3), -0.0)
    assert m_unary("Abs", MIN) == MIN and m_unary("Negate", MIN) == MIN and m_unary("Abs", MIN + 1) == MAX
    assert same(m_unary("Sign", -0.0), -0.0) and same(m_unary("Sign", NAN), NAN) and same(m_unary("Sign", -3), -1)
    assert same(m_unary("Ceil", -0.5), -0.0) and same(m_unary("Floor", -0.0), -0.0) and same(m_unary("Floor", -0.5), -1.0)
    assert same(m_unary("Ceil", 5), 5) and same(m_unary("Abs", -0.0), 0.0) and same(m_unary("Negate", 0.0), -0.0)
    assert same(m_arith("%", -1.5, 0.5), -0.0) and same(m_arith("%", 5.5, INF), 5.5) and same(m_arith("%", INF, 2.0), NAN)
    assert same(m_arith("/", 1.0, -0.0), -INF) and same(m_arith("/", 0.0, 0.0), NAN) and same(m_arith("/", 1, 2.0), 0.5)
    assert same(m_arith("+", 2 ** 53 + 1, 0.0), 9007199254740992.0) and same(m_arith("*", 1.7976931348623157e308, 2.5), INF)
    for op, want in (("=", False), ("<", False), ("<=", False), (">", False), (">=", False), ("<>", True)):
        assert m_cmp(op, NAN, 1.0) is want and m_cmp(op, 1, NAN) is want and m_cmp(op, NAN, NAN) is want
    assert m_cmp("=", -0.0, 0.0) and m_cmp("=", 2 ** 53 + 1, 2.0 ** 53) and not m_cmp("=", 2 ** 53 + 1, 2 ** 53)
    assert m_cmp("=", MAX, 2.0 ** 63) and m_cmp("<", MAX - 1, MAX) and m_cmp("<=", None, 1) is None
    assert m_in(NAN, [NAN]) is False and m_in(NAN, [None, NAN]) is None and m_in(1.0, [NAN, 1.0]) is True
    assert m_in(None, []) is False and m_in(1.0, None) is None and m_in(0.0, [-0.0, None]) is True
    assert not same(1, 1.0) and not same(0.0, -0.0) and not same(True, 1) and same(NAN, -NAN)
    assert len(E_VALS) == 18 and len(F_VALS) == 32


@pytest.mark.parametrize("name", ORACLE_GROUPS + ["windows", "shape"])
def test_oracle_matches_the_model(name):
    """oracle/table_np.py on every table and expression of the GPU tests."""
    o = OracleSession()
    if name == "windows":
        for _, _, tb in windows():
            check(tb.on(o), tb, window_exprs(tb))
    elif name == "shape":
        tb = shape_tab()
        check(tb.on(o), tb, shape_exprs())
        for kind in ("Ands", "Ors", "Coalesce"):
            nt = nary_tab(kind)
            check(nt.on(o), nt, nary_exprs(kind))
    else:
        tb, exprs = group(name)
        check(tb.on(o), tb, exprs)


# ------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("name", ORACLE_GROUPS + ["in_list"])
def test_edge_values_on_the_gpu(gpu_session, name):
    tb, exprs = group(name)
    check(tb.on(gpu_session), tb, exprs)


@pytest.mark.gpu
def test_nan_predicates_both_ways(gpu_session):
    """`f <= 1.0` drops the NaN rows, `NOT (f = 1.0)` keeps them — and
    sqrt of a negative is no number that is <= 2."""
    tb = tab("ff")
    t, f = tb.on(gpu_session), Var("f")
    nan_rows = {r["id"] for r in tb.rows if r["f"] is not None and r["f"] != r["f"]}
    assert len(nan_rows) == len(F_VALS)
    le = set(t.filter(LessThanOrEqual(f, FloatLit(1.0)), tb.header, {}).column_values("id"))
    assert not le & nan_rows
    assert le == {r["id"] for r in tb.rows if r["f"] is not None and r["f"] <= 1.0}
    ne = set(t.filter(Not(Equals(f, FloatLit(1.0))), tb.header, {}).column_values("id"))
    assert nan_rows <= ne
    assert ne == {r["id"] for r in tb.rows if r["f"] is not None and r["f"] != 1.0}
    sq = set(t.filter(LessThanOrEqual(Sqrt(f), FloatLit(2.0)), tb.header, {}).column_values("id"))
    assert sq == {r["id"] for r in tb.rows if r["f"] is not None and 0.0 <= r["f"] <= 4.0}


@pytest.mark.gpu
def test_bare_literals_are_constant_columns(gpu_session):
    """IntegerLit(MIN), FloatLit(-0.0), FloatLit(nan) as projections: the
    constant-column shortcut of eval_program keeps every bit."""
    tb = tab("ii")
    exprs = [IntegerLit(MIN), FloatLit(-0.0), FloatLit(NAN), IntegerLit(MAX)]
    bad = projection_diffs(tb.on(gpu_session), tb, exprs)
    assert not bad, bad


def _raw(t, ops, ia, names, pred):
    """A program given as opcodes (what the JVM mapper sends) as a projection
    `x` or as a filter; returns the values / the surviving ids."""
    prog = (list(ops), list(ia), [0.0] * len(ops), list(names))
    if pred:
        e, keep = _lib._keepalive_expr(prog)
        return t._new("capf_table_filter", t._h, byref(e), cols=t._cols).column_values("id")
    arr, keep = _lib.expr_array([prog])
    return t._new("capf_table_with_columns", t._h, 1, arr, _lib.strs(["x"])).column_values("x")


@pytest.mark.gpu
def test_neq_opcode(gpu_session):
    """CAPF_OP_NEQ (GpuExprMapper.scala lowers Not(Equals) to it): col <> col
    over E × E and F × F, col <> literal over E (the filter_terms path)."""
    cases = [(tab("ii"), "a", "b", None), (tab("ff"), "f", "g", None)] + \
        [(tab("ii"), "a", None, v) for v in INT_LITS]
    for tb, l, r, v in cases:
        t = tb.on(gpu_session)
        ops, ia, names = ([OP_COL, OP_COL, OP_NEQ], [0, 1, 0], [l, r]) if r else \
            ([OP_COL, OP_LIT_INT, OP_NEQ], [0, v, 0], [l])
        want = [m_cmp("<>", row[l], row[r] if r else v) for row in tb.rows]
        got = _raw(t, ops, ia, names, False)
        assert all(same(x, y) for x, y in zip(got, want)) and len(got) == tb.n, (l, r, v)
        assert _raw(t, ops, ia, names, True) == [i for i, w in enumerate(want) if w is True], (l, r, v)


# ------------------------------------------------------------ encoded operands
def windows():
    """(compact width, base, table): value windows as wide as FOR24 (2^24 − 1)
    and FOR32 (2^32 − 1) allow, based at MIN, straddling zero, and ending at
    MAX — ld_int adds an unsigned offset to `base` at both ends of the range."""
    out = []
    for width, w in ((3, (1 << 24) - 1), (4, (1 << 32) - 1)):
        for base in (MIN, -(1 << 23), MAX - w):
            vals = sorted({base, base + 1, base + 2, base + w // 2, base + w - 1, base + w} |
                          ({-1, 0, 1} if base < 0 <= base + w else set())) + [None]
            a, b = _pairs(vals, vals, (base, base + w))
            if len(a) % 4 == 0:
                a, b = a + [base + w], b + [base]
            out.append((width, base, Tab([("a", T_INT, a), ("b", T_INT, b)])))
    return out


def window_exprs(tb):
    a, b = Var("a"), Var("b")
    lits = [-1, 3, min(r["a"] for r in tb.rows if r["a"] is not None) + 1]
    return [op(a, b) for op in ARITH + CMPS] + \
        [x for v in lits for op in ARITH + CMPS for x in (op(a, IntegerLit(v)), op(IntegerLit(v), b))]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(6))
def test_encoded_operands(gpu_session, k):
    width, base, tb = windows()[k]
    t = tb.on(gpu_session, compact=width)
    assert t.encoding("a") == (2 if width == 3 else 1, base) and t.encoding("b") == (2 if width == 3 else 1, base)
    assert t.column_values("a") == [r["a"] for r in tb.rows]
    check(t, tb, window_exprs(tb))


# --------------------------------------------------------------- program shape
NCOLS = 49
C = [Var(f"c{i}") for i in range(NCOLS)]


def shape_tab():
    """49 INTEGER columns of small values, 7 rows; a NULL in the last row."""
    if "shape" not in _TABS:
        cols = [(f"c{i}", T_INT, [(i * 7 + r * 3) % 11 - 4 + r for r in range(7)]) for i in range(NCOLS)]
        cols[5][2][6] = None
        _TABS["shape"] = Tab(cols)
    return _TABS["shape"]


def left_sum(k):
    e = C[0]
    for x in C[1:k]:
        e = Add(e, x)
    return e


def right_sum(k):
    e = C[k - 1]
    for x in reversed(C[:k - 1]):
        e = Add(x, e)
    return e


def shape_exprs():
    """Sums of 32 / 33 distinct columns (the 32-view LDS limit), 96 and 97
    instructions (the LDS code limit), a stack 24 deep."""
    return [left_sum(32), left_sum(33), Negate(left_sum(48)), left_sum(49), right_sum(24), right_sum(5),
            Multiply(right_sum(23), left_sum(33))]


POS = [0, 7, 8, 15, 16, 23, 24, 39]
NARY_ROWS = [(None, None)] + [(p, None) for p in POS] + [(None, q) for q in POS] + \
    [(0, 39), (39, 0), (7, 8), (8, 7), (23, 24), (24, 23), (16, 0), (24, 39), (39, 24), (15, 16)]
NARY_KS = (1, 2, 8, 9, 16, 17, 24, 25, 40)


def nary_tab(kind):
    """40 operand columns, one row per (position of the dominant value,
    position of a NULL).  Ands / Ors: BOOLEAN columns, every other value
    neutral.  Coalesce: INTEGER columns, NULL except i − 20 at the first
    position and i + 30 at the second (the predicate `e <= 0` tells them
    apart)."""
    key = "nary" + kind
    if key not in _TABS:
        cols = []
        for i in range(40):
            if kind == "Coalesce":
                v = [i - 20 if p == i else i + 30 if q == i else None for p, q in NARY_ROWS]
            else:
                v = [(kind == "Ors") if p == i else None if q == i else (kind == "Ands") for p, q in NARY_ROWS]
            cols.append((f"c{i}", T_INT if kind == "Coalesce" else T_BOOL, v))
        _TABS[key] = Tab(cols)
    return _TABS[key]


def nary_exprs(kind, ks=NARY_KS):
    cls = {"Ands": Ands, "Ors": Ors, "Coalesce": Coalesce}[kind]
    return [cls(*C[:k]) for k in ks] + [cls(*reversed(C[:k])) for k in ks if k > 8]


def _lower(e, tb):
    types = {c: t for c, t, _ in tb.cols}
    return compile_program(e, tb.header, set(types), {}, None, lambda c: types[c])


def _depth(ops, ia):
    """The deepest stack of a program of columns, +, unary − and n-ary ops
    (the host check of upload_program, restated)."""
    d = mx = 0
    for op, i in zip(ops, ia):
        d += 1 if op == OP_COL else 1 - i if op in (OP_AND, OP_OR, OP_COALESCE) else 0 if op == OP_NEG else -1
        mx = max(mx, d)
    assert d == 1
    return mx


def test_shape_programs_sit_on_the_limits():
    """Read off the lowered programs, not assumed: 32 / 33 views, 96 / 97
    instructions, depth 24 / 25."""
    tb = shape_tab()
    size = lambda e: (len(_lower(e, tb)[0]), len(_lower(e, tb)[3]))  # noqa: E731
    assert size(left_sum(32)) == (63, 32) and size(left_sum(33)) == (65, 33)
    assert size(Negate(left_sum(48))) == (96, 48) and size(left_sum(49)) == (97, 49)
    for k in (24, 25):
        ops, ia, _, _ = _lower(right_sum(k), tb)
        assert _depth(ops, ia) == k
    assert _depth(*_lower(left_sum(49), tb)[:2]) == 2


def _run(ops, ia, names, row):
    """AND / OR / COALESCE programs over columns, as run_program states them."""
    st = []
    for op, i in zip(ops, ia):
        if op == OP_COL:
            st.append(row[names[i]])
        else:
            vals = st[len(st) - i:]
            del st[len(st) - i:]
            st.append(m_nary({OP_AND: "Ands", OP_OR: "Ors", OP_COALESCE: "Coalesce"}[op], vals))
    assert len(st) == 1
    return st[0]


@pytest.mark.parametrize("kind", ["Ands", "Ors", "Coalesce"])
def test_nary_lowering_bounds_the_stack(kind):
    """Ands / Ors / Coalesce of any arity lower to chunks: the stack stays
    within 8 operands, up to 8 operands give the single n-ary instruction
    (the shape the filter fast path reads), and the chunked program computes
    what the n-ary operator does on every row."""
    tb = nary_tab(kind)
    opc = {"Ands": OP_AND, "Ors": OP_OR, "Coalesce": OP_COALESCE}[kind]
    for e in nary_exprs(kind):
        ops, ia, _, names = _lower(e, tb)
        k = len(e.exprs)
        assert _depth(ops, ia) == min(k, 8), k
        if k <= 8:
            assert list(ops) == [OP_COL] * k + [opc] and ia[-1] == k
        assert sum(1 for op in ops if op == OP_COL) == k
        for row in tb.rows:
            assert same(_run(ops, ia, names, row), model(e, row)), (k, row)


@pytest.mark.gpu
def test_program_shape_limits(gpu_session):
    """More than 32 column views and more than 96 instructions leave LDS for
    global memory; a stack 24 deep is the deepest that runs."""
    tb = shape_tab()
    check(tb.on(gpu_session), tb, shape_exprs())


@pytest.mark.gpu
def test_too_deep_is_refused_and_the_session_goes_on(gpu_session):
    """25 genuinely nested operands: NotImplementedException from the host
    check, before any launch; the next expression evaluates as usual."""
    tb = shape_tab()
    t = tb.on(gpu_session)
    with pytest.raises(_lib.NotImplementedException, match="too deep"):
        t.withColumns((right_sum(25), "x"), header=tb.header, params={}).column_values("x")
    with pytest.raises(_lib.NotImplementedException, match="too deep"):
        t.filter(GreaterThan(right_sum(25), IntegerLit(0)), tb.header, {}).column_values("id")
    check(t, tb, [right_sum(24), left_sum(25)])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["Ands", "Ors", "Coalesce"])
def test_nary_operators_of_any_arity(gpu_session, kind):
    """24, 25 and 40 operands (and the chunk boundaries below), NULLs and the
    dominant value in varying positions."""
    tb = nary_tab(kind)
    check(tb.on(gpu_session), tb, nary_exprs(kind))
