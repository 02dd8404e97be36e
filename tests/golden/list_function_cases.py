"""List function cases transcribed from the shared acceptance suite:
MTa/FunctionTests.scala:1502-1556 (range, 4 cases), :1631-1697 (head / tail /
last, 6 cases), :1710-1718 (reverse of a list, 1 case),
MTa/ExpressionTests.scala:47-80 (slices, 4 cases) and MTa/NullTests.scala:55-57,
63, 107 (5 cases).  Same format as string_predicate_cases.py; the okapi IR is
Head / Last / Reverse (okapi-ir/.../ir/api/expr/Expr.scala:640-653), Range
(:859-880) and ListSliceFromTo / ListSliceFrom / ListSliceTo (:1166-1176).
tail(xs) is ListSliceFrom(xs, 1), as the front end rewrites it.
"""
import capf_import  # noqa: F401
from capf_amd.expr import (ElementProperty, Head, IntegerLit, Last, ListLit, ListSliceFrom, ListSliceFromTo,
                           ListSliceTo, NullLit, Range, Reverse, StringLit, Var)
from capf_amd.planner import Match, NodeP, Query, Stage, Unwind

NT = "MTa/NullTests.scala:"
ET = "MTa/ExpressionTests.scala:"
FT = "MTa/FunctionTests.scala:"
NL = NullLit()


def I(v):  # noqa: E743
    return IntegerLit(v)


def _unit(name, e):
    return Query([], [Stage([(name, e)])])


def _things(items, name, fn):
    # WITH <items> AS things RETURN fn(things) AS name
    return Query([], [Stage([("things", ListLit(*items))]), Stage([(name, fn(Var("things")))])])


def _unwind(rng):
    # UNWIND range(...) AS x RETURN x
    return Query([Unwind(rng, "x")], [Stage([("x", Var("x"))])])


def _match(e):
    # MATCH (n) RETURN <e> AS x
    return Query([Match([NodeP("n")])], [Stage([("x", e)])])


N = Var("n", "NODE")
ABCD = ListLit(*[StringLit(c) for c in "abcd"])
ONE23 = [I(1), I(2), I(3)]


def tail(xs):
    return ListSliceFrom(xs, I(1))


CASES = [
    ("range_literals", FT + "1503-1511", "", _unwind(Range(I(1), I(3))), [{"x": 1}, {"x": 2}, {"x": 3}]),
    ("range_literals_step", FT + "1513-1521", "", _unwind(Range(I(1), I(7), I(3))), [{"x": 1}, {"x": 4}, {"x": 7}]),
    ("range_columns", FT + "1523-1539",
     "CREATE (:A {from: 1, to: 2}) CREATE (:A {from: 1, to: 3}) CREATE (:A {from: 1, to: 4})",
     _match(Range(ElementProperty(N, "from", "INTEGER"), ElementProperty(N, "to", "INTEGER"))),
     [{"x": [1, 2]}, {"x": [1, 2, 3]}, {"x": [1, 2, 3, 4]}]),
    ("range_varying_step", FT + "1541-1555", "CREATE (:A {step: 2}) CREATE (:A {step: 3})",
     _match(Range(I(1), I(4), ElementProperty(N, "step", "INTEGER"))), [{"x": [1, 3]}, {"x": [1, 4]}]),
    ("head", FT + "1632-1641", "", _things(ONE23, "head", Head), [{"head": 1}]),
    ("head_empty", FT + "1643-1652", "", _things([], "head", Head), [{"head": None}]),
    ("tail", FT + "1654-1663", "", _things(ONE23, "tail", tail), [{"tail": [2, 3]}]),
    ("tail_empty", FT + "1665-1674", "", _things([], "tail", tail), [{"tail": None}]),
    ("last", FT + "1676-1685", "", _things(ONE23, "last", Last), [{"last": 3}]),
    ("last_empty", FT + "1687-1696", "", _things([], "last", Last), [{"last": None}]),
    ("reverse_list", FT + "1710-1718", "", _unit("rev", Reverse(ListLit(*ONE23))), [{"rev": [3, 2, 1]}]),
    ("slice", ET + "49-54", "", _unit("r", ListSliceFromTo(ABCD, I(0), I(3))), [{"r": ["a", "b", "c"]}]),
    ("slice_without_from", ET + "56-61", "", _unit("r", ListSliceTo(ABCD, I(3))), [{"r": ["a", "b", "c"]}]),
    ("slice_without_to", ET + "63-68", "", _unit("r", ListSliceFrom(ABCD, I(0))), [{"r": ["a", "b", "c", "d"]}]),
    ("slice_empty_list", ET + "70-79", "", _things([], "r", tail), [{"r": None}]),
    # calling: head(null) / last(null) / tail(null) / reverse(null) / range(null, null) → RETURN <call> AS res
    ("null_55", NT + "55", "", _unit("res", Head(NL)), [{"res": None}]),
    ("null_56", NT + "56", "", _unit("res", Last(NL)), [{"res": None}]),
    ("null_57", NT + "57", "", _unit("res", tail(NL)), [{"res": None}]),
    ("null_63", NT + "63", "", _unit("res", Reverse(NL)), [{"res": None}]),
    ("null_107", NT + "107", "", _unit("res", Range(NL, NL)), [{"res": None}]),
]
assert len(CASES) == 20
