"""STARTS WITH / ENDS WITH / CONTAINS cases transcribed from the shared
acceptance suite: MTa/ExpressionTests.scala:1169-1287 (9 cases) and
MTa/NullTests.scala:89-91 (3 cases).  Same format as expression_cases.py; the
okapi IR is StartsWith / EndsWith / Contains (okapi-ir/.../ir/api/expr/
Expr.scala:369-379).

The ENDS WITH and CONTAINS "can handle nulls" tests ask `n.s STARTS WITh n.r`
in the reference; they are transcribed as written.
"""
import capf_import  # noqa: F401
from capf_amd.expr import Contains, ElementProperty, EndsWith, NullLit, StartsWith, StringLit, Var
from capf_amd.planner import Match, NodeP, Query, Stage

NT = "MTa/NullTests.scala:"
ET = "MTa/ExpressionTests.scala:"
NL = NullLit()


def _unit(name, e):
    return Query([], [Stage([(name, e)])])


def _lits(cls, s, p):
    return _unit("x", cls(StringLit(s), StringLit(p)))


def _nulls_query():
    n = Var("n", "NODE")
    # MATCH (n) RETURN n.s STARTS WITh n.r as x
    return Query([Match([NodeP("n")])],
                 [Stage([("x", StartsWith(ElementProperty(n, "s", "STRING"), ElementProperty(n, "r", "STRING")))])])


def _nulls_graph(r):
    return f'CREATE ({{s: "foobar", r: null}}) CREATE ({{s: null, r: "{r}"}})'


TWO_NULLS = [{"x": None}, {"x": None}]

CASES = [
    ("strpred_starts_true", ET + "1170-1178", "", _lits(StartsWith, "foobar", "foo"), [{"x": True}]),
    ("strpred_starts_false", ET + "1180-1188", "", _lits(StartsWith, "foobar", "bar"), [{"x": False}]),
    ("strpred_starts_nulls", ET + "1190-1206", _nulls_graph("foo"), _nulls_query(), TWO_NULLS),
    ("strpred_ends_true", ET + "1210-1218", "", _lits(EndsWith, "foobar", "bar"), [{"x": True}]),
    ("strpred_ends_false", ET + "1220-1228", "", _lits(EndsWith, "foobar", "foo"), [{"x": False}]),
    ("strpred_ends_nulls", ET + "1230-1246", _nulls_graph("bar"), _nulls_query(), TWO_NULLS),
    ("strpred_contains_true", ET + "1250-1258", "", _lits(Contains, "foobarbaz", "baz"), [{"x": True}]),
    ("strpred_contains_false", ET + "1260-1268", "", _lits(Contains, "foobarbaz", "abc"), [{"x": False}]),
    ("strpred_contains_nulls", ET + "1270-1286", _nulls_graph("bar"), _nulls_query(), TWO_NULLS),
    # calling: null STARTS WITH null / null ENDS WITH null / null CONTAINS null → RETURN <call> AS res
    ("null_89", NT + "89", "", _unit("res", StartsWith(NL, NL)), [{"res": None}]),
    ("null_90", NT + "90", "", _unit("res", EndsWith(NL, NL)), [{"res": None}]),
    ("null_91", NT + "91", "", _unit("res", Contains(NL, NL)), [{"res": None}]),
]
assert len(CASES) == 12
