"""Lambda-expression cases transcribed from the shared acceptance suite:
MTa/ExpressionTests.scala:1502-1560 (list comprehension, 5 cases), :1575-1586
(reduce, 1 case) and :1588-1643 (any / none / all / single, 5 cases); the nested
comprehension :1562-1572 is kept apart as NESTED — nested lists are not
supported, so it is an expected NotImplemented.  Same format as
list_function_cases.py; the okapi IR is LambdaVar
(okapi-ir/.../ir/api/expr/Expr.scala:199), ListComprehension / ListReduction /
ListFilter / ListAny / ListNone / ListAll / ListSingle (:1178-1237).
"""
import capf_import  # noqa: F401
from capf_amd.expr import (Add, GreaterThan, IntegerLit, LambdaVar, LessThan, ListAll, ListAny, ListComprehension,
                           ListLit, ListNone, ListReduction, ListSingle, Multiply, StringLit, ToInteger, Var)
from capf_amd.planner import Query, Stage

ET = "MTa/ExpressionTests.scala:"


def I(v):  # noqa: E743
    return IntegerLit(v)


def _things(items, fn):
    # WITH <items> AS things RETURN fn(things) AS value
    return Query([], [Stage([("things", ListLit(*items))]), Stage([("value", fn(Var("things")))])])


n = LambdaVar("n")
acc = LambdaVar("acc")
ONE23 = [I(1), I(2), I(3)]
STR123 = [StringLit(c) for c in "123"]
N4 = Add(Multiply(ToInteger(n), I(3)), ToInteger(n))  # toInteger(n)*3 + toInteger(n)

CASES = [
    ("comprehension_static_mapping", ET + "1503-1513", "",
     _things(ONE23, lambda xs: ListComprehension(n, None, I(1), xs)), [{"value": [1, 1, 1]}]),
    ("comprehension_simple_mapping", ET + "1515-1525", "",
     _things(ONE23, lambda xs: ListComprehension(n, None, Multiply(n, I(3)), xs)), [{"value": [3, 6, 9]}]),
    ("comprehension_complex_mapping", ET + "1527-1537", "",
     _things(STR123, lambda xs: ListComprehension(n, None, N4, xs)), [{"value": [4, 8, 12]}]),
    ("comprehension_inner_predicate", ET + "1539-1549", "",
     _things(ONE23, lambda xs: ListComprehension(n, GreaterThan(n, I(2)), None, xs)), [{"value": [3]}]),
    ("comprehension_predicate_and_mapping", ET + "1551-1560", "",
     _things(STR123, lambda xs: ListComprehension(n, GreaterThan(ToInteger(n), I(2)), N4, xs)), [{"value": [12]}]),
    ("reduce_simple", ET + "1576-1585", "",
     _things(ONE23, lambda xs: ListReduction(acc, n, Add(acc, n), I(0), xs)), [{"value": 6}]),
    ("any", ET + "1589-1598", "", _things(ONE23, lambda xs: ListAny(n, LessThan(n, I(2)), xs)), [{"value": True}]),
    ("none", ET + "1600-1609", "", _things(ONE23, lambda xs: ListNone(n, LessThan(n, I(2)), xs)), [{"value": False}]),
    ("all", ET + "1611-1620", "", _things(ONE23, lambda xs: ListAll(n, LessThan(n, I(4)), xs)), [{"value": True}]),
    ("single_negative", ET + "1622-1631", "",
     _things(ONE23, lambda xs: ListSingle(n, LessThan(n, I(3)), xs)), [{"value": False}]),
    ("single_positive", ET + "1633-1642", "",
     _things(ONE23, lambda xs: ListSingle(n, LessThan(n, I(2)), xs)), [{"value": True}]),
]
assert len(CASES) == 11

# WITH [[1,2,3], [2,2,3], [3,4]] AS things RETURN [n IN things | [n IN n WHERE n < 2]] AS value
# expects [[1], [], []]: a list of lists, and a lambda expression inside a lambda body.
NESTED = ("comprehension_nested", ET + "1562-1572", "",
          _things([ListLit(I(1), I(2), I(3)), ListLit(I(2), I(2), I(3)), ListLit(I(3), I(4))],
                  lambda xs: ListComprehension(n, None, ListComprehension(n, LessThan(n, I(2)), None, n), xs)),
          [{"value": [[1], [], []]}])
