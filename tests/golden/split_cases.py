"""split cases transcribed from the shared acceptance suite:
MTa/FunctionTests.scala:1721-1746 (`describe("split")`, 2 cases).  Same format
as list_function_cases.py; the okapi IR is Split (okapi-ir/.../ir/api/expr/
Expr.scala:904-912), lowered by Morpheus to Spark's StringSplit
(SparkSQLExprMapper.scala:272).
"""
import capf_import  # noqa: F401
from capf_amd.expr import ElementProperty, Split, StringLit, Var
from capf_amd.planner import Match, NodeP, Query, Stage

FT = "MTa/FunctionTests.scala:"
N = Var("n", "NODE")

CASES = [
    # RETURN split("1,2,3", ",2,") AS split
    ("split_constant_delimiter", FT + "1722-1731", "",
     Query([], [Stage([("split", Split(StringLit("1,2,3"), StringLit(",2,")))])]),
     [{"split": ["1", "3"]}]),
    # MATCH (n) RETURN split(n.friends, n.delimiter) AS split
    ("split_variable_delimiter", FT + "1733-1745",
     "CREATE ({friends: 'Bob,Eve', delimiter: \",\"}), ({friends: 'Eve;Bob', delimiter: \";\"})",
     Query([Match([NodeP("n")])],
           [Stage([("split", Split(ElementProperty(N, "friends", "STRING"), ElementProperty(N, "delimiter", "STRING")))])]),
     [{"split": ["Bob", "Eve"]}, {"split": ["Eve", "Bob"]}]),
]
assert len(CASES) == 2
