"""split(original, delimiter): LIST<STRING> from two STRINGs (okapi Split,
Expr.scala:904-912; capf_table_str_split, csrc/string_fn.hip).

The reference is expr.split_fn — java.lang.String.split(regex, -1), what Spark
2.4.3's StringSplit computes — applied row by row in Python, plus the literal
answers below.  A plain delimiter (expr.plain_split_delimiter) is split on the
device string heap; any other on the host.  The session profile tells which
kernels ran: str_split_count / str_split_write (the thread tier; the count
pass's bytes = the subjects' bytes over the rows neither operand makes NULL +
41 per row), str_split_long_count / str_split_long_write (one wave per subject
of at least CAPF_STR_LONG bytes).  Lists are compared with ==, element order
included.
"""
import os
import re
import shutil
from ctypes import byref, c_int64, c_uint64, c_void_p

import numpy as np
import pytest

from conftest import case_parts
from split_cases import CASES

from capf_amd import _lib
from capf_amd.expr import (T_INT, T_LIST, T_NULL, T_STRING, ContainerIndex, Explode, In, IntegerLit,
                           ListComprehension, Equals, Not, NullLit, Size, Split, StringLit, ToUpper, Var, _static_type,
                           compile_program, fold_split, may_hold_list_fn, plain_split_delimiter, split_fn)
from capf_amd.header import RecordHeader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = RecordHeader({Var(c): c for c in ("k", "s", "d", "xs", "x", "z")})
S, D = Var("s"), Var("d")
KNOWN = [("1,2,3", ",2,", ["1", "3"]), ("boo:and:foo", "o", ["b", "", ":and:f", "", ""]), ("", ",", [""]),
         (",", ",", ["", ""]), ("aaa", "aa", ["", "a"]), ("aaaa", "aa", ["", "", ""]), ("abc", "abcd", ["abc"])]


def utf8_len(s):
    return len(s.encode("utf-8", "surrogatepass"))


def _dictionary(s):
    cnt, dig = c_int64(), c_uint64()
    _lib.call("capf_string_digest", s._h, byref(cnt), byref(dig))
    return [s.lookup(c) for c in range(cnt.value)], dig.value


def values(t, e, name="z"):
    out = t.withColumns((e, name), header=H, params={})
    assert [c for c in out.physicalColumns if c.startswith("\x03")] == [], out.physicalColumns
    return out.column_values(name)


def split_launches(prof):
    return sorted(k for k in prof if k.startswith("str_split"))


@pytest.fixture()
def sess():
    """A fresh session with profiling on (the dictionary and the profile are the test's own)."""
    from capf_amd.table import GpuSession
    s = GpuSession(0)
    s.set_profiling(True)
    yield s
    s.close()


# ------------------------------------------------------------------------ CPU
def test_split_fn_known_answers():
    for s, d, want in KNOWN:
        assert split_fn(s, d) == want, (s, d)
    assert split_fn("abc", "") == ["a", "b", "c", ""]
    assert split_fn("a1b22c", "[0-9]+") == ["a", "b", "c"]
    for s in ("", "abc", "x€y"):
        assert split_fn(s, ";") == [s]
    assert split_fn(None, ",") is None and split_fn("a", None) is None


def test_route_classifier():
    for d in (",", "ab", "€", " "):
        assert plain_split_delimiter(d), d
    for d in ("|", ".", "", "a*", "\ud800", "a\udfff"):
        assert not plain_split_delimiter(d), repr(d)


def test_static_type_and_hoisting_flags():
    e = Split(S, StringLit(","))
    assert _static_type(e, H, {"s"}, {}, lambda c: T_STRING) == T_LIST
    assert _static_type(Split(NullLit(), StringLit(",")), H, {"s"}, {}, lambda c: T_STRING) == T_NULL
    assert may_hold_list_fn(e) and may_hold_list_fn(Size(e)) and may_hold_list_fn(In(StringLit("q"), e))
    assert str(e) == "split(s, ',')"


def test_bare_split_is_a_table_operation():
    with pytest.raises(_lib.NotImplementedException):
        compile_program(Split(S, StringLit(",")), H, {"s"}, {}, lambda x: 7, lambda c: T_STRING)


def test_literals_fold_without_a_table():
    lit = fold_split(Split(StringLit("1,2,3"), StringLit(",2,")))
    assert [x.v for x in lit.items] == ["1", "3"]
    assert [x.v for x in fold_split(Split(StringLit("abc"), StringLit(""))).items] == ["a", "b", "c", ""]
    assert isinstance(fold_split(Split(NullLit(), StringLit(","))), NullLit)
    assert isinstance(fold_split(Split(StringLit("a"), NullLit())), NullLit)
    assert fold_split(Split(S, StringLit(","))) is None and fold_split(Split(StringLit("a"), D)) is None


def test_scala_and_jni_declare_the_entry_point():
    """Native.tableStrSplit (@native) and its JNI binding take the same
    parameters, the binding calls capf_table_str_split, and the mapper's twin
    chooses the route with the classifier's twin."""
    import okapi_scala_scan as sc
    srcs = sc.integration_sources()
    native, table, mapper, fns = (sc.strip_comments(srcs[f]) for f in
                                  ("Native.scala", "GpuTable.scala", "GpuExprMapper.scala", "GpuStringFunctions.scala"))
    assert re.search(r"@native\s+def\s+tableStrSplit\(table:\s*Long,\s*strCol:\s*String,\s*delimCol:\s*String,"
                     r"\s*name:\s*String\):\s*Long", native)
    jni = open(os.path.join(ROOT, "integration", "jni", "capf_jni.cpp")).read()
    assert re.search(r"JNI\(jlong,\s*tableStrSplit\)\(JNIEnv \*env,\s*jobject,\s*jlong t,\s*jstring strCol,"
                     r"\s*jstring delimCol,\s*jstring name\)", jni)
    assert "capf_table_str_split(T(t)," in jni
    header = open(os.path.join(ROOT, "include", "capf_gpu.h")).read()
    assert re.search(r"capf_table_str_split\(capf_table \*t, const char \*str_col, const char \*delim_col,\s*"
                     r"const char \*name, capf_table \*\*out\)", header)
    assert re.search(r"case\s+\w+:\s*Split\s*=>", mapper) and "Native.tableStrSplit(" in table
    assert "def plainSplitDelimiter(" in fns and "plainSplitDelimiter(" in table
    assert ".split(" in fns and ", -1)" in fns  # the host route is String.split(d, -1) itself


# ------------------------------------------------------------ GPU: thread tier
SUBJECTS = ["", "a", ",", ",,", "a,", ",a", "a,b", "a,,b", "abc", "aaa", "aaaa", "aaaaa", "abab", "aba", "x€y€", "€",
            "x\U0001F600,y", None]
# neighbours of odd lengths, so that subjects start at every byte alignment of the heap
FILL = ["q", "rst", "uvwxy", "z,z,z,z", "ab,", ",ab", "é", "ab€ab", "aab", "baa", "aabaa", ",abcd,", "abcdabcd"]
LITERALS = [",", "aa", "ab", "€", "abcd"]


def thread_rows():
    rows = []
    for i, x in enumerate(SUBJECTS):
        rows.append(x)
        rows.append(FILL[i % len(FILL)])
    return rows + FILL


def thread_table(s):
    rows = thread_rows()
    return s.table([("k", T_INT, list(range(len(rows))), None), ("s", T_STRING, rows, None)], nrows=len(rows)), rows


def run_thread_tier(s):
    t, rows = thread_table(s)
    d, _ = _dictionary(s)
    at, starts = 0, {}
    for x in d:
        starts[x] = at
        at += utf8_len(x)
    assert {starts[x] % 4 for x in rows if x is not None} == {0, 1, 2, 3}
    out = {}
    for lit in LITERALS:
        got = values(t, Split(S, StringLit(lit)))
        assert got == [split_fn(x, lit) for x in rows], (lit, got)
        out[lit] = got
    return out


@pytest.mark.gpu
def test_known_answers_on_the_device(sess):
    t = sess.table([("s", T_STRING, [k[0] for k in KNOWN], None), ("d", T_STRING, [k[1] for k in KNOWN], None)])
    out = t.withColumns((Split(S, D), "z"), header=H, params={})
    assert out.column_values("z") == [k[2] for k in KNOWN]
    assert out.capf_type("z") == T_LIST and out.list_elem_type("z") == T_STRING
    assert out.list_elem_valid("z", 1) is None  # elements are never NULL: no element validity
    assert split_launches(sess.profile()) == ["str_split_count", "str_split_write"]


@pytest.mark.gpu
def test_thread_tier_literals(sess, monkeypatch):
    monkeypatch.delenv("CAPF_STR_LONG", raising=False)
    run_thread_tier(sess)
    prof = sess.profile()
    assert prof["str_split_count"]["launches"] == prof["str_split_write"]["launches"] == len(LITERALS)
    assert "str_split_long_count" not in prof and "str_split_long_write" not in prof


@pytest.mark.gpu
def test_both_tiers_on_one_corpus(monkeypatch):
    """The thread-tier table again with CAPF_STR_LONG=8 in a fresh session:
    subjects of 8 bytes and more go to the wave tier, the results are equal."""
    from capf_amd.table import GpuSession
    monkeypatch.delenv("CAPF_STR_LONG", raising=False)
    a = GpuSession(0)
    want = run_thread_tier(a)
    a.close()
    monkeypatch.setenv("CAPF_STR_LONG", "8")
    b = GpuSession(0)
    b.set_profiling(True)
    got = run_thread_tier(b)
    prof = b.profile()
    b.close()
    assert got == want
    assert prof["str_split_long_count"]["launches"] == prof["str_split_long_write"]["launches"] == len(LITERALS)


@pytest.mark.gpu
def test_per_row_delimiter_column(sess):
    delims = [",", ";", "ab", None]
    subj = [x for x in SUBJECTS + ["a;b", ";", "ab;ab,ab"] for _ in delims]
    dl = [delims[(i + i // len(delims)) % len(delims)] for i in range(len(subj))]
    t = sess.table([("s", T_STRING, subj, None), ("d", T_STRING, dl, None)], nrows=len(subj))
    got = values(t, Split(S, D))
    assert got == [split_fn(a, b) for a, b in zip(subj, dl)]
    assert all(g is None for g, a in zip(got, subj) if a is None)
    assert all(g is None for g, b in zip(got, dl) if b is None)
    assert any(g is not None for g in got)
    # a NULL-typed operand: a NULL-typed column
    out = t.withColumns((Split(S, NullLit()), "z"), (Split(NullLit(), D), "y"), header=H, params={})
    assert out.capf_type("z") == T_NULL and out.capf_type("y") == T_NULL
    assert out.column_values("z") == [None] * len(subj)


# -------------------------------------------------------------- GPU: wave tier
def wave_rows():
    rows = []
    for n in (255, 256, 257, 64 * 5 - 1, 64 * 5, 64 * 5 + 1, 64 * 9 - 1, 64 * 9, 64 * 9 + 1):
        rows += ["x" * n, ("w,v" * n)[:n], "," * n, "x" * (n - 1) + ","]
    for at in (62, 63):  # a delimiter starting at bytes 62 and 63 of a window and ending in the next
        for window in (0, 1, 3):
            pad = 64 * window + at
            rows += ["x" * pad + "ab" + "y" * 300, "x" * pad + "abcde" + "y" * 300,
                     "x" * pad + "abab" + "y" * 200 + "abcdeabcde"]
    rows += ["a" * 130 + "b" * 130,          # "aa": the overlap resolution carried across windows
             "a" * 129 + "b" * 131, "b" + "a" * 259,
             "p" * 300 + "," + "q" * 300 + "ab" + "r" * 5,  # pieces of 300 bytes: copy_wave
             ",x" * 300,                      # 600 bytes, 300 one-byte pieces (and a leading "")
             "€" * 100 + ",é" * 50, None, "short,row"]
    return rows


@pytest.mark.gpu
def test_wave_tier(sess, monkeypatch):
    monkeypatch.delenv("CAPF_STR_LONG", raising=False)
    rows = wave_rows()
    assert {utf8_len(r) for r in rows if r} >= {255, 256, 257, 319, 320, 321, 575, 576, 577, 600}
    t = sess.table([("s", T_STRING, rows, None)], nrows=len(rows))
    lits = [",", "ab", "abcde", "aa", "x", "€"]
    for lit in lits:
        got = values(t, Split(S, StringLit(lit)))
        want = [split_fn(x, lit) for x in rows]
        bad = [(lit, i, len(rows[i])) for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, bad[:5]
    assert split_fn("a" * 130 + "b" * 130, "aa") == [""] * 65 + ["b" * 130]
    assert len(split_fn(",x" * 300, ",")) == 301
    prof = sess.profile()
    assert prof["str_split_long_count"]["launches"] == prof["str_split_long_write"]["launches"] == len(lits)
    # per-row delimiters over long subjects
    dl = [[",", "ab", "aa", "x"][i % 4] for i in range(len(rows))]
    t2 = sess.table([("s", T_STRING, rows, None), ("d", T_STRING, dl, None)], nrows=len(rows))
    assert values(t2, Split(S, D)) == [split_fn(a, b) for a, b in zip(rows, dl)]


# --------------------------------------------------------------- GPU: interning
def _intern_tables(s):
    for x in ("p", "", ",", ";", "1"):  # in the dictionary before any split (the delimiter literals too)
        s.intern(x)
    a = s.table([("s", T_STRING, ["p,q1,r1", "q1,p", None, "r1,,new1", "solo", "q1"], None)])
    b = s.table([("s", T_STRING, ["new2;p", "p;new2;new3", "new3"], None)])
    return a, b


@pytest.mark.gpu
def test_interning(sess):
    a, b = _intern_tables(sess)
    before, _ = _dictionary(sess)
    n0 = len(before)
    code = {x: i for i, x in enumerate(before)}
    sess.reset_profile()
    out = a.withColumns((Split(S, StringLit(",")), "z"), header=H, params={})
    et, offs, vals, valid, ev = out.list_arrays("z")
    assert et == T_STRING and ev is None and valid.tolist() == [1, 1, 0, 1, 1, 1]
    pieces = [sess.lookup(int(c)) for c in vals]
    assert pieces == ["p", "q1", "r1", "q1", "p", "r1", "", "new1", "solo", "q1"]
    after, _ = _dictionary(sess)
    assert after[:n0] == before and len(set(after)) == len(after)
    # old strings keep their codes; new ones ascend by the first piece position producing them
    assert after[n0:] == ["r1", "new1"]
    assert [int(c) for c in vals] == [code["p"], code["q1"], n0, code["q1"], code["p"], n0, code[""], n0 + 1,
                                      code["solo"], code["q1"]]
    # the count pass's bytes: the subjects' bytes over the non-NULL rows + 41 per row
    prof = sess.profile()
    subj_bytes = sum(utf8_len(x) for x in ["p,q1,r1", "q1,p", "r1,,new1", "solo", "q1"])
    assert prof["str_split_count"]["bytes"] == subj_bytes + 41 * 6
    # a second split over the same table adds no string
    assert values(a, Split(S, StringLit(","))) == out.column_values("z")
    assert _dictionary(sess)[0] == after


@pytest.mark.gpu
def test_equal_sessions_end_with_equal_dictionaries():
    from capf_amd.table import GpuSession
    digests = []
    for _ in range(2):
        s = GpuSession(0)
        a, b = _intern_tables(s)
        values(a, Split(S, StringLit(",")))
        values(b, Split(S, StringLit(";")))
        values(a, Split(S, StringLit("1")))
        digests.append(_dictionary(s))
        s.close()
    assert digests[0] == digests[1]
    assert {"new2", "new3", "q", ",r", ",,new"} <= set(digests[0][0])


# -------------------------------------------------------------------- GPU: size
@pytest.mark.gpu
@pytest.mark.parametrize("n", [257, (1 << 20) + 3], ids=["257", "2^20+3"])
def test_size(gpu_session, n):
    """More than one block, and more than one sweep of the 4096 x 256 grid."""
    pool = [f"p{i},q{i % 3}" for i in range(7)] + ["p0,", ",q1", "solo"]
    want = [split_fn(x, ",") for x in pool]
    idx = np.arange(n) % len(pool)
    t = gpu_session.table([("s", T_STRING, [pool[i] for i in idx.tolist()], None)], nrows=n)
    out = t.withColumns((Split(S, StringLit(",")), "z"), header=H, params={})
    et, offs, vals, valid, ev = out.list_arrays("z")
    lens = np.array([len(w) for w in want], dtype=np.int64)[idx]
    assert et == T_STRING and valid.all() and ev is None
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum(lens)]))
    flat = np.array([gpu_session.intern(p) for w in want for p in w], dtype=np.int64)
    first = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    for i in list(range(0, n, max(1, n // 97))) + [n - 3, n - 2, n - 1]:
        k = int(idx[i])
        assert vals[offs[i]:offs[i + 1]].tolist() == flat[first[k]:first[k + 1]].tolist(), i
    # every row's first piece at once
    assert np.array_equal(vals[offs[:-1]], flat[first[:-1]][idx])


# ------------------------------------------------------------- GPU: composition
@pytest.mark.gpu
def test_composition(sess):
    """(A session of its own: toUpper of the lambda variable is a code map of
    the whole dictionary, which a dictionary grown past code maps refuses.)"""
    gpu_session = sess
    subj = ["p,q", "q", "", ",", "a,,b", None, "x,q,", "Q,q"]
    py = [None if x is None else x.split(",") for x in subj]
    t = gpu_session.table([("k", T_INT, list(range(len(subj))), None), ("s", T_STRING, subj, None)], nrows=len(subj))
    sp = Split(S, StringLit(","))
    assert values(t, Size(sp)) == [None if p is None else len(p) for p in py]
    assert values(t, ContainerIndex(sp, IntegerLit(1))) == [None if p is None or len(p) < 2 else p[1] for p in py]
    assert values(t, In(StringLit("q"), sp)) == [None if p is None else "q" in p for p in py]
    x = Var("x")
    comp = ListComprehension(x, Not(Equals(x, StringLit(""))), ToUpper(x), sp)
    assert values(t, comp) == [None if p is None else [e.upper() for e in p if e != ""] for p in py]
    # WHERE 'q' IN split(s, ',')
    f = t.filter(In(StringLit("q"), sp), header=H, params={})
    assert f.physicalColumns == t.physicalColumns
    assert f.column_values("k") == [i for i, p in enumerate(py) if p is not None and "q" in p]
    # WITH split(s, ',') AS xs UNWIND xs AS x
    w = t.withColumns((sp, "xs"), header=H, params={})
    u = w.withColumns((Explode(Var("xs")), "x"), header=H, params={})
    assert [(r["k"], r["x"]) for r in u.rows] == [(i, e) for i, p in enumerate(py) if p is not None for e in p]
    # literal x literal folds to a list literal; orderBy arguments are not hoisted
    assert values(t, Split(StringLit("1,2,3"), StringLit(",2,"))) == [["1", "3"]] * len(subj)
    assert values(t, Size(Split(StringLit("abc"), StringLit("")))) == [4] * len(subj)
    with pytest.raises(_lib.NotImplementedException):
        t.orderBy((sp, "asc"), header=H, params={}).size


# -------------------------------------------------------------- GPU: host route
@pytest.mark.gpu
def test_host_route(sess):
    subj = ["a|b", "a,b;c", "", "abc", None, "x.y", "|", "a1b22c"]
    t = sess.table([("s", T_STRING, subj, None)], nrows=len(subj))
    sess.reset_profile()
    for lit in ("|", "[,;]", "", ".", "[0-9]+"):
        assert values(t, Split(S, StringLit(lit))) == [split_fn(x, lit) for x in subj], lit
    assert split_launches(sess.profile()) == []
    # one non-plain value in a delimiter column: the host route for the whole column
    dl = [",", ",", ",", "", ",", None, "|", ","]
    t2 = sess.table([("s", T_STRING, subj, None), ("d", T_STRING, dl, None)], nrows=len(subj))
    out = t2.withColumns((Split(S, D), "z"), header=H, params={})
    assert out.column_values("z") == [split_fn(a, b) for a, b in zip(subj, dl)]
    assert out.list_elem_type("z") == T_STRING
    assert split_launches(sess.profile()) == []
    # the same column without its non-plain values: the device route
    dl3 = [d if d in (",", None) else ";" for d in dl]
    t3 = sess.table([("s", T_STRING, subj, None), ("d", T_STRING, dl3, None)], nrows=len(subj))
    assert values(t3, Split(S, D)) == [split_fn(a, b) for a, b in zip(subj, dl3)]
    assert split_launches(sess.profile()) == ["str_split_count", "str_split_write"]


# -------------------------------------------------------------------- GPU: C ABI
@pytest.mark.gpu
def test_c_abi_checks(gpu_session):
    t = gpu_session.table([("k", T_INT, [1, 2], None), ("s", T_STRING, ["a,b", "c"], None),
                           ("d", T_STRING, [",", ""], None)], nrows=2)
    with pytest.raises(_lib.IllegalArgumentException):  # when the node is built
        t._new("capf_table_str_split", t._h, b"k", b"d", b"z")
    with pytest.raises(_lib.IllegalArgumentException):
        t._new("capf_table_str_split", t._h, b"s", b"k", b"z")
    with pytest.raises(_lib.IllegalArgumentException):
        t._new("capf_table_str_split", t._h, b"s", b"d", b"s")  # the name is taken
    lazy = t._new("capf_table_str_split", t._h, b"s", b"d", b"z")  # an empty delimiter: when evaluated
    assert lazy.capf_type("z") == T_LIST and lazy.list_elem_type("z") == T_STRING
    with pytest.raises(_lib.IllegalArgumentException, match="empty delimiter"):
        lazy.column_values("z")
    ok = t.filter(Not(Equals(D, StringLit(""))), header=H, params={})
    assert ok._new("capf_table_str_split", ok._h, b"s", b"d", b"z").column_values("z") == [["a", "b"]]


# ------------------------------------------------------- GPU: reference cases
def rows_key(rows):
    return sorted(repr(sorted(r.items())) for r in rows)


@pytest.mark.gpu
@pytest.mark.parametrize("compact", [False, True], ids=["int64", "compact"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_case_on_gpu(gpu_session, case, compact):
    from capf_amd.graph import ScanGraph
    from capf_amd.planner import run
    from oracle.create_parser import parse_create
    cid, src, create, query, expected, opts = case_parts(case)
    got = run(ScanGraph.from_data(gpu_session, parse_create(create), compact=compact), query, opts.get("params"))
    assert rows_key(got) == rows_key(expected), f"{cid} ({src}): {got}"


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_reference_cases_through_jni():
    """Both cases with every C-ABI call routed through the JNI adapter
    (tests/jni_route.py), capf_table_str_split through Native.tableStrSplit."""
    import jni_route
    from capf_amd.graph import ScanGraph
    from capf_amd.planner import run
    from capf_amd.table import GpuSession
    from oracle.create_parser import parse_create
    jni_route.build()
    route = jni_route.JniRoute()
    calls = []

    def str_split(t, sc, dc, name, ref):
        calls.append(name)
        r = route.native("tableStrSplit", c_int64, (c_int64, t.value if isinstance(t, c_void_p) else (t or 0)),
                         route.jstr(sc), route.jstr(dc), route.jstr(name))
        ref._obj.value = r
        return route.done()

    route.install()
    _lib._FNS["capf_table_str_split"] = str_split
    try:
        for case in CASES:
            cid, src, create, query, expected, opts = case_parts(case)
            got = run(ScanGraph.from_data(GpuSession(0), parse_create(create)), query, opts.get("params"))
            assert rows_key(got) == rows_key(expected), f"{cid} ({src}): {got}"
        # the adapter's own argument check, and a C-ABI error rethrown by kind
        with pytest.raises(_lib.IllegalArgumentException, match="must not be null"):
            route.native("tableStrSplit", c_int64, (c_int64, 0), None, route.jstr(b"d"), route.jstr(b"z"))
        route.done()
        s = GpuSession(0)
        t = s.table([("k", T_INT, [1], None), ("s", T_STRING, ["a"], None)])
        with pytest.raises(_lib.IllegalArgumentException, match="not a STRING"):
            t._new("capf_table_str_split", t._h, b"k", b"s", b"z")
    finally:
        route.uninstall()
    assert len(calls) >= 2  # the variable-delimiter case (and the error case) went through the binding


# ------------------------------------------------------------ GPU: distributed
@pytest.mark.gpu
def test_distributed_layer_raises(sess):
    t = sess.table([("s", T_STRING, ["a,b"], None)])
    sess.value_map_gather = lambda rows: [rows]
    try:
        with pytest.raises(_lib.NotImplementedException, match="distributed"):
            values(t, Split(S, StringLit(",")))
    finally:
        del sess.value_map_gather
    assert values(t, Split(S, StringLit(","))) == [["a", "b"]]
