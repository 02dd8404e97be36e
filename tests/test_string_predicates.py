"""STARTS WITH / ENDS WITH / CONTAINS (okapi Expr.scala:369-379) on the device
string heap (CAPF_OP_STR_MATCH).

Flink's mapper raises NotImplemented for the three (FlinkSQLExprMapper.scala:
96-98) and the numpy oracle does not know them, so the expectations are the
reference suite's own (tests/golden/string_predicate_cases.py) and plain
Python — str.startswith / str.endswith / in — over the same host strings.

Two device paths answer the predicate and both are pinned here: a literal
pattern is matched once per dictionary string (a cached uint8 table the rows
look up by subject code; csrc/strings.hip), a column pattern — or a literal
one when the dictionary is larger than the input — row by row in the
interpreter.  CAPF_STR_MATCH=dict|rows forces one; the session profile tells
which kernels ran (str_match: the per-dictionary-string launch, its bytes =
the bytes of the strings it covered + 9 per string; str_contains_long: the
one-wave-per-long-subject launch of CONTAINS).
"""
import json
import os
import re
import shutil

import numpy as np
import pytest

from conftest import bag, case_parts, check_case
from string_predicate_cases import CASES

from capf_amd.expr import (OP_COL, OP_LIT_BOOL, OP_LIT_NULL, OP_LIT_STRING, OP_STR_MATCH, T_BOOL, T_INT, T_STRING,
                           Ands, BoolLit, CaseExpr, Contains, ElementProperty, EndsWith, Equals, IntegerLit, Not, NullLit,
                           Ors, Param, StartsWith, StringLit, Var, compile_program)
from capf_amd.header import RecordHeader

KINDS = [(StartsWith, 0, lambda s, p: s.startswith(p)), (EndsWith, 1, lambda s, p: s.endswith(p)),
         (Contains, 2, lambda s, p: p in s)]
KIND_IDS = ["starts_with", "ends_with", "contains"]
H = RecordHeader({Var("s"): "s", Var("p"): "p", Var("k"): "k"})
PAT_LDS_BYTES = 256  # csrc/strings.hip: the pattern staging area


def py_match(fn, s, p):
    return None if s is None or p is None else fn(s, p)


def utf8_len(s):
    return len(s.encode("utf-8"))


# ------------------------------------------------------------------ CPU
def _compile(e, types=None, params=None):
    types = types or {"s": T_STRING, "p": T_STRING, "k": T_INT}
    codes = {}
    return compile_program(e, H, set(types), params or {}, lambda x: codes.setdefault(x, 100 + len(codes)),
                           lambda c: types[c])


@pytest.mark.parametrize("cls,kind,fn", KINDS, ids=KIND_IDS)
def test_lowering_to_the_opcode(cls, kind, fn):
    """subject, pattern, CAPF_OP_STR_MATCH with the kind in iarg; a literal or
    parameter pattern is interned like any StringLit."""
    ops, ia, fa, names = _compile(cls(Var("s"), Var("p")))
    assert list(ops) == [OP_COL, OP_COL, OP_STR_MATCH] and ia[2] == kind
    assert [names[ia[0]], names[ia[1]]] == ["s", "p"]
    ops, ia, fa, names = _compile(cls(Var("s"), StringLit("ab")))
    assert list(ops) == [OP_COL, OP_LIT_STRING, OP_STR_MATCH] and ia[1] == 100 and ia[2] == kind
    ops, ia, fa, names = _compile(cls(Var("s"), Param("q")), params={"q": "ab"})
    assert list(ops) == [OP_COL, OP_LIT_STRING, OP_STR_MATCH] and ia[2] == kind
    ops, ia, fa, names = _compile(cls(StringLit("ab"), Var("p")))  # a literal subject, a column pattern
    assert list(ops) == [OP_LIT_STRING, OP_COL, OP_STR_MATCH]


@pytest.mark.parametrize("cls,kind,fn", KINDS, ids=KIND_IDS)
def test_folds(cls, kind, fn):
    """Two literals fold on the host; a NULL literal on either side, or an
    operand whose type is known and is not STRING, gives NULL of type BOOLEAN."""
    for s, p in [("foobar", "foo"), ("foobar", "bar"), ("foobar", "oba"), ("foo", ""), ("", "x"), ("a€b", "€b")]:
        ops, ia, fa, _ = _compile(cls(StringLit(s), StringLit(p)))
        assert (list(ops), list(ia)) == ([OP_LIT_BOOL], [1 if fn(s, p) else 0]), (s, p)
    null_bool = ([OP_LIT_NULL], [T_BOOL])
    for e in [cls(NullLit(), Var("p")), cls(Var("s"), NullLit()), cls(NullLit(), NullLit()),
              cls(StringLit("a"), NullLit()), cls(Var("s"), Param("q")),  # the parameter is NULL
              cls(Var("k"), Var("p")), cls(Var("s"), Var("k")), cls(Var("s"), IntegerLit(3)),
              cls(BoolLit(True), StringLit("t"))]:
        ops, ia, fa, _ = _compile(e, params={"q": None})
        assert (list(ops), list(ia)) == null_bool, str(e)
    # a column that holds only NULLs (typed NULL): NULL as well
    ops, ia, fa, _ = _compile(cls(Var("s"), Var("p")), types={"s": T_STRING, "p": 0, "k": T_INT})
    assert (list(ops), list(ia)) == null_bool


@pytest.mark.parametrize("cls,kind,fn", KINDS, ids=KIND_IDS)
def test_static_type_is_boolean(cls, kind, fn):
    """static_type gives BOOLEAN: a CASE over the predicate and a BOOLEAN types
    as BOOLEAN, and an ordering of the predicate against a STRING folds to NULL
    as incomparable (both decisions are static_type's)."""
    from capf_amd.expr import LessThan
    ops, ia, fa, _ = _compile(LessThan(cls(Var("s"), Var("p")), StringLit("x")))
    assert (list(ops), list(ia)) == ([OP_LIT_NULL], [T_BOOL])
    assert str(cls(Var("s"), StringLit("x"))) == f"(s {KIND_IDS[kind].upper().replace('_', ' ')} 'x')"


def test_scala_mapper_names_the_three_classes():
    """GpuExprMapper.scala lowers StartsWith / EndsWith / Contains (binary case
    classes of okapi-ir, tests/golden/okapi_api.json) to the same opcode."""
    import okapi_scala_scan as sc
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "okapi_api.json")) as f:
        api = json.load(f)
    srcs = sc.integration_sources()
    mapper, native = sc.strip_comments(srcs["GpuExprMapper.scala"]), sc.strip_comments(srcs["Native.scala"])
    assert ("org.opencypher.okapi.ir.api.expr", "_") in sc.imports(srcs["GpuExprMapper.scala"])
    for name, kind in (("StartsWith", "StartsWithKind"), ("EndsWith", "EndsWithKind"), ("Contains", "ContainsKind")):
        assert name in api["wildcard_packages"]["org.opencypher.okapi.ir.api.expr"]
        # matched by type, the operands read through the case class's lhs / rhs fields
        assert re.search(rf"case\s+(\w+):\s*{name}\s*=>\s*strMatch\(\1\.lhs,\s*\1\.rhs,\s*{kind}\)", mapper), name
    assert re.search(r"OpStrMatch\s*=\s*96\b", native) and "Native.OpStrMatch" in mapper
    for k, name in enumerate(("StrMatchStartsWith", "StrMatchEndsWith", "StrMatchContains")):
        assert re.search(rf"{name}\s*=\s*{k}\b", native) and f"Native.{name}" in mapper


# ------------------------------------------------------- GPU: reference cases
@pytest.mark.gpu
@pytest.mark.parametrize("compact", [False, True, 3], ids=["int64", "for32", "for24"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_case_on_gpu(gpu_session, case, compact):
    from capf_amd.graph import ScanGraph
    from capf_amd.planner import run
    from oracle.create_parser import parse_create
    cid, src, create, query, expected, opts = case_parts(case)
    g = ScanGraph.from_data(gpu_session, parse_create(create), compact=compact)
    got = run(g, query, opts.get("params"))
    assert check_case(got, expected, opts), f"{cid} ({src}): {got}"


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_reference_cases_through_jni():
    """The 12 cases through the JNI adapter (tests/jni_route.py): programs cross
    as op / iarg / farg arrays, no new native method."""
    import jni_route
    from capf_amd.graph import ScanGraph
    from capf_amd.planner import run
    from capf_amd.table import GpuSession
    from oracle.create_parser import parse_create
    jni_route.build()
    route = jni_route.JniRoute()
    bad = []
    for case in CASES:
        cid, src, create, query, expected, opts = case_parts(case)
        before = route.jni_calls
        route.install()
        try:
            got = run(ScanGraph.from_data(GpuSession(0), parse_create(create)), query, opts.get("params"))
        finally:
            route.uninstall()
        if not check_case(got, expected, opts) or route.jni_calls == before:
            bad.append((cid, got))
    assert not bad, bad


# ------------------------------------------------------------ GPU: edge table
LONG_PAT = "ab" * 150 + "c"  # 301 bytes: longer than the LDS staging area
SPECIAL = [
    "", "a", "b", "ab", "aab", "aaab", "abab", "abaabab", "ababab", "foobar", "foo", "bar", "barfoo", "foobarfoo",
    "xfoo", "foox", "fo", "oo",
    # 2-, 3- and 4-byte UTF-8
    "é", "aé", "éa", "€", "a€", "€a", "a€b", "\U0001F600", "x\U0001F600", "\U0001F600y", "x\U0001F600yz", "日本語", "本",
    # share trailing bytes with the characters above: ¬ = C2 AC against € = E2 82 AC, ؀ = D8 80 and 𐀀 = F0 90 80 80
    # against 😀 = F0 9F 98 80; © = C3 A9's neighbour C2 A9 against é
    "¬", "¬b", "؀", "\U00010000", "©", "a©", "\u0080", "\u0082¬",
    LONG_PAT, "z" + LONG_PAT, LONG_PAT + "z", "q" + LONG_PAT[:-1] + "d", LONG_PAT[1:], "ab" * 200,
]
LITERALS = ["", "a", "ab", "aab", "abab", "foo", "bar", "foobar", "é", "€", "€b", "\U0001F600", "本", "¬", "¬b",
            "؀", "\U00010000", "©", "\u0080", LONG_PAT, "ab" * 130, "zzzz-not-there"]
assert utf8_len(LONG_PAT) > PAT_LDS_BYTES and utf8_len("ab" * 130) > PAT_LDS_BYTES


def _edge_data(n=70001, seed=17):
    rng = np.random.default_rng(seed)
    alphabet = ["a", "b", "a", "b", "é", "€", "\U0001F600", "c"]
    filler = set()
    while len(filler) < 2400:  # random strings over a small alphabet: restarts and partial matches everywhere
        filler.add("".join(alphabet[i] for i in rng.integers(0, len(alphabet), int(rng.integers(1, 24)))))
    pool = SPECIAL + sorted(filler)
    piece = {}  # one piece per subject: from offset 0, up to the last byte, or inside
    for k, s in enumerate(pool):
        if s:
            a = 0 if k % 3 == 0 else int(rng.integers(0, len(s)))
            b = len(s) if k % 3 == 1 else int(rng.integers(a, len(s) + 1))
            piece[s] = s[a:b]
    subj = [pool[i] for i in rng.integers(0, len(pool), n)]
    pats = []
    for s in subj:
        r = rng.random()
        if r < 0.05:
            pats.append(None)
        elif r < 0.10:
            pats.append(s)  # equal to the subject
        elif r < 0.40 and s:
            pats.append(piece[s])
        elif r < 0.50:
            pats.append(s + "a")  # longer than the subject
        else:
            pats.append(LITERALS[int(rng.integers(0, len(LITERALS)))])
    for i in range(0, n, 13):
        subj[i] = None
    return subj, pats


@pytest.fixture(scope="module")
def edge():
    """(session, table, subjects, patterns): ~5,000 distinct strings in 70,001
    rows (274 blocks of 256 and a tail), on a session of its own (the tests
    read its profile)."""
    from capf_amd.table import GpuSession
    s = GpuSession(0)
    subj, pats = _edge_data()
    t = s.table([("s", T_STRING, subj, None), ("p", T_STRING, pats, None)])
    s.set_profiling(True)
    yield s, t, subj, pats
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["dict", "rows"])
@pytest.mark.parametrize("cls,kind,fn", KINDS, ids=KIND_IDS)
def test_edge_table_literal_patterns(edge, monkeypatch, cls, kind, fn, mode):
    """Every literal pattern as a withColumns value, row by row against Python,
    on the forced path (the profile shows the per-dictionary launch under dict
    and none under rows)."""
    s, t, subj, pats = edge
    distinct = len({x for x in subj + pats if x is not None} | set(LITERALS))
    assert 4000 <= distinct <= 7500 and len(subj) == 70001, distinct
    monkeypatch.setenv("CAPF_STR_MATCH", mode)
    s.reset_profile()
    out = t.withColumns(*[(cls(Var("s"), StringLit(p)), f"x{i}") for i, p in enumerate(LITERALS)],
                        header=H, params={})
    bad = []
    for i, p in enumerate(LITERALS):
        got = out.column_values(f"x{i}")
        want = [py_match(fn, x, p) for x in subj]
        if got != want:
            j = next(j for j, (a, b) in enumerate(zip(got, want)) if a != b)
            bad.append((p[:20], j, subj[j][:40], got[j], want[j]))
    assert not bad, bad[:5]
    # one per-dictionary launch per pattern of this kind (each new to the session), or none
    launches = s.profile().get("str_match", {"launches": 0})["launches"]
    assert launches == (len(LITERALS) if mode == "dict" else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["dict", "rows"])
@pytest.mark.parametrize("cls,kind,fn", KINDS, ids=KIND_IDS)
def test_edge_table_column_pattern(edge, monkeypatch, cls, kind, fn, mode):
    """A column pattern (NULL subjects and NULL patterns, the pattern equal to
    the subject, a piece of it, longer than it) runs row by row whatever the
    forced path; as a value and as a filter."""
    s, t, subj, pats = edge
    monkeypatch.setenv("CAPF_STR_MATCH", mode)
    s.reset_profile()
    e = cls(Var("s"), Var("p"))
    got = t.withColumns((e, "x"), header=H, params={}).column_values("x")
    want = [py_match(fn, a, b) for a, b in zip(subj, pats)]
    assert got == want, next((j, subj[j], pats[j], a, b) for j, (a, b) in enumerate(zip(got, want)) if a != b)
    assert want.count(True) > 5000 and want.count(False) > 5000 and want.count(None) > 5000
    kept = t.filter(e, H, {})
    assert kept.size == want.count(True)
    assert kept.column_values("s") == [a for a, w in zip(subj, want) if w]
    assert "str_match" not in s.profile()


# ------------------------------------------------------------------ GPU: tiers
def _tier_subjects(L, needle):
    """Subjects of L − 1, L, L + 1 and 4 L + 3 bytes (and two that reach past a
    wave's 64 start positions whatever L): the only occurrence of the needle in
    the last bytes, starting at position 63 / 64 or 255 / 256, at 0, or nowhere (a needle
    missing its last byte is there instead)."""
    out = []
    k = len(needle)
    near = needle[:-1]
    for n in sorted({L - 1, L, L + 1, 4 * L + 3, 64 + k + 3, 131}):
        if n < k:
            out.append("x" * n)
            continue
        out.append("x" * n)  # nowhere
        out.append(near + "x" * (n - len(near)))  # nowhere, a near miss at 0
        out.append("x" * (n - len(near)) + near)  # nowhere, a near miss at the end
        out.append("x" * (n - k) + needle)  # in the last plen bytes
        out.append(needle + "x" * (n - k))  # at offset 0 only
        for pos in (63, 64, 255, 256):  # a lane-stride boundary, and the boundary between two ballots
            if pos + k <= n:
                out.append("x" * pos + needle + "y" * (n - pos - k))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("L", [8, None], ids=["long8", "default"])
def test_contains_tiers(monkeypatch, L):
    """CONTAINS across the thread tier / wave tier threshold (CAPF_STR_LONG=8
    and the default 256): subjects around the threshold and past a wave's
    lane stride, against Python; the wave tier's launch ran.  Then a dictionary
    of short strings only: the worklist is empty and the second launch skipped."""
    from capf_amd.table import GpuSession
    if L is not None:
        monkeypatch.setenv("CAPF_STR_LONG", str(L))
    else:
        monkeypatch.delenv("CAPF_STR_LONG", raising=False)
    monkeypatch.setenv("CAPF_STR_MATCH", "dict")
    thr = L or 256
    for needle in ("abcab", "ab", "abcabcabd"):
        s = GpuSession(0)
        try:
            s.set_profiling(True)
            subj = _tier_subjects(thr, needle) + ["", needle, needle[1:]]
            assert {utf8_len(x) for x in subj} >= {thr - 1, thr, thr + 1, 4 * thr + 3}
            t = s.table([("s", T_STRING, subj, None)])
            got = t.withColumns((Contains(Var("s"), StringLit(needle)), "x"), header=H, params={}).column_values("x")
            want = [needle in x for x in subj]
            assert got == want, [(len(a), w) for a, g, w in zip(subj, got, want) if g != w]
            assert True in want and False in want
            prof = s.profile()
            assert prof["str_match"]["launches"] == 1 and prof["str_contains_long"]["launches"] == 1
        finally:
            s.close()
    s = GpuSession(0)
    try:
        s.set_profiling(True)
        subj = ["x" * n + "abcab"[: n % 6] for n in range(thr - len("abcab"))] + ["abcab"]
        assert max(utf8_len(x) for x in subj) < thr
        t = s.table([("s", T_STRING, subj, None)])
        got = t.withColumns((Contains(Var("s"), StringLit("abcab")), "x"), header=H, params={}).column_values("x")
        assert got == ["abcab" in x for x in subj]
        prof = s.profile()
        assert prof["str_match"]["launches"] == 1 and "str_contains_long" not in prof
    finally:
        s.close()


# ----------------------------------------------------------------- GPU: growth
def _dictionary(s):
    """The session dictionary's strings by code."""
    from ctypes import byref, c_int64, c_uint64
    from capf_amd import _lib
    cnt, dig = c_int64(), c_uint64()
    _lib.call("capf_string_digest", s._h, byref(cnt), byref(dig))
    return [s.lookup(c) for c in range(cnt.value)]


@pytest.mark.gpu
def test_dictionary_growth_extends_table_and_heap(monkeypatch):
    """Filter, intern new strings through a second table (matching and not),
    filter again with the same literal: the cached table is extended over the
    new codes only (the launch's profiled bytes are exactly theirs) from the
    appended heap; a table created — and a filter planned — before the growth
    still answer correctly.  With neither path forced, a one-row table over
    the grown dictionary takes the per-row path for a new pattern (the
    dictionary path would examine more strings than there are rows)."""
    from capf_amd.table import GpuSession
    monkeypatch.delenv("CAPF_STR_MATCH", raising=False)
    s = GpuSession(0)
    try:
        s.set_profiling(True)
        first = ["alphabet", "crab", "cab", "", "b", "a", "tabby", "€ab", "a€b", None] * 7
        pred = Contains(Var("s"), StringLit("ab"))
        t1 = s.table([("s", T_STRING, first, None)])
        want1 = [x for x in first if x is not None and "ab" in x]
        assert t1.filter(pred, H, {}).column_values("s") == want1
        d1 = _dictionary(s)
        assert set(d1) >= {x for x in first if x is not None} | {"ab"}
        prof = s.profile()["str_match"]
        assert prof["launches"] == 1 and prof["bytes"] == 9 * len(d1) + sum(utf8_len(x) for x in d1)
        assert t1.filter(pred, H, {}).column_values("s") == want1  # cached: no launch
        assert s.profile()["str_match"]["launches"] == 1
        early = t1.filter(pred, H, {})  # planned now, evaluated after the growth
        # growth: far more new bytes than the heap's first capacity, so both buffers are reallocated
        new = [f"{'ab' if i % 3 == 0 else 'ba-'}{i:05d}{'x' * (i % 97)}" for i in range(3000)] + ["grab", "no", "y" * 70000 + "ab"]
        t2 = s.table([("s", T_STRING, new + [None], None)])
        s.reset_profile()
        assert t2.filter(pred, H, {}).column_values("s") == [x for x in new if "ab" in x]
        d2 = _dictionary(s)[len(d1):]  # the strings interned since: the launch covered exactly these
        assert set(d2) >= set(new)
        prof = s.profile()["str_match"]
        assert prof["launches"] == 1 and prof["bytes"] == 9 * len(d2) + sum(utf8_len(x) for x in d2)
        assert s.profile()["str_contains_long"]["launches"] == 1  # the 70,002-byte string
        assert t1.filter(pred, H, {}).column_values("s") == want1
        assert early.column_values("s") == want1
        assert t1.filter(StartsWith(Var("s"), StringLit("a")), H, {}).column_values("s") == \
            [x for x in first if x is not None and x.startswith("a")]
        # the rule: 1 row, > 3000 strings not covered by a table for this new pattern → row by row
        s.reset_profile()
        one = s.table([("s", T_STRING, ["grab"], None)])
        assert one.withColumns((EndsWith(Var("s"), StringLit("rab")), "x"), header=H, params={}).column_values("x") == [True]
        assert "str_match" not in s.profile()
        # ... and the dictionary path once the rows are at least the strings not covered
        many = s.table([("s", T_STRING, ["grab", "crab", "no"] * 1200, None)])
        assert many.withColumns((EndsWith(Var("s"), StringLit("rab")), "x"), header=H,
                                params={}).column_values("x") == [True, True, False] * 1200
        assert s.profile()["str_match"]["launches"] == 1
    finally:
        s.close()


# ------------------------------------------------------------ GPU: composition
def _not3(a):
    return None if a is None else not a


def _and3(*xs):
    return False if any(x is False for x in xs) else None if any(x is None for x in xs) else True


def _or3(*xs):
    return True if any(x is True for x in xs) else None if any(x is None for x in xs) else False


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["dict", "rows"])
def test_composition_three_valued(gpu_session, monkeypatch, mode):
    """The predicate inside NOT, AND and OR (3-valued), inside CASE, as a
    filter and as a withColumns value."""
    monkeypatch.setenv("CAPF_STR_MATCH", mode)
    subj = ["foobar", "barfoo", "foo", "bar", "", None, "foofoo", "xbarx"] * 5
    pats = ["foo", None, "o", "bar", "", "x", "foofoo", "rx", "ba", "b"] * 4
    ks = list(range(40))
    t = gpu_session.table([("s", T_STRING, subj, None), ("p", T_STRING, pats, None), ("k", T_INT, ks, None)])
    sw = [py_match(str.startswith, a, "foo") for a in subj]
    ew = [py_match(str.endswith, a, b) for a, b in zip(subj, pats)]
    ct = [py_match(lambda a, b: b in a, a, "bar") for a in subj]
    e_sw, e_ew, e_ct = StartsWith(Var("s"), StringLit("foo")), EndsWith(Var("s"), Var("p")), \
        Contains(Var("s"), StringLit("bar"))
    exprs = {
        "n": (Not(e_sw), [_not3(a) for a in sw]),
        "a": (Ands(e_sw, e_ew), [_and3(a, b) for a, b in zip(sw, ew)]),
        "o": (Ors(e_ct, e_ew, Not(e_sw)), [_or3(c, b, _not3(a)) for a, b, c in zip(sw, ew, ct)]),
        "c": (CaseExpr([(e_ct, IntegerLit(1)), (e_ew, IntegerLit(2))], IntegerLit(0)),
              [1 if c else 2 if b else 0 for b, c in zip(ew, ct)]),
        "q": (Equals(e_sw, e_ct), [None if a is None or c is None else a == c for a, c in zip(sw, ct)]),
    }
    out = t.withColumns(*[(e, name) for name, (e, _) in exprs.items()], header=H, params={})
    for name, (e, want) in exprs.items():
        assert out.column_values(name) == want, (name, str(e))
    for e, want in [(Ands(e_ct, Not(e_sw)), [_and3(c, _not3(a)) for a, c in zip(sw, ct)]),
                    (Ors(e_ew, e_sw), [_or3(b, a) for a, b in zip(sw, ew)]), (Not(e_ew), [_not3(b) for b in ew])]:
        assert t.filter(e, H, {}).column_values("k") == [k for k, w in zip(ks, want) if w is True], str(e)


@pytest.mark.gpu
def test_where_ends_with_through_the_planner(gpu_session):
    """MATCH (n) WHERE n.name ENDS WITH 'e' RETURN n.name on the ACTORS graph
    (nodes without a name drop out: NULL is not TRUE)."""
    from expression_cases import ACTORS
    from capf_amd.graph import ScanGraph
    from capf_amd.planner import Match, NodeP, Query, Stage, run
    from oracle.create_parser import parse_create
    name = ElementProperty(Var("n", "NODE"), "name")
    q = Query([Match([NodeP("n")], where=[EndsWith(name, StringLit("e"))])], [Stage([("n.name", name)])])
    got = run(ScanGraph.from_data(gpu_session, parse_create(ACTORS)), q)
    names = re.findall(r"\{name: '([^']*)'", ACTORS)
    assert len(names) == 8
    want = [{"n.name": x} for x in names if x.endswith("e")]
    assert len(want) == 3 and bag(got) == bag(want)
