"""toUpper / toLower / trim / lTrim / rTrim / substring / replace / s + 'lit' /
'lit' + s evaluated on the device string heap and interned there
(capf_string_fn_codes, csrc/string_fn.hip).

The reference is expr.string_fn — the JVM semantics Flink's lowering gives the
functions (FlinkSQLExprMapper.scala:187-195) — applied row by row in Python.
CAPF_STR_FN=device|host forces a route; the session profile tells which
kernels ran: str_fn_len (the length pass, its bytes = the source strings'
bytes + 25 per source: one offset read, status + length + start written),
str_fn_long_len / str_fn_long (the one-wave-per-long-string launches),
str_idx_build / str_idx_extend (the dictionary's hash index).
"""
import os
import re
import shutil
import socket
from ctypes import byref, c_int64, c_uint64

import numpy as np
import pytest

from capf_amd import _lib
from capf_amd.expr import (OP_COL, OP_STR_MAP, T_INT, T_STRING, Add, IntegerLit, LTrim, Replace, RTrim, StringLit,
                           Substring, ToLower, ToString, ToUpper, Trim, Var, compile_program, device_string_fn,
                           plain_replace_literal, string_fn)
from capf_amd.header import RecordHeader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = RecordHeader({Var("s"): "s", Var("k"): "k"})
S = Var("s")

UNARY = [(ToUpper(S), ("upper",)), (ToLower(S), ("lower",)), (Trim(S), ("trim",)), (LTrim(S), ("ltrim",)),
         (RTrim(S), ("rtrim",))]
PAST_END = 100000
# `from` as string_fn receives it (1-based; Cypher's start is one less), `len`
SUBSTRINGS = [(Substring(S, IntegerLit(f - 1), IntegerLit(n)), ("substring", f, n))
              for f in (1, 2, 0, -1, -3, PAST_END) for n in (0, 1, 3, 1 << 40)]
LIT301 = "ab" * 150 + "c"
CONCATS = [(e, k) for lit in ("", "x", "€", LIT301)
           for e, k in ((Add(S, StringLit(lit)), ("concat_r", lit)), (Add(StringLit(lit), S), ("concat_l", lit)))]
REPLACES = [(Replace(S, StringLit(a), StringLit(b)), ("replace", a, b))
            for a, b in (("ab", "x"), ("ab", "abab"), ("a", ""), ("aa", "a"), ("€", "e"))]
HOST_REPLACES = [(Replace(S, StringLit("a.b"), StringLit("-")), ("replace", "a.b", "-"))]
FAMILIES = {"unary": UNARY, "substring": SUBSTRINGS, "concat": CONCATS, "replace": REPLACES + HOST_REPLACES}


@pytest.fixture(autouse=True)
def _no_programs_from_other_sessions(monkeypatch):
    """compile_program's memo is shared by all sessions: a program memoised for
    another session asks this one for its map, finds another name, and the
    recompilation asks again — after the first answer's results entered the
    dictionary, so the map is extended over them.  The tests below count
    launches and host calls: each starts with an empty memo."""
    import capf_amd.expr as ex
    monkeypatch.setattr(ex, "_PROGRAM_MEMO", {})


def utf8_len(s):
    return len(s.encode("utf-8", "surrogatepass"))


def _dictionary(s):
    """The session dictionary's strings by code, and its digest."""
    cnt, dig = c_int64(), c_uint64()
    _lib.call("capf_string_digest", s._h, byref(cnt), byref(dig))
    return [s.lookup(c) for c in range(cnt.value)], dig.value


def _want(key, subj, fn=string_fn):
    memo = {}
    return [None if x is None else memo[x] if x in memo else memo.setdefault(x, fn(key, x)) for x in subj]


def _check(t, subj, family, fn=string_fn):
    out = t.withColumns(*[(e, f"x{i}") for i, (e, _) in enumerate(family)], header=H, params={})
    bad = []
    for i, (e, key) in enumerate(family):
        got, want = out.column_values(f"x{i}"), _want(key, subj, fn)
        if got != want:
            j = next(j for j, (a, b) in enumerate(zip(got, want)) if a != b)
            bad.append((str(e)[:60], j, subj[j][:40], len(subj[j]), str(got[j])[:40], str(want[j])[:40]))
    assert not bad, bad[:5]


# ------------------------------------------------------------------ CPU
def test_plain_literal_classifier():
    """replace's search literal goes to the device only when it is non-empty
    and free of every Java regex metacharacter."""
    for ch in "\\^$.|?*+()[]{}":
        assert not plain_replace_literal(ch) and not plain_replace_literal("a" + ch + "b"), ch
    assert not plain_replace_literal("")
    for ok in ("a", "ab", "hello world", "a-b", "a,b;c", "€", "日本語", "x\U0001F600", "é#~&", "a b"):
        assert plain_replace_literal(ok), ok
    codes = {}
    intern = lambda x: codes.setdefault(x, 100 + len(codes))  # noqa: E731
    assert device_string_fn(("replace", "a.b", "x"), intern) is None and not codes
    assert device_string_fn(("regex", "ab"), intern) is None
    assert device_string_fn(("replace", "ab", "x"), intern) == (8, 0, 0, 100, 101)
    assert device_string_fn(("concat_l", "x"), intern) == (6, 0, 0, 101, -1)
    assert device_string_fn(("substring", -3, 2), intern) == (5, -3, 2, -1, -1)
    assert device_string_fn(("substring", 1, -1), intern) is None
    assert [device_string_fn((k,), intern)[0] for k in ("upper", "lower", "trim", "ltrim", "rtrim")] == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("e,key", UNARY + SUBSTRINGS[:2] + CONCATS[:4] + REPLACES[:1] + HOST_REPLACES,
                         ids=lambda v: str(v)[:40])
def test_lowering_is_unchanged(e, key):
    """Every function still lowers to its operand and CAPF_OP_STR_MAP naming
    the code map the session gives for the same key."""
    asked = []
    ops, ia, fa, names = compile_program(e, H, {"s", "k"}, {}, lambda x: 7, lambda c: T_STRING, None,
                                         lambda k: asked.append(k) or "\x01map:5", None)
    if key == ("concat_r", "") or key == ("concat_l", ""):
        assert asked in ([], [key])  # s + '' may fold to s
    else:
        assert asked == [key]
    if asked:
        assert list(ops) == [OP_COL, OP_STR_MAP] and [names[ia[0]], names[ia[1]]] == ["s", "\x01map:5"]


def test_scala_session_calls_the_native_method():
    """GpuCypherSession.stringMap fills its code map through
    Native.stringFnCodes (declared @native, the StrFn* ids equal to
    CAPF_STR_FN_*), GpuStringFunctions left for the strings answered
    StrFnOnHost and the classifier's twin deciding replace's route."""
    import okapi_scala_scan as sc
    from capf_amd.expr import STR_FN_IDS
    srcs = sc.integration_sources()
    session, native, fns = (sc.strip_comments(srcs[f]) for f in
                            ("GpuCypherSession.scala", "Native.scala", "GpuStringFunctions.scala"))
    assert re.search(r"@native\s+def\s+stringFnCodes\(session:\s*Long,\s*fn:\s*Int,\s*iarg0:\s*Long,\s*iarg1:\s*Long,"
                     r"\s*lit0:\s*Long,\s*lit1:\s*Long,\s*src:\s*ByteBuffer,\s*c0:\s*Long,\s*n:\s*Long,"
                     r"\s*out:\s*ByteBuffer\):\s*Unit", native)
    header = open(os.path.join(ROOT, "include", "capf_gpu.h")).read()
    for (name, scala) in (("upper", "StrFnUpper"), ("lower", "StrFnLower"), ("trim", "StrFnTrim"),
                          ("ltrim", "StrFnLTrim"), ("rtrim", "StrFnRTrim"), ("substring", "StrFnSubstring"),
                          ("concat_l", "StrFnConcatL"), ("concat_r", "StrFnConcatR"), ("replace", "StrFnReplace")):
        k = STR_FN_IDS[name]
        assert re.search(rf"{scala}\s*=\s*{k}\b", native) and f"Native.{scala}" in session, name
        assert re.search(rf"CAPF_STR_FN_{name.upper()}\s*=\s*{k}\b", header), name
    assert re.search(r"StrFnOnHost\s*=\s*-2L", native) and "Native.StrFnOnHost" in session
    assert re.search(r"Native\.stringFnCodes\(handle,", session)
    assert "GpuStringFunctions.plainReplaceLiteral(" in session and "def plainReplaceLiteral(" in fns
    body = session[session.index("def stringMap("):]
    assert "stringFnCodes(key," in body and "Native.sessionCodeMapExtend(" in body


# ------------------------------------------------------------ GPU: edge table
def _tier_strings(L):
    """Strings of L − 1, L, L + 1 and 4 L + 3 bytes: plain, upper-case, spaces at
    both ends, multi-byte, with 'ab' inside, and with a 4-byte character."""
    out = []
    for n in sorted({L - 1, L, L + 1, 4 * L + 3}):
        out += ["x" * n, "X" * n, "xY" * (n // 2) + "z" * (n % 2), " " * 3 + "q" * (n - 5) + " " * 2,
                " " * (n - 1) + "w", "w" + " " * (n - 1), " " * n, "ab" * (n // 2) + "c" * (n % 2),
                "é" * (n // 2) + "e" * (n % 2), "€" * (n // 3) + "u" * (n % 3),
                "x" * (n - 4) + "\U0001F600" if n >= 4 else "y" * n]
    return out


def _boundary_strings():
    """Spaces, and substring's cut (`from` −3 or −1 counted from the end, or 2
    from the start), at bytes 63 / 64 and 255 / 256."""
    out = []
    for pos in (63, 64, 65, 255, 256, 257):
        out += [" " * pos + "t" * 9, "t" * 9 + " " * pos, " " * pos + "Tt" + " " * pos,  # trim's bounds
                "c" * (pos + 3), "c" * (pos + 1), "é" * (pos // 2) + "c" * (pos % 2) + "xyz",  # the cut from the end
                "€" + "c" * pos, "é" * ((pos - 1) // 2) + "€xy"]
    return out


SPECIAL = ["", " ", "   ", " a ", "a b", "  lead", "trail  ", " both ", "MiXeD Case", "UPPER", "lower", "UPPER 123 !",
           "lower 123 !", "z", "Z", "@[`{", "ab", "abab", "aaaa", "aaaaa", "xabx", "a.b", "aXb", "ba", "aab", "€", "€€",
           "a€b", " é ", "é", "É", "straße", " € ", "€uro", " \U0001F600 ", "x\U0001F600y", "\U0001F600", "日本語",
           " 日本 ", "\ud800", " \ud800x ", "a\udfffb", "ß", "ǆ", "ŉ"]


def _edge_data(n=70001, seed=23):
    rng = np.random.default_rng(seed)
    alphabet = list("abABxyZ  ") + ["é", "€", "a", "b"]
    filler = set()
    while len(filler) < 4600:
        filler.add("".join(alphabet[i] for i in rng.integers(0, len(alphabet), int(rng.integers(1, 30)))))
    pool = SPECIAL + _tier_strings(8) + _tier_strings(256) + _boundary_strings() + sorted(filler)
    pool = list(dict.fromkeys(pool))
    subj = [pool[i] for i in rng.integers(0, len(pool), n)]
    subj[:len(pool)] = pool  # every string is there
    for i in range(5, n, 13):
        subj[i] = None
    return pool, subj


@pytest.fixture(scope="module", params=[("device", None), ("device", 8), ("host", None)],
                ids=["device", "device-long8", "host"])
def edge(request):
    """(session, table, subjects, route, CAPF_STR_LONG): ~5,000 distinct strings
    in 70,001 rows (274 blocks of 256 and a tail), a session per route (a
    function's code map is cached per session) with profiling on."""
    from capf_amd.table import GpuSession
    mode, L = request.param
    s = GpuSession(0)
    pool, subj = _edge_data()
    assert 4500 <= len(pool) <= 5500 and len(subj) == 70001
    assert {utf8_len(x) for x in pool} >= {7, 8, 9, 35, 255, 256, 257, 1027}
    t = s.table([("s", T_STRING, subj, None)])
    s.set_profiling(True)
    yield s, t, subj, mode, L
    s.close()


def _route(monkeypatch, mode, L):
    monkeypatch.setenv("CAPF_STR_FN", mode)
    if L is None:
        monkeypatch.delenv("CAPF_STR_LONG", raising=False)
    else:
        monkeypatch.setenv("CAPF_STR_LONG", str(L))


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_edge_table_against_string_fn(edge, monkeypatch, family):
    """Every function and argument over the edge table, row by row against
    expr.string_fn, on the forced route; the device route launches the length
    pass (and, for the functions that have one, the wave tier), the host route
    launches neither."""
    s, t, subj, mode, L = edge
    _route(monkeypatch, mode, L)
    s.reset_profile()
    _check(t, subj, FAMILIES[family])
    prof = s.profile()
    if mode == "host":
        assert not [k for k in prof if k.startswith(("str_fn", "str_idx"))], sorted(prof)
        return
    assert prof["str_fn_len"]["launches"] >= len(FAMILIES[family]) - 2  # (s + '' may fold; one replace is the host's)
    assert prof["str_fn_write"]["launches"] == prof["str_fn_len"]["launches"]
    if family in ("unary", "substring"):
        assert prof["str_fn_long_len"]["launches"] >= 1 and prof["str_fn_long"]["launches"] >= 1
    elif family == "concat":
        assert "str_fn_long_len" not in prof and prof["str_fn_long"]["launches"] >= 1
    else:  # a long subject is the host's: no wave tier
        assert "str_fn_long_len" not in prof and "str_fn_long" not in prof


@pytest.mark.gpu
def test_edge_dictionary_has_no_duplicates(edge):
    """After every function has run (the tests above), no string is in the
    dictionary twice."""
    s = edge[0]
    d, _ = _dictionary(s)
    assert len(set(d)) == len(d), [x for x in set(d) if d.count(x) > 1][:5]


# ------------------------------------------------------- GPU: the host status
ASCII_POOL = ["", " ", " a ", "Hello World", "UPPER", "lower", "  x", "y  ", "abab", "aaaa", "a.b", "q" * 255,
              "Ab" * 200, " " * 300 + "k" + " " * 300, "M" * 1027] + [f"Row {i:04d} ab{'a' * (i % 7)} " for i in range(500)]


@pytest.mark.gpu
def test_ascii_dictionary_never_reaches_the_host(monkeypatch):
    """An all-ASCII dictionary: with expr.string_fn raising, every function but
    the host-routed replaces (a regex search literal; 'ab' in a subject of 256
    bytes or more) still gives the right rows."""
    import capf_amd.expr as ex
    from capf_amd.table import GpuSession
    _route(monkeypatch, "device", None)

    def boom(key, sv):
        raise AssertionError(f"string_fn{key} evaluated on the host for {sv[:30]!r}")
    monkeypatch.setattr(ex, "string_fn", boom)
    s = GpuSession(0)
    try:
        subj = [ASCII_POOL[i % len(ASCII_POOL)] for i in range(3001)] + [None]
        t = s.table([("s", T_STRING, subj, None)])
        for family in (UNARY, SUBSTRINGS, CONCATS):
            _check(t, subj, family)
        # (a code map covers the whole dictionary: the short subjects get a session of their own)
        s2 = GpuSession(0)
        try:
            short = [x if x is None or len(x) < 256 else x[:200] for x in subj]
            _check(s2.table([("s", T_STRING, short, None)]), short, REPLACES)
        finally:
            s2.close()
        with pytest.raises(AssertionError, match="on the host"):  # the literal is a regex
            t.withColumns((HOST_REPLACES[0][0], "x"), header=H, params={}).column_values("x")
        with pytest.raises(AssertionError, match="on the host"):  # "Ab" * 200: a long subject
            t.withColumns((REPLACES[0][0], "x"), header=H, params={}).column_values("x")
    finally:
        s.close()


@pytest.mark.gpu
def test_to_upper_calls_the_host_once_per_non_ascii_string(monkeypatch):
    """k strings with a byte ≥ 0x80 in the dictionary: toUpper evaluates exactly
    those on the host (ß → SS is not bytewise), substring exactly the strings
    holding a supplementary character."""
    import capf_amd.expr as ex
    from capf_amd.table import GpuSession
    _route(monkeypatch, "device", None)
    calls = []

    def counting(key, sv):
        calls.append((key, sv))
        return string_fn(key, sv)
    monkeypatch.setattr(ex, "string_fn", counting)
    non_ascii = ["straße", "é", " € ", "x\U0001F600y", "\ud800", "日本語", "e" * 300 + "é", "\U00010000" * 70]
    s = GpuSession(0)
    try:
        subj = ASCII_POOL[:100] + non_ascii
        t = s.table([("s", T_STRING, subj, None)])
        _check(t, subj, UNARY[:1])
        assert sorted(sv for _, sv in calls) == sorted(non_ascii) and {k for k, _ in calls} == {("upper",)}
        del calls[:]
        before, _ = _dictionary(s)  # (toUpper's results included: the map covers the whole dictionary)
        _check(t, subj, [SUBSTRINGS[6]])  # from 2, len 3
        supplementary = sorted(x for x in before if any(ord(c) > 0xFFFF for c in x))
        assert len(supplementary) >= 2 and sorted(sv for _, sv in calls) == supplementary
    finally:
        s.close()


# ------------------------------------------------------------ GPU: interning
@pytest.mark.gpu
def test_results_take_existing_codes_and_new_ones_once(monkeypatch):
    from capf_amd.table import GpuSession
    _route(monkeypatch, "device", None)
    s = GpuSession(0)
    try:
        words = ["ab", "Ab", "aB", "AB", " ab", "ab "]
        t = s.table([("s", T_STRING, words * 3, None)])
        assert _dictionary(s)[0] == words
        up = s.string_fn_codes(("upper",), s._device_fn_args(("upper",)), None, 0, 6)
        # "AB" is code 3 (itself: identity); the two new strings ascend in worklist order
        assert up.tolist() == [3, 3, 3, 3, 6, 7] and _dictionary(s)[0][6:] == [" AB", "AB "]
        tr = s.string_fn_codes(("trim",), s._device_fn_args(("trim",)), np.array([5, 4, -1, 7, 6, 0]), 0, 6)
        assert tr.tolist() == [0, 0, -1, 3, 3, 0] and len(_dictionary(s)[0]) == 8  # nothing new
        for fam in (UNARY, CONCATS[:4], REPLACES, SUBSTRINGS[4:12]):
            _check(t, words * 3, fam)
        d, _ = _dictionary(s)
        assert len(set(d)) == len(d)
        with pytest.raises(_lib.IllegalArgumentException):
            s.string_fn_codes(("upper",), (9, 0, 0, -1, -1), None, 0, 1)
        with pytest.raises(_lib.IllegalArgumentException):
            s.string_fn_codes(("upper",), (0, 0, 0, -1, -1), None, 0, len(d) + 1)
        with pytest.raises(_lib.IllegalArgumentException):
            s.string_fn_codes(("upper",), (0, 0, 0, -1, -1), np.array([len(d)]), 0, 1)
        with pytest.raises(_lib.IllegalArgumentException):
            s.string_fn_codes(("substring", 1, -1), (5, 1, -1, -1, -1), None, 0, 1)
    finally:
        s.close()


@pytest.mark.gpu
def test_two_sessions_end_with_identical_dictionaries(monkeypatch):
    """Code assignment is deterministic: the same inputs give the same
    dictionary, order included, whatever order the threads ran in."""
    from capf_amd.table import GpuSession
    _route(monkeypatch, "device", None)
    pool, subj = _edge_data(n=20001)
    ends = []
    for _ in range(2):
        s = GpuSession(0)
        try:
            t = s.table([("s", T_STRING, subj, None)])
            out = t.withColumns(*[(e, f"x{i}") for i, (e, _) in
                                  enumerate(UNARY + SUBSTRINGS[5:8] + CONCATS[2:4] + REPLACES[:3])], header=H, params={})
            out.size
            ends.append(_dictionary(s))
        finally:
            s.close()
    assert ends[0][1] == ends[1][1] and ends[0][0] == ends[1][0]
    assert len(ends[0][0]) > 2 * len(pool)


@pytest.mark.gpu
def test_many_equal_results_give_one_code_each(monkeypatch):
    """3,000 results that are one of three strings: three new codes, ascending
    in the order of each string's first source."""
    from capf_amd.table import GpuSession
    _route(monkeypatch, "device", None)
    s = GpuSession(0)
    try:
        subj = [f"{'qpr'[i * 7 % 3]}-{i:05d}" for i in range(3000)]
        assert [x[0] for x in subj[:3]] == ["q", "p", "r"]
        t = s.table([("s", T_STRING, subj, None)])
        n0 = len(_dictionary(s)[0])
        _check(t, subj, [(Substring(S, IntegerLit(0), IntegerLit(1)), ("substring", 1, 1))])
        assert _dictionary(s)[0][n0:] == ["q", "p", "r"]
    finally:
        s.close()


# ----------------------------------------------------------------- GPU: growth
@pytest.mark.gpu
def test_dictionary_growth_extends_the_map_the_heap_and_the_index(monkeypatch):
    """toUpper, 3,000 more strings (one of 70,000 bytes) through a second table,
    toUpper again: the length pass covers exactly the codes interned since (its
    profiled bytes are theirs), the index — 4,096 slots at first, half full at
    2,048 strings — is rebuilt once and the heap's buffers (1,024 offsets,
    64 KiB) are reallocated; a projection planned before the growth evaluates
    correctly after it."""
    from capf_amd.table import GpuSession
    _route(monkeypatch, "device", None)
    s = GpuSession(0)
    try:
        s.set_profiling(True)
        first = ["alphabet", "Crab", " cab ", "", "B", "a€b", None] * 5
        up = (ToUpper(S), "x")
        t1 = s.table([("s", T_STRING, first, None)])
        d0, _ = _dictionary(s)
        assert t1.withColumns(up, header=H, params={}).column_values("x") == _want(("upper",), first)
        prof = s.profile()
        assert prof["str_fn_len"]["launches"] == 1
        assert prof["str_fn_len"]["bytes"] == 25 * len(d0) + sum(utf8_len(x) for x in d0)
        assert prof["str_idx_build"]["launches"] == 1 and "str_idx_extend" not in prof
        early = t1.withColumns(up, header=H, params={})  # planned now, evaluated after the growth
        covered = len(_dictionary(s)[0])  # (planning it extended the map over the first call's results)
        assert covered > len(d0) and s.profile()["str_fn_len"]["launches"] == 2
        new = [f"{'Ab' if i % 3 == 0 else 'ba-'}{i:05d}{'x' * (i % 97)}" for i in range(3000)] + ["y" * 70000 + "ab"]
        t2 = s.table([("s", T_STRING, new + [None], None)])
        d1, _ = _dictionary(s)
        assert len(d1) > 2048 + len(d0)
        s.reset_profile()
        assert t2.withColumns(up, header=H, params={}).column_values("x") == _want(("upper",), new) + [None]
        prof = s.profile()
        since = d1[covered:]  # the second table's strings: exactly the codes interned since
        assert prof["str_fn_len"]["launches"] == 1
        assert prof["str_fn_len"]["bytes"] == 25 * len(since) + sum(utf8_len(x) for x in since)
        assert prof["str_fn_long_len"]["launches"] == 1 and prof["str_fn_long"]["launches"] == 1
        assert prof["str_idx_build"]["launches"] == 1 and "str_idx_extend" not in prof
        assert early.column_values("x") == _want(("upper",), first)
        # a third, small step: the index is extended over the codes added since, not rebuilt
        s.reset_profile()
        t3 = s.table([("s", T_STRING, ["one more", "Two More"], None)])
        assert t3.withColumns(up, header=H, params={}).column_values("x") == ["ONE MORE", "TWO MORE"]
        prof = s.profile()
        assert prof["str_idx_extend"]["launches"] == 1 and "str_idx_build" not in prof
        d, _ = _dictionary(s)
        assert len(set(d)) == len(d)
    finally:
        s.close()


# ------------------------------------------------------------ GPU: the cap
@pytest.mark.gpu
def test_no_cap_on_distinct_values(monkeypatch):
    """Past CODE_MAP_MAX dictionary strings and past VALUE_MAP_MAX distinct
    operand values the functions still run — the distinct codes are mapped on
    the device, no Python string per value; toString, whose strings the host
    builds, keeps the cap."""
    import capf_amd.table as tb
    from capf_amd.table import GpuSession
    monkeypatch.delenv("CAPF_STR_FN", raising=False)
    monkeypatch.delenv("CAPF_STR_LONG", raising=False)
    monkeypatch.setattr(tb, "CODE_MAP_MAX", 4)
    monkeypatch.setattr(tb, "VALUE_MAP_MAX", 8)
    s = GpuSession(0)
    try:
        s.set_profiling(True)
        subj = [f" Value {i:04d} ab " for i in range(1000)] * 2 + [None]
        t = s.table([("s", T_STRING, subj, None), ("k", T_INT, list(range(2001)), None)])
        _check(t, subj, [UNARY[0], UNARY[2], SUBSTRINGS[6], REPLACES[0]])
        prof = s.profile()
        assert prof["str_fn_len"]["launches"] == 4 and prof["str_fn_write"]["launches"] == 4
        assert prof["str_fn_len"]["bytes"] == 4 * (25 * 1000 + sum(utf8_len(x) for x in subj[:1000]))
        with pytest.raises(_lib.NotImplementedException):
            t.withColumns((ToString(Var("k")), "x"), header=H, params={}).column_values("x")
    finally:
        s.close()


# ------------------------------------------------------- GPU: reference cases
def _string_fn_cases():
    from reference_cases import CASES
    pat = re.compile(r"\b(ToUpper|ToLower|Trim|LTrim|RTrim|Substring|Replace)\(")
    return [c for c in CASES if pat.search(repr(c[3]))]


def test_reference_cases_selected():
    assert len(_string_fn_cases()) >= 20


@pytest.mark.gpu
@pytest.mark.parametrize("compact", [False, True, 3], ids=["int64", "for32", "for24"])
def test_reference_cases_on_device_route(gpu_session, monkeypatch, compact):
    from conftest import case_parts, check_case
    from capf_amd.graph import ScanGraph
    from capf_amd.planner import run
    from oracle.create_parser import parse_create
    _route(monkeypatch, "device", None)
    bad = []
    for case in _string_fn_cases():
        cid, src, create, query, expected, opts = case_parts(case)
        got = run(ScanGraph.from_data(gpu_session, parse_create(create), compact=compact), query, opts.get("params"))
        if not check_case(got, expected, opts):
            bad.append((cid, got))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_reference_cases_through_jni(monkeypatch):
    """The same cases through the JNI adapter: Native.stringFnCodes carries the
    source range and the result codes as direct buffers."""
    import ctypes
    import jni_route
    from conftest import case_parts, check_case
    from capf_amd.graph import ScanGraph
    from capf_amd.planner import run
    from capf_amd.table import GpuSession
    from oracle.create_parser import parse_create
    _route(monkeypatch, "device", None)
    jni_route.build()
    native_calls = []

    class Route(jni_route.JniRoute):
        def adapters(self):
            A = super().adapters()
            L, I = ctypes.c_int64, ctypes.c_int32

            def fn_codes(s, fn, i0, i1, l0, l1, src, c0, n, out):
                native_calls.append(fn)
                self.native("stringFnCodes", None, (L, s.value), (I, fn), (L, i0), (L, i1), (L, l0), (L, l1),
                            self.direct(src, 8 * n), (L, c0), (L, n), self.direct(out, 8 * n))
                return self.done()
            A["capf_string_fn_codes"] = fn_codes
            return A

    route = Route()
    bad = []
    for case in _string_fn_cases():
        cid, src, create, query, expected, opts = case_parts(case)
        route.install()
        try:
            got = run(ScanGraph.from_data(GpuSession(0), parse_create(create)), query, opts.get("params"))
        finally:
            route.uninstall()
        if not check_case(got, expected, opts):
            bad.append((cid, got))
    assert not bad, bad
    assert native_calls, "Native.stringFnCodes was never called"
    # a buffer shorter than 8 * n bytes is refused by the adapter, not read past its end
    s = GpuSession(0)
    try:
        s.intern("abc")
        out = np.zeros(1, dtype=np.int64)
        with pytest.raises(_lib.IllegalArgumentException):
            route.native("stringFnCodes", None, (ctypes.c_int64, s._h.value), (ctypes.c_int32, 0), (ctypes.c_int64, 0),
                         (ctypes.c_int64, 0), (ctypes.c_int64, -1), (ctypes.c_int64, -1), None, (ctypes.c_int64, 0),
                         (ctypes.c_int64, 1), route.direct(out.ctypes.data, 4))
    finally:
        route.lib.fj_reset()
        s.close()


# ---------------------------------------------------------- GPU: distributed
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.gpu
def test_to_upper_distributed_keeps_dictionaries_equal():
    """Two ranks (gloo, both on device 0), each holding its hash share of the
    rows and so its own distinct values: every rank maps the sorted union of
    all ranks' codes, the rows are right and the dictionaries end equal."""
    import queue
    import time
    import torch.multiprocessing as mp
    from string_fn_dist_worker import subjects, worker
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res, deadline = [], time.monotonic() + 100
    try:
        while len(res) < len(procs) and time.monotonic() < deadline:
            try:
                res.append(q.get(timeout=1))
            except queue.Empty:  # a rank that died without reporting ends the wait
                if not all(p.is_alive() or p.exitcode == 0 for p in procs):
                    break
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    assert len(res) == len(procs), [p.exitcode for p in procs]
    subj = subjects()
    want = sorted((i, x.upper()) for i, x in enumerate(subj))
    for rank, rows, n_mine, cnt, dig, launches in res:
        assert n_mine is not None, rows
        assert rows == want and 0 < n_mine < 1000 and launches == 1, (rank, n_mine, launches)
    assert res[0][3:5] == res[1][3:5]
