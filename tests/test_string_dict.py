"""The session's string dictionary (csrc/string_dict.h): the host parsers its
device tables are filled from (csrc/string_parse.h), and the tables, the heap,
the match tables and the hash index as the dictionary grows past each of
their first capacities.

The parsers are compiled alone, with the host compiler under
AddressSanitizer and UBSan, and compared with plain Python: UTF-16 lengths and
order from `str.encode("utf-16-le")`, the casts from the grammar of
java.lang.Double.valueOf / the reference's toInteger expectations, restated
here.  The device side is compared with the numpy oracle (STARTS WITH, which
the oracle does not know, with str.startswith).
"""
import math
import os
import re
import struct
import subprocess

import pytest

from capf_amd.expr import (T_INT, T_STRING, IntegerLit, Size, StartsWith, StringLit, Substring, ToBoolean, ToFloat,
                           ToInteger, Var)
from capf_amd.header import RecordHeader
from oracle.table_np import OracleSession

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------ string_parse.h
STRING_PARSE_MAIN = r"""
#include <cstdio>
#include <string>
#include <vector>
#include "string_parse.h"
// argv: strings as hex bytes behind "h:".  One line per string — UTF-16
// length, boolean (0 / 1 / 2), "d <%.17g>" or "-", "i <value>" or "-" — then
// one line per string of utf16_cmp against every string.
int main(int argc, char **argv) {
  std::vector<std::string> in;
  for (int a = 1; a < argc; ++a) {
    std::string s;
    for (const char *p = argv[a] + 2; p[0] && p[1]; p += 2) {
      unsigned v = 0;
      sscanf(p, "%2x", &v);
      s.push_back((char)v);
    }
    in.push_back(s);
  }
  for (const std::string &s : in) {
    double d = 0;
    int64_t v = 0;
    printf("%lld %d ", (long long)capf::utf16_length(s), (int)capf::parse_bool(s));
    if (capf::parse_java_double(s, &d)) printf("d %.17g ", d); else printf("- ");
    if (capf::parse_int32(s, &v)) printf("i %lld\n", (long long)v); else printf("-\n");
  }
  for (const std::string &a : in) {
    for (const std::string &b : in) printf("%d ", capf::utf16_cmp(a, b));
    printf("\n");
  }
}
"""

DIGITS40 = "1234567890" * 4
TEXT = [
    "", "a", "é", "€", "\U0001F600",  # empty, 1, 2, 3 and 4 bytes
    "\uffff", "\U00010000",  # UTF-16 order (D800 DC00 < FFFF) differs from code-point order
    "\U0001F600", "\U0001F601", "x\U0001F600", "x\U0001F601y",  # the same high surrogate D83D
    "\ud800", "a\ud800b", "\udfff",  # lone surrogates: WTF-8 bytes ED A0 80 / ED BF BF
    "ab", "a€", "a€b", "straße", "", "z",
]
CASTS = [" TrUe ", "false", "FALSE\t", "tru", "82.9", "2147483647", "2147483648", "-2147483648", "-2147483649",
         DIGITS40, "-" + DIGITS40, "+", ".", "1e", "1e5f", "NaN", "-Infinity", "+Infinity", "0x10", " 12 ", "+7", "-0",
         ".5", "5.", "1.5e-3D", "1e+", "12a", "1 2", "--1", "٣"]
# cut off inside a multi-byte sequence: a lead byte with too few continuation bytes behind it
CUT = [b"ab\xe2\x82", b"\xf0\x9f", b"x\xc3"]

_DOUBLE = re.compile(r"[+-]?(NaN|Infinity|(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?[fFdD]?)", re.ASCII)
_INT = re.compile(r"[+-]?\d+(\.\d*)?", re.ASCII)


def _jtrim(s):  # java.lang.String.trim
    return s.strip("".join(chr(c) for c in range(33)))


def _units(s):
    b = s.encode("utf-16-le", "surrogatepass")
    return list(struct.unpack("<%dH" % (len(b) // 2), b))


def _want_line(s):
    t = _jtrim(s)
    boolean = {"true": 1, "false": 0}.get(t.lower(), 2)
    d = None
    if _DOUBLE.fullmatch(t):
        if t.lstrip("+-") in ("NaN", "Infinity"):
            d = float(t.replace("Infinity", "inf"))
        else:
            d = float(t[:-1] if t[-1] in "fFdD" else t)
    i = None
    if _INT.fullmatch(t):
        i = int(t.split(".")[0])
        i = i if -2 ** 31 <= i < 2 ** 31 else None
    return len(s.encode("utf-16-le", "surrogatepass")) // 2, boolean, d, i


def _parse_line(line):
    f = line.split()
    d = float(f[3]) if f[2] == "d" else None
    rest = f[4:] if f[2] == "d" else f[3:]
    return int(f[0]), int(f[1]), d, (int(rest[1]) if rest[0] == "i" else None)


def _same(a, b):
    """== on the parsed tuples, doubles by bit pattern (NaN equals NaN, −0.0 is not 0.0)."""
    da, db = a[2], b[2]
    if da is not None and db is not None:
        if not (math.isnan(da) and math.isnan(db)) and struct.pack("<d", da) != struct.pack("<d", db):
            return False
        da = db = None
    return (a[0], a[1], da, a[3]) == (b[0], b[1], db, b[3])


def test_string_parse_under_asan_ubsan(tmp_path):
    """csrc/string_parse.h compiled alone with the host compiler under
    -fsanitize=address,undefined (any report aborts): lengths, casts and the
    comparison of every pair against plain Python; the strings cut off inside a
    multi-byte sequence have no Java meaning, so for them the run must be clean
    and the comparison a consistent order."""
    src = tmp_path / "string_parse_main.cpp"
    src.write_text(STRING_PARSE_MAIN)
    exe = tmp_path / "string_parse_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "cypher-for-apache-flink_amd", "csrc"), str(src), "-o", str(exe)])
    strings = TEXT + CASTS
    raw = [s.encode("utf-8", "surrogatepass") for s in strings] + CUT
    out = subprocess.run([str(exe)] + ["h:" + b.hex() for b in raw], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    n, m = len(strings), len(raw)
    assert len(lines) == 2 * m
    got = [_parse_line(x) for x in lines[:m]]
    bad = [(s, g, _want_line(s)) for s, g in zip(strings, got) if not _same(g, _want_line(s))]
    assert not bad, bad
    # known answers, so that a mistake shared with the restatement above shows
    known = {" TrUe ": (6, 1, None, None), "82.9": (4, 2, 82.9, 82), "2147483647": (10, 2, 2147483647.0, 2147483647),
             "2147483648": (10, 2, 2147483648.0, None), "-2147483648": (11, 2, -2147483648.0, -2147483648),
             DIGITS40: (40, 2, float(DIGITS40), None), "+": (1, 2, None, None), ".": (1, 2, None, None),
             "1e": (2, 2, None, None), "1e5f": (4, 2, 100000.0, None), "NaN": (3, 2, math.nan, None),
             "-Infinity": (9, 2, -math.inf, None), "0x10": (4, 2, None, None), "": (0, 2, None, None),
             "\U0001F600": (2, 2, None, None), "\uffff": (1, 2, None, None), "\ud800": (1, 2, None, None),
             "a€b": (3, 2, None, None)}
    for s, want in known.items():
        assert _same(got[strings.index(s)], want), (s, got[strings.index(s)], want)
    cmp = [[int(x) for x in line.split()] for line in lines[m:]]
    units = [_units(s) for s in strings]
    want_cmp = [[(a > b) - (a < b) for b in units] for a in units]
    assert [row[:n] for row in cmp[:n]] == want_cmp
    i, j = strings.index("\uffff"), strings.index("\U00010000")
    assert cmp[i][j] == 1 and cmp[j][i] == -1  # FFFF above the pair D800 DC00
    by_cmp = sorted(range(n), key=lambda k: sum(c > 0 for c in cmp[k][:n]))
    assert [units[k] for k in by_cmp] == sorted(units)
    for k in range(n, m):  # the cut-off strings: reflexive, antisymmetric, above their own proper prefix
        assert cmp[k][k] == 0 and all(cmp[k][q] == -cmp[q][k] for q in range(m))
    assert cmp[n][strings.index("ab")] == 1 and got[n][1:] == (2, None, None)


# ------------------------------------------------------------------ GPU: growth
H = RecordHeader({Var("s"): "s", Var("k"): "k"})
EXPRS = [("size", Size(Var("s"))), ("int", ToInteger(Var("s"))), ("float", ToFloat(Var("s"))),
         ("bool", ToBoolean(Var("s"))), ("sub", Substring(Var("s"), IntegerLit(1), IntegerLit(2)))]
PATTERN = "1"


def _dict_size(s):
    from ctypes import byref, c_int64, c_uint64
    from capf_amd import _lib
    cnt, dig = c_int64(), c_uint64()
    _lib.call("capf_string_digest", s._h, byref(cnt), byref(dig))
    return cnt.value


def _cols(strings):
    return [("s", T_STRING, strings, None), ("k", T_INT, list(range(len(strings))), None)]


def _check(gpu, cols):
    """Every table of the dictionary read through `cols`, against the oracle."""
    g, o = gpu.table(cols), OracleSession().table(cols)
    for name, e in EXPRS:
        got = g.withColumns((e, "x"), header=H, params={}).column_values("x")
        want = [r["x"] for r in o.withColumns((e, "x"), header=H, params={}).rows]
        assert got == want, (name, next((a, b) for a, b in zip(got, want) if a != b))
    keys = [(Var("s"), "asc"), (Var("k"), "asc")]
    assert g.orderBy(*keys, header=H).rows == o.orderBy(*keys, header=H).rows
    got = g.withColumns((StartsWith(Var("s"), StringLit(PATTERN)), "x"), header=H, params={}).column_values("x")
    assert got == [None if x is None else x.startswith(PATTERN) for x in cols[0][2]]


@pytest.mark.gpu
def test_tables_heap_and_indexes_across_growth(monkeypatch):
    """size, toInteger, toFloat, toBoolean, ORDER BY, a literal STARTS WITH on
    the dictionary path and a device string function over one session whose
    dictionary grows 1 → 1025 → 4097 strings: past the heap offsets' first
    capacity (1024), then past the match table's and the hash index's (4096
    each) and the heap bytes' (64 KiB).  After each growth the earlier tables
    are read again: every derived table was rebuilt, every grown buffer took
    its content along."""
    from capf_amd.table import GpuSession
    monkeypatch.setenv("CAPF_STR_MATCH", "dict")
    monkeypatch.delenv("CAPF_STR_FN", raising=False)
    first = ["17", None]
    second = [str(7 * i - 3000) for i in range(700)] + [f"{i}.75" for i in range(150)] + \
        [f"1e{i}" for i in range(40)] + ["true", "FALSE", " True ", "\U0001F600x", "€", "", "é1"] + \
        [f"w{i:03d}" for i in range(140)] + [None]
    third = [f"{i:020d}" for i in range(1500)] + [f"{i:018d}.5" for i in range(800)] + \
        [f"1-row-{i:05d}-padding-padding-€" for i in range(800)] + [None]
    assert all(len(x) >= 17 for x in third if x is not None)
    assert sum(len(x.encode()) for x in third if x is not None) > 1 << 16
    s = GpuSession(0)
    try:
        s.set_profiling(True)
        steps = [_cols(first)]
        t = s.table(steps[0])
        assert _dict_size(s) == 1  # every table's first build is over one string
        for name, e in EXPRS[:4]:
            assert t.withColumns((e, "x"), header=H, params={}).column_values("x") == \
                [{"size": 2, "int": 17, "float": 17.0, "bool": None}[name], None]
        _check(s, steps[0])
        for strings, at_least, below in ((second, 1025, 4096), (third, 4097, 1 << 16)):
            before = _dict_size(s)
            steps.append(_cols(strings))
            s.table(steps[-1])
            assert before < at_least - 1 and at_least <= _dict_size(s) < below
            for cols in reversed(steps):  # the new table first, then the old ones again
                _check(s, cols)
        prof = s.profile()
        assert "str_match" in prof and "str_fn_probe" in prof and "str_idx_hash" in prof
    finally:
        s.close()


@pytest.mark.gpu
def test_empty_dictionary_gives_empty_and_null_results():
    """No string interned: an empty table gives empty columns, and a row whose
    string is NULL reads the one-row tables of the empty dictionary."""
    from capf_amd.table import GpuSession
    s = GpuSession(0)
    try:
        for strings in ([], [None]):
            cols = _cols(strings)
            g, o = s.table(cols), OracleSession().table(cols)
            assert _dict_size(s) == 0
            for name, e in EXPRS[:4]:
                got = g.withColumns((e, "x"), header=H, params={}).column_values("x")
                assert got == [r["x"] for r in o.withColumns((e, "x"), header=H, params={}).rows] == [None] * len(strings)
            assert g.orderBy((Var("s"), "asc"), header=H).rows == o.orderBy((Var("s"), "asc"), header=H).rows
    finally:
        s.close()
