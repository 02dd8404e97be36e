"""Typed CSV ingest of the FS graph source (capf_csv_parse_typed / _read_typed,
csrc/edge_list.hip; DESIGN.md "Typed CSV ingest").

The host reader `fs_source._parse_csv` is the specification: every input the
device parser accepts must give that reader's INTEGER / FLOAT / BOOLEAN /
STRING values, NULL positions included (FLOATs compared as bit patterns);
DATE / LOCALDATETIME expectations come from `datetime`.  Every input outside
the device grammars must be rejected naming the first bad line, and through
`FSGraphSource` such a file must load by the host reader exactly as before
(route "host") or raise the host reader's own error.
"""
import datetime
import json
import os
import random
import struct

import pytest

from conftest import bag

import capf_import  # noqa: F401
from capf_amd import _lib
from capf_amd import fs_source as fs
from capf_amd.expr import (T_BOOL, T_DATE, T_FLOAT, T_INT, T_LOCALDATETIME, T_STRING, ElementProperty, Var)
from capf_amd.fs_source import FSGraphSource
from capf_amd.planner import Match, NodeP, Query, RelP, Stage, run

HERE = os.path.dirname(os.path.abspath(__file__))
TYPED_ROOT = os.path.join(HERE, "golden", "fs_typed")
CHUNK = 16384  # bytes per workgroup of the parse kernels (EL_CHUNK)
D, DT = datetime.date, datetime.datetime


def bits(v):
    return None if v is None else struct.pack("<d", v)


def iso(s, t):
    """Expected temporal of a field written by the tests themselves (fixed-width ISO text)."""
    if s is None:
        return None
    d = D(int(s[0:4]), int(s[5:7]), int(s[8:10]))
    if t == T_DATE:
        return d
    return DT(d.year, d.month, d.day, int(s[11:13]), int(s[14:16]), int(s[17:19]), int(s[20:].ljust(6, "0") or 0))


def expected_columns(tmp_path, data, types, sep=","):
    """The host reader on the same bytes: its INTEGER / FLOAT / BOOLEAN / STRING
    paths as they are; temporal columns read as STRING and converted by iso()."""
    path = tmp_path / "expected.csv"
    path.write_bytes(data)
    names = [f"c{i}" for i in range(len(types))]
    host_types = [T_STRING if t in (T_DATE, T_LOCALDATETIME) else t for t in types]
    assert sep == ","  # the host reader splits on ',' only
    cols = [vals for _, _, vals, _ in fs._parse_csv(str(path), host_types, names)]
    return [[iso(v, t) for v in vals] if t in (T_DATE, T_LOCALDATETIME) else vals for vals, t in zip(cols, types)]


def typed_columns(session, data, types, sep=","):
    names = [f"c{i}" for i in range(len(types))]
    t = session.csv_parse_typed(data, sep, names, types)
    return t, [t.column_values(n) for n in names]


def same(got, want, types):
    assert len(got) == len(want)
    for g, w, t in zip(got, want, types):
        if t == T_FLOAT:
            assert [bits(x) for x in g] == [bits(x) for x in w]
        else:
            assert g == w
            assert [type(x) for x in g] == [type(x) for x in w]


def has_mask(table, col):
    from ctypes import byref, c_int32
    v = c_int32()
    _lib.call("capf_table_has_nulls", table._h, col.encode(), byref(v))
    return bool(v.value)


def check(session, tmp_path, data, types):
    t, got = typed_columns(session, data, types)
    same(got, expected_columns(tmp_path, data, types), types)
    return t, got


ALL6 = [T_INT, T_FLOAT, T_BOOL, T_STRING, T_DATE, T_LOCALDATETIME]

# ----------------------------------------------------------------- CPU
DATES = {"0001-01-01": D(1, 1, 1), "9999-12-31": D(9999, 12, 31), "1970-01-01": D(1970, 1, 1),
         "1969-12-31": D(1969, 12, 31), "2000-02-29": D(2000, 2, 29), "2100-02-28": D(2100, 2, 28)}
DATETIMES = {"2010-10-10T12:00:00.5": DT(2010, 10, 10, 12, 0, 0, 500000),
             "2010-10-10T12:00:00.123": DT(2010, 10, 10, 12, 0, 0, 123000),
             "2010-10-10T12:00:00.000001": DT(2010, 10, 10, 12, 0, 0, 1),
             "9999-12-31T23:59:59.999999": DT(9999, 12, 31, 23, 59, 59, 999999),
             "1969-12-31T23:59:59.25": DT(1969, 12, 31, 23, 59, 59, 250000),
             "0001-01-01T00:00:00": DT(1, 1, 1)}
BAD_DATES = ["1900-02-29", "2010-1-01", "0000-01-01", "2010-13-01", "2010-01-32", "2010-01-1x", " 2010-01-01"]
BAD_DATETIMES = ["2010-10-10T24:00:00", "2010-10-10T12:00:00.1234567", "2010-10-10 12:00:00", "2010-10-10T12:60:00",
                 "2010-10-10T12:00:60", "2010-10-10T12:00:00.", "2010-10-10"]


def test_host_reader_parses_temporals():
    for s, want in DATES.items():
        assert fs._parse_field(s, T_DATE, 1, "p") == want and type(fs._parse_field(s, T_DATE, 1, "p")) is D
    for s, want in DATETIMES.items():
        assert fs._parse_field(s, T_LOCALDATETIME, 1, "p") == want
    assert fs._parse_field("", T_DATE, 1, "p") is None
    for s in BAD_DATES:
        with pytest.raises(ValueError, match="line 3"):
            fs._parse_field(s, T_DATE, 3, "p")
    for s in BAD_DATETIMES:
        with pytest.raises(ValueError, match="line 3"):
            fs._parse_field(s, T_LOCALDATETIME, 3, "p")


def test_formatter_writes_temporals_and_delegates():
    for s, v in DATES.items():
        assert fs._format_csv_field(v) == s
    assert fs._format_csv_field(DT(2010, 10, 10, 12, 0, 0, 500000)) == "2010-10-10T12:00:00.500000"
    assert fs._format_csv_field(DT(1, 1, 1)) == "0001-01-01T00:00:00"
    assert fs._format_csv_field(DT(9999, 12, 31, 23, 59, 59, 999999)) == "9999-12-31T23:59:59.999999"
    for v in (None, True, False, 7, -1.5, "x,y"):
        assert fs._format_csv_field(v) == fs._format_field(v)
    # what is written is read back
    for v in list(DATES.values()):
        assert fs._parse_field(fs._format_csv_field(v), T_DATE, 1, "p") == v
    for v in list(DATETIMES.values()):
        assert fs._parse_field(fs._format_csv_field(v), T_LOCALDATETIME, 1, "p") == v


class HostOnlySession:
    """A session without the device CSV entries (as the distributed layer's):
    `table` hands back what the host reader produced."""

    def table(self, columns):
        return columns

    def empty(self, names, types):
        return [(n, t, [], None) for n, t in zip(names, types)]


def test_read_table_takes_temporal_fields_on_the_host():
    src = FSGraphSource(HostOnlySession(), TYPED_ROOT)
    fields = [("id", "INTEGER")] + [(fs.PROPERTY_PREFIX + k, ct) for k, ct in fs._canonical_props(
        src.schema("typed")[0][frozenset(["Person"])])]
    assert [f for f, _ in fields] == ["id"] + ["property_" + k for k in ("active", "age", "born", "name", "nick",
                                                                         "score", "seen")]
    cols = {n: vals for n, _, vals, _ in src._read_table(src.node_table_path("typed", {"Person"}), fields)}
    assert [r for _, r in src.routes] == ["host"]
    assert cols["property_born"] == [D(1980, 2, 29), D(1969, 12, 31), D(2000, 1, 1), D(9999, 12, 31)]
    assert cols["property_seen"] == [DT(2020, 1, 2, 3, 4, 5), DT(1969, 12, 31, 23, 59, 59, 999999),
                                     DT(2001, 9, 9, 1, 46, 40, 500000), DT(1, 1, 1)]
    assert cols["property_age"] == [42, None, 7, 23] and cols["property_nick"] == ["zo", None, "em", None]
    assert cols["property_active"] == [True, False, True, False]
    assert [bits(x) for x in cols["property_score"]] == [bits(x) for x in (1.5, 0.30000000000000004, -0.0, 1e23)]
    # the '\r\n' relationship file, and a table directory without files
    rel = [("id", "INTEGER"), ("source", "INTEGER"), ("target", "INTEGER"), ("property_note", "STRING"),
           ("property_since", "DATE"), ("property_weight", "FLOAT?")]
    cols = {n: vals for n, _, vals, _ in src._read_table(src.rel_table_path("typed", "KNOWS"), rel)}
    assert cols["property_since"] == [D(2010, 10, 10), D(1999, 12, 31), D(2016, 2, 29), D(1970, 1, 1)]
    assert cols["property_weight"] == [0.25, None, 2.0, 0.001] and cols["property_note"] == ["café", "old", "café", "x"]
    assert src._read_table(os.path.join(TYPED_ROOT, "absent"), rel)[4] == ("property_since", T_DATE, [], None)


def test_typed_fixture_layout_and_schema():
    from oracle.table_np import OracleSession
    src = FSGraphSource(OracleSession(), TYPED_ROOT)
    assert src.graph_names() == {"typed"} and src.has_graph("typed")
    assert src.metadata("typed") == {"tableStorageFormat": "csv", "tags": [0]}
    nodes, rels = src.schema("typed")
    assert nodes == {frozenset(["Person"]): {"name": "STRING", "nick": "STRING?", "age": "INTEGER?", "score": "FLOAT",
                                             "active": "BOOLEAN", "born": "DATE", "seen": "LOCALDATETIME"}}
    assert rels == {"KNOWS": {"note": "STRING", "since": "DATE", "weight": "FLOAT?"}}
    assert os.path.isfile(os.path.join(src.node_table_path("typed", {"Person"}), "table.csv"))
    rel_file = os.path.join(src.rel_table_path("typed", "KNOWS"), "table.csv")
    assert open(rel_file, "rb").read().count(b"\r\n") == 4  # the '\r\n' file of the fixture


# ----------------------------------------------------------------- GPU, raw entry
@pytest.mark.gpu
@pytest.mark.parametrize("data", [b"", b"1,1.5,true,a,2010-10-10,2010-10-10T01:02:03",
                                  b"1,1.5,true,a,2010-10-10,2010-10-10T01:02:03\n",
                                  b"1,1.5,true,a,2010-10-10,2010-10-10T01:02:03\r\n2,,,,,\r\n3,2,FALSE,b,1999-01-01,"
                                  b"1999-01-01T00:00:00.5\r",
                                  b"\n\n", b"7\r\n", b"1,2,3,4,5,6,seven,eight\n"],
                         ids=["empty", "no-newline", "newline", "crlf", "blank-lines", "one-field", "extra-fields"])
def test_small_shapes(gpu_session, tmp_path, data):
    types = ALL6 if data not in (b"\n\n", b"7\r\n") else [T_INT]
    if data.startswith(b"1,2,3,4"):
        types = [T_INT, T_FLOAT, T_STRING]
    t, got = check(gpu_session, tmp_path, data, types)
    assert t.size == len(got[0])
    if data == b"":
        assert t.size == 0


@pytest.mark.gpu
def test_exactly_one_chunk(gpu_session, tmp_path):
    line = b"12345,0.5,true,abcdefgh,2001-02-03,2001-02-03T04:05:06.789\n"
    n = CHUNK // len(line)
    pad = CHUNK - n * len(line)
    data = line * (n - 1) + line[:-1] + b"," + b"x" * (pad - 1) + b"\n"
    assert len(data) == CHUNK and data[-1:] == b"\n"
    check(gpu_session, tmp_path, data, ALL6)
    check(gpu_session, tmp_path, data[:-1] + b"y", ALL6)  # the same size without a final newline


POOL = ["a", "Zoë", "名前", "😀 smile", "repeat", "x" * 40, "é", "tab\there", " lead", "trail ", "q\"uote"]


def straddle_file(seed=7):
    """A file just over two chunks with all six types and lines of varying
    length; a line, a field and a 3-byte character straddle the first chunk
    boundary, a '\\r\\n' pair the second."""
    rng = random.Random(seed)
    out = bytearray()

    def fields(i):
        nint = "" if rng.random() < 0.2 else str(rng.randrange(-10**rng.randrange(1, 18), 10**rng.randrange(1, 18)))
        flt = rng.choice(["", "0", "-0.0", "1.5", "1e22", "1e23", "0.1", "123456.789e-3", "9007199254740993",
                          repr(rng.random()), str(rng.randrange(10**6)) + "." + str(rng.randrange(10**4))])
        boo = rng.choice(["", "true", "false", "TRUE", "False"])
        day = D.fromordinal(rng.randrange(1, D.max.toordinal() + 1))
        date = "" if rng.random() < 0.1 else day.isoformat()
        frac = rng.choice(["", ".5", ".123", ".000001", ".999999"])
        dt = "" if rng.random() < 0.1 else "%sT%02d:%02d:%02d%s" % (day.isoformat(), rng.randrange(24), rng.randrange(60),
                                                                   rng.randrange(60), frac)
        return f"{i},{nint},{flt},{boo},", f",{date},{dt}"

    i = 0
    for boundary, what in ((CHUNK, "char"), (2 * CHUNK, "crlf"), (2 * CHUNK + 700, None)):
        while len(out) < boundary - 400:
            pre, post = fields(i)
            s = "" if rng.random() < 0.1 else rng.choice(POOL)
            out += (pre + s + post + rng.choice(["\n", "\r\n"])).encode()
            i += 1
        pre, post = fields(i)
        at = len(out) + len(pre.encode())
        if what == "char":  # '€' = E2 82 AC starts on the last byte of the chunk
            out += (pre + "x" * (boundary - 1 - at) + "€" + post + "\n").encode()
        elif what == "crlf":  # '\r' the last byte of the chunk, '\n' the first of the next
            out += (pre + "y" * (boundary - 1 - at - len(post.encode())) + post + "\r\n").encode()
        i += 1
    return bytes(out)


@pytest.mark.gpu
def test_three_chunks_with_straddles(gpu_session, tmp_path):
    data = straddle_file()
    assert 2 * CHUNK < len(data) < 2 * CHUNK + 600
    # the generator produced every straddle
    assert data[CHUNK - 1:CHUNK + 2] == "€".encode()  # a multi-byte character
    assert b"\n" not in data[CHUNK - 1:CHUNK + 1] and b"," not in data[CHUNK - 1:CHUNK + 1]  # a line and a field
    assert data[2 * CHUNK - 1:2 * CHUNK + 1] == b"\r\n"  # a '\r\n' pair
    lens = {len(x) for x in data.split(b"\n")}
    assert len(lens) > 20  # lines of varying length
    types = [T_INT, T_INT, T_FLOAT, T_BOOL, T_STRING, T_DATE, T_LOCALDATETIME]
    t, got = check(gpu_session, tmp_path, data, types)
    # strings repeat across chunks, and every type has NULLs and values
    assert all(data[k * CHUNK:(k + 1) * CHUNK].count(b",repeat,") for k in range(2))
    for col in got[1:]:
        assert None in col and any(v is not None for v in col)
    assert not has_mask(t, "c0") and all(has_mask(t, f"c{k}") for k in range(1, 7))
    assert gpu_session.csv_slow_floats() > 0


@pytest.mark.gpu
def test_line_longer_than_a_chunk(gpu_session, tmp_path):
    long = "é" * 9000 + "z" * 2000  # 20 000 bytes
    data = ("1,short\n2," + long + "\n3,short,ignored\n4," + long).encode()
    t, got = check(gpu_session, tmp_path, data, [T_INT, T_STRING])
    assert got[1][1] == long and got[1][3] == long


@pytest.mark.gpu
def test_null_columns_and_masks(gpu_session, tmp_path):
    data = b"1,,x,\n2,,y,\n3,,z,\n"
    t, got = check(gpu_session, tmp_path, data, [T_INT, T_FLOAT, T_STRING, T_DATE])
    assert got[1] == [None] * 3 and got[3] == [None] * 3
    assert not has_mask(t, "c0") and has_mask(t, "c1") and not has_mask(t, "c2") and has_mask(t, "c3")


@pytest.mark.gpu
def test_multi_byte_separator(gpu_session):
    data = "1||a|b||2.5||\n2||||1e3||true\n".encode()
    _, got = typed_columns(gpu_session, data, [T_INT, T_STRING, T_FLOAT, T_BOOL], sep="||")
    assert got == [[1, 2], ["a|b", None], [2.5, 1000.0], [None, True]]
    with pytest.raises(_lib.IllegalArgumentException):
        gpu_session.csv_parse_typed(b"1\n", "é", ["a"], [T_INT])
    with pytest.raises(_lib.IllegalArgumentException):
        gpu_session.csv_parse_typed(b"1\n", ",", ["a"], [5])  # LIST is not a field type


@pytest.mark.gpu
def test_strings(gpu_session, tmp_path):
    known = "already interned ✓"
    code = gpu_session.intern(known)
    units = ["a", "é", "€", "😀", "a é € 😀", "ÿĀ߿ࠀ￿\U00010000\U0010ffff", "\x7f\x01"]
    rows = [(u, units[(i + 3) % len(units)]) for i, u in enumerate(units)] + [(known, "fresh"), ("fresh", known),
                                                                              ("", "same"), ("same", "same")]
    filler = [("pad%d" % (i % 5), "x" * 50) for i in range(400)]  # pushes the repeats below into a second chunk
    rows = rows + filler + rows
    data = "".join(f"{i},{a},{b}\n" for i, (a, b) in enumerate(rows)).encode()
    assert len(data) > CHUNK
    t, got = check(gpu_session, tmp_path, data, [T_INT, T_STRING, T_STRING])
    assert got[1] == [a or None for a, _ in rows] and got[2] == [b for _, b in rows]
    # a string the dictionary held keeps its code; equal strings share one
    c1 = t.column_arrays("c1")[0].tolist()
    c2 = t.column_arrays("c2")[0].tolist()
    at = [a for a, _ in rows].index(known)
    assert c1[at] == code and c2[at + 1] == code
    assert c1[at + 3] == c2[at + 3] == c2[at + 2]  # "same" in two columns


FLOATS_SLOW = ["1e23", "9007199254740993", "0.30000000000000004", "12345678901234567", "1.2345678901234567",
               "1e-23", "5e-324", "1e400", "-1e400", "1.7976931348623157e308", "1e-400", "123456789012345678901234567890",
               "0.1e-22", "2.2250738585072011e-308", "100000000000000000000000"]
FLOATS_FAST = ["0", "-0.0", ".5", "5.", "+1.5", "1e22", "9007199254740992", "123456789012345", "1234567890123456",
               "0.1", "1e-22", "-1E+5", "1.5e-3", "00012.50", "9007199254740992e22", "-.0e0", "4.35", "0.000001"]


@pytest.mark.gpu
def test_floats_bit_for_bit(gpu_session, tmp_path):
    for group, slow in ((FLOATS_FAST, False), (FLOATS_SLOW, True), (FLOATS_FAST + FLOATS_SLOW, True)):
        data = "".join(f"{i},{s}\n" for i, s in enumerate(group)).encode()
        _, got = check(gpu_session, tmp_path, data, [T_INT, T_FLOAT])
        assert [bits(x) for x in got[1]] == [bits(float(s)) for s in group]
        n = gpu_session.csv_slow_floats()
        # neither path can stand in for the other
        assert n == (len(FLOATS_SLOW) if slow else 0), (n, group)
    assert bits(got[1][1]) == bits(-0.0) != bits(0.0)
    # the same through the file entry (the host conversions read the file's bytes)
    path = tmp_path / "floats.csv"
    path.write_bytes(data)
    t = gpu_session.csv_read_typed(str(path), ",", ["i", "f"], [T_INT, T_FLOAT])
    assert [bits(x) for x in t.column_values("f")] == [bits(float(s)) for s in FLOATS_FAST + FLOATS_SLOW]
    assert gpu_session.csv_slow_floats() == len(FLOATS_SLOW)


@pytest.mark.gpu
def test_temporals(gpu_session):
    data = "".join(f"{d},\n" for d in DATES) + "".join(f",{d}\n" for d in DATETIMES)
    _, got = typed_columns(gpu_session, data.encode(), [T_DATE, T_LOCALDATETIME])
    assert got[0] == list(DATES.values()) + [None] * len(DATETIMES)
    assert got[1] == [None] * len(DATES) + list(DATETIMES.values())


# (name, types, bytes, first bad line)
REJECTED = [
    ("1900-02-29", [T_INT, T_DATE], b"1,1900-02-28\n2,1900-02-29\n", 2),
    ("2010-1-01", [T_DATE], b"2010-1-01\n", 1),
    ("0000-01-01", [T_DATE], b"0001-01-01\n0000-01-01\n", 2),
    ("2010-13-01", [T_DATE], b"2010-13-01", 1),
    ("24:00:00", [T_LOCALDATETIME], b"2010-10-10T23:00:00\n2010-10-10T24:00:00\n", 2),
    ("7-digit fraction", [T_LOCALDATETIME], b"2010-10-10T12:00:00.1234567\n", 1),
    ("space for T", [T_LOCALDATETIME], b"2010-10-10 12:00:00\n", 1),
    ("' 1.0'", [T_INT, T_FLOAT], b"1, 1.0\n", 1),
    ("inf", [T_FLOAT], b"1\ninf\n", 2),
    ("nan", [T_FLOAT], b"nan\n", 1),
    ("1_0 float", [T_FLOAT], b"1_0\n", 1),
    ("1_0 int", [T_INT], b"1_0\n", 1),
    ("+1", [T_INT], b"1\n+1\n", 2),
    ("yes", [T_BOOL], b"true\nyes\n", 2),
    ("lone cr", [T_INT, T_STRING], b"1,a\n2,b\rc\n", 2),
    ("lone cr in the ignored text", [T_INT], b"1,a\rb\n", 1),
    ("cr cr lf", [T_INT, T_STRING], b"1,a\r\r\n", 1),
    ("short row", [T_INT, T_STRING, T_STRING], b"1,a,b\n2,a\n", 2),
    ("overlong", [T_STRING], b"ok\n\xc0\xaf\n", 2),
    ("overlong 3", [T_STRING], b"\xe0\x80\xaf\n", 1),
    ("surrogate", [T_STRING], b"\xed\xa0\x80\n", 1),
    ("above U+10FFFF", [T_STRING], b"\xf4\x90\x80\x80\n", 1),
    ("truncated at the end", [T_INT, T_STRING], b"1,a\n2,\xe2\x82", 2),
    ("truncated before the separator", [T_STRING, T_INT], b"\xe2\x82,1\n", 1),
    ("nul byte", [T_INT, T_STRING], b"1,a\x00b\n", 1),
    ("high byte in an integer", [T_INT], "1\n١\n".encode(), 2),
    ("high byte in the ignored text", [T_INT], "1,x\n2,é\n".encode(), 2),
    ("int64 overflow", [T_INT], b"9223372036854775807\n9223372036854775808\n", 2),
    ("float garbage", [T_FLOAT], b"1.5\n1.5.2\n", 2),
    ("bare exponent", [T_FLOAT], b"1e\n", 1),
    ("bare point", [T_FLOAT], b".\n", 1),
    ("two bad lines", [T_INT, T_BOOL], b"1,true\n2,maybe\n3,true\nx,true\n", 2),
    ("two bad lines in two chunks", [T_INT, T_STRING], b"1,a\n" * 3000 + b"x,a\n" + b"1,a\n" * 3000 + b"y,b\n", 3001),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,types,data,line", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected(gpu_session, name, types, data, line):
    names = [f"c{i}" for i in range(len(types))]
    with pytest.raises(_lib.IllegalArgumentException, match=rf"CSV line {line} could not be parsed: ") as err:
        gpu_session.csv_parse_typed(data, ",", names, types)
    assert type(err.value) is _lib.IllegalArgumentException


# ----------------------------------------------------------------- GPU, through FSGraphSource
def rows_key(rows):
    """Rows as a sorted list of exact keys (conftest.bag has no temporal kind; repr keeps -0.0 and types)."""
    return sorted(repr(sorted(r.items())) for r in rows)


def _prop(var, key, ct, kind="NODE"):
    return ElementProperty(Var(var, kind), key, ct)


@pytest.mark.gpu
def test_typed_fixture_on_the_typed_route(gpu_session):
    src = FSGraphSource(gpu_session, TYPED_ROOT)
    g = src.graph("typed")
    assert [r for _, r in src.routes] == ["typed", "typed"]
    q = Query([Match([NodeP("a", ("Person",)), NodeP("b", ("Person",))], [RelP("k", "a", "b", ("KNOWS",))])],
              [Stage([("a", _prop("a", "name", "STRING")), ("nick", _prop("a", "nick", "STRING")),
                      ("age", _prop("b", "age", "INTEGER")), ("ok", _prop("a", "active", "BOOLEAN")),
                      ("score", _prop("b", "score", "FLOAT")), ("born", _prop("a", "born", "DATE")),
                      ("seen", _prop("b", "seen", "LOCALDATETIME")),
                      ("note", _prop("k", "note", "STRING", "RELATIONSHIP")),
                      ("since", _prop("k", "since", "DATE", "RELATIONSHIP")),
                      ("w", _prop("k", "weight", "FLOAT", "RELATIONSHIP"))])])
    want = [
        {"a": "Zoë", "nick": "zo", "age": None, "ok": True, "score": 0.30000000000000004, "born": D(1980, 2, 29),
         "seen": DT(1969, 12, 31, 23, 59, 59, 999999), "note": "café", "since": D(2010, 10, 10), "w": 0.25},
        {"a": "名前", "nick": None, "age": 7, "ok": False, "score": -0.0, "born": D(1969, 12, 31),
         "seen": DT(2001, 9, 9, 1, 46, 40, 500000), "note": "old", "since": D(1999, 12, 31), "w": None},
        {"a": "Émile 😀", "nick": "em", "age": 23, "ok": True, "score": 1e23, "born": D(2000, 1, 1),
         "seen": DT(1, 1, 1), "note": "café", "since": D(2016, 2, 29), "w": 2.0},
        {"a": "Bob", "nick": None, "age": 42, "ok": False, "score": 1.5, "born": D(9999, 12, 31),
         "seen": DT(2020, 1, 2, 3, 4, 5), "note": "x", "since": D(1970, 1, 1), "w": 0.001},
    ]
    assert rows_key(run(g, q)) == rows_key(want)


@pytest.mark.gpu
def test_store_read_round_trip_on_the_typed_route(gpu_session, tmp_path):
    from capf_amd.graph import GraphData, ScanGraph
    people = [("Zoë", D(1980, 2, 29), DT(2019, 5, 10, 10, 10, 12, 113114), 4, 1.5),
              ("名前", None, DT(1969, 12, 31, 23, 59, 59, 999999), None, 0.1),
              ("Bob", D(1, 1, 1), None, 7, None), ("Zoë", D(9999, 12, 31), DT(1, 1, 1), -3, 1e-7)]
    keys = ("name", "born", "seen", "n", "x")
    data = GraphData(nodes=[(i, frozenset(["P"]), {k: v for k, v in zip(keys, p) if v is not None})
                            for i, p in enumerate(people)],
                     rels=[(10 + i, i, (i + 1) % 4, "R", {"at": p[2]} if p[2] else {}) for i, p in enumerate(people)])
    g = ScanGraph.from_data(gpu_session, data)
    src = FSGraphSource(gpu_session, str(tmp_path))
    src.store("t", g)
    written = (tmp_path / "t" / "nodes" / "P" / "part-00000.csv").read_text()
    assert "1980-02-29" in written and "2019-05-10T10:10:12.113114" in written and "0001-01-01T00:00:00," in written
    back = src.graph("t")
    assert [r for _, r in src.routes] == ["typed", "typed"]
    q = Query([Match([NodeP("a", ("P",)), NodeP("b", ("P",))], [RelP("r", "a", "b", ("R",))])],
              [Stage([("name", _prop("a", "name", "STRING")), ("born", _prop("a", "born", "DATE")),
                      ("seen", _prop("b", "seen", "LOCALDATETIME")), ("n", _prop("b", "n", "INTEGER")),
                      ("x", _prop("a", "x", "FLOAT")), ("at", _prop("r", "at", "LOCALDATETIME", "RELATIONSHIP"))])])
    got = run(back, q)
    assert rows_key(got) == rows_key(run(g, q))
    assert rows_key(got) == rows_key([{"name": p[0], "born": p[1], "seen": people[(i + 1) % 4][2], "n": people[(i + 1) % 4][3],
                             "x": p[4], "at": p[2]} for i, p in enumerate(people)])


def _one_table_graph(root, props, body):
    """A graph `g` of one node table N: properties {key: type}, the file's bytes."""
    gdir = root / "g"
    (gdir / "nodes" / "N").mkdir(parents=True)
    (gdir / "capsGraphMetaData.json").write_text(json.dumps({"tableStorageFormat": "csv", "tags": [0]}))
    (gdir / "propertyGraphSchema.json").write_text(json.dumps(
        {"version": "1.0", "labelPropertyMap": [{"labels": ["N"], "properties": props}], "relTypePropertyMap": []}))
    (gdir / "nodes" / "N" / "table.csv").write_bytes(body)
    return str(gdir / "nodes" / "N" / "table.csv")


# rejected by the device, accepted by the host reader: (name, {key: type}, bytes)
HOST_ACCEPTS = [
    ("' 1.0'", {"v": "FLOAT"}, b"1, 1.0\n2,2\n"),
    ("inf", {"v": "FLOAT"}, b"1,inf\n2,-Infinity\n"),
    ("nan", {"v": "FLOAT"}, b"1,nan\n"),
    ("1_0 float", {"v": "FLOAT"}, b"1,1_0\n"),
    ("1_0 int", {"v": "INTEGER?"}, b"1,1_0\n2,\n"),
    ("lone cr", {"v": "INTEGER?"}, b"1,5\r2,6\n"),
    ("nul byte", {"v": "STRING"}, b"1,a\x00b\n"),
    ("high byte in an integer", {"v": "INTEGER?"}, "1,١٢\n".encode()),
    ("high byte in the ignored text", {"v": "INTEGER?"}, "1,2,é\n".encode()),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,props,body", HOST_ACCEPTS, ids=[r[0] for r in HOST_ACCEPTS])
def test_host_route_with_todays_values(gpu_session, tmp_path, name, props, body):
    path = _one_table_graph(tmp_path, props, body)
    types = [T_INT] + [fs.CT_TO_CAPF[fs._base_type(ct)[0]] for ct in props.values()]
    with pytest.raises(_lib.IllegalArgumentException):  # no fallback in the way: the device does reject it
        gpu_session.csv_parse_typed(body, ",", ["id", "v"], types)
    today = gpu_session.table(fs._parse_csv(path, types, ["id", "v"]))  # the parent commit's route
    src = FSGraphSource(gpu_session, str(tmp_path))
    t = src.graph("g").node_tables[0].table
    assert src.routes == [(path, "host")]
    for got, want in ((t.column_values("id"), today.column_values("id")),
                      (t.column_values("p_v"), today.column_values("v"))):
        assert [bits(x) if isinstance(x, float) else x for x in got] == \
               [bits(x) if isinstance(x, float) else x for x in want]
    assert t.size == today.size >= 1


# rejected by both: the host reader's own exception is what the caller sees
BOTH_REJECT = [
    ("1900-02-29", {"v": "DATE"}, b"1,1900-02-29\n", ValueError, "line 1"),
    ("2010-1-01", {"v": "DATE"}, b"1,2010-1-01\n", ValueError, "line 1"),
    ("0000-01-01", {"v": "DATE"}, b"1,2000-01-01\n2,0000-01-01\n", ValueError, "line 2"),
    ("2010-13-01", {"v": "DATE?"}, b"1,\n2,2010-13-01\n", ValueError, "line 2"),
    ("24:00:00", {"v": "LOCALDATETIME"}, b"1,2010-10-10T24:00:00\n", ValueError, "line 1"),
    ("7-digit fraction", {"v": "LOCALDATETIME"}, b"1,2010-10-10T12:00:00.1234567\n", ValueError, "line 1"),
    ("space for T", {"v": "LOCALDATETIME"}, b"1,2010-10-10 12:00:00\n", ValueError, "line 1"),
    ("+1", {"v": "INTEGER?"}, b"1,+1\n", ValueError, "line 1"),
    ("yes", {"v": "BOOLEAN"}, b"1,true\n2,yes\n", ValueError, "line 2"),
    ("short row", {"v": "STRING"}, b"1,a\n2\n", ValueError, "too short"),
    ("lone cr, short", {"v": "STRING"}, b"1,a\rb\n", ValueError, "too short"),
    ("overlong", {"v": "STRING"}, b"1,\xc0\xaf\n", UnicodeDecodeError, "invalid start byte"),
    ("surrogate", {"v": "STRING"}, b"1,\xed\xa0\x80\n", UnicodeDecodeError, "invalid continuation byte"),
    ("truncated at the end", {"v": "STRING"}, b"1,\xe2\x82", UnicodeDecodeError, "unexpected end of data"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,props,body,exc,text", BOTH_REJECT, ids=[r[0] for r in BOTH_REJECT])
def test_host_readers_error_propagates(gpu_session, tmp_path, name, props, body, exc, text):
    _one_table_graph(tmp_path, props, body)
    src = FSGraphSource(gpu_session, str(tmp_path))
    with pytest.raises(exc, match=text) as err:
        src.graph("g")
    assert not isinstance(err.value, _lib.CypherException)
    assert src.routes == []


@pytest.mark.gpu
def test_products_keeps_its_rows_and_the_longs_route(gpu_session):
    import test_fs_source as base
    src = FSGraphSource(gpu_session, base.FS_ROOT)
    g = src.graph("products")
    assert bag(run(g, base.BOUGHT_QUERY)) == bag(base.expected_bought())
    routes = {os.path.relpath(p, base.FS_ROOT): r for p, r in src.routes}
    assert routes == {os.path.join("products", "nodes", "Customer", "table.csv"): "typed",
                      os.path.join("products", "nodes", "Product", "table.csv"): "typed",
                      os.path.join("products", "relationships", "BOUGHT", "table.csv"): "longs"}
    # the same rows as the host reader gives (the route of these two node tables until now)
    for t in g.node_tables:
        label = next(iter(t.labels))
        props = src.schema("products")[0][frozenset([label])]
        fields = [("id", "INTEGER")] + [(fs.PROPERTY_PREFIX + k, ct) for k, ct in fs._canonical_props(props)]
        host = fs._parse_csv(os.path.join(src.node_table_path("products", t.labels), "table.csv"),
                             [fs.CT_TO_CAPF[ct] for _, ct in fields], [f for f, _ in fields])
        for (name, _, vals, _), (_, col) in zip(host, FSGraphSource._renames(fields)):
            assert t.table.column_values(col) == vals, (label, name)


@pytest.mark.gpu
def test_distributed_style_session_keeps_the_host_reader(gpu_session, tmp_path):
    """A session without the device entries (the distributed layer's) reads by
    the host reader, and its temporals upload."""
    class HostOnly:
        def __init__(self, s):
            self.table, self.empty = s.table, s.empty

    path = _one_table_graph(tmp_path, {"v": "DATE?"}, b"1,2010-10-10\n2,\n")
    src = FSGraphSource(HostOnly(gpu_session), str(tmp_path))
    t = src._read_table(os.path.dirname(path), [("id", "INTEGER"), ("property_v", "DATE?")])
    assert src.routes == [(path, "host")] and t.column_values("property_v") == [D(2010, 10, 10), None]
