"""DATE and LOCALDATETIME columns, their accessors (CAPF_OP_TEMPORAL_FIELD),
temporal ± duration (CAPF_OP_TEMPORAL_ADD) and the durations that fold on the
host.

The reference is Python's datetime — the same proleptic ISO calendar as
java.time: isocalendar / isoweekday / timetuple().tm_yday for the fields and
`plus_months` below (java.time's plusMonths: the day of month clamped to the
target month's length) for the arithmetic.  The acceptance cases are
tests/golden/temporal_cases.py.  Rows are compared with `rows_key`: typed ==
on the Python values, rows sorted by repr (conftest.cypher_value_key does not
know dates).
"""
import datetime
import os
import re

import numpy as np
import pytest

from conftest import case_parts
from temporal_cases import CASES

from capf_amd import _lib, temporal as T
from capf_amd.expr import (CAPF_TO_CT, CT_TO_CAPF, OP_EQ, OP_GE, OP_GT, OP_LE, OP_LIT_INT, OP_LIT_NULL, OP_LIT_TEMPORAL,
                           OP_LT, OP_TEMPORAL_ADD, OP_TEMPORAL_FIELD, T_DATE, T_INT, T_LOCALDATETIME, TEMPORAL_FIELDS,
                           TEMPORAL_HOUR, Add, Ands, CaseExpr, Coalesce, Collect, Count, CountStar, Date, DateProperty,
                           Duration, DurationProperty, ElementProperty, Equals, GreaterThanOrEqual, In, IntegerLit,
                           LessThan, ListLit, LocalDateTime, LocalDateTimeProperty, MapExpression, Max, Min, NullLit,
                           StringLit, Subtract, Sum, TemporalProperty, Var, _compile_program, explode_values)
from capf_amd.header import RecordHeader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPOCH = datetime.date(1970, 1, 1).toordinal()
DAY_US = 86400 * 10 ** 6
ERRORS = {"IllegalArgumentException": _lib.IllegalArgumentException,
          "IllegalStateException": _lib.IllegalStateException,
          "NotImplementedException": _lib.NotImplementedException,
          "UnsupportedOperationException": _lib.UnsupportedOperationException}
DATE_FIELDS = ("year", "quarter", "month", "week", "weekYear", "dayOfQuarter", "day", "ordinalDay", "dayOfWeek")
TIME_FIELDS = ("hour", "minute", "second", "millisecond", "microsecond")


def I(v):  # noqa: E743
    return IntegerLit(v)


def M(**kw):
    return MapExpression([(k, I(v)) for k, v in kw.items()])


def rows_key(rows):
    return sorted(repr(sorted((k, type(v).__name__, v) for k, v in r.items())) for r in rows)


# ------------------------------------------------------------------- the model
def day_of(n):
    return datetime.date.fromordinal(n + EPOCH)


def m_field(v, name):
    """Field `name` of a datetime.date / datetime.datetime, from datetime's own calendar."""
    key = name.lower()
    iso = v.isocalendar()
    q0 = datetime.date(v.year, (v.month - 1) // 3 * 3 + 1, 1)
    return {"year": v.year, "quarter": (v.month - 1) // 3 + 1, "month": v.month, "week": iso[1], "weekyear": iso[0],
            "dayofquarter": v.toordinal() - q0.toordinal() + 1, "day": v.day, "ordinalday": v.timetuple().tm_yday,
            "dayofweek": v.isoweekday(), "weekday": v.isoweekday(),
            **({"hour": v.hour, "minute": v.minute, "second": v.second, "millisecond": v.microsecond // 1000,
                "microsecond": v.microsecond} if isinstance(v, datetime.datetime) else {})}[key]


def plus_months(d, months):
    """java.time's plusMonths: the day of month clamped to the target month's length, nothing else."""
    total = d.year * 12 + d.month - 1 + months
    y, m = total // 12, total % 12 + 1
    last = (datetime.date(y + m // 12, m % 12 + 1, 1) - datetime.timedelta(days=1)).day
    return d.replace(year=y, month=m, day=min(d.day, last))


def m_add(v, months, micros):
    """CAPF_OP_TEMPORAL_ADD's definition: plusMonths on the date part, then the
    microseconds — whole days of them, truncated toward zero, on a DATE."""
    if isinstance(v, datetime.datetime):
        return plus_months(v, months) + datetime.timedelta(microseconds=micros)
    return plus_months(v, months) + datetime.timedelta(days=abs(micros) // DAY_US * (1 if micros >= 0 else -1))


def m_run(prog):
    """The literal-only programs of the fixture cases, run with the model."""
    ops, ia, fa, _ = prog
    st = []
    for op, i, f in zip(ops, ia, fa):
        if op == OP_LIT_TEMPORAL:
            st.append(T.days_to_date(i) if f == T_DATE else T.micros_to_datetime(i))
        elif op == OP_LIT_NULL:
            st.append(None)
        elif op == OP_LIT_INT:
            st.append(i)
        elif op == OP_TEMPORAL_FIELD:
            v = st.pop()
            st.append(None if v is None else m_field(v, next(k for k, x in TEMPORAL_FIELDS.items() if x == i)))
        elif op == OP_TEMPORAL_ADD:
            v = st.pop()
            st.append(None if v is None else m_add(v, int(f), i))
        elif op in (OP_EQ, OP_LT, OP_LE, OP_GT, OP_GE):
            b, a = st.pop(), st.pop()
            st.append(None if a is None or b is None else
                      {OP_EQ: a == b, OP_LT: a < b, OP_LE: a <= b, OP_GT: a > b, OP_GE: a >= b}[op])
        else:
            raise AssertionError(f"opcode {op} in a fixture program")
    assert len(st) == 1
    return st[0]


def q(a, b):
    """Java's long division (the few-line model of TemporalUdfs.scala:115-150 uses it)."""
    return abs(a) // abs(b) * (1 if (a < 0) == (b < 0) else -1)


def m_duration_accessor(months, micros, name):
    days = q(micros, DAY_US)
    sub = micros - days * DAY_US
    r = lambda a, b: a - q(a, b) * b  # noqa: E731
    return {"years": q(months, 12), "quarters": q(months, 3), "months": months, "weeks": q(q(micros, DAY_US), 7),
            "days": days, "hours": q(sub, 3600 * 10 ** 6), "minutes": q(sub, 60 * 10 ** 6), "seconds": q(sub, 10 ** 6),
            "milliseconds": q(sub, 1000), "microseconds": sub, "quartersofyear": r(q(months, 3), 4),
            "monthsofquarter": r(months, 3), "monthsofyear": r(months, 12), "daysofweek": r(days, 7),
            "minutesofhour": r(q(sub, 60 * 10 ** 6), 60), "secondsofminute": r(q(sub, 10 ** 6), 60),
            "millisecondsofsecond": r(q(sub, 1000), 1000), "microsecondsofsecond": r(sub, 10 ** 6)}[name]


# --------------------------------------------------------------- CPU: the host
def _single_expr(query):
    return query.stages[0].items[0][1] if not query.matches and len(query.stages) == 1 else None


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fixture_case_on_the_host(case):
    """Every case: its constructors parse (or fail) when the program is
    compiled, and the literal-only program gives the expected value under the
    model; the UNWIND cases' lists resolve to typed values."""
    cid, src, _, query, expected, _ = case_parts(case)
    e = _single_expr(query)
    if e is None:  # UNWIND [temporal, ...] AS d RETURN min / max(d)
        t, vals = explode_values(query.matches[0].list, {})
        assert t in (T_DATE, T_LOCALDATETIME) and all(type(v) is type(expected[0]["res"]) for v in vals)
        agg = min if type(query.stages[0].items[0][1]).__name__ == "Min" else max
        assert agg(vals) == expected[0]["res"]
        return
    if isinstance(expected, tuple):
        with pytest.raises(ERRORS[expected[0]]) as err:
            _compile_program(e, None, set(), {})
        for frag in expected[1]:
            assert frag in str(err.value), (cid, src, str(err.value))
        return
    got, want = m_run(_compile_program(e, None, set(), {})), expected[0][query.stages[0].items[0][0]]
    assert type(got) is type(want) and got == want, (cid, src, got)


def test_parsers_beyond_the_fixture():
    # SMART resolving: a day of month 29..31 past the month's end is its last day; 32 is no date
    assert T.parse_date("2019-02-30") == datetime.date(2019, 2, 28) and T.parse_date("20200231") == datetime.date(2020, 2, 29)
    for bad in ("2019-02-32", "2019-13-01", "2019-366", "2015-Q5", "0000", "20101", "2010-1-1", "+2010", ""):
        with pytest.raises(_lib.IllegalArgumentException, match="valid date construction string"):
            T.parse_date(bad)
    # ISO_WEEK_DATE is strict (2015 has 53 weeks, 2016 has 52), the W formats of the builder are smart and case-insensitive
    assert T.parse_date("2015-W53-7") == datetime.date(2016, 1, 3)
    assert T.parse_date("2016w531") == datetime.date(2017, 1, 2)
    with pytest.raises(_lib.IllegalArgumentException):
        T.parse_date("2016-W53-1")
    assert T.parse_date("2020-366") == datetime.date(2020, 12, 31) and T.parse_date("2015Q192") == datetime.date(2015, 4, 2)
    # the time formats: nanoseconds parse, and are then refused below a microsecond
    assert T.parse_time_string("214032.142000001") == (21, 40, 32, 142000001)
    assert T.parse_local_datetime("2010-10-10T21:40:32.1") == datetime.datetime(2010, 10, 10, 21, 40, 32, 100000)
    with pytest.raises(_lib.IllegalStateException, match="nanosecond resolution"):
        T.parse_local_datetime("2010-10-10T21:40:32.1234567")
    for bad in ("24:00", "2140325", "21:4", "21:40:", "T"):
        with pytest.raises(_lib.IllegalArgumentException, match="valid time construction string"):
            T.parse_local_datetime("2010-10-10T" + bad)
    # maps: week / ordinal day / quarter routes, keys case-insensitive
    assert T.parse_date({"year": 2015, "week": 30, "dayOfWeek": 2}) == datetime.date(2015, 7, 21)
    assert T.parse_date({"YEAR": 2015, "ordinalDay": 202}) == datetime.date(2015, 7, 21)
    assert T.parse_date({"year": 2015, "quarter": 2, "dayOfQuarter": 60}) == datetime.date(2015, 5, 30)
    with pytest.raises(_lib.IllegalArgumentException, match="valid significance order"):
        T.parse_date({"year": 2015, "day": 3})
    # payloads round-trip at the ends of the range and before the epoch
    for v in (datetime.date(1, 1, 1), datetime.date(1969, 12, 31), datetime.date(9999, 12, 31)):
        assert T.days_to_date(T.date_to_days(v)) == v
    for v in (datetime.datetime(1, 1, 1), datetime.datetime(1969, 12, 31, 23, 59, 59, 999999),
              datetime.datetime(9999, 12, 31, 23, 59, 59, 999999)):
        assert T.micros_to_datetime(T.datetime_to_micros(v)) == v
    assert T.date_to_days(datetime.date(1969, 12, 31)) == -1
    assert T.datetime_to_micros(datetime.datetime(1969, 12, 31, 23, 59, 59, 999999)) == -1
    for bad in (T.MIN_DAY - 1, T.MAX_DAY + 1):
        with pytest.raises(_lib.IllegalStateException):
            T.days_to_date(bad)
        with pytest.raises(_lib.IllegalStateException):
            T.micros_to_datetime(bad * DAY_US)


DURATION_STRINGS = [  # TemporalTests.scala:52-93 (the host value: these results have no column type)
    ("P1Y2M20D", dict(years=1, months=2, days=20)), ("PT1S", dict(seconds=1)),
    ("PT111.123456S", dict(seconds=111, nanoseconds=123456000)), ("PT1M10S", dict(minutes=1, seconds=10)),
    ("PT3H1M10S", dict(hours=3, minutes=1, seconds=10)), ("P5DT3H1M10S", dict(days=5, hours=3, minutes=1, seconds=10)),
    ("P1W5DT3H1M10S", dict(weeks=1, days=5, hours=3, minutes=1, seconds=10)),
    ("P12M1W5DT3H1M10S", dict(months=12, weeks=1, days=5, hours=3, minutes=1, seconds=10)),
    ("P3Y12M1W5DT3H1M10S", dict(years=3, months=12, weeks=1, days=5, hours=3, minutes=1, seconds=10)),
]


def test_duration_values():
    for s, fields in DURATION_STRINGS:
        assert T.DurationValue.parse(s) == T.DurationValue.of(**fields), s
    full = dict(years=3, months=12, weeks=1, days=5, hours=3, minutes=1, seconds=10, milliseconds=10, microseconds=10)
    d = T.DurationValue.from_map({k.upper(): v for k, v in full.items()})  # (TemporalTests.scala:95-118; keys any case)
    assert (d.months, d.days, d.seconds, d.nanos) == (48, 12, 3 * 3600 + 70, 10010000)
    # toCalendarInterval: months, and everything else in microseconds (nanoseconds below one dropped)
    assert d.interval == (48, 12 * DAY_US + (3 * 3600 + 70) * 10 ** 6 + 10010)
    assert T.DurationValue.of(nanoseconds=1999).interval == (0, 1) and T.DurationValue.of(nanoseconds=-1999).interval == (0, -1)
    assert T.DurationValue.of(milliseconds=-1500).seconds == -1 and T.DurationValue.of(milliseconds=-1500).nanos == -500000000
    # duration ± duration (TemporalTests.scala:121-125, 153-161): interval arithmetic, renormalised
    p1d = T.DurationValue.parse("P1D")
    assert p1d + p1d == T.DurationValue.of(days=2) and p1d - p1d == T.DurationValue.of()
    assert p1d - T.DurationValue.parse("PT12H") == T.DurationValue.of(hours=12)
    with pytest.raises(_lib.IllegalArgumentException, match="Unsupported duration values: fortnights"):
        T.DurationValue.from_map({"days": 1, "fortnights": 2})
    for bad in ("1D", "P1H", "PT1.1234567S", "P-1D", "P1D1Y"):
        with pytest.raises(_lib.IllegalArgumentException, match="valid duration construction string"):
            T.DurationValue.parse(bad)


def test_duration_accessors_match_the_model():
    assert len(T.DURATION_ACCESSORS) == 18
    durations = [dict(years=2, months=14), dict(years=2, days=15), dict(hours=5, minutes=60), dict(milliseconds=142),
                 dict(months=-25, days=-15, hours=-30, microseconds=-1), dict(days=400, seconds=86399, microseconds=999999),
                 dict(weeks=-3, minutes=1), dict()]
    for fields in durations:
        d = T.DurationValue.of(**fields)
        months, micros = d.interval
        assert months == fields.get("years", 0) * 12 + fields.get("months", 0)
        for name in T.DURATION_ACCESSORS:
            assert d.accessor(name) == m_duration_accessor(months, micros, name), (fields, name)
            prog = _compile_program(DurationProperty(Duration(M(**fields)), name.upper()), None, set(), {})
            assert prog == ([OP_LIT_INT], [d.accessor(name)], [0.0], []), (fields, name)  # folds: an INTEGER literal
    with pytest.raises(_lib.UnsupportedOperationException, match="fortnights"):
        _compile_program(DurationProperty(Duration(StringLit("P1D")), "fortnights"), None, set(), {})
    assert _compile_program(DurationProperty(Duration(NullLit()), "years"), None, set(), {})[0] == [OP_LIT_NULL]


def test_constants_agree_between_python_header_and_scala():
    import capf_amd.expr as ex
    import okapi_scala_scan as sc
    with open(os.path.join(ROOT, "include", "capf_gpu.h")) as f:
        hdr = dict((k, int(v)) for k, v in re.findall(r"\b(CAPF_\w+) = (-?\d+)", f.read()))
    native = sc.strip_comments(sc.integration_sources()["Native.scala"])
    scala = dict((k, int(v)) for k, v in re.findall(r"final val (\w+) = (-?\d+)", native))
    camel = lambda s: "".join(w.capitalize() for w in s.split("_"))  # noqa: E731
    assert (hdr["CAPF_TYPE_DATE"], hdr["CAPF_TYPE_LOCALDATETIME"]) == (ex.T_DATE, ex.T_LOCALDATETIME) == (6, 7)
    assert (scala["TypeDate"], scala["TypeLocalDateTime"]) == (6, 7)
    for name in ("LIT_TEMPORAL", "TEMPORAL_FIELD", "TEMPORAL_ADD"):
        assert hdr["CAPF_OP_" + name] == getattr(ex, "OP_" + name) == scala["Op" + camel(name)], name
    fields = {k: v for k, v in hdr.items() if k.startswith("CAPF_TEMPORAL_")}
    assert len(fields) == 14 and sorted(fields.values()) == list(range(14))
    for k, v in fields.items():
        nm = k[len("CAPF_TEMPORAL_"):]
        assert TEMPORAL_FIELDS[nm.replace("_", "").lower()] == v == scala["Temporal" + camel(nm)], k
    assert TEMPORAL_FIELDS["weekday"] == TEMPORAL_FIELDS["dayofweek"] and TEMPORAL_HOUR == hdr["CAPF_TEMPORAL_HOUR"]
    assert CT_TO_CAPF["DATE"] == T_DATE and CT_TO_CAPF["LOCALDATETIME"] == T_LOCALDATETIME
    assert CAPF_TO_CT[T_DATE] == "DATE" and CAPF_TO_CT[T_LOCALDATETIME] == "LOCALDATETIME"
    with open(os.path.join(ROOT, "cypher-for-apache-flink_amd", "csrc", "capf_internal.h")) as f:
        internal = f.read()
    assert "Date = CAPF_TYPE_DATE" in internal and "LocalDateTime = CAPF_TYPE_LOCALDATETIME" in internal


def test_property_types_of_a_graph():
    from capf_amd.graph import _join_type, ctype_of
    assert ctype_of(datetime.date(2010, 1, 1)) == "DATE"
    assert ctype_of(datetime.datetime(2010, 1, 1, 12)) == "LOCALDATETIME"  # (datetime is a subclass of date: tested first)
    assert _join_type("DATE", "DATE") == "DATE"
    for a, b in (("DATE", "LOCALDATETIME"), ("DATE", "INTEGER"), ("LOCALDATETIME", "STRING")):
        with pytest.raises(_lib.IllegalArgumentException):
            _join_type(a, b)
    with pytest.raises(_lib.NotImplementedException):
        ctype_of([datetime.date(2010, 1, 1)])


COLS = {"d": T_DATE, "l": T_LOCALDATETIME, "k": T_INT, "s": 4}
HDR = RecordHeader({Var(c): c for c in COLS})
Dv, Lv, Kv, Sv = Var("d"), Var("l"), Var("k"), Var("s")


def compile_over_columns(e):
    return _compile_program(e, HDR, set(COLS), {}, intern=lambda s: 0, coltype=COLS.get)


def test_lowering_of_columns():
    assert compile_over_columns(DateProperty(Dv, "weekYear")) == ([1, OP_TEMPORAL_FIELD], [0, 4], [0.0, 0.0], ["d"])
    assert compile_over_columns(TemporalProperty(Lv, "MICROSECOND"))[1] == [0, 13]
    # subtraction negates both immediates; duration + temporal commutes; P1M3DT12H = (1, 3.5 days of microseconds)
    dur = Duration(StringLit("P1M3DT12H"))
    us = 3 * DAY_US + DAY_US // 2
    assert compile_over_columns(Add(Dv, dur)) == ([1, OP_TEMPORAL_ADD], [0, us], [0.0, 1.0], ["d"])
    assert compile_over_columns(Add(dur, Lv)) == ([1, OP_TEMPORAL_ADD], [0, us], [0.0, 1.0], ["l"])
    assert compile_over_columns(Subtract(Dv, dur)) == ([1, OP_TEMPORAL_ADD], [0, -us], [0.0, -1.0], ["d"])
    assert compile_over_columns(Add(Dv, Add(dur, dur)))[1:3] == ([0, 2 * us], [0.0, 2.0])  # durations fold first
    assert compile_over_columns(Add(Dv, Duration(NullLit()))) == ([OP_LIT_NULL], [T_DATE], [0.0], [])
    lit = compile_over_columns(Date(StringLit("1969-12-31")))
    assert lit == ([OP_LIT_TEMPORAL], [-1], [float(T_DATE)], [])


REJECTED = {
    "d + 1": (Add(Dv, I(1)), _lib.IllegalArgumentException),
    "1 - l": (Subtract(I(1), Lv), _lib.IllegalArgumentException),
    "duration - d": (Subtract(Duration(StringLit("P1D")), Dv), _lib.IllegalArgumentException),
    "d < 1": (LessThan(Dv, I(1)), _lib.IllegalArgumentException),
    "d < l": (LessThan(Dv, Lv), _lib.IllegalArgumentException),
    "d.hour": (DateProperty(Dv, "hour"), _lib.UnsupportedOperationException),
    "d.foo": (DateProperty(Dv, "foo"), _lib.UnsupportedOperationException),
    "k.year": (DateProperty(Kv, "year"), _lib.IllegalArgumentException),
    "date(s)": (Date(Sv), _lib.NotImplementedException),
    "date({year: k})": (Date(MapExpression([("year", Kv)])), _lib.NotImplementedException),
    "duration": (Duration(StringLit("P1D")), _lib.NotImplementedException),
    "duration + duration": (Add(Duration(StringLit("P1D")), Duration(StringLit("P1D"))), _lib.NotImplementedException),
    "duration < duration": (LessThan(Duration(StringLit("P1D")), Duration(StringLit("P2D"))), _lib.NotImplementedException),
    "d + duration(s)": (Add(Dv, Duration(Sv)), _lib.NotImplementedException),
}


@pytest.mark.parametrize("name", list(REJECTED))
def test_rejected_when_compiled(name):
    e, cls = REJECTED[name]
    with pytest.raises(cls) as err:
        compile_over_columns(e)
    assert type(err.value) is cls
    if name in ("d.hour", "d.foo"):
        assert name[2:] in str(err.value)
    if name == "date(s)":  # worded as TemporalConversions.scala:149
        assert "only supported for Literal-Maps and String literals" in str(err.value)


# ------------------------------------------------------ GPU: the fixture cases
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_case_on_gpu(gpu_session, case):
    from capf_amd.graph import ScanGraph
    from capf_amd.planner import run
    from oracle.create_parser import parse_create
    cid, src, create, query, expected, opts = case_parts(case)
    g = ScanGraph.from_data(gpu_session, parse_create(create))
    if isinstance(expected, tuple):
        with pytest.raises(ERRORS[expected[0]]) as err:
            run(g, query, opts.get("params"))
        assert all(frag in str(err.value) for frag in expected[1]), str(err.value)
        return
    got = run(g, query, opts.get("params"))
    assert rows_key(got) == rows_key(expected), f"{cid} ({src}): {got}"


# ------------------------------------------------------------ GPU: accessors
def _year_days(y0, y1):
    return range(datetime.date(y0, 1, 1).toordinal() - EPOCH, datetime.date(y1, 12, 31).toordinal() - EPOCH + 1)


RANGES = [(1970, 2369), (1, 4), (1899, 1901), (2099, 2101), (9996, 9999)]  # the first: one whole Gregorian cycle
_memo = {}


def all_days():
    if "days" not in _memo:
        _memo["days"] = np.array([n for y0, y1 in RANGES for n in _year_days(y0, y1)] + [-1], dtype=np.int64)
    return _memo["days"]


def project(t, header, items):
    out = t.withColumns(*[(e, c) for c, e in items], header=header, params={})
    return {c: out.column_arrays(c) for c, _ in items}, out


@pytest.mark.gpu
def test_date_accessors_over_a_gregorian_cycle(gpu_session):
    days = all_days()
    assert len(days) > 146097 and days[0] == 0 and -1 in days
    valid = (np.arange(len(days)) % 7 != 6).astype(np.uint8)  # every 7th row NULL
    t = gpu_session.table([("d", T_DATE, days, valid)])
    got, out = project(t, RecordHeader({Dv: "d"}), [(f, DateProperty(Dv, f)) for f in DATE_FIELDS])
    assert all(out.columnType[f] == "INTEGER" for f in DATE_FIELDS) and out.columnType["d"] == "DATE"
    want = np.array([[m_field(v, f) for f in DATE_FIELDS] for v in map(day_of, days.tolist())], dtype=np.int64)
    for j, f in enumerate(DATE_FIELDS):
        vals, ok = got[f]
        assert np.array_equal(ok, valid.astype(bool)), f
        bad = np.nonzero(ok & (vals != want[:, j]))[0]
        assert len(bad) == 0, (f, [(str(day_of(int(days[i]))), int(vals[i]), int(want[i, j])) for i in bad[:5]])
    # the days where a wrong formula shows are among them
    at = {str(day_of(int(n))): i for i, n in enumerate(days.tolist())}
    for day, field, value in (("1969-12-31", "dayOfWeek", 3), ("1900-03-01", "ordinalDay", 60), ("2000-02-29", "day", 29),
                              ("2018-12-31", "week", 1), ("2018-12-31", "weekYear", 2019), ("2021-01-03", "week", 53),
                              ("2021-01-03", "weekYear", 2020), ("2015-12-31", "week", 53), ("2010-01-03", "week", 53),
                              ("2010-01-03", "weekYear", 2009), ("1900-02-28", "dayOfQuarter", 59)):
        assert want[at[day], DATE_FIELDS.index(field)] == value, (day, field)


@pytest.mark.gpu
def test_localdatetime_accessors(gpu_session):
    days = np.concatenate([all_days()[:-1][::97], [-1]])
    tods = [0, ((12 * 60 + 34) * 60 + 56) * 10 ** 6 + 789012, DAY_US - 1]
    us = np.array([n * DAY_US + tod for n in days.tolist() for tod in tods], dtype=np.int64)
    assert -1 in us  # 1969-12-31T23:59:59.999999
    valid = (np.arange(len(us)) % 7 != 6).astype(np.uint8)
    t = gpu_session.table([("l", T_LOCALDATETIME, us, valid)])
    fields = DATE_FIELDS + TIME_FIELDS
    got, _ = project(t, RecordHeader({Lv: "l"}), [(f, LocalDateTimeProperty(Lv, f)) for f in fields])
    values = [T.micros_to_datetime(v) for v in us.tolist()]
    for f in fields:
        vals, ok = got[f]
        assert np.array_equal(ok, valid.astype(bool)), f
        want = np.array([m_field(v, f) for v in values], dtype=np.int64)
        bad = np.nonzero(ok & (vals != want))[0]
        assert len(bad) == 0, (f, [(str(values[i]), int(vals[i]), int(want[i])) for i in bad[:5]])


# ------------------------------------------------- GPU: addition, subtraction
MONTHS = (-1200, -25, -13, -12, -1, 0, 1, 11, 12, 13, 1200)
DAYS = (-366, -1, 0, 1, 365)
HOURS = (0, 12, -12)


def month_ends():
    out = []
    for y in (1999, 2000, 2001, 2002, 2003, 2004, 2100):
        for m in range(1, 13):
            last = (plus_months(datetime.date(y, m, 1), 1) - datetime.timedelta(days=1)).day
            out += [datetime.date(y, m, dd) for dd in range(28, last + 1)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ctype", ["DATE", "LOCALDATETIME"])
def test_plus_and_minus_duration(gpu_session, ctype):
    dates = month_ends()
    if ctype == "DATE":
        values = dates + [None]
    else:  # the three times of day of the accessor test
        values = [datetime.datetime(d.year, d.month, d.day, *hms) for d in dates
                  for hms in ((0, 0, 0, 0), (12, 34, 56, 789012), (23, 59, 59, 999999))][::2] + [None]
    v = Var("v")
    t = gpu_session.table([("v", CT_TO_CAPF[ctype], values, None)])
    items, want = [], {}
    for mo in MONTHS:
        for dd in DAYS:
            for hh in HOURS:
                dur = Duration(M(months=mo, days=dd, hours=hh))
                micros = dd * DAY_US + hh * 3600 * 10 ** 6
                for sign, cls in ((1, Add), (-1, Subtract)):
                    name = f"c{len(items)}"
                    items.append((name, cls(v, dur)))
                    want[name] = [None if x is None else m_add(x, sign * mo, sign * micros) for x in values]
    out = t.withColumns(*[(e, c) for c, e in items], header=RecordHeader({v: "v"}), params={})
    assert set(out.columnType.values()) == {ctype}
    for name, e in items:
        got = out.column_values(name)
        assert got == want[name], (str(e), next((a, b, c) for a, b, c in zip(values, got, want[name]) if b != c))
    if ctype == "DATE":  # sub-day parts are dropped, truncating toward zero: P1DT12H moves one day, either way
        d0 = [datetime.date(2010, 10, 10)]
        t1 = gpu_session.table([("v", T_DATE, d0, None)])
        h = RecordHeader({v: "v"})
        p = Duration(StringLit("P1DT12H"))
        n = Duration(M(days=-1, hours=-12))
        got = t1.withColumns((Subtract(v, p), "a"), (Add(v, p), "b"), (Add(v, n), "c"), (Subtract(v, n), "e"),
                             (Add(p, v), "f"), header=h, params={}).rows[0]
        assert (got["a"], got["b"], got["c"], got["e"], got["f"]) == (
            datetime.date(2010, 10, 9), datetime.date(2010, 10, 11), datetime.date(2010, 10, 9),
            datetime.date(2010, 10, 11), datetime.date(2010, 10, 11))


# ------------------------------------------- GPU: the type through int64 paths
N_ROWS = 1000


def paths_table(sess):
    """~1000 rows: a DATE with duplicates, NULLs and pre-epoch values, the same
    payloads as an INTEGER, a LOCALDATETIME, and the row number."""
    rng = np.random.default_rng(11)
    pool = np.concatenate([rng.integers(-30000, 30000, 120), [-1, 0, 1, T.MIN_DAY, T.MAX_DAY]])
    days = pool[rng.integers(0, len(pool), N_ROWS)]
    dvalid = (rng.integers(0, 10, N_ROWS) != 0).astype(np.uint8)
    us = days * DAY_US + rng.integers(0, DAY_US, N_ROWS)
    lvalid = (rng.integers(0, 13, N_ROWS) != 0).astype(np.uint8)
    t = sess.table([("d", T_DATE, days, dvalid), ("di", T_INT, days, dvalid), ("l", T_LOCALDATETIME, us, lvalid),
                    ("i", T_INT, np.arange(N_ROWS, dtype=np.int64), None)])
    d = [day_of(int(x)) if ok else None for x, ok in zip(days, dvalid)]
    ls = [T.micros_to_datetime(int(x)) if ok else None for x, ok in zip(us, lvalid)]
    return t, d, ls, RecordHeader({Var(c): c for c in ("d", "di", "l", "i")})


@pytest.mark.gpu
def test_upload_forms_and_download(gpu_session):
    vals = [datetime.date(1969, 12, 31), None, datetime.date(2020, 2, 29)]
    lv = [datetime.datetime(1969, 12, 31, 23, 59, 59, 999999), datetime.datetime(2020, 2, 29, 1, 2, 3, 4), None]
    t = gpu_session.table([("d", T_DATE, vals, None), ("l", T_LOCALDATETIME, lv, None)])
    assert t.columnType == {"d": "DATE", "l": "LOCALDATETIME"}
    assert t.column_values("d") == vals and t.column_values("l") == lv
    assert type(t.column_values("l")[0]) is datetime.datetime and type(t.column_values("d")[0]) is datetime.date
    assert t.column_arrays("d")[0].tolist() == [-1, 0, 18321]
    d64 = np.array(["1969-12-31", "2020-02-29"], dtype="datetime64[D]")
    l64 = np.array(["1969-12-31T23:59:59.999999", "2020-02-29T01:02:03.000004"], dtype="datetime64[us]")
    t2 = gpu_session.table([("d", T_DATE, d64, None), ("l", T_LOCALDATETIME, l64, None),
                            ("d2", T_DATE, np.array([-1, 18321], dtype=np.int64), None)])
    assert t2.column_values("d") == t2.column_values("d2") == [vals[0], vals[2]]
    assert t2.column_values("l") == lv[:2]
    with pytest.raises(_lib.IllegalArgumentException):
        gpu_session.table([("d", T_DATE, [datetime.datetime(2020, 1, 1)], None)])
    far = gpu_session.table([("d", T_DATE, np.array([T.MAX_DAY + 1], dtype=np.int64), None)])
    with pytest.raises(_lib.IllegalStateException):
        far.column_values("d")


@pytest.mark.gpu
def test_order_distinct_skip_limit_and_encodings(gpu_session):
    t, d, ls, h = paths_table(gpu_session)
    for o in ("asc", "desc"):
        got = t.orderBy((Dv, o), header=h, params={})
        assert got.columnType["d"] == "DATE" and got.columnType["l"] == "LOCALDATETIME"
        # the INTEGER path: the same permutation as the same payloads typed INTEGER
        assert got.column_values("i") == t.orderBy((Var("di"), o), header=h, params={}).column_values("i")
        seq = [x for x in got.column_values("d") if x is not None]
        assert seq == sorted((x for x in d if x is not None), reverse=o == "desc")
        assert got.column_values("d") == [d[i] for i in got.column_values("i")]
        lo = t.orderBy((Lv, o), header=h, params={}).column_values("l")
        assert [x for x in lo if x is not None] == sorted((x for x in ls if x is not None), reverse=o == "desc")
    top = t.orderBy((Dv, "asc"), header=h, params={}).skip(5).limit(300)
    assert top.columnType["d"] == "DATE" and top.size == 300
    dist = t.select("d").distinct()
    assert dist.columnType == {"d": "DATE"}
    got = dist.column_values("d")
    assert len(got) == len(set(d)) and set(got) == set(d)
    for width in (4, 3):  # the FOR encodings apply by the INTEGER rules and keep type and values
        c = t.select("d", "di", "i").compact(width)
        assert c.columnType["d"] == "DATE" and c.encoding("d") == c.encoding("di")
        assert c.column_values("d") == d
        assert c.filter(GreaterThanOrEqual(Dv, Date(StringLit("2000-01-01"))), header=h, params={}).size == \
            sum(1 for x in d if x is not None and x >= datetime.date(2000, 1, 1))


@pytest.mark.gpu
def test_group_by_a_date_key(gpu_session):
    t, d, ls, h = paths_table(gpu_session)
    g = t.select("d", "l").group([Dv], {"n": CountStar(), "c": Count(Lv), "lo": Min(Lv), "hi": Max(Lv), "dd": Count(Dv, True)},
                                 header=h, params={})
    assert g.columnType == {"d": "DATE", "n": "INTEGER", "c": "INTEGER", "lo": "LOCALDATETIME", "hi": "LOCALDATETIME",
                            "dd": "INTEGER"}
    want = {}
    for k, v in zip(d, ls):
        w = want.setdefault(k, {"d": k, "n": 0, "c": 0, "lo": None, "hi": None, "dd": 0 if k is None else 1})
        w["n"] += 1
        if v is not None:
            w["c"] += 1
            w["lo"] = v if w["lo"] is None else min(w["lo"], v)
            w["hi"] = v if w["hi"] is None else max(w["hi"], v)
    assert rows_key(g.rows) == rows_key(list(want.values()))
    whole = t.group([], {"lo": Min(Dv), "hi": Max(Dv), "n": Count(Dv), "u": Count(Dv, True)}, header=h, params={})
    nn = [x for x in d if x is not None]
    assert whole.rows == [{"lo": min(nn), "hi": max(nn), "n": len(nn), "u": len(set(nn))}]
    assert whole.columnType["lo"] == "DATE"


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["default", "hash", "radix"])
def test_inner_join_on_a_date_key(gpu_session, monkeypatch, route):
    if route != "default":
        monkeypatch.setenv("CAPF_JOIN", route)
    t, d, _, _ = paths_table(gpu_session)
    keys = sorted({x for x in d if x is not None})[::3]  # a unique build side (dense route: days in a narrow range)
    r = gpu_session.table([("rd", T_DATE, keys, None), ("j", T_INT, np.arange(len(keys), dtype=np.int64), None)])
    got = t.select("d", "i").join(r, "inner", ("d", "rd"))
    assert got.columnType["d"] == "DATE" and got.columnType["rd"] == "DATE"
    at = {k: j for j, k in enumerate(keys)}
    want = [{"d": x, "i": i, "rd": x, "j": at[x]} for i, x in enumerate(d) if x in at]
    assert rows_key(got.rows) == rows_key(want)
    with pytest.raises(_lib.IllegalArgumentException):  # equal-typed keys only
        t.select("d", "i").join(r.select(("j", "rd2")), "inner", ("d", "rd2")).size


@pytest.mark.gpu
def test_union_filter_in_coalesce_case(gpu_session):
    t, d, ls, h = paths_table(gpu_session)
    u = t.select("d").unionAll(t.select("d"))
    assert u.columnType == {"d": "DATE"} and u.column_values("d") == d + d
    with pytest.raises(_lib.CypherException):
        t.select("d").unionAll(t.select(("l", "d"))).size
    # WHERE d >= date('2000-01-01') AND d.year < 2010
    f = t.filter(Ands(GreaterThanOrEqual(Dv, Date(StringLit("2000-01-01"))), LessThan(DateProperty(Dv, "year"), I(2010))),
                 header=h, params={})
    assert f.columnType["d"] == "DATE"
    assert f.column_values("i") == [i for i, x in enumerate(d) if x is not None and datetime.date(2000, 1, 1) <= x
                                    and x.year < 2010]
    present = sorted({x for x in d if x is not None})
    for k in (3, 20):  # a short OR chain, and a session set (CAPF_OP_IN_SET)
        lits = present[:: max(len(present) // k, 1)][:k - 1] + [datetime.date(1234, 5, 6)]
        assert len(lits) == k
        e = In(Dv, ListLit(*[Date(StringLit(x.isoformat())) for x in lits]))
        got = t.withColumns((e, "z"), header=h, params={}).column_values("z")
        assert got == [None if x is None else x in lits for x in d], k
        with_null = In(Dv, ListLit(*([Date(StringLit(x.isoformat())) for x in lits] + [Date(NullLit())])))
        got = t.withColumns((with_null, "z"), header=h, params={}).column_values("z")
        assert got == [None if x is None or x not in lits else True for x in d], k
    first = [v for v in ls if v is not None][:20]
    lsel = In(Lv, ListLit(*[LocalDateTime(StringLit(x.isoformat())) for x in first]))
    assert t.filter(lsel, header=h, params={}).column_values("i") == [i for i, x in enumerate(ls) if x in first]
    fallback = datetime.date(1, 1, 1)
    out = t.withColumns((Coalesce(Dv, Date(StringLit("0001-01-01"))), "c"),
                        (CaseExpr([(LessThan(Dv, Date(StringLit("1970-01-01"))), Date(StringLit("1970-01-01")))], Dv), "w"),
                        (CaseExpr([(LessThan(DateProperty(Lv, "hour"), I(12)), Lv)]), "m"), header=h, params={})
    assert (out.columnType["c"], out.columnType["w"], out.columnType["m"]) == ("DATE", "DATE", "LOCALDATETIME")
    assert out.column_values("c") == [fallback if x is None else x for x in d]
    assert out.column_values("w") == [None if x is None else max(x, datetime.date(1970, 1, 1)) for x in d]
    assert out.column_values("m") == [x if x is not None and x.hour < 12 else None for x in ls]


@pytest.mark.gpu
def test_graph_properties_and_element_property(gpu_session):
    from capf_amd.graph import GraphData, ScanGraph
    from capf_amd.planner import Match, NodeP, Query, Stage, run
    born = [datetime.date(1969, 12, 31), datetime.date(2000, 2, 29), None]
    seen = [datetime.datetime(2019, 5, 10, 10, 10, 12, 113114), None, datetime.datetime(1969, 12, 31, 23, 59, 59, 999999)]
    data = GraphData(nodes=[(i, frozenset(["P"]), {k: v for k, v in (("born", b), ("seen", s)) if v is not None})
                            for i, (b, s) in enumerate(zip(born, seen))])
    g = ScanGraph.from_data(gpu_session, data)
    n = Var("n", "NODE")
    b, s = ElementProperty(n, "born", "DATE"), ElementProperty(n, "seen", "LOCALDATETIME")
    q = Query([Match([NodeP("n", ["P"])])],
              [Stage([("b", b), ("y", DateProperty(b, "year")), ("us", LocalDateTimeProperty(s, "microsecond")),
                      ("next", Add(b, Duration(StringLit("P1M"))))])])
    want = [{"b": x, "y": None if x is None else x.year, "us": None if y is None else y.microsecond,
             "next": None if x is None else plus_months(x, 1)} for x, y in zip(born, seen)]
    assert rows_key(run(g, q)) == rows_key(want)


GPU_REJECTED = {
    "d = 1": (lambda t, h: t.filter(Equals(Dv, I(1)), header=h, params={}), _lib.IllegalArgumentException),
    "d < 1": (lambda t, h: t.filter(LessThan(Dv, I(1)), header=h, params={}), _lib.IllegalArgumentException),
    "d = l": (lambda t, h: t.filter(Equals(Dv, Lv), header=h, params={}), _lib.IllegalArgumentException),
    "d + 1": (lambda t, h: t.withColumns((Add(Dv, I(1)), "z"), header=h, params={}), _lib.IllegalArgumentException),
    "sum(d)": (lambda t, h: t.group([], {"z": Sum(Dv)}, header=h, params={}), _lib.IllegalArgumentException),
    "collect(d)": (lambda t, h: t.group([], {"z": Collect(Dv)}, header=h, params={}), _lib.NotImplementedException),
    "[d]": (lambda t, h: t.withColumns((ListLit(Dv), "z"), header=h, params={}), _lib.NotImplementedException),
    "d.hour": (lambda t, h: t.withColumns((DateProperty(Dv, "hour"), "z"), header=h, params={}),
               _lib.UnsupportedOperationException),
    "d.foo": (lambda t, h: t.withColumns((DateProperty(Dv, "foo"), "z"), header=h, params={}),
              _lib.UnsupportedOperationException),
    "date(n.s)": (lambda t, h: t.withColumns((Date(Var("i")), "z"), header=h, params={}), _lib.NotImplementedException),
    "duration": (lambda t, h: t.withColumns((Duration(StringLit("P1D")), "z"), header=h, params={}),
                 _lib.NotImplementedException),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GPU_REJECTED))
def test_rejected_on_a_table(gpu_session, name):
    t, _, _, h = paths_table(gpu_session)
    fn, cls = GPU_REJECTED[name]
    with pytest.raises(cls) as err:
        fn(t, h).size
    assert type(err.value) is cls, err.value


def test_csv_source_refuses_temporal_values():
    from capf_amd.fs_source import _format_field
    for v in (datetime.date(2010, 1, 1), datetime.datetime(2010, 1, 1, 12)):
        with pytest.raises(_lib.NotImplementedException):
            _format_field(v)


def test_accessor_over_an_aggregate_is_split_like_any_projection():
    from capf_amd.expr import aggregators_in
    assert aggregators_in(DateProperty(Min(Dv), "year")) == [Min(Dv)]
