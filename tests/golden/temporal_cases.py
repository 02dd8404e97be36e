"""Temporal cases transcribed from the shared acceptance suite:
morpheus-testing/.../acceptance/TemporalTests.scala (TT) and the date /
localdatetime MIN / MAX cases of AggregationTests.scala (AT) :353, :361, :458,
:466.  Same format as list_function_cases.py — id, source lines, CREATE, Query,
expected rows — except that an expected error is (exception class name,
message fragments).  Expected values are datetime.date / datetime.datetime
(java.time.LocalDate / LocalDateTime in the source).  The okapi IR is Date /
LocalDateTime / Duration (okapi-ir/.../ir/api/expr/Expr.scala:1258-1277),
DateProperty / LocalDateTimeProperty / DurationProperty (:487-507) and Add /
Subtract with a CTDuration side (:544-548).  Each string of the two parse
tables (TT:207-226, :300-327) is a case of its own.

Left out, because the result column would be a DURATION (there is no such
column type):
  TT:52-93   "parses cypher compatible duration strings"
  TT:95-118  "constructs duration from a map"
  TT:121-125 "supports addition to duration"
  TT:153-161 "supports subtraction to duration"
  TT:732-738 "supports nanoseconds" (`ignore`d in the source)
  AT:369-375, :474-480 min / max on durations; AT:377-…, :482-… the
  mixed-type and duration aggregates around them.
TT:168-176 binds the date and the duration with WITH before subtracting; a WITH
variable cannot hold a duration here, so the case is transcribed with both
inlined (`sub_date_from_maps`).  The two "current date" cases (TT:280-287,
:407-414) compare this import's date / date-time with the constructor's, read
when the query is compiled: `<=` holds.
"""
import datetime

import capf_import  # noqa: F401
from capf_amd.expr import (Add, Date, DateProperty, Duration, DurationProperty, GreaterThan, IntegerLit,
                           LessThan, LessThanOrEqual, ListLit, LocalDateTime, LocalDateTimeProperty, MapExpression, Max,
                           Min, NullLit, StringLit, Subtract, Var)
from capf_amd.planner import Query, Stage, Unwind

TT = "MTa/TemporalTests.scala:"
AT = "MTa/AggregationTests.scala:"
NL = NullLit()
IAE, ISE, UOE = "IllegalArgumentException", "IllegalStateException", "UnsupportedOperationException"


def D(s):
    return Date(StringLit(s))


def L(s):
    return LocalDateTime(StringLit(s))


def DUR(s):
    return Duration(StringLit(s))


def M(**kw):
    return MapExpression([(k, StringLit(v) if isinstance(v, str) else IntegerLit(v)) for k, v in kw.items()])


def d(s):
    return datetime.date.fromisoformat(s)


def ldt(s):
    return datetime.datetime.fromisoformat(s)


def _unit(name, e):
    return Query([], [Stage([(name, e)])])


def _agg(items, agg):
    # UNWIND [<items>] AS d RETURN agg(d) AS res (over the empty graph)
    return Query([Unwind(ListLit(*items), "d")], [Stage([("res", agg(Var("d")))])])


DATE_STRINGS = [  # TT:208-223
    ("2010-10-10", "2010-10-10"), ("20101010", "2010-10-10"), ("2010-12", "2010-12-01"), ("201012", "2010-12-01"),
    ("2015-W30-2", "2015-07-21"), ("2015W302", "2015-07-21"), ("2015-W30", "2015-07-20"), ("2015W30", "2015-07-20"),
    ("2015-Q2-60", "2015-05-30"), ("2015Q260", "2015-05-30"), ("2015-Q2", "2015-04-01"), ("2015Q2", "2015-04-01"),
    ("2015-202", "2015-07-21"), ("2015202", "2015-07-21"), ("2010", "2010-01-01"),
]
TIME_STRINGS = [  # TT:317-323
    ("2010-10-10T21:40:32.142", "2010-10-10T21:40:32.142"), ("2010-10-10T214032.142", "2010-10-10T21:40:32.142"),
    ("2010-10-10T21:40:32", "2010-10-10T21:40:32"), ("2010-10-10T214032", "2010-10-10T21:40:32"),
    ("2010-10-10T21:40", "2010-10-10T21:40:00"), ("2010-10-10T2140", "2010-10-10T21:40:00"),
    ("2010-10-10T21", "2010-10-10T21:00:00"),
]
TODAY = datetime.date.today().isoformat()
NOW = datetime.datetime.now().isoformat()


def _accessor(name, date_s, ldt_s, value, lines):
    a, b = lines
    return [
        (f"{name}_date", TT + a, "", _unit(name, DateProperty(D(date_s), name)), [{name: value}]),
        (f"{name}_localdatetime", TT + b, "", _unit(name, LocalDateTimeProperty(L(ldt_s), name)), [{name: value}]),
    ]


def _time_accessor(name, ldt_s, value, lines):
    return (f"{name}_localdatetime", TT + lines, "", _unit(name, LocalDateTimeProperty(L(ldt_s), name)),
            [{name: value}])


def _duration_accessor(name, alias, m, value, lines):
    return (f"duration_{name}", TT + lines, "", _unit(alias, DurationProperty(Duration(M(**m)), name)),
            [{alias: value}])


CASES = [
    # ---- duration arithmetic on dates and date-times
    ("add_date", TT + "127-131", "", _unit("time", Add(D("2010-10-10"), DUR("P1D"))), [{"time": d("2010-10-11")}]),
    ("add_date_time_part", TT + "133-137", "", _unit("time", Add(D("2010-10-10"), DUR("P1DT12H"))),
     [{"time": d("2010-10-11")}]),
    ("add_localdatetime", TT + "139-143", "", _unit("time", Add(L("2010-10-10T12:00"), DUR("P1D"))),
     [{"time": ldt("2010-10-11T12:00:00")}]),
    ("add_localdatetime_time_part", TT + "145-149", "", _unit("time", Add(L("2010-10-10T12:00"), DUR("P1DT12H"))),
     [{"time": ldt("2010-10-12T00:00:00")}]),
    ("sub_date", TT + "163-166", "", _unit("time", Subtract(D("2010-10-10"), DUR("P1D"))),
     [{"time": d("2010-10-09")}]),
    # WITH date({…}) AS date, duration({…}) AS duration RETURN date - duration AS diff: inlined (see above)
    ("sub_date_from_maps", TT + "168-176", "",
     _unit("diff", Subtract(Date(M(year=1984, month=10, day=11)), Duration(M(months=1, days=-14)))),
     [{"diff": d("1984-09-25")}]),
    ("sub_date_time_part", TT + "179-183", "", _unit("time", Subtract(D("2010-10-10"), DUR("P1DT12H"))),
     [{"time": d("2010-10-09")}]),
    ("sub_localdatetime", TT + "185-189", "", _unit("time", Subtract(L("2010-10-10T12:00"), DUR("P1D"))),
     [{"time": ldt("2010-10-09T12:00:00")}]),
    ("sub_localdatetime_time_part", TT + "191-195", "", _unit("time", Subtract(L("2010-10-10T12:00"), DUR("P1DT12H"))),
     [{"time": ldt("2010-10-09T00:00:00")}]),
    # ---- date
    ("date_valid", TT + "201-205", "", _unit("time", D("2010-10-10")), [{"time": d("2010-10-10")}]),
] + [
    (f"date_parse_{given}", TT + "207-226", "", _unit("time", D(given)), [{"time": d(want)}])
    for given, want in DATE_STRINGS
] + [
    ("date_map_ymd", TT + "229-231", "", _unit("time", Date(M(year=2010, month=10, day=10))),
     [{"time": d("2010-10-10")}]),
    ("date_map_ym", TT + "233-235", "", _unit("time", Date(M(year=2010, month=10))), [{"time": d("2010-10-01")}]),
    ("date_map_string_year", TT + "237-239", "", _unit("time", Date(M(year="2010"))), [{"time": d("2010-01-01")}]),
    ("date_map_order_year_day", TT + "243-245", "", _unit("time", Date(M(year=2018, day=356))),
     (IAE, ("valid significance order", "year, day"))),
    ("date_map_no_year_month_day", TT + "247-249", "", _unit("time", Date(M(month=11, day=2))),
     (IAE, ("`year` needs to be set", "month, day"))),
    ("date_map_no_year_day", TT + "251-253", "", _unit("time", Date(M(day=2))),
     (IAE, ("`year` needs to be set", "day"))),
    ("date_wrong_dashes", TT + "257-259", "", _unit("time", D("2018-10-10-10")),
     (IAE, ("valid date construction string", "2018-10-10-10"))),
    ("date_wrong_digits", TT + "261-263", "", _unit("time", D("201810101")),
     (IAE, ("valid date construction string", "201810101"))),
    ("date_less_than", TT + "267-271", "", _unit("time", LessThan(D("2015-10-10"), D("2015-10-12"))), [{"time": True}]),
    ("date_greater_than", TT + "273-277", "", _unit("time", GreaterThan(D("2015-10-10"), D("2015-10-12"))),
     [{"time": False}]),
    ("date_current", TT + "280-287", "", _unit("time", LessThanOrEqual(D(TODAY), Date())), [{"time": True}]),
    ("date_null", TT + "289-295", "", _unit("time", Date(NL)), [{"time": None}]),
    # ---- localdatetime
] + [
    (f"localdatetime_parse_{given}", TT + "300-327", "", _unit("time", L(given)), [{"time": ldt(want)}])
    for given, want in [(g, w + "T00:00:00") for g, w in DATE_STRINGS] + TIME_STRINGS
] + [
    ("localdatetime_map_millis", TT + "330-342", "",
     _unit("time", LocalDateTime(M(year=2015, month=10, day=12, hour=12, minute=50, second=35, millisecond=556))),
     [{"time": ldt("2015-10-12T12:50:35.556")}]),
    ("localdatetime_map_minutes", TT + "344-354", "",
     _unit("time", LocalDateTime(M(year=2015, month=10, day=1, hour=12, minute=50))),
     [{"time": ldt("2015-10-01T12:50:00")}]),
    ("localdatetime_map_nanosecond", TT + "357-369", "",
     _unit("time", LocalDateTime(M(year=2015, month=10, day=1, hour=12, minute=50, second=1, nanosecond=42))),
     (ISE, ("nanosecond resolution",))),
    ("localdatetime_map_order_minute", TT + "372-373", "", _unit("time", LocalDateTime(M(year=2011, minute=50))),
     (IAE, ("valid significance order", "minute"))),
    ("localdatetime_map_order_second", TT + "375-376", "",
     _unit("time", LocalDateTime(M(year=2018, hour=12, second=14))),
     (IAE, ("valid significance order", "year, hour, second"))),
    ("localdatetime_wrong_colons", TT + "380-382", "", _unit("time", L("2018-10-10T12:10:30:15")),
     (IAE, ("valid time construction string", "12:10:30:15"))),
    ("localdatetime_wrong_digits", TT + "384-386", "", _unit("time", L("20181010T1210301")),
     (IAE, ("valid time construction string", "1210301"))),
    ("localdatetime_wrong_date", TT + "388-390", "", _unit("time", L("20181010123123T12:00")),
     (IAE, ("valid date construction string", "20181010123123"))),
    ("localdatetime_less_than", TT + "394-398", "",
     _unit("time", LessThan(L("2015-10-10T00:00:00"), L("2015-10-12T00:00:00"))), [{"time": True}]),
    ("localdatetime_greater_than", TT + "400-404", "",
     _unit("time", GreaterThan(L("2015-10-10T00:00:00"), L("2015-10-12T00:00:00"))), [{"time": False}]),
    ("localdatetime_current", TT + "407-414", "", _unit("time", LessThanOrEqual(L(NOW), LocalDateTime())),
     [{"time": True}]),
    ("localdatetime_null", TT + "416-422", "", _unit("time", LocalDateTime(NL)), [{"time": None}]),
    # ---- accessors
    ("accessor_null_date", TT + "427-431", "", _unit("year", DateProperty(Date(NL), "year")), [{"year": None}]),
    ("accessor_null_localdatetime", TT + "433-437", "", _unit("year", LocalDateTimeProperty(LocalDateTime(NL), "year")),
     [{"year": None}]),
    ("accessor_unknown", TT + "440-444", "", _unit("foo", DateProperty(Date(), "foo")), (UOE, ("foo",))),
] + _accessor("year", "2015-10-10", "2015-10-10T10:10", 2015, ("447-453", "455-461")) \
  + _accessor("quarter", "2015-10-10", "2015-10-10T10:10", 4, ("465-471", "473-479")) \
  + _accessor("month", "2015-10-10", "2015-10-10T10:10", 10, ("483-489", "491-497")) \
  + _accessor("week", "2019-01-01", "2019-01-01T10:10", 1, ("501-507", "509-515")) \
  + _accessor("weekYear", "1813-01-01", "1813-01-01T10:10", 1812, ("519-525", "527-533")) \
  + _accessor("dayOfQuarter", "2019-01-01", "2019-01-01T10:10", 1, ("537-543", "545-551")) \
  + _accessor("day", "2019-05-10", "2019-05-10T10:10", 10, ("555-561", "563-569")) \
  + _accessor("ordinalDay", "2019-05-10", "2019-05-10T10:10", 130, ("573-579", "581-587")) \
  + _accessor("dayOfWeek", "2019-05-10", "2019-05-10T10:10", 5, ("591-597", "599-605")) + [
    _time_accessor("hour", "2019-05-10T10:10", 10, "609-615"),
    _time_accessor("minute", "2019-05-10T10:11", 11, "619-625"),
    _time_accessor("second", "2019-05-10T10:10:12", 12, "629-635"),
    _time_accessor("millisecond", "2019-05-10T10:10:12.113", 113, "639-645"),
    _time_accessor("microsecond", "2019-05-10T10:10:12.113114", 113114, "649-655"),
    _duration_accessor("years", "years", dict(years=2, months=14), 3, "659-665"),
    _duration_accessor("months", "months", dict(years=2, months=14), 38, "667-673"),
    _duration_accessor("weeks", "weeks", dict(years=2, days=15), 2, "675-681"),
    _duration_accessor("days", "days", dict(years=2, days=14), 14, "683-689"),
    _duration_accessor("hours", "hours", dict(years=2, hours=5, minutes=60), 6, "691-697"),
    _duration_accessor("minutes", "minutes", dict(years=2, hours=2, minutes=2), 122, "699-705"),
    _duration_accessor("seconds", "seconds", dict(years=2, minutes=1, seconds=2), 62, "707-713"),
    _duration_accessor("milliseconds", "millis", dict(years=2, milliseconds=142), 142, "715-721"),
    _duration_accessor("microseconds", "micros", dict(years=2, microseconds=142), 142, "723-729"),
    ("duration_null", TT + "740-746", "", _unit("years", DurationProperty(Duration(NL), "years")), [{"years": None}]),
    # ---- MIN / MAX
    ("min_dates", AT + "353-359", "", _agg([D("2018-01-01"), D("2019-01-01")], Min), [{"res": d("2018-01-01")}]),
    ("min_localdatetimes", AT + "361-367", "", _agg([L("2010-10-10T12:00"), L("2010-10-10T12:01")], Min),
     [{"res": ldt("2010-10-10T12:00")}]),
    ("max_dates", AT + "458-464", "", _agg([D("2018-01-01"), D("2019-01-01")], Max), [{"res": d("2019-01-01")}]),
    ("max_localdatetimes", AT + "466-472", "", _agg([L("2010-10-10T12:00"), L("2010-10-10T12:01")], Max),
     [{"res": ldt("2010-10-10T12:01")}]),
]
assert len(CASES) == 111, len(CASES)
assert len({c[0] for c in CASES}) == len(CASES)
