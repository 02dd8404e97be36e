"""Temporal values on the host: the DATE / LOCALDATETIME payloads, the
constructor parsers and the duration value.

A DATE column holds days since 1970-01-01, a LOCALDATETIME column microseconds
since 1970-01-01T00:00:00 (both int64, negative before the epoch; no time
zone, no nanoseconds — TemporalConversions.scala:98-107).  Constructor
arguments are resolved when a program is compiled, as the Morpheus lowering
does (TemporalConversions.scala:123-151); the parsers restate

 * okapi-api/.../impl/temporal/TemporalTypesHelper.scala:51-150 — the 15 date
   and 8 time formats, tried in that order, with java.time's parsing rules
   (fixed digit counts, SMART resolving: a day of month 29..31 past the
   month's end is its last day; ISO_WEEK_DATE and ISO_LOCAL_TIME are STRICT);
 * :184-280 — parseDateMap / parseTimeMap, their significance-order and
   missing-year errors;
 * okapi-api/.../impl/temporal/Duration.scala:108-194 — Duration.apply(map) and
   Duration.parse, the double-based fraction split included.

There is no DURATION column type: a duration folds on the host (its accessors,
duration ± duration) or becomes the (months, microseconds) immediate of
CAPF_OP_TEMPORAL_ADD — `DurationValue.interval`, toCalendarInterval of
TemporalConversions.scala:54-67.
"""
import datetime
import math
import re

EPOCH = datetime.date(1970, 1, 1)
EPOCH_ORDINAL = EPOCH.toordinal()
MICROS_PER_SECOND = 1000000
MICROS_PER_DAY = 86400 * MICROS_PER_SECOND
MIN_DAY = datetime.date.min.toordinal() - EPOCH_ORDINAL  # 0001-01-01
MAX_DAY = datetime.date.max.toordinal() - EPOCH_ORDINAL  # 9999-12-31


def _illegal(expected, actual, explanation=""):
    """okapi's IllegalArgumentException(expected, actual, explanation)."""
    from ._lib import IllegalArgumentException
    head = explanation + "\n" if explanation else ""
    return IllegalArgumentException(f"{head}Expected:\n\t{expected}\nFound:\n\t{actual}")


# ------------------------------------------------------------------ payloads
def date_to_days(d):
    return d.toordinal() - EPOCH_ORDINAL


def datetime_to_micros(dt):
    return ((dt.toordinal() - EPOCH_ORDINAL) * MICROS_PER_DAY
            + (dt.hour * 3600 + dt.minute * 60 + dt.second) * MICROS_PER_SECOND + dt.microsecond)


def days_to_date(n):
    n = int(n)
    if not MIN_DAY <= n <= MAX_DAY:
        from ._lib import IllegalStateException
        raise IllegalStateException(f"DATE day number {n} is outside years 0001 to 9999")
    return datetime.date.fromordinal(n + EPOCH_ORDINAL)


def micros_to_datetime(us):
    us = int(us)
    day, tod = divmod(us, MICROS_PER_DAY)
    if not MIN_DAY <= day <= MAX_DAY:
        from ._lib import IllegalStateException
        raise IllegalStateException(f"LOCALDATETIME value {us} is outside years 0001 to 9999")
    sod, micro = divmod(tod, MICROS_PER_SECOND)
    d = datetime.date.fromordinal(day + EPOCH_ORDINAL)
    return datetime.datetime(d.year, d.month, d.day, sod // 3600, sod // 60 % 60, sod % 60, micro)


def temporal_payload(v):
    """The int64 of a datetime.date / datetime.datetime (datetime first: it is
    a subclass of date)."""
    return datetime_to_micros(v) if isinstance(v, datetime.datetime) else date_to_days(v)


# ------------------------------------------------------------- date strings
def _month_len(y, m):
    if m == 2 and y % 4 == 0 and (y % 100 != 0 or y % 400 == 0):
        return 29
    return (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)[m - 1]


def _ymd_smart(y, m, d):
    """SMART resolving of year-month-day: 29..31 past the month's end is its last day."""
    if not (1 <= y <= 9999 and 1 <= m <= 12 and 1 <= d <= 31):
        raise ValueError
    return datetime.date(y, m, min(d, _month_len(y, m)))


def _week1_monday(y):
    jan4 = datetime.date(y, 1, 4)
    return jan4.toordinal() - (jan4.isoweekday() - 1)


def _weeks_in(y):
    return datetime.date(y, 12, 28).isocalendar()[1]


def _week_date(y, w, dow, strict):
    """IsoFields week-based-year resolving: January 4th plus (w − 1) weeks,
    on weekday dow.  STRICT: w within the year's weeks; SMART: 1..53, week 53
    of a 52-week year rolling into the next."""
    if not (1 <= y <= 9999 and 1 <= dow <= 7 and 1 <= w <= (_weeks_in(y) if strict else 53)):
        raise ValueError
    return datetime.date.fromordinal(_week1_monday(y) + 7 * (w - 1) + dow - 1)


def _quarter_date(y, q, doq):
    """IsoFields DAY_OF_QUARTER SMART resolving: the quarter's first day plus doq − 1 (doq in 1..92)."""
    if not (1 <= y <= 9999 and 1 <= q <= 4 and 1 <= doq <= 92):
        raise ValueError
    return datetime.date.fromordinal(datetime.date(y, 3 * (q - 1) + 1, 1).toordinal() + doq - 1)


def _year_day(y, doy):
    if not (1 <= y <= 9999 and 1 <= doy <= 365 + (_month_len(y, 2) == 29)):
        raise ValueError
    return datetime.date.fromordinal(datetime.date(y, 1, 1).toordinal() + doy - 1)


_OFFSET = r"(?:Z|[+-]\d{2}(?::\d{2}(?::\d{2})?)?)?"  # ISO_WEEK_DATE's optional offset id (ignored by LocalDate)

# (pattern, groups → date) in TemporalTypesHelper.scala:51-139's order.  A
# `yyyy` / week-based-year value takes exactly four digits: more need a sign
# (SignStyle.EXCEEDS_PAD in strict parsing), and such years are out of range.
DATE_FORMATS = (
    (r"(\d{4})-(\d{2})-(\d{2})", lambda y, m, d: _ymd_smart(y, m, d)),                      # 2010-01-01
    (r"(\d{4})(\d{2})(\d{2})", lambda y, m, d: _ymd_smart(y, m, d)),                        # 20100101
    (r"(\d{4})-(\d{2})", lambda y, m: _ymd_smart(y, m, 1)),                                  # 2010-10
    (r"(\d{4})(\d{2})", lambda y, m: _ymd_smart(y, m, 1)),                                   # 201010
    (r"(?i)(\d{4})-W(\d{2})-(\d)" + _OFFSET, lambda y, w, d: _week_date(y, w, d, True)),     # 2015-W30-2 (ISO_WEEK_DATE)
    (r"(?i)(\d{4})W(\d{2})(\d)", lambda y, w, d: _week_date(y, w, d, False)),               # 2015W302
    (r"(?i)(\d{4})-W(\d{2})", lambda y, w: _week_date(y, w, 1, False)),                      # 2015-W30
    (r"(?i)(\d{4})W(\d{2})", lambda y, w: _week_date(y, w, 1, False)),                       # 2015W30
    (r"(\d{4})-Q(\d)-(\d{2})", lambda y, q, d: _quarter_date(y, q, d)),                      # 2015-Q2-60
    (r"(\d{4})Q(\d)(\d{2})", lambda y, q, d: _quarter_date(y, q, d)),                        # 2015Q260
    (r"(\d{4})-Q(\d)", lambda y, q: _quarter_date(y, q, 1)),                                 # 2015-Q2
    (r"(\d{4})Q(\d)", lambda y, q: _quarter_date(y, q, 1)),                                  # 2015Q2
    (r"(\d{4})-(\d{3})", lambda y, d: _year_day(y, d)),                                      # 2015-202
    (r"(\d{4})(\d{3})", lambda y, d: _year_day(y, d)),                                       # 2015202
    (r"(\d{4})", lambda y: _ymd_smart(y, 1, 1)),                                             # 2015
)
_DATE_RES = tuple((re.compile(p), fn) for p, fn in DATE_FORMATS)


def parse_date_string(s):
    """parseDateString (:218-231): the first format that parses."""
    for rx, fn in _DATE_RES:
        m = rx.fullmatch(s)
        if m is None:
            continue
        try:
            return fn(*[int(g) for g in m.groups()])
        except ValueError:
            continue
    raise _illegal("a valid date construction string", s)


# ------------------------------------------------------------- time strings
def _hms(h, mi=0, s=0, frac=""):
    if not (0 <= h <= 23 and 0 <= mi <= 59 and 0 <= s <= 59):
        raise ValueError
    return h, mi, s, int((frac or "0").ljust(9, "0"))


# (pattern → (hour, minute, second, nanos)) in TemporalTypesHelper.scala:141-150's order
TIME_FORMATS = (
    r"(\d{2}):(\d{2})(?::(\d{2})(?:\.(\d{1,9}))?)?",  # ISO_LOCAL_TIME
    r"(\d{2})(\d{2})(\d{2})\.(\d{3})",                # HHmmss.SSS
    r"(\d{2})(\d{2})(\d{2})\.(\d{6})",                # HHmmss.SSSSSS
    r"(\d{2})(\d{2})(\d{2})\.(\d{9})",                # HHmmss.SSSSSSSSS
    r"(\d{2})(\d{2})(\d{2})",                         # HHmmss
    r"(\d{2}):(\d{2})",                               # HH:mm
    r"(\d{2})(\d{2})",                                # HHmm
    r"(\d{2})",                                       # HH
)
_TIME_RES = tuple(re.compile(p) for p in TIME_FORMATS)


def parse_time_string(s):
    """parseTimeString (:251-264): (hour, minute, second, nanos)."""
    for rx in _TIME_RES:
        m = rx.fullmatch(s)
        if m is None:
            continue
        g = m.groups()
        try:
            return _hms(*[int(x) for x in g[:3] if x is not None], frac=g[3] if len(g) > 3 else "")
        except ValueError:
            continue
    raise _illegal("a valid time construction string", s)


def _local_datetime(d, hmsn):
    """LocalDateTime.of(date, time) under resolveTimestamp's nanosecond rule
    (TemporalConversions.scala:103-104)."""
    h, mi, s, nanos = hmsn
    if nanos % 1000:
        from ._lib import IllegalStateException
        raise IllegalStateException("Spark does not support nanosecond resolution in 'localdatetime'")
    return datetime.datetime(d.year, d.month, d.day, h, mi, s, nanos // 1000)


# --------------------------------------------------------------------- maps
DATE_BY_MONTH = ("year", "month", "day")
DATE_BY_WEEK = ("year", "week", "dayofweek")
DATE_BY_ORDINAL_DAY = ("year", "ordinalday")
DATE_BY_QUARTER = ("year", "quarter", "dayofquarter")
TIME_IDS = ("hour", "minute", "second")


def _check_significance_order(m, keys):
    """checkSignificanceOrder (:266-280): no key set after an omitted one."""
    have = [k in m for k in keys]
    if any(not a and b for a, b in zip(have, have[1:])):
        raise _illegal("a valid significance order", ", ".join(m),
                       "When constructing dates from a map it is forbidden to omit values of higher significance")


def parse_date_map(m):
    """parseDateMap (:184-216) of {key: int}."""
    sm = {k.lower(): v for k, v in m.items()}
    if "year" not in sm:
        raise _illegal("the key `year` needs to be set", ", ".join(m))
    try:
        if "week" in sm:
            _check_significance_order(sm, DATE_BY_WEEK)
            return _week_date(sm["year"], sm["week"], sm.get("dayofweek", 1), False)
        if "ordinalday" in sm:
            _check_significance_order(sm, DATE_BY_ORDINAL_DAY)
            return _year_day(sm["year"], sm["ordinalday"])
        if "quarter" in sm:
            _check_significance_order(sm, DATE_BY_QUARTER)
            d = _quarter_date(sm["year"], sm["quarter"], sm.get("dayofquarter", 1))
            if d.year != sm["year"]:  # (java.time's with(DAY_OF_YEAR, …) past the year's end)
                raise ValueError
            return d
        _check_significance_order(sm, DATE_BY_MONTH)
        if not 1 <= sm["year"] <= 9999:
            raise ValueError
        return datetime.date(sm["year"], sm.get("month", 1), sm.get("day", 1))
    except ValueError:
        raise _illegal("a valid date", ", ".join(f"{k}: {v}" for k, v in m.items())) from None


def parse_time_map(m):
    """parseTimeMap (:233-249): (hour, minute, second, nanos)."""
    sm = {k.lower(): v for k, v in m.items()}
    _check_significance_order(sm, TIME_IDS)
    nanos = sm.get("millisecond", 0) * 1000000 + sm.get("microsecond", 0) * 1000 + sm.get("nanosecond", 0)
    h, mi, s = sm.get("hour", 0), sm.get("minute", 0), sm.get("second", 0)
    if not (0 <= h <= 23 and 0 <= mi <= 59 and 0 <= s <= 59 and 0 <= nanos <= 999999999):
        raise _illegal("a valid time", ", ".join(f"{k}: {v}" for k, v in m.items()))
    return h, mi, s, nanos


def parse_date(arg):
    """parseDate (:152-157): a {key: int} map or a string."""
    return parse_date_map(arg) if isinstance(arg, dict) else parse_date_string(arg)


def parse_local_datetime(arg):
    """parseLocalDateTime (:159-182) with resolveTimestamp's nanosecond rule."""
    if isinstance(arg, dict):
        return _local_datetime(parse_date_map(arg), parse_time_map(arg))
    ds, _, ts = arg.partition("T")
    d = parse_date_string(ds)
    return _local_datetime(d, parse_time_string(ts) if "T" in arg else (0, 0, 0, 0))


# ---------------------------------------------------------------- durations
def _tdiv(a, b):
    """Java's long division: truncated toward zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _trem(a, b):
    """Java's long remainder: the sign of the dividend."""
    return a - _tdiv(a, b) * b


DURATION_KEYS = ("years", "months", "weeks", "days", "hours", "minutes", "seconds", "milliseconds", "microseconds",
                 "nanoseconds")
DURATION_ACCESSORS = ("years", "quarters", "months", "weeks", "days", "hours", "minutes", "seconds", "milliseconds",
                      "microseconds", "quartersofyear", "monthsofquarter", "monthsofyear", "daysofweek",
                      "minutesofhour", "secondsofminute", "millisecondsofsecond", "microsecondsofsecond")
_DURATION_RE = re.compile(r"^P(\d+Y)?(\d+M)?(\d+W)?(\d+D)?(T(\d+H)?(\d+M)?(\d+(\.\d{1,6})?S)?)?$")


class DurationValue:
    """okapi's Duration (Duration.scala:45): months, days, seconds and the
    nanoseconds below a second."""
    __slots__ = ("months", "days", "seconds", "nanos")

    def __init__(self, months=0, days=0, seconds=0, nanos=0):
        self.months, self.days, self.seconds, self.nanos = int(months), int(days), int(seconds), int(nanos)

    @classmethod
    def of(cls, years=0, months=0, weeks=0, days=0, hours=0, minutes=0, seconds=0, milliseconds=0, microseconds=0,
           nanoseconds=0):
        """Duration.apply (:108-124)."""
        nano_sum = milliseconds * 1000000 + microseconds * 1000 + nanoseconds
        return cls(years * 12 + months, weeks * 7 + days,
                   hours * 3600 + minutes * 60 + seconds + _tdiv(nano_sum, 1000000000), _trem(nano_sum, 1000000000))

    @classmethod
    def from_map(cls, m):
        """Duration.apply(map) (:134-158)."""
        sm = {k.lower(): int(v) for k, v in m.items()}
        bad = [k for k in sm if k not in DURATION_KEYS]
        if bad:
            raise _illegal(", ".join(DURATION_KEYS), ", ".join(sm), f"Unsupported duration values: {', '.join(bad)}")
        return cls.of(**sm)

    @classmethod
    def parse(cls, s):
        """Duration.parse (:160-194)."""
        m = _DURATION_RE.search(s)
        if m is None:
            raise _illegal("a valid duration construction string", s)
        names = ("years", "months", "weeks", "days", None, "hours", "minutes", "seconds")
        parts = {nm: int(g[:-1]) for nm, g in zip(names, m.groups()) if nm not in (None, "seconds") and g is not None}
        sec = m.group(8)
        if sec is not None:  # the double-based split of :175-179
            dv = float(sec[:-1])
            seconds = int(dv)
            fraction = (dv - seconds) * 1000000
            parts.update(seconds=seconds, milliseconds=int(fraction / 1000), microseconds=int(math.fmod(fraction, 1000)))
        return cls.from_map(parts)

    @classmethod
    def from_interval(cls, months, micros):
        """toDuration (TemporalConversions.scala:76-87)."""
        seconds = _tdiv(micros, MICROS_PER_SECOND)
        return cls.of(months=months, days=_tdiv(seconds, 86400), seconds=_trem(seconds, 86400),
                      nanoseconds=_trem(micros, MICROS_PER_SECOND) * 1000)

    @property
    def interval(self):
        """(months, microseconds): toCalendarInterval (TemporalConversions.scala:54-67);
        nanoseconds below a microsecond are dropped."""
        return self.months, _tdiv(self.nanos, 1000) + self.seconds * MICROS_PER_SECOND + self.days * MICROS_PER_DAY

    def __add__(self, other):
        (m1, u1), (m2, u2) = self.interval, other.interval
        return DurationValue.from_interval(m1 + m2, u1 + u2)

    def __sub__(self, other):
        (m1, u1), (m2, u2) = self.interval, other.interval
        return DurationValue.from_interval(m1 - m2, u1 - u2)

    def __eq__(self, other):
        return isinstance(other, DurationValue) and \
            (self.months, self.days, self.seconds, self.nanos) == (other.months, other.days, other.seconds, other.nanos)

    def __hash__(self):
        return hash((self.months, self.days, self.seconds, self.nanos))

    def __repr__(self):
        return f"Duration(months = {self.months}, days = {self.days}, seconds = {self.seconds}, nanos = {self.nanos})"

    def accessor(self, name):
        """durationAccessor (TemporalUdfs.scala:115-150) over the interval; days
        and weeks are their own group, so everything below a day excludes them."""
        months, micros = self.interval
        days = _tdiv(micros, MICROS_PER_DAY)
        sub = micros - days * MICROS_PER_DAY
        key = name.lower()
        table = {
            "years": lambda: _tdiv(months, 12),
            "quarters": lambda: _tdiv(months, 3),
            "months": lambda: months,
            "weeks": lambda: _tdiv(days, 7),
            "days": lambda: days,
            "hours": lambda: _tdiv(sub, 3600 * MICROS_PER_SECOND),
            "minutes": lambda: _tdiv(sub, 60 * MICROS_PER_SECOND),
            "seconds": lambda: _tdiv(sub, MICROS_PER_SECOND),
            "milliseconds": lambda: _tdiv(sub, 1000),
            "microseconds": lambda: sub,
            "quartersofyear": lambda: _trem(_tdiv(months, 3), 4),
            "monthsofquarter": lambda: _trem(months, 3),
            "monthsofyear": lambda: _trem(months, 12),
            "daysofweek": lambda: _trem(days, 7),
            "minutesofhour": lambda: _trem(_tdiv(sub, 60 * MICROS_PER_SECOND), 60),
            "secondsofminute": lambda: _trem(_tdiv(sub, MICROS_PER_SECOND), 60),
            "millisecondsofsecond": lambda: _trem(_tdiv(sub, 1000), 1000),
            "microsecondsofsecond": lambda: _trem(sub, 1000000),
        }
        if key not in table:
            from ._lib import UnsupportedOperationException
            raise UnsupportedOperationException(f"Unknown Duration accessor: {key}")
        return table[key]()


def parse_duration(arg):
    """resolveInterval's value (TemporalConversions.scala:116-121): a map or a string."""
    return DurationValue.from_map(arg) if isinstance(arg, dict) else DurationValue.parse(arg)
