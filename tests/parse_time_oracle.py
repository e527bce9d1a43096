"""THE PARSE, TIME of include/brx.h (brx_parse_time_batch), stated twice on the CPU, for the tests of the call.
Form 1 (parse_re): regular expressions over the trimmed text, the calendar from datetime.date (toordinal; year 0000 as year 0400 minus
146097 days, because datetime starts at year 1), the value on Python integers.
Form 2 (parse_fsm): a byte-serial state machine that reads the text once from left to right, with days-from-civil arithmetic on Python
integers.  It shares nothing with form 1 but the status numbers.
Both return (val, status, zone): val as a signed Python integer, zone NO_ZONE where none is reported.  CHECK is the contract's table.
parse_take states a whole call on top of tests/take_oracle.py."""
import datetime
import re

import numpy as np

import take_oracle

OK, INEXACT, EMPTY, RANGE, BAD, LONG = 0, 1, 2, 3, 4, 5
NAMES = {OK: "OK", INEXACT: "INEXACT", EMPTY: "EMPTY", RANGE: "RANGE", BAD: "BAD", LONG: "LONG"}
DATE, TIME, STAMP = 0, 1, 2
KIND_NAMES = {DATE: "DATE", TIME: "TIME", STAMP: "STAMP"}
SPACES, QUOTED = 16, 32
MAX_LEN = 64
MAX_SCALE = 9
NO_ZONE = -32768
MAX, MIN = (1 << 63) - 1, -(1 << 63)


def _trim(r, spaces, quote):
    t = bytes(r)
    if spaces:
        t = t.strip(b" \t")
    if quote is not None and len(t) >= 2 and t[0] == quote and t[-1] == quote:
        t = t[1:-1]
    return t


def _finish(secs, frac, scale, zone):
    """steps 7 and 8 from secs, the fraction digits (bytes) and the zone in minutes or None"""
    kept = frac[:scale].ljust(scale, b"0")
    v = secs * 10 ** scale + (int(kept) if kept else 0)
    if v > MAX:
        return MAX, RANGE, NO_ZONE
    if v < MIN:
        return MIN, RANGE, NO_ZONE
    return v, (INEXACT if frac[scale:].strip(b"0") else OK), (NO_ZONE if zone is None else zone)


# ---- form 1 ------------------------------------------------------------------------------------------------------------------------------
_DATE = rb"([0-9]{4})-([0-9]{2})-([0-9]{2})"
_TIME = rb"([0-9]{2}):([0-9]{2})(?::([0-9]{2})(?:[.,]([0-9]+))?)?"
_ZONE = rb"([Zz]|[+-][0-9]{2}:[0-9]{2}|[+-][0-9]{4}|[+-][0-9]{2})"
_RE = {DATE: re.compile(_DATE), TIME: re.compile(_TIME), STAMP: re.compile(_DATE + rb"(?:[Tt ]" + _TIME + _ZONE + rb"?)?")}


def _days_datetime(y, mo, d):
    try:
        if y == 0:
            return datetime.date(400, mo, d).toordinal() - 146097 - datetime.date(1970, 1, 1).toordinal()
        return datetime.date(y, mo, d).toordinal() - datetime.date(1970, 1, 1).toordinal()
    except ValueError:
        return None


def parse_re(r, kind, scale=0, spaces=False, quote=None):
    if len(r) > MAX_LEN:
        return 0, LONG, NO_ZONE
    t = _trim(r, spaces, quote)
    if not t:
        return 0, EMPTY, NO_ZONE
    m = _RE[kind].fullmatch(t)
    if not m:
        return 0, BAD, NO_ZONE
    g = list(m.groups())
    days = 0
    if kind != TIME:
        days = _days_datetime(int(g[0]), int(g[1]), int(g[2]))
        if days is None:
            return 0, BAD, NO_ZONE
        if kind == DATE:
            return days, OK, NO_ZONE
        g = g[3:]
    hh, mi, ss = (int(x) if x is not None else 0 for x in g[:3])
    if hh > 23 or mi > 59 or ss > 59:
        return 0, BAD, NO_ZONE
    zone = None
    if kind == STAMP and g[4] is not None:
        z = g[4].replace(b":", b"")
        if z in (b"Z", b"z"):
            zone = 0
        else:
            zh, zm = int(z[1:3]), int(z[3:5] or b"0")
            if zh > 23 or zm > 59:
                return 0, BAD, NO_ZONE
            zone = (zh * 60 + zm) * (-1 if z[:1] == b"-" else 1)
    secs = days * 86400 + hh * 3600 + mi * 60 + ss - (zone or 0) * 60
    return _finish(secs, g[3] or b"", scale, zone)


# ---- form 2 ------------------------------------------------------------------------------------------------------------------------------
def _days_civil(y, m, d):
    y -= m <= 2
    era = y // 400  # (Python's floor division: year -1 is era -1)
    yoe = y - era * 400
    mp = (m + 9) % 12
    doy = (153 * mp + 2) // 5 + d - 1
    doe = yoe * 365 + yoe // 4 - yoe // 100 + doy
    return era * 146097 + doe - 719468


def _month_len(y, m):
    if m == 2:
        return 29 if y % 4 == 0 and (y % 100 != 0 or y % 400 == 0) else 28
    return 30 if m in (4, 6, 9, 11) else 31


class _Reader:
    def __init__(self, t):
        self.t, self.i = t, 0

    def peek(self):
        return self.t[self.i] if self.i < len(self.t) else -1

    def digits(self, c):
        """exactly c digits as a number, or None"""
        v = 0
        for _ in range(c):
            b = self.peek()
            if not 0x30 <= b <= 0x39:
                return None
            v = v * 10 + b - 0x30
            self.i += 1
        return v

    def byte(self, allowed):
        b = self.peek()
        if b < 0 or b not in allowed:
            return None
        self.i += 1
        return b


def parse_fsm(r, kind, scale=0, spaces=False, quote=None):
    bad = (0, BAD, NO_ZONE)
    if len(r) > MAX_LEN:
        return 0, LONG, NO_ZONE
    lo, hi = 0, len(r)
    if spaces:
        while lo < hi and r[lo] in (0x20, 0x09):
            lo += 1
        while hi > lo and r[hi - 1] in (0x20, 0x09):
            hi -= 1
    if quote is not None and hi - lo >= 2 and r[lo] == quote and r[hi - 1] == quote:
        lo, hi = lo + 1, hi - 1
    if lo == hi:
        return 0, EMPTY, NO_ZONE
    rd = _Reader(bytes(r[lo:hi]))
    days = 0
    have_time = kind == TIME
    if kind != TIME:
        y = rd.digits(4)
        if y is None or rd.byte(b"-") is None:
            return bad
        mo = rd.digits(2)
        if mo is None or rd.byte(b"-") is None:
            return bad
        d = rd.digits(2)
        if d is None or not 1 <= mo <= 12 or not 1 <= d <= _month_len(y, mo):
            return bad
        days = _days_civil(y, mo, d)
        if kind == DATE:
            return (days, OK, NO_ZONE) if rd.peek() < 0 else bad
        if rd.peek() >= 0:
            if rd.byte(b"Tt ") is None:
                return bad
            have_time = True
    hh = mi = ss = 0
    kept, keep_n, dropped_nonzero, zone = 0, 0, False, None
    if have_time:
        hh = rd.digits(2)
        if hh is None or rd.byte(b":") is None:
            return bad
        mi = rd.digits(2)
        if mi is None:
            return bad
        if rd.peek() == 0x3A:
            rd.i += 1
            ss = rd.digits(2)
            if ss is None:
                return bad
            if rd.peek() in (0x2E, 0x2C):
                rd.i += 1
                nf = 0
                while 0x30 <= rd.peek() <= 0x39:
                    if nf < scale:
                        kept, keep_n = kept * 10 + rd.peek() - 0x30, keep_n + 1
                    elif rd.peek() != 0x30:
                        dropped_nonzero = True
                    nf += 1
                    rd.i += 1
                if nf == 0:
                    return bad
        if hh > 23 or mi > 59 or ss > 59:
            return bad
        if kind == STAMP and rd.peek() >= 0:
            c = rd.byte(b"Zz+-")
            if c is None:
                return bad
            if c in b"Zz":
                zone = 0
            else:
                zh = rd.digits(2)
                if zh is None:
                    return bad
                zm = 0
                if rd.peek() >= 0:
                    if rd.peek() == 0x3A:
                        rd.i += 1
                    zm = rd.digits(2)
                    if zm is None:
                        return bad
                if zh > 23 or zm > 59:
                    return bad
                zone = zh * 60 + zm
                if c == 0x2D:
                    zone = -zone
        if rd.peek() >= 0:
            return bad
    secs = days * 86400 + hh * 3600 + mi * 60 + ss - (zone or 0) * 60
    v = secs * 10 ** scale + kept * 10 ** (scale - keep_n)
    if v > MAX:
        return MAX, RANGE, NO_ZONE
    if v < MIN:
        return MIN, RANGE, NO_ZONE
    return v, INEXACT if dropped_nonzero else OK, NO_ZONE if zone is None else zone


FORMS = {"re": parse_re, "fsm": parse_fsm}


def parse_records(form, arena, src, L, kind, scale=0, spaces=False, quote=None):
    """(val int64[m], status uint8[m], zone int16[m]) of the records arena[src[j] .. + L[j]) under one form."""
    f = FORMS[form] if isinstance(form, str) else form
    buf = bytes(np.asarray(arena, dtype=np.uint8))
    m = len(src)
    val, status, zone = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.uint8), np.zeros(m, dtype=np.int16)
    memo = {}
    for j, (s, ln) in enumerate(zip(src, L)):
        rec = buf[int(s):int(s) + int(ln)]
        if rec not in memo:
            memo[rec] = f(rec, kind, scale, spaces, quote)
        val[j], status[j], zone[j] = memo[rec]
    return val, status, zone


def parse_take(form, arena, off, length, count, pos_off, pos, n_pos, D, flags, kind, scale=0, quote=0, si=None, sk=None, m=None):
    """A whole call: `flags` is the call's flags word (BRX_TAKE_* and BRX_PARSE_* bits), `quote` the call's byte (ignored without
    QUOTED).  -> (val, status, zone, L), L the records' lengths under tests/take_oracle.py."""
    src, L = take_oracle.take_vec(arena, off, length, count, pos_off, pos, n_pos, D, flags & 3, si, sk, m)
    val, status, zone = parse_records(form, arena, src, L, kind, scale, bool(flags & SPACES), quote if flags & QUOTED else None)
    return val, status, zone, L


# ---- the check values of the contract: (record, kind, scale, flags, val, status, zone) ----------------------------------------------------
_S = b"2024-03-10T07:08:09"
_L64 = _S + b"." + b"0" * 38 + b"+05:30"
_L65 = _S + b"." + b"0" * 39 + b"+05:30"
_I64 = _S + b".123" + b"0" * 40 + b"1"
_SQ = SPACES | QUOTED


def _bad(kind, scale, recs, flags=0):
    return [(r, kind, scale, flags, 0, BAD, NO_ZONE) for r in recs]


CHECK = (
    [(b"1970-01-01", DATE, 0, 0, 0, OK, NO_ZONE), (b"1969-12-31", DATE, 0, 0, -1, OK, NO_ZONE), (b"0000-01-01", DATE, 0, 0, -719528, OK, NO_ZONE),
     (b"0000-02-29", DATE, 0, 0, -719469, OK, NO_ZONE), (b"2000-02-29", DATE, 0, 0, 11016, OK, NO_ZONE),
     (b"9999-12-31", DATE, 0, 0, 2932896, OK, NO_ZONE)]
    + _bad(DATE, 0, [b"1900-02-29", b"2100-02-29", b"2024-02-30", b"2023-04-31", b"2023-00-10", b"2023-13-01", b"2023-01-00", b"2023-1-01",
                     b"20230101", b"+2023-01-01", b"2023-01-01T00:00"])
    + [(b"", DATE, 0, 0, 0, EMPTY, NO_ZONE),
       (b"00:00", TIME, 0, 0, 0, OK, NO_ZONE), (b"23:59:59", TIME, 0, 0, 86399, OK, NO_ZONE)]
    + _bad(TIME, 0, [b"24:00:00", b"12:60", b"23:59:60", b"12:34:56.", b"12:34.5", b"12:34:56Z", b"1:02:03"])
    + [(b"12:34:56.789", TIME, 3, 0, 45296789, OK, NO_ZONE), (b"12:34:56,7891", TIME, 3, 0, 45296789, INEXACT, NO_ZONE),
       (b"23:59:59.999999999", TIME, 9, 0, 86399999999999, OK, NO_ZONE),
       (b"1970-01-01T00:00:00Z", STAMP, 0, 0, 0, OK, 0), (b"2024-03-10", STAMP, 0, 0, 1710028800, OK, NO_ZONE),
       (b"2024-03-10 07:08", STAMP, 0, 0, 1710054480, OK, NO_ZONE), (b"2024-03-10T07:08Z", STAMP, 0, 0, 1710054480, OK, 0),
       (b"2024-03-10t07:08:09z", STAMP, 0, 0, 1710054489, OK, 0), (_S + b"-0800", STAMP, 0, 0, 1710083289, OK, -480),
       (_S + b"+01", STAMP, 0, 0, 1710050889, OK, 60), (_S + b"-00:00", STAMP, 0, 0, 1710054489, OK, 0),
       (b"1969-12-31T23:59:59.5Z", STAMP, 0, 0, -1, INEXACT, 0), (b"0000-01-01T00:00:00+23:59", STAMP, 0, 0, -62167305540, OK, 1439),
       (b"9999-12-31T23:59:59-23:59", STAMP, 0, 0, 253402387139, OK, -1439)]
    + _bad(STAMP, 0, [_S + b"+24:00", _S + b"+05:60", _S + b"+5", _S + b"+05:3", _S + b" Z", b"2024-03-10T07:08:60Z", b"2024-03-10T24:00:00Z",
                      _S + b".Z", b"2024-03-10T07Z", b"2024-03-10T", b"2024-02-30T00:00:00Z", b"2024-03-10_07:08:09", _S + b"ZZ"])
    + [(b"2024-03-10 07:08:09,123", STAMP, 3, 0, 1710054489123, OK, NO_ZONE), (_S + b".1239", STAMP, 3, 0, 1710054489123, INEXACT, NO_ZONE),
       (b"1969-12-31T23:59:59.5Z", STAMP, 3, 0, -500, OK, 0), (_L64, STAMP, 3, 0, 1710034689000, OK, 330), (_L65, STAMP, 3, 0, 0, LONG, NO_ZONE),
       (_I64, STAMP, 3, 0, 1710054489123, INEXACT, NO_ZONE),
       (_S + b".5+05:30", STAMP, 6, 0, 1710034689500000, OK, 330),
       (b"2262-04-11T23:47:16.854775807Z", STAMP, 9, 0, MAX, OK, 0), (b"2262-04-11T23:47:16.854775808Z", STAMP, 9, 0, MAX, RANGE, NO_ZONE),
       (b"2262-04-11T23:47:16.8547758079Z", STAMP, 9, 0, MAX, INEXACT, 0), (b"1677-09-21T00:12:43.145224192Z", STAMP, 9, 0, MIN, OK, 0),
       (b"1677-09-21T00:12:43.145224191Z", STAMP, 9, 0, MIN, RANGE, NO_ZONE), (b"1677-09-21T00:12:43.1452241919Z", STAMP, 9, 0, MIN, RANGE, NO_ZONE),
       (b"9999-12-31T23:59:59Z", STAMP, 9, 0, MAX, RANGE, NO_ZONE), (b"0000-01-01T00:00:00Z", STAMP, 9, 0, MIN, RANGE, NO_ZONE),
       (b' "2024-03-10T07:08:09Z"\t', STAMP, 0, _SQ, 1710054489, OK, 0), (b'" 2024-03-10"', STAMP, 0, _SQ, 0, BAD, NO_ZONE),
       (b'""', STAMP, 0, _SQ, 0, EMPTY, NO_ZONE)])
assert [len(x) for x in (_L64, _L65, _I64)] == [64, 65, 64]


# ---- generators for the tests ----------------------------------------------------------------------------------------------------------------
_MDAYS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)
JUNK = b"0123456789-:.,TtZz+ \t\"'_/\r\x80\xff\x00"


def random_date(rng, year=None):
    y = int(rng.integers(0, 10000)) if year is None else year
    mo = int(rng.integers(1, 13))
    return b"%04d-%02d-%02d" % (y, mo, int(rng.integers(1, _MDAYS[mo - 1] + 1)))


def random_time(rng, nfrac=None, secs=True):
    t = b"%02d:%02d" % (int(rng.integers(0, 24)), int(rng.integers(0, 60)))
    if not secs:
        return t
    t += b":%02d" % int(rng.integers(0, 60))
    if nfrac is None:
        nfrac = int(rng.integers(0, 13)) if rng.integers(0, 3) else 0
    if nfrac:
        digs = bytes(rng.integers(0x30, 0x3A, nfrac).astype(np.uint8))
        if rng.integers(0, 3) == 0:  # zeros behind some place: OK where the scale cuts there
            cut = int(rng.integers(0, nfrac + 1))
            digs = digs[:cut] + b"0" * (nfrac - cut)
        t += b".,"[int(rng.integers(0, 4)) == 0:][:1] + digs
    return t


def random_zone(rng):
    k = int(rng.integers(0, 6))
    if k == 0:
        return b""
    if k == 1:
        return b"Zz"[int(rng.integers(0, 2)):][:1]
    sg, zh, zm = b"+-"[int(rng.integers(0, 2)):][:1], int(rng.integers(0, 24)), int(rng.integers(0, 60))
    return sg + (b"%02d:%02d" % (zh, zm), b"%02d%02d" % (zh, zm), b"%02d" % zh, b"%02d:%02d" % (zh, zm))[k - 2]


def random_stamp(rng, year=None, nfrac=None):
    secs = bool(rng.integers(0, 8))
    return random_date(rng, year) + b"Tt "[int(rng.integers(0, 3)):][:1] + random_time(rng, nfrac if secs else 0, secs) + random_zone(rng)


def stamp_of_length(rng, L):
    """a record of exactly L bytes: mostly a well-formed stamp, the fraction stretched or cut to fit; below 10 bytes a cut stamp"""
    if L < 10:
        return random_stamp(rng)[:L]
    if L == 10:
        return random_date(rng)
    z = random_zone(rng)
    for _ in range(50):
        if L - 11 - len(z) in (5, 8) or L - 11 - len(z) >= 10:
            break
        z = random_zone(rng)
    room = L - 11 - len(z)
    if room == 5:
        t = random_time(rng, 0, False)
    elif room == 8:
        t = random_time(rng, 0)
    elif room >= 10:
        t = random_time(rng, room - 9)
    else:
        return (random_stamp(rng) + b"0" * L)[:L]
    r = random_date(rng) + b"Tt "[int(rng.integers(0, 3)):][:1] + t + z
    assert len(r) == L
    return r


def mutate(rng, r):
    """one byte of r replaced, removed or doubled: mostly BAD, sometimes still a stamp"""
    if not r:
        return r
    i, k = int(rng.integers(0, len(r))), int(rng.integers(0, 3))
    c = JUNK[int(rng.integers(0, len(JUNK))):][:1]
    return r[:i] + (c + r[i + 1:], r[i + 1:], r[i:i + 1] + r[i:])[k]


def random_field(rng, kind, quote=0x22):
    """a record for `kind`: well-formed ones, mutated ones, blanks and quotes around them, junk, the empty record"""
    k = int(rng.integers(0, 16))
    if k == 0:
        return bytes(JUNK[int(i)] for i in rng.integers(0, len(JUNK), int(rng.integers(0, 30))))
    if k == 1:
        return b""
    r = (random_date(rng), random_time(rng), random_stamp(rng))[kind if k < 13 else int(rng.integers(0, 3))]
    if k in (2, 3, 4):
        r = mutate(rng, r)
    if k == 5:
        r = bytes([quote]) + r + bytes([quote])
    if k == 6:
        r = b" " * int(rng.integers(0, 3)) + bytes([quote]) * int(rng.integers(0, 2)) + r + bytes([quote]) * int(rng.integers(0, 2)) + b"\t "[
            int(rng.integers(0, 2)):]
    if k == 7:
        r = r + b"0" * int(rng.integers(30, 60))  # towards and beyond 64 bytes
    return r


def range_edges(scale, form="re"):
    """Stamps one unit inside, on and one unit outside the 64-bit bounds at scale 8 or 9, derived from the bounds on Python integers
    (datetime gives the civil date), in UTC and with zones, so that the wall-clock text lies on either side of the bound's own:
    [(record, expected)].  At scale 8 the lower bound is the year -953, outside the calendar: only the upper one has stamps, and the
    calendar's first second is inside."""
    P = 10 ** scale
    epoch = datetime.datetime(1970, 1, 1)
    out = [b"0000-01-01T00:00:00." + b"0" * scale + b"+23:59", b"0000-01-01T00:00:00Z", b"9999-12-31T23:59:59.999999999-23:59"]
    for bound in (MAX, MIN) if scale == 9 else (MAX,):
        for delta in (-1, 0, 1):
            for zmin in (0, 1439, -1439, 330, -1):
                secs, frac = divmod(bound + delta, P)
                days, sod = divmod(secs + zmin * 60, 86400)
                d = epoch + datetime.timedelta(days=days)
                z = b"Z" if zmin == 0 else b"%s%02d:%02d" % (b"+" if zmin > 0 else b"-", abs(zmin) // 60, abs(zmin) % 60)
                out.append(b"%04d-%02d-%02dT%02d:%02d:%02d.%0*d%s" % (d.year, d.month, d.day, sod // 3600, sod // 60 % 60, sod % 60, scale, frac, z))
    f = FORMS[form]
    return [(r, f(r, STAMP, scale)) for r in out]
