"""THE PARSE, F64 of brx_parse_f64_batch (include/brx.h) on the CPU, twice.  parse_re is the contract by its grammar: the `re` module,
and float() -- Python's correctly rounded conversion -- on strings that it constructs for a, b and the value.  parse_fsm is a
hand-written state machine that sees one byte at a time and rounds exactly on Python integers (no float anywhere).  Neither uses a
helper of the other.  tests/test_parse_f64_abi.py holds each to the contract's check values and the two to each other on a corpus;
tests/test_gpu_parse_f64.py and tools/gpu_parse_f64_rate.py take every expected value from here.  The records themselves are those of
tests/take_oracle.py (the rule of brx_take_batch), used as it is.

A record is `bytes`; spaces a bool (BRX_PARSE_SPACES); quote a byte value or None (None: BRX_PARSE_QUOTED off); words a bool
(BRX_PARSE_WORDS).  A result is (bits, status), bits the binary64 pattern as a Python int."""
import re
import struct
from fractions import Fraction

import numpy as np

import take_oracle

SPACES, QUOTED, WORDS = 16, 32, 64   # BRX_PARSE_SPACES, BRX_PARSE_QUOTED, BRX_PARSE_WORDS
OK, EMPTY, RANGE, BAD, LONG, HARD = 0, 2, 3, 4, 5, 6
NAMES = {OK: "OK", EMPTY: "EMPTY", RANGE: "RANGE", BAD: "BAD", LONG: "LONG", HARD: "HARD"}
MAX_LEN = 64
INF, NAN, SIGN = 0x7FF0000000000000, 0x7FF8000000000000, 0x8000000000000000


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def float_of(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


# ---- form 1: the grammar as a regular expression, the values by float() ---------------------------------------------------------------
_RE_NUM = re.compile(rb"([+-]?)(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?")
_RE_WORD = re.compile(rb"([+-]?)(nan|inf|infinity)", re.I)


def parse_re(r, spaces=False, quote=None, words=False):
    r = bytes(r)
    if len(r) > MAX_LEN:
        return 0, LONG
    t = r.strip(b" \t") if spaces else r
    if quote is not None and len(t) >= 2 and t[0] == quote and t[-1] == quote:
        t = t[1:-1]
    if not t:
        return 0, EMPTY
    if words:
        m = _RE_WORD.fullmatch(t)
        if m:
            return (NAN if m.group(2).lower() == b"nan" else INF) | (SIGN if m.group(1) == b"-" else 0), OK
    m = _RE_NUM.fullmatch(t)
    if not m:
        return 0, BAD
    sg, whole, frac, frac_only, ex = m.groups()
    whole = (whole or b"").decode()
    frac = (frac_only if frac_only is not None else (frac or b"")).decode()
    q = (int(ex) if ex else 0) - len(frac)
    sign = "-" if sg == b"-" else ""
    s = (whole + frac).lstrip("0")
    if not s:
        return bits_of(float(sign + "0")), OK
    if len(s) <= 19 or not s[19:].strip("0"):
        v = float("%s%se%d" % (sign, s, q))
    else:
        q19 = q + len(s) - 19
        v, b = float("%s%se%d" % (sign, s[:19], q19)), float("%s%de%d" % (sign, int(s[:19]) + 1, q19))
        if v != b:
            return bits_of(v), HARD
    return bits_of(v), (RANGE if v == 0 or v in (float("inf"), float("-inf")) else OK)


# ---- form 2: one byte at a time, rounding on integers ----------------------------------------------------------------------------------
def round_exact(w, q):
    """The binary64 pattern of w * 10^q (w >= 0) rounded to nearest, ties to even, subnormals included; INF beyond the largest."""
    if w == 0:
        return 0
    # w >= 1 and q >= 309: at least 10^309, above the largest double plus half its ulp.  w <= 10^19 and q <= -346: at most 10^-327,
    # below 2^-1075, half the least subnormal.  (This keeps the integers below small; the cuts are not the kernel's.)
    if q >= 309:
        return INF
    if q <= -346 and w <= 10 ** 19:
        return 0
    num, den = (w * 10 ** q, 1) if q >= 0 else (w, 10 ** -q)
    e = num.bit_length() - den.bit_length()  # floor(log2(num / den)) or one above it
    if (num < (den << e)) if e >= 0 else ((num << -e) < den):
        e -= 1
    u = max(e - 52, -1074)  # the exponent of the unit in the last place
    if u >= 0:
        den <<= u
    else:
        num <<= -u
    m, rem = divmod(num, den)
    if 2 * rem > den or (2 * rem == den and (m & 1)):
        m += 1
    if m == 1 << 53:
        m, u = 1 << 52, u + 1
    if m < 1 << 52:
        return m  # subnormal, or zero
    biased = u + 52 + 1023
    return INF if biased >= 2047 else (biased << 52) | (m - (1 << 52))


def _is_digit(c):
    return 0x30 <= c <= 0x39


def _lower(c):
    return c + 0x20 if 0x41 <= c <= 0x5A else c


def parse_fsm(r, spaces=False, quote=None, words=False):
    n = len(r)
    if n > MAX_LEN:
        return 0, LONG
    a, e = 0, n
    if spaces:
        while a < e and r[a] in (0x20, 0x09):
            a += 1
        while e > a and r[e - 1] in (0x20, 0x09):
            e -= 1
    if quote is not None and e - a >= 2 and r[a] == quote and r[e - 1] == quote:
        a, e = a + 1, e - 1
    if a == e:
        return 0, EMPTY
    sign = 0
    if r[a] in (0x2B, 0x2D):
        sign = SIGN if r[a] == 0x2D else 0
        a += 1
    if words:
        low = [_lower(c) for c in r[a:e]]
        if low == [0x6E, 0x61, 0x6E]:
            return NAN | sign, OK
        if low == [0x69, 0x6E, 0x66] or low == [0x69, 0x6E, 0x66, 0x69, 0x6E, 0x69, 0x74, 0x79]:
            return INF | sign, OK
    # states: 0 integer digits, 1 fraction digits, 2 just behind e / E, 3 just behind the exponent's sign, 4 exponent digits
    state, mant_digits = 0, 0
    w, sig, dropped, tail, nfrac = 0, 0, 0, False, 0
    ex, eneg = 0, False
    for c in r[a:e]:
        if state <= 1:
            if _is_digit(c):
                mant_digits += 1
                if state == 1:
                    nfrac += 1
                if sig or c != 0x30:
                    if sig < 19:
                        w = w * 10 + (c - 0x30)
                        sig += 1
                    else:
                        dropped += 1
                        tail = tail or c != 0x30
            elif c == 0x2E and state == 0:
                state = 1
            elif c in (0x65, 0x45) and mant_digits:
                state = 2
            else:
                return 0, BAD
        elif state == 2 and c in (0x2B, 0x2D):
            eneg, state = c == 0x2D, 3
        elif _is_digit(c):
            ex, state = ex * 10 + (c - 0x30), 4
        else:
            return 0, BAD
    if mant_digits == 0 or state in (2, 3):
        return 0, BAD
    if sig == 0:
        return sign, OK
    q = (-ex if eneg else ex) - nfrac + dropped
    lo = round_exact(w, q)
    if tail and round_exact(w + 1, q) != lo:
        return lo | sign, HARD
    return lo | sign, (RANGE if lo in (0, INF) else OK)


FORMS = {"re": parse_re, "fsm": parse_fsm}


def exact_bits(text):
    """The correctly rounded pattern of a text that matches the grammar, by exact rational arithmetic (for what HARD leaves open)."""
    m = _RE_NUM.fullmatch(bytes(text))
    sg, whole, frac, frac_only, ex = m.groups()
    frac = frac_only if frac_only is not None else (frac or b"")
    digits = int((whole or b"") + frac or b"0")
    return round_exact(digits, (int(ex) if ex else 0) - len(frac)) | (SIGN if sg == b"-" else 0)


def parse_records(form, arena, src, L, spaces=False, quote=None, words=False):
    """(bits uint64[m], status uint8[m]) of the records arena[src[j] .. + L[j]) under one form."""
    f = FORMS[form] if isinstance(form, str) else form
    buf = bytes(np.asarray(arena, dtype=np.uint8))
    val, status = np.zeros(len(src), dtype=np.uint64), np.zeros(len(src), dtype=np.uint8)
    memo = {}
    for j, (s, ln) in enumerate(zip(src, L)):
        rec = buf[int(s):int(s) + int(ln)]
        if rec not in memo:
            memo[rec] = f(rec, spaces, quote, words)
        val[j], status[j] = memo[rec]
    return val, status


def parse_take(form, arena, off, length, count, pos_off, pos, n_pos, D, flags, quote=0, si=None, sk=None, m=None):
    """A whole call: `flags` is the call's flags word (BRX_TAKE_* and BRX_PARSE_* bits), `quote` the call's byte (ignored without
    QUOTED).  -> (bits, status, L), L the records' lengths under tests/take_oracle.py."""
    src, L = take_oracle.take_vec(arena, off, length, count, pos_off, pos, n_pos, D, flags & 3, si, sk, m)
    val, status = parse_records(form, arena, src, L, bool(flags & SPACES), quote if flags & QUOTED else None, bool(flags & WORDS))
    return val, status, L


# ---- the check values of the contract: (record, flags, bits, status) -------------------------------------------------------------------
_E62 = b"1e" + b"0" * 59 + b"5"
_E64 = b"1e" + b"0" * 61 + b"5"  # the exponent field up to the 64-byte bound
_Z64 = b"0" * 63 + b"1"
CHECK = [
    (b"0", 0, 0x0000000000000000, OK), (b"-0", 0, 0x8000000000000000, OK), (b"1", 0, 0x3FF0000000000000, OK),
    (b"-1.5", 0, 0xBFF8000000000000, OK), (b"0.1", 0, 0x3FB999999999999A, OK), (b".5", 0, 0x3FE0000000000000, OK),
    (b"5.", 0, 0x4014000000000000, OK), (b"1e23", 0, 0x44B52D02C7E14AF6, OK), (b"1E+2", 0, 0x4059000000000000, OK),
    (b"1e-2", 0, 0x3F847AE147AE147B, OK), (b"9007199254740993", 0, 0x4340000000000000, OK),
    (b"9007199254740995", 0, 0x4340000000000002, OK), (b"1.7976931348623157e308", 0, 0x7FEFFFFFFFFFFFFF, OK),
    (b"1.7976931348623158e308", 0, 0x7FEFFFFFFFFFFFFF, OK), (b"1.7976931348623159e308", 0, 0x7FF0000000000000, RANGE),
    (b"-1e309", 0, 0xFFF0000000000000, RANGE), (b"4.9e-324", 0, 0x0000000000000001, OK),
    (b"2.4703282292062328e-324", 0, 0x0000000000000001, OK), (b"2.4703282292062327e-324", 0, 0x0000000000000000, RANGE),
    (b"1e-400", 0, 0x0000000000000000, RANGE), (b"2.2250738585072014e-308", 0, 0x0010000000000000, OK),
    (b"2.2250738585072011e-308", 0, 0x000FFFFFFFFFFFFF, OK), (b"0.1000000000000000055511151231257827", 0, 0x3FB999999999999A, OK),
    (b"123456789012345678901234567890", 0, 0x45F8EE90FF6C373E, OK), (b"9007199254740993.0000000000000000", 0, 0x4340000000000000, OK),
    (b"9007199254740993.0000000000000001", 0, 0x4340000000000000, HARD), (b"0e99999", 0, 0x0000000000000000, OK),
    (_E62, 0, 0x40F86A0000000000, OK), (_E64, 0, 0x40F86A0000000000, OK), (_Z64, 0, 0x3FF0000000000000, OK), (b"0" + _Z64, 0, 0, LONG),
    (b"1e", 0, 0, BAD), (b"e5", 0, 0, BAD), (b".", 0, 0, BAD), (b"1.2.3", 0, 0, BAD), (b"+.e1", 0, 0, BAD), (b"0x10", 0, 0, BAD),
    (b"1e+", 0, 0, BAD), (b"nan", 0, 0, BAD), (b"-Infinity", WORDS, 0xFFF0000000000000, OK),
]

# ---- records biased to where the grammar and the rounding turn --------------------------------------------------------------------------
CORNERS = [b"", b"-", b"+", b".", b"-.", b"e", b"E5", b"1e", b"1e+", b"1e-", b"1e+-1", b"1ee1", b"1e1e1", b"1e1.5", b"1.e1", b".1e1", b".e1",
           b"+.e1", b"1.2.3", b"0x10", b"1,5", b"1 ", b" 1", b"--1", b"+-1", b"5.", b".5", b"-0", b"+0", b"-0.0e-0", b"0e99999", b"-0e-99999",
           b"1e308", b"1e309", b"1e-323", b"1e-324", b"1e-325", b"1e999999", b"1e-999999", b"1e1000000", b"1e-1000000",
           b"123e00000000000000000000000000000000000000000000000000000000002", b"nan", b"NaN", b"-nan", b"+NAN", b"inf", b"-Inf", b"+INF",
           b"infinity", b"-iNfInItY", b"na", b"nanx", b"infinit", b"infinityy", b"+-inf", b"in", b"i", b"n", b"1nan", b"nane1", b'"nan"',
           b" inf ", b'" 42"', b'"4.2', b'4.2"', b'""', b'"', b"  ", b"\t", b"1e5 ", b"9007199254740993.0000000000000001",
           b"17976931348623157" + b"0" * 40 + b"e252", b"179769313486231580793728971405303415079934132710037826936173778", b"8.5", b"8.50000000000000000000"]
JUNK = b"0123456789+-.. \t\"'eEeExXnaNAifIF,\r_\x80\xb0\xff\x00/:@`"


def _digits(rng, c):
    return bytes(rng.integers(0x30, 0x3A, c).astype(np.uint8))


def random_field(rng, quote=0x22):
    """One record (no 0x0A in it): 1 .. 45 significant digits, the point anywhere, exponents -345 .. 312 pulled back by the digits in
    front of the point, leading zeros, exponent fields with leading zeros, words, corners and garbage, blanks and quotes around."""
    form = int(rng.integers(0, 10))
    if form == 0:
        return bytes(JUNK[int(i)] for i in rng.integers(0, len(JUNK), int(rng.integers(0, 70))))
    if form == 1:
        d = CORNERS[int(rng.integers(0, len(CORNERS)))]
    else:
        c = int(rng.integers(1, 46)) if form < 6 else int(rng.integers(1, 20))
        d = bytes([0x31 + int(rng.integers(0, 9))]) + _digits(rng, c - 1)
        if rng.integers(0, 4) == 0:
            d = d[:19] + b"0" * (len(d) - 19) if rng.integers(0, 2) else d[:19] + b"0" * max(len(d) - 20, 0) + d[-1:]
        ex = int(rng.integers(-345, 313))
        if rng.integers(0, 4) == 0:
            d = b"0" * int(rng.integers(1, 8)) + d
        if rng.integers(0, 2):
            k = int(rng.integers(0, len(d) + 1))
            ex += len(d) - k
            d = d[:k] + b"." + d[k:]
            if d == b".":
                d = b"0."
        if rng.integers(0, 5) > 0 or form >= 8:
            d += (b"e", b"E")[int(rng.integers(0, 2))] + (b"", b"+")[int(rng.integers(0, 2)) if ex >= 0 else 0]
            d += (b"%d" % ex if rng.integers(0, 6) else b"%s%s%d" % (b"-" if ex < 0 else b"", b"0" * int(rng.integers(1, 12)), abs(ex)))
        if rng.integers(0, 3) == 0:
            d = (b"-", b"+")[int(rng.integers(0, 2))] + d
    q = bytes([quote])
    if rng.integers(0, 5) == 0:
        d = q + d + q
    if rng.integers(0, 5) == 0:
        d = (b" ", b"\t")[int(rng.integers(0, 2))] * int(rng.integers(0, 8)) + d + (b" ", b"\t")[int(rng.integers(0, 2))] * int(rng.integers(0, 8))
    if rng.integers(0, 12) == 0:
        d = q + d + q
    return d


def midpoint_records(rng, qs):
    """For every q of qs: the decimal expansion of the midpoint of a random double near 10^q and its successor, cut to 17 .. 45 digits,
    with the last digit moved by -1, 0 and +1 -- the texts that a conversion finds hardest.  Subnormals for q below -308."""
    out = []
    for q in qs:
        d = float("%de%d" % (int(rng.integers(10 ** 16, 10 ** 17)), q - 16))
        b0 = min(bits_of(d), 0x7FEFFFFFFFFFFFFE)
        mid = (Fraction(float_of(b0)) + Fraction(float_of(b0 + 1))) / 2
        k = int(rng.integers(17, 46))
        p = k + 345  # enough decimals for k digits of anything above the least subnormal's half
        big = mid.numerator * 10 ** p // mid.denominator
        cut = len(str(big)) - k
        for delta in (-1, 0, 1):
            digits = b"%d" % (big // 10 ** cut + delta)
            ex = cut - p
            if rng.integers(0, 2):  # d.ddd e X
                ex += len(digits) - 1
                digits = digits[:1] + b"." + digits[1:]
            t = digits + b"e%d" % ex
            if len(t) <= MAX_LEN:
                out.append(t)
    return out
