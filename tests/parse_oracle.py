"""THE PARSE of brx_parse_batch (include/brx.h) on the CPU, twice, on Python integers: parse_re is the contract by its grammar (the
`re` module, int(), slicing); parse_fsm is a hand-written state machine that sees one byte at a time.  Neither uses a helper of the
other.  tests/test_parse_abi.py holds each to the contract's check values and the two to each other on random records;
tests/test_gpu_parse.py and tools/gpu_parse_rate.py take every expected value from here.  The records themselves are those of
tests/take_oracle.py (the rule of brx_take_batch), used as it is.

A record is `bytes`; kind is INT / DEC / HEX; scale 0 .. 18 (DEC); spaces a bool (BRX_PARSE_SPACES); quote a byte value or None
(None: BRX_PARSE_QUOTED off).  A result is (val, status) with val a signed 64-bit Python int."""
import re

import numpy as np

import take_oracle

SPACES, QUOTED = 16, 32          # BRX_PARSE_SPACES, BRX_PARSE_QUOTED
INT, DEC, HEX = 0, 1, 2          # BRX_PARSE_INT ...
OK, INEXACT, EMPTY, RANGE, BAD, LONG = 0, 1, 2, 3, 4, 5
MAX_LEN = 64
MAX, MIN = (1 << 63) - 1, -(1 << 63)


# ---- form 1: the grammar as regular expressions, the value by int() ------------------------------------------------------------------
_RE_INT = re.compile(rb"([+-]?)([0-9]+)")
_RE_DEC = re.compile(rb"([+-]?)(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))")
_RE_HEX = re.compile(rb"(?:0[xX])?([0-9a-fA-F]+)")


def parse_re(r, kind, scale=0, spaces=False, quote=None):
    r = bytes(r)
    if len(r) > MAX_LEN:
        return 0, LONG
    t = r.strip(b" \t") if spaces else r
    if quote is not None and len(t) >= 2 and t[0] == quote and t[-1] == quote:
        t = t[1:-1]
    if not t:
        return 0, EMPTY
    if kind == HEX:
        m = _RE_HEX.fullmatch(t)
        if not m:
            return 0, BAD
        v = int(m.group(1), 16)
        return (-1, RANGE) if v >= 1 << 64 else (v - (1 << 64) if v >> 63 else v, OK)
    m = (_RE_INT if kind == INT else _RE_DEC).fullmatch(t)
    if not m:
        return 0, BAD
    if kind == INT:
        whole, frac = m.group(2), b""
    else:
        whole, frac = (m.group(2) or b""), (m.group(3) or b"") if m.group(2) is not None else m.group(4)
    kept = frac[:scale] + b"0" * (scale - len(frac[:scale]))
    v = int(whole + kept or b"0")
    if m.group(1) == b"-":
        v = -v
    if v > MAX:
        return MAX, RANGE
    if v < MIN:
        return MIN, RANGE
    return v, (INEXACT if frac[scale:].strip(b"0") else OK)


# ---- form 2: one byte at a time ------------------------------------------------------------------------------------------------------
def parse_fsm(r, kind, scale=0, spaces=False, quote=None):
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
    if kind == HEX:
        if e - a >= 2 and r[a] == 0x30 and r[a + 1] in (0x78, 0x58):
            a += 2
        if a == e:
            return 0, BAD
        v = 0
        for c in r[a:e]:
            if 0x30 <= c <= 0x39:
                d = c - 0x30
            elif 0x61 <= c <= 0x66:
                d = c - 0x61 + 10
            elif 0x41 <= c <= 0x46:
                d = c - 0x41 + 10
            else:
                return 0, BAD
            v = v * 16 + d
        if v > 0xFFFFFFFFFFFFFFFF:
            return -1, RANGE
        return (v - 0x10000000000000000 if v >= 0x8000000000000000 else v), OK
    neg = False
    if r[a] in (0x2B, 0x2D):
        neg = r[a] == 0x2D
        a += 1
    state, v, digits, taken, lost = 0, 0, 0, 0, False  # state 0: in I, 1: in F
    for c in r[a:e]:
        if c == 0x2E and kind == DEC and state == 0:
            state = 1
        elif 0x30 <= c <= 0x39:
            digits += 1
            if state == 0:
                v = v * 10 + (c - 0x30)
            elif taken < scale:
                v = v * 10 + (c - 0x30)
                taken += 1
            elif c != 0x30:
                lost = True
        else:
            return 0, BAD
    if digits == 0:
        return 0, BAD
    while taken < scale:
        v *= 10
        taken += 1
    if neg:
        if v > 0x8000000000000000:
            return MIN, RANGE
        return -v, (INEXACT if lost else OK)
    if v > 0x7FFFFFFFFFFFFFFF:
        return MAX, RANGE
    return v, (INEXACT if lost else OK)


FORMS = {"re": parse_re, "fsm": parse_fsm}


def parse_records(form, arena, src, L, kind, scale=0, spaces=False, quote=None):
    """(val int64[m], status uint8[m]) of the records arena[src[j] .. + L[j]) under one form."""
    f = FORMS[form] if isinstance(form, str) else form
    buf = bytes(np.asarray(arena, dtype=np.uint8))
    val, status = np.zeros(len(src), dtype=np.int64), np.zeros(len(src), dtype=np.uint8)
    for j, (s, ln) in enumerate(zip(src, L)):
        val[j], status[j] = f(buf[int(s):int(s) + int(ln)], kind, scale, spaces, quote)
    return val, status


def parse_take(form, arena, off, length, count, pos_off, pos, n_pos, D, flags, kind, scale=0, quote=0, si=None, sk=None, m=None):
    """A whole call: `flags` is the call's flags word (BRX_TAKE_* and BRX_PARSE_* bits), `quote` the call's byte (ignored without
    QUOTED).  -> (val, status, L), L the records' lengths under tests/take_oracle.py."""
    src, L = take_oracle.take_vec(arena, off, length, count, pos_off, pos, n_pos, D, flags & 3, si, sk, m)
    val, status = parse_records(form, arena, src, L, kind, scale, bool(flags & SPACES), quote if flags & QUOTED else None)
    return val, status, L


# ---- the check values of the contract: (record, kind, scale, flags, val, status), quote '"' where QUOTED -----------------------------
_Z45 = b"0" * 45
CHECK = [
    (b"0", INT, 0, 0, 0, OK), (b"-0", INT, 0, 0, 0, OK), (b"+17", INT, 0, 0, 17, OK), (b"9223372036854775807", INT, 0, 0, MAX, OK),
    (b"9223372036854775808", INT, 0, 0, MAX, RANGE), (b"-9223372036854775808", INT, 0, 0, MIN, OK),
    (b"-9223372036854775809", INT, 0, 0, MIN, RANGE), (_Z45 + b"9223372036854775807", INT, 0, 0, MAX, OK),
    (_Z45 + b"09223372036854775807", INT, 0, 0, 0, LONG), (b"12.5", INT, 0, 0, 0, BAD), (b"", INT, 0, 0, 0, EMPTY), (b"-", INT, 0, 0, 0, BAD),
    (b"1 ", INT, 0, 0, 0, BAD),
    (b"12.34", DEC, 2, 0, 1234, OK), (b"12.345", DEC, 2, 0, 1234, INEXACT), (b"12.340", DEC, 2, 0, 1234, OK), (b"-.5", DEC, 2, 0, -50, OK),
    (b"5.", DEC, 2, 0, 500, OK), (b".", DEC, 2, 0, 0, BAD), (b"-0.009", DEC, 2, 0, 0, INEXACT), (b"1e3", DEC, 2, 0, 0, BAD),
    (b"92233720368547758.07", DEC, 2, 0, MAX, OK), (b"92233720368547758.08", DEC, 2, 0, MAX, RANGE),
    (b"-92233720368547758.089", DEC, 2, 0, MIN, INEXACT),
    (b"12.5", DEC, 0, 0, 12, INEXACT), (b"9.223372036854775807", DEC, 18, 0, MAX, OK), (b"9.3", DEC, 18, 0, MAX, RANGE),
    (b"ff", HEX, 0, 0, 255, OK), (b"0xFFFFFFFFFFFFFFFF", HEX, 0, 0, -1, OK), (b"0x10000000000000000", HEX, 0, 0, -1, RANGE),
    (b"0x", HEX, 0, 0, 0, BAD), (b"x1", HEX, 0, 0, 0, BAD), (b"0X0000000000000000000000001f", HEX, 0, 0, 31, OK),
    (b' "42"\t', INT, 0, SPACES | QUOTED, 42, OK), (b'" 42"', INT, 0, SPACES | QUOTED, 0, BAD), (b'"42', INT, 0, SPACES | QUOTED, 0, BAD),
    (b'"', INT, 0, SPACES | QUOTED, 0, BAD), (b'""', INT, 0, SPACES | QUOTED, 0, EMPTY), (b"  ", INT, 0, SPACES | QUOTED, 0, EMPTY),
]

# ---- records biased to the grammar's edges (for the tests' random sweeps) ------------------------------------------------------------
EDGES = [b"9223372036854775807", b"9223372036854775808", b"9223372036854775809", b"9223372036854775806", b"18446744073709551615",
         b"18446744073709551616", b"9999999999999999999", b"10000000000000000000", b"1000000000000000000", b"99999999", b"100000000",
         b"9999999999999999", b"10000000000000000", b"0", b"00", b"1"]
CORNERS = [b"", b"-", b"+", b".", b"-.", b"0x", b"0X", b"x1", b'"', b'""', b'"""', b" ", b"  ", b"\t", b"1 ", b" 1", b"1e3", b"+-1", b"--1",
           b"1.2.3", b"5.", b".5", b"-0", b"+0", b"-0.009", b"0x0", b"00x1", b"0xg", b'" 42"', b'"42', b'42"', b".0", b"0.", b"-.0", b"1,2"]
JUNK = b"0123456789+-. \t\"'xXabfABFgG,eE\r_\x80\xb0\xff\x00/:@`"


def random_field(rng, quote=0x22):
    """One record (no 0x0A in it) from a generator biased to where the grammar and the arithmetic turn: digit counts around 8, 16, 19
    and 20, values around 2^63 and 2^64, the point anywhere, leading zeros up to and past the 64 bytes, blanks and quotes around."""
    form = int(rng.integers(0, 9))
    if form == 0:
        return bytes(JUNK[int(i)] for i in rng.integers(0, len(JUNK), int(rng.integers(0, 70))))
    if form <= 3:
        d = EDGES[int(rng.integers(0, len(EDGES)))] if rng.integers(0, 3) == 0 else bytes(rng.integers(0x30, 0x3A, int(rng.integers(1, 22))).astype(np.uint8))
        if rng.integers(0, 3) == 0:
            d = b"0" * int(rng.integers(0, 50)) + d
        if rng.integers(0, 3) == 0:
            d += (b"", b"0", b"00", b"01", b"000")[int(rng.integers(0, 5))]
        if form >= 2:
            k = int(rng.integers(0, len(d) + 1))
            d = d[:k] + b"." + d[k:]
        if rng.integers(0, 3) == 0:
            d = (b"-", b"+")[int(rng.integers(0, 2))] + d
    elif form <= 5:
        d = bytes(b"0123456789abcdefABCDEF"[int(i)] for i in rng.integers(0, 22, int(rng.integers(1, 20))))
        if rng.integers(0, 3) == 0:
            d = (b"f", b"F")[int(rng.integers(0, 2))] * int(rng.integers(15, 18))
        if rng.integers(0, 3) == 0:
            d = b"0" * int(rng.integers(0, 48)) + d
        if rng.integers(0, 2):
            d = (b"0x", b"0X")[int(rng.integers(0, 2))] + d
    elif form == 6:
        d = CORNERS[int(rng.integers(0, len(CORNERS)))]
    else:
        d = bytes(rng.integers(0x30, 0x3A, int(rng.integers(1, 10))).astype(np.uint8))
    q = bytes([quote])
    if rng.integers(0, 4) == 0:
        d = q + d + q
    if rng.integers(0, 4) == 0:
        d = (b" ", b"\t")[int(rng.integers(0, 2))] * int(rng.integers(0, 20)) + d + (b" ", b"\t")[int(rng.integers(0, 2))] * int(rng.integers(0, 20))
    if rng.integers(0, 10) == 0:
        d = q + d + q
    return d
