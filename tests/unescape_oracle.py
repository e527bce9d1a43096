"""THE TEXT of brx_unescape_batch (include/brx.h) on the CPU, twice: `text_serial` is the byte-serial walk as the contract words it, a
direct transcription with nothing vectorised; `text_re` tokenises with regular expressions (and bytes.replace for CSV) and leaves the
UTF-8 to Python.  tests/test_unescape_abi.py holds the two to each other, to the contract's table and to json / csv of the standard
library; tests/test_gpu_unescape.py takes every expected value from here.  `unescape_take` composes with tests/take_oracle.py."""
import re

import numpy as np

import take_oracle

CSV, JSON, BACKSLASH = 0, 1, 2
OK, BARE, NULL, BAD = 0, 1, 2, 3
SPACES = 16  # BRX_PARSE_SPACES
QT, ESC = 0x22, 0x5C
BLANKS = b" \t"


def _trim(r, spaces):
    r = bytes(r)
    return r.strip(BLANKS) if spaces else r


# ---- form 1: the walk ---------------------------------------------------------------------------------------------------------------
def _hex4(t, i):
    """the code unit of t[i .. i + 4), or None where that does not lie inside t or is not four hex digits"""
    if i + 4 > len(t):
        return None
    v = 0
    for c in t[i:i + 4]:
        if 0x30 <= c <= 0x39:
            d = c - 0x30
        elif 0x61 <= c <= 0x66:
            d = c - 0x61 + 10
        elif 0x41 <= c <= 0x46:
            d = c - 0x41 + 10
        else:
            return None
        v = v * 16 + d
    return v


def _utf8(cp):
    if cp < 0x80:
        return bytes([cp])
    if cp < 0x800:
        return bytes([0xC0 | cp >> 6, 0x80 | cp & 63])
    if cp < 0x10000:
        return bytes([0xE0 | cp >> 12, 0x80 | cp >> 6 & 63, 0x80 | cp & 63])
    return bytes([0xF0 | cp >> 18, 0x80 | cp >> 12 & 63, 0x80 | cp >> 6 & 63, 0x80 | cp & 63])


def text_serial(r, dialect, q=QT, e=ESC, spaces=False):
    """-> (text, status)"""
    t = _trim(r, spaces)
    T = len(t)
    u = bytearray()
    bad = False
    if dialect == CSV:
        if T == 0 or t[0] != q:
            return t, BARE
        if T < 2 or t[T - 1] != q:
            return t, BAD
        i = 1
        while i < T - 1:
            if t[i] == q:
                if i + 1 < T - 1 and t[i + 1] == q:
                    u.append(q)
                    i += 2
                    continue
                bad = True
            u.append(t[i])
            i += 1
        return bytes(u), BAD if bad else OK
    if dialect == JSON:
        if T == 0 or t[0] != q:
            return t, BARE
        i, closed = 1, False
        while i < T:
            b = t[i]
            if b == e:
                if i == T - 1:
                    u.append(e)
                    bad = True
                    i += 1
                    continue
                c = t[i + 1]
                if c == q or c == e or c == 0x2F:
                    u.append(c)
                    i += 2
                    continue
                if c in b"bfnrt":
                    u.append(b"\x08\x0c\x0a\x0d\x09"[b"bfnrt".index(c)])
                    i += 2
                    continue
                cu = _hex4(t, i + 2) if c == 0x75 else None
                if cu is None:
                    u.append(e)
                    bad = True
                    i += 1
                    continue
                if not 0xD800 <= cu <= 0xDFFF:
                    u += _utf8(cu)
                    i += 6
                    continue
                if cu <= 0xDBFF and i + 12 <= T and t[i + 6] == e and t[i + 7] == 0x75:
                    lo = _hex4(t, i + 8)
                    if lo is not None and 0xDC00 <= lo <= 0xDFFF:
                        u += _utf8(0x10000 + ((cu - 0xD800) << 10) + (lo - 0xDC00))
                        i += 12
                        continue
                u += b"\xef\xbf\xbd"
                bad = True
                i += 6
                continue
            if b == q:
                if i == T - 1:
                    closed = True
                    break
                bad = True
            u.append(b)
            i += 1
        return bytes(u), BAD if bad or not closed else OK
    if T == 2 and t[0] == e and t[1] == 0x4E:
        return b"", NULL
    i = 0
    while i < T:
        if t[i] == e:
            if i == T - 1:
                u.append(e)
                bad = True
                i += 1
                continue
            c = t[i + 1]
            u.append(b"\x08\x0c\x0a\x0d\x09\x0b\x00"[b"bfnrtv0".index(c)] if c in b"bfnrtv0" else c)
            i += 2
            continue
        u.append(t[i])
        i += 1
    return bytes(u), BAD if bad else OK


# ---- form 2: tokens by regular expression ---------------------------------------------------------------------------------------
_RE = {}
_H = b"[0-9a-fA-F]"


def _json_re(q, e):
    if (q, e) not in _RE:
        Q, E = re.escape(bytes([q])), re.escape(bytes([e]))
        _RE[q, e] = re.compile(b"(?s)(?P<c>" + E + b"(?:" + Q + b"|" + E + b"|/))|(?P<n>" + E + b"[bfnrt])"
                               b"|(?P<p>" + E + b"u[dD][89abAB]" + _H + b"{2}" + E + b"u[dD][c-fC-F]" + _H + b"{2})"
                               b"|(?P<u>" + E + b"u" + _H + b"{4})|(?P<e>" + E + b")|(?P<q>" + Q + b")|(?P<t>[^" + Q + E + b"]+)")
    return _RE[q, e]


def text_re(r, dialect, q=QT, e=ESC, spaces=False):
    """-> (text, status), by other means than text_serial"""
    t = _trim(r, spaces)
    Q, E = bytes([q]), bytes([e])
    if dialect == BACKSLASH:
        if t == E + b"N":
            return b"", NULL
        table = dict(zip(b"bfnrtv0", b"\x08\x0c\x0a\x0d\x09\x0b\x00"))
        parts = re.split(b"(?s)" + re.escape(E) + b"(.)", t)  # plain, escaped byte, plain, ...
        last = parts[-1]
        out = b"".join(p if k % 2 == 0 else bytes([table.get(p[0], p[0])]) for k, p in enumerate(parts))
        return out, BAD if last.endswith(E) else OK
    if not t.startswith(Q):
        return t, BARE
    if dialect == CSV:
        if len(t) < 2 or not t.endswith(Q):
            return t, BAD
        body = t[1:-1]
        return body.replace(Q + Q, Q), BAD if Q in body.replace(Q + Q, b"") else OK
    out, bad, closed = [], False, False
    for m in _json_re(q, e).finditer(t, 1):
        kind, s = m.lastgroup, m.group()
        if kind == "c":
            out.append(s[1:])
        elif kind == "n":
            out.append({0x62: b"\b", 0x66: b"\f", 0x6E: b"\n", 0x72: b"\r", 0x74: b"\t"}[s[1]])
        elif kind == "p":
            out.append((chr(int(s[2:6], 16)) + chr(int(s[8:12], 16))).encode("utf-16", "surrogatepass").decode("utf-16").encode("utf-8"))
        elif kind == "u":
            cu = int(s[2:6], 16)
            if 0xD800 <= cu <= 0xDFFF:
                out.append(b"\xef\xbf\xbd")
                bad = True
            else:
                out.append(chr(cu).encode("utf-8"))
        elif kind == "e":
            out.append(E)
            bad = True
        elif kind == "q":
            if m.start() == len(t) - 1:
                closed = True
                break
            out.append(Q)
            bad = True
        else:
            out.append(s)
    return b"".join(out), BAD if bad or not closed else OK


FORMS = {"serial": text_serial, "re": text_re}


# ---- whole calls ----------------------------------------------------------------------------------------------------------------
def unescape_take(form, arena, off, length, count, pos_off, pos, n_pos, D, flags, dialect, q=QT, e=ESC, si=None, sk=None, m=None):
    """A whole call: `flags` is the call's flags word (BRX_TAKE_* bits and SPACES).  -> (texts, text_len, status, L): the list of the
    entries' texts, their lengths and statuses as arrays, and the records' lengths under tests/take_oracle.py."""
    src, L = take_oracle.take_vec(arena, off, length, count, pos_off, pos, n_pos, D, flags & 3, si, sk, m)
    host = np.asarray(arena, dtype=np.uint8).tobytes()
    f, memo, res = FORMS[form], {}, []
    for s, ln in zip(src, L):  # (a batch often holds one record many times)
        r = host[int(s):int(s) + int(ln)]
        if r not in memo:
            memo[r] = f(r, dialect, q, e, bool(flags & SPACES))
        res.append(memo[r])
    texts = [x[0] for x in res]
    return texts, np.array([len(x) for x in texts], dtype=np.int64), np.array([x[1] for x in res], dtype=np.uint8), np.asarray(L, dtype=np.int64)


def fill(texts, dst_off, total, dst):
    """dst (a uint8 array, changed in place and returned): the rule of fill mode, the room of brx_take_batch."""
    m = len(texts)
    for j, u in enumerate(texts):
        s = int(dst_off[j])
        en = min(int(dst_off[j + 1]) if j + 1 < m else total, total)
        k = max(min(len(u), en - s), 0)
        if k:
            dst[s:s + k] = np.frombuffer(u[:k], dtype=np.uint8)
    return dst


# ---- records rich in everything the walk branches on ------------------------------------------------------------------------------
_FRAG = ["En", "EE", "EQ", "E/", "Eb", "Et", "Ef", "Er", "Eu00e9", "Eu00E9", "Eu0041", "Eu0000", "Eu20AC", "Eud83dEude00", "EuD83DEuDE00",
         "Eud83d", "Eude00", "Eud83dEu0041", "Eud83dEud83dEude00", "EEud83d", "Eu12", "Eu12g4", "Ex", "E", "Q", "QQ", "QQQ", "u", "d83d",
         "N", "EN", " ", "\t", "Ev", "E0", "Eud83dE", "Eud83dEu", "Eud83dEude0", ",", "0", "9", "a", "F"]


def rich_record(rng, length, dialect, q=QT, e=ESC, rich=0.5, quoted=0.85):
    """a record of exactly `length` bytes"""
    out = bytearray()
    if dialect != BACKSLASH and rng.random() < quoted:
        out.append(q)
    run = q if dialect == CSV else e
    while len(out) < length:
        x = rng.random()
        if x < rich / 6:
            out += bytes([run]) * int(rng.integers(1, 41))
        elif x < rich:
            out += bytes(e if c == "E" else q if c == "Q" else ord(c) for c in _FRAG[int(rng.integers(0, len(_FRAG)))])
        else:
            out += bytes(rng.integers(0x61, 0x7B, int(rng.integers(1, 40))).astype(np.uint8))
    out = out[:length]
    if length >= 2 and dialect != BACKSLASH and rng.random() < quoted:
        out[-1] = q
    return bytes(out)


# ---- the check values of the contract: (dialect, spaces, record, text, status) ----------------------------------------------------
CHECK = [
    (JSON, False, b'"a\\tb"', b"a\tb", OK), (JSON, False, b'"\\u00e9"', b"\xc3\xa9", OK), (JSON, False, b'"\\ud83d\\ude00"', b"\xf0\x9f\x98\x80", OK),
    (JSON, False, b'"\\\\"', b"\\", OK), (JSON, False, b'""', b"", OK), (JSON, False, b"null", b"null", BARE),
    (JSON, False, b'"\\ud83d"', b"\xef\xbf\xbd", BAD), (JSON, False, b'"\\ud83d\\u0041"', b"\xef\xbf\xbdA", BAD),
    (JSON, False, b'"\\ude00x"', b"\xef\xbf\xbdx", BAD), (JSON, False, b'"\\u12"', b"\\u12", BAD), (JSON, False, b'"\\x"', b"\\x", BAD),
    (JSON, False, b'"a"b"', b'a"b', BAD), (JSON, False, b'"abc\\"', b'abc"', BAD), (JSON, False, b'"abc', b"abc", BAD),
    (JSON, False, b'"', b"", BAD), (JSON, True, b' "x"\t', b"x", OK),
    (CSV, False, b'"a""b"', b'a"b', OK), (CSV, False, b'""""', b'"', OK), (CSV, False, b'""', b"", OK), (CSV, False, b"", b"", BARE),
    (CSV, False, b"abc", b"abc", BARE), (CSV, False, b'"""', b'"', BAD), (CSV, False, b'"a"b"', b'a"b', BAD), (CSV, False, b'"abc', b'"abc', BAD),
    (CSV, False, b'"', b'"', BAD),
    (BACKSLASH, False, b"a\\tb", b"a\tb", OK), (BACKSLASH, False, b"\\,", b",", OK), (BACKSLASH, False, b"\\\\N", b"\\N", OK),
    (BACKSLASH, False, b"x\\N", b"xN", OK), (BACKSLASH, False, b"\\N", b"", NULL), (BACKSLASH, False, b"a\\", b"a\\", BAD),
]


def header_form(dialect, spaces, rec, text, status):
    """a check value as include/brx.h prints it"""
    def show(b, is_text):
        if is_text and not b:
            return "empty"
        if is_text and any(c < 0x20 or c > 0x7E for c in b) or (is_text and rec in (b'"\\\\"',)):
            return " ".join("%02X" % c for c in b)
        return "[" + b.decode("ascii").replace("\t", "<09>") + "]"
    return "%s %s / %s" % (show(rec, False), show(text, True), ("OK", "BARE", "NULL", "BAD")[status])
