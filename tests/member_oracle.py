"""THE RULE of brx_member_batch (include/brx.h), stated twice and independently, plus what the tests of the call share: the structural
index of a JSON Lines text on the CPU, the check values of the contract, a fixed-seed generator of JSON Lines and the comparison
with json.loads.

  members_boundaries  walks the boundaries (pos, what) of a stream in order, as the contract words it: depth from `what`, the key
                      record of a depth-1 ':' from `pos` under take's rule, the value's kind from the next boundary.
  members_bytes       walks the BYTES of the stream and never sees pos or what: a small reader of JSON-ish text that keeps the
                      string state, the depth, the text since the last structural byte and the number of structural bytes so far.

Both return (lines, per line {name: (kind, rec)}, per line flags) for one stream."""
import json

import numpy as np

MISSING, SCALAR, OBJECT, ARRAY, BAD = 0, 1, 2, 3, 4
KIND_NAMES = {MISSING: "MISSING", SCALAR: "SCALAR", OBJECT: "OBJECT", ARRAY: "ARRAY", BAD: "BAD"}
LONG_KEY, ESCAPED_KEY, UNBALANCED = 1, 2, 4
MAX_NAMES, MAX_NAME, MAX_KEY = 8, 32, 64
NONE = (1 << 64) - 1  # sel_rec of MISSING
SET = b"{}[]:,\n"
BLANKS = b" \t\r"


def index_set(s, delims=SET, quote=0x22, escape=0x5C):
    """pos, what of brx_index_set_batch for one stream (its rule restated: include/brx.h)."""
    pos, what = [], bytearray()
    esc, quotes = False, 0
    for j, c in enumerate(s):
        if esc:
            esc = False
            continue
        if c == escape:
            esc = True
        elif c == quote:
            quotes += 1
        elif c in delims and quotes % 2 == 0:
            pos.append(j)
            what.append(c)
    return pos, bytes(what)


def _key_of(record, names):
    """(index of the name the key record carries or None, flag bits) -- of the boundary-serial statement only"""
    if len(record) > MAX_KEY:
        return None, LONG_KEY
    flags = ESCAPED_KEY if b"\\" in record else 0
    t = record.strip(BLANKS)
    if len(t) >= 2 and t[:1] == b'"' and t[-1:] == b'"' and t[1:-1] in names:
        return names.index(t[1:-1]), flags
    return None, flags


def _kind_of(w):
    return SCALAR if w in b",}" else OBJECT if w == b"{" else ARRAY if w == b"[" else BAD


def members_boundaries(s, pos, what, names, count=None, n_pos=None):
    """The boundary-serial statement.  count / n_pos: as the call's (boundaries at or behind n_pos are neutral and not looked at)."""
    count = len(pos) if count is None else count
    n_pos = len(pos) if n_pos is None else n_pos
    l = len(s)

    def w(k):
        return what[k:k + 1] if k < min(count, n_pos) else b"\0"

    def P(k):
        return min(pos[k], l) if k < n_pos else l

    found, flags, d, cur, f = [], [], 0, {}, 0
    for k in range(count):
        c = w(k)
        if c == b"\n":
            if d != 0:
                f |= UNBALANCED
            found.append(cur)
            flags.append(f)
            d, cur, f = 0, {}, 0
            continue
        if c in b"{[":
            d += 1
        elif c in b"}]":
            d -= 1
            if d < 0:
                f |= UNBALANCED
        elif c == b":" and d == 1:
            start = min(P(k - 1) + 1, l) if k > 0 else 0
            end = max(P(k), start)
            q, bits = _key_of(s[start:end], names)
            f |= bits
            if q is not None:
                nxt = w(k + 1) if k + 1 < count else b"\0"
                cur[q] = (_kind_of(nxt) if nxt != b"\0" else BAD, k + 1)
    if d != 0:
        f |= UNBALANCED
    found.append(cur)
    flags.append(f)
    return len(found), found, flags


_BYTES_KINDS = {0x2C: SCALAR, 0x7D: SCALAR, 0x7B: OBJECT, 0x5B: ARRAY}  # the byte-serial statement's own: what follows the ':'


def _bytes_key(since, names):
    """The byte-serial statement's own look at a key: the index of the name between the quotes, or None.  Shares nothing with
    _key_of: the blanks are skipped from both ends by index, the name is compared byte by byte."""
    if len(since) > 64:
        return None
    a, b = 0, len(since)
    while a < b and since[a] in (0x20, 0x09, 0x0D):
        a += 1
    while b > a and since[b - 1] in (0x20, 0x09, 0x0D):
        b -= 1
    if b - a < 2 or since[a] != 0x22 or since[b - 1] != 0x22:
        return None
    for q, nm in enumerate(names):
        if len(nm) == b - a - 2 and all(since[a + 1 + t] == nm[t] for t in range(len(nm))):
            return q
    return None


def members_bytes(s, names):
    """The byte-serial statement: no pos, no what."""
    found, flags = [], []
    d, cur, f = 0, {}, 0
    in_str, esc = False, False
    since = bytearray()  # the bytes since the last structural byte: a key record when a ':' ends them
    nb = 0               # structural bytes so far in the stream: the next one is boundary nb
    pending = None       # name index of a depth-1 member whose value's kind the next structural byte tells
    for c in s:
        ch = bytes([c])
        if esc:
            esc = False
            since += ch
            continue
        if c == 0x5C:
            esc = True
            since += ch
            continue
        if c == 0x22:
            in_str = not in_str
            since += ch
            continue
        if in_str or ch not in (b"{", b"}", b"[", b"]", b":", b",", b"\n"):
            since += ch
            continue
        if pending is not None:
            cur[pending] = (_BYTES_KINDS.get(c, BAD), nb)
            pending = None
        if ch == b"\n":
            if d != 0:
                f |= UNBALANCED
            found.append(cur)
            flags.append(f)
            d, cur, f = 0, {}, 0
        elif ch in b"{[":
            d += 1
        elif ch in b"}]":
            d -= 1
            if d < 0:
                f |= UNBALANCED
        elif ch == b":" and d == 1:
            q = _bytes_key(since, names)
            if len(since) > 64:
                f |= LONG_KEY
            elif 0x5C in since:
                f |= ESCAPED_KEY
            if q is not None:
                pending = q
                cur[q] = (BAD, nb + 1)  # unless another structural byte follows in the line
        nb += 1
        since = bytearray()
    if d != 0:
        f |= UNBALANCED
    found.append(cur)
    flags.append(f)
    return len(found), found, flags


FORMS = {"boundaries": lambda s, names: members_boundaries(s, *index_set(s), names), "bytes": members_bytes}


def batch(streams, names, form="boundaries"):
    """The call's outputs for a batch: lines [n], line_off [n], sel_stream, sel_rec, kind [Q, M] and line_flags [M] as numpy arrays."""
    per = [FORMS[form](s, names) for s in streams]
    lines = np.array([p[0] for p in per], dtype=np.int64)
    line_off = np.cumsum(lines) - lines
    M, Q = int(lines.sum()), len(names)
    sel_stream = np.zeros((Q, M), dtype=np.int64)
    sel_rec = np.full((Q, M), NONE, dtype=np.uint64)
    kind = np.zeros((Q, M), dtype=np.uint8)
    line_flags = np.zeros(M, dtype=np.uint8)
    for i, (_, found, flags) in enumerate(per):
        for r, (cur, f) in enumerate(zip(found, flags)):
            j = int(line_off[i]) + r
            sel_stream[:, j] = i
            line_flags[j] = f
            for q, (kd, rec) in cur.items():
                kind[q, j] = kd
                sel_rec[q, j] = rec
    return lines, line_off, sel_stream, sel_rec, kind, line_flags


def record(s, pos, k):
    """record k of the stream under BRX_TAKE_NO_DELIM, D = 1"""
    start = min(pos[k - 1] + 1, len(s)) if k > 0 else 0
    end = pos[k] if k < len(pos) else len(s)
    return s[start:max(end, start)]


# ---- the check values of the contract: (stream, names, per line ({name: (kind, rec)}, flags)) -------------------------------------
CHECK_STREAM = b'{"a":"x,\\"y:}","b":[1,2]}\n{"c":"\\\\"}\n{"open":"[\\'
K32 = b"k" * 32
CHECK = [
    (CHECK_STREAM, [b"a", b"b", b"c", b"open"],
     [({b"a": (SCALAR, 2), b"b": (ARRAY, 4)}, 0), ({b"c": (SCALAR, 11)}, 0), ({b"open": (BAD, 15)}, UNBALANCED)]),
    (b'{"a":1,"a":2}', [b"a"], [({b"a": (SCALAR, 4)}, 0)]),
    (b'{"user":{"text":1},"text":2}', [b"text", b"user"], [({b"text": (SCALAR, 7), b"user": (OBJECT, 2)}, 0)]),
    (b'{ "a"\t:1}', [b"a"], [({b"a": (SCALAR, 2)}, 0)]),
    (b"{" + b" " * 30 + b'"' + K32 + b'":1}', [K32], [({K32: (SCALAR, 2)}, 0)]),
    (b"{" + b" " * 31 + b'"' + K32 + b'":1}', [K32], [({}, LONG_KEY)]),
    (b'{"a":1}}', [b"a"], [({b"a": (SCALAR, 2)}, UNBALANCED)]),
    (b'}{"a":1}', [b"a"], [({}, UNBALANCED)]),
    (b'{"a\\u0062":1}\n', [b"ab"], [({}, ESCAPED_KEY), ({}, 0)]),
]


def header_form(stream, names, want):
    """One check value as include/brx.h prints it (blanks squeezed, a run of n > 8 equal bytes as <n x c>)."""
    out, i = "", 0
    text = stream.decode("ascii")
    while i < len(text):
        j = i
        while j < len(text) and text[j] == text[i]:
            j += 1
        c = {"\n": "\\n", "\t": "<09>"}.get(text[i], text[i])
        out += "<%d x %s>" % (j - i, "20" if c == " " else c) if j - i > 8 else c * (j - i)
        i = j
    parts = []
    for r, (cur, f) in enumerate(want):
        vals = " ".join("%s %s %d" % ("k32" if nm == K32 else nm.decode(), KIND_NAMES[kd], rec) for nm, (kd, rec) in sorted(cur.items()))
        parts.append("line %d: %s flags %d" % (r, vals if vals else "none", f))
    return " ".join(("[%s] %s" % (out, "; ".join(parts))).split())


# ---- a generator of JSON Lines with a fixed seed ------------------------------------------------------------------------------------
KEYS = [b"id", b"text", b"user", b"tags", b"score", b"lang", b"k", b"a_rather_long_key_of_32_bytes_xx", b"ts", b"ok", b"note", b"geo"]
assert len(KEYS[7]) == 32


def _scalar(rng):
    t = int(rng.integers(0, 8))
    if t == 0:
        return str(int(rng.integers(-10**9, 10**9))).encode()
    if t == 1:
        return b"%.3f" % float(rng.uniform(-100, 100))
    if t == 2:
        return (b"true", b"false", b"null")[int(rng.integers(0, 3))]
    alphabet = [b"a", b"b", b" ", b",", b":", b"{", b"}", b"[", b"]", b'\\"', b"\\\\", b"\\n", b"\\u00e9", b"x", b"Z", b"0"]
    return b'"' + b"".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), int(rng.integers(0, 12)))) + b'"'


def _value(rng, depth):
    t = int(rng.integers(0, 10))
    if depth < 2 and t == 0:
        return b"{" + b",".join(b'"' + KEYS[int(rng.integers(0, len(KEYS)))] + b'":' + _value(rng, depth + 1)
                                for _ in range(int(rng.integers(0, 4)))) + b"}"
    if depth < 2 and t == 1:
        return b"[" + b",".join(_value(rng, depth + 1) for _ in range(int(rng.integers(0, 4)))) + b"]"
    return _scalar(rng)


def gen_line(rng):
    """One line without its line feed.  About 19 of 20 are JSON objects that json.loads can be asked about (keys in any order, optional, some duplicated, blanks around
    keys and values, nested values that repeat key names); the rest are broken on purpose."""
    nk = int(rng.integers(0, 7))
    keys = [KEYS[int(x)] for x in rng.integers(0, len(KEYS), nk)]  # (with repeats: duplicates)
    blank = lambda: (b"", b"", b"", b" ", b"\t", b" \r")[int(rng.integers(0, 6))]
    body = b",".join(blank() + b'"' + k + b'"' + blank() + b":" + blank() + _value(rng, 0) + blank() for k in keys)
    line = b"{" + body + b"}"
    t = int(rng.integers(0, 100))
    if t == 0:
        line = line[:int(rng.integers(0, len(line) + 1))]  # cut
    elif t == 1:
        line = line + b"}"
    elif t == 2:
        line = b"[" + line + b"," + line + b"]"  # an array as the line
    elif t == 3:
        line = b""
    elif t == 4:
        line = b'{"a\\u0062":1,' + line[1:] if len(line) > 2 else line
    elif t == 5:
        line = b"{" + b" " * int(rng.integers(25, 40)) + b'"' + KEYS[7] + b'":1' + (b"," + line[1:] if len(line) > 2 else b"}")
    return line


def gen_stream(rng, n_lines, final_lf=None):
    lines = [gen_line(rng) for _ in range(n_lines)]
    s = b"\n".join(lines)
    if n_lines and (final_lf if final_lf is not None else bool(rng.integers(0, 2))):
        s += b"\n"
    return s


def json_view(line, names):
    """What json.loads says of a line that is valid JSON with an object on top: {name: the value} for the names present (the LAST of
    duplicates), or None where the comparison does not apply."""
    try:
        pairs = json.loads(line.decode("utf-8"), object_pairs_hook=lambda p: p)
    except ValueError:
        return None
    if not isinstance(pairs, list) or (pairs and not all(isinstance(p, tuple) and len(p) == 2 and isinstance(p[0], str) for p in pairs)):
        return None
    if line.strip(b" \t\r")[:1] != b"{":
        return None
    got = {}
    for k, v in pairs:
        if k.encode() in names:
            got[k.encode()] = v
    return got


def agrees_with_json(line, names, cur, flags):
    """True / False where json.loads applies to the line (None where it does not): the same names are present, a scalar member's
    record is the bytes json.loads reads that value from, a nested one has the right kind.  A key with an escape is not resolved by the
    rule and a long key is not looked at, so lines with ESCAPED_KEY or LONG_KEY are left out."""
    view = json_view(line, names)
    if view is None or flags & (ESCAPED_KEY | LONG_KEY):
        return None
    if flags != 0:
        return False  # valid JSON has balanced brackets
    pos, _ = index_set(line)
    if set(view) != set(names[q] for q in cur):
        return False
    for q, (kd, rec) in cur.items():
        v = view[names[q]]
        if isinstance(v, list):  # (object_pairs_hook: an object is a list of pairs, an empty one [] as an empty array is)
            want = (OBJECT, ARRAY) if not v else (OBJECT,) if isinstance(v[0], tuple) else (ARRAY,)
            if kd not in want:
                return False
            continue
        if kd != SCALAR:
            return False
        try:
            if json.loads(record(line, pos, rec).decode("utf-8")) != v:
                return False
        except ValueError:
            return False
    return True
