"""THE RULE of brx_elements_batch (include/brx.h), stated twice and independently, plus what the tests of the call share: the check
values of the contract, a fixed-seed generator of JSON Lines with an array under a known key and the comparison with json.loads.

  elements_boundaries  walks the boundaries (pos, what) of a stream behind an opener, as the contract words it: relative depth from
                       `what`, an element's kind from the boundary behind its separator, the blank test of `[]` from `pos`.
  elements_bytes       walks the BYTES of the stream and never sees pos or what: a small reader that keeps the string state, the
                       depth, the number of structural bytes so far and what stands between them.

Both return (status, end, [(el_rec, kind), ...]) for one (stream, r).  The index of a text, a record and the members of a line are
tests/member_oracle.py's."""
import json

import numpy as np

from member_oracle import ARRAY, BAD, OBJECT, SCALAR, index_set, members_boundaries, record  # noqa: F401  (shared with the tests)

OK, NONE, NOT_ARRAY, UNCLOSED, MISMATCH = 0, 1, 2, 3, 4
STATUS_NAMES = {OK: "OK", NONE: "NONE", NOT_ARRAY: "NOT_ARRAY", UNCLOSED: "UNCLOSED", MISMATCH: "MISMATCH"}
KIND_NAMES = {SCALAR: "SCALAR", OBJECT: "OBJECT", ARRAY: "ARRAY", BAD: "BAD"}
NO_END = (1 << 64) - 1
MAX_BLANK = 64
BLANKS = b" \t\r"


def _kind_of(w):
    return SCALAR if w in (b",", b"]", b"}") else OBJECT if w == b"{" else ARRAY if w == b"[" else BAD


def elements_boundaries(s, pos, what, r, count=None, n_pos=None):
    """The boundary-serial statement.  pos / what: the stream's part of the tables (as far as they go); count / n_pos: as the call's,
    n_pos counted from the stream's first boundary (boundaries at or behind it do not count and are not looked at)."""
    count = len(pos) if count is None else count
    n_pos = len(pos) if n_pos is None else n_pos
    C, l = min(count, max(n_pos, 0)), len(s)

    def P(k):
        return min(pos[k], l) if k < n_pos else l

    if r >= C:
        return NONE, NO_END, []
    if what[r:r + 1] != b"[":
        return NOT_ARRAY, NO_END, []
    els, e, sep, k = [], 1, r, r + 1
    while True:
        if k == C:
            return UNCLOSED, C, els
        w = what[k:k + 1]
        if w == b"\n":
            return UNCLOSED, k, els
        if w in (b"{", b"["):
            e += 1
        elif w in (b"}", b"]"):
            e -= 1
            if e == 0:
                status = OK if w == b"]" else MISMATCH
                if k == r + 1:  # `[]` and `[1]` look alike in what: record r + 1 tells them apart
                    start = min(P(k - 1) + 1, l)
                    rec = s[start:max(P(k), start)]
                    if len(rec) <= MAX_BLANK and not rec.strip(BLANKS):
                        return status, k, []
                els.append((sep + 1, _kind_of(what[sep + 1:sep + 2])))
                return status, k, els
        elif w == b"," and e == 1:
            els.append((sep + 1, _kind_of(what[sep + 1:sep + 2])))
            sep = k
        k += 1


_BYTES_KINDS = {0x2C: SCALAR, 0x5D: SCALAR, 0x7D: SCALAR, 0x7B: OBJECT, 0x5B: ARRAY}


def elements_bytes(s, r):
    """The byte-serial statement: no pos, no what.  The r-th structural byte outside strings is the opener."""
    in_str = esc = False
    nb = 0          # structural bytes so far: the next one is boundary nb
    state = None    # None: in front of the opener; else the walk's [depth, kind of the element in hand or None, its first boundary]
    els, since = [], 0  # `since`: the non-blank bytes since the last structural byte, and how many bytes in all (for the blank test)
    total_since = 0
    for c in s:
        structural = False
        if esc:
            esc = False
        elif c == 0x5C:
            esc = True
        elif c == 0x22:
            in_str = not in_str
        elif not in_str and c in b"{}[]:,\n":
            structural = True
        if not structural:
            total_since += 1
            if c not in (0x20, 0x09, 0x0D):
                since += 1
            continue
        if state is None:
            if nb == r:
                if c != 0x5B:
                    return NOT_ARRAY, NO_END, []
                state = [1, None, nb + 1]
        else:
            depth, kind, first = state
            if kind is None:  # the first structural byte behind the separator tells the element's kind
                kind = _BYTES_KINDS.get(c, BAD)
            if c == 0x0A:
                return UNCLOSED, nb, els
            if c in b"{[":
                depth += 1
            elif c in b"}]":
                depth -= 1
                if depth == 0:
                    status = OK if c == 0x5D else MISMATCH
                    if not (nb == r + 1 and since == 0 and total_since <= MAX_BLANK):
                        els.append((first, kind))
                    return status, nb, els
            elif c == 0x2C and depth == 1:
                els.append((first, kind))
                kind, first = None, nb + 1
            state = [depth, kind, first]
        nb += 1
        since = total_since = 0
    if state is None:
        return NONE, NO_END, []
    return UNCLOSED, nb, els


def form_boundaries(s, r):
    pos, what = index_set(s)
    return elements_boundaries(s, pos, what, r)


FORMS = {"boundaries": form_boundaries, "bytes": elements_bytes}

# ---- the check values of the contract: (stream, r, status, [(el_rec, kind)], end) ------------------------------------------------
CHECK = [
    (b'{"a":[]}', 2, OK, [], 3),
    (b'{"a":[ ]}', 2, OK, [], 3),
    (b'{"a":[1,]}', 2, OK, [(3, SCALAR), (4, SCALAR)], 4),
    (b'{"a":[1:2]}', 2, OK, [(3, BAD)], 4),
    (b'{"a":[1}', 2, MISMATCH, [(3, SCALAR)], 3),
    (b'{"a":[1,2\n', 2, UNCLOSED, [(3, SCALAR)], 4),
    (b'{"a":[1,[2', 2, UNCLOSED, [(3, SCALAR)], 5),
    (b'{"a":[[1,2],{"b":[3]},4]}', 2, OK, [(3, ARRAY), (7, OBJECT), (13, SCALAR)], 13),
    (b'{"a":["],[",2]}', 2, OK, [(3, SCALAR), (4, SCALAR)], 4),
    (b'{"a":[' + b" " * 64 + b"]}", 2, OK, [], 3),
    (b'{"a":[' + b" " * 65 + b"]}", 2, OK, [(3, SCALAR)], 3),
    (b'{"a":[,]}', 2, OK, [(3, SCALAR), (4, SCALAR)], 4),
    (b'{"a":{}}', 2, NOT_ARRAY, [], NO_END),
    (b'{"a":[1]}', 9, NONE, [], NO_END),
]


def header_form(stream, r, status, els, end):
    """One check value as include/brx.h prints it (a run of n > 8 equal bytes as <n x c>)."""
    out, i = "", 0
    text = stream.decode("ascii")
    while i < len(text):
        j = i
        while j < len(text) and text[j] == text[i]:
            j += 1
        c = {"\n": "\\n"}.get(text[i], text[i])
        out += "<%d x %s>" % (j - i, "20" if c == " " else c) if j - i > 8 else c * (j - i)
        i = j
    body = "".join("(%d %s)" % (rec, KIND_NAMES[kd]) for rec, kd in els)
    tail = " end %d" % end if end != NO_END else ""
    return "[%s] r %d: %s %d%s%s" % (out, r, STATUS_NAMES[status], len(els), " " + body if body else "", tail)


# ---- a generator of valid JSON Lines with an array under the key "arr" ---------------------------------------------------------------
_ALPHABET = ["a", "b", " ", ",", ":", "{", "}", "[", "]", '"', "\\", "\n", "é", "x", "],[", "0"]


def _gen_scalar(rng):
    t = int(rng.integers(0, 6))
    if t == 0:
        return int(rng.integers(-10**9, 10**9))
    if t == 1:
        return float(np.round(rng.uniform(-100, 100), int(rng.integers(0, 6))))
    if t == 2:
        return (True, False, None)[int(rng.integers(0, 3))]
    return "".join(_ALPHABET[int(x)] for x in rng.integers(0, len(_ALPHABET), int(rng.integers(0, 10))))


def _gen_value(rng, depth):
    t = int(rng.integers(0, 8))
    if depth < 3 and t == 0:
        return {"k%d" % q: _gen_value(rng, depth + 1) for q in range(int(rng.integers(0, 3)))}
    if depth < 3 and t == 1:
        return [_gen_value(rng, depth + 1) for _ in range(int(rng.integers(0, 4)))]
    return _gen_scalar(rng)


SPACINGS = [(",", ":"), (", ", ": "), (" , ", " : ")]


def gen_line(rng):
    """(line, the array): a valid JSON object in one line with "arr" somewhere among other members, in one of three spacing styles."""
    arr = [_gen_value(rng, 1) for _ in range(int(rng.integers(0, 9)))]
    row = {"id": int(rng.integers(0, 1000)), "arr": arr, "s": _gen_scalar(rng), "o": {"arr": [1, 2]}}
    keys = list(row)
    rng.shuffle(keys)
    line = json.dumps({k: row[k] for k in keys}, separators=SPACINGS[int(rng.integers(0, 3))], ensure_ascii=bool(rng.integers(0, 2)))
    return line.encode("utf-8"), arr


def opener_of(line, pos, what, name=b"arr"):
    """the boundary index of the opener of the depth-1 member `name` of a one-line stream, by member's boundary-serial statement"""
    _, found, _ = members_boundaries(line, pos, what, [name])
    kind, rec = found[0][0]
    assert kind == ARRAY
    return rec


def agrees_with_json(line, arr, status, els):
    """True iff the rule's answer for the array of a valid line is json.loads's: as many elements, each of its kind, and every scalar
    element's record the bytes that json.loads reads that value from.  -> (agrees, scalar elements compared)"""
    if status != OK or len(els) != len(arr):
        return False, 0
    pos, _ = index_set(line)
    scalars = 0
    for (rec, kind), v in zip(els, arr):
        want = OBJECT if isinstance(v, dict) else ARRAY if isinstance(v, list) else SCALAR
        if kind != want:
            return False, scalars
        if kind == SCALAR:
            try:
                got = json.loads(record(line, pos, rec).decode("utf-8"))
            except ValueError:
                return False, scalars
            if got != v or type(got) is not type(v):
                return False, scalars
            scalars += 1
    return True, scalars


def break_line(rng, line):
    """a line broken on purpose: cut, a closer swapped, a line feed inside, a closer dropped"""
    t = int(rng.integers(0, 4))
    if t == 0:
        return line[:int(rng.integers(0, len(line) + 1))]
    at = int(rng.integers(0, len(line)))
    if t == 1:
        return line[:at] + line[at:].replace(b"]", b"}", 1)
    if t == 2:
        return line[:at] + b"\n" + line[at:]
    return line[:at] + line[at:].replace(b"]", b"", 1)
