"""THE RULE of brx_object_batch (include/brx.h), stated twice and independently, plus what the tests of the call share: the check
values of the contract, a fixed-seed generator of nested JSON Lines (objects in objects, arrays of objects, duplicate keys, keys
repeated in nested values) and the comparison with json.loads.

  object_boundaries  walks the boundaries (pos, what) of a stream behind an opener, as the contract words it: relative depth from
                     `what`, the key record of a depth-1 ':' from `pos` under take's rule, the value's kind from the next boundary.
  object_bytes       walks the BYTES of the stream and never sees pos or what: a small reader that keeps the string state, the depth,
                     the number of structural bytes so far and the text since the last of them.

Both return (status, end, n_members, {q: (kind, rec)}, flags) for one (stream, r, names).  The index of a text, a record and the look
at a key are tests/member_oracle.py's (each statement uses the one of member's two that shares nothing with the other's); the elements
of an array are tests/elements_oracle.py's."""
import json

import numpy as np

from elements_oracle import elements_boundaries
from member_oracle import (ARRAY, BAD, ESCAPED_KEY, LONG_KEY, MISSING, OBJECT, SCALAR, _BYTES_KINDS, _bytes_key, _key_of, index_set,  # noqa: F401
                           record)

OK, NONE, NOT_OBJECT, UNCLOSED, MISMATCH = 0, 1, 2, 3, 4
STATUS_NAMES = {OK: "OK", NONE: "NONE", NOT_OBJECT: "NOT_OBJECT", UNCLOSED: "UNCLOSED", MISMATCH: "MISMATCH"}
KIND_NAMES = {MISSING: "MISSING", SCALAR: "SCALAR", OBJECT: "OBJECT", ARRAY: "ARRAY", BAD: "BAD"}
NO_END = (1 << 64) - 1
ELEMENTS_OK = 0


def object_boundaries(s, pos, what, r, names, count=None, n_pos=None):
    """The boundary-serial statement.  pos / what: the stream's part of the tables (as far as they go); count / n_pos: as the call's,
    n_pos counted from the stream's first boundary (boundaries at or behind it do not count and are not looked at)."""
    count = len(pos) if count is None else count
    n_pos = len(pos) if n_pos is None else n_pos
    C, l = min(count, max(n_pos, 0)), len(s)
    names = list(names)

    def P(k):
        return min(pos[k], l) if k < n_pos else l

    if r >= C:
        return NONE, NO_END, 0, {}, 0
    if what[r:r + 1] != b"{":
        return NOT_OBJECT, NO_END, 0, {}, 0
    found, flags, members, e, k = {}, 0, 0, 1, r + 1
    while True:
        if k == C:
            return UNCLOSED, C, members, found, flags
        w = what[k:k + 1]
        if w == b"\n":
            return UNCLOSED, k, members, found, flags
        if w in (b"{", b"["):
            e += 1
        elif w in (b"}", b"]"):
            e -= 1
            if e == 0:
                return (OK if w == b"}" else MISMATCH), k, members, found, flags
        elif w == b":" and e == 1:
            members += 1
            start = min(P(k - 1) + 1, l)
            q, bits = _key_of(s[start:max(P(k), start)], names)
            flags |= bits
            if q is not None:
                nxt = what[k + 1:k + 2] if k + 1 < C else b""
                kind = SCALAR if nxt in (b",", b"}") else OBJECT if nxt == b"{" else ARRAY if nxt == b"[" else BAD
                found[q] = (kind, k + 1)
        k += 1


def object_bytes(s, r, names):
    """The byte-serial statement: no pos, no what.  The r-th structural byte outside strings is the opener."""
    names = list(names)
    in_str = esc = False
    nb = 0            # structural bytes so far: the next one is boundary nb
    depth = None      # None: in front of the opener
    since = bytearray()
    found, flags, members, pending = {}, 0, 0, None
    for c in s:
        if esc:
            esc = False
            since.append(c)
            continue
        if c == 0x5C:
            esc = True
            since.append(c)
            continue
        if c == 0x22:
            in_str = not in_str
            since.append(c)
            continue
        if in_str or c not in b"{}[]:,\n":
            since.append(c)
            continue
        if depth is None:
            if nb == r:
                if c != 0x7B:
                    return NOT_OBJECT, NO_END, 0, {}, 0
                depth = 1
        else:
            if pending is not None:  # the first structural byte behind the ':' tells the value's kind
                found[pending] = (_BYTES_KINDS.get(c, BAD), nb)
                pending = None
            if c == 0x0A:
                return UNCLOSED, nb, members, found, flags
            if c in b"{[":
                depth += 1
            elif c in b"}]":
                depth -= 1
                if depth == 0:
                    return (OK if c == 0x7D else MISMATCH), nb, members, found, flags
            elif c == 0x3A and depth == 1:
                members += 1
                if len(since) > 64:
                    flags |= LONG_KEY
                else:
                    if 0x5C in since:
                        flags |= ESCAPED_KEY
                    q = _bytes_key(since, names)
                    if q is not None:
                        pending = q
                        found[q] = (BAD, nb + 1)  # unless another structural byte follows
        nb += 1
        since = bytearray()
    if depth is None:
        return NONE, NO_END, 0, {}, 0
    return UNCLOSED, nb, members, found, flags


def form_boundaries(s, r, names):
    pos, what = index_set(s)
    return object_boundaries(s, pos, what, r, names)


FORMS = {"boundaries": form_boundaries, "bytes": object_bytes}

# ---- the check values of the contract: (stream, names, r, status, n_members, end, {name: (kind, rec)}, flags) -----------------------
ABCUX = [b"a", b"b", b"c", b"u", b"x"]
K32 = b"k" * 32
CHECK = [
    (b'{"u":{"a":1,"b":[2,3],"a":4},"a":5}', ABCUX, 2, OK, 3, 11, {b"a": (SCALAR, 11), b"b": (ARRAY, 6)}, 0),
    (b'{"u":{"a":1,"b":[2,3],"a":4},"a":5}', ABCUX, 0, OK, 2, 14, {b"u": (OBJECT, 2), b"a": (SCALAR, 14)}, 0),
    (b'{"a":{}}', ABCUX, 2, OK, 0, 3, {}, 0),
    (b'{"a":{"b":1]}', ABCUX, 2, MISMATCH, 1, 4, {b"b": (BAD, 4)}, 0),
    (b'{"a":{"b":1,"c":2\n', ABCUX, 2, UNCLOSED, 2, 6, {b"b": (SCALAR, 4), b"c": (BAD, 6)}, 0),
    (b'{"a":{"b":', ABCUX, 2, UNCLOSED, 1, 4, {b"b": (BAD, 4)}, 0),
    (b'{"a":{"x":{"b":1},"b":2}}', ABCUX, 2, OK, 2, 9, {b"x": (OBJECT, 4), b"b": (SCALAR, 9)}, 0),
    (b'{"a":{"x":{"b":1},"b":2}}', ABCUX, 4, OK, 1, 6, {b"b": (SCALAR, 6)}, 0),
    (b'{"items":[{"id":1},{"id":2}]}', [b"id"], 3, OK, 1, 5, {b"id": (SCALAR, 5)}, 0),
    (b'{"items":[{"id":1},{"id":2}]}', [b"id"], 7, OK, 1, 9, {b"id": (SCALAR, 9)}, 0),
    (b'{"a":{' + b" " * 30 + b'"' + K32 + b'":1}}', [K32], 2, OK, 1, 4, {K32: (SCALAR, 4)}, 0),
    (b'{"a":{' + b" " * 31 + b'"' + K32 + b'":1}}', [K32], 2, OK, 1, 4, {}, LONG_KEY),
    (b'{"a":{"a\\u0062":1}}', [b"ab"], 2, OK, 1, 4, {}, ESCAPED_KEY),
    (b'{"a":[1]}', ABCUX, 2, NOT_OBJECT, 0, NO_END, {}, 0),
    (b'{"a":[1]}', ABCUX, 9, NONE, 0, NO_END, {}, 0),
]


def check_answer(c):
    """a check value as the two statements return it"""
    stream, names, r, status, members, end, found, flags = c
    return status, end, members, {names.index(nm): v for nm, v in found.items()}, flags


def header_form(stream, names, r, status, members, end, found, flags):
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
    vals = " ".join("%s %s %d" % ("k32" if nm == K32 else nm.decode(), KIND_NAMES[kd], rec) for nm, (kd, rec) in sorted(found.items()))
    tail = " members %d end %d" % (members, end) if end != NO_END else ""
    return "[%s] r %d: %s%s%s flags %d" % (out, r, STATUS_NAMES[status], tail, "; " + vals if vals else "", flags)


# ---- a generator of valid nested JSON Lines ------------------------------------------------------------------------------------------
NAMES = [b"a", b"b", b"c", b"u", b"x", b"id", b"items", b"meta"]  # every key the generator uses: 8 names, one call
_ALPHABET = ["a", "b", " ", ",", ":", "{", "}", "[", "]", '\\"', "\\\\", "\\n", "\\u00e9", "x", "],[", "0", '{\\"a\\":1}']
SPACINGS = [(",", ":", ""), (", ", ": ", " "), (" , ", " : ", "\t"), (",\r", " :", " ")]


def _gen_scalar(rng):
    t = int(rng.integers(0, 6))
    if t == 0:
        return str(int(rng.integers(-10**9, 10**9)))
    if t == 1:
        return repr(float(np.round(rng.uniform(-100, 100), int(rng.integers(0, 6)))))
    if t == 2:
        return ("true", "false", "null")[int(rng.integers(0, 3))]
    return '"' + "".join(_ALPHABET[int(x)] for x in rng.integers(0, len(_ALPHABET), int(rng.integers(0, 10)))) + '"'


def _gen_object(rng, depth, max_depth, sp):
    n = int(rng.integers(0, 6))
    keys = [NAMES[int(x)].decode() for x in rng.integers(0, len(NAMES), n)]  # (with repeats: duplicate keys)
    body = sp[0].join(sp[2] + '"' + k + '"' + sp[1] + _gen_value(rng, depth + 1, max_depth, sp) for k in keys)
    return "{" + body + (sp[2] if n else "") + "}"


def _gen_value(rng, depth, max_depth, sp):
    t = int(rng.integers(0, 8))
    if depth < max_depth and t <= 1:
        return _gen_object(rng, depth, max_depth, sp)
    if depth < max_depth and t == 2:  # an array, of objects mostly
        return "[" + sp[0].join(_gen_object(rng, depth + 1, max_depth, sp) if rng.integers(0, 3) else _gen_value(rng, depth + 1, max_depth, sp)
                                for _ in range(int(rng.integers(0, 4)))) + "]"
    return _gen_scalar(rng)


def gen_line(rng):
    """One valid JSON object in one line, nested two or three levels deep, in one of four spacing styles; always with an object
    under "meta" and an array of objects under "items" among what the dice give."""
    sp = SPACINGS[int(rng.integers(0, len(SPACINGS)))]
    max_depth = 2 + int(rng.integers(0, 2))
    parts = ['"meta"' + sp[1] + _gen_object(rng, 1, max_depth, sp),
             '"items"' + sp[1] + "[" + sp[0].join(_gen_object(rng, 2, max_depth, sp) for _ in range(int(rng.integers(0, 4)))) + "]"]
    for _ in range(int(rng.integers(0, 4))):
        parts.append('"' + NAMES[int(rng.integers(0, len(NAMES)))].decode() + '"' + sp[1] + _gen_value(rng, 1, max_depth, sp))
    rng.shuffle(parts)
    return ("{" + sp[0].join(parts) + "}").encode("utf-8")


def json_pairs(line):
    """json.loads of a line with every object as the list of its (key, value) pairs, duplicates kept"""
    return json.loads(line.decode("utf-8"), object_pairs_hook=lambda p: [("\0pair", k, v) for k, v in p])


def _is_object(v):
    return isinstance(v, list) and all(isinstance(p, tuple) and len(p) == 3 and p[0] == "\0pair" for p in v)


def agrees_with_json(line, form, stats=None):
    """Every object of a valid line, found from the top by the rule itself (an OBJECT member is again an opener; the OBJECT elements
    of an ARRAY member are openers, by elements' rule), against json.loads: as many members, the same names present, the LAST of
    duplicates, a scalar member's record the bytes json.loads reads that value from, a nested one of the right kind.  `form`: one of
    FORMS' values.  -> the number of objects compared; raises AssertionError where they differ."""
    pos, what = index_set(line)
    todo, n_objects = [(0, json_pairs(line), 1)], 0
    while todo:
        r, pairs, depth = todo.pop()
        status, end, members, found, flags = form(line, r, NAMES)
        assert status == OK and flags == 0 and members == len(pairs), (line, r, status, members, len(pairs))
        assert what[end:end + 1] == b"}"
        view = {}
        for _, k, v in pairs:
            view[k.encode()] = v
        assert set(view) == set(NAMES[q] for q in found), (line, r, found)
        for q, (kind, rec) in found.items():
            v = view[NAMES[q]]
            if isinstance(v, list) and kind == OBJECT:
                assert _is_object(v), (line, r, q)
                todo.append((rec, v, depth + 1))
            elif isinstance(v, list):
                assert kind == ARRAY and (not v or not _is_object(v)), (line, r, q, kind)
                st, _, els = elements_boundaries(line, pos, what, rec)
                assert st == ELEMENTS_OK and len(els) == len(v), (line, r, q)
                for (el_rec, el_kind), ev in zip(els, v):
                    if el_kind == OBJECT:
                        assert _is_object(ev)
                        todo.append((el_rec, ev, depth + 1))
                        if stats is not None:
                            stats["in_arrays"] = stats.get("in_arrays", 0) + 1
            else:
                assert kind == SCALAR, (line, r, q, kind)
                got = json.loads(record(line, pos, rec).decode("utf-8"))
                assert got == v and type(got) is type(v), (line, r, q, got, v)
                if stats is not None:
                    stats["scalars"] = stats.get("scalars", 0) + 1
        n_objects += 1
        if stats is not None:
            stats["max_depth"] = max(stats.get("max_depth", 0), depth)
            stats["dups"] = stats.get("dups", 0) + (1 if len(view) < len(pairs) else 0)
    return n_objects


def break_line(rng, line):
    """a line broken on purpose: cut, a closer swapped, a line feed inside, a closer dropped, a colon doubled"""
    t = int(rng.integers(0, 5))
    if t == 0:
        return line[:int(rng.integers(0, len(line) + 1))]
    at = int(rng.integers(0, len(line)))
    if t == 1:
        return line[:at] + line[at:].replace(b"}", b"]", 1)
    if t == 2:
        return line[:at] + b"\n" + line[at:]
    if t == 3:
        return line[:at] + line[at:].replace(b"}", b"", 1)
    return line[:at] + line[at:].replace(b":", b"::", 1)


def batch(b_streams, tables, sel, names, memo=None):
    """The call's outputs for a selection over a batch, by the boundary-serial statement over the call's own tables.  tables: (count,
    pos_off, pos, what, n_pos) as the call gets them (numpy / bytes); memo: a dict that a caller keeps per state of the tables and
    names, so that an opener is walked once however many selections name it.  -> (n_members, status, end, mem_stream, mem_rec,
    mem_kind, obj_flags) as lists, the three member outputs [Q][m]."""
    count, pos_off, pos, what, n_pos = tables
    n, Q, m = len(b_streams), len(names), len(sel)
    out = ([0] * m, [NONE] * m, [NO_END] * m, [[i for i, _ in sel] for _ in range(Q)], [[NO_END] * m for _ in range(Q)],
           [[MISSING] * m for _ in range(Q)], [0] * m)
    memo = {} if memo is None else memo
    for j, (i, r) in enumerate(sel):
        if i >= n:
            continue
        if (i, r) not in memo:
            a = int(pos_off[i])
            left = max(0, n_pos - a)
            c = min(int(count[i]), left)
            memo[(i, r)] = object_boundaries(b_streams[i], [int(x) for x in pos[a:a + c]], what[a:a + c], r, names, count=c, n_pos=left)
        status, end, members, found, flags = memo[(i, r)]
        out[0][j], out[1][j], out[2][j], out[6][j] = members, status, end, flags
        for q, (kind, rec) in found.items():
            out[4][q][j], out[5][q][j] = rec, kind
    return out
