"""brx_object_batch (include/brx.h, brx_object.hip): the named members of nested JSON objects as selections for the record calls, and
the extent of an object.  Every expected value comes from tests/object_oracle.py (its two statements are held to each other, to the
contract's check values and to json.loads by tests/test_object_abi.py): the boundary-serial statement over the very pos / what /
count / n_pos that the call gets, so that cut and garbage tables have an expectation too.  Every output is pre-filled with poison and
carries guard words in front of it and behind it that must be unchanged.  In-process, one context."""
import json
import os
import re

import numpy as np
import pytest

import brx_knobs
import craft
import object_oracle as oo
from brotli_rs_amd.brx import MEMBER_ARRAY, MEMBER_OBJECT, MEMBER_SCALAR, OBJECT_OK, PARSE_OK, TEXT_OK  # noqa: F401  (without the call nothing here runs)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_H = open(os.path.join(ROOT, "brotli-rs_amd", "csrc", "brx_object.h")).read()
_HM = open(os.path.join(ROOT, "brotli-rs_amd", "csrc", "brx_member.h")).read()
L = 16 * int(re.search(r"#define\s+BRX_OB_UNITS\s+(\d+)u", _H).group(1))  # boundaries that one lane walks alone
R = int(re.search(r"#define\s+BRX_MB_ROW\s+(\d+)u", _HM).group(1))         # boundaries per wave step
P64, P32, P8 = 0x5151515151515151, 0x51515151, 0x51
G = 16       # guard words in front of every output and behind it
SPARE = 16   # table entries behind n_pos that must never be loaded
NONE = (1 << 64) - 1
ABCUX = oo.ABCUX
EIGHT = [b"a", b"id", b"items", b"meta", oo.K32, b"a_rather_long_key_of_32_bytes_xx", b"b", b"ab"]
Z16 = b'"z":0,' * 8  # 16 boundaries of members that carry none of the names: one unit


@pytest.fixture(scope="module")
def ctx():
    c = brx_knobs.context(0)
    yield c
    c.close()


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a))
    return (t.to(dtype) if dtype is not None else t).to("cuda:0")


def _u64(a):
    return np.array(a, dtype=np.uint64).view(np.int64)


class Batch:
    """Streams in an arena (brackets, quotes and colons between them) with the tables of an index at {}[]:,\\n computed on the CPU --
    or whatever the test puts in their place."""

    def __init__(self, streams, lead=3):
        self.streams = [bytes(s) for s in streams]
        self.n = len(self.streams)
        parts, offs, at = [b'{":'[:lead]], [], lead
        for p, s in enumerate(self.streams):
            offs.append(at)
            gap = b'}:"{\n'[:1 + p % 5]
            parts += [s, gap]
            at += len(s) + len(gap)
        self.host = np.frombuffer(b"".join(parts), dtype=np.uint8)
        self.offs, self.lens = np.array(offs, dtype=np.int64), np.array([len(s) for s in self.streams], dtype=np.int64)
        per = [oo.index_set(s) for s in self.streams]
        self.count = np.array([len(p[0]) for p in per], dtype=np.int64)
        self.pos_off = np.cumsum(self.count) - self.count
        self.pos = np.array([x for p in per for x in p[0]], dtype=np.int64)
        self.what = np.frombuffer(b"".join(p[1] for p in per), dtype=np.uint8).copy()
        self.n_pos = len(self.pos)

    def upload(self):
        self.arena = _dev(self.host)
        self.d_off, self.d_len = _dev(self.offs), _dev(self.lens)
        self.d_count, self.d_pos_off = _dev(self.count), _dev(self.pos_off)
        self.d_pos = _dev(np.concatenate([self.pos[:self.n_pos], np.full(SPARE, 1 << 40, dtype=np.int64)]))  # (behind n_pos: never loaded)
        self.d_what = _dev(np.concatenate([self.what[:self.n_pos], np.full(SPARE, 0x7D, dtype=np.uint8)]))
        return self

    def head(self):
        return (self.arena.data_ptr(), self.d_off.data_ptr(), self.d_len.data_ptr(), self.n, int(self.arena.numel()),
                self.d_count.data_ptr(), self.d_pos_off.data_ptr(), self.d_pos.data_ptr(), self.d_what.data_ptr(), self.n_pos)

    def tables(self):
        return self.count, self.pos_off, self.pos, bytes(self.what), self.n_pos

    def want(self, sel, names):
        """the oracle's boundary-serial statement over these very tables (one walk per opener, names and state of the tables)"""
        key = (self.n_pos, self.what.tobytes(), self.pos.tobytes(), self.count.tobytes())
        if getattr(self, "_memo_for", None) != key:
            self._memo_for, self._memo = key, {}
        return oo.batch(self.streams, self.tables(), sel, names, memo=self._memo.setdefault(tuple(names), {}))

    def openers(self):
        """every '{' boundary of every stream, as pairs"""
        return [(i, k) for i in range(self.n) for k in range(int(self.count[i])) if self.what[int(self.pos_off[i]) + k] == 0x7B]


class _Out:
    """a poisoned device buffer of `size` elements with G guard words on either side"""

    def __init__(self, size, dtype, poison):
        import torch
        self.size, self.poison = size, poison
        self.t = torch.full((size + 2 * G,), poison, dtype=dtype, device="cuda:0")

    def ptr(self):
        return self.t.data_ptr() + G * self.t.element_size()

    def host(self):
        """-> the buffer's elements as int64 / the bit pattern; asserts the guards"""
        got = self.t.cpu().numpy()
        got = got.view(np.uint32).astype(np.int64) if got.dtype == np.int32 else got.astype(np.int64)
        assert (got[:G] == self.poison).all() and (got[G + self.size:] == self.poison).all(), "a guard word changed"
        return got[G:G + self.size]


def _check(ctx, b, sel, names, given=(True, True, True, True), hip_stream=None, sync=None):
    """One call against the oracle's boundary-serial statement over these very tables.  given: whether n_members, status, end and
    obj_flags are passed (obj_flags never in extent mode).  -> what the oracle says: (n_members, status, end, mem_stream, mem_rec,
    mem_kind, obj_flags)"""
    import torch
    if not hasattr(b, "arena"):
        b.upload()
    want = b.want(sel, names)
    m, Q = len(sel), len(names)
    d_ss = _dev(np.array([i for i, _ in sel] + [0] * SPARE, dtype=np.uint32).view(np.int32))
    d_sr = _dev(_u64([r for _, r in sel] + [2] * SPARE))
    outs = {"n_members": _Out(m, torch.int64, P64), "status": _Out(m, torch.uint8, P8), "end": _Out(m, torch.int64, P64),
            "obj_flags": _Out(m, torch.uint8, P8), "mem_stream": _Out(Q * m, torch.int32, P32), "mem_rec": _Out(Q * m, torch.int64, P64),
            "mem_kind": _Out(Q * m, torch.uint8, P8)}
    on = {"n_members": given[0], "status": given[1], "end": given[2], "obj_flags": given[3] and Q > 0, "mem_stream": Q > 0, "mem_rec": Q > 0,
          "mem_kind": Q > 0}
    p = {k: (outs[k].ptr() if on[k] else None) for k in outs}
    torch.cuda.synchronize()
    ctx.object_batch_device(*b.head(), d_ss.data_ptr(), d_sr.data_ptr(), m, names, p["n_members"], p["status"], p["end"], p["mem_stream"],
                            p["mem_rec"], p["mem_kind"], p["obj_flags"], hip_stream=hip_stream)
    if sync:
        sync()
    expect = {"n_members": want[0], "status": want[1], "end": want[2], "obj_flags": want[6],
              "mem_stream": [x for row in want[3] for x in row], "mem_rec": [x for row in want[4] for x in row],
              "mem_kind": [x for row in want[5] for x in row]}
    for name, o in outs.items():
        got = o.host()
        if not on[name]:
            assert (got == o.poison).all(), name
            continue
        w = np.array(expect[name], dtype=np.uint64).view(np.int64) if name in ("end", "mem_rec", "n_members") else np.array(expect[name], dtype=np.int64)
        bad = np.flatnonzero(got != w)
        assert bad.size == 0, (name, bad[:5].tolist(), [sel[x % m] for x in bad[:5]], got[bad[:5]].tolist(), w[bad[:5]].tolist())
    return want


def _object(dist, style, rng, keys=(b"a", b"b", b"c", b"u", b"x", b"ab", b"zz", b"id")):
    """an object whose closer stands `dist` boundaries behind its opener: style 0 scalar members only, 1 nested values and strings too"""
    s, have = b"{", 0
    while have + 1 < dist:
        left = dist - 1 - have
        key = (b"", b" ")[int(rng.integers(0, 4)) == 0] + b'"' + keys[int(rng.integers(0, len(keys)))] + b'"' + (b"", b"\t")[int(rng.integers(0, 5)) == 0]
        pick = 0 if style == 0 else int(rng.integers(0, 6))
        if pick == 1 and left >= 5:
            s, have = s + key + b":[1,2],", have + 5
        elif pick == 2 and left >= 5:
            s, have = s + key + b':{"a":7},', have + 5
        elif pick == 3 and left >= 7:
            s, have = s + key + b':[{"b":[]}],', have + 7
        elif pick == 4 and left >= 2:
            s, have = s + key + b':"a}:{,\\"",', have + 2
        elif left >= 2:
            s, have = s + key + b":%d," % int(rng.integers(0, 100)), have + 2
        else:
            s, have = s + key + b":1", have + 1
    return s + b"}"


def test_the_thresholds_are_the_headers():
    assert L % 16 == 0 and 16 <= L <= 240 and R == 64 * 16 and L < R
    assert (OBJECT_OK, MEMBER_OBJECT, MEMBER_ARRAY) == (oo.OK, oo.OBJECT, oo.ARRAY)


def test_check_values_of_the_contract(ctx):
    for c in oo.CHECK:
        stream, names, r = c[0], c[1], c[2]
        st, end, members, found, flags = oo.check_answer(c)
        want = _check(ctx, Batch([stream]), [(0, r)], names)
        assert (want[1][0], want[2][0], want[0][0], want[6][0]) == (st, end, members, flags), stream
        assert {q: (want[5][q][0], want[4][q][0]) for q in range(len(names)) if want[5][q][0]} == found, stream
    b = Batch([c[0] for c in oo.CHECK])  # all of them as one batch, every boundary of every stream an opener and two behind
    sel = [(i, r) for i in range(b.n) for r in range(int(b.count[i]) + 2)]
    for names in (ABCUX, [b"id"], [oo.K32, b"ab"], []):
        _check(ctx, b, sel, names)


def test_closer_distances_at_every_phase(ctx):
    """The closer 1 .. 40, L - 1 .. L + 2, R - 1 .. R + 2, R + L and 2R + 3 boundaries behind the opener, behind 0, 1, 5 and 15 leading
    boundaries (and whatever the streams in front add: the opener stands at each of the 16 phases of `what`); closed by '}' and by
    ']', cut by a line feed and by the stream's end; scalar members only and nested values."""
    rng = np.random.default_rng(1)
    dists = list(range(1, 41)) + [L - 1, L, L + 1, L + 2, R - 1, R, R + 1, R + 2, R + L, 2 * R + 3]
    streams, sel = [], []
    for lead in (0, 1, 5, 15):
        for q, d in enumerate(dists):
            a = _object(d, (lead + q) % 2, rng)
            for v in range(4 if d > 2 else 1):
                body = (a + b"}\n", a[:-1] + b'],"a":1}', a[:-1] + b'\n{"a":1}', a[:-1])[v]
                streams.append(b"," * (lead + (q + v) % 2) + body)
                sel.append((len(streams) - 1, lead + (q + v) % 2))
    b = Batch(streams)
    assert set((int(b.pos_off[i]) + r) % 16 for i, r in sel) == set(range(16))
    want = _check(ctx, b, sel, ABCUX)
    assert set(want[1]) == {oo.OK, oo.MISMATCH, oo.UNCLOSED}
    assert set(e - r for e, (_, r) in zip(want[2], sel)) >= set(dists)
    assert max(want[0]) > R and set(x for row in want[5] for x in row) == {oo.MISSING, oo.SCALAR, oo.OBJECT, oo.ARRAY, oo.BAD}
    _check(ctx, b, sel[::-1] + sel[::7], [b"b"])  # another order, repeats, m not a multiple of the block, one name
    _check(ctx, b, sel, [])                      # the extent mode
    assert (len(sel) + len(sel[::7])) % 256 != 0


def test_matches_in_lane_0_lane_63_and_a_second_row(ctx):
    """Long objects with a matching member at chosen places: lane 0 and lane 63 of the first row, the second row; the same name in two
    lanes of one row and in two rows (last wins across both borders), three times in one unit; a match behind the stop lane in the same
    row, which must not count; colons at depth 2 and deeper, which must not count."""
    fill = lambda units: Z16 * units
    deep = b'{"a":' * 1500 + b"1" + b"}" * 1500
    streams = [
        b'{"a":1,' + fill(70) + b'"q":0}',                                                                 # 0: lane 0 of the first row
        b"{" + fill(63) + b'"b":[1],"z":0,' + fill(8) + b"}",                                              # 1: lane 63
        b"{" + fill(64) + b'"c":{"a":9},"z":0,' + fill(3) + b"}",                                          # 2: the second row; an "a" at depth 2
        b'{"a":1,' + fill(20) + b'"a":2,' + fill(20) + b'"a":3,' + fill(70) + b'"a":4,' + fill(70) + b'"b":5}',  # 3: two lanes, two rows
        b'{"a":1,"a":2,"b":3,"a":4,' + fill(70) + b"}",                                                    # 4: one unit with three of a name
        b"{" + fill(10) + b'"a":1},"a":2,"b":3,' + fill(70) + b"}",                                        # 5: matches behind the stop lane
        b"{" + fill(10) + b'"a":1\n,"a":2,"b":3,' + fill(70) + b"}",                                       # 6: ... behind a line feed
        b"{" + fill(70) + b'"u":{"a":1,"x":{"a":2,"b":[{"a":3}]}},"x":[{"a":4}],' + fill(70) + b"}",       # 7: deeper colons
        b'{"u":{' + fill(200) + b'"a":1},"a":2}',                                                          # 8: a long object inside
        b'{"b":' + deep + b',"a":2}',                                                                      # 9: closers rows behind their openers
        b"{" + b":" * 3000 + b"}",                                                                         # 10: rows of colons only
        b"{[" + b":" * 2500 + b"]" + b":" * 1100 + b"}",                                                   # 11: rows of colons at depth 2
    ]
    b = Batch(streams)
    sel = [(i, 0) for i in range(b.n)]
    want = _check(ctx, b, sel, ABCUX)
    rec = lambda i, q: (want[5][q][i], want[4][q][i])
    assert rec(0, 0) == (oo.SCALAR, 2) and rec(1, 1) == (oo.ARRAY, 16 * 63 + 2) and rec(2, 2) == (oo.OBJECT, 16 * 64 + 2)
    assert rec(2, 0) == (oo.MISSING, NONE)
    assert rec(3, 0) == (oo.SCALAR, 1 + 3 * 2 + 110 * 16 + 1) and want[0][3] == 5 + 180 * 8
    assert rec(4, 0) == (oo.SCALAR, 8) and rec(5, 0)[1] == 162 and rec(5, 1)[0] == oo.MISSING and want[1][5] == oo.OK
    assert rec(6, 0) == (oo.BAD, 162) and want[1][6] == oo.UNCLOSED and rec(6, 1)[0] == oo.MISSING
    assert rec(7, 0)[0] == oo.MISSING and rec(7, 3)[0] == oo.OBJECT and rec(7, 4)[0] == oo.ARRAY and want[0][7] == 2 + 140 * 8
    assert want[0][8] == 2 and rec(8, 0) == (oo.SCALAR, want[2][8]) and want[0][9] == 2 and want[0][10] == 3000 and want[0][11] == 1100
    _check(ctx, b, [(8, 2), (7, 1122), (9, 2), (9, 4), (11, 1)] + sel, [b"a"])  # the inner objects, NOT_OBJECT for the '['
    _check(ctx, b, sel, [])


def test_keys(ctx):
    """Key records of 64 and 65 bytes before trimming; keys at every offset of the arena's 16-byte units; blanks, tabs and CRs around
    keys; a backslash in a key; keys that are a prefix or an extension of a name; not quoted, half quoted, empty; names of 1 and 32
    bytes."""
    k32, n32 = oo.K32, b"a_rather_long_key_of_32_bytes_xx"
    bodies = [b" " * 30 + b'"' + k32 + b'":1', b" " * 31 + b'"' + k32 + b'":1', b"\t" * 62 + b'"":1', b" " * 61 + b'"a":1', b" " * 62 + b'"a":1',
              b' "b"\t:1,\r"ab" :2,"":3,"bb":4,b:5,\'b\':6', b'"a\\u0062":1,"b":2', b'"a\\"":1,"\\\\":2', b'"a ":1," a":2,"a":3', b'"A":1,"aa":2,"":3',
              b'"' + n32 + b'":1,"' + n32[:31] + b'":2,"' + n32 + b'x":3', b'"' + k32 + b'k":1', b'"a"x:1,x"a":2,"a""a":3']
    streams = [b'{"o":{' + x + b"}}" for x in bodies]
    streams += [b'{"o":{' + b" " * p + b'"' + n32 + b'":1,' + b" " * p + b'"ab":2}}' for p in range(17)]  # keys across the arena's units
    names = [b"a", b"b", b"ab", k32, n32, b"bb", b"a ", b"A"]
    for lead in (3, 2):  # the arena's phase
        b = Batch(streams, lead=lead)
        sel = [(i, 2) for i in range(b.n)] + [(i, 0) for i in range(b.n)]
        want = _check(ctx, b, sel, names)
        assert want[6][:9] == [0, oo.LONG_KEY, 0, 0, oo.LONG_KEY, 0, oo.ESCAPED_KEY, oo.ESCAPED_KEY, 0]
        assert want[5][3][0] == oo.SCALAR and want[5][3][1] == oo.MISSING and want[5][0][3] == oo.SCALAR and want[5][0][4] == oo.MISSING
        assert [want[5][q][5] for q in (1, 2, 5)] == [oo.SCALAR] * 3 and want[0][5] == 6
        assert want[5][2][6] == oo.MISSING and want[5][1][6] == oo.SCALAR and want[4][0][8] == 8 and want[5][6][8] == oo.SCALAR
        assert want[5][4][10] == oo.SCALAR and want[4][4][10] == 4 and want[5][3][11] == oo.MISSING and want[5][0][12] == oo.MISSING
        assert all(want[5][4][13 + p] == oo.SCALAR and want[5][2][13 + p] == oo.SCALAR for p in range(17))
        assert all(x == oo.MISSING for row in want[5] for x in row[b.n:]) and want[0][b.n:] == [1] * b.n  # the outer object has "o" alone
    _check(ctx, b, sel, [b"a"])
    _check(ctx, b, sel, [n32])


def test_long_and_short_entries_in_one_wave(ctx):
    """Several long objects in one wave next to short ones and entries that select nothing, the first long one not in lane 0; a
    selection with repeats, MISSING, streams behind n and a whole column of member's output (SCALAR and ARRAY openers included);
    m = 1, 63, 64, 65, 257 and beyond a block; 0, 1, 5 and 8 names."""
    rng = np.random.default_rng(3)
    lines = []
    for k in range(300):
        nm_ = (0, 1, 2, 5, 40, 70, 300, 1100)[int(rng.integers(0, 8))] if k % 3 else int(rng.integers(0, 9))
        inner = _object(2 * nm_ + 1, 1, rng)
        meta = inner if k % 7 else (b"7" if k % 14 else b"[" + inner + b"]")
        parts = [b'"id":%d' % k, b'"meta":' + meta, b'"t":"{:"']
        if k % 11 == 0:
            del parts[1]
        rng.shuffle(parts)
        lines.append(b"{" + b",".join(parts) + b"}")
    b = Batch([b"\n".join(lines[:200]) + b"\n", b"\n".join(lines[200:])])
    sel, kinds = [], []
    for i, s in enumerate(b.streams):  # member's column for "meta", by member's oracle
        _, found, _ = oo_members(s)
        for cur in found:
            kd, rec = cur.get(0, (0, NONE))
            sel.append((i, rec))
            kinds.append(kd)
    assert len(sel) == 301 and set(kinds) == {0, oo.SCALAR, oo.OBJECT, oo.ARRAY}
    want = _check(ctx, b, sel, ABCUX)
    for st, kd in zip(want[1], kinds):
        assert st == (oo.OK if kd == oo.OBJECT else oo.NONE if kd == 0 else oo.NOT_OBJECT)
    long_ = [j for j, (e, (_, r)) in enumerate(zip(want[2], sel)) if want[1][j] == oo.OK and e - r > L]
    assert len(long_) > 60 and min(long_) % 64 != 0 and any(a // 64 == c // 64 for a, c in zip(long_, long_[1:]))
    more = sel + sel[::3] + [(2, 0), (5, 1), (1 << 31, 0), ((1 << 32) - 1, 3), (0, NONE), (1, NONE - 1), (0, int(b.count[0])), (1, int(b.count[1]) + 7)] + sel[::-1]
    assert len(more) % 256 != 0 and len(more) > 512
    _check(ctx, b, more, EIGHT)
    first = long_[0]
    for m in (1, 63, 64, 65, 257):
        part = (sel[first:] + sel)[:m]  # (a long entry first: the only entry of m = 1 takes the wave path)
        for names in ([], [b"b"], EIGHT):
            _check(ctx, b, part, names)
    _check(ctx, b, more, [])


def oo_members(s):
    from member_oracle import members_boundaries
    return members_boundaries(s, *oo.index_set(s), [b"meta"])


def test_bounds(ctx):
    rng = np.random.default_rng(4)
    streams = [b"\n".join(oo.gen_line(rng) for _ in range(int(rng.integers(0, 12)))) for _ in range(12)]
    streams += [b'{"a":{' + b'"b":1,' * 1500 + b'"a":2}}', b'{"a":{' + b'"u":{"a":1},' * 40 + b'"b":2}}']
    b = Batch(streams)
    sel = b.openers() + [(i, int(b.count[i]) + d) for i in range(b.n) for d in (-1, 0, 1) if int(b.count[i]) + d >= 0]
    _check(ctx, b, sel, oo.NAMES)
    for cut in (1, 17, 1400, b.n_pos // 3, b.n_pos - 1, b.n_pos):  # n_pos below sum(count), inside the long object too
        c = Batch(streams)
        c.n_pos = b.n_pos - cut
        _check(ctx, c, sel, ABCUX)  # (upload() puts closers and huge positions behind n_pos)
    g = Batch(streams)                   # garbage in pos: decreasing, beyond len
    g.pos = g.pos[::-1].copy()
    g.pos[::3] += 1 << 33
    _check(ctx, g, sel, ABCUX)
    w = Batch(streams)                   # garbage in what
    w.what[::5] = rng.integers(0, 256, len(w.what[::5])).astype(np.uint8)
    w.what[1::7] = 0
    _check(ctx, w, [(i, k) for i in range(w.n) for k in range(0, int(w.count[i]), 3)] + w.openers(), ABCUX)
    k = Batch(streams)                   # counts that reach beyond n_pos and into the neighbours
    k.count = k.count + rng.integers(0, 50, k.n)
    k.count[-1] += 1 << 40
    _check(ctx, k, sel + [(k.n - 1, int(b.count[-1]) + 5), (0, int(b.count[0]) + 3)], ABCUX)
    _check(ctx, k, sel, [])


def test_optional_outputs(ctx):
    rng = np.random.default_rng(5)
    streams = [_object(d, 1, rng) for d in (1, 2, 3, 9, 17, L + 5, R + 9, 2 * R + 40, 30, 5)] + [b'{" a\\\\":1}', b"[1]"]
    b = Batch(streams)
    sel = [(i, 0) for i in range(b.n)] + [(b.n, 0), (0, NONE)]
    for given in ((False, False, False, False), (False, True, True, True), (True, False, True, True), (True, True, False, True),
                  (True, True, True, False)):
        want = _check(ctx, b, sel, ABCUX, given=given)
    assert want[6][10] == oo.ESCAPED_KEY and want[1][11] == oo.NOT_OBJECT
    for given in ((True, False, False, False), (True, False, True, False), (True, True, False, False)):
        _check(ctx, b, sel, [], given=given)  # the extent mode: n_members is required there


def test_on_a_stream_behind_index_set_and_member(ctx):
    """index_set_batch (count, fill), member_batch (count, fill) and object_batch twice -- one level down and two -- enqueued on one
    caller's stream, nothing in between: the totals come from the CPU."""
    import torch
    rng = np.random.default_rng(6)
    lines = [[oo.gen_line(rng) for _ in range(int(rng.integers(1, 40)))] for _ in range(16)]
    b = Batch([b"\n".join(part) for part in lines]).upload()
    n, total = b.n, b.n_pos
    M = sum(len(part) for part in lines)
    count = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    pos = torch.full((total + SPARE,), -7, dtype=torch.int64, device="cuda:0")
    what = torch.full((total + SPARE,), 0x7D, dtype=torch.uint8, device="cuda:0")
    d_lines = torch.full((n,), P64, dtype=torch.int64, device="cuda:0")
    d_ss = torch.full((M,), P32, dtype=torch.int32, device="cuda:0")
    d_sr = torch.full((M,), P64, dtype=torch.int64, device="cuda:0")
    d_kind = torch.full((M,), P8, dtype=torch.uint8, device="cuda:0")
    Q = len(oo.NAMES)
    o1 = [_Out(M, torch.int64, P64), _Out(M, torch.uint8, P8), _Out(M, torch.int64, P64), _Out(Q * M, torch.int32, P32), _Out(Q * M, torch.int64, P64),
          _Out(Q * M, torch.uint8, P8), _Out(M, torch.uint8, P8)]
    o2 = [_Out(M, torch.int64, P64), _Out(M, torch.uint8, P8), _Out(M, torch.int64, P64), _Out(M, torch.int32, P32), _Out(M, torch.int64, P64),
          _Out(M, torch.uint8, P8), _Out(M, torch.uint8, P8)]
    s = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        args = (b"{}[]:,\n", 0x22, 0x5C, 0, b.arena.data_ptr(), b.d_off.data_ptr(), b.d_len.data_ptr(), n, int(b.arena.numel()))
        ctx.index_set_batch_device(*args, count.data_ptr(), None, hip_stream=s.cuda_stream)
        pos_off = torch.cumsum(count, 0) - count
        ctx.index_set_batch_device(*args, None, None, pos_off.data_ptr(), pos.data_ptr(), what.data_ptr(), total, hip_stream=s.cuda_stream)
        head = args[4:] + (count.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), what.data_ptr(), total)
        ctx.member_batch_device(*head, [b"meta"], d_lines.data_ptr(), hip_stream=s.cuda_stream)
        d_line_off = torch.cumsum(d_lines, 0) - d_lines
        ctx.member_batch_device(*head, [b"meta"], None, d_line_off.data_ptr(), M, d_ss.data_ptr(), d_sr.data_ptr(), d_kind.data_ptr(), None,
                                hip_stream=s.cuda_stream)
        ctx.object_batch_device(*head, d_ss.data_ptr(), d_sr.data_ptr(), M, oo.NAMES, *[o.ptr() for o in o1], hip_stream=s.cuda_stream)
        # one level further down: the column of "u" of the first call is the selection of the second
        u = oo.NAMES.index(b"u")
        ctx.object_batch_device(*head, o1[3].ptr() + 4 * u * M, o1[4].ptr() + 8 * u * M, M, [b"a"], *[o.ptr() for o in o2], hip_stream=s.cuda_stream)
    s.synchronize()
    found = [cur[0] for st in b.streams for cur in oo_members(st)[1]]  # (kind, rec) of "meta": a later duplicate may be no object
    sel = [(i, cur[0][1]) for i, st in enumerate(b.streams) for cur in oo_members(st)[1]]
    assert d_kind.cpu().tolist() == [kd for kd, _ in found] and d_sr.cpu().tolist() == [r for _, r in sel]
    assert [kd for kd, _ in found].count(oo.OBJECT) > M // 2
    want = oo.batch(b.streams, b.tables(), sel, oo.NAMES)
    got = [o.host() for o in o1]
    flat = lambda rows: [x for row in rows for x in row]
    for g_, w_ in zip(got, (want[0], want[1], want[2], flat(want[3]), flat(want[4]), flat(want[5]), want[6])):
        assert g_.tolist() == np.array(w_, dtype=np.uint64).view(np.int64).tolist()
    sel2 = list(zip(want[3][u], want[4][u]))
    want2 = oo.batch(b.streams, b.tables(), sel2, [b"a"])
    got2 = [o.host() for o in o2]
    for g_, w_ in zip(got2, (want2[0], want2[1], want2[2], flat(want2[3]), flat(want2[4]), flat(want2[5]), want2[6])):
        assert g_.tolist() == np.array(w_, dtype=np.uint64).view(np.int64).tolist()
    assert want2[1].count(oo.OK) > 10 and want2[1].count(oo.NONE) > 20 and oo.NOT_OBJECT in want2[1]  # "u" is an object only in places


def test_differential_on_generated_lines(ctx):
    rng = np.random.default_rng(20251021)
    streams = []
    for _ in range(60):
        part = []
        for _ in range(int(rng.integers(0, 30))):
            line = oo.gen_line(rng)
            part.append(oo.break_line(rng, line) if rng.integers(0, 5) == 0 else line)
        streams.append(b"\n".join(part))
    b = Batch(streams)
    sel = b.openers()
    want = _check(ctx, b, sel, oo.NAMES)
    assert len(sel) > 3000 and set(want[1]) == {oo.OK, oo.UNCLOSED, oo.MISMATCH}
    assert set(x for row in want[5] for x in row) == {oo.MISSING, oo.SCALAR, oo.OBJECT, oo.ARRAY, oo.BAD}
    for j, (i, r) in list(enumerate(sel))[::9]:  # the other statement of the rule, which never sees pos or what, on a part
        st, end, members, found, flags = oo.object_bytes(b.streams[i], r, oo.NAMES)
        assert (st, end, members, flags) == (want[1][j], want[2][j], want[0][j], want[6][j]), (i, r)
        assert {q: (want[5][q][j], want[4][q][j]) for q in range(len(oo.NAMES)) if want[5][q][j]} == found, (i, r)


def test_end_to_end_from_compressed_streams(ctx):
    """Brotli streams (hand-assembled, tests/craft.py) of JSON Lines {"meta":{"lang":...,"score":...,"geo":{"lat":...}},"items":[{"id":...,
    "price":...},...]} in shuffled key order: decode, index_set_batch, member_batch, then object_batch -> parse_f64_batch /
    unescape_batch for the members of "meta"; elements_batch -> object_batch -> parse_batch / parse_f64_batch for the objects of
    "items"; object_batch twice for the three-level path meta.geo.lat -- all equal to json.loads, exactly."""
    import torch
    rng = np.random.default_rng(7)
    langs = ["en", "de", "pt-BR", 'q"uo\\te', "日本", "", "a}{:,b"]
    texts, rows = [], []
    for i in range(10):
        part = []
        for r in range(int(rng.integers(1, 30))):
            meta = {"lang": langs[int(rng.integers(0, len(langs)))], "score": float(np.round(rng.uniform(0, 1), int(rng.integers(1, 12)))),
                    "geo": {"lat": float(rng.uniform(-90, 90)), "lon": float(rng.uniform(-180, 180))}}
            items = [{"id": int(rng.integers(-2**40, 2**40)), "price": float(np.round(rng.uniform(0, 999), 2)), "tags": ["id", {"id": -1}]}
                     for _ in range(int(rng.integers(0, 9)))]
            row = {"meta": meta, "items": items, "id": r, "price": "top", "lang": {"lang": 1}}
            keys = list(row)
            rng.shuffle(keys)
            mk = list(meta)
            rng.shuffle(mk)
            row = {k: ({q: meta[q] for q in mk} if k == "meta" else row[k]) for k in keys}
            part.append(json.dumps(row, separators=oo.SPACINGS[int(rng.integers(0, 3))][:2], ensure_ascii=bool(rng.integers(0, 2))))
            rows.append(row)
        texts.append("\n".join(part).encode("utf-8"))
    streams = []
    for t in texts:
        bits = craft.Bits()
        craft.stream_header(bits)
        for at in range(0, len(t), 700):
            craft.raw_block(bits, t[at:at + 700])
        bits.put(1, 1)
        bits.put(1, 1)  # ISLAST, ISLASTEMPTY
        streams.append(bits.bytes())
    n = len(texts)
    in_off = np.concatenate([[0], np.cumsum([len(x) for x in streams])]).astype(np.int64)
    caps = [len(t) + 40 + 7 * i for i, t in enumerate(texts)]
    out_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    blob, d_in_off, offs = _dev(np.frombuffer(b"".join(streams), dtype=np.uint8)), _dev(in_off), _dev(out_off)
    out = torch.full((int(out_off[-1]),), 0x7B, dtype=torch.uint8, device="cuda:0")
    lens = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    ctx.decode_batch_device(blob.data_ptr(), d_in_off.data_ptr(), n, out.data_ptr(), offs.data_ptr(), lens.data_ptr(), status.data_ptr())
    assert status.cpu().tolist() == [0] * n and lens.cpu().tolist() == [len(t) for t in texts]
    offs = offs[:n]
    count, _, pos_off, pos, what = ctx.index_set_batch(out, offs, lens, delims=b"{}[]:,\n")
    tabs = (out, offs, lens, count, pos_off, pos)
    lines, line_off, ss, sr, kind, flags = ctx.member_batch(*tabs, what, [b"meta", b"items"])
    M = len(rows)
    assert int(lines.sum().item()) == M and (kind[0] == MEMBER_OBJECT).all().item() and (kind[1] == MEMBER_ARRAY).all().item()
    # meta.lang, meta.score, meta.geo
    n_mem, st, end, ms, mr, mk, fl = ctx.object_batch(*tabs, what, ss[0], sr[0], [b"lang", b"score", b"geo"])
    assert (n_mem == 3).all().item() and (st == OBJECT_OK).all().item() and not fl.any().item()
    assert (mk[:2] == MEMBER_SCALAR).all().item() and (mk[2] == MEMBER_OBJECT).all().item()
    assert (what.cpu().numpy()[(pos_off[ss[0].long()] + end).cpu().numpy()] == 0x7D).all()  # `end` is the closing brace
    score, vst = ctx.parse_f64_batch(*tabs, sel_stream=ms[1], sel_rec=mr[1], spaces=True)
    assert (vst == PARSE_OK).all().item() and score.cpu().tolist() == [row["meta"]["score"] for row in rows]
    dst, dst_off, text_len, tst = ctx.unescape_batch(*tabs, sel_stream=ms[0], sel_rec=mr[0], dialect="json", spaces=True)
    assert (tst == TEXT_OK).all().item()
    raw, o_, l_ = dst.cpu().numpy().tobytes(), dst_off.cpu().tolist(), text_len.cpu().tolist()
    assert [raw[a:a + c].decode("utf-8") for a, c in zip(o_, l_)] == [row["meta"]["lang"] for row in rows]
    # the three-level path meta.geo.lat: object twice
    n2, st2, _, gs, gr, gk, _ = ctx.object_batch(*tabs, what, ms[2], mr[2], [b"lat"])
    assert (n2 == 2).all().item() and (st2 == OBJECT_OK).all().item() and (gk == MEMBER_SCALAR).all().item()
    lat, vst = ctx.parse_f64_batch(*tabs, sel_stream=gs[0], sel_rec=gr[0], spaces=True)
    assert (vst == PARSE_OK).all().item() and lat.cpu().tolist() == [row["meta"]["geo"]["lat"] for row in rows]
    # items[*].id, items[*].price: member -> elements -> object -> parse
    n_e, e_off, est, _, es, er, ek = ctx.elements_batch(*tabs, what, ss[1], sr[1])
    assert n_e.cpu().tolist() == [len(row["items"]) for row in rows] and (ek == MEMBER_OBJECT).all().item()
    n3, st3, _, is_, ir, ik, _ = ctx.object_batch(*tabs, what, es, er, [b"id", b"price", b"tags", b"lang"])
    E = sum(len(row["items"]) for row in rows)
    assert n3.cpu().tolist() == [3] * E and (st3 == OBJECT_OK).all().item() and (ik[2] == MEMBER_ARRAY).all().item() and (ik[3] == 0).all().item()
    ids, ist = ctx.parse_batch(*tabs, sel_stream=is_[0], sel_rec=ir[0], spaces=True)
    price, pst = ctx.parse_f64_batch(*tabs, sel_stream=is_[1], sel_rec=ir[1], spaces=True)
    torch.cuda.synchronize()
    assert (ist == PARSE_OK).all().item() and ids.cpu().tolist() == [it["id"] for row in rows for it in row["items"]]
    assert (pst == PARSE_OK).all().item() and price.cpu().tolist() == [it["price"] for row in rows for it in row["items"]]
    # the extent mode over the same openers: the same counts and closers, nothing else
    n4, st4, end4, none_s, none_r, none_k, none_f = ctx.object_batch(*tabs, what, es, er)
    assert none_s is None and none_r is None and none_k is None and none_f is None
    assert torch.equal(n4, n3) and torch.equal(st4, st3)
