"""brx_elements_batch (include/brx.h, brx_elements.hip): the elements of JSON arrays as selections for the record calls.  Every expected
value comes from tests/elements_oracle.py (its two statements are held to each other, to the contract's check values and to json.loads
by tests/test_elements_abi.py): the boundary-serial statement over the very pos / what / count / n_pos that the call gets, so that cut
and garbage tables have an expectation too.  Every output is pre-filled with poison and carries a canary region behind m (behind
total) that must be unchanged; in fill mode every slot that holds no element must be unchanged too.  In-process, one context."""
import json
import os
import re

import numpy as np
import pytest

import brx_knobs
import elements_oracle as eo
from brotli_rs_amd.brx import ELEMENTS_OK, MEMBER_ARRAY, PARSE_OK  # noqa: F401  (without the call nothing here runs)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_H = open(os.path.join(ROOT, "brotli-rs_amd", "csrc", "brx_elements.h")).read()
_HM = open(os.path.join(ROOT, "brotli-rs_amd", "csrc", "brx_member.h")).read()
L = 16 * int(re.search(r"#define\s+BRX_EL_UNITS\s+(\d+)u", _H).group(1))  # boundaries that one lane walks alone
R = int(re.search(r"#define\s+BRX_MB_ROW\s+(\d+)u", _HM).group(1))         # boundaries per wave step
P64, P32, P8 = 0x5151515151515151, 0x51515151, 0x51
SPARE = 16
NONE = (1 << 64) - 1


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
    """Streams in an arena (brackets, quotes and commas between them) with the tables of an index at {}[]:,\\n computed on the CPU --
    or whatever the test puts in their place."""

    def __init__(self, streams, per=None):
        self.streams = [bytes(s) for s in streams]
        self.n = len(self.streams)
        parts, offs, at = [b'["]'], [], 3
        for p, s in enumerate(self.streams):
            offs.append(at)
            gap = b'],"[\n'[:1 + p % 5]
            parts += [s, gap]
            at += len(s) + len(gap)
        self.host = np.frombuffer(b"".join(parts), dtype=np.uint8)
        self.offs, self.lens = np.array(offs, dtype=np.int64), np.array([len(s) for s in self.streams], dtype=np.int64)
        per = [eo.index_set(s) for s in self.streams] if per is None else per  # (per: the index of every stream, where the test has it)
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
        self.d_what = _dev(np.concatenate([self.what[:self.n_pos], np.full(SPARE, 0x5D, dtype=np.uint8)]))
        return self

    def head(self):
        return (self.arena.data_ptr(), self.d_off.data_ptr(), self.d_len.data_ptr(), self.n, int(self.arena.numel()),
                self.d_count.data_ptr(), self.d_pos_off.data_ptr(), self.d_pos.data_ptr(), self.d_what.data_ptr(), self.n_pos)

    def want(self, sel):
        """the oracle's boundary-serial statement over these very tables, for the pairs of `sel` -> [(status, end, elements)]"""
        if getattr(self, "_memo_for", None) != (self.n_pos, self.what.tobytes(), self.pos.tobytes(), self.count.tobytes()):
            self._memo_for, self._memo = (self.n_pos, self.what.tobytes(), self.pos.tobytes(), self.count.tobytes()), {}
        memo, out = self._memo, []  # (one walk per pair and state of the tables, however many calls ask)
        what = bytes(self.what)
        for i, r in sel:
            if (i, r) not in memo:
                if i >= self.n:
                    memo[(i, r)] = (eo.NONE, eo.NO_END, [])
                else:
                    a = int(self.pos_off[i])
                    left = max(0, self.n_pos - a)
                    c = min(int(self.count[i]), left)
                    memo[(i, r)] = eo.elements_boundaries(self.streams[i], [int(x) for x in self.pos[a:a + c]], what[a:a + c], r, count=c, n_pos=left)
            out.append(memo[(i, r)])
        return out


def _check(ctx, b, sel, rooms=None, total=None, el_off=None, optional=(True, True, True), hip_stream=None, sync=None):
    """Count mode and fill mode against the oracle.  rooms: per entry, instead of its number of elements; total: instead of their sum;
    el_off: instead of the rooms' prefix sum; optional: whether fill mode gets n_elem, status, end.  -> what the oracle says"""
    import torch
    if not hasattr(b, "arena"):
        b.upload()
    want = b.want(sel)
    m = len(sel)
    d_ss = _dev(np.array([i for i, _ in sel] + [0] * SPARE, dtype=np.int64), torch.int32)
    d_sr = _dev(_u64([r for _, r in sel] + [2] * SPARE))
    w_n = np.array([len(w[2]) for w in want], dtype=np.int64)
    w_st = np.array([w[0] for w in want], dtype=np.int64)
    w_end = _u64([w[1] for w in want])
    d_n = torch.full((m + SPARE,), P64, dtype=torch.int64, device="cuda:0")
    d_st = torch.full((m + SPARE,), P8, dtype=torch.uint8, device="cuda:0")
    d_end = torch.full((m + SPARE,), P64, dtype=torch.int64, device="cuda:0")

    def results(given):
        for name, d, w, poison, on in (("n_elem", d_n, w_n, P64, given[0]), ("status", d_st, w_st, P8, given[1]), ("end", d_end, w_end, P64, given[2])):
            got = d.cpu().numpy().astype(np.int64)
            if on:
                bad = np.flatnonzero(got[:m] != w)
                assert bad.size == 0, (name, bad[:5].tolist(), [sel[x] for x in bad[:5]], got[bad[:5]].tolist(), w[bad[:5]].tolist())
                assert (got[m:] == poison).all(), name  # the canary
            else:
                assert (got == poison).all(), name

    torch.cuda.synchronize()
    ctx.elements_batch_device(*b.head(), d_ss.data_ptr(), d_sr.data_ptr(), m, d_n.data_ptr(), d_st.data_ptr(), d_end.data_ptr(), hip_stream=hip_stream)
    if sync:
        sync()
    results((True, True, True))
    # fill mode
    rooms = w_n if rooms is None else np.array(rooms, dtype=np.int64)
    off = (np.cumsum(rooms) - rooms) if el_off is None else np.array(el_off, dtype=np.int64)
    total = int(rooms.sum()) if total is None else total
    e_ss, e_sr, e_kd = np.full(total + SPARE, P32, dtype=np.int64), np.full(total + SPARE, P64, dtype=np.int64), np.full(total + SPARE, P8, dtype=np.int64)
    for j, (w, (i, _)) in enumerate(zip(want, sel)):
        room = max(0, (int(off[j + 1]) if j + 1 < m else total) - int(off[j]))
        for t, (rec, kd) in enumerate(w[2][:room]):
            if int(off[j]) + t < total:
                e_ss[off[j] + t], e_sr[off[j] + t], e_kd[off[j] + t] = i, rec, kd
    d_off = _dev(np.concatenate([off, np.zeros(1, dtype=np.int64)]))
    d_es = torch.full((total + SPARE,), P32, dtype=torch.int32, device="cuda:0")
    d_er = torch.full((total + SPARE,), P64, dtype=torch.int64, device="cuda:0")
    d_ek = torch.full((total + SPARE,), P8, dtype=torch.uint8, device="cuda:0")
    for d, p in ((d_n, P64), (d_st, P8), (d_end, P64)):
        d.fill_(p)
    torch.cuda.synchronize()
    ctx.elements_batch_device(*b.head(), d_ss.data_ptr(), d_sr.data_ptr(), m, d_n.data_ptr() if optional[0] else None,
                              d_st.data_ptr() if optional[1] else None, d_end.data_ptr() if optional[2] else None, d_off.data_ptr(), total,
                              d_es.data_ptr(), d_er.data_ptr(), d_ek.data_ptr(), hip_stream=hip_stream)
    if sync:
        sync()
    results(optional)
    for name, d, e in (("el_stream", d_es, e_ss), ("el_rec", d_er, e_sr), ("el_kind", d_ek, e_kd)):
        got = d.cpu().numpy().astype(np.int64)
        bad = np.flatnonzero(got != e)  # the elements, the slots that hold none and the canary behind total
        assert bad.size == 0, (name, total, bad[:5].tolist(), got[bad[:5]].tolist(), e[bad[:5]].tolist())
    return want


def _array(dist, style, rng):
    """an array whose closer stands `dist` boundaries behind its opener: style 0 numbers only, 1 nested values and strings too"""
    s, have = b"[", 0
    while have + 1 < dist:
        left = dist - 1 - have
        pick = 0 if style == 0 else int(rng.integers(0, 6))
        if pick == 1 and left >= 4:
            s, have = s + b"[1,2]", have + 3
        elif pick == 2 and left >= 5:
            s, have = s + b'{"k":[]}', have + 5
        elif pick == 3:
            s += b'"a],[b\\""'
        elif pick == 4:
            s += b" 1.5e3 "
        else:
            s += b"%d" % int(rng.integers(0, 100))
        if have + 1 < dist:
            s, have = s + b",", have + 1
    return s + b"]"


def _openers(b):
    """every '[' boundary of every stream, as pairs"""
    return [(i, k) for i in range(b.n) for k in range(int(b.count[i])) if b.what[int(b.pos_off[i]) + k] == 0x5B]


def test_the_thresholds_are_the_headers():
    assert L % 16 == 0 and L >= 16 and R == 64 * 16 and L < R
    assert (ELEMENTS_OK, MEMBER_ARRAY) == (eo.OK, eo.ARRAY)


def test_check_values_of_the_contract(ctx):
    for stream, r, status, els, end in eo.CHECK:
        assert _check(ctx, Batch([stream]), [(0, r)]) == [(status, end, els)], stream
    b = Batch([c[0] for c in eo.CHECK])  # all of them as one batch, every boundary of every stream an opener and two behind
    _check(ctx, b, [(i, r) for i in range(b.n) for r in range(int(b.count[i]) + 2)])


def test_short_arrays_and_blanks(ctx):
    bodies = [b"", b" ", b"\t\r ", b" " * 63, b" " * 64, b" " * 65, b" " * 63 + b"\t", b" " * 31 + b"x" + b" " * 32, b" " * 200, b"1", b" 1 ", b'"]"',
              b"1,2", b" 1 , 2 ", b",", b"1,", b",1", b"[]", b"[ ],[]", b"{}", b'{"a":[]},[[]]', b":", b"1:2,3"]
    streams = [b'{"a":[' + x + close + tail for x in bodies for close in (b"]", b"}") for tail in (b"}", b',"b":[2]}\n', b"")]
    b = Batch(streams)
    want = _check(ctx, b, [(i, 2) for i in range(b.n)])
    by_body = {streams[i]: w for i, w in enumerate(want)}
    assert [len(by_body[b'{"a":[' + x + b"]}"][2]) for x in bodies[:9]] == [0, 0, 0, 0, 0, 1, 0, 1, 1]
    assert by_body[b'{"a":[1,2}}'][0] == eo.MISMATCH and by_body[b'{"a":[}}'] == (eo.MISMATCH, 3, [])
    _check(ctx, b, _openers(b))


def test_closer_distances_at_every_phase(ctx):
    """The closer 1, 2, 3, 15, 16, 17, L - 1, L, L + 1, R - 1, R, R + 1 and 2R + 3 boundaries behind the opener, the opener at each of
    the 16 phases of `what`; closed by ']' and by '}', cut by a line feed and by the stream's end; numbers only and nested values."""
    rng = np.random.default_rng(1)
    dists = sorted(set([1, 2, 3, 15, 16, 17, L - 1, L, L + 1, R - 1, R, R + 1, 2 * R + 3]))
    streams, per, sel, tot = [], [], [], 0
    for phase in range(16):
        for q, d in enumerate(dists):
            a = _array(d, (phase + q) % 2, rng)
            for v in range(4 if d > 2 else 1):
                body = (a + b"}\n", a[:-1] + b"},1]", a[:-1] + b"\n[1]", a[:-1])[v]
                lead = (phase - tot) % 16
                streams.append(b"," * lead + body)
                per.append(eo.index_set(streams[-1]))
                sel.append((len(streams) - 1, lead))
                tot += len(per[-1][0])
    b = Batch(streams, per)
    assert set((int(b.pos_off[i]) + r) % 16 for i, r in sel) == set(range(16))
    want = _check(ctx, b, sel)
    assert set(w[0] for w in want) == {eo.OK, eo.MISMATCH, eo.UNCLOSED}
    assert set(w[1] - r for w, (_, r) in zip(want, sel)) >= set(dists)
    _check(ctx, b, sel[::-1] + sel[::7])  # another order, repeats, m not a multiple of the block
    assert (len(sel) + len(sel[::7])) % 256 != 0


def test_the_stop_in_lane_0_lane_63_and_a_second_row(ctx):
    """The stop (a closer, a line feed, the stream's end) at given offsets behind the opener: inside the lane path; in lane 63 of the
    first row; in lane 0 and lane 63 of a second and a third row; with commas (separators) or colons (neutral) in front of it."""
    offsets = [0, 15, L - 1, L, R - 16, R - 1, R, R + 15, 2 * R - 1, 2 * R, 2 * R + 1, 3 * R - 1]
    streams = []
    for at in offsets:
        for fill in (b",", b":"):
            streams += [b"[" + fill * at + b"]", b"[" + fill * at + b"\n]", b"[" + fill * at, b"[" + fill * at + b"}", b"[1" + fill * at + b"[]"]
    b = Batch(streams)
    want = _check(ctx, b, [(i, 0) for i in range(b.n)])
    assert [w[1] for w in want[:5]] == [1, 1, 1, 1, 3] and want[10 * offsets.index(R - 16)][1] == R - 16 + 1
    _check(ctx, b, _openers(b))


def test_nested_elements_across_lanes_and_rows(ctx):
    deep = b"[" * 1500 + b"1" + b"]" * 1500
    streams = [
        b"[1," + deep + b",2," + deep + b"]",                     # inner closers in later lanes and rows than their openers
        b"[" + deep[:2800] + b"\n",                                # ... and a line feed before the depth comes back
        b"[" + b"," * 3000 + b"]",                                 # bracket-free rows of commas only
        b"[[" + b"," * 2500 + b"]," + b"," * 1100 + b"{" + b"," * 1030 + b"}]",  # rows of commas at depth 2: none is a separator
        b"[1,[" + b"," * 40 + b'],2,{"a":[' + b"," * 1000 + b"]},3" + b"," * 1024 + b"]",
        b"[" + b"[1,2]," * 700 + b'{"k":[1,{"k":2}]}]',            # nested elements in every lane
        b"[" + b"1:2," * 600 + b"]",                               # BAD elements
    ]
    b = Batch(streams)
    want = _check(ctx, b, [(i, 0) for i in range(b.n)])
    assert [len(w[2]) for w in want] == [4, 0, 3001, 1102, 1029, 701, 601] and want[1][0] == eo.UNCLOSED
    assert set(kd for _, kd in want[6][2]) == {eo.BAD, eo.SCALAR}
    sel = _openers(b)
    _check(ctx, b, sel[:100] + sel[1450:1560] + sel[-100:])       # the nested openers: arrays that end at every depth


def test_long_and_short_entries_in_one_wave(ctx):
    """Several long arrays in one wave next to short ones and entries that select nothing; a selection with repeats, MISSING, streams
    behind n and a whole column of member's output (SCALAR and OBJECT openers included); m not a multiple of the block."""
    rng = np.random.default_rng(3)
    lines, arrs = [], []
    for k in range(300):
        ne = (0, 1, 2, 5, 40, 70, 300, 1100)[int(rng.integers(0, 8))] if k % 3 else int(rng.integers(0, 9))
        v = [[1.5, [2, 3], {"a": [k]}, "x],[", None][int(rng.integers(0, 5))] if rng.integers(0, 4) == 0 else int(x) for x in rng.integers(-99, 99, ne)]
        row = {"id": k, "arr": v if k % 7 else (7 if k % 14 else {"arr": v}), "t": "[,"}
        keys = list(row)
        rng.shuffle(keys)
        if k % 11 == 0:
            del row["arr"]
            keys.remove("arr")
        lines.append(json.dumps({q: row[q] for q in keys}, separators=eo.SPACINGS[k % 3]).encode())
        arrs.append(row.get("arr"))
    arrs.insert(200, None)  # the trailing line of the first stream
    b = Batch([b"\n".join(lines[:200]) + b"\n", b"\n".join(lines[200:])])
    sel, kinds = [], []
    for i, s in enumerate(b.streams):  # member's column for "arr", by member's oracle
        _, found, _ = eo.members_boundaries(s, *eo.index_set(s), [b"arr"])
        for cur in found:
            kd, rec = cur.get(0, (0, NONE))
            sel.append((i, rec))
            kinds.append(kd)
    assert len(sel) == 301 and set(kinds) == {0, eo.SCALAR, eo.OBJECT, eo.ARRAY}
    want = _check(ctx, b, sel)
    for (st, end, els), kd, arr in zip(want, kinds, arrs):
        assert st == (eo.OK if kd == eo.ARRAY else eo.NONE if kd == 0 else eo.NOT_ARRAY)
        if kd == eo.ARRAY:
            assert len(els) == len(arr)
    more = sel + sel[::3] + [(2, 0), (5, 1), (1 << 31, 0), (0, NONE), (1, NONE - 1)] + sel[::-1]
    assert len(more) % 256 != 0 and len(more) > 512
    _check(ctx, b, more)
    _check(ctx, b, more[:1])
    _check(ctx, b, more[:65])


def test_bounds(ctx):
    rng = np.random.default_rng(4)
    streams = [b"\n".join(eo.gen_line(rng)[0] for _ in range(int(rng.integers(0, 12)))) for _ in range(12)]
    streams += [b'{"a":[' + b"1," * 1500 + b"2]}", b'{"a":[' + b"[1]," * 40 + b"2]}"]
    b = Batch(streams)
    sel = _openers(b) + [(i, int(b.count[i]) + d) for i in range(b.n) for d in (-1, 0, 1) if int(b.count[i]) + d >= 0]
    _check(ctx, b, sel)
    for cut in (1, 17, 1400, b.n_pos // 3, b.n_pos - 1, b.n_pos):  # n_pos below sum(count), inside the long array too
        c = Batch(streams)
        c.n_pos = b.n_pos - cut
        _check(ctx, c, sel)  # (upload() puts closers and huge positions behind n_pos)
    g = Batch(streams)                   # garbage in pos: decreasing, beyond len
    g.pos = g.pos[::-1].copy()
    g.pos[::3] += 1 << 33
    _check(ctx, g, sel)
    w = Batch(streams)                   # garbage in what
    w.what[::5] = rng.integers(0, 256, len(w.what[::5])).astype(np.uint8)
    w.what[1::7] = 0
    _check(ctx, w, [(i, k) for i in range(w.n) for k in range(0, int(w.count[i]), 3)] + _openers(w))
    k = Batch(streams)                   # counts that reach beyond n_pos and into the neighbours
    k.count = k.count + rng.integers(0, 50, k.n)
    k.count[-1] += 1 << 40
    _check(ctx, k, sel + [(k.n - 1, int(b.count[-1]) + 5), (0, int(b.count[0]) + 3)])


def test_rooms_total_and_optional_outputs(ctx):
    rng = np.random.default_rng(5)
    streams = [_array(d, 1, rng) for d in (1, 2, 3, 9, 17, L + 5, R + 9, 2 * R + 40, 30, 5)]
    b = Batch(streams)
    sel = [(i, 0) for i in range(b.n)]
    n = [len(w[2]) for w in b.want(sel)]
    assert min(n) == 0 and max(n) > 300
    _check(ctx, b, sel, rooms=[max(0, x - 1 - x // 3) for x in n])                  # every room below the number of elements
    _check(ctx, b, sel, rooms=[x + 2 for x in n])                                    # ... above it: the slots behind stay as they were
    _check(ctx, b, sel, rooms=[0] * len(n))
    for cut in (1, 3, n[-1], n[-1] + n[-2] + 1, sum(n[-3:]) + R):                    # a total that cuts the last entries
        _check(ctx, b, sel, total=max(0, sum(n) - cut))
    _check(ctx, b, sel, total=0)
    four = [(3, 0), (4, 0), (3, 0), (8, 0)]                                          # an el_off that runs backwards: a room below 0
    m4 = [len(w[2]) for w in b.want(four)]
    assert m4[0] <= 10 and m4[2] <= 10 and m4[3] > 2
    _check(ctx, b, four, el_off=[0, 40, 20, 30], total=30 + m4[3] - 2)
    for optional in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        _check(ctx, b, sel, optional=optional)


def test_on_a_stream_behind_index_set_and_member(ctx):
    """index_set_batch, member_batch and elements_batch (count, fill each) enqueued on one caller's stream, nothing in between: the
    totals come from the CPU."""
    import torch
    rng = np.random.default_rng(6)
    lines = [[eo.gen_line(rng) for _ in range(int(rng.integers(1, 40)))] for _ in range(16)]
    b = Batch([b"\n".join(x[0] for x in part) for part in lines]).upload()
    n, total = b.n, b.n_pos
    M = sum(len(part) for part in lines)
    sel = []
    for i, s in enumerate(b.streams):
        _, found, _ = eo.members_boundaries(s, *eo.index_set(s), [b"arr"])
        sel += [(i, cur[0][1]) for cur in found]
    want = b.want(sel)
    E = sum(len(w[2]) for w in want)
    count = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    pos = torch.full((total + SPARE,), -7, dtype=torch.int64, device="cuda:0")
    what = torch.full((total + SPARE,), 0x5D, dtype=torch.uint8, device="cuda:0")
    d_lines = torch.full((n,), P64, dtype=torch.int64, device="cuda:0")
    d_ss = torch.full((M,), P32, dtype=torch.int32, device="cuda:0")
    d_sr = torch.full((M,), P64, dtype=torch.int64, device="cuda:0")
    d_kind = torch.full((M,), P8, dtype=torch.uint8, device="cuda:0")
    d_n = torch.full((M + SPARE,), P64, dtype=torch.int64, device="cuda:0")
    d_st = torch.full((M + SPARE,), P8, dtype=torch.uint8, device="cuda:0")
    d_end = torch.full((M + SPARE,), P64, dtype=torch.int64, device="cuda:0")
    d_es = torch.full((E + SPARE,), P32, dtype=torch.int32, device="cuda:0")
    d_er = torch.full((E + SPARE,), P64, dtype=torch.int64, device="cuda:0")
    d_ek = torch.full((E + SPARE,), P8, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        args = (b"{}[]:,\n", 0x22, 0x5C, 0, b.arena.data_ptr(), b.d_off.data_ptr(), b.d_len.data_ptr(), n, int(b.arena.numel()))
        ctx.index_set_batch_device(*args, count.data_ptr(), None, hip_stream=s.cuda_stream)
        pos_off = torch.cumsum(count, 0) - count
        ctx.index_set_batch_device(*args, None, None, pos_off.data_ptr(), pos.data_ptr(), what.data_ptr(), total, hip_stream=s.cuda_stream)
        head = args[4:] + (count.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), what.data_ptr(), total)
        ctx.member_batch_device(*head, [b"arr"], d_lines.data_ptr(), hip_stream=s.cuda_stream)
        d_line_off = torch.cumsum(d_lines, 0) - d_lines
        ctx.member_batch_device(*head, [b"arr"], None, d_line_off.data_ptr(), M, d_ss.data_ptr(), d_sr.data_ptr(), d_kind.data_ptr(), None,
                                hip_stream=s.cuda_stream)
        ctx.elements_batch_device(*head, d_ss.data_ptr(), d_sr.data_ptr(), M, d_n.data_ptr(), d_st.data_ptr(), d_end.data_ptr(), hip_stream=s.cuda_stream)
        d_el_off = torch.cumsum(d_n[:M], 0) - d_n[:M]
        ctx.elements_batch_device(*head, d_ss.data_ptr(), d_sr.data_ptr(), M, None, None, None, d_el_off.data_ptr(), E, d_es.data_ptr(),
                                  d_er.data_ptr(), d_ek.data_ptr(), hip_stream=s.cuda_stream)
    s.synchronize()
    assert (d_kind.cpu().numpy() == eo.ARRAY).all() and d_sr.cpu().tolist() == [r for _, r in sel]
    assert d_n.cpu().tolist() == [len(w[2]) for w in want] + [P64] * SPARE and d_st.cpu().tolist() == [0] * M + [P8] * SPARE
    assert d_end.cpu().tolist() == [w[1] for w in want] + [P64] * SPARE
    assert d_er.cpu().tolist() == [rec for w in want for rec, _ in w[2]] + [P64] * SPARE
    assert d_ek.cpu().tolist() == [kd for w in want for _, kd in w[2]] + [P8] * SPARE
    assert d_es.cpu().tolist() == [i for w, (i, _) in zip(want, sel) for _ in w[2]] + [P32] * SPARE


def test_differential_on_generated_lines(ctx):
    rng = np.random.default_rng(20241021)
    streams = []
    for _ in range(60):
        part = []
        for _ in range(int(rng.integers(0, 40))):
            line = eo.gen_line(rng)[0]
            part.append(eo.break_line(rng, line) if rng.integers(0, 6) == 0 else line)
        streams.append(b"\n".join(part))
    b = Batch(streams)
    sel = _openers(b)
    want = _check(ctx, b, sel)
    assert len(sel) > 2000 and set(w[0] for w in want) == {eo.OK, eo.UNCLOSED, eo.MISMATCH}
    assert set(kd for w in want for _, kd in w[2]) >= {eo.SCALAR, eo.OBJECT, eo.ARRAY}
    for (i, r), w in list(zip(sel, want))[:300]:  # the other statement of the rule, on a part
        assert eo.elements_bytes(b.streams[i], r) == w


def test_end_to_end_embeddings_and_tokens(ctx):
    """JSON Lines with "emb" (floats) and "tok" (ints) in shuffled key order, in an arena: index_set_batch, member_batch,
    elements_batch, parse_f64_batch / parse_batch -- equal to json.loads, exactly: repr(float) text is correctly rounded."""
    import torch
    rng = np.random.default_rng(7)
    D, texts, rows = 48, [], []
    for i in range(12):
        part = []
        for r in range(int(rng.integers(1, 30))):
            row = {"id": int(rng.integers(0, 10**9)), "emb": [float(x) for x in rng.standard_normal(D) * 10.0 ** rng.integers(-8, 8, D)],
                   "tok": [int(x) for x in rng.integers(-2**40, 2**40, int(rng.integers(0, 140)))], "note": "emb],[tok"}
            keys = list(row)
            rng.shuffle(keys)
            part.append(json.dumps({k: row[k] for k in keys}, separators=eo.SPACINGS[int(rng.integers(0, 3))]))
            rows.append(row)
        texts.append("\n".join(part).encode("ascii"))
    for text, row in zip(b"\n".join(texts).split(b"\n"), rows):
        assert json.loads(text) == row
    b = Batch(texts).upload()
    out, offs, lens = b.arena, b.d_off, b.d_len
    count, _, pos_off, pos, what = ctx.index_set_batch(out, offs, lens, delims=b"{}[]:,\n")
    lines, line_off, ss, sr, kind, flags = ctx.member_batch(out, offs, lens, count, pos_off, pos, what, [b"emb", b"tok"])
    M = len(rows)
    assert int(lines.sum().item()) == M and (kind == MEMBER_ARRAY).all().item() and not flags.any().item()
    n_e, e_off, st, end, es, er, ek = ctx.elements_batch(out, offs, lens, count, pos_off, pos, what, ss[0], sr[0])
    assert (n_e == D).all().item() and (st == ELEMENTS_OK).all().item() and (ek == eo.SCALAR).all().item()
    assert e_off.cpu().tolist() == [D * j for j in range(M)]
    val, vst = ctx.parse_f64_batch(out, offs, lens, count, pos_off, pos, sel_stream=es, sel_rec=er, spaces=True)
    assert (vst == PARSE_OK).all().item()
    emb = val.view(M, D).cpu().numpy()
    assert (emb == np.array([row["emb"] for row in rows], dtype=np.float64)).all()
    n_t, t_off, st, end, ts, tr, tk = ctx.elements_batch(out, offs, lens, count, pos_off, pos, what, ss[1], sr[1])
    assert n_t.cpu().tolist() == [len(row["tok"]) for row in rows] and (st == ELEMENTS_OK).all().item()
    tok, tst = ctx.parse_batch(out, offs, lens, count, pos_off, pos, sel_stream=ts, sel_rec=tr, spaces=True)
    torch.cuda.synchronize()
    assert (tst == PARSE_OK).all().item() and tok.cpu().tolist() == [x for row in rows for x in row["tok"]]
    assert (what.cpu().numpy()[(pos_off[ss[0].long()] + end).cpu().numpy()] == 0x5D).all()  # `end` is the closing bracket
