"""brx_member_batch (include/brx.h, brx_member.hip): the named members of the JSON Lines objects of a batch as selections for the record
calls.  Every expected value comes from tests/member_oracle.py (its two statements are held to each other, to the contract's check
values and to json.loads by tests/test_member_abi.py): the boundary-serial statement over the very pos / what / count / n_pos that
the call gets, so that cut and garbage tables have an expectation too.  Every output is pre-filled with poison and carries a canary
region behind n_names * m (behind m, behind n) that must be unchanged.  In-process, one context."""
import json
import os
import re

import numpy as np
import pytest

import brx_knobs
import member_oracle as mo
from brotli_rs_amd.brx import MEMBER_MISSING, MEMBER_SCALAR, PARSE_EMPTY, PARSE_OK, TEXT_BARE, TEXT_OK  # noqa: F401  (without the call nothing here runs)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_H = open(os.path.join(ROOT, "brotli-rs_amd", "csrc", "brx_member.h")).read()
T = int(re.search(r"#define\s+BRX_MB_TILE\s+(\d+)u", _H).group(1))  # boundaries per tile
R = int(re.search(r"#define\s+BRX_MB_ROW\s+(\d+)u", _H).group(1))   # boundaries per wave step
P64, P32, P8 = 0x5151515151515151, 0x51515151, 0x51
SPARE = 16
NONE = -1  # UINT64_MAX as the int64 that torch shows
K32 = mo.KEYS[7]


@pytest.fixture(scope="module")
def ctx():
    c = brx_knobs.context(0)
    yield c
    c.close()


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a))
    return (t.to(dtype) if dtype is not None else t).to("cuda:0")


class Batch:
    """Streams in an arena (stream p at phase (3 + p) % 16-ish, colons and quotes between them) with the tables of an index at
    {}[]:,\\n computed on the CPU -- or whatever the test puts in their place."""

    def __init__(self, streams, index=mo.index_set):
        self.streams = [bytes(s) for s in streams]
        self.n = len(self.streams)
        parts, offs, at = [b':"{'], [], 3
        for p, s in enumerate(self.streams):
            offs.append(at)
            gap = b'":{,\n'[:1 + p % 5]
            parts += [s, gap]
            at += len(s) + len(gap)
        self.host = np.frombuffer(b"".join(parts), dtype=np.uint8)
        self.offs, self.lens = np.array(offs, dtype=np.int64), np.array([len(s) for s in self.streams], dtype=np.int64)
        per = [index(s) for s in self.streams]
        self.count = np.array([len(p[0]) for p in per], dtype=np.int64)
        self.pos_off = np.cumsum(self.count) - self.count
        self.pos = np.array([x for p in per for x in p[0]], dtype=np.int64)
        self.what = np.frombuffer(b"".join(p[1] for p in per), dtype=np.uint8).copy()
        self.n_pos = len(self.pos)

    def upload(self):
        self.arena = _dev(self.host)
        self.d_off, self.d_len = _dev(self.offs), _dev(self.lens)
        self.d_count, self.d_pos_off = _dev(self.count), _dev(self.pos_off)
        self.d_pos = _dev(np.concatenate([self.pos, np.full(SPARE, 1 << 40, dtype=np.int64)]))  # (behind n_pos: never loaded)
        self.d_what = _dev(np.concatenate([self.what, np.full(SPARE, 0x3A, dtype=np.uint8)]))
        return self

    def head(self):
        return (self.arena.data_ptr(), self.d_off.data_ptr(), self.d_len.data_ptr(), self.n, int(self.arena.numel()),
                self.d_count.data_ptr(), self.d_pos_off.data_ptr(), self.d_pos.data_ptr(), self.d_what.data_ptr(), self.n_pos)

    def want(self, names):
        """the oracle's boundary-serial statement over these very tables"""
        per = []
        for i, s in enumerate(self.streams):
            a = int(self.pos_off[i])
            c = min(int(self.count[i]), max(0, self.n_pos - a))  # (the boundaries behind n_pos are neutral: nothing to walk)
            per.append(mo.members_boundaries(s, [int(x) for x in self.pos[a:a + c]], bytes(self.what[a:a + c]), names, count=c,
                                             n_pos=max(0, self.n_pos - a)))
        lines = np.array([p[0] for p in per], dtype=np.int64)
        line_off = np.cumsum(lines) - lines
        M, Q = int(lines.sum()), len(names)
        ss, sr = np.zeros((Q, M), dtype=np.int64), np.full((Q, M), NONE, dtype=np.int64)
        kind, flags = np.zeros((Q, M), dtype=np.int64), np.zeros(M, dtype=np.int64)
        for i, (_, found, fl) in enumerate(per):
            for r, (cur, f) in enumerate(zip(found, fl)):
                j = int(line_off[i]) + r
                ss[:, j], flags[j] = i, f
                for q, (kd, rec) in cur.items():
                    kind[q, j], sr[q, j] = kd, rec
        return lines, line_off, ss, sr, kind, flags


def _check(ctx, b, names, m=None, with_lines=True, with_flags=True, hip_stream=None, sync=None):
    """Count mode and fill mode against the oracle.  -> what the oracle says"""
    import torch
    if not hasattr(b, "arena"):
        b.upload()
    lines, line_off, ss, sr, kind, flags = want = b.want(names)
    Q, M, n = len(names), int(lines.sum()), b.n
    m = M if m is None else m
    d_lines = torch.full((n + SPARE,), P64, dtype=torch.int64, device="cuda:0")
    d_line_off = _dev(line_off)
    d_ss = torch.full((Q * m + SPARE,), P32, dtype=torch.int32, device="cuda:0")
    d_sr = torch.full((Q * m + SPARE,), P64, dtype=torch.int64, device="cuda:0")
    d_kind = torch.full((Q * m + SPARE,), P8, dtype=torch.uint8, device="cuda:0")
    d_flags = torch.full((m + SPARE,), P8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.member_batch_device(*b.head(), names, d_lines.data_ptr(), hip_stream=hip_stream)
    if sync:
        sync()
    got = d_lines.cpu().numpy()
    assert (got[:n] == lines).all(), (got[:n].tolist()[:20], lines.tolist()[:20])
    assert (got[n:] == P64).all()
    d_lines.fill_(P64)
    torch.cuda.synchronize()
    ctx.member_batch_device(*b.head(), names, d_lines.data_ptr() if with_lines else None, d_line_off.data_ptr(), m, d_ss.data_ptr(),
                            d_sr.data_ptr(), d_kind.data_ptr(), d_flags.data_ptr() if with_flags else None, hip_stream=hip_stream)
    if sync:
        sync()
    got = d_lines.cpu().numpy()
    assert (got[:n] == (lines if with_lines else P64)).all() and (got[n:] == P64).all()
    g_ss, g_sr, g_kind, g_flags = d_ss.cpu().numpy(), d_sr.cpu().numpy(), d_kind.cpu().numpy(), d_flags.cpu().numpy()
    mm = min(m, M)
    for q in range(Q):
        lo = q * m
        bad = np.flatnonzero((g_sr[lo:lo + mm] != sr[q, :mm]) | (g_kind[lo:lo + mm] != kind[q, :mm]) | (g_ss[lo:lo + mm] != ss[q, :mm]))
        assert bad.size == 0, (names[q], bad[:5].tolist(), g_sr[lo + bad[:5]].tolist(), sr[q, bad[:5]].tolist(), g_kind[lo + bad[:5]].tolist(),
                               kind[q, bad[:5]].tolist())
    assert (g_ss[Q * m:] == P32).all() and (g_sr[Q * m:] == P64).all() and (g_kind[Q * m:] == P8).all()  # the canaries
    if with_flags:
        assert (g_flags[:mm] == flags[:mm]).all(), (g_flags[:mm].tolist()[:20], flags[:mm].tolist()[:20])
        assert (g_flags[m:] == P8).all()
    else:
        assert (g_flags == P8).all()
    return want


def _with_boundaries(c, rng, per_line=3):
    """a stream of exactly c boundaries: lines {"k":v,...} and commas for the rest"""
    keys = [b"id", b"text", b"x", K32, b"textual"]
    s, have = b"", 0
    while have < c:
        left = c - have
        if left < 4:
            s, have = s + b",", have + 1
            continue
        mem = min((left - 2) // 2, 1 + int(rng.integers(0, per_line)))
        s += b"{" + b",".join(b'"%s":%d' % (keys[int(rng.integers(0, 5))], int(rng.integers(0, 1000))) for _ in range(mem)) + b"}\n"
        have += 2 * mem + 2
    assert len(mo.index_set(s)[0]) == c
    return s


def test_the_tile_is_the_headers():
    assert T % R == 0 and R == 64 * 16 and T >= R
    assert (MEMBER_MISSING, MEMBER_SCALAR) == (mo.MISSING, mo.SCALAR)


def test_check_values_of_the_contract(ctx):
    for stream, names, want in mo.CHECK:
        lines, _, ss, sr, kind, flags = _check(ctx, Batch([stream]), names)
        assert lines.tolist() == [len(want)]
        for r, (cur, f) in enumerate(want):
            assert flags[r] == f
            for q, nm in enumerate(names):
                assert (kind[q, r], sr[q, r]) == (cur[nm] if nm in cur else (mo.MISSING, NONE)), (stream, nm)
    # all of them as one batch, under all of their names that fit
    _check(ctx, Batch([c[0] for c in mo.CHECK]), [b"a", b"b", b"c", b"open", b"text", b"user", K32, b"ab"])


def test_boundary_counts_around_rows_and_tiles(ctx):
    rng = np.random.default_rng(1)
    counts = [0, 1, R - 1, R, R + 1, T - 1, T, T + 1, 2 * T + 3]
    for per_line in (3, 200, 1 << 20):  # short lines; lines across rows; one line across all tiles
        streams = [_with_boundaries(c, rng, per_line) for c in counts]
        b = Batch(streams)
        assert b.count.tolist() == counts
        _check(ctx, b, [b"id", b"text", K32])
    _check(ctx, Batch([streams[-1]]), [b"text"])  # n = 1, three tiles


def test_forty_streams_at_every_alignment(ctx):
    rng = np.random.default_rng(2)
    b = Batch([_with_boundaries(c, rng, 4) for c in range(40)])
    assert b.count.tolist() == list(range(40))  # `what` segments start at every alignment mod 16
    assert set(int(x) % 16 for x in b.pos_off) == set(range(16))
    _check(ctx, b, [b"id", b"text", b"x", K32, b"textual", b"te", b"i", b"idx"])


def test_more_streams_and_tiles_than_a_workgroup_has_threads(ctx):
    """3000 small streams, one of them of several tiles in their middle: every thread of the plan and of the compose kernel owns a
    slice of several streams / tiles, and slices cross streams."""
    rng = np.random.default_rng(7)
    counts = [int(x) for x in rng.integers(0, 24, 3000)]
    counts[1500] = 3 * T + 5
    counts[2999] = T + 1
    b = Batch([_with_boundaries(c, rng, 3 if k != 1500 else 1 << 20) for k, c in enumerate(counts)])
    assert b.n > 2048 and int(((b.count + T - 1) // T).sum()) > 2048
    lines, line_off, ss, sr, kind, flags = _check(ctx, b, [b"id", b"text"])
    assert lines[1500] == 2 and kind[:, int(line_off[1500])].any()


def test_members_at_the_edges_of_tiles(ctx):
    commas = lambda c: b"," * c
    streams = [
        commas(T - 2) + b'{"a":1,"b":2}',                       # ':' the last boundary of a tile, its value's ',' the first of the next
        commas(T - 1) + b'{"a":1,"b":2}\n',                     # ':' the first boundary of a tile, its key record across the edge
        b'{"a":1,' + b'"x":0,' * (T // 2 + 10) + b'"a":2}',     # a duplicate name, its two members in different tiles
        b'{"b":7,' + b'"x":[1,2],' * (T // 2) + b'"a":{"b":1}}\n{"b":8}',  # one line that spans three tiles
        commas(T - 3) + b'{"a":1\n{"a":2}\n',                   # an unbalanced line at a tile's end, followed by a good line
        b'{"a":1}\n' * (T // 4) + b'{"a":[{"a":1}],"b":2}',     # line feeds up to a tile's last boundary
    ]
    b = Batch(streams)
    assert int(b.count[3]) > 2 * T and b.what[int(b.pos_off[0]) + T - 1] == 0x3A and b.what[int(b.pos_off[1]) + T] == 0x3A
    lines, line_off, ss, sr, kind, flags = _check(ctx, b, [b"a", b"b"])
    assert (kind[0, 0], sr[0, 0], kind[1, 0]) == (mo.SCALAR, T, mo.SCALAR)
    assert (kind[0, int(line_off[2])], sr[0, int(line_off[2])]) == (mo.SCALAR, int(b.count[2]) - 1)  # the last "a" wins
    j = int(line_off[3])
    assert (kind[0, j], kind[1, j], sr[1, j], flags[j], kind[1, j + 1]) == (mo.OBJECT, mo.SCALAR, 2, 0, mo.SCALAR)
    j = int(line_off[4])
    assert (kind[0, j], flags[j], kind[0, j + 1], flags[j + 1], flags[j + 2]) == (mo.BAD, mo.UNBALANCED, mo.SCALAR, 0, 0)


def test_depth(ctx):
    streams = [b'{"user":{"text":1},"text":2}\n{"user":{"text":1}}\n{"l":[{"text":1},{"text":2}]}\n{"l":[{"text":1}],"text":[3]}',
               b'}{"text":1}\n{"text":1}}\n]\n[', b'[{"text":1},{"text":2}]\n["text",1]', b'"text":1', b"no boundary at all",
               b'{"text":\n"text":2}\n{"text"}\n{:1}\n{"text":}\n{"text"::}']
    lines, line_off, ss, sr, kind, flags = _check(ctx, Batch(streams), [b"text", b"user", b"l"])
    assert kind[0, :4].tolist() == [mo.SCALAR, mo.MISSING, mo.MISSING, mo.ARRAY] and kind[1, :2].tolist() == [mo.OBJECT, mo.OBJECT]
    j = int(line_off[1])
    assert flags[j:j + 4].tolist() == [mo.UNBALANCED] * 4 and kind[0, j:j + 4].tolist() == [mo.MISSING, mo.SCALAR, mo.MISSING, mo.MISSING]
    j = int(line_off[2])
    assert kind[:, j:j + 2].tolist() == [[0, 0]] * 3 and flags[j:j + 2].tolist() == [0, 0]  # a line that is an array
    assert lines[3:5].tolist() == [1, 1] and kind[:, int(line_off[3])].tolist() == [0, 0, 0]
    assert kind[0, int(line_off[5]):].tolist() == [mo.BAD, mo.MISSING, mo.MISSING, mo.MISSING, mo.SCALAR, mo.BAD]


def test_line_ends(ctx):
    _check(ctx, Batch([b'{"a":1}\n{"a":2}\n', b'{"a":1}\n{"a":2}', b"", b"\n", b"\n\n\n", b'{"a":1}']), [b"a"])
    for s in (b"", b"\n", b'{"a":1}', b'{"a":1}\n'):
        lines, _, _, _, kind, _ = _check(ctx, Batch([s]), [b"a", b"b"])  # n = 1
        assert lines.tolist() == [s.count(b"\n") + 1]


def test_names_and_keys(ctx):
    n17 = b"seventeen_bytes_x"
    names = [b"k", b"fifteen_bytes_x", b"sixteen_bytes_xx", n17, K32, b"text", b"tex", b"textual"]
    assert [len(x) for x in names[:5]] == [1, 15, 16, 17, 32]
    line = b"{" + b",".join(b'"%s":%d' % (nm, q) for q, nm in enumerate(names)) + b"}"
    streams = [line, b'{"te":1,"texts":2,"Text":3,"text ":4," text":5,"":6,"t":7}',     # prefixes and their reverse: none is a name
               b'{ "text" :1,\t"tex"\r:2,\r "k": 3}', b'{"te\\u0078t":1,"k":2}\n{"k\\\\":1}\n{"text":"\\\\"}',
               b"{" + b" " * 30 + b'"' + K32 + b'":1}\n{' + b" " * 31 + b'"' + K32 + b'":1,"k":2}',  # key records of 64 and 65 bytes
               b'{"' + K32 + b'x":1,"' + K32[:31] + b'":2}', b'{text:1,"text:2,\'text\':3}']
    b = Batch(streams)
    lines, line_off, ss, sr, kind, flags = _check(ctx, b, names)
    assert kind[:, 0].tolist() == [mo.SCALAR] * 8 and not kind[:, 1].any() and flags[:2].tolist() == [0, 0]
    assert kind[:, int(line_off[2])].tolist() == [1, 0, 0, 0, 0, 1, 1, 0]
    j = int(line_off[3])
    assert flags[j:j + 3].tolist() == [mo.ESCAPED_KEY, mo.ESCAPED_KEY, 0] and kind[5, j:j + 3].tolist() == [0, 0, 1]
    j = int(line_off[4])
    assert (kind[4, j], flags[j], kind[4, j + 1], kind[0, j + 1], flags[j + 1]) == (mo.SCALAR, 0, mo.MISSING, mo.SCALAR, mo.LONG_KEY)
    assert not kind[:, int(line_off[5]):].any()
    _check(ctx, b, [b"text"])            # 1 name
    _check(ctx, b, names[::-1])          # 8 names in another order
    _check(ctx, b, [K32, b"k"], with_lines=False, with_flags=False)
    _check(ctx, b, [K32, b"k"], with_lines=False)   # fill mode without lines, with line_flags
    _check(ctx, b, [K32, b"k"], with_flags=False)   # ... and the reverse


def test_bounds(ctx):
    rng = np.random.default_rng(3)
    streams = [mo.gen_stream(rng, int(rng.integers(0, 40))) for _ in range(24)] + [_with_boundaries(T + 7, rng, 5)]
    names = [b"id", b"text", b"user"]
    b = Batch(streams)
    M = int(b.want(names)[0].sum())
    for m in (M - 1, M // 2, 1, 0):      # m below the number of lines: nothing behind n_names * m is touched
        _check(ctx, b, names, m=m)
        _check(ctx, b, names, m=m, with_lines=False, with_flags=False)
    for cut in (1, 17, b.n_pos // 3, b.n_pos - 1, b.n_pos):  # n_pos below sum(count): the boundaries behind it are neutral
        c = Batch(streams)
        c.n_pos = b.n_pos - cut
        c.pos, c.what = c.pos[:c.n_pos], c.what[:c.n_pos]   # (upload() puts colons and huge positions behind n_pos)
        _check(ctx, c, names)
    g = Batch(streams)                   # garbage in pos: decreasing, beyond len
    g.pos = g.pos[::-1].copy()
    g.pos[::3] += 1 << 33
    _check(ctx, g, names)
    w = Batch(streams)                   # bytes in what that are not in the set
    w.what[::5] = rng.integers(0, 256, len(w.what[::5])).astype(np.uint8)
    w.what[1::7] = 0
    _check(ctx, w, names)
    k = Batch(streams)                   # counts that reach beyond n_pos and into the neighbours
    k.count = k.count + rng.integers(0, 50, k.n)
    k.count[-1] += 1 << 40
    _check(ctx, k, names)


def test_on_a_stream_behind_the_index_pass(ctx):
    """index_set_batch (count, fill) and member_batch (count, fill) enqueued on one caller's stream, nothing in between: the totals
    come from the CPU."""
    import torch
    rng = np.random.default_rng(4)
    b = Batch([mo.gen_stream(rng, int(rng.integers(0, 120))) for _ in range(48)]).upload()
    names = [b"id", b"text", b"tags", b"geo"]
    lines, line_off, ss, sr, kind, flags = b.want(names)
    M, Q, n, total = int(lines.sum()), 4, b.n, b.n_pos
    count = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    pos = torch.full((total + SPARE,), -7, dtype=torch.int64, device="cuda:0")
    what = torch.full((total + SPARE,), 0x3A, dtype=torch.uint8, device="cuda:0")
    d_lines = torch.full((n,), P64, dtype=torch.int64, device="cuda:0")
    d_ss = torch.full((Q * M + SPARE,), P32, dtype=torch.int32, device="cuda:0")
    d_sr = torch.full((Q * M + SPARE,), P64, dtype=torch.int64, device="cuda:0")
    d_kind = torch.full((Q * M + SPARE,), P8, dtype=torch.uint8, device="cuda:0")
    d_flags = torch.full((M + SPARE,), P8, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        args = (mo.SET, 0x22, 0x5C, 0, b.arena.data_ptr(), b.d_off.data_ptr(), b.d_len.data_ptr(), n, int(b.arena.numel()))
        ctx.index_set_batch_device(*args, count.data_ptr(), None, hip_stream=s.cuda_stream)
        pos_off = torch.cumsum(count, 0) - count
        ctx.index_set_batch_device(*args, None, None, pos_off.data_ptr(), pos.data_ptr(), what.data_ptr(), total, hip_stream=s.cuda_stream)
        head = args[4:] + (count.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), what.data_ptr(), total)
        ctx.member_batch_device(*head, names, d_lines.data_ptr(), hip_stream=s.cuda_stream)
        d_line_off = torch.cumsum(d_lines, 0) - d_lines
        ctx.member_batch_device(*head, names, None, d_line_off.data_ptr(), M, d_ss.data_ptr(), d_sr.data_ptr(), d_kind.data_ptr(),
                                d_flags.data_ptr(), hip_stream=s.cuda_stream)
    s.synchronize()
    assert (what.cpu().numpy()[:total] == b.what).all() and (d_lines.cpu().numpy() == lines).all()
    assert (d_sr.cpu().numpy()[:Q * M].reshape(Q, M) == sr).all() and (d_kind.cpu().numpy()[:Q * M].reshape(Q, M) == kind).all()
    assert (d_ss.cpu().numpy()[:Q * M].reshape(Q, M) == ss).all() and (d_flags.cpu().numpy()[:M] == flags).all()
    assert (d_sr.cpu().numpy()[Q * M:] == P64).all() and (d_flags.cpu().numpy()[M:] == P8).all()


def test_differential_on_random_streams(ctx):
    rng = np.random.default_rng(20240521)
    streams = [mo.gen_stream(rng, int(rng.integers(0, 201))) for _ in range(300)]
    b = Batch(streams)
    names = [b"id", b"text", b"user", b"tags", K32, b"k", b"score", b"geo"]
    lines, _, _, _, kind, flags = _check(ctx, b, names)
    assert int(lines.sum()) > 20000 and set(np.unique(kind)) == {0, 1, 2, 3, 4} and set(np.unique(flags)) >= {0, 1, 2, 4}
    two = mo.batch(streams[:40], names, form="bytes")  # the other statement of the rule, on a part
    M = int(two[0].sum())
    assert (two[4] == kind[:, :M]).all() and (two[5] == flags[:M]).all()
    _check(ctx, b, [b"text", b"id"])


def test_end_to_end_through_the_decoder(ctx):
    """JSON Lines with mixed key order and optional keys: compressed on the device, decoded, indexed, its members found, "id" parsed
    and "text" unescaped -- equal to json.loads line by line; MISSING gives EMPTY and an empty text."""
    import torch
    from brotli_rs_amd import shard
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(6)
    texts, rows = [], []
    for i in range(24):
        part = []
        for r in range(int(rng.integers(1, 60))):
            row = {}
            if rng.integers(0, 4):
                row["id"] = int(rng.integers(-10**12, 10**12))
            if rng.integers(0, 4):
                row["text"] = "".join(["a", "é", "\n", '"', "\\", ",", ":", "{", "}", " ", "😀", "x"][int(x)] for x in rng.integers(0, 12, int(rng.integers(0, 40))))
            row["user"] = {"id": -1, "text": "nested"}
            row["tags"] = [1, {"text": "in an array"}]
            keys = list(row)
            rng.shuffle(keys)
            part.append(json.dumps({k: row[k] for k in keys}, separators=[(",", ":"), (", ", ": "), (" ,", " : ")][int(rng.integers(0, 3))]))
            rows.append(row)
        texts.append(("\n".join(part) + "\n").encode("ascii"))
        rows.append(None)  # the trailing line
    n = len(texts)
    src_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=src_off[1:])
    slots = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([ctx.generate_slot_bytes(len(t)) for t in texts], out=slots[1:])
    out_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(t) + 64 + 7 * (k % 5) for k, t in enumerate(texts)], out=out_off[1:])
    src = _dev(np.frombuffer(b"".join(texts), dtype=np.uint8))
    d_src_off, d_slots, d_out_off = _dev(src_off), _dev(slots), _dev(out_off)
    comp = torch.zeros(int(slots[-1]), dtype=torch.uint8, device=dev)
    comp_len = torch.zeros(n, dtype=torch.int64, device=dev)
    gst = torch.full((n,), -1, dtype=torch.int32, device=dev)
    out = torch.full((int(out_off[-1]),), 0x3A, dtype=torch.uint8, device=dev)
    out_len = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.generate_batch_device(src.data_ptr(), d_src_off.data_ptr(), n, comp.data_ptr(), d_slots.data_ptr(), comp_len.data_ptr(), gst.data_ptr())
    ctx.synchronize()
    blob, in_off = shard.compact(comp, d_slots, comp_len)
    torch.cuda.synchronize()
    ctx.decode_batch_device(blob.data_ptr(), in_off.data_ptr(), n, out.data_ptr(), d_out_off.data_ptr(), out_len.data_ptr(), status.data_ptr())
    ctx.synchronize()
    assert status.cpu().tolist() == [0] * n and out_len.cpu().tolist() == [len(t) for t in texts]
    offs = d_out_off[:n].contiguous()
    count, _, pos_off, pos, what = ctx.index_set_batch(out, offs, out_len, delims=mo.SET)
    lines, line_off, ss, sr, kind, flags = ctx.member_batch(out, offs, out_len, count, pos_off, pos, what, [b"id", b"text", b"user", b"tags"])
    M = int(lines.sum().item())
    assert M == len(rows) and tuple(ss.shape) == (4, M) and not flags.any().item()
    val, st = ctx.parse_batch(out, offs, out_len, count, pos_off, pos, sel_stream=ss[0], sel_rec=sr[0], spaces=True)
    dst, dst_off, text_len, tst = ctx.unescape_batch(out, offs, out_len, count, pos_off, pos, sel_stream=ss[1], sel_rec=sr[1], dialect="json",
                                                     spaces=True)
    torch.cuda.synchronize()
    kind, val, st, dst, dst_off, text_len, tst = (x.cpu().numpy() for x in (kind, val, st, dst, dst_off, text_len, tst))
    for j, row in enumerate(rows):
        has_id, has_text = row is not None and "id" in row, row is not None and "text" in row
        assert kind[:, j].tolist() == ([mo.SCALAR if has_id else 0, mo.SCALAR if has_text else 0, mo.OBJECT, mo.ARRAY] if row is not None else [0] * 4), j
        assert (st[j], val[j]) == ((PARSE_OK, row["id"]) if has_id else (PARSE_EMPTY, 0)), j
        text = bytes(dst[dst_off[j]:dst_off[j] + text_len[j]])
        assert (text, tst[j]) == ((row["text"].encode("utf-8"), TEXT_OK) if has_text else (b"", TEXT_BARE)), j
