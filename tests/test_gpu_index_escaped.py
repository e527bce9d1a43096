"""brx_index_escaped_batch (include/brx.h, brx_index_escaped.hip): the record delimiters of the decoded streams of a batch under a
dialect with an escape byte, counted and located on the device.  Every expected value comes from escaped_oracle.vec (numpy on the
CPU, held to the serial rule by tests/test_index_escaped_abi.py).  In every arena the slack of the slots and the gaps between them
hold escape, quote and delimiter bytes repeating: a kernel that reads one byte too far, or lets a byte in front of a stream or behind
it into its state, gets another result.  In-process, one context."""
import json
import os

import numpy as np
import pytest

import brx_knobs
import escaped_oracle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))
TILE = 65536  # one work item of the pass (brx_tiles.h); the tests below only choose lengths and addresses around it
SENTINEL = -0x0123456789ABCDEF
TRIPLES = ((0x0A, 0x22, 0x5C), (0x00, 0xFF, 0x80), (0xFF, 0x7F, 0x00))  # (delim, quote, escape)
NL, QT, BS = 0x0A, 0x22, 0x5C
NO_QUOTE = 1  # BRX_INDEX_NO_QUOTE


@pytest.fixture(scope="module")
def ctx():
    c = brx_knobs.context(0)
    yield c
    c.close()


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a))  # (a writable copy)
    return (t.to(dtype) if dtype is not None else t).to("cuda:0")


def _reference(host, offs, lens, D, Q, E, no_quote=False):
    """-> (counts, open, exclusive prefix sum, all positions back to back)"""
    per = [escaped_oracle.vec(host[o:o + ln], D, Q, E, no_quote) for o, ln in zip(offs, lens)]
    counts = np.array([p.size for p, _ in per], dtype=np.int64)
    opens = np.array([o for _, o in per], dtype=np.int32)
    pos_off = np.zeros(len(per), dtype=np.int64)
    np.cumsum(counts[:-1], out=pos_off[1:])
    return counts, opens, pos_off, (np.concatenate([p for p, _ in per]) if per else np.zeros(0, dtype=np.int64))


def _filler(size, D, Q, E):
    """escape, quote and delimiter bytes repeating"""
    return np.array([E, Q, D], dtype=np.uint8)[np.arange(size) % 3]


def _check(ctx, host, arena, offs, lens, D, Q, E, no_quote=False):
    """Count mode, then fill mode (pos_off by torch.cumsum from the device's counts; count and open written again), both on raw
    pointers, against the oracle.  -> (counts, open, positions) of the oracle."""
    import torch
    offs, lens = np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    n = len(lens)
    want_count, want_open, _, want_pos = _reference(host, offs, lens, D, Q, E, no_quote)
    tag = (hex(D), hex(Q), hex(E), no_quote)
    d_off, d_len = _dev(offs), _dev(lens)
    count = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    open_ = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    args = (D, Q, E, NO_QUOTE if no_quote else 0, arena.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, arena.numel())
    ctx.index_escaped_batch_device(*args, count.data_ptr(), open_.data_ptr())
    got = count.cpu().numpy()
    bad = np.nonzero(got != want_count)[0]
    assert bad.size == 0, ("count", tag, [(int(offs[i]), int(lens[i]), int(got[i]), int(want_count[i])) for i in bad[:8]])
    got = open_.cpu().numpy()
    bad = np.nonzero(got != want_open)[0]
    assert bad.size == 0, ("open", tag, [(int(offs[i]), int(lens[i]), int(got[i]), int(want_open[i])) for i in bad[:8]])
    pos_off = torch.cumsum(count, 0) - count
    total = int(want_count.sum())
    pos = torch.full((total + 8,), SENTINEL, dtype=torch.int64, device="cuda:0")
    count2 = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    open2 = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.index_escaped_batch_device(*args, count2.data_ptr(), open2.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), total)
    assert (count2.cpu().numpy() == want_count).all(), ("count written by fill mode", tag)
    assert (open2.cpu().numpy() == want_open).all(), ("open written by fill mode", tag)
    got_pos = pos.cpu().numpy()
    assert (got_pos[total:] == SENTINEL).all(), tag
    bad = np.nonzero(got_pos[:total] != want_pos)[0]
    assert bad.size == 0, ("pos", tag, bad[:8].tolist(), got_pos[bad[:8]].tolist(), want_pos[bad[:8]].tolist())
    return want_count, want_open, want_pos


def _arena_tile_aligned(n_bytes):
    """A device arena and the offset in it of a 64 KiB aligned ADDRESS (tiles are cut in the address range)."""
    import torch
    arena = torch.empty(n_bytes + TILE, dtype=torch.uint8, device="cuda:0")
    return arena, (-arena.data_ptr()) % TILE


def test_check_values(ctx):
    """The contract's 33-byte text -- an escaped quote and a line feed inside a string, an escaped line feed outside, an escaped
    escape in front of a closing quote, an escaped comma, an unterminated string that ends on an escape -- at offset 1000 of a 4 KiB
    arena, by record delimiter, by field separator and without quotes; empty streams at offset 0, at 1000 and at the arena's end."""
    raw = b'a,"x\\"y\ny",b\\\nc\n"q\\\\"\nz\\,w\n"open\\'
    assert len(raw) == 33
    text = np.frombuffer(raw, dtype=np.uint8)
    offs, lens = [1000, 1000, 0, 4096], [len(text), 0, 0, 0]
    d_off, d_len = _dev(np.array(offs, dtype=np.int64)), _dev(np.array(lens, dtype=np.int64))
    for delim, no_quote, want_pos, want_open in ((NL, False, [15, 21, 26], 3), (ord(","), False, [1, 10], 3), (NL, True, [7, 15, 21, 26], 2)):
        got = escaped_oracle.vec(text, delim, QT, BS, no_quote)
        assert got[0].tolist() == want_pos and got[1] == want_open
        host = _filler(4096, delim, QT, BS)
        host[1000:1000 + len(text)] = text
        arena = _dev(host)
        k = len(want_pos)
        count, open_, pos_off, pos = ctx.index_escaped_batch(arena, d_off, d_len, delim=delim, quote=QT, escape=BS, no_quote=no_quote)
        assert count.cpu().tolist() == [k, 0, 0, 0]
        assert open_.cpu().tolist() == [want_open, 0, 0, 0]
        assert pos_off.cpu().tolist() == [0, k, k, k]
        assert pos.cpu().tolist() == want_pos
        count, open_ = ctx.index_escaped_batch(arena, d_off, d_len, delim=delim, quote=QT, escape=BS, no_quote=no_quote, positions=False)
        assert count.cpu().tolist() == [k, 0, 0, 0] and open_.cpu().tolist() == [want_open, 0, 0, 0]
        _check(ctx, host, arena, offs, lens, delim, QT, BS, no_quote)


EDGE_LENS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 65535, 65536, 65537, 131077)


def _other(D, Q, E):
    return next(b for b in (D ^ 0x80, D ^ 0xFF, 0x41, 0x42) if b not in (D, Q, E))


def _draw(rng, ln, D, Q, E, heavy):
    """ln bytes over {D, Q, E, x}: uniform, or E with probability 4/5"""
    alphabet = np.array([D, Q, E, _other(D, Q, E)], dtype=np.uint8)
    return alphabet[rng.choice(4, ln, p=[1 / 15, 1 / 15, 4 / 5, 1 / 15] if heavy else [1 / 4] * 4)]


@pytest.mark.parametrize("heavy", [False, True])
@pytest.mark.parametrize("D,Q,E", TRIPLES)
def test_chunk_row_and_tile_edges_at_every_alignment(ctx, D, Q, E, heavy):
    """Every length around a chunk, a row and a tile at all 16 phases of out_off in one batch; in a second one a stream that starts 3
    bytes before a 64 KiB address boundary, one that starts 3 bytes behind one and ends on the next, one that starts 3 bytes before one
    and ends on the next.  Alphabet {D, Q, E, x}, uniform and with E at 4 in 5; count mode and fill mode."""
    rng = np.random.default_rng(3000 + D + heavy)
    offs, lens, at = [], [], 0
    for ln in EDGE_LENS:
        for phase in range(16):
            at = (at + 15) // 16 * 16 + phase + 16 * int(rng.integers(0, 5))
            offs.append(at)
            lens.append(ln)
            at += ln + int(rng.integers(0, 40))
    arena, base = _arena_tile_aligned(at + 64)  # (a 64 KiB aligned base: out_off mod 16 is the address mod 16)
    host = _filler(arena.numel(), D, Q, E)
    offs = [base + o for o in offs]
    for o, ln in zip(offs, lens):
        host[o:o + ln] = _draw(rng, ln, D, Q, E, heavy)
    arena.copy_(_dev(host))
    _check(ctx, host, arena, offs, lens, D, Q, E)

    arena, base = _arena_tile_aligned(7 * TILE)
    host = _filler(arena.numel(), D, Q, E)
    offs = [base + TILE - 3, base + 3 * TILE + 3, base + 5 * TILE - 3]
    lens = [70000, TILE - 3, TILE + 3]
    for o, ln in zip(offs, lens):
        host[o:o + ln] = _draw(rng, ln, D, Q, E, heavy)
    arena.copy_(_dev(host))
    _check(ctx, host, arena, offs, lens, D, Q, E)


CARRY_START = 5               # the stream starts 5 bytes behind a 64 KiB address
CARRY_LEN = 3 * TILE - 100    # ... and has 3 tiles
# address of the last byte of the run of escape bytes, from that 64 KiB address
CARRY_END = {"chunk_last": TILE + 3 * 1024 + 16 * 7 + 15, "row_last": TILE + 5 * 1024 + 1023, "tile_last": 2 * TILE - 1,
             "stream_last": CARRY_START + CARRY_LEN - 1}
CARRY_RUNS = (1, 2, 15, 16, 17, 1023, 1024, 1025)


def _carry_arena():
    """-> arena, base, host: one stream of delimiters only, in an arena of filler"""
    arena, base = _arena_tile_aligned(4 * TILE)
    host = _filler(arena.numel(), NL, QT, BS)
    host[base + CARRY_START:base + CARRY_START + CARRY_LEN] = NL
    return arena, base, host


def _carry_case(ctx, first, k, behind):
    """All delimiters, except a run of k escape bytes whose first byte is at address `first` (from the 64 KiB address) and the byte
    `behind` behind it (None: the run ends the stream).  What must come out is asserted on the CPU first: the run's bytes are never
    positions; the byte behind it is escaped, and so missing from pos, iff k is odd; a quote behind an even run opens a field that
    never closes, so nothing behind it is a position; a run that ends the stream leaves open bit 1 = k & 1."""
    arena, base, host = _carry_arena()
    assert (arena.data_ptr() + base) % TILE == 0
    p = first - CARRY_START  # stream offset of the run's first byte
    assert 0 < p and p + k <= CARRY_LEN
    host[base + first:base + first + k] = BS
    want = np.ones(CARRY_LEN, dtype=bool)
    want[p:p + k] = False
    want_open = 0
    if behind is None:
        assert p + k == CARRY_LEN
        want_open = (k & 1) << 1
    else:
        assert p + k < CARRY_LEN
        host[base + first + k] = behind
        if k & 1:
            want[p + k] = False  # escaped: data
        elif behind == QT:
            want[p + k:] = False  # an active quote: everything behind it is inside
            want_open = 1
    arena.copy_(_dev(host))
    counts, opens, pos = _check(ctx, host, arena, [base + CARRY_START], [CARRY_LEN], NL, QT, BS)
    assert opens.tolist() == [want_open] and (pos == np.flatnonzero(want)).all() and counts.tolist() == [int(want.sum())]


@pytest.mark.parametrize("where", sorted(CARRY_END))
def test_a_run_of_escapes_where_the_carry_crosses(ctx, where):
    """One run of k escape bytes that ends on the last byte of a lane's chunk, of a row, of a tile and of the stream, for k around a
    chunk and a row; behind it a delimiter, then a quote."""
    for k in CARRY_RUNS:
        first = CARRY_END[where] - k + 1
        if where == "stream_last":
            _carry_case(ctx, first, k, None)
        else:
            _carry_case(ctx, first, k, NL)
            _carry_case(ctx, first, k, QT)


def test_runs_that_cover_a_whole_tile(ctx):
    """Runs of 65536 + 1 and 65536 + 2 escape bytes that cover the stream's middle tile, a delimiter and a quote behind them; and a
    middle tile made only of escape bytes with a quote as the first byte of the next tile: the run is even, the quote is active."""
    for first, k in ((TILE - 1, TILE + 1), (TILE - 1, TILE + 2), (TILE - 2, TILE + 2), (TILE, TILE)):
        for behind in (NL, QT):
            _carry_case(ctx, first, k, behind)


def test_streams_do_not_leak(ctx):
    """Adjacent streams with no gap: the first ends on an active escape (open bit 1) and the second starts with a delimiter, which
    counts, at pos 0; the first ends inside a quoted field and the second starts outside.  Both again with an empty stream between
    the two, for short streams and for ones of more than a tile."""
    rng = np.random.default_rng(5)
    for la, lb in ((7, 9), (100, 1030), (70001, 66000)):
        for ending in ("escape", "quote"):
            for gap_stream in (False, True):
                a = _draw(rng, la, NL, QT, BS, False)
                b = _draw(rng, lb, NL, QT, BS, False)
                b[0] = NL
                if ending == "escape":
                    a[-2:] = (0x78, BS)  # ... x E: one active escape on the last byte
                else:
                    a[-2:] = (0x78, 0x78)
                    if escaped_oracle.vec(a, NL, QT, BS)[1] & 1 == 0:
                        a[-1] = QT  # (behind x: not escaped)
                want_a = escaped_oracle.vec(a, NL, QT, BS)[1]
                assert (want_a >> 1 == 1) if ending == "escape" else (want_a & 1 == 1)
                host = _filler(333 + la + lb + 64, NL, QT, BS)
                host[333:333 + la] = a
                host[333 + la:333 + la + lb] = b
                offs, lens = [333, 333 + la], [la, lb]
                if gap_stream:
                    offs, lens = [333, 333 + la, 333 + la], [la, 0, lb]
                counts, opens, pos = _check(ctx, host, _dev(host), offs, lens, NL, QT, BS)
                assert opens[0] == want_a and pos[counts[:-1].sum()] == 0  # the second stream's first position is its byte 0


def _big_body(rng, ln, kind):
    if kind == "dense":  # escapes 1 in 4, quotes 1 in 50
        body = np.array([NL, 0x61, 0x0D], dtype=np.uint8)[rng.integers(0, 3, ln)]
        body[rng.integers(0, 50, ln) == 0] = QT
        body[rng.integers(0, 4, ln) == 0] = BS
        return body
    # escapes in long runs: runs and the gaps between them geometric with mean 40; quotes 1 in 5000
    body = np.array([NL, 0x61, 0x0D], dtype=np.uint8)[rng.integers(0, 3, ln)]
    body[rng.integers(0, 5000, ln) == 0] = QT
    edges = np.cumsum(rng.geometric(1 / 40, ln // 30))
    edges = edges[edges < ln]
    is_run = np.zeros(ln + 1, dtype=np.int64)
    np.add.at(is_run, edges, 1)
    body[(np.cumsum(is_run[:-1]) & 1) == 1] = BS
    return body


@pytest.mark.parametrize("kind", ["dense", "runs"])
def test_order_and_state_across_many_tiles(ctx, kind):
    """One stream of 4 MiB + 3 at an odd offset: 65 tiles that finish in any order, positions in order; the escapes dense, and in long
    runs with few quotes, so that tiles are entered in every one of the four states (asserted from the oracle's states at the tile
    edges) and runs of tiles pass a state on."""
    rng = np.random.default_rng(60 + len(kind))
    ln = (4 << 20) + 3
    arena, base = _arena_tile_aligned(ln + 4096)
    host = _filler(arena.numel(), NL, QT, BS)
    host[base + 777:base + 777 + ln] = _big_body(rng, ln, kind)
    arena.copy_(_dev(host))
    st = escaped_oracle.states(host[base + 777:base + 777 + ln], NL, QT, BS)
    edges = np.arange(1, 65) * TILE - 777  # stream offsets of the first bytes of tiles 1 .. 64
    assert edges[-1] < ln and set(st[edges].tolist()) == {0, 1, 2, 3}
    counts, _, _ = _check(ctx, host, arena, [base + 777], [ln], NL, QT, BS)
    assert counts[0] > 1000
    count, open_, pos_off, pos = ctx.index_escaped_batch(arena, _dev(np.array([base + 777], dtype=np.int64)), _dev(np.array([ln], dtype=np.int64)))
    want, want_open = escaped_oracle.vec(host[base + 777:base + 777 + ln], NL, QT, BS)
    assert count.cpu().tolist() == [want.size] and pos_off.cpu().tolist() == [0] and open_.cpu().tolist() == [want_open]
    assert (pos.cpu().numpy() == want).all()


def _small_batch(seed, n, top, D=NL, Q=QT, E=BS):
    """n streams of 0 .. top bytes over {D, Q, E, 'x'} with gaps of 0 .. 20 filler bytes -> host arena, offs, lens.  Empty streams sit
    between streams that end on an active escape and inside a quote."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, top + 1, n).astype(np.int64)
    lens[10::50] = 0
    lens[9::50] = np.maximum(lens[9::50], 2)
    lens[11::50] = np.maximum(lens[11::50], 2)
    gaps = rng.integers(0, 21, n).astype(np.int64)
    offs = np.cumsum(gaps) + np.concatenate(([0], np.cumsum(lens[:-1])))
    host = _filler(int(offs[-1] + lens[-1] + 16), D, Q, E)
    body = np.array([D, Q, E, 0x78], dtype=np.uint8)[rng.integers(0, 4, host.size)]
    for k, (o, ln) in enumerate(zip(offs, lens)):
        host[o:o + ln] = body[o:o + ln]
        if k % 50 in (9, 11):
            host[o + ln - 2:o + ln] = (0x78, E)  # ends on an active escape
    return host, offs, lens


def test_many_small_streams(ctx):
    """9000 streams of 0 .. 40 bytes, one item each -- more items than the 8192 waves of a full grid on 256 CUs take by their index,
    so the rest come from the ticket counter.  Empty streams sit between streams that end escaped: nothing leaks across them."""
    host, offs, lens = _small_batch(79, 9000, 40)
    _, opens, _, _ = _reference(host, offs, lens, NL, QT, BS)
    assert (opens[9::50] >> 1).all() and (opens[11::50] >> 1).all() and not lens[10::50].any() and (opens & 1).sum() > 1000
    _check(ctx, host, _dev(host), offs, lens, NL, QT, BS)


def test_no_quote(ctx):
    """BRX_INDEX_NO_QUOTE with `quote` set to the delimiter's value (ignored, not refused): the oracle with no_quote, and bit 0 of
    open is 0 everywhere.  Quote bytes are in the data and are plain data."""
    host, offs, lens = _small_batch(80, 3000, 300)
    assert (host == QT).sum() > 1000
    _, opens, _ = _check(ctx, host, _dev(host), offs, lens, NL, NL, BS, no_quote=True)
    assert not (opens & 1).any() and (opens >> 1).sum() > 100
    with_q, _, _, _ = _reference(host, offs, lens, NL, QT, BS)
    without, _, _, _ = _reference(host, offs, lens, NL, QT, BS, True)
    assert (with_q != without).sum() > 1000  # (the flag matters on this batch)


def _json_texts(n, top):
    """n JSON-Lines-like texts of 0 .. top bytes: strings with \\", \\\\ and \\n (an escape pair, not a line feed) inside, and raw
    line feeds between rows; every third is cut inside a string or right behind a backslash."""
    rng = np.random.default_rng(12)
    strings = [b'"plain"', b'"say \\"hi\\""', b'"back\\\\"', b'"a\\nb"', b'"x\\\\\\"y"', b'""', b'"tab\\there, comma"', b'"\\\\\\\\"']
    rows = []
    for _ in range(400):
        fields = []
        for j in range(int(rng.integers(1, 7))):
            fields.append(b'"k%d":' % j + (strings[int(rng.integers(0, len(strings)))] if rng.integers(0, 3) else b"%d" % int(rng.integers(0, 999))))
        rows.append(b"{" + b",".join(fields) + b"}\n")
    texts = []
    sizes = np.concatenate(([0, 1, top], rng.integers(0, top + 1, n - 3)))
    for k, size in enumerate(sizes):
        parts, have = [], 0
        while have < size:
            parts.append(rows[int(rng.integers(0, len(rows)))])
            have += len(parts[-1])
        t = b"".join(parts)[:int(size)]
        if k % 3 == 0 and len(t) > 20:
            t = t + (b'{"cut":"in here\n' if k % 6 == 0 else b'{"cut":"x\\\\\\')  # inside a string / right behind an active backslash
        texts.append(t)
    return texts


def test_behind_a_decode_without_a_synchronisation(ctx):
    """64 JSON-Lines-like texts (0 .. 200 KiB) compressed on the device, then on one HIP stream: decode, lens = out_len * (status ==
    0), escaped count mode, torch.cumsum, escaped fill mode with `total` from the CPU's count -- the host needs nothing from the
    device in between."""
    import torch
    from brotli_rs_amd import shard
    dev = torch.device("cuda:0")
    texts = _json_texts(64, 200 << 10)
    n = len(texts)
    refs = [escaped_oracle.vec(np.frombuffer(t, dtype=np.uint8), NL, QT, BS) for t in texts]
    assert sum(1 for _, o in refs if o == 1) >= 5 and sum(1 for _, o in refs if o == 3) >= 5 and sum(1 for _, o in refs if not o) >= 10
    total = int(sum(p.size for p, _ in refs))
    src_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=src_off[1:])
    slots = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([ctx.generate_slot_bytes(len(t)) for t in texts], out=slots[1:])
    caps = [len(t) + 64 + 7 * (k % 5) for k, t in enumerate(texts)]
    out_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(caps, out=out_off[1:])
    src = _dev(np.frombuffer(b"".join(texts), dtype=np.uint8))
    d_src_off, d_slots, d_out_off = _dev(src_off), _dev(slots), _dev(out_off)
    comp = torch.zeros(int(slots[-1]), dtype=torch.uint8, device=dev)
    comp_len = torch.zeros(n, dtype=torch.int64, device=dev)
    gst = torch.full((n,), -1, dtype=torch.int32, device=dev)
    out = _dev(_filler(int(out_off[-1]), NL, QT, BS))
    out_len = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    count = torch.full((n,), -7, dtype=torch.int64, device=dev)
    open_ = torch.full((n,), -7, dtype=torch.int32, device=dev)
    pos = torch.full((total + 8,), SENTINEL, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        ctx.generate_batch_device(src.data_ptr(), d_src_off.data_ptr(), n, comp.data_ptr(), d_slots.data_ptr(), comp_len.data_ptr(),
                                  gst.data_ptr(), hip_stream=s.cuda_stream)
        blob, in_off = shard.compact(comp, d_slots, comp_len)  # (the generator's slots have slack; this reads the compressed total back)
        assert not gst.any().item()
        ctx.decode_batch_device(blob.data_ptr(), in_off.data_ptr(), n, out.data_ptr(), d_out_off.data_ptr(), out_len.data_ptr(),
                                status.data_ptr(), hip_stream=s.cuda_stream)
        lens = out_len * (status == 0)
        args = (NL, QT, BS, 0, out.data_ptr(), d_out_off.data_ptr(), lens.data_ptr(), n, out.numel())
        ctx.index_escaped_batch_device(*args, count.data_ptr(), open_.data_ptr(), hip_stream=s.cuda_stream)
        pos_off = torch.cumsum(count, 0) - count
        ctx.index_escaped_batch_device(*args, None, None, pos_off.data_ptr(), pos.data_ptr(), total, hip_stream=s.cuda_stream)
    s.synchronize()
    assert status.cpu().tolist() == [0] * n
    assert out_len.cpu().tolist() == [len(t) for t in texts]
    assert count.cpu().tolist() == [p.size for p, _ in refs]
    assert open_.cpu().tolist() == [o for _, o in refs]
    got = pos.cpu().numpy()
    assert (got[:total] == np.concatenate([p for p, _ in refs])).all() and (got[total:] == SENTINEL).all()


def test_agreement_with_the_other_passes_on_the_golden_batch(ctx):
    """All of tests/golden/data decoded in one BRX_MEM_DEVICE batch.  A few of the golden outputs (compressed or random data) hold
    every one of the 256 byte values; the escape is a byte value absent from all the other outputs, and the quote another one (the
    test asserts that there are two).  With them the escaped pass equals brx_index_quoted_batch in count, pos and bit 0 of open, and
    bit 1 is 0; with BRX_INDEX_NO_QUOTE it equals brx_index_batch.  The streams that hold every byte value are held to the oracle."""
    import torch
    dev = torch.device("cuda:0")
    streams = [open(os.path.join(GOLDEN, "data", e["stream"]), "rb").read() for e in MANIFEST]
    outs = [np.frombuffer(open(os.path.join(GOLDEN, "data", e["expected"]), "rb").read() if e["status"] == 0 else b"", dtype=np.uint8)
            for e in MANIFEST]
    holds = np.array([np.bincount(o, minlength=256) > 0 for o in outs])
    full = holds.all(axis=1)
    assert full.sum() <= 5
    free = np.flatnonzero(~holds[~full].any(axis=0))
    free = free[free != NL]
    assert free.size > 1
    quote, escape = int(free[0]), int(free[1])
    caps = [e["out_bytes"] + 64 + 7 * (k % 5) if e["status"] == 0 else 1 << 17 for k, e in enumerate(MANIFEST)]
    n = len(streams)
    in_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(s) for s in streams], out=in_off[1:])
    out_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(caps, out=out_off[1:])
    blob = _dev(np.frombuffer(b"".join(streams), dtype=np.uint8))
    d_in_off, d_out_off = _dev(in_off), _dev(out_off)
    out = _dev(_filler(int(out_off[-1]), NL, quote, escape))
    out_len = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.decode_batch_device(blob.data_ptr(), d_in_off.data_ptr(), n, out.data_ptr(), d_out_off.data_ptr(), out_len.data_ptr(),
                            status.data_ptr())
    ctx.synchronize()
    assert status.cpu().tolist() == [e["status"] for e in MANIFEST]
    lens = out_len * (status == 0)
    plain = [t.cpu().numpy() for t in ctx.index_batch(out, d_out_off, lens, delim=NL)]
    quoted = [t.cpu().numpy() for t in ctx.index_quoted_batch(out, d_out_off, lens, delim=NL, quote=quote)]
    got_q = [t.cpu().numpy() for t in ctx.index_escaped_batch(out, d_out_off, lens, delim=NL, quote=quote, escape=escape)]
    got_n = [t.cpu().numpy() for t in ctx.index_escaped_batch(out, d_out_off, lens, delim=NL, quote=NL, escape=escape, no_quote=True)]
    for i in range(n):
        count, open_, pos_off, pos = got_q
        mine = pos[pos_off[i]:pos_off[i] + count[i]]
        ncount, nopen, npos_off, npos = got_n
        mine_n = npos[npos_off[i]:npos_off[i] + ncount[i]]
        if full[i]:
            want, want_open = escaped_oracle.vec(outs[i], NL, quote, escape)
            assert count[i] == want.size and open_[i] == want_open and (mine == want).all(), i
            want, want_open = escaped_oracle.vec(outs[i], NL, quote, escape, True)
            assert ncount[i] == want.size and nopen[i] == want_open and (mine_n == want).all(), i
        else:
            qcount, qopen, qoff, qpos = quoted
            assert count[i] == qcount[i] and open_[i] == qopen[i], i
            assert (mine == qpos[qoff[i]:qoff[i] + qcount[i]]).all(), i
            pcount, poff, ppos = plain
            assert ncount[i] == pcount[i] and nopen[i] == 0, i
            assert (mine_n == ppos[poff[i]:poff[i] + pcount[i]]).all(), i
    assert plain[0].sum() > 10000


def test_total_is_a_bound(ctx):
    """Fill mode with room for half the entries: those are right, and the sentinels behind them are untouched."""
    import torch
    host, offs, lens = _small_batch(6, 300, 3000)
    arena = _dev(host)
    want_count, _, want_off, want_pos = _reference(host, offs, lens, NL, QT, BS)
    half = int(want_pos.size // 2)
    assert half > 1000
    pos = torch.full((want_pos.size + 8,), SENTINEL, dtype=torch.int64, device="cuda:0")
    d_off, d_len, d_pos_off = _dev(offs), _dev(lens), _dev(want_off)
    torch.cuda.synchronize()
    ctx.index_escaped_batch_device(NL, QT, BS, 0, arena.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), len(lens), arena.numel(), None, None,
                                   d_pos_off.data_ptr(), pos.data_ptr(), half)
    got = pos.cpu().numpy()
    assert (got[:half] == want_pos[:half]).all()
    assert (got[half:] == SENTINEL).all()


def test_overlapping_calls_on_two_streams(ctx):
    """20 fill-mode calls alternating between two HIP streams over different small batches -- more than the 16 regions of the scratch
    ring -- and one synchronisation at the end."""
    import torch
    dev = torch.device("cuda:0")
    jobs = []
    for k in range(20):
        host, offs, lens = _small_batch(800 + k, 60 + k, 3000)
        want_count, want_open, want_off, want_pos = _reference(host, offs, lens, NL, QT, BS)
        jobs.append(dict(arena=_dev(host), offs=_dev(offs), lens=_dev(lens), pos_off=_dev(want_off), n=len(lens), total=int(want_pos.size),
                         count=torch.full((len(lens),), -7, dtype=torch.int64, device=dev),
                         open=torch.full((len(lens),), -7, dtype=torch.int32, device=dev),
                         pos=torch.full((want_pos.size + 8,), SENTINEL, dtype=torch.int64, device=dev),
                         want_count=want_count, want_open=want_open, want_pos=want_pos))
    s = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    torch.cuda.synchronize()
    for k, j in enumerate(jobs):
        ctx.index_escaped_batch_device(NL, QT, BS, 0, j["arena"].data_ptr(), j["offs"].data_ptr(), j["lens"].data_ptr(), j["n"],
                                       j["arena"].numel(), j["count"].data_ptr(), j["open"].data_ptr(), j["pos_off"].data_ptr(),
                                       j["pos"].data_ptr(), j["total"], hip_stream=s[k % 2].cuda_stream)
    torch.cuda.synchronize()
    for k, j in enumerate(jobs):
        assert (j["count"].cpu().numpy() == j["want_count"]).all(), k
        assert (j["open"].cpu().numpy() == j["want_open"]).all(), k
        got = j["pos"].cpu().numpy()
        assert (got[:j["total"]] == j["want_pos"]).all() and (got[j["total"]:] == SENTINEL).all(), k


def test_arguments(ctx):
    """The contract's table on a real context: unknown flag bits, delim == escape, quote == delim and quote == escape without
    BRX_INDEX_NO_QUOTE, only one of pos_off / pos, count NULL in count mode, a NULL table -> BRX_ERR_INVALID_ARGUMENT and nothing is
    launched; n = 0 -> BRX_SUCCESS; open NULL in either mode; then a good call on the same context still works."""
    import torch
    dev = torch.device("cuda:0")
    arena = torch.full((64,), NL, dtype=torch.uint8, device=dev)
    arena[20] = QT  # stream 1 = 4 delimiters, a quote, 3 delimiters inside the field it opens
    arena[5] = BS   # stream 0 = 5 delimiters, an escape, an escaped delimiter, a delimiter
    offs = torch.tensor([0, 16], dtype=torch.int64, device=dev)
    lens = torch.full((2,), 8, dtype=torch.int64, device=dev)
    count = torch.zeros(2, dtype=torch.int64, device=dev)
    open_ = torch.full((2,), -7, dtype=torch.int32, device=dev)
    pos_off = torch.tensor([0, 6], dtype=torch.int64, device=dev)
    pos = torch.full((14,), SENTINEL, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    lib, h = ctx._lib, ctx._h
    f = lib.brx_index_escaped_batch
    args = (arena.data_ptr(), offs.data_ptr(), lens.data_ptr())
    c, o = count.data_ptr(), open_.data_ptr()
    assert f(h, NL, QT, BS, 0, *args, 0, 64, c, o, None, None, 0, None) == 0
    assert f(h, NL, QT, BS, 0, None, None, None, 0, 0, c, None, None, None, 0, None) == 0
    assert f(h, NL, QT, BS, 2, *args, 2, 64, c, o, None, None, 0, None) == -1
    assert b"brx_index_escaped_batch" in lib.brx_last_error() and b"flag" in lib.brx_last_error()
    assert f(h, BS, QT, BS, 0, *args, 2, 64, c, o, None, None, 0, None) == -1
    assert b"brx_index_escaped_batch" in lib.brx_last_error() and b"escape" in lib.brx_last_error()
    assert f(h, BS, QT, BS, NO_QUOTE, *args, 2, 64, c, o, None, None, 0, None) == -1 and b"escape" in lib.brx_last_error()
    assert f(h, NL, NL, BS, 0, *args, 2, 64, c, o, None, None, 0, None) == -1 and b"quote" in lib.brx_last_error()
    assert f(h, NL, BS, BS, 0, *args, 2, 64, c, o, None, None, 0, None) == -1
    assert b"quote" in lib.brx_last_error() and b"escape" in lib.brx_last_error()
    assert f(h, NL, QT, BS, 0, *args, 2, 64, c, o, pos_off.data_ptr(), None, 14, None) == -1
    assert b"brx_index_escaped_batch" in lib.brx_last_error()
    assert f(h, NL, QT, BS, 0, *args, 2, 64, c, o, None, pos.data_ptr(), 14, None) == -1
    assert f(h, NL, QT, BS, 0, *args, 2, 64, None, o, None, None, 0, None) == -1
    assert f(h, NL, QT, BS, 0, arena.data_ptr(), None, lens.data_ptr(), 2, 64, c, o, None, None, 0, None) == -1
    assert f(h, NL, QT, BS, 0, arena.data_ptr(), offs.data_ptr(), None, 2, 64, c, o, None, None, 0, None) == -1
    torch.cuda.synchronize()
    assert open_.cpu().tolist() == [-7, -7] and count.cpu().tolist() == [0, 0]  # (nothing was launched)
    assert f(h, NL, QT, BS, 0, *args, 2, 64, c, None, None, None, 0, None) == 0  # open NULL, count mode
    assert count.cpu().tolist() == [6, 4]
    assert f(h, NL, NL, BS, NO_QUOTE, *args, 2, 64, c, o, None, None, 0, None) == 0  # quote == delim is ignored under the flag
    assert count.cpu().tolist() == [6, 7] and open_.cpu().tolist() == [0, 0]  # (the quote byte of stream 1 is data, no delimiter)
    assert f(h, NL, QT, BS, 0, *args, 2, 64, None, None, pos_off.data_ptr(), pos.data_ptr(), 14, None) == 0  # both NULL, fill mode
    assert f(h, NL, QT, BS, 0, *args, 2, 64, c, o, pos_off.data_ptr(), pos.data_ptr(), 14, None) == 0  # (the context still works)
    assert count.cpu().tolist() == [6, 4] and open_.cpu().tolist() == [0, 1]
    assert pos.cpu().tolist() == [0, 1, 2, 3, 4, 7] + list(range(4)) + [SENTINEL] * 4
