"""brx_index_quoted_batch (include/brx.h, brx_index_quoted.hip): the delimiters of the decoded streams of a batch that lie outside
quoted fields, counted and located on the device.  Every expected value is numpy on the CPU (_one below).  In every arena the slack of
the slots and the gaps between them hold quote and delimiter bytes alternating: a kernel that reads one byte too far, or lets a byte in
front of a stream into its parity, gets another result.  In-process, one context."""
import json
import os

import numpy as np
import pytest

import brx_knobs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))
TILE = 65536  # one work item of the pass (brx_tiles.h); the tests below only choose lengths and addresses around it
SENTINEL = -0x0123456789ABCDEF
PAIRS = ((0x0A, 0x22), (0x00, 0xFF), (0x80, 0x00), (0xFF, 0x7F))  # (delim, quote)
NL, QT = 0x0A, 0x22


@pytest.fixture(scope="module")
def ctx():
    c = brx_knobs.context(0)
    yield c
    c.close()


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a))  # (a writable copy)
    return (t.to(dtype) if dtype is not None else t).to("cuda:0")


def _one(s, delim, quote):
    """-> (positions of the record delimiters of one stream, open)"""
    is_q = s == quote
    inside = (np.cumsum(is_q) - is_q) & 1
    pos = np.flatnonzero((s == delim) & (inside == 0))
    open_ = int(is_q.sum() & 1)
    return pos.astype(np.int64), open_


def _reference(host, offs, lens, delim, quote):
    """-> (counts, open, exclusive prefix sum, all positions back to back)"""
    per = [_one(host[o:o + ln], delim, quote) for o, ln in zip(offs, lens)]
    counts = np.array([p.size for p, _ in per], dtype=np.int64)
    opens = np.array([o for _, o in per], dtype=np.int32)
    pos_off = np.zeros(len(per), dtype=np.int64)
    np.cumsum(counts[:-1], out=pos_off[1:])
    return counts, opens, pos_off, (np.concatenate([p for p, _ in per]) if per else np.zeros(0, dtype=np.int64))


def _filler(size, delim, quote):
    """quote and delimiter bytes alternating"""
    return np.where(np.arange(size) % 2 == 0, quote, delim).astype(np.uint8)


def _check(ctx, host, arena, offs, lens, delim, quote):
    """Count mode, then fill mode (pos_off by torch.cumsum from the device's counts; count and open written again), both on raw
    pointers, against numpy."""
    import torch
    offs, lens = np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    n = len(lens)
    want_count, want_open, _, want_pos = _reference(host, offs, lens, delim, quote)
    tag = (hex(delim), hex(quote))
    d_off, d_len = _dev(offs), _dev(lens)
    count = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    open_ = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    args = (delim, quote, arena.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, arena.numel())
    ctx.index_quoted_batch_device(*args, count.data_ptr(), open_.data_ptr())
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
    ctx.index_quoted_batch_device(*args, count2.data_ptr(), open2.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), total)
    assert (count2.cpu().numpy() == want_count).all(), ("count written by fill mode", tag)
    assert (open2.cpu().numpy() == want_open).all(), ("open written by fill mode", tag)
    got_pos = pos.cpu().numpy()
    assert (got_pos[total:] == SENTINEL).all(), tag
    bad = np.nonzero(got_pos[:total] != want_pos)[0]
    assert bad.size == 0, ("pos", tag, bad[:8].tolist(), got_pos[bad[:8]].tolist(), want_pos[bad[:8]].tolist())


def _arena_tile_aligned(n_bytes):
    """A device arena and the offset in it of a 64 KiB aligned ADDRESS (tiles are cut in the address range)."""
    import torch
    arena = torch.empty(n_bytes + TILE, dtype=torch.uint8, device="cuda:0")
    return arena, (-arena.data_ptr()) % TILE


def test_check_values(ctx):
    """A CSV text with an embedded line feed, a doubled quote and an unterminated field at offset 1000 of a 4 KiB arena, by record
    delimiter and by field separator; empty streams at offset 0, at 1000 and at the arena's end -> 0 and 0.  The line feeds of the
    text are at 4, 9, 14, 17 and 23 with 1, 2, 5, 6 and 7 quotes in front of them, its commas at 1 and 7 with 0 and 2: by the rule
    of brx.h (and by numpy, asserted below) the positions are [9, 17] and [1, 7], count 2 and open 1 either way."""
    text = np.frombuffer(b'a,"x\ny",b\n"q""\nr"\n"open\n', dtype=np.uint8)
    offs, lens = [1000, 1000, 0, 4096], [len(text), 0, 0, 0]
    d_off, d_len = _dev(np.array(offs, dtype=np.int64)), _dev(np.array(lens, dtype=np.int64))
    for delim, want_pos in ((NL, [9, 17]), (ord(","), [1, 7])):
        assert _one(text, delim, QT)[0].tolist() == want_pos and _one(text, delim, QT)[1] == 1
        host = _filler(4096, delim, QT)
        host[1000:1000 + len(text)] = text
        arena = _dev(host)
        count, open_, pos_off, pos = ctx.index_quoted_batch(arena, d_off, d_len, delim=delim, quote=QT)
        assert count.cpu().tolist() == [2, 0, 0, 0]
        assert open_.cpu().tolist() == [1, 0, 0, 0]
        assert pos_off.cpu().tolist() == [0, 2, 2, 2]
        assert pos.cpu().tolist() == want_pos
        count, open_ = ctx.index_quoted_batch(arena, d_off, d_len, delim=delim, quote=QT, positions=False)
        assert count.cpu().tolist() == [2, 0, 0, 0] and open_.cpu().tolist() == [1, 0, 0, 0]
        _check(ctx, host, arena, offs, lens, delim, QT)


EDGE_LENS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 65535, 65536, 65537, 131077)


@pytest.mark.parametrize("delim,quote", PAIRS)
def test_chunk_row_and_tile_edges_at_every_alignment(ctx, delim, quote):
    """Every length around a chunk, a row and a tile at all 16 phases of out_off in one batch; in a second one a stream that starts 3
    bytes before a 64 KiB address boundary, one that starts 3 bytes behind one and ends on the next, one that starts 3 bytes before one
    and ends on the next.  Three-symbol alphabet {delim, quote, other}; count mode and fill mode."""
    rng = np.random.default_rng(2000 + delim)
    other = next(b for b in (delim ^ 0x80, delim ^ 0xFF, 0x41) if b not in (delim, quote))
    alphabet = np.array([delim, quote, other], dtype=np.uint8)
    offs, lens, at = [], [], 0
    for ln in EDGE_LENS:
        for phase in range(16):
            at = (at + 15) // 16 * 16 + phase + 16 * int(rng.integers(0, 5))
            offs.append(at)
            lens.append(ln)
            at += ln + int(rng.integers(0, 40))
    arena, base = _arena_tile_aligned(at + 64)  # (a 64 KiB aligned base: out_off mod 16 is the address mod 16)
    host = _filler(arena.numel(), delim, quote)
    offs = [base + o for o in offs]
    for o, ln in zip(offs, lens):
        host[o:o + ln] = alphabet[rng.integers(0, 3, ln)]
    arena.copy_(_dev(host))
    _check(ctx, host, arena, offs, lens, delim, quote)

    arena, base = _arena_tile_aligned(7 * TILE)
    host = _filler(arena.numel(), delim, quote)
    offs = [base + TILE - 3, base + 3 * TILE + 3, base + 5 * TILE - 3]
    lens = [70000, TILE - 3, TILE + 3]
    for o, ln in zip(offs, lens):
        host[o:o + ln] = alphabet[rng.integers(0, 3, ln)]
    arena.copy_(_dev(host))
    _check(ctx, host, arena, offs, lens, delim, quote)


CARRY_START = 5               # the stream starts 5 bytes behind a 64 KiB address
CARRY_LEN = 3 * TILE - 100    # ... and has 3 tiles
# address of the single quote, from that 64 KiB address: the last and the first byte of a lane's chunk, of a row and of a tile
CARRY_AT = {"chunk_last": TILE + 3 * 1024 + 16 * 7 + 15, "chunk_first": TILE + 3 * 1024 + 16 * 8, "row_last": TILE + 5 * 1024 + 1023,
            "row_first": TILE + 6 * 1024, "tile_last": 2 * TILE - 1, "tile_first": 2 * TILE, "stream_first": CARRY_START,
            "stream_last": CARRY_START + CARRY_LEN - 1}


def _carry_arena():
    arena, base = _arena_tile_aligned(4 * TILE)
    host = _filler(arena.numel(), NL, QT)
    host[base + CARRY_START:base + CARRY_START + CARRY_LEN] = NL
    return arena, base, host


@pytest.mark.parametrize("where", sorted(CARRY_AT))
def test_a_single_quote_where_the_carry_crosses(ctx, where):
    """All delimiters except one quote at stream offset p: the p delimiters in front of it count, those behind it do not, open = 1."""
    arena, base, host = _carry_arena()
    p = CARRY_AT[where] - CARRY_START
    assert (arena.data_ptr() + base) % TILE == 0 and 0 <= p < CARRY_LEN
    host[base + CARRY_START + p] = QT
    arena.copy_(_dev(host))
    counts, opens, _, pos = _reference(host, [base + CARRY_START], [CARRY_LEN], NL, QT)
    assert counts.tolist() == [p] and opens.tolist() == [1] and (pos == np.arange(p)).all()
    _check(ctx, host, arena, [base + CARRY_START], [CARRY_LEN], NL, QT)


def test_two_quotes_across_a_tile_edge_and_a_tile_of_quotes(ctx):
    """A quote on the last byte of the stream's second tile and one on the first byte of its third: only those two offsets are missing
    from pos, open = 0.  Then a middle tile made only of quotes, 65536 of them: parity 0, no delimiter of its own."""
    arena, base, host = _carry_arena()
    host[base + 2 * TILE - 1] = host[base + 2 * TILE] = QT
    arena.copy_(_dev(host))
    counts, opens, _, pos = _reference(host, [base + CARRY_START], [CARRY_LEN], NL, QT)
    p = 2 * TILE - 1 - CARRY_START
    assert counts.tolist() == [CARRY_LEN - 2] and opens.tolist() == [0]
    assert (pos == np.delete(np.arange(CARRY_LEN), [p, p + 1])).all()
    _check(ctx, host, arena, [base + CARRY_START], [CARRY_LEN], NL, QT)

    arena, base, host = _carry_arena()
    host[base + TILE:base + 2 * TILE] = QT
    arena.copy_(_dev(host))
    counts, opens, _, pos = _reference(host, [base + CARRY_START], [CARRY_LEN], NL, QT)
    assert counts.tolist() == [CARRY_LEN - TILE] and opens.tolist() == [0]
    _check(ctx, host, arena, [base + CARRY_START], [CARRY_LEN], NL, QT)


@pytest.mark.parametrize("one_quote_in", [4, 5000])
def test_order_and_parity_across_many_tiles(ctx, one_quote_in):
    """One stream of 4 MiB + 3 over {delim, quote, 'a', CR} at an odd offset: 65 tiles that finish in any order, positions in order,
    with quotes dense (every tile's parity matters) and sparse (long runs of tiles inside a quoted field)."""
    rng = np.random.default_rng(40 + one_quote_in)
    ln = (4 << 20) + 3
    host = _filler(ln + 4096, NL, QT)
    body = np.array([NL, 0x61, 0x0D], dtype=np.uint8)[rng.integers(0, 3, ln)]
    body[rng.integers(0, one_quote_in, ln) == 0] = QT
    host[777:777 + ln] = body
    arena = _dev(host)
    assert (arena.data_ptr() + 777) % 1024 + ln > 64 * TILE  # 65 tiles
    _check(ctx, host, arena, [777], [ln], NL, QT)
    count, open_, pos_off, pos = ctx.index_quoted_batch(arena, _dev(np.array([777], dtype=np.int64)), _dev(np.array([ln], dtype=np.int64)))
    want, want_open = _one(host[777:777 + ln], NL, QT)
    assert want.size > 1000
    assert count.cpu().tolist() == [want.size] and pos_off.cpu().tolist() == [0] and open_.cpu().tolist() == [want_open]
    assert (pos.cpu().numpy() == want).all()


def _small_batch(seed, n, top, delim=NL, quote=QT):
    """n streams of 0 .. top bytes over {delim, quote, 'x'} with gaps of 0 .. 20 filler bytes -> host arena, offs, lens"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, top + 1, n).astype(np.int64)
    lens[10::50] = 0  # empty streams ...
    lens[9::50] = np.maximum(lens[9::50], 1)  # ... between streams that get an odd number of quotes below
    lens[11::50] = np.maximum(lens[11::50], 1)
    gaps = rng.integers(0, 21, n).astype(np.int64)
    offs = np.cumsum(gaps) + np.concatenate(([0], np.cumsum(lens[:-1])))
    host = _filler(int(offs[-1] + lens[-1] + 16), delim, quote)
    body = np.array([delim, quote, 0x78], dtype=np.uint8)[rng.integers(0, 3, host.size)]
    for k, (o, ln) in enumerate(zip(offs, lens)):
        host[o:o + ln] = body[o:o + ln]
        if k % 50 in (9, 11) and (host[o:o + ln] == quote).sum() % 2 == 0:
            host[o] = 0x78 if host[o] == quote else quote
    return host, offs, lens


def test_many_small_streams(ctx):
    """9000 streams of 0 .. 40 bytes, one item each -- more items than the 8192 waves of a full grid on 256 CUs take by their index,
    so the rest come from the ticket counter.  Empty streams sit between streams of odd parity: nothing leaks across them."""
    host, offs, lens = _small_batch(79, 9000, 40)
    _, opens, _, _ = _reference(host, offs, lens, NL, QT)
    assert opens[9::50].all() and opens[11::50].all() and not lens[10::50].any()
    _check(ctx, host, _dev(host), offs, lens, NL, QT)


def _csv_texts(n, top):
    """n CSV texts of 0 .. top bytes: fields with embedded line feeds, doubled quotes and commas; every third cut inside a quoted field."""
    rng = np.random.default_rng(11)
    plain = [b"alpha", b"12", b"", b"x y z", b"3.14"]
    quoted = [b'"a\nb"', b'"say ""hi"""', b'"1,2"', b'"\n\n"', b'""', b'"tail\r\n"']
    rows = []
    for _ in range(400):
        fields = []
        for _ in range(int(rng.integers(1, 8))):
            kind = quoted if rng.integers(0, 3) == 0 else plain
            fields.append(kind[int(rng.integers(0, len(kind)))])
        rows.append(b",".join(fields) + b"\n")
    texts = []
    sizes = np.concatenate(([0, 1, top], rng.integers(0, top + 1, n - 3)))
    for k, size in enumerate(sizes):
        parts, have = [], 0
        while have < size:
            parts.append(rows[int(rng.integers(0, len(rows)))])
            have += len(parts[-1])
        t = b"".join(parts)[:int(size)]
        if k % 3 == 0 and len(t) > 20:  # cut in the middle of a quoted field
            t = t + b'x,"cut\nhere'
        texts.append(t)
    return texts


def test_behind_a_decode_without_a_synchronisation(ctx):
    """64 CSV texts (0 .. 200 KiB) compressed on the device, then on one HIP stream: decode, lens = out_len * (status == 0), quoted
    count mode, torch.cumsum, quoted fill mode with `total` from the CPU's count -- the host needs nothing from the device in between."""
    import torch
    from brotli_rs_amd import shard
    dev = torch.device("cuda:0")
    texts = _csv_texts(64, 200 << 10)
    n = len(texts)
    refs = [_one(np.frombuffer(t, dtype=np.uint8), NL, QT) for t in texts]
    assert sum(o for _, o in refs) >= 10 and sum(1 for _, o in refs if not o) >= 10
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
    out = _dev(_filler(int(out_off[-1]), NL, QT))
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
        args = (NL, QT, out.data_ptr(), d_out_off.data_ptr(), lens.data_ptr(), n, out.numel())
        ctx.index_quoted_batch_device(*args, count.data_ptr(), open_.data_ptr(), hip_stream=s.cuda_stream)
        pos_off = torch.cumsum(count, 0) - count
        ctx.index_quoted_batch_device(*args, None, None, pos_off.data_ptr(), pos.data_ptr(), total, hip_stream=s.cuda_stream)
    s.synchronize()
    assert status.cpu().tolist() == [0] * n
    assert out_len.cpu().tolist() == [len(t) for t in texts]
    assert count.cpu().tolist() == [p.size for p, _ in refs]
    assert open_.cpu().tolist() == [o for _, o in refs]
    got = pos.cpu().numpy()
    assert (got[:total] == np.concatenate([p for p, _ in refs])).all() and (got[total:] == SENTINEL).all()


def test_agreement_with_the_plain_pass_on_the_golden_batch(ctx):
    """All of tests/golden/data decoded in one BRX_MEM_DEVICE batch; with a quote byte that occurs in none of the outputs the quoted
    pass equals brx_index_batch in count and pos, and open is all 0.  Five of the golden outputs (compressed or random data) hold every
    one of the 256 byte values, so no byte value is absent from the whole batch: the quote is the first byte value absent from all the
    other outputs (the test asserts that there is one), both passes run over the whole batch, every stream without the quote byte
    must agree with the plain pass, and the five that hold it are held to the numpy rule instead."""
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
    assert free.size > 0
    quote = int(free[0])
    caps = [e["out_bytes"] + 64 + 7 * (k % 5) if e["status"] == 0 else 1 << 17 for k, e in enumerate(MANIFEST)]
    n = len(streams)
    in_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(s) for s in streams], out=in_off[1:])
    out_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(caps, out=out_off[1:])
    blob = _dev(np.frombuffer(b"".join(streams), dtype=np.uint8))
    d_in_off, d_out_off = _dev(in_off), _dev(out_off)
    out = _dev(_filler(int(out_off[-1]), NL, quote))
    out_len = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.decode_batch_device(blob.data_ptr(), d_in_off.data_ptr(), n, out.data_ptr(), d_out_off.data_ptr(), out_len.data_ptr(),
                            status.data_ptr())
    ctx.synchronize()
    assert status.cpu().tolist() == [e["status"] for e in MANIFEST]
    lens = out_len * (status == 0)
    plain_count, plain_off, plain_pos = ctx.index_batch(out, d_out_off, lens, delim=NL)
    count, open_, pos_off, pos = ctx.index_quoted_batch(out, d_out_off, lens, delim=NL, quote=quote)
    plain_count, plain_off, plain_pos = plain_count.cpu().numpy(), plain_off.cpu().numpy(), plain_pos.cpu().numpy()
    count, open_, pos_off, pos = count.cpu().numpy(), open_.cpu().numpy(), pos_off.cpu().numpy(), pos.cpu().numpy()
    for i in range(n):
        got = pos[pos_off[i]:pos_off[i] + count[i]]
        if full[i]:
            want, want_open = _one(outs[i], NL, quote)
            assert count[i] == want.size and open_[i] == want_open and (got == want).all(), i
        else:
            assert count[i] == plain_count[i] and open_[i] == 0, i
            assert (got == plain_pos[plain_off[i]:plain_off[i] + plain_count[i]]).all(), i
    assert plain_count.sum() > 10000


def test_total_is_a_bound(ctx):
    """Fill mode with room for half the entries: those are right, and the sentinels behind them are untouched."""
    import torch
    host, offs, lens = _small_batch(6, 300, 3000)
    arena = _dev(host)
    want_count, _, want_off, want_pos = _reference(host, offs, lens, NL, QT)
    half = int(want_pos.size // 2)
    assert half > 1000
    pos = torch.full((want_pos.size + 8,), SENTINEL, dtype=torch.int64, device="cuda:0")
    d_off, d_len, d_pos_off = _dev(offs), _dev(lens), _dev(want_off)
    torch.cuda.synchronize()
    ctx.index_quoted_batch_device(NL, QT, arena.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), len(lens), arena.numel(), None, None,
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
        want_count, want_open, want_off, want_pos = _reference(host, offs, lens, NL, QT)
        jobs.append(dict(arena=_dev(host), offs=_dev(offs), lens=_dev(lens), pos_off=_dev(want_off), n=len(lens), total=int(want_pos.size),
                         count=torch.full((len(lens),), -7, dtype=torch.int64, device=dev),
                         open=torch.full((len(lens),), -7, dtype=torch.int32, device=dev),
                         pos=torch.full((want_pos.size + 8,), SENTINEL, dtype=torch.int64, device=dev),
                         want_count=want_count, want_open=want_open, want_pos=want_pos))
    s = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    torch.cuda.synchronize()
    for k, j in enumerate(jobs):
        ctx.index_quoted_batch_device(NL, QT, j["arena"].data_ptr(), j["offs"].data_ptr(), j["lens"].data_ptr(), j["n"],
                                      j["arena"].numel(), j["count"].data_ptr(), j["open"].data_ptr(), j["pos_off"].data_ptr(),
                                      j["pos"].data_ptr(), j["total"], hip_stream=s[k % 2].cuda_stream)
    torch.cuda.synchronize()
    for k, j in enumerate(jobs):
        assert (j["count"].cpu().numpy() == j["want_count"]).all(), k
        assert (j["open"].cpu().numpy() == j["want_open"]).all(), k
        got = j["pos"].cpu().numpy()
        assert (got[:j["total"]] == j["want_pos"]).all() and (got[j["total"]:] == SENTINEL).all(), k


def test_arguments(ctx):
    """n = 0 -> BRX_SUCCESS; only one of pos_off / pos, count NULL in count mode, a NULL table, delim == quote ->
    BRX_ERR_INVALID_ARGUMENT; open NULL in either mode; then a good call on the same context still works."""
    import torch
    dev = torch.device("cuda:0")
    arena = torch.full((64,), NL, dtype=torch.uint8, device=dev)
    arena[20] = QT  # stream 1 = 4 delimiters, a quote, 3 delimiters inside the field it opens
    offs = torch.tensor([0, 16], dtype=torch.int64, device=dev)
    lens = torch.full((2,), 8, dtype=torch.int64, device=dev)
    count = torch.zeros(2, dtype=torch.int64, device=dev)
    open_ = torch.full((2,), -7, dtype=torch.int32, device=dev)
    pos_off = torch.tensor([0, 8], dtype=torch.int64, device=dev)
    pos = torch.full((16,), SENTINEL, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    lib, h = ctx._lib, ctx._h
    args = (arena.data_ptr(), offs.data_ptr(), lens.data_ptr())
    c, o = count.data_ptr(), open_.data_ptr()
    assert lib.brx_index_quoted_batch(h, NL, QT, *args, 0, 64, c, o, None, None, 0, None) == 0
    assert lib.brx_index_quoted_batch(h, NL, QT, None, None, None, 0, 0, c, None, None, None, 0, None) == 0
    assert lib.brx_index_quoted_batch(h, NL, QT, *args, 2, 64, c, o, pos_off.data_ptr(), None, 16, None) == -1
    assert b"brx_index_quoted_batch" in lib.brx_last_error()
    assert lib.brx_index_quoted_batch(h, NL, QT, *args, 2, 64, c, o, None, pos.data_ptr(), 16, None) == -1
    assert lib.brx_index_quoted_batch(h, NL, QT, *args, 2, 64, None, o, None, None, 0, None) == -1
    assert lib.brx_index_quoted_batch(h, NL, QT, arena.data_ptr(), None, lens.data_ptr(), 2, 64, c, o, None, None, 0, None) == -1
    assert lib.brx_index_quoted_batch(h, NL, NL, *args, 2, 64, c, o, None, None, 0, None) == -1
    assert b"quote" in lib.brx_last_error()
    assert open_.cpu().tolist() == [-7, -7] and count.cpu().tolist() == [0, 0]  # (nothing was launched)
    assert lib.brx_index_quoted_batch(h, NL, QT, *args, 2, 64, c, None, None, None, 0, None) == 0  # open NULL, count mode
    assert count.cpu().tolist() == [8, 4]
    assert lib.brx_index_quoted_batch(h, NL, QT, *args, 2, 64, None, None, pos_off.data_ptr(), pos.data_ptr(), 16, None) == 0  # both NULL, fill mode
    assert lib.brx_index_quoted_batch(h, NL, QT, *args, 2, 64, c, o, pos_off.data_ptr(), pos.data_ptr(), 16, None) == 0  # (the context still works)
    assert count.cpu().tolist() == [8, 4] and open_.cpu().tolist() == [0, 1]
    assert pos.cpu().tolist() == list(range(8)) + list(range(4)) + [SENTINEL] * 4
