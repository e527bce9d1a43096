"""brx_index_batch (include/brx.h, brx_index.hip): the delimiters of the decoded streams of a batch, counted and located on the device.
Every expected value is np.flatnonzero(buf[off:off+len] == delim) on the CPU.  In every arena the slack of the slots and the gaps
between them hold the delimiter itself: a kernel that reads one byte too far counts it.  In-process, one context."""
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
DELIMS = (0x0A, 0x00, 0x80, 0xFF)


@pytest.fixture(scope="module")
def ctx():
    c = brx_knobs.context(0)
    yield c
    c.close()


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a))  # (a writable copy)
    return (t.to(dtype) if dtype is not None else t).to("cuda:0")


def _reference(host, offs, lens, delim):
    """-> (counts, exclusive prefix sum, all positions back to back), int64"""
    per = [np.flatnonzero(host[o:o + ln] == delim).astype(np.int64) for o, ln in zip(offs, lens)]
    counts = np.array([p.size for p in per], dtype=np.int64)
    pos_off = np.zeros(len(per), dtype=np.int64)
    np.cumsum(counts[:-1], out=pos_off[1:])
    return counts, pos_off, (np.concatenate(per) if per else np.zeros(0, dtype=np.int64))


def _check(ctx, host, arena, offs, lens, delim):
    """Count mode, then fill mode (pos_off by torch.cumsum from the device's counts), both on raw pointers, against numpy."""
    import torch
    offs, lens = np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    n = len(lens)
    want_count, _, want_pos = _reference(host, offs, lens, delim)
    d_off, d_len = _dev(offs), _dev(lens)
    count = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    args = (delim, arena.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, arena.numel())
    ctx.index_batch_device(*args, count.data_ptr())
    got = count.cpu().numpy()
    bad = np.nonzero(got != want_count)[0]
    assert bad.size == 0, ("count", hex(delim), [(int(offs[i]), int(lens[i]), int(got[i]), int(want_count[i])) for i in bad[:8]])
    pos_off = torch.cumsum(count, 0) - count
    total = int(want_count.sum())
    pos = torch.full((total + 8,), SENTINEL, dtype=torch.int64, device="cuda:0")
    count2 = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.index_batch_device(*args, count2.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), total)
    assert (count2.cpu().numpy() == want_count).all(), ("count written by fill mode", hex(delim))
    got_pos = pos.cpu().numpy()
    assert (got_pos[total:] == SENTINEL).all(), hex(delim)
    bad = np.nonzero(got_pos[:total] != want_pos)[0]
    assert bad.size == 0, ("pos", hex(delim), bad[:8].tolist(), got_pos[bad[:8]].tolist(), want_pos[bad[:8]].tolist())


def _arena_tile_aligned(n_bytes):
    """A device arena and the offset in it of a 64 KiB aligned ADDRESS (tiles are cut in the address range)."""
    import torch
    arena = torch.empty(n_bytes + TILE, dtype=torch.uint8, device="cuda:0")
    return arena, (-arena.data_ptr()) % TILE


def test_check_values(ctx):
    """b"\\na\\n\\nbc\\n" at offset 1000 of a 4 KiB arena -> count 4, pos [0, 2, 3, 6]; empty streams there, at offset 0 and at the
    arena's end -> nothing."""
    host = np.full(4096, 0x0A, dtype=np.uint8)
    text = np.frombuffer(b"\na\n\nbc\n", dtype=np.uint8)
    host[1000:1000 + len(text)] = text
    arena = _dev(host)
    offs, lens = [1000, 1000, 0, 4096], [len(text), 0, 0, 0]
    count, pos_off, pos = ctx.index_batch(arena, _dev(np.array(offs, dtype=np.int64)), _dev(np.array(lens, dtype=np.int64)), delim=10)
    assert count.cpu().tolist() == [4, 0, 0, 0]
    assert pos_off.cpu().tolist() == [0, 4, 4, 4]
    assert pos.cpu().tolist() == [0, 2, 3, 6]
    only = ctx.index_batch(arena, _dev(np.array(offs, dtype=np.int64)), _dev(np.array(lens, dtype=np.int64)), delim=10, positions=False)
    assert only.cpu().tolist() == [4, 0, 0, 0]
    _check(ctx, host, arena, offs, lens, 0x0A)


EDGE_LENS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 65535, 65536, 65537, 131077)


@pytest.mark.parametrize("delim", DELIMS)
def test_chunk_row_and_tile_edges_at_every_alignment(ctx, delim):
    """Every length around a chunk, a row and a tile at all 16 phases of out_off in one batch; in a second one a stream that starts 3
    bytes before a 64 KiB address boundary, one that starts 3 bytes behind one and ends on the next, one that starts 3 bytes before one
    and ends on the next.  Two-symbol alphabet {delim, other}; count mode and fill mode."""
    rng = np.random.default_rng(1000 + delim)
    other = delim ^ 0x80 if delim in (0x00, 0x80) else delim ^ 0xFF  # 0x00 <-> 0x80 differ in the top bit only: the unsigned compare
    offs, lens, at = [], [], 0
    for ln in EDGE_LENS:
        for phase in range(16):
            at = (at + 15) // 16 * 16 + phase + 16 * int(rng.integers(0, 5))
            offs.append(at)
            lens.append(ln)
            at += ln + int(rng.integers(0, 40))
    arena, base = _arena_tile_aligned(at + 64)  # (a 64 KiB aligned base: out_off mod 16 is the address mod 16)
    host = np.full(arena.numel(), delim, dtype=np.uint8)
    offs = [base + o for o in offs]
    for o, ln in zip(offs, lens):
        host[o:o + ln] = np.where(rng.integers(0, 2, ln) == 1, delim, other).astype(np.uint8)
    arena.copy_(_dev(host))
    _check(ctx, host, arena, offs, lens, delim)

    arena, base = _arena_tile_aligned(7 * TILE)
    host = np.full(arena.numel(), delim, dtype=np.uint8)
    offs = [base + TILE - 3, base + 3 * TILE + 3, base + 5 * TILE - 3]
    lens = [70000, TILE - 3, TILE + 3]
    for o, ln in zip(offs, lens):
        host[o:o + ln] = np.where(rng.integers(0, 2, ln) == 1, delim, other).astype(np.uint8)
    arena.copy_(_dev(host))
    _check(ctx, host, arena, offs, lens, delim)


def test_densities(ctx):
    """All delimiters (count = len, pos = arange); none; only the first and the last byte; only the last byte of one tile and the
    first byte of the next."""
    arena, base = _arena_tile_aligned(10 * TILE)
    host = np.full(arena.numel(), 0x0A, dtype=np.uint8)
    offs = [base + 7, base + 4 * TILE + 1, base + 6 * TILE + 100 + 9, base + 8 * TILE + 200 + 5]
    lens = [200000, 70000, 70001, 100000]
    host[offs[1]:offs[1] + lens[1]] = 0x20
    host[offs[2] + 1:offs[2] + lens[2] - 1] = 0x20
    host[offs[3]:offs[3] + lens[3]] = 0x20
    edge = TILE - (offs[3] - base) % 1024  # stream offset of the first byte of the stream's second tile
    host[offs[3] + edge - 1] = host[offs[3] + edge] = 0x0A
    arena.copy_(_dev(host))
    counts, _, pos = _reference(host, offs, lens, 0x0A)
    assert counts.tolist() == [200000, 0, 2, 2]
    assert (pos[:200000] == np.arange(200000)).all() and pos[200000:].tolist() == [0, 70000, edge - 1, edge]
    _check(ctx, host, arena, offs, lens, 0x0A)


def test_order_across_many_tiles(ctx):
    """One stream of 4 MiB + 3 over a four-symbol alphabet at an odd offset: 65 tiles that finish in any order, positions in order."""
    rng = np.random.default_rng(4)
    ln = (4 << 20) + 3
    host = np.full(ln + 4096, 0x0A, dtype=np.uint8)
    host[777:777 + ln] = np.array([0x0A, 0x20, 0x61, 0x0D], dtype=np.uint8)[rng.integers(0, 4, ln)]
    arena = _dev(host)
    assert (arena.data_ptr() + 777) % 1024 + ln > 64 * TILE  # 65 tiles
    _check(ctx, host, arena, [777], [ln], 0x0A)
    count, pos_off, pos = ctx.index_batch(arena, _dev(np.array([777], dtype=np.int64)), _dev(np.array([ln], dtype=np.int64)))
    want = np.flatnonzero(host[777:777 + ln] == 0x0A)
    assert count.cpu().tolist() == [want.size] and pos_off.cpu().tolist() == [0]
    assert (pos.cpu().numpy() == want).all()


def test_every_golden_stream_behind_its_decode_without_a_synchronisation(ctx):
    """All of tests/golden/data in one BRX_MEM_DEVICE batch (the reject vectors with their lengths zeroed on the device): decode, count
    mode, torch.cumsum and fill mode enqueued on one HIP stream; `total` comes from the CPU's count of the golden outputs, so the host
    needs nothing from the device in between."""
    import torch
    dev = torch.device("cuda:0")
    streams = [open(os.path.join(GOLDEN, "data", e["stream"]), "rb").read() for e in MANIFEST]
    want = []
    for e in MANIFEST:
        data = open(os.path.join(GOLDEN, "data", e["expected"]), "rb").read() if e["status"] == 0 else b""
        want.append(np.flatnonzero(np.frombuffer(data, dtype=np.uint8) == 0x0A).astype(np.int64))
    total = int(sum(w.size for w in want))
    caps = [e["out_bytes"] + 64 + 7 * (k % 5) if e["status"] == 0 else 1 << 17 for k, e in enumerate(MANIFEST)]
    n = len(streams)
    in_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(s) for s in streams], out=in_off[1:])
    out_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(caps, out=out_off[1:])
    blob = _dev(np.frombuffer(b"".join(streams), dtype=np.uint8))
    d_in_off, d_out_off = _dev(in_off), _dev(out_off)
    out = torch.full((int(out_off[-1]),), 0x0A, dtype=torch.uint8, device=dev)
    out_len = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    count = torch.full((n,), -7, dtype=torch.int64, device=dev)
    pos = torch.full((total + 8,), SENTINEL, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        ctx.decode_batch_device(blob.data_ptr(), d_in_off.data_ptr(), n, out.data_ptr(), d_out_off.data_ptr(), out_len.data_ptr(),
                                status.data_ptr(), hip_stream=s.cuda_stream)
        lens = out_len * (status == 0)
        args = (0x0A, out.data_ptr(), d_out_off.data_ptr(), lens.data_ptr(), n, out.numel())
        ctx.index_batch_device(*args, count.data_ptr(), hip_stream=s.cuda_stream)
        pos_off = torch.cumsum(count, 0) - count
        ctx.index_batch_device(*args, None, pos_off.data_ptr(), pos.data_ptr(), total, hip_stream=s.cuda_stream)
    s.synchronize()
    assert status.cpu().tolist() == [e["status"] for e in MANIFEST]
    assert count.cpu().tolist() == [w.size for w in want]
    got = pos.cpu().numpy()
    assert (got[:total] == np.concatenate(want)).all() and (got[total:] == SENTINEL).all()


def _small_batch(seed, n, top, delim=0x0A):
    """n streams of 0 .. top bytes over {delim, 'x'} with gaps of 0 .. 20 delimiters -> host arena, offs, lens"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, top + 1, n).astype(np.int64)
    gaps = rng.integers(0, 21, n).astype(np.int64)
    offs = np.cumsum(gaps) + np.concatenate(([0], np.cumsum(lens[:-1])))
    host = np.full(int(offs[-1] + lens[-1] + 16), delim, dtype=np.uint8)
    body = np.where(rng.integers(0, 3, host.size) == 0, delim, 0x78).astype(np.uint8)
    for o, ln in zip(offs, lens):
        host[o:o + ln] = body[o:o + ln]
    return host, offs, lens


def test_total_is_a_bound(ctx):
    """Fill mode with room for half the entries: those are right, and the sentinels behind them are untouched."""
    import torch
    host, offs, lens = _small_batch(6, 300, 3000)
    arena = _dev(host)
    want_count, want_off, want_pos = _reference(host, offs, lens, 0x0A)
    half = int(want_pos.size // 2)
    assert half > 1000
    pos = torch.full((want_pos.size + 8,), SENTINEL, dtype=torch.int64, device="cuda:0")
    d_off, d_len, d_pos_off = _dev(offs), _dev(lens), _dev(want_off)
    torch.cuda.synchronize()
    ctx.index_batch_device(0x0A, arena.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), len(lens), arena.numel(), None,
                           d_pos_off.data_ptr(), pos.data_ptr(), half)
    got = pos.cpu().numpy()
    assert (got[:half] == want_pos[:half]).all()
    assert (got[half:] == SENTINEL).all()


@pytest.mark.parametrize("n", [5000, 9000])
def test_many_small_streams(ctx, n):
    """Streams of 0 .. 40 bytes, one item each: 5000 of them, and 9000 -- more items than the 8192 waves of a full grid on 256 CUs take
    by their index, so the rest come from the ticket counter."""
    host, offs, lens = _small_batch(70 + n, n, 40)
    _check(ctx, host, _dev(host), offs, lens, 0x0A)


def test_overlapping_calls_on_two_streams(ctx):
    """20 fill-mode calls alternating between two HIP streams over different small batches -- more than the 16 regions of the scratch
    ring -- and one synchronisation at the end."""
    import torch
    dev = torch.device("cuda:0")
    jobs = []
    for k in range(20):
        host, offs, lens = _small_batch(800 + k, 40 + k, 3000)
        want_count, want_off, want_pos = _reference(host, offs, lens, 0x0A)
        jobs.append(dict(arena=_dev(host), offs=_dev(offs), lens=_dev(lens), pos_off=_dev(want_off), n=len(lens), total=int(want_pos.size),
                         count=torch.full((len(lens),), -7, dtype=torch.int64, device=dev),
                         pos=torch.full((want_pos.size + 8,), SENTINEL, dtype=torch.int64, device=dev),
                         want_count=want_count, want_pos=want_pos))
    s = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    torch.cuda.synchronize()
    for k, j in enumerate(jobs):
        ctx.index_batch_device(0x0A, j["arena"].data_ptr(), j["offs"].data_ptr(), j["lens"].data_ptr(), j["n"], j["arena"].numel(),
                               j["count"].data_ptr(), j["pos_off"].data_ptr(), j["pos"].data_ptr(), j["total"],
                               hip_stream=s[k % 2].cuda_stream)
    torch.cuda.synchronize()
    for k, j in enumerate(jobs):
        assert (j["count"].cpu().numpy() == j["want_count"]).all(), k
        got = j["pos"].cpu().numpy()
        assert (got[:j["total"]] == j["want_pos"]).all() and (got[j["total"]:] == SENTINEL).all(), k


def test_arguments(ctx):
    """n = 0 -> BRX_SUCCESS; only one of pos_off / pos, count NULL in count mode -> BRX_ERR_INVALID_ARGUMENT."""
    import torch
    dev = torch.device("cuda:0")
    arena = torch.full((64,), 0x0A, dtype=torch.uint8, device=dev)
    offs = torch.tensor([0, 16], dtype=torch.int64, device=dev)
    lens = torch.full((2,), 8, dtype=torch.int64, device=dev)
    count = torch.zeros(2, dtype=torch.int64, device=dev)
    pos_off = torch.tensor([0, 8], dtype=torch.int64, device=dev)
    pos = torch.zeros(16, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    lib, h = ctx._lib, ctx._h
    args = (arena.data_ptr(), offs.data_ptr(), lens.data_ptr())
    assert lib.brx_index_batch(h, 10, *args, 0, 64, count.data_ptr(), None, None, 0, None) == 0
    assert lib.brx_index_batch(h, 10, None, None, None, 0, 0, count.data_ptr(), None, None, 0, None) == 0
    assert lib.brx_index_batch(h, 10, *args, 2, 64, count.data_ptr(), pos_off.data_ptr(), None, 16, None) == -1
    assert lib.brx_index_batch(h, 10, *args, 2, 64, count.data_ptr(), None, pos.data_ptr(), 16, None) == -1
    assert lib.brx_index_batch(h, 10, *args, 2, 64, None, None, None, 0, None) == -1
    assert lib.brx_index_batch(h, 10, arena.data_ptr(), None, lens.data_ptr(), 2, 64, count.data_ptr(), None, None, 0, None) == -1
    assert lib.brx_index_batch(h, 10, *args, 2, 64, count.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), 16, None) == 0  # (the context still works)
    assert count.cpu().tolist() == [8, 8] and pos.cpu().tolist() == list(range(8)) * 2
