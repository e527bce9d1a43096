"""The two pieces that brx_digest_batch and brx_index_batch share (csrc/brx_tiles.h, brx_tiles.hip, PassRing in brx_api.cpp): the plan
kernel's slices with empty streams in them, and the ring of scratch regions with calls in flight.  Every expected value comes from the
CPU: zlib.crc32, the table-driven CRC-32C of test_gpu_digest.py, np.flatnonzero.  In-process, one context."""
import zlib

import numpy as np
import pytest

import brx_knobs
from brotli_rs_amd import brx
from test_gpu_digest import crc32c, crc32c_rows

pytestmark = pytest.mark.gpu

TILE = 65536  # one work item of a pass (brx_tiles.h)
PLAN_THREADS = 1024  # the plan kernel gives each of its threads ceil(n / 1024) consecutive streams
SENTINEL = -0x0123456789ABCDEF
NL, OTHER = 0x0A, 0x41
BIG = (65537, 131077, 1)


@pytest.fixture(scope="module")
def ctx():
    c = brx_knobs.context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")  # (a writable copy)


def _plan_lens(n, rng):
    """Lengths 0 .. 40, one in eight 0; the first and the last stream empty; four empty streams in a row across the boundary between the
    slices of plan threads 299 and 300; BIG with an empty stream on either side of each.  A batch too small for that mix (n = 1, 2)
    is the end of [0, 131077]: one stream of three tiles, with an empty one in front of it where there is room."""
    if n < 16:
        return np.array([0, 131077][-n:], dtype=np.int64)
    lens = rng.integers(1, 41, n).astype(np.int64)
    lens[rng.integers(0, 8, n) == 0] = 0
    per = (n + PLAN_THREADS - 1) // PLAN_THREADS
    b = 300 * per
    lens[b - 2:b + 2] = 0
    p = n // 2
    lens[p:p + 7] = [0, BIG[0], 0, BIG[1], 0, BIG[2], 0]
    lens[0] = lens[n - 1] = 0
    return lens


def _crcs(host, offs, lens):
    """-> {kind: np.uint32 per stream}: zlib for CRC-32; CRC-32C by rows for the short streams, one by one for the long ones"""
    short = lens <= 40
    rows = np.zeros((len(lens), 40), dtype=np.uint8)
    for i in np.nonzero(short)[0]:
        rows[i, :lens[i]] = host[offs[i]:offs[i] + lens[i]]
    c = crc32c_rows(rows, np.where(short, lens, 0))
    for i in np.nonzero(~short)[0]:
        c[i] = crc32c(host[offs[i]:offs[i] + lens[i]])
    return {"crc32": np.array([zlib.crc32(host[o:o + ln].tobytes()) & 0xFFFFFFFF for o, ln in zip(offs, lens)], dtype=np.uint32), "crc32c": c}


def _positions(host, offs, lens):
    """-> (counts, exclusive prefix sum, all positions back to back), int64"""
    per = [np.flatnonzero(host[o:o + ln] == NL).astype(np.int64) for o, ln in zip(offs, lens)]
    counts = np.array([p.size for p in per], dtype=np.int64)
    return counts, np.cumsum(counts) - counts, np.concatenate(per)


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 2049])
def test_plan_slices_and_empty_streams_in_both_passes(ctx, n):
    """n where the plan's slice per thread changes (1 -> 2 -> 3 streams) and where trailing threads get nothing, over the lengths of
    _plan_lens at mixed 16-byte phases in a 64 KiB aligned arena of {0x0A, 0x41} whose slack is 0x0A: every digest of both kinds, every
    count (count mode and fill mode; the plan clears both halves of a 64-bit word), every position, the sentinels behind `total`."""
    import torch
    rng = np.random.default_rng(4000 + n)
    lens = _plan_lens(n, rng)
    assert n < 16 or (lens[0] == 0 and lens[-1] == 0 and set(BIG) <= set(lens.tolist()))
    offs, at = np.zeros(n, dtype=np.int64), 0
    for i in range(n):
        at = (at + 15) // 16 * 16 + int(rng.integers(0, 16)) + 16 * int(rng.integers(0, 3))
        offs[i] = at
        at += int(lens[i])
    arena = torch.empty(at + 64 + TILE, dtype=torch.uint8, device="cuda:0")
    offs += (-arena.data_ptr()) % TILE  # (a 64 KiB aligned base: out_off mod 16 is the address mod 16)
    host = np.full(arena.numel(), NL, dtype=np.uint8)
    for o, ln in zip(offs, lens):
        host[o:o + ln] = np.where(rng.integers(0, 2, ln) == 1, NL, OTHER).astype(np.uint8)
    arena.copy_(_dev(host))
    d_off, d_len = _dev(offs), _dev(lens)
    want = _crcs(host, offs, lens)
    for kind in ("crc32", "crc32c"):
        got = ctx.digest_batch(arena, d_off, d_len, kind=kind).cpu().numpy().view(np.uint32)
        bad = np.nonzero(got != want[kind])[0]
        assert bad.size == 0, (kind, [(int(i), int(lens[i])) for i in bad[:8]])
    want_count, want_off, want_pos = _positions(host, offs, lens)
    total = int(want_count.sum())
    args = (NL, arena.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, arena.numel())
    count = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.index_batch_device(*args, count.data_ptr())
    bad = np.nonzero(count.cpu().numpy() != want_count)[0]
    assert bad.size == 0, ("count", [(int(i), int(lens[i])) for i in bad[:8]])
    count2 = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    pos = torch.full((total + 8,), SENTINEL, dtype=torch.int64, device="cuda:0")
    d_pos_off = _dev(want_off)
    torch.cuda.synchronize()
    ctx.index_batch_device(*args, count2.data_ptr(), d_pos_off.data_ptr(), pos.data_ptr(), total)
    assert (count2.cpu().numpy() == want_count).all(), "count written by fill mode"
    got_pos = pos.cpu().numpy()
    assert (got_pos[total:] == SENTINEL).all()
    bad = np.nonzero(got_pos[:total] != want_pos)[0]
    assert bad.size == 0, ("pos", bad[:8].tolist(), got_pos[bad[:8]].tolist(), want_pos[bad[:8]].tolist())


def _ring_batch(seed, n):
    """n streams of 0 .. 24 bytes over {0x0A, 0x41} with gaps of 0 .. 8 delimiters -> host arena, offs, lens"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 25, n).astype(np.int64)
    offs = np.cumsum(rng.integers(0, 9, n)) + np.concatenate(([0], np.cumsum(lens[:-1])))
    host = np.full(int(offs[-1] + lens[-1] + 16), NL, dtype=np.uint8)
    body = np.where(rng.integers(0, 3, host.size) == 0, NL, OTHER).astype(np.uint8)
    for o, ln in zip(offs, lens):
        host[o:o + ln] = body[o:o + ln]
    return host, offs, lens


def test_ring_wrap_and_growth_with_calls_in_flight():
    """40 digest calls, then 40 fill-mode index calls, on one HIP stream with no synchronisation in between: more than twice the 16
    regions of either ring.  Every call has a batch and outputs of its own; calls 1 .. 20 of either pass have 8 streams, calls 21 .. 40
    have 1100 -- beyond the 8 + 2 + 1024 the first regions hold, so the scratch grows once in mid-sequence (a context of its own: its
    rings start empty)."""
    import torch
    ctx = brx_knobs.context(0)
    dev = torch.device("cuda:0")
    jobs, data = [], 0
    for k in range(80):
        n = 8 if k % 40 < 20 else 1100
        host, offs, lens = _ring_batch(9000 + k, n)
        data += host.size
        j = dict(n=n, arena=_dev(host), offs=_dev(offs), lens=_dev(lens))
        if k < 40:
            j["kind"] = ("crc32", "crc32c")[k % 2]
            rows = np.zeros((n, 24), dtype=np.uint8)
            for i in range(n):
                rows[i, :lens[i]] = host[offs[i]:offs[i] + lens[i]]
            j["want"] = (crc32c_rows(rows, lens) if k % 2 else
                         np.array([zlib.crc32(rows[i, :lens[i]].tobytes()) & 0xFFFFFFFF for i in range(n)], dtype=np.uint32))
            j["digest"] = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        else:
            j["want_count"], want_off, j["want_pos"] = _positions(host, offs, lens)
            j["total"] = int(j["want_pos"].size)
            j["pos_off"] = _dev(want_off)
            j["count"] = torch.full((n,), -7, dtype=torch.int64, device=dev)
            j["pos"] = torch.full((j["total"] + 8,), SENTINEL, dtype=torch.int64, device=dev)
        jobs.append(j)
    assert data < 2 << 20
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for j in jobs[:40]:
        ctx.digest_batch_device(brx.DIGEST_KINDS[j["kind"]], j["arena"].data_ptr(), j["offs"].data_ptr(), j["lens"].data_ptr(), j["n"],
                                j["digest"].data_ptr(), hip_stream=s.cuda_stream)
    for j in jobs[40:]:
        ctx.index_batch_device(NL, j["arena"].data_ptr(), j["offs"].data_ptr(), j["lens"].data_ptr(), j["n"], j["arena"].numel(),
                               j["count"].data_ptr(), j["pos_off"].data_ptr(), j["pos"].data_ptr(), j["total"], hip_stream=s.cuda_stream)
    s.synchronize()
    ctx.close()
    for k, j in enumerate(jobs[:40]):
        assert (j["digest"].cpu().numpy().view(np.uint32) == j["want"]).all(), (k, j["kind"])
    for k, j in enumerate(jobs[40:]):
        assert (j["count"].cpu().numpy() == j["want_count"]).all(), k
        got = j["pos"].cpu().numpy()
        assert (got[:j["total"]] == j["want_pos"]).all() and (got[j["total"]:] == SENTINEL).all(), k
