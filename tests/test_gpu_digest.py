"""brx_digest_batch (include/brx.h, brx_digest.hip): CRC-32 / CRC-32C of the decoded streams of a batch, computed on the device.
Every expected value comes from the CPU: zlib.crc32 for kind 1, the table-driven CRC-32C below (pinned by the standard check
value) for kind 2.  In-process, one context."""
import ctypes
import json
import os
import zlib

import numpy as np
import pytest

import brx_knobs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))
TILE = 65536  # one work item of the pass (brx_tiles.h); the tests below only choose lengths around it

_C_TABLE = np.zeros(256, dtype=np.uint32)
for _i in range(256):
    _r = _i
    for _ in range(8):
        _r = (_r >> 1) ^ (0x82F63B78 if _r & 1 else 0)
    _C_TABLE[_i] = _r
_C_LIST = [int(x) for x in _C_TABLE]


def crc32c(data):
    """Table-driven CRC-32C (Castagnoli, reflected 0x82F63B78, init / xorout 0xFFFFFFFF), one byte per step."""
    c = 0xFFFFFFFF
    t = _C_LIST
    for b in bytes(data):
        c = t[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def crc32c_rows(rows, lens):
    """The same recurrence for many byte strings at once: rows[i, :lens[i]] (numpy uint8 2-D), one byte position per step."""
    lens = np.asarray(lens, dtype=np.int64)
    c = np.full(len(lens), 0xFFFFFFFF, dtype=np.uint32)
    for j in range(int(lens.max()) if len(lens) else 0):
        live = lens > j
        cj = c[live]
        c[live] = _C_TABLE[(cj ^ rows[live, j]) & 255] ^ (cj >> 8)
    return c ^ np.uint32(0xFFFFFFFF)


def test_the_cpu_crc32c_is_the_standard_one():
    assert crc32c(b"123456789") == 0xE3069283 and crc32c(b"") == 0
    rows = np.zeros((3, 9), dtype=np.uint8)
    rows[0] = rows[1] = np.frombuffer(b"123456789", dtype=np.uint8)
    assert crc32c_rows(rows, [9, 4, 0]).tolist() == [0xE3069283, crc32c(b"1234"), 0]
    assert zlib.crc32(b"123456789") == 0xCBF43926


CPU = {"crc32": lambda b: zlib.crc32(bytes(b)) & 0xFFFFFFFF, "crc32c": crc32c}


@pytest.fixture(scope="module")
def ctx():
    c = brx_knobs.context(0)
    yield c
    c.close()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a))  # (a writable copy)
    return (t.to(dtype) if dtype is not None else t).to("cuda:0")


def _digests(ctx, arena, offs, lens, kind, **kw):
    """arena: uint8 device tensor; offs / lens: host integer arrays -> np.uint32 digests."""
    return _u32(ctx.digest_batch(arena, _dev(np.asarray(offs, dtype=np.int64)), _dev(np.asarray(lens, dtype=np.int64)), kind=kind, **kw))


def test_check_values(ctx):
    """b"123456789" -> 0xCBF43926 / 0xE3069283; the empty string -> 0 for both kinds."""
    import torch
    arena = torch.full((4096,), 0xEE, dtype=torch.uint8, device="cuda:0")
    arena[1000:1009] = _dev(np.frombuffer(b"123456789", dtype=np.uint8))
    for kind, want in (("crc32", 0xCBF43926), ("crc32c", 0xE3069283)):
        got = _digests(ctx, arena, [1000, 1000, 0, 1009], [9, 0, 0, 0], kind)
        assert got.tolist() == [want, 0, 0, 0], (kind, [hex(x) for x in got])


def test_every_golden_stream_behind_its_decode_without_a_synchronisation(ctx):
    """All of tests/golden/data in one BRX_MEM_DEVICE batch (the reject vectors with their lengths zeroed), decode and both digest
    calls enqueued on one HIP stream with nothing in between but the zeroing."""
    import torch
    dev = torch.device("cuda:0")
    streams = [open(os.path.join(GOLDEN, "data", e["stream"]), "rb").read() for e in MANIFEST]
    caps = [e["out_bytes"] + 64 + 7 * (k % 5) if e["status"] == 0 else 1 << 17 for k, e in enumerate(MANIFEST)]
    n = len(streams)
    in_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(s) for s in streams], out=in_off[1:])
    out_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(caps, out=out_off[1:])
    blob = _dev(np.frombuffer(b"".join(streams), dtype=np.uint8))
    d_in_off, d_out_off = _dev(in_off), _dev(out_off)
    out = torch.full((int(out_off[-1]),), 0x77, dtype=torch.uint8, device=dev)
    out_len = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        ctx.decode_batch_device(blob.data_ptr(), d_in_off.data_ptr(), n, out.data_ptr(), d_out_off.data_ptr(), out_len.data_ptr(),
                                status.data_ptr(), hip_stream=s.cuda_stream)
        lens = out_len * (status == 0)
        d1 = ctx.digest_batch(out, d_out_off, lens, kind="crc32", stream=s)
        d2 = ctx.digest_batch(out, d_out_off, lens, kind="crc32c", stream=s)
    s.synchronize()
    assert status.cpu().tolist() == [e["status"] for e in MANIFEST]
    d1, d2 = _u32(d1), _u32(d2)
    for k, e in enumerate(MANIFEST):
        if e["status"] == 0:
            want = open(os.path.join(GOLDEN, "data", e["expected"]), "rb").read()
            assert len(want) == e["out_bytes"]
            assert int(d1[k]) == zlib.crc32(want) & 0xFFFFFFFF, e["stream"]
            assert int(d2[k]) == crc32c(want), e["stream"]
        else:
            assert int(d1[k]) == 0 and int(d2[k]) == 0, e["stream"]


def test_every_length_and_alignment(ctx):
    """Random bytes, every length 0 .. 3000 at all 16 phases of out_off; the slack of every slot is 0xA5 in one pass and 0x5A in the
    next: identical and correct results -- no byte beyond len[i] (or in front of out_off[i]) enters a digest."""
    import torch
    dev = torch.device("cuda:0")
    max_len, pitch = 3000, 3104  # pitch: a multiple of 16 with room for a phase of 15 and some slack behind the longest stream
    lens = np.repeat(np.arange(max_len + 1, dtype=np.int64), 16)
    phase = np.tile(np.arange(16, dtype=np.int64), max_len + 1)
    n = len(lens)
    offs = np.arange(n, dtype=np.int64) * pitch + phase
    g = torch.Generator(device=dev)
    g.manual_seed(20240607)
    data = torch.randint(0, 256, (n, pitch), dtype=torch.uint8, device=dev, generator=g)
    col = torch.arange(pitch, device=dev, dtype=torch.int32)[None, :]
    d_phase, d_lens = _dev(phase, torch.int32)[:, None], _dev(lens, torch.int32)[:, None]
    valid = (col >= d_phase) & (col < d_phase + d_lens)
    host = data.cpu().numpy()
    rows = np.zeros((n, max_len), dtype=np.uint8)
    for p in range(16):  # rows[i, :lens[i]] = the stream's bytes
        rows[p::16] = host[p::16, p:p + max_len]
    want = {"crc32": np.array([zlib.crc32(rows[i, :lens[i]].tobytes()) & 0xFFFFFFFF for i in range(n)], dtype=np.uint32),
            "crc32c": crc32c_rows(rows, lens)}
    for kind in ("crc32", "crc32c"):
        got = []
        for fill in (0xA5, 0x5A):
            arena = torch.where(valid, data, torch.full_like(data, fill)).reshape(-1)
            got.append(_digests(ctx, arena, offs, lens, kind))
        assert (got[0] == got[1]).all(), kind
        bad = np.nonzero(got[0] != want[kind])[0]
        assert bad.size == 0, (kind, [(int(lens[i]), int(phase[i])) for i in bad[:8]])


def test_one_stream_of_70_mib(ctx):
    """A single large stream is many work items, not one wavefront's serial job: the tiles of one stream fold into one digest."""
    import torch
    dev = torch.device("cuda:0")
    n_bytes = (70 << 20) + 12345
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    arena = torch.randint(0, 256, (n_bytes + 64,), dtype=torch.uint8, device=dev, generator=g)
    host = arena.cpu().numpy()
    for kind in ("crc32", "crc32c"):
        got = _digests(ctx, arena, [3, 0], [n_bytes, 17], kind)
        assert int(got[0]) == CPU[kind](host[3:3 + n_bytes]), kind
        assert int(got[1]) == CPU[kind](host[:17]), kind


def test_lengths_around_one_and_two_tiles(ctx):
    """Exactly one tile, one tile +- 1, two tiles - 1 -- at a 1 KiB aligned address (tiles are cut in the address range) and off it."""
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    lens1 = [TILE, TILE - 1, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, TILE - 1023, TILE - 1024, 1024, 1023, 1025]
    pitch = 3 * TILE
    arena = torch.randint(0, 256, (pitch * len(lens1) * 4 + 2048,), dtype=torch.uint8, device=dev, generator=g)
    base = (-arena.data_ptr()) % 1024
    offs, lens = [], []
    for k, ph in enumerate((0, 1, 16, 1023)):
        for j, ln in enumerate(lens1):
            offs.append(base + (k * len(lens1) + j) * pitch + ph)
            lens.append(ln)
    host = arena.cpu().numpy()
    for kind in ("crc32", "crc32c"):
        got = _digests(ctx, arena, offs, lens, kind)
        for o, ln, d in zip(offs, lens, got):
            assert int(d) == CPU[kind](host[o:o + ln]), (kind, o - base, ln)


def _log_uniform_batch(seed=1234, n=4096, top=4 << 20):
    rng = np.random.default_rng(seed)
    lens = np.clip(np.floor(np.exp(rng.uniform(0.0, np.log(top), n))).astype(np.int64), 1, top)
    slots = lens + rng.integers(0, 64, n)
    offs = np.zeros(n, dtype=np.int64)
    np.cumsum(slots[:-1], out=offs[1:])
    return offs, lens, int(offs[-1] + slots[-1])


def test_batch_of_4096_log_uniform_lengths(ctx):
    """4096 streams, lengths log-uniform over 1 B .. 4 MiB (fixed seed), at whatever phase the slots leave them: CRC-32 of all of them,
    CRC-32C of a fixed sample (the CPU implementation is slow)."""
    import torch
    dev = torch.device("cuda:0")
    offs, lens, total = _log_uniform_batch()
    g = torch.Generator(device=dev)
    g.manual_seed(99)
    arena = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=g)
    host = arena.cpu().numpy()
    got = _digests(ctx, arena, offs, lens, "crc32")
    want = np.array([zlib.crc32(host[o:o + ln]) & 0xFFFFFFFF for o, ln in zip(offs, lens)], dtype=np.uint32)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(int(i), int(lens[i])) for i in bad[:8]]
    got_c = _digests(ctx, arena, offs, lens, "crc32c")
    sample = [i for i in range(0, len(lens), 128) if lens[i] <= (1 << 20)]
    assert len(sample) >= 16
    for i in sample:
        assert int(got_c[i]) == crc32c(host[offs[i]:offs[i] + lens[i]]), (i, int(lens[i]))


def test_expect_and_mismatch(ctx):
    """With the right digests and three of them corrupted, mismatch has exactly those three ones; digest is written as without."""
    import torch
    dev = torch.device("cuda:0")
    offs, lens, total = _log_uniform_batch(seed=5, n=300, top=200000)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    arena = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=g)
    host = arena.cpu().numpy()
    d_offs, d_lens = _dev(offs), _dev(lens)
    for kind in ("crc32", "crc32c"):
        right = np.array([CPU[kind](host[o:o + ln]) for o, ln in zip(offs, lens)], dtype=np.uint32)
        wrong = right.copy()
        for i, flip in ((0, 1), (137, 0x80000000), (299, 0xFFFFFFFF)):
            wrong[i] ^= np.uint32(flip)
        digest, mismatch = ctx.digest_batch(arena, d_offs, d_lens, kind=kind, expect=_dev(wrong.view(np.int32)))
        assert (_u32(digest) == right).all(), kind
        assert np.nonzero(mismatch.cpu().numpy())[0].tolist() == [0, 137, 299], kind
        assert int(mismatch.sum()) == 3
        digest, mismatch = ctx.digest_batch(arena, d_offs, d_lens, kind=kind, expect=_dev(right.view(np.int32)))
        assert int(mismatch.sum()) == 0 and (_u32(digest) == right).all()


def test_two_calls_on_two_streams_of_one_context(ctx):
    """Two calls enqueued back to back on two HIP streams over different batches: each launch has scratch of its own."""
    import torch
    dev = torch.device("cuda:0")
    batches = []
    for seed in (21, 22):
        offs, lens, total = _log_uniform_batch(seed=seed, n=1500, top=1 << 20)
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        arena = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=g)
        batches.append((arena, _dev(offs), _dev(lens), offs, lens))
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for _ in range(3):  # (more calls than one pair: regions of the scratch ring are taken in turn)
        r1 = ctx.digest_batch(batches[0][0], batches[0][1], batches[0][2], kind="crc32", stream=s1)
        r2 = ctx.digest_batch(batches[1][0], batches[1][1], batches[1][2], kind="crc32", stream=s2)
    s1.synchronize()
    s2.synchronize()
    for (arena, _, _, offs, lens), r in zip(batches, (r1, r2)):
        host = arena.cpu().numpy()
        want = np.array([zlib.crc32(host[o:o + ln]) & 0xFFFFFFFF for o, ln in zip(offs, lens)], dtype=np.uint32)
        assert (_u32(r) == want).all()


def test_arguments(ctx):
    """Unknown kind, digest NULL, only one of expect / mismatch -> BRX_ERR_INVALID_ARGUMENT; n == 0 -> BRX_SUCCESS."""
    import torch
    dev = torch.device("cuda:0")
    arena = torch.zeros(64, dtype=torch.uint8, device=dev)
    offs = torch.zeros(2, dtype=torch.int64, device=dev)
    lens = torch.full((2,), 8, dtype=torch.int64, device=dev)
    words = torch.zeros(2, dtype=torch.int32, device=dev)
    other = torch.zeros(2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    lib, h = ctx._lib, ctx._h
    args = (arena.data_ptr(), offs.data_ptr(), lens.data_ptr())
    for kind in (0, 3, 0xFFFFFFFF):
        assert lib.brx_digest_batch(h, kind, *args, 2, words.data_ptr(), None, None, None) == -1
    assert lib.brx_digest_batch(h, 1, *args, 2, None, None, None, None) == -1
    assert lib.brx_digest_batch(h, 1, *args, 2, words.data_ptr(), other.data_ptr(), None, None) == -1
    assert lib.brx_digest_batch(h, 2, *args, 2, words.data_ptr(), None, other.data_ptr(), None) == -1
    assert lib.brx_digest_batch(h, 1, *args, 0, words.data_ptr(), None, None, None) == 0
    assert lib.brx_digest_batch(h, 2, None, None, None, 0, words.data_ptr(), None, None, None) == 0
    assert lib.brx_digest_batch(h, 1, *args, 2, words.data_ptr(), None, None, None) == 0  # (and the context still works)
    assert _u32(words).tolist() == [zlib.crc32(bytes(8)) & 0xFFFFFFFF] * 2
