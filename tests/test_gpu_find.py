"""brx_find_batch (include/brx.h, brx_find.hip): the occurrences of a byte sequence of 1 .. 16 bytes in the decoded streams of a batch,
counted and located on the device.  Every expected value is numpy on the CPU (_one below).  In every arena the slack of the slots and
the gaps between them hold the needle repeated: a kernel that reads one byte too far, or lets a byte in front of a stream into a
match, finds something there.  In-process, one context."""
import ctypes

import numpy as np
import pytest

import brx_knobs

pytestmark = pytest.mark.gpu

TILE = 65536  # one work item of the pass (brx_tiles.h); the tests below only choose lengths and addresses around it
ROW = 1024    # what a wave reads per step, 16 bytes per lane
SENTINEL = -0x0123456789ABCDEF
CRLF = b"\r\n"
NEEDLES = (bytes([0x00, 0xFF]), bytes([0x80, 0x80, 0x0A]), bytes([0x0D, 0x0A, 0xFF, 0x0D, 0x0A]), bytes(range(16)))  # m = 2, 3, 5, 16


@pytest.fixture(scope="module")
def ctx():
    c = brx_knobs.context(0)
    yield c
    c.close()


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a))  # (a writable copy)
    return (t.to(dtype) if dtype is not None else t).to("cuda:0")


def _np(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def _one(s, needle):
    """-> offsets of the occurrences of `needle` in the stream s, overlapping ones included"""
    m, L = len(needle), int(s.size)
    if L < m:
        return np.zeros(0, dtype=np.int64)
    ok = np.ones(L - m + 1, dtype=bool)
    for k in range(m):
        ok &= s[k:L - m + 1 + k] == needle[k]
    return np.flatnonzero(ok).astype(np.int64)


def _reference(host, offs, lens, needle):
    """-> (counts, exclusive prefix sum, all positions back to back)"""
    per = [_one(host[o:o + ln], needle) for o, ln in zip(offs, lens)]
    counts = np.array([p.size for p in per], dtype=np.int64)
    pos_off = np.zeros(len(per), dtype=np.int64)
    np.cumsum(counts[:-1], out=pos_off[1:])
    return counts, pos_off, (np.concatenate(per) if per else np.zeros(0, dtype=np.int64))


def _filler(size, needle):
    """the needle repeated"""
    return np.resize(_np(needle), size).copy()


def _check(ctx, host, arena, offs, lens, needle):
    """Count mode, then fill mode (pos_off by torch.cumsum from the device's counts; count written again), both on raw pointers,
    against numpy.  -> (counts, positions) as numpy gave them."""
    import torch
    offs, lens = np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    n = len(lens)
    want_count, _, want_pos = _reference(host, offs, lens, needle)
    tag = needle.hex()
    d_off, d_len = _dev(offs), _dev(lens)
    count = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    args = (needle, arena.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, arena.numel())
    ctx.find_batch_device(*args, count.data_ptr())
    got = count.cpu().numpy()
    bad = np.nonzero(got != want_count)[0]
    assert bad.size == 0, ("count", tag, [(int(offs[i]), int(lens[i]), int(got[i]), int(want_count[i])) for i in bad[:8]])
    pos_off = torch.cumsum(count, 0) - count
    total = int(want_count.sum())
    pos = torch.full((total + 8,), SENTINEL, dtype=torch.int64, device="cuda:0")
    count2 = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.find_batch_device(*args, count2.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), total)
    assert (count2.cpu().numpy() == want_count).all(), ("count written by fill mode", tag)
    got_pos = pos.cpu().numpy()
    assert (got_pos[total:] == SENTINEL).all(), tag
    bad = np.nonzero(got_pos[:total] != want_pos)[0]
    assert bad.size == 0, ("pos", tag, bad[:8].tolist(), got_pos[bad[:8]].tolist(), want_pos[bad[:8]].tolist())
    return want_count, want_pos


def _arena_tile_aligned(n_bytes):
    """A device arena and the offset in it of a 64 KiB aligned ADDRESS (tiles are cut in the address range)."""
    import torch
    arena = torch.empty(n_bytes + TILE, dtype=torch.uint8, device="cuda:0")
    return arena, (-arena.data_ptr()) % TILE


def _pieces(rng, size, needle, alphabet=None):
    """`size` bytes of a random concatenation of pieces, each the needle (probability 1/2) or 1 .. m random bytes of `alphabet`
    (default: the needle's own bytes)."""
    m = len(needle)
    p = _np(needle)
    alphabet = np.unique(p) if alphabet is None else np.asarray(alphabet, dtype=np.uint8)
    k = 2 * size // (m + 1) + 16  # (a piece has (m + (m + 1) / 2) / 2 >= (m + 1) / 2 bytes on average; the assert below holds it)
    is_needle = rng.integers(0, 2, k).astype(bool)
    lens = np.where(is_needle, m, rng.integers(1, m + 1, k))
    assert lens.sum() >= size
    starts = np.cumsum(lens) - lens
    within = np.arange(lens.sum()) - np.repeat(starts, lens)
    body = np.where(np.repeat(is_needle, lens), p[within], alphabet[rng.integers(0, alphabet.size, within.size)])
    return body[:size].astype(np.uint8)


def test_check_values(ctx):
    """b'ab\\r\\ncd\\n\\r\\n\\r\\n\\r' at offset 1000 of a 4 KiB arena: CR LF at 2, 7 and 9 (the LF at 6 is alone, the CR at 11 ends the
    text), LF CR LF at 6 and 8 (overlapping).  Empty streams at 0, at 1000 and at the arena's end."""
    text = _np(b"ab\r\ncd\n\r\n\r\n\r")
    offs, lens = [1000, 1000, 0, 4096], [len(text), 0, 0, 0]
    d_off, d_len = _dev(np.array(offs, dtype=np.int64)), _dev(np.array(lens, dtype=np.int64))
    for needle, want_pos in ((CRLF, [2, 7, 9]), (b"\n\r\n", [6, 8])):
        assert _one(text, needle).tolist() == want_pos
        host = _filler(4096, needle)
        host[1000:1000 + len(text)] = text
        arena = _dev(host)
        k = len(want_pos)
        count, pos_off, pos = ctx.find_batch(arena, d_off, d_len, needle)
        assert count.cpu().tolist() == [k, 0, 0, 0]
        assert pos_off.cpu().tolist() == [0, k, k, k]
        assert pos.cpu().tolist() == want_pos
        count = ctx.find_batch(arena, d_off, d_len, needle, positions=False)
        assert count.cpu().tolist() == [k, 0, 0, 0]
        _check(ctx, host, arena, offs, lens, needle)


EDGE_LENS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 65535, 65536, 65537, 131077)


def _edge_layout(rng):
    """Every length around a chunk, a row and a tile at all 16 phases of out_off -> (offs relative to a 64 KiB aligned base, lens, size)"""
    offs, lens, at = [], [], 0
    for ln in EDGE_LENS:
        for phase in range(16):
            at = (at + 15) // 16 * 16 + phase + 16 * int(rng.integers(0, 5))
            offs.append(at)
            lens.append(ln)
            at += ln + int(rng.integers(0, 40))
    return offs, lens, at + 64


def _edge_batch(rng, needle, alphabet=None):
    """-> (host, arena, offs, lens): the edge-length batch against a 64 KiB aligned base (out_off mod 16 is the address mod 16)"""
    offs, lens, size = _edge_layout(rng)
    arena, base = _arena_tile_aligned(size)
    host = _filler(arena.numel(), needle)
    offs = [base + o for o in offs]
    body = _pieces(rng, sum(lens), needle, alphabet)
    at = 0
    for o, ln in zip(offs, lens):
        host[o:o + ln] = body[at:at + ln]
        at += ln
    arena.copy_(_dev(host))
    return host, arena, offs, lens


@pytest.mark.parametrize("delim", [0x0A, 0x00, 0x80, 0xFF])
def test_m1_is_the_plain_pass(ctx, delim):
    """A needle of one byte over the edge-length batch (three-symbol alphabet): count and pos equal numpy and brx_index_batch."""
    rng = np.random.default_rng(3000 + delim)
    needle = bytes([delim])
    alphabet = [delim, delim ^ 0x80, delim ^ 0xFF]
    host, arena, offs, lens = _edge_batch(rng, needle, alphabet)
    want_count, want_pos = _check(ctx, host, arena, offs, lens, needle)
    assert want_pos.size > 1000
    d_off, d_len = _dev(np.array(offs, dtype=np.int64)), _dev(np.array(lens, dtype=np.int64))
    count, pos_off, pos = ctx.find_batch(arena, d_off, d_len, needle)
    plain_count, plain_off, plain_pos = ctx.index_batch(arena, d_off, d_len, delim=delim)
    assert (count.cpu().numpy() == want_count).all() and (plain_count.cpu().numpy() == want_count).all()
    assert (pos_off.cpu().numpy() == plain_off.cpu().numpy()).all()
    assert (pos.cpu().numpy() == want_pos).all() and (plain_pos.cpu().numpy() == want_pos).all()


@pytest.mark.parametrize("needle", NEEDLES, ids=lambda b: b.hex())
def test_chunk_row_and_tile_edges_at_every_alignment(ctx, needle):
    """Every length around a chunk, a row and a tile at all 16 phases of out_off in one batch; in a second one a stream that starts 3
    bytes before a 64 KiB address boundary, one that starts 3 bytes behind one and ends on the next, one that starts 3 bytes before one
    and ends on the next.  Contents: the needle and fragments over its alphabet (0x00 / 0xFF / 0x80 in the needles: the zero-byte test
    has no carry to get wrong; all of 0 .. 15 in the last one: the filler byte is 16)."""
    rng = np.random.default_rng(2000 + len(needle))
    host, arena, offs, lens = _edge_batch(rng, needle)
    _, want_pos = _check(ctx, host, arena, offs, lens, needle)
    assert want_pos.size >= 1000

    arena, base = _arena_tile_aligned(7 * TILE)
    host = _filler(arena.numel(), needle)
    offs = [base + TILE - 3, base + 3 * TILE + 3, base + 5 * TILE - 3]
    lens = [70000, TILE - 3, TILE + 3]
    for o, ln in zip(offs, lens):
        host[o:o + ln] = _pieces(rng, ln, needle)
    arena.copy_(_dev(host))
    _check(ctx, host, arena, offs, lens, needle)


SPLIT_START = 5                # the stream starts 5 bytes behind a 64 KiB address
SPLIT_LEN = 16 * TILE + 5000   # ... and has 17 tiles


@pytest.mark.parametrize("background", ["absent", "first"])
@pytest.mark.parametrize("m", [16, 2, 3, 5])
def test_every_split_across_every_kind_of_edge(ctx, m, background):
    """needle = 1, 2, .. m.  For every split k = 1 .. m - 1 three copies: one whose first k bytes end on the last byte of a lane's chunk
    inside a row, one whose first k bytes end on the last byte of a row inside a tile, one whose first k bytes end on the last byte of
    tile k.  Everything else is one byte value: one that is not in the needle, or the needle's first byte (every copy is then preceded
    by partial matches).  Exactly the 3 (m - 1) planted positions are found."""
    needle = bytes(range(1, m + 1))
    arena, base = _arena_tile_aligned(17 * TILE)
    assert (arena.data_ptr() + base) % TILE == 0
    host = _filler(arena.numel(), needle)
    s0 = base + SPLIT_START
    host[s0:s0 + SPLIT_LEN] = 0x61 if background == "absent" else needle[0]
    plants = []
    for k in range(1, m):
        for last_of_prefix in (2 * k * ROW + 16 * (7 + k) + 15,   # row 2 k of tile 0, lane 7 + k: the last byte of its chunk
                               (2 * k + 1) * ROW + ROW - 1,       # the last byte of row 2 k + 1 of tile 0
                               (k + 1) * TILE - 1):               # the last byte of tile k
            start = base + last_of_prefix - (k - 1)
            host[start:start + m] = _np(needle)
            plants.append(start - s0)
    plants = np.array(sorted(plants), dtype=np.int64)
    assert plants.size == 3 * (m - 1) and plants[0] > 0 and plants[-1] + m <= SPLIT_LEN and (np.diff(plants) >= 32).all()
    arena.copy_(_dev(host))
    want_count, want_pos = _check(ctx, host, arena, [s0], [SPLIT_LEN], needle)
    assert want_count.tolist() == [3 * (m - 1)] and (want_pos == plants).all()


@pytest.mark.parametrize("needle", NEEDLES, ids=lambda b: b.hex())
def test_stream_edges(ctx, needle):
    """Back-to-back slots with gap 0, the first stream at arena offset 0, the last one ending at `span` (no multiple of 16).  No byte
    outside a stream takes part in a match: not a neighbouring stream, not the slack in front of or behind the stream."""
    m = len(needle)
    x = bytes([0x61])
    parts, want = [], []  # parts: (bytes, is it a stream); want: the expected count of every stream

    def stream(b, k):
        parts.append((bytes(b), True))
        want.append(k)

    def slack(b):
        parts.append((bytes(b), False))

    stream(needle + x * 20, 1)  # at arena offset 0
    for k in range(1, m):  # A ends with the needle's first k bytes, B starts with its remaining ones
        stream(x * 20 + needle[:k], 0)
        stream(needle[k:] + x * 20, 0)
    stream(needle, 1)  # exactly the needle
    stream(b"", 0)
    for k in range(m):  # the needle's first k bytes, the rest of it follows in the slack
        stream(needle[:k], 0)
        slack(needle[k:])
    for _ in range(3):  # the needle's last m - 1 bytes lead, its first byte lies in front of the stream in the slot
        slack(needle[:1])
        stream(needle[1:] + x * 10, 0)
    stream(needle + x * (70000 - 2 * m) + needle, 2)  # first and last m bytes of a 70 000-byte stream
    size = sum(len(b) for b, _ in parts)
    pad = 33 + ((size + 33 + m) % 16 == 0)  # (span is no multiple of 16)
    stream(x * pad + needle, 1)  # the last stream ends at span
    host = np.concatenate([_np(b) for b, _ in parts])
    assert host.size % 16 != 0
    offs, lens, at = [], [], 0
    for b, is_stream in parts:
        if is_stream:
            offs.append(at)
            lens.append(len(b))
        at += len(b)
    assert offs[0] == 0 and offs[-1] + lens[-1] == host.size
    arena = _dev(host)
    want_count, want_pos = _check(ctx, host, arena, offs, lens, needle)
    assert want_count.tolist() == want
    big = lens.index(70000)
    lo = int(want_count[:big].sum())
    assert want_pos[lo:lo + 2].tolist() == [0, 70000 - m]


@pytest.mark.parametrize("m", [1, 2, 16])
def test_self_overlap_in_a_run(ctx, m):
    """200 000 bytes of 'a' at an odd offset, needle 'a' * m: every offset up to L - m is an occurrence -- 16 per lane chunk, every
    lane, every row: the prefix sum over the lanes and the up to 16 stores per lane of the fill pass."""
    needle = b"a" * m
    ln = 200000
    host = _filler(ln + 4096, needle)  # ('a' everywhere: one byte too far is one occurrence too many)
    arena = _dev(host)
    want_count, want_pos = _check(ctx, host, arena, [1237], [ln], needle)
    assert want_count.tolist() == [ln - m + 1] and (want_pos == np.arange(ln - m + 1)).all()


def _small_batch(seed, n, top, needle, alphabet=(0x61, 0x62)):
    """n streams of 0 .. top bytes over `alphabet` with gaps of 0 .. 20 filler bytes -> host arena, offs, lens"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, top + 1, n).astype(np.int64)
    lens[10::50] = 0  # empty streams between the others
    gaps = rng.integers(0, 21, n).astype(np.int64)
    offs = np.cumsum(gaps) + np.concatenate(([0], np.cumsum(lens[:-1])))
    host = _filler(int(offs[-1] + lens[-1] + 16), needle)
    body = np.array(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), host.size)]
    for o, ln in zip(offs, lens):
        host[o:o + ln] = body[o:o + ln]
    return host, offs, lens


def test_many_small_streams(ctx):
    """9000 streams of 0 .. 40 bytes over two letters, one item each -- more items than the 8192 waves of a full grid on 256 CUs take
    by their index, so the rest come from the ticket counter.  Empty streams and streams shorter than the needle sit between the others."""
    needle = b"aba"
    host, offs, lens = _small_batch(79, 9000, 40, needle)
    assert not lens[10::50].any() and ((lens > 0) & (lens < 3)).sum() > 100
    want_count, _ = _check(ctx, host, _dev(host), offs, lens, needle)
    assert want_count.sum() > 10000


def test_order_across_many_tiles(ctx):
    """One stream of 4 MiB + 3 over four symbols at an odd offset: 65 tiles that finish in any order, positions in order."""
    rng = np.random.default_rng(41)
    ln = (4 << 20) + 3
    host = _filler(ln + 4096, CRLF)
    host[777:777 + ln] = np.array([0x0D, 0x0A, 0x61, 0x20], dtype=np.uint8)[rng.integers(0, 4, ln)]
    arena = _dev(host)
    assert (arena.data_ptr() + 777) % 1024 + ln > 64 * TILE  # 65 tiles
    _check(ctx, host, arena, [777], [ln], CRLF)
    count, pos_off, pos = ctx.find_batch(arena, _dev(np.array([777], dtype=np.int64)), _dev(np.array([ln], dtype=np.int64)), CRLF)
    want = _one(host[777:777 + ln], CRLF)
    assert want.size > 1000
    assert count.cpu().tolist() == [want.size] and pos_off.cpu().tolist() == [0]
    got = pos.cpu().numpy()
    assert (np.diff(got) > 0).all() and (got == want).all()


def _crlf_texts(n, top):
    """n CRLF texts of 0 .. top bytes; every third holds lone line feeds, every fourth lone carriage returns."""
    rng = np.random.default_rng(12)
    words = [b"alpha", b"12", b"", b"x y z", b"3.14", b"Content-Length: 0", b"WARC/1.0"]
    texts = []
    sizes = np.concatenate(([0, 1, top], rng.integers(0, top + 1, n - 3)))
    for k, size in enumerate(sizes):
        ends = [CRLF] * 6 + ([b"\n"] if k % 3 == 0 else []) + ([b"\r"] if k % 4 == 0 else [])
        lines = [b" ".join(words[int(i)] for i in rng.integers(0, len(words), 4)) + ends[int(rng.integers(0, len(ends)))]
                 for _ in range(200)]
        parts, have = [], 0
        while have < size:
            parts.append(lines[int(rng.integers(0, len(lines)))])
            have += len(parts[-1])
        texts.append(b"".join(parts)[:int(size)])
    return texts


def test_behind_a_decode_without_a_synchronisation(ctx):
    """64 CRLF texts (0 .. 200 KiB) compressed on the device, then on one HIP stream: decode, lens = out_len * (status == 0), find CR LF
    in count mode, torch.cumsum, fill mode with `total` from the CPU's count -- the host needs nothing from the device in between."""
    import torch
    from brotli_rs_amd import shard
    dev = torch.device("cuda:0")
    texts = _crlf_texts(64, 200 << 10)
    n = len(texts)
    refs = [_one(_np(t), CRLF) for t in texts]
    lone_lf = sum(1 for t, r in zip(texts, refs) if t.count(b"\n") > r.size)
    lone_cr = sum(1 for t, r in zip(texts, refs) if t.count(b"\r") > r.size)
    assert lone_lf >= 10 and lone_cr >= 10
    total = int(sum(p.size for p in refs))
    src_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=src_off[1:])
    slots = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([ctx.generate_slot_bytes(len(t)) for t in texts], out=slots[1:])
    caps = [len(t) + 64 + 7 * (k % 5) for k, t in enumerate(texts)]
    out_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(caps, out=out_off[1:])
    src = _dev(_np(b"".join(texts)))
    d_src_off, d_slots, d_out_off = _dev(src_off), _dev(slots), _dev(out_off)
    comp = torch.zeros(int(slots[-1]), dtype=torch.uint8, device=dev)
    comp_len = torch.zeros(n, dtype=torch.int64, device=dev)
    gst = torch.full((n,), -1, dtype=torch.int32, device=dev)
    out = _dev(_filler(int(out_off[-1]), CRLF))
    out_len = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    count = torch.full((n,), -7, dtype=torch.int64, device=dev)
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
        args = (CRLF, out.data_ptr(), d_out_off.data_ptr(), lens.data_ptr(), n, out.numel())
        ctx.find_batch_device(*args, count.data_ptr(), hip_stream=s.cuda_stream)
        pos_off = torch.cumsum(count, 0) - count
        ctx.find_batch_device(*args, None, pos_off.data_ptr(), pos.data_ptr(), total, hip_stream=s.cuda_stream)
    s.synchronize()
    assert status.cpu().tolist() == [0] * n
    assert out_len.cpu().tolist() == [len(t) for t in texts]
    assert count.cpu().tolist() == [p.size for p in refs]
    got = pos.cpu().numpy()
    assert (got[:total] == np.concatenate(refs)).all() and (got[total:] == SENTINEL).all()


def test_total_is_a_bound(ctx):
    """Fill mode with room for half the entries: those are right, and the sentinels behind them are untouched."""
    import torch
    needle = b"ab"
    host, offs, lens = _small_batch(6, 300, 3000, needle)
    arena = _dev(host)
    _, want_off, want_pos = _reference(host, offs, lens, needle)
    half = int(want_pos.size // 2)
    assert half > 1000
    pos = torch.full((want_pos.size + 8,), SENTINEL, dtype=torch.int64, device="cuda:0")
    d_off, d_len, d_pos_off = _dev(offs), _dev(lens), _dev(want_off)
    torch.cuda.synchronize()
    ctx.find_batch_device(needle, arena.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), len(lens), arena.numel(), None,
                          d_pos_off.data_ptr(), pos.data_ptr(), half)
    got = pos.cpu().numpy()
    assert (got[:half] == want_pos[:half]).all()
    assert (got[half:] == SENTINEL).all()


def test_overlapping_calls_on_two_streams(ctx):
    """20 fill-mode calls alternating between two HIP streams over different small batches, each with a needle of its own -- more
    than the 16 regions of the scratch ring -- and one synchronisation at the end."""
    import torch
    dev = torch.device("cuda:0")
    jobs = []
    for k in range(20):
        needle = bytes(0x61 + int(d) for d in format(k + 1, "b"))  # 1 .. 5 letters of {a, b}, different for every k
        host, offs, lens = _small_batch(800 + k, 60 + k, 3000, needle)
        want_count, want_off, want_pos = _reference(host, offs, lens, needle)
        jobs.append(dict(needle=needle, arena=_dev(host), offs=_dev(offs), lens=_dev(lens), pos_off=_dev(want_off), n=len(lens),
                         total=int(want_pos.size), count=torch.full((len(lens),), -7, dtype=torch.int64, device=dev),
                         pos=torch.full((want_pos.size + 8,), SENTINEL, dtype=torch.int64, device=dev),
                         want_count=want_count, want_pos=want_pos))
    assert len(set(j["needle"] for j in jobs)) == 20
    s = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    torch.cuda.synchronize()
    for k, j in enumerate(jobs):
        ctx.find_batch_device(j["needle"], j["arena"].data_ptr(), j["offs"].data_ptr(), j["lens"].data_ptr(), j["n"], j["arena"].numel(),
                              j["count"].data_ptr(), j["pos_off"].data_ptr(), j["pos"].data_ptr(), j["total"],
                              hip_stream=s[k % 2].cuda_stream)
    torch.cuda.synchronize()
    for k, j in enumerate(jobs):
        assert j["total"] > 100, k
        assert (j["count"].cpu().numpy() == j["want_count"]).all(), k
        got = j["pos"].cpu().numpy()
        assert (got[:j["total"]] == j["want_pos"]).all() and (got[j["total"]:] == SENTINEL).all(), k


def test_arguments(ctx):
    """needle NULL, needle_len 0 and 17, only one of pos_off / pos, count NULL in count mode, a NULL table -> BRX_ERR_INVALID_ARGUMENT
    with nothing launched; n = 0 -> BRX_SUCCESS; count NULL in fill mode; the Python wrapper raises from the library's answer; then a
    good call on the same context.  A needle buffer overwritten right behind an enqueue-only call does not change that call's result."""
    import torch
    from brotli_rs_amd import brx
    dev = torch.device("cuda:0")
    arena = torch.full((64,), 0x0A, dtype=torch.uint8, device=dev)  # stream 0 = 8 LF: 7 x LF LF; stream 1 = 8 LF at 16
    arena[20] = 0x0D                                                # ... with a CR at its byte 4: LF LF at 0, 1, 2, 5, 6
    offs = torch.tensor([0, 16], dtype=torch.int64, device=dev)
    lens = torch.full((2,), 8, dtype=torch.int64, device=dev)
    count = torch.full((2,), -7, dtype=torch.int64, device=dev)
    pos_off = torch.tensor([0, 7], dtype=torch.int64, device=dev)
    pos = torch.full((16,), SENTINEL, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    lib, h = ctx._lib, ctx._h
    args = (arena.data_ptr(), offs.data_ptr(), lens.data_ptr())
    c, nn = count.data_ptr(), b"\n\n"
    refused = [lib.brx_find_batch(h, None, 2, *args, 2, 64, c, None, None, 0, None),
               lib.brx_find_batch(h, nn, 0, *args, 2, 64, c, None, None, 0, None),
               lib.brx_find_batch(h, b"\n" * 17, 17, *args, 2, 64, c, None, None, 0, None),
               lib.brx_find_batch(h, nn, 2, *args, 2, 64, c, pos_off.data_ptr(), None, 16, None),
               lib.brx_find_batch(h, nn, 2, *args, 2, 64, c, None, pos.data_ptr(), 16, None),
               lib.brx_find_batch(h, nn, 2, *args, 2, 64, None, None, None, 0, None),
               lib.brx_find_batch(h, nn, 2, arena.data_ptr(), None, lens.data_ptr(), 2, 64, c, None, None, 0, None),
               lib.brx_find_batch(h, nn, 2, arena.data_ptr(), offs.data_ptr(), None, 2, 64, c, None, None, 0, None)]
    assert refused == [-1] * len(refused)
    assert lib.brx_last_error().startswith(b"brx_find_batch:")
    for bad in (b"", b"x" * 17):
        with pytest.raises(brx.BrxError, match="brx_find_batch"):
            ctx.find_batch_device(bad, *args, 2, 64, c)
    assert lib.brx_find_batch(h, nn, 2, *args, 0, 64, c, None, None, 0, None) == 0  # n = 0
    assert lib.brx_find_batch(h, nn, 2, None, None, None, 0, 0, c, None, None, 0, None) == 0
    ctx.synchronize()
    assert count.cpu().tolist() == [-7, -7] and pos.cpu().tolist() == [SENTINEL] * 16  # (nothing was launched)
    assert lib.brx_find_batch(h, nn, 2, *args, 2, 64, None, pos_off.data_ptr(), pos.data_ptr(), 16, None) == 0  # count NULL, fill mode
    assert pos.cpu().tolist() == list(range(7)) + [0, 1, 2, 5, 6] + [SENTINEL] * 4
    pos.fill_(SENTINEL)
    torch.cuda.synchronize()
    assert lib.brx_find_batch(h, nn, 2, *args, 2, 64, c, pos_off.data_ptr(), pos.data_ptr(), 16, None) == 0  # (the context still works)
    assert count.cpu().tolist() == [7, 5]
    assert pos.cpu().tolist() == list(range(7)) + [0, 1, 2, 5, 6] + [SENTINEL] * 4
    # the needle's bytes are taken during the call: the buffer is the caller's again when it returns
    buf = ctypes.create_string_buffer(b"\n\n", 2)
    count.fill_(-7)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    assert lib.brx_find_batch(h, buf, 2, *args, 2, 64, c, None, None, 0, s.cuda_stream) == 0
    buf.raw = b"\r\n"
    s.synchronize()
    assert count.cpu().tolist() == [7, 5]
