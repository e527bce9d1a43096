"""brx_hash_batch (include/brx.h, brx_hash.hip): a 64-bit key of every selected record of the decoded streams of a batch.  Every expected
value comes from tests/hash_oracle.py (Python integers), the records from tests/take_oracle.py.  hash and rec_len are pre-filled with
a sentinel and carry spare entries behind m, which must keep it.  In-process, one context."""
import numpy as np
import pytest

import brx_knobs
import hash_oracle
import take_oracle

pytestmark = pytest.mark.gpu

LONG = 1024   # BRX_HASH_LONG (brx_hash.h): from here on a record is hashed by its wave, one row of 64 x 16 bytes at a time
SENT = -7     # the sentinel of hash and rec_len
SPARE = 8
NO_DELIM, TRIM_CR = 1, 2
FLAGS = (0, NO_DELIM, NO_DELIM | TRIM_CR)
M64 = (1 << 64) - 1


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


class Batch:
    """An arena on the host and on the device with its tables, and the positions of an index at `delims` (or whatever the test puts
    in their place)."""

    def __init__(self, host, offs, lens, delims=b"\n", positions=None):
        self.host = np.ascontiguousarray(host, dtype=np.uint8)
        self.offs, self.lens = np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64)
        self.n = len(self.lens)
        self.count, self.pos_off, self.pos = positions if positions is not None else take_oracle.index_positions(self.host, offs, lens, delims)
        self.n_pos = len(self.pos)
        self.arena = _dev(self.host)
        self.d_off, self.d_len = _dev(self.offs), _dev(self.lens)
        self.d_count, self.d_pos_off = _dev(np.asarray(self.count, dtype=np.int64)), _dev(np.asarray(self.pos_off, dtype=np.int64))
        self.d_pos = _dev(np.asarray(self.pos, dtype=np.int64)) if len(self.pos) else None

    def head(self):
        return (self.arena.data_ptr(), self.d_off.data_ptr(), self.d_len.data_ptr(), self.n, int(self.arena.numel()),
                self.d_count.data_ptr(), self.d_pos_off.data_ptr(), self.d_pos.data_ptr() if self.d_pos is not None else None, self.n_pos)


def _check(ctx, b, D=1, flags=0, sel=None, m=None, seed=0):
    """One call with rec_len and one without, on raw pointers, against hash_oracle.  sel = (streams, records) or None for
    all-records mode over m entries (default sum(count) + n).  -> (hash as int64, L) as numpy."""
    import torch
    if sel is not None:
        si, sk = np.asarray(sel[0], dtype=np.int64), np.asarray(sel[1], dtype=np.int64)
        m = len(si)
        d_ss, d_sr = _dev(si, torch.int32), _dev(sk)
        sel_ptrs = (d_ss.data_ptr(), d_sr.data_ptr())
        want, L = hash_oracle.hash_take(b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, D, flags, seed, si & 0xFFFFFFFF, sk)
    else:
        if m is None:
            m = int(np.sum(b.count)) + b.n
        sel_ptrs = (None, None)
        want, L = hash_oracle.hash_take(b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, D, flags, seed, m=m)
    tag = (D, flags, sel is not None, m, seed)
    args = b.head() + (D, flags) + sel_ptrs + (m, seed)
    for with_len in (True, False):
        h = torch.full((m + SPARE,), SENT, dtype=torch.int64, device="cuda:0")
        rec_len = torch.full((m + SPARE,), SENT, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        ctx.hash_batch_device(*args, h.data_ptr(), rec_len.data_ptr() if with_len else None)
        got, got_len = h.cpu().numpy(), rec_len.cpu().numpy()
        assert (got[m:] == SENT).all() and (got_len[m:] == SENT).all(), tag
        if with_len:
            bad = np.flatnonzero(got_len[:m] != L)
            assert bad.size == 0, ("rec_len", tag, bad[:8].tolist(), got_len[bad[:8]].tolist(), L[bad[:8]].tolist())
        else:
            assert (got_len == SENT).all(), tag
        bad = np.flatnonzero(got[:m] != want)
        assert bad.size == 0, ("hash", with_len, tag, bad[:8].tolist(), L[bad[:8]].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert (want[L == 0] == 0).all()
    return want, L


def _text(rng, size, every=40, crlf=0.25):
    """`size` lower-case letters with a line feed every `every` bytes on average, a quarter of them behind a CR"""
    s = rng.integers(97, 123, size).astype(np.uint8)
    lf = np.flatnonzero(rng.random(size) < 1.0 / every)
    s[lf] = 10
    cr = lf[(rng.random(lf.size) < crlf) & (lf > 0)] - 1
    s[cr] = 13
    return s


def _binary(rng, size):
    """`size` bytes of every value but the line feed"""
    s = rng.integers(0, 256, size).astype(np.uint8)
    s[s == 10] = 11
    return s


def _ragged(seed, top):
    """64 streams of log-uniform lengths, 0 .. top, empty ones included, in slots with slack (CRs and LFs: a stray byte shows)"""
    rng = np.random.default_rng(seed)
    lens = np.floor(np.exp(rng.uniform(0, np.log(top), 64))).astype(np.int64)
    lens[[5, 17, 63]] = 0
    lens[40] = top
    slots = lens + rng.integers(0, 40, 64)
    offs = np.cumsum(slots) - slots
    host = np.resize(np.array([13, 10], dtype=np.uint8), int(slots.sum())).copy()
    for o, ln in zip(offs, lens):
        host[o:o + ln] = _text(rng, int(ln))
    return Batch(host, offs, lens)


@pytest.fixture(scope="module")
def ragged():
    return _ragged(16, 65536)


# 1 -------------------------------------------------------------------------------------------------------------------------------
def test_check_values_through_both_wrappers_and_the_raw_call(ctx):
    """The contract's table: its records in one stream split at "\\n" (the one that holds a line feed is a stream of its own, whole),
    three seeds, through the raw call, hash_batch_device and hash_batch."""
    import torch
    recs = [b"a", b"a\0", b"abcd", b"abcde", hash_oracle.R256[:10] + hash_oracle.R256[11:], b""]
    s0 = b"\n".join(recs)  # (bytes 0..255 cannot sit between line feeds: stream 2 holds them whole)
    s1, s2 = b"hello, world\n", hash_oracle.R256
    host = _np(b"\r\r\r" + s0 + b"\r" + s1 + b"\r\r" + s2 + b"\r")
    offs = [3, 3 + len(s0) + 1, 3 + len(s0) + 1 + len(s1) + 2]
    lines = Batch(host, offs[:1], [len(s0)])
    whole = Batch(host, offs, [len(s0), len(s1), len(s2)], positions=(np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int64)))
    for seed, (K, table) in hash_oracle.CHECK.items():
        want = [hash_oracle.as_i64(table[r]) if r in table else None for r in recs]
        got, L = _check(ctx, lines, 1, NO_DELIM, seed=seed)
        assert L.tolist() == [len(r) for r in recs]
        assert [g for g, w in zip(got.tolist(), want) if w is not None] == [w for w in want if w is not None]
        got, L = _check(ctx, whole, 1, 0, seed=seed)
        assert got.tolist()[1:] == [hash_oracle.as_i64(table[s1]), hash_oracle.as_i64(table[s2])] and L.tolist()[1:] == [13, 256]
        # the wrapper on tensors, and the raw call
        key, rec_len = ctx.hash_batch(lines.arena, lines.d_off, lines.d_len, lines.d_count, lines.d_pos_off, lines.d_pos, keep_delim=False,
                                      seed=seed, want_len=True)
        assert rec_len.cpu().tolist() == [len(r) for r in recs]
        assert [g for g, w in zip(key.cpu().tolist(), want) if w is not None] == [w for w in want if w is not None]
        none = torch.zeros(0, dtype=torch.int64, device="cuda:0")
        key = ctx.hash_batch(whole.arena, whole.d_off, whole.d_len, whole.d_count, whole.d_pos_off, none, seed=seed)
        assert key.dtype == torch.int64 and key.cpu().tolist()[1:] == [hash_oracle.as_i64(table[s1]), hash_oracle.as_i64(table[s2])]
        h = torch.full((3,), SENT, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        assert ctx._lib.brx_hash_batch(ctx._h, *whole.head(), 1, 0, None, None, 3, seed, h.data_ptr(), None, None) == 0
        assert h.cpu().tolist() == key.cpu().tolist()


# 2 -------------------------------------------------------------------------------------------------------------------------------
def test_every_length_at_every_phase(ctx):
    """One stream of records of every length 0 .. 2 * LONG + 40 in order, delimiters not kept, placed at each source phase 0 .. 15:
    every L mod 16 and mod 4, the edge between the two paths, the edge of a row, both paths."""
    rng = np.random.default_rng(2)
    top = 2 * LONG + 40
    one = np.concatenate([np.concatenate([_binary(rng, ln), _np(b"\n")]) for ln in range(top + 1)])
    slot = (one.size + 64) // 16 * 16
    offs = [p * slot + p for p in range(16)]
    host = np.full(16 * slot + 32, 13, dtype=np.uint8)
    for o in offs:
        host[o:o + one.size] = one
    b = Batch(host, offs, [one.size] * 16)
    got, L = _check(ctx, b, 1, NO_DELIM, seed=0x1234567890ABCDEF)
    assert L.tolist() == (list(range(top + 1)) + [0]) * 16
    g = got.reshape(16, top + 2)
    assert (g == g[0]).all()  # the phase does not show
    assert np.unique(g[0]).size == top + 1  # (and no two of these lengths share a key: the empty record comes twice)


# 3 -------------------------------------------------------------------------------------------------------------------------------
def test_equal_bytes_equal_hash(ctx):
    """The same records of 1, 15, 16, 17 and 1500 bytes in 16 streams, stream p at an address with phase p."""
    rng = np.random.default_rng(3)
    one = np.concatenate([np.concatenate([_binary(rng, ln - 1), _np(b"\n")]) for ln in (1, 15, 16, 17, 1500)])
    offs = [p * 1600 + p for p in range(16)]
    host = np.full(16 * 1600 + 32, 13, dtype=np.uint8)
    for o in offs:
        host[o:o + one.size] = one
    b = Batch(host, offs, [one.size] * 16)
    for flags, lens in ((0, [1, 15, 16, 17, 1500, 0]), (NO_DELIM, [0, 14, 15, 16, 1499, 0])):
        got, L = _check(ctx, b, 1, flags, seed=3)
        assert L.tolist() == lens * 16
        g = got.reshape(16, 6)
        assert (g == g[0]).all() and np.unique(g[0]).size == 5 + (flags == 0)


# 4 -------------------------------------------------------------------------------------------------------------------------------
def test_more_long_records_than_lanes(ctx):
    """70 records of 1100 .. 1169 bytes, then 200 short ones: the wave's loop runs 64 times in the first wave, which has long records
    only, and 6 times in the second.  Then long records at entries 63, 64, 255 and 256, the ends of a wave and of a workgroup."""
    rng = np.random.default_rng(4)
    lens = list(range(1100, 1170)) + rng.integers(0, 60, 200).tolist()
    s = np.concatenate([np.concatenate([_binary(rng, ln), _np(b"\n")]) for ln in lens])
    b = Batch(np.concatenate([_np(b"\r\r\r\r\r"), s, _np(b"\r")]), [5], [s.size])
    got, L = _check(ctx, b, 1, NO_DELIM, seed=4)
    assert L.tolist() == lens + [0]
    lens = rng.integers(0, 90, 300)
    lens[[63, 64, 255, 256]] = [LONG, 3 * LONG + 7, 2 * LONG - 1, LONG + 16]
    s = np.concatenate([np.concatenate([_binary(rng, ln), _np(b"\n")]) for ln in lens])
    b = Batch(np.concatenate([_np(b"\r"), s]), [1], [s.size])
    got, L = _check(ctx, b, 1, NO_DELIM, seed=M64)
    assert L.tolist() == lens.tolist() + [0]
    _check(ctx, b, 1, 0, seed=5)


# 5 -------------------------------------------------------------------------------------------------------------------------------
def test_whole_streams(ctx, ragged):
    """count = 0, n_pos = 0, all-records mode, m = n: entry i is the whole of stream i -- rows with a partial last row and unit."""
    zero = np.zeros(64, dtype=np.int64)
    b = Batch(ragged.host, ragged.offs, ragged.lens, positions=(zero, zero, np.zeros(0, dtype=np.int64)))
    got, L = _check(ctx, b, 1, 0, m=64, seed=55)
    assert L.tolist() == ragged.lens.tolist() and (got[[5, 17, 63]] == 0).all()
    _check(ctx, b, 1, NO_DELIM | TRIM_CR, m=64, seed=56)


# 6 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
def test_shuffled_selection_with_duplicates(ctx, ragged, flags):
    """6000 draws with repeats from the records of 64 ragged streams, out-of-range streams and records among them: those give hash 0
    and rec_len 0.  Then all-records mode with m beyond sum(count) + n."""
    rng = np.random.default_rng(6 + flags)
    m = 6000
    si = rng.integers(0, 64, m)
    sk = (rng.random(m) * (ragged.count[si] + 1)).astype(np.int64)
    bad = rng.choice(m, 200, replace=False)
    si[bad[:100]] = rng.integers(64, 70, 100)
    si[bad[:10]] = 0xFFFFFFFF
    sk[bad[100:]] = ragged.count[si[bad[100:]]] + rng.integers(1, 4, 100)
    sk[bad[100:110]] = -1  # 2^64 - 1
    got, L = _check(ctx, ragged, 1, flags, sel=(si, sk), seed=60 + flags)
    assert (L[bad] == 0).all() and (got[bad] == 0).all() and L.sum() > 100000
    total = int(ragged.count.sum()) + 64
    got, L = _check(ctx, ragged, 1, flags, m=total + 9, seed=61)
    assert (L[total:] == 0).all() and (got[total:] == 0).all()


# 7 -------------------------------------------------------------------------------------------------------------------------------
def test_flags_and_two_byte_delimiters(ctx):
    """The three flag combinations on CRLF text: TRIM_CR changes the hash exactly where the record ends in a CR.  Then delim_len 2
    with the device's brx_find_batch positions: "\\r\\n", and "\\n\\n" in "\\n\\n\\n\\n", whose overlapping occurrences give clamped records."""
    rng = np.random.default_rng(7)
    text = _text(rng, 20000, every=30, crlf=0.6)
    streams = [text, _np(b"\n\n\n\n"), _np(b"a\r\nb\r\n\r\nc")]
    offs = np.cumsum([3] + [s.size + 3 for s in streams[:-1]])
    host = np.resize(_np(b"\r\n"), int(offs[-1] + streams[-1].size + 2)).copy()
    for o, s in zip(offs, streams):
        host[o:o + s.size] = s
    lens = [s.size for s in streams]
    b = Batch(host, offs, lens)
    kept, L0 = _check(ctx, b, 1, 0, seed=7)
    plain, L1 = _check(ctx, b, 1, NO_DELIM, seed=7)
    trimmed, L3 = _check(ctx, b, 1, NO_DELIM | TRIM_CR, seed=7)
    assert ((plain != trimmed) == (L1 != L3)).all() and (L1 != L3).sum() > 100 and (L1 == L3).sum() > 100
    assert ((kept != plain) == (L0 != L1)).all() and (L0 == L1).sum() == 3  # (only the three trailing records have no delimiter to lose)
    for needle in (b"\r\n", b"\n\n"):
        count, pos_off, pos = ctx.find_batch(b.arena, b.d_off, b.d_len, needle)
        f = Batch(host, offs, lens, positions=(count.cpu().numpy(), pos_off.cpu().numpy(), pos.cpu().numpy()))
        if needle == b"\n\n":
            assert f.pos[f.pos_off[1]:f.pos_off[1] + f.count[1]].tolist() == [0, 1, 2]
        for flags in FLAGS:
            got, L = _check(ctx, f, 2, flags, seed=70 + flags)
        key = ctx.hash_batch(f.arena, f.d_off, f.d_len, count, pos_off, pos, delim_len=2, keep_delim=False, trim_cr=True, seed=70 + FLAGS[-1])
        assert key.cpu().tolist() == got.tolist()
        first = int(f.pos_off[2]) + 2  # "a\r\nb\r\n\r\nc"
        if needle == b"\r\n":
            assert L[first:first + 4].tolist() == [1, 1, 0, 1]


# 8 -------------------------------------------------------------------------------------------------------------------------------
def test_stale_positions(ctx):
    """pos entries above len (2^62, 2^64 - 1), entries in decreasing order, n_pos smaller than sum(count), m beyond sum(count) + n:
    the hashes of the clamped records.  (Streams of up to 6 KiB: a garbage position makes records of up to a stream's length, on
    both paths, and the oracle walks every one of them word by word.)"""
    rng = np.random.default_rng(12)
    ragged = _ragged(8, 6144)
    pos = ragged.pos.copy()
    j = rng.choice(pos.size, pos.size // 4, replace=False)
    third = j.size // 3
    pos[j[:third]] = 1 << 62
    pos[j[third:2 * third]] = -1
    pos[j[2 * third:]] = rng.integers(0, 7000, j.size - 2 * third)
    pos[100:200] = pos[100:200][::-1].copy()
    b = Batch(ragged.host, ragged.offs, ragged.lens, positions=(ragged.count, ragged.pos_off, pos))
    m = int(b.count.sum()) + 64
    for flags in FLAGS:
        _check(ctx, b, 1, flags, seed=80 + flags)
    _check(ctx, b, 16, 0, m=m + 5, seed=83)
    b.n_pos = pos.size // 2
    _check(ctx, b, 1, NO_DELIM | TRIM_CR, seed=84)
    b.n_pos = 0
    got, L = _check(ctx, b, 1, 0, sel=(rng.integers(0, 64, 500), rng.integers(0, 3, 500)), seed=85)
    assert L.sum() > 0


# 9 -------------------------------------------------------------------------------------------------------------------------------
def test_streams_on_the_first_and_the_last_byte_of_the_arena(ctx):
    """Stream 0 starts on the arena's first byte, stream 1 ends on its last: the short records there are loaded by the byte (a 16-byte
    load would leave the arena; tools/hash_emu.cpp is the check that none does).  Then an arena of one byte."""
    s0, s1 = b"ab\ncdefg\r\n", b"0123456789abcdefXYZ\n\nq\nrs\r\nt\r"
    b = Batch(_np(s0 + b"\r" * 5 + s1), [0, len(s0) + 5], [len(s0), len(s1)])
    for flags in FLAGS:
        got, L = _check(ctx, b, 1, flags, seed=9)
    assert L.tolist() == [2, 5, 0, 19, 0, 1, 2, 1]
    _check(ctx, b, 1, 0, sel=([1, 1, 0, 1], [4, 3, 0, 4]), seed=9)
    rng = np.random.default_rng(9)
    long_last = np.concatenate([_np(b"x\n"), _binary(rng, LONG + 5)])  # a long record up to the arena's last byte, too
    _check(ctx, Batch(long_last, [0], [long_last.size]), 1, NO_DELIM, seed=9)
    tiny = Batch(_np(b"\n"), [0], [1])
    got, L = _check(ctx, tiny, 1, 0, seed=9)
    assert L.tolist() == [1, 0] and got.tolist() == [hash_oracle.as_i64(hash_oracle.hash_direct(b"\n", 9)), 0]


# 10 ------------------------------------------------------------------------------------------------------------------------------
def test_rec_len_is_what_take_size_mode_writes(ctx, ragged):
    import torch
    rng = np.random.default_rng(10)
    si, sk = rng.integers(0, 66, 3000), rng.integers(0, 40, 3000)
    d_ss, d_sr = _dev(si, torch.int32), _dev(sk)
    for flags in FLAGS:
        for sel, m in (((None, None), int(ragged.count.sum()) + 64 + 3), ((d_ss.data_ptr(), d_sr.data_ptr()), 3000)):
            args = ragged.head() + (1, flags) + sel + (m,)
            a, c = (torch.full((m + SPARE,), SENT, dtype=torch.int64, device="cuda:0") for _ in range(2))
            h1, h2 = (torch.full((m + SPARE,), SENT, dtype=torch.int64, device="cuda:0") for _ in range(2))
            torch.cuda.synchronize()
            ctx.take_batch_device(*args, a.data_ptr())
            ctx.hash_batch_device(*args, 10, h1.data_ptr(), c.data_ptr())
            ctx.hash_batch_device(*args, 10, h2.data_ptr(), None)
            assert torch.equal(a, c) and torch.equal(h1, h2) and (h1[m:] == SENT).all()


# 11 ------------------------------------------------------------------------------------------------------------------------------
def test_enqueued_behind_the_index_pass(ctx, ragged):
    """brx_index_set_batch in fill mode and brx_hash_batch on a caller's stream, nothing in between."""
    import torch
    s = torch.cuda.Stream(device="cuda:0")
    want, L = hash_oracle.hash_take(ragged.host, ragged.offs, ragged.lens, ragged.count, ragged.pos_off, ragged.pos, ragged.n_pos, 1, NO_DELIM, 11)
    m = len(L)
    count = torch.full((64,), SENT, dtype=torch.int64, device="cuda:0")
    pos = torch.full((ragged.n_pos,), SENT, dtype=torch.int64, device="cuda:0")
    h = torch.full((m,), SENT, dtype=torch.int64, device="cuda:0")
    rec_len = torch.full((m,), SENT, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    head = (ragged.arena.data_ptr(), ragged.d_off.data_ptr(), ragged.d_len.data_ptr(), 64, int(ragged.arena.numel()))
    ctx.index_set_batch_device(b"\n", 0, 0, 3, *head, count.data_ptr(), None, ragged.d_pos_off.data_ptr(), pos.data_ptr(), None, ragged.n_pos,
                               hip_stream=s.cuda_stream)
    ctx.hash_batch_device(*head, count.data_ptr(), ragged.d_pos_off.data_ptr(), pos.data_ptr(), ragged.n_pos, 1, NO_DELIM, None, None, m, 11,
                          h.data_ptr(), rec_len.data_ptr(), hip_stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(pos.cpu().numpy(), ragged.pos) and np.array_equal(count.cpu().numpy(), ragged.count)
    assert np.array_equal(rec_len.cpu().numpy(), L) and np.array_equal(h.cpu().numpy(), want)


# 12 ------------------------------------------------------------------------------------------------------------------------------
def test_exact_deduplication_end_to_end(ctx):
    """64 streams of short lines drawn with many repeats from a pool of about 3000 distinct ones: index -> hash -> torch.unique ->
    the first entry of each key -> take_batch in pairs mode returns exactly the set of distinct lines."""
    import torch
    rng = np.random.default_rng(12)
    pool = sorted(set(bytes(rng.integers(97, 123, int(rng.integers(0, 60))).astype(np.uint8)) for _ in range(3000)))
    streams = [b"".join(pool[i] + (b"\r\n" if rng.integers(0, 3) == 0 else b"\n") for i in rng.integers(0, len(pool), int(rng.integers(0, 600))))
               for _ in range(64)]
    lens = np.array([len(s) for s in streams], dtype=np.int64)
    slots = lens + rng.integers(0, 30, 64)
    offs = np.cumsum(slots) - slots
    host = np.full(int(slots.sum()) + 1, 13, dtype=np.uint8)
    for o, s in zip(offs, streams):
        host[o:o + len(s)] = _np(s)
    lines = set()
    for s in streams:
        lines.update(ln.rstrip(b"\r") if ln.endswith(b"\r") else ln for ln in s.split(b"\n"))  # (the trailing record is empty)
    seed = 2026
    # a condition on the input, from the oracle alone: distinct lines, distinct keys under this seed
    assert len(set(hash_oracle.hash_direct(ln, seed) for ln in lines)) == len(lines)
    arena, d_off, d_len = _dev(host), _dev(offs), _dev(lens)
    count, _, pos_off, pos, _ = ctx.index_set_batch(arena, d_off, d_len, delims=b"\n", no_quote=True, no_escape=True)
    key = ctx.hash_batch(arena, d_off, d_len, count, pos_off, pos, keep_delim=False, trim_cr=True, seed=seed)
    assert int(key.numel()) == int(count.sum().item()) + 64
    uniq, inverse = torch.unique(key, return_inverse=True)
    assert int(uniq.numel()) == len(lines)
    j = torch.arange(key.numel(), device=key.device)
    first = torch.full_like(uniq, key.numel()).scatter_reduce_(0, inverse, j, "amin")
    keys = pos_off + torch.arange(64, device=key.device)  # entry j of all-records mode is record j - keys[i] of stream i
    stream_of = torch.searchsorted(keys, first, right=True) - 1
    rec_of = first - keys[stream_of]
    dst, dst_off, rec_len = ctx.take_batch(arena, d_off, d_len, count, pos_off, pos, sel_stream=stream_of, sel_rec=rec_of,
                                           keep_delim=False, trim_cr=True)
    data, o, ln = dst.cpu().numpy(), dst_off.cpu().tolist(), rec_len.cpu().tolist()
    got = [bytes(data[a:a + b]) for a, b in zip(o, ln)]
    assert len(got) == len(lines) and set(got) == lines


# 13 ------------------------------------------------------------------------------------------------------------------------------
def test_an_empty_selection_and_the_refusals_on_a_live_context(ctx):
    """m = 0: BRX_SUCCESS and nothing launched, raw and through the wrapper; the refusals leave the context working."""
    import torch
    from brotli_rs_amd import brx
    b = Batch(_np(b"ab\ncd\n"), [0], [6])
    h = torch.full((4,), SENT, dtype=torch.int64, device="cuda:0")
    rec_len = torch.full((4,), SENT, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert ctx._lib.brx_hash_batch(ctx._h, *b.head(), 1, 0, None, None, 0, 0, h.data_ptr(), rec_len.data_ptr(), None) == 0
    ctx.synchronize()
    assert h.cpu().tolist() == [SENT] * 4 and rec_len.cpu().tolist() == [SENT] * 4
    none = torch.zeros(0, dtype=torch.int64, device="cuda:0")
    k, r = ctx.hash_batch(b.arena, b.d_off, b.d_len, b.d_count, b.d_pos_off, b.d_pos, sel_stream=none.to(torch.int32), sel_rec=none, want_len=True)
    assert k.numel() == 0 and r.numel() == 0
    with pytest.raises(brx.BrxError, match="brx_hash_batch: BRX_TAKE_TRIM_CR"):
        ctx.hash_batch_device(*b.head(), 1, TRIM_CR, None, None, 3, 0, h.data_ptr())
    with pytest.raises(brx.BrxError, match="brx_hash_batch: delim_len"):
        ctx.hash_batch_device(*b.head(), 17, 0, None, None, 3, 0, h.data_ptr())
    with pytest.raises(brx.BrxError, match="brx_hash_batch: hash is NULL"):
        ctx.hash_batch_device(*b.head(), 1, 0, None, None, 3, 0, None)
    with pytest.raises(brx.BrxError, match="trim_cr"):
        ctx.hash_batch(b.arena, b.d_off, b.d_len, b.d_count, b.d_pos_off, b.d_pos, trim_cr=True)
    got, L = _check(ctx, b, seed=13)
    assert L.tolist() == [3, 3, 0] and got[0] == hash_oracle.as_i64(hash_oracle.hash_direct(b"ab\n", 13))
