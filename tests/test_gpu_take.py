"""brx_take_batch (include/brx.h, brx_take.hip): the selected records of the decoded streams of a batch, as lengths (size mode) or as bytes
in a destination (fill mode).  Every expected value comes from tests/take_oracle.py.  Every destination is pre-filled with a sentinel
byte and carries 64 spare bytes behind `total` (and its phase in front): each byte that the rule does not write must still hold the
sentinel.  In-process, one context."""
import numpy as np
import pytest

import brx_knobs
import take_oracle

pytestmark = pytest.mark.gpu

CHUNK = 4096  # BRX_TAKE_CHUNK (brx_take.h): what one wavefront owns of the destination; the tests only choose lengths around it
FILL = 0xEE   # the destinations' sentinel (no text below holds it)
SPARE = 64
NO_DELIM, TRIM_CR = 1, 2
FLAGS = (0, NO_DELIM, NO_DELIM | TRIM_CR)
C = b'a,"b,c\n",d\r\ne,"f""g",h\n"x'  # text C of brx_index_set_batch's contract


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
        self.upload()

    def upload(self):
        self.arena = _dev(self.host)
        self.d_off, self.d_len = _dev(self.offs), _dev(self.lens)
        self.d_count, self.d_pos_off = _dev(np.asarray(self.count, dtype=np.int64)), _dev(np.asarray(self.pos_off, dtype=np.int64))
        self.d_pos = _dev(np.asarray(self.pos, dtype=np.int64)) if len(self.pos) else None

    def head(self):
        return (self.arena.data_ptr(), self.d_off.data_ptr(), self.d_len.data_ptr(), self.n, int(self.arena.numel()),
                self.d_count.data_ptr(), self.d_pos_off.data_ptr(), self.d_pos.data_ptr() if self.d_pos is not None else None, self.n_pos)


def _check(ctx, b, D=1, flags=0, sel=None, m=None, stride=None, total=None, phase=0):
    """Size mode, then fill mode with rec_len written again, on raw pointers, against take_oracle.  sel = (streams, records) or None
    for all-records mode over m entries (default sum(count) + n).  stride None: packed rooms.  total None: all of it.
    -> (L, dst_off, the destination's bytes [0, total)) as numpy."""
    import torch
    if sel is not None:
        si, sk = np.asarray(sel[0], dtype=np.int64), np.asarray(sel[1], dtype=np.int64)
        m = len(si)
        d_ss, d_sr = _dev(si, torch.int32), _dev(sk)
        sel_ptrs = (d_ss.data_ptr(), d_sr.data_ptr())
        src, L = take_oracle.records_vec(b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, D, flags, si & 0xFFFFFFFF, sk)
    else:
        if m is None:
            m = int(np.sum(b.count)) + b.n
        sel_ptrs = (None, None)
        src, L = take_oracle.take_vec(b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, D, flags, m=m)
    tag = (D, flags, sel is not None, m, stride, total, phase)
    rec_len = torch.full((m + 8,), -7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    args = b.head() + (D, flags) + sel_ptrs + (m,)
    ctx.take_batch_device(*args, rec_len.data_ptr())
    got = rec_len.cpu().numpy()
    assert (got[m:] == -7).all(), tag
    bad = np.flatnonzero(got[:m] != L)
    assert bad.size == 0, ("rec_len", tag, bad[:8].tolist(), got[bad[:8]].tolist(), L[bad[:8]].tolist())
    if stride is None:
        dst_off = np.cumsum(L) - L
        full = int(L.sum())
    else:
        dst_off = np.arange(m, dtype=np.int64) * stride
        full = m * stride
    total = full if total is None else total
    want = take_oracle.fill_vec(b.host, src, L, dst_off, total, np.full(phase + total + SPARE, FILL, dtype=np.uint8)[phase:])
    buf = torch.full((phase + total + SPARE,), FILL, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    d_dst_off = _dev(dst_off) if m else torch.zeros(1, dtype=torch.int64, device="cuda:0")
    rec_len.fill_(-7)
    torch.cuda.synchronize()
    ctx.take_batch_device(*args, rec_len.data_ptr(), d_dst_off.data_ptr(), buf.data_ptr() + phase, total)
    got = rec_len.cpu().numpy()
    assert (got[m:] == -7).all() and (got[:m] == L).all(), ("rec_len written by fill mode", tag)
    out = buf.cpu().numpy()
    assert (out[:phase] == FILL).all(), ("in front of dst", tag)
    assert (out[phase + total:] == FILL).all(), ("at or behind total", tag)
    out = out[phase:]
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, ("dst", tag, bad[:8].tolist(), out[bad[:8]].tolist(), want[bad[:8]].tolist())
    return L, dst_off, out[:total]


def _records(data, dst_off, L):
    return [bytes(data[o:o + ln]) for o, ln in zip(dst_off, L)]


def _text(rng, size, every=40, crlf=0.25):
    """`size` lower-case letters with a line feed every `every` bytes on average, a quarter of them behind a CR"""
    s = rng.integers(97, 123, size).astype(np.uint8)
    lf = np.flatnonzero(rng.random(size) < 1.0 / every)
    s[lf] = 10
    cr = lf[(rng.random(lf.size) < crlf) & (lf > 0)] - 1
    s[cr] = 13
    return s


@pytest.fixture(scope="module")
def ragged():
    """64 streams of log-uniform lengths, 0 .. 64 KiB, empty ones included, in slots with slack (CRs and LFs: a stray byte shows)"""
    rng = np.random.default_rng(16)
    lens = np.floor(np.exp(rng.uniform(0, np.log(65536), 64))).astype(np.int64)
    lens[[5, 17, 63]] = 0
    lens[40] = 65536
    slots = lens + rng.integers(0, 40, 64)
    offs = np.cumsum(slots) - slots
    host = np.resize(np.array([13, 10], dtype=np.uint8), int(slots.sum())).copy()
    for o, ln in zip(offs, lens):
        host[o:o + ln] = _text(rng, int(ln))
    return Batch(host, offs, lens)


# 1 -------------------------------------------------------------------------------------------------------------------------------
WANT_C = {0: [b"a,", b'"b,', b"c\n", b'",', b"d\r", b"\n", b"e,", b'"f""g",', b"h\n", b'"x'],
          NO_DELIM: [b"a", b'"b', b"c", b'"', b"d", b"", b"e", b'"f""g"', b"h", b'"x'],
          NO_DELIM | TRIM_CR: [b"a", b'"b', b"c", b'"', b"d", b"", b"e", b'"f""g"', b"h", b'"x']}


def test_check_values_through_both_wrappers_and_the_raw_call(ctx):
    """Text C of brx_index_set_batch's contract (25 bytes, delims ",\\n\\r", both switches off): positions from the device, the ten
    records written out by hand under each flag combination; and at "\\n" alone, where TRIM_CR has a CR to drop."""
    import torch
    arena = _dev(_np(b"\r\n" + C + b"\r\n"))
    offs, lens = _dev(np.array([2], dtype=np.int64)), _dev(np.array([25], dtype=np.int64))
    count, _, pos_off, pos, _ = ctx.index_set_batch(arena, offs, lens, delims=b",\n\r", no_quote=True, no_escape=True)
    assert pos.cpu().tolist() == [1, 4, 6, 8, 10, 11, 13, 20, 22]
    for flags in FLAGS:
        dst, dst_off, rec_len = ctx.take_batch(arena, offs, lens, count, pos_off, pos, keep_delim=not flags & NO_DELIM,
                                               trim_cr=bool(flags & TRIM_CR))
        assert _records(dst.cpu().numpy(), dst_off.cpu().tolist(), rec_len.cpu().tolist()) == WANT_C[flags]
        assert int(dst.numel()) == sum(len(r) for r in WANT_C[flags])
    # pairs mode through the wrapper: the last record, the CR record twice, one out of range; rows of 4 bytes, the rest of a row zero
    ss, sr = _dev(np.array([0, 0, 0, 0, 1], dtype=np.int32)), _dev(np.array([9, 4, 4, 10, 0], dtype=np.int64))
    dst, dst_off, rec_len = ctx.take_batch(arena, offs, lens, count, pos_off, pos, sel_stream=ss, sel_rec=sr, stride=4)
    assert rec_len.cpu().tolist() == [2, 2, 2, 0, 0] and dst_off.cpu().tolist() == [0, 4, 8, 12, 16]
    assert bytes(dst.cpu().numpy()) == b'"x\0\0d\r\0\0d\r\0\0' + bytes(8)
    # the raw call and the device-pointer wrapper, held to the oracle and to the hand-written lists
    b = Batch(_np(b"\r\n" + C + b"\r\n"), [2], [25], positions=(count.cpu().numpy(), pos_off.cpu().numpy(), pos.cpu().numpy()))
    for flags in FLAGS:
        L, dst_off, data = _check(ctx, b, 1, flags)
        assert _records(data, dst_off, L) == WANT_C[flags]
    rec_len = torch.full((10,), -7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert ctx._lib.brx_take_batch(ctx._h, *b.head(), 1, NO_DELIM, None, None, 10, rec_len.data_ptr(), None, None, 0, None) == 0
    assert rec_len.cpu().tolist() == [len(r) for r in WANT_C[NO_DELIM]]
    lines = Batch(_np(b"\r\n" + C + b"\r\n"), [2], [25], delims=b"\n")
    L, dst_off, data = _check(ctx, lines, 1, NO_DELIM | TRIM_CR)
    assert _records(data, dst_off, L) == [b'a,"b,c', b'",d', b'e,"f""g",h', b'"x']


# 2 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [NO_DELIM, 0])
def test_5000_empty_lines(ctx, flags):
    """5000 x "\\n": with NO_DELIM every record is empty (nothing is written); with the delimiters kept 16 records share every unit and
    4096 entries start in one chunk, 64 windows of it.  Then the same entries in rooms of one byte each."""
    b = Batch(_np(b"x" + b"\n" * 5000 + b"x"), [1], [5000])
    L, _, data = _check(ctx, b, 1, flags, phase=3)
    assert len(L) == 5001 and int(L.sum()) == (0 if flags else 5000) and (data == 10).all()
    _check(ctx, b, 1, flags, stride=1, phase=9)


# 3 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", [0, 5])
def test_one_long_record_between_two_short_ones(ctx, phase):
    """"\\n", then 3 x CHUNK + 1 bytes, then "\\n": the long record is served by four or five waves independently."""
    rng = np.random.default_rng(3)
    body = rng.integers(97, 123, 3 * CHUNK).astype(np.uint8)
    s = np.concatenate([_np(b"\n"), body, _np(b"\n\n")])
    b = Batch(np.concatenate([_np(b"\r\r\r"), s, _np(b"\r")]), [3], [s.size])
    L, _, data = _check(ctx, b, 1, 0, phase=phase)
    assert L.tolist() == [1, 3 * CHUNK + 1, 1, 0] and bytes(data) == bytes(s)
    _check(ctx, b, 1, NO_DELIM, phase=phase)
    _check(ctx, b, 1, 0, sel=([0, 0, 0, 0], [2, 1, 0, 1]), phase=phase)


# 4 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dphase", range(16))
def test_every_phase_of_source_and_destination(ctx, dphase):
    """Records of 1, 15, 16, 17 and 33 bytes in 16 streams, stream p at an address with phase p; dst at phase `dphase`."""
    rng = np.random.default_rng(4)
    one = b"".join(bytes(rng.integers(97, 123, ln - 1).astype(np.uint8)) + b"\n" for ln in (1, 15, 16, 17, 33))
    offs = [p * 128 + p for p in range(16)]
    host = np.full(16 * 128 + 32, 13, dtype=np.uint8)
    for o in offs:
        host[o:o + len(one)] = _np(one)
    b = Batch(host, offs, [len(one)] * 16)
    L, _, _ = _check(ctx, b, 1, 0, phase=dphase)
    assert L.tolist() == [1, 15, 16, 17, 33, 0] * 16
    L, _, _ = _check(ctx, b, 1, NO_DELIM, phase=dphase)
    assert L.tolist() == [0, 14, 15, 16, 32, 0] * 16


# 5 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", [0, 1, 15])
def test_record_lengths_around_the_chunk(ctx, phase):
    """Packed at phase 0 the records end at 4096 (on a chunk's edge), 8191 (a byte in front of one), 12289 (a byte behind one), 16386,
    16387, 20481 and 24577; the other phases move every edge through the records."""
    rng = np.random.default_rng(5)
    want = [CHUNK, CHUNK - 1, CHUNK + 2, CHUNK + 1, 1, CHUNK - 2, CHUNK]
    s = np.concatenate([np.concatenate([rng.integers(97, 123, ln - 1).astype(np.uint8), _np(b"\n")]) for ln in want])
    b = Batch(np.concatenate([_np(b"\n"), s]), [1], [s.size])
    L, dst_off, data = _check(ctx, b, 1, 0, phase=phase)
    assert L.tolist() == want + [0] and bytes(data) == bytes(s)
    _check(ctx, b, 1, 0, stride=CHUNK, phase=phase)
    _check(ctx, b, 1, NO_DELIM, sel=([0] * 7, [6, 5, 4, 3, 2, 1, 0]), phase=phase)


# 6 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
def test_shuffled_selection_with_duplicates(ctx, ragged, flags):
    """6000 draws with repeats from the records of 64 ragged streams, out-of-range streams and records among them (they give 0)."""
    rng = np.random.default_rng(6 + flags)
    m = 6000
    si = rng.integers(0, 64, m)
    sk = (rng.random(m) * (ragged.count[si] + 1)).astype(np.int64)
    bad = rng.choice(m, 200, replace=False)
    si[bad[:100]] = rng.integers(64, 70, 100)
    si[bad[:10]] = 0xFFFFFFFF
    sk[bad[100:]] = ragged.count[si[bad[100:]]] + rng.integers(1, 4, 100)
    sk[bad[100:110]] = -1  # 2^64 - 1
    L, _, _ = _check(ctx, ragged, 1, flags, sel=(si, sk), phase=int(rng.integers(0, 16)))
    assert (L[bad] == 0).all() and L.sum() > 100000


# 7 -------------------------------------------------------------------------------------------------------------------------------
def test_all_records_packed_equal_the_compacted_batch(ctx, ragged):
    """All-records mode, delimiters kept, packed: the batch without its slack, byte for byte what brx_compact_batch writes."""
    import torch
    L, dst_off, data = _check(ctx, ragged, 1, 0, phase=7)
    total = int(ragged.lens.sum())
    assert data.size == total
    d_dst_off = _dev(np.cumsum(ragged.lens) - ragged.lens)
    compact = torch.full((total + SPARE,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.compact_batch_device(ragged.arena.data_ptr(), ragged.d_off.data_ptr(), ragged.d_len.data_ptr(), 64, compact.data_ptr(),
                             d_dst_off.data_ptr(), total)
    assert np.array_equal(compact.cpu().numpy()[:total], data)
    for flags in (NO_DELIM, NO_DELIM | TRIM_CR):
        _check(ctx, ragged, 1, flags, phase=flags)


# 8 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [8, 16, 100])
def test_rooms_of_a_fixed_stride(ctx, ragged, stride):
    """Every record in a row of its own: cut at the stride, the rest of a row untouched."""
    L, dst_off, data = _check(ctx, ragged, 1, NO_DELIM | TRIM_CR, stride=stride, phase=stride % 16)
    assert (L > stride).any() and (L < stride).any()
    rows = data.reshape(-1, stride)
    assert (rows[L < stride, -1] == FILL).all()  # (a short record's row keeps its last byte)
    _check(ctx, ragged, 1, 0, stride=stride, phase=1)


# 9 -------------------------------------------------------------------------------------------------------------------------------
def test_total_cut_to_half(ctx, ragged):
    """`total` at half of what the rooms need: nothing at or behind it is written (the entry across it is cut), rec_len is complete."""
    full = int(take_oracle.take_vec(ragged.host, ragged.offs, ragged.lens, ragged.count, ragged.pos_off, ragged.pos, ragged.n_pos, 1, 0)[1].sum())
    _check(ctx, ragged, 1, 0, total=full // 2, phase=11)
    _check(ctx, ragged, 1, 0, total=full // 2 + 5, phase=0)
    m = int(ragged.count.sum()) + 64
    _check(ctx, ragged, 1, NO_DELIM, stride=100, total=m * 50 + 33, phase=2)
    _check(ctx, ragged, 1, 0, total=0)


# 10 ------------------------------------------------------------------------------------------------------------------------------
def test_trim_cr(ctx):
    """A lone CR, a record ending in two CRs (one goes), the trailing record, mixed LF / CRLF text; CRs in the slack are never looked at."""
    streams = [b"\r", b"ab\r\r\ncd\r\n", b"x\ny\r", b"\r\n\r\n\n\r", b"", b"one\r\ntwo\nthree\r\nfour"]
    host, offs = [], []
    for s in streams:
        host.append(b"\r\r")
        offs.append(sum(len(h) for h in host))
        host.append(s)
    b = Batch(_np(b"".join(host) + b"\r"), offs, [len(s) for s in streams])
    L, dst_off, data = _check(ctx, b, 1, NO_DELIM | TRIM_CR, phase=13)
    assert _records(data, dst_off, L) == [b"", b"ab\r", b"cd", b"", b"x", b"y", b"", b"", b"", b"", b"", b"one", b"two", b"three", b"four"]
    L, dst_off, data = _check(ctx, b, 1, NO_DELIM)
    assert _records(data, dst_off, L)[:4] == [b"\r", b"ab\r\r", b"cd\r", b""]
    rng = np.random.default_rng(10)
    text = _text(rng, 30000, every=12, crlf=0.5)
    _check(ctx, Batch(np.concatenate([_np(b"\r"), text, _np(b"\r")]), [1], [text.size]), 1, NO_DELIM | TRIM_CR, phase=6)


# 11 ------------------------------------------------------------------------------------------------------------------------------
def test_two_byte_delimiters_from_find_batch(ctx):
    """delim_len 2 with the device's brx_find_batch positions: "\\r\\n" in CRLF text, and "\\n\\n" in "\\n\\n\\n\\n", whose overlapping
    occurrences (0, 1, 2) give clamped records."""
    rng = np.random.default_rng(11)
    text = _text(rng, 20000, every=30, crlf=0.6)
    streams = [text, _np(b"\n\n\n\n"), _np(b"a\r\nb\r\n\r\nc")]
    offs = np.cumsum([3] + [s.size + 3 for s in streams[:-1]])
    host = np.resize(_np(b"\r\n"), int(offs[-1] + streams[-1].size + 2)).copy()
    for o, s in zip(offs, streams):
        host[o:o + s.size] = s
    arena, d_off, d_len = _dev(host), _dev(offs.astype(np.int64)), _dev(np.array([s.size for s in streams], dtype=np.int64))
    for needle, stream, want in ((b"\r\n", 2, {0: [b"a\r\n", b"b\r\n", b"\r\n", b"c"], NO_DELIM: [b"a", b"b", b"", b"c"]}),
                                 (b"\n\n", 1, {0: [b"\n\n", b"\n", b"\n", b""], NO_DELIM: [b"", b"", b"", b""]})):
        count, pos_off, pos = ctx.find_batch(arena, d_off, d_len, needle)
        b = Batch(host, offs, [s.size for s in streams], positions=(count.cpu().numpy(), pos_off.cpu().numpy(), pos.cpu().numpy()))
        if needle == b"\n\n":
            assert b.pos[b.pos_off[1]:b.pos_off[1] + b.count[1]].tolist() == [0, 1, 2]
        for flags in FLAGS:
            L, dst_off, data = _check(ctx, b, 2, flags, phase=flags + 1)
            first = int(b.pos_off[stream]) + stream
            got = _records(data, dst_off[first:first + 4], L[first:first + 4])
            assert got == want[flags & NO_DELIM], (needle, flags)
        dst, dst_off, rec_len = ctx.take_batch(arena, d_off, d_len, count, pos_off, pos, delim_len=2, keep_delim=False)
        want_L = take_oracle.take_vec(host, offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, 2, NO_DELIM)[1]
        assert rec_len.cpu().tolist() == want_L.tolist() and int(dst.numel()) == int(want_L.sum())


# 12 ------------------------------------------------------------------------------------------------------------------------------
def test_stale_positions(ctx, ragged):
    """pos entries above len (2^62, 2^64 - 1), entries in decreasing order, n_pos smaller than sum(count), m beyond sum(count) + n:
    short or empty records, nothing outside the rooms."""
    rng = np.random.default_rng(12)
    pos = ragged.pos.copy()
    j = rng.choice(pos.size, pos.size // 4, replace=False)
    third = j.size // 3
    pos[j[:third]] = 1 << 62
    pos[j[third:2 * third]] = -1
    pos[j[2 * third:]] = rng.integers(0, 70000, j.size - 2 * third)
    pos[100:200] = pos[100:200][::-1].copy()
    b = Batch(ragged.host, ragged.offs, ragged.lens, positions=(ragged.count, ragged.pos_off, pos))
    m = int(b.count.sum()) + 64
    for flags in FLAGS:
        _check(ctx, b, 1, flags, phase=flags)
    _check(ctx, b, 16, 0, m=m + 5)
    b.n_pos = pos.size // 2
    _check(ctx, b, 1, NO_DELIM | TRIM_CR, phase=4)
    _check(ctx, b, 2, 0, stride=16)
    b.n_pos = 0
    L, _, _ = _check(ctx, b, 1, 0, sel=(rng.integers(0, 64, 500), rng.integers(0, 3, 500)))
    assert L.sum() > 0


# 13 ------------------------------------------------------------------------------------------------------------------------------
def test_streams_on_the_first_and_the_last_byte_of_the_arena(ctx):
    """Stream 0 starts on the arena's first byte, stream 1 ends on its last: the short records there are fetched by the byte (a
    16-byte load would leave the arena; tools/take_emu.cpp is the check that none does)."""
    s0, s1 = b"ab\ncdefg\r\n", b"0123456789abcdefXYZ\n\nq\nrs\r\nt\r"
    host = _np(s0 + b"\r" * 5 + s1)
    b = Batch(host, [0, len(s0) + 5], [len(s0), len(s1)])
    for flags in FLAGS:
        for phase in (0, 9):
            L, dst_off, data = _check(ctx, b, 1, flags, phase=phase)
    assert _records(data, dst_off, L) == [b"ab", b"cdefg", b"", b"0123456789abcdefXYZ", b"", b"q", b"rs", b"t"]
    _check(ctx, b, 1, 0, sel=([1, 1, 0, 1], [4, 3, 0, 4]), stride=3)
    tiny = Batch(_np(b"\n"), [0], [1])
    L, _, data = _check(ctx, tiny, 1, 0)
    assert L.tolist() == [1, 0] and bytes(data) == b"\n"


# 14 ------------------------------------------------------------------------------------------------------------------------------
def test_enqueued_behind_the_index_pass(ctx, ragged):
    """brx_index_set_batch in fill mode and brx_take_batch (size + fill in one call) on a caller's stream, nothing in between."""
    import torch
    s = torch.cuda.Stream(device="cuda:0")
    src, L = take_oracle.take_vec(ragged.host, ragged.offs, ragged.lens, ragged.count, ragged.pos_off, ragged.pos, ragged.n_pos, 1, NO_DELIM)
    m, total = len(L), int(L.sum())
    dst_off = np.cumsum(L) - L
    want = take_oracle.fill_vec(ragged.host, src, L, dst_off, total, np.full(total + SPARE, FILL, dtype=np.uint8))
    d_dst_off = _dev(dst_off)
    count = torch.full((64,), -7, dtype=torch.int64, device="cuda:0")
    pos = torch.full((ragged.n_pos,), -7, dtype=torch.int64, device="cuda:0")
    rec_len = torch.full((m,), -7, dtype=torch.int64, device="cuda:0")
    dst = torch.full((total + SPARE,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    head = (ragged.arena.data_ptr(), ragged.d_off.data_ptr(), ragged.d_len.data_ptr(), 64, int(ragged.arena.numel()))
    ctx.index_set_batch_device(b"\n", 0, 0, 3, *head, count.data_ptr(), None, ragged.d_pos_off.data_ptr(), pos.data_ptr(), None, ragged.n_pos,
                               hip_stream=s.cuda_stream)
    ctx.take_batch_device(*head, count.data_ptr(), ragged.d_pos_off.data_ptr(), pos.data_ptr(), ragged.n_pos, 1, NO_DELIM, None, None, m,
                          rec_len.data_ptr(), d_dst_off.data_ptr(), dst.data_ptr(), total, hip_stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(pos.cpu().numpy(), ragged.pos) and np.array_equal(count.cpu().numpy(), ragged.count)
    assert np.array_equal(rec_len.cpu().numpy(), L) and np.array_equal(dst.cpu().numpy(), want)


# 15 ------------------------------------------------------------------------------------------------------------------------------
def test_an_empty_selection_and_the_refusals_on_a_live_context(ctx):
    """m = 0: BRX_SUCCESS and nothing launched, in both modes and through the wrapper; the refusals leave the context working."""
    import torch
    from brotli_rs_amd import brx
    b = Batch(_np(b"ab\ncd\n"), [0], [6])
    rec_len = torch.full((4,), -7, dtype=torch.int64, device="cuda:0")
    dst = torch.full((16,), FILL, dtype=torch.uint8, device="cuda:0")
    dst_off = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    lib, h = ctx._lib, ctx._h
    assert lib.brx_take_batch(h, *b.head(), 1, 0, None, None, 0, rec_len.data_ptr(), None, None, 0, None) == 0
    assert lib.brx_take_batch(h, *b.head(), 1, 0, None, None, 0, rec_len.data_ptr(), dst_off.data_ptr(), dst.data_ptr(), 16, None) == 0
    ctx.synchronize()
    assert rec_len.cpu().tolist() == [-7] * 4 and (dst.cpu().numpy() == FILL).all()
    none = torch.zeros(0, dtype=torch.int64, device="cuda:0")
    d, o, r = ctx.take_batch(b.arena, b.d_off, b.d_len, b.d_count, b.d_pos_off, b.d_pos, sel_stream=none.to(torch.int32), sel_rec=none)
    assert d.numel() == 0 and o.numel() == 0 and r.numel() == 0
    with pytest.raises(brx.BrxError, match="brx_take_batch: BRX_TAKE_TRIM_CR"):
        ctx.take_batch_device(*b.head(), 1, TRIM_CR, None, None, 3, rec_len.data_ptr())
    with pytest.raises(brx.BrxError, match="brx_take_batch: delim_len"):
        ctx.take_batch_device(*b.head(), 17, 0, None, None, 3, rec_len.data_ptr())
    with pytest.raises(brx.BrxError, match="brx_take_batch: rec_len"):
        ctx.take_batch_device(*b.head(), 1, 0, None, None, 3, None)
    with pytest.raises(brx.BrxError, match="trim_cr"):
        ctx.take_batch(b.arena, b.d_off, b.d_len, b.d_count, b.d_pos_off, b.d_pos, trim_cr=True)
    L, dst_off, data = _check(ctx, b)
    assert _records(data, dst_off, L) == [b"ab\n", b"cd\n", b""]
