"""brx_index_set_batch (include/brx.h, brx_index_escaped.hip): the boundaries of the decoded streams of a batch at a set of delimiter
bytes, with optional quote and escape, counted and located on the device, with the byte that stands at each.  Every expected value
comes from set_oracle.vec (numpy on the CPU, held to the serial rule and to escaped_oracle by tests/test_index_set_abi.py).  In every
arena the slack of the slots and the gaps between them hold escape, quote and all the set's delimiters repeating: a kernel that reads
one byte too far, or lets a byte in front of a stream or behind it into its state, gets another result.  In-process, one context."""
import json
import os

import numpy as np
import pytest

import brx_knobs
import set_oracle
from test_gpu_index_escaped import _json_texts

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))
TILE = 65536  # one work item of the pass (brx_tiles.h); the tests below only choose lengths and addresses around it
SENTINEL = -0x0123456789ABCDEF
WHAT_SENTINEL = 0xA5
NL, CM, CR, QT, BS = 0x0A, 0x2C, 0x0D, 0x22, 0x5C
CSV = bytes([NL, CM, CR])
SETS = ((CSV, QT, BS),                                                   # (delims, quote, escape)
        (bytes([0x00, 0x01, 0x02]), 0xFF, 0x80),                         # the filler has to walk past several values
        (bytes([0x00, 0x7F, 0x80, 0xFF, 0x01, 0x02, 0x05, 0x06]), 0x03, 0x04))
NO_QUOTE, NO_ESCAPE = 1, 2  # BRX_INDEX_NO_QUOTE, BRX_INDEX_NO_ESCAPE


@pytest.fixture(scope="module")
def ctx():
    c = brx_knobs.context(0)
    yield c
    c.close()


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a))  # (a writable copy)
    return (t.to(dtype) if dtype is not None else t).to("cuda:0")


def _reference(host, offs, lens, delims, Q, E, flags=0):
    """-> (counts, open, exclusive prefix sum, all positions back to back, the bytes there)"""
    per = [set_oracle.vec(host[o:o + ln], delims, Q, E, bool(flags & NO_QUOTE), bool(flags & NO_ESCAPE)) for o, ln in zip(offs, lens)]
    counts = np.array([p.size for p, _, _ in per], dtype=np.int64)
    opens = np.array([o for _, _, o in per], dtype=np.int32)
    pos_off = np.zeros(len(per), dtype=np.int64)
    np.cumsum(counts[:-1], out=pos_off[1:])
    return (counts, opens, pos_off, np.concatenate([p for p, _, _ in per]) if per else np.zeros(0, dtype=np.int64),
            np.concatenate([w for _, w, _ in per]) if per else np.zeros(0, dtype=np.uint8))


def _filler(size, delims, Q, E):
    """escape, quote and all the set's delimiters repeating"""
    cyc = np.array([E, Q] + list(delims), dtype=np.uint8)
    return cyc[np.arange(size) % cyc.size]


def _check(ctx, host, arena, offs, lens, delims, Q, E, flags=0, q_arg=None, e_arg=None):
    """Count mode, then fill mode (pos_off by torch.cumsum from the device's counts; count and open written again; what next to pos),
    both on raw pointers, against the oracle.  q_arg / e_arg: what is passed for an argument that the flags switch off.
    -> (counts, open, positions, what) of the oracle."""
    import torch
    offs, lens = np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    n = len(lens)
    want_count, want_open, _, want_pos, want_what = _reference(host, offs, lens, delims, Q, E, flags)
    tag = (delims.hex(), hex(Q), hex(E), flags)
    d_off, d_len = _dev(offs), _dev(lens)
    count = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    open_ = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    args = (delims, Q if q_arg is None else q_arg, E if e_arg is None else e_arg, flags, arena.data_ptr(), d_off.data_ptr(),
            d_len.data_ptr(), n, arena.numel())
    ctx.index_set_batch_device(*args, count.data_ptr(), open_.data_ptr())
    got = count.cpu().numpy()
    bad = np.nonzero(got != want_count)[0]
    assert bad.size == 0, ("count", tag, [(int(offs[i]), int(lens[i]), int(got[i]), int(want_count[i])) for i in bad[:8]])
    got = open_.cpu().numpy()
    bad = np.nonzero(got != want_open)[0]
    assert bad.size == 0, ("open", tag, [(int(offs[i]), int(lens[i]), int(got[i]), int(want_open[i])) for i in bad[:8]])
    pos_off = torch.cumsum(count, 0) - count
    total = int(want_count.sum())
    pos = torch.full((total + 8,), SENTINEL, dtype=torch.int64, device="cuda:0")
    what = torch.full((total + 8,), WHAT_SENTINEL, dtype=torch.uint8, device="cuda:0")
    count2 = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    open2 = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.index_set_batch_device(*args, count2.data_ptr(), open2.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), what.data_ptr(), total)
    assert (count2.cpu().numpy() == want_count).all(), ("count written by fill mode", tag)
    assert (open2.cpu().numpy() == want_open).all(), ("open written by fill mode", tag)
    got_pos, got_what = pos.cpu().numpy(), what.cpu().numpy()
    assert (got_pos[total:] == SENTINEL).all() and (got_what[total:] == WHAT_SENTINEL).all(), tag
    bad = np.nonzero(got_pos[:total] != want_pos)[0]
    assert bad.size == 0, ("pos", tag, bad[:8].tolist(), got_pos[bad[:8]].tolist(), want_pos[bad[:8]].tolist())
    bad = np.nonzero(got_what[:total] != want_what)[0]
    assert bad.size == 0, ("what", tag, bad[:8].tolist(), got_what[bad[:8]].tolist(), want_what[bad[:8]].tolist())
    return want_count, want_open, want_pos, want_what


def _arena_tile_aligned(n_bytes):
    """A device arena and the offset in it of a 64 KiB aligned ADDRESS (tiles are cut in the address range)."""
    import torch
    arena = torch.empty(n_bytes + TILE, dtype=torch.uint8, device="cuda:0")
    return arena, (-arena.data_ptr()) % TILE


def test_check_values(ctx):
    """The contract's texts J (JSON Lines: a comma, a colon and a brace inside a string, an escaped quote, an escaped escape in front
    of a closing quote, an unterminated string that ends on an escape) and C (CSV with CRLF, a quoted line feed, a doubled quote, an
    unterminated field) at offset 1000 of a 4 KiB arena; empty streams at offset 0, at 1000 and at the arena's end.  Through
    index_set_batch and through the raw call."""
    offs = [1000, 1000, 0, 4096]
    for raw, delims, nq, ne, want_pos, want_what, want_open in (
            (set_oracle.J, set_oracle.J_SET, False, False, set_oracle.J_POS, set_oracle.J_WHAT, 3),
            (set_oracle.C, set_oracle.C_SET, False, True, set_oracle.C_POS_NO_ESCAPE, set_oracle.C_WHAT_NO_ESCAPE, 1),
            (set_oracle.C, set_oracle.C_SET, True, True, set_oracle.C_POS_PLAIN, bytes(set_oracle.C[j] for j in set_oracle.C_POS_PLAIN), 0)):
        text = np.frombuffer(raw, dtype=np.uint8)
        got = set_oracle.vec(text, delims, QT, BS, nq, ne)
        assert got[0].tolist() == want_pos and bytes(got[1]) == want_what and got[2] == want_open
        lens = [len(text), 0, 0, 0]
        d_off, d_len = _dev(np.array(offs, dtype=np.int64)), _dev(np.array(lens, dtype=np.int64))
        host = _filler(4096, delims, QT, BS)
        host[1000:1000 + len(text)] = text
        arena = _dev(host)
        k = len(want_pos)
        count, open_, pos_off, pos, what = ctx.index_set_batch(arena, d_off, d_len, delims=delims, quote=QT, escape=BS, no_quote=nq,
                                                               no_escape=ne)
        assert count.cpu().tolist() == [k, 0, 0, 0]
        assert open_.cpu().tolist() == [want_open, 0, 0, 0]
        assert pos_off.cpu().tolist() == [0, k, k, k]
        assert pos.cpu().tolist() == want_pos and bytes(what.cpu().tolist()) == want_what
        count, open_ = ctx.index_set_batch(arena, d_off, d_len, delims=delims, quote=QT, escape=BS, no_quote=nq, no_escape=ne,
                                           positions=False)
        assert count.cpu().tolist() == [k, 0, 0, 0] and open_.cpu().tolist() == [want_open, 0, 0, 0]
        _check(ctx, host, arena, offs, lens, delims, QT, BS, (NO_QUOTE if nq else 0) | (NO_ESCAPE if ne else 0))


EDGE_LENS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 65535, 65536, 65537, 131077)


def _other(delims, Q, E):
    return next(b for b in (0x78, 0x41, 0x42, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A) if b not in delims and b not in (Q, E))


def _draw(rng, ln, delims, Q, E, heavy):
    """ln bytes over the set, Q, E and one other byte: uniform, or E with probability 4/5"""
    alphabet = np.array(list(delims) + [Q, _other(delims, Q, E), E], dtype=np.uint8)
    k = alphabet.size
    return alphabet[rng.choice(k, ln, p=[1 / (5 * (k - 1))] * (k - 1) + [4 / 5] if heavy else [1 / k] * k)]


@pytest.mark.parametrize("heavy", [False, True])
@pytest.mark.parametrize("which,flags", [(0, 0), (1, 0), (2, 0), (0, NO_QUOTE), (0, NO_ESCAPE), (0, NO_QUOTE | NO_ESCAPE)])
def test_chunk_row_and_tile_edges_at_every_alignment(ctx, which, flags, heavy):
    """Every length around a chunk, a row and a tile at all 16 phases of out_off in one batch; in a second one a stream that starts 3
    bytes before a 64 KiB address boundary, one that starts 3 bytes behind one and ends on the next, one that starts 3 bytes before one
    and ends on the next.  Alphabet = the set, Q, E and one other byte, uniform and with E at 4 in 5; count mode and fill mode."""
    delims, Q, E = SETS[which]
    rng = np.random.default_rng(4000 + 8 * which + 2 * flags + heavy)
    offs, lens, at = [], [], 0
    for ln in EDGE_LENS:
        for phase in range(16):
            at = (at + 15) // 16 * 16 + phase + 16 * int(rng.integers(0, 5))
            offs.append(at)
            lens.append(ln)
            at += ln + int(rng.integers(0, 40))
    arena, base = _arena_tile_aligned(at + 64)  # (a 64 KiB aligned base: out_off mod 16 is the address mod 16)
    host = _filler(arena.numel(), delims, Q, E)
    offs = [base + o for o in offs]
    for o, ln in zip(offs, lens):
        host[o:o + ln] = _draw(rng, ln, delims, Q, E, heavy)
    arena.copy_(_dev(host))
    _check(ctx, host, arena, offs, lens, delims, Q, E, flags)

    arena, base = _arena_tile_aligned(7 * TILE)
    host = _filler(arena.numel(), delims, Q, E)
    offs = [base + TILE - 3, base + 3 * TILE + 3, base + 5 * TILE - 3]
    lens = [70000, TILE - 3, TILE + 3]
    for o, ln in zip(offs, lens):
        host[o:o + ln] = _draw(rng, ln, delims, Q, E, heavy)
    arena.copy_(_dev(host))
    _check(ctx, host, arena, offs, lens, delims, Q, E, flags)


CARRY_START = 5               # the stream starts 5 bytes behind a 64 KiB address
CARRY_LEN = 3 * TILE - 100    # ... and has 3 tiles
# address of the last byte of the run of escape bytes, from that 64 KiB address
CARRY_END = {"chunk_last": TILE + 3 * 1024 + 16 * 7 + 15, "row_last": TILE + 5 * 1024 + 1023, "tile_last": 2 * TILE - 1,
             "stream_last": CARRY_START + CARRY_LEN - 1}
CARRY_RUNS = (1, 2, 15, 16, 17, 1023, 1024, 1025)


def _carry_case(ctx, first, k, behind):
    """Line feeds and commas alternating, except a run of k escape bytes whose first byte is at address `first` (from the 64 KiB
    address) and the byte `behind` behind it (None: the run ends the stream).  What must come out is asserted on the CPU first: the
    run's bytes are never positions; the byte behind it is escaped, and so missing from pos, iff k is odd; a quote behind an even run
    opens a field that never closes, so nothing behind it is a position; a run that ends the stream leaves open bit 1 = k & 1; and
    `what` is the stream's byte at every position."""
    arena, base = _arena_tile_aligned(4 * TILE)
    host = _filler(arena.numel(), CSV, QT, BS)
    body = np.array([NL, CM], dtype=np.uint8)[np.arange(CARRY_LEN) % 2]
    assert (arena.data_ptr() + base) % TILE == 0
    p = first - CARRY_START  # stream offset of the run's first byte
    assert 0 < p and p + k <= CARRY_LEN
    body[p:p + k] = BS
    want = np.ones(CARRY_LEN, dtype=bool)
    want[p:p + k] = False
    want_open = 0
    if behind is None:
        assert p + k == CARRY_LEN
        want_open = (k & 1) << 1
    else:
        assert p + k < CARRY_LEN
        body[p + k] = behind
        if k & 1:
            want[p + k] = False  # escaped: data
        elif behind == QT:
            want[p + k:] = False  # an active quote: everything behind it is inside
            want_open = 1
    host[base + CARRY_START:base + CARRY_START + CARRY_LEN] = body
    arena.copy_(_dev(host))
    counts, opens, pos, what = _check(ctx, host, arena, [base + CARRY_START], [CARRY_LEN], CSV, QT, BS)
    assert opens.tolist() == [want_open] and (pos == np.flatnonzero(want)).all() and counts.tolist() == [int(want.sum())]
    assert (what == body[want]).all() and len(set(what.tolist())) >= 2


@pytest.mark.parametrize("where", sorted(CARRY_END))
def test_a_run_of_escapes_where_the_carry_crosses(ctx, where):
    """One run of k escape bytes that ends on the last byte of a lane's chunk, of a row, of a tile and of the stream, for k around a
    chunk and a row; behind it the last delimiter of the set, then a quote."""
    for k in CARRY_RUNS:
        first = CARRY_END[where] - k + 1
        if where == "stream_last":
            _carry_case(ctx, first, k, None)
        else:
            _carry_case(ctx, first, k, CSV[-1])
            _carry_case(ctx, first, k, QT)


def test_runs_that_cover_a_whole_tile(ctx):
    """Runs of 65536 + 1 and 65536 + 2 escape bytes that cover the stream's middle tile, a delimiter and a quote behind them; and a
    middle tile made only of escape bytes with a quote as the first byte of the next tile: the run is even, the quote is active."""
    for first, k in ((TILE - 1, TILE + 1), (TILE - 1, TILE + 2), (TILE - 2, TILE + 2), (TILE, TILE)):
        for behind in (CSV[-1], QT):
            _carry_case(ctx, first, k, behind)


def test_streams_do_not_leak(ctx):
    """Adjacent streams with no gap: the first ends on an active escape (open bit 1) and the second starts with a delimiter, which
    counts, at pos 0 with the right `what`; the first ends inside a quoted field and the second starts outside.  Both again with an
    empty stream between the two, for short streams and for ones of more than a tile."""
    rng = np.random.default_rng(5)
    turn = 0
    for la, lb in ((7, 9), (100, 1030), (70001, 66000)):
        for ending in ("escape", "quote"):
            for gap_stream in (False, True):
                a = _draw(rng, la, CSV, QT, BS, False)
                b = _draw(rng, lb, CSV, QT, BS, False)
                b[0] = CSV[turn % 3]
                turn += 1
                if ending == "escape":
                    a[-2:] = (0x78, BS)  # ... x E: one active escape on the last byte
                else:
                    a[-2:] = (0x78, 0x78)
                    if set_oracle.vec(a, CSV, QT, BS)[2] & 1 == 0:
                        a[-1] = QT  # (behind x: not escaped)
                want_a = set_oracle.vec(a, CSV, QT, BS)[2]
                assert (want_a >> 1 == 1) if ending == "escape" else (want_a & 1 == 1)
                host = _filler(333 + la + lb + 64, CSV, QT, BS)
                host[333:333 + la] = a
                host[333 + la:333 + la + lb] = b
                offs, lens = [333, 333 + la], [la, lb]
                if gap_stream:
                    offs, lens = [333, 333 + la, 333 + la], [la, 0, lb]
                counts, opens, pos, what = _check(ctx, host, _dev(host), offs, lens, CSV, QT, BS)
                at = counts[:-1].sum()
                assert opens[0] == want_a and pos[at] == 0 and what[at] == b[0]  # the second stream's first position is its byte 0


def test_order_and_state_across_many_tiles(ctx):
    """One stream of 4 MiB + 3 at an odd offset: 65 tiles that finish in any order, positions and `what` in order; the escapes dense,
    so that tiles are entered in every one of the four states (asserted from the oracle's states at the tile edges)."""
    rng = np.random.default_rng(61)
    ln = (4 << 20) + 3
    arena, base = _arena_tile_aligned(ln + 4096)
    host = _filler(arena.numel(), CSV, QT, BS)
    body = np.array([NL, 0x61, CR, CM], dtype=np.uint8)[rng.integers(0, 4, ln)]
    body[rng.integers(0, 50, ln) == 0] = QT
    body[rng.integers(0, 4, ln) == 0] = BS
    host[base + 777:base + 777 + ln] = body
    arena.copy_(_dev(host))
    st = set_oracle.states(body, QT, BS)
    edges = np.arange(1, 65) * TILE - 777  # stream offsets of the first bytes of tiles 1 .. 64
    assert edges[-1] < ln and set(st[edges].tolist()) == {0, 1, 2, 3}
    counts, _, pos, what = _check(ctx, host, arena, [base + 777], [ln], CSV, QT, BS)
    assert counts[0] > 1000 and (np.diff(pos) > 0).all() and set(what.tolist()) == set(CSV)
    got = ctx.index_set_batch(arena, _dev(np.array([base + 777], dtype=np.int64)), _dev(np.array([ln], dtype=np.int64)), delims=CSV)
    assert got[0].cpu().tolist() == [pos.size] and got[2].cpu().tolist() == [0]
    assert (got[3].cpu().numpy() == pos).all() and (got[4].cpu().numpy() == what).all()


def _small_batch(seed, n, top, delims=CSV, Q=QT, E=BS):
    """n streams of 0 .. top bytes over the set, Q, E and 'x' with gaps of 0 .. 20 filler bytes -> host arena, offs, lens.  Empty
    streams sit between streams that end on an active escape."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, top + 1, n).astype(np.int64)
    lens[10::50] = 0
    lens[9::50] = np.maximum(lens[9::50], 2)
    lens[11::50] = np.maximum(lens[11::50], 2)
    gaps = rng.integers(0, 21, n).astype(np.int64)
    offs = np.cumsum(gaps) + np.concatenate(([0], np.cumsum(lens[:-1])))
    host = _filler(int(offs[-1] + lens[-1] + 16), delims, Q, E)
    alphabet = np.array(list(delims) + [Q, E, 0x78], dtype=np.uint8)
    body = alphabet[rng.integers(0, alphabet.size, host.size)]
    for k, (o, ln) in enumerate(zip(offs, lens)):
        host[o:o + ln] = body[o:o + ln]
        if k % 50 in (9, 11):
            host[o + ln - 2:o + ln] = (0x78, E)  # ends on an active escape
    return host, offs, lens


def test_many_small_streams(ctx):
    """9000 streams of 0 .. 40 bytes, one item each -- more items than the 8192 waves of a full grid on 256 CUs take by their index,
    so the rest come from the ticket counter.  Empty streams sit between streams that end escaped: nothing leaks across them."""
    host, offs, lens = _small_batch(79, 9000, 40)
    _, opens, _, _, _ = _reference(host, offs, lens, CSV, QT, BS)
    assert (opens[9::50] >> 1).all() and (opens[11::50] >> 1).all() and not lens[10::50].any() and (opens & 1).sum() > 1000
    _check(ctx, host, _dev(host), offs, lens, CSV, QT, BS)


def test_the_flags(ctx):
    """BRX_INDEX_NO_ESCAPE, BRX_INDEX_NO_QUOTE and both, with the ignored argument set to a delimiter's value (ignored, not refused):
    the oracle under the flag, and the open bit that belongs to the flag is 0 everywhere.  Quote and escape bytes are in the data and
    are plain data under their flag; each flag changes more than 1000 counts on this batch."""
    host, offs, lens = _small_batch(80, 3000, 300)
    assert (host == QT).sum() > 1000 and (host == BS).sum() > 1000
    arena = _dev(host)
    base = _reference(host, offs, lens, CSV, QT, BS)[0]
    _, opens, _, _ = _check(ctx, host, arena, offs, lens, CSV, QT, BS, NO_ESCAPE, e_arg=NL)
    assert not (opens >> 1).any() and (opens & 1).sum() > 100
    assert (_reference(host, offs, lens, CSV, QT, BS, NO_ESCAPE)[0] != base).sum() > 1000
    _, opens, _, _ = _check(ctx, host, arena, offs, lens, CSV, QT, BS, NO_QUOTE, q_arg=CM)
    assert not (opens & 1).any() and (opens >> 1).sum() > 100
    assert (_reference(host, offs, lens, CSV, QT, BS, NO_QUOTE)[0] != base).sum() > 1000
    counts, opens, _, _ = _check(ctx, host, arena, offs, lens, CSV, QT, BS, NO_QUOTE | NO_ESCAPE, q_arg=CR, e_arg=CR)
    assert not opens.any()
    assert counts.tolist() == [int(np.isin(host[o:o + ln], list(CSV)).sum()) for o, ln in zip(offs, lens)]


def test_behind_a_decode_without_a_synchronisation(ctx):
    """64 JSON-Lines-like texts (0 .. 200 KiB, every third cut inside a string or behind a backslash) compressed on the device, then
    on one HIP stream: decode, lens = out_len * (status == 0), count mode with the 7-byte set of JSON's structure, torch.cumsum, fill
    mode with `total` from the CPU's count -- the host needs nothing from the device in between."""
    import torch
    from brotli_rs_amd import shard
    dev = torch.device("cuda:0")
    delims = set_oracle.J_SET
    texts = _json_texts(64, 200 << 10)
    n = len(texts)
    refs = [set_oracle.vec(np.frombuffer(t, dtype=np.uint8), delims, QT, BS) for t in texts]
    assert sum(1 for r in refs if r[2] == 1) >= 5 and sum(1 for r in refs if r[2] == 3) >= 5 and sum(1 for r in refs if not r[2]) >= 10
    total = int(sum(r[0].size for r in refs))
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
    out = _dev(_filler(int(out_off[-1]), delims, QT, BS))
    out_len = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    count = torch.full((n,), -7, dtype=torch.int64, device=dev)
    open_ = torch.full((n,), -7, dtype=torch.int32, device=dev)
    pos = torch.full((total + 8,), SENTINEL, dtype=torch.int64, device=dev)
    what = torch.full((total + 8,), WHAT_SENTINEL, dtype=torch.uint8, device=dev)
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
        args = (delims, QT, BS, 0, out.data_ptr(), d_out_off.data_ptr(), lens.data_ptr(), n, out.numel())
        ctx.index_set_batch_device(*args, count.data_ptr(), open_.data_ptr(), hip_stream=s.cuda_stream)
        pos_off = torch.cumsum(count, 0) - count
        ctx.index_set_batch_device(*args, None, None, pos_off.data_ptr(), pos.data_ptr(), what.data_ptr(), total, hip_stream=s.cuda_stream)
    s.synchronize()
    assert status.cpu().tolist() == [0] * n
    assert out_len.cpu().tolist() == [len(t) for t in texts]
    assert count.cpu().tolist() == [r[0].size for r in refs]
    assert open_.cpu().tolist() == [r[2] for r in refs]
    got, got_what = pos.cpu().numpy(), what.cpu().numpy()
    assert (got[:total] == np.concatenate([r[0] for r in refs])).all() and (got[total:] == SENTINEL).all()
    assert (got_what[:total] == np.concatenate([r[1] for r in refs])).all() and (got_what[total:] == WHAT_SENTINEL).all()


def test_agreement_with_the_shipped_passes_on_the_golden_batch(ctx):
    """All of tests/golden/data decoded in one BRX_MEM_DEVICE batch; quote and escape are byte values absent from all outputs but the
    few that hold every byte value, as in test_gpu_index_escaped.  One delimiter with flags 0 equals brx_index_escaped_batch,
    BRX_INDEX_NO_ESCAPE equals brx_index_quoted_batch, both flags equal brx_index_batch (the rules are the same, so this holds for
    every stream); a set of two equals the merge of two single calls, `what` telling them apart."""
    import torch
    dev = torch.device("cuda:0")
    streams = [open(os.path.join(GOLDEN, "data", e["stream"]), "rb").read() for e in MANIFEST]
    outs = [np.frombuffer(open(os.path.join(GOLDEN, "data", e["expected"]), "rb").read() if e["status"] == 0 else b"", dtype=np.uint8)
            for e in MANIFEST]
    holds = np.array([np.bincount(o, minlength=256) > 0 for o in outs])
    full = holds.all(axis=1)
    assert full.sum() <= 5
    free = np.flatnonzero(~holds[~full].any(axis=0))
    free = free[(free != NL) & (free != 0x20)]
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
    out = _dev(_filler(int(out_off[-1]), bytes([NL, 0x20]), quote, escape))
    out_len = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.decode_batch_device(blob.data_ptr(), d_in_off.data_ptr(), n, out.data_ptr(), d_out_off.data_ptr(), out_len.data_ptr(),
                            status.data_ptr())
    ctx.synchronize()
    assert status.cpu().tolist() == [e["status"] for e in MANIFEST]
    lens = out_len * (status == 0)

    def host(ts):
        return [t.cpu().numpy() for t in ts]

    plain = host(ctx.index_batch(out, d_out_off, lens, delim=NL))
    quoted = host(ctx.index_quoted_batch(out, d_out_off, lens, delim=NL, quote=quote))
    escaped = host(ctx.index_escaped_batch(out, d_out_off, lens, delim=NL, quote=quote, escape=escape))
    spaces = host(ctx.index_escaped_batch(out, d_out_off, lens, delim=0x20, quote=quote, escape=escape))
    one = host(ctx.index_set_batch(out, d_out_off, lens, delims=bytes([NL]), quote=quote, escape=escape))
    ne = host(ctx.index_set_batch(out, d_out_off, lens, delims=bytes([NL]), quote=quote, escape=NL, no_escape=True))
    both = host(ctx.index_set_batch(out, d_out_off, lens, delims=bytes([NL]), quote=NL, escape=NL, no_quote=True, no_escape=True))
    two = host(ctx.index_set_batch(out, d_out_off, lens, delims=bytes([0x20, NL]), quote=quote, escape=escape))
    for got, want in ((one, escaped), (ne, quoted)):
        for k in range(4):
            assert (got[k] == want[k]).all(), k
        assert (got[4] == NL).all()
    assert (both[0] == plain[0]).all() and not both[1].any() and (both[2] == plain[1]).all() and (both[3] == plain[2]).all()
    assert (two[0] == escaped[0] + spaces[0]).all() and (two[1] == escaped[1]).all() and (two[1] == spaces[1]).all()
    count, _, pos_off, pos, what = two
    for i in range(n):
        mine, w = pos[pos_off[i]:pos_off[i] + count[i]], what[pos_off[i]:pos_off[i] + count[i]]
        assert (np.diff(mine) > 0).all(), i
        assert (mine[w == NL] == escaped[3][escaped[2][i]:escaped[2][i] + escaped[0][i]]).all(), i
        assert (mine[w == 0x20] == spaces[3][spaces[2][i]:spaces[2][i] + spaces[0][i]]).all(), i
    assert plain[0].sum() > 10000 and spaces[0].sum() > 10000


def test_total_is_a_bound(ctx):
    """Fill mode with room for half the entries: pos and what are right up to it, and the sentinels behind it are untouched."""
    import torch
    host, offs, lens = _small_batch(6, 300, 3000)
    arena = _dev(host)
    _, _, want_off, want_pos, want_what = _reference(host, offs, lens, CSV, QT, BS)
    half = int(want_pos.size // 2)
    assert half > 1000
    pos = torch.full((want_pos.size + 8,), SENTINEL, dtype=torch.int64, device="cuda:0")
    what = torch.full((want_pos.size + 8,), WHAT_SENTINEL, dtype=torch.uint8, device="cuda:0")
    d_off, d_len, d_pos_off = _dev(offs), _dev(lens), _dev(want_off)
    torch.cuda.synchronize()
    ctx.index_set_batch_device(CSV, QT, BS, 0, arena.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), len(lens), arena.numel(), None, None,
                               d_pos_off.data_ptr(), pos.data_ptr(), what.data_ptr(), half)
    got, got_what = pos.cpu().numpy(), what.cpu().numpy()
    assert (got[:half] == want_pos[:half]).all() and (got_what[:half] == want_what[:half]).all()
    assert (got[half:] == SENTINEL).all() and (got_what[half:] == WHAT_SENTINEL).all()


def test_overlapping_calls_on_two_streams(ctx):
    """20 fill-mode calls alternating between two HIP streams over different small batches -- more than the 16 regions of the scratch
    ring -- and one synchronisation at the end."""
    import torch
    dev = torch.device("cuda:0")
    jobs = []
    for k in range(20):
        host, offs, lens = _small_batch(800 + k, 60 + k, 3000)
        want_count, want_open, want_off, want_pos, want_what = _reference(host, offs, lens, CSV, QT, BS)
        jobs.append(dict(arena=_dev(host), offs=_dev(offs), lens=_dev(lens), pos_off=_dev(want_off), n=len(lens), total=int(want_pos.size),
                         count=torch.full((len(lens),), -7, dtype=torch.int64, device=dev),
                         open=torch.full((len(lens),), -7, dtype=torch.int32, device=dev),
                         pos=torch.full((want_pos.size + 8,), SENTINEL, dtype=torch.int64, device=dev),
                         what=torch.full((want_pos.size + 8,), WHAT_SENTINEL, dtype=torch.uint8, device=dev),
                         want_count=want_count, want_open=want_open, want_pos=want_pos, want_what=want_what))
    s = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    torch.cuda.synchronize()
    for k, j in enumerate(jobs):
        ctx.index_set_batch_device(CSV, QT, BS, 0, j["arena"].data_ptr(), j["offs"].data_ptr(), j["lens"].data_ptr(), j["n"],
                                   j["arena"].numel(), j["count"].data_ptr(), j["open"].data_ptr(), j["pos_off"].data_ptr(),
                                   j["pos"].data_ptr(), j["what"].data_ptr(), j["total"], hip_stream=s[k % 2].cuda_stream)
    torch.cuda.synchronize()
    for k, j in enumerate(jobs):
        assert (j["count"].cpu().numpy() == j["want_count"]).all(), k
        assert (j["open"].cpu().numpy() == j["want_open"]).all(), k
        got, got_what = j["pos"].cpu().numpy(), j["what"].cpu().numpy()
        assert (got[:j["total"]] == j["want_pos"]).all() and (got[j["total"]:] == SENTINEL).all(), k
        assert (got_what[:j["total"]] == j["want_what"]).all() and (got_what[j["total"]:] == WHAT_SENTINEL).all(), k


def test_arguments(ctx):
    """The contract's table on a real context: every refusal -> BRX_ERR_INVALID_ARGUMENT with its message and nothing is launched
    (the sentinels in count and open survive); n = 0 -> BRX_SUCCESS; open NULL, count NULL in fill mode and what NULL are accepted;
    then a good call on the same context is right."""
    import torch
    dev = torch.device("cuda:0")
    arena = torch.full((64,), NL, dtype=torch.uint8, device=dev)
    arena[1] = CM   # stream 0 = \n , \n \n \n, an escape, an escaped delimiter, a delimiter
    arena[5] = BS
    arena[20] = QT  # stream 1 = 4 delimiters, a quote, 3 delimiters inside the field it opens
    offs = torch.tensor([0, 16], dtype=torch.int64, device=dev)
    lens = torch.full((2,), 8, dtype=torch.int64, device=dev)
    count = torch.full((2,), -7, dtype=torch.int64, device=dev)
    open_ = torch.full((2,), -7, dtype=torch.int32, device=dev)
    pos_off = torch.tensor([0, 6], dtype=torch.int64, device=dev)
    pos = torch.full((14,), SENTINEL, dtype=torch.int64, device=dev)
    what = torch.full((14,), WHAT_SENTINEL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    lib, h = ctx._lib, ctx._h
    f = lib.brx_index_set_batch
    args = (arena.data_ptr(), offs.data_ptr(), lens.data_ptr())
    c, o, po, p, w = count.data_ptr(), open_.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), what.data_ptr()
    D = b",\n"

    def refused(word, rc):
        e = lib.brx_last_error()
        return rc == -1 and b"brx_index_set_batch" in e and word in e

    assert f(h, D, 2, QT, BS, 0, *args, 0, 64, c, o, None, None, None, 0, None) == 0  # n = 0
    assert f(h, D, 2, QT, BS, 0, None, None, None, 0, 0, c, None, None, None, None, 0, None) == 0
    assert refused(b"ctx", f(None, D, 2, QT, BS, 0, *args, 2, 64, c, o, None, None, None, 0, None))
    assert refused(b"flag", f(h, D, 2, QT, BS, 4, *args, 2, 64, c, o, None, None, None, 0, None))
    assert refused(b"delims", f(h, None, 2, QT, BS, 0, *args, 2, 64, c, o, None, None, None, 0, None))
    assert refused(b"delims", f(h, D, 0, QT, BS, 0, *args, 2, 64, c, o, None, None, None, 0, None))
    assert refused(b"delims", f(h, b"123456789", 9, QT, BS, 0, *args, 2, 64, c, o, None, None, None, 0, None))
    assert refused(b"twice", f(h, b",\n,", 3, QT, BS, 0, *args, 2, 64, c, o, None, None, None, 0, None))
    assert refused(b"escape", f(h, b",\\", 2, QT, BS, 0, *args, 2, 64, c, o, None, None, None, 0, None))
    assert refused(b"quote", f(h, b",\"", 2, QT, BS, 0, *args, 2, 64, c, o, None, None, None, 0, None))
    assert refused(b"quote", f(h, D, 2, BS, BS, 0, *args, 2, 64, c, o, None, None, None, 0, None)) and b"escape" in lib.brx_last_error()
    assert refused(b"pos_off", f(h, D, 2, QT, BS, 0, *args, 2, 64, c, o, po, None, None, 14, None))
    assert refused(b"pos_off", f(h, D, 2, QT, BS, 0, *args, 2, 64, c, o, None, p, w, 14, None))
    assert refused(b"what", f(h, D, 2, QT, BS, 0, *args, 2, 64, c, o, None, None, w, 14, None))
    assert refused(b"count", f(h, D, 2, QT, BS, 0, *args, 2, 64, None, o, None, None, None, 0, None))
    assert f(h, D, 2, QT, BS, 0, arena.data_ptr(), None, lens.data_ptr(), 2, 64, c, o, None, None, None, 0, None) == -1
    assert f(h, D, 2, QT, BS, 0, arena.data_ptr(), offs.data_ptr(), None, 2, 64, c, o, None, None, None, 0, None) == -1
    torch.cuda.synchronize()
    assert open_.cpu().tolist() == [-7, -7] and count.cpu().tolist() == [-7, -7]  # (nothing was launched)
    assert pos.cpu().tolist() == [SENTINEL] * 14 and what.cpu().tolist() == [WHAT_SENTINEL] * 14
    assert f(h, D, 2, QT, BS, 0, *args, 2, 64, c, None, None, None, None, 0, None) == 0  # open NULL, count mode
    assert count.cpu().tolist() == [6, 4]
    assert f(h, D, 2, CM, NL, NO_QUOTE | NO_ESCAPE, *args, 2, 64, c, o, None, None, None, 0, None) == 0  # both ignored under their flags
    assert count.cpu().tolist() == [7, 7] and open_.cpu().tolist() == [0, 0]  # (the escape and the quote are data, no delimiters)
    assert f(h, D, 2, QT, BS, 0, *args, 2, 64, None, None, po, p, None, 14, None) == 0  # count, open and what NULL, fill mode
    assert pos.cpu().tolist() == [0, 1, 2, 3, 4, 7] + list(range(4)) + [SENTINEL] * 4 and what.cpu().tolist() == [WHAT_SENTINEL] * 14
    pos.fill_(SENTINEL)
    torch.cuda.synchronize()
    assert f(h, D, 2, QT, BS, 0, *args, 2, 64, c, o, po, p, w, 14, None) == 0  # (the context still works)
    assert count.cpu().tolist() == [6, 4] and open_.cpu().tolist() == [0, 1]
    assert pos.cpu().tolist() == [0, 1, 2, 3, 4, 7] + list(range(4)) + [SENTINEL] * 4
    assert what.cpu().tolist() == [NL, CM, NL, NL, NL, NL] + [NL] * 4 + [WHAT_SENTINEL] * 4
