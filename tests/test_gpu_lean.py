"""The lean short-stream kernel (brx_small.h) against the CPU oracle over its whole range: streams of 1 .. 500 compressed bytes with
BRX_OPTION_SMALL_BYTES = 500, through every entry of brx_decode_batch.  tests/lean_cases.py builds the cases and says for each one
which kernel instance must decode it; the per-stream trace (all-zero record = the lean instance) and brx_last_timing(5) are held to
that, so a stream the lean kernel quietly leaves to the regular one fails here like a wrong byte does.

Contexts are made with brx.Context directly: the suite's environment knobs must not change who decodes."""
import ctypes
import random
import time

import numpy as np
import pytest

import lean_cases as lc
from capacity_cases import read

pytestmark = pytest.mark.gpu

FILL = 0xEE
MARGIN = 64
SENTINEL = 0xEEEEEEEEEEEEEEEE
PATHS = ["pageable", "pinned", "device", "device_order"]


def _context(**opts):
    from brotli_rs_amd import brx
    return brx.Context(0, options=dict({"small_bytes": 500, "trace": 1}, **opts))


def _decode(ctx, cases, path):
    """One batch: streams back to back, slot i exactly cases[i].cap bytes (odd: every output phase mod 16), status pre-filled with
    -1, out_len with a sentinel, the arena with 0xEE.  -> (status, out_len, arena as a host array, out_off); slot i is at
    arena[MARGIN + out_off[i] ..]."""
    from brotli_rs_amd import brx
    blob, in_off, out_off = lc.tables(cases)
    n = len(cases)
    total = int(out_off[-1])
    if path in ("device", "device_order"):
        import torch
        dev = torch.device("cuda:0")
        arena = torch.full((2 * MARGIN + total,), FILL, dtype=torch.uint8, device=dev)
        d_blob = torch.from_numpy(blob.copy()).to(dev)
        assert d_blob.data_ptr() % 4 == 0 and arena.data_ptr() % 16 == 0
        d_in_off = torch.from_numpy(in_off.astype(np.int64)).to(dev)
        d_out_off = torch.from_numpy(out_off.astype(np.int64)).to(dev)
        d_len = torch.full((n,), SENTINEL - (1 << 64), dtype=torch.int64, device=dev)  # (the same bit pattern as on the host paths)
        d_status = torch.full((n,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.decode_batch_device(d_blob.data_ptr(), d_in_off.data_ptr(), n, arena.data_ptr() + MARGIN, d_out_off.data_ptr(), d_len.data_ptr(),
                                d_status.data_ptr(), order=path == "device_order")
        ctx.synchronize()
        return d_status.cpu().numpy(), d_len.cpu().numpy().astype(np.uint64), arena.cpu().numpy(), out_off
    pinned = path == "pinned"
    if pinned:
        h_in, arena = brx.host_alloc(len(blob)), brx.host_alloc(2 * MARGIN + total)
        h_in[:] = blob
    else:
        h_in, arena = blob.copy(), np.empty(2 * MARGIN + total, dtype=np.uint8)
    try:
        assert h_in.ctypes.data % 4 == 0
        arena[:] = FILL
        out_len = np.full(n, SENTINEL, dtype=np.uint64)
        status = np.full(n, -1, dtype=np.int32)
        opts = brx._Opts(brx.MEM_HOST, 0, None)
        rc = brx.load_library().brx_decode_batch(ctx._h, h_in.ctypes.data, in_off.ctypes.data, n, arena.ctypes.data + MARGIN, out_off.ctypes.data,
                                                 out_len.ctypes.data, status.ctypes.data, ctypes.byref(opts))
        assert rc == 0, rc
        return status, out_len, np.array(arena), out_off
    finally:
        if pinned:
            brx.host_free(h_in)
            brx.host_free(arena)


def _check(ctx, cases, status, out_len, arena, out_off, slack, small_bytes=500):
    """Steps 3 .. 6 of the batch protocol.  slack: also nothing behind out_len inside a status-0 slot (device and pinned paths: a
    pageable batch is staged, and the copy back brings a slot's slack along).
    What "nothing outside a slot" covers: the 64 bytes in front of the first slot and behind the last, and -- slots lie back to
    back -- every status-0 slot, whose bytes and slack are compared in full, so an overrun into one shows.  What the slot of a
    stream that fails (or gets status 25) holds behind its prefix is not specified (brx.h): the lean kernel may have written
    there before it gave the stream up.  An overrun from one such slot into another such slot is therefore not seen here."""
    n = len(cases)
    assert out_len.dtype == np.uint64 and not (out_len == SENTINEL).any(), "an out_len that was never written"
    bad = []
    for i, c in enumerate(cases):
        st, ln, o0 = int(status[i]), int(out_len[i]), MARGIN + int(out_off[i])
        what = None
        if st != c.status:
            what = "status"
        elif c.status in (0, 25):
            if ln != c.out_len:
                what = "out_len"
            elif c.status == 0 and arena[o0:o0 + ln].tobytes() != c.out:
                what = "bytes"
            elif c.status == 0 and slack and not (arena[o0 + ln:o0 + c.cap] == FILL).all():
                what = "written behind out_len"
        else:  # (the prefix contract of brx.h, as tools/prefix_fuzz.py holds it)
            m = min(ln, len(c.out), c.cap)
            if ln == SENTINEL or arena[o0:o0 + m].tobytes() != c.out[:m]:
                what = "prefix"
        if what:
            bad.append((what, i, c.name, len(c.data), "cap", c.cap, "want", c.status, c.out_len, "got", st, ln, c.owner))
    for b in bad[:30]:
        print(b)
    assert not bad, (len(bad), bad[:6])
    assert (arena[:MARGIN] == FILL).all() and (arena[MARGIN + int(out_off[-1]):] == FILL).all(), "bytes written outside the batch's slots"
    trace = ctx.last_trace(n)
    lean_rec = ~trace.any(axis=1)
    want_lean = np.array([c.owner == "lean" for c in cases])
    wrong = np.flatnonzero(lean_rec != want_lean)
    for i in wrong[:30]:
        print("owner", int(i), cases[i].name, len(cases[i].data), "B, want", cases[i].owner, "trace", "lean" if lean_rec[i] else "regular")
    assert not len(wrong), (len(wrong), [(cases[i].name, cases[i].owner) for i in wrong[:8]])
    listed = int(ctx._lib.brx_last_timing(ctx._h, 5))
    assert listed == (n - int(want_lean.sum()) if small_bytes else 0), (listed, n, int(want_lean.sum()))  # (0: no lean instance ran)


def _all_phases(cases):
    """Every size edge of the batch starts at each of the four input phases (in_off % 4; the blob itself is 4-byte aligned)."""
    _, in_off, _ = lc.tables(cases)
    seen = {}
    for i, c in enumerate(cases):
        if "edge" in c.tags:
            seen.setdefault(c.name, set()).add(int(in_off[i]) % 4)
    assert len(seen) == 29 and all(p == {0, 1, 2, 3} for p in seen.values()), {k: v for k, v in seen.items() if v != {0, 1, 2, 3}}


@pytest.fixture(scope="module")
def everything():
    """lean_cases.full_batch(): the plain and the deferred set, truncated streams followed directly by a neighbour's first bytes, every
    size edge at all four input phases behind junk streams."""
    t0 = time.time()
    out = list(lc.full_batch())
    _all_phases(out)
    print("lean cases: %d in the batch, built in %.1f s" % (len(out), time.time() - t0))
    return out


@pytest.mark.parametrize("path", PATHS)
def test_every_path(everything, path):
    """Plain and deferred sets with small_bytes = 500 through pageable host pointers (the order-tail entry), brx_host_alloc buffers
    (the mirror stores), device pointers without BRX_OPT_ORDER (the classification entry) and with it."""
    ctx = _context()
    try:
        t0 = time.time()
        status, out_len, arena, out_off = _decode(ctx, everything, path)
        print("%s: %d streams, %.2f s" % (path, len(everything), time.time() - t0))
        _check(ctx, everything, status, out_len, arena, out_off, slack=path != "pageable")
    finally:
        ctx.close()


def test_small_bytes_500_128_and_0_agree(everything):
    """The same batch with small_bytes 500, 128 and 0: identical results, all the oracle's, and the owners follow the size rule --
    with 128 the streams of 129 .. 500 B turn to the regular kernel, with 0 every trace record is non-zero."""
    cases = everything
    results = []
    for sb in (500, 128, 0):
        ctx = _context(small_bytes=sb)
        try:
            owned = lc.with_small_bytes(cases, sb)
            if sb == 0:
                assert all(c.owner == "regular" for c in owned)
            status, out_len, arena, out_off = _decode(ctx, owned, "device")
            _check(ctx, owned, status, out_len, arena, out_off, slack=True, small_bytes=sb)
            ok = [i for i, c in enumerate(cases) if c.status in (0, 25)]
            results.append((status.copy(), out_len[ok].copy(), [arena[MARGIN + int(out_off[i]):MARGIN + int(out_off[i]) + int(out_len[i])].tobytes()
                                                                 for i in ok if cases[i].status == 0]))
        finally:
            ctx.close()
    for r in results[1:]:
        assert (r[0] == results[0][0]).all() and (r[1] == results[0][1]).all() and r[2] == results[0][2]


def _stale_sequence(deferred_every=0):
    """About 3 x the lean grid of small_waves = 1 (one wave per CU) in rows of one grid each: wave w decodes row 0's w-th stream, then
    row 1's, ... with the same LDS -- a many-tree stream behind a one-tree one, raw-only behind compressed, 500 B behind 1 B."""
    import torch
    grid = torch.cuda.get_device_properties(0).multi_processor_count
    P = [c for c in lc.plain_set() if c.owner == "lean" and c.out_len <= 70000]
    census = {c.name: lc.full(c.data)[2] for c in P}
    many = [c for c in P if census[c.name]["ntrees_l_mask"] & ~0x0002000200020002]  # some meta-block with NTREESL > 1
    one = [c for c in P if c not in many and census[c.name]["commands"]]
    tiny = [c for c in P if not census[c.name]["commands"]]  # raw only, or the empty 1-byte stream
    big = [c for c in P if len(c.data) >= 499]
    assert many and one and len(tiny) == 2 and len(big) >= 2
    rng = random.Random(3)
    row0 = [rng.choice(P) for _ in range(grid)]
    row1 = [rng.choice(one if c in many else many) for c in row0]
    row2 = [(big if w % 2 else tiny)[(w // 2) % 2] for w in range(grid)]
    row3 = [(tiny if w % 2 else big)[(w // 2) % 2] for w in range(grid)]
    seq = row0 + row1 + row2 + row3
    if deferred_every:
        D = [c for c in lc.deferred_named()] + list(lc.prefix_set()[::13]) + list(lc.bitflip_set()[::61])
        rng.shuffle(D)
        for k in range(len(seq)):  # (stream k of row r goes to wave k - r * grid: every wave meets a deferred stream between plain ones)
            if (k % grid + k // grid) % deferred_every == 0:
                seq[k] = D[k % len(D)]
    return seq, grid


@pytest.mark.parametrize("deferred_every", [0, 3], ids=["plain", "every_third_deferred"])
def test_state_left_by_the_previous_stream(deferred_every):
    """small_waves = 1: every wave decodes several different streams in a row (device pointers, no queue order: stream index =
    workgroup + k * grid).  Tree handles, the context-id table and table memory of the stream before must not show.
    (No junk streams here: which wave decodes what goes by the stream's index, and the rows must stay rows.  The input phases are the
    other tests'.)"""
    seq, grid = _stale_sequence(deferred_every)
    assert len(seq) >= 3 * grid
    ctx = _context(small_waves=1)
    try:
        status, out_len, arena, out_off = _decode(ctx, seq, "device")
        _check(ctx, seq, status, out_len, arena, out_off, slack=True)
    finally:
        ctx.close()


@pytest.mark.parametrize("levels", [0, 2])
def test_mixed_batch(levels):
    """Plain and deferred cases, the 501-byte stream, alice29 and a 200-byte text through the flat generator (its insert&copy code
    alone spans all 704 symbols: tables beyond the lean table memory) in one batch, under both launch plans."""
    ctx = _context(levels=levels)
    try:
        text = (b"It is a truth universally acknowledged, that a single man in possession of a good fortune, must be in want of a wife. "
                b"However little known the feelings or views of such a man may be on his first entering a neighbourhood, this truth")[:200]
        gen = ctx.generate_batch([text])[0]
        flat = lc.case("generated_flat_200", gen, tags=("deferred",))
        print("generated: %d B, %d table words" % (len(gen), lc.full(gen)[2]["max_table_words"]))
        assert flat.status == 0 and flat.out == text and flat.owner == "regular"
        assert len(gen) <= lc.SMALL_MAX and lc.full(gen)[2]["max_table_words"] > lc.TM_WORDS  # deferred for its tables, not its size
        alice = lc.case("alice29", read("alice29.txt.compressed"))
        assert alice.status == 0 and alice.owner == "regular"
        cases = list(lc.plain_set() + lc.deferred_set()) + [flat, alice]
        random.Random(levels).shuffle(cases)
        cases = lc.with_phases(cases)  # (last: the junk is sized by the offsets of this very sequence)
        _all_phases(cases)
        for path in ("device", "pageable"):
            status, out_len, arena, out_off = _decode(ctx, cases, path)
            _check(ctx, cases, status, out_len, arena, out_off, slack=path == "device")
    finally:
        ctx.close()
