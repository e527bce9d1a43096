"""The output-capacity edge of brx_decode_batch against the CPU oracle (tests/capacity_cases.py builds the cases).  A stream's slot is
out[out_off[i] .. out_off[i + 1]):  nothing outside it is ever written;  a slot that is too small gives status 25 with out_len = the
position in front of the item that did not fit + that item's size;  one bad stream never affects another."""
import ctypes
import io
import random

import numpy as np
import pytest

import brx_knobs
import capacity_cases as cc
import oracle_py as oracle

pytestmark = pytest.mark.gpu

FILL = 0xEE
MARGIN = 64
EMPTY = cc.read("empty.compressed")

# the paths that enforce the capacity differently: C++ command loops (8: whole meta-blocks, 7: re-entered per command, 6: the default
# loop with no meta-block given to the assembly loop), both builds of the assembly loop, no lean instance, tiny streams through
# the assembly loop, both launch plans, no hand-up to the wider instances
PATHS = [{}, {"command_loop": 8}, {"command_loop": 7}, {"command_loop": 6}, {"loop_build": 0}, {"loop_build": 1}, {"small_bytes": 0},
         {"tiny_bytes": 0}, {"levels": 0}, {"levels": 2}, {"hand_up": 0}]


def _id(opts):
    return "-".join("%s=%d" % kv for kv in sorted(opts.items())) or "default"


def _context(opts):
    c = brx_knobs.context(0, **opts)
    if "levels" in opts:  # (a context that has handed a stream up lately runs the full chain of wider kernels)
        lcet = next(s for s in cc.streams() if s.name == "level1_tables")
        outs, status, _ = c.decode_batch([lcet.data], 1 << 19)
        assert int(status[0]) == 0 and outs[0] == lcet.full
    return c


@pytest.fixture(scope="module")
def ctx():
    c = brx_knobs.context(0)
    yield c
    c.close()


def _tables(cases):
    """(blob, in_off, out_off) of a batch of cases, each slot exactly its case's capacity."""
    S = cc.streams()
    n = len(cases)
    in_off = np.zeros(n + 1, dtype=np.uint64)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    in_off[1:] = np.cumsum([len(S[c.stream].data) for c in cases])
    out_off[1:] = np.cumsum([c.cap for c in cases])
    blob = np.frombuffer(b"".join(S[c.stream].data for c in cases) + bytes(MARGIN), dtype=np.uint8)
    return blob, in_off, out_off


def _mismatches(cases, status, out_len, out, out_off, base=0):
    """Cases whose status, out_len or bytes are not the oracle's.  out: host array, slot i at out[base + out_off[i] ..]."""
    S = cc.streams()
    bad = []
    for i, c in enumerate(cases):
        st, ln, o0 = int(status[i]), int(out_len[i]), base + int(out_off[i])
        what = None
        if st != c.status:
            what = "status"
        elif c.status in (0, 25):  # out_len is specified: the decoded size / the bytes needed so far
            if ln != c.out_len:
                what = "out_len"
            elif c.status == 0 and out[o0:o0 + ln].tobytes() != cc.case_bytes(c):
                what = "bytes"
        else:
            # An invalid stream at its error: the prefix contract of brx.h -- the slot's bytes [0, min(out_len, capacity)) are the
            # stream's output in front of the error.  How far INTO the failing command out_len points is not specified: the oracle
            # counts an insert's literals when all of them are there and a copy when it is done, the kernels count every literal
            # as it lands and may meet the next command's error before the copy in flight has landed.  So the bytes are compared
            # as far as both sides report them.
            m = min(ln, c.cap, c.out_len)
            if out[o0:o0 + m].tobytes() != cc.streams()[c.stream].full[:m]:
                what = "prefix"
        if what:
            bad.append((what, S[c.stream].name, "cap", c.cap, "want", c.status, c.out_len, "got", st, ln))
    return bad


@pytest.mark.parametrize("opts", PATHS, ids=_id)
def test_status_length_and_bytes_of_every_case(opts):
    """The whole table as ONE batch through host buffers, in a shuffled order: a status-25 slot sits next to valid ones of other
    streams.  Status and out_len are the oracle's for every case -- under status 25 that is `needed`, exactly -- and so are the
    bytes of every case that is not status 25."""
    cases = list(cc.table())
    random.Random(2025).shuffle(cases)
    blob, in_off, out_off = _tables(cases)
    out = np.full(int(out_off[-1]) + 2 * MARGIN, FILL, dtype=np.uint8)
    c = _context(opts)
    try:
        status, out_len = c.decode_batch_host_raw(blob.ctypes.data, in_off, len(cases), out.ctypes.data + MARGIN, out_off)
    finally:
        c.close()
    bad = _mismatches(cases, status, out_len, out, out_off, MARGIN)
    print("%s: %d cases, %d mismatches" % (_id(opts), len(cases), len(bad)))
    for b in bad[:40]:
        print(b)
    assert not bad, (len(bad), bad[:8])
    assert (out[:MARGIN] == FILL).all() and (out[MARGIN + int(out_off[-1]):] == FILL).all()


def _guarded_layout():
    """The guard cases with an `empty` stream in a slot of 33 .. 48 bytes between every two of them, sized so that real slot k starts
    at out_off = k (mod 16): whatever the phase of `out` itself, the real slots start at all 16 phases of a 16-byte unit.
    -> (cases with None for a guard slot, blob, in_off, out_off)."""
    real = list(cc.guard_cases())
    random.Random(7).shuffle(real)
    S = cc.streams()
    slots, caps, at = [], [], 0
    for k, c in enumerate(real):
        if k:
            g = 33 + (k - (at + 33)) % 16  # the guard slot that makes the next real slot start at k (mod 16)
            slots.append(None); caps.append(g)
            at += g
        assert at % 16 == k % 16
        slots.append(c); caps.append(c.cap)
        at += c.cap
    assert {o % 16 for o, s in zip(np.cumsum([0] + caps[:-1]), slots) if s is not None} == set(range(16))
    data = [EMPTY if s is None else S[s.stream].data for s in slots]
    n = len(slots)
    in_off = np.zeros(n + 1, dtype=np.uint64)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    in_off[1:] = np.cumsum([len(d) for d in data])
    out_off[1:] = np.cumsum(caps)
    blob = np.frombuffer(b"".join(data) + bytes(MARGIN), dtype=np.uint8)
    return slots, blob, in_off, out_off


def _check_guarded(slots, status, out_len, arena, out_off, base):
    """arena: host copy, 0xEE before the call; slot i at arena[base + out_off[i] ..].  Every byte in front of the first slot, behind
    the last, in a guard slot and behind the output of a status-0 slot is still 0xEE; statuses, lengths and bytes are
    the oracle's.  (What a status-25 slot or the slot of an invalid stream holds behind its prefix is not specified.)"""
    real = [(i, s) for i, s in enumerate(slots) if s is not None]
    bad = _mismatches([s for _, s in real], [status[i] for i, _ in real], [out_len[i] for i, _ in real], arena,
                      [out_off[i] for i, _ in real], base)
    assert not bad, (len(bad), bad[:8])
    untouched = np.ones(len(arena), dtype=bool)
    for i, s in enumerate(slots):
        o0, o1 = base + int(out_off[i]), base + int(out_off[i + 1])
        if s is None:
            assert (int(status[i]), int(out_len[i])) == (0, 0), (i, int(status[i]), int(out_len[i]))
        elif s.status == 0:
            untouched[o0:o0 + s.out_len] = False
        else:
            untouched[o0:o1] = False
    dirty = np.flatnonzero(untouched & (arena != FILL))
    if len(dirty):
        at = int(dirty[0]) - base
        i = int(np.searchsorted(out_off, at, side="right")) - 1
        who = None if not 0 <= i < len(slots) else "guard slot" if slots[i] is None else (cc.streams()[slots[i].stream].name, slots[i])
        assert False, ("%d bytes written outside the streams' own" % len(dirty), "first at out +", at, "slot", i, who,
                       "value", int(arena[dirty[0]]))


@pytest.mark.parametrize("opts", [{}, {"command_loop": 8}], ids=_id)
def test_device_path_writes_nothing_outside_a_slot(opts):
    """Device pointers: one arena of 0xEE, 64 guard bytes in front of out_off[0] and behind out_off[n], guard slots (an `empty` stream
    each) between the real ones, the real slots starting at all 16 phases of a 16-byte unit."""
    import torch
    dev = torch.device("cuda:0")
    c = _context(opts)
    try:
        for phase in (0, 5):
            slots, blob, in_off, out_off = _guarded_layout()
            n = len(slots)
            arena = torch.full((2 * MARGIN + 16 + int(out_off[-1]),), FILL, dtype=torch.uint8, device=dev)
            assert arena.data_ptr() % 16 == 0
            d_blob = torch.from_numpy(blob.copy()).to(dev)
            d_in_off = torch.from_numpy(in_off.astype(np.int64)).to(dev)
            d_out_off = torch.from_numpy(out_off.astype(np.int64)).to(dev)
            d_len = torch.full((n,), -1, dtype=torch.int64, device=dev)
            d_status = torch.full((n,), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            c.decode_batch_device(d_blob.data_ptr(), d_in_off.data_ptr(), n, arena.data_ptr() + MARGIN + phase, d_out_off.data_ptr(),
                                  d_len.data_ptr(), d_status.data_ptr())
            c.synchronize()
            _check_guarded(slots, d_status.cpu().numpy(), d_len.cpu().numpy(), arena.cpu().numpy(), out_off, MARGIN + phase)
    finally:
        c.close()


def test_pinned_path_writes_nothing_outside_a_slot(ctx):
    """Pinned host buffers, used in place (the output pointer at the 16-byte phase of the staging slots): the same layout, the same
    assertions, the slack of every status-0 slot included."""
    from brotli_rs_amd import brx
    for phase in (0, 16):
        slots, blob, in_off, out_off = _guarded_layout()
        pin_in = brx.host_alloc(len(blob))
        pin_out = brx.host_alloc(2 * MARGIN + 16 + int(out_off[-1]))
        try:
            assert pin_out.ctypes.data % 16 == 0
            pin_in[:] = blob
            pin_out[:] = FILL
            status, out_len = ctx.decode_batch_host_raw(pin_in.ctypes.data, in_off, len(slots), pin_out.ctypes.data + MARGIN + phase, out_off)
            _check_guarded(slots, status, out_len, pin_out, out_off, MARGIN + phase)
        finally:
            brx.host_free(pin_in)
            brx.host_free(pin_out)


def test_pageable_path_writes_nothing_outside_the_batch(ctx):
    """Pageable host buffers are staged: a copy may bring a slot's slack along, so only the 64 bytes in front of out + out_off[0] and
    behind out + out_off[n] (and the statuses, lengths and bytes) are held."""
    for phase in (0, 5):
        slots, blob, in_off, out_off = _guarded_layout()
        arena = np.full(2 * MARGIN + 16 + int(out_off[-1]), FILL, dtype=np.uint8)
        status, out_len = ctx.decode_batch_host_raw(blob.ctypes.data, in_off, len(slots), arena.ctypes.data + MARGIN + phase, out_off)
        base = MARGIN + phase
        bad = _mismatches([s for s in slots if s is not None], [x for x, s in zip(status, slots) if s is not None],
                          [x for x, s in zip(out_len, slots) if s is not None], arena, [o for o, s in zip(out_off, slots) if s is not None], base)
        assert not bad, (len(bad), bad[:8])
        assert all((int(status[i]), int(out_len[i])) == (0, 0) for i, s in enumerate(slots) if s is None)
        assert (arena[:base] == FILL).all() and (arena[base + int(out_off[-1]):] == FILL).all(), phase


def _offset_batch(ctx, names, in_off, out_off, arena_bytes):
    """A small device-pointer batch with the given offset tables.  -> (status, out_len, arena) on the host; arena was 0xEE."""
    import torch
    dev = torch.device("cuda:0")
    n = len(in_off) - 1
    blob = b"".join(cc.read(nm + ".compressed") for nm in names) + bytes(MARGIN)
    d_blob = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    d_in_off = torch.tensor(in_off, dtype=torch.int64, device=dev)
    d_out_off = torch.tensor(out_off, dtype=torch.int64, device=dev)
    arena = torch.full((arena_bytes + 2 * MARGIN,), FILL, dtype=torch.uint8, device=dev)
    d_len = torch.full((n,), -1, dtype=torch.int64, device=dev)
    d_status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.decode_batch_device(d_blob.data_ptr(), d_in_off.data_ptr(), n, arena.data_ptr() + MARGIN, d_out_off.data_ptr(), d_len.data_ptr(),
                            d_status.data_ptr())
    ctx.synchronize()
    return d_status.cpu().tolist(), d_len.cpu().tolist(), arena.cpu().numpy()


def _only_these_bytes(arena, written):
    """arena holds `written` = [(offset behind the margin, bytes)] and 0xEE everywhere else."""
    want = np.full(len(arena), FILL, dtype=np.uint8)
    for at, data in written:
        want[MARGIN + at:MARGIN + at + len(data)] = np.frombuffer(data, dtype=np.uint8)
    diff = np.flatnonzero(arena != want)
    assert not len(diff), (len(diff), int(diff[0]) - MARGIN)


def test_decreasing_out_off_pair_in_device_memory(ctx):
    """out_off = [0, 1000, 900, 2000, 3000] in device memory: stream 1's pair decreases -- zero capacity, status 25 with the oracle's
    out_len for capacity 0, nothing written for it.  The others are right.  (Stream 2's slot begins at 900, inside stream 0's slack:
    behind stream 2's own 20 bytes that slack is still 0xEE, as is every byte no valid stream owns.)"""
    names = ["quickfox", "quickfox", "10x10y", "x"]
    data = [cc.read(nm + ".compressed") for nm in names]
    exp = [cc.read(nm) for nm in names]
    in_off = np.concatenate([[0], np.cumsum([len(d) for d in data])]).tolist()
    out_off = [0, 1000, 900, 2000, 3000]
    status, out_len, arena = _offset_batch(ctx, names, in_off, out_off, 3000)
    w = oracle.decode_at(data[1], 0)
    assert w[0] == 25 and w[1] > 0
    assert status == [0, 25, 0, 0], status
    assert out_len == [len(exp[0]), w[1], len(exp[2]), len(exp[3])], out_len
    assert len(exp[0]) < 900 and 900 + len(exp[2]) < 1000
    _only_these_bytes(arena, [(0, exp[0]), (900, exp[2]), (2000, exp[3])])


def test_decreasing_in_off_pair_in_device_memory(ctx):
    """in_off = [0, a, 0, a, a + b]: stream 1's pair decreases -- an empty input, status 24 and out_len 0 as the oracle gives for no
    input at all; streams 0 and 2 (the same bytes) and stream 3 are right."""
    names = ["quickfox", "10x10y"]
    a, b = (len(cc.read(nm + ".compressed")) for nm in names)
    exp = [cc.read(nm) for nm in names]
    status, out_len, arena = _offset_batch(ctx, names, [0, a, 0, a, a + b], [0, 800, 1600, 2400, 3200], 3200)
    assert oracle.decode_at(b"", 800)[:2] == (24, 0)
    assert status == [0, 24, 0, 0], status
    assert out_len == [len(exp[0]), 0, len(exp[0]), len(exp[1])], out_len
    _only_these_bytes(arena, [(0, exp[0]), (1600, exp[0]), (2400, exp[1])])


@pytest.mark.parametrize("which", ["in_off", "out_off"])
def test_decreasing_offsets_in_host_memory_are_an_invalid_argument(ctx, which):
    """The same tables in host memory: BRX_ERR_INVALID_ARGUMENT, and neither status nor the output is written."""
    from brotli_rs_amd import brx
    names = ["quickfox", "10x10y"]
    a, b = (len(cc.read(nm + ".compressed")) for nm in names)
    blob = np.frombuffer(b"".join(cc.read(nm + ".compressed") for nm in names) + bytes(MARGIN), dtype=np.uint8)
    if which == "in_off":
        in_off, out_off = [0, a, 0, a, a + b], [0, 800, 1600, 2400, 3200]
    else:
        in_off, out_off = [0, a, a, a, a + b], [0, 1000, 900, 2000, 3000]
    in_off, out_off = np.array(in_off, dtype=np.uint64), np.array(out_off, dtype=np.uint64)
    out = np.full(3200, FILL, dtype=np.uint8)
    out_len = np.zeros(4, dtype=np.uint64)
    status = np.full(4, -1, dtype=np.int32)
    opts = brx._Opts(brx.MEM_HOST, 0, None)
    rc = brx.load_library().brx_decode_batch(ctx._h, blob.ctypes.data, in_off.ctypes.data, 4, out.ctypes.data, out_off.ctypes.data,
                                             out_len.ctypes.data, status.ctypes.data, ctypes.byref(opts))
    assert rc == -1  # BRX_ERR_INVALID_ARGUMENT
    assert status.tolist() == [-1] * 4 and (out == FILL).all() and not out_len.any()


def test_the_read_facade_retries_with_the_size_status_25_asked_for():
    """Seven Decompressors queued on one context before the first read: one batch.  The facade guesses 8 * in + 65536 bytes a stream
    and queues every status-25 stream again with max(4 * capacity, out_len): quickfox_repeated, zeros and backward65536 decode only
    through that retry.  Every stream reads back bit-exact, and the facade launched exactly the streams the rule, replayed on the
    oracle, predicts -- in at least two batches."""
    from brotli_rs_amd import brx
    names = ["quickfox_repeated", "zeros", "backward65536", "64x", "alice29.txt", "monkey", "x"]
    data = [cc.read(nm + ".compressed") for nm in names]
    r = sum(cc.facade_retries(d) for d in data)
    assert r >= 3
    c = brx_knobs.context(0)
    try:
        b0, s0 = c.facade_batches()
        decs = [brx.Decompressor(io.BytesIO(d), c).prepare() for d in data]
        got = [d.read() for d in decs]
        for d in decs:
            d.close()
        b1, s1 = c.facade_batches()
    finally:
        c.close()
    for nm, g in zip(names, got):
        assert g == cc.read(nm), nm
    assert b1 - b0 >= 2, (b0, b1)
    assert s1 - s0 == len(names) + r, (s0, s1, r)
