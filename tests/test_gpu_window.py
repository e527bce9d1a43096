"""The bit window of the assembly command loop (brx_hot.S, TAKE / REFILL_CORE) against the CPU oracle.

The full-chip build of the loop keeps the window as a fixed pair of input dwords and a count S of the bits consumed from it; a field
of n bits moves the pair on exactly when S + n >= 32.  The streams here put the widest fields the format has -- 24 extra bits
of insert code 23 and of copy code 23, distance symbols with 1 .. 24 extra bits -- and fields of no bits at all next to that
boundary, at every bit phase: the builder counts, on the CPU, that every kind of field lands on S + n = 32 and on S + n = 31."""
import functools
import io
import random

import numpy as np
import pytest

import brx_knobs
import craft
import oracle_py as oracle

pytestmark = pytest.mark.gpu

N_STREAMS = 32
KINDS = ("iac", "insert_extra", "copy_extra", "literal", "distance", "distance_extra")
# the default choice of the loop's build, and both builds forced
BUILDS = [{}, {"loop_build": 0}, {"loop_build": 1}]


def _id(opts):
    return "-".join("%s=%d" % kv for kv in sorted(opts.items())) or "default"


class _LogBits(craft.Bits):
    """A bit writer that remembers (position, width) of every field."""

    def __init__(self):
        super().__init__()
        self.log = []

    def put(self, value, nbits):  # (Bits.put restated: a million literals go through here)
        self.log.append((self.n, nbits))
        self.acc |= value << self.nacc
        self.nacc += nbits
        self.n += nbits
        if self.nacc >= 64:
            self.buf += (self.acc & 0xffffffffffffffff).to_bytes(8, "little")
            self.acc >>= 64
            self.nacc -= 64

    def bytes(self):
        k = (self.nacc + 7) >> 3
        return bytes(self.buf) + self.acc.to_bytes(k, "little")


def _commands(seed):
    """About 64 commands and their output.  Command 0 (a quarter of the seeds: command 20 as well) has insert code 23 -- 22 594 literals and more,
    24 extra bits; every fourth command has copy code 23 (2 118 bytes and more, 24 extra bits), the extra values small; the others
    mix inserts and copies with and without extra bits, explicit distances from 1 to the whole output so far (1 .. 15 extra bits),
    last-distance codes (no extra bits) and implicit distances (no distance symbol).  Odd seeds end with a distance symbol of the
    widest fields there are -- 22 extra bits, the most a window of 24 bits can name, or the format's 24: that distance is a
    dictionary reference with an impossible transform, the stream is invalid there."""
    rng = random.Random(7000 + seed)
    out, cmds = bytearray(), []

    def add(lits, clen, d):
        out.extend(lits)
        cmds.append((lits, clen, d))
        dist = last[0] if d == "implicit" or isinstance(d, tuple) else d
        last[0] = dist
        for _ in range(clen):
            out.append(out[-dist])

    last = [4]  # (the ring's most recent distance at the start of a stream)
    for k in range(62 + seed % 5):
        if k == 0 or (k == 20 and seed % 4 == 1):
            lits = rng.randbytes(22594 + rng.randrange(40))
        else:
            lits = rng.randbytes(rng.choice((0, 0, 1, 2, 3, 5, 6, 9, 19, 70)))
        if k % 4 == 0:
            clen = 2118 + rng.randrange(50)
        else:
            clen = rng.choice((2, 3, 4, 5, 7, 9, 10, 13, 25, 60, 140))
        reach = len(out) + len(lits)
        pick = rng.randrange(8)
        if k and pick == 0 and len(lits) < 6 and clen < 70:
            d = "implicit"
        elif k and pick == 1:
            d = ("code", 0)  # the last distance again, by its symbol
        else:
            d = max(1, min(reach, 1 << rng.randrange(1, 18)) - rng.randrange(3))
        add(lits, clen, d)
    bad = None
    if seed % 2:
        bad = (1 << 23) + 5 + seed if seed % 4 == 1 else (1 << 25) + 9 + seed
        cmds.append((rng.randbytes(2), 4, bad))
    return cmds, bytes(out), bad


def _fields(cmds, log):
    """(kind index, position, width) of every command field as three arrays, from the tail of the writer's log."""
    kinds = []
    for lits, clen, d in cmds:
        kinds += [0, 1, 2]
        kinds += [3] * len(lits)
        if d is not None and d != "implicit":
            kinds += [4, 5]
    tail = np.array(log[len(log) - len(kinds):], dtype=np.int64)
    return np.array(kinds), tail[:, 0], tail[:, 1]


@functools.lru_cache(maxsize=None)
def _streams():
    """[(stream, oracle status, oracle output)] of the 32 streams.  Asserts the coverage the test is about: with the streams at any
    of the four byte phases of a dword, every kind of field has a take that ends exactly on the pair's boundary (S + n = 32) and
    one that ends one bit short of it (S + n = 31); the widest insert, copy and distance fields are all there."""
    hit = {(p, kind, t): 0 for p in range(4) for kind in KINDS for t in (31, 32)}
    widest = dict.fromkeys(KINDS, 0)
    rev, craft.rev = craft.rev, functools.lru_cache(maxsize=None)(craft.rev)  # (a million literals: the bit reversal once per code)
    try:
        built = []
        for seed in range(N_STREAMS):
            cmds, out, bad = _commands(seed)
            b = _LogBits()
            craft.stream_header(b, 24)
            craft.MetaBlock(cmds, mlen=len(out) + (6 if bad else 0)).emit(b, True, len(out))
            kinds, pos, n = _fields(cmds, b.log)
            for k, kind in enumerate(KINDS):
                widest[kind] = max(widest[kind], int(n[kinds == k].max()))
                for p in range(4):
                    t = ((pos + 8 * p) % 32 + n)[(kinds == k) & (n > 0)]
                    hit[(p, kind, 31)] += int((t == 31).sum())
                    hit[(p, kind, 32)] += int((t == 32).sum())
            built.append((b.bytes(), out, bad))
    finally:
        craft.rev = rev
    missing = [k for k, v in hit.items() if not v]
    assert not missing, missing
    assert widest["insert_extra"] == 24 and widest["copy_extra"] == 24 and widest["distance_extra"] == 24, widest
    res = []
    for stream, out, bad in built:
        assert len(out) < (256 << 10)
        st, got = oracle.decode(stream, 0, cap=256 << 10)
        if bad:
            assert st not in (0, 25) and got[:len(out)] == out[:len(got)], (st, len(got), len(out))
        else:
            assert st == 0 and got == out, (st, len(got), len(out))
        res.append((stream, st, got))
    assert sum(1 for _, st, _ in res if st == 0) == N_STREAMS // 2
    return res


def _decode(ctx, streams, caps):
    """-> (status, out_len, [the slot's first min(out_len, capacity) bytes])"""
    n = len(streams)
    in_off = np.zeros(n + 1, dtype=np.uint64)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    in_off[1:] = np.cumsum([len(s) for s in streams])
    out_off[1:] = np.cumsum(caps)
    blob = np.frombuffer(b"".join(streams) + bytes(64), dtype=np.uint8)
    out = np.zeros(int(out_off[-1]) + 64, dtype=np.uint8)
    status, out_len = ctx.decode_batch_host_raw(blob.ctypes.data, in_off, n, out.ctypes.data, out_off)
    got = [out[int(out_off[i]):int(out_off[i]) + min(int(out_len[i]), caps[i])].tobytes() for i in range(n)]
    return status, out_len, got


def _mismatches(want, status, out_len, got):
    """want: [(oracle status, oracle output)].  A valid stream: status, length and bytes; an invalid one: the status, and the bytes in
    front of the error as far as both sides report them (how far into the failing command out_len points is not specified)."""
    bad = []
    for i, (st, ref) in enumerate(want):
        if int(status[i]) != st:
            bad.append((i, "status", st, int(status[i])))
        elif st == 0 and (int(out_len[i]) != len(ref) or got[i] != ref):
            bad.append((i, "bytes", len(ref), int(out_len[i])))
        elif st != 0 and got[i][:len(ref)] != ref[:len(got[i])]:
            bad.append((i, "prefix", len(ref), int(out_len[i])))
    return bad


@pytest.mark.parametrize("opts", BUILDS, ids=_id)
def test_widest_fields_at_every_bit_phase(opts):
    """(a) Every one of the 32 streams at every one of the four byte phases of the batch's input -- a pad stream of 1 .. 3 bytes in
    front of a copy puts it there, so what runs is what the builder counted -- against the oracle: status, length, bytes."""
    S = _streams()
    streams, want, at, placed = [], [], 0, set()
    for p in range(4):
        for k, (stream, st, ref) in enumerate(S):
            pad = (p - at) % 4
            if pad:
                streams.append(bytes(pad))
                want.append(oracle.decode(bytes(pad), 0, cap=64))
                at += pad
            placed.add((k, at % 4))
            streams.append(stream)
            want.append((st, ref))
            at += len(stream)
    assert placed == {(k, p) for k in range(len(S)) for p in range(4)}
    c = brx_knobs.context(0, **opts)
    try:
        status, out_len, got = _decode(c, streams, [len(w[1]) + 16 for w in want])
    finally:
        c.close()
    bad = _mismatches(want, status, out_len, got)
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("opts", BUILDS, ids=_id)
def test_fields_of_no_bits_next_to_the_boundary(opts):
    """(b) One-symbol insert&copy and distance codes take no bits: a take of 0 never moves the pair on, whatever S is.  The periodic
    streams with such codes, one to three units, every unit of the stream starting at another byte; and 300 short commands under
    both one-symbol codes with 3-bit literals, so that the zero-bit symbols fall on every S, 31 included."""
    streams, want = [], []
    for seed, kw in ((31, dict(single_iac=True)), (32, dict(single_dist=True)), (33, dict(single_iac=True, single_dist=True))):
        prefix, unit, final, unit_out = craft.periodic_stream_parts(seed, raw=True, literals=(64 << 10) + 37 + seed, **kw)
        for k in (1, 2, 3):
            streams.append(prefix + unit * k + final)
            want.append((0, unit_out * k))
    lens = [3] * 8 + [0] * 248
    for seed in range(6):
        rng = random.Random(90 + seed)
        out, cmds = bytearray(), []
        for k in range(300):
            lits = bytes(rng.randrange(8) for _ in range(1 + seed % 3))
            out += lits
            cmds.append((lits, 3, 1 + seed % 3))
            for _ in range(3):
                out.append(out[-(1 + seed % 3)])
        b = craft.Bits()
        craft.stream_header(b, 22)
        craft.MetaBlock(cmds, mlen=len(out), lit_lengths=lens, single_iac=True, single_dist=True).emit(b, True, len(out))
        streams.append(b.bytes())
        want.append((0, bytes(out)))
    for s, (st, ref) in zip(streams, want):
        assert oracle.decode(s, 0, cap=len(ref) + 16) == (st, ref)
    c = brx_knobs.context(0, **opts)
    try:
        status, out_len, got = _decode(c, streams, [len(w[1]) + 16 for w in want])
    finally:
        c.close()
    bad = _mismatches(want, status, out_len, got)
    assert not bad, (len(bad), bad[:8])


@functools.lru_cache(maxsize=None)
def _cuts():
    """(streams, [(oracle status, oracle output)], capacities): every stream of (a) cut at every byte of its last 48 bytes.  The
    oracle and the kernels get the same capacity, what the whole stream needs and a little more, so that no cut stream ends on it."""
    streams, want, caps = [], [], []
    for stream, _, full in _streams():
        for cut in range(1, 49):
            s = stream[:len(stream) - cut]
            st, ref = oracle.decode(s, 0, cap=len(full) + 64)
            assert st not in (0, 25), (st, cut)
            streams.append(s)
            want.append((st, ref))
            caps.append(len(full) + 64)
    return streams, want, caps


@pytest.mark.parametrize("opts", BUILDS, ids=_id)
def test_truncation_in_the_last_48_bytes(opts):
    """(c) Every stream of (a) cut at every byte of its last 48 bytes, one batch: the loop runs on behind the real end, is
    poisoned there and the kernel goes back.  Status and the bytes in front of the error are the oracle's."""
    streams, want, caps = _cuts()
    c = brx_knobs.context(0, **opts)
    try:
        status, out_len, got = _decode(c, streams, caps)
    finally:
        c.close()
    bad = _mismatches(want, status, out_len, got)
    assert not bad, (len(bad), bad[:8])


def _read_all(d):
    """-> (bytes read, the error's text or None)"""
    got = bytearray()
    try:
        while True:
            part = d.read(1 << 16)
            if not part:
                return bytes(got), None
            got += part
    except ValueError as e:
        return bytes(got), str(e)


def test_bounded_reader_keeps_its_margin_in_front_of_the_end():
    """(d) The streams of (a) through the pulled reader with its smallest window (1 MiB: each is resident as a whole): the loop is
    poisoned END_MARGIN dwords in front of the end of the stream and the C++ loop finishes with the exact rules.  Valid streams read
    back bit-exact; an invalid one serves bytes of the oracle's prefix and then raises the oracle's error."""
    from brotli_rs_amd import brx
    c = brx_knobs.context(0)
    try:
        c.set_option("reader_window", 1 << 20)
        for i, (stream, st, ref) in enumerate(_streams()):
            d = brx.Decompressor(io.BytesIO(stream), c, streaming=True)
            got, err = _read_all(d)
            d.close()
            if st == 0:
                assert err is None and got == ref, (i, err, len(got), len(ref))
            else:
                assert err is not None and [k for k in range(1, 28) if brx.status_str(k) == err] == [st], (i, err, st)
                assert got[:len(ref)] == ref[:len(got)], (i, len(got), len(ref))
    finally:
        c.close()


def test_bounded_reader_margin_in_front_of_the_resident_end():
    """(d) One stream LONGER than the reader's window: the meta-blocks of the 16 valid streams of (a), each behind an empty metadata
    block (so that a unit is whole bytes), four times over -- 1.5 MB of input through a window of 1 MiB.  The first slices end with
    more input to come: the loop is poisoned END_MARGIN dwords in front of the end of what is resident, hands the command at that
    end back, and goes on when the window has moved.  Bit-exact against the units' outputs, which the oracle confirms."""
    from brotli_rs_amd import brx

    def empty_metadata(b):
        b.put(0, 1); b.put(3, 2); b.put(0, 1); b.put(0, 2)  # ISLAST = 0, MNIBBLES code 3, reserved, MSKIPBYTES = 0
        b.put(0, (-b.n) % 8)

    b = craft.Bits()
    craft.stream_header(b, 24)
    empty_metadata(b)
    parts, outs = [b.bytes()], []
    rev, craft.rev = craft.rev, functools.lru_cache(maxsize=None)(craft.rev)
    try:
        for seed in range(0, N_STREAMS, 2):
            cmds, out, bad = _commands(seed)
            assert bad is None
            b = _LogBits()
            craft.MetaBlock(cmds, mlen=len(out)).emit(b, False, len(out))
            empty_metadata(b)
            assert b.n % 8 == 0
            parts.append(b.bytes())
            outs.append(out)
    finally:
        craft.rev = rev
    stream = parts[0] + b"".join(parts[1:]) * 4 + b"\x03"
    want = b"".join(outs) * 4
    assert len(stream) > (1 << 20) + (1 << 18)
    assert oracle.decode(stream, 0, cap=len(want) + 64) == (0, want)
    c = brx_knobs.context(0)
    try:
        c.set_option("reader_window", 1 << 20)
        d = brx.Decompressor(io.BytesIO(stream), c, streaming=True)
        got, err = _read_all(d)
        d.close()
    finally:
        c.close()
    assert err is None and got == want, (err, len(got), len(want))
