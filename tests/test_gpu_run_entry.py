"""The entry of a literal run in the resident loops of the assembly command loop (brx_hot.S, LIT_CTX_ENTRY) against the CPU oracle.

A run that follows copies finds its first context in the LAST TWO PENDING BYTES: the copies' bytes are still in the lanes of a
register, PFREE of them, when the run begins.  The full-chip build forms that context with all pending lanes at once -- every
lane looks up the context info of its byte, one shift by a lane joins the neighbours, lane PFREE - 1 is read -- the sparse-launch
build reads the two bytes and their info through v_readlane.  The streams here are groups of k copy-only commands behind the copy
of a command with literals, so that the next command's literals are entered with a chosen number of pending lanes.  What keeps the
copies pending is restated from the loop (.Lcopy, .Ldict, .Ldict_xform) and held by construction: the lanes in use, this copy
included, are at most 63 and at most the copy's distance; an identity dictionary word needs them to be at most 63; a transformed
word (no Uppercase form) needs at most 23 lanes in use before it.  Every literal tree has two symbols of its own, so each output byte
shows which tree, and with the context map which context id, the decoder used.

The builder counts, from what it emitted alone, the cells listed in _check_coverage and asserts them before anything runs on the GPU."""
import functools
import os
import random

import numpy as np
import pytest

import brx_knobs
import craft
import oracle_py as oracle

pytestmark = pytest.mark.gpu

N_STREAMS = 32
BUILDS = [{}, {"loop_build": 0}, {"loop_build": 1}]
# PFREE at a run's entry: both sides of every 16-lane row and of the 32-lane half, the smallest and the largest
PENDING = [p + 1 for p in (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 62)]
KINDS = ("far", "near", "dict", "suffix", "straddle")
CORNERS = (0x00, 0x7f, 0x80, 0xff)  # the four corners of the context-info table
RAW = 3072      # an uncompressed meta-block first: the flush cursor is aligned, the commands run in the assembly loop
PAIRS_AT = 16   # where the chosen byte pairs start in it
DICT = open(os.path.join(craft.ROOT, "brotli-rs_amd", "tables", "dictionary.bin"), "rb").read()
# RFC 7932 appendix B, the three transforms used here: (prefix, first word byte used, suffix)
TRANSFORMS = {0: (b"", 0, b""), 5: (b"", 0, b" the "), 26: (b"", 3, b"")}


def _id(opts):
    return "-".join("%s=%d" % kv for kv in sorted(opts.items())) or "default"


def _word(wl, idx, tid):
    prefix, first, suffix = TRANSFORMS[tid]
    at = craft.DOFFSET[wl] + idx * wl
    return prefix + DICT[at + first:at + wl] + suffix


def _p2_share(mode, byte):
    return craft.LUT[256 + byte] if mode == 2 else craft.LUT[512 + byte] if mode == 3 else 0


class _Builder:
    """One stream: [an uncompressed meta-block of chosen bytes,] one compressed meta-block of `ntrees` two-symbol literal trees behind
    a context map under `mode`.  lits(n) and copy(...) append a command and model it: the output, and the lanes pending behind it."""

    def __init__(self, seed, mode, ntrees, raw=True):
        self.rng = rng = random.Random(seed)
        self.mode, self.ntrees = mode, ntrees
        self.cmap = [(c + seed) % ntrees for c in range(64)]
        syms = rng.sample(range(256), 2 * ntrees)
        self.trees = [sorted(syms[2 * t:2 * t + 2]) for t in range(ntrees)]
        self.out = bytearray()
        self.pairs = {}  # (p2, p1) -> offset behind the pair in the uncompressed block
        if raw:
            data = bytearray(rng.randrange(256) for _ in range(RAW))
            want = [(a, b) for a in CORNERS for b in CORNERS] + self._share_pairs()
            for k, pr in enumerate(want):
                at = PAIRS_AT + 24 * k  # (22 random bytes in front of every pair: what a copy of up to 24 bytes that ends on it begins with)
                data[at + 22:at + 24] = bytes(pr)
                self.pairs[pr] = at + 24
            self.out += data
        self.start = len(self.out)
        self.cmds = []       # (literal bytes, copy length code, distance)
        self.pending = 0     # lanes in use behind the last command
        self.last_kind = None
        self.entries = []    # (pending lanes, kind of the last two, p2, p1, tree of the first literal, position) per run
        self.queued = None   # literals that ride on the next command

    def lits(self, n):
        """n literals: the entry of their run is recorded, they land everything; they ride on the next command (copy / end)."""
        assert not self.queued and n
        out, lits = self.out, bytearray()
        for k in range(n):
            p1 = out[-1] if len(out) >= 1 else 0
            p2 = out[-2] if len(out) >= 2 else 0
            t = self.cmap[craft.context_id(self.mode, p1, p2)]
            if k == 0:
                self.entries.append((self.pending, self.last_kind if self.pending else None, p2, p1, t, len(out)))
            x = self.rng.choice(self.trees[t])
            lits.append(x)
            out.append(x)
        self.pending, self.last_kind, self.queued = 0, None, bytes(lits)

    def end(self):
        self.cmds.append((self.queued, 0, None))

    def _share_pairs(self):
        """Two pairs with the same p1 whose context ids differ only in the p2 share AND whose trees differ (modes 2 and 3)."""
        if self.mode < 2:
            return []
        p1 = 0x41
        for a in range(256):
            for b in range(a + 1, 256):
                ia, ib = craft.context_id(self.mode, p1, a), craft.context_id(self.mode, p1, b)
                if _p2_share(self.mode, a) != _p2_share(self.mode, b) and self.cmap[ia] != self.cmap[ib]:
                    return [(a, p1), (b, p1)]
        return []

    def copy(self, copy):
        """One command: the queued literals and ("win", length, distance, kind) | ("dict", word length, index, transform id, kind)"""
        out, lits, self.queued = self.out, self.queued or b"", None
        if copy[0] == "win":
            _, n, dist, kind = copy
            assert 2 <= n and dist <= len(out)
            if n <= dist and self.pending + n <= min(dist, 63):
                self.pending += n   # joins the pending lanes (.Lcopy)
            elif n <= min(dist, 63):
                self.pending = n    # lands what is pending, then takes lanes of its own (.Lcopy_slow)
            else:
                self.pending = 0    # overlapping or long: written to the ring at once
            for _ in range(n):
                out.append(out[-dist])
            self.cmds.append((bytes(lits), n, dist))
        else:
            _, wl, idx, tid, kind = copy
            w = _word(wl, idx, tid)
            if tid == 0:
                self.pending = self.pending + wl if self.pending + wl <= 63 else wl   # (.Ldict)
            else:
                if self.pending > 23:
                    self.pending = 0                                                # (.Ldict_xform: 40 lanes must be free)
                self.pending = 0 if self.pending + len(w) == 1 else self.pending + len(w)
            self.cmds.append((bytes(lits), wl, len(out) + 1 + ((tid << craft.NDBITS[wl]) | idx)))
            out += w
        self.last_kind = kind

    def stream(self):
        b = craft.Bits()
        craft.stream_header(b, 22)
        if self.start:
            craft.raw_block(b, bytes(self.out[:self.start]))
        mlen = len(self.out) - self.start
        b.put(1, 1); b.put(0, 1)                 # ISLAST, not empty
        nib = 4 if mlen <= 1 << 16 else 5
        b.put(nib - 4, 2); b.put(mlen - 1, 4 * nib)
        b.put(0, 1); b.put(0, 1); b.put(0, 1)    # one block type per category
        b.put(0, 2); b.put(0, 4)                 # NPOSTFIX, NDIRECT
        b.put(self.mode, 2)
        craft.context_map(b, self.rng, self.ntrees, 64, cmap=self.cmap)
        craft.context_map(b, self.rng, 1, 4)
        for t in self.trees:
            craft.simple_code(b, t, 8)
        iac_of = lambda l, c: craft.iac_symbol(len(l), c if c else 2)
        iac = craft.complex_code(b, craft.uniform_lengths(704, {iac_of(l, c)[0] for l, c, d in self.cmds}), zero_run_17=True)
        dist = craft.complex_code(b, craft.uniform_lengths(64))
        treeof = {s: t for t in self.trees for s in t}
        for lits, c, d in self.cmds:
            sym, ie, ce = iac_of(lits, c)
            craft.put_sym(b, iac, sym)
            b.put(*ie)
            b.put(*ce)
            for x in lits:
                b.put(*craft.code_bits(treeof[x], x))
            if d is not None:
                code, ev, eb = craft.distance_code(d)
                craft.put_sym(b, dist, code)
                b.put(ev, eb)
        return b.bytes()


def _fill(B, lanes):
    """Copy-only commands from the ring that bring the pending lanes up to `lanes` (at least two more, or none)."""
    rng = B.rng
    while B.pending < lanes:
        left = lanes - B.pending
        n = min(left, rng.choice((2, 3, 5, 9, 14, 24)))
        if left - n == 1:
            n += -1 if n > 2 else 1  # (no copy of one byte)
        B.copy(("win", n, rng.randrange(max(B.pending + n, 64), min(len(B.out), 2000)), "near"))
    assert B.pending == lanes


def _group(B, lanes, kind, pair=None):
    """The copies that leave `lanes` lanes pending with last two bytes of `kind`; False when the kind cannot give that many lanes."""
    rng = B.rng
    if kind in ("far", "near"):
        n = min(lanes, rng.choice((2, 3, 4, 7, 12)))
        if lanes - n == 1:
            n = lanes
        _fill(B, lanes - n)
        if kind == "far":  # (behind the first 900 bytes of the uncompressed block: more than 2048 + 64 back)
            dist = len(B.out) - ((B.pairs[pair] if pair else rng.randrange(600, 900)) - n)
            assert dist > 2048 + 64
        else:
            dist = rng.randrange(max(lanes, 64), min(len(B.out), 2000))
        B.copy(("win", n, dist, kind))
    elif kind == "dict":
        if lanes < 4:
            return False
        wl = lanes if lanes <= 24 else rng.choice([w for w in range(4, 25) if lanes - w >= 2])
        _fill(B, lanes - wl)
        B.copy(("dict", wl, rng.randrange(1 << craft.NDBITS[wl]), 0, kind))
    elif kind == "suffix":  # word + " the ": the last two pending bytes are placed from the transform's record
        fits = [w for w in range(4, 25) if lanes - w - 5 == 0 or 2 <= lanes - w - 5 <= 23]
        if not fits:
            return False
        wl = rng.choice(fits)
        _fill(B, lanes - wl - 5)
        B.copy(("dict", wl, rng.randrange(1 << craft.NDBITS[wl]), 5, kind))
    else:  # straddle: a ONE-byte transformed word (OmitFirst3 of a four-letter one) behind another copy
        if not 2 <= lanes - 1 <= 23:
            return False
        _fill(B, lanes - 1)
        B.copy(("dict", 4, rng.randrange(1 << craft.NDBITS[4]), 26, kind))
    assert B.pending == lanes, (kind, lanes, B.pending)
    return True


def _build(i):
    """Stream i: 0 .. 29 = the four context modes over 2 .. 12 literal trees (every pair of the two is different: 4 and 11 are coprime),
    30 = one literal tree (the control: its loop has no contexts), 31 = no uncompressed block in front -- its first run starts at
    stream position 0 -- and no copies from beyond the ring."""
    mode, ntrees, raw = i % 4, 2 + i % 11, True
    if i == 30:
        mode, ntrees = 2, 1
    if i == 31:
        mode, ntrees, raw = 3, 3, False
    B = _Builder(100 + i, mode, ntrees, raw)
    rng = B.rng
    nl = lambda: rng.choice((1, 1, 2, 3, 4, 6))
    B.lits(6)  # the first run: nothing pending; at position 0 in stream 31
    if not raw:
        for _ in range(40):  # enough output for distances of 64 and more
            B.copy(("win", 2 + rng.randrange(3), 1 + rng.randrange(min(len(B.out), 9)), "near"))
            B.lits(nl())
    plan = [(p, k, None) for p in PENDING for k in KINDS if raw or k != "far"]
    plan += [(PENDING[j % len(PENDING)], "far", pr) for j, pr in enumerate(sorted(B.pairs))]
    rng.shuffle(plan)
    for lanes, kind, pair in plan:
        if _group(B, lanes, kind, pair):
            B.lits(nl())
    # a copy that overlaps its source lands everything: the next run is entered with nothing pending, mid-stream (the ring path)
    B.copy(("win", 10, 3, "near"))
    assert B.pending == 0
    for k in range(47):  # (the assembly loop hands the last 256 bits of a stream to the C++ loop: padding)
        B.lits(6)
        B.copy(("win", 2, 7, "near"))
    B.lits(6)
    B.end()
    return B


def _check_coverage(builders):
    """What the test is about, counted from what the builders emitted."""
    seen = {"lanes": set(), "kind": set(), "p1": set(), "p2": set(), "trees": set(), "nopend": set(), "share": set()}
    for i, B in enumerate(builders):
        by_p1 = {}
        for lanes, kind, p2, p1, tree, pos in B.entries:
            if lanes == 0:
                seen["nopend"].add(i)
                if pos < 2:
                    seen["start"] = i
                continue
            assert lanes >= 2
            if B.ntrees >= 2:
                seen["lanes"].add((B.mode, lanes)); seen["kind"].add((B.mode, kind)); seen["p1"].add((B.mode, p1)); seen["p2"].add((B.mode, p2))
                seen["trees"].add(B.ntrees)
                if B.mode >= 2 and any(t != tree and _p2_share(B.mode, q) != _p2_share(B.mode, p2) for q, t in by_p1.get(p1, ())):
                    seen["share"].add(B.mode)  # same p1, another p2 share, another tree: a wrong neighbour lane shows
                by_p1.setdefault(p1, set()).add((p2, tree))
            else:
                seen["control"] = i
    modes = range(4)
    assert seen["lanes"] >= {(m, p) for m in modes for p in PENDING}
    assert seen["kind"] >= {(m, k) for m in modes for k in KINDS}
    assert seen["p1"] >= {(m, c) for m in modes for c in CORNERS} and seen["p2"] >= {(m, c) for m in modes for c in CORNERS}
    assert seen["trees"] == set(range(2, 13)) and seen.get("control") == 30
    assert seen["share"] == {2, 3}
    assert seen["nopend"] == set(range(N_STREAMS)) and seen.get("start") == 31


@functools.lru_cache(maxsize=None)
def _streams():
    """[(stream, expected output)]; the coverage is asserted, and the oracle decodes every stream to what the builder's model of the
    context rules expects -- so the trees the builder counted are the trees the format means."""
    builders = [_build(i) for i in range(N_STREAMS)]
    _check_coverage(builders)
    res = []
    for B in builders:
        s, want = B.stream(), bytes(B.out)
        assert 150 <= len(B.cmds) <= 700, len(B.cmds)
        assert oracle.decode(s, 0, cap=len(want) + 16) == (0, want)
        res.append((s, want))
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


@pytest.mark.parametrize("opts", BUILDS, ids=_id)
def test_run_entry_with_pending_lanes(opts):
    """The 32 streams in one batch, under the default choice of the loop's build and under both builds forced: status, length and
    bytes are the oracle's."""
    S = _streams()
    c = brx_knobs.context(0, **opts)
    try:
        status, out_len, got = _decode(c, [s for s, _ in S], [len(w) + 16 for _, w in S])
    finally:
        c.close()
    bad = []
    for i, (_, want) in enumerate(S):
        if int(status[i]) != 0 or int(out_len[i]) != len(want) or got[i] != want:
            first = next((k for k, (a, b) in enumerate(zip(got[i], want)) if a != b), None)
            bad.append((i, int(status[i]), int(out_len[i]), len(want), first))
    assert not bad, (len(bad), bad[:8])
