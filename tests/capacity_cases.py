"""Output-capacity cases: (stream, capacity) pairs with the CPU oracle's status, out_len and bytes at exactly that capacity.
tests/test_capacity_cases.py checks the table; tests/test_gpu_capacity.py holds brx_decode_batch to it.

bro_decode applies the kernels' rule (out_room): an insert, a copy, a dictionary word or an uncompressed meta-block that does not
fit ends the stream with status 25 and out_len = the position in front of the item + the item's size."""
import collections
import functools
import os
import random

import craft
import oracle_py as oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
FIXTURES = ["alice29.txt", "backward65536", "quickfox_repeated", "compressed_repeated", "zeros", "monkey", "10x10y", "64x", "ukkonooa",
            "x", "empty", "quickfox"]
N_SAMPLED = 48

# stream: index into streams(); status / out_len: bro_decode's at capacity `cap`; the bytes: Stream.full[:n_bytes] (see Case docs below)
Case = collections.namedtuple("Case", "stream cap status out_len n_bytes")


class Stream:
    """name, data (compressed), status / full: the oracle's answer with ample room, L = len(full): the decoded length of a valid
    stream, the prefix in front of the error of an invalid one.  ends: output positions of the meta-block ends, where known."""

    def __init__(self, name, data, ends=()):
        self.name, self.data, self.ends = name, data, tuple(ends)
        self.status, self.full = oracle.decode(data)
        self.L = len(self.full)
        self.valid = self.status == 0


def read(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _dictionary_stream():
    D = bytes(oracle.lib().bro_dictionary()[:122784])
    refs = [(t, 17 * t + 1) for t in (0, 12, 23, 3, 49, 64, 73, 120, 44)]
    s, e = craft.dictionary_stream(7, refs, 307, True, oracle.transform, D)
    assert e is not None
    return s, e


def _meta_blocks_stream():
    """Four compressed meta-blocks of a few hundred bytes each, wbits 16 -> (stream, expected, [end of every meta-block])."""
    rng = random.Random(41)
    b = craft.Bits()
    craft.stream_header(b, 16)
    out, ends = bytearray(), []
    n_mb = 4
    for k in range(n_mb):
        start, cmds = len(out), []
        for j in range(24 + 5 * k):
            lits = bytes(rng.randrange(97, 123) for _ in range(2 + rng.randrange(9)))
            out += lits
            dist = 1 + rng.randrange(min(len(out), 200))
            n = 2 + rng.randrange(8)
            cmds.append((lits, n, dist))
            for _ in range(n):
                out.append(out[-dist])
        craft.MetaBlock(cmds, mlen=len(out) - start).emit(b, k == n_mb - 1, 0)
        ends.append(len(out))
    return b.bytes(), bytes(out), ends


def _raw_stream(n, seed):
    """One uncompressed meta-block of n bytes (from 8192 bytes on the kernel copies it in bulk) and a short compressed one behind it."""
    rng = random.Random(seed)
    data = bytes(rng.getrandbits(8) for _ in range(n))
    tail = b"behind the uncompressed meta-block"
    b = craft.Bits()
    craft.stream_header(b, 18)
    craft.raw_block(b, data)
    craft.MetaBlock([(tail[:9], 4, 3), (tail[9:], 0, None)], mlen=len(tail) + 4).emit(b, True, 0)
    out = bytearray(data + tail[:9])
    for _ in range(4):
        out.append(out[-3])
    return b.bytes(), bytes(out) + tail[9:], [n]


@functools.lru_cache(maxsize=None)
def streams():
    """Every stream of the table, in a fixed order."""
    out = [Stream(n, read(n + ".compressed")) for n in FIXTURES]

    def crafted(name, s, e, ends=()):
        st = Stream(name, s, ends)
        assert st.valid and st.full == e, name  # (the model of craft.py and the oracle agree)
        out.append(st)

    crafted("dictionary_words", *_dictionary_stream())
    crafted("farcopy_8192_65536", *craft.farcopy_stream(3, 8192, 1 << 16))
    crafted("four_meta_blocks", *_meta_blocks_stream())
    crafted("raw_9000", *_raw_stream(9000, 5))      # bulk-copy path (>= 8192 bytes)
    crafted("raw_8000", *_raw_stream(8000, 6))      # its twin below the threshold
    crafted("level1_tables", *craft.growing_tables_stream(77, [105], mode=2, n_cmds=500))
    crafted("late_hand_up", *craft.growing_tables_stream(401, [2, 2, 105, 2, 150], mode=1, n_cmds=300, first_dist=2047))
    alice = read("alice29.txt.compressed")
    flipped = bytearray(alice)
    flipped[30000] ^= 0x40
    out.append(Stream("alice29_bitflip_30000", bytes(flipped)))
    out.append(Stream("alice29_cut_60_percent", alice[:len(alice) * 60 // 100]))
    assert not out[-1].valid and not out[-2].valid
    return tuple(out)


def _case(si, cap, flags=0):
    s = streams()[si]
    status, out_len, got = oracle.decode_at(s.data, cap, flags)
    if status == oracle.STATUS_OUTPUT_TOO_SMALL:  # (the slot's bytes are not specified under status 25)
        return Case(si, cap, status, out_len, 0)
    assert got == s.full[:len(got)], (s.name, cap)  # the oracle's bytes at this capacity are the shared reference's: keep no copy
    return Case(si, cap, status, out_len, len(got))


def capacities(si):
    """The capacities of stream si (sorted): the fixed ones, a seeded sample below L, both sides of every item's end the oracle
    reports for one of those (needed - 1, needed), and both sides of every known meta-block end."""
    s = streams()[si]
    L = s.L
    caps = {0, 1, 15, 16, 17, L // 2, L - 1, L, L + 1}
    rng = random.Random(1000 + si)
    caps.update(rng.randrange(L) for _ in range(N_SAMPLED if L else 0))
    caps = {max(c, 0) for c in caps}
    for c in sorted(caps):
        status, needed, _ = oracle.decode_at(s.data, c)
        if status == oracle.STATUS_OUTPUT_TOO_SMALL:
            caps.update((needed - 1, needed))
    for e in s.ends:
        caps.update((e - 1, e, e + 1))
    return sorted(max(c, 0) for c in caps)


@functools.lru_cache(maxsize=None)
def table():
    """Every case, grouped by stream, capacities rising."""
    return tuple(_case(si, c) for si in range(len(streams())) for c in capacities(si))


def tree_walk_table():
    """The same cases decoded in the oracle's tree-walk mode (the reference's own Huffman lookup)."""
    return tuple(_case(c.stream, c.cap, oracle.FLAG_TREE_WALK) for c in table())


def case_bytes(c):
    """The oracle's output bytes of a case whose status is not 25."""
    return streams()[c.stream].full[:c.n_bytes]


@functools.lru_cache(maxsize=None)
def guard_cases():
    """About 200 cases for the tests that look at memory around the slots, every stream among them: room to spare (L + 0 / 1 / 7 /
    13), the smallest slots (0, 1), one byte short (L - 1), and one byte short of an item's end (needed - 1 of up to five status-25
    cases of the table, spread over the stream, the last one among them)."""
    by_stream = collections.defaultdict(list)
    for c in table():
        if c.status == oracle.STATUS_OUTPUT_TOO_SMALL:
            by_stream[c.stream].append(c.out_len)
    out = []
    for si, s in enumerate(streams()):
        caps = {s.L + pad for pad in (0, 1, 7, 13)} | {0, 1, max(s.L - 1, 0)}
        v = sorted(set(by_stream[si]))
        caps.update(x - 1 for x in v[::max(1, len(v) // 4)][:4] + v[-1:])
        out += [_case(si, c) for c in sorted(caps)]
    return tuple(out)


def facade_retries(data):
    """How often the Read facade decodes a stream again: its first slot is 8 * len + 65536 bytes, every slot is rounded up to 16, and
    a status-25 stream is queued again with max(4 * capacity, out_len).  Replayed on the oracle."""
    cap, r = 8 * len(data) + 65536, 0
    while True:
        status, needed, _ = oracle.decode_at(data, (cap + 15) & ~15)
        if status != oracle.STATUS_OUTPUT_TOO_SMALL:
            return r
        cap, r = max(4 * cap, needed), r + 1
