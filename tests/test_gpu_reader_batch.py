"""Reader rounds (include/brx.h, brx_stream_advance): the slices of many bounded / pulled streams of one context in shared launches
of the resumable kernel over per-stream descriptors (BrxReaderDesc).  Driven from one thread with brx_stream_advance and from many
threads with brx_stream_read; results against the inputs and against the same streams decoded one slice per launch
(BRX_OPTION_READER_BATCH = 0)."""
import ctypes
import os
import random
import subprocess
import threading

import pytest

import brx_knobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
TEXTS = ["lcet10.txt", "plrabn12.txt", "alice29.txt", "asyoulik.txt"]
MIB = 1 << 20


def _read(name):
    with open(os.path.join(DATA, name), "rb") as f:
        return f.read()


def _text(rng, n):
    """n bytes of the golden texts from a random offset, one byte in 4 KiB changed (no two streams alike)."""
    corpus = b"".join(_read(t) for t in TEXTS)
    start = rng.randrange(len(corpus))
    reps = (start + n) // len(corpus) + 1
    out = bytearray((corpus * reps)[start:start + n])
    for i in range(0, n, 4096):
        out[i] = rng.randrange(256)
    return bytes(out)


class _Stream:
    """One brx_stream over the raw C ABI: bounded over a buffer, or pulled through a callback with random piece sizes."""

    def __init__(self, ctx, comp, pulled, seed=0, over_cap=False):
        from brotli_rs_amd import brx
        self.lib = brx.load_library()
        self.comp, self.at, self.rng = comp, 0, random.Random(seed)
        if pulled:
            def pull(_user, buf, cap):
                if over_cap:
                    return cap + 1
                k = min(len(self.comp) - self.at, 1 + self.rng.randrange(min(cap, 3 * MIB)))
                ctypes.memmove(buf, self.comp[self.at:self.at + k], k)
                self.at += k
                return k
            self.cb = brx.READ_FN(pull)
            self.h = self.lib.brx_stream_new_reader(ctx._h, self.cb, None)
        else:
            self.h = self.lib.brx_stream_new_bounded(ctx._h, comp, len(comp))
        assert self.h
        self.buf = ctypes.create_string_buffer(4 * MIB)
        self.out = bytearray()
        self.end = None  # 0, -status or -1000 + BRX_ERR_*

    def ready(self):
        return self.lib.brx_stream_ready(self.h)

    def read(self, n):
        r = self.lib.brx_stream_read(self.h, self.buf, min(n, len(self.buf)))
        if r > 0:
            self.out += ctypes.string_at(self.buf, r)
        elif self.end is None:
            self.end = r
        return r

    def drain_ready(self):
        while self.ready() > 0:
            assert self.read(self.ready()) > 0

    def read_to_end(self):
        while self.end is None:
            self.read(len(self.buf))
        return self.end

    def free(self):
        if self.h:
            self.lib.brx_stream_free(self.h)
            self.h = None


def _advance(ctx, streams):
    from brotli_rs_amd import brx
    arr = (ctypes.c_void_p * len(streams))(*[s.h for s in streams])
    rc = brx.load_library().brx_stream_advance(arr, len(streams))
    assert rc >= 0, brx.load_library().brx_last_error()
    return rc


def _drive(ctx, streams):
    """brx_stream_advance + brx_stream_read only (reads of decoded bytes, never one that decodes) until no stream moves on."""
    calls = slices = 0
    while True:
        k = _advance(ctx, streams)
        if k == 0:
            break
        calls += 1
        slices += k
        for s in streams:
            s.drain_ready()
    for s in streams:
        s.read_to_end()
    return calls, slices


def _alone(comp, pulled, seed):
    """The same stream decoded one slice per launch on a context of its own: status and served bytes."""
    c = brx_knobs.context(0, reader_batch=0)
    try:
        s = _Stream(c, comp, pulled, seed)
        end = s.read_to_end()
        out = bytes(s.out)
        s.free()
        return end, out
    finally:
        c.close()


def test_round_robin_advance_is_bit_exact():
    """32 generator streams (adaptive and greedy, 6 .. 20 MiB of output, meta-blocks of 64 KiB .. 16 MiB) and four odd ones -- cut in
    the middle of a meta-block, one byte flipped, an empty input, a crafted stream with a 7 MiB copy (the window's buffer has to grow:
    BrxResume::need_room) -- half bounded over buffers, half pulled through callbacks with random piece sizes, driven with
    brx_stream_advance + brx_stream_read only.  Valid streams give their inputs back; invalid ones give the status and the bytes that
    the same stream gives alone, one slice per launch.  One launch per advance call, several slices in it."""
    import craft
    rng = random.Random(71)
    c = brx_knobs.context(0)
    try:
        # (the greedy generator runs one GPU thread per stream: its streams are kept short, 6 .. 9 MiB)
        combos = [(True, mb) for mb in (64 << 10, 256 << 10, MIB, 4 * MIB, 16 * MIB)] + [(False, mb) for mb in (64 << 10, MIB, 16 * MIB)]
        srcs, comps = [], []
        for adaptive, mb in combos:
            group = [_text(rng, rng.randrange(6 * MIB, (20 if adaptive else 9) * MIB)) for _ in range(4)]
            srcs += group
            comps += c.generate_batch(group, metablock_bytes=mb, adaptive=adaptive)
        assert len(srcs) == 32
        big, big_want = craft.takeback_stream(5, 4, [(5000, (7 << 20) + 5, 8), (6, 2, 1500)])
        cut = comps[3][: len(comps[3]) * 3 // 5]
        flip = bytearray(comps[9])
        flip[len(flip) * 2 // 5] ^= 0x5A
        odd = [cut, bytes(flip), b""]
        streams = [_Stream(c, x, pulled=i % 2 == 1, seed=i) for i, x in enumerate(comps + [big] + odd)]
        l0, s0, g0 = c.reader_slice_launches(), c.reader_slices(), c.stream_regrown()
        calls, slices = _drive(c, streams)
        launches, in_them = c.reader_slice_launches() - l0, c.reader_slices() - s0
        assert launches == calls and in_them == slices, (launches, calls, in_them, slices)
        assert in_them >= 4 * launches, (launches, in_them)
        assert c.stream_regrown() > g0  # (the 7 MiB copy)
        for i, (s, want) in enumerate(zip(streams, srcs + [big_want])):
            assert s.end == 0 and len(s.out) == len(want) and s.out == want, (i, s.end, len(s.out), len(want))
        for k, s in enumerate(streams[33:]):
            i = 33 + k
            end, out = _alone(odd[k], pulled=i % 2 == 1, seed=i)
            assert s.end == end and bytes(s.out) == out, (i, s.end, end, len(s.out), len(out))
            assert end < 0 or k == 1, (i, end)  # (a flipped byte may, rarely, still make a valid stream)
        for s in streams:
            s.free()
    finally:
        c.close()


def test_reader_batch_option_is_accepted_and_unknown_ones_are_not():
    from brotli_rs_amd import brx
    c = brx_knobs.context(0)
    try:
        lib = brx.load_library()
        assert lib.brx_ctx_set_option(c._h, 15, 0) == 0 and lib.brx_ctx_set_option(c._h, 15, 1) == 0
        assert lib.brx_ctx_set_option(c._h, 15, 2) == -1
        assert lib.brx_ctx_set_option(c._h, 9999, 1) == -1
        # brx_stream_advance's argument checks: NULL entries, streams of two contexts
        c2 = brx_knobs.context(0)
        a, b = _Stream(c, b"", False), _Stream(c2, b"", False)
        assert lib.brx_stream_advance((ctypes.c_void_p * 2)(a.h, None), 2) == -1
        assert lib.brx_stream_advance((ctypes.c_void_p * 2)(a.h, b.h), 2) == -1
        assert lib.brx_stream_advance(None, 0) == 0
        a.free()
        b.free()
        c2.close()
    finally:
        c.close()


def test_readers_on_many_threads_share_launches(tmp_path):
    """tests/cpp/reader_threads.cpp, through host/decompressor.hpp: 32 threads start together, each reads a pulled Decompressor of 8 .. 16
    MiB in 64 KiB reads -- every byte right, and at least four slices per launch; the same with BRX_OPTION_READER_BATCH = 0 gives one
    slice per launch.  And one thread moving 8 Decompressors on with brotli::advance, reading what ready() says: right, and shared
    launches."""
    exe = str(tmp_path / "reader_threads")
    lib = os.path.join(ROOT, "brotli-rs_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "reader_threads.cpp"), "-o", exe, "-L", lib, "-lbrx",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"])
    texts = [os.path.join(DATA, t) for t in TEXTS]

    def run(mode, batch, streams, lo, hi):
        out = subprocess.run([exe, mode, str(batch), str(streams), str(lo), str(hi)] + texts, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        line = [ln for ln in out.stdout.splitlines() if "launches" in ln][-1]
        words = line.split("launches")[1].split()
        return float(words[0]), float(words[2]), line

    launches, slices, line = run("threads", 1, 32, 8, 16)
    assert launches > 0 and slices >= 4 * launches, line
    launches, slices, line = run("threads", 0, 6, 8, 9)
    assert launches > 0 and slices == launches, line
    launches, slices, line = run("advance", 1, 8, 8, 10)
    assert launches > 0 and slices >= 2 * launches, line


def _hip_mem_used():
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return total.value - free.value


def _spilling_stream(raw):
    """A stream that claims its spill slab at its first meta-block and keeps it: craft.growing_tables_stream's meta-block of 200 literal
    trees (more table memory than the regular kernel's LDS holds -- under a reader its tables go to the stream's slab), then `raw` in
    uncompressed meta-blocks of 64 KiB inserted in front of its short last meta-block.  -> (stream, expected output from the oracle)."""
    import craft
    import oracle_py
    from unittest import mock
    header = craft._mb_header

    def with_raw_in_front_of_the_last(b, mlen, is_last=True):
        if is_last:
            for k in range(0, len(raw), 1 << 16):
                craft.raw_block(b, raw[k:k + (1 << 16)])
        header(b, mlen, is_last)

    with mock.patch.object(craft, "_mb_header", with_raw_in_front_of_the_last):
        stream = craft.growing_tables_stream(91, [200, 1], n_cmds=30)[0]
    st, out = oracle_py.decode(stream, 0, cap=len(raw) + 4096)
    assert st == 0 and len(out) > len(raw)
    return stream, out


def test_freeing_paused_streams_between_rounds_leaks_nothing():
    """200 times: a stream of 6 MiB whose first meta-block spills its tables into the stream's own slab is made, moved on by one slice
    next to three long text streams (it pauses at about 4 MiB, holding its slab) and freed while paused.  Its buffers and its slab go
    back -- the device memory in use does not grow (hipMemGetInfo) -- rounds never touch the context's own slab pool (counter 13), and
    the three others finish bit-exact."""
    rng = random.Random(72)
    c = brx_knobs.context(0)
    try:
        srcs = [_text(rng, 24 * MIB) for _ in range(3)]
        comps = c.generate_batch(srcs, metablock_bytes=MIB, adaptive=True)
        others = [_Stream(c, x, pulled=i == 1, seed=i) for i, x in enumerate(comps)]
        spill, spill_want = _spilling_stream(rng.randbytes(6 * MIB))
        used0 = slabs0 = None
        for k in range(200):
            s = _Stream(c, spill, pulled=k % 2 == 1, seed=k)
            assert _advance(c, others + [s]) >= 1
            assert 0 < s.ready() < len(spill_want)
            assert s.read(s.ready()) > 0 and s.out == spill_want[: len(s.out)]
            s.free()
            for o in others:
                o.drain_ready()
            if k == 9:
                used0, slabs0 = _hip_mem_used(), c.pool_slabs()
        assert _hip_mem_used() <= used0 + 64 * MIB, (used0, _hip_mem_used())
        assert c.pool_slabs() == slabs0
        _drive(c, others)
        for o, want in zip(others, srcs):
            assert o.end == 0 and o.out == want
            o.free()
        s = _Stream(c, spill, pulled=False)  # (and read to its end, the same stream is right)
        assert s.read_to_end() == 0 and s.out == spill_want
        s.free()
    finally:
        c.close()


def test_switching_the_option_in_the_middle_of_a_stream():
    """BRX_OPTION_READER_BATCH may change while streams are being read.  A round stages a little more than its slice (up to the pause
    position + the slack, over bytes not decoded yet); a slice of its own, read from the device, must not be served from that stale
    staging.  Two streams (bounded, pulled) read in 64 KiB pieces through brx_stream_read and, after them, two through
    brx_stream_advance, the option flipped between 1 and 0 after every slice: every byte right."""
    from brotli_rs_amd import brx
    rng = random.Random(77)
    c = brx_knobs.context(0)
    lib = brx.load_library()
    try:
        srcs = [_text(rng, 18 * MIB) for _ in range(4)]
        comps = c.generate_batch(srcs, metablock_bytes=MIB, adaptive=True)
        l0 = c.reader_slice_launches()
        for k in range(2):  # brx_stream_read: the option flips whenever the bytes of a slice have all been read
            s = _Stream(c, comps[k], pulled=k == 1, seed=k)
            batch = 1
            while s.end is None:
                if s.ready() == 0:
                    assert lib.brx_ctx_set_option(c._h, 15, batch) == 0
                    batch ^= 1
                s.read(64 << 10)
            assert s.end == 0 and s.out == srcs[k], (k, len(s.out))
            s.free()
        streams = [_Stream(c, comps[k], pulled=k == 3, seed=k) for k in (2, 3)]
        batch = 1
        while True:  # brx_stream_advance, the option flipped between the calls
            assert lib.brx_ctx_set_option(c._h, 15, batch) == 0
            batch ^= 1
            if _advance(c, streams) == 0:
                break
            for s in streams:
                s.drain_ready()
        for s, want in zip(streams, srcs[2:]):
            assert s.read_to_end() == 0 and s.out == want
            s.free()
        assert c.reader_slice_launches() - l0 >= 10
    finally:
        c.close()


def test_free_waits_for_the_round_that_holds_the_stream():
    """One thread moves four streams on with brx_stream_advance; another frees one of them as soon as the round is launched (counter 16
    moved): the free waits for the round, the advance call returns, the three others finish bit-exact, and the context's memory is as
    before."""
    from brotli_rs_amd import brx
    rng = random.Random(73)
    c = brx_knobs.context(0)
    try:
        srcs = [_text(rng, 12 * MIB) for _ in range(4)]
        comps = c.generate_batch(srcs, metablock_bytes=256 << 10, adaptive=True)
        warm = _Stream(c, comps[0], pulled=False)
        _drive(c, [warm])  # (the round's own allocations: descriptor tables, staging)
        warm.free()
        used0 = _hip_mem_used()
        streams = [_Stream(c, x, pulled=i % 2 == 1, seed=i) for i, x in enumerate(comps)]
        l0 = c.reader_slice_launches()
        victim = streams[2]
        freed = []

        def freer():
            while c.reader_slice_launches() == l0:
                pass
            victim.free()
            freed.append(1)

        t = threading.Thread(target=freer)
        t.start()
        assert _advance(c, streams) == 4
        t.join(timeout=120)
        assert freed and victim.h is None
        rest = [s for s in streams if s is not victim]
        _drive(c, rest)
        for s, want in zip(streams, srcs):
            if s is not victim:
                assert s.end == 0 and s.out == want
                s.free()
        assert _hip_mem_used() <= used0 + 16 * MIB, (used0, _hip_mem_used())
        assert brx.load_library() is not None
    finally:
        c.close()


def test_a_callback_that_overfills_fails_only_its_own_stream():
    """A pull callback that returns more than `cap` fails its stream with -1000 + BRX_ERR_INVALID_ARGUMENT; the stream next to it in the
    same advance call decodes right."""
    rng = random.Random(74)
    c = brx_knobs.context(0)
    try:
        src = _text(rng, 9 * MIB)
        comp = c.generate_batch([src], metablock_bytes=MIB, adaptive=True)[0]
        good, bad = _Stream(c, comp, pulled=True, seed=1), _Stream(c, comp, pulled=True, over_cap=True)
        _drive(c, [good, bad])
        assert bad.end == -1000 - 1 and not bad.out
        assert good.end == 0 and good.out == src
        good.free()
        bad.free()
    finally:
        c.close()


def test_whole_stream_and_bounded_readers_at_once():
    """Whole-stream facade Decompressors (batched by the facade's leader) and streaming ones (reader rounds) on one context, on
    twelve threads at the same time: every byte right."""
    import io
    from brotli_rs_amd import brx
    rng = random.Random(75)
    c = brx_knobs.context(0)
    try:
        small, small_want = _read("alice29.txt.compressed"), _read("alice29.txt")
        srcs = [_text(rng, 9 * MIB) for _ in range(4)]
        comps = c.generate_batch(srcs, metablock_bytes=MIB, adaptive=True)
        wrong = []

        def facade():
            for _ in range(6):
                d = brx.Decompressor(io.BytesIO(small), c)
                if d.read() != small_want:
                    wrong.append("facade")
                d.close()

        def streaming(k):
            d = brx.Decompressor(io.BytesIO(comps[k]), c, streaming=True)
            got = bytearray()
            while True:
                chunk = d.read(1 << 16)
                if not chunk:
                    break
                got += chunk
            if got != srcs[k]:
                wrong.append(k)
            d.close()

        ths = [threading.Thread(target=facade) for _ in range(8)] + [threading.Thread(target=streaming, args=(k,)) for k in range(4)]
        [t.start() for t in ths]
        [t.join(timeout=300) for t in ths]
        assert not wrong and not any(t.is_alive() for t in ths)
        assert c.reader_slices() >= c.reader_slice_launches() > 0
    finally:
        c.close()


def test_python_advance_over_decompressors():
    """brx.advance / Context.advance over streaming Decompressors, read between the calls with Decompressor.ready()."""
    import io
    from brotli_rs_amd import brx
    rng = random.Random(76)
    c = brx_knobs.context(0)
    try:
        srcs = [_text(rng, 7 * MIB) for _ in range(3)]
        comps = c.generate_batch(srcs, metablock_bytes=MIB, adaptive=True)
        ds = [brx.Decompressor(io.BytesIO(x), c, streaming=True) for x in comps]
        outs = [bytearray() for _ in ds]
        rounds = 0
        while brx.advance(ds):
            rounds += 1
            for d, o in zip(ds, outs):
                while d.ready():
                    o += d.read(d.ready())
        assert rounds >= 2
        for d, o, want in zip(ds, outs, srcs):
            assert d.read() == b"" and o == want
            d.close()
    finally:
        c.close()
