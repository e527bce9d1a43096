"""Reader rounds, measured (profiles/r07_reader_batch.txt): pulled readers over 16 MiB each of generator text on one context.

    python3 tools/gpu_reader_rounds.py alone   [n]    n readers (default 8) read one after the other, BRX_OPTION_READER_BATCH = 0
    python3 tools/gpu_reader_rounds.py advance [n]    n readers (default 64) moved on together with brx_stream_advance from one thread
    python3 tools/gpu_reader_rounds.py threads [n]    n threads (default 64), each reads its own pulled Decompressor (tests/cpp/reader_threads.cpp)

Prints the aggregate MB/s of decoded output and the slices per launch (brx_last_timing 16 / 17); `advance` also the wall time of
every advance call (the round: host prepare + launch + wait + settle) and how much of it the host spends outside the wait.  Run
`advance` under  rocprofv3 --kernel-trace --stats -- python3 ...  for the kernel's own time per round."""
import ctypes
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from brotli_rs_amd import brx  # noqa: E402

MIB = 1 << 20
TEXTS = ["lcet10.txt", "plrabn12.txt", "alice29.txt", "asyoulik.txt"]
DATA = os.path.join(ROOT, "tests", "golden", "data")


def sources(n, size=16 * MIB):
    corpus = b"".join(open(os.path.join(DATA, t), "rb").read() for t in TEXTS)
    rng = random.Random(5)
    out = []
    for _ in range(n):
        start = rng.randrange(len(corpus))
        s = bytearray((corpus * ((start + size) // len(corpus) + 1))[start:start + size])
        for i in range(0, size, 4096):
            s[i] = rng.randrange(256)
        out.append(bytes(s))
    return out


class Pulled:
    def __init__(self, ctx, comp):
        self.comp, self.at = comp, 0
        lib = brx.load_library()

        def pull(_user, buf, cap):
            k = min(cap, len(self.comp) - self.at)
            ctypes.memmove(buf, self.comp[self.at:self.at + k], k)
            self.at += k
            return k
        self.cb = brx.READ_FN(pull)
        self.h = lib.brx_stream_new_reader(ctx._h, self.cb, None)


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "advance"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else (8 if mode == "alone" else 64)
    if mode == "threads":
        exe = os.path.join("/tmp", "reader_threads_%d" % os.getpid())
        lib = os.path.join(ROOT, "brotli-rs_amd")
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "reader_threads.cpp"), "-o", exe, "-L", lib,
                               "-lbrx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"])
        try:
            subprocess.check_call([exe, "threads", "1", str(n), "16", "16"] + [os.path.join(DATA, t) for t in TEXTS])
        finally:
            os.unlink(exe)
        return
    ctx = brx.Context(0, options={"reader_batch": 0 if mode == "alone" else 1})
    srcs = sources(n)
    comps = ctx.generate_batch(srcs, metablock_bytes=MIB, adaptive=True)
    lib = brx.load_library()
    buf = ctypes.create_string_buffer(4 * MIB)
    total = sum(len(s) for s in srcs)
    l0, s0 = ctx.reader_slice_launches(), ctx.reader_slices()
    wrong = 0
    t0 = time.perf_counter()
    if mode == "alone":
        for comp, want in zip(comps, srcs):
            r = Pulled(ctx, comp)
            got = bytearray()
            while True:
                k = lib.brx_stream_read(r.h, buf, len(buf))
                if k <= 0:
                    wrong += k != 0
                    break
                got += ctypes.string_at(buf, k)
            wrong += got != want
            lib.brx_stream_free(r.h)
        rounds = []
    else:
        rs = [Pulled(ctx, c) for c in comps]
        outs = [bytearray() for _ in rs]
        arr = (ctypes.c_void_p * n)(*[r.h for r in rs])
        rounds = []
        while True:
            a = time.perf_counter()
            k = lib.brx_stream_advance(arr, n)
            b = time.perf_counter()
            if k <= 0:
                break
            for r, o in zip(rs, outs):
                while lib.brx_stream_ready(r.h) > 0:
                    m = lib.brx_stream_read(r.h, buf, len(buf))
                    o += ctypes.string_at(buf, m)
            rounds.append((k, (b - a) * 1e3, (time.perf_counter() - b) * 1e3))
        for r, o, want in zip(rs, outs, srcs):
            wrong += lib.brx_stream_read(r.h, buf, len(buf)) != 0 or o != want
            lib.brx_stream_free(r.h)
    ms = (time.perf_counter() - t0) * 1e3
    launches, slices = ctx.reader_slice_launches() - l0, ctx.reader_slices() - s0
    print("%s: %d readers x 16 MiB, %.1f MiB in %.1f ms = %.0f MB/s; launches %d slices %d (%.2f per launch); %d wrong"
          % (mode, n, total / MIB, ms, total / ms / 1e3, launches, slices, slices / max(launches, 1), wrong))
    for i, (k, adv, rd) in enumerate(rounds):
        print("  round %2d: %3d slices, advance %.1f ms, reading the staged bytes %.1f ms" % (i, k, adv, rd))
    ctx.close()
    return 1 if wrong else 0


if __name__ == "__main__":
    sys.exit(main())
