#!/usr/bin/env python3
"""Times brx_digest_batch (CRC-32 / CRC-32C of a decoded batch, on the device) with HIP events:

  headline  the decoded output of N x alice29 (default 4096) in device memory: the digest pass of both kinds, brx_compact_batch over
            the same bytes (the yardstick for ONE pass over this ragged layout; it also writes what it reads) and the decode kernels
            that produced them (brx_last_timing 1), all in this run
  large     one stream of 70 MiB
  ragged    4096 streams, lengths log-uniform over 1 B .. 4 MiB (fixed seed)

Every timed call is warmed up first, timed `--reps` times in windows of `--inner` back-to-back calls between two events; the median
and the spread of the per-call times are printed.  Digests are checked against zlib on the host (not in the timed window).
Usage: python tools/gpu_digest_rate.py [--n 4096] [--reps 9] [--inner 100] [--out FILE]"""
import argparse
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from brotli_rs_amd import brx  # noqa: E402
import brx_knobs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=100)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = brx_knobs.context(0)
stream = torch.cuda.Stream(device=dev)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    """fn() enqueues one call on `stream`.  -> (median, min, max) milliseconds per call."""
    for _ in range(3):
        fn()
    stream.synchronize()
    per = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.inner):
            fn()
        b.record(stream)
        b.synchronize()
        per.append(a.elapsed_time(b) / args.inner)
    per.sort()
    return per[len(per) // 2], per[0], per[-1]


def digest_rates(name, arena, offs, lens, check):
    """Both kinds over one batch.  -> {kind: median ms}"""
    total = int(lens.sum().item())
    res = {}
    for kind in ("crc32", "crc32c"):
        digest = torch.zeros(lens.numel(), dtype=torch.int32, device=dev)

        def call():
            ctx.digest_batch_device(brx.DIGEST_KINDS[kind], arena.data_ptr(), offs.data_ptr(), lens.data_ptr(), lens.numel(),
                                    digest.data_ptr(), hip_stream=stream.cuda_stream)
        med, lo, hi = timed(call)
        res[kind] = med
        if kind == "crc32":
            check(digest.cpu().numpy().view(np.uint32))
        say("%-9s digest %-6s %9.3f ms  (min %.3f, max %.3f)  %7.1f GB/s   [%d streams, %.1f MB]"
            % (name, kind, med, lo, hi, total / med / 1e6, lens.numel(), total / 1e6))
    return res


# ---- headline: N x alice29, decoded on the device -------------------------------------------------------------------------
n = args.n
comp = open(os.path.join(ROOT, "tests", "golden", "data", "alice29.txt.compressed"), "rb").read()
text = open(os.path.join(ROOT, "tests", "golden", "data", "alice29.txt"), "rb").read()
cap = (len(text) + 15) & ~15
blob = torch.frombuffer(bytearray(comp), dtype=torch.uint8).to(dev).repeat(n).contiguous()
in_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * len(comp)
out_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * cap
out = torch.zeros(n * cap, dtype=torch.uint8, device=dev)
out_len = torch.zeros(n, dtype=torch.int64, device=dev)
status = torch.full((n,), -1, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
kernel_ms = []
for k in range(3 + args.reps):
    ctx.decode_batch_device(blob.data_ptr(), in_off.data_ptr(), n, out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(),
                            status.data_ptr(), timing=True)
    if k >= 3:
        kernel_ms.append(ctx.last_timing_ms(1))
ctx.synchronize()
assert not status.any().item() and (out_len == len(text)).all().item()
kernel_ms.sort()
decode_ms = kernel_ms[len(kernel_ms) // 2]
say("headline  decode kernels   %9.3f ms  (min %.3f, max %.3f)  %7.1f GB/s   [%d x alice29, %.1f MB decoded]"
    % (decode_ms, kernel_ms[0], kernel_ms[-1], n * len(text) / decode_ms / 1e6, n, n * len(text) / 1e6))

dst = torch.zeros(n * len(text), dtype=torch.uint8, device=dev)
dst_off = torch.arange(n, dtype=torch.int64, device=dev) * len(text)


def compact():
    ctx.compact_batch_device(out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), n, dst.data_ptr(), dst_off.data_ptr(),
                             n * len(text), hip_stream=stream.cuda_stream)


compact_ms, lo, hi = timed(compact)
say("headline  compact          %9.3f ms  (min %.3f, max %.3f)  %7.1f GB/s read + as much written" % (compact_ms, lo, hi, n * len(text) / compact_ms / 1e6))
want = zlib.crc32(text) & 0xFFFFFFFF


def check_headline(d):
    assert (d == want).all(), "headline digests differ from zlib"


res = digest_rates("headline", out, out_off, out_len, check_headline)
for kind, ms in res.items():
    say("headline  digest %-6s = %.3f x compact, %.4f x decode kernels (must stay under 0.1)" % (kind, ms / compact_ms, ms / decode_ms))
del blob, dst

# ---- one large stream ------------------------------------------------------------------------------------------------
g = torch.Generator(device=dev)
g.manual_seed(7)
big_n = (70 << 20) + 12345
arena = torch.randint(0, 256, (big_n + 64,), dtype=torch.uint8, device=dev, generator=g)
host = arena.cpu().numpy()
offs = torch.tensor([3], dtype=torch.int64, device=dev)
lens = torch.tensor([big_n], dtype=torch.int64, device=dev)


def check_big(d):
    assert int(d[0]) == zlib.crc32(host[3:3 + big_n]) & 0xFFFFFFFF, "large-stream digest differs from zlib"


digest_rates("large", arena, offs, lens, check_big)

# ---- 4096 log-uniform lengths -------------------------------------------------------------------------------------------
rng = np.random.default_rng(1234)
top = 4 << 20
h_lens = np.clip(np.floor(np.exp(rng.uniform(0.0, np.log(top), 4096))).astype(np.int64), 1, top)
slots = h_lens + rng.integers(0, 64, 4096)
h_offs = np.zeros(4096, dtype=np.int64)
np.cumsum(slots[:-1], out=h_offs[1:])
g.manual_seed(99)
arena = torch.randint(0, 256, (int(h_offs[-1] + slots[-1]),), dtype=torch.uint8, device=dev, generator=g)
host = arena.cpu().numpy()


def check_ragged(d):
    w = np.array([zlib.crc32(host[o:o + ln]) & 0xFFFFFFFF for o, ln in zip(h_offs, h_lens)], dtype=np.uint32)
    assert (d == w).all(), "ragged digests differ from zlib"


digest_rates("ragged", arena, torch.from_numpy(h_offs).to(dev), torch.from_numpy(h_lens).to(dev), check_ragged)
ctx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
