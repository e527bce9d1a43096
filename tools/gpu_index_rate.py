#!/usr/bin/env python3
"""Times brx_index_batch, brx_index_quoted_batch, brx_index_escaped_batch (record boundaries of a decoded batch, on the device; the
second with RFC 4180 quoting, quote = '"'; the third with an escape byte on top, escape = '\\'), brx_index_set_batch (the third with a
set of delimiters and optional quote and escape) and brx_find_batch with HIP events, in one run:

  headline  the decoded output of N x alice29 (default 4096) in device memory, delim = '\\n': count mode and fill mode of the three calls
            (pos_off from a count-mode call and torch.cumsum, outside the timed window), brx_compact_batch over the same slots (the
            yardstick for ONE pass over this ragged layout; it also writes what it reads) and brx_digest_batch (CRC-32) over the same
            slots
  large     the same six modes over one stream of 70 MiB (random bytes: one delimiter and one quote in 256)
  ragged    the same six modes over 4096 streams, lengths log-uniform over 1 B .. 4 MiB (fixed seed, random bytes)

Behind the six modes of each batch (the escaped ones with their ratio to the quoted pass of the same run) come the find lines: brx_find_batch (occurrences of a byte sequence) with needles of 1, 2, 4 and
16 bytes that occur in the data -- for alice29 its line feed, its line ending CR LF, "the " and "the Mock Turtle "; for the random
bytes a line feed, two line feeds, and 4 and 16 bytes taken from the data -- in count mode and fill mode, each with its ratio to the
brx_index_batch line of the same batch and mode.

Behind them come the set lines: brx_index_set_batch in count mode and fill mode (with `what`) for b"\\n", b",\\n" and b"{}[]:,\\n" at
flags 0, b",\\n" under BRX_INDEX_NO_ESCAPE and b"\\r\\n" under both flags, each with its ratio to the brx_index_escaped_batch line of the same
batch and mode; the one-delimiter line says whether it lies within the spread (min .. max) of the escaped pass's repetitions, and the
b",\\n" fill line carries its ratio to the two brx_index_escaped_batch fill calls (one for '\\n', one for ',') that it replaces.

Every timed call is warmed up first, timed `--reps` times in windows of `--inner` back-to-back calls between two events; the median
and the spread of the per-call times are printed.  Counts and positions are checked against numpy on the host (not in the timed
window).  Usage: python tools/gpu_index_rate.py [--n 4096] [--reps 9] [--inner 100] [--out FILE]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from brotli_rs_amd import brx  # noqa: E402
import brx_knobs  # noqa: E402
import escaped_oracle  # noqa: E402
import set_oracle  # noqa: E402

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
NL = 10
QUOTE = 0x22
ESCAPE = 0x5C


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


def quoted_reference(s):
    """-> (positions of the bytes of s equal to NL with an even number of QUOTE bytes in front of them, parity of the quotes)"""
    is_q = s == QUOTE
    inside = (np.cumsum(is_q) - is_q) & 1
    return np.flatnonzero((s == NL) & (inside == 0)), int(is_q.sum() & 1)


def index_rates(name, arena, offs, lens, stream_bytes):
    """Count mode and fill mode of brx_index_batch, brx_index_quoted_batch and brx_index_escaped_batch over one batch; stream_bytes(i) -> the bytes of
    stream i as a numpy array (results checked on a sample).  -> {mode: median ms}, {mode: (median, min, max) ms}"""
    n = lens.numel()
    total_bytes = int(lens.sum().item())
    base = (arena.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, arena.numel())
    res, shown = {}, {}
    sample = sorted(set(np.linspace(0, n - 1, 16).astype(int).tolist()))
    for kind in ("index", "quoted", "escaped"):
        count = torch.zeros(n, dtype=torch.int64, device=dev)
        open_ = torch.zeros(n, dtype=torch.int32, device=dev)

        def call(count_ptr, open_ptr, *fill):
            if kind == "index":
                ctx.index_batch_device(NL, *base, count_ptr, *fill, hip_stream=stream.cuda_stream)
            elif kind == "quoted":
                ctx.index_quoted_batch_device(NL, QUOTE, *base, count_ptr, open_ptr, *fill, hip_stream=stream.cuda_stream)
            else:
                ctx.index_escaped_batch_device(NL, QUOTE, ESCAPE, 0, *base, count_ptr, open_ptr, *fill, hip_stream=stream.cuda_stream)

        def count_call():
            call(count.data_ptr(), open_.data_ptr())
        count_call()
        stream.synchronize()
        res[kind + " count"] = timed(count_call)
        pos_off = torch.cumsum(count, 0) - count
        entries = int(count.sum().item())
        pos = torch.zeros(max(entries, 1), dtype=torch.int64, device=dev)

        def fill_call():
            call(None, None, pos_off.data_ptr(), pos.data_ptr(), entries)
        res[kind + " fill"] = timed(fill_call)
        h_count, h_open, h_off, h_pos = count.cpu().numpy(), open_.cpu().numpy(), pos_off.cpu().numpy(), pos.cpu().numpy()
        for i in sample:
            s = stream_bytes(i)
            want, want_open = ((np.flatnonzero(s == NL), 0) if kind == "index" else quoted_reference(s) if kind == "quoted" else
                               escaped_oracle.vec(s, NL, QUOTE, ESCAPE))
            assert h_count[i] == want.size, "%s %s: count of stream %d differs from numpy" % (name, kind, i)
            assert h_open[i] == want_open, "%s %s: open of stream %d differs from numpy" % (name, kind, i)
            assert (h_pos[h_off[i]:h_off[i] + h_count[i]] == want).all(), "%s %s: positions of stream %d differ from numpy" % (name, kind, i)
        shown[kind] = entries
    for mode, (med, lo, hi) in res.items():
        say("%-9s %-12s  %9.3f ms  (min %.3f, max %.3f)  %7.1f GB/s   [%d streams, %.1f MB, %d entries]"
            % (name, mode, med, lo, hi, total_bytes / med / 1e6, n, total_bytes / 1e6, shown[mode.split()[0]]))
    for mode in ("count", "fill"):
        say("%-9s quoted %-5s = %.3f x index %s" % (name, mode, res["quoted " + mode][0] / res["index " + mode][0], mode))
    for mode in ("count", "fill"):
        say("%-9s escaped %-5s = %.3f x quoted %s, %.3f x index %s" % (name, mode, res["escaped " + mode][0] / res["quoted " + mode][0], mode,
                                                                      res["escaped " + mode][0] / res["index " + mode][0], mode))
    return {m: v[0] for m, v in res.items()}, res


SET_CASES = ((b"\n", 0), (b",\n", 0), (b"{}[]:,\n", 0), (b",\n", brx.INDEX_NO_ESCAPE), (b"\r\n", brx.INDEX_NO_QUOTE | brx.INDEX_NO_ESCAPE))


def set_rates(name, arena, offs, lens, stream_bytes, escaped):
    """Count mode and fill mode (with `what`) of brx_index_set_batch over one batch for every case of SET_CASES (results checked on a
    sample); escaped = the (median, min, max) of index_rates for the same batch: the yardstick of every line.  The two escaped fill
    calls that the b",\\n" case replaces: the '\\n' one of index_rates and a ',' one timed here."""
    n = lens.numel()
    total_bytes = int(lens.sum().item())
    base = (arena.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, arena.numel())
    sample = sorted(set(np.linspace(0, n - 1, 16).astype(int).tolist()))
    count = torch.zeros(n, dtype=torch.int64, device=dev)
    open_ = torch.zeros(n, dtype=torch.int32, device=dev)
    ctx.index_escaped_batch_device(0x2C, QUOTE, ESCAPE, 0, *base, count.data_ptr(), open_.data_ptr(), hip_stream=stream.cuda_stream)
    stream.synchronize()
    comma_off = torch.cumsum(count, 0) - count
    comma_entries = int(count.sum().item())
    comma_pos = torch.zeros(max(comma_entries, 1), dtype=torch.int64, device=dev)
    comma_ms, lo, hi = timed(lambda: ctx.index_escaped_batch_device(0x2C, QUOTE, ESCAPE, 0, *base, None, None, comma_off.data_ptr(),
                                                                    comma_pos.data_ptr(), comma_entries, hip_stream=stream.cuda_stream))
    say("%-9s escaped fill ','  %9.3f ms  (min %.3f, max %.3f)   [%d entries]" % (name, comma_ms, lo, hi, comma_entries))
    for delims, flags in SET_CASES:
        tag = "set %s%s" % ("".join("%02x" % b for b in delims), {0: "", 1: " nq", 2: " ne", 3: " nq ne"}[flags])

        def call(count_ptr, open_ptr, *fill):
            ctx.index_set_batch_device(delims, QUOTE, ESCAPE, flags, *base, count_ptr, open_ptr, *fill, hip_stream=stream.cuda_stream)

        def count_call():
            call(count.data_ptr(), open_.data_ptr())
        count_call()
        stream.synchronize()
        res = {"count": timed(count_call)}
        pos_off = torch.cumsum(count, 0) - count
        entries = int(count.sum().item())
        pos = torch.zeros(max(entries, 1), dtype=torch.int64, device=dev)
        what = torch.zeros(max(entries, 1), dtype=torch.uint8, device=dev)

        def fill_call():
            call(None, None, pos_off.data_ptr(), pos.data_ptr(), what.data_ptr(), entries)
        res["fill"] = timed(fill_call)
        h_count, h_open, h_off, h_pos, h_what = count.cpu().numpy(), open_.cpu().numpy(), pos_off.cpu().numpy(), pos.cpu().numpy(), what.cpu().numpy()
        for i in sample:
            want, want_what, want_open = set_oracle.vec(stream_bytes(i), delims, QUOTE, ESCAPE, bool(flags & brx.INDEX_NO_QUOTE),
                                                        bool(flags & brx.INDEX_NO_ESCAPE))
            assert h_count[i] == want.size, "%s %s: count of stream %d differs from numpy" % (name, tag, i)
            assert h_open[i] == want_open, "%s %s: open of stream %d differs from numpy" % (name, tag, i)
            assert (h_pos[h_off[i]:h_off[i] + h_count[i]] == want).all(), "%s %s: positions of stream %d differ from numpy" % (name, tag, i)
            assert (h_what[h_off[i]:h_off[i] + h_count[i]] == want_what).all(), "%s %s: what of stream %d differs from numpy" % (name, tag, i)
        for mode, (med, lo, hi) in res.items():
            e_med, e_lo, e_hi = escaped["escaped " + mode]
            more = ""
            if delims == b"\n" and flags == 0:
                more = "  (escaped %.3f .. %.3f: %s its spread)" % (e_lo, e_hi, "within" if e_lo <= med <= e_hi else "OUTSIDE")
            if delims == b",\n" and flags == 0 and mode == "fill":
                more = "  = %.3f x two escaped fills (%.3f ms)" % (med / (e_med + comma_ms), e_med + comma_ms)
            say("%-9s %-24s %-5s  %9.3f ms  (min %.3f, max %.3f)  %7.1f GB/s  = %.3f x escaped %-5s  [%d entries]%s"
                % (name, tag, mode, med, lo, hi, total_bytes / med / 1e6, med / e_med, mode, entries, more))


def find_reference(s, needle):
    """-> offsets of the occurrences of needle in s, overlapping ones included"""
    m = len(needle)
    if s.size < m:
        return np.zeros(0, dtype=np.int64)
    ok = np.ones(s.size - m + 1, dtype=bool)
    for k in range(m):
        ok &= s[k:s.size - m + 1 + k] == needle[k]
    return np.flatnonzero(ok)


def find_rates(name, arena, offs, lens, stream_bytes, needles, index_ms):
    """Count mode and fill mode of brx_find_batch over one batch for every needle (results checked on a sample); index_ms = what
    index_rates returned for the same batch: the yardstick of every line."""
    n = lens.numel()
    total_bytes = int(lens.sum().item())
    base = (arena.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, arena.numel())
    sample = sorted(set(np.linspace(0, n - 1, 16).astype(int).tolist()))
    for needle in needles:
        count = torch.zeros(n, dtype=torch.int64, device=dev)

        def count_call():
            ctx.find_batch_device(needle, *base, count.data_ptr(), hip_stream=stream.cuda_stream)
        count_call()
        stream.synchronize()
        res = {"count": timed(count_call)}
        pos_off = torch.cumsum(count, 0) - count
        entries = int(count.sum().item())
        assert entries > 0, "%s: the needle %r does not occur" % (name, needle)
        pos = torch.zeros(entries, dtype=torch.int64, device=dev)

        def fill_call():
            ctx.find_batch_device(needle, *base, None, pos_off.data_ptr(), pos.data_ptr(), entries, hip_stream=stream.cuda_stream)
        res["fill"] = timed(fill_call)
        h_count, h_off, h_pos = count.cpu().numpy(), pos_off.cpu().numpy(), pos.cpu().numpy()
        for i in sample:
            want = find_reference(stream_bytes(i), needle)
            assert h_count[i] == want.size, "%s find %r: count of stream %d differs from numpy" % (name, needle, i)
            assert (h_pos[h_off[i]:h_off[i] + h_count[i]] == want).all(), "%s find %r: positions of stream %d differ from numpy" % (name, needle, i)
        for mode, (med, lo, hi) in res.items():
            say("%-9s find m=%-2d %-5s  %9.3f ms  (min %.3f, max %.3f)  %7.1f GB/s  = %.3f x index %-5s  [%d entries, needle %s]"
                % (name, len(needle), mode, med, lo, hi, total_bytes / med / 1e6, med / index_ms["index " + mode], mode, entries,
                   needle.hex()))


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
ctx.decode_batch_device(blob.data_ptr(), in_off.data_ptr(), n, out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), status.data_ptr())
ctx.synchronize()
assert not status.any().item() and (out_len == len(text)).all().item()
say("headline  %d x alice29 decoded on the device: %.1f MB in slots of %d bytes" % (n, n * len(text) / 1e6, cap))

dst = torch.zeros(n * len(text), dtype=torch.uint8, device=dev)
dst_off = torch.arange(n, dtype=torch.int64, device=dev) * len(text)


def compact():
    ctx.compact_batch_device(out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), n, dst.data_ptr(), dst_off.data_ptr(),
                             n * len(text), hip_stream=stream.cuda_stream)


compact_ms, lo, hi = timed(compact)
say("headline  compact       %9.3f ms  (min %.3f, max %.3f)  %7.1f GB/s read + as much written" % (compact_ms, lo, hi, n * len(text) / compact_ms / 1e6))
digest = torch.zeros(n, dtype=torch.int32, device=dev)


def digest_call():
    ctx.digest_batch_device(brx.DIGEST_KINDS["crc32"], out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), n, digest.data_ptr(),
                            hip_stream=stream.cuda_stream)


digest_ms, lo, hi = timed(digest_call)
say("headline  digest crc32  %9.3f ms  (min %.3f, max %.3f)  %7.1f GB/s" % (digest_ms, lo, hi, n * len(text) / digest_ms / 1e6))
np_text = np.frombuffer(text, dtype=np.uint8)
res, spreads = index_rates("headline", out, out_off, out_len, lambda i: np_text)
for mode, ms in res.items():
    say("headline  %-12s = %.3f x compact, %.3f x digest" % (mode, ms / compact_ms, ms / digest_ms))
find_rates("headline", out, out_off, out_len, lambda i: np_text, (b"\n", b"\r\n", b"the ", b"the Mock Turtle "), res)
set_rates("headline", out, out_off, out_len, lambda i: np_text, spreads)
del blob, dst

# ---- one large stream ------------------------------------------------------------------------------------------------
g = torch.Generator(device=dev)
g.manual_seed(7)
big_n = (70 << 20) + 12345
arena = torch.randint(0, 256, (big_n + 64,), dtype=torch.uint8, device=dev, generator=g)
host = arena.cpu().numpy()
big_off, big_len = torch.tensor([3], dtype=torch.int64, device=dev), torch.tensor([big_n], dtype=torch.int64, device=dev)
res, spreads = index_rates("large", arena, big_off, big_len, lambda i: host[3:3 + big_n])
find_rates("large", arena, big_off, big_len, lambda i: host[3:3 + big_n],
           (b"\n", b"\n\n", host[100000:100004].tobytes(), host[200000:200016].tobytes()), res)
set_rates("large", arena, big_off, big_len, lambda i: host[3:3 + big_n], spreads)

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
d_offs, d_lens = torch.from_numpy(h_offs).to(dev), torch.from_numpy(h_lens).to(dev)
big = int(np.argmax(h_lens))  # (the 4- and 16-byte needles are bytes of the longest stream)
res, spreads = index_rates("ragged", arena, d_offs, d_lens, lambda i: host[h_offs[i]:h_offs[i] + h_lens[i]])
find_rates("ragged", arena, d_offs, d_lens, lambda i: host[h_offs[i]:h_offs[i] + h_lens[i]],
           (b"\n", b"\n\n", host[h_offs[big] + 1000:h_offs[big] + 1004].tobytes(), host[h_offs[big] + 2000:h_offs[big] + 2016].tobytes()),
           res)
set_rates("ragged", arena, d_offs, d_lens, lambda i: host[h_offs[i]:h_offs[i] + h_lens[i]], spreads)
ctx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
