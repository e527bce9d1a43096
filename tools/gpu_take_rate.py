#!/usr/bin/env python3
"""Times brx_take_batch (the selected records of a decoded batch gathered on the device) with HIP events, in one run, over two
batches indexed at '\\n' by brx_index_batch:

  headline  the decoded output of N x alice29 (default 4096) in device memory
  ragged    4096 streams, lengths log-uniform over 1 B .. 4 MiB (fixed seed, random bytes: one line feed in 256)

Cases, fill mode, rec_len not written (dst_off comes from a size-mode call and torch.cumsum, outside the timed window):
  (a) all records, packed, delimiters kept            (c) a random permutation of all records (pairs mode), packed
  (b) all records, packed, NO_DELIM | TRIM_CR         (d) all records in rooms of 128 bytes
and the size-mode call of (a).  The yardstick, timed in the same run, is brx_compact_batch over the same batch: the HBM-rate copy of
the same bytes that works on whole streams.  For (c) there is a second one: the same ragged-copy kernel, through brx_compact_batch,
with ONE ITEM PER RECORD (out_off = the records' source offsets in the permuted order, len = their lengths).

Before timing, rec_len of every case is held to tests/take_oracle.py in full and the destination's bytes on a sample of entries.
Every timed call is warmed up first, timed `--reps` times in windows of `--inner` back-to-back calls between two events (a call that
takes more than 20 ms gets windows of --inner / 10); the median and the spread of the per-call times are printed, with the ratio to the
yardstick, the bytes read and written (payload, and the tables' share per entry) and the share of the 8 TB/s HBM peak that the payload
traffic alone amounts to.  Usage: python tools/gpu_take_rate.py [--n 4096] [--reps 9] [--inner 100] [--out FILE]"""
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
import take_oracle  # noqa: E402

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
HBM_PEAK = 8.0e12  # bytes / s (spec)
ROOM = 128


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    """fn() enqueues one call on `stream`.  -> (median, min, max) milliseconds per call, calls per window."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    stream.synchronize()
    a.record(stream)
    for _ in range(2):
        fn()
    b.record(stream)
    b.synchronize()
    inner = args.inner if a.elapsed_time(b) / 2 <= 20.0 else max(args.inner // 10, 1)
    per = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(inner):
            fn()
        b.record(stream)
        b.synchronize()
        per.append(a.elapsed_time(b) / inner)
    per.sort()
    return per[len(per) // 2], per[0], per[-1], inner


def take_rates(name, arena, offs, lens, host):
    n = lens.numel()
    h_offs, h_lens = offs.cpu().numpy()[:n], lens.cpu().numpy()
    stream_bytes = int(h_lens.sum())
    head = (arena.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, arena.numel())
    hs = stream.cuda_stream
    # positions, by the device
    count = torch.zeros(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.index_batch_device(NL, *head, count.data_ptr())
    pos_off = torch.cumsum(count, 0) - count
    n_pos = int(count.sum().item())
    pos = torch.zeros(max(n_pos, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.index_batch_device(NL, *head, None, pos_off.data_ptr(), pos.data_ptr(), n_pos)
    m = n_pos + n
    h_count, h_pos_off, h_pos = count.cpu().numpy(), pos_off.cpu().numpy(), pos.cpu().numpy()[:n_pos]
    say("%-9s %d streams, %.1f MB, %d records (%.1f bytes each on average)" % (name, n, stream_bytes / 1e6, m, stream_bytes / m))
    tabs = (count.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), n_pos)

    # the yardstick: whole streams, back to back
    c_dst = torch.zeros(max(stream_bytes, 1), dtype=torch.uint8, device=dev)
    c_off = torch.cumsum(lens, 0) - lens
    torch.cuda.synchronize()

    def compact():
        ctx.compact_batch_device(*head[:4], c_dst.data_ptr(), c_off.data_ptr(), stream_bytes, hip_stream=hs)
    compact_ms, lo, hi, _ = timed(compact)
    say("%-9s compact (whole streams)      %9.3f ms  (min %.3f, max %.3f)  %7.1f GB/s read + as much written = %.1f %% of HBM peak"
        % (name, compact_ms, lo, hi, stream_bytes / compact_ms / 1e6, 100 * 2 * stream_bytes / (compact_ms * 1e-3) / HBM_PEAK))
    del c_dst

    oracle = {}
    for flags in (0, brx.TAKE_NO_DELIM | brx.TAKE_TRIM_CR):
        oracle[flags] = take_oracle.take_vec(host, h_offs, h_lens, h_count, h_pos_off, h_pos, n_pos, 1, flags)
    rng = np.random.default_rng(2024)
    perm = rng.permutation(m)
    all_i, all_k = take_oracle.entries_all_vec(h_count, h_pos_off, m)
    sel_stream = torch.from_numpy(all_i[perm].astype(np.int32)).to(dev)
    sel_rec = torch.from_numpy(all_k[perm].astype(np.int64)).to(dev)
    sample = np.sort(rng.choice(m, min(m, 20000), replace=False))
    rec_len = torch.zeros(m, dtype=torch.int64, device=dev)

    cases = (("(a) all, packed, delimiters kept", 0, False, None), ("(b) all, packed, NO_DELIM|TRIM_CR", brx.TAKE_NO_DELIM | brx.TAKE_TRIM_CR, False, None),
             ("(c) permuted, packed", 0, True, None), ("(d) all, rooms of %d bytes" % ROOM, 0, False, ROOM))
    for label, flags, permuted, stride in cases:
        src, L = oracle[flags]
        if permuted:
            src, L = src[perm], L[perm]
        sel = (sel_stream.data_ptr(), sel_rec.data_ptr()) if permuted else (None, None)
        call = head + tabs + (1, flags) + sel + (m,)
        torch.cuda.synchronize()
        ctx.take_batch_device(*call, rec_len.data_ptr())
        assert np.array_equal(rec_len.cpu().numpy(), L), "%s %s: rec_len differs from take_oracle" % (name, label)
        if stride is None:
            dst_off = torch.cumsum(rec_len, 0) - rec_len
            total = int(L.sum())
            dst = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        else:
            dst_off = torch.arange(m, dtype=torch.int64, device=dev) * stride
            total = m * stride
            dst = torch.zeros(total, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.take_batch_device(*call, None, dst_off.data_ptr(), dst.data_ptr(), total)
        h_dst, h_dst_off = dst.cpu().numpy(), dst_off.cpu().numpy()
        cnt = np.minimum(L, stride) if stride is not None else L
        for j in sample:
            assert np.array_equal(h_dst[h_dst_off[j]:h_dst_off[j] + cnt[j]], host[src[j]:src[j] + cnt[j]]), \
                "%s %s: bytes of entry %d differ from take_oracle" % (name, label, j)
        if label.startswith("(a)"):
            assert total == stream_bytes  # ... and (a) is the compacted batch

            def size_call():
                ctx.take_batch_device(*call, rec_len.data_ptr(), hip_stream=hs)
            med, lo, hi, _ = timed(size_call)
            say("%-9s size mode of (a)             %9.3f ms  (min %.3f, max %.3f)  %7.1f M entries/s" % (name, med, lo, hi, m / med / 1e3))
        del h_dst

        def fill_call():
            ctx.take_batch_device(*call, None, dst_off.data_ptr(), dst.data_ptr(), total, hip_stream=hs)
        med, lo, hi, inner = timed(fill_call)
        payload = int(cnt.sum())
        tab = 16 + (12 if permuted else 0)  # per entry: dst_off and pos once each (neighbours come from cache), the pair in pairs mode
        say("%-9s %-34s %9.3f ms  (min %.3f, max %.3f)  = %.3f x compact   reads %.1f MB + %d B/entry of tables (%.1f MB), writes %.1f MB, "
            "%.1f GB/s of payload each way = %.1f %% of HBM peak  [%d calls per window]"
            % (name, label, med, lo, hi, med / compact_ms, payload / 1e6, tab, tab * m / 1e6, payload / 1e6, payload / med / 1e6,
               100 * 2 * payload / (med * 1e-3) / HBM_PEAK, inner))
        if permuted:  # the second yardstick: the ragged-copy kernel with one item per record
            if m < 1 << 32:
                r_off, r_len = torch.from_numpy(src).to(dev), torch.from_numpy(L).to(dev)
                torch.cuda.synchronize()

                def per_record():
                    ctx.compact_batch_device(arena.data_ptr(), r_off.data_ptr(), r_len.data_ptr(), m, dst.data_ptr(), dst_off.data_ptr(), total,
                                             hip_stream=hs)
                rmed, lo, hi, inner = timed(per_record)
                stream.synchronize()
                h2 = dst.cpu().numpy()
                for j in sample[:2000]:
                    assert np.array_equal(h2[h_dst_off[j]:h_dst_off[j] + L[j]], host[src[j]:src[j] + L[j]])
                say("%-9s ragged copy, one item per record %6.3f ms  (min %.3f, max %.3f)  = %.3f x compact;  (c) = %.3f x this  [%d calls per window]"
                    % (name, rmed, lo, hi, rmed / compact_ms, med / rmed, inner))
                del r_off, r_len
        del dst, dst_off


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
del blob
take_rates("headline", out, out_off, out_len, out.cpu().numpy())
del out

# ---- 4096 log-uniform lengths (the batch of tools/gpu_index_rate.py) ---------------------------------------------------------
rng = np.random.default_rng(1234)
top = 4 << 20
h_lens = np.clip(np.floor(np.exp(rng.uniform(0.0, np.log(top), 4096))).astype(np.int64), 1, top)
slots = h_lens + rng.integers(0, 64, 4096)
h_offs = np.zeros(4096, dtype=np.int64)
np.cumsum(slots[:-1], out=h_offs[1:])
g = torch.Generator(device=dev)
g.manual_seed(99)
arena = torch.randint(0, 256, (int(h_offs[-1] + slots[-1]),), dtype=torch.uint8, device=dev, generator=g)
take_rates("ragged", arena, torch.from_numpy(h_offs).to(dev), torch.from_numpy(h_lens).to(dev), arena.cpu().numpy())
ctx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
