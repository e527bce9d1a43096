#!/usr/bin/env python3
"""Times brx_hash_batch (a 64-bit key of every selected record of a decoded batch, on the device) with HIP events, in one run, over
the two batches of tools/gpu_take_rate.py, indexed at '\\n' by brx_index_batch:

  headline  the decoded output of N x alice29 (default 4096) in device memory
  ragged    4096 streams, lengths log-uniform over 1 B .. 4 MiB (fixed seed, random bytes: one line feed in 256)

and over the same two with count = 0 (`whole`): entry i is the whole of stream i, every record on the wave path.

Cases: all records with rec_len not written / written, a random permutation of all records (pairs mode), whole streams.
Yardsticks, timed in the same run: brx_take_batch in size mode (the same tables, no bytes), brx_take_batch in fill mode, all records
packed with delimiters kept -- case (a) of tools/gpu_take_rate.py, the cost floor of the only other route to a key per record (gather
the bytes, then hash them with a kernel of one's own) -- and for whole streams brx_digest_batch (CRC-32 of every stream).

Before timing, the hashes of a sample of entries of every case are held to tests/hash_oracle.py.  Every timed call is warmed up first,
timed `--reps` times in windows of `--inner` back-to-back calls between two events (a call that takes more than 20 ms gets windows of
--inner / 10); the median and the spread of the per-call times are printed.
Usage: python tools/gpu_hash_rate.py [--n 4096] [--reps 9] [--inner 100] [--out FILE]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from brotli_rs_amd import brx  # noqa: E402,F401
import brx_knobs  # noqa: E402
import hash_oracle  # noqa: E402
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
SEED = 0x5EED


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


def checked(label, name, host, tables, call, m, si, sk, sample):
    """one call, synchronous; the sample's hashes and lengths against the oracle -> (hash tensor, rec_len tensor)"""
    h = torch.zeros(m, dtype=torch.int64, device=dev)
    rec_len = torch.zeros(m, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.hash_batch_device(*call, SEED, h.data_ptr(), rec_len.data_ptr())
    src, L = take_oracle.records_vec(host, *tables, 1, 0, si[sample], sk[sample])
    want = hash_oracle.hash_records(host, src, L, SEED)
    assert np.array_equal(rec_len.cpu().numpy()[sample], L), "%s %s: rec_len differs from take_oracle" % (name, label)
    assert np.array_equal(h.cpu().numpy()[sample], want), "%s %s: hashes differ from hash_oracle" % (name, label)
    return h, rec_len


def hash_rates(name, arena, offs, lens, host):
    n = lens.numel()
    h_offs, h_lens = offs.cpu().numpy()[:n], lens.cpu().numpy()
    stream_bytes = int(h_lens.sum())
    head = (arena.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, arena.numel())
    hs = stream.cuda_stream
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
    tables = (h_offs, h_lens, h_count, h_pos_off, h_pos, n_pos)
    rng = np.random.default_rng(2025)
    all_i, all_k = take_oracle.entries_all_vec(h_count, h_pos_off, m)
    sample = np.sort(rng.choice(m, min(m, 3000), replace=False))
    call = head + tabs + (1, 0, None, None, m)

    # yardsticks: take's size mode, and take's fill mode (a)
    h, rec_len = checked("all records", name, host, tables, call, m, all_i, all_k, sample)
    long_share = float((rec_len >= 1024).sum().item()) / m
    dst_off = torch.cumsum(rec_len, 0) - rec_len
    dst = torch.empty(max(stream_bytes, 1), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def size_call():
        ctx.take_batch_device(*call, rec_len.data_ptr(), hip_stream=hs)
    size_ms, lo, hi, _ = timed(size_call)
    say("%-9s take, size mode                    %9.3f ms  (min %.3f, max %.3f)  %7.1f M entries/s" % (name, size_ms, lo, hi, m / size_ms / 1e3))

    def fill_call():
        ctx.take_batch_device(*call, None, dst_off.data_ptr(), dst.data_ptr(), stream_bytes, hip_stream=hs)
    fill_ms, lo, hi, _ = timed(fill_call)
    say("%-9s take, fill mode (a)                %9.3f ms  (min %.3f, max %.3f)  reads %.1f MB, writes as much" % (name, fill_ms, lo, hi, stream_bytes / 1e6))
    del dst, dst_off

    def report(label, fn, entries, payload):
        med, lo, hi, inner = timed(fn)
        say("%-9s %-34s %9.3f ms  (min %.3f, max %.3f)  = %.3f x take fill (a), %.2f x take size   %7.1f M entries/s, reads %.1f MB = %.1f GB/s = "
            "%.1f %% of HBM peak  [%d calls per window]"
            % (name, label, med, lo, hi, med / fill_ms, med / size_ms, entries / med / 1e3, payload / 1e6, payload / med / 1e6,
               100 * payload / (med * 1e-3) / HBM_PEAK, inner))
        return med

    say("%-9s %.4f %% of the records have 1024 bytes and more (the wave path)" % (name, 100 * long_share))
    report("hash, all records", lambda: ctx.hash_batch_device(*call, SEED, h.data_ptr(), None, hip_stream=hs), m, stream_bytes)
    report("hash, all records, rec_len written", lambda: ctx.hash_batch_device(*call, SEED, h.data_ptr(), rec_len.data_ptr(), hip_stream=hs), m,
           stream_bytes)
    distinct = int(torch.unique(h).numel())
    say("%-9s %d distinct keys among the %d records" % (name, distinct, m))
    perm = rng.permutation(m)
    sel_stream = torch.from_numpy(all_i[perm].astype(np.int32)).to(dev)
    sel_rec = torch.from_numpy(all_k[perm].astype(np.int64)).to(dev)
    pcall = head + tabs + (1, 0, sel_stream.data_ptr(), sel_rec.data_ptr(), m)
    hp, _ = checked("permuted", name, host, tables, pcall, m, all_i[perm], all_k[perm], sample)
    assert torch.equal(hp, h[torch.from_numpy(perm).to(dev)]), "%s: the permuted call's hashes are not the permuted hashes" % name
    report("hash, a random permutation", lambda: ctx.hash_batch_device(*pcall, SEED, hp.data_ptr(), None, hip_stream=hs), m, stream_bytes)
    del sel_stream, sel_rec, hp

    # whole streams: count = 0, every entry on the wave path; the yardstick is the CRC pass over the same streams
    zero = torch.zeros(n, dtype=torch.int64, device=dev)
    wcall = head + (zero.data_ptr(), zero.data_ptr(), None, 0, 1, 0, None, None, n)
    hw = torch.zeros(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.hash_batch_device(*wcall, SEED, hw.data_ptr(), None)
    order = rng.permutation(n)
    picked, budget = [], 3 << 20
    for i in order:  # a sample of whole streams within 3 MiB of oracle work
        if h_lens[i] <= budget:
            picked.append(int(i))
            budget -= int(h_lens[i])
        if len(picked) == 40:
            break
    picked = np.array(picked)
    want = hash_oracle.hash_records(host, h_offs[picked], h_lens[picked], SEED)
    assert np.array_equal(hw.cpu().numpy()[picked], want), "%s whole streams: hashes differ from hash_oracle" % name
    digest = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    crc_ms, lo, hi, _ = timed(lambda: ctx.digest_batch_device(1, *head[:4], digest.data_ptr(), hip_stream=hs))
    say("%-9s digest (CRC-32), whole streams     %9.3f ms  (min %.3f, max %.3f)  %7.1f GB/s" % (name, crc_ms, lo, hi, stream_bytes / crc_ms / 1e6))
    med = report("hash, whole streams", lambda: ctx.hash_batch_device(*wcall, SEED, hw.data_ptr(), None, hip_stream=hs), n, stream_bytes)
    say("%-9s hash, whole streams = %.3f x digest" % (name, med / crc_ms))


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
hash_rates("headline", out, out_off, out_len, out.cpu().numpy())
del out

# ---- 4096 log-uniform lengths (the batch of tools/gpu_take_rate.py) ----------------------------------------------------------
rng = np.random.default_rng(1234)
top = 4 << 20
h_lens = np.clip(np.floor(np.exp(rng.uniform(0.0, np.log(top), 4096))).astype(np.int64), 1, top)
slots = h_lens + rng.integers(0, 64, 4096)
h_offs = np.zeros(4096, dtype=np.int64)
np.cumsum(slots[:-1], out=h_offs[1:])
g = torch.Generator(device=dev)
g.manual_seed(99)
arena = torch.randint(0, 256, (int(h_offs[-1] + slots[-1]),), dtype=torch.uint8, device=dev, generator=g)
hash_rates("ragged", arena, torch.from_numpy(h_offs).to(dev), torch.from_numpy(h_lens).to(dev), arena.cpu().numpy())
ctx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
