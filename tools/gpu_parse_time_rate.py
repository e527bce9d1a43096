#!/usr/bin/env python3
"""Times brx_parse_time_batch (every selected record of a decoded batch as a date, a time or a timestamp, on the device) with HIP
events, in one run, over two batches:

  log       N streams (default 4096) of ROWS rows `stamp,level,int,float`, the stamps RFC 3339 with milliseconds and a numeric zone
            ("2024-03-10T07:08:09.123+05:30"), an eighth of all fields in quotes or between blanks, indexed at ",\\n" by
            brx_index_set_batch: every field is a record, a quarter of them stamps.
  alice29   the lines of N x alice29, decoded on the device, indexed at "\\n": none is a stamp -- the early-out cost.

Yardsticks, timed in the same run over the same entries: brx_take_batch in size mode (the rule alone), brx_hash_batch (the same tables
and the same bytes) and brx_parse_batch with BRX_PARSE_DEC at scale 2.

Before timing, val, status and zone of a sample of 3000 entries of every case are held to tests/parse_time_oracle.py.  Every timed call
is warmed up first and timed `--reps` times in windows of `--inner` back-to-back calls between two events; the median and the spread
of the per-call times are printed.
Usage: python tools/gpu_parse_time_rate.py [--n 4096] [--rows 48] [--reps 9] [--inner 100] [--out FILE]"""
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
import parse_oracle as po  # noqa: E402
import parse_time_oracle as to  # noqa: E402
import take_oracle  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--rows", type=int, default=48)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=100)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = brx_knobs.context(0)
stream = torch.cuda.Stream(device=dev)
lines = []
NO_DELIM, TRIM_CR = 1, 2
SQ = to.SPACES | to.QUOTED


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    """fn() enqueues one call on `stream`.  -> (median, min, max) milliseconds per call"""
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


def rates(name, arena, offs, lens, host, delims, cases):
    """cases: (scale, with zone, parse flags)"""
    n = lens.numel()
    h_offs, h_lens = offs.cpu().numpy()[:n], lens.cpu().numpy()
    stream_bytes = int(h_lens.sum())
    count, _, pos_off, pos, _ = ctx.index_set_batch(arena, offs[:n], lens, delims=delims, no_quote=True, no_escape=True)
    n_pos = int(pos.numel())
    m = n_pos + n
    hs = stream.cuda_stream
    call = (arena.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, arena.numel(), count.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), n_pos, 1,
            NO_DELIM | TRIM_CR, None, None, m)
    tables = (h_offs, h_lens, count.cpu().numpy(), pos_off.cpu().numpy(), pos.cpu().numpy(), n_pos)
    say("%-8s %d streams, %.1f MB, %d records (%.1f bytes each on average, delimiters included)" % (name, n, stream_bytes / 1e6, m, stream_bytes / m))
    rng = np.random.default_rng(2026)
    all_i, all_k = take_oracle.entries_all_vec(tables[2], tables[3], m)
    sample = np.sort(rng.choice(m, min(m, 3000), replace=False))
    src, L = take_oracle.records_vec(host, *tables, 1, NO_DELIM | TRIM_CR, all_i[sample], all_k[sample])
    h = torch.zeros(m, dtype=torch.int64, device=dev)
    ival = torch.zeros(m, dtype=torch.int64, device=dev)
    val = torch.zeros(m, dtype=torch.int64, device=dev)
    st = torch.zeros(m, dtype=torch.uint8, device=dev)
    zn = torch.zeros(m, dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    take_ms, lo, hi = timed(lambda: ctx.take_batch_device(*call, h.data_ptr(), hip_stream=hs))
    say("%-8s take, size mode                      %8.3f ms  (min %.3f, max %.3f)  %7.1f M entries/s" % (name, take_ms, lo, hi, m / take_ms / 1e3))
    hash_ms, lo, hi = timed(lambda: ctx.hash_batch_device(*call, 1, h.data_ptr(), None, hip_stream=hs))
    say("%-8s hash                                 %8.3f ms  (min %.3f, max %.3f)  %7.1f M entries/s" % (name, hash_ms, lo, hi, m / hash_ms / 1e3))
    dec_ms = {}
    for scale, with_zone, pf in cases:
        label = "scale %d, %s%s" % (scale, "zone" if with_zone else "no zone", ", SPACES | QUOTED" if pf else "")
        dcall = call[:10] + (NO_DELIM | TRIM_CR | pf,) + call[11:] + (po.DEC, 2, 0x22)
        if pf not in dec_ms:
            torch.cuda.synchronize()
            ctx.parse_batch_device(*dcall, ival.data_ptr(), st.data_ptr())
            want, wst = po.parse_records("fsm", host, src, L, po.DEC, 2, bool(pf & po.SPACES), 0x22 if pf & po.QUOTED else None)
            assert np.array_equal(ival.cpu().numpy()[sample], want) and np.array_equal(st.cpu().numpy()[sample], wst), \
                "%s %s: the DEC sample differs from parse_oracle" % (name, label)
            dec_ms[pf], lo, hi = timed(lambda: ctx.parse_batch_device(*dcall, ival.data_ptr(), st.data_ptr(), hip_stream=hs))
            say("%-8s parse DEC scale 2%-19s %8.3f ms  (min %.3f, max %.3f)  = %.2f x hash  %7.1f M entries/s"
                % (name, ", SPACES | QUOTED" if pf else "", dec_ms[pf], lo, hi, dec_ms[pf] / hash_ms, m / dec_ms[pf] / 1e3))
        tcall = call[:10] + (NO_DELIM | TRIM_CR | pf,) + call[11:] + (to.STAMP, scale, 0x22)
        zp = zn.data_ptr() if with_zone else None
        zn.fill_(-1)
        torch.cuda.synchronize()
        ctx.parse_time_batch_device(*tcall, val.data_ptr(), st.data_ptr(), zp)
        want, wst, wzn = to.parse_records("fsm", host, src, L, to.STAMP, scale, bool(pf & to.SPACES), 0x22 if pf & to.QUOTED else None)
        assert np.array_equal(val.cpu().numpy()[sample], want) and np.array_equal(st.cpu().numpy()[sample], wst), \
            "%s %s: the sample differs from parse_time_oracle" % (name, label)
        assert np.array_equal(zn.cpu().numpy()[sample], wzn) if with_zone else (zn == -1).all().item(), "%s %s: zone" % (name, label)
        share = torch.bincount(st.to(torch.int64), minlength=6).cpu().numpy() / m
        med, lo, hi = timed(lambda: ctx.parse_time_batch_device(*tcall, val.data_ptr(), st.data_ptr(), zp, hip_stream=hs))
        say("%-8s parse STAMP %-36s %8.3f ms  (min %.3f, max %.3f)  = %.2f x DEC scale 2, %.2f x hash, %.2f x take  %7.1f M entries/s, "
            "%.1f GB/s of stream bytes  [%s]"
            % (name, label, med, lo, hi, med / dec_ms[pf], med / hash_ms, med / take_ms, m / med / 1e3, stream_bytes / med / 1e6,
               ", ".join("%s %.1f %%" % (to.NAMES[k], 100 * share[k]) for k in sorted(to.NAMES) if share[k] > 0)))


def batch_of(texts):
    """texts (bytes, one per stream) -> arena, offs (n + 1), lens on the device, and the arena on the host"""
    lens_h = np.array([len(t) for t in texts], dtype=np.int64)
    offs_h = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum(lens_h, out=offs_h[1:])
    host = np.frombuffer(b"".join(texts), dtype=np.uint8)
    return torch.from_numpy(host.copy()).to(dev), torch.from_numpy(offs_h).to(dev), torch.from_numpy(lens_h).to(dev), host


# ---- (a) the synthetic log batch ------------------------------------------------------------------------------------------------------------
def rows_of(seed):
    rng = np.random.default_rng(seed)

    def dress(f):
        r = rng.integers(0, 16)
        return b'"' + f + b'"' if r == 0 else (b" " + f + b"  " if r == 1 else f)

    def ri(lo, hi):
        return int(rng.integers(lo, hi))

    def row():
        zm = ri(-14 * 4, 14 * 4 + 1) * 15
        stamp = b"%04d-%02d-%02dT%02d:%02d:%02d.%03d%s%02d:%02d" % (ri(1990, 2040), ri(1, 13), ri(1, 29), ri(0, 24), ri(0, 60), ri(0, 60), ri(0, 1000),
                                                                   b"+" if zm >= 0 else b"-", abs(zm) // 60, abs(zm) % 60)
        f = [stamp, (b"INFO", b"WARN", b"ERROR", b"DEBUG")[ri(0, 4)], b"%d" % ri(0, 10 ** 6), b"%r" % float(rng.normal())]
        return b",".join(dress(x) for x in f) + b"\n"

    return [b"".join(row() for _ in range(args.rows)) for _ in range(64)]


CASES = [(scale, z, pf) for pf in (0, SQ) for scale in (0, 3, 9) for z in (False, True)]
distinct = rows_of(21)
arena, offs, lens, host = batch_of([distinct[i % 64] for i in range(args.n)])
rates("log", arena, offs, lens, host, b",\n", CASES)
del arena

# ---- (b) the lines of N x alice29, decoded on the device ---------------------------------------------------------------------------------
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
rates("alice29", out, out_off, out_len, out.cpu().numpy(), b"\n", [(3, True, 0), (3, True, SQ)])
ctx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
