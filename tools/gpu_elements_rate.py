#!/usr/bin/env python3
"""Times brx_elements_batch (the elements of the JSON arrays of a decoded batch as selections, on the device) with HIP events, in one
run, over two batches:

  emb       N streams (default 4096) of ROWS lines {"id": .., "emb": [256 floats], "lang": ".."}, keys in shuffled order: every
            array is the wave's (the wave path).
  short     N streams of ROWS lines with a "tags" array of 0 .. 8 short strings and a 4-element "bbox" among other keys: every
            array is its lane's (the lane path).

On each batch: elements_batch in count mode and in fill mode over member's column(s) of openers; THE YARDSTICKS of the same run on the
same batch: the fill-mode brx_index_set_batch call and the fill-mode brx_member_batch call that fed it, and brx_parse_f64_batch over
the emitted elements.  Before timing, status, end, count, records and kinds of the entries of a sample of streams are held to
tests/elements_oracle.py (its byte-serial statement, which never sees pos or what).  Every timed call is warmed up first and timed
`--reps` times in windows of `--inner` back-to-back calls between two events; the median and the spread of the per-call times are
printed.  `--note` goes into the first line (which build of the library this is, where several are compared).
Usage: python tools/gpu_elements_rate.py [--n 4096] [--rows 4] [--short-rows 24] [--reps 9] [--inner 100] [--only emb|short] [--units K] [--note TEXT] [--out FILE]"""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from brotli_rs_amd import brx  # noqa: E402,F401
import brx_knobs  # noqa: E402
import elements_oracle as eo  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--rows", type=int, default=4)
ap.add_argument("--short-rows", type=int, default=24)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=100)
ap.add_argument("--only", default=None)
ap.add_argument("--units", type=int, default=None)  # BRX_EL_UNITS of the library, where it was built with another value than the header's
ap.add_argument("--note", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = brx_knobs.context(0)
stream = torch.cuda.Stream(device=dev)
lines = []
NO_DELIM, SPACES = 1, 16
SET = b"{}[]:,\n"


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


def rates(name, texts, distinct, names):
    n = len(texts)
    lens_h = np.array([len(t) for t in texts], dtype=np.int64)
    offs_h = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens_h, out=offs_h[1:])
    arena = torch.from_numpy(np.frombuffer(b"".join(texts), dtype=np.uint8).copy()).to(dev)
    offs, lens = torch.from_numpy(offs_h[:n].copy()).to(dev), torch.from_numpy(lens_h).to(dev)
    count, open_, pos_off, pos, what = ctx.index_set_batch(arena, offs, lens, delims=SET)
    n_pos = int(pos.numel())
    hs = stream.cuda_stream
    base = (arena.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, arena.numel())
    head = base + (count.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), what.data_ptr(), n_pos)
    say("%-6s %d streams, %.1f MB, %d boundaries (%.1f per KB)" % (name, n, lens_h.sum() / 1e6, n_pos, 1e3 * n_pos / lens_h.sum()))
    row = "%-6s %-44s %8.3f ms  (min %.3f, max %.3f)%s"
    ix_args = (SET, 0x22, 0x5C, 0) + base
    ti, lo, hi = timed(lambda: ctx.index_set_batch_device(*ix_args, None, None, pos_off.data_ptr(), pos.data_ptr(), what.data_ptr(), n_pos,
                                                          hip_stream=hs))
    say(row % (name, "index_set, fill mode (yardstick)", ti, lo, hi, "  %.1f GB/s" % (lens_h.sum() / ti / 1e6)))
    ln, line_off, ss, sr, kind, flags = ctx.member_batch(arena, offs, lens, count, pos_off, pos, what, names)
    M, Q = int(ln.sum().item()), len(names)
    tm, lo, hi = timed(lambda: ctx.member_batch_device(*head, names, None, line_off.data_ptr(), M, ss.data_ptr(), sr.data_ptr(), kind.data_ptr(),
                                                       flags.data_ptr(), hip_stream=hs))
    say(row % (name, "member, fill mode, %d name(s) (yardstick)" % Q, tm, lo, hi, "  = %.2f x index_set fill" % (tm / ti)))
    # the selection: member's columns one behind the other, MISSING entries (the trailing lines) included
    sel_s, sel_r = ss.reshape(-1).contiguous(), sr.reshape(-1).contiguous()
    m = int(sel_s.numel())
    n_elem, el_off, status, end, es, er, ek = ctx.elements_batch(arena, offs, lens, count, pos_off, pos, what, sel_s, sel_r)
    E = int(es.numel())
    # a sample of streams against the byte-serial statement of the oracle
    h = [x.cpu().numpy() for x in (sel_s, sel_r, n_elem, el_off, status, end, er, ek, es)]
    checked = 0
    for j in range(m):
        i = int(h[0][j])
        if i >= distinct:
            continue
        r = int(h[1][j]) if int(h[1][j]) >= 0 else eo.NO_END
        st, e, els = eo.elements_bytes(texts[i], r)
        a = int(h[3][j])
        got = (int(h[4][j]), int(h[5][j]) if st in (eo.OK, eo.UNCLOSED, eo.MISMATCH) else eo.NO_END,
               [(int(h[6][a + t]), int(h[7][a + t])) for t in range(int(h[2][j]))])
        assert got == (st, e, els) and all(int(h[8][a + t]) == i for t in range(len(els))), "%s: entry %d differs from elements_oracle" % (name, j)
        checked += 1
    long_share = float(((end - sel_r) > LONG).sum().item()) / max(m, 1)
    say("%-6s %d entries (%d arrays OK, %d NONE), %d elements; %d entries of %d streams equal tests/elements_oracle.py  [arrays beyond "
        "BRX_EL_LONG = %d: %.1f %%]" % (name, m, int((status == 0).sum().item()), int((status == 1).sum().item()), E, checked, distinct, LONG,
                                       100 * long_share))
    d_n = torch.zeros(m, dtype=torch.int64, device=dev)
    d_st = torch.zeros(m, dtype=torch.uint8, device=dev)
    d_end = torch.zeros(m, dtype=torch.int64, device=dev)
    sel = (sel_s.data_ptr(), sel_r.data_ptr(), m)
    tc, lo, hi = timed(lambda: ctx.elements_batch_device(*head, *sel, d_n.data_ptr(), d_st.data_ptr(), d_end.data_ptr(), hip_stream=hs))
    spread_c = hi - lo
    say(row % (name, "elements, count mode", tc, lo, hi, "  = %.2f x index_set fill, %.2f x member fill, %.1f M arrays/s, %.2f G elements/s"
               % (tc / ti, tc / tm, m / tc / 1e3, E / tc / 1e6)))
    tf, lo, hi = timed(lambda: ctx.elements_batch_device(*head, *sel, None, None, None, el_off.data_ptr(), E, es.data_ptr(), er.data_ptr(),
                                                         ek.data_ptr(), hip_stream=hs))
    say(row % (name, "elements, fill mode", tf, lo, hi, "  = %.2f x index_set fill, %.2f x member fill, %.1f M arrays/s, %.2f G elements/s"
               % (tf / ti, tf / tm, m / tf / 1e3, E / tf / 1e6)))
    val = torch.zeros(max(E, 1), dtype=torch.float64, device=dev)
    pst = torch.zeros(max(E, 1), dtype=torch.uint8, device=dev)
    pc = base + (count.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), n_pos, 1, NO_DELIM | SPACES, es.data_ptr(), er.data_ptr(), E, 0)
    tp, lo, hi = timed(lambda: ctx.parse_f64_batch_device(*pc, val.data_ptr(), pst.data_ptr(), hip_stream=hs))
    say(row % (name, "parse_f64 over the emitted elements (yardstick)", tp, lo, hi, "  %d of %d OK; elements count = %.2f x, fill = %.2f x this"
               % (int((pst == 0).sum().item()), E, tc / tp, tf / tp)))
    return spread_c


def emb_streams(seed):
    rng = np.random.default_rng(seed)

    def line(r):
        row = {"id": r, "emb": [float(np.float32(x)) for x in rng.standard_normal(256)], "lang": "en"}
        keys = list(row)
        rng.shuffle(keys)
        return json.dumps({k: row[k] for k in keys}, separators=(",", ":")).encode() + b"\n"

    return [b"".join(line(r) for r in range(args.rows)) for _ in range(64)]


def short_streams(seed):
    rng = np.random.default_rng(seed)
    words = ["cat", "dog", "a,b", "x]y", "tree", "q", "street sign", "[1]", "car"]

    def line(r):
        row = {"id": r, "tags": [words[int(x)] for x in rng.integers(0, len(words), int(rng.integers(0, 9)))],
               "bbox": [float(np.round(x, 2)) for x in rng.uniform(0, 640, 4)], "ok": True, "src": "web"}
        keys = list(row)
        rng.shuffle(keys)
        return json.dumps({k: row[k] for k in keys}, separators=(",", ":")).encode() + b"\n"

    return [b"".join(line(r) for r in range(args.short_rows)) for _ in range(64)]


_H = open(os.path.join(ROOT, "brotli-rs_amd", "csrc", "brx_elements.h")).read()
LONG = 16 * (args.units or int(re.search(r"#define\s+BRX_EL_UNITS\s+(\d+)u", _H).group(1)))
if args.note:
    say("# " + args.note)
if args.only in (None, "emb"):
    distinct = emb_streams(31)
    rates("emb", [distinct[i % 64] for i in range(args.n)], 8, [b"emb"])
if args.only in (None, "short"):
    distinct = short_streams(32)
    rates("short", [distinct[i % 64] for i in range(args.n)], 8, [b"tags", b"bbox"])
ctx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
