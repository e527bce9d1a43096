#!/usr/bin/env python3
"""Times brx_object_batch (the named members of the nested JSON objects of a decoded batch as selections, on the device) with HIP
events, in one run, over two batches:

  short     N streams (default 4096) of ROWS lines {"meta":{"lang":..,"score":..},"items":[0 .. 8 x {"id":..,"price":..}],"text":..},
            keys in shuffled order: every object is its lane's (the lane path).  Openers: member's column of "meta" and the elements
            of "items".
  long      N streams of LONG_ROWS lines {"id":..,"doc":{about 600 members, some of them nested, "title" and "score" among them},
            "arr":[as many numbers as the document has boundaries]}: every object is the wave's (the wave path).  Openers: member's
            column of "doc".

On each batch: object_batch with 2 names, with 8 names and in extent mode; THE YARDSTICKS of the same run on the same batch: the
fill-mode brx_index_set_batch call, the fill-mode brx_member_batch call with as many names (the one that fed the selection), and
brx_elements_batch in count mode over comparable openers ("items" / "arr").  Before timing, every output for the entries of a sample
of streams is held to tests/object_oracle.py (its byte-serial statement, which never sees pos or what).  Every timed call is warmed up
first and timed `--reps` times in windows of `--inner` back-to-back calls between two events; the median and the min - max spread of
the per-call times are printed.  `--note` goes into the first line (which build of the library this is, where several are compared).
Usage: python tools/gpu_object_rate.py [--n 4096] [--rows 24] [--long-rows 2] [--reps 9] [--inner 100] [--only short|long] [--units K] [--note TEXT] [--out FILE]"""
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
import object_oracle as oo  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--rows", type=int, default=24)
ap.add_argument("--long-rows", type=int, default=2)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=100)
ap.add_argument("--only", default=None)
ap.add_argument("--units", type=int, default=None)  # BRX_OB_UNITS of the library, where it was built with another value than the header's
ap.add_argument("--note", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = brx_knobs.context(0)
stream = torch.cuda.Stream(device=dev)
lines = []
SET = b"{}[]:,\n"
PAD = [b"pad_one", b"pad_two", b"pad_three", b"pad_four", b"pad_five", b"pad_six"]  # names that no key carries: 2 + 6 = 8 names


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


def rates(name, texts, distinct, top, obj_col, arr_col, via_elements, names):
    """top: the names of the member call; obj_col / arr_col: which of them holds the objects (or the array of objects, with
    via_elements) and the array for the elements yardstick; names: the two names asked of every object."""
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
    tabs = (arena, offs, lens, count, pos_off, pos, what)
    say("%-6s %d streams, %.1f MB, %d boundaries (%.1f per KB)" % (name, n, lens_h.sum() / 1e6, n_pos, 1e3 * n_pos / lens_h.sum()))
    row = "%-6s %-46s %8.3f ms  (min %.3f, max %.3f)%s"
    ix_args = (SET, 0x22, 0x5C, 0) + base
    ti, lo, hi = timed(lambda: ctx.index_set_batch_device(*ix_args, None, None, pos_off.data_ptr(), pos.data_ptr(), what.data_ptr(), n_pos,
                                                          hip_stream=hs))
    say(row % (name, "index_set, fill mode (yardstick)", ti, lo, hi, "  %.1f GB/s" % (lens_h.sum() / ti / 1e6)))
    ln, line_off, ss, sr, kind, flags = ctx.member_batch(*tabs, top)
    M = int(ln.sum().item())
    tm, lo, hi = timed(lambda: ctx.member_batch_device(*head, top, None, line_off.data_ptr(), M, ss.data_ptr(), sr.data_ptr(), kind.data_ptr(),
                                                       flags.data_ptr(), hip_stream=hs))
    say(row % (name, "member, fill mode, %d names (yardstick)" % len(top), tm, lo, hi, "  = %.2f x index_set fill" % (tm / ti)))
    # the elements yardstick: count mode over the column of arrays
    a_s, a_r = ss[arr_col].contiguous(), sr[arr_col].contiguous()
    d_n = torch.zeros(M, dtype=torch.int64, device=dev)
    d_st = torch.zeros(M, dtype=torch.uint8, device=dev)
    d_end = torch.zeros(M, dtype=torch.int64, device=dev)
    te, lo, hi = timed(lambda: ctx.elements_batch_device(*head, a_s.data_ptr(), a_r.data_ptr(), M, d_n.data_ptr(), d_st.data_ptr(), d_end.data_ptr(),
                                                         hip_stream=hs))
    stream.synchronize()
    say(row % (name, "elements, count mode, %d openers (yardstick)" % M, te, lo, hi, "  %d elements, %d boundaries walked"
               % (int(d_n.sum().item()), int((d_end - a_r)[d_st == 0].sum().item()))))
    # the selection of object openers
    if via_elements:  # member's column of the objects and the objects of the array, one behind the other
        n_elem, el_off, est, eend, es, er, ek = ctx.elements_batch(*tabs, a_s, a_r)
        sel_s, sel_r = torch.cat([ss[obj_col], es]).contiguous(), torch.cat([sr[obj_col], er]).contiguous()
    else:
        sel_s, sel_r = ss[obj_col].contiguous(), sr[obj_col].contiguous()
    m = int(sel_s.numel())
    n_mem, status, end, ms, mr, mk, fl = ctx.object_batch(*tabs, sel_s, sel_r, names)
    # a sample of streams against the byte-serial statement of the oracle
    h = [x.cpu().numpy() for x in (sel_s, sel_r, n_mem, status, end, fl)] + [ms.cpu().numpy(), mr.cpu().numpy(), mk.cpu().numpy()]
    checked = 0
    for j in range(m):
        i = int(h[0][j])
        if i >= distinct:
            continue
        r = int(h[1][j]) if int(h[1][j]) >= 0 else oo.NO_END
        st, e, members, found, flags_ = oo.object_bytes(texts[i], r, names)
        got = (int(h[3][j]), int(h[4][j]) & ((1 << 64) - 1), int(h[2][j]), {q: (int(h[8][q][j]), int(h[7][q][j])) for q in range(len(names)) if h[8][q][j]},
               int(h[5][j]))
        assert got == (st, e, members, found, flags_) and all(int(h[6][q][j]) == i for q in range(len(names))), \
            "%s: entry %d differs from object_oracle: %r, want %r" % (name, j, got, (st, e, members, found, flags_))
        checked += 1
    ok = status == 0
    walked = int((end - sel_r)[ok].sum().item())
    long_share = float(((end - sel_r)[ok] > LONG).sum().item()) / max(int(ok.sum().item()), 1)
    say("%-6s %d entries (%d objects OK, %d NONE), %d members, %d boundaries walked, %d slots found; %d entries of %d streams equal "
        "tests/object_oracle.py  [objects beyond BRX_OB_LONG = %d: %.1f %%]"
        % (name, m, int(ok.sum().item()), int((status == 1).sum().item()), int(n_mem.sum().item()), walked, int((mk != 0).sum().item()), checked,
           distinct, LONG, 100 * long_share))
    sel = (sel_s.data_ptr(), sel_r.data_ptr(), m)
    o_n = torch.zeros(m, dtype=torch.int64, device=dev)
    o_st = torch.zeros(m, dtype=torch.uint8, device=dev)
    o_end = torch.zeros(m, dtype=torch.int64, device=dev)
    o_fl = torch.zeros(m, dtype=torch.uint8, device=dev)
    o_ms = torch.zeros(8 * m, dtype=torch.int32, device=dev)
    o_mr = torch.zeros(8 * m, dtype=torch.int64, device=dev)
    o_mk = torch.zeros(8 * m, dtype=torch.uint8, device=dev)
    spreads = []
    for label, nm in (("2 names", names), ("8 names", names + PAD)):
        t, lo, hi = timed(lambda: ctx.object_batch_device(*head, *sel, nm, o_n.data_ptr(), o_st.data_ptr(), o_end.data_ptr(), o_ms.data_ptr(),
                                                          o_mr.data_ptr(), o_mk.data_ptr(), o_fl.data_ptr(), hip_stream=hs))
        spreads.append(hi - lo)
        say(row % (name, "object, " + label, t, lo, hi, "  = %.2f x index_set fill, %.2f x member fill, %.2f x elements count, %.1f M objects/s, "
                   "%.2f G boundaries/s" % (t / ti, t / tm, t / te, m / t / 1e3, walked / t / 1e6)))
    t, lo, hi = timed(lambda: ctx.object_batch_device(*head, *sel, [], o_n.data_ptr(), o_st.data_ptr(), o_end.data_ptr(), hip_stream=hs))
    say(row % (name, "object, extent mode", t, lo, hi, "  = %.2f x index_set fill, %.2f x member fill, %.2f x elements count, %.1f M objects/s, "
               "%.2f G boundaries/s" % (t / ti, t / tm, t / te, m / t / 1e3, walked / t / 1e6)))
    return spreads


def short_streams(seed):
    rng = np.random.default_rng(seed)
    langs = ["en", "de", "pt-BR", "ja", "a}{:b"]

    def line(r):
        row = {"meta": {"lang": langs[int(rng.integers(0, len(langs)))], "score": float(np.round(rng.uniform(0, 1), 3))},
               "items": [{"id": int(x), "price": float(np.round(rng.uniform(0, 99), 2))} for x in rng.integers(0, 10**6, int(rng.integers(0, 9)))],
               "text": "some {text}: with, structure", "id": r}
        keys = list(row)
        rng.shuffle(keys)
        return json.dumps({k: row[k] for k in keys}, separators=(",", ":")).encode() + b"\n"

    return [b"".join(line(r) for r in range(args.rows)) for _ in range(64)]


def long_streams(seed):
    rng = np.random.default_rng(seed)

    def line(r):
        doc = {}
        for k in range(600):
            t = int(rng.integers(0, 10))
            doc["k%04d" % k] = [int(k), {"title": "inner", "score": 0}] if t == 0 else {"a": k, "title": [1, 2]} if t == 1 else "v{%d}:," % k if t == 2 else k
            if k == 300:
                doc["title"] = "the %d-th document" % r
            if k == 560:
                doc["score"] = float(np.round(rng.uniform(0, 1), 4))
        row = {"id": r, "doc": doc, "arr": [int(x) for x in rng.integers(0, 1000, 2000)]}
        keys = list(row)
        rng.shuffle(keys)
        return json.dumps({k: row[k] for k in keys}, separators=(",", ":")).encode() + b"\n"

    return [b"".join(line(r) for r in range(args.long_rows)) for _ in range(64)]


_H = open(os.path.join(ROOT, "brotli-rs_amd", "csrc", "brx_object.h")).read()
LONG = 16 * (args.units or int(re.search(r"#define\s+BRX_OB_UNITS\s+(\d+)u", _H).group(1)))
if args.note:
    say("# " + args.note)
if args.only in (None, "short"):
    distinct = short_streams(41)
    rates("short", [distinct[i % 64] for i in range(args.n)], 8, [b"meta", b"items"], 0, 1, True, [b"score", b"price"])
if args.only in (None, "long"):
    distinct = long_streams(42)
    rates("long", [distinct[i % 64] for i in range(args.n)], 4, [b"doc", b"arr"], 0, 1, False, [b"title", b"score"])
ctx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
