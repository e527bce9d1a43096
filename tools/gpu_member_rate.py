#!/usr/bin/env python3
"""Times brx_member_batch (the named members of the JSON Lines objects of a decoded batch as selections, on the device) with HIP events,
in one run, over two batches:

  jsonl     N streams (default 4096) of ROWS rows {"id": .., "text": ".."}: the batch of tools/gpu_unescape_rate.py (texts of
            log-uniform lengths 16 B .. 8 KiB, one byte in 40 an escape).
  mixed     N streams of ROWS rows with 12 keys in shuffled order, two nested values per row (an object and an array that repeat key
            names) and one optional key.

On each batch: member_batch in count mode and in fill mode with 1, 2 and 8 names; the fill-mode brx_index_set_batch call that fed it
(THE YARDSTICK: the index pass on the same batch in the same run); brx_parse_batch over the emitted "id" column.  Before timing,
lines, kinds, records and flags of a sample of streams are held to tests/member_oracle.py (its byte-serial statement, which never
sees pos or what).  Every timed call is warmed up first and timed `--reps` times in windows of `--inner` back-to-back calls between
two events; the median and the spread of the per-call times are printed.
Usage: python tools/gpu_member_rate.py [--n 4096] [--rows 24] [--reps 9] [--inner 100] [--out FILE]"""
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
import member_oracle as mo  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--rows", type=int, default=24)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=100)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = brx_knobs.context(0)
stream = torch.cuda.Stream(device=dev)
lines = []
NO_DELIM, SPACES = 1, 16


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


def rates(name, texts, distinct, name_sets):
    n = len(texts)
    lens_h = np.array([len(t) for t in texts], dtype=np.int64)
    offs_h = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens_h, out=offs_h[1:])
    arena = torch.from_numpy(np.frombuffer(b"".join(texts), dtype=np.uint8).copy()).to(dev)
    offs, lens = torch.from_numpy(offs_h[:n].copy()).to(dev), torch.from_numpy(lens_h).to(dev)
    count, open_, pos_off, pos, what = ctx.index_set_batch(arena, offs, lens, delims=mo.SET)
    n_pos = int(pos.numel())
    hs = stream.cuda_stream
    base = (arena.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, arena.numel())
    head = base + (count.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), what.data_ptr(), n_pos)
    say("%-6s %d streams, %.1f MB, %d boundaries (%.1f per KB)" % (name, n, lens_h.sum() / 1e6, n_pos, 1e3 * n_pos / lens_h.sum()))
    row = "%-6s %-40s %8.3f ms  (min %.3f, max %.3f)%s"
    ix_args = (mo.SET, 0x22, 0x5C, 0) + base
    ti, lo, hi = timed(lambda: ctx.index_set_batch_device(*ix_args, None, None, pos_off.data_ptr(), pos.data_ptr(), what.data_ptr(), n_pos,
                                                          hip_stream=hs))
    say(row % (name, "index_set, fill mode (the yardstick)", ti, lo, hi, "  %.1f GB/s" % (lens_h.sum() / ti / 1e6)))
    for names in name_sets:
        ln, line_off, ss, sr, kind, flags = ctx.member_batch(arena, offs, lens, count, pos_off, pos, what, names)
        M, Q = int(ln.sum().item()), len(names)
        # a sample of streams against the byte-serial statement of the oracle
        for i in range(distinct):
            want = mo.members_bytes(texts[i], names)
            a = int(line_off[i].item())
            assert int(ln[i].item()) == want[0], "%s: lines of stream %d differ from member_oracle" % (name, i)
            g_kind, g_rec, g_fl = kind[:, a:a + want[0]].cpu().numpy(), sr[:, a:a + want[0]].cpu().numpy(), flags[a:a + want[0]].cpu().numpy()
            for r in range(want[0]):
                assert int(g_fl[r]) == want[2][r]
                for q in range(Q):
                    kd, rec = want[1][r].get(q, (mo.MISSING, -1))
                    assert (int(g_kind[q, r]), int(g_rec[q, r])) == (kd, rec), "%s: stream %d line %d name %d differs" % (name, i, r, q)
        share = torch.bincount(kind.flatten().to(torch.int64), minlength=5).cpu().numpy() / max(Q * M, 1)
        say("%-6s %d name(s): %d lines, %d slots; %d streams equal tests/member_oracle.py  [%s; lines with flags: %d]"
            % (name, Q, M, Q * M, distinct, ", ".join("%s %.1f %%" % (mo.KIND_NAMES[k], 100 * share[k]) for k in range(5) if share[k] > 0),
               int((flags != 0).sum().item())))
        d_lines = torch.zeros(n, dtype=torch.int64, device=dev)
        tc, lo, hi = timed(lambda: ctx.member_batch_device(*head, names, d_lines.data_ptr(), hip_stream=hs))
        say(row % (name, "member, count mode, %d name(s)" % Q, tc, lo, hi, "  = %.2f x index_set fill" % (tc / ti)))
        tf, lo, hi = timed(lambda: ctx.member_batch_device(*head, names, None, line_off.data_ptr(), M, ss.data_ptr(), sr.data_ptr(),
                                                           kind.data_ptr(), flags.data_ptr(), hip_stream=hs))
        say(row % (name, "member, fill mode, %d name(s)" % Q, tf, lo, hi, "  = %.2f x index_set fill, %.1f M lines/s, %.2f G boundaries/s"
                   % (tf / ti, M / tf / 1e3, n_pos / tf / 1e6)))
        if names[0] == b"id":
            s0, r0 = ss[0].contiguous(), sr[0].contiguous()
            val = torch.zeros(M, dtype=torch.int64, device=dev)
            st = torch.zeros(M, dtype=torch.uint8, device=dev)
            pc = base + (count.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), n_pos, 1, NO_DELIM | SPACES, s0.data_ptr(), r0.data_ptr(), M, 0, 0, 0)
            tp, lo, hi = timed(lambda: ctx.parse_batch_device(*pc, val.data_ptr(), st.data_ptr(), hip_stream=hs))
            ok = int((st == 0).sum().item())
            say(row % (name, "parse over the emitted id column", tp, lo, hi, "  %d of %d OK" % (ok, M)))


# ---- (a) the JSON Lines batch of tools/gpu_unescape_rate.py -----------------------------------------------------------------------
def jsonl_streams(seed):
    rng = np.random.default_rng(seed)
    escapes = [b"\\n", b"\\n", b'\\"', b"\\\\", b"\\t", b"\\/", b"\\u00e9", b"\\u20ac", b"\\ud83d\\ude00"]
    words = [b"the", b"quick", b"brown", b"fox", b"jumps", b"over", b"a", b"lazy", b"dog", b"and", b"keeps", b"running", b"7", b"2024"]

    def text():
        want = int(np.exp(rng.uniform(np.log(16), np.log(8192))))
        out = bytearray()
        while len(out) < want:
            out += words[int(rng.integers(0, len(words)))] + b" "
            if rng.random() < 0.12:
                out += escapes[int(rng.integers(0, len(escapes)))]
        return bytes(out)

    return [b"".join(b'{"id": %d, "text": "%s"}\n' % (r, text()) for r in range(args.rows)) for _ in range(64)]


# ---- (b) 12 keys in shuffled order, two nested values and one optional key per row --------------------------------------------------
def mixed_streams(seed):
    rng = np.random.default_rng(seed)
    scalars = [b"id", b"text", b"lang", b"score", b"ts", b"ok", b"note", b"k", b"src"]

    def row(r):
        items = [(b"id", b"%d" % r), (b"text", b'"row %d, with a comma: and a \\"quote\\""' % r), (b"lang", b'"en"'), (b"score", b"%.3f" % rng.random()),
                 (b"ts", b'"2024-05-21T10:00:00Z"'), (b"ok", b"true"), (b"note", b"null"), (b"k", b"%d" % int(rng.integers(0, 1 << 30))),
                 (b"src", b'"web"'), (b"user", b'{"id": %d, "text": "nested", "geo": [1.5, 2.5]}' % (r + 1)),
                 (b"tags", b'[{"id": 1, "text": "a"}, {"id": 2}]'), (b"geo", b'"here"')]
        if rng.random() < 0.5:
            items.pop()  # the optional key
        order = rng.permutation(len(items))
        return b"{" + b", ".join(b'"%s": %s' % items[int(x)] for x in order) + b"}\n"

    assert len(scalars) + 3 == 12
    return [b"".join(row(r) for r in range(args.rows)) for _ in range(64)]


eight = [b"id", b"text", b"user", b"tags", b"geo", b"score", b"ts", b"k"]
sets = [[b"id"], [b"id", b"text"], eight]
distinct = jsonl_streams(21)
rates("jsonl", [distinct[i % 64] for i in range(args.n)], 8, sets)
distinct = mixed_streams(22)
rates("mixed", [distinct[i % 64] for i in range(args.n)], 8, sets)
ctx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
