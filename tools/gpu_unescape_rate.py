#!/usr/bin/env python3
"""Times brx_unescape_batch (every selected record of a decoded batch as the string it spells, on the device) with HIP events, in one
run, over two batches:

  jsonl     N streams (default 4096) of ROWS rows {"id": .., "text": ".."}, the texts of log-uniform lengths 16 B .. 8 KiB with about
            one byte in 40 an escape (\\n, \\", \\\\, \\uXXXX and surrogate pairs), indexed at "{}[]:,\\n" by brx_index_set_batch; timed over
            the `text` values (pairs mode), BRX_TEXT_JSON with BRX_PARSE_SPACES.
  alice29   the lines of N x alice29, decoded on the device, indexed at "\\n", every record as BRX_TEXT_BACKSLASH: there is no escape
            in it, so this is the pure-copy floor.

Yardsticks, timed in the same run over the same entries: brx_take_batch in size mode against the size mode, brx_take_batch in fill mode
(rooms from its own rec_len) against the fill mode (rooms from text_len), and brx_hash_batch.

Before timing, text_len, status and the bytes of a sample of 3000 entries of every batch are held to tests/unescape_oracle.py.  Every
timed call is warmed up first and timed `--reps` times in windows of `--inner` back-to-back calls between two events; the median and
the spread of the per-call times are printed.  The share of the record bytes that lie in records of BRX_TEXT_LONG bytes and more is
printed as an approximation of the wave path's share: the kernel decides on the walk range, which is up to two quotes and the blanks
shorter than the record.
Usage: python tools/gpu_unescape_rate.py [--n 4096] [--rows 24] [--reps 9] [--inner 100] [--out FILE]"""
import argparse
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
import take_oracle  # noqa: E402
import unescape_oracle as uo  # noqa: E402

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
NO_DELIM, TRIM_CR, SPACES = 1, 2, 16
LONG = int(re.search(r"#define\s+BRX_TEXT_LONG\s+(\d+)u", open(os.path.join(ROOT, "brotli-rs_amd", "csrc", "brx_unescape.h")).read()).group(1))


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


def rates(name, arena, offs, lens, host, delims, index_kw, dialect, flags, pick):
    """pick(count, pos_off) -> (sel_stream, sel_rec) device tensors, or None for all-records mode"""
    n = lens.numel()
    h_offs, h_lens = offs.cpu().numpy()[:n], lens.cpu().numpy()
    count, _, pos_off, pos, _ = ctx.index_set_batch(arena, offs[:n], lens, delims=delims, **index_kw)
    n_pos = int(pos.numel())
    sel = pick(count, pos_off)
    if sel is None:
        m, sel_ptrs = n_pos + n, (None, None)
        h_si, h_sk = take_oracle.entries_all_vec(count.cpu().numpy(), pos_off.cpu().numpy(), m)
    else:
        ss, sr = sel[0].to(torch.int32).contiguous(), sel[1].to(torch.int64).contiguous()
        m, sel_ptrs = int(ss.numel()), (ss.data_ptr(), sr.data_ptr())
        h_si, h_sk = ss.cpu().numpy().astype(np.int64), sr.cpu().numpy()
    hs = stream.cuda_stream
    head = (arena.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, arena.numel(), count.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), n_pos, 1)
    call = head + (flags & 3,) + sel_ptrs + (m,)
    ucall = head + (flags,) + sel_ptrs + (m, dialect, uo.QT, uo.ESC)
    tables = (h_offs, h_lens, count.cpu().numpy(), pos_off.cpu().numpy(), pos.cpu().numpy(), n_pos)
    rec_len = torch.zeros(m, dtype=torch.int64, device=dev)
    text_len = torch.zeros(m, dtype=torch.int64, device=dev)
    st = torch.zeros(m, dtype=torch.uint8, device=dev)
    h = torch.zeros(m, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.take_batch_device(*call, rec_len.data_ptr())
    ctx.unescape_batch_device(*ucall, text_len.data_ptr(), st.data_ptr())
    L = rec_len.cpu().numpy()
    rec_bytes, text_bytes = int(L.sum()), int(text_len.sum().item())
    t_off = torch.cumsum(rec_len, 0) - rec_len
    u_off = torch.cumsum(text_len, 0) - text_len
    t_dst = torch.zeros(max(rec_bytes, 1), dtype=torch.uint8, device=dev)
    u_dst = torch.zeros(max(text_bytes, 1), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.unescape_batch_device(*ucall, None, None, u_off.data_ptr(), u_dst.data_ptr(), text_bytes)
    say("%-8s %d streams, %.1f MB; %d entries, %.1f MB of records (%.0f bytes each on average), %.1f MB of text; %.1f %% of the record bytes "
        "in records of %d bytes and more (about the wave path's share: the kernel decides on the text between the blanks and the quotes)"
        % (name, n, int(h_lens.sum()) / 1e6, m, rec_bytes / 1e6, rec_bytes / m, text_bytes / 1e6, 100.0 * L[L >= LONG].sum() / max(rec_bytes, 1), LONG))
    # a sample against the oracle
    rng = np.random.default_rng(2026)
    sample = np.sort(rng.choice(m, min(m, 3000), replace=False))
    src, sl = take_oracle.records_vec(host, *tables, 1, flags & 3, h_si[sample], h_sk[sample])
    assert np.array_equal(sl, L[sample]), "%s: the record lengths of the sample differ from take_oracle" % name
    raw = host.tobytes() if len(host) < (1 << 28) else None
    g_len, g_st, g_off = text_len.cpu().numpy()[sample], st.cpu().numpy()[sample], u_off.cpu().numpy()[sample]
    for k in range(len(sample)):
        r = raw[int(src[k]):int(src[k]) + int(sl[k])] if raw is not None else host[int(src[k]):int(src[k]) + int(sl[k])].tobytes()
        text, status = uo.text_re(r, dialect, spaces=bool(flags & SPACES))
        assert (len(text), status) == (int(g_len[k]), int(g_st[k])), "%s: entry %d differs from unescape_oracle" % (name, sample[k])
        assert u_dst[int(g_off[k]):int(g_off[k]) + len(text)].cpu().numpy().tobytes() == text, "%s: the text of entry %d differs" % (name, sample[k])
    share = torch.bincount(st.to(torch.int64), minlength=4).cpu().numpy() / m
    say("%-8s sample of %d entries equals tests/unescape_oracle.py  [%s]"
        % (name, len(sample), ", ".join("%s %.1f %%" % (("OK", "BARE", "NULL", "BAD")[k], 100 * share[k]) for k in range(4) if share[k] > 0)))
    row = "%-8s %-34s %8.3f ms  (min %.3f, max %.3f)  %7.1f M entries/s  %7.1f GB/s of record bytes%s"
    ts, lo, hi = timed(lambda: ctx.take_batch_device(*call, rec_len.data_ptr(), hip_stream=hs))
    say(row % (name, "take, size mode", ts, lo, hi, m / ts / 1e3, rec_bytes / ts / 1e6, ""))
    tf, lo, hi = timed(lambda: ctx.take_batch_device(*call, None, t_off.data_ptr(), t_dst.data_ptr(), rec_bytes, hip_stream=hs))
    say(row % (name, "take, fill mode", tf, lo, hi, m / tf / 1e3, rec_bytes / tf / 1e6, ""))
    th, lo, hi = timed(lambda: ctx.hash_batch_device(*call, 1, h.data_ptr(), None, hip_stream=hs))
    say(row % (name, "hash", th, lo, hi, m / th / 1e3, rec_bytes / th / 1e6, ""))
    us, lo, hi = timed(lambda: ctx.unescape_batch_device(*ucall, text_len.data_ptr(), st.data_ptr(), hip_stream=hs))
    say(row % (name, "unescape, size mode", us, lo, hi, m / us / 1e3, rec_bytes / us / 1e6, "  = %.2f x take size, %.2f x hash" % (us / ts, us / th)))
    uf, lo, hi = timed(lambda: ctx.unescape_batch_device(*ucall, None, None, u_off.data_ptr(), u_dst.data_ptr(), text_bytes, hip_stream=hs))
    say(row % (name, "unescape, fill mode", uf, lo, hi, m / uf / 1e3, rec_bytes / uf / 1e6, "  = %.2f x take fill, %.2f x hash" % (uf / tf, uf / th)))
    ub, lo, hi = timed(lambda: ctx.unescape_batch_device(*ucall, text_len.data_ptr(), st.data_ptr(), u_off.data_ptr(), u_dst.data_ptr(), text_bytes,
                                                         hip_stream=hs))
    say(row % (name, "unescape, fill mode + len, status", ub, lo, hi, m / ub / 1e3, rec_bytes / ub / 1e6, "  = %.2f x take fill" % (ub / tf)))


def batch_of(texts):
    """texts (bytes, one per stream) -> arena, offs (n + 1), lens on the device, and the arena on the host"""
    lens_h = np.array([len(t) for t in texts], dtype=np.int64)
    offs_h = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum(lens_h, out=offs_h[1:])
    host = np.frombuffer(b"".join(texts), dtype=np.uint8)
    return torch.from_numpy(host.copy()).to(dev), torch.from_numpy(offs_h).to(dev), torch.from_numpy(lens_h).to(dev), host


# ---- (a) JSON Lines -------------------------------------------------------------------------------------------------------------------
def jsonl_streams(seed):
    rng = np.random.default_rng(seed)
    escapes = [b"\\n", b"\\n", b'\\"', b"\\\\", b"\\t", b"\\/", b"\\u00e9", b"\\u20ac", b"\\ud83d\\ude00"]
    words = [b"the", b"quick", b"brown", b"fox", b"jumps", b"over", b"a", b"lazy", b"dog", b"and", b"keeps", b"running", b"7", b"2024"]

    def text():
        want = int(np.exp(rng.uniform(np.log(16), np.log(8192))))
        out = bytearray()
        while len(out) < want:
            out += words[int(rng.integers(0, len(words)))] + b" "
            if rng.random() < 0.12:  # (words are about 5 bytes: one escape byte in about 40)
                out += escapes[int(rng.integers(0, len(escapes)))]
        return bytes(out)

    return [b"".join(b'{"id": %d, "text": "%s"}\n' % (r, text()) for r in range(args.rows)) for _ in range(64)]


def pick_text(count, pos_off):
    n = count.numel()
    streams = torch.repeat_interleave(torch.arange(n, device=dev), count + 1)
    rec = torch.arange(streams.numel(), device=dev) - (pos_off + torch.arange(n, device=dev))[streams]
    keep = rec % 6 == 4
    return streams[keep], rec[keep]


distinct = jsonl_streams(21)
arena, offs, lens, host = batch_of([distinct[i % 64] for i in range(args.n)])
rates("jsonl", arena, offs, lens, host, b"{}[]:,\n", {}, uo.JSON, NO_DELIM | TRIM_CR | SPACES, pick_text)
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
rates("alice29", out, out_off, out_len, out.cpu().numpy(), b"\n", dict(no_quote=True, no_escape=True), uo.BACKSLASH, NO_DELIM | TRIM_CR,
      lambda count, pos_off: None)
ctx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
