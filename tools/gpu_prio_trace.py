"""Diagnostics: how evenly the waves of a SIMD share one launch (BRX_OPTION_TRACE) -- per-stream durations, the same by AGE RANK
within the SIMD (start order among the waves of one place: XCC, SE, SH, CU, SIMD), and whether the co-resident waves of every SIMD
hold wave slots / priority ranks that differ mod 4 (brx_hot.S, .Lspecial: issue priority by turns).
    python tools/gpu_prio_trace.py [workload [label [prio_shift]]]      (default alice29x4096; prio_shift: the option, if given)
A library from before the option (no XCC_ID in the trace word: bits 19:16 then hold HW_ID's TG_ID) is told by `label` = parent:
the XCC then comes from the workgroup index (workgroup i runs on XCD i % 8) and there are no ranks."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import bench, brx_knobs

wl = sys.argv[1] if len(sys.argv) > 1 else "alice29x4096"
label = sys.argv[2] if len(sys.argv) > 2 else "new"
old = label == "parent"
more = {"prio_shift": int(sys.argv[3])} if len(sys.argv) > 3 else {}
names, n = bench.WORKLOADS[wl]
fx = [bench.load_fixture(f) for f in names]
ctx = brx_knobs.context(0, trace=1, **more)
b = bench.Batch(torch, np, torch.device("cuda:0"), fx, n)
for rep in range(3):
    b.step(ctx, timing=True); ctx.synchronize()
t = ctx.last_trace(n)
ms = ctx.last_timing_ms(1)
ok = b.verify(torch)
ctx.close()

live = t[:, 0] > 0  # (streams of the lean instance have all-zero records)
t = t[live]
st, en = t[:, 0].astype(np.int64), t[:, 1].astype(np.int64)
dur = (en - st) / 100.0  # us
w2 = t[:, 2] & np.uint64(0xffffffff)
hw = w2.astype(np.int64)
slot, simd, cu, sh, se = hw & 15, (hw >> 4) & 3, (hw >> 8) & 15, (hw >> 12) & 1, (hw >> 13) & 7
wg = (t[:, 3] & np.uint64(0xffffffff)).astype(np.int64)
xcc = wg % 8 if old else (hw >> 16) & 15
rank = slot * 0 - 1 if old else (hw >> 20) & 3
shift = -1 if old else int((hw[0] >> 24) & 31)
place = (((xcc * 8 + se) * 2 + sh) * 16 + cu) * 4 + simd


def four(x):
    return "min %9.1f  median %9.1f  mean %9.1f  max %9.1f" % (x.min(), np.median(x), x.mean(), x.max())


print("== %s  %s  prio_shift %s  kernel ms %.4f  ok %s  streams traced %d of %d" % (label, wl, shift if shift >= 0 else "-", ms, ok, len(t), n))
print("launch: first start to last end %.1f us; (max - mean) / max of the stream durations = %.4f" % ((en.max() - st.min()) / 100.0, (dur.max() - dur.mean()) / dur.max()))
print("HW_ID fields seen: XCC %s  SE %s  SH %s  CU %s  SIMD %s  wave slot %s" % tuple(sorted(set(x.tolist())) for x in (xcc, se, sh, cu, simd, slot)))
print("places %d, streams per place: %s" % (len(set(place.tolist())), dict(zip(*[x.tolist() for x in np.unique(np.unique(place, return_counts=True)[1], return_counts=True)]))))
print("duration us, all streams:        " + four(dur))
# age rank: start order among the streams of one place whose intervals overlap the place's first stream (one round of waves)
age = np.full(len(t), -1)
bad_slot, bad_rank, full = 0, 0, 0
for p in np.unique(place):
    idx = np.flatnonzero(place == p)
    idx = idx[np.argsort(st[idx], kind="stable")]
    age[idx] = np.arange(len(idx))
    # co-resident: every pair whose [start, end) intervals overlap
    ov = (st[idx][:, None] < en[idx][None, :]) & (st[idx][None, :] < en[idx][:, None]) & ~np.eye(len(idx), dtype=bool)
    full += int((ov.sum(axis=1) >= 3).any())
    same = lambda v: bool((ov & ((v[idx][:, None] & 3) == (v[idx][None, :] & 3))).any())
    bad_slot += same(slot)
    if not old:
        bad_rank += same(rank)
for a in range(int(age.max()) + 1):
    if (age == a).sum() >= 8:
        print("duration us, age rank %d (%4d):  " % (a, (age == a).sum()) + four(dur[age == a]))
print("SIMDs with four or more co-resident waves: %d" % full)
print("SIMDs where two co-resident waves hold the same wave slot mod 4: %d of %d" % (bad_slot, len(np.unique(place))))
if not old:
    print("SIMDs where two co-resident waves hold the same rank mod 4:      %d of %d" % (bad_rank, len(np.unique(place))))
for p in np.unique(place)[:3]:  # a few places as they are
    idx = np.flatnonzero(place == p); idx = idx[np.argsort(st[idx], kind="stable")]
    print("  place xcc %d se %d sh %d cu %2d simd %d: " % (xcc[idx[0]], se[idx[0]], sh[idx[0]], cu[idx[0]], simd[idx[0]]) +
          "  ".join("slot %d rank %s start +%.1f us dur %.1f" % (slot[i], rank[i] if not old else "-", (st[i] - st.min()) / 100.0, dur[i]) for i in idx[:6]))
