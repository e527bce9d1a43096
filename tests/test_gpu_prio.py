"""Issue priority by turns (brx_hot.S, .Lspecial; BRX_OPTION_PRIO_SHIFT): the waves of a SIMD hold ranks that differ mod 4, and what is
decoded does not depend on the level a wave holds."""
import os

import numpy as np
import pytest

import oracle_py as oracle
from brotli_rs_amd import brx

pytestmark = pytest.mark.gpu

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")


def _read(name):
    with open(os.path.join(DATA, name), "rb") as f:
        return f.read()


def test_ranks_of_coresident_waves_differ():
    """4096 x monkey is the smallest launch that puts four waves on every SIMD (16 on every CU).  Among the streams of one place --
    XCC, SE, SH, CU, SIMD -- whose start-to-end intervals overlap, the ranks in the trace are pairwise different mod 4."""
    n = 4096
    ctx = brx.Context(0, options={"trace": 1})
    try:
        outs, status, out_len = ctx.decode_batch([_read("monkey.compressed")] * n, 1024)
        assert not status.any()
        t = ctx.last_trace(n)
    finally:
        ctx.close()
    st, en = t[:, 0].astype(np.int64), t[:, 1].astype(np.int64)
    assert (st > 0).all() and (st < en).all()
    if int(t[0, 3] >> np.uint64(32)) < n or st.max() >= en.min():
        pytest.skip("fewer than 4096 workgroups were resident at once")
    w = (t[:, 2] & np.uint64(0xffffffff)).astype(np.int64)
    place = ((w >> 16) & 15) << 10 | ((w >> 8) & 255) << 2 | ((w >> 4) & 3)  # XCC_ID | SE, SH, CU | SIMD
    rank = (w >> 20) & 3
    places, counts = np.unique(place, return_counts=True)
    print("places", len(places), "streams per place", sorted(set(counts.tolist())), "shift", sorted(set(((w >> 24) & 31).tolist())))
    assert counts.max() >= 4  # (every stream was resident at once: some SIMD holds four of them)
    bad = []
    for p in places:
        idx = np.flatnonzero(place == p)  # (all intervals overlap here: st.max() < en.min())
        if len(set(rank[idx].tolist())) != len(idx):
            bad.append((int(p), rank[idx].tolist()))
    assert not bad, (len(bad), bad[:8])


NAMES = ["alice29.txt", "asyoulik.txt", "monkey", "ukkonooa", "x"]


@pytest.fixture(scope="module")
def batch():
    """64 streams, their slots back to back at offsets that are no multiples of 16, and what the oracle makes of each."""
    streams = [_read(NAMES[i % len(NAMES)] + ".compressed") for i in range(64)]
    want = {}
    for i, s in enumerate(streams[:len(NAMES)]):
        want[i] = oracle.decode(s)
    caps = [len(want[i % len(NAMES)][1]) + (1, 7, 13, 3, 5)[i % 5] for i in range(64)]
    off = np.cumsum([0] + caps[:-1])
    assert (off % 16 != 0).sum() >= 48
    return streams, caps, want


@pytest.mark.parametrize("loop_build", [0, 1])
@pytest.mark.parametrize("shift", [0, None, 31], ids=["shift0", "default", "shift31"])
def test_results_do_not_depend_on_the_level(batch, shift, loop_build):
    """Status, length and bytes equal the oracle's under both builds of the loop, whatever the rotation: shift 0 turns the level
    every 10 ns, so that every roll of the input staging sees another one and a short stream passes through all four s_setprio
    arms; 31 never changes it."""
    streams, caps, want = batch
    opts = {"loop_build": loop_build}
    if shift is not None:
        opts["prio_shift"] = shift
    ctx = brx.Context(0, options=opts)
    try:
        outs, status, out_len = ctx.decode_batch(streams, caps)
    finally:
        ctx.close()
    for i in range(len(streams)):
        st, exp = want[i % len(NAMES)]
        assert int(status[i]) == st, (i, int(status[i]))
        assert int(out_len[i]) == len(exp), (i, int(out_len[i]))
        assert outs[i] == exp, i
