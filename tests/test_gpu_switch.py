"""Block switching in all three block categories against the CPU oracle, through every implementation of it.

The table of the 26 block count codes is written three times (hd_block_count and read_block_count / K_BLEN in brx_kernels.hip,
.Lswitch in brx_hot.S), the block type rule twice (cat_tick, .Lswitch), and the assembly loop ticks its three counters at eleven
places.  switch_cases.py builds streams that use all of it -- every count code as a first count, as a later count between complete
general codes (the assembly's switch) and as a later count behind a simple or one-symbol code (the C++ side's), every kind of block
type symbol, switches next to commands that do not tick -- and asserts, on the CPU, that they do (its census).  Here they are decoded:
on the default choice of the loop's build, on both builds forced, and with the C++ loop alone (command_loop=6)."""
import functools
import time

import numpy as np
import pytest

import brx_knobs
import craft
import oracle_py as oracle
import switch_cases

pytestmark = pytest.mark.gpu

BUILDS = [{}, {"loop_build": 0}, {"loop_build": 1}]


def _id(opts):
    return "-".join("%s=%d" % kv for kv in sorted(opts.items())) or "default"


@functools.lru_cache(maxsize=None)
def _want(name):
    """(stream, oracle status, oracle output) of a case; a valid case's output is the builder's own model of it."""
    c = {c.name: c for c in switch_cases.all_cases()}[name]
    st, out = oracle.decode(c.stream, 0, cap=len(c.out) + 64)
    if c.valid:
        assert st == 0 and out == c.out, (name, st, len(out), len(c.out))
    else:
        assert st not in (0, oracle.STATUS_OUTPUT_TOO_SMALL) and c.out[:len(out)] == out, (name, st)
    return c.stream, st, out


def _decode(ctx, streams, caps):
    """-> (status, out_len, [the slot's first min(out_len, capacity) bytes])"""
    n = len(streams)
    in_off = np.zeros(n + 1, dtype=np.uint64)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    in_off[1:] = np.cumsum([len(s) for s in streams])
    out_off[1:] = np.cumsum(caps)
    blob = np.frombuffer(b"".join(streams) + bytes(64), dtype=np.uint8)
    out = np.zeros(int(out_off[-1]) + 64, dtype=np.uint8)
    status, out_len = ctx.decode_batch_host_raw(blob.ctypes.data, in_off, n, out.ctypes.data, out_off)
    got = [out[int(out_off[i]):int(out_off[i]) + min(int(out_len[i]), caps[i])].tobytes() for i in range(n)]
    return status, out_len, got


def _mismatches(want, status, out_len, got):
    """want: [(oracle status, oracle output)].  A valid stream: status, length and bytes; an invalid one: the status, and the bytes in
    front of the error as far as both sides report them (how far into the failing command out_len points is not specified)."""
    bad = []
    for i, (st, ref) in enumerate(want):
        if int(status[i]) != st:
            bad.append((i, "status", st, int(status[i])))
        elif st == 0 and (int(out_len[i]) != len(ref) or got[i] != ref):
            bad.append((i, "bytes", len(ref), int(out_len[i])))
        elif st != 0 and got[i][:len(ref)] != ref[:len(got[i])]:
            bad.append((i, "prefix", len(ref), int(out_len[i])))
    return bad


def _run(opts, names_streams_want, caps=None):
    """Decode [(name, stream, status, output)] in one batch: slots of len + 16 and a few ragged bytes, so that slot alignments differ."""
    streams = [s for _, s, _, _ in names_streams_want]
    want = [(st, ref) for _, _, st, ref in names_streams_want]
    caps = caps or [len(ref) + 16 + (5 * i) % 13 for i, (_, ref) in enumerate(want)]
    c = brx_knobs.context(0, **opts)
    try:
        t = time.perf_counter()
        status, out_len, got = _decode(c, streams, caps)
        dt = time.perf_counter() - t
    finally:
        c.close()
    bad = [(names_streams_want[b[0]][0],) + b[1:] for b in _mismatches(want, status, out_len, got)]
    return bad, dt


def _batch(kinds):
    """The cases of these kinds three times over, each time in another order: a wave meets a switching stream behind a plain one and
    the other way round."""
    names = [c.name for c in switch_cases.all_cases() if c.kind in kinds]
    items = [(n,) + _want(n) for n in names]
    stream, out = craft.context_mode_stream(2, 5)  # (one block type per category: no switch at all)
    plain = ("plain", stream) + oracle.decode(stream, 0, cap=len(out) + 64)
    assert plain[2:] == (0, out)
    order2 = sorted(items, key=lambda it: len(it[1]))
    order3 = items[::-1]
    batch = []
    for rep in (items, order2, order3):
        for k, it in enumerate(rep):
            batch.append(it)
            if k % 3 == 0:
                batch.append(plain)
    return batch


@pytest.mark.parametrize("opts", BUILDS + [{"command_loop": 6}], ids=_id)
def test_every_case(opts):
    """Every small, all-codes, three-meta-block and invalid case in one batch, three times in three orders: status, length and bytes
    are the oracle's.  top_bit is left out here: with the C++ loop alone (command_loop=6) its 8.4 million literals would take many
    seconds at that loop's cost per literal; it has a test of its own on the assembly builds, and command_loop=6 covers count code
    25 with extras up to 0xFFFF through the all-codes streams."""
    batch = _batch(("small", "all_codes", "three", "invalid"))
    assert len(batch) > 150
    bad, _ = _run(opts, batch)
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("opts", BUILDS, ids=_id)
def test_top_bit_of_a_24_bit_count(opts):
    """Count code 25 with extra 2^23 + 5: the top bit of the 24 extra bits, a literal block of 8 405 238 literals under a one-symbol
    tree, then 40 000 literals of another type and back with symbol 0."""
    name, (stream, st, ref) = "top_bit", _want("top_bit")
    bad, dt = _run(opts, [(name, stream, st, ref)])
    print("top_bit: %.3f s for the decode call (%s)" % (dt, _id(opts)))
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def _cuts():
    items, caps = [], []
    for name, s, full in switch_cases.truncations():
        st, ref = oracle.decode(s, 0, cap=len(full) + 64)
        assert st not in (0, oracle.STATUS_OUTPUT_TOO_SMALL) and full[:len(ref)] == ref, (name, len(s), st)
        items.append(("%s[:%d]" % (name, len(s)), s, st, ref))
        caps.append(len(full) + 64)
    return items, caps


@pytest.mark.parametrize("opts", [{}, {"command_loop": 6}], ids=_id)
def test_truncated_at_every_byte(opts):
    """Three small streams -- switching mostly literals, mostly insert&copy, mostly distances -- cut at every byte, one batch: the loop
    runs on behind the real end with poisoned counters (LBLEN_REAL, IBLEN_REAL) and a switch near the end is the C++ side's.  Status
    and the bytes in front of the error are the oracle's."""
    items, caps = _cuts()
    assert len(items) > 1500
    bad, _ = _run(opts, items, caps)
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("opts", [{"levels": 0}, {"levels": 2}], ids=_id)
def test_levels(opts):
    """The streams with 100 trees (DESC_GATHER) and with 256 block types (maps that outgrow the table memory of the regular
    instance) under plans A and B: whichever kernel instance takes them must be right."""
    names = [c.name for c in switch_cases.all_cases() if "ntl100" in c.name or "ntd100" in c.name or "256_types" in c.name]
    assert len(names) >= 6
    items = [(n,) + _want(n) for n in names]
    bad, _ = _run(opts, items * 2)
    assert not bad, (len(bad), bad[:8])
