"""The rule of brx_index_escaped_batch (include/brx.h) on the CPU, twice: serial() is the state machine as the contract states it,
vec() the same in numpy so that streams of megabytes cost nothing.  tests/test_index_escaped_abi.py holds the one to the other;
tests/test_gpu_index_escaped.py takes every expected value from vec()."""
import numpy as np


def serial(s, D, Q, E, no_quote=False):
    """s: bytes or a uint8 array -> (positions of the record delimiters, open): byte by byte, esc(j + 1) = (s[j] == E and not esc(j)),
    an active quote toggles, a delimiter counts where it is neither escaped nor inside."""
    pos, esc, q = [], 0, 0
    for j, b in enumerate(bytes(bytearray(s))):
        if not esc and b == D and not q:
            pos.append(j)
        if not esc and not no_quote and b == Q:
            q ^= 1
        esc = int(b == E and not esc)
    return np.array(pos, dtype=np.int64), q | (esc << 1)


def escaped(s, E):
    """-> esc(0 .. len(s)) as a bool array of len(s) + 1 entries: byte j is escaped iff the run of E bytes directly in front of it
    has odd length.  The run in front of j is j - 1 - (index of the last byte before j that is not E), the latter by a running maximum
    over the indices of the non-E bytes."""
    s = np.asarray(s, dtype=np.uint8)
    n = s.size
    idx = np.where(s != E, np.arange(n, dtype=np.int64), -1)
    last = np.concatenate(([-1], np.maximum.accumulate(idx) if n else idx))  # last[j]: last non-E index < j, or -1
    run = np.arange(n + 1, dtype=np.int64) - 1 - last
    return (run & 1).astype(bool)


def states(s, D, Q, E, no_quote=False):
    """-> the state in front of every byte and behind the last, len(s) + 1 entries: bit 0 = parity of the active quotes in front of
    it, bit 1 = it is escaped (the bits of open[])."""
    s = np.asarray(s, dtype=np.uint8)
    esc = escaped(s, E)
    active = np.zeros(s.size, dtype=np.int64) if no_quote else ((s == Q) & ~esc[:-1]).astype(np.int64)
    par = np.concatenate(([0], np.cumsum(active))) & 1
    return (par | (esc.astype(np.int64) << 1)).astype(np.int64)


def vec(s, D, Q, E, no_quote=False):
    """serial() in numpy -> (positions, open)"""
    s = np.asarray(s, dtype=np.uint8)
    st = states(s, D, Q, E, no_quote)
    pos = np.flatnonzero((s == D) & (st[:-1] == 0))
    return pos.astype(np.int64), int(st[-1])
