"""The rule of brx_index_set_batch (include/brx.h) on the CPU, twice: serial() is the state machine as the contract states it, vec()
the same in numpy so that streams of megabytes cost nothing.  tests/test_index_set_abi.py holds the one to the other and both to
escaped_oracle; tests/test_gpu_index_set.py takes every expected value from vec()."""
import numpy as np

import escaped_oracle

# the check values of the contract
J = b'{"a":"x,\\"y:}","b":[1,2]}\n{"c":"\\\\"}\n{"open":"[\\'
J_SET = b"{}[]:,\n"
J_POS = [0, 4, 14, 18, 19, 21, 23, 24, 25, 26, 30, 35, 36, 37, 44]
J_WHAT = b"{:,:[,]}\n{:}\n{:"
C = b'a,"b,c\n",d\r\ne,"f""g",h\n"x'
C_SET = b",\n\r"
C_POS_NO_ESCAPE = [1, 8, 10, 11, 13, 20, 22]
C_WHAT_NO_ESCAPE = b",,\r\n,,\n"
C_POS_PLAIN = [1, 4, 6, 8, 10, 11, 13, 20, 22]


def serial(s, delims, Q, E, no_quote=False, no_escape=False):
    """s: bytes or a uint8 array -> (positions of the boundaries, the bytes there, open): byte by byte, esc(j + 1) = (s[j] == E and
    not esc(j)), an active quote toggles, a byte of `delims` counts where it is neither escaped nor inside."""
    delims = bytes(delims)
    pos, what, esc, q = [], [], 0, 0
    for j, b in enumerate(bytes(bytearray(s))):
        if not esc and b in delims and not q:
            pos.append(j)
            what.append(b)
        if not esc and not no_quote and b == Q:
            q ^= 1
        esc = int(not no_escape and b == E and not esc)
    return np.array(pos, dtype=np.int64), np.array(what, dtype=np.uint8), q | (esc << 1)


def states(s, Q, E, no_quote=False, no_escape=False):
    """-> the state in front of every byte and behind the last, len(s) + 1 entries: bit 0 = parity of the active quotes in front of
    it, bit 1 = it is escaped (the bits of open[]).  No delimiter takes part in it."""
    s = np.asarray(s, dtype=np.uint8)
    esc = np.zeros(s.size + 1, dtype=bool) if no_escape else escaped_oracle.escaped(s, E)
    active = np.zeros(s.size, dtype=np.int64) if no_quote else ((s == Q) & ~esc[:-1]).astype(np.int64)
    par = np.concatenate(([0], np.cumsum(active))) & 1
    return (par | (esc.astype(np.int64) << 1)).astype(np.int64)


def vec(s, delims, Q, E, no_quote=False, no_escape=False):
    """serial() in numpy -> (positions, what, open)"""
    s = np.asarray(s, dtype=np.uint8)
    st = states(s, Q, E, no_quote, no_escape)
    member = np.zeros(256, dtype=bool)
    member[np.frombuffer(bytes(delims), dtype=np.uint8)] = True
    pos = np.flatnonzero(member[s] & (st[:-1] == 0))
    return pos.astype(np.int64), s[pos].copy(), int(st[-1])
