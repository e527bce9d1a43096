#!/usr/bin/env python3
"""R of a stream: how many of its literal runs are entered with pending bytes (brx_hot.S, LIT_CTX_ENTRY), counted on the CPU from the
oracle's command trace with the loop's own rules for what stays pending (.Lcopy, .Ldict, .Ldict_xform): a window copy joins the
pending lanes when the lanes in use, its own included, are at most 63 and at most its distance; one that only fits alone lands the
others first; an overlapping or longer one is written at once; an identity dictionary word joins up to 63 lanes; a transformed word
joins when at most 23 lanes are in use (the Uppercase forms, which land, are counted as joining: an upper bound).  What the count
leaves out: the loop's hand-overs to the C++ side (a run behind one is entered with nothing pending), so R is an upper bound by the
number of those.  Usage: tools/count_run_entries.py <stream.compressed> [window bits, default 22]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import asm_emu  # noqa: E402
import craft  # noqa: E402

out, cmds = asm_emu.oracle_trace(sys.argv[1])
window = (1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 22)) - 16
pending = runs = entered = words = 0
for k, c in enumerate(cmds):
    pos, ins, n = c[0], c[2], c[3]
    if ins:
        runs += 1
        entered += pending > 0
        pending = 0
    if len(c) <= 8:
        continue
    dist, at = c[8], pos + ins
    produced = (cmds[k + 1][0] if k + 1 < len(cmds) else len(out)) - at
    if dist > min(at, window):  # a dictionary word
        words += 1
        if (dist - min(at, window) - 1) >> craft.NDBITS[n] == 0:
            pending = pending + n if pending + n <= 63 else n
        else:
            pending = 0 if pending > 23 else pending
            pending = 0 if pending + produced == 1 else pending + produced
    elif n <= dist and pending + n <= min(dist, 63):
        pending += n
    else:
        pending = n if n <= min(dist, 63) else 0
print("%d commands, %d literals in %d runs, %d dictionary words; R = %d runs entered with pending bytes"
      % (len(cmds), sum(c[2] for c in cmds), runs, words, entered))
