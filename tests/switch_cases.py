"""Block switching in all three block categories: hand-assembled streams, their expected output and a census of what they reach.

craft.many_trees_stream switches literals and distances with type symbols 0 / 1 and two of the 26 block count codes.  The builder
here generalises its category / count / tick helpers: one compressed meta-block from a PLAN -- NBLTYPES of L, I and D; per category
a block type code and a block count code, each a complete complex code, a simple code of 2 .. 4 symbols or a one-symbol code, with
scripts that say which type symbols and which (count code, extra) pairs come first; one context mode per literal block type;
NTREESL / NTREESD with context maps; one insert&copy tree per insert&copy block type; and a command source.  The builder computes
the output itself (literal bytes from the context rules, the distance ring, copies, dictionary words under the identity transform),
and the trees differ from type to type so that a wrong type is a wrong byte: literal tree t holds the bytes 2t and 2t + 1, distance
tree t one ring code and one explicit code chosen by t, the insert&copy tree of type t gives symbol t (mod the alphabet in use)
the one-bit codeword.

While it emits, the builder counts what it emitted into CENSUS; all_cases() asserts every key of census_keys() non-zero before it
returns, so the tests that decode these streams cannot pass on less than the census names.  Test tooling only."""
import collections
import functools
import os
import random

import craft
from craft import Bits, CELL, CPY_BASE, CPY_EXTRA, INS_BASE, INS_EXTRA, code_bits, complex_code, context_id, simple_code, uniform_lengths

# block count code -> (base, extra bits), RFC 7932 section 6
BLEN = [(1, 2), (5, 2), (9, 2), (13, 2), (17, 3), (25, 3), (33, 3), (41, 3), (49, 4), (65, 4), (81, 4), (97, 4), (113, 5), (145, 5),
        (177, 5), (209, 5), (241, 6), (305, 6), (369, 7), (497, 8), (753, 9), (1265, 10), (2289, 11), (4337, 12), (8433, 13),
        (16625, 24)]
CATS = "LID"
DICT = open(os.path.join(craft.ROOT, "brotli-rs_amd", "tables", "dictionary.bin"), "rb").read()
DICT_CODE = 36          # distance code 16 + hcode 20: 11 extra bits, distances 4093 .. 6140 (NPOSTFIX = NDIRECT = 0)
DICT_BASE = 4093
RAW = 300               # bytes of the uncompressed meta-block in front: every ring and explicit distance is inside the output

# insert&copy vocabulary: (insert code, copy code, implicit distance)
VOCAB = ([(ic, cc, False) for ic in (0, 1, 2, 3, 4, 6) for cc in (0, 2, 5)]
         + [(1, cc, False) for cc in (8, 9, 10, 11, 13, 14, 15)]
         + [(2, 12, False), (0, 16, False), (1, 16, False), (10, 0, False), (14, 2, False), (18, 0, False), (20, 2, False)]
         + [(ic, cc, True) for ic in (0, 1, 3, 6) for cc in (0, 3)] + [(2, 12, True)])
LEAN = [(1, 0, False), (0, 0, False), (1, 0, True), (3, 0, False), (2, 2, False)]
TWO = [(1, 0, False), (3, 0, False)]
SINGLE_ENTRY = (1, 0, False)

CENSUS = collections.Counter()


def iac_sym(ic, cc, implicit):
    if implicit:
        assert ic < 8 and cc < 16
        return 64 * (cc >> 3) + 8 * ic + (cc & 7)
    return 64 * CELL[(ic >> 3, cc >> 3)] + 8 * (ic & 7) + (cc & 7)


class Code:
    """A prefix code as it is sent: kind 'complex' (a complete general code), 'simple' (2 .. 4 symbols) or 'single'."""

    def __init__(self, b, alphabet, kind, symbols, lengths=None):
        self.kind, self.symbols = kind, sorted(symbols)
        bits = max(1, (alphabet - 1).bit_length())
        if kind == "complex":
            assert len(self.symbols) >= 2
            codes = complex_code(b, lengths or uniform_lengths(alphabet, self.symbols), zero_run_17=alphabet > 32)
            self.fields = {s: (craft.rev(c, l), l) for s, (c, l) in codes.items()}
        else:
            assert len(self.symbols) == 1 if kind == "single" else 2 <= len(self.symbols) <= 4, (kind, symbols)
            simple_code(b, self.symbols, bits)
            self.fields = {s: code_bits(self.symbols, s) for s in self.symbols}

    def put(self, b, sym):
        b.put(*self.fields[sym])


class Cat:
    """The state of one block category: NBLTYPES, the current and the previous type, what is left of the count."""

    def __init__(self, M, name, spec):
        self.M, self.name, self.n = M, name, spec.get("n", 1)
        self.cur, self.prev, self.left, self.switches = 0, 1, 1 << 62, 0
        self.last_sym, self.last_was_cur, self.explicit = None, False, set()
        self.tscript, self.cscript = list(spec.get("tscript", ())), list(spec.get("cscript", ()))
        self.pending, self.fallbacks = None, 0
        b, n = M.hb, self.n
        craft._nbltypes(b, n)
        if n < 2:
            return
        tsyms = spec.get("tsyms") or list(range(n + 2))
        self.tcode = Code(b, n + 2, spec.get("tkind", "complex"), tsyms)
        self.ccode = Code(b, 26, spec.get("ckind", "complex"), spec.get("csyms") or [0, 1, 2, 4, 5, 8])
        self.asm = self.tcode.kind == "complex" and self.ccode.kind == "complex"
        self.count("first")

    def count(self, role):
        M, rng = self.M, self.M.rng
        if self.cscript:
            code, extra = self.cscript.pop(0)
        else:  # (a small count, so that the stream goes on switching and ends soon)
            self.fallbacks += 1
            small = [s for s in self.ccode.symbols if BLEN[s][0] <= 48] or self.ccode.symbols[:1]
            code = rng.choice(small if self.name == "L" else small[:2])  # (commands are fewer than literals)
            extra = rng.randrange(1 << min(BLEN[code][1], 4))
        assert code in self.ccode.symbols and extra < (1 << BLEN[code][1])
        self.ccode.put(M.hb, code)
        M.hb.put(extra, BLEN[code][1])
        if self.pending is not None:  # the count before this one was used up: its value has been checked
            prole, pcode, pextra = self.pending
            nb = BLEN[pcode][1]
            CENSUS[(self.name, "count", prole, pcode)] += 1
            if pcode == 25:
                cls = {0: "0", 1: "1", 0xFFFF: "0xFFFF"}.get(pextra, "other")
            else:
                cls = "zero" if pextra == 0 else "max" if pextra == (1 << nb) - 1 else "mid"
            CENSUS[(self.name, "extra", pcode, cls)] += 1
        self.pending = (role, code, extra)
        self.left = BLEN[code][0] + extra

    def type_symbol(self):
        valid = [s for s in self.tcode.symbols if s < self.n + 2]
        while self.tscript:
            e = self.tscript.pop(0)
            e = self.cur + 2 if e == "cur" else e
            if e in valid:
                return e
        return self.M.rng.choice(valid)

    def tick(self):
        """one symbol of the category is about to be read: the block switch in front of it, if its count is used up"""
        if self.left == 0:
            M, name = self.M, self.name
            M.switch_bits.append((name, M.hb.n))
            sym = self.type_symbol()
            self.tcode.put(M.hb, sym)
            new = self.prev if sym == 0 else (self.cur + 1) % self.n if sym == 1 else sym - 2
            assert new < self.n
            CENSUS[(name, "type", "explicit" if sym > 1 else str(sym))] += 1
            if self.switches == 0 and sym == 0:
                CENSUS[(name, "type", "0 first")] += 1
            if sym == 0 and self.last_sym == 0:
                CENSUS[(name, "type", "0 twice")] += 1
            if sym == 1 and self.cur == self.n - 1:
                CENSUS[(name, "type", "1 wraps")] += 1
            if sym == 0 and self.last_was_cur:
                CENSUS[(name, "type", "current, then 0")] += 1
            if sym > 1:
                self.explicit.add(sym)
                if self.n <= 5 and len(self.explicit) == self.n:
                    CENSUS[(name, "type", "every explicit symbol")] += 1
                    self.explicit.add(-1)
            self.last_was_cur = sym > 1 and sym - 2 == self.cur
            self.last_sym = sym
            self.prev, self.cur = self.cur, new
            self.count("asm" if self.asm else "cpp")
            self.switches += 1
        self.left -= 1

    def scripts_done(self):
        return self.n < 2 or (not self.cscript and not self.tscript and self.fallbacks >= 1)  # (the last scripted count is used up)


class Stream:
    def __init__(self, wbits=18, seed=0, raw=RAW):
        self.b, self.out, self.ring = Bits(), bytearray(), [4, 11, 15, 16]
        self.switch_bits, self.switches, self.max_types = [], [0, 0, 0], 1
        craft.stream_header(self.b, wbits)
        if raw:
            data = random.Random(seed).randbytes(raw)
            craft.raw_block(self.b, data)
            self.out += data

    def finish(self):
        stream = self.b.bytes()
        for name, bit in self.switch_bits:
            for tail in (16, 256):
                if 8 * len(stream) - bit <= 8 * tail:
                    CENSUS[(name, "starts in the last %d bytes" % tail)] += 1
        return stream, bytes(self.out)


class MetaBlock:
    """One compressed meta-block of a Stream from a plan (a dict):
      L, I, D     per category: n, tkind / tsyms / tscript (block type code, its symbols, the type symbols to use first -- "cur" names the
                  current type explicitly), ckind / csyms / cscript (block count code, its symbols, (code, extra) pairs first)
      modes       the context mode of every literal block type
      ntl, ntd    NTREESL, NTREESD;  lmap / dmap: "type" (type t -> tree t mod NTREES) or "ctx" (drawn per context id)
      rle         the context maps are sent run-length coded behind a move-to-front transform
      single_l, single_d, single_i: trees (insert&copy: block types) with a one-symbol code
      vocab       the insert&copy symbols in use;  cmds: the commands (ic, cc, implicit, insert, copy), else they are drawn until
                  every script is used up and min_cmds commands are out;  dict: dictionary references are placed"""

    def __init__(self, S, plan, is_last=True):
        self.S, self.plan, self.rng, self.hb = S, plan, random.Random(plan.get("seed", 0)), Bits()
        self.switch_bits = []
        rng, b = self.rng, self.hb
        self.L, self.I, self.D = L, I, D = [Cat(self, c, plan.get(c, {})) for c in CATS]
        S.max_types = max(S.max_types, L.n, I.n, D.n)
        b.put(0, 2); b.put(0, 4)  # NPOSTFIX, NDIRECT
        self.modes = list(plan.get("modes") or [2] * L.n)
        assert len(self.modes) == L.n
        for m in self.modes:
            b.put(m, 2)
        if len(set(self.modes)) > 1:
            CENSUS[("L", "block types of different context modes")] += 1
        ntl, ntd = plan.get("ntl", 1), plan.get("ntd", 1)
        rle = dict(rlemax=6, imtf=True) if plan.get("rle") else {}
        given = [t % ntl for t in range(L.n) for _ in range(64)] if plan.get("lmap", "ctx") == "type" else None
        self.cmap_l = craft.context_map(b, rng, ntl, 64 * L.n, cmap=given, **rle)
        given = [t % ntd for t in range(D.n) for _ in range(4)] if plan.get("dmap", "ctx") == "type" else None
        self.cmap_d = craft.context_map(b, rng, ntd, 4 * D.n, cmap=given, **rle)
        CENSUS[("NTREESL", ntl, "one mode" if len(set(self.modes)) == 1 else "modes %d" % len(set(self.modes)))] += L.n > 1
        CENSUS[("NTREESD", ntd)] += D.n > 1
        single_l, single_d, single_i = (set(plan.get(k, ())) for k in ("single_l", "single_d", "single_i"))
        # literal tree t: the bytes 2t and 2t + 1 (one bit per literal under any tree), or 2t alone (no bits)
        assert ntl <= 128
        self.ltrees = [(2 * t,) if t in single_l else (2 * t, 2 * t + 1) for t in range(ntl)]
        for t in self.ltrees:
            simple_code(b, list(t), 8)
        # (a block type all of whose contexts lead to one one-symbol tree: its literals need no per-literal work)
        self.flat = [len({self.cmap_l[64 * t + c] for c in range(64)}) == 1 and len(self.ltrees[self.cmap_l[64 * t]]) == 1 for t in range(L.n)]
        # insert&copy tree of type t: a complete code over the vocabulary's symbols, the one-bit codeword on symbol t mod k
        self.vocab = list(plan.get("vocab") or VOCAB)
        syms = sorted(iac_sym(*e) for e in self.vocab)
        assert len(set(syms)) == len(syms)
        self.itrees = []
        for t in range(I.n):
            if t in single_i:
                self.itrees.append(Code(b, 704, "single", [iac_sym(*SINGLE_ENTRY)]))
                continue
            lens = [0] * 704
            if len(syms) == 2:
                lens[syms[0]] = lens[syms[1]] = 1
            else:
                rest = [s for s in syms if s != syms[t % len(syms)]]
                lens[syms[t % len(syms)]] = 1
                for s, l in zip(rest, uniform_lengths(len(rest))):
                    lens[s] = l + 1
            self.itrees.append(Code(b, 704, "complex", syms, lengths=lens))
        self.single_i = single_i
        # distance tree t: ring code t mod 4 and the explicit code 16 + (t + t / 4) mod 12 (1 .. 6 extra bits, distances 1 .. 252)
        self.dtrees, self.with_dict = [], bool(plan.get("dict"))
        for t in range(ntd):
            rc, ec = t % 4, 16 + (t + t // 4) % 12
            tr = ((rc if t % 2 == 0 else ec,) if t in single_d else (rc, ec) + ((DICT_CODE,) if self.with_dict else ()))
            simple_code(b, list(tr), 6)
            self.dtrees.append(tr)
        self.dict_left = 3 if self.with_dict else 0
        self.long_left = plan.get("long", 2)
        self.start = len(S.out)
        self.prev_cmd = None  # ("copy" / "dict", its length, the literal run ended on a flush block, the literal count ended with the run)
        self.force_ins = 0
        self.ncmds = 0
        self.body(plan)
        # the header in front of what was written: ISLAST, MNIBBLES by MLEN (a zero top nibble is refused), MLEN - 1
        mlen = len(S.out) - self.start
        nib = 4 if mlen <= 1 << 16 else 5 if mlen <= 1 << 20 else 6
        S.b.put(1 if is_last else 0, 1)
        if is_last:
            S.b.put(0, 1)
        S.b.put(nib - 4, 2)
        S.b.put(mlen - 1, 4 * nib)
        if not is_last:
            S.b.put(0, 1)
        S.switch_bits += [(name, S.b.n + bit) for name, bit in self.switch_bits]
        S.b.put(int.from_bytes(self.hb.bytes(), "little"), self.hb.n)
        S.switches = [a + c.switches for a, c in zip(S.switches, (L, I, D))]
        if all(c.n > 1 and c.left == 0 for c in (L, I, D)):
            CENSUS[("meta-block ends with all three counts at zero",)] += 1

    # ---- the command loop -------------------------------------------------------------------------------------------
    def body(self, plan):
        cmds = plan.get("cmds")
        k = 0
        while True:
            last = (k == len(cmds) - 1) if cmds else self.enough(plan)
            self.command(cmds[k] if cmds else None, last)
            k += 1
            if last:
                break
            assert k < plan.get("max_cmds", 400000), "the scripts are not used up"

    def enough(self, plan):
        return (self.ncmds >= plan.get("min_cmds", 60) and len(self.S.out) - self.start >= plan.get("min_out", 0)
                and all(c.scripts_done() for c in (self.L, self.I, self.D)) and not self.force_ins)

    def entry(self, ic, cc, implicit, ins=None, clen=None):
        rng = self.rng
        if ins is None:
            ins = INS_BASE[ic] + (rng.randrange(1 << INS_EXTRA[ic]) if INS_EXTRA[ic] else 0)
        if clen is None:
            clen = CPY_BASE[cc] + (rng.randrange(1 << CPY_EXTRA[cc]) if CPY_EXTRA[cc] else 0)
        return ic, cc, implicit, ins, clen

    def choose(self, last):
        """The next command (ic, cc, implicit, insert, copy, distance kind), after its insert&copy block switch."""
        rng, L, I, D, S = self.rng, self.L, self.I, self.D, self.S
        pos = len(S.out)
        if I.cur in self.single_i:
            return self.entry(*SINGLE_ENTRY) + ("tree",)
        vocab = self.vocab
        if last:  # literals only: the copy is cut off by MLEN
            e = (3, 0, False) if (3, 0, False) in vocab else SINGLE_ENTRY
            return self.entry(*e) + ("tree",)
        if len(vocab) <= 8:
            return self.entry(*rng.choice(vocab)) + ("tree",)
        if self.force_ins:  # (a hook of the command before: this run must reach the literal block switch)
            need, self.force_ins = self.force_ins, 0
            ic = 6 if need <= 6 else 10
            ins = max(need, INS_BASE[ic])
            return self.entry(ic, 0, False, ins=ins) + ("tree",)
        # a dictionary word right in front of a literal block switch
        if self.dict_left and L.n > 1 and L.left == 1 and 3100 <= pos <= 6000 and DICT_CODE in self.dtree_of(4):
            self.dict_left -= 1
            self.force_ins = 1
            return self.entry(1, 2, False) + ("dict",)
        # the insert&copy count is used up with this command: let its literal run end on a flush block
        if I.n > 1 and I.left == 0:
            need = (-pos) % 1024
            for ic in (0, 1, 2, 3, 4, 6, 10, 14, 18, 20):
                if INS_BASE[ic] <= need < INS_BASE[ic] + (1 << INS_EXTRA[ic]) and (ic < 14 or self.long_left > 0):
                    self.long_left -= ic >= 14
                    cc = {10: 0, 14: 2, 18: 0, 20: 2}.get(ic, rng.choice((0, 2, 5)))
                    return self.entry(ic, cc, False, ins=need) + ("tree",)
        # the literal count ends a few literals into the NEXT run: a copy length that puts that literal on a flush block's edge
        if L.n > 1:
            for target in (0, 1, 1023):
                clen = (target - pos - L.left) % 1024
                for ic, cc, imp in vocab:
                    ins = INS_BASE[ic]
                    if not imp and INS_EXTRA[ic] == 0 and ins <= L.left <= ins + 17 and CPY_BASE[cc] <= clen < CPY_BASE[cc] + (1 << CPY_EXTRA[cc]):
                        self.force_ins = L.left - ins + 1
                        return self.entry(ic, cc, False, clen=clen) + ("tree",)
        r = rng.random()
        if r < 0.33:
            pool = [e for e in vocab if e[2] and e[1] < 12]
        elif r < 0.36 and self.long_left > 0:
            self.long_left -= 1
            pool = [e for e in vocab if e[0] >= 14]
        elif r < 0.45:
            pool = [e for e in vocab if e[1] >= 8 or e[0] == 10]
        else:
            pool = [e for e in vocab if not e[2] and e[0] < 10 and e[1] < 8]
        return self.entry(*rng.choice(pool)) + ("tree",)

    def dtree_of(self, clen):
        return self.dtrees[self.cmap_d[4 * self.D.cur + min(clen - 2, 3)]]

    def literals(self, ins):
        S, L, rng, hb, out = self.S, self.L, self.rng, self.hb, self.S.out
        modes, cmap, trees = self.modes, self.cmap_l, self.ltrees
        k = 0
        while k < ins:
            if L.left == 0:
                pos = len(out)
                CENSUS[("L", "switch on the first literal of a run" if k == 0 else "switch inside a run")] += 1
                if pos % 1024 in (0, 1, 1023):
                    CENSUS[("L", "switch at output position mod 1024 =", pos % 1024)] += 1
                if k == 0 and self.prev_cmd and self.prev_cmd[0] == "copy" and self.prev_cmd[1] <= 63:
                    CENSUS[("L", "switch on the first literal behind a copy of at most 63 bytes")] += 1
                if k == 0 and self.prev_cmd and self.prev_cmd[0] == "dict":
                    CENSUS[("L", "switch on the first literal behind a dictionary word")] += 1
                if k == 0 and self.prev_cmd and self.prev_cmd[3]:
                    CENSUS[("L", "count ended exactly with the run before")] += 1
            L.tick()
            bt = L.cur
            if self.flat[bt]:  # a one-symbol tree under every context: the rest of the block (of the run) at once
                n = min(ins - k - 1, L.left)
                out += bytes([trees[cmap[64 * bt]][0]]) * (n + 1)
                L.left -= n
                k += n + 1
                continue
            p1, p2 = out[-1], out[-2]
            t = trees[cmap[64 * bt + context_id(modes[bt], p1, p2)]]
            if len(t) == 1:
                out.append(t[0])
            else:
                bit = rng.getrandbits(1)
                hb.put(bit, 1)
                out.append(t[bit])
            k += 1

    def command(self, given, last):
        S, L, I, D, rng, hb, out = self.S, self.L, self.I, self.D, self.rng, self.hb, self.S.out
        if I.left == 0 and self.prev_cmd:
            kind, n, flush, _ = self.prev_cmd
            CENSUS[("I", "switch behind a copy of more than 64 bytes" if n > 64 else "switch behind a short copy")] += 1
            if flush:
                CENSUS[("I", "switch behind a literal run that ended on a flush block")] += 1
        I.tick()
        ic, cc, implicit, ins, clen, dkind = (self.entry(*given) + ("tree",)) if given else self.choose(last)
        self.ncmds += 1
        self.itrees[I.cur].put(hb, iac_sym(ic, cc, implicit))
        hb.put(ins - INS_BASE[ic], INS_EXTRA[ic])
        hb.put(clen - CPY_BASE[cc], CPY_EXTRA[cc])
        CENSUS[("command", "insert 0" if ins == 0 else "insert 1 .. 4" if ins <= 4 else "insert of 300 and more" if ins >= 300 else "insert 5 .. 299")] += 1
        before = len(out) // 1024
        self.literals(ins)
        if ins >= 300 and len(out) // 1024 > before and L.n > 1:
            CENSUS[("command", "insert across literal blocks and a flush block")] += 1
        flush = ins > 0 and len(out) % 1024 == 0
        ended = L.n > 1 and ins > 0 and L.left == 0
        if last:
            CENSUS[("command", "last copy cut off by MLEN")] += 1
            return
        pos = len(out)
        if implicit:
            CENSUS[("command", "implicit distance")] += 1
            if D.n > 1 and D.left <= 1:
                CENSUS[("D", "implicit distance while the count is", D.left)] += 1
            dist = S.ring[0]
        else:
            if D.left == 0:
                CENSUS[("D", "switch on a command with literals" if ins else "switch on a copy-only command")] += 1
            switched = D.left == 0
            D.tick()
            tr = self.dtree_of(clen)
            if switched and len(tr) == 1:
                CENSUS[("D", "switch onto a one-symbol distance tree")] += 1
            codes = sorted(tr)
            if dkind == "dict":
                idx = max(0, DICT_BASE - pos - 1) + rng.randrange(8)
                dist = pos + 1 + idx
                assert DICT_BASE <= dist < DICT_BASE + 2048 and idx < 1024 and clen == 4
                hb.put(*code_bits(codes, DICT_CODE))
                hb.put(dist - DICT_BASE, 11)
                out += DICT[4 * idx:4 * idx + 4]  # (words of length 4 start the dictionary; transform 0 is the identity)
                CENSUS[("command", "dictionary reference")] += 1
                self.prev_cmd = ("dict", 4, flush, ended)
                return
            ring_ok = [c for c in tr if c < 4 and S.ring[c] <= pos]
            if len(tr) == 1:
                code = tr[0]
            else:
                code = ring_ok[0] if ring_ok and rng.getrandbits(1) else tr[1]
            hb.put(*code_bits(codes, code))
            if code < 4:
                CENSUS[("command", "ring code")] += 1
                dist = S.ring[code]
                assert dist <= pos
                if code:
                    S.ring = [dist] + S.ring[:3]
            else:
                CENSUS[("command", "explicit code with extra bits")] += 1
                hcode = code - 16
                nbits = 1 + (hcode >> 1)
                base = ((2 + (hcode & 1)) << nbits) - 4 + 1
                x = rng.randrange(1 << nbits)
                hb.put(x, nbits)
                dist = base + x
                assert dist <= pos
                S.ring = [dist] + S.ring[:3]
        if dist >= clen:
            out += out[pos - dist:pos - dist + clen]
        else:
            out += (bytes(out[pos - dist:]) * (clen // dist + 1))[:clen]
        self.prev_cmd = ("copy", clen, flush, ended)


# ======================================================================================================== the case list
Case = collections.namedtuple("Case", "name kind stream out valid switches max_types")  # switches: (L, I, D)


def _cat(rng, n, tkind="complex", ckind="complex", csyms=None, cscript=None, tsyms=None):
    """A category's plan with the type script that walks through the census: 0 first, 0 again, the last type and 1 (the wrap), every
    explicit symbol, the current type and 0."""
    spec = dict(n=n, tkind=tkind, ckind=ckind)
    if n < 2:
        return spec
    spec["tscript"] = [0, 0, n + 1, 1] + list(range(2, min(n, 5) + 2)) + ["cur", 0]
    if tkind == "simple":
        tsyms = tsyms or [0, 1, n + 1][:2 if n == 2 and rng.getrandbits(1) else 3]
    elif tkind == "single":
        tsyms = tsyms or [rng.randrange(2)]
    if tsyms:
        spec["tsyms"] = tsyms
    if ckind == "single":
        csyms = csyms or [rng.randrange(3)]
    elif ckind == "simple":
        csyms = csyms or sorted(rng.sample(range(6), 2 + rng.randrange(3)))
    else:
        csyms = csyms or sorted(set([0, 1, 2]) | set(rng.sample(range(3, 10), 3)))
    spec["csyms"] = csyms
    spec["cscript"] = cscript or [(c, rng.randrange(1 << BLEN[c][1])) for c in csyms if BLEN[c][0] <= 60][:3]
    return spec


def _one(name, kind, plan, wbits=18):
    S = Stream(wbits, seed=plan.get("seed", 0))
    MetaBlock(S, plan)
    stream, out = S.finish()
    return Case(name, kind, stream, out, True, tuple(S.switches), S.max_types)


def _small_cases():
    """Streams of 0.5 .. 4 KB: NBLTYPES 2, 3, 5, 16 in every category, NTREESL 1, 2, 12, 13, 40, 100 each with one context mode and with all
    four, NTREESD 1, 4, 100, the three kinds of block type and block count codes."""
    cases = []
    nbls = [(2, 3, 5), (5, 16, 2), (3, 5, 16), (16, 2, 3), (2, 2, 2), (5, 5, 5), (3, 3, 3), (16, 16, 16), (2, 16, 5), (16, 3, 2), (3, 2, 16), (5, 3, 2)]
    kinds = [("complex", "complex"), ("complex", "complex"), ("simple", "complex"), ("complex", "simple"), ("single", "complex"), ("complex", "single")]
    k = 0
    for ntl in (1, 2, 12, 13, 40, 100):
        for mixed in (False, True):
            rng = random.Random(500 + k)
            nl, ni, nd = nbls[k % len(nbls)]
            ntd = (1, 4, 100, 4)[k % 4]
            plan = dict(seed=900 + k, ntl=ntl, ntd=ntd, lmap="type" if k % 3 == 0 else "ctx", dmap="type" if k % 2 else "ctx",
                        modes=[(t + k) % 4 if mixed else k % 4 for t in range(nl)], dict=k % 2 == 0, min_cmds=120, min_out=1800,
                        single_d={1} if ntd == 4 else {3, 8} if ntd == 100 else (), rle=k % 4 == 3)
            for j, (c, n) in enumerate(zip(CATS, (nl, ni, nd))):
                tk, ck = kinds[(k + 2 * j) % len(kinds)] if k >= 4 else kinds[0]
                plan[c] = _cat(rng, n, tk, ck)
            cases.append(_one("small_ntl%d_%s_nbl%d_%d_%d_ntd%d" % (ntl, "modes" if mixed else "mode", nl, ni, nd, ntd), "small", plan))
            k += 1
    # one stream per category with 256 block types: a type symbol of 257 in an alphabet of 258, two-symbol trees; the context maps of
    # 16 384 (literals) and 1 024 (distances) entries are sent run-length coded
    for j, c in enumerate(CATS):
        rng = random.Random(600 + j)
        plan = dict(seed=950 + j, ntl=128 if c == "L" else 2, ntd=100 if c == "D" else 2, lmap="type", dmap="type", rle=True, vocab=TWO,
                    min_cmds=150, min_out=2200, modes=[rng.randrange(4) for _ in range(256)] if c == "L" else [j, 3 - j])
        for d in CATS:
            plan[d] = _cat(rng, 2)
        plan[c] = _cat(rng, 256, tsyms=[0, 1, 130, 257])
        plan[c]["tscript"] = [257, 1, 0, 0, 130, 257, "cur", 0]
        cases.append(_one("small_256_types_%s" % c, "small", plan))
    # the insert&copy tree of one type is a one-symbol code
    rng = random.Random(610)
    plan = dict(seed=960, ntl=4, ntd=4, single_i={1}, modes=[0, 3, 2], min_cmds=150, min_out=1500)
    for c, n in zip(CATS, (3, 3, 2)):
        plan[c] = _cat(rng, n)
    cases.append(_one("small_one_symbol_iac_tree", "small", plan))
    # most of the switches in one category: the streams that are also cut at every byte
    for j, c in enumerate(CATS):
        rng = random.Random(620 + j)
        plan = dict(seed=970 + j, ntl=4, ntd=4, modes=[(t + j) % 4 for t in range(4 if c == "L" else 2)], min_cmds=60, long=0, dict=False)
        for d in CATS:
            plan[d] = _cat(rng, 4, csyms=[0, 1]) if d == c else _cat(rng, 2, csyms=[5, 6, 8] if d == "L" else [3, 4, 5])
        cases.append(_one("small_mostly_%s" % c, "small", plan))
        assert max(cases[-1].switches) == cases[-1].switches[j], cases[-1].switches
    # every command one symbol of each category, the counts such that the meta-block ends with all three at zero
    rng = random.Random(611)
    plan = dict(seed=961, ntl=2, ntd=2, lmap="type", dmap="type", modes=[1, 1], cmds=[(1, 0, False)] * 8)
    for c, counts in zip(CATS, ([(0, 2), (1, 0)], [(0, 3), (0, 3)], [(0, 1), (1, 0)])):  # 3 + 5, 4 + 4 symbols; 2 + 5 distances
        plan[c] = dict(n=2, csyms=[0, 1], cscript=list(counts), tscript=[1])
    cases.append(_one("small_ends_on_zero", "small", plan))
    assert CENSUS[("meta-block ends with all three counts at zero",)]
    return cases


def _big_plan(seed, tkind, cscript):
    plan = dict(seed=seed, ntl=2, ntd=2, lmap="type", dmap="type", modes=[2, 2, 2], vocab=LEAN, min_cmds=50)
    for c in CATS:
        plan[c] = dict(n=3, tkind=tkind, tsyms=None if tkind == "complex" else [1], csyms=sorted({s for s, _ in cscript} | {0, 1}),
                       cscript=list(cscript))
    return plan


def _all_codes_cases():
    """Every one of the 26 count codes, used up, in every category: as a later count between complete general codes (extras 0), as a later
    count behind a one-symbol block type code, which the assembly's switch leaves to the C++ side (the largest extras; code 25 with 0xFFFF), and -- 26 streams -- as the first count of all three
    categories (an extra in between; code 25 with extra 1)."""
    cases = []
    a = [(25, 0)] + [(c, 0) for c in range(26)]
    cases.append(_one("all_codes_extras_0", "all_codes", _big_plan(700, "complex", a), wbits=22))
    m = [(24, (1 << 13) - 1)] + [(c, (1 << BLEN[c][1]) - 1) for c in range(25)] + [(25, 0xFFFF)]
    cases.append(_one("all_codes_largest_extras", "all_codes", _big_plan(701, "single", m), wbits=22))
    for c in range(26):
        nb = BLEN[c][1]
        extra = 1 if c == 25 else 1 + (c * 5) % ((1 << nb) - 2)
        cases.append(_one("first_count_code_%02d" % c, "all_codes", _big_plan(710 + c, "complex", [(c, extra)]), wbits=22))
    return cases


def _top_bit_case(bit=23):
    """The literal category's first count is code 25 with extra 2^bit + 5 under a one-symbol literal tree (no bits per literal), then 40 000
    one-bit literals of a second type -- the switch behind the long block is far from the end of the input --, then back with symbol 0."""
    n0 = 16625 + (1 << bit) + 5
    plan = dict(seed=720, ntl=2, ntd=1, lmap="type", modes=[0, 0], single_l={0}, vocab=[(1, 0, False), (23, 0, False), (3, 0, False)],
                L=dict(n=2, csyms=[0, 25], cscript=[(25, (1 << bit) + 5), (25, 40000 - 16625), (0, 3)], tscript=[1, 0, 0]),
                cmds=[(1, 0, False)] * 3 + [(23, 0, False, n0 + 40000 + 9, 2)] + [(1, 0, False)] * 3)
    S = Stream(24, seed=720)
    MetaBlock(S, plan)
    stream, out = S.finish()
    assert S.switches[0] >= 3 and len(out) > n0 + 40000
    return Case("top_bit", "top_bit", stream, out, True, tuple(S.switches), 2)


def _three_meta_blocks_case():
    """Block types (3, 2, 4) -> (1, 1, 1) -> (2, 5, 1) in one stream: type 0, previous type 1 and "no count" are set anew each time."""
    S = Stream(18, seed=730)
    total = 0
    for k, nbl in enumerate(((3, 2, 4), (1, 1, 1), (2, 5, 1))):
        rng = random.Random(731 + k)
        plan = dict(seed=735 + k, ntl=(3, 1, 2)[k], ntd=(4, 1, 1)[k], lmap="type", dmap="type", modes=[(t + k) % 4 for t in range(nbl[0])],
                    min_cmds=50)
        for c, n in zip(CATS, nbl):
            plan[c] = _cat(rng, n)
        MetaBlock(S, plan, is_last=k == 2)
    stream, out = S.finish()
    return Case("three_meta_blocks", "three", stream, out, True, tuple(S.switches), 5)


def _invalid_cases():
    cases = []
    for kind in ("block_type", "block_count", "type_beyond"):
        for c in CATS:
            info = {}
            stream = craft.incomplete_code_stream(kind, category=c, info=info)
            CENSUS[(c, "invalid", kind)] += 1
            cases.append(Case("invalid_%s_%s" % (kind, c), "invalid", stream, info["model"], False, None, None))
    return cases


def census_keys():
    keys = []
    for c in CATS:
        keys += [(c, "type", k) for k in ("0 first", "0 twice", "1 wraps", "every explicit symbol", "current, then 0")]
        keys += [(c, "count", role, code) for role in ("first", "asm", "cpp") for code in range(26)]
        keys += [(c, "extra", code, cls) for code in range(25) for cls in ("zero", "mid", "max")]
        keys += [(c, "extra", 25, cls) for cls in ("0", "1", "0xFFFF")]
        keys += [(c, "starts in the last %d bytes" % t) for t in (16, 256)]
        keys += [(c, "invalid", k) for k in ("block_type", "block_count", "type_beyond")]
    keys += [("L", k) for k in ("switch on the first literal of a run", "switch inside a run", "count ended exactly with the run before",
                                "switch on the first literal behind a copy of at most 63 bytes",
                                "switch on the first literal behind a dictionary word", "block types of different context modes")]
    keys += [("L", "switch at output position mod 1024 =", r) for r in (0, 1, 1023)]
    keys += [("D", k) for k in ("switch on a command with literals", "switch on a copy-only command", "switch onto a one-symbol distance tree")]
    keys += [("D", "implicit distance while the count is", r) for r in (0, 1)]
    keys += [("I", k) for k in ("switch behind a short copy", "switch behind a copy of more than 64 bytes",
                                "switch behind a literal run that ended on a flush block")]
    keys += [("command", k) for k in ("insert 0", "insert 1 .. 4", "insert across literal blocks and a flush block", "implicit distance", "ring code",
                                      "explicit code with extra bits", "dictionary reference", "last copy cut off by MLEN")]
    keys += [("meta-block ends with all three counts at zero",)]
    keys += [("NTREESL", n, m) for n in (1, 2, 12, 13, 40, 100) for m in ("one mode", "modes 4")]
    keys += [("NTREESD", n) for n in (1, 4, 100)]
    return keys


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every case, built once.  Asserts the census complete: the condition under which the tests cover what they claim."""
    CENSUS.clear()
    rev, craft.rev = craft.rev, functools.lru_cache(maxsize=None)(craft.rev)
    try:
        cases = _small_cases() + _all_codes_cases() + [_top_bit_case(), _three_meta_blocks_case()] + _invalid_cases()
    finally:
        craft.rev = rev
    missing = [k for k in census_keys() if not CENSUS[k]]
    assert not missing, missing
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def census():
    all_cases()
    return dict(CENSUS)


def census_lines():
    """The census as text: the 26 count codes of a (category, role) and the extras of a (category, class) on one line each."""
    counted, rows = census(), collections.OrderedDict()
    for k in sorted(counted, key=str):
        if k[1:2] == ("count",):
            rows.setdefault("%s count as %s, codes 0 .. 25" % (k[0], k[2]), [0] * 26)[k[3]] = counted[k]
        elif k[1:2] == ("extra",) and k[2] < 25:
            rows.setdefault("%s extra %s, codes 0 .. 24" % (k[0], k[3]), [0] * 25)[k[2]] = counted[k]
        else:
            rows[" ".join(str(x) for x in k)] = counted[k]
    return ["%-70s %s" % (k, " ".join(map(str, v)) if isinstance(v, list) else v) for k, v in rows.items()]


TRUNCATED = ("small_mostly_L", "small_mostly_I", "small_mostly_D")


@functools.lru_cache(maxsize=None)
def truncations():
    """Those three cut at every byte: [(name, cut stream, the whole stream's output)]."""
    by_name = {c.name: c for c in all_cases()}
    return tuple((name, by_name[name].stream[:cut], by_name[name].out) for name in TRUNCATED for cut in range(len(by_name[name].stream)))
