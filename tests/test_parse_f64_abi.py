"""CPU-side checks of the f64 parse ABI (include/brx.h): brx_parse_f64_batch is declared and exported, its kernel is native code in
the library, the header compiles from plain C++, the argument checks that need no GPU answer in the order the contract gives, the
layers above the ABI expose the call, the two statements of THE PARSE, F64 in tests/parse_f64_oracle.py agree with the contract's check
values and with each other on a corpus that meets every status, the table of powers of five is what its generator and its definition
say, and the kernel's logic restated on the CPU (tools/parse_f64_emu.cpp around the real text of csrc/brx_parse_f64.h) holds against
the oracle without a load outside the arena or from a record above 64 bytes.  No GPU needed."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import brotli_rs_amd
import parse_f64_oracle as fo
import take_oracle
from brotli_rs_amd import brx
from brotli_rs_amd.brx import PARSE_HARD, PARSE_WORDS  # noqa: F401  (without the call nothing in this file has anything to check)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QT = 0x22


def _header():
    return open(os.path.join(ROOT, "include", "brx.h")).read()


def test_parse_f64_batch_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    cu64p = r"const\s+uint64_t\s*\*\s*"
    assert re.search(r"int\s+brx_parse_f64_batch\s*\(\s*brx_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*out\s*,\s*" + cu64p + r"out_off\s*,\s*" + cu64p
                     + r"len\s*,\s*uint32_t\s+n\s*,\s*uint64_t\s+span\s*,\s*" + cu64p + r"count\s*,\s*" + cu64p + r"pos_off\s*,\s*" + cu64p
                     + r"pos\s*,\s*uint64_t\s+n_pos\s*,\s*uint32_t\s+delim_len\s*,\s*uint32_t\s+flags\s*,\s*"
                     r"const\s+uint32_t\s*\*\s*sel_stream\s*,\s*" + cu64p + r"sel_rec\s*,\s*uint64_t\s+m\s*,\s*uint8_t\s+quote\s*,\s*"
                     r"double\s*\*\s*val\s*,\s*uint8_t\s*\*\s*status\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", hdr)
    assert hdr.index("int brx_parse_batch") < hdr.index("BRX_PARSE_WORDS") < hdr.index("int brx_parse_f64_batch")  # behind its prototype
    for name, v in (("BRX_PARSE_WORDS", fo.WORDS), ("BRX_PARSE_HARD", fo.HARD)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, v), hdr), name
    assert (brx.PARSE_WORDS, brx.PARSE_HARD) == (64, 6)
    path = brotli_rs_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    exported = set(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip())
    assert "brx_parse_f64_batch" in exported
    # (tests/test_abi.py reads the header's names by brx_[a-z_]+ and holds EXPORTED_SYMBOLS to exactly those: a name with a digit is
    # listed apart, and held to the header here)
    assert brx.EXPORTED_SYMBOLS_NUMBERED == sorted(set(re.findall(r"\b(brx_[a-z0-9_]+)\s*\(", hdr)) - set(brx.EXPORTED_SYMBOLS))
    assert brx.EXPORTED_SYMBOLS_NUMBERED == ["brx_parse_f64_batch"]
    assert brx.load_library().brx_parse_f64_batch is not None
    assert b"brx_parse_f64_kernel" in open(path, "rb").read()  # the pass is native code in the library


def test_header_compiles_from_plain_cpp():
    src = ('#include "include/brx.h"\n'
           "static_assert(BRX_PARSE_WORDS == 64u && BRX_PARSE_HARD == 6u && BRX_PARSE_LONG == 5u && BRX_PARSE_MAX_LEN == 64u, \"\");\n"
           "int (*f)(brx_ctx *, const uint8_t *, const uint64_t *, const uint64_t *, uint32_t, uint64_t, const uint64_t *, const uint64_t *,\n"
           "         const uint64_t *, uint64_t, uint32_t, uint32_t, const uint32_t *, const uint64_t *, uint64_t, uint8_t,\n"
           "         double *, uint8_t *, void *) = brx_parse_f64_batch;\n"
           "int main() { return f == nullptr; }\n")
    for std in ("c++11", "c++17"):
        r = subprocess.run(["g++", "-std=" + std, "-Wall", "-Werror", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_header_states_the_parse_and_its_check_values():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define[^\n]*\n\s*)*int\s+brx_parse_f64_batch", _header(), flags=re.S)
    assert m
    text = m.group(1)
    for word in ("DEVICE", "THE PARSE, F64", "BRX_PARSE_MAX_LEN", "0x20 and 0x09", "EMPTY", "[+-]? ( D+ ( '.' D* )? | '.' D+ ) ( [eE] [+-]? D+ )?",
                 "nan", "inf", "infinity", "0x7FF8000000000000", "0x7FF0000000000000", "ties to even", "ubnormal", "0x8000000000000000",
                 "HARD wins over RANGE", "19", "plus 1", "is ever loaded", "BRX_TAKE_NO_DELIM", "BRX_TAKE_TRIM_CR", "BRX_PARSE_WORDS",
                 "No scratch", "one launch", "in this order", "Not in scope", "hex float"):
        assert word in text, word
    flat = " ".join(text.split())
    for r, flags, bits, status in fo.CHECK:
        if len(r) > 40 or flags or r == b"nan":
            continue  # (spelled out in words below)
        assert '"%s" %016X / %s' % (r.decode(), bits, fo.NAMES[status]) in flat, r
    for word in ('(62 bytes) 40F86A0000000000 / OK', '(64 bytes) 40F86A0000000000 / OK', '(64 bytes) 3FF0000000000000 / OK', '(65 bytes) 0000000000000000 / LONG',
                 '"nan" without BRX_PARSE_WORDS 0000000000000000 / BAD', '"-Infinity" with BRX_PARSE_WORDS FFF0000000000000 / OK'):
        assert word in flat, word
    # the comment of brx_parse_batch keeps its words and points here
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define[^\n]*\n\s*)*int\s+brx_parse_batch", _header(), flags=re.S)
    for word in ("No exponent", "Not in scope", "floating point", "exponents", "brx_parse_f64_batch"):
        assert word in m.group(1), word


def _call(lib, h, flags=0, D=1, ss=None, sr=None, m=0, quote=0, val=None, status=None, out_off=None, ln=None, count=None, pos_off=None,
          pos=None, n_pos=0, n=0, span=0):
    return lib.brx_parse_f64_batch(h, None, out_off, ln, n, span, count, pos_off, pos, n_pos, D, flags, ss, sr, m, quote, val, status, None)


def _refuser():
    lib = brx.load_library()
    fake = ctypes.create_string_buffer(1 << 16)  # never read: the checks come first (the handle is no context: a call that got past
    h = ctypes.addressof(fake)                   # the checks would not come back with these messages)
    P = ctypes.addressof(ctypes.create_string_buffer(64))  # stands for any non-NULL device pointer: never dereferenced by the host

    def refused(word, *a, **kw):
        assert _call(lib, *a, **kw) == -1, word  # BRX_ERR_INVALID_ARGUMENT
        e = lib.brx_last_error()
        assert e.startswith(b"brx_parse_f64_batch:") and word in e, (word, e)

    return lib, h, P, refused, fake


# Each case violates its own check AND every later one it can, so that a check out of order shows.
def test_refusal_1_ctx_null():
    lib, h, P, refused, _ = _refuser()
    refused(b"ctx is NULL", None, flags=128, D=0, ss=P, m=1)


def test_refusal_2_unknown_flag_bits():
    lib, h, P, refused, _ = _refuser()
    for bad in (4, 8, 128, 1 << 31, 2 | 4, 64 | 256):
        refused(b"unknown flag bits", h, flags=bad, D=0, ss=P, m=1)


def test_refusal_3_trim_cr_without_no_delim():
    lib, h, P, refused, _ = _refuser()
    for flags in (2, 2 | 16 | 32 | 64):
        refused(b"BRX_TAKE_TRIM_CR without", h, flags=flags, D=0, ss=P, m=1)


def test_refusal_4_delim_len():
    lib, h, P, refused, _ = _refuser()
    for bad in (0, 17, 1 << 31):
        refused(b"delim_len", h, flags=3 | 48 | 64, D=bad, ss=P, m=1)


def test_refusal_5_half_a_selection():
    lib, h, P, refused, _ = _refuser()
    refused(b"sel_stream and sel_rec", h, ss=P, m=1)
    refused(b"sel_stream and sel_rec", h, sr=P, m=1)


def test_refusal_6_val_or_status_null():
    lib, h, P, refused, _ = _refuser()
    refused(b"val or status is NULL", h, m=5, n_pos=3)
    refused(b"val or status is NULL", h, m=5, n_pos=3, val=P)
    refused(b"val or status is NULL", h, m=5, n_pos=3, status=P, flags=64)
    refused(b"val or status is NULL", h, m=0, val=P)  # (in front of the m = 0 exit)


def test_7_an_empty_selection_succeeds_without_a_launch():
    lib, h, P, refused, _ = _refuser()
    assert _call(lib, h, val=P, status=P) == 0  # whatever else is NULL
    assert _call(lib, h, flags=3 | 48 | 64, D=16, ss=P, sr=P, quote=34, val=P, status=P, n_pos=3, span=1 << 63) == 0


def test_refusal_8_to_11_tables_and_ranges():
    lib, h, P, refused, _ = _refuser()
    tabs = dict(out_off=P, ln=P, count=P, pos_off=P)
    for missing in tabs:
        kw = dict(tabs)
        kw[missing] = None
        refused(b"NULL table", h, m=1, val=P, status=P, n_pos=3, span=1 << 63, **kw)
    refused(b"pos is NULL with n_pos > 0", h, m=1, val=P, status=P, n_pos=3, span=1 << 63, **tabs)
    refused(b"all-records mode with n = 0", h, m=1, val=P, status=P, span=1 << 63, **tabs)
    refused(b"span out of range", h, m=1 << 62, val=P, status=P, n=1, span=1 << 63, **tabs)
    refused(b"span out of range", h, m=1, val=P, status=P, ss=P, sr=P, span=1 << 63, **tabs)
    refused(b"m out of range", h, m=1 << 62, val=P, status=P, n=1, span=64, **tabs)


def test_parse_batch_still_refuses_the_words_flag():
    lib = brx.load_library()
    fake = ctypes.create_string_buffer(1 << 16)
    assert lib.brx_parse_batch(ctypes.addressof(fake), None, None, None, 0, 0, None, None, None, 0, 1, 64, None, None, 0, 0, 0, 0, None, None,
                               None) == -1
    assert b"brx_parse_batch: unknown flag bits" in lib.brx_last_error()


def test_wrappers_expose_the_call():
    assert callable(brx.Context.parse_f64_batch) and callable(brx.Context.parse_f64_batch_device)
    sig = inspect.signature(brx.Context.parse_f64_batch)
    assert list(sig.parameters)[1:] == ["out", "out_off", "out_len", "count", "pos_off", "pos", "sel_stream", "sel_rec", "delim_len", "keep_delim",
                                        "trim_cr", "spaces", "quote", "words", "finish", "stream"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["sel_stream"], d["sel_rec"], d["delim_len"], d["keep_delim"], d["trim_cr"], d["spaces"], d["quote"], d["words"], d["finish"],
            d["stream"]) == (None, None, 1, False, False, False, None, False, False, None)
    doc = brx.Context.parse_f64_batch.__doc__
    for word in ("torch.float64", "PARSE_HARD", "finish=True", "only when some entry is PARSE_HARD", "float()", "index_set_batch"):
        assert word in doc, word
    src = ('#include "brotli-rs_amd/host/decompressor.hpp"\n'
           "int main() { uint64_t t[4]; uint32_t s[1]; double v[2]; uint8_t st[2];\n"
           "             brotli::parse_f64_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, 1, 1, BRX_TAKE_NO_DELIM | BRX_TAKE_TRIM_CR | BRX_PARSE_SPACES |\n"
           "                                     BRX_PARSE_QUOTED | BRX_PARSE_WORDS, s, t, 1, '\"', v, st);\n"
           "             brotli::parse_f64_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, 1, 2, 0, nullptr, nullptr, 2, 0, v, st, nullptr);\n"
           "             return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_check_values_of_the_contract_in_both_forms():
    assert len(fo.CHECK) == 40
    for r, flags, bits, status in fo.CHECK:
        for name, f in fo.FORMS.items():
            assert f(r, bool(flags & fo.SPACES), QT if flags & fo.QUOTED else None, bool(flags & fo.WORDS)) == (bits, status), (name, r)
    assert [len(fo.CHECK[i][0]) for i in (27, 28, 29, 30)] == [62, 64, 64, 65]
    # the check values that float() decides are float()'s
    for r, flags, bits, status in fo.CHECK:
        if status in (fo.OK, fo.RANGE) and not flags:
            assert fo.bits_of(float(r.decode())) == bits, r
    assert fo.exact_bits(b"9007199254740993.0000000000000001") == 0x4340000000000001  # what HARD leaves open: val + 1 here


@pytest.fixture(scope="module")
def corpus():
    """Fixed seed: random digit strings of 1 .. 45 significant digits with exponents -345 .. 312, garbage, corners and words, and for
    every q in -342 .. 308 the near-midpoint texts at 17 .. 45 digits."""
    rng = np.random.default_rng(20)
    return [fo.random_field(rng, QT) for _ in range(5000)] + fo.midpoint_records(rng, range(-342, 309))


def test_the_two_forms_agree_on_the_corpus(corpus):
    seen = {s: 0 for s in fo.NAMES}
    mid_hard = 0
    for it, r in enumerate(corpus + [b"0" * 65, b"1" * 66]):
        for spaces in (False, True):
            for quote in (None, QT):
                for words in (False, True):
                    a, b = fo.parse_re(r, spaces, quote, words), fo.parse_fsm(r, spaces, quote, words)
                    assert a == b, (r, spaces, quote, words, a, b)
                    assert a[1] in (fo.OK, fo.RANGE, fo.HARD) or a[0] == 0, (r, a)
                    if a[1] == fo.HARD:  # the correctly rounded pattern is val or val + 1
                        t = r.strip(b" \t") if spaces else r
                        t = t[1:-1] if quote is not None and len(t) >= 2 and t[0] == quote and t[-1] == quote else t
                        assert fo.exact_bits(t) - a[0] in (0, 1) and fo.bits_of(float(t.decode())) == fo.exact_bits(t), r
                    seen[a[1]] += 1
        mid_hard += it >= 5000 and fo.parse_re(r)[1] == fo.HARD
    assert all(v >= 100 for v in seen.values()), seen  # every status was met, HARD at least 100 times
    assert mid_hard >= 100, mid_hard


def test_the_table_is_what_its_generator_and_its_definition_say():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_pow5
    finally:
        sys.path.pop(0)
    committed = open(os.path.join(ROOT, "brotli-rs_amd", "csrc", "brx_pow5.h")).read()
    assert gen_pow5.text() == committed  # byte for byte
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_pow5.py"), "--stdout"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == committed
    rows = re.findall(r"\{0x([0-9A-F]{16})ull, 0x([0-9A-F]{16})ull\}, // (-?\d+)", committed)
    assert [int(q) for _, _, q in rows] == list(range(-342, 309))
    for hi, lo, q in rows:  # every entry equals its definition, restated here on Python integers
        q, c = int(q), (int(hi, 16) << 64) | int(lo, 16)
        assert c >> 127 == 1
        if q >= 0:
            p = 5 ** q
            assert c == (p << (128 - p.bit_length()) if p.bit_length() <= 128 else p >> (p.bit_length() - 128)), q
        else:
            p = 5 ** -q
            z = (p - 1).bit_length()  # the least z with 2^z >= p
            full = (1 << (z + 127)) // p + 1 if q >= -27 else (1 << (2 * z + 128)) // p + 1
            assert c == full >> max(full.bit_length() - 128, 0) and full.bit_length() >= 128, q


# ---- the emulator: the corpus placed as records of whole calls ---------------------------------------------------------------------
MAGIC = 0x3436465F58524221
TAKE_FLAGS = (0, 1, 3)        # the three BRX_TAKE flag combinations
PARSE_FLAGS = (0, 16, 32, 48, 64, 80, 96, 112)


def _write_call(f, phase, arena, off, ln, count, pos_off, pos, n_pos, D, flags, quote, sel, m):
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    if sel is None:
        si = sk = None
    else:
        si, sk = np.asarray(sel[0], dtype=np.int64), np.asarray(sel[1], dtype=np.int64)
        m = len(si)
    src, L = take_oracle.take_vec(arena, off, ln, count, pos_off, pos, n_pos, D, flags & 3, si, sk, m)
    bits, status = fo.parse_records("re", arena, src, L, bool(flags & fo.SPACES), quote if flags & fo.QUOTED else None, bool(flags & fo.WORDS))
    u = lambda a: np.asarray(a, dtype=np.int64).astype(np.uint64)
    np.array([MAGIC, phase, len(arena), len(ln), len(pos), n_pos, D, flags, quote, sel is not None, m], dtype=np.uint64).tofile(f)
    padded = np.zeros((len(arena) + 7) // 8 * 8, dtype=np.uint8)
    padded[:len(arena)] = arena
    padded.tofile(f)
    for a in (off, ln, count, pos_off, pos):
        u(a).tofile(f)
    if sel is not None:
        u(si).tofile(f)
        u(sk).tofile(f)
    want = np.stack([u(src), u(L), bits.astype(np.uint64), status.astype(np.uint64)], axis=1)
    want.tofile(f)
    return status, L


def _exact(rng, pool, L):
    """a record of exactly L bytes: a corpus number with zeros or blanks in front (mostly a number still), or L bytes of one"""
    fit = pool[min(L, 64)]
    if L == 0 or not fit:
        return b" " * L
    r = fit[int(rng.integers(0, len(fit)))]
    return (b"0", b"0", b" ")[int(rng.integers(0, 3))] * (L - len(r)) + r


def _streams(rng, records, D, cr):
    """One stream of the records, each followed by D line feeds (so the trailing record is empty), and its positions."""
    s, pos = b"", []
    for r in records:
        s += r + (b"\r" if cr and rng.integers(0, 4) == 0 else b"")
        pos.append(len(s))
        s += b"\n" * D
    return s, pos


def test_the_header_logic_holds_against_the_oracle(tmp_path, corpus):
    """tools/parse_f64_emu.cpp: brx_parse_f64_lane lane by lane on the CPU around the real text of csrc/brx_parse_f64.h, csrc/brx_parse.h
    and csrc/brx_take.h, over the corpus placed as records: every length 0 .. 66 at all 16 source phases, records on the arena's first
    and last byte, arenas of 1 .. 40 bytes, both selection modes, the three BRX_TAKE flag combinations, delim_len 1, 2 and 16, stale
    positions.  It fails on the first difference from the oracle, on any load outside [out, out + span) and on a record byte loaded
    for an entry above 64 bytes."""
    rng = np.random.default_rng(21)
    numbers = [r for r in corpus if r[:1].isdigit() and b" " not in r and b'"' not in r and b"\t" not in r and b"\r" not in r]
    pool = {L: [r for r in numbers if len(r) <= L and len(r) >= L - 30] for L in range(65)}
    path = str(tmp_path / "calls.bin")
    seen, lens, calls = set(), set(), 0
    with open(path, "wb") as f:
        # PART 1: one stream that is the whole arena, records of every length 0 .. 67 in order, the arena at each phase: the first
        # record starts on the arena's first byte; without a trailing delimiter the last one ends on its last
        for it in range(96):
            recs = [_exact(rng, pool, L) for L in range(68)]
            s, pos = _streams(rng, recs, 1, False)
            s, pos = s[:-1], pos[:-1]  # the 67-byte record is the stream's last, up to the arena's last byte
            flags = TAKE_FLAGS[(it // 16) % 3] | PARSE_FLAGS[it % 8]
            sel = ([0] * 68, list(range(67, -1, -1))) if it % 2 else None
            st, L = _write_call(f, it % 16, np.frombuffer(s, dtype=np.uint8), [0], [len(s)], [len(pos)], [0], pos, len(pos), 1, flags, QT, sel, 68)
            seen.update(st.tolist())
            calls += 1
        # PART 2: the corpus as the lines of streams in slots with slack, D in {1, 2, 16}, CRs, stale positions
        order = rng.permutation(len(corpus))
        at, it = 0, 0
        while at < len(order):
            D, tf = (1, 2, 16)[it % 3], TAKE_FLAGS[(it // 3) % 3]
            pairs, stale = (it // 9) % 2 == 1, (it // 18) % 4 == 3
            flags = tf | PARSE_FLAGS[int(rng.integers(0, 8))]
            n = int(rng.integers(1, 5))
            arena, off, ln, count, pos_off, pos = b"", [], [], [], [], []
            for i in range(n):
                k = int(rng.integers(0, 40))
                s, p = _streams(rng, [corpus[j] for j in order[at:at + k]], D, tf == 3)
                at += k
                if rng.integers(0, 2) and p:
                    s, p = s[:-D], p[:-1]  # no trailing delimiter: the last record ends the stream
                off.append(len(arena)); ln.append(len(s)); count.append(len(p)); pos_off.append(len(pos))
                pos += p
                arena += s + (b"\r7"[int(rng.integers(0, 2)):][:1] * int(rng.integers(0, 20)) if i + 1 < n else b"")
            if not arena:
                arena = b"7"
            n_pos = len(pos)
            if stale:
                pos = [int(rng.integers(0, 1000)) if rng.integers(0, 4) == 0 else p for p in pos]
                n_pos = int(rng.integers(0, len(pos) + 1)) if rng.integers(0, 2) else n_pos
                count = [c + int(rng.integers(0, 3)) for c in count]
            m = sum(count) + n + (int(rng.integers(0, 4)) if stale else 0)
            sel = None
            if pairs:
                si = rng.integers(0, n, 60)
                sk = np.array([int(rng.integers(0, count[i] + 1)) for i in si])
                wild = rng.integers(0, 25, 60) == 0
                si, sk = np.where(wild, si + n, si), np.where(np.roll(wild, 1), sk + np.array(count)[si % n] + 1, sk)
                sel = (si, sk)
            st, L = _write_call(f, int(rng.integers(0, 16)), np.frombuffer(arena, dtype=np.uint8), off, ln, count, pos_off, pos, n_pos, D, flags, QT,
                                sel, m)
            seen.update(st.tolist())
            calls += 1
            it += 1
        # PART 3: arenas of 1 .. 40 bytes that are one record (the byte-by-byte fetch), at every phase, and as two records
        for size in range(1, 41):
            for rep in range(4):
                r = _exact(rng, pool, size)
                a = np.frombuffer(r, dtype=np.uint8)
                st, L = _write_call(f, (size * 4 + rep * 5) % 16, a, [0], [size], [0], [0], [], 0, 1, TAKE_FLAGS[rep % 3] | PARSE_FLAGS[rep], QT,
                                    ([0], [0]) if rep == 3 else None, 1)
                assert L.tolist() == [size]
                seen.update(st.tolist())
                calls += 1
            if size >= 3:
                cut = int(rng.integers(0, size - 1))
                r = bytearray(_exact(rng, pool, size))
                r[cut] = 0x0A
                st, L = _write_call(f, size % 16, np.frombuffer(bytes(r), dtype=np.uint8), [0], [size], [1], [0], [cut], 1, 1, 1, QT, None, 2)
                assert L.tolist() == [cut, size - cut - 1]
                calls += 1
    assert seen == set(fo.NAMES), seen
    exe = str(tmp_path / "parse_f64_emu")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "brotli-rs_amd", "csrc"),
                        os.path.join(ROOT, "tools", "parse_f64_emu.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "--full", path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK: %d calls (" % calls) \
        and int(re.search(r"\((\d+) in arenas of at most 40 bytes\)", r.stdout).group(1)) >= 198 \
        and " 0 (length, phase) pairs not met" in r.stdout \
        and "none outside the arena, none from a record above 64 bytes" in r.stdout, r.stdout[-2000:]
