"""CPU-side checks of the set index ABI (include/brx.h): brx_index_set_batch is declared and exported, its kernels are native code in
the library, the argument checks that need no GPU answer in the order the contract gives, the layers above the ABI expose the call,
the two statements of the rule in tests/set_oracle.py agree with each other and with tests/escaped_oracle.py, and the row body of the
kernels restated on the CPU (tools/index_set_emu.cpp) holds against the serial rule.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np

import brotli_rs_amd
import escaped_oracle
import set_oracle
from brotli_rs_amd import brx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_QUOTE, NO_ESCAPE = 1, 2  # BRX_INDEX_NO_QUOTE, BRX_INDEX_NO_ESCAPE


def _header():
    return open(os.path.join(ROOT, "include", "brx.h")).read()


def test_index_set_batch_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+BRX_INDEX_NO_ESCAPE\s+2u\b", hdr)
    assert re.search(r"#define\s+BRX_INDEX_SET_MAX\s+8u\b", hdr)
    assert re.search(r"int\s+brx_index_set_batch\s*\(\s*brx_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*delims\s*,\s*uint32_t\s+n_delims\s*,\s*"
                     r"uint8_t\s+quote\s*,\s*uint8_t\s+escape\s*,\s*uint32_t\s+flags\s*,\s*"
                     r"const\s+uint8_t\s*\*\s*out\s*,\s*const\s+uint64_t\s*\*\s*out_off\s*,\s*const\s+uint64_t\s*\*\s*len\s*,\s*"
                     r"uint32_t\s+n\s*,\s*uint64_t\s+span\s*,\s*uint64_t\s*\*\s*count\s*,\s*uint32_t\s*\*\s*open\s*,\s*"
                     r"const\s+uint64_t\s*\*\s*pos_off\s*,\s*uint64_t\s*\*\s*pos\s*,\s*uint8_t\s*\*\s*what\s*,\s*uint64_t\s+total\s*,\s*"
                     r"void\s*\*\s*hip_stream\s*\)\s*;", hdr)
    path = brotli_rs_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    exported = set(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip())
    assert "brx_index_set_batch" in exported
    assert "brx_index_set_batch" in brx.EXPORTED_SYMBOLS
    assert brx.load_library().brx_index_set_batch is not None
    blob = open(path, "rb").read()
    for kernel in (b"brx_index_set_count_kernel", b"brx_index_set_fill_kernel", b"brx_index_escaped_resolve_kernel"):
        assert kernel in blob  # the pass is native code in the library; resolve is the escaped pass's


def test_header_states_the_rule_and_its_limits():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+BRX_INDEX_NO_ESCAPE\s+2u[^\n]*\n#define\s+BRX_INDEX_SET_MAX\s+8u\s*int\s+brx_index_set_batch",
                  _header(), flags=re.S)
    assert m
    text = m.group(1)
    for word in ("8", "what", "BRX_INDEX_NO_ESCAPE", "more than one byte", "HOST", "not its index"):
        assert word in text, word
    # the escaped pass no longer calls several delimiters simply out of scope: it points here
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+BRX_INDEX_NO_QUOTE\s+1u\s*int\s+brx_index_escaped_batch", _header(), flags=re.S)
    assert m and "brx_index_set_batch" in m.group(1)
    assert not re.search(r"CR handling;\s*several delimiters in one call\.", m.group(1))


def _call(lib, h, delims, nd, quote, escape, flags, count=None, pos_off=None, pos=None, what=None):
    return lib.brx_index_set_batch(h, delims, nd, quote, escape, flags, None, None, None, 0, 0, count, None, pos_off, pos, what, 0, None)


def test_argument_checks_that_need_no_gpu():
    """The whole order of the contract by message, before anything touches HIP (the handle below is no context: a call that got past
    the checks to HIP would not come back with these messages).  n = 0 comes behind them all, so every call here has n = 0."""
    lib = brx.load_library()
    inval = -1  # BRX_ERR_INVALID_ARGUMENT

    def err():
        e = lib.brx_last_error()
        assert b"brx_index_set_batch" in e
        return e

    assert _call(lib, None, b",\n", 2, 34, 92, 0) == inval and b"ctx is NULL" in err()
    assert _call(lib, None, None, 0, 10, 10, 4) == inval and b"ctx is NULL" in err()  # (1 before everything)
    fake = ctypes.create_string_buffer(1 << 16)  # never read: the checks come first
    h = ctypes.addressof(fake)
    c = ctypes.addressof(ctypes.create_string_buffer(64))
    # 2: unknown flag bits, before the set is looked at
    assert _call(lib, h, b",\n", 2, 34, 92, 4, c) == inval and b"flag" in err()
    assert _call(lib, h, b",\n", 2, 34, 92, 0x80000000, c) == inval and b"flag" in err()
    assert _call(lib, h, None, 0, 34, 92, 8, c) == inval and b"flag" in err()
    # 3: delims NULL, before its count
    assert _call(lib, h, None, 0, 34, 92, 0, c) == inval and b"delims" in err() and b"NULL" in err()
    assert _call(lib, h, None, 9, 34, 92, 3, c) == inval and b"NULL" in err()
    # 4: n_delims 0 or above 8, before the bytes are compared (the nine bytes below hold a value twice and the escape)
    assert _call(lib, h, b",\n", 0, 34, 92, 0, c) == inval and b"delims" in err() and b"1 .. 8" in err()
    assert _call(lib, h, b",,\\345678", 9, 34, 92, 0, c) == inval and b"1 .. 8" in err()
    # 5: a value twice, before escape and quote are compared
    assert _call(lib, h, b",\n,", 3, 34, 92, 0, c) == inval and b"delims" in err() and b"twice" in err()
    assert _call(lib, h, b"\\\"\\", 3, 34, 92, 0, c) == inval and b"twice" in err()
    assert _call(lib, h, b"\x00\x01\x02\x03\x04\x05\x06\x00", 8, 34, 92, 3, c) == inval and b"twice" in err()
    # 6: a delimiter equal to the escape, refused without NO_ESCAPE (before the quote) and accepted with it
    assert _call(lib, h, b",\\", 2, 34, 92, 0, c) == inval and b"escape" in err() and b"quote" not in err()
    assert _call(lib, h, b"\"\\", 2, 34, 92, 0, c) == inval and b"escape" in err() and b"quote" not in err()
    assert _call(lib, h, b",\\", 2, 34, 92, NO_QUOTE, c) == inval and b"escape" in err()
    assert _call(lib, h, b",\\", 2, 34, 92, NO_ESCAPE, c) == 0
    assert _call(lib, h, b",\\", 2, 34, 92, NO_ESCAPE | NO_QUOTE, c) == 0
    # 7: the quote in the set, refused without NO_QUOTE and accepted with it
    assert _call(lib, h, b",\"", 2, 34, 92, 0, c) == inval and b"quote" in err() and b"escape" not in err()
    assert _call(lib, h, b",\"", 2, 34, 92, NO_ESCAPE, c) == inval and b"quote" in err()
    assert _call(lib, h, b",\"", 2, 34, 92, NO_QUOTE, c) == 0
    assert _call(lib, h, b",\"", 2, 34, 92, NO_QUOTE | NO_ESCAPE, c) == 0
    # 8: quote == escape, with neither flag only
    assert _call(lib, h, b",\n", 2, 92, 92, 0, c) == inval and b"quote" in err() and b"escape" in err()
    assert _call(lib, h, b",\n", 2, 92, 92, 0, None, c, None) == inval and b"escape" in err()  # (the bytes before pos_off / pos)
    assert _call(lib, h, b",\n", 2, 92, 92, NO_QUOTE, c) == 0
    assert _call(lib, h, b",\n", 2, 7, 7, NO_ESCAPE, c) == 0
    assert _call(lib, h, b",\n", 2, 44, 10, NO_QUOTE | NO_ESCAPE, c) == 0  # (both ignored: they may even be delimiters)
    # 9: only one of pos_off / pos, before `what` is looked at
    assert _call(lib, h, b",\n", 2, 34, 92, 0, c, c, None) == inval and b"pos_off" in err()
    assert _call(lib, h, b",\n", 2, 34, 92, 0, c, None, c) == inval and b"pos_off" in err()
    assert _call(lib, h, b",\n", 2, 34, 92, 0, c, c, None, c) == inval and b"pos_off" in err()
    # 10: what without pos, before count
    assert _call(lib, h, b",\n", 2, 34, 92, 0, c, None, None, c) == inval and b"what" in err()
    assert _call(lib, h, b",\n", 2, 34, 92, 0, None, None, None, c) == inval and b"what" in err()
    # 11: count NULL in count mode
    assert _call(lib, h, b",\n", 2, 34, 92, 0, None) == inval and b"count" in err()
    # then n = 0: success, in count mode and in fill mode with and without what and count
    assert _call(lib, h, b",\n", 2, 34, 92, 0, c) == 0
    assert _call(lib, h, b"{}[]:,\n", 7, 34, 92, 0, c, c, c, c) == 0
    assert _call(lib, h, b"\x00\x7f\x80\xff\x01\x02\x05\x06", 8, 3, 4, 0, None, c, c, None) == 0
    # brx_index_escaped_batch keeps refusing bit 1
    assert lib.brx_index_escaped_batch(h, 10, 34, 92, NO_ESCAPE, None, None, None, 0, 0, c, None, None, None, 0, None) == inval
    assert b"brx_index_escaped_batch" in lib.brx_last_error() and b"flag" in lib.brx_last_error()


def test_wrappers_expose_the_call():
    assert callable(brx.Context.index_set_batch) and callable(brx.Context.index_set_batch_device)
    assert brx.INDEX_NO_QUOTE == NO_QUOTE and brx.INDEX_NO_ESCAPE == NO_ESCAPE
    src = ('#include "brotli-rs_amd/host/decompressor.hpp"\n'
           "int main() { uint64_t c[1], p[1]; uint32_t o[1]; uint8_t w[1]; const uint8_t d[8] = {',', '\\n', '{', '}', '[', ']', ':', 0};\n"
           "             brotli::index_set_batch(nullptr, d, 2, '\"', '\\\\', 0, nullptr, nullptr, nullptr, 0, 0, c);\n"
           "             brotli::index_set_batch(nullptr, d, 8, 0, 0, BRX_INDEX_NO_QUOTE | BRX_INDEX_NO_ESCAPE, nullptr, nullptr, nullptr, 0, 0, c, o);\n"
           "             brotli::index_set_batch(nullptr, d, BRX_INDEX_SET_MAX, 255, 128, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, c, p, w, 1, nullptr);\n"
           "             return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


FLAGS = ((False, False), (True, False), (False, True), (True, True))  # (no_quote, no_escape)


def test_the_two_statements_of_the_rule_agree():
    """vec == serial on 2 000 random strings of 0 .. 60 bytes over {D1, D2, Q, E, x}, a third of them E-heavy, under all four flag
    combinations; and the check values of the contract by both."""
    rng = np.random.default_rng(16)
    D, Q, E = b",\n", 0x22, 0x5C
    alphabet = np.array([D[0], D[1], Q, E, 0x78], dtype=np.uint8)
    for k in range(2000):
        ln = int(rng.integers(0, 61))
        p = [0.05, 0.05, 0.05, 0.8, 0.05] if k % 3 == 0 else [0.2] * 5
        s = alphabet[rng.choice(5, ln, p=p)]
        for nq, ne in FLAGS:
            want = set_oracle.serial(s, D, Q, E, nq, ne)
            got = set_oracle.vec(s, D, Q, E, nq, ne)
            assert got[2] == want[2] and got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist(), (bytes(s), nq, ne)
            assert got[1].tolist() == s[got[0]].tolist()
            st = set_oracle.states(s, Q, E, nq, ne)
            assert st.size == ln + 1 and st[0] == 0 and st[-1] == want[2]
            assert not (nq and want[2] & 1) and not (ne and want[2] & 2)
    assert len(set_oracle.J) == 48 and len(set_oracle.C) == 25
    for rule in (set_oracle.serial, set_oracle.vec):
        pos, what, open_ = rule(np.frombuffer(set_oracle.J, dtype=np.uint8), set_oracle.J_SET, Q, E)
        assert pos.tolist() == set_oracle.J_POS and bytes(what) == set_oracle.J_WHAT and open_ == 3
        pos, what, open_ = rule(np.frombuffer(set_oracle.C, dtype=np.uint8), set_oracle.C_SET, Q, E, False, True)
        assert pos.tolist() == set_oracle.C_POS_NO_ESCAPE and bytes(what) == set_oracle.C_WHAT_NO_ESCAPE and open_ == 1
        pos, what, open_ = rule(np.frombuffer(set_oracle.C, dtype=np.uint8), set_oracle.C_SET, Q, E, True, True)
        assert pos.tolist() == set_oracle.C_POS_PLAIN and open_ == 0 and bytes(what) == bytes(set_oracle.C[j] for j in pos)


def test_the_rule_agrees_with_the_escaped_oracle():
    """For a set of two, pos is the sorted merge of escaped_oracle.vec for each delimiter alone and open is equal; for one delimiter
    pos equals escaped_oracle.vec.  With and without quotes (the escaped rule has no NO_ESCAPE)."""
    rng = np.random.default_rng(17)
    D1, D2, Q, E = 0x0A, 0x2C, 0x22, 0x5C
    alphabet = np.array([D1, D2, Q, E, 0x78], dtype=np.uint8)
    for k in range(600):
        ln = int(rng.integers(0, 200))
        p = [0.05, 0.05, 0.05, 0.8, 0.05] if k % 3 == 0 else [0.2] * 5
        s = alphabet[rng.choice(5, ln, p=p)]
        for nq in (False, True):
            p1, o1 = escaped_oracle.vec(s, D1, Q, E, nq)
            p2, o2 = escaped_oracle.vec(s, D2, Q, E, nq)
            pos, what, open_ = set_oracle.vec(s, bytes([D1, D2]), Q, E, nq)
            assert o1 == o2 == open_
            assert pos.tolist() == sorted(p1.tolist() + p2.tolist())
            assert pos[what == D1].tolist() == p1.tolist() and pos[what == D2].tolist() == p2.tolist()
            pos, what, open_ = set_oracle.vec(s, bytes([D1]), Q, E, nq)
            assert pos.tolist() == p1.tolist() and open_ == o1 and (what == D1).all()


def test_the_row_body_holds_against_a_serial_walk(tmp_path):
    """tools/index_set_emu.cpp: the pass lane by lane on the CPU around the real arithmetic of csrc/brx_index_escaped.h -- the union
    mask, the `lead` class "a byte of the set", the filler and `what`, under all four flag combinations, on 480 random batches."""
    exe = str(tmp_path / "is_emu")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "brotli-rs_amd", "csrc"),
                        os.path.join(ROOT, "tools", "index_set_emu.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all ok" in r.stdout, r.stdout[-2000:]
