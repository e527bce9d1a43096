"""CPU-side checks of the escaped index ABI (include/brx.h): brx_index_escaped_batch is declared and exported, its kernels are native
code in the library, the argument checks that need no GPU answer in the order the contract gives, the layers above the ABI expose the
call, the two statements of the rule in tests/escaped_oracle.py agree, and the arithmetic on the tiles' state maps that the kernels
use (csrc/brx_index_escaped.h) holds against a serial walk on the CPU.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np

import brotli_rs_amd
import escaped_oracle
from brotli_rs_amd import brx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_QUOTE = 1  # BRX_INDEX_NO_QUOTE


def _header():
    return open(os.path.join(ROOT, "include", "brx.h")).read()


def test_index_escaped_batch_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+BRX_INDEX_NO_QUOTE\s+1u\b", hdr)
    assert re.search(r"int\s+brx_index_escaped_batch\s*\(\s*brx_ctx\s*\*\s*ctx\s*,\s*uint8_t\s+delim\s*,\s*uint8_t\s+quote\s*,\s*"
                     r"uint8_t\s+escape\s*,\s*uint32_t\s+flags\s*,\s*"
                     r"const\s+uint8_t\s*\*\s*out\s*,\s*const\s+uint64_t\s*\*\s*out_off\s*,\s*const\s+uint64_t\s*\*\s*len\s*,\s*"
                     r"uint32_t\s+n\s*,\s*uint64_t\s+span\s*,\s*uint64_t\s*\*\s*count\s*,\s*uint32_t\s*\*\s*open\s*,\s*"
                     r"const\s+uint64_t\s*\*\s*pos_off\s*,\s*uint64_t\s*\*\s*pos\s*,\s*uint64_t\s+total\s*,\s*"
                     r"void\s*\*\s*hip_stream\s*\)\s*;", hdr)
    path = brotli_rs_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    exported = set(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip())
    assert "brx_index_escaped_batch" in exported
    assert "brx_index_escaped_batch" in brx.EXPORTED_SYMBOLS
    assert brx.load_library().brx_index_escaped_batch is not None
    blob = open(path, "rb").read()
    for kernel in (b"brx_index_escaped_count_kernel", b"brx_index_escaped_resolve_kernel", b"brx_index_escaped_fill_kernel"):
        assert kernel in blob  # the pass is native code in the library, next to the other index passes


def test_header_states_the_rule_and_its_limits():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define\s+BRX_INDEX_NO_QUOTE\s+1u\s*)?int\s+brx_index_escaped_batch", _header(), flags=re.S)
    assert m
    text = m.group(1)
    for word in ("odd", "open[i]", "BRX_INDEX_NO_QUOTE", "more than one byte", "delim == escape"):
        assert word in text, word
    # the quoted pass no longer says that nothing handles escapes: it points here (and keeps the word its own test asks for)
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+brx_index_quoted_batch", _header(), flags=re.S)
    assert m and "escape" in m.group(1) and "brx_index_escaped_batch" in m.group(1)


def _call(lib, h, delim, quote, escape, flags, count=None, pos_off=None, pos=None):
    return lib.brx_index_escaped_batch(h, delim, quote, escape, flags, None, None, None, 0, 0, count, None, pos_off, pos, 0, None)


def test_argument_checks_that_need_no_gpu():
    """A NULL context, unknown flag bits and clashing bytes are refused before anything touches HIP, in the contract's order (the
    handle below is no context: a call that got past the checks to HIP would not come back with these messages).  n = 0 comes behind
    them all, so every call here has n = 0."""
    lib = brx.load_library()
    inval = -1  # BRX_ERR_INVALID_ARGUMENT
    assert _call(lib, None, 10, 34, 92, 0) == inval
    assert b"brx_index_escaped_batch" in lib.brx_last_error() and b"ctx is NULL" in lib.brx_last_error()
    assert _call(lib, None, 10, 10, 10, 2) == inval and b"ctx is NULL" in lib.brx_last_error()  # (first in the order)
    fake = ctypes.create_string_buffer(1 << 16)  # never read: the checks come first
    h = ctypes.addressof(fake)
    c = ctypes.addressof(ctypes.create_string_buffer(64))
    assert _call(lib, h, 10, 34, 92, 2, c) == inval
    assert b"brx_index_escaped_batch" in lib.brx_last_error() and b"flag" in lib.brx_last_error()
    assert _call(lib, h, 10, 34, 92, 0x80000000, c) == inval and b"flag" in lib.brx_last_error()
    assert _call(lib, h, 92, 92, 92, 3, c) == inval and b"flag" in lib.brx_last_error()  # (flags before the bytes)
    assert _call(lib, h, 92, 34, 92, 0, c) == inval
    assert b"brx_index_escaped_batch" in lib.brx_last_error() and b"escape" in lib.brx_last_error()
    assert _call(lib, h, 92, 34, 92, NO_QUOTE, c) == inval and b"escape" in lib.brx_last_error()
    assert _call(lib, h, 10, 92, 92, 0, c) == inval
    assert b"brx_index_escaped_batch" in lib.brx_last_error() and b"quote" in lib.brx_last_error() and b"escape" in lib.brx_last_error()
    assert _call(lib, h, 10, 10, 92, 0, c) == inval
    assert b"brx_index_escaped_batch" in lib.brx_last_error() and b"quote" in lib.brx_last_error()
    assert _call(lib, h, 10, 10, 92, 0, None, c, None) == inval and b"quote" in lib.brx_last_error()  # (the bytes before pos_off / pos)
    assert _call(lib, h, 10, 34, 92, 0, c, c, None) == inval and b"pos_off" in lib.brx_last_error()
    assert _call(lib, h, 10, 34, 92, 0, c, None, c) == inval and b"pos_off" in lib.brx_last_error()
    assert _call(lib, h, 10, 34, 92, 0, None) == inval and b"count" in lib.brx_last_error()
    # under BRX_INDEX_NO_QUOTE the quote argument is ignored: equal to the delimiter or to the escape it is NOT refused (n = 0: success)
    assert _call(lib, h, 10, 10, 92, NO_QUOTE, c) == 0
    assert _call(lib, h, 10, 92, 92, NO_QUOTE, c) == 0
    assert _call(lib, h, 10, 34, 92, 0, c) == 0


def test_wrappers_expose_the_call():
    assert callable(brx.Context.index_escaped_batch) and callable(brx.Context.index_escaped_batch_device)
    assert brx.INDEX_NO_QUOTE == NO_QUOTE
    src = ('#include "brotli-rs_amd/host/decompressor.hpp"\n'
           "int main() { uint64_t c[1], p[1]; uint32_t o[1];\n"
           "             brotli::index_escaped_batch(nullptr, '\\n', '\"', '\\\\', 0, nullptr, nullptr, nullptr, 0, 0, c);\n"
           "             brotli::index_escaped_batch(nullptr, '\\t', 0, '\\\\', BRX_INDEX_NO_QUOTE, nullptr, nullptr, nullptr, 0, 0, c, o);\n"
           "             brotli::index_escaped_batch(nullptr, 0, 255, 128, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, c, p, 1, nullptr);\n"
           "             return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_two_statements_of_the_rule_agree():
    """vec == serial on 2 000 random strings of 0 .. 60 bytes over {D, Q, E, x}, a third of them E-heavy, with and without no_quote;
    and the check values of the contract by the serial rule."""
    rng = np.random.default_rng(14)
    D, Q, E = 0x0A, 0x22, 0x5C
    alphabet = np.array([D, Q, E, 0x78], dtype=np.uint8)
    for k in range(2000):
        ln = int(rng.integers(0, 61))
        p = [0.2 / 3, 0.2 / 3, 0.8, 0.2 / 3] if k % 3 == 0 else [0.25] * 4
        s = alphabet[rng.choice(4, ln, p=p)]
        for no_quote in (False, True):
            want_pos, want_open = escaped_oracle.serial(s, D, Q, E, no_quote)
            got_pos, got_open = escaped_oracle.vec(s, D, Q, E, no_quote)
            assert got_open == want_open and got_pos.tolist() == want_pos.tolist(), (bytes(s), no_quote)
            st = escaped_oracle.states(s, D, Q, E, no_quote)
            assert st.size == ln + 1 and st[0] == 0 and st[-1] == want_open
    text = b'a,"x\\"y\ny",b\\\nc\n"q\\\\"\nz\\,w\n"open\\'
    assert len(text) == 33
    for args, want in (((0x0A, Q, E, False), ([15, 21, 26], 3)), ((0x2C, Q, E, False), ([1, 10], 3)), ((0x0A, Q, E, True), ([7, 15, 21, 26], 2))):
        for rule in (escaped_oracle.serial, escaped_oracle.vec):
            pos, open_ = rule(np.frombuffer(text, dtype=np.uint8), *args)
            assert (pos.tolist(), open_) == want, args


def test_the_tile_maps_hold_against_a_serial_walk(tmp_path):
    """tools/index_escaped_emu.cpp: the pass lane by lane on the CPU around the real arithmetic of csrc/brx_index_escaped.h -- the
    escaped mask for all 2^17 inputs, then count, resolve (composition of the tiles' state maps) and fill on 400 random batches against
    the serial rule."""
    exe = str(tmp_path / "ie_emu")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "brotli-rs_amd", "csrc"),
                        os.path.join(ROOT, "tools", "index_escaped_emu.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ie_escaped ok" in r.stdout and "all ok" in r.stdout, r.stdout[-2000:]
