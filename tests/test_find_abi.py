"""CPU-side checks of the find ABI (include/brx.h): brx_find_batch is declared and exported, its kernels are native code in the library,
the argument checks that need no GPU answer in the order the header gives, and the layers above the ABI expose the call.  No GPU
needed."""
import ctypes
import os
import re
import subprocess

import brotli_rs_amd
from brotli_rs_amd import brx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "brx.h")).read()


def test_find_batch_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+brx_find_batch\s*\(\s*brx_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*needle\s*,\s*uint32_t\s+needle_len\s*,\s*"
                     r"const\s+uint8_t\s*\*\s*out\s*,\s*const\s+uint64_t\s*\*\s*out_off\s*,\s*const\s+uint64_t\s*\*\s*len\s*,\s*"
                     r"uint32_t\s+n\s*,\s*uint64_t\s+span\s*,\s*uint64_t\s*\*\s*count\s*,\s*"
                     r"const\s+uint64_t\s*\*\s*pos_off\s*,\s*uint64_t\s*\*\s*pos\s*,\s*uint64_t\s+total\s*,\s*"
                     r"void\s*\*\s*hip_stream\s*\)\s*;", hdr)
    path = brotli_rs_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    exported = set(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip())
    assert "brx_find_batch" in exported
    assert "brx_find_batch" in brx.EXPORTED_SYMBOLS
    assert brx.load_library().brx_find_batch is not None
    blob = open(path, "rb").read()
    for kernel in (b"brx_find_count_kernel", b"brx_find_fill_kernel"):
        assert kernel in blob  # the pass is native code in the library, next to the index passes


def test_header_states_the_rule_and_its_limits():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+brx_find_batch", _header(), flags=re.S)
    assert m
    text = m.group(1)
    for word in ("overlapping", "needle_len", "HOST", "16", "OCCURRENCE", "shorter than m", "case folding", "brx_index_batch"):
        assert word in text, word


def test_argument_checks_that_need_no_gpu():
    """ctx NULL, then needle NULL, needle_len 0 and 17 are refused before anything touches HIP (the handle below is no context: a call
    that got past the checks would not come back with these messages)."""
    lib = brx.load_library()
    assert lib.brx_find_batch(None, b"\r\n", 2, None, None, None, 0, 0, None, None, None, 0, None) == -1  # BRX_ERR_INVALID_ARGUMENT
    assert lib.brx_last_error().startswith(b"brx_find_batch:") and b"ctx is NULL" in lib.brx_last_error()
    fake = ctypes.create_string_buffer(1 << 16)  # never read: the checks come first
    h = ctypes.addressof(fake)
    assert lib.brx_find_batch(h, None, 2, None, None, None, 0, 0, None, None, None, 0, None) == -1
    assert lib.brx_last_error().startswith(b"brx_find_batch:") and b"needle is NULL" in lib.brx_last_error()
    for bad in (0, 17, 1 << 31):
        assert lib.brx_find_batch(h, b"x" * 17, bad, None, None, None, 0, 0, None, None, None, 0, None) == -1
        assert lib.brx_last_error().startswith(b"brx_find_batch:") and b"needle_len" in lib.brx_last_error()
    # the order: a NULL context wins over a bad needle, a NULL needle over a bad length
    assert lib.brx_find_batch(None, None, 0, None, None, None, 0, 0, None, None, None, 0, None) == -1
    assert b"ctx is NULL" in lib.brx_last_error()
    assert lib.brx_find_batch(h, None, 0, None, None, None, 0, 0, None, None, None, 0, None) == -1
    assert b"needle is NULL" in lib.brx_last_error()


def test_wrappers_expose_the_call():
    assert callable(brx.Context.find_batch) and callable(brx.Context.find_batch_device)
    src = ('#include "brotli-rs_amd/host/decompressor.hpp"\n'
           "int main() { uint64_t c[1], p[1]; const uint8_t crlf[2] = {13, 10};\n"
           "             brotli::find_batch(nullptr, crlf, 2, nullptr, nullptr, nullptr, 0, 0, c);\n"
           "             brotli::find_batch(nullptr, crlf, 2, nullptr, nullptr, nullptr, 0, 0, nullptr, c, p, 1, nullptr);\n"
           "             return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
