"""CPU-side checks of the quoted index ABI (include/brx.h): brx_index_quoted_batch is declared and exported, its kernels are native
code in the library, the argument checks that need no GPU answer, and the layers above the ABI expose the call.  No GPU needed."""
import os
import re
import subprocess

import brotli_rs_amd
from brotli_rs_amd import brx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "brx.h")).read()


def test_index_quoted_batch_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+brx_index_quoted_batch\s*\(\s*brx_ctx\s*\*\s*ctx\s*,\s*uint8_t\s+delim\s*,\s*uint8_t\s+quote\s*,\s*"
                     r"const\s+uint8_t\s*\*\s*out\s*,\s*const\s+uint64_t\s*\*\s*out_off\s*,\s*const\s+uint64_t\s*\*\s*len\s*,\s*"
                     r"uint32_t\s+n\s*,\s*uint64_t\s+span\s*,\s*uint64_t\s*\*\s*count\s*,\s*uint32_t\s*\*\s*open\s*,\s*"
                     r"const\s+uint64_t\s*\*\s*pos_off\s*,\s*uint64_t\s*\*\s*pos\s*,\s*uint64_t\s+total\s*,\s*"
                     r"void\s*\*\s*hip_stream\s*\)\s*;", hdr)
    path = brotli_rs_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    exported = set(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip())
    assert "brx_index_quoted_batch" in exported
    assert "brx_index_quoted_batch" in brx.EXPORTED_SYMBOLS
    assert brx.load_library().brx_index_quoted_batch is not None
    blob = open(path, "rb").read()
    for kernel in (b"brx_index_quoted_count_kernel", b"brx_index_quoted_resolve_kernel", b"brx_index_quoted_fill_kernel"):
        assert kernel in blob  # the pass is native code in the library, next to the plain index pass


def test_header_states_the_rule_and_its_limits():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+brx_index_quoted_batch", _header(), flags=re.S)
    assert m
    text = m.group(1)
    for word in ("even", "open[i]", "escape", "CR", "more than one byte", "delim == quote"):
        assert word in text, word


def test_argument_checks_that_need_no_gpu():
    """A NULL context and delim == quote are refused before anything touches HIP (the handle below is no context: a call that got
    past the check would not come back with this message)."""
    lib = brx.load_library()
    assert lib.brx_index_quoted_batch(None, 10, 34, None, None, None, 0, 0, None, None, None, None, 0, None) == -1  # BRX_ERR_INVALID_ARGUMENT
    assert b"brx_index_quoted_batch" in lib.brx_last_error() and b"ctx is NULL" in lib.brx_last_error()
    import ctypes
    fake = ctypes.create_string_buffer(1 << 16)  # never read: the check comes first
    assert lib.brx_index_quoted_batch(ctypes.addressof(fake), 34, 34, None, None, None, 0, 0, None, None, None, None, 0, None) == -1
    assert b"brx_index_quoted_batch" in lib.brx_last_error() and b"quote" in lib.brx_last_error()


def test_wrappers_expose_the_call():
    assert callable(brx.Context.index_quoted_batch) and callable(brx.Context.index_quoted_batch_device)
    src = ('#include "brotli-rs_amd/host/decompressor.hpp"\n'
           "int main() { uint64_t c[1], p[1]; uint32_t o[1];\n"
           "             brotli::index_quoted_batch(nullptr, '\\n', '\"', nullptr, nullptr, nullptr, 0, 0, c);\n"
           "             brotli::index_quoted_batch(nullptr, '\\n', '\"', nullptr, nullptr, nullptr, 0, 0, c, o);\n"
           "             brotli::index_quoted_batch(nullptr, 0, 255, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, c, p, 1, nullptr);\n"
           "             return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
