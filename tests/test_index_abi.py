"""CPU-side checks of the index ABI (include/brx.h): brx_index_batch is declared and exported, its kernels are native code in the
library, the argument check that needs no GPU answers, and the layers above the ABI expose the call.  No GPU needed."""
import os
import re
import subprocess

import brotli_rs_amd
from brotli_rs_amd import brx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "brx.h")).read()


def test_index_batch_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+brx_index_batch\s*\(\s*brx_ctx\s*\*\s*ctx\s*,\s*uint8_t\s+delim\s*,\s*const\s+uint8_t\s*\*\s*out\s*,\s*"
                     r"const\s+uint64_t\s*\*\s*out_off\s*,\s*const\s+uint64_t\s*\*\s*len\s*,\s*uint32_t\s+n\s*,\s*uint64_t\s+span\s*,\s*"
                     r"uint64_t\s*\*\s*count\s*,\s*const\s+uint64_t\s*\*\s*pos_off\s*,\s*uint64_t\s*\*\s*pos\s*,\s*uint64_t\s+total\s*,\s*"
                     r"void\s*\*\s*hip_stream\s*\)\s*;", hdr)
    path = brotli_rs_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    exported = set(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip())
    assert "brx_index_batch" in exported
    assert brx.load_library().brx_index_batch is not None
    assert "brx_index_batch" in brx.EXPORTED_SYMBOLS
    blob = open(path, "rb").read()
    for kernel in (b"brx_tile_plan_kernel", b"brx_index_count_kernel", b"brx_index_scan_kernel", b"brx_index_fill_kernel"):
        assert kernel in blob  # the pass is native code in the library, next to the decode kernels


def test_argument_check_that_needs_no_gpu():
    """A NULL context is refused before anything touches HIP."""
    lib = brx.load_library()
    assert lib.brx_index_batch(None, 10, None, None, None, 0, 0, None, None, None, 0, None) == -1  # BRX_ERR_INVALID_ARGUMENT
    assert b"ctx is NULL" in lib.brx_last_error()


def test_wrappers_expose_the_call():
    assert callable(brx.Context.index_batch) and callable(brx.Context.index_batch_device)
    src = ('#include "brotli-rs_amd/host/decompressor.hpp"\n'
           "int main() { uint64_t c[1], p[1]; brotli::index_batch(nullptr, '\\n', nullptr, nullptr, nullptr, 0, 0, c);\n"
           "             brotli::index_batch(nullptr, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, c, p, 1, nullptr); return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
