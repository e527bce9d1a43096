"""CPU-side checks of the digest ABI (include/brx.h): brx_digest_batch is declared and exported, the two BRX_DIGEST_* kinds have the
documented values, the argument checks that need no GPU answer, and the layers above the ABI expose the call.  No GPU needed."""
import os
import re
import subprocess

import brotli_rs_amd
from brotli_rs_amd import brx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "brx.h")).read()


def test_digest_batch_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+brx_digest_batch\s*\(\s*brx_ctx\s*\*\s*ctx\s*,\s*uint32_t\s+kind\s*,\s*const\s+uint8_t\s*\*\s*out\s*,\s*"
                     r"const\s+uint64_t\s*\*\s*out_off\s*,\s*const\s+uint64_t\s*\*\s*len\s*,\s*uint32_t\s+n\s*,\s*uint32_t\s*\*\s*digest\s*,\s*"
                     r"const\s+uint32_t\s*\*\s*expect\s*,\s*uint32_t\s*\*\s*mismatch\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", hdr)
    path = brotli_rs_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    exported = set(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip())
    assert "brx_digest_batch" in exported
    assert brx.load_library().brx_digest_batch is not None
    assert "brx_digest_batch" in brx.EXPORTED_SYMBOLS
    blob = open(path, "rb").read()
    for kernel in (b"brx_tile_plan_kernel", b"brx_digest_tiles_kernel", b"brx_digest_fold_kernel"):
        assert kernel in blob  # the pass is native code in the library, next to the decode kernels


def test_digest_kinds_have_the_documented_values():
    hdr = _header()
    assert re.search(r"^#define\s+BRX_DIGEST_CRC32\s+1u\b", hdr, flags=re.M)
    assert re.search(r"^#define\s+BRX_DIGEST_CRC32C\s+2u\b", hdr, flags=re.M)
    assert brx.DIGEST_KINDS == {"crc32": 1, "crc32c": 2}


def test_argument_checks_that_need_no_gpu():
    """A NULL context is refused before anything touches HIP."""
    lib = brx.load_library()
    assert lib.brx_digest_batch(None, 1, None, None, None, 0, None, None, None, None) == -1  # BRX_ERR_INVALID_ARGUMENT
    assert b"ctx is NULL" in lib.brx_last_error()


def test_wrappers_expose_the_call():
    assert callable(brx.Context.digest_batch) and callable(brx.Context.digest_batch_device)
    src = ('#include "brotli-rs_amd/host/decompressor.hpp"\n'
           "int main() { uint32_t d[1]; brotli::digest_batch(nullptr, BRX_DIGEST_CRC32C, nullptr, nullptr, nullptr, 0, d); return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
