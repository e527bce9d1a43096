"""CPU-side checks of the reader-round ABI (include/brx.h): brx_stream_advance / brx_stream_ready are declared and exported, the
option and the counters are documented, and the Python / C++ layers above the ABI expose them.  No GPU needed."""
import os
import re
import subprocess

import brotli_rs_amd
from brotli_rs_amd import brx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "brx.h")).read()


def test_advance_and_ready_are_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+brx_stream_advance\s*\(\s*brx_stream\s*\*const\s*\*\s*streams\s*,\s*uint32_t\s+n\s*\)\s*;", hdr)
    assert re.search(r"int64_t\s+brx_stream_ready\s*\(\s*const\s+brx_stream\s*\*\s*s\s*\)\s*;", hdr)
    path = brotli_rs_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    exported = set(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip())
    assert {"brx_stream_advance", "brx_stream_ready"} <= exported
    lib = brx.load_library()
    assert lib.brx_stream_advance is not None and lib.brx_stream_ready is not None
    assert lib.brx_stream_advance(None, 0) == 0  # (nothing to do: no GPU call)
    assert lib.brx_stream_ready(None) == 0


def test_reader_batch_option_and_counters_are_documented():
    hdr = _header()
    assert re.search(r"BRX_OPTION_READER_BATCH\s*=\s*15\b", hdr)
    assert re.search(r"\*\s+16, 17\s+\(since the context was made\) slice launches", hdr)
    assert brx.OPTIONS["reader_batch"] == 15
    for name in ("advance", "reader_slice_launches", "reader_slices"):
        assert callable(getattr(brx.Context, name))
    assert callable(brx.advance) and callable(brx.Decompressor.ready)


def test_cpp_wrapper_has_a_free_advance():
    src = ('#include "brotli-rs_amd/host/decompressor.hpp"\n'
           "int main() { std::vector<brotli::Decompressor<brotli::SliceReader> *> v; return (int)brotli::advance(v); }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
