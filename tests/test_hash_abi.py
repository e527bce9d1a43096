"""CPU-side checks of the hash ABI (include/brx.h): brx_hash_batch is declared and exported, its kernel is native code in the library, the
argument checks that need no GPU answer in the order the contract gives, the layers above the ABI expose the call, the two statements
of the definition in tests/hash_oracle.py agree with each other and with the contract's check values, and the lane path and the wave
path of the kernel restated on the CPU (tools/hash_emu.cpp) hold against a byte-serial walk without a load outside the arena.  No GPU
needed."""
import ctypes
import os
import re
import subprocess

import numpy as np

import brotli_rs_amd
import hash_oracle
from brotli_rs_amd import brx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "brx.h")).read()


def test_hash_batch_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    u64p, cu64p = r"uint64_t\s*\*\s*", r"const\s+uint64_t\s*\*\s*"
    assert re.search(r"int\s+brx_hash_batch\s*\(\s*brx_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*out\s*,\s*" + cu64p + r"out_off\s*,\s*" + cu64p
                     + r"len\s*,\s*uint32_t\s+n\s*,\s*uint64_t\s+span\s*,\s*" + cu64p + r"count\s*,\s*" + cu64p + r"pos_off\s*,\s*" + cu64p
                     + r"pos\s*,\s*uint64_t\s+n_pos\s*,\s*uint32_t\s+delim_len\s*,\s*uint32_t\s+flags\s*,\s*"
                     r"const\s+uint32_t\s*\*\s*sel_stream\s*,\s*" + cu64p + r"sel_rec\s*,\s*uint64_t\s+m\s*,\s*uint64_t\s+seed\s*,\s*" + u64p
                     + r"hash\s*,\s*" + u64p + r"rec_len\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", hdr)
    assert hdr.index("brx_take_batch") < hdr.index("brx_hash_batch")  # behind brx_take_batch
    path = brotli_rs_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    exported = set(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip())
    assert "brx_hash_batch" in exported
    assert "brx_hash_batch" in brx.EXPORTED_SYMBOLS
    assert brx.load_library().brx_hash_batch is not None
    assert b"brx_hash_kernel" in open(path, "rb").read()  # the pass is native code in the library


def test_header_states_the_definition_and_its_limits():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+brx_hash_batch", _header(), flags=re.S)
    assert m
    text = m.group(1)
    for word in ("DEVICE", "2^61", "K(seed)", "mix", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "0x9E3779B97F4A7C15", "little-endian",
                 "U = ceil(L / 4)", "The empty record hashes to 0", "Equal records", "ceil(Lmax / 4) / p", "14.8 M", "two seeds",
                 "not cryptographic", "S(A || B) = S(A) * K^(U_B) + S(B)", "never loaded", "BRX_TAKE_NO_DELIM", "BRX_TAKE_TRIM_CR",
                 "rec_len", "whole of stream i", "No scratch", "Not in scope", "in this order"):
        assert word in text, word
    flat = text.lower()
    for seed, (K, table) in hash_oracle.CHECK.items():  # the check values, all of them
        assert "0x%x" % K in flat, (seed, "K")
        for r, v in table.items():
            assert "0x%016x" % v in flat, (seed, r[:16])
    for v in hash_oracle.CHECK_PRE_MIX.values():
        assert "0x%016x" % v in flat


def _call(lib, h, flags=0, D=1, ss=None, sr=None, m=0, hash_=None, rec_len=None, out_off=None, ln=None, count=None, pos_off=None, pos=None,
          n_pos=0, n=0, span=0, seed=0):
    return lib.brx_hash_batch(h, None, out_off, ln, n, span, count, pos_off, pos, n_pos, D, flags, ss, sr, m, seed, hash_, rec_len, None)


def test_argument_checks_that_need_no_gpu():
    """Every refusal that needs no GPU, in the contract's order (the handle below is no context: a call that got past the checks would
    not come back with these messages).  Each case violates its own check AND every later one it can, so a check out of order shows."""
    lib = brx.load_library()
    fake = ctypes.create_string_buffer(1 << 16)  # never read: the checks come first
    h = ctypes.addressof(fake)
    P = ctypes.addressof(ctypes.create_string_buffer(64))  # stands for any non-NULL device pointer: never dereferenced by the host

    def refused(word, *a, **kw):
        assert _call(lib, *a, **kw) == -1, word  # BRX_ERR_INVALID_ARGUMENT
        e = lib.brx_last_error()
        assert e.startswith(b"brx_hash_batch:") and word in e, (word, e)

    refused(b"ctx is NULL", None, flags=4, D=0, ss=P, m=1)
    refused(b"unknown flag bits", h, flags=4, D=0, ss=P, m=1)
    refused(b"unknown flag bits", h, flags=1 << 31, D=0, ss=P, m=1)
    refused(b"BRX_TAKE_TRIM_CR without", h, flags=2, D=0, ss=P, m=1)
    for bad in (0, 17, 1 << 31):
        refused(b"delim_len", h, flags=3, D=bad, ss=P, m=1)
    refused(b"sel_stream and sel_rec", h, ss=P, m=1)
    refused(b"sel_stream and sel_rec", h, sr=P, m=1)
    refused(b"hash is NULL", h, m=5, n_pos=3)
    refused(b"hash is NULL", h, m=0, rec_len=P)  # (in front of the m = 0 exit)
    # m = 0: success, no launch, whatever else is NULL
    assert _call(lib, h, hash_=P) == 0
    assert _call(lib, h, flags=3, D=16, ss=P, sr=P, hash_=P, rec_len=P, n_pos=3, span=1 << 63) == 0
    tabs = dict(out_off=P, ln=P, count=P, pos_off=P)
    for missing in tabs:
        kw = dict(tabs)
        kw[missing] = None
        refused(b"NULL table", h, m=1, hash_=P, n_pos=3, **kw)
    refused(b"pos is NULL with n_pos > 0", h, m=1, hash_=P, n_pos=3, **tabs)
    refused(b"all-records mode with n = 0", h, m=1, hash_=P, span=1 << 63, **tabs)
    refused(b"span out of range", h, m=1 << 62, hash_=P, n=1, span=1 << 63, **tabs)
    refused(b"span out of range", h, m=1, hash_=P, ss=P, sr=P, span=1 << 63, **tabs)
    refused(b"m out of range", h, m=1 << 62, hash_=P, rec_len=P, n=1, span=64, **tabs)


def test_wrappers_expose_the_call():
    assert callable(brx.Context.hash_batch) and callable(brx.Context.hash_batch_device)
    doc = brx.Context.hash_batch.__doc__
    for word in ("index_set_batch", "torch.unique", "return_inverse", "take_batch", "sel_stream"):  # the dedup idiom
        assert word in doc, word
    src = ('#include "brotli-rs_amd/host/decompressor.hpp"\n'
           "int main() { uint64_t t[4]; uint32_t s[1];\n"
           "             brotli::hash_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, 1, 1, BRX_TAKE_NO_DELIM | BRX_TAKE_TRIM_CR, s, t, 1, 7u, t);\n"
           "             brotli::hash_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, 1, 2, 0, nullptr, nullptr, 2, 0, t, t, nullptr);\n"
           "             return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_two_statements_of_the_definition_agree():
    rng = np.random.default_rng(17)
    for it in range(2000):
        r = rng.integers(0, 256, int(rng.integers(0, 71))).astype(np.uint8).tobytes()
        seed = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)) if it % 5 else (0, 1, hash_oracle.M64, 1 << 63)[it // 5 % 4]
        want = hash_oracle.hash_direct(r, seed)
        assert 0 <= want < 1 << 64
        for chunk in (1, 4, 5, 256):
            assert hash_oracle.hash_chunked(r, seed, chunk) == want, (it, chunk)
        arena = np.frombuffer(b"\r" + r + b"\r", dtype=np.uint8)
        assert hash_oracle.hash_records(arena, [1], [len(r)], seed).tolist() == [hash_oracle.as_i64(want)]
        if not r:
            assert want == 0
    assert hash_oracle.mix(0) == 0 and 2 <= hash_oracle.key(0) <= hash_oracle.P - 2


def test_the_composition_law_at_every_word_aligned_split():
    rng = np.random.default_rng(18)
    P = hash_oracle.P
    for L in (0, 1, 3, 4, 5, 16, 17, 63, 64, 70, 1030):
        r = rng.integers(0, 256, L).astype(np.uint8).tobytes()
        seed = int(rng.integers(0, 1 << 62))
        K = hash_oracle.key(seed)
        S = (hash_oracle.h_direct(r, seed) - L) % P
        for cut in range(0, L + 1, 4):  # A = r[:cut] is a whole number of words
            A, B = r[:cut], r[cut:]
            SA, SB = (hash_oracle.h_direct(A, seed) - len(A)) % P, (hash_oracle.h_direct(B, seed) - len(B)) % P
            assert (SA * pow(K, (len(B) + 3) // 4, P) + SB) % P == S, (L, cut)


def test_check_values_of_the_contract():
    for seed, (K, table) in hash_oracle.CHECK.items():
        assert hash_oracle.key(seed) == K
        for r, v in table.items():
            assert hash_oracle.hash_direct(r, seed) == v and hash_oracle.hash_chunked(r, seed) == v, (seed, r[:16])
    for r, v in hash_oracle.CHECK_PRE_MIX.items():
        assert hash_oracle.h_direct(r, 0) == v
    # a trailing zero byte is not padding: L is part of the hash
    assert hash_oracle.hash_direct(b"a", 0) != hash_oracle.hash_direct(b"a\0", 0)


def test_both_paths_hold_against_a_serial_walk(tmp_path):
    """tools/hash_emu.cpp: the lane path and the wave path, lane by lane on the CPU around the real text of csrc/brx_hash.h and
    csrc/brx_take.h; it fails on any load outside [out, out + span) and on a length x phase combination that was not met."""
    exe = str(tmp_path / "hash_emu")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "brotli-rs_amd", "csrc"),
                        os.path.join(ROOT, "tools", "hash_emu.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK: 416 batches") and "every length 0 .. 2088 at all 16 phases" in r.stdout \
        and "none outside" in r.stdout, r.stdout[-2000:]
