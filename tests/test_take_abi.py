"""CPU-side checks of the take ABI (include/brx.h): brx_take_batch is declared and exported, its kernels are native code in the library,
the argument checks that need no GPU answer in the order the contract gives, the layers above the ABI expose the call, the two
statements of the rule in tests/take_oracle.py agree, and the lane logic of the fill kernel restated on the CPU (tools/take_emu.cpp)
holds against a serial walk without a load outside the arena.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np

import brotli_rs_amd
import take_oracle
from brotli_rs_amd import brx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "brx.h")).read()


def test_take_batch_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+BRX_TAKE_NO_DELIM\s+1u", hdr) and re.search(r"#define\s+BRX_TAKE_TRIM_CR\s+2u", hdr)
    assert re.search(r"#define\s+BRX_TAKE_MAX_DELIM\s+16u", hdr)
    u64p, cu64p = r"uint64_t\s*\*\s*", r"const\s+uint64_t\s*\*\s*"
    assert re.search(r"int\s+brx_take_batch\s*\(\s*brx_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*out\s*,\s*" + cu64p + r"out_off\s*,\s*" + cu64p
                     + r"len\s*,\s*uint32_t\s+n\s*,\s*uint64_t\s+span\s*,\s*" + cu64p + r"count\s*,\s*" + cu64p + r"pos_off\s*,\s*" + cu64p
                     + r"pos\s*,\s*uint64_t\s+n_pos\s*,\s*uint32_t\s+delim_len\s*,\s*uint32_t\s+flags\s*,\s*"
                     r"const\s+uint32_t\s*\*\s*sel_stream\s*,\s*" + cu64p + r"sel_rec\s*,\s*uint64_t\s+m\s*,\s*" + u64p + r"rec_len\s*,\s*"
                     + cu64p + r"dst_off\s*,\s*uint8_t\s*\*\s*dst\s*,\s*uint64_t\s+total\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", hdr)
    assert hdr.index("brx_find_batch") < hdr.index("brx_take_batch")  # behind brx_find_batch
    path = brotli_rs_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    exported = set(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip())
    assert "brx_take_batch" in exported
    assert "brx_take_batch" in brx.EXPORTED_SYMBOLS
    assert brx.load_library().brx_take_batch is not None
    assert brx.TAKE_NO_DELIM == 1 and brx.TAKE_TRIM_CR == 2
    blob = open(path, "rb").read()
    for kernel in (b"brx_take_size_kernel", b"brx_take_fill_kernel"):
        assert kernel in blob  # the pass is native code in the library


def test_header_states_the_rule_and_its_limits():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+BRX_TAKE_NO_DELIM[^\n]*\n#define\s+BRX_TAKE_TRIM_CR[^\n]*\n#define\s+BRX_TAKE_MAX_DELIM"
                  r"\s+16u\s*int\s+brx_take_batch", _header(), flags=re.S)
    assert m
    text = m.group(1)
    for word in ("DEVICE", "P(i,k)", "n_pos", "delim_len", "TRAILING", "max(end, start)", "0x0D", "BRX_TAKE_NO_DELIM", "BRX_TAKE_TRIM_CR",
                 "Pairs mode", "All-records mode", "sum(count) + n", "SIZE MODE", "FILL MODE", "ROOM", "non-decreasing", "left as they were",
                 ">=\n * total is written", "last entry whose dst_off is not behind it", "must not overlap", "never a load outside",
                 "No scratch", "Not in scope", "in this order"):
        assert word in text, word


def _call(lib, h, flags=0, D=1, ss=None, sr=None, m=0, rec_len=None, dst_off=None, dst=None, out_off=None, ln=None, count=None, pos_off=None,
          pos=None, n_pos=0, n=0, span=0):
    return lib.brx_take_batch(h, None, out_off, ln, n, span, count, pos_off, pos, n_pos, D, flags, ss, sr, m, rec_len, dst_off, dst, 0, None)


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
        assert e.startswith(b"brx_take_batch:") and word in e, (word, e)

    refused(b"ctx is NULL", None, flags=4, D=0)
    refused(b"unknown flag bits", h, flags=4, D=0)
    refused(b"unknown flag bits", h, flags=1 << 31, D=0)
    refused(b"BRX_TAKE_TRIM_CR without", h, flags=2, D=0)
    for bad in (0, 17, 1 << 31):
        refused(b"delim_len", h, flags=3, D=bad, ss=P)
    refused(b"sel_stream and sel_rec", h, ss=P, dst=P)
    refused(b"sel_stream and sel_rec", h, sr=P, dst=P)
    refused(b"dst_off and dst", h, dst=P)
    refused(b"dst_off and dst", h, dst_off=P)
    refused(b"rec_len is NULL in size mode", h, m=5)
    # m = 0: success, no launch, whatever else is NULL
    assert _call(lib, h, rec_len=P) == 0
    assert _call(lib, h, dst_off=P, dst=P) == 0
    assert _call(lib, h, flags=3, D=16, ss=P, sr=P, rec_len=P, dst_off=P, dst=P) == 0
    tabs = dict(out_off=P, ln=P, count=P, pos_off=P)
    for missing in tabs:
        kw = dict(tabs)
        kw[missing] = None
        refused(b"NULL table", h, m=1, rec_len=P, n_pos=3, **kw)
    refused(b"pos is NULL with n_pos > 0", h, m=1, rec_len=P, n_pos=3, **tabs)
    refused(b"all-records mode with n = 0", h, m=1, rec_len=P, span=1 << 63, **tabs)
    refused(b"span out of range", h, m=1, rec_len=P, n=1, span=1 << 63, **tabs)
    refused(b"span out of range", h, m=1, rec_len=P, ss=P, sr=P, span=1 << 63, **tabs)


def test_wrappers_expose_the_call():
    assert callable(brx.Context.take_batch) and callable(brx.Context.take_batch_device)
    src = ('#include "brotli-rs_amd/host/decompressor.hpp"\n'
           "int main() { uint64_t t[4]; uint32_t s[1]; uint8_t d[8];\n"
           "             brotli::take_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, 1, 1, BRX_TAKE_NO_DELIM | BRX_TAKE_TRIM_CR, s, t, 1, t);\n"
           "             brotli::take_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, 1, 2, 0, nullptr, nullptr, 2, nullptr, t, d, 8, nullptr);\n"
           "             return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_lane_logic_holds_against_a_serial_walk(tmp_path):
    """tools/take_emu.cpp: the fill kernel's loop lane by lane on the CPU around the real text of csrc/brx_take.h, on 720 random
    batches; it fails on any load outside [out, out + span) and on any store outside dst[0 .. total)."""
    exe = str(tmp_path / "take_emu")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "brotli-rs_amd", "csrc"),
                        os.path.join(ROOT, "tools", "take_emu.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK: 720 batches") and "none outside" in r.stdout, r.stdout[-2000:]


def _random_batch(rng, stale):
    n = int(rng.integers(1, 6))
    lens = [int(rng.integers(0, 90)) if rng.integers(0, 6) else 0 for _ in range(n)]
    off, arena = [], []
    for ln in lens:
        arena += [13] * int(rng.integers(0, 5))
        off.append(len(arena))
        arena += rng.choice(np.array([10, 13, 97, 98], dtype=np.uint8), ln, p=[0.2, 0.2, 0.3, 0.3]).tolist()
    arena = np.array(arena + [13], dtype=np.uint8)
    count, pos_off, pos = take_oracle.index_positions(arena, off, lens, b"\n")
    n_pos = len(pos)
    if stale:
        pos = pos.copy()
        for j in range(len(pos)):
            r = int(rng.integers(0, 4))
            if r == 0:
                pos[j] = int(rng.integers(0, 200))
            elif r == 1:
                pos[j] = -1 - int(rng.integers(0, 3))  # 2^64 - 1 ... as the device reads it
        n_pos = int(rng.integers(0, len(pos) + 1))
    return arena, off, lens, count, pos_off, pos, n_pos


def test_the_two_statements_of_the_rule_agree():
    rng = np.random.default_rng(23)
    for it in range(400):
        arena, off, lens, count, pos_off, pos, n_pos = _random_batch(rng, stale=it % 4 == 3)
        n = len(lens)
        D = (1, 2, 16)[it % 3]
        flags = (0, 1, 3)[(it // 3) % 3]
        if it % 2:
            m = int(rng.integers(0, 40))
            si = [int(rng.integers(0, n + 2)) for _ in range(m)]
            sk = [int(rng.integers(0, int(count[min(i, n - 1)]) + 3)) for i in si]
        else:
            m = int(count.sum()) + n + int(rng.integers(0, 3))
            si, sk = take_oracle.entries_all_serial(count, pos_off, m)
            vi, vk = take_oracle.entries_all_vec(count, pos_off, m)
            assert list(vi) == si and list(vk) == sk
        src, L = take_oracle.records_serial(arena, off, lens, count, pos_off, pos, n_pos, D, flags, si, sk)
        vsrc, vL = take_oracle.records_vec(arena, off, lens, count, pos_off, pos, n_pos, D, flags, si, sk)
        assert list(vsrc) == src and list(vL) == L, it
        for i, k, a, ln in zip(si, sk, src, L):  # every record lies inside its stream
            if ln:
                assert off[i] <= a and a + ln <= off[i] + lens[i]
        stride = int(rng.integers(1, 30))
        dst_off = np.arange(m) * stride if it % 5 == 0 else np.cumsum([0] + L[:-1]) if m else np.zeros(0, dtype=np.int64)
        total = (m * stride if it % 5 == 0 else sum(L))
        if it % 7 == 0:
            total //= 2
        want = take_oracle.fill_serial(arena, src, L, dst_off, total, np.full(total + 8, 0xEE, dtype=np.uint8))
        got = take_oracle.fill_vec(arena, src, L, dst_off, total, np.full(total + 8, 0xEE, dtype=np.uint8))
        assert want.tolist() == got.tolist(), it
        assert (want[total:] == 0xEE).all()


def test_check_values_of_the_contract():
    """Text C of brx_index_set_batch's contract, plain index at ",\\n\\r": the record lists written out by hand."""
    C = b'a,"b,c\n",d\r\ne,"f""g",h\n"x'
    assert len(C) == 25
    arena = np.frombuffer(C, dtype=np.uint8)
    count, pos_off, pos = take_oracle.index_positions(arena, [0], [25], b",\n\r")
    assert pos.tolist() == [1, 4, 6, 8, 10, 11, 13, 20, 22]
    for flags, want in ((0, [b"a,", b'"b,', b"c\n", b'",', b"d\r", b"\n", b"e,", b'"f""g",', b"h\n", b'"x']),
                        (1, [b"a", b'"b', b"c", b'"', b"d", b"", b"e", b'"f""g"', b"h", b'"x']),
                        (3, [b"a", b'"b', b"c", b'"', b"d", b"", b"e", b'"f""g"', b"h", b'"x'])):
        for fn in (take_oracle.records_serial, take_oracle.records_vec):
            src, L = fn(arena, [0], [25], count, pos_off, pos, 9, 1, flags, [0] * 10, list(range(10)))
            assert [C[a:a + ln] for a, ln in zip(src, L)] == want
    # at "\n" alone TRIM_CR drops the CR of the CRLF line
    count, pos_off, pos = take_oracle.index_positions(arena, [0], [25], b"\n")
    src, L = take_oracle.take_vec(arena, [0], [25], count, pos_off, pos, len(pos), 1, 3)
    assert [C[a:a + ln] for a, ln in zip(src, L)] == [b'a,"b,c', b'",d', b'e,"f""g",h', b'"x']
