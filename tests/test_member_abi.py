"""CPU-side checks of the member ABI (include/brx.h): brx_member_batch is declared behind brx_unescape_batch and exported, its kernels are
native code in the library, the header states the rule with every check value, the argument checks that need no GPU answer in the
order the contract gives, the layers above the ABI expose the call, the two statements of THE RULE in tests/member_oracle.py agree
with each other, with the contract's check values and with json.loads, and the five steps of the pass restated on the CPU
(tools/member_emu.cpp) hold against a boundary-serial walk without a load or a store outside their bounds.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np

import brotli_rs_amd
import member_oracle as mo
from brotli_rs_amd import brx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "brx.h")).read()


def test_member_batch_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    u64p, cu64p, cu8p, u8p = r"uint64_t\s*\*\s*", r"const\s+uint64_t\s*\*\s*", r"const\s+uint8_t\s*\*\s*", r"uint8_t\s*\*\s*"
    assert re.search(r"int\s+brx_member_batch\s*\(\s*brx_ctx\s*\*\s*ctx\s*,\s*" + cu8p + r"out\s*,\s*" + cu64p + r"out_off\s*,\s*" + cu64p
                     + r"len\s*,\s*uint32_t\s+n\s*,\s*uint64_t\s+span\s*,\s*" + cu64p + r"count\s*,\s*" + cu64p + r"pos_off\s*,\s*" + cu64p
                     + r"pos\s*,\s*" + cu8p + r"what\s*,\s*uint64_t\s+n_pos\s*,\s*" + cu8p + r"names\s*,\s*const\s+uint32_t\s*\*\s*name_len\s*,\s*"
                     r"uint32_t\s+n_names\s*,\s*" + u64p + r"lines\s*,\s*" + cu64p + r"line_off\s*,\s*uint64_t\s+m\s*,\s*uint32_t\s*\*\s*sel_stream"
                     r"\s*,\s*" + u64p + r"sel_rec\s*,\s*" + u8p + r"kind\s*,\s*" + u8p + r"line_flags\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", hdr)
    assert hdr.index("brx_unescape_batch") < hdr.index("brx_member_batch") < hdr.index("brx_stream_advance")  # directly behind it
    for name, v in (("MAX_NAMES", 8), ("MAX_NAME", 32), ("MAX_KEY", 64), ("MISSING", 0), ("SCALAR", 1), ("OBJECT", 2), ("ARRAY", 3), ("BAD", 4),
                    ("LONG_KEY", 1), ("ESCAPED_KEY", 2), ("UNBALANCED", 4)):
        assert re.search(r"#define\s+BRX_MEMBER_%s\s+%du" % (name, v), hdr), name
        assert getattr(brx, "MEMBER_" + name) == v
        assert getattr(mo, name) == v
    path = brotli_rs_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    exported = set(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip())
    assert "brx_member_batch" in exported
    assert "brx_member_batch" in brx.EXPORTED_SYMBOLS
    assert brx.load_library().brx_member_batch is not None
    lib = open(path, "rb").read()
    for kernel in (b"brx_member_kernel", b"brx_member_plan_kernel", b"brx_member_compose_kernel", b"brx_member_finish_kernel"):
        assert kernel in lib, kernel  # the pass is native code in the library


def test_header_states_the_rule_and_its_limits():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+BRX_MEMBER_MAX_NAMES", _header(), flags=re.S)
    assert m
    text = m.group(1)
    for word in ("DEVICE", "HOST memory", "THE RULE", "LINES", "DEPTH", "MEMBER", "VALUE", "LAST WINS", "TRAILING", "neutral", "signed",
                 "BRX_TAKE_NO_DELIM", "KEY RECORD", "0x20, 0x09 and 0x0D", "bytewise", "BRX_MEMBER_MAX_KEY = 64", "UINT64_MAX", "column-major",
                 "q * m + j", "COUNT MODE", "FILL MODE", "n_names * m", "Not in scope", "in this order", "never a load or a store", "json.loads",
                 "launch arguments", "pretty-printed", "nested", "BRX_MEMBER_LONG_KEY", "BRX_MEMBER_ESCAPED_KEY", "BRX_MEMBER_UNBALANCED",
                 "lines = 3", "no synchronisation"):
        assert word in text, word
    flat = " ".join(text.replace("*", " ").split())
    for c in mo.CHECK:  # the check values, all of them
        assert mo.header_form(*c) in flat, mo.header_form(*c)


def _call(lib, h, names=None, name_len=None, n_names=0, lines=None, line_off=None, m=0, ss=None, sr=None, kind=None, line_flags=None,
          out_off=None, ln=None, count=None, pos_off=None, pos=None, what=None, n_pos=0, n=0, span=0):
    lens = (ctypes.c_uint32 * len(name_len))(*name_len) if name_len is not None else None
    return lib.brx_member_batch(h, None, out_off, ln, n, span, count, pos_off, pos, what, n_pos, names, lens, n_names, lines, line_off, m,
                                ss, sr, kind, line_flags, None)


def test_argument_checks_that_need_no_gpu():
    """Every refusal, in the contract's order (the handle below is no context: a call that got past the checks would not come back
    with these messages).  Each case violates its own check AND every later one it can, so a check out of order shows."""
    lib = brx.load_library()
    fake = ctypes.create_string_buffer(1 << 16)  # never read: the checks come first
    h = ctypes.addressof(fake)
    P = ctypes.addressof(ctypes.create_string_buffer(64))  # stands for any non-NULL device pointer: never dereferenced by the host

    def refused(word, *a, **kw):
        assert _call(lib, *a, **kw) == -1, word  # BRX_ERR_INVALID_ARGUMENT
        err = lib.brx_last_error()
        assert err.startswith(b"brx_member_batch:") and word in err, (word, err)

    two = b"a".ljust(32, b"\0") + b"a".ljust(32, b"\0")  # the same name twice
    ab = b"a".ljust(32, b"\0") + b"ab".ljust(32, b"\0")
    later = dict(ss=P, line_flags=P, n=1, n_pos=3, span=1 << 63)  # violates the checks from "go together" on
    refused(b"ctx is NULL", None, n_names=9, **later)
    refused(b"names or name_len is NULL", h, n_names=9, **later)
    refused(b"names or name_len is NULL", h, names=two, n_names=9, **later)
    refused(b"names or name_len is NULL", h, name_len=[0], n_names=9, **later)
    for bad in (0, 9, 1 << 31):
        refused(b"n_names is not 1 .. 8", h, names=two, name_len=[0, 33], n_names=bad, **later)
    for bad in (0, 33, 1 << 31):
        refused(b"a name_len is not 1 .. 32", h, names=two, name_len=[1, bad], n_names=2, **later)
    refused(b"a name stands twice", h, names=two, name_len=[1, 1], n_names=2, **later)
    ok = dict(names=ab, name_len=[1, 2], n_names=2)
    assert _call(lib, h, names=ab, name_len=[1, 1], n_names=2, lines=P) == -1  # ("a" and "a" again: only name_len bytes count)
    full = dict(line_off=P, ss=P, sr=P, kind=P)
    for missing in full:
        kw = dict(full)
        kw[missing] = None
        refused(b"go together", h, n=1, n_pos=3, span=1 << 63, **ok, **kw)
        refused(b"go together", h, n=1, n_pos=3, span=1 << 63, **ok, **{missing: P})
    refused(b"line_flags is given in count mode", h, line_flags=P, n=1, n_pos=3, span=1 << 63, **ok)
    refused(b"lines is NULL in count mode", h, n=1, n_pos=3, span=1 << 63, **ok)
    # n = 0: success, no launch, whatever else is NULL
    assert _call(lib, h, lines=P, **ok) == 0
    assert _call(lib, h, n_pos=3, span=1 << 63, m=1 << 62, **ok, **full) == 0  # (fill mode needs no lines)
    assert _call(lib, h, m=5, line_flags=P, lines=P, **ok, **full) == 0
    tabs = dict(out_off=P, ln=P, count=P, pos_off=P)
    for missing in tabs:
        kw = dict(tabs)
        kw[missing] = None
        refused(b"NULL table", h, n=1, n_pos=3, span=1 << 63, lines=P, **ok, **kw)
    refused(b"pos or what is NULL with n_pos > 0", h, n=1, n_pos=3, span=1 << 63, lines=P, **ok, **tabs)
    refused(b"pos or what is NULL with n_pos > 0", h, n=1, n_pos=3, span=1 << 63, lines=P, pos=P, **ok, **tabs)
    refused(b"pos or what is NULL with n_pos > 0", h, n=1, n_pos=3, span=1 << 63, lines=P, what=P, **ok, **tabs)
    refused(b"span out of range", h, n=1, n_pos=1 << 62, span=1 << 63, m=1 << 62, pos=P, what=P, **ok, **tabs, **full)
    refused(b"m out of range", h, n=1, n_pos=1 << 62, span=64, m=1 << 62, pos=P, what=P, **ok, **tabs, **full)
    refused(b"n_pos out of range", h, n=1, n_pos=1 << 62, span=64, m=5, pos=P, what=P, **ok, **tabs, **full)


def test_refusals_through_the_python_wrapper():
    """Context.member_batch_device packs the names (32 bytes each, the true lengths beside them) and turns a refusal into BrxError with
    the library's text: every refusal again, in the contract's order, through it.  The Context stands on a handle that is no context,
    as above: a call that got past the checks would not raise these messages."""
    import pytest
    fake = ctypes.create_string_buffer(1 << 16)
    P = ctypes.addressof(ctypes.create_string_buffer(64))
    c = brx.Context.__new__(brx.Context)
    c._lib, c._h = brx.load_library(), None
    try:
        def refused(word, names, *a, **kw):
            with pytest.raises(brx.BrxError, match=r"brx_member_batch failed \(-1\): brx_member_batch: .*" + re.escape(word)):
                c.member_batch_device(P, P, P, 1, 1 << 63, P, P, None, None, 3, names, *a, **kw)

        late = dict(sel_stream_ptr=P, line_flags_ptr=P)  # violates the checks from "go together" on
        refused("ctx is NULL", [], None, **late)
        c._h = ctypes.addressof(fake)
        refused("n_names is not 1 .. 8", [], None, **late)                                      # 0 names
        refused("n_names is not 1 .. 8", [b"%d" % q for q in range(9)] + [b""], None, **late)   # 9 names and more
        refused("a name_len is not 1 .. 32", [b"a", b"x" * 33, b"a"], None, **late)             # a 33-byte name is not cut to fit
        refused("a name_len is not 1 .. 32", [b"a", b"", b"a"], None, **late)
        refused("a name stands twice", [b"a", b"ab", b"a"], None, **late)
        refused("a name stands twice", [b"k" * 32, b"k" * 32], None, **late)
        names = [b"a", b"ab", b"k" * 32]
        full = dict(line_off_ptr=P, sel_stream_ptr=P, sel_rec_ptr=P, kind_ptr=P)
        for missing in full:
            kw = dict(full)
            kw[missing] = None
            refused("go together", names, None, m=5, line_flags_ptr=P, **kw)
            refused("go together", names, None, **{missing: P})
        refused("line_flags is given in count mode", names, None, line_flags_ptr=P)
        refused("lines is NULL in count mode", names, None)
        refused("pos or what is NULL with n_pos > 0", names, P)                                 # (behind the n = 0 exit: n is 1 here)
        refused("pos or what is NULL with n_pos > 0", names, None, m=5, **full)
        # n = 0 succeeds without a launch, names of 1 and of 32 bytes pass
        c.member_batch_device(None, None, None, 0, 0, None, None, None, None, 0, names, P)
        c.member_batch_device(None, None, None, 0, 0, None, None, None, None, 0, [b"x"], None, m=7, line_flags_ptr=P, **full)
    finally:
        c._h = None  # (nothing to destroy)


def test_wrappers_expose_the_call():
    assert callable(brx.Context.member_batch) and callable(brx.Context.member_batch_device)
    doc = brx.Context.member_batch.__doc__
    for word in ("index_set_batch", "delims=b'{}[]:,\\n'", "json.loads", "MEMBER_SCALAR", "MEMBER_MISSING", "line_flags", "parse_batch",
                 "unescape_batch", "sel_stream=ss[0]"):
        assert word in doc, word
    src = ('#include "brotli-rs_amd/host/decompressor.hpp"\n'
           "int main() { uint64_t t[4]; uint32_t s[1]; uint8_t b[64];\n"
           "             brotli::member_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, b, 1, b, s, 1, t);\n"
           "             brotli::member_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, b, 1, b, s, 1, nullptr, t, 1, s, t, b, b, nullptr);\n"
           "             return BRX_MEMBER_MISSING + BRX_MEMBER_SCALAR + BRX_MEMBER_OBJECT + BRX_MEMBER_ARRAY + BRX_MEMBER_BAD +\n"
           "                    BRX_MEMBER_LONG_KEY + BRX_MEMBER_ESCAPED_KEY + BRX_MEMBER_UNBALANCED + BRX_MEMBER_MAX_NAMES; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read() + open(os.path.join(ROOT, "README.md")).read()
    assert text.count("brx_member_batch") >= 3


def test_check_values_of_the_contract():
    assert len(mo.CHECK) == 9
    for stream, names, want in mo.CHECK:
        for f in mo.FORMS.values():
            lines, found, flags = f(stream, names)
            assert lines == len(want)
            assert [({names[q]: v for q, v in cur.items()}, fl) for cur, fl in zip(found, flags)] == want, stream
    # the check stream is brx_index_set_batch's, with its pos and what, and record 11 is "\\"
    pos, what = mo.index_set(mo.CHECK_STREAM)
    assert len(mo.CHECK_STREAM) == 48 and pos == [0, 4, 14, 18, 19, 21, 23, 24, 25, 26, 30, 35, 36, 37, 44] and what == b"{:,:[,]}\n{:}\n{:"
    assert mo.record(mo.CHECK_STREAM, pos, 11) == b'"\\\\"'


NAMES = [b"id", b"text", b"user", b"tags", mo.KEYS[7], b"k", b"zz", b"i"]


def test_the_two_statements_agree_and_agree_with_json():
    """A fixed-seed generator of JSON Lines: both statements of the rule give the same members, kinds, records and flags for every
    line; where json.loads reads the line as an object (at least 90 % of them, asserted), the same names are present, a duplicate's
    LAST value is the one, a scalar's record is the bytes json.loads reads that value from and a nested value has its kind."""
    rng = np.random.default_rng(20240521)
    n_lines, applies = 0, 0
    kinds, flag_bits = set(), set()
    for _ in range(3200):
        line = mo.gen_line(rng)
        a = mo.members_boundaries(line, *mo.index_set(line), NAMES)
        b = mo.members_bytes(line, NAMES)
        assert a == b, (line, a, b)
        assert a[0] == 1
        n_lines += 1
        r = mo.agrees_with_json(line, NAMES, a[1][0], a[2][0])
        assert r is not False, (line, a)
        applies += r is True
        kinds.update(v[0] for v in a[1][0].values())
        flag_bits.add(a[2][0])
    assert n_lines >= 3000 and applies >= 0.9 * n_lines, (applies, n_lines)
    assert kinds == {mo.SCALAR, mo.OBJECT, mo.ARRAY, mo.BAD} and {0, mo.LONG_KEY, mo.ESCAPED_KEY, mo.UNBALANCED} <= flag_bits
    # whole streams (a cut line may leave a string open across the line feed, as brx_index_set_batch has it: both statements follow)
    for it in range(200):
        s = mo.gen_stream(rng, int(rng.integers(0, 30)))
        a, b = mo.FORMS["boundaries"](s, NAMES), mo.FORMS["bytes"](s, NAMES)
        assert a == b, s
        assert a[0] == mo.index_set(s)[1].count(b"\n") + 1


def test_all_steps_hold_against_a_serial_walk(tmp_path):
    """tools/member_emu.cpp: plan, sum, compose, emit and finish, lane by lane on the CPU around the real text of csrc/brx_member.h; it
    fails on a load outside a stream or at / behind n_pos, a store outside n_names * m, a slot of a line that was not written, and a
    member, a kind, a flag or a line count that differs."""
    exe = str(tmp_path / "member_emu")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "brotli-rs_amd", "csrc"),
                        os.path.join(ROOT, "tools", "member_emu.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    src = open(os.path.join(ROOT, "brotli-rs_amd", "csrc", "brx_member.h")).read()
    tile = int(re.search(r"#define\s+BRX_MB_TILE\s+(\d+)u", src).group(1))
    row = int(re.search(r"#define\s+BRX_MB_ROW\s+(\d+)u", src).group(1))
    assert r.returncode == 0 and r.stdout.startswith("OK: ") and "tiles of %d boundaries in rows of %d" % (tile, row) in r.stdout, r.stdout[-2000:]
