"""CPU-side checks of the unescape ABI (include/brx.h): brx_unescape_batch is declared and exported, its kernel is native code in the
library, the header states the rule with every check value, the argument checks that need no GPU answer in the order the contract
gives, the layers above the ABI expose the call, the two statements of THE TEXT in tests/unescape_oracle.py agree with each other,
with the contract's table and with json / csv of the standard library, and the lane path and the wave path of the kernel restated on
the CPU (tools/unescape_emu.cpp) hold against a byte-serial walk without a load outside the record or a store outside the room.  No
GPU needed."""
import csv
import ctypes
import json
import os
import re
import subprocess

import numpy as np

import brotli_rs_amd
import unescape_oracle as uo
from brotli_rs_amd import brx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "brx.h")).read()


def test_unescape_batch_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    u64p, cu64p, u32 = r"uint64_t\s*\*\s*", r"const\s+uint64_t\s*\*\s*", r"uint32_t\s+"
    assert re.search(r"int\s+brx_unescape_batch\s*\(\s*brx_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*out\s*,\s*" + cu64p + r"out_off\s*,\s*"
                     + cu64p + r"len\s*,\s*uint32_t\s+n\s*,\s*uint64_t\s+span\s*,\s*" + cu64p + r"count\s*,\s*" + cu64p + r"pos_off\s*,\s*"
                     + cu64p + r"pos\s*,\s*uint64_t\s+n_pos\s*,\s*uint32_t\s+delim_len\s*,\s*uint32_t\s+flags\s*,\s*"
                     r"const\s+uint32_t\s*\*\s*sel_stream\s*,\s*" + cu64p + r"sel_rec\s*,\s*uint64_t\s+m\s*,\s*" + u32 + r"dialect\s*,\s*" + u32
                     + r"quote\s*,\s*" + u32 + r"escape\s*,\s*" + u64p + r"text_len\s*,\s*uint8_t\s*\*\s*status\s*,\s*" + cu64p
                     + r"dst_off\s*,\s*uint8_t\s*\*\s*dst\s*,\s*uint64_t\s+total\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", hdr)
    assert hdr.index("brx_parse_time_batch") < hdr.index("brx_unescape_batch") < hdr.index("brx_stream_advance")  # directly behind it
    for name, v in (("CSV", 0), ("JSON", 1), ("BACKSLASH", 2), ("OK", 0), ("BARE", 1), ("NULL", 2), ("BAD", 3)):
        assert re.search(r"#define\s+BRX_TEXT_%s\s+%du" % (name, v), hdr), name
        assert getattr(brx, "TEXT_" + name) == v
    path = brotli_rs_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    exported = set(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip())
    assert "brx_unescape_batch" in exported
    assert "brx_unescape_batch" in brx.EXPORTED_SYMBOLS
    assert brx.load_library().brx_unescape_batch is not None
    assert b"brx_unescape_kernel" in open(path, "rb").read()  # the pass is native code in the library


def test_header_states_the_rule_and_its_limits():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+BRX_TEXT_CSV", _header(), flags=re.S)
    assert m
    text = m.group(1)
    for word in ("DEVICE", "L' <= T <= L", "Not in scope", "in this order", "never loaded", "THE TEXT", "SIZE MODE", "FILL MODE", "ROOM",
                 "BRX_PARSE_SPACES", "BRX_TAKE_NO_DELIM", "BRX_TAKE_TRIM_CR", "RFC 4180", "DC00..DFFF", "EF BF BD", "inside a UTF-8 sequence",
                 "rec_len", "No scratch", "octal", "re-quoting", "quote == escape"):
        assert word in text, word
    flat = " ".join(text.replace("*", " ").split())
    for c in uo.CHECK:  # the check values, all of them
        assert uo.header_form(*c) in flat, uo.header_form(*c)


def _call(lib, h, flags=0, D=1, ss=None, sr=None, m=0, dialect=1, q=0x22, e=0x5C, text_len=None, status=None, dst_off=None, dst=None, total=0,
          out_off=None, ln=None, count=None, pos_off=None, pos=None, n_pos=0, n=0, span=0):
    return lib.brx_unescape_batch(h, None, out_off, ln, n, span, count, pos_off, pos, n_pos, D, flags, ss, sr, m, dialect, q, e, text_len,
                                  status, dst_off, dst, total, None)


def test_argument_checks_that_need_no_gpu():
    """Every refusal that needs no GPU, in the contract's order (the handle below is no context: a call that got past the checks would
    not come back with these messages).  Each case violates its own check AND every later one it can, so a check out of order shows."""
    lib = brx.load_library()
    fake = ctypes.create_string_buffer(1 << 16)  # never read: the checks come first
    h = ctypes.addressof(fake)
    P = ctypes.addressof(ctypes.create_string_buffer(64))  # stands for any non-NULL device pointer: never dereferenced by the host

    def refused(word, *a, **kw):
        assert _call(lib, *a, **kw) == -1, word  # BRX_ERR_INVALID_ARGUMENT
        err = lib.brx_last_error()
        assert err.startswith(b"brx_unescape_batch:") and word in err, (word, err)

    later = dict(dialect=3, q=256, e=256, dst_off=P, m=1)  # violates every check from the dialect on
    refused(b"ctx is NULL", None, flags=4, D=0, ss=P, **later)
    for bits in (4, 8, 32, 64, 1 << 31):  # (BRX_PARSE_QUOTED and BRX_PARSE_WORDS among them)
        refused(b"unknown flag bits", h, flags=bits | 2, D=0, ss=P, **later)
    refused(b"BRX_TAKE_TRIM_CR without", h, flags=2 | 16, D=0, ss=P, **later)
    for bad in (0, 17, 1 << 31):
        refused(b"delim_len", h, flags=3 | 16, D=bad, ss=P, **later)
    refused(b"sel_stream and sel_rec", h, ss=P, **later)
    refused(b"sel_stream and sel_rec", h, sr=P, **later)
    for bad in (3, 1 << 31):
        refused(b"dialect", h, dialect=bad, q=256, e=256, dst_off=P, m=1)
    refused(b"quote or escape", h, dialect=1, q=256, e=256, dst_off=P, m=1)
    refused(b"quote or escape", h, dialect=1, q=7, e=1 << 31, dst_off=P, m=1)
    refused(b"quote == escape", h, dialect=1, q=7, e=7, dst_off=P, m=1)
    assert _call(lib, h, dialect=0, q=7, e=7, text_len=P, status=P) == 0  # (only JSON needs them apart)
    assert _call(lib, h, dialect=2, q=7, e=7, text_len=P, status=P) == 0
    refused(b"dst_off and dst", h, dst_off=P, m=1)
    refused(b"dst_off and dst", h, dst=P, m=1)
    refused(b"NULL in size mode", h, m=5, n_pos=3)
    refused(b"NULL in size mode", h, m=5, n_pos=3, text_len=P)
    refused(b"NULL in size mode", h, m=0, status=P)  # (in front of the m = 0 exit)
    # m = 0: success, no launch, whatever else is NULL
    assert _call(lib, h, text_len=P, status=P) == 0
    assert _call(lib, h, dst_off=P, dst=P) == 0  # (fill mode needs neither)
    assert _call(lib, h, flags=3 | 16, D=16, ss=P, sr=P, dst_off=P, dst=P, n_pos=3, span=1 << 63, total=1 << 63) == 0
    tabs = dict(out_off=P, ln=P, count=P, pos_off=P)
    out = dict(text_len=P, status=P)
    for missing in tabs:
        kw = dict(tabs)
        kw[missing] = None
        refused(b"NULL table", h, m=1, n_pos=3, **out, **kw)
    refused(b"pos is NULL with n_pos > 0", h, m=1, n_pos=3, **out, **tabs)
    refused(b"all-records mode with n = 0", h, m=1, span=1 << 63, **out, **tabs)
    refused(b"span out of range", h, m=1 << 62, n=1, span=1 << 63, **out, **tabs)
    refused(b"span out of range", h, m=1, ss=P, sr=P, span=1 << 63, **out, **tabs)
    refused(b"m out of range", h, m=1 << 62, n=1, span=64, dst_off=P, dst=P, total=1 << 63, **tabs)
    refused(b"total out of range", h, m=1, n=1, span=64, dst_off=P, dst=P, total=1 << 63, **tabs)


def test_wrappers_expose_the_call():
    assert callable(brx.Context.unescape_batch) and callable(brx.Context.unescape_batch_device)
    doc = brx.Context.unescape_batch.__doc__
    for word in ("index_set_batch", "delims=b'{}[]:,\\n'", 'dialect="json"', "spaces=True", "sel_stream", "stride=S", "TEXT_BARE"):
        assert word in doc, word
    assert brx.TEXT_DIALECTS == {"csv": 0, "json": 1, "backslash": 2}
    src = ('#include "brotli-rs_amd/host/decompressor.hpp"\n'
           "int main() { uint64_t t[4]; uint32_t s[1]; uint8_t b[4];\n"
           "             brotli::unescape_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, 1, 1, BRX_TAKE_NO_DELIM | BRX_PARSE_SPACES, s, t, 1,\n"
           "                                    BRX_TEXT_JSON, '\"', '\\\\', t, b);\n"
           "             brotli::unescape_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, 1, 2, 0, nullptr, nullptr, 2, BRX_TEXT_CSV, '\"', 0,\n"
           "                                    nullptr, nullptr, t, b, 4, nullptr);\n"
           "             return BRX_TEXT_BACKSLASH + BRX_TEXT_OK + BRX_TEXT_BARE + BRX_TEXT_NULL + BRX_TEXT_BAD; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read() + open(os.path.join(ROOT, "README.md")).read()
    assert text.count("brx_unescape_batch") >= 3


def _random_records(seed, dialect, count, q=uo.QT, e=uo.ESC):
    rng = np.random.default_rng(seed)
    for it in range(count):
        yield uo.rich_record(rng, int(rng.integers(0, 48)) if it % 16 else int(rng.integers(0, 1200)), dialect, q, e,
                             rich=float(rng.uniform(0.2, 0.95)))


def test_the_two_statements_of_the_text_agree():
    for dialect in (uo.CSV, uo.JSON, uo.BACKSLASH):
        seen = set()
        for it, r in enumerate(_random_records(100 + dialect, dialect, 20000)):
            spaces = bool(it & 1)
            if it & 2:
                r = b" \t"[:it % 3] + r + b"\t  "[:it % 4]
            a, b = uo.text_serial(r, dialect, spaces=spaces), uo.text_re(r, dialect, spaces=spaces)
            assert a == b, (dialect, r, a, b)
            assert len(a[0]) <= len(r)
            seen.add(a[1])
        assert seen == ({uo.OK, uo.BARE, uo.BAD} if dialect != uo.BACKSLASH else {uo.OK, uo.NULL, uo.BAD}), (dialect, seen)
    # other quote and escape bytes, a hex digit and 'u' among them
    for q, e in ((0x27, 0x5E), (0x75, 0x5C), (0x22, 0x75), (0x39, 0x61), (0x22, 0x46), (0x62, 0x6E), (0, 0xFF)):
        for dialect in (uo.CSV, uo.JSON, uo.BACKSLASH):
            for r in _random_records(q * 256 + e, dialect, 1500, q, e):
                a, b = uo.text_serial(r, dialect, q, e), uo.text_re(r, dialect, q, e)
                assert a == b, (dialect, q, e, r, a, b)
                assert len(a[0]) <= len(r)


def test_check_values_of_the_contract():
    assert len(uo.CHECK) == 31
    for dialect, spaces, rec, text, status in uo.CHECK:
        for f in uo.FORMS.values():
            assert f(rec, dialect, spaces=spaces) == (text, status), (dialect, rec)
    assert uo.text_serial(b' "x"\t', uo.JSON) == (b' "x"\t', uo.BARE)  # (without BRX_PARSE_SPACES)
    assert uo.text_serial(b'"\\u0000"', uo.JSON) == (b"\0", uo.OK)


def test_json_agrees_with_the_standard_library():
    """Every record that json.loads accepts as a str that encodes to UTF-8 is OK with that encoding as its text; every other record
    that starts with the quote is BAD.  (strict=False: raw control bytes pass unchecked here as well.)"""
    n_ok = n_bad = 0
    for r in _random_records(7, uo.JSON, 30000):
        if not r.startswith(b'"'):
            assert uo.text_serial(r, uo.JSON) == (r, uo.BARE)
            continue
        try:
            v = json.loads(r.decode("ascii"), strict=False)
            want = v.encode("utf-8") if isinstance(v, str) else None
        except (ValueError, UnicodeEncodeError):
            want = None
        text, status = uo.text_serial(r, uo.JSON)
        if want is None:
            assert status == uo.BAD, r
            n_bad += 1
        else:
            assert (text, status) == (want, uo.OK), r
            n_ok += 1
    assert n_ok > 2000 and n_bad > 2000, (n_ok, n_bad)


def test_csv_agrees_with_the_standard_library():
    n_ok = 0
    for r in _random_records(8, uo.CSV, 30000):
        text, status = uo.text_serial(r, uo.CSV)
        if status == uo.OK:
            assert next(csv.reader([r.decode("ascii")], strict=True)) == [text.decode("ascii")], r
            n_ok += 1
    assert n_ok > 2000, n_ok


def test_both_paths_hold_against_a_serial_walk(tmp_path):
    """tools/unescape_emu.cpp: the lane path, the wave path and the serial path, lane by lane on the CPU around the real text of
    csrc/brx_unescape.h; it fails on a load outside the record, a store outside the room or at or behind total, a destination byte
    written twice, a text that differs, and on a length x source phase x destination phase combination that was not met."""
    exe = str(tmp_path / "unescape_emu")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "brotli-rs_amd", "csrc"),
                        os.path.join(ROOT, "tools", "unescape_emu.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    long_ = int(re.search(r"#define\s+BRX_TEXT_LONG\s+(\d+)u", open(os.path.join(ROOT, "brotli-rs_amd", "csrc", "brx_unescape.h")).read()).group(1))
    assert r.returncode == 0 and r.stdout.startswith("OK: ") and "lengths 0 .. %d at 16 x 16 phases" % (long_ + 2048) in r.stdout, r.stdout[-2000:]
