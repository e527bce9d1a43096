"""CPU-side checks of the parse ABI (include/brx.h): brx_parse_batch is declared and exported, its kernel is native code in the library,
the header compiles from plain C++, the argument checks that need no GPU answer in the order the contract gives, the layers above the
ABI expose the call, the two statements of THE PARSE in tests/parse_oracle.py agree with the contract's check values and with each
other, and the kernel's logic restated on the CPU (tools/parse_emu.cpp around the real text of csrc/brx_parse.h) holds against a
byte-serial walk without a load outside the arena or from a record above 64 bytes.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np

import brotli_rs_amd
import parse_oracle as po
from brotli_rs_amd import brx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {po.OK: "OK", po.INEXACT: "INEXACT", po.EMPTY: "EMPTY", po.RANGE: "RANGE", po.BAD: "BAD", po.LONG: "LONG"}


def _header():
    return open(os.path.join(ROOT, "include", "brx.h")).read()


def test_parse_batch_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    cu64p = r"const\s+uint64_t\s*\*\s*"
    assert re.search(r"int\s+brx_parse_batch\s*\(\s*brx_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*out\s*,\s*" + cu64p + r"out_off\s*,\s*" + cu64p
                     + r"len\s*,\s*uint32_t\s+n\s*,\s*uint64_t\s+span\s*,\s*" + cu64p + r"count\s*,\s*" + cu64p + r"pos_off\s*,\s*" + cu64p
                     + r"pos\s*,\s*uint64_t\s+n_pos\s*,\s*uint32_t\s+delim_len\s*,\s*uint32_t\s+flags\s*,\s*"
                     r"const\s+uint32_t\s*\*\s*sel_stream\s*,\s*" + cu64p + r"sel_rec\s*,\s*uint64_t\s+m\s*,\s*uint32_t\s+kind\s*,\s*"
                     r"uint32_t\s+scale\s*,\s*uint8_t\s+quote\s*,\s*int64_t\s*\*\s*val\s*,\s*uint8_t\s*\*\s*status\s*,\s*"
                     r"void\s*\*\s*hip_stream\s*\)\s*;", hdr)
    assert hdr.index("brx_hash_batch") < hdr.index("brx_parse_batch")  # behind brx_hash_batch
    for name, v in (("BRX_PARSE_SPACES", po.SPACES), ("BRX_PARSE_QUOTED", po.QUOTED), ("BRX_PARSE_INT", po.INT), ("BRX_PARSE_DEC", po.DEC),
                    ("BRX_PARSE_HEX", po.HEX), ("BRX_PARSE_OK", po.OK), ("BRX_PARSE_INEXACT", po.INEXACT), ("BRX_PARSE_EMPTY", po.EMPTY),
                    ("BRX_PARSE_RANGE", po.RANGE), ("BRX_PARSE_BAD", po.BAD), ("BRX_PARSE_LONG", po.LONG), ("BRX_PARSE_MAX_LEN", po.MAX_LEN),
                    ("BRX_PARSE_MAX_SCALE", 18)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, v), hdr), name
    assert (brx.PARSE_SPACES, brx.PARSE_QUOTED, brx.PARSE_INT, brx.PARSE_DEC, brx.PARSE_HEX) == (po.SPACES, po.QUOTED, po.INT, po.DEC, po.HEX)
    assert (brx.PARSE_OK, brx.PARSE_INEXACT, brx.PARSE_EMPTY, brx.PARSE_RANGE, brx.PARSE_BAD, brx.PARSE_LONG) == (0, 1, 2, 3, 4, 5)
    assert brx.PARSE_MAX_LEN == 64 and brx.PARSE_MAX_SCALE == 18
    path = brotli_rs_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    exported = set(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip())
    assert "brx_parse_batch" in exported
    assert "brx_parse_batch" in brx.EXPORTED_SYMBOLS
    assert brx.load_library().brx_parse_batch is not None
    assert b"brx_parse_kernel" in open(path, "rb").read()  # the pass is native code in the library


def test_header_compiles_from_plain_cpp():
    src = ('#include "include/brx.h"\n'
           "static_assert(BRX_PARSE_SPACES == 16u && BRX_PARSE_QUOTED == 32u && BRX_PARSE_LONG == 5u && BRX_PARSE_MAX_LEN == 64u, \"\");\n"
           "int (*f)(brx_ctx *, const uint8_t *, const uint64_t *, const uint64_t *, uint32_t, uint64_t, const uint64_t *, const uint64_t *,\n"
           "         const uint64_t *, uint64_t, uint32_t, uint32_t, const uint32_t *, const uint64_t *, uint64_t, uint32_t, uint32_t, uint8_t,\n"
           "         int64_t *, uint8_t *, void *) = brx_parse_batch;\n"
           "int main() { return f == nullptr; }\n")
    for std in ("c++11", "c++17"):
        r = subprocess.run(["g++", "-std=" + std, "-Wall", "-Werror", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_header_states_the_parse_and_its_limits():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define[^\n]*\n\s*)*int\s+brx_parse_batch", _header(), flags=re.S)
    assert m
    text = m.group(1)
    for word in ("DEVICE", "THE PARSE", "BRX_PARSE_MAX_LEN = 64", "0x20 and 0x09", "once", "T = 0", "EMPTY", "[+-]? D+",
                 "[+-]? ( D+ ( '.' D* )? | '.' D+ )", "( '0' [xX] )? H+", "No exponent", "truncated toward zero", "INT64_MAX", "INT64_MIN",
                 "RANGE wins over INEXACT", "leading zeros", "-0 is 0", "all ones", "is ever loaded",
                 "BRX_TAKE_NO_DELIM", "BRX_TAKE_TRIM_CR", "No scratch", "one launch", "Not in scope", "in this order", "floating point",
                 "exponents", "dates", "unescaping", "records above 64 bytes"):
        assert word in text, word
    flat = " ".join(text.split())
    for r, kind, scale, flags, val, status in po.CHECK:  # the check values, all of them
        if len(r) > 40 or not r or flags:
            continue  # (spelled out in words: the 64 / 65 byte ones, the empty record and the quoted table)
        v = {po.MAX: "MAX", po.MIN: "MIN", -1: "all ones"}.get(val, str(val))
        assert '"%s" %s / %s' % (r.decode(), v, NAMES[status]) in flat, r
    for word in ('(64 bytes) MAX / OK', '(65 bytes) 0 / LONG', '"" 0 / EMPTY', '[ "42"\\t] 42 / OK', '[" 42"] 0 / BAD', '["42] 0 / BAD', '["] 0 / BAD',
                 '[""] 0 / EMPTY', '[two spaces] 0 / EMPTY'):
        assert word in flat, word


def _call(lib, h, flags=0, D=1, ss=None, sr=None, m=0, kind=0, scale=0, quote=0, val=None, status=None, out_off=None, ln=None, count=None,
          pos_off=None, pos=None, n_pos=0, n=0, span=0):
    return lib.brx_parse_batch(h, None, out_off, ln, n, span, count, pos_off, pos, n_pos, D, flags, ss, sr, m, kind, scale, quote, val, status,
                               None)


def _refuser():
    lib = brx.load_library()
    fake = ctypes.create_string_buffer(1 << 16)  # never read: the checks come first (the handle is no context: a call that got past
    h = ctypes.addressof(fake)                   # the checks would not come back with these messages)
    P = ctypes.addressof(ctypes.create_string_buffer(64))  # stands for any non-NULL device pointer: never dereferenced by the host

    def refused(word, *a, **kw):
        assert _call(lib, *a, **kw) == -1, word  # BRX_ERR_INVALID_ARGUMENT
        e = lib.brx_last_error()
        assert e.startswith(b"brx_parse_batch:") and word in e, (word, e)

    return lib, h, P, refused, fake


# Each case violates its own check AND every later one it can, so that a check out of order shows.
def test_refusal_1_ctx_null():
    lib, h, P, refused, _ = _refuser()
    refused(b"ctx is NULL", None, flags=64, D=0, ss=P, m=1, kind=3, scale=19)


def test_refusal_2_unknown_flag_bits():
    lib, h, P, refused, _ = _refuser()
    for bad in (4, 8, 64, 1 << 31, 2 | 4):
        refused(b"unknown flag bits", h, flags=bad, D=0, ss=P, m=1, kind=3, scale=19)


def test_refusal_3_trim_cr_without_no_delim():
    lib, h, P, refused, _ = _refuser()
    for flags in (2, 2 | 16 | 32):
        refused(b"BRX_TAKE_TRIM_CR without", h, flags=flags, D=0, ss=P, m=1, kind=3, scale=19)


def test_refusal_4_delim_len():
    lib, h, P, refused, _ = _refuser()
    for bad in (0, 17, 1 << 31):
        refused(b"delim_len", h, flags=3 | 48, D=bad, ss=P, m=1, kind=3, scale=19)


def test_refusal_5_half_a_selection():
    lib, h, P, refused, _ = _refuser()
    refused(b"sel_stream and sel_rec", h, ss=P, m=1, kind=3, scale=19)
    refused(b"sel_stream and sel_rec", h, sr=P, m=1, kind=3, scale=19)


def test_refusal_6_kind():
    lib, h, P, refused, _ = _refuser()
    for bad in (3, 4, 1 << 31):
        refused(b"kind", h, m=1, kind=bad, scale=19)


def test_refusal_7_scale():
    lib, h, P, refused, _ = _refuser()
    refused(b"scale", h, m=1, kind=po.DEC, scale=19)
    refused(b"scale", h, m=1, kind=po.DEC, scale=1 << 31)
    refused(b"scale", h, m=1, kind=po.INT, scale=1)
    refused(b"scale", h, m=1, kind=po.HEX, scale=18)


def test_refusal_8_val_or_status_null():
    lib, h, P, refused, _ = _refuser()
    refused(b"val or status is NULL", h, m=5, n_pos=3)
    refused(b"val or status is NULL", h, m=5, n_pos=3, val=P)
    refused(b"val or status is NULL", h, m=5, n_pos=3, status=P, kind=po.DEC, scale=18)
    refused(b"val or status is NULL", h, m=0, val=P)  # (in front of the m = 0 exit)


def test_9_an_empty_selection_succeeds_without_a_launch():
    lib, h, P, refused, _ = _refuser()
    assert _call(lib, h, val=P, status=P) == 0  # whatever else is NULL
    assert _call(lib, h, flags=3 | 48, D=16, ss=P, sr=P, kind=po.DEC, scale=18, quote=34, val=P, status=P, n_pos=3, span=1 << 63) == 0


def test_refusal_10_tables_and_ranges():
    lib, h, P, refused, _ = _refuser()
    tabs = dict(out_off=P, ln=P, count=P, pos_off=P)
    for missing in tabs:
        kw = dict(tabs)
        kw[missing] = None
        refused(b"NULL table", h, m=1, val=P, status=P, n_pos=3, **kw)
    refused(b"pos is NULL with n_pos > 0", h, m=1, val=P, status=P, n_pos=3, **tabs)
    refused(b"all-records mode with n = 0", h, m=1, val=P, status=P, span=1 << 63, **tabs)
    refused(b"span out of range", h, m=1 << 62, val=P, status=P, n=1, span=1 << 63, **tabs)
    refused(b"span out of range", h, m=1, val=P, status=P, ss=P, sr=P, span=1 << 63, **tabs)
    refused(b"m out of range", h, m=1 << 62, val=P, status=P, n=1, span=64, **tabs)


def test_wrappers_expose_the_call():
    import inspect
    assert callable(brx.Context.parse_batch) and callable(brx.Context.parse_batch_device)
    sig = inspect.signature(brx.Context.parse_batch)
    assert list(sig.parameters)[1:] == ["out", "out_off", "out_len", "count", "pos_off", "pos", "sel_stream", "sel_rec", "delim_len", "keep_delim",
                                        "trim_cr", "kind", "scale", "spaces", "quote", "stream"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["keep_delim"], d["trim_cr"], d["kind"], d["scale"], d["spaces"], d["quote"], d["delim_len"]) == (False, False, "int", 0, False, None, 1)
    doc = brx.Context.parse_batch.__doc__
    for word in ("keep_delim defaults to False", "a number never contains its delimiter", "index_set_batch", "PARSE_EMPTY", "PARSE_LONG"):
        assert word in doc, word
    src = ('#include "brotli-rs_amd/host/decompressor.hpp"\n'
           "int main() { uint64_t t[4]; uint32_t s[1]; int64_t v[2]; uint8_t st[2];\n"
           "             brotli::parse_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, 1, 1, BRX_TAKE_NO_DELIM | BRX_TAKE_TRIM_CR | BRX_PARSE_SPACES |\n"
           "                                 BRX_PARSE_QUOTED, s, t, 1, BRX_PARSE_DEC, 2, '\"', v, st);\n"
           "             brotli::parse_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, 1, 2, 0, nullptr, nullptr, 2, BRX_PARSE_HEX, 0, 0, v, st, nullptr);\n"
           "             return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_check_values_of_the_contract_in_both_forms():
    assert len(po.CHECK) == 39
    for r, kind, scale, flags, val, status in po.CHECK:
        for name, f in po.FORMS.items():
            assert f(r, kind, scale, bool(flags & po.SPACES), 0x22 if flags & po.QUOTED else None) == (val, status), (name, r)
    assert len(po.CHECK[7][0]) == 64 and len(po.CHECK[8][0]) == 65


def test_the_two_forms_agree_on_random_records():
    rng = np.random.default_rng(19)
    seen = {s: 0 for s in NAMES}
    for it in range(6000):
        r = po.random_field(rng, 0x22 if it % 2 else 0x27)
        for kind, scale in ((po.INT, 0), (po.DEC, int(rng.integers(0, 19))), (po.DEC, (0, 1, 2, 9, 18)[it % 5]), (po.HEX, 0)):
            for spaces in (False, True):
                for quote in (None, 0x22, 0x27):
                    a, b = po.parse_re(r, kind, scale, spaces, quote), po.parse_fsm(r, kind, scale, spaces, quote)
                    assert a == b, (r, kind, scale, spaces, quote, a, b)
                    assert po.MIN <= a[0] <= po.MAX and (a[0] == 0 or a[1] in (po.OK, po.INEXACT, po.RANGE))
                    seen[a[1]] += 1
    assert all(v >= 500 for v in seen.values()), seen  # (a floor on the generator, not on the forms: it reaches every status)


def test_parse_take_follows_the_rule_of_take():
    """parse_take on a small arena by hand: kept delimiters are BAD, a CR is BAD unless trimmed, out-of-range entries are EMPTY."""
    arena = np.frombuffer(b"\r\r12,-3\r\n 0x1f ,\n\r", dtype=np.uint8)
    off, ln = [2], [15]
    count, pos_off, pos = po.take_oracle.index_positions(arena, off, ln, b",\n")
    assert count.tolist() == [4]
    for form in po.FORMS:
        v, s, L = po.parse_take(form, arena, off, ln, count, pos_off, pos, len(pos), 1, 0, po.INT)
        assert L.tolist() == [3, 4, 7, 1, 0] and s.tolist() == [po.BAD] * 4 + [po.EMPTY]
        v, s, L = po.parse_take(form, arena, off, ln, count, pos_off, pos, len(pos), 1, 1, po.INT)
        assert v.tolist() == [12, 0, 0, 0, 0] and s.tolist() == [po.OK, po.BAD, po.BAD, po.EMPTY, po.EMPTY]
        v, s, L = po.parse_take(form, arena, off, ln, count, pos_off, pos, len(pos), 1, 3, po.INT)
        assert v.tolist() == [12, -3, 0, 0, 0] and s.tolist() == [po.OK, po.OK, po.BAD, po.EMPTY, po.EMPTY]
        v, s, L = po.parse_take(form, arena, off, ln, count, pos_off, pos, len(pos), 1, 3 | po.SPACES, po.HEX, si=[0, 0, 1, 0], sk=[2, 0, 0, 5])
        assert v.tolist() == [31, 18, 0, 0] and s.tolist() == [po.OK, po.OK, po.EMPTY, po.EMPTY]


def test_the_header_logic_holds_against_a_serial_walk(tmp_path):
    """tools/parse_emu.cpp: brx_parse_lane lane by lane on the CPU around the real text of csrc/brx_parse.h and csrc/brx_take.h; it fails
    on any load outside [out, out + span), on a record byte loaded for an entry above 64 bytes, and on a length x phase combination
    that was not met."""
    exe = str(tmp_path / "parse_emu")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "brotli-rs_amd", "csrc"),
                        os.path.join(ROOT, "tools", "parse_emu.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK: 735 batches") and "every length 0 .. 66 at all 16 phases" in r.stdout \
        and "none outside the arena, none from a record above 64 bytes" in r.stdout, r.stdout[-2000:]
