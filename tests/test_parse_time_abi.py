"""CPU-side checks of the time parse ABI (include/brx.h): brx_parse_time_batch is declared and exported, its kernel is native code in
the library, the header compiles from plain C++, the argument checks that need no GPU answer in the order the contract gives, the
layers above the ABI expose the call, the two statements of THE PARSE, TIME in tests/parse_time_oracle.py agree with the contract's
check values and with each other on a corpus that meets every status that a kind can give, and the kernel's logic restated on the CPU
(tools/parse_time_emu.cpp around the real text of csrc/brx_parse_time.h) holds against the oracle without a load outside the arena or
from a record above 64 bytes.  No GPU needed."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import brotli_rs_amd
import parse_time_oracle as to
import take_oracle
from brotli_rs_amd import brx
from brotli_rs_amd.brx import TIME_DATE, TIME_MAX_SCALE, TIME_NO_ZONE, TIME_STAMP, TIME_TIME  # noqa: F401  (without the call nothing here runs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QT = 0x22


def _header():
    return open(os.path.join(ROOT, "include", "brx.h")).read()


def _comment_of(name):
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define[^\n]*\n\s*)*int\s+%s\b" % name, _header(), flags=re.S)
    assert m, name
    return m.group(1)


def test_parse_time_batch_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    cu64p = r"const\s+uint64_t\s*\*\s*"
    assert re.search(r"int\s+brx_parse_time_batch\s*\(\s*brx_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*out\s*,\s*" + cu64p + r"out_off\s*,\s*" + cu64p
                     + r"len\s*,\s*uint32_t\s+n\s*,\s*uint64_t\s+span\s*,\s*" + cu64p + r"count\s*,\s*" + cu64p + r"pos_off\s*,\s*" + cu64p
                     + r"pos\s*,\s*uint64_t\s+n_pos\s*,\s*uint32_t\s+delim_len\s*,\s*uint32_t\s+flags\s*,\s*"
                     r"const\s+uint32_t\s*\*\s*sel_stream\s*,\s*" + cu64p + r"sel_rec\s*,\s*uint64_t\s+m\s*,\s*"
                     r"uint32_t\s+kind\s*,\s*uint32_t\s+scale\s*,\s*uint8_t\s+quote\s*,\s*"
                     r"int64_t\s*\*\s*val\s*,\s*uint8_t\s*\*\s*status\s*,\s*int16_t\s*\*\s*zone\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", hdr)
    # behind the prototype of brx_parse_f64_batch, in front of the stream facade; the defines in front of the prototype
    assert hdr.index("int brx_parse_f64_batch") < hdr.index("BRX_TIME_DATE") < hdr.index("int brx_parse_time_batch") < hdr.index("brx_stream_new")
    for name, v in (("BRX_TIME_DATE", "0u"), ("BRX_TIME_TIME", "1u"), ("BRX_TIME_STAMP", "2u"), ("BRX_TIME_MAX_SCALE", "9u"),
                    ("BRX_TIME_NO_ZONE", r"\(-32768\)")):
        assert re.search(r"#define\s+%s\s+%s(?!\w)" % (name, v), hdr), name
    assert (brx.TIME_DATE, brx.TIME_TIME, brx.TIME_STAMP, brx.TIME_MAX_SCALE, brx.TIME_NO_ZONE) == (0, 1, 2, 9, -32768)
    assert (to.DATE, to.TIME, to.STAMP, to.MAX_SCALE, to.NO_ZONE) == (0, 1, 2, 9, -32768)
    path = brotli_rs_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    exported = set(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip())
    assert "brx_parse_time_batch" in exported
    assert "brx_parse_time_batch" in brx.EXPORTED_SYMBOLS and "brx_parse_time_batch" not in brx.EXPORTED_SYMBOLS_NUMBERED
    assert brx.load_library().brx_parse_time_batch is not None
    assert b"brx_parse_time_kernel" in open(path, "rb").read()  # the pass is native code in the library


def test_header_compiles_from_plain_cpp():
    src = ('#include "include/brx.h"\n'
           "static_assert(BRX_TIME_DATE == 0u && BRX_TIME_TIME == 1u && BRX_TIME_STAMP == 2u && BRX_TIME_MAX_SCALE == 9u, \"\");\n"
           "static_assert(BRX_TIME_NO_ZONE == -32768 && (int16_t)BRX_TIME_NO_ZONE == BRX_TIME_NO_ZONE && BRX_PARSE_MAX_LEN == 64u, \"\");\n"
           "int (*f)(brx_ctx *, const uint8_t *, const uint64_t *, const uint64_t *, uint32_t, uint64_t, const uint64_t *, const uint64_t *,\n"
           "         const uint64_t *, uint64_t, uint32_t, uint32_t, const uint32_t *, const uint64_t *, uint64_t, uint32_t, uint32_t, uint8_t,\n"
           "         int64_t *, uint8_t *, int16_t *, void *) = brx_parse_time_batch;\n"
           "int main() { return f == nullptr; }\n")
    for std in ("c++11", "c++17"):
        r = subprocess.run(["g++", "-std=" + std, "-Wall", "-Werror", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def _spelled(r, val, status, zone):
    v = {to.MAX: "MAX", to.MIN: "MIN"}.get(val, str(val))
    return '"%s" %s / %s' % (r.decode(), v, to.NAMES[status])


def test_header_states_the_parse_and_its_check_values():
    text = _comment_of("brx_parse_time_batch")
    for word in ("DEVICE", "THE PARSE, TIME", "BRX_PARSE_MAX_LEN", "0x20 and 0x09", "EMPTY", "date = DDDD '-' DD '-' DD",
                 "time = DD ':' DD ( ':' DD ( [.,] D+ )? )?", "zone = [Zz] | [+-] DD ':' DD | [+-] DDDD | [+-] DD",
                 "STAMP: date ( [Tt ] time zone? )?", "A date alone is midnight", "logging", "proleptic Gregorian",
                 "y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)", "year 0000 is leap", "no 24:00", "no second 60", "east of UTC", "-00:00",
                 "rounded toward minus infinity", "RANGE wins over INEXACT", "Only scales 8 and 9", "-1439 .. 1439", "BRX_TIME_NO_ZONE",
                 "may be NULL", "is ever loaded", "BRX_TAKE_NO_DELIM", "BRX_TAKE_TRIM_CR", "BRX_PARSE_WORDS", "no new status value", "No scratch",
                 "one launch", "in this order", "Not in scope", "week dates", "ordinal dates", "month names", "12-hour", "zone names", "DST",
                 "leap seconds", "durations", "intervals", "records above 64 bytes", "kind above 2", "scale above 9"):
        assert word in text, word
    flat = " ".join(text.split())
    for r, kind, scale, flags, val, status, zone in to.CHECK:
        if len(r) > 40 or flags:
            continue  # (spelled out in words below)
        at = flat.index("%s%s:" % (to.KIND_NAMES[kind], "" if kind == to.DATE else ", scale %d" % scale))
        nxt = min([flat.index(w, at + 1) for w in ("TIME, scale", "STAMP, scale", "hip_stream NULL") if flat.find(w, at + 1) > 0])
        assert _spelled(r, val, status, zone) in flat[at:nxt], (r, kind, scale)
    for word in ('"2024-03-10T07:08:09." + 38 zeros + "+05:30" (64 bytes) 1710034689000 / OK', "the same with 39 zeros (65 bytes) 0 / LONG",
                 '"2024-03-10T07:08:09.123" + 40 zeros + "1" (64 bytes) 1710054489123 / INEXACT', "zone BRX_TIME_NO_ZONE",
                 '-0800" 1710083289 / OK, zone -480', '+01" 1710050889 / OK, zone 60', '-00:00" 1710054489 / OK, zone 0',
                 '+05:30" 1710034689500000 / OK, zone 330',
                 '[ "2024-03-10T07:08:09Z"\\t] 1710054489 / OK', '[" 2024-03-10"] 0 / BAD', '[""] 0 / EMPTY'):
        assert word in flat, word
    # the comments of the two sibling calls keep their words; the first one points here
    sib = _comment_of("brx_parse_batch")
    for word in ("No exponent", "Not in scope", "floating point", "exponents", "brx_parse_f64_batch", "dates and times", "brx_parse_time_batch"):
        assert word in sib, word


def _call(lib, h, flags=0, D=1, ss=None, sr=None, m=0, kind=2, scale=0, quote=0, val=None, status=None, zone=None, out_off=None, ln=None,
          count=None, pos_off=None, pos=None, n_pos=0, n=0, span=0):
    return lib.brx_parse_time_batch(h, None, out_off, ln, n, span, count, pos_off, pos, n_pos, D, flags, ss, sr, m, kind, scale, quote, val,
                                    status, zone, None)


def _refuser():
    lib = brx.load_library()
    fake = ctypes.create_string_buffer(1 << 16)  # never read: the checks come first (the handle is no context: a call that got past
    h = ctypes.addressof(fake)                   # the checks would not come back with these messages)
    keep = ctypes.create_string_buffer(64)
    P = ctypes.addressof(keep)  # stands for any non-NULL device pointer: never dereferenced by the host

    def refused(word, *a, **kw):
        assert _call(lib, *a, **kw) == -1, word  # BRX_ERR_INVALID_ARGUMENT
        e = lib.brx_last_error()
        assert e.startswith(b"brx_parse_time_batch:") and word in e, (word, e)

    return lib, h, P, refused, (fake, keep)


# Each case violates its own check AND every later one it can, so that a check out of order shows.
def test_refusal_1_ctx_null():
    lib, h, P, refused, _ = _refuser()
    refused(b"ctx is NULL", None, flags=128, D=0, ss=P, m=1, kind=3, scale=10)


def test_refusal_2_unknown_flag_bits():
    lib, h, P, refused, _ = _refuser()
    for bad in (4, 8, 64, 128, 1 << 31, 2 | 4, 2 | 64, 64 | 256):
        refused(b"unknown flag bits", h, flags=bad, D=0, ss=P, m=1, kind=3, scale=10)


def test_refusal_3_trim_cr_without_no_delim():
    lib, h, P, refused, _ = _refuser()
    for flags in (2, 2 | 16 | 32):
        refused(b"BRX_TAKE_TRIM_CR without", h, flags=flags, D=0, ss=P, m=1, kind=3, scale=10)


def test_refusal_4_delim_len():
    lib, h, P, refused, _ = _refuser()
    for bad in (0, 17, 1 << 31):
        refused(b"delim_len", h, flags=3 | 48, D=bad, ss=P, m=1, kind=3, scale=10)


def test_refusal_5_half_a_selection():
    lib, h, P, refused, _ = _refuser()
    refused(b"sel_stream and sel_rec", h, ss=P, m=1, kind=3, scale=10)
    refused(b"sel_stream and sel_rec", h, sr=P, m=1, kind=3, scale=10)


def test_refusal_6_kind():
    lib, h, P, refused, _ = _refuser()
    for bad in (3, 4, 1 << 31):
        refused(b"kind is not", h, m=1, kind=bad, scale=10)


def test_refusal_7_scale():
    lib, h, P, refused, _ = _refuser()
    for kind, bad in ((1, 10), (2, 10), (2, 18), (2, 1 << 31), (0, 1), (0, 9), (0, 10)):
        refused(b"scale is not", h, m=1, kind=kind, scale=bad)


def test_refusal_8_val_or_status_null():
    lib, h, P, refused, _ = _refuser()
    refused(b"val or status is NULL", h, m=5, n_pos=3)
    refused(b"val or status is NULL", h, m=5, n_pos=3, val=P, zone=P)
    refused(b"val or status is NULL", h, m=5, n_pos=3, status=P, kind=1, scale=9)
    refused(b"val or status is NULL", h, m=0, val=P)  # (in front of the m = 0 exit)


def test_9_an_empty_selection_succeeds_without_a_launch():
    lib, h, P, refused, _ = _refuser()
    assert _call(lib, h, val=P, status=P) == 0  # whatever else is NULL, zone included
    assert _call(lib, h, flags=3 | 48, D=16, ss=P, sr=P, kind=1, scale=9, quote=34, val=P, status=P, zone=P, n_pos=3, span=1 << 63) == 0


def test_refusal_10_tables_and_ranges():
    lib, h, P, refused, _ = _refuser()
    tabs = dict(out_off=P, ln=P, count=P, pos_off=P)
    for missing in tabs:
        kw = dict(tabs)
        kw[missing] = None
        refused(b"NULL table", h, m=1, val=P, status=P, n_pos=3, span=1 << 63, **kw)
    refused(b"pos is NULL with n_pos > 0", h, m=1, val=P, status=P, n_pos=3, span=1 << 63, **tabs)
    refused(b"all-records mode with n = 0", h, m=1, val=P, status=P, span=1 << 63, **tabs)
    refused(b"span out of range", h, m=1 << 62, val=P, status=P, n=1, span=1 << 63, **tabs)
    refused(b"span out of range", h, m=1, val=P, status=P, ss=P, sr=P, span=1 << 63, **tabs)
    refused(b"m out of range", h, m=1 << 62, val=P, status=P, zone=P, n=1, span=64, **tabs)


def test_the_sibling_calls_still_refuse_what_they_refused():
    lib = brx.load_library()
    fake = ctypes.create_string_buffer(1 << 16)
    h = ctypes.addressof(fake)
    keep = ctypes.create_string_buffer(64)
    P = ctypes.addressof(keep)
    pb = lambda flags=0, kind=0, scale=0, val=None, status=None: lib.brx_parse_batch(
        h, None, None, None, 0, 0, None, None, None, 0, 1, flags, None, None, 0, kind, scale, 0, val, status, None)
    assert pb(flags=64) == -1 and b"brx_parse_batch: unknown flag bits" in lib.brx_last_error()
    assert pb(kind=3) == -1 and b"brx_parse_batch: kind is not" in lib.brx_last_error()
    assert pb(kind=2, scale=1) == -1 and b"brx_parse_batch: scale is not" in lib.brx_last_error()  # kind 2 is HEX there, not a timestamp
    assert pb(kind=1, scale=19) == -1 and b"brx_parse_batch: scale is not" in lib.brx_last_error()
    assert pb(kind=2) == -1 and b"brx_parse_batch: val or status is NULL" in lib.brx_last_error()
    assert pb(kind=2, val=P, status=P) == 0  # HEX with an empty selection
    pf = lambda flags=0, val=None, status=None: lib.brx_parse_f64_batch(
        h, None, None, None, 0, 0, None, None, None, 0, 1, flags, None, None, 0, 0, val, status, None)
    assert pf(flags=128) == -1 and b"brx_parse_f64_batch: unknown flag bits" in lib.brx_last_error()
    assert pf(flags=64) == -1 and b"brx_parse_f64_batch: val or status is NULL" in lib.brx_last_error()  # WORDS is its own flag still
    assert pf(flags=64, val=P, status=P) == 0


def test_wrappers_expose_the_call():
    assert callable(brx.Context.parse_time_batch) and callable(brx.Context.parse_time_batch_device)
    sig = inspect.signature(brx.Context.parse_time_batch)
    assert list(sig.parameters)[1:] == ["out", "out_off", "out_len", "count", "pos_off", "pos", "sel_stream", "sel_rec", "delim_len", "keep_delim",
                                        "trim_cr", "spaces", "quote", "kind", "unit", "zones", "stream"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["sel_stream"], d["sel_rec"], d["delim_len"], d["keep_delim"], d["trim_cr"], d["spaces"], d["quote"], d["kind"], d["unit"],
            d["zones"], d["stream"]) == (None, None, 1, False, False, False, None, "stamp", "s", False, None)
    assert brx.TIME_KINDS == {"date": 0, "time": 1, "stamp": 2} and brx.TIME_UNITS == {"s": 0, "ms": 3, "us": 6, "ns": 9}
    doc = brx.Context.parse_time_batch.__doc__
    for word in ("torch.int64", "torch.uint8", "torch.int16", "datetime64[ns]", "zones=True", "TIME_NO_ZONE", "index_set_batch", '"ms"'):
        assert word in doc, word
    dev = list(inspect.signature(brx.Context.parse_time_batch_device).parameters)
    assert dev[-6:] == ["scale", "quote", "val_ptr", "status_ptr", "zone_ptr", "hip_stream"]
    src = ('#include "brotli-rs_amd/host/decompressor.hpp"\n'
           "int main() { uint64_t t[4]; uint32_t s[1]; int64_t v[2]; uint8_t st[2]; int16_t z[2];\n"
           "             brotli::parse_time_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, 1, 1, BRX_TAKE_NO_DELIM | BRX_TAKE_TRIM_CR | BRX_PARSE_SPACES |\n"
           "                                      BRX_PARSE_QUOTED, s, t, 1, BRX_TIME_STAMP, 9, '\"', v, st);\n"
           "             brotli::parse_time_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, 1, 2, 0, nullptr, nullptr, 2, BRX_TIME_DATE, 0, 0, v, st, z,\n"
           "                                      nullptr);\n"
           "             return z[0] == BRX_TIME_NO_ZONE; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_check_values_of_the_contract_in_both_forms():
    assert len(to.CHECK) == 72
    for r, kind, scale, flags, val, status, zone in to.CHECK:
        for name, f in to.FORMS.items():
            assert f(r, kind, scale, bool(flags & to.SPACES), QT if flags & to.QUOTED else None) == (val, status, zone), (name, r)
    assert sorted(set(len(c[0]) for c in to.CHECK if len(c[0]) > 40)) == [64, 65]
    # the values that numpy's datetime64 can state are numpy's
    for r, kind, scale, flags, val, status, zone in to.CHECK:
        if status == to.OK and not flags and kind != to.TIME and r[:4] != b"0000" and len(r) < 40 and scale in (0, 3, 6, 9):
            unit = {0: "D" if kind == to.DATE else "s", 3: "ms", 6: "us", 9: "ns"}[scale]
            text = re.sub(rb"[Zz]$|[+-]\d\d(:?\d\d)?$", b"", r.replace(b",", b".")) if kind == to.STAMP and len(r) > 10 else r
            naive = int(np.datetime64(text.decode().replace("t", "T"), unit).astype(np.int64))
            assert naive - (0 if zone == to.NO_ZONE else zone * 60 * 10 ** scale) == val, r


@pytest.fixture(scope="module")
def corpus():
    """Fixed seed: per kind 4000 fields (well-formed, mutated, wrapped in blanks and quotes, junk, empty, stretched beyond 64 bytes), the
    check values' records and the stamps around the 64-bit bounds."""
    rng = np.random.default_rng(21)
    c = [to.random_field(rng, kind, QT) for kind in (to.DATE, to.TIME, to.STAMP) for _ in range(4000)]
    return c + [x[0] for x in to.CHECK] + [r for s in (8, 9) for r, _ in to.range_edges(s)]


def test_the_two_forms_agree_on_the_corpus(corpus):
    seen = {(k, s): 0 for k in to.KIND_NAMES for s in to.NAMES}
    for r in corpus + [b"0" * 65, b"2024-03-10T07:08:09." + b"1" * 46]:
        for kind in to.KIND_NAMES:
            for scale in ((0,) if kind == to.DATE else (0, 3, 6, 8, 9)):
                for spaces in (False, True):
                    for quote in (None, QT):
                        a, b = to.parse_re(r, kind, scale, spaces, quote), to.parse_fsm(r, kind, scale, spaces, quote)
                        assert a == b, (r, kind, scale, spaces, quote, a, b)
                        assert a[1] in (to.OK, to.INEXACT, to.RANGE) or a[0] == 0, (r, a)
                        assert a[2] == to.NO_ZONE or (a[1] in (to.OK, to.INEXACT) and kind == to.STAMP and -1439 <= a[2] <= 1439), (r, a)
                        seen[(kind, a[1])] += 1
    # every status that a kind can give was met: a date has no fraction and no scale, a time of day stays below 86400 * 10^9
    cannot = {(to.DATE, to.INEXACT), (to.DATE, to.RANGE), (to.TIME, to.RANGE)}
    assert all((v >= 20) != (k in cannot) for k, v in seen.items()), seen
    assert all(seen[k] == 0 for k in cannot)
    # the range edges: at both scales both sides of a bound were met, and a zone moves a stamp across it
    for scale in (8, 9):
        e = to.range_edges(scale)
        st = [x[1] for _, x in e]
        assert st.count(to.RANGE) >= 6 and st.count(to.OK) >= 10, (scale, st)
    wall = b"2262-04-11T23:47:16.854775808"
    assert to.parse_re(wall + b"Z", to.STAMP, 9)[1] == to.RANGE and to.parse_re(wall + b"+00:01", to.STAMP, 9)[1:] == (to.OK, 1)
    assert to.parse_re(b"2262-04-11T23:47:16.854775807-00:01", to.STAMP, 9)[1] == to.RANGE


# ---- the emulator: the corpus placed as records of whole calls ---------------------------------------------------------------------
MAGIC = 0x454D49545F585242
TAKE_FLAGS = (0, 1, 3)        # the three BRX_TAKE flag combinations
PARSE_FLAGS = (0, 16, 32, 48)
KIND_SCALE = ((2, 3), (2, 0), (2, 9), (0, 0), (1, 6), (2, 8), (1, 0), (2, 6))


def _write_call(f, phase, arena, off, ln, count, pos_off, pos, n_pos, D, flags, quote, sel, m, kind, scale):
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    if sel is None:
        si = sk = None
    else:
        si, sk = np.asarray(sel[0], dtype=np.int64), np.asarray(sel[1], dtype=np.int64)
        m = len(si)
    src, L = take_oracle.take_vec(arena, off, ln, count, pos_off, pos, n_pos, D, flags & 3, si, sk, m)
    val, status, zone = to.parse_records("re", arena, src, L, kind, scale, bool(flags & to.SPACES), quote if flags & to.QUOTED else None)
    u = lambda a: np.asarray(a, dtype=np.int64).astype(np.uint64)
    np.array([MAGIC, phase, len(arena), len(ln), len(pos), n_pos, D, flags, quote, sel is not None, m, kind, scale], dtype=np.uint64).tofile(f)
    padded = np.zeros((len(arena) + 7) // 8 * 8, dtype=np.uint8)
    padded[:len(arena)] = arena
    padded.tofile(f)
    for a in (off, ln, count, pos_off, pos):
        u(a).tofile(f)
    if sel is not None:
        u(si).tofile(f)
        u(sk).tofile(f)
    want = np.stack([u(src), u(L), u(val), u(status), u(zone)], axis=1)
    want.tofile(f)
    return status, L


def _streams(rng, records, D, cr):
    """One stream of the records, each followed by D line feeds (so the trailing record is empty), and its positions."""
    s, pos = b"", []
    for r in records:
        s += r + (b"\r" if cr and rng.integers(0, 4) == 0 else b"")
        pos.append(len(s))
        s += b"\n" * D
    return s, pos


def test_the_header_logic_holds_against_the_oracle(tmp_path, corpus):
    """tools/parse_time_emu.cpp: brx_parse_time_lane lane by lane on the CPU around the real text of csrc/brx_parse_time.h,
    csrc/brx_parse.h and csrc/brx_take.h, over the corpus placed as records: every length 0 .. 66 at all 16 source phases, records on the
    arena's first and last byte, arenas of 1 .. 40 bytes, both selection modes, the three BRX_TAKE flag combinations, delim_len 1, 2
    and 16, stale positions.  It fails on the first difference from the oracle, on any load outside [out, out + span) and on a record
    byte loaded for an entry above 64 bytes."""
    rng = np.random.default_rng(22)
    corpus = [r for r in corpus if b"\n" not in r]
    path = str(tmp_path / "calls.bin")
    seen, calls = set(), 0
    with open(path, "wb") as f:
        # PART 1: one stream that is the whole arena, records of every length 0 .. 67 in order, the arena at each phase: the first
        # record starts on the arena's first byte; without a trailing delimiter the last one ends on its last
        for it in range(96):
            recs = [to.stamp_of_length(rng, L) for L in range(65)] + [(to.random_date(rng) + b"T" + to.random_time(rng, 50))[:L] for L in (65, 66, 67)]
            s, pos = _streams(rng, recs, 1, False)
            s, pos = s[:-1], pos[:-1]  # the 67-byte record is the stream's last, up to the arena's last byte
            flags = TAKE_FLAGS[(it // 16) % 3] | PARSE_FLAGS[it % 4]
            sel = ([0] * 68, list(range(67, -1, -1))) if it % 2 else None
            kind, scale = KIND_SCALE[(it // 4) % 8] if it % 3 else (2, it % 10)
            st, L = _write_call(f, it % 16, np.frombuffer(s, dtype=np.uint8), [0], [len(s)], [len(pos)], [0], pos, len(pos), 1, flags, QT, sel, 68,
                                kind, scale)
            seen.update(st.tolist())
            calls += 1
        # PART 2: the corpus as the lines of streams in slots with slack, D in {1, 2, 16}, CRs, stale positions
        order = rng.permutation(len(corpus))
        at, it = 0, 0
        while at < len(order):
            D, tf = (1, 2, 16)[it % 3], TAKE_FLAGS[(it // 3) % 3]
            pairs, stale = (it // 9) % 2 == 1, (it // 18) % 4 == 3
            flags = tf | PARSE_FLAGS[int(rng.integers(0, 4))]
            kind, scale = KIND_SCALE[int(rng.integers(0, 8))]
            n = int(rng.integers(1, 5))
            arena, off, ln, count, pos_off, pos = b"", [], [], [], [], []
            for i in range(n):
                k = int(rng.integers(0, 40))
                s, p = _streams(rng, [corpus[j] for j in order[at:at + k]], D, tf == 3)
                at += k
                if rng.integers(0, 2) and p:
                    s, p = s[:-D], p[:-1]  # no trailing delimiter: the last record ends the stream
                off.append(len(arena)); ln.append(len(s)); count.append(len(p)); pos_off.append(len(pos))
                pos += p
                arena += s + (b"\r7"[int(rng.integers(0, 2)):][:1] * int(rng.integers(0, 20)) if i + 1 < n else b"")
            if not arena:
                arena = b"7"
            n_pos = len(pos)
            if stale:
                pos = [int(rng.integers(0, 1000)) if rng.integers(0, 4) == 0 else p for p in pos]
                n_pos = int(rng.integers(0, len(pos) + 1)) if rng.integers(0, 2) else n_pos
                count = [c + int(rng.integers(0, 3)) for c in count]
            m = sum(count) + n + (int(rng.integers(0, 4)) if stale else 0)
            sel = None
            if pairs:
                si = rng.integers(0, n, 60)
                sk = np.array([int(rng.integers(0, count[i] + 1)) for i in si])
                wild = rng.integers(0, 25, 60) == 0
                si, sk = np.where(wild, si + n, si), np.where(np.roll(wild, 1), sk + np.array(count)[si % n] + 1, sk)
                sel = (si, sk)
            st, L = _write_call(f, int(rng.integers(0, 16)), np.frombuffer(arena, dtype=np.uint8), off, ln, count, pos_off, pos, n_pos, D, flags, QT,
                                sel, m, kind, scale)
            seen.update(st.tolist())
            calls += 1
            it += 1
        # PART 3: arenas of 1 .. 40 bytes that are one record (the byte-by-byte fetch), at every phase, and as two records
        for size in range(1, 41):
            for rep in range(4):
                a = np.frombuffer(to.stamp_of_length(rng, size), dtype=np.uint8)
                st, L = _write_call(f, (size * 4 + rep * 5) % 16, a, [0], [size], [0], [0], [], 0, 1, TAKE_FLAGS[rep % 3] | PARSE_FLAGS[rep], QT,
                                    ([0], [0]) if rep == 3 else None, 1, 2, (3, 0, 9, 6)[rep])
                assert L.tolist() == [size]
                seen.update(st.tolist())
                calls += 1
            if size >= 3:
                cut = int(rng.integers(0, size - 1))
                r = bytearray(to.stamp_of_length(rng, size))
                r[cut] = 0x0A
                st, L = _write_call(f, size % 16, np.frombuffer(bytes(r), dtype=np.uint8), [0], [size], [1], [0], [cut], 1, 1, 1, QT, None, 2, 2, 3)
                assert L.tolist() == [cut, size - cut - 1]
                calls += 1
    assert seen == set(to.NAMES), seen
    exe = str(tmp_path / "parse_time_emu")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "brotli-rs_amd", "csrc"),
                        os.path.join(ROOT, "tools", "parse_time_emu.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "--full", path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK: %d calls (" % calls) \
        and int(re.search(r"\((\d+) in arenas of at most 40 bytes\)", r.stdout).group(1)) >= 198 \
        and " 0 (length, phase) pairs not met" in r.stdout \
        and "none outside the arena, none from a record above 64 bytes" in r.stdout, r.stdout[-2000:]
    if os.environ.get("BRX_KEEP_EMU_CALLS"):  # for a run of the emulator by hand (a sanitized build of it, say)
        import shutil
        shutil.copy(path, os.environ["BRX_KEEP_EMU_CALLS"])
