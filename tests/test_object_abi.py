"""CPU-side checks of the object ABI (include/brx.h): brx_object_batch is declared behind brx_elements_batch and exported, its kernel is
native code in the library, the header states the rule with every check value, the argument checks that need no GPU answer in the
order the contract gives with their exact texts, the layers above the ABI expose the call, the two statements of THE RULE in
tests/object_oracle.py agree with each other, with the contract's check values and with json.loads, and the lane path and the wave
path restated on the CPU (tools/object_emu.cpp) hold against a boundary-serial walk without a load or a store outside their bounds and
with every slot written exactly once.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np

import brotli_rs_amd
import object_oracle as oo
from brotli_rs_amd import brx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "brx.h")).read()


def test_object_batch_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    u64p, cu64p, cu8p, u8p = r"uint64_t\s*\*\s*", r"const\s+uint64_t\s*\*\s*", r"const\s+uint8_t\s*\*\s*", r"uint8_t\s*\*\s*"
    cu32p = r"const\s+uint32_t\s*\*\s*"
    assert re.search(r"int\s+brx_object_batch\s*\(\s*brx_ctx\s*\*\s*ctx\s*,\s*" + cu8p + r"out\s*,\s*" + cu64p + r"out_off\s*,\s*" + cu64p
                     + r"len\s*,\s*uint32_t\s+n\s*,\s*uint64_t\s+span\s*,\s*" + cu64p + r"count\s*,\s*" + cu64p + r"pos_off\s*,\s*" + cu64p
                     + r"pos\s*,\s*" + cu8p + r"what\s*,\s*uint64_t\s+n_pos\s*,\s*" + cu32p + r"sel_stream\s*,\s*" + cu64p
                     + r"sel_rec\s*,\s*uint64_t\s+m\s*,\s*" + cu8p + r"names\s*,\s*" + cu32p + r"name_len\s*,\s*uint32_t\s+n_names\s*,\s*"
                     + u64p + r"n_members\s*,\s*" + u8p + r"status\s*,\s*" + u64p + r"end\s*,\s*uint32_t\s*\*\s*mem_stream\s*,\s*" + u64p
                     + r"mem_rec\s*,\s*" + u8p + r"mem_kind\s*,\s*" + u8p + r"obj_flags\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", hdr)
    assert hdr.index("brx_elements_batch") < hdr.index("brx_object_batch") < hdr.index("brx_stream_advance")  # directly behind it
    for name, v in (("OK", 0), ("NONE", 1), ("NOT_OBJECT", 2), ("UNCLOSED", 3), ("MISMATCH", 4)):
        assert re.search(r"#define\s+BRX_OBJECT_%s\s+%du" % (name, v), hdr), name
        assert getattr(brx, "OBJECT_" + name) == v
        assert getattr(oo, name) == v
    assert (oo.MISSING, oo.SCALAR, oo.OBJECT, oo.ARRAY, oo.BAD) == (brx.MEMBER_MISSING, brx.MEMBER_SCALAR, brx.MEMBER_OBJECT, brx.MEMBER_ARRAY,
                                                                     brx.MEMBER_BAD)
    assert (oo.LONG_KEY, oo.ESCAPED_KEY) == (brx.MEMBER_LONG_KEY, brx.MEMBER_ESCAPED_KEY)
    src = open(os.path.join(ROOT, "brotli-rs_amd", "csrc", "brx_object.h")).read()
    for name, v in (("OK", 0), ("NONE", 1), ("NOT_OBJECT", 2), ("UNCLOSED", 3), ("MISMATCH", 4)):
        assert re.search(r"#define\s+BRX_OB_%s\s+%du" % (name, v), src), name
    path = brotli_rs_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    exported = set(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip())
    assert "brx_object_batch" in exported
    assert "brx_object_batch" in brx.EXPORTED_SYMBOLS
    assert brx.load_library().brx_object_batch is not None
    assert b"brx_object_kernel" in open(path, "rb").read()  # the pass is native code in the library


def test_argtypes():
    L = brx.load_library()
    P, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    assert L.brx_object_batch.restype is ctypes.c_int
    assert L.brx_object_batch.argtypes == [P, P, P, P, U32, U64, P, P, P, P, U64, P, P, U64, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32),
                                           U32, P, P, P, P, P, P, P, P]
    assert L.brx_object_batch.argtypes[:14] == L.brx_elements_batch.argtypes[:14]  # out ... m: exactly as for brx_elements_batch


def test_header_states_the_rule_and_its_limits():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+BRX_OBJECT_OK", _header(), flags=re.S)
    assert m
    text = m.group(1)
    for word in ("DEVICE", "HOST memory", "THE RULE", "THE WALK", "A MEMBER", "VALUE", "LAST WINS", "EXTENT MODE", "BRX_OBJECT_NONE",
                 "BRX_OBJECT_NOT_OBJECT", "BRX_OBJECT_UNCLOSED", "BRX_OBJECT_MISMATCH", "BRX_OBJECT_OK", "UINT64_MAX", "neutral",
                 "BRX_TAKE_NO_DELIM", "KEY RECORD", "0x20, 0x09 and 0x0D", "bytewise", "BRX_MEMBER_MAX_KEY = 64", "BRX_MEMBER_MAX_NAMES = 8",
                 "BRX_MEMBER_MAX_NAME = 32", "column-major", "q * m + j", "n_names * m", "Not in scope", "in this order",
                 "never a load or a store", "json.loads", "launch arguments", "pretty-printed", "no synchronisation", "MISSING",
                 "BRX_MEMBER_SCALAR", "BRX_MEMBER_OBJECT", "BRX_MEMBER_ARRAY", "BRX_MEMBER_BAD", "BRX_MEMBER_LONG_KEY", "BRX_MEMBER_ESCAPED_KEY",
                 "again an opener", "brx_elements_batch", "One launch", "sel_stream[j] in every case"):
        assert word in text, word
    flat = " ".join(text.replace("*", " ").split())
    for c in oo.CHECK:  # the check values, all of them
        assert oo.header_form(*c) in flat, oo.header_form(*c)
    hdr = _header()
    member = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+BRX_MEMBER_MAX_NAMES", hdr, flags=re.S).group(1)
    elements = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+BRX_ELEMENTS_MAX_BLANK", hdr, flags=re.S).group(1)
    assert "brx_object_batch" in member and "brx_object_batch" in elements  # the extent of a nested object is no longer nobody's


def _call(lib, h, ss=None, sr=None, m=0, names=None, name_len=None, n_names=0, n_members=None, status=None, end=None, mem_stream=None,
          mem_rec=None, mem_kind=None, obj_flags=None, out_off=None, ln=None, count=None, pos_off=None, pos=None, what=None, n_pos=0, n=0, span=0):
    lens = None if name_len is None else (ctypes.c_uint32 * max(len(name_len), 1))(*name_len)
    return lib.brx_object_batch(h, None, out_off, ln, n, span, count, pos_off, pos, what, n_pos, ss, sr, m, names, lens, n_names, n_members,
                                status, end, mem_stream, mem_rec, mem_kind, obj_flags, None)


def _names(*names):
    return b"".join(x.ljust(32, b"\0") for x in names)


def test_argument_checks_that_need_no_gpu():
    """Every refusal, in the contract's order and with its exact text (the handle below is no context: a call that got past the checks
    would not come back with these messages).  Each case violates its own check AND every later one it can, so a check out of order
    shows."""
    lib = brx.load_library()
    fake = ctypes.create_string_buffer(1 << 16)  # never read: the checks come first
    h = ctypes.addressof(fake)
    P = ctypes.addressof(ctypes.create_string_buffer(64))  # stands for any non-NULL device pointer: never dereferenced by the host

    def refused(text, *a, **kw):
        assert _call(lib, *a, **kw) == -1, text  # BRX_ERR_INVALID_ARGUMENT
        assert lib.brx_last_error() == b"brx_object_batch: " + text, (text, lib.brx_last_error())

    later = dict(m=1 << 62, n=1, n_pos=1 << 62, span=1 << 63)  # violates the checks behind the m = 0 exit
    # (one of sel_stream / sel_rec, no member outputs: the later refusals in front of the m = 0 exit)
    refused(b"ctx is NULL", None, ss=P, n_names=9, **later)
    refused(b"n_names is not 0 .. 8", h, ss=P, n_names=9, **later)
    refused(b"n_names is not 0 .. 8", h, ss=P, n_names=1 << 31, names=_names(b"a"), name_len=[0], **later)
    refused(b"names or name_len is NULL with n_names > 0", h, ss=P, n_names=2, name_len=[0, 40], **later)
    refused(b"names or name_len is NULL with n_names > 0", h, ss=P, n_names=2, names=_names(b"a", b"a"), **later)
    refused(b"a name_len is not 1 .. 32", h, ss=P, n_names=2, names=_names(b"a", b"a"), name_len=[1, 0], **later)
    refused(b"a name_len is not 1 .. 32", h, ss=P, n_names=3, names=_names(b"a", b"a", b"b"), name_len=[1, 1, 33], **later)
    refused(b"a name stands twice in names", h, ss=P, n_names=2, names=_names(b"a", b"a"), name_len=[1, 1], **later)
    refused(b"a name stands twice in names", h, ss=P, n_names=3, names=_names(b"ab", b"a", b"ab"), name_len=[2, 1, 2], **later)
    two = dict(n_names=2, names=_names(b"ab", b"a"), name_len=[2, 1])  # (a prefix of a name is another name)
    refused(b"sel_stream and sel_rec go together", h, ss=P, **two, **later)
    refused(b"sel_stream and sel_rec go together", h, sr=P, **two, **later)
    refused(b"sel_stream and sel_rec go together", h, sr=P, mem_stream=P, **later)  # (extent mode with an output it must not have)
    full = dict(mem_stream=P, mem_rec=P, mem_kind=P)
    for missing in full:
        kw = dict(full)
        kw[missing] = None
        refused(b"mem_stream, mem_rec or mem_kind is NULL with n_names > 0", h, **two, **later, **kw)
    refused(b"mem_stream, mem_rec or mem_kind is NULL with n_names > 0", h, obj_flags=P, n_members=P, **two, **later)
    for given in ("mem_stream", "mem_rec", "mem_kind", "obj_flags"):
        refused(b"mem_stream, mem_rec, mem_kind or obj_flags is given in extent mode", h, **later, **{given: P})
    refused(b"mem_stream, mem_rec, mem_kind or obj_flags is given in extent mode", h, n_members=P, obj_flags=P, **later, **full)
    refused(b"n_members is NULL in extent mode", h, status=P, end=P, **later)
    # m = 0: success, no launch, whatever else is NULL; n = 0 needs no tables either
    assert _call(lib, h, n_members=P) == 0
    assert _call(lib, h, n=1, n_pos=1 << 62, span=1 << 63, **two, **full) == 0  # (with names n_members is optional)
    assert _call(lib, h, ss=P, sr=P, n=5, n_members=P, status=P, end=P) == 0
    assert _call(lib, h, n=0, **two, **full, obj_flags=P) == 0
    big = dict(n=1, n_pos=1 << 62, span=1 << 63)
    refused(b"sel_stream and sel_rec are NULL", h, m=1 << 62, **big, **two, **full)
    sel = dict(ss=P, sr=P)
    tabs = dict(out_off=P, ln=P, count=P, pos_off=P)
    for missing in tabs:
        kw = dict(tabs)
        kw[missing] = None
        refused(b"NULL table", h, m=1 << 62, **big, **two, **full, **sel, **kw)
    refused(b"pos or what is NULL with n_pos > 0", h, m=1 << 62, **big, **two, **full, **sel, **tabs)
    refused(b"pos or what is NULL with n_pos > 0", h, m=1 << 62, pos=P, **big, **two, **full, **sel, **tabs)
    refused(b"pos or what is NULL with n_pos > 0", h, m=1 << 62, what=P, **big, **two, **full, **sel, **tabs)
    refused(b"span out of range", h, m=1 << 62, pos=P, what=P, **big, **two, **full, **sel, **tabs)
    big["span"] = 64
    refused(b"m out of range", h, m=1 << 62, pos=P, what=P, **big, **two, **full, **sel, **tabs)
    refused(b"n_pos out of range", h, m=5, pos=P, what=P, **big, **two, **full, **sel, **tabs)
    # n = 0 needs no tables: behind the checks a call reaches the context (not tried here: the handle is none)
    refused(b"m out of range", h, m=1 << 62, n_members=P, **sel)
    assert (1 << 39) * 8 < 1 << 64 and ((1 << 39) + 255) // 256 > 0x7fffffff  # the bound on m keeps n_names * m in range


def test_refusals_through_the_python_wrapper():
    """Context.object_batch_device turns a refusal into BrxError with the library's text."""
    import pytest
    fake = ctypes.create_string_buffer(1 << 16)
    P = ctypes.addressof(ctypes.create_string_buffer(64))
    c = brx.Context.__new__(brx.Context)
    c._lib, c._h = brx.load_library(), None
    try:
        def refused(word, *a, **kw):
            with pytest.raises(brx.BrxError, match=r"brx_object_batch failed \(-1\): brx_object_batch: " + re.escape(word) + "$"):
                c.object_batch_device(P, P, P, 1, 1 << 63, P, P, None, None, 3, *a, **kw)

        refused("ctx is NULL", P, None, 5, [b"a"], None)
        c._h = ctypes.addressof(fake)
        refused("n_names is not 0 .. 8", P, P, 5, [b"%d" % q for q in range(9)], P)
        refused("a name_len is not 1 .. 32", P, P, 5, [b"a", b""], P)
        refused("a name_len is not 1 .. 32", P, P, 5, [b"x" * 33], P)
        refused("a name stands twice in names", P, P, 5, [b"a", b"b", b"a"], P)
        refused("sel_stream and sel_rec go together", P, None, 5, [b"a"], P)
        refused("mem_stream, mem_rec or mem_kind is NULL with n_names > 0", P, P, 5, [b"a"], P, mem_stream_ptr=P, mem_rec_ptr=P)
        refused("mem_stream, mem_rec, mem_kind or obj_flags is given in extent mode", P, P, 5, [], P, obj_flags_ptr=P)
        refused("n_members is NULL in extent mode", P, P, 5, [], None, status_ptr=P)
        refused("sel_stream and sel_rec are NULL", None, None, 5, [], P)
        refused("pos or what is NULL with n_pos > 0", P, P, 5, [], P)
        c.object_batch_device(None, None, None, 0, 0, None, None, None, None, 0, None, None, 0, [], P)  # m = 0 succeeds without a launch
        c.object_batch_device(P, P, P, 1, 1 << 63, P, P, None, None, 3, P, P, 0, [b"a", b"b"], None, None, None, P, P, P)
    finally:
        c._h = None  # (nothing to destroy)


def test_wrappers_expose_the_call():
    assert callable(brx.Context.object_batch) and callable(brx.Context.object_batch_device)
    doc = brx.Context.object_batch.__doc__
    for word in ("index_set_batch", "delims=b'{}[]:,\\n'", "member_batch", '[b"meta", b"items"]', "ss[0], sr[0]", "elements_batch", "es, er",
                 "parse_f64_batch", "sel_stream=ms[0]", "sel_rec=mr[0]", "spaces=True", "OBJECT_OK", "OBJECT_MISMATCH", "MEMBER_OBJECT",
                 "MEMBER_ARRAY", "MEMBER_MISSING", "json.loads", "extent"):
        assert word in doc, word
    src = ('#include "brotli-rs_amd/host/decompressor.hpp"\n'
           "int main() { uint64_t t[4]; uint32_t s[1]; uint8_t b[64];\n"
           "             brotli::object_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, b, 1, s, t, 1, nullptr, nullptr, 0, t);\n"
           "             brotli::object_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, b, 1, s, t, 1, b, s, 1, nullptr, b, t, s, t, b, b, nullptr);\n"
           "             return BRX_OBJECT_OK + BRX_OBJECT_NONE + BRX_OBJECT_NOT_OBJECT + BRX_OBJECT_UNCLOSED + BRX_OBJECT_MISMATCH; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read() + open(os.path.join(ROOT, "README.md")).read()
    assert text.count("brx_object_batch") >= 3
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 25." in design and "brx_object_batch" in design and "BRX_OB_LONG" in design
    build = open(os.path.join(ROOT, "brotli-rs_amd", "build.py")).read()
    assert '"brx_object.hip"' in build and '"brx_object.h"' in build


def test_check_values_of_the_contract():
    assert len(oo.CHECK) == 15
    for c in oo.CHECK:
        for f in oo.FORMS.values():
            assert f(c[0], c[2], c[1]) == oo.check_answer(c), (c[0], c[2], f)
    # r = 2 is where brx_member_batch points for "u" / "a", and a nested object member is again an opener
    s = oo.CHECK[6][0]
    pos, what = oo.index_set(s)
    assert what == b"{:{:{:},:}}"
    assert oo.object_boundaries(s, pos, what, 0, [b"a"]) == (oo.OK, 10, 1, {0: (oo.OBJECT, 2)}, 0)
    assert oo.record(s, pos, 9) == b"2" and oo.record(s, pos, 6) == b"1"
    # the names of an outer object are not seen from an inner one and the other way round
    assert oo.object_boundaries(s, pos, what, 4, [b"x", b"a"]) == (oo.OK, 6, 1, {}, 0)
    # extent mode is the same walk without names (the key flags are no output of it)
    for c in oo.CHECK:
        for f in oo.FORMS.values():
            status, end, members, found, _ = f(c[0], c[2], [])
            assert (status, end, members, found) == (c[3], c[5], c[4], {})


def test_the_two_statements_agree_and_agree_with_json():
    """A fixed-seed generator of valid JSON Lines nested two and three levels deep, with duplicate keys, keys repeated in nested values,
    arrays of objects, strings with brackets, colons, quotes and escapes, four spacing styles: both statements of the rule give the same
    answer for every boundary as an opener, and for EVERY line (none is left out) and every object in it -- found from the top by the
    rule itself, through OBJECT members and the OBJECT elements of ARRAY members -- the member count, the names present, the last of
    duplicates, the kinds and the bytes of every scalar member are json.loads's.  Broken lines (cut, a closer swapped or dropped, a
    line feed inside, a colon doubled) are held between the two statements."""
    rng = np.random.default_rng(20251021)
    stats, n_lines, n_objects, statuses, kinds = {}, 0, 0, set(), set()
    for _ in range(1500):
        line = oo.gen_line(rng)
        for f in oo.FORMS.values():
            n_objects += oo.agrees_with_json(line, f, stats)
        n_lines += 1
        for text in (line, oo.break_line(rng, line)):
            pos, what = oo.index_set(text)
            for r in range(len(pos) + 2):
                a, b = oo.object_boundaries(text, pos, what, r, oo.NAMES), oo.object_bytes(text, r, oo.NAMES)
                assert a == b, (text, r, a, b)
                statuses.add(a[0])
                kinds.update(kd for kd, _ in a[3].values())
    assert n_lines == 1500 and n_objects > 10000 and stats["scalars"] > 10000 and stats["dups"] > 1000 and stats["in_arrays"] > 1000
    assert stats["max_depth"] >= 3
    assert statuses == {oo.OK, oo.NONE, oo.NOT_OBJECT, oo.UNCLOSED, oo.MISMATCH} and kinds == {oo.SCALAR, oo.OBJECT, oo.ARRAY, oo.BAD}


def test_both_paths_hold_against_a_serial_walk(tmp_path):
    """tools/object_emu.cpp: the lane path and the wave path, lane by lane on the CPU around the real text of csrc/brx_object.h; it fails
    on a load outside a stream's boundaries that count or at / behind n_pos, an arena load outside the stream, a store at or beyond
    n_names * m, a slot that was not written exactly once, and a result that differs."""
    exe = str(tmp_path / "object_emu")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "brotli-rs_amd", "csrc"),
                        os.path.join(ROOT, "tools", "object_emu.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    src = open(os.path.join(ROOT, "brotli-rs_amd", "csrc", "brx_object.h")).read()
    units = int(re.search(r"#define\s+BRX_OB_UNITS\s+(\d+)u", src).group(1))
    assert r.returncode == 0 and r.stdout.startswith("OK: ") and "BRX_OB_LONG %d)" % (16 * units) in r.stdout, r.stdout[-2000:]
