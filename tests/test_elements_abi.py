"""CPU-side checks of the elements ABI (include/brx.h): brx_elements_batch is declared behind brx_member_batch and exported, its kernel is
native code in the library, the header states the rule with every check value, the argument checks that need no GPU answer in the
order the contract gives, the layers above the ABI expose the call, the two statements of THE RULE in tests/elements_oracle.py agree
with each other, with the contract's check values and with json.loads, and the lane path and the wave path restated on the CPU
(tools/elements_emu.cpp) hold against a boundary-serial walk without a load or a store outside their bounds.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np

import brotli_rs_amd
import elements_oracle as eo
from brotli_rs_amd import brx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "brx.h")).read()


def test_elements_batch_is_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    u64p, cu64p, cu8p, u8p = r"uint64_t\s*\*\s*", r"const\s+uint64_t\s*\*\s*", r"const\s+uint8_t\s*\*\s*", r"uint8_t\s*\*\s*"
    assert re.search(r"int\s+brx_elements_batch\s*\(\s*brx_ctx\s*\*\s*ctx\s*,\s*" + cu8p + r"out\s*,\s*" + cu64p + r"out_off\s*,\s*" + cu64p
                     + r"len\s*,\s*uint32_t\s+n\s*,\s*uint64_t\s+span\s*,\s*" + cu64p + r"count\s*,\s*" + cu64p + r"pos_off\s*,\s*" + cu64p
                     + r"pos\s*,\s*" + cu8p + r"what\s*,\s*uint64_t\s+n_pos\s*,\s*const\s+uint32_t\s*\*\s*sel_stream\s*,\s*" + cu64p
                     + r"sel_rec\s*,\s*uint64_t\s+m\s*,\s*" + u64p + r"n_elem\s*,\s*" + u8p + r"status\s*,\s*" + u64p + r"end\s*,\s*" + cu64p
                     + r"el_off\s*,\s*uint64_t\s+total\s*,\s*uint32_t\s*\*\s*el_stream\s*,\s*" + u64p + r"el_rec\s*,\s*" + u8p
                     + r"el_kind\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", hdr)
    assert hdr.index("brx_member_batch") < hdr.index("brx_elements_batch") < hdr.index("brx_stream_advance")  # directly behind it
    for name, v in (("OK", 0), ("NONE", 1), ("NOT_ARRAY", 2), ("UNCLOSED", 3), ("MISMATCH", 4), ("MAX_BLANK", 64)):
        assert re.search(r"#define\s+BRX_ELEMENTS_%s\s+%du" % (name, v), hdr), name
        assert getattr(brx, "ELEMENTS_" + name) == v
        assert getattr(eo, name) == v
    assert (eo.SCALAR, eo.OBJECT, eo.ARRAY, eo.BAD) == (brx.MEMBER_SCALAR, brx.MEMBER_OBJECT, brx.MEMBER_ARRAY, brx.MEMBER_BAD)
    path = brotli_rs_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    exported = set(ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip())
    assert "brx_elements_batch" in exported
    assert "brx_elements_batch" in brx.EXPORTED_SYMBOLS
    assert brx.load_library().brx_elements_batch is not None
    assert b"brx_elements_kernel" in open(path, "rb").read()  # the pass is native code in the library


def test_header_states_the_rule_and_its_limits():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+BRX_ELEMENTS_MAX_BLANK", _header(), flags=re.S)
    assert m
    text = m.group(1)
    for word in ("DEVICE", "THE RULE", "THE WALK", "AN ELEMENT", "EMPTY ARRAY", "BRX_ELEMENTS_NONE", "BRX_ELEMENTS_NOT_ARRAY",
                 "BRX_ELEMENTS_UNCLOSED", "BRX_ELEMENTS_MISMATCH", "BRX_ELEMENTS_OK", "UINT64_MAX", "neutral", "BRX_TAKE_NO_DELIM",
                 "0x20, 0x09 and 0x0D", "BRX_ELEMENTS_MAX_BLANK = 64", "COUNT MODE", "FILL MODE", "the room of j", "Not in scope",
                 "in this order", "never a load or a store", "pretty-printed", "nested", "no synchronisation", "MISSING", "EMPTY",
                 "BRX_MEMBER_SCALAR", "BRX_MEMBER_OBJECT", "BRX_MEMBER_ARRAY", "BRX_MEMBER_BAD", "a second call", "paths", "One launch"):
        assert word in text, word
    flat = " ".join(text.replace("*", " ").split())
    for c in eo.CHECK:  # the check values, all of them
        assert eo.header_form(*c) in flat, eo.header_form(*c)
    member = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+BRX_MEMBER_MAX_NAMES", _header(), flags=re.S).group(1)
    assert "brx_elements_batch" in member  # the extent of a nested array is no longer nobody's


def _call(lib, h, ss=None, sr=None, m=0, n_elem=None, status=None, end=None, el_off=None, total=0, el_stream=None, el_rec=None, el_kind=None,
          out_off=None, ln=None, count=None, pos_off=None, pos=None, what=None, n_pos=0, n=0, span=0):
    return lib.brx_elements_batch(h, None, out_off, ln, n, span, count, pos_off, pos, what, n_pos, ss, sr, m, n_elem, status, end, el_off, total,
                                  el_stream, el_rec, el_kind, None)


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
        assert err.startswith(b"brx_elements_batch:") and word in err, (word, err)

    later = dict(m=1 << 62, n=1, n_pos=1 << 62, span=1 << 63, total=1 << 62)  # violates the checks behind the m = 0 exit
    refused(b"ctx is NULL", None, ss=P, el_off=P, **later)
    refused(b"sel_stream and sel_rec go together", h, ss=P, el_off=P, **later)
    refused(b"sel_stream and sel_rec go together", h, sr=P, el_off=P, **later)
    full = dict(el_off=P, el_stream=P, el_rec=P, el_kind=P)
    for missing in full:
        kw = dict(full)
        kw[missing] = None
        refused(b"el_off, el_stream, el_rec and el_kind go together", h, **later, **kw)
        refused(b"el_off, el_stream, el_rec and el_kind go together", h, **later, **{missing: P})
    refused(b"n_elem is NULL in count mode", h, status=P, end=P, **later)
    # m = 0: success, no launch, whatever else is NULL
    assert _call(lib, h, n_elem=P) == 0
    assert _call(lib, h, n=1, n_pos=1 << 62, span=1 << 63, total=1 << 62, **full) == 0  # (fill mode needs no n_elem)
    assert _call(lib, h, ss=P, sr=P, n=5, n_elem=P, status=P, end=P) == 0
    big = dict(n=1, n_pos=1 << 62, span=1 << 63, total=1 << 62)
    refused(b"sel_stream and sel_rec are NULL", h, m=1 << 62, **big, **full)
    sel = dict(ss=P, sr=P)
    tabs = dict(out_off=P, ln=P, count=P, pos_off=P)
    for missing in tabs:
        kw = dict(tabs)
        kw[missing] = None
        refused(b"NULL table", h, m=1 << 62, **big, **full, **sel, **kw)
    refused(b"pos or what is NULL with n_pos > 0", h, m=1 << 62, **big, **full, **sel, **tabs)
    refused(b"pos or what is NULL with n_pos > 0", h, m=1 << 62, pos=P, **big, **full, **sel, **tabs)
    refused(b"pos or what is NULL with n_pos > 0", h, m=1 << 62, what=P, **big, **full, **sel, **tabs)
    refused(b"span out of range", h, m=1 << 62, pos=P, what=P, **big, **full, **sel, **tabs)
    big["span"] = 64
    refused(b"m out of range", h, m=1 << 62, pos=P, what=P, **big, **full, **sel, **tabs)
    refused(b"n_pos out of range", h, m=5, pos=P, what=P, **big, **full, **sel, **tabs)
    big["n_pos"] = 3
    refused(b"total out of range", h, m=5, pos=P, what=P, **big, **full, **sel, **tabs)
    # n = 0 needs no tables: behind the checks a call reaches the context (not tried here: the handle is none)
    refused(b"m out of range", h, m=1 << 62, n_elem=P, **sel)


def test_refusals_through_the_python_wrapper():
    """Context.elements_batch_device turns a refusal into BrxError with the library's text."""
    import pytest
    fake = ctypes.create_string_buffer(1 << 16)
    P = ctypes.addressof(ctypes.create_string_buffer(64))
    c = brx.Context.__new__(brx.Context)
    c._lib, c._h = brx.load_library(), None
    try:
        def refused(word, *a, **kw):
            with pytest.raises(brx.BrxError, match=r"brx_elements_batch failed \(-1\): brx_elements_batch: .*" + re.escape(word)):
                c.elements_batch_device(P, P, P, 1, 1 << 63, P, P, None, None, 3, *a, **kw)

        refused("ctx is NULL", P, None, 5, None, el_off_ptr=P)
        c._h = ctypes.addressof(fake)
        refused("sel_stream and sel_rec go together", P, None, 5, None, el_off_ptr=P)
        refused("go together", P, P, 5, None, el_off_ptr=P)
        refused("go together", P, P, 5, P, el_off_ptr=P, el_stream_ptr=P, el_rec_ptr=P)
        refused("n_elem is NULL in count mode", P, P, 5, None, status_ptr=P)
        refused("sel_stream and sel_rec are NULL", None, None, 5, P)
        refused("pos or what is NULL with n_pos > 0", P, P, 5, P)
        c.elements_batch_device(None, None, None, 0, 0, None, None, None, None, 0, None, None, 0, P)  # m = 0 succeeds without a launch
        c.elements_batch_device(P, P, P, 1, 1 << 63, P, P, None, None, 3, P, P, 0, None, None, None, P, 7, P, P, P)
    finally:
        c._h = None  # (nothing to destroy)


def test_wrappers_expose_the_call():
    assert callable(brx.Context.elements_batch) and callable(brx.Context.elements_batch_device)
    doc = brx.Context.elements_batch.__doc__
    for word in ("index_set_batch", "delims=b'{}[]:,\\n'", "member_batch", '[b"emb"]', "ss[0], sr[0]", "parse_f64_batch", "sel_stream=el_stream",
                 "sel_rec=el_rec", "spaces=True", "val.view(M, D)", "ELEMENTS_OK", "ELEMENTS_MISMATCH", "MEMBER_ARRAY", "PARSE_EMPTY"):
        assert word in doc, word
    src = ('#include "brotli-rs_amd/host/decompressor.hpp"\n'
           "int main() { uint64_t t[4]; uint32_t s[1]; uint8_t b[64];\n"
           "             brotli::elements_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, b, 1, s, t, 1, t);\n"
           "             brotli::elements_batch(nullptr, nullptr, t, t, 1, 0, t, t, t, b, 1, s, t, 1, nullptr, b, t, t, 1, s, t, b, nullptr);\n"
           "             return BRX_ELEMENTS_OK + BRX_ELEMENTS_NONE + BRX_ELEMENTS_NOT_ARRAY + BRX_ELEMENTS_UNCLOSED + BRX_ELEMENTS_MISMATCH; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read() + open(os.path.join(ROOT, "README.md")).read()
    assert text.count("brx_elements_batch") >= 3
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 24." in design and "brx_elements_batch" in design and "BRX_EL_LONG" in design


def test_check_values_of_the_contract():
    assert len(eo.CHECK) == 14
    for stream, r, status, els, end in eo.CHECK:
        for f in eo.FORMS.values():
            assert f(stream, r) == (status, end, els), (stream, f)
    # r = 2 is where brx_member_batch points for "a", and a nested array element is again an opener
    s = eo.CHECK[7][0]
    pos, what = eo.index_set(s)
    assert eo.opener_of(s, pos, what, b"a") == 2 and what == b"{:[[,],{:[]},]}"
    assert eo.elements_boundaries(s, pos, what, 3) == (eo.OK, 5, [(4, eo.SCALAR), (5, eo.SCALAR)])
    assert eo.elements_boundaries(s, pos, what, 9) == (eo.OK, 10, [(10, eo.SCALAR)])
    assert eo.record(s, pos, 13) == b"4" and eo.record(eo.CHECK[8][0], eo.index_set(eo.CHECK[8][0])[0], 3) == b'"],["'


def test_the_two_statements_agree_and_agree_with_json():
    """A fixed-seed generator of valid JSON Lines with an array of 0 .. 8 values under "arr", nested to depth 3, strings with brackets,
    commas, quotes and escapes, three spacing styles: both statements of the rule give the same status, end and elements, and for
    EVERY line (none is left out) the count, the kinds and the bytes of every scalar element are json.loads's.  Broken lines (cut,
    a closer swapped or dropped, a line feed inside) are held between the two statements, with every boundary as an opener."""
    rng = np.random.default_rng(20241021)
    n_lines = scalars = 0
    sizes, kinds, statuses = set(), set(), set()
    for _ in range(4000):
        line, arr = eo.gen_line(rng)
        pos, what = eo.index_set(line)
        r = eo.opener_of(line, pos, what)
        a, b = eo.elements_boundaries(line, pos, what, r), eo.elements_bytes(line, r)
        assert a == b, (line, a, b)
        ok, k = eo.agrees_with_json(line, arr, a[0], a[2])
        assert ok, (line, a)
        assert a[1] < len(pos) and what[a[1]:a[1] + 1] == b"]"
        n_lines, scalars = n_lines + 1, scalars + k
        sizes.add(len(arr))
        kinds.update(kd for _, kd in a[2])
        broken = eo.break_line(rng, line)
        pos, what = eo.index_set(broken)
        for r in range(len(pos) + 2):
            a, b = eo.elements_boundaries(broken, pos, what, r), eo.elements_bytes(broken, r)
            assert a == b, (broken, r, a, b)
            statuses.add(a[0])
    assert n_lines == 4000 and scalars > 10000 and sizes == set(range(9)) and kinds == {eo.SCALAR, eo.OBJECT, eo.ARRAY}
    assert statuses == {eo.OK, eo.NONE, eo.NOT_ARRAY, eo.UNCLOSED, eo.MISMATCH}


def test_both_paths_hold_against_a_serial_walk(tmp_path):
    """tools/elements_emu.cpp: the lane path and the wave path, lane by lane on the CPU around the real text of csrc/brx_elements.h; it
    fails on a load outside a stream's boundaries that count or at / behind n_pos, an arena load outside the stream, a store outside
    an entry's room or at / beyond total, an element that was not stored, a slot stored that holds none, and a result that differs."""
    exe = str(tmp_path / "elements_emu")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "brotli-rs_amd", "csrc"),
                        os.path.join(ROOT, "tools", "elements_emu.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    src = open(os.path.join(ROOT, "brotli-rs_amd", "csrc", "brx_elements.h")).read()
    units = int(re.search(r"#define\s+BRX_EL_UNITS\s+(\d+)u", src).group(1))
    assert r.returncode == 0 and r.stdout.startswith("OK: ") and "BRX_EL_LONG %d)" % (16 * units) in r.stdout, r.stdout[-2000:]
