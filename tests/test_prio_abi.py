"""CPU-side checks of BRX_OPTION_PRIO_SHIFT (include/brx.h): the option's number, its name on the Python side and the range check of
brx_ctx_set_option, which needs no device -- a value outside 0 .. 31 is refused before the context is looked at.  No GPU needed."""
import re
import os

import pytest

from brotli_rs_amd import brx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1  # BRX_ERR_INVALID_ARGUMENT


def test_option_is_declared_and_named():
    hdr = open(os.path.join(ROOT, "include", "brx.h")).read()
    assert re.search(r"BRX_OPTION_PRIO_SHIFT\s*=\s*16\b", hdr)
    assert re.search(r"#define\s+BRX_ERR_INVALID_ARGUMENT\s+\(?-1\)?|BRX_ERR_INVALID_ARGUMENT\s*=\s*-1", hdr)
    assert brx.OPTIONS["prio_shift"] == 16


@pytest.mark.parametrize("value", [-1, 32, 33, 1 << 20, -(1 << 40), 1 << 40])
def test_out_of_range_is_a_library_error(value):
    lib = brx.load_library()
    assert lib.brx_ctx_set_option(None, brx.OPTIONS["prio_shift"], value) == INVALID
    assert b"prio shift is 0 .. 31" in lib.brx_last_error()


@pytest.mark.parametrize("value", [0, 14, 31])
def test_in_range_gets_as_far_as_the_context(value):
    lib = brx.load_library()
    assert lib.brx_ctx_set_option(None, brx.OPTIONS["prio_shift"], value) == INVALID
    assert b"ctx is NULL" in lib.brx_last_error()
