"""Every refusal of the five boundary calls (brx_index_batch, brx_index_quoted_batch, brx_index_escaped_batch, brx_index_set_batch,
brx_find_batch), in the order each call tests them, with the exact text brx_last_error() gives: one table per call.  A row changes
the arguments of a call that would succeed (n = 0) so that exactly one refusal applies; the rows behind each table break two rules at
once and name the one that must answer, which pins the order.  The handle is no context, as in tests/test_index_escaped_abi.py: a
call that got past the checks to HIP would not come back with these messages.  No GPU needed."""
import ctypes

import pytest

from brotli_rs_amd import brx

INVAL = -1  # BRX_ERR_INVALID_ARGUMENT
NO_QUOTE, NO_ESCAPE = 1, 2  # BRX_INDEX_NO_QUOTE, BRX_INDEX_NO_ESCAPE

_fake = ctypes.create_string_buffer(1 << 16)  # never read: the checks come first
H = ctypes.addressof(_fake)
_buf = ctypes.create_string_buffer(64)
P = ctypes.addressof(_buf)  # any non-NULL table or result pointer: never read or written either

# the arguments of each call in the order of include/brx.h, with values under which the call succeeds without a launch (n = 0)
CALLS = {
    "brx_index_batch": dict(ctx=H, delim=10, out=None, out_off=None, len=None, n=0, span=0, count=P, pos_off=None, pos=None, total=0,
                            hip_stream=None),
    "brx_index_quoted_batch": dict(ctx=H, delim=10, quote=34, out=None, out_off=None, len=None, n=0, span=0, count=P, open=None,
                                   pos_off=None, pos=None, total=0, hip_stream=None),
    "brx_index_escaped_batch": dict(ctx=H, delim=10, quote=34, escape=92, flags=0, out=None, out_off=None, len=None, n=0, span=0, count=P,
                                    open=None, pos_off=None, pos=None, total=0, hip_stream=None),
    "brx_index_set_batch": dict(ctx=H, delims=b",\n", n_delims=2, quote=34, escape=92, flags=0, out=None, out_off=None, len=None, n=0,
                                span=0, count=P, open=None, pos_off=None, pos=None, what=None, total=0, hip_stream=None),
    "brx_find_batch": dict(ctx=H, needle=b"\r\n", needle_len=2, out=None, out_off=None, len=None, n=0, span=0, count=P, pos_off=None,
                           pos=None, total=0, hip_stream=None),
}

# what the five share, in their order: behind a call's own checks
POS_A = (dict(pos_off=P), "pos_off and pos go together")
POS_B = (dict(pos=P), "pos_off and pos go together")
COUNT = (dict(count=None), "count is NULL in count mode")
TABLE_A = (dict(n=1, len=P), "NULL table")
TABLE_B = (dict(n=1, out_off=P), "NULL table")
SPAN = (dict(n=1, out_off=P, len=P, span=1 << 63), "span out of range")
SHARED = [POS_A, POS_B, COUNT, TABLE_A, TABLE_B, SPAN]

# per call: every refusal in the order the call tests them (several rows for a refusal with several ways in)
REFUSALS = {
    "brx_index_batch": [(dict(ctx=None), "ctx is NULL")] + SHARED,
    "brx_index_quoted_batch": [
        (dict(ctx=None), "ctx is NULL"),
        (dict(quote=10), "delim and quote are the same byte"),
    ] + SHARED,
    "brx_index_escaped_batch": [
        (dict(ctx=None), "ctx is NULL"),
        (dict(flags=2), "unknown flag bits"),
        (dict(flags=0x80000000), "unknown flag bits"),
        (dict(delim=92), "delim and escape are the same byte"),
        (dict(delim=92, flags=NO_QUOTE), "delim and escape are the same byte"),
        (dict(quote=10), "delim and quote are the same byte"),
        (dict(quote=92), "quote and escape are the same byte"),
    ] + SHARED,
    "brx_index_set_batch": [
        (dict(ctx=None), "ctx is NULL"),
        (dict(flags=4), "unknown flag bits"),
        (dict(delims=None), "delims is NULL"),
        (dict(n_delims=0), "n_delims must be 1 .. 8 (delims)"),
        (dict(delims=b"123456789", n_delims=9), "n_delims must be 1 .. 8 (delims)"),
        (dict(delims=b",\n,", n_delims=3), "a byte stands twice in delims"),
        (dict(escape=0x2C), "escape is one of delims"),
        (dict(quote=10), "quote is one of delims"),
        (dict(quote=92), "quote and escape are the same byte"),
        POS_A,
        POS_B,
        (dict(what=P), "what is given without pos"),
        COUNT,
        TABLE_A,
        TABLE_B,
        SPAN,
    ],
    "brx_find_batch": [
        (dict(ctx=None), "ctx is NULL"),
        (dict(needle=None), "needle is NULL"),
        (dict(needle_len=0), "needle_len is not 1 .. 16"),
        (dict(needle=b"0123456789abcdefg", needle_len=17), "needle_len is not 1 .. 16"),
    ] + SHARED,
}

# two rules broken at once: the earlier one in the call's order answers
ORDER = {
    "brx_index_batch": [
        (dict(ctx=None, pos_off=P, count=None), "ctx is NULL"),  # first in the order
        (dict(pos_off=P, count=None), "pos_off and pos go together"),
        (dict(count=None, n=1), "count is NULL in count mode"),  # the modes before the tables
        (dict(n=1, span=1 << 63), "NULL table"),
    ],
    "brx_index_quoted_batch": [
        (dict(ctx=None, quote=10), "ctx is NULL"),
        (dict(quote=10, pos_off=P), "delim and quote are the same byte"),  # the bytes before pos_off / pos
        (dict(pos=P, count=None, n=1), "pos_off and pos go together"),
        (dict(n=1, span=1 << 63), "NULL table"),
    ],
    "brx_index_escaped_batch": [
        (dict(ctx=None, delim=10, quote=10, escape=10, flags=2), "ctx is NULL"),  # first in the order
        (dict(delim=92, quote=92, flags=3), "unknown flag bits"),  # flags before the bytes
        (dict(delim=92, quote=92), "delim and escape are the same byte"),
        (dict(quote=10, escape=10), "delim and escape are the same byte"),  # the escape before the quote
        (dict(quote=10, count=None, pos_off=P), "delim and quote are the same byte"),  # the bytes before pos_off / pos
        (dict(quote=92, pos=P), "quote and escape are the same byte"),
        (dict(pos_off=P, count=None), "pos_off and pos go together"),
        (dict(count=None, n=1), "count is NULL in count mode"),
        (dict(n=1, span=1 << 63), "NULL table"),
    ],
    "brx_index_set_batch": [
        (dict(ctx=None, flags=4, delims=None), "ctx is NULL"),
        (dict(flags=8, delims=None), "unknown flag bits"),  # flags before the set
        (dict(delims=None, n_delims=0), "delims is NULL"),
        (dict(delims=b",,3456789", n_delims=9), "n_delims must be 1 .. 8 (delims)"),  # the size before the bytes
        (dict(delims=b",,", escape=0x2C), "a byte stands twice in delims"),
        (dict(escape=0x2C, quote=10), "escape is one of delims"),  # the escape before the quote
        (dict(quote=10, pos_off=P), "quote is one of delims"),
        (dict(quote=92, pos_off=P), "quote and escape are the same byte"),  # the bytes before pos_off / pos
        (dict(pos_off=P, what=P), "pos_off and pos go together"),  # `what` without `pos` stands behind pos_off / pos ...
        (dict(what=P, count=None), "what is given without pos"),  # ... and in front of count
        (dict(what=P, n=1), "what is given without pos"),
        (dict(count=None, n=1), "count is NULL in count mode"),
        (dict(n=1, span=1 << 63), "NULL table"),
    ],
    "brx_find_batch": [
        (dict(ctx=None, needle=None), "ctx is NULL"),
        (dict(needle=None, needle_len=0), "needle is NULL"),
        (dict(needle_len=17, pos_off=P), "needle_len is not 1 .. 16"),  # the needle before pos_off / pos
        (dict(pos=P, count=None), "pos_off and pos go together"),
        (dict(count=None, n=1), "count is NULL in count mode"),
        (dict(n=1, span=1 << 63), "NULL table"),
    ],
}

# not refused: a quote or an escape that is switched off may be any byte, and fill mode needs no count (n = 0: success without a launch)
ACCEPTED = {
    "brx_index_batch": [dict(count=None, pos_off=P, pos=P)],
    "brx_index_quoted_batch": [dict(count=None, pos_off=P, pos=P)],
    "brx_index_escaped_batch": [dict(quote=10, flags=NO_QUOTE), dict(quote=92, flags=NO_QUOTE), dict(count=None, pos_off=P, pos=P)],
    "brx_index_set_batch": [dict(quote=10, flags=NO_QUOTE), dict(escape=10, flags=NO_ESCAPE), dict(quote=92, flags=NO_QUOTE),
                            dict(quote=92, escape=92, flags=NO_ESCAPE), dict(count=None, pos_off=P, pos=P, what=P),
                            dict(count=None, pos_off=P, pos=P)],
    "brx_find_batch": [dict(count=None, pos_off=P, pos=P)],
}


def _call(lib, name, change):
    args = dict(CALLS[name])
    assert set(change) <= set(args), change
    args.update(change)
    return getattr(lib, name)(*args.values())


@pytest.mark.parametrize("name", sorted(CALLS))
def test_every_refusal_in_order_with_its_text(name):
    lib = brx.load_library()
    assert _call(lib, name, {}) == 0  # the unchanged arguments pass: every row below is refused for its change alone
    for table in (REFUSALS[name], ORDER[name]):
        for change, what in table:
            assert _call(lib, name, change) == INVAL, (name, change)
            assert lib.brx_last_error().decode() == "%s: %s" % (name, what), (name, change)
    for change in ACCEPTED[name]:
        assert _call(lib, name, change) == 0, (name, change, lib.brx_last_error())


def test_the_tables_cover_the_shared_refusals_of_every_call():
    """the six shared texts stand in every call's table, in one order, behind the call's own"""
    shared = [what for _, what in SHARED]
    for name, table in REFUSALS.items():
        texts = [what for _, what in table if what in shared]
        assert texts == shared, name
        own = [what for _, what in table if what not in shared and what != "what is given without pos"]
        assert own == [what for _, what in table][:len(own)] and own[0] == "ctx is NULL", name
