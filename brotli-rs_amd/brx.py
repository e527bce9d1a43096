"""ctypes binding of libbrx.so (include/brx.h) + a `Decompressor` that mirrors the reference's only public
item, `brotli::Decompressor<R: Read>` (reference src/lib.rs:377-410, 2173-2193).

Plumbing only: every decode goes through the C ABI into the gfx950 kernels.  If the library or a GPU is
missing this module FAILS LOUDLY (BrxError); there is no CPU fallback anywhere in the product path.
"""
import collections
import contextlib
import ctypes
import io
import os

import numpy as np

from .build import LIB_PATH, build_library

MEM_HOST = 0
MEM_DEVICE = 1
OPT_TIMING = 2
OPT_ORDER = 4
GEN_SWITCHES = 8
GEN_ADAPTIVE = 16

OK = 0
OUTPUT_TOO_SMALL = 25
REF_PANIC = 26

DIGEST_KINDS = {"crc32": 1, "crc32c": 2}  # BRX_DIGEST_*
INDEX_NO_QUOTE = 1  # BRX_INDEX_NO_QUOTE
INDEX_NO_ESCAPE = 2  # BRX_INDEX_NO_ESCAPE (brx_index_set_batch only)
TAKE_NO_DELIM = 1  # BRX_TAKE_NO_DELIM
TAKE_TRIM_CR = 2  # BRX_TAKE_TRIM_CR (only with TAKE_NO_DELIM)
PARSE_SPACES = 16  # BRX_PARSE_SPACES (brx_parse_batch only, in the same flags word)
PARSE_QUOTED = 32  # BRX_PARSE_QUOTED
PARSE_INT, PARSE_DEC, PARSE_HEX = 0, 1, 2  # BRX_PARSE_INT / _DEC / _HEX
PARSE_KINDS = {"int": PARSE_INT, "dec": PARSE_DEC, "hex": PARSE_HEX}
PARSE_OK, PARSE_INEXACT, PARSE_EMPTY, PARSE_RANGE, PARSE_BAD, PARSE_LONG = 0, 1, 2, 3, 4, 5  # BRX_PARSE_OK ... (the status byte)
PARSE_MAX_LEN = 64  # BRX_PARSE_MAX_LEN
PARSE_MAX_SCALE = 18  # BRX_PARSE_MAX_SCALE
PARSE_WORDS = 64  # BRX_PARSE_WORDS (brx_parse_f64_batch only)
PARSE_HARD = 6  # BRX_PARSE_HARD (brx_parse_f64_batch only: val or the next double away from zero)
TIME_DATE, TIME_TIME, TIME_STAMP = 0, 1, 2  # BRX_TIME_DATE / _TIME / _STAMP (brx_parse_time_batch)
TIME_KINDS = {"date": TIME_DATE, "time": TIME_TIME, "stamp": TIME_STAMP}
TIME_UNITS = {"s": 0, "ms": 3, "us": 6, "ns": 9}  # unit -> scale
TIME_MAX_SCALE = 9  # BRX_TIME_MAX_SCALE
TIME_NO_ZONE = -32768  # BRX_TIME_NO_ZONE
TEXT_CSV, TEXT_JSON, TEXT_BACKSLASH = 0, 1, 2  # BRX_TEXT_CSV / _JSON / _BACKSLASH (brx_unescape_batch)
TEXT_DIALECTS = {"csv": TEXT_CSV, "json": TEXT_JSON, "backslash": TEXT_BACKSLASH}
TEXT_OK, TEXT_BARE, TEXT_NULL, TEXT_BAD = 0, 1, 2, 3  # BRX_TEXT_OK ... (the status byte)
MEMBER_MAX_NAMES, MEMBER_MAX_NAME, MEMBER_MAX_KEY = 8, 32, 64  # BRX_MEMBER_MAX_NAMES ... (brx_member_batch)
MEMBER_MISSING, MEMBER_SCALAR, MEMBER_OBJECT, MEMBER_ARRAY, MEMBER_BAD = 0, 1, 2, 3, 4  # BRX_MEMBER_MISSING ... (the kind byte)
MEMBER_LONG_KEY, MEMBER_ESCAPED_KEY, MEMBER_UNBALANCED = 1, 2, 4  # BRX_MEMBER_LONG_KEY ... (the bits of line_flags)
ELEMENTS_OK, ELEMENTS_NONE, ELEMENTS_NOT_ARRAY, ELEMENTS_UNCLOSED, ELEMENTS_MISMATCH = 0, 1, 2, 3, 4  # BRX_ELEMENTS_OK ... (brx_elements_batch)
ELEMENTS_MAX_BLANK = 64  # BRX_ELEMENTS_MAX_BLANK
OBJECT_OK, OBJECT_NONE, OBJECT_NOT_OBJECT, OBJECT_UNCLOSED, OBJECT_MISMATCH = 0, 1, 2, 3, 4  # BRX_OBJECT_OK ... (brx_object_batch)


class BrxError(RuntimeError):
    pass


class _Opts(ctypes.Structure):
    _fields_ = [("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("hip_stream", ctypes.c_void_p)]


class _NodeOpts(ctypes.Structure):  # brx_node_opts
    _fields_ = [("flags", ctypes.c_uint32), ("deal", ctypes.c_uint32), ("use_gpus", ctypes.c_int32), ("root", ctypes.c_int32),
                ("hip_stream", ctypes.c_void_p)]


_lib = None


def load_library():
    """dlopen libbrx.so.  torch is imported first on purpose: its bundled libamdhip64 has the same SONAME
    as the system one, and loading torch first makes both share ONE HIP runtime so device pointers of torch
    tensors are valid inside libbrx."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401
    except Exception:  # torch is optional for the binding itself
        pass
    path = build_library()
    if not os.path.exists(path):
        raise BrxError("libbrx.so is missing (%s): build it with __graft_entry__.build()" % path)
    L = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    L.brx_ctx_create.restype = ctypes.c_int
    L.brx_ctx_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
    L.brx_ctx_set_option.restype = ctypes.c_int
    L.brx_ctx_set_option.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int64]
    L.brx_ctx_destroy.restype = None
    L.brx_ctx_destroy.argtypes = [ctypes.c_void_p]
    L.brx_decode_batch.restype = ctypes.c_int
    L.brx_decode_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.POINTER(_Opts)]
    L.brx_generate_batch.restype = ctypes.c_int
    L.brx_generate_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                     ctypes.POINTER(_Opts)]
    L.brx_compact_batch.restype = ctypes.c_int
    L.brx_compact_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    L.brx_digest_batch.restype = ctypes.c_int
    L.brx_digest_batch.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.brx_index_batch.restype = ctypes.c_int
    L.brx_index_batch.argtypes = [ctypes.c_void_p, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                  ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    L.brx_index_quoted_batch.restype = ctypes.c_int
    L.brx_index_quoted_batch.argtypes = [ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_uint64, ctypes.c_void_p]
    L.brx_index_escaped_batch.restype = ctypes.c_int
    L.brx_index_escaped_batch.argtypes = [ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    L.brx_index_set_batch.restype = ctypes.c_int
    L.brx_index_set_batch.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint32,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    L.brx_find_batch.restype = ctypes.c_int
    L.brx_find_batch.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                 ctypes.c_void_p]
    # the record calls: ctx, then out, out_off, len, n, span, count, pos_off, pos, n_pos, delim_len, flags, sel_stream, sel_rec, m
    P, U32, U64, U8 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint8
    rec = [P, P, P, P, U32, U64, P, P, P, U64, U32, U32, P, P, U64]
    for name, own in (("brx_take_batch", [P, P, P, U64, P]), ("brx_hash_batch", [U64, P, P, P]), ("brx_parse_batch", [U32, U32, U8, P, P, P]),
                      ("brx_parse_f64_batch", [U8, P, P, P]), ("brx_parse_time_batch", [U32, U32, U8, P, P, P, P]),
                      ("brx_unescape_batch", [U32, U32, U32, P, P, P, P, U64, P])):
        getattr(L, name).restype = ctypes.c_int
        getattr(L, name).argtypes = rec + own
    L.brx_member_batch.restype = ctypes.c_int
    L.brx_member_batch.argtypes = [P, P, P, P, U32, U64, P, P, P, P, U64, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), U32, P, P, U64,
                                   P, P, P, P, P]
    L.brx_elements_batch.restype = ctypes.c_int
    L.brx_elements_batch.argtypes = [P, P, P, P, U32, U64, P, P, P, P, U64, P, P, U64, P, P, P, P, U64, P, P, P, P]
    L.brx_object_batch.restype = ctypes.c_int
    L.brx_object_batch.argtypes = [P, P, P, P, U32, U64, P, P, P, P, U64, P, P, U64, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), U32,
                                   P, P, P, P, P, P, P, P]
    L.brx_status_str.restype = ctypes.c_char_p
    L.brx_status_str.argtypes = [ctypes.c_int32]
    L.brx_last_error.restype = ctypes.c_char_p
    L.brx_last_timing.restype = ctypes.c_double
    L.brx_last_trace.restype = ctypes.c_int
    L.brx_last_trace.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    L.brx_last_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.brx_synchronize.restype = ctypes.c_int
    L.brx_synchronize.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.brx_stream_new.restype = ctypes.c_void_p
    L.brx_stream_new.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    L.brx_stream_new_bounded.restype = ctypes.c_void_p
    L.brx_stream_new_bounded.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    L.brx_stream_new_reader.restype = ctypes.c_void_p
    L.brx_stream_new_reader.argtypes = [ctypes.c_void_p, READ_FN, ctypes.c_void_p]
    L.brx_stream_read.restype = ctypes.c_int64
    L.brx_stream_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.brx_stream_free.restype = None
    L.brx_stream_free.argtypes = [ctypes.c_void_p]
    L.brx_stream_advance.restype = ctypes.c_int
    L.brx_stream_advance.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32]
    L.brx_stream_ready.restype = ctypes.c_int64
    L.brx_stream_ready.argtypes = [ctypes.c_void_p]
    L.brx_host_alloc.restype = ctypes.c_void_p
    L.brx_host_alloc.argtypes = [ctypes.c_size_t]
    L.brx_host_free.restype = None
    L.brx_host_free.argtypes = [ctypes.c_void_p]
    L.brx_node_create.restype = ctypes.c_int
    L.brx_node_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    L.brx_node_destroy.restype = None
    L.brx_node_destroy.argtypes = [ctypes.c_void_p]
    L.brx_node_size.restype = ctypes.c_int
    L.brx_node_size.argtypes = [ctypes.c_void_p]
    L.brx_node_ctx.restype = ctypes.c_void_p
    L.brx_node_ctx.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.brx_node_set_option.restype = ctypes.c_int
    L.brx_node_set_option.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int64]
    L.brx_node_decode_batch.restype = ctypes.c_int
    L.brx_node_decode_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(_NodeOpts)]
    L.brx_node_deal.restype = ctypes.c_int
    L.brx_node_deal.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    L.brx_node_last_timing.restype = ctypes.c_double
    L.brx_node_last_timing.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    _lib = L
    return L


READ_FN = ctypes.CFUNCTYPE(ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_ubyte), ctypes.c_size_t)  # brx_read_fn

EXPORTED_SYMBOLS = ["brx_ctx_create", "brx_ctx_destroy", "brx_decode_batch", "brx_status_str", "brx_last_error",
                    "brx_last_timing", "brx_synchronize", "brx_stream_new", "brx_stream_read", "brx_stream_free",
                    "brx_host_alloc", "brx_host_free", "brx_stream_new_bounded", "brx_generate_batch", "brx_compact_batch",
                    "brx_ctx_set_option", "brx_last_trace", "brx_stream_new_reader", "brx_node_create", "brx_node_destroy",
                    "brx_node_size", "brx_node_ctx", "brx_node_set_option", "brx_node_decode_batch", "brx_node_last_timing", "brx_node_deal",
                    "brx_stream_advance", "brx_stream_ready", "brx_digest_batch", "brx_index_batch", "brx_index_quoted_batch",
                    "brx_find_batch", "brx_index_escaped_batch", "brx_index_set_batch", "brx_take_batch", "brx_hash_batch",
                    "brx_parse_batch", "brx_parse_time_batch", "brx_unescape_batch", "brx_member_batch", "brx_elements_batch",
                    "brx_object_batch"]
# Exported names with a digit in them.  They are kept apart because tests/test_abi.py compares EXPORTED_SYMBOLS with the names it reads
# from include/brx.h by the pattern brx_[a-z_]+, which such a name does not match; tests/test_parse_f64_abi.py holds this list to the
# header and to the library.
EXPORTED_SYMBOLS_NUMBERED = ["brx_parse_f64_batch"]


def status_str(code: int) -> str:
    return load_library().brx_status_str(int(code)).decode("utf-8")


# brx_ctx_set_option (include/brx.h, BRX_OPTION_*): explicit knobs -- neither the library nor this module reads the environment
OPTIONS = {"command_loop": 1, "loop_build": 2, "queue_order": 3, "hand_up": 4, "levels": 5, "tiny_bytes": 6,
           "host_in_place": 7, "grid_cap": 8, "small_bytes": 9, "small_waves": 10, "trace": 11, "reader_window": 12, "level4": 13, "reader_mb_room": 14,
           "reader_batch": 15, "prio_shift": 16}


def _on(stream):
    """The torch stream that a call's own torch work goes to: `stream`, or the current one."""
    import torch
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


# ---- what the wrappers of the record calls share (take, hash, parse, parse_f64, parse_time, unescape: DESIGN.md 17.1) ----------------
# A wrapper raises in this order: _rec_flags (trim_cr), its own checks, _rec_begin (the pairing); `who` is the method's name.
def _rec_flags(who, keep_delim, trim_cr, own=0):
    """The flags word: take's two bits from keep_delim / trim_cr, and the call's own."""
    if trim_cr and keep_delim:
        raise BrxError("%s: trim_cr needs keep_delim=False" % who)
    return (0 if keep_delim else TAKE_NO_DELIM) | (TAKE_TRIM_CR if trim_cr else 0) | own


_Rec = collections.namedtuple("_Rec", "head m hs sel_stream sel_rec bufs")


def _rec_begin(who, out, out_off, out_len, count, pos_off, pos, sel_stream, sel_rec, delim_len, flags, stream, dtypes):
    """The selection as the device call takes it: a _Rec of the 14 leading arguments of the *_batch_device method (`head`), the number
    of entries (`m`), the hip stream (`hs`), the converted selection tensors (`sel_stream`, `sel_rec`: `head` holds their addresses,
    so the wrapper keeps the _Rec until its last device call) and one uninitialised tensor of max(m, 1) elements (an empty view has no
    address) per name in `dtypes` (None for None), allocated on `stream` (`bufs`)."""
    import torch
    n = int(out_len.numel())
    if (sel_stream is None) != (sel_rec is None):
        raise BrxError("%s: sel_stream and sel_rec go together" % who)
    with _on(stream):
        if sel_stream is not None:
            sel_stream = sel_stream.to(torch.int32).contiguous()
            sel_rec = sel_rec.to(torch.int64).contiguous()
            m = int(sel_stream.numel())
        else:
            m = int(pos.numel()) + n  # sum(count) + n for a consistent caller; no read back
        bufs = [None if t is None else torch.empty(max(m, 1), dtype=getattr(torch, t), device=out.device) for t in dtypes]
    head = (out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), n, int(out.numel()), count.data_ptr(), pos_off.data_ptr(),
            pos.data_ptr() if pos.numel() else None, int(pos.numel()), int(delim_len), flags,
            sel_stream.data_ptr() if sel_stream is not None else None, sel_rec.data_ptr() if sel_rec is not None else None, m)
    return _Rec(head, m, stream.cuda_stream if stream is not None else None, sel_stream, sel_rec, bufs)


def _rec_sync(out, stream):
    """In front of a device call that follows torch work: without `stream` the call runs on the context's stream, which is not ordered
    behind torch's."""
    import torch
    if stream is None:
        torch.cuda.current_stream(out.device).synchronize()


def _rec_gather(out, stream, m, length, stride, fill_pass):
    """The destination of m records and its filling.  stride=None: the records back to back, dst_off the exclusive prefix sum of
    `length`, which a size pass has been launched to write (one scalar is read back for the total).  stride=S: rows of S bytes, zero
    behind a record's end; `length` is not read and nothing is read back.  Then fill_pass(dst_off_ptr, dst_ptr, total), unless m is 0.
    Returns (dst, dst_off)."""
    import torch
    with _on(stream):
        if stride is None:
            ends = torch.cumsum(length, 0)
            dst_off = ends - length
            total = int(ends[-1].item()) if m else 0  # (the read-back: waits for the size pass)
            dst = torch.empty(max(total, 1), dtype=torch.uint8, device=out.device)
        else:
            dst_off = torch.arange(m, dtype=torch.int64, device=out.device) * int(stride)
            total = m * int(stride)
            dst = torch.zeros(max(total, 1), dtype=torch.uint8, device=out.device)
    _rec_sync(out, stream)
    if m:
        fill_pass(dst_off.data_ptr(), dst.data_ptr(), total)
    return dst[:total], dst_off


# ---- what the wrappers of the boundary calls share (index, index_quoted, index_escaped, index_set, find: DESIGN.md 11.1) --------------
def _two_pass(device, args, out, out_len, stream, positions, has_open=False, has_what=False):
    """Count mode, then fill mode, of `device`, the pass's *_batch_device method: behind its own leading arguments `args` it takes
    count_ptr, open_ptr (only with has_open), pos_off_ptr, pos_ptr, what_ptr (only with has_what), total and hip_stream.  Returns count,
    or (count, open) with has_open; with `positions` (count[, open], pos_off, pos[, what]): the grand total is read back to allocate
    `pos` (and `what`)."""
    import torch
    n = int(out_len.numel())
    count = torch.empty(max(n, 1), dtype=torch.int64, device=out.device)[:n]  # (the pass clears it, or writes every entry)
    head = (count, torch.empty(max(n, 1), dtype=torch.int32, device=out.device)[:n]) if has_open else (count,)
    hs = stream.cuda_stream if stream is not None else None
    _rec_sync(out, stream)
    device(*args, *(t.data_ptr() for t in head), hip_stream=hs)
    if not positions:
        return head if has_open else count
    with _on(stream):
        ends = torch.cumsum(count, 0)
        pos_off = ends - count
        total = int(ends[-1].item()) if n else 0  # (the read-back: waits for the count pass)
        tail = (torch.empty(max(total, 1), dtype=torch.int64, device=out.device),)
        if has_what:
            tail += (torch.empty(max(total, 1), dtype=torch.uint8, device=out.device),)
    device(*args, *(None for _ in head), pos_off.data_ptr(), *(t.data_ptr() for t in tail), total, hip_stream=hs)
    return head + (pos_off,) + tuple(t[:total] for t in tail)


class Context:
    """One brx_ctx: a GPU, its tables, scratch and stream.  `options`: {name: value} of OPTIONS, applied at creation."""

    def __init__(self, device: int = 0, options=None):
        self._lib = load_library()
        h = ctypes.c_void_p()
        rc = self._lib.brx_ctx_create(ctypes.byref(h), device)
        if rc != 0:
            raise BrxError("brx_ctx_create failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))
        self._h = h
        self.device = device
        for name, value in (options or {}).items():
            self.set_option(name, value)

    def set_option(self, name, value):
        rc = self._lib.brx_ctx_set_option(self._h, OPTIONS[name], int(value))
        if rc != 0:
            raise BrxError("brx_ctx_set_option(%s, %d) failed: %s" % (name, value, self._lib.brx_last_error().decode()))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.brx_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host-memory batch --------------------------------------------------------------------------
    def decode_batch(self, streams, capacities, timing=False):
        """Decode a list of compressed byte strings.  `capacities`: per-stream output capacity (int or list).
        Returns (outputs: list[bytes], status: np.int32[n], out_len: np.uint64[n])."""
        n = len(streams)
        if isinstance(capacities, int):
            capacities = [capacities] * n
        in_off = np.zeros(n + 1, dtype=np.uint64)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in streams], out=in_off[1:])
        np.cumsum(capacities, out=out_off[1:])
        blob = np.frombuffer(b"".join(streams), dtype=np.uint8) if in_off[-1] else np.zeros(1, dtype=np.uint8)
        out = np.zeros(max(int(out_off[-1]), 1), dtype=np.uint8)
        out_len = np.zeros(max(n, 1), dtype=np.uint64)
        status = np.full(max(n, 1), -1, dtype=np.int32)
        opts = _Opts(MEM_HOST | (OPT_TIMING if timing else 0), 0, None)
        rc = self._lib.brx_decode_batch(self._h, blob.ctypes.data, in_off.ctypes.data, n, out.ctypes.data,
                                        out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data,
                                        ctypes.byref(opts))
        if rc != 0:
            raise BrxError("brx_decode_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))
        outs = []
        for i in range(n):
            ln = int(out_len[i]) if status[i] == OK else 0
            outs.append(out[int(out_off[i]):int(out_off[i]) + ln].tobytes())
        return outs, status[:n], out_len[:n]

    # ---- host-memory batch in caller-owned (e.g. pinned) buffers ----------------------------------------
    def decode_batch_host_raw(self, in_ptr, in_off, n, out_ptr, out_off, timing=False):
        """Host pointers as they are (no copies on the Python side): `in_ptr` / `out_ptr` are addresses, e.g. of
        buffers from host_alloc(); in_off / out_off are np.uint64[n+1].  Returns (status, out_len)."""
        out_len = np.zeros(max(n, 1), dtype=np.uint64)
        status = np.full(max(n, 1), -1, dtype=np.int32)
        opts = _Opts(MEM_HOST | (OPT_TIMING if timing else 0), 0, None)
        rc = self._lib.brx_decode_batch(self._h, in_ptr, in_off.ctypes.data, n, out_ptr, out_off.ctypes.data,
                                        out_len.ctypes.data, status.ctypes.data, ctypes.byref(opts))
        if rc != 0:
            raise BrxError("brx_decode_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))
        return status[:n], out_len[:n]

    # ---- stream generator (brx_generate_batch): inputs -> valid Brotli streams, made on the GPU ----------
    @staticmethod
    def generate_slot_bytes(n_bytes, metablock_bytes=65536, adaptive=False):
        """A slot size that always suffices for an input of n_bytes (brx.h)."""
        return n_bytes + n_bytes // 8 + (2048 if adaptive else 256) * (n_bytes // metablock_bytes + 2)

    def generate_batch(self, sources, metablock_bytes=65536, switches=False, adaptive=False):
        """list of bytes -> list of Brotli streams (host buffers; the work happens on the device).  switches: two literal
        block types taking turns every 100 literals (BRX_GEN_SWITCHES).  adaptive: the wave-per-stream generator with codes
        from each meta-block's statistics, two literal trees behind a context map, real block switches (BRX_GEN_ADAPTIVE)."""
        n = len(sources)
        if n == 0:
            return []
        src_off = np.zeros(n + 1, dtype=np.uint64)
        src_off[1:] = np.cumsum([len(x) for x in sources], dtype=np.uint64)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        out_off[1:] = np.cumsum([self.generate_slot_bytes(len(x), metablock_bytes, adaptive) for x in sources], dtype=np.uint64)
        blob = np.frombuffer(b"".join(sources) or b"\0", dtype=np.uint8)
        out = np.zeros(int(out_off[-1]), dtype=np.uint8)
        out_len = np.zeros(n, dtype=np.uint64)
        status = np.full(n, -1, dtype=np.int32)
        opts = _Opts(MEM_HOST | (GEN_SWITCHES if switches else 0) | (GEN_ADAPTIVE if adaptive else 0), 0, None)
        rc = self._lib.brx_generate_batch(self._h, blob.ctypes.data, src_off.ctypes.data, n, out.ctypes.data, out_off.ctypes.data,
                                          out_len.ctypes.data, status.ctypes.data, metablock_bytes, ctypes.byref(opts))
        if rc != 0:
            raise BrxError("brx_generate_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))
        assert not status.any(), status
        return [out[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes() for i in range(n)]

    def generate_batch_device(self, src_ptr, src_off_ptr, n, out_ptr, out_off_ptr, out_len_ptr, status_ptr, metablock_bytes=65536,
                              hip_stream=None, switches=False, adaptive=False):
        """Raw device pointers (e.g. torch tensors): nothing leaves the GPU."""
        opts = _Opts(MEM_DEVICE | (GEN_SWITCHES if switches else 0) | (GEN_ADAPTIVE if adaptive else 0), 0, hip_stream)
        rc = self._lib.brx_generate_batch(self._h, src_ptr, src_off_ptr, n, out_ptr, out_off_ptr, out_len_ptr, status_ptr,
                                          metablock_bytes, ctypes.byref(opts))
        if rc != 0:
            raise BrxError("brx_generate_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    # ---- device-memory batch (pointers are raw device addresses, e.g. torch tensor .data_ptr()) ------
    def decode_batch_device(self, in_ptr, in_off_ptr, n, out_ptr, out_off_ptr, out_len_ptr, status_ptr,
                            hip_stream=None, timing=False, order=False):
        opts = _Opts(MEM_DEVICE | (OPT_TIMING if timing else 0) | (OPT_ORDER if order else 0), 0, hip_stream)
        rc = self._lib.brx_decode_batch(self._h, in_ptr, in_off_ptr, n, out_ptr, out_off_ptr, out_len_ptr,
                                        status_ptr, ctypes.byref(opts))
        if rc != 0:
            raise BrxError("brx_decode_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def compact_batch_device(self, out_ptr, out_off_ptr, len_ptr, n, dst_ptr, dst_off_ptr, total, hip_stream=None):
        """dst[dst_off[i] ..] = out[out_off[i] .. + len[i]) for the n streams of a decoded batch (device pointers)."""
        rc = self._lib.brx_compact_batch(self._h, out_ptr, out_off_ptr, len_ptr, n, dst_ptr, dst_off_ptr, total, hip_stream)
        if rc != 0:
            raise BrxError("brx_compact_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def digest_batch_device(self, kind, out_ptr, out_off_ptr, len_ptr, n, digest_ptr, expect_ptr=None, mismatch_ptr=None, hip_stream=None):
        """brx_digest_batch on raw device pointers: digest[i] = CRC-32 (kind 1) / CRC-32C (kind 2) of out[out_off[i] .. + len[i])."""
        rc = self._lib.brx_digest_batch(self._h, kind, out_ptr, out_off_ptr, len_ptr, n, digest_ptr, expect_ptr, mismatch_ptr, hip_stream)
        if rc != 0:
            raise BrxError("brx_digest_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def digest_batch(self, out, out_off, out_len, kind="crc32", expect=None, stream=None):
        """CRC-32 / CRC-32C ("crc32" / "crc32c") of the decoded streams of a batch, on the device.  out: uint8 device tensor;
        out_off: int64 device tensor, the first len(out_len) entries are used; out_len: int64 device tensor, the entries of failed
        streams zeroed.  Returns the digests (int32 tensor holding the 32-bit patterns: `& 0xFFFFFFFF` after .tolist()), and with
        `expect` (same layout) also the mismatch tensor (1 where a digest differs, else 0).  stream: a torch.cuda.Stream the work
        is enqueued on (no synchronisation); None = the context's own stream, and the call returns when the digests are there."""
        import torch
        n = int(out_len.numel())
        digest = torch.empty(max(n, 1), dtype=torch.int32, device=out.device)
        mismatch = torch.empty(max(n, 1), dtype=torch.int32, device=out.device) if expect is not None else None
        if stream is None:
            torch.cuda.current_stream(out.device).synchronize()  # (the context's stream is not ordered behind torch's)
        self.digest_batch_device(DIGEST_KINDS[kind], out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), n, digest.data_ptr(),
                                 expect.data_ptr() if expect is not None else None,
                                 mismatch.data_ptr() if mismatch is not None else None,
                                 stream.cuda_stream if stream is not None else None)
        if expect is not None:
            return digest[:n], mismatch[:n]
        return digest[:n]

    def index_batch_device(self, delim, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr=None, pos_ptr=None, total=0,
                           hip_stream=None):
        """brx_index_batch on raw device pointers: count[i] = bytes equal to `delim` in out[out_off[i] .. + len[i]); with pos_off / pos
        also pos[pos_off[i] + k] = offset within stream i of the k-th of them (entries at or beyond `total` are not written)."""
        rc = self._lib.brx_index_batch(self._h, delim, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, total,
                                       hip_stream)
        if rc != 0:
            raise BrxError("brx_index_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def index_batch(self, out, out_off, out_len, delim=10, stream=None, positions=True):
        """Record boundaries of the decoded streams of a batch, on the device.  out: uint8 device tensor (the whole arena); out_off:
        int64 device tensor, the first len(out_len) entries are used; out_len: int64 device tensor, the entries of failed streams
        zeroed; delim: the delimiter byte (default newline).  Returns (count, pos_off, pos), int64 device tensors: count[i] delimiters
        in stream i, pos[pos_off[i] + k] the offset within stream i of the k-th -- or `count` alone with positions=False.  stream: a
        torch.cuda.Stream the work is enqueued on; None = the context's own stream.  With positions the call reads the grand total
        back to allocate `pos`: the one synchronisation a caller that wants the positions cannot avoid."""
        args = (int(delim), out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), int(out_len.numel()), int(out.numel()))
        return _two_pass(self.index_batch_device, args, out, out_len, stream, positions)

    def index_quoted_batch_device(self, delim, quote, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, open_ptr=None, pos_off_ptr=None,
                                  pos_ptr=None, total=0, hip_stream=None):
        """brx_index_quoted_batch on raw device pointers: count[i] = bytes equal to `delim` in out[out_off[i] .. + len[i]) with an even
        number of `quote` bytes of the stream in front of them; open[i] (uint32) = 1 where the stream holds an odd number of quotes;
        with pos_off / pos also pos[pos_off[i] + k] = offset within stream i of the k-th of them (entries at or beyond `total` are not
        written)."""
        rc = self._lib.brx_index_quoted_batch(self._h, delim, quote, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, open_ptr,
                                              pos_off_ptr, pos_ptr, total, hip_stream)
        if rc != 0:
            raise BrxError("brx_index_quoted_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def index_quoted_batch(self, out, out_off, out_len, delim=10, quote=0x22, stream=None, positions=True):
        """Record boundaries of the decoded streams of a batch that respect quoted fields (RFC 4180), on the device: a `delim` byte
        counts only where the number of `quote` bytes in front of it in its stream is even.  Arguments as for index_batch.  Returns
        (count, open, pos_off, pos): count, pos_off and pos as index_batch gives them (int64 device tensors), open an int32 device
        tensor, 1 where stream i ends inside a quoted field -- or (count, open) with positions=False.  With positions the call reads
        the grand total back to allocate `pos`, as index_batch does."""
        args = (int(delim), int(quote), out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), int(out_len.numel()), int(out.numel()))
        return _two_pass(self.index_quoted_batch_device, args, out, out_len, stream, positions, has_open=True)

    def index_escaped_batch_device(self, delim, quote, escape, flags, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, open_ptr=None,
                                   pos_off_ptr=None, pos_ptr=None, total=0, hip_stream=None):
        """brx_index_escaped_batch on raw device pointers: a byte of out[out_off[i] .. + len[i]) behind an odd run of `escape` bytes is
        data; count[i] = bytes equal to `delim` that are not escaped and have an even number of unescaped `quote` bytes of the stream
        in front of them (flags = INDEX_NO_QUOTE: no byte is a quote); open[i] (uint32): bit 0 = the stream ends inside a quoted field,
        bit 1 = it ends on an escape with nothing to escape; with pos_off / pos also pos[pos_off[i] + k] = offset within stream i of
        the k-th of them (entries at or beyond `total` are not written)."""
        rc = self._lib.brx_index_escaped_batch(self._h, delim, quote, escape, flags, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr,
                                               open_ptr, pos_off_ptr, pos_ptr, total, hip_stream)
        if rc != 0:
            raise BrxError("brx_index_escaped_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def index_escaped_batch(self, out, out_off, out_len, delim=10, quote=0x22, escape=0x5C, no_quote=False, stream=None, positions=True):
        """Record boundaries of the decoded streams of a batch under a dialect with an escape byte (JSON Lines, SQL text dumps, CSV
        with an escape character), on the device: a byte behind an odd run of `escape` bytes is data; a `delim` byte counts where it
        is not escaped and the number of unescaped `quote` bytes in front of it in its stream is even.  no_quote: no byte is a quote
        (`quote` is ignored).  Arguments otherwise as for index_batch.  Returns what index_quoted_batch returns, (count, open, pos_off,
        pos) or (count, open) with positions=False; open has two bits: 1 = stream i ends inside a quoted field, 2 = it ends on an
        escape that has nothing to escape.  With positions the call reads the grand total back to allocate `pos`, as index_batch
        does."""
        args = (int(delim), int(quote), int(escape), INDEX_NO_QUOTE if no_quote else 0, out.data_ptr(), out_off.data_ptr(),
                out_len.data_ptr(), int(out_len.numel()), int(out.numel()))
        return _two_pass(self.index_escaped_batch_device, args, out, out_len, stream, positions, has_open=True)

    def index_set_batch_device(self, delims, quote, escape, flags, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, open_ptr=None,
                               pos_off_ptr=None, pos_ptr=None, what_ptr=None, total=0, hip_stream=None):
        """brx_index_set_batch on raw device pointers: index_escaped_batch_device with a set of delimiters (`delims`: bytes, 1 .. 8
        distinct values, host memory, taken during the call) and with flags = INDEX_NO_QUOTE | INDEX_NO_ESCAPE switching the quote and
        the escape off; with pos_off / pos also what[pos_off[i] + k] (uint8, may be None) = the byte at the k-th boundary of stream i."""
        delims = bytes(delims)
        rc = self._lib.brx_index_set_batch(self._h, delims, len(delims), quote, escape, flags, out_ptr, out_off_ptr, len_ptr, n, span,
                                           count_ptr, open_ptr, pos_off_ptr, pos_ptr, what_ptr, total, hip_stream)
        if rc != 0:
            raise BrxError("brx_index_set_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def index_set_batch(self, out, out_off, out_len, delims=b",\n", quote=0x22, escape=0x5C, no_quote=False, no_escape=False, stream=None,
                        positions=True):
        """Boundaries of the decoded streams of a batch at a SET of delimiter bytes (`delims`: bytes, 1 .. 8 distinct values -- b",\\n"
        for CSV fields and records, b"{}[]:,\\n" for the structure of JSON Lines), on the device, under the rule of index_escaped_batch:
        a byte of the set counts where it is not escaped and outside quotes.  no_quote: no byte is a quote; no_escape: no byte is an
        escape (alone: RFC 4180; both: a plain index of the set).  Arguments otherwise as for index_batch.  Returns (count, open,
        pos_off, pos, what) -- what index_escaped_batch returns and `what`, a uint8 device tensor with the byte that stands at each
        position -- or (count, open) with positions=False.  With positions the call reads the grand total back to allocate `pos`
        and `what`, as index_batch does."""
        flags = (INDEX_NO_QUOTE if no_quote else 0) | (INDEX_NO_ESCAPE if no_escape else 0)
        args = (bytes(delims), int(quote), int(escape), flags, out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), int(out_len.numel()),
                int(out.numel()))
        return _two_pass(self.index_set_batch_device, args, out, out_len, stream, positions, has_open=True, has_what=True)

    def find_batch_device(self, needle, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr=None, pos_ptr=None, total=0,
                          hip_stream=None):
        """brx_find_batch on raw device pointers: count[i] = occurrences of `needle` (bytes, 1 .. 16 of them, host memory) in
        out[out_off[i] .. + len[i]), overlapping ones included; with pos_off / pos also pos[pos_off[i] + k] = offset within stream i of
        the first byte of the k-th of them (entries at or beyond `total` are not written).  The needle's bytes are taken during the call."""
        needle = bytes(needle)
        rc = self._lib.brx_find_batch(self._h, needle, len(needle), out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr,
                                      pos_ptr, total, hip_stream)
        if rc != 0:
            raise BrxError("brx_find_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def find_batch(self, out, out_off, out_len, needle, stream=None, positions=True):
        """Occurrences of a byte sequence in the decoded streams of a batch, on the device: needle is bytes, 1 .. 16 of them (b"\\r\\n"
        for CRLF text); every occurrence counts, overlapping ones included.  out, out_off, out_len and stream as for index_batch.
        Returns (count, pos_off, pos), int64 device tensors: count[i] occurrences in stream i, pos[pos_off[i] + k] the offset within
        stream i of the first byte of the k-th -- or `count` alone with positions=False.  With positions the call reads the grand
        total back to allocate `pos`, as index_batch does."""
        args = (needle, out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), int(out_len.numel()), int(out.numel()))
        return _two_pass(self.find_batch_device, args, out, out_len, stream, positions)

    def take_batch_device(self, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, n_pos, delim_len, flags,
                          sel_stream_ptr, sel_rec_ptr, m, rec_len_ptr, dst_off_ptr=None, dst_ptr=None, total=0, hip_stream=None):
        """brx_take_batch on raw device pointers: entry j of the selection is record sel_rec[j] of stream sel_stream[j] (uint32 / uint64;
        both None: every record of every stream in turn, m = sum(count) + n) under the positions count / pos_off / pos of an index or
        find pass (delim_len = 1, or the needle's length).  Size mode (dst_off_ptr and dst_ptr None): rec_len[j] = the record's length.
        Fill mode: dst[dst_off[j] + t] = the record's byte t for t below its length and its room; nothing at or beyond `total` is
        written.  flags: TAKE_NO_DELIM | TAKE_TRIM_CR."""
        rc = self._lib.brx_take_batch(self._h, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, n_pos, delim_len,
                                      flags, sel_stream_ptr, sel_rec_ptr, m, rec_len_ptr, dst_off_ptr, dst_ptr, total, hip_stream)
        if rc != 0:
            raise BrxError("brx_take_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def take_batch(self, out, out_off, out_len, count, pos_off, pos, sel_stream=None, sel_rec=None, delim_len=1, keep_delim=True,
                   trim_cr=False, stride=None, stream=None):
        """The selected records of the decoded streams of a batch, gathered on the device.  out, out_off, out_len and stream as for
        index_batch; count, pos_off, pos as index_batch, index_quoted_batch, index_escaped_batch, index_set_batch (delim_len = 1) or
        find_batch (delim_len = len(needle)) returned them.  sel_stream (int32 device tensor) and sel_rec (int64): entry j is record
        sel_rec[j] of stream sel_stream[j], in any order, repeats allowed, out-of-range entries empty; both None: every record of
        every stream in turn (count[i] + 1 per stream: the last one is what follows the last delimiter).  keep_delim=False drops the
        delimiter, trim_cr=True (only then) also one CR in front of it.  Returns (dst, dst_off, rec_len): uint8 and two int64 device
        tensors.  stride=None: the records back to back, dst_off the exclusive prefix sum of rec_len (one scalar is read back for the
        total).  stride=S: record j in dst[j * S .. (j + 1) * S), cut at S, the rest of its row zero; nothing is read back."""
        flags = _rec_flags("take_batch", keep_delim, trim_cr)
        r = _rec_begin("take_batch", out, out_off, out_len, count, pos_off, pos, sel_stream, sel_rec, delim_len, flags, stream, ("int64",))
        rec_len = r.bufs[0][:r.m]
        _rec_sync(out, stream)
        self.take_batch_device(*r.head, r.bufs[0].data_ptr(), hip_stream=r.hs)
        dst, dst_off = _rec_gather(out, stream, r.m, rec_len, stride,
                                   lambda off, dst, total: self.take_batch_device(*r.head, None, off, dst, total, hip_stream=r.hs))
        return dst, dst_off, rec_len

    def hash_batch_device(self, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, n_pos, delim_len, flags,
                          sel_stream_ptr, sel_rec_ptr, m, seed, hash_ptr, rec_len_ptr=None, hip_stream=None):
        """brx_hash_batch on raw device pointers: hash[j] = the 64-bit key of entry j of the selection under `seed`, the selection, the
        positions and the flags exactly as for take_batch_device; rec_len (optional) as its size mode writes it."""
        rc = self._lib.brx_hash_batch(self._h, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, n_pos, delim_len,
                                      flags, sel_stream_ptr, sel_rec_ptr, m, int(seed) & 0xFFFFFFFFFFFFFFFF, hash_ptr, rec_len_ptr, hip_stream)
        if rc != 0:
            raise BrxError("brx_hash_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def hash_batch(self, out, out_off, out_len, count, pos_off, pos, sel_stream=None, sel_rec=None, delim_len=1, keep_delim=True,
                   trim_cr=False, seed=0, want_len=False, stream=None):
        """A 64-bit key of every selected record of the decoded streams of a batch, computed on the device.  Every argument up to
        trim_cr as for take_batch.  Returns an int64 device tensor (the 64-bit pattern of the hash that include/brx.h defines: equal
        records get equal keys under one seed; the empty record gets 0), and with want_len=True the pair (hash, rec_len).  Nothing is
        read back.  Exact de-duplication of the lines of a batch, the bytes copied once and only for the survivors:
            count, _, pos_off, pos, _ = ctx.index_set_batch(out, out_off, out_len, delims=b"\\n", no_quote=True, no_escape=True)
            key = ctx.hash_batch(out, out_off, out_len, count, pos_off, pos, keep_delim=False, trim_cr=True)
            uniq, inverse = torch.unique(key, return_inverse=True)
            first = torch.full_like(uniq, key.numel()).scatter_reduce_(0, inverse, torch.arange(key.numel(), device=key.device), "amin")
            stream_of = torch.searchsorted(pos_off + torch.arange(pos_off.numel(), device=key.device), first, right=True) - 1
            rec_of = first - (pos_off + torch.arange(pos_off.numel(), device=key.device))[stream_of]
            dst, dst_off, rec_len = ctx.take_batch(out, out_off, out_len, count, pos_off, pos, sel_stream=stream_of, sel_rec=rec_of,
                                                   keep_delim=False, trim_cr=True)
        (entry j of all-records mode is record j - (pos_off[i] + i) of stream i).  key % G shards the records over G workers."""
        flags = _rec_flags("hash_batch", keep_delim, trim_cr)
        r = _rec_begin("hash_batch", out, out_off, out_len, count, pos_off, pos, sel_stream, sel_rec, delim_len, flags, stream,
                       ("int64", "int64" if want_len else None))
        hash_buf, len_buf = r.bufs
        _rec_sync(out, stream)
        self.hash_batch_device(*r.head, seed, hash_buf.data_ptr(), len_buf.data_ptr() if want_len else None, hip_stream=r.hs)
        return (hash_buf[:r.m], len_buf[:r.m]) if want_len else hash_buf[:r.m]

    def parse_batch_device(self, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, n_pos, delim_len, flags,
                           sel_stream_ptr, sel_rec_ptr, m, kind, scale, quote, val_ptr, status_ptr, hip_stream=None):
        """brx_parse_batch on raw device pointers: val[j] (int64) = the number that entry j of the selection spells, status[j] (uint8) =
        PARSE_OK .. PARSE_LONG; the selection, the positions and the TAKE_* flags exactly as for take_batch_device, PARSE_SPACES /
        PARSE_QUOTED in the same flags word; kind PARSE_INT / PARSE_DEC / PARSE_HEX, scale 0 .. 18 (PARSE_DEC only), quote a byte value."""
        rc = self._lib.brx_parse_batch(self._h, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, n_pos, delim_len,
                                       flags, sel_stream_ptr, sel_rec_ptr, m, kind, scale, quote, val_ptr, status_ptr, hip_stream)
        if rc != 0:
            raise BrxError("brx_parse_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def parse_batch(self, out, out_off, out_len, count, pos_off, pos, sel_stream=None, sel_rec=None, delim_len=1, keep_delim=False,
                    trim_cr=False, kind="int", scale=0, spaces=False, quote=None, stream=None):
        """Every selected record of the decoded streams of a batch as a 64-bit number, parsed on the device.  Every argument up to
        trim_cr as for take_batch -- except that keep_delim defaults to False here, because a number never contains its delimiter (with
        keep_delim=True every record that has one comes out PARSE_BAD).  kind: "int" ([+-]? digits), "dec" (digits with an optional
        point; the value is x * 10**scale truncated toward zero, scale 0 .. 18) or "hex" (an optional 0x / 0X, then hex digits, no
        sign).  spaces=True drops leading and trailing blanks and tabs; quote=b'"' then drops one enclosing pair of that byte
        (quote=None: no unquoting).  Returns (val, status): an int64 and a uint8 device tensor, status[j] one of PARSE_OK,
        PARSE_INEXACT (a non-zero fraction digit was cut off), PARSE_EMPTY (nothing there: a missing value), PARSE_RANGE (outside 64
        bits: val is the nearest bound, all ones for hex), PARSE_BAD (not such a number) and PARSE_LONG (a record above 64 bytes,
        not looked at); val is 0 for EMPTY, BAD and LONG.  Nothing is read back.  The prices of a CSV batch, in cents:
            count, _, pos_off, pos, _ = ctx.index_set_batch(out, out_off, out_len, delims=b",\n", no_quote=True, no_escape=True)
            val, status = ctx.parse_batch(out, out_off, out_len, count, pos_off, pos, trim_cr=True, kind="dec", scale=2)"""
        flags = _rec_flags("parse_batch", keep_delim, trim_cr, (PARSE_SPACES if spaces else 0) | (PARSE_QUOTED if quote is not None else 0))
        if kind not in PARSE_KINDS:
            raise BrxError("parse_batch: kind is one of %s" % ", ".join(sorted(PARSE_KINDS)))
        if quote is not None and len(bytes(quote)) != 1:
            raise BrxError("parse_batch: quote is one byte, or None")
        r = _rec_begin("parse_batch", out, out_off, out_len, count, pos_off, pos, sel_stream, sel_rec, delim_len, flags, stream,
                       ("int64", "uint8"))
        val_buf, status_buf = r.bufs
        _rec_sync(out, stream)
        self.parse_batch_device(*r.head, PARSE_KINDS[kind], int(scale), bytes(quote)[0] if quote is not None else 0, val_buf.data_ptr(),
                                status_buf.data_ptr(), hip_stream=r.hs)
        return val_buf[:r.m], status_buf[:r.m]

    def parse_time_batch_device(self, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, n_pos, delim_len, flags,
                                sel_stream_ptr, sel_rec_ptr, m, kind, scale, quote, val_ptr, status_ptr, zone_ptr=None, hip_stream=None):
        """brx_parse_time_batch on raw device pointers: val[j] (int64) = the day number (TIME_DATE) or the count of 10**-scale s (TIME_TIME,
        TIME_STAMP) that entry j of the selection spells, status[j] (uint8) = PARSE_OK .. PARSE_LONG, zone[j] (int16, zone_ptr may be None) =
        the offset in minutes east of UTC or TIME_NO_ZONE; the selection, the positions and the TAKE_* flags exactly as for
        take_batch_device, PARSE_SPACES / PARSE_QUOTED in the same flags word; scale 0 .. 9 (0 with TIME_DATE), quote a byte value."""
        rc = self._lib.brx_parse_time_batch(self._h, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, n_pos, delim_len,
                                            flags, sel_stream_ptr, sel_rec_ptr, m, kind, scale, quote, val_ptr, status_ptr, zone_ptr, hip_stream)
        if rc != 0:
            raise BrxError("brx_parse_time_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def parse_time_batch(self, out, out_off, out_len, count, pos_off, pos, sel_stream=None, sel_rec=None, delim_len=1, keep_delim=False,
                         trim_cr=False, spaces=False, quote=None, kind="stamp", unit="s", zones=False, stream=None):
        """Every selected record of the decoded streams of a batch as a date, a time of day or a timestamp, parsed on the device.  Every
        argument up to trim_cr as for parse_batch (keep_delim defaults to False: a stamp never contains its delimiter).  kind: "date"
        (YYYY-MM-DD: val = days since 1970-01-01, unit must be "s" or 0), "time" (HH:MM[:SS[.fff]]: val = units since midnight) or "stamp"
        (a date, then optionally T, t or a blank, a time and a zone Z / +HH:MM / +HHMM / +HH: val = units since 1970-01-01T00:00:00Z; a
        stamp without a zone is read as UTC, a date alone is midnight).  unit: "s", "ms", "us", "ns", or an integer scale 0 .. 9 (units
        of 10**-scale s); fraction digits beyond the unit are cut off toward minus infinity.  A comma is accepted as the decimal mark.
        spaces=True drops leading and trailing blanks and tabs; quote=b'"' then drops one enclosing pair of that byte.
        Returns (val, status), or (val, status, zone) with zones=True: torch.int64 / torch.uint8 / torch.int16 device tensors.  status[j]
        is one of PARSE_OK, PARSE_INEXACT (a non-zero fraction digit was cut off), PARSE_EMPTY (nothing there), PARSE_RANGE (outside 64
        bits, only at scales 8 and 9: val is the nearest bound), PARSE_BAD (not such a stamp, or a field out of its range) and
        PARSE_LONG (a record above 64 bytes, not looked at); val is 0 for EMPTY, BAD and LONG.  zone[j] is the offset in minutes east
        of UTC where the status is OK or INEXACT and the text carried a zone, else TIME_NO_ZONE.  Nothing is read back.  With unit="ns",
        val.cpu().numpy().view("datetime64[ns]") matches numpy.datetime64[ns] (with "date", view("datetime64[D]")).  The stamps of a log
        batch:
            count, _, pos_off, pos, _ = ctx.index_set_batch(out, out_off, out_len, delims=b",\n", no_quote=True, no_escape=True)
            val, status, zone = ctx.parse_time_batch(out, out_off, out_len, count, pos_off, pos, trim_cr=True, unit="ms", zones=True)"""
        flags = _rec_flags("parse_time_batch", keep_delim, trim_cr, (PARSE_SPACES if spaces else 0) | (PARSE_QUOTED if quote is not None else 0))
        if kind not in TIME_KINDS:
            raise BrxError("parse_time_batch: kind is one of %s" % ", ".join(sorted(TIME_KINDS)))
        if isinstance(unit, str):
            if unit not in TIME_UNITS:
                raise BrxError("parse_time_batch: unit is one of %s, or a scale 0 .. 9" % ", ".join(sorted(TIME_UNITS)))
            scale = TIME_UNITS[unit]
        else:
            scale = int(unit)
            if not 0 <= scale <= TIME_MAX_SCALE:
                raise BrxError("parse_time_batch: unit is one of %s, or a scale 0 .. 9" % ", ".join(sorted(TIME_UNITS)))
        if quote is not None and len(bytes(quote)) != 1:
            raise BrxError("parse_time_batch: quote is one byte, or None")
        r = _rec_begin("parse_time_batch", out, out_off, out_len, count, pos_off, pos, sel_stream, sel_rec, delim_len, flags, stream,
                       ("int64", "uint8", "int16" if zones else None))
        val_buf, status_buf, zone_buf = r.bufs
        _rec_sync(out, stream)
        self.parse_time_batch_device(*r.head, TIME_KINDS[kind], scale, bytes(quote)[0] if quote is not None else 0, val_buf.data_ptr(),
                                     status_buf.data_ptr(), zone_buf.data_ptr() if zones else None, hip_stream=r.hs)
        return (val_buf[:r.m], status_buf[:r.m], zone_buf[:r.m]) if zones else (val_buf[:r.m], status_buf[:r.m])

    def unescape_batch_device(self, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, n_pos, delim_len, flags,
                              sel_stream_ptr, sel_rec_ptr, m, dialect, quote, escape, text_len_ptr, status_ptr, dst_off_ptr=None,
                              dst_ptr=None, total=0, hip_stream=None):
        """brx_unescape_batch on raw device pointers: the string that entry j of the selection spells under `dialect` (TEXT_CSV, TEXT_JSON,
        TEXT_BACKSLASH; quote and escape are byte values); the selection, the positions and the TAKE_* flags exactly as for
        take_batch_device, PARSE_SPACES in the same flags word.  Size mode (dst_off_ptr and dst_ptr None): text_len[j] (uint64) = the
        text's length, status[j] (uint8) = TEXT_OK, TEXT_BARE, TEXT_NULL or TEXT_BAD.  Fill mode: dst[dst_off[j] + t] = the text's byte t
        for t below its length and its room; nothing at or beyond `total` is written; text_len_ptr and status_ptr may be None."""
        rc = self._lib.brx_unescape_batch(self._h, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, n_pos, delim_len,
                                          flags, sel_stream_ptr, sel_rec_ptr, m, dialect, quote, escape, text_len_ptr, status_ptr,
                                          dst_off_ptr, dst_ptr, total, hip_stream)
        if rc != 0:
            raise BrxError("brx_unescape_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def unescape_batch(self, out, out_off, out_len, count, pos_off, pos, sel_stream=None, sel_rec=None, delim_len=1, keep_delim=False,
                       trim_cr=True, dialect="json", quote=0x22, escape=0x5C, spaces=False, stride=None, stream=None):
        """Every selected record of the decoded streams of a batch as the string it spells, unquoted and unescaped on the device.  Every
        argument up to trim_cr as for take_batch -- except that keep_delim defaults to False and trim_cr to True (with keep_delim=True
        trim_cr must be False).  dialect: "csv" (RFC 4180: an enclosing pair of `quote`, "" inside it is one quote), "json" (a JSON
        string: \\n \\" \\/ \\uXXXX and surrogate pairs come out as UTF-8; anything not quoted -- null, a number, true -- comes out as
        it stands, TEXT_BARE) or "backslash" (PostgreSQL COPY text, MySQL tab dumps: \\t \\n \\\\ ..., \\N alone is TEXT_NULL).  quote and
        escape are byte values; spaces=True drops leading and trailing blanks and tabs first.
        Returns (dst, dst_off, text_len, status): uint8, int64, int64 and uint8 device tensors; status[j] is TEXT_OK, TEXT_BARE,
        TEXT_NULL or TEXT_BAD (malformed somewhere: the text is what the walk emitted, see include/brx.h).  stride=None: the texts back
        to back, dst_off the exclusive prefix sum of text_len (a size-mode call, a cumsum on the device, one scalar read back for the
        total, a fill-mode call).  stride=S: one call, text j in dst[j * S .. (j + 1) * S), cut at S (at the byte: text_len[j] > S
        tells), the rest of its row zero; nothing is read back.  The "text" values of a JSON Lines batch, rows {"id": 7, "text": "..."}:
            count, _, pos_off, pos, what = ctx.index_set_batch(out, out_off, out_len, delims=b'{}[]:,\\n')
            # the records are the pieces between two structural bytes: per row "", the key "id", 7, the key "text", the value, ""
            streams = torch.repeat_interleave(torch.arange(count.numel(), device=out.device), count + 1)
            rec = torch.arange(streams.numel(), device=out.device) - (pos_off + torch.arange(count.numel(), device=out.device))[streams]
            pick = rec % 6 == 4
            dst, dst_off, text_len, status = ctx.unescape_batch(out, out_off, out_len, count, pos_off, pos, sel_stream=streams[pick],
                                                                sel_rec=rec[pick], dialect="json", spaces=True)"""
        flags = _rec_flags("unescape_batch", keep_delim, trim_cr, PARSE_SPACES if spaces else 0)
        if dialect not in TEXT_DIALECTS:
            raise BrxError("unescape_batch: dialect is one of %s" % ", ".join(sorted(TEXT_DIALECTS)))
        r = _rec_begin("unescape_batch", out, out_off, out_len, count, pos_off, pos, sel_stream, sel_rec, delim_len, flags, stream,
                       ("int64", "uint8"))
        len_buf, status_buf = r.bufs
        head = r.head + (TEXT_DIALECTS[dialect], int(quote), int(escape))
        sizes = (len_buf.data_ptr(), status_buf.data_ptr())
        if stride is None:  # (with rows of `stride` the one call below is both passes)
            _rec_sync(out, stream)
            self.unescape_batch_device(*head, *sizes, hip_stream=r.hs)
            sizes = (None, None)
        dst, dst_off = _rec_gather(out, stream, r.m, len_buf[:r.m], stride,
                                   lambda off, dst, total: self.unescape_batch_device(*head, *sizes, off, dst, total, hip_stream=r.hs))
        return dst, dst_off, len_buf[:r.m], status_buf[:r.m]

    def member_batch_device(self, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, what_ptr, n_pos, names,
                            lines_ptr, line_off_ptr=None, m=0, sel_stream_ptr=None, sel_rec_ptr=None, kind_ptr=None, line_flags_ptr=None,
                            hip_stream=None):
        """brx_member_batch on raw device pointers: the named members of the JSON Lines objects of a batch, under the positions count /
        pos_off / pos / what of a fill-mode index_set_batch call with delims b'{}[]:,\\n'.  `names`: a sequence of 1 .. 8 distinct
        bytes objects of 1 .. 32 bytes, host memory, taken during the call.  Count mode (line_off_ptr, sel_stream_ptr, sel_rec_ptr and
        kind_ptr None): lines[i] (uint64) = line feeds outside strings of stream i, plus 1.  Fill mode: entry (q, j) at q * m + j, line
        j = line_off[i] + r: sel_stream (uint32), sel_rec (uint64) and kind (uint8, MEMBER_MISSING ... MEMBER_BAD) of the last depth-1
        member of the line whose key is names[q]; line_flags[j] (uint8, may be None) = MEMBER_LONG_KEY | MEMBER_ESCAPED_KEY |
        MEMBER_UNBALANCED.  Nothing at or beyond n_names * m is written."""
        names = [bytes(x) for x in names]
        packed = b"".join(x[:MEMBER_MAX_NAME].ljust(MEMBER_MAX_NAME, b"\0") for x in names)
        lens = (ctypes.c_uint32 * max(len(names), 1))(*[len(x) for x in names])
        rc = self._lib.brx_member_batch(self._h, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, what_ptr, n_pos,
                                        packed, lens, len(names), lines_ptr, line_off_ptr, m, sel_stream_ptr, sel_rec_ptr, kind_ptr,
                                        line_flags_ptr, hip_stream)
        if rc != 0:
            raise BrxError("brx_member_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def member_batch(self, out, out_off, out_len, count, pos_off, pos, what, names, stream=None):
        """The named members of the JSON Lines objects of a batch as selections for the record calls, found on the device.  out, out_off,
        out_len and stream as for index_batch; count, pos_off, pos, what as index_set_batch(delims=b'{}[]:,\\n') returned them; names:
        1 .. 8 distinct keys (bytes, 1 .. 32 of them each, compared bytewise with what stands between the key's quotes).
        Returns (lines, line_off, sel_stream, sel_rec, kind, line_flags): lines[i] = lines of stream i (the last one is what follows
        the last line feed), line_off its exclusive prefix sum, M = sum(lines); sel_stream (int32), sel_rec (int64) and kind (uint8) of
        shape [len(names), M]: row q is the selection of names[q] for a record call, entry j its value in line j -- the LAST depth-1
        member with that key, as json.loads has it; kind MEMBER_SCALAR (the record is the value), MEMBER_OBJECT / MEMBER_ARRAY (a nested
        value starts there), MEMBER_BAD, or MEMBER_MISSING (sel_rec -1: selects nothing, so parse_batch gives PARSE_EMPTY and
        unescape_batch an empty text); line_flags[j] (uint8): MEMBER_LONG_KEY, MEMBER_ESCAPED_KEY, MEMBER_UNBALANCED.  A count-mode
        call, a cumsum on the device, one scalar read back (the total of lines), a fill-mode call.  The ids and texts of a batch whose
        lines carry "id" and "text" in any order, among other keys:
            count, _, pos_off, pos, what = ctx.index_set_batch(out, out_off, out_len, delims=b'{}[]:,\\n')
            lines, line_off, ss, sr, kind, flags = ctx.member_batch(out, out_off, out_len, count, pos_off, pos, what, [b"id", b"text"])
            ids, st = ctx.parse_batch(out, out_off, out_len, count, pos_off, pos, sel_stream=ss[0], sel_rec=sr[0], spaces=True)
            dst, dst_off, text_len, st = ctx.unescape_batch(out, out_off, out_len, count, pos_off, pos, sel_stream=ss[1],
                                                            sel_rec=sr[1], dialect="json", spaces=True)"""
        import torch
        n, Q = int(out_len.numel()), len(names)
        dev = out.device
        hs = stream.cuda_stream if stream is not None else None
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            lines = torch.empty(max(n, 1), dtype=torch.int64, device=dev)[:n]
        _rec_sync(out, stream)
        head = (out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), n, int(out.numel()), count.data_ptr(), pos_off.data_ptr(),
                pos.data_ptr(), what.data_ptr(), int(pos.numel()), names)
        self.member_batch_device(*head, lines.data_ptr(), hip_stream=hs)
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            ends = torch.cumsum(lines, 0)
            line_off = ends - lines
            M = int(ends[-1].item()) if n else 0  # (the read-back: waits for the count pass)
            sel_stream = torch.empty((Q, max(M, 1)), dtype=torch.int32, device=dev)
            sel_rec = torch.empty((Q, max(M, 1)), dtype=torch.int64, device=dev)
            kind = torch.empty((Q, max(M, 1)), dtype=torch.uint8, device=dev)
            line_flags = torch.empty(max(M, 1), dtype=torch.uint8, device=dev)
        if M > 0:  # (the buffers are exactly [Q, M]: entry (q, j) is at q * M + j)
            _rec_sync(out, stream)
            self.member_batch_device(*head, None, line_off.data_ptr(), M, sel_stream.data_ptr(), sel_rec.data_ptr(), kind.data_ptr(),
                                     line_flags.data_ptr(), hip_stream=hs)
        return lines, line_off, sel_stream[:, :M], sel_rec[:, :M], kind[:, :M], line_flags[:M]

    def elements_batch_device(self, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, what_ptr, n_pos, sel_stream_ptr,
                              sel_rec_ptr, m, n_elem_ptr, status_ptr=None, end_ptr=None, el_off_ptr=None, total=0, el_stream_ptr=None,
                              el_rec_ptr=None, el_kind_ptr=None, hip_stream=None):
        """brx_elements_batch on raw device pointers: the elements of the JSON arrays whose openers the pairs (sel_stream, sel_rec) name
        (sel_rec = the boundary index of a '[', as member_batch_device gives it for MEMBER_ARRAY), under the positions count / pos_off /
        pos / what of a fill-mode index_set_batch call with delims b'{}[]:,\\n'.  Count mode (el_off_ptr, el_stream_ptr, el_rec_ptr and
        el_kind_ptr None): n_elem[j] (uint64), status[j] (uint8, ELEMENTS_OK ... ELEMENTS_MISMATCH, may be None) and end[j] (uint64,
        the closer's boundary index, may be None).  Fill mode: element t of entry j at el_off[j] + t, where that is inside the entry's
        room and below `total`: el_stream (uint32), el_rec (uint64) and el_kind (uint8, MEMBER_SCALAR ... MEMBER_BAD); n_elem_ptr may
        be None.  Nothing at or beyond `total` is written."""
        rc = self._lib.brx_elements_batch(self._h, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, what_ptr, n_pos,
                                          sel_stream_ptr, sel_rec_ptr, m, n_elem_ptr, status_ptr, end_ptr, el_off_ptr, total, el_stream_ptr,
                                          el_rec_ptr, el_kind_ptr, hip_stream)
        if rc != 0:
            raise BrxError("brx_elements_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def elements_batch(self, out, out_off, out_len, count, pos_off, pos, what, sel_stream, sel_rec, stream=None):
        """The elements of JSON arrays as a selection for the record calls, found on the device.  out, out_off, out_len and stream as
        for index_batch; count, pos_off, pos, what as index_set_batch(delims=b'{}[]:,\\n') returned them; (sel_stream, sel_rec): the
        openers, as one row of member_batch's sel_stream / sel_rec -- entries that are not MEMBER_ARRAY may stay in it.
        Returns (n_elem, el_off, status, end, el_stream, el_rec, el_kind): per entry the number of elements (int64), its exclusive
        prefix sum, the status (uint8: ELEMENTS_OK, ELEMENTS_NONE for MISSING, ELEMENTS_NOT_ARRAY, ELEMENTS_UNCLOSED, ELEMENTS_MISMATCH
        for an array closed by '}') and the boundary index of the closer (int64, -1 for NONE and NOT_ARRAY); per element, E =
        sum(n_elem) of them, element t of entry j at el_off[j] + t: el_stream (int32) and el_rec (int64), a pairs-mode selection for
        the record calls, and el_kind (uint8): MEMBER_SCALAR (the record is the element), MEMBER_OBJECT, MEMBER_ARRAY (el_rec is again
        an opener: a second elements_batch call takes the nested arrays), MEMBER_BAD.  `[]` and `[ ]` have 0 elements; `[1,]` has a
        blank second one, which parse_batch reports as PARSE_EMPTY.  A count-mode call, a cumsum on the device, one scalar read back
        (the total of elements), a fill-mode call.  The embedding matrix of a batch whose lines carry "emb":[...]:
            count, _, pos_off, pos, what = ctx.index_set_batch(out, out_off, out_len, delims=b'{}[]:,\\n')
            lines, line_off, ss, sr, kind, flags = ctx.member_batch(out, out_off, out_len, count, pos_off, pos, what, [b"emb"])
            n_elem, el_off, status, end, el_stream, el_rec, el_kind = ctx.elements_batch(out, out_off, out_len, count, pos_off, pos, what,
                                                                                         ss[0], sr[0])
            val, st = ctx.parse_f64_batch(out, out_off, out_len, count, pos_off, pos, sel_stream=el_stream, sel_rec=el_rec, spaces=True)
            emb = val.view(M, D)  # where every n_elem is D"""
        import torch
        n, dev = int(out_len.numel()), out.device
        hs = stream.cuda_stream if stream is not None else None
        with _on(stream):
            sel_stream = sel_stream.to(torch.int32).contiguous()
            sel_rec = sel_rec.to(torch.int64).contiguous()
            m = int(sel_stream.numel())
            n_elem = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
            status = torch.empty(max(m, 1), dtype=torch.uint8, device=dev)
            end = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
        head = (out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), n, int(out.numel()), count.data_ptr(), pos_off.data_ptr(),
                pos.data_ptr() if pos.numel() else None, what.data_ptr() if what.numel() else None, int(pos.numel()),
                sel_stream.data_ptr() if m else None, sel_rec.data_ptr() if m else None, m)
        _rec_sync(out, stream)
        self.elements_batch_device(*head, n_elem.data_ptr(), status.data_ptr(), end.data_ptr(), hip_stream=hs)
        with _on(stream):
            n_elem = n_elem[:m]
            ends = torch.cumsum(n_elem, 0)
            el_off = ends - n_elem
            E = int(ends[-1].item()) if m else 0  # (the read-back: waits for the count pass)
            el_stream = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
            el_rec = torch.empty(max(E, 1), dtype=torch.int64, device=dev)
            el_kind = torch.empty(max(E, 1), dtype=torch.uint8, device=dev)
        if E > 0:
            _rec_sync(out, stream)
            self.elements_batch_device(*head, None, None, None, el_off.data_ptr(), E, el_stream.data_ptr(), el_rec.data_ptr(),
                                       el_kind.data_ptr(), hip_stream=hs)
        return n_elem, el_off, status[:m], end[:m], el_stream[:E], el_rec[:E], el_kind[:E]

    def object_batch_device(self, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, what_ptr, n_pos, sel_stream_ptr,
                            sel_rec_ptr, m, names, n_members_ptr, status_ptr=None, end_ptr=None, mem_stream_ptr=None, mem_rec_ptr=None,
                            mem_kind_ptr=None, obj_flags_ptr=None, hip_stream=None):
        """brx_object_batch on raw device pointers: the named members of the nested JSON objects whose openers the pairs (sel_stream,
        sel_rec) name (sel_rec = the boundary index of a '{', as member_batch_device gives it for MEMBER_OBJECT and
        elements_batch_device for an object element), under the positions count / pos_off / pos / what of a fill-mode index_set_batch
        call with delims b'{}[]:,\\n'.  `names`: a sequence of 0 .. 8 distinct bytes objects of 1 .. 32 bytes, host memory, taken
        during the call.  Entry (q, j) at q * m + j: mem_stream (uint32), mem_rec (uint64) and mem_kind (uint8, MEMBER_MISSING ...
        MEMBER_BAD) of the last member of object j whose key is names[q]; n_members[j] (uint64), status[j] (uint8, OBJECT_OK ...
        OBJECT_MISMATCH), end[j] (uint64, the closer's boundary index) and obj_flags[j] (uint8, MEMBER_LONG_KEY | MEMBER_ESCAPED_KEY)
        may each be None.  No names: the extent mode, n_members (required), status and end alone.  Nothing at or beyond
        len(names) * m is written."""
        names = [bytes(x) for x in names]
        packed = b"".join(x[:MEMBER_MAX_NAME].ljust(MEMBER_MAX_NAME, b"\0") for x in names)
        lens = (ctypes.c_uint32 * max(len(names), 1))(*[len(x) for x in names])
        rc = self._lib.brx_object_batch(self._h, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, what_ptr, n_pos,
                                        sel_stream_ptr, sel_rec_ptr, m, packed if names else None, lens if names else None, len(names),
                                        n_members_ptr, status_ptr, end_ptr, mem_stream_ptr, mem_rec_ptr, mem_kind_ptr, obj_flags_ptr,
                                        hip_stream)
        if rc != 0:
            raise BrxError("brx_object_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def object_batch(self, out, out_off, out_len, count, pos_off, pos, what, sel_stream, sel_rec, names=(), stream=None):
        """The named members of nested JSON objects as selections for the record calls, found on the device.  out, out_off, out_len and
        stream as for index_batch; count, pos_off, pos, what as index_set_batch(delims=b'{}[]:,\\n') returned them; (sel_stream,
        sel_rec): the openers, as one row of member_batch's sel_stream / sel_rec or elements_batch's el_stream / el_rec -- entries
        that are not MEMBER_OBJECT may stay in it; names: 0 .. 8 distinct keys (bytes, 1 .. 32 of them each).
        Returns (n_members, status, end, mem_stream, mem_rec, mem_kind, obj_flags): per entry the number of members (int64), the status
        (uint8: OBJECT_OK, OBJECT_NONE for MISSING, OBJECT_NOT_OBJECT, OBJECT_UNCLOSED, OBJECT_MISMATCH for an object closed by ']')
        and the boundary index of the closer (int64, -1 for NONE and NOT_OBJECT); mem_stream (int32), mem_rec (int64) and mem_kind
        (uint8) of shape [len(names), m]: row q is the selection of names[q] for a record call, entry j its value in object j -- the
        LAST member with that key, as json.loads has it; MEMBER_SCALAR (the record is the value), MEMBER_OBJECT (mem_rec is again an
        opener: a second object_batch call goes one level down), MEMBER_ARRAY (an opener for elements_batch), MEMBER_BAD or
        MEMBER_MISSING (mem_rec -1: selects nothing); obj_flags[j] (uint8): MEMBER_LONG_KEY, MEMBER_ESCAPED_KEY.  Without names the
        last four are None: the extent of every object alone.  One call, nothing read back.  The scores under "meta" and the prices
        of the objects in "items", rows {"meta":{"lang":"en","score":0.93},"items":[{"id":1,"price":2.5}]}:
            count, _, pos_off, pos, what = ctx.index_set_batch(out, out_off, out_len, delims=b'{}[]:,\\n')
            lines, line_off, ss, sr, kind, flags = ctx.member_batch(out, out_off, out_len, count, pos_off, pos, what, [b"meta", b"items"])
            _, st, end, ms, mr, mk, _ = ctx.object_batch(out, out_off, out_len, count, pos_off, pos, what, ss[0], sr[0], [b"score"])
            score, vst = ctx.parse_f64_batch(out, out_off, out_len, count, pos_off, pos, sel_stream=ms[0], sel_rec=mr[0], spaces=True)
            n_elem, el_off, est, eend, es, er, ek = ctx.elements_batch(out, out_off, out_len, count, pos_off, pos, what, ss[1], sr[1])
            _, st, end, ms, mr, mk, _ = ctx.object_batch(out, out_off, out_len, count, pos_off, pos, what, es, er, [b"price"])
            price, vst = ctx.parse_f64_batch(out, out_off, out_len, count, pos_off, pos, sel_stream=ms[0], sel_rec=mr[0], spaces=True)"""
        import torch
        n, dev, Q = int(out_len.numel()), out.device, len(names)
        hs = stream.cuda_stream if stream is not None else None
        with _on(stream):
            sel_stream = sel_stream.to(torch.int32).contiguous()
            sel_rec = sel_rec.to(torch.int64).contiguous()
            m = int(sel_stream.numel())
            n_members = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
            status = torch.empty(max(m, 1), dtype=torch.uint8, device=dev)
            end = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
            mem_stream = mem_rec = mem_kind = obj_flags = None
            if Q:  # (the buffers are exactly [Q, m]: entry (q, j) is at q * m + j)
                mem_stream = torch.empty((Q, max(m, 1)), dtype=torch.int32, device=dev)
                mem_rec = torch.empty((Q, max(m, 1)), dtype=torch.int64, device=dev)
                mem_kind = torch.empty((Q, max(m, 1)), dtype=torch.uint8, device=dev)
                obj_flags = torch.empty(max(m, 1), dtype=torch.uint8, device=dev)
        _rec_sync(out, stream)
        self.object_batch_device(out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), n, int(out.numel()), count.data_ptr(),
                                 pos_off.data_ptr(), pos.data_ptr() if pos.numel() else None, what.data_ptr() if what.numel() else None,
                                 int(pos.numel()), sel_stream.data_ptr() if m else None, sel_rec.data_ptr() if m else None, m, names,
                                 n_members.data_ptr(), status.data_ptr(), end.data_ptr(), mem_stream.data_ptr() if Q else None,
                                 mem_rec.data_ptr() if Q else None, mem_kind.data_ptr() if Q else None,
                                 obj_flags.data_ptr() if Q else None, hip_stream=hs)
        if not Q:
            return n_members[:m], status[:m], end[:m], None, None, None, None
        return n_members[:m], status[:m], end[:m], mem_stream[:, :m], mem_rec[:, :m], mem_kind[:, :m], obj_flags[:m]

    def parse_f64_batch_device(self, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, n_pos, delim_len, flags,
                               sel_stream_ptr, sel_rec_ptr, m, quote, val_ptr, status_ptr, hip_stream=None):
        """brx_parse_f64_batch on raw device pointers: val[j] (binary64) = the correctly rounded double that entry j of the selection
        spells, status[j] (uint8) = PARSE_OK, PARSE_EMPTY, PARSE_RANGE, PARSE_BAD, PARSE_LONG or PARSE_HARD; the selection, the positions
        and the TAKE_* flags exactly as for take_batch_device, PARSE_SPACES / PARSE_QUOTED / PARSE_WORDS in the same flags word; quote
        a byte value."""
        rc = self._lib.brx_parse_f64_batch(self._h, out_ptr, out_off_ptr, len_ptr, n, span, count_ptr, pos_off_ptr, pos_ptr, n_pos,
                                           delim_len, flags, sel_stream_ptr, sel_rec_ptr, m, quote, val_ptr, status_ptr, hip_stream)
        if rc != 0:
            raise BrxError("brx_parse_f64_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def parse_f64_batch(self, out, out_off, out_len, count, pos_off, pos, sel_stream=None, sel_rec=None, delim_len=1, keep_delim=False,
                        trim_cr=False, spaces=False, quote=None, words=False, finish=False, stream=None):
        """Every selected record of the decoded streams of a batch as a correctly rounded double, parsed on the device.  Every argument
        up to trim_cr as for parse_batch (keep_delim defaults to False: a number never contains its delimiter).  The grammar is
        [+-]? digits with an optional point, then an optional e / E exponent; words=True also takes [+-]? nan / inf / infinity in any
        letter case.  spaces=True drops leading and trailing blanks and tabs; quote=b'"' then drops one enclosing pair of that byte.
        Returns (val, status): a torch.float64 and a torch.uint8 device tensor, status[j] one of PARSE_OK, PARSE_EMPTY (nothing there),
        PARSE_RANGE (beyond the largest double: val is +-inf; or non-zero and rounded to +-0), PARSE_BAD (not such a number),
        PARSE_LONG (a record above 64 bytes, not looked at) and PARSE_HARD (more than 19 significant digits and too close to a
        rounding boundary for the device: the correctly rounded double is val or the next one away from zero); val is +0 for EMPTY,
        BAD and LONG.  Text printed with up to 17 digits never comes out PARSE_HARD.
        finish=True completes the PARSE_HARD entries on the host: their (stream, record) pairs are derived (in all-records mode from
        pos_off, as the device derives them), their bytes fetched with take_batch in pairs mode, trimmed as the call trims, converted
        with float() and written back with status PARSE_OK or PARSE_RANGE.  It synchronises and reads back one flag, and the bytes
        only when some entry is PARSE_HARD; with finish=False nothing is read back.  The measurements of a CSV batch:
            count, _, pos_off, pos, _ = ctx.index_set_batch(out, out_off, out_len, delims=b",\\n", no_quote=True, no_escape=True)
            val, status = ctx.parse_f64_batch(out, out_off, out_len, count, pos_off, pos, trim_cr=True, finish=True)"""
        import torch
        flags = _rec_flags("parse_f64_batch", keep_delim, trim_cr, (PARSE_SPACES if spaces else 0) | (PARSE_QUOTED if quote is not None else 0)
                           | (PARSE_WORDS if words else 0))
        if quote is not None and len(bytes(quote)) != 1:
            raise BrxError("parse_f64_batch: quote is one byte, or None")
        n = int(out_len.numel())
        r = _rec_begin("parse_f64_batch", out, out_off, out_len, count, pos_off, pos, sel_stream, sel_rec, delim_len, flags, stream,
                       ("float64", "uint8"))
        m, sel_stream, sel_rec, (val_buf, status_buf) = r.m, r.sel_stream, r.sel_rec, r.bufs
        _rec_sync(out, stream)
        self.parse_f64_batch_device(*r.head, bytes(quote)[0] if quote is not None else 0, val_buf.data_ptr(), status_buf.data_ptr(),
                                    hip_stream=r.hs)
        val, status = val_buf[:m], status_buf[:m]
        if not finish or m == 0:
            return val, status
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            hard = torch.nonzero(status == PARSE_HARD).flatten()
            k = int(hard.numel())  # (the read-back: waits for the parse)
            if k == 0:
                return val, status
            if sel_stream is not None:
                h_stream, h_rec = sel_stream[hard], sel_rec[hard]
            else:  # entry j is record j - (pos_off[i] + i) of stream i, the last stream with pos_off[i] + i <= j
                keys = pos_off.to(torch.int64) + torch.arange(n, dtype=torch.int64, device=out.device)
                h_stream = torch.searchsorted(keys, hard, right=True) - 1
                h_rec = hard - keys[h_stream]
        rows, _, rec_len = self.take_batch(out, out_off, out_len, count, pos_off, pos, sel_stream=h_stream, sel_rec=h_rec,
                                           delim_len=delim_len, keep_delim=keep_delim, trim_cr=trim_cr, stride=PARSE_MAX_LEN, stream=stream)
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            rows, rec_len = rows.cpu().numpy().reshape(k, PARSE_MAX_LEN), rec_len.cpu().tolist()
            new_val, new_status = [], []
            for row, ln in zip(rows, rec_len):
                t = row[:ln].tobytes()
                if spaces:
                    t = t.strip(b" \t")
                if quote is not None and len(t) >= 2 and t[:1] == bytes(quote) and t[-1:] == bytes(quote):
                    t = t[1:-1]
                x = float(t.decode("ascii"))  # correctly rounded; a PARSE_HARD entry is a number of the grammar
                new_val.append(x)
                new_status.append(PARSE_RANGE if x == 0.0 or x in (float("inf"), float("-inf")) else PARSE_OK)
            val[hard] = torch.tensor(new_val, dtype=torch.float64).to(out.device)
            status[hard] = torch.tensor(new_status, dtype=torch.uint8).to(out.device)
        return val, status

    def last_timing_ms(self, which=1):
        return float(self._lib.brx_last_timing(self._h, which))

    def last_wide_streams(self, level=1):
        """Streams of the most recent launch decoded at level >= `level` (1..3) of the kernel: their tables spill the LDS table
        memory of the levels below.  Level 1 = every stream that left the regular kernel."""
        return int(self._lib.brx_last_timing(self._h, 1 + level))

    def last_late_streams(self):
        """Streams of the most recent launch handed up at a LATER meta-block with their decoder state (resumed, not restarted)."""
        return int(self._lib.brx_last_timing(self._h, 6))

    def last_redo_bytes(self):
        """Output bytes of the most recent launch that were decoded twice because of hand-overs (0: all of them resumed)."""
        return int(self._lib.brx_last_timing(self._h, 7))

    def last_trace(self, n):
        """(n, 4) uint64: start, end (100 MHz realtime), place | level << 32, workgroup | grid << 32 per stream (option trace = 1).
        place: HW_ID[15:0] | XCC_ID << 16 | the wave's rank in the priority rotation << 20 | option prio_shift << 24 (include/brx.h)."""
        import numpy as np
        buf = np.zeros((n, 4), dtype=np.uint64)
        rc = self._lib.brx_last_trace(self._h, buf.ctypes.data, n)
        if rc != 0:
            raise BrxError("brx_last_trace failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))
        return buf

    def stream_short_slices(self):
        """Slices of bounded / pulled streams of this context that paused in front of an item the resident input did not hold."""
        return int(self._lib.brx_last_timing(self._h, 8))

    def last_spec_rollbacks(self):
        """Meta-blocks of the most recent launch taken back after a speculative end (the fast loop read on past the stream's input)."""
        return int(self._lib.brx_last_timing(self._h, 10))

    def last_level4(self):
        """Streams of the most recent launch that level-3 kernels handed on to the level-4 instance (tables beyond 37.6 KiB)."""
        return int(self._lib.brx_last_timing(self._h, 11))

    def slab_waits(self):
        """Waves that ever had to wait for a spill slab on this context (0 by construction since round 6: brx_last_timing 12)."""
        return int(self._lib.brx_last_timing(self._h, 12))

    def pool_slabs(self):
        """Slabs of the context's spill pool right now (brx_last_timing 13)."""
        return int(self._lib.brx_last_timing(self._h, 13))

    def facade_batches(self):
        """(batches, streams) the Read facade has launched for queued streams on this context (brx_last_timing 14 / 15)."""
        return int(self._lib.brx_last_timing(self._h, 14)), int(self._lib.brx_last_timing(self._h, 15))

    def facade_streams(self):
        """Streams in those batches, a stream queued again after status 25 counted every time (brx_last_timing 15)."""
        return int(self._lib.brx_last_timing(self._h, 15))

    def stream_regrown(self):
        """Slices of bounded / pulled streams of this context run again with a larger output buffer (one command beyond the slack)."""
        return int(self._lib.brx_last_timing(self._h, 9))

    def reader_slice_launches(self):
        """Slice launches of bounded / pulled streams on this context since it was made (brx_last_timing 16)."""
        return int(self._lib.brx_last_timing(self._h, 16))

    def reader_slices(self):
        """Slices of bounded / pulled streams in those launches (brx_last_timing 17): / reader_slice_launches() = slices per round."""
        return int(self._lib.brx_last_timing(self._h, 17))

    def advance(self, decompressors):
        """brx_stream_advance: every streaming Decompressor (or raw brx_stream handle) of this context that is unfinished and has no
        decoded bytes left to read moves on by one slice, all of them in shared launches.  -> how many moved on."""
        handles = []
        for d in decompressors:
            if isinstance(d, Decompressor):
                d.prepare()
                if d._ctx is not self:
                    raise BrxError("advance: a Decompressor of another context")
                d = d._stream
            handles.append(d)
        arr = (ctypes.c_void_p * len(handles))(*handles)
        rc = self._lib.brx_stream_advance(arr, len(handles))
        if rc < 0:
            raise BrxError("brx_stream_advance failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))
        return rc

    def last_lean_listed(self):
        """Streams of the most recent launch that the lean instance (short streams, 32 waves per CU) left to the regular kernel:
        the ones larger than its limit plus the short ones it gave up on (errors, block switches, large tables)."""
        return int(self._lib.brx_last_timing(self._h, 5))

    def synchronize(self, hip_stream=None):
        rc = self._lib.brx_synchronize(self._h, hip_stream)
        if rc != 0:
            raise BrxError("brx_synchronize failed: %s" % self._lib.brx_last_error().decode())

    def decode(self, data: bytes):
        """Decode one stream of unknown size: grow the capacity on OUTPUT_TOO_SMALL.  -> (status, bytes)."""
        cap = max(1 << 16, 8 * len(data))
        while True:
            outs, st, ln = self.decode_batch([data], [cap])
            if st[0] == OUTPUT_TOO_SMALL:
                cap = max(cap * 4, int(ln[0]))
                continue
            return int(st[0]), outs[0]


DEALS = {"ranges": 0, "bytes": 1, "snake": 2}
NODE_OPTIONS = {"transport": 100, "min_streams": 101, "exchange_root": 102}


def node_deal(sizes, gpus, deal="ranges"):
    """brx_node_deal: (order np.uint32[n], cut np.uint32[gpus + 1]) for streams of the given compressed sizes.  No GPU needed."""
    L = load_library()
    n = len(sizes)
    in_off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.asarray(sizes, dtype=np.uint64), out=in_off[1:])
    order = np.zeros(max(n, 1), dtype=np.uint32)
    cut = np.zeros(gpus + 1, dtype=np.uint32)
    rc = L.brx_node_deal(in_off.ctypes.data, n, gpus, DEALS[deal], order.ctypes.data, cut.ctypes.data)
    if rc != 0:
        raise BrxError("brx_node_deal failed (%d): %s" % (rc, L.brx_last_error().decode()))
    return order[:n], cut


class Node:
    """brx_node: the GPUs of one machine behind one call (one process, one context and one host thread per GPU).  `devices`: HIP
    device index per rank (None = every visible GPU); a device may appear more than once -- "virtual ranks", the same code on one GPU."""

    def __init__(self, devices=None, options=None):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        arr = (ctypes.c_int * len(devices))(*devices) if devices else None
        rc = self._lib.brx_node_create(ctypes.byref(self._h), arr, len(devices) if devices else 0)
        if rc != 0:
            raise BrxError("brx_node_create failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))
        for name, value in (options or {}).items():
            self.set_option(name, value)

    @property
    def size(self):
        return int(self._lib.brx_node_size(self._h))

    def set_option(self, name, value):
        opt = NODE_OPTIONS[name] if name in NODE_OPTIONS else OPTIONS[name]
        rc = self._lib.brx_node_set_option(self._h, opt, int(value))
        if rc != 0:
            raise BrxError("brx_node_set_option(%s) failed (%d): %s" % (name, rc, self._lib.brx_last_error().decode()))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.brx_node_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _opts(self, flags, deal, use_gpus, root, hip_stream, timing):
        return _NodeOpts(flags | (OPT_TIMING if timing else 0), DEALS[deal], int(use_gpus), int(root), hip_stream)

    def decode_batch(self, streams, capacities, deal="ranges", use_gpus=0, timing=False, raw=False):
        """As Context.decode_batch, over the node (host pointers: every GPU reads / writes the caller's buffers itself).  raw=True:
        outputs are the slots' bytes up to min(out_len, capacity) whatever the status (the bytes in front of an error)."""
        n = len(streams)
        if isinstance(capacities, int):
            capacities = [capacities] * n
        in_off = np.zeros(n + 1, dtype=np.uint64)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in streams], out=in_off[1:])
        np.cumsum(capacities, out=out_off[1:])
        blob = np.frombuffer(b"".join(streams), dtype=np.uint8) if in_off[-1] else np.zeros(1, dtype=np.uint8)
        out = np.zeros(max(int(out_off[-1]), 1), dtype=np.uint8)
        out_len = np.zeros(max(n, 1), dtype=np.uint64)
        status = np.full(max(n, 1), -1, dtype=np.int32)
        opts = self._opts(MEM_HOST, deal, use_gpus, 0, None, timing)
        rc = self._lib.brx_node_decode_batch(self._h, blob.ctypes.data, in_off.ctypes.data, n, out.ctypes.data, out_off.ctypes.data,
                                             out_len.ctypes.data, status.ctypes.data, ctypes.byref(opts))
        if rc != 0:
            raise BrxError("brx_node_decode_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))
        outs = []
        for i in range(n):
            ln = min(int(out_len[i]), int(capacities[i])) if (raw or status[i] == OK) else 0
            outs.append(out[int(out_off[i]):int(out_off[i]) + ln].tobytes())
        return outs, status[:n], out_len[:n]

    def decode_batch_host_raw(self, in_ptr, in_off, n, out_ptr, out_off, deal="ranges", use_gpus=0, timing=False):
        """Host pointers as they are (e.g. pinned buffers from host_alloc(): used in place by every GPU).  Returns (status, out_len)."""
        out_len = np.zeros(max(n, 1), dtype=np.uint64)
        status = np.full(max(n, 1), -1, dtype=np.int32)
        opts = self._opts(MEM_HOST, deal, use_gpus, 0, None, timing)
        rc = self._lib.brx_node_decode_batch(self._h, in_ptr, in_off.ctypes.data, n, out_ptr, out_off.ctypes.data,
                                             out_len.ctypes.data, status.ctypes.data, ctypes.byref(opts))
        if rc != 0:
            raise BrxError("brx_node_decode_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))
        return status[:n], out_len[:n]

    def decode_batch_device(self, in_ptr, in_off_ptr, n, out_ptr, out_off_ptr, out_len_ptr, status_ptr, deal="ranges", use_gpus=0,
                            root=0, hip_stream=None, timing=False):
        """Every pointer is memory of the root rank's GPU: scatter over xGMI, decode everywhere, ragged gather.  Returns when done."""
        opts = self._opts(MEM_DEVICE, deal, use_gpus, root, hip_stream, timing)
        rc = self._lib.brx_node_decode_batch(self._h, in_ptr, in_off_ptr, n, out_ptr, out_off_ptr, out_len_ptr, status_ptr,
                                             ctypes.byref(opts))
        if rc != 0:
            raise BrxError("brx_node_decode_batch failed (%d): %s" % (rc, self._lib.brx_last_error().decode()))

    def last(self):
        """Of the most recent batch: {gpus, streams[], in_bytes[], kernel_ms[], wall_ms, scatter_ms, rccl}."""
        t = lambda which, rank=0: float(self._lib.brx_node_last_timing(self._h, which, rank))  # noqa: E731
        g = int(t(0))
        return {"gpus": g, "streams": [int(t(1, r)) for r in range(g)], "in_bytes": [int(t(2, r)) for r in range(g)],
                "kernel_ms": [t(3, r) for r in range(g)], "wall_ms": t(4), "scatter_ms": t(5), "rccl": bool(t(6))}


def host_alloc(nbytes):
    """Pinned host memory from the library (brx_host_alloc) as a numpy uint8 view; free with host_free(view)."""
    L = load_library()
    p = L.brx_host_alloc(nbytes)
    if not p:
        raise BrxError("brx_host_alloc(%d) failed: %s" % (nbytes, L.brx_last_error().decode()))
    arr = np.ctypeslib.as_array((ctypes.c_ubyte * nbytes).from_address(p))
    arr = arr.view(np.uint8)
    _PINNED[arr.ctypes.data] = p
    return arr


def host_free(arr):
    p = _PINNED.pop(arr.ctypes.data, None)
    if p:
        load_library().brx_host_free(p)


_PINNED = {}
_default_ctx = None


def advance(streams):
    """Context.advance over the context of the streams (streaming Decompressors, all on one context)."""
    streams = list(streams)
    if not streams:
        return 0
    for d in streams:
        d.prepare()
    return streams[0]._ctx.advance(streams)


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class Decompressor(io.RawIOBase):
    """Mirror of `brotli::Decompressor<R: Read>` (reference src/lib.rs:377-410): wraps a reader of compressed
    bytes and is itself a reader of decompressed bytes.

        Decompressor(open("x.compressed", "rb")).read()        # == read_to_end

    Semantics of `read` follow the reference's `impl Read` (src/lib.rs:2173-2193): n > 0 bytes, b"" at end of
    stream forever after, and an error carrying the reference's description string for invalid input --
    raised as ValueError here (the reference returns io::ErrorKind::InvalidData).  Differences, documented
    in INTEGRATION.md: the inner reader is drained eagerly on the first read; a stream that fails serves the bytes
    decoded before the error first and raises afterwards (the reference delivers a prefix too).  The object
    keeps its context alive; should the context be closed explicitly first, later reads raise BrxError.
    """

    def __init__(self, reader, ctx: Context = None, streaming: bool = False):
        """streaming=True: the inner reader is PULLED while the stream decodes (brx_stream_new_reader: compressed input and output
        both in bounded sliding windows on the device, any stream length) instead of being drained on the first read."""
        super().__init__()
        self._reader = reader
        self._ctx = ctx
        self._stream = None
        self._lib = load_library()
        self._streaming = streaming
        self._cb = None

    def readable(self):
        return True

    def prepare(self):
        """Drain the inner reader and queue the stream on its context WITHOUT decoding: the first read of any queued
        stream then decodes all of them in one batch (many live Decompressors cost about one batch)."""
        if self._stream is None and self._streaming:
            self._ctx = self._ctx or default_context()
            reader = self._reader

            def pull(_user, buf, cap):
                try:
                    data = reader.read(cap)
                except Exception:  # an exception must not cross the C ABI: the stream ends here (UnexpectedEOF if it was not done)
                    return 0
                n = len(data) if data else 0
                if n:
                    ctypes.memmove(buf, bytes(data), n)
                return n

            self._cb = READ_FN(pull)  # (kept alive as long as the stream)
            self._stream = self._lib.brx_stream_new_reader(self._ctx._h, self._cb, None)
            if not self._stream:
                raise BrxError("brx_stream_new_reader failed")
        if self._stream is None:
            data = self._reader.read() if hasattr(self._reader, "read") else bytes(self._reader)
            self._ctx = self._ctx or default_context()  # (held: the context must outlive the stream object)
            self._stream = self._lib.brx_stream_new(self._ctx._h, data, len(data))
            if not self._stream:
                raise BrxError("brx_stream_new failed")
        return self

    def ready(self):
        """Decoded bytes a read hands out without decoding anything (brx_stream_ready; between advance() calls)."""
        self.prepare()
        return int(self._lib.brx_stream_ready(self._stream))

    def readinto(self, b):
        self.prepare()
        mv = memoryview(b).cast("B")
        buf = (ctypes.c_ubyte * len(mv)).from_buffer(mv) if len(mv) else None
        n = self._lib.brx_stream_read(self._stream, buf, len(mv))
        if n < -900:
            raise BrxError("libbrx failure: %s" % self._lib.brx_last_error().decode())
        if n < 0:
            raise ValueError(status_str(-n))  # InvalidData + description, src/lib.rs:2177
        return int(n)

    def close(self):
        if self._stream:
            self._lib.brx_stream_free(self._stream)
            self._stream = None
        super().close()
