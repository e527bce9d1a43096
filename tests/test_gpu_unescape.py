"""brx_unescape_batch (include/brx.h, brx_unescape.hip): every selected record of the decoded streams of a batch as the string it spells:
the text's length, a status byte and the text's bytes in a destination.  Every expected value comes from tests/unescape_oracle.py (its
two forms are held to each other, to the contract's table and to json / csv by tests/test_unescape_abi.py), the records from
tests/take_oracle.py.  text_len and status are pre-filled with sentinels and carry spare entries behind m, which must keep them; dst is
pre-filled with a sentinel that every byte outside the texts' places must keep.  In-process, one context."""
import numpy as np
import pytest

import brx_knobs
import unescape_oracle as uo
from brotli_rs_amd.brx import TEXT_BACKSLASH, TEXT_BAD, TEXT_BARE, TEXT_CSV, TEXT_JSON, TEXT_NULL, TEXT_OK  # noqa: F401  (without the call nothing here runs)

pytestmark = pytest.mark.gpu

SENT = -7      # the sentinel of text_len
SENT8 = 0xA5   # the sentinel of status and of dst
SPARE = 8
NO_DELIM, TRIM_CR, SPACES = 1, 2, 16
QT, ESC = uo.QT, uo.ESC
CSV, JSON, BSL = uo.CSV, uo.JSON, uo.BACKSLASH
DIALECTS = (CSV, JSON, BSL)
LONG = 512  # BRX_TEXT_LONG (csrc/brx_unescape.h)
ROW = 1024


@pytest.fixture(scope="module")
def ctx():
    c = brx_knobs.context(0)
    yield c
    c.close()


def test_the_threshold_is_the_headers():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "brotli-rs_amd", "csrc", "brx_unescape.h")).read()
    assert int(re.search(r"#define\s+BRX_TEXT_LONG\s+(\d+)u", text).group(1)) == LONG
    assert (TEXT_CSV, TEXT_JSON, TEXT_BACKSLASH, TEXT_OK, TEXT_BARE, TEXT_NULL, TEXT_BAD) == (CSV, JSON, BSL, uo.OK, uo.BARE, uo.NULL, uo.BAD)


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a))  # (a writable copy)
    return (t.to(dtype) if dtype is not None else t).to("cuda:0")


def _np(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


class Batch:
    """An arena on the host and on the device with its tables, and the positions of an index at `delims` (or whatever the test puts
    in their place)."""

    def __init__(self, host, offs, lens, delims=b"\n", positions=None):
        import take_oracle
        self.host = np.ascontiguousarray(host, dtype=np.uint8)
        self.offs, self.lens = np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64)
        self.n = len(self.lens)
        self.count, self.pos_off, self.pos = positions if positions is not None else take_oracle.index_positions(self.host, offs, lens, delims)
        self.n_pos = len(self.pos)
        self.arena = _dev(self.host)
        self.d_off, self.d_len = _dev(self.offs), _dev(self.lens)
        self.d_count, self.d_pos_off = _dev(np.asarray(self.count, dtype=np.int64)), _dev(np.asarray(self.pos_off, dtype=np.int64))
        self.d_pos = _dev(np.asarray(self.pos, dtype=np.int64)) if len(self.pos) else None

    def head(self):
        return (self.arena.data_ptr(), self.d_off.data_ptr(), self.d_len.data_ptr(), self.n, int(self.arena.numel()),
                self.d_count.data_ptr(), self.d_pos_off.data_ptr(), self.d_pos.data_ptr() if self.d_pos is not None else None, self.n_pos)

    def tensors(self):
        import torch
        return (self.arena, self.d_off, self.d_len, self.d_count, self.d_pos_off,
                self.d_pos if self.d_pos is not None else torch.zeros(0, dtype=torch.int64, device="cuda:0"))


def _lines(records, pad=3, tail=3, copies=1):
    """`copies` streams, each the records followed by "\\n" each (so the trailing record is empty); stream p starts at source phase
    (pad + p) % 16 of the arena, with bytes that are escapes around it."""
    s = b"".join(bytes(r) + b"\n" for r in records)
    slot = (len(s) + 48) // 16 * 16
    offs = [pad + p * slot + p for p in range(copies)]
    host = np.full(offs[-1] + len(s) + tail, ESC, dtype=np.uint8)
    for o in offs:
        host[o:o + len(s)] = _np(s)
    return Batch(host, offs, [len(s)] * copies)


def _want(b, D, flags, dialect, q, e, sel, m, form):
    if sel is not None:
        si, sk = np.asarray(sel[0], dtype=np.int64), np.asarray(sel[1], dtype=np.int64)
        return uo.unescape_take(form, b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, D, flags, dialect, q, e, si & 0xFFFFFFFF, sk) + (len(si),)
    if m is None:
        m = int(np.sum(b.count)) + b.n
    return uo.unescape_take(form, b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, D, flags, dialect, q, e, m=m) + (m,)


def _check(ctx, b, dialect, flags=NO_DELIM, q=QT, e=ESC, D=1, sel=None, m=None, form="serial", dst_off=None, total=None, phase=0,
           modes=("size", "fill", "bare")):
    """One selection against the oracle in up to three calls: size mode; fill mode with text_len and status; fill mode without them.
    dst_off / total default to the texts back to back; `phase` is the destination's address mod 16.  -> (texts, text_len, status, L)"""
    import torch
    texts, tl, st, L, m = _want(b, D, flags, dialect, q, e, sel, m, form)
    sel_ptrs = (None, None)
    if sel is not None:
        d_ss, d_sr = _dev(np.asarray(sel[0], dtype=np.int64), torch.int32), _dev(np.asarray(sel[1], dtype=np.int64))
        sel_ptrs = (d_ss.data_ptr(), d_sr.data_ptr())
    if dst_off is None:
        dst_off = np.cumsum(tl) - tl
    dst_off = np.asarray(dst_off, dtype=np.int64)
    if total is None:
        total = int(tl.sum())
    tag = (dialect, flags, q, e, sel is not None, m, total, phase)
    args = b.head() + (D, flags) + sel_ptrs + (m, dialect, q, e)
    expect = uo.fill(texts, dst_off, total, np.full(total + 64, SENT8, dtype=np.uint8))
    d_off = _dev(dst_off) if m else None
    for mode in modes:
        out_len = torch.full((m + SPARE,), SENT, dtype=torch.int64, device="cuda:0")
        out_st = torch.full((m + SPARE,), SENT8, dtype=torch.uint8, device="cuda:0")
        dst = torch.full((total + 64 + 16,), SENT8, dtype=torch.uint8, device="cuda:0")
        assert dst.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        outs = (None, None) if mode == "bare" else (out_len.data_ptr(), out_st.data_ptr())
        fill = () if mode == "size" else (d_off.data_ptr() if m else dst.data_ptr(), dst.data_ptr() + phase, total)
        ctx.unescape_batch_device(*args, *outs, *fill)
        gl, gs, gd = out_len.cpu().numpy(), out_st.cpu().numpy(), dst.cpu().numpy()
        assert (gl[m:] == SENT).all() and (gs[m:] == SENT8).all(), (tag, mode)
        if mode == "bare":
            assert (gl == SENT).all() and (gs == SENT8).all(), (tag, mode)
        else:
            bad = np.flatnonzero((gl[:m] != tl) | (gs[:m] != st))
            assert bad.size == 0, (tag, mode, bad[:8].tolist(), L[bad[:8]].tolist(), gl[bad[:8]].tolist(), tl[bad[:8]].tolist(),
                                   gs[bad[:8]].tolist(), st[bad[:8]].tolist())
        if mode == "size":
            assert (gd == SENT8).all(), (tag, mode)
        else:
            assert (gd[:phase] == SENT8).all() and (gd[phase + total + 64:] == SENT8).all(), (tag, mode)
            bad = np.flatnonzero(gd[phase:phase + total + 64] != expect)
            assert bad.size == 0, (tag, mode, bad[:8].tolist(), gd[phase:][bad[:8]].tolist(), expect[bad[:8]].tolist(),
                                   (np.searchsorted(dst_off, bad[:8], side="right") - 1).tolist())
    return texts, tl, st, L


# 1 -------------------------------------------------------------------------------------------------------------------------------
def test_check_values_in_both_selection_modes_and_through_the_wrappers(ctx):
    """The contract's table, every value, each as a record of its own, per dialect, with and without BRX_PARSE_SPACES, in all-records
    mode and in pairs mode (reversed, so the texts land in another order), and through unescape_batch with and without a stride."""
    import torch
    recs = [c[2] for c in uo.CHECK]
    b = _lines(recs)
    m = len(recs) + 1
    rev = (np.zeros(m, dtype=np.int64), np.arange(m - 1, -1, -1))
    name = {CSV: "csv", JSON: "json", BSL: "backslash"}
    for dialect in DIALECTS:
        for sp in (0, SPACES):
            texts, tl, st, L = _check(ctx, b, dialect, NO_DELIM | sp)
            assert L.tolist() == [len(r) for r in recs] + [0]
            for j, c in enumerate(uo.CHECK):
                if c[0] == dialect and (c[1] == bool(sp) or not c[1] and c[2].strip(b" \t") == c[2]):
                    assert (texts[j], int(st[j])) == c[3:], c
            rt, rl, rs, _ = _check(ctx, b, dialect, NO_DELIM | sp, sel=rev)
            assert rt == texts[::-1] and rs.tolist() == st.tolist()[::-1]
            dst, dst_off, text_len, status = ctx.unescape_batch(*b.tensors(), dialect=name[dialect], spaces=bool(sp))
            assert (dst.dtype, dst_off.dtype, text_len.dtype, status.dtype) == (torch.uint8, torch.int64, torch.int64, torch.uint8)
            assert text_len.cpu().tolist() == tl.tolist() and status.cpu().tolist() == st.tolist()
            assert dst.cpu().numpy().tobytes() == b"".join(texts) and dst_off.cpu().tolist() == (np.cumsum(tl) - tl).tolist()
            dst, dst_off, text_len, status = ctx.unescape_batch(*b.tensors(), dialect=name[dialect], spaces=bool(sp), stride=3,
                                                                sel_stream=_dev(rev[0]), sel_rec=_dev(rev[1]))
            assert text_len.cpu().tolist() == rl.tolist() and status.cpu().tolist() == rs.tolist()
            assert dst.cpu().numpy().tobytes() == b"".join(t[:3].ljust(3, b"\0") for t in rt)


# 2 -------------------------------------------------------------------------------------------------------------------------------
def test_runs_across_unit_and_row_boundaries_at_every_source_phase(ctx):
    """Runs of 1 .. 40 escape bytes (JSON, BACKSLASH) and of 1 .. 40 quotes inside a CSV body, placed so that the run crosses the unit
    boundary at 16 (short records: the lane path) and the row boundary at 1024 (long ones: the wave path; runs above 16 bytes also
    fill whole units), at each of the 16 source phases; even and odd runs, followed by a letter, by 'n' and by the closing quote."""
    for dialect in DIALECTS:
        run = bytes([QT if dialect == CSV else ESC])
        opening = b"" if dialect == BSL else b'"'
        recs = []
        for k in range(1, 41):
            for edge in (16, ROW):
                start = edge - max((k + 1) // 2, 1)  # the run begins in front of the edge and, for k > 1, crosses it
                body = b"a" * (start - len(opening)) + run * k + (b"n", b"x", b"")[k % 3] + b"tail"
                recs.append(opening + body + opening)
        b = _lines(recs, pad=0, copies=16)
        texts, tl, st, L = _check(ctx, b, dialect, modes=("size", "fill"))
        assert uo.OK in st and (uo.BAD in st or dialect == BSL) and (L >= LONG).sum() >= 16 * 40  # (an escape byte always finds a byte to escape here)


# 3 -------------------------------------------------------------------------------------------------------------------------------
def test_unicode_escapes_across_boundaries_and_cut_by_the_records_end(ctx):
    """A \\uXXXX escape and a surrogate pair whose 6 / 12 bytes straddle the unit boundary at 16 and the row boundaries at 1024 and 2048
    at every offset, and the same with the record ending at every offset inside them (with and without a closing quote)."""
    pair, bmp = b"\\ud83d\\ude00", b"\\u20AC"
    recs = []
    for edge in (16, ROW, 2 * ROW):
        for esc in (pair, bmp, b"\\udE00", b"\\ud83d\\u0041", pair + pair):
            for back in range(0, len(esc) + 1):
                recs.append(b'"' + b"b" * (edge - back - 1) + esc + b'z"')
        for cut in range(0, 13):
            for close in (b"", b'"'):
                recs.append(b'"' + b"c" * (edge - 1 - cut // 2) + pair[:cut] + close)
    b = _lines(recs, pad=5)
    texts, tl, st, L = _check(ctx, b, JSON, modes=("size", "fill"))
    assert (st == uo.OK).sum() > 50 and (st == uo.BAD).sum() > 50
    _check(ctx, b, BSL, modes=("fill",))  # the same bytes as backslash text: \u is u


# 4 -------------------------------------------------------------------------------------------------------------------------------
def test_record_lengths_around_every_threshold(ctx):
    """Record lengths 0, 1, 2, 15, 16, 17, BRX_TEXT_LONG - 1, BRX_TEXT_LONG, BRX_TEXT_LONG + 1 (and + 2, + 3: the walk range is up to two
    bytes shorter than the record) and two rows + 1: once as pure copy, once with an escape in every unit."""
    lens = (0, 1, 2, 15, 16, 17, LONG - 1, LONG, LONG + 1, LONG + 2, LONG + 3, 2 * ROW + 1)
    for dialect in DIALECTS:
        q = b"" if dialect == BSL else b'"'
        piece = {CSV: b'ab""cdefgh', JSON: b"ab\\ncd\\u00e9gh\\\\", BSL: b"ab\\tcdefg\\\\"}[dialect]
        recs = []
        for n in lens:
            quoted = n >= 2 and dialect != BSL
            recs.append(b"p" * n)                                                      # pure copy, bare
            recs.append(q + b"p" * (n - 2) + q if quoted else b"p" * n)                # pure copy, quoted where there is room
            recs.append(q + (piece * (n // len(piece) + 1))[:n - 2] + q if quoted else (piece * (n // len(piece) + 1))[:n])  # escapes in every unit
        assert sorted(set(len(r) for r in recs)) == sorted(lens)
        texts, tl, st, L = _check(ctx, _lines(recs, pad=7), dialect)
        assert sorted(set(L.tolist())) == sorted(lens)
        _check(ctx, _lines(recs, pad=0), dialect, NO_DELIM | SPACES, modes=("fill",))


# 5 -------------------------------------------------------------------------------------------------------------------------------
def test_one_wave_of_short_and_long_records_in_random_order(ctx):
    """Pairs mode over three streams: short and long records in one wave, in random order, with repeats, with entries whose stream or
    record does not exist, a ragged last wave."""
    rng = np.random.default_rng(5)
    for dialect in DIALECTS:
        recs = [uo.rich_record(rng, int(n), dialect, rich=0.3) for n in (0, 3, 40, 700, 17, LONG, 2500, 90, LONG - 1, 1030, 5, 1500)]
        b = _lines(recs, pad=9, copies=3)
        si = rng.integers(0, 5, 150)             # 3 and 4: no such stream
        sk = rng.integers(0, len(recs) + 4, 150)  # above len(recs): no such record
        texts, tl, st, L = _check(ctx, b, dialect, sel=(si, sk))
        assert (L >= LONG).sum() > 20 and (L == 0).sum() > 20 and ((L > 0) & (L < LONG)).sum() > 20


# 6 -------------------------------------------------------------------------------------------------------------------------------
def test_rooms_strides_totals_and_destination_phases(ctx):
    """Packed and strided destinations; rooms of 0 and 1 bytes; rooms that cut inside an escape's output (the 4 bytes of a pair, at
    every byte); a total that ends inside a text; all 16 destination phases."""
    rng = np.random.default_rng(6)
    pair = b"\\ud83d\\ude00"
    recs = [b'"' + pair + b'"', b'"ab' + pair + b'cd"', b'"\\u20ac"', b'""', b"null", b'"' + b"x" * 40 + pair * 3 + b'"',
            b'"' + (b"y" * 15 + pair) * 70 + b'"', b'"' + b"z" * 1500 + b'"', b'"\\n"'] + [uo.rich_record(rng, int(n), JSON) for n in (30, 600, 2100)]
    b = _lines(recs, pad=2)
    m = len(recs) + 1
    texts, tl, st, L = _check(ctx, b, JSON)
    for stride in (0, 1, 2, 3, 5, 16, 17, 100, 2200):
        _check(ctx, b, JSON, dst_off=np.arange(m) * stride, total=m * stride, phase=stride % 16, modes=("fill",))
    for phase in range(16):
        _check(ctx, b, JSON, phase=phase, total=int(tl.sum()) - (phase * 37) % 60, modes=("fill", "bare")[phase % 2:][:1])
    for cut in range(0, 8):  # every room `cut` bytes short: the first text is the pair alone, the second has it at bytes 2 .. 5
        rooms = np.maximum(tl - cut, 0)
        _check(ctx, b, JSON, dst_off=np.cumsum(rooms) - rooms, total=int(rooms.sum()), modes=("fill",), phase=cut)
    _check(ctx, b, JSON, total=0, modes=("fill",))
    _check(ctx, b, JSON, dst_off=np.full(m, 7), total=9, modes=("fill",))  # every room but the last is empty, the last has 2 bytes
    for dialect in (CSV, BSL):
        r2 = [uo.rich_record(rng, int(n), dialect) for n in (0, 1, 2, 33, 600, 1300)]
        b2 = _lines(r2, pad=11)
        _check(ctx, b2, dialect, dst_off=np.arange(7) * 70, total=7 * 70 - 5, phase=13, modes=("fill",))


# 7 -------------------------------------------------------------------------------------------------------------------------------
def test_records_at_the_arenas_first_and_last_bytes(ctx):
    """The arena is one stream is one record of 1 .. 40 bytes that touches the arena's first and last byte (below 16 bytes every byte is
    fetched on its own), and a long one; then a stream whose last record lies in the arena's last 15 bytes."""
    rng = np.random.default_rng(7)
    for size in list(range(1, 41)) + [LONG + 5, ROW + 16]:
        dialect = DIALECTS[size % 3]
        text = uo.rich_record(rng, size, dialect)
        t = Batch(_np(text), [0], [size], delims=b"\n")
        texts, tl, st, L = _check(ctx, t, dialect, flags=(0, NO_DELIM, NO_DELIM | SPACES)[size % 3], modes=("fill",))
        assert L.tolist() == [size]
    for last in range(1, 16):
        s = b'"first\\n"\n' + b"a" * 40 + b"\n" + (b'"\\u00e9\\ud83d\\ude00\\\\\\\\"')[:last]
        _check(ctx, Batch(_np(s), [0], [len(s)]), JSON, modes=("size", "fill"))


# 8 -------------------------------------------------------------------------------------------------------------------------------
def test_stale_decreasing_and_garbage_positions(ctx):
    """pos that is stale, decreasing or garbage, count that overstates pos, pos_off beyond n_pos: the result is the oracle's over the
    clamped records, and nothing outside a stream is loaded (an escape's look-ahead included: the arena around the streams is all
    escape bytes)."""
    rng = np.random.default_rng(8)
    streams = [b"".join(uo.rich_record(rng, int(rng.integers(0, 60)), JSON) + b"\n" for _ in range(12)) for _ in range(6)]
    lens = np.array([len(s) for s in streams], dtype=np.int64)
    offs = np.cumsum(lens + 5) - lens
    host = np.full(int(offs[-1] + lens[-1]) + 3, ESC, dtype=np.uint8)
    for o, s in zip(offs, streams):
        host[o:o + len(s)] = _np(s)
    good = Batch(host, offs, lens)
    for variant in range(5):
        count, pos_off, pos = good.count.copy(), good.pos_off.copy(), good.pos.copy()
        if variant == 0:
            pos = pos[::-1].copy()                               # decreasing
        elif variant == 1:
            pos = rng.integers(0, 1 << 40, len(pos))             # garbage
        elif variant == 2:
            count = count + 7                                    # overstates pos: positions of the next stream, then none
        elif variant == 3:
            pos = np.roll(pos, 5)                                # stale: another batch's positions
        else:
            pos_off = pos_off + len(pos) - 3                     # mostly behind n_pos
        b = Batch(host, offs, lens, positions=(count, pos_off, pos))
        for dialect, flags in ((JSON, NO_DELIM), (BSL, 0), (CSV, NO_DELIM | TRIM_CR | SPACES)):
            _check(ctx, b, dialect, flags, modes=("size", "fill"), m=int(count.sum()) + b.n + 3)


# 9 -------------------------------------------------------------------------------------------------------------------------------
def test_other_quote_and_escape_bytes(ctx):
    """Quote and escape bytes that are letters of the escapes themselves: 'u', 'n', a digit as the quote, 0 and 0xFF, and a hex digit
    as the JSON escape (walked by one lane per record, also the long ones)."""
    rng = np.random.default_rng(9)
    for q, e in ((0x27, 0x5E), (0x75, 0x5C), (0x22, 0x75), (0x39, 0x61), (0x22, 0x46), (0x62, 0x6E), (0, 0xFF)):
        for dialect in DIALECTS:
            recs = [uo.rich_record(rng, int(n), dialect, q, e) for n in list(rng.integers(0, 70, 40)) + [LONG + 9, 1100, 2300]]
            _check(ctx, _lines(recs, pad=4), dialect, q=q, e=e, form="re", modes=("size", "fill"))


# 10 ------------------------------------------------------------------------------------------------------------------------------
def _jsonl_batch(rng, n_streams, rows):
    streams, values = [], []
    for i in range(n_streams):
        s = b""
        for r in range(int(rows[i])):
            v = uo.rich_record(rng, int(np.exp(rng.uniform(np.log(2), np.log(1500)))), JSON, rich=0.1, quoted=1.0)
            if r % 11 == 0:  # long and well-formed: the wave path
                v = b'"' + b"long text \\n \\u00e9 \\ud83d\\ude00 " * int(rng.integers(20, 60)) + b'"'
            if uo.text_serial(v, JSON)[1] != uo.OK:  # (an unclosed string would hide the row's structure from the index)
                v = b'"plain %d"' % r
            values.append(v)
            s += b'{"id": %d, "text": %s}\n' % (r, v)
        streams.append(s)
    lens = np.array([len(s) for s in streams], dtype=np.int64)
    offs = np.cumsum(lens + 7) - lens
    host = np.full(int(offs[-1] + lens[-1]) + 7, 0x20, dtype=np.uint8)
    for o, s in zip(offs, streams):
        host[o:o + len(s)] = _np(s)
    return host, offs, lens, values


def test_json_lines_end_to_end_through_the_wrapper(ctx):
    """64 streams of about 32 JSON Lines rows {"id": .., "text": ".."}, uploaded (no fixture under tests/golden/ is JSON Lines), indexed
    on the device at the structural bytes, the text values selected as the wrapper's docstring shows and unescaped with stride=None
    and with a stride; against json.loads of every row as well."""
    import json
    import torch
    rng = np.random.default_rng(10)
    rows = rng.integers(28, 37, 64)
    host, offs, lens, values = _jsonl_batch(rng, 64, rows)
    arena, d_off, d_len = _dev(host), _dev(offs), _dev(lens)
    count, _, pos_off, pos, what = ctx.index_set_batch(arena, d_off, d_len, delims=b"{}[]:,\n")
    assert count.cpu().tolist() == (rows * 6).tolist()
    streams = torch.repeat_interleave(torch.arange(count.numel(), device="cuda:0"), count + 1)
    rec = torch.arange(streams.numel(), device="cuda:0") - (pos_off + torch.arange(count.numel(), device="cuda:0"))[streams]
    pick = rec % 6 == 4
    dst, dst_off, text_len, status = ctx.unescape_batch(arena, d_off, d_len, count, pos_off, pos, sel_stream=streams[pick],
                                                        sel_rec=rec[pick], dialect="json", spaces=True)
    want = [uo.text_serial(v, JSON)[0] for v in values]
    assert status.cpu().tolist() == [uo.OK] * len(values) and text_len.cpu().tolist() == [len(w) for w in want]
    assert dst.cpu().numpy().tobytes() == b"".join(want)
    assert max(len(w) for w in want) >= LONG and min(len(w) for w in want) < 16
    lines = b"".join(host[o:o + n].tobytes() for o, n in zip(offs, lens)).split(b"\n")[:-1]
    assert [json.loads(ln.decode("ascii"), strict=False)["text"].encode("utf-8") for ln in lines if ln] == want
    S = 48
    dst, dst_off, text_len, status = ctx.unescape_batch(arena, d_off, d_len, count, pos_off, pos, sel_stream=streams[pick],
                                                        sel_rec=rec[pick], dialect="json", spaces=True, stride=S)
    assert text_len.cpu().tolist() == [len(w) for w in want] and dst_off.cpu().tolist() == [j * S for j in range(len(want))]
    assert dst.cpu().numpy().tobytes() == b"".join(w[:S].ljust(S, b"\0") for w in want)
    # all-records mode: keys, numbers and the empty pieces come out BARE, as they stand
    dst, dst_off, text_len, status = ctx.unescape_batch(arena, d_off, d_len, count, pos_off, pos, dialect="json", spaces=True)
    st = status.cpu().numpy()
    assert (st == uo.BARE).sum() == 3 * len(values) + 64 and (st == uo.OK).sum() == 3 * len(values)


# 11 ------------------------------------------------------------------------------------------------------------------------------
def test_enqueued_behind_index_set_batch_on_a_callers_stream(ctx):
    """brx_index_set_batch in count mode, torch.cumsum, fill mode, brx_unescape_batch in size mode, torch.cumsum and brx_unescape_batch in
    fill mode on a caller's HIP stream, nothing in between."""
    import torch
    rng = np.random.default_rng(11)
    recs = [uo.rich_record(rng, int(n), BSL, rich=0.25).replace(b"\n", b"") for n in list(rng.integers(0, 90, 300)) + [700, 1500, 2600]]
    b = _lines(recs, pad=1, copies=2)
    n, total = b.n, b.n_pos
    m = total + n
    count = torch.full((n,), SENT, dtype=torch.int64, device="cuda:0")
    pos = torch.full((total,), SENT, dtype=torch.int64, device="cuda:0")
    tlen = torch.full((m + SPARE,), SENT, dtype=torch.int64, device="cuda:0")
    stat = torch.full((m + SPARE,), SENT8, dtype=torch.uint8, device="cuda:0")
    texts, tl, st, L = uo.unescape_take("re", b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, total, 1, NO_DELIM, BSL)
    room = int(tl.sum())
    dst = torch.full((room + 64,), SENT8, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        head = (b.arena.data_ptr(), b.d_off.data_ptr(), b.d_len.data_ptr(), n, int(b.arena.numel()))
        ctx.index_set_batch_device(b"\n", 0, 0, 3, *head, count.data_ptr(), hip_stream=s.cuda_stream)
        pos_off = torch.cumsum(count, 0) - count
        ctx.index_set_batch_device(b"\n", 0, 0, 3, *head, None, None, pos_off.data_ptr(), pos.data_ptr(), None, total, hip_stream=s.cuda_stream)
        tail = (count.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), total, 1, NO_DELIM, None, None, m, BSL, QT, ESC)
        ctx.unescape_batch_device(*head, *tail, tlen.data_ptr(), stat.data_ptr(), hip_stream=s.cuda_stream)
        dst_off = torch.cumsum(tlen[:m], 0) - tlen[:m]
        ctx.unescape_batch_device(*head, *tail, None, None, dst_off.data_ptr(), dst.data_ptr(), room, hip_stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(pos.cpu().numpy(), b.pos) and np.array_equal(count.cpu().numpy(), b.count)
    gl, gs, gd = tlen.cpu().numpy(), stat.cpu().numpy(), dst.cpu().numpy()
    assert np.array_equal(gl[:m], tl) and np.array_equal(gs[:m], st) and (gl[m:] == SENT).all() and (gs[m:] == SENT8).all()
    assert gd[:room].tobytes() == b"".join(texts) and (gd[room:] == SENT8).all()
    assert (L >= LONG).sum() == 6 and {uo.OK, uo.BAD} <= set(st.tolist())


# 12 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dialect", DIALECTS)
def test_differential_fuzz(ctx, dialect):
    """2000 random records from the rich alphabet, lengths 0 .. 3 rows, in all-records mode over 8 streams; with and without
    BRX_PARSE_SPACES (the records then carry blanks around them)."""
    rng = np.random.default_rng(120 + dialect)
    recs = []
    for it in range(2000):
        n = int(rng.integers(0, 80)) if it % 4 else int(rng.integers(0, 3 * ROW + 1))
        r = uo.rich_record(rng, n, dialect, rich=float(rng.uniform(0.05, 0.9)))
        recs.append(b" \t "[:it % 4 if it % 3 == 0 else 0] + r + b"\t "[:it % 3 if it % 5 == 0 else 0])
    recs[7], recs[8] = b"\\N", b" \\N\t"
    streams = [b"".join(r + b"\n" for r in recs[i::8]) for i in range(8)]
    lens = np.array([len(s) for s in streams], dtype=np.int64)
    offs = np.cumsum(lens + 3) - lens
    host = np.full(int(offs[-1] + lens[-1]) + 1, ESC, dtype=np.uint8)
    for o, s in zip(offs, streams):
        host[o:o + len(s)] = _np(s)
    b = Batch(host, offs, lens)
    for flags in (NO_DELIM, NO_DELIM | SPACES):
        texts, tl, st, L = _check(ctx, b, dialect, flags, form="re", modes=("size", "fill"), phase=5)
        assert len(set(st.tolist())) == 3 and (L >= LONG).sum() > 200


# 13 ------------------------------------------------------------------------------------------------------------------------------
def test_an_empty_selection_and_the_refusals_on_a_live_context(ctx):
    """m = 0: BRX_SUCCESS and nothing launched, raw and through the wrapper; the refusals leave the context working."""
    import torch
    from brotli_rs_amd import brx
    b = _lines([b'"a\\nb"', b"7"], pad=0, tail=0)
    tl = torch.full((4,), SENT, dtype=torch.int64, device="cuda:0")
    st = torch.full((4,), SENT8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert ctx._lib.brx_unescape_batch(ctx._h, *b.head(), 1, 0, None, None, 0, JSON, QT, ESC, tl.data_ptr(), st.data_ptr(), None, None, 0, None) == 0
    ctx.synchronize()
    assert tl.cpu().tolist() == [SENT] * 4 and st.cpu().tolist() == [SENT8] * 4
    none = torch.zeros(0, dtype=torch.int64, device="cuda:0")
    for stride in (None, 8):
        dst, dst_off, text_len, status = ctx.unescape_batch(*b.tensors(), sel_stream=none.to(torch.int32), sel_rec=none, stride=stride)
        assert dst.numel() == 0 and dst_off.numel() == 0 and text_len.numel() == 0 and status.numel() == 0 and status.dtype == torch.uint8
    tail = (None, None, 3)
    out = (tl.data_ptr(), st.data_ptr())
    with pytest.raises(brx.BrxError, match="brx_unescape_batch: BRX_TAKE_TRIM_CR"):
        ctx.unescape_batch_device(*b.head(), 1, TRIM_CR, *tail, JSON, QT, ESC, *out)
    for bad in (32, 64, 128):
        with pytest.raises(brx.BrxError, match="brx_unescape_batch: unknown flag bits"):
            ctx.unescape_batch_device(*b.head(), 1, bad, *tail, JSON, QT, ESC, *out)
    with pytest.raises(brx.BrxError, match="brx_unescape_batch: dialect is not"):
        ctx.unescape_batch_device(*b.head(), 1, 0, *tail, 3, QT, ESC, *out)
    with pytest.raises(brx.BrxError, match="brx_unescape_batch: quote or escape"):
        ctx.unescape_batch_device(*b.head(), 1, 0, *tail, JSON, 256, ESC, *out)
    with pytest.raises(brx.BrxError, match="quote == escape"):
        ctx.unescape_batch_device(*b.head(), 1, 0, *tail, JSON, QT, QT, *out)
    with pytest.raises(brx.BrxError, match="NULL in size mode"):
        ctx.unescape_batch_device(*b.head(), 1, 0, *tail, JSON, QT, ESC, tl.data_ptr(), None)
    for kw in (dict(keep_delim=True, trim_cr=True), dict(dialect="yaml")):
        with pytest.raises(brx.BrxError):
            ctx.unescape_batch(*b.tensors(), **kw)
    assert tl.cpu().tolist() == [SENT] * 4 and st.cpu().tolist() == [SENT8] * 4
    texts, wl, ws, L = _check(ctx, b, JSON)
    assert texts == [b"a\nb", b"7", b""] and ws.tolist() == [uo.OK, uo.BARE, uo.BARE]
    dst, dst_off, text_len, status = ctx.unescape_batch(*b.tensors(), keep_delim=True, trim_cr=False)
    assert status.cpu().tolist() == [uo.BAD, uo.BARE, uo.BARE] and dst.cpu().numpy().tobytes() == b'a\nb"\n7\n'
