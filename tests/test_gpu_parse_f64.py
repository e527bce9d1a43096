"""brx_parse_f64_batch (include/brx.h, brx_parse_f64.hip): every selected record of the decoded streams of a batch as a correctly rounded
double and a status byte.  Every expected value comes from tests/parse_f64_oracle.py (float() and exact integer rounding; its two forms
are held to each other by tests/test_parse_f64_abi.py), the records from tests/take_oracle.py.  Values are compared as bit patterns.
val and status are pre-filled with a sentinel and carry spare entries behind m, which must keep it.  In-process, one context."""
import numpy as np
import pytest

import brx_knobs
import parse_f64_oracle as fo
import take_oracle
from brotli_rs_amd.brx import PARSE_HARD, PARSE_WORDS  # noqa: F401  (without the call nothing in this file has anything to check)

pytestmark = pytest.mark.gpu

SENT = -7      # the sentinel of val (as a 64-bit pattern)
SENT8 = 0xA5   # the sentinel of status
SPARE = 8
NO_DELIM, TRIM_CR = 1, 2
SQ = fo.SPACES | fo.QUOTED
QT = 0x22


@pytest.fixture(scope="module")
def ctx():
    c = brx_knobs.context(0)
    yield c
    c.close()


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


def _lines(records, pad=3, tail=3, sep=b"\n", delims=b"\n"):
    """One stream: the records, each followed by `sep` (so the trailing record is empty), `pad` CRs in front of it in the arena (the
    source phase) and `tail` behind."""
    s = b"".join(bytes(r) + sep for r in records)
    return Batch(_np(b"\r" * pad + s + b"\r" * tail), [pad], [len(s)], delims)


def _check(ctx, b, D=1, flags=NO_DELIM, quote=QT, sel=None, m=None, form="re"):
    """One call on raw pointers against parse_f64_oracle.  sel = (streams, records) or None for all-records mode over m entries
    (default sum(count) + n).  -> (bits, status, L) as numpy, the oracle's (equal to the device's)."""
    import torch
    if sel is not None:
        si, sk = np.asarray(sel[0], dtype=np.int64), np.asarray(sel[1], dtype=np.int64)
        m = len(si)
        d_ss, d_sr = _dev(si, torch.int32), _dev(sk)
        sel_ptrs = (d_ss.data_ptr(), d_sr.data_ptr())
        want, wst, L = fo.parse_take(form, b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, D, flags, quote, si & 0xFFFFFFFF, sk)
    else:
        if m is None:
            m = int(np.sum(b.count)) + b.n
        sel_ptrs = (None, None)
        want, wst, L = fo.parse_take(form, b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, D, flags, quote, m=m)
    tag = (D, flags, sel is not None, m)
    val = torch.full((m + SPARE,), SENT, dtype=torch.int64, device="cuda:0")
    status = torch.full((m + SPARE,), SENT8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.parse_f64_batch_device(*(b.head() + (D, flags) + sel_ptrs + (m, quote)), val.data_ptr(), status.data_ptr())
    got, gst = val.cpu().numpy().view(np.uint64), status.cpu().numpy()
    assert (got[m:] == np.uint64(SENT & 0xFFFFFFFFFFFFFFFF)).all() and (gst[m:] == SENT8).all(), tag
    bad = np.flatnonzero((got[:m] != want) | (gst[:m] != wst))
    assert bad.size == 0, (tag, bad[:8].tolist(), L[bad[:8]].tolist(), ["%016X" % v for v in got[bad[:8]]], ["%016X" % v for v in want[bad[:8]]],
                           gst[bad[:8]].tolist(), wst[bad[:8]].tolist())
    return want, wst, L


def _bits(t):
    import torch
    return t.view(torch.int64).cpu().numpy().view(np.uint64)


# 1 -------------------------------------------------------------------------------------------------------------------------------
def test_check_values_through_both_wrappers_and_the_raw_call(ctx):
    """The contract's table, every value, each as a record of its own (one stream split at "\\n"), through parse_f64_batch_device,
    parse_f64_batch and the raw call; BRX_PARSE_WORDS as the table says."""
    import torch
    recs = [c[0] for c in fo.CHECK]
    b = _lines(recs)
    for flags in sorted(set(c[1] for c in fo.CHECK)):
        want, wst, L = _check(ctx, b, 1, NO_DELIM | flags)
        assert L.tolist() == [len(r) for r in recs] + [0]
        v, s = ctx.parse_f64_batch(*b.tensors(), words=bool(flags & fo.WORDS))
        assert v.dtype == torch.float64 and s.dtype == torch.uint8
        raw_v = torch.full((len(recs) + 1,), SENT, dtype=torch.int64, device="cuda:0")
        raw_s = torch.full((len(recs) + 1,), SENT8, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert ctx._lib.brx_parse_f64_batch(ctx._h, *b.head(), 1, NO_DELIM | flags, None, None, len(recs) + 1, QT, raw_v.data_ptr(),
                                            raw_s.data_ptr(), None) == 0
        vb, rb, sb, rs = _bits(v), raw_v.cpu().numpy().view(np.uint64), s.cpu().numpy(), raw_s.cpu().numpy()
        for j, c in enumerate(fo.CHECK):
            if c[1] == flags:
                assert (int(want[j]), int(wst[j])) == c[2:], c
                assert (int(vb[j]), int(sb[j])) == c[2:] and (int(rb[j]), int(rs[j])) == c[2:], c
        assert vb.tolist() == want.tolist() and rb.tolist() == want.tolist() and rs.tolist() == wst.tolist() and sb.tolist() == wst.tolist()


def _exact(rng, L):
    """a record of exactly L bytes that is mostly a number: leading zeros or blanks, then digits with a point, an exponent, a sign"""
    if L == 0:
        return b""
    t = int(rng.integers(0, 8))
    body = bytes(rng.integers(0x30, 0x3A, int(rng.integers(1, min(L, 24) + 1))).astype(np.uint8))
    if t in (1, 2, 3) and len(body) >= 2:
        k = int(rng.integers(0, len(body)))
        body = body[:k] + b"." + body[k + 1:]
    if t in (2, 3, 4) and len(body) + 4 <= L:
        body += b"e%d" % int(rng.integers(-30, 30))
    if t == 5 and len(body) + 1 <= L:
        body = b"-" + body
    body = body[:L]
    r = bytearray((b"0", b"0", b" ")[int(rng.integers(0, 3))] * (L - len(body)) + body)
    if t == 6 and L >= 2:
        r[0] = r[-1] = QT
    elif t == 7:
        r[-1] = 0x09
    return bytes(r)


# 2 -------------------------------------------------------------------------------------------------------------------------------
def test_every_length_at_every_phase(ctx):
    """Records of every length 0 .. 66 in order, placed at each source phase 0 .. 15: the 64 / 65 edge, the unit edges at 16 / 32 / 48,
    the empty record; with and without SPACES | QUOTED."""
    rng = np.random.default_rng(2)
    one = b"".join(_exact(rng, ln) + b"\n" for ln in range(67))
    slot = (len(one) + 64) // 16 * 16
    offs = [p * slot + p for p in range(16)]
    host = np.full(16 * slot + 32, 13, dtype=np.uint8)
    for o in offs:
        host[o:o + len(one)] = _np(one)
    b = Batch(host, offs, [len(one)] * 16)
    for flags in (NO_DELIM, NO_DELIM | SQ, NO_DELIM | SQ | fo.WORDS):
        _, st, L = _check(ctx, b, 1, flags)
        assert L.reshape(16, 68)[:, :67].tolist() == [list(range(67))] * 16
        assert (st.reshape(16, 68)[:, 65:67] == fo.LONG).all() and (st.reshape(16, 68)[:, :65] != fo.LONG).all()
        assert (st == fo.OK).sum() > 100


# 3 -------------------------------------------------------------------------------------------------------------------------------
def test_a_one_record_arena_of_1_to_40_bytes(ctx):
    """The arena is one stream is one record that touches its first and its last byte: below 16 bytes every byte is fetched on its
    own, above that the last unit is (tools/parse_f64_emu.cpp is the check that no load leaves the arena)."""
    rng = np.random.default_rng(3)
    seen = set()
    for size in range(1, 41):
        digits = bytes(rng.integers(0x30, 0x3A, size).astype(np.uint8))
        for text in (digits, (digits[:size // 2] + b"." + digits[size // 2 + 1:]) if size > 1 else b"7", (b"1e" + b"0" * size + b"7")[:2] + b"0" * (size - 3) + b"7" if size >= 3 else b"-" * size):
            assert len(text) == size
            t = Batch(_np(text), [0], [size])
            for flags in (0, NO_DELIM, NO_DELIM | SQ):
                want, st, L = _check(ctx, t, 1, flags)
                assert L.tolist() == [size]
                seen.update(st.tolist())
    assert {fo.OK, fo.BAD} <= seen
    want, st, L = _check(ctx, Batch(_np(b"7"), [0], [1]), 1, NO_DELIM)
    assert want.tolist() == [fo.bits_of(7.0)] and st.tolist() == [fo.OK]


@pytest.fixture(scope="module")
def table():
    """16 streams of CSV-like rows (fields from parse_f64_oracle.random_field, some rows ending in CR LF), empty streams among them, in
    slots with slack, indexed at ",\\n": about 2700 fields.  -> Batch"""
    rng = np.random.default_rng(12)
    streams = []
    for i in range(16):
        rows = []
        for _ in range(0 if i in (3, 11) else int(rng.integers(1, 90))):
            rows.append(b",".join(fo.random_field(rng).replace(b",", b";") for _ in range(int(rng.integers(1, 9)))) + (b"\r\n" if rng.integers(0, 4) == 0 else b"\n"))
        s = b"".join(rows)
        streams.append(s[:-1] if i % 4 == 1 and s else s)  # (a stream that does not end on a delimiter)
    lens = np.array([len(s) for s in streams], dtype=np.int64)
    slots = lens + rng.integers(0, 40, 16)
    offs = np.cumsum(slots) - slots
    host = np.resize(np.array([0x37, 13, 10, 0x2C], dtype=np.uint8), int(slots.sum()) + 1).copy()
    for o, s in zip(offs, streams):
        host[o:o + len(s)] = _np(s)
    return Batch(host, offs, lens, delims=b",\n")


# 4 -------------------------------------------------------------------------------------------------------------------------------
def test_selection_modes_delimiters_trim_cr_and_stale_positions(ctx, table):
    """Pairs mode with a shuffled selection, repeats and out-of-range entries (EMPTY); all-records mode with m below, at and above
    sum(count) + n; delim_len 2 and 16; BRX_TAKE_TRIM_CR; pos entries above len, in decreasing order, n_pos smaller than sum(count)."""
    rng = np.random.default_rng(13)
    total = int(table.count.sum()) + table.n
    assert total > 2000
    si = rng.integers(0, 16, 4000)
    sk = (rng.random(4000) * (table.count[si] + 1)).astype(np.int64)
    si[::50], sk[::50] = 16 + rng.integers(0, 3, 80), 0                 # no such stream
    sk[25::50] = table.count[si[25::50] % 16] + 1 + rng.integers(0, 3, 80)  # no such record
    si[7::100] = -1                                                     # (2^32 - 1 as the device reads it)
    sk[10::100] = -1
    sk[1000:2000] = sk[:1000]
    si[1000:2000] = si[:1000]                                           # repeats
    want, st, L = _check(ctx, table, 1, NO_DELIM | TRIM_CR | SQ, sel=(si, sk))
    assert (st[::50] == fo.EMPTY).all() and (st[25::50] == fo.EMPTY).all() and (st == fo.OK).sum() > 200
    _check(ctx, table, 1, NO_DELIM | TRIM_CR | SQ | fo.WORDS)
    _check(ctx, table, 1, NO_DELIM | TRIM_CR, m=total - 777)
    _, st, _ = _check(ctx, table, 1, NO_DELIM, m=total + 5)
    assert (st[total:] == fo.EMPTY).all()
    _, st_cr, _ = _check(ctx, table, 1, NO_DELIM | TRIM_CR)
    assert (st_cr != st[:total]).sum() > 10  # (the rows that end in CR LF)
    _check(ctx, table, 1, 0)
    # delim_len 2: the positions that a search for "\r\n" leaves; delim_len 16 over the same positions
    recs = [b"10", b"-2.5e3", b"", b"3\n4", b"5\r", b"1e5", b"7.5", b"\r", b"8"]
    s = b"\r\n".join(recs)
    host = _np(b"\n\n" + s + b"\r\n\r")
    a = host[2:2 + len(s)]
    pos = np.flatnonzero((a[:-1] == 13) & (a[1:] == 10)).astype(np.int64)
    b2 = Batch(host, [2], [len(s)], positions=(np.array([pos.size]), np.array([0]), pos))
    want, st, L = _check(ctx, b2, 2, NO_DELIM)
    assert L.tolist() == [len(r) for r in recs]
    assert st.tolist() == [fo.OK, fo.OK, fo.EMPTY, fo.BAD, fo.BAD, fo.OK, fo.OK, fo.BAD, fo.OK] and want[1] == fo.bits_of(-2500.0)
    for flags in (0, NO_DELIM | TRIM_CR, NO_DELIM | TRIM_CR | SQ):
        _check(ctx, b2, 2, flags)
    _check(ctx, b2, 16, NO_DELIM)
    _check(ctx, table, 16, NO_DELIM, m=total + 5)
    # stale positions
    pos = table.pos.copy()
    j = rng.choice(pos.size, pos.size // 4, replace=False)
    third = j.size // 3
    pos[j[:third]] = 1 << 62
    pos[j[third:2 * third]] = -1
    pos[j[2 * third:]] = rng.integers(0, 3000, j.size - 2 * third)
    pos[100:200] = pos[100:200][::-1].copy()
    b = Batch(table.host, table.offs, table.lens, positions=(table.count, table.pos_off, pos))
    for flags in (0, NO_DELIM, NO_DELIM | TRIM_CR | SQ):
        _, st, _ = _check(ctx, b, 1, flags)
    assert (st == fo.LONG).sum() > 0
    b.n_pos = pos.size // 2
    _check(ctx, b, 1, NO_DELIM | TRIM_CR)
    _check(ctx, b, 2, NO_DELIM)
    b.n_pos = 0
    _, _, L = _check(ctx, b, 1, NO_DELIM, sel=(rng.integers(0, 16, 500), rng.integers(0, 3, 500)))
    assert L.sum() > 0


# 5 -------------------------------------------------------------------------------------------------------------------------------
def test_the_near_midpoint_corpus(ctx):
    """The decimal expansions of midpoints between neighbouring doubles at every 7th q of -342 .. 308 and seven times over (about 2000
    records), cut to 17 .. 45 digits with the last digit moved by -1, 0, +1: against both forms of the oracle."""
    rng = np.random.default_rng(5)
    recs = []
    for rep in range(7):
        recs += fo.midpoint_records(rng, range(-342 + rep, 309, 7))
    recs += [b"1.7976931348623158e308", b"1.7976931348623159e308", b"17976931348623158079372897140530341507993413271003782e256",
             b"2.4703282292062327e-324", b"2.4703282292062328e-324", b"24703282292062327208051355972538975e-358", b"4.9e-324", b"1e-310",
             b"2.2250738585072011e-308"]
    assert 1800 < len(recs) < 2400
    b = _lines(recs, pad=5)
    want, st, L = _check(ctx, b, 1, NO_DELIM, form="re")
    _check(ctx, b, 1, NO_DELIM, form="fsm")
    hard, rng_ = st == fo.HARD, st == fo.RANGE
    mag = want & np.uint64(0x7FFFFFFFFFFFFFFF)
    assert hard.sum() >= 100, hard.sum()
    assert (rng_ & (mag == np.uint64(fo.INF))).any() and (rng_ & (mag == 0)).any()          # RANGE at both ends
    assert ((st == fo.OK) & (mag > 0) & (mag < np.uint64(1 << 52))).sum() >= 4               # subnormal results
    for j in np.flatnonzero(hard)[:200]:  # what HARD leaves open is val or val + 1
        assert fo.bits_of(float(recs[j].decode())) - int(want[j]) in (0, 1), recs[j]


# 6 -------------------------------------------------------------------------------------------------------------------------------
def test_exponent_and_digit_count_edges(ctx):
    """1e308 .. 1e309 and 1e-323 .. 1e-325 in steps of the 17th digit; 19, 20 and 21 digits with zero and non-zero tails; the point at
    every place among the first 20 digits; exponent fields with leading zeros up to the 64-byte bound; exponents of 6 and more digits."""
    recs = [b"1e308", b"1e309", b"1.0e308", b"10e307", b"0.1e310", b"1e-323", b"1e-324", b"1e-325", b"10e-325", b"0.1e-322", b"3e-324", b"2e-324"]
    recs += [b"1.%016de308" % k for k in range(0, 8 * 10 ** 15, 10 ** 15 - 7)]
    recs += [b"%d.%de-324" % (k // 10, k % 10) for k in range(10, 110, 7)]
    d19 = b"9007199254740993123"
    for d in (d19, d19 + b"0", d19 + b"00", d19 + b"1", d19 + b"01", d19 + b"5", b"9999999999999999999", b"99999999999999999999", b"999999999999999999999",
              b"1000000000000000000", b"10000000000000000000", b"10000000000000000001", b"18446744073709551615", b"18446744073709551616"):
        recs += [d, b"-" + d, d + b"e-30", d + b"e290", b"000" + d]
        for k in range(0, min(len(d), 20) + 1):  # the point at every place
            recs += [d[:k] + b"." + d[k:], d[:k] + b"." + d[k:] + b"e5"]
    for z in range(0, 62):
        recs += [b"1e" + b"0" * z + b"5", b"2.5E-" + b"0" * max(z - 4, 0) + b"3"]
    recs += [b"1e" + b"0" * 61 + b"5", b"1e" + b"0" * 62 + b"5", b"1e+" + b"0" * 60 + b"5", b"1e-" + b"0" * 60 + b"5"]
    recs += [b"1e100000", b"1e-100000", b"1e999999", b"1e-999999", b"1e1000000", b"1e-1000000", b"1e123456789012345678901234567890",
             b"1e-123456789012345678901234567890", b"0e123456789012345678901234567890", b"-0.000e-99999999", b"0." + b"0" * 50 + b"1e1000051",
             b"0." + b"0" * 50 + b"1e358", b"0." + b"0" * 50 + b"1e359", b"1" + b"0" * 55 + b"e-379", b"1" + b"0" * 55 + b"e-380",
             b"1" + b"0" * 50 + b"e-1000050"]
    b = _lines(recs, pad=1)
    want, st, L = _check(ctx, b, 1, NO_DELIM, form="re")
    _check(ctx, b, 1, NO_DELIM, form="fsm")
    assert L.max() == 65 and {fo.OK, fo.RANGE, fo.HARD, fo.LONG} <= set(st.tolist()) and fo.BAD not in set(st[:-1].tolist())
    look = dict(zip(recs, zip(want.tolist(), st.tolist())))
    assert look[b"1e308"] == (fo.bits_of(1e308), fo.OK) and look[b"1e309"] == (fo.INF, fo.RANGE)
    assert look[b"1e-323"] == (2, fo.OK) and look[b"1e-324"] == (0, fo.RANGE) and look[b"3e-324"] == (1, fo.OK)
    assert look[b"1e-1000000"] == (0, fo.RANGE) and look[b"1e1000000"] == (fo.INF, fo.RANGE)
    assert look[b"0e123456789012345678901234567890"] == (0, fo.OK) and look[b"-0.000e-99999999"] == (fo.SIGN, fo.OK)
    assert look[b"0." + b"0" * 50 + b"1e359"] == (fo.bits_of(1e308), fo.OK)


# 7 -------------------------------------------------------------------------------------------------------------------------------
def test_the_words_flag_on_and_off(ctx):
    recs = [b"nan", b"NaN", b"NAN", b"-nan", b"+nAn", b"inf", b"Inf", b"-INF", b"+inf", b"infinity", b"Infinity", b"-INFINITY", b"+iNfInItY",
            b"na", b"n", b"i", b"in", b"infinit", b"infinityy", b"nanx", b"xnan", b"+-inf", b"-+nan", b"inf1", b"1inf", b"nane5", b"infe5", b"in f",
            b"nan ", b" nan", b"\tinf\t", b'"nan"', b' "-inf" ', b'"infinity', b"  -Infinity  ", b'" inf"', b"n.n", b"1nf", b"1e5", b"-", b"+",
            b"\xeeNF", b"\x0eAN", b"iNF\x00", b"0" * 61 + b"inf", b" " * 61 + b"inf", b" " * 56 + b"infinity", b" " * 57 + b"infinity"]
    b = _lines(recs, pad=2)
    on = {}
    for flags in (NO_DELIM, NO_DELIM | fo.WORDS, NO_DELIM | SQ, NO_DELIM | SQ | fo.WORDS, NO_DELIM | fo.SPACES | fo.WORDS):
        want, st, _ = _check(ctx, b, 1, flags, form="re")
        _check(ctx, b, 1, flags, form="fsm")
        on[flags] = dict(zip(recs, zip(want.tolist(), st.tolist())))
    off, w, sqw = on[NO_DELIM], on[NO_DELIM | fo.WORDS], on[NO_DELIM | SQ | fo.WORDS]
    assert all(off[r][1] in (fo.BAD, fo.LONG) and off[r][0] == 0 for r in recs if r != b"1e5")
    assert w[b"NaN"] == (fo.NAN, fo.OK) and w[b"-nan"] == (fo.NAN | fo.SIGN, fo.OK) and w[b"+iNfInItY"] == (fo.INF, fo.OK)
    assert w[b"-INF"] == (fo.INF | fo.SIGN, fo.OK) and sum(v[1] == fo.OK for v in w.values()) == 14
    assert sqw[b' "-inf" '] == (fo.INF | fo.SIGN, fo.OK) and sqw[b"  -Infinity  "] == (fo.INF | fo.SIGN, fo.OK) and sqw[b'" inf"'][1] == fo.BAD
    assert sqw[b" " * 56 + b"infinity"] == (fo.INF, fo.OK) and sqw[b" " * 57 + b"infinity"] == (0, fo.LONG)
    for r in (b"na", b"infinit", b"nanx", b"+-inf", b"infinityy", b"\xeeNF", b"\x0eAN", b"iNF\x00"):
        assert w[r] == (0, fo.BAD) and sqw[r] == (0, fo.BAD), r


# 8 -------------------------------------------------------------------------------------------------------------------------------
def test_finish_completes_the_hard_entries_on_the_host(ctx):
    """finish=True: a batch with known HARD entries comes back equal to float() everywhere with no HARD left, in both selection modes;
    a batch without HARD entries is what finish=False gives."""
    import torch
    rng = np.random.default_rng(8)
    mids = [r for r in fo.midpoint_records(rng, range(-330, 300, 9)) if fo.parse_re(r)[1] == fo.HARD and len(r) <= 60][:60]
    assert len(mids) >= 30
    rows, k = [], 0
    for i in range(40):
        rows.append(b",".join([b"%r" % float(rng.normal()), b' "%s" ' % mids[k % len(mids)], b"-" + mids[(k + 1) % len(mids)], b"x", b"", b"1e400"]) + b"\r\n")
        k += 2
    s0, s1 = b"".join(rows[:25]), b"".join(rows[25:])
    b = Batch(_np(s0 + b"\r\r\r" + s1), [0, len(s0) + 3], [len(s0), len(s1)], delims=b",\n")
    kw = dict(trim_cr=True, spaces=True, quote=b'"')
    fl = NO_DELIM | TRIM_CR | SQ
    want, wst, L = fo.parse_take("re", b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, 1, fl, QT)
    assert (wst == fo.HARD).sum() == 80
    src, L = take_oracle.take_vec(b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, 1, 3)
    buf = bytes(b.host)

    def finished(idx):
        v, s = want[idx].copy(), wst[idx].copy()
        for t, j in enumerate(idx):
            if wst[j] == fo.HARD:
                x = float(buf[src[j]:src[j] + L[j]].strip(b" \t").strip(b'"').decode())
                v[t], s[t] = fo.bits_of(x), (fo.RANGE if x == 0 or abs(x) == float("inf") else fo.OK)  # (step 6's statuses)
        return v, s

    m = len(want)
    v0, s0_ = ctx.parse_f64_batch(*b.tensors(), **kw)
    assert _bits(v0).tolist() == want.tolist() and s0_.cpu().numpy().tolist() == wst.tolist()
    v1, s1_ = ctx.parse_f64_batch(*b.tensors(), finish=True, **kw)
    fv, fs = finished(np.arange(m))
    assert _bits(v1).tolist() == fv.tolist() and s1_.cpu().numpy().tolist() == fs.tolist() and fo.HARD not in fs.tolist()
    assert (fv != want).sum() >= 10  # (some of them were val + 1)
    si = rng.integers(0, 2, 300)
    sk = (rng.random(300) * (b.count[si] + 2)).astype(np.int64)
    pw, pst, _ = fo.parse_take("re", b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, 1, fl, QT, si, sk)
    v2, s2 = ctx.parse_f64_batch(*b.tensors(), sel_stream=_dev(si, torch.int32), sel_rec=_dev(sk), finish=True, **kw)
    keys = b.pos_off + np.arange(2)
    entry = np.where(sk <= b.count[si], keys[si] + sk, m - 1)  # (out of range: the empty record, as the batch's last entry is)
    assert wst[m - 1] == fo.EMPTY and (pst == fo.HARD).sum() > 20
    fv2, fs2 = finished(entry)
    assert _bits(v2).tolist() == fv2.tolist() and s2.cpu().numpy().tolist() == fs2.tolist()
    # no HARD entry: the same as finish=False
    plain = _lines([b"1.5", b"-2e-3", b"x", b"", b"1e400", b"0.1000000000000000055511151231257827"])
    a = ctx.parse_f64_batch(*plain.tensors())
    c = ctx.parse_f64_batch(*plain.tensors(), finish=True)
    assert _bits(a[0]).tolist() == _bits(c[0]).tolist() and a[1].cpu().tolist() == c[1].cpu().tolist() == [0, 0, fo.BAD, fo.EMPTY, fo.RANGE, 0, fo.EMPTY]
    assert a[0].cpu().tolist()[:2] == [1.5, -2e-3]


# 9 -------------------------------------------------------------------------------------------------------------------------------
def test_300_streams_of_log_uniform_lengths(ctx):
    """300 streams of 1 .. 3000 bytes of mixed content in slots with slack, one call in each mode: many workgroups, a ragged last one."""
    rng = np.random.default_rng(9)
    streams = []
    for i in range(300):
        want_len = int(np.exp(rng.uniform(0, np.log(3000))))
        s = b""
        while len(s) < want_len:
            s += fo.random_field(rng).replace(b",", b";") + (b"\n" if rng.integers(0, 5) == 0 else b",")
        streams.append(s[:want_len])
    lens = np.array([len(s) for s in streams], dtype=np.int64)
    slots = lens + rng.integers(0, 24, 300)
    offs = np.cumsum(slots) - slots
    host = np.full(int(slots.sum()) + 1, 0x37, dtype=np.uint8)
    for o, s in zip(offs, streams):
        host[o:o + len(s)] = _np(s)
    b = Batch(host, offs, lens, delims=b",\n")
    total = int(b.count.sum()) + 300
    assert total > 4000 and total % 256 != 0
    want, st, L = _check(ctx, b, 1, NO_DELIM | SQ | fo.WORDS)
    assert set(st.tolist()) == set(fo.NAMES)
    _check(ctx, b, 1, NO_DELIM | TRIM_CR, sel=(rng.integers(0, 300, 3001), rng.integers(0, 4, 3001)))


# 10 ------------------------------------------------------------------------------------------------------------------------------
def test_enqueued_behind_index_set_batch_on_a_callers_stream(ctx, table):
    """brx_index_set_batch in count mode, torch.cumsum, fill mode and brx_parse_f64_batch on a caller's HIP stream, nothing in between."""
    import torch
    n, total = table.n, table.n_pos
    m = total + n
    count = torch.full((n,), SENT, dtype=torch.int64, device="cuda:0")
    pos = torch.full((total,), SENT, dtype=torch.int64, device="cuda:0")
    val = torch.full((m + SPARE,), SENT, dtype=torch.int64, device="cuda:0")
    pst = torch.full((m + SPARE,), SENT8, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        head = (table.arena.data_ptr(), table.d_off.data_ptr(), table.d_len.data_ptr(), n, int(table.arena.numel()))
        ctx.index_set_batch_device(b",\n", 0, 0, 3, *head, count.data_ptr(), hip_stream=s.cuda_stream)
        pos_off = torch.cumsum(count, 0) - count
        ctx.index_set_batch_device(b",\n", 0, 0, 3, *head, None, None, pos_off.data_ptr(), pos.data_ptr(), None, total, hip_stream=s.cuda_stream)
        ctx.parse_f64_batch_device(*head, count.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), total, 1, NO_DELIM | TRIM_CR | SQ | fo.WORDS, None,
                                   None, m, QT, val.data_ptr(), pst.data_ptr(), hip_stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(pos.cpu().numpy(), table.pos) and np.array_equal(count.cpu().numpy(), table.count)
    want, wst, L = fo.parse_take("re", table.host, table.offs, table.lens, table.count, table.pos_off, table.pos, total, 1,
                                 NO_DELIM | TRIM_CR | SQ | fo.WORDS, QT)
    got, gst = val.cpu().numpy().view(np.uint64), pst.cpu().numpy()
    assert np.array_equal(got[:m], want) and np.array_equal(gst[:m], wst) and (val.cpu().numpy()[m:] == SENT).all() and (gst[m:] == SENT8).all()
    assert (wst == fo.OK).sum() > 500


def test_an_empty_selection_and_the_refusals_on_a_live_context(ctx):
    """m = 0: BRX_SUCCESS and nothing launched, raw and through the wrapper; the refusals leave the context working; brx_parse_batch
    keeps refusing BRX_PARSE_WORDS."""
    import torch
    from brotli_rs_amd import brx
    b = _lines([b"1.5", b"x"], pad=0, tail=0)
    val = torch.full((4,), SENT, dtype=torch.int64, device="cuda:0")
    st = torch.full((4,), SENT8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert ctx._lib.brx_parse_f64_batch(ctx._h, *b.head(), 1, 0, None, None, 0, 0, val.data_ptr(), st.data_ptr(), None) == 0
    ctx.synchronize()
    assert val.cpu().tolist() == [SENT] * 4 and st.cpu().tolist() == [SENT8] * 4
    none = torch.zeros(0, dtype=torch.int64, device="cuda:0")
    v, s = ctx.parse_f64_batch(*b.tensors(), sel_stream=none.to(torch.int32), sel_rec=none, finish=True)
    assert v.numel() == 0 and s.numel() == 0 and v.dtype == torch.float64
    tail = (None, None, 3)
    with pytest.raises(brx.BrxError, match="brx_parse_f64_batch: BRX_TAKE_TRIM_CR"):
        ctx.parse_f64_batch_device(*b.head(), 1, TRIM_CR, *tail, 0, val.data_ptr(), st.data_ptr())
    with pytest.raises(brx.BrxError, match="brx_parse_f64_batch: unknown flag bits"):
        ctx.parse_f64_batch_device(*b.head(), 1, 128, *tail, 0, val.data_ptr(), st.data_ptr())
    with pytest.raises(brx.BrxError, match="brx_parse_f64_batch: val or status is NULL"):
        ctx.parse_f64_batch_device(*b.head(), 1, 0, *tail, 0, val.data_ptr(), None)
    with pytest.raises(brx.BrxError, match="brx_parse_batch: unknown flag bits"):
        ctx.parse_batch_device(*b.head(), 1, 64, *tail, 0, 0, 0, val.data_ptr(), st.data_ptr())
    with pytest.raises(brx.BrxError, match="trim_cr"):
        ctx.parse_f64_batch(*b.tensors(), keep_delim=True, trim_cr=True)
    want, wst, L = _check(ctx, b)
    assert want.tolist() == [fo.bits_of(1.5), 0, 0] and wst.tolist() == [fo.OK, fo.BAD, fo.EMPTY]
    v, s = ctx.parse_f64_batch(*b.tensors(), keep_delim=True)
    assert s.cpu().tolist() == [fo.BAD, fo.BAD, fo.EMPTY]
