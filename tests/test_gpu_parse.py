"""brx_parse_batch (include/brx.h, brx_parse.hip): every selected record of the decoded streams of a batch as a 64-bit number and a status
byte.  Every expected value comes from tests/parse_oracle.py (Python integers; its two forms are held to each other by
tests/test_parse_abi.py), the records from tests/take_oracle.py.  val and status are pre-filled with a sentinel and carry spare
entries behind m, which must keep it.  In-process, one context."""
import numpy as np
import pytest

import brx_knobs
import craft
import parse_oracle as po
import take_oracle

pytestmark = pytest.mark.gpu

SENT = -7      # the sentinel of val
SENT8 = 0xA5   # the sentinel of status
SPARE = 8
NO_DELIM, TRIM_CR = 1, 2
SQ = po.SPACES | po.QUOTED
QT = 0x22
D63 = b"9223372036854775807"  # 2^63 - 1
KINDS = ((po.INT, 0), (po.DEC, 2), (po.HEX, 0))
SCALES = (0, 1, 2, 9, 18)


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


def _lines(records, pad=3, tail=3, sep=b"\n", delims=b"\n"):
    """One stream: the records, each followed by `sep` (so the trailing record is empty), `pad` CRs in front of it in the arena (the
    source phase) and `tail` behind."""
    s = b"".join(bytes(r) + sep for r in records)
    return Batch(_np(b"\r" * pad + s + b"\r" * tail), [pad], [len(s)], delims)


def _check(ctx, b, D=1, flags=NO_DELIM, kind=po.INT, scale=0, quote=QT, sel=None, m=None, form="fsm"):
    """One call on raw pointers against parse_oracle.  sel = (streams, records) or None for all-records mode over m entries (default
    sum(count) + n).  -> (val, status, L) as numpy, the oracle's (equal to the device's)."""
    import torch
    if sel is not None:
        si, sk = np.asarray(sel[0], dtype=np.int64), np.asarray(sel[1], dtype=np.int64)
        m = len(si)
        d_ss, d_sr = _dev(si, torch.int32), _dev(sk)
        sel_ptrs = (d_ss.data_ptr(), d_sr.data_ptr())
        want, wst, L = po.parse_take(form, b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, D, flags, kind, scale, quote,
                                     si & 0xFFFFFFFF, sk)
    else:
        if m is None:
            m = int(np.sum(b.count)) + b.n
        sel_ptrs = (None, None)
        want, wst, L = po.parse_take(form, b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, D, flags, kind, scale, quote, m=m)
    tag = (D, flags, kind, scale, sel is not None, m)
    val = torch.full((m + SPARE,), SENT, dtype=torch.int64, device="cuda:0")
    status = torch.full((m + SPARE,), SENT8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.parse_batch_device(*(b.head() + (D, flags) + sel_ptrs + (m, kind, scale, quote)), val.data_ptr(), status.data_ptr())
    got, gst = val.cpu().numpy(), status.cpu().numpy()
    assert (got[m:] == SENT).all() and (gst[m:] == SENT8).all(), tag
    bad = np.flatnonzero((got[:m] != want) | (gst[:m] != wst))
    assert bad.size == 0, (tag, bad[:8].tolist(), L[bad[:8]].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist(), gst[bad[:8]].tolist(),
                           wst[bad[:8]].tolist())
    return want, wst, L


def _all_kinds(ctx, b, flag_sets=(NO_DELIM, NO_DELIM | SQ), kinds=KINDS, **kw):
    seen = set()
    for flags in flag_sets:
        for kind, scale in kinds:
            _, st, _ = _check(ctx, b, 1, flags, kind, scale, **kw)
            seen.update(st.tolist())
    return seen


def _exact(rng, L, kind):
    """a record of exactly L bytes that is mostly a number of `kind`: leading zeros or blanks, then digits, sometimes a point / a sign"""
    if L == 0:
        return b""
    alphabet = b"0123456789abcdefABCDEF" if kind == po.HEX else b"0123456789"
    sig = int(rng.integers(0, min(L, 21) + 1))
    lead = (b"0", b"0", b" ")[int(rng.integers(0, 3))] * (L - sig)
    r = bytearray(lead + bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), sig)))
    t = int(rng.integers(0, 6))
    if t == 0 and kind == po.DEC:
        r[int(rng.integers(0, L))] = 0x2E
    elif t == 1 and kind != po.HEX:
        r[0] = (0x2B, 0x2D)[int(rng.integers(0, 2))]
    elif t == 2 and L >= 2:
        r[0] = r[-1] = QT
    elif t == 3:
        r[-1] = 0x09
    return bytes(r)


# 1 -------------------------------------------------------------------------------------------------------------------------------
def test_check_values_through_both_wrappers_and_the_raw_call(ctx):
    """The contract's table, every value, each as a record of its own (one stream split at "\\n"; the empty record among them), through
    parse_batch_device, parse_batch and the raw call."""
    import torch
    recs = [c[0] for c in po.CHECK]
    b = _lines(recs)
    names = {po.INT: "int", po.DEC: "dec", po.HEX: "hex"}
    for kind, scale, flags in sorted(set(c[1:4] for c in po.CHECK)):
        want, wst, L = _check(ctx, b, 1, NO_DELIM | flags, kind, scale)
        assert L.tolist() == [len(r) for r in recs] + [0]
        v, s = ctx.parse_batch(b.arena, b.d_off, b.d_len, b.d_count, b.d_pos_off, b.d_pos, kind=names[kind], scale=scale,
                               spaces=bool(flags & po.SPACES), quote=b'"' if flags & po.QUOTED else None)
        assert v.dtype == torch.int64 and s.dtype == torch.uint8
        raw_v = torch.full((len(recs) + 1,), SENT, dtype=torch.int64, device="cuda:0")
        raw_s = torch.full((len(recs) + 1,), SENT8, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert ctx._lib.brx_parse_batch(ctx._h, *b.head(), 1, NO_DELIM | flags, None, None, len(recs) + 1, kind, scale, QT, raw_v.data_ptr(),
                                        raw_s.data_ptr(), None) == 0
        for j, c in enumerate(po.CHECK):
            if c[1:4] == (kind, scale, flags):
                assert (int(want[j]), int(wst[j])) == c[4:], c
                assert (int(v[j].item()), int(s[j].item())) == c[4:] and (int(raw_v[j].item()), int(raw_s[j].item())) == c[4:], c
        assert v.cpu().tolist() == want.tolist() and raw_s.cpu().tolist() == wst.tolist()


# 2 -------------------------------------------------------------------------------------------------------------------------------
def test_every_length_at_every_phase(ctx):
    """Records of every length 0 .. 66 in order, placed at each source phase 0 .. 15: the 64 / 65 edge, the unit edges at 16 / 32 / 48,
    the empty record; every kind, with and without SPACES | QUOTED."""
    rng = np.random.default_rng(2)
    for kind, scale in KINDS:
        one = b"".join(_exact(rng, ln, kind) + b"\n" for ln in range(67))
        slot = (len(one) + 64) // 16 * 16
        offs = [p * slot + p for p in range(16)]
        host = np.full(16 * slot + 32, 13, dtype=np.uint8)
        for o in offs:
            host[o:o + len(one)] = _np(one)
        b = Batch(host, offs, [len(one)] * 16)
        for flags in (NO_DELIM, NO_DELIM | SQ):
            _, st, L = _check(ctx, b, 1, flags, kind, scale)
            assert L.reshape(16, 68)[:, :67].tolist() == [list(range(67))] * 16
            assert (st.reshape(16, 68)[:, 65:67] == po.LONG).all() and (st.reshape(16, 68)[:, :65] != po.LONG).all()
            assert (st == po.OK).sum() > 100


# 3 -------------------------------------------------------------------------------------------------------------------------------
def test_records_on_the_first_and_the_last_bytes_of_the_arena(ctx):
    """Stream 0 starts on the arena's first byte, stream 1 ends on its last: the records within 15 bytes of either end are fetched by
    the byte (a 16-byte load would leave the arena; tools/parse_emu.cpp is the check that none does).  Then arenas of 1 .. 15 bytes."""
    s0, s1 = b"12,-3.5\n0x1F,\r\n", b"00000000000000000000017\n9,8.257,ff\n+7\r\n-1"
    b = Batch(_np(s0 + b"\r" * 5 + s1), [0, len(s0) + 5], [len(s0), len(s1)], delims=b",\n")
    seen = _all_kinds(ctx, b, (0, NO_DELIM, NO_DELIM | TRIM_CR, NO_DELIM | TRIM_CR | SQ))
    assert {po.OK, po.BAD, po.EMPTY, po.INEXACT} <= seen
    want, st, L = _check(ctx, b, 1, NO_DELIM | TRIM_CR, po.DEC, 2)
    assert want.tolist() == [1200, -350, 0, 0, 0, 1700, 900, 825, 0, 700, -100] and L.tolist() == [2, 4, 4, 0, 0, 23, 1, 5, 2, 2, 2]
    _check(ctx, b, 1, NO_DELIM, po.INT, sel=([1, 1, 0, 1, 0], [4, 0, 0, 3, 1]))
    for text in (b"7", b"\n", b"-", b"42", b"4\n2", b"0x7fffffffffff", b"123456789012345"):
        t = Batch(_np(text), [0], [len(text)])
        _all_kinds(ctx, t, (0, NO_DELIM, NO_DELIM | SQ))
    want, st, L = _check(ctx, Batch(_np(b"7"), [0], [1]), 1, NO_DELIM, po.INT)
    assert want.tolist() == [7] and st.tolist() == [po.OK] and L.tolist() == [1]


# 4 -------------------------------------------------------------------------------------------------------------------------------
def test_digit_counts_around_the_eight_digit_steps(ctx):
    """1, 7, 8, 9, 15, 16, 17, 18, 19 and 20 digits, the smallest and the largest number of each count and a random one, bare, with
    either sign, and behind leading zeros: the steps of the eight-digit conversion and the count that decides RANGE."""
    rng = np.random.default_rng(4)
    recs = []
    for c in (1, 7, 8, 9, 15, 16, 17, 18, 19, 20):
        for d in (b"1" + b"0" * (c - 1), b"9" * c, bytes(rng.integers(0x31, 0x3A, c).astype(np.uint8))):
            recs += [d, b"-" + d, b"+" + d, b"000" + d, b"-" + b"0" * 17 + d]
    b = _lines(recs)
    want, st, _ = _check(ctx, b, kind=po.INT)
    assert want[0] == 1 and (st[:-1] != po.BAD).all() and (st == po.RANGE).sum() >= 10 and (st == po.OK).sum() >= 100
    for scale in SCALES:
        _check(ctx, b, kind=po.DEC, scale=scale)
    _check(ctx, b, kind=po.HEX)


# 5 -------------------------------------------------------------------------------------------------------------------------------
def test_the_point_at_every_offset(ctx):
    """A 21-byte number, 20 digits and the point at every offset 0 .. 20, at scales 0, 1, 2, 9 and 18; the same behind a sign, with
    zeros for the leading digits (so that the value fits) and with a second point (BAD)."""
    rng = np.random.default_rng(5)
    recs = []
    for digits in (bytes(rng.integers(0x30, 0x3A, 20).astype(np.uint8)), b"0" * 12 + bytes(rng.integers(0x31, 0x3A, 8).astype(np.uint8)),
                   b"00000000000000000001", b"92233720368547758070"):
        for k in range(21):
            r = digits[:k] + b"." + digits[k:]
            recs += [r, b"-" + r]
        recs.append(digits[:5] + b"." + digits[5:9] + b"." + digits[9:])
    b = _lines(recs)
    assert all(len(r) in (21, 22) for r in recs)
    for scale in SCALES:
        _, st, _ = _check(ctx, b, kind=po.DEC, scale=scale)
        assert {po.OK, po.INEXACT, po.RANGE, po.BAD} <= set(st.tolist()) or scale == 18
    _, st, _ = _check(ctx, b, kind=po.INT)
    assert (st[:-1] == po.BAD).all()


# 6 -------------------------------------------------------------------------------------------------------------------------------
def test_the_bounds_of_64_bits_at_every_scale(ctx):
    """INT64_MAX - 1, INT64_MAX, INT64_MAX + 1 and -(2^63 - 1), -2^63, -(2^63 + 1), the point moved so that x * 10^scale is that
    number, at EVERY scale 0 .. 18; each also with one more fraction digit, 0 and 9 (INEXACT must not tip the bound)."""
    for scale in range(19):
        recs = []
        for v in (po.MAX - 1, po.MAX, po.MAX + 1):
            d = str(v).encode()
            r = d[:len(d) - scale] + b"." + d[len(d) - scale:]
            for sign in (b"", b"-", b"+"):
                recs += [sign + r, sign + r + b"0", sign + r + b"9", sign + b"00" + r]
        if scale == 0:
            recs += [D63, b"-" + D63, b"-9223372036854775808"]  # (no point at all)
        b = _lines(recs)
        want, st, _ = _check(ctx, b, kind=po.DEC, scale=scale)
        assert (int(want[4]), int(st[4])) == (-(po.MAX - 1), po.OK), scale     # -(2^63 - 2)
        assert (int(want[12]), int(st[12])) == (po.MAX, po.OK), scale          # 2^63 - 1
        assert (int(want[14]), int(st[14])) == (po.MAX, po.INEXACT), scale     # 2^63 - 1 and a cut-off 9
        assert (int(want[24]), int(st[24])) == (po.MAX, po.RANGE), scale       # 2^63
        assert (int(want[28]), int(st[28])) == (po.MIN, po.OK), scale          # -2^63
        assert (int(want[30]), int(st[30])) == (po.MIN, po.INEXACT), scale
    d = str(po.MAX + 2).encode()
    _check(ctx, _lines([b"-" + d, b"-" + d[:1] + b"." + d[1:]]), kind=po.DEC, scale=18)


# 7 -------------------------------------------------------------------------------------------------------------------------------
def test_hex_around_sixteen_digits(ctx):
    """15, 16 and 17 significant hex digits in mixed case, bare and behind 0x / 0X, behind leading zeros up to the 64 bytes; what is
    no prefix and no digit."""
    rng = np.random.default_rng(7)
    recs = []
    for c in (1, 7, 8, 9, 15, 16, 17):
        for it in range(4):
            d = bytes(b"123456789abcdefABCDEF"[int(i)] for i in rng.integers(0, 21, 1)) + \
                bytes(b"0123456789abcdefABCDEF"[int(i)] for i in rng.integers(0, 22, c - 1))
            if it == 3:
                d = (b"f" if c % 2 else b"F") * c
            recs += [d, b"0x" + d, b"0X" + d, b"0x" + b"0" * (62 - c) + d, b"0" * (64 - c) + d, b"0x000" + d, b"-" + d, b"+0x" + d]
    recs += [b"0x", b"0X", b"x1", b"0xx1", b"00x1", b"0x0x1", b"g", b"0xG", b"1 ", b"0", b"0x0", b"8000000000000000", b"0x" + b"0" * 62, b"0" * 64]
    b = _lines(recs)
    want, st, L = _check(ctx, b, kind=po.HEX)
    assert L.max() == 64 and {po.OK, po.RANGE, po.BAD, po.EMPTY} == set(st.tolist())
    assert int(want[recs.index(b"8000000000000000")]) == po.MIN
    _check(ctx, b, kind=po.INT)


# 8 -------------------------------------------------------------------------------------------------------------------------------
def test_leading_zeros_up_to_the_bound(ctx):
    """INT64_MAX, INT64_MAX + 1 and a short number behind 0 .. 64 - len leading zeros, and one zero more (LONG); with a sign, and with a
    point for DEC."""
    recs = []
    for d in (D63, b"9223372036854775808", b"17", b"1.5", b"-" + D63):
        sign, body = (d[:1], d[1:]) if d[:1] == b"-" else (b"", d)
        for z in list(range(0, 64 - len(d) + 2, 3)) + [64 - len(d) - 1, 64 - len(d), 64 - len(d) + 1]:
            recs.append(sign + b"0" * z + body)
    b = _lines(recs)
    _, st, L = _check(ctx, b, kind=po.INT)
    assert ((st == po.LONG) == (L > 64)).all() and (L == 64).sum() >= 5 and (L == 65).sum() >= 5
    for scale in (0, 2, 18):
        _check(ctx, b, kind=po.DEC, scale=scale)
    _check(ctx, b, kind=po.HEX)


# 9 -------------------------------------------------------------------------------------------------------------------------------
def test_spaces_and_quotes_alone_and_together(ctx):
    """Runs of blanks and tabs of 0 .. 40 bytes in front of and behind a number, so that the number's ends cross the unit edges at 16,
    32 and 48; quotes inside and outside the blanks; under no flag, SPACES, QUOTED and both, with two different quote bytes."""
    recs = []
    for lead in (0, 1, 7, 8, 14, 15, 16, 17, 30, 31, 32, 33, 40):
        for trail in (0, 1, 15, 16, 17, 23):
            sp = (b" ", b"\t", b" \t")[(lead + trail) % 3]
            pre, post = (sp * lead)[:lead], (sp * trail)[:trail]
            for core in (b"42", b'"42"', b"-12.5", b"0x1f"):
                recs.append(pre + core + post)
            recs += [b'"' + pre + b"7" + post + b'"', pre + post, pre + b'""' + post, pre + b'"' + post, pre + b"'9'" + post, pre + b'""7""' + post]
    b = _lines(recs)
    for flags in (NO_DELIM, NO_DELIM | po.SPACES, NO_DELIM | po.QUOTED, NO_DELIM | SQ):
        for quote in (QT, 0x27):
            for kind, scale in KINDS:
                _check(ctx, b, 1, flags, kind, scale, quote=quote)
    want, st, _ = _check(ctx, b, 1, NO_DELIM | SQ, po.INT)
    assert (st == po.OK).sum() > 100 and (st == po.EMPTY).sum() > 100 and (st == po.LONG).sum() > 0 and set(want.tolist()) == {0, 7, 42}


# 10 ------------------------------------------------------------------------------------------------------------------------------
def test_the_three_take_flag_combinations(ctx):
    """A kept delimiter makes every record BAD; a CR in front of the line feed is BAD unless BRX_TAKE_TRIM_CR takes it off (once)."""
    recs = [b"1", b"22\r", b"", b"\r", b"-5\r\r", b"3.25\r", b"ff", b" 8 \r", b"9"]
    b = _lines(recs, tail=0)
    want, st, L = _check(ctx, b, 1, 0, po.INT)
    assert st.tolist() == [po.BAD] * 9 + [po.EMPTY] and L.tolist() == [len(r) + 1 for r in recs] + [0]
    want, st, L = _check(ctx, b, 1, NO_DELIM, po.INT)
    assert st.tolist() == [po.OK, po.BAD, po.EMPTY, po.BAD, po.BAD, po.BAD, po.BAD, po.BAD, po.OK, po.EMPTY]
    want, st, L = _check(ctx, b, 1, NO_DELIM | TRIM_CR, po.INT)
    assert st.tolist() == [po.OK, po.OK, po.EMPTY, po.EMPTY, po.BAD, po.BAD, po.BAD, po.BAD, po.OK, po.EMPTY]
    assert want.tolist() == [1, 22, 0, 0, 0, 0, 0, 0, 9, 0]
    want, st, L = _check(ctx, b, 1, NO_DELIM | TRIM_CR | po.SPACES, po.DEC, 2)
    assert want.tolist() == [100, 2200, 0, 0, 0, 325, 0, 800, 900, 0]
    for flags in (0, NO_DELIM, NO_DELIM | TRIM_CR):
        _all_kinds(ctx, b, (flags, flags | SQ))
    # a record of 65 bytes that TRIM_CR takes to 64 is parsed; one of 66 is LONG
    b = _lines([b"0" * 63 + b"7\r", b"0" * 64 + b"7\r"])
    want, st, L = _check(ctx, b, 1, NO_DELIM | TRIM_CR, po.INT)
    assert want.tolist() == [7, 0, 0] and st.tolist() == [po.OK, po.LONG, po.EMPTY]
    _, st, _ = _check(ctx, b, 1, NO_DELIM, po.INT)
    assert st.tolist() == [po.LONG, po.LONG, po.EMPTY]


# 11 ------------------------------------------------------------------------------------------------------------------------------
def test_a_two_byte_delimiter(ctx):
    """delim_len 2 with the positions that brx_find_batch leaves for "\\r\\n": the first byte of every occurrence."""
    recs = [b"10", b"-20", b"", b"3\n4", b"5\r", b"0x60", b"7.5", b"\r", b"8"]
    s = b"\r\n".join(recs)
    host = _np(b"\n\n" + s + b"\r\n\r")
    ln = len(s)
    a = host[2:2 + ln]
    pos = np.flatnonzero((a[:-1] == 13) & (a[1:] == 10)).astype(np.int64)
    b = Batch(host, [2], [ln], positions=(np.array([pos.size]), np.array([0]), pos))
    want, st, L = _check(ctx, b, 2, NO_DELIM, po.INT)
    assert L.tolist() == [len(r) for r in recs] and want.tolist() == [10, -20, 0, 0, 0, 0, 0, 0, 8]
    assert st.tolist() == [po.OK, po.OK, po.EMPTY, po.BAD, po.BAD, po.BAD, po.BAD, po.BAD, po.OK]
    for flags in (0, NO_DELIM, NO_DELIM | TRIM_CR, NO_DELIM | TRIM_CR | SQ):
        for kind, scale in KINDS:
            _check(ctx, b, 2, flags, kind, scale)
    _check(ctx, b, 16, NO_DELIM, po.INT)


@pytest.fixture(scope="module")
def table():
    """16 streams of CSV-like rows (fields from parse_oracle.random_field, some rows ending in CR LF), empty streams among them, in
    slots with slack, indexed at ",\\n": about 2700 fields.  -> Batch"""
    rng = np.random.default_rng(12)
    streams = []
    for i in range(16):
        rows = []
        for _ in range(0 if i in (3, 11) else int(rng.integers(1, 90))):
            rows.append(b",".join(po.random_field(rng).replace(b",", b";") for _ in range(int(rng.integers(1, 9)))) + (b"\r\n" if rng.integers(0, 4) == 0 else b"\n"))
        s = b"".join(rows)
        streams.append(s[:-1] if i % 4 == 1 and s else s)  # (a stream that does not end on a delimiter)
    lens = np.array([len(s) for s in streams], dtype=np.int64)
    slots = lens + rng.integers(0, 40, 16)
    offs = np.cumsum(slots) - slots
    host = np.resize(np.array([0x37, 13, 10, 0x2C], dtype=np.uint8), int(slots.sum()) + 1).copy()
    for o, s in zip(offs, streams):
        host[o:o + len(s)] = _np(s)
    return Batch(host, offs, lens, delims=b",\n")


# 12 ------------------------------------------------------------------------------------------------------------------------------
def test_both_selection_modes(ctx, table):
    """Pairs mode with a shuffled selection, repeats and out-of-range entries (EMPTY); all-records mode with m = sum(count) + n, cut
    short, and beyond."""
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
    for kind, scale in KINDS:
        want, st, L = _check(ctx, table, 1, NO_DELIM | TRIM_CR | SQ, kind, scale, sel=(si, sk))
        assert (st[::50] == po.EMPTY).all() and (st[25::50] == po.EMPTY).all() and (st == po.OK).sum() > 200
        _check(ctx, table, 1, NO_DELIM | TRIM_CR | SQ, kind, scale)
        _check(ctx, table, 1, NO_DELIM | TRIM_CR, kind, scale, m=total - 777)
        _, st, _ = _check(ctx, table, 1, NO_DELIM, kind, scale, m=total + 5)
        assert (st[total:] == po.EMPTY).all()


# 13 ------------------------------------------------------------------------------------------------------------------------------
def test_selection_sizes_around_a_wave_and_a_workgroup(ctx, table):
    for m in (1, 63, 64, 65, 255, 256, 257):
        _check(ctx, table, 1, NO_DELIM | TRIM_CR, po.DEC, 2, m=m)
        _check(ctx, table, 1, NO_DELIM | TRIM_CR, po.INT, sel=(np.arange(m) % 16, np.arange(m) % 5))


# 14 ------------------------------------------------------------------------------------------------------------------------------
def test_stale_positions(ctx, table):
    """pos entries above len (2^62, 2^64 - 1), entries in decreasing order, n_pos smaller than sum(count), m beyond sum(count) + n:
    the result is that of the clamped records."""
    rng = np.random.default_rng(14)
    pos = table.pos.copy()
    j = rng.choice(pos.size, pos.size // 4, replace=False)
    third = j.size // 3
    pos[j[:third]] = 1 << 62
    pos[j[third:2 * third]] = -1
    pos[j[2 * third:]] = rng.integers(0, 3000, j.size - 2 * third)
    pos[100:200] = pos[100:200][::-1].copy()
    b = Batch(table.host, table.offs, table.lens, positions=(table.count, table.pos_off, pos))
    m = int(b.count.sum()) + 16
    for flags in (0, NO_DELIM, NO_DELIM | TRIM_CR | SQ):
        for kind, scale in KINDS:
            _, st, _ = _check(ctx, b, 1, flags, kind, scale)
    assert (st == po.LONG).sum() > 0
    _check(ctx, b, 16, 0, po.INT, m=m + 5)
    b.n_pos = pos.size // 2
    _check(ctx, b, 1, NO_DELIM | TRIM_CR, po.DEC, 9)
    _check(ctx, b, 2, NO_DELIM, po.HEX)
    b.n_pos = 0
    _, _, L = _check(ctx, b, 1, NO_DELIM, po.INT, sel=(rng.integers(0, 16, 500), rng.integers(0, 3, 500)))
    assert L.sum() > 0


# 15 ------------------------------------------------------------------------------------------------------------------------------
def test_enqueued_behind_decode_and_index(ctx):
    """Two hand-assembled Brotli streams (tests/craft.py: uncompressed meta-blocks) of CSV text: decode, brx_index_set_batch in count
    mode, torch.cumsum, fill mode and brx_parse_batch on a caller's HIP stream, nothing in between; checked on the host copy."""
    import torch
    rng = np.random.default_rng(15)
    texts = []
    for rows in (40, 25):
        texts.append(b"".join(b",".join((b"%d" % rng.integers(-10 ** 6, 10 ** 6), b"%d.%02d" % (rng.integers(0, 9999), rng.integers(0, 100)),
                                         b"0x%x" % rng.integers(0, 1 << 40), b"", b" 7 ")) + b"\r\n" for _ in range(rows)))
    streams = []
    for t in texts:
        bits = craft.Bits()
        craft.stream_header(bits)
        for at in range(0, len(t), 700):
            craft.raw_block(bits, t[at:at + 700])
        bits.put(1, 1)
        bits.put(1, 1)  # ISLAST, ISLASTEMPTY
        streams.append(bits.bytes())
    n = 2
    in_off = np.array([0, len(streams[0]), len(streams[0]) + len(streams[1])], dtype=np.int64)
    caps = [len(texts[0]) + 70, len(texts[1]) + 33]
    out_off = np.array([0, caps[0], caps[0] + caps[1]], dtype=np.int64)
    host = np.full(int(out_off[-1]), 0x2C, dtype=np.uint8)
    for o, t in zip(out_off, texts):
        host[o:o + len(t)] = _np(t)
    ref = Batch(host, out_off[:2], [len(t) for t in texts], delims=b",\n")
    total = ref.n_pos
    m = total + n
    blob, d_in_off, d_out_off = _dev(_np(b"".join(streams))), _dev(in_off), _dev(out_off)
    out = torch.full((int(out_off[-1]),), 0x2C, dtype=torch.uint8, device="cuda:0")
    out_len = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    count = torch.full((n,), SENT, dtype=torch.int64, device="cuda:0")
    pos = torch.full((total,), SENT, dtype=torch.int64, device="cuda:0")
    val = torch.full((m + SPARE,), SENT, dtype=torch.int64, device="cuda:0")
    pst = torch.full((m + SPARE,), SENT8, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        ctx.decode_batch_device(blob.data_ptr(), d_in_off.data_ptr(), n, out.data_ptr(), d_out_off.data_ptr(), out_len.data_ptr(),
                                status.data_ptr(), hip_stream=s.cuda_stream)
        head = (out.data_ptr(), d_out_off.data_ptr(), out_len.data_ptr(), n, int(out.numel()))
        ctx.index_set_batch_device(b",\n", 0, 0, 3, *head, count.data_ptr(), hip_stream=s.cuda_stream)
        pos_off = torch.cumsum(count, 0) - count
        ctx.index_set_batch_device(b",\n", 0, 0, 3, *head, None, None, pos_off.data_ptr(), pos.data_ptr(), None, total, hip_stream=s.cuda_stream)
        ctx.parse_batch_device(*head, count.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), total, 1, NO_DELIM | TRIM_CR | po.SPACES, None, None,
                               m, po.DEC, 2, 0, val.data_ptr(), pst.data_ptr(), hip_stream=s.cuda_stream)
    s.synchronize()
    assert status.cpu().tolist() == [0, 0] and out_len.cpu().tolist() == [len(t) for t in texts]
    assert np.array_equal(out.cpu().numpy(), host) and np.array_equal(pos.cpu().numpy(), ref.pos)
    want, wst, L = po.parse_take("re", host, ref.offs, ref.lens, ref.count, ref.pos_off, ref.pos, total, 1, NO_DELIM | TRIM_CR | po.SPACES, po.DEC, 2)
    got, gst = val.cpu().numpy(), pst.cpu().numpy()
    assert np.array_equal(got[:m], want) and np.array_equal(gst[:m], wst) and (got[m:] == SENT).all() and (gst[m:] == SENT8).all()
    assert (wst == po.OK).sum() == 3 * 65 and (wst == po.BAD).sum() == 65 and (wst == po.EMPTY).sum() == 65 + 2 and want[4] == 700


# 16 ------------------------------------------------------------------------------------------------------------------------------
def test_random_sweep(ctx, table):
    """About 2700 CSV-like fields per call from the generator biased to the grammar's edges, fixed seed, full comparison: every kind,
    DEC at scales 0, 1, 2, 9, 18, the flags apart and together, against both forms of the oracle."""
    seen = set()
    for form in ("fsm", "re"):
        seen |= _all_kinds(ctx, table, (NO_DELIM | TRIM_CR, NO_DELIM | TRIM_CR | po.SPACES, NO_DELIM | po.QUOTED, NO_DELIM | TRIM_CR | SQ),
                           kinds=((po.INT, 0), (po.HEX, 0)) + tuple((po.DEC, s) for s in SCALES), form=form)
    assert seen == {po.OK, po.INEXACT, po.EMPTY, po.RANGE, po.BAD, po.LONG}
    _check(ctx, table, 1, NO_DELIM | TRIM_CR | SQ, po.DEC, 2, quote=0x27)


# 17 ------------------------------------------------------------------------------------------------------------------------------
def test_an_empty_selection_and_the_refusals_on_a_live_context(ctx):
    """m = 0: BRX_SUCCESS and nothing launched, raw and through the wrapper; the refusals leave the context working."""
    import torch
    from brotli_rs_amd import brx
    b = _lines([b"12", b"x"], pad=0, tail=0)
    val = torch.full((4,), SENT, dtype=torch.int64, device="cuda:0")
    st = torch.full((4,), SENT8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert ctx._lib.brx_parse_batch(ctx._h, *b.head(), 1, 0, None, None, 0, 0, 0, 0, val.data_ptr(), st.data_ptr(), None) == 0
    ctx.synchronize()
    assert val.cpu().tolist() == [SENT] * 4 and st.cpu().tolist() == [SENT8] * 4
    none = torch.zeros(0, dtype=torch.int64, device="cuda:0")
    v, s = ctx.parse_batch(b.arena, b.d_off, b.d_len, b.d_count, b.d_pos_off, b.d_pos, sel_stream=none.to(torch.int32), sel_rec=none)
    assert v.numel() == 0 and s.numel() == 0
    tail = (None, None, 3)
    with pytest.raises(brx.BrxError, match="brx_parse_batch: BRX_TAKE_TRIM_CR"):
        ctx.parse_batch_device(*b.head(), 1, TRIM_CR, *tail, 0, 0, 0, val.data_ptr(), st.data_ptr())
    with pytest.raises(brx.BrxError, match="brx_parse_batch: unknown flag bits"):
        ctx.parse_batch_device(*b.head(), 1, 64, *tail, 0, 0, 0, val.data_ptr(), st.data_ptr())
    with pytest.raises(brx.BrxError, match="brx_parse_batch: kind"):
        ctx.parse_batch_device(*b.head(), 1, 0, *tail, 3, 0, 0, val.data_ptr(), st.data_ptr())
    with pytest.raises(brx.BrxError, match="brx_parse_batch: scale"):
        ctx.parse_batch_device(*b.head(), 1, 0, *tail, po.INT, 2, 0, val.data_ptr(), st.data_ptr())
    with pytest.raises(brx.BrxError, match="brx_parse_batch: val or status is NULL"):
        ctx.parse_batch_device(*b.head(), 1, 0, *tail, 0, 0, 0, val.data_ptr(), None)
    with pytest.raises(brx.BrxError, match="trim_cr"):
        ctx.parse_batch(b.arena, b.d_off, b.d_len, b.d_count, b.d_pos_off, b.d_pos, keep_delim=True, trim_cr=True)
    with pytest.raises(brx.BrxError, match="kind"):
        ctx.parse_batch(b.arena, b.d_off, b.d_len, b.d_count, b.d_pos_off, b.d_pos, kind="float")
    want, wst, L = _check(ctx, b)
    assert want.tolist() == [12, 0, 0] and wst.tolist() == [po.OK, po.BAD, po.EMPTY]
    v, s = ctx.parse_batch(b.arena, b.d_off, b.d_len, b.d_count, b.d_pos_off, b.d_pos, keep_delim=True)
    assert s.cpu().tolist() == [po.BAD, po.BAD, po.EMPTY]
