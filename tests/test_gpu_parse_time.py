"""brx_parse_time_batch (include/brx.h, brx_parse_time.hip): every selected record of the decoded streams of a batch as a date, a time of
day or a timestamp: val, a status byte and the zone's offset.  Every expected value comes from tests/parse_time_oracle.py (its two
forms are held to each other and to the contract's table by tests/test_parse_time_abi.py), the records from tests/take_oracle.py.
val, status and zone are pre-filled with sentinels and carry spare entries behind m, which must keep them.  In-process, one context."""
import numpy as np
import pytest

import brx_knobs
import parse_time_oracle as to
import take_oracle
from brotli_rs_amd.brx import TIME_DATE, TIME_MAX_SCALE, TIME_NO_ZONE, TIME_STAMP, TIME_TIME  # noqa: F401  (without the call nothing here runs)

pytestmark = pytest.mark.gpu

SENT = -7       # the sentinel of val
SENT8 = 0xA5    # the sentinel of status
SENT16 = -21846  # the sentinel of zone (0xAAAA)
SPARE = 8
NO_DELIM, TRIM_CR = 1, 2
SQ = to.SPACES | to.QUOTED
QT = 0x22
DATE, TIME, STAMP = to.DATE, to.TIME, to.STAMP


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


def _want(b, D, flags, kind, scale, quote, sel, m, form):
    """the oracle's (val, status, zone, L) of one call, and m"""
    if sel is not None:
        si, sk = np.asarray(sel[0], dtype=np.int64), np.asarray(sel[1], dtype=np.int64)
        return to.parse_take(form, b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, D, flags, kind, scale, quote,
                             si & 0xFFFFFFFF, sk) + (len(si),)
    if m is None:
        m = int(np.sum(b.count)) + b.n
    return to.parse_take(form, b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, D, flags, kind, scale, quote, m=m) + (m,)


def _run(ctx, b, D, flags, kind, scale, quote, sel, m, zones, want, wst, wzn, L):
    """one call on raw pointers into sentinel-filled outputs with spare entries, compared with the oracle's arrays"""
    import torch
    sel_ptrs = (None, None)
    if sel is not None:
        d_ss, d_sr = _dev(np.asarray(sel[0], dtype=np.int64), torch.int32), _dev(np.asarray(sel[1], dtype=np.int64))
        sel_ptrs = (d_ss.data_ptr(), d_sr.data_ptr())
    tag = (D, flags, kind, scale, sel is not None, m, zones)
    val = torch.full((m + SPARE,), SENT, dtype=torch.int64, device="cuda:0")
    status = torch.full((m + SPARE,), SENT8, dtype=torch.uint8, device="cuda:0")
    zone = torch.full((m + SPARE,), SENT16, dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    ctx.parse_time_batch_device(*(b.head() + (D, flags) + sel_ptrs + (m, kind, scale, quote)), val.data_ptr(), status.data_ptr(),
                                zone.data_ptr() if zones else None)
    got, gst, gzn = val.cpu().numpy(), status.cpu().numpy(), zone.cpu().numpy()
    assert (got[m:] == SENT).all() and (gst[m:] == SENT8).all() and (gzn[m if zones else 0:] == SENT16).all(), tag
    bad = np.flatnonzero((got[:m] != want) | (gst[:m] != wst) | ((gzn[:m] != wzn) if zones else False))
    assert bad.size == 0, (tag, bad[:8].tolist(), L[bad[:8]].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist(), gst[bad[:8]].tolist(),
                           wst[bad[:8]].tolist(), gzn[bad[:8]].tolist(), wzn[bad[:8]].tolist())


def _check(ctx, b, D=1, flags=NO_DELIM, kind=STAMP, scale=0, quote=QT, sel=None, m=None, form="re", zones=True):
    """One call against parse_time_oracle.  sel = (streams, records) or None for all-records mode over m entries (default sum(count)
    + n).  -> (val, status, zone, L) as numpy, the oracle's (equal to the device's)."""
    want, wst, wzn, L, m = _want(b, D, flags, kind, scale, quote, sel, m, form)
    _run(ctx, b, D, flags, kind, scale, quote, sel, m, zones, want, wst, wzn, L)
    return want, wst, wzn, L


# 1 -------------------------------------------------------------------------------------------------------------------------------
def test_check_values_through_both_wrappers_and_the_raw_call(ctx):
    """The contract's table, every value, each as a record of its own (one stream split at "\\n"), through parse_time_batch_device,
    parse_time_batch and the raw call, for every (kind, scale, flags) of the table; zone given and NULL."""
    import torch
    recs = [c[0] for c in to.CHECK]
    b = _lines(recs)
    m = len(recs) + 1
    kind_name = {DATE: "date", TIME: "time", STAMP: "stamp"}
    unit_name = {0: "s", 3: "ms", 6: "us", 9: "ns"}
    groups = sorted(set(c[1:4] for c in to.CHECK))
    assert len(groups) == 9
    for kind, scale, flags in groups:
        want, wst, wzn, L = _check(ctx, b, 1, NO_DELIM | flags, kind, scale)
        _check(ctx, b, 1, NO_DELIM | flags, kind, scale, zones=False)
        assert L.tolist() == [len(r) for r in recs] + [0]
        kw = dict(kind=kind_name[kind], spaces=bool(flags & to.SPACES), quote=b'"' if flags & to.QUOTED else None)
        v, s, z = ctx.parse_time_batch(*b.tensors(), unit=unit_name[scale], zones=True, **kw)
        v2, s2 = ctx.parse_time_batch(*b.tensors(), unit=scale, **kw)
        assert (v.dtype, s.dtype, z.dtype) == (torch.int64, torch.uint8, torch.int16) and (v.numel(), s.numel(), z.numel()) == (m, m, m)
        raw_v = torch.full((m,), SENT, dtype=torch.int64, device="cuda:0")
        raw_s = torch.full((m,), SENT8, dtype=torch.uint8, device="cuda:0")
        raw_z = torch.full((m,), SENT16, dtype=torch.int16, device="cuda:0")
        torch.cuda.synchronize()
        assert ctx._lib.brx_parse_time_batch(ctx._h, *b.head(), 1, NO_DELIM | flags, None, None, m, kind, scale, QT, raw_v.data_ptr(),
                                             raw_s.data_ptr(), raw_z.data_ptr(), None) == 0
        for j, c in enumerate(to.CHECK):
            if c[1:4] == (kind, scale, flags):
                assert (int(want[j]), int(wst[j]), int(wzn[j])) == c[4:], c
        for gv, gs, gz in ((v, s, z), (v2, s2, None), (raw_v, raw_s, raw_z)):
            assert gv.cpu().tolist() == want.tolist() and gs.cpu().tolist() == wst.tolist()
            assert gz is None or gz.cpu().tolist() == wzn.tolist()
    # what unit="ns" gives is numpy's datetime64[ns]
    v, s = ctx.parse_time_batch(*_lines([b"2024-03-10T07:08:09.123456789Z", b"1969-12-31 23:59:59.5"]).tensors(), unit="ns")
    assert v.cpu().numpy().view("datetime64[ns]")[:2].tolist() == np.array(["2024-03-10T07:08:09.123456789", "1969-12-31T23:59:59.5"],
                                                                           dtype="datetime64[ns]").tolist()


# 2 -------------------------------------------------------------------------------------------------------------------------------
def test_every_length_at_every_phase(ctx):
    """Records of every length 0 .. 66 in order, placed at each source phase 0 .. 15: the 64 / 65 edge, the unit edges at 16 / 32 / 48,
    the empty record; mostly well-formed stamps of exactly that length, the fraction stretched or cut; with and without SPACES |
    QUOTED, at three scales."""
    rng = np.random.default_rng(2)
    recs = [to.stamp_of_length(rng, ln) for ln in range(65)] + [(to.random_date(rng) + b"T" + to.random_time(rng, 50))[:ln] for ln in (65, 66)]
    one = b"".join(r + b"\n" for r in recs)
    slot = (len(one) + 64) // 16 * 16
    offs = [p * slot + p for p in range(16)]
    host = np.full(16 * slot + 32, 13, dtype=np.uint8)
    for o in offs:
        host[o:o + len(one)] = _np(one)
    b = Batch(host, offs, [len(one)] * 16)
    for flags, scale in ((NO_DELIM, 3), (NO_DELIM | SQ, 0), (NO_DELIM, 9)):
        _, st, zn, L = _check(ctx, b, 1, flags, STAMP, scale)
        assert L.reshape(16, 68)[:, :67].tolist() == [list(range(67))] * 16
        assert (st.reshape(16, 68)[:, 65:67] == to.LONG).all() and (st.reshape(16, 68)[:, :65] != to.LONG).all()
        if scale == 9:  # (the years are random in 0000 .. 9999: most of them lie outside 64 bits of nanoseconds)
            assert (st == to.RANGE).sum() > 16 * 30
        else:
            assert ((st == to.OK) | (st == to.INEXACT)).sum() > 16 * 30 and (zn != to.NO_ZONE).sum() > 16 * 15


# 3 -------------------------------------------------------------------------------------------------------------------------------
def test_a_one_record_arena_of_1_to_40_bytes(ctx):
    """The arena is one stream is one record that touches its first and its last byte: below 16 bytes every byte is fetched on its
    own, above that the last unit is (tools/parse_time_emu.cpp is the check that no load leaves the arena)."""
    rng = np.random.default_rng(3)
    seen = set()
    for size in range(1, 41):
        for rep in range(2):
            text = to.stamp_of_length(rng, size)
            t = Batch(_np(text), [0], [size])
            for flags in (0, NO_DELIM, NO_DELIM | SQ):
                want, st, zn, L = _check(ctx, t, 1, flags, STAMP, (3, 9)[rep])
                assert L.tolist() == [size]
                seen.update(st.tolist())
    assert {to.OK, to.INEXACT, to.BAD} <= seen
    want, st, zn, L = _check(ctx, Batch(_np(b"1970-01-02"), [0], [10]), 1, NO_DELIM, DATE)
    assert want.tolist() == [1] and st.tolist() == [to.OK]
    want, st, zn, L = _check(ctx, Batch(_np(b"00:01"), [0], [5]), 1, NO_DELIM, TIME)
    assert want.tolist() == [60] and st.tolist() == [to.OK]


# 4 -------------------------------------------------------------------------------------------------------------------------------
YEARS = (0, 1, 4, 100, 400, 1600, 1700, 1900, 1969, 1970, 1972, 2000, 2023, 2024, 2100, 2400, 9999)


def test_calendar_edges_as_date_and_as_stamp(ctx):
    """In each of 17 years every month with day 00, 01, last, last + 1 and 32, and months 00 and 13: as DATE, as a STAMP that is the
    date alone, and as a STAMP with a time and a zone."""
    dates, good = [], 0
    for y in YEARS:
        for mo in range(1, 13):
            last = to._month_len(y, mo)
            for d in (0, 1, last, last + 1, 32):
                dates.append(b"%04d-%02d-%02d" % (y, mo, d))
                good += 1 <= d <= last
        dates += [b"%04d-00-10" % y, b"%04d-13-01" % y]
    assert len(dates) == 17 * 62
    b = _lines(dates, pad=7)
    want, st, zn, L = _check(ctx, b, 1, NO_DELIM, DATE)
    _check(ctx, b, 1, NO_DELIM, DATE, form="fsm")
    assert (st[:-1] == to.OK).sum() == good == 17 * 24 and (st[:-1] == to.BAD).sum() == len(dates) - good
    assert want.min() == -719528 and want.max() == 2932896
    ws, sst, _, _ = _check(ctx, b, 1, NO_DELIM, STAMP)
    assert (ws == want * 86400).all() and (sst == st).all()
    b = _lines([d + b"T23:59:59.999-23:59" for d in dates], pad=2)
    for scale in (0, 3, 9):
        _, sst2, zn, _ = _check(ctx, b, 1, NO_DELIM, STAMP, scale, form="fsm")
        assert ((sst2[:-1] == to.BAD) == (st[:-1] == to.BAD)).all() and ((zn[:-1] == -1439) == (sst2[:-1] <= to.INEXACT)).all()


# 5 -------------------------------------------------------------------------------------------------------------------------------
def test_clock_and_zone_edges(ctx):
    """Every hour 00 .. 24, minute and second 00 .. 60; zone hours 00 .. 24 and zone minutes 00 .. 60 in every zone spelling with both
    signs; the three separators; fractions of 0 .. 40 digits at every scale 0 .. 9 with '.' and ','; a non-zero digit at every dropped
    place."""
    rng = np.random.default_rng(5)
    clocks = [b"%02d:30:30" % h for h in range(25)] + [b"12:%02d:30" % v for v in range(61)] + [b"12:30:%02d" % v for v in range(61)]
    clocks += [b"%02d:30" % h for h in range(25)] + [b"12:%02d" % v for v in range(61)]
    stamps = [b"2024-03-10" + sep + c for c in clocks for sep in (b"T", b"t", b" ")]
    for sg in (b"+", b"-"):
        for zh in range(25):
            stamps += [b"2024-03-10T07:08:09" + sg + z for z in (b"%02d:30" % zh, b"%02d30" % zh, b"%02d" % zh)]
        for zm in range(61):
            stamps += [b"2024-03-10T07:08:09.25" + sg + z for z in (b"05:%02d" % zm, b"05%02d" % zm)]
    stamps += [b"2024-03-10T07:08:09" + z for z in (b"Z", b"z", b"", b"+Z", b"Z+01", b"+0", b"+010", b"+01:0", b"+01:000", b"+0:100", b"+01-00", b"*01")]
    bs = _lines(stamps, pad=4)
    for scale in (0, 2):
        want, st, zn, _ = _check(ctx, bs, 1, NO_DELIM, STAMP, scale)
        _check(ctx, bs, 1, NO_DELIM, STAMP, scale, form="fsm", zones=False)
    look = dict(zip(stamps, zip(st.tolist(), zn.tolist())))
    assert look[b"2024-03-10T24:30:30"][0] == to.BAD and look[b"2024-03-10 23:30"][0] == to.OK and look[b"2024-03-10t12:30:60"][0] == to.BAD
    assert look[b"2024-03-10T07:08:09+2330"] == (to.OK, 1410) and look[b"2024-03-10T07:08:09-24"][0] == to.BAD
    assert look[b"2024-03-10T07:08:09.25-05:59"] == (to.OK, -359) and look[b"2024-03-10T07:08:09.25+0560"][0] == to.BAD
    bt = _lines(clocks, pad=9)
    want, st, zn, _ = _check(ctx, bt, 1, NO_DELIM, TIME, 0)
    assert (st[:-1] == to.OK).sum() == 24 + 60 + 60 + 24 + 60 and (zn == to.NO_ZONE).all() and want.max() == 23 * 3600 + 30 * 60 + 30
    # fractions
    fr = []
    for n in range(41):
        digs = bytes(rng.integers(0x30, 0x3A, n).astype(np.uint8))
        fr += [b"1969-12-31T23:59:59" + mark + digs + z for mark, z in ((b".", b"Z"), (b",", b""), (b".", b"-00:00"))]
    for p in range(40):  # a single non-zero digit at place p: INEXACT exactly where p >= scale
        fr += [b"2024-03-10 07:08:09," + b"0" * p + b"7" + b"0" * (39 - p), b"2024-03-10T07:08:09." + b"0" * p + b"1+01"]
    bf = _lines(fr, pad=11)
    ft = _lines([r[11:] for r in fr if r[-1:] not in b"Z1"], pad=6)
    for scale in range(10):
        want, st, zn, L = _check(ctx, bf, 1, NO_DELIM, STAMP, scale, form=("re", "fsm")[scale % 2])
        single = st[3 * 41:-1].reshape(40, 2)
        assert (single == np.where(np.arange(40) >= scale, to.INEXACT, to.OK)[:, None]).all()
        assert L.max() == 66 and (st == to.LONG).sum() == 2 and st[0] == st[1] == st[2] == to.BAD  # (an empty fraction; 65 and 66 bytes)
        _check(ctx, ft, 1, NO_DELIM, TIME, scale)


# 6 -------------------------------------------------------------------------------------------------------------------------------
def test_the_range_edges(ctx):
    """At scales 8 and 9 the stamps one unit inside, on and one unit outside the 64-bit bounds, from the oracle, in UTC and with zones; a
    zone moves a wall-clock text across the bound; at scales 0 .. 7 nothing is RANGE."""
    for scale in (8, 9):
        edges = to.range_edges(scale)
        recs = [r for r, _ in edges]
        wall = b"2262-04-11T23:47:16.854775808"
        recs += [wall + z for z in (b"Z", b"+00:01", b"-00:01", b"", b"+23:59")] + [b"1677-09-21T00:12:43.145224191" + z for z in (b"Z", b"-00:01", b"+00:01")]
        b = _lines(recs, pad=scale)
        want, st, zn, _ = _check(ctx, b, 1, NO_DELIM, STAMP, scale, form="re")
        _check(ctx, b, 1, NO_DELIM, STAMP, scale, form="fsm")
        assert [(int(v), int(s), int(z)) for v, s, z in zip(want, st, zn)][:len(edges)] == [x for _, x in edges]
        assert (st == to.RANGE).sum() >= 6 and (st == to.OK).sum() >= 10 and ((st == to.RANGE) & (want == to.MAX)).any()
        assert ((st == to.OK) & (want == to.MAX)).any()
        if scale == 9:
            assert ((st == to.RANGE) & (want == to.MIN)).any() and ((st == to.OK) & (want == to.MIN)).any()
            k = len(edges)
            assert st[k:k + 3].tolist() == [to.RANGE, to.OK, to.RANGE] and st[k + 5:k + 8].tolist() == [to.RANGE, to.OK, to.RANGE]
        assert (zn[st == to.RANGE] == to.NO_ZONE).all()
    b = _lines([b"0000-01-01T00:00:00.0000000+23:59", b"9999-12-31T23:59:59.9999999-23:59"])
    for scale in range(8):
        _, st, _, _ = _check(ctx, b, 1, NO_DELIM, STAMP, scale)
        assert st.tolist() == [to.OK, to.OK if scale == 7 else to.INEXACT, to.EMPTY]


@pytest.fixture(scope="module")
def table():
    """16 streams of rows of fields (parse_time_oracle.random_field of all three kinds, some rows ending in CR LF), empty streams among
    them, in slots with slack, indexed at ";\\n" (a comma is a decimal mark here): about 2700 fields.  -> Batch"""
    rng = np.random.default_rng(12)
    streams = []
    for i in range(16):
        rows = []
        for _ in range(0 if i in (3, 11) else int(rng.integers(1, 90))):
            rows.append(b";".join(to.random_field(rng, (STAMP, STAMP, DATE, TIME)[int(rng.integers(0, 4))]) for _ in range(int(rng.integers(1, 9))))
                        + (b"\r\n" if rng.integers(0, 4) == 0 else b"\n"))
        s = b"".join(rows)
        streams.append(s[:-1] if i % 4 == 1 and s else s)  # (a stream that does not end on a delimiter)
    lens = np.array([len(s) for s in streams], dtype=np.int64)
    slots = lens + rng.integers(0, 40, 16)
    offs = np.cumsum(slots) - slots
    host = np.resize(np.array([0x37, 13, 10, 0x3B], dtype=np.uint8), int(slots.sum()) + 1).copy()
    for o, s in zip(offs, streams):
        host[o:o + len(s)] = _np(s)
    return Batch(host, offs, lens, delims=b";\n")


# 7 -------------------------------------------------------------------------------------------------------------------------------
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
    want, st, zn, L = _check(ctx, table, 1, NO_DELIM | TRIM_CR | SQ, STAMP, 3, sel=(si, sk))
    assert (st[::50] == to.EMPTY).all() and (st[25::50] == to.EMPTY).all() and (st <= to.INEXACT).sum() > 200
    _check(ctx, table, 1, NO_DELIM | TRIM_CR | SQ, DATE, 0)
    _check(ctx, table, 1, NO_DELIM | TRIM_CR, TIME, 6, m=total - 777)
    _, st, _, _ = _check(ctx, table, 1, NO_DELIM, STAMP, 9, m=total + 5)
    assert (st[total:] == to.EMPTY).all()
    _, st_cr, _, _ = _check(ctx, table, 1, NO_DELIM | TRIM_CR, STAMP, 9)
    assert (st_cr != st[:total]).sum() > 10  # (the rows that end in CR LF)
    _check(ctx, table, 1, 0, STAMP, 0)
    # delim_len 2: the positions that a search for "\r\n" leaves; delim_len 16 over the same positions
    recs = [b"2024-03-10", b"2024-03-10T07:08:09.5+05:30", b"", b"2024-03-10\n07:08", b"2024-03-10\r", b"2024-03-10 07:08", b"1970-01-01T00:00:01Z",
            b"\r", b"1970-01-02"]
    s = b"\r\n".join(recs)
    host = _np(b"\n\n" + s + b"\r\n\r")
    a = host[2:2 + len(s)]
    pos = np.flatnonzero((a[:-1] == 13) & (a[1:] == 10)).astype(np.int64)
    b2 = Batch(host, [2], [len(s)], positions=(np.array([pos.size]), np.array([0]), pos))
    want, st, zn, L = _check(ctx, b2, 2, NO_DELIM, STAMP, 0)
    assert L.tolist() == [len(r) for r in recs]
    assert st.tolist() == [to.OK, to.INEXACT, to.EMPTY, to.BAD, to.BAD, to.OK, to.OK, to.BAD, to.OK] and want[6] == 1 and zn[1] == 330
    for flags in (0, NO_DELIM | TRIM_CR, NO_DELIM | TRIM_CR | SQ):
        _check(ctx, b2, 2, flags, STAMP, 6)
    _check(ctx, b2, 16, NO_DELIM, STAMP, 0)
    _check(ctx, table, 16, NO_DELIM, STAMP, 3, m=total + 5)
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
        _, st, _, _ = _check(ctx, b, 1, flags, STAMP, 3)
    assert (st == to.LONG).sum() > 0
    b.n_pos = pos.size // 2
    _check(ctx, b, 1, NO_DELIM | TRIM_CR, STAMP, 0)
    _check(ctx, b, 2, NO_DELIM, TIME, 0)
    b.n_pos = 0
    _, _, _, L = _check(ctx, b, 1, NO_DELIM, DATE, 0, sel=(rng.integers(0, 16, 500), rng.integers(0, 3, 500)))
    assert L.sum() > 0


# 8 -------------------------------------------------------------------------------------------------------------------------------
def test_spaces_and_quoted_on_and_off_over_the_same_records(ctx):
    s = b"2024-03-10T07:08:09Z"
    recs = [s, b" " + s, s + b"\t", b" \t" + s + b" \t ", b'"' + s + b'"', b' "' + s + b'" ', b'" ' + s + b'"', b'"' + s, s + b'"', b'""' + s + b'""',
            b'"', b'""', b'" "', b" ", b"\t \t", b'"""', b"' '" + s, b"'" + s + b"'", b"2024-03-10 07:08", b" 2024-03-10 07:08 ", b'"2024-03-10"',
            b" " * 44 + s, b" " * 45 + s, b'"' + b"2024-03-10T07:08:09." + b"0" * 42 + b'"', b"2" + s + b"2", b"22024-03-10T07:08:0922"]
    b = _lines(recs, pad=5)
    on = {}
    for flags in (NO_DELIM, NO_DELIM | to.SPACES, NO_DELIM | to.QUOTED, NO_DELIM | SQ):
        for quote in (QT, 0x27, 0x32):
            want, st, zn, _ = _check(ctx, b, 1, flags, STAMP, 0, quote=quote)
            _check(ctx, b, 1, flags, STAMP, 3, quote=quote, form="fsm")
            on[(flags & SQ, quote)] = dict(zip(recs, zip(want.tolist(), st.tolist())))
    ok = (1710054489, to.OK)
    assert on[(0, QT)][s] == ok and on[(0, QT)][b" " + s][1] == to.BAD and on[(0, QT)][b'"' + s + b'"'][1] == to.BAD
    assert on[(to.SPACES, QT)][b" \t" + s + b" \t "] == ok and on[(to.SPACES, QT)][b' "' + s + b'" '][1] == to.BAD
    assert on[(to.QUOTED, QT)][b'"' + s + b'"'] == ok and on[(to.QUOTED, QT)][b' "' + s + b'" '][1] == to.BAD
    assert on[(SQ, QT)][b' "' + s + b'" '] == ok and on[(SQ, QT)][b'" ' + s + b'"'][1] == to.BAD and on[(SQ, QT)][b'""'][1] == to.EMPTY
    assert on[(SQ, QT)][b'"'][1] == to.BAD and on[(SQ, QT)][b" " * 44 + s] == ok and on[(SQ, QT)][b" " * 45 + s] == (0, to.LONG)
    assert on[(SQ, 0x27)][b"'" + s + b"'"] == ok and on[(SQ, QT)][b"'" + s + b"'"][1] == to.BAD
    assert on[(to.QUOTED, 0x32)][b"2" + s + b"2"] == ok and on[(to.QUOTED, 0x32)][b"22024-03-10T07:08:0922"][1] == to.BAD  # a digit as the quote
    assert on[(SQ, QT)][b" 2024-03-10 07:08 "] == (1710054480, to.OK)


def _log_line(rng):
    """stamp;level;int;float with an RFC 3339 stamp, sometimes another spelling or none"""
    k = int(rng.integers(0, 10))
    st = to.random_stamp(rng, year=int(rng.integers(1990, 2040)), nfrac=3) if k else to.random_field(rng, STAMP)
    return st + b";" + (b"INFO", b"WARN", b"ERROR")[int(rng.integers(0, 3))] + b";%d;%r" % (int(rng.integers(0, 10 ** 6)), float(rng.normal()))


# 9 -------------------------------------------------------------------------------------------------------------------------------
def test_300_streams_of_log_lines_indexed_on_the_device(ctx):
    """300 streams of 1 .. 3000 bytes of synthetic log lines in slots with slack, indexed with index_set_batch on the device and parsed
    in all-records mode through the wrapper, zones and all: many workgroups, a ragged last one."""
    import torch
    rng = np.random.default_rng(9)
    streams = []
    for i in range(300):
        want_len = int(np.exp(rng.uniform(0, np.log(3000))))
        s = b""
        while len(s) < want_len:
            s += _log_line(rng) + b"\n"
        streams.append(s[:want_len])
    lens = np.array([len(s) for s in streams], dtype=np.int64)
    slots = lens + rng.integers(0, 24, 300)
    offs = np.cumsum(slots) - slots
    host = np.full(int(slots.sum()) + 1, 0x37, dtype=np.uint8)
    for o, s in zip(offs, streams):
        host[o:o + len(s)] = _np(s)
    b = Batch(host, offs, lens, delims=b";\n")
    total = int(b.count.sum()) + 300
    assert total > 4000 and total % 256 != 0
    count, _, pos_off, pos, _ = ctx.index_set_batch(b.arena, b.d_off, b.d_len, delims=b";\n", no_quote=True, no_escape=True)
    assert np.array_equal(count.cpu().numpy(), b.count) and np.array_equal(pos.cpu().numpy(), b.pos)
    want, wst, wzn, L = to.parse_take("re", b.host, b.offs, b.lens, b.count, b.pos_off, b.pos, b.n_pos, 1, NO_DELIM | SQ, STAMP, 3, QT)
    v, s, z = ctx.parse_time_batch(b.arena, b.d_off, b.d_len, count, pos_off, pos, spaces=True, quote=b'"', unit="ms", zones=True)
    assert (v.dtype, s.dtype, z.dtype) == (torch.int64, torch.uint8, torch.int16)
    assert np.array_equal(v.cpu().numpy(), want) and np.array_equal(s.cpu().numpy(), wst) and np.array_equal(z.cpu().numpy(), wzn)
    assert {to.OK, to.INEXACT, to.EMPTY, to.BAD, to.LONG} <= set(wst.tolist()) and (wst == to.OK).sum() > 500 and (wzn != to.NO_ZONE).sum() > 300
    _check(ctx, b, 1, NO_DELIM | TRIM_CR, STAMP, 9, sel=(rng.integers(0, 300, 3001), rng.integers(0, 4, 3001)))


# 10 ------------------------------------------------------------------------------------------------------------------------------
def test_enqueued_behind_index_set_batch_on_a_callers_stream(ctx, table):
    """brx_index_set_batch in count mode, torch.cumsum, fill mode and brx_parse_time_batch on a caller's HIP stream, nothing in between."""
    import torch
    n, total = table.n, table.n_pos
    m = total + n
    count = torch.full((n,), SENT, dtype=torch.int64, device="cuda:0")
    pos = torch.full((total,), SENT, dtype=torch.int64, device="cuda:0")
    val = torch.full((m + SPARE,), SENT, dtype=torch.int64, device="cuda:0")
    pst = torch.full((m + SPARE,), SENT8, dtype=torch.uint8, device="cuda:0")
    zon = torch.full((m + SPARE,), SENT16, dtype=torch.int16, device="cuda:0")
    s = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    flags = NO_DELIM | TRIM_CR | SQ
    with torch.cuda.stream(s):
        head = (table.arena.data_ptr(), table.d_off.data_ptr(), table.d_len.data_ptr(), n, int(table.arena.numel()))
        ctx.index_set_batch_device(b";\n", 0, 0, 3, *head, count.data_ptr(), hip_stream=s.cuda_stream)
        pos_off = torch.cumsum(count, 0) - count
        ctx.index_set_batch_device(b";\n", 0, 0, 3, *head, None, None, pos_off.data_ptr(), pos.data_ptr(), None, total, hip_stream=s.cuda_stream)
        ctx.parse_time_batch_device(*head, count.data_ptr(), pos_off.data_ptr(), pos.data_ptr(), total, 1, flags, None, None, m, STAMP, 6, QT,
                                    val.data_ptr(), pst.data_ptr(), zon.data_ptr(), hip_stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(pos.cpu().numpy(), table.pos) and np.array_equal(count.cpu().numpy(), table.count)
    want, wst, wzn, L = to.parse_take("re", table.host, table.offs, table.lens, table.count, table.pos_off, table.pos, total, 1, flags, STAMP, 6, QT)
    got, gst, gzn = val.cpu().numpy(), pst.cpu().numpy(), zon.cpu().numpy()
    assert np.array_equal(got[:m], want) and np.array_equal(gst[:m], wst) and np.array_equal(gzn[:m], wzn)
    assert (got[m:] == SENT).all() and (gst[m:] == SENT8).all() and (gzn[m:] == SENT16).all()
    assert (wst <= to.INEXACT).sum() > 300


# 11 ------------------------------------------------------------------------------------------------------------------------------
def test_an_empty_selection_and_the_refusals_on_a_live_context(ctx):
    """m = 0: BRX_SUCCESS and nothing launched, raw and through the wrapper; the refusals leave the context working; brx_parse_batch
    keeps reading kind 2 as HEX."""
    import torch
    from brotli_rs_amd import brx
    b = _lines([b"1970-01-01T00:00:05Z", b"ff"], pad=0, tail=0)
    val = torch.full((4,), SENT, dtype=torch.int64, device="cuda:0")
    st = torch.full((4,), SENT8, dtype=torch.uint8, device="cuda:0")
    zn = torch.full((4,), SENT16, dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    assert ctx._lib.brx_parse_time_batch(ctx._h, *b.head(), 1, 0, None, None, 0, STAMP, 9, 0, val.data_ptr(), st.data_ptr(), zn.data_ptr(), None) == 0
    ctx.synchronize()
    assert val.cpu().tolist() == [SENT] * 4 and st.cpu().tolist() == [SENT8] * 4 and zn.cpu().tolist() == [SENT16] * 4
    none = torch.zeros(0, dtype=torch.int64, device="cuda:0")
    v, s, z = ctx.parse_time_batch(*b.tensors(), sel_stream=none.to(torch.int32), sel_rec=none, zones=True)
    assert v.numel() == 0 and s.numel() == 0 and z.numel() == 0 and z.dtype == torch.int16
    tail = (None, None, 3)
    out = (val.data_ptr(), st.data_ptr(), zn.data_ptr())
    with pytest.raises(brx.BrxError, match="brx_parse_time_batch: BRX_TAKE_TRIM_CR"):
        ctx.parse_time_batch_device(*b.head(), 1, TRIM_CR, *tail, STAMP, 0, 0, *out)
    for bad in (64, 128):
        with pytest.raises(brx.BrxError, match="brx_parse_time_batch: unknown flag bits"):
            ctx.parse_time_batch_device(*b.head(), 1, bad, *tail, STAMP, 0, 0, *out)
    with pytest.raises(brx.BrxError, match="brx_parse_time_batch: kind is not"):
        ctx.parse_time_batch_device(*b.head(), 1, 0, *tail, 3, 0, 0, *out)
    with pytest.raises(brx.BrxError, match="brx_parse_time_batch: scale is not"):
        ctx.parse_time_batch_device(*b.head(), 1, 0, *tail, STAMP, 10, 0, *out)
    with pytest.raises(brx.BrxError, match="brx_parse_time_batch: scale is not"):
        ctx.parse_time_batch_device(*b.head(), 1, 0, *tail, DATE, 3, 0, *out)
    with pytest.raises(brx.BrxError, match="brx_parse_time_batch: val or status is NULL"):
        ctx.parse_time_batch_device(*b.head(), 1, 0, *tail, STAMP, 0, 0, val.data_ptr(), None, zn.data_ptr())
    for kw in (dict(keep_delim=True, trim_cr=True), dict(kind="week"), dict(unit="min"), dict(unit=10), dict(kind="date", unit="ms")):
        with pytest.raises(brx.BrxError):
            ctx.parse_time_batch(*b.tensors(), **kw)
    assert val.cpu().tolist() == [SENT] * 4 and st.cpu().tolist() == [SENT8] * 4 and zn.cpu().tolist() == [SENT16] * 4
    want, wst, wzn, L = _check(ctx, b)
    assert want.tolist() == [5, 0, 0] and wst.tolist() == [to.OK, to.BAD, to.EMPTY] and wzn.tolist() == [0, to.NO_ZONE, to.NO_ZONE]
    v, s = ctx.parse_time_batch(*b.tensors(), keep_delim=True)
    assert s.cpu().tolist() == [to.BAD, to.BAD, to.EMPTY]
    v, s = ctx.parse_batch(*b.tensors(), kind="hex")  # kind 2 of brx_parse_batch is HEX still
    assert v.cpu().tolist() == [0, 255, 0] and s.cpu().tolist() == [to.BAD, to.OK, to.EMPTY]
