// brx_unescape.h -- shared by brx_unescape.hip (kernel), brx_api.cpp (brx_unescape_batch) and tools/unescape_emu.cpp (the same text on a
// CPU, lane by lane).  Everything of the pass that is not HIP-specific lives here: the plan of a record (blanks, quotes, status), the
// classification of a 16-byte unit, the decoding of one escape, the walk of one unit, the store of its output, the lane path and one
// lane's share of a row of the wave path.  Which bytes an entry's record is comes from brx_take.h (brx_take_entry_record).
//
// Memory goes through a policy type M (as in brx_take.h) so that the emulator sees every load and every store:
//   uint8_t M::ld8(const uint8_t *p)            one record byte
//   BrxTake128 M::ld128(const uint8_t *p)       16 record bytes at any alignment (only where all 16 lie inside the record)
//   void M::st8(uint8_t *p, uint8_t v)          one destination byte
//   void M::st128(uint8_t *p, BrxTake128 v)     16 destination bytes at ANY alignment (only where all 16 lie inside the text's room)
//
// The definition is THE TEXT of include/brx.h (brx_unescape_batch), a byte-serial walk.  How it is computed here.  Positions are the
// record's own, r[0 .. L); a UNIT is r[16u .. 16u + 16), a ROW 64 units.  brx_text_plan finds t = r[lo .. hi) and the WALK RANGE
// [ws, we) inside it (the body between the quotes for CSV, behind the opening quote for JSON, all of t otherwise).  In every dialect
// one byte value forms the runs that decide a byte's role (the RUN BYTE: e for JSON and BACKSLASH, q inside a CSV body):
//   E(i) := position i ends a run of ODD length of run bytes that started inside the walk range.
// The serial walk stands on a run byte as a token's first byte exactly at the positions with E(i) (runs are eaten in pairs from their
// left end, and the bytes an escape covers -- 'u' and hex digits -- are no run bytes), except that a JSON low-surrogate escape is
// eaten by the high-surrogate escape 6 bytes in front of it.  Here a pair counts as two tokens of 6 bytes: the first emits all 4
// bytes, the second nothing.  So with E known every token covers at most 6 bytes, looks at most 11 bytes ahead and 6 back, and a
// unit's output follows from the unit, its two neighbours and 32 bits of E.  E of a unit follows from its own bytes and ONE bit from
// in front (the parity of the run that reaches the unit): the carry of the lane path from unit to unit, and of the wave path across
// lanes (ballot of the units that are not all run bytes, bit scan, shuffle) and rows.
// JSON with an escape byte that is a hex digit breaks "hex digits are no run bytes": such a call walks every record byte by byte in
// its own lane (brx_text_serial), whatever its length.
#ifndef BRX_UNESCAPE_H
#define BRX_UNESCAPE_H
#include <stdint.h>
#include "brx_take.h"

// Records whose walk range has this many bytes and more are taken by their whole wave.  A lane walks a unit in about as many
// instructions as the wave spends on a row on top of its units (two ballots, a dozen shuffles), but the other 63 lanes wait for the
// lane with the longest record: at 32 units one such lane already costs the wave what two half-filled rows cost it, and below that
// the rows are mostly empty lanes.  Half a row is the break-even of that estimate; it is not tuned by measurement.
#define BRX_TEXT_LONG 512u
#define BRX_TEXT_UNIT 16
#define BRX_TEXT_ROW 1024
#define BRX_TEXT_F_SPACES 16u // == BRX_PARSE_SPACES (include/brx.h)
#define BRX_TEXT_D_CSV 0u     // == BRX_TEXT_CSV
#define BRX_TEXT_D_JSON 1u    // == BRX_TEXT_JSON
#define BRX_TEXT_D_BACKSLASH 2u
#define BRX_TEXT_S_OK 0u      // == BRX_TEXT_OK
#define BRX_TEXT_S_BARE 1u
#define BRX_TEXT_S_NULL 2u
#define BRX_TEXT_S_BAD 3u
#define BRX_TEXT_M_COPY 0u    // the walk range is copied as it stands: the status is the plan's
#define BRX_TEXT_M_CSV 1u
#define BRX_TEXT_M_JSON 2u
#define BRX_TEXT_M_BACKSLASH 3u

// the outputs and the dialect of a call
struct BrxTextArgs {
    uint32_t dialect, q, e;
    uint64_t *text_len;
    uint8_t *status;
    const uint64_t *dst_off;
    uint8_t *dst;
    uint64_t total;
};

struct BrxTextPlan { int64_t ws, we; uint32_t mode, status; };

BRX_TAKE_HD bool brx_text_hex_escape(uint32_t dialect, uint32_t e) {
    return dialect == BRX_TEXT_D_JSON && (e - 0x30u < 10u || (e | 0x20u) - 0x61u < 6u);
}

// t and the walk range of the record at `rec`, L bytes.  Loads blanks, t's first byte and at most two more.
template <class M>
BRX_TAKE_HD BrxTextPlan brx_text_plan(M &mem, const uint8_t *rec, int64_t L, uint32_t flags, uint32_t dialect, uint32_t q, uint32_t e) {
    int64_t lo = 0, hi = L;
    if (flags & BRX_TEXT_F_SPACES) {
        while (lo < hi) { const uint32_t c = mem.ld8(rec + lo); if (c != 0x20u && c != 0x09u) break; lo++; }
        while (hi > lo) { const uint32_t c = mem.ld8(rec + hi - 1); if (c != 0x20u && c != 0x09u) break; hi--; }
    }
    const int64_t T = hi - lo;
    BrxTextPlan p = {lo, hi, BRX_TEXT_M_COPY, BRX_TEXT_S_OK};
    if (dialect == BRX_TEXT_D_BACKSLASH) {
        if (T == 2 && mem.ld8(rec + lo) == e && mem.ld8(rec + lo + 1) == 0x4Eu) { p.we = lo; p.status = BRX_TEXT_S_NULL; }
        else p.mode = BRX_TEXT_M_BACKSLASH;
    } else if (T == 0 || mem.ld8(rec + lo) != q) {
        p.status = BRX_TEXT_S_BARE;
    } else if (dialect == BRX_TEXT_D_CSV) {
        if (T < 2 || mem.ld8(rec + hi - 1) != q) p.status = BRX_TEXT_S_BAD;
        else { p.mode = BRX_TEXT_M_CSV; p.ws = lo + 1; p.we = hi - 1; }
    } else {
        p.mode = BRX_TEXT_M_JSON;
        p.ws = lo + 1;
    }
    return p;
}

// the status of a walked record
BRX_TAKE_HD uint32_t brx_text_status(const BrxTextPlan &p, uint32_t bad, uint32_t closed) {
    if (p.mode == BRX_TEXT_M_COPY) return p.status;
    return (bad || (p.mode == BRX_TEXT_M_JSON && !closed)) ? BRX_TEXT_S_BAD : BRX_TEXT_S_OK;
}

// the 16 bytes r[x .. x + 16); those outside the record are 0 and are not loaded
template <class M>
BRX_TAKE_HD BrxTake128 brx_text_fetch(M &mem, const uint8_t *rec, int64_t L, int64_t x) {
    if (x >= 0 && x + 16 <= L) return mem.ld128(rec + x);
    BrxTake128 v = {0, 0};
    for (int32_t t = 0; t < 16; t++) {
        const int64_t p = x + t;
        if (p >= 0 && p < L) {
            const uint64_t b = mem.ld8(rec + p);
            if (t < 8) v.lo |= b << (8 * t); else v.hi |= b << (8 * (t - 8));
        }
    }
    return v;
}

// SWAR: bit t of the result is set iff byte t of x equals c (exact: no carries between bytes)
BRX_TAKE_HD uint32_t brx_text_eq8(uint64_t x, uint32_t c) {
    const uint64_t y = x ^ ((uint64_t)c * 0x0101010101010101ull);
    const uint64_t z = ~(((y & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | y) & 0x8080808080808080ull;
    return (uint32_t)(((z >> 7) * 0x0102040810204080ull) >> 56);
}
BRX_TAKE_HD uint32_t brx_text_eq16(BrxTake128 v, uint32_t c) { return brx_text_eq8(v.lo, c) | (brx_text_eq8(v.hi, c) << 8); }

// bit t set iff position b + t lies in [ws, we)
BRX_TAKE_HD uint32_t brx_text_range16(int64_t b, int64_t ws, int64_t we) {
    int64_t a = ws - b, z = we - b;
    if (a < 0) a = 0;
    if (z > 16) z = 16;
    if (z <= a) return 0;
    return ((1u << (uint32_t)z) - 1u) & ~((1u << (uint32_t)a) - 1u);
}

// E of a unit from the mask of its run bytes, pin = the parity of the run that ends in front of the unit
BRX_TAKE_HD uint32_t brx_text_ebits(uint32_t em, uint32_t pin) {
    uint32_t pe = pin, E = 0;
    for (uint32_t t = 0; t < 16u; t++) {
        pe = ((em >> t) & 1u) ? pe ^ 1u : 0u;
        E |= pe << t;
    }
    return E;
}
// the bits of ebits(em, 0) that pin = 1 inverts: the run bytes that the unit begins with
BRX_TAKE_HD uint32_t brx_text_lead(uint32_t em) { return em & (em ^ (em + 1u)); }

// a unit's bytes and masks: what a lane knows before it knows anything of its neighbours
struct BrxTextPre { BrxTake128 cur; uint32_t rng, sm, em; };
template <uint32_t MODE, class M>
BRX_TAKE_HD BrxTextPre brx_text_pre(M &mem, const uint8_t *rec, int64_t L, const BrxTextPlan &p, uint32_t q, uint32_t e, int64_t b) {
    BrxTextPre u;
    u.cur.lo = u.cur.hi = 0;
    u.sm = u.em = 0;
    u.rng = brx_text_range16(b, p.ws, p.we);
    if (!u.rng) return u;
    u.cur = brx_text_fetch(mem, rec, L, b);
    if (p.mode == BRX_TEXT_M_COPY) return u;
    const uint32_t mq = brx_text_eq16(u.cur, q) & u.rng, me = brx_text_eq16(u.cur, e) & u.rng;
    u.em = MODE == BRX_TEXT_M_CSV ? mq : me;
    u.sm = MODE == BRX_TEXT_M_JSON ? (mq | me) : u.em; // (JSON: a quote inside the body closes the text or is BAD)
    return u;
}

// ---- one token --------------------------------------------------------------------------------------------------------------
// bytes: the output, first byte lowest; n of them; ext: record bytes covered; kind 1: a \u escape with a high surrogate, 2: with a low
struct BrxTextTok { uint32_t ext, n, bytes, bad, kind; };

BRX_TAKE_HD uint32_t brx_text_hex4(uint32_t w) { // four hex digits, the first in the lowest byte -> the code unit, or above 0xFFFF
    uint32_t v = 0;
    for (uint32_t t = 0; t < 4u; t++) {
        const uint32_t c = (w >> (8u * t)) & 0xFFu, d = c - 0x30u, l = (c | 0x20u) - 0x61u;
        if (d < 10u) v = (v << 4) | d;
        else if (l < 6u) v = (v << 4) | (l + 10u);
        else return 0x10000u;
    }
    return v;
}

// the token whose first byte is an e at position i: a = r[i .. i + 8), b4 = r[i + 8 .. i + 12), avail = we - i >= 1 bytes of them count
BRX_TAKE_HD BrxTextTok brx_text_tok_json(uint64_t a, uint32_t b4, int64_t avail, uint32_t q, uint32_t e) {
    BrxTextTok k = {1u, 1u, e, 1u, 0u}; // malformed: the escape byte itself, BAD, one byte on
    if (avail < 2) return k;
    const uint32_t c = (uint32_t)(a >> 8) & 0xFFu;
    uint32_t o = 0x100u;
    if (c == q || c == e || c == 0x2Fu) o = c;
    else if (c == 0x62u) o = 0x08u;
    else if (c == 0x66u) o = 0x0Cu;
    else if (c == 0x6Eu) o = 0x0Au;
    else if (c == 0x72u) o = 0x0Du;
    else if (c == 0x74u) o = 0x09u;
    if (o < 0x100u) { k.ext = 2u; k.bytes = o; k.bad = 0u; return k; }
    if (c != 0x75u || avail < 6) return k;
    const uint32_t cu = brx_text_hex4((uint32_t)(a >> 16));
    if (cu > 0xFFFFu) return k;
    k.ext = 6u;
    k.bad = 0u;
    if (cu < 0x80u) { k.bytes = cu; return k; }
    if (cu < 0x800u) { k.n = 2u; k.bytes = (0xC0u | (cu >> 6)) | ((0x80u | (cu & 0x3Fu)) << 8); return k; }
    if (cu - 0xD800u >= 0x800u) {
        k.n = 3u;
        k.bytes = (0xE0u | (cu >> 12)) | ((0x80u | ((cu >> 6) & 0x3Fu)) << 8) | ((0x80u | (cu & 0x3Fu)) << 16);
        return k;
    }
    k.n = 3u; k.bytes = 0xBDBFEFu; k.bad = 1u; // a surrogate alone, unless ...
    if (cu >= 0xDC00u) { k.kind = 2u; return k; } // (the caller looks 6 bytes back)
    k.kind = 1u;
    if (avail >= 12 && ((uint32_t)(a >> 48) & 0xFFu) == e && (uint32_t)(a >> 56) == 0x75u) {
        const uint32_t lo = brx_text_hex4(b4);
        if (lo - 0xDC00u < 0x400u) {
            const uint32_t cp = 0x10000u + ((cu - 0xD800u) << 10) + (lo - 0xDC00u);
            k.n = 4u;
            k.bad = 0u;
            k.bytes = (0xF0u | (cp >> 18)) | ((0x80u | ((cp >> 12) & 0x3Fu)) << 8) | ((0x80u | ((cp >> 6) & 0x3Fu)) << 16) |
                      ((0x80u | (cp & 0x3Fu)) << 24);
        }
    }
    return k;
}

BRX_TAKE_HD BrxTextTok brx_text_tok_backslash(uint64_t a, int64_t avail, uint32_t e) {
    BrxTextTok k = {1u, 1u, e, 1u, 0u};
    if (avail < 2) return k;
    const uint32_t c = (uint32_t)(a >> 8) & 0xFFu;
    uint32_t o = c;
    if (c == 0x62u) o = 0x08u;
    else if (c == 0x66u) o = 0x0Cu;
    else if (c == 0x6Eu) o = 0x0Au;
    else if (c == 0x72u) o = 0x0Du;
    else if (c == 0x74u) o = 0x09u;
    else if (c == 0x76u) o = 0x0Bu;
    else if (c == 0x30u) o = 0x00u;
    k.ext = 2u; k.bytes = o; k.bad = 0u;
    return k;
}

BRX_TAKE_HD BrxTextTok brx_text_tok_csv(uint64_t a, int64_t avail, uint32_t q) {
    BrxTextTok k = {1u, 1u, q, 1u, 0u}; // a quote alone
    if (avail >= 2 && ((uint32_t)(a >> 8) & 0xFFu) == q) { k.ext = 2u; k.bad = 0u; }
    return k;
}

// what brx_text_tok_json's token covers, without its output: 1, 2 or 6 record bytes
BRX_TAKE_HD uint32_t brx_text_ext_json(uint64_t a, int64_t avail, uint32_t q, uint32_t e) {
    if (avail < 2) return 1u;
    const uint32_t c = (uint32_t)(a >> 8) & 0xFFu;
    if (c == q || c == e || c == 0x2Fu || c == 0x62u || c == 0x66u || c == 0x6Eu || c == 0x72u || c == 0x74u) return 2u;
    return (c == 0x75u && avail >= 6 && brx_text_hex4((uint32_t)(a >> 16)) <= 0xFFFFu) ? 6u : 1u;
}
// is brx_text_tok_json's token a \u escape with a high surrogate (kind 1)
BRX_TAKE_HD bool brx_text_high_json(uint64_t a, int64_t avail, uint32_t q, uint32_t e) {
    return brx_text_ext_json(a, avail, q, e) == 6u && brx_text_hex4((uint32_t)(a >> 16)) - 0xD800u < 0x400u;
}
// what the token at an E position covers (a token of CSV or BACKSLASH covers 2 bytes where a second one is there)
BRX_TAKE_HD uint32_t brx_text_ext(uint32_t mode, uint64_t a, int64_t avail, uint32_t q, uint32_t e) {
    if (mode == BRX_TEXT_M_JSON) return brx_text_ext_json(a, avail, q, e);
    if (mode == BRX_TEXT_M_CSV) return (avail >= 2 && ((uint32_t)(a >> 8) & 0xFFu) == q) ? 2u : 1u;
    return avail >= 2 ? 2u : 1u;
}

BRX_TAKE_HD BrxTextTok brx_text_tok(uint32_t mode, uint64_t a, uint32_t b4, int64_t avail, uint32_t q, uint32_t e) {
    if (mode == BRX_TEXT_M_JSON) return brx_text_tok_json(a, b4, avail, q, e);
    if (mode == BRX_TEXT_M_CSV) return brx_text_tok_csv(a, avail, q);
    return brx_text_tok_backslash(a, avail, e);
}

// ---- one unit ---------------------------------------------------------------------------------------------------------------
// word j of the 48 bytes prev | cur | next (0 behind them); a chain of selects, not an indexed array: no scratch
BRX_TAKE_HD uint64_t brx_text_word(const BrxTake128 &p, const BrxTake128 &c, const BrxTake128 &n, uint32_t j) {
    return j == 0u ? p.lo : j == 1u ? p.hi : j == 2u ? c.lo : j == 3u ? c.hi : j == 4u ? n.lo : j == 5u ? n.hi : 0u;
}
// the 12 bytes from byte k of prev | cur | next on
BRX_TAKE_HD void brx_text_view(const BrxTake128 &p, const BrxTake128 &c, const BrxTake128 &n, uint32_t k, uint64_t &a, uint32_t &b4) {
    const uint32_t j = k >> 3, s = 8u * (k & 7u);
    const uint64_t x0 = brx_text_word(p, c, n, j), x1 = brx_text_word(p, c, n, j + 1u), x2 = brx_text_word(p, c, n, j + 2u);
    a = s ? (x0 >> s) | (x1 << (64u - s)) : x0;
    b4 = (uint32_t)(s ? (x1 >> s) | (x2 << (64u - s)) : x1);
}

// the output of a unit: cnt <= 19 bytes (20 fit), byte t in lo (t < 8), hi (t < 16) or ext
struct BrxTextOut { uint64_t lo, hi; uint32_t ext, cnt, bad, closed; };
// n <= 16 bytes of v (the bytes above them 0) behind the cnt bytes that o holds; cnt + n <= 20
BRX_TAKE_HD void brx_text_append(BrxTextOut &o, BrxTake128 v, uint32_t n) {
    const uint32_t c = o.cnt, w = c >> 3, s = 8u * (c & 7u);
    const uint64_t p0 = v.lo << s, p1 = s ? (v.lo >> (64u - s)) | (v.hi << s) : v.hi, p2 = s ? v.hi >> (64u - s) : 0u;
    if (w == 0u) { o.lo |= p0; o.hi |= p1; o.ext |= (uint32_t)p2; }
    else if (w == 1u) { o.hi |= p0; o.ext |= (uint32_t)p1; }
    else o.ext |= (uint32_t)p0;
    o.cnt = c + n;
}
BRX_TAKE_HD void brx_text_put(BrxTextOut &o, uint32_t bytes, uint32_t n) { // n <= 4 bytes, the first lowest, the bytes above them 0
    BrxTake128 v = {bytes, 0};
    brx_text_append(o, v, n);
}

// v moved down by s < 16 bytes
BRX_TAKE_HD BrxTake128 brx_text_shr(BrxTake128 v, uint32_t s) {
    BrxTake128 r;
    if (s == 0u) return v;
    if (s < 8u) { r.lo = (v.lo >> (8u * s)) | (v.hi << (64u - 8u * s)); r.hi = v.hi >> (8u * s); }
    else { r.lo = v.hi >> (8u * (s - 8u)); r.hi = 0; }
    return r;
}

// What the unit at b emits.  Eb: bits 0 .. 15 E of the unit in front, bits 16 .. 31 E of this one.  A unit without a special byte that
// no token reaches into is moved whole; every other one is walked, with its neighbours loaded for the look-ahead and the look-back.
template <uint32_t MODE, class M>
BRX_TAKE_HD BrxTextOut brx_text_unit(M &mem, const uint8_t *rec, int64_t L, const BrxTextPlan &p, uint32_t q, uint32_t e, int64_t b,
                                     const BrxTextPre &u, uint32_t Eb) {
    BrxTextOut o = {0, 0, 0, 0, 0, 0};
    if (!u.rng) return o;
    if (u.sm == 0u && (Eb & 0xFC00u) == 0u) {
        const uint32_t first = (uint32_t)__builtin_ctz(u.rng), n = (uint32_t)__builtin_popcount(u.rng);
        const BrxTake128 v = brx_take_place(brx_text_shr(u.cur, first), 0u, n);
        o.lo = v.lo; o.hi = v.hi; o.cnt = n;
        return o;
    }
    const BrxTake128 prev = brx_text_fetch(mem, rec, L, b - 16), next = brx_text_fetch(mem, rec, L, b + 16);
    uint64_t a;
    uint32_t b4;
    int64_t cu = b; // positions in front of cu are covered by a token already
    for (uint32_t back = Eb & 0xFC00u; back; back &= back - 1u) {
        const uint32_t k = (uint32_t)__builtin_ctz(back);
        const int64_t pos = b - 16 + (int64_t)k;
        brx_text_view(prev, u.cur, next, k, a, b4);
        const int64_t end = pos + (int64_t)brx_text_ext(MODE, a, p.we - pos, q, e);
        if (end > cu) cu = end;
    }
    // from special byte to special byte: the plain bytes between two of them are appended as one span
    const uint32_t first = (uint32_t)__builtin_ctz(u.rng), end = first + (uint32_t)__builtin_popcount(u.rng), E = Eb >> 16;
    uint32_t t = cu - b > (int64_t)first ? (uint32_t)(cu - b) : first; // the first position that no token covers yet (may be >= end)
    uint32_t todo = (E | u.sm) & u.rng;
    while (todo) {
        const uint32_t s = (uint32_t)__builtin_ctz(todo);
        todo &= todo - 1u;
        const bool tok = (E >> s) & 1u;
        if (!tok && s < t) continue; // a quote that an escape covers
        if (s > t) brx_text_append(o, brx_take_place(brx_text_shr(u.cur, t), 0u, s - t), s - t);
        if (s > t) t = s;
        const int64_t i = b + (int64_t)s;
        if (tok) {
            brx_text_view(prev, u.cur, next, 16u + s, a, b4);
            BrxTextTok k = brx_text_tok(MODE, a, b4, p.we - i, q, e);
            if (k.kind == 2u && ((Eb >> (10u + s)) & 1u)) { // a low surrogate: eaten if a high one starts 6 bytes in front
                brx_text_view(prev, u.cur, next, 10u + s, a, b4);
                if (brx_text_high_json(a, p.we - (i - 6), q, e)) { k.n = 0u; k.bad = 0u; k.bytes = 0u; }
            }
            brx_text_put(o, k.bytes, k.n);
            o.bad |= k.bad;
            t = s + k.ext;
        } else if (MODE == BRX_TEXT_M_JSON) { // a quote in the open: the closing one, or BAD and a plain byte of the next span
            if (i == p.we - 1) { o.closed = 1u; t = s + 1u; }
            else o.bad = 1u;
        }
    }
    if (t < end) brx_text_append(o, brx_take_place(brx_text_shr(u.cur, t), 0u, end - t), end - t);
    return o;
}

// the unit's output to dstp[at ..), cut at the room; one 16-byte store where 16 bytes of it fall inside the room
template <class M>
BRX_TAKE_HD void brx_text_store(M &mem, uint8_t *dstp, uint64_t at, uint64_t room, const BrxTextOut &o) {
    if (!dstp || at >= room) return;
    const uint64_t left = room - at;
    const uint32_t n = o.cnt < left ? o.cnt : (uint32_t)left;
    uint32_t t = 0;
    if (n >= 16u) {
        BrxTake128 v = {o.lo, o.hi};
        mem.st128(dstp + at, v);
        t = 16u;
    }
    for (; t < n; t++)
        mem.st8(dstp + at + t, (uint8_t)((t < 8u ? o.lo >> (8u * t) : t < 16u ? o.hi >> (8u * (t - 8u)) : (uint64_t)(o.ext >> (8u * (t - 16u)))) & 0xFFu));
}

// where an entry's text goes and how much of it: the room of brx_take_batch's fill mode, cut at total whatever dst_off holds
struct BrxTextRoom { uint8_t *dstp; uint64_t room; };
BRX_TAKE_HD BrxTextRoom brx_text_room(const BrxTextArgs &x, uint64_t m, uint64_t j) {
    BrxTextRoom r = {0, 0};
    if (!x.dst) return r;
    const uint64_t s = x.dst_off[j];
    uint64_t en = j + 1u < m ? x.dst_off[j + 1u] : x.total;
    if (en > x.total) en = x.total;
    if (en <= s) return r;
    r.dstp = x.dst + s;
    r.room = en - s;
    return r;
}

// ---- the lane path: one lane, one record ------------------------------------------------------------------------------------
struct BrxTextRes { uint64_t len; uint32_t bad, closed; };
template <uint32_t MODE, class M>
BRX_TAKE_HD BrxTextRes brx_text_lane(M &mem, const uint8_t *rec, int64_t L, const BrxTextPlan &p, uint32_t q, uint32_t e, BrxTextRoom d) {
    BrxTextRes r = {0, 0, 0};
    uint32_t pin = 0, Eprev = 0;
    for (int64_t b = p.ws & ~(int64_t)15; b < p.we; b += 16) {
        const BrxTextPre u = brx_text_pre<MODE>(mem, rec, L, p, q, e, b);
        const uint32_t E = brx_text_ebits(u.em, pin);
        const BrxTextOut o = brx_text_unit<MODE>(mem, rec, L, p, q, e, b, u, Eprev | (E << 16));
        brx_text_store(mem, d.dstp, r.len, d.room, o);
        r.len += o.cnt;
        r.bad |= o.bad;
        r.closed |= o.closed;
        pin = E >> 15;
        Eprev = E;
    }
    return r;
}

// JSON with a hex digit as its escape byte: THE TEXT as it is written, byte by byte
template <class M>
BRX_TAKE_HD BrxTextRes brx_text_serial(M &mem, const uint8_t *rec, int64_t L, const BrxTextPlan &p, uint32_t q, uint32_t e, BrxTextRoom d) {
    BrxTextRes r = {0, 0, 0};
    int64_t i = p.ws;
    while (i < p.we) {
        const uint32_t c = mem.ld8(rec + i);
        BrxTextTok k = {1u, 1u, c, 0u, 0u};
        if (c == e) {
            const BrxTake128 v = brx_text_fetch(mem, rec, L, i);
            k = brx_text_tok_json(v.lo, (uint32_t)v.hi, p.we - i, q, e);
            if (k.n == 4u) k.ext = 12u;
        } else if (c == q) {
            if (i == p.we - 1) { r.closed = 1u; break; }
            k.bad = 1u;
        }
        for (uint32_t z = 0; z < k.n; z++, r.len++)
            if (d.dstp && r.len < d.room) mem.st8(d.dstp + r.len, (uint8_t)((k.bytes >> (8u * z)) & 0xFFu));
        r.bad |= k.bad;
        i += k.ext;
    }
    return r;
}

// ---- the wave path: 64 lanes, one record, lane l on unit 64 row + l -------------------------------------------------------------
// A row in three steps, each of them one lane's share; between them the lanes exchange one value each (ballot, shuffle, prefix sum:
// brx_unescape.hip does that with the wave's instructions, tools/unescape_emu.cpp with array reads around the same text):
//   1. brx_text_pre, brx_text_ebits(em, 0): the unit, its masks, and E as if no run reached it.  Exchanged: who is not all run bytes.
//   2. brx_text_pin_lane says whose last bit is this lane's parity (or the row's carry); brx_text_row_e gives E.  Exchanged: E of the
//      lane in front (brx_text_row_prev) and of lane 63 (brx_text_row_carry: the carry into the next row).
//   3. brx_text_unit walks the unit.  Exchanged: the inclusive prefix sum of the output counts; brx_text_row_at is the lane's place.
struct BrxTextCarry { uint32_t e, p; }; // E of the last unit of the row in front, and the parity of the run that ends it

// The lane whose unit's last run parity is lane's pin: the nearest lane below `lane` whose unit is not all run bytes (nonall: their
// ballot), or -1 where the row's carry is the pin.
BRX_TAKE_HD int32_t brx_text_pin_lane(uint64_t nonall, uint32_t lane) {
    const uint64_t below = nonall & (((uint64_t)1 << lane) - 1u);
    return below ? 63 - (int32_t)__builtin_clzll(below) : -1;
}
// E of the lane's unit: e0 = brx_text_ebits(em, 0) of its own, e0_src that of lane src = brx_text_pin_lane (any value where src < 0)
BRX_TAKE_HD uint32_t brx_text_row_e(uint32_t em, uint32_t e0, int32_t src, uint32_t e0_src, BrxTextCarry c) {
    const uint32_t pin = src < 0 ? c.p : e0_src >> 15;
    return pin ? e0 ^ brx_text_lead(em) : e0;
}
// E of the unit in front of the lane's: that of lane - 1, for lane 0 the carry
BRX_TAKE_HD uint32_t brx_text_row_prev(uint32_t lane, uint32_t e_below, BrxTextCarry c) { return lane ? e_below : c.e; }
// the carry into the next row from E of lane 63
BRX_TAKE_HD BrxTextCarry brx_text_row_carry(uint32_t e_63) {
    BrxTextCarry c = {e_63, e_63 >> 15};
    return c;
}
// where the lane's output goes in the text: the row's base and the inclusive prefix sum of the lanes' counts
BRX_TAKE_HD uint64_t brx_text_row_at(uint64_t base, uint32_t sum_incl, uint32_t cnt) { return base + (sum_incl - cnt); }
// the first row's base of a walk range that starts at ws
BRX_TAKE_HD int64_t brx_text_row0(int64_t ws) { return ws & ~(int64_t)(BRX_TEXT_ROW - 1); }

// host side (brx_api.cpp)
void brx_launch_unescape(const BrxTakeArgs &a, const BrxTextArgs &x, void *hip_stream);
#endif
