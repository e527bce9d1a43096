// brx_parse.h -- shared by brx_parse.hip (kernel), brx_api.cpp (brx_parse_batch) and tools/parse_emu.cpp (the same text on a CPU, lane
// by lane).  Everything of the pass that is not HIP-specific lives here: the fetch of a record's at most four 16-byte units, the
// classification of their bytes, the grammar on bit masks and the conversion of the digits.  Which bytes an entry's record is comes
// from brx_take.h (brx_take_entry_record), and they are loaded through brx_take_fetch with the memory policy M of brx_take.h (ld8,
// ld128): a 16-byte load only where all 16 bytes lie inside the arena, else the record's own bytes one by one.
//
// The definition is THE PARSE of include/brx.h (brx_parse_batch).  How it is computed here:
//   * a record of at most 64 bytes is held as eight 64-bit words (byte q of the record = bits [8 (q % 8), + 8) of word q / 8), bytes
//     at or behind L zero.  The words are named, never indexed: a word is chosen by a select tree (brx_parse_word);
//   * every word is classified once with carry-free SWAR tests (bit 7 of a byte = the answer for that byte) and each answer is
//     compressed to one bit per byte, so that the record has four 64-bit masks, bit q = byte q: digit (hex digit for HEX), non-zero
//     digit, point, space;
//   * spaces, quotes, sign, prefix, the grammar, the point, the leading zeros, the kept and the dropped fraction are bit scans and
//     mask tests on those four;
//   * the significant digits are counted before any arithmetic (above 19, or 16 hex digits, is RANGE); what remains is converted
//     eight ASCII digits at a time from windows that END at the field's last digit, the bytes in front of the field masked to 0.
#ifndef BRX_PARSE_H
#define BRX_PARSE_H
#include <stdint.h>
#include "brx_take.h"

#define BRX_PARSE_F_SPACES 16u // == BRX_PARSE_SPACES (include/brx.h)
#define BRX_PARSE_F_QUOTED 32u // == BRX_PARSE_QUOTED
#define BRX_PARSE_K_INT 0u     // == BRX_PARSE_INT
#define BRX_PARSE_K_DEC 1u     // == BRX_PARSE_DEC
#define BRX_PARSE_K_HEX 2u     // == BRX_PARSE_HEX
#define BRX_PARSE_S_OK 0u      // == BRX_PARSE_OK ...
#define BRX_PARSE_S_INEXACT 1u
#define BRX_PARSE_S_EMPTY 2u
#define BRX_PARSE_S_RANGE 3u
#define BRX_PARSE_S_BAD 4u
#define BRX_PARSE_S_LONG 5u
#define BRX_PARSE_LEN 64u      // == BRX_PARSE_MAX_LEN

#define BRX_PARSE_ONES 0x0101010101010101ull
#define BRX_PARSE_HIGH 0x8080808080808080ull
#define BRX_PARSE_LOW7 0x7F7F7F7F7F7F7F7Full

struct BrxParseBuf { uint64_t w0, w1, w2, w3, w4, w5, w6, w7; }; // the record's bytes, zero behind L
struct BrxParseMasks { uint64_t dig, nz, pt, sp; };                 // bit q = byte q of the record is a ...
struct BrxParseOut { int64_t val; uint32_t status; };

// ---- classification: bit 7 of every byte of the result answers for that byte; no carry crosses a byte ------------------------------
// a >= c for the 7-bit bytes of a (a & HIGH == 0) and a constant 1 <= c <= 0x80
BRX_TAKE_HD uint64_t brx_parse_ge(uint64_t a, uint32_t c) { return (a + (0x80u - c) * BRX_PARSE_ONES) & BRX_PARSE_HIGH; }
// x == c, for any bytes
BRX_TAKE_HD uint64_t brx_parse_eq(uint64_t x, uint32_t c) {
    const uint64_t y = x ^ (c * BRX_PARSE_ONES);
    return ~(((y & BRX_PARSE_LOW7) + BRX_PARSE_LOW7) | y) & BRX_PARSE_HIGH;
}
// bit 7 of bytes 0 .. 7 -> bits 0 .. 7.  By the dword: bits 0, 8, 16, 24 times (2^24 + 2^17 + 2^10 + 2^3) land on bits 24 .. 27 and no
// two partial products share a bit.
BRX_TAKE_HD uint32_t brx_parse_bits(uint64_t m) {
    const uint32_t lo = (((uint32_t)m >> 7) * 0x01020408u) >> 24, hi = (((uint32_t)(m >> 32) >> 7) * 0x01020408u) >> 24;
    return lo | (hi << 4);
}

// one word of the record -> its 8 bits of each mask, at bit `at`
BRX_TAKE_HD void brx_parse_classify(uint64_t x, uint32_t kind, uint32_t flags, uint32_t at, BrxParseMasks &k) {
    const uint64_t a = x & BRX_PARSE_LOW7, ascii = ~x & BRX_PARSE_HIGH;
    const uint64_t lt3a = ~brx_parse_ge(a, 0x3Au) & ascii;
    uint64_t dig = brx_parse_ge(a, 0x30u) & lt3a, nz = brx_parse_ge(a, 0x31u) & lt3a; // '0' .. '9', '1' .. '9'
    if (kind == BRX_PARSE_K_HEX) {
        const uint64_t l = a | (0x20u * BRX_PARSE_ONES); // only 'A' .. 'F' and 'a' .. 'f' come out as 'a' .. 'f'
        const uint64_t alpha = brx_parse_ge(l, 0x61u) & ~brx_parse_ge(l, 0x67u) & ascii;
        dig |= alpha;
        nz |= alpha;
    }
    k.dig |= (uint64_t)brx_parse_bits(dig) << at;
    k.nz |= (uint64_t)brx_parse_bits(nz) << at;
    if (kind == BRX_PARSE_K_DEC) k.pt |= (uint64_t)brx_parse_bits(brx_parse_eq(x, 0x2Eu)) << at;
    if (flags & BRX_PARSE_F_SPACES) k.sp |= (uint64_t)brx_parse_bits(brx_parse_eq(x, 0x20u) | brx_parse_eq(x, 0x09u)) << at;
}

// ---- the record's bytes -----------------------------------------------------------------------------------------------------------
// the first n = 1 .. 16 bytes of a unit of the record at p, the bytes behind them 0
template <class M>
BRX_TAKE_HD BrxTake128 brx_parse_fetch(M &mem, const uint8_t *p, uint32_t n, const uint8_t *arena, uint64_t span) {
    return brx_take_place(brx_take_fetch(mem, p, n, arena, arena + span), 0, n);
}

#define BRX_PARSE_UNIT(g, wa, wb)                                                                               \
    if (L > 16u * (g)) {                                                                                        \
        const uint32_t n_ = L - 16u * (g) < 16u ? L - 16u * (g) : 16u;                                          \
        const BrxTake128 v_ = brx_parse_fetch(mem, p + 16u * (g), n_, arena, span);                             \
        b.wa = v_.lo;                                                                                           \
        b.wb = v_.hi;                                                                                           \
        brx_parse_classify(v_.lo, kind, flags, 16u * (g), k);                                                   \
        if (n_ > 8u) brx_parse_classify(v_.hi, kind, flags, 16u * (g) + 8u, k);                                 \
    }

// a record of L <= 64 bytes: its words and its masks; a unit behind the record's end is not loaded
template <class M>
BRX_TAKE_HD void brx_parse_load(M &mem, const uint8_t *arena, uint64_t span, BrxTakeRec r, uint32_t kind, uint32_t flags, BrxParseBuf &b,
                                BrxParseMasks &k) {
    const uint8_t *p = arena + r.src;
    const uint32_t L = (uint32_t)r.len;
    b.w0 = b.w1 = b.w2 = b.w3 = b.w4 = b.w5 = b.w6 = b.w7 = 0;
    k.dig = k.nz = k.pt = k.sp = 0;
    BRX_PARSE_UNIT(0u, w0, w1)
    BRX_PARSE_UNIT(1u, w2, w3)
    BRX_PARSE_UNIT(2u, w4, w5)
    BRX_PARSE_UNIT(3u, w6, w7)
}

// The helpers below take the record as a whole BrxParseBuf BY VALUE and read its words only at constant places, so that the words stay
// registers: a word is chosen by a select tree over values, never by an address (an address would make the record an indexed array).
// word i of the record for i < 8, else 0 (i may have wrapped below 0)
BRX_TAKE_HD uint64_t brx_parse_word(const BrxParseBuf b, uint32_t i) {
    const uint64_t w0 = b.w0, w1 = b.w1, w2 = b.w2, w3 = b.w3, w4 = b.w4, w5 = b.w5, w6 = b.w6, w7 = b.w7;
    const uint64_t a0 = (i & 1u) ? w1 : w0, a1 = (i & 1u) ? w3 : w2, a2 = (i & 1u) ? w5 : w4, a3 = (i & 1u) ? w7 : w6;
    const uint64_t c0 = (i & 2u) ? a1 : a0, c1 = (i & 2u) ? a3 : a2;
    const uint64_t d = (i & 4u) ? c1 : c0;
    return i < 8u ? d : 0;
}

// the 8 bytes of the record from byte s on, -24 <= s < 64; bytes in front of the record and behind its 64 read as 0
BRX_TAKE_HD uint64_t brx_parse_window(const BrxParseBuf b, int32_t s) {
    const uint32_t t = (uint32_t)(s + 24), q = (t >> 3) - 3u, sh = (t & 7u) * 8u;
    const uint64_t lo = brx_parse_word(b, q), hi = brx_parse_word(b, q + 1u);
    return sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
}

BRX_TAKE_HD uint32_t brx_parse_byte(const BrxParseBuf b, uint32_t q) { return (uint32_t)(brx_parse_window(b, (int32_t)q) & 0xFFu); }

// ---- conversion -------------------------------------------------------------------------------------------------------------------
// the last nb = 1 .. 8 bytes of x (ASCII digits, the first of them the most significant) as a number: the three-multiply reduction
BRX_TAKE_HD uint64_t brx_parse_dec8(uint64_t x, uint32_t nb) {
    x &= (~(uint64_t)0 << (8u * (8u - nb))) & 0x0F0F0F0F0F0F0F0Full;
    x = (x * 2561u) >> 8;                                          // 10 * 2^8 + 1: pairs
    x = ((x & 0x00FF00FF00FF00FFull) * 6553601u) >> 16;            // 100 * 2^16 + 1: fours
    return ((x & 0x0000FFFF0000FFFFull) * 42949672960001ull) >> 32; // 10000 * 2^32 + 1: all eight
}

// the same for hex digits: nibbles, packed by shifts
BRX_TAKE_HD uint64_t brx_parse_hex8(uint64_t x, uint32_t nb) {
    x &= (~(uint64_t)0 << (8u * (8u - nb))) & BRX_PARSE_LOW7;
    x = (x & 0x0F0F0F0F0F0F0F0Full) + 9u * ((x >> 6) & BRX_PARSE_ONES); // a letter has bit 6, a digit has not
    x = ((x << 4) | (x >> 8)) & 0x00FF00FF00FF00FFull;
    x = ((x << 8) | (x >> 16)) & 0x0000FFFF0000FFFFull;
    return ((x << 16) | (x >> 32)) & 0xFFFFFFFFull;
}

// the decimal digits at bytes [start, end) of the record, end - start <= 19: below 10^19, so inside 64 bits
BRX_TAKE_HD uint64_t brx_parse_dec_field(const BrxParseBuf b, uint32_t start, uint32_t end) {
    const uint32_t c = end - start;
    const int32_t e = (int32_t)end;
    uint64_t v = 0;
    if (c > 16u) v = brx_parse_dec8(brx_parse_window(b, e - 24), c - 16u);
    if (c > 8u) v = v * 100000000u + brx_parse_dec8(brx_parse_window(b, e - 16), c - 8u < 8u ? c - 8u : 8u);
    if (c > 0u) v = v * 100000000u + brx_parse_dec8(brx_parse_window(b, e - 8), c < 8u ? c : 8u);
    return v;
}

// the hex digits at bytes [start, end), end - start <= 16
BRX_TAKE_HD uint64_t brx_parse_hex_field(const BrxParseBuf b, uint32_t start, uint32_t end) {
    const uint32_t c = end - start;
    const int32_t e = (int32_t)end;
    uint64_t v = 0;
    if (c > 8u) v = brx_parse_hex8(brx_parse_window(b, e - 16), c - 8u);
    if (c > 0u) v = (v << 32) | brx_parse_hex8(brx_parse_window(b, e - 8), c < 8u ? c : 8u);
    return v;
}

// 10^e for e <= 31 that fits (e <= 19)
BRX_TAKE_HD uint64_t brx_parse_pow10(uint32_t e) {
    uint64_t p = 1;
    if (e & 1u) p *= 10u;
    if (e & 2u) p *= 100u;
    if (e & 4u) p *= 10000u;
    if (e & 8u) p *= 100000000u;
    if (e & 16u) p *= 10000000000000000ull;
    return p;
}

// bits [0, n) for n <= 64, and bits [a, b) for a <= b <= 64
BRX_TAKE_HD uint64_t brx_parse_below(uint32_t n) { return n >= 64u ? ~(uint64_t)0 : ((uint64_t)1 << n) - 1u; }
BRX_TAKE_HD uint64_t brx_parse_range(uint32_t a, uint32_t b) { return brx_parse_below(b) & ~brx_parse_below(a); }

BRX_TAKE_HD BrxParseOut brx_parse_result(int64_t val, uint32_t status) {
    BrxParseOut o;
    o.val = val;
    o.status = status;
    return o;
}

// ---- THE PARSE, steps 2 .. 7, on a loaded record of L <= 64 bytes -----------------------------------------------------------------
BRX_TAKE_HD BrxParseOut brx_parse_text(const BrxParseBuf &b, const BrxParseMasks &k, uint32_t L, uint32_t kind, uint32_t scale,
                                       uint32_t flags, uint32_t quote) {
    uint32_t lo = 0, e = L; // t = bytes [lo, e)
    if (flags & BRX_PARSE_F_SPACES) {
        const uint64_t ns = brx_parse_below(L) & ~k.sp;
        if (!ns) return brx_parse_result(0, BRX_PARSE_S_EMPTY);
        lo = (uint32_t)__builtin_ctzll(ns);
        e = 64u - (uint32_t)__builtin_clzll(ns);
    }
    if ((flags & BRX_PARSE_F_QUOTED) && e - lo >= 2u && brx_parse_byte(b, lo) == quote && brx_parse_byte(b, e - 1u) == quote) {
        lo++;
        e--;
    }
    if (lo == e) return brx_parse_result(0, BRX_PARSE_S_EMPTY);

    if (kind == BRX_PARSE_K_HEX) {
        if (e - lo >= 2u && brx_parse_byte(b, lo) == 0x30u && (brx_parse_byte(b, lo + 1u) | 0x20u) == 0x78u) lo += 2u;
        const uint64_t body = brx_parse_range(lo, e);
        if (lo == e || (body & ~k.dig)) return brx_parse_result(0, BRX_PARSE_S_BAD);
        const uint64_t nz = body & k.nz;
        const uint32_t first = nz ? (uint32_t)__builtin_ctzll(nz) : e;
        if (e - first > 16u) return brx_parse_result(-1, BRX_PARSE_S_RANGE);
        return brx_parse_result((int64_t)brx_parse_hex_field(b, first, e), BRX_PARSE_S_OK);
    }

    const uint32_t c0 = brx_parse_byte(b, lo);
    const bool neg = c0 == 0x2Du;
    if (neg || c0 == 0x2Bu) lo++;
    const uint64_t body = brx_parse_range(lo, e), pts = body & k.pt; // (k.pt is 0 for INT: a point is then no digit, so BAD)
    if ((body & ~(k.dig | k.pt)) || !(body & k.dig) || (pts & (pts - 1u))) return brx_parse_result(0, BRX_PARSE_S_BAD);
    const uint32_t pp = pts ? (uint32_t)__builtin_ctzll(pts) : e; // the point, or the end
    const uint64_t nzi = brx_parse_range(lo, pp) & k.nz;
    const uint32_t first = nzi ? (uint32_t)__builtin_ctzll(nzi) : pp; // I without its leading zeros = [first, pp)
    const uint32_t fs = pp < e ? pp + 1u : e;                          // F = [fs, e), its kept part [fs, fe)
    const uint32_t keep = e - fs < scale ? e - fs : scale, fe = fs + keep;
    const bool inexact = (brx_parse_range(fe, e) & k.nz) != 0;
    const int64_t big = neg ? INT64_MIN : INT64_MAX;
    if (pp - first + scale > 19u) return brx_parse_result(big, BRX_PARSE_S_RANGE); // V >= 10^19 > 2^63
    // at most 19 digits in all: V < 10^19 < 2^64, and neither product nor the sum leaves 64 bits
    uint64_t V = brx_parse_dec_field(b, first, pp) * brx_parse_pow10(scale);
    if (keep) V += brx_parse_dec_field(b, fs, fe) * brx_parse_pow10(scale - keep);
    if (V > (uint64_t)INT64_MAX + (neg ? 1u : 0u)) return brx_parse_result(big, BRX_PARSE_S_RANGE);
    return brx_parse_result((int64_t)(neg ? 0u - V : V), inexact ? BRX_PARSE_S_INEXACT : BRX_PARSE_S_OK);
}

// one lane, one record: THE PARSE.  A record above 64 bytes has none of its bytes loaded.
template <class M>
BRX_TAKE_HD BrxParseOut brx_parse_lane(M &mem, const uint8_t *arena, uint64_t span, BrxTakeRec r, uint32_t kind, uint32_t scale,
                                       uint32_t flags, uint32_t quote) {
    if (r.len > BRX_PARSE_LEN) return brx_parse_result(0, BRX_PARSE_S_LONG);
    BrxParseBuf b;
    BrxParseMasks k;
    brx_parse_load(mem, arena, span, r, kind, flags, b, k);
    return brx_parse_text(b, k, (uint32_t)r.len, kind, scale, flags, quote);
}

// host side (brx_api.cpp)
void brx_launch_parse(const BrxTakeArgs &a, uint32_t kind, uint32_t scale, uint32_t quote, int64_t *val, uint8_t *status,
                      void *hip_stream);
#endif
