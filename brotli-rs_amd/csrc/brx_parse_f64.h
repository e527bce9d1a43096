// brx_parse_f64.h -- shared by brx_parse_f64.hip (kernel), brx_api.cpp (brx_parse_f64_batch) and tools/parse_f64_emu.cpp (the same text
// on a CPU, lane by lane).  The record's fetch, its words, its masks and the digit helpers are those of brx_parse.h, used as they are
// with the DEC classification (digit, non-zero digit, point, space); which bytes a record is comes from brx_take.h.  This header adds
// what a double needs: the exponent's grammar, the first 19 significant digits, and the conversion of w * 10^q to binary64.
//
// The definition is THE PARSE, F64 of include/brx.h (brx_parse_f64_batch).  How it is computed here:
//   * the body behind the sign may hold bytes that are neither digit nor point: the first of them must be 'e' / 'E', the byte behind it
//     may be a sign, and everything behind that must be digits.  That is one bit scan, two byte reads and one mask test; no new mask;
//   * s = the mantissa's digits from its first non-zero one.  Up to 19 of them are w, read as two dec_field pieces around the point
//     and one pow10; "something behind the 19th digit is not 0" is one test of the non-zero mask;
//   * the exponent's digits are counted behind their leading zeros; seven or more saturate (the result is then out of range whatever
//     the mantissa's at most 64 digits do);
//   * w * 10^q -> binary64 is the Eisel-Lemire algorithm in integer arithmetic, one path: w normalised, times the 128-bit power of
//     five of csrc/brx_pow5.h (a second multiply only where the first leaves the low bits in doubt), then round to nearest even.
//     For w < 2^64 it is exact without a fallback (Mushtak and Lemire, "Fast number parsing without fallback", 2023), so an s of at
//     most 19 digits is never HARD.  q < -342 is 0 and q > 308 is inf before the table is touched: w < 10^19 then lies below half the
//     least subnormal, or w >= 1 above the largest double;
//   * more than 19 digits with a non-zero tail: the conversion runs for w and for w + 1 (<= 10^19 < 2^64); equal results are the
//     answer by monotonicity, different ones are HARD with the lower one as val.
// No double arithmetic anywhere: the result is a bit pattern.
#ifndef BRX_PARSE_F64_H
#define BRX_PARSE_F64_H
#include <stdint.h>
#include "brx_parse.h"
#include "brx_pow5.h"

#define BRX_PARSE_F_WORDS 64u // == BRX_PARSE_WORDS (include/brx.h)
#define BRX_PARSE_S_HARD 6u   // == BRX_PARSE_HARD
#define BRX_F64_INF 0x7FF0000000000000ull
#define BRX_F64_NAN 0x7FF8000000000000ull
#define BRX_F64_SIGN 0x8000000000000000ull
#define BRX_F64_EXP_SAT 1000000 // an exponent of seven or more digits counts as this: beyond any q that a 64-byte mantissa can pull back

struct BrxParseF64Out { uint64_t bits; uint32_t status; };

BRX_TAKE_HD BrxParseF64Out brx_parse_f64_result(uint64_t bits, uint32_t status) {
    BrxParseF64Out o;
    o.bits = bits;
    o.status = status;
    return o;
}

// the high 64 bits of a * b
BRX_TAKE_HD uint64_t brx_f64_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// RN(w * 10^q) as a binary64 pattern without its sign, for any w and BRX_POW5_Q_MIN <= q <= BRX_POW5_Q_MAX; 0 and BRX_F64_INF are the
// out-of-range answers.  tab = brx_pow5 wherever it lives.
BRX_TAKE_HD uint64_t brx_f64_convert(const BrxPow5 *tab, uint64_t w, int32_t q) {
    if (w == 0) return 0;
    const uint32_t lz = (uint32_t)__builtin_clzll(w);
    w <<= lz;
    const BrxPow5 p = tab[q - BRX_POW5_Q_MIN]; // one 16-byte load
    uint64_t lower = w * p.hi, upper = brx_f64_mulhi(w, p.hi);
    if ((upper & 0x1FFu) == 0x1FFu) { // the 55 bits that matter could still move: the second half of the power
        const uint64_t second = brx_f64_mulhi(w, p.lo);
        lower += second;
        if (second > lower) upper++;
    }
    const uint32_t upperbit = (uint32_t)(upper >> 63), shift = upperbit + 9u;
    uint64_t mant = upper >> shift; // 54 bits: 53 and the rounding bit
    // floor(log2(10^q)) + 63, then the exponent's bias
    int32_t power2 = (int32_t)((217706 * q) >> 16) + 63 + (int32_t)upperbit - (int32_t)lz + 1023;
    if (power2 <= 0) { // subnormal, or nothing
        if (1 - power2 >= 64) return 0;
        mant >>= (uint32_t)(1 - power2);
        mant += mant & 1u;
        mant >>= 1;
        return mant; // (mant == 2^52 is the least normal number: the same pattern)
    }
    // a product that is exactly halfway between two doubles (possible only for 5^q below 2^64) goes to the even one
    if (lower <= 1u && q >= -4 && q <= 23 && (mant & 3u) == 1u && (mant << shift) == upper) mant &= ~(uint64_t)1;
    mant += mant & 1u;
    mant >>= 1;
    if (mant >= (uint64_t)2 << 52) {
        mant = (uint64_t)1 << 52;
        power2++;
    }
    mant &= ~((uint64_t)1 << 52);
    if (power2 >= 0x7FF) return BRX_F64_INF;
    return mant | ((uint64_t)power2 << 52);
}

// the same with the cuts in front of the table
BRX_TAKE_HD uint64_t brx_f64_from_decimal(const BrxPow5 *tab, uint64_t w, int32_t q) {
    if (q < BRX_POW5_Q_MIN) return 0;
    if (q > BRX_POW5_Q_MAX) return w ? BRX_F64_INF : 0;
    return brx_f64_convert(tab, w, q);
}

// [+-]? ( nan | inf | infinity ) in any letter case: t = bytes [lo, e) behind the sign, 8 bytes of it in x
BRX_TAKE_HD uint64_t brx_parse_f64_word(uint64_t x, uint32_t n) {
    x |= 0x2020202020202020ull;
    if (n == 3u && (x & 0xFFFFFFu) == 0x6E616Eu) return BRX_F64_NAN;           // "nan"
    if (n == 3u && (x & 0xFFFFFFu) == 0x666E69u) return BRX_F64_INF;           // "inf"
    if (n == 8u && x == 0x7974696E69666E69ull) return BRX_F64_INF;             // "infinity"
    return 0;
}

// ---- THE PARSE, F64, steps 2 .. 7, on a loaded record of L <= 64 bytes ------------------------------------------------------------
BRX_TAKE_HD BrxParseF64Out brx_parse_f64_text(const BrxPow5 *tab, const BrxParseBuf &b, const BrxParseMasks &k, uint32_t L, uint32_t flags,
                                              uint32_t quote) {
    uint32_t lo = 0, e = L; // t = bytes [lo, e)
    if (flags & BRX_PARSE_F_SPACES) {
        const uint64_t ns = brx_parse_below(L) & ~k.sp;
        if (!ns) return brx_parse_f64_result(0, BRX_PARSE_S_EMPTY);
        lo = (uint32_t)__builtin_ctzll(ns);
        e = 64u - (uint32_t)__builtin_clzll(ns);
    }
    if ((flags & BRX_PARSE_F_QUOTED) && e - lo >= 2u && brx_parse_byte(b, lo) == quote && brx_parse_byte(b, e - 1u) == quote) {
        lo++;
        e--;
    }
    if (lo == e) return brx_parse_f64_result(0, BRX_PARSE_S_EMPTY);

    const uint32_t c0 = brx_parse_byte(b, lo);
    const uint64_t sign = c0 == 0x2Du ? BRX_F64_SIGN : 0;
    if (sign || c0 == 0x2Bu) lo++;
    const uint64_t body = brx_parse_range(lo, e), other = body & ~(k.dig | k.pt);
    uint32_t me = e;      // the mantissa is [lo, me)
    int32_t ex = 0;       // the exponent field's value
    if (other) {
        const uint32_t ep = (uint32_t)__builtin_ctzll(other);
        if ((flags & BRX_PARSE_F_WORDS) && ep == lo) {
            const uint64_t v = brx_parse_f64_word(brx_parse_window(b, (int32_t)lo), e - lo);
            if (v) return brx_parse_f64_result(v | sign, BRX_PARSE_S_OK);
        }
        if ((brx_parse_byte(b, ep) | 0x20u) != 0x65u) return brx_parse_f64_result(0, BRX_PARSE_S_BAD);
        uint32_t x = ep + 1u;
        const uint32_t c1 = brx_parse_byte(b, x); // (0 at or behind byte 64)
        const bool eneg = c1 == 0x2Du;
        if (x < e && (eneg || c1 == 0x2Bu)) x++;
        if (x >= e || (brx_parse_range(x, e) & ~k.dig)) return brx_parse_f64_result(0, BRX_PARSE_S_BAD);
        const uint64_t enz = brx_parse_range(x, e) & k.nz;
        if (enz) {
            const uint32_t fx = (uint32_t)__builtin_ctzll(enz);
            ex = e - fx > 6u ? BRX_F64_EXP_SAT : (int32_t)brx_parse_dec_field(b, fx, e);
            if (eneg) ex = -ex;
        }
        me = ep;
    }
    const uint64_t mbody = brx_parse_range(lo, me), pts = mbody & k.pt;
    if (!(mbody & k.dig) || (pts & (pts - 1u))) return brx_parse_f64_result(0, BRX_PARSE_S_BAD);
    const uint64_t nz = mbody & k.nz;
    if (!nz) return brx_parse_f64_result(sign, BRX_PARSE_S_OK); // zero, whatever the exponent says
    const uint32_t pp = pts ? (uint32_t)__builtin_ctzll(pts) : me; // the point, or the mantissa's end
    const uint32_t first = (uint32_t)__builtin_ctzll(nz);          // s starts here
    const uint32_t nfrac = pp < me ? me - pp - 1u : 0u;            // digits behind the point
    const uint32_t nd = me - first - (first < pp && pp < me ? 1u : 0u); // digits of s
    uint32_t end = me; // w = the digits in [first, end)
    if (nd > 19u) end = first + 19u + (first < pp && pp < first + 19u ? 1u : 0u);
    const uint32_t dropped = (uint32_t)__builtin_popcountll(brx_parse_range(end, me) & k.dig);
    const bool tail = (brx_parse_range(end, me) & k.nz) != 0;
    uint64_t w;
    if (first < pp && pp < end) w = brx_parse_dec_field(b, first, pp) * brx_parse_pow10(end - pp - 1u) + brx_parse_dec_field(b, pp + 1u, end);
    else w = brx_parse_dec_field(b, first, end);
    const int32_t q = ex - (int32_t)nfrac + (int32_t)dropped; // w * 10^q <= |x| < (w + 1) * 10^q, with equality iff no tail
    const uint64_t a = brx_f64_from_decimal(tab, w, q);
    if (tail && brx_f64_from_decimal(tab, w + 1u, q) != a) return brx_parse_f64_result(a | sign, BRX_PARSE_S_HARD);
    return brx_parse_f64_result(a | sign, (a == 0 || a == BRX_F64_INF) ? BRX_PARSE_S_RANGE : BRX_PARSE_S_OK);
}

// one lane, one record: THE PARSE, F64.  A record above 64 bytes has none of its bytes loaded.
template <class M>
BRX_TAKE_HD BrxParseF64Out brx_parse_f64_lane(M &mem, const BrxPow5 *tab, const uint8_t *arena, uint64_t span, BrxTakeRec r, uint32_t flags,
                                              uint32_t quote) {
    if (r.len > BRX_PARSE_LEN) return brx_parse_f64_result(0, BRX_PARSE_S_LONG);
    BrxParseBuf b;
    BrxParseMasks k;
    brx_parse_load(mem, arena, span, r, BRX_PARSE_K_DEC, flags, b, k);
    return brx_parse_f64_text(tab, b, k, (uint32_t)r.len, flags, quote);
}

// host side (brx_api.cpp)
void brx_launch_parse_f64(const BrxTakeArgs &a, uint32_t quote, uint64_t *val, uint8_t *status, void *hip_stream);
#endif
