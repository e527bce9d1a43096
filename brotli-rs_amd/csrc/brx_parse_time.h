// brx_parse_time.h -- shared by brx_parse_time.hip (kernel), brx_api.cpp (brx_parse_time_batch) and tools/parse_time_emu.cpp (the same
// text on a CPU, lane by lane).  Everything of the pass that is not HIP-specific lives here, around the unchanged brx_take.h (which
// bytes an entry's record is) and brx_parse.h (the record as eight words and its digit, non-zero and space masks, BRX_PARSE_K_DEC
// classification; the windows; the digit conversion).
//
// The definition is THE PARSE, TIME of include/brx.h (brx_parse_time_batch).  How it is computed here: the grammar has fixed places, so
// after the trim the digit mask is shifted to the text's first byte and "digits where digits must be" is one AND with a constant per
// part (date 0x36F of 10 bits, clock 0x1B of 5, seconds 0xC0), the punctuation a masked compare of the 8-byte window that holds it, a
// two-digit field one brx_parse_dec8 of that window.  The fraction ends at the first non-digit behind its mark (one bit scan), its kept
// part is one brx_parse_dec_field of at most 9 digits, "a dropped digit is not '0'" one test of the non-zero mask.  What is left behind
// the clock is the zone, told apart by its length (1, 3, 5 or 6 bytes).  The calendar is days-from-civil in 32 bits with divisions by
// constants only; the month lengths are a packed constant and the leap test.  The 64-bit bound is decided before the multiply, against
// the quotient and the remainder of the bound by 10^scale (constants: only scales 8 and 9 can reach it).
#ifndef BRX_PARSE_TIME_H
#define BRX_PARSE_TIME_H
#include <stdint.h>
#include "brx_parse.h"

#define BRX_TIME_K_DATE 0u  // == BRX_TIME_DATE (include/brx.h)
#define BRX_TIME_K_TIME 1u  // == BRX_TIME_TIME
#define BRX_TIME_K_STAMP 2u // == BRX_TIME_STAMP
#define BRX_TIME_Z_NONE (-32768) // == BRX_TIME_NO_ZONE

struct BrxParseTimeOut { int64_t val; uint32_t status; int32_t zone; };

BRX_TAKE_HD BrxParseTimeOut brx_parse_time_result(int64_t val, uint32_t status, int32_t zone) {
    BrxParseTimeOut o;
    o.val = val;
    o.status = status;
    o.zone = zone;
    return o;
}
BRX_TAKE_HD BrxParseTimeOut brx_parse_time_bad() { return brx_parse_time_result(0, BRX_PARSE_S_BAD, BRX_TIME_Z_NONE); }

// the two ASCII digits at bytes q, q + 1 of the window w (q <= 6) as a number
BRX_TAKE_HD uint32_t brx_parse_time_dd(uint64_t w, uint32_t q) { return (uint32_t)brx_parse_dec8(w << (8u * (6u - q)), 2u); }

// the length of month m = 1 .. 12 of year y: 28 + two bits of a packed constant (bits [2m, 2m + 2)), February by the leap test
BRX_TAKE_HD uint32_t brx_parse_time_month_len(uint32_t y, uint32_t m) {
    const uint32_t packed = (3u << 2) | (0u << 4) | (3u << 6) | (2u << 8) | (3u << 10) | (2u << 12) | (3u << 14) | (3u << 16) | (2u << 18) |
                            (3u << 20) | (2u << 22) | (3u << 24);
    const bool leap = (y % 4u) == 0 && ((y % 100u) != 0 || (y % 400u) == 0);
    return 28u + ((packed >> (2u * m)) & 3u) + ((m == 2u && leap) ? 1u : 0u);
}

// days from 1970-01-01 to y-m-d in the proleptic Gregorian calendar, y = 0 .. 9999, m = 1 .. 12: the years are counted from March of
// year -400, so that nothing goes below zero
BRX_TAKE_HD int32_t brx_parse_time_days(uint32_t y, uint32_t m, uint32_t d) {
    const uint32_t yy = y + 400u - (m <= 2u ? 1u : 0u), era = yy / 400u, yoe = yy - era * 400u;
    const uint32_t mp = m > 2u ? m - 3u : m + 9u, doy = (153u * mp + 2u) / 5u + d - 1u;
    const uint32_t doe = yoe * 365u + yoe / 4u - yoe / 100u + doy;
    return (int32_t)(era * 146097u + doe) - (719468 + 146097);
}

// ---- THE PARSE, TIME, steps 2 .. 8, on a loaded record of L <= 64 bytes -----------------------------------------------------------
BRX_TAKE_HD BrxParseTimeOut brx_parse_time_text(const BrxParseBuf b, const BrxParseMasks k, uint32_t L, uint32_t kind, uint32_t scale,
                                                uint32_t flags, uint32_t quote) {
    uint32_t lo = 0, e = L; // t = bytes [lo, e)
    if (flags & BRX_PARSE_F_SPACES) {
        const uint64_t ns = brx_parse_below(L) & ~k.sp;
        if (!ns) return brx_parse_time_result(0, BRX_PARSE_S_EMPTY, BRX_TIME_Z_NONE);
        lo = (uint32_t)__builtin_ctzll(ns);
        e = 64u - (uint32_t)__builtin_clzll(ns);
    }
    if ((flags & BRX_PARSE_F_QUOTED) && e - lo >= 2u && brx_parse_byte(b, lo) == quote && brx_parse_byte(b, e - 1u) == quote) {
        lo++;
        e--;
    }
    if (lo == e) return brx_parse_time_result(0, BRX_PARSE_S_EMPTY, BRX_TIME_Z_NONE);
    const uint32_t T = e - lo;                                // 1 .. 64, and lo < 64
    const uint64_t in = brx_parse_below(T);
    const uint64_t dg = (k.dig >> lo) & in, nz = (k.nz >> lo) & in; // bit q = byte q of t is a digit / a digit that is not '0'

    int64_t secs = 0;
    uint32_t o = 0; // where the clock starts in t
    if (kind != BRX_TIME_K_TIME) {
        if (T < 10u || (dg & 0x3FFu) != 0x36Fu) return brx_parse_time_bad();
        const uint64_t w0 = brx_parse_window(b, (int32_t)lo), w1 = brx_parse_window(b, (int32_t)lo + 8); // "YYYY-MM-" "DD?HH:MM"
        if ((w0 & 0xFF0000FF00000000ull) != 0x2D00002D00000000ull) return brx_parse_time_bad();
        const uint32_t y = (uint32_t)brx_parse_dec8(w0 << 32, 4u), mo = brx_parse_time_dd(w0, 5u), d = brx_parse_time_dd(w1, 0u);
        if (mo - 1u > 11u) return brx_parse_time_bad();
        if (d - 1u >= brx_parse_time_month_len(y, mo)) return brx_parse_time_bad();
        const int32_t days = brx_parse_time_days(y, mo, d);
        if (kind == BRX_TIME_K_DATE)
            return T == 10u ? brx_parse_time_result(days, BRX_PARSE_S_OK, BRX_TIME_Z_NONE) : brx_parse_time_bad();
        secs = (int64_t)days * 86400;
        if (T > 10u) {
            const uint32_t sep = (uint32_t)(w1 >> 16) & 0xFFu;
            if ((sep | 0x20u) != 0x74u && sep != 0x20u) return brx_parse_time_bad(); // 'T', 't' or a blank
            o = 11u;
        }
    }

    uint32_t fs = 0, fe = 0; // the fraction's digits are t[fs, fe)
    int32_t zone = BRX_TIME_Z_NONE;
    if (kind == BRX_TIME_K_TIME || T > 10u) {
        const uint64_t tm = dg >> o;
        if (T < o + 5u || (tm & 0x1Bu) != 0x1Bu) return brx_parse_time_bad();
        const uint64_t tw = brx_parse_window(b, (int32_t)(lo + o)); // "HH:MM:SS"
        if (((tw >> 16) & 0xFFu) != 0x3Au) return brx_parse_time_bad();
        const uint32_t hh = brx_parse_time_dd(tw, 0u), mi = brx_parse_time_dd(tw, 3u);
        uint32_t ss = 0, cur = o + 5u;
        if (T > cur && ((tw >> 40) & 0xFFu) == 0x3Au) {
            if ((tm & 0xC0u) != 0xC0u) return brx_parse_time_bad();
            ss = brx_parse_time_dd(tw, 6u);
            cur = o + 8u;
            const uint32_t mark = T > cur ? brx_parse_byte(b, lo + cur) : 0u;
            if (mark == 0x2Eu || mark == 0x2Cu) {
                fs = cur + 1u;
                const uint64_t nd = ~dg & ~brx_parse_below(fs); // (behind T nothing is a digit)
                fe = nd ? (uint32_t)__builtin_ctzll(nd) : 64u;
                if (fe == fs) return brx_parse_time_bad();
                cur = fe;
            }
        }
        if (hh > 23u || mi > 59u || ss > 59u) return brx_parse_time_bad();
        secs += (int64_t)(hh * 3600u + mi * 60u + ss);
        if (cur < T) { // the zone: 'Z', +DD, +DDDD or +DD:DD, and nothing else
            if (kind == BRX_TIME_K_TIME) return brx_parse_time_bad();
            const uint32_t rem = T - cur, c = brx_parse_byte(b, lo + cur);
            if (rem == 1u && (c | 0x20u) == 0x7Au) {
                zone = 0;
            } else {
                if ((c != 0x2Bu && c != 0x2Du) || (rem != 3u && rem != 5u && rem != 6u)) return brx_parse_time_bad();
                const uint64_t zm = dg >> (cur + 1u), zw = brx_parse_window(b, (int32_t)(lo + cur + 1u)); // "DD:DD", "DDDD" or "DD"
                uint32_t zmin = 0;
                if (rem == 3u) {
                    if (zm != 0x3u) return brx_parse_time_bad();
                } else if (rem == 5u) {
                    if (zm != 0xFu) return brx_parse_time_bad();
                    zmin = brx_parse_time_dd(zw, 2u);
                } else {
                    if (zm != 0x1Bu || ((zw >> 16) & 0xFFu) != 0x3Au) return brx_parse_time_bad();
                    zmin = brx_parse_time_dd(zw, 3u);
                }
                const uint32_t zh = brx_parse_time_dd(zw, 0u);
                if (zh > 23u || zmin > 59u) return brx_parse_time_bad();
                zone = (int32_t)(zh * 60u + zmin);
                if (c == 0x2Du) zone = -zone;
            }
            secs -= (int64_t)zone * 60;
        }
    }

    // V = secs * P + frac with P = 10^scale and 0 <= frac < P.  |secs| < 2^38 (years 0000 .. 9999 and a day of zone), so below scale 8
    // V stays inside 64 bits.  At scales 8 and 9 the bound is decided before the multiply, against its quotient and remainder by P:
    // 2^63 - 1 = qmax * P + rmax, and -2^63 = (-qmax - 1) * P + (P - rmax - 1).  The product then wraps to the right value.
    const uint32_t keep = fe - fs < scale ? fe - fs : scale;
    const uint64_t P = brx_parse_pow10(scale);
    const uint64_t frac = keep ? brx_parse_dec_field(b, lo + fs, lo + fs + keep) * brx_parse_pow10(scale - keep) : 0u;
    const bool inexact = (brx_parse_range(fs + keep, fe) & nz) != 0;
    if (scale >= 8u) {
        const int64_t qmax = scale == 9u ? 9223372036ll : 92233720368ll, rmax = scale == 9u ? 854775807ll : 54775807ll;
        const int64_t qmin = -qmax - 1, rmin = (int64_t)P - rmax - 1;
        if (secs > qmax || (secs == qmax && (int64_t)frac > rmax)) return brx_parse_time_result(INT64_MAX, BRX_PARSE_S_RANGE, BRX_TIME_Z_NONE);
        if (secs < qmin || (secs == qmin && (int64_t)frac < rmin)) return brx_parse_time_result(INT64_MIN, BRX_PARSE_S_RANGE, BRX_TIME_Z_NONE);
    }
    return brx_parse_time_result((int64_t)((uint64_t)secs * P + frac), inexact ? BRX_PARSE_S_INEXACT : BRX_PARSE_S_OK, zone);
}

// one lane, one record: THE PARSE, TIME.  A record above 64 bytes has none of its bytes loaded.
template <class M>
BRX_TAKE_HD BrxParseTimeOut brx_parse_time_lane(M &mem, const uint8_t *arena, uint64_t span, BrxTakeRec r, uint32_t kind, uint32_t scale,
                                                uint32_t flags, uint32_t quote) {
    if (r.len > BRX_PARSE_LEN) return brx_parse_time_result(0, BRX_PARSE_S_LONG, BRX_TIME_Z_NONE);
    BrxParseBuf b;
    BrxParseMasks k;
    brx_parse_load(mem, arena, span, r, BRX_PARSE_K_DEC, flags, b, k);
    return brx_parse_time_text(b, k, (uint32_t)r.len, kind, scale, flags, quote);
}

// host side (brx_api.cpp)
void brx_launch_parse_time(const BrxTakeArgs &a, uint32_t kind, uint32_t scale, uint32_t quote, int64_t *val, uint8_t *status, int16_t *zone,
                           void *hip_stream);
#endif
