// brx_elements.h -- shared by brx_elements.hip (the kernel), brx_api.cpp (brx_elements_batch) and tools/elements_emu.cpp (the same text
// on a CPU, lane by lane).  Everything of the pass that is not HIP-specific lives here: the resolution of an entry, the masks of a unit
// of 16 boundary bytes, one lane's walk of a short array (the lane path), one lane's share of a row of a long one (the wave path), the
// blank test of `[]` and the stores of an element.  The rule is THE RULE of include/brx.h (brx_elements_batch); the boundaries that
// count, the units and their bounds are brx_member.h's; which bytes record r + 1 is comes from brx_take.h (brx_take_record).
//
// Memory goes through a policy type M so that the emulator sees every load and every store:
//   uint8_t M::ld8(const uint8_t *p), BrxTake128 M::ld128(const uint8_t *p)     arena bytes, as in brx_take.h
//   uint8_t M::ldw8(const uint8_t *p), BrxTake128 M::ldw128(const uint8_t *p)   bytes of `what`, 16 of them at any alignment
//   void M::st64(uint64_t *p, uint64_t v), st32(uint32_t *p, uint32_t v), st8(uint8_t *p, uint8_t v)   the results
// The tables (out_off, len, count, pos_off, pos, sel_stream, sel_rec, el_off) are read directly.
//
// How it is computed.  One lane owns one entry and walks the boundaries behind its opener in units of 16, from structural bit to
// structural bit, for at most BRX_EL_LONG boundaries (brx_el_lane).  An array that has not ended by then is left to the wave, which
// starts over behind the opener and takes a ROW of 64 units per step: every lane sums its unit's brackets (brx_el_unit_sum), the sums
// are scanned across the lanes, every lane walks its unit with the depth in front of it known (brx_el_unit_walk) and says where the
// array stops in it, if it does; the first such lane is the row's stop, the lanes behind it count nothing.  The depth-1 commas in
// front of the stop are the SEPARATORS: separator number t (the opener is number 0) begins element t, and that is an element iff
// something ends it -- a later separator or the closer.  So a lane stores the elements behind all its separators but its last, and
// behind its last where a later lane of the row has one or the row stops at a closer; the row's last separator travels to the next row
// as the PENDING one (at first the opener) and is stored by lane 0 of the row that ends it.  Depth, separators so far and the pending
// separator are carried from row to row in scalars.
#ifndef BRX_ELEMENTS_H
#define BRX_ELEMENTS_H
#include <stddef.h>
#include <stdint.h>
#include "brx_member.h"

#ifndef BRX_EL_UNITS
#define BRX_EL_UNITS 4u                           // units of 16 boundaries that one lane walks alone (measured: DESIGN.md 24)
#endif
#define BRX_EL_LONG (BRX_EL_UNITS * BRX_MB_UNIT)  // an array that has not ended this many boundaries behind its opener is the wave's
#define BRX_EL_ROW BRX_MB_ROW                     // boundaries per wave step
#define BRX_EL_MAX_BLANK 64u                      // == BRX_ELEMENTS_MAX_BLANK (include/brx.h)
#define BRX_EL_OK 0u                              // == BRX_ELEMENTS_OK ...
#define BRX_EL_NONE 1u
#define BRX_EL_NOT_ARRAY 2u
#define BRX_EL_UNCLOSED 3u
#define BRX_EL_MISMATCH 4u
// how a unit's walk stopped (the wave path)
#define BRX_EL_STOP_NONE 0u
#define BRX_EL_STOP_OK 1u
#define BRX_EL_STOP_MISMATCH 2u
#define BRX_EL_STOP_OPEN 3u // a line feed, or the stream's last boundary that counts is behind

// everything the pass reads and writes, as the call got it
struct BrxElArgs {
    BrxTakeArgs a; // flags = BRX_TAKE_F_NO_DELIM, delim_len = 1, the selection and m: record r + 1 of the blank test
    const uint8_t *what;
    uint64_t *n_elem;
    uint8_t *status;
    uint64_t *end;
    const uint64_t *el_off; // NULL: count mode
    uint64_t total;
    uint32_t *el_stream;
    uint64_t *el_rec;
    uint8_t *el_kind;
};

// entry j, resolved: status BRX_EL_OK = an opener, to be walked
struct BrxElEntry {
    uint32_t status, i;
    uint64_t r, c, base; // the opener, C(i), pos_off[i]
    uint64_t off, lim;   // fill mode: element t < lim goes to slot off + t
};
struct BrxElRes { uint64_t n_elem, end; uint32_t status; };

BRX_TAKE_HD uint32_t brx_el_kind(uint32_t w) {
    return (w == 0x2Cu || w == 0x5Du || w == 0x7Du) ? BRX_MB_K_SCALAR : w == 0x7Bu ? BRX_MB_K_OBJECT : w == 0x5Bu ? BRX_MB_K_ARRAY : BRX_MB_K_BAD;
}

template <class M>
BRX_TAKE_HD BrxElEntry brx_el_entry(M &mem, const BrxElArgs &x, uint64_t j) {
    BrxElEntry en = {BRX_EL_NONE, 0, 0, 0, 0, 0, 0};
    const uint64_t i = x.a.sel_stream[j], r = x.a.sel_rec[j];
    if (i >= x.a.n) return en;
    en.i = (uint32_t)i;
    en.c = brx_mb_count(x.a, i);
    if (r >= en.c) return en;
    en.r = r;
    en.base = x.a.pos_off[i];
    en.status = BRX_EL_OK;
    if (mem.ldw8(x.what + en.base + r) != 0x5Bu) en.status = BRX_EL_NOT_ARRAY;
    if (x.el_off) { // the room of j, cut at total
        const uint64_t s = x.el_off[j], e = j + 1u < x.a.m ? x.el_off[j + 1u] : x.total;
        const uint64_t room = e > s ? e - s : 0u, left = s < x.total ? x.total - s : 0u;
        en.off = s;
        en.lim = room < left ? room : left;
    }
    return en;
}

// nv <= 16 bytes of `what` of a stream with c boundaries that count, from its boundary k0 on (brx_mb_valid), the bytes behind them 0 and
// not loaded: member's unit, except that a unit cut by the stream's end is ONE wide load of the stream's last 16 boundaries that
// count, shifted down, where the stream has 16 (the bytes of a cut unit one by one cost a wave that waits for it 15 loads in a row)
template <class M>
BRX_TAKE_HD BrxTake128 brx_el_unit(M &mem, const uint8_t *what, uint64_t base, uint64_t c, uint64_t k0, uint32_t nv) {
    BrxTake128 v = {0, 0};
    if (nv == 0) return v;
    if (nv == BRX_MB_UNIT || c < BRX_MB_UNIT) return brx_mb_unit(mem, what, base + k0, nv);
    v = mem.ldw128(what + base + (c - BRX_MB_UNIT)); // (k0 + nv == c: the unit's bytes are the load's last nv)
    const uint32_t sh = 8u * (BRX_MB_UNIT - nv);     // 8 .. 120
    if (sh < 64u) { v.lo = (v.lo >> sh) | (v.hi << (64u - sh)); v.hi >>= sh; }
    else { v.lo = v.hi >> (sh - 64u); v.hi = 0; }
    return v;
}
BRX_TAKE_HD uint32_t brx_el_byte(BrxTake128 v, uint32_t b) { return (uint32_t)((b < 8u ? v.lo >> (8u * b) : v.hi >> (8u * (b - 8u))) & 0xFFu); }

// member's masks, the two closers apart, and the commas
struct BrxElMasks { uint32_t open, close, sq, nl, comma; };
BRX_TAKE_HD BrxElMasks brx_el_masks(BrxTake128 v) {
    const BrxMbMasks b = brx_mb_masks(v);
    BrxElMasks k = {b.open, b.close, brx_text_eq16(v, 0x5Du), b.nl, brx_text_eq16(v, 0x2Cu)};
    return k;
}

// element t of the entry begins behind separator s (a boundary of the stream, s + 1 < C(i)): with its kind where the caller has it,
// else from the byte of `what` at s + 1
template <class M>
BRX_TAKE_HD void brx_el_store(M &mem, const BrxElArgs &x, const BrxElEntry &en, uint64_t t, uint64_t s, uint32_t kind) {
    if (t >= en.lim) return;
    const uint64_t at = en.off + t;
    mem.st32(x.el_stream + at, en.i);
    mem.st64(x.el_rec + at, s + 1u);
    mem.st8(x.el_kind + at, (uint8_t)kind);
}
template <class M>
BRX_TAKE_HD void brx_el_store_at(M &mem, const BrxElArgs &x, const BrxElEntry &en, uint64_t t, uint64_t s) {
    if (t >= en.lim) return;
    brx_el_store(mem, x, en, t, s, brx_el_kind(mem.ldw8(x.what + en.base + s + 1u)));
}

// record k of stream i is at most 64 bytes and holds nothing but 0x20, 0x09 and 0x0D (an empty record is blank)
template <class M>
BRX_TAKE_HD bool brx_el_blank(M &mem, const BrxTakeArgs &args, uint64_t i, uint64_t k) {
    BrxTakeArgs a = args; // (the record rule under BRX_TAKE_NO_DELIM with D = 1, whatever the caller left in these two)
    a.flags = BRX_TAKE_F_NO_DELIM; a.delim_len = 1u;
    const BrxTakeRec r = brx_take_record(mem, a, i, k);
    if (r.len > BRX_EL_MAX_BLANK) return false;
    const uint32_t L = (uint32_t)r.len;
    // (wide loads stay inside the STREAM, as in brx_mb_member)
    const uint8_t *p = a.out + r.src, *lo_a = a.out + a.out_off[i], *hi_a = lo_a + a.len[i];
    uint64_t blank = 0;
    for (uint32_t g = 0; g < BRX_EL_MAX_BLANK / 16u; g++) {
        if (L > 16u * g) {
            const uint32_t n_ = L - 16u * g < 16u ? L - 16u * g : 16u;
            const BrxTake128 v_ = brx_take_place(brx_take_fetch(mem, p + 16u * g, n_, lo_a, hi_a), 0u, n_);
            blank |= (uint64_t)(brx_text_eq16(v_, 0x20u) | brx_text_eq16(v_, 0x09u) | brx_text_eq16(v_, 0x0Du)) << (16u * g);
        }
    }
    return (blank & brx_mb_below(L)) == brx_mb_below(L);
}

// The lane path: the array of entry `en` (status BRX_EL_OK) walked by one lane.  true: it ended within BRX_EL_LONG boundaries and
// `res` is the entry's; false: it is the wave's, and what this lane stored stands (the wave stores it again).  The kind of the
// element in hand is the byte behind its separator: the unit's next byte, or the next unit's first (BRX_EL_K_NEXT until that is loaded),
// so the lane loads nothing but its units.
#define BRX_EL_K_NEXT 0xFFu
template <bool FILL, class M>
BRX_TAKE_HD bool brx_el_lane(M &mem, const BrxElArgs &x, const BrxElEntry &en, BrxElRes &res) {
    int32_t e = 1;
    uint64_t s = en.r, t = 0;
    uint32_t pk = BRX_EL_K_NEXT, how = BRX_EL_STOP_NONE;
    for (uint32_t g = 0; g < BRX_EL_UNITS && how == BRX_EL_STOP_NONE; g++) {
        const uint64_t k0 = en.r + 1u + g * BRX_MB_UNIT;
        const uint32_t nv = brx_mb_valid(en.c, k0);
        const BrxTake128 v = brx_el_unit(mem, x.what, en.base, en.c, k0, nv);
        const BrxElMasks k = brx_el_masks(v);
        const uint32_t last = nv < BRX_MB_UNIT ? 1u << nv : 0u; // C(i) stands in this unit
        if (FILL && pk == BRX_EL_K_NEXT) pk = brx_el_kind(brx_el_byte(v, 0u));
        if (!FILL && e == 1 && !(k.open | k.close | k.nl | last)) { // nothing but commas and neutral bytes: their number
            if (k.comma) {
                t += (uint32_t)__builtin_popcount(k.comma);
                s = k0 + (31u - (uint32_t)__builtin_clz(k.comma));
            }
            continue;
        }
        for (uint32_t todo = k.open | k.close | k.nl | k.comma | last; todo; todo &= todo - 1u) {
            const uint32_t b = (uint32_t)__builtin_ctz(todo), bit = 1u << b;
            if (bit & (last | k.nl)) { // (bytes behind nv are 0: no mask has a bit at or behind `last`)
                res.end = k0 + b;
                how = BRX_EL_STOP_OPEN;
                break;
            }
            if (k.open & bit) e++;
            else if (k.close & bit) {
                if (--e == 0) {
                    res.end = k0 + b;
                    how = (k.sq & bit) ? BRX_EL_STOP_OK : BRX_EL_STOP_MISMATCH;
                    break;
                }
            } else if (e == 1) { // a separator: it ends the element in hand and begins the next
                if (FILL) {
                    brx_el_store(mem, x, en, t, s, pk);
                    pk = b + 1u < BRX_MB_UNIT ? brx_el_kind(brx_el_byte(v, b + 1u)) : BRX_EL_K_NEXT;
                }
                t++;
                s = k0 + b;
            }
        }
    }
    if (how == BRX_EL_STOP_NONE) return false;
    res.status = how == BRX_EL_STOP_OK ? BRX_EL_OK : how == BRX_EL_STOP_MISMATCH ? BRX_EL_MISMATCH : BRX_EL_UNCLOSED;
    if (how != BRX_EL_STOP_OPEN && !(res.end == en.r + 1u && brx_el_blank(mem, x.a, en.i, res.end))) { // (not [] or [ ]): the last element
        if (FILL) brx_el_store(mem, x, en, t, s, pk);
        t++;
    }
    res.n_elem = t;
    return true;
}

// ---- the wave path: one lane's share of a row --------------------------------------------------------------------------------
BRX_TAKE_HD int32_t brx_el_unit_sum(const BrxElMasks &k) { return (int32_t)__builtin_popcount(k.open) - (int32_t)__builtin_popcount(k.close); }

// the depth in front of a unit as its walk takes it: the row's carry plus the lanes in front, held to where a unit of 16 can tell
BRX_TAKE_HD int32_t brx_el_depth(int64_t carry, int32_t in_front) {
    const int64_t d = carry + in_front;
    return d > 64 ? 64 : d < -64 ? -64 : (int32_t)d;
}

struct BrxElUnit { uint32_t sep, stop, at; }; // the unit's separators in front of its stop; how it stops (BRX_EL_STOP_*) and at which bit
// One lane, one unit of nv boundaries with depth e in front of it.  (A lane behind the row's stop has a depth that means nothing; what
// it returns is dropped.)
BRX_TAKE_HD BrxElUnit brx_el_unit_walk(const BrxElMasks &k, uint32_t nv, int32_t e) {
    BrxElUnit u = {0, BRX_EL_STOP_NONE, 0};
    const uint32_t last = nv < BRX_MB_UNIT ? 1u << nv : 0u;
    if (!(k.open | k.close | k.nl | last)) {
        if (e == 1) u.sep = k.comma;
        return u;
    }
    for (uint32_t todo = k.open | k.close | k.nl | k.comma | last; todo; todo &= todo - 1u) {
        const uint32_t b = (uint32_t)__builtin_ctz(todo), bit = 1u << b;
        if (bit & (last | k.nl)) { u.stop = BRX_EL_STOP_OPEN; u.at = b; return u; }
        if (k.open & bit) e++;
        else if (k.close & bit) {
            if (--e == 0) { u.stop = (k.sq & bit) ? BRX_EL_STOP_OK : BRX_EL_STOP_MISMATCH; u.at = b; return u; }
        } else if (e == 1) u.sep |= bit;
    }
    return u;
}

// Fill mode: the elements behind this lane's separators `sep` of the unit v at k0, the first of them element t0; `later`: something in
// the row ends the element behind the lane's last separator.  The kind's byte is the unit's next one; behind the unit's last byte it
// is one more byte of what (in the next lane's unit or the next row's: an element that something ends has s + 1 < C(i)).
template <class M>
BRX_TAKE_HD void brx_el_unit_store(M &mem, const BrxElArgs &x, const BrxElEntry &en, uint64_t k0, BrxTake128 v, uint32_t sep, uint64_t t0,
                                   bool later) {
    for (; sep; sep &= sep - 1u, t0++) {
        if (!(sep & (sep - 1u)) && !later) return;
        const uint32_t b = (uint32_t)__builtin_ctz(sep);
        if (b + 1u < BRX_MB_UNIT) brx_el_store(mem, x, en, t0, k0 + b, brx_el_kind(brx_el_byte(v, b + 1u)));
        else brx_el_store_at(mem, x, en, t0, k0 + b);
    }
}

// host side (brx_api.cpp): the one launch of a call
void brx_launch_elements(const BrxElArgs &x, void *hip_stream);
#endif
