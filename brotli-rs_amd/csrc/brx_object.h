// brx_object.h -- shared by brx_object.hip (the kernel), brx_api.cpp (brx_object_batch) and tools/object_emu.cpp (the same text on a
// CPU, lane by lane).  Everything of the pass that is not HIP-specific lives here: the resolution of an entry, the masks of a unit of
// 16 boundary bytes, one lane's walk of a short object (the lane path), the keys of one lane's members of a unit (both paths), the
// kind of a value and the stores of a slot.  The rule is THE RULE of include/brx.h (brx_object_batch); the boundaries that count, the
// units, the look at a key record and the names are brx_member.h's (brx_mb_count, brx_mb_valid, brx_mb_masks, brx_mb_key,
// brx_mb_key_is), a unit's load and its walk with the depth known are brx_elements.h's (brx_el_unit, brx_el_unit_walk: an object's
// walk is an array's with ':' where that has ',' and '}' where that has ']'); which bytes a key record is comes from brx_take.h.
//
// Memory goes through a policy type M so that the emulator sees every load and every store:
//   uint8_t M::ld8(const uint8_t *p), BrxTake128 M::ld128(const uint8_t *p)     arena bytes, as in brx_take.h
//   uint8_t M::ldw8(const uint8_t *p), BrxTake128 M::ldw128(const uint8_t *p)   bytes of `what`, 16 of them at any alignment
//   void M::st64(uint64_t *p, uint64_t v), st32(uint32_t *p, uint32_t v), st8(uint8_t *p, uint8_t v)   the slots (q, j)
// The tables (out_off, len, count, pos_off, pos, sel_stream, sel_rec) are read directly.
//
// How it is computed.  One lane owns one entry and walks the boundaries behind its opener in units of 16, from structural bit to
// structural bit, for at most BRX_OB_LONG boundaries (brx_ob_lane).  A ':' met at depth 1 is a member: its key record is looked at
// (brx_mb_key) and compared with the names one after the other; per name the lane keeps the last member that carries it (brx_ob_key:
// 8 small fields of one register, no array that a rolled loop would index) and stores every slot once at the end.  An object that has
// not ended by then is left to the wave, which starts over behind the opener and takes a ROW of 64 units per step: the depth in front
// of every unit comes from a scan of the units' bracket sums, every lane walks its unit with that depth (brx_el_unit_walk) and says
// where the object stops in it, if it does; the first such lane is the row's stop, the lanes behind it count nothing.  Every lane in
// front of the stop looks at the keys of its own depth-1 colons and keeps, per name, the last of them that carries it
// (brx_ob_unit_keys).  Per name the row's last lane with a match wins, and the winner of the rows so far is carried in lane q's
// register for name q.  WHO STORES: every slot (q, j) is written exactly once, by the thread that owns entry j -- at the end of its
// lane path, or behind the last row of the wave path from the carried winners -- so no slot's value depends on the order in which
// stores land.
#ifndef BRX_OBJECT_H
#define BRX_OBJECT_H
#include <stddef.h>
#include <stdint.h>
#include "brx_member.h"
#include "brx_elements.h"

#ifndef BRX_OB_UNITS
#define BRX_OB_UNITS 4u                           // units of 16 boundaries that one lane walks alone (measured: DESIGN.md 25)
#endif
#define BRX_OB_LONG (BRX_OB_UNITS * BRX_MB_UNIT)  // an object that has not ended this many boundaries behind its opener is the wave's
#define BRX_OB_ROW BRX_MB_ROW                     // boundaries per wave step
#define BRX_OB_OK 0u                              // == BRX_OBJECT_OK ...
#define BRX_OB_NONE 1u
#define BRX_OB_NOT_OBJECT 2u
#define BRX_OB_UNCLOSED 3u
#define BRX_OB_MISMATCH 4u

// everything the pass reads and writes, as the call got it (the names travel beside it: BrxMbNames, n = 0 in extent mode)
struct BrxObArgs {
    BrxTakeArgs a; // flags = BRX_TAKE_F_NO_DELIM, delim_len = 1, the selection and m: the key record of the member at k is record k
    const uint8_t *what;
    uint64_t *n_members;
    uint8_t *status;
    uint64_t *end;
    uint32_t *mem_stream; // NULL (all three): extent mode
    uint64_t *mem_rec;
    uint8_t *mem_kind;
    uint8_t *obj_flags;
};

// entry j, resolved: status BRX_OB_OK = an opener, to be walked
struct BrxObEntry {
    uint32_t status, i;
    uint64_t r, c, base; // the opener, C(i), pos_off[i]
};
struct BrxObRes { uint64_t n_members, end; uint32_t status, flags; };

// what follows a member's ':' (member's VALUE rule: a ']' closes nothing that a value could be)
BRX_TAKE_HD uint32_t brx_ob_kind(uint32_t w) {
    return (w == 0x2Cu || w == 0x7Du) ? BRX_MB_K_SCALAR : w == 0x7Bu ? BRX_MB_K_OBJECT : w == 0x5Bu ? BRX_MB_K_ARRAY : BRX_MB_K_BAD;
}

template <class M>
BRX_TAKE_HD BrxObEntry brx_ob_entry(M &mem, const BrxObArgs &x, uint64_t j) {
    BrxObEntry en = {BRX_OB_NONE, 0, 0, 0, 0};
    const uint64_t i = x.a.sel_stream[j], r = x.a.sel_rec[j];
    if (i >= x.a.n) return en;
    en.i = (uint32_t)i;
    en.c = brx_mb_count(x.a, i);
    if (r >= en.c) return en;
    en.r = r;
    en.base = x.a.pos_off[i];
    en.status = mem.ldw8(x.what + en.base + r) == 0x7Bu ? BRX_OB_OK : BRX_OB_NOT_OBJECT;
    return en;
}

// elements' masks for an object's walk: the closer that is the right one is '}', what separates at depth 1 is ':'
BRX_TAKE_HD BrxElMasks brx_ob_masks(BrxTake128 v) {
    const BrxMbMasks b = brx_mb_masks(v);
    BrxElMasks k = {b.open, b.close, brx_text_eq16(v, 0x7Du), b.nl, b.colon};
    return k;
}

// ---- the members that carry a name ------------------------------------------------------------------------------------------------
// The key of the member at boundary km of stream i against the names: `last` holds, per name q, a field of 8 bits at 8 q, and every
// name that the key carries has its field set to `tag` (1 .. 255; 0 = no member so far).  Members are looked at in their order, so a
// field holds the tag of the LAST member that carries the name.  Returns the flag bits of the key.
template <class M>
BRX_TAKE_HD uint32_t brx_ob_key(M &mem, const BrxObArgs &x, const BrxMbNames &nm, uint64_t i, uint64_t km, uint32_t tag, uint64_t &last) {
    BrxTakeArgs a = x.a; // (the record rule under BRX_TAKE_NO_DELIM with D = 1 as constants: its other branches fold away)
    a.flags = BRX_TAKE_F_NO_DELIM; a.delim_len = 1u;
    return brx_mb_key(mem, a, i, km, [&](const BrxMbKey &ky) {
        // (not unrolled: the names stay in the launch arguments, one name per turn -- brx_mb_member)
#pragma unroll 1
        for (uint32_t q = 0; q < nm.n; q++) {
            if (brx_mb_key_is(nm, q, ky)) last = (last & ~((uint64_t)0xFFu << (8u * q))) | ((uint64_t)tag << (8u * q));
        }
    });
}
BRX_TAKE_HD uint32_t brx_ob_last_of(uint64_t last, uint32_t q) { return (uint32_t)(last >> (8u * q)) & 0xFFu; }

// ---- the slots of entry j: (q, j) at q * m + j --------------------------------------------------------------------------------------
// name q's slot from the winner v = k + 1 of the last member that carries it, or 0 (MISSING); en = NULL: an entry that is no opener.
// The kind is the byte of what at v, bounded by C(i).  mem_stream is sel_stream[j] whatever that is.
template <class M>
BRX_TAKE_HD void brx_ob_store_slot(M &mem, const BrxObArgs &x, const BrxObEntry *en, uint32_t q, uint64_t j, uint64_t v) {
    const uint64_t at = (uint64_t)q * x.a.m + j;
    uint32_t kind = BRX_MB_K_MISSING;
    if (v) kind = v < en->c ? brx_ob_kind(mem.ldw8(x.what + en->base + v)) : BRX_MB_K_BAD;
    mem.st32(x.mem_stream + at, x.a.sel_stream[j]);
    mem.st64(x.mem_rec + at, v ? v : ~(uint64_t)0);
    mem.st8(x.mem_kind + at, (uint8_t)kind);
}
// every name's slot of an entry that is no opener
template <class M>
BRX_TAKE_HD void brx_ob_store_missing(M &mem, const BrxObArgs &x, uint32_t n_names, uint64_t j) {
#pragma unroll 1
    for (uint32_t q = 0; q < n_names; q++) brx_ob_store_slot(mem, x, (const BrxObEntry *)0, q, j, 0u);
}

// The keys of one lane's members `sep` (the depth-1 colons of the unit at k0 in front of its stop) against the names; the tag of the
// member at the unit's bit b is tag0 + b + 1.  Returns the flag bits of the keys.
template <class M>
BRX_TAKE_HD uint32_t brx_ob_unit_keys(M &mem, const BrxObArgs &x, const BrxMbNames &nm, uint32_t i, uint64_t k0, uint32_t sep, uint32_t tag0,
                                      uint64_t &last) {
    uint32_t flags = 0;
    for (; sep; sep &= sep - 1u) {
        const uint32_t b = (uint32_t)__builtin_ctz(sep);
        flags |= brx_ob_key(mem, x, nm, i, k0 + b, tag0 + b + 1u, last);
    }
    return flags;
}

// The lane path: the object of entry `en` (status BRX_OB_OK) walked by one lane, unit by unit as the wave path does it, the depth in
// front of a unit from the units in front (at most BRX_OB_LONG brackets: no clamp).  true: it ended within BRX_OB_LONG boundaries,
// `res` is the entry's and, with names, every slot of the entry has been stored, once; false: it is the wave's and nothing was
// stored.  The tag of the member at km is km - r (1 .. BRX_OB_LONG).
template <bool NAMES, class M>
BRX_TAKE_HD bool brx_ob_lane(M &mem, const BrxObArgs &x, const BrxMbNames &nm, const BrxObEntry &en, uint64_t j, BrxObRes &res) {
    int32_t e = 1;
    uint64_t t = 0, last = 0;
    uint32_t how = BRX_EL_STOP_NONE, flags = 0;
#pragma unroll 1
    for (uint32_t g = 0; g < BRX_OB_UNITS && how == BRX_EL_STOP_NONE; g++) { // (rolled: one copy of the look at a key, not four)
        const uint64_t k0 = en.r + 1u + g * BRX_MB_UNIT;
        const uint32_t nv = brx_mb_valid(en.c, k0);
        const BrxElMasks k = brx_ob_masks(brx_el_unit(mem, x.what, en.base, en.c, k0, nv));
        const BrxElUnit u = brx_el_unit_walk(k, nv, e);
        t += (uint32_t)__builtin_popcount(u.sep);
        if (NAMES) flags |= brx_ob_unit_keys(mem, x, nm, en.i, k0, u.sep, g * BRX_MB_UNIT, last);
        how = u.stop;
        res.end = k0 + u.at;
        e += brx_el_unit_sum(k);
    }
    if (how == BRX_EL_STOP_NONE) return false;
    res.status = how == BRX_EL_STOP_OK ? BRX_OB_OK : how == BRX_EL_STOP_MISMATCH ? BRX_OB_MISMATCH : BRX_OB_UNCLOSED;
    res.n_members = t;
    res.flags = flags;
    if (NAMES) {
#pragma unroll 1
        for (uint32_t q = 0; q < nm.n; q++) {
            const uint32_t tag = brx_ob_last_of(last, q);
            brx_ob_store_slot(mem, x, &en, q, j, tag ? en.r + tag + 1u : 0u);
        }
    }
    return true;
}

// host side (brx_api.cpp): the one launch of a call
void brx_launch_object(const BrxObArgs &x, const BrxMbNames &nm, void *hip_stream);
#endif
