// brx_hash.h -- shared by brx_hash.hip (kernel), brx_api.cpp (brx_hash_batch) and tools/hash_emu.cpp (the same text on a CPU, lane by
// lane).  Everything of the pass that is not HIP-specific lives here: the arithmetic mod p = 2^61 - 1, the key and its powers, the
// value of a 16-byte unit, the Horner steps, the tail of a record, the lane path (one lane, one record) and one lane's share of the
// wave path (64 lanes, one record).  Which bytes an entry's record is comes from brx_take.h (brx_take_entry_record), and they are
// loaded through brx_take_fetch, with the memory policy M of brx_take.h (ld8, ld128): a 16-byte load only where all 16 bytes lie
// inside the arena, else the record's own bytes one by one.
//
// The definition (include/brx.h, brx_hash_batch): for a record r[0 .. L) with U = ceil(L / 4) little-endian 32-bit words c_u (bytes at
// or behind L taken as 0), S(r) = sum_{u<U} c_u K^(U-u) mod p, h(r) = (L + S(r)) mod p, hash = mix(h).  S composes: with A a whole
// number of words, S(A || B) = S(A) K^(U_B) + S(B).  Horner word by word is acc = (acc + c) K; unit by unit (four words) it is
// acc = acc K^4 + (c0 K^4 + c1 K^3 + c2 K^2 + c3 K).
#ifndef BRX_HASH_H
#define BRX_HASH_H
#include <stdint.h>
#include "brx_take.h"

#define BRX_HASH_P (((uint64_t)1 << 61) - 1u)
#define BRX_HASH_LONG 1024u      // records of this many bytes and more are hashed by their whole wave (one row = 64 lanes x 16 bytes)
#define BRX_HASH_UNIT 16u        // bytes of a unit: four words
#define BRX_HASH_ROW_WORDS 256u  // words of a row
#ifndef BRX_HASH_GROUP
#define BRX_HASH_GROUP 4u        // whole rows that a lane takes between two sums across the wave: their loads are in flight together
#endif

// K, K^2, K^3, K^4 and the row stride K^256, computed once per call on the host and passed as launch arguments
struct BrxHashKeys { uint64_t k1, k2, k3, k4, k256; };

// any x -> [0, p)
BRX_TAKE_HD uint64_t brx_hash_red(uint64_t x) {
    x = (x & BRX_HASH_P) + (x >> 61); // <= p + 7
    return x >= BRX_HASH_P ? x - BRX_HASH_P : x;
}

// a b mod p for a, b < 2^61, from 32 x 32 -> 64 multiplies.  With a = a1 2^32 + a0, b = b1 2^32 + b0 (a1, b1 < 2^29):
// a b = a1 b1 2^64 + (a1 b0 + a0 b1) 2^32 + a0 b0, and 2^61 = 1, 2^64 = 8 (mod p).
BRX_TAKE_HD uint64_t brx_hash_mul(uint64_t a, uint64_t b) {
    const uint32_t a0 = (uint32_t)a, a1 = (uint32_t)(a >> 32), b0 = (uint32_t)b, b1 = (uint32_t)(b >> 32);
    const uint64_t hh = (uint64_t)a1 * b1;                       // < 2^58
    const uint64_t mid = (uint64_t)a1 * b0 + (uint64_t)a0 * b1;  // < 2^62
    const uint64_t ll = (uint64_t)a0 * b0;
    // mid 2^32 = (mid >> 29) 2^61 + (mid & (2^29 - 1)) 2^32
    const uint64_t s = (hh << 3) + (mid >> 29) + ((mid & 0x1FFFFFFFu) << 32) + (ll & BRX_HASH_P) + (ll >> 61); // < 2^63
    return brx_hash_red(s);
}

BRX_TAKE_HD uint64_t brx_hash_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// K(seed) = 2 + mix(seed + 0x9E3779B97F4A7C15) mod (p - 3), and its powers
BRX_TAKE_HD BrxHashKeys brx_hash_keys(uint64_t seed) {
    BrxHashKeys k;
    k.k1 = 2u + brx_hash_mix(seed + 0x9E3779B97F4A7C15ull) % (BRX_HASH_P - 3u);
    k.k2 = brx_hash_mul(k.k1, k.k1);
    k.k3 = brx_hash_mul(k.k2, k.k1);
    k.k4 = brx_hash_mul(k.k2, k.k2);
    uint64_t x = k.k4; // K^4 -> K^256: six squarings
    for (int t = 0; t < 6; t++) x = brx_hash_mul(x, x);
    k.k256 = x;
    return k;
}

// c k as the pair (c (k mod 2^32) folded below 2^61 + 8, c (k >> 32) < 2^61) for a 32-bit c and k < 2^61
#define BRX_HASH_TERM(c, k, lo, hi) do { const uint64_t t_ = (uint64_t)(c) * (uint32_t)(k); lo += (t_ & BRX_HASH_P) + (t_ >> 61); \
                                         hi += (uint64_t)(c) * (uint32_t)((k) >> 32); } while (0)

// lo + hi 2^32 mod p for lo < 2^63 + 32, hi < 2^63:  hi 2^32 = (hi >> 29) 2^61 + (hi & (2^29 - 1)) 2^32
BRX_TAKE_HD uint64_t brx_hash_fold(uint64_t lo, uint64_t hi) {
    return brx_hash_red((lo & BRX_HASH_P) + (lo >> 61) + (hi >> 29) + ((hi & 0x1FFFFFFFu) << 32)); // < 2^62 + 2^35
}

// the value of a whole unit, c0 K^4 + c1 K^3 + c2 K^2 + c3 K mod p: four 93-bit products accumulated as two sums, reduced once
BRX_TAKE_HD uint64_t brx_hash_unit(BrxTake128 v, const BrxHashKeys &k) {
    uint64_t lo = 0, hi = 0; // lo < 2^63 + 32, hi < 2^63: the value is lo + hi 2^32
    BRX_HASH_TERM((uint32_t)v.lo, k.k4, lo, hi);
    BRX_HASH_TERM((uint32_t)(v.lo >> 32), k.k3, lo, hi);
    BRX_HASH_TERM((uint32_t)v.hi, k.k2, lo, hi);
    BRX_HASH_TERM((uint32_t)(v.hi >> 32), k.k1, lo, hi);
    return brx_hash_fold(lo, hi);
}

// Horner, a whole unit: acc K^4 + unit
BRX_TAKE_HD uint64_t brx_hash_step(uint64_t acc, BrxTake128 v, const BrxHashKeys &k) {
    return brx_hash_red(brx_hash_mul(acc, k.k4) + brx_hash_unit(v, k));
}

// Horner over a record's last unit, n = 1 .. 16 bytes of it inside the record (v masked to them, so the words behind them are 0): with
// w = ceil(n / 4) words, acc K^w + (c0 K^w + c1 K^(w-1) + c2 K^(w-2)), the weights chosen by w
BRX_TAKE_HD uint64_t brx_hash_tail(uint64_t acc, BrxTake128 v, uint32_t n, const BrxHashKeys &k) {
    if (n > 12u) return brx_hash_step(acc, v, k);
    const uint64_t e0 = n <= 4u ? k.k1 : (n <= 8u ? k.k2 : k.k3), e1 = n <= 8u ? k.k1 : k.k2; // (c1 = 0 for w = 1, c2 = 0 for w < 3)
    uint64_t lo = 0, hi = 0;
    BRX_HASH_TERM((uint32_t)v.lo, e0, lo, hi);
    BRX_HASH_TERM((uint32_t)(v.lo >> 32), e1, lo, hi);
    BRX_HASH_TERM((uint32_t)v.hi, k.k1, lo, hi);
    return brx_hash_red(brx_hash_mul(acc, e0) + brx_hash_fold(lo, hi));
}

// S of the record -> the hash
BRX_TAKE_HD uint64_t brx_hash_finish(uint64_t S, uint64_t L) { return brx_hash_mix(brx_hash_red(brx_hash_red(L) + S)); }

// n = 1 .. 16 bytes of the record at p, the bytes behind them 0: one 16-byte load where all 16 lie inside the arena, else by the byte.
// (A WHOLE unit of a record lies inside its stream, so inside the arena: those are loaded by mem.ld128 without asking.)
template <class M>
BRX_TAKE_HD BrxTake128 brx_hash_fetch(M &mem, const uint8_t *p, uint32_t n, const uint8_t *arena, uint64_t span) {
    return brx_take_place(brx_take_fetch(mem, p, n, arena, arena + span), 0, n);
}

// ---- the lane path: one lane, one record of fewer than BRX_HASH_LONG bytes ------------------------------------------------------
template <class M>
BRX_TAKE_HD uint64_t brx_hash_lane(M &mem, const uint8_t *arena, uint64_t span, BrxTakeRec r, const BrxHashKeys &k) {
    const uint8_t *p = arena + r.src;
    const uint32_t full = (uint32_t)(r.len / BRX_HASH_UNIT), rest = (uint32_t)(r.len % BRX_HASH_UNIT);
    uint64_t acc = 0;
    for (uint32_t g = 0; g < full; g++) acc = brx_hash_step(acc, mem.ld128(p + (uint64_t)g * BRX_HASH_UNIT), k);
    if (rest) acc = brx_hash_tail(acc, brx_hash_fetch(mem, p + (uint64_t)full * BRX_HASH_UNIT, rest, arena, span), rest, k);
    return brx_hash_finish(acc, r.len);
}

// ---- the wave path: 64 lanes, one record of L >= 1 bytes ------------------------------------------------------------------------
// The record has N = ceil(L / 16) units in rows of 64; lane l takes unit 64 row + l.  Every row but the last is whole:
//   row = sum_l unit_l W_l  with  W_l = K^(4 (63 - l)),     acc = acc K^256 + row.
// BRX_HASH_GROUP whole rows at a time are joined inside the lane first, x_l = ((u0 K^256 + u1) K^256 + u2) K^256 + u3 of the lane's four
// units, so that their loads are in flight together and the wave is summed once per group:  acc = acc K^(256 GROUP) + sum_l x_l W_l.
// The last row has nu = 1 .. 64 units, the last of them with n = 1 .. 16 bytes.  The units in front of the last one and the rows
// so far are joined by the same weights, taken from other lanes:
//   X = acc W_(64-nu) + sum_{l < nu-1} unit_l W_(l+65-nu)        (= S of everything in front of the last unit)
// and the last unit goes on top by brx_hash_tail(X, ...) in lane nu - 1.  Nothing behind the record is loaded: a lane without a
// unit loads nothing.

// W_l, by square and multiply on K^4 (exponent 63 - l < 64)
BRX_TAKE_HD uint64_t brx_hash_lane_weight(const BrxHashKeys &k, uint32_t lane) {
    uint64_t w = 1, b = k.k4;
    for (uint32_t e = 63u - lane; e; e >>= 1) {
        if (e & 1u) w = brx_hash_mul(w, b);
        b = brx_hash_mul(b, b);
    }
    return w;
}

struct BrxHashShape { uint64_t rows; uint32_t nu, n; }; // rows >= 1 in all; units of the last row; bytes of the last unit
BRX_TAKE_HD BrxHashShape brx_hash_shape(uint64_t L) {
    const uint64_t units = (L + BRX_HASH_UNIT - 1u) / BRX_HASH_UNIT;
    BrxHashShape s;
    s.rows = (units + 63u) / 64u;
    s.nu = (uint32_t)(units - (s.rows - 1u) * 64u);
    s.n = (uint32_t)(L - (units - 1u) * BRX_HASH_UNIT);
    return s;
}

// lane's term of a whole row: unit_l W_l
template <class M>
BRX_TAKE_HD uint64_t brx_hash_row_term(M &mem, const uint8_t *arena, uint64_t span, uint64_t src, uint64_t row, uint32_t lane, uint64_t w,
                                       const BrxHashKeys &k) {
    (void)span;
    return brx_hash_mul(brx_hash_unit(mem.ld128(arena + src + (row * 64u + lane) * BRX_HASH_UNIT), k), w);
}

// lane's term of BRX_HASH_GROUP whole rows from `row` on: the loads first, then Horner over the lane's units with the row stride
template <class M>
BRX_TAKE_HD uint64_t brx_hash_group_term(M &mem, const uint8_t *arena, uint64_t src, uint64_t row, uint32_t lane, uint64_t w,
                                         const BrxHashKeys &k) {
    const uint8_t *p = arena + src + (row * 64u + lane) * BRX_HASH_UNIT;
    BrxTake128 v[BRX_HASH_GROUP];
#if defined(__clang__)
#pragma unroll
#endif
    for (uint32_t g = 0; g < BRX_HASH_GROUP; g++) v[g] = mem.ld128(p + g * (64u * BRX_HASH_UNIT));
    uint64_t x = brx_hash_unit(v[0], k);
#if defined(__clang__)
#pragma unroll
#endif
    for (uint32_t g = 1; g < BRX_HASH_GROUP; g++) x = brx_hash_red(brx_hash_mul(x, k.k256) + brx_hash_unit(v[g], k));
    return brx_hash_mul(x, w);
}

// K^(256 GROUP), the stride of a group
BRX_TAKE_HD uint64_t brx_hash_group_stride(const BrxHashKeys &k) {
    uint64_t x = k.k256;
    for (uint32_t g = 1; g < BRX_HASH_GROUP; g++) x = brx_hash_mul(x, k.k256);
    return x;
}

// the lane whose weight `lane` needs in the last row
BRX_TAKE_HD uint32_t brx_hash_last_weight_lane(uint32_t lane, uint32_t nu) { return (lane + 1u < nu ? lane + 65u - nu : 64u - nu) & 63u; }

// lane's unit of the last row (0 where it has none) and its term of X, w being the weight of lane brx_hash_last_weight_lane(lane, nu)
template <class M>
BRX_TAKE_HD uint64_t brx_hash_last_term(M &mem, const uint8_t *arena, uint64_t span, uint64_t src, BrxHashShape s, uint32_t lane, uint64_t w,
                                        uint64_t acc, const BrxHashKeys &k, BrxTake128 &v) {
    v.lo = v.hi = 0;
    if (lane >= s.nu) return 0;
    const uint8_t *p = arena + src + ((s.rows - 1u) * 64u + lane) * BRX_HASH_UNIT;
    if (lane + 1u == s.nu) {
        v = brx_hash_fetch(mem, p, s.n, arena, span);
        return brx_hash_mul(acc, w);
    }
    v = mem.ld128(p);
    return brx_hash_mul(brx_hash_unit(v, k), w);
}

// the sum of two row terms, kept below 2^61 + 4 (so that 64 of them can be summed pairwise without overflow)
BRX_TAKE_HD uint64_t brx_hash_add(uint64_t x, uint64_t y) {
    x += y;
    return (x & BRX_HASH_P) + (x >> 61);
}

// host side (brx_api.cpp)
void brx_launch_hash(const BrxTakeArgs &a, const BrxHashKeys &k, uint64_t *hash, uint64_t *rec_len, void *hip_stream);
#endif
