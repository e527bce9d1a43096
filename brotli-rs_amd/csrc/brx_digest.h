// brx_digest.h -- shared by brx_digest.hip (kernels) and brx_api.cpp (brx_digest_batch): layout of the per-kind table block and the
// host code that fills it.  Nothing here is a committed constant: every word follows from the generator polynomial at run time.
//
// Algebra (reflected CRCs, both kinds).  A CRC register is a polynomial over GF(2) modulo P, bit 31 = x^0, bit 0 = x^31.  With a zero
// initial value and no final xor ("raw") the CRC is linear in the message, and
//     raw(A || B) = raw(A) * x^(8 |B|)  ^  raw(B)          (appending |B| bytes = shifting by 8 |B| bits = one multiplication mod P)
//     raw(0 .. 0 || A) = raw(A)                            (leading zero bytes change nothing)
// The standard CRC of M (init and xorout 0xFFFFFFFF) is  raw(M) ^ 0xFFFFFFFF * x^(8 |M|) ^ 0xFFFFFFFF.
#pragma once
#include <stdint.h>

#include "brx_tiles.h"

// Table block of one kind, in 32-bit words:
#define BRX_DG_SLICE 0u             // 16 x 256: SLICE[j][b] = raw CRC of byte b followed by 15 - j zero bytes (byte j of a 16-byte chunk)
#define BRX_DG_ROWSHIFT 4096u       // 4 x 256:  ROWSHIFT[j][b] = (b << 8 j) * x^(8 * 1024): a register moved on by one row, bytewise
#define BRX_DG_LDS_WORDS 5120u      // ... the two above live in LDS (20 KiB per workgroup)
#define BRX_DG_SMALLPOW 5120u       // 2048:     x^(8 d), d < 2048: a lane's distance to the end of its tile
#define BRX_DG_POW 7168u            // 32:       x^(8 * 2^k): the squares for square-and-multiply over the bits of a byte count
#define BRX_DG_WORDS 7200u

// Scratch region of one launch: the header of the tile pass (brx_tiles.h), then one accumulator word per stream.
static inline size_t brx_dg_region_bytes(size_t cap_n) { return brx_tp_region_bytes(cap_n, cap_n * 4u); }

// brx_digest.hip: plan, tiles and fold on `hip_stream`
void brx_launch_digest(const void *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, const uint32_t *tab, uint32_t poly,
                       void *scratch, uint32_t *digest, const uint32_t *expect, uint32_t *mismatch, unsigned workgroups, void *hip_stream);

// ---- host side: the table block from the polynomial ----
// a * b mod P (bit 31 = x^0)
static inline uint32_t brx_dg_mul(uint32_t a, uint32_t b, uint32_t poly) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? poly : 0u);
    }
    return p;
}

static inline void brx_dg_build_tables(uint32_t poly, uint32_t *t) {
    // the byte table of the bitwise definition: register b, eight zero bits shifted in
    uint32_t byte_tab[256];
    for (uint32_t b = 0; b < 256; b++) {
        uint32_t r = b;
        for (int k = 0; k < 8; k++) r = (r >> 1) ^ ((r & 1u) ? poly : 0u);
        byte_tab[b] = r;
    }
    // SLICE[15][b] = raw CRC of the single byte b; one more zero byte behind it per table towards j = 0
    for (uint32_t b = 0; b < 256; b++) t[BRX_DG_SLICE + 15u * 256u + b] = byte_tab[b];
    for (int j = 14; j >= 0; j--)
        for (uint32_t b = 0; b < 256; b++) {
            const uint32_t r = t[BRX_DG_SLICE + (uint32_t)(j + 1) * 256u + b];
            t[BRX_DG_SLICE + (uint32_t)j * 256u + b] = (r >> 8) ^ byte_tab[r & 255u];
        }
    // x^8, then its squares
    uint32_t sq = 0x00800000u; // x^8
    for (uint32_t k = 0; k < 32; k++) {
        t[BRX_DG_POW + k] = sq;
        sq = brx_dg_mul(sq, sq, poly);
    }
    uint32_t p = 0x80000000u; // x^0
    for (uint32_t d = 0; d < 2048; d++) {
        t[BRX_DG_SMALLPOW + d] = p;
        p = brx_dg_mul(p, t[BRX_DG_POW], poly);
    }
    const uint32_t row = t[BRX_DG_POW + 10]; // x^(8 * 1024)
    for (uint32_t j = 0; j < 4; j++)
        for (uint32_t b = 0; b < 256; b++) t[BRX_DG_ROWSHIFT + j * 256u + b] = brx_dg_mul(b << (8u * j), row, poly);
}
