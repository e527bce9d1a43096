// brx_index.h -- shared by brx_index.hip (kernels) and brx_api.cpp (brx_index_batch): the pass's part of one launch's scratch region;
// and, for the kernels of brx_index.hip, brx_index_quoted.hip, brx_index_escaped.hip and brx_find.hip, how a row is loaded and matched.
#pragma once
#include <stdint.h>

#include "brx_tiles.h"

// Scratch region of one launch: the header of the tile pass (brx_tiles.h), then max_tiles words of 64 bits: delimiters per tile (count
// pass), then their exclusive prefix sum (scan).
// A stream of l > 0 bytes has at most l / tile + 2 tiles (its first row starts up to 1023 bytes in front of it), one of 0 bytes has
// none; slots do not overlap and lie within `span`, so this bounds the tiles of a batch without a length read back.
static inline uint64_t brx_ix_max_tiles(uint32_t n, uint64_t span) { return span / BRX_TP_TILE + 2u * (uint64_t)n; }
static inline size_t brx_ix_region_bytes(size_t cap_n, size_t cap_tiles) { return brx_tp_region_bytes(cap_n, cap_tiles * 8u); }

// brx_index.hip: plan and count on `hip_stream`, and scan and fill behind them if `pos`
void brx_launch_index(const void *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span, uint8_t delim,
                      void *scratch, uint64_t max_tiles, uint64_t *count, const uint64_t *pos_off, uint64_t *pos, uint64_t total,
                      unsigned workgroups, void *hip_stream);

#ifdef __HIPCC__
// brx_index.hip, one workgroup of 1024: tile_cnt[0 .. tiles of the batch) -> its exclusive prefix sum, in place (also launched by brx_find.hip)
__global__ void brx_index_scan_kernel(uint32_t n, const uint64_t *__restrict__ pre, uint64_t max_tiles, uint64_t *__restrict__ tile_cnt);

// ---- what a row is matched with, shared by brx_index.hip, brx_index_quoted.hip, brx_index_escaped.hip and brx_find.hip ----
// 0x80 in every byte of w that equals the delimiter (d4 = the delimiter in all four bytes).  x = w ^ d4 has a zero byte there; the sum
// of a byte's low seven bits and 0x7F carries into bit 7 exactly when they are not all zero and never into the next byte, so the test
// is exact for every byte value, 0x00, 0x80 and 0xFF included.
__device__ __forceinline__ uint32_t ix_eq(uint32_t w, uint32_t d4) {
    const uint32_t x = w ^ d4;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}

// bits 7, 15, 23, 31 of m -> bits 0 .. 3
__device__ __forceinline__ uint32_t ix_nib(uint32_t m) {
    uint32_t t = m >> 7; // bits 0, 8, 16, 24
    t |= t >> 7;         // bit 8 -> 1, bit 24 -> 17
    t |= t >> 14;        // bit 16 -> 2, bit 17 -> 3
    return t & 15u;
}

// bit k: byte k of the chunk equals the byte b4 holds four times
__device__ __forceinline__ uint32_t ix_mask(uint4 v, uint32_t b4) {
    return ix_nib(ix_eq(v.x, b4)) | (ix_nib(ix_eq(v.y, b4)) << 4) | (ix_nib(ix_eq(v.z, b4)) << 8) | (ix_nib(ix_eq(v.w, b4)) << 12);
}

// The first byte value that is none of these, four times: none of the nd (0 .. 8) bytes of `set` (byte k for k < nd), not `quote` if
// `quotes`, not `escape` if `escapes`.  It is what ix_chunk puts where the stream is not: in front of a stream it ends any run and
// toggles nothing, so the stream starts unescaped and outside quotes; behind it it changes no count.  At most 10 values are excluded,
// so the walk ends at 10 or before.
__device__ __forceinline__ uint32_t ix_filler(uint64_t set, uint32_t nd, uint32_t quote, uint32_t quotes, uint32_t escape,
                                              uint32_t escapes) {
    uint32_t f = 0u;
    for (;;) {
        bool hit = (quotes && f == quote) || (escapes && f == escape);
        for (uint32_t k = 0; k < nd; k++) hit = hit || f == ((uint32_t)(set >> (8u * k)) & 0xFFu);
        if (!hit) break;
        f++;
    }
    return f * 0x01010101u;
}

// the low k bytes of a 64-bit word (k >= 8: all of it)
__device__ __forceinline__ uint64_t ix_low_bytes(uint32_t k) { return k >= 8u ? ~0ull : (1ull << (8u * k)) - 1ull; }

// The chunk of `lane` in the row at `row`, with every byte outside the stream [a, e) replaced by one that the pass reports nowhere
// (nd4 in all four bytes: brx_index.hip passes ~delimiter, the others ix_filler or, brx_find.hip, a byte that is not in the needle).
// Only aligned 16-byte chunks that hold a byte of the stream are loaded; of the (at most two) chunks that reach over an end of the
// arena [arena0, arena1) only the stream's own bytes are, one by one.
__device__ __forceinline__ uint4 ix_chunk(const uint8_t *out, uint64_t row, uint32_t lane, uint64_t a, uint64_t e, uint64_t arena0,
                                          uint64_t arena1, uint32_t nd4) {
    const uint64_t c = row + 16u * lane;
    const uint8_t *pc = out + (int64_t)(c - arena0); // (from the kernel's argument: a global load, not a flat one)
    if (row >= a && row + BRX_TP_ROW <= e) return *(const uint4 *)pc; // (uniform) a row inside the stream
    uint4 v = make_uint4(nd4, nd4, nd4, nd4);
    if (c < e && c + 16u > a) {
        const uint32_t lo = a > c ? (uint32_t)(a - c) : 0u, hi = e < c + 16u ? (uint32_t)(e - c) : 16u; // bytes [lo, hi) are the stream's
        uint64_t p = 0, q = 0;
        if (c >= arena0 && c + 16u <= arena1) {
            const uint4 w = *(const uint4 *)pc;
            if (lo == 0u && hi == 16u) return w;
            p = (uint64_t)w.x | ((uint64_t)w.y << 32);
            q = (uint64_t)w.z | ((uint64_t)w.w << 32);
        } else {
            for (uint32_t k = lo; k < hi; k++) {
                const uint64_t b = pc[k];
                if (k < 8u) p |= b << (8u * k); else q |= b << (8u * (k - 8u));
            }
        }
        const uint64_t kp = ix_low_bytes(hi) & ~ix_low_bytes(lo);
        const uint64_t kq = ix_low_bytes(hi > 8u ? hi - 8u : 0u) & ~ix_low_bytes(lo > 8u ? lo - 8u : 0u);
        const uint64_t nd8 = (uint64_t)nd4 | ((uint64_t)nd4 << 32);
        p = (p & kp) | (nd8 & ~kp);
        q = (q & kq) | (nd8 & ~kq);
        v = make_uint4((uint32_t)p, (uint32_t)(p >> 32), (uint32_t)q, (uint32_t)(q >> 32));
    }
    return v;
}
#endif
