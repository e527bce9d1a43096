// brx_digest.hip -- brx_digest_batch: CRC-32 / CRC-32C of every decoded stream of a batch, on the device (algebra: brx_digest.h).
//
// Three launches on the caller's stream, in the shape of the tile pass (brx_tiles.h: tiling, plan, the wave's walk over the items,
// item search):
//   plan   brx_tiles.hip, with one accumulator word per stream cleared.
//   tiles  the pass over the bytes.  Every lane keeps the raw CRC of ITS column of the rows (the rows flush_range wrote): 16 LDS lookups
//          for the chunk, 4 to move the register on by one row.  Head and tail are masked; the chunk that holds the stream's last byte is
//          moved up so that its zeros lead, and counts on its own.  At the end of the tile a lane multiplies its register by
//          x^(8 * its distance to the tile's end) (a table of 2048 fixed distances), the lanes xor together, the tile's partial is
//          multiplied by x^(8 * bytes behind the tile) -- the squares x^(8 * 2^k) picked by the bits of that count, multiplied together
//          by a butterfly over the lanes -- and xor-ed into the stream's accumulator (an atomic: xor commutes, so tiles finish in any
//          order and nobody waits for anybody).
//   fold   half a wave per stream: init / xorout conditioning (0xFFFFFFFF * x^(8 len) ^ 0xFFFFFFFF, the same butterfly over the bits of
//          len), the digest, and the comparison with `expect`.  It runs behind the tiles kernel in stream order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "brx_digest.h"

#define DG_ONE 0x80000000u // x^0

// a * b mod P (bit 31 = x^0): 32 steps of shift-and-add
__device__ __forceinline__ uint32_t dg_mul(uint32_t a, uint32_t b, uint32_t poly) {
    uint32_t p = 0;
#pragma unroll
    for (int i = 31; i >= 0; i--) {
        p ^= (0u - ((a >> i) & 1u)) & b;
        b = (b >> 1) ^ ((0u - (b & 1u)) & poly);
    }
    return p;
}

// x^(8 * count) in every lane: lane k (mod 32) takes the k-th square if bit k of `count` is set, a butterfly multiplies them together
__device__ __forceinline__ uint32_t dg_pow_bytes(uint32_t count, const uint32_t *__restrict__ tab, uint32_t poly) {
    const uint32_t k = threadIdx.x & 31u;
    uint32_t f = ((count >> k) & 1u) ? tab[BRX_DG_POW + k] : DG_ONE;
#pragma unroll
    for (int s = 16; s >= 1; s >>= 1) f = dg_mul(f, (uint32_t)__shfl_xor((int)f, s), poly);
    return f;
}

// the 16 bytes of a chunk and the register of the rows before it -> the register behind this row
__device__ __forceinline__ uint32_t dg_step(uint32_t s, uint4 v, const uint32_t *lds) {
    const uint32_t *sl = lds + BRX_DG_SLICE, *rs = lds + BRX_DG_ROWSHIFT;
    uint32_t r = rs[s & 255u] ^ rs[256u + ((s >> 8) & 255u)] ^ rs[512u + ((s >> 16) & 255u)] ^ rs[768u + (s >> 24)];
    r ^= sl[0 * 256 + (v.x & 255u)] ^ sl[1 * 256 + ((v.x >> 8) & 255u)] ^ sl[2 * 256 + ((v.x >> 16) & 255u)] ^ sl[3 * 256 + (v.x >> 24)];
    r ^= sl[4 * 256 + (v.y & 255u)] ^ sl[5 * 256 + ((v.y >> 8) & 255u)] ^ sl[6 * 256 + ((v.y >> 16) & 255u)] ^ sl[7 * 256 + (v.y >> 24)];
    r ^= sl[8 * 256 + (v.z & 255u)] ^ sl[9 * 256 + ((v.z >> 8) & 255u)] ^ sl[10 * 256 + ((v.z >> 16) & 255u)] ^ sl[11 * 256 + (v.z >> 24)];
    r ^= sl[12 * 256 + (v.w & 255u)] ^ sl[13 * 256 + ((v.w >> 8) & 255u)] ^ sl[14 * 256 + ((v.w >> 16) & 255u)] ^ sl[15 * 256 + (v.w >> 24)];
    return r;
}

// A chunk at the edge of its stream: bytes [lo, hi) of it belong to the stream (0 <= lo < hi <= 16).  The others go, and the kept ones
// move up by 16 - hi bytes: zeros lead (free), none trails, and the chunk counts as ending where the stream's byte hi - 1 is.
__device__ __forceinline__ uint4 dg_edge(uint4 v, uint32_t lo, uint32_t hi) {
    uint64_t a = (uint64_t)v.x | ((uint64_t)v.y << 32), b = (uint64_t)v.z | ((uint64_t)v.w << 32);
    uint32_t down = 8u * lo, up = 8u * (16u - hi + lo); // (down <= 120, 0 <= up <= 120 as hi - lo >= 1)
    if (down >= 64u) { a = b; b = 0; down -= 64u; }
    if (down) { a = (a >> down) | (b << (64u - down)); b >>= down; }
    if (up >= 64u) { b = a; a = 0; up -= 64u; }
    if (up) { b = (b << up) | (a >> (64u - up)); a <<= up; }
    return make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
}

__global__ __launch_bounds__(BRX_TP_WG, 8) void brx_digest_tiles_kernel(const uint8_t *out, const uint64_t *__restrict__ out_off,
                                                                        const uint64_t *__restrict__ len, uint32_t n,
                                                                        const uint32_t *__restrict__ tab, uint32_t poly,
                                                                        const uint64_t *__restrict__ pre, uint32_t *acc,
                                                                        unsigned long long *ticket) {
    __shared__ uint32_t lds[BRX_DG_LDS_WORDS];
    const uint64_t total = pre[n];
    const uint32_t waves_per_wg = BRX_TP_WG / 64u;
    if ((uint64_t)blockIdx.x * waves_per_wg >= total) return; // (the whole workgroup: nothing for any of its waves, not even a first item)
    for (uint32_t i = threadIdx.x; i < BRX_DG_LDS_WORDS; i += BRX_TP_WG) lds[i] = tab[i];
    __syncthreads();
    for (TpWalk w = tp_walk(total); w.item < w.total; tp_advance(w, ticket)) {
        const TpItem it = tp_item(w.item, out, out_off, len, n, pre);
        const uint64_t a = it.a, e = it.e, t1 = it.t1; // t1: the reference point of the tile
        uint32_t s = 0, tail = 0;
        for (uint32_t r = 0; r < it.rows; r++) {
            const uint64_t row = it.t0 + (uint64_t)r * BRX_TP_ROW;
            const uint64_t c = row + 16u * w.lane;
            if (row >= a && row + BRX_TP_ROW <= e) { // (uniform) a row inside the stream
                s = dg_step(s, *(const uint4 *)(uintptr_t)c, lds);
            } else if (c < e) { // an edge row: lanes behind the stream's end stand still, lanes in front of its start read nothing
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                bool last = false;
                if (c + 16u > a) {
                    v = *(const uint4 *)(uintptr_t)c; // (an aligned 16-byte chunk that holds a byte of the stream: same page)
                    const uint32_t lo = a > c ? (uint32_t)(a - c) : 0u, hi = e < c + 16u ? (uint32_t)(e - c) : 16u;
                    if (lo != 0u || hi != 16u) v = dg_edge(v, lo, hi);
                    last = hi != 16u;
                }
                // the chunk that ends short, at the stream's last byte, stands where the stream ends by itself (moved up, it is a
                // chunk of its own and not 1 KiB behind the lane's register): the register stands still here too
                const uint32_t r1 = dg_step(last ? 0u : s, v, lds);
                if (last) tail = r1; else s = r1;
            }
        }
        // where this lane's register stands: behind its chunk of the last row, or one row further up if that chunk reaches beyond
        // the stream's end -- and from there to the reference point (< 2048 bytes by construction)
        const uint64_t cl = it.t0 + (uint64_t)(it.rows - 1u) * BRX_TP_ROW + 16u * w.lane;
        const uint64_t at = cl + 16u > e ? cl + 16u - BRX_TP_ROW : cl + 16u;
        uint32_t part = dg_mul(s, tab[BRX_DG_SMALLPOW + ((uint32_t)(t1 - at) & 2047u)], poly) ^ tail;
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) part ^= (uint32_t)__shfl_xor((int)part, k);
        const uint64_t behind = e - t1; // bytes of the stream behind this tile (< 2^32: the per-stream limit)
        if (behind) part = dg_mul(part, dg_pow_bytes((uint32_t)behind, tab, poly), poly);
        if (w.lane == 0u && part) atomicXor(&acc[it.si], part);
    }
}

__global__ __launch_bounds__(256) void brx_digest_fold_kernel(const uint64_t *__restrict__ len, uint32_t n, const uint32_t *__restrict__ tab,
                                                              uint32_t poly, const uint32_t *__restrict__ acc, uint32_t *__restrict__ digest,
                                                              const uint32_t *__restrict__ expect, uint32_t *__restrict__ mismatch) {
    const uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 5; // 32 lanes per stream
    const bool live = i < n;
    const uint32_t l = live ? (uint32_t)len[i] : 0u;
    const uint32_t f = dg_pow_bytes(l, tab, poly); // (every lane takes part in the butterfly)
    if (live && (threadIdx.x & 31u) == 0u) {
        const uint32_t d = acc[i] ^ dg_mul(0xFFFFFFFFu, f, poly) ^ 0xFFFFFFFFu;
        digest[i] = d;
        if (mismatch) mismatch[i] = d != expect[i] ? 1u : 0u;
    }
}

void brx_launch_digest(const void *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, const uint32_t *tab, uint32_t poly,
                       void *scratch, uint32_t *digest, const uint32_t *expect, uint32_t *mismatch, unsigned workgroups, void *hip_stream) {
    // scratch of one launch: the header of the tile pass, and n accumulators
    uint32_t *acc = (uint32_t *)brx_tp_own(scratch, n);
    hipStream_t st = (hipStream_t)hip_stream;
    brx_launch_tile_plan(out, out_off, len, n, scratch, acc, 1u, st);
    hipLaunchKernelGGL(brx_digest_tiles_kernel, dim3(workgroups), dim3(BRX_TP_WG), 0, st, (const uint8_t *)out, out_off, len, n, tab, poly,
                       brx_tp_pre(scratch), acc, brx_tp_ticket_a(scratch));
    const uint64_t fold_wgs = ((uint64_t)n * 32u + 255u) / 256u;
    hipLaunchKernelGGL(brx_digest_fold_kernel, dim3((unsigned)fold_wgs), dim3(256), 0, st, len, n, tab, poly, acc, digest, expect, mismatch);
}
