// brx_digest.hip -- brx_digest_batch: CRC-32 / CRC-32C of every decoded stream of a batch, on the device (algebra: brx_digest.h).
//
// Three launches on the caller's stream:
//   plan   one workgroup: tiles per stream (a tile = 64 KiB of the stream's 1 KiB aligned address range), their exclusive prefix sum,
//          the per-stream accumulators and the ticket counter cleared.  The host never learns a length.
//   tiles  persistent grid, 4 workgroups of 8 waves per CU.  A work item is one (stream, tile) pair: a wave's first item is its index
//          in the grid, the following ones come from the ticket counter.  The wave walks its tile in aligned 1 KiB rows, 16 B per lane
//          (the rows flush_range wrote), every lane keeping the raw CRC of ITS column: 16 LDS lookups for the chunk, 4 to move the
//          register on by one row.  Head and tail are masked; the chunk that holds the stream's last byte is moved up so that its
//          zeros lead, and counts on its own.  At the end of the tile a lane multiplies its register by x^(8 * its distance to the tile's end) (a table of 2048
//          fixed distances), the lanes xor together, the tile's partial is multiplied by x^(8 * bytes behind the tile) -- the squares
//          x^(8 * 2^k) picked by the bits of that count, multiplied together by a butterfly over the lanes -- and xor-ed into the
//          stream's accumulator (an atomic: xor commutes, so tiles finish in any order and nobody waits for anybody).
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

__global__ __launch_bounds__(1024) void brx_digest_plan_kernel(const uint8_t *out, const uint64_t *__restrict__ out_off,
                                                               const uint64_t *__restrict__ len, uint32_t n, uint64_t *__restrict__ pre,
                                                               uint32_t *__restrict__ acc, unsigned long long *ticket) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint64_t per = ((uint64_t)n + 1023u) / 1024u;
    const uint64_t i0 = per * t < n ? per * t : n, i1 = i0 + per < n ? i0 + per : n;
    uint64_t sum = 0;
    for (uint64_t i = i0; i < i1; i++) {
        const uint64_t l = len[i];
        const uint64_t a = (uint64_t)(uintptr_t)out + out_off[i];
        sum += l ? ((a & (BRX_DG_ROW - 1u)) + l + BRX_DG_TILE - 1u) / BRX_DG_TILE : 0u;
    }
    part[t] = sum;
    __syncthreads();
    for (uint32_t s = 1; s < 1024u; s <<= 1) { // inclusive scan of the 1024 partial sums
        const uint64_t v = t >= s ? part[t - s] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t run = part[t] - sum;
    for (uint64_t i = i0; i < i1; i++) {
        const uint64_t l = len[i];
        const uint64_t a = (uint64_t)(uintptr_t)out + out_off[i];
        pre[i] = run;
        acc[i] = 0u;
        run += l ? ((a & (BRX_DG_ROW - 1u)) + l + BRX_DG_TILE - 1u) / BRX_DG_TILE : 0u;
    }
    if (t == 1023u) {
        pre[n] = part[1023];
        *ticket = 0ull;
    }
}

// a value that is the same in every lane of the wave, said so to the compiler: what depends on it is loaded by the scalar unit
__device__ __forceinline__ uint64_t dg_uniform(uint64_t v) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32);
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

__global__ __launch_bounds__(BRX_DG_WG, 8) void brx_digest_tiles_kernel(const uint8_t *out, const uint64_t *__restrict__ out_off,
                                                                        const uint64_t *__restrict__ len, uint32_t n,
                                                                        const uint32_t *__restrict__ tab, uint32_t poly,
                                                                        const uint64_t *__restrict__ pre, uint32_t *acc,
                                                                        unsigned long long *ticket) {
    __shared__ uint32_t lds[BRX_DG_LDS_WORDS];
    const uint64_t total = pre[n];
    const uint32_t waves_per_wg = BRX_DG_WG / 64u;
    if ((uint64_t)blockIdx.x * waves_per_wg >= total) return; // (the whole workgroup: nothing for any of its waves, not even a first item)
    for (uint32_t i = threadIdx.x; i < BRX_DG_LDS_WORDS; i += BRX_DG_WG) lds[i] = tab[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t grid_waves = (uint64_t)gridDim.x * waves_per_wg;
    uint64_t item = dg_uniform((uint64_t)blockIdx.x * waves_per_wg + (threadIdx.x >> 6));
    while (item < total) {
        // the stream of this item: the last i < n with pre[i] <= item (streams without tiles share their successor's value and lose)
        uint32_t lo_i = 0, hi_i = n;
        while (hi_i - lo_i > 1u) {
            const uint32_t mid = lo_i + (hi_i - lo_i) / 2u;
            if (pre[mid] <= item) lo_i = mid; else hi_i = mid;
        }
        const uint32_t si = lo_i;
        const uint64_t a = (uint64_t)(uintptr_t)out + out_off[si]; // first byte of the stream
        const uint64_t e = a + len[si];                            // one past its last
        const uint64_t t0 = (a & ~(uint64_t)(BRX_DG_ROW - 1u)) + (item - pre[si]) * BRX_DG_TILE;
        const uint64_t t1 = t0 + BRX_DG_TILE < e ? t0 + BRX_DG_TILE : e; // reference point of the tile: its end, or the stream's
        const uint32_t rows = (uint32_t)((t1 - t0 + BRX_DG_ROW - 1u) / BRX_DG_ROW);
        uint32_t s = 0, tail = 0;
        for (uint32_t r = 0; r < rows; r++) {
            const uint64_t row = t0 + (uint64_t)r * BRX_DG_ROW;
            const uint64_t c = row + 16u * lane;
            if (row >= a && row + BRX_DG_ROW <= e) { // (uniform) a row inside the stream
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
        const uint64_t cl = t0 + (uint64_t)(rows - 1u) * BRX_DG_ROW + 16u * lane;
        const uint64_t at = cl + 16u > e ? cl + 16u - BRX_DG_ROW : cl + 16u;
        uint32_t part = dg_mul(s, tab[BRX_DG_SMALLPOW + ((uint32_t)(t1 - at) & 2047u)], poly) ^ tail;
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) part ^= (uint32_t)__shfl_xor((int)part, k);
        const uint64_t behind = e - t1; // bytes of the stream behind this tile (< 2^32: the per-stream limit)
        if (behind) part = dg_mul(part, dg_pow_bytes((uint32_t)behind, tab, poly), poly);
        if (lane == 0u && part) atomicXor(&acc[si], part);
        // next item
        unsigned long long next = 0;
        if (lane == 0u) {
            next = __hip_atomic_load(ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (a load first: most waves end here, cheaply)
            if (grid_waves + next < total) next = atomicAdd(ticket, 1ull);
        }
        next = (unsigned long long)__shfl((long long)next, 0);
        item = dg_uniform(grid_waves + next);
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
    // scratch of one launch: the ticket counter on a line of its own, n + 1 prefix sums, n accumulators
    unsigned long long *ticket = (unsigned long long *)scratch;
    uint64_t *pre = (uint64_t *)((uint8_t *)scratch + 128);
    uint32_t *acc = (uint32_t *)(pre + (size_t)n + 1u);
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(brx_digest_plan_kernel, dim3(1), dim3(1024), 0, st, (const uint8_t *)out, out_off, len, n, pre, acc, ticket);
    hipLaunchKernelGGL(brx_digest_tiles_kernel, dim3(workgroups), dim3(BRX_DG_WG), 0, st, (const uint8_t *)out, out_off, len, n, tab, poly,
                       pre, acc, ticket);
    const uint64_t fold_wgs = ((uint64_t)n * 32u + 255u) / 256u;
    hipLaunchKernelGGL(brx_digest_fold_kernel, dim3((unsigned)fold_wgs), dim3(256), 0, st, len, n, tab, poly, acc, digest, expect, mismatch);
}
