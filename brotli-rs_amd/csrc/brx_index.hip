// brx_index.hip -- brx_index_batch: where the records of every decoded stream of a batch end, on the device (layout: brx_index.h).
//
// Count mode is two launches on the caller's stream, fill mode four, in the shape of the tile pass (brx_tiles.h: tiling, plan, ticket
// counters, item search):
//   plan   brx_tiles.hip, with `count` cleared.
//   count  a pass over the bytes: the wave compares the four dwords of its chunk with the delimiter by packed arithmetic, and adds the
//          population count to a per-lane sum.  At the tile's end the lanes add up; the tile's count goes to the tile's scratch word
//          (fill mode) and, by one atomic add, to count[i] (addition commutes: tiles finish in any order and nobody waits for anybody).
//   scan   one workgroup: the tile counts -> their exclusive prefix sum G over ALL tiles of the batch, in place.  Tile t of stream i
//          starts at delimiter G[t] - G[first tile of i] of its stream.
//   fill   the same grid over the same items.  Per row: every lane's matches as a 16-bit mask, a wave prefix sum of their population
//          counts (__shfl_up, no LDS memory), the row's total added to a running base kept in a scalar, and the positions stored.
// Ordering between tiles comes from the kernel boundaries alone: no wave ever waits for a value that another wave of the same launch
// produces (no chained scan, no look-back), so there is nothing that could spin.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "brx_index.h"

__global__ __launch_bounds__(BRX_TP_WG, 8) void brx_index_count_kernel(const uint8_t *out, const uint64_t *__restrict__ out_off,
                                                                       const uint64_t *__restrict__ len, uint32_t n, uint64_t span,
                                                                       uint32_t delim, const uint64_t *__restrict__ pre,
                                                                       uint64_t max_tiles, uint64_t *__restrict__ tile_cnt,
                                                                       uint64_t *count, unsigned long long *ticket) {
    const uint64_t total = pre[n] < max_tiles ? pre[n] : max_tiles; // (more tiles than `span` allows: a caller's error, nothing is written for them)
    const uint32_t waves_per_wg = BRX_TP_WG / 64u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t grid_waves = (uint64_t)gridDim.x * waves_per_wg;
    const uint32_t d4 = delim * 0x01010101u, nd4 = ~d4;
    const uint64_t arena0 = (uint64_t)(uintptr_t)out, arena1 = arena0 + span;
    uint64_t item = tp_uniform((uint64_t)blockIdx.x * waves_per_wg + (threadIdx.x >> 6));
    while (item < total) {
        const TpItem it = tp_item(item, out, out_off, len, n, pre);
        uint32_t acc = 0;
        for (uint32_t r = 0; r < it.rows; r++) {
            const uint4 v = ix_chunk(out, it.t0 + (uint64_t)r * BRX_TP_ROW, lane, it.a, it.e, arena0, arena1, nd4);
            acc += __popc(ix_eq(v.x, d4)) + __popc(ix_eq(v.y, d4)) + __popc(ix_eq(v.z, d4)) + __popc(ix_eq(v.w, d4));
        }
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) acc += (uint32_t)__shfl_xor((int)acc, k);
        if (lane == 0u) {
            if (tile_cnt) tile_cnt[item] = acc;
            if (count && acc) atomicAdd((unsigned long long *)&count[it.si], (unsigned long long)acc);
        }
        item = tp_next(ticket, grid_waves, total, lane);
    }
}

__global__ __launch_bounds__(1024) void brx_index_scan_kernel(uint32_t n, const uint64_t *__restrict__ pre, uint64_t max_tiles,
                                                              uint64_t *__restrict__ tile_cnt) {
    __shared__ uint64_t part[1024];
    const uint64_t total = pre[n] < max_tiles ? pre[n] : max_tiles;
    const uint32_t t = threadIdx.x;
    const uint64_t per = (total + 1023u) / 1024u;
    const uint64_t i0 = per * t < total ? per * t : total, i1 = i0 + per < total ? i0 + per : total;
    uint64_t sum = 0;
    for (uint64_t i = i0; i < i1; i++) sum += tile_cnt[i];
    uint64_t run = tp_block_scan_1024(part, t, sum) - sum;
    for (uint64_t i = i0; i < i1; i++) {
        const uint64_t c = tile_cnt[i];
        tile_cnt[i] = run;
        run += c;
    }
}

__global__ __launch_bounds__(BRX_TP_WG, 8) void brx_index_fill_kernel(const uint8_t *out, const uint64_t *__restrict__ out_off,
                                                                      const uint64_t *__restrict__ len, uint32_t n, uint64_t span,
                                                                      uint32_t delim, const uint64_t *__restrict__ pre,
                                                                      uint64_t max_tiles, const uint64_t *__restrict__ tile_base,
                                                                      const uint64_t *__restrict__ pos_off, uint64_t *__restrict__ pos,
                                                                      uint64_t pos_total, unsigned long long *ticket) {
    const uint64_t total = pre[n] < max_tiles ? pre[n] : max_tiles;
    const uint32_t waves_per_wg = BRX_TP_WG / 64u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t grid_waves = (uint64_t)gridDim.x * waves_per_wg;
    const uint32_t d4 = delim * 0x01010101u, nd4 = ~d4;
    const uint64_t arena0 = (uint64_t)(uintptr_t)out, arena1 = arena0 + span;
    uint64_t item = tp_uniform((uint64_t)blockIdx.x * waves_per_wg + (threadIdx.x >> 6));
    while (item < total) {
        const TpItem it = tp_item(item, out, out_off, len, n, pre);
        // index in pos of the tile's first delimiter: the stream's first entry + the delimiters of the stream's tiles in front of this one
        uint64_t base = tp_uniform(pos_off[it.si] + (tile_base[item] - tile_base[pre[it.si]]));
        for (uint32_t r = 0; r < it.rows; r++) {
            const uint64_t row = it.t0 + (uint64_t)r * BRX_TP_ROW;
            const uint4 v = ix_chunk(out, row, lane, it.a, it.e, arena0, arena1, nd4);
            uint32_t m = ix_nib(ix_eq(v.x, d4)) | (ix_nib(ix_eq(v.y, d4)) << 4) | (ix_nib(ix_eq(v.z, d4)) << 8) |
                         (ix_nib(ix_eq(v.w, d4)) << 12); // bit k: byte k of the chunk is a delimiter of the stream
            if (__ballot(m != 0u) == 0ull) continue; // (uniform) a row without one
            const uint32_t c = (uint32_t)__popc(m);
            uint32_t incl = c;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, s);
                if (lane >= (uint32_t)s) incl += up;
            }
            uint64_t idx = base + (incl - c);
            const uint64_t rel = row + 16u * lane - it.a; // offset of the chunk's byte 0 in the stream (m == 0 where that is in front of it)
            while (m) {
                const uint32_t k = (uint32_t)__ffs((int)m) - 1u;
                m &= m - 1u;
                if (idx < pos_total) pos[idx] = rel + k;
                idx++;
            }
            base += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
        item = tp_next(ticket, grid_waves, total, lane);
    }
}

void brx_launch_index(const void *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span, uint8_t delim,
                      void *scratch, uint64_t max_tiles, uint64_t *count, const uint64_t *pos_off, uint64_t *pos, uint64_t total,
                      unsigned workgroups, void *hip_stream) {
    uint64_t *pre = brx_tp_pre(scratch), *tiles = (uint64_t *)brx_tp_own(scratch, n);
    hipStream_t st = (hipStream_t)hip_stream;
    brx_launch_tile_plan(out, out_off, len, n, scratch, (uint32_t *)count, count ? 2u : 0u, st);
    hipLaunchKernelGGL(brx_index_count_kernel, dim3(workgroups), dim3(BRX_TP_WG), 0, st, (const uint8_t *)out, out_off, len, n, span,
                       (uint32_t)delim, pre, max_tiles, pos ? tiles : nullptr, count, brx_tp_ticket_a(scratch));
    if (!pos) return;
    hipLaunchKernelGGL(brx_index_scan_kernel, dim3(1), dim3(1024), 0, st, n, pre, max_tiles, tiles);
    hipLaunchKernelGGL(brx_index_fill_kernel, dim3(workgroups), dim3(BRX_TP_WG), 0, st, (const uint8_t *)out, out_off, len, n, span,
                       (uint32_t)delim, pre, max_tiles, tiles, pos_off, pos, total, brx_tp_ticket_b(scratch));
}
