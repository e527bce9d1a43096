// brx_index.hip -- brx_index_batch: where the records of every decoded stream of a batch end, on the device (layout: brx_index.h).
//
// Count mode is two launches on the caller's stream, fill mode four, in the shape of the tile pass (brx_tiles.h: tiling, plan, the
// wave's walk over the items, item search, wave sum, slices of the one-workgroup kernel, row emit):
//   plan   brx_tiles.hip, with `count` cleared.
//   count  a pass over the bytes: the wave compares the four dwords of its chunk with the delimiter by packed arithmetic, and adds the
//          population count to a per-lane sum.  At the tile's end the lanes add up; the tile's count goes to the tile's scratch word
//          (fill mode) and, by one atomic add, to count[i] (addition commutes: tiles finish in any order and nobody waits for anybody).
//   scan   one workgroup: the tile counts -> their exclusive prefix sum G over ALL tiles of the batch, in place.  Tile t of stream i
//          starts at delimiter G[t] - G[first tile of i] of its stream.
//   fill   the same grid over the same items.  Per row: every lane's matches as a 16-bit mask (ix_mask), and tp_emit_row: a wave prefix
//          sum of their population counts, the row's total added to a running base kept in a scalar, and the positions stored.
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
    const uint32_t d4 = delim * 0x01010101u, nd4 = ~d4;
    const uint64_t arena0 = (uint64_t)(uintptr_t)out, arena1 = arena0 + span;
    for (TpWalk w = tp_walk(tp_total(pre, n, max_tiles)); w.item < w.total; tp_advance(w, ticket)) {
        const TpItem it = tp_item(w.item, out, out_off, len, n, pre);
        uint32_t acc = 0;
        for (uint32_t r = 0; r < it.rows; r++) {
            const uint4 v = ix_chunk(out, it.t0 + (uint64_t)r * BRX_TP_ROW, w.lane, it.a, it.e, arena0, arena1, nd4);
            acc += __popc(ix_eq(v.x, d4)) + __popc(ix_eq(v.y, d4)) + __popc(ix_eq(v.z, d4)) + __popc(ix_eq(v.w, d4));
        }
        acc = tp_wave_sum(acc);
        if (w.lane == 0u) {
            if (tile_cnt) tile_cnt[w.item] = acc;
            if (count && acc) atomicAdd((unsigned long long *)&count[it.si], (unsigned long long)acc);
        }
    }
}

__global__ __launch_bounds__(1024) void brx_index_scan_kernel(uint32_t n, const uint64_t *__restrict__ pre, uint64_t max_tiles,
                                                              uint64_t *__restrict__ tile_cnt) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const TpSlice sl = tp_slice_1024(tp_total(pre, n, max_tiles), t);
    uint64_t sum = 0;
    for (uint64_t i = sl.i0; i < sl.i1; i++) sum += tile_cnt[i];
    uint64_t run = tp_block_scan_1024(part, t, sum) - sum;
    for (uint64_t i = sl.i0; i < sl.i1; i++) {
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
    const uint32_t d4 = delim * 0x01010101u, nd4 = ~d4;
    const uint64_t arena0 = (uint64_t)(uintptr_t)out, arena1 = arena0 + span;
    for (TpWalk w = tp_walk(tp_total(pre, n, max_tiles)); w.item < w.total; tp_advance(w, ticket)) {
        const TpItem it = tp_item(w.item, out, out_off, len, n, pre);
        // index in pos of the tile's first delimiter: the stream's first entry + the delimiters of the stream's tiles in front of this one
        uint64_t base = tp_uniform(pos_off[it.si] + (tile_base[w.item] - tile_base[pre[it.si]]));
        for (uint32_t r = 0; r < it.rows; r++) {
            const uint64_t row = it.t0 + (uint64_t)r * BRX_TP_ROW;
            const uint4 v = ix_chunk(out, row, w.lane, it.a, it.e, arena0, arena1, nd4);
            const uint64_t rel = row + 16u * w.lane - it.a; // offset of the chunk's byte 0 in the stream (no bit is set where that is in front of it)
            // bit k of the mask: byte k of the chunk is a delimiter of the stream
            tp_emit_row(ix_mask(v, d4), w.lane, base, pos_total, [&](uint64_t idx, uint32_t k) { pos[idx] = rel + k; });
        }
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
