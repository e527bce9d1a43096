// brx_find.hip -- brx_find_batch: where a byte sequence of 1 .. 16 bytes (the needle) occurs in every decoded stream of a batch, on the
// device (layout: brx_find.h).
//
// The pass is the tile pass (brx_tiles.h) as brx_index.hip runs it -- plan, count, and in fill mode scan (brx_index_scan_kernel itself)
// and fill -- with a row body that looks across the edges of lane chunks, rows and tiles.  An occurrence belongs to the lane chunk
// that holds its LAST byte: everything else of it lies in that chunk or in the 16 bytes in front of it, which have been loaded
// already -- by the lane below (one __shfl_up of the four dwords), by lane 63 of the row before (four wave-uniform dwords kept across
// the row loop), or, in a tile's first row, by one extra 16-byte load in front of the tile.  The order by last byte is the order by
// first byte, and the position reported is the last byte's minus (m - 1).  A row's chain (load, shuffle, match) is longer than the
// plain pass's, so both kernels issue the load of row r + 1 before they match row r.
// A byte outside the stream is replaced by ix_chunk with a value that occurs nowhere in the needle, so a window that reaches in front
// of the stream or behind it mismatches whatever needle position falls there.
// Ordering between tiles comes from the kernel boundaries alone: no wave ever waits for a value that another wave of the same launch
// produces (no chained scan, no look-back), so there is nothing that could spin.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "brx_find.h"

__device__ __forceinline__ uint4 fd_uniform(uint4 v) {
    return make_uint4((uint32_t)__builtin_amdgcn_readfirstlane((int)v.x), (uint32_t)__builtin_amdgcn_readfirstlane((int)v.y),
                      (uint32_t)__builtin_amdgcn_readfirstlane((int)v.z), (uint32_t)__builtin_amdgcn_readfirstlane((int)v.w));
}

// The 16 bytes in front of the tile at t0, as lane 63 of the row before would have loaded them (every lane asks for that chunk: one
// address, wave-uniform): masked to the stream and to the arena like any chunk, and not loaded where they lie in front of the stream.
__device__ __forceinline__ uint4 fd_halo(const uint8_t *out, uint64_t t0, uint64_t a, uint64_t e, uint64_t arena0, uint64_t arena1,
                                         uint32_t f4) {
    return fd_uniform(ix_chunk(out, t0 - BRX_TP_ROW, 63u, a, e, arena0, arena1, f4));
}

// -> the chunk in front of the lane's chunk v: that of the lane below, for lane 0 `carry`; carry moves on to this row's lane 63
__device__ __forceinline__ uint4 fd_prev(uint4 v, uint4 &carry, uint32_t lane) {
    uint4 p = make_uint4((uint32_t)__shfl_up((int)v.x, 1), (uint32_t)__shfl_up((int)v.y, 1), (uint32_t)__shfl_up((int)v.z, 1),
                         (uint32_t)__shfl_up((int)v.w, 1));
    if (lane == 0u) p = carry;
    carry = make_uint4((uint32_t)__builtin_amdgcn_readlane((int)v.x, 63), (uint32_t)__builtin_amdgcn_readlane((int)v.y, 63),
                       (uint32_t)__builtin_amdgcn_readlane((int)v.z, 63), (uint32_t)__builtin_amdgcn_readlane((int)v.w, 63));
    return p;
}

// 0x80 in byte b of f[d] where an occurrence of the needle ENDS at byte 4 d + b of the chunk v; p = the chunk in front of it.
// rn = the needle reversed (byte u = needle[m - 1 - u]): window byte 16 + 4 d + b - u must equal rn byte u for every u < m.  One step
// per distance u back from the end, u a template argument: every index into w[] and r[] is a constant and nothing is addressed in
// scratch memory.  acc[d] collects the differences: a byte of it is zero iff all m comparisons held.
template <uint32_t U>
__device__ __forceinline__ void fd_step(const uint32_t (&w)[8], const uint32_t (&r)[4], uint32_t (&acc)[4]) {
    const uint32_t b4 = ((r[U >> 2] >> (8u * (U & 3u))) & 255u) * 0x01010101u;
#pragma unroll
    for (uint32_t d = 0; d < 4u; d++) {
        const uint32_t hi = 4u + d - (U >> 2); // the dword whose byte b is window byte 16 + 4 d + b - U starts in w[hi - 1] ...
        const uint32_t s = (U & 3u) ? __builtin_amdgcn_alignbyte(w[hi], w[hi - 1u], 4u - (U & 3u)) : w[hi]; // ... unless U % 4 == 0
        acc[d] |= s ^ b4;
    }
}

// The steps commute (they OR into acc), so they run from u = m - 1 down to 0: the one test at run time is the wave-uniform entry into
// the unrolled sequence.
__device__ __forceinline__ void fd_ends(uint4 p, uint4 v, uint4 rn, uint32_t m, uint32_t f[4]) {
    const uint32_t w[8] = {p.x, p.y, p.z, p.w, v.x, v.y, v.z, v.w};
    const uint32_t r[4] = {rn.x, rn.y, rn.z, rn.w};
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
    switch (m) {
    case 16: fd_step<15>(w, r, acc); [[fallthrough]];
    case 15: fd_step<14>(w, r, acc); [[fallthrough]];
    case 14: fd_step<13>(w, r, acc); [[fallthrough]];
    case 13: fd_step<12>(w, r, acc); [[fallthrough]];
    case 12: fd_step<11>(w, r, acc); [[fallthrough]];
    case 11: fd_step<10>(w, r, acc); [[fallthrough]];
    case 10: fd_step<9>(w, r, acc); [[fallthrough]];
    case 9: fd_step<8>(w, r, acc); [[fallthrough]];
    case 8: fd_step<7>(w, r, acc); [[fallthrough]];
    case 7: fd_step<6>(w, r, acc); [[fallthrough]];
    case 6: fd_step<5>(w, r, acc); [[fallthrough]];
    case 5: fd_step<4>(w, r, acc); [[fallthrough]];
    case 4: fd_step<3>(w, r, acc); [[fallthrough]];
    case 3: fd_step<2>(w, r, acc); [[fallthrough]];
    case 2: fd_step<1>(w, r, acc); [[fallthrough]];
    default: fd_step<0>(w, r, acc); // (the host lets 1 .. 16 through)
    }
#pragma unroll
    for (uint32_t d = 0; d < 4u; d++) f[d] = ix_eq(acc[d], 0u);
}

__global__ __launch_bounds__(BRX_TP_WG, 8) void brx_find_count_kernel(const uint8_t *out, const uint64_t *__restrict__ out_off,
                                                                      const uint64_t *__restrict__ len, uint32_t n, uint64_t span,
                                                                      uint4 rn, uint32_t m, uint32_t f4,
                                                                      const uint64_t *__restrict__ pre, uint64_t max_tiles,
                                                                      uint64_t *__restrict__ tile_cnt, uint64_t *count,
                                                                      unsigned long long *ticket) {
    const uint64_t arena0 = (uint64_t)(uintptr_t)out, arena1 = arena0 + span;
    for (TpWalk w = tp_walk(tp_total(pre, n, max_tiles)); w.item < w.total; tp_advance(w, ticket)) {
        const TpItem it = tp_item(w.item, out, out_off, len, n, pre);
        uint4 carry = fd_halo(out, it.t0, it.a, it.e, arena0, arena1, f4);
        uint32_t acc = 0;
        uint4 nx = ix_chunk(out, it.t0, w.lane, it.a, it.e, arena0, arena1, f4);
        for (uint32_t r = 0; r < it.rows; r++) {
            const uint4 v = nx; // (the next row's load is in flight while this row is matched)
            if (r + 1u < it.rows) nx = ix_chunk(out, it.t0 + (uint64_t)(r + 1u) * BRX_TP_ROW, w.lane, it.a, it.e, arena0, arena1, f4);
            const uint4 p = fd_prev(v, carry, w.lane);
            uint32_t f[4];
            fd_ends(p, v, rn, m, f);
            acc += __popc(f[0]) + __popc(f[1]) + __popc(f[2]) + __popc(f[3]);
        }
        acc = tp_wave_sum(acc);
        if (w.lane == 0u) {
            if (tile_cnt) tile_cnt[w.item] = acc;
            if (count && acc) atomicAdd((unsigned long long *)&count[it.si], (unsigned long long)acc);
        }
    }
}

// This kernel keeps the walk, the mask and the row emit in its own text: they are tp_walk / tp_advance, ix_mask and tp_emit_row
// (brx_tiles.h, brx_index.h) letter for letter.  It holds 16 needle bytes next to the walk's scalars and spills about 30 of them, and
// with the shared functions in it the compiler spills differently and find's fill lines of the rate tool come out up to 0.4 % above
// the range of the text below (profiles/r24_boundary_passes.txt).  A change to one of the three goes here too.
__global__ __launch_bounds__(BRX_TP_WG, 8) void brx_find_fill_kernel(const uint8_t *out, const uint64_t *__restrict__ out_off,
                                                                     const uint64_t *__restrict__ len, uint32_t n, uint64_t span,
                                                                     uint4 rn, uint32_t m, uint32_t f4,
                                                                     const uint64_t *__restrict__ pre, uint64_t max_tiles,
                                                                     const uint64_t *__restrict__ tile_base,
                                                                     const uint64_t *__restrict__ pos_off, uint64_t *__restrict__ pos,
                                                                     uint64_t pos_total, unsigned long long *ticket) {
    const uint64_t total = pre[n] < max_tiles ? pre[n] : max_tiles;
    const uint32_t waves_per_wg = BRX_TP_WG / 64u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t grid_waves = (uint64_t)gridDim.x * waves_per_wg;
    const uint64_t arena0 = (uint64_t)(uintptr_t)out, arena1 = arena0 + span;
    uint64_t item = tp_uniform((uint64_t)blockIdx.x * waves_per_wg + (threadIdx.x >> 6));
    while (item < total) {
        const TpItem it = tp_item(item, out, out_off, len, n, pre);
        // index in pos of the tile's first occurrence: the stream's first entry + the occurrences of the stream's tiles in front of this one
        uint64_t base = tp_uniform(pos_off[it.si] + (tile_base[item] - tile_base[pre[it.si]]));
        uint4 carry = fd_halo(out, it.t0, it.a, it.e, arena0, arena1, f4);
        uint4 nx = ix_chunk(out, it.t0, lane, it.a, it.e, arena0, arena1, f4);
        for (uint32_t r = 0; r < it.rows; r++) {
            const uint64_t row = it.t0 + (uint64_t)r * BRX_TP_ROW;
            const uint4 v = nx; // (the next row's load is in flight while this row is matched)
            if (r + 1u < it.rows) nx = ix_chunk(out, row + BRX_TP_ROW, lane, it.a, it.e, arena0, arena1, f4);
            const uint4 p = fd_prev(v, carry, lane); // (every row: one without an occurrence still moves the carry on)
            uint32_t f[4];
            fd_ends(p, v, rn, m, f);
            uint32_t mk = ix_nib(f[0]) | (ix_nib(f[1]) << 4) | (ix_nib(f[2]) << 8) | (ix_nib(f[3]) << 12); // bit k: an occurrence ends at byte k of the chunk
            if (__ballot(mk != 0u) == 0ull) continue; // (uniform) a row without one
            const uint32_t c = (uint32_t)__popc(mk);
            uint32_t incl = c;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, s);
                if (lane >= (uint32_t)s) incl += up;
            }
            uint64_t idx = base + (incl - c);
            // offset in the stream of the first byte of an occurrence that ends at the chunk's byte 0 (an occurrence lies inside the
            // stream, so rel + k never wraps for a set bit k)
            const uint64_t rel = row + 16u * lane - it.a - (m - 1u);
            while (mk) {
                const uint32_t k = (uint32_t)__ffs((int)mk) - 1u;
                mk &= mk - 1u;
                if (idx < pos_total) pos[idx] = rel + k;
                idx++;
            }
            base += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
        item = tp_next(ticket, grid_waves, total, lane);
    }
}

void brx_launch_find(const void *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span, const uint8_t *needle,
                     uint32_t needle_len, void *scratch, uint64_t max_tiles, uint64_t *count, const uint64_t *pos_off, uint64_t *pos,
                     uint64_t total, unsigned workgroups, void *hip_stream) {
    // the needle reversed, in four dwords; and the filler: the first of 0 .. 16 that is none of its (at most 16) bytes
    uint32_t r[4] = {0u, 0u, 0u, 0u}, seen = 0u, filler = 0u;
    for (uint32_t u = 0; u < needle_len; u++) {
        const uint32_t b = needle[needle_len - 1u - u];
        r[u >> 2] |= b << (8u * (u & 3u));
        if (b <= BRX_FIND_MAX_NEEDLE) seen |= 1u << b;
    }
    while (seen >> filler & 1u) filler++;
    const uint4 rn = make_uint4(r[0], r[1], r[2], r[3]);
    const uint32_t f4 = filler * 0x01010101u;
    uint64_t *pre = brx_tp_pre(scratch), *tiles = (uint64_t *)brx_tp_own(scratch, n);
    hipStream_t st = (hipStream_t)hip_stream;
    brx_launch_tile_plan(out, out_off, len, n, scratch, (uint32_t *)count, count ? 2u : 0u, st);
    hipLaunchKernelGGL(brx_find_count_kernel, dim3(workgroups), dim3(BRX_TP_WG), 0, st, (const uint8_t *)out, out_off, len, n, span, rn,
                       needle_len, f4, pre, max_tiles, pos ? tiles : nullptr, count, brx_tp_ticket_a(scratch));
    if (!pos) return;
    hipLaunchKernelGGL(brx_index_scan_kernel, dim3(1), dim3(1024), 0, st, n, pre, max_tiles, tiles);
    hipLaunchKernelGGL(brx_find_fill_kernel, dim3(workgroups), dim3(BRX_TP_WG), 0, st, (const uint8_t *)out, out_off, len, n, span, rn,
                       needle_len, f4, pre, max_tiles, tiles, pos_off, pos, total, brx_tp_ticket_b(scratch));
}
