// brx_index_quoted.hip -- brx_index_quoted_batch: the record delimiters of every decoded stream of a batch that lie outside quoted
// fields (RFC 4180), on the device (layout: brx_index_quoted.h).
//
// A byte of a stream lies inside a quoted field exactly when the number of quote bytes in front of it in the stream is odd (a doubled
// quote toggles twice), so "inside" is a prefix parity and the pass is the tile pass (brx_tiles.h) of brx_index.hip with one more
// carried bit per lane, row and tile.  Count mode is three launches on the caller's stream, fill mode four:
//   plan     brx_tiles.hip.
//   count    a pass over the bytes.  Per tile, taken as if it started outside quotes: c0 = delimiters at even parity, c1 = delimiters
//            at odd parity, par = parity of its quotes, packed into the tile's scratch word.  If the tile really starts inside a quoted
//            field every parity in it is inverted, so its record delimiters are c1 instead of c0.
//   resolve  one workgroup, over all tiles of the batch in order: P = exclusive prefix parity of par; tile t of stream i starts with
//            parity P[t] ^ P[first tile of i]; G = exclusive prefix sum of the counts selected by it.  Then per stream count[i] and
//            open[i] as differences of G and P between the stream's first tile and its successor's.
//   fill     the count kernel's row body with the tile's real start parity, then tp_emit_row (brx_tiles.h) on the selected mask.
// Ordering between tiles comes from the kernel boundaries alone: no wave ever waits for a value that another wave of the same launch
// produces (no chained scan, no look-back), so there is nothing that could spin.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "brx_index_quoted.h"

// qm = the lane's quote bytes of a row, rp = the parity in front of the row (wave-uniform, moved on to the row's end).  -> bit k: an
// odd number of quotes in front of and including byte k of the lane's chunk.  A delimiter is no quote, so for the bytes that are looked
// at the inclusive parity is the exclusive one.  In the lane four shift-xor steps; across the lanes one ballot of the lanes' parities
// and a population count of the bits below the lane: no shuffle chain.
__device__ __forceinline__ uint32_t iq_inside(uint32_t qm, uint32_t &rp) {
    uint32_t x = qm;
    x ^= x << 1;
    x ^= x << 2;
    x ^= x << 4;
    x ^= x << 8;
    const uint64_t b = __ballot((x >> 15) & 1u);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    const uint32_t carry = (below ^ rp) & 1u;
    rp ^= (uint32_t)__popcll(b) & 1u;
    return (x ^ (0u - carry)) & 0xFFFFu;
}

__global__ __launch_bounds__(BRX_TP_WG, 8) void brx_index_quoted_count_kernel(const uint8_t *out, const uint64_t *__restrict__ out_off,
                                                                              const uint64_t *__restrict__ len, uint32_t n,
                                                                              uint64_t span, uint32_t delim, uint32_t quote,
                                                                              const uint64_t *__restrict__ pre, uint64_t max_tiles,
                                                                              uint64_t *__restrict__ tile_word,
                                                                              unsigned long long *ticket) {
    const uint32_t d4 = delim * 0x01010101u, q4 = quote * 0x01010101u, f4 = ix_filler(delim, 1u, quote, 1u, 0u, 0u);
    const uint64_t arena0 = (uint64_t)(uintptr_t)out, arena1 = arena0 + span;
    for (TpWalk w = tp_walk(tp_total(pre, n, max_tiles)); w.item < w.total; tp_advance(w, ticket)) {
        const TpItem it = tp_item(w.item, out, out_off, len, n, pre);
        uint32_t all = 0, odd = 0, rp = 0;
        for (uint32_t r = 0; r < it.rows; r++) {
            const uint4 v = ix_chunk(out, it.t0 + (uint64_t)r * BRX_TP_ROW, w.lane, it.a, it.e, arena0, arena1, f4);
            const uint32_t dm = ix_mask(v, d4);
            const uint32_t in = iq_inside(ix_mask(v, q4), rp);
            all += __popc(dm);
            odd += __popc(dm & in);
        }
        all = tp_wave_sum(all);
        odd = tp_wave_sum(odd);
        if (w.lane == 0u)
            tile_word[w.item] = (uint64_t)(all - odd) | ((uint64_t)odd << BRX_IQ_C0_BITS) | ((uint64_t)rp << BRX_IQ_PAR_SHIFT);
    }
}

// One workgroup; thread t takes its slice of the tiles (tp_slice_1024), as brx_index_scan_kernel does.  A word of another thread's slice
// is read only for its bit 63 (P), which step 1 writes and nothing changes behind the barrier that follows it.
__global__ __launch_bounds__(1024) void brx_index_quoted_resolve_kernel(uint32_t n, const uint64_t *__restrict__ pre, uint64_t max_tiles,
                                                                        uint64_t *tile_word, uint64_t *__restrict__ count,
                                                                        uint32_t *__restrict__ open) {
    __shared__ uint64_t part[1024];
    const uint64_t total = tp_total(pre, n, max_tiles);
    const uint32_t t = threadIdx.x;
    const TpSlice sl = tp_slice_1024(total, t);
    const uint64_t i0 = sl.i0, i1 = sl.i1;
    // 1: P[t], the parity of the quotes of all tiles in front of tile t, into bit 63 of the tile's word
    uint64_t par = 0;
    for (uint64_t i = i0; i < i1; i++) par ^= tile_word[i] >> BRX_IQ_PAR_SHIFT & 1u;
    uint64_t p = (tp_block_scan_1024(part, t, par) - par) & 1u;
    for (uint64_t i = i0; i < i1; i++) {
        const uint64_t w = tile_word[i];
        tile_word[i] = (w & ~(1ull << BRX_IQ_P_SHIFT)) | (p << BRX_IQ_P_SHIFT);
        p ^= w >> BRX_IQ_PAR_SHIFT & 1u;
    }
    if (t == 1023u) tile_word[total] = p << BRX_IQ_P_SHIFT;
    __syncthreads();
    // 2: the parity a tile of stream i starts with is P[t] ^ P[first tile of i] (every stream starts outside quotes); it selects c1 or c0
    const uint32_t s0 = i0 < i1 ? tp_stream_of(i0, n, pre) : 0u;
    uint32_t si = s0;
    uint64_t sum = 0;
    for (uint64_t i = i0; i < i1; i++) {
        while (si + 1u < n && pre[si + 1u] <= i) si++;
        const uint64_t w = tile_word[i];
        const uint64_t first = __hip_atomic_load(&tile_word[pre[si]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const uint64_t start = (w ^ first) >> BRX_IQ_P_SHIFT;
        sum += (start ? w >> BRX_IQ_C0_BITS : w) & BRX_IQ_C_MASK;
    }
    // 3: G, the exclusive prefix sum of the selected counts over all tiles of the batch, into the word, next to the start parity and P
    uint64_t run = tp_block_scan_1024(part, t, sum) - sum;
    si = s0;
    for (uint64_t i = i0; i < i1; i++) {
        while (si + 1u < n && pre[si + 1u] <= i) si++;
        const uint64_t w = tile_word[i];
        const uint64_t first = __hip_atomic_load(&tile_word[pre[si]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const uint64_t start = (w ^ first) >> BRX_IQ_P_SHIFT;
        __hip_atomic_store(&tile_word[i], run | (start << BRX_IQ_START_SHIFT) | (w & (1ull << BRX_IQ_P_SHIFT)), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
        run += (start ? w >> BRX_IQ_C0_BITS : w) & BRX_IQ_C_MASK;
    }
    if (t == 1023u) tile_word[total] = run | (tile_word[total] & (1ull << BRX_IQ_P_SHIFT));
    __syncthreads();
    // 4: per stream, differences over the whole batch: no segmented scan, nothing leaks from a stream into the next, and streams
    // without tiles (which share their successor's pre[]) get 0 and 0
    for (uint64_t i = t; i < n; i += 1024u) {
        const uint64_t a = tile_word[pre[i] < total ? pre[i] : total], b = tile_word[pre[i + 1u] < total ? pre[i + 1u] : total];
        if (count) count[i] = (b & BRX_IQ_G_MASK) - (a & BRX_IQ_G_MASK);
        if (open) open[i] = (uint32_t)((a ^ b) >> BRX_IQ_P_SHIFT);
    }
}

__global__ __launch_bounds__(BRX_TP_WG, 8) void brx_index_quoted_fill_kernel(const uint8_t *out, const uint64_t *__restrict__ out_off,
                                                                             const uint64_t *__restrict__ len, uint32_t n, uint64_t span,
                                                                             uint32_t delim, uint32_t quote,
                                                                             const uint64_t *__restrict__ pre, uint64_t max_tiles,
                                                                             const uint64_t *__restrict__ tile_word,
                                                                             const uint64_t *__restrict__ pos_off,
                                                                             uint64_t *__restrict__ pos, uint64_t pos_total,
                                                                             unsigned long long *ticket) {
    const uint32_t d4 = delim * 0x01010101u, q4 = quote * 0x01010101u, f4 = ix_filler(delim, 1u, quote, 1u, 0u, 0u);
    const uint64_t arena0 = (uint64_t)(uintptr_t)out, arena1 = arena0 + span;
    for (TpWalk w = tp_walk(tp_total(pre, n, max_tiles)); w.item < w.total; tp_advance(w, ticket)) {
        const TpItem it = tp_item(w.item, out, out_off, len, n, pre);
        const uint64_t tw = tp_uniform(tile_word[w.item]);
        // index in pos of the tile's first record delimiter: the stream's first entry + those of the stream's tiles in front of this one
        uint64_t base = tp_uniform(pos_off[it.si] + ((tw & BRX_IQ_G_MASK) - (tile_word[pre[it.si]] & BRX_IQ_G_MASK)));
        uint32_t rp = (uint32_t)(tw >> BRX_IQ_START_SHIFT) & 1u;
        for (uint32_t r = 0; r < it.rows; r++) {
            const uint64_t row = it.t0 + (uint64_t)r * BRX_TP_ROW;
            const uint4 v = ix_chunk(out, row, w.lane, it.a, it.e, arena0, arena1, f4);
            const uint32_t in = iq_inside(ix_mask(v, q4), rp); // (every row: one without a delimiter still moves the parity on)
            const uint32_t m = ix_mask(v, d4) & ~in; // bit k: byte k of the chunk is a record delimiter of the stream
            const uint64_t rel = row + 16u * w.lane - it.a; // offset of the chunk's byte 0 in the stream (m == 0 where that is in front of it)
            tp_emit_row(m, w.lane, base, pos_total, [&](uint64_t idx, uint32_t k) { pos[idx] = rel + k; });
        }
    }
}

void brx_launch_index_quoted(const void *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span, uint8_t delim,
                             uint8_t quote, void *scratch, uint64_t max_tiles, uint64_t *count, uint32_t *open, const uint64_t *pos_off,
                             uint64_t *pos, uint64_t total, unsigned workgroups, void *hip_stream) {
    uint64_t *pre = brx_tp_pre(scratch), *tiles = (uint64_t *)brx_tp_own(scratch, n);
    hipStream_t st = (hipStream_t)hip_stream;
    brx_launch_tile_plan(out, out_off, len, n, scratch, nullptr, 0u, st); // (resolve writes every count[i] and open[i]: nothing to clear)
    hipLaunchKernelGGL(brx_index_quoted_count_kernel, dim3(workgroups), dim3(BRX_TP_WG), 0, st, (const uint8_t *)out, out_off, len, n,
                       span, (uint32_t)delim, (uint32_t)quote, pre, max_tiles, tiles, brx_tp_ticket_a(scratch));
    hipLaunchKernelGGL(brx_index_quoted_resolve_kernel, dim3(1), dim3(1024), 0, st, n, pre, max_tiles, tiles, count, open);
    if (!pos) return;
    hipLaunchKernelGGL(brx_index_quoted_fill_kernel, dim3(workgroups), dim3(BRX_TP_WG), 0, st, (const uint8_t *)out, out_off, len, n,
                       span, (uint32_t)delim, (uint32_t)quote, pre, max_tiles, tiles, pos_off, pos, total, brx_tp_ticket_b(scratch));
}
