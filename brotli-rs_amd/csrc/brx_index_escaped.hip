// brx_index_escaped.hip -- brx_index_escaped_batch: the record delimiters of every decoded stream of a batch under a dialect with an
// escape byte (JSON Lines, SQL text dumps, CSV with an escape character), on the device (layout and state maps: brx_index_escaped.h).
//
// A byte is escaped exactly when the run of escape bytes directly in front of it, inside its stream, has odd length; an escaped byte
// is data.  A quote that is not escaped toggles "inside a quoted field", a delimiter that is neither escaped nor inside is a record
// delimiter.  So the pass is the tile pass of brx_index_quoted.hip with a second carried bit -- and that bit is no xor-able parity:
// what a tile does to it depends on the state the tile is entered in, so a tile hands on a map of the four states, and resolve
// composes the maps in tile order.  Count mode is three launches on the caller's stream, fill mode four:
//   plan     brx_tiles.hip.
//   count    a pass over the bytes.  Per tile, walked as if it were entered unescaped and outside quotes: c0 / c1 = unescaped delimiters
//            at even / odd parity of the tile's active quotes, that parity, the escape bit behind the tile, and what stands behind the
//            tile's leading run of escape bytes.  Entered escaped, only the status of that one byte changes, so the walk from the other
//            entry state follows from the word (ie_tile_map, ie_select): the bytes are walked once.
//   resolve  one workgroup, over all tiles of the batch in order: a scan with the composition of maps gives every tile the state it is
//            entered in (a stream's first tile is a constant map: segmentation falls out of the composition); G = exclusive prefix sum
//            of the counts selected by it; per stream count[i] as a difference of G and open[i] from the state behind its last tile.
//   fill     the count kernel's row body from the tile's real entry state, then tp_emit_row (brx_tiles.h) on the selected mask.
// brx_index_set_batch (a set of delimiters, the escape optional) is the same pass in a second dialect: see IeByte / IeSet below.
// Ordering between tiles comes from the kernel boundaries alone: no wave ever waits for a value that another wave of the same launch
// produces (no chained scan, no look-back), so there is nothing that could spin.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "brx_index_escaped.h"

// One row.  em, qm = the lane's escape and quote bytes; re, rp = the escape bit and the quote parity in front of the row (wave-uniform,
// moved on to the row's end).  -> bit k: byte k of the lane's chunk is escaped; in: bit k: an odd number of active quotes in front of
// and including byte k (a delimiter is no quote, so for the bytes that are looked at the inclusive parity is the exclusive one);
// some: the lanes whose chunk is not made of escape bytes only.
// The carry into a lane: a chunk of 16 escape bytes hands the run parity in front of it through unchanged (16 is even), any other
// chunk hands on the parity of its own trailing run whatever came in.  So it is the trailing-run parity of the nearest lower lane
// whose chunk is not all escape bytes, or the row's if there is none: two ballots and bit arithmetic, no shuffle chain.  The quote
// parity then goes as in brx_index_quoted.hip, over the quotes that are not escaped.
__device__ __forceinline__ uint32_t ie_row(uint32_t em, uint32_t qm, uint32_t lane, uint32_t &re, uint32_t &rp, uint32_t &in,
                                           uint64_t &some) {
    const bool mixed = em != 0xFFFFu;
    const uint32_t trail = (uint32_t)__clz((int)(~em << 16)) & 1u; // length of the run of escape bytes the chunk ends with, mod 2
    const uint64_t a = __ballot(mixed), t = __ballot(mixed && trail);
    const uint64_t below = a & ((1ull << lane) - 1ull);
    const uint32_t c = below ? (uint32_t)(t >> (63 - __clzll((long long)below))) & 1u : re;
    if (a) re = (uint32_t)(t >> (63 - __clzll((long long)a))) & 1u;
    some = a;
    const uint32_t esc = ie_escaped(em, c) & 0xFFFFu;
    uint32_t x = qm & ~esc;
    x ^= x << 1;
    x ^= x << 2;
    x ^= x << 4;
    x ^= x << 8;
    const uint64_t b = __ballot((x >> 15) & 1u);
    const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    const uint32_t carry = (before ^ rp) & 1u;
    rp ^= (uint32_t)__popcll(b) & 1u;
    in = (x ^ (0u - carry)) & 0xFFFFu;
    return esc;
}

// The state behind the tile's last byte of the stream, at address `end` - 1 in the row at `row` (the last one walked: it always holds
// that byte): escaped iff that byte is an escape byte that is not escaped itself.  Not the row's carry, which for a stream's last tile
// has passed the filler behind the stream.
__device__ __forceinline__ uint32_t ie_exit_escape(uint32_t em, uint32_t esc, uint32_t lane, uint64_t row, uint64_t end) {
    const uint32_t at = (uint32_t)(end - 1u - row);
    return __ballot(lane == (at >> 4) && ((em & ~esc) >> (at & 15u) & 1u)) != 0ull ? 1u : 0u;
}

// ---- the two dialects of this file ------------------------------------------------------------------------------------------
// brx_index_set_batch is brx_index_escaped_batch with a set of 1 .. 8 delimiter bytes, and with the escape as optional as the quote.
// A delimiter never changes the carried state, so "is the delimiter" becomes "is one of the set" in the row body and nothing else
// moves: ie_row, ie_exit_escape, the tile word, the resolve kernel and ie_select / ie_tile_map are the same.  So there is one count
// body and one fill body, and a dialect says what a delimiter is and whether an escape byte escapes.

// bit k: byte k of the chunk is one of the nd (1 .. 8) bytes of `set`: the OR of ix_mask over the set, taken before the bits are
// gathered so that the gathering is done once
__device__ __forceinline__ uint32_t is_mask(uint4 v, uint64_t set, uint32_t nd) {
    uint32_t x = 0, y = 0, z = 0, w = 0;
    for (uint32_t k = 0; k < nd; k++) { // (uniform)
        const uint32_t d4 = ((uint32_t)set & 0xFFu) * 0x01010101u;
        set >>= 8;
        x |= ix_eq(v.x, d4);
        y |= ix_eq(v.y, d4);
        z |= ix_eq(v.z, d4);
        w |= ix_eq(v.w, d4);
    }
    return ix_nib(x) | (ix_nib(y) << 4) | (ix_nib(z) << 8) | (ix_nib(w) << 12);
}

// byte k of the chunk
__device__ __forceinline__ uint32_t is_byte(uint4 v, uint32_t k) {
    const uint32_t w = k & 8u ? (k & 4u ? v.w : v.z) : (k & 4u ? v.y : v.x);
    return w >> (8u * (k & 3u)) & 0xFFu;
}

// brx_index_escaped_batch: one delimiter byte (d4 = four times), the escape always on -- which the compiler sees
struct IeByte {
    uint32_t d4;
    __device__ __forceinline__ uint32_t delims(uint4 v) const { return ix_mask(v, d4); }
    __device__ __forceinline__ uint32_t escapes(uint32_t em) const { return em; }
};

// brx_index_set_batch: the set travels as launch arguments (byte k of `set` for k < nd: SGPRs), the loop over it is wave-uniform;
// eon = 0 forces the escape mask to 0 as qon = 0 does the quote mask
struct IeSet {
    uint64_t set;
    uint32_t nd, eon;
    __device__ __forceinline__ uint32_t delims(uint4 v) const { return is_mask(v, set, nd); }
    __device__ __forceinline__ uint32_t escapes(uint32_t em) const { return em & eon; }
};

// count: per tile, walked as if it were entered unescaped and outside quotes, the tile word (brx_index_escaped.h)
template <class D>
__device__ __forceinline__ void ie_count_tiles(const uint8_t *out, const uint64_t *__restrict__ out_off, const uint64_t *__restrict__ len,
                                               uint32_t n, uint64_t span, const D d, uint32_t quote, uint32_t escape, uint32_t quotes,
                                               uint32_t f4, const uint64_t *__restrict__ pre, uint64_t max_tiles,
                                               uint64_t *__restrict__ tile_word, unsigned long long *ticket) {
    const uint32_t q4 = quote * 0x01010101u, e4 = escape * 0x01010101u, qon = quotes ? 0xFFFFu : 0u;
    const uint64_t arena0 = (uint64_t)(uintptr_t)out, arena1 = arena0 + span;
    for (TpWalk w = tp_walk(tp_total(pre, n, max_tiles)); w.item < w.total; tp_advance(w, ticket)) {
        const TpItem it = tp_item(w.item, out, out_off, len, n, pre);
        uint32_t all = 0, odd = 0, rp = 0, re = 0, em = 0, esc = 0;
        uint32_t lead = 4u, rodd = 0; // 4: the leading run of escape bytes has not ended yet
        uint64_t row = it.t0;
        for (uint32_t r = 0; r < it.rows; r++) {
            row = it.t0 + (uint64_t)r * BRX_TP_ROW;
            const uint4 v = ix_chunk(out, row, w.lane, it.a, it.e, arena0, arena1, f4);
            em = d.escapes(ix_mask(v, e4));
            const uint32_t qm = ix_mask(v, q4) & qon, dm = d.delims(v);
            uint32_t in;
            uint64_t some;
            esc = ie_row(em, qm, w.lane, re, rp, in, some);
            if (lead == 4u && some) { // (uniform) once per tile: the first byte that is no escape byte
                const uint32_t fl = (uint32_t)__ffsll((long long)some) - 1u;
                const uint32_t k = (uint32_t)__ffs((int)(~em & 0xFFFFu)) - 1u; // (a lane without one: not the lane that is read)
                const uint32_t mine = (k & 15u) | ((dm >> (k & 15u) & 1u) << 4) | ((qm >> (k & 15u) & 1u) << 5);
                const uint32_t got = (uint32_t)__shfl((int)mine, (int)fl);
                // the chunks and rows in front of it are escape bytes only, an even number: the run's parity is that of the offset
                rodd = got & 1u;
                lead = row + 16u * fl + (got & 15u) >= it.e ? BRX_IE_LEAD_ALL : got >> 4; // (filler behind the stream's end is no byte of it)
            }
            const uint32_t m = dm & ~esc;
            all += __popc(m);
            odd += __popc(m & in);
        }
        if (lead == 4u) lead = BRX_IE_LEAD_ALL;
        const uint32_t x = ie_exit_escape(em, esc, w.lane, row, it.t1);
        all = tp_wave_sum(all);
        odd = tp_wave_sum(odd);
        if (w.lane == 0u)
            tile_word[w.item] = (uint64_t)(all - odd) | ((uint64_t)odd << BRX_IE_C0_BITS) | ((uint64_t)rp << BRX_IE_PAR_SHIFT) |
                                ((uint64_t)x << BRX_IE_X_SHIFT) | ((uint64_t)lead << BRX_IE_LEAD_SHIFT) |
                                ((uint64_t)rodd << BRX_IE_RODD_SHIFT);
    }
}

// fill: the count body's row from the tile's real entry state, then tp_emit_row (brx_tiles.h) on the selected mask; next to every
// position goes the byte that stands there, taken from the chunk in registers, if `what` is given
template <class D>
__device__ __forceinline__ void ie_fill_tiles(const uint8_t *out, const uint64_t *__restrict__ out_off, const uint64_t *__restrict__ len,
                                              uint32_t n, uint64_t span, const D d, uint32_t quote, uint32_t escape, uint32_t quotes,
                                              uint32_t f4, const uint64_t *__restrict__ pre, uint64_t max_tiles,
                                              const uint64_t *__restrict__ tile_word, const uint64_t *__restrict__ pos_off,
                                              uint64_t *__restrict__ pos, uint8_t *__restrict__ what, uint64_t pos_total,
                                              unsigned long long *ticket) {
    const uint32_t q4 = quote * 0x01010101u, e4 = escape * 0x01010101u, qon = quotes ? 0xFFFFu : 0u;
    const uint64_t arena0 = (uint64_t)(uintptr_t)out, arena1 = arena0 + span;
    for (TpWalk w = tp_walk(tp_total(pre, n, max_tiles)); w.item < w.total; tp_advance(w, ticket)) {
        const TpItem it = tp_item(w.item, out, out_off, len, n, pre);
        const uint64_t tw = tp_uniform(tile_word[w.item]);
        // index in pos of the tile's first boundary: the stream's first entry + those of the stream's tiles in front of this one
        uint64_t base = tp_uniform(pos_off[it.si] + ((tw & BRX_IE_G_MASK) - (tile_word[pre[it.si]] & BRX_IE_G_MASK)));
        uint32_t rp = (uint32_t)(tw >> BRX_IE_ENTRY_SHIFT) & 1u, re = (uint32_t)(tw >> (BRX_IE_ENTRY_SHIFT + 1u)) & 1u;
        for (uint32_t r = 0; r < it.rows; r++) {
            const uint64_t row = it.t0 + (uint64_t)r * BRX_TP_ROW;
            const uint4 v = ix_chunk(out, row, w.lane, it.a, it.e, arena0, arena1, f4);
            uint32_t in;
            uint64_t some;
            // (every row: one without a boundary still moves the state on)
            const uint32_t esc = ie_row(d.escapes(ix_mask(v, e4)), ix_mask(v, q4) & qon, w.lane, re, rp, in, some);
            const uint32_t m = d.delims(v) & ~esc & ~in; // bit k: byte k of the chunk is a boundary of the stream
            const uint64_t rel = row + 16u * w.lane - it.a; // offset of the chunk's byte 0 in the stream (m == 0 where that is in front of it)
            tp_emit_row(m, w.lane, base, pos_total, [&](uint64_t idx, uint32_t k) {
                pos[idx] = rel + k;
                if (what) what[idx] = (uint8_t)is_byte(v, k); // (uniform)
            });
        }
    }
}

__global__ __launch_bounds__(BRX_TP_WG, 8) void brx_index_escaped_count_kernel(const uint8_t *out, const uint64_t *__restrict__ out_off,
                                                                               const uint64_t *__restrict__ len, uint32_t n,
                                                                               uint64_t span, uint32_t delim, uint32_t quote,
                                                                               uint32_t escape, uint32_t quotes,
                                                                               const uint64_t *__restrict__ pre, uint64_t max_tiles,
                                                                               uint64_t *__restrict__ tile_word,
                                                                               unsigned long long *ticket) {
    ie_count_tiles(out, out_off, len, n, span, IeByte{delim * 0x01010101u}, quote, escape, quotes,
                   ix_filler(delim, 1u, quote, quotes, escape, 1u), pre, max_tiles, tile_word, ticket);
}

// the tile word is the escaped pass's, BRX_IE_LEAD_DELIM meaning "a byte of the set"
__global__ __launch_bounds__(BRX_TP_WG, 8) void brx_index_set_count_kernel(const uint8_t *out, const uint64_t *__restrict__ out_off,
                                                                           const uint64_t *__restrict__ len, uint32_t n, uint64_t span,
                                                                           uint64_t set, uint32_t nd, uint32_t quote, uint32_t escape,
                                                                           uint32_t quotes, uint32_t escapes,
                                                                           const uint64_t *__restrict__ pre, uint64_t max_tiles,
                                                                           uint64_t *__restrict__ tile_word, unsigned long long *ticket) {
    ie_count_tiles(out, out_off, len, n, span, IeSet{set, nd, escapes ? 0xFFFFu : 0u}, quote, escape, quotes,
                   ix_filler(set, nd, quote, quotes, escape, escapes), pre, max_tiles, tile_word, ticket);
}

// inclusive scan with ie_compose of one map per thread of a 1024-thread workgroup in `part` (1024 words of LDS), the earlier tile being
// the left operand: -> the composition of the maps of threads 0 .. t
__device__ __forceinline__ uint32_t ie_block_scan_1024(uint32_t *part, uint32_t t, uint32_t map) {
    part[t] = map;
    __syncthreads();
    for (uint32_t s = 1; s < 1024u; s <<= 1) {
        const uint32_t f = t >= s ? part[t - s] : BRX_IE_MAP_IDENTITY;
        __syncthreads();
        part[t] = ie_compose(f, part[t]);
        __syncthreads();
    }
    return part[t];
}

// One workgroup; thread t takes its slice of the tiles (tp_slice_1024), as brx_index_scan_kernel does, and until the last barrier reads
// and writes the words of its own slice only: what crosses slices goes through the two scans in LDS.
__global__ __launch_bounds__(1024) void brx_index_escaped_resolve_kernel(uint32_t n, const uint64_t *__restrict__ pre, uint64_t max_tiles,
                                                                         uint64_t *tile_word, uint64_t *tile_exit,
                                                                         uint64_t *__restrict__ count, uint32_t *__restrict__ open) {
    __shared__ uint64_t part[1024];
    __shared__ uint32_t maps[1024];
    const uint64_t total = tp_total(pre, n, max_tiles);
    const uint32_t t = threadIdx.x;
    const TpSlice sl = tp_slice_1024(total, t);
    const uint64_t i0 = sl.i0, i1 = sl.i1;
    // 1: the slice's map, tile by tile in order; the scan gives the state in front of the slice (the batch starts in state 0, and its
    // first tile is a stream's first anyway)
    const uint32_t s0 = i0 < i1 ? tp_stream_of(i0, n, pre) : 0u;
    uint32_t si = s0;
    uint32_t map = BRX_IE_MAP_IDENTITY;
    for (uint64_t i = i0; i < i1; i++) {
        while (si + 1u < n && pre[si + 1u] <= i) si++;
        map = ie_compose(map, ie_tile_map(tile_word[i], pre[si] == i));
    }
    ie_block_scan_1024(maps, t, map);
    uint32_t state = t ? ie_apply(maps[t - 1u], 0u) : 0u;
    // 2: every tile's entry state, the count it selects and the state behind the tile
    si = s0;
    uint64_t sum = 0;
    for (uint64_t i = i0; i < i1; i++) {
        while (si + 1u < n && pre[si + 1u] <= i) si++;
        const uint64_t w = tile_word[i];
        const int first = pre[si] == i;
        if (first) state = 0u;
        const uint64_t c = ie_select(w, state);
        tile_word[i] = c | ((uint64_t)state << BRX_IE_ENTRY_SHIFT);
        state = ie_apply(ie_tile_map(w, first), state);
        tile_exit[i] = state;
        sum += c;
    }
    // 3: G, the exclusive prefix sum of the selected counts over all tiles of the batch, into the word, next to the entry state
    uint64_t run = tp_block_scan_1024(part, t, sum) - sum;
    for (uint64_t i = i0; i < i1; i++) {
        const uint64_t w = tile_word[i];
        tile_word[i] = run | (w & ~BRX_IE_G_MASK);
        run += w & BRX_IE_G_MASK;
    }
    if (t == 1023u) tile_word[total] = run;
    __syncthreads();
    // 4: per stream: count as a difference of G over the whole batch, open from the state behind the stream's last tile; streams
    // without tiles (which share their successor's pre[]) get 0 and 0
    for (uint64_t i = t; i < n; i += 1024u) {
        const uint64_t a = pre[i] < total ? pre[i] : total, b = pre[i + 1u] < total ? pre[i + 1u] : total;
        if (count) count[i] = (tile_word[b] & BRX_IE_G_MASK) - (tile_word[a] & BRX_IE_G_MASK);
        if (open) open[i] = b > a ? (uint32_t)tile_exit[b - 1u] : 0u;
    }
}

__global__ __launch_bounds__(BRX_TP_WG, 8) void brx_index_escaped_fill_kernel(const uint8_t *out, const uint64_t *__restrict__ out_off,
                                                                              const uint64_t *__restrict__ len, uint32_t n, uint64_t span,
                                                                              uint32_t delim, uint32_t quote, uint32_t escape,
                                                                              uint32_t quotes, const uint64_t *__restrict__ pre,
                                                                              uint64_t max_tiles, const uint64_t *__restrict__ tile_word,
                                                                              const uint64_t *__restrict__ pos_off,
                                                                              uint64_t *__restrict__ pos, uint64_t pos_total,
                                                                              unsigned long long *ticket) {
    ie_fill_tiles(out, out_off, len, n, span, IeByte{delim * 0x01010101u}, quote, escape, quotes,
                  ix_filler(delim, 1u, quote, quotes, escape, 1u), pre, max_tiles, tile_word, pos_off, pos, nullptr, pos_total, ticket);
}

// `what` may be NULL
__global__ __launch_bounds__(BRX_TP_WG, 8) void brx_index_set_fill_kernel(const uint8_t *out, const uint64_t *__restrict__ out_off,
                                                                          const uint64_t *__restrict__ len, uint32_t n, uint64_t span,
                                                                          uint64_t set, uint32_t nd, uint32_t quote, uint32_t escape,
                                                                          uint32_t quotes, uint32_t escapes,
                                                                          const uint64_t *__restrict__ pre, uint64_t max_tiles,
                                                                          const uint64_t *__restrict__ tile_word,
                                                                          const uint64_t *__restrict__ pos_off, uint64_t *__restrict__ pos,
                                                                          uint8_t *__restrict__ what, uint64_t pos_total,
                                                                          unsigned long long *ticket) {
    ie_fill_tiles(out, out_off, len, n, span, IeSet{set, nd, escapes ? 0xFFFFu : 0u}, quote, escape, quotes,
                  ix_filler(set, nd, quote, quotes, escape, escapes), pre, max_tiles, tile_word, pos_off, pos, what, pos_total, ticket);
}

void brx_launch_index_escaped(const void *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span, uint8_t delim,
                              uint8_t quote, uint8_t escape, uint32_t flags, void *scratch, uint64_t max_tiles, uint64_t *count,
                              uint32_t *open, const uint64_t *pos_off, uint64_t *pos, uint64_t total, unsigned workgroups,
                              void *hip_stream) {
    uint64_t *pre = brx_tp_pre(scratch), *words = (uint64_t *)brx_tp_own(scratch, n), *exits = words + max_tiles + 1u;
    const uint32_t quotes = (flags & BRX_INDEX_ESCAPED_NO_QUOTE) ? 0u : 1u;
    hipStream_t st = (hipStream_t)hip_stream;
    brx_launch_tile_plan(out, out_off, len, n, scratch, nullptr, 0u, st); // (resolve writes every count[i] and open[i]: nothing to clear)
    hipLaunchKernelGGL(brx_index_escaped_count_kernel, dim3(workgroups), dim3(BRX_TP_WG), 0, st, (const uint8_t *)out, out_off, len, n,
                       span, (uint32_t)delim, (uint32_t)quote, (uint32_t)escape, quotes, pre, max_tiles, words,
                       brx_tp_ticket_a(scratch));
    hipLaunchKernelGGL(brx_index_escaped_resolve_kernel, dim3(1), dim3(1024), 0, st, n, pre, max_tiles, words, exits, count, open);
    if (!pos) return;
    hipLaunchKernelGGL(brx_index_escaped_fill_kernel, dim3(workgroups), dim3(BRX_TP_WG), 0, st, (const uint8_t *)out, out_off, len, n,
                       span, (uint32_t)delim, (uint32_t)quote, (uint32_t)escape, quotes, pre, max_tiles, words, pos_off, pos, total,
                       brx_tp_ticket_b(scratch));
}

// ---- brx_index_set_batch: the same launches with the set's two kernels around the one resolve kernel ---------------------------
void brx_launch_index_set(const void *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span, uint64_t set,
                          uint32_t n_delims, uint8_t quote, uint8_t escape, uint32_t flags, void *scratch, uint64_t max_tiles,
                          uint64_t *count, uint32_t *open, const uint64_t *pos_off, uint64_t *pos, uint8_t *what, uint64_t total,
                          unsigned workgroups, void *hip_stream) {
    uint64_t *pre = brx_tp_pre(scratch), *words = (uint64_t *)brx_tp_own(scratch, n), *exits = words + max_tiles + 1u;
    const uint32_t quotes = (flags & BRX_INDEX_SET_NO_QUOTE) ? 0u : 1u, escapes = (flags & BRX_INDEX_SET_NO_ESCAPE) ? 0u : 1u;
    hipStream_t st = (hipStream_t)hip_stream;
    brx_launch_tile_plan(out, out_off, len, n, scratch, nullptr, 0u, st); // (resolve writes every count[i] and open[i]: nothing to clear)
    hipLaunchKernelGGL(brx_index_set_count_kernel, dim3(workgroups), dim3(BRX_TP_WG), 0, st, (const uint8_t *)out, out_off, len, n, span,
                       set, n_delims, (uint32_t)quote, (uint32_t)escape, quotes, escapes, pre, max_tiles, words,
                       brx_tp_ticket_a(scratch));
    hipLaunchKernelGGL(brx_index_escaped_resolve_kernel, dim3(1), dim3(1024), 0, st, n, pre, max_tiles, words, exits, count, open);
    if (!pos) return;
    hipLaunchKernelGGL(brx_index_set_fill_kernel, dim3(workgroups), dim3(BRX_TP_WG), 0, st, (const uint8_t *)out, out_off, len, n, span,
                       set, n_delims, (uint32_t)quote, (uint32_t)escape, quotes, escapes, pre, max_tiles, words, pos_off, pos, what,
                       total, brx_tp_ticket_b(scratch));
}
