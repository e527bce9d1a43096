// brx_tiles.h -- the tile pass: the one shape of every pass that walks the decoded streams of a device-resident batch (brx_digest.hip,
// brx_index.hip, brx_index_quoted.hip, brx_index_escaped.hip, brx_find.hip; the host side of its scratch in brx_api.cpp).
//
// A work item is one (stream, tile) pair, a tile = 64 KiB of the stream's 1 KiB aligned address range.  The host never learns a length,
// so a one-workgroup plan kernel (brx_tiles.hip) computes tiles per stream and their exclusive prefix sum pre[0 .. n] on the device.
// A pass over the bytes is a persistent grid of 4 workgroups of 8 waves per CU: a wave's first item is its index in the grid, the
// following ones come from a ticket counter (TpWalk); the stream of an item is found by binary search in pre[] (tp_stream_of).  The
// wave walks its tile in aligned 1 KiB rows, 16 B per lane.  What a pass does with a row, and what it loads at a stream's edges, is
// its own: a kernel states its per-tile body.  What several bodies do the same way stands here too: the sum over a wave's lanes
// (tp_wave_sum), the positions of a row's set bits in stream order (tp_emit_row), and for the one-workgroup kernels between two
// passes the slice of a thread (tp_slice_1024) and the scan over the slices (tp_block_scan_1024).
#pragma once
#include <stddef.h>
#include <stdint.h>

#define BRX_TP_ROW 1024u            // bytes a wavefront reads per step: 64 lanes x 16 B, 1 KiB aligned
#define BRX_TP_TILE_ROWS 64u
#define BRX_TP_TILE (BRX_TP_ROW * BRX_TP_TILE_ROWS) // one work item: 64 KiB of a stream's (1 KiB aligned) address range
#define BRX_TP_WG 512u              // threads per workgroup of a pass over the bytes: 8 waves

// Scratch region of one launch, in bytes from its start:
#define BRX_TP_TICKET_A 0u          // ticket counter of the pass over the bytes, on a line of its own
#define BRX_TP_TICKET_B 128u        // ticket counter of a second pass over the same items, likewise
#define BRX_TP_PRE 256u             // n + 1 words of 64 bits: exclusive prefix sum of the tiles per stream; behind them the pass's own words

static inline unsigned long long *brx_tp_ticket_a(void *scratch) { return (unsigned long long *)((uint8_t *)scratch + BRX_TP_TICKET_A); }
static inline unsigned long long *brx_tp_ticket_b(void *scratch) { return (unsigned long long *)((uint8_t *)scratch + BRX_TP_TICKET_B); }
static inline uint64_t *brx_tp_pre(void *scratch) { return (uint64_t *)((uint8_t *)scratch + BRX_TP_PRE); }
static inline void *brx_tp_own(void *scratch, uint32_t n) { return brx_tp_pre(scratch) + (size_t)n + 1u; }
// bytes of a region for n streams and `own` bytes of the pass's own words
static inline size_t brx_tp_region_bytes(size_t n, size_t own) { return (BRX_TP_PRE + (n + 1u) * 8u + own + 127u) & ~(size_t)127u; }

// plan (brx_tiles.hip), first launch of every pass: pre[0 .. n] of the region at `scratch`, both ticket counters cleared, and `w` 32-bit
// words per stream cleared at `clear` (w == 0: nothing)
void brx_launch_tile_plan(const void *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, void *scratch, uint32_t *clear,
                          uint32_t w, void *hip_stream);

#ifdef __HIPCC__
// a value that is the same in every lane of the wave, said so to the compiler: what depends on it is loaded by the scalar unit
__device__ __forceinline__ uint64_t tp_uniform(uint64_t v) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32);
}

// tiles of a stream of l bytes whose first byte is at address a
__device__ __forceinline__ uint64_t tp_tiles(uint64_t a, uint64_t l) {
    return l ? ((a & (BRX_TP_ROW - 1u)) + l + BRX_TP_TILE - 1u) / BRX_TP_TILE : 0u;
}

// inclusive scan of one value per thread of a 1024-thread workgroup in `part` (1024 words of LDS): -> this thread's sum, part[1023] the total
__device__ __forceinline__ uint64_t tp_block_scan_1024(uint64_t *part, uint32_t t, uint64_t sum) {
    part[t] = sum;
    __syncthreads();
    for (uint32_t s = 1; s < 1024u; s <<= 1) {
        const uint64_t v = t >= s ? part[t - s] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    return part[t];
}

struct TpItem {
    uint32_t si;  // the stream
    uint64_t a;   // address of its first byte
    uint64_t e;   // one past its last
    uint64_t t0;  // address of the tile's first row (the stream starts up to 1023 bytes inside the first tile's)
    uint64_t t1;  // the tile's end, or the stream's
    uint32_t rows;
};

// the stream of an item: the last i < n with pre[i] <= item (streams without tiles share their successor's value and lose)
__device__ __forceinline__ uint32_t tp_stream_of(uint64_t item, uint32_t n, const uint64_t *__restrict__ pre) {
    uint32_t lo_i = 0, hi_i = n;
    while (hi_i - lo_i > 1u) {
        const uint32_t mid = lo_i + (hi_i - lo_i) / 2u;
        if (pre[mid] <= item) lo_i = mid; else hi_i = mid;
    }
    return lo_i;
}

// an item's stream and tile (all of it wave-uniform)
__device__ __forceinline__ TpItem tp_item(uint64_t item, const uint8_t *out, const uint64_t *__restrict__ out_off,
                                          const uint64_t *__restrict__ len, uint32_t n, const uint64_t *__restrict__ pre) {
    TpItem it;
    it.si = tp_stream_of(item, n, pre);
    it.a = (uint64_t)(uintptr_t)out + out_off[it.si];
    it.e = it.a + len[it.si];
    it.t0 = (it.a & ~(uint64_t)(BRX_TP_ROW - 1u)) + (item - pre[it.si]) * BRX_TP_TILE;
    it.t1 = it.t0 + BRX_TP_TILE < it.e ? it.t0 + BRX_TP_TILE : it.e;
    it.rows = (uint32_t)((it.t1 - it.t0 + BRX_TP_ROW - 1u) / BRX_TP_ROW);
    return it;
}

// the wave's next item: a load first (most waves end here, cheaply), the atomic only while there is something left
__device__ __forceinline__ uint64_t tp_next(unsigned long long *ticket, uint64_t grid_waves, uint64_t total, uint32_t lane) {
    unsigned long long next = 0;
    if (lane == 0u) {
        next = __hip_atomic_load(ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (grid_waves + next < total) next = atomicAdd(ticket, 1ull);
    }
    next = (unsigned long long)__shfl((long long)next, 0);
    return tp_uniform(grid_waves + next);
}

// the tiles a pass walks: those of the batch, but no more than its scratch has words for (more tiles than `span` allows: a caller's
// error, nothing is written for them)
__device__ __forceinline__ uint64_t tp_total(const uint64_t *__restrict__ pre, uint32_t n, uint64_t max_tiles) {
    return pre[n] < max_tiles ? pre[n] : max_tiles;
}

// A wave's walk over the items of a pass of BRX_TP_WG threads per workgroup:
//     for (TpWalk w = tp_walk(total); w.item < w.total; tp_advance(w, ticket)) { const TpItem it = tp_item(w.item, ...); ... }
struct TpWalk {
    uint32_t lane;
    uint64_t grid_waves;
    uint64_t total;
    uint64_t item; // (wave-uniform)
};

__device__ __forceinline__ TpWalk tp_walk(uint64_t total) {
    const uint32_t waves_per_wg = BRX_TP_WG / 64u;
    TpWalk w;
    w.lane = threadIdx.x & 63u;
    w.grid_waves = (uint64_t)gridDim.x * waves_per_wg;
    w.total = total;
    w.item = tp_uniform((uint64_t)blockIdx.x * waves_per_wg + (threadIdx.x >> 6));
    return w;
}

__device__ __forceinline__ void tp_advance(TpWalk &w, unsigned long long *ticket) {
    w.item = tp_next(ticket, w.grid_waves, w.total, w.lane);
}

// the sum of v over the wave's 64 lanes, in every lane
__device__ __forceinline__ uint32_t tp_wave_sum(uint32_t v) {
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v += (uint32_t)__shfl_xor((int)v, k);
    return v;
}

// thread t of a 1024-thread workgroup takes the tiles [i0, i1) of `total`: ceil(total / 1024) each, in order (thread 1023: i1 == total)
struct TpSlice {
    uint64_t i0, i1;
};

__device__ __forceinline__ TpSlice tp_slice_1024(uint64_t total, uint32_t t) {
    const uint64_t per = (total + 1023u) / 1024u;
    TpSlice s;
    s.i0 = per * t < total ? per * t : total;
    s.i1 = s.i0 + per < total ? s.i0 + per : total;
    return s;
}

// One row's entries.  m = the lane's 16-bit mask (bit k: byte k of its chunk is reported), base = the index of the row's first entry
// (wave-uniform, moved on to the next row's).  The entries are numbered in stream order by a wave prefix sum of the lanes' population
// counts (__shfl_up, no LDS memory); store(idx, k) is called for every set bit k whose index idx lies below pos_total.
template <class Store>
__device__ __forceinline__ void tp_emit_row(uint32_t m, uint32_t lane, uint64_t &base, uint64_t pos_total, Store store) {
    if (__ballot(m != 0u) == 0ull) return; // (uniform) a row without one: no position work
    const uint32_t c = (uint32_t)__popc(m);
    uint32_t incl = c;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, s);
        if (lane >= (uint32_t)s) incl += up;
    }
    uint64_t idx = base + (incl - c);
    while (m) {
        const uint32_t k = (uint32_t)__ffs((int)m) - 1u;
        m &= m - 1u;
        if (idx < pos_total) store(idx, k);
        idx++;
    }
    base += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
}
#endif
