// brx_elements.hip -- brx_elements_batch: the elements of the JSON arrays that a selection of openers names, as a selection for the
// record calls.  The rule's arithmetic, the lane path and one lane's share of the wave path are plain C++ in brx_elements.h, shared with
// tools/elements_emu.cpp.  This file holds what is HIP: the memory policy, the ballot over the long arrays, the scans across the wave,
// the carries from row to row and the launch.  What the record kernels share on the device is brx_record_dev.h.
//
// One lane owns one entry.  An array that ends within BRX_EL_LONG boundaries behind its opener is walked by its lane alone.  The lanes
// with longer arrays leave them; the wave then takes those one at a time in a wave-uniform loop over their ballot, lane l on unit l of
// a row of BRX_EL_ROW boundaries, so that no lane ever walks more than BRX_EL_LONG boundaries alone.  No scratch, no atomics, no LDS.
#include "brx_record_dev.h"
#include "brx_elements.h"

struct BrxElMem : BrxRecMem {
    __device__ __forceinline__ uint8_t ldw8(const uint8_t *p) { return *p; }
    __device__ __forceinline__ BrxTake128 ldw128(const uint8_t *p) { return ld128(p); }
    __device__ __forceinline__ void st64(uint64_t *p, uint64_t v) { *p = v; }
    __device__ __forceinline__ void st32(uint32_t *p, uint32_t v) { *p = v; }
};

// inclusive scan of x over the lanes
__device__ __forceinline__ int32_t brx_el_wave_scan(int32_t x, uint32_t lane) {
    for (int st = 1; st < 64; st <<= 1) {
        const int32_t y = __shfl_up(x, st, 64);
        if (lane >= (uint32_t)st) x += y;
    }
    return x;
}

// x of lane `src` in every lane, in a vector register
__device__ __forceinline__ uint64_t brx_el_from(uint64_t x, uint32_t src) { return (uint64_t)__shfl((unsigned long long)x, (int)src, 64); }

template <bool FILL>
__global__ __launch_bounds__(BRX_REC_BLOCK) void brx_elements_kernel(BrxElArgs x) {
    // every lane stays to the end: the loop over the long arrays needs the whole wave
    const uint64_t j = brx_rec_entry();
    const uint32_t lane = threadIdx.x & 63u;
    BrxElMem mem;
    BrxElRes res = {0, ~(uint64_t)0, BRX_EL_NONE};
    bool is_long = false;
    BrxElEntry mine = {BRX_EL_NONE, 0, 0, 0, 0, 0, 0};
    if (j < x.a.m) {
        mine = brx_el_entry(mem, x, j);
        res.status = mine.status;
        if (mine.status == BRX_EL_OK) is_long = !brx_el_lane<FILL>(mem, x, mine, res);
    }
    uint64_t todo = __ballot(is_long);
    while (todo) { // (wave-uniform)
        const uint32_t owner = (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1u;
        // the owner's entry in every lane: the opener as a scalar (the rows count from it), the rest in vector registers, where the
        // addresses and the bounds that they go into are formed anyway (as scalars they cost the loop 9 scalar registers it has not got)
        BrxElEntry en;
        en.status = BRX_EL_OK;
        en.r = brx_rec_bcast(mine.r, owner);
        en.i = (uint32_t)__shfl((int)mine.i, (int)owner, 64);
        en.c = brx_el_from(mine.c, owner); en.base = brx_el_from(mine.base, owner);
        en.off = brx_el_from(mine.off, owner); en.lim = brx_el_from(mine.lim, owner);
        int64_t depth = 1;             // in front of the row
        uint64_t seps = 0, pend = en.r; // separators so far (the opener apart); the last one, whose element nothing has ended yet
        for (uint64_t kb = en.r + 1u;; kb += BRX_EL_ROW) {
            const uint64_t k0 = kb + lane * BRX_MB_UNIT;
            const uint32_t nv = brx_mb_valid(en.c, k0);
            const BrxTake128 v = brx_el_unit(mem, x.what, en.base, en.c, k0, nv);
            const BrxElMasks k = brx_el_masks(v);
            const int32_t sum = brx_el_unit_sum(k), incl = brx_el_wave_scan(sum, lane);
            BrxElUnit u = brx_el_unit_walk(k, nv, brx_el_depth(depth, incl - sum));
            const uint64_t stops = __ballot(u.stop != BRX_EL_STOP_NONE);
            const uint32_t sl = stops ? (uint32_t)__builtin_ctzll(stops) : 64u;
            if (lane > sl) u.sep = 0;
            const int32_t cl = __builtin_popcount(u.sep), cincl = brx_el_wave_scan(cl, lane);
            const uint64_t with = __ballot(cl != 0);
            const uint32_t how = stops ? brx_rec_bcast32(u.stop, sl) : BRX_EL_STOP_NONE;
            const bool closed = how == BRX_EL_STOP_OK || how == BRX_EL_STOP_MISMATCH;
            if (FILL) {
                if ((with || closed) && lane == 0u) brx_el_store_at(mem, x, en, seps, pend);
                const bool later = closed || (lane < 63u && (with >> (lane + 1u)) != 0);
                brx_el_unit_store(mem, x, en, k0, v, u.sep, seps + 1u + (uint32_t)(cincl - cl), later);
            }
            if (with) {
                const uint32_t ll = 63u - (uint32_t)__builtin_clzll(with);
                pend = kb + ll * BRX_MB_UNIT + (31u - (uint32_t)__builtin_clz(brx_rec_bcast32(u.sep, ll)));
            }
            seps += brx_rec_bcast32((uint32_t)cincl, 63u);
            if (stops) {
                const uint32_t at = brx_rec_bcast32(u.at, sl);
                if (lane == owner) {
                    res.n_elem = seps + (closed ? 1u : 0u);
                    res.end = kb + sl * BRX_MB_UNIT + at;
                    res.status = how == BRX_EL_STOP_OK ? BRX_EL_OK : how == BRX_EL_STOP_MISMATCH ? BRX_EL_MISMATCH : BRX_EL_UNCLOSED;
                }
                break;
            }
            depth += (int32_t)brx_rec_bcast32((uint32_t)incl, 63u);
        }
    }
    if (j < x.a.m) {
        if (x.n_elem) x.n_elem[j] = res.n_elem;
        if (x.status) x.status[j] = (uint8_t)res.status;
        if (x.end) x.end[j] = res.end;
    }
}

void brx_launch_elements(const BrxElArgs &x, void *hip_stream) {
    if (x.a.m == 0) return;
    const dim3 grid(brx_rec_blocks(x.a.m)), block(BRX_REC_BLOCK);
    if (x.el_off) hipLaunchKernelGGL(brx_elements_kernel<true>, grid, block, 0, (hipStream_t)hip_stream, x);
    else hipLaunchKernelGGL(brx_elements_kernel<false>, grid, block, 0, (hipStream_t)hip_stream, x);
}
