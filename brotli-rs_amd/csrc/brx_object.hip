// brx_object.hip -- brx_object_batch: the named members of the nested JSON objects that a selection of openers names, as selections
// for the record calls, and the extent of every object.  The rule's arithmetic, the lane path and one lane's share of the wave path
// are plain C++ in brx_object.h, shared with tools/object_emu.cpp.  This file holds what is HIP: the memory policy, the ballot over the
// long objects, the scan across the wave, the ballots that find a row's last match per name, the carries from row to row and the
// launch.  What the record kernels share on the device is brx_record_dev.h.
//
// One lane owns one entry.  An object that ends within BRX_OB_LONG boundaries behind its opener is walked by its lane alone.  The
// lanes with longer objects leave them; the wave then takes those one at a time in a wave-uniform loop over their ballot, lane l on
// unit l of a row of BRX_OB_ROW boundaries.  Last wins without atomics: an entry belongs to one wave, its rows run in order, per name
// and row one ballot finds the last lane with a match, and lane q carries name q's winner from row to row.  Every slot of entry j is
// stored by the thread of entry j alone (brx_object.h, WHO STORES).  No scratch, no atomics, no LDS.
#include "brx_record_dev.h"
#include "brx_object.h"

struct BrxObMem : BrxRecMem {
    __device__ __forceinline__ uint8_t ldw8(const uint8_t *p) { return *p; }
    __device__ __forceinline__ BrxTake128 ldw128(const uint8_t *p) { return ld128(p); }
    __device__ __forceinline__ void st64(uint64_t *p, uint64_t v) { *p = v; }
    __device__ __forceinline__ void st32(uint32_t *p, uint32_t v) { *p = v; }
};

// inclusive scan of x over the lanes
__device__ __forceinline__ int32_t brx_ob_wave_scan(int32_t x, uint32_t lane) {
    for (int st = 1; st < 64; st <<= 1) {
        const int32_t y = __shfl_up(x, st, 64);
        if (lane >= (uint32_t)st) x += y;
    }
    return x;
}

// the sum of x over the lanes, in every lane: a butterfly, once per long object
__device__ __forceinline__ uint64_t brx_ob_wave_sum(uint64_t x) {
    for (int st = 1; st < 64; st <<= 1) x += (uint64_t)__shfl_xor((unsigned long long)x, st, 64);
    return x;
}

// x of lane `src` in every lane, in a vector register
__device__ __forceinline__ uint64_t brx_ob_from(uint64_t x, uint32_t src) { return (uint64_t)__shfl((unsigned long long)x, (int)src, 64); }

#define BRX_OB_DEAD 0xFFu // the status of a lane behind m, in the kernel only

template <bool NAMES>
__global__ __launch_bounds__(BRX_REC_BLOCK) void brx_object_kernel(BrxObArgs x, BrxMbNames nm) {
    // every lane stays to the end: the loop over the long objects needs the whole wave
    const uint64_t j = brx_rec_entry();
    const uint32_t lane = threadIdx.x & 63u;
    BrxObMem mem;
    BrxObRes res = {0, ~(uint64_t)0, BRX_OB_DEAD, 0};
    bool is_long = false;
    BrxObEntry mine = {BRX_OB_NONE, 0, 0, 0, 0};
    if (j < x.a.m) {
        mine = brx_ob_entry(mem, x, j);
        res.status = mine.status; // (from here on not BRX_OB_DEAD: the lane has an entry)
    }
    // (one after the other, not nested: every level of nesting around the lane path holds a lane mask in two scalar registers)
    if (res.status == BRX_OB_OK) is_long = !brx_ob_lane<NAMES>(mem, x, nm, mine, j, res);
    if (NAMES && (res.status == BRX_OB_NONE || res.status == BRX_OB_NOT_OBJECT)) brx_ob_store_missing(mem, x, nm.n, j);
    uint64_t todo = __ballot(is_long);
    while (todo) { // (wave-uniform)
        const uint32_t owner = (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1u;
        // the owner's entry in every lane, in vector registers: the addresses that it goes into are formed there anyway, and the
        // scalar side has none to spare
        BrxObEntry en;
        en.status = BRX_OB_OK;
        en.r = brx_ob_from(mine.r, owner);
        en.i = (uint32_t)__shfl((int)mine.i, (int)owner, 64);
        en.c = brx_ob_from(mine.c, owner); en.base = brx_ob_from(mine.base, owner);
        int64_t depth = 1;     // in front of the row
        uint64_t members = 0;  // this lane's, so far: summed over the lanes behind the last row
        uint32_t flags = 0;    // this lane's keys'
        uint64_t best = 0;     // lane q: k + 1 of the last member so far that carries name q, or 0
        for (uint64_t kb = en.r + 1u;; kb += BRX_OB_ROW) {
            const uint64_t k0 = kb + lane * BRX_MB_UNIT;
            const uint32_t nv = brx_mb_valid(en.c, k0);
            const BrxTake128 v = brx_el_unit(mem, x.what, en.base, en.c, k0, nv);
            const BrxElMasks k = brx_ob_masks(v);
            const int32_t sum = brx_el_unit_sum(k), incl = brx_ob_wave_scan(sum, lane);
            BrxElUnit u = brx_el_unit_walk(k, nv, brx_el_depth(depth, incl - sum));
            const uint64_t stops = __ballot(u.stop != BRX_EL_STOP_NONE);
            const uint32_t sl = stops ? (uint32_t)__builtin_ctzll(stops) : 64u;
            if (lane > sl) u.sep = 0; // behind the stop nothing counts
            members += (uint32_t)__builtin_popcount(u.sep);
            if (NAMES) {
                uint64_t last = 0;
                if (u.sep) flags |= brx_ob_unit_keys(mem, x, nm, en.i, k0, u.sep, 0u, last);
#pragma unroll 1
                for (uint32_t q = 0; q < nm.n; q++) { // per name: the row's last lane with a match, and in it the unit's last
                    const uint32_t lb = brx_ob_last_of(last, q);
                    const uint64_t hit = __ballot(lb != 0);
                    if (hit) {
                        const uint32_t ll = 63u - (uint32_t)__builtin_clzll(hit);
                        const uint64_t win = kb + ll * BRX_MB_UNIT + brx_rec_bcast32(lb, ll); // (k + 1: the field holds the bit + 1)
                        if (lane == q) best = win;
                    }
                }
            }
            if (stops) {
                const uint32_t at = brx_rec_bcast32(u.at, sl), how = brx_rec_bcast32(u.stop, sl);
                members = brx_ob_wave_sum(members);
                if (NAMES) flags = (__ballot(flags & BRX_MB_F_LONG_KEY) ? BRX_MB_F_LONG_KEY : 0u) | (__ballot(flags & BRX_MB_F_ESCAPED_KEY) ? BRX_MB_F_ESCAPED_KEY : 0u);
                if (lane == owner) {
                    res.n_members = members;
                    res.end = kb + sl * BRX_MB_UNIT + at;
                    res.status = how == BRX_EL_STOP_OK ? BRX_OB_OK : how == BRX_EL_STOP_MISMATCH ? BRX_OB_MISMATCH : BRX_OB_UNCLOSED;
                    res.flags = flags;
                }
                break;
            }
            depth += __shfl(incl, 63, 64); // (the row's sum, in a vector register like the depth)
        }
        if (NAMES) { // the owner's thread stores every slot of its entry (its lane path stored none)
#pragma unroll 1
            for (uint32_t q = 0; q < nm.n; q++) {
                const uint64_t win = brx_rec_bcast(best, q);
                if (lane == owner) brx_ob_store_slot(mem, x, &mine, q, j, win);
            }
        }
    }
    if (res.status != BRX_OB_DEAD) { // (j < m, held in a vector register: as a lane mask it cost two scalar registers across the kernel)
        if (x.n_members) x.n_members[j] = res.n_members;
        if (x.status) x.status[j] = (uint8_t)res.status;
        if (x.end) x.end[j] = res.end;
        if (NAMES && x.obj_flags) x.obj_flags[j] = (uint8_t)res.flags;
    }
}

void brx_launch_object(const BrxObArgs &x, const BrxMbNames &nm, void *hip_stream) {
    if (x.a.m == 0) return;
    const dim3 grid(brx_rec_blocks(x.a.m)), block(BRX_REC_BLOCK);
    if (nm.n) hipLaunchKernelGGL(brx_object_kernel<true>, grid, block, 0, (hipStream_t)hip_stream, x, nm);
    else hipLaunchKernelGGL(brx_object_kernel<false>, grid, block, 0, (hipStream_t)hip_stream, x, nm);
}
