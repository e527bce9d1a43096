// brx_hash.hip -- brx_hash_batch: a 64-bit key of every selected record of the decoded streams of a batch.  The arithmetic, the lane
// path and one lane's share of the wave path are plain C++ in brx_hash.h, shared with tools/hash_emu.cpp; the record rule is that of
// brx_take.h.  This file holds what is HIP and its own: the ballot over the long records, the sums across the wave and the launch.  What
// the record kernels share on the device is brx_record_dev.h.
//
// One lane owns one entry.  A record shorter than BRX_HASH_LONG is hashed by its lane alone, unit by unit.  The lanes with longer records
// leave them out; the wave then takes those one at a time in a wave-uniform loop over their ballot, lane l on unit 64 row + l, so that
// no lane ever runs through more than a row's worth of units alone.  No scratch, no atomics, no LDS; the row sums go by shuffles.
#include "brx_record_dev.h"
#include "brx_hash.h"

// the sum of x over the 64 lanes mod p (below 2^61 + 4), in every lane
__device__ __forceinline__ uint64_t brx_hash_wave_sum(uint64_t x) {
    for (int d = 32; d > 0; d >>= 1) x = brx_hash_add(x, (uint64_t)__shfl_xor((unsigned long long)x, d, 64));
    return x;
}

// The lane path alone fits 7 waves per SIMD; the loop over the long records, whose group of loads would take the kernel to 102 VGPRs
// and 4 waves, is held to the same budget (70 VGPRs, no spill: -Rpass-analysis=kernel-resource-usage).
__global__ __launch_bounds__(BRX_REC_BLOCK) __attribute__((amdgpu_waves_per_eu(7, 7))) void brx_hash_kernel(BrxTakeArgs a, BrxHashKeys k, uint64_t *__restrict__ hash, uint64_t *__restrict__ rec_len) {
    // every lane stays to the end: the loop over the long records needs the whole wave
    const uint64_t j = brx_rec_entry();
    const uint32_t lane = threadIdx.x & 63u;
    BrxRecMem mem;
    BrxTakeRec r = {0, 0};
    if (j < a.m) r = brx_take_entry_record(mem, a, j);
    const bool is_long = r.len >= BRX_HASH_LONG;
    uint64_t h = 0;
    if (!is_long) h = brx_hash_lane(mem, a.out, a.span, r, k);
    uint64_t todo = __ballot(is_long);
    if (todo) { // (wave-uniform)
        const uint64_t w = brx_hash_lane_weight(k, lane), kg = brx_hash_group_stride(k);
        while (todo) {
            const uint32_t owner = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1u;
            const uint64_t src = brx_rec_bcast(r.src, owner), L = brx_rec_bcast(r.len, owner);
            const BrxHashShape s = brx_hash_shape(L);
            uint64_t acc = 0;
            uint64_t row = 0;
            for (; row + BRX_HASH_GROUP < s.rows; row += BRX_HASH_GROUP) { // whole rows in front of the last one, a group at a time
                const uint64_t sum = brx_hash_wave_sum(brx_hash_group_term(mem, a.out, src, row, lane, w, k));
                acc = brx_hash_red(brx_hash_mul(acc, kg) + brx_hash_red(sum));
            }
            for (; row + 1u < s.rows; row++) {
                const uint64_t sum = brx_hash_wave_sum(brx_hash_row_term(mem, a.out, a.span, src, row, lane, w, k));
                acc = brx_hash_red(brx_hash_mul(acc, k.k256) + brx_hash_red(sum));
            }
            const uint64_t wl = (uint64_t)__shfl((unsigned long long)w, (int)brx_hash_last_weight_lane(lane, s.nu), 64);
            BrxTake128 v;
            const uint64_t X = brx_hash_red(brx_hash_wave_sum(brx_hash_last_term(mem, a.out, a.span, src, s, lane, wl, acc, k, v)));
            const uint64_t S = brx_rec_bcast(brx_hash_tail(X, v, s.n, k), s.nu - 1u); // (the last unit is lane nu - 1's)
            if (lane == owner) h = brx_hash_finish(S, L);
        }
    }
    if (j < a.m) {
        hash[j] = h;
        if (rec_len) rec_len[j] = r.len;
    }
}

void brx_launch_hash(const BrxTakeArgs &a, const BrxHashKeys &k, uint64_t *hash, uint64_t *rec_len, void *hip_stream) {
    if (a.m == 0) return;
    hipLaunchKernelGGL(brx_hash_kernel, dim3(brx_rec_blocks(a.m)), dim3(BRX_REC_BLOCK), 0, (hipStream_t)hip_stream, a, k, hash, rec_len);
}
