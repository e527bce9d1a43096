// brx_member.hip -- brx_member_batch: the named members of the JSON Lines objects of a batch as selections for the record calls.  The
// rule's arithmetic (the summary of a unit of boundaries, how summaries join, the walk of a unit, the look at a key record, the last
// step) is plain C++ in brx_member.h, shared with tools/member_emu.cpp.  This file holds what is HIP: the memory policy, the scan of
// the lanes' summaries across the wave, the scan of the tiles' summaries by one workgroup, and the launches.
//
// A work item is one (stream, tile) pair, a tile = BRX_MB_TILE boundaries of the stream, taken by one wave in rows of BRX_MB_ROW, 16
// bytes of `what` per lane.  The host knows n and n_pos, so an upper bound of the tiles is known without a read-back: the grids cover
// the bound, and a wave behind the real number of tiles (pre[n], written by the plan kernel) ends at once.  No LDS outside the compose
// kernel, no scratch; the only atomics are the two that settle a slot (brx_member.h).
#include "brx_record_dev.h"
#include "brx_member.h"

struct BrxMbMem : BrxRecMem {
    __device__ __forceinline__ uint8_t ldw8(const uint8_t *p) { return *p; }
    __device__ __forceinline__ BrxTake128 ldw128(const uint8_t *p) { return ld128(p); }
    __device__ __forceinline__ void max64(uint64_t *p, uint64_t v) { (void)atomicMax((unsigned long long *)p, (unsigned long long)v); }
    __device__ __forceinline__ void or32(uint32_t *p, uint32_t v) { (void)atomicOr(p, v); }
    __device__ __forceinline__ uint64_t get64(const uint64_t *p) { return *p; }
    __device__ __forceinline__ uint32_t get32(const uint32_t *p) { return *p; }
    __device__ __forceinline__ void st64(uint64_t *p, uint64_t v) { *p = v; }
    __device__ __forceinline__ void st32(uint32_t *p, uint32_t v) { *p = v; }
};

// Every thread takes a slice of ceil(n / 1024) streams: tiles per stream and their exclusive prefix sum pre[0 .. n], cut at max_tiles
// (counts that are not what pos_off sums lose tiles there, never the scratch its bounds).
__global__ __launch_bounds__(1024) void brx_member_plan_kernel(BrxMbArgs x) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x, n = x.a.n;
    const uint64_t per = ((uint64_t)n + 1023u) / 1024u;
    const uint64_t i0 = per * t < n ? per * t : n, i1 = i0 + per < n ? i0 + per : n;
    uint64_t sum = 0;
    for (uint64_t i = i0; i < i1; i++) sum += brx_mb_tiles(brx_mb_count(x.a, i));
    part[t] = sum;
    __syncthreads();
    for (uint32_t s = 1; s < 1024u; s <<= 1) {
        const uint64_t v = t >= s ? part[t - s] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t run = part[t] - sum;
    for (uint64_t i = i0; i < i1; i++) {
        x.pre[i] = run < x.max_tiles ? run : x.max_tiles;
        run += brx_mb_tiles(brx_mb_count(x.a, i));
    }
    if (t == 1023u) x.pre[n] = part[1023] < x.max_tiles ? part[1023] : x.max_tiles;
}

// inclusive scan of the lanes' summaries (rd is nl != 0: two values travel)
__device__ __forceinline__ BrxMbSum brx_mb_wave_scan(BrxMbSum s, uint32_t lane) {
    for (int st = 1; st < 64; st <<= 1) {
        BrxMbSum y;
        y.nl = (uint32_t)__shfl_up((int)s.nl, st, 64);
        y.d = __shfl_up(s.d, st, 64);
        y.rd = y.nl ? 1u : 0u;
        if (lane >= (uint32_t)st) s = brx_mb_join(y, s);
    }
    return s;
}

// One wave, one tile.  EMIT = false: the tile's summary to x.sum.  EMIT = true: every unit walked, with x.in in front of the tile.
template <bool EMIT>
__global__ __launch_bounds__(BRX_REC_BLOCK) void brx_member_kernel(BrxMbArgs x, BrxMbNames nm) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t t = (uint64_t)blockIdx.x * (BRX_REC_BLOCK / 64u) + (threadIdx.x >> 6);
    if (t >= x.pre[x.a.n]) return; // (wave-uniform)
    BrxMbMem mem;
    const uint32_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)brx_mb_tile_stream(x.pre, x.a.n, t));
    const uint64_t c = brx_mb_count(x.a, i), base = x.a.pos_off[i], kt = (t - x.pre[i]) * BRX_MB_TILE;
    BrxMbSeg in = {0, 0, 0};
    if (EMIT) in = x.in[t];
    BrxMbSum carry = {0, 0, 0};
    for (uint32_t row = 0; row < BRX_MB_TILE / BRX_MB_ROW && kt + row * BRX_MB_ROW < c; row++) {
        const uint64_t k0 = kt + row * BRX_MB_ROW + lane * BRX_MB_UNIT;
        const uint32_t nv = brx_mb_valid(c, k0);
        const BrxMbMasks k = brx_mb_masks(brx_mb_unit(mem, x.what, base + k0, nv));
        const BrxMbSum incl = brx_mb_wave_scan(brx_mb_unit_sum(k), lane);
        if (EMIT) {
            BrxMbSum ex;
            ex.nl = (uint32_t)__shfl_up((int)incl.nl, 1, 64);
            ex.d = __shfl_up(incl.d, 1, 64);
            if (lane == 0u) { ex.nl = 0; ex.d = 0; }
            ex.rd = ex.nl ? 1u : 0u;
            const BrxMbSum st = brx_mb_join(carry, ex);
            brx_mb_walk(mem, x, nm, i, c, k0, nv, k, in.L + st.nl, st.rd ? st.d : in.d + st.d);
        }
        BrxMbSum last;
        last.nl = brx_rec_bcast32(incl.nl, 63u);
        last.d = (int32_t)brx_rec_bcast32((uint32_t)incl.d, 63u);
        last.rd = last.nl ? 1u : 0u;
        carry = brx_mb_join(carry, last);
    }
    if (!EMIT && lane == 0u) x.sum[t] = carry;
}

// The scan of the tiles' summaries in tile order, restarted in front of every stream's first tile: x.in[t], and lines[i].  Every
// thread takes a slice of ceil(tiles / 1024) tiles; a thread reads back from memory only what it wrote itself.
__global__ __launch_bounds__(1024) void brx_member_compose_kernel(BrxMbArgs x) {
    __shared__ BrxMbSeg part[1024];
    const uint32_t th = threadIdx.x, n = x.a.n;
    const uint64_t nt = x.pre[n], per = (nt + 1023u) / 1024u;
    const uint64_t t0 = per * th < nt ? per * th : nt, t1 = t0 + per < nt ? t0 + per : nt;
    BrxMbSeg acc = {0, 0, 0};
    uint32_t s0 = 0;
    if (t0 < t1) {
        uint32_t si = s0 = brx_mb_tile_stream(x.pre, n, t0);
        for (uint64_t t = t0; t < t1; t++) {
            while (t >= x.pre[si + 1u]) si++;
            if (t == x.pre[si]) acc = brx_mb_seg_join(acc, brx_mb_seg_start());
            x.in[t] = acc;
            acc = brx_mb_seg_join(acc, brx_mb_seg_of(x.sum[t]));
        }
    }
    part[th] = acc;
    __syncthreads();
    for (uint32_t s = 1; s < 1024u; s <<= 1) {
        BrxMbSeg v = part[th];
        if (th >= s) v = brx_mb_seg_join(part[th - s], v);
        __syncthreads();
        part[th] = v;
        __syncthreads();
    }
    BrxMbSeg pfx = {0, 0, 0};
    if (th) pfx = part[th - 1u];
    if (t0 < t1) {
        uint32_t si = s0;
        for (uint64_t t = t0; t < t1; t++) {
            while (t >= x.pre[si + 1u]) si++;
            const BrxMbSeg in = brx_mb_seg_join(pfx, x.in[t]);
            x.in[t] = in;
            if (t + 1u == x.pre[si + 1u]) { // the stream's last tile
                const uint64_t l = in.L + x.sum[t].nl + 1u;
                x.slines[si] = l;
                if (x.lines) x.lines[si] = l;
            }
        }
    }
    for (uint32_t i = th; i < n; i += 1024u) {
        if (x.pre[i] == x.pre[i + 1u]) { // no boundary that counts: one line
            x.slines[i] = 1u;
            if (x.lines) x.lines[i] = 1u;
        }
    }
}

__global__ __launch_bounds__(BRX_REC_BLOCK) void brx_member_finish_kernel(BrxMbArgs x, uint32_t n_names) {
    const uint64_t j = brx_rec_entry();
    BrxMbMem mem;
    if (j < x.m) brx_mb_finish(mem, x, n_names, j);
}

void brx_launch_member(BrxMbArgs x, const BrxMbNames &nm, void *scratch, void *hip_stream) {
    hipStream_t st = (hipStream_t)hip_stream;
    const uint32_t n = x.a.n;
    x.pre = (uint64_t *)scratch;
    x.slines = x.pre + (size_t)n + 1u;
    x.in = (BrxMbSeg *)(x.slines + n);
    x.sum = (BrxMbSum *)(x.in + x.max_tiles);
    const bool fill = x.kind != nullptr && x.m > 0;
    if (fill) { // the slots while they are being settled: 0 = no member yet, no flag yet
        (void)hipMemsetAsync(x.sel_rec, 0, (size_t)nm.n * x.m * 8u, st);
        (void)hipMemsetAsync(x.sel_stream, 0, (size_t)x.m * 4u, st);
    }
    const dim3 tiles((unsigned)((x.max_tiles + BRX_REC_BLOCK / 64u - 1u) / (BRX_REC_BLOCK / 64u))), block(BRX_REC_BLOCK);
    hipLaunchKernelGGL(brx_member_plan_kernel, dim3(1), dim3(1024), 0, st, x);
    hipLaunchKernelGGL(brx_member_kernel<false>, tiles, block, 0, st, x, nm);
    hipLaunchKernelGGL(brx_member_compose_kernel, dim3(1), dim3(1024), 0, st, x);
    if (fill) {
        hipLaunchKernelGGL(brx_member_kernel<true>, tiles, block, 0, st, x, nm);
        hipLaunchKernelGGL(brx_member_finish_kernel, dim3(brx_rec_blocks(x.m)), block, 0, st, x, nm.n);
    }
}
