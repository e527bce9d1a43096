// brx_take.hip -- brx_take_batch: the selected records of the decoded streams of a batch, as lengths (size kernel) or as bytes in a
// destination (fill kernel).  The rule, the descriptor of an entry and the assembly of a destination unit are plain C++ in brx_take.h,
// shared with tools/take_emu.cpp; this file holds what is HIP and its own: the descriptor window in LDS and the launches.  What the
// record kernels share on the device is brx_record_dev.h.
//
// Size kernel: one thread per selection entry.
// Fill kernel: DESTINATION-centric, so its cost does not depend on how small the records are.  One wavefront (a workgroup of its own,
// so that the barrier around the LDS window is the wave's) owns one BRX_TAKE_CHUNK of the destination's address range, cut at 16-byte
// aligned addresses.  It finds the chunk's first entry by a wave-uniform binary search in dst_off (scalar loads), computes 64
// descriptors at a time, one per lane, into LDS, and every lane assembles one 16-byte unit per 1 KiB row from the entries the unit
// spans: one aligned dwordx4 store where the unit is covered, byte stores where it is not.  Source bytes come by unaligned 16-byte
// loads wherever those lie inside the arena.  A chunk in which more than 64 entries start refills the window; a record longer than a
// chunk is served by several waves independently.  No scratch, no atomics, no inter-workgroup traffic.
#include "brx_record_dev.h"

__global__ __launch_bounds__(BRX_REC_BLOCK) void brx_take_size_kernel(BrxTakeArgs a, uint64_t *__restrict__ rec_len) {
    const uint64_t j = brx_rec_entry();
    if (j >= a.m) return;
    BrxRecMem mem;
    rec_len[j] = brx_take_entry_record(mem, a, j).len;
}

__global__ __launch_bounds__(64) void brx_take_fill_kernel(BrxTakeArgs a, const uint64_t *__restrict__ dst_off, uint8_t *dst,
                                                           uint64_t total) {
    __shared__ uint64_t w_start[BRX_TAKE_WINDOW], w_src[BRX_TAKE_WINDOW], w_cnt[BRX_TAKE_WINDOW];
    BrxRecMemAligned mem; // (a unit goes out at a 16-byte aligned address)
    const uint32_t lane = threadIdx.x;
    const uint32_t phase = (uint32_t)((uintptr_t)dst & 15u);
    uint8_t *dst_al = dst - phase;
    // this wave's chunk, in y = index + phase
    const uint64_t c0 = (uint64_t)blockIdx.x * BRX_TAKE_CHUNK;
    const uint64_t end = total + phase;
    uint64_t g = c0 > phase ? c0 : phase;
    const uint64_t hi = c0 + BRX_TAKE_CHUNK < end ? c0 + BRX_TAKE_CHUNK : end;
    if (g >= hi) return;
    // the entry owning the chunk's first byte: the last j with dst_off[j] + phase <= g (wave-uniform: scalar loads)
    uint64_t lo = 0, top = a.m;
    while (top - lo > 1u) {
        const uint64_t mid = lo + (top - lo) / 2u;
        if (dst_off[mid] + phase <= g) lo = mid; else top = mid;
    }
    uint64_t jw = lo;
    while (g < hi) {
        __syncthreads(); // (one wave per workgroup) the units of the previous window are done with LDS
        const BrxTakeDesc d = brx_take_descriptor(mem, a, dst_off, total, phase, jw + lane);
        w_start[lane] = d.start;
        w_src[lane] = d.src;
        w_cnt[lane] = d.cnt;
        __syncthreads();
        const uint64_t next_start = jw + BRX_TAKE_WINDOW < a.m ? dst_off[jw + BRX_TAKE_WINDOW] + phase : BRX_TAKE_NONE;
        uint64_t wend, jnext;
        brx_take_window_end(w_start, g, hi, next_start, jw, wend, jnext);
        if (wend > g) {
            const uint32_t r0 = (uint32_t)((g - c0) / BRX_TAKE_ROW), r1 = (uint32_t)((wend - 1u - c0) / BRX_TAKE_ROW);
            for (uint32_t r = r0; r <= r1; r++)
                brx_take_unit(mem, w_start, w_src, w_cnt, c0 + (uint64_t)r * BRX_TAKE_ROW + lane * BRX_TAKE_UNIT, g, wend, a.out, a.span,
                              dst_al);
        }
        g = wend;
        jw = jnext;
    }
}

void brx_launch_take_size(const BrxTakeArgs &a, uint64_t *rec_len, void *hip_stream) {
    if (a.m == 0) return;
    hipLaunchKernelGGL(brx_take_size_kernel, dim3(brx_rec_blocks(a.m)), dim3(BRX_REC_BLOCK), 0, (hipStream_t)hip_stream, a, rec_len);
}

void brx_launch_take_fill(const BrxTakeArgs &a, const uint64_t *dst_off, uint8_t *dst, uint64_t total, void *hip_stream) {
    const uint64_t chunks = brx_take_chunks(total, dst);
    if (chunks == 0) return;
    hipLaunchKernelGGL(brx_take_fill_kernel, dim3((unsigned)chunks), dim3(64), 0, (hipStream_t)hip_stream, a, dst_off, dst, total);
}
