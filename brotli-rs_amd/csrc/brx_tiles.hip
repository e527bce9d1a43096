// brx_tiles.hip -- the plan kernel of the tile pass (brx_tiles.h): one workgroup, first launch of brx_digest_batch, brx_index_batch and
// brx_index_quoted_batch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "brx_tiles.h"

// Every thread takes a slice of ceil(n / 1024) streams: tiles per stream, their exclusive prefix sum pre[0 .. n], `w` words per stream
// cleared at `clear`, both ticket counters cleared.
__global__ __launch_bounds__(1024) void brx_tile_plan_kernel(const uint8_t *out, const uint64_t *__restrict__ out_off,
                                                             const uint64_t *__restrict__ len, uint32_t n, uint64_t *__restrict__ pre,
                                                             uint32_t *__restrict__ clear, uint32_t w, unsigned long long *ticket_a,
                                                             unsigned long long *ticket_b) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint64_t per = ((uint64_t)n + 1023u) / 1024u;
    const uint64_t i0 = per * t < n ? per * t : n, i1 = i0 + per < n ? i0 + per : n;
    uint64_t sum = 0;
    for (uint64_t i = i0; i < i1; i++) sum += tp_tiles((uint64_t)(uintptr_t)out + out_off[i], len[i]);
    uint64_t run = tp_block_scan_1024(part, t, sum) - sum;
    for (uint64_t i = i0; i < i1; i++) {
        pre[i] = run;
        for (uint32_t k = 0; k < w; k++) clear[i * w + k] = 0u;
        run += tp_tiles((uint64_t)(uintptr_t)out + out_off[i], len[i]);
    }
    if (t == 1023u) {
        pre[n] = part[1023];
        *ticket_a = 0ull;
        *ticket_b = 0ull;
    }
}

void brx_launch_tile_plan(const void *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, void *scratch, uint32_t *clear,
                          uint32_t w, void *hip_stream) {
    hipLaunchKernelGGL(brx_tile_plan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)hip_stream, (const uint8_t *)out, out_off, len, n,
                       brx_tp_pre(scratch), clear, w, brx_tp_ticket_a(scratch), brx_tp_ticket_b(scratch));
}
