// brx_parse.hip -- brx_parse_batch: every selected record of the decoded streams of a batch as a 64-bit number and a status byte.
// The fetch, the classification, the grammar and the conversion are plain C++ in brx_parse.h, shared with tools/parse_emu.cpp; the
// record rule is that of brx_take.h.  This file holds what is HIP: the memory policy, the kernel and the launch.
//
// One lane owns one entry and needs no other lane: a record above 64 bytes is answered from its length alone, so no lane runs through
// more than four 16-byte units.  No scratch, no atomics, no LDS; the status goes out as a byte store, the value as a qword store.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "brx_parse.h"

struct __attribute__((packed, aligned(1))) brx_parse_u128u { uint32_t w[4]; };

struct BrxParseDevMem {
    __device__ __forceinline__ uint8_t ld8(const uint8_t *p) { return *p; }
    __device__ __forceinline__ BrxTake128 ld128(const uint8_t *p) {
        const brx_parse_u128u v = *(const brx_parse_u128u *)p;
        BrxTake128 r;
        r.lo = (uint64_t)v.w[0] | ((uint64_t)v.w[1] << 32);
        r.hi = (uint64_t)v.w[2] | ((uint64_t)v.w[3] << 32);
        return r;
    }
};

__global__ __launch_bounds__(256) void brx_parse_kernel(BrxTakeArgs a, uint32_t kind, uint32_t scale, uint32_t quote,
                                                        int64_t *__restrict__ val, uint8_t *__restrict__ status) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= a.m) return;
    BrxParseDevMem mem;
    const BrxTakeRec r = brx_take_entry_record(mem, a, j);
    const BrxParseOut o = brx_parse_lane(mem, a.out, a.span, r, kind, scale, a.flags, quote);
    val[j] = o.val;
    status[j] = (uint8_t)o.status;
}

void brx_launch_parse(const BrxTakeArgs &a, uint32_t kind, uint32_t scale, uint32_t quote, int64_t *val, uint8_t *status,
                      void *hip_stream) {
    const uint64_t blocks = (a.m + 255u) / 256u;
    if (blocks == 0) return;
    hipLaunchKernelGGL(brx_parse_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, a, kind, scale, quote, val, status);
}
