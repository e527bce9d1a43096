// brx_parse_f64.hip -- brx_parse_f64_batch: every selected record of the decoded streams of a batch as a correctly rounded binary64
// pattern and a status byte.  The grammar, the digits and the conversion are plain C++ in brx_parse_f64.h (around the unchanged
// brx_parse.h and brx_take.h), shared with tools/parse_f64_emu.cpp.  This file holds what is HIP: the memory policy, the table in
// device global memory, the kernel and the launch.
//
// One lane owns one entry and needs no other lane.  A record above 64 bytes is answered from its length alone; every other lane runs
// through at most four 16-byte units, one or two conversions and so one or two 16-byte loads of the table of csrc/brx_pow5.h (10.4 KB,
// read-only, shared by all lanes: it stays in the caches).  Integer arithmetic only; no scratch, no atomics, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>
#define BRX_POW5_STORAGE __device__
#include "brx_parse_f64.h"

struct __attribute__((packed, aligned(1))) brx_parse_f64_u128u { uint32_t w[4]; };

struct BrxParseF64DevMem {
    __device__ __forceinline__ uint8_t ld8(const uint8_t *p) { return *p; }
    __device__ __forceinline__ BrxTake128 ld128(const uint8_t *p) {
        const brx_parse_f64_u128u v = *(const brx_parse_f64_u128u *)p;
        BrxTake128 r;
        r.lo = (uint64_t)v.w[0] | ((uint64_t)v.w[1] << 32);
        r.hi = (uint64_t)v.w[2] | ((uint64_t)v.w[3] << 32);
        return r;
    }
};

__global__ __launch_bounds__(256) void brx_parse_f64_kernel(BrxTakeArgs a, uint32_t quote, uint64_t *__restrict__ val,
                                                            uint8_t *__restrict__ status) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= a.m) return;
    BrxParseF64DevMem mem;
    const BrxTakeRec r = brx_take_entry_record(mem, a, j);
    const BrxParseF64Out o = brx_parse_f64_lane(mem, brx_pow5, a.out, a.span, r, a.flags, quote);
    val[j] = o.bits;
    status[j] = (uint8_t)o.status;
}

void brx_launch_parse_f64(const BrxTakeArgs &a, uint32_t quote, uint64_t *val, uint8_t *status, void *hip_stream) {
    const uint64_t blocks = (a.m + 255u) / 256u;
    if (blocks == 0) return;
    hipLaunchKernelGGL(brx_parse_f64_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, a, quote, val, status);
}
