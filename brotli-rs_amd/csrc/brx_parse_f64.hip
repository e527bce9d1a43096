// brx_parse_f64.hip -- brx_parse_f64_batch: every selected record of the decoded streams of a batch as a correctly rounded binary64
// pattern and a status byte.  The grammar, the digits and the conversion are plain C++ in brx_parse_f64.h (around the unchanged
// brx_parse.h and brx_take.h), shared with tools/parse_f64_emu.cpp.  This file holds what is HIP and its own: the table in device
// global memory, the kernel and the launch.  What the record kernels share on the device is brx_record_dev.h.
//
// One lane owns one entry and needs no other lane.  A record above 64 bytes is answered from its length alone; every other lane runs
// through at most four 16-byte units, one or two conversions and so one or two 16-byte loads of the table of csrc/brx_pow5.h (10.4 KB,
// read-only, shared by all lanes: it stays in the caches).  Integer arithmetic only; no scratch, no atomics, no LDS.
#include "brx_record_dev.h"
#define BRX_POW5_STORAGE __device__
#include "brx_parse_f64.h"

__global__ __launch_bounds__(BRX_REC_BLOCK) void brx_parse_f64_kernel(BrxTakeArgs a, uint32_t quote, uint64_t *__restrict__ val,
                                                                      uint8_t *__restrict__ status) {
    const uint64_t j = brx_rec_entry();
    if (j >= a.m) return;
    BrxRecMem mem;
    const BrxTakeRec r = brx_take_entry_record(mem, a, j);
    const BrxParseF64Out o = brx_parse_f64_lane(mem, brx_pow5, a.out, a.span, r, a.flags, quote);
    val[j] = o.bits;
    status[j] = (uint8_t)o.status;
}

void brx_launch_parse_f64(const BrxTakeArgs &a, uint32_t quote, uint64_t *val, uint8_t *status, void *hip_stream) {
    if (a.m == 0) return;
    hipLaunchKernelGGL(brx_parse_f64_kernel, dim3(brx_rec_blocks(a.m)), dim3(BRX_REC_BLOCK), 0, (hipStream_t)hip_stream, a, quote, val, status);
}
