// brx_parse.hip -- brx_parse_batch: every selected record of the decoded streams of a batch as a 64-bit number and a status byte.
// The fetch, the classification, the grammar and the conversion are plain C++ in brx_parse.h, shared with tools/parse_emu.cpp; the
// record rule is that of brx_take.h.  This file holds what is HIP and its own: the kernel and the launch.  What the record kernels share
// on the device is brx_record_dev.h.
//
// One lane owns one entry and needs no other lane: a record above 64 bytes is answered from its length alone, so no lane runs through
// more than four 16-byte units.  No scratch, no atomics, no LDS; the status goes out as a byte store, the value as a qword store.
#include "brx_record_dev.h"
#include "brx_parse.h"

__global__ __launch_bounds__(BRX_REC_BLOCK) void brx_parse_kernel(BrxTakeArgs a, uint32_t kind, uint32_t scale, uint32_t quote,
                                                                  int64_t *__restrict__ val, uint8_t *__restrict__ status) {
    const uint64_t j = brx_rec_entry();
    if (j >= a.m) return;
    BrxRecMem mem;
    const BrxTakeRec r = brx_take_entry_record(mem, a, j);
    const BrxParseOut o = brx_parse_lane(mem, a.out, a.span, r, kind, scale, a.flags, quote);
    val[j] = o.val;
    status[j] = (uint8_t)o.status;
}

void brx_launch_parse(const BrxTakeArgs &a, uint32_t kind, uint32_t scale, uint32_t quote, int64_t *val, uint8_t *status,
                      void *hip_stream) {
    if (a.m == 0) return;
    hipLaunchKernelGGL(brx_parse_kernel, dim3(brx_rec_blocks(a.m)), dim3(BRX_REC_BLOCK), 0, (hipStream_t)hip_stream, a, kind, scale, quote, val, status);
}
