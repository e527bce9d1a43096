// brx_parse_time.hip -- brx_parse_time_batch: every selected record of the decoded streams of a batch as a date, a time of day or a
// timestamp: a 64-bit count of days, or of units of 10^-scale s, a status byte and optionally the zone's offset in minutes.  The
// grammar, the calendar and the arithmetic are plain C++ in brx_parse_time.h (around the unchanged brx_parse.h and brx_take.h), shared
// with tools/parse_time_emu.cpp.  This file holds what is HIP and its own: the kernel and the launch.  What the record kernels share on
// the device is brx_record_dev.h.
//
// One lane owns one entry and needs no other lane.  A record above 64 bytes is answered from its length alone; every other lane runs
// through at most four 16-byte units and a fixed sequence of mask tests.  Integer arithmetic only; no table, no scratch, no atomics,
// no LDS.
#include "brx_record_dev.h"
#include "brx_parse_time.h"

__global__ __launch_bounds__(BRX_REC_BLOCK) void brx_parse_time_kernel(BrxTakeArgs a, uint32_t kind, uint32_t scale, uint32_t quote,
                                                                       int64_t *__restrict__ val, uint8_t *__restrict__ status,
                                                                       int16_t *__restrict__ zone) {
    const uint64_t j = brx_rec_entry();
    if (j >= a.m) return;
    BrxRecMem mem;
    const BrxTakeRec r = brx_take_entry_record(mem, a, j);
    const BrxParseTimeOut o = brx_parse_time_lane(mem, a.out, a.span, r, kind, scale, a.flags, quote);
    val[j] = o.val;
    status[j] = (uint8_t)o.status;
    if (zone) zone[j] = (int16_t)o.zone;
}

void brx_launch_parse_time(const BrxTakeArgs &a, uint32_t kind, uint32_t scale, uint32_t quote, int64_t *val, uint8_t *status, int16_t *zone,
                           void *hip_stream) {
    if (a.m == 0) return;
    hipLaunchKernelGGL(brx_parse_time_kernel, dim3(brx_rec_blocks(a.m)), dim3(BRX_REC_BLOCK), 0, (hipStream_t)hip_stream, a, kind, scale,
                       quote, val, status, zone);
}
