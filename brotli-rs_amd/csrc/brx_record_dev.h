// brx_record_dev.h -- what is HIP and shared by the six record kernels (brx_take.hip, brx_hash.hip, brx_parse.hip, brx_parse_f64.hip,
// brx_parse_time.hip, brx_unescape.hip): the memory policy M of brx_take.h on the device, the broadcast of one lane's value as a scalar
// and the grid of a kernel with one thread per selection entry.  Included by the .hip files only: the emulators under tools/ bring
// their own, checking, policies.
#ifndef BRX_RECORD_DEV_H
#define BRX_RECORD_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "brx_take.h"

#define BRX_REC_BLOCK 256u // threads of a workgroup of a kernel with one thread per entry

struct __attribute__((packed, aligned(1))) brx_rec_u128u { uint32_t w[4]; }; // 16 bytes at any alignment

// the loads and the byte store: all that a kernel needs that stores no 16-byte unit
struct BrxRecMem {
    __device__ __forceinline__ uint8_t ld8(const uint8_t *p) { return *p; }
    __device__ __forceinline__ BrxTake128 ld128(const uint8_t *p) {
        const brx_rec_u128u v = *(const brx_rec_u128u *)p;
        BrxTake128 r;
        r.lo = (uint64_t)v.w[0] | ((uint64_t)v.w[1] << 32);
        r.hi = (uint64_t)v.w[2] | ((uint64_t)v.w[3] << 32);
        return r;
    }
    __device__ __forceinline__ void st8(uint8_t *p, uint8_t v) { *p = v; }
};

// ... with st128 at a 16-byte aligned address: one aligned dwordx4 (brx_take.h)
struct BrxRecMemAligned : BrxRecMem {
    __device__ __forceinline__ void st128(uint8_t *p, BrxTake128 v) {
        *(uint4 *)p = make_uint4((uint32_t)v.lo, (uint32_t)(v.lo >> 32), (uint32_t)v.hi, (uint32_t)(v.hi >> 32));
    }
};

// ... with st128 at any address (brx_unescape.h)
struct BrxRecMemUnaligned : BrxRecMem {
    __device__ __forceinline__ void st128(uint8_t *p, BrxTake128 v) {
        brx_rec_u128u w;
        w.w[0] = (uint32_t)v.lo; w.w[1] = (uint32_t)(v.lo >> 32); w.w[2] = (uint32_t)v.hi; w.w[3] = (uint32_t)(v.hi >> 32);
        *(brx_rec_u128u *)p = w;
    }
};

// x of lane `src` (wave-uniform) in every lane, as a scalar
__device__ __forceinline__ uint32_t brx_rec_bcast32(uint32_t x, uint32_t src) {
    return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)src);
}
__device__ __forceinline__ uint64_t brx_rec_bcast(uint64_t x, uint32_t src) {
    return (uint64_t)brx_rec_bcast32((uint32_t)x, src) | ((uint64_t)brx_rec_bcast32((uint32_t)(x >> 32), src) << 32);
}

// one thread per entry: this thread's entry, and the workgroups for m of them (brx_api.cpp has refused an m that does not fit a grid)
__device__ __forceinline__ uint64_t brx_rec_entry() { return (uint64_t)blockIdx.x * BRX_REC_BLOCK + threadIdx.x; }
static inline unsigned brx_rec_blocks(uint64_t m) { return (unsigned)((m + (BRX_REC_BLOCK - 1u)) / BRX_REC_BLOCK); }

#endif
