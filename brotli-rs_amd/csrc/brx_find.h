// brx_find.h -- shared by brx_find.hip (kernels) and brx_api.cpp (brx_find_batch).  The pass's part of one launch's scratch region is
// that of brx_index_batch (brx_index.h: one 64-bit word per tile, brx_ix_max_tiles, brx_ix_region_bytes).
#pragma once
#include <stdint.h>

#include "brx_index.h"

#define BRX_FIND_MAX_NEEDLE 16u // bytes: what a lane's chunk and the chunk in front of it always hold

// brx_find.hip: plan and count on `hip_stream`, and scan and fill behind them if `pos`.  `needle` (HOST memory, 1 .. 16 bytes) is read
// here and travels in the launch arguments.
void brx_launch_find(const void *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span, const uint8_t *needle,
                     uint32_t needle_len, void *scratch, uint64_t max_tiles, uint64_t *count, const uint64_t *pos_off, uint64_t *pos,
                     uint64_t total, unsigned workgroups, void *hip_stream);
