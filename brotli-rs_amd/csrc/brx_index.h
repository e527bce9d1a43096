// brx_index.h -- shared by brx_index.hip (kernels) and brx_api.cpp (brx_index_batch): the pass's part of one launch's scratch region.
#pragma once
#include <stdint.h>

#include "brx_tiles.h"

// Scratch region of one launch: the header of the tile pass (brx_tiles.h), then max_tiles words of 64 bits: delimiters per tile (count
// pass), then their exclusive prefix sum (scan).
// A stream of l > 0 bytes has at most l / tile + 2 tiles (its first row starts up to 1023 bytes in front of it), one of 0 bytes has
// none; slots do not overlap and lie within `span`, so this bounds the tiles of a batch without a length read back.
static inline uint64_t brx_ix_max_tiles(uint32_t n, uint64_t span) { return span / BRX_TP_TILE + 2u * (uint64_t)n; }
static inline size_t brx_ix_region_bytes(size_t cap_n, size_t cap_tiles) { return brx_tp_region_bytes(cap_n, cap_tiles * 8u); }

// brx_index.hip: plan and count on `hip_stream`, and scan and fill behind them if `pos`
void brx_launch_index(const void *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span, uint8_t delim,
                      void *scratch, uint64_t max_tiles, uint64_t *count, const uint64_t *pos_off, uint64_t *pos, uint64_t total,
                      unsigned workgroups, void *hip_stream);
