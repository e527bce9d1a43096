// brx_index_quoted.h -- shared by brx_index_quoted.hip (kernels) and brx_api.cpp (brx_index_quoted_batch): the pass's part of one
// launch's scratch region.
#pragma once
#include <stdint.h>

#include "brx_index.h"

// Scratch region of one launch: the header of the tile pass (brx_tiles.h), then max_tiles + 1 words of 64 bits (brx_ix_max_tiles bounds
// the tiles as for brx_index_batch).  Word t is written twice:
//   count    the tile's delimiters at even (c0) and odd (c1) quote parity and the parity of its quotes, all taken as if the tile
//            started outside quotes (each count <= 65536)
//   resolve  G[t], the record delimiters of all tiles of the batch in front of tile t, the parity the tile really starts with, and
//            P[t], the parity of all quotes of the batch in front of tile t; word `total` holds G and P behind the last tile
#define BRX_IQ_C0_BITS 24u
#define BRX_IQ_C_MASK ((1ull << BRX_IQ_C0_BITS) - 1ull)
#define BRX_IQ_PAR_SHIFT 48u                // count: parity of the tile's quotes
#define BRX_IQ_G_MASK ((1ull << 62) - 1ull) // resolve: G[t]
#define BRX_IQ_START_SHIFT 62u              // resolve: 1 = the tile's first byte lies inside a quoted field
#define BRX_IQ_P_SHIFT 63u                  // resolve: P[t]
static inline size_t brx_iq_region_bytes(size_t cap_n, size_t cap_tiles) { return brx_tp_region_bytes(cap_n, (cap_tiles + 1u) * 8u); }

// brx_index_quoted.hip: plan, count and resolve on `hip_stream`, and fill behind them if `pos`
void brx_launch_index_quoted(const void *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span, uint8_t delim,
                             uint8_t quote, void *scratch, uint64_t max_tiles, uint64_t *count, uint32_t *open, const uint64_t *pos_off,
                             uint64_t *pos, uint64_t total, unsigned workgroups, void *hip_stream);
