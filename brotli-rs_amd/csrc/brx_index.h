// brx_index.h -- shared by brx_index.hip (kernels) and brx_api.cpp (brx_index_batch): the tiling constants and the layout of one
// launch's scratch region.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define BRX_IX_ROW 1024u            // bytes a wavefront reads per step: 64 lanes x 16 B, 1 KiB aligned
#define BRX_IX_TILE_ROWS 64u
#define BRX_IX_TILE (BRX_IX_ROW * BRX_IX_TILE_ROWS) // one work item: 64 KiB of a stream's (1 KiB aligned) address range
#define BRX_IX_WG 512u              // threads per workgroup of the two passes over the bytes: 8 waves

// Scratch region of one launch, in bytes from its start:
#define BRX_IX_TICKET_A 0u          // ticket counter of the count pass, on a line of its own
#define BRX_IX_TICKET_C 128u        // ticket counter of the fill pass, likewise
#define BRX_IX_PRE 256u             // n + 1 words of 64 bits: exclusive prefix sum of the tiles per stream; behind them max_tiles
                                    // words of 64 bits: delimiters per tile (count pass), then their exclusive prefix sum (scan)

// A stream of l > 0 bytes has at most l / tile + 2 tiles (its first row starts up to 1023 bytes in front of it), one of 0 bytes has
// none; slots do not overlap and lie within `span`, so this bounds the tiles of a batch without a length read back.
static inline uint64_t brx_ix_max_tiles(uint32_t n, uint64_t span) { return span / BRX_IX_TILE + 2u * (uint64_t)n; }
static inline size_t brx_ix_region_bytes(size_t cap_n, size_t cap_tiles) {
    return (BRX_IX_PRE + (cap_n + 1u) * 8u + cap_tiles * 8u + 127u) & ~(size_t)127u;
}
