// brx_index_escaped.h -- shared by brx_index_escaped.hip (kernels) and brx_api.cpp (brx_index_escaped_batch): the pass's part of one
// launch's scratch region, and the arithmetic on a tile's state map (plain C: the kernels use it on the device, and it can be held to
// a serial walk on a CPU).
#pragma once
#include <stdint.h>

#include "brx_index.h"

#ifdef __HIPCC__
#define BRX_IE_HD __host__ __device__ __forceinline__
#else
#define BRX_IE_HD static inline
#endif

// The state in front of a byte, two bits, the bits of open[]: bit 0 = the parity of the active quotes in front of it, bit 1 = the byte
// is escaped.
#define BRX_IE_STATE_QUOTE 1u
#define BRX_IE_STATE_ESC 2u

// Scratch region of one launch: the header of the tile pass (brx_tiles.h), then max_tiles + 1 words of 64 bits ("word"), then
// max_tiles words of 64 bits ("exit"); brx_ix_max_tiles bounds the tiles as for brx_index_batch.  Word t is written twice:
//   count    the tile walked as if it were entered unescaped and outside quotes: its unescaped delimiters at even (c0) and odd (c1)
//            parity of its own active quotes (each <= 65536), the parity of its active quotes, whether the byte behind it is escaped,
//            and what stands behind its leading run of escape bytes (BRX_IE_LEAD_*) with the parity of that run's length -- from
//            which the walk from an escaped entry follows without a second look at the bytes (ie_select, ie_tile_map)
//   resolve  G[t], the record delimiters of all tiles of the batch in front of tile t, and the state tile t is really entered in;
//            word `total` holds G behind the last tile.  exit[t] = the state behind tile t (at the stream's end for its last tile).
#define BRX_IE_C0_BITS 24u
#define BRX_IE_C_MASK ((1ull << BRX_IE_C0_BITS) - 1ull)
#define BRX_IE_PAR_SHIFT 48u                // count: parity of the tile's active quotes
#define BRX_IE_X_SHIFT 49u                  // count: the byte behind the tile is escaped
#define BRX_IE_LEAD_SHIFT 50u               // count: BRX_IE_LEAD_*, two bits
#define BRX_IE_RODD_SHIFT 52u               // count: the leading run of escape bytes has odd length
#define BRX_IE_LEAD_OTHER 0u                // behind the leading run: a byte that is neither delimiter nor quote
#define BRX_IE_LEAD_DELIM 1u
#define BRX_IE_LEAD_QUOTE 2u
#define BRX_IE_LEAD_ALL 3u                  // nothing: all the tile's bytes of the stream are escape bytes
#define BRX_IE_G_MASK ((1ull << 62) - 1ull) // resolve: G[t]
#define BRX_IE_ENTRY_SHIFT 62u              // resolve: the state the tile is entered in, two bits
static inline size_t brx_ie_region_bytes(size_t cap_n, size_t cap_tiles) { return brx_tp_region_bytes(cap_n, (2u * cap_tiles + 1u) * 8u); }

// The carries of the kernels hand a run's parity through units that consist of escape bytes only, which is right because each unit
// has an even number of bytes: a lane's chunk, a row, a full tile.
static_assert(16u % 2u == 0u, "a lane's chunk of escape bytes must leave the run's parity as it is");
static_assert(BRX_TP_ROW % 2u == 0u, "a row of escape bytes must leave the run's parity as it is");
static_assert(BRX_TP_TILE % 2u == 0u, "a tile of escape bytes must leave the run's parity as it is");

// em = the escape bytes of 16 bytes (bit k: byte k), c = byte 0 is escaped.  -> bit k: byte k is escaped, for k = 0 .. 16 (bit 16: the
// byte behind the 16).  The recurrence esc(k + 1) = em[k] & ~esc(k) says that a byte is escaped iff the run of escape bytes in front
// of it has odd length (counting c as one more).  A run that starts at an even bit escapes the odd bits behind it, one that starts at
// an odd bit the even ones; adding the runs to their starts at odd bits carries through exactly those runs and flips the pattern
// behind them (the add-carry step known from simdjson's odd-backslash-run detection): no loop over the bits, no shift chain.
BRX_IE_HD uint32_t ie_escaped(uint32_t em, uint32_t c) {
    const uint32_t bs = em & ~c;              // (an escaped escape byte at byte 0 is data)
    const uint32_t follows = (bs << 1) | c;   // bytes directly behind an escape byte, or behind the carry
    const uint32_t odd_starts = bs & 0xAAAAAAAAu & ~follows;
    const uint32_t invert = (odd_starts + bs) << 1;
    return (0x55555555u ^ invert) & follows & 0x1FFFFu;
}

// A tile is a map from the state it is entered in to the state behind it: eight bits, two per entry state s at bit 2 s.
BRX_IE_HD uint32_t ie_apply(uint32_t map, uint32_t s) { return map >> (2u * s) & 3u; }

// first `f`, then `g` (associative, not commutative)
BRX_IE_HD uint32_t ie_compose(uint32_t f, uint32_t g) {
    return ie_apply(g, ie_apply(f, 0u)) | (ie_apply(g, ie_apply(f, 1u)) << 2) | (ie_apply(g, ie_apply(f, 2u)) << 4) |
           (ie_apply(g, ie_apply(f, 3u)) << 6);
}
#define BRX_IE_MAP_IDENTITY 0xE4u // 0 -> 0, 1 -> 1, 2 -> 2, 3 -> 3

// The map of the tile whose count word is w.  An escaped entry flips the escaped status of the one byte behind the tile's leading run
// of escape bytes and nothing else: if that byte is a quote the tile's quote parity flips; if there is no such byte (only escape bytes)
// the exit's escape bit flips; a delimiter or any other byte changes no state.  The quote parity of the entry is added to the tile's.
// The tile in which its stream starts is entered unescaped and outside quotes whatever lies in front of it: a constant map.
BRX_IE_HD uint32_t ie_tile_map(uint64_t w, int first) {
    const uint32_t lead = (uint32_t)(w >> BRX_IE_LEAD_SHIFT) & 3u;
    const uint32_t par = (uint32_t)(w >> BRX_IE_PAR_SHIFT) & 1u, x = (uint32_t)(w >> BRX_IE_X_SHIFT) & 1u;
    const uint32_t par1 = par ^ (lead == BRX_IE_LEAD_QUOTE ? 1u : 0u), x1 = x ^ (lead == BRX_IE_LEAD_ALL ? 1u : 0u);
    const uint32_t s0 = par | (x << 1), s1 = par1 | (x1 << 1); // behind the tile, entered (unescaped, escaped) outside quotes
    if (first) return s0 * 0x55u;
    return s0 | ((s0 ^ 1u) << 2) | (s1 << 4) | ((s1 ^ 1u) << 6);
}

// The record delimiters of the tile whose count word is w when it is entered in state s.  Escaped entry: a delimiter behind the
// leading run r is escaped iff r is even (it was counted at even parity, no quote precedes it: one less) and unescaped iff r is odd
// (one more); a quote there turns every parity behind it over, and no delimiter precedes it: the two counts swap.  Entered inside a
// quoted field the record delimiters are those at odd parity of the tile's own quotes.
BRX_IE_HD uint64_t ie_select(uint64_t w, uint32_t s) {
    uint64_t c0 = w & BRX_IE_C_MASK, c1 = w >> BRX_IE_C0_BITS & BRX_IE_C_MASK;
    if (s & BRX_IE_STATE_ESC) {
        const uint32_t lead = (uint32_t)(w >> BRX_IE_LEAD_SHIFT) & 3u;
        if (lead == BRX_IE_LEAD_DELIM) c0 = (w >> BRX_IE_RODD_SHIFT & 1u) ? c0 + 1u : c0 - 1u;
        if (lead == BRX_IE_LEAD_QUOTE) { const uint64_t t = c0; c0 = c1; c1 = t; }
    }
    return (s & BRX_IE_STATE_QUOTE) ? c1 : c0;
}

#define BRX_INDEX_ESCAPED_NO_QUOTE 1u // == BRX_INDEX_NO_QUOTE of brx.h

// brx_index_escaped.hip: plan, count and resolve on `hip_stream`, and fill behind them if `pos`
void brx_launch_index_escaped(const void *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span, uint8_t delim,
                              uint8_t quote, uint8_t escape, uint32_t flags, void *scratch, uint64_t max_tiles, uint64_t *count,
                              uint32_t *open, const uint64_t *pos_off, uint64_t *pos, uint64_t total, unsigned workgroups,
                              void *hip_stream);

// brx_index_set_batch: the same scratch region, tile word, state maps and resolve kernel, with a set of 1 .. 8 delimiter bytes (byte k
// of `set` for k < n_delims) and with the escape switched off by a flag as the quote is
#define BRX_INDEX_SET_NO_QUOTE 1u  // == BRX_INDEX_NO_QUOTE of brx.h
#define BRX_INDEX_SET_NO_ESCAPE 2u // == BRX_INDEX_NO_ESCAPE of brx.h
void brx_launch_index_set(const void *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span, uint64_t set,
                          uint32_t n_delims, uint8_t quote, uint8_t escape, uint32_t flags, void *scratch, uint64_t max_tiles,
                          uint64_t *count, uint32_t *open, const uint64_t *pos_off, uint64_t *pos, uint8_t *what, uint64_t total,
                          unsigned workgroups, void *hip_stream);
