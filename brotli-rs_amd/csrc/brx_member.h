// brx_member.h -- shared by brx_member.hip (kernels), brx_api.cpp (brx_member_batch) and tools/member_emu.cpp (the same text on a CPU,
// lane by lane).  Everything of the pass that is not HIP-specific lives here: the boundaries of a stream that count, the summary of a
// unit of 16 boundary bytes and how two summaries join, the walk of a unit that knows its depth and its line, the look at one key
// record, the element of the scan over the tiles, and the last step that turns the settled slots into the call's results.  The rule is
// THE RULE of include/brx.h (brx_member_batch); which bytes a key record is comes from brx_take.h (brx_take_record).
//
// Memory goes through a policy type M so that the emulator sees every load and every store:
//   uint8_t M::ld8(const uint8_t *p), BrxTake128 M::ld128(const uint8_t *p)     arena bytes, as in brx_take.h
//   uint8_t M::ldw8(const uint8_t *p), BrxTake128 M::ldw128(const uint8_t *p)   bytes of `what`, 16 of them at any alignment
//   void M::max64(uint64_t *p, uint64_t v)    *p = max(*p, v), atomically: a slot of sel_rec while it is being settled
//   void M::or32(uint32_t *p, uint32_t v)     *p |= v, atomically: a line's flag bits while they are being collected
//   uint64_t M::get64(const uint64_t *p), uint32_t M::get32(const uint32_t *p)  a settled slot, read back by the last step
//   void M::st64(uint64_t *p, uint64_t v), st32(uint32_t *p, uint32_t v), st8(uint8_t *p, uint8_t v)   the results
// The tables (out_off, len, count, pos_off, pos, line_off) and the pass's own scratch are read directly.
//
// How it is computed.  The boundaries of stream i that count are k < C(i) = min(count[i], n_pos - pos_off[i]): those behind them would
// be neutral and change nothing.  They are cut into TILES of BRX_MB_TILE boundaries, a tile into ROWS of BRX_MB_ROW, a row into one
// UNIT of 16 per lane.  A span of boundaries is summed up as BrxMbSum: its line feeds, and the bracket sum behind its last line feed
// (or of all of it, where it has none).  Summaries join left to right (brx_mb_join); that is all a lane needs from the lanes in front of
// it and a tile from the tiles in front of it, since the depth restarts at every line feed.  Whether the depth fell below 0 is NOT
// part of the summary: the walk knows the absolute depth, sees the fall where it happens and flags the line there.
//   plan      tiles per stream, their exclusive prefix sum pre[0 .. n] (one workgroup)
//   sum       BrxMbSum of every tile (one wave per tile)
//   compose   the scan of the tiles' summaries in tile order, restarted at every stream's first tile: line index and depth in front of
//             every tile, lines[i] of every stream (one workgroup)
//   emit      every unit walked with its depth and line known: a ':' at depth 1 has its key record looked at; a match raises the slot
//             of (name, line) to k + 1 (max64: the last member wins whichever tile found it), flag bits are collected in the line's
//             slot of sel_stream's first column (or32), which is the pass's own until the last step
//   finish    one thread per line slot j < m: the stream by binary search in line_off, every name's slot from k + 1 to the results
#ifndef BRX_MEMBER_H
#define BRX_MEMBER_H
#include <stddef.h>
#include <stdint.h>
#include "brx_take.h"
#include "brx_unescape.h" // brx_text_eq16: the SWAR byte compare of a 16-byte unit

#define BRX_MB_UNIT 16u
#define BRX_MB_ROW 1024u  // boundaries per wave step: 64 lanes x 16 bytes of `what`
#define BRX_MB_TILE 4096u // boundaries per tile: one wave's work item, 4 rows
#define BRX_MB_MAX_NAMES 8u // == BRX_MEMBER_MAX_NAMES (include/brx.h)
#define BRX_MB_MAX_NAME 32u // == BRX_MEMBER_MAX_NAME
#define BRX_MB_MAX_KEY 64u  // == BRX_MEMBER_MAX_KEY
#define BRX_MB_K_MISSING 0u // == BRX_MEMBER_MISSING ...
#define BRX_MB_K_SCALAR 1u
#define BRX_MB_K_OBJECT 2u
#define BRX_MB_K_ARRAY 3u
#define BRX_MB_K_BAD 4u
#define BRX_MB_F_LONG_KEY 1u // == BRX_MEMBER_LONG_KEY ...
#define BRX_MB_F_ESCAPED_KEY 2u
#define BRX_MB_F_UNBALANCED 4u

// the names, as launch arguments: name q is the low name_len[q] bytes of w[q][0 .. 4), the bytes above them 0
struct BrxMbNames {
    uint64_t w[BRX_MB_MAX_NAMES][4];
    uint32_t len[BRX_MB_MAX_NAMES];
    uint32_t n;
};

struct BrxMbSum { uint32_t nl; int32_t d; uint32_t rd; };     // line feeds; bracket sum behind the last of them; is there one
struct BrxMbSeg { uint64_t L; int32_t d; uint32_t r; };       // the scan over the tiles: r bit 0: d restarted, bit 1: L restarted

// everything the pass reads and writes, as the call got it, and its scratch
struct BrxMbArgs {
    BrxTakeArgs a; // flags = BRX_TAKE_F_NO_DELIM, delim_len = 1: the key record of the member at k is record k
    const uint8_t *what;
    uint64_t *lines;
    const uint64_t *line_off;
    uint64_t m;
    uint32_t *sel_stream;
    uint64_t *sel_rec;
    uint8_t *kind, *line_flags;
    uint64_t max_tiles;
    uint64_t *pre;    // n + 1: exclusive prefix sum of the tiles per stream
    uint64_t *slines; // n: lines[i], for the last step (the caller's `lines` may be NULL)
    BrxMbSum *sum;    // max_tiles
    BrxMbSeg *in;     // max_tiles: line index and depth in front of the tile
};

static inline size_t brx_mb_region_bytes(size_t n, size_t max_tiles) {
    return ((n + 1u) * 8u + n * 8u + max_tiles * (sizeof(BrxMbSum) + sizeof(BrxMbSeg)) + 127u) & ~(size_t)127u;
}
// an upper bound of the tiles of a call whose pos_off is the prefix sum of its counts: what the scratch holds and the grid covers
static inline uint64_t brx_mb_max_tiles(uint32_t n, uint64_t n_pos) { return (uint64_t)n + n_pos / BRX_MB_TILE; }

// C(i): the boundaries of stream i that count.  pos_off[i] + k < n_pos for every k < C(i).
BRX_TAKE_HD uint64_t brx_mb_count(const BrxTakeArgs &a, uint64_t i) {
    const uint64_t base = a.pos_off[i], c = a.count[i];
    if (base >= a.n_pos) return 0;
    const uint64_t room = a.n_pos - base;
    return c < room ? c : room;
}
BRX_TAKE_HD uint64_t brx_mb_tiles(uint64_t c) { return c / BRX_MB_TILE + (c % BRX_MB_TILE ? 1u : 0u); }
// boundaries of the unit that starts at boundary k0 of a stream with c of them
BRX_TAKE_HD uint32_t brx_mb_valid(uint64_t c, uint64_t k0) { return k0 >= c ? 0u : c - k0 < BRX_MB_UNIT ? (uint32_t)(c - k0) : BRX_MB_UNIT; }

// nv <= 16 bytes of `what` from index g on; the bytes behind them 0, which is neutral, and not loaded
template <class M>
BRX_TAKE_HD BrxTake128 brx_mb_unit(M &mem, const uint8_t *what, uint64_t g, uint32_t nv) {
    if (nv == BRX_MB_UNIT) return mem.ldw128(what + g);
    BrxTake128 v = {0, 0};
    for (uint32_t t = 0; t < BRX_MB_UNIT; t++) {
        if (t < nv) {
            const uint64_t b = mem.ldw8(what + g + t);
            if (t < 8u) v.lo |= b << (8u * t); else v.hi |= b << (8u * (t - 8u));
        }
    }
    return v;
}

// bit t: byte t of the unit opens / closes a bracket ('{' and '[', '}' and ']' differ in bit 5 only), is a line feed, is a colon
struct BrxMbMasks { uint32_t open, close, nl, colon; };
BRX_TAKE_HD BrxMbMasks brx_mb_masks(BrxTake128 v) {
    BrxTake128 w = {v.lo | 0x2020202020202020ull, v.hi | 0x2020202020202020ull};
    BrxMbMasks k;
    k.open = brx_text_eq16(w, 0x7Bu);
    k.close = brx_text_eq16(w, 0x7Du);
    k.nl = brx_text_eq16(v, 0x0Au);
    k.colon = brx_text_eq16(v, 0x3Au);
    return k;
}

BRX_TAKE_HD BrxMbSum brx_mb_unit_sum(const BrxMbMasks &k) {
    BrxMbSum s = {(uint32_t)__builtin_popcount(k.nl), 0, k.nl ? 1u : 0u};
    const uint32_t behind = k.nl ? ~((2u << (31u - (uint32_t)__builtin_clz(k.nl))) - 1u) & 0xFFFFu : 0xFFFFu;
    s.d = (int32_t)__builtin_popcount(k.open & behind) - (int32_t)__builtin_popcount(k.close & behind);
    return s;
}
// a span and the span behind it, as one
BRX_TAKE_HD BrxMbSum brx_mb_join(BrxMbSum a, BrxMbSum b) {
    BrxMbSum s = {a.nl + b.nl, b.rd ? b.d : a.d + b.d, a.rd | b.rd};
    return s;
}
// ... over the tiles of all streams: L counts line feeds from the stream's first tile on
BRX_TAKE_HD BrxMbSeg brx_mb_seg_join(BrxMbSeg a, BrxMbSeg b) {
    BrxMbSeg s = {(b.r & 2u) ? b.L : a.L + b.L, (b.r & 1u) ? b.d : a.d + b.d, a.r | b.r};
    return s;
}
BRX_TAKE_HD BrxMbSeg brx_mb_seg_of(BrxMbSum t) { BrxMbSeg s = {t.nl, t.d, t.rd}; return s; }
BRX_TAKE_HD BrxMbSeg brx_mb_seg_start() { BrxMbSeg s = {0, 0, 3u}; return s; } // in front of a stream's first tile

// the stream of tile t: the last i < n with pre[i] <= t (streams without tiles share their successor's value and lose)
BRX_TAKE_HD uint32_t brx_mb_tile_stream(const uint64_t *pre, uint32_t n, uint64_t t) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (pre[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// `bits` for line `line` of stream i, where that line has a slot
template <class M>
BRX_TAKE_HD void brx_mb_flag(M &mem, const BrxMbArgs &x, uint64_t i, uint64_t line, uint32_t bits) {
    const uint64_t j = x.line_off[i] + line;
    if (bits && j >= line && j < x.m) mem.or32(x.sel_stream + j, bits);
}

BRX_TAKE_HD uint64_t brx_mb_below(uint32_t n) { return n >= 64u ? ~(uint64_t)0 : ((uint64_t)1 << n) - 1u; }

// The key record of the member whose ':' is boundary k of stream i (a: flags = BRX_TAKE_F_NO_DELIM, delim_len = 1), trimmed.  Returns
// the flag bits it adds.  Where '"', bn = 1 .. 32 bytes and '"' are left, `carries(key)` is called with those bytes as a name is kept;
// the caller says there which names they are (brx_mb_key_is) and what follows.  Shared with brx_object.h.  Loads the record's bytes (at
// most 64) once for the masks and the key's body (at most 32) once more where it is placed.
struct BrxMbKey { uint32_t bn; BrxTake128 b0, b1; };
template <class M, class F>
BRX_TAKE_HD uint32_t brx_mb_key(M &mem, const BrxTakeArgs &a, uint64_t i, uint64_t k, F carries) {
    const BrxTakeRec r = brx_take_record(mem, a, i, k);
    if (r.len > BRX_MB_MAX_KEY) return BRX_MB_F_LONG_KEY;
    const uint32_t L = (uint32_t)r.len;
    // (wide loads stay inside the STREAM, not only inside the arena: its bounds stand where brx_take_fetch takes the arena's)
    const uint8_t *p = a.out + r.src, *lo_a = a.out + a.out_off[i], *hi_a = lo_a + a.len[i];
    uint64_t blank = 0, bs = 0, qt = 0;
#define BRX_MB_KEY_UNIT(g)                                                                                           \
    if (L > 16u * (g)) {                                                                                              \
        const uint32_t n_ = L - 16u * (g) < 16u ? L - 16u * (g) : 16u;                                                \
        const BrxTake128 v_ = brx_take_place(brx_take_fetch(mem, p + 16u * (g), n_, lo_a, hi_a), 0u, n_);          \
        blank |= (uint64_t)(brx_text_eq16(v_, 0x20u) | brx_text_eq16(v_, 0x09u) | brx_text_eq16(v_, 0x0Du)) << (16u * (g)); \
        bs |= (uint64_t)brx_text_eq16(v_, 0x5Cu) << (16u * (g));                                                      \
        qt |= (uint64_t)brx_text_eq16(v_, 0x22u) << (16u * (g));                                                      \
    }
    BRX_MB_KEY_UNIT(0u)
    BRX_MB_KEY_UNIT(1u)
    BRX_MB_KEY_UNIT(2u)
    BRX_MB_KEY_UNIT(3u)
#undef BRX_MB_KEY_UNIT
    const uint64_t in = brx_mb_below(L);
    const uint32_t flags = (bs & in) ? BRX_MB_F_ESCAPED_KEY : 0u;
    const uint64_t ns = in & ~blank;
    if (!ns) return flags;
    const uint32_t lo = (uint32_t)__builtin_ctzll(ns), hi = 64u - (uint32_t)__builtin_clzll(ns), T = hi - lo;
    if (T < 3u || T > BRX_MB_MAX_NAME + 2u || !((qt >> lo) & 1u) || !((qt >> (hi - 1u)) & 1u)) return flags;
    const uint32_t bn = T - 2u, n0 = bn < 16u ? bn : 16u;
    const BrxTake128 b0 = brx_take_place(brx_take_fetch(mem, p + lo + 1u, n0, lo_a, hi_a), 0u, n0);
    BrxTake128 b1 = {0, 0};
    if (bn > 16u) b1 = brx_take_place(brx_take_fetch(mem, p + lo + 17u, bn - 16u, lo_a, hi_a), 0u, bn - 16u);
    const BrxMbKey ky = {bn, b0, b1};
    carries(ky);
    return flags;
}
// the key carries name q
BRX_TAKE_HD bool brx_mb_key_is(const BrxMbNames &nm, uint32_t q, const BrxMbKey &ky) {
    return nm.len[q] == ky.bn && nm.w[q][0] == ky.b0.lo && nm.w[q][1] == ky.b0.hi && nm.w[q][2] == ky.b1.lo && nm.w[q][3] == ky.b1.hi;
}

// The member whose ':' is boundary k of stream i, in line `line`: its key record against the names.  Returns the flag bits it adds
// to its line.
template <class M>
BRX_TAKE_HD uint32_t brx_mb_member(M &mem, const BrxMbArgs &x, const BrxMbNames &nm, uint64_t i, uint64_t k, uint64_t line) {
    return brx_mb_key(mem, x.a, i, k, [&](const BrxMbKey &ky) {
        const uint64_t j = x.line_off[i] + line;
        if (j < line || j >= x.m) return;
        // (not unrolled: the names stay in the launch arguments and are fetched by the scalar unit, one name per turn, instead of all
        // 8 x 32 bytes living in scalar registers across the walk)
#pragma unroll 1
        for (uint32_t q = 0; q < nm.n; q++) {
            if (brx_mb_key_is(nm, q, ky)) mem.max64(x.sel_rec + (uint64_t)q * x.m + j, k + 1u);
        }
    });
}

// One lane, one unit: the nv boundaries from k0 on of stream i (c of them count), with `line` and depth `d` in front of the unit.
template <class M>
BRX_TAKE_HD void brx_mb_walk(M &mem, const BrxMbArgs &x, const BrxMbNames &nm, uint64_t i, uint64_t c, uint64_t k0, uint32_t nv,
                             const BrxMbMasks &k, uint64_t line, int32_t d) {
    uint32_t flags = 0;
    for (uint32_t todo = k.open | k.close | k.nl | k.colon; todo; todo &= todo - 1u) {
        const uint32_t t = (uint32_t)__builtin_ctz(todo), bit = 1u << t;
        if (k.open & bit) d++;
        else if (k.close & bit) { if (--d < 0) flags |= BRX_MB_F_UNBALANCED; }
        else if (k.colon & bit) { if (d == 1) flags |= brx_mb_member(mem, x, nm, i, k0 + t, line); }
        else {
            if (d != 0) flags |= BRX_MB_F_UNBALANCED;
            brx_mb_flag(mem, x, i, line, flags);
            flags = 0;
            d = 0;
            line++;
        }
    }
    if (nv && k0 + nv == c && d != 0) flags |= BRX_MB_F_UNBALANCED; // the stream's last line ends here, without a line feed
    brx_mb_flag(mem, x, i, line, flags);
}

// The last step, slot j < m: the stream whose line it is, the line's flags, and every name's slot from "k + 1 of the last member, or
// 0" to sel_rec, kind and sel_stream.  A slot that is no stream's line (line_off is not what the count pass gave) selects nothing.
template <class M>
BRX_TAKE_HD void brx_mb_finish(M &mem, const BrxMbArgs &x, uint32_t n_names, uint64_t j) {
    uint32_t lo = 0, hi = x.a.n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (x.line_off[mid] <= j) lo = mid; else hi = mid;
    }
    const uint64_t i = lo, first = x.line_off[i];
    const bool owned = first <= j && j - first < x.slines[i];
    const uint32_t flags = mem.get32(x.sel_stream + j);
    const uint64_t c = owned ? brx_mb_count(x.a, i) : 0u, base = x.a.pos_off[i];
    for (uint32_t q = 0; q < n_names; q++) {
        const uint64_t at = (uint64_t)q * x.m + j, v = mem.get64(x.sel_rec + at);
        uint32_t kind = BRX_MB_K_MISSING;
        if (owned && v) {
            kind = BRX_MB_K_BAD;
            if (v < c) {
                const uint32_t w = mem.ldw8(x.what + base + v);
                if (w == 0x2Cu || w == 0x7Du) kind = BRX_MB_K_SCALAR;
                else if (w == 0x7Bu) kind = BRX_MB_K_OBJECT;
                else if (w == 0x5Bu) kind = BRX_MB_K_ARRAY;
            }
        }
        mem.st64(x.sel_rec + at, kind == BRX_MB_K_MISSING ? ~(uint64_t)0 : v);
        mem.st8(x.kind + at, (uint8_t)kind);
        mem.st32(x.sel_stream + at, owned ? (uint32_t)i : x.a.n);
    }
    if (x.line_flags) mem.st8(x.line_flags + j, owned ? (uint8_t)(flags & 7u) : (uint8_t)0);
}

// host side (brx_api.cpp): the launches of a call, `scratch` a region of brx_mb_region_bytes(n, max_tiles)
void brx_launch_member(BrxMbArgs x, const BrxMbNames &nm, void *scratch, void *hip_stream);
#endif
