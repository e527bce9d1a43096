// brx_take.h -- shared by brx_take.hip (kernels), brx_api.cpp (brx_take_batch) and tools/take_emu.cpp (the same text on a CPU, lane by
// lane).  Everything of the pass that is not HIP-specific lives here: the rule (brx_take_record), the resolution of a selection entry,
// the descriptor of an entry, the window arithmetic of the fill kernel and the assembly of one 16-byte destination unit.
//
// Memory goes through a policy type M so that the emulator can see every arena load and every destination store:
//   uint8_t  M::ld8(const uint8_t *p)             one arena byte
//   BrxTake128 M::ld128(const uint8_t *p)         16 arena bytes at any alignment (only where the caller proved them inside the arena)
//   void     M::st8(uint8_t *p, uint8_t v)        one destination byte
//   void     M::st128(uint8_t *p, BrxTake128 v)   16 destination bytes, p 16-byte aligned (on the device BrxRecMemAligned of
//                                                 brx_record_dev.h: one aligned dwordx4; brx_unescape.h stores at any address, through
//                                                 BrxRecMemUnaligned)
// The tables (out_off, len, count, pos_off, pos, sel_*, dst_off) are read directly: the caller owns their sizes.
#ifndef BRX_TAKE_H
#define BRX_TAKE_H
#include <stdint.h>

#if defined(__HIP__)
#define BRX_TAKE_HD __host__ __device__ __forceinline__
#else
#define BRX_TAKE_HD inline
#endif

#define BRX_TAKE_CHUNK 4096u // bytes of the destination's address range that one wavefront owns; cut at 16-byte aligned addresses
#define BRX_TAKE_UNIT 16u    // one lane's share of a row: an aligned dwordx4 of the destination
#define BRX_TAKE_ROW (64u * BRX_TAKE_UNIT)
#define BRX_TAKE_WINDOW 64u  // descriptors resident at a time: one per lane
#define BRX_TAKE_F_NO_DELIM 1u // == BRX_TAKE_NO_DELIM (include/brx.h)
#define BRX_TAKE_F_TRIM_CR 2u  // == BRX_TAKE_TRIM_CR
#define BRX_TAKE_NONE (~(uint64_t)0)

struct BrxTake128 { uint64_t lo, hi; }; // byte q of a unit is bits [8q, 8q + 8) of lo (q < 8) or of hi

// everything the rule reads, as the call got it
struct BrxTakeArgs {
    const uint8_t *out;
    const uint64_t *out_off, *len;
    uint32_t n;
    uint64_t span; // of the arena: wide loads stay inside [out, out + span)
    const uint64_t *count, *pos_off, *pos;
    uint64_t n_pos;
    uint32_t delim_len, flags;
    const uint32_t *sel_stream; // both NULL: all-records mode
    const uint64_t *sel_rec;
    uint64_t m;
};

struct BrxTakeRec { uint64_t src, len; }; // offset of the record's first byte in the arena, and L

// P(i,k) of the contract, for a stream of length l: never above l, pos not loaded at or behind n_pos
BRX_TAKE_HD uint64_t brx_take_pos(const BrxTakeArgs &a, uint64_t base, uint64_t k, uint64_t l) {
    const uint64_t idx = base + k;
    if (idx < base || idx >= a.n_pos) return l;
    const uint64_t p = a.pos[idx];
    return p < l ? p : l;
}

// THE RULE (include/brx.h, brx_take_batch): record k of stream i.  An entry that selects nothing gives {0, 0}.
template <class M>
BRX_TAKE_HD BrxTakeRec brx_take_record(M &mem, const BrxTakeArgs &a, uint64_t i, uint64_t k) {
    BrxTakeRec r = {0, 0};
    if (i >= a.n) return r;
    const uint64_t cnt = a.count[i];
    if (k > cnt) return r;
    const uint64_t l = a.len[i], base = a.pos_off[i], off = a.out_off[i], D = a.delim_len;
    uint64_t start = 0, end = l;
    if (k > 0) {
        start = brx_take_pos(a, base, k - 1u, l) + D;
        if (start > l) start = l;
    }
    if (k < cnt) {
        end = brx_take_pos(a, base, k, l);
        if (!(a.flags & BRX_TAKE_F_NO_DELIM)) {
            end += D;
            if (end > l) end = l;
        }
    }
    if (end < start) end = start;
    if ((a.flags & BRX_TAKE_F_TRIM_CR) && end > start && mem.ld8(a.out + off + end - 1u) == 0x0Du) end--;
    r.src = off + start;
    r.len = end - start;
    return r;
}

// Entry j of the selection -> (stream, record).  All-records mode: the last stream with pos_off[i] + i <= j, by binary search.
BRX_TAKE_HD void brx_take_entry(const BrxTakeArgs &a, uint64_t j, uint64_t &i, uint64_t &k) {
    if (a.sel_stream) {
        i = a.sel_stream[j];
        k = a.sel_rec[j];
        return;
    }
    uint32_t lo = 0, hi = a.n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (a.pos_off[mid] + mid <= j) lo = mid; else hi = mid;
    }
    const uint64_t key = a.pos_off[lo] + lo;
    i = lo;
    k = j - key;
    if (key > j) i = a.n; // no stream starts at or in front of j: nothing
}

template <class M>
BRX_TAKE_HD BrxTakeRec brx_take_entry_record(M &mem, const BrxTakeArgs &a, uint64_t j) {
    uint64_t i, k;
    brx_take_entry(a, j, i, k);
    return brx_take_record(mem, a, i, k);
}

// ---- the fill kernel's lane logic ------------------------------------------------------------------------------------------------
// Coordinates: y = (index into dst) + phase with phase = (address of dst) & 15, so that y % 16 == 0 is a 16-byte aligned address and
// dst_al = dst - phase is the aligned base that y counts from.  Chunk c owns y in [max(c * CHUNK, phase), min((c + 1) * CHUNK, total +
// phase)).  A destination byte belongs to the LAST entry whose dst_off is not behind it; the byte is written iff it lies inside that
// entry's first min(L, room) bytes.

// One entry's descriptor: where its room starts (in y), where its bytes come from, how many of them land (L clamped by the room).
struct BrxTakeDesc { uint64_t start, src, cnt; };

template <class M>
BRX_TAKE_HD BrxTakeDesc brx_take_descriptor(M &mem, const BrxTakeArgs &a, const uint64_t *dst_off, uint64_t total, uint32_t phase,
                                            uint64_t j) {
    BrxTakeDesc d = {BRX_TAKE_NONE, 0, 0};
    if (j >= a.m) return d; // sorts behind every real entry
    const uint64_t s = dst_off[j], e = j + 1u < a.m ? dst_off[j + 1u] : total;
    const BrxTakeRec r = brx_take_entry_record(mem, a, j);
    const uint64_t room = e > s ? e - s : 0;
    d.start = s + phase;
    d.src = r.src;
    d.cnt = r.len < room ? r.len : room;
    return d;
}

// the last e in [0, 64) with start[e] <= y, or 0 when there is none (the window's starts are non-decreasing)
BRX_TAKE_HD uint32_t brx_take_window_find(const uint64_t *start, uint64_t y) {
    uint32_t lo = 0, hi = BRX_TAKE_WINDOW;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (start[mid] <= y) lo = mid; else hi = mid;
    }
    return lo;
}

// How far the window that starts at entry jw serves the chunk, and where the next window starts (wave-uniform).  `g` is the first byte
// (in y) not served yet, `hi` the chunk's end, `next_start` = dst_off[jw + 64] + phase where that entry exists, else BRX_TAKE_NONE.
// The window serves [g, wend).  Where the window ends inside the chunk and inside a unit, wend is taken back to the unit's first byte
// and the next window starts at the entry owning that byte, so that the unit is assembled whole and stored as one dwordx4 -- unless
// that would not advance (63 entries starting inside one unit): then the unit is split and stored by the byte.
BRX_TAKE_HD void brx_take_window_end(const uint64_t *start, uint64_t g, uint64_t hi, uint64_t next_start, uint64_t jw, uint64_t &wend,
                                     uint64_t &jnext) {
    wend = next_start < hi ? next_start : hi;
    jnext = jw + BRX_TAKE_WINDOW;
    if (wend < g) wend = g;
    if (wend < hi) {
        const uint64_t wr = wend & ~(uint64_t)(BRX_TAKE_UNIT - 1u);
        if (wr > g && wr < wend) {
            const uint32_t p = brx_take_window_find(start, wr);
            if (p > 0 && start[p] <= wr) {
                wend = wr;
                jnext = jw + p;
            }
        }
    }
}

// n <= 16 bytes from p, as the low n bytes of a unit.  One unaligned 16-byte load where all 16 lie inside the arena [lo, hi), else
// by the byte.
template <class M>
BRX_TAKE_HD BrxTake128 brx_take_fetch(M &mem, const uint8_t *p, uint32_t n, const uint8_t *arena_lo, const uint8_t *arena_hi) {
    BrxTake128 v = {0, 0};
    if (p >= arena_lo && p <= arena_hi && (uint64_t)(arena_hi - p) >= 16u) {
        v = mem.ld128(p);
    } else {
        for (uint32_t t = 0; t < 16u; t++) {
            if (t < n) {
                const uint64_t b = mem.ld8(p + t);
                if (t < 8u) v.lo |= b << (8u * t); else v.hi |= b << (8u * (t - 8u));
            }
        }
    }
    return v;
}

// bytes [0, n) of v moved to bytes [q, q + n) of a unit, everything else 0 (q < 16, 1 <= n, q + n <= 16)
BRX_TAKE_HD BrxTake128 brx_take_place(BrxTake128 v, uint32_t q, uint32_t n) {
    if (n < 8u) { v.lo &= ((uint64_t)1 << (8u * n)) - 1u; v.hi = 0; }
    else if (n < 16u) v.hi &= ((uint64_t)1 << (8u * (n - 8u))) - 1u;
    BrxTake128 r;
    if (q == 0) r = v;
    else if (q < 8u) { r.lo = v.lo << (8u * q); r.hi = (v.hi << (8u * q)) | (v.lo >> (64u - 8u * q)); }
    else { r.lo = 0; r.hi = v.lo << (8u * (q - 8u)); }
    return r;
}

// One lane, one unit: the destination bytes y in [u, u + 16) that the window serves, [g, wend) being the window's range.  Finds the
// unit's first entry among the 64 resident descriptors, gathers the unit's bytes from as many entries as it spans, and stores an
// aligned 16 bytes when all 16 are covered, else the covered bytes one by one.  Returns the mask of bytes written (for the emulator).
template <class M>
BRX_TAKE_HD uint32_t brx_take_unit(M &mem, const uint64_t *start, const uint64_t *src, const uint64_t *cnt, uint64_t u, uint64_t g,
                                   uint64_t wend, const uint8_t *arena, uint64_t span, uint8_t *dst_al) {
    const uint64_t a = u > g ? u : g, b = u + BRX_TAKE_UNIT < wend ? u + BRX_TAKE_UNIT : wend;
    if (a >= b) return 0;
    uint32_t e = brx_take_window_find(start, a);
    BrxTake128 acc = {0, 0};
    uint32_t mask = 0;
    uint64_t x = a;
    while (x < b && e < BRX_TAKE_WINDOW) {
        const uint64_t ds = start[e], nx = e + 1u < BRX_TAKE_WINDOW ? start[e + 1u] : BRX_TAKE_NONE;
        if (ds >= b) break;    // (also the entries behind the selection's end: their start is BRX_TAKE_NONE)
        if (nx <= x) { e++; continue; } // an empty room, or one that ends in front of x: the byte belongs to a later entry
        const uint64_t seg_end = nx < b ? nx : b;
        const uint64_t c0 = x > ds ? x : ds, c1 = ds + cnt[e] < seg_end ? ds + cnt[e] : seg_end;
        if (c0 < c1) {
            const uint32_t q = (uint32_t)(c0 - u), nb = (uint32_t)(c1 - c0);
            const BrxTake128 v = brx_take_place(brx_take_fetch(mem, arena + src[e] + (c0 - ds), nb, arena, arena + span), q, nb);
            acc.lo |= v.lo;
            acc.hi |= v.hi;
            mask |= ((1u << nb) - 1u) << q;
        }
        x = seg_end;
        e++;
    }
    if (mask == 0xFFFFu) {
        mem.st128(dst_al + u, acc);
    } else {
        for (uint32_t t = 0; t < 16u; t++)
            if ((mask >> t) & 1u) mem.st8(dst_al + u + t, (uint8_t)((t < 8u ? acc.lo >> (8u * t) : acc.hi >> (8u * (t - 8u))) & 0xFFu));
    }
    return mask;
}

// host side (brx_api.cpp)
void brx_launch_take_size(const BrxTakeArgs &a, uint64_t *rec_len, void *hip_stream);
void brx_launch_take_fill(const BrxTakeArgs &a, const uint64_t *dst_off, uint8_t *dst, uint64_t total, void *hip_stream);
static inline uint64_t brx_take_chunks(uint64_t total, const void *dst) {
    return (total + ((uint64_t)(uintptr_t)dst & 15u) + BRX_TAKE_CHUNK - 1u) / BRX_TAKE_CHUNK;
}
#endif
