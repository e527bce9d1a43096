// index_set_emu.cpp -- brx_index_set_batch on a CPU, lane by lane: tools/index_escaped_emu.cpp with what the set pass changes in the
// row body of csrc/brx_index_escaped.hip -- the union mask over 1 .. 8 delimiter bytes, the `lead` class "a byte of the set", the escape
// switched off as the quote is, the filler that walks past every byte in use, and `what` next to every position -- around the REAL
// arithmetic of csrc/brx_index_escaped.h (ie_escaped, ie_tile_map, ie_select, ie_compose), held to the serial rule of include/brx.h on
// 480 random batches of 1 .. 6 streams (uniform, escape-heavy, escape-only and long-run texts, all four flag combinations, sets of
// 1 .. 8 bytes that start at 0 so that the filler has to walk, lengths around every tile edge).
// No GPU.  Build and run: g++ -O2 -std=c++17 -I brotli-rs_amd/csrc tools/index_set_emu.cpp -o is_emu && ./is_emu
// (tests/test_index_set_abi.py does).  It proves the bit arithmetic, not the kernels' own text: that is tests/test_gpu_index_set.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <random>
#include "brx_index_escaped.h"
typedef std::vector<uint8_t> Bytes;
static uint8_t Q = 34, E = 92, F = 0;
static uint64_t SET = 10;
static uint32_t ND = 1;
static bool quotes = true, escapes = true;

static bool in_set(uint8_t b) {
    for (uint32_t k = 0; k < ND; k++) if (b == (uint8_t)(SET >> (8 * k))) return true;
    return false;
}
// ix_filler of the kernels (brx_index.h)
static uint8_t filler() {
    uint32_t f = 0;
    for (;;) {
        bool hit = (quotes && f == Q) || (escapes && f == E);
        for (uint32_t k = 0; k < ND; k++) hit = hit || f == ((uint32_t)(SET >> (8 * k)) & 0xFF);
        if (!hit) break;
        f++;
    }
    return (uint8_t)f;
}

struct Lane { uint32_t em, qm, dm; uint8_t v[16]; };
static int clzll(uint64_t x) { return __builtin_clzll(x); }
struct RowOut { uint32_t esc[64], in[64]; uint64_t some; };
static void row_eval(const Lane *L, uint32_t &re, uint32_t &rp, RowOut &o) {
    uint64_t a = 0, t = 0;
    for (int l = 0; l < 64; l++) {
        bool mixed = L[l].em != 0xFFFFu;
        uint32_t x = ~L[l].em << 16;
        uint32_t trail = (x ? __builtin_clz(x) : 32) & 1u;
        if (mixed) a |= 1ull << l;
        if (mixed && trail) t |= 1ull << l;
    }
    uint32_t xs[64]; uint64_t b = 0;
    for (int l = 0; l < 64; l++) {
        uint64_t below = a & ((1ull << l) - 1ull);
        uint32_t c = below ? (uint32_t)(t >> (63 - clzll(below))) & 1u : re;
        o.esc[l] = ie_escaped(L[l].em, c) & 0xFFFFu;
        uint32_t x = L[l].qm & ~o.esc[l];
        x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8;
        xs[l] = x;
        if ((x >> 15) & 1u) b |= 1ull << l;
    }
    if (a) re = (uint32_t)(t >> (63 - clzll(a))) & 1u;
    o.some = a;
    for (int l = 0; l < 64; l++) {
        uint32_t before = __builtin_popcountll(b & ((1ull << l) - 1ull));
        uint32_t carry = (before ^ rp) & 1u;
        o.in[l] = (xs[l] ^ (0u - carry)) & 0xFFFFu;
    }
    rp ^= __builtin_popcountll(b) & 1u;
}
// mem: flat address space; stream [a, e).  The masks as the kernels form them: escape and quote masks forced to 0 by the flags, the
// delimiter mask the union over the set.
static void load_row(const Bytes &mem, uint64_t row, uint64_t a, uint64_t e, Lane *L) {
    for (int l = 0; l < 64; l++) {
        L[l].em = L[l].qm = L[l].dm = 0;
        for (int k = 0; k < 16; k++) {
            uint64_t ad = row + 16 * l + k;
            uint8_t b = (ad >= a && ad < e) ? mem[ad] : F;
            L[l].v[k] = b;
            if (escapes && b == E) L[l].em |= 1u << k;
            if (quotes && b == Q) L[l].qm |= 1u << k;
            for (uint32_t d = 0; d < ND; d++) if (b == (uint8_t)(SET >> (8 * d))) L[l].dm |= 1u << k;
        }
    }
}
int main() {
    std::mt19937_64 rng(2);
    for (int iter = 0; iter < 480; iter++) {
        quotes = (iter & 1) == 0;
        escapes = (iter & 2) == 0;
        int heavy = (iter >> 2) % 4;
        // the set: 1 .. 8 distinct bytes; every third one starts at 0, 1, 2 ... so that the filler has to walk past them
        ND = 1 + rng() % 8;
        SET = 0;
        Q = 34; E = 92;
        if (iter % 3 == 0) {
            for (uint32_t k = 0; k < ND; k++) SET |= (uint64_t)k << (8 * k);
            Q = (uint8_t)ND; E = (uint8_t)(ND + 1); // (filler: ND, ND + 1 or ND + 2 by the flags)
        } else {
            const uint8_t pool[8] = {10, 44, 13, 0x7F, 0x80, 0xFF, 0, 9};
            uint32_t start = rng() % 8;
            for (uint32_t k = 0; k < ND; k++) SET |= (uint64_t)pool[(start + k) % 8] << (8 * k);
        }
        F = filler();
        if (in_set(F) || (quotes && F == Q) || (escapes && F == E)) { printf("iter %d: filler %u is in use\n", iter, F); return 1; }
        uint32_t n = 1 + rng() % 6;
        std::vector<uint64_t> off(n), len(n);
        uint64_t at = rng() % 3000;
        for (uint32_t i = 0; i < n; i++) {
            off[i] = at;
            int kind = rng() % 6;
            len[i] = kind == 0 ? 0 : kind == 1 ? rng() % 40 : kind == 2 ? rng() % 3000 : kind == 3 ? 65536 - 20 + rng() % 40 : rng() % 200000;
            if (iter % 7 == 0 && i == 1) len[i] = 3 * 65536;
            at += len[i] + (rng() % 3 ? rng() % 40 : 0);
        }
        Bytes mem(at + 2048);
        // alphabet: the set, Q, E and one other byte
        uint8_t alpha[11]; uint32_t na = 0;
        for (uint32_t k = 0; k < ND; k++) alpha[na++] = (uint8_t)(SET >> (8 * k));
        alpha[na++] = Q; alpha[na++] = E; alpha[na++] = 'x';
        for (auto &b : mem) b = alpha[rng() % (na - 1)];
        for (uint32_t i = 0; i < n; i++) {
            bool longruns = rng() % 2;
            uint64_t j = 0;
            while (j < len[i]) {
                if (heavy == 0) mem[off[i] + j++] = alpha[rng() % na];
                else if (heavy == 1) mem[off[i] + j++] = (rng() % 5) ? E : alpha[rng() % na];
                else if (heavy == 2) mem[off[i] + j++] = E;
                else { // long runs
                    uint64_t k = longruns ? rng() % 140000 : rng() % 70;
                    while (k-- && j < len[i]) mem[off[i] + j++] = E;
                    if (j < len[i]) mem[off[i] + j++] = alpha[rng() % na];
                }
            }
            if (heavy == 2 && len[i] > 3 && rng() % 2) mem[off[i] + rng() % len[i]] = alpha[rng() % na];
        }
        // serial
        std::vector<std::vector<uint64_t>> want(n); std::vector<Bytes> wwhat(n); std::vector<uint32_t> wopen(n);
        for (uint32_t i = 0; i < n; i++) {
            uint32_t esc = 0, q = 0;
            for (uint64_t j = 0; j < len[i]; j++) {
                uint8_t b = mem[off[i] + j];
                if (!esc && in_set(b) && !q) { want[i].push_back(j); wwhat[i].push_back(b); }
                if (!esc && quotes && b == Q) q ^= 1;
                esc = (escapes && b == E && !esc);
            }
            wopen[i] = q | esc << 1;
        }
        // plan
        std::vector<uint64_t> pre(n + 1);
        pre[0] = 0;
        for (uint32_t i = 0; i < n; i++) pre[i + 1] = pre[i] + (len[i] ? ((off[i] & 1023) + len[i] + 65535) / 65536 : 0);
        uint64_t total = pre[n];
        std::vector<uint64_t> word(total + 1), ex(total);
        auto item_of = [&](uint64_t item, uint32_t &si, uint64_t &a, uint64_t &e, uint64_t &t0, uint64_t &t1, uint32_t &rows) {
            si = 0; for (uint32_t i = 0; i < n; i++) if (pre[i] <= item) si = i;
            a = off[si]; e = a + len[si]; t0 = (a & ~1023ull) + (item - pre[si]) * 65536; t1 = t0 + 65536 < e ? t0 + 65536 : e;
            rows = (t1 - t0 + 1023) / 1024;
        };
        // count
        for (uint64_t item = 0; item < total; item++) {
            uint32_t si, rows; uint64_t a, e, t0, t1; item_of(item, si, a, e, t0, t1, rows);
            uint32_t all = 0, odd = 0, rp = 0, re = 0, lead = 4, rodd = 0; Lane L[64]; RowOut o; uint64_t row = t0;
            for (uint32_t r = 0; r < rows; r++) {
                row = t0 + r * 1024ull; load_row(mem, row, a, e, L); row_eval(L, re, rp, o);
                if (lead == 4 && o.some) {
                    uint32_t fl = __builtin_ffsll(o.some) - 1;
                    uint32_t k = __builtin_ffs(~L[fl].em & 0xFFFF) - 1;
                    uint32_t got = (k & 15) | ((L[fl].dm >> (k & 15) & 1) << 4) | ((L[fl].qm >> (k & 15) & 1) << 5);
                    rodd = got & 1; lead = row + 16 * fl + (got & 15) >= e ? 3 : got >> 4;
                }
                for (int l = 0; l < 64; l++) { uint32_t m = L[l].dm & ~o.esc[l]; all += __builtin_popcount(m); odd += __builtin_popcount(m & o.in[l]); }
            }
            if (lead == 4) lead = 3;
            uint32_t atb = (uint32_t)(t1 - 1 - row);
            uint32_t x = ((L[atb >> 4].em & ~o.esc[atb >> 4]) >> (atb & 15)) & 1;
            word[item] = (uint64_t)(all - odd) | ((uint64_t)odd << BRX_IE_C0_BITS) | ((uint64_t)rp << BRX_IE_PAR_SHIFT) | ((uint64_t)x << BRX_IE_X_SHIFT) |
                         ((uint64_t)lead << BRX_IE_LEAD_SHIFT) | ((uint64_t)rodd << BRX_IE_RODD_SHIFT);
        }
        // resolve, 1024 emulated threads
        {
            uint64_t per = (total + 1023) / 1024;
            std::vector<uint32_t> maps(1024);
            auto sof = [&](uint64_t item) { uint32_t lo = 0, hi = n; while (hi - lo > 1) { uint32_t mid = lo + (hi - lo) / 2; if (pre[mid] <= item) lo = mid; else hi = mid; } return lo; };
            for (uint32_t t = 0; t < 1024; t++) {
                uint64_t i0 = per * t < total ? per * t : total, i1 = i0 + per < total ? i0 + per : total;
                uint32_t si = i0 < i1 ? sof(i0) : 0, map = BRX_IE_MAP_IDENTITY;
                for (uint64_t i = i0; i < i1; i++) { while (si + 1 < n && pre[si + 1] <= i) si++; map = ie_compose(map, ie_tile_map(word[i], pre[si] == i)); }
                maps[t] = map;
            }
            for (uint32_t s = 1; s < 1024; s <<= 1) { std::vector<uint32_t> nx(1024); for (uint32_t t = 0; t < 1024; t++) nx[t] = ie_compose(t >= s ? maps[t - s] : BRX_IE_MAP_IDENTITY, maps[t]); maps = nx; }
            for (uint32_t t = 0; t < 1024; t++) {
                uint64_t i0 = per * t < total ? per * t : total, i1 = i0 + per < total ? i0 + per : total;
                uint32_t si = i0 < i1 ? sof(i0) : 0, state = t ? ie_apply(maps[t - 1], 0) : 0;
                for (uint64_t i = i0; i < i1; i++) {
                    while (si + 1 < n && pre[si + 1] <= i) si++;
                    uint64_t w = word[i]; int first = pre[si] == i; if (first) state = 0;
                    uint64_t c = ie_select(w, state); word[i] = c | ((uint64_t)state << BRX_IE_ENTRY_SHIFT);
                    state = ie_apply(ie_tile_map(w, first), state); ex[i] = state;
                }
            }
            uint64_t run = 0;
            for (uint64_t i = 0; i < total; i++) { uint64_t w = word[i]; word[i] = run | (w & ~BRX_IE_G_MASK); run += w & BRX_IE_G_MASK; }
            word[total] = run;
        }
        for (uint32_t i = 0; i < n; i++) {
            uint64_t a = pre[i], b = pre[i + 1];
            uint64_t cnt = (word[b] & BRX_IE_G_MASK) - (word[a] & BRX_IE_G_MASK);
            uint32_t op = b > a ? (uint32_t)ex[b - 1] : 0;
            if (cnt != want[i].size() || op != wopen[i]) { printf("iter %d stream %u len %llu: count %llu want %zu open %u want %u\n", iter, i, (unsigned long long)len[i], (unsigned long long)cnt, want[i].size(), op, wopen[i]); return 1; }
            if ((!quotes && (op & 1)) || (!escapes && (op & 2))) { printf("iter %d stream %u: open %u has a bit its flag switches off\n", iter, i, op); return 1; }
        }
        // fill
        for (uint64_t item = 0; item < total; item++) {
            uint32_t si, rows; uint64_t a, e, t0, t1; item_of(item, si, a, e, t0, t1, rows);
            uint64_t w = word[item], base = (w & BRX_IE_G_MASK) - (word[pre[si]] & BRX_IE_G_MASK);
            uint32_t rp = (w >> 62) & 1, re = (w >> 63) & 1; Lane L[64]; RowOut o;
            for (uint32_t r = 0; r < rows; r++) {
                uint64_t row = t0 + r * 1024ull; load_row(mem, row, a, e, L); row_eval(L, re, rp, o);
                for (int l = 0; l < 64; l++) { uint32_t m = L[l].dm & ~o.esc[l] & ~o.in[l]; for (int k = 0; k < 16; k++) if (m >> k & 1) {
                    uint64_t p = row + 16 * l + k - a;
                    if (base >= want[si].size() || want[si][base] != p || wwhat[si][base] != L[l].v[k]) { printf("iter %d stream %u pos / what mismatch at %llu\n", iter, si, (unsigned long long)base); return 1; }
                    base++; } }
            }
        }
    }
    printf("all ok\n");
    return 0;
}
