// hash_emu.cpp -- brx_hash_batch on a CPU, lane by lane: the lane path (brx_hash_lane) and the wave path (the loop of brx_hash_kernel,
// csrc/brx_hash.hip, with its 64 lanes in turn and its shuffles as array reads) around the REAL text of csrc/brx_hash.h and
// csrc/brx_take.h, held to a byte-serial restatement of the definition of include/brx.h in unsigned __int128 that shares nothing with
// either header.  BOTH paths are run on EVERY record, whatever its length, so each is checked on all lengths 0 .. 2 * 1024 + 40 at
// all 16 source phases (the run fails if one combination was not met), on records that start on the arena's first byte and end on
// its last, in both selection modes, under the three flag combinations and with stale positions.
// Every emulated arena load is recorded and the run fails if one lies outside [out, out + span): this is the check of the
// contract's "never loaded" clause, which a GPU test cannot see.
// No GPU.  Build and run: g++ -O2 -std=c++17 -I brotli-rs_amd/csrc tools/hash_emu.cpp -o hash_emu && ./hash_emu
// (tests/test_hash_abi.py does).  It proves the arithmetic, not the kernel's own text: that is tests/test_gpu_hash.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <random>
#include "brx_hash.h"
typedef std::vector<uint8_t> Bytes;
typedef unsigned __int128 u128;

static const uint8_t *A_LO, *A_HI; // the arena
static uint64_t n_wide_loads, n_byte_loads;
static void die(const char *what) { printf("FAIL: %s\n", what); exit(1); }

struct EmuMem {
    uint8_t ld8(const uint8_t *p) {
        if (p < A_LO || p >= A_HI) die("byte load outside the arena");
        n_byte_loads++;
        return *p;
    }
    BrxTake128 ld128(const uint8_t *p) {
        if (p < A_LO || p + 16 > A_HI) die("16-byte load outside the arena");
        n_wide_loads++;
        BrxTake128 v;
        memcpy(&v.lo, p, 8);
        memcpy(&v.hi, p + 8, 8);
        return v;
    }
};

// the sum across the wave as the kernel's xor-shuffles form it
static uint64_t emu_wave_sum(uint64_t *x) {
    uint64_t y[64];
    for (uint32_t d = 32; d > 0; d >>= 1) {
        for (uint32_t l = 0; l < 64u; l++) y[l] = brx_hash_add(x[l], x[l ^ d]);
        memcpy(x, y, sizeof(y));
    }
    for (uint32_t l = 1; l < 64u; l++) if (x[l] != x[0]) die("the lanes disagree on a row sum");
    return x[0];
}

// the body of the loop over the long records in brx_hash_kernel, for one record of L >= 1 bytes
static uint64_t emu_wave(const BrxTakeArgs &a, BrxTakeRec r, const BrxHashKeys &k, const uint64_t *W) {
    EmuMem mem;
    const BrxHashShape s = brx_hash_shape(r.len);
    uint64_t acc = 0, t[64];
    const uint64_t kg = brx_hash_group_stride(k);
    uint64_t row = 0;
    for (; row + BRX_HASH_GROUP < s.rows; row += BRX_HASH_GROUP) {
        for (uint32_t lane = 0; lane < 64u; lane++) t[lane] = brx_hash_group_term(mem, a.out, r.src, row, lane, W[lane], k);
        acc = brx_hash_red(brx_hash_mul(acc, kg) + brx_hash_red(emu_wave_sum(t)));
    }
    for (; row + 1u < s.rows; row++) {
        for (uint32_t lane = 0; lane < 64u; lane++) t[lane] = brx_hash_row_term(mem, a.out, a.span, r.src, row, lane, W[lane], k);
        acc = brx_hash_red(brx_hash_mul(acc, k.k256) + brx_hash_red(emu_wave_sum(t)));
    }
    BrxTake128 v[64];
    for (uint32_t lane = 0; lane < 64u; lane++)
        t[lane] = brx_hash_last_term(mem, a.out, a.span, r.src, s, lane, W[brx_hash_last_weight_lane(lane, s.nu)], acc, k, v[lane]);
    const uint64_t X = brx_hash_red(emu_wave_sum(t));
    return brx_hash_finish(brx_hash_tail(X, v[s.nu - 1u], s.n, k), r.len);
}

// ---- the definition, serially, with nothing shared with brx_hash.h or brx_take.h ---------------------------------------------------
static const uint64_t P61 = (((uint64_t)1) << 61) - 1;
static uint64_t ref_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
static uint64_t ref_key(uint64_t seed) { return 2 + ref_mix(seed + 0x9E3779B97F4A7C15ull) % (P61 - 3); }
static uint64_t ref_pow(uint64_t b, uint64_t e) {
    u128 r = 1;
    for (uint64_t t = 0; t < e; t++) r = r * b % P61;
    return (uint64_t)r;
}
static uint64_t ref_hash(const uint8_t *r, uint64_t L, uint64_t K) {
    u128 acc = 0; // Horner over the words: ((c_0 K + c_1) K + ...) K
    for (uint64_t u = 0; u < (L + 3) / 4; u++) {
        uint64_t c = 0;
        for (uint64_t t = 0; t < 4; t++) if (4 * u + t < L) c |= (uint64_t)r[4 * u + t] << (8 * t);
        acc = (acc + c) * K % P61;
    }
    return ref_mix((uint64_t)((acc + L) % P61));
}

struct Batch {
    uint8_t *arena; // (allocated: its address sets the phases)
    uint64_t span;
    std::vector<uint64_t> off, len, count, pos_off, pos;
    uint64_t n_pos;
    uint32_t D, flags;
};
static void serial_record(const Batch &b, uint64_t i, uint64_t k, uint64_t &src, uint64_t &L) {
    src = 0; L = 0;
    if (i >= b.off.size() || k > b.count[i]) return;
    const uint64_t l = b.len[i];
    auto P = [&](uint64_t kk) -> uint64_t {
        uint64_t idx = b.pos_off[i] + kk;
        if (idx >= b.n_pos) return l;
        return b.pos[idx] < l ? b.pos[idx] : l;
    };
    uint64_t start = 0, end;
    if (k > 0) { start = P(k - 1) + b.D; if (start > l) start = l; }
    if (k < b.count[i]) {
        end = P(k);
        if (!(b.flags & 1u)) { end += b.D; if (end > l) end = l; }
    } else end = l;
    if (end < start) end = start;
    if ((b.flags & 2u) && end > start && b.arena[b.off[i] + end - 1] == 13) end--;
    src = b.off[i] + start; L = end - start;
}

#define MAXLEN (2u * BRX_HASH_LONG + 40u)
static uint8_t covered[MAXLEN + 1][16][2]; // [L][phase of the first byte][path]
static uint64_t n_records, n_bytes, n_long;

// one call: every entry through both paths and the serial walk
static void run(const Batch &b, bool pairs, const std::vector<uint32_t> &ss, const std::vector<uint64_t> &sr, uint64_t m, uint64_t seed, int it) {
    const uint32_t n = (uint32_t)b.off.size();
    BrxTakeArgs a;
    a.out = b.arena; a.out_off = b.off.data(); a.len = b.len.data(); a.n = n; a.span = b.span;
    a.count = b.count.data(); a.pos_off = b.pos_off.data(); a.pos = b.pos.empty() ? nullptr : b.pos.data(); a.n_pos = b.n_pos;
    a.delim_len = b.D; a.flags = b.flags;
    a.sel_stream = pairs ? ss.data() : nullptr; a.sel_rec = pairs ? sr.data() : nullptr; a.m = m;
    A_LO = b.arena; A_HI = A_LO + b.span;
    const BrxHashKeys k = brx_hash_keys(seed);
    const uint64_t K = ref_key(seed);
    if (k.k1 != K || k.k2 != ref_pow(K, 2) || k.k3 != ref_pow(K, 3) || k.k4 != ref_pow(K, 4) || k.k256 != ref_pow(K, 256)) die("the key's powers");
    uint64_t W[64];
    for (uint32_t lane = 0; lane < 64u; lane++) {
        W[lane] = brx_hash_lane_weight(k, lane);
        if (W[lane] != ref_pow(K, 4 * (63 - lane))) die("a lane's weight");
    }
    EmuMem mem;
    for (uint64_t j = 0; j < m; j++) {
        uint64_t i = n, kk = 0, src, L;
        if (pairs) { i = ss[j]; kk = sr[j]; }
        else for (uint32_t t = 0; t < n; t++) if (b.pos_off[t] + t <= j) { i = t; kk = j - (b.pos_off[t] + t); }
        serial_record(b, i, kk, src, L);
        const uint64_t want = ref_hash(b.arena + src, L, K);
        if (L == 0 && want != 0) die("the empty record does not hash to 0");
        const BrxTakeRec r = brx_take_entry_record(mem, a, j);
        if (r.len != L || (L && r.src != src)) { printf("FAIL: it %d entry %llu: the record\n", it, (unsigned long long)j); exit(1); }
        const uint64_t lane_h = brx_hash_lane(mem, a.out, a.span, r, k);
        const uint64_t wave_h = L ? emu_wave(a, r, k, W) : 0;
        if (lane_h != want || wave_h != want) {
            printf("FAIL: it %d entry %llu (L %llu, phase %u, flags %u, pairs %d): lane path %016llx, wave path %016llx, want %016llx\n", it,
                   (unsigned long long)j, (unsigned long long)L, (unsigned)((uintptr_t)(b.arena + src) & 15u), b.flags, (int)pairs,
                   (unsigned long long)lane_h, (unsigned long long)wave_h, (unsigned long long)want);
            exit(1);
        }
        if (L <= MAXLEN) {
            const uint32_t ph = (uint32_t)((uintptr_t)(b.arena + src) & 15u);
            covered[L][ph][0] = covered[L][ph][1] = 1;
        }
        n_records++; n_bytes += L; n_long += L >= BRX_HASH_LONG;
    }
}

int main() {
    std::mt19937_64 rng(20260117);
    auto rnd = [&](uint64_t m) { return (uint64_t)(rng() % m); };
    const uint32_t Ds[3] = {1, 2, 16}, FL[3] = {0, 1, 3};
    // the multiplication against 128-bit arithmetic, operands at the edges among them
    for (int t = 0; t < 200000; t++) {
        uint64_t x = rng() % (P61 + 5), y = rng() % P61;
        if (t % 7 == 0) x = P61 - 1 - rnd(3);
        if (t % 11 == 0) y = P61 - 1 - rnd(3);
        if (t % 13 == 0) x = rnd(3);
        if (brx_hash_mul(x, y) != (uint64_t)((u128)x * y % P61)) die("brx_hash_mul");
        if (brx_hash_red(rng()) >= P61) die("brx_hash_red");
    }
    uint64_t batches = 0;
    uint8_t *raw = (uint8_t *)aligned_alloc(64, (size_t)1 << 23);
    // PART 0: check values of the contract, as whole streams (count = 0), so that the serial walk itself is held to the table
    {
        struct { const char *r; uint64_t L, seed, want; } cv[] = {
            {"a", 1, 0, 0xba350051cabf3ed3ull}, {"a\0", 2, 0, 0xbb6016563a245ebaull}, {"abcd", 4, 0, 0xada6cd48c13c1c39ull},
            {"abcde", 5, 1, 0x78061f9a959b2150ull}, {"hello, world\n", 13, 1, 0x6879e40593ee90c8ull},
            {"hello, world\n", 13, ~(uint64_t)0, 0x4e8c2d5bfbc9d732ull}, {nullptr, 256, 0, 0x5bb278495e403ce2ull},
            {nullptr, 256, ~(uint64_t)0, 0x0bc6190075701881ull}};
        for (auto &c : cv) {
            Batch b;
            b.arena = raw + 64 + rnd(16);
            for (uint64_t t = 0; t < c.L; t++) b.arena[t] = c.r ? (uint8_t)c.r[t] : (uint8_t)t;
            b.span = c.L; b.D = 1; b.flags = 0; b.n_pos = 0;
            b.off.push_back(0); b.len.push_back(c.L); b.count.push_back(0); b.pos_off.push_back(0);
            if (ref_hash(b.arena, c.L, ref_key(c.seed)) != c.want) die("a check value of the contract");
            run(b, false, {}, {}, 1, c.seed, -1);
            batches++;
        }
    }
    // PART 1: one stream that is the whole arena, records of every length 0 .. MAXLEN + 1 in order, at each phase of the arena: the
    // first record starts on the arena's first byte, the last one ends on its last
    for (int it = 0; it < 48; it++) {
        Batch b;
        const uint32_t phase = it % 16;
        b.D = 1; b.flags = FL[(it / 16) % 3];
        const bool pairs = it % 2;
        b.arena = raw + 64 + phase;
        uint64_t at = 0;
        b.pos_off.push_back(0);
        for (uint32_t L = 0; L <= MAXLEN + 1u; L++) {
            for (uint32_t t = 0; t < L; t++) { uint8_t c = (uint8_t)rng(); b.arena[at++] = c == 10 ? 11 : c; }
            if (L && rnd(3) == 0) b.arena[at - 1] = 13;
            if (L <= MAXLEN) { b.pos.push_back(at); b.arena[at++] = 10; }
        }
        b.span = at;
        b.off.push_back(0); b.len.push_back(at); b.count.push_back(b.pos.size());
        b.n_pos = b.pos.size();
        std::vector<uint32_t> ss; std::vector<uint64_t> sr;
        uint64_t m = b.pos.size() + 1;
        if (pairs) for (uint64_t j = 0; j < m; j++) { ss.push_back(0); sr.push_back(m - 1 - j); }
        run(b, pairs, ss, sr, m, it < 3 ? (uint64_t)0 - it : rng(), it);
        batches++;
    }
    // PART 2: random batches of several streams in slots with slack (the first stream on the arena's first byte, the last one up to
    // its last), dense and sparse delimiters, D in {1, 2, 16}, stale positions
    for (int it = 0; it < 360; it++) {
        Batch b;
        b.D = Ds[it % 3];
        b.flags = FL[(it / 3) % 3];
        const bool pairs = (it / 9) % 2;
        const int stale = (it / 18) % 5 == 4;
        const int text = (it / 7) % 3; // 0 dense delimiters (tiny records), 1 lines, 2 long records among short ones
        const uint32_t n = 1 + (uint32_t)rnd(6);
        b.arena = raw + 64 + rnd(16);
        uint64_t at = 0;
        b.off.resize(n); b.len.resize(n); b.count.resize(n); b.pos_off.resize(n);
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t l = rnd(8) == 0 ? 0 : (text == 2 ? rnd(11 * BRX_HASH_LONG) : rnd(700));
            const uint32_t dens = text == 0 ? 2 : (text == 1 ? 30 : 1500);
            b.off[i] = at; b.len[i] = l;
            for (uint64_t t = 0; t < l; t++) {
                uint64_t r = rnd(dens);
                b.arena[at++] = r == 0 ? 10 : (r == 1 || rnd(9) == 0 ? 13 : (uint8_t)rng());
            }
            if (i + 1 < n) for (uint64_t t = rnd(20); t > 0; t--) b.arena[at++] = 13; // slack: CRs, so that a stray trim would show
        }
        if (at == 0) b.arena[at++] = 13;
        b.span = at;
        for (uint32_t i = 0; i < n; i++) {
            b.pos_off[i] = b.pos.size();
            for (uint64_t j = 0; j + b.D <= b.len[i]; j++) {
                bool hit = true;
                for (uint32_t t = 0; t < b.D && hit; t++) hit = b.arena[b.off[i] + j + t] == 10;
                if (b.D == 16 && !hit && rnd(40) == 0) hit = true;
                if (hit) b.pos.push_back(j);
            }
            b.count[i] = b.pos.size() - b.pos_off[i];
        }
        b.n_pos = b.pos.size();
        if (stale) {
            for (auto &p : b.pos) { uint64_t r = rnd(4); if (r == 0) p = rnd(2000); else if (r == 1) p = ~(uint64_t)0 - rnd(3); }
            if (rnd(2)) b.n_pos = rnd(b.pos.size() + 1);
            if (rnd(2)) for (uint32_t i = 0; i < n; i++) b.count[i] += rnd(3);
        }
        std::vector<uint32_t> ss; std::vector<uint64_t> sr;
        uint64_t m;
        if (pairs) {
            m = 1 + rnd(text == 0 ? 900 : 200);
            for (uint64_t j = 0; j < m; j++) {
                uint32_t i = (uint32_t)rnd(n);
                ss.push_back(rnd(25) == 0 ? n + (uint32_t)rnd(3) : i);
                sr.push_back(rnd(25) == 0 ? b.count[i] + 1 + rnd(3) : rnd(b.count[i] + 1));
            }
        } else {
            m = 0;
            for (uint32_t i = 0; i < n; i++) m += b.count[i] + 1;
            if (stale) m += rnd(4);
        }
        run(b, pairs, ss, sr, m, rng(), 1000 + it);
        batches++;
    }
    for (uint32_t L = 0; L <= MAXLEN; L++)
        for (uint32_t ph = 0; ph < 16u; ph++)
            if (!covered[L][ph][0] || !covered[L][ph][1]) { printf("FAIL: length %u at phase %u was not met\n", L, ph); return 1; }
    free(raw);
    printf("OK: %llu batches, %llu records (%llu of %u bytes and more), %llu bytes, each by the lane path and by the wave path; every length 0 .. %u at "
           "all 16 phases; loads %llu wide + %llu byte, none outside\n",
           (unsigned long long)batches, (unsigned long long)n_records, (unsigned long long)n_long, BRX_HASH_LONG, (unsigned long long)n_bytes,
           MAXLEN, (unsigned long long)n_wide_loads, (unsigned long long)n_byte_loads);
    return 0;
}
