// take_emu.cpp -- brx_take_batch on a CPU, lane by lane: the loop of brx_take_fill_kernel (csrc/brx_take.hip) around the REAL lane logic
// of csrc/brx_take.h (brx_take_record, brx_take_entry, brx_take_descriptor, brx_take_window_end, brx_take_unit), held to a serial
// byte-by-byte restatement of the rule of include/brx.h on random batches: both selection modes, all three flag combinations, D in
// {1, 2, 16}, packed and strided rooms, `total` cut short, stale positions, every phase of dst.
// Every emulated arena load is recorded and the run fails if one lies outside [out, out + span); it fails on a write at or beyond
// `total` (or in front of dst), on a 16-byte store that is not aligned, and on a destination byte written twice.  This is the check
// of the contract's "never loaded" clause: a GPU test cannot see a stray read.
// No GPU.  Build and run: g++ -O2 -std=c++17 -I brotli-rs_amd/csrc tools/take_emu.cpp -o take_emu && ./take_emu
// (tests/test_take_abi.py does).  It proves the arithmetic, not the kernels' own text: that is tests/test_gpu_take.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <random>
#include "brx_take.h"
typedef std::vector<uint8_t> Bytes;

static const uint8_t *A_LO, *A_HI; // the arena
static uint8_t *D_LO, *D_HI;       // dst[0 .. total)
static std::vector<uint8_t> written;
static uint64_t n_wide_loads, n_byte_loads, n_wide_stores, n_byte_stores;
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
    void st8(uint8_t *p, uint8_t v) {
        if (p < D_LO || p >= D_HI) die("byte store outside dst[0 .. total)");
        if (written[p - D_LO]++) die("destination byte written twice");
        n_byte_stores++;
        *p = v;
    }
    void st128(uint8_t *p, BrxTake128 v) {
        if (p < D_LO || p + 16 > D_HI) die("16-byte store outside dst[0 .. total)");
        if ((uintptr_t)p & 15u) die("16-byte store not aligned");
        for (int t = 0; t < 16; t++) if (written[p + t - D_LO]++) die("destination byte written twice");
        n_wide_stores++;
        memcpy(p, &v.lo, 8);
        memcpy(p + 8, &v.hi, 8);
    }
};

// the loop of brx_take_fill_kernel, one chunk; the 64 lanes in turn where the kernel has them side by side
static void emu_chunk(const BrxTakeArgs &a, const uint64_t *dst_off, uint8_t *dst, uint64_t total, uint64_t chunk) {
    EmuMem mem;
    uint64_t w_start[BRX_TAKE_WINDOW], w_src[BRX_TAKE_WINDOW], w_cnt[BRX_TAKE_WINDOW];
    const uint32_t phase = (uint32_t)((uintptr_t)dst & 15u);
    uint8_t *dst_al = dst - phase;
    const uint64_t c0 = chunk * BRX_TAKE_CHUNK, end = total + phase;
    uint64_t g = c0 > phase ? c0 : phase;
    const uint64_t hi = c0 + BRX_TAKE_CHUNK < end ? c0 + BRX_TAKE_CHUNK : end;
    if (g >= hi) return;
    uint64_t lo = 0, top = a.m;
    while (top - lo > 1u) {
        const uint64_t mid = lo + (top - lo) / 2u;
        if (dst_off[mid] + phase <= g) lo = mid; else top = mid;
    }
    uint64_t jw = lo;
    while (g < hi) {
        for (uint32_t lane = 0; lane < 64u; lane++) {
            const BrxTakeDesc d = brx_take_descriptor(mem, a, dst_off, total, phase, jw + lane);
            w_start[lane] = d.start; w_src[lane] = d.src; w_cnt[lane] = d.cnt;
        }
        const uint64_t next_start = jw + BRX_TAKE_WINDOW < a.m ? dst_off[jw + BRX_TAKE_WINDOW] + phase : BRX_TAKE_NONE;
        uint64_t wend, jnext;
        brx_take_window_end(w_start, g, hi, next_start, jw, wend, jnext);
        if (jnext <= jw) die("the window does not advance");
        if (wend > g) {
            const uint32_t r0 = (uint32_t)((g - c0) / BRX_TAKE_ROW), r1 = (uint32_t)((wend - 1u - c0) / BRX_TAKE_ROW);
            for (uint32_t r = r0; r <= r1; r++)
                for (uint32_t lane = 0; lane < 64u; lane++)
                    brx_take_unit(mem, w_start, w_src, w_cnt, c0 + (uint64_t)r * BRX_TAKE_ROW + lane * BRX_TAKE_UNIT, g, wend, a.out, a.span,
                                  dst_al);
        }
        g = wend;
        jw = jnext;
    }
}

// ---- the rule, serially, with nothing shared with brx_take.h ------------------------------------------------------------------------
struct Batch {
    Bytes arena;
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

int main() {
    std::mt19937_64 rng(20260101);
    auto rnd = [&](uint64_t m) { return (uint64_t)(rng() % m); };
    const uint32_t Ds[3] = {1, 2, 16}, FL[3] = {0, 1, 3};
    uint64_t cases = 0, bytes = 0;
    for (int it = 0; it < 720; it++) {
        Batch b;
        b.D = Ds[it % 3];
        b.flags = FL[(it / 3) % 3];
        const bool pairs = (it / 9) % 2, strided = (it / 18) % 2, cut = (it / 36) % 2;
        const int stale = (it / 72) % 5 == 4;               // every fifth block of 72: garbage positions
        const int text = (it / 7) % 3;                      // 0 dense delimiters (tiny records), 1 lines, 2 one long record among short ones
        const uint32_t n = 1 + (uint32_t)rnd(6);
        // the arena: the first stream starts on its first byte, the last one ends on its last
        std::vector<Bytes> s(n);
        for (uint32_t i = 0; i < n; i++) {
            uint64_t l = rnd(8) == 0 ? 0 : (text == 2 ? rnd(3 * BRX_TAKE_CHUNK + 40) : rnd(700));
            s[i].resize(l);
            const uint32_t dens = text == 0 ? 2 : (text == 1 ? 30 : 3000);
            for (auto &c : s[i]) {
                uint64_t r = rnd(dens);
                c = r == 0 ? 10 : (r == 1 || rnd(9) == 0 ? 13 : (uint8_t)(97 + rnd(4)));
            }
        }
        b.off.resize(n); b.len.resize(n); b.count.resize(n); b.pos_off.resize(n);
        for (uint32_t i = 0; i < n; i++) {
            b.off[i] = b.arena.size();
            b.len[i] = s[i].size();
            b.arena.insert(b.arena.end(), s[i].begin(), s[i].end());
            if (i + 1 < n) b.arena.resize(b.arena.size() + rnd(20), 13); // slack between the slots: CRs, so that a stray trim would show
        }
        if (b.arena.empty()) b.arena.push_back(13), b.len[n - 1] = 0;
        const uint64_t span = b.arena.size();
        // positions: occurrences of the needle (D bytes of '\n'; D = 2 and 16 overlap themselves), as brx_find_batch reports them
        for (uint32_t i = 0; i < n; i++) {
            b.pos_off[i] = b.pos.size();
            for (uint64_t j = 0; j + b.D <= b.len[i]; j++) {
                bool hit = true;
                for (uint32_t t = 0; t < b.D && hit; t++) hit = b.arena[b.off[i] + j + t] == 10;
                if (b.D == 16 && !hit && rnd(40) == 0) hit = true; // (a 16-byte needle hardly occurs: take arbitrary places)
                if (hit) b.pos.push_back(j);
            }
            b.count[i] = b.pos.size() - b.pos_off[i];
        }
        b.n_pos = b.pos.size();
        if (stale) {
            for (auto &p : b.pos) { uint64_t r = rnd(4); if (r == 0) p = rnd(2000); else if (r == 1) p = ~(uint64_t)0 - rnd(3); }
            if (rnd(2)) b.n_pos = rnd(b.pos.size() + 1);
            if (rnd(2)) for (uint32_t i = 0; i < n; i++) b.count[i] += rnd(3); // counts that overstate what pos holds
        }
        // the selection
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
        BrxTakeArgs a;
        a.out = b.arena.data(); a.out_off = b.off.data(); a.len = b.len.data(); a.n = n; a.span = span;
        a.count = b.count.data(); a.pos_off = b.pos_off.data(); a.pos = b.pos.empty() ? nullptr : b.pos.data(); a.n_pos = b.n_pos;
        a.delim_len = b.D; a.flags = b.flags;
        a.sel_stream = pairs ? ss.data() : nullptr; a.sel_rec = pairs ? sr.data() : nullptr; a.m = m;
        A_LO = b.arena.data(); A_HI = A_LO + span;
        // serial: entry -> (i, k) -> (src, L)
        std::vector<uint64_t> esrc(m), eL(m);
        for (uint64_t j = 0; j < m; j++) {
            uint64_t i = n, k = 0;
            if (pairs) { i = ss[j]; k = sr[j]; }
            else for (uint32_t t = 0; t < n; t++) if (b.pos_off[t] + t <= j) { i = t; k = j - (b.pos_off[t] + t); }
            serial_record(b, i, k, esrc[j], eL[j]);
        }
        // size mode through the shared text
        EmuMem mem;
        for (uint64_t j = 0; j < m; j++)
            if (brx_take_entry_record(mem, a, j).len != eL[j]) { printf("FAIL: it %d entry %llu: size\n", it, (unsigned long long)j); return 1; }
        // rooms
        std::vector<uint64_t> dst_off(m);
        uint64_t total = 0;
        const uint64_t stride = strided ? 1 + rnd(40) : 0;
        for (uint64_t j = 0; j < m; j++) { dst_off[j] = strided ? j * stride : total; total += strided ? stride : eL[j]; }
        if (cut) total = rnd(total + 1);
        const uint32_t phase = (uint32_t)rnd(16);
        uint8_t *raw = (uint8_t *)aligned_alloc(64, (total + 256 + 63) & ~(uint64_t)63);
        uint8_t *dst = raw + 64 + phase;
        memset(raw, 0xEE, total + 256);
        Bytes want(total, 0xEE);
        for (uint64_t j = 0; j < m; j++) {
            const uint64_t e = j + 1 < m ? dst_off[j + 1] : total;
            for (uint64_t t = 0; t < eL[j] && dst_off[j] + t < e && dst_off[j] + t < total; t++) want[dst_off[j] + t] = b.arena[esrc[j] + t];
        }
        D_LO = dst; D_HI = dst + total;
        written.assign(total, 0);
        const uint64_t chunks = brx_take_chunks(total, dst);
        for (uint64_t c = chunks; c-- > 0;) emu_chunk(a, dst_off.data(), dst, total, c); // (any order: the chunks are independent)
        if (total && memcmp(dst, want.data(), total)) {
            uint64_t x = 0;
            while (dst[x] == want[x]) x++;
            printf("FAIL: it %d (D %u flags %u pairs %d strided %d cut %d stale %d): byte %llu of %llu is %02x, want %02x\n", it, b.D, b.flags,
                   pairs, strided, cut, stale, (unsigned long long)x, (unsigned long long)total, dst[x], want[x]);
            return 1;
        }
        for (uint64_t x = 0; x < 64 + phase; x++) if (raw[x] != 0xEE) die("a byte in front of dst changed");
        for (uint64_t x = 64 + phase + total; x < total + 256; x++) if (raw[x] != 0xEE) die("a byte at or behind total changed");
        free(raw);
        cases++; bytes += total;
    }
    printf("OK: %llu batches, %llu destination bytes; loads %llu wide + %llu byte, stores %llu wide + %llu byte, none outside\n",
           (unsigned long long)cases, (unsigned long long)bytes, (unsigned long long)n_wide_loads, (unsigned long long)n_byte_loads,
           (unsigned long long)n_wide_stores, (unsigned long long)n_byte_stores);
    return 0;
}
