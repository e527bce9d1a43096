// parse_emu.cpp -- brx_parse_batch on a CPU, lane by lane: the REAL text of csrc/brx_parse.h and csrc/brx_take.h (brx_take_entry_record,
// then brx_parse_lane, as brx_parse_kernel of csrc/brx_parse.hip calls them) held to a byte-serial restatement of THE PARSE of
// include/brx.h that shares nothing with either header: one byte at a time, the value in unsigned __int128 with a cap.
// EVERY record is parsed as every kind (DEC at scales 0, 1, 2, 9, 18) under all four combinations of BRX_PARSE_SPACES /
// BRX_PARSE_QUOTED, so each is checked on all lengths 0 .. 66 at all 16 source phases (the run fails if one combination was not met),
// on records that start on the arena's first byte and end on its last, on arenas of 1 .. 40 bytes, in both selection modes, under the
// three BRX_TAKE flag combinations, with delimiters of 1, 2 and 16 bytes and with stale positions.
// Every emulated arena load is recorded and the run fails if one lies outside [out, out + span), or if the parse of an entry of more
// than 64 bytes loads one of the record's bytes: these are the contract's "never loaded" clauses, which a GPU test cannot see.
// No GPU.  Build and run: g++ -O2 -std=c++17 -I brotli-rs_amd/csrc tools/parse_emu.cpp -o parse_emu && ./parse_emu
// (tests/test_parse_abi.py does).  It proves the header's logic, not the kernel's own code: that is tests/test_gpu_parse.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <random>
#include "brx_parse.h"
typedef unsigned __int128 u128;

static const uint8_t *A_LO, *A_HI;   // the arena
static const uint8_t *F_LO, *F_HI;   // bytes that must not be loaded now: the record of an entry above 64 bytes, while it is parsed
static uint64_t n_wide_loads, n_byte_loads;
static void die(const char *what) { printf("FAIL: %s\n", what); exit(1); }

struct EmuMem {
    uint8_t ld8(const uint8_t *p) {
        if (p < A_LO || p >= A_HI) die("byte load outside the arena");
        if (p >= F_LO && p < F_HI) die("byte load from a record above 64 bytes");
        n_byte_loads++;
        return *p;
    }
    BrxTake128 ld128(const uint8_t *p) {
        if (p < A_LO || p + 16 > A_HI) die("16-byte load outside the arena");
        if (p + 16 > F_LO && p < F_HI) die("16-byte load from a record above 64 bytes");
        n_wide_loads++;
        BrxTake128 v;
        memcpy(&v.lo, p, 8);
        memcpy(&v.hi, p + 8, 8);
        return v;
    }
};

// ---- THE PARSE, serially, with nothing shared with brx_parse.h or brx_take.h --------------------------------------------------------
enum { S_OK = 0, S_INEXACT = 1, S_EMPTY = 2, S_RANGE = 3, S_BAD = 4, S_LONG = 5 };
static const u128 CAP = (u128)1 << 100; // a value that reached it stays there: far above 2^64, far below 2^128 / 16
static int ref_parse(const uint8_t *r, uint64_t L, uint32_t kind, uint32_t scale, bool spaces, bool quoted, uint8_t quote, uint64_t &val) {
    val = 0;
    if (L > 64) return S_LONG;
    uint64_t a = 0, e = L;
    if (spaces) {
        while (a < e && (r[a] == ' ' || r[a] == '\t')) a++;
        while (e > a && (r[e - 1] == ' ' || r[e - 1] == '\t')) e--;
    }
    if (quoted && e - a >= 2 && r[a] == quote && r[e - 1] == quote) { a++; e--; }
    if (a == e) return S_EMPTY;
    u128 V = 0;
    if (kind == 2) {
        if (e - a >= 2 && r[a] == '0' && (r[a + 1] == 'x' || r[a + 1] == 'X')) a += 2;
        if (a == e) return S_BAD;
        for (; a < e; a++) {
            const uint8_t c = r[a];
            int d;
            if (c >= '0' && c <= '9') d = c - '0';
            else if (c >= 'a' && c <= 'f') d = c - 'a' + 10;
            else if (c >= 'A' && c <= 'F') d = c - 'A' + 10;
            else return S_BAD;
            V = V * 16 + (unsigned)d;
            if (V > CAP) V = CAP;
        }
        if (V >> 64) { val = ~(uint64_t)0; return S_RANGE; }
        val = (uint64_t)V;
        return S_OK;
    }
    bool neg = false;
    if (r[a] == '+' || r[a] == '-') { neg = r[a] == '-'; a++; }
    uint64_t ni = 0, nf = 0;
    bool point = false, lost = false;
    for (; a < e; a++) {
        const uint8_t c = r[a];
        if (c == '.' && kind == 1 && !point) { point = true; continue; }
        if (c < '0' || c > '9') return S_BAD;
        if (!point) ni++; else nf++;
        if (!point || nf <= scale) { V = V * 10 + (unsigned)(c - '0'); if (V > CAP) V = CAP; }
        else if (c != '0') lost = true;
    }
    if (ni + nf == 0) return S_BAD;
    for (uint64_t t = nf; t < scale; t++) { V *= 10; if (V > CAP) V = CAP; }
    const u128 lim = neg ? (u128)1 << 63 : ((u128)1 << 63) - 1;
    if (V > lim) { val = neg ? (uint64_t)1 << 63 : ~((uint64_t)1 << 63); return S_RANGE; }
    val = neg ? (uint64_t)0 - (uint64_t)V : (uint64_t)V;
    return lost ? S_INEXACT : S_OK;
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

#define MAXLEN 66u
static uint8_t covered[MAXLEN + 1][16]; // [L][phase of the first byte]
static uint64_t n_records, n_parses, n_status[6];
static const uint32_t KINDS[7][2] = {{0, 0}, {1, 0}, {1, 1}, {1, 2}, {1, 9}, {1, 18}, {2, 0}};

// one call: every entry, as every kind under every combination of the parse flags, through the header and the serial walk
static void run(const Batch &b, bool pairs, const std::vector<uint32_t> &ss, const std::vector<uint64_t> &sr, uint64_t m, uint8_t quote, int it) {
    const uint32_t n = (uint32_t)b.off.size();
    BrxTakeArgs a;
    a.out = b.arena; a.out_off = b.off.data(); a.len = b.len.data(); a.n = n; a.span = b.span;
    a.count = b.count.data(); a.pos_off = b.pos_off.data(); a.pos = b.pos.empty() ? nullptr : b.pos.data(); a.n_pos = b.n_pos;
    a.delim_len = b.D;
    a.sel_stream = pairs ? ss.data() : nullptr; a.sel_rec = pairs ? sr.data() : nullptr; a.m = m;
    A_LO = b.arena; A_HI = A_LO + b.span;
    F_LO = F_HI = nullptr;
    EmuMem mem;
    for (uint64_t j = 0; j < m; j++) {
        uint64_t i = n, kk = 0, src, L;
        if (pairs) { i = ss[j]; kk = sr[j]; }
        else for (uint32_t t = 0; t < n; t++) if (b.pos_off[t] + t <= j) { i = t; kk = j - (b.pos_off[t] + t); }
        serial_record(b, i, kk, src, L);
        for (uint32_t pf = 0; pf < 4u; pf++) {
            a.flags = b.flags | (pf << 4); // the flags word as the kernel gets it: the rule reads its own two bits only
            const BrxTakeRec r = brx_take_entry_record(mem, a, j);
            if (r.len != L || (L && r.src != src)) { printf("FAIL: it %d entry %llu: the record\n", it, (unsigned long long)j); exit(1); }
            if (L > 64) { F_LO = b.arena + src; F_HI = F_LO + L; }
            for (uint32_t q = 0; q < 7u; q++) {
                uint64_t want;
                const int ws = ref_parse(b.arena + src, L, KINDS[q][0], KINDS[q][1], pf & 1u, (pf & 2u) != 0, quote, want);
                const BrxParseOut o = brx_parse_lane(mem, a.out, a.span, r, KINDS[q][0], KINDS[q][1], a.flags, quote);
                if (o.status != (uint32_t)ws || (uint64_t)o.val != want) {
                    printf("FAIL: it %d entry %llu (L %llu, phase %u, flags %u, pairs %d, kind %u, scale %u) \"%.*s\": got %lld / %u, want %lld / %d\n",
                           it, (unsigned long long)j, (unsigned long long)L, (unsigned)((uintptr_t)(b.arena + src) & 15u), a.flags, (int)pairs,
                           KINDS[q][0], KINDS[q][1], (int)(L < 70 ? L : 70), (const char *)b.arena + src, (long long)o.val, o.status,
                           (long long)want, ws);
                    exit(1);
                }
                n_parses++; n_status[ws]++;
            }
            F_LO = F_HI = nullptr;
        }
        if (L <= MAXLEN) covered[L][(uintptr_t)(b.arena + src) & 15u] = 1;
        n_records++;
    }
}

// ---- text biased to the grammar's edges ---------------------------------------------------------------------------------------------
static std::mt19937_64 rng(20260118);
static uint64_t rnd(uint64_t m) { return (uint64_t)(rng() % m); }
static std::string digits(uint32_t c, const char *alphabet, uint32_t na) {
    std::string s;
    for (uint32_t t = 0; t < c; t++) s += alphabet[rnd(na)];
    return s;
}
static const char *EDGES[] = {"9223372036854775807", "9223372036854775808", "9223372036854775809", "9223372036854775806", "18446744073709551615",
                              "18446744073709551616", "9999999999999999999", "10000000000000000000", "1000000000000000000", "99999999", "100000000",
                              "9999999999999999", "10000000000000000", "0", "00", "1"};
static const char JUNK[] = "0123456789+-. \t\"'xXabfABFgG,eE\r_\x80\xB0\xFF\x00";
// a field of about `want` bytes (exactly `want` for the plain forms); never holds 0x0A
static std::string field(uint32_t want) {
    std::string s;
    const uint32_t form = (uint32_t)rnd(10);
    if (form == 0) { // junk
        for (uint32_t t = 0; t < want; t++) s += JUNK[rnd(sizeof(JUNK) - 1)];
        return s;
    }
    if (form <= 3) { // decimal digits: leading zeros, then digits or an edge value, a sign and a point somewhere
        std::string d = rnd(3) ? digits(1 + (uint32_t)rnd(21), "0123456789", 10) : std::string(EDGES[rnd(16)]);
        if (rnd(2) && d.size() < want) d = std::string(want - d.size(), '0') + d;
        if (rnd(3) == 0) d += digits((uint32_t)rnd(4), "0000000001", 10);
        if (form >= 2) d.insert(rnd(d.size() + 1), ".");
        if (rnd(3) == 0) d.insert(0, rnd(2) ? "-" : "+");
        s = d;
    } else if (form <= 5) { // hex
        s = digits(1 + (uint32_t)rnd(19), "0123456789abcdefABCDEF", 22);
        if (rnd(3) == 0) s = std::string(rnd(3) ? 16 : 17, "fF"[rnd(2)]);
        if (rnd(2) && s.size() + 2 < want) s = std::string(want - 2 - s.size(), '0') + s;
        if (rnd(2)) s.insert(0, rnd(2) ? "0x" : "0X");
    } else if (form == 6) { // short things around the grammar's corners
        static const char *C[] = {"", "-", "+", ".", "-.", "0x", "0X", "x1", "\"", "\"\"", "\"\"\"", " ", "  ", "\t", "1 ", " 1", "1e3", "+-1", "--1", "1.2.3", "5.",
                                  ".5", "-0", "+0", "-0.009", "0x0", "00x1", "0xg", "\" 42\"", "\"42", "42\"", ".0", "0.", "-.0"};
        s = C[rnd(sizeof(C) / sizeof(C[0]))];
    } else { // exactly `want` bytes of digits with leading zeros
        s = std::string(rnd(want + 1), '0');
        if (s.size() < want) s += digits(want - (uint32_t)s.size(), "0123456789", 10);
        if (form == 8 && want >= 2) s[rnd(want)] = '.';
        if (form == 9 && want >= 1) s[0] = "+-"[rnd(2)];
        return s;
    }
    // spaces and quotes around it
    if (rnd(3) == 0) s = "\"" + s + "\"";
    if (rnd(3) == 0) s = std::string(rnd(20), rnd(2) ? ' ' : '\t') + s + std::string(rnd(20), rnd(2) ? ' ' : '\t');
    if (rnd(8) == 0) s = "\"" + s + "\"";
    return s;
}
// exactly L bytes
static std::string field_of(uint32_t L) {
    std::string s = field(L);
    if (s.size() > L) s.resize(L);
    if (s.size() < L) s = (rnd(2) ? std::string(L - s.size(), rnd(2) ? ' ' : '0') + s : s + std::string(L - s.size(), rnd(2) ? ' ' : '0'));
    return s;
}

int main() {
    const uint32_t Ds[3] = {1, 2, 16}, FL[3] = {0, 1, 3};
    uint64_t batches = 0;
    uint8_t *raw = (uint8_t *)aligned_alloc(64, (size_t)1 << 22);
    // PART 0: the check values of the contract, as whole streams (count = 0), so that the serial walk itself is held to the table
    {
        const int64_t MAX = INT64_MAX, MIN = INT64_MIN;
        const std::string z45(45, '0');
        struct CV { std::string r; uint32_t kind, scale, pf; int64_t val; int st; } cv[] = {
            {"0", 0, 0, 0, 0, S_OK}, {"-0", 0, 0, 0, 0, S_OK}, {"+17", 0, 0, 0, 17, S_OK}, {"9223372036854775807", 0, 0, 0, MAX, S_OK},
            {"9223372036854775808", 0, 0, 0, MAX, S_RANGE}, {"-9223372036854775808", 0, 0, 0, MIN, S_OK},
            {"-9223372036854775809", 0, 0, 0, MIN, S_RANGE}, {z45 + "9223372036854775807", 0, 0, 0, MAX, S_OK},
            {z45 + "09223372036854775807", 0, 0, 0, 0, S_LONG}, {"12.5", 0, 0, 0, 0, S_BAD}, {"", 0, 0, 0, 0, S_EMPTY}, {"-", 0, 0, 0, 0, S_BAD},
            {"1 ", 0, 0, 0, 0, S_BAD},
            {"12.34", 1, 2, 0, 1234, S_OK}, {"12.345", 1, 2, 0, 1234, S_INEXACT}, {"12.340", 1, 2, 0, 1234, S_OK}, {"-.5", 1, 2, 0, -50, S_OK},
            {"5.", 1, 2, 0, 500, S_OK}, {".", 1, 2, 0, 0, S_BAD}, {"-0.009", 1, 2, 0, 0, S_INEXACT}, {"1e3", 1, 2, 0, 0, S_BAD},
            {"92233720368547758.07", 1, 2, 0, MAX, S_OK}, {"92233720368547758.08", 1, 2, 0, MAX, S_RANGE},
            {"-92233720368547758.089", 1, 2, 0, MIN, S_INEXACT},
            {"12.5", 1, 0, 0, 12, S_INEXACT}, {"9.223372036854775807", 1, 18, 0, MAX, S_OK}, {"9.3", 1, 18, 0, MAX, S_RANGE},
            {"ff", 2, 0, 0, 255, S_OK}, {"0xFFFFFFFFFFFFFFFF", 2, 0, 0, -1, S_OK}, {"0x10000000000000000", 2, 0, 0, -1, S_RANGE},
            {"0x", 2, 0, 0, 0, S_BAD}, {"x1", 2, 0, 0, 0, S_BAD}, {"0X0000000000000000000000001f", 2, 0, 0, 31, S_OK},
            {" \"42\"\t", 0, 0, 3, 42, S_OK}, {"\" 42\"", 0, 0, 3, 0, S_BAD}, {"\"42", 0, 0, 3, 0, S_BAD}, {"\"", 0, 0, 3, 0, S_BAD},
            {"\"\"", 0, 0, 3, 0, S_EMPTY}, {"  ", 0, 0, 3, 0, S_EMPTY}};
        for (auto &c : cv) {
            Batch b;
            b.arena = raw + 64 + rnd(16);
            memcpy(b.arena, c.r.data(), c.r.size());
            b.span = c.r.size() ? c.r.size() : 1; b.D = 1; b.flags = 0; b.n_pos = 0;
            b.off.push_back(0); b.len.push_back(c.r.size()); b.count.push_back(0); b.pos_off.push_back(0);
            uint64_t v;
            if (ref_parse(b.arena, c.r.size(), c.kind, c.scale, c.pf & 1u, (c.pf & 2u) != 0, '"', v) != c.st || (int64_t)v != c.val)
                die("a check value of the contract");
            run(b, false, {}, {}, 1, '"', -1);
            batches++;
        }
    }
    // PART 1: one stream that is the whole arena, records of every length 0 .. MAXLEN + 1 in order, at each phase of the arena: the
    // first record starts on the arena's first byte, the last one ends on its last
    for (int it = 0; it < 96; it++) {
        Batch b;
        const uint32_t phase = it % 16;
        b.D = 1; b.flags = FL[(it / 16) % 3];
        const bool pairs = it % 2;
        b.arena = raw + 64 + phase;
        uint64_t at = 0;
        b.pos_off.push_back(0);
        for (uint32_t L = 0; L <= MAXLEN + 1u; L++) {
            const std::string s = field_of(L);
            memcpy(b.arena + at, s.data(), L);
            at += L;
            if (L && rnd(4) == 0) b.arena[at - 1] = 13;
            if (L <= MAXLEN) { b.pos.push_back(at); b.arena[at++] = 10; }
        }
        b.span = at;
        b.off.push_back(0); b.len.push_back(at); b.count.push_back(b.pos.size());
        b.n_pos = b.pos.size();
        std::vector<uint32_t> ss; std::vector<uint64_t> sr;
        uint64_t m = b.pos.size() + 1;
        if (pairs) for (uint64_t j = 0; j < m; j++) { ss.push_back(0); sr.push_back(m - 1 - j); }
        run(b, pairs, ss, sr, m, "\"'"[rnd(2)], it);
        batches++;
    }
    // PART 2: random batches of several streams in slots with slack (the first stream on the arena's first byte, the last one up to
    // its last): CSV-like text, D in {1, 2, 16}, stale positions; every fourth batch in an arena of 1 .. 40 bytes
    for (int it = 0; it < 600; it++) {
        Batch b;
        b.D = Ds[it % 3];
        b.flags = FL[(it / 3) % 3];
        const bool pairs = (it / 9) % 2;
        const int stale = (it / 18) % 5 == 4;
        const bool tiny = it % 4 == 3;
        const uint32_t n = tiny ? 1 + (uint32_t)rnd(2) : 1 + (uint32_t)rnd(6);
        b.arena = raw + 64 + rnd(16);
        uint64_t at = 0;
        b.off.resize(n); b.len.resize(n); b.count.resize(n); b.pos_off.resize(n);
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t l = rnd(8) == 0 ? 0 : (tiny ? 1 + rnd(20) : rnd(900));
            b.off[i] = at; b.len[i] = l;
            std::string s;
            while (s.size() < l) {
                s += field(rnd(6) == 0 ? (uint32_t)rnd(70) : (uint32_t)rnd(22));
                if (rnd(5) == 0) s += '\r';
                for (uint32_t t = 0; t < b.D; t++) s += '\n';
            }
            if (rnd(2)) s = s.substr(s.size() - l); // a stream may start inside a field, or end inside one
            memcpy(b.arena + at, s.data(), l);
            at += l;
            if (i + 1 < n) for (uint64_t t = rnd(tiny ? 4 : 20); t > 0; t--) b.arena[at++] = rnd(2) ? 13 : '7'; // slack: what a stray load would take up
        }
        if (at == 0) b.arena[at++] = '7';
        b.span = at;
        for (uint32_t i = 0; i < n; i++) {
            b.pos_off[i] = b.pos.size();
            for (uint64_t j = 0; j + b.D <= b.len[i]; j++) {
                bool hit = true;
                for (uint32_t t = 0; t < b.D && hit; t++) hit = b.arena[b.off[i] + j + t] == 10;
                if (hit) b.pos.push_back(j);
            }
            b.count[i] = b.pos.size() - b.pos_off[i];
        }
        b.n_pos = b.pos.size();
        if (stale) {
            for (auto &p : b.pos) { uint64_t r = rnd(4); if (r == 0) p = rnd(1000); else if (r == 1) p = ~(uint64_t)0 - rnd(3); }
            if (rnd(2)) b.n_pos = rnd(b.pos.size() + 1);
            if (rnd(2)) for (uint32_t i = 0; i < n; i++) b.count[i] += rnd(3);
        }
        std::vector<uint32_t> ss; std::vector<uint64_t> sr;
        uint64_t m;
        if (pairs) {
            m = 1 + rnd(200);
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
        run(b, pairs, ss, sr, m, "\"'"[rnd(2)], 1000 + it);
        batches++;
    }
    for (uint32_t L = 0; L <= MAXLEN; L++)
        for (uint32_t ph = 0; ph < 16u; ph++)
            if (!covered[L][ph]) { printf("FAIL: length %u at phase %u was not met\n", L, ph); return 1; }
    free(raw);
    printf("OK: %llu batches, %llu records, %llu parses (OK %llu, INEXACT %llu, EMPTY %llu, RANGE %llu, BAD %llu, LONG %llu); every length 0 .. %u at "
           "all 16 phases; loads %llu wide + %llu byte, none outside the arena, none from a record above 64 bytes\n",
           (unsigned long long)batches, (unsigned long long)n_records, (unsigned long long)n_parses, (unsigned long long)n_status[0],
           (unsigned long long)n_status[1], (unsigned long long)n_status[2], (unsigned long long)n_status[3], (unsigned long long)n_status[4],
           (unsigned long long)n_status[5], MAXLEN, (unsigned long long)n_wide_loads, (unsigned long long)n_byte_loads);
    return 0;
}
