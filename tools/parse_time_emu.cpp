// parse_time_emu.cpp -- brx_parse_time_batch on a CPU, lane by lane: the REAL text of csrc/brx_parse_time.h, csrc/brx_parse.h and
// csrc/brx_take.h (brx_take_entry_record, then brx_parse_time_lane, as brx_parse_time_kernel of csrc/brx_parse_time.hip calls them).
// What is expected comes from outside: a file of whole calls -- arena, tables, selection, flags, kind, scale -- with the record (source
// offset, length), val, the status and the zone of every entry, as tests/parse_time_oracle.py states them
// (tests/test_parse_time_abi.py writes the file).  The first difference ends the run, exit code 1.
// Every emulated arena load is checked: the run fails if one lies outside [out, out + span), or if the parse of an entry of more than
// 64 bytes loads one of the record's bytes -- the contract's "never loaded" clauses, which a GPU test cannot see.  The arena of each
// call is placed at the 16-byte phase that the file asks for, so that "every length at every phase" is the file's to arrange; the
// run reports which (length, phase) pairs it met and fails if `--full` is given and one of 0 .. 66 x 0 .. 15 is missing.
// No GPU.  Build and run: g++ -O2 -std=c++17 -I brotli-rs_amd/csrc tools/parse_time_emu.cpp -o parse_time_emu && ./parse_time_emu FILE
// Built with -fsanitize=address,undefined as this stand-alone program it must run clean too.
// It proves the header's logic, not the kernel's own code: that is tests/test_gpu_parse_time.py.
//
// The file: little-endian 64-bit words.  Per call: MAGIC, phase, span, n, pos_len, n_pos, delim_len, flags, quote, pairs, m, kind, scale;
// the arena (span bytes, padded with zeros to a multiple of 8); out_off[n], len[n], count[n], pos_off[n]; pos[pos_len]; if pairs
// sel_stream[m] (one word each) and sel_rec[m]; then m times (src, L, val, status, zone), the signed ones as two's complement.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "brx_parse_time.h"

static const uint64_t MAGIC = 0x454D49545F585242ull; // "BRX_TIME"
static const uint8_t *A_LO, *A_HI; // the arena
static const uint8_t *F_LO, *F_HI; // bytes that must not be loaded now: the record of an entry above 64 bytes, while it is parsed
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

static FILE *in;
static bool word(uint64_t &v) { return fread(&v, 8, 1, in) == 1; }
static uint64_t need() {
    uint64_t v;
    if (!word(v)) die("the file ends inside a call");
    return v;
}
static void words(std::vector<uint64_t> &v, uint64_t c) {
    v.resize(c);
    if (c && fread(v.data(), 8, c, in) != c) die("the file ends inside a call");
}

#define MAXLEN 66u
static uint8_t covered[MAXLEN + 1][16]; // [L][phase of the first byte]

int main(int argc, char **argv) {
    const char *path = nullptr;
    bool full = false;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--full")) full = true; else path = argv[i];
    }
    if (!path || !(in = fopen(path, "rb"))) die("usage: parse_time_emu [--full] FILE");
    uint64_t calls = 0, entries = 0, n_status[6] = {0, 0, 0, 0, 0, 0}, tiny = 0, zoned = 0;
    uint64_t magic;
    while (word(magic)) {
        if (magic != MAGIC) die("not a call");
        const uint64_t phase = need(), span = need(), n = need(), pos_len = need(), n_pos = need(), D = need(), flags = need(), quote = need(),
                       pairs = need(), m = need(), kind = need(), scale = need();
        if (phase > 15 || span == 0 || span > ((uint64_t)1 << 24) || n > ((uint64_t)1 << 20) || pos_len > ((uint64_t)1 << 24) ||
            m > ((uint64_t)1 << 24) || kind > 2 || scale > 9)
            die("a call's header");
        // the arena alone in an allocation of its own: with the address sanitizer a load outside it is caught a second time
        std::vector<uint64_t> padded;
        words(padded, (span + 7) / 8);
        uint8_t *raw = (uint8_t *)aligned_alloc(16, (size_t)((span + 15 + 15) / 16 * 16));
        uint8_t *arena = raw + phase;
        memcpy(arena, padded.data(), (size_t)span);
        std::vector<uint64_t> off, len, count, pos_off, pos, ss64, sr, want;
        words(off, n); words(len, n); words(count, n); words(pos_off, n); words(pos, pos_len);
        if (pairs) { words(ss64, m); words(sr, m); }
        words(want, 5 * m);
        std::vector<uint32_t> ss(ss64.begin(), ss64.end());
        BrxTakeArgs a;
        a.out = arena; a.out_off = off.data(); a.len = len.data(); a.n = (uint32_t)n; a.span = span;
        a.count = count.data(); a.pos_off = pos_off.data(); a.pos = pos_len ? pos.data() : nullptr; a.n_pos = n_pos;
        a.delim_len = (uint32_t)D; a.flags = (uint32_t)flags;
        a.sel_stream = pairs ? ss.data() : nullptr; a.sel_rec = pairs ? sr.data() : nullptr; a.m = m;
        A_LO = arena; A_HI = arena + span;
        EmuMem mem;
        for (uint64_t j = 0; j < m; j++) {
            const uint64_t src = want[5 * j], L = want[5 * j + 1], st = want[5 * j + 3];
            const int64_t val = (int64_t)want[5 * j + 2], zone = (int64_t)want[5 * j + 4];
            F_LO = F_HI = nullptr;
            const BrxTakeRec r = brx_take_entry_record(mem, a, j);
            if (r.len != L || (L && r.src != src)) {
                printf("FAIL: call %llu entry %llu: the record is (%llu, %llu), want (%llu, %llu)\n", (unsigned long long)calls, (unsigned long long)j,
                       (unsigned long long)r.src, (unsigned long long)r.len, (unsigned long long)src, (unsigned long long)L);
                return 1;
            }
            if (L > 64) { F_LO = arena + src; F_HI = F_LO + L; }
            const BrxParseTimeOut o = brx_parse_time_lane(mem, a.out, a.span, r, (uint32_t)kind, (uint32_t)scale, a.flags, (uint32_t)quote);
            F_LO = F_HI = nullptr;
            if (o.val != val || o.status != st || o.zone != zone) {
                printf("FAIL: call %llu entry %llu (L %llu, phase %u, flags %llu, kind %llu, scale %llu, pairs %d) \"%.*s\": got %lld / %u / %d, "
                       "want %lld / %llu / %lld\n",
                       (unsigned long long)calls, (unsigned long long)j, (unsigned long long)L, (unsigned)((uintptr_t)(arena + src) & 15u),
                       (unsigned long long)flags, (unsigned long long)kind, (unsigned long long)scale, (int)pairs, (int)(L < 70 ? L : 70),
                       (const char *)arena + src, (long long)o.val, o.status, o.zone, (long long)val, (unsigned long long)st, (long long)zone);
                return 1;
            }
            if (st > 5) die("a status of the file");
            n_status[st]++;
            zoned += zone != BRX_TIME_Z_NONE;
            if (L <= MAXLEN) covered[L][(uintptr_t)(arena + src) & 15u] = 1;
            entries++;
        }
        if (span <= 40) tiny++;
        free(raw);
        calls++;
    }
    fclose(in);
    uint32_t missing = 0;
    for (uint32_t L = 0; L <= MAXLEN; L++)
        for (uint32_t ph = 0; ph < 16u; ph++) missing += !covered[L][ph];
    if (full && missing) { printf("FAIL: %u (length, phase) pairs of 0 .. %u x 0 .. 15 were not met\n", missing, MAXLEN); return 1; }
    printf("OK: %llu calls (%llu in arenas of at most 40 bytes), %llu entries (OK %llu, INEXACT %llu, EMPTY %llu, RANGE %llu, BAD %llu, LONG %llu; "
           "%llu with a zone); %u (length, phase) pairs not met; loads %llu wide + %llu byte, none outside the arena, none from a record above "
           "64 bytes\n",
           (unsigned long long)calls, (unsigned long long)tiny, (unsigned long long)entries, (unsigned long long)n_status[0],
           (unsigned long long)n_status[1], (unsigned long long)n_status[2], (unsigned long long)n_status[3], (unsigned long long)n_status[4],
           (unsigned long long)n_status[5], (unsigned long long)zoned, missing, (unsigned long long)n_wide_loads, (unsigned long long)n_byte_loads);
    return 0;
}
