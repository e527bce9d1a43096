// unescape_emu.cpp -- brx_unescape_batch on a CPU, lane by lane: the lane path (brx_text_lane), the wave path (the loop of
// brx_unescape_kernel, csrc/brx_unescape.hip, with its 64 lanes in turn and its ballots and shuffles as array reads) and the serial
// path (brx_text_serial) around the REAL text of csrc/brx_unescape.h, held to a byte-serial restatement of THE TEXT of include/brx.h
// that shares nothing with the header.  The lane path and the wave path are BOTH run on EVERY record, whatever its length, so each is
// checked on all lengths 0 .. BRX_TEXT_LONG + 2 rows at all 16 source phases and all 16 destination phases (the run fails if one
// combination was not met), then on random records with blanks, cut rooms and odd quote / escape bytes.
// The run fails on: a load outside the arena or outside the record; a store outside the entry's room or at or behind `total`; a
// destination byte written twice; a text, a length or a status that differs.
// No GPU.  Build and run: g++ -O2 -std=c++17 -I brotli-rs_amd/csrc tools/unescape_emu.cpp -o unescape_emu && ./unescape_emu
// (tests/test_unescape_abi.py does).  It proves the arithmetic, not the kernel's own text: that is tests/test_gpu_unescape.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <random>
#include "brx_unescape.h"
typedef std::vector<uint8_t> Bytes;

static const uint8_t *A_LO, *A_HI, *R_LO, *R_HI; // the arena and the record
static uint8_t *D_LO, *D_HI;                     // the entry's room, already cut at total
static std::vector<uint8_t> written;
static uint64_t n_wide_loads, n_byte_loads, n_wide_stores, n_byte_stores;
static void die(const char *what) { printf("FAIL: %s\n", what); exit(1); }

struct EmuMem {
    uint8_t ld8(const uint8_t *p) {
        if (p < A_LO || p >= A_HI) die("byte load outside the arena");
        if (p < R_LO || p >= R_HI) die("byte load outside the record");
        n_byte_loads++;
        return *p;
    }
    BrxTake128 ld128(const uint8_t *p) {
        if (p < A_LO || p + 16 > A_HI) die("16-byte load outside the arena");
        if (p < R_LO || p + 16 > R_HI) die("16-byte load outside the record");
        n_wide_loads++;
        BrxTake128 v;
        memcpy(&v.lo, p, 8);
        memcpy(&v.hi, p + 8, 8);
        return v;
    }
    void mark(uint8_t *p, uint32_t n) {
        if (p < D_LO || p + n > D_HI) die("store outside the room or at or behind total");
        for (uint32_t t = 0; t < n; t++) {
            if (written[(size_t)(p + t - D_LO)]) die("destination byte written twice");
            written[(size_t)(p + t - D_LO)] = 1;
        }
    }
    void st8(uint8_t *p, uint8_t v) { mark(p, 1); n_byte_stores++; *p = v; }
    void st128(uint8_t *p, BrxTake128 v) { mark(p, 16); n_wide_stores++; memcpy(p, &v.lo, 8); memcpy(p + 8, &v.hi, 8); }
};

// the body of the loop over the long records in brx_unescape_kernel, for one record: the three steps of a row as brx_unescape.h
// words them, what the lanes exchange between the steps as array reads
template <uint32_t MODE>
static BrxTextRes emu_wave_as(const uint8_t *rec, int64_t L, const BrxTextPlan &p, uint32_t q, uint32_t e, BrxTextRoom d) {
    EmuMem mem;
    BrxTextRes r = {0, 0, 0};
    BrxTextCarry carry = {0, 0};
    for (int64_t row = brx_text_row0(p.ws); row < p.we; row += BRX_TEXT_ROW) {
        BrxTextPre u[64];
        uint32_t e0[64], E[64], sum[64];
        BrxTextOut o[64];
        uint64_t nonall = 0; // the ballot
        for (uint32_t l = 0; l < 64u; l++) {
            u[l] = brx_text_pre<MODE>(mem, rec, L, p, q, e, row + (int64_t)l * BRX_TEXT_UNIT);
            e0[l] = brx_text_ebits(u[l].em, 0u);
            if (u[l].em != 0xFFFFu) nonall |= (uint64_t)1 << l;
        }
        for (uint32_t l = 0; l < 64u; l++) {
            const int32_t src = brx_text_pin_lane(nonall, l);
            E[l] = brx_text_row_e(u[l].em, e0[l], src, e0[src < 0 ? 0 : src], carry); // (the shuffle)
        }
        for (uint32_t l = 0; l < 64u; l++) {
            const uint32_t Eprev = brx_text_row_prev(l, E[l ? l - 1u : 0u], carry); // (shuffle up by one: lane 0 gets its own)
            o[l] = brx_text_unit<MODE>(mem, rec, L, p, q, e, row + (int64_t)l * BRX_TEXT_UNIT, u[l], Eprev | (E[l] << 16));
            sum[l] = o[l].cnt + (l ? sum[l - 1u] : 0u); // (the prefix sum)
        }
        for (uint32_t l = 0; l < 64u; l++) {
            brx_text_store(mem, d.dstp, brx_text_row_at(r.len, sum[l], o[l].cnt), d.room, o[l]);
            r.bad |= o[l].bad;
            r.closed |= o[l].closed;
        }
        r.len += sum[63];
        carry = brx_text_row_carry(E[63]);
    }
    return r;
}
// the kernel is compiled once per dialect: MODE is the dialect's, also where the record's own mode is "copy"
static BrxTextRes emu_wave(uint32_t dialect, const uint8_t *rec, int64_t L, const BrxTextPlan &p, uint32_t q, uint32_t e, BrxTextRoom d) {
    if (dialect == BRX_TEXT_D_CSV) return emu_wave_as<BRX_TEXT_M_CSV>(rec, L, p, q, e, d);
    if (dialect == BRX_TEXT_D_JSON) return emu_wave_as<BRX_TEXT_M_JSON>(rec, L, p, q, e, d);
    return emu_wave_as<BRX_TEXT_M_BACKSLASH>(rec, L, p, q, e, d);
}
static BrxTextRes emu_lane(uint32_t dialect, EmuMem &mem, const uint8_t *rec, int64_t L, const BrxTextPlan &p, uint32_t q, uint32_t e, BrxTextRoom d) {
    if (dialect == BRX_TEXT_D_CSV) return brx_text_lane<BRX_TEXT_M_CSV>(mem, rec, L, p, q, e, d);
    if (dialect == BRX_TEXT_D_JSON) return brx_text_lane<BRX_TEXT_M_JSON>(mem, rec, L, p, q, e, d);
    return brx_text_lane<BRX_TEXT_M_BACKSLASH>(mem, rec, L, p, q, e, d);
}

// ---- the definition, serially, with nothing shared with brx_unescape.h ----------------------------------------------------------
static int ref_hex(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}
static long ref_unit(const Bytes &t, size_t i) { // the code unit of t[i .. i + 4), or -1
    if (i + 4 > t.size()) return -1;
    long v = 0;
    for (size_t k = 0; k < 4; k++) {
        const int h = ref_hex(t[i + k]);
        if (h < 0) return -1;
        v = v * 16 + h;
    }
    return v;
}
static void ref_utf8(Bytes &u, long cp) {
    if (cp < 0x80) u.push_back((uint8_t)cp);
    else if (cp < 0x800) { u.push_back((uint8_t)(0xC0 | (cp >> 6))); u.push_back((uint8_t)(0x80 | (cp & 63))); }
    else if (cp < 0x10000) { u.push_back((uint8_t)(0xE0 | (cp >> 12))); u.push_back((uint8_t)(0x80 | ((cp >> 6) & 63))); u.push_back((uint8_t)(0x80 | (cp & 63))); }
    else { u.push_back((uint8_t)(0xF0 | (cp >> 18))); u.push_back((uint8_t)(0x80 | ((cp >> 12) & 63))); u.push_back((uint8_t)(0x80 | ((cp >> 6) & 63))); u.push_back((uint8_t)(0x80 | (cp & 63))); }
}
static int ref_text(const Bytes &r, int dialect, int q, int e, bool spaces, Bytes &u) {
    size_t lo = 0, hi = r.size();
    if (spaces) {
        while (lo < hi && (r[lo] == 0x20 || r[lo] == 0x09)) lo++;
        while (hi > lo && (r[hi - 1] == 0x20 || r[hi - 1] == 0x09)) hi--;
    }
    const Bytes t(r.begin() + (long)lo, r.begin() + (long)hi);
    const size_t T = t.size();
    u.clear();
    bool bad = false;
    if (dialect == 0) {
        if (T == 0 || t[0] != q) { u = t; return 1; }
        if (T < 2 || t[T - 1] != q) { u = t; return 3; }
        for (size_t i = 1; i < T - 1;) {
            if (t[i] == q) {
                if (i + 1 < T - 1 && t[i + 1] == q) { u.push_back((uint8_t)q); i += 2; continue; }
                bad = true;
            }
            u.push_back(t[i]);
            i++;
        }
        return bad ? 3 : 0;
    }
    if (dialect == 1) {
        if (T == 0 || t[0] != q) { u = t; return 1; }
        size_t i = 1;
        bool closed = false;
        while (i < T) {
            const int b = t[i];
            if (b == e) {
                if (i + 1 >= T) { u.push_back((uint8_t)e); bad = true; i++; continue; }
                const int c = t[i + 1];
                if (c == q || c == e || c == '/') { u.push_back((uint8_t)c); i += 2; continue; }
                const char *names = "bfnrt", *vals = "\x08\x0C\x0A\x0D\x09";
                const char *at = c ? strchr(names, c) : NULL;
                if (at) { u.push_back((uint8_t)vals[at - names]); i += 2; continue; }
                const long cu = c == 'u' ? ref_unit(t, i + 2) : -1;
                if (cu < 0) { u.push_back((uint8_t)e); bad = true; i++; continue; }
                if (cu < 0xD800 || cu > 0xDFFF) { ref_utf8(u, cu); i += 6; continue; }
                if (cu <= 0xDBFF && i + 12 <= T && t[i + 6] == e && t[i + 7] == 'u') {
                    const long lw = ref_unit(t, i + 8);
                    if (lw >= 0xDC00 && lw <= 0xDFFF) { ref_utf8(u, 0x10000 + ((cu - 0xD800) << 10) + (lw - 0xDC00)); i += 12; continue; }
                }
                u.push_back(0xEF); u.push_back(0xBF); u.push_back(0xBD);
                bad = true;
                i += 6;
                continue;
            }
            if (b == q) {
                if (i == T - 1) { closed = true; break; }
                bad = true;
            }
            u.push_back((uint8_t)b);
            i++;
        }
        return (bad || !closed) ? 3 : 0;
    }
    if (T == 2 && t[0] == e && t[1] == 'N') return 2;
    for (size_t i = 0; i < T;) {
        if (t[i] == e) {
            if (i + 1 >= T) { u.push_back((uint8_t)e); bad = true; i++; continue; }
            const int c = t[i + 1];
            const char *names = "bfnrtv0", *vals = "\x08\x0C\x0A\x0D\x09\x0B";
            const char *at = c ? strchr(names, c) : NULL;
            u.push_back(at ? (uint8_t)vals[at - names] : (uint8_t)c); // (vals[6] is the string's own 0)
            i += 2;
            continue;
        }
        u.push_back(t[i]);
        i++;
    }
    return bad ? 3 : 0;
}

// ---- one record through every path ----------------------------------------------------------------------------------------------
static uint64_t n_records, n_lane_long, n_wave_short, n_serial;
static std::vector<uint8_t> met; // (length, source phase, destination phase) combinations of the sweep

// path 0 lane, 1 wave, 2 serial.  `room` is the entry's room and `cut` what total leaves of it.
static void run_path(int path, const Bytes &rec, uint32_t sp, uint32_t dp, int dialect, uint32_t q, uint32_t e, bool spaces, uint64_t room,
                     uint64_t cut, const Bytes &want, int want_status) {
    const size_t L = rec.size();
    // the arena: the record at source phase sp, with bytes around it that must not be loaded
    std::vector<uint8_t> store(L + 96, 0x5C);
    size_t off = 32;
    while (((uintptr_t)(store.data() + off) & 15u) != sp) off++;
    if (L) memcpy(store.data() + off, rec.data(), L);
    A_LO = store.data(); A_HI = store.data() + store.size();
    R_LO = store.data() + off; R_HI = R_LO + L;
    std::vector<uint8_t> dstbuf(room + 96, 0xA5);
    size_t doff = 32;
    while (((uintptr_t)(dstbuf.data() + doff) & 15u) != dp) doff++;
    const uint64_t usable = room < cut ? room : cut;
    D_LO = dstbuf.data() + doff; D_HI = D_LO + usable;
    written.assign((size_t)usable + 1, 0);
    // dst_off = {0, room}, total = cut behind the first entry's start: brx_text_room as the kernel calls it, entry 0 of 2
    const uint64_t dst_off[2] = {0, room};
    BrxTextArgs x;
    x.dialect = (uint32_t)dialect; x.q = q; x.e = e; x.text_len = NULL; x.status = NULL;
    x.dst_off = dst_off; x.dst = D_LO; x.total = cut;
    const BrxTextRoom d = brx_text_room(x, 2, 0);
    if (d.room != usable) die("brx_text_room");
    EmuMem mem;
    const BrxTextPlan p = brx_text_plan(mem, R_LO, (int64_t)L, spaces ? BRX_TEXT_F_SPACES : 0u, (uint32_t)dialect, q, e);
    BrxTextRes r;
    if (path == 0) r = emu_lane((uint32_t)dialect, mem, R_LO, (int64_t)L, p, q, e, d);
    else if (path == 1) r = emu_wave((uint32_t)dialect, R_LO, (int64_t)L, p, q, e, d);
    else r = p.mode == BRX_TEXT_M_JSON ? brx_text_serial(mem, R_LO, (int64_t)L, p, q, e, d) : emu_lane((uint32_t)dialect, mem, R_LO, (int64_t)L, p, q, e, d); // (as the kernel chooses)
    const int status = (int)brx_text_status(p, r.bad, r.closed);
    if (r.len != want.size()) { printf("len %llu want %zu (path %d dialect %d L %zu)\n", (unsigned long long)r.len, want.size(), path, dialect, L); die("text length differs"); }
    if (status != want_status) { printf("status %d want %d (path %d dialect %d L %zu)\n", status, want_status, path, dialect, L); die("status differs"); }
    const uint64_t n = want.size() < usable ? want.size() : usable;
    for (uint64_t t = 0; t < n; t++) {
        if (!written[(size_t)t]) die("a text byte inside the room was not written");
        if (D_LO[t] != want[(size_t)t]) { printf("byte %llu (path %d dialect %d L %zu)\n", (unsigned long long)t, path, dialect, L); die("text differs"); }
    }
    for (uint64_t t = n; t < usable; t++) if (written[(size_t)t]) die("a byte behind the text was written");
    for (size_t t = 0; t < dstbuf.size(); t++)
        if ((t < doff || t >= doff + usable) && dstbuf[t] != 0xA5) die("a byte outside the room changed");
}

static void run_record(const Bytes &rec, uint32_t sp, uint32_t dp, int dialect, uint32_t q, uint32_t e, bool spaces, uint64_t room, uint64_t cut) {
    Bytes want;
    const int st = ref_text(rec, dialect, (int)q, (int)e, spaces, want);
    if (want.size() > rec.size()) die("L' <= L does not hold");
    n_records++;
    if (brx_text_hex_escape((uint32_t)dialect, e)) { n_serial++; run_path(2, rec, sp, dp, dialect, q, e, spaces, room, cut, want, st); return; }
    run_path(0, rec, sp, dp, dialect, q, e, spaces, room, cut, want, st);
    run_path(1, rec, sp, dp, dialect, q, e, spaces, room, cut, want, st);
    if (rec.size() >= BRX_TEXT_LONG) n_lane_long++; else n_wave_short++;
}

// a record of exactly `len` bytes, rich in everything the walk branches on
static Bytes make_record(std::mt19937_64 &g, size_t len, int dialect, uint32_t q, uint32_t e, int richness) {
    static const char *frag[] = {"En", "E\\", "EE", "EQ", "E/", "Eb", "Et", "Eu00e9", "Eu00E9", "Eu0041", "Eu0000", "Eud83dEude00", "EuD83DEuDE00",
                                 "Eud83d", "Eude00", "Eud83dEu0041", "Eud83dEud83dEude00", "EEud83d", "Eu12", "Eu12g4", "Ex", "E", "Q", "QQ",
                                 "QQQ", "u", "d83d", "N", "EN", " ", "\t", "Ev", "E0", "Eud83dE", "Eud83dEu", "Eud83dEude0"};
    const size_t n_frag = sizeof(frag) / sizeof(frag[0]);
    Bytes r;
    if (dialect != 2 && g() % 8u) r.push_back((uint8_t)q);
    while (r.size() < len) {
        const uint32_t w = (uint32_t)(g() % 100u);
        if ((int)w < richness) {
            if (g() % 6u == 0) { // a run of the run byte
                const size_t k = 1 + g() % 40u;
                for (size_t t = 0; t < k; t++) r.push_back((uint8_t)(dialect == 0 ? q : e));
            } else {
                for (const char *s = frag[g() % n_frag]; *s; s++) r.push_back(*s == 'E' ? (uint8_t)e : *s == 'Q' ? (uint8_t)q : (uint8_t)*s);
            }
        } else {
            const uint64_t x = g(); // one draw per plain run
            const size_t k = 1 + x % 48u;
            for (size_t t = 0; t < k; t++) r.push_back((uint8_t)('a' + ((x >> 8) + t * 7u) % 26u));
        }
    }
    r.resize(len);
    if (len >= 2 && dialect != 2 && g() % 8u) r[len - 1] = (uint8_t)q;
    return r;
}

struct Check { int dialect; const char *rec; const char *text; size_t n; int status; bool spaces; };

int main() {
    std::mt19937_64 g(20261020);
    // the check values of include/brx.h
    static const Check table[] = {
        {1, "\"a\\tb\"", "a\tb", 3, 0, false}, {1, "\"\\u00e9\"", "\xC3\xA9", 2, 0, false}, {1, "\"\\ud83d\\ude00\"", "\xF0\x9F\x98\x80", 4, 0, false},
        {1, "\"\\\\\"", "\\", 1, 0, false}, {1, "\"\"", "", 0, 0, false}, {1, "null", "null", 4, 1, false},
        {1, "\"\\ud83d\"", "\xEF\xBF\xBD", 3, 3, false}, {1, "\"\\ud83d\\u0041\"", "\xEF\xBF\xBD" "A", 4, 3, false},
        {1, "\"\\ude00x\"", "\xEF\xBF\xBDx", 4, 3, false}, {1, "\"\\u12\"", "\\u12", 4, 3, false}, {1, "\"\\x\"", "\\x", 2, 3, false},
        {1, "\"a\"b\"", "a\"b", 3, 3, false}, {1, "\"abc\\\"", "abc\"", 4, 3, false}, {1, "\"abc", "abc", 3, 3, false}, {1, "\"", "", 0, 3, false},
        {1, " \"x\"\t", "x", 1, 0, true},
        {0, "\"a\"\"b\"", "a\"b", 3, 0, false}, {0, "\"\"\"\"", "\"", 1, 0, false}, {0, "\"\"", "", 0, 0, false}, {0, "", "", 0, 1, false},
        {0, "abc", "abc", 3, 1, false}, {0, "\"\"\"", "\"", 1, 3, false}, {0, "\"a\"b\"", "a\"b", 3, 3, false}, {0, "\"abc", "\"abc", 4, 3, false},
        {0, "\"", "\"", 1, 3, false},
        {2, "a\\tb", "a\tb", 3, 0, false}, {2, "\\,", ",", 1, 0, false}, {2, "\\\\N", "\\N", 2, 0, false}, {2, "x\\N", "xN", 2, 0, false},
        {2, "\\N", "", 0, 2, false}, {2, "a\\", "a\\", 2, 3, false}};
    for (const Check &c : table) {
        const Bytes rec(c.rec, c.rec + strlen(c.rec)), text(c.text, c.text + c.n);
        Bytes want;
        if (ref_text(rec, c.dialect, '"', '\\', c.spaces, want) != c.status || want != text) { printf("%s\n", c.rec); die("the restatement misses a check value"); }
        run_record(rec, 3, 5, c.dialect, '"', '\\', c.spaces, 64, 64);
    }
    // every length at every source phase and every destination phase
    const size_t max_len = BRX_TEXT_LONG + 2u * BRX_TEXT_ROW;
    met.assign((max_len + 1) * 256, 0);
    for (size_t len = 0; len <= max_len; len++) {
        for (uint32_t sp = 0; sp < 16u; sp++) {
            for (uint32_t dp = 0; dp < 16u; dp++) {
                const int dialect = (int)((len + sp + dp) % 3u);
                // long records are mostly plain (the copy path and its wide stores), short ones mostly escapes
                const Bytes rec = make_record(g, len, dialect, '"', '\\', len < 96 ? 60 : (sp + dp) % 8u == 0 ? 35 : 3);
                run_record(rec, sp, dp, dialect, '"', '\\', false, len, len);
                met[len * 256 + sp * 16 + dp] = 1;
            }
        }
    }
    for (size_t t = 0; t < met.size(); t++) if (!met[t]) die("a (length, source phase, destination phase) combination was not met");
    // random records: blanks around them, rooms and totals that cut the text, other quote and escape bytes (a hex digit among them)
    static const uint8_t qs[] = {'"', '\'', 'u', '9', 0}, es[] = {'\\', '^', 'u', 'n', 'a', 'F', '7', 0xFF};
    for (uint32_t it = 0; it < 60000u; it++) {
        const int dialect = (int)(g() % 3u);
        uint32_t q = qs[g() % sizeof(qs)], e = es[g() % sizeof(es)];
        if (it % 3u == 0) { q = '"'; e = '\\'; }
        if (dialect == 1 && q == e) continue;
        const size_t body = g() % 5u == 0 ? g() % 2600u : g() % 80u;
        Bytes rec;
        const bool spaces = g() % 2u;
        for (size_t k = g() % 4u; k && g() % 2u; k--) rec.push_back(g() % 2u ? 0x20 : 0x09);
        const Bytes mid = make_record(g, body, dialect, q, e, 10 + (int)(g() % 60u));
        rec.insert(rec.end(), mid.begin(), mid.end());
        for (size_t k = g() % 4u; k && g() % 2u; k--) rec.push_back(g() % 2u ? 0x20 : 0x09);
        const uint64_t room = g() % 3u ? rec.size() : g() % (rec.size() + 2);
        const uint64_t cut = g() % 4u ? room : g() % (room + 1);
        run_record(rec, (uint32_t)(g() % 16u), (uint32_t)(g() % 16u), dialect, q, e, spaces, room, cut);
    }
    // size mode: no destination at all
    {
        const Bytes rec = make_record(g, 3000, 1, '"', '\\', 30);
        Bytes want;
        ref_text(rec, 1, '"', '\\', false, want);
        A_LO = R_LO = rec.data(); A_HI = R_HI = rec.data() + rec.size();
        D_LO = D_HI = NULL;
        EmuMem mem;
        const BrxTextRoom none = {0, 0};
        const BrxTextPlan p = brx_text_plan(mem, R_LO, (int64_t)rec.size(), 0, 1, '"', '\\');
        if (emu_lane(1, mem, R_LO, (int64_t)rec.size(), p, '"', '\\', none).len != want.size()) die("size mode, lane path");
        if (emu_wave(1, R_LO, (int64_t)rec.size(), p, '"', '\\', none).len != want.size()) die("size mode, wave path");
    }
    printf("OK: %llu records, lengths 0 .. %zu at 16 x 16 phases; lane path on %llu long, wave path on %llu short, serial path on %llu; "
           "loads %llu wide %llu byte, stores %llu wide %llu byte\n",
           (unsigned long long)n_records, max_len, (unsigned long long)n_lane_long, (unsigned long long)n_wave_short, (unsigned long long)n_serial,
           (unsigned long long)n_wide_loads, (unsigned long long)n_byte_loads, (unsigned long long)n_wide_stores, (unsigned long long)n_byte_stores);
    return 0;
}
