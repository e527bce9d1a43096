// object_emu.cpp -- brx_object_batch on a CPU, lane by lane: the body of brx_object_kernel (brx_object.hip) around the REAL text of
// csrc/brx_object.h (and, through it, of brx_member.h's look at a key and brx_elements.h's unit walk) -- the lane path of every entry,
// the ballot over the long objects, the wave path with its scan across the lanes as a serial loop, the per-name ballots for the
// row's last match, the winners carried in lane q's register and the owner's stores -- with names and in extent mode, held to a
// boundary-serial restatement of THE RULE of include/brx.h that shares nothing with the headers.  Batches: the contract's check
// values; objects whose closer stands 1 .. 40, around BRX_OB_LONG, around one and two rows behind the opener, closed by '}' and by
// ']', cut by a line feed and by the stream's end, behind 0, 1, 5 and 15 leading boundaries; matches in lane 0, in lane 63 and in a
// second row, the same name in two lanes and in two rows, a match behind the stop lane, colons at depth 2 and deeper; key records of
// 64 and 65 bytes, blanks, tabs and CRs around keys, backslashes in keys, keys that are a prefix or an extension of a name; random
// JSON-ish lines with broken objects; every batch with each boundary of a stream (and indices behind them, and streams behind n) as
// an opener, with 0, 1, 5 and 8 names, and also with n_pos cut, garbage in what and pos, counts beyond the tables and optional
// outputs NULL.
// The run fails on: a load of `what` outside the stream's boundaries that count or at / behind n_pos; an arena load outside the
// stream; a store outside n_names * m; a slot (q, j) with j < m that was not written, or written more than once; a result that
// differs.
// No GPU.  Build and run: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I brotli-rs_amd/csrc tools/object_emu.cpp -o object_emu
// && ./object_emu (tests/test_object_abi.py does, without the sanitizers).  It proves the arithmetic, not the kernel's own text:
// that is tests/test_gpu_object.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include <string>
#include <vector>
#include "brx_object.h"
typedef std::vector<uint8_t> Bytes;

static void die(const char *what) { printf("FAIL: %s\n", what); exit(1); }

// what the policy checks against: set per batch, per entry in hand
static const uint8_t *S_LO, *S_HI;          // the stream of the entry in hand
static const uint8_t *W_BASE, *W_LO, *W_HI; // `what`, and the part of it that the entry in hand may load
static uint64_t N_POS, SLOTS;               // slots that may be stored to: [0, SLOTS) = n_names * m
static uint32_t *MEM_STREAM; static uint64_t *MEM_REC; static uint8_t *MEM_KIND;
static std::vector<uint8_t> w_stream, w_rec, w_kind; // how often a slot was stored to
static uint64_t n_wide, n_byte, n_arena;

struct EmuMem {
    uint8_t ld8(const uint8_t *p) { if (p < S_LO || p >= S_HI) die("byte load outside the stream"); n_arena++; return *p; }
    BrxTake128 ld128(const uint8_t *p) {
        if (p < S_LO || p + 16 > S_HI) die("16-byte load outside the stream");
        n_arena++;
        BrxTake128 v; memcpy(&v.lo, p, 8); memcpy(&v.hi, p + 8, 8); return v;
    }
    void chk_w(const uint8_t *p, uint32_t n) {
        if (p < W_LO || p + n > W_HI) die("load of what outside the boundaries of the stream that count");
        if ((uint64_t)(p - W_BASE) + n > N_POS) die("load of what at or behind n_pos");
    }
    uint8_t ldw8(const uint8_t *p) { chk_w(p, 1); n_byte++; return *p; }
    BrxTake128 ldw128(const uint8_t *p) { chk_w(p, 16); n_wide++; BrxTake128 v; memcpy(&v.lo, p, 8); memcpy(&v.hi, p + 8, 8); return v; }
    void slot(uint64_t at) { if (at >= SLOTS) die("store at or beyond n_names * m"); }
    void st32(uint32_t *p, uint32_t v) { const uint64_t at = p - MEM_STREAM; slot(at); w_stream[at]++; *p = v; }
    void st64(uint64_t *p, uint64_t v) { const uint64_t at = p - MEM_REC; slot(at); w_rec[at]++; *p = v; }
    void st8(uint8_t *p, uint8_t v) { const uint64_t at = p - MEM_KIND; slot(at); w_kind[at]++; *p = v; }
};

// ---- the definition, serially, with nothing shared with the headers ------------------------------------------------------------------
struct RefMem { uint64_t rec; uint8_t kind; };
struct Ref { uint8_t status; uint64_t end, members; uint8_t flags; std::vector<RefMem> mem; };
static uint8_t ref_kind(uint8_t w) { return (w == ',' || w == '}') ? 1 : w == '{' ? 2 : w == '[' ? 3 : 4; }
// s: the stream; pos, what: its part of the tables; C: its boundaries that count
static Ref ref_object(const Bytes &s, const uint64_t *pos, const uint8_t *what, uint64_t C, uint64_t r, const std::vector<std::string> &names) {
    Ref out = {1, ~(uint64_t)0, 0, 0, std::vector<RefMem>(names.size(), RefMem{~(uint64_t)0, 0})};
    if (r >= C) return out;
    if (what[r] != '{') { out.status = 2; return out; }
    long e = 1;
    for (uint64_t k = r + 1;; k++) {
        if (k == C) { out.status = 3; out.end = C; return out; }
        const uint8_t w = what[k];
        if (w == '\n') { out.status = 3; out.end = k; return out; }
        if (w == '{' || w == '[') e++;
        else if (w == '}' || w == ']') {
            if (--e == 0) { out.status = w == '}' ? 0 : 4; out.end = k; return out; }
        } else if (w == ':' && e == 1) {
            out.members++;
            const uint64_t l = s.size();
            uint64_t a = (pos[k - 1] < l ? pos[k - 1] : l) + 1, b = pos[k] < l ? pos[k] : l;
            if (a > l) a = l;
            if (b < a) b = a;
            if (b - a > 64) { out.flags |= 1; continue; }
            std::string key(s.begin() + a, s.begin() + b);
            if (key.find('\\') != std::string::npos) out.flags |= 2;
            size_t x = 0, y = key.size();
            while (x < y && (key[x] == ' ' || key[x] == '\t' || key[x] == '\r')) x++;
            while (y > x && (key[y - 1] == ' ' || key[y - 1] == '\t' || key[y - 1] == '\r')) y--;
            if (y - x < 2 || key[x] != '"' || key[y - 1] != '"') continue;
            const std::string body = key.substr(x + 1, y - x - 2);
            for (size_t q = 0; q < names.size(); q++)
                if (names[q] == body) out.mem[q] = {k + 1, k + 1 < C ? ref_kind(what[k + 1]) : (uint8_t)4};
        }
    }
}

// pos and what of brx_index_set_batch for one stream, restated
static void ref_index(const Bytes &s, std::vector<uint64_t> &pos, Bytes &what) {
    bool esc = false; uint64_t quotes = 0;
    for (size_t j = 0; j < s.size(); j++) {
        const uint8_t c = s[j];
        if (esc) { esc = false; continue; }
        if (c == '\\') esc = true;
        else if (c == '"') quotes++;
        else if (c && strchr("{}[]:,\n", c) && !(quotes & 1)) { pos.push_back(j); what.push_back(c); }
    }
}

// ---- one launch: the body of brx_object_kernel<NAMES>, wave by wave, its 64 lanes in turn --------------------------------------------
static uint64_t n_batches, n_entries, n_long, n_rows, n_hits, n_row_hits, n_two_lanes, n_later_rows, n_flagged;
#define DEAD 0xFFu

static void in_hand(const BrxObArgs &x, const BrxObEntry &en) {
    S_LO = x.a.out + x.a.out_off[en.i]; S_HI = S_LO + x.a.len[en.i];
    W_LO = x.what + en.base; W_HI = W_LO + en.c;
}

template <bool NAMES>
static void launch(const BrxObArgs &x, const BrxMbNames &nm) {
    EmuMem mem;
    const uint64_t m = x.a.m;
    for (uint64_t j0 = 0; j0 < m; j0 += 64) {
        BrxObRes res[64]; BrxObEntry mine[64]; bool is_long[64];
        for (uint32_t l = 0; l < 64; l++) {
            const uint64_t j = j0 + l;
            res[l] = {0, ~(uint64_t)0, DEAD, 0};
            mine[l] = {BRX_OB_NONE, 0, 0, 0, 0};
            is_long[l] = false;
            if (j >= m) continue;
            // (the opener's byte: the entry may load it if it is a boundary that counts; brx_ob_entry has checked that)
            W_LO = x.what; W_HI = x.what + N_POS; S_LO = S_HI = nullptr;
            mine[l] = brx_ob_entry(mem, x, j);
            res[l].status = mine[l].status;
            if (mine[l].status != BRX_OB_NONE && (mine[l].r >= mine[l].c || mine[l].base + mine[l].c > N_POS)) die("an entry that counts beyond C(i)");
            if (res[l].status == BRX_OB_OK) {
                in_hand(x, mine[l]);
                is_long[l] = !brx_ob_lane<NAMES>(mem, x, nm, mine[l], j, res[l]);
            }
            W_LO = W_HI = nullptr; S_LO = S_HI = nullptr; // (an entry that is no opener loads nothing more)
            if (NAMES && (res[l].status == BRX_OB_NONE || res[l].status == BRX_OB_NOT_OBJECT)) brx_ob_store_missing(mem, x, nm.n, j);
        }
        for (uint32_t owner = 0; owner < 64; owner++) { // (the loop over the ballot)
            if (!is_long[owner]) continue;
            n_long++;
            const BrxObEntry en = mine[owner];
            in_hand(x, en);
            int64_t depth = 1;
            uint64_t members[64], best[64]; uint32_t flags[64];
            for (uint32_t l = 0; l < 64; l++) { members[l] = 0; best[l] = 0; flags[l] = 0; }
            uint32_t rows_with_hit[BRX_MB_MAX_NAMES] = {0};
            for (uint64_t kb = en.r + 1u;; kb += BRX_OB_ROW) {
                n_rows++;
                BrxElMasks k[64]; int32_t sum[64], incl[64]; BrxElUnit u[64]; uint32_t nv[64]; uint64_t last[64];
                for (uint32_t l = 0; l < 64; l++) {
                    const uint64_t k0 = kb + l * BRX_MB_UNIT;
                    nv[l] = brx_mb_valid(en.c, k0);
                    k[l] = brx_ob_masks(brx_el_unit(mem, x.what, en.base, en.c, k0, nv[l]));
                    sum[l] = brx_el_unit_sum(k[l]);
                    incl[l] = (l ? incl[l - 1] : 0) + sum[l]; // (the scan)
                }
                uint32_t sl = 64;
                for (uint32_t l = 0; l < 64; l++) {
                    u[l] = brx_el_unit_walk(k[l], nv[l], brx_el_depth(depth, incl[l] - sum[l]));
                    if (u[l].stop != BRX_EL_STOP_NONE && sl == 64) sl = l; // (the ballot's first lane)
                }
                for (uint32_t l = 0; l < 64; l++) {
                    if (l > sl) u[l].sep = 0;
                    members[l] += (uint32_t)__builtin_popcount(u[l].sep);
                    last[l] = 0;
                    if (NAMES && u[l].sep) flags[l] |= brx_ob_unit_keys(mem, x, nm, en.i, kb + l * BRX_MB_UNIT, u[l].sep, 0u, last[l]);
                }
                if (NAMES) {
                    for (uint32_t q = 0; q < nm.n; q++) {
                        uint64_t hit = 0; // (the ballot)
                        for (uint32_t l = 0; l < 64; l++) if (brx_ob_last_of(last[l], q)) hit |= (uint64_t)1 << l;
                        if (hit) {
                            const uint32_t ll = 63u - (uint32_t)__builtin_clzll(hit);
                            best[q] = kb + ll * BRX_MB_UNIT + brx_ob_last_of(last[ll], q); // (lane q's register)
                            n_row_hits++;
                            if (hit & (hit - 1)) n_two_lanes++;
                            if (rows_with_hit[q]++) n_later_rows++;
                        }
                    }
                }
                if (sl < 64) {
                    uint64_t total = 0; uint32_t fl = 0;
                    for (uint32_t l = 0; l < 64; l++) { total += members[l]; fl |= flags[l]; } // (the wave sum, the two ballots)
                    res[owner].n_members = total;
                    res[owner].end = kb + sl * BRX_MB_UNIT + u[sl].at;
                    res[owner].status = u[sl].stop == BRX_EL_STOP_OK ? BRX_OB_OK : u[sl].stop == BRX_EL_STOP_MISMATCH ? BRX_OB_MISMATCH : BRX_OB_UNCLOSED;
                    res[owner].flags = fl & (BRX_MB_F_LONG_KEY | BRX_MB_F_ESCAPED_KEY);
                    break;
                }
                depth += incl[63];
            }
            if (NAMES) for (uint32_t q = 0; q < nm.n; q++) brx_ob_store_slot(mem, x, &mine[owner], q, j0 + owner, best[q]); // (the owner's thread)
        }
        for (uint32_t l = 0; l < 64; l++) {
            if (res[l].status == DEAD) continue;
            if (x.n_members) x.n_members[j0 + l] = res[l].n_members;
            if (x.status) x.status[j0 + l] = (uint8_t)res[l].status;
            if (x.end) x.end[j0 + l] = res[l].end;
            if (NAMES && x.obj_flags) x.obj_flags[j0 + l] = (uint8_t)res[l].flags;
        }
    }
}

// variant bits: 1 n_pos cut, 2 garbage in what, 4 garbage in pos, 8 counts beyond the tables, 64 optional outputs NULL
static void run(const std::vector<Bytes> &streams, const std::vector<std::string> &names, uint32_t variant, std::mt19937 &g) {
    const uint32_t n = (uint32_t)streams.size(), Q = (uint32_t)names.size();
    Bytes arena(5, '{'), what;
    std::vector<uint64_t> out_off(n), len(n), count(n), pos_off(n), pos;
    for (uint32_t i = 0; i < n; i++) {
        out_off[i] = arena.size(); len[i] = streams[i].size();
        arena.insert(arena.end(), streams[i].begin(), streams[i].end());
        arena.insert(arena.end(), i % 5, '"'); // slack between streams, of quotes
        pos_off[i] = pos.size();
        ref_index(streams[i], pos, what);
        count[i] = pos.size() - pos_off[i];
    }
    uint64_t n_pos = pos.size();
    if ((variant & 1) && n_pos) n_pos -= 1 + g() % (n_pos < 40 ? n_pos : 40);
    if (variant & 2) for (size_t t = g() % 7; t < what.size(); t += 1 + g() % 9) what[t] = (uint8_t)g();
    if (variant & 4) for (size_t t = g() % 7; t < pos.size(); t += 1 + g() % 9) pos[t] = g() % 3 ? g() % 5000 : ~(uint64_t)0 - g() % 3;
    // the selection: every boundary of every stream as an opener, two indices behind them, a stream behind n, MISSING, and repeats
    std::vector<uint32_t> sel_stream; std::vector<uint64_t> sel_rec;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t c = count[i], step = c > 3000 ? 1 + g() % 40 : 1;
        for (uint64_t r = 0; r < c + 2; r += (what.size() > pos_off[i] + r && what[pos_off[i] + r] == '{') ? 1 : step) { sel_stream.push_back(i); sel_rec.push_back(r); }
        sel_stream.push_back(i); sel_rec.push_back(~(uint64_t)0);
        sel_stream.push_back(n + g() % 3); sel_rec.push_back(g() % 4);
        if (c) { const uint64_t r = g() % c; for (int t = 0; t < 2; t++) { sel_stream.push_back(i); sel_rec.push_back(r); } }
    }
    if (variant & 8) for (uint32_t i = 0; i < n; i++) count[i] += i + 1 == n ? (uint64_t)1 << 40 : g() % 50;
    const uint64_t m = sel_stream.size(), slots = (uint64_t)Q * m;
    // the reference, under the cut and the garbage
    std::vector<Ref> ref(m);
    for (uint64_t j = 0; j < m; j++) {
        const uint32_t i = sel_stream[j];
        if (i >= n) { ref[j] = {1, ~(uint64_t)0, 0, 0, std::vector<RefMem>(Q, RefMem{~(uint64_t)0, 0})}; continue; }
        uint64_t c = count[i];
        if (pos_off[i] >= n_pos) c = 0; else if (c > n_pos - pos_off[i]) c = n_pos - pos_off[i];
        ref[j] = ref_object(streams[i], pos.data() + pos_off[i], what.data() + pos_off[i], c, sel_rec[j], names);
    }
    const uint64_t P64 = 0x5151515151515151ull;
    std::vector<uint64_t> n_members(m + 4, P64), end(m + 4, P64), mem_rec(slots + 4, P64);
    std::vector<uint32_t> mem_stream(slots + 4, 0x51515151u);
    Bytes status(m + 4, 0x51), obj_flags(m + 4, 0x51), mem_kind(slots + 4, 0x51);
    BrxMbNames nm; memset(&nm, 0, sizeof nm);
    nm.n = Q;
    for (uint32_t q = 0; q < Q; q++) { nm.len[q] = (uint32_t)names[q].size(); memcpy(nm.w[q], names[q].data(), names[q].size()); }
    BrxObArgs x; memset(&x, 0, sizeof x);
    x.a.out = arena.data(); x.a.out_off = out_off.data(); x.a.len = len.data(); x.a.n = n; x.a.span = arena.size();
    x.a.count = count.data(); x.a.pos_off = pos_off.data(); x.a.pos = pos.data(); x.a.n_pos = n_pos; x.a.delim_len = 1; x.a.flags = BRX_TAKE_F_NO_DELIM;
    x.a.sel_stream = sel_stream.data(); x.a.sel_rec = sel_rec.data(); x.a.m = m;
    x.what = what.data(); x.n_members = n_members.data(); x.status = status.data(); x.end = end.data();
    bool have_flags = false;
    if (Q) { x.mem_stream = mem_stream.data(); x.mem_rec = mem_rec.data(); x.mem_kind = mem_kind.data(); x.obj_flags = obj_flags.data(); have_flags = true; }
    if (variant & 64) { // optional outputs NULL (n_members stays in extent mode: it is required there)
        if (Q) x.n_members = nullptr;
        x.end = nullptr;
        if (g() % 2) x.status = nullptr;
        if (g() % 2) { x.obj_flags = nullptr; have_flags = false; }
    }
    W_BASE = what.data(); N_POS = n_pos; SLOTS = slots;
    MEM_STREAM = mem_stream.data(); MEM_REC = mem_rec.data(); MEM_KIND = mem_kind.data();
    w_stream.assign(slots, 0); w_rec.assign(slots, 0); w_kind.assign(slots, 0);
    if (Q) launch<true>(x, nm); else launch<false>(x, nm);
    for (uint64_t j = 0; j < m; j++) {
        const Ref &w = ref[j];
        if (x.n_members ? n_members[j] != w.members : n_members[j] != P64) { printf("entry %llu (stream %u r %llu): n_members %llu, want %llu\n", (unsigned long long)j, sel_stream[j], (unsigned long long)sel_rec[j], (unsigned long long)n_members[j], (unsigned long long)w.members); die("n_members differs"); }
        if (x.status ? status[j] != w.status : status[j] != 0x51) { printf("entry %llu: status %u, want %u\n", (unsigned long long)j, status[j], w.status); die("status differs"); }
        if (x.end ? end[j] != w.end : end[j] != P64) { printf("entry %llu: end %llu, want %llu\n", (unsigned long long)j, (unsigned long long)end[j], (unsigned long long)w.end); die("end differs"); }
        if (have_flags ? obj_flags[j] != w.flags : obj_flags[j] != 0x51) { printf("entry %llu (stream %u r %llu): flags %u, want %u\n", (unsigned long long)j, sel_stream[j], (unsigned long long)sel_rec[j], obj_flags[j], w.flags); die("obj_flags differs"); }
        for (uint32_t q = 0; q < Q; q++) {
            const uint64_t at = (uint64_t)q * m + j;
            if (w_stream[at] != 1 || w_rec[at] != 1 || w_kind[at] != 1) die("a slot was not written exactly once");
            if (mem_stream[at] != sel_stream[j] || mem_rec[at] != w.mem[q].rec || mem_kind[at] != w.mem[q].kind) {
                printf("entry %llu (stream %u r %llu) name %u: stream %u rec %llu kind %u, want rec %llu kind %u\n", (unsigned long long)j, sel_stream[j],
                       (unsigned long long)sel_rec[j], q, mem_stream[at], (unsigned long long)mem_rec[at], mem_kind[at],
                       (unsigned long long)w.mem[q].rec, w.mem[q].kind);
                die("a member differs");
            }
            if (w.mem[q].kind) n_hits++;
        }
        if (w.flags) n_flagged++;
        n_entries++;
    }
    for (uint64_t t = m; t < m + 4; t++) if (n_members[t] != P64 || end[t] != P64 || status[t] != 0x51 || obj_flags[t] != 0x51) die("canary behind m");
    for (uint64_t t = slots; t < slots + 4; t++) if (mem_stream[t] != 0x51515151u || mem_rec[t] != P64 || mem_kind[t] != 0x51) die("canary behind n_names * m");
    n_batches++;
}

static const std::vector<std::string> ABCUX = {"a", "b", "c", "u", "x"};
static const std::string K32(32, 'k');
static const std::vector<std::string> EIGHT = {"a", "id", "items", "meta", K32, "a_rather_long_key_of_32_bytes_xx", "b", "ab"};

static void run_all(const std::vector<Bytes> &streams, std::mt19937 &g) {
    for (uint32_t v : {0u, 1u, 2u, 4u, 8u, 64u, 1u | 2u | 4u | 8u, 79u}) run(streams, ABCUX, v, g);
    for (uint32_t v : {0u, 79u}) {
        run(streams, {}, v, g);
        run(streams, {"b"}, v, g);
        run(streams, EIGHT, v, g);
    }
}

static Bytes B(const std::string &s) { return Bytes(s.begin(), s.end()); }

// an object whose closer stands `dist` boundaries behind its opener; style 0: scalar members only, 1: nested values and strings too
static std::string object_with(uint64_t dist, std::mt19937 &g, int style) {
    static const char *keys[] = {"a", "b", "c", "u", "x", "ab", "zz", "id"};
    std::string s = "{";
    uint64_t have = 0; // boundaries behind the opener so far
    while (have + 1 < dist) {
        const uint64_t left = dist - 1 - have;
        const std::string key = std::string(g() % 4 ? "" : " ") + "\"" + keys[g() % 8] + "\"" + (g() % 5 ? "" : "\t");
        const uint32_t pick = style == 0 ? 0 : g() % 6;
        if (pick == 1 && left >= 5) { s += key + ":[1,2],"; have += 5; }
        else if (pick == 2 && left >= 5) { s += key + ":{\"a\":7},"; have += 5; }
        else if (pick == 3 && left >= 7) { s += key + ":[{\"b\":[]}],"; have += 7; }
        else if (pick == 4 && left >= 2) { s += key + ":\"a}:{,\\\"\","; have += 2; }
        else if (left >= 2) { s += key + ":" + std::to_string(g() % 100) + ","; have += 2; }
        else { s += key + ":1"; have += 1; }
    }
    return s + "}";
}

static Bytes line_with(uint64_t lead, const std::string &obj, const std::string &tail) {
    std::string s;
    for (uint64_t t = 0; t < lead; t++) s += ",";
    return B(s + obj + tail);
}

static Bytes random_jsonl(std::mt19937 &g, uint32_t n_lines) {
    std::string s;
    const char *vals[] = {"1", "\"a,b:{c}\"", "{\"a\":1,\"b\":[2,{\"a\":3}]}", "[1,2,{\"id\":7}]", "null", "\"\\\\\"", "\"q\\\"}\"", " 12 ", "-3.5e2", "{}", "{ }", "{\"u\":{\"u\":{}}}", "", ":"};
    const char *keys[] = {"a", "b", "c", "u", "x", "id", "items", "meta", "ab", "a\\u0062", "a_rather_long_key_of_32_bytes_xx", ""};
    for (uint32_t r = 0; r < n_lines; r++) {
        std::string line = "{\"meta\":{";
        const uint32_t nm_ = g() % 4 ? g() % 9 : g() % 200;
        for (uint32_t e = 0; e < nm_; e++) {
            if (e) line += g() % 3 ? "," : " , ";
            line += std::string(g() % 6 ? 0 : g() % 70, ' ') + "\"" + keys[g() % 12] + "\"" + (g() % 4 ? "" : " \r") + ":" + vals[g() % 14];
        }
        line += "},\"items\":[{\"id\":1,\"a\":2},{\"id\":2}]}";
        const uint32_t kind = g() % 12;
        if (kind == 0) line = line.substr(0, g() % (line.size() + 1));
        else if (kind == 1) { const size_t at = line.find('}', g() % line.size()); if (at != std::string::npos) line[at] = ']'; }
        else if (kind == 2) { const size_t at = line.find('}', g() % line.size()); if (at != std::string::npos) line.erase(at, 1); }
        else if (kind == 3) line.insert(g() % line.size(), "\n");
        s += line;
        if (r + 1 < n_lines || g() % 2) s += "\n";
    }
    return B(s);
}

int main() {
    std::mt19937 g(2025);
    run_all({B("{\"u\":{\"a\":1,\"b\":[2,3],\"a\":4},\"a\":5}"), B("{\"a\":{}}"), B("{\"a\":{\"b\":1]}"), B("{\"a\":{\"b\":1,\"c\":2\n"), B("{\"a\":{\"b\":"),
             B("{\"a\":{\"x\":{\"b\":1},\"b\":2}}"), B("{\"items\":[{\"id\":1},{\"id\":2}]}"), B("{\"a\":[1]}"),
             B("{\"a\":{" + std::string(30, ' ') + "\"" + K32 + "\":1}}"), B("{\"a\":{" + std::string(31, ' ') + "\"" + K32 + "\":1}}"),
             B("{\"a\":{\"a\\u0062\":1}}"), B("{\"a\":{ \"b\"\t:1,\r\"ab\" :2,\"\":3,\"bb\":4,b:5,\"b:6}}"),
             B(""), B("{"), B("{}"), B("}"), B("{\n"), B("{]"), B("{:"), B("{:}"), B("{\"b\":\n")}, g);
    const uint64_t L = BRX_OB_LONG, R = BRX_OB_ROW;
    std::vector<uint64_t> dists;
    for (uint64_t d = 1; d <= 40; d++) dists.push_back(d);
    for (uint64_t d : {L - 1, L, L + 1, L + 2, R - 1, R, R + 1, R + 2, R + L, 2 * R - 1, 2 * R, 2 * R + 1, 2 * R + 3, 3 * R + 17}) dists.push_back(d);
    for (int style = 0; style < 2; style++)
        for (uint64_t lead : {0u, 1u, 5u, 15u}) {
            std::vector<Bytes> streams;
            for (uint64_t d : dists) {
                streams.push_back(line_with(lead + d % 3, object_with(d, g, style), d % 2 ? "}\n" : ""));
                if (d > 2) { // the same object cut by a line feed, by the stream's end, closed by ']'
                    std::string a = object_with(d, g, style);
                    streams.push_back(line_with(lead, a.substr(0, a.size() - 1), "\n{\"a\":1}"));
                    streams.push_back(line_with(lead, a.substr(0, a.size() - 1), ""));
                    streams.push_back(line_with(lead, a.substr(0, a.size() - 1) + "]", ",\"a\":1}"));
                }
            }
            run_all(streams, g);
        }
    { // matches at chosen places of long objects: lane 0, lane 63, a second row, two lanes of a row, two rows, behind the stop, at depth 2
        std::vector<Bytes> streams;
        const std::string f16 = "\"z\":0,\"z\":0,\"z\":0,\"z\":0,\"z\":0,\"z\":0,\"z\":0,\"z\":0,"; // 16 boundaries of members that carry no name
        auto fill = [&](uint64_t units) { std::string s; for (uint64_t t = 0; t < units; t++) s += f16; return s; };
        streams.push_back(B("{\"a\":1," + fill(70) + "\"q\":0}"));                          // lane 0 of the first row
        streams.push_back(B("{" + fill(63) + "\"b\":[1],\"z\":0," + fill(8) + "}"));       // lane 63
        streams.push_back(B("{" + fill(64) + "\"c\":{\"a\":9},\"z\":0," + fill(3) + "}")); // the second row's lane 0; an 'a' at depth 2
        streams.push_back(B("{\"a\":1," + fill(20) + "\"a\":2," + fill(20) + "\"a\":3," + fill(70) + "\"a\":4," + fill(70) + "\"b\":5}")); // two lanes, two rows
        streams.push_back(B("{\"a\":1,\"a\":2,\"b\":3,\"a\":4," + fill(70) + "}"));         // one unit with three of a name
        streams.push_back(B("{" + fill(10) + "\"a\":1},\"a\":2,\"b\":3," + fill(70) + "}")); // matches behind the stop lane in the same row
        streams.push_back(B("{" + fill(10) + "\"a\":1\n,\"a\":2,\"b\":3," + fill(70) + "}"));
        streams.push_back(B("{" + fill(70) + "\"u\":{\"a\":1,\"x\":{\"a\":2,\"b\":[{\"a\":3}]}},\"x\":[{\"a\":4}]," + fill(70) + "}")); // deeper colons
        streams.push_back(B("{\"u\":{" + fill(200) + "\"a\":1},\"a\":2}"));                  // a long object inside: the outer sees one 'a'
        std::string deep;
        for (int t = 0; t < 1500; t++) deep += "{\"a\":";
        deep += "1";
        for (int t = 0; t < 1500; t++) deep += "}";
        streams.push_back(B("{\"b\":" + deep + ",\"a\":2}"));
        streams.push_back(B("{" + std::string(3000, ':') + "}"));
        streams.push_back(B("{[" + std::string(2500, ':') + "]" + std::string(1100, ':') + "}"));
        for (uint32_t at : {0u, 15u, 16u, 1007u, 1008u, 1023u, 1024u, 1025u, 2047u, 2048u}) { // the stop at a given boundary behind the opener
            streams.push_back(B("{" + std::string(at, ',') + "\"a\":1}"));
            streams.push_back(B("{" + std::string(at, ',') + "\"a\":1\n}"));
            streams.push_back(B("{" + std::string(at, ',') + "\"a\":"));
            streams.push_back(B("{" + std::string(at, ',') + "\"a\":]"));
        }
        run_all(streams, g);
    }
    for (uint32_t it = 0; it < 30; it++) {
        std::vector<Bytes> streams;
        const uint32_t n = 1 + g() % 10;
        for (uint32_t i = 0; i < n; i++) streams.push_back(random_jsonl(g, g() % 6 ? g() % 12 : g() % 60));
        run_all(streams, g);
    }
    if (n_long < 1000 || n_rows < n_long || n_hits < 100000 || n_two_lanes < 100 || n_later_rows < 100 || n_flagged < 1000) die("the batches did not reach what they are for");
    printf("OK: %llu batches, %llu entries (%llu of them the wave's, in %llu rows of %u boundaries; BRX_OB_LONG %u), %llu slots that hold a member, "
           "%llu (name, row) pairs with a match, %llu of them in two lanes or more, %llu in a later row than an earlier match, %llu entries with flags, "
           "%llu wide and %llu byte loads of what, %llu arena loads\n",
           (unsigned long long)n_batches, (unsigned long long)n_entries, (unsigned long long)n_long, (unsigned long long)n_rows, BRX_OB_ROW,
           BRX_OB_LONG, (unsigned long long)n_hits, (unsigned long long)n_row_hits, (unsigned long long)n_two_lanes,
           (unsigned long long)n_later_rows, (unsigned long long)n_flagged, (unsigned long long)n_wide, (unsigned long long)n_byte,
           (unsigned long long)n_arena);
    return 0;
}
