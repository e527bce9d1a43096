// elements_emu.cpp -- brx_elements_batch on a CPU, lane by lane: the body of brx_elements_kernel (brx_elements.hip) around the REAL text
// of csrc/brx_elements.h -- the lane path of every entry, the ballot over the long arrays, the wave path with its two scans across the
// lanes as serial loops and its carries from row to row -- in count mode and in fill mode, held to a boundary-serial restatement of
// THE RULE of include/brx.h that shares nothing with the header.  Batches: the contract's check values; arrays of 0, 1, 2 elements
// with blanks; closers at every distance 1 .. 40, around BRX_EL_LONG, around one and two rows; nested elements across lanes and rows;
// rows of commas only; stops by line feed and by the stream's end in every lane; random JSON-ish streams with broken arrays; every
// batch with each boundary of a stream (and indices behind them, and streams behind n) as an opener, and also with n_pos cut, garbage
// in what and pos, counts beyond the tables, rooms smaller than the arrays and a total that cuts the last entries.
// The run fails on: a load of `what` outside the stream's boundaries that count or at / behind n_pos; an arena load outside the
// stream; a store outside the entry's room or at / beyond total; an element's slot that was not written or a slot written that holds
// no element; a result that differs.
// No GPU.  Build and run: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I brotli-rs_amd/csrc tools/elements_emu.cpp -o elements_emu
// && ./elements_emu (tests/test_elements_abi.py does, without the sanitizers).  It proves the arithmetic, not the kernel's own text:
// that is tests/test_gpu_elements.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include <string>
#include <vector>
#include "brx_elements.h"
typedef std::vector<uint8_t> Bytes;

static void die(const char *what) { printf("FAIL: %s\n", what); exit(1); }

// what the policy checks against: set per batch, per entry in hand
static const uint8_t *S_LO, *S_HI;          // the stream of the entry in hand
static const uint8_t *W_BASE, *W_LO, *W_HI; // `what`, and the part of it that the entry in hand may load
static uint64_t N_POS, TOTAL, ROOM_LO, ROOM_HI; // the slots the entry in hand may store to: [ROOM_LO, ROOM_HI), below TOTAL
static uint32_t *EL_STREAM; static uint64_t *EL_REC; static uint8_t *EL_KIND;
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
    void slot(uint64_t at) { if (at < ROOM_LO || at >= ROOM_HI || at >= TOTAL) die("store outside the entry's room or at / beyond total"); }
    void st32(uint32_t *p, uint32_t v) { const uint64_t at = p - EL_STREAM; slot(at); w_stream[at]++; *p = v; }
    void st64(uint64_t *p, uint64_t v) { const uint64_t at = p - EL_REC; slot(at); w_rec[at]++; *p = v; }
    void st8(uint8_t *p, uint8_t v) { const uint64_t at = p - EL_KIND; slot(at); w_kind[at]++; *p = v; }
};

// ---- the definition, serially, with nothing shared with brx_elements.h ---------------------------------------------------------------
struct RefEl { uint64_t rec; uint8_t kind; };
struct Ref { uint8_t status; uint64_t end; std::vector<RefEl> els; };
static uint8_t ref_kind(uint8_t w) { return (w == ',' || w == ']' || w == '}') ? 1 : w == '{' ? 2 : w == '[' ? 3 : 4; }
// s: the stream; pos, what: its part of the tables; C: its boundaries that count
static Ref ref_elements(const Bytes &s, const uint64_t *pos, const uint8_t *what, uint64_t C, uint64_t r) {
    Ref out = {1, ~(uint64_t)0, {}};
    if (r >= C) return out;
    if (what[r] != '[') { out.status = 2; return out; }
    long e = 1;
    uint64_t sep = r;
    for (uint64_t k = r + 1;; k++) {
        if (k == C) { out.status = 3; out.end = C; return out; }
        const uint8_t w = what[k];
        if (w == '\n') { out.status = 3; out.end = k; return out; }
        if (w == '{' || w == '[') e++;
        else if (w == '}' || w == ']') {
            if (--e == 0) {
                out.status = w == ']' ? 0 : 4; out.end = k;
                if (k == r + 1) {
                    const uint64_t l = s.size();
                    uint64_t a = (pos[r] < l ? pos[r] : l) + 1, b = pos[k] < l ? pos[k] : l;
                    if (a > l) a = l;
                    if (b < a) b = a;
                    bool blank = b - a <= 64;
                    for (uint64_t t = a; t < b && blank; t++) blank = s[t] == ' ' || s[t] == '\t' || s[t] == '\r';
                    if (blank) return out;
                }
                out.els.push_back({sep + 1, ref_kind(what[sep + 1])});
                return out;
            }
        } else if (w == ',' && e == 1) { out.els.push_back({sep + 1, ref_kind(what[sep + 1])}); sep = k; }
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

// ---- one launch: the body of brx_elements_kernel<FILL>, wave by wave, its 64 lanes in turn -------------------------------------------
static uint64_t n_batches, n_entries, n_elements, n_long, n_rows, n_pending_rows, n_empty;

static void in_hand(const BrxElArgs &x, const BrxElEntry &en, uint64_t j) {
    S_LO = x.a.out + x.a.out_off[en.i]; S_HI = S_LO + x.a.len[en.i];
    W_LO = x.what + en.base; W_HI = W_LO + en.c;
    ROOM_LO = ROOM_HI = 0;
    if (x.el_off) {
        const uint64_t a = x.el_off[j], b = j + 1 < x.a.m ? x.el_off[j + 1] : x.total;
        ROOM_LO = a; ROOM_HI = b > a ? b : a;
    }
}

template <bool FILL>
static void launch(const BrxElArgs &x) {
    EmuMem mem;
    const uint64_t m = x.a.m;
    for (uint64_t j0 = 0; j0 < m; j0 += 64) {
        BrxElRes res[64]; BrxElEntry mine[64]; bool is_long[64];
        for (uint32_t l = 0; l < 64; l++) {
            const uint64_t j = j0 + l;
            res[l] = {0, ~(uint64_t)0, BRX_EL_NONE};
            mine[l] = {BRX_EL_NONE, 0, 0, 0, 0, 0, 0};
            is_long[l] = false;
            if (j >= m) continue;
            // (the opener's byte: the entry may load it if it is a boundary that counts; brx_el_entry has checked that)
            W_LO = x.what; W_HI = x.what + N_POS; S_LO = S_HI = nullptr; ROOM_LO = ROOM_HI = 0;
            mine[l] = brx_el_entry(mem, x, j);
            res[l].status = mine[l].status;
            if (mine[l].status != BRX_EL_NONE) {
                if (mine[l].r >= mine[l].c || mine[l].base + mine[l].c > N_POS) die("an entry that counts beyond C(i)");
            }
            if (mine[l].status == BRX_EL_OK) {
                in_hand(x, mine[l], j);
                is_long[l] = !brx_el_lane<FILL>(mem, x, mine[l], res[l]);
            }
        }
        for (uint32_t owner = 0; owner < 64; owner++) { // (the loop over the ballot)
            if (!is_long[owner]) continue;
            n_long++;
            const BrxElEntry en = mine[owner];
            in_hand(x, en, j0 + owner);
            int64_t depth = 1;
            uint64_t seps = 0, pend = en.r;
            for (uint64_t kb = en.r + 1u;; kb += BRX_EL_ROW) {
                n_rows++;
                BrxElMasks k[64]; BrxTake128 v[64]; int32_t sum[64], incl[64], cl[64], cincl[64]; BrxElUnit u[64]; uint32_t nv[64];
                for (uint32_t l = 0; l < 64; l++) {
                    const uint64_t k0 = kb + l * BRX_MB_UNIT;
                    nv[l] = brx_mb_valid(en.c, k0);
                    v[l] = brx_el_unit(mem, x.what, en.base, en.c, k0, nv[l]);
                    k[l] = brx_el_masks(v[l]);
                    sum[l] = brx_el_unit_sum(k[l]);
                    incl[l] = (l ? incl[l - 1] : 0) + sum[l]; // (the scan)
                }
                uint32_t sl = 64;
                for (uint32_t l = 0; l < 64; l++) {
                    u[l] = brx_el_unit_walk(k[l], nv[l], brx_el_depth(depth, incl[l] - sum[l]));
                    if (u[l].stop != BRX_EL_STOP_NONE && sl == 64) sl = l; // (the ballot's first lane)
                }
                uint64_t with = 0;
                for (uint32_t l = 0; l < 64; l++) {
                    if (l > sl) u[l].sep = 0;
                    cl[l] = __builtin_popcount(u[l].sep);
                    cincl[l] = (l ? cincl[l - 1] : 0) + cl[l];
                    if (cl[l]) with |= (uint64_t)1 << l;
                }
                const uint32_t how = sl < 64 ? u[sl].stop : BRX_EL_STOP_NONE;
                const bool closed = how == BRX_EL_STOP_OK || how == BRX_EL_STOP_MISMATCH;
                if (FILL) {
                    if (with || closed) brx_el_store_at(mem, x, en, seps, pend); // (lane 0)
                    else n_pending_rows++;
                    for (uint32_t l = 0; l < 64; l++) {
                        const bool later = closed || (l < 63u && (with >> (l + 1u)) != 0);
                        brx_el_unit_store(mem, x, en, kb + l * BRX_MB_UNIT, v[l], u[l].sep, seps + 1u + (uint32_t)(cincl[l] - cl[l]), later);
                    }
                }
                if (with) {
                    const uint32_t ll = 63u - (uint32_t)__builtin_clzll(with);
                    pend = kb + ll * BRX_MB_UNIT + (31u - (uint32_t)__builtin_clz(u[ll].sep));
                }
                seps += (uint32_t)cincl[63];
                if (sl < 64) {
                    res[owner].n_elem = seps + (closed ? 1u : 0u);
                    res[owner].end = kb + sl * BRX_MB_UNIT + u[sl].at;
                    res[owner].status = how == BRX_EL_STOP_OK ? BRX_EL_OK : how == BRX_EL_STOP_MISMATCH ? BRX_EL_MISMATCH : BRX_EL_UNCLOSED;
                    break;
                }
                depth += incl[63];
            }
        }
        for (uint32_t l = 0; l < 64 && j0 + l < m; l++) {
            if (x.n_elem) x.n_elem[j0 + l] = res[l].n_elem;
            if (x.status) x.status[j0 + l] = (uint8_t)res[l].status;
            if (x.end) x.end[j0 + l] = res[l].end;
        }
    }
}

// variant bits: 1 n_pos cut, 2 garbage in what, 4 garbage in pos, 8 counts beyond the tables, 16 small rooms, 32 total cuts, 64 optional outputs NULL
static void run(const std::vector<Bytes> &streams, uint32_t variant, std::mt19937 &g) {
    const uint32_t n = (uint32_t)streams.size();
    Bytes arena(5, '['), what;
    std::vector<uint64_t> out_off(n), len(n), count(n), pos_off(n), pos;
    for (uint32_t i = 0; i < n; i++) {
        out_off[i] = arena.size(); len[i] = streams[i].size();
        arena.insert(arena.end(), streams[i].begin(), streams[i].end());
        arena.insert(arena.end(), i % 5, ' '); // slack between streams, of blanks
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
        for (uint64_t r = 0; r < c + 2; r += (what.size() > pos_off[i] + r && what[pos_off[i] + r] == '[') ? 1 : step) { sel_stream.push_back(i); sel_rec.push_back(r); }
        sel_stream.push_back(i); sel_rec.push_back(~(uint64_t)0);
        sel_stream.push_back(n + g() % 3); sel_rec.push_back(g() % 4);
        if (c) { const uint64_t r = g() % c; for (int t = 0; t < 2; t++) { sel_stream.push_back(i); sel_rec.push_back(r); } }
    }
    if (variant & 8) for (uint32_t i = 0; i < n; i++) count[i] += i + 1 == n ? (uint64_t)1 << 40 : g() % 50;
    const uint64_t m = sel_stream.size();
    // the reference, under the cut and the garbage
    std::vector<Ref> ref(m);
    std::vector<uint64_t> el_off(m);
    uint64_t total = 0;
    for (uint64_t j = 0; j < m; j++) {
        const uint32_t i = sel_stream[j];
        el_off[j] = total;
        if (i >= n) { ref[j] = {1, ~(uint64_t)0, {}}; continue; }
        uint64_t c = count[i];
        if (pos_off[i] >= n_pos) c = 0; else if (c > n_pos - pos_off[i]) c = n_pos - pos_off[i];
        ref[j] = ref_elements(streams[i], pos.data() + pos_off[i], what.data() + pos_off[i], c, sel_rec[j]);
        uint64_t room = ref[j].els.size();
        if ((variant & 16) && room && g() % 3 == 0) room = g() % room; // a room below the number of elements
        if ((variant & 16) && g() % 5 == 0) room += g() % 3;          // ... or above it
        total += room;
    }
    if ((variant & 32) && total) total -= 1 + g() % (total < 70 ? total : 70);
    if (variant & 16) for (uint64_t j = g() % 9; j + 1 < m; j += 1 + g() % 300) el_off[j] = el_off[j + 1] + g() % 3; // a negative room
    std::vector<uint64_t> n_elem(m + 4, 0x5151515151515151ull), end(m + 4, 0x5151515151515151ull), el_rec(total + 4, 0x5151515151515151ull);
    std::vector<uint32_t> el_stream(total + 4, 0x51515151u);
    Bytes status(m + 4, 0x51), el_kind(total + 4, 0x51);
    BrxElArgs x; memset(&x, 0, sizeof x);
    x.a.out = arena.data(); x.a.out_off = out_off.data(); x.a.len = len.data(); x.a.n = n; x.a.span = arena.size();
    x.a.count = count.data(); x.a.pos_off = pos_off.data(); x.a.pos = pos.data(); x.a.n_pos = n_pos; x.a.delim_len = 1; x.a.flags = BRX_TAKE_F_NO_DELIM;
    x.a.sel_stream = sel_stream.data(); x.a.sel_rec = sel_rec.data(); x.a.m = m;
    x.what = what.data(); x.n_elem = n_elem.data(); x.status = status.data(); x.end = end.data();
    W_BASE = what.data(); N_POS = n_pos; TOTAL = 0;
    EL_STREAM = el_stream.data(); EL_REC = el_rec.data(); EL_KIND = el_kind.data();
    w_stream.assign(total, 0); w_rec.assign(total, 0); w_kind.assign(total, 0);
    auto results = [&](const char *mode) {
        for (uint64_t j = 0; j < m; j++) {
            if (x.n_elem && n_elem[j] != ref[j].els.size()) { printf("%s entry %llu (stream %u r %llu): n_elem %llu, want %zu\n", mode, (unsigned long long)j, sel_stream[j], (unsigned long long)sel_rec[j], (unsigned long long)n_elem[j], ref[j].els.size()); die("n_elem differs"); }
            if (x.status && status[j] != ref[j].status) { printf("%s entry %llu: status %u, want %u\n", mode, (unsigned long long)j, status[j], ref[j].status); die("status differs"); }
            if (x.end && end[j] != ref[j].end) { printf("%s entry %llu: end %llu, want %llu\n", mode, (unsigned long long)j, (unsigned long long)end[j], (unsigned long long)ref[j].end); die("end differs"); }
        }
        for (uint64_t t = m; t < m + 4; t++) if (n_elem[t] != 0x5151515151515151ull || end[t] != 0x5151515151515151ull || status[t] != 0x51) die("canary behind m");
    };
    launch<false>(x); // count mode
    results("count");
    // fill mode
    std::fill(n_elem.begin(), n_elem.end(), 0x5151515151515151ull); std::fill(end.begin(), end.end(), 0x5151515151515151ull);
    std::fill(status.begin(), status.end(), 0x51);
    if (variant & 64) { x.n_elem = nullptr; x.end = nullptr; if (g() % 2) x.status = nullptr; }
    x.el_off = el_off.data(); x.total = total; x.el_stream = el_stream.data(); x.el_rec = el_rec.data(); x.el_kind = el_kind.data();
    TOTAL = total;
    launch<true>(x);
    results("fill");
    // every slot: the LAST entry whose room holds it wrote it iff it is one of that entry's elements (rooms of a consistent el_off are
    // disjoint; where el_off runs backwards rooms overlap and a slot may have several writers: then only "some writer's value")
    std::vector<uint8_t> want_written(total, 0);
    for (uint64_t j = 0; j < m; j++) {
        const uint64_t a = el_off[j], b = j + 1 < m ? el_off[j + 1] : total;
        for (uint64_t t = 0; t < ref[j].els.size() && a + t < b && a + t < total; t++) if (want_written[a + t] < 100) want_written[a + t]++;
    }
    for (uint64_t j = 0; j < m; j++) {
        const uint64_t a = el_off[j], b = j + 1 < m ? el_off[j + 1] : total;
        for (uint64_t t = 0; t < ref[j].els.size() && a + t < b && a + t < total; t++) {
            const uint64_t at = a + t;
            n_elements++;
            if (!w_stream[at] || !w_rec[at] || !w_kind[at]) die("an element's slot was not written");
            if (want_written[at] == 1 && (el_stream[at] != sel_stream[j] || el_rec[at] != ref[j].els[t].rec || el_kind[at] != ref[j].els[t].kind)) {
                printf("entry %llu element %llu: rec %llu kind %u, want rec %llu kind %u\n", (unsigned long long)j, (unsigned long long)t,
                       (unsigned long long)el_rec[at], el_kind[at], (unsigned long long)ref[j].els[t].rec, ref[j].els[t].kind);
                die("an element differs");
            }
        }
        n_entries++;
        if (ref[j].status == 0 && ref[j].els.empty()) n_empty++;
    }
    for (uint64_t at = 0; at < total; at++) {
        // (a long entry's first elements are stored by its lane and again by the wave: at most twice per writer)
        if (w_stream[at] > 2 * want_written[at] || w_rec[at] != w_stream[at] || w_kind[at] != w_stream[at]) die("a slot that holds no element was written");
        if (!want_written[at] && (el_stream[at] != 0x51515151u || el_rec[at] != 0x5151515151515151ull || el_kind[at] != 0x51)) die("a slot that holds no element changed");
    }
    for (uint64_t t = total; t < total + 4; t++)
        if (el_stream[t] != 0x51515151u || el_rec[t] != 0x5151515151515151ull || el_kind[t] != 0x51) die("canary behind total");
    n_batches++;
}

static void run_all(const std::vector<Bytes> &streams, std::mt19937 &g) {
    for (uint32_t v : {0u, 1u, 2u, 4u, 8u, 16u, 32u, 64u, 16u | 32u, 1u | 2u | 4u | 8u, 127u}) run(streams, v, g);
}

static Bytes B(const std::string &s) { return Bytes(s.begin(), s.end()); }

// `lead` boundaries in front, then an array whose closer stands `dist` boundaries behind its opener, elements of the given style
static std::string array_with(uint64_t dist, std::mt19937 &g, int style) {
    std::string s = "[";
    uint64_t have = 0; // boundaries behind the opener so far
    while (have + 1 < dist) {
        const uint64_t left = dist - 1 - have;
        const uint32_t pick = style == 0 ? 0 : g() % 6;
        if (pick == 1 && left >= 4) { s += "[1,2]"; have += 3; }                  // [ , ]
        else if (pick == 2 && left >= 5) { s += "{\"k\":[]}"; have += 5; }         // { : [ ] }
        else if (pick == 3 && left >= 3) { s += "\"a],[b\\\"\""; }
        else if (pick == 4) s += " 1.5e3 ";
        else s += std::to_string(g() % 100);
        if (have + 1 < dist) { s += ","; have++; }
    }
    return s + "]";
}

static Bytes line_with(uint64_t lead, const std::string &arr, const std::string &tail) {
    std::string s;
    for (uint64_t t = 0; t < lead; t++) s += ",";
    return B(s + arr + tail);
}

static Bytes random_jsonl(std::mt19937 &g, uint32_t n_lines) {
    std::string s;
    const char *vals[] = {"1", "\"a,b:{c}\"", "{\"text\":1,\"id\":[2,{\"k\":3}]}", "[1,2,{\"id\":7}]", "null", "\"\\\\\"", "\"q\\\"]\"", " 12 ", "-3.5e2", "[]", "[ ]", "[[],[[]]]", "", ":"};
    for (uint32_t r = 0; r < n_lines; r++) {
        std::string line = "{\"arr\":[";
        const uint32_t ne = g() % 4 ? g() % 9 : g() % 200;
        for (uint32_t e = 0; e < ne; e++) { if (e) line += g() % 3 ? "," : " , "; line += vals[g() % 14]; }
        line += "],\"x\":[1]}";
        const uint32_t kind = g() % 12;
        if (kind == 0) line = line.substr(0, g() % (line.size() + 1));
        else if (kind == 1) { const size_t at = line.find(']', g() % line.size()); if (at != std::string::npos) line[at] = '}'; }
        else if (kind == 2) { const size_t at = line.find(']', g() % line.size()); if (at != std::string::npos) line.erase(at, 1); }
        else if (kind == 3) line.insert(g() % line.size(), "\n");
        s += line;
        if (r + 1 < n_lines || g() % 2) s += "\n";
    }
    return B(s);
}

int main() {
    std::mt19937 g(2024);
    run_all({B("{\"a\":[]}"), B("{\"a\":[ ]}"), B("{\"a\":[1,]}"), B("{\"a\":[1:2]}"), B("{\"a\":[1}"), B("{\"a\":[1,2\n"), B("{\"a\":[1,[2"),
             B("{\"a\":[[1,2],{\"b\":[3]},4]}"), B("{\"a\":[\"],[\",2]}"), B("{\"a\":[,]}"), B("{\"a\":{}}"), B("{\"a\":[1]}"),
             B("{\"a\":[" + std::string(64, ' ') + "]}"), B("{\"a\":[" + std::string(65, ' ') + "]}"), B("{\"a\":[" + std::string(63, ' ') + "\t]}"),
             B(""), B("["), B("[]"), B("]"), B("[\n"), B("[}")}, g);
    const uint64_t L = BRX_EL_LONG, R = BRX_EL_ROW;
    std::vector<uint64_t> dists;
    for (uint64_t d = 1; d <= 40; d++) dists.push_back(d);
    for (uint64_t d : {L - 1, L, L + 1, L + 2, R - 1, R, R + 1, R + 2, R + L, 2 * R - 1, 2 * R, 2 * R + 1, 2 * R + 3, 3 * R + 17}) dists.push_back(d);
    for (int style = 0; style < 2; style++)
        for (uint64_t lead : {0u, 1u, 5u, 15u}) {
            std::vector<Bytes> streams;
            for (uint64_t d : dists) {
                streams.push_back(line_with(lead + d % 3, array_with(d, g, style), d % 2 ? "}\n" : ""));
                if (d > 2) { // the same array cut by a line feed, by the stream's end, closed by '}'
                    std::string a = array_with(d, g, style);
                    streams.push_back(line_with(lead, a.substr(0, a.size() - 1), "\n[1]"));
                    streams.push_back(line_with(lead, a.substr(0, a.size() - 1), ""));
                    streams.push_back(line_with(lead, a.substr(0, a.size() - 1) + "}", ",1]"));
                }
            }
            run_all(streams, g);
        }
    { // nested elements whose closers stand in a later lane and a later row; rows of commas only; deep nesting
        std::vector<Bytes> streams;
        std::string deep;
        for (int t = 0; t < 1500; t++) deep += "[";
        deep += "1";
        for (int t = 0; t < 1500; t++) deep += "]";
        streams.push_back(B("[1," + deep + ",2," + deep + "]"));
        streams.push_back(B("[" + deep.substr(0, 2800) + "\n"));
        streams.push_back(B("[" + std::string(3000, ',') + "]"));
        streams.push_back(B("[[" + std::string(2500, ',') + "]," + std::string(1100, ',') + "{" + std::string(1030, ',') + "}]"));
        streams.push_back(B("[1,[" + std::string(40, ',') + "],2,{\"a\":[" + std::string(1000, ',') + "]},3" + std::string(1024, ',') + "]"));
        for (uint32_t at : {0u, 15u, 16u, 1007u, 1008u, 1023u, 1024u, 1025u, 2047u, 2048u}) { // the stop at a given boundary behind the opener
            streams.push_back(B("[" + std::string(at, ',') + "]"));
            streams.push_back(B("[" + std::string(at, ',') + "\n]"));
            streams.push_back(B("[" + std::string(at, ',')));
            streams.push_back(B("[" + std::string(at, ',') + "}"));
            streams.push_back(B("[" + std::string(at, ':') + "]"));
        }
        run_all(streams, g);
    }
    for (uint32_t it = 0; it < 40; it++) {
        std::vector<Bytes> streams;
        const uint32_t n = 1 + g() % 10;
        for (uint32_t i = 0; i < n; i++) streams.push_back(random_jsonl(g, g() % 6 ? g() % 12 : g() % 60));
        run_all(streams, g);
    }
    if (n_long < 1000 || n_rows < n_long || n_pending_rows == 0 || n_empty < 100 || n_elements < 100000) die("the batches did not reach what they are for");
    printf("OK: %llu batches, %llu entries (%llu of them the wave's, in %llu rows of %u boundaries, %llu rows that left their pending element "
           "pending; BRX_EL_LONG %u), %llu elements stored, %llu empty arrays, %llu wide and %llu byte loads of what, %llu arena loads\n",
           (unsigned long long)n_batches, (unsigned long long)n_entries, (unsigned long long)n_long, (unsigned long long)n_rows, BRX_EL_ROW,
           (unsigned long long)n_pending_rows, BRX_EL_LONG, (unsigned long long)n_elements, (unsigned long long)n_empty,
           (unsigned long long)n_wide, (unsigned long long)n_byte, (unsigned long long)n_arena);
    return 0;
}
