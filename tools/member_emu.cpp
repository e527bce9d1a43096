// member_emu.cpp -- brx_member_batch on a CPU, lane by lane: the five steps of brx_member.hip (plan, sum, compose, emit, finish) around
// the REAL text of csrc/brx_member.h, with the wave's scan of the lanes' summaries and the workgroup's scan of the tiles' summaries as
// serial loops over the same join functions, held to a boundary-serial restatement of THE RULE of include/brx.h that shares nothing
// with the header.  Batches: the contract's check stream, streams with 0, 1, R - 1, R, R + 1, T - 1, T, T + 1 and 2T + 3 boundaries,
// 40 streams with 0 .. 39 boundaries, 3000 streams (more streams and tiles than a workgroup has threads), lines that span tiles, random JSON Lines with broken lines, blanks and long keys, each batch
// also with m below the number of lines and with n_pos below the sum of the counts.
// The run fails on: a load of `what` outside the stream's boundaries that count or at / behind n_pos; an arena load outside the
// stream; a store outside n_names * m (outside m for the flags); a slot of a line that was not written; a result that differs.
// No GPU.  Build and run: g++ -O2 -std=c++17 -I brotli-rs_amd/csrc tools/member_emu.cpp -o member_emu && ./member_emu
// (tests/test_member_abi.py does).  It proves the arithmetic, not the kernel's own text: that is tests/test_gpu_member.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include <string>
#include <vector>
#include "brx_member.h"
typedef std::vector<uint8_t> Bytes;

static void die(const char *what) { printf("FAIL: %s\n", what); exit(1); }

// what the policy checks against: set per batch, the stream per work item
static const uint8_t *S_LO, *S_HI;          // the stream in hand
static const uint8_t *W_BASE, *W_LO, *W_HI; // `what`, and the part of it that the stream in hand may load
static uint64_t N_POS;
static uint64_t *REC; static uint32_t *STREAM; static uint8_t *KIND, *FLAGS;
static uint64_t SLOTS, M;
static std::vector<uint8_t> w_rec, w_kind, w_stream, w_flags;
static uint64_t n_wide, n_byte, n_max, n_or;

struct EmuMem {
    uint8_t ld8(const uint8_t *p) { if (p < S_LO || p >= S_HI) die("byte load outside the stream"); return *p; }
    BrxTake128 ld128(const uint8_t *p) {
        if (p < S_LO || p + 16 > S_HI) die("16-byte load outside the stream");
        BrxTake128 v; memcpy(&v.lo, p, 8); memcpy(&v.hi, p + 8, 8); return v;
    }
    void chk_w(const uint8_t *p, uint32_t n) {
        if (p < W_LO || p + n > W_HI) die("load of what outside the boundaries of the stream that count");
        if ((uint64_t)(p - W_BASE) + n > N_POS) die("load of what at or behind n_pos");
    }
    uint8_t ldw8(const uint8_t *p) { chk_w(p, 1); n_byte++; return *p; }
    BrxTake128 ldw128(const uint8_t *p) { chk_w(p, 16); n_wide++; BrxTake128 v; memcpy(&v.lo, p, 8); memcpy(&v.hi, p + 8, 8); return v; }
    void max64(uint64_t *p, uint64_t v) { if (p < REC || p >= REC + SLOTS) die("max64 outside n_names * m"); n_max++; if (*p < v) *p = v; }
    void or32(uint32_t *p, uint32_t v) { if (p < STREAM || p >= STREAM + M) die("or32 outside m"); n_or++; *p |= v; }
    uint64_t get64(const uint64_t *p) { if (p < REC || p >= REC + SLOTS) die("get64 outside n_names * m"); return *p; }
    uint32_t get32(const uint32_t *p) { if (p < STREAM || p >= STREAM + M) die("get32 outside m"); return *p; }
    void st64(uint64_t *p, uint64_t v) { if (p < REC || p >= REC + SLOTS) die("sel_rec store outside n_names * m"); w_rec[p - REC] = 1; *p = v; }
    void st32(uint32_t *p, uint32_t v) { if (p < STREAM || p >= STREAM + SLOTS) die("sel_stream store outside n_names * m"); w_stream[p - STREAM] = 1; *p = v; }
    void st8(uint8_t *p, uint8_t v) {
        if (p >= KIND && p < KIND + SLOTS) w_kind[p - KIND] = 1;
        else if (p >= FLAGS && p < FLAGS + M) w_flags[p - FLAGS] = 1;
        else die("byte store outside kind's n_names * m and line_flags' m");
        *p = v;
    }
};

// ---- the definition, serially, with nothing shared with brx_member.h ------------------------------------------------------------
struct RefLine { uint64_t rec[8]; uint8_t kind[8]; uint8_t flags; };
static void ref_stream(const Bytes &s, const uint64_t *pos, const uint8_t *what, uint64_t cnt, const std::vector<std::string> &names,
                       std::vector<RefLine> &out) {
    RefLine cur;
    auto fresh = [&]() { for (int q = 0; q < 8; q++) { cur.rec[q] = ~(uint64_t)0; cur.kind[q] = 0; } cur.flags = 0; };
    fresh();
    long d = 0;
    const uint64_t l = s.size();
    for (uint64_t k = 0; k < cnt; k++) {
        const uint8_t c = what[k];
        if (c == '\n') { if (d) cur.flags |= 4; out.push_back(cur); fresh(); d = 0; continue; }
        if (c == '{' || c == '[') d++;
        else if (c == '}' || c == ']') { if (--d < 0) cur.flags |= 4; }
        else if (c == ':' && d == 1) {
            uint64_t a = 0, b = pos[k] < l ? pos[k] : l;
            if (k) { a = (pos[k - 1] < l ? pos[k - 1] : l) + 1; if (a > l) a = l; }
            if (b < a) b = a;
            if (b - a > 64) { cur.flags |= 1; continue; }
            std::string t(s.begin() + a, s.begin() + b);
            if (t.find('\\') != std::string::npos) cur.flags |= 2;
            while (!t.empty() && (t[0] == ' ' || t[0] == '\t' || t[0] == '\r')) t.erase(0, 1);
            while (!t.empty() && (t.back() == ' ' || t.back() == '\t' || t.back() == '\r')) t.pop_back();
            for (size_t q = 0; q < names.size(); q++)
                if (t == "\"" + names[q] + "\"") {
                    const uint8_t w = k + 1 < cnt ? what[k + 1] : 0;
                    cur.rec[q] = k + 1;
                    cur.kind[q] = (w == ',' || w == '}') ? 1 : w == '{' ? 2 : w == '[' ? 3 : 4;
                }
        }
    }
    if (d) cur.flags |= 4;
    out.push_back(cur);
}

// pos and what of brx_index_set_batch for one stream, restated
static void ref_index(const Bytes &s, std::vector<uint64_t> &pos, Bytes &what) {
    bool esc = false; uint64_t quotes = 0;
    for (size_t j = 0; j < s.size(); j++) {
        const uint8_t c = s[j];
        if (esc) { esc = false; continue; }
        if (c == '\\') esc = true;
        else if (c == '"') quotes++;
        else if (strchr("{}[]:,\n", c) && c && !(quotes & 1)) { pos.push_back(j); what.push_back(c); }
    }
}

// ---- one batch through the five steps -------------------------------------------------------------------------------------------
static uint64_t n_batches, n_lines, n_members, n_tiles_seen, n_multi, n_sliced;

static void run(const std::vector<Bytes> &streams, const std::vector<std::string> &names, int cut_m, int cut_pos, bool with_flags, bool with_lines) {
    const uint32_t n = (uint32_t)streams.size();
    Bytes arena(7, 0xEE), what;
    std::vector<uint64_t> out_off(n), len(n), count(n), pos_off(n), pos;
    for (uint32_t i = 0; i < n; i++) {
        out_off[i] = arena.size(); len[i] = streams[i].size();
        arena.insert(arena.end(), streams[i].begin(), streams[i].end());
        arena.insert(arena.end(), i % 5, 0x3A); // slack between streams, of colons
        pos_off[i] = pos.size();
        ref_index(streams[i], pos, what);
        count[i] = pos.size() - pos_off[i];
    }
    uint64_t n_pos = pos.size();
    if (cut_pos && n_pos) n_pos -= (n_pos < 5 ? 1 : n_pos / 5);
    // the reference, under the cut
    std::vector<std::vector<RefLine>> ref(n);
    std::vector<uint64_t> line_off(n), lines_want(n);
    uint64_t total_lines = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint64_t c = count[i];
        if (pos_off[i] >= n_pos) c = 0; else if (pos_off[i] + c > n_pos) c = n_pos - pos_off[i];
        ref_stream(streams[i], pos.data() + pos_off[i], what.data() + pos_off[i], c, names, ref[i]);
        line_off[i] = total_lines; lines_want[i] = ref[i].size(); total_lines += ref[i].size();
    }
    const uint64_t m = cut_m ? total_lines - (total_lines + 2) / 3 : total_lines;
    BrxMbNames nm; memset(&nm, 0, sizeof nm); nm.n = (uint32_t)names.size();
    for (uint32_t q = 0; q < nm.n; q++) { nm.len[q] = (uint32_t)names[q].size(); memcpy(nm.w[q], names[q].data(), names[q].size()); }
    const uint64_t slots = nm.n * m;
    std::vector<uint64_t> sel_rec(slots + 8, 0x5151515151515151ull), lines(n + 1, 0x77), slines(n);
    std::vector<uint32_t> sel_stream(slots + 8, 0x51515151u);
    Bytes kind(slots + 8, 0x51), line_flags(m + 8, 0x51);
    BrxMbArgs x; memset(&x, 0, sizeof x);
    x.a.out = arena.data(); x.a.out_off = out_off.data(); x.a.len = len.data(); x.a.n = n; x.a.span = arena.size();
    x.a.count = count.data(); x.a.pos_off = pos_off.data(); x.a.pos = pos.data(); x.a.n_pos = n_pos; x.a.delim_len = 1; x.a.flags = BRX_TAKE_F_NO_DELIM;
    x.a.m = m; x.what = what.data(); x.lines = with_lines ? lines.data() : nullptr; x.line_off = line_off.data(); x.m = m;
    x.sel_stream = sel_stream.data(); x.sel_rec = sel_rec.data(); x.kind = kind.data(); x.line_flags = with_flags ? line_flags.data() : nullptr;
    x.max_tiles = brx_mb_max_tiles(n, n_pos);
    std::vector<uint64_t> pre(n + 1);
    std::vector<BrxMbSum> sum(x.max_tiles);
    std::vector<BrxMbSeg> in(x.max_tiles);
    x.pre = pre.data(); x.slines = slines.data(); x.sum = sum.data(); x.in = in.data();
    W_BASE = what.data(); N_POS = n_pos; REC = sel_rec.data(); STREAM = sel_stream.data(); KIND = kind.data(); FLAGS = line_flags.data();
    SLOTS = slots; M = m;
    w_rec.assign(slots, 0); w_kind.assign(slots, 0); w_stream.assign(slots, 0); w_flags.assign(m, 0);
    EmuMem mem;
    // the clears
    for (uint64_t t = 0; t < slots; t++) sel_rec[t] = 0;
    for (uint64_t t = 0; t < m; t++) sel_stream[t] = 0;
    // plan
    // (the body of brx_member_plan_kernel: every thread sums its slice of the streams, the sums are scanned, every thread writes its slice)
    const uint32_t threads = n_batches % 3 == 0 ? 1024u : n_batches % 3 == 1 ? 7u : 3u; // (the kernels have 1024: fewer here so that small batches have slices of several elements too)
    uint64_t run_t = 0;
    {
        const uint64_t per_s = ((uint64_t)n + threads - 1) / threads;
        std::vector<uint64_t> psum(threads);
        for (uint32_t th = 0; th < threads; th++) {
            const uint64_t i0 = per_s * th < n ? per_s * th : n, i1 = i0 + per_s < n ? i0 + per_s : n;
            uint64_t sm = 0;
            for (uint64_t i = i0; i < i1; i++) sm += brx_mb_tiles(brx_mb_count(x.a, i));
            psum[th] = sm + (th ? psum[th - 1] : 0);
        }
        for (uint32_t th = 0; th < threads; th++) {
            const uint64_t i0 = per_s * th < n ? per_s * th : n, i1 = i0 + per_s < n ? i0 + per_s : n;
            uint64_t r = th ? psum[th - 1] : 0;
            for (uint64_t i = i0; i < i1; i++) { pre[i] = r < x.max_tiles ? r : x.max_tiles; r += brx_mb_tiles(brx_mb_count(x.a, i)); }
        }
        run_t = psum[threads - 1];
    }
    pre[n] = run_t < x.max_tiles ? run_t : x.max_tiles;
    if (run_t > x.max_tiles) die("more tiles than the bound");
    n_tiles_seen += run_t;
    // sum (EMIT = false) and emit (EMIT = true): the body of brx_member_kernel, its 64 lanes in turn
    for (int emit = 0; emit < 2; emit++) {
        for (uint64_t t = 0; t < pre[n]; t++) {
            const uint32_t i = brx_mb_tile_stream(pre.data(), n, t);
            const uint64_t c = brx_mb_count(x.a, i), base = pos_off[i], kt = (t - pre[i]) * BRX_MB_TILE;
            S_LO = arena.data() + out_off[i]; S_HI = S_LO + len[i];
            W_LO = what.data() + base; W_HI = W_LO + c;
            BrxMbSum carry = {0, 0, 0};
            for (uint32_t row = 0; row < BRX_MB_TILE / BRX_MB_ROW && kt + row * BRX_MB_ROW < c; row++) {
                BrxMbMasks k[64]; BrxMbSum incl[64]; uint32_t nv[64];
                for (uint32_t l = 0; l < 64; l++) {
                    const uint64_t k0 = kt + row * BRX_MB_ROW + l * BRX_MB_UNIT;
                    nv[l] = brx_mb_valid(c, k0);
                    k[l] = brx_mb_masks(brx_mb_unit(mem, x.what, base + k0, nv[l]));
                    const BrxMbSum s = brx_mb_unit_sum(k[l]);
                    incl[l] = l ? brx_mb_join(incl[l - 1], s) : s; // (the scan)
                }
                if (emit) for (uint32_t l = 0; l < 64; l++) {
                    BrxMbSum ex = {0, 0, 0};
                    if (l) ex = incl[l - 1];
                    const BrxMbSum st = brx_mb_join(carry, ex);
                    brx_mb_walk(mem, x, nm, i, c, kt + row * BRX_MB_ROW + l * BRX_MB_UNIT, nv[l], k[l], in[t].L + st.nl, st.rd ? st.d : in[t].d + st.d);
                }
                carry = brx_mb_join(carry, incl[63]);
            }
            if (!emit) sum[t] = carry;
        }
        if (emit) break;
        // compose: the body of brx_member_compose_kernel, its threads in turn: every thread joins its slice of the tiles, the slices'
        // sums are scanned (the LDS scan, here a serial loop over the same join), every thread finishes its slice with its prefix
        const uint64_t nt = pre[n], per = (nt + threads - 1) / threads;
        std::vector<BrxMbSeg> part(threads);
        for (uint32_t th = 0; th < threads; th++) {
            const uint64_t t0 = per * th < nt ? per * th : nt, t1 = t0 + per < nt ? t0 + per : nt;
            BrxMbSeg acc = {0, 0, 0};
            if (t0 < t1) {
                uint32_t si = brx_mb_tile_stream(pre.data(), n, t0);
                for (uint64_t t = t0; t < t1; t++) {
                    while (t >= pre[si + 1]) si++;
                    if (t == pre[si]) acc = brx_mb_seg_join(acc, brx_mb_seg_start());
                    in[t] = acc;
                    acc = brx_mb_seg_join(acc, brx_mb_seg_of(sum[t]));
                }
                if (t1 - t0 > 1) n_sliced++;
            }
            part[th] = th ? brx_mb_seg_join(part[th - 1], acc) : acc; // (the scan)
        }
        for (uint32_t th = 0; th < threads; th++) {
            const uint64_t t0 = per * th < nt ? per * th : nt, t1 = t0 + per < nt ? t0 + per : nt;
            BrxMbSeg pfx = {0, 0, 0};
            if (th) pfx = part[th - 1];
            if (t0 >= t1) continue;
            uint32_t si = brx_mb_tile_stream(pre.data(), n, t0);
            for (uint64_t t = t0; t < t1; t++) {
                while (t >= pre[si + 1]) si++;
                in[t] = brx_mb_seg_join(pfx, in[t]);
                if (t + 1 == pre[si + 1]) { slines[si] = in[t].L + sum[t].nl + 1; if (x.lines) x.lines[si] = slines[si]; }
            }
        }
        for (uint32_t i = 0; i < n; i++) if (pre[i] == pre[i + 1]) { slines[i] = 1; if (x.lines) x.lines[i] = 1; }
    }
    // finish
    W_LO = what.data(); W_HI = what.data() + n_pos;
    for (uint64_t j = 0; j < m; j++) brx_mb_finish(mem, x, nm.n, j);
    // compare
    for (uint32_t i = 0; i < n; i++) {
        if (slines[i] != lines_want[i] || (with_lines && lines[i] != lines_want[i])) die("lines differ");
        if (ref[i].size() > 1) n_multi++;
        for (uint64_t r = 0; r < ref[i].size(); r++) {
            const uint64_t j = line_off[i] + r;
            if (j >= m) continue;
            n_lines++;
            if (with_flags && (!w_flags[j] || line_flags[j] != ref[i][r].flags)) die("line_flags differ or were not written");
            for (uint32_t q = 0; q < nm.n; q++) {
                const uint64_t at = q * m + j;
                if (!w_rec[at] || !w_kind[at] || !w_stream[at]) die("a slot of a line was not written");
                if (sel_rec[at] != ref[i][r].rec[q] || kind[at] != ref[i][r].kind[q] || sel_stream[at] != i) {
                    printf("stream %u line %llu name %u: rec %llu kind %u, want rec %llu kind %u\n", i, (unsigned long long)r, q,
                           (unsigned long long)sel_rec[at], kind[at], (unsigned long long)ref[i][r].rec[q], ref[i][r].kind[q]);
                    die("a member differs");
                }
                if (kind[at]) n_members++;
            }
        }
    }
    if (with_lines && lines[n] != 0x77) die("lines written behind n");
    for (uint64_t t = slots; t < slots + 8; t++)
        if (sel_rec[t] != 0x5151515151515151ull || sel_stream[t] != 0x51515151u || kind[t] != 0x51) die("canary behind the results");
    for (uint64_t t = with_flags ? m : 0; t < m + 8; t++) if (line_flags[t] != 0x51) die("canary in line_flags");
    n_batches++;
}

static void run_all(const std::vector<Bytes> &streams, const std::vector<std::string> &names) {
    for (int v = 0; v < 8; v++) run(streams, names, v & 1, (v >> 1) & 1, !(v & 4), !(v & 1));
}

static Bytes B(const std::string &s) { return Bytes(s.begin(), s.end()); }

// a stream of exactly `want` boundaries: objects {"k":1,...} in lines, then commas
static Bytes with_boundaries(uint64_t want, std::mt19937 &g, uint32_t per_line) {
    std::string s;
    uint64_t have = 0;
    const char *keys[] = {"id", "text", "x", "a_rather_long_key_of_32_bytes_xx", "textual"};
    while (have < want) {
        const uint64_t left = want - have;
        if (left < 4) { s += ","; have++; continue; }
        uint64_t mem = (left - 2) / 2;
        if (mem > per_line) mem = 1 + g() % per_line;
        s += "{";
        for (uint64_t e = 0; e < mem; e++) { s += (e ? ",\"" : "\""); s += keys[g() % 5]; s += "\":"; s += std::to_string(g() % 1000); }
        s += "}\n";
        have += 2 * mem + 2; // { , ... : ... } \n : mem colons, mem - 1 commas, 3
    }
    return B(s);
}

static Bytes random_jsonl(std::mt19937 &g, uint32_t n_lines) {
    std::string s;
    const char *keys[] = {"id", "text", "tex", "textual", "user", "a_rather_long_key_of_32_bytes_xx", "k", "tags"};
    const char *vals[] = {"1", "\"a,b:{c}\"", "{\"text\":1,\"id\":[2,{\"k\":3}]}", "[1,2,{\"id\":7}]", "null", "\"\\\\\"", "\"q\\\"}\"", " 12 ", "-3.5e2", "[]"};
    const char *blanks[] = {"", "", " ", "\t", " \r", "                              ", "                               "};
    for (uint32_t r = 0; r < n_lines; r++) {
        const uint32_t kind = g() % 40;
        std::string line = "{";
        const uint32_t nk = g() % 6;
        for (uint32_t e = 0; e < nk; e++) {
            if (e) line += ",";
            line += blanks[g() % 7]; line += "\""; line += keys[g() % 8]; if (g() % 50 == 0) line += "\\u0041"; line += "\""; line += blanks[g() % 5];
            line += ":"; line += vals[g() % 10];
        }
        line += "}";
        if (kind == 0) line = line.substr(0, g() % (line.size() + 1));
        else if (kind == 1) line += "}";
        else if (kind == 2) line = "}" + line;
        else if (kind == 3) line = "[" + line + "]";
        else if (kind == 4) line = "";
        else if (kind == 5) line = "\"id\":1";
        s += line;
        if (r + 1 < n_lines || g() % 2) s += "\n";
    }
    return B(s);
}

int main() {
    std::mt19937 g(12345);
    const std::vector<std::string> four = {"a", "b", "c", "open"};
    run_all({B("{\"a\":\"x,\\\"y:}\",\"b\":[1,2]}\n{\"c\":\"\\\\\"}\n{\"open\":\"[\\")}, four);
    const std::vector<std::string> some = {"id", "text", "a_rather_long_key_of_32_bytes_xx"};
    const std::vector<std::string> eight = {"id", "text", "tex", "textual", "user", "a_rather_long_key_of_32_bytes_xx", "k", "tags"};
    const std::vector<std::string> one = {"text"};
    const uint64_t R = BRX_MB_ROW, T = BRX_MB_TILE;
    const uint64_t counts[] = {0, 1, R - 1, R, R + 1, T - 1, T, T + 1, 2 * T + 3};
    for (uint32_t per_line : {3u, 100u, 100000u}) { // short lines, lines across rows, one line across all tiles
        std::vector<Bytes> streams;
        for (uint64_t c : counts) streams.push_back(with_boundaries(c, g, per_line));
        run_all(streams, some);
        for (auto &s : streams) run_all({s}, one); // n = 1
    }
    {
        std::vector<Bytes> streams;
        for (uint64_t c = 0; c < 40; c++) streams.push_back(with_boundaries(c, g, 4));
        run_all(streams, eight);
    }
    { // more streams and more tiles than a workgroup has threads: slices of several elements with 1024 threads too
        std::vector<Bytes> streams;
        for (uint32_t i = 0; i < 3000; i++) streams.push_back(with_boundaries(i == 1500 ? 3 * T + 5 : g() % 24, g, 3));
        for (int v = 0; v < 3; v++) run(streams, some, 0, v == 2, true, true);
    }
    for (uint32_t it = 0; it < 60; it++) {
        std::vector<Bytes> streams;
        const uint32_t n = 1 + g() % 12;
        for (uint32_t i = 0; i < n; i++) streams.push_back(random_jsonl(g, g() % 8 ? g() % 40 : g() % 700));
        run_all(streams, it % 3 == 0 ? eight : it % 3 == 1 ? some : one);
    }
    if (!n_multi || n_members < 1000 || n_or == 0 || n_sliced < 1000) die("the batches did not reach what they are for");
    printf("OK: %llu batches, %llu lines, %llu members, %llu tiles of %u boundaries in rows of %u, %llu wide and %llu byte loads of what, "
           "%llu raises, %llu flag updates\n", (unsigned long long)n_batches, (unsigned long long)n_lines, (unsigned long long)n_members,
           (unsigned long long)n_tiles_seen, BRX_MB_TILE, BRX_MB_ROW, (unsigned long long)n_wide, (unsigned long long)n_byte,
           (unsigned long long)n_max, (unsigned long long)n_or);
    return 0;
}
