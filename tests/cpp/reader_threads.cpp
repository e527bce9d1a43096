// Many pulled readers of one context through host/decompressor.hpp (brotli::Decompressor<R>, the reference's Decompressor::new(r: R)
// over a reader, src/lib.rs:398-410), each over a source that hands out its compressed bytes in pieces of random size.
//   threads: T threads start together behind a barrier, each reads its own Decompressor (8 .. 16 MiB of output) in 64 KiB reads.
//   advance: one thread moves all T Decompressors on with brotli::advance and reads what Decompressor::ready() says is there.
// With BRX_OPTION_READER_BATCH = 1 their slices go out together as reader rounds (brx.h); with 0 every slice is a launch of its own.
// The streams are made on the GPU from text (brx_generate_batch, adaptive) with every third byte random, so that each one's input
// does not end within the Decompressor's first 4 MiB and it is PULLED, not pooled (checked).  Prints the rate and the slice launches /
// slices of the run (brx_last_timing 16 / 17); exits 1 on any wrong byte.
// usage: reader_threads <threads|advance> <reader_batch 0|1> <streams> <min MiB> <max MiB> <text file>...
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

#include "../../brotli-rs_amd/host/decompressor.hpp"

static std::vector<uint8_t> slurp(const char *p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct Pieces { // an R: the compressed bytes, handed out in pieces of random size (1 .. len)
    const uint8_t *p;
    size_t n, at;
    std::mt19937 rng;
    size_t read(uint8_t *buf, size_t len) {
        const size_t k = std::min<size_t>(n - at, 1 + rng() % std::max<size_t>(1, std::min<size_t>(len, 3u << 20)));
        memcpy(buf, p + at, k);
        at += k;
        return k;
    }
};
using Dec = brotli::Decompressor<Pieces>;

int main(int argc, char **argv) {
    if (argc < 7) return 2;
    const bool threads = strcmp(argv[1], "threads") == 0;
    const int batch = atoi(argv[2]), T = atoi(argv[3]);
    const size_t lo = (size_t)atoi(argv[4]) << 20, hi = (size_t)atoi(argv[5]) << 20;
    std::vector<uint8_t> corpus;
    for (int i = 6; i < argc; i++) {
        std::vector<uint8_t> t = slurp(argv[i]);
        corpus.insert(corpus.end(), t.begin(), t.end());
    }
    if (corpus.size() < 4096 || T < 1) return 2;
    brx_ctx *ctx = brotli::default_context();
    if (brx_ctx_set_option(ctx, BRX_OPTION_READER_BATCH, batch) != BRX_SUCCESS) {
        fprintf(stderr, "brx_ctx_set_option: %s\n", brx_last_error());
        return 1;
    }
    // T inputs: the corpus from a different offset each, every third byte random (no two streams alike, > 4 MiB compressed)
    std::mt19937 rng(7);
    std::vector<uint64_t> src_off(T + 1, 0), out_off(T + 1, 0);
    for (int t = 0; t < T; t++) src_off[t + 1] = src_off[t] + lo + (hi > lo ? rng() % (hi - lo) : 0);
    std::vector<uint8_t> src(src_off[T]);
    for (int t = 0; t < T; t++) {
        const size_t start = rng() % corpus.size();
        for (uint64_t i = src_off[t]; i < src_off[t + 1]; i++) src[i] = corpus[(start + i - src_off[t]) % corpus.size()];
        for (uint64_t i = src_off[t]; i < src_off[t + 1]; i += 3) src[i] = (uint8_t)rng();
    }
    const uint32_t mb = 1u << 20;
    for (int t = 0; t < T; t++) {
        const uint64_t len = src_off[t + 1] - src_off[t];
        out_off[t + 1] = out_off[t] + len + len / 8 + 2048 * (len / mb + 2);
    }
    std::vector<uint8_t> comp(out_off[T]);
    std::vector<uint64_t> comp_len(T);
    std::vector<int32_t> gst(T);
    brx_opts go = {BRX_MEM_HOST | BRX_GEN_ADAPTIVE, 0, nullptr};
    if (brx_generate_batch(ctx, src.data(), src_off.data(), T, comp.data(), out_off.data(), comp_len.data(), gst.data(), mb, &go) != BRX_SUCCESS) {
        fprintf(stderr, "brx_generate_batch: %s\n", brx_last_error());
        return 1;
    }
    for (int t = 0; t < T; t++)
        if (gst[t] != 0 || comp_len[t] <= Dec::POOLED_LIMIT) {
            fprintf(stderr, "stream %d: status %d, %llu compressed bytes (a pulled Decompressor needs more than %zu)\n", t, gst[t],
                    (unsigned long long)comp_len[t], Dec::POOLED_LIMIT);
            return 1;
        }
    std::vector<std::unique_ptr<Dec>> ds;
    for (int t = 0; t < T; t++) ds.emplace_back(new Dec(Pieces{comp.data() + out_off[t], (size_t)comp_len[t], 0, std::mt19937(100 + t)}));
    const double l0 = brx_last_timing(ctx, 16), s0 = brx_last_timing(ctx, 17);
    std::atomic<int> bad{0};
    const auto t0 = std::chrono::steady_clock::now();
    // one stream's output against its input, piece by piece
    auto check = [&](int t, size_t at, const uint8_t *p, size_t n) {
        return at + n <= src_off[t + 1] - src_off[t] && memcmp(p, src.data() + src_off[t] + at, n) == 0;
    };
    if (threads) {
        std::mutex m;
        std::condition_variable cv;
        int arrived = 0;
        std::vector<std::thread> th;
        for (int t = 0; t < T; t++)
            th.emplace_back([&, t] {
                {
                    std::unique_lock<std::mutex> l(m);
                    if (++arrived == T) cv.notify_all();
                    cv.wait(l, [&] { return arrived == T; });
                }
                std::vector<uint8_t> buf(1 << 16);
                size_t at = 0;
                try {
                    for (size_t n; (n = ds[t]->read(buf.data(), buf.size())) > 0; at += n)
                        if (!check(t, at, buf.data(), n)) { bad++; return; }
                } catch (const std::exception &e) {
                    fprintf(stderr, "stream %d: %s\n", t, e.what());
                    bad++;
                    return;
                }
                if (at != src_off[t + 1] - src_off[t]) bad++;
            });
        for (auto &x : th) x.join();
    } else {
        std::vector<Dec *> all;
        for (auto &d : ds) all.push_back(d.get());
        std::vector<size_t> at(T, 0);
        std::vector<uint8_t> buf(4u << 20);
        try {
            while (brotli::advance(all) > 0) {
                for (int t = 0; t < T; t++)
                    for (size_t r; (r = ds[t]->ready()) > 0;) {
                        const size_t n = ds[t]->read(buf.data(), std::min(r, buf.size()));
                        if (n == 0 || !check(t, at[t], buf.data(), n)) { bad++; break; }
                        at[t] += n;
                    }
                if (bad) break;
            }
            for (int t = 0; t < T; t++) // (every stream has ended: the reads that follow decode nothing)
                if (ds[t]->read(buf.data(), buf.size()) != 0 || at[t] != src_off[t + 1] - src_off[t] || ds[t]->handle() == nullptr) bad++;
        } catch (const std::exception &e) {
            fprintf(stderr, "advance: %s\n", e.what());
            bad++;
        }
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const double launches = brx_last_timing(ctx, 16) - l0, slices = brx_last_timing(ctx, 17) - s0;
    printf("%s, reader_batch %d, %d streams: %.1f MiB in %.1f ms = %.0f MB/s; launches %.0f slices %.0f (%.2f per launch); %d wrong\n",
           threads ? "threads" : "advance", batch, T, (double)src.size() / (1 << 20), ms, (double)src.size() / ms / 1e3, launches, slices,
           launches > 0 ? slices / launches : 0.0, bad.load());
    ds.clear(); // (the Decompressors free their streams; the default context lives to the end of the process)
    return bad.load() ? 1 : 0;
}
