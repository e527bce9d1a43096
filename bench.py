#!/usr/bin/env python3
"""bench.py -- decompressed MB/s of the batched Brotli decode hot path on MI355X.

  python bench.py --gpus N --steps K --warmup W          (N > 1 without a launcher around it: starts the N ranks itself)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

--gpus N with fewer than N visible GPUs, or under a launcher whose WORLD_SIZE differs from N, exits non-zero without a line.

A "step" = one pass of the hot path (brx_decode_batch through the C ABI) over one batch of synthetic input
already resident in HBM.  Workload at every N: BASELINE.json configs[1], "4096 x data/alice29.txt.compressed"
PER GPU (weak scaling: independent streams shard across ranks with no data-path collective; the RCCL
scatter/gather of SURVEY 8e lives in brotli-rs_amd/shard.py and is never inside `value`).  Prints ONE JSON line on
rank 0.  A plain run does only what that line's headline needs: set up, warm up, time the K steps, write --dump-outputs,
check the last step's output (`bit_exact`) and print `value`, `ms_per_step` and `kernel_ms_per_rank`.

--full adds everything else the benchmark measures, after the timed region as before: `strong` (the same 4096-stream batch
split over the N GPUs) and the RCCL `gather` at N > 1; at rank 0 the CPU baselines, `roofline` (with in-run rocprofv3 PMC
passes and the single-stream chain floor), at N = 1 `copy_path` (the LZ77 copy path against the physical HBM roofline: far
copies and the two fills of configs 3 / 4), `configs` and `node_abi`, and the PCIe-inclusive host path.  The --no-* switches
thin a --full run.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GOLD = os.path.join(ROOT, "tests", "golden", "data")
STUB = os.environ.get("BRX_BENCH_STUB") == "1"  # CPU test of the launcher path only (tests/test_bench_launch.py)
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak

C5 = os.path.join(ROOT, "tests", "golden", "config5")
WORKLOADS = {
    # name: (fixtures, streams per GPU); stream i of a batch decodes fixture i mod K
    "alice29x4096": (["alice29.txt"], 4096),                       # BASELINE configs[1]: the headline
    "backward65536x4096": (["backward65536"], 4096),               # configs[2]
    "quickfox_repeatedx8192": (["quickfox_repeated"], 8192),       # configs[3], per-GPU share
    "compressed_repeatedx4096": (["compressed_repeated"], 4096),   # supplementary long-distance copy
    "config5_1MiBx1024": (["c5_0", "c5_1", "c5_2", "c5_3"], 1024), # configs[4], per-GPU share
    # the LZ77 back-reference on its own (north_star: ">= 40 % of HBM peak on the copy"): hand-assembled streams, 64 KiB of
    # raw bytes then non-overlapping copies from distance >= 64 KiB doubling the output to 1 MiB (tests/craft.py)
    "farcopy_1MiBx4096": (["farcopy_0", "farcopy_1", "farcopy_2", "farcopy_3"], 4096),
    # INCOMPRESSIBLE payloads: every encoder stores them as uncompressed meta-blocks (reference src/lib.rs:1701-1734) -- a memcpy from the
    # compressed input to the output: 256 KiB of random bytes in 64-KiB meta-blocks, hand-assembled (tests/craft.py raw_block)
    "raw_256KiBx4096": (["raw_0", "raw_1", "raw_2", "raw_3"], 4096),
    # the other Canterbury texts the reference holds (supplementary: bigger files, more trees per meta-block)
    "asyoulikx4096": (["asyoulik.txt"], 4096),
    "lcet10x4096": (["lcet10.txt"], 4096),
    "plrabn12x4096": (["plrabn12.txt"], 4096),
    "mapsdatazrhx4096": (["mapsdatazrh"], 4096),
    # 64 KiB of text at quality 11 (libbrotlienc fixtures, tests/golden/enc): 10 - 11 literal trees in one meta-block -- more than the
    # eight the register-resident literal loop holds, small enough for the regular instance (round 5: the tree cache)
    "text64k_q11x4096": (["enc:e042_text64k", "enc:e043_text64k", "enc:e051_text64k", "enc:e062_text64k"], 4096),
    # 40 KB of text at quality 0 .. 4 (what a server compressing on the fly emits): ONE literal tree, no contexts, literal-heavy
    "text40k_lowqx4096": (["enc:e000_text40k", "enc:e001_text40k", "enc:e002_text40k", "enc:e004_text40k"], 4096),
    # streams FLUSHED every KiB or so (an encoder behind a chatty protocol): a third of their time is meta-block headers
    "flush1k_textx4096": (["enc:e046_text64k"], 4096),
    "flush1k_mixedx4096": (["enc:e093_mixed"], 4096),
    # small streams (a launch of many short messages): 47 / 69 / 425 compressed bytes
    "quickfoxx16384": (["quickfox"], 16384),
    "ukkonooax16384": (["ukkonooa"], 16384),
    "monkeyx16384": (["monkey"], 16384),
    # BASELINE configs[4]'s shape WITHOUT a committed fixture: 64 distinct 1 MiB streams made on the GPU by the adaptive generator
    # (brx_generate_batch, BRX_GEN_ADAPTIVE) from rotations of the Canterbury texts the reference holds: 16 meta-blocks each,
    # codes from each meta-block's statistics, two literal trees behind a context map, ~80 literal block switches per stream
    "gen_c5x1024": (["gen:%d" % k for k in range(64)], 1024),
    # a MIXED batch of the reference's texts (rows of different length and statistics side by side)
    "mixed_textx4096": (["alice29.txt", "asyoulik.txt", "plrabn12.txt", "lcet10.txt"], 4096),
    # ... and a wider mix: 1 MiB multi-meta-block streams, texts that need the level-1 and the level-2 kernel, tiny streams
    "mixed_allx4096": (["alice29.txt", "c5_0", "lcet10.txt", "monkey", "asyoulik.txt", "mapsdatazrh", "plrabn12.txt", "c5_1"], 4096),
}
# workloads whose PHYSICAL HBM traffic is known by construction: every copied byte is read from HBM once ("rw") or the
# copy is a periodic fill served from registers / LDS ("w"); for the others the physical figure is the PMC traffic
PHYSICAL_MODEL = {"farcopy_1MiBx4096": "rw", "backward65536x4096": "w", "quickfox_repeatedx8192": "w", "raw_256KiBx4096": "w"}


def load_fixture(name):
    """(compressed, expected).  config-5 fixtures carry only a sha256: their expected bytes come from the oracle."""
    if name.startswith("farcopy_"):
        import craft
        return craft.farcopy_stream(int(name.split("_")[1]))
    if name.startswith("raw_"):
        import random
        import craft
        data = random.Random(int(name.split("_")[1])).randbytes(256 << 10)
        b = craft.Bits()
        craft.stream_header(b, 22)
        b.put(0, 1); b.put(3, 2); b.put(0, 1); b.put(0, 2); b.put(0, (-b.n) % 8)  # an empty metadata block: byte boundary
        for o in range(0, len(data), 1 << 16):
            craft.raw_block(b, data[o:o + (1 << 16)])
        b.put(3, 2)  # ISLAST, ISLASTEMPTY
        return b.bytes(), data
    if name.startswith("enc:"):
        import hashlib
        import oracle_py
        enc = os.path.join(os.path.dirname(GOLD), "enc")
        comp = open(os.path.join(enc, name[4:] + ".compressed"), "rb").read()
        st, out = oracle_py.decode(comp)[:2]
        man = {e["name"]: e for e in json.load(open(os.path.join(enc, "manifest.json")))["streams"]}
        assert st == 0 and hashlib.sha256(out).hexdigest() == man[name[4:]]["sha256"]
        return comp, out
    if name.startswith("c5_"):
        import hashlib
        import oracle_py
        comp = open(os.path.join(C5, name + ".compressed"), "rb").read()
        st, out = oracle_py.decode(comp)[:2]
        man = {e["name"]: e for e in json.load(open(os.path.join(C5, "manifest.json")))["streams"]}
        assert st == 0 and hashlib.sha256(out).hexdigest() == man[name]["sha256"]
        return comp, out
    return (open(os.path.join(GOLD, name + ".compressed"), "rb").read(), open(os.path.join(GOLD, name), "rb").read())


def cpu_baseline(comp, expect, seconds=12.0):
    """The oracle (CPU restatement of the reference, canonical-lookup mode) on ONE host core, on a bounded
    sample of the same workload: repeated decodes of the same stream for ~`seconds` of CPU time."""
    import ctypes
    import oracle_py
    L = oracle_py.lib()
    cap = len(expect) + 64
    buf = ctypes.create_string_buffer(cap)
    n = ctypes.c_size_t(0)
    st = oracle_py.Stats()
    rc = L.bro_decode(comp, len(comp), buf, cap, ctypes.byref(n), 0, ctypes.byref(st))
    assert rc == 0 and buf.raw[:n.value] == expect
    reps = 0
    t0 = time.perf_counter()
    while True:
        for _ in range(8):
            L.bro_decode(comp, len(comp), buf, cap, ctypes.byref(n), 0, None)
        reps += 8
        dt = time.perf_counter() - t0
        if dt >= seconds:
            break
    return {"value": round(reps * len(expect) / dt / 1e6, 2), "unit": "MB/s", "cores": 1, "kind": "port",
            "sample": "%d sequential decodes of %d B -> %d B in %.1f s, single thread, oracle canonical mode"
                      % (reps, len(comp), len(expect), dt)}, st.as_dict()


def config1_monkey(iters=3000):
    """BASELINE configs[0]: the reference's own bench_monkey plumbing (benches/lib.rs:9-47) on the CPU path that exists
    here, the oracle: the 425-byte stream in memory -> construct the decoder -> read the whole output, ns per iteration
    (median of `iters`), next to the reference's published figure (docs/bench_notes.txt:15, unknown 2015 CPU)."""
    import ctypes
    import oracle_py
    comp, expect = load_fixture("monkey")
    L = oracle_py.lib()
    buf = ctypes.create_string_buffer(len(expect) + 64)
    n = ctypes.c_size_t(0)
    assert L.bro_decode(comp, len(comp), buf, len(buf), ctypes.byref(n), 0, None) == 0 and buf.raw[:n.value] == expect
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter_ns()
        L.bro_decode(comp, len(comp), buf, len(buf), ctypes.byref(n), 0, None)
        ts.append(time.perf_counter_ns() - t0)
    ts.sort()
    med = ts[len(ts) // 2]
    return {"workload": "data/monkey.compressed, single stream, CPU path (bench_monkey plumbing)", "ns_per_iter": med,
            "MB_per_s": round(len(expect) / med * 1e3, 1), "iters": iters, "kind": "port",
            "reference_ns_per_iter": 96182, "reference_source": "docs/bench_notes.txt:15 (2015, CPU not stated)",
            "note": "includes the ctypes call overhead (~1 us)"}


def kernel_source_id():
    """sha256 (16 hex digits) of the kernel sources: ties a committed PMC traffic measurement to the kernel it measured."""
    import hashlib
    h = hashlib.sha256()
    for f in ("brx_hot.S", "brx_lens.S", "brx_kernels.hip", "brx_small.h", "brx_device.h"):
        h.update(open(os.path.join(ROOT, "brotli-rs_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def under_profiler():
    """True when this process already runs under rocprofv3 (the profiles/ passes): no nested profiler then."""
    return any(k.startswith(("ROCPROF", "ROCPROFILER", "ROCP_")) for k in os.environ) or "rocprofiler" in os.environ.get("LD_PRELOAD", "")


def measured_traffic(workload, streams):
    """HBM-side bytes and issued instructions of one launch, measured in this run: three child passes of this script under
    `rocprofv3 --kernel-trace --pmc <counters>` (FETCH_SIZE and WRITE_SIZE do not share a pass, MI355X_MICROARCH.md; the SQ
    instruction counters are a third), 2 launches each, no other trace domain.  Per launch = the regular kernel + the other
    instances around it.  Counter unit KiB; fetch bytes = 2 x FETCH_SIZE (64 counted per 128-byte memory-side request in
    every access pattern of this kernel, profiles/r03_fetchcal.txt), WRITE_SIZE exact.  SQ_BUSY_CYCLES sums the 32 shader
    engines' busy cycles (8 XCDs x 4): / 32 = the launch's cycles.  Returns (total_bytes, detail) or (None, reason)."""
    import csv
    import glob
    import shutil
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    got = {}
    for counters in (("FETCH_SIZE",), ("WRITE_SIZE",), ("SQ_INSTS_SALU", "SQ_INSTS_VALU", "SQ_BUSY_CYCLES")):
        d = tempfile.mkdtemp(prefix="brx_pmc_", dir="/tmp")
        try:
            cmd = [exe, "--kernel-trace", "--pmc"] + list(counters) + ["--output-format", "csv", "-d", d, "-o", "p", "--",
                   sys.executable, os.path.abspath(__file__), "--workload", workload, "--steps", "2", "--warmup", "1",
                   "--no-cpu-baseline", "--no-copy-path", "--no-traffic", "--no-chain-floor", "--no-configs", "--verify", "0"] + (["--streams", str(streams)] if streams else [])
            env = dict(os.environ, TMPDIR="/tmp")
            for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
                env.pop(k, None)
            r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240)
            tot, launches = {c: 0.0 for c in counters}, set()
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if "brx_decode" in row["Kernel_Name"] and row["Counter_Name"] in tot:
                        tot[row["Counter_Name"]] += float(row["Counter_Value"])
                        if row["Kernel_Name"].startswith("brx_decode_kernel("):
                            launches.add(row["Dispatch_Id"])
            if not launches:
                if counters[0].startswith("SQ_"):
                    continue  # (the instruction counters are an extra: the traffic figure stands without them)
                return None, "rocprofv3 --pmc %s: no counter rows (rc %d)" % (counters[0], r.returncode)
            for c in counters:
                got[c] = tot[c] / len(launches)
        except (OSError, subprocess.SubprocessError, KeyError, ValueError) as e:
            if counters[0].startswith("SQ_"):
                continue
            return None, "rocprofv3 --pmc %s failed: %s" % (counters[0], type(e).__name__)
        finally:
            shutil.rmtree(d, ignore_errors=True)
    detail = {"fetch_size_counter_bytes": int(got["FETCH_SIZE"] * 1024.0), "fetch_bytes": int(2 * got["FETCH_SIZE"] * 1024.0),
              "write_bytes": int(got["WRITE_SIZE"] * 1024.0)}
    if "SQ_INSTS_SALU" in got:
        detail["sq"] = {"SQ_INSTS_SALU": int(got["SQ_INSTS_SALU"]), "SQ_INSTS_VALU": int(got["SQ_INSTS_VALU"]),
                        "SQ_BUSY_CYCLES": int(got["SQ_BUSY_CYCLES"])}
    return int((2 * got["FETCH_SIZE"] + got["WRITE_SIZE"]) * 1024.0), detail


def chain_floor(torch, np, dev, ctx, fx, barrier, steps=3, most=8):
    """What one wavefront = one stream bounds a launch by: ONE stream of the workload decoded alone (a launch of one wave on an
    otherwise empty chip), kernel time by HIP events -- the slowest of the workload's distinct members (the first `most`)."""
    worst, which = 0.0, 0
    for k, f in enumerate(fx[:most]):
        b = Batch(torch, np, dev, [f], 1)
        _, kms = timed_pass(ctx, b, steps, 1, barrier)
        if min(kms) > worst:
            worst, which = min(kms), k
        del b
    return worst, which


def libbrotlidec_rate(comp, expect, seconds=3.0):
    """Single-thread rate of the system libbrotlidec (1.0.9 in this image) on the same stream -- not the reference, not
    the baseline of record, just a second CPU yardstick next to the oracle.  None when the library is absent."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import ctypes
        import brotli_enc
        if not brotli_enc.available():
            return None
        dec = ctypes.CDLL("libbrotlidec.so.1")
        dec.BrotliDecoderDecompress.argtypes = [ctypes.c_size_t, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_char_p]
        out = ctypes.create_string_buffer(len(expect) + 64)
        reps, t0 = 0, time.perf_counter()
        while True:
            for _ in range(8):
                n = ctypes.c_size_t(len(out))
                if dec.BrotliDecoderDecompress(len(comp), comp, ctypes.byref(n), out) != 1:
                    return None
            reps += 8
            dt = time.perf_counter() - t0
            if dt >= seconds:
                break
        if out.raw[:n.value] != expect:
            return None
        return {"value": round(reps * len(expect) / dt / 1e6, 2), "unit": "MB/s", "cores": 1,
                "sample": "%d decodes in %.1f s, libbrotlidec.so.1 one-shot API" % (reps, dt)}
    except OSError:
        return None


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it: start N ranks (one per GPU) under
    torch.distributed.run on 127.0.0.1 and hand its exit code back.  Fewer than N visible devices is an error -- never an
    N=1 number under an N-GPU label.  (BRX_BENCH_STUB=1: the CPU test of this launcher -- gloo, no GPU, a stand-in decode.)"""
    import subprocess
    if not STUB:
        import torch
        have = torch.cuda.device_count()
        if have < args.gpus:
            sys.stderr.write("bench.py: --gpus %d asked for, %d GPU(s) visible: refusing to print a number\n" % (args.gpus, have))
            sys.exit(3)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.exit(subprocess.call(cmd, env=env))


class Batch:
    """One synthetic batch resident on the device: stream i = fixture i mod K, each in its own region of the input blob,
    distinct 16-byte aligned output slots."""

    def __init__(self, torch, np, dev, fx, n):
        self.fx, self.n, self.K = fx, n, len(fx)
        K = self.K
        self.cap = (max(len(f[1]) for f in fx) + 15) & ~15  # 16-B aligned slots: every stream's flushes are full 16-B stores
        self.lens = np.array([len(fx[i % K][0]) for i in range(n)], dtype=np.int64)
        in_off_h = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(self.lens, out=in_off_h[1:])
        if K == 1:
            one = torch.frombuffer(bytearray(fx[0][0]), dtype=torch.uint8).to(dev)
            self.blob = one.repeat(n).contiguous()
        else:
            parts = [torch.frombuffer(bytearray(f[0]), dtype=torch.uint8).to(dev) for f in fx]
            self.blob = torch.cat([parts[i % K] for i in range(n)]).contiguous()
        self.in_off = torch.from_numpy(in_off_h).to(dev)
        self.out_off = (torch.arange(n + 1, dtype=torch.int64, device=dev) * self.cap).contiguous()
        self.out = torch.empty(n * self.cap, dtype=torch.uint8, device=dev)
        self.out_len = torch.zeros(n, dtype=torch.int64, device=dev)
        self.status = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.out_bytes = sum(len(fx[i % K][1]) for i in range(n) if len(fx[i % K]) < 3 or fx[i % K][2] == 0)

    def step(self, ctx, timing=False):
        if STUB:  # (launcher test only) stand-in for the decode: the expected bytes into every slot
            import torch
            for k, f in enumerate(self.fx):
                e = f[1]
                want = torch.frombuffer(bytearray(e), dtype=torch.uint8)
                self.out.view(self.n, self.cap)[k::self.K, :len(e)] = want
                self.out_len[k::self.K] = len(e)
            self.status.zero_()
            return
        ctx.decode_batch_device(self.blob.data_ptr(), self.in_off.data_ptr(), self.n, self.out.data_ptr(), self.out_off.data_ptr(),
                                self.out_len.data_ptr(), self.status.data_ptr(), timing=timing)

    def poison(self, torch):
        """Overwrite every output slot, length and status, so that a verify() afterwards proves that the NEXT step wrote them (without
        this the bytes of the warm-up would satisfy it: VERDICT r4).  Waits for the fill: the decode runs on the context's own HIP stream."""
        self.out.fill_(0xA5)
        self.out_len.fill_(-1)
        self.status.fill_(-1)
        if self.out.is_cuda:
            torch.cuda.synchronize()

    def verify(self, torch):
        """status, lengths, and every stream's bytes (checksum of checksums by equality)"""
        ok = True
        for k, f in enumerate(self.fx):
            e, want_st = f[1], (f[2] if len(f) > 2 else 0)
            ok = ok and bool((self.status[k::self.K] == want_st).all().item())
            if want_st == 0:
                want = torch.frombuffer(bytearray(e), dtype=torch.uint8).to(self.out.device)
                ok = ok and bool((self.out_len[k::self.K] == len(e)).all().item())
                got = self.out.view(self.n, self.cap)[k::self.K, :len(e)]
                ok = ok and bool((got == want.unsqueeze(0)).all().item())
            else:  # a stream that fails (cut short): the reference's error kind, and the bytes in front of the error are the oracle's
                m = min(int(self.out_len[k::self.K].min().item()), len(e), self.cap)
                if m > 0:
                    want = torch.frombuffer(bytearray(e[:m]), dtype=torch.uint8).to(self.out.device)
                    ok = ok and bool((self.out.view(self.n, self.cap)[k::self.K, :m] == want.unsqueeze(0)).all().item())
        return ok

    def byte_model(self, which):
        """bytes of one launch: 'alg' (in + out + window-copy bytes read + dictionary bytes read), 'rw' (physical:
        in + out + every copied byte read from HBM) or 'w' (physical: in + out; the fill's source period stays in LDS)"""
        import oracle_py
        per = []
        for f in self.fx:
            c, e = f[0], f[1]
            st = oracle_py.decode(c, want_stats=True)[2]
            per.append(len(c) + len(e) + {"alg": st["copy_bytes"] + st["dict_bytes"], "rw": st["copy_bytes"], "w": 0}[which])
        return sum(per[i % self.K] for i in range(self.n))


def timed_pass(ctx, batch, steps, warmup, barrier):
    """W untimed steps, barrier + synchronize, exactly K timed steps (HIP events around each kernel, on the stream it is
    launched on), barrier + synchronize.  Returns (wall seconds, kernel ms of every step)."""
    import torch
    for _ in range(warmup):
        batch.step(ctx)
    barrier()
    kernel_ms = []
    t0 = time.perf_counter()
    for k in range(steps):
        if k == steps - 1:
            batch.poison(torch)  # inside the timed wall time (one device fill, ~0.1 % of a default run), outside the kernel's HIP events:
                                 # what verify() sees afterwards is the LAST TIMED step's output
        batch.step(ctx, timing=True)
        kernel_ms.append(0.0 if STUB else ctx.last_timing_ms(1))
    barrier()
    return time.perf_counter() - t0, kernel_ms


DUMP_BYTES = 64_000_000  # --dump-outputs writes at most this much


def dump_outputs(path, torch, np, slots, out_len, status):
    """--dump-outputs: what a caller of the timed path received from its last step, so that two builds can be compared output for
    output.  slots: the [n, capacity] uint8 output slots (torch, any device); out_len / status: numpy arrays of n.  Writes
      status.npy, out_len.npy   every stream's (float64)
      sample_streams.npy        a fixed, seeded sample of stream indices -- as many as DUMP_BYTES leaves room for (float64)
      out_bytes.npy             [sample, capacity]: byte j of a sampled stream's slot for j < min(out_len, capacity) (brx.h: the
                                stream's output, or the bytes in front of its error), -1 behind it (float32)"""
    n, cap = slots.shape
    lens = np.asarray(out_len, dtype=np.float64)
    room = (DUMP_BYTES - 3 * 8 * n - 4 * 128) // 4  # float32 bytes left after the three per-stream arrays and the four .npy headers
    width = min(cap, room)
    pick = np.sort(np.random.default_rng(0).choice(n, min(n, room // width), replace=False))
    got = slots[torch.from_numpy(pick).to(slots.device), :width].cpu().numpy().astype(np.float32)
    got[np.arange(width)[None, :] >= np.minimum(lens[pick], cap)[:, None]] = -1.0
    os.makedirs(path, exist_ok=True)
    for name, a in (("status", np.asarray(status, dtype=np.float64)), ("out_len", lens), ("sample_streams", pick.astype(np.float64)),
                    ("out_bytes", got)):
        np.save(os.path.join(path, name + ".npy"), a)


def copy_path(torch, np, dev, ctx, barrier, steps=5):
    """The LZ77 copy path in the driver-run line (north_star: the copy at >= 40 % of HBM peak): three short runs with the
    PHYSICAL bytes known by construction -- far copies HBM -> registers -> HBM (every copied byte read once), the two
    fills of BASELINE configs[2] / configs[3] (in + out only), and uncompressed meta-blocks (input -> registers -> output)."""
    res = {}
    for name in ("farcopy_1MiBx4096", "backward65536x4096", "quickfox_repeatedx8192", "raw_256KiBx4096"):
        fixtures, n = WORKLOADS[name]
        b = Batch(torch, np, dev, [load_fixture(f) for f in fixtures], n)
        dt, kms = timed_pass(ctx, b, steps, 2, barrier)
        ok = b.verify(torch)
        kavg = sum(kms) / len(kms)
        phys = b.byte_model(PHYSICAL_MODEL[name])
        res[name] = {"kernel_ms_avg": round(kavg, 4), "steps": steps, "physical_bytes_per_launch": phys,
                     "achieved_physical_GBs": round(phys / (kavg * 1e-3) / 1e9, 1),
                     "frac_physical": round(phys / (kavg * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                     "decompressed_MB_per_s": round(b.out_bytes * steps / dt / 1e6, 1),
                     "physical_model": PHYSICAL_MODEL[name], "bit_exact": ok}
        del b
        torch.cuda.empty_cache()
    res["frac_physical"] = res["farcopy_1MiBx4096"]["frac_physical"]
    res["note"] = ("physical_model rw = input read + output written + every copied byte read from HBM; w = input read + output "
                   "written (periodic fill, source period in LDS); peak %.0f GB/s" % HBM_PEAK_GBS)
    return res


def other_configs(torch, np, dev, ctx, barrier, with_traffic, steps=5):
    """The other BASELINE configs' per-GPU shares in the driver-run line (VERDICT r5 missing #6): config 5 (1024 x 1 MiB multi-meta-block
    streams with block switches: kernel ms, one stream alone, roofline fraction, counter traffic, bit-exact), and the same batch
    with every 64th stream CUT at a random byte -- one bad stream must not stall its batch (a cut
    1 MiB stream used to be decoded again by the C++ loop, ~8 x the batch)."""
    import random
    import oracle_py
    res = {}
    fixtures, n = WORKLOADS["config5_1MiBx1024"]
    fx = [load_fixture(f) for f in fixtures]
    b = Batch(torch, np, dev, fx, n)
    dt, kms = timed_pass(ctx, b, steps, 1, barrier)
    ok = b.verify(torch)
    kavg = sum(kms) / len(kms)
    alg = b.byte_model("alg")

    def local_sync():
        ctx.synchronize()
        torch.cuda.synchronize()
    floor_ms, _ = chain_floor(torch, np, dev, ctx, fx, local_sync, steps=2, most=4)
    r = {"workload": "%d x %s per GPU (BASELINE configs[4], per-GPU share of 8192 over 8)" % (n, "|".join(fixtures)), "kernel_ms_avg": round(kavg, 3),
         "steps": steps, "decompressed_MB_per_s": round(b.out_bytes * steps / dt / 1e6, 1), "algorithmic_bytes_per_launch": alg,
         "achieved": round(alg / (kavg * 1e-3) / 1e9, 1), "frac": round(alg / (kavg * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
         "chain_floor_ms": round(floor_ms, 3), "frac_of_chain_floor": round(floor_ms / kavg, 4), "bit_exact": ok, "traffic": None}
    if with_traffic:
        try:
            t, detail = measured_traffic("config5_1MiBx1024", 0)
            r["traffic"] = t
            if t:
                r["traffic_over_algorithmic"] = round(t / alg, 2)
            else:
                r["traffic_error"] = detail
        except Exception as e:
            r["traffic_error"] = repr(e)[:200]
    res["config5_1MiBx1024"] = r
    # every 64th stream cut at a random byte (seeded); expected status and bytes from the oracle
    rng = random.Random(64)
    cut_fx = []
    for i in range(n):
        comp, exp = fx[i % len(fx)]
        if i % 64 == 63:
            c = comp[:rng.randrange(len(comp) // 20, len(comp) - 1)]
            st, out = oracle_py.decode(c, 0, cap=len(exp) + 64)[:2]
            cut_fx.append((c, out, st))
        else:
            cut_fx.append((comp, exp, 0))
    bc = Batch(torch, np, dev, cut_fx, n)
    dtc, kmsc = timed_pass(ctx, bc, steps, 1, barrier)
    okc = bc.verify(torch)
    kc = sum(kmsc) / len(kmsc)
    res["config5_cut_1MiBx1024"] = {"workload": "the same batch, every 64th stream cut at a random byte (16 streams: status and bytes in front of the error "
                                                "against the oracle)", "kernel_ms_avg": round(kc, 3), "over_all_valid": round(kc / kavg, 3),
                                    "rollbacks_last_launch": ctx.last_spec_rollbacks(), "cut_statuses": sorted({f[2] for f in cut_fx if f[2]}),
                                    "bit_exact": okc}
    del b, bc
    torch.cuda.empty_cache()
    return res


def node_abi(torch, np, dev, local_rank, fx, n, ctx_ms, steps=5):
    """The node entry of the C ABI (brx_node_decode_batch, round 6) on the GPU this run has: the headline batch through a node of ONE
    rank (the root decodes in place: what the extra layer costs), and over TWO virtual ranks on this GPU (half the batch travels by
    peer copy, is decoded into slots of its own, compacted, copied back and expanded: the whole exchange on one GPU -- function, not
    speed).  Real multi-GPU numbers: `bench.py --gpus N --node device|host` on a machine that has the GPUs."""
    from brotli_rs_amd import brx
    res = {}
    for tag, devices, ranks in (("one_rank", [local_rank], 1), ("two_virtual_ranks", [local_rank, local_rank], 2)):
        node = brx.Node(devices)
        try:
            b = Batch(torch, np, dev, fx, n)
            best = 1e9
            for k in range(steps + 1):
                if k == steps:
                    b.poison(torch)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                node.decode_batch_device(b.blob.data_ptr(), b.in_off.data_ptr(), n, b.out.data_ptr(), b.out_off.data_ptr(), b.out_len.data_ptr(),
                                         b.status.data_ptr(), use_gpus=ranks, timing=True)
                if k:
                    best = min(best, time.perf_counter() - t0)
            last = node.last()
            res[tag] = {"wall_ms_best": round(best * 1e3, 3), "kernel_ms_per_rank": [round(v, 3) for v in last["kernel_ms"]], "streams_per_rank": last["streams"],
                        "bit_exact": b.verify(torch), "rccl": last["rccl"]}
            del b
        finally:
            node.close()
        torch.cuda.empty_cache()
    res["one_rank"]["over_ctx_kernel_ms"] = round(res["one_rank"]["wall_ms_best"] - ctx_ms, 3)
    res["what"] = "brx_node_decode_batch, BRX_MEM_DEVICE, wall time of the synchronous call (the decode kernels + the call; two ranks: + scatter, compaction, gather, expansion)"
    return res


def node_main(args):
    """`--gpus N --node host|device`: ONE process, N GPUs, brx_node_decode_batch (the C ABI's node entry; no torch.distributed).  The
    batch is N x the per-GPU workload; `host`: pinned host buffers used in place by every GPU (no exchange, PCIe inside the time);
    `device`: everything on GPU 0, shards scattered over xGMI, results gathered back (RCCL or peer copies) -- the exchange is INSIDE
    the time here, unlike the driver's one-process-per-GPU mode whose `value` has the inputs resident on every GPU."""
    import numpy as np
    import torch
    from brotli_rs_amd import brx
    if torch.cuda.device_count() < args.gpus:
        sys.stderr.write("bench.py: --gpus %d asked for, %d GPU(s) visible: refusing to print a number\n" % (args.gpus, torch.cuda.device_count()))
        sys.exit(3)
    fixtures, n = WORKLOADS[args.workload]
    if args.streams:
        n = args.streams
    fx = [load_fixture(f) for f in fixtures]
    N = n * args.gpus
    node = brx.Node(list(range(args.gpus)))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    b = Batch(torch, np, dev, fx, N)
    if args.node == "host":
        hin, hout = brx.host_alloc(int(b.blob.numel())), brx.host_alloc(N * b.cap)
        hin[:] = b.blob.cpu().numpy()
        io, oo = b.in_off.cpu().numpy().astype(np.uint64), b.out_off.cpu().numpy().astype(np.uint64)

    def step(timing=False):
        if args.node == "host":
            return node.decode_batch_host_raw(hin.ctypes.data, io, N, hout.ctypes.data, oo, deal=args.deal, use_gpus=args.gpus, timing=timing)
        node.decode_batch_device(b.blob.data_ptr(), b.in_off.data_ptr(), N, b.out.data_ptr(), b.out_off.data_ptr(), b.out_len.data_ptr(),
                                 b.status.data_ptr(), deal=args.deal, use_gpus=args.gpus, timing=timing)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        if k == args.steps - 1 and args.node == "device":
            b.poison(torch)
        r = step(timing=(k == args.steps - 1))
    dt = time.perf_counter() - t0
    last = node.last()
    if args.node == "host":
        st, ln = r
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, torch, np, torch.from_numpy(hout[:N * b.cap]).view(N, b.cap), ln, st)
        ok = (not st.any()) and all(hout[i * b.cap:i * b.cap + len(fx[i % len(fx)][1])].tobytes() == fx[i % len(fx)][1] for i in (0, N // 2, N - 1))
    else:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, torch, np, b.out.view(N, b.cap), b.out_len.cpu().numpy(), b.status.cpu().numpy())
        ok = b.verify(torch)
    res = {"metric": "decompressed MB/s (whole node), %s batch, single process through brx_node_decode_batch (%s pointers)" % (args.workload, args.node),
           "value": round(b.out_bytes * args.steps / dt / 1e6, 1), "unit": "MB/s", "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8",
           "data": "synthetic (fixture(s) %s replicated)" % ",".join(fixtures[:8]),
           "config": {"workload": "%d x %s per GPU" % (n, "|".join(f + ".compressed" for f in fixtures[:8])), "streams_per_gpu": n, "streams_total": N,
                      "sharding": "one process, brx_node_decode_batch: %s deal over %d GPUs; %s" % (args.deal, args.gpus,
                                  "pinned host buffers used in place by every GPU, PCIe inside the time" if args.node == "host" else
                                  "batch resident on GPU 0, scatter + ragged gather over xGMI INSIDE the time (%s)" % ("RCCL" if last["rccl"] else "peer copies"))},
           "exchange_inclusive": True, "bit_exact": bool(ok), "kernel_ms_per_rank": [round(v, 4) for v in last["kernel_ms"]], "streams_per_rank": last["streams"],
           "last_call_wall_ms": round(last["wall_ms"], 3), "scatter_ms": round(last["scatter_ms"], 3)}
    node.close()
    print(json.dumps(res), flush=True)
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(0 if ok else 2)  # (RCCL prints its banner to stdout from a destructor at interpreter exit: the JSON line stays the last one)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="alice29x4096", choices=sorted(WORKLOADS))
    ap.add_argument("--streams", type=int, default=0, help="override streams per GPU")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure everything besides the headline: strong scaling and the gather (N>1), CPU "
                         "baselines, roofline with PMC traffic and chain floor, copy_path, configs, node_abi, the host path")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines (and the host path that goes with them)")
    ap.add_argument("--no-copy-path", action="store_true", help="--full: skip copy_path")
    ap.add_argument("--no-traffic", action="store_true", help="--full: skip the in-run rocprofv3 --pmc passes (roofline.traffic from the committed file)")
    ap.add_argument("--no-chain-floor", action="store_true", help="--full: skip roofline.chain_floor_ms (the single-stream launches after the timed region)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--verify", type=int, default=1)
    ap.add_argument("--gather", action="store_true", help="also time the ragged gather of the outputs to rank 0 (--full at N>1: always)")
    ap.add_argument("--node", choices=["host", "device"], default=None, help="ONE process for all N GPUs through brx_node_decode_batch (the C ABI's node entry) instead of one rank per GPU")
    ap.add_argument("--deal", choices=["ranges", "bytes", "snake"], default="ranges", help="--node: how the batch is dealt over the GPUs")
    ap.add_argument("--no-configs", action="store_true", help="--full: skip the `configs` block (config 5's per-GPU share, the cut-stream batch) and `node_abi`")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy (rank 0's batch; see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1 (the last timed step is the one verified and dumped)")

    if args.node and not STUB:
        node_main(args)  # does not return

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)  # does not return

    import numpy as np
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE=%d: the line would carry the wrong n_gpus\n" % (args.gpus, world))
        sys.exit(3)
    if STUB:
        dev = torch.device("cpu")
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group(backend="gloo")
    else:
        if torch.cuda.device_count() <= local_rank:
            sys.stderr.write("bench.py: rank %d has no GPU (%d visible)\n" % (rank, torch.cuda.device_count()))
            sys.exit(3)
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group(backend="nccl", device_id=dev)
    if world > 1:
        assert dist.get_world_size() == args.gpus

    ctx = None
    if not STUB:
        from brotli_rs_amd import brx
        import brx_knobs  # (A/B knobs of the tools/gpu_*.sh scripts: explicit brx_ctx_set_option calls, reported in the line as `options`)
        ctx = brx_knobs.context(local_rank)

    fixtures, n = WORKLOADS[args.workload]
    if args.streams:
        n = args.streams
    if fixtures[0].startswith("gen:"):  # made here, on the GPU, before anything is timed
        corpus = b"".join(open(os.path.join(GOLD, t), "rb").read() for t in ("lcet10.txt", "alice29.txt", "plrabn12.txt", "asyoulik.txt"))
        srcs = [(corpus[(k * 18211) % len(corpus):] + corpus)[:1 << 20] for k in range(len(fixtures))]
        fx = list(zip(ctx.generate_batch(srcs, metablock_bytes=65536, adaptive=True), srcs))
    else:
        fx = [load_fixture(f) for f in fixtures]
    K = len(fx)
    comp, expect = fx[0]
    batch = Batch(torch, np, dev, fx, n)
    if not STUB:
        torch.cuda.synchronize()

    def barrier():
        if world > 1:
            dist.barrier()
        if not STUB:
            ctx.synchronize()
            torch.cuda.synchronize()

    def max_over_ranks(x):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def all_ranks(x):
        if world == 1:
            return [x]
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        ts = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(ts, t)
        return [float(v.item()) for v in ts]

    dt, kernel_ms = timed_pass(ctx, batch, args.steps, args.warmup, barrier)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, torch, np, batch.out.view(n, batch.cap), batch.out_len.cpu().numpy(), batch.status.cpu().numpy())
    dt = max_over_ranks(dt)
    kavg = sum(kernel_ms) / max(len(kernel_ms), 1)
    kavg_ranks = all_ranks(kavg)

    # The RCCL exchange around the decode, timed on its own AFTER the timed region -- never part of `value`:
    # compaction of the capacity slots + grouped send/recv of the ragged outputs to rank 0 (brotli-rs_amd/shard.py).
    gather_info = None
    if ((world > 1 and args.full) or args.gather) and not STUB:
        try:
            from brotli_rs_amd import shard
            if world == 1 and not dist.is_initialized():
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                os.environ.setdefault("MASTER_PORT", str(_free_port()))
                dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=dev)
            produced = torch.where(batch.status == 0, batch.out_len, torch.zeros_like(batch.out_len))
            times = []
            for _ in range(3):
                barrier()
                tg = time.perf_counter()
                cdata, coffs = shard.compact(batch.out, batch.out_off, produced, ctx=ctx)
                full, offs_all, st_all = shard.gather_ragged(cdata, coffs, batch.status, n * world, dst=0, device=dev)
                torch.cuda.synchronize()
                if world > 1:
                    dist.barrier()
                times.append(time.perf_counter() - tg)
            g = min(times)
            gather_info = {"ms": round(g * 1e3, 3), "bytes_at_root": int(full.numel()) if full is not None else None,
                           "what": "device-side compaction + grouped send/recv of the ragged outputs to rank 0 (best of 3)"}
            del full, cdata
        except Exception as e:  # the gather must never take the decode measurement down with it
            gather_info = {"error": repr(e)[:200]}

    # parity on the timed output
    ok = batch.verify(torch) if args.verify else True

    # Strong scaling, the metric as BASELINE.json words it ("a 4096-stream batch at 1/2/4/8 GPUs"): the SAME total batch
    # split over the ranks, n / N streams per GPU.  At N = 1 it is the weak figure.  Never `value`; --full only.
    strong = None
    if world > 1 and args.full:
        ns = max(n // world, 1)
        sb = Batch(torch, np, dev, fx, ns)
        sdt, skms = timed_pass(ctx, sb, args.steps, 1, barrier)
        sdt = max_over_ranks(sdt)
        ok = ok and (sb.verify(torch) if args.verify else True)
        strong = {"streams_total": ns * world, "streams_per_gpu": ns, "ms_per_step": round(sdt / args.steps * 1e3, 4),
                  "value": round(float(sb.out_bytes) * world * args.steps / sdt / 1e6, 1), "unit": "MB/s",
                  "kernel_ms_per_rank": [round(v, 4) for v in all_ranks(sum(skms) / len(skms))]}
        del sb
    if world > 1:
        f = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(f, op=dist.ReduceOp.MIN)
        ok = bool(f.item())

    if rank == 0:
        out_bytes_gpu = batch.out_bytes
        lens = batch.lens
        total_out = float(out_bytes_gpu) * world
        ms_per_step = dt / args.steps * 1e3
        value = total_out * args.steps / dt / 1e6
        res = {"metric": "decompressed MB/s (whole node), %s batch" % args.workload, "value": round(value, 1),
               "unit": "MB/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": "u8", "data": "synthetic (fixture(s) %s replicated)" % (",".join(fixtures) if len(fixtures) <= 8 else "%s .. %s" % (fixtures[0], fixtures[-1])),
               "config": {"workload": "%d x %s per GPU" % (n, ("%d distinct 1 MiB streams made on the GPU (brx_generate_batch, adaptive)" % len(fixtures))
                                                              if fixtures[0].startswith("gen:") else "|".join(f + ".compressed" for f in fixtures)),
                          "streams_per_gpu": n,
                          "in_bytes_per_stream": int(lens.mean()), "out_bytes_per_stream": out_bytes_gpu // n,
                          "sharding": "independent streams, contiguous index range per rank, no data-path collective"},
               "bit_exact": ok, "bit_exact_of": "the last timed step (outputs, lengths and status poisoned in front of it)", "kernel_ms_per_rank": [round(v, 4) for v in kavg_ranks]}
        if not STUB and brx_knobs.options_from_env():
            res["options"] = brx_knobs.options_from_env()  # (non-default library options of this run, tests/brx_knobs.py)
        if STUB:
            res["stub"] = "BRX_BENCH_STUB=1: launcher test on CPU, the decode is a stand-in -- `value` means nothing"
            res["data"] = "STUB"
        if args.full:
            if strong is None:
                strong = {"streams_total": n, "streams_per_gpu": n, "ms_per_step": round(ms_per_step, 4), "value": round(value, 1),
                          "unit": "MB/s", "note": "N = 1: the strong-scaling batch is the weak one"}
            strong["what"] = ("the SAME %d-stream batch split over N GPUs (BASELINE.json's metric as worded).  One wavefront decodes one stream, so "
                              "a GPU's time is bounded below by ONE stream alone (profiles/r04_sweep.txt: 256 .. 4096 x alice29 take 6.6 .. 8.3 ms): "
                              "N GPUs buy at most that ratio on a 4096-stream batch; throughput scales with N only at >= 4096 streams per GPU "
                              "(`value`, weak)" % strong["streams_total"])
            res["strong"] = strong
        if gather_info:
            if "ms" in gather_info:
                gather_info["decode_plus_gather_MB_per_s"] = round(total_out / (dt / args.steps + gather_info["ms"] * 1e-3) / 1e6, 1)
            res["gather"] = gather_info
        if STUB:
            print(json.dumps(res), flush=True)
    if STUB:
        if dist.is_initialized():
            dist.destroy_process_group()
        sys.exit(0 if ok else 2)

    # Every collective of this run is behind us.  What follows is rank 0's alone and, with --full, takes a while (CPU baseline ~12 s,
    # rocprofv3 child passes, single-stream launches): the other ranks must not sit in an RCCL call meanwhile (its watchdog would end the
    # job) -- the group is taken down HERE, together, and they leave.  (VERDICT r4 #6b)
    used_rccl = dist.is_initialized()
    if used_rccl:
        try:
            dist.barrier()
        except Exception:
            pass
        dist.destroy_process_group()  # (RCCL prints its library path to stdout around here: the JSON line goes last)
    if rank != 0:
        ctx.close()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0 if ok else 2)  # (no interpreter teardown: RCCL's destructor prints to stdout, the contract is ONE JSON line)

    if rank == 0 and args.full:
        import oracle_py
        cb = None
        if not args.no_cpu_baseline:
            try:
                cb, _ = cpu_baseline(comp, expect, args.cpu_seconds)
            except Exception as e:  # (a leg of rank 0 never takes the line down with it)
                res["cpu_baseline_error"] = repr(e)[:200]
        # ALGORITHMIC bytes per stream: compressed in + decompressed out + window-copy bytes read +
        # dictionary bytes read; per launch = summed over the streams of one GPU.
        alg_launch = batch.byte_model("alg")
        kms = sorted(kernel_ms)[len(kernel_ms) // 2] if kernel_ms else float("nan")
        achieved = alg_launch / (kavg * 1e-3) / 1e9
        # HBM-side bytes per launch: PMC counters cannot be read from inside this process, so two short child passes of
        # this script run under rocprofv3 --pmc (FETCH_SIZE, WRITE_SIZE; measured_traffic) after the timed region.  When
        # that is not possible (--no-traffic, already under a profiler, no rocprofv3) the committed measurement
        # profiles/hbm_traffic.json is used -- only if it is of THIS kernel (kernel_source_id), else traffic = null.
        traffic, traffic_src, traffic_detail = None, None, None
        if not args.no_traffic and world == 1 and not under_profiler() and not STUB:
            try:
                traffic, traffic_detail = measured_traffic(args.workload, args.streams)
            except Exception as e:
                traffic, traffic_detail = None, repr(e)[:200]
            if traffic is not None:
                traffic_src = "in-run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (two child passes, 2 launches each)"
            else:
                traffic_src, traffic_detail = "in-run passes failed (%s); " % traffic_detail, None
        if traffic is None:
            try:
                tj = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))
                if tj.get("kernel_source_id") == kernel_source_id():
                    traffic = tj["workloads"][args.workload]["total_bytes"]
                    traffic_src = (traffic_src or "") + "profiles/hbm_traffic.json (%s)" % tj.get("round", "?")
                else:
                    traffic_src = (traffic_src or "") + "stale: profiles/hbm_traffic.json (%s) measured kernel %s, this is %s" % (
                        tj.get("round", "?"), tj.get("kernel_source_id", "?"), kernel_source_id())
            except (OSError, KeyError, ValueError):
                pass
        res["roofline"] = {"bound": "hbm", "kernel": "brx_decode_kernel", "achieved": round(achieved, 1),
                           "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                           "traffic": traffic, "traffic_source": traffic_src,
                           **({"traffic_detail": traffic_detail} if traffic_detail else {}),
                           "algorithmic_bytes_per_launch": alg_launch,
                           "kernel_ms_avg": round(kavg, 4), "kernel_ms_median": round(kms, 4)}
        # The fractions that bind this kernel (one wavefront decodes one stream): the launch against ONE stream alone, the
        # CU's scalar-ALU issue share, instructions per output byte -- measured in this run.
        try:
            if args.no_chain_floor:
                raise RuntimeError("--no-chain-floor")
            def local_sync():
                ctx.synchronize()
                torch.cuda.synchronize()
            floor_ms, floor_k = chain_floor(torch, np, dev, ctx, fx, local_sync)
            res["roofline"]["chain_floor_ms"] = round(floor_ms, 4)
            res["roofline"]["frac_of_chain_floor"] = round(floor_ms / kavg, 4)
            res["roofline"]["chain_floor_what"] = ("one launch of ONE stream of the workload (%s), best of 3, HIP events: the time below which "
                                                   "no batch of such streams can finish" % (fixtures[floor_k] if K > 1 else fixtures[0]))
        except Exception as e:
            res["roofline"]["chain_floor_ms"] = None
            res["roofline"]["chain_floor_error"] = repr(e)[:200]
        sq = (traffic_detail or {}).get("sq")
        if sq:
            cus = torch.cuda.get_device_properties(dev).multi_processor_count
            cycles = sq["SQ_BUSY_CYCLES"] / 32.0
            res["roofline"]["salu_issue_frac"] = round(sq["SQ_INSTS_SALU"] / (cus * cycles), 4)
            res["roofline"]["valu_issue_frac_per_simd"] = round(sq["SQ_INSTS_VALU"] / (cus * 4 * cycles) * 4.0, 4)
            res["roofline"]["insts_per_output_byte"] = round((sq["SQ_INSTS_SALU"] + sq["SQ_INSTS_VALU"]) / float(out_bytes_gpu), 3)
            res["roofline"]["issue_note"] = ("SQ_INSTS_SALU / (CUs x launch cycles): one scalar ALU per CU issues one instruction per cycle for all its "
                                             "waves; VALU: one wave64 instruction occupies its SIMD for 4 cycles (4 SIMDs per CU); launch cycles = SQ_BUSY_CYCLES / 32 shader engines")
        model = PHYSICAL_MODEL.get(args.workload)
        if model:  # physical HBM bytes known by construction ("report both")
            phys_launch = batch.byte_model(model)
            res["roofline"]["physical_bytes_per_launch"] = phys_launch
            res["roofline"]["achieved_physical"] = round(phys_launch / (kavg * 1e-3) / 1e9, 1)
            res["roofline"]["frac_physical"] = round(phys_launch / (kavg * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
            res["roofline"]["physical_model"] = ("input read + output written + every copied byte read from HBM" if model == "rw"
                                                 else "input read + output written (the fill's source period stays in LDS)")
        elif traffic:
            res["roofline"]["achieved_physical"] = round(traffic / (kavg * 1e-3) / 1e9, 1)
            res["roofline"]["frac_physical"] = round(traffic / (kavg * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
            res["roofline"]["physical_model"] = "PMC traffic (FETCH_SIZE + WRITE_SIZE)"
    del batch
    torch.cuda.empty_cache()
    if rank == 0 and args.full:
        if not args.no_copy_path and world == 1:
            try:
                res["copy_path"] = copy_path(torch, np, dev, ctx, barrier)
            except Exception as e:  # never takes the headline down with it
                res["copy_path"] = {"error": repr(e)[:200]}
        if not args.no_configs and world == 1 and args.workload == "alice29x4096" and not under_profiler():  # (under rocprofv3 the kernel statistics must be the headline's alone)
            try:
                res["configs"] = other_configs(torch, np, dev, ctx, barrier, with_traffic=not args.no_traffic and not under_profiler())
            except Exception as e:
                res["configs"] = {"error": repr(e)[:200]}
            try:
                res["node_abi"] = node_abi(torch, np, dev, local_rank, fx, n, kavg)
            except Exception as e:
                res["node_abi"] = {"error": repr(e)[:200]}
        if cb and world == 1 and K == 1:
            # informational, never part of `value`: the same batch from pinned HOST buffers to pinned host buffers through the
            # C ABI's host-pointer path (the kernel reads the input and stores the output over PCIe while it decodes)
            try:
                cap = (len(expect) + 15) & ~15
                hin, hout = brx.host_alloc(len(comp) * n), brx.host_alloc(cap * n)
                hin[:] = np.frombuffer(comp * n, dtype=np.uint8)
                io = np.arange(n + 1, dtype=np.uint64) * len(comp)
                oo = np.arange(n + 1, dtype=np.uint64) * cap
                best = 1e9
                for _ in range(3):
                    t1 = time.perf_counter()
                    hst, hln = ctx.decode_batch_host_raw(hin.ctypes.data, io, n, hout.ctypes.data, oo)
                    best = min(best, time.perf_counter() - t1)
                okh = (not hst.any()) and hout[:len(expect)].tobytes() == expect and hout[(n - 1) * cap:(n - 1) * cap + len(expect)].tobytes() == expect
                res["host_path_pcie_inclusive"] = {"ms": round(best * 1e3, 3), "MB_per_s": round(n * len(expect) / best / 1e6, 1),
                                                   "bit_exact": bool(okh), "buffers": "pinned (brx_host_alloc), used in place"}
                brx.host_free(hin)
                brx.host_free(hout)
            except Exception as e:
                res["host_path_pcie_inclusive"] = {"error": repr(e)[:200]}
        if cb:
            res["config1"] = config1_monkey()
            res["cpu_baseline"] = cb
            res["speedup_vs_cpu_1core"] = round(value / world / cb["value"], 1)
            other = libbrotlidec_rate(comp, expect)
            if other:
                res["cpu_libbrotlidec"] = other  # informational: Google's optimized C decoder, if the image has it
            try:  # informational: the oracle on every host core at once (CPU baseline item b)
                import subprocess
                if fixtures[0].startswith("gen:"):
                    raise KeyError("no file")
                fixture_path = os.path.join(C5 if fixtures[0].startswith("c5_") else GOLD, fixtures[0] + ".compressed")
                o = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cpu_all_cores.py"), fixture_path, "4"],
                                   capture_output=True, text=True, timeout=180)
                res["cpu_all_cores"] = json.loads(o.stdout.strip().splitlines()[-1])
            except Exception:
                pass
    ctx.close()
    if rank == 0:
        sys.stdout.flush()
        print(json.dumps(res), flush=True)
    if used_rccl:
        # RCCL prints "Librccl path : ..." to stdout from a destructor at interpreter exit; the contract is ONE JSON line
        # (and it must be the last thing on stdout): leave without running destructors -- everything is flushed and closed.
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0 if ok else 2)
    if not ok:
        sys.exit(2)


if __name__ == "__main__":
    main()
