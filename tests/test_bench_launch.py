"""bench.py's own launcher: `python bench.py --gpus N` must start N ranks by itself, and must refuse
to print a number when it cannot.  CPU only: BRX_BENCH_STUB=1 swaps the decode for a stand-in and RCCL for gloo -- what is
tested is the launch, the rendezvous, the max-over-ranks reduction and the shape of the line, never a rate."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, stub):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    env.pop("LOCAL_RANK", None)
    if stub:
        env["BRX_BENCH_STUB"] = "1"
    else:
        env.pop("BRX_BENCH_STUB", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=600)


def test_gpus_2_starts_two_ranks():
    r = _run(["--gpus", "2", "--full", "--steps", "2", "--warmup", "1", "--workload", "monkeyx16384", "--streams", "8"], stub=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["stub"] and res["data"] == "STUB"
    assert len(res["kernel_ms_per_rank"]) == 2
    assert res["strong"]["streams_per_gpu"] == 4 and res["strong"]["streams_total"] == 8
    assert res["scaling"] == "weak" and res["bit_exact"] is True
    assert len(res["strong"]["kernel_ms_per_rank"]) == 2 and res["strong"]["unit"] == "MB/s" and "what" in res["strong"]
    assert res["steps"] == 2 and res["warmup"] == 1 and res["higher_is_better"] is True and res["vs_baseline"] is None
    assert "poisoned" in res["bit_exact_of"]


EXTRAS = ("strong", "gather", "roofline", "copy_path", "configs", "node_abi", "host_path_pcie_inclusive", "config1", "cpu_baseline",
          "speedup_vs_cpu_1core", "cpu_libbrotlidec", "cpu_all_cores")


def test_plain_run_prints_the_headline_alone():
    """Without --full a run times its steps and prints the headline line: nothing measured besides it, at N = 1 and N = 2; with
    --full the N = 1 line carries `strong` again."""
    for gpus in ("1", "2"):
        r = _run(["--gpus", gpus, "--steps", "2", "--warmup", "1", "--workload", "monkeyx16384", "--streams", "8"], stub=True)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        res = json.loads(lines[0])
        assert res["n_gpus"] == int(gpus) and len(res["kernel_ms_per_rank"]) == int(gpus) and res["steps"] == 2 and res["warmup"] == 1
        assert res["unit"] == "MB/s" and res["higher_is_better"] is True and res["dtype"] == "u8" and res["bit_exact"] is True
        assert res["value"] > 0 and res["ms_per_step"] > 0 and res["metric"] == "decompressed MB/s (whole node), monkeyx16384 batch"
        assert not [k for k in EXTRAS if k in res], res
    r = _run(["--gpus", "1", "--full", "--steps", "2", "--warmup", "1", "--workload", "monkeyx16384", "--streams", "8"], stub=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["strong"]["streams_per_gpu"] == 8 and res["strong"]["ms_per_step"] == res["ms_per_step"]


def test_gpus_2_without_two_gpus_fails_loudly():
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("two GPUs present")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], stub=False)
    assert r.returncode != 0
    assert not any(l.startswith("{") for l in r.stdout.splitlines()), r.stdout
    assert "refusing" in r.stderr


def test_world_size_mismatch_fails_loudly():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", BRX_BENCH_STUB="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and not any(l.startswith("{") for l in r.stdout.splitlines())


def test_in_run_traffic_reads_the_pmc_passes(tmp_path, monkeypatch):
    """roofline.traffic is measured by the bench itself: three child passes under `rocprofv3 --pmc` (bench.measured_traffic).  Here
    a stand-in `rocprofv3` on PATH writes the counter files a real pass leaves; what is tested is the command line (one counter
    per pass, --kernel-trace, no other trace domain, the child told not to recurse), the per-launch sum over the regular
    kernel and the wider instances behind it, the KiB unit and the calibrated x 2 of FETCH_SIZE."""
    fake = tmp_path / "rocprofv3"
    fake.write_text('''#!%s
import os, sys
a = sys.argv[1:]
d = a[a.index("-d") + 1]
i = a.index("--pmc") + 1
cs = []
while not a[i].startswith("--"):
    cs.append(a[i]); i += 1
assert "--kernel-trace" in a and "--no-traffic" in a and "--no-chain-floor" in a and "--sys-trace" not in a and "-s" not in a and "--hip-trace" not in a
assert a.count("--pmc") == 1 and (len(cs) == 1 or all(c.startswith("SQ_") for c in cs))  # FETCH_SIZE / WRITE_SIZE: a pass each
open(os.path.join(os.environ["FAKE_LOG"]), "a").write("+".join(cs) + "\\n")
os.makedirs(os.path.join(d, "host", "123"), exist_ok=True)
rows = ["Dispatch_Id,Kernel_Name,Counter_Name,Counter_Value"]
for c in cs:
    v = {"FETCH_SIZE": 1000.0, "WRITE_SIZE": 300.0, "SQ_INSTS_SALU": 7000.0, "SQ_INSTS_VALU": 5000.0, "SQ_BUSY_CYCLES": 3200.0}[c]
    for disp in (1, 5):  # two launches: the regular kernel + one wider instance behind each, and a kernel that is not ours
        rows.append('%%d,"brx_decode_kernel(BrxKernelArgs)",%%s,%%f' %% (disp, c, v))
        rows.append('%%d,"brx_decode_kernel_l3(BrxKernelArgs)",%%s,%%f' %% (disp + 1, c, 24.0))
        rows.append('%%d,"fill_kernel",%%s,%%f' %% (disp + 2, c, 1e9))
open(os.path.join(d, "host", "123", "p_counter_collection.csv"), "w").write("\\n".join(rows) + "\\n")
''' % sys.executable)
    fake.chmod(0o755)
    monkeypatch.setenv("PATH", str(tmp_path) + os.pathsep + os.environ["PATH"])
    monkeypatch.setenv("FAKE_LOG", str(tmp_path / "log.txt"))
    sys.path.insert(0, ROOT)
    import bench
    total, detail = bench.measured_traffic("alice29x4096", 0)
    assert (tmp_path / "log.txt").read_text().split() == ["FETCH_SIZE", "WRITE_SIZE", "SQ_INSTS_SALU+SQ_INSTS_VALU+SQ_BUSY_CYCLES"]
    assert detail == {"fetch_size_counter_bytes": 1024 * 1024, "fetch_bytes": 2 * 1024 * 1024, "write_bytes": 324 * 1024,
                      "sq": {"SQ_INSTS_SALU": 7024, "SQ_INSTS_VALU": 5024, "SQ_BUSY_CYCLES": 3224}}
    assert total == 2 * 1024 * 1024 + 324 * 1024
    assert not bench.under_profiler()
    monkeypatch.setenv("ROCPROF_OUTPUT_PATH", "/tmp/x")
    assert bench.under_profiler()


def test_dump_outputs_is_the_last_timed_step_and_repeats(tmp_path):
    """--dump-outputs DIR: the slots, lengths and status the last timed step left (the stand-in decode writes the fixture's bytes),
    the same from run to run; --steps is the number of timed steps and must be at least 1."""
    import numpy as np
    runs = []
    for k in range(2):
        d = tmp_path / ("d%d" % k)
        r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "monkeyx16384", "--streams", "8", "--dump-outputs", str(d)], stub=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["steps"] == 3
        runs.append({n: np.load(d / (n + ".npy")) for n in ("status", "out_len", "sample_streams", "out_bytes")})
    a, b = runs
    assert all(np.array_equal(a[n], b[n]) and a[n].dtype == b[n].dtype for n in a)
    want = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "data", "monkey"), "rb").read(), dtype=np.uint8)
    assert a["out_bytes"].dtype == np.float32 and a["out_len"].dtype == np.float64
    assert (a["status"] == 0).all() and (a["out_len"] == len(want)).all() and (a["sample_streams"] == np.arange(8)).all()
    assert (a["out_bytes"][:, :len(want)] == want).all() and (a["out_bytes"][:, len(want):] == -1).all()
    r = _run(["--gpus", "1", "--steps", "0", "--warmup", "1", "--dump-outputs", str(tmp_path / "none")], stub=True)
    assert r.returncode != 0 and not any(l.startswith("{") for l in r.stdout.splitlines()) and not (tmp_path / "none").exists()


def test_dump_outputs_samples_a_large_batch_within_64_MB(tmp_path):
    """A batch whose slots exceed the budget: a fixed, seeded sample of whole streams, each slot's bytes up to min(out_len, capacity)
    and -1 behind (statuses other than 0 keep the bytes in front of the error, brx.h), at most 64 MB in all."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n, cap = 600, 152096
    g = torch.Generator().manual_seed(5)
    slots = torch.randint(0, 256, (n, cap), dtype=torch.uint8, generator=g)
    out_len = np.random.default_rng(5).integers(0, 2 * cap, n).astype(np.uint64)
    status = np.where(out_len > cap, 25, 0).astype(np.int32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch, np, slots, out_len, status)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["out_bytes.npy", "out_len.npy", "sample_streams.npy", "status.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64_000_000
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    pick = np.load(tmp_path / "a" / "sample_streams.npy").astype(np.int64)
    got = np.load(tmp_path / "a" / "out_bytes.npy")
    assert 50 < len(pick) < n and (np.diff(pick) > 0).all() and got.shape == (len(pick), cap)
    assert np.array_equal(np.load(tmp_path / "a" / "out_len.npy"), out_len.astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "a" / "status.npy"), status.astype(np.float64))
    for row, i in zip(got, pick):
        m = min(int(out_len[i]), cap)
        assert (row[:m] == slots[i, :m].numpy()).all() and (row[m:] == -1).all()
