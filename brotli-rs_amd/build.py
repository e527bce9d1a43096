"""Build libbrx.so (HIP kernels + C ABI) in-tree for gfx950.  hipcc cross-compiles without a GPU."""
import os
import re
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIB_PATH = os.path.join(PKG, "libbrx.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCES = ["brx_kernels.hip", "brx_kernels_l1.hip", "brx_kernels_l2.hip", "brx_kernels_l3.hip", "brx_kernels_l4.hip", "brx_kernels_s.hip", "brx_gen.hip", "brx_util.hip", "brx_tiles.hip", "brx_digest.hip", "brx_index.hip", "brx_index_quoted.hip", "brx_index_escaped.hip", "brx_find.hip", "brx_take.hip", "brx_hash.hip", "brx_parse.hip", "brx_parse_f64.hip", "brx_parse_time.hip", "brx_unescape.hip", "brx_member.hip", "brx_elements.hip", "brx_object.hip", "brx_api.cpp", "brx_node.cpp"]
DEPS = SOURCES + ["brx_device.h", "brx_layout.h", "brx_tiles.h", "brx_digest.h", "brx_index.h", "brx_index_quoted.h", "brx_index_escaped.h", "brx_find.h", "brx_take.h", "brx_record_dev.h", "brx_hash.h", "brx_parse.h", "brx_parse_f64.h", "brx_parse_time.h", "brx_unescape.h", "brx_member.h", "brx_elements.h", "brx_object.h", "brx_pow5.h", "brx_internal.h", "brx_plan.h", "brx_small.h", "brx_hot.S", "brx_lens.S", os.path.join("..", "host", "brx_walk.cpp"), os.path.join("..", "..", "include", "brx.h"),
                  os.path.join("..", "tables", "dictionary.bin"), os.path.join("..", "tables", "context_lut.bin"),
                  os.path.join("..", "tables", "transforms.bin"), os.path.join("..", "tables", "gen_header.bin"), os.path.join("..", "build.py")]


def _stale():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(os.path.join(CSRC, d)) > t for d in DEPS)


def build_library(force=False, verbose=False):
    """Compile csrc/ into brotli-rs_amd/libbrx.so.  Returns the library path.  Safe to call from several processes at
    once (one rank per GPU): the build is serialised by a lock file and the library is replaced atomically."""
    if not force and not _stale():
        return LIB_PATH
    import fcntl
    with open(os.path.join(PKG, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not _stale():  # another process built it while this one waited
            return LIB_PATH
        return _build_locked(verbose)


def _build_locked(verbose):
    if not os.path.exists(HIPCC):
        if os.path.exists(LIB_PATH):
            return LIB_PATH  # GPU box without a need to rebuild: use the prebuilt library that travelled
        raise RuntimeError("hipcc not found at %s and no prebuilt libbrx.so" % HIPCC)
    gen = os.path.join(CSRC, "_gen", "brx_tables_gen.h")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "bin2h.py"), gen, "BRX", "static const"])
    prof = ["-DBRX_PROF"] if os.environ.get("BRX_PROF") == "1" else []  # bring-up: timers inside the loop
    if os.environ.get("BRX_NO_SPEC") == "1":
        prof.append("-DBRX_NO_SPEC")  # A/B: serial symbol fetch instead of the lane-speculative one
    if os.environ.get("BRX_PIN_NOPS"):
        prof.append("-DPIN_NOPS=%d" % int(os.environ["BRX_PIN_NOPS"]))  # A/B: position of the loop (profiles/r03_pins.txt)
    extra = ["-D" + d for d in os.environ.get("BRX_DEFS", "").split()]  # A/B: defines for the loop AND the C++ side
    prof += extra
    # The instances of the kernel (brx_device.h): levels 0 .. 4 and the lean one.  brx_layout.h gives each its LDS offsets.
    instances = [("" if k == 0 else "_l%d" % k, "-DBRX_LEVEL=%d" % k) for k in range(5)] + [("_s", "-DBRX_SMALL")]

    def emit(src, name, defs):  # cpp resolves register names and offsets; the text becomes one asm statement (a raw string)
        txt = subprocess.check_output(["cpp", "-P", "-x", "assembler-with-cpp"] + defs + [os.path.join(CSRC, src)]).decode()
        assert ")BRXASM" not in txt and "%" not in txt and "{" not in txt and "$" not in txt
        if src == "brx_hot.S":
            if "-DBRX_WIN_SGPR" in defs:
                txt = txt.replace(".L", ".LS_")  # both builds land in one assembly file: distinct local labels
            macros = re.findall(r"^\s*\.macro\s+(\w+)", txt, flags=re.M)
            txt += "".join(".purgem %s\n" % m for m in macros)  # ... and macro names free again after each
        else:  # an asm statement WITH operands: `@n@` in the source is operand n, local labels get the statement's unique suffix
            txt = re.sub(r"@(\d+)@", r"%\1", txt).replace(".Lls_", ".Lls%=_")
        with open(os.path.join(CSRC, "_gen", name), "w") as f:
            f.write("// generated from %s by build.py -- do not edit\n" % src)
            f.write('R"BRXASM(\n' + txt + ')BRXASM"\n')

    for suffix, level in instances:
        if suffix != "_s":  # the command loop (the lean instance has a compiled one of its own), in its two builds (brx_hot.S, "Two
            # builds of this file"): bit window in VGPRs (full chip) / in SGPRs (few waves per CU)
            emit("brx_hot.S", "brx_hot_asm%s.h" % suffix, prof + [level])
            emit("brx_hot.S", "brx_hot_asm_sw%s.h" % suffix, prof + [level, "-DBRX_WIN_SGPR"])
        emit("brx_lens.S", "brx_lens_asm%s.h" % suffix, [level])  # the code-length symbol loop of the header path
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-comment"]
    if os.environ.get("BRX_BRINGUP") == "1" or os.environ.get("BRX_PROF") == "1":
        cmd.append("-DBRX_BRINGUP")  # bring-up: BRX_DEBUG_STATS / BRX_DEBUG_STOP=9 + BRX_DEBUG_DUMP (tools/gpu_dumps.sh, tools/span_stats.py)
    cmd += extra + [os.path.join(CSRC, s) for s in SOURCES]
    tmp = "%s.tmp.%d" % (LIB_PATH, os.getpid())
    cmd += ["-ldl", "-lpthread", "-o", tmp]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    os.replace(tmp, LIB_PATH)
    # host program above the C ABI: the reference's file walker (src/main.rs:49-70) on the batched decoder
    walk = os.path.join(PKG, "brx_walk")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(PKG, "host", "brx_walk.cpp"), "-o", walk + ".tmp", "-L", PKG,
                           "-lbrx", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    os.replace(walk + ".tmp", walk)
    return LIB_PATH


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
