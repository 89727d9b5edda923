"""Build recipe for the native parts (run by __graft_entry__.build()).

  libminivideo.so        product: host front end (C++) + HIP kernels, gfx950 only
  liboracle_recon.so     checker (oracle/, plain C) -- test infrastructure
  libmvgen.so            synthetic-stream generator -- test/bench infrastructure

Everything is built in-tree so the shared objects travel with the repository
snapshot to the GPU box.
"""
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "minivideo_amd")
CSRC = os.path.join(PKG, "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

LIB = os.path.join(PKG, "libminivideo.so")
GEN = os.path.join(PKG, "libmvgen.so")
ORACLE = os.path.join(ROOT, "oracle", "liboracle_recon.so")


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


COMMANDS = []   # every compiler / linker command this process has run (build_report())


def _run(cmd):
    print("+", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    COMMANDS.append(cmd)


def build_product(force=False):
    hip_src = sorted(glob.glob(os.path.join(CSRC, "hip", "*.hip")))
    host_src = sorted(glob.glob(os.path.join(CSRC, "host", "*.cpp")))
    hdrs = (glob.glob(os.path.join(CSRC, "*", "*.h")) + glob.glob(os.path.join(CSRC, "*", "*.hpp"))
            + glob.glob(os.path.join(CSRC, "*", "*.inc")) + glob.glob(os.path.join(ROOT, "include", "*.h")))
    checker = os.path.join(ROOT, "tools", "check_prefetch_hazard.py")
    if not force and not _newer(LIB, hip_src + host_src + hdrs + [checker]):
        return LIB
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(CSRC, "hip"), "-I" + os.path.join(CSRC, "host")]
    objdir = os.path.join(PKG, "build")
    os.makedirs(objdir, exist_ok=True)
    objs = []
    for s in host_src:  # host C++ is compiled on its own: mixing `-x c++` inputs into the hipcc line loses --offload-arch
        o = os.path.join(objdir, os.path.basename(s)[:-4] + ".o")
        if force or _newer(o, [s] + hdrs):
            # (-O3: the entropy decoders measure 3 % (CAVLC) / 2.5 % (CABAC) faster than at -O2; -march=x86-64-v3 and a
            #  profile-guided build were tried too: -2.5 % / +3 % and -0.5 % / +2.4 % -- not worth a CPU floor or a training run)
            _run(["g++", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-pthread", "-c", s, "-o", o] + inc)
        objs.append(o)
    # The batch kernels keep their record prefetch in registers that only inline assembly names: check, on the ISA of
    # THE compile whose object is linked (-save-temps=obj keeps its .s), that the compiler's code stays off them while
    # loads are in flight and that the hand-padded hazards are in place (tools/check_prefetch_hazard.py).
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_prefetch_hazard
    checked = ("recon_quad", "recon_oct")
    # per-file device flags.  LLVM's "max-ilp" scheduling strategy (instead of the default, which weighs occupancy first): measured
    # per kernel file on the same buffers (profiles/r04n_ab6.log, r04n_ab7.log): recon_oct -1.1 % (High) / -0.9 % (Baseline),
    # recon_pipe -1.7 ... -2.6 %; recon_kernels +1 %, recon_pipe1 +37 % (more registers, fewer waves) and recon_quad does not pass
    # the register check with it -- those keep the default.  (-Xarch_device: the host pass of hipcc does not know the option.)
    extra_flags = {"recon_oct": ["-Xarch_device", "-mllvm=-amdgpu-sched-strategy=max-ilp"],
                   "recon_pipe": ["-Xarch_device", "-mllvm=-amdgpu-sched-strategy=max-ilp"]}
    for s in hip_src:   # device + host objects of the kernels, gfx950 only
        base = os.path.basename(s)[:-4]
        o = os.path.join(objdir, base + ".hip.o")
        tmpd = os.path.join(objdir, "temps_" + base)
        asm = os.path.join(tmpd, base + "-hip-amdgcn-amd-amdhsa-gfx950.s")
        need_asm = base in checked
        # (the checked objects also depend on the checker's rules: a changed rule re-checks objects already built)
        deps = [s] + hdrs + ([check_prefetch_hazard.__file__] if need_asm else [])
        if force or _newer(o, deps) or (need_asm and not os.path.exists(asm)):
            cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wno-unused-value"] + extra_flags.get(base, [])
            if need_asm:
                os.makedirs(tmpd, exist_ok=True)
                o_tmp = os.path.join(tmpd, base + ".hip.o")
                _run(cmd + ["-save-temps=obj", "-c", s, "-o", o_tmp] + inc)
                check_prefetch_hazard.main(asm)   # raises HazardError: the object is not installed then
                os.replace(o_tmp, o)
            else:
                _run(cmd + ["-c", s, "-o", o] + inc)
        objs.append(o)
    _run([HIPCC, "--offload-arch=gfx950", "--hip-link", "-shared", "-fPIC", "-pthread", "-o", LIB] + objs)
    blob = open(LIB, "rb").read()
    if b"amdgcn-amd-amdhsa--gfx950" not in blob:
        os.remove(LIB)
        raise RuntimeError("libminivideo.so was built without a gfx950 code object")
    return LIB


def build_generator(force=False):
    src = sorted(glob.glob(os.path.join(CSRC, "gen", "*.cpp")))
    if not src:
        return None
    hdrs = glob.glob(os.path.join(CSRC, "*", "*.h")) + glob.glob(os.path.join(CSRC, "*", "*.inc"))
    if not force and not _newer(GEN, src + hdrs):
        return GEN
    _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden",
          "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(CSRC, "host"), "-o", GEN] + src)
    return GEN


def build_oracle(force=False):
    src = [os.path.join(ROOT, "oracle", "recon_ref.c"), os.path.join(ROOT, "include", "minivideo_hotpath.h")]
    if not force and not _newer(ORACLE, src):
        return ORACLE
    _run(["make", "-C", os.path.join(ROOT, "oracle"), "-B", "liboracle_recon.so"])
    return ORACLE


STOCK_CLI = os.path.join(ROOT, "oracle", "_ref", "mini_thumbnailer_stock")
STOCK_MAIN = os.path.join("mini_thumbnailer", "src", "main.cpp")


def reference_dir():
    """the upstream MiniVideo checkout, if there is one: $MINIVIDEO_REFERENCE, else the `reference_path` BASELINE.json
    records, else reference/ beside this repository or in the home directory"""
    import json
    try:
        recorded = json.load(open(os.path.join(ROOT, "BASELINE.json"))).get("reference_path")
    except (OSError, ValueError):
        recorded = None
    for d in (os.environ.get("MINIVIDEO_REFERENCE"), recorded, os.path.join(os.path.dirname(ROOT), "reference"),
              os.path.expanduser(os.path.join("~", "reference"))):
        if d and os.path.exists(os.path.join(d, STOCK_MAIN)):
            return os.path.abspath(d)
    return None


def build_stock_cli(force=False):
    """The reference's own mini_thumbnailer front end, built unchanged against include/minivideo.h (oracle/Makefile).  Only
    where the upstream sources are present; elsewhere a binary that came with the tree is kept as it is."""
    ref = reference_dir()
    if ref is None:
        return STOCK_CLI if os.path.exists(STOCK_CLI) else None
    if not force and not _newer(STOCK_CLI, [os.path.join(ref, STOCK_MAIN), os.path.join(ROOT, "include", "minivideo.h"), LIB]):
        return STOCK_CLI
    _run(["make", "-C", os.path.join(ROOT, "oracle"), "-B", "REFERENCE=" + ref, "_ref/mini_thumbnailer_stock"])
    return STOCK_CLI


REF_CLI = os.path.join(ROOT, "oracle", "_ref", "mini_thumbnailer_ref")


def build_reference_cli(force=False):
    """The reference decoder itself: upstream minivideo/ as a static archive + upstream mini_thumbnailer/src/main.cpp
    (oracle/Makefile), the expected value of tests/test_reference_diff.py and tests/test_gpu_reference_diff.py.  Only where
    the upstream sources are present; elsewhere a binary that came with the tree is kept as it is."""
    ref = reference_dir()
    if ref is None:
        return REF_CLI if os.path.exists(REF_CLI) else None
    srcs = [os.path.join(ref, STOCK_MAIN), os.path.join(ref, "minivideo", "CMakeLists.txt"),
            os.path.join(ROOT, "oracle", "Makefile")]
    if not force and not _newer(REF_CLI, srcs):
        return REF_CLI
    try:   # (needs cmake; without it the reference tests skip, saying how to build the tool, and the recorded digests stand in)
        _run(["make", "-C", os.path.join(ROOT, "oracle"), "-B", "REFERENCE=" + ref, "_ref/mini_thumbnailer_ref"])
    except (OSError, subprocess.CalledProcessError) as e:
        print("build: the reference decoder was not built (%s)" % e, flush=True)
        return None
    return REF_CLI


CLI = os.path.join(PKG, "mini_thumbnailer")


def build_cli(force=False):
    src = [os.path.join(ROOT, "tools", "mini_thumbnailer.cpp")]
    if not force and not _newer(CLI, src + [LIB, os.path.join(ROOT, "include", "minivideo.h")]):
        return CLI
    _run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src[0], "-L" + PKG, "-lminivideo",
          "-Wl,-rpath,$ORIGIN", "-o", CLI])
    return CLI


def build_all(force=False):
    build_product(force)
    build_cli(force)
    build_generator(force)
    build_oracle(force)
    build_stock_cli(force)
    build_reference_cli(force)
    return build_report(force)


def build_report(force=False):
    """what this process's build did: compiled (how many commands) or reused the binaries in the tree"""
    return {"build_mode": "forced rebuild" if force else "incremental (only what is older than its sources)",
            "build_exercised": len(COMMANDS) > 0, "commands_run": len(COMMANDS),
            "hip_objects_compiled": sum(1 for c in COMMANDS if "--offload-arch=gfx950" in c and "-c" in c),
            "artifacts": [os.path.relpath(p, ROOT) for p in (LIB, CLI, GEN, ORACLE, STOCK_CLI, REF_CLI) if os.path.exists(p)]}


if __name__ == "__main__":
    build_all(force="--force" in sys.argv)
