"""Builds the native parts in-tree: libmcgpu.so (HIP, gfx950) and the C++ host tool.

hipcc cross-compiles without a GPU.  Outputs land in metacherchant_amd/lib/ (git-ignored, but they
travel to the GPU box with the gpurun snapshot).
"""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libmcgpu.so")
CLI = os.path.join(LIBDIR, "metacherchant")

# the library's units (csrc/context.h says what each holds), and the host readers the read-file entry points use
HIP_SOURCES = ["mcgpu.hip", "reads_file.hip", "walk.hip", "group.hip", "classify.hip", "last_copy.hip", "seq_cov.hip", "presence.hip", "reads_in_set.hip", "components.hip", "unitigs.hip", "env_join.hip", "whole_reads.hip", "trim_paths.hip", "kmers_bin.hip", "render_fastq.hip", "walk_order.hip",
               os.path.join("host", "reads_io.cpp")]
# every header under csrc/ makes every object stale (a stale library would travel to the GPU box unnoticed)
HIP_DEPS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join("host", "reads_io.h"), os.path.join("test", "bfs_old_race.h"),
                                                                      os.path.join(ROOT, "include", "mcgpu.h")]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm to build libmcgpu.so)")


MAX_JOBS = 16  # compilers at once, whatever the machine's CPU count says


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)


def _stale(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources if os.path.exists(s))


def build_lib(force=False, verbose=False, variant=None, defines=()):
    """variant/defines: a tuning build next to the product library (lib/libmcgpu_<variant>.so, compiled with the given
    -D flags); MC_LIB=<path> makes native.load() use it (scripts/variants.py)."""
    os.makedirs(LIBDIR, exist_ok=True)
    srcs = [os.path.join(CSRC, s) for s in HIP_SOURCES]
    deps = srcs + [d if os.path.isabs(d) else os.path.join(CSRC, d) for d in HIP_DEPS]
    out = LIB if not variant else os.path.join(LIBDIR, "libmcgpu_%s.so" % variant)
    if not force and not _stale(out, deps):
        return out
    # one hipcc -c per unit, side by side, into an object directory of this library's own; then one link
    objdir = os.path.join(LIBDIR, "obj_" + os.path.splitext(os.path.basename(out))[0])
    os.makedirs(objdir, exist_ok=True)
    objs = [os.path.join(objdir, os.path.splitext(os.path.basename(s))[0] + ".o") for s in srcs]
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include")]
    cmds = [[_hipcc(), "-c"] + flags + ["-D" + d for d in defines] + ["-o", o, s] for s, o in zip(srcs, objs)]
    with ThreadPoolExecutor(min(len(cmds), MAX_JOBS)) as ex:
        list(ex.map(lambda c: _run(c, verbose), cmds))
    _run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs + ["-lz", "-ldl"], verbose)
    return out


def code_objects(lib, outdir):
    """Paths of every gfx950 code object inside a library, written to outdir.  .hip_fatbin holds one offload bundle per unit, one
    behind the other, and clang-offload-bundler reads only the first: the section is cut at every bundle's magic and each piece
    unbundled on its own."""
    llvm = "/opt/rocm/lib/llvm/bin"
    fat = os.path.join(outdir, "fatbin")
    subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(outdir, "stripped.so")])
    with open(fat, "rb") as f:
        data = f.read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts, i = [], data.find(magic)
    while i >= 0:
        starts.append(i)
        i = data.find(magic, i + 1)
    cos = []
    for n, (a, b) in enumerate(zip(starts, starts[1:] + [len(data)])):
        piece, co = os.path.join(outdir, "bundle%d" % n), os.path.join(outdir, "unit%d.co" % n)
        with open(piece, "wb") as f:
            f.write(data[a:b])
        subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + piece,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        cos.append(co)
    return cos


HOSTTEST = os.path.join(LIBDIR, "mc_hosttest")
HOSTDIR = os.path.join(CSRC, "host")
HOST_FLAGS = ["-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include")]


# what every host program is made of beside its own units: the readers of read files (the library's too), the replay of the JDK, the
# picture of a subgraph, environment-finder's host side and environment-finder-multi's
HOST_CORE = ["reads_io", "java_replay", "picture", "envfinder", "multi"]


def _host_sources(suffix):
    return sorted(os.path.join(HOSTDIR, f) for f in os.listdir(HOSTDIR) if f.endswith(suffix))


def _hosttest_inputs():
    """(sources, headers) of mc_hosttest: the CPU-only program, plain or under a sanitizer"""
    srcs = [os.path.join(HOSTDIR, u + ".cpp") for u in ["hosttest"] + HOST_CORE]
    return srcs, _host_sources(".h") + [os.path.join(ROOT, "include", "mcgpu.h")] + [os.path.join(CSRC, h) for h in ("kmer_hash.h", "read_ptr.h", "switches.h")]


def _link_host(out, units, force, verbose):
    """A host program of csrc/host/<units>.cpp + HOST_CORE against libmcgpu.so and HIP's host API (no device code).  Any host
    header, any of its units or the library newer than the program rebuilds it; several units compile side by side into lib/obj_<name>."""
    srcs = [os.path.join(HOSTDIR, u + ".cpp") for u in units + HOST_CORE]
    if not force and not _stale(out, srcs + _host_sources(".h") + [os.path.join(ROOT, "include", "mcgpu.h"), LIB]):
        return out
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(_hipcc())))
    flags = HOST_FLAGS + ["-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(rocm, "include")]
    if len(units) > 1:
        objdir = os.path.join(LIBDIR, "obj_" + os.path.basename(out))
        os.makedirs(objdir, exist_ok=True)
        objs = [os.path.join(objdir, os.path.splitext(os.path.basename(s))[0] + ".o") for s in srcs]
        with ThreadPoolExecutor(min(len(srcs), MAX_JOBS)) as ex:
            list(ex.map(lambda so: _run(["g++", "-c"] + flags + ["-o", so[1], so[0]], verbose), zip(srcs, objs)))
        srcs = objs
    _run(["g++"] + flags + ["-o", out] + srcs + ["-L", LIBDIR, "-lmcgpu", "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath,$ORIGIN",
                                                 "-Wl,-rpath," + os.path.join(rocm, "lib"), "-lpthread", "-lz", "-ldl"], verbose)
    return out


# the CLI's units (csrc/host/main.cpp says what each holds)
CLI_UNITS = ["main", "options", "cli", "tool_kmer_counter", "tool_multi", "tool_classifiers", "tool_seq_cov", "tool_visualisers",
             "tool_assembler_finder", "tool_environment_finder"]


def build_host(force=False, verbose=False):
    """C++ host side: the `metacherchant` CLI (links libmcgpu.so) and the CPU-only `mc_hosttest`."""
    os.makedirs(LIBDIR, exist_ok=True)
    srcs, hdrs = _hosttest_inputs()
    if force or _stale(HOSTTEST, srcs + hdrs):
        _run(["g++"] + HOST_FLAGS + ["-o", HOSTTEST] + srcs + ["-lz", "-ldl"], verbose)
    if os.path.exists(LIB):
        # (the CLI keeps the triple-reads-classifier's reads on the device itself: HIP's host API, no device code)
        _link_host(CLI, CLI_UNITS, force, verbose)
    return CLI


UNITIGS_BENCH = os.path.join(LIBDIR, "mc_unitigs_bench")
TRIM_PATHS_BENCH = os.path.join(LIBDIR, "mc_trim_paths_bench")
WHOLE_READS_BENCH = os.path.join(LIBDIR, "mc_whole_reads_bench")
WALK_ORDER_BENCH = os.path.join(LIBDIR, "mc_walk_order_bench")


def build_unitigs_bench(force=False, verbose=False):
    """mc_unitigs_bench (csrc/host/unitigs_bench.cpp): make_picture with and without mc_unitigs, timed; scripts/unitigs_bench.py runs it"""
    return _link_host(UNITIGS_BENCH, ["unitigs_bench"], force, verbose)


def build_trim_paths_bench(force=False, verbose=False):
    """mc_trim_paths_bench (csrc/host/trim_paths_bench.cpp): the trim of one pass, the host's walk against mc_trim_paths, timed;
    scripts/trim_paths_bench.py runs it"""
    return _link_host(TRIM_PATHS_BENCH, ["trim_paths_bench"], force, verbose)


def build_walk_order_bench(force=False, verbose=False):
    """mc_walk_order_bench (csrc/host/walk_order_bench.cpp): the walk order of one component, the host's replay against mc_walk_order, timed;
    scripts/walk_order_bench.py runs it"""
    return _link_host(WALK_ORDER_BENCH, ["walk_order_bench"], force, verbose)


def build_whole_reads_bench(force=False, verbose=False):
    """mc_whole_reads_bench (csrc/host/whole_reads_bench.cpp): the reader stage of the classifying tools, host against device, timed;
    scripts/whole_reads_bench.py runs it"""
    return _link_host(WHOLE_READS_BENCH, ["whole_reads_bench"], force, verbose)


def build_host_sanitized(kind, force=False, verbose=False):
    """mc_hosttest under a CPU sanitizer (kind: "asan" = address + undefined behaviour, "tsan" = threads): the host code --
    readers on several threads, the replay of java.util.HashMap with its tree bins, compaction, writers -- run by
    tests/test_host_sanitizers.py.  (No GPU sanitizer runs on this pool; the HIP side has the device self-check instead.)"""
    os.makedirs(LIBDIR, exist_ok=True)
    out = os.path.join(LIBDIR, "mc_hosttest_" + kind)
    srcs, hdrs = _hosttest_inputs()
    san = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tsan": ["-fsanitize=thread"]}[kind]
    if force or _stale(out, srcs + hdrs):
        cmd = ["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include")] + san + [
            "-o", out] + srcs + ["-lz", "-ldl", "-lpthread"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return out


# Tuning builds the GPU tests and scripts load with MC_LIB.  `fuzz` (the walk with a pause behind every barrier) is what the
# gating test of tests/test_gpu_bfs_race.py runs: build_all makes it beside the product library.  The others are made when
# somebody asks for them (build_variant): `fuzz_old` = round 3's racy walk fuzzed the same way (the opt-in half of that test,
# MC_RUN_OLD_RACE=1), `trace_old` and `sctime` what scripts/gpu_bfs_hunt.sh and scripts/gpu_r4_bfs.sh load.
VARIANTS = {
    "fuzz": ("MC_BFS_FUZZ", "MC_BFS_TRACE"),
    "fuzz_old": ("MC_BFS_FUZZ", "MC_BFS_TRACE", "MC_BFS_OLD_RACE"),
    "trace_old": ("MC_BFS_TRACE", "MC_BFS_OLD_RACE"),
    "sctime": ("MC_SCOUT_TIMING",),
}
DEFAULT_VARIANTS = ("fuzz",)


def build_variant(name, force=False, verbose=False):
    """lib/libmcgpu_<name>.so for a name of VARIANTS (a minute of hipcc when it is missing or stale)"""
    return build_lib(force, verbose, variant=name, defines=VARIANTS[name])


def build_variants(force=False, verbose=False, names=DEFAULT_VARIANTS):
    with ThreadPoolExecutor(max(len(names), 1)) as ex:
        return list(ex.map(lambda n: build_variant(n, force, verbose), names))


def build_all(force=False, verbose=False):
    with ThreadPoolExecutor(2) as ex:  # (the product and the fuzzed walk side by side)
        v = ex.submit(build_variants, force, verbose)
        build_lib(force, verbose)
        v.result()
    build_host(force, verbose)


if __name__ == "__main__":
    build_all(force=True, verbose=True)
