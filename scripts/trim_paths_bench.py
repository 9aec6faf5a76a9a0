"""The trim of one BFS pass, the host's reverse walk against mc_trim_paths, both as Environment::add_pass runs them
(csrc/host/envfinder.cpp trim_pass): `--trim-on host` is the walk over the pass's hash map and retainAll's removals (the parent's
code); `--trim-on gpu` is mc_trim_paths from host arrays, copies included, and the removals by its mask.  The map is built before
either and is not timed: add_pass builds it anyway.  Both are wall-clock times around work that ends on the host, taken by
mc_trim_paths_bench (csrc/host/trim_paths_bench.cpp), which also holds the two ways' maps to be the same.  The pass: the k-windows of
the synthetic genome with a side arm every --fork-every bases, `last` on the far ends (the walk's shape: long, and a few k-mers wide).

For every k, dir and number of entries one JSON line: the medians of --reps runs (the two ways in turn, the GPU's after one untimed
run of the same size), the spread of each (max - min of its runs), all runs beside them, the time inside mc_trim_paths and its
device_ms.  A last line gives TRIM_AUTO_MIN as csrc/host/cli.h wants it: the smallest measured size from which, at every larger measured
size too, for every k and dir, the GPU way's median is below the host's by more than the host's own spread; null when there is none.

    python scripts/trim_paths_bench.py [--entries 10000 100000 1000000 10000000] [--k 31 63] [--dirs 1 0] [--reps 5] [--fork-every 300]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(exe, k, direction, entries, args):
    p = subprocess.run([exe, str(k), str(entries), str(args.fork_every), str(direction), str(args.reps), str(args.device), "both"],
                       capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit("mc_trim_paths_bench failed (%d) at k = %d, dir = %d, %d entries" % (p.returncode, k, direction, entries))
    out = json.loads(p.stdout.strip().splitlines()[-1])
    med, spread = statistics.median, lambda v: max(v) - min(v)
    res = {"k": k, "dir": direction, "entries": out["entries"], "kept": out["kept"], "same_maps": out["same_maps"],
           "host_s": med(out["host_s"]), "host_spread_s": spread(out["host_s"]), "gpu_s": med(out["gpu_s"]), "gpu_spread_s": spread(out["gpu_s"]),
           "gpu_call_s": med(out["gpu_call_s"]), "device_ms": med(out["device_ms"]),
           "host_s_all": out["host_s"], "gpu_s_all": out["gpu_s"], "device_ms_all": out["device_ms"]}
    res["gpu_wins"] = res["gpu_s"] < res["host_s"] - res["host_spread_s"]
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, nargs="*", default=[10_000, 100_000, 1_000_000, 10_000_000])
    ap.add_argument("--k", type=int, nargs="*", default=[31, 63])
    ap.add_argument("--dirs", type=int, nargs="*", default=[1, 0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fork-every", type=int, default=300)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    from metacherchant_amd import build
    build.build_lib()
    exe = build.build_trim_paths_bench()
    sizes = sorted(args.entries)
    wins = {n: True for n in sizes}
    for n in sizes:  # (the small sizes first: they are done in seconds)
        for k in args.k:
            for d in args.dirs:
                wins[n] = run(exe, k, d, n, args)["gpu_wins"] and wins[n]
    at = None
    for n in reversed(sizes):
        if not wins[n]:
            break
        at = n
    print(json.dumps({"TRIM_AUTO_MIN": at}), flush=True)


if __name__ == "__main__":
    main()
