"""Unitig compaction of one environment, the host's loop against mc_unitigs, both through make_picture (csrc/host/picture.cpp), the
entry every graph-writing tool compacts through: `--compact host` is make_picture without a compactor (the reference's loop on
labels, the parent's code), `--compact gpu` make_picture with mc_unitigs as the compactor (the k-mers split into words and copied up,
the passes, the result copied back and into vectors, the nodes built from it, the loop over the irregular entries).  Both are
wall-clock times around work that ends on the host, taken by mc_unitigs_bench (csrc/host/unitigs_bench.cpp), which also holds the two
ways' alive nodes to be the same.  The environment: k-mers of pieces of --seq-len bases of the synthetic genome (mc_synth_genome),
one chain a piece, in a seeded random order and orientation.

For every k and every number of entries one JSON line: the medians of --reps runs (the two ways in turn, the GPU's after one untimed
run of the same size), all runs beside them, the part of the GPU way spent inside the compactor, mc_unitigs' device_ms and, from
MC_UNITIGS_STATS=1, its passes (set, lists + links, ranks, chains, order, output) as medians.  A last line gives for every k the
smallest measured size from which the GPU way is the faster one: what `--compact auto` takes its threshold from.

    python scripts/unitigs_bench.py [--entries 100000 10000000] [--k 31 63] [--reps 3] [--seq-len 10000] [--skip-host-above N]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PASSES = ("set_ms", "lists_ms", "ranks_ms", "chains_ms", "order_ms", "output_ms")


def run(exe, k, entries, args):
    what = "gpu" if args.skip_host_above and entries > args.skip_host_above else "both"
    env = dict(os.environ, MC_UNITIGS_STATS="1")
    p = subprocess.run([exe, str(k), str(entries), str(args.seq_len), str(args.reps), str(args.device), what], env=env, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit("mc_unitigs_bench failed (%d) at k = %d, %d entries" % (p.returncode, k, entries))
    out = json.loads(p.stdout.strip().splitlines()[-1])
    calls = [dict((name, float(v)) for name, v in re.findall(r"(\w+_ms)=([0-9.]+)", line)) for line in p.stderr.splitlines() if line.startswith("mc_unitigs: n=")]
    calls = calls[1:]  # (the untimed run's)
    assert len(calls) == args.reps, (len(calls), args.reps)
    med = statistics.median
    res = {"k": k, "entries": out["entries"], "alive_nodes": out["alive_nodes"], "same_nodes": out["same_nodes"],
           "host_s": med(out["host_s"]) if out["host_s"] else None, "gpu_s": med(out["gpu_s"]),
           "gpu_compactor_s": med(out["gpu_compactor_s"]), "device_ms": med(out["device_ms"]),
           "passes_ms": {name: med([c[name] for c in calls]) for name in PASSES},
           "host_s_all": out["host_s"], "gpu_s_all": out["gpu_s"], "device_ms_all": out["device_ms"]}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, nargs="*", default=[100_000, 10_000_000])
    ap.add_argument("--k", type=int, nargs="*", default=[31, 63])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seq-len", type=int, default=10_000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--skip-host-above", type=int, default=0, help="no host runs above this many entries (0: always)")
    args = ap.parse_args()
    from metacherchant_amd import build
    build.build_lib()
    exe = build.build_unitigs_bench()
    crossover = {}
    for k in args.k:
        faster = [(r["entries"], r["host_s"] is not None and r["gpu_s"] < r["host_s"]) for r in (run(exe, k, n, args) for n in sorted(args.entries))]
        # the smallest size from which on every measured size the GPU way wins (None: it does not at the largest)
        at = None
        for n, wins in reversed(faster):
            if not wins:
                break
            at = n
        crossover[str(k)] = at
    print(json.dumps({"gpu_faster_from_entries": crossover}), flush=True)


if __name__ == "__main__":
    main()
