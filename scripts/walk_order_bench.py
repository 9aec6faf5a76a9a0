"""The walk order of one component, the host's replay of the reference's queue against mc_walk_order, both as the fmt-visualizer runs
them (csrc/host/tool_visualisers.cpp): `--replay host` is replay_component_walk over the component's sorted k-mers (the parent's
code); `--replay gpu` is mc_walk_order from host arrays, copies included, and the puts made from its answer.  Both are wall-clock
times around work that ends on the host, taken by mc_walk_order_bench (csrc/host/walk_order_bench.cpp), which also holds the two
ways' puts to leave the same map.  Two kinds of component: (a) the k-windows of the synthetic genome, what error-free reads give, a
thin chain; (b) the same with a copy that has a substitution every --error-every bases, what reads with errors give, bubbles in a
row: there the host runs with `--replay auto`'s cap and is expected to be abandoned, which is reported in place of a time.

For every kind, k and size one JSON line: the medians of --reps runs (the two ways in turn, the GPU's after one untimed run of the
same size), the spread of each (max - min of its runs), device_ms, levels, wide_levels, queue_entries.  A last line gives
REPLAY_AUTO_MIN as csrc/host/cli.h wants it: the smallest measured size of kind (a) from which, at every larger measured size too and
for every k, the GPU way's median is below the host's by more than the host's own spread; null ("never") when there is none.

    python scripts/walk_order_bench.py [--kmers 10000 100000 1000000 10000000] [--k 31 63] [--reps 5] [--error-every 200]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(exe, k, kmers, error_every, args):
    p = subprocess.run([exe, str(k), str(kmers), str(error_every), str(args.reps), str(args.device), "both"], capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit("mc_walk_order_bench failed (%d) at k = %d, %d k-mers, error_every = %d" % (p.returncode, k, kmers, error_every))
    out = json.loads(p.stdout.strip().splitlines()[-1])
    med, spread = statistics.median, lambda v: max(v) - min(v)
    res = {"kind": "b" if error_every else "a", "k": k, "members": out["members"], "reached": out["reached"], "same_puts": out["same_puts"],
           "host_abandoned": out["host_abandoned"], "host_s": med(out["host_s"]) if out["host_s"] else None,
           "host_spread_s": spread(out["host_s"]) if out["host_s"] else None, "gpu_s": med(out["gpu_s"]), "gpu_spread_s": spread(out["gpu_s"]),
           "device_ms": med(out["device_ms"]), "levels": out["levels"], "wide_levels": out["wide_levels"], "queue_entries": out["queue_entries"],
           "host_s_all": out["host_s"], "gpu_s_all": out["gpu_s"]}
    res["gpu_wins"] = res["host_s"] is not None and res["gpu_s"] < res["host_s"] - res["host_spread_s"]
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kmers", type=int, nargs="*", default=[10_000, 100_000, 1_000_000, 10_000_000])
    ap.add_argument("--k", type=int, nargs="*", default=[31, 63])
    ap.add_argument("--kinds", nargs="*", default=["a", "b"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--error-every", type=int, default=200)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    from metacherchant_amd import build
    build.build_lib()
    exe = build.build_walk_order_bench()
    sizes = sorted(args.kmers)
    wins = {n: True for n in sizes}
    for n in sizes:  # (the small sizes first: they are done in seconds)
        for k in args.k:
            if "a" in args.kinds:
                wins[n] = run(exe, k, n, 0, args)["gpu_wins"] and wins[n]
            if "b" in args.kinds:
                run(exe, k, n, args.error_every, args)
    at = None
    for n in reversed(sizes):
        if not wins[n]:
            break
        at = n
    print(json.dumps({"REPLAY_AUTO_MIN": at if "a" in args.kinds else None, "sizes": sizes}))


if __name__ == "__main__":
    main()
