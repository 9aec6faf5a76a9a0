"""environment-finder-multi, three ways of joining G graph files, wall-clock time of the whole tool (process start, reading the files,
the join, the compaction, writing the five files):
  string  `metacherchant --tool environment-finder-multi --join host`: environment_finder_multi on k-mer strings, the reference's way;
  packed  `mc_hosttest multi-packed`: environment_finder_multi_packed with env_join_host and unitigs_by_links, no GPU;
  gpu     `metacherchant ... --join gpu`: the same with mc_env_join and mc_unitigs, whose device_ms (the DEBUG line of the log) stand
          beside the wall time.
The graph files are cut from one random contig as tests/test_gpu_cli_multi_join.py cuts them (tests/env_join_model.py
contig_environments): G = 4 slices that overlap widely, two of them with a variant, one on the other strand.  The three ways run in
turn, --reps times each after one untimed run of the GPU's way, and must write the same five files.  One JSON line for every k and every
size with the medians and all runs; a last line gives for every k the smallest measured size from which the GPU's way beats the
string path at every larger measured size: what `--join auto` takes its threshold from.

    python scripts/multi_join_bench.py [--entries 10000 100000 1000000] [--k 31 63] [--graphs 4] [--reps 3] [--out DIR]"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILES = ["seqs.fasta", "graph.gfa", "gene.fasta", "Jacard_sym.txt", "Jacard_alt.txt"]


def timed(cmd):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, capture_output=True, text=True)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit("%s failed (%d)" % (" ".join(cmd[:4]), p.returncode))
    return dt, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, nargs="*", default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--k", type=int, nargs="*", default=[31, 63])
    ap.add_argument("--graphs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="directory for the inputs and outputs (default: a temporary one, removed)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    from metacherchant_amd import build
    from tests import env_join_model as M
    build.build_lib()
    cli, hosttest = build.build_host(), build.HOSTTEST
    work = args.out or tempfile.mkdtemp(prefix="multi_join_bench_")
    os.makedirs(work, exist_ok=True)
    crossover, warmed = {}, False
    med = statistics.median
    for k in args.k:
        wins = []
        for n in sorted(args.entries):
            d = os.path.join(work, "k%d_n%d" % (k, n))
            os.makedirs(d, exist_ok=True)
            texts, gene = M.contig_environments(k, args.graphs, n)
            envs = []
            for g, t in enumerate(texts):
                envs.append(os.path.join(d, "env%d.txt" % g))
                with open(envs[-1], "wb") as f:
                    f.write(t)
            seq = os.path.join(d, "gene.fasta")
            with open(seq, "w") as f:
                f.write(">thegene\n%s\n" % gene)
            tool = lambda how: [cli, "--tool", "environment-finder-multi", "--env"] + envs + ["--seq", seq, "-o", os.path.join(d, how), "-w",
                                os.path.join(d, "wd_" + how), "--force", "--join", how, "--device", str(args.device)]
            cmds = {"string": tool("host"), "packed": [hosttest, "multi-packed", os.path.join(d, "packed"), seq, "1"] + envs, "gpu": tool("gpu")}
            if not warmed:
                timed(cmds["gpu"])
                warmed = True
            runs = {w: [] for w in cmds}
            join_ms, unitigs_ms, entries = [], [], None
            for _ in range(args.reps):
                for way, cmd in cmds.items():
                    dt, p = timed(cmd)
                    runs[way].append(round(dt, 4))
                    if way == "gpu":
                        log = open(os.path.join(d, "wd_gpu", "log")).read()
                        m = re.findall(r"mc_env_join ([0-9.]+) ms, mc_unitigs ([0-9.]+) ms", log)[-1]
                        join_ms.append(float(m[0]))
                        unitigs_ms.append(float(m[1]))
                        entries = int(re.findall(r"environments \((\d+) k-mers\) on the GPU", log)[-1])
            same = all(open(os.path.join(d, "host", f), "rb").read() == open(os.path.join(d, w, f), "rb").read() for f in FILES for w in ("packed", "gpu"))
            res = {"k": k, "graphs": args.graphs, "entries": entries, "same_files": same, "string_s": med(runs["string"]), "packed_s": med(runs["packed"]),
                   "gpu_s": med(runs["gpu"]), "env_join_device_ms": med(join_ms), "unitigs_device_ms": med(unitigs_ms), "string_s_all": runs["string"],
                   "packed_s_all": runs["packed"], "gpu_s_all": runs["gpu"]}
            print(json.dumps(res), flush=True)
            if not same:
                raise SystemExit("the three ways wrote different files at k = %d, %d entries" % (k, n))
            wins.append((n, res["gpu_s"] < res["string_s"]))
            if not args.out:
                shutil.rmtree(d)
        at = None
        for n, w in reversed(wins):
            if not w:
                break
            at = n
        crossover[str(k)] = at
    print(json.dumps({"gpu_faster_than_string_from_entries": crossover}), flush=True)
    if not args.out:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
