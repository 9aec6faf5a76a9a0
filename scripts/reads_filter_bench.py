"""The reads-in-set kernel (mc_reads_in_set_dev) on the environment-assembler-finder's workload: --reads x 150 bp synthetic reads
(configs[1]'s genome, 1 % errors) counted at k, the environment of a 500-base stretch of the genome walked with --maxkmers 100000
(both directions, coverage 2), and every read tested against that environment's k-mers.  At k = 31 and k = 63, HIP events around
every call, warm, the sides in turns, the median of --reps runs.  Prints one JSON line a k:
  filter_ms        the call as the tool makes it (set's table and bit filter built, windows counted, keep decided)
  weak_filter_ms   the same with MC_READS_IN_SET_WEAK_FILTER: no filter in LDS, every window goes to the set's table
  classify_ms      mc_classify_reads_dev on the same reads against the full count table: the nearest existing per-read pass, a
                   yardstick only (it answers another question)

    python scripts/reads_filter_bench.py [--reads 10000000] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENOME_SEED, READ_SEED = 20240531, 42


def run(args, k):
    import numpy as np
    import torch

    import metacherchant_amd as m
    from tests.helpers import seed_windows

    L, n = args.read_len, args.reads
    mode = m.KEY_PACKED if k <= 31 else m.KEY_POLY
    dev = torch.device("cuda", 0)
    windows = n * (L - k + 1)
    hint = int(min(windows, args.contigs * args.contig_len + windows * (1 - (1 - args.err / 1e4) ** k))) + (1 << 20)
    ctx = m.Context(k, mode, 0, hint)
    ctx.set_coverage_hint(2)
    w = torch.empty((n * L + 31) // 32 + 1, dtype=torch.int64, device=dev)
    o = torch.empty(n + 1, dtype=torch.int64, device=dev)
    ctx.synth_reads_dev(GENOME_SEED, args.contigs, args.contig_len, READ_SEED, 0, n, L, args.err, w, o)
    ctx.add_reads_packed_dev(w, o, n, n * L)
    distinct = ctx.finalize()
    seed = m.native.synth_genome(GENOME_SEED, args.contig_len // 2, 500)
    shi, slo = seed_windows(seed, k)
    r = ctx.bfs(shi, slo, 0, 2, max_kmers=args.maxkmers)
    hi, lo = np.ascontiguousarray(r["hi"], dtype=np.uint64), np.ascontiguousarray(r["lo"], dtype=np.uint64)
    n_set = len(lo)
    d_hi = torch.from_numpy(hi.view(np.int64)).to(dev)
    d_lo = torch.from_numpy(lo.view(np.int64)).to(dev)
    d_hits = torch.empty(n, dtype=torch.int32, device=dev)
    d_keep = torch.empty(n, dtype=torch.uint8, device=dev)
    d_cov = torch.empty(n * 12, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def filt():
        m.reads_in_set_dev(ctx, w, o, n, d_hi, d_lo, n_set, d_hits, d_keep, pct=1)

    def weak():
        m.reads_in_set_dev(ctx, w, o, n, d_hi, d_lo, n_set, d_hits, d_keep, pct=1, weak=True)

    def classify():
        ctx.classify_reads_dev(w, o, n, d_cov)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    sides = {"filter": filt, "weak_filter": weak, "classify": classify}
    for f in sides.values():  # warm
        f()
    filt()
    hits_f, kept = d_hits.clone(), int(d_keep.sum())
    weak()
    agree = bool((hits_f == d_hits).all()) and kept == int(d_keep.sum())
    times = {name: [] for name in sides}
    for _ in range(args.reps):  # the sides in turns
        for name, f in sides.items():
            times[name].append(timed(f))
    med = {name: statistics.median(t) for name, t in times.items()}
    out = {"metric": "reads_in_set", "k": k, "reads": n, "read_len": L, "set_kmers": n_set, "filter_ms": round(med["filter"], 3),
           "weak_filter_ms": round(med["weak_filter"], 3), "classify_ms": round(med["classify"], 3),
           "filter_over_weak": round(med["filter"] / med["weak_filter"], 4), "filter_over_classify": round(med["filter"] / med["classify"], 4),
           "ms_all": {name: [round(x, 3) for x in t] for name, t in times.items()}, "answers_agree": agree, "reads_kept": kept,
           "reads_hit": int((hits_f > 0).sum()), "windows_hit": int(hits_f.to(torch.int64).sum()), "distinct_kmers": distinct}
    print(json.dumps(out), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[31, 63])
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--maxkmers", type=int, default=100_000)
    ap.add_argument("--contigs", type=int, default=10)
    ap.add_argument("--contig-len", type=int, default=5_000_000)
    ap.add_argument("--err", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    for k in args.ks:
        run(args, k)


if __name__ == "__main__":
    main()
