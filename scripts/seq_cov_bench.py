"""seq-cov's kernel at configs[1] scale (mc_seq_coverage_dev): four tables of 2.5 M x 150 bp synthetic reads each (configs[1]'s
genome, four read seeds, 1 % errors), then the same 1.5 G query bases in two shapes: (a) 10 M reads of 150 bp, (b) 300 sequences of
5 Mbases.  Prints one JSON line a shape: the median and all call times, windows/s, probes/s and a bytes-over-bandwidth bound -- every
probe one random 16-byte slot read, which costs at least one 64-byte sector, at the copy rate of 6.29 TB/s.
Shape (a) is timed in turns with its baseline, four calls of mc_classify_reads_dev (one a table); shape (b) goes through
mc_classify_reads_dev once, for scale (one wave a sequence).

    python scripts/seq_cov_bench.py [--k 31] [--reads 10000000] [--window-s 1.0] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENOME_SEED, QUERY_SEED = 20240531, 4242
TABLE_SEEDS = (42, 43, 44, 45)
HBM_BYTES_PER_S = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reads", type=int, default=10_000_000, help="query reads of shape (a); shape (b) holds the same bases")
    ap.add_argument("--table-reads", type=int, default=2_500_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--contigs", type=int, default=10)
    ap.add_argument("--contig-len", type=int, default=5_000_000)
    ap.add_argument("--err", type=int, default=100)
    ap.add_argument("--window-s", type=float, default=1.0, help="length of one timed window (calls are repeated to fill it)")
    ap.add_argument("--reps", type=int, default=5, help="timed windows a side")
    ap.add_argument("--skip-slow", action="store_true", help="leave out shape (b) through mc_classify_reads_dev")
    args = ap.parse_args()

    import numpy as np
    import torch

    import metacherchant_amd as m
    from metacherchant_amd import native

    k, L, R, NT = args.k, args.read_len, args.reads, len(TABLE_SEEDS)
    mode = m.KEY_PACKED if k <= 31 else m.KEY_POLY
    dev = torch.device("cuda", 0)

    def reads_dev(ctx, seed, n):
        w = torch.empty((n * L + 31) // 32 + 1, dtype=torch.int64, device=dev)
        o = torch.empty(n + 1, dtype=torch.int64, device=dev)
        ctx.synth_reads_dev(GENOME_SEED, args.contigs, args.contig_len, seed, 0, n, L, args.err, w, o)
        return w, o

    ctxs, distinct = [], []
    for seed in TABLE_SEEDS:
        n = args.table_reads
        windows = n * (L - k + 1)
        hint = int(min(windows, args.contigs * args.contig_len + windows * (1 - (1 - args.err / 1e4) ** k))) + (1 << 20)
        ctx = m.Context(k, mode, 0, hint)
        ctx.set_read_pointers(0)
        w, o = reads_dev(ctx, seed, n)
        ctx.add_reads_packed_dev(w, o, n, n * L)
        distinct.append(ctx.finalize())
        ctx.trim()
        del w, o
        ctxs.append(ctx)
    # shape (a): reads of another seed; shape (b): the same number of bases of the synthetic genome as 5 Mbase sequences
    a_words, a_off = reads_dev(ctxs[0], QUERY_SEED, R)
    seq_len = 5_000_000
    n_long = max(R * L // seq_len, 1)
    genome_len = args.contigs * args.contig_len
    g = native.synth_genome(GENOME_SEED, 0, genome_len)
    codes = np.concatenate([g] * (n_long * seq_len // genome_len + 1))[:n_long * seq_len]
    b_words = torch.from_numpy(ctxs[0]._words(codes, np.array([0, len(codes)], dtype=np.uint64), False).view(np.int64)).to(dev)
    b_off = torch.arange(n_long + 1, dtype=torch.int64, device=dev) * seq_len
    del codes, g
    out_a = torch.empty(R * NT * 2, dtype=torch.int64, device=dev)
    out_b = torch.empty(n_long * NT * 2, dtype=torch.int64, device=dev)
    cls_a = torch.empty(R * 12, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def fused_a():
        m.seq_coverage_dev(ctxs, a_words, a_off, R, out_a)  # (returns with the kernel done)

    def fused_b():
        m.seq_coverage_dev(ctxs, b_words, b_off, n_long, out_b)

    def four_calls_a():
        for c in ctxs:
            c.classify_reads_dev(a_words, a_off, R, cls_a, None, 90, 1.0, False)

    def window(f, calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        return (time.perf_counter() - t0) * 1e3 / calls

    sides = {"fused_reads": fused_a, "fused_contigs": fused_b, "four_classify_calls": four_calls_a}
    calls = {}
    for name, f in sides.items():  # warm-up of every shape, and how many calls fill a window
        f()
        one = window(f, 2)
        calls[name] = max(int(args.window_s * 1e3 / one), 1)
    times = {name: [] for name in sides}
    for _ in range(args.reps):  # the sides in turns
        for name, f in sides.items():
            times[name].append(window(f, calls[name]))
    # the answers of the two ways agree (the classifier's sum is an int that wraps; breadth is its `covered`)
    rec = cls_a.view(R, 12)[:, 4:8].contiguous().view(torch.int32).view(-1).to(torch.int64)
    agree = bool((out_a.view(R, NT, 2)[:, NT - 1, 1] == rec).all())

    win_a = R * (L - k + 1)
    win_b = n_long * (seq_len - k + 1)

    def line(shape, name, windows):
        ms = statistics.median(times[name])
        floor = windows * NT * 64 / HBM_BYTES_PER_S * 1e3
        return {"metric": "seq_coverage", "shape": shape, "k": k, "n_tables": NT, "windows": windows, "ms": round(ms, 3),
                "ms_all": [round(t, 3) for t in times[name]], "calls_a_window": calls[name], "windows_per_s": windows / (ms / 1e3),
                "probes_per_s": windows * NT / (ms / 1e3), "bytes_over_bandwidth_floor_ms": round(floor, 3),
                "frac_of_floor": round(floor / ms, 3), "distinct_kmers": distinct}

    base = times["four_classify_calls"]
    la = line("reads", "fused_reads", win_a)
    la.update({"baseline_four_classify_calls_ms": round(statistics.median(base), 3), "baseline_ms_all": [round(t, 3) for t in base],
               "baseline_spread_ms": round(max(base) - min(base), 3), "fused_over_baseline": round(la["ms"] / statistics.median(base), 3),
               "clears_spread": statistics.median(base) - la["ms"] > max(base) - min(base), "breadth_agrees_with_classify": agree})
    print(json.dumps(la), flush=True)
    lb = line("contigs", "fused_contigs", win_b)
    lb["contigs_over_reads"] = round(lb["ms"] / la["ms"] * win_a / win_b, 4)  # (time a window, shape (b) over shape (a))
    if not args.skip_slow:  # one wave a sequence: one call, for scale
        cls_b = torch.empty(n_long * 12, dtype=torch.uint8, device=dev)
        t0 = time.perf_counter()
        ctxs[0].classify_reads_dev(b_words, b_off, n_long, cls_b, None, 90, 1.0, False)
        lb["classify_one_table_one_call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    print(json.dumps(lb), flush=True)
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    main()
