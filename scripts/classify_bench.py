"""The reads-classifier's kernel at configs[1] scale (mc_classify_reads_dev): the table of 10 M x 150 bp synthetic reads (k = 31,
1 % errors, built as bench.py builds it), then 10 M reads of another read seed classified against it.  Prints one JSON line: the
median call time, reads/s, window probes/s and the HBM estimate -- every window one random 16-byte slot read, which costs at least
one 64-byte sector -- against the measured copy rate of MI355X_MICROARCH.md (6.29 TB/s).

    python scripts/classify_bench.py [--reads 10000000] [--steps 5] [--correction]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENOME_SEED, READ_SEED, QUERY_SEED = 20240531, 42, 4242
HBM_BYTES_PER_S = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--contigs", type=int, default=10)
    ap.add_argument("--contig-len", type=int, default=5_000_000)
    ap.add_argument("--err", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--correction", action="store_true", help="every read gets one low-quality position (the correction path)")
    args = ap.parse_args()

    import torch

    import metacherchant_amd as m

    k, L, R = args.k, args.read_len, args.reads
    dev = torch.device("cuda", 0)
    windows = R * (L - k + 1)
    hint = int(min(windows, args.contigs * args.contig_len + windows * (1 - (1 - args.err / 1e4) ** k))) + (1 << 20)
    ctx = m.Context(k, m.KEY_PACKED if k <= 31 else m.KEY_POLY, 0, hint)
    n_words = (R * L + 31) // 32 + 1
    d_words = torch.empty(n_words, dtype=torch.int64, device=dev)
    d_off = torch.empty(R + 1, dtype=torch.int64, device=dev)
    ctx.synth_reads_dev(GENOME_SEED, args.contigs, args.contig_len, READ_SEED, 0, R, L, args.err, d_words, d_off)
    ctx.add_reads_packed_dev(d_words, d_off, R, R * L)
    n_distinct = ctx.finalize()
    # the second metagenome: reads of the same genome under another read seed
    q_words = torch.empty(n_words, dtype=torch.int64, device=dev)
    q_off = torch.empty(R + 1, dtype=torch.int64, device=dev)
    ctx.synth_reads_dev(GENOME_SEED, args.contigs, args.contig_len, QUERY_SEED, 0, R, L, args.err, q_words, q_off)
    d_out = torch.empty(R * 12, dtype=torch.uint8, device=dev)
    d_bad = torch.full((R,), L // 2, dtype=torch.int32, device=dev) if args.correction else None
    torch.cuda.synchronize()
    ctx.classify_reads_dev(q_words, q_off, R, d_out, d_bad, 90, 1.0, args.correction)  # warm-up
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        ctx.classify_reads_dev(q_words, q_off, R, d_out, d_bad, 90, 1.0, args.correction)  # (returns with the kernel done)
        times.append((time.perf_counter() - t0) * 1e3)
    rec = d_out.view(R, 12).cpu()
    found = int(rec[:, 10].sum())
    ms = statistics.median(times)
    probes = windows + (R * 4 * k if args.correction else 0)  # (upper bound of the correction's look-ups: four substitutions, k windows)
    est_bytes = windows * 64
    print(json.dumps({
        "metric": "classify_reads", "reads": R, "read_len": L, "k": k, "correction": args.correction, "distinct_kmers": n_distinct,
        "ms": round(ms, 3), "ms_all": [round(t, 3) for t in times], "reads_per_s": R / (ms / 1e3), "probes_per_s": windows / (ms / 1e3),
        "probes": windows, "probes_upper_bound": probes, "est_hbm_bytes": est_bytes, "est_floor_ms": round(est_bytes / HBM_BYTES_PER_S * 1e3, 3),
        "frac_of_floor": round(est_bytes / HBM_BYTES_PER_S * 1e3 / ms, 3), "found_fraction": found / R,
        "table_bytes": int(ctx.stats().table_bytes)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
