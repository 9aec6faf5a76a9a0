"""The triple-reads-classifier's device phases at scale: 10 M pairs x 150 bp (two read seeds of the synthetic genome, as
scripts/classify_bench.py makes them), graphs at k = 31 and k2 = 61 from 10 M reads of a third seed.  Prints one JSON line with the
time of every phase: the two tables, the four probe passes (mc_classify_reads_dev), last_copy per side (mc_reads_last_copy_dev),
the two class launches (mc_triple_classes_dev), and last_copy's estimated sort-traffic floor at the measured copy rate of
MI355X_MICROARCH.md (6.29 TB/s).

    python scripts/triple_classify_bench.py [--pairs 10000000] [--k 31] [--k2 61]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENOME_SEED, GRAPH_SEED, SIDE_SEEDS = 20240531, 42, (4242, 4343)
HBM_BYTES_PER_S = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--k2", type=int, default=61)
    ap.add_argument("--contigs", type=int, default=10)
    ap.add_argument("--contig-len", type=int, default=5_000_000)
    ap.add_argument("--err", type=int, default=100)
    args = ap.parse_args()

    import torch

    import metacherchant_amd as m

    R, L = args.pairs, args.read_len
    dev = torch.device("cuda", 0)
    n_words = (R * L + 31) // 32 + 1
    out = {"metric": "triple_classify", "pairs": R, "read_len": L, "k": args.k, "k2": args.k2}

    def timed(name, f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        out[name] = round((time.perf_counter() - t0) * 1e3, 3)
        return r

    g_words = torch.empty(n_words, dtype=torch.int64, device=dev)
    g_off = torch.empty(R + 1, dtype=torch.int64, device=dev)
    sides = []
    cov = [torch.empty(R * 12, dtype=torch.uint8, device=dev) for _ in range(2)]
    cls1 = [torch.empty(R, dtype=torch.uint8, device=dev) for _ in range(2)]
    cls2 = [torch.empty(R, dtype=torch.uint8, device=dev) for _ in range(2)]
    last = [torch.empty(R, dtype=torch.int32, device=dev) for _ in range(2)]
    for p, k in enumerate((args.k, args.k2)):
        windows = R * (L - k + 1)
        hint = int(min(windows, args.contigs * args.contig_len + windows * (1 - (1 - args.err / 1e4) ** k))) + (1 << 20)
        ctx = m.Context(k, m.KEY_PACKED if k <= 31 else m.KEY_POLY, 0, hint)
        ctx.synth_reads_dev(GENOME_SEED, args.contigs, args.contig_len, GRAPH_SEED, 0, R, L, args.err, g_words, g_off)
        if not sides:
            for seed in SIDE_SEEDS:
                w = torch.empty(n_words, dtype=torch.int64, device=dev)
                o = torch.empty(R + 1, dtype=torch.int64, device=dev)
                ctx.synth_reads_dev(GENOME_SEED, args.contigs, args.contig_len, seed, 0, R, L, args.err, w, o)
                sides.append((w, o))

        def table():
            ctx.add_reads_packed_dev(g_words, g_off, R, R * L)
            return ctx.finalize()
        out["distinct_kmers_%d" % (p + 1)] = timed("table_%d_ms" % (p + 1), table)
        for s in (0, 1):
            timed("probe_%d_side%d_ms" % (p + 1, s + 1), lambda: ctx.classify_reads_dev(sides[s][0], sides[s][1], R, cov[s], None, 90, 1.0, False))
        if p == 0:
            timed("class_1_ms", lambda: ctx.triple_classes_dev(cov[0], cov[1], sides[0][1], sides[1][1], R, cls1[0], cls1[1], 40))
            for s in (0, 1):
                timed("last_copy_side%d_ms" % (s + 1), lambda: ctx.reads_last_copy_dev(sides[s][0], sides[s][1], R, last[s]))
        else:
            timed("class_2_ms", lambda: ctx.triple_classes_dev(cov[0], cov[1], sides[0][1], sides[1][1], R, cls2[0], cls2[1], 40,
                                                               cls1[0], cls1[1], last[0], last[1]))
        ctx.close()
    # last_copy's floor: 8 radix passes over 12-byte (fingerprint, index) pairs read and written, plus the fingerprint and resolve reads
    est = R * (8 * 24 + 2 * (L // 4 + 16))
    out["last_copy_est_bytes"] = est
    out["last_copy_est_floor_ms"] = round(est / HBM_BYTES_PER_S * 1e3, 3)
    for c in range(2):
        counts = torch.bincount(cls2[c].long(), minlength=3).tolist()
        out["classes_side%d" % (c + 1)] = {"not_found": counts[0], "half_found": counts[1], "found": counts[2]}
    out["last_copy_self_fraction"] = float((last[0].cpu() == torch.arange(R, dtype=torch.int32)).double().mean())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
