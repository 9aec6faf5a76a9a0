"""The presence kernel (mc_kmer_presence_dev) against the only way to the same answer without it: keys through mc_kmer_keys (on the
host, then copied up), four mc_get_dev calls, and the four columns folded into a mask.  Four tables of --table-reads x 150 bp synthetic
reads each (configs[1]'s genome, four read seeds, 1 % errors), at k = 31 and k = 63; 10^6 query k-mers, half of them windows of reads
of another seed, half random.  HIP events around every call, warm, the sides in turns, the median of --reps runs.  Prints one JSON
line a k.  `lookups_only`: the four mc_get_dev calls alone, with the keys already on the device (what is left of the old way
when the caller keeps the keys).

    python scripts/presence_bench.py [--table-reads 10000000] [--queries 1000000] [--reps 9]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENOME_SEED, QUERY_SEED = 20240531, 4242
TABLE_SEEDS = (42, 43, 44, 45)


def run(args, k):
    import numpy as np
    import torch

    import metacherchant_amd as m

    L, NT, Q = args.read_len, len(TABLE_SEEDS), args.queries
    mode = m.KEY_PACKED if k <= 31 else m.KEY_POLY
    dev = torch.device("cuda", 0)
    ctxs, distinct = [], []
    for seed in TABLE_SEEDS:
        n = args.table_reads
        windows = n * (L - k + 1)
        hint = int(min(windows, args.contigs * args.contig_len + windows * (1 - (1 - args.err / 1e4) ** k))) + (1 << 20)
        ctx = m.Context(k, mode, 0, hint)
        ctx.set_read_pointers(0)
        w = torch.empty((n * L + 31) // 32 + 1, dtype=torch.int64, device=dev)
        o = torch.empty(n + 1, dtype=torch.int64, device=dev)
        ctx.synth_reads_dev(GENOME_SEED, args.contigs, args.contig_len, seed, 0, n, L, args.err, w, o)
        ctx.add_reads_packed_dev(w, o, n, n * L)
        distinct.append(ctx.finalize())
        ctx.trim()
        del w, o
        ctxs.append(ctx)
    # the queries: one window of each of Q / 2 reads of another seed, and Q / 2 random k-mers
    nq = Q // 2
    w = torch.empty((nq * L + 31) // 32 + 1, dtype=torch.int64, device=dev)
    o = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    ctxs[0].synth_reads_dev(GENOME_SEED, args.contigs, args.contig_len, QUERY_SEED, 0, nq, L, args.err, w, o)
    words = w.cpu().numpy().view(np.uint64)
    del w, o
    rng = np.random.default_rng(k)
    mask = (1 << (2 * k)) - 1
    vals = []
    for r in range(nq):
        p = r * L + int(rng.integers(0, L - k + 1))
        v = 0
        for wi in range(p // 32, (p + k + 31) // 32 + 1):
            v = (v << 64) | int(words[wi])
        n_words = (p + k + 31) // 32 + 1 - p // 32
        vals.append((v >> (64 * n_words - 2 * (p % 32) - 2 * k)) & mask)
    vals += [int.from_bytes(rng.bytes(16), "little") & mask for _ in range(Q - nq)]
    hi = np.array([v >> 64 for v in vals], dtype=np.uint64)
    lo = np.array([v & 0xFFFFFFFFFFFFFFFF for v in vals], dtype=np.uint64)
    d_hi = torch.from_numpy(hi.view(np.int64)).to(dev)
    d_lo = torch.from_numpy(lo.view(np.int64)).to(dev)
    d_mask = torch.empty(Q, dtype=torch.uint8, device=dev)
    d_keys = torch.empty(Q, dtype=torch.int64, device=dev)
    d_cnt = torch.empty((NT, Q), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()

    def fused():
        m.kmer_presence_dev(ctxs, d_hi, d_lo, Q, d_mask)

    def lookups_only():
        for t, c in enumerate(ctxs):
            c.get_dev(d_keys, Q, d_cnt[t])

    def old_way():
        keys = ctxs[0].kmer_keys(hi, lo)
        d_keys.copy_(torch.from_numpy(keys))
        lookups_only()
        old_mask = ((d_cnt != -1).to(torch.uint8) << torch.arange(NT, dtype=torch.uint8, device=dev)[:, None]).sum(0, dtype=torch.uint8)
        return old_mask

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    sides = {"fused": fused, "old_way": old_way, "lookups_only": lookups_only}
    for f in sides.values():  # warm
        f()
    d_mask.fill_(0xEE)
    fused()
    agree = bool((old_way() == d_mask).all())
    times = {name: [] for name in sides}
    for _ in range(args.reps):  # the sides in turns
        for name, f in sides.items():
            times[name].append(timed(f))
    med = {name: statistics.median(t) for name, t in times.items()}
    hist = torch.bincount(d_mask.to(torch.int64), minlength=16).tolist()
    out = {"metric": "kmer_presence", "k": k, "n_tables": NT, "queries": Q, "fused_ms": round(med["fused"], 4),
           "old_way_ms": round(med["old_way"], 4), "lookups_only_ms": round(med["lookups_only"], 4),
           "fused_over_old_way": round(med["fused"] / med["old_way"], 4), "fused_over_lookups_only": round(med["fused"] / med["lookups_only"], 4),
           "ms_all": {name: [round(x, 4) for x in t] for name, t in times.items()}, "answers_agree": agree, "mask_histogram": hist,
           "distinct_kmers": distinct}
    print(json.dumps(out), flush=True)
    for c in ctxs:
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[31, 63])
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--table-reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--contigs", type=int, default=10)
    ap.add_argument("--contig-len", type=int, default=5_000_000)
    ap.add_argument("--err", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    for k in args.ks:
        run(args, k)


if __name__ == "__main__":
    main()
