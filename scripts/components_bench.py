"""mc_components_dev on configs[1]'s reads (--reads x 150 bp synthetic reads, 1 % errors) at k = 31 and k = 63: the call's device_ms, the
median of --reps calls after a warm one.  Beside it the only like-for-like figure there is without the call: the table's keys through
mc_export (export_s includes the sort of the keys in Context.export), then a host pass over the same keys.  That pass is numpy label
propagation, not a union-find with path compression: the eight neighbours of every canonical k-mer looked up in the sorted keys, labels
lowered along the edges and jumped until none changes.  It counts the components of ALL keys of the table (host_components), those
that no window holds too, so it is not n_components.  It needs the k-mers' bases, which only packed keys carry: at k = 63 (polynomial
hashes) it reports the export alone.  Prints one JSON line a k.  No threshold is set anywhere.

    python scripts/components_bench.py [--reads 10000000] [--reps 5] [--skip-host]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENOME_SEED, READ_SEED = 20240531, 42


def host_components(keys, k):
    """connected components of the packed canonical k-mers `keys` (sorted int64): their number"""
    import numpy as np
    keys = keys.astype(np.uint64)
    n, mask = len(keys), np.uint64((1 << (2 * k)) - 1)

    def rc(x):
        r = np.zeros_like(x)
        y = x.copy()
        for _ in range(k):
            r = (r << np.uint64(2)) | (np.uint64(3) - (y & np.uint64(3)))
            y >>= np.uint64(2)
        return r

    label = np.arange(n, dtype=np.int64)
    edges = []
    for c in range(4):  # right neighbours of the k-mer and of its reverse complement: all eight allNeighbors, as canonical keys
        for v in (keys, rc(keys)):
            nb = ((v << np.uint64(2)) | np.uint64(c)) & mask
            nb = np.minimum(nb, rc(nb))
            at = np.searchsorted(keys, nb)
            at[at >= n] = 0
            hit = keys[at] == nb
            edges.append((np.nonzero(hit)[0], at[hit]))
    while True:
        before = label.copy()
        for a, b in edges:
            m = np.minimum(label[a], label[b])
            np.minimum.at(label, a, m)
            np.minimum.at(label, b, m)
        label = label[label]
        if np.array_equal(before, label):
            break
    return int((label == np.arange(n)).sum())


def run(args, k):
    import torch

    import metacherchant_amd as m

    L, n = args.read_len, args.reads
    mode = m.KEY_PACKED if k <= 31 else m.KEY_POLY
    dev = torch.device("cuda", 0)
    windows = n * (L - k + 1)
    hint = int(min(windows, args.contigs * args.contig_len + windows * (1 - (1 - args.err / 1e4) ** k))) + (1 << 20)
    ctx = m.Context(k, mode, 0, hint)
    ctx.set_read_pointers(0)
    w = torch.empty((n * L + 31) // 32 + 1, dtype=torch.int64, device=dev)
    o = torch.empty(n + 1, dtype=torch.int64, device=dev)
    ctx.synth_reads_dev(GENOME_SEED, args.contigs, args.contig_len, READ_SEED, 0, n, L, args.err, w, o)
    ctx.add_reads_packed_dev(w, o, n, n * L)
    distinct = ctx.finalize()
    ctx.trim()
    torch.cuda.synchronize()
    ms, res = [], None
    for i in range(args.reps + 1):
        res = m.components_dev(ctx, w, o, n)
        if i:
            ms.append(res["device_ms"])
    out = {"k": k, "reads": n, "windows": windows, "distinct_kmers": distinct, "n_components": res["n_components"], "n_kmers": res["n_kmers"],
           "largest_component": int((res["comp_offsets"][1:] - res["comp_offsets"][:-1]).max()) if res["n_components"] else 0,
           "components_device_ms": statistics.median(ms), "components_device_ms_all": ms}
    if not args.skip_host:
        t0 = time.perf_counter()
        keys, _ = ctx.export(1)
        out["export_s"] = time.perf_counter() - t0
        if mode == m.KEY_PACKED:
            t0 = time.perf_counter()
            out["host_components"] = host_components(keys, k)
            out["host_union_find_s"] = time.perf_counter() - t0
        else:
            out["host_union_find_s"] = None  # (hash keys carry no bases: the host has nothing to take neighbours of)
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--contigs", type=int, default=10)
    ap.add_argument("--contig-len", type=int, default=5_000_000)
    ap.add_argument("--err", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, nargs="*", default=[31, 63])
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    for k in args.k:
        run(args, k)


if __name__ == "__main__":
    main()
