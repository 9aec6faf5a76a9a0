"""The table as a file, the host loops against the kernels: mc_save_kmers against mc_save_kmers_gpu and mc_load_kmers against
mc_load_kmers_gpu (csrc/kmers_bin.hip), as `--kmers-io host` and `--kmers-io gpu` run them.

For every size a table of that many random distinct keys is filled through add_pairs_dev with counts from a skewed distribution
(60 % ones, 25 % twos, a tail into the thousands), k = 31 packed at every size and k = 63 poly at 10^6 and 10^8.  Timed, wall clock
around calls that end on the host: the save of the table (threshold 0, with the statistics file), and the load of that file into
a fresh context with a capacity hint, up to and including finalize.  The files go to the system's temporary directory.  Each way
runs --reps times, the two in turn, after one untimed run of either.  Reported: the median and the range (min .. max) of each way; for
the GPU's way, from MC_KMERS_STATS=1, the medians of its stages -- device time of the count sweep and of the write sweep (HIP events),
of the copies, the time the writer thread spent in write(), the reader's time in h2d_pinned (pread and the copies together), the
decoder's device time, mc_add_pairs_dev's calls -- and the extra device memory; and the encoder's rate, (table bytes read in both
sweeps + bytes written) / (count sweep + write sweep), as a fraction of the 6.3 TB/s that MI355X_MICROARCH.md gives for streaming HBM.
File time depends on the machine's storage; it is common to both ways and is reported, not judged.

Every size is a process of its own under its own time limit (one process holds the GPU at a time); the first failure ends the run.
The last line gives the `auto` constants of csrc/host/cli.h: for the save and for the load the smallest measured size from
which on, at every measured size and k, the GPU way's median is below the host way's fastest run; null when there is none.

    python scripts/kmers_bin_bench.py [--sizes 10000 100000 1000000 10000000 100000000] [--reps 5] [--out profiles/kmers_bin_bench.txt]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_STREAM_BYTES_PER_S = 6.3e12  # MI355X_MICROARCH.md, "HBM": achievable (8 TB/s is the peak)
POLY_SIZES = (1_000_000, 100_000_000)


def one(n, k, reps, device):
    """the child: one table, both ways, JSON on stdout (the stages' lines go to stderr, the parent reads them)"""
    import numpy as np
    import torch
    import metacherchant_amd as m
    dev = "cuda:%d" % device
    mode = m.KEY_PACKED if k <= 31 else m.KEY_POLY
    g = torch.Generator(device=dev)
    g.manual_seed(1234 + k)
    ctx = m.Context(k, mode, device, n)
    batch = 1 << 24
    for a in range(0, n, batch):
        i = torch.arange(a + 1, min(a + batch, n) + 1, dtype=torch.int64, device=dev)
        keys = i * -7046029254386353131  # (0x9E3779B97F4A7C15, odd: a bijection modulo 2^64, and modulo 2^62)
        if mode == m.KEY_PACKED:
            keys &= (1 << 62) - 1
        assert not bool((keys == -1).any())
        u = torch.rand(len(i), device=dev, generator=g)
        tail = (3 + torch.empty(len(i), device=dev).exponential_(1 / 40.0, generator=g)).clamp(max=32767)
        counts = torch.where(u < 0.6, torch.ones_like(tail), torch.where(u < 0.85, torch.full_like(tail, 2), tail)).to(torch.int16)
        ctx.add_pairs_dev(keys, counts, len(i))
        torch.cuda.synchronize(dev)  # (the call only enqueues; the next batch's tensors may take this one's memory)
    assert ctx.finalize() == n
    tmp = tempfile.gettempdir()
    files = {w: (os.path.join(tmp, "kb_bench_%d_%s.kmers.bin" % (os.getpid(), w)), os.path.join(tmp, "kb_bench_%d_%s.stat.txt" % (os.getpid(), w)))
             for w in ("host", "gpu")}
    save = {"host": ctx.save_kmers, "gpu": ctx.save_kmers_gpu}
    times = {"save_host": [], "save_gpu": [], "load_host": [], "load_gpu": []}
    try:
        pairs = {}
        for rep in range(reps + 1):  # (the first one untimed)
            for w in ("host", "gpu"):
                sys.stderr.write("@@ save %s rep %d\n" % (w, rep))
                sys.stderr.flush()
                t0 = time.perf_counter()
                pairs[w] = save[w](files[w][0], files[w][1], 0)
                if rep:
                    times["save_" + w].append(time.perf_counter() - t0)
        assert pairs["host"] == pairs["gpu"] == (n, n), pairs
        assert os.path.getsize(files["host"][0]) == os.path.getsize(files["gpu"][0]) == 10 * n
        assert open(files["host"][1], "rb").read() == open(files["gpu"][1], "rb").read()
        same_records = None
        if n <= 1_000_000:  # (the records, sorted: the orders differ)
            a = np.sort(np.fromfile(files["host"][0], dtype="S10"))
            b = np.sort(np.fromfile(files["gpu"][0], dtype="S10"))
            same_records = bool(np.array_equal(a, b))
            assert same_records
        ctx.close()
        os.remove(files["host"][0])
        path = files["gpu"][0]
        sizes = {}
        for rep in range(reps + 1):
            for w in ("host", "gpu"):
                sys.stderr.write("@@ load %s rep %d\n" % (w, rep))
                sys.stderr.flush()
                c2 = m.Context(k, mode, device, n)
                t0 = time.perf_counter()
                got = (c2.load_kmers if w == "host" else c2.load_kmers_gpu)(path, 0)
                sizes[w] = c2.finalize()
                if rep:
                    times["load_" + w].append(time.perf_counter() - t0)
                assert got == (n, n), got
                c2.close()
        assert sizes["host"] == sizes["gpu"] == n
    finally:
        for w in files:
            for f in files[w]:
                if os.path.exists(f):
                    os.remove(f)
    print(json.dumps({"n": n, "k": k, "reps": reps, "same_records": same_records, **times}), flush=True)


def stage_medians(stderr, reps):
    """the medians of the figures of the timed calls' MC_KMERS_STATS lines"""
    out = {}
    for what, tag in (("mc_save_kmers_gpu", "save"), ("mc_load_kmers_gpu", "load")):
        rows, timed = [], False
        for line in stderr.splitlines():
            mark = re.match(r"@@ (\w+) (\w+) rep (\d+)", line)
            if mark:
                timed = mark.group(1) == tag and mark.group(2) == "gpu" and int(mark.group(3)) > 0
            elif line.startswith(what + ":") and timed:
                rows.append({a: float(b) for a, b in re.findall(r"(\w+) ([0-9.]+)", line.split(":", 1)[1])})
        assert len(rows) == reps, (what, len(rows))
        out[tag] = {key: statistics.median(r[key] for r in rows) for key in rows[0]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[10_000, 100_000, 1_000_000, 10_000_000, 100_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmers_bin_bench.txt"))
    ap.add_argument("--one", type=int, nargs=2, metavar=("N", "K"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        one(args.one[0], args.one[1], args.reps, args.device)
        return
    from metacherchant_amd import build
    build.build_lib()
    env = dict(os.environ, MC_KMERS_STATS="1")
    env.pop("MC_KMERS_CHUNK_RECORDS", None)
    results = []
    for n in sorted(args.sizes):
        for k in [31] + ([63] if n in POLY_SIZES else []):
            limit = 120 + n // 150_000  # seconds: the 10^8 tables take their time on the host's side
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), str(k), "--reps", str(args.reps), "--device", str(args.device)],
                                   capture_output=True, text=True, env=env, timeout=limit)
            except subprocess.TimeoutExpired:
                raise SystemExit("n = %d, k = %d: no result after %d s" % (n, k, limit))
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-4000:])
                raise SystemExit("n = %d, k = %d failed (%d)" % (n, k, p.returncode))
            r = json.loads(p.stdout.strip().splitlines()[-1])
            r["stages"] = stage_medians(p.stderr, args.reps)
            s = r["stages"]["save"]
            moved = 2 * s["slots"] * 16 + 10 * s["records"]
            r["encoder_bytes_per_s"] = moved / ((s["count_ms"] + s["write_ms"]) * 1e-3)
            r["encoder_fraction_of_hbm_stream"] = r["encoder_bytes_per_s"] / HBM_STREAM_BYTES_PER_S
            for w in ("save", "load"):
                r[w + "_gpu_wins"] = statistics.median(r[w + "_gpu"]) < min(r[w + "_host"])
            print(json.dumps(r), flush=True)
            results.append(r)
    auto = {}
    for w in ("save", "load"):
        at = None
        for n in sorted({r["n"] for r in results}, reverse=True):
            if not all(r[w + "_gpu_wins"] for r in results if r["n"] == n):
                break
            at = n
        auto[w] = at
    med, ms = statistics.median, lambda v: "%9.2f" % (1e3 * v)
    lines = ["# scripts/kmers_bin_bench.py: wall clock in ms, median (min .. max) of %d runs, the two ways in turn; stages: medians, ms" % args.reps,
             "# save = the table to <name>.kmers.bin + <name>.stat.txt; load = the file into a fresh hinted context, finalize included",
             "%11s %3s %5s  %-34s %-34s %s" % ("keys", "k", "what", "host", "gpu", "gpu wins")]
    for r in results:
        for w in ("save", "load"):
            h, g = r[w + "_host"], r[w + "_gpu"]
            lines.append("%11d %3d %5s  %s (%s ..%s) %s (%s ..%s) %s" % (r["n"], r["k"], w, ms(med(h)), ms(min(h)), ms(max(h)), ms(med(g)), ms(min(g)), ms(max(g)),
                                                                       "yes" if r[w + "_gpu_wins"] else "no"))
    lines.append("")
    lines.append("# the GPU way's stages: save = count sweep | write sweep | copies (device, HIP events) | writer thread in write() | chunks | extra device MB")
    lines.append("#                       load = reader in h2d_pinned (pread + copies) | decode (device) | mc_add_pairs_dev calls | chunks | extra device MB")
    lines.append("# encoder rate = (2 x slots x 16 B + 10 B x records) / (count + write sweep); fraction of %.1f TB/s streaming HBM" % (HBM_STREAM_BYTES_PER_S / 1e12))
    for r in results:
        s, l = r["stages"]["save"], r["stages"]["load"]
        lines.append("%11d %3d  save  %8.3f | %8.3f | %8.3f | %9.3f | %4d | %8.1f   encoder %7.1f GB/s = %.3f" % (
            r["n"], r["k"], s["count_ms"], s["write_ms"], s["copy_ms"], s["file_ms"], s["chunks"], s["extra_device_bytes"] / 1e6,
            r["encoder_bytes_per_s"] / 1e9, r["encoder_fraction_of_hbm_stream"]))
        lines.append("%11d %3d  load  %8.3f | %8.3f | %8.3f | %4d | %8.1f" % (
            r["n"], r["k"], l["fetch_ms"], l["decode_ms"], l["add_ms"], l["chunks"], l["extra_device_bytes"] / 1e6))
    lines.append("")
    lines.append("# auto (smallest measured size from which the GPU way's median is below the host way's fastest run): save %s, load %s" % (auto["save"], auto["load"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"KMERS_SAVE_AUTO_MIN": auto["save"], "KMERS_LOAD_AUTO_MIN": auto["load"]}), flush=True)


if __name__ == "__main__":
    main()
