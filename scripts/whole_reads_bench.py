"""Who should parse the whole reads of the classifying tools?  Synthetic FASTQ (reads of a synthetic genome, mc_synth_genome, written as
text: 150 bases, Sanger qualities, one read in sixteen with a low-quality position) of 10^5, 10^6 and 10^7 records, and for each size
  - the reader stage alone (mc_whole_reads_bench): DnaQReader plus the packing of classify_batch, against WholeReadsSource to a device view;
  - `metacherchant --tool reads-classifier` as a whole with --parse host and with --parse gpu.
Every figure is the median of three runs, the two ways run in turn, the file in the page cache (it was just written and is read once
before).  Usage: python scripts/whole_reads_bench.py [--sizes 100000,1000000,10000000] [--dir DIR] [--out FILE]"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metacherchant_amd import build, native  # noqa: E402

READ_LEN, GENOME = 150, 2_000_000


def write_reads(path, n, genome, rng):
    """n records of fixed width, built as one byte matrix a block of 10^6 records"""
    acgt = np.frombuffer(b"AGCT", dtype=np.uint8)
    with open(path, "wb") as f:
        for start in range(0, n, 1_000_000):
            m = min(1_000_000, n - start)
            head = np.frombuffer(b"".join(b"@r%09d\n" % i for i in range(start, start + m)), dtype=np.uint8).reshape(m, 12)
            pos = rng.integers(0, len(genome) - READ_LEN, m)
            bases = acgt[genome[pos[:, None] + np.arange(READ_LEN)[None, :]]]
            err = rng.random((m, READ_LEN)) < 0.01
            bases[err] = acgt[rng.integers(0, 4, int(err.sum()))]
            qual = (rng.integers(20, 41, (m, READ_LEN)) + 33).astype(np.uint8)
            low = np.flatnonzero(rng.integers(0, 16, m) == 0)
            qual[low, rng.integers(0, READ_LEN, len(low))] = 33 + 5
            rec = np.concatenate([head, bases, np.tile(np.frombuffer(b"\n+\n", dtype=np.uint8), (m, 1)), qual, np.full((m, 1), 10, dtype=np.uint8)], axis=1)
            f.write(rec.tobytes())


def timed(cmd):
    t = time.perf_counter()
    p = subprocess.run(cmd, capture_output=True, text=True)
    dt = time.perf_counter() - t
    if p.returncode != 0:
        raise SystemExit("%s failed:\n%s" % (" ".join(cmd), p.stderr[-2000:]))
    return dt, p.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build_all()
    bench = build.build_whole_reads_bench()
    work = a.dir or tempfile.mkdtemp(prefix="whole_reads_bench_")
    os.makedirs(work, exist_ok=True)
    rng = np.random.default_rng(1)
    genome = native.synth_genome(20240607, 0, GENOME)
    graph = os.path.join(work, "graph.fasta")
    with open(graph, "wb") as f:
        f.write(b">genome\n" + np.frombuffer(b"AGCT", dtype=np.uint8)[genome].tobytes() + b"\n")
    rows = []
    for n in [int(x) for x in a.sizes.split(",")]:
        reads = os.path.join(work, "reads_%d.fastq" % n)
        write_reads(reads, n, genome, rng)
        with open(reads, "rb") as f:
            while f.read(1 << 26):
                pass
        row = {"records": n, "text_MB": round(os.path.getsize(reads) / 1e6, 1)}
        stage = {"host": [], "gpu": []}
        tool = {"host": [], "gpu": []}
        for _ in range(3):
            for way in ("host", "gpu"):
                out = timed([bench, reads, way])[1].split()
                assert int(out[0]) == n and int(out[1]) == n * READ_LEN, out
                stage[way].append(float(out[2]))
        for rep in range(3):
            for way in ("host", "gpu"):
                wd, od = os.path.join(work, "wd"), os.path.join(work, "out_" + way)
                shutil.rmtree(wd, ignore_errors=True)
                shutil.rmtree(od, ignore_errors=True)
                tool[way].append(timed([build.CLI, "--tool", "reads-classifier", "-k", "31", "-i", graph, "-r", reads, "-o", od, "-w", wd, "--correction",
                                        "--parse", way])[0])
        same = all(open(os.path.join(work, "out_host", f), "rb").read() == open(os.path.join(work, "out_gpu", f), "rb").read()
                   for f in os.listdir(os.path.join(work, "out_host")))
        for way in ("host", "gpu"):
            row["stage_%s_s" % way] = round(statistics.median(stage[way]), 4)
            row["tool_%s_s" % way] = round(statistics.median(tool[way]), 3)
        row["same_files"] = same
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
        os.remove(reads)
    if not a.dir:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
