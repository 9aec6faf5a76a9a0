"""Who should render the classifiers' FASTQ records?  Synthetic FASTQ pairs (scripts/whole_reads_bench.py's recipe: reads of a synthetic
genome, 150 bases, Sanger qualities) of 10^5, 10^6 and 10^7 records a file, and for each size, under --parse gpu,
  - `metacherchant --tool reads-classifier` (single-end, the first file) and `--tool triple-reads-classifier` (both files) as a whole with
    --render host and with --render gpu;
  - the stage from the tools' MC_INGEST_DEBUG timers: the seconds in FastqOut::put (host) against the seconds in the render calls, the
    copies down and the writes (gpu), the kernels' device_ms, and the bytes a second the emitter reaches (text bytes / device_ms: the
    measuring passes are in the figure, so it is a lower bound);
  - optionally (--parent-cli) the parent commit's binary in turn with the two ways, once a size or (--parent-runs 3) every round:
    --render host is the old path at the old speed.
Every figure is the median of three runs, the two ways run in turn, the files in the page cache (they were just written and are read
once before).  Usage: python scripts/render_bench.py [--sizes 100000,1000000,10000000] [--dir DIR] [--out FILE] [--parent-cli PATH]"""
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

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metacherchant_amd import build, native  # noqa: E402
from scripts.whole_reads_bench import GENOME, write_reads  # noqa: E402

PUT = re.compile(r"\[ingest\] FastqOut: ([0-9.]+) s in put\(\) for (\d+) records")
RENDER = re.compile(r"\[ingest\] render: (\d+) records in (\d+) call\(s\) on the device, (\d+) through the host")
STAGE = re.compile(r"\[ingest\] render stage: ([0-9.]+) s in the calls \(([0-9.]+) ms on the device\), ([0-9.]+) s in the copies down")


def timed(cmd):
    t = time.perf_counter()
    p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, MC_INGEST_DEBUG="1"))
    dt = time.perf_counter() - t
    if p.returncode != 0:
        raise SystemExit("%s failed:\n%s" % (" ".join(cmd), p.stderr[-2000:]))
    return dt, p.stderr


def same_files(a, b):
    return sorted(os.listdir(a)) == sorted(os.listdir(b)) and all(
        open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read() for f in os.listdir(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-cli", default=None, help="the parent commit's metacherchant binary: run once a size, for the old path's speed")
    ap.add_argument("--parent-runs", type=int, default=1, help="how many of the three rounds the parent's binary takes part in")
    ap.add_argument("--tools", default="reads-classifier,triple-reads-classifier")
    a = ap.parse_args()
    build.build_all()
    work = a.dir or tempfile.mkdtemp(prefix="render_bench_")
    os.makedirs(work, exist_ok=True)
    rng = np.random.default_rng(1)
    genome = native.synth_genome(20240607, 0, GENOME)
    graph = os.path.join(work, "graph.fasta")
    with open(graph, "wb") as f:
        f.write(b">genome\n" + np.frombuffer(b"AGCT", dtype=np.uint8)[genome].tobytes() + b"\n")
    rows = []
    for n in [int(x) for x in a.sizes.split(",")]:
        reads = [os.path.join(work, "reads_%d_%d.fastq" % (n, s)) for s in (1, 2)]
        for path in reads:
            write_reads(path, n, genome, rng)
            with open(path, "rb") as f:
                while f.read(1 << 26):
                    pass
        text_mb = round(os.path.getsize(reads[0]) / 1e6, 1)
        for tool in a.tools.split(","):
            args = ["--tool", tool, "-i", graph, "--parse", "gpu"]
            args += ["-k", "31", "--correction", "-r", reads[0]] if tool == "reads-classifier" else ["-k", "21", "-k2", "31", "-r"] + reads
            row = {"tool": tool, "records_a_file": n, "text_MB_a_file": text_mb}
            runs = {"host": [], "gpu": [], "parent": []}
            for rep in range(3):
                for way in ("host", "gpu") + (("parent",) if a.parent_cli and rep < a.parent_runs else ()):
                    wd, od = os.path.join(work, "wd"), os.path.join(work, "out_" + way)
                    shutil.rmtree(wd, ignore_errors=True)
                    shutil.rmtree(od, ignore_errors=True)
                    dt, err = timed([a.parent_cli] + args + ["-o", od, "-w", wd] if way == "parent" else [build.CLI] + args + ["-o", od, "-w", wd, "--render", way])
                    put, ren, st = PUT.search(err), RENDER.search(err), STAGE.search(err)
                    r = {"tool_s": dt, "write_s": float(put.group(1)) if put else None}
                    if way == "gpu":
                        r.update(records=int(ren.group(1)), calls=int(ren.group(2)), through_host=int(ren.group(3)), call_s=float(st.group(1)),
                                 device_ms=float(st.group(2)), copy_s=float(st.group(3)))
                    runs[way].append(r)
            med = lambda way, key: statistics.median(x[key] for x in runs[way]) if runs[way][0].get(key) is not None else None  # noqa: E731
            out_bytes = sum(os.path.getsize(os.path.join(work, "out_gpu", f)) for f in os.listdir(os.path.join(work, "out_gpu")))
            row.update(tool_host_s=round(med("host", "tool_s"), 3), tool_gpu_s=round(med("gpu", "tool_s"), 3),
                       tool_host_runs=[round(x["tool_s"], 3) for x in runs["host"]], tool_gpu_runs=[round(x["tool_s"], 3) for x in runs["gpu"]],
                       stage_host_put_s=med("host", "write_s"), stage_gpu_call_s=med("gpu", "call_s"), stage_gpu_copy_s=med("gpu", "copy_s"),
                       stage_gpu_write_s=med("gpu", "write_s"), device_ms=med("gpu", "device_ms"), calls=runs["gpu"][0]["calls"],
                       records=runs["gpu"][0]["records"], through_host=runs["gpu"][0]["through_host"], text_bytes=out_bytes,
                       emit_GB_s=round(out_bytes / 1e6 / med("gpu", "device_ms"), 2) if med("gpu", "device_ms") else None,
                       same_files=same_files(os.path.join(work, "out_host"), os.path.join(work, "out_gpu")))
            if a.parent_cli:
                row.update(parent_tool_s=round(med("parent", "tool_s"), 3), parent_tool_runs=[round(x["tool_s"], 3) for x in runs["parent"]],
                           parent_put_s=med("parent", "write_s"), parent_same_files=same_files(os.path.join(work, "out_host"), os.path.join(work, "out_parent")))
            rows.append(row)
            print(json.dumps(row), flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(rows, f, indent=1)
        for path in reads:
            os.remove(path)
    if not a.dir:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
