"""GPU: `metacherchant --kmers-io host|gpu|auto`: kmer-counter's files either way against each other and the oracle, reads-classifier
with a <name>.kmers.bin graph either way, the log line that says which way was taken, and the refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import host_oracle as ho
from oracle import pyoracle as po
from tests.helpers import synth_case

pytestmark = pytest.mark.gpu
OUTS = ("found_1.fastq", "found_2.fastq", "not_found_1.fastq", "not_found_2.fastq", "found_s.fastq", "not_found_s.fastq")


@pytest.fixture(scope="module")
def cli():
    from metacherchant_amd import build
    build.build_all()
    return build.CLI


def _plain(stderr, *dirs):
    """the log without its time stamps and the run's own directories"""
    out = []
    for line in stderr.splitlines():
        line = re.sub(r"^\d{4}-\d\d-\d\d \d\d:\d\d:\d\d ", "", line)
        for d in dirs:
            line = line.replace(d, "<dir>")
        out.append(line)
    return out


@pytest.mark.parametrize("k,mode", [(25, po.KEY_PACKED), (40, po.KEY_POLY)])
def test_cli_kmer_counter_either_way(cli, tmp_path, k, mode):
    _, reads, _ = synth_case(1, 30000, 4000, 150, 80)
    fa = str(tmp_path / "Sample_A.fasta")
    with open(fa, "w") as f:
        for i in range(4000):
            f.write(">r%d\n%s\n" % (i, po.decode(reads[i * 150:(i + 1) * 150])))
    t = po.Table()
    t.count_reads(reads, np.arange(4001, dtype=np.uint64) * 150, k, mode)
    want_recs, want_stat = ho.kmer_counter_files(t)
    logs, stats = {}, {}
    for way in ("host", "gpu"):
        wd = str(tmp_path / ("wd_" + way))
        p = subprocess.run([cli, "-t", "kmer-counter", "-k", str(k), "-i", fa, "-w", wd, "--force", "--kmers-io", way],
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr
        stats[way] = open(os.path.join(wd, "kmers", "Sample_A.stat.txt"), "rb").read()
        assert ho.read_kmers_bin(os.path.join(wd, "kmers", "Sample_A.kmers.bin")) == want_recs, way
        logs[way] = _plain(p.stderr, wd)
    assert stats["host"] == stats["gpu"] == want_stat.encode()
    line = {"host": "INFO: Writing %d k-mer records on the host (mc_save_kmers)" % t.size(),
            "gpu": "INFO: Writing %d k-mer records on the GPU (mc_save_kmers_gpu)" % t.size()}
    for way in logs:
        assert logs[way].count(line[way]) == 1, logs[way]
    assert [l for l in logs["host"] if l != line["host"]] == [l for l in logs["gpu"] if l != line["gpu"]]


def test_cli_reads_classifier_with_a_kmers_bin_graph_either_way(cli, tmp_path):
    """the smallest case of tests/test_gpu_cli_classifier.py ("kmers_bin_from_kmer_counter")"""
    from tests.test_gpu_cli_classifier import _queries, _write_fastq
    k = 31
    genome, reads, _ = synth_case(1, 20000, 3000, 150, 50)
    graph = str(tmp_path / "graph.fastq")
    with open(graph, "w") as f:
        for i in range(3000):
            f.write("@g%d\n%s\n+\n%s\n" % (i, po.decode(reads[i * 150:(i + 1) * 150]), "h" * 150))
    p = subprocess.run([cli, "--tool", "kmer-counter", "-k", str(k), "-i", graph, "-w", str(tmp_path / "wd_kc"), "--output-dir", str(tmp_path / "kc"),
                        "--kmers-io", "gpu"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    graph_arg = str(tmp_path / "kc" / "graph.kmers.bin")
    n_records = os.path.getsize(graph_arg) // 10
    rq = str(tmp_path / "reads_1.fastq")
    _write_fastq(rq, _queries(genome, 700, np.random.default_rng(5), with_n=True), 64)
    outs, logs = {}, {}
    for way in ("host", "gpu", "auto"):
        out, wd = str(tmp_path / ("out_" + way)), str(tmp_path / ("wd_" + way))
        p = subprocess.run([cli, "--tool", "reads-classifier", "-k", str(k), "-i", graph_arg, "-r", rq, "-o", out, "-w", wd, "-corr", "--kmers-io", way],
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr
        outs[way] = [open(os.path.join(out, f), "rb").read() for f in OUTS]
        logs[way] = _plain(p.stderr, wd, out)
    assert outs["host"] == outs["gpu"] == outs["auto"] and any(len(b) for b in outs["host"])
    line = {"host": "INFO: Loading %d k-mer records on the host (mc_load_kmers)" % n_records,
            "gpu": "INFO: Loading %d k-mer records on the GPU (mc_load_kmers_gpu)" % n_records}
    for way in ("host", "gpu"):
        assert logs[way].count(line[way]) == 1, logs[way]
    assert [l for l in logs["host"] if l != line["host"]] == [l for l in logs["gpu"] if l != line["gpu"]]
    assert logs["auto"] in (logs["host"], logs["gpu"])


def test_cli_kmers_io_refusals(cli, tmp_path):
    wd = str(tmp_path / "wd")
    p = subprocess.run([cli, "-t", "kmer-counter", "-k", "25", "-i", "x.fasta", "-w", wd, "--kmers-io", "cpu"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--kmers-io" in p.stderr and "'cpu'" in p.stderr
    assert all(v in p.stderr for v in ("host", "gpu", "auto"))
    p = subprocess.run([cli, "-t", "environment-finder", "-k", "25", "-i", "x.fasta", "--seq", "s.fa", "-o", str(tmp_path / "o"), "--maxkmers", "10",
                        "-w", wd, "--kmers-io", "gpu"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--kmers-io does not apply to --tool environment-finder" in p.stderr
    p = subprocess.run([cli, "-t", "environment-finder-multi", "-e", "g.txt", "--seq", "s.fa", "-o", str(tmp_path / "o"), "-w", wd, "--kmers-io", "host"],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--kmers-io does not apply to --tool environment-finder-multi" in p.stderr
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert "--kmers-io host|gpu|auto" in p.stdout
