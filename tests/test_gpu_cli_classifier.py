"""GPU: `metacherchant --tool reads-classifier` end to end -- every output file byte-identical to the model
(tests/classifier_model.py) over the oracle's table, and the statistics lines in the log."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import classifier_model as cm
from tests.helpers import synth_case

pytestmark = pytest.mark.gpu

OUTS = ("found_1.fastq", "found_2.fastq", "not_found_1.fastq", "not_found_2.fastq", "found_s.fastq", "not_found_s.fastq")


@pytest.fixture(scope="module")
def cli():
    from metacherchant_amd import build
    build.build_all()
    return build.CLI


def _queries(genome, n, rng, with_n=False, low_q=True):
    """reads of the genome (some with errors, some absent), as (codes, phred) the way the reader will see them"""
    reads = []
    for i in range(n):
        L = int(rng.integers(60, 160))
        if i % 9 == 4:
            codes = rng.integers(0, 4, L).astype(np.uint8)
        else:
            s = int(rng.integers(0, len(genome) - L))
            codes = genome[s:s + L].copy()
            if rng.integers(0, 2):
                codes = (3 - codes[::-1]).astype(np.uint8)
            for _ in range(int(rng.integers(0, 3))):
                codes[int(rng.integers(0, L))] = int(rng.integers(0, 4))
        phred = rng.integers(12, 41, L).astype(np.uint8)
        if low_q:
            for _ in range(int(rng.integers(0, 3))):
                phred[int(rng.integers(0, L))] = int(rng.integers(1, 10))
        n_pos = []
        if with_n and i % 5 == 1:
            n_pos = [int(rng.integers(0, L))]
        for p in n_pos:
            codes[p] = 0
            phred[p] = 0
        reads.append((codes, phred, n_pos))
    return reads


def _write_fastq(path, reads, offset):
    lines = []
    for i, (codes, phred, n_pos) in enumerate(reads):
        s = list(po.decode(codes))
        for p in n_pos:
            s[p] = "N"
        lines.append("@q%d\n%s\n+\n%s\n" % (i, "".join(s), "".join(chr(int(q) + offset) if j not in n_pos else "#" for j, q in enumerate(phred))))
    data = "".join(lines).encode()
    with open(path, "wb") as f:
        f.write(gzip.compress(data) if path.endswith(".gz") else data)


def _write_fasta(path, reads):
    with open(path, "w") as f:
        for i, (codes, _, n_pos) in enumerate(reads):
            s = list(po.decode(codes))
            for p in n_pos:
                s[p] = "N"
            s = "".join(s)
            f.write(">q%d\n%s\n%s\n" % (i, s[:50], s[50:]))


CASES = {
    # name: (k, mode, -i kind, read files (suffix, quality offset), extra flags, found, z, correction)
    "single_end_illumina": (31, 0, "fastq", [(".fastq", 64)], [], 90, 1.0, False),
    "single_end_sanger_correction": (31, 0, "fastq", [(".fq", 33)], ["-corr"], 90, 1.0, True),
    "paired_unequal_interval95": (25, 0, "fastq", [(".fastq", 64), (".fastq", 33)], ["--interval95", "-found", "80"], 80, 1.96, False),
    "fasta_with_n_found50": (31, 0, "fastq", [(".fasta", None)], ["-found", "50", "--correction", "true"], 50, 1.0, True),
    "gz_k45_poly": (45, 1, "fastq", [(".fastq.gz", 64)], [], 90, 1.0, False),
    "kmers_bin_from_kmer_counter": (31, 0, "kmers.bin", [(".fastq", 64)], ["-corr"], 90, 1.0, True),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_cli_reads_classifier_matches_the_model(cli, tmp_path, name):
    k, mode, graph_kind, rfiles, extra, found, z, corr = CASES[name]
    genome, reads, _ = synth_case(1, 20000, 3000, 150, 50)
    graph = str(tmp_path / "graph.fastq")
    with open(graph, "w") as f:
        for i in range(3000):
            f.write("@g%d\n%s\n+\n%s\n" % (i, po.decode(reads[i * 150:(i + 1) * 150]), "h" * 150))
    t = po.Table()
    t.count_reads(reads, np.arange(3001, dtype=np.uint64) * 150, k, mode)
    get = cm.table_getter(t, k, mode)
    wd = str(tmp_path / "wd")
    graph_arg = graph
    if graph_kind == "kmers.bin":
        p = subprocess.run([cli, "--tool", "kmer-counter", "-k", str(k), "-i", graph, "-w", str(tmp_path / "wd_kc"),
                            "--output-dir", str(tmp_path / "kc")], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr
        graph_arg = str(tmp_path / "kc" / "graph.kmers.bin")
    rng = np.random.default_rng(sum(map(ord, name)))
    files, sets = [], []
    for j, (suffix, offset) in enumerate(rfiles):
        q = _queries(genome, 700 - 90 * j, rng, with_n=True)  # (the second file shorter: pairs end with it)
        path = str(tmp_path / ("reads_%d%s" % (j + 1, suffix)))
        if offset is None:
            _write_fasta(path, q)
            q = [(c, np.where(np.isin(np.arange(len(c)), n_pos), 0, 20).astype(np.uint8), n_pos) for c, _, n_pos in q]
        else:
            _write_fastq(path, q, offset)
        files.append(path)
        sets.append([(c, ph) for c, ph, _ in q])
    out = str(tmp_path / "out")
    cmd = [cli, "--tool", "reads-classifier", "-k", str(k), "-i", graph_arg, "-r"] + files + ["-o", out, "-w", wd] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    pairs = list(zip(sets[0], sets[1])) if len(sets) == 2 else cm.single_end(sets[0])
    lists = cm.split(pairs, k, get, found, z, corr)
    want = cm.outputs(lists)
    for f in OUTS:
        with open(os.path.join(out, f), "rb") as fh:
            assert fh.read() == want[f], (name, f)
    for line in cm.stats_lines(lists):
        assert line in p.stderr, (line, p.stderr[-2000:])
    assert "Hashtable size: %d kmers" % t.size() in p.stderr
    assert ("Searching for corrected reads in graph..." if corr else "Searching for reads in graph...") in p.stderr
    assert os.path.exists(os.path.join(wd, "SUCCESS"))
    assert any(len(lists[n]) for n in ("first", "second")) and (len(sets) == 1 or len(lists["both"]) and len(lists["neither"]))


def test_cli_reads_classifier_default_output_dir_and_errors(cli, tmp_path):
    genome, reads, _ = synth_case(1, 20000, 500, 150, 50)
    graph = str(tmp_path / "graph.fasta")
    with open(graph, "w") as f:
        for i in range(500):
            f.write(">g%d\n%s\n" % (i, po.decode(reads[i * 150:(i + 1) * 150])))
    rq = str(tmp_path / "r.fastq")
    with open(rq, "w") as f:
        f.write("@a\n%s\n+\n%s\n" % (po.decode(genome[100:200]), "5" * 100))
    wd = str(tmp_path / "wd")
    p = subprocess.run([cli, "-t", "reads-classifier", "-k", "31", "-i", graph, "-r", rq, "-w", wd], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert sorted(os.listdir(os.path.join(wd, "reads_classifier"))) == sorted(OUTS)
    with open(os.path.join(wd, "reads_classifier", "found_s.fastq")) as fh:
        assert fh.read() == "@1\n%s\n+\n%s\n" % (po.decode(genome[100:200]), "T" * 100)  # '5' is below 64: Sanger, phred 20 -> Illumina 'T'
    # paired input whose "both" list holds an empty read: the writer's failure, exit status 1
    r1, r2 = str(tmp_path / "p_1.fastq"), str(tmp_path / "p_2.fastq")
    with open(r1, "w") as f:
        f.write("@a\n\n+\n\n")
    with open(r2, "w") as f:
        f.write("@a\n%s\n+\n%s\n" % ("ACGT" * 5, "I" * 20))
    p = subprocess.run([cli, "-t", "reads-classifier", "-k", "31", "-i", graph, "-r", r1, r2, "-w", wd, "-o", str(tmp_path / "o2")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 1 and "Empty DnaQ!" in p.stderr, p.stderr
