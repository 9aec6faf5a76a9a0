"""The environment-assembler-finder's host pieces (metacherchant_amd/csrc/host, through mc_hosttest; no GPU): the cut-reads
writer's numbering and spelling against the model (tests/reads_filter_model.py), and Environment::kmers, the set the filter is
given, against the oracle's graph.txt."""
import os
import subprocess

import numpy as np
import pytest

from oracle import host_oracle as ho
from oracle import pyoracle as po
from tests import reads_filter_model as rf


@pytest.fixture(scope="module")
def hosttest():
    from metacherchant_amd import build
    build.build_host()
    return build.HOSTTEST


@pytest.mark.parametrize("suffix", [".fasta", ".fastq"])
def test_cut_reads_are_numbered_from_one_and_spell_n_as_a(hosttest, tmp_path, suffix):
    reads = ["ACGTNACGT", "GGGG", "ttnnacg.a", "C", "ACACACACACAC"]
    keep = "10101"
    path = str(tmp_path / ("reads" + suffix))
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write(">r%d\n%s\n" % (i, r) if suffix == ".fasta" else "@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    out = str(tmp_path / "deep" / "dir" / "cutReads7.fasta")
    p = subprocess.run([hosttest, "cutreads", path, keep, out, "7"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout == "3\n", p.stderr
    want = "".join(">7|%d\n%s\n" % (n + 1, rf.read_text(r)) for n, r in enumerate(r for r, c in zip(reads, keep) if c == "1"))
    assert want == ">7|1\nACGTAACGT\n>7|2\nTTAAACGAA\n>7|3\nACACACACACAC\n"
    assert open(out).read() == want
    # no kept read: the file is still created, empty
    out0 = str(tmp_path / "none" / "cutReads0.fasta")
    p = subprocess.run([hosttest, "cutreads", path, "00000", out0, "0"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout == "0\n" and os.path.getsize(out0) == 0


@pytest.mark.parametrize("k,trim", [(21, False), (41, True)])
def test_environment_kmers_are_graph_txts(hosttest, tmp_path, k, trim):
    from tests.test_host_cpp import _dump
    rng = np.random.default_rng(k)
    genome = rng.integers(0, 4, 3000).astype(np.uint8)
    starts = rng.integers(0, len(genome) - 80, 600)
    codes = np.concatenate([genome[s:s + 80] for s in starts])
    off = np.arange(601, dtype=np.uint64) * 80
    mode = po.KEY_PACKED if k <= 31 else po.KEY_POLY
    t = po.Table()
    t.count_reads(codes, off, k, mode)
    gene = po.decode(genome[1000:1100])
    passes = [(d, po.bfs(t, k, mode, [po.encode(gene)], d, 1, 200, -1, trim)) for d in (-1, 1)]
    dump = str(tmp_path / "dump.txt")
    _dump(dump, k, 1, trim, [gene], passes)
    got = subprocess.check_output([hosttest, "kmers", dump], text=True).splitlines()
    env = ho.Environment(k, [gene], False)
    for _, r in passes:
        env.add_pass([po.kmer_string(h, l, k) for h, l in zip(r["hi"], r["lo"])], r["dist"], r["cov"], r["kept"] if trim else None)
    want = [line.split(" ")[0] for line in env.files(1)["graph.txt"].splitlines()]
    assert got == want and len(got) > 100
    assert all(x == rf.normalize_dna(x) for x in got)  # the subgraph's keys are normalised: what the filter's set is made of
