"""GPU: `--compact gpu` (mc_unitigs, then the loop over the irregular entries only) writes, byte for byte, the files that
`--compact host` (the loop on labels) writes, for every tool that compacts environments; the log names the compactor.  The inputs
are the small ones of the tools' own CLI tests."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import components_model as cm
from tests.helpers import synth_case
from tests.test_gpu_cli import _write_fasta
from tests.test_gpu_cli_fmt_visualizer import _phase_inputs
from tests.test_gpu_cli_recipient import _inputs, _write_reads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    from metacherchant_amd import build
    build.build_all()
    return build.CLI


def _tree(root):
    got = {}
    for d, _, names in os.walk(root):
        for n in names:
            got[os.path.relpath(os.path.join(d, n), root)] = open(os.path.join(d, n), "rb").read()
    return got


def _both_ways(cmd, tmp_path):
    """runs cmd with -o / -w of its own for each compactor; the trees must be the same and not empty"""
    trees, logs = {}, {}
    for how in ("host", "gpu"):
        out, wd = str(tmp_path / ("out_" + how)), str(tmp_path / ("wd_" + how))
        p = subprocess.run(cmd + ["-o", out, "-w", wd, "--force", "--compact", how], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        trees[how], logs[how] = _tree(out), open(os.path.join(wd, "log")).read()
    assert sorted(trees["gpu"]) == sorted(trees["host"]) and trees["host"]
    for name in sorted(trees["host"]):
        assert trees["gpu"][name] == trees["host"][name], name
    assert any(n.endswith(".gfa") and b"\nL\t" in t for n, t in trees["host"].items())  # (graphs with links, not empty files)
    n_host, n_gpu = logs["host"].count(") on the host"), logs["gpu"].count(") on the GPU (mc_unitigs)")
    assert n_host == n_gpu >= 1 and "mc_unitigs" not in logs["host"] and ") on the host" not in logs["gpu"]
    return trees["host"]


@pytest.mark.parametrize("k,merge", [(21, False), (41, False), (21, True), (41, True)])
def test_environment_finder(cli, tmp_path, k, merge):
    genome, reads, _ = synth_case(1, 30000, 5000, 150, 30)
    r1 = str(tmp_path / "reads.fna")
    _write_fasta(r1, reads, 150)
    seq = str(tmp_path / "seed.fasta")
    with open(seq, "w") as f:
        f.write(">s\n%s\n>t\n%s\n" % (po.decode(genome[15000:15300]), po.decode(genome[4000:4200])))
    cmd = [cli, "-k", str(k), "-i", r1, "--seq", seq, "--maxkmers", "3000", "--coverage", "3", "--bothdirs", "True"] + (["--merge", "true"] if merge else [])
    tree = _both_ways(cmd, tmp_path)
    assert sum(n.endswith("seqs.fasta") for n in tree) == (1 if merge else 2)


def test_recipient_visualiser(cli, tmp_path):
    k, ext = 31, "fasta"
    after, class_reads, seqs = _inputs(k)
    in_dir = str(tmp_path / "in")
    os.makedirs(in_dir)
    for name, reads in class_reads.items():
        _write_reads(os.path.join(in_dir, name + "." + ext), reads)
    after_path, seq_path = str(tmp_path / "after.fasta"), str(tmp_path / "genes.fasta")
    _write_reads(after_path, after)
    with open(seq_path, "w") as f:
        f.write("".join(">g%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    _both_ways([cli, "--tool", "recipient-visualiser", "-k", str(k), "-after", after_path, "-seq", seq_path, "-i", in_dir, "-ext", ext,
                "--maxkmers", "300"], tmp_path)


def test_fmt_visualizer(cli, tmp_path):
    k, ext = 21, "fasta"
    rng = np.random.default_rng(100 + k)
    inputs = {name: _phase_inputs(rng, k, classes) for name, classes in cm.PHASES}
    in_dir = str(tmp_path / "in")
    os.makedirs(in_dir)
    paths = {}
    for name, classes in cm.PHASES:
        reads, class_reads = inputs[name]
        paths[name] = str(tmp_path / ("%s.fasta" % name))
        _write_reads(paths[name], reads)
        for c in classes:
            for i, m in enumerate("12s"):
                _write_reads(os.path.join(in_dir, "%s_%s.%s" % (c, m, ext)), class_reads[c][i::3])
    _both_ways([cli, "--tool", "fmt-visualizer", "-k", str(k), "-donor", paths["donor"], "-before", paths["before"], "-after", paths["after"],
                "-i", in_dir, "-ext", ext, "-p", "4"], tmp_path)


def test_environment_assembler_finder(cli, tmp_path):
    """the small input of the tool's own CLI test: ~2 000 reads of 100 bases over a 20 kb genome in a FASTQ and a FASTA, one seed"""
    rng = np.random.default_rng(20240531)
    genome = rng.integers(0, 4, 20000).astype(np.uint8)
    reads = []
    for i in range(2000):
        s = int(rng.integers(0, len(genome) - 100))
        r = genome[s:s + 100]
        reads.append(po.decode((3 - r[::-1]).astype(np.uint8) if i % 3 == 1 else r))
    fq, fa, seq = str(tmp_path / "reads_a.fastq"), str(tmp_path / "reads_b.fasta"), str(tmp_path / "seed.fasta")
    with open(fq, "w") as f:
        f.write("".join("@r%d\n%s\n+\n%s\n" % (i, t, "I" * 100) for i, t in enumerate(reads[:1000])))
    with open(fa, "w") as f:
        f.write("".join(">r%d\n%s\n" % (i, t) for i, t in enumerate(reads[1000:])))
    with open(seq, "w") as f:
        f.write(">gene one\n%s\n" % po.decode(genome[8000:8120]))
    tree = _both_ways([cli, "--tool", "environment-assembler-finder", "-k", "21", "-i", fq, fa, "--seq", seq, "--maxkmers", "300"], tmp_path)
    assert {"graph.gfa", "seqs.fasta", "cutReads0.fasta", "cutReads1.fasta"} <= set(tree) and tree["cutReads0.fasta"]


@pytest.mark.parametrize("tool", ["kmer-counter", "environment-finder-multi"])
def test_tools_that_compact_nothing_refuse_the_option(cli, tmp_path, tool):
    p = subprocess.run([cli, "--tool", tool, "-k", "21", "--compact", "gpu", "-w", str(tmp_path / "wd")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "--compact does not apply to --tool " + tool in p.stderr + p.stdout
    assert not os.path.exists(str(tmp_path / "wd"))
