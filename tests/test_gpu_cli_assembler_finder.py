"""GPU: `metacherchant --tool environment-assembler-finder` end to end -- the graph files byte-identical to the oracle's
environment_finder for the same arguments, cutReads<i>.fasta byte-identical to the model (tests/reads_filter_model.py) fed the
k-mers of the oracle's graph.txt, the second stage behind a stub assembler, and the refusals."""
import os
import subprocess

import numpy as np
import pytest

from oracle import host_oracle as ho
from oracle import pyoracle as po
from tests import reads_filter_model as rf

pytestmark = pytest.mark.gpu

GENOME = 20000
SEED_AT, SEED_LEN = 8000, 120


@pytest.fixture(scope="module")
def cli():
    from metacherchant_amd import build
    build.build_all()
    return build.CLI


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """two files of ~1 000 reads of 100 bases over a 20 kb genome (1 % substitutions, every third reverse-complemented), the first a
    FASTQ (some reads with an N, some with a phred-0 base, where the counting splits them), the second a FASTA in two-line records
    (some reads with an N: the counting drops them, the filter reads them with A); and the seed."""
    d = tmp_path_factory.mktemp("assembler_finder")
    rng = np.random.default_rng(20240531)
    genome = rng.integers(0, 4, GENOME).astype(np.uint8)
    texts = []
    for i in range(2000):
        s = int(rng.integers(0, GENOME - 100))
        r = genome[s:s + 100].copy()
        flip = rng.random(100) < 0.01
        r[flip] = (r[flip] + rng.integers(1, 4, int(flip.sum()))) & 3
        if i % 3 == 1:
            r = (3 - r[::-1]).astype(np.uint8)
        t = po.decode(r)
        if i % 13 == 5:
            t = t[:37] + "N" + t[38:]
        texts.append(t)
    fq, fa = str(d / "reads_a.fastq"), str(d / "reads_b.fasta")
    with open(fq, "w") as f:
        for i, t in enumerate(texts[:1000]):
            q = ["I"] * 100
            if i % 7 == 0:
                q[60] = "!"
            f.write("@r%d\n%s\n+\n%s\n" % (i, t, "".join(q)))
    with open(fa, "w") as f:
        for i, t in enumerate(texts[1000:]):
            f.write(">r%d\n%s\n%s\n" % (i, t[:70], t[70:]))
    seq = str(d / "seed.fasta")
    with open(seq, "w") as f:
        f.write(">gene one\n%s\n" % po.decode(genome[SEED_AT:SEED_AT + SEED_LEN]))
    return {"genome": genome, "files": [fq, fa], "texts": [texts[:1000], texts[1000:]], "seq": seq, "dir": d}


def _oracle(read_files, k, mode, seq, out_dir, **kw):
    """the oracle's files for the one sequence: the table counted as environment-finder counts it, then its walk and writers"""
    t = po.Table()
    for p in read_files:
        reads = ho.read_fastq_reads(p) if p.endswith((".fastq", ".fq")) else ho.read_fasta_reads(p)
        codes = np.concatenate([po.encode(r) for r in reads])
        off = np.zeros(len(reads) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in reads])
        t.count_reads(codes, off, k, mode)
    seqs, _ = ho.rich_fasta_read(seq)
    res = ho.environment_finder(t, k, mode, seqs[:1], ["x"], out_dir, **kw)
    (files,) = res.values()
    return files


def _check_phase(got_dir, want_files, k, texts, pct=1):
    """graph files equal the oracle's, cutReads<i>.fasta the model's; returns the kept reads a file"""
    assert want_files is not None
    for name, text in want_files.items():
        with open(os.path.join(got_dir, name)) as f:
            assert f.read() == text, (got_dir, name)
    members = rf.make_set(line.split(" ")[0] for line in want_files["graph.txt"].splitlines())
    assert len(members) == len(want_files["graph.txt"].splitlines())
    kept = []
    for i, reads in enumerate(texts):
        want = rf.cut_reads_fasta(reads, k, members, pct, i)
        with open(os.path.join(got_dir, "cutReads%d.fasta" % i)) as f:
            got = f.read()
        assert got == want, (got_dir, i, got[:300], want[:300])
        kept.append(want.count(">"))
    return kept


def _run(cli, args, wd):
    return subprocess.run([cli, "--tool", "environment-assembler-finder", "-w", str(wd), "--force"] + args, capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("k,mode,extra,kw", [
    (21, po.KEY_PACKED, [], {}),
    (31, po.KEY_POLY, ["--forcehash"], {}),
    (41, po.KEY_POLY, ["--trim", "--bothdirs"], dict(trim=True, bothdirs=True)),
])
def test_phase_one_is_the_oracles_graph_and_the_models_reads(cli, inputs, tmp_path, k, mode, extra, kw):
    out, want = str(tmp_path / "out"), str(tmp_path / "want")
    p = _run(cli, ["-k", str(k), "-i"] + inputs["files"] + ["--seq", inputs["seq"], "-o", out, "--maxkmers", "300"] + extra, tmp_path / "wd")
    assert p.returncode == 0, p.stderr[-2000:]
    files = _oracle(inputs["files"], k, mode, inputs["seq"], want, max_kmers=300, **kw)
    kept = _check_phase(out, files, k, inputs["texts"])
    # the test's own input: at -pf 1 some reads of every file are kept and most are not; a kept read with an N is printed with A
    assert all(0 < n < 500 for n in kept), kept
    assert sorted(os.listdir(out)) == ["cutReads0.fasta", "cutReads1.fasta", "env.txt", "graph.gfa", "graph.txt", "seqs.fasta", "tsvs"]
    for line in ("Finding environment for sequence", "Filtration done!", "Finished processing all sequences!"):
        assert line in p.stderr
    assert os.path.exists(str(tmp_path / "wd" / "SUCCESS"))


def test_pf_100_keeps_nothing_and_pf_50_less_than_pf_1(cli, inputs, tmp_path):
    files = _oracle(inputs["files"], 21, po.KEY_PACKED, inputs["seq"], str(tmp_path / "want"), max_kmers=300)
    kept = {}
    for pf in ("100", "50"):
        out = str(tmp_path / ("out" + pf))
        p = _run(cli, ["-k", "21", "-i"] + inputs["files"] + ["--seq", inputs["seq"], "-o", out, "--maxkmers", "300", "-pf", pf], tmp_path / "wd")
        assert p.returncode == 0, p.stderr[-2000:]
        kept[pf] = _check_phase(out, files, 21, inputs["texts"], pct=int(pf))
    assert kept["100"] == [0, 0] and os.path.getsize(os.path.join(str(tmp_path / "out100"), "cutReads1.fasta")) == 0
    assert all(n > 0 for n in kept["50"])


def test_two_sequences_write_nothing(cli, inputs, tmp_path):
    seq2 = str(tmp_path / "two.fasta")
    with open(seq2, "w") as f:
        f.write(open(inputs["seq"]).read() + ">gene two\n%s\n" % po.decode(inputs["genome"][100:200]))
    out = str(tmp_path / "out")
    p = _run(cli, ["-k", "21", "-i"] + inputs["files"] + ["--seq", seq2, "-o", out, "--maxkmers", "300"], tmp_path / "wd")
    assert p.returncode == 0 and "EnvironmentAssemblerFinder works only with one input sequence!" in p.stderr
    assert not os.path.exists(out)


def test_refusals(cli, inputs, tmp_path):
    base = ["-k", "21", "-i"] + inputs["files"] + ["--seq", inputs["seq"], "-o", str(tmp_path / "out")]
    for args, text in [
        (base + ["--maxkmers", "300", "--devices", "0,1"], "--devices"),
        (["-k", "64"] + base[2:] + ["--maxkmers", "300"], "k = 64 is not supported"),
        (base + ["--maxkmers", "300", "-pf", "101"], "--procfiltration"),
        (base + ["--maxkmers", "300", "--procfiltration", "-1"], "--procfiltration"),
        (base, "At least one of --maxkmers and --maxradius parameters should be set"),
        (base + ["--maxkmers", "300", "--merge"], "Unrecognized option: --merge"),
    ]:
        p = _run(cli, args, tmp_path / "wd")
        assert p.returncode == 1 and text in p.stderr + p.stdout, (args, p.stderr[-500:])
    assert not os.path.exists(str(tmp_path / "out"))
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=120)
    assert "--tool environment-assembler-finder" in p.stdout and "--procfiltration" in p.stdout


def _stub(path, lines):
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    os.chmod(path, 0o755)


def test_the_second_stage_behind_a_stub_assembler(cli, inputs, tmp_path):
    genome = inputs["genome"]
    # contigs of 200 .. 900 bases cut from the genome round the seed, overlapping, some reverse-complemented: what an assembler gives
    rng = np.random.default_rng(55)
    contigs = []
    for i in range(40):
        n = int(rng.integers(200, 900))
        s = int(rng.integers(SEED_AT - 2500, SEED_AT + 2500))
        c = genome[s:s + n]
        contigs.append(po.decode((3 - c[::-1]).astype(np.uint8) if i % 4 == 2 else c))
    prepared = str(tmp_path / "prepared.fa")
    with open(prepared, "w") as f:
        for i, c in enumerate(contigs):
            f.write(">k55_%d flag=1 multi=2.0 len=%d\n%s\n" % (i, len(c), c))
    bindir, argv_log = tmp_path / "bin", str(tmp_path / "argv.txt")
    bindir.mkdir()
    _stub(str(bindir / "megahit"), ["#!/bin/sh", "echo \"$@\" >> %s" % argv_log, "mkdir -p \"$4\" && echo assembling into \"$4\"",
                                    "cp %s \"$4/final.contigs.fa\"" % prepared])
    out, want = str(tmp_path / "out"), str(tmp_path / "want")
    p = _run(cli, ["-k", "21", "-i"] + inputs["files"] + ["--seq", inputs["seq"], "-o", out, "--maxkmers", "300", "--assembler", "megahit",
                   "--assemblerpath", str(bindir)], tmp_path / "wd")
    assert p.returncode == 0, p.stderr[-2000:]
    # the reference's argv, cutReads<i>.fastq included (AssemblerCalculator.java:65-66)
    assert open(argv_log).read().splitlines() == ["--12 %s/cutReads%d.fastq -o %s/out_megahit%d" % (out, i, out, i) for i in range(2)]
    assert "assembling into %s/out_megahit1" % out in p.stderr and "Finished assembling all sequences!" in p.stderr
    for i in range(2):
        assert open(os.path.join(out, "contigs%d.fasta" % i)).read() == open(prepared).read()
        assert not os.path.exists(os.path.join(out, "out_megahit%d" % i, "final.contigs.fa"))
    files1 = _oracle(inputs["files"], 21, po.KEY_PACKED, inputs["seq"], want, max_kmers=300)
    _check_phase(out, files1, 21, inputs["texts"])
    # k = 55, every k-mer counts, the contigs are the reads: hash keys, two-word k-mers in the filter
    cfiles = [os.path.join(out, "contigs%d.fasta" % i) for i in range(2)]
    files2 = _oracle(cfiles, 55, po.KEY_POLY, inputs["seq"], str(tmp_path / "want2"), max_kmers=300, coverage=0)
    kept = _check_phase(os.path.join(out, "result"), files2, 55, [contigs, contigs])
    assert all(0 < n < len(contigs) for n in kept), kept
    assert p.stderr.count("Filtration done!") == 2


def test_an_assembler_that_writes_nothing(cli, inputs, tmp_path):
    bindir = tmp_path / "bin"
    bindir.mkdir()
    _stub(str(bindir / "megahit"), ["#!/bin/sh", "echo nothing to do"])
    out = str(tmp_path / "out")
    p = _run(cli, ["-k", "21", "-i"] + inputs["files"] + ["--seq", inputs["seq"], "-o", out, "--maxkmers", "300", "--assembler", "megahit",
                   "--assemblerpath", str(bindir)], tmp_path / "wd")
    assert p.returncode != 0 and os.path.join(out, "contigs0.fasta") in p.stderr
    assert os.path.getsize(os.path.join(out, "graph.txt")) > 0 and os.path.getsize(os.path.join(out, "cutReads0.fasta")) > 0
    assert not os.path.exists(os.path.join(out, "result"))
    assert not os.path.exists(str(tmp_path / "wd" / "SUCCESS"))
