"""GPU: --render gpu against --render host in the same test, the classifying tools end to end, under --parse gpu and under --parse
host.  Every FASTQ file whose records mc_render_fastq rendered must equal, byte for byte, the file FastqOut::put writes.
MC_TOKENIZER_CHUNK_BYTES=4096 cuts a file of a few hundred records into many chunks, so under --parse gpu a batch is many segments and
a file's numbers run over many calls; with MC_INGEST_DEBUG=1 the tool says on stderr how many records the device rendered and how many
went through the host -- a quiet fall-back to the host's loop would make every comparison here pass without the kernels having run.
(The data recipe is that of tests/test_gpu_cli_whole_reads.py.)"""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENV = {"MC_INGEST_DEBUG": "1", "MC_TOKENIZER_CHUNK_BYTES": "4096"}
RENDER = re.compile(r"\[ingest\] render: (\d+) records in (\d+) call\(s\) on the device, (\d+) through the host")


@pytest.fixture(scope="module")
def cli():
    from metacherchant_amd import build
    build.build_all()
    return build.CLI


def _bases(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """a graph file, and pairs of its reads: the mates' lengths differ (the chunk cuts of the two files never line up), the second file
    is a few records shorter, quality offset 33, some reads with one low-quality position, some with two, some with an N"""
    d = tmp_path_factory.mktemp("render_cli")
    rng = np.random.default_rng(77)
    genome = _bases(rng, 6000)
    with open(d / "graph.fasta", "w") as f:
        for i in range(0, 5800, 40):
            f.write(">g%d\n%s\n" % (i, genome[i:i + 200]))
    texts = []
    for side, (lo, hi, n) in enumerate([(90, 151, 420), (60, 121, 413)]):
        out = []
        for i in range(n):
            L = int(rng.integers(lo, hi))
            s = int(rng.integers(0, len(genome) - L))
            r = list(genome[s:s + L] if i % 7 else _bases(rng, L))
            q = [chr(33 + int(x)) for x in rng.integers(12, 41, L)]
            for _ in range(int(rng.integers(0, 3)) if i % 3 == 0 else 0):
                p = int(rng.integers(0, L))
                q[p] = chr(33 + int(rng.integers(0, 10)))
                r[p] = "ACGT"[int(rng.integers(0, 4))]  # (what --correction is for: a wrong base under a low quality)
            if i % 11 == 5:
                r[int(rng.integers(0, L))] = "N"
            out.append("@p%d/%d\n%s\n+\n%s\n" % (i, side + 1, "".join(r), "".join(q)))
        texts.append(out)
        with open(d / ("reads_%d.fastq" % (side + 1)), "w") as f:
            f.write("".join(out))
    # one record with a quality char of offset + 63: phred 63, which the writers refuse
    bad = list(texts[0])
    head, seq, plus, qual = bad[200].split("\n")[:4]
    bad[200] = "%s\n%s\n%s\n%s\n" % (head, seq, plus, qual[:10] + chr(33 + 63) + qual[11:])
    with open(d / "reads_q63.fastq", "w") as f:
        f.write("".join(bad))
    return d


def _run(cli, args, parse, render, wd):
    return subprocess.run([cli] + args + ["--parse", parse, "--render", render, "-w", str(wd)], capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, **ENV))


def _files(root):
    out = {}
    for dirpath, _, names in os.walk(root):
        for n in names:
            with open(os.path.join(dirpath, n), "rb") as f:
                out[os.path.relpath(os.path.join(dirpath, n), root)] = f.read()
    return out


def _records(text):
    return text.count(b"\n+\n")


def _both_ways(cli, args, parse, tmp_path, nonempty=None):
    """(the files, equal both ways; the records that went through the host under --render gpu).  nonempty: the files that must hold
    reads (default: all)"""
    got = {}
    for render in ("host", "gpu"):
        out = tmp_path / ("out_" + render)
        p = _run(cli, args + ["-o", str(out)], parse, render, tmp_path / ("wd_" + render))
        assert p.returncode == 0, p.stderr[-3000:]
        m = RENDER.findall(p.stderr)
        assert len(m) == 1, p.stderr[-2000:]
        got[render] = (_files(out), tuple(int(x) for x in m[0]))
    files = got["host"][0]
    # (every file has reads: the comparison is of something)
    assert all(len(files[k]) > 0 for k in (nonempty or files)), {k: len(v) for k, v in files.items()}
    assert got["gpu"][0] == files
    total = sum(_records(v) for v in files.values())
    assert got["host"][1] == (0, 0, total)
    r, calls, h = got["gpu"][1]
    assert r == total and calls >= (5 if parse == "gpu" else 1)  # (--parse gpu: a call per sub-range of a batch's segments)
    return files, h


@pytest.mark.parametrize("parse", ["gpu", "host"])
def test_reads_classifier_paired_with_correction(cli, data, tmp_path, parse):
    files, h = _both_ways(cli, ["--tool", "reads-classifier", "-k", "21", "-i", str(data / "graph.fasta"), "-r", str(data / "reads_1.fastq"),
                                str(data / "reads_2.fastq"), "--correction"], parse, tmp_path)
    assert sorted(files) == sorted(["found_1.fastq", "found_2.fastq", "not_found_1.fastq", "not_found_2.fastq", "found_s.fastq", "not_found_s.fastq"])
    # only the "second only" pairs' records are numbered by the host: a pair's two reads, one to each _s file
    assert 0 < h < _records(files["found_s.fastq"]) + _records(files["not_found_s.fastq"]) and h % 2 == 0


@pytest.mark.parametrize("parse", ["gpu", "host"])
def test_reads_classifier_single_end(cli, data, tmp_path, parse):
    """every read is paired with an empty one: a found read goes to found_s's head, a read that is not found to not_found_s's tail"""
    files, h = _both_ways(cli, ["--tool", "reads-classifier", "-k", "21", "-i", str(data / "graph.fasta"), "-r", str(data / "reads_2.fastq"),
                                "-found", "60"], parse, tmp_path, nonempty=["found_s.fastq", "not_found_s.fastq"])
    assert {k for k, v in files.items() if v} == {"found_s.fastq", "not_found_s.fastq"}  # (the pair files stay empty)
    assert h == _records(files["not_found_s.fastq"])


@pytest.mark.parametrize("parse", ["gpu", "host"])
def test_triple_reads_classifier(cli, data, tmp_path, parse):
    files, h = _both_ways(cli, ["--tool", "triple-reads-classifier", "-k", "21", "-k2", "41", "-i", str(data / "graph.fasta"), "-r",
                                str(data / "reads_1.fastq"), str(data / "reads_2.fastq"), "--correction"], parse, tmp_path)
    assert len(files) == 9 and h == 0


@pytest.mark.parametrize("parse", ["gpu", "host"])
def test_a_phred_of_63_fails_both_ways(cli, data, tmp_path, parse):
    for render in ("host", "gpu"):
        p = _run(cli, ["--tool", "reads-classifier", "-k", "21", "-i", str(data / "graph.fasta"), "-r", str(data / "reads_q63.fastq"), "-o",
                       str(tmp_path / ("out_" + render))], parse, render, tmp_path / ("wd_" + render))
        assert p.returncode != 0 and "Invalid quality code byte: 63" in p.stderr, (render, p.stderr[-2000:])


def test_render_does_not_apply_to_the_other_tools(cli, tmp_path):
    for tool in ("environment-finder", "kmer-counter", "environment-finder-multi"):
        p = subprocess.run([cli, "--tool", tool, "--render", "gpu", "-w", str(tmp_path / "wd")], capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "--render does not apply to --tool " + tool in p.stderr, (tool, p.stderr[-500:])
    p = subprocess.run([cli, "--tool", "seq-cov", "--render", "gpu", "-w", str(tmp_path / "wd")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "Unrecognized option: --render" in p.stderr, p.stderr[-500:]
    p = subprocess.run([cli, "--tool", "reads-classifier", "--render", "device"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "--render takes host, gpu or auto, not 'device'" in p.stderr


def test_help_names_the_switch(cli):
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--render host|gpu|auto" in p.stdout
