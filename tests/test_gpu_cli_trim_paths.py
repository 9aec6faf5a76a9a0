"""GPU: `--trim --trim-on gpu` of environment-finder and environment-assembler-finder end to end: every output file byte-identical
to the `--trim-on host` run and to the oracle pipeline, on the walk of tests/trim_paths_model.py walk_case, where the trim removes
k-mers in every direction; and the option's handling."""
import os
import subprocess

import numpy as np
import pytest

from oracle import host_oracle as ho
from oracle import pyoracle as po
from tests import trim_paths_model as tm

pytestmark = pytest.mark.gpu

GPU_LINE = "on the GPU (mc_trim_paths)"


@pytest.fixture(scope="module")
def cli():
    from metacherchant_amd import build
    build.build_all()
    return build.CLI


def _inputs(d, k, n_seeds):
    """the walk case as a FASTA of reads and a FASTA of its first n_seeds seeds; returns (reads file, seq file, radius)"""
    codes, off, seeds, radius = tm.walk_case(k)
    reads, seq = str(d / ("reads%d.fasta" % k)), str(d / ("seeds%d_%d.fasta" % (k, n_seeds)))
    with open(reads, "w") as f:
        for i in range(len(off) - 1):
            f.write(">r%d\n%s\n" % (i, po.decode(codes[int(off[i]):int(off[i + 1])])))
    with open(seq, "w") as f:
        for i, s in enumerate(seeds[:n_seeds]):
            f.write(">seed%d\n%s\n" % (i, po.decode(s)))
    return reads, seq, radius


def _oracle(reads, seq, k, mode, out_dir, n_seqs=None, **kw):
    t = po.Table()
    rs = ho.read_fasta_reads(reads)
    off = np.zeros(len(rs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rs])
    t.count_reads(np.concatenate([po.encode(r) for r in rs]), off, k, mode)
    seqs, comments = ho.rich_fasta_read(seq)
    return ho.environment_finder(t, k, mode, seqs[:n_seqs], comments[:n_seqs], out_dir, **kw)


def _tree(root):
    """every file under root: relative path -> bytes"""
    out = {}
    for d, _, files in os.walk(root):
        for name in files:
            with open(os.path.join(d, name), "rb") as f:
                out[os.path.relpath(os.path.join(d, name), root)] = f.read()
    return out


def _run(cli, tool, args, wd):
    return subprocess.run([cli, "--tool", tool, "-w", str(wd), "--force"] + args, capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("k,mode,bothdirs", [(21, po.KEY_PACKED, False), (41, po.KEY_POLY, True)])
def test_environment_finder_files_are_the_hosts_and_the_oracles(cli, tmp_path, k, mode, bothdirs):
    reads, seq, radius = _inputs(tmp_path, k, 3)
    base = ["-k", str(k), "-i", reads, "--seq", seq, "--coverage", "2", "--maxradius", str(radius), "--merge", "true", "--trim",
            "--bothdirs", str(bothdirs)]
    trees = {}
    for on in ("host", "gpu"):
        out = str(tmp_path / on)
        p = _run(cli, "environment-finder", base + ["-o", out, "--trim-on", on], tmp_path / ("wd_" + on))
        assert p.returncode == 0, p.stderr[-2000:]
        assert (GPU_LINE in p.stderr) == (on == "gpu")
        assert p.stderr.count(GPU_LINE) == (0 if on == "host" else 1 if bothdirs else 2)  # every pass
        trees[on] = _tree(out)
    assert trees["gpu"] and trees["gpu"] == trees["host"]
    want_dir = str(tmp_path / "want")
    want = _oracle(reads, seq, k, mode, want_dir, coverage=2, max_radius=radius, merge=True, trim=True, bothdirs=bothdirs)
    (files,) = want.values()
    for name, text in files.items():
        assert trees["gpu"][os.path.join("merged", name)].decode() == text, name
    untrimmed = _oracle(reads, seq, k, mode, str(tmp_path / "untrimmed"), coverage=2, max_radius=radius, merge=True, trim=False, bothdirs=bothdirs)
    (files0,) = untrimmed.values()
    assert 0 < len(files["graph.txt"].splitlines()) < len(files0["graph.txt"].splitlines())  # (the trim removed something)


def test_assembler_finder_files_are_the_hosts_and_the_oracles(cli, tmp_path):
    k = 21
    reads, seq, radius = _inputs(tmp_path, k, 1)
    base = ["-k", str(k), "-i", reads, "--seq", seq, "--coverage", "2", "--maxradius", str(radius), "--trim"]
    trees = {}
    for on in ("host", "gpu"):
        out = str(tmp_path / on)
        p = _run(cli, "environment-assembler-finder", base + ["-o", out, "--trim-on", on], tmp_path / ("wd_" + on))
        assert p.returncode == 0, p.stderr[-2000:]
        assert p.stderr.count(GPU_LINE) == (2 if on == "gpu" else 0)
        trees[on] = _tree(out)
    assert "cutReads0.fasta" in trees["gpu"] and trees["gpu"] == trees["host"]
    want = _oracle(reads, seq, k, po.KEY_PACKED, str(tmp_path / "want"), n_seqs=1, coverage=2, max_radius=radius, trim=True)
    (files,) = want.values()
    for name, text in files.items():
        assert trees["gpu"][name].decode() == text, name
    untrimmed = _oracle(reads, seq, k, po.KEY_PACKED, str(tmp_path / "untrimmed"), n_seqs=1, coverage=2, max_radius=radius, trim=False)
    (files0,) = untrimmed.values()
    assert 0 < len(files["graph.txt"].splitlines()) < len(files0["graph.txt"].splitlines())


def test_the_options_handling(cli, tmp_path):
    k = 21
    reads, seq, radius = _inputs(tmp_path, k, 3)
    base = ["-k", str(k), "-i", reads, "--seq", seq, "--coverage", "2", "--maxradius", str(radius), "--merge", "true"]
    trees = {}
    for name, extra in (("plain", []), ("gpu", ["--trim-on", "gpu"])):  # without --trim: accepted, and nothing changes
        out = str(tmp_path / name)
        p = _run(cli, "environment-finder", base + ["-o", out] + extra, tmp_path / ("wd_" + name))
        assert p.returncode == 0, p.stderr[-2000:]
        assert GPU_LINE not in p.stderr
        trees[name] = _tree(out)
    assert trees["plain"] and trees["plain"] == trees["gpu"]
    out = str(tmp_path / "auto")  # auto on a pass this small: the host, and no new log line
    p = _run(cli, "environment-finder", base + ["-o", out, "--trim"], tmp_path / "wd_auto")
    assert p.returncode == 0 and GPU_LINE not in p.stderr and "mc_trim_paths" not in p.stderr
    for tool in ("environment-finder", "environment-assembler-finder"):
        p = _run(cli, tool, base[:8] + ["-o", str(tmp_path / "bad"), "--trim", "--trim-on", "cpu"], tmp_path / "wd_bad")
        assert p.returncode != 0 and all(w in p.stderr + p.stdout for w in ("--trim-on", "host", "gpu", "auto", "'cpu'")), p.stderr[-500:]
    p = _run(cli, "environment-finder", base + ["-o", str(tmp_path / "bad"), "--trim", "--trim-on", "gpu", "--devices", "0"], tmp_path / "wd_bad")
    assert p.returncode != 0 and "--trim-on gpu does not go with --devices" in p.stderr + p.stdout
    p = _run(cli, "kmer-counter", ["-k", str(k), "-i", reads, "--trim-on", "gpu"], tmp_path / "wd_bad")
    assert p.returncode != 0 and "--trim-on does not apply to --tool kmer-counter" in p.stderr + p.stdout
    assert not os.path.exists(str(tmp_path / "bad"))
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=120)
    assert "--trim-on host|gpu|auto" in p.stdout
