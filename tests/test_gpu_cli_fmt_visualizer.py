"""GPU: `metacherchant --tool fmt-visualizer` end to end -- every file under donor/, before/ and after/ byte-identical to the model's
(tests/components_model.py), the set of files, the log lines, and the refusals."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import components_model as cm
from tests.test_gpu_cli_recipient import _write_reads

pytestmark = pytest.mark.gpu

CLASSES = [c for _, cs in cm.PHASES for c in cs]


@pytest.fixture(scope="module")
def cli():
    from metacherchant_amd import build
    build.build_all()
    return build.CLI


def _rand(rng, n):
    return po.decode(rng.integers(0, 4, n).astype(np.uint8))


def _phase_inputs(rng, k, classes):
    """A dozen loci of 3k bases tiled by overlapping reads, one of them with a one-base variant in the middle (a bubble: a k-mer queued
    twice), one read twice, one read as its reverse complement, a read shorter than k; locus j goes to the classes whose bits its mask
    has -- one class each, then several, then none, in turn -- so that every colour of the phase's rule occurs."""
    reads, locus_of = [], []
    for j in range(12):
        g = _rand(rng, 3 * k)
        tiles = [g[s:s + 2 * k] for s in range(0, k + 1, k // 2)]
        if j == 3:
            v = g[:3 * k // 2] + "ACGT"[("ACGT".index(g[3 * k // 2]) + 1) % 4] + g[3 * k // 2 + 1:]
            tiles += [v[k // 2:k // 2 + 2 * k]]
        if j == 5:
            tiles += [tiles[0]]
        if j == 7:
            tiles[1] = cm.reverse_complement(tiles[1])
        reads += tiles
        locus_of += [j] * len(tiles)
    reads.append(_rand(rng, k - 1))
    locus_of.append(99)
    class_reads = {}
    masks = (1, 2, 3, 0) if len(classes) == 2 else (1, 2, 4, 8, 9, 0)
    for t, c in enumerate(classes):
        class_reads[c] = [r for r, j in zip(reads, locus_of) if j != 99 and masks[j % len(masks)] >> t & 1]
    return reads, class_reads


@pytest.mark.parametrize("k,mode,ext", [(21, 0, "fasta"), (41, 1, "fastq")])
def test_fmt_visualizer_files_are_the_models(cli, tmp_path, k, mode, ext):
    rng = np.random.default_rng(100 + k)
    inputs = {name: _phase_inputs(rng, k, classes) for name, classes in cm.PHASES}
    want, comps = cm.fmt_visualizer(k, mode, inputs)
    # the test's own input, on the model's output: up to 40 components a phase, a coverage of 0, colours of both rules
    assert all(10 <= len(comps[p]) <= 40 for p in comps), {p: len(comps[p]) for p in comps}
    assert all(any("\tKC:i:0\t" in text.decode() for n, text in want.items() if n.startswith(p) and n.endswith(".gfa")) for p in comps)
    colours = {p: {ln.split("CL:Z:")[1] for n, text in want.items() if n.startswith(p) and n.endswith(".gfa")
                   for ln in text.decode().splitlines() if ln[0] == "S"} for p in comps}
    assert colours["donor"] == colours["before"] == {"GREEN", "BLUE", "GREY", "BLACK"}, colours
    assert colours["after"] == {"RED", "BLUE", "GREEN", "YELLOW", "GREY", "BLACK"}, colours

    in_dir, out, wd = str(tmp_path / "in"), str(tmp_path / "out"), str(tmp_path / "wd")
    os.makedirs(in_dir)
    paths = {}
    for name, classes in cm.PHASES:
        reads, class_reads = inputs[name]
        paths[name] = [str(tmp_path / ("%s_a.fasta" % name)), str(tmp_path / ("%s_b.fastq" % name))]
        _write_reads(paths[name][0], reads[:len(reads) // 2])  # (file order is scan order)
        _write_reads(paths[name][1], reads[len(reads) // 2:])
        for c in classes:
            for i, m in enumerate("12s"):
                _write_reads(os.path.join(in_dir, "%s_%s.%s" % (c, m, ext)), class_reads[c][i::3])
    cmd = [cli, "--tool", "fmt-visualizer", "-k", str(k), "-donor"] + paths["donor"] + ["-before"] + paths["before"] + ["-after"] + paths["after"] + [
        "-i", in_dir, "-ext", ext, "-o", out, "-w", wd, "--force", "-p", "4"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    got = {}
    for root, _, names in os.walk(out):
        for n in names:
            got[os.path.relpath(os.path.join(root, n), out)] = open(os.path.join(root, n), "rb").read()
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        if got[name] != want[name]:
            g, w = got[name].decode().split("\n"), want[name].decode().split("\n")
            bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
            raise AssertionError((name, len(g), len(w), bad[:3], g[bad[0]][:300] if bad else None, w[bad[0]][:300] if bad else None))
    log = open(os.path.join(wd, "log")).read()
    order = [log.index(s) for s in ("Loading donor reads ...", "Creating donor image ...", "Loading before reads ...", "Creating before image ...",
                                    "Loading after reads ...", "Creating after image ...")]
    assert order == sorted(order)
    assert log.count("Reading hashes of k-mers instead") == (3 if k > 31 else 0)
    assert log.count("Using default polynomial hash function") == (3 if k > 31 else 0)
    assert log.count("Hashtable size") == 3 + 2 + 2 + 4
    assert os.path.exists(os.path.join(wd, "SUCCESS"))


def test_fmt_visualizer_refusals(cli, tmp_path):
    in_dir = str(tmp_path / "in")
    os.makedirs(in_dir)
    read = "ACGTACGTACGTAGCTAGCTAGCATCGATCGATCAGCTACGACTAGCATCAGC"
    for c in CLASSES:
        for m in "12s":
            _write_reads(os.path.join(in_dir, "%s_%s.fasta" % (c, m)), [read])
    for n in "dba":
        _write_reads(str(tmp_path / (n + ".fasta")), [read])
    full = {"-k": "31", "-donor": str(tmp_path / "d.fasta"), "-before": str(tmp_path / "b.fasta"), "-after": str(tmp_path / "a.fasta"), "-i": in_dir,
            "-ext": "fasta"}
    names = {"-k": "k", "-donor": "donor-files", "-before": "before-files", "-after": "after-files", "-i": "input-dir", "-ext": "ext"}

    def run(args, extra=(), tool="fmt-visualizer"):
        a = [x for key, v in args.items() for x in (key, v)]
        p = subprocess.run([cli, "--tool", tool, "-w", str(tmp_path / "wd"), "-o", str(tmp_path / "out"), "--force"] + a + list(extra),
                           capture_output=True, text=True, timeout=300)
        return p.returncode, p.stderr + p.stdout

    for missing in full:
        rc, text = run({key: v for key, v in full.items() if key != missing})
        assert rc == 1 and "Parameter '%s' is mandatory" % names[missing] in text, (missing, text)
    rc, text = run(dict(full, **{"-k": "64"}))
    assert rc == 1 and "k = 64 is not supported" in text
    rc, text = run(full, ["--devices", "0,1"])
    assert rc == 1 and "--devices is for --tool environment-finder" in text
    rc, text = run(full, ["--maxkmers", "2"])
    assert rc == 1 and "Unrecognized option: --maxkmers" in text
    assert not os.path.exists(str(tmp_path / "out"))  # nothing was written by any of them
    rc, text = run({}, tool="fmt-visualiser")  # (with an s: no defined output, still refused)
    assert rc == 1 and "is not part of this build" in text and "fmt-visualizer and seq-cov are" in text
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=120)
    assert "--tool fmt-visualizer" in p.stdout and "--donor-files" in p.stdout and "--before-files" in p.stdout
