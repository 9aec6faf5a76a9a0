"""GPU: `metacherchant --tool seq-cov` end to end -- seq_cov.csv byte-identical to the model (tests/seq_cov_model.py) over the
oracle's tables, the four `Hashtable size` lines, and the refusals."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import seq_cov_model as sm
from tests.helpers import synth_case

pytestmark = pytest.mark.gpu

GENOME = 60000
BINS = ("donor", "before", "both", "itself")  # the reference's order of columns and of loading


@pytest.fixture(scope="module")
def cli():
    from metacherchant_amd import build
    build.build_all()
    return build.CLI


def _bin_reads(i):
    """bin i's reads: another part of the read set and another depth for each bin"""
    first, n = ((0, 1500), (1500, 2500), (4000, 800), (4800, 3000))[i]
    _, reads, off = synth_case(1, GENOME, n, 150, 100, first_read=first)
    return reads, off


def _sequences(genome, k, rng):
    """(codes, positions printed as N): reads, one of length k, k - 1 (NaN), k - 2 (-0.0), one with N, and a 100 kbase sequence of
    random bases of which exactly one window is the genome's (an E- value)"""
    seqs = []
    for i in range(40):
        L = int(rng.integers(60, 300))
        s = int(rng.integers(0, GENOME - L))
        r = genome[s:s + L].copy()
        if i % 4 == 1:
            r = (3 - r[::-1]).astype(np.uint8)
        if i % 7 == 3:
            r = rng.integers(0, 4, L).astype(np.uint8)
        seqs.append((r, []))
    seqs.append((genome[500:500 + k].copy(), []))
    seqs.append((genome[700:700 + k - 1].copy(), []))
    seqs.append((genome[900:900 + k - 2].copy(), []))
    with_n = genome[2000:2200].copy()
    with_n[[50, 120]] = 0
    seqs.append((with_n, [50, 120]))
    big = rng.integers(0, 4, 100000).astype(np.uint8)
    big[40000:40000 + k] = genome[3000:3000 + k]
    seqs.insert(20, (big, []))
    return seqs


def _text(codes, n_pos):
    s = list(po.decode(codes))
    for p in n_pos:
        s[p] = "N"
    return "".join(s)


def _write_sequences(path, seqs):
    if ".fastq" in path:
        data = "".join("@s%d\n%s\n+\n%s\n" % (i, _text(c, n), "".join("#" if j in n else "I" for j in range(len(c)))) for i, (c, n) in enumerate(seqs))
    else:
        data = "".join(">s%d\n%s\n%s\n" % (i, _text(c, n)[:70], _text(c, n)[70:]) for i, (c, n) in enumerate(seqs))
    with open(path, "wb") as f:
        f.write(gzip.compress(data.encode()) if path.endswith(".gz") else data.encode())


@pytest.mark.parametrize("k,mode,hash_args,suffix", [(31, 0, [], ".fasta"), (41, 1, [], ".fastq.gz"), (41, 2, ["--hash", "fnv1a"], ".fasta")])
def test_seq_cov_csv_is_the_models(cli, tmp_path, k, mode, hash_args, suffix):
    genome = po.synth_genome(20240531, GENOME)
    tables, paths = [], {}
    for i, name in enumerate(BINS):
        reads, off = _bin_reads(i)
        t = po.Table()
        t.count_reads(reads, off, k, mode)
        tables.append(t)
        paths[name] = str(tmp_path / (name + ".fasta"))
        with open(paths[name], "w") as f:
            for r in range(len(off) - 1):
                f.write(">r%d\n%s\n" % (r, po.decode(reads[int(off[r]):int(off[r + 1])])))
    seqs = _sequences(genome, k, np.random.default_rng(k))
    seq_path = str(tmp_path / ("seqs" + suffix))
    _write_sequences(seq_path, seqs)
    # the model's file
    lines = [sm.HEADER]
    for codes, _ in seqs:
        wk = sm.window_keys(codes, k, mode)
        covs = []
        for t in tables:
            keys, counts = t.dump()
            at = np.minimum(np.searchsorted(keys, wk), len(keys) - 1)
            covs.append(np.where(keys[at] == wk, np.maximum(counts[at].astype(np.int64), 0), 0).tolist() if len(wk) else [])
        lines.append(sm.csv_row(codes, k, covs))
    want = "\n".join(lines) + "\n"
    # the test's own input: rows of NaN, of -0.0, of an E- value, a sequence with N printed as A, and columns that differ
    assert ", NaN" * 8 + "\n" in want and ", -0.0" * 8 + "\n" in want and re.search(r", \d\.\d+E-\d", want)
    n_row = [ln for ln, (c, n) in zip(lines[1:], seqs) if n][0]
    assert "N" not in n_row and n_row.startswith(po.decode(seqs[-1][0])) and _text(*seqs[-1]).count("N") == 2
    cols = np.array([[float(x) for x in ln.split(", ")[1:]] for ln in lines[1:41]])
    assert all(not np.array_equal(cols[:, 2 * a], cols[:, 2 * b]) for a in range(4) for b in range(a))
    assert (cols > 0).any(axis=0).all() and (cols == 0).any(axis=0).all()
    # the four options in another order than the columns'
    wd, out = str(tmp_path / "wd"), str(tmp_path / "out")
    cmd = [cli, "--tool", "seq-cov", "-k", str(k), "--itself", paths["itself"], "--from-both", paths["both"], "--from-before", paths["before"],
           "--from-donor", paths["donor"], "-r", seq_path, "-o", out, "-w", wd, "--force"] + hash_args
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    got = open(os.path.join(out, "seq_cov.csv")).read()
    if got != want:
        g, w = got.split("\n"), want.split("\n")
        bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
        raise AssertionError((len(g), len(w), bad[:3], g[bad[0]][-200:] if bad else None, w[bad[0]][-200:] if bad else None))
    log = open(os.path.join(wd, "log")).read()
    assert re.findall(r"Hashtable size: (\d+) kmers", log) == [str(t.size()) for t in tables]
    order = [log.index(s) for s in ("Loading bins ...", "Hashtable size", "Calculating sequence coverage...", "Processed all sequences...")]
    assert order == sorted(order)
    assert (log.count("Using default polynomial hash function"), log.count("Using FNV1a hash function")) == ((0, 0), (4, 0), (0, 4))[mode]
    assert os.path.exists(os.path.join(wd, "SUCCESS"))
    # --continue: nothing to do; default output directory
    p = subprocess.run(cmd + ["--continue"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "already finished" in p.stderr + p.stdout + open(os.path.join(wd, "log")).read()


def test_seq_cov_refusals(cli, tmp_path):
    full = {"-k": "31", "--from-before": "b.fa", "--from-donor": "d.fa", "--from-both": "x.fa", "--itself": "i.fa", "-r": "s.fa"}
    names = {"-k": "k", "--from-before": "from-before", "--from-donor": "from-donor", "--from-both": "from-both", "--itself": "itself", "-r": "read-file"}
    for missing in full:
        args = [a for key, v in full.items() if key != missing for a in (key, v)]
        p = subprocess.run([cli, "--tool", "seq-cov", "-w", str(tmp_path / "wd")] + args, capture_output=True, text=True, timeout=120)
        assert p.returncode == 1 and "Parameter '%s' is mandatory" % names[missing] in p.stderr + p.stdout, (missing, p.stderr)
    args = [a for key, v in dict(full, **{"-k": "64"}).items() for a in (key, v)]
    p = subprocess.run([cli, "--tool", "seq-cov", "-w", str(tmp_path / "wd")] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "k = 64 is not supported" in p.stderr + p.stdout
    p = subprocess.run([cli, "--tool", "seq-cov", "--forcehash"] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "Unrecognized option: --forcehash" in p.stderr + p.stdout
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=120)
    assert "--tool seq-cov" in p.stdout and "--from-donor" in p.stdout
    p = subprocess.run([cli, "--tool", "fmt-visualiser"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "not part of this build" in p.stderr + p.stdout and "seq-cov are" in p.stderr + p.stdout
