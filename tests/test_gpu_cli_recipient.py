"""GPU: `metacherchant --tool recipient-visualiser` end to end -- every comp_* file byte-identical to the model's
(tests/recipient_model.py) over the oracle's tables, the set of files, the log lines, and the refusals."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import recipient_model as rm
from tests.helpers import synth_case

pytestmark = pytest.mark.gpu

GENOME = 30000
L = 100


@pytest.fixture(scope="module")
def cli():
    from metacherchant_amd import build
    build.build_all()
    return build.CLI


def _write_reads(path, reads):
    """reads (strings) as FASTA, FASTQ or either gzipped, by the path's suffix"""
    if ".fastq" in path:
        data = "".join("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(reads))
    else:
        data = "".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads))
    with open(path, "wb") as f:
        f.write(gzip.compress(data.encode()) if path.endswith(".gz") else data.encode())


def _inputs(k):
    """The after reads: a thin read set over a genome and a mutated copy of its first third (branches).  The class files: the reads
    that start in one of eight stretches of the genome go to the classes whose bit the stretch's number (1, 2, 4, 8, 3, 12, 0, 15)
    has, mate by mate (_1, _2, _s by the read's number), so k-mers of every mask lie along the genome.  The sequences: genes across
    the stretches, a reverse complement, one with N, one shorter than k, random ones that the graph does not hold."""
    genome, reads, off = synth_case(1, GENOME, 2400, L, 50)
    rng = np.random.default_rng(7 + k)
    variant = genome[:GENOME // 3].copy()
    for p in rng.integers(100, GENOME // 3 - 100, 40):
        variant[p] = (variant[p] + 1) & 3
    after = [po.decode(reads[int(off[r]):int(off[r + 1])]) for r in range(len(off) - 1)]
    starts = []
    for r in after:  # (where a read lies: its first 20 bases, or their reverse complement, in the genome)
        g = po.decode(genome)
        at = g.find(r[:24])
        if at < 0:
            at = g.find(rm.reverse_complement(r)[:24])
        starts.append(at)
    for s in range(0, GENOME // 3 - L, 45):
        after.append(po.decode(variant[s:s + L]))
        starts.append(-1)
    stretch_masks = (1, 2, 4, 8, 3, 12, 0, 15)
    files = {"%s_%s" % (c, m): [] for c in rm.CLASS_NAMES for m in "12s"}
    for i, (r, at) in enumerate(zip(after, starts)):
        if at < 0:
            continue
        mask = stretch_masks[(at * len(stretch_masks)) // GENOME]
        for t, c in enumerate(rm.CLASS_NAMES):
            if mask >> t & 1:
                files["%s_%s" % (c, "12s"[i % 3])].append(r)
    with_n = list(po.decode(genome[20000:20000 + 150]))
    with_n[40] = with_n[90] = "N"
    seqs = [po.decode(genome[3700:3700 + 200]), rm.reverse_complement(po.decode(genome[7400:7400 + 150])), po.decode(genome[11200:11200 + 120]),
            po.decode(rng.integers(0, 4, 120).astype(np.uint8)), po.decode(genome[15000:15000 + k - 1]), "".join(with_n),
            po.decode(genome[18700:18700 + 130]), po.decode(genome[22400:22400 + k]), po.decode(rng.integers(0, 4, k).astype(np.uint8)),
            po.decode(genome[26200:26200 + 140]), po.decode(variant[5000:5000 + 90])]
    return after, files, seqs


def _table(reads, k, mode):
    t = po.Table()
    for r in reads:
        c = po.encode(r)
        t.count_reads(c, np.array([0, len(c)], dtype=np.uint64), k, mode)
    return t


CASES = [(31, 0, [], "fasta", ["--maxkmers", "300"]), (41, 1, [], "fastq", ["--maxradius", "25"]),
         (41, 2, ["--hash", "fnv1a"], "fastq.gz", ["--maxkmers", "150", "--maxradius", "40"])]


@pytest.mark.parametrize("k,mode,hash_args,ext,limits", CASES)
def test_recipient_visualiser_files_are_the_models(cli, tmp_path, k, mode, hash_args, ext, limits):
    after, class_reads, seqs = _inputs(k)
    in_dir, out, wd = str(tmp_path / "in"), str(tmp_path / "out"), str(tmp_path / "wd")
    os.makedirs(in_dir)
    for name, reads in class_reads.items():
        _write_reads(os.path.join(in_dir, name + "." + ext), reads)
    after_paths = [str(tmp_path / "after_1.fasta"), str(tmp_path / "after_2.fastq.gz")]
    _write_reads(after_paths[0], after[0::2])
    _write_reads(after_paths[1], after[1::2])
    seq_path = str(tmp_path / "genes.fasta")
    with open(seq_path, "w") as f:
        f.write("".join(">g%d\n%s\n%s\n" % (i, s[:60], s[60:]) for i, s in enumerate(seqs)))
    graph = _table(after, k, mode)
    classes = [_table([r for m in "12s" for r in class_reads["%s_%s" % (c, m)]], k, mode) for c in rm.CLASS_NAMES]
    lim = dict(zip(limits[0::2], limits[1::2]))
    mk = int(lim["--maxkmers"]) if "--maxkmers" in lim else None
    mr = int(lim.get("--maxradius", 1000))
    want, want_log, envs = rm.recipient_visualiser(k, mode, graph, classes, [s.replace("N", "A") for s in seqs], max_kmers=mk, max_radius=mr)
    # the test's own input, on the model's output: all six colours; sequences that write nothing; --maxkmers cutting a level
    colours = {ln.split("CL:Z:")[1] for name, text in want.items() if name.endswith(".gfa") for ln in text.splitlines() if ln[0] == "S"}
    assert colours == {"RED", "GREEN", "BLUE", "GREY", "YELLOW", "BLACK"}, colours
    silent = [i for i, e in enumerate(envs) if e.nodes is None]
    assert len(silent) >= 3 and len(silent) < len(seqs) and len(want) == 2 * (len(seqs) - len(silent))
    if mk is not None:
        assert any(e.cut_a_level for e in envs)
    assert any(int(ln.split()[3]) > 0 for ln in want_log if ln.startswith("Extending"))

    cmd = [cli, "--tool", "recipient-visualiser", "-k", str(k), "-after"] + after_paths + ["-seq", seq_path, "-i", in_dir, "-ext", ext, "-o", out,
                                                                                          "-w", wd, "--force"] + limits + hash_args
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    got = {}
    for root, _, names in os.walk(out):
        for n in names:
            got[os.path.relpath(os.path.join(root, n), out)] = open(os.path.join(root, n)).read()
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        if got[name] != want[name]:
            g, w = got[name].split("\n"), want[name].split("\n")
            bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
            raise AssertionError((name, len(g), len(w), bad[:3], g[bad[0]][:300] if bad else None, w[bad[0]][:300] if bad else None))
    log = open(os.path.join(wd, "log")).read()
    assert re.findall(r"Hashtable size: (\d+) kmers", log) == [str(t.size()) for t in [graph] + classes]
    steps = [ln.split(": ", 1)[1] for ln in log.splitlines() if re.search(r"INFO: (Extending endings|Could not find any|Finished processing)", ln)]
    assert steps == want_log
    order = [log.index(s) for s in ("Loading after reads ...", "Hashtable size", "Creating after images ...", "Finished processing all sequences!")]
    assert order == sorted(order)
    assert (log.count("Using default polynomial hash function"), log.count("Using FNV1a hash function")) == ((0, 0), (1, 0), (0, 1))[mode]
    assert os.path.exists(os.path.join(wd, "SUCCESS"))


def test_recipient_visualiser_refusals(cli, tmp_path):
    in_dir = str(tmp_path / "in")
    os.makedirs(in_dir)
    for c in rm.CLASS_NAMES:
        for m in "12s":
            _write_reads(os.path.join(in_dir, "%s_%s.fasta" % (c, m)), ["ACGTACGTACGTAGCTAGCTAGCATCGATCGATCAGCTACGACTAGCATCAGC"])
    _write_reads(str(tmp_path / "a.fasta"), ["ACGTACGTACGTAGCTAGCTAGCATCGATCGATCAGCTACGACTAGCATCAGC"])
    _write_reads(str(tmp_path / "s.fasta"), ["ACGTACGTACGTAGCTAGCTAGCATCGATCGATCAGCTACGACTAGCATCAGC"])
    full = {"-k": "31", "-after": str(tmp_path / "a.fasta"), "-seq": str(tmp_path / "s.fasta"), "-i": in_dir, "-ext": "fasta"}
    names = {"-k": "k", "-after": "after-files", "-seq": "seq", "-i": "input-dir", "-ext": "ext"}

    def run(args, extra=()):
        a = [x for key, v in args.items() for x in (key, v)]
        p = subprocess.run([cli, "--tool", "recipient-visualiser", "-w", str(tmp_path / "wd"), "-o", str(tmp_path / "out"), "--force"] + a + list(extra),
                           capture_output=True, text=True, timeout=300)
        return p.returncode, p.stderr + p.stdout

    for missing in full:
        rc, text = run({key: v for key, v in full.items() if key != missing})
        assert rc == 1 and "Parameter '%s' is mandatory" % names[missing] in text, (missing, text)
    rc, text = run(dict(full, **{"-k": "64"}))
    assert rc == 1 and "k = 64 is not supported" in text
    rc, text = run(full, ["--devices", "0,1"])
    assert rc == 1 and "--devices is for --tool environment-finder" in text
    rc, text = run(full, ["--coverage", "2"])
    assert rc == 1 and "Unrecognized option: --coverage" in text
    os.remove(os.path.join(in_dir, "came_from_both_s.fasta"))
    rc, text = run(full)
    assert rc == 1 and "came_from_both_s.fasta" in text
    assert not os.path.exists(str(tmp_path / "out"))  # nothing was written by any of them
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=120)
    assert "--tool recipient-visualiser" in p.stdout and "--after-files" in p.stdout and "--input-dir" in p.stdout
