"""GPU: `metacherchant --tool triple-reads-classifier` end to end -- all nine files byte-identical to the model
(tests/triple_classifier_model.py) over the oracle's tables, and the statistics lines in the log."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import classifier_model as cm
from tests import triple_classifier_model as tm
from tests.helpers import synth_case
from tests.test_gpu_cli_classifier import _queries, _write_fastq

pytestmark = pytest.mark.gpu

OUTS = tuple("%s_%s.fastq" % (c, s) for c in ("found", "half_found", "not_found") for s in ("1", "2", "s"))


@pytest.fixture(scope="module")
def cli():
    from metacherchant_amd import build
    build.build_all()
    return build.CLI


CASES = {
    # name: (k, mode, k2, mode2, graph source, read-file suffix, extra flags, found, half, z, correction)
    "reads_21_41": (21, 0, 41, 1, "reads", ".fastq", [], 90, 40, 1.0, False),
    "kmers_bin_31_63_fnv1a_corr": (31, 0, 63, 2, "kmers.bin", ".fastq", ["--hash", "fnv1a", "-corr", "--interval95"], 90, 40, 1.96, True),
    "gz_25_31_half0": (25, 0, 31, 0, "reads", ".fastq.gz", ["-found", "80", "-half", "0", "--correction", "true"], 80, 0, 1.0, True),
}


def _graph(tmp_path):
    genome, reads, _ = synth_case(1, 20000, 3000, 150, 50)
    graph = str(tmp_path / "graph.fastq")
    with open(graph, "w") as f:
        for i in range(3000):
            f.write("@g%d\n%s\n+\n%s\n" % (i, po.decode(reads[i * 150:(i + 1) * 150]), "h" * 150))
    return genome, reads, graph


def _getter(reads, k, mode):
    t = po.Table()
    t.count_reads(reads, np.arange(3001, dtype=np.uint64) * 150, k, mode)
    return cm.table_getter(t, k, mode), t.size()


def _kmer_counter(cli, tmp_path, graph, k, extra):
    out = tmp_path / ("kc%d" % k)
    p = subprocess.run([cli, "--tool", "kmer-counter", "-k", str(k), "-i", graph, "-w", str(tmp_path / ("wd_kc%d" % k)), "--output-dir", str(out)] + extra,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    return str(out / "graph.kmers.bin")


@pytest.mark.parametrize("name", sorted(CASES))
def test_cli_triple_reads_classifier_matches_the_model(cli, tmp_path, name):
    k, mode, k2, mode2, source, suffix, extra, found, half, z, corr = CASES[name]
    genome, reads, graph = _graph(tmp_path)
    get1, size1 = _getter(reads, k, mode)
    get2, size2 = _getter(reads, k2, mode2)
    rng = np.random.default_rng(sum(map(ord, name)))
    q1 = _queries(genome, 700, rng, with_n=True)
    q2 = _queries(genome, 610, rng, with_n=True)  # (the second file shorter: pairs end with it)
    for i in range(0, 600, 9):  # copies of earlier first mates with other qualities: the last copy decides their class
        j = int(rng.integers(0, i + 1))
        c, ph, n_pos = q1[j]
        ph = ph.copy()
        ph[int(rng.integers(0, len(ph)))] = int(rng.integers(1, 10)) if rng.integers(0, 2) else 30
        q1[i] = (c.copy(), ph, list(n_pos))
    for i in range(5, 600, 13):  # empty second mates
        q2[i] = (np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), [])
    files = [str(tmp_path / ("r_1" + suffix)), str(tmp_path / ("r_2" + suffix))]
    _write_fastq(files[0], q1, 64)
    _write_fastq(files[1], q2, 33)
    sets = [[(c, ph) for c, ph, _ in q] for q in (q1, q2)]
    pairs = list(zip(sets[0], sets[1]))
    if source == "reads":
        graph_args = ["-i", graph]
    else:
        h = ["--hash", "fnv1a"] if "fnv1a" in extra else []
        graph_args = ["-ik1", _kmer_counter(cli, tmp_path, graph, k, h), "-ik2", _kmer_counter(cli, tmp_path, graph, k2, h)]
    out, wd = str(tmp_path / "out"), str(tmp_path / "wd")
    cmd = [cli, "--tool", "triple-reads-classifier", "-k", str(k), "-k2", str(k2)] + graph_args + ["-r"] + files + ["-o", out, "-w", wd] + extra
    cls = tm.classes(pairs, k, k2, get1, get2, found, half, z, corr)
    both, single = tm.route(pairs, cls)
    empty_found_2 = any(len(b[0]) == 0 for _, b in both[tm.FOUND])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if empty_found_2:  # (found_2.fastq is not filtered: the reference's writer fails)
        assert p.returncode == 1 and "Empty DnaQ!" in p.stderr, p.stderr[-2000:]
        pytest.fail("the case should not put an empty read into found_2")
    assert p.returncode == 0, p.stderr[-3000:]
    want = tm.outputs(both, single)
    for f in OUTS:
        with open(os.path.join(out, f), "rb") as fh:
            assert fh.read() == want[f], (name, f)
    for line in tm.stats_lines(both, single):
        assert line in p.stderr, (line, p.stderr[-2000:])
    assert "Hashtable size: %d kmers" % size1 in p.stderr and "Hashtable size: %d kmers" % size2 in p.stderr
    log = p.stderr
    order = ["Loading reads...", "Building graph with k = %d ..." % k, "Building graph with k = %d ..." % k2, "|\tTotal: ",
             "|\tHalf found: ", "Writing classified reads...", "Reads have been written. Finishing..."]
    assert [log.find(s) for s in order] == sorted(log.find(s) for s in order) and all(log.find(s) >= 0 for s in order)
    assert log.count("Searching for corrected reads in graph..." if corr else "Searching for reads in graph...") == 2
    assert os.path.exists(os.path.join(wd, "SUCCESS"))
    # the case covers every class, mixed pairs, and reads whose pass-1 class comes from a later copy
    assert len(both[tm.FOUND]) and len(single[tm.FOUND]) and len(single[tm.HALF_FOUND])
    if half:  # (with -half 0 every read reaches HALF_FOUND)
        assert len(both[tm.NOT_FOUND]) and len(single[tm.NOT_FOUND])
    last = tm.last_copy([pr[0][0] for pr in pairs])
    assert any(last[i] != i for i in range(len(pairs)))


def test_cli_triple_reads_classifier_empty_second_mates(cli, tmp_path):
    """Empty second mates share the key "": the class of the last pair with one decides all of them in pass 2.  found_2.fastq is
    not filtered, as in the reference, but an empty mate 2 never reaches it: found_2 = !found_1 at both k, so mate 1 and mate 2
    are never both FOUND -- the run succeeds and the empty reads are counted, not written."""
    genome, reads, graph = _graph(tmp_path)
    absent = "ACGT" * 30
    firsts = [absent, po.decode(genome[100:220]), po.decode(genome[5000:5120]), absent[:60]]
    r1, r2 = str(tmp_path / "p_1.fastq"), str(tmp_path / "p_2.fastq")
    with open(r1, "w") as f:
        for i, s in enumerate(firsts):
            f.write("@a%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
    with open(r2, "w") as f:
        for i in range(len(firsts)):
            f.write("@a%d\n\n+\n\n" % i)
    get1, _ = _getter(reads, 21, 0)
    get2, _ = _getter(reads, 31, 0)
    pairs = [((np.array(["AGCT".index(c) for c in s], np.uint8), np.full(len(s), 9, np.uint8)), cm.EMPTY) for s in firsts]
    cls = tm.classes(pairs, 21, 31, get1, get2)
    assert cls[1] == (tm.FOUND, tm.HALF_FOUND) and cls[0][1] == tm.FOUND  # (the key "": the last pair's mate 1 is not found, so "" was FOUND)
    both, single = tm.route(pairs, cls)
    p = subprocess.run([cli, "-t", "triple-reads-classifier", "-k", "21", "-k2", "31", "-i", graph, "-r", r1, r2, "-w", str(tmp_path / "wd"),
                        "-o", str(tmp_path / "o")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    for f, data in tm.outputs(both, single).items():
        with open(os.path.join(str(tmp_path / "o"), f), "rb") as fh:
            assert fh.read() == data, f
    for line in tm.stats_lines(both, single):
        assert line in p.stderr, (line, p.stderr[-2000:])
