"""CPU: the triple-reads-classifier's model (tests/triple_classifier_model.py) on hand-worked cases, and the CLI's refusals, which
come before any device is opened."""
import os
import subprocess

import numpy as np
import pytest

from tests import classifier_model as cm
from tests import triple_classifier_model as tm

F, H, N = tm.FOUND, tm.HALF_FOUND, tm.NOT_FOUND


def _read(s, low=()):
    codes = np.array(["AGCT".index(c) for c in s], dtype=np.uint8)
    phred = np.full(len(s), 30, dtype=np.uint8)
    for p in low:
        phred[p] = 5
    return codes, phred


def _getter(truth, k):
    """a graph of the k-mers of the strings in truth, every one counted 5 times"""
    kmers = {bytes(bytearray("AGCT".index(c) for c in t[i:i + k])) for t in truth for i in range(len(t) - k + 1)}
    return lambda w: 5 if bytes(bytearray(int(x) for x in w)) in kmers else -1


def test_pass2_truth_table():
    half = 0.4
    for f in (False, True):
        for c1 in (N, H, F):
            for w in (0.0, 0.5):
                got = tm.class_pass2(f, c1, w, half)
                want = F if f and c1 == F else H if f or c1 == F or (w >= half and c1 == H) else N
                assert got == want
    assert tm.class_pass2(True, F, 0.0, half) == F
    assert tm.class_pass2(True, N, 0.0, half) == H and tm.class_pass2(False, F, 0.0, half) == H
    assert tm.class_pass2(False, H, 0.5, half) == H and tm.class_pass2(False, H, 0.3, half) == N
    assert tm.class_pass2(False, N, 1.0, half) == N
    assert [tm.class_pass1(True, 0, 0.4), tm.class_pass1(False, 0.4, 0.4), tm.class_pass1(False, 0.39, 0.4)] == [F, H, N]


def test_width_is_that_of_the_read_as_given():
    T = "ACGTTGCAAGTC"
    get = _getter([T], 4)
    assert tm.width(_read(T)[0], 4, get) == 1.0
    assert tm.width(_read("ACG")[0], 4, get) == 0.0
    X = T[:6] + ("A" if T[6] != "A" else "C") + T[7:]
    assert tm.width(_read(X)[0], 4, get) == (5 + 3) / 12  # windows 3..6 cover the error; the last one is present


def test_half_zero_makes_an_empty_read_half_found():
    T = "ACGTTGCAAGTC"
    pairs = [(cm.EMPTY, _read(T))]
    get1, get2 = _getter([T], 4), _getter([T], 5)
    assert tm.classes(pairs, 4, 5, get1, get2, half_pct=0) == [(H, F)]
    assert tm.classes(pairs, 4, 5, get1, get2, half_pct=40) == [(N, F)]


def test_empty_mate_2_records_share_one_key():
    T, U = "ACGTTGCAAGTC", "TTTTGGGGCCCCAAAA"
    get1, get2 = _getter([T], 4), _getter([T], 5)
    pairs = [(_read(T), cm.EMPTY), (_read(U), cm.EMPTY)]
    # pass 1: found_2 = !found_1, so the first empty mate is NOT and the second FOUND; the key "" keeps the last: FOUND
    assert tm.classes(pairs, 4, 5, get1, get2) == [(F, H), (N, F)]
    # one pair alone: its own pass-1 class decides
    assert tm.classes(pairs[:1], 4, 5, get1, get2) == [(F, N)]


def test_copies_with_different_correction_verdicts_depend_on_the_order():
    T, M2 = "ACGTTGCAAGTC", "GATTACAGATTACA"
    X = T[:6] + ("A" if T[6] != "A" else "C") + T[7:]
    get1, get2 = _getter([T, M2], 4), _getter([T, M2], 5)
    a, b = _read(X, low=[6]), _read(X)  # a: the error is the one low-quality base, corrected; b: the same bases, no low base
    assert cm.classify(a, 4, get1, 90, 1.0, True) and not cm.classify(b, 4, get1, 90, 1.0, True)
    m2 = _read(M2)
    ab = tm.classes([(a, m2), (b, m2)], 4, 5, get1, get2, correction=True)
    ba = tm.classes([(b, m2), (a, m2)], 4, 5, get1, get2, correction=True)
    assert ab == [(H, F), (H, F)]  # the last copy (b) was HALF in pass 1
    assert ba == [(H, F), (F, F)]  # the last copy (a) was FOUND
    out_ab = tm.outputs(*tm.route([(a, m2), (b, m2)], ab))
    out_ba = tm.outputs(*tm.route([(b, m2), (a, m2)], ba))
    assert out_ab["found_1.fastq"] == b"" and out_ab["found_s.fastq"] == cm.fastq_bytes([m2, m2])
    assert out_ba["found_1.fastq"] == cm.fastq_bytes([a]) and out_ba["found_s.fastq"] == cm.fastq_bytes([m2])
    assert out_ab["half_found_s.fastq"] == cm.fastq_bytes([a, b]) and out_ba["half_found_s.fastq"] == cm.fastq_bytes([b])


def test_routing_files_and_statistics_on_a_tiny_case():
    r = [_read(s) for s in ("ACGTA", "CCGTA", "GGGTA", "TTGTA", "ACGTT", "")]
    pairs = [(r[0], r[1]), (r[2], r[3]), (r[4], r[5]), (r[1], r[2])]
    cls = [(F, F), (N, N), (F, H), (H, F)]
    both, single = tm.route(pairs, cls)
    out = tm.outputs(both, single)
    assert out["found_1.fastq"] == cm.fastq_bytes([r[0]]) and out["found_2.fastq"] == cm.fastq_bytes([r[1]])
    assert out["not_found_1.fastq"] == cm.fastq_bytes([r[2]]) and out["not_found_2.fastq"] == cm.fastq_bytes([r[3]])
    assert out["found_s.fastq"] == cm.fastq_bytes([r[4], r[2]])  # first mate first, input order
    assert out["half_found_s.fastq"] == cm.fastq_bytes([r[1]])  # (the empty read is counted, not written)
    assert out["half_found_1.fastq"] == out["half_found_2.fastq"] == out["not_found_s.fastq"] == b""
    assert tm.stats_lines(both, single) == [
        "|\tTotal: 8 reads", "|\tPaired: 4 reads", "|\tTotal quality: 50.00 %",
        "|\tFound: 4 reads", "|\tPercent of found reads: 50.00 %", "|\tQuality of found bin: 50.00 %",
        "|\tNot found: 2 reads", "|\tPercent of not found reads: 25.00 %", "|\tQuality of not found bin: 100.00 %",
        "|\tHalf found: 2 reads", "|\tPercent of half found reads: 25.00 %", "|\tQuality of half found bin: 0.00 %",
    ]
    with pytest.raises(RuntimeError, match="Empty DnaQ!"):
        tm.outputs(*tm.route([(r[0], r[5])], [(F, F)]))


def test_last_copy_model():
    assert tm.last_copy([[0, 1], [1], [0, 1], [], [1], []]) == [2, 4, 2, 5, 4, 5]


@pytest.fixture(scope="module")
def cli():
    from metacherchant_amd import build
    build.build_lib()
    return build.build_host()


def _run(cli, args, wd):
    return subprocess.run([cli, "--tool", "triple-reads-classifier"] + args + ["-w", str(wd)], capture_output=True, text=True, timeout=120)


def test_cli_refuses_k2_not_above_k(cli, tmp_path):
    p = _run(cli, ["-k", "31", "-k2", "31", "-i", "g.fastq", "-r", "a.fastq", "b.fastq"], tmp_path / "wd")
    assert p.returncode == 1 and "k2 should be greater than k, given: 31 31" in p.stderr, p.stderr
    p = _run(cli, ["-k", "41", "-k2", "21", "-i", "g.fastq", "-r", "a.fastq", "b.fastq"], tmp_path / "wd")
    assert p.returncode == 1 and "k2 should be greater than k, given: 41 21" in p.stderr, p.stderr
    assert not os.path.exists(tmp_path / "wd" / "reads_classifier")


def test_cli_refuses_a_single_read_file(cli, tmp_path):
    p = _run(cli, ["-k", "21", "-k2", "31", "-i", "g.fastq", "-r", "a.fastq"], tmp_path / "wd")
    assert p.returncode == 1 and "--read-files needs two files of paired reads" in p.stderr, p.stderr
    p = _run(cli, ["-k", "21", "-k2", "31", "-i", "g.fastq"], tmp_path / "wd")
    assert p.returncode == 1 and "Parameter 'read-files' is mandatory" in p.stderr, p.stderr
    assert not os.path.exists(tmp_path / "wd" / "reads_classifier")


def test_cli_refuses_a_pass_without_a_graph(cli, tmp_path):
    p = _run(cli, ["-k", "21", "-k2", "31", "-ik1", "g.kmers.bin", "-r", "a.fastq", "b.fastq"], tmp_path / "wd")
    assert p.returncode == 1 and "No graph for k = 31" in p.stderr, p.stderr
    p = _run(cli, ["-k", "21", "-k2", "31", "-ik1", "g.fastq", "-ik2", "g2.kmers.bin", "-r", "a.fastq", "b.fastq"], tmp_path / "wd")
    assert p.returncode == 1 and "No graph for k = 21" in p.stderr, p.stderr  # (-ik1 is read only as a .kmers.bin)
    assert not os.path.exists(tmp_path / "wd" / "reads_classifier")


def test_cli_refuses_thresholds_outside_a_percentage(cli, tmp_path):
    p = _run(cli, ["-k", "21", "-k2", "31", "-i", "g.fastq", "-r", "a.fastq", "b.fastq", "-half", "101"], tmp_path / "wd")
    assert p.returncode == 1 and "--half-threshold must be within 0 .. 100" in p.stderr, p.stderr
    p = _run(cli, ["-k", "21", "-k2", "31", "-i", "g.fastq", "-r", "a.fastq", "b.fastq", "-found", "-1"], tmp_path / "wd")
    assert p.returncode == 1 and "--found-threshold must be within 0 .. 100" in p.stderr, p.stderr
    p = _run(cli, ["-k", "21", "-k2", "64", "-i", "g.fastq", "-r", "a.fastq", "b.fastq"], tmp_path / "wd")
    assert p.returncode == 1 and "k = 64 is not supported" in p.stderr, p.stderr
    assert not os.path.exists(tmp_path / "wd" / "reads_classifier")
