"""CPU: the reads-classifier's model (tests/classifier_model.py) pinned on hand-worked cases, the CLI's parameter check, and the
classifier kernel's compiled resources."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import classifier_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(codes, phred=None):
    codes = np.asarray(codes, dtype=np.uint8)
    return codes, np.asarray(phred if phred is not None else [40] * len(codes), dtype=np.uint8)


def _dict_getter(d):
    return lambda w: d.get(bytes(np.asarray(w, dtype=np.uint8)), -1)


def test_a_read_shorter_than_k_is_not_found():
    get = lambda w: 100  # noqa: E731  (every k-mer present)
    assert not cm.find_read(np.zeros(20, dtype=np.uint8), 21, get, 0.0, 1.0)
    assert cm.find_read(np.zeros(21, dtype=np.uint8), 21, get, 0.0, 1.0)
    assert cm.numbers(np.zeros(20, dtype=np.uint8), 21, get) == (0, 0, 0)


def test_width_exactly_at_the_threshold_passes():
    # L = 150, k = 31: 105 covered windows, the last one among them -> breadth (105 + 30) / 150 = 0.9 = 90 / 100 exactly;
    # sum 315 + 30 x 1 -> cov_mean 2.3, theory 1 - e^-2.3 = 0.8997, std sqrt(0.1003 x 0.8997 / 150) = 0.0245
    assert (105 + 30) / 150 == 90 / 100
    assert cm.verdict(315, 105, 1, 150, 31, 90 / 100, 1.0)
    assert not cm.verdict(315, 105, 1, 150, 31, 91 / 100, 1.0)
    # one covered window fewer: 134 / 150 < 0.9
    assert not cm.verdict(315, 104, 1, 150, 31, 90 / 100, 1.96)


def test_width_one_passes_whatever_the_depth():
    # every window covered: (120 + 30) / 150 = 1, found even where the depth is far from what the breadth predicts
    assert cm.verdict(120 * 5000, 120, 5000, 150, 31, 1.0, 1.0)
    assert cm.verdict(120, 120, 1, 150, 31, 1.0, 1.0)


def test_width_zero_fails_even_at_threshold_zero():
    assert not cm.verdict(0, 0, 0, 150, 31, 0.0, 1.0)
    assert not cm.verdict(0, 0, 0, 150, 31, 0.0, 1.96)


def test_the_depth_test_and_z():
    # L = 20, k = 8: 12 of 13 windows at count 2, the last absent -> width 0.6, cov_mean 1.2, theory 0.6988, std 0.1026 (z = 1)
    assert cm.verdict(24, 12, 0, 20, 8, 0.5, 1.0)
    # count 4: cov_mean 2.4, theory 0.9093, |0.6 - 0.9093| = 0.309 > 0.0643 (z = 1) and > 0.126 (z = 1.96)
    assert not cm.verdict(48, 12, 0, 20, 8, 0.5, 1.0)
    assert not cm.verdict(48, 12, 0, 20, 8, 0.5, 1.96)
    # count 3: cov_mean 1.8, theory 0.8347, |diff| 0.2347 > 0.083 (z = 1) but > 0.163 (z = 1.96) too; count 2.5 (sum 30):
    # cov_mean 1.5, theory 0.7769, |diff| 0.1769 > 0.0932 (z = 1), <= 0.1827 (z = 1.96)
    assert not cm.verdict(30, 12, 0, 20, 8, 0.5, 1.0)
    assert cm.verdict(30, 12, 0, 20, 8, 0.5, 1.96)


def test_sums_are_java_ints():
    assert cm.int32(2**31) == -2**31
    assert cm.int32(-1) == -1


def test_correction_uses_the_hard_coded_0_9_under_found_50():
    rng = np.random.default_rng(7)
    codes = rng.integers(0, 4, 20).astype(np.uint8)
    k = 8
    windows = [bytes(codes[i:i + k]) for i in range(13)]
    assert len(set(windows)) == 13
    table = {w: 2 for w in windows[:12]}  # the last window (the only one covering base 19) absent in every variant
    for nuc in range(4):
        v = codes.copy()
        v[19] = nuc
        assert bytes(v[12:20]) not in table
    get = _dict_getter(table)
    phred = [40] * 20
    phred[19] = 5  # one low-quality position: base 19
    read = _read(codes, phred)
    assert cm.bad_pos(read[1]) == 19
    assert cm.numbers(codes, k, get) == (24, 12, 0)
    # plain: width 0.6 passes -found 50 ...
    assert cm.classify(read, k, get, 50, 1.0, False)
    # ... with correction the four variants are held to 0.9 and the original is not tested
    assert not cm.classify(read, k, get, 50, 1.0, True)
    # two low-quality positions: no correction, plain findRead
    phred[3] = 2
    assert cm.bad_pos(phred) == -2
    assert cm.classify(_read(codes, phred), k, get, 50, 1.0, True)


def test_correction_finds_a_read_one_substitution_away():
    rng = np.random.default_rng(11)
    codes = rng.integers(0, 4, 30).astype(np.uint8)
    k = 10
    fixed = codes.copy()
    codes = codes.copy()
    codes[12] = (codes[12] + 1) % 4  # a sequencing error at 12
    table = {bytes(fixed[i:i + k]): 3 for i in range(21)}
    get = _dict_getter(table)
    phred = [40] * 30
    phred[12] = 3
    read = _read(codes, phred)
    assert not cm.classify(read, k, get, 90, 1.96, False)  # windows 3 .. 12 miss
    assert cm.classify(read, k, get, 90, 1.96, True)


def test_n_is_printed_as_a_with_quality_at_sign():
    # N -> base 0, phred 0 (DnaQBuilder.unsafeAppendUnknown); Illumina prints phred + 64
    assert cm.fastq_bytes([_read([0, 1, 2, 3], [0, 20, 40, 62])]) == b"@1\nAGCT\n+\n@Th~\n"
    with pytest.raises(RuntimeError, match="Empty DnaQ"):
        cm.fastq_bytes([_read([], [])])
    with pytest.raises(RuntimeError, match="quality code byte"):
        cm.fastq_bytes([_read([0], [63])])


def test_the_lists_and_the_order_of_the_s_files():
    def r(*codes):
        return _read(codes)
    a1, a2, b1, b2, c1, c2, d1, d2 = r(0), r(1), r(2), r(3), r(0, 0), r(1, 1), r(2, 2), r(3, 3)
    e1, e2 = r(0, 1), r(1, 0)
    found = {id(a1), id(a2), id(b1), id(c2), id(e1)}
    pairs = [(a1, a2), (b1, b2), (c1, c2), (d1, d2), (e1, e2)]
    lists = cm.split(pairs, 1, None, verdicts=lambda x: id(x) in found)
    assert [p[0] is a1 for p in lists["both"]] == [True]
    assert [p[0] for p in lists["first"]] == [b1, e1] and [p[0] for p in lists["second"]] == [c1]
    out = cm.outputs(lists)
    assert out["found_1.fastq"] == cm.fastq_bytes([a1]) and out["found_2.fastq"] == cm.fastq_bytes([a2])
    assert out["not_found_1.fastq"] == cm.fastq_bytes([d1]) and out["not_found_2.fastq"] == cm.fastq_bytes([d2])
    # found_s: the firsts of "first only" (b1, e1), then the seconds of "second only" (c2), numbered 1 .. 3
    assert out["found_s.fastq"] == cm.fastq_bytes([b1, e1, c2])
    assert out["not_found_s.fastq"] == cm.fastq_bytes([b2, e2, c1])
    # single-end: a read is paired with an empty one, found_2 = !found_1, and empty reads leave the _s files
    lists = cm.split(cm.single_end([a1, b2, c1]), 1, None, verdicts=lambda x: x is not b2 and len(x[0]) > 0)
    out = cm.outputs(lists)
    assert out["found_s.fastq"] == cm.fastq_bytes([a1, c1]) and out["not_found_s.fastq"] == cm.fastq_bytes([b2])
    assert out["found_1.fastq"] == out["not_found_1.fastq"] == b""
    assert cm.stats_lines(lists)[:3] == ["|\tTotal: 6 reads", "|\tPaired: 0 reads", "|\tTotal quality: 0.00 %"]


def test_java_percent_format():
    assert cm.java_format_2f(3.125) == "3.13"  # HALF_UP, not half-even
    assert cm.java_format_2f(0.125) == "0.13"
    assert cm.java_format_2f(100.0) == "100.00"
    assert cm.java_format_2f(200 / 3) == "66.67"
    assert cm.java_format_2f(float("nan")) == "NaN"


def test_cli_rejects_reads_classifier_without_read_files(tmp_path):
    from metacherchant_amd import build
    build.build_lib()
    cli = build.build_host()
    p = subprocess.run([cli, "--tool", "reads-classifier", "-k", "31", "-i", str(tmp_path / "graph.fastq"), "-w", str(tmp_path / "wd")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 1, (p.stdout, p.stderr)
    assert "Parameter 'read-files' is mandatory" in p.stderr
    # -o is --output-dir in this tool, and -found / -corr are its short options
    p = subprocess.run([cli, "-t", "reads-classifier", "-k", "31", "-i", "g.fastq", "-o", str(tmp_path / "o"), "-corr", "-found", "101",
                        "-w", str(tmp_path / "wd")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "--found-threshold must be within 0 .. 100" not in p.stderr
    assert "Parameter 'read-files' is mandatory" in p.stderr
    p = subprocess.run([cli, "-t", "reads-classifier", "-k", "31", "-i", "g.fastq", "-r", "x.fastq", "-found", "101", "-w", str(tmp_path / "wd")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "--found-threshold must be within 0 .. 100" in p.stderr
    assert not os.path.exists(tmp_path / "wd" / "reads_classifier")


def test_the_classifier_kernel_uses_no_scratch_and_no_vgpr_spills(tmp_path):
    from metacherchant_amd import build
    lib = build.build_lib()
    llvm = "/opt/rocm/lib/llvm/bin"
    if not all(os.path.exists(os.path.join(llvm, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("ROCm's llvm tools are not here")
    found = {}
    for co in build.code_objects(lib, str(tmp_path)):
        text = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], text=True)
        for block in text.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            if "k_classify" in name:
                found[name] = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_count|vgpr_spill_count):\s+(\d+)", block)}
    assert len(found) == 3, sorted(found)  # one a key mode
    for name, r in found.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] <= 128, (name, r)  # (at least 4 waves a SIMD to keep probes in flight)
