"""CPU: the seq-cov model (tests/seq_cov_model.py) on cases worked by hand."""
import numpy as np

from tests import seq_cov_model as sm

PINS = [(1.0, "1.0"), (0.5, "0.5"), (0.125, "0.125"), (100.0, "100.0"), (32767.0, "32767.0"), (1 / 3, "0.3333333333333333"),
        (2 / 3, "0.6666666666666666"), (0.001, "0.001"), (1 / 1024, "9.765625E-4"), (1 / 4096, "2.44140625E-4"), (1e-4, "1.0E-4"),
        (9999999.0, "9999999.0"), (1e7, "1.0E7"), (0.0, "0.0"), (-0.0, "-0.0"), (float("nan"), "NaN")]


def test_double_to_string_pins():
    for x, want in PINS:
        assert sm.java_double_to_string(x) == want, (x, want)
    assert sm.java_double_to_string(123456.789) == "123456.789" and sm.java_double_to_string(1.5e10) == "1.5E10"
    assert sm.java_double_to_string(-2.5e-7) == "-2.5E-7" and sm.java_double_to_string(12345678.0) == "1.2345678E7"


def test_a_row_for_every_length_round_k():
    k = 5
    cov_of = lambda codes: [3] * max(len(codes) - k + 1, 0)  # every window found three times
    for L, want in ((k, ", 3.0, 1.0"), (k - 1, ", NaN, NaN"), (k - 2, ", -0.0, -0.0"), (0, ", -0.0, -0.0"), (k + 3, ", 3.0, 1.0")):
        codes = np.zeros(L, dtype=np.uint8)
        d, b = sm.seq_bin(cov_of(codes))
        assert sm.bin_text(d, b, L, k) == want, L
    row = sm.csv_row(np.array([0, 1, 2, 3], dtype=np.uint8), k, [[]] * 4)
    assert row == "AGCT" + ", NaN, NaN" * 4
    assert sm.csv_row(np.zeros(0, dtype=np.uint8), k, [[]] * 4) == ", -0.0, -0.0" * 4
    assert sm.HEADER.count(",") == 8 and sm.HEADER.startswith("name, from_donor_depth")


def test_depth_beyond_an_int_stays_positive():
    d, b = sm.seq_bin([32767] * 70000)  # a saturated repeat: 2 293 690 000 > 2^31
    assert d == 32767 * 70000 > 2**31 and b == 70000
    assert sm.bin_text(d, b, 70000 + 30, 31) == ", 32767.0, 1.0"
    assert sm.bin_text(1, 1, 1024 + 30, 31) == ", 9.765625E-4, 9.765625E-4"


def test_window_keys_match_the_oracle():
    from oracle import pyoracle as po
    rng = np.random.default_rng(7)
    codes = rng.integers(0, 4, 300).astype(np.uint8)
    for k, mode in ((21, 0), (31, 0), (41, 1), (63, 1), (63, 2)):
        wk = sm.window_keys(codes, k, mode)
        assert len(wk) == 300 - k + 1
        assert all(int(wk[i]) == po.key(codes[i:i + k], k, mode) for i in range(0, len(wk), 7))


def test_store_coverage_is_the_sum_of_its_windows():
    from oracle import pyoracle as po
    rng = np.random.default_rng(8)
    genome = rng.integers(0, 4, 2000).astype(np.uint8)
    k = 21
    t = po.Table()
    t.count_reads(np.concatenate([genome, genome[:900]]), np.array([0, 2000, 2900], dtype=np.uint64), k, 0)
    lens = [0, 5, k - 1, k, 100, 0, 700]
    codes = np.concatenate([genome[100:100 + L] for L in lens])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    got = sm.store_coverage(codes, off, k, 0, t)
    for s, L in enumerate(lens):
        seq = codes[int(off[s]):int(off[s + 1])]
        cov = [max(t.get(po.key(seq[i:i + k], k, 0)), 0) for i in range(L - k + 1)]
        assert tuple(int(x) for x in got[s]) == sm.seq_bin(cov), s
    assert int(got[3][0]) == 2 and int(got[6][1]) == 700 - k + 1


def test_the_cpp_double_to_string_equals_the_model(tmp_path):
    """csrc/host/java_replay.cpp java_double_to_string through `mc_hosttest dtoa`: the pins, 100 000 ratios a / n as seq-cov forms them
    (a < 2^40, 1 <= n < 2^31) and 20 000 random bit patterns, in one process call"""
    import struct
    import subprocess

    from metacherchant_amd import build
    build.build_host()
    rng = np.random.default_rng(2020)
    xs = [x for x, _ in PINS]
    a = rng.integers(0, 2**40, 100000)
    n = rng.integers(1, 2**31, 100000)
    a[:20000] = rng.integers(0, 2**20, 20000)   # small counts over small and large n: E- values and short decimals
    n[:10000] = rng.integers(1, 4096, 10000)
    xs += [sm.java_div(int(p), int(q)) for p, q in zip(a, n)]
    xs += [struct.unpack("<d", struct.pack("<Q", int(b)))[0] for b in rng.integers(0, 2**64, 20000, dtype=np.uint64)]
    xs += [5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, float("inf"), float("-inf"), 1e23, 9.999999999999999e22, 1e-3, 9.999e-4, 1e7 - 1e-9]
    path = tmp_path / "doubles.txt"
    path.write_text("".join("%016x\n" % struct.unpack("<Q", struct.pack("<d", x))[0] for x in xs))
    got = subprocess.run([build.HOSTTEST, "dtoa", str(path)], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(got) == len(xs)
    bad = [(x, g, sm.java_double_to_string(x)) for x, g in zip(xs, got) if g != sm.java_double_to_string(x)]
    assert not bad, bad[:5]
    assert got[:len(PINS)] == [w for _, w in PINS]
