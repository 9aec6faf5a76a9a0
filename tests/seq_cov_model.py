"""A small Python restatement of seq-cov's numbers, the yardstick of its tests (test infrastructure only): printSeqBin
(src/tools/SequenceCoverage.java:162-185) and Java's Double.toString as JDK 19 and later document it (the shortest decimal that
reads back as the value -- repr(float)'s digits -- in Java's layout).

A sequence is an array of base codes A0 G1 C2 T3 with N as 0.  `cov_of(codes)` gives getWithZero of every window of one sequence."""
import math

import numpy as np


def java_double_to_string(x):
    """Double.toString: at least one digit after the point, plain notation for 10^-3 <= |x| < 10^7, d.dddE[-]n outside it"""
    x = float(x)
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "-Infinity" if x < 0 else "Infinity"
    sign = "-" if math.copysign(1.0, x) < 0 else ""
    if x == 0:
        return sign + "0.0"
    # repr's shortest digits and decimal exponent: value = 0.d1 d2 ... dn x 10^e10
    mant, _, exp = ("%r" % abs(x)).partition("e")
    ip, _, fp = mant.partition(".")
    digits = (ip + fp).lstrip("0")
    e10 = (int(exp) if exp else 0) + len(ip) - (len(ip + fp) - len((ip + fp).lstrip("0")))
    digits = digits.rstrip("0") or "0"
    if 1e-3 <= abs(x) < 1e7:
        if e10 <= 0:
            return sign + "0." + "0" * (-e10) + digits
        if len(digits) <= e10:
            return sign + digits + "0" * (e10 - len(digits)) + ".0"
        return sign + digits[:e10] + "." + digits[e10:]
    return sign + digits[0] + "." + (digits[1:] or "0") + "E" + str(e10 - 1)


def java_div(a, n):
    """`a * 1. / n` with a long a and an int n: IEEE division, NaN for 0.0 / 0 and a signed zero or infinity for x / 0"""
    a, n = float(a), float(n)
    if n == 0:
        return float("nan") if a == 0 else math.copysign(float("inf"), a)
    return a / n


def seq_bin(cov):
    """printSeqBin's two sums over one sequence's window coverages (Java longs: they do not wrap here)"""
    return sum(int(c) for c in cov), sum(1 for c in cov if c > 0)


def bin_text(depth, breadth, length, k):
    """what printSeqBin prints for one table"""
    n = length - k + 1  # (a Java int; negative for a sequence shorter than k - 1)
    return ", " + java_double_to_string(java_div(depth, n)) + ", " + java_double_to_string(java_div(breadth, n))


HEADER = ("name, from_donor_depth, from_donor_breadth, from_before_depth, from_before_breadth"
          ", from_both_depth, from_both_breadth, itself_depth, itself_breadth")


def csv_row(codes, k, covs):
    """one line of seq_cov.csv: the bases (N as A), then donor, before, both, itself; covs: each table's window coverages"""
    row = bytes(np.frombuffer(b"AGCT", dtype=np.uint8)[np.asarray(codes, dtype=np.uint8)]).decode()
    for cov in covs:
        d, b = seq_bin(cov)
        row += bin_text(d, b, len(codes), k)
    return row


# ---- the windows' keys of a whole store at once (the oracle's mco_key, vectorised: 64-bit arithmetic that wraps)
def window_keys(codes, k, mode):
    """the key of the window starting at every position 0 .. len(codes) - k of one array of codes (int64)"""
    c = np.asarray(codes, dtype=np.uint64)
    n = len(c) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    with np.errstate(over="ignore"):
        if mode == 0:  # Math.min(fw, rc) of the 2k-bit numbers (itmo!/dna/kmers/ShortKmer.java:54-56)
            fw = np.zeros(n, dtype=np.uint64)
            rc = np.zeros(n, dtype=np.uint64)
            for i in range(k):
                fw = (fw << np.uint64(2)) | c[i:i + n]
                rc = (rc << np.uint64(2)) | (np.uint64(3) - c[k - 1 - i:k - 1 - i + n])
        elif mode == 1:  # src/utils/PolynomialHash.java:19-28
            fw = np.ones(n, dtype=np.uint64)
            rc = np.ones(n, dtype=np.uint64)
            for i in range(k):
                fw = fw * np.uint64(5) + c[i:i + n]
                rc = rc * np.uint64(5) + (np.uint64(3) ^ c[k - 1 - i:k - 1 - i + n])
        else:  # src/utils/FNV1AHash.java:33-42
            fw = np.full(n, 14695981039346656037, dtype=np.uint64)
            rc = fw.copy()
            for i in range(k):
                fw = (fw ^ c[i:i + n]) * np.uint64(1099511628211)
                rc = (rc ^ (np.uint64(3) ^ c[k - 1 - i:k - 1 - i + n])) * np.uint64(1099511628211)
    return np.minimum(fw.view(np.int64), rc.view(np.int64))


def store_coverage(codes, offsets, k, mode, table, wk=None):
    """[n_seqs, 2] uint64 (depth, breadth) of every sequence of a store in one oracle table (oracle.pyoracle.Table): the keys of all
    positions at once, looked up in the table's sorted dump, then summed between the sequences' bounds -- a window belongs to a
    sequence when it ends inside it"""
    keys, counts = table.dump()
    wk = window_keys(codes, k, mode) if wk is None else wk  # (a caller with several tables computes them once)
    cov = np.zeros(len(codes) + 1, dtype=np.int64)  # by start position; positions where no window of the store starts stay 0
    if len(wk) and len(keys):
        at = np.minimum(np.searchsorted(keys, wk), len(keys) - 1)
        cov[:len(wk)] = np.where(keys[at] == wk, np.maximum(counts[at].astype(np.int64), 0), 0)
    out = np.zeros((len(offsets) - 1, 2), dtype=np.uint64)
    csum = np.concatenate([[0], np.cumsum(cov)])
    bsum = np.concatenate([[0], np.cumsum(cov > 0)])
    off = np.asarray(offsets).astype(np.int64)
    b, e = off[:-1], off[1:]
    has = e - b >= k  # (a sequence shorter than k has no window)
    out[has, 0] = csum[e[has] - k + 1] - csum[b[has]]
    out[has, 1] = bsum[e[has] - k + 1] - bsum[b[has]]
    return out
