"""A small Python restatement of the reads-classifier, the yardstick of its tests (test infrastructure only):
findRead / findReadWithCorrection (src/algo/ReadsFinderInGraph.java:37-161), PairFinder.run (src/algo/PairFinder.java:32-57),
the lists and statistics of ReadsClassifier.runImpl (src/tools/ReadsClassifier.java:154-260) and the FASTQ writer
(itmo!/io/writers/FastqDedicatedWriter.java:39-60, Illumina.getPhredChar).

A read is a pair (codes, phred): base codes A0 G1 C2 T3 with N as 0, phreds 0..63 as DnaQ.phredAt returns them.
`get(codes_of_one_window)` is the table: the saturated count, or -1 when the k-mer's key is absent."""
import math
from decimal import ROUND_HALF_UP, Decimal

import numpy as np


def int32(x):
    return (int(x) + 2**31) % 2**32 - 2**31


def verdict(sum_, covered, last, length, k, thr, z):
    """findRead's test on the three numbers (ints as in Java, the rest in double)"""
    cov_mean = int32(sum_ + last * (k - 1)) / length
    width = int32(covered + (k - 1 if last > 0 else 0)) / length
    theory = 1.0 - math.exp(-cov_mean)
    std = z * math.sqrt(math.exp(-cov_mean) * (1 - math.exp(-cov_mean)) / length)
    return not (width < thr) and (width == 1 or (width != 0 and -std <= width - theory and width - theory <= std))


def coverage(codes, k, get):
    """getCoverage: getWithZero of every window"""
    return [max(int(get(codes[i:i + k])), 0) for i in range(len(codes) - k + 1)]


def numbers(codes, k, get):
    """(sum, covered, last) of a read of length >= k; zeros for a shorter one"""
    if len(codes) < k:
        return 0, 0, 0
    cov = coverage(codes, k, get)
    return int32(sum(cov)), sum(1 for c in cov if c > 0), cov[-1]


def find_read(codes, k, get, thr, z):
    if len(codes) < k:
        return False
    s, c, last = numbers(codes, k, get)
    return verdict(s, c, last, len(codes), k, thr, z)


def bad_pos(phred):
    """the only position with phred < 10, -1 for none, -2 for several (what the host hands the kernel)"""
    low = [i for i, q in enumerate(phred) if q < 10]
    return -1 if not low else (low[0] if len(low) == 1 else -2)


def find_read_with_correction(codes, phred, k, get, thr, z):
    if len(codes) < k:
        return False
    p = bad_pos(phred)
    if p < 0:
        return find_read(codes, k, get, thr, z)
    for nuc in range(4):
        c = np.array(codes, dtype=np.uint8).copy()
        c[p] = nuc
        if find_read(c, k, get, 0.9, z):  # (the reference's constant, whatever -found says)
            return True
    return False


def classify(read, k, get, found_pct, z, correction):
    codes, phred = read
    thr = found_pct / 100
    return find_read_with_correction(codes, phred, k, get, thr, z) if correction else find_read(codes, k, get, thr, z)


EMPTY = (np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8))


def split(pairs, k, get, found_pct=90, z=1.0, correction=False, verdicts=None):
    """PairFinder.run over the pairs in input order: the four lists (both, first only, second only, neither).
    verdicts (optional): a function read -> found, instead of classify (e.g. what the device said)."""
    lists = {"both": [], "first": [], "second": [], "neither": []}
    f = verdicts or (lambda r: classify(r, k, get, found_pct, z, correction))
    for a, b in pairs:
        f1, f2 = f(a), f(b)
        if len(b[0]) == 0:
            f2 = not f1
        key = "both" if f1 and f2 else "first" if f1 else "second" if f2 else "neither"
        lists[key].append((a, b))
    return lists


def single_end(reads):
    return [(r, EMPTY) for r in reads]


def fastq_bytes(reads):
    """writeDnaQsToFastqFile; raises RuntimeError as the reference does"""
    out = []
    for n, (codes, phred) in enumerate(reads, 1):
        if len(codes) == 0:
            raise RuntimeError("Empty DnaQ!")
        if any(int(q) > 62 for q in phred):
            raise RuntimeError("Invalid quality code byte")
        out.append("@%d\n%s\n+\n%s\n" % (n, "".join("AGCT"[int(c)] for c in codes), "".join(chr(int(q) + 64) for q in phred)))
    return "".join(out).encode()


def outputs(lists):
    """the six files' bytes"""
    nonempty = lambda rs: [r for r in rs if len(r[0]) > 0]  # noqa: E731
    return {
        "found_1.fastq": fastq_bytes([a for a, _ in lists["both"]]),
        "found_2.fastq": fastq_bytes([b for _, b in lists["both"]]),
        "not_found_1.fastq": fastq_bytes([a for a, _ in lists["neither"]]),
        "not_found_2.fastq": fastq_bytes([b for _, b in lists["neither"]]),
        "found_s.fastq": fastq_bytes(nonempty([a for a, _ in lists["first"]]) + nonempty([b for _, b in lists["second"]])),
        "not_found_s.fastq": fastq_bytes(nonempty([b for _, b in lists["first"]]) + nonempty([a for a, _ in lists["second"]])),
    }


def java_format_2f(x):
    """String.format("%.2f", x): HALF_UP on the shortest decimal that reads back as x"""
    if x != x:
        return "NaN"
    if math.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"
    return str(Decimal(repr(x)).quantize(Decimal("0.01"), rounding=ROUND_HALF_UP))


def stats_lines(lists):
    bf, ff, sf, nf = (len(lists[n]) for n in ("both", "first", "second", "neither"))
    total, found, not_found, paired = 2 * (bf + ff + sf + nf), 2 * bf + ff + sf, 2 * nf + ff + sf, 2 * (bf + nf)
    div = lambda a, b: a / b if b else (math.nan if a == 0 else math.inf)  # noqa: E731  (Java's double division)
    return [
        "|\tTotal: %d reads" % total,
        "|\tPaired: %d reads" % paired,
        "|\tTotal quality: %s %%" % java_format_2f(div(100 * paired, total)),
        "|\tFound: %d reads" % found,
        "|\tPercent of found reads: %s %%" % java_format_2f(div(100 * found, total)),
        "|\tQuality of found bin: %s %%" % java_format_2f(div(bf * 2, bf * 2 + ff + sf) * 100),
        "|\tNot found: %d reads" % not_found,
        "|\tPercent of not found reads: %s %%" % java_format_2f(div(100 * not_found, total)),
        "|\tQuality of not found bin: %s %%" % java_format_2f(div(nf * 2, nf * 2 + ff + sf) * 100),
    ]


def table_getter(table, k, mode):
    """get() over an oracle table (oracle/pyoracle.py), cached by window"""
    from oracle import pyoracle as po
    cache = {}

    def get(window):
        b = bytes(np.asarray(window, dtype=np.uint8))
        if b not in cache:
            cache[b] = table.get(po.key(np.frombuffer(b, dtype=np.uint8), k, mode))
        return cache[b]
    return get
