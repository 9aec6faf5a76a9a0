"""A small sequential Python restatement of the triple-reads-classifier, the yardstick of its tests (test infrastructure only):
TripleFinder.run (src/algo/TripleFinder.java:32-67), TripleFinder2.run (src/algo/TripleFinder2.java:45-110), the six queues and the
FoundStats of TripleReadsClassifier.runImpl (src/tools/TripleReadsClassifier.java:164-333) and its nine files.

Reads are (codes, phred) pairs as in tests/classifier_model.py, whose verdicts, numbers, writer and number format are reused.  The
reference's maps are dicts keyed by bytes(codes) -- the bases with N as A, no qualities -- filled in input order, so the last
writer wins: the sequential meaning of the reference's thread pool (-p 1)."""
import math

from tests import classifier_model as cm

NOT_FOUND, HALF_FOUND, FOUND = 0, 1, 2


def width(codes, k, get):
    """getWidth: (covered + [last > 0] (k - 1)) / len of the read as given, 0 when len < k"""
    if len(codes) < k:
        return 0.0
    _, covered, last = cm.numbers(codes, k, get)
    return cm.int32(covered + (k - 1 if last > 0 else 0)) / len(codes)


def class_pass1(found, w, half):
    return FOUND if found else HALF_FOUND if w >= half else NOT_FOUND


def class_pass2(f, c1, w, half):
    if f and c1 == FOUND:
        return FOUND
    if f or c1 == FOUND or (w >= half and c1 == HALF_FOUND):
        return HALF_FOUND
    return NOT_FOUND


def _verdicts(pair, k, get, found_pct, z, correction):
    a, b = pair
    f1 = cm.classify(a, k, get, found_pct, z, correction)
    f2 = cm.classify(b, k, get, found_pct, z, correction)
    if len(b[0]) == 0:
        f2 = not f1
    return f1, f2


def classes(pairs, k, k2, get1, get2, found_pct=90, half_pct=40, z=1.0, correction=False):
    """the final (class of mate 1, class of mate 2) of every pair, in input order"""
    half = half_pct / 100
    maps = ({}, {})
    for pair in pairs:  # pass 1 at k: TripleFinder
        fs = _verdicts(pair, k, get1, found_pct, z, correction)
        for s in (0, 1):
            codes = pair[s][0]
            maps[s][bytes(bytearray(int(c) for c in codes))] = class_pass1(fs[s], width(codes, k, get1), half)
    out = []
    for pair in pairs:  # pass 2 at k2: TripleFinder2
        fs = _verdicts(pair, k2, get2, found_pct, z, correction)
        res = []
        for s in (0, 1):
            codes = pair[s][0]
            c1 = maps[s][bytes(bytearray(int(c) for c in codes))]
            res.append(class_pass2(fs[s], c1, width(codes, k2, get2), half))
        out.append(tuple(res))
    return out


def route(pairs, cls):
    """the six queues: both_found, both_half_found, both_not_found (pairs) and s_found, s_half_found, s_not_found (reads, first mate
    first), each in input order"""
    both = {FOUND: [], HALF_FOUND: [], NOT_FOUND: []}
    single = {FOUND: [], HALF_FOUND: [], NOT_FOUND: []}
    for (a, b), (c1, c2) in zip(pairs, cls):
        if c1 == c2:
            both[c1].append((a, b))
        else:
            single[c1].append(a)
            single[c2].append(b)
    return both, single


def outputs(both, single):
    """the nine files' bytes; raises RuntimeError("Empty DnaQ!") when found_1 / found_2 would hold an empty read"""
    nonempty = lambda rs: [r for r in rs if len(r[0]) > 0]  # noqa: E731
    out = {
        "found_1.fastq": cm.fastq_bytes([a for a, _ in both[FOUND]]),
        "found_2.fastq": cm.fastq_bytes([b for _, b in both[FOUND]]),
    }
    for name, c in (("half_found", HALF_FOUND), ("not_found", NOT_FOUND)):
        out[name + "_1.fastq"] = cm.fastq_bytes(nonempty([a for a, _ in both[c]]))
        out[name + "_2.fastq"] = cm.fastq_bytes(nonempty([b for _, b in both[c]]))
    for name, c in (("found", FOUND), ("half_found", HALF_FOUND), ("not_found", NOT_FOUND)):
        out[name + "_s.fastq"] = cm.fastq_bytes(nonempty(single[c]))
    return out


def stats_lines(both, single):
    """FoundStats and its twelve log lines"""
    bf, bh, bn = len(both[FOUND]), len(both[HALF_FOUND]), len(both[NOT_FOUND])
    sf, sh, sn = len(single[FOUND]), len(single[HALF_FOUND]), len(single[NOT_FOUND])
    total, paired = 2 * (bn + bf + bh) + sf + sn + sh, 2 * (bf + bn + bh)
    found, not_found, half_found = 2 * bf + sf, 2 * bn + sn, 2 * bh + sh
    div = lambda a, b: a / b if b else (math.nan if a == 0 else math.inf)  # noqa: E731  (Java's double division)
    f = cm.java_format_2f
    return [
        "|\tTotal: %d reads" % total,
        "|\tPaired: %d reads" % paired,
        "|\tTotal quality: %s %%" % f(div(100 * paired, total)),
        "|\tFound: %d reads" % found,
        "|\tPercent of found reads: %s %%" % f(div(100 * found, total)),
        "|\tQuality of found bin: %s %%" % f(div(bf * 2, found) * 100),
        "|\tNot found: %d reads" % not_found,
        "|\tPercent of not found reads: %s %%" % f(div(100 * not_found, total)),
        "|\tQuality of not found bin: %s %%" % f(div(bn * 2, not_found) * 100),
        "|\tHalf found: %d reads" % half_found,
        "|\tPercent of half found reads: %s %%" % f(div(100 * half_found, total)),
        "|\tQuality of half found bin: %s %%" % f(div(bh * 2, half_found) * 100),
    ]


def last_copy(reads_codes):
    """for every read, the greatest index of a read with the same bases (what mc_reads_last_copy computes)"""
    last = {}
    for i, c in enumerate(reads_codes):
        last[bytes(bytearray(int(x) for x in c))] = i
    return [last[bytes(bytearray(int(x) for x in c))] for c in reads_codes]
