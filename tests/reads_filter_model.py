"""A string-level model of the environment-assembler-finder's read filter, written from src/algo/ReadsFilter.java:47-68 and
src/algo/OneSequenceCalculator.java:150-152: a `set` of normalize_dna strings, one substring a window.  The GPU tests hold
mc_reads_in_set and the tool's cutReads<i>.fasta to it."""

_COMPLEMENT = str.maketrans("ACGT", "TGCA")


def reverse_complement(s):
    return s.translate(_COMPLEMENT)[::-1]


def normalize_dna(s):
    """src/utils/StringUtils.java normalizeDna: the smaller of the string and its reverse complement, as strings"""
    rc = reverse_complement(s)
    return s if s <= rc else rc


def read_text(s):
    """DnaQ.toString() of a read as the file spells it: N, n and . are printed as A, other letters in upper case"""
    return "".join("A" if c in "Nn." else c.upper() for c in s)


def make_set(kmers):
    """the subgraph's keys: k-mers in any orientation, duplicates allowed"""
    return {normalize_dna(x) for x in kmers}


def java_div(a, b):
    """Java's int division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def tested_windows(read, k):
    """the windows ReadsFilter tests, normalised: 0 .. L - k - 1 -- the loop is `i < len - k`, so the last window is never tested"""
    return [normalize_dna(read[i:i + k]) for i in range(len(read) - k)]


def threshold(n, k, pct):
    """kmersFiltration of a read of n bases"""
    return max(1, java_div((n - k + 1) * pct, 100))


def hits_and_keep(read, k, members, pct):
    """(hits, keep) of one read (already as read_text gives it).  The reference stops counting when the threshold is reached;
    hits here goes on (no early exit), which decides the same reads."""
    hits = sum(1 for w in tested_windows(read, k) if w in members)
    return hits, len(read) > k and hits >= threshold(len(read), k, pct)


def cut_reads_fasta(reads, k, members, pct, file_index):
    """cutReads<file_index>.fasta for the reads of one file, in order: `>i|n`, n counting the kept reads from 1"""
    out, n = [], 0
    for r in reads:
        text = read_text(r)
        if hits_and_keep(text, k, members, pct)[1]:
            n += 1
            out.append(">%d|%d\n%s\n" % (file_index, n, text))
    return "".join(out)
