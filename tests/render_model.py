"""A small Python restatement of mc_render_fastq (include/mcgpu.h), the yardstick of its tests (test infrastructure only), written from
the record's definition -- "@<n>\\n<bases>\\n+\\n<quals>\\n", a base "AGCT"[code], a quality phred + 64, <n> counting from the stream's
first number -- and not from the kernel's passes: one walk over the items in item order, a list of bytes per stream.

A read is a pair (codes, phred) as in classifier_model; a side is (reads, stream): the side's reads and one stream byte per read."""
import numpy as np

MAX_STREAMS, SKIP, UNNUMBERED = 16, 0xFF, 2**64 - 1
EMPTY, QUALITY, STREAM = 1, 2, 3


def record(codes, phred, number):
    """one record; number None: the unnumbered form, which starts at the newline behind the number"""
    head = b"\n" if number is None else b"@%d\n" % number
    return head + bytes(b"AGCT"[int(c) & 3] for c in codes) + b"\n+\n" + bytes(int(q) + 64 for q in phred) + b"\n"


def render(sides, n_streams, first_number):
    """(the bytes of every stream, the first error or None).  The error is (kind, side, read, value): the offending item with the lowest
    item index n_sides * read + side, of a read with several bad phreds the first.  A stream byte that names no stream comes before
    any data error, as the call refuses its arguments.  With an error the bytes are None."""
    n_sides, n_reads = len(sides), len(sides[0][0])
    assert all(len(reads) == n_reads and len(stream) == n_reads for reads, stream in sides)
    items = [(i, s) for i in range(n_reads) for s in range(n_sides)]
    for i, s in items:
        b = int(sides[s][1][i])
        if b != SKIP and b >= n_streams:
            return None, (STREAM, s, i, b)
    out, nxt = [[] for _ in range(n_streams)], [int(f) for f in first_number]
    for i, s in items:
        t = int(sides[s][1][i])
        if t == SKIP:
            continue
        codes, phred = sides[s][0][i]
        if len(codes) == 0:
            return None, (EMPTY, s, i, 0)
        high = [int(q) for q in phred if int(q) > 62]
        if high:
            return None, (QUALITY, s, i, high[0])
        if nxt[t] == UNNUMBERED:
            out[t].append(record(codes, phred, None))
        else:
            out[t].append(record(codes, phred, nxt[t]))
            nxt[t] += 1
    return [b"".join(o) for o in out], None


def number_bodies(bodies, first):
    """what the host does with an unnumbered stream once it knows the numbers: "@<n>" in front of every body.  bodies: the stream's
    bytes with the reads' lengths, [(length, bytes)]"""
    return b"".join(b"@%d" % (first + i) + body for i, (_, body) in enumerate(bodies))


def split_bodies(text, lengths):
    """an unnumbered stream cut into its records by the reads' lengths (a record is 2 len + 5 bytes)"""
    out, at = [], 0
    for n in lengths:
        out.append((n, text[at:at + 2 * n + 5]))
        at += 2 * n + 5
    assert at == len(text)
    return out


def pack_side(reads, lead=0):
    """the arrays mc_render_fastq takes for a side's reads: words (with the pad word), phred, offsets.  lead: that many bases (of other
    reads, as in a slice of a larger result) come first, so offsets[0] == lead"""
    filler = (np.arange(lead) * 7 + 3) % 4
    codes = np.concatenate([filler.astype(np.uint8)] + [np.asarray(c, dtype=np.uint8) for c, _ in reads]) if reads or lead else np.zeros(0, np.uint8)
    phred = np.concatenate([np.full(lead, 63, np.uint8)] + [np.asarray(q, dtype=np.uint8) for _, q in reads]) if reads or lead else np.zeros(0, np.uint8)
    n = len(codes)
    words = np.zeros((n + 31) // 32 + 1, dtype=np.uint64)
    g = np.arange(n, dtype=np.uint64)
    np.bitwise_or.at(words, (g // 32).astype(np.int64), (codes.astype(np.uint64) & np.uint64(3)) << (np.uint64(62) - np.uint64(2) * (g % np.uint64(32))))
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    offsets[0] = lead
    if reads:
        offsets[1:] = lead + np.cumsum([len(c) for c, _ in reads])
    return words, phred, offsets


# reads-classifier's eight streams (csrc/host/classifier_streams.h): the four pair files, the heads of the two _s files (the
# "first only" pairs) and their tails (the "second only" pairs, unnumbered: they are numbered behind the heads when the run ends)
FOUND_1, FOUND_2, NOT_FOUND_1, NOT_FOUND_2, FOUND_S, NOT_FOUND_S, FOUND_S_TAIL, NOT_FOUND_S_TAIL = range(8)
CLASSIFIER_FIRST = [1, 1, 1, 1, 1, 1, UNNUMBERED, UNNUMBERED]


def classifier_sides(pairs, found):
    """the two sides of reads-classifier's pairs with the stream of every read; found: read -> bool (PairFinder.run's rule for an
    empty mate applied here)"""
    s1, s2 = [], []
    for a, b in pairs:
        f1 = found(a)
        f2 = (not f1) if len(b[0]) == 0 else found(b)
        if f1 and f2:
            t = (FOUND_1, FOUND_2)
        elif f1:
            t = (FOUND_S if len(a[0]) else SKIP, NOT_FOUND_S if len(b[0]) else SKIP)
        elif f2:
            t = (NOT_FOUND_S_TAIL if len(a[0]) else SKIP, FOUND_S_TAIL if len(b[0]) else SKIP)
        else:
            t = (NOT_FOUND_1, NOT_FOUND_2)
        s1.append(t[0])
        s2.append(t[1])
    return [([a for a, _ in pairs], s1), ([b for _, b in pairs], s2)]


def classifier_files(pairs, found):
    """the six files through render(): the tails numbered behind the heads"""
    sides = classifier_sides(pairs, found)
    text, err = render(sides, 8, CLASSIFIER_FIRST)
    assert err is None, err
    lengths = {t: [len(sides[s][0][i][0]) for i in range(len(pairs)) for s in range(2) if sides[s][1][i] == t] for t in (FOUND_S_TAIL, NOT_FOUND_S_TAIL)}
    heads = {t: sum(1 for s in range(2) for x in sides[s][1] if x == t) for t in (FOUND_S, NOT_FOUND_S)}
    return {
        "found_1.fastq": text[FOUND_1], "found_2.fastq": text[FOUND_2], "not_found_1.fastq": text[NOT_FOUND_1], "not_found_2.fastq": text[NOT_FOUND_2],
        "found_s.fastq": text[FOUND_S] + number_bodies(split_bodies(text[FOUND_S_TAIL], lengths[FOUND_S_TAIL]), heads[FOUND_S] + 1),
        "not_found_s.fastq": text[NOT_FOUND_S] + number_bodies(split_bodies(text[NOT_FOUND_S_TAIL], lengths[NOT_FOUND_S_TAIL]), heads[NOT_FOUND_S] + 1),
    }


# triple-reads-classifier's nine streams: a pair file is 2 * class + side, an _s file 6 + class (the classes as include/mcgpu.h
# numbers them)
NOT_FOUND, HALF_FOUND, FOUND = range(3)


def triple_sides(pairs, classes):
    """the two sides of triple-reads-classifier's pairs with the stream of every read; classes: a (class of the first mate, class of
    the second) per pair.  Written from the reference's lists and files (TripleFinder2.run, TripleReadsClassifier.java:248-267): a pair
    whose mates share a class goes to that class's both_ list, whose first mates make <class>_1 and second mates <class>_2 -- all of
    them for found, those of length > 0 for the other two classes; the mates of any other pair go each to its own class's s_ list,
    which is written without its empty reads."""
    both = {c: [] for c in (NOT_FOUND, HALF_FOUND, FOUND)}
    single = {c: [] for c in (NOT_FOUND, HALF_FOUND, FOUND)}
    for i, (ca, cb) in enumerate(classes):
        if ca == cb:
            both[ca].append(i)
        else:
            single[ca].append((i, 0))
            single[cb].append((i, 1))
    streams = [[SKIP] * len(pairs), [SKIP] * len(pairs)]
    for c in both:
        for side in (0, 1):
            for i in both[c]:
                if c == FOUND or len(pairs[i][side][0]) > 0:
                    streams[side][i] = 2 * c + side
        for i, side in single[c]:
            if len(pairs[i][side][0]) > 0:
                streams[side][i] = 6 + c
    return [([a for a, _ in pairs], streams[0]), ([b for _, b in pairs], streams[1])]
