"""Designed texts for the counting tokeniser (csrc/tokenizer.h, driven by csrc/reads_file.hip mc_add_reads_file): newlines at tile
edges, line lengths around the 64-lane stretch, output offsets at every residue of the 32-base word, FASTQ pieces that start at
lane 0 with and without a good base carried in, records longer than the WavePacker holds, more lines than one round of k_scan_one
scans -- and the chunk sizes that cut them.  The reads come from oracle/host_oracle.py (read_fasta_reads / read_fastq_reads: the
reference); cuts() restates the drivers' cut rule and plain_record_start (csrc/host/reads_io.cpp plain_chunks) and says what every chunk holds.
tests/test_tokenizer_cases_model.py checks that the texts hold what they are for; tests/test_gpu_tokenizer_edges.py holds the
kernels to them."""
import collections
import functools
import os
import tempfile

import numpy as np

from oracle import host_oracle as ho

T_BYTES = 32        # csrc/device_types.h:110  bytes per thread of the newline passes
T_TILE = 8192       # csrc/device_types.h:111  T_THREADS * T_BYTES: bytes per workgroup of the newline passes
SCAN_TILE = 4096    # csrc/tokenizer_device.h:10  elements per workgroup of the generic scan
SCAN_ROUND = 1024   # csrc/tokenizer.h:35-41  k_scan_one takes the tile sums 1024 at a time and carries between rounds
LANES = 64          # csrc/tokenizer.h:129, 206, 240, 273  a wave takes a line / record in stretches of 64 bytes
WORD = 32           # csrc/tokenizer_device.h:121  bases per packed 64-bit word
WP_WORDS = 65       # csrc/tokenizer_device.h:89  LDS words of a WavePacker
FLUSH = WP_WORDS * WORD  # csrc/tokenizer_device.h:118  put() flushes when the next stretch would pass 2080 bases
DEFAULT_CHUNK = 1 << 28  # csrc/switches.h:30  MC_TOKENIZER_CHUNK_BYTES (64 B .. 1.5 GB)
MIN_CHUNK = 64           # csrc/switches.h  tokenizer_chunk_bytes_of

LARGE = "fa_scan_rounds"
SEED = 20241020

Cut = collections.namedtuple("Cut", "b e probe lines reads bases")  # probe: the position plain_record_start was asked about (None: the last cut)


# ------------------------------------------------------------------------------------------------------------------ the models

def _with_file(text, fastq, fn):
    fd, path = tempfile.mkstemp(suffix=".fq" if fastq else ".fa")
    try:
        with os.fdopen(fd, "wb") as f:
            f.write(text)
        return fn(path)
    finally:
        os.unlink(path)


def expected_reads(text, fastq):
    """the reads of a file with these bytes, in file order: what the reference's readers give (oracle/host_oracle.py)"""
    return _with_file(text, fastq, ho.read_fastq_reads if fastq else ho.read_fasta_reads)


def lines_of(text):
    """the lines as the kernels see them (wave_line_spans): split at '\\n', none behind a last '\\n', one trailing '\\r' off"""
    if not text:
        return []
    parts = text.split(b"\n")
    if text.endswith(b"\n"):
        parts.pop()
    return [p[:-1] if p.endswith(b"\r") else p for p in parts]


def count_lines(chunk):
    """tokenize_chunk_locked (csrc/reads_file.hip): the newlines, plus one if the chunk does not end in one"""
    return chunk.count(b"\n") + (0 if chunk.endswith(b"\n") else 1)


def sniff_offset(text):
    """ReadersUtils.determineQualityFormat as the readers do it: 64 unless one of the first 1000 records has, under a base that is
    not N n ., a quality char below 64 or above 126"""
    lines = lines_of(text)
    for r in range(min(len(lines) // 4, 1000)):
        d, q = lines[4 * r + 1], lines[4 * r + 3]
        if any(c not in b"Nn." and (x < 64 or x > 126) for c, x in zip(d, q)):
            return 33
    return 64


def fq_good(bases, qual, offset):
    """per base: does it stay (csrc/tokenizer.h fq_bad_base; FastaReaderFromXQSourceTrunc.java:61-95, DnaQBuilder.java:32-35)"""
    d = np.frombuffer(bases, dtype=np.uint8)
    q = np.frombuffer(qual, dtype=np.uint8).astype(np.int64)
    unknown = (d == ord("N")) | (d == ord("n")) | (d == ord("."))
    return ~unknown & (((q - offset) & 63) >= 1)


def pieces_of(good):
    """(start, length) of every run of good bases"""
    g = np.concatenate([[False], np.asarray(good, dtype=bool), [False]])
    edges = np.flatnonzero(g[1:] != g[:-1])
    return [(int(s), int(e - s)) for s, e in zip(edges[0::2], edges[1::2])]


def fq_records(text):
    """(bases, qualities) of every four-line record"""
    lines = lines_of(text)
    return [(lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def record_start(text, fastq, q):
    """plain_record_start (csrc/host/reads_io.cpp): the first record start at or behind the line that byte q - 1 ends or lies in"""
    end = len(text)

    def next_line(s):
        nl = text.find(b"\n", s)
        return nl + 1 if nl >= 0 else end

    def len_of(s):
        nl = text.find(b"\n", s)
        e = nl if nl >= 0 else end
        return e - s - (1 if e > s and text[e - 1] == 13 else 0)

    line = 0
    if q > 0:
        nl = text.find(b"\n", q - 1)
        line = nl + 1 if nl >= 0 else end
    while line < end:
        c = text[line]
        if not fastq:
            if c in b">;":
                return line
        elif c == ord("@"):
            # an '@' line whose third line starts with '+' and whose second and fourth lines are equally long
            l2 = next_line(line)
            l3 = next_line(l2) if l2 < end else end
            if l3 < end and text[l3] == ord("+"):
                l4 = next_line(l3)
                if l4 < end and len_of(l2) == len_of(l4):
                    return line
        line = next_line(line)
    return end


def cut_positions(text, fastq, chunk):
    """plain_chunks (csrc/host/reads_io.cpp) with the chunk size as MC_TOKENIZER_CHUNK_BYTES gives it (csrc/switches.h tokenizer_chunk_bytes_of;
    None: unset): (b, e, probe)"""
    chunk = DEFAULT_CHUNK if chunk is None else min(max(int(chunk), MIN_CHUNK), 3 << 29)
    out, b, end = [], 0, len(text)
    while b < end:
        if end - b <= chunk + chunk // 4:
            out.append((b, end, None))
            b = end
        else:
            e = record_start(text, fastq, b + chunk)
            out.append((b, e, b + chunk))
            b = e
    return out


def cuts(text, fastq, chunk, whole_reads=None):
    """The chunks a run with MC_TOKENIZER_CHUNK_BYTES=chunk (None: the default) tokenises, each with the lines, reads and bases the
    device has to find in it.  whole_reads: the file's reads where they are known (used when the file is one chunk)."""
    pos = cut_positions(text, fastq, chunk)
    if len(pos) == 1 and whole_reads is not None:
        return [Cut(0, len(text), None, count_lines(text), len(whole_reads), sum(len(r) for r in whole_reads))]
    out = []
    offset = sniff_offset(text) if fastq else 0
    for b, e, probe in pos:
        part = text[b:e]
        if fastq:  # (the offset is the file's, so a chunk is not read as a file of its own)
            reads = bases = 0
            for d, q in fq_records(part):
                for _, n in pieces_of(fq_good(d, q, offset)):
                    reads += 1
                    bases += n
        else:
            rs = expected_reads(part, False)
            reads, bases = len(rs), sum(len(r) for r in rs)
        out.append(Cut(b, e, probe, count_lines(part), reads, bases))
    return out


def dst_bases(cs):
    """where each chunk's first base goes behind the chunks before it (reserve_words: dst_base = pend->bases)"""
    out, at = [], 0
    for c in cs:
        out.append(at)
        at += c.bases
    return out


def device_declines(text, fastq):
    """Would a kernel raise a flag on this text (TOK_BAD_CHAR, TOK_BAD_STRUCTURE, TOK_BAD_QUALITY), or the driver decline it for its
    line count?  By byte classes and the four-line shape, not by running anything."""
    arr = np.frombuffer(text, dtype=np.uint8)
    if not fastq:
        ok = np.zeros(256, dtype=bool)
        ok[list(b"ACGTacgtNn\n")] = True
        bad = ~ok[arr]
        if not bad.any():
            return False
        # only header lines may hold anything else, and a '\r' may stand in front of a '\n' (or of the end of the text)
        starts = np.concatenate([[0], np.flatnonzero(arr == 10) + 1])
        line_of = np.searchsorted(starts, np.flatnonzero(bad), side="right") - 1
        first = arr[np.minimum(starts[line_of], len(arr) - 1)]
        in_header = (first == ord(">")) | (first == ord(";"))
        at = np.flatnonzero(bad)
        nxt = np.where(at + 1 < len(arr), arr[np.minimum(at + 1, len(arr) - 1)], 10)
        cr = (arr[at] == 13) & (nxt == 10)
        return bool((~in_header & ~cr).any())
    lines = lines_of(text)
    if len(lines) % 4:
        return True
    offset = sniff_offset(text)
    for i in range(0, len(lines), 4):
        ident, d, plus, q = lines[i:i + 4]
        if ident[:1] != b"@" or plus[:1] != b"+" or len(d) != len(q):
            return True
        for c, x in zip(d, q):
            if c in b"Nn.":
                continue
            if c not in b"ACGTacgt" or x < offset or x > 126:
                return True
    return False


# ------------------------------------------------------------------------------------------------------------------- the texts

def _bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))


def _put(s, at, c):
    return s[:at] + c + s[at + len(c):]


def _fold(b, width):
    return [b[i:i + width] for i in range(0, len(b), width)]


def _fasta(records):
    """records: (header line or None, list of lines)"""
    lines = []
    for h, body in records:
        if h is not None:
            lines.append(h)
        lines += body
    return b"\n".join(lines) + b"\n"


def _fastq(records):
    """records: (bases, qualities); every other '+' line repeats the id"""
    lines = []
    for i, (b, q) in enumerate(records):
        ident = b"r%d/1" % i
        lines += [b"@" + ident, b, b"+" + (ident if i % 2 else b""), q]
    return b"\n".join(lines) + b"\n"


def _chunks(text):
    """64 (the switch's minimum), 100, 4096, and the smallest chunk for which the whole file is still `chunk + chunk / 4`: a little
    above 4/5 of its size"""
    c = len(text) * 4 // 5
    while c + c // 4 < len(text):
        c += 1
    return [64, 100, 4096, c]


TILE_NEWLINES = (31, 32, 8190, 8191, 8192, 8193, 16383, 16384)
LONG_LINE = 17000


def _tile_edges(rng):
    """'\\n' at every offset of TILE_NEWLINES (the neighbours make empty lines), then short records up to a little before a tile's end
    and one line that runs through the two whole tiles behind it"""
    t = _bases(rng, 31) + b"\n\n"                                  # 31, 32: bases in front of the first header, an empty line
    t += b">h1\n"
    t += _bases(rng, 8190 - len(t)) + b"\n\n\n\n"                  # 8190 .. 8193
    t += b">h2 x\n"
    t += _bases(rng, 16383 - len(t)) + b"\n\n"                     # 16383, 16384
    i = 0
    while len(t) < 3 * T_TILE - 300:
        t += b">s%d\n" % i + _bases(rng, 7 + 11 * (i % 9)) + b"\n"
        i += 1
    t += b">long\n" + _bases(rng, LONG_LINE) + b"\n>tail\n" + _bases(rng, 50) + b"\n"
    return t


def _exact_size(rng, size, last_eol, crlf_at=None):
    """A FASTA text of exactly `size` bytes: lines of 60 (a header every ninth), after a short header, a line of 14 bases and another
    header.  crlf_at: lines end in "\\r\\n", the '\\n's 62 apart and one of them at this offset."""
    arr = np.frombuffer(_bases(rng, size), dtype=np.uint8).copy()
    if crlf_at is None:
        nls = [10, 25, 36] + list(range(97, size - 3, 61))
    else:
        nls = [14, 30, 42] + [p for p in range(crlf_at % 62, size - 3, 62) if p >= 62]
    starts = [0] + [p + 1 for p in nls]
    for j, s in enumerate(starts):
        if j % 9 == 0 or j == 2:
            arr[s] = ord(">")
    for p in nls:
        arr[p] = 10
        if crlf_at is not None:
            arr[p - 1] = 13
    if last_eol:
        arr[-1] = 10
        if crlf_at is not None:
            arr[-2] = 13
    return arr.tobytes()


LENGTHS = list(range(1, 131)) + [2015, 2016, 2017, 2047, 2048, 2049, 2079, 2080, 2081, 2111, 2112, 2113, 4159, 4160, 4161, 6241]


def _lengths_order():
    """32 and 64 first (they start at bases 0 and 32: whole words only), then 1 .. 130 in order (the reads' first bases are 96 plus the
    triangular numbers, which take every residue mod 32), the long ones, and 32 and 64 once more behind a read that ends a word"""
    order = [32, 64] + LENGTHS
    order.append(-sum(order) % WORD or WORD)
    return order + [32, 64]


def _lengths(rng):
    return _fasta([(b">len %d" % n, [_bases(rng, n)]) for n in _lengths_order()])


WIDTHS = (1, 31, 32, 33, 64, 70)
ODD_HEADER = b">N has >N> nn 0123456789 RYKMSWBDHV *#@+;. \tx"


def _shapes(rng):
    recs = [(None, _fold(_bases(rng, 45), 9))]                                                  # bases before the first header
    for w in WIDTHS:
        tag = b" w%d" % w
        recs.append((b">plain" + tag, _fold(_bases(rng, 150), w)))
        recs.append((b">N first line" + tag, _fold(_put(_bases(rng, 150), min(w - 1, 5), b"N"), w)))
        recs.append((b">after a dropped one" + tag, _fold(_bases(rng, 37), w)))                 # kept, dropped, kept: the kept two
        recs.append((b">N last line" + tag, _fold(_put(_bases(rng, 150), 149, b"N"), w)))       # share a border word
        recs.append((b">and kept again" + tag, _fold(_bases(rng, 45), w)))
        recs.append((b">N alone" + tag, _fold(_bases(rng, 100), w) + [b"N"] + _fold(_bases(rng, 40), w)))
        recs.append((b">lower n" + tag, _fold(_put(_bases(rng, 150), 77, b"n"), w)))
        recs.append((b">only empty lines" + tag, [b"", b"", b""]))
        recs.append((b";semicolon" + tag, _fold(_bases(rng, 70), w)))
        recs.append((b">", _fold(_bases(rng, 33), w)))
        recs.append((ODD_HEADER + tag, _fold(_bases(rng, 29), w) + [b""] + _fold(_bases(rng, 64), w)))  # an empty line inside
        recs.append((b">lower" + tag, _fold(_bases(rng, 90).lower(), w)))
        mixed = bytes(c | 0x20 if i % 3 == 0 else c for i, c in enumerate(_bases(rng, 95)))
        recs.append((b">Mixed" + tag, _fold(mixed, w)))
        recs.append((b">short" + tag, [_bases(rng, 7)]))
    recs.append((b">a header at the very end", []))
    return _fasta(recs)


def _probe_in_header(rng):
    """chunk 64: the first probe, byte 64, lies in a header whose byte 64 is '>' itself"""
    recs = [(b">a", [_bases(rng, 50)]), (b">second N>>>>>>>> header with > signs", [_bases(rng, 40), _bases(rng, 12)])]
    recs += [(b">r%d > x" % i, _fold(_bases(rng, 10 + 7 * i), 31)) for i in range(12)]
    return _fasta(recs)


def _good_quals(rng, n, offset):
    return bytes((rng.randint(2, 41, size=n) + offset).astype(np.uint8))


PIECE_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 200)
BAD_POSITIONS = (0, -1, 62, 63, 64, 65, 127, 128)  # -1: the last base


def _bad_kinds(offset):
    kinds = [(b"N", None), (b"n", None), (b".", None), (None, 0)]
    return kinds + [(None, 64)] if offset == 33 else kinds  # (phred 64 wraps to 0; at offset 64 its char would be past '~')


def _spoil(b, q, at, kind, offset):
    base, phred = kind
    if base is not None:
        b = _put(b, at, base)
    if phred is not None:
        q = _put(q, at, bytes([offset + phred]))
    return b, q


def _pieces(rng, offset):
    kinds = _bad_kinds(offset)
    recs, n = [], 0

    def rq(length):
        return _bases(rng, length), _good_quals(rng, length, offset)

    def spoiled(length, positions):
        nonlocal n
        b, q = rq(length)
        for at in positions:
            b, q = _spoil(b, q, at, kinds[n % len(kinds)], offset)
            n += 1
        return b, q

    for length in PIECE_LENGTHS:
        recs.append(rq(length))
        where = sorted({length - 1 if p < 0 else p for p in BAD_POSITIONS if (length - 1 if p < 0 else p) in range(length)})
        for at in where:
            for kind in (kinds if length in (129, 200) else [kinds[n % len(kinds)]]):
                recs.append(_spoil(*rq(length), at, kind, offset))
                n += 1
    recs.append(spoiled(200, range(60, 67)))               # runs of bad bases: over the stretch's edge, at the ends
    recs.append(spoiled(200, [0, 1, 2, 197, 198, 199]))
    recs.append(spoiled(129, [126, 127, 128]))
    recs.append((b"N" * 65, rq(65)[1]))                    # all bad
    recs.append((rq(64)[0], bytes([offset]) * 64))
    recs.append(spoiled(130, range(130)))
    recs.append(spoiled(129, [62, 64]))                    # a piece of one base at 63
    recs.append(spoiled(129, [63, 65]))                    # ... and at 64: it starts at lane 0, nothing carried in
    recs.append(spoiled(129, [62, 64, 66]))
    recs.append(spoiled(200, [126, 128, 130]))             # (the same at the next edge)
    recs.append(spoiled(129, [62, 65]))                    # good at 63 and at 64: one piece over the edge (carry = 1)
    recs.append(spoiled(200, [0, 199]))
    recs.append(spoiled(129, [63]))                        # bad at 63, good at 64: a piece starts at lane 0 (carry = 0)
    recs.append(spoiled(200, [63, 127]))
    for length in (40, 64, 129):                           # quality char '~', and a quality line that starts with '@'
        b, q = rq(length)
        recs.append((b, _put(_put(q, length // 2, b"~"), length - 1, b"~")))
        b, q = rq(length)
        recs.append((b, _put(q, 0, b"@")))
    return _fastq(recs)


def _probe_in_quality(rng):
    """chunk 64: the first probe, byte 64, lies in a quality line that begins with '@'.  chunk 100: the first probe is the '+' of
    the record behind it, so the first line plain_record_start looks at is a quality line that begins with '@'."""
    recs = [(_bases(rng, 38), b"@" + _good_quals(rng, 37, 33)), (_bases(rng, 5), b"@" + _good_quals(rng, 4, 33))]
    recs += [(_bases(rng, n), _put(_good_quals(rng, n, 33), 0, b"@" if n % 2 else b"I")) for n in (33, 20, 64, 9, 70, 31, 30, 45, 12, 90)]
    return _fastq(recs)


def _long_record(rng, offset):
    kinds = _bad_kinds(offset)
    b, q = _bases(rng, 5000), _good_quals(rng, 5000, offset)
    for i, at in enumerate(range(96, 5000, 97)):
        b, q = _spoil(b, q, at, kinds[i % len(kinds)], offset)
    recs = [(_bases(rng, 5), _good_quals(rng, 5, offset)), (b, q), (_bases(rng, 2200), _good_quals(rng, 2200, offset)),
            (_bases(rng, 21), _good_quals(rng, 21, offset))]
    recs += [(_bases(rng, n), _good_quals(rng, n, offset)) for n in (33, 64, 7)]
    return _fastq(recs)


def _many_fastq(rng, n_rec, offset):
    kinds = _bad_kinds(offset)
    recs = []
    for i in range(n_rec):
        length = int(rng.randint(1, 41))
        b, q = _bases(rng, length), _good_quals(rng, length, offset)
        for _ in range(int(rng.randint(0, 3))):
            b, q = _spoil(b, q, int(rng.randint(0, length)), kinds[int(rng.randint(0, len(kinds)))], offset)
        recs.append((b, q))
    return _fastq(recs)


def _many_fasta(rng, n_rec):
    """records of 1 to 3 bases, every fifth with an N; three of 64 bases among them, for the k that the short ones do not reach"""
    recs = []
    for i in range(n_rec):
        b = _bases(rng, int(rng.randint(1, 4)))
        if i % 5 == 4:
            b = _put(b, int(rng.randint(0, len(b))), b"N" if i % 2 else b"n")
        recs.append((b">%d" % i, [b]))
        if i in (0, n_rec // 2, n_rec - 1):
            recs.append((b">long %d" % i, [_bases(rng, 64)]))
    return _fasta(recs)


SCAN_ROUNDS_LINES = SCAN_ROUND * SCAN_TILE + SCAN_TILE + 3000


def _scan_rounds(rng):
    """One base a line, a few lines that are '>' alone: more lines than one round of k_scan_one scans, records on both sides of the
    round's edge and one across it, one of them dropped for an N.  Returns the text and its reads, from the arrays."""
    n = SCAN_ROUNDS_LINES
    edge = SCAN_ROUND * SCAN_TILE
    codes = rng.randint(0, 4, size=n)
    first = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].copy()
    headers = [0, 10, 1000003, 2500000, edge - 4096 - 7, edge - 50, edge + 700, edge + 4096 + 100, edge + 4096 + 900, edge + 4096 + 2000, n - 40]
    first[headers] = ord(">")
    n_at = edge + 4096 + 500                     # an N in the record [edge + 4196, edge + 4996): dropped
    first[n_at] = ord("N")
    text = np.empty(2 * n, dtype=np.uint8)
    text[0::2] = first
    text[1::2] = 10
    reads = []
    for a, b in zip(headers, headers[1:] + [n]):
        if b - a > 1 and not a < n_at < b:
            reads.append(first[a + 1:b].tobytes().decode())
    return text.tobytes(), reads


@functools.lru_cache(maxsize=None)
def _built():
    rng = np.random.RandomState(SEED)
    out, reads = {}, {}

    def add(name, text, fastq, chunks=True):
        out[name] = (text, fastq, _chunks(text) if chunks else [])

    add("fa_tile_edges", _tile_edges(rng), False)
    for size in (8191, 8192, 8193, 16384):
        add("fa_tile_edges_%d" % size, _exact_size(rng, size, True), False)
        add("fa_tile_edges_%d_no_last_newline" % size, _exact_size(rng, size, False), False)
    add("fa_tile_edges_crlf", _exact_size(rng, 16500, True, crlf_at=T_TILE), False)
    add("fa_lengths", _lengths(rng), False)
    add("fa_shapes", _shapes(rng), False)
    add("fa_shapes_crlf", out["fa_shapes"][0].replace(b"\n", b"\r\n"), False)
    add("fa_probe_in_header", _probe_in_header(rng), False)
    add("fa_many_records", _many_fasta(rng, 9000), False)
    for offset in (33, 64):
        add("fq_pieces_%d" % offset, _pieces(rng, offset), True)
        add("fq_pieces_%d_crlf" % offset, out["fq_pieces_%d" % offset][0].replace(b"\n", b"\r\n"), True)
    add("fq_probe_in_quality", _probe_in_quality(rng), True)
    for offset in (33, 64):
        add("fq_long_record_%d" % offset, _long_record(rng, offset), True)
    add("fq_many", _many_fastq(rng, 5000, 33), True)
    text, reads[LARGE] = _scan_rounds(rng)
    add(LARGE, text, False, chunks=False)
    return out, reads


def cases():
    """name -> (text, fastq, chunk sizes)"""
    return _built()[0]


@functools.lru_cache(maxsize=None)
def case_reads(name):
    """the reads of a case: the oracle's, or for the large case the ones it was built from"""
    built, reads = _built()
    if name in reads:
        return tuple(reads[name])
    text, fastq, _ = built[name]
    return tuple(expected_reads(text, fastq))


@functools.lru_cache(maxsize=None)
def case_cuts(name, chunk):
    text, fastq, _ = cases()[name]
    return tuple(cuts(text, fastq, chunk, whole_reads=case_reads(name)))
