"""DnaQReader (csrc/host/reads_io.cpp) restated in Python: the text of a FASTQ / FASTA file in, every read whole with a code and a phred
a base out -- what the classifying tools read their -r files with, and what mc_tokenize_whole has to give on the device.  The reader
restates readDnaQLazy of the reference (itmo!/io/ReadersUtils.java:185-215, FastqReader.java:53-82, FastaWithNsReader,
DnaQBuilder.java:32-45).  tests/test_whole_reads_model.py holds this model to the C++ reader (mc_hosttest dnaq); tests/test_gpu_whole_reads.py
holds the kernels to this model.  cases() are the inputs both use."""
import numpy as np

UNKNOWN = b"Nn."
_CODE = np.full(256, -1, dtype=np.int16)
for _i, _c in enumerate("AGCT"):  # itmo!/dna/DnaTools.java:31
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i
_UNKNOWN = np.zeros(256, dtype=bool)
_UNKNOWN[list(UNKNOWN)] = True


class ReaderError(Exception):
    """what DnaQReader throws (mch::Error): str() is its message"""


def lines_of(text):
    """LineSource::getline / MemLines::getline: the pieces between '\\n's (none behind the last one), one trailing '\\r' off each"""
    if not text:
        return []
    parts = text.split(b"\n")
    if text.endswith(b"\n"):
        parts.pop()
    return [p[:-1] if p.endswith(b"\r") else p for p in parts]


def _fastq_records(lines):
    """DnaQReader::Impl::fastq_record over the lines: (bases, qualities) pairs; raises as it throws"""
    it = iter(lines)

    def data_line():  # FastqReader.readNextDataLine: empty lines skipped, a line starting with '@' or '+', then the content line
        for line in it:
            if line:
                break
        else:
            return None
        if line[:1] not in (b"@", b"+"):
            raise ReaderError('Unknown structure of fastq file! Waiting "@ID" or "+ID" string')
        out = next(it, None)
        if out is None:
            raise ReaderError("Unexpected end of file. File is corrupted/Format mismatch.")
        return out

    while True:
        data = data_line()
        if data is None:
            return
        qual = data_line()
        if qual is None:
            raise ReaderError("Unexpected end of file. File is corrupted/Format mismatch.")
        if len(data) != len(qual):
            raise ReaderError("Bad DnaQ record: length of chars and quality is not the same.")
        yield data, qual


def _fasta_records(lines):
    """FastaWithNsReader.readNextDataLine: the lines between two '>' / ';' lines joined; empty records give nothing"""
    data = []
    for line in lines:
        if line[:1] in (b">", b";"):
            if any(data):
                yield b"".join(data)
            data = []
        else:
            data.append(line)
    if any(data):
        yield b"".join(data)


def sniff_offset(lines):
    """ReadersUtils.determineQualityFormat as DnaQReader does it: Illumina (64) unless, in the first 1000 records, a base that is not
    N n . has a quality char below 64 or above 126 -- then Sanger (33).  Raises what the reader's constructor throws."""
    for r, (data, qual) in enumerate(_fastq_records(lines)):
        if r >= 1000:
            break
        d, q = np.frombuffer(data, dtype=np.uint8), np.frombuffer(qual, dtype=np.uint8)
        if np.any(~_UNKNOWN[d] & ((q < 64) | (q > 126))):
            return 33
    return 64


class WholeReads:
    """offset: the quality offset found (0 for FASTA); codes, phred: a byte a base; offsets: n_reads + 1; bad_pos: per read the one
    position with phred < 10, -1 none, -2 several; error: the reader's message when it threw (the reads before it are here)"""

    def __init__(self, offset):
        self.offset, self.error = offset, None
        self._codes, self._phred, self._lens = [], [], []

    def _finish(self):
        z = np.zeros(0, dtype=np.uint8)
        self.codes = np.concatenate(self._codes + [z])
        self.phred = np.concatenate(self._phred + [z])
        self.offsets = np.concatenate([[0], np.cumsum(np.array(self._lens, dtype=np.uint64))]).astype(np.uint64)
        self.n_reads = len(self._lens)
        bad = np.full(self.n_reads, -1, dtype=np.int32)
        for r in range(self.n_reads):  # findReadWithCorrection's count of phred < 10 (csrc/host/device.h bad_positions)
            low = np.flatnonzero(self.phred[int(self.offsets[r]):int(self.offsets[r + 1])] < 10)
            if len(low):
                bad[r] = low[0] if len(low) == 1 else -2
        self.bad_pos = bad
        return self

    def words(self):
        """the bases packed as mc_classify_reads takes them, the pad word included"""
        n = len(self.codes)
        w = np.zeros((n + 31) // 32 + 1, dtype=np.uint64)
        if n:
            c = np.concatenate([self.codes & 3, np.zeros((-n) % 32, dtype=np.uint8)]).reshape(-1, 32).astype(np.uint64)
            w[:len(c)] = np.bitwise_or.reduce(c << (np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64)), axis=1)
        return w


def read_whole(text, fastq):
    """DnaQReader over a file with these bytes: a WholeReads"""
    lines = lines_of(text)
    if not fastq:
        out = WholeReads(0)
        records = ((d, None) for d in _fasta_records(lines))
    else:
        try:
            out = WholeReads(sniff_offset(lines))
        except ReaderError as e:  # (the constructor throws: no read is delivered)
            out = WholeReads(0)
            out.error = str(e)
            return out._finish()
        records = _fastq_records(lines)
    try:
        for data, qual in records:
            d = np.frombuffer(data, dtype=np.uint8)
            unknown = _UNKNOWN[d]
            code = _CODE[d]
            bad = np.flatnonzero(~unknown & (code < 0))
            if len(bad):
                raise ReaderError("read contains the character '%s': IUPAC codes other than N are replaced at random by the reference "
                                  "(itmo!/dna/DnaTools.java:66-117), which has no defined result; rejecting the input" % chr(d[bad[0]]))
            if fastq:
                q = np.frombuffer(qual, dtype=np.uint8).astype(np.int32)
                wrong = np.flatnonzero(~unknown & ((q < out.offset) | (q > 126)))
                if len(wrong):
                    qc = int(q[wrong[0]])
                    raise ReaderError('Invalid quality code char: "%s" char code = %d' % (chr(qc), qc))
                ph = (q - out.offset) & 63  # (DnaQ keeps the phred in 6 bits)
            else:
                ph = np.full(len(d), 20, dtype=np.int32)  # ReadersUtils.DEFAULT_PHRED_FOR_FASTA
            out._codes.append(np.where(unknown, 0, code).astype(np.uint8))
            out._phred.append(np.where(unknown, 0, ph).astype(np.uint8))
            out._lens.append(len(d))
    except ReaderError as e:
        out.error = str(e)
    return out._finish()


# ---------------------------------------------------------------------------------------------------------------- the tests' inputs

def _bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))


def _quals(rng, n, offset, lo=10, hi=41):
    return bytes((rng.randint(lo, hi, size=n) + offset).astype(np.uint8))


def fastq_text(reads, eol=b"\n", last_eol=True, plus=b"+"):
    """reads: (bases, qualities) pairs"""
    lines = []
    for i, (b, q) in enumerate(reads):
        lines += [b"@r%d" % i, b, plus, q]
    t = eol.join(lines)
    return t + eol if last_eol else t


def fasta_text(records, width, eol=b"\n", last_eol=True):
    """records: (header line, bases) pairs; bases folded at `width`"""
    lines = []
    for h, b in records:
        if h is not None:
            lines.append(h)
        lines += [b[i:i + width] for i in range(0, len(b), width)]
    t = eol.join(lines)
    return t + eol if last_eol else t


LENGTHS = [31, 1, 0, 33, 2017, 63, 65, 2081, 127, 129, 150, 5000, 32, 64, 128, 2016]  # (odd sums first: neighbours share words)


def _put(s, at, c):
    return s[:at] + c + s[at + 1:]


def cases():
    """name -> (text, fastq, declined): what mc_tokenize_whole has to decline, and what it must not"""
    rng = np.random.RandomState(20240607)
    out = {}

    def rq(n, offset=33, **kw):
        return _bases(rng, n), _quals(rng, n, offset, **kw)

    reads = [rq(n) for n in LENGTHS]
    out["lengths"] = (fastq_text(reads), True, False)
    out["lengths_with_ones"] = (fastq_text([x for r in reads for x in (r, rq(1))]), True, False)

    # N n . at the first base, the last, 31, 32, 63, 64; all N; lower case
    unk = []
    for at in (0, 129, 31, 32, 63, 64):
        for c in (b"N", b"n", b"."):
            b, q = rq(130)
            unk.append((_put(b, at, c), q))
    b, q = rq(130)
    for at in (0, 129, 31, 32, 63, 64):
        b = _put(b, at, b"N")
    unk += [(b, q), (b"N" * 70, rq(70)[1]), (b"n" * 64, rq(64)[1]), (b"." * 65, rq(65)[1])]
    unk += [(x.lower(), y) for x, y in (rq(100), rq(64), rq(33))]
    out["unknown_bases"] = (fastq_text(unk), True, False)

    def with_phreds(n, lows, offset, low_phred=9):  # a read whose positions `lows` have phred 9 and the others 10 or more
        b, q = rq(n, offset)
        for at in lows:
            q = _put(q, at, bytes([offset + low_phred]))
        return b, q

    for offset in (33, 64):
        ph = [rq(130, offset) for _ in range(4)]                                       # no low position
        ph += [with_phreds(130, [at], offset) for at in (0, 63, 64, 129)]              # one, at a stretch's end
        ph += [with_phreds(130, [10, 100], offset), with_phreds(130, [3, 40], offset)]  # two: one a stretch, both in one
        ph += [with_phreds(200, [0, 199], offset), with_phreds(64, [63], offset), with_phreds(65, [64], offset)]
        ph += [with_phreds(130, [70], offset, low_phred=0)]
        b, q = rq(130, offset)
        ph.append((b, _put(_put(q, 50, bytes([offset + 9])), 51, bytes([offset + 10]))))  # phreds 9 and 10 side by side
        ph.append((b, _put(_put(q, 50, bytes([offset + 10])), 51, bytes([offset + 9]))))
        b, q = rq(130, offset)
        ph.append((_put(b, 77, b"N"), q))                                              # an N as the only low position
        ph.append((_put(b, 77, b"N"), _put(q, 12, bytes([offset + 3]))))               # ... and as one of two
        b, q = rq(130, offset)
        ph.append((b, _put(q, 5, b"~")))  # quality char 126: phred 93 & 63 = 29 at offset 33, 62 at offset 64
        out["phred_%d" % offset] = (fastq_text(ph), True, False)

    some = [rq(n) for n in (150, 0, 64, 1, 129, 31)]
    out["crlf"] = (fastq_text(some, eol=b"\r\n"), True, False)
    out["no_last_newline"] = (fastq_text(some, last_eol=False), True, False)
    out["crlf_no_last_newline"] = (fastq_text(some, eol=b"\r\n", last_eol=False), True, False)
    out["size_20000"] = (fastq_text([with_phreds(n, [n // 2] if n % 3 == 0 else [], 33) for n in rng.randint(20, 61, size=20000)]), True, False)

    for width in (60, 64, 70):
        recs = [(b">s%d x" % i, _bases(rng, n)) for i, n in enumerate([1, 59, 60, 61, 64, 65, 70, 71, 127, 128, 129, 140, 400, 2081])]
        out["fasta_%d" % width] = (fasta_text(recs, width), False, False)
    fa = [(None, _bases(rng, 90)), (b";old style", _bases(rng, 100)), (b">empty", b""), (b">after two headers", _bases(rng, 61))]
    n1 = _put(_bases(rng, 150), 64, b"N")
    n2 = _put(_put(_bases(rng, 150), 3, b"n"), 140, b".")
    fa += [(b">one N", n1), (b">two", n2), (b">all", b"N" * 61), (b">lower", _bases(rng, 75).lower())]
    t = fasta_text(fa, 60)
    t = t.replace(b">lower\n", b">gap\n" + _bases(rng, 60) + b"\n\n" + _bases(rng, 17) + b"\n>lower\n")  # an empty line inside a record
    out["fasta_shapes"] = (t, False, False)
    out["fasta_crlf_no_last_newline"] = (fasta_text(fa, 64, eol=b"\r\n", last_eol=False), False, False)
    out["fasta_100000"] = (fasta_text([(b">a", _bases(rng, 77)), (b">long", _put(_bases(rng, 100000), 70001, b"N")), (b">b", _bases(rng, 33))], 70), False, False)

    # what the device declines: the host reader gives its error, or its laxer reading
    good = [rq(n) for n in (40, 64, 65, 31, 50, 70)]
    bad = list(good)
    bad[3] = (_put(good[3][0], 7, b"R"), good[3][1])
    out["declined_R"] = (fastq_text(bad), True, True)
    bad = list(good)
    bad[4] = (good[4][0], _put(good[4][1], 9, b" "))
    out["declined_quality"] = (fastq_text(bad), True, True)
    bad = list(good)
    bad[2] = (good[2][0], good[2][1][:-1])
    out["declined_lengths"] = (fastq_text(bad), True, True)
    t = fastq_text(good)
    out["declined_blank_line"] = (t.replace(b"\n@r3\n", b"\n\n@r3\n"), True, True)
    out["declined_three_lines"] = (fastq_text(good[:-1]) + b"@r5\n" + good[-1][0] + b"\n+\n", True, True)
    out["declined_plus_first"] = (t.replace(b"\n@r2\n", b"\n+r2\n"), True, True)
    out["declined_fasta_R"] = (fasta_text([(b">a", _bases(rng, 100)), (b">b", _put(_bases(rng, 100), 64, b"R"))], 60), False, True)
    return out
