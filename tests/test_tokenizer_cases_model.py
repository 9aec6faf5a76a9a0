"""tests/tokenizer_cases.py holds what it is for: the newlines sit at the tile edges, the lengths and start residues are all there,
the FASTQ pieces meet the lane edge in both carry states, the chunked runs pack behind every kind of border word, the two designed
probes land where they should, and no text holds anything the device would decline (tests/test_gpu_tokenizer_edges.py relies on
that: it asserts that no chunk went to the host parser)."""
import numpy as np
import pytest

from tests import tokenizer_cases as tc

CASES = tc.cases()
SMALL = [n for n in CASES if n != tc.LARGE]


def _newlines(text):
    return np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)


def test_constants_are_the_headers():
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metacherchant_amd", "csrc")
    src = "".join(open(os.path.join(root, f)).read() for f in ("device_types.h", "tokenizer_device.h", "switches.h"))
    assert re.search(r"T_THREADS = 256;", src) and re.search(r"T_BYTES = %d;" % tc.T_BYTES, src) and tc.T_TILE == 256 * tc.T_BYTES
    assert re.search(r"SCAN_TILE = %d;" % tc.SCAN_TILE, src) and re.search(r"WP_WORDS = %d;" % tc.WP_WORDS, src)
    assert tc.FLUSH == 2080 and "tokenizer_chunk_bytes = 1ull << 28" in src and tc.DEFAULT_CHUNK == 1 << 28


def test_tile_edges():
    text = CASES["fa_tile_edges"][0]
    nl = set(_newlines(text).tolist())
    assert set(tc.TILE_NEWLINES) <= nl
    assert {p % tc.T_TILE for p in tc.TILE_NEWLINES} >= {31, 32, 8190, 8191, 0, 1} and {p % tc.T_BYTES for p in tc.TILE_NEWLINES} >= {31, 0, 30, 1}
    lines = tc.lines_of(text)
    at = text.index(b">long\n") + 6
    assert len(lines[lines.index(b">long") + 1]) == tc.LONG_LINE
    first_tile = (at + tc.T_TILE - 1) // tc.T_TILE
    assert (first_tile + 2) * tc.T_TILE <= at + tc.LONG_LINE, "the long line covers two whole tiles"
    assert not nl & set(range(first_tile * tc.T_TILE, (first_tile + 2) * tc.T_TILE))
    for size in (8191, 8192, 8193, 16384):
        a, b = CASES["fa_tile_edges_%d" % size][0], CASES["fa_tile_edges_%d_no_last_newline" % size][0]
        assert len(a) == len(b) == size and a.endswith(b"\n") and not b.endswith(b"\n") and b[-1:] in b"ACGT"
    crlf = CASES["fa_tile_edges_crlf"][0]
    assert crlf[tc.T_TILE - 1:tc.T_TILE + 1] == b"\r\n" and crlf.count(b"\r\n") == crlf.count(b"\n") == crlf.count(b"\r")
    line = crlf[:tc.T_TILE - 1].rsplit(b"\n", 1)[1]
    assert line[:1] not in b">;" and len(line) == 60, "the line whose '\\r' ends the tile holds bases"


def test_lengths_and_start_residues():
    text = CASES["fa_lengths"][0]
    reads = tc.case_reads("fa_lengths")
    assert [len(r) for r in reads] == tc._lengths_order() and set(tc.LENGTHS) <= {len(r) for r in reads}
    assert set(range(1, 131)) | {2015, 2016, 2017, 2047, 2048, 2049, 2079, 2080, 2081, 2111, 2112, 2113, 4159, 4160, 4161, 6241} == set(tc.LENGTHS)
    starts = np.concatenate([[0], np.cumsum([len(r) for r in reads])])[:-1]
    assert {int(s) % tc.WORD for s in starts} == set(range(tc.WORD))
    for n in (32, 64):  # whole words only: no OR at either end
        assert sum(1 for s, r in zip(starts, reads) if len(r) == n and s % tc.WORD == 0) >= 2
    assert all(len(l) in tc.LENGTHS + [tc.WORD] for l in tc.lines_of(text) if l[:1] != b">")


def test_fasta_shapes():
    for name, eol in (("fa_shapes", b"\n"), ("fa_shapes_crlf", b"\r\n")):
        text = CASES[name][0]
        lines = text.split(b"\n")
        assert lines.pop() == b"" and lines[-1].startswith(b">a header at the very end")
        assert lines[0][:1] in b"ACGT", "bases in front of the first header"
        widths = {len(l.rstrip(b"\r")) for l in lines if l[:1] not in b">;"}
        assert set(tc.WIDTHS) <= widths
        assert (b"N" + eol) in text and any(l.rstrip(b"\r") == b"N" for l in lines)
        assert any(l[:1] == b";" for l in lines) and any(l.rstrip(b"\r") == b">" for l in lines)
        assert sum(1 for l in lines if l.startswith(tc.ODD_HEADER)) == len(tc.WIDTHS)
        assert (eol * 3) in text or (b"\r\n\r\n\r\n") in text
        body = b"".join(l for l in lines if l[:1] not in b">;")
        assert any(c in body for c in b"acgt") and b"n" in body and b"N" in body
        if eol == b"\r\n":
            assert b"\n\r\n" in text, "a line that is only '\\r'"
        reads = tc.case_reads(name)
        assert len(reads) == 1 + len(tc.WIDTHS) * 9  # of 14 records a width, 4 hold an N and one is empty
    assert tc.case_reads("fa_shapes") == tc.case_reads("fa_shapes_crlf")
    # the kept neighbours of a dropped record share a word
    reads = tc.case_reads("fa_shapes")
    starts = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    assert any(len(a) == 37 and len(b) == 45 and s % tc.WORD for a, b, s in zip(reads, reads[1:], starts[1:]))


def test_many_records_and_scan_rounds():
    text = CASES["fa_many_records"][0]
    lines = tc.lines_of(text)
    n_rec = sum(1 for l in lines if l[:1] == b">")
    assert len(lines) > 2 * tc.SCAN_TILE and n_rec > 2 * tc.SCAN_TILE
    short = [l for l in lines if l[:1] != b">" and len(l) <= 3]
    assert len(short) == 9000 and {len(l) for l in short} == {1, 2, 3} and sum(1 for l in short if b"N" in l or b"n" in l) == 1800
    text = CASES[tc.LARGE][0]
    assert tc.count_lines(text) == tc.SCAN_ROUNDS_LINES > tc.SCAN_ROUND * tc.SCAN_TILE + tc.SCAN_TILE
    assert CASES[tc.LARGE][2] == [] and len(text) < 9e6
    reads = tc.case_reads(tc.LARGE)
    edge = tc.SCAN_ROUND * tc.SCAN_TILE
    assert len(reads) == 10 and sum(len(r) for r in reads) == tc.SCAN_ROUNDS_LINES - 11 - 799
    # a record ends on either side of the round's edge, one lies across it, and the dropped one lies behind it
    hdr = np.flatnonzero(np.frombuffer(text, dtype=np.uint8)[0::2] == ord(">"))
    assert any(a < edge < b for a, b in zip(hdr, hdr[1:])) and (hdr < edge).sum() >= 3 and (hdr > edge + tc.SCAN_TILE).sum() >= 3
    assert text.index(b"N") // 2 > edge + tc.SCAN_TILE
    # (the oracle agrees on a slice that a test can afford to read line by line: the text's end, cut at a header)
    tail = text[2 * int(hdr[-4]):]  # (the dropped record and the three behind it)
    assert b"N" in tail and tuple(tc.expected_reads(tail, False)) == reads[-3:]


def _fq_shapes(name):
    """per record of a FASTQ case: (good mask, pieces)"""
    text = CASES[name][0]
    offset = tc.sniff_offset(text)
    out = []
    for d, q in tc.fq_records(text):
        good = tc.fq_good(d, q, offset)
        out.append((good, tc.pieces_of(good)))
    return out


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("fq_")])
def test_fastq_policy_restated_is_the_oracle(name):
    """cuts() counts a chunk's pieces with fq_good / pieces_of: together they give the oracle's reads"""
    text = CASES[name][0]
    got = []
    for (d, _), (_, pieces) in zip(tc.fq_records(text), _fq_shapes(name)):
        got += [d[s:s + n].decode().upper() for s, n in pieces]
    assert tuple(got) == tc.case_reads(name)


@pytest.mark.parametrize("name,offset", [("fq_pieces_33", 33), ("fq_pieces_64", 64), ("fq_pieces_33_crlf", 33), ("fq_pieces_64_crlf", 64)])
def test_fastq_pieces(name, offset):
    text = CASES[name][0]
    assert tc.sniff_offset(text) == offset
    if offset == 64:
        assert all(x >= 64 for _, q in tc.fq_records(text) for x in q)
    recs = tc.fq_records(text)
    shapes = _fq_shapes(name)
    assert {len(d) for d, _ in recs} >= set(tc.PIECE_LENGTHS)
    # every kind of bad base at every designed position
    kinds = {}
    for (d, q), (good, _) in zip(recs, shapes):
        for at in np.flatnonzero(~good):
            c = bytes([d[at]])
            kind = c if c in (b"N", b"n", b".") else "phred %d" % (q[at] - offset)
            for p in tc.BAD_POSITIONS:
                if at == (len(d) - 1 if p < 0 else p):
                    kinds.setdefault(p, set()).add(kind)
    want = {b"N", b"n", b".", "phred 0"} | ({"phred 64"} if offset == 33 else set())
    assert set(kinds) == set(tc.BAD_POSITIONS) and all(k == want for k in kinds.values()), kinds
    starts = [s for _, ps in shapes for s, _ in ps]
    assert any(not g[63] and g[64] for g, _ in shapes if len(g) > 64) and 64 in starts, "a piece starts at lane 0, carry = 0"
    assert any(g[63] and g[64] and not g[62] for g, _ in shapes if len(g) > 64), "a piece goes on over 63 -> 64, carry = 1"
    assert any(not g[127] and g[128] for g, _ in shapes if len(g) > 128) and any(g[127] and g[128] for g, _ in shapes if len(g) > 128)
    ones = {s for _, ps in shapes for s, n in ps if n == 1}
    assert {63, 64} <= ones
    assert any(len(g) and not g.any() for g, _ in shapes) and any(len(g) == 0 for g, _ in shapes)
    assert any(len(g) > 3 and not g[i:i + 3].any() for g, _ in shapes for i in (60, 62, 64))  # runs of bad bases at the edge
    assert any(b"~" in q for _, q in recs) and any(q[:1] == b"@" for _, q in recs)
    plus = [l for l in tc.lines_of(text)[2::4]]
    assert any(l == b"+" for l in plus) and any(len(l) > 1 for l in plus)
    if name.endswith("crlf"):
        assert text.count(b"\r\n") == text.count(b"\n") and tc.case_reads(name) == tc.case_reads(name[:-5])


def test_fastq_long_and_many():
    for offset in (33, 64):
        name = "fq_long_record_%d" % offset
        assert tc.sniff_offset(CASES[name][0]) == offset
        shapes = _fq_shapes(name)
        # the WavePacker flushes inside a record, with piece offsets still to come, and inside one piece
        assert any(int(g.sum()) > tc.FLUSH and len(ps) > 40 for g, ps in shapes) and any(n > tc.FLUSH for _, ps in shapes for _, n in ps)
        assert [len(g) for g, _ in shapes] == [5, 5000, 2200, 21, 33, 64, 7]
        assert not shapes[1][0][96::97].any() and int(shapes[1][0].sum()) == 5000 - 51
    shapes = _fq_shapes("fq_many")
    assert len(shapes) == 5000 > tc.SCAN_TILE and {len(g) for g, _ in shapes} == set(range(1, 41))
    lens = [n for _, ps in shapes for _, n in ps]
    assert sum(1 for n in lens if n < 11) > len(lens) // 4 and sum(1 for n in lens if n < 31) > len(lens) // 2


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_has_short_and_long_reads_and_nothing_to_decline(name):
    text, fastq, chunks = CASES[name]
    lens = {len(r) for r in tc.case_reads(name)}
    assert min(lens) < 31 <= max(lens)
    assert not tc.device_declines(text, fastq)
    if name != tc.LARGE:
        assert chunks[:3] == [64, 100, 4096] and chunks[3] + chunks[3] // 4 >= len(text) > (chunks[3] - 1) + (chunks[3] - 1) // 4
        assert len(text) * 4 // 5 <= chunks[3] <= len(text) * 4 // 5 + 2


def test_the_decline_scan_can_see():
    assert tc.device_declines(b">a\nACGTRACGT\n", False) and tc.device_declines(b">a\nAC\rGT\n", False) and tc.device_declines(b"AC GT\n", False)
    assert not tc.device_declines(b">R\r\nACGTn\r\n\r\n;x y\r\nacgt", False)
    assert tc.device_declines(b"@a\nACGT\n+\nIII\n", True) and tc.device_declines(b"@a\nACGT\n+\nIIII\n\n@b\nA\n+\nI\n", True)
    assert tc.device_declines(b"@a\nACGR\n+\nIIII\n", True) and tc.device_declines(b"@a\nACGT\n+\nII II\n"[:-2] + b"\n", True)
    assert tc.device_declines(b"@a\nACGT\n+\nhhhh\n" * 1000 + b"@a\nACGT\n+\nhh5h\n", True) and not tc.device_declines(b"@a\nACNT\n+\nhh5h\n", True)
    assert not tc.device_declines(b"@a\r\nAC.T\r\n+a\r\n@II~\r\n", True)


@pytest.mark.parametrize("name", SMALL)
def test_cuts(name):
    """every chunk begins a record, the chunks' lines, reads and bases add up to the file's, and a chunk's reads are the oracle's"""
    text, fastq, chunks = CASES[name]
    reads = tc.case_reads(name)
    n_lines = tc.count_lines(text)
    for chunk in [None] + chunks:
        cs = tc.case_cuts(name, chunk)
        assert cs[0].b == 0 and cs[-1].e == len(text) and all(a.e == b.b for a, b in zip(cs, cs[1:])) and all(c.e > c.b for c in cs)
        assert sum(c.reads for c in cs) == len(reads) and sum(c.bases for c in cs) == sum(len(r) for r in reads)
        assert sum(c.lines for c in cs) == n_lines
        for c in cs[1:]:
            assert text[c.b - 1:c.b] == b"\n" and text[c.b:c.b + 1] in (b"@" if fastq else b">;")
        if fastq:
            assert all(c.lines % 4 == 0 for c in cs)
        assert all(c.probe is None or (c.probe == c.b + max(chunk, tc.MIN_CHUNK) and c.e >= c.probe) for c in cs)
    assert len(tc.case_cuts(name, None)) == 1 and len(tc.case_cuts(name, chunks[3])) == 1 and len(tc.case_cuts(name, 64)) > 3
    # the reads of a chunk are a slice of the file's reads (FASTQ: test_fastq_policy_restated_is_the_oracle, record by record)
    at = 0
    for c in tc.case_cuts(name, 100) if not fastq else ():
        assert tuple(tc.expected_reads(text[c.b:c.e], False)) == reads[at:at + c.reads]
        at += c.reads


def test_cuts_pack_behind_every_kind_of_border_word():
    residues = set()
    for name in SMALL:
        for chunk in CASES[name][2]:
            residues |= {b % tc.WORD for b in tc.dst_bases(tc.case_cuts(name, chunk))[1:]}
    assert {0, 31} <= residues and len(residues) >= 16, sorted(residues)
    # and one case alone, so that a run of it is enough
    for name in ("fa_lengths", "fq_pieces_33"):
        got = {b % tc.WORD for chunk in CASES[name][2] for b in tc.dst_bases(tc.case_cuts(name, chunk))[1:]}
        assert len(got) >= 16, (name, sorted(got))


def test_the_designed_probes():
    # FASTA: byte 64 is a '>' inside a header
    text = CASES["fa_probe_in_header"][0]
    c = tc.case_cuts("fa_probe_in_header", 64)[0]
    line_start = text.rfind(b"\n", 0, c.probe) + 1
    assert c.probe == 64 and text[line_start:line_start + 1] == b">" and line_start < 64 and text[64:65] == b">"
    assert c.e == text.index(b"\n", 64) + 1 + 41 + 13 and text[c.e:c.e + 3] == b">r0"
    # FASTQ: byte 64 lies in a quality line that begins with '@' ...
    text = CASES["fq_probe_in_quality"][0]
    lines = text.split(b"\n")
    c = tc.case_cuts("fq_probe_in_quality", 64)[0]
    line_start = text.rfind(b"\n", 0, c.probe) + 1
    assert c.probe == 64 and line_start == len(b"\n".join(lines[:3])) + 1 and lines[3][:1] == b"@" and line_start < 64
    assert c.e == len(b"\n".join(lines[:4])) + 1
    # ... and byte 100 in the '+' line in front of one, which is then the first line plain_record_start looks at
    c = tc.case_cuts("fq_probe_in_quality", 100)[0]
    line_start = text.rfind(b"\n", 0, c.probe) + 1
    assert c.probe == 100 and line_start == len(b"\n".join(lines[:6])) + 1 and lines[6][:1] == b"+" and lines[7][:1] == b"@"
    assert c.e == len(b"\n".join(lines[:8])) + 1 and tc.record_start(text, True, c.e - len(lines[7])) == c.e


@pytest.fixture(scope="module")
def hosttest():
    import os
    from metacherchant_amd import build
    build.build_host()
    assert os.path.exists(build.HOSTTEST)
    return build.HOSTTEST


@pytest.mark.parametrize("name", list(CASES))
def test_plain_chunks_is_the_model(name, hosttest):
    """`mc_hosttest cuts` (csrc/host/reads_io.cpp plain_chunks, the one cut rule of the library, the CLI's WholeReadsSource and
    mc_hosttest) prints cut_positions' chunks, at the designed chunk sizes and the switch's default (the small texts: the default's
    one chunk says nothing more about a text of megabytes)."""
    import subprocess
    text, fastq, _ = CASES[name]
    chunks = tc._chunks(text) + ([None] if name != tc.LARGE else [])

    def run(path):
        return {c: subprocess.check_output([hosttest, "cuts", path] + ([] if c is None else [str(c)]), text=True) for c in chunks}
    got = tc._with_file(text, fastq, run)
    for c in chunks:
        want = [(b, e) for b, e, _ in tc.cut_positions(text, fastq, c)]
        assert [tuple(int(x) for x in line.split()) for line in got[c].splitlines()] == want, (name, c)
        assert want[0][0] == 0 and want[-1][1] == len(text)
