"""The counting tokeniser's kernels (csrc/tokenizer.h) and their driver (csrc/reads_file.hip) on the designed texts of
tests/tokenizer_cases.py, whole and cut into chunks of every listed size.  Three things are held, all exactly:
  * the device ran: MC_INGEST_DEBUG prints one line for every chunk the device did not decline, with the lines, reads and bases it
    found there; there must be one per cut of the model, each with the model's three numbers (a chunk that went to the host parser
    would give the right table all the same);
  * the reads: add_reads_file returns the oracle's number of reads, and for k = 1, 3, 11 and 31 the exported (key, count) table is
    the oracle's -- the small k see the pieces that a large k skips, k = 31 sees every base position and every join or split;
  * the read store: it advances by the words of the file's bases, as it does for one batch of the host reader (rs_append,
    csrc/mcgpu.hip: the bases of ONE batch, rounded up to whole words -- the host reader makes one batch of up to 2^20 reads, the
    deferred device path one of the whole file, so the two agree on every text here; several host batches would round up each).
Both store modes run: the default (chunks packed back to back into the read store and counted once) and set_read_pointers(0)
(words in a buffer of the chunk's own, counted chunk by chunk)."""
import functools
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import tokenizer_cases as tc
from tests.helpers import oracle_table

pytestmark = pytest.mark.gpu

KS = (1, 3, 11, 31)
CASES = tc.cases()
SMALL = [n for n in CASES if n != tc.LARGE]
CHUNK_LINE = re.compile(r"\[ingest\] device tokeniser: [0-9.]+ MB text, (\d+) lines, (\d+) reads, (\d+) bases")
CLOSING_LINE = re.compile(r"\[ingest\] device tokeniser: (\d+) chunk\(s\)")


@pytest.fixture(scope="module")
def mc():
    import metacherchant_amd as m
    m.native.load()
    return m


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("tokenizer_cases")
    out = {}
    for name, (text, fastq, _) in CASES.items():
        out[name] = d / (name + (".fq" if fastq else ".fa"))
        out[name].write_bytes(text)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(name, k):
    reads = tc.case_reads(name)
    codes = np.concatenate([po.encode(r) for r in reads])
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    t = oracle_table(codes, off, k, po.KEY_PACKED)[0]
    return (t.size(),) + t.dump()


def _words(name):
    return (sum(len(r) for r in tc.case_reads(name)) + tc.WORD - 1) // tc.WORD * tc.WORD


def _add_file(mc, path, k, monkeypatch, capfd, tokenizer="device", chunk=None, pointers=True):
    """one context, one file: (reads returned, the chunks' (lines, reads, bases), the closing line's chunk counts, how far the read
    store advanced, the table)"""
    monkeypatch.setenv("MC_TOKENIZER", tokenizer)
    monkeypatch.setenv("MC_INGEST_DEBUG", "1")
    if chunk is None:
        monkeypatch.delenv("MC_TOKENIZER_CHUNK_BYTES", raising=False)
    else:
        monkeypatch.setenv("MC_TOKENIZER_CHUNK_BYTES", str(chunk))
    ctx = mc.Context(k, mc.KEY_PACKED, 0, 0)
    try:
        if not pointers:
            ctx.set_read_pointers(0)
        at = ctx.read_store_tell()
        capfd.readouterr()
        n = ctx.add_reads_file(str(path))
        err = capfd.readouterr().err
        advanced = ctx.read_store_tell() - at
        size = ctx.finalize()
        keys, counts = ctx.export(0)
    finally:
        ctx.close()
    chunks = [tuple(int(x) for x in m.groups()) for m in CHUNK_LINE.finditer(err)]
    closing = [int(m.group(1)) for m in CLOSING_LINE.finditer(err)]
    return n, chunks, closing, advanced, (size, keys, counts)


_host_advance = {}


def _check(mc, paths, name, chunk, pointers, monkeypatch, capfd, ks=KS):
    cuts = tc.case_cuts(name, chunk)
    want_chunks = [(c.lines, c.reads, c.bases) for c in cuts]
    for k in ks:
        n, chunks, closing, advanced, table = _add_file(mc, paths[name], k, monkeypatch, capfd, chunk=chunk, pointers=pointers)
        print("%s chunk %s k %d pointers %d: %d chunk lines for %d cuts, closing %s, %d reads, store + %d, table %d" % (
            name, chunk, k, pointers, len(chunks), len(cuts), closing, n, advanced, table[0]))
        # the device ran, chunk by chunk
        assert len(chunks) == len(cuts), "chunks the device did not decline"
        assert closing == [len(cuts)]
        assert chunks == want_chunks
        # the reads
        assert n == len(tc.case_reads(name))
        size, keys, counts = _oracle(name, k)
        assert table[0] == size and np.array_equal(table[1], keys) and np.array_equal(table[2], counts), "k = %d" % k
        # the read store
        if pointers:
            if name not in _host_advance:
                _host_advance[name] = _add_file(mc, paths[name], k, monkeypatch, capfd, tokenizer="host")[3]
            assert advanced == _host_advance[name] == _words(name)
        else:
            assert advanced == 0


@pytest.mark.parametrize("name,chunk", [(n, c) for n in SMALL for c in [None] + CASES[n][2]], ids=lambda v: str(v))
def test_designed_text(mc, paths, monkeypatch, capfd, name, chunk):
    """the default store mode: the chunks are packed back to back into the read store (chunk i + 1 at a dst_base that is no multiple
    of 32, sharing a border word with chunk i) and counted once, at the end of the file"""
    _check(mc, paths, name, chunk, True, monkeypatch, capfd)


def _chunked_setting(name):
    """4096 where that cuts the file, 100 for the texts that are smaller"""
    return 4096 if len(tc.case_cuts(name, 4096)) > 1 else 100


@pytest.mark.parametrize("name,chunk", [(n, c) for n in SMALL for c in (None, _chunked_setting(n))], ids=lambda v: str(v))
def test_designed_text_without_a_read_store(mc, paths, monkeypatch, capfd, name, chunk):
    """set_read_pointers(0): every chunk's words go to a buffer of its own (own_words) and are counted as the chunk comes"""
    assert chunk is None or len(tc.case_cuts(name, chunk)) > 1
    _check(mc, paths, name, chunk, False, monkeypatch, capfd)


def test_scan_rounds(mc, paths, monkeypatch, capfd):
    """More than 1024 x 4096 lines in one chunk: k_scan_one scans the tile sums of the per-line scans in two rounds and carries from
    the first into the second.  Once, unchunked, k = 31."""
    assert tc.case_cuts(tc.LARGE, None)[0].lines > tc.SCAN_ROUND * tc.SCAN_TILE + tc.SCAN_TILE
    _check(mc, paths, tc.LARGE, None, True, monkeypatch, capfd, ks=(31,))


def test_device_tokeniser_feeds_the_read_store_in_chunks(mc, tmp_path, monkeypatch, capfd):
    """Read pointers behind about ten chunks: the reads of chunk i + 1 lie behind those of chunk i in the read store, and a BFS that
    walks by read pointers gives the oracle's answer in both directions."""
    from tests.helpers import assert_bfs_equal, seed_windows, synth_case
    genome, reads, off = synth_case(2, 30000, 12000, 150, 50)
    n = len(off) - 1
    text = "".join(">r%d\n%s\n" % (i, po.decode(reads[int(off[i]):int(off[i + 1])])) for i in range(n)).encode()
    p = tmp_path / "r.fasta"
    p.write_bytes(text)
    chunk = len(text) // 10
    n_cuts = len(tc.cut_positions(text, False, chunk))
    assert 9 <= n_cuts <= 11
    t, _ = oracle_table(reads, off, 31, po.KEY_PACKED)
    seed = genome[10000:10500]
    hi, lo = seed_windows(seed, 31)
    monkeypatch.setenv("MC_TOKENIZER", "device")
    monkeypatch.setenv("MC_INGEST_DEBUG", "1")
    monkeypatch.setenv("MC_TOKENIZER_CHUNK_BYTES", str(chunk))
    ctx = mc.Context(31, mc.KEY_PACKED, 0, 0)
    ctx.set_coverage_hint(5)
    capfd.readouterr()
    assert ctx.add_reads_file(str(p)) == n
    err = capfd.readouterr().err
    assert len(CHUNK_LINE.findall(err)) == n_cuts and [int(x) for x in CLOSING_LINE.findall(err)] == [n_cuts]
    assert sum(int(m.group(2)) for m in CHUNK_LINE.finditer(err)) == n
    assert ctx.read_store_tell() == (n * 150 + 31) // 32 * 32
    assert ctx.finalize() == t.size()
    assert_bfs_equal(ctx.bfs(hi, lo, 1, 5, 3000, -1), po.bfs(t, 31, po.KEY_PACKED, [seed], 1, 5, 3000, -1))
    assert_bfs_equal(ctx.bfs(hi, lo, -1, 3, 3000, 400), po.bfs(t, 31, po.KEY_PACKED, [seed], -1, 3, 3000, 400))
    ctx.close()
