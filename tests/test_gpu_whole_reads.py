"""GPU: mc_tokenize_whole (csrc/whole_reads.hip) against the model of DnaQReader (tests/whole_reads_model.py), array for array: the
packed words, the offsets, the low-quality positions, and a byte a base of codes and phreds.  The inputs are the model's cases(): every
read length around the 64-lane stretch, the 32-base word and the WavePacker's flush; N n . at the stretches' ends; both quality offsets;
line endings; FASTA shapes; 20 000 records (several tiles of the newline passes and of the scans); and what the device has to decline."""
import numpy as np
import pytest

from tests import whole_reads_model as wm

pytestmark = pytest.mark.gpu

CASES = wm.cases()


@pytest.fixture(scope="module")
def ctx():
    import metacherchant_amd as m
    with m.Context(21) as c:
        yield c


@pytest.fixture(scope="module")
def models():
    return {name: wm.read_whole(text, fastq) for name, (text, fastq, _) in CASES.items()}


def _equal(got, m, tag):
    assert got is not None, (tag, "declined")
    assert got["n_reads"] == m.n_reads and got["n_bases"] == len(m.codes), (tag, got["n_reads"], got["n_bases"])
    assert np.array_equal(got["offsets"], m.offsets), tag
    for name, want in (("codes", m.codes), ("phred", m.phred), ("bad_pos", m.bad_pos), ("words", m.words())):
        diff = np.flatnonzero(got[name] != want) if len(got[name]) == len(want) else None
        assert diff is not None and len(diff) == 0, (tag, name, len(got[name]), len(want), None if diff is None else diff[:8].tolist())


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if not c[2]))
def test_whole_reads_are_the_models(ctx, models, name):
    import metacherchant_amd as m
    text, fastq, _ = CASES[name]
    mod = models[name]
    assert mod.error is None
    got = m.tokenize_whole(ctx, text, fastq, mod.offset or 33)
    _equal(got, mod, name)
    # without the byte arrays: the same words, offsets and positions
    lean = m.tokenize_whole(ctx, text, fastq, mod.offset or 33, codes=False, phred=False)
    assert lean["codes"] is None and lean["phred"] is None
    for key in ("words", "offsets", "bad_pos"):
        assert np.array_equal(lean[key], got[key]), (name, key)


def test_the_cases_hold_what_they_are_for(models):
    """(the inputs, not the kernels: every position a case is there for is in it)"""
    ph = models["phred_33"]
    assert {-2, -1, 0, 63, 64, 129, 77}.issubset(set(ph.bad_pos.tolist())) and 93 & 63 in ph.phred.tolist()
    assert models["phred_64"].offset == 64 and 62 in models["phred_64"].phred.tolist()
    lens = np.diff(models["lengths"].offsets.astype(np.int64)).tolist()
    assert sorted(lens) == sorted(wm.LENGTHS) and (models["lengths"].offsets[1:-1] % 32 != 0).sum() >= 10
    fa = models["fasta_shapes"]
    assert fa.n_reads == 8 and fa.bad_pos.tolist() == [-1, -1, -1, 64, -2, -2, -1, -1]
    assert models["fasta_100000"].bad_pos.tolist() == [-1, 70001, -1]
    assert models["size_20000"].n_reads == 20000


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c[2]))
def test_the_device_declines_what_the_host_reader_defines(ctx, models, name):
    import metacherchant_amd as m
    text, fastq, _ = CASES[name]
    # (the offset the host reader finds; a file whose first records throw has none: Sanger, as every case here is)
    assert m.tokenize_whole(ctx, text, fastq, models[name].offset or 33) is None
    assert m.tokenize_whole_dev(ctx, text, fastq, models[name].offset or 33) is None


def test_a_quality_char_below_the_offset_declines_only_at_that_offset(ctx):
    import metacherchant_amd as m
    text = b"@a\nACGT\n+\nII5I\n"  # '5' is 53: phred 20 at offset 33, below the offset at 64
    got = m.tokenize_whole(ctx, text, True, 33)
    assert got["phred"].tolist() == [40, 40, 20, 40]
    assert m.tokenize_whole(ctx, text, True, 64) is None
    assert m.tokenize_whole(ctx, b"@a\nACNT\n+\nII5I\n", True, 64)["phred"].tolist() == [9, 9, 0, 9]  # (an N's quality char is not looked at)


def test_two_calls_give_the_same_bytes_and_no_text_gives_no_reads(ctx):
    import metacherchant_amd as m
    for name in ("lengths_with_ones", "fasta_70", "size_20000"):
        text, fastq, _ = CASES[name]
        a, b = m.tokenize_whole(ctx, text, fastq, 33), m.tokenize_whole(ctx, text, fastq, 33)
        for key in ("words", "offsets", "bad_pos", "codes", "phred"):
            assert a[key].tobytes() == b[key].tobytes(), (name, key)
    for fastq in (False, True):
        e = m.tokenize_whole(ctx, b"", fastq, 33)
        assert e["n_reads"] == 0 and e["n_bases"] == 0 and e["offsets"].tolist() == [0] and e["words"].tolist() == [0]
        assert len(e["bad_pos"]) == 0 and len(e["codes"]) == 0 and len(e["phred"]) == 0


def test_wrong_arguments_are_errors(ctx):
    import metacherchant_amd as m
    with pytest.raises(m.McError, match="phred offset"):
        m.tokenize_whole(ctx, b"@a\nA\n+\nI\n", True, 50)


def test_the_device_result_goes_straight_into_classify_reads_dev(models):
    """the words, offsets and bad positions of tokenize_whole_dev, never on the host, give mc_classify_reads_dev the coverage that
    mc_classify_reads gives on the model's arrays"""
    import torch
    import metacherchant_amd as m
    from metacherchant_amd import native
    k = 21
    text, fastq, _ = CASES["size_20000"]
    mod = models["size_20000"]
    with m.Context(k) as c:
        # the graph: the first half of the reads themselves, so that some reads are covered and some are not
        half = mod.n_reads // 2
        c.add_reads_packed(native.Context._words(mod.codes[:int(mod.offsets[half])], mod.offsets[:half + 1], False), mod.offsets[:half + 1])
        c.finalize()
        for corr in (False, True):
            want = c.classify_reads(mod.codes, mod.offsets, mod.bad_pos if corr else None, found=50, correction=corr)
            with m.tokenize_whole_dev(c, text, fastq, mod.offset, codes=False, phred=False) as d:
                assert d.n_reads == mod.n_reads and d.d_codes == 0 and d.d_phred == 0
                out = torch.zeros(d.n_reads * 12, dtype=torch.uint8, device="cuda")
                c.classify_reads_dev(d.d_words, d.d_offsets, d.n_reads, out, d.d_bad_pos if corr else None, found=50, correction=corr)
                got = out.cpu().numpy().view(native.READ_COV_DTYPE)
            assert np.array_equal(got["sum"], want[0]) and np.array_equal(got["covered"], want[1]) and np.array_equal(got["last"], want[2])
            assert np.array_equal(got["found"].astype(bool), want[3])
            assert want[3].any() and not want[3].all() and (want[1] > 0).any()


@pytest.mark.parametrize("name", ["lengths_with_ones", "unknown_bases", "fasta_70"])
def test_slices_of_a_device_result_join_into_one_array(ctx, models, name):
    """mc_reads_append_dev: slices of a result -- cut so that the joins fall inside words, at word ends, and around reads of length 0 and
    empty slices -- appended one behind the other give the model's words, pad word and offsets again; then the same reads once more
    behind them, so that a join also starts from an array that does not end at a word"""
    import torch
    import metacherchant_amd as m
    text, fastq, _ = CASES[name]
    mod = models[name]
    n, nb = mod.n_reads, len(mod.codes)
    cuts = sorted({0, 1, 2, 3, 3, n // 3, n // 3, n // 2, n - 1, n})
    cuts = [0, 0] + cuts[1:] + [n]  # (an empty slice first and last)
    with m.tokenize_whole_dev(ctx, text, fastq, mod.offset or 33, codes=False, phred=False) as d:
        n_words = (2 * nb + 31) // 32 + 1
        words = torch.full((n_words + 4,), -1, dtype=torch.int64, device="cuda")  # (ones: what the call does not write shows)
        words[0] = 0
        offsets = torch.full((2 * n + 1,), -1, dtype=torch.int64, device="cuda")
        offsets[0] = 0
        at_reads = 0
        for rep in range(2):
            for a, b in zip(cuts, cuts[1:]):
                dst_bases = rep * nb + int(mod.offsets[a])
                m.reads_append_dev(ctx, d.d_words, d.d_offsets + 8 * a, b - a, words, dst_bases, offsets.data_ptr() + 8 * at_reads)
                at_reads += b - a
        assert at_reads == 2 * n
        got_w, got_o = words.cpu().numpy().view(np.uint64), offsets.cpu().numpy().view(np.uint64)
    two = wm.WholeReads(0)
    two._codes, two._phred, two._lens = [mod.codes, mod.codes], [mod.phred, mod.phred], np.diff(mod.offsets.astype(np.int64)).tolist() * 2
    two._finish()
    assert np.array_equal(got_o, two.offsets)
    assert np.array_equal(got_w[:n_words], two.words()), np.flatnonzero(got_w[:n_words] != two.words())[:8]
    assert (got_w[n_words:] == np.uint64(2**64 - 1)).all()  # nothing behind the pad word was touched
