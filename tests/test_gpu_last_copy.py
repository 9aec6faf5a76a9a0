"""GPU: mc_reads_last_copy against a dict of the reads' bases (tests/triple_classifier_model.py last_copy), with the full fingerprint
and with the tests' 4-bit one (MC_LAST_COPY_WEAK_FP), which makes distinct reads collide and runs the exact resolution."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import metacherchant_amd as m
    with m.Context(31, m.KEY_PACKED, 0, 0) as c:
        yield c


def _want(codes, off):
    """the greatest index of a read with the same bases, by a dict (vectorised: reads as bytes)"""
    last = {}
    keys = [codes[off[i]:off[i + 1]].tobytes() for i in range(len(off) - 1)]
    for i, kb in enumerate(keys):
        last[kb] = i
    return np.array([last[kb] for kb in keys], dtype=np.uint32)


def _layout(reads):
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    codes = np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads]) if reads else np.zeros(0, dtype=np.uint8)
    return codes, off


def _check(ctx, reads, lead=0):
    """lead: bases of a throw-away first read, so every read starts at another bit alignment"""
    if lead:
        reads = [np.zeros(lead, dtype=np.uint8)] + list(reads)
    codes, off = _layout(reads)
    want = _want(codes, off)
    for weak in (False, True):
        got = ctx.reads_last_copy(codes, off, weak=weak)
        assert got.dtype == np.uint32 and len(got) == len(reads)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (weak, lead, bad[:5], got[bad[:5]], want[bad[:5]])
    return want


def test_no_read_and_one_read(ctx):
    assert len(ctx.reads_last_copy(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))) == 0
    assert ctx.reads_last_copy(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), weak=True).tolist() == []
    for L in (0, 1, 150):
        assert _check(ctx, [np.full(L, 2, dtype=np.uint8)]).tolist() == [0]


def test_heavy_duplication(ctx):
    rng = np.random.default_rng(1)
    one = rng.integers(0, 4, 150).astype(np.uint8)
    others = [rng.integers(0, 4, int(rng.integers(0, 200))).astype(np.uint8) for _ in range(50)]
    reads = [one] * 10000
    for i in range(3000):  # others interleaved, with copies of their own
        reads.insert(int(rng.integers(0, len(reads))), others[i % 50])
    want = _check(ctx, reads)
    assert np.sum(want == want[[i for i, r in enumerate(reads) if r is one][0]]) == 10000


def test_reads_that_differ_in_one_base(ctx):
    rng = np.random.default_rng(2)
    base = rng.integers(0, 4, 150).astype(np.uint8)
    reads = []
    for p in (0, 1, 31, 32, 33, 63, 64, 75, 95, 96, 127, 128, 149):  # the first, middle and last words
        r = base.copy()
        r[p] = (r[p] + 1) % 4
        reads += [r, base.copy(), r.copy()]
    for lead in (0, 1, 17, 31):
        _check(ctx, reads, lead)


def test_a_read_that_is_a_prefix_of_another(ctx):
    rng = np.random.default_rng(3)
    long_r = rng.integers(0, 4, 100).astype(np.uint8)
    reads = [long_r[:L].copy() for L in (0, 1, 31, 32, 33, 64, 99, 100)] * 3
    reads += [np.zeros(L, dtype=np.uint8) for L in (0, 1, 31, 32, 33)]  # poly-A: only the length tells them apart
    for lead in (0, 5):
        _check(ctx, reads, lead)


def test_every_length_at_every_bit_alignment(ctx):
    rng = np.random.default_rng(4)
    templates = {L: [rng.integers(0, 4, L).astype(np.uint8) for _ in range(3)] for L in (0, 1, 31, 32, 33, 64, 150)}
    reads = []
    for _ in range(400):
        L = list(templates)[int(rng.integers(0, len(templates)))]
        reads.append(templates[L][int(rng.integers(0, 3))].copy())
    for lead in range(32):
        _check(ctx, reads, lead)


def test_a_million_reads(ctx):
    """several blocks of the radix sort, and the collision path with 16 fingerprints for a million reads"""
    rng = np.random.default_rng(5)
    n = 1 << 20
    pool = rng.integers(0, 4, (200000, 100)).astype(np.uint8)
    pick = rng.integers(0, len(pool), n)
    lens = rng.integers(90, 101, n)
    reads = [pool[p, :L] for p, L in zip(pick, lens)]
    codes, off = _layout(reads)
    # the dict, by the reads' bytes
    keys = np.array([codes[off[i]:off[i + 1]].tobytes() for i in range(n)], dtype=object)
    last = {}
    for i, kb in enumerate(keys):
        last[kb] = i
    want = np.array([last[kb] for kb in keys], dtype=np.uint32)
    assert np.sum(want != np.arange(n)) > n // 10  # (a fifth of the reads have a later copy)
    for weak in (False, True):
        got = ctx.reads_last_copy(codes, off, weak=weak)
        assert np.array_equal(got, want), (weak, np.nonzero(got != want)[0][:5])


def test_dev_entry_point_and_limits(ctx):
    import torch
    import metacherchant_amd as m
    rng = np.random.default_rng(6)
    reads = [rng.integers(0, 4, 40).astype(np.uint8) for _ in range(20)] * 2
    codes, off = _layout(reads)
    words = ctx._words(codes, off, None)
    d_w = torch.from_numpy(words.view(np.int64)).cuda()
    d_o = torch.from_numpy(off.view(np.int64)).cuda()
    d_last = torch.zeros(len(reads), dtype=torch.int32, device="cuda")
    ctx.reads_last_copy_dev(d_w, d_o, len(reads), d_last)
    torch.cuda.synchronize()
    assert np.array_equal(d_last.cpu().numpy().view(np.uint32), _want(codes, off))
    with pytest.raises(m.McError):
        ctx.reads_last_copy_dev(d_w, d_o, 1 << 32, d_last)
