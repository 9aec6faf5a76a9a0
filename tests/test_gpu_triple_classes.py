"""GPU: the triple-reads-classifier's two passes through the C ABI -- mc_classify_reads at k and k2, mc_reads_last_copy and
mc_triple_classes -- against the model (tests/triple_classifier_model.py) over the oracle's tables."""
import numpy as np
import pytest

from tests import classifier_model as cm
from tests import triple_classifier_model as tm
from tests.test_gpu_classify import _graph_reads, _pack, _query_reads

pytestmark = pytest.mark.gpu

CASES = [(21, 0, 41, 1), (31, 0, 63, 2), (22, 0, 32, 1)]  # (k, mode, k2, mode2): packed then polynomial, packed then FNV-1a


@pytest.fixture(scope="module")
def oracle():
    from oracle import pyoracle as po
    return po


def _pairs(genome, k2, rng):
    """pairs of query reads with copies of one another (other qualities, other mates) and empty second mates"""
    reads = _query_reads(genome, k2, rng)
    rng.shuffle(reads)
    half = len(reads) // 2
    firsts, seconds = reads[:half], reads[half:2 * half]
    for i in range(0, half, 7):  # a copy of an earlier first mate, its quality changed (another correction verdict, maybe)
        j = int(rng.integers(0, i + 1))
        codes, phred = firsts[j]
        q = phred.copy()
        if len(q):
            q[int(rng.integers(0, len(q)))] = int(rng.integers(1, 10)) if rng.integers(0, 2) else 35
        firsts[i] = (codes.copy(), q)
    for i in range(3, half, 11):
        seconds[i] = cm.EMPTY
    return list(zip(firsts, seconds))


@pytest.mark.parametrize("k,mode,k2,mode2", CASES)
def test_triple_classes_match_the_model(k, mode, k2, mode2, oracle):
    import metacherchant_amd as m
    genome, codes, off = _graph_reads(k2)
    tables = []
    for kk, mm in ((k, mode), (k2, mode2)):
        t = oracle.Table()
        t.count_reads(codes, off, kk, mm)
        tables.append(cm.table_getter(t, kk, mm))
    pairs = _pairs(genome, k2, np.random.default_rng(k * 100 + k2))
    sides = [_pack([p[s] for p in pairs]) for s in (0, 1)]
    last = [np.array(tm.last_copy([p[s][0] for p in pairs]), dtype=np.uint32) for s in (0, 1)]
    seen = set()
    for corr in (False, True):
        for z in (1.0, 1.96):
            for found, half in ((90, 40), (50, 0)):
                cls = []
                for pas, (kk, mm) in enumerate(((k, mode), (k2, mode2))):
                    with m.Context(kk, mm, 0, 0) as ctx:
                        ctx.add_reads_packed(oracle.pack(codes), off)
                        ctx.finalize()
                        covs = [ctx.classify_reads(sc, so, sb if corr else None, found=found, z=z, correction=corr) for sc, so, sb in sides]
                        if pas == 0:
                            got_last = [ctx.reads_last_copy(sc, so) for sc, so, _ in sides]
                            assert all(np.array_equal(g, w) for g, w in zip(got_last, last))
                            cls = ctx.triple_classes(covs[0], covs[1], sides[0][1], sides[1][1], half=half)
                        else:
                            cls = ctx.triple_classes(covs[0], covs[1], sides[0][1], sides[1][1], half=half, prev=cls, last=got_last)
                want = tm.classes(pairs, k, k2, tables[0], tables[1], found, half, z, corr)
                got = list(zip(cls[0].tolist(), cls[1].tolist()))
                bad = [i for i in range(len(want)) if got[i] != want[i]]
                assert not bad, (corr, z, found, half, bad[:5], [got[i] for i in bad[:5]], [want[i] for i in bad[:5]])
                seen.update(c for pr in want for c in pr)
    assert seen == {tm.NOT_FOUND, tm.HALF_FOUND, tm.FOUND}


def test_triple_classes_arguments(oracle):
    import metacherchant_amd as m
    cov = np.zeros(2, dtype=m.native.READ_COV_DTYPE)
    cov["found"] = [1, 0]
    cov["covered"] = [0, 10]
    cov["last"] = [0, 1]
    off = np.array([0, 0, 20], dtype=np.uint64)  # (both mates of pair 0 are empty)
    with m.Context(11, m.KEY_PACKED, 0, 0) as ctx:  # (no table: the classes need only the context's k)
        c1, c2 = ctx.triple_classes(cov, cov, off, off, half=40)
        # pair 0: mate 1 found; empty mate 2 -> found_2 = !found_1 = false, width 0 -> NOT; pair 1: width (10 + 10) / 20 = 1 -> HALF
        assert c1.tolist() == [2, 1] and c2.tolist() == [0, 1]
        p1, p2 = ctx.triple_classes(cov, cov, off, off, half=40, prev=(c1, c2), last=(np.array([0, 1], np.uint32),) * 2)
        assert p1.tolist() == [2, 1] and p2.tolist() == [0, 1]
        with pytest.raises(m.McError):
            ctx.triple_classes(cov, cov, off, off, half=101)
