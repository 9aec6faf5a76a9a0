"""tests/read_pointers.py against the C code (no GPU): its restatements of ptr_encode, ptr_decode, ptr_advance and ptr_advance_long
equal what `mc_hosttest pointers` prints from csrc/read_ptr.h, at every position within 80 of the four tier boundaries, at the
store's first position, at the last exact positions, at a few thousand random positions of every tier and past the end of the
range.  Then the model's own properties: the range of the code of window j of a record holds that window's position, for the 16
windows of a super-k-mer record and the 32 of a long record, in every tier and across every boundary."""
import subprocess

import numpy as np
import pytest

from tests import read_pointers as rp

BOUNDARIES = [rp.EXACT_END, rp.T2_POS, rp.T3_POS, rp.END]


def positions():
    rng = np.random.default_rng(31)
    p = [np.arange(b - 80, b + 81) for b in BOUNDARIES]
    p += [np.array([0, 1, 15, 16, 31, 32]), np.arange(rp.EXACT_END - 17, rp.EXACT_END + 1)]
    p += [rng.integers(lo, end, 3000) for lo, end, _, _ in rp.TIERS]
    p += [rp.END + rng.integers(0, 1 << 40, 200), np.array([150 * 10 ** 9, (1 << 63) - 1])]  # past the end (150 G: the ninth of ten ranks' place at 1 G reads)
    return np.unique(np.concatenate(p).astype(np.int64))


@pytest.fixture(scope="module")
def hosttest():
    from metacherchant_amd import build
    build.build_host()
    return build.HOSTTEST


def pointers(hosttest, pos):
    rows = []
    for i in range(0, len(pos), 2000):  # (positions are arguments: a few thousand a call)
        out = subprocess.run([hosttest, "pointers"] + [str(int(x)) for x in pos[i:i + 2000]], check=True, capture_output=True, text=True).stdout
        rows += [[int(x) for x in line.split()] for line in out.splitlines()]
    a = np.array(rows, dtype=np.int64)
    assert a.shape == (len(pos), 3 + 16 + 32)
    return a


def test_the_restatements_give_what_the_header_gives(hosttest):
    pos = positions()
    assert len(pos) > 12000
    got = pointers(hosttest, pos)
    code = rp.ptr_encode(pos)
    assert np.array_equal(got[:, 0], code)
    some = code != 0
    assert some.sum() > 12000 and (~some).sum() > 200
    lo, span = rp.ptr_range(code[some])
    assert np.array_equal(got[some, 1], lo) and np.array_equal(got[some, 2], span)
    assert not got[~some, 1:3].any()
    for j in range(16):
        assert np.array_equal(got[:, 3 + j], rp.ptr_advance(code, j)), j
    for j in range(32):
        assert np.array_equal(got[:, 19 + j], rp.ptr_advance_long(code, j)), j


def test_the_tiers():
    """the constants as the header's comment states them; every tier's codes follow the codes of the tier before"""
    assert [t[0] for t in rp.TIERS] == [0, 1 << 31, 6442450944, 15032385536] and rp.END == 49392123776
    assert [t[3] for t in rp.TIERS] == [1, 20, 32, 96]
    for (lo, end, lg, span), first in zip(rp.TIERS, [1, (1 << 31) + 1, (1 << 31) + (1 << 30) + 1, (1 << 31) + 3 * (1 << 29) + 1]):
        assert (end - lo) % (1 << lg) == 0
        assert int(rp.ptr_encode(lo)[0]) == first and int(rp.ptr_encode(end - 1)[0]) == first + ((end - lo) >> lg) - 1
        assert [int(x[0]) for x in rp.ptr_range(first)] == [lo, span]
    assert int(rp.ptr_encode(rp.END - 1)[0]) == (1 << 32) - 2  # (32 bits hold every code, 0 and 2^32 - 1 apart)


def test_a_code_holds_its_position_and_past_the_end_there_is_none():
    pos = positions()
    code = rp.ptr_encode(pos)
    assert np.array_equal(code != 0, pos < rp.END)
    inside = pos < rp.END
    lo, span = rp.ptr_range(code[inside])
    assert rp.holds(code[inside], pos[inside]).all()
    assert (span[pos[inside] < rp.EXACT_END] == 1).all() and (lo < rp.END).all()
    # the granule is the smallest range: the position before lo and the one at lo + granule have other codes
    for t_lo, t_end, lg, _ in rp.TIERS:
        m = (pos[inside] >= t_lo) & (pos[inside] < t_end)
        assert m.sum() > 3000
        assert ((pos[inside][m] - lo[m]) < (1 << lg)).all() and (lo[m] % (1 << lg) == t_lo % (1 << lg)).all()


@pytest.mark.parametrize("name,n", [("ptr_advance", 16), ("ptr_advance_long", 32)])
def test_the_code_of_window_j_holds_position_p_plus_j(name, n):
    """for every position p of the range and every window j of a record whose first window sits at p: a code unless p + j lies
    past the end, and its range holds p + j; exact positions stay exact.  The 64-base tier is where ptr_advance_long needs the
    reader's 96 offsets: it names the granule of the record's first window, which starts up to 63 + 31 bases before window 31."""
    advance = getattr(rp, name)
    pos = positions()
    pos = pos[pos < rp.END]
    code = rp.ptr_encode(pos)
    worst = 0
    for j in range(n):
        got = advance(code, j)
        there = pos + j < rp.END
        assert (got[there] != 0).all(), j
        assert (advance(0, j) == 0).all()
        some = got != 0
        assert rp.holds(got[some], pos[some] + j).all(), (j, pos[some][~rp.holds(got[some], pos[some] + j)][:5])
        exact = pos + j < rp.EXACT_END
        assert np.array_equal(got[exact], pos[exact] + j + 1), j
        worst = max(worst, int((pos[some] + j - rp.ptr_range(got[some])[0]).max()))
    assert worst == (63 + 15 if n == 16 else 63 + 31)  # (the positions hold a granule's last base: the bound is reached)
