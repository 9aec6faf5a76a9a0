"""The window minima of the extract kernel's 16-position tile (csrc/count_pipeline.h sk_window_minima: sk_core_minima8,
sk_block_minima16) restated on numpy arrays, with the kernel's own blocks, cores and joins, against the minimum taken window by
window, on the CPU.

A lane holds 32 hashes hh: its own 16 and the next lane's.  Window j = min hh[j .. j + w - 1], j = 0 .. 15, w = 9 .. 17.

w >= 15, blocks of w hashes (block 0 = hh[0 .. w-1], block 1 = hh[w .. 2w-1]):
    s0[i] = min hh[i .. w-1]       p1[i] = min hh[w .. w+i]
    window 0 = s0[0];  window j < w: min(s0[j], p1[j-1]);  window w (w = 15) = p1[w-1]
w <= 14, the scheme of the 8-position tile on the windows B .. B+7, B = 0 and 8:
    core = min hh[B+7 .. B+w-1];  window B+7 = core;  window B+j = min(min hh[B+j .. B+6], core, min hh[B+w .. B+w+j-1])
The kernel takes for each w the one that compiles to fewer v_min instructions (the header gives the counts)."""
import numpy as np

WS = range(9, 18)


def core_minima8(hh, w, b, out):
    """sk_core_minima8<w, b>: fills out[b .. b+7]; returns the number of two-operand minima as written (those against the all-ones
    start value left out)"""
    n_min = 0
    core = hh[:, b + 7]
    for i in range(8, w):
        core = np.minimum(core, hh[:, b + i]); n_min += 1
    out[b + 7] = core
    suf = None
    for j in range(6, -1, -1):
        suf = hh[:, b + j] if suf is None else np.minimum(suf, hh[:, b + j])
        n_min += j != 6
        out[b + j] = np.minimum(suf, core); n_min += 1
    pre = None
    for j in range(1, 8):
        pre = hh[:, b + w + j - 1] if pre is None else np.minimum(pre, hh[:, b + w + j - 1])
        n_min += j != 1
        out[b + j] = np.minimum(out[b + j], pre); n_min += 1
    return n_min


def block_minima16(hh, w, out):
    """sk_block_minima16<w>, w >= 15"""
    assert 15 <= w <= 17
    n_min = 0
    a = min(w, 16)
    np1 = w if w == 15 else a - 1
    s0, p1 = [None] * w, [None] * w
    s0[w - 1] = hh[:, w - 1]
    for i in range(w - 2, -1, -1):
        s0[i] = np.minimum(s0[i + 1], hh[:, i]); n_min += 1
    p1[0] = hh[:, w]
    for i in range(1, np1):
        p1[i] = np.minimum(p1[i - 1], hh[:, w + i]); n_min += 1
    out[0] = s0[0]
    for j in range(1, a):
        out[j] = np.minimum(s0[j], p1[j - 1]); n_min += 1
    if w == 15:
        out[w] = p1[w - 1]
    return n_min


def kernel_minima(hh, w):
    """hh: (cases, 32) -> (cases, 16) as sk_window_minima<w, 16> forms them, and the number of two-operand minima it writes"""
    hh = np.asarray(hh)
    assert hh.shape[1] == 32
    out = [None] * 16
    n_min = block_minima16(hh, w, out) if w >= 15 else core_minima8(hh, w, 0, out) + core_minima8(hh, w, 8, out)
    assert all(o is not None for o in out)
    return np.stack(out, axis=1), n_min


def brute(hh, w):
    return np.stack([hh[:, j:j + w].min(axis=1) for j in range(16)], axis=1)


def test_random_hashes_at_every_w():
    hh = np.random.default_rng(41).integers(0, 1 << 32, (20000, 32), dtype=np.uint64).astype(np.uint32)
    for w in WS:
        got, _ = kernel_minima(hh, w)
        assert got.dtype == np.uint32 and np.array_equal(got, brute(hh, w)), w


def test_the_smallest_hash_at_every_place():
    """one hash far below the rest at each of the 32 places, and the two smallest side by side at each of the 31 pairs of places"""
    rng = np.random.default_rng(42)
    hh = rng.integers(1 << 20, 1 << 32, (32 + 31, 32), dtype=np.uint64).astype(np.uint32)
    for p in range(32):
        hh[p, p] = p + 1
    for p in range(31):
        hh[32 + p, p], hh[32 + p, p + 1] = 7, 5
    for w in WS:
        got, _ = kernel_minima(hh, w)
        want = brute(hh, w)
        assert np.array_equal(got, want), w
        for p in range(32):  # (the smallest one is what every window that holds its place gives)
            js = [j for j in range(16) if j <= p < j + w]
            assert (want[p, js] == p + 1).all() and (got[p, js] == p + 1).all()


def test_equal_neighbouring_hashes():
    """few distinct values: runs of equal hashes across the block edges, whole windows of one value, all 32 equal"""
    rng = np.random.default_rng(43)
    hh = rng.integers(0, 3, (5000, 32), dtype=np.uint64).astype(np.uint32) * np.uint32(0x40000000)
    hh[0, :] = 0xFFFFFFFE
    hh[1, :] = 0
    rep = np.repeat(rng.integers(0, 1 << 32, (2000, 8), dtype=np.uint64).astype(np.uint32), 4, axis=1)  # runs of four equal values
    both = np.concatenate([hh, rep])
    for w in WS:
        got, _ = kernel_minima(both, w)
        assert np.array_equal(got, brute(both, w)), w


def test_no_w_takes_more_minima_a_window_than_the_tile_of_8_positions():
    """as written, before the compiler joins some into three-operand ones: the 8-position scheme takes (w - 8) + 26 for 8 windows"""
    zeros = np.zeros((1, 32), dtype=np.uint32)
    n16 = [kernel_minima(zeros, w)[1] for w in WS]
    n8 = [(w - 8) + 26 for w in WS]
    assert all(a <= 2 * b for a, b in zip(n16, n8)), (n16, n8)
    assert n16 == [54, 56, 58, 60, 62, 64, 42, 44, 45]
