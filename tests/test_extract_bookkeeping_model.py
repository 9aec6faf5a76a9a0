"""The extract kernels' run bookkeeping as mask arithmetic (csrc/count_pipeline.h sk_break_bits, sk_start_bits) against the rule
stated window by window, on the CPU.

A lane owns N windows of its wave's tile.  `valid`: bit j <-> window j is a window of one read.  `ne`: bit j <-> the minimizer
hash of window j differs from that of window j - 1 (bit 0: from the previous lane's last).  `pv`: the previous lane's last window
is one (0 on lane 0).  `cur`: the tile window of the last break before the lane's first window.

The rule, window by window: window j breaks the run when it or the window before it is none, or their hashes differ; a window
starts a record when it is one and sits a multiple of MAXW windows behind the last break at or before it.

The masks:  brk = (~valid | ~((valid << 1) | pv) | ne) & mask
            low = (brk & -brk) - 1                          (the bits below the first break; all when there is none)
            start = valid & (brk | ((1 << ((cur - lane * N) mod MAXW)) & low))
The kernels fold pv into ne's bit 0 (a missing window's hash is SK_NONE, which no window has); here the two stay apart as the
rule has them."""
import numpy as np

MAXW = 16  # csrc/count_pipeline.h SK_MAX_WINDOWS (count_long.h: 32, with N = 8)


def rule_break(n, valid, ne, pv):
    """break bits of one lane, window by window"""
    bits, before = 0, pv
    for j in range(n):
        v = (valid >> j) & 1
        if not v or not before or (ne >> j) & 1:
            bits |= 1 << j
        before = v
    return bits


def rule_start(n, lane, valid, brk, cur, maxw=MAXW):
    """start bits of one lane, window by window: cur is carried along the windows"""
    bits = 0
    for j in range(n):
        pos = lane * n + j
        if (brk >> j) & 1:
            cur = pos
        if (valid >> j) & 1 and (pos - cur) % maxw == 0:
            bits |= 1 << j
    return bits


def mask_break(n, valid, ne, pv):
    m = (1 << n) - 1
    return (~valid | ~((valid << 1) | pv) | ne) & m


def mask_start(n, lane, valid, brk, cur, maxw=MAXW):
    low = (brk & -brk) - 1  # (-1 = all ones when brk == 0)
    deep = (1 << ((cur - lane * n) % maxw)) & low
    return valid & (brk | deep)


def mask_break_np(n, valid, ne, pv):
    return (~valid | ~((valid << 1) | pv) | ne) & ((1 << n) - 1)


def mask_start_np(n, lane, valid, brk, cur, maxw=MAXW):
    low = (brk & -brk) - 1
    deep = (np.int64(1) << ((cur - lane * n) % maxw)) & low
    return valid & (brk | deep)


def rule_np(n, lane, valid, ne, pv, cur, maxw=MAXW):
    """both rules over arrays of cases, a window at a time"""
    brk = np.zeros_like(valid)
    start = np.zeros_like(valid)
    before = pv.copy()
    cur = cur.copy()
    for j in range(n):
        v = (valid >> j) & 1
        b = (v == 0) | (before == 0) | (((ne >> j) & 1) == 1)
        brk |= b.astype(np.int64) << j
        before = v
        pos = lane * n + j
        cur = np.where(b, pos, cur)
        start |= ((v == 1) & ((pos - cur) % maxw == 0)).astype(np.int64) << j
    return brk, start


def test_the_array_form_of_the_rule_is_the_scalar_one():
    """(the exhaustive test below runs on arrays: 500 random cases of it against the plain loops)"""
    rng = np.random.default_rng(5)
    for n in (8, 16):
        lane = rng.integers(1, 62, 500)
        valid, ne = rng.integers(0, 1 << n, 500), rng.integers(0, 1 << n, 500)
        pv = rng.integers(0, 2, 500)
        cur = lane * n - 1 - rng.integers(0, 40, 500).clip(max=lane * n - 1)
        brk, start = rule_np(n, lane, valid, ne, pv, cur)
        for i in range(500):
            b = rule_break(n, int(valid[i]), int(ne[i]), int(pv[i]))
            assert b == brk[i] and rule_start(n, int(lane[i]), int(valid[i]), b, int(cur[i])) == start[i]
            assert mask_break(n, int(valid[i]), int(ne[i]), int(pv[i])) == b
            assert mask_start(n, int(lane[i]), int(valid[i]), b, int(cur[i])) == start[i]


def test_every_valid_and_ne_mask_at_8_windows_in_every_phase():
    """all 2^8 x 2^8 (valid, ne) pairs, both values of pv, all 16 phases of cur (and the 32 of the long records' cut)"""
    valid, ne = [a.reshape(-1).astype(np.int64) for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij")]
    lane = np.full_like(valid, 5)
    for maxw in (16, 32):
        for pv in (0, 1):
            pvs = np.full_like(valid, pv)
            for phase in range(maxw):
                cur = lane * 8 - 1 - phase  # the last break before my first window: 1 .. maxw windows back
                brk, start = rule_np(8, lane, valid, ne, pvs, cur, maxw)
                assert np.array_equal(mask_break_np(8, valid, ne, pvs), brk)
                assert np.array_equal(mask_start_np(8, lane, valid, brk, cur, maxw), start), (maxw, pv, phase)


def test_a_seeded_sample_at_16_windows():
    """10^5 cases at N = 16: any lane -- lane 0 among them, whose previous window is none (its break bit 0 is always set and its
    cur is whatever the kernel computes: any value here) --, cur any distance back; a tenth of the cases with no window valid, a tenth
    with no break inside the lane (all valid, no hash differs, the previous window one)"""
    rng = np.random.default_rng(20)
    n, cases = 16, 100000
    lane = rng.integers(0, 62, cases)
    valid, ne = rng.integers(0, 1 << n, cases), rng.integers(0, 1 << n, cases)
    pv = rng.integers(0, 2, cases)
    valid[:cases // 10] = 0
    valid[cases // 10:cases // 5] = (1 << n) - 1
    ne[cases // 10:cases // 5] = 0
    pv[cases // 10:cases // 5] = 1
    pv[lane == 0] = 0
    cur = np.where(lane == 0, rng.integers(0, 1000, cases), lane * n - 1 - rng.integers(0, 1000, cases) % np.maximum(lane * n, 1))
    brk, start = rule_np(n, lane, valid, ne, pv, cur)
    assert (lane == 0).sum() > 1000 and (brk == 0).sum() > 5000 and (valid == 0).sum() >= cases // 10
    assert (brk[lane == 0] & 1).all()
    assert np.array_equal(mask_break_np(n, valid, ne, pv), brk)
    got = mask_start_np(n, lane, valid, brk, cur)
    assert np.array_equal(got, start), np.nonzero(got != start)[0][:5]
    # the cuts themselves occur: windows that start a record without being a break
    assert ((start & ~brk) != 0).sum() > 1000
