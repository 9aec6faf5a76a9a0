"""CPU: tests/walk_order_model.py's two walks against each other on the designed components of tests/walk_order_shapes.py.  The exact
replay is KmerEnvCalculator.runBfs as it is; the bounded walk is what mc_walk_order computes (tests/test_gpu_walk_order.py holds the
device to it).  Where the exact replay ends they agree; where it cannot end the bounded one still does."""
import numpy as np
import pytest

from tests import walk_order_model as wm
from tests import walk_order_shapes as ws


def _agree(members, cap=2_000_000):
    exact = wm.exact_replay(members, cap)
    order, twice, stats = wm.bounded_walk(members)
    assert stats["queue"] <= 2 * len(members)
    assert sorted(order) == sorted(set(order))
    if exact is not None:
        assert (order, twice) == exact[:2]
        assert stats["queue"] <= exact[2]
    return exact, (order, twice, stats)


def test_single_kmers():
    _, (order, twice, _) = _agree(["ACGGTCA"])
    assert order == [0] and twice == [False]
    _, (order, twice, _) = _agree(["AAAAAAA"])  # its own neighbour: pushed again while it is popped
    assert order == [0] and twice == [True]
    _agree(["ACGCGT"])  # its own reverse complement
    _agree(["TGACCGT"])  # the seed the other way round
    a, b = _agree(ws.members_of(["ACGGTCAT"], 7))[1], _agree(ws.members_of([wm.rc("ACGGTCAT")], 7))[1]
    assert a[0] == b[0] == [0, 1]


@pytest.mark.parametrize("n", [2, 63, 64, 65, 1025])
def test_chains(n):
    rng = np.random.default_rng(n)
    for seed_at in (0, n // 2, n - 1):
        exact, (order, twice, stats) = _agree(ws.chain(rng, 21, n, seed_at))
        assert exact is not None and len(order) == n and not any(twice)
        assert stats["levels"] == max(seed_at, n - 1 - seed_at) + 1


@pytest.mark.parametrize("n", [40, 41])
def test_cycles(n):
    exact, (order, twice, _) = _agree(ws.cycle(np.random.default_rng(n), 21, n))
    assert exact is not None and len(order) == n
    # the fronts meet on one k-mer, which both push, or on an edge, whose earlier end pushes the later one before that is popped
    assert sum(twice) == 1


def test_bubbles():
    rng = np.random.default_rng(5)
    exact, (order, twice, _) = _agree(ws.bubbles(rng, 21, 1))
    assert exact is not None and sum(twice) > 0  # what lies behind the bubble is popped once an arm
    assert _agree(ws.unequal_bubble_and_tip(rng, 21))[0] is not None
    members = ws.bubbles(rng, 21, 10)
    exact, (order, twice, stats) = _agree(members)
    assert exact is not None and exact[2] > 20 * len(members)  # 2^10 copies of the last stretch


def test_forty_bubbles_end_only_bounded():
    members = ws.bubbles(np.random.default_rng(40), 21, 40)
    assert wm.exact_replay(members, cap=10**6) is None
    order, twice, stats = wm.bounded_walk(members)
    assert len(order) == len(members) and stats["queue"] <= 2 * len(members)
    assert sum(twice) > len(members) // 2


@pytest.mark.parametrize("k", [3, 4])
def test_complete_graphs(k):
    members = ws.complete(k)
    exact, (order, _, _) = _agree(members)
    assert len(order) == len(members)


def test_disconnected_slice():
    rng = np.random.default_rng(9)
    members = ws.chain(rng, 21, 30) + ws.chain(rng, 21, 10)
    exact, (order, twice, _) = _agree(members)
    assert exact is not None and sorted(order) == list(range(30))
