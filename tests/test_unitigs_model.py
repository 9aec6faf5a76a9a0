"""The link analysis that mc_unitigs is defined by (include/mcgpu.h) leaves the nodes that the reference's loop leaves: pinned at
string level on hand-written shapes and on random sets (tests/unitigs_model.py; no GPU, no library)."""
import pytest

import unitigs_model as um

HAND = um.hand_cases()


@pytest.mark.parametrize("name", sorted(HAND))
def test_link_analysis_leaves_the_loops_nodes(name):
    k, kmers, cls = HAND[name]
    assert um.state(um.from_links(kmers, cls, k)) == um.state(um.reference_loop(kmers, cls, k))


@pytest.mark.parametrize("seed,k,n", [(1, 5, 150), (2, 5, 250), (2, 5, 100), (22, 4, 50), (4, 6, 600), (5, 21, 300)])
def test_link_analysis_leaves_the_loops_nodes_on_random_sets(seed, k, n):
    kmers, cls = um.random_set(seed, k, n)
    res = um.link_analysis(kmers, cls, k)
    assert um.state(um.from_links(kmers, cls, k, res)) == um.state(um.reference_loop(kmers, cls, k))
    if k <= 5:
        assert res["irregular"] and res["first"]  # (these sets hold both kinds of chain)


@pytest.mark.parametrize("seed,k", [(11, 4), (12, 5), (13, 21), (14, 32), (15, 33)])
def test_link_analysis_leaves_the_loops_nodes_on_mixed_sets(seed, k):
    kmers, cls = um.mixed_set(seed, k, (1, 2, 3) if k <= 5 else (1, 2, 3, 64, 65))
    res = um.link_analysis(kmers, cls, k)
    assert um.state(um.from_links(kmers, cls, k, res)) == um.state(um.reference_loop(kmers, cls, k))
    if k > 5:
        assert {64, 65} <= {len(s) - k + 1 for s in res["seqs"]}
        assert res["irregular"]


def test_a_chain_of_three_is_one_unitig_whatever_its_order():
    for name, (k, kmers, cls) in HAND.items():
        if not name.startswith("chain3_"):
            continue
        res = um.link_analysis(kmers, cls, k)
        assert len(res["seqs"]) == 1 and len(res["seqs"][0]) == k + 2 and res["irregular"] == [], name
        assert res["first"][0] < res["last_rc"][0]
        alive = [i for i, nd in enumerate(um.reference_loop(kmers, cls, k)) if not nd["deleted"]]
        assert alive == sorted([res["first"][0], res["last_rc"][0]]), name


def test_the_shapes_are_what_their_names_say():
    def res(name):
        k, kmers, cls = HAND[name]
        return um.link_analysis(kmers, cls, k), len(kmers)
    r, n = res("cycle")
    assert r["irregular"] == list(range(n)) and r["first"] == []
    r, n = res("poly_a")
    assert r["irregular"] == [0] and r["deg"] == [1, 1] and r["nbr"] == [1, 0]
    r, n = res("poly_a_beside_a_chain")
    assert r["irregular"] == [0] and len(r["first"]) == 1
    r, n = res("hairpin")
    assert r["irregular"] and r["first"] == []
    r, n = res("palindrome_k4")  # (both nodes of a palindrome spell it: whoever it follows has two neighbours, and it links to nobody)
    assert r["irregular"] == [] and r["deg"][3] == 2 and r["nbr"][sum(r["deg"][:3]):sum(r["deg"][:4])] == [4, 5]
    r, n = res("palindrome_k4_alone")
    assert r["irregular"] == [] and r["first"] == [] and r["deg"] == [0, 0]
    r, n = res("palindrome_k4_five_neighbours")
    assert max(r["deg"]) == 5
    r, n = res("class_change")
    assert sorted(len(s) for s in r["seqs"]) == [7, 7]
    r, n = res("branch")
    assert max(r["deg"]) >= 2 and len(r["first"]) >= 2 and r["irregular"] == []


def test_two_entries_of_one_kmer_are_refused():
    with pytest.raises(ValueError):
        um.link_analysis(["ACGTA", "TACGT"], [0, 0], 5)
