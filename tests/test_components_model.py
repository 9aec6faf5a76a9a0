"""CPU: tests/components_model.py (the fmt-visualizer restated from the Java) on cases small enough to follow by hand, k = 5, packed
keys.  The expected files are written out; KC is the sum of the unitig's k-mer coverages plus (k - 1) times the last one's."""
from tests import components_model as cm

K = 5


def black(_):
    return "BLACK"


def run(reads, colour=black):
    return cm.phase(K, 0, cm.count_table(reads, K, 0), colour, reads)


def test_a_linear_read_is_one_component_with_every_coverage_its_count():
    files, comps = run(["ACTTCAGTAGC"])
    assert comps == [(0, 0, {"ACTTC": 1, "CTTCA": 1, "CTGAA": 1, "ACTGA": 1, "CAGTA": 1, "AGTAG": 1, "GCTAC": 1})]
    assert files == {  # 7 k-mers of coverage 1: KC = 7 + 4
        "comp0.gfa": "S\t5\tACTTCAGTAGC\tLN:i:11\tKC:i:11\tCL:Z:BLACK\n",
        "comp0_seqs.fasta": "> Id5 Length:11 Neighbors:[]\nACTTCAGTAGC\n"}


def test_a_bubble_queues_the_rejoining_kmer_twice_and_its_coverage_is_zero():
    reads = ["CAGTCATTGGA", "CAGTCGTTGGA"]  # CAGTC, then A or G, then TTGGA: two paths of five k-mers each
    graph = cm.count_table(reads, K, 0)
    e = cm.KmerEnv("CAGTC", K, 0, graph, black, "comp0")
    e.run_bfs()
    assert e.pops == 13 and len(e.members) == 12          # TTGGA is popped twice: ATTGG and GTTGG both queue it before its first pop
    assert e.members["TCCAA"] == 2                         # (TTGGA's canonical form) the table's count ...
    assert e.subgraph.get("TCCAA") == 0                    # ... and what the second put left
    assert sorted(v for _, v in e.subgraph.items()) == [0] + [1] * 10 + [2]
    assert not any(graph.values())                         # the walk zeroed its component
    files, comps = run(reads)
    assert len(comps) == 1 and comps[0][:2] == (0, 0) and comps[0][2] == e.members
    assert files == {
        "comp0.gfa": "S\t3\tCAGTC\tLN:i:5\tKC:i:10\tCL:Z:BLACK\n"       # count 2: 2 + 4 * 2
                     "S\t5\tAGTCGTTGG\tLN:i:9\tKC:i:9\tCL:Z:BLACK\n"   # five k-mers of count 1: 5 + 4
                     "S\t9\tAGTCATTGG\tLN:i:9\tKC:i:9\tCL:Z:BLACK\n"
                     "S\t15\tTCCAA\tLN:i:5\tKC:i:0\tCL:Z:BLACK\n"       # count 2, coverage 0
                     "L\t3\t+\t5\t+\t4M\nL\t3\t+\t9\t+\t4M\nL\t5\t-\t3\t-\t4M\nL\t9\t-\t3\t-\t4M\nL\t9\t+\t15\t-\t4M\n"
                     "L\t15\t+\t9\t-\t4M\nL\t15\t+\t5\t-\t4M\nL\t5\t+\t15\t-\t4M\n",
        "comp0_seqs.fasta": "> Id3 Length:5 Neighbors:[5, 9]\nCAGTC\n> Id5 Length:9 Neighbors:[3, 15]\nAGTCGTTGG\n"
                            "> Id9 Length:9 Neighbors:[3, 15]\nAGTCATTGG\n> Id15 Length:5 Neighbors:[5, 9]\nTCCAA\n"}


def test_poly_a_is_its_own_neighbour_and_gets_coverage_zero():
    reads = ["AAAAAAA"]
    graph = cm.count_table(reads, K, 0)
    e = cm.KmerEnv("AAAAA", K, 0, graph, black, "comp0")
    e.run_bfs()
    assert e.pops == 3 and e.members == {"AAAAA": 3}  # AAAAA queues itself as its left and as its right neighbour
    assert list(e.subgraph.items()) == [("AAAAA", 0)]
    files, comps = run(reads)
    assert comps == [(0, 0, {"AAAAA": 3})]
    # the node's only neighbour is the node itself: doMerge merges it with itself and deletes it, so both files are empty
    assert files == {"comp0.gfa": "", "comp0_seqs.fasta": ""}


def test_two_disjoint_reads_and_a_repeat_of_the_first_are_two_components():
    files, comps = run(["ACCGTAG", "TTGACATC", "ACCGTAG"])
    assert comps == [(0, 0, {"ACCGT": 2, "CCGTA": 2, "CGTAG": 2}), (1, 0, {"GTCAA": 1, "TGACA": 1, "ATGTC": 1, "ACATC": 1})]
    assert files == {  # (no comp2: the third read's k-mers are zero when the scan comes to them)
        "comp0.gfa": "S\t2\tACCGTAG\tLN:i:7\tKC:i:14\tCL:Z:BLACK\n", "comp0_seqs.fasta": "> Id2 Length:7 Neighbors:[]\nCTACGGT\n",
        "comp1.gfa": "S\t4\tGATGTCAA\tLN:i:8\tKC:i:8\tCL:Z:BLACK\n", "comp1_seqs.fasta": "> Id4 Length:8 Neighbors:[]\nTTGACATC\n"}


def test_the_two_table_and_the_four_table_colour_rules():
    assert [cm.two_table_colour(m) for m in range(4)] == ["BLACK", "GREEN", "BLUE", "GREY"]
    r = "ACTTCAGTAGC"
    inputs = {"donor": ([r], {"settle": ["ACTTCAG"], "not_settle": ["TTCAGTA"]}),  # ACTTC CTTCA | TTCAG in both | TCAGT CAGTA | none
              "before": ([r], {"stay": [], "gone": [r]}),
              "after": ([r + "A"], {"came_from_donor": ["ACTTCA", "GTAGCA"], "came_from_baseline": ["TTCAG"], "came_from_both": ["TCAGT"],
                                    "came_itself": ["CAGTAG", "GTAGCA"]})}
    files, comps = cm.fmt_visualizer(K, 0, inputs)
    assert [len(comps[p]) for p in ("donor", "before", "after")] == [1, 1, 1]
    assert sorted(files) == [p + "/comp0" + e for p in ("after", "before", "donor") for e in (".gfa", "_seqs.fasta")]
    assert files["donor/comp0.gfa"].decode() == (
        "S\t1\tCTGAA\tLN:i:5\tKC:i:5\tCL:Z:GREY\nS\t3\tAGTAGC\tLN:i:6\tKC:i:6\tCL:Z:BLACK\nS\t5\tACTTCA\tLN:i:6\tKC:i:6\tCL:Z:GREEN\n"
        "S\t12\tTACTGA\tLN:i:6\tKC:i:6\tCL:Z:BLUE\n"
        "L\t1\t-\t12\t-\t4M\nL\t1\t+\t5\t-\t4M\nL\t3\t-\t12\t+\t4M\nL\t5\t+\t1\t-\t4M\nL\t12\t-\t3\t+\t4M\nL\t12\t+\t1\t+\t4M\n")
    assert files["donor/comp0_seqs.fasta"].decode() == (
        "> Id1 Length:5 Neighbors:[5, 12]\nCTGAA\n> Id3 Length:6 Neighbors:[12]\nAGTAGC\n> Id5 Length:6 Neighbors:[1]\nACTTCA\n"
        "> Id12 Length:6 Neighbors:[1, 3]\nTACTGA\n")
    assert files["before/comp0.gfa"].decode() == "S\t5\tACTTCAGTAGC\tLN:i:11\tKC:i:11\tCL:Z:BLUE\n"
    assert files["after/comp0.gfa"].decode() == (
        "S\t1\tCTGAA\tLN:i:5\tKC:i:5\tCL:Z:BLUE\nS\t5\tACTTCA\tLN:i:6\tKC:i:6\tCL:Z:RED\nS\t8\tGTAGCA\tLN:i:6\tKC:i:6\tCL:Z:GREY\n"
        "S\t4\tCAGTAG\tLN:i:6\tKC:i:6\tCL:Z:YELLOW\nS\t15\tACTGA\tLN:i:5\tKC:i:5\tCL:Z:GREEN\n"
        "L\t1\t-\t15\t-\t4M\nL\t1\t+\t5\t-\t4M\nL\t4\t+\t8\t+\t4M\nL\t8\t-\t4\t-\t4M\nL\t5\t+\t1\t-\t4M\nL\t4\t-\t15\t+\t4M\n"
        "L\t15\t-\t4\t+\t4M\nL\t15\t+\t1\t+\t4M\n")


def test_two_kmers_with_one_key_trip_the_assertion():
    import pytest
    r = "ACTTCAGTAGCTTGACCATGCAATCGGATCAGCTAGCTAAGCTTCCGATAGGCTAACGT"
    a, b = r[:41], r[1:42]
    e = cm.KmerEnv(a, 41, 1, {}, black, "c", keys={a: 7, b: 7})  # (the cache says that both hash to 7)
    assert e._key(a) == 7 and e._key(cm.reverse_complement(a)) != 7
    with pytest.raises(AssertionError):
        e._key(b)
    assert cm.KmerEnv(a, 5, 0, {}, black, "c", keys={"ACTTC": 7, "CTTCA": 7})._key("CTTCA") == 7  # packed keys: nothing to assert


def test_hash_modes_assert_that_no_two_kmers_share_a_key():
    reads = ["ACTTCAGTAGCTTGACCATGCAATCGGATCAGCTAGCTAAGCTTCCGATAGGCTAACGT"]
    for mode in (1, 2):
        files, comps = cm.phase(41, mode, cm.count_table(reads, 41, mode), black, reads)
        assert len(comps) == 1 and len(comps[0][2]) == len(reads[0]) - 40 and len(files) == 2
