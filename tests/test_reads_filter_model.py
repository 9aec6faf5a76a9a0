"""The read filter's model (tests/reads_filter_model.py) pinned on small cases spelled out as text: what
src/algo/ReadsFilter.java:47-68 does to them, quirks included.  No GPU."""
from tests import reads_filter_model as rf

K = 5
GENE = "ACGGTCATTGCAGG"  # its 5-mers are the set below
MEMBERS = rf.make_set(GENE[i:i + K] for i in range(len(GENE) - K + 1))


def test_the_set_is_canonical_and_takes_any_orientation():
    assert rf.normalize_dna("TTTTT") == "AAAAA" and rf.normalize_dna("ACGGT") == "ACCGT" and rf.normalize_dna("ACCGT") == "ACCGT"
    flipped = rf.make_set([rf.reverse_complement(GENE[i:i + K]) for i in range(len(GENE) - K + 1)] + [GENE[:K]] * 3)
    assert flipped == MEMBERS and len(MEMBERS) == 10


def test_short_reads_have_no_tested_window():
    assert rf.hits_and_keep(GENE[:K - 1], K, MEMBERS, 0) == (0, False)  # L < k
    assert rf.hits_and_keep(GENE[:K], K, MEMBERS, 0) == (0, False)  # L = k: its only window is the last one
    assert rf.hits_and_keep(GENE[:K + 1], K, MEMBERS, 0) == (1, True)  # L = k + 1: window 0 is tested, window 1 is not


def test_the_last_window_is_never_tested():
    read = "TTTTTTTT" + GENE[:K]  # the only member window is the last one
    assert rf.normalize_dna(read[-K:]) in MEMBERS
    assert rf.hits_and_keep(read, K, MEMBERS, 1) == (0, False)
    assert rf.hits_and_keep(read + "T", K, MEMBERS, 1) == (1, True)  # one base more and it is tested


def test_percentages():
    read = GENE + "TTTTTTTTTTTTTTTTTTTTTTTTTT"  # 40 bases: 36 windows, 35 tested, the first 10 are members
    assert len(read) == 40
    assert rf.hits_and_keep(read, K, MEMBERS, 0) == (10, True)  # max(1, 0)
    assert rf.hits_and_keep(read, K, MEMBERS, 1) == (10, True)  # 36 * 1 / 100 = 0 -> 1
    assert rf.hits_and_keep(read, K, MEMBERS, 27) == (10, True)  # 36 * 27 / 100 = 9
    assert rf.hits_and_keep(read, K, MEMBERS, 28) == (10, True)  # 10
    assert rf.hits_and_keep(read, K, MEMBERS, 50) == (10, False)  # 18
    assert rf.hits_and_keep(GENE + "T", K, MEMBERS, 50) == (10, True)  # 11 windows: 5
    assert rf.java_div(-7, 2) == -3 and rf.java_div(7, 2) == 3


def test_pct_100_keeps_nothing():
    # every window a member: L - k hits against a threshold of L - k + 1
    assert rf.hits_and_keep(GENE, K, MEMBERS, 100) == (len(GENE) - K, False)
    assert rf.hits_and_keep(GENE, K, MEMBERS, 99) == (9, True)  # 10 * 99 / 100 = 9
    assert rf.cut_reads_fasta([GENE, GENE + "A"], K, MEMBERS, 100, 0) == ""


def test_a_reverse_complement_hit():
    read = rf.reverse_complement(GENE)
    assert rf.hits_and_keep(read, K, MEMBERS, 1) == (len(GENE) - K, True)
    assert rf.hits_and_keep("TTTTTTTTTTT", K, MEMBERS, 0) == (0, False)


def test_n_is_printed_as_a_and_the_kept_reads_are_numbered():
    reads = ["ACGGTNATTG", "TTTTTTTTTT", "acggtcattg", "GGGGGGGGGG", "ACGG.CATTGC"]
    assert rf.read_text(reads[0]) == "ACGGTAATTG" and rf.read_text(reads[4]) == "ACGGACATTGC"
    # read 0: ACGGT is a member, GTAAT .. are not; read 4: no window without the A survives but CATTG (window 5 of 0 .. 5) is tested
    assert rf.cut_reads_fasta(reads, K, MEMBERS, 1, 3) == ">3|1\nACGGTAATTG\n>3|2\nACGGTCATTG\n>3|3\nACGGACATTGC\n"
    assert rf.cut_reads_fasta(reads[1:2], K, MEMBERS, 1, 0) == ""
