"""The recipient-visualiser's model (tests/recipient_model.py) on cases small enough to follow by hand, with the expected files written
out, and the C++ host side (Environment with colours, driven from a dump file as tests/test_host_cpp.py drives it) against the model
on randomised graphs.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import recipient_model as rm


def table(k, reads, mode=0):
    """a dict table: every k-window of the reads, counted under the tool's key"""
    t = {}
    for r in reads:
        for i in range(len(r) - k + 1):
            key = rm.kmer_key(r[i:i + k], k, mode)
            t[key] = t.get(key, 0) + 1
    return t


def run(k, graph_reads, class_reads, seqs, **kw):
    return rm.recipient_visualiser(k, 0, table(k, graph_reads), [table(k, c) for c in class_reads], seqs, **kw)


def test_all_six_colours_and_merges_that_stop_at_a_colour_change():
    """One path ACGGTCATTGCAGGATC (its end GGATC is its own reverse complement's neighbour: the walk turns round there).  donor holds
    ACGGT, CGGTC; baseline GGTCA, GTCAT, CGGTC; both TCATT, CATTG; itself CATTG, ATTGC.  So ACGGT is RED, CGGTC GREY (donor and
    baseline), GGTCA + GTCAT BLUE and merged into one node of 6 bases, TCATT GREEN, CATTG GREY (both and itself), ATTGC YELLOW, the
    rest BLACK: neighbours of different colours stay apart although each has one neighbour."""
    files, log, envs = run(5, ['ACGGTCATTGCAGGATC'], [['ACGGTC'], ['GGTCAT', 'CGGTC'], ['TCATTG'], ['CATTGC']], ['ACGGTCATTGCAGGATC'])
    assert log == ['Extending endings by 0 kmers', 'Finished processing all sequences!']
    assert sorted(files) == ['after/comp_0.gfa', 'after/comp_0_seqs.fasta']
    assert files['after/comp_0.gfa'] == (
        'S\t3_start\tCGGTC\tLN:i:5\tKC:i:5\tCL:Z:GREY\n'
        'S\t6_start\tTGCAGGATCCTGCA\tLN:i:14\tKC:i:14\tCL:Z:BLACK\n'
        'S\t7_start\tATTGC\tLN:i:5\tKC:i:5\tCL:Z:YELLOW\n'
        'S\t11_start\tATGACC\tLN:i:6\tKC:i:6\tCL:Z:BLUE\n'
        'S\t13_start\tTGCAA\tLN:i:5\tKC:i:5\tCL:Z:BLACK\n'
        'S\t17_start\tCAATG\tLN:i:5\tKC:i:5\tCL:Z:GREY\n'
        'S\t19_start\tAATGA\tLN:i:5\tKC:i:5\tCL:Z:GREEN\n'
        'S\t23_start\tACCGT\tLN:i:5\tKC:i:5\tCL:Z:RED\n'
        'L\t3_start\t-\t23_start\t+\t4M\n'
        'L\t3_start\t+\t11_start\t-\t4M\n'
        'L\t6_start\t+\t6_start\t+\t4M\n'
        'L\t6_start\t+\t13_start\t+\t4M\n'
        'L\t7_start\t-\t17_start\t+\t4M\n'
        'L\t7_start\t+\t13_start\t-\t4M\n'
        'L\t11_start\t-\t19_start\t-\t4M\n'
        'L\t13_start\t-\t6_start\t+\t4M\n'
        'L\t13_start\t-\t13_start\t+\t4M\n'
        'L\t13_start\t+\t7_start\t-\t4M\n'
        'L\t11_start\t+\t3_start\t-\t4M\n'
        'L\t17_start\t-\t7_start\t+\t4M\n'
        'L\t17_start\t+\t19_start\t+\t4M\n'
        'L\t19_start\t-\t17_start\t-\t4M\n'
        'L\t19_start\t+\t11_start\t+\t4M\n'
        'L\t23_start\t-\t3_start\t+\t4M\n'
    )
    assert files['after/comp_0_seqs.fasta'] == (
        '> Id3_start Length:5 Neighbors:[11, 23]\n'
        'CGGTC\n'
        '> Id7_start Length:5 Neighbors:[13, 17]\n'
        'ATTGC\n'
        '> Id11_start Length:6 Neighbors:[3, 19]\n'
        'ATGACC\n'
        '> Id13_start Length:5 Neighbors:[6, 7]\n'
        'TGCAA\n'
        '> Id17_start Length:5 Neighbors:[7, 19]\n'
        'CAATG\n'
        '> Id19_start Length:5 Neighbors:[11, 17]\n'
        'AATGA\n'
        '> Id23_start Length:5 Neighbors:[3]\n'
        'ACCGT\n'
    )
    assert {l.split('CL:Z:')[1].strip() for l in files['after/comp_0.gfa'].splitlines() if l[0] == 'S'} == {'RED', 'GREEN', 'BLUE', 'GREY', 'YELLOW', 'BLACK'}

def test_a_merge_stops_at_the_gene_boundary():
    """The gene ACGGTCAT lies inside the read TTACGGTCATTGCA: its four k-mers merge into one _start node, the flanks into their own."""
    files, log, envs = run(5, ['TTACGGTCATTGCA'], [[], [], [], []], ['ACGGTCAT'])
    assert log == ['Extending endings by 0 kmers', 'Finished processing all sequences!']
    assert sorted(files) == ['after/comp_0.gfa', 'after/comp_0_seqs.fasta']
    assert files['after/comp_0.gfa'] == (
        'S\t2\tCCGTAA\tLN:i:6\tKC:i:6\tCL:Z:BLACK\n'
        'S\t4\tTCATTGCAA\tLN:i:9\tKC:i:9\tCL:Z:BLACK\n'
        'S\t18_start\tACGGTCAT\tLN:i:8\tKC:i:8\tCL:Z:BLACK\n'
        'L\t2\t-\t18_start\t+\t4M\n'
        'L\t4\t-\t18_start\t-\t4M\n'
        'L\t18_start\t-\t2\t+\t4M\n'
        'L\t18_start\t+\t4\t+\t4M\n'
    )
    assert files['after/comp_0_seqs.fasta'] == (
        '> Id2 Length:6 Neighbors:[18]\n'
        'TTACGG\n'
        '> Id18_start Length:8 Neighbors:[2, 4]\n'
        'ACGGTCAT\n'
    )

def test_kc_of_a_unitig_of_three_kmers():
    """ACGGT x2, CGGTC x3, GGTCA x2: KC = 2 + 3 + 2 + (k - 1) x the last k-mer's 2 = 15"""
    files, log, envs = run(5, ['ACGGTCA', 'ACGGTCA', 'CGGTC'], [[], [], [], []], ['ACGGTCA'])
    assert log == ['Extending endings by 0 kmers', 'Finished processing all sequences!']
    assert sorted(files) == ['after/comp_0.gfa', 'after/comp_0_seqs.fasta']
    assert files['after/comp_0.gfa'] == (
        'S\t4_start\tACGGTCA\tLN:i:7\tKC:i:15\tCL:Z:BLACK\n'
    )
    assert files['after/comp_0_seqs.fasta'] == (
        '> Id4_start Length:7 Neighbors:[]\n'
        'TGACCGT\n'
    )

def test_a_palindromic_kmer():
    """ACGT is its own reverse complement: both of its nodes print (the reference's <= on equal labels), each edge twice"""
    files, log, envs = run(4, ['TTACGTCC'], [[], [], [], []], ['ACGT'])
    assert log == ['Extending endings by 0 kmers', 'Finished processing all sequences!']
    assert sorted(files) == ['after/comp_0.gfa', 'after/comp_0_seqs.fasta']
    assert files['after/comp_0.gfa'] == (
        'S\t1_start\tACGT\tLN:i:4\tKC:i:4\tCL:Z:BLACK\n'
        'S\t1_start\tACGT\tLN:i:4\tKC:i:4\tCL:Z:BLACK\n'
        'S\t3\tCGTCC\tLN:i:5\tKC:i:5\tCL:Z:BLACK\n'
        'S\t6\tCGTAA\tLN:i:5\tKC:i:5\tCL:Z:BLACK\n'
        'L\t1_start\t+\t3\t+\t3M\n'
        'L\t1_start\t+\t6\t+\t3M\n'
        'L\t1_start\t+\t3\t+\t3M\n'
        'L\t1_start\t+\t6\t+\t3M\n'
        'L\t3\t-\t1_start\t+\t3M\n'
        'L\t3\t-\t1_start\t+\t3M\n'
        'L\t6\t-\t1_start\t+\t3M\n'
        'L\t6\t-\t1_start\t+\t3M\n'
    )
    assert files['after/comp_0_seqs.fasta'] == (
        '> Id1_start Length:4 Neighbors:[3, 6]\n'
        'ACGT\n'
        '> Id3 Length:5 Neighbors:[1]\n'
        'GGACG\n'
        '> Id6 Length:5 Neighbors:[1]\n'
        'TTACG\n'
    )

def test_a_repeated_window_is_queued_twice_and_inserted_once():
    """ACGGT and CGGTA come twice in the sequence: five k-mers in the subgraph, counted 2, 2, 1, 1, 1 (KC 7 + 4 x 1 = 11)"""
    files, log, envs = run(5, ['ACGGTACGGTA'], [[], [], [], []], ['ACGGTACGGTA'])
    assert log == ['Extending endings by 0 kmers', 'Finished processing all sequences!']
    assert sorted(files) == ['after/comp_0.gfa', 'after/comp_0_seqs.fasta']
    assert files['after/comp_0.gfa'] == (
        'S\t4_start\tGTACCGTAC\tLN:i:9\tKC:i:11\tCL:Z:BLACK\n'
        'L\t4_start\t+\t4_start\t-\t4M\n'
        'L\t4_start\t+\t4_start\t+\t4M\n'
        'L\t4_start\t-\t4_start\t-\t4M\n'
        'L\t4_start\t-\t4_start\t+\t4M\n'
    )
    assert files['after/comp_0_seqs.fasta'] == (
        '> Id4_start Length:9 Neighbors:[]\n'
        'GTACGGTAC\n'
    )

def test_maxradius_1():
    """the seed and its two neighbours; both ends could go on, by exactly one k-mer each: 2 endings"""
    files, log, envs = run(5, ['TTACGGTCATTGCA'], [[], [], [], []], ['CGGTC'], max_radius=1)
    assert log == ['Extending endings by 2 kmers', 'Finished processing all sequences!']
    assert sorted(files) == ['after/comp_0.gfa', 'after/comp_0_seqs.fasta']
    assert files['after/comp_0.gfa'] == (
        'S\t1_start\tCGGTC\tLN:i:5\tKC:i:5\tCL:Z:BLACK\n'
        'S\t3\tGGTCA\tLN:i:5\tKC:i:5\tCL:Z:BLACK\n'
        'S\t5\tACCGT\tLN:i:5\tKC:i:5\tCL:Z:BLACK\n'
        'L\t1_start\t-\t5\t+\t4M\n'
        'L\t1_start\t+\t3\t+\t4M\n'
        'L\t3\t-\t1_start\t-\t4M\n'
        'L\t5\t-\t1_start\t+\t4M\n'
    )
    assert files['after/comp_0_seqs.fasta'] == (
        '> Id1_start Length:5 Neighbors:[3, 5]\n'
        'CGGTC\n'
        '> Id3 Length:5 Neighbors:[1]\n'
        'GGTCA\n'
        '> Id5 Length:5 Neighbors:[1]\n'
        'ACCGT\n'
    )
    assert not envs[0].cut_a_level

def test_maxkmers_cuts_a_level():
    """4 k-mers: the seed, ACGGT and GGTCA at distance 1, then TACGG at distance 2 -- and GTCAT, also at distance 2, is refused"""
    files, log, envs = run(5, ['TTACGGTCATTGCA'], [[], [], [], []], ['CGGTC'], max_kmers=4)
    assert log == ['Extending endings by 2 kmers', 'Finished processing all sequences!']
    assert sorted(files) == ['after/comp_0.gfa', 'after/comp_0_seqs.fasta']
    assert files['after/comp_0.gfa'] == (
        'S\t1_start\tCGGTC\tLN:i:5\tKC:i:5\tCL:Z:BLACK\n'
        'S\t3\tGGTCA\tLN:i:5\tKC:i:5\tCL:Z:BLACK\n'
        'S\t6\tACCGTA\tLN:i:6\tKC:i:6\tCL:Z:BLACK\n'
        'L\t1_start\t-\t6\t+\t4M\n'
        'L\t1_start\t+\t3\t+\t4M\n'
        'L\t3\t-\t1_start\t-\t4M\n'
        'L\t6\t-\t1_start\t+\t4M\n'
    )
    assert files['after/comp_0_seqs.fasta'] == (
        '> Id1_start Length:5 Neighbors:[3, 6]\n'
        'CGGTC\n'
        '> Id3 Length:5 Neighbors:[1]\n'
        'GGTCA\n'
        '> Id6 Length:6 Neighbors:[1]\n'
        'TACGGT\n'
    )
    assert envs[0].cut_a_level

def test_a_sequence_without_a_kmer_in_the_graph_writes_nothing():
    """sequence 0 has no k-mer in the graph, sequence 1 is shorter than k, sequence 2 is found: only comp_2 is written"""
    files, log, envs = run(5, ['TTACGGTCATTGCA'], [[], [], [], []], ['GGGGGGGG', 'ACG', 'CGGTC'], max_radius=0)
    assert log == ['Could not find any k-mers of the target gene in the input, halting.', 'Could not find any k-mers of the target gene in the input, halting.', 'Extending endings by 0 kmers', 'Finished processing all sequences!']
    assert sorted(files) == ['after/comp_2.gfa', 'after/comp_2_seqs.fasta']
    assert files['after/comp_2.gfa'] == (
        'S\t1_start\tCGGTC\tLN:i:5\tKC:i:5\tCL:Z:BLACK\n'
    )
    assert files['after/comp_2_seqs.fasta'] == (
        '> Id1_start Length:5 Neighbors:[]\n'
        'CGGTC\n'
    )


def test_colour_of_mask():
    """RecipientVisualiser.java:157-169"""
    want = {0: "BLACK", 1: "RED", 2: "BLUE", 4: "GREEN", 8: "YELLOW"}
    for m in range(16):
        assert rm.colour_of_mask(m) == want.get(m, "GREY")


@pytest.fixture(scope="module")
def hosttest():
    if os.environ.get("MC_HOSTTEST"):
        return os.environ["MC_HOSTTEST"]
    from metacherchant_amd import build
    build.build_host()
    return build.HOSTTEST


@pytest.mark.parametrize("k,seed", [(5, 1), (7, 2), (11, 3), (21, 4), (31, 5), (41, 6), (63, 7)])
def test_the_cpp_environment_with_colours_equals_the_model(hosttest, tmp_path, k, seed):
    """Random genomes with repeats and branches (a mutated copy), four random class tables, --maxkmers and --maxradius biting: the C++
    Environment, given the model's walk and masks through a dump file, writes the model's files byte for byte and counts its endings."""
    rng = np.random.default_rng(seed)
    mode = 0 if k <= 31 else 1
    genome = rng.integers(0, 4, 600).astype(np.uint8)
    variant = genome.copy()
    for p in rng.integers(50, 550, 10):
        variant[p] = (variant[p] + 1) & 3
    reads = []
    for src in (genome, variant, genome):
        for _ in range(60):
            s = int(rng.integers(0, 600 - 80))
            r = src[s:s + 80]
            reads.append(po.decode(r if rng.integers(0, 2) else (3 - r[::-1]).astype(np.uint8)))
    graph = table(k, reads, mode)
    classes = [table(k, [reads[i] for i in rng.choice(len(reads), 8, replace=False)], mode) for _ in range(4)]
    seqs = [po.decode(genome[100:100 + 2 * k]), po.decode(variant[300:300 + k + 3]), po.decode(rng.integers(0, 4, 50).astype(np.uint8))]
    colours = set()
    for mk, mr in ((None, 1000), (40, 1000), (None, 6), (25, 3)):
        files, log, envs = rm.recipient_visualiser(k, mode, graph, classes, seqs, max_kmers=mk, max_radius=mr)
        assert files and (k < 11 or len(files) == 4)  # (from k = 11 on the random sequence is not in the graph)
        for i, e in enumerate(envs):
            if e.nodes is None:
                continue
            colours |= {n.color for n in e.nodes}
            d = e.distance
            kmers = list(d.keys())
            outside = set()
            for s in e.subgraph.keys():
                for nb in rm.all_neighbors(s):
                    if rm.count_in(graph, rm.kmer_key(nb, k, mode)) > 0:
                        outside.add(nb)
            # (the walk goes to the C++ side in the map's iteration order: add_pass builds its own map from it, in insertion
            # order -- so hand it the order in which the k-mers were inserted)
            dump = tmp_path / ("dump_%d_%s_%s_%d" % (k, mk, mr, i))
            with open(dump, "w") as f:
                f.write("%d\n%s\n%d\n" % (k, e.sequence, len(e.inserted)))
                for s in e.inserted:
                    f.write("%s %d %d %d\n" % (s, d.get(s), e._cov(s), rm.mask_of(s, k, mode, classes)))
                f.write("%d\n%s\n" % (len(outside), "\n".join(sorted(outside))))
            out = tmp_path / ("out_%d_%s_%s" % (k, mk, mr))
            got_log = subprocess.check_output([hosttest, "colour", str(dump), str(out), "comp_%d" % i], text=True)
            assert got_log.splitlines() == ["Extending endings by %d kmers" % e.n_extensions]
            assert len(kmers) == len(e.inserted)
            for suffix in ("_seqs.fasta", ".gfa"):
                with open(os.path.join(out, "comp_%d%s" % (i, suffix))) as f:
                    assert f.read() == files["after/comp_%d%s" % (i, suffix)], (mk, mr, i, suffix)
    assert k < 11 or len(colours) >= 5, colours  # (the inputs: at k = 5 and 7 nearly every k-mer is in several classes)
