"""The packed path of environment-finder-multi on the CPU: `mc_hosttest multi-packed` (environment_finder_multi_packed with env_join_host and
unitigs_by_links; csrc/host/multi.cpp, picture.cpp) must write what `mc_hosttest multi` (the string function) and oracle/host_oracle.py write, byte
for byte, and tests/env_join_model.py -- mc_env_join's definitions on dicts of strings -- must give the oracle's Jaccard tables and the
KC and colour of every S line.  Designed graph files: env_join_model.designed_case says what is in them."""
import os
import subprocess

import numpy as np
import pytest

from metacherchant_amd import build
from oracle import host_oracle as ho
from tests import env_join_model as M

FILES = ["seqs.fasta", "graph.gfa", "gene.fasta", "Jacard_sym.txt", "Jacard_alt.txt"]
KS = [5, 21, 31, 32, 33, 63]
GS = [1, 2, 3, 4, 9]


@pytest.fixture(scope="module")
def hosttest():
    build.build_host()
    return build.HOSTTEST


def write_inputs(tmp_path, files, gene):
    envs = []
    for g, lines in enumerate(files):
        p = tmp_path / ("env%d.txt" % g)
        p.write_text(M.graph_text(lines))
        envs.append(str(p))
    seq = tmp_path / "seq.fasta"
    seq.write_text(">the gene\n%s\n" % gene)
    return envs, str(seq)


def run_tool(hosttest, sub, out_dir, seq, envs, check=True):
    r = subprocess.run([hosttest, sub, str(out_dir), seq, "1"] + envs, capture_output=True, text=True)
    if check:
        assert r.returncode == 0, r.stderr
    return r


def read_files(out_dir):
    return {f: open(os.path.join(str(out_dir), f)).read() for f in FILES}


def three_ways(hosttest, tmp_path, files, gene):
    """the five files of the string function, checked equal to the packed path's and the oracle's; and the packed path's output"""
    envs, seq = write_inputs(tmp_path, files, gene)
    want, log = ho.environment_finder_multi(envs, seq, None, 1)
    a = run_tool(hosttest, "multi", tmp_path / "string", seq, envs)
    b = run_tool(hosttest, "multi-packed", tmp_path / "packed", seq, envs)
    got_a, got_b = read_files(tmp_path / "string"), read_files(tmp_path / "packed")
    for f in FILES:
        assert got_a[f] == want[f], f
        assert got_b[f] == want[f], f
    assert a.stdout.splitlines() == log
    assert b.stdout.splitlines()[:-1] == log
    return want, envs, b.stdout.splitlines()[-1]


def jaccard_tables(j, envs):
    """Jacard_sym.txt and Jacard_alt.txt from the model's matrices: printProbability's int and float conversions"""
    G = len(envs)
    i32 = lambda v: v - (1 << 32) if v >> 31 else v
    sym = ["The[31mWarning! symmetric <<Jaccard distance>> (1 - AB/AUB):\n", "\n"]
    alt = ["The[31mWarning! alternative <<Jaccard distance>> (1 - AB/A):\n", "\n"]
    for a in range(G):
        sym.append(envs[a])
        alt.append(envs[a])
        for b in range(G):
            diff, diff_alt, uni = j["diff"][a][b], j["diff_alt"][a][b], j["uni"][a][b]
            inter, u, ua = i32((uni - diff) & M.M32), i32(uni), i32((uni - diff_alt) & M.M32)
            with np.errstate(divide="ignore", invalid="ignore"):
                sym.append(ho.java_format_6_2f(np.float32(1) - np.float32(inter) / np.float32(u)) + " ")
                alt.append(ho.java_format_6_2f(np.float32(1) - np.float32(inter) / np.float32(ua)) + " ")
        sym.append("\n")
        alt.append("\n")
    return "".join(sym), "".join(alt)


def colour(is_gene, n_member, G):
    if is_gene:
        return "#00ff00"
    if G == 2:
        return {1: "#ff0000", 2: "#0000ff"}.get(n_member, "#000000")
    if G == 3:
        return {1: "#ff0000", 2: "#0000ff", 3: "#ff00ff", 4: "#ffff00", 5: "#ffaa00", 6: "#00ffff"}.get(n_member, "#000000")
    v = 256 * n_member // G
    return "#%02X%02X%02X" % (v, v, v)


def check_model(want, envs, files, gene, k):
    graphs = [M.graph_dict(lines) for lines in files]
    entries = M.entries_of(graphs)
    j = M.join(entries, graphs, gene)
    sym, alt = jaccard_tables(j, envs)
    assert sym == want["Jacard_sym.txt"]
    assert alt == want["Jacard_alt.txt"]
    at = {e: i for i, e in enumerate(entries)}
    n_s = 0
    for line in want["graph.gfa"].splitlines():
        t = line.split("\t")
        if t[0] != "S":
            continue
        n_s += 1
        es = [at[M.normalize(w)] for w in M.windows(t[2], k)]
        assert t[4] == "KC:i:%d" % sum(j["kc"][e] for e in es), line
        # a unitig's entries are of one class: one is_gene, one set of graphs
        assert len({(j["is_gene"][e], j["member"][e]) for e in es}) == 1, line
        col = colour(j["is_gene"][es[0]], bin(j["member"][es[0]]).count("1"), len(files))
        assert t[5] == "CL:Z:" + col and t[6] == "C2:Z:" + col, line
        assert t[1].endswith("_start") == bool(j["is_gene"][es[0]]), line
    assert n_s > 0
    return j, entries


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("k", KS)
def test_designed_graphs_three_ways_and_model(hosttest, tmp_path, k, G):
    files, gene = M.designed_case(k, G)
    want, envs, last = three_ways(hosttest, tmp_path, files, gene)
    j, entries = check_model(want, envs, files, gene, k)
    assert last == "ENTRIES %d" % len(entries)
    # the case is what it says it is
    graphs = [M.graph_dict(lines) for lines in files]
    assert any(j["is_gene"]) and not all(j["is_gene"])
    assert any(x in graphs[0] and M.rc(x) in graphs[0] for x in graphs[0])              # both orientations in one graph
    assert len(files[0]) > len(graphs[0])                                                 # a k-mer on two lines
    if G > 1:
        assert any(M.rc(x) in graphs[0] and x not in graphs[0] for x in graphs[G - 1])   # one orientation here, the other there
        assert len(set(j["member"])) > 1                                                  # the arms are in different sets of graphs
    if G >= 3:
        assert not files[1]                                                               # an empty graph
    # the bubble: no unitig runs from the stem into an arm (check_model saw one class a unitig), and the gene cuts the stem
    assert sum(1 for line in want["graph.gfa"].splitlines() if line.startswith("S\t")) >= (3 if G == 1 else 5)


def test_gene_shorter_than_k(hosttest, tmp_path):
    files, gene = M.designed_case(21, 2)
    want, envs, _ = three_ways(hosttest, tmp_path, files, gene[:20])
    j, _ = check_model(want, envs, files, gene[:20], 21)
    assert not any(j["is_gene"])
    assert "_start" not in want["graph.gfa"]


def test_treeified_bin_at_k5(hosttest, tmp_path):
    files, gene = M.treeified_case()
    want, envs, _ = three_ways(hosttest, tmp_path, files, gene)
    check_model(want, envs, files, gene, 5)
    union = ho.JavaHashMap()   # the union map of the k-mers and their reverse complements, as the tool fills it
    for p in envs:
        for kmer in ho.load_graph(p).keys():
            union.put(kmer, None)
            union.put(ho.reverse_complement(kmer), None)
    assert union.n_treeified > 0


def test_last_line_wins_in_kc(hosttest, tmp_path):
    """one k-mer on three lines of a file: the last depth is the one in KC and in the tables"""
    files, gene = M.designed_case(21, 1)
    graphs = [M.graph_dict(files[0])]
    x = files[0][-1][0]
    assert [d for y, d in files[0] if y == x][-2:] == [11, 13] and graphs[0][x] == 13
    want, envs, _ = three_ways(hosttest, tmp_path, files, gene)
    j, entries = check_model(want, envs, files, gene, 21)
    assert j["uni"][0][0] == sum(graphs[0].values())


@pytest.mark.parametrize("what", ["k70", "lower", "g65", "classes"])
def test_unpacked_inputs_are_named(hosttest, tmp_path, what):
    """what the packed path cannot represent ends it with a reason, and the string function takes the same input: its five files and
    its log are the oracle's, byte for byte (k above 63, more than 64 graphs and more than 256 merge classes reach the tool's writer
    through the string function alone)"""
    import random
    rng = random.Random(7)
    if what == "k70":
        s = M.random_dna(rng, 90)
        files, reason = [[(w, 3) for w in M.windows(s, 70)]], "k = 70 is above 63"
    elif what == "lower":
        s = M.random_dna(rng, 40)
        lines = [(w, 3) for w in M.windows(s, 21)]
        lines[5] = (lines[5][0].lower(), 3)
        files, reason = [lines], "outside upper-case ACGT"
    elif what == "g65":
        s = M.random_dna(rng, 40)
        files, reason = [[(w, 1 + g) for w in M.windows(s, 21)] for g in range(65)], "65 environments are more than 64"
    else:
        files, reason = many_classes_case(), "merge classes"
    envs, seq = write_inputs(tmp_path, files, "ACGTACGTTTGACCAGTACCCAT")
    r = run_tool(hosttest, "multi-packed", tmp_path / "packed", seq, envs, check=False)
    assert r.returncode == 3 and r.stderr.startswith("unpacked: ") and reason in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(str(tmp_path / "packed"))
    a = run_tool(hosttest, "multi", tmp_path / "string", seq, envs, check=False)
    if what == "lower":   # (the string function fails on it as the reference does: DnaTools.complement knows no 'c')
        assert a.returncode == 1 and "Incorrect nucleotide char" in a.stderr
    else:
        assert a.returncode == 0, a.stderr
        want, log = ho.environment_finder_multi(envs, seq, None, 1)
        got = read_files(tmp_path / "string")
        for f in FILES:
            assert got[f] == want[f], f
        assert a.stdout.splitlines() == log


def many_classes_case(k=21, G=9, n=300):
    """n k-mers, each in a different set of the G graphs"""
    import random
    rng = random.Random(300)
    kmers = set()
    while len(kmers) < n:
        w = M.random_dna(rng, k)
        if M.rc(w) not in kmers:
            kmers.add(w)
    files = [[] for _ in range(G)]
    for i, w in enumerate(sorted(kmers)):
        for g in range(G):
            if (i + 1) >> g & 1:
                files[g].append((w, 2))
    return files


def test_different_lengths_and_palindrome_keep_their_texts(hosttest, tmp_path):
    rng = __import__("random").Random(3)
    s = M.random_dna(rng, 40)
    files = [[(w, 3) for w in M.windows(s, 21)], [(w, 3) for w in M.windows(s, 22)]]
    envs, seq = write_inputs(tmp_path, files, s)
    a = run_tool(hosttest, "multi", tmp_path / "a", seq, envs, check=False)
    b = run_tool(hosttest, "multi-packed", tmp_path / "b", seq, envs, check=False)
    assert a.returncode == 1 and "K-mers of different lengths encountered" in a.stderr
    assert (b.returncode, b.stderr) == (a.returncode, a.stderr)
    pal = "ACGTTGCAAGCTTGCAACGT"  # its own reverse complement, k = 20
    assert M.rc(pal) == pal
    t = s[:15] + pal + s[15:]
    (tmp_path / "p").mkdir()
    envs, seq = write_inputs(tmp_path / "p", [[(w, 2) for w in M.windows(t, 20)]], s)
    a = run_tool(hosttest, "multi", tmp_path / "pa", seq, envs, check=False)
    b = run_tool(hosttest, "multi-packed", tmp_path / "pb", seq, envs, check=False)
    assert a.returncode == 1 and "palindromic k-mer" in a.stderr
    assert (b.returncode, b.stderr) == (a.returncode, a.stderr)
