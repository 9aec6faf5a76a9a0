"""The recipient-visualiser in plain Python, restated from the reference's source: src/tools/RecipientVisualiser.java (the tool, the
colour rule), src/algo/SeqEnvCalculator.java (one sequence: walk, extension count, nodes, merge, the FASTA) and
src/io/writers/GFAWriter.java (the GFA with its five-argument constructor).  Test infrastructure only.

Tables are anything with get(key) -> count or -1 (oracle.pyoracle.Table) or a dict key -> count; keys are the tool's getKmerKey
(oracle.pyoracle.key: the canonical packed k-mer for k <= 31, the polynomial or FNV-1a hash above).  java.util.HashMap's
iteration order, which decides the node ids, is oracle.host_oracle.JavaHashMap's."""
from oracle import pyoracle as po
from oracle.host_oracle import JavaHashMap, SingleNode, normalize_dna, reverse_complement

NUCLEOTIDES = "AGCT"  # src/utils/StringUtils.java:8
CLASS_NAMES = ("came_from_donor", "came_from_baseline", "came_from_both", "came_itself")  # bits 0..3 of a mask


def kmer_key(s, k, mode):
    """getKmerKey (SeqEnvCalculator.java:106-113, RecipientVisualiser.java:99-106)"""
    return po.key(po.encode(s), k, mode)


def count_in(table, key):
    """getWithZero"""
    c = table.get(key, 0) if isinstance(table, dict) else table.get(key)
    return max(int(c), 0)


def contains(table, key):
    """BigLong2ShortHashMap.contains"""
    return key in table if isinstance(table, dict) else table.get(key) != -1


def all_neighbors(kmer):
    """src/utils/StringUtils.java:23-32: left and right neighbours interleaved, A G C T"""
    out = []
    for c in NUCLEOTIDES:
        out.append(c + kmer[:-1])
        out.append(kmer[1:] + c)
    return out


def colour_of_mask(mask):
    """RecipientVisualiser.java:157-169 with bit 0 donor, 1 baseline (from_before), 2 both, 3 itself"""
    return {1: "RED", 2: "BLUE", 4: "GREEN", 8: "YELLOW", 0: "BLACK"}.get(mask, "GREY")


def mask_of(kmer, k, mode, classes):
    key = kmer_key(kmer, k, mode)
    return sum(1 << t for t, tab in enumerate(classes) if contains(tab, key))


class SeqEnv:
    """One SeqEnvCalculator.  run() returns (files or None, log lines)."""

    def __init__(self, sequence, k, mode, graph, classes, name, max_kmers=None, max_radius=None):
        self.sequence, self.k, self.mode, self.graph, self.classes, self.name = sequence, k, mode, graph, classes, name
        self.max_kmers, self.max_radius = max_kmers, max_radius
        self.subgraph = JavaHashMap()
        self.nodes = None
        self.cut_a_level = False  # (for the tests: --maxkmers refused a k-mer while others of its distance were taken)

    def _cov(self, kmer):
        return count_in(self.graph, kmer_key(kmer, self.k, self.mode))

    def _allows(self, d, kmer, new_distance):
        """TerminationMode.allowsAddition (src/algo/TerminationMode.java:31-47)"""
        if kmer in d:
            return False
        if self.max_kmers is not None and len(d) >= self.max_kmers:
            self.refused_at.add(new_distance)
            return False
        if self.max_radius is not None and new_distance > self.max_radius:
            return False
        return True

    def run_bfs(self):
        """:71-104; False when no window of the sequence is in the graph"""
        k, seq = self.k, self.sequence
        queue, d = [], JavaHashMap()
        self.refused_at = set()
        self.inserted = []  # (distanceToKmer's keys in insertion order: what mc_bfs_batch lists)
        for i in range(len(seq) - k + 1):
            kmer = seq[i:i + k]
            if self._cov(kmer) > 0:
                queue.append(kmer)  # (a repeated window is queued again; the map keeps its one entry where it is)
                if kmer not in d:
                    self.inserted.append(kmer)
                d.put(kmer, 0)
        if not queue:
            return False
        head = 0
        while head < len(queue):
            kmer = queue[head]
            head += 1
            distance = d.get(kmer)
            for nb in all_neighbors(kmer):
                if self._cov(nb) > 0 and self._allows(d, nb, distance + 1):
                    queue.append(nb)
                    self.inserted.append(nb)
                    d.put(nb, distance + 1)
        self.distance = d
        self.cut_a_level = any(dist in self.refused_at for _, dist in d.items())
        for kmer in d.keys():
            self.subgraph.put(normalize_dna(kmer), self._cov(kmer))
        return True

    def extend_environment(self):
        """:119-149.  `cont` is the k-mer itself, so an addition is a k-mer the subgraph holds already: nothing changes but the count."""
        additions = set()
        for kmer0 in list(self.subgraph.keys()):
            kmer = kmer0
            while True:
                cont = None
                for nb in all_neighbors(kmer):
                    if normalize_dna(nb) not in self.subgraph and self._cov(nb) > 0:
                        cont = kmer if cont is None else ""
                if cont is not None and cont != "" and cont not in additions:
                    additions.add(cont)
                    kmer = cont
                else:
                    break
        for kmer in additions:
            self.subgraph.put(normalize_dna(kmer), self._cov(kmer))
        return len(additions)

    def initialize_structures(self):
        """:165-206"""
        k, seq = self.k, self.sequence
        gene = {seq[i:i + k] for i in range(len(seq) - k + 1)}
        nodes = []
        for s, _ in self.subgraph.items():
            rc = reverse_complement(s)
            colour = colour_of_mask(mask_of(s, k, self.mode, self.classes))
            g = s in gene or rc in gene
            a, b = SingleNode(s, len(nodes), colour, g), SingleNode(rc, len(nodes) + 1, colour, g)
            a.rc, b.rc = b, a
            nodes += [a, b]
        by_prefix = {}
        for n in nodes:
            by_prefix.setdefault(n.sequence[:k - 1], []).append(n)
        for n in nodes:
            lst = by_prefix.get(n.sequence[1:])
            if lst is not None:
                n.rc.neighbors.extend(lst)
        self.nodes = nodes

    def do_merge(self):
        """:208-250"""
        k = self.k

        def merge_labels(a, b):
            assert a[len(a) - (k - 1):] == b[:k - 1], "Labels should be merged, but can not: %s and %s" % (a, b)
            return a + b[k - 1:]

        while True:
            acted = False
            for n in self.nodes:
                if not n.deleted and len(n.neighbors) == 1:
                    other = n.neighbors[0]
                    if len(other.neighbors) != 1 or n.color != other.color or n.is_gene != other.is_gene:
                        continue
                    first_minus, second_plus = n.rc, other.rc
                    new_seq = merge_labels(second_plus.sequence, n.sequence)
                    new_seq_rc = merge_labels(first_minus.sequence, other.sequence)
                    second_plus.sequence, first_minus.sequence = new_seq, new_seq_rc
                    second_plus.rc, first_minus.rc = first_minus, second_plus
                    n.deleted = other.deleted = True
                    acted = True
            if not acted:
                break

    @staticmethod
    def _min_id(n):
        return min(n.id, n.rc.id) + 1

    def _node_id(self, n):
        return "%d%s" % (self._min_id(n), "_start" if n.is_gene else "")

    def seqs_fasta(self):
        """:252-287 (the TreeSet prints as [a, b])"""
        out = []
        for n in self.nodes:
            if not n.deleted and n.id < n.rc.id and len(n.sequence) >= 1:
                ids = {self._min_id(x) for x in n.neighbors} | {self._min_id(x) for x in n.rc.neighbors}
                ids.discard(self._min_id(n))
                out.append("> Id%s Length:%d Neighbors:[%s]\n%s\n" % (self._node_id(n), len(n.sequence), ", ".join(map(str, sorted(ids))),
                                                                      n.sequence))
        return "".join(out)

    def graph_gfa(self):
        """GFAWriter.java:47-99"""
        k, out = self.k, []
        for n in self.nodes:
            if not n.deleted and n.sequence <= n.rc.sequence:
                s = n.sequence
                cov = sum(self.subgraph.get(normalize_dna(s[i:i + k])) for i in range(len(s) - k + 1))
                cov += self.subgraph.get(normalize_dna(s[len(s) - k:])) * (k - 1)
                out.append("S\t%s\t%s\tLN:i:%d\tKC:i:%d\tCL:Z:%s\n" % (self._node_id(n), s, len(s), cov, n.color))
        for i in self.nodes:
            if not i.deleted:
                for j in i.neighbors:
                    if not j.deleted:
                        out.append("L\t%s\t%s\t%s\t%s\t%dM\n" % (self._node_id(i), "+" if i.sequence >= i.rc.sequence else "-",
                                                                 self._node_id(j), "+" if j.sequence <= j.rc.sequence else "-", k - 1))
        return "".join(out)

    def run(self):
        """:58-69, :151-163"""
        if not self.run_bfs():
            return None, ["Could not find any k-mers of the target gene in the input, halting."]
        self.n_extensions = self.extend_environment()
        log = ["Extending endings by %d kmers" % self.n_extensions]
        self.initialize_structures()
        self.do_merge()
        return {self.name + "_seqs.fasta": self.seqs_fasta(), self.name + ".gfa": self.graph_gfa()}, log


def recipient_visualiser(k, mode, graph, classes, sequences, max_kmers=None, max_radius=1000):
    """RecipientVisualiser.runImpl (:185-223) over loaded tables: classes = (donor, baseline, both, itself), sequences = the records of
    --seq as strings (N already A).  Returns ({path under the output directory: text}, log lines in sequence order, the SeqEnv objects)."""
    files, log, envs = {}, [], []
    for i, s in enumerate(sequences):
        e = SeqEnv(s, k, mode, graph, classes, "comp_%d" % i, max_kmers, max_radius)
        f, lines = e.run()
        envs.append(e)
        log += lines
        for name, text in (f or {}).items():
            files["after/" + name] = text
    log.append("Finished processing all sequences!")
    return files, log, envs
