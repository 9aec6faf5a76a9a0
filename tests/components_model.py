"""The fmt-visualizer in plain Python, restated from the reference's source: src/tools/FMTVisualizer.java (runImpl: three phases, the
scan of every window of every read, the colour rules of :195-221) and src/algo/KmerEnvCalculator.java (one walk: a FIFO of oriented
strings without a visited set, over a table that it zeroes; then nodes, merge, FASTA and GFA as SeqEnvCalculator's, without gene
nodes).  Test infrastructure only.

The graph is a dict key -> count which the walks zero (count_table builds one); class tables are anything recipient_model.contains
takes.  java.util.HashMap's iteration order, all_neighbors, kmer_key and the writers are tests/recipient_model.py's.

Hash keys (k > 31 or --hash): mc_components lets the first-seen k-mer of a key explore for it, so its answer is the reference's only
while no two distinct canonical k-mers among the members and their neighbours share a key; the model asserts that on its input."""
from oracle.host_oracle import JavaHashMap, SingleNode, normalize_dna, reverse_complement
from tests.recipient_model import SeqEnv, all_neighbors, colour_of_mask, contains, kmer_key

PHASES = (("donor", ("settle", "not_settle")), ("before", ("stay", "gone")),
          ("after", ("came_from_donor", "came_from_baseline", "came_from_both", "came_itself")))


def count_table(reads, k, mode):
    """loadReads as a dict: every window's key counted, saturating at 32767 (NumUtils.addAndBound)"""
    t = {}
    for r in reads:
        for i in range(len(r) - k + 1):
            key = kmer_key(r[i:i + k], k, mode)
            t[key] = min(t.get(key, 0) + 1, 32767)
    return t


def two_table_colour(mask):
    """getDonorColorNode / getBeforeColorNode (:195-207): bit 0 the found class (settle, stay), bit 1 the other"""
    return {1: "GREEN", 2: "BLUE", 3: "GREY", 0: "BLACK"}[mask]


class KmerEnv(SeqEnv):
    """One KmerEnvCalculator.  graph is the phase's dict, shared by all its walks: run_bfs zeroes what it reaches."""

    def __init__(self, kmer, k, mode, graph, classes, name, keys=None):
        SeqEnv.__init__(self, kmer, k, mode, graph, classes, name)
        self.keys = {} if keys is None else keys  # string -> key, shared by the walks of a phase (a cache, nothing more)
        self.members = {}                         # canonical k-mer -> the count the table held when it was first popped
        self.owner = {}                           # key -> the canonical k-mer that was seen with it (the no-collision condition)

    def _key(self, s):
        key = self.keys.get(s)
        if key is None:
            key = self.keys[s] = kmer_key(s, self.k, self.mode)
        if self.k > 31 or self.mode != 0:
            assert self.owner.setdefault(key, normalize_dna(s)) == normalize_dna(s), "two k-mers share key %d: %s" % (key, s)
        return key

    def run_bfs(self):
        """:60-76.  get > 0 is asked of the table as it is NOW; a k-mer popped a second time is put again, with coverage 0."""
        queue, head = [self.sequence], 0
        while head < len(queue):
            kmer = queue[head]
            head += 1
            for nb in all_neighbors(kmer):
                if self.graph.get(self._key(nb), -1) > 0:
                    queue.append(nb)
            key = self._key(kmer)
            now = self.graph.get(key, -1)
            self.subgraph.put(normalize_dna(kmer), now)
            if now > 0:
                self.members[normalize_dna(kmer)] = now
            if key in self.graph:  # (always: the seed and every queued k-mer had get > 0 when they were queued)
                self.graph[key] = 0  # addAndBound(key, -get): 0, from a saturated 32767 too
        self.pops = len(queue)
        return True

    def initialize_structures(self):
        """:105-140: SeqEnvCalculator's without gene nodes; the colour is the tool's function of the k-mer"""
        k, nodes = self.k, []
        for s, _ in self.subgraph.items():
            colour = self.classes(s)
            a, b = SingleNode(s, len(nodes), colour, False), SingleNode(reverse_complement(s), len(nodes) + 1, colour, False)
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

    def run(self):
        """:52-58, :91-103"""
        self.run_bfs()
        self.initialize_structures()
        self.do_merge()
        return {self.name + "_seqs.fasta": self.seqs_fasta(), self.name + ".gfa": self.graph_gfa()}


def phase(k, mode, graph, colour, sequences, pictures=True):
    """One block of runImpl (:228-254) over a loaded graph, which it zeroes.  Returns ({file name: text}, [(seed_seq, seed_pos,
    {canonical k-mer: count})]); pictures=False leaves the files out (the walks alone)."""
    files, comps, keys = {}, [], {}
    for s, seq in enumerate(sequences):
        for i in range(len(seq) - k + 1):
            kmer = seq[i:i + k]
            key = keys.get(kmer)
            if key is None:
                key = keys[kmer] = kmer_key(kmer, k, mode)
            if graph.get(key, -1) > 0:
                e = KmerEnv(kmer, k, mode, graph, colour, "comp%d" % len(comps), keys)
                if pictures:
                    files.update(e.run())
                else:
                    e.run_bfs()
                comps.append((s, i, e.members))
    return files, comps


def fmt_visualizer(k, mode, inputs):
    """FMTVisualizer.runImpl.  inputs[phase] = (graph reads, {class name: reads}) as strings (N already A), for the phases donor,
    before, after; the phase's reads are both its graph and its scan.  Returns ({path under the output directory: bytes},
    {phase: components})."""
    files, comps = {}, {}
    for name, classes in PHASES:
        reads, class_reads = inputs[name]
        tables = [count_table(class_reads[c], k, mode) for c in classes]

        def colour(s, tables=tables):
            mask = sum(1 << t for t, tab in enumerate(tables) if contains(tab, kmer_key(s, k, mode)))
            return two_table_colour(mask) if len(tables) == 2 else colour_of_mask(mask)
        f, comps[name] = phase(k, mode, count_table(reads, k, mode), colour, reads)
        for fn, text in f.items():
            files[name + "/" + fn] = text.encode()
    return files, comps
