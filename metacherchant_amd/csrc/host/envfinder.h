// Host side of the environment-finder path above the C ABI: seed reading, read ingest (the
// readers' N policy + 2-bit packing), runTrimPaths, the subgraph map, unitig compaction and the
// writers.  It mirrors the reference's classes (names below) so that the output files are
// byte-identical; the k-mer table and the BFS themselves live behind include/mcgpu.h.
//
// Citations: src/... = reference src/; itmo!/x = ru/ifmo/genetics/x in lib/itmo-assembler-src.jar.
#pragma once
#include <cstdint>
#include <cstdio>
#include <deque>
#include <functional>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "reads_io.h"  // Error, code_of, the readers of read files

namespace mch {

// ---- DNA strings (itmo!/dna/DnaTools.java:31,46-64,131-145; src/utils/StringUtils.java:8-41)
std::string reverse_complement(const std::string &s);
std::string normalize_dna(const std::string &s);  // ASCII-lexicographic min of (s, rc(s))
std::vector<std::string> neighbors_by_dir(int dir, const std::string &kmer);  // A,G,C,T order; dir 0 interleaves L,R
void pack_kmer(const std::string &s, uint64_t *hi, uint64_t *lo);
std::string unpack_kmer(uint64_t hi, uint64_t lo, int k);

// ---- treeified bins of java.util.HashMap (JDK 8 HashMap.TreeNode).  A bin's iteration order is
// its nodes' next-chain, kept here as a vector of entry ids; the red-black tree over the same nodes decides where a new
// node is linked in: treeify() builds the tree in chain order and moves its root to the front (moveRootToFront),
// put() is putTreeVal (the new node goes right behind its tree parent, then balanceInsertion, then the root to the front).
// dir(x, p) = which way x goes below p: by the (signed) spread hash, then String.compareTo -- < 0 left, > 0 right.
class JavaTreeOrder {
public:
    explicit JavaTreeOrder(std::function<int(uint32_t, uint32_t)> dir) : dir_(std::move(dir)) {}
    void treeify(std::vector<uint32_t> &chain);
    void put(std::vector<uint32_t> &chain, uint32_t id);
    // removeTreeNode + balanceDeletion: the chain only loses `id` (with `movable` -- HashMap.remove; an iterator's remove, which
    // is what retainAll uses, passes false -- the root then moves to the front).  Returns true when the bin untreeifies (the tree
    // was too small BEFORE the removal) or is empty: the caller forgets the tree and keeps the chain as a plain list.
    bool remove(std::vector<uint32_t> &chain, uint32_t id, bool movable);
    void forget(const std::vector<uint32_t> &chain) { for (uint32_t id : chain) t_.erase(id); }

private:
    static constexpr uint32_t NIL = 0xFFFFFFFFu;
    struct Node { uint32_t parent = NIL, left = NIL, right = NIL; bool red = false; };
    uint32_t rotate_left(uint32_t root, uint32_t p);
    uint32_t rotate_right(uint32_t root, uint32_t p);
    uint32_t balance_insertion(uint32_t root, uint32_t x);
    uint32_t balance_deletion(uint32_t root, uint32_t x);
    static void root_to_front(std::vector<uint32_t> &chain, uint32_t root);
    std::function<int(uint32_t, uint32_t)> dir_;
    std::unordered_map<uint32_t, Node> t_;
};

// ---- java.util.HashMap<String,Integer> iteration order (JDK 8)
class JavaHashMap {
public:
    JavaHashMap();
    void put(const std::string &key, int value);  // new keys go to the tail of their bin; existing keep their place
    bool contains(const std::string &key) const { return index_.count(key) != 0; }
    int get(const std::string &key) const;         // throws if absent
    bool find(const std::string &key, int *value) const;
    void remove(const std::string &key, bool movable = false);
    size_t size() const { return size_; }
    // The order of a treeified bin is replayed node for node (JavaTreeOrder), removals included (removeTreeNode): nothing sets
    // the flag any more; it stays for callers that ask.
    bool treeified() const { return order_unknown_; }
    size_t bins_treeified() const { return n_treeified_; }  // bins that were treeified at some point (tests)
    template <typename F>
    void for_each(F &&f) const
    {
        for (const auto &bin : bins_)
            for (uint32_t e : bin) f(entries_[e].key, entries_[e].value);
    }

private:
    struct Entry { std::string key; int value; uint32_t hash; };
    void resize();
    int tree_dir(uint32_t x, uint32_t p) const;
    std::deque<Entry> entries_;
    std::vector<std::vector<uint32_t>> bins_;  // (a treeified bin's vector is its next-chain)
    std::vector<char> is_tree_;
    std::unordered_map<std::string, uint32_t> index_;
    JavaTreeOrder tree_;
    size_t cap_ = 16, size_ = 0, n_treeified_ = 0;
    bool order_unknown_ = false;
};

// ---- src/io/RichFastaReader.java:38-77 (+ DnaQ(String,0).toString(): N/n/. -> 'A', itmo!/dna/DnaQ.java:21-30)
struct SeedFile {
    std::vector<std::string> dnas, comments;
};
SeedFile read_seed_fasta(const std::string &path);  // throws Error when the file cannot be opened

// String.format("%.2f", x) for a double: HALF_UP on the shortest decimal that reads back as x (Java's FormattedFloatingDecimal)
std::string java_format_2f(double x);
// Double.toString as JDK 19 and later document it: the shortest decimal that reads back as x, at least one digit after the point,
// plain notation for 10^-3 <= |x| < 10^7 and d.dddE[-]n outside it (seq-cov's columns, src/tools/SequenceCoverage.java:184)
std::string java_double_to_string(double x);

// ---- 2-bit packed k-mers (k <= 63): base i of the string is bits 2(k-1-i)+1..2(k-1-i), codes A0 G1 C2 T3,
// the layout of mc_bfs_result's hi/lo words (include/mcgpu.h)
typedef unsigned __int128 kmer_t;
kmer_t pack_kmer128(const std::string &s);
inline std::string unpack_kmer128(kmer_t v, int k) { return unpack_kmer((uint64_t)(v >> 64), (uint64_t)v, k); }
kmer_t reverse_complement128(kmer_t v, int k);
kmer_t normalize128(kmer_t v, int k);  // the packed form of normalize_dna(string)

// java.util.HashMap<String, Integer> over k-mer strings held packed: the same bins, resize points, in-bin
// order and treeify detection as JavaHashMap, with String.hashCode() evaluated on the characters the
// packed key stands for.  Entries are chained per bin the way the JDK chains them.
class JavaKmerMap {
public:
    explicit JavaKmerMap(int k);
    int put(kmer_t key, int value);   // entry index; an existing key keeps its place and gets the value
    int find_entry(kmer_t key) const;  // -1 when absent
    int value_at(int e) const { return entries_[(size_t)e].value; }
    void remove(kmer_t key, bool movable = false);
    size_t size() const { return size_; }
    size_t n_entries() const { return entries_.size(); }  // removed ones included: bound of the entry indices
    bool treeified() const { return order_unknown_; }  // (see JavaHashMap::treeified)
    size_t bins_treeified() const { return n_treeified_; }
    template <typename F>
    void for_each(F &&f) const  // f(key, value, entry index) in HashMap iteration order
    {
        for (uint32_t h : head_)
            for (uint32_t e = h; e != NIL; e = entries_[e].next) f(entries_[e].key, entries_[e].value, (int)e);
    }

private:
    static constexpr uint32_t NIL = 0xFFFFFFFFu;
    struct Entry { kmer_t key; int value; uint32_t hash, next; };
    uint32_t hash_of(kmer_t key) const;
    void resize();
    int tree_dir(uint32_t x, uint32_t p) const;
    void relink(size_t bin, const std::vector<uint32_t> &chain);  // head_/tail_/next of a bin from its chain
    int k_;
    std::vector<Entry> entries_;
    std::vector<uint32_t> head_, tail_;
    std::unordered_map<size_t, std::vector<uint32_t>> tree_bins_;  // treeified bins: their next-chains
    JavaTreeOrder tree_;
    size_t cap_ = 16, size_ = 0, n_treeified_ = 0;
    bool order_unknown_ = false;
};

// ---- one runBfs pass as delivered by mc_bfs_batch (or by a dump file in the CPU tests)
struct BfsPass {
    int dir = 0;
    std::vector<kmer_t> kmers;  // distanceToKmer insertion order
    std::vector<int32_t> dist;
    std::vector<int16_t> cov;
    std::vector<uint8_t> last;
};

// ---- initializeStructures + doMerge (src/algo/OneSequenceCalculator.java:387-451) over oriented k-mers in node order: entry e makes
// node 2e (kmers[e]) and node 2e + 1 (its reverse complement); two nodes merge only when cls is equal for their entries.
struct PictureNode {
    std::string sequence;
    bool deleted = false;
    int rc = 0;                  // index of the reverse-complement node
    std::vector<int> neighbors;  // successors of rc(this), in node-array order
};
// What the loop ends in, from link analysis: the fields of mc_unitigs_result (include/mcgpu.h has the definitions), owned.
struct UnitigsResult {
    std::vector<uint8_t> deg;
    std::vector<uint32_t> nbr, first, last_rc, irregular;
    std::vector<uint64_t> base_offsets, bases;
};
// fills a result for the k-mers and classes given (mc_unitigs on a context, or unitigs_by_links); throws Error
using Compactor = std::function<void(int k, const std::vector<kmer_t> &kmers, const std::vector<uint8_t> &cls, UnitigsResult &out)>;
// the host's link analysis: no label is built before the chains are known.  The model of csrc/unitigs.hip.
void unitigs_by_links(int k, const std::vector<kmer_t> &kmers, const std::vector<uint8_t> &cls, UnitigsResult &out);
// Without a compactor: the reference's loop on labels, pass after pass over all nodes.  With one: the nodes are built from its result
// and the same loop runs over the nodes of the irregular entries only.  Alive nodes, `deleted` and the neighbours lists come out
// the same either way; what a deleted node keeps as label and rc depends on the loop's scan order and is never read.
std::vector<PictureNode> make_picture(int k, const std::vector<kmer_t> &kmers, const std::vector<uint8_t> &cls, const Compactor *compact = nullptr);

// ---- src/algo/OneSequenceCalculator.java (after the BFS) + src/algo/SingleNode.java +
// src/io/writers/GFAWriter.java + src/io/writers/TSVWriter.java; with set_colours, src/algo/SeqEnvCalculator.java (after its BFS)
// runTrimPaths (src/algo/OneSequenceCalculator.java:241-262) on `d`, distanceToKmer holding the k-mers of pass p: the walk from the
// `last` k-mers through getNeighborsByDir(-dir) inside d, then keySet().retainAll(visited), entry by entry in p's order.  kept: the
// walk's answer, one byte a k-mer of p (mc_trim_paths makes it): only the removals are done then.  (What Environment::add_pass
// does with trim, and what scripts/trim_paths_bench.py times.)
void trim_pass(JavaKmerMap &d, const BfsPass &p, int k, const std::vector<uint8_t> *kept = nullptr);

class Environment {
public:
    Environment(int k, std::vector<std::string> gene_sequences);
    // SingleNode.Color, in the enum's order; colour_of_mask: src/tools/RecipientVisualiser.java:157-169 with bit 0 = from_donor,
    // 1 = from_before (the came_from_baseline files), 2 = from_both, 3 = itself
    enum Colour : int8_t { NO_COLOUR = -1, RED, GREEN, BLUE, GREY, YELLOW, BLACK };
    static Colour colour_of_mask(unsigned mask);
    static const char *colour_name(Colour c);
    // The recipient-visualiser's nodes (SeqEnvCalculator.java:165-206): of(k-mer) is asked for every entry of the subgraph in its
    // iteration order; create_picture then merges only nodes of one colour (:214) and graph_gfa ends every S line with CL:Z:<colour>.
    // Without this call nothing changes: environment-finder's files.
    void set_colours(const std::function<Colour(kmer_t)> &of);
    // extendEnvironment (SeqEnvCalculator.java:119-149) adds nothing -- its `cont` is the k-mer itself -- but logs how many k-mers of
    // the subgraph have exactly one of their eight neighbours outside it and in the graph.  outside_neighbours: those neighbours that
    // are not in the subgraph (oriented, allNeighbors order, one entry an occurrence) with the ordinal of their k-mer;
    // extensions: the count, given which of them the graph holds.
    struct Outside { std::vector<kmer_t> kmers; std::vector<uint32_t> of; };
    Outside outside_neighbours() const;
    static size_t extensions(const Outside &o, const uint8_t *in_graph);
    // :217-219 (+ runTrimPaths :241-262 when trim): distanceToKmer -> subgraph
    // kept (with trim): one byte an entry of p, whether runTrimPaths' walk visits it (mc_trim_paths makes it); the walk is then left
    // out and only retainAll's removals are done, in the same order
    void add_pass(const BfsPass &p, bool trim, const std::vector<uint8_t> *kept = nullptr);
    // The fmt-visualizer's subgraph (src/algo/KmerEnvCalculator.java:87-89): subgraph.put(normalizeDna(kmer), value) for every entry,
    // in the order given -- the walk's pops, a k-mer popped again overwriting its value where it is.  With no gene sequences the
    // nodes are not gene nodes and seqs_fasta's header is KmerEnvCalculator's `Id<n>`; colours as set_colours gives them.
    void add_puts(const std::vector<std::pair<kmer_t, int>> &puts);
    size_t size() const { return subgraph_.size(); }
    // the subgraph's keys (normalised k-mers) in its iteration order, graph.txt's: what isContainedInSubgraph tests against
    // (OneSequenceCalculator.java:150-152)
    std::vector<kmer_t> kmers() const;
    bool order_guaranteed() const { return !subgraph_.treeified() && !d_treeified_; }
    std::string graph_txt() const;                    // printEnvironment :297-310
    // initializeStructures + doMerge :387-451 (make_picture; colour and is_gene make the merge class)
    void create_picture(const Compactor *compact = nullptr);
    std::string seqs_fasta(int chunk_length) const;   // outputNodeSequences :354-385
    std::string graph_gfa() const;                    // GFAWriter.java:47-99
    std::string tsv_nodes() const;                    // TSVWriter.java:35-49
    std::string tsv_edges() const;                    // TSVWriter.java:51-79
    // writes graph.txt (+ the identical env.txt README.md:98 names), seqs.fasta, graph.gfa, tsvs/*
    void write_all(const std::string &out_prefix, int chunk_length, const Compactor *compact = nullptr);

private:
    struct Node {
        std::string sequence;
        int id;
        bool is_gene, deleted = false;
        int rc;                      // index of the reverse-complement node
        std::vector<int> neighbors;  // successors of rc(this), in node-array order
        Colour colour = NO_COLOUR;
    };
    std::string node_id(const Node &n) const;
    int k_;
    std::vector<std::string> genes_;
    std::vector<kmer_t> gene_kmers_;  // sorted: every k-window of the gene sequences, for isGeneNode
    JavaKmerMap subgraph_;
    bool d_treeified_ = false;
    bool coloured_ = false;
    std::vector<Colour> colours_;  // by the subgraph's iteration order (set_colours)
    std::vector<Node> nodes_;
};

void write_file(const std::string &path, const std::string &text);  // mkdirs + write

// ---- the environment-assembler-finder's cutReads<i>.fasta (src/algo/ReadsFilter.java:36-41,58-66): created empty with its
// directory, then `>i|n` and the bases as DnaQ.toString() prints them for every kept read of file i, n counting them from 1
class CutReadsWriter {
public:
    CutReadsWriter(const std::string &path, int file_index);
    ~CutReadsWriter();
    CutReadsWriter(const CutReadsWriter &) = delete;
    CutReadsWriter &operator=(const CutReadsWriter &) = delete;
    void add(const uint8_t *codes, size_t n);  // base codes A0 G1 C2 T3 (N is 0 already)
    uint64_t kept() const { return kept_; }
    void close();  // throws Error when the file could not be written

private:
    std::string path_, buf_;
    FILE *f_;
    int index_;
    uint64_t kept_ = 0;
    void flush();
};

// ---- --tool environment-finder-multi: src/tools/EnvironmentFinderMultiMain.java,
// src/algo/MultiSequenceCalculator.java, src/algo/MultiNode.java, src/io/writers/GFAWriterMulti.java,
// src/io/graph/DeBruijnGraphUtils.java.  Joins the graph.txt / env.txt files of several
// environment-finder runs into one coloured graph and two distance tables: on strings as the reference does
// (environment_finder_multi), or on packed k-mers with hooks for the join and the compaction (environment_finder_multi_packed).
struct MultiResult {
    std::string seqs_fasta, graph_gfa, gene_fasta, jacard_sym, jacard_alt;  // <output>/seqs.fasta, graph.gfa, gene.fasta, Jacard_*.txt
    std::vector<std::string> log;                                            // "INFO ..." / "WARN ..." lines, in order
};
MultiResult environment_finder_multi(const std::vector<std::string> &env_paths, const std::string &seq_path, int gene_id);

// ---- the same tool on packed k-mers.  The join of the graph files (which graphs hold a k-mer, the KC column's depths, is it a gene
// k-mer, the sums of the two distance tables) is a Joiner's work and the merge loop a Compactor's: include/mcgpu.h mc_env_join has the
// definitions of the join's fields, which are EnvJoinResult's.
struct EnvJoinInput {
    int k = 0;
    std::vector<kmer_t> entries;                       // entry e: nodes 2e (as given) and 2e + 1 (its reverse complement)
    std::vector<kmer_t> rec_kmers;                     // the graphs' records one graph after another, as the files spell them
    std::vector<int32_t> rec_depth;
    std::vector<uint64_t> graph_offsets;               // n_graphs + 1
    std::vector<uint64_t> gene_words;                  // the gene packed as reads are, gene_len bases
    uint64_t gene_len = 0;
    size_t n_graphs() const { return graph_offsets.empty() ? 0 : graph_offsets.size() - 1; }
};
struct EnvJoinResult {
    std::vector<uint64_t> member;
    std::vector<uint8_t> is_gene;
    std::vector<int64_t> kc;
    std::vector<uint32_t> diff, diff_alt, uni;  // n_graphs x n_graphs, row i column j at i * n_graphs + j
};
// fills a result for the input given (mc_env_join on a context, or env_join_host); throws Error
using Joiner = std::function<void(const EnvJoinInput &in, EnvJoinResult &out)>;
// the host's join on packed keys, from the definitions.  The model of csrc/env_join.hip.
void env_join_host(const EnvJoinInput &in, EnvJoinResult &out);
// What the packed path cannot represent (what() names it): k above 63, a k-mer with a character outside upper-case ACGT, more than
// 64 graphs, more than 256 merge classes.  environment_finder_multi takes those inputs.
struct MultiUnpacked : Error {
    using Error::Error;
};
// The files and log lines of environment_finder_multi, byte for byte, with no string k-mer on the way.  n_entries: where the number of
// entries goes once it is known (NULL: nowhere).
MultiResult environment_finder_multi_packed(const std::vector<std::string> &env_paths, const std::string &seq_path, int gene_id, const Joiner &join,
                                            const Compactor &compact, size_t *n_entries = nullptr);
void write_multi(const MultiResult &r, const std::string &output_dir);
std::string java_format_6_2f(float x);  // String.format("%6.2f", x)

}  // namespace mch
