// Host side of the environment-finder path above the C ABI: seed reading, runTrimPaths, the subgraph map and the writers of
// environment-finder's files, with the cutReads writer of the assembler-finder.  It mirrors the reference's classes (names below)
// so that the output files are byte-identical; the k-mer table and the BFS themselves live behind include/mcgpu.h.  What restates
// the JDK is java_replay.h, the merge into unitigs picture.h, environment-finder-multi multi.h: included here for the units
// that want the whole host side.
//
// Citations: src/... = reference src/; itmo!/x = ru/ifmo/genetics/x in lib/itmo-assembler-src.jar.
#pragma once
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "java_replay.h"
#include "multi.h"
#include "picture.h"
#include "reads_io.h"  // Error, code_of, the readers of read files

namespace mch {

// ---- src/io/RichFastaReader.java:38-77 (+ DnaQ(String,0).toString(): N/n/. -> 'A', itmo!/dna/DnaQ.java:21-30)
struct SeedFile {
    std::vector<std::string> dnas, comments;
};
SeedFile read_seed_fasta(const std::string &path);  // throws Error when the file cannot be opened

void write_file(const std::string &path, const std::string &text);  // mkdirs + write
bool read_lines(const std::string &path, std::vector<std::string> *lines);  // without their ends (\n, \r\n); false when the file cannot be opened

// ---- one runBfs pass as delivered by mc_bfs_batch (or by a dump file in the CPU tests)
struct BfsPass {
    int dir = 0;
    std::vector<kmer_t> kmers;  // distanceToKmer insertion order
    std::vector<int32_t> dist;
    std::vector<int16_t> cov;
    std::vector<uint8_t> last;
};

// ---- src/algo/OneSequenceCalculator.java (after the BFS) + src/algo/SingleNode.java +
// src/io/writers/GFAWriter.java + src/io/writers/TSVWriter.java; with set_colours, src/algo/SeqEnvCalculator.java (after its BFS)
// runTrimPaths (src/algo/OneSequenceCalculator.java:241-262) on `d`, distanceToKmer holding the k-mers of pass p: the walk from the
// `last` k-mers through getNeighborsByDir(-dir) inside d, then keySet().retainAll(visited), entry by entry in p's order.  kept: the
// walk's answer, one byte a k-mer of p (mc_trim_paths makes it): only the removals are done then.  (What Environment::add_pass
// does with trim, and what scripts/trim_paths_bench.py times.)
void trim_pass(JavaKmerMap &d, const BfsPass &p, int k, const std::vector<uint8_t> *kept = nullptr);

// The fmt-visualizer's host replay of KmerEnvCalculator.runBfs (:60-76) over one component: `canon` its canonical k-mers sorted,
// `count` beside them (zeroed here), seed its first k-mer as the read has it; returns the puts in pop order.  The queue has no
// visited set; with cap > 0 the replay gives up once the queue holds more entries than that, sets *abandoned and returns nothing.
std::vector<std::pair<kmer_t, int>> replay_component_walk(int k, kmer_t seed, const std::vector<kmer_t> &canon, std::vector<int> &count,
                                                          size_t cap = 0, bool *abandoned = nullptr);

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
    std::string node_id(size_t i) const;  // SingleNode's label: the smaller id of the node and its reverse complement, from 1
    int k_;
    std::vector<std::string> genes_;
    std::vector<kmer_t> gene_kmers_;  // sorted: every k-window of the gene sequences, for isGeneNode
    JavaKmerMap subgraph_;
    bool d_treeified_ = false;
    bool coloured_ = false;
    std::vector<Colour> colours_;  // by the subgraph's iteration order (set_colours)
    std::vector<PictureNode> nodes_;  // as make_picture leaves them: a node's id is its index, its entry index / 2
    std::vector<uint8_t> is_gene_;    // by entry (create_picture)
};

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

}  // namespace mch
