// The picture of a subgraph: its oriented k-mers as nodes, merged into unitigs (initializeStructures + doMerge of
// src/algo/OneSequenceCalculator.java:387-451 and src/algo/MultiSequenceCalculator.java:51-139), by the reference's loop on labels
// or from a Compactor's link analysis, and the seqs.fasta record both calculators write for a node.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "java_replay.h"

namespace mch {

// the one hash of packed k-mers for the host's own tables (none of them is iterated: the hash decides no output)
struct KmerHash {
    size_t operator()(kmer_t key) const
    {
        uint64_t h = (uint64_t)key ^ ((uint64_t)(key >> 64) * 0x9E3779B97F4A7C15ull);
        h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull; h ^= h >> 33;
        return (size_t)h;
    }
};

// ---- initializeStructures + doMerge over oriented k-mers in node order: entry e makes node 2e (kmers[e]) and node 2e + 1 (its
// reverse complement); two nodes merge only when their entries are of one class.
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
// doMerge alone, pass after pass over all the nodes a caller built itself (k-mer strings of any length and alphabet);
// same_class(e, f): may nodes of the entries e and f merge
void merge_picture(std::vector<PictureNode> &nodes, int k, const std::function<bool(size_t, size_t)> &same_class);

// outputNodeSequences (OneSequenceCalculator.java:354-385, MultiSequenceCalculator.java:141-160) for node i:
// the header `> Id<label> Length:<n> Neighbors:` with the list in brackets, then the label's line.  The list: the min ids (from 1)
// of both strands' neighbours, sorted, each once, without the node's own
void append_fasta_record(std::string &out, const std::vector<PictureNode> &nodes, size_t i, const std::string &label);

}  // namespace mch
