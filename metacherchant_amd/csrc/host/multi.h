// --tool environment-finder-multi: src/tools/EnvironmentFinderMultiMain.java,
// src/algo/MultiSequenceCalculator.java, src/algo/MultiNode.java, src/io/writers/GFAWriterMulti.java,
// src/io/graph/DeBruijnGraphUtils.java.  Joins the graph.txt / env.txt files of several
// environment-finder runs into one coloured graph and two distance tables: on strings as the reference does
// (environment_finder_multi), or on packed k-mers with hooks for the join and the compaction (environment_finder_multi_packed).
// Both end in one writer (multi.cpp render_multi).
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "picture.h"

namespace mch {

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

}  // namespace mch
