// The command line of `metacherchant` (options.cpp): every tool's parameters and the launch options in one struct, as
// parse_args fills it from the parameter table of the tool the line names.
#pragma once
#include <string>
#include <vector>

namespace mch {

struct Options {
    int k = -1;
    std::vector<std::string> reads;
    std::string seq, hicseq, output, output_dir, work_dir = "workDir", hash = "poly", tool = "environment-finder";
    long long maxkmers = -1, maxradius = -1;
    int coverage = 1, chunklength = 1, device = 0, geneid = 1;
    std::vector<std::string> env;
    bool bothdirs = false, forcehash = false, trim = false, merge = false, cont = false, force = false, help = false;
    unsigned long long capacity_hint = 0;
    std::vector<int> devices;  // --devices 0,1,...: several GPUs as one table (mc_group_*); empty: --device alone
    // --tool reads-classifier (src/tools/ReadsClassifier.java:42-95)
    std::vector<std::string> input_files, read_files;
    bool correction = false, interval95 = false;
    long long found_threshold = 90;
    // --tool triple-reads-classifier (src/tools/TripleReadsClassifier.java:40-105)
    int k2 = -1;
    std::vector<std::string> input_kmers_1, input_kmers_2;
    long long half_threshold = 40;
    // --tool seq-cov (src/tools/SequenceCoverage.java:30-72)
    std::vector<std::string> from_before, from_donor, from_both, itself;
    std::string read_file;
    // --tool recipient-visualiser (src/tools/RecipientVisualiser.java:42-92)
    std::vector<std::string> after_files;
    std::string input_dir, ext;
    // --tool fmt-visualizer (src/tools/FMTVisualizer.java:39-85)
    std::vector<std::string> donor_files, before_files;
    int processors = 0;  // -p: the threads that replay the components' walks (0: as many as the machine has, 16 at most)
    // --tool environment-assembler-finder (src/tools/EnvironmentAssemblerFinder.java:33-122)
    long long procfiltration = 1;
    std::string assembler, assemblerpath;
    // --compact: who compacts an environment's k-mers into unitigs (no counterpart in the reference; the files are the same)
    std::string compact = "auto";
    bool compact_given = false;
    // --join (environment-finder-multi): who joins the graph files and compacts the result (no counterpart in the reference; the files are the same)
    std::string join = "auto";
    bool join_given = false;
    // --parse: who parses the whole reads of the classifying tools (no counterpart in the reference; the files are the same)
    std::string parse = "auto";
    bool parse_given = false;
    // --trim-on: who works out which k-mers --trim keeps (no counterpart in the reference; the files are the same)
    std::string trim_on = "auto";
    bool trim_on_given = false;
    // --replay: who replays the order of the fmt-visualizer's walks (no counterpart in the reference; the files are the same)
    std::string replay = "auto";
    // --kmers-io: who encodes / decodes the records of a <name>.kmers.bin (no counterpart in the reference; the files are the same)
    std::string kmers_io = "auto";
    bool kmers_io_given = false;
    // --render: who turns the classifiers' reads into the text of their FASTQ files (no counterpart in the reference; the files are the same)
    std::string render = "auto";
    bool render_given = false;
};

std::string tool_of(int argc, char **argv);
bool java_bool(const std::string &s);
Options parse_args(int argc, char **argv);  // (-v / --verbose goes to g_verbose of cli.h)
void usage();

}  // namespace mch
