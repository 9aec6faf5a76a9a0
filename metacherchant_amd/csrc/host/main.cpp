// metacherchant -- native launcher of the MI355X environment-finder path.  Mirrors the command line
// of the reference (src/Runner.java + src/tools/EnvironmentFinderMain.java:32-105 + the launch
// options of itmo!/utils/tool/Tool.java:59-143) and its output surface, and
// drives libmcgpu.so through the C ABI of include/mcgpu.h exactly where the Java tool calls
// IOUtils.loadReads / LargeKIOUtils.loadReads and OneSequenceCalculator.runBfs.
#include <spawn.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "envfinder.h"
#include "fastq_out.h"
#include "gpu_compactor.h"
#include "gpu_joiner.h"
#include "mcgpu.h"
#include "whole_reads_source.h"

using namespace mch;

namespace {

FILE *g_log = nullptr, *g_log2 = nullptr;
bool g_verbose = false;

void logline(const char *level, const std::string &msg)
{
    char ts[32];
    const time_t now = time(nullptr);
    strftime(ts, sizeof ts, "%Y-%m-%d %H:%M:%S", localtime(&now));
    const bool debug = strcmp(level, "DEBUG") == 0;
    if (!debug || g_verbose) fprintf(stderr, "%s %s: %s\n", ts, level, msg.c_str());
    for (FILE *f : {g_log, g_log2})
        if (f) { fprintf(f, "%s %s: %s\n", ts, level, msg.c_str()); fflush(f); }
}
void info(const std::string &m) { logline("INFO", m); }

std::string group_digits(unsigned long long v)  // itmo!/utils/NumUtils.java:163-174
{
    std::string vs = std::to_string(v), ans;
    while (vs.size() > 3) {
        ans = "'" + vs.substr(vs.size() - 3) + ans;
        vs = vs.substr(0, vs.size() - 3);
    }
    return vs + ans;
}

std::string shorten_label(const std::string &label, int k)  // src/utils/StringUtils.java:43-49
{
    if ((int)label.size() >= 2 * k)
        return label.substr(0, (size_t)k) + "..." + label.substr(label.size() - (size_t)k) + " (length=" +
               std::to_string(label.size()) + ")";
    return label;
}

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
    // --kmers-io: who encodes / decodes the records of a <name>.kmers.bin (no counterpart in the reference; the files are the same)
    std::string kmers_io = "auto";
    bool kmers_io_given = false;
    // --render: who turns the classifiers' reads into the text of their FASTQ files (no counterpart in the reference; the files are the same)
    std::string render = "auto";
    bool render_given = false;
};

struct OptSpec { const char *name; const char *shortopt; int kind; };  // kind: 0 value, 1 bool (optional arg), 2 multi
// Every tool has its own parameters (itmo!/utils/tool/Tool.java: a tool's addParameter calls plus the launch options), and a
// short option may mean something else in another tool: -o is --output here and --output-dir in reads-classifier.
const OptSpec SPECS[] = {
    {"k", "k", 0}, {"reads", "i", 2}, {"seq", nullptr, 0}, {"hicseq", nullptr, 0}, {"output", "o", 0},
    {"maxkmers", nullptr, 0}, {"maxradius", nullptr, 0}, {"coverage", nullptr, 0}, {"bothdirs", nullptr, 1},
    {"chunklength", nullptr, 0}, {"forcehash", nullptr, 1}, {"hash", nullptr, 0}, {"trim", nullptr, 1},
    {"merge", nullptr, 1}, {"work-dir", "w", 0}, {"available-processors", "p", 0}, {"memory", "m", 0},
    {"continue", "c", 1}, {"force", nullptr, 1}, {"verbose", "v", 1}, {"help", "h", 1}, {"tool", "t", 0},
    {"device", nullptr, 0}, {"devices", nullptr, 0}, {"capacity-hint", nullptr, 0}, {"output-dir", nullptr, 0}, {"env", "e", 2}, {"geneid", "g", 0},
    {"compact", nullptr, 0}, {"join", nullptr, 0}, {"parse", nullptr, 0}, {"trim-on", nullptr, 0}, {"kmers-io", nullptr, 0},
    {"render", nullptr, 0},
};

// --tool reads-classifier: its parameters (ReadsClassifier.java:42-95) and the launch options
const OptSpec CLASSIFIER_SPECS[] = {
    {"k", "k", 0}, {"input-files", "i", 2}, {"read-files", "r", 2}, {"output-dir", "o", 0}, {"correction", "corr", 1},
    {"hash", nullptr, 0}, {"interval95", nullptr, 1}, {"found-threshold", "found", 0},
    {"work-dir", "w", 0}, {"available-processors", "p", 0}, {"memory", "m", 0}, {"continue", "c", 1}, {"force", nullptr, 1},
    {"verbose", "v", 1}, {"help", "h", 1}, {"tool", "t", 0}, {"device", nullptr, 0}, {"capacity-hint", nullptr, 0}, {"parse", nullptr, 0},
    {"kmers-io", nullptr, 0}, {"render", nullptr, 0},
};

// --tool triple-reads-classifier: its parameters (TripleReadsClassifier.java:40-105) and the launch options
const OptSpec TRIPLE_SPECS[] = {
    {"k", "k", 0}, {"k2", "k2", 0}, {"input-files", "i", 2}, {"input-kmers-1", "ik1", 2}, {"input-kmers-2", "ik2", 2}, {"read-files", "r", 2},
    {"output-dir", "o", 0}, {"hash", nullptr, 0}, {"correction", "corr", 1}, {"interval95", nullptr, 1}, {"found-threshold", "found", 0},
    {"half-threshold", "half", 0},
    {"work-dir", "w", 0}, {"available-processors", "p", 0}, {"memory", "m", 0}, {"continue", "c", 1}, {"force", nullptr, 1},
    {"verbose", "v", 1}, {"help", "h", 1}, {"tool", "t", 0}, {"device", nullptr, 0}, {"capacity-hint", nullptr, 0}, {"parse", nullptr, 0},
    {"kmers-io", nullptr, 0}, {"render", nullptr, 0},
};

// --tool seq-cov: its parameters (SequenceCoverage.java:30-72) and the launch options
const OptSpec SEQ_COV_SPECS[] = {
    {"k", "k", 0}, {"from-before", nullptr, 2}, {"from-donor", nullptr, 2}, {"from-both", nullptr, 2}, {"itself", nullptr, 2},
    {"read-file", "r", 0}, {"output-dir", "o", 0}, {"hash", nullptr, 0},
    {"work-dir", "w", 0}, {"available-processors", "p", 0}, {"memory", "m", 0}, {"continue", "c", 1}, {"force", nullptr, 1},
    {"verbose", "v", 1}, {"help", "h", 1}, {"tool", "t", 0}, {"device", nullptr, 0}, {"capacity-hint", nullptr, 0}, {"parse", nullptr, 0},
};

// --tool recipient-visualiser: its parameters (RecipientVisualiser.java:42-92) and the launch options
const OptSpec RECIPIENT_SPECS[] = {
    {"k", "k", 0}, {"after-files", "after", 2}, {"seq", "seq", 0}, {"maxkmers", nullptr, 0}, {"maxradius", nullptr, 0}, {"hash", nullptr, 0},
    {"output-dir", "o", 0}, {"input-dir", "i", 0}, {"ext", "ext", 0},
    {"work-dir", "w", 0}, {"available-processors", "p", 0}, {"memory", "m", 0}, {"continue", "c", 1}, {"force", nullptr, 1},
    {"verbose", "v", 1}, {"help", "h", 1}, {"tool", "t", 0}, {"device", nullptr, 0}, {"devices", nullptr, 0}, {"capacity-hint", nullptr, 0}, {"compact", nullptr, 0}, {"parse", nullptr, 0},
};

// --tool fmt-visualizer: its parameters (FMTVisualizer.java:39-85) and the launch options
const OptSpec FMT_SPECS[] = {
    {"k", "k", 0}, {"donor-files", "donor", 2}, {"before-files", "before", 2}, {"after-files", "after", 2}, {"hash", nullptr, 0},
    {"output-dir", "o", 0}, {"input-dir", "i", 0}, {"ext", "ext", 0},
    {"work-dir", "w", 0}, {"available-processors", "p", 0}, {"memory", "m", 0}, {"continue", "c", 1}, {"force", nullptr, 1},
    {"verbose", "v", 1}, {"help", "h", 1}, {"tool", "t", 0}, {"device", nullptr, 0}, {"devices", nullptr, 0}, {"capacity-hint", nullptr, 0}, {"compact", nullptr, 0}, {"parse", nullptr, 0},
};

// --tool environment-assembler-finder: its parameters (EnvironmentAssemblerFinder.java:33-122) and the launch options
const OptSpec ASSEMBLER_SPECS[] = {
    {"k", "k", 0}, {"reads", "i", 2}, {"seq", nullptr, 0}, {"output", "o", 0}, {"maxkmers", nullptr, 0}, {"maxradius", nullptr, 0},
    {"coverage", nullptr, 0}, {"bothdirs", nullptr, 1}, {"chunklength", nullptr, 0}, {"forcehash", nullptr, 1}, {"hash", nullptr, 0},
    {"threads", nullptr, 0}, {"trim", nullptr, 1}, {"procfiltration", "pf", 0}, {"assembler", nullptr, 0}, {"assemblerpath", nullptr, 0},
    {"work-dir", "w", 0}, {"available-processors", "p", 0}, {"memory", "m", 0}, {"continue", "c", 1}, {"force", nullptr, 1},
    {"verbose", "v", 1}, {"help", "h", 1}, {"tool", "t", 0}, {"device", nullptr, 0}, {"devices", nullptr, 0}, {"capacity-hint", nullptr, 0}, {"compact", nullptr, 0}, {"parse", nullptr, 0}, {"trim-on", nullptr, 0},
};

struct SpecTable {
    const OptSpec *b, *e;
};

// the tool a command line names (the last -t / --tool wins, as every option's last value does): it decides the parameter table
std::string tool_of(int argc, char **argv)
{
    std::string tool = "environment-finder";
    for (int i = 1; i < argc; i++) {
        const std::string tok = argv[i];
        if ((tok == "-t" || tok == "--tool") && i + 1 < argc) tool = argv[++i];
        else if (tok.rfind("--tool=", 0) == 0) tool = tok.substr(7);
    }
    return tool;
}

const OptSpec *find_spec(SpecTable t, const std::string &tok)
{
    for (const OptSpec *p = t.b; p != t.e; p++) {
        const OptSpec &s = *p;
        if (tok == std::string("--") + s.name) return &s;
        if (s.shortopt && tok == std::string("-") + s.shortopt) return &s;
    }
    return nullptr;
}

bool java_bool(const std::string &s)  // new Boolean(String): true iff equalsIgnoreCase("true")
{
    return s.size() == 4 && tolower(s[0]) == 't' && tolower(s[1]) == 'r' && tolower(s[2]) == 'u' && tolower(s[3]) == 'e';
}

long long parse_int(const std::string &name, const std::string &v)
{
    char *end = nullptr;
    errno = 0;
    const long long x = strtoll(v.c_str(), &end, 10);
    if (errno || end == v.c_str() || *end) throw Error("Can't convert value '" + v + "' of parameter '" + name + "' to type 'Integer'");
    return x;
}

Options parse_args(int argc, char **argv)
{
    const std::string tool = tool_of(argc, argv);
    const SpecTable specs = tool == "reads-classifier"          ? SpecTable{std::begin(CLASSIFIER_SPECS), std::end(CLASSIFIER_SPECS)}
                            : tool == "triple-reads-classifier" ? SpecTable{std::begin(TRIPLE_SPECS), std::end(TRIPLE_SPECS)}
                            : tool == "seq-cov"                 ? SpecTable{std::begin(SEQ_COV_SPECS), std::end(SEQ_COV_SPECS)}
                            : tool == "recipient-visualiser"    ? SpecTable{std::begin(RECIPIENT_SPECS), std::end(RECIPIENT_SPECS)}
                            : tool == "environment-assembler-finder" ? SpecTable{std::begin(ASSEMBLER_SPECS), std::end(ASSEMBLER_SPECS)}
                            : tool == "fmt-visualizer"          ? SpecTable{std::begin(FMT_SPECS), std::end(FMT_SPECS)}
                                                                : SpecTable{std::begin(SPECS), std::end(SPECS)};
    std::map<std::string, std::vector<std::string>> got;
    for (int i = 1; i < argc; i++) {
        std::string tok = argv[i], inline_val;
        bool has_inline = false;
        const size_t eq = tok.find('=');
        if (tok.rfind("--", 0) == 0 && eq != std::string::npos) {  // --opt=value
            inline_val = tok.substr(eq + 1);
            tok = tok.substr(0, eq);
            has_inline = true;
        }
        const OptSpec *s = find_spec(specs, tok);
        if (!s) throw Error("Cannot parse command line: Unrecognized option: " + tok);
        auto &vals = got[s->name];
        vals.clear();
        if (has_inline) {
            vals.push_back(inline_val);
        } else if (s->kind == 2) {
            while (i + 1 < argc && !find_spec(specs, argv[i + 1]) && argv[i + 1][0] != '-') vals.push_back(argv[++i]);
        } else if (s->kind == 1) {
            if (i + 1 < argc && argv[i + 1][0] != '-') vals.push_back(argv[++i]);
            else vals.push_back("true");  // option without an argument, itmo!/utils/tool/Tool.java:650-652
        } else {
            if (i + 1 >= argc) throw Error("Cannot parse command line: Missing argument for option: " + tok);
            vals.push_back(argv[++i]);
        }
    }
    Options o;
    auto val = [&](const char *n) -> const std::string * { auto it = got.find(n); return it == got.end() || it->second.empty() ? nullptr : &it->second[0]; };
    if (auto v = val("k")) o.k = (int)parse_int("k", *v);
    auto multi = [&](const char *name, std::vector<std::string> &dst) {
        if (!got.count(name)) return;
        for (const std::string &v : got[name]) {  // arrays are re-tokenised on "[, ]" (Tool.java:888-895)
            std::string cur;
            for (char c : v + " ") {
                if (c == '[' || c == ',' || c == ' ' || c == ']') { if (!cur.empty()) dst.push_back(cur); cur.clear(); }
                else cur.push_back(c);
            }
        }
    };
    multi("reads", o.reads);
    multi("env", o.env);
    multi("input-files", o.input_files);
    multi("read-files", o.read_files);
    multi("from-before", o.from_before);
    multi("from-donor", o.from_donor);
    multi("from-both", o.from_both);
    multi("itself", o.itself);
    multi("after-files", o.after_files);
    multi("donor-files", o.donor_files);
    multi("before-files", o.before_files);
    if (auto v = val("available-processors")) o.processors = (int)parse_int("available-processors", *v);
    if (auto v = val("input-dir")) o.input_dir = *v;
    if (auto v = val("ext")) o.ext = *v;
    if (auto v = val("read-file")) o.read_file = *v;
    if (auto v = val("correction")) o.correction = java_bool(*v);
    if (auto v = val("interval95")) o.interval95 = java_bool(*v);
    if (auto v = val("found-threshold")) o.found_threshold = parse_int("found-threshold", *v);
    multi("input-kmers-1", o.input_kmers_1);
    multi("input-kmers-2", o.input_kmers_2);
    if (auto v = val("k2")) o.k2 = (int)parse_int("k2", *v);
    if (auto v = val("half-threshold")) o.half_threshold = parse_int("half-threshold", *v);
    if (auto v = val("procfiltration")) o.procfiltration = parse_int("procfiltration", *v);
    if (auto v = val("threads")) (void)parse_int("threads", *v);  // (accepted, unused: the filter is one launch a batch)
    if (auto v = val("assembler")) o.assembler = *v;
    if (auto v = val("assemblerpath")) o.assemblerpath = *v;
    if (auto v = val("compact")) {
        if (*v != "host" && *v != "gpu" && *v != "auto") throw Error("--compact takes host, gpu or auto, not '" + *v + "'");
        o.compact = *v;
        o.compact_given = true;
    }
    if (auto v = val("join")) {
        if (*v != "host" && *v != "gpu" && *v != "auto") throw Error("--join takes host, gpu or auto, not '" + *v + "'");
        o.join = *v;
        o.join_given = true;
    }
    if (auto v = val("parse")) {
        if (*v != "host" && *v != "gpu" && *v != "auto") throw Error("--parse takes host, gpu or auto, not '" + *v + "'");
        o.parse = *v;
        o.parse_given = true;
    }
    if (auto v = val("trim-on")) {
        if (*v != "host" && *v != "gpu" && *v != "auto") throw Error("--trim-on takes host, gpu or auto, not '" + *v + "'");
        o.trim_on = *v;
        o.trim_on_given = true;
    }
    if (auto v = val("kmers-io")) {
        if (*v != "host" && *v != "gpu" && *v != "auto") throw Error("--kmers-io takes host, gpu or auto, not '" + *v + "'");
        o.kmers_io = *v;
        o.kmers_io_given = true;
    }
    if (auto v = val("render")) {
        if (*v != "host" && *v != "gpu" && *v != "auto") throw Error("--render takes host, gpu or auto, not '" + *v + "'");
        o.render = *v;
        o.render_given = true;
    }
    if (auto v = val("seq")) o.seq = *v;
    if (auto v = val("hicseq")) o.hicseq = *v;
    if (auto v = val("output")) o.output = *v;
    if (auto v = val("maxkmers")) o.maxkmers = parse_int("maxkmers", *v);
    if (auto v = val("maxradius")) o.maxradius = parse_int("maxradius", *v);
    if (auto v = val("coverage")) o.coverage = (int)parse_int("coverage", *v);
    if (auto v = val("chunklength")) o.chunklength = (int)parse_int("chunklength", *v);
    if (auto v = val("bothdirs")) o.bothdirs = java_bool(*v);
    if (auto v = val("forcehash")) o.forcehash = java_bool(*v);
    if (auto v = val("trim")) o.trim = java_bool(*v);
    if (auto v = val("merge")) o.merge = java_bool(*v);
    if (auto v = val("continue")) o.cont = java_bool(*v);
    if (auto v = val("force")) o.force = java_bool(*v);
    if (auto v = val("verbose")) g_verbose = java_bool(*v);
    if (auto v = val("help")) o.help = java_bool(*v);
    if (auto v = val("hash")) o.hash = *v;
    if (auto v = val("work-dir")) o.work_dir = *v;
    if (auto v = val("tool")) o.tool = *v;
    if (auto v = val("output-dir")) o.output_dir = *v;
    if (auto v = val("geneid")) o.geneid = (int)parse_int("geneid", *v);
    if (auto v = val("device")) o.device = (int)parse_int("device", *v);
    if (auto v = val("capacity-hint")) o.capacity_hint = (unsigned long long)parse_int("capacity-hint", *v);
    if (auto v = val("devices")) {  // "0,1,2" or "0-7"
        const std::string &d = *v;
        const size_t dash = d.find('-');
        if (dash != std::string::npos && d.find(',') == std::string::npos) {
            const long long a = parse_int("devices", d.substr(0, dash)), b = parse_int("devices", d.substr(dash + 1));
            for (long long i = a; i <= b; i++) o.devices.push_back((int)i);
        } else {
            size_t at = 0;
            while (at <= d.size()) {
                const size_t comma = d.find(',', at);
                const std::string tok = d.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
                if (!tok.empty()) o.devices.push_back((int)parse_int("devices", tok));
                if (comma == std::string::npos) break;
                at = comma + 1;
            }
        }
        if (o.devices.empty() || o.devices.size() > 64) throw Error("--devices: give 1 to 64 GPU ordinals, e.g. 0,1,2,3 or 0-7");
    }
    return o;
}

void usage()
{
    puts("MetaCherchant: genomic environment analysis tool (MI355X-native environment-finder path)\n");
    puts("Usage:     metacherchant [<Launch options>] [<Input parameters>]\n");
    puts("Input parameters of --tool environment-finder:");
    puts("  -k, --k <arg>            k-mer size (MANDATORY)");
    puts("  -i, --reads <args>       FASTQ, FASTA reads");
    puts("      --seq <arg>          FASTA file with sequences (MANDATORY)");
    puts("      --hicseq <arg>       FASTA file with Hi-C sequences");
    puts("  -o, --output <arg>       output directory (MANDATORY)");
    puts("      --maxkmers <arg>     maximum number of k-mers in created subgraph");
    puts("      --maxradius <arg>    maximum distance in k-mers from starting gene");
    puts("      --coverage <arg>     minimum depth of k-mers to consider (default 1)");
    puts("      --bothdirs [<arg>]   run graph search in both directions from starting sequence (default false)");
    puts("      --chunklength <arg>  minimum node length for BLAST search (default 1)");
    puts("      --forcehash [<arg>]  force k-mer hashing (even for k <= 31) (default false)");
    puts("      --hash <arg>         hash function to use: poly or fnv1a (default poly)");
    puts("      --trim [<arg>]       trim all not maximal paths? (default false)");
    puts("      --merge [<arg>]      draw single environment for multiple input sequences? (default false)");
    puts("Input parameters of --tool environment-finder-multi: -e/--env <graph.txt files>, --seq, -o/--output, -g/--geneid (default 1),");
    puts("  --join host|gpu|auto (who joins the graphs and compacts the result; the files are the same.  host: on k-mer strings, as the");
    puts("  reference does; gpu: on packed k-mers with mc_env_join and mc_unitigs on --device; auto, the default: the GPU from 100000");
    puts("  k-mers on, the smallest size measured at which it wins, and whenever the packed form holds the input; else the host)");
    puts("Input parameters of --tool kmer-counter: -k, -i/--reads, --hash, --output-dir <dir> (default <work-dir>/kmers)");
    puts("Input parameters of --tool reads-classifier (splits the reads of -r into found / not found in the graph of -i):");
    puts("  -k, --k <arg>                  k-mer size (MANDATORY)");
    puts("  -i, --input-files <args>       reads for the de Bruijn graph, or its <name>.kmers.bin from kmer-counter (MANDATORY)");
    puts("  -r, --read-files <args>        one FASTQ / FASTA file of reads to classify, or two of paired reads (MANDATORY)");
    puts("  -o, --output-dir <arg>         directory of found_{1,2,s}.fastq, not_found_{1,2,s}.fastq (default <work-dir>/reads_classifier)");
    puts("  -corr, --correction [<arg>]    try the four bases at a read's one low-quality position (default false)");
    puts("      --hash <arg>               hash function to use for k > 31: poly or fnv1a (default poly)");
    puts("      --interval95 [<arg>]       set the interval width to probability 0.95 (default false)");
    puts("  -found, --found-threshold <arg>  minimum coverage breadth for class `found`, 0 - 100 % (default 90)");
    puts("Input parameters of --tool triple-reads-classifier (splits the pairs of -r into found / half found / not found with two k):");
    puts("  -k, --k <arg>                  k-mer size of the first graph (MANDATORY)");
    puts("  -k2, --k2 <arg>                k-mer size of the second graph, k2 > k (MANDATORY)");
    puts("  -i, --input-files <args>       reads for both de Bruijn graphs (unless -ik1 / -ik2 give them)");
    puts("  -ik1, --input-kmers-1 <args>   the first graph as <name>.kmers.bin from kmer-counter at k");
    puts("  -ik2, --input-kmers-2 <args>   the second graph as <name>.kmers.bin from kmer-counter at k2");
    puts("  -r, --read-files <args>        two FASTQ / FASTA files of paired reads to classify (MANDATORY)");
    puts("  -o, --output-dir <arg>         directory of the nine {found,half_found,not_found}_{1,2,s}.fastq (default <work-dir>/reads_classifier)");
    puts("  -corr, --correction [<arg>]    try the four bases at a read's one low-quality position (default false)");
    puts("      --hash <arg>               hash function to use for k > 31: poly or fnv1a (default poly)");
    puts("      --interval95 [<arg>]       set the interval width to probability 0.95 (default false)");
    puts("  -found, --found-threshold <arg>  minimum coverage breadth for class `found`, 0 - 100 % (default 90)");
    puts("  -half, --half-threshold <arg>  minimum coverage breadth for class `half-found`, 0 - 100 % (default 40)");
    puts("Input parameters of --tool seq-cov (depth and breadth of every sequence's k-mers in four bins of reads; writes seq_cov.csv):");
    puts("  -k, --k <arg>                  k-mer size (MANDATORY)");
    puts("      --from-before <args>       reads of the came_from_before bin (MANDATORY)");
    puts("      --from-donor <args>        reads of the came_from_donor bin (MANDATORY)");
    puts("      --from-both <args>         reads of the came_from_both bin (MANDATORY)");
    puts("      --itself <args>            reads of the came_itself bin (MANDATORY)");
    puts("  -r, --read-file <arg>          file with sequences to classify: reads, genes or contigs (MANDATORY)");
    puts("  -o, --output-dir <arg>         directory of seq_cov.csv (default <work-dir>/sequence_coverage)");
    puts("      --hash <arg>               hash function to use for k > 31: poly or fnv1a (default poly)");
    puts("Input parameters of --tool recipient-visualiser (one coloured GFA a sequence: its environment in the post-FMT graph, every k-mer");
    puts("coloured by the class files of the reads-classifier script that hold it; writes <output-dir>/after/comp_<i>{.gfa,_seqs.fasta}):");
    puts("  -k, --k <arg>                  k-mer size (MANDATORY)");
    puts("  -after, --after-files <args>   post-FMT recipient metagenomic reads (MANDATORY)");
    puts("  -seq, --seq <arg>              FASTA file with sequences (MANDATORY)");
    puts("      --maxkmers <arg>           maximum number of k-mers in created subgraph");
    puts("      --maxradius <arg>          maximum distance in k-mers from starting gene (default 1000)");
    puts("      --hash <arg>               hash function to use for k > 31: poly or fnv1a (default poly)");
    puts("  -o, --output-dir <arg>         output directory (default <work-dir>/graph)");
    puts("  -i, --input-dir <arg>          directory of came_from_{donor,baseline,both}_{1,2,s}.<ext> and came_itself_{1,2,s}.<ext> (MANDATORY)");
    puts("  -ext, --ext <arg>              extension of those files (MANDATORY)");
    puts("Input parameters of --tool fmt-visualizer (one coloured GFA a connected component of the donor, the pre-FMT and the post-FMT graph, every");
    puts("k-mer coloured by the class files that hold it; writes <output-dir>/{donor,before,after}/comp<N>{.gfa,_seqs.fasta}):");
    puts("  -k, --k <arg>                  k-mer size (MANDATORY)");
    puts("  -donor, --donor-files <args>   donor metagenomic reads (MANDATORY)");
    puts("  -before, --before-files <args> pre-FMT recipient metagenomic reads (MANDATORY)");
    puts("  -after, --after-files <args>   post-FMT recipient metagenomic reads (MANDATORY)");
    puts("      --hash <arg>               hash function to use for k > 31: poly or fnv1a (default poly)");
    puts("  -o, --output-dir <arg>         output directory (default <work-dir>/graph)");
    puts("  -i, --input-dir <arg>          directory of {settle,not_settle,stay,gone,came_from_*,came_itself}_{1,2,s}.<ext> (MANDATORY)");
    puts("  -ext, --ext <arg>              extension of those files (MANDATORY)");
    puts("  -p, --available-processors <n> threads that replay the components' walks");
    puts("Input parameters of --tool environment-assembler-finder (the environment of ONE sequence, then the reads of every -i file that belong");
    puts("to it as <output>/cutReads<i>.fasta; with --assembler, their assembly and the environment again, at k = 55, in the contigs):");
    puts("  -k, --k <arg>                  k-mer size (MANDATORY)");
    puts("  -i, --reads <args>             FASTQ, FASTA reads");
    puts("      --seq <arg>                FASTA file with the sequence (MANDATORY)");
    puts("  -o, --output <arg>             output directory (MANDATORY)");
    puts("      --maxkmers, --maxradius, --coverage, --bothdirs, --chunklength, --forcehash, --hash, --trim: as for environment-finder");
    puts("      --threads <arg>            accepted, unused");
    puts("  -pf, --procfiltration <arg>    a read is kept when this percentage of its k-mers is in the environment, at least one (default 1)");
    puts("      --assembler <arg>          spades or megahit: assemble every cutReads<i> (without it the tool ends after the filter)");
    puts("      --assemblerpath <arg>      directory of spades.py / megahit");
    puts("Launch options: -w/--work-dir <dir> (default workDir), -c/--continue, --force, -v/--verbose, -h/--help,");
    puts("                -t/--tool <name>, -p/--available-processors <n> and -m/--memory <arg> (accepted, unused),");
    puts("                --device <n> (GPU ordinal), --devices <a,b,...|a-b> (several GPUs as one table: reads dealt to them,");
    puts("                k-mers exchanged by owner over xGMI, BFS on the first), --capacity-hint <distinct k-mers>");
    puts("                (sizes the table once; with -k 33..63 every batch then travels as super-k-mer records, not only the first)");
    puts("                --compact host|gpu|auto (environment-finder, environment-assembler-finder, recipient-visualiser, fmt-visualizer:");
    puts("                who compacts an environment's k-mers into unitigs; the files are the same; default auto: the GPU from");
    puts("                10000 k-mers on, the smallest size measured, where it already wins; the host below)");
    puts("                --trim-on host|gpu|auto (environment-finder, environment-assembler-finder: who works out which k-mers --trim keeps.");
    puts("                host: the reverse walk over the pass's hash map; gpu: mc_trim_paths on the tool's context, every pass; the files are");
    puts("                the same; default auto: the GPU for a pass of 10000 k-mers or more, the smallest size measured, where it already wins;");
    puts("                it does nothing without --trim; with --devices auto is host and gpu is refused)");
    puts("                --parse host|gpu|auto (the classifiers, seq-cov, fmt-visualizer, environment-assembler-finder: who parses the whole reads of");
    puts("                -r / --read-file / the read filter.  host: one thread reads the records and the tool packs them; gpu: the text of an");
    puts("                uncompressed FASTA / FASTQ file is tokenised on the device and stays there for the kernels; the files are the same;");
    puts("                default auto: gpu for an uncompressed file of 31.6 MB or more, the smallest size measured, where it already wins)");
    puts("                --render host|gpu|auto (reads-classifier, triple-reads-classifier: who turns the reads of the output files into FASTQ text.");
    puts("                host: a record and a base at a time; gpu: mc_render_fastq renders every file's records of a batch in one call and each");
    puts("                file takes them with one write; the files are the same; default auto: the GPU only for reads --parse gpu has already");
    puts("                taken to the device, from the measured size on at which the whole tool wins: a first -r file of 31.6 MB for the triple");
    puts("                classifier, of 3.16 GB for reads-classifier; the host otherwise)");
    puts("                --kmers-io host|gpu|auto (kmer-counter, reads-classifier, triple-reads-classifier: who turns the table into the records");
    puts("                of <name>.kmers.bin and such a file's records into (key, count) pairs.  host: one thread, byte by byte; gpu: kernels on");
    puts("                --device, the file streamed in chunks beside them (the records then come in the order of the table's slots); the files");
    puts("                hold the same records; default auto: the GPU for a save of 10^7 keys or more and a load of 10^4 records or more, from where it was measured to win)");
}

#define MC_CHECK(ctx, call)                                                       \
    do {                                                                          \
        const int rc_ = (call);                                                   \
        if (rc_ != MC_OK) throw Error(std::string(mc_last_error(ctx)));           \
    } while (0)

struct CtxGuard {
    mc_ctx *c = nullptr;
    ~CtxGuard() { mc_destroy(c); }
};

// buildEnvironment (src/algo/OneSequenceCalculator.java:137-144): the passes of one calculator
std::vector<int> pass_dirs(bool bothdirs) { return bothdirs ? std::vector<int>{0} : std::vector<int>{-1, 1}; }

// work dir: log files, in.properties / SUCCESS (itmo!/utils/tool/Tool.java:31-33,318-392,666-689).
// Returns false when --continue finds the tool finished already.
bool open_work_dir(const Options &o, const std::string &props)
{
    const std::string wd = o.work_dir;
    write_file(wd + "/logs/.keep", "");
    char ts[32];
    const time_t now = time(nullptr);
    strftime(ts, sizeof ts, "%Y.%m.%d_%H.%M.%S", localtime(&now));
    g_log = fopen((wd + "/log").c_str(), "w");
    g_log2 = fopen((wd + "/logs/log_" + ts).c_str(), "w");
    struct stat st;
    if (stat((wd + "/in.properties").c_str(), &st) == 0 && !o.force && !o.cont)
        logline("WARN", "Work directory " + wd + " holds a previous run; overwriting (the reference would prompt; pass --force to silence)");
    if (o.cont && stat((wd + "/SUCCESS").c_str(), &st) == 0) {
        info("Tool " + o.tool + " already finished in " + wd + " (--continue), nothing to do");
        return false;
    }
    remove((wd + "/SUCCESS").c_str());
    write_file(wd + "/in.properties", props);
    return true;
}

// One table on one GPU (mc_*), or on several (mc_group_*: --devices): the calls environment-finder makes
struct Engine {
    mc_ctx *c = nullptr;
    mc_group *g = nullptr;
    ~Engine() { if (g) mc_group_destroy(g); else mc_destroy(c); }
    void open(const mc_config &cfg, const std::vector<int> &devices)
    {
        if (devices.empty()) {
            if (mc_create(&cfg, &c) != MC_OK) throw Error(std::string(mc_last_error(nullptr)));
        } else {
            std::vector<int32_t> d(devices.begin(), devices.end());
            if (mc_group_create(&cfg, d.data(), (uint32_t)d.size(), &g) != MC_OK) throw Error(std::string(mc_group_last_error(nullptr)));
        }
    }
    void check(int rc) const { if (rc != MC_OK) throw Error(std::string(g ? mc_group_last_error(g) : mc_last_error(c))); }
    void set_coverage_hint(int cov) { check(g ? mc_group_set_coverage_hint(g, cov) : mc_set_coverage_hint(c, cov)); }
    void add_reads_file(const std::string &path, uint64_t *n) { check(g ? mc_group_add_reads_file(g, path.c_str(), n) : mc_add_reads_file(c, path.c_str(), n)); }
    void finalize(uint64_t *n) { check(g ? mc_group_finalize_counts(g, n) : mc_finalize_counts(c, n)); }
    void bfs_batch(const mc_bfs_job *jobs, uint32_t n, int cov, int64_t mk, int64_t mr, mc_bfs_result *out)
    {
        check(g ? mc_group_bfs_batch(g, jobs, n, cov, mk, mr, out) : mc_bfs_batch(c, jobs, n, cov, mk, mr, out));
    }
};

// --compact: the unitig compaction of an environment on the host (Environment::create_picture's loop on labels), on the GPU (mc_unitigs
// on a context of the run; the host then only runs the loop over the entries of irregular chains), or `auto`, the default: on the GPU
// from COMPACT_AUTO_MIN k-mers on.  That is the smallest size scripts/unitigs_bench.py has timed, and there the GPU's way already
// takes less than half the host's time, as at every larger size; nobody has measured below it, so the host keeps those.
constexpr size_t COMPACT_AUTO_MIN = 10000;
struct Compaction {
    std::string mode;
    const Options &o;
    int k;
    mc_ctx *ctx = nullptr;
    CtxGuard own;  // (a group has no context of its own to lend: one more, with an empty table, on the first device, when first needed)
    Compactor gpu;
    std::mutex mu;
    Compaction(const Options &o, const Engine &e, int k) : mode(o.compact), o(o), k(k), ctx(e.c) {}
    // the compactor for an environment of n k-mers (NULL: the host's loop), named in the log
    const Compactor *pick(size_t n, const std::string &what)
    {
        const bool on_gpu = mode == "gpu" || (mode == "auto" && n >= COMPACT_AUTO_MIN);
        std::lock_guard<std::mutex> g(mu);
        info("Compacting " + what + " (" + std::to_string(n) + " k-mers) on the " + (on_gpu ? "GPU (mc_unitigs)" : "host"));
        if (!on_gpu) return nullptr;
        if (!gpu) {
            if (!ctx) {
                mc_config cfg{};
                cfg.k = k;
                cfg.key_mode = MC_KEY_POLY;
                cfg.device = o.devices.empty() ? o.device : o.devices[0];
                if (mc_create(&cfg, &own.c) != MC_OK) throw Error(std::string(mc_last_error(nullptr)));
                ctx = own.c;
            }
            gpu = gpu_compactor(ctx);
        }
        return &gpu;
    }
};

// --trim-on: which k-mers of a pass --trim keeps, by the host's reverse walk (Environment::add_pass) or by mc_trim_paths on the tool's
// context; `auto`, the default, takes the GPU from TRIM_AUTO_MIN k-mers in a pass on.
// That is the smallest size scripts/trim_paths_bench.py has timed (10^4 to 10^7 k-mers, k = 31 and 63, dir +1 and 0, medians of 5):
// there the GPU's way -- the call with its copies, then the removals by its mask -- takes 0.28 .. 0.41 ms against the host walk's
// 1.9 .. 6.1 ms, and the gap only widens (10^6: 2.0 .. 18 ms against 0.41 .. 1.04 s), each time by far more than the host figures'
// own spread.  Nobody has measured below it, so the host keeps those; with --devices (no single context) auto is host.
constexpr size_t TRIM_AUTO_MIN = 10000;
struct Trimmer {
    const Options &o;
    mc_ctx *ctx;  // (NULL: a group)
    Trimmer(const Options &o, const Engine &e) : o(o), ctx(e.c) {}
    // add_pass with the pass's mask where the GPU makes it
    void add_pass(Environment &env, const BfsPass &p, const mc_bfs_result &r) const
    {
        const bool on_gpu = o.trim && ctx && (o.trim_on == "gpu" || (o.trim_on == "auto" && r.n >= TRIM_AUTO_MIN));
        if (!on_gpu) {
            env.add_pass(p, o.trim);
            return;
        }
        std::vector<uint8_t> kept(r.n);
        double ms = 0;
        MC_CHECK(ctx, mc_trim_paths(ctx, r.hi, r.lo, r.last, r.n, p.dir, kept.data(), &ms));
        info("Trimmed a pass of " + std::to_string(r.n) + " k-mers on the GPU (mc_trim_paths)");
        env.add_pass(p, true, &kept);
    }
};

// --kmers-io: the records of a <name>.kmers.bin by the host's loops (mc_save_kmers, mc_load_kmers) or by the kernels of csrc/kmers_bin.hip
// with the file streamed in chunks beside them (mc_save_kmers_gpu, mc_load_kmers_gpu); `auto`, the default, takes the GPU from
// KMERS_SAVE_AUTO_MIN keys in the table for a save, from KMERS_LOAD_AUTO_MIN records in the file for a load.
// Each is the smallest size at which scripts/kmers_bin_bench.py (tables of 10^4 to 10^8 random keys, k = 31 and 63, medians of 5 runs, the
// two ways in turn; profiles/kmers_bin_bench.txt) found the GPU way's median below the host way's FASTEST run, there and at
// every larger size.  The save: the host's loop is the faster one up to 10^6 keys (0.32 ms against 1.22 ms at 10^4, 5.9 against 6.4 ms at
// 10^6 of k = 31; at k = 63 the medians cross, 9.8 against 9.0 ms, but the host's fastest run, 6.2 ms, is below: no win) -- the GPU way
// sets up two pinned and two device staging buffers, a stream and a thread a call -- and the slower one from 10^7 on: 76.3 ms (74.3 at
// best) against 45.3 ms, and 833 (795) against 259 ms at 10^8, 798 (757) against 261 ms at k = 63.
// The load: the GPU way wins at every measured size, 8.3 ms against 38.0 (36.7 at best) at 10^4 records, 19.5 against 63.6 (60.1) at
// 10^7, 45 against 236 (222) at 10^8: the host loop sizes and zeroes its 80 MB and 64 + 16 MB vectors whatever the file's length.
// Below the smallest measured size (10^4) nothing is measured and `auto` is the host.  File time is the storage's and common to both ways.
constexpr uint64_t KMERS_SAVE_AUTO_MIN = 10000000, KMERS_LOAD_AUTO_MIN = 10000;
bool kmers_on_gpu(const Options &o, uint64_t records, uint64_t auto_min)
{
    return o.kmers_io == "gpu" || (o.kmers_io == "auto" && records >= auto_min);
}

// IOUtils.loadKmers of one file (threshold 0) into the table
void load_kmers_file(const Options &o, mc_ctx *ctx, const std::string &path)
{
    struct stat st;
    const uint64_t records = stat(path.c_str(), &st) == 0 ? (uint64_t)st.st_size / 10 : 0;
    const bool on_gpu = kmers_on_gpu(o, records, KMERS_LOAD_AUTO_MIN);
    info("Loading " + std::to_string(records) + " k-mer records on the " + (on_gpu ? "GPU (mc_load_kmers_gpu)" : "host (mc_load_kmers)"));
    MC_CHECK(ctx, on_gpu ? mc_load_kmers_gpu(ctx, path.c_str(), 0, nullptr, nullptr) : mc_load_kmers(ctx, path.c_str(), 0, nullptr, nullptr));
}

// the reads of all --reads files into the table; returns hm.size()
uint64_t load_reads(const std::vector<std::string> &files, Engine &e)
{
    for (const std::string &path : files) {
        const size_t slash = path.find_last_of('/');
        info("Loading file " + (slash == std::string::npos ? path : path.substr(slash + 1)) + "...");
        uint64_t n = 0;
        e.add_reads_file(path, &n);
        info(group_digits(n) + " reads added");
    }
    uint64_t n_distinct = 0;
    e.finalize(&n_distinct);
    info("Hashtable size: " + std::to_string(n_distinct) + " kmers");
    return n_distinct;
}

// --tool kmer-counter (src/tools/KmersCounter.java:56-121): count, then <name>.kmers.bin + <name>.stat.txt
int run_kmer_counter(const Options &o)
{
    if (o.k < 0) throw Error("Parameter 'k' is mandatory");
    if (o.reads.empty()) throw Error("Parameter 'reads' is mandatory");
    if (!open_work_dir(o, "k=" + std::to_string(o.k) + "\n")) return 0;
    const std::string out_dir = o.output_dir.empty() ? o.work_dir + "/kmers" : o.output_dir;
    int mode = MC_KEY_PACKED;
    if (o.k > 31) {  // (no --forcehash here: KmersCounter.java:59-69)
        info("Reading hashes of k-mers instead");
        std::string h = o.hash;
        for (char &c : h) c = (char)tolower((unsigned char)c);
        if (h == "fnv1a") { info("Using FNV1a hash function"); mode = MC_KEY_FNV1A; }
        else { info("Using default polynomial hash function"); mode = MC_KEY_POLY; }
    }
    mc_config cfg{};
    cfg.k = o.k;
    cfg.key_mode = mode;
    cfg.device = o.device;
    cfg.capacity_hint = o.capacity_hint;
    if (!o.devices.empty()) throw Error("--devices is for --tool environment-finder: kmer-counter writes one device's table (--device)");
    Engine E;
    E.open(cfg, {});
    mc_ctx *ctx = E.c;
    const uint64_t size = load_reads(o.reads, E);
    // ReadersUtils.readDnaLazy(file).name(): the first file's name without its format extension
    std::string name = o.reads[0];
    const size_t slash = name.find_last_of('/');
    if (slash != std::string::npos) name = name.substr(slash + 1);
    {
        std::string low = name;
        for (char &c : low) c = (char)tolower((unsigned char)c);
        for (const char *ext : {".fasta.gz", ".fa.gz", ".fn.gz", ".fna.gz", ".fastq.gz", ".fq.gz", ".fasta.bz2", ".fa.bz2", ".fn.bz2", ".fna.bz2",
                                ".fastq.bz2", ".fq.bz2", ".fasta", ".fa", ".fn", ".fna", ".fastq", ".fq", ".binq"}) {
            const size_t n = strlen(ext);
            if (low.size() >= n && low.compare(low.size() - n, n, ext) == 0) { name.resize(name.size() - n); break; }
        }
    }
    const std::string bin = out_dir + "/" + name + ".kmers.bin", st = out_dir + "/" + name + ".stat.txt";
    write_file(out_dir + "/.keep", "");
    remove((out_dir + "/.keep").c_str());
    logline("DEBUG", "Starting to print k-mers to " + bin);
    uint64_t total = 0, good = 0;
    const bool on_gpu = kmers_on_gpu(o, size, KMERS_SAVE_AUTO_MIN);
    info("Writing " + std::to_string(size) + " k-mer records on the " + (on_gpu ? "GPU (mc_save_kmers_gpu)" : "host (mc_save_kmers)"));
    MC_CHECK(ctx, on_gpu ? mc_save_kmers_gpu(ctx, bin.c_str(), st.c_str(), 0, &total, &good) : mc_save_kmers(ctx, bin.c_str(), st.c_str(), 0, &total, &good));
    char pct[32];
    if (size) snprintf(pct, sizeof pct, "%.1f", good * 100.0 / (double)size);
    else snprintf(pct, sizeof pct, "NaN");  // (Java's String.format of 0.0 / 0)
    info(group_digits(size) + " k-mers found, " + group_digits(good) + " (" + pct + "%) of them is good (not erroneous)");
    if (size == 0) logline("WARN", "No k-mers found in reads! Perhaps you reads file is empty or k-mer size is too big");
    else if (good == 0 || good < (uint64_t)((double)size * 0.03))
        logline("WARN", "Too few good k-mers were found! Perhaps you should decrease k-mer size or --maximal-bad-frequency value");
    if (o.k <= 31) {
        const uint64_t all = (1ull << (2 * o.k)) / 2;  // (4^k)/2
        if (size == all) logline("WARN", "All possible k-mers were found in reads! Perhaps you should increase k-mer size");
        else if (size >= (uint64_t)((double)all * 0.99))
            logline("WARN", "Almost all possible k-mers were found in reads! Perhaps you should increase k-mer size");
    }
    info("k-mers printed to " + bin);
    write_file(o.work_dir + "/SUCCESS", "");
    return 0;
}

// --tool environment-finder-multi (src/tools/EnvironmentFinderMultiMain.java).  --join: the join of the graph files and the compaction
// on the host on k-mer strings (environment_finder_multi, the reference's way), on the GPU on packed k-mers (mc_env_join and mc_unitigs
// on a context of its own with an empty table), or `auto`, the default: on the GPU from JOIN_AUTO_MIN entries on.  That is the smallest
// size at which scripts/multi_join_bench.py has timed the whole tool faster the GPU's way than on strings (0.34 s against 1.57 s at
// k = 31, 0.46 s against 1.77 s at k = 63, four graphs); at 10 000 entries the GPU's way took 0.27 s, as at 2 000 (a process opens the device and
// creates a context before its first kernel), three times the string path's whole run.
constexpr size_t JOIN_AUTO_MIN = 100000;
struct BelowJoinAutoMin {
    size_t n;
};
int run_multi(const Options &o)
{
    if (o.env.empty()) throw Error("Parameter 'env' is mandatory");
    if (o.seq.empty()) throw Error("Parameter 'seq' is mandatory");
    if (o.output.empty()) throw Error("Parameter 'output' is mandatory");
    if (!o.devices.empty()) throw Error("--devices is for --tool environment-finder: environment-finder-multi joins the graphs on one device (--device)");
    if (!open_work_dir(o, "seq=" + o.seq + "\noutput=" + o.output + "\n")) return 0;
    const std::string joining = "Joining " + std::to_string(o.env.size()) + " environments";
    bool packed = o.join != "host";
    if (o.join == "auto") {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) {
            info(joining + " on the host (k-mer strings): no HIP device is available");
            packed = false;
        }
    } else if (!packed) {
        info(joining + " on the host (k-mer strings)");
    }
    MultiResult r;
    if (packed) {
        CtxGuard own;
        double join_ms = 0, unitigs_ms = 0;
        bool small = false;
        const Joiner join = [&](const EnvJoinInput &in, EnvJoinResult &out) {
            const size_t n = in.entries.size();
            if (o.join == "auto" && n < JOIN_AUTO_MIN) {  // (too few for the GPU: joined here all the same, to hear whether the classes fit; then the compactor ends it)
                small = true;
                env_join_host(in, out);
                return;
            }
            info(joining + " (" + std::to_string(n) + " k-mers) on the GPU (mc_env_join, mc_unitigs)");
            mc_config cfg{};
            cfg.k = in.k;
            cfg.key_mode = MC_KEY_POLY;
            cfg.device = o.device;
            if (mc_create(&cfg, &own.c) != MC_OK) throw Error(std::string(mc_last_error(nullptr)));
            gpu_joiner(own.c, &join_ms)(in, out);
        };
        const Compactor compact = [&](int k, const std::vector<kmer_t> &kmers, const std::vector<uint8_t> &cls, UnitigsResult &out) {
            if (small) throw BelowJoinAutoMin{kmers.size()};
            gpu_compactor(own.c, &unitigs_ms)(k, kmers, cls, out);
        };
        try {
            r = environment_finder_multi_packed(o.env, o.seq, o.geneid, join, compact);
            char ms[96];
            snprintf(ms, sizeof ms, "mc_env_join %.3f ms, mc_unitigs %.3f ms on the device", join_ms, unitigs_ms);
            logline("DEBUG", ms);
        } catch (const MultiUnpacked &e) {
            if (o.join == "gpu") throw Error(std::string("--join gpu: ") + e.what() + " (--join host takes such input)");
            info(joining + " on the host (k-mer strings): " + e.what());
            packed = false;
        } catch (const BelowJoinAutoMin &b) {
            info(joining + " (" + std::to_string(b.n) + " k-mers) on the host (k-mer strings)");
            packed = false;
        }
    }
    if (!packed) r = environment_finder_multi(o.env, o.seq, o.geneid);
    write_multi(r, o.output);
    for (const std::string &l : r.log) logline(l.substr(0, 4).c_str(), l.substr(5));
    write_file(o.work_dir + "/SUCCESS", "");
    return 0;
}

// --tool reads-classifier (src/tools/ReadsClassifier.java:154-200, src/algo/PairFinder.java:32-57): the reads of -r split by how
// well their k-mers are covered in the graph of -i (mc_classify_reads), written to six FASTQ files.  The reference fills its four
// lists from a thread pool, so their order is only defined at -p 1; here it is that order: input order within every list.

// WritersUtils.writeDnaQsToFastqFile (itmo!/io/writers/FastqDedicatedWriter.java:39-60): "@<n>" counting from 1 (DataCounter), the
// bases with N printed as A (the DnaQ holds base 0 there), "+", the qualities as Illumina (phred + 64, Illumina.getPhredChar)
// (FastqOut and SideList: fastq_out.h)

void hip_check(hipError_t e, const char *what)
{
    if (e != hipSuccess) throw Error(std::string(what) + ": " + hipGetErrorString(e));
}

// device memory of the tool's own, grown by doubling
struct DevArray {
    char *p = nullptr;
    size_t cap = 0, size = 0;
    DevArray() = default;
    DevArray(const DevArray &) = delete;
    DevArray &operator=(const DevArray &) = delete;
    ~DevArray() { if (p) (void)hipFree(p); }
    void reserve(size_t bytes)
    {
        if (bytes <= cap) return;
        const size_t nc = std::max(bytes, 2 * cap);
        char *q = nullptr;
        hip_check(hipMalloc(reinterpret_cast<void **>(&q), nc), "hipMalloc");
        if (size) hip_check(hipMemcpy(q, p, size, hipMemcpyDeviceToDevice), "hipMemcpy");
        if (p) (void)hipFree(p);
        p = q;
        cap = nc;
    }
    void put(size_t at, const void *h, size_t bytes)  // host bytes to [at, at + bytes)
    {
        reserve(at + bytes);
        if (bytes) hip_check(hipMemcpy(p + at, h, bytes, hipMemcpyHostToDevice), "hipMemcpy");
        size = std::max(size, at + bytes);
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = size = 0;
    }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// --parse: who reads the whole reads of a -r file.  host: DnaQReader on one thread, then the tool packs the bases and looks for the
// low-quality positions itself; gpu: WholeReadsSource -- the text is tokenised on the device (mc_tokenize_whole_dev) and its words,
// offsets and positions go into the _dev entry points where they are; auto: gpu for an uncompressed file of PARSE_AUTO_MIN bytes or
// more.  That is the smallest file scripts/whole_reads_bench.py has timed (10^5 FASTQ records of 150 bases), and there the whole
// reads-classifier is already faster the GPU's way; below it nothing is measured, and auto is host.
constexpr uint64_t PARSE_AUTO_MIN = 31600000;

bool parse_on_gpu(const Options &o, const std::string &path)
{
    std::string name = path;
    for (char &c : name) c = (char)tolower((unsigned char)c);
    auto ends = [&](const char *suffix) { const size_t n = strlen(suffix); return name.size() >= n && name.compare(name.size() - n, n, suffix) == 0; };
    const bool compressed = ends(".gz") || ends(".bz2");
    if (o.parse == "gpu") {
        if (compressed) throw Error("--parse gpu reads uncompressed FASTA and FASTQ files, and " + path + " is compressed: use --parse host");
        return true;
    }
    if (o.parse == "host" || compressed) return false;
    struct stat st;
    return stat(path.c_str(), &st) == 0 && (uint64_t)st.st_size >= PARSE_AUTO_MIN;
}

// a file of whole reads, read one way or the other
struct ReadsIn {
    std::unique_ptr<DnaQReader> host;
    std::unique_ptr<WholeReadsSource> gpu;
    mc_ctx *ctx;
    ReadsIn(const Options &o, mc_ctx *c, const std::string &path) : ctx(c)
    {
        if (parse_on_gpu(o, path)) gpu.reset(new WholeReadsSource(ctx, o.device, path));
        else host.reset(new DnaQReader(path));
    }
    size_t read(DnaQBatch &b, size_t max_reads, uint64_t max_bases = ~0ull) { return gpu ? gpu->read(b, max_reads, max_bases) : host->read(b, max_reads); }
};

// --render: who turns the reads that go to the classifiers' FASTQ files into text.  host: FastqOut::put, a record and a base at a
// time; gpu: mc_render_fastq* renders every output stream of a batch in one call, the text comes down into one staging buffer and
// each file takes its stream with one fwrite; auto: gpu only for reads that are on the device already (--parse gpu took every -r file
// there) and a first -r file of at least the size from which the whole tool was measured to be faster that way
// (scripts/render_bench.py): the triple classifier at 10^5 records of 150 bases, the smallest size measured;
// reads-classifier at 10^7 -- at 10^5 and 10^6 its two ways lie within each other's spread, and auto stays host.
constexpr uint64_t RENDER_AUTO_MIN = 3160000000, RENDER_AUTO_MIN_TRIPLE = 31600000;

bool render_on_gpu(const Options &o, bool reads_on_device, uint64_t auto_min)
{
    if (o.render == "gpu") return true;
    if (o.render == "host" || !reads_on_device) return false;
    struct stat st;
    return stat(o.read_files[0].c_str(), &st) == 0 && (uint64_t)st.st_size >= auto_min;
}

// page-locked host memory that grows: where the rendered text comes down
struct PinnedStage {
    uint8_t *p = nullptr;
    size_t cap = 0;
    PinnedStage() = default;
    PinnedStage(const PinnedStage &) = delete;
    PinnedStage &operator=(const PinnedStage &) = delete;
    ~PinnedStage() { if (p) (void)hipHostFree(p); }
    void reserve(size_t bytes)
    {
        if (bytes <= cap) return;
        const size_t nc = std::max(bytes, 2 * cap);
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        hip_check(hipHostMalloc(reinterpret_cast<void **>(&p), nc), "hipHostMalloc");
        cap = nc;
    }
};

// The output streams of a tool under --render gpu: stream t is a file (out[t]: its records are numbered from the file's count on) or
// a list kept aside (tail[t]: unnumbered bodies, numbered when the list is appended).  A batch is rendered from its device view
// (render_segments) or, for reads the host parsed, from the batch itself (render_batch); st[s][i] is the stream of read i of side s.
struct Renderer {
    mc_ctx *ctx = nullptr;
    uint32_t n_streams = 0;
    FastqOut *out[MC_RENDER_MAX_STREAMS] = {};
    SideList *tail[MC_RENDER_MAX_STREAMS] = {};
    std::vector<uint8_t> st[2];
    DevArray text, d_stream[2];
    PinnedStage stage;
    std::vector<uint8_t> host_text;
    unsigned long long records = 0, tail_records = 0, calls = 0;
    double call_s = 0, copy_s = 0, device_ms = 0;  // MC_INGEST_DEBUG: in mc_render_fastq*, in the copies down, on the device

    static double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
    void first_numbers(uint64_t *first) const
    {
        for (uint32_t t = 0; t < n_streams; t++) first[t] = out[t] ? out[t]->n + 1 : MC_RENDER_UNNUMBERED;
    }
    static void data_error(const mc_render_result &r)  // FastqOut::put's messages
    {
        if (r.error == MC_RENDER_EMPTY) throw Error("Empty DnaQ!");
        if (r.error == MC_RENDER_QUALITY) throw Error("Invalid quality code byte: " + std::to_string(r.error_value));
    }
    // the streams of reads [a, b) of the batch, rendered into `bytes`, go to their files and lists
    void deliver(const uint8_t *bytes, const mc_render_result &r, int n_sides, const DnaQBatch *const *b, uint64_t a, uint64_t e)
    {
        std::vector<uint64_t> lens;
        for (uint32_t t = 0; t < n_streams; t++) {
            records += r.records[t];
            if (out[t]) {
                out[t]->put_rendered(bytes + r.start[t], r.bytes[t], r.records[t]);
            } else if (r.records[t]) {
                lens.clear();
                for (uint64_t i = a; i < e; i++)
                    for (int s = 0; s < n_sides; s++)
                        if (st[s][i] == t) lens.push_back(b[s]->offsets[i + 1] - b[s]->offsets[i]);
                tail[t]->put_bodies(bytes + r.start[t], r.bytes[t], lens.data(), lens.size());
                tail_records += r.records[t];
            }
        }
        calls++;
    }
    // the first n reads of a batch from its device view: a call per sub-range of reads that lie in one segment on every side
    void render_segments(int n_sides, const std::vector<WholeSegment> *const *segs, const DnaQBatch *const *b, uint64_t n)
    {
        std::vector<std::pair<uint64_t, uint64_t>> cover[2];
        for (int s = 0; s < n_sides; s++) {
            for (const WholeSegment &g : *segs[s]) cover[s].emplace_back(g.first, g.n_reads);
            d_stream[s].put(0, st[s].data(), n);
        }
        for (const RenderRange &r : render_ranges(cover, n_sides, n)) {
            mc_render_side sides[2] = {};
            uint64_t bases = 0;
            for (int s = 0; s < n_sides; s++) {
                const WholeSegment &g = (*segs[s])[r.seg[s]];
                // (a view without bases may come without phreds: no base, no phred is read)
                sides[s] = mc_render_side{g.d_words, g.d_phred ? g.d_phred : reinterpret_cast<const uint8_t *>(g.d_words), g.d_offsets + (r.a - g.first),
                                          d_stream[s].as<uint8_t>() + r.a};
                bases += b[s]->offsets[r.b] - b[s]->offsets[r.a];
            }
            text.reserve(mc_render_fastq_bound(bases, (uint64_t)n_sides * (r.b - r.a)));
            uint64_t first[MC_RENDER_MAX_STREAMS];
            first_numbers(first);
            mc_render_result res;
            auto t0 = std::chrono::steady_clock::now();
            MC_CHECK(ctx, mc_render_fastq_dev(ctx, sides, (uint32_t)n_sides, r.b - r.a, n_streams, first, text.as<uint8_t>(), text.cap, &res));
            call_s += since(t0);
            device_ms += res.device_ms;
            data_error(res);
            const uint64_t end = res.start[n_streams - 1] + res.bytes[n_streams - 1];
            stage.reserve(end);
            t0 = std::chrono::steady_clock::now();
            if (end) hip_check(hipMemcpy(stage.p, text.p, end, hipMemcpyDeviceToHost), "hipMemcpy");
            copy_s += since(t0);
            deliver(stage.p, res, n_sides, b, r.a, r.b);
        }
    }
    // ... and of reads the host parsed: packed as classify_batch packs them, one call
    void render_batch(int n_sides, const DnaQBatch *const *b, uint64_t n)
    {
        static const uint8_t none = 0;
        std::vector<uint64_t> words[2];
        mc_render_side sides[2] = {};
        uint64_t bases = 0;
        for (int s = 0; s < n_sides; s++) {
            pack_whole_reads(*b[s], 0, n, words[s], nullptr);
            sides[s] = mc_render_side{words[s].data(), b[s]->phred.empty() ? &none : b[s]->phred.data(), b[s]->offsets.data(), st[s].empty() ? &none : st[s].data()};
            bases += b[s]->offsets[n];
        }
        host_text.resize(mc_render_fastq_bound(bases, (uint64_t)n_sides * n));
        uint64_t first[MC_RENDER_MAX_STREAMS];
        first_numbers(first);
        mc_render_result res;
        const auto t0 = std::chrono::steady_clock::now();
        MC_CHECK(ctx, mc_render_fastq(ctx, sides, (uint32_t)n_sides, n, n_streams, first, host_text.data(), host_text.size(), &res));
        call_s += since(t0);
        device_ms += res.device_ms;
        data_error(res);
        deliver(host_text.data(), res, n_sides, b, 0, n);
    }
    // the debug line's numbers: `written` the records of all files when they are complete
    void report(unsigned long long written) const
    {
        fprintf(stderr, "[ingest] render: %llu records in %llu call(s) on the device, %llu through the host\n", records, calls,
                written - (records - tail_records));
        if (calls) fprintf(stderr, "[ingest] render stage: %.3f s in the calls (%.3f ms on the device), %.3f s in the copies down\n", call_s, device_ms, copy_s);
    }
};

// findReadWithCorrection's one low-quality position of each of the first n reads: -1 for none, -2 for several (mc_classify_reads)
std::vector<int32_t> bad_positions(const DnaQBatch &b, size_t n)
{
    return low_quality_positions(b, 0, n);
}

// one batch of whole reads through mc_classify_reads: N is base 0 already (DnaQReader), bad_pos as findReadWithCorrection counts
std::vector<mc_read_cov> classify_batch(mc_ctx *ctx, const DnaQBatch &b, size_t n, const Options &o)
{
    std::vector<mc_read_cov> out(n);
    if (n == 0) return out;
    std::vector<uint64_t> words;
    pack_whole_reads(b, 0, n, words, nullptr);
    const std::vector<int32_t> bad = o.correction ? bad_positions(b, n) : std::vector<int32_t>();
    MC_CHECK(ctx, mc_classify_reads(ctx, words.data(), b.offsets.data(), n, o.correction ? bad.data() : nullptr, (int)o.found_threshold,
                                    o.interval95 ? 1.96 : 1.0, o.correction ? MC_CLASSIFY_CORRECTION : 0, out.data()));
    return out;
}

// ... and the first n reads of a batch WholeReadsSource delivered, from its device view (defined behind DevArray)
std::vector<mc_read_cov> classify_segments(mc_ctx *ctx, const std::vector<WholeSegment> &segs, size_t n, const Options &o);

std::vector<mc_read_cov> classify_side(mc_ctx *ctx, const ReadsIn &in, const DnaQBatch &b, size_t n, const Options &o)
{
    return in.gpu ? classify_segments(ctx, in.gpu->segments(), n, o) : classify_batch(ctx, b, n, o);
}

// file.getName().toLowerCase().endsWith("kmers.bin"): loadGraph reads such a file as kmer-counter's output
bool names_kmers_bin(const std::string &path)
{
    std::string first = path;
    const size_t slash = first.find_last_of('/');
    if (slash != std::string::npos) first = first.substr(slash + 1);
    for (char &c : first) c = (char)tolower((unsigned char)c);
    return first.size() >= 9 && first.compare(first.size() - 9, 9, "kmers.bin") == 0;
}

// loadGraph (ReadsClassifier.java:98-132, TripleReadsClassifier.java:127-160): the hash-function line for k > 31, then the table at k
// from kmer_files when the first one's name ends in kmers.bin (IOUtils.loadKmers), else counted from the reads of --input-files
void load_graph(const Options &o, int k, const std::vector<std::string> &kmer_files, Engine &E)
{
    int mode = MC_KEY_PACKED;
    if (k > 31) {  // determineHashFunction
        std::string h = o.hash;
        for (char &c : h) c = (char)tolower((unsigned char)c);
        if (h == "fnv1a") { info("Using FNV1a hash function"); mode = MC_KEY_FNV1A; }
        else { info("Using default polynomial hash function"); mode = MC_KEY_POLY; }
    }
    const bool kmers_bin = !kmer_files.empty() && names_kmers_bin(kmer_files[0]);
    mc_config cfg{};
    cfg.k = k;
    cfg.key_mode = mode;
    cfg.device = o.device;
    cfg.capacity_hint = o.capacity_hint;
    E.open(cfg, {});
    mc_ctx *ctx = E.c;
    uint64_t n_distinct = 0;
    if (kmers_bin) {  // IOUtils.loadKmers(files, 0, ...)
        for (const std::string &path : kmer_files) load_kmers_file(o, ctx, path);
        E.finalize(&n_distinct);
        info("Hashtable size: " + std::to_string(n_distinct) + " kmers");
    } else {
        if (k > 31) info("Reading hashes of k-mers instead");
        load_reads(o.input_files, E);
    }
}

int run_reads_classifier(const Options &o)
{
    // (every parameter is checked before a device is opened)
    if (o.k < 0) throw Error("Parameter 'k' is mandatory");
    if (o.input_files.empty()) throw Error("Parameter 'input-files' is mandatory");
    if (o.read_files.empty()) throw Error("Parameter 'read-files' is mandatory");
    if (o.k < 1 || o.k > 63)
        throw Error("k = " + std::to_string(o.k) + " is not supported: this build handles k <= 31 (packed keys) and 32 <= k <= 63 (hash keys)");
    if (o.found_threshold < 0 || o.found_threshold > 100) throw Error("--found-threshold must be within 0 .. 100 (a percentage of the read)");
    if (!open_work_dir(o, "k=" + std::to_string(o.k) + "\n")) return 0;
    const std::string out_dir = o.output_dir.empty() ? o.work_dir + "/reads_classifier" : o.output_dir;
    write_file(out_dir + "/.keep", "");  // outputDir.mkdirs()
    remove((out_dir + "/.keep").c_str());

    Engine E;
    load_graph(o, o.k, o.input_files, E);
    mc_ctx *ctx = E.c;

    info("Loading reads...");
    const bool paired = o.read_files.size() == 2;
    ReadsIn r1(o, ctx, o.read_files[0]);
    std::unique_ptr<ReadsIn> r2(paired ? new ReadsIn(o, ctx, o.read_files[1]) : nullptr);
    info(o.correction ? "Searching for corrected reads in graph..." : "Searching for reads in graph...");
    FastqOut found1(out_dir + "/found_1.fastq"), found2(out_dir + "/found_2.fastq"), nf1(out_dir + "/not_found_1.fastq"),
        nf2(out_dir + "/not_found_2.fastq"), found_s(out_dir + "/found_s.fastq"), nf_s(out_dir + "/not_found_s.fastq");
    SideList found_s_tail, nf_s_tail;
    // (the reads are on the device when --parse gpu took every file there)
    const bool on_device = r1.gpu && (!paired || r2->gpu);
    std::unique_ptr<Renderer> R;
    if (render_on_gpu(o, on_device, RENDER_AUTO_MIN)) {
        R.reset(new Renderer);
        R->ctx = ctx;
        R->n_streams = 8;
        FastqOut *files[6] = {&found1, &found2, &nf1, &nf2, &found_s, &nf_s};
        for (int t = 0; t < 6; t++) R->out[t] = files[t];
        R->tail[6] = &found_s_tail;
        R->tail[7] = &nf_s_tail;
        hip_check(hipSetDevice(o.device), "hipSetDevice");
    }
    long long both = 0, first_only = 0, second_only = 0, neither = 0;
    constexpr size_t BATCH = 1u << 20;
    DnaQBatch b1, b2;
    for (;;) {
        b1.clear();
        b2.clear();
        size_t n = r1.read(b1, BATCH);
        if (paired) n = r2->read(b2, n);  // PairSource (itmo!/io/sources/PairSource.java:35-45): pairs end with the shorter file
        if (n == 0) break;
        const std::vector<mc_read_cov> c1 = classify_side(ctx, r1, b1, n, o);
        const std::vector<mc_read_cov> c2 = paired ? classify_side(ctx, *r2, b2, n, o) : std::vector<mc_read_cov>(n);
        if (R) {  // --render gpu: the host still decides every read's stream (and counts); the records are rendered on the device
            enum { FOUND_1, FOUND_2, NF_1, NF_2, FOUND_S, NF_S, FOUND_S_TAIL, NF_S_TAIL };
            R->st[0].assign(n, MC_RENDER_SKIP);
            if (paired) R->st[1].assign(n, MC_RENDER_SKIP);
            for (size_t i = 0; i < n; i++) {
                const size_t l1 = b1.offsets[i + 1] - b1.offsets[i], l2 = paired ? b2.offsets[i + 1] - b2.offsets[i] : 0;
                const bool f1 = c1[i].found != 0;
                const bool f2 = l2 == 0 ? !f1 : c2[i].found != 0;  // (a single-end read is paired with an empty one)
                uint8_t t1 = MC_RENDER_SKIP, t2 = MC_RENDER_SKIP;
                if (f1 && f2) { both++; t1 = FOUND_1; t2 = FOUND_2; }
                else if (f1) { first_only++; if (l1) t1 = FOUND_S; if (l2) t2 = NF_S; }
                else if (f2) { second_only++; if (l2) t2 = FOUND_S_TAIL; if (l1) t1 = NF_S_TAIL; }
                else { neither++; t1 = NF_1; t2 = NF_2; }
                R->st[0][i] = t1;
                if (paired) R->st[1][i] = t2;
            }
            const DnaQBatch *bs[2] = {&b1, &b2};
            const std::vector<WholeSegment> *segs[2] = {r1.gpu ? &r1.gpu->segments() : nullptr, paired && r2->gpu ? &r2->gpu->segments() : nullptr};
            if (on_device) R->render_segments(paired ? 2 : 1, segs, bs, n);
            else R->render_batch(paired ? 2 : 1, bs, n);
            if (paired && n < BATCH) break;  // (one of the files is done)
            continue;
        }
        for (size_t i = 0; i < n; i++) {
            const uint8_t *s1 = b1.codes.data() + b1.offsets[i], *q1 = b1.phred.data() + b1.offsets[i];
            const size_t l1 = b1.offsets[i + 1] - b1.offsets[i];
            const uint8_t *s2 = paired ? b2.codes.data() + b2.offsets[i] : nullptr, *q2 = paired ? b2.phred.data() + b2.offsets[i] : nullptr;
            const size_t l2 = paired ? b2.offsets[i + 1] - b2.offsets[i] : 0;
            const bool f1 = c1[i].found != 0;
            const bool f2 = l2 == 0 ? !f1 : c2[i].found != 0;  // (a single-end read is paired with an empty one)
            if (f1 && f2) {
                both++;
                found1.put(s1, q1, l1);
                found2.put(s2, q2, l2);
            } else if (f1) {
                first_only++;
                if (l1) found_s.put(s1, q1, l1);
                if (l2) nf_s.put(s2, q2, l2);
            } else if (f2) {
                second_only++;
                if (l2) found_s_tail.put(s2, q2, l2);
                if (l1) nf_s_tail.put(s1, q1, l1);
            } else {
                neither++;
                nf1.put(s1, q1, l1);
                nf2.put(s2, q2, l2);
            }
        }
        if (paired && n < BATCH) break;  // (one of the files is done)
    }

    // FoundStats (ReadsClassifier.java:203-260): Java ints, String.format("%.2f")
    const long long total = 2 * (both + first_only + second_only + neither), found = 2 * both + first_only + second_only,
                    not_found = 2 * neither + first_only + second_only, pairs = 2 * (both + neither);
    info("|\tTotal: " + std::to_string(total) + " reads");
    info("|\tPaired: " + std::to_string(pairs) + " reads");
    info("|\tTotal quality: " + java_format_2f(100 * (double)pairs / (double)total) + " %");
    info("|\tFound: " + std::to_string(found) + " reads");
    info("|\tPercent of found reads: " + java_format_2f(100 * (double)found / (double)total) + " %");
    info("|\tQuality of found bin: " + java_format_2f((double)both * 2 / (double)(both * 2 + first_only + second_only) * 100) + " %");
    info("|\tNot found: " + std::to_string(not_found) + " reads");
    info("|\tPercent of not found reads: " + java_format_2f(100 * (double)not_found / (double)total) + " %");
    info("|\tQuality of not found bin: " + java_format_2f((double)neither * 2 / (double)(neither * 2 + first_only + second_only) * 100) + " %");
    info("Writing classified reads...");
    found_s_tail.append_to(found_s);
    nf_s_tail.append_to(nf_s);
    for (FastqOut *f : {&found1, &found2, &nf1, &nf2, &found_s, &nf_s}) f->close();
    info("Reads have been written. Finishing...");
    if (g_time_writers) {
        fprintf(stderr, "[ingest] FastqOut: %.3f s in put() for %llu records\n", g_fastq_out_s, g_fastq_out_n);
        const Renderer none;
        (R ? R.get() : &none)->report(found1.n + found2.n + nf1.n + nf2.n + found_s.n + nf_s.n);
    }
    write_file(o.work_dir + "/SUCCESS", "");
    return 0;
}

// --tool triple-reads-classifier (src/tools/TripleReadsClassifier.java:164-270, src/algo/TripleFinder.java, src/algo/TripleFinder2.java):
// the pairs of -r classed found / half found / not found by their k-mers in the graph at k, then at k2, written to nine FASTQ files.
// Both sides' reads stay on the device for both passes.  A read's pass-1 class is that of the last read of its side with the same bases
// (the reference's maps keyed by bases: mc_reads_last_copy).  The reference runs pairs on a thread pool, so its lists' order and its
// maps' last writer are only defined at -p 1; here they are that: input order in every file, "last" = the greatest input index.

std::vector<mc_read_cov> classify_segments(mc_ctx *ctx, const std::vector<WholeSegment> &segs, size_t n, const Options &o)
{
    std::vector<mc_read_cov> out(n);
    if (n == 0) return out;
    DevArray cov;
    cov.reserve(n * sizeof(mc_read_cov));
    for (const WholeSegment &g : segs) {
        if (g.first >= n) break;  // (pairs end with the shorter file: the longer one's batch may hold more reads)
        const uint64_t m = std::min<uint64_t>(g.n_reads, n - g.first);
        MC_CHECK(ctx, mc_classify_reads_dev(ctx, g.d_words, g.d_offsets, m, o.correction ? g.d_bad_pos : nullptr, (int)o.found_threshold,
                                            o.interval95 ? 1.96 : 1.0, o.correction ? MC_CLASSIFY_CORRECTION : 0, cov.as<mc_read_cov>() + g.first));
    }
    hip_check(hipMemcpy(out.data(), cov.p, n * sizeof(mc_read_cov), hipMemcpyDeviceToHost), "hipMemcpy");
    return out;
}

// one side of the pairs on the device, in mc_classify_reads' layout: words (the pad word included), offsets, bad positions
struct SideStore {
    DevArray words, offsets, bad;
    uint64_t n_reads = 0, n_bases = 0, carry = 0;  // carry: the partly filled last word, written again with the next batch
    void add(const DnaQBatch &b, size_t n, bool correction)
    {
        if (n_reads == 0) {
            const uint64_t z = 0;
            offsets.put(0, &z, 8);
        }
        const uint64_t nb = b.offsets[n], end = n_bases + nb, w0 = n_bases / 32;
        std::vector<uint64_t> w((end + 31) / 32 - w0 + 1, 0);
        w[0] = carry;
        for (uint64_t i = 0; i < nb; i++) {
            const uint64_t g = n_bases + i;
            w[g / 32 - w0] |= (uint64_t)(b.codes[i] & 3) << (62 - 2 * (g & 31));
        }
        words.put(w0 * 8, w.data(), w.size() * 8);
        carry = end % 32 ? w[end / 32 - w0] : 0;
        std::vector<uint64_t> off(n);
        for (size_t i = 0; i < n; i++) off[i] = n_bases + b.offsets[i + 1];
        offsets.put((n_reads + 1) * 8, off.data(), n * 8);
        if (correction) {
            const std::vector<int32_t> bp = bad_positions(b, n);
            bad.put(n_reads * 4, bp.data(), n * 4);
        }
        n_reads += n;
        n_bases = end;
    }
    // --parse gpu: the first n reads of a batch's device view, joined behind what is here on the device (mc_reads_append_dev).  A store
    // is filled one way or the other, never both (the host's way keeps the last word here).
    void add_dev(mc_ctx *ctx, const std::vector<WholeSegment> &segs, const DnaQBatch &b, size_t n, bool correction)
    {
        if (n_reads == 0 && words.size == 0) {
            const uint64_t z = 0;
            words.put(0, &z, 8);
            offsets.put(0, &z, 8);
        }
        const uint64_t end = n_bases + b.offsets[n];
        words.reserve(((end + 31) / 32 + 1) * 8);
        offsets.reserve((n_reads + n + 1) * 8);
        if (correction) bad.reserve((n_reads + n) * 4);
        uint64_t at_reads = n_reads, at_bases = n_bases;
        for (const WholeSegment &g : segs) {
            if (g.first >= n) break;  // (pairs end with the shorter file)
            const uint64_t m = std::min<uint64_t>(g.n_reads, n - g.first);
            MC_CHECK(ctx, mc_reads_append_dev(ctx, g.d_words, g.d_offsets, m, words.as<uint64_t>(), at_bases, offsets.as<uint64_t>() + at_reads));
            if (correction && m) hip_check(hipMemcpy(bad.p + at_reads * 4, g.d_bad_pos, m * 4, hipMemcpyDeviceToDevice), "hipMemcpy");
            at_bases += b.offsets[g.first + m] - b.offsets[g.first];
            at_reads += m;
        }
        if (at_reads != n_reads + n || at_bases != end) throw Error("internal: a batch's device view does not cover it");
        words.size = ((end + 31) / 32 + 1) * 8;
        offsets.size = (n_reads + n + 1) * 8;
        if (correction) bad.size = (n_reads + n) * 4;
        n_reads += n;
        n_bases = end;
    }
};

// the pairs of two DnaQ readers, batch by batch: PairSource (itmo!/io/sources/PairSource.java:35-45) ends them with the shorter file
template <typename F>
void for_each_pair_batch(const Options &o, F &&f, bool need_ctx = false)
{
    Engine T;  // (--parse gpu: any context tokenises, and --render gpu: any context renders; the graphs are not loaded yet)
    if (need_ctx || parse_on_gpu(o, o.read_files[0]) || parse_on_gpu(o, o.read_files[1])) {
        mc_config cfg{};
        cfg.k = o.k;
        cfg.device = o.device;
        T.open(cfg, {});
    }
    ReadsIn r1(o, T.c, o.read_files[0]), r2(o, T.c, o.read_files[1]);
    constexpr size_t BATCH = 1u << 20;
    DnaQBatch b1, b2;
    for (;;) {
        b1.clear();
        b2.clear();
        size_t n = r1.read(b1, BATCH);
        n = r2.read(b2, n);
        if (n == 0) break;
        f(b1, b2, n, r1, r2);
        if (n < BATCH) break;  // (one of the files is done)
    }
}

int run_triple_reads_classifier(const Options &o)
{
    // (every parameter is checked before a device is opened)
    if (o.k < 0) throw Error("Parameter 'k' is mandatory");
    if (o.k2 < 0) throw Error("Parameter 'k2' is mandatory");
    if (o.read_files.empty()) throw Error("Parameter 'read-files' is mandatory");
    if (o.k >= o.k2) throw Error("k2 should be greater than k, given: " + std::to_string(o.k) + " " + std::to_string(o.k2));
    if (o.read_files.size() < 2)  // (the reference takes sources.get(1); files after the second are ignored, as there)
        throw Error("--read-files needs two files of paired reads, given: " + std::to_string(o.read_files.size()));
    const std::vector<std::string> *kmers[2] = {&o.input_kmers_1, &o.input_kmers_2};
    for (int pass = 0; pass < 2; pass++)
        if (o.input_files.empty() && (kmers[pass]->empty() || !names_kmers_bin((*kmers[pass])[0])))
            throw Error("No graph for k = " + std::to_string(pass ? o.k2 : o.k) + ": give --input-files, or --input-kmers-" +
                        std::to_string(pass + 1) + " with a <name>.kmers.bin from kmer-counter");
    for (int kk : {o.k, o.k2})
        if (kk < 1 || kk > 63)
            throw Error("k = " + std::to_string(kk) + " is not supported: this build handles k <= 31 (packed keys) and 32 <= k <= 63 (hash keys)");
    if (o.found_threshold < 0 || o.found_threshold > 100) throw Error("--found-threshold must be within 0 .. 100 (a percentage of the read)");
    if (o.half_threshold < 0 || o.half_threshold > 100) throw Error("--half-threshold must be within 0 .. 100 (a percentage of the read)");
    if (!open_work_dir(o, "k=" + std::to_string(o.k) + "\nk2=" + std::to_string(o.k2) + "\n")) return 0;
    const std::string out_dir = o.output_dir.empty() ? o.work_dir + "/reads_classifier" : o.output_dir;
    write_file(out_dir + "/.keep", "");  // outputDir.mkdirs()
    remove((out_dir + "/.keep").c_str());

    info("Loading reads...");
    hip_check(hipSetDevice(o.device), "hipSetDevice");
    SideStore side[2];
    for_each_pair_batch(o, [&](const DnaQBatch &b1, const DnaQBatch &b2, size_t n, const ReadsIn &r1, const ReadsIn &r2) {
        const DnaQBatch *b[2] = {&b1, &b2};
        const ReadsIn *r[2] = {&r1, &r2};
        for (int s = 0; s < 2; s++) {
            if (r[s]->gpu) side[s].add_dev(r[s]->ctx, r[s]->gpu->segments(), *b[s], n, o.correction);
            else side[s].add(*b[s], n, o.correction);
        }
    });
    const uint64_t n = side[0].n_reads;

    // the two passes: each side's coverage at k (mc_classify_reads), then its classes (mc_triple_classes); pass 2 reads pass 1's
    // class of every read's last copy
    DevArray cov[2], cls1[2], cls2[2], last[2];
    for (int s = 0; s < 2; s++) {
        cov[s].reserve(n * sizeof(mc_read_cov));
        cls1[s].reserve(n);
        cls2[s].reserve(n);
        last[s].reserve(n * 4);
    }
    const double z = o.interval95 ? 1.96 : 1.0;
    for (int pass = 0; pass < 2; pass++) {
        const int k = pass ? o.k2 : o.k;
        info("Building graph with k = " + std::to_string(k) + " ...");
        Engine E;  // (one graph at a time: cleanImpl frees the first before the second is built)
        load_graph(o, k, *kmers[pass], E);
        mc_ctx *ctx = E.c;
        info(o.correction ? "Searching for corrected reads in graph..." : "Searching for reads in graph...");
        for (int s = 0; s < 2; s++)
            MC_CHECK(ctx, mc_classify_reads_dev(ctx, side[s].words.as<uint64_t>(), side[s].offsets.as<uint64_t>(), n,
                                                o.correction ? side[s].bad.as<int32_t>() : nullptr, (int)o.found_threshold, z,
                                                o.correction ? MC_CLASSIFY_CORRECTION : 0, cov[s].as<mc_read_cov>()));
        DevArray *out = pass ? cls2 : cls1;
        MC_CHECK(ctx, mc_triple_classes_dev(ctx, cov[0].as<mc_read_cov>(), cov[1].as<mc_read_cov>(), side[0].offsets.as<uint64_t>(),
                                            side[1].offsets.as<uint64_t>(), n, (int)o.half_threshold, pass ? cls1[0].as<uint8_t>() : nullptr,
                                            pass ? cls1[1].as<uint8_t>() : nullptr, pass ? last[0].as<uint32_t>() : nullptr,
                                            pass ? last[1].as<uint32_t>() : nullptr, out[0].as<uint8_t>(), out[1].as<uint8_t>()));
        if (pass == 0)
            for (int s = 0; s < 2; s++)
                MC_CHECK(ctx, mc_reads_last_copy_dev(ctx, side[s].words.as<uint64_t>(), side[s].offsets.as<uint64_t>(), n, 0, last[s].as<uint32_t>()));
    }
    std::vector<uint8_t> c1(n), c2(n);
    if (n) {
        hip_check(hipMemcpy(c1.data(), cls2[0].p, n, hipMemcpyDeviceToHost), "hipMemcpy");
        hip_check(hipMemcpy(c2.data(), cls2[1].p, n, hipMemcpyDeviceToHost), "hipMemcpy");
    }
    for (int s = 0; s < 2; s++)  // (the reads are read again from the files below)
        for (DevArray *a : {&side[s].words, &side[s].offsets, &side[s].bad, &cov[s], &cls1[s], &cls2[s], &last[s]}) a->release();

    // FoundStats (TripleReadsClassifier.java:225-242,276-333): Java ints, String.format("%.2f")
    long long both[3] = {0, 0, 0}, single[3] = {0, 0, 0};  // by class: both mates in it, one mate of a mixed pair in it
    for (uint64_t i = 0; i < n; i++) {
        if (c1[i] == c2[i]) both[c1[i]]++;
        else { single[c1[i]]++; single[c2[i]]++; }
    }
    const long long bf = both[MC_CLASS_FOUND], bh = both[MC_CLASS_HALF_FOUND], bn = both[MC_CLASS_NOT_FOUND];
    const long long total = 2 * (bn + bf + bh) + single[0] + single[1] + single[2], paired = 2 * (bf + bn + bh);
    const long long found = 2 * bf + single[MC_CLASS_FOUND], not_found = 2 * bn + single[MC_CLASS_NOT_FOUND],
                    half_found = 2 * bh + single[MC_CLASS_HALF_FOUND];
    info("|\tTotal: " + std::to_string(total) + " reads");
    info("|\tPaired: " + std::to_string(paired) + " reads");
    info("|\tTotal quality: " + java_format_2f(100 * (double)paired / (double)total) + " %");
    info("|\tFound: " + std::to_string(found) + " reads");
    info("|\tPercent of found reads: " + java_format_2f(100 * (double)found / (double)total) + " %");
    info("|\tQuality of found bin: " + java_format_2f((double)bf * 2 / (double)found * 100) + " %");
    info("|\tNot found: " + std::to_string(not_found) + " reads");
    info("|\tPercent of not found reads: " + java_format_2f(100 * (double)not_found / (double)total) + " %");
    info("|\tQuality of not found bin: " + java_format_2f((double)bn * 2 / (double)not_found * 100) + " %");
    info("|\tHalf found: " + std::to_string(half_found) + " reads");
    info("|\tPercent of half found reads: " + java_format_2f(100 * (double)half_found / (double)total) + " %");
    info("|\tQuality of half found bin: " + java_format_2f((double)bh * 2 / (double)half_found * 100) + " %");

    // the nine files, streamed from a second read of -r in input order: found_{1,2} take every read (an empty one fails the writer,
    // "Empty DnaQ!"), the others only reads of length > 0
    info("Writing classified reads...");
    FastqOut found1(out_dir + "/found_1.fastq"), found2(out_dir + "/found_2.fastq"), half1(out_dir + "/half_found_1.fastq"),
        half2(out_dir + "/half_found_2.fastq"), nf1(out_dir + "/not_found_1.fastq"), nf2(out_dir + "/not_found_2.fastq"),
        found_s(out_dir + "/found_s.fastq"), half_s(out_dir + "/half_found_s.fastq"), nf_s(out_dir + "/not_found_s.fastq");
    FastqOut *pair_out[3][2] = {{&nf1, &nf2}, {&half1, &half2}, {&found1, &found2}}, *single_out[3] = {&nf_s, &half_s, &found_s};
    uint64_t at = 0;
    // (the reads are on the device when --parse gpu takes both files there)
    const bool render_gpu = render_on_gpu(o, parse_on_gpu(o, o.read_files[0]) && parse_on_gpu(o, o.read_files[1]), RENDER_AUTO_MIN_TRIPLE);
    Renderer R;
    R.n_streams = 9;  // stream 2 * class + side: the pair files; 6 + class: the _s files, which take both sides in item order
    for (int c = 0; c < 3; c++) {
        R.out[2 * c] = pair_out[c][0];
        R.out[2 * c + 1] = pair_out[c][1];
        R.out[6 + c] = single_out[c];
    }
    for_each_pair_batch(o, [&](const DnaQBatch &b1, const DnaQBatch &b2, size_t m, const ReadsIn &r1, const ReadsIn &r2) {
        if (at + m > n) throw Error("The read files changed while they were being classified");
        const DnaQBatch *b[2] = {&b1, &b2};
        if (render_gpu) {
            R.ctx = r1.ctx;
            for (int s = 0; s < 2; s++) R.st[s].assign(m, MC_RENDER_SKIP);
            for (size_t i = 0; i < m; i++, at++) {
                const uint8_t cls[2] = {c1[at], c2[at]};
                for (int s = 0; s < 2; s++) {
                    const uint64_t len = b[s]->offsets[i + 1] - b[s]->offsets[i];
                    if (cls[0] == cls[1]) {
                        if (len || cls[0] == MC_CLASS_FOUND) R.st[s][i] = (uint8_t)(2 * cls[0] + s);
                    } else if (len) {
                        R.st[s][i] = (uint8_t)(6 + cls[s]);
                    }
                }
            }
            const std::vector<WholeSegment> *segs[2] = {r1.gpu ? &r1.gpu->segments() : nullptr, r2.gpu ? &r2.gpu->segments() : nullptr};
            if (r1.gpu && r2.gpu) R.render_segments(2, segs, b, m);
            else R.render_batch(2, b, m);
            return;
        }
        for (size_t i = 0; i < m; i++, at++) {
            const uint8_t cls[2] = {c1[at], c2[at]};
            for (int s = 0; s < 2; s++) {
                const uint64_t o0 = b[s]->offsets[i], len = b[s]->offsets[i + 1] - o0;
                const uint8_t *codes = b[s]->codes.data() + o0, *phred = b[s]->phred.data() + o0;
                if (cls[0] == cls[1]) {
                    if (len || cls[0] == MC_CLASS_FOUND) pair_out[cls[0]][s]->put(codes, phred, len);
                } else if (len) {
                    single_out[cls[s]]->put(codes, phred, len);
                }
            }
        }
    }, render_gpu);
    for (FastqOut *f : {&found1, &found2, &half1, &half2, &nf1, &nf2, &found_s, &half_s, &nf_s}) f->close();
    if (g_time_writers) {
        fprintf(stderr, "[ingest] FastqOut: %.3f s in put() for %llu records\n", g_fastq_out_s, g_fastq_out_n);
        R.report(found1.n + found2.n + half1.n + half2.n + nf1.n + nf2.n + found_s.n + half_s.n + nf_s.n);
    }
    info("Reads have been written. Finishing...");
    write_file(o.work_dir + "/SUCCESS", "");
    return 0;
}

// --tool seq-cov (src/tools/SequenceCoverage.java:127-185): four bins of reads counted into four tables (every k-mer), then for
// every sequence of --read-file the mean depth and the breadth of its k-mers in each (mc_seq_coverage: one key, four probes a
// window).  Nothing walks these tables: no read store is kept, and a table's counting scratch goes back before the next is counted.
struct SeqCovBin { const char *param; const std::vector<std::string> *files; };

// one batch of whole sequences through mc_seq_coverage, and its rows.  segs: the batch's device view (--parse gpu), else NULL
void seq_cov_batch(mc_ctx *const *tables, const DnaQBatch &b, int k, FILE *out, const std::vector<WholeSegment> *segs = nullptr)
{
    const size_t n = b.n_reads();
    if (n == 0) return;
    std::vector<mc_seq_cov> cov(n * 4);
    if (segs) {
        DevArray d_cov;
        d_cov.reserve(n * 4 * sizeof(mc_seq_cov));
        for (const WholeSegment &g : *segs)
            MC_CHECK(tables[0], mc_seq_coverage_dev(tables, 4, g.d_words, g.d_offsets, g.n_reads, d_cov.as<mc_seq_cov>() + g.first * 4));
        hip_check(hipMemcpy(cov.data(), d_cov.p, n * 4 * sizeof(mc_seq_cov), hipMemcpyDeviceToHost), "hipMemcpy");
    } else {
        const uint64_t n_bases = b.offsets[n];
        std::vector<uint64_t> words((n_bases + 31) / 32 + 1, 0);
        for (uint64_t i = 0; i < n_bases; i++) words[i >> 5] |= (uint64_t)(b.codes[i] & 3) << (62 - 2 * (i & 31));
        MC_CHECK(tables[0], mc_seq_coverage(tables, 4, words.data(), b.offsets.data(), n, cov.data()));
    }
    std::string line;
    for (size_t s = 0; s < n; s++) {
        const uint64_t len = b.offsets[s + 1] - b.offsets[s];
        line.resize(len);  // dna.toString(): N is A already (a contig's row is megabytes: built once, written, reused)
        for (uint64_t i = 0; i < len; i++) line[i] = "AGCT"[b.codes[b.offsets[s] + i] & 3];
        const double windows = (double)((int32_t)len - k + 1);  // (a Java int; 0 or negative for a sequence shorter than k)
        for (int t = 0; t < 4; t++) {
            line += ", " + java_double_to_string((double)cov[s * 4 + t].depth / windows);  // depth * 1. / n: NaN for 0.0 / 0, -0.0 for 0.0 / negative
            line += ", " + java_double_to_string((double)cov[s * 4 + t].breadth / windows);
        }
        line.push_back('\n');
        if (fwrite(line.data(), 1, line.size(), out) != line.size()) throw Error("cannot write seq_cov.csv");
    }
}

int run_seq_cov(const Options &o)
{
    // the reference's order of bins (runImpl: donor, before, both, itself), whatever the command line's
    const SeqCovBin bins[4] = {{"from-donor", &o.from_donor}, {"from-before", &o.from_before}, {"from-both", &o.from_both}, {"itself", &o.itself}};
    if (o.k < 0) throw Error("Parameter 'k' is mandatory");
    for (const SeqCovBin &b : {bins[1], bins[0], bins[2], bins[3]})  // (the order the tool declares them in)
        if (b.files->empty()) throw Error(std::string("Parameter '") + b.param + "' is mandatory");
    if (o.read_file.empty()) throw Error("Parameter 'read-file' is mandatory");
    if (o.k < 1 || o.k > 63)
        throw Error("k = " + std::to_string(o.k) + " is not supported: this build handles k <= 31 (packed keys) and 32 <= k <= 63 (hash keys)");
    if (!open_work_dir(o, "k=" + std::to_string(o.k) + "\n")) return 0;
    const std::string out_dir = o.output_dir.empty() ? o.work_dir + "/sequence_coverage" : o.output_dir;
    write_file(out_dir + "/.keep", "");  // outputDir.mkdirs()
    remove((out_dir + "/.keep").c_str());

    info("Loading bins ...");
    Engine E[4];
    mc_ctx *tables[4];
    for (int t = 0; t < 4; t++) {  // loadGraph (SequenceCoverage.java:87-101)
        int mode = MC_KEY_PACKED;
        if (o.k > 31) {
            info("Reading hashes of k-mers instead");
            std::string h = o.hash;
            for (char &c : h) c = (char)tolower((unsigned char)c);
            if (h == "fnv1a") { info("Using FNV1a hash function"); mode = MC_KEY_FNV1A; }
            else { info("Using default polynomial hash function"); mode = MC_KEY_POLY; }
        }
        mc_config cfg{};
        cfg.k = o.k;
        cfg.key_mode = mode;
        cfg.device = o.device;
        cfg.capacity_hint = o.capacity_hint;
        E[t].open(cfg, {});
        tables[t] = E[t].c;
        MC_CHECK(tables[t], mc_set_read_pointers(tables[t], 0));  // (no walk: no read store)
        load_reads(*bins[t].files, E[t]);
        MC_CHECK(tables[t], mc_trim(tables[t]));  // (four tables fit where four sets of staging buffers would not)
    }

    info("Calculating sequence coverage...");
    ReadsIn reader(o, tables[0], o.read_file);
    FILE *out = fopen((out_dir + "/seq_cov.csv").c_str(), "w");
    if (!out) throw Error("cannot create " + out_dir + "/seq_cov.csv");
    struct Closer { FILE *f; ~Closer() { if (f) fclose(f); } } closer{out};
    fputs("name, from_donor_depth, from_donor_breadth, from_before_depth, from_before_breadth"
          ", from_both_depth, from_both_breadth, itself_depth, itself_breadth\n", out);
    // batches bounded by bases (a batch grows to hold one sequence that is longer); rows in input order
    constexpr uint64_t BATCH_BASES = 256ull << 20;
    constexpr size_t BATCH_SEQS = 1u << 22;
    DnaQBatch b;
    b.clear();
    for (;;) {
        if (reader.gpu) {  // (a batch a call: the device view is of the batch the call delivered)
            b.clear();
            if (reader.read(b, BATCH_SEQS, BATCH_BASES) == 0) break;
            seq_cov_batch(tables, b, o.k, out, &reader.gpu->segments());
            continue;
        }
        const size_t got = reader.read(b, 1);
        if (got == 0 || b.codes.size() >= BATCH_BASES || b.n_reads() >= BATCH_SEQS) {
            seq_cov_batch(tables, b, o.k, out);
            b.clear();
        }
        if (got == 0) break;
    }
    closer.f = nullptr;
    if (fclose(out) != 0) throw Error("cannot write seq_cov.csv");
    info("Processed all sequences...");
    write_file(o.work_dir + "/SUCCESS", "");
    return 0;
}

// --tool recipient-visualiser (src/tools/RecipientVisualiser.java:185-223, src/algo/SeqEnvCalculator.java): the environment of every
// sequence of --seq in the graph of the post-FMT reads (mc_bfs_batch: all eight neighbours, count > 0), every k-mer coloured by which
// of the four class tables hold it (mc_kmer_presence: one call a batch of sequences), one coloured GFA and one FASTA a sequence.
// The reference runs the sequences on a thread pool; each writes its own files, and the log lines here come in sequence order.
int run_recipient_visualiser(const Options &o)
{
    if (o.k < 0) throw Error("Parameter 'k' is mandatory");
    if (o.after_files.empty()) throw Error("Parameter 'after-files' is mandatory");
    if (o.seq.empty()) throw Error("Parameter 'seq' is mandatory");
    if (o.input_dir.empty()) throw Error("Parameter 'input-dir' is mandatory");
    if (o.ext.empty()) throw Error("Parameter 'ext' is mandatory");
    if (o.k < 1 || o.k > 63)
        throw Error("k = " + std::to_string(o.k) + " is not supported: this build handles k <= 31 (packed keys) and 32 <= k <= 63 (hash keys)");
    if (!o.devices.empty()) throw Error("--devices is for --tool environment-finder: recipient-visualiser keeps its five tables on one device (--device)");
    // (the class files, RecipientVisualiser.java:194-205: donor, baseline, both, itself are bits 0..3 of a k-mer's mask)
    const char *const classes[4] = {"came_from_donor", "came_from_baseline", "came_from_both", "came_itself"};
    std::vector<std::string> class_files[4];
    for (int t = 0; t < 4; t++)
        for (const char *part : {"_1.", "_2.", "_s."}) {
            class_files[t].push_back(o.input_dir + "/" + classes[t] + part + o.ext);
            FILE *f = fopen(class_files[t].back().c_str(), "rb");
            if (!f) throw Error("Could not read class file " + class_files[t].back());
            fclose(f);
        }
    if (!open_work_dir(o, "k=" + std::to_string(o.k) + "\nseq=" + o.seq + "\ninput-dir=" + o.input_dir + "\next=" + o.ext + "\n")) return 0;
    const std::string out_dir = (o.output_dir.empty() ? o.work_dir + "/graph" : o.output_dir) + "/after";
    const int64_t maxradius = o.maxradius < 0 ? 1000 : o.maxradius;  // (the parameter's default; --maxkmers has none)

    info("Loading after reads ...");
    int mode = MC_KEY_PACKED;
    if (o.k > 31) {  // loadAfterGraphs :108-123
        info("Reading hashes of k-mers instead");
        std::string h = o.hash;
        for (char &c : h) c = (char)tolower((unsigned char)c);
        if (h == "fnv1a") { info("Using FNV1a hash function"); mode = MC_KEY_FNV1A; }
        else { info("Using default polynomial hash function"); mode = MC_KEY_POLY; }
    }
    mc_config cfg{};
    cfg.k = o.k;
    cfg.key_mode = mode;
    cfg.device = o.device;
    cfg.capacity_hint = o.capacity_hint;
    Engine G, E[4];  // the graph, then the class tables: all five stay on the device
    G.open(cfg, {});
    G.set_coverage_hint(1);
    load_reads(o.after_files, G);
    MC_CHECK(G.c, mc_trim(G.c));
    mc_ctx *tables[4];
    cfg.capacity_hint = 0;
    Compaction compaction(o, G, o.k);
    for (int t = 0; t < 4; t++) {
        E[t].open(cfg, {});
        tables[t] = E[t].c;
        MC_CHECK(tables[t], mc_set_read_pointers(tables[t], 0));  // (no walk on these: no read store)
        load_reads(class_files[t], E[t]);
        MC_CHECK(tables[t], mc_trim(tables[t]));
    }

    // ReadersUtils.loadDnaQs: every record whole, N as A
    DnaQBatch seqs;
    seqs.clear();
    try {
        DnaQReader reader(o.seq);
        while (reader.read(seqs, 1u << 16)) {}
    } catch (const Error &) {
        throw Error("Could not load sequences from " + o.after_files[0]);  // (the reference names this file, :127)
    }
    const size_t n_seqs = seqs.n_reads();

    info("Creating after images ...");
    // Jobs a call: mc_bfs_batch gives every job device arrays for max(--maxkmers, its windows) + 512 vertices -- 2^20 when --maxkmers
    // is not given -- at some 64 bytes a vertex (k-mer, distance, coverage, flags, the visited index), and its result comes back in
    // host arrays of 23 bytes a vertex.  A call takes as many sequences as fit a quarter of the device memory that is free now that
    // the five tables are loaded: at most 256 (the environment-finder's chunk; beyond it a launch gains nothing), at least one.
    size_t free_b = 0, total_b = 0;
    hip_check(hipSetDevice(o.device), "hipSetDevice");
    hip_check(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo");
    uint64_t longest = 0;
    for (size_t s = 0; s < n_seqs; s++) longest = std::max<uint64_t>(longest, seqs.offsets[s + 1] - seqs.offsets[s]);
    const uint64_t per_job = 64 * ((o.maxkmers >= 0 ? std::max<uint64_t>((uint64_t)o.maxkmers, longest) : std::max<uint64_t>(1ull << 20, longest)) + 512);
    const size_t chunk = (size_t)std::min<uint64_t>(256, std::max<uint64_t>(1, free_b / 4 / per_job));
    const kmer_t kmask = o.k >= 64 ? ~(kmer_t)0 : (((kmer_t)1 << (2 * o.k)) - 1);

    for (size_t s0 = 0; s0 < n_seqs; s0 += chunk) {
        const size_t s1 = std::min(n_seqs, s0 + chunk);
        std::vector<std::string> text(s1 - s0);
        std::vector<std::vector<uint64_t>> shi(s1 - s0), slo(s1 - s0);
        std::vector<mc_bfs_job> jobs;
        for (size_t s = s0; s < s1; s++) {
            std::string &t = text[s - s0];
            for (uint64_t i = seqs.offsets[s]; i < seqs.offsets[s + 1]; i++) t.push_back("AGCT"[seqs.codes[i] & 3]);  // DnaQ.toString()
            kmer_t v = 0;
            for (size_t i = 0; i < t.size(); i++) {
                v = ((v << 2) | (seqs.codes[seqs.offsets[s] + i] & 3u)) & kmask;
                if (i + 1 >= (size_t)o.k) { shi[s - s0].push_back((uint64_t)(v >> 64)); slo[s - s0].push_back((uint64_t)v); }
            }
            jobs.push_back(mc_bfs_job{shi[s - s0].data(), slo[s - s0].data(), shi[s - s0].size(), 0});
        }
        std::vector<mc_bfs_result> res(jobs.size());
        struct ResGuard {  // (an exception below must not leak the library's result arrays)
            std::vector<mc_bfs_result> &r;
            ~ResGuard() { for (auto &x : r) mc_bfs_result_free(&x); }
        } guard{res};
        G.bfs_batch(jobs.data(), (uint32_t)jobs.size(), 1, o.maxkmers, maxradius, res.data());

        // the colours of the whole batch: one call over the concatenated results
        std::vector<uint64_t> qhi, qlo;
        std::vector<size_t> at(res.size() + 1, 0);
        for (size_t j = 0; j < res.size(); j++) {
            qhi.insert(qhi.end(), res[j].hi, res[j].hi + res[j].n);
            qlo.insert(qlo.end(), res[j].lo, res[j].lo + res[j].n);
            at[j + 1] = qlo.size();
        }
        std::vector<uint8_t> mask(qlo.size());
        if (!qlo.empty()) MC_CHECK(tables[0], mc_kmer_presence(tables, 4, qhi.data(), qlo.data(), qlo.size(), mask.data()));

        // the subgraphs, and what extendEnvironment asks the graph: again one call for the batch
        std::vector<std::unique_ptr<Environment>> envs(res.size());
        std::vector<Environment::Outside> outside(res.size());
        std::vector<std::map<kmer_t, uint8_t>> mask_of(res.size());
        std::vector<size_t> oat(res.size() + 1, 0);
        qhi.clear();
        qlo.clear();
        for (size_t j = 0; j < res.size(); j++) {
            const mc_bfs_result &r = res[j];
            if (r.n) {
                envs[j].reset(new Environment(o.k, {text[j]}));
                BfsPass p;
                p.dir = 0;
                p.kmers.reserve(r.n);
                for (uint64_t i = 0; i < r.n; i++) {
                    p.kmers.push_back(((kmer_t)r.hi[i] << 64) | r.lo[i]);
                    mask_of[j][normalize128(p.kmers.back(), o.k)] = mask[at[j] + i];
                }
                p.dist.assign(r.dist, r.dist + r.n);
                p.cov.assign(r.cov, r.cov + r.n);
                p.last.assign(r.n, 0);
                envs[j]->add_pass(p, false);
                outside[j] = envs[j]->outside_neighbours();
                for (const kmer_t x : outside[j].kmers) { qhi.push_back((uint64_t)(x >> 64)); qlo.push_back((uint64_t)x); }
            }
            oat[j + 1] = qlo.size();
        }
        std::vector<uint8_t> in_graph(qlo.size());
        mc_ctx *graph[1] = {G.c};
        if (!qlo.empty()) MC_CHECK(G.c, mc_kmer_presence(graph, 1, qhi.data(), qlo.data(), qlo.size(), in_graph.data()));

        for (size_t j = 0; j < res.size(); j++) {
            info("Finding environment for sequence " + shorten_label(text[j], o.k));
            if (!envs[j]) {
                info("Could not find any k-mers of the target gene in the input, halting.");
                continue;
            }
            Environment &env = *envs[j];
            info("Extending endings by " + std::to_string(Environment::extensions(outside[j], in_graph.data() + oat[j])) + " kmers");
            env.set_colours([&](kmer_t kmer) { return Environment::colour_of_mask(mask_of[j].at(kmer)); });
            env.create_picture(compaction.pick(env.size(), "comp_" + std::to_string(s0 + j)));
            const std::string name = out_dir + "/comp_" + std::to_string(s0 + j);
            write_file(name + "_seqs.fasta", env.seqs_fasta(0));  // (no chunk-length filter here: SeqEnvCalculator.java:258)
            write_file(name + ".gfa", env.graph_gfa());
            envs[j].reset();
        }
    }
    info("Finished processing all sequences!");
    write_file(o.work_dir + "/SUCCESS", "");
    return 0;
}

// --tool fmt-visualizer (src/tools/FMTVisualizer.java:223-317, src/algo/KmerEnvCalculator.java): for the donor, the pre-FMT and the
// post-FMT reads in turn, one coloured GFA and one FASTA a connected component of the phase's graph.  The reference walks from every
// window whose count is still above 0 and zeroes what it reaches; here mc_components gives the components with their seeds at once,
// mc_kmer_presence the class tables of every member, and only what the walk's ORDER decides is replayed on the host, a component
// at a time on -p threads (the reference cannot: every walk writes the one shared map): the FIFO without a visited set over the
// component's own k-mer -> count map, which gives the order of the subgraph's puts and the coverage 0 of a k-mer popped twice.

// KmerEnvCalculator.runBfs (:60-76) over one component: `canon` sorted, `count` beside it (zeroed here); the puts in pop order
std::vector<std::pair<kmer_t, int>> replay_component_walk(int k, kmer_t seed, const std::vector<kmer_t> &canon, std::vector<int> &count)
{
    const kmer_t kmask = ((kmer_t)1 << (2 * k)) - 1;
    const int top = 2 * (k - 1);
    auto at = [&](kmer_t v) -> int {
        const kmer_t c = normalize128(v, k);
        const auto it = std::lower_bound(canon.begin(), canon.end(), c);
        return it != canon.end() && *it == c ? (int)(it - canon.begin()) : -1;
    };
    std::vector<kmer_t> queue{seed};
    std::vector<std::pair<kmer_t, int>> puts;
    for (size_t head = 0; head < queue.size(); head++) {
        const kmer_t kmer = queue[head];
        for (unsigned c = 0; c < 4; c++) {  // allNeighbors: A, G, C, T, the left neighbour before the right one
            const kmer_t nb[2] = {((kmer_t)c << top) | (kmer >> 2), ((kmer << 2) & kmask) | c};
            for (const kmer_t x : nb) {
                const int e = at(x);
                if (e >= 0 && count[(size_t)e] > 0) queue.push_back(x);
            }
        }
        const int e = at(kmer);  // (a member: it was queued with a count above 0)
        puts.emplace_back(kmer, count[(size_t)e]);
        count[(size_t)e] = 0;  // addAndBound(key, -get)
    }
    return puts;
}

void fmt_phase(const Options &o, int mode, const std::string &name, const std::vector<std::string> &files, const std::vector<std::string> &classes,
               const std::string &out_root)
{
    info("Loading " + name + " reads ...");
    if (o.k > 31) {
        info("Reading hashes of k-mers instead");
        info(mode == MC_KEY_FNV1A ? "Using FNV1a hash function" : "Using default polynomial hash function");
    }
    const uint32_t nt = (uint32_t)classes.size();
    std::vector<std::vector<std::string>> class_files(nt);
    for (uint32_t t = 0; t < nt; t++)
        for (const char *part : {"_1.", "_2.", "_s."}) {
            class_files[t].push_back(o.input_dir + "/" + classes[t] + part + o.ext);
            FILE *f = fopen(class_files[t].back().c_str(), "rb");
            if (!f) throw Error("Could not read class file " + class_files[t].back());
            fclose(f);
        }
    mc_config cfg{};
    cfg.k = o.k;
    cfg.key_mode = mode;
    cfg.device = o.device;
    cfg.capacity_hint = o.capacity_hint;
    Engine G, E[4];  // the graph, then the two or four class tables: all on the device until the phase ends
    G.open(cfg, {});
    MC_CHECK(G.c, mc_set_read_pointers(G.c, 0));  // (nothing walks these tables: no read store)
    load_reads(files, G);
    MC_CHECK(G.c, mc_trim(G.c));
    mc_ctx *tables[4] = {};
    Compaction compaction(o, G, o.k);
    cfg.capacity_hint = 0;
    for (uint32_t t = 0; t < nt; t++) {
        E[t].open(cfg, {});
        tables[t] = E[t].c;
        MC_CHECK(tables[t], mc_set_read_pointers(tables[t], 0));
        load_reads(class_files[t], E[t]);
        MC_CHECK(tables[t], mc_trim(tables[t]));
    }
    // ReadersUtils.loadDnaQs: the phase's reads again, every record whole, N as A
    DnaQBatch seqs;
    seqs.clear();
    // --parse gpu (every file of the phase, or none): the reads stay on the device, joined into one array for mc_components_dev
    bool on_gpu = !files.empty();
    for (const std::string &f : files) on_gpu = parse_on_gpu(o, f) && on_gpu;
    SideStore dev_seqs;
    try {
        for (const std::string &f : files) {
            if (on_gpu) {
                WholeReadsSource src(G.c, o.device, f, false);
                DnaQBatch b;
                for (;;) {
                    b.clear();
                    const size_t got = src.read(b, 1u << 20);
                    if (got == 0) break;
                    dev_seqs.add_dev(G.c, src.segments(), b, got, false);
                }
                continue;
            }
            DnaQReader reader(f);
            while (reader.read(seqs, 1u << 16)) {}
        }
    } catch (const Error &) {
        throw Error("Could not load sequences from " + o.donor_files[0]);  // (all three phases name this file, :117,137,161)
    }
    info("Creating " + name + " image ...");
    const uint64_t n_bases = seqs.codes.size();
    std::vector<uint64_t> words(n_bases / 32 + 2, 0);
    for (uint64_t i = 0; i < n_bases; i++) words[i >> 5] |= (uint64_t)(seqs.codes[i] & 3u) << (62 - 2 * (i & 31));
    mc_components_result res{};
    struct ResGuard {
        mc_components_result &r;
        ~ResGuard() { mc_components_free(&r); }
    } guard{res};
    if (on_gpu) MC_CHECK(G.c, mc_components_dev(G.c, dev_seqs.words.as<uint64_t>(), dev_seqs.offsets.as<uint64_t>(), dev_seqs.n_reads, &res));
    else MC_CHECK(G.c, mc_components(G.c, words.data(), seqs.offsets.data(), seqs.n_reads(), &res));
    std::vector<uint8_t> mask(res.n_kmers);
    if (res.n_kmers) MC_CHECK(tables[0], mc_kmer_presence(tables, nt, res.hi, res.lo, res.n_kmers, mask.data()));
    const std::string out_dir = out_root + "/" + name;
    std::atomic<uint64_t> next{0};
    std::mutex err_mu;
    std::string err;
    auto work = [&] {
        for (uint64_t c; (c = next.fetch_add(1)) < res.n_components;) {
            try {
                const uint64_t a = res.comp_offsets[c], b = res.comp_offsets[c + 1];
                std::vector<std::pair<kmer_t, uint64_t>> order;  // (canonical k-mer, member)
                order.reserve(b - a);
                for (uint64_t i = a; i < b; i++) order.emplace_back(normalize128(((kmer_t)res.hi[i] << 64) | res.lo[i], o.k), i);
                std::sort(order.begin(), order.end());
                std::vector<kmer_t> canon;
                std::vector<int> count;
                for (const auto &e : order) { canon.push_back(e.first); count.push_back(res.cov[e.second]); }
                const kmer_t seed = ((kmer_t)res.hi[a] << 64) | res.lo[a];
                Environment env(o.k, {});
                env.add_puts(replay_component_walk(o.k, seed, canon, count));
                env.set_colours([&](kmer_t kmer) {
                    const auto it = std::lower_bound(canon.begin(), canon.end(), kmer);
                    const unsigned m = mask[order[(size_t)(it - canon.begin())].second];
                    if (nt == 4) return Environment::colour_of_mask(m);
                    // getDonorColorNode / getBeforeColorNode (:195-207): bit 0 the found class (settle, stay), bit 1 the other
                    return m == 1 ? Environment::GREEN : m == 2 ? Environment::BLUE : m == 3 ? Environment::GREY : Environment::BLACK;
                });
                env.create_picture(compaction.pick(env.size(), "comp" + std::to_string(c)));
                const std::string file = out_dir + "/comp" + std::to_string(c);
                write_file(file + "_seqs.fasta", env.seqs_fasta(1));
                write_file(file + ".gfa", env.graph_gfa());
            } catch (const std::exception &e) {
                std::lock_guard<std::mutex> g(err_mu);
                if (err.empty()) err = e.what();
            }
        }
    };
    if (res.n_components) write_file(out_dir + "/comp0.gfa", "");  // (the directory, made once before the threads write into it)
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const uint64_t n_threads = std::max<uint64_t>(1, std::min<uint64_t>(o.processors > 0 ? (uint64_t)o.processors : std::min(hw, 16u), res.n_components));
    std::vector<std::thread> pool;
    for (uint64_t t = 1; t < n_threads; t++) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
    if (!err.empty()) throw Error(err);
}

int run_fmt_visualizer(const Options &o)
{
    if (o.k < 0) throw Error("Parameter 'k' is mandatory");
    if (o.donor_files.empty()) throw Error("Parameter 'donor-files' is mandatory");
    if (o.before_files.empty()) throw Error("Parameter 'before-files' is mandatory");
    if (o.after_files.empty()) throw Error("Parameter 'after-files' is mandatory");
    if (o.input_dir.empty()) throw Error("Parameter 'input-dir' is mandatory");
    if (o.ext.empty()) throw Error("Parameter 'ext' is mandatory");
    if (o.k < 1 || o.k > 63)
        throw Error("k = " + std::to_string(o.k) + " is not supported: this build handles k <= 31 (packed keys) and 32 <= k <= 63 (hash keys)");
    if (!o.devices.empty()) throw Error("--devices is for --tool environment-finder: fmt-visualizer keeps a phase's tables on one device (--device)");
    if (!open_work_dir(o, "k=" + std::to_string(o.k) + "\ninput-dir=" + o.input_dir + "\next=" + o.ext + "\n")) return 0;
    const std::string out_root = o.output_dir.empty() ? o.work_dir + "/graph" : o.output_dir;
    int mode = MC_KEY_PACKED;
    if (o.k > 31) {
        std::string h = o.hash;
        for (char &c : h) c = (char)tolower((unsigned char)c);
        mode = h == "fnv1a" ? MC_KEY_FNV1A : MC_KEY_POLY;
    }
    fmt_phase(o, mode, "donor", o.donor_files, {"settle", "not_settle"}, out_root);
    fmt_phase(o, mode, "before", o.before_files, {"stay", "gone"}, out_root);
    fmt_phase(o, mode, "after", o.after_files, {"came_from_donor", "came_from_baseline", "came_from_both", "came_itself"}, out_root);
    write_file(o.work_dir + "/SUCCESS", "");
    return 0;
}

// --tool environment-assembler-finder (src/tools/EnvironmentAssemblerFinder.java:175-240): the environment of one sequence, then every
// read of every --reads file tested against it (src/algo/ReadsFilter.java: mc_reads_in_set_dev, whole reads in batches, the set of
// the environment's k-mers on the device once a phase) and the reads that belong to it written to <output>/cutReads<i>.fasta; with
// --assembler, their assembly (src/algo/AssemblerCalculator.java) and all of it again at k = 55 with the contigs as the reads.

// a child process as ProcessBuilder starts it -- argv as given, no shell, stderr into stdout -- every line of its output logged
void run_logged(const std::vector<std::string> &argv)
{
    int fds[2];
    if (pipe(fds) != 0) throw Error("pipe: " + std::string(strerror(errno)));
    posix_spawn_file_actions_t fa;
    posix_spawn_file_actions_init(&fa);
    posix_spawn_file_actions_addclose(&fa, fds[0]);
    posix_spawn_file_actions_adddup2(&fa, fds[1], 1);
    posix_spawn_file_actions_adddup2(&fa, fds[1], 2);
    posix_spawn_file_actions_addclose(&fa, fds[1]);
    std::vector<char *> av;
    for (const std::string &a : argv) av.push_back(const_cast<char *>(a.c_str()));
    av.push_back(nullptr);
    pid_t pid = 0;
    const int rc = posix_spawnp(&pid, av[0], &fa, nullptr, av.data(), environ);
    posix_spawn_file_actions_destroy(&fa);
    close(fds[1]);
    if (rc != 0) {  // (the reference catches the IOException, logs its message and goes on)
        close(fds[0]);
        info("Cannot run program \"" + argv[0] + "\": " + strerror(rc));
        return;
    }
    FILE *f = fdopen(fds[0], "r");
    std::string line;
    for (int c; f && (c = fgetc(f)) != EOF;) {
        if (c == '\n') { info(line); line.clear(); }
        else line.push_back((char)c);
    }
    if (!line.empty()) info(line);
    if (f) fclose(f); else close(fds[0]);
    int status = 0;
    while (waitpid(pid, &status, 0) < 0 && errno == EINTR) {}
}

// AssemblerCalculator.runAssembler (:28-97) for reads file i: the assembler, then the `mv` of its contigs.  The reference names
// cutReads<i>.fastq although ReadsFilter writes cutReads<i>.fasta (DESIGN.md "environment-assembler-finder"): the argv is kept.
void run_assembler(const Options &o, const std::string &prefix, size_t i)
{
    const std::string n = std::to_string(i);
    if (o.assembler == "spades") {
        run_logged({"python", o.assemblerpath + "/spades.py", "--12", prefix + "cutReads" + n + ".fastq", "-o", prefix + "out_spades" + n});
        run_logged({"mv", prefix + "out_spades" + n + "/contigs.fasta", prefix + "contigs" + n + ".fasta"});
    }
    if (o.assembler == "megahit") {
        run_logged({o.assemblerpath + "/megahit", "--12", prefix + "cutReads" + n + ".fastq", "-o", prefix + "out_megahit" + n});
        run_logged({"mv", prefix + "out_megahit" + n + "/final.contigs.fa", prefix + "contigs" + n + ".fasta"});
    }
}

// one batch of whole reads through mc_reads_in_set_dev; the kept ones go to the writer
void filter_batch(mc_ctx *ctx, const DnaQBatch &b, const DevArray &set_hi, const DevArray &set_lo, uint64_t n_set, int k, int pct, DevArray &dev,
                  CutReadsWriter &out, const std::vector<WholeSegment> *segs = nullptr)
{
    const size_t n = b.n_reads();
    if (n == 0) return;
    if (segs) {  // --parse gpu: the batch's device view, a segment a launch; hits and keep in one block
        dev.size = 0;
        dev.reserve(n * 4 + n);
        for (const WholeSegment &g : *segs)
            MC_CHECK(ctx, mc_reads_in_set_dev(ctx, g.d_words, g.d_offsets, g.n_reads, k > 32 ? set_hi.as<uint64_t>() : nullptr, set_lo.as<uint64_t>(), n_set, pct,
                                              0, dev.as<uint32_t>() + g.first, reinterpret_cast<uint8_t *>(dev.p + n * 4) + g.first));
        std::vector<uint8_t> keep(n);
        hip_check(hipMemcpy(keep.data(), dev.p + n * 4, n, hipMemcpyDeviceToHost), "hipMemcpy");
        for (size_t r = 0; r < n; r++)
            if (keep[r]) out.add(b.codes.data() + b.offsets[r], (size_t)(b.offsets[r + 1] - b.offsets[r]));
        return;
    }
    const uint64_t n_bases = b.offsets[n];
    std::vector<uint64_t> words((n_bases + 31) / 32 + 1, 0);
    for (uint64_t i = 0; i < n_bases; i++) words[i >> 5] |= (uint64_t)(b.codes[i] & 3) << (62 - 2 * (i & 31));
    // one block of device memory a batch: words, offsets, hits, keep
    const size_t at_off = words.size() * 8, at_hits = at_off + (n + 1) * 8, at_keep = at_hits + n * 4;
    dev.size = 0;
    dev.reserve(at_keep + n);
    dev.put(0, words.data(), words.size() * 8);
    dev.put(at_off, b.offsets.data(), (n + 1) * 8);
    MC_CHECK(ctx, mc_reads_in_set_dev(ctx, dev.as<uint64_t>(), reinterpret_cast<uint64_t *>(dev.p + at_off), n, k > 32 ? set_hi.as<uint64_t>() : nullptr,
                                      set_lo.as<uint64_t>(), n_set, pct, 0, reinterpret_cast<uint32_t *>(dev.p + at_hits),
                                      reinterpret_cast<uint8_t *>(dev.p + at_keep)));
    std::vector<uint8_t> keep(n);
    hip_check(hipMemcpy(keep.data(), dev.p + at_keep, n, hipMemcpyDeviceToHost), "hipMemcpy");
    for (size_t r = 0; r < n; r++)
        if (keep[r]) out.add(b.codes.data() + b.offsets[r], (size_t)(b.offsets[r + 1] - b.offsets[r]));
}

// loadInput + one OneSequenceCalculator + one ReadsFilter a file (EnvironmentAssemblerFinder.java:176-201, again :225-239).
// false: more than one sequence, nothing was written.
bool assembler_finder_phase(const Options &o, int k, int coverage, const std::vector<std::string> &reads, const std::string &prefix)
{
    const bool hashed = k > 31 || o.forcehash;
    int mode = MC_KEY_PACKED;
    if (hashed) {
        info("Reading hashes of k-mers instead");
        std::string h = o.hash;
        for (char &c : h) c = (char)tolower((unsigned char)c);
        if (h == "fnv1a") { info("Using FNV1a hash function"); mode = MC_KEY_FNV1A; }
        else { info("Using default polynomial hash function"); mode = MC_KEY_POLY; }
    }
    mc_config cfg{};
    cfg.k = k;
    cfg.key_mode = mode;
    cfg.device = o.device;
    cfg.capacity_hint = o.capacity_hint;
    Engine E;
    E.open(cfg, {});
    Compaction compaction(o, E, k);
    const Trimmer trimmer(o, E);
    E.set_coverage_hint(coverage);
    load_reads(reads, E);

    // ReadersUtils.loadDnaQs: every record whole, N as A (not the rich FASTA reader of environment-finder)
    DnaQBatch seqs;
    seqs.clear();
    try {
        DnaQReader reader(o.seq);
        while (reader.read(seqs, 1u << 16)) {}
    } catch (const Error &) {
        throw Error("Could not load sequences from " + o.seq);
    }
    if (seqs.n_reads() > 1) {
        info("EnvironmentAssemblerFinder works only with one input sequence!");
        return false;
    }
    if (seqs.n_reads() == 0) throw Error("No sequence in " + o.seq);
    std::string seq;
    for (uint64_t i = 0; i < seqs.offsets[1]; i++) seq.push_back("AGCT"[seqs.codes[i] & 3]);

    // OneSequenceCalculator.run (:137-144), as environment-finder runs one calculator
    info("Finding environment for sequence " + shorten_label(seq, k));
    std::vector<uint64_t> shi, slo;
    for (size_t i = 0; i + (size_t)k <= seq.size(); i++) {
        uint64_t hi, lo;
        pack_kmer(seq.substr(i, (size_t)k), &hi, &lo);
        shi.push_back(hi);
        slo.push_back(lo);
    }
    const std::vector<int> dirs = pass_dirs(o.bothdirs);
    std::vector<mc_bfs_job> jobs;
    for (int d : dirs) jobs.push_back(mc_bfs_job{shi.data(), slo.data(), shi.size(), d});
    std::vector<mc_bfs_result> res(jobs.size());
    struct ResGuard {  // (an exception below must not leak the library's result arrays)
        std::vector<mc_bfs_result> &r;
        ~ResGuard() { for (auto &x : r) mc_bfs_result_free(&x); }
    } guard{res};
    E.bfs_batch(jobs.data(), (uint32_t)jobs.size(), coverage, o.maxkmers, o.maxradius, res.data());
    Environment env(k, {seq});
    bool fail = false;
    for (size_t d = 0; d < dirs.size() && !fail; d++) {
        const mc_bfs_result &r = res[d];
        if (r.n == 0) { fail = true; break; }  // runBfs: queue.size() == 0 -> fail (:193-196)
        BfsPass p;
        p.dir = dirs[d];
        p.kmers.reserve(r.n);
        for (uint64_t i = 0; i < r.n; i++) p.kmers.push_back(((kmer_t)r.hi[i] << 64) | r.lo[i]);
        p.dist.assign(r.dist, r.dist + r.n);
        p.cov.assign(r.cov, r.cov + r.n);
        p.last.assign(r.last, r.last + r.n);
        trimmer.add_pass(env, p, r);
    }
    std::vector<kmer_t> members;
    if (fail) {  // (the calculator stops there: no graph files, and an empty subgraph for the filter)
        info("Could not find any k-mers of the target gene in the input, halting.");
    } else {
        info("Extending endings by 0 kmers");
        if (!env.order_guaranteed())
            logline("WARN", "--trim removed k-mers from a treeified java.util.HashMap bin: line order of " + prefix + " may differ from the JVM's inside that bin");
        members = env.kmers();
        env.write_all(prefix, o.chunklength, compaction.pick(env.size(), prefix));
    }

    // the set goes up once; every file's reads stream through in batches
    std::vector<uint64_t> mhi(members.size()), mlo(members.size());
    for (size_t i = 0; i < members.size(); i++) { mhi[i] = (uint64_t)(members[i] >> 64); mlo[i] = (uint64_t)members[i]; }
    hip_check(hipSetDevice(o.device), "hipSetDevice");
    DevArray set_hi, set_lo, dev;
    set_hi.put(0, mhi.data(), mhi.size() * 8);
    set_lo.put(0, mlo.data(), mlo.size() * 8);
    set_hi.reserve(8);
    set_lo.reserve(8);  // (an empty set still has an address)
    constexpr uint64_t BATCH_BASES = 256ull << 20;
    constexpr size_t BATCH_READS = 1u << 22;
    for (size_t i = 0; i < reads.size(); i++) {
        CutReadsWriter out(prefix + "cutReads" + std::to_string(i) + ".fasta", (int)i);
        ReadsIn reader(o, E.c, reads[i]);
        DnaQBatch b;
        b.clear();
        for (;;) {
            if (reader.gpu) {  // (a batch a call: the device view is of the batch the call delivered)
                b.clear();
                if (reader.read(b, BATCH_READS, BATCH_BASES) == 0) break;
                filter_batch(E.c, b, set_hi, set_lo, members.size(), k, (int)o.procfiltration, dev, out, &reader.gpu->segments());
                continue;
            }
            const size_t got = reader.read(b, 1u << 14);
            if (got == 0 || b.codes.size() >= BATCH_BASES || b.n_reads() >= BATCH_READS) {
                filter_batch(E.c, b, set_hi, set_lo, members.size(), k, (int)o.procfiltration, dev, out);
                b.clear();
            }
            if (got == 0) break;
        }
        out.close();
    }
    info("Filtration done!");
    info("Finished processing all sequences!");
    return true;
}

int run_assembler_finder(const Options &o)
{
    if (o.k < 0) throw Error("Parameter 'k' is mandatory");
    if (o.seq.empty()) throw Error("Parameter 'seq' is mandatory");
    if (o.output.empty()) throw Error("Parameter 'output' is mandatory");
    if (!o.devices.empty()) throw Error("--devices is for --tool environment-finder: environment-assembler-finder filters the reads on one device (--device)");
    if (o.k < 1 || o.k > 63)
        throw Error("k = " + std::to_string(o.k) + " is not supported: this build handles k <= 31 (packed keys) and 32 <= k <= 63 (hash keys)");
    if (o.procfiltration < 0 || o.procfiltration > 100) throw Error("--procfiltration must be a percentage, 0 .. 100");
    if (o.maxkmers < 0 && o.maxradius < 0)  // EnvironmentAssemblerFinder.java:163-165
        throw Error("At least one of --maxkmers and --maxradius parameters should be set");
    if (o.coverage < 0) throw Error("--coverage must not be negative (absent k-mers read as -1 and would pass)");
    if (o.assembler.empty() != o.assemblerpath.empty()) throw Error("--assembler and --assemblerpath go together");
    if (!open_work_dir(o, "k=" + std::to_string(o.k) + "\nseq=" + o.seq + "\noutput=" + o.output + "\ncoverage=" + std::to_string(o.coverage) +
                              "\nprocfiltration=" + std::to_string(o.procfiltration) + "\n"))
        return 0;
    const std::string prefix = o.output + "/";
    if (!assembler_finder_phase(o, o.k, o.coverage, o.reads, prefix)) return 0;
    if (o.assembler.empty()) {  // (mandatory in the reference; here the filter alone is a use of its own)
        write_file(o.work_dir + "/SUCCESS", "");
        return 0;
    }
    for (size_t i = 0; i < o.reads.size(); i++) run_assembler(o, prefix, i);
    info("Finished assembling all sequences!");
    // :216-239: the contigs are the reads now, k = 55, every k-mer counts
    std::vector<std::string> contigs;
    for (size_t i = 0; i < o.reads.size(); i++) {
        contigs.push_back(prefix + "contigs" + std::to_string(i) + ".fasta");
        struct stat st;
        if (stat(contigs.back().c_str(), &st) != 0) throw Error("The assembler left no " + contigs.back() + ": the second stage needs it");
    }
    assembler_finder_phase(o, 55, 0, contigs, prefix + "result/");
    write_file(o.work_dir + "/SUCCESS", "");
    return 0;
}

int run(const Options &o)
{
    if (o.compact_given && (o.tool == "kmer-counter" || o.tool == "environment-finder-multi"))  // (they share environment-finder's table)
        throw Error("--compact does not apply to --tool " + o.tool);
    if (o.trim_on_given && (o.tool == "kmer-counter" || o.tool == "environment-finder-multi")) throw Error("--trim-on does not apply to --tool " + o.tool);
    if (o.trim && o.trim_on == "gpu" && !o.devices.empty())  // (a group has no single context to run mc_trim_paths on)
        throw Error("--trim-on gpu does not go with --devices: the trim of a group's walk runs on the host (--trim-on host or auto)");
    if (o.join_given && o.tool != "environment-finder-multi") throw Error("--join does not apply to --tool " + o.tool);
    if (o.kmers_io_given && o.tool != "kmer-counter" && o.tool != "reads-classifier" && o.tool != "triple-reads-classifier")
        throw Error("--kmers-io does not apply to --tool " + o.tool);
    if (o.parse_given && o.tool != "reads-classifier" && o.tool != "triple-reads-classifier" && o.tool != "seq-cov" && o.tool != "fmt-visualizer" &&
        o.tool != "environment-assembler-finder")
        throw Error("--parse does not apply to --tool " + o.tool);
    if (o.render_given && o.tool != "reads-classifier" && o.tool != "triple-reads-classifier") throw Error("--render does not apply to --tool " + o.tool);
    if (o.tool == "kmer-counter") return run_kmer_counter(o);
    if (o.tool == "environment-finder-multi") return run_multi(o);
    if (o.tool == "reads-classifier") return run_reads_classifier(o);
    if (o.tool == "triple-reads-classifier") return run_triple_reads_classifier(o);
    if (o.tool == "seq-cov") return run_seq_cov(o);
    if (o.tool == "recipient-visualiser") return run_recipient_visualiser(o);
    if (o.tool == "environment-assembler-finder") return run_assembler_finder(o);
    if (o.tool == "fmt-visualizer") return run_fmt_visualizer(o);
    if (o.tool != "environment-finder")
        throw Error("Tool '" + o.tool + "' is not part of this build: only environment-finder, kmer-counter, environment-finder-multi, "
                    "reads-classifier, triple-reads-classifier, recipient-visualiser, environment-assembler-finder, fmt-visualizer and seq-cov are");
    if (o.k < 0) throw Error("Parameter 'k' is mandatory");
    if (o.seq.empty()) throw Error("Parameter 'seq' is mandatory");
    if (o.output.empty()) throw Error("Parameter 'output' is mandatory");
    if (o.maxkmers < 0 && o.maxradius < 0)  // EnvironmentFinderMain.java:171-175
        throw Error("At least one of --maxkmers and --maxradius parameters should be set");
    if (o.coverage < 0) throw Error("--coverage must not be negative (absent k-mers read as -1 and would pass)");
    if (o.k > 63)  // (the reference hashes k-mer STRINGS of any length for k > 31; the walk here keeps oriented k-mers in 128 bits)
        throw Error("k = " + std::to_string(o.k) + " is not supported: this build handles k <= 31 (packed keys) and 32 <= k <= 63 (hash keys)");

    const std::string wd = o.work_dir;
    if (!open_work_dir(o, "k=" + std::to_string(o.k) + "\nseq=" + o.seq + "\noutput=" + o.output + "\ncoverage=" +
                              std::to_string(o.coverage) + "\nbothdirs=" + (o.bothdirs ? "true" : "false") + "\n"))
        return 0;

    // loadInput (EnvironmentFinderMain.java:127-154)
    const bool hashed = o.k > 31 || o.forcehash;
    int mode = MC_KEY_PACKED;
    if (hashed) {
        info("Reading hashes of k-mers instead");
        std::string h = o.hash;
        for (char &c : h) c = (char)tolower((unsigned char)c);
        if (h == "fnv1a") { info("Using FNV1a hash function"); mode = MC_KEY_FNV1A; }
        else { info("Using default polynomial hash function"); mode = MC_KEY_POLY; }
    }
    mc_config cfg{};
    cfg.k = o.k;
    cfg.key_mode = mode;
    cfg.device = o.device;
    cfg.capacity_hint = o.capacity_hint;
    Engine E;
    E.open(cfg, o.devices);
    Compaction compaction(o, E, o.k);
    const Trimmer trimmer(o, E);
    if (!o.devices.empty()) info("Counting on " + std::to_string(o.devices.size()) + " devices");
    E.set_coverage_hint(o.coverage);

    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t n_distinct = load_reads(o.reads, E);
    logline("DEBUG", "k-mers HM size = " + group_digits(n_distinct));
    const auto t1 = std::chrono::steady_clock::now();

    SeedFile seeds;
    try {
        seeds = read_seed_fasta(o.seq);
    } catch (const Error &) {
        throw Error("Could not load sequences from " + o.seq);
    }
    SeedFile hic;
    std::vector<std::string> comments = seeds.comments;
    if (!o.hicseq.empty()) {
        try {
            hic = read_seed_fasta(o.hicseq);
        } catch (const Error &) {
            throw Error("Could not load Hi-C sequences from " + o.hicseq);
        }
        comments = hic.comments;  // the reference overwrites the comments (EnvironmentFinderMain.java:149)
    }

    // runImpl (:185-243): one calculator per sequence, or one for all with --merge
    struct Calc { std::string out_prefix; std::vector<std::string> bfs_seqs, genes; };
    std::vector<Calc> calcs;
    if (!o.merge) {
        for (size_t i = 0; i < seeds.dnas.size(); i++) {
            if (i >= comments.size()) throw Error("sequence " + std::to_string(i) + " has no FASTA comment to name its output directory");
            calcs.push_back(Calc{o.output + "/" + comments[i] + "/", {seeds.dnas[i]}, {seeds.dnas[i]}});
        }
    } else {
        info("hicSequences = " + std::to_string(hic.dnas.size()));
        Calc c{o.output + "/merged/", seeds.dnas, seeds.dnas};
        c.bfs_seqs.insert(c.bfs_seqs.end(), hic.dnas.begin(), hic.dnas.end());
        calcs.push_back(c);
    }
    const std::vector<int> dirs = pass_dirs(o.bothdirs);
    // The passes of up to CHUNK_JOBS / dirs calculators go to the GPU in one batch (the reference runs one
    // OneSequenceCalculator per sequence on a thread pool, EnvironmentFinderMain.java:218-225, without a limit on their
    // number): a chunk's environments are written and its results freed before the next one starts, so neither the job
    // count of mc_bfs_batch nor the memory of the per-job arrays grows with the number of seed sequences.
    constexpr size_t CHUNK_JOBS = 256;
    const size_t calcs_per_chunk = std::max<size_t>(1, CHUNK_JOBS / dirs.size());
    double bfs_ms = 0, out_ms = 0;
    unsigned long long bfs_rounds = 0, bfs_levels = 0;  // (metrics.json: how well the walks' look-ahead did -- levels per verification round)
    auto ms_between = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    for (size_t c0 = 0; c0 < calcs.size(); c0 += calcs_per_chunk) {
        const size_t c1 = std::min(calcs.size(), c0 + calcs_per_chunk);
        const auto tb0 = std::chrono::steady_clock::now();
        std::vector<std::vector<uint64_t>> shi(c1 - c0), slo(c1 - c0);
        std::vector<mc_bfs_job> jobs;
        for (size_t c = c0; c < c1; c++) {
            if (!o.merge) info("Finding environment for sequence " + shorten_label(calcs[c].bfs_seqs[0], o.k));
            else info("Finding single environment for " + std::to_string(seeds.dnas.size()) + " sequences");
            for (const std::string &s : calcs[c].bfs_seqs)
                for (size_t i = 0; i + (size_t)o.k <= s.size(); i++) {
                    uint64_t hi, lo;
                    pack_kmer(s.substr(i, (size_t)o.k), &hi, &lo);
                    shi[c - c0].push_back(hi);
                    slo[c - c0].push_back(lo);
                }
            for (int d : dirs) jobs.push_back(mc_bfs_job{shi[c - c0].data(), slo[c - c0].data(), shi[c - c0].size(), d});
        }
        std::vector<mc_bfs_result> res(jobs.size());
        struct ResGuard {  // (an exception below must not leak the library's result arrays)
            std::vector<mc_bfs_result> &r;
            ~ResGuard() { for (auto &x : r) mc_bfs_result_free(&x); }
        } guard{res};
        if (!jobs.empty()) E.bfs_batch(jobs.data(), (uint32_t)jobs.size(), o.coverage, o.maxkmers, o.maxradius, res.data());
        const auto tb1 = std::chrono::steady_clock::now();
        bfs_ms += ms_between(tb0, tb1);
        for (const mc_bfs_result &r : res) { bfs_rounds += r.rounds; bfs_levels += r.levels; }

        size_t j = 0;
        for (size_t c = c0; c < c1; c++) {
            Environment env(o.k, calcs[c].genes);
            bool fail = false;
            for (size_t d = 0; d < dirs.size(); d++, j++) {
                mc_bfs_result &r = res[j];
                if (r.n == 0) { fail = true; continue; }  // runBfs: queue.size() == 0 -> fail (:193-196)
                if (fail) continue;
                BfsPass p;
                p.dir = dirs[d];
                p.kmers.reserve(r.n);
                for (uint64_t i = 0; i < r.n; i++) p.kmers.push_back(((kmer_t)r.hi[i] << 64) | r.lo[i]);
                p.dist.assign(r.dist, r.dist + r.n);
                p.cov.assign(r.cov, r.cov + r.n);
                p.last.assign(r.last, r.last + r.n);
                trimmer.add_pass(env, p, r);
            }
            if (fail) {
                info("Could not find any k-mers of the target gene in the input, halting.");
                continue;
            }
            info("Extending endings by 0 kmers");  // extendEnvironment never adds anything
            if (!env.order_guaranteed())
                logline("WARN", "--trim removed k-mers from a treeified java.util.HashMap bin: line order of " + calcs[c].out_prefix +
                                " may differ from the JVM's inside that bin");
            env.write_all(calcs[c].out_prefix, o.chunklength, compaction.pick(env.size(), calcs[c].out_prefix));
        }
        out_ms += ms_between(tb1, std::chrono::steady_clock::now());
    }
    info("Finished processing all sequences!");

    mc_stats stt{};
    if (E.c) mc_get_stats(E.c, &stt);
    else if (E.g) mc_group_get_stats(E.g, &stt);  // (summed over the devices; times: the slowest device's)
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    char buf[512];
    snprintf(buf, sizeof buf,
             "{\"windows\": %llu, \"distinct_kmers\": %llu, \"load_and_count_ms\": %.3f, \"count_kernel_ms\": %.3f, "
             "\"bfs_ms\": %.3f, \"output_ms\": %.3f, \"table_bytes\": %llu, \"binned_runs\": %llu, \"bfs_levels\": %llu, \"bfs_rounds\": %llu}\n",
             (unsigned long long)stt.windows, (unsigned long long)n_distinct, ms(t0, t1), stt.count_total_ms, bfs_ms,
             out_ms, (unsigned long long)stt.table_bytes, (unsigned long long)stt.binned_runs, bfs_levels, bfs_rounds);  // (binned_runs: --devices, counting runs fed by the binned exchange)
    write_file(wd + "/metrics.json", buf);
    write_file(wd + "/SUCCESS", "");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    try {
        if (argc <= 1) { usage(); return 0; }
        const Options o = parse_args(argc, argv);
        if (o.help) { usage(); return 0; }
        return run(o);
    } catch (const std::exception &e) {
        logline("ERROR", e.what());
        return 1;  // System.exit(1) on ExecutionFailedException, itmo!/utils/tool/Tool.java:450-462
    }
}
