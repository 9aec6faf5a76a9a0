// metacherchant's command line: the parameter table of every tool, the parser and the usage text.  Mirrors the launch options of
// itmo!/utils/tool/Tool.java:59-143 and each tool's own addParameter calls.
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <map>

#include "cli.h"

namespace mch {

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
    {"replay", nullptr, 0},
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

static const OptSpec *find_spec(SpecTable t, const std::string &tok)
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

static long long parse_int(const std::string &name, const std::string &v)
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
    if (auto v = val("replay")) {
        if (*v != "host" && *v != "gpu" && *v != "auto") throw Error("--replay takes host, gpu or auto, not '" + *v + "'");
        o.replay = *v;
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
    puts("                --replay host|gpu|auto (fmt-visualizer: who replays the walk's order over every component.  host: the reference's");
    puts("                queue, a component a thread -- it has no visited set and does not end on components with many bubbles in a row;");
    puts("                gpu: mc_walk_order over all components of a phase at once, at most two queue entries a k-mer; the files are the");
    puts("                same; default auto: the host, and the GPU for the components whose host queue passes 64 entries a k-mer + 4096)");
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

}  // namespace mch
