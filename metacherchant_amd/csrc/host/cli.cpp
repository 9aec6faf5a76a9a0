// What the tools of the `metacherchant` CLI share (cli.h says what): the file-scope state of the log lives here.
#include <sys/stat.h>

#include <cstring>
#include <ctime>

#include "cli.h"

namespace mch {

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

std::vector<int> pass_dirs(bool bothdirs) { return bothdirs ? std::vector<int>{0} : std::vector<int>{-1, 1}; }

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

void make_dirs(const std::string &path)
{
    write_file(path + "/.keep", "");
    remove((path + "/.keep").c_str());
}

void require_supported_k(int k)
{
    if (k < 1 || k > 63)
        throw Error("k = " + std::to_string(k) + " is not supported: this build handles k <= 31 (packed keys) and 32 <= k <= 63 (hash keys)");
}

bool kmers_on_gpu(const Options &o, uint64_t records, uint64_t auto_min)
{
    return o.kmers_io == "gpu" || (o.kmers_io == "auto" && records >= auto_min);
}

void load_kmers_file(const Options &o, mc_ctx *ctx, const std::string &path)
{
    struct stat st;
    const uint64_t records = stat(path.c_str(), &st) == 0 ? (uint64_t)st.st_size / 10 : 0;
    const bool on_gpu = kmers_on_gpu(o, records, KMERS_LOAD_AUTO_MIN);
    info("Loading " + std::to_string(records) + " k-mer records on the " + (on_gpu ? "GPU (mc_load_kmers_gpu)" : "host (mc_load_kmers)"));
    MC_CHECK(ctx, on_gpu ? mc_load_kmers_gpu(ctx, path.c_str(), 0, nullptr, nullptr) : mc_load_kmers(ctx, path.c_str(), 0, nullptr, nullptr));
}

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

bool render_on_gpu(const Options &o, bool reads_on_device, uint64_t auto_min)
{
    if (o.render == "gpu") return true;
    if (o.render == "host" || !reads_on_device) return false;
    struct stat st;
    return stat(o.read_files[0].c_str(), &st) == 0 && (uint64_t)st.st_size >= auto_min;
}

int key_mode_for(const Options &o, bool hashed)
{
    if (!hashed) return MC_KEY_PACKED;
    std::string h = o.hash;
    for (char &c : h) c = (char)tolower((unsigned char)c);
    if (h == "fnv1a") { info("Using FNV1a hash function"); return MC_KEY_FNV1A; }
    info("Using default polynomial hash function");
    return MC_KEY_POLY;
}

mc_config table_config(const Options &o, int k, int mode)
{
    mc_config cfg{};
    cfg.k = k;
    cfg.key_mode = mode;
    cfg.device = o.device;
    cfg.capacity_hint = o.capacity_hint;
    return cfg;
}

bool names_kmers_bin(const std::string &path)
{
    std::string first = path;
    const size_t slash = first.find_last_of('/');
    if (slash != std::string::npos) first = first.substr(slash + 1);
    for (char &c : first) c = (char)tolower((unsigned char)c);
    return first.size() >= 9 && first.compare(first.size() - 9, 9, "kmers.bin") == 0;
}

void load_graph(const Options &o, int k, const std::vector<std::string> &kmer_files, Engine &E)
{
    const int mode = key_mode_for(o, k > 31);  // determineHashFunction
    const bool kmers_bin = !kmer_files.empty() && names_kmers_bin(kmer_files[0]);
    E.open(table_config(o, k, mode), {});
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

}  // namespace mch
