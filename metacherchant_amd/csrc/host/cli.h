// What the tools of the `metacherchant` CLI share (cli.cpp): the log, the work directory, the table behind Engine and how it is
// configured and filled, and the host|gpu|auto choices with the measured sizes they go by.  main.cpp dispatches to the run_* functions
// below, one unit a tool or pair of tools (tool_*.cpp); device.h adds what needs HIP's host API.
#pragma once
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <vector>

#include "envfinder.h"
#include "gpu_compactor.h"
#include "mcgpu.h"
#include "options.h"

namespace mch {

// the log: stderr (DEBUG only with --verbose), <work-dir>/log and <work-dir>/logs/log_<stamp> once open_work_dir has opened them
extern FILE *g_log, *g_log2;
extern bool g_verbose;
void logline(const char *level, const std::string &msg);
void info(const std::string &m);
std::string group_digits(unsigned long long v);               // itmo!/utils/NumUtils.java:163-174
std::string shorten_label(const std::string &label, int k);  // src/utils/StringUtils.java:43-49

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
std::vector<int> pass_dirs(bool bothdirs);
// work dir: log files, in.properties / SUCCESS (itmo!/utils/tool/Tool.java:31-33,318-392,666-689).
// Returns false when --continue finds the tool finished already.
bool open_work_dir(const Options &o, const std::string &props);
void make_dirs(const std::string &path);  // File.mkdirs()
void require_supported_k(int k);          // throws for a k outside 1 .. 63

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

// --replay: the order of the fmt-visualizer's walks over a phase's components, by the host's replay of the reference's queue (a
// component a thread) or by one mc_walk_order call over all of them; `auto`, the default, takes the GPU for a phase of REPLAY_AUTO_MIN
// k-mers or more, and below that the host with a cap: a component whose queue passes 64 entries a member + 4096 (the exact queue of
// 780 random small components never passed 13.4 a member; a few bubbles in a row double it each) is abandoned and goes to the GPU.
// REPLAY_AUTO_MIN is "never": on thin chains (one component of 10^4 to 10^6 k-mers of error-free reads, k = 31 and 63, medians of 5,
// scripts/walk_order_bench.py, profiles/walk_order_bench.txt) the host's replay takes 5.6 ms / 74 .. 83 ms / 0.96 s
// against the GPU way's 23 ms / 0.23 s / 2.3 s, call and copies included -- 2.3 us a level on the device, 0.6 .. 1 us a k-mer on the
// host -- each time by far more than either spread: no measured size from which the whole phase is faster the device's way.  So `auto`
// uses the device only behind the cap, for components that the host's queue cannot finish.
constexpr uint64_t REPLAY_AUTO_MIN = ~0ull;

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
bool kmers_on_gpu(const Options &o, uint64_t records, uint64_t auto_min);

// --parse: who reads the whole reads of a -r file.  host: DnaQReader on one thread, then the tool packs the bases and looks for the
// low-quality positions itself; gpu: WholeReadsSource -- the text is tokenised on the device (mc_tokenize_whole_dev) and its words,
// offsets and positions go into the _dev entry points where they are; auto: gpu for an uncompressed file of PARSE_AUTO_MIN bytes or
// more.  That is the smallest file scripts/whole_reads_bench.py has timed (10^5 FASTQ records of 150 bases), and there the whole
// reads-classifier is already faster the GPU's way; below it nothing is measured, and auto is host.
constexpr uint64_t PARSE_AUTO_MIN = 31600000;
bool parse_on_gpu(const Options &o, const std::string &path);

// --render: who turns the reads that go to the classifiers' FASTQ files into text.  host: FastqOut::put, a record and a base at a
// time; gpu: mc_render_fastq* renders every output stream of a batch in one call, the text comes down into one staging buffer and
// each file takes its stream with one fwrite; auto: gpu only for reads that are on the device already (--parse gpu took every -r file
// there) and a first -r file of at least the size from which the whole tool was measured to be faster that way
// (scripts/render_bench.py): the triple classifier at 10^5 records of 150 bases, the smallest size measured;
// reads-classifier at 10^7 -- at 10^5 and 10^6 its two ways lie within each other's spread, and auto stays host.
constexpr uint64_t RENDER_AUTO_MIN = 3160000000, RENDER_AUTO_MIN_TRIPLE = 31600000;
bool render_on_gpu(const Options &o, bool reads_on_device, uint64_t auto_min);

// the key mode of a table: packed, or for hashed keys what --hash names, with the reference's "Using ... hash function" line
int key_mode_for(const Options &o, bool hashed);
// a table of k-mers of length k in that mode on --device, sized by --capacity-hint
mc_config table_config(const Options &o, int k, int mode);

// the reads of all --reads files into the table; returns hm.size()
uint64_t load_reads(const std::vector<std::string> &files, Engine &e);
// IOUtils.loadKmers of one file (threshold 0) into the table
void load_kmers_file(const Options &o, mc_ctx *ctx, const std::string &path);
// file.getName().toLowerCase().endsWith("kmers.bin"): loadGraph reads such a file as kmer-counter's output
bool names_kmers_bin(const std::string &path);
// loadGraph (ReadsClassifier.java:98-132, TripleReadsClassifier.java:127-160): the hash-function line for k > 31, then the table at k
// from kmer_files when the first one's name ends in kmers.bin (IOUtils.loadKmers), else counted from the reads of --input-files
void load_graph(const Options &o, int k, const std::vector<std::string> &kmer_files, Engine &E);

// the tools
int run_kmer_counter(const Options &o);
int run_multi(const Options &o);
int run_reads_classifier(const Options &o);
int run_triple_reads_classifier(const Options &o);
int run_seq_cov(const Options &o);
int run_recipient_visualiser(const Options &o);
int run_fmt_visualizer(const Options &o);
int run_assembler_finder(const Options &o);
int run_environment_finder(const Options &o);

}  // namespace mch
