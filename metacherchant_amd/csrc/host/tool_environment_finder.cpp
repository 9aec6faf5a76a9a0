// --tool environment-finder (src/tools/EnvironmentFinderMain.java:32-243): the reads counted into the table exactly where the Java tool
// calls IOUtils.loadReads / LargeKIOUtils.loadReads, one OneSequenceCalculator.runBfs a sequence as a job of mc_bfs_batch, and the
// reference's output surface from Environment.
#include <algorithm>
#include <chrono>

#include "cli.h"

namespace mch {

int run_environment_finder(const Options &o)
{
    if (o.k < 0) throw Error("Parameter 'k' is mandatory");
    if (o.seq.empty()) throw Error("Parameter 'seq' is mandatory");
    if (o.output.empty()) throw Error("Parameter 'output' is mandatory");
    if (o.maxkmers < 0 && o.maxradius < 0)  // EnvironmentFinderMain.java:171-175
        throw Error("At least one of --maxkmers and --maxradius parameters should be set");
    if (o.coverage < 0) throw Error("--coverage must not be negative (absent k-mers read as -1 and would pass)");
    if (o.k > 63) require_supported_k(o.k);  // (the reference hashes k-mer STRINGS of any length for k > 31; the walk here keeps oriented k-mers in 128 bits)

    const std::string wd = o.work_dir;
    if (!open_work_dir(o, "k=" + std::to_string(o.k) + "\nseq=" + o.seq + "\noutput=" + o.output + "\ncoverage=" +
                              std::to_string(o.coverage) + "\nbothdirs=" + (o.bothdirs ? "true" : "false") + "\n"))
        return 0;

    // loadInput (EnvironmentFinderMain.java:127-154)
    const bool hashed = o.k > 31 || o.forcehash;
    if (hashed) info("Reading hashes of k-mers instead");
    Engine E;
    E.open(table_config(o, o.k, key_mode_for(o, hashed)), o.devices);
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

}  // namespace mch
