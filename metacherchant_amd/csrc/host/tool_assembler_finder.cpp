// --tool environment-assembler-finder (src/tools/EnvironmentAssemblerFinder.java:175-240): the environment of one sequence, then every
// read of every --reads file tested against it (src/algo/ReadsFilter.java: mc_reads_in_set_dev, whole reads in batches, the set of
// the environment's k-mers on the device once a phase) and the reads that belong to it written to <output>/cutReads<i>.fasta; with
// --assembler, their assembly (src/algo/AssemblerCalculator.java) and all of it again at k = 55 with the contigs as the reads.
#include <spawn.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <cerrno>
#include <cstring>

#include "device.h"

namespace mch {
namespace {

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
    std::vector<uint64_t> words;
    pack_whole_reads(b, 0, n, words, nullptr);
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
    if (hashed) info("Reading hashes of k-mers instead");
    Engine E;
    E.open(table_config(o, k, key_mode_for(o, hashed)), {});
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

}  // namespace

int run_assembler_finder(const Options &o)
{
    if (o.k < 0) throw Error("Parameter 'k' is mandatory");
    if (o.seq.empty()) throw Error("Parameter 'seq' is mandatory");
    if (o.output.empty()) throw Error("Parameter 'output' is mandatory");
    if (!o.devices.empty()) throw Error("--devices is for --tool environment-finder: environment-assembler-finder filters the reads on one device (--device)");
    require_supported_k(o.k);
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

}  // namespace mch
