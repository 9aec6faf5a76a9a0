// --tool kmer-counter (src/tools/KmersCounter.java:56-121): count, then <name>.kmers.bin + <name>.stat.txt
#include <cstring>

#include "cli.h"

namespace mch {

int run_kmer_counter(const Options &o)
{
    if (o.k < 0) throw Error("Parameter 'k' is mandatory");
    if (o.reads.empty()) throw Error("Parameter 'reads' is mandatory");
    if (!open_work_dir(o, "k=" + std::to_string(o.k) + "\n")) return 0;
    const std::string out_dir = o.output_dir.empty() ? o.work_dir + "/kmers" : o.output_dir;
    if (o.k > 31) info("Reading hashes of k-mers instead");  // (no --forcehash here: KmersCounter.java:59-69)
    const int mode = key_mode_for(o, o.k > 31);
    if (!o.devices.empty()) throw Error("--devices is for --tool environment-finder: kmer-counter writes one device's table (--device)");
    Engine E;
    E.open(table_config(o, o.k, mode), {});
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
    make_dirs(out_dir);
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

}  // namespace mch
