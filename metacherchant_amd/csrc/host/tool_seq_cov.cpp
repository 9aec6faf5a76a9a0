// --tool seq-cov (src/tools/SequenceCoverage.java:127-185): four bins of reads counted into four tables (every k-mer), then for
// every sequence of --read-file the mean depth and the breadth of its k-mers in each (mc_seq_coverage: one key, four probes a
// window).  Nothing walks these tables: no read store is kept, and a table's counting scratch goes back before the next is counted.
#include "device.h"

namespace mch {

struct SeqCovBin { const char *param; const std::vector<std::string> *files; };

// one batch of whole sequences through mc_seq_coverage, and its rows.  segs: the batch's device view (--parse gpu), else NULL
static void seq_cov_batch(mc_ctx *const *tables, const DnaQBatch &b, int k, FILE *out, const std::vector<WholeSegment> *segs = nullptr)
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
        std::vector<uint64_t> words;
        pack_whole_reads(b, 0, n, words, nullptr);
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
    require_supported_k(o.k);
    if (!open_work_dir(o, "k=" + std::to_string(o.k) + "\n")) return 0;
    const std::string out_dir = o.output_dir.empty() ? o.work_dir + "/sequence_coverage" : o.output_dir;
    make_dirs(out_dir);  // outputDir.mkdirs()

    info("Loading bins ...");
    Engine E[4];
    mc_ctx *tables[4];
    for (int t = 0; t < 4; t++) {  // loadGraph (SequenceCoverage.java:87-101)
        if (o.k > 31) info("Reading hashes of k-mers instead");
        E[t].open(table_config(o, o.k, key_mode_for(o, o.k > 31)), {});
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

}  // namespace mch
