// --tool reads-classifier (src/tools/ReadsClassifier.java:154-200, src/algo/PairFinder.java:32-57): the reads of -r split by how
// well their k-mers are covered in the graph of -i (mc_classify_reads), written to six FASTQ files.  The reference fills its four
// lists from a thread pool, so their order is only defined at -p 1; here it is that order: input order within every list.

// WritersUtils.writeDnaQsToFastqFile (itmo!/io/writers/FastqDedicatedWriter.java:39-60): "@<n>" counting from 1 (DataCounter), the
// bases with N printed as A (the DnaQ holds base 0 there), "+", the qualities as Illumina (phred + 64, Illumina.getPhredChar)
// (FastqOut and SideList: fastq_out.h; which read goes to which of them: classifier_streams.h)
#include <chrono>

#include "classifier_streams.h"
#include "device.h"
#include "fastq_out.h"

namespace mch {
namespace {

// The output streams of a tool: stream t is a file (out[t]: its records are numbered from the file's count on) or a list kept aside
// (tail[t]: under --render gpu unnumbered bodies, numbered when the list is appended).  st[s][i] is the stream of read i of side s.
// --render gpu: a batch is rendered from its device view (render_segments) or, for reads the host parsed, from the batch itself
// (render_batch); --render host: every read goes through its stream's put (put_batch).
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
    // --render host: the first n reads of a batch in item order, each through the put of its stream's file or list (which refuses
    // an empty read: "Empty DnaQ!")
    void put_batch(int n_sides, const DnaQBatch *const *b, uint64_t n)
    {
        for (uint64_t i = 0; i < n; i++)
            for (int s = 0; s < n_sides; s++) {
                const uint8_t t = st[s][i];
                if (t == MC_RENDER_SKIP) continue;
                const uint64_t o0 = b[s]->offsets[i], len = b[s]->offsets[i + 1] - o0;
                const uint8_t *codes = b[s]->codes.data() + o0, *phred = b[s]->phred.data() + o0;
                if (out[t]) out[t]->put(codes, phred, len);
                else tail[t]->put(codes, phred, len);
            }
    }
    // the debug line's numbers: `written` the records of all files when they are complete
    void report(unsigned long long written) const
    {
        fprintf(stderr, "[ingest] render: %llu records in %llu call(s) on the device, %llu through the host\n", records, calls,
                written - (records - tail_records));
        if (calls) fprintf(stderr, "[ingest] render stage: %.3f s in the calls (%.3f ms on the device), %.3f s in the copies down\n", call_s, device_ms, copy_s);
    }
};

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

// ... and the first n reads of a batch WholeReadsSource delivered, from its device view
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

std::vector<mc_read_cov> classify_side(mc_ctx *ctx, const ReadsIn &in, const DnaQBatch &b, size_t n, const Options &o)
{
    return in.gpu ? classify_segments(ctx, in.gpu->segments(), n, o) : classify_batch(ctx, b, n, o);
}

}  // namespace

int run_reads_classifier(const Options &o)
{
    // (every parameter is checked before a device is opened)
    if (o.k < 0) throw Error("Parameter 'k' is mandatory");
    if (o.input_files.empty()) throw Error("Parameter 'input-files' is mandatory");
    if (o.read_files.empty()) throw Error("Parameter 'read-files' is mandatory");
    require_supported_k(o.k);
    if (o.found_threshold < 0 || o.found_threshold > 100) throw Error("--found-threshold must be within 0 .. 100 (a percentage of the read)");
    if (!open_work_dir(o, "k=" + std::to_string(o.k) + "\n")) return 0;
    const std::string out_dir = o.output_dir.empty() ? o.work_dir + "/reads_classifier" : o.output_dir;
    make_dirs(out_dir);  // outputDir.mkdirs()

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
    Renderer R;
    R.ctx = ctx;
    R.n_streams = CLASSIFIER_STREAMS;
    FastqOut *files[6] = {&found1, &found2, &nf1, &nf2, &found_s, &nf_s};  // FOUND_1 .. NF_S
    for (int t = 0; t < 6; t++) R.out[t] = files[t];
    R.tail[FOUND_S_TAIL] = &found_s_tail;
    R.tail[NF_S_TAIL] = &nf_s_tail;
    const bool render_gpu = render_on_gpu(o, on_device, RENDER_AUTO_MIN);
    if (render_gpu) hip_check(hipSetDevice(o.device), "hipSetDevice");
    long long pairs_of[4] = {0, 0, 0, 0};  // by PAIR_*
    const int n_sides = paired ? 2 : 1;
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
        // the host decides every read's stream (and counts), whoever renders the records
        for (int s = 0; s < n_sides; s++) R.st[s].resize(n);
        for (size_t i = 0; i < n; i++) {
            const size_t l1 = b1.offsets[i + 1] - b1.offsets[i], l2 = paired ? b2.offsets[i + 1] - b2.offsets[i] : 0;
            const ClassifiedPair p = classifier_streams(c1[i].found != 0, c2[i].found != 0, l1, l2, paired);
            pairs_of[p.counter]++;
            for (int s = 0; s < n_sides; s++) R.st[s][i] = p.st[s];
        }
        const DnaQBatch *bs[2] = {&b1, &b2};
        const std::vector<WholeSegment> *segs[2] = {r1.gpu ? &r1.gpu->segments() : nullptr, paired && r2->gpu ? &r2->gpu->segments() : nullptr};
        if (!render_gpu) R.put_batch(n_sides, bs, n);
        else if (on_device) R.render_segments(n_sides, segs, bs, n);
        else R.render_batch(n_sides, bs, n);
        if (paired && n < BATCH) break;  // (one of the files is done)
    }
    const long long both = pairs_of[PAIR_BOTH], first_only = pairs_of[PAIR_FIRST_ONLY], second_only = pairs_of[PAIR_SECOND_ONLY],
                    neither = pairs_of[PAIR_NEITHER];

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
        R.report(found1.n + found2.n + nf1.n + nf2.n + found_s.n + nf_s.n);
    }
    write_file(o.work_dir + "/SUCCESS", "");
    return 0;
}

// --tool triple-reads-classifier (src/tools/TripleReadsClassifier.java:164-270, src/algo/TripleFinder.java, src/algo/TripleFinder2.java):
// the pairs of -r classed found / half found / not found by their k-mers in the graph at k, then at k2, written to nine FASTQ files.
// Both sides' reads stay on the device for both passes.  A read's pass-1 class is that of the last read of its side with the same bases
// (the reference's maps keyed by bases: mc_reads_last_copy).  The reference runs pairs on a thread pool, so its lists' order and its
// maps' last writer are only defined at -p 1; here they are that: input order in every file, "last" = the greatest input index.

// the pairs of two DnaQ readers, batch by batch: PairSource (itmo!/io/sources/PairSource.java:35-45) ends them with the shorter file
template <typename F>
static void for_each_pair_batch(const Options &o, F &&f, bool need_ctx = false)
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
    for (int kk : {o.k, o.k2}) require_supported_k(kk);
    if (o.found_threshold < 0 || o.found_threshold > 100) throw Error("--found-threshold must be within 0 .. 100 (a percentage of the read)");
    if (o.half_threshold < 0 || o.half_threshold > 100) throw Error("--half-threshold must be within 0 .. 100 (a percentage of the read)");
    if (!open_work_dir(o, "k=" + std::to_string(o.k) + "\nk2=" + std::to_string(o.k2) + "\n")) return 0;
    const std::string out_dir = o.output_dir.empty() ? o.work_dir + "/reads_classifier" : o.output_dir;
    make_dirs(out_dir);  // outputDir.mkdirs()

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
        for (int s = 0; s < 2; s++) R.st[s].resize(m);
        for (size_t i = 0; i < m; i++, at++) {
            const TripleStreams t = triple_streams(c1[at], c2[at], b1.offsets[i + 1] - b1.offsets[i], b2.offsets[i + 1] - b2.offsets[i]);
            for (int s = 0; s < 2; s++) R.st[s][i] = t.st[s];
        }
        if (!render_gpu) {
            R.put_batch(2, b, m);
            return;
        }
        R.ctx = r1.ctx;
        const std::vector<WholeSegment> *segs[2] = {r1.gpu ? &r1.gpu->segments() : nullptr, r2.gpu ? &r2.gpu->segments() : nullptr};
        if (r1.gpu && r2.gpu) R.render_segments(2, segs, b, m);
        else R.render_batch(2, b, m);
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

}  // namespace mch
