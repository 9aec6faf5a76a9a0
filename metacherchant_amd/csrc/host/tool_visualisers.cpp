// --tool recipient-visualiser (src/tools/RecipientVisualiser.java:185-223, src/algo/SeqEnvCalculator.java): the environment of every
// sequence of --seq in the graph of the post-FMT reads (mc_bfs_batch: all eight neighbours, count > 0), every k-mer coloured by which
// of the four class tables hold it (mc_kmer_presence: one call a batch of sequences), one coloured GFA and one FASTA a sequence.
// The reference runs the sequences on a thread pool; each writes its own files, and the log lines here come in sequence order.
#include <atomic>
#include <map>
#include <thread>

#include "device.h"

namespace mch {

int run_recipient_visualiser(const Options &o)
{
    if (o.k < 0) throw Error("Parameter 'k' is mandatory");
    if (o.after_files.empty()) throw Error("Parameter 'after-files' is mandatory");
    if (o.seq.empty()) throw Error("Parameter 'seq' is mandatory");
    if (o.input_dir.empty()) throw Error("Parameter 'input-dir' is mandatory");
    if (o.ext.empty()) throw Error("Parameter 'ext' is mandatory");
    require_supported_k(o.k);
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
    if (o.k > 31) info("Reading hashes of k-mers instead");  // loadAfterGraphs :108-123
    mc_config cfg = table_config(o, o.k, key_mode_for(o, o.k > 31));
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
// mc_kmer_presence the class tables of every member, and only what the walk's ORDER decides is replayed, a component
// at a time on -p threads (the reference cannot: every walk writes the one shared map): the FIFO without a visited set over the
// component's own k-mer -> count map, which gives the order of the subgraph's puts and the coverage 0 of a k-mer popped twice
// (replay_component_walk, envfinder.cpp) -- or, under --replay gpu | auto, mc_walk_order's bounded form of it for all components at once.

static void fmt_phase(const Options &o, const std::string &name, const std::vector<std::string> &files, const std::vector<std::string> &classes,
                      const std::string &out_root)
{
    info("Loading " + name + " reads ...");
    if (o.k > 31) info("Reading hashes of k-mers instead");
    mc_config cfg = table_config(o, o.k, key_mode_for(o, o.k > 31));
    const uint32_t nt = (uint32_t)classes.size();
    std::vector<std::vector<std::string>> class_files(nt);
    for (uint32_t t = 0; t < nt; t++)
        for (const char *part : {"_1.", "_2.", "_s."}) {
            class_files[t].push_back(o.input_dir + "/" + classes[t] + part + o.ext);
            FILE *f = fopen(class_files[t].back().c_str(), "rb");
            if (!f) throw Error("Could not read class file " + class_files[t].back());
            fclose(f);
        }
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
    std::vector<uint64_t> words;
    pack_whole_reads(seqs, 0, seqs.n_reads(), words, nullptr);
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
    // --replay: the walk's order by the host's queue, or by mc_walk_order (at most two queue entries a k-mer).  wo_at[c]: where
    // component c's slice starts in the device's answer, or all ones for a component the host replays.
    const bool all_gpu = o.replay == "gpu" || (o.replay == "auto" && res.n_kmers >= REPLAY_AUTO_MIN);
    const bool capped = o.replay == "auto";
    mc_walk_order_result wo{};
    struct WoGuard {
        mc_walk_order_result &r;
        ~WoGuard() { mc_walk_order_free(&r); }
    } wo_guard{wo};
    std::vector<uint64_t> wo_at(res.n_components, ~0ull), wo_comp(res.n_components, 0);  // (wo_comp[c]: its number in that call)
    if (all_gpu && res.n_components) {
        MC_CHECK(G.c, mc_walk_order(G.c, res.hi, res.lo, res.comp_offsets, res.n_components, 0, &wo));
        for (uint64_t c = 0; c < res.n_components; c++) { wo_at[c] = res.comp_offsets[c]; wo_comp[c] = c; }
    }
    std::vector<uint64_t> todo(res.n_components), abandoned;
    for (uint64_t c = 0; c < res.n_components; c++) todo[c] = c;
    std::atomic<uint64_t> next{0};
    std::mutex err_mu;
    std::string err;
    auto work = [&] {
        for (uint64_t at; (at = next.fetch_add(1)) < todo.size();) {
            const uint64_t c = todo[at];
            try {
                const uint64_t a = res.comp_offsets[c], b = res.comp_offsets[c + 1];
                std::vector<std::pair<kmer_t, uint64_t>> order;  // (canonical k-mer, member)
                order.reserve(b - a);
                for (uint64_t i = a; i < b; i++) order.emplace_back(normalize128(((kmer_t)res.hi[i] << 64) | res.lo[i], o.k), i);
                std::sort(order.begin(), order.end());
                std::vector<kmer_t> canon;
                for (const auto &e : order) canon.push_back(e.first);
                Environment env(o.k, {});
                if (wo_at[c] != ~0ull) {
                    // the first pops in order; a k-mer that is popped again ends with the 0 of its second put
                    std::vector<std::pair<kmer_t, int>> puts;
                    const uint64_t reached = wo.reached[wo_comp[c]];
                    puts.reserve(reached);
                    for (uint64_t i = 0; i < reached; i++) {
                        const uint64_t m = wo.order[wo_at[c] + i];
                        puts.emplace_back(((kmer_t)res.hi[a + m] << 64) | res.lo[a + m], wo.twice[wo_at[c] + m] ? 0 : (int)res.cov[a + m]);
                    }
                    env.add_puts(puts);
                } else {
                    std::vector<int> count;
                    for (const auto &e : order) count.push_back(res.cov[e.second]);
                    const kmer_t seed = ((kmer_t)res.hi[a] << 64) | res.lo[a];
                    bool gave_up = false;
                    const auto puts = replay_component_walk(o.k, seed, canon, count, capped ? 64 * (size_t)(b - a) + 4096 : 0, &gave_up);
                    if (gave_up) {
                        std::lock_guard<std::mutex> g(err_mu);
                        abandoned.push_back(c);
                        continue;
                    }
                    env.add_puts(puts);
                }
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
    auto run_pool = [&] {
        next = 0;
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        const uint64_t n_threads = std::max<uint64_t>(1, std::min<uint64_t>(o.processors > 0 ? (uint64_t)o.processors : std::min(hw, 16u), todo.size()));
        std::vector<std::thread> pool;
        for (uint64_t t = 1; t < n_threads; t++) pool.emplace_back(work);
        work();
        for (auto &th : pool) th.join();
        if (!err.empty()) throw Error(err);
    };
    if (res.n_components) write_file(out_dir + "/comp0.gfa", "");  // (the directory, made once before the threads write into it)
    run_pool();
    if (!abandoned.empty()) {
        // what the host gave up goes to the device in one call, and the pool runs over it again
        std::sort(abandoned.begin(), abandoned.end());
        std::vector<uint64_t> hi, lo, off{0};
        for (const uint64_t c : abandoned) {
            wo_at[c] = off.back();
            wo_comp[c] = off.size() - 1;
            hi.insert(hi.end(), res.hi + res.comp_offsets[c], res.hi + res.comp_offsets[c + 1]);
            lo.insert(lo.end(), res.lo + res.comp_offsets[c], res.lo + res.comp_offsets[c + 1]);
            off.push_back(lo.size());
        }
        MC_CHECK(G.c, mc_walk_order(G.c, hi.data(), lo.data(), off.data(), abandoned.size(), 0, &wo));
        todo = abandoned;
    }
    std::string line = "Replayed the walks of " + std::to_string(all_gpu ? 0 : res.n_components - abandoned.size()) + " components on the host, " +
                       std::to_string(all_gpu ? res.n_components : abandoned.size()) + " on the GPU (mc_walk_order)";
    if (!abandoned.empty()) {
        line += "; the host's queue passed its cap on";
        for (size_t i = 0; i < abandoned.size() && i < 8; i++) line += " comp" + std::to_string(abandoned[i]);
        if (abandoned.size() > 8) line += " ...";
    }
    info(line);
    if (!abandoned.empty()) run_pool();
}

int run_fmt_visualizer(const Options &o)
{
    if (o.k < 0) throw Error("Parameter 'k' is mandatory");
    if (o.donor_files.empty()) throw Error("Parameter 'donor-files' is mandatory");
    if (o.before_files.empty()) throw Error("Parameter 'before-files' is mandatory");
    if (o.after_files.empty()) throw Error("Parameter 'after-files' is mandatory");
    if (o.input_dir.empty()) throw Error("Parameter 'input-dir' is mandatory");
    if (o.ext.empty()) throw Error("Parameter 'ext' is mandatory");
    require_supported_k(o.k);
    if (!o.devices.empty()) throw Error("--devices is for --tool environment-finder: fmt-visualizer keeps a phase's tables on one device (--device)");
    if (!open_work_dir(o, "k=" + std::to_string(o.k) + "\ninput-dir=" + o.input_dir + "\next=" + o.ext + "\n")) return 0;
    const std::string out_root = o.output_dir.empty() ? o.work_dir + "/graph" : o.output_dir;
    fmt_phase(o, "donor", o.donor_files, {"settle", "not_settle"}, out_root);
    fmt_phase(o, "before", o.before_files, {"stay", "gone"}, out_root);
    fmt_phase(o, "after", o.after_files, {"came_from_donor", "came_from_baseline", "came_from_both", "came_itself"}, out_root);
    write_file(o.work_dir + "/SUCCESS", "");
    return 0;
}

}  // namespace mch
