// --tool environment-finder-multi (src/tools/EnvironmentFinderMultiMain.java).  --join: the join of the graph files and the compaction
// on the host on k-mer strings (environment_finder_multi, the reference's way), on the GPU on packed k-mers (mc_env_join and mc_unitigs
// on a context of its own with an empty table), or `auto`, the default: on the GPU from JOIN_AUTO_MIN entries on.  That is the smallest
// size at which scripts/multi_join_bench.py has timed the whole tool faster the GPU's way than on strings (0.34 s against 1.57 s at
// k = 31, 0.46 s against 1.77 s at k = 63, four graphs); at 10 000 entries the GPU's way took 0.27 s, as at 2 000 (a process opens the device and
// creates a context before its first kernel), three times the string path's whole run.
#include <hip/hip_runtime_api.h>

#include "cli.h"
#include "gpu_joiner.h"

namespace mch {

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

}  // namespace mch
