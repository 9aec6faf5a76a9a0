// mc_walk_order_bench: times the walk order of one synthetic component both ways, as the fmt-visualizer takes it (tool_visualisers.cpp):
//   host  replay_component_walk over the component's sorted k-mers (`--replay host`, the parent's code), with `--replay auto`'s cap
//         of 64 entries a member + 4096 when asked: a run that passes it is reported as abandoned, not timed;
//   gpu   mc_walk_order from host arrays, copies included, and the puts made from its order (`--replay gpu`).
// The sorted list is made before either and is not timed: the tool sorts it anyway, for the colours.  scripts/walk_order_bench.py
// runs this and takes the medians; DESIGN.md 3.18 has the figures.
//
//   mc_walk_order_bench <k> <kmers> <error_every> <reps> <device> <host|gpu|both>
//
// The component: the k-windows of a stretch of the synthetic genome (mc_synth_genome, seed below) in genome order, the first one
// the seed -- what error-free reads give: a thin chain.  error_every > 0 adds the windows of a copy with a substitution at every
// error_every-th base, what reads with errors give: equal-arm bubbles in a row.  A k-mer met again (itself or its reverse
// complement) is left out.  Every run is a wall-clock time around work that ends on the host; the GPU runs come after one untimed
// run of the same size, the two ways in turn.  The two ways' puts are compared once.  Prints one JSON line.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "envfinder.h"
#include "mcgpu.h"

using namespace mch;

namespace {

constexpr uint64_t GENOME_SEED = 20240531;

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

std::vector<kmer_t> make_component(int k, size_t kmers, size_t error_every)
{
    const size_t len = (error_every ? kmers * error_every / (error_every + (size_t)k) : kmers) + (size_t)k - 1;
    std::vector<uint8_t> g(len);
    if (mc_synth_genome(GENOME_SEED, 0, g.size(), g.data()) != MC_OK) throw Error("mc_synth_genome failed");
    const kmer_t mask = ((kmer_t)1 << (2 * k)) - 1;
    std::vector<kmer_t> all;
    for (int copy = 0; copy < (error_every ? 2 : 1); copy++) {
        kmer_t v = 0;
        for (size_t i = 0; i < g.size(); i++) {
            const unsigned base = copy && i % error_every == error_every / 2 && i >= (size_t)k && i + k < g.size() ? (g[i] + 1u) & 3 : g[i];
            v = ((v << 2) | base) & mask;
            if (i + 1 >= (size_t)k) all.push_back(v);
        }
    }
    std::vector<std::pair<kmer_t, uint32_t>> order(all.size());
    for (size_t i = 0; i < all.size(); i++) order[i] = {normalize128(all[i], k), (uint32_t)i};
    std::sort(order.begin(), order.end());
    std::vector<char> again(all.size(), 0);
    for (size_t i = 1; i < order.size(); i++)
        if (order[i].first == order[i - 1].first) again[order[i].second] = 1;
    std::vector<kmer_t> out;
    for (size_t i = 0; i < all.size(); i++)
        if (!again[i]) out.push_back(all[i]);
    return out;
}

std::string list(const std::vector<double> &v)
{
    std::string s = "[";
    for (size_t i = 0; i < v.size(); i++) s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "]";
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 7) {
        fprintf(stderr, "usage: mc_walk_order_bench <k> <kmers> <error_every> <reps> <device> <host|gpu|both>\n");
        return 2;
    }
    mc_ctx *ctx = nullptr;
    try {
        const int k = atoi(argv[1]), reps = atoi(argv[4]), device = atoi(argv[5]);
        const size_t kmers = strtoull(argv[2], nullptr, 10), error_every = strtoull(argv[3], nullptr, 10);
        const std::string what = argv[6];
        const bool host = what != "gpu", gpu = what != "host";
        if (k < 2 || k > 63 || kmers < 16 || reps < 1 || (error_every && error_every < 2 * (size_t)k)) throw Error("k = 2 .. 63, kmers >= 16, reps >= 1, error_every 0 or >= 2k");
        const std::vector<kmer_t> members = make_component(k, kmers, error_every);
        const size_t n = members.size();
        std::vector<uint64_t> hi(n), lo(n), off{0, n};
        for (size_t i = 0; i < n; i++) { hi[i] = (uint64_t)(members[i] >> 64); lo[i] = (uint64_t)members[i]; }
        std::vector<std::pair<kmer_t, uint32_t>> order(n);
        for (size_t i = 0; i < n; i++) order[i] = {normalize128(members[i], k), (uint32_t)i};
        std::sort(order.begin(), order.end());
        std::vector<kmer_t> canon(n);
        for (size_t i = 0; i < n; i++) canon[i] = order[i].first;
        const size_t cap = error_every ? 64 * n + 4096 : 0;
        fprintf(stderr, "mc_walk_order_bench: k=%d, %zu members, error_every=%zu\n", k, n, error_every);

        mc_walk_order_result wo{};
        const auto gpu_puts = [&] {
            mc_walk_order_free(&wo);
            if (mc_walk_order(ctx, k > 32 ? hi.data() : nullptr, lo.data(), off.data(), 1, 0, &wo) != MC_OK) throw Error(std::string(mc_last_error(ctx)));
            std::vector<std::pair<kmer_t, int>> puts;
            puts.reserve(wo.reached[0]);
            for (uint64_t i = 0; i < wo.reached[0]; i++) puts.emplace_back(members[wo.order[i]], wo.twice[wo.order[i]] ? 0 : 1);
            return puts;
        };
        if (gpu) {
            mc_config cfg{};
            cfg.k = k;
            cfg.key_mode = MC_KEY_POLY;
            cfg.device = device;
            if (mc_create(&cfg, &ctx) != MC_OK) throw Error(std::string(mc_last_error(nullptr)));
            gpu_puts();  // (untimed: the code objects load)
            fprintf(stderr, "mc_walk_order_bench: warm\n");
        }
        std::vector<double> host_s, gpu_s, dev_ms;
        int same = -1, abandoned = 0;
        for (int r = 0; r < reps; r++) {  // (the two ways in turn: what else the machine does meets both)
            std::vector<std::pair<kmer_t, int>> hp, gp;
            if (host && !abandoned) {
                std::vector<int> count(n, 1);
                bool gave_up = false;
                const double t0 = now_s();
                hp = replay_component_walk(k, members[0], canon, count, cap, &gave_up);
                const double t = now_s() - t0;
                if (gave_up) abandoned = 1;
                else host_s.push_back(t);
                fprintf(stderr, "mc_walk_order_bench: host %.4f s%s\n", t, gave_up ? " (abandoned at the cap)" : "");
            }
            if (gpu) {
                const double t0 = now_s();
                gp = gpu_puts();
                gpu_s.push_back(now_s() - t0);
                dev_ms.push_back(wo.device_ms);
                fprintf(stderr, "mc_walk_order_bench: gpu %.4f s\n", gpu_s.back());
            }
            if (r == 0 && host && gpu && !abandoned) {
                // the map that the host's puts leave: the keys in the order of their first puts, each with its last value
                const auto entry = [&](kmer_t v) { return (size_t)(std::lower_bound(canon.begin(), canon.end(), normalize128(v, k)) - canon.begin()); };
                std::vector<int> value(n, -1);
                std::vector<size_t> firsts;
                for (const auto &p : hp) {
                    const size_t e = entry(p.first);
                    if (value[e] < 0) firsts.push_back(e);
                    value[e] = p.second;
                }
                same = firsts.size() == gp.size();
                for (size_t i = 0; same && i < gp.size(); i++) same = entry(gp[i].first) == firsts[i] && gp[i].second == value[firsts[i]];
            }
        }
        printf("{\"k\": %d, \"members\": %zu, \"error_every\": %zu, \"same_puts\": %s, \"host_abandoned\": %s, \"host_s\": %s, \"gpu_s\": %s, "
               "\"device_ms\": %s, \"levels\": %llu, \"wide_levels\": %llu, \"queue_entries\": %llu, \"reached\": %llu}\n",
               k, n, error_every, same < 0 ? "null" : same ? "true" : "false", abandoned ? "true" : "false", list(host_s).c_str(), list(gpu_s).c_str(),
               list(dev_ms).c_str(), (unsigned long long)wo.levels, (unsigned long long)wo.wide_levels, (unsigned long long)wo.queue_entries,
               (unsigned long long)(wo.reached ? wo.reached[0] : 0));
        mc_walk_order_free(&wo);
        mc_destroy(ctx);
        return same == 0 ? 1 : 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "mc_walk_order_bench: %s\n", e.what());
        mc_destroy(ctx);
        return 1;
    }
}
