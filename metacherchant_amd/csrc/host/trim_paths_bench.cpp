// mc_trim_paths_bench: times the trim of one synthetic BFS pass both ways, as Environment::add_pass does it (envfinder.cpp):
//   host  trim_pass on the pass's map: runTrimPaths' reverse walk and retainAll's removals (`--trim-on host`, the parent's code);
//   gpu   mc_trim_paths from host arrays, copies included, then trim_pass with its mask: the removals alone (`--trim-on gpu`).
// The map, distanceToKmer, is built before either and is not timed: add_pass builds it anyway.  scripts/trim_paths_bench.py runs
// this and takes the medians; DESIGN.md 3.15 has the figures.
//
//   mc_trim_paths_bench <k> <entries> <fork_every> <dir> <reps> <device> <host|gpu|both>
//
// The pass: the k-windows of a stretch of the synthetic genome (mc_synth_genome, seed below) in genome order, as a walk finds
// them, and at every fork_every-th base a side arm of fork_every / 4 bases that leaves the main path by another base; every other
// arm ends in `last`, the others are dead; `last` also on the far end of the main path (dir = +1) or on both (dir = 0).  A k-mer
// met again is left out.  Every run is a wall-clock time around work that ends on the host; the GPU runs come after one untimed
// run of the same size, the two ways in turn.  The two ways' maps are compared once, key by key in iteration order.  Prints one
// JSON line.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "envfinder.h"
#include "mcgpu.h"

using namespace mch;

namespace {

constexpr uint64_t GENOME_SEED = 20240531, ARM_SEED = 42;

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

BfsPass make_pass(int k, size_t entries, size_t fork_every, int dir)
{
    const size_t arm = std::max<size_t>(fork_every / 4, 2);
    const size_t per_fork = fork_every + arm;  // entries a stretch of fork_every bases gives, about
    const size_t main_len = (entries / per_fork + 1) * fork_every + (size_t)k + fork_every;
    std::vector<uint8_t> g(main_len);
    if (mc_synth_genome(GENOME_SEED, 0, g.size(), g.data()) != MC_OK) throw Error("mc_synth_genome failed");
    const kmer_t mask = k >= 64 ? ~(kmer_t)0 : (((kmer_t)1 << (2 * k)) - 1);
    std::mt19937_64 rng(ARM_SEED);
    std::vector<kmer_t> kmers;
    std::vector<uint8_t> last;
    kmer_t v = 0;
    size_t forks = 0;
    for (size_t i = 0; i < g.size() && kmers.size() < entries; i++) {
        if (i >= (size_t)k && i % fork_every == 0 && kmers.size() + arm < entries) {  // an arm leaves here: v's last k - 1 bases, another base
            kmer_t a = ((v << 2) | (unsigned)((g[i] + 1 + forks % 3) & 3)) & mask;
            for (size_t j = 0; j < arm; j++) {
                kmers.push_back(a);
                last.push_back(j + 1 == arm && forks % 2 == 0);
                a = ((a << 2) | (unsigned)(rng() & 3)) & mask;
            }
            forks++;
        }
        v = ((v << 2) | g[i]) & mask;
        if (i + 1 >= (size_t)k) {
            kmers.push_back(v);
            last.push_back(0);
        }
    }
    // a k-mer met again is left out (its first copy stays)
    std::vector<std::pair<kmer_t, uint32_t>> order(kmers.size());
    for (size_t i = 0; i < kmers.size(); i++) order[i] = {kmers[i], (uint32_t)i};
    std::sort(order.begin(), order.end());
    std::vector<char> again(kmers.size(), 0);
    for (size_t i = 1; i < order.size(); i++)
        if (order[i].first == order[i - 1].first) again[order[i].second] = 1;
    BfsPass p;
    p.dir = dir;
    for (size_t i = 0; i < kmers.size(); i++) {
        if (again[i]) continue;
        p.kmers.push_back(kmers[i]);
        p.last.push_back(last[i]);
    }
    // the main path's ends: its first window is the pass's first entry, its last window the pass's last
    if (dir >= 0) p.last.back() = 1;
    if (dir <= 0) p.last.front() = 1;
    p.dist.assign(p.kmers.size(), 0);
    p.cov.assign(p.kmers.size(), 1);
    return p;
}

void fill(JavaKmerMap &d, const BfsPass &p)
{
    for (size_t i = 0; i < p.kmers.size(); i++) d.put(p.kmers[i], p.dist[i]);
}

std::vector<kmer_t> keys_of(const JavaKmerMap &d)
{
    std::vector<kmer_t> out;
    d.for_each([&](kmer_t key, int, int) { out.push_back(key); });
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
    if (argc != 8) {
        fprintf(stderr, "usage: mc_trim_paths_bench <k> <entries> <fork_every> <dir> <reps> <device> <host|gpu|both>\n");
        return 2;
    }
    mc_ctx *ctx = nullptr;
    try {
        const int k = atoi(argv[1]), dir = atoi(argv[4]), reps = atoi(argv[5]), device = atoi(argv[6]);
        const size_t entries = strtoull(argv[2], nullptr, 10), fork_every = strtoull(argv[3], nullptr, 10);
        const std::string what = argv[7];
        const bool host = what != "gpu", gpu = what != "host";
        if (k < 2 || k > 63 || fork_every < 8 || reps < 1 || entries < 16 || dir < -1 || dir > 1) throw Error("k = 2 .. 63, fork_every >= 8, entries >= 16, reps >= 1, dir -1 .. 1");
        const BfsPass p = make_pass(k, entries, fork_every, dir);
        const size_t n = p.kmers.size();
        std::vector<uint64_t> hi(n), lo(n);
        for (size_t i = 0; i < n; i++) { hi[i] = (uint64_t)(p.kmers[i] >> 64); lo[i] = (uint64_t)p.kmers[i]; }
        fprintf(stderr, "mc_trim_paths_bench: k=%d dir=%d, %zu entries\n", k, dir, n);

        std::vector<uint8_t> kept(n);
        double device_ms = 0;
        const auto gpu_mask = [&] {
            if (mc_trim_paths(ctx, hi.data(), lo.data(), p.last.data(), n, dir, kept.data(), &device_ms) != MC_OK) throw Error(std::string(mc_last_error(ctx)));
        };
        if (gpu) {
            mc_config cfg{};
            cfg.k = k;
            cfg.key_mode = MC_KEY_POLY;
            cfg.device = device;
            if (mc_create(&cfg, &ctx) != MC_OK) throw Error(std::string(mc_last_error(nullptr)));
            gpu_mask();  // (untimed: the code objects load)
            fprintf(stderr, "mc_trim_paths_bench: warm\n");
        }
        std::vector<double> host_s, gpu_s, call_s, dev_ms;
        size_t kept_n = 0;
        int same = -1;
        for (int r = 0; r < reps; r++) {  // (the two ways in turn: what else the machine does meets both)
            std::vector<kmer_t> hk, gk;
            if (host) {
                JavaKmerMap d(k);
                fill(d, p);
                const double t0 = now_s();
                trim_pass(d, p, k);
                host_s.push_back(now_s() - t0);
                fprintf(stderr, "mc_trim_paths_bench: host %.4f s\n", host_s.back());
                if (r == 0) hk = keys_of(d);
            }
            if (gpu) {
                JavaKmerMap d(k);
                fill(d, p);
                const double t0 = now_s();
                gpu_mask();
                const double t1 = now_s();
                trim_pass(d, p, k, &kept);
                gpu_s.push_back(now_s() - t0);
                call_s.push_back(t1 - t0);
                dev_ms.push_back(device_ms);
                fprintf(stderr, "mc_trim_paths_bench: gpu %.4f s\n", gpu_s.back());
                if (r == 0) gk = keys_of(d);
            }
            if (r == 0) {
                kept_n = host ? hk.size() : gk.size();
                if (host && gpu) same = hk == gk ? 1 : 0;
            }
        }
        printf("{\"k\": %d, \"dir\": %d, \"entries\": %zu, \"fork_every\": %zu, \"kept\": %zu, \"same_maps\": %s, \"host_s\": %s, \"gpu_s\": %s, "
               "\"gpu_call_s\": %s, \"device_ms\": %s}\n",
               k, dir, n, fork_every, kept_n, same < 0 ? "null" : same ? "true" : "false", list(host_s).c_str(), list(gpu_s).c_str(),
               list(call_s).c_str(), list(dev_ms).c_str());
        mc_destroy(ctx);
        return same == 0 ? 1 : 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "mc_trim_paths_bench: %s\n", e.what());
        mc_destroy(ctx);
        return 1;
    }
}
