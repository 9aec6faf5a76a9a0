// mc_unitigs_bench: times the unitig compaction of one synthetic environment both ways through the one entry the tools use,
// make_picture (picture.h): without a compactor (the reference's loop on labels, `--compact host`) and with mc_unitigs as the
// compactor (`--compact gpu`: the k-mers up, the result back, the nodes built from it, the loop over the irregular entries).
// scripts/unitigs_bench.py runs it and takes the medians; DESIGN.md 3.12 has the figures.
//
//   mc_unitigs_bench <k> <entries> <seq_len> <reps> <device> <host|gpu|both>
//
// The environment: the k-mers of consecutive pieces of seq_len bases of the synthetic genome (mc_synth_genome, seed below), one
// chain a piece, a k-mer met again left out; entries in a seeded random order and orientation, as a HashMap's iteration order
// is no order of the genome.  One class.  Every run is a wall-clock time around work that ends on the host; the GPU runs come
// after one untimed run of the same size.  The two ways' alive nodes are compared once.  Prints one JSON line.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "envfinder.h"
#include "gpu_compactor.h"
#include "mcgpu.h"

using namespace mch;

namespace {

constexpr uint64_t GENOME_SEED = 20240531, ORDER_SEED = 42;

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

std::vector<kmer_t> environment(int k, size_t entries, size_t seq_len)
{
    const size_t per = seq_len - (size_t)k + 1, n_seqs = (entries + per - 1) / per;
    std::vector<uint8_t> codes(n_seqs * seq_len);
    if (mc_synth_genome(GENOME_SEED, 0, codes.size(), codes.data()) != MC_OK) throw Error("mc_synth_genome failed");
    const kmer_t mask = k >= 64 ? ~(kmer_t)0 : (((kmer_t)1 << (2 * k)) - 1);
    std::vector<std::pair<kmer_t, uint32_t>> canon;  // (canonical form, ordinal)
    std::vector<kmer_t> all;
    for (size_t s = 0; s < n_seqs; s++) {
        kmer_t v = 0;
        for (size_t i = 0; i < seq_len; i++) {
            v = ((v << 2) | codes[s * seq_len + i]) & mask;
            if (i + 1 >= (size_t)k) {
                canon.emplace_back(std::min(v, reverse_complement128(v, k)), (uint32_t)all.size());
                all.push_back(v);
            }
        }
    }
    std::sort(canon.begin(), canon.end());
    std::vector<char> again(all.size(), 0);
    for (size_t i = 1; i < canon.size(); i++)
        if (canon[i].first == canon[i - 1].first) again[canon[i].second] = 1;
    std::vector<kmer_t> kmers;
    for (size_t i = 0; i < all.size() && kmers.size() < entries; i++)
        if (!again[i]) kmers.push_back(all[i]);
    std::mt19937_64 rng(ORDER_SEED);
    for (size_t i = kmers.size(); i > 1; i--) std::swap(kmers[i - 1], kmers[(size_t)(rng() % i)]);
    for (kmer_t &v : kmers)
        if (rng() & 1) v = reverse_complement128(v, k);
    return kmers;
}

bool same_alive(const std::vector<PictureNode> &a, const std::vector<PictureNode> &b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) {
        if (a[i].deleted != b[i].deleted || a[i].neighbors != b[i].neighbors) return false;
        if (!a[i].deleted && (a[i].rc != b[i].rc || a[i].sequence != b[i].sequence)) return false;
    }
    return true;
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
        fprintf(stderr, "usage: mc_unitigs_bench <k> <entries> <seq_len> <reps> <device> <host|gpu|both>\n");
        return 2;
    }
    mc_ctx *ctx = nullptr;
    try {
        const int k = atoi(argv[1]), reps = atoi(argv[4]), device = atoi(argv[5]);
        const size_t entries = strtoull(argv[2], nullptr, 10), seq_len = strtoull(argv[3], nullptr, 10);
        const std::string what = argv[6];
        const bool host = what != "gpu", gpu = what != "host";
        if (k < 2 || k > 63 || seq_len < (size_t)k + 1 || reps < 1 || entries < 1) throw Error("k = 2 .. 63, seq_len > k, reps and entries >= 1");
        const std::vector<kmer_t> kmers = environment(k, entries, seq_len);
        const std::vector<uint8_t> cls(kmers.size(), 1);
        fprintf(stderr, "mc_unitigs_bench: k=%d, %zu entries\n", k, kmers.size());

        double device_ms = 0, in_compactor_s = 0;
        Compactor timed_gpu;
        if (gpu) {
            mc_config cfg{};
            cfg.k = k;
            cfg.key_mode = MC_KEY_POLY;
            cfg.device = device;
            if (mc_create(&cfg, &ctx) != MC_OK) throw Error(std::string(mc_last_error(nullptr)));
            const Compactor inner = gpu_compactor(ctx, &device_ms);
            timed_gpu = [inner, &in_compactor_s](int kk, const std::vector<kmer_t> &km, const std::vector<uint8_t> &c, UnitigsResult &out) {
                const double t0 = now_s();
                inner(kk, km, c, out);
                in_compactor_s = now_s() - t0;
            };
            make_picture(k, kmers, cls, &timed_gpu);  // (untimed: the code objects load, the scans' library sizes its blocks)
            fprintf(stderr, "mc_unitigs_bench: warm\n");
        }
        std::vector<double> host_s, gpu_s, compactor_s, dev_ms;
        size_t alive = 0;
        int same = -1;
        for (int r = 0; r < reps; r++) {  // (the two ways in turn: what else the machine does meets both)
            std::vector<PictureNode> h, g;
            if (host) {
                const double t0 = now_s();
                h = make_picture(k, kmers, cls, nullptr);
                host_s.push_back(now_s() - t0);
                fprintf(stderr, "mc_unitigs_bench: host %.3f s\n", host_s.back());
            }
            if (gpu) {
                const double t0 = now_s();
                g = make_picture(k, kmers, cls, &timed_gpu);
                gpu_s.push_back(now_s() - t0);
                compactor_s.push_back(in_compactor_s);
                dev_ms.push_back(device_ms);
                fprintf(stderr, "mc_unitigs_bench: gpu %.3f s\n", gpu_s.back());
            }
            if (r == 0) {
                for (const PictureNode &nd : host ? h : g) alive += !nd.deleted;
                if (host && gpu) same = same_alive(h, g) ? 1 : 0;
            }
        }
        printf("{\"k\": %d, \"entries\": %zu, \"seq_len\": %zu, \"alive_nodes\": %zu, \"same_nodes\": %s, \"host_s\": %s, \"gpu_s\": %s, "
               "\"gpu_compactor_s\": %s, \"device_ms\": %s}\n",
               k, kmers.size(), seq_len, alive, same < 0 ? "null" : same ? "true" : "false", list(host_s).c_str(), list(gpu_s).c_str(),
               list(compactor_s).c_str(), list(dev_ms).c_str());
        mc_destroy(ctx);
        return same == 0 ? 1 : 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "mc_unitigs_bench: %s\n", e.what());
        mc_destroy(ctx);
        return 1;
    }
}
