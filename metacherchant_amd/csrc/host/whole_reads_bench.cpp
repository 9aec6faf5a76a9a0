// mc_whole_reads_bench <reads file> host|gpu: the reader stage of the classifying tools alone, timed.  host: DnaQReader, then the
// packing and the low-quality positions as classify_batch does them, and the copy of words, offsets and positions to the device (what
// mc_classify_reads' host form does first); gpu: WholeReadsSource to its device view, the batch's codes and phreds copied back for the
// writers.  Batches of 2^20 reads, as the reads-classifier takes them.  Prints "<reads> <bases> <seconds>"; scripts/whole_reads_bench.py
// runs it.
#include <chrono>
#include <cstdio>
#include <cstring>

#include "whole_reads_source.h"

using namespace mch;

int main(int argc, char **argv)
{
    if (argc != 3 || (strcmp(argv[2], "host") && strcmp(argv[2], "gpu"))) {
        fprintf(stderr, "usage: mc_whole_reads_bench <reads file> host|gpu\n");
        return 2;
    }
    try {
        mc_config cfg{};
        cfg.k = 21;
        mc_ctx *ctx = nullptr;
        if (mc_create(&cfg, &ctx) != MC_OK) throw Error(std::string("mc_create: ") + mc_last_error(nullptr));
        (void)hipFree(nullptr);
        const auto t0 = std::chrono::steady_clock::now();
        constexpr size_t BATCH = 1u << 20;
        uint64_t reads = 0, bases = 0;
        DnaQBatch b;
        if (!strcmp(argv[2], "gpu")) {
            WholeReadsSource src(ctx, 0, argv[1]);
            for (;;) {
                b.clear();
                const size_t n = src.read(b, BATCH);
                if (n == 0) break;
                reads += n;
                bases += b.offsets[n];
            }
        } else {
            DnaQReader reader(argv[1]);
            char *d = nullptr;
            size_t cap = 0;
            for (;;) {
                b.clear();
                const size_t n = reader.read(b, BATCH);
                if (n == 0) break;
                const uint64_t nb = b.offsets[n];
                std::vector<uint64_t> words;
                pack_whole_reads(b, 0, n, words, nullptr);
                const std::vector<int32_t> bad = low_quality_positions(b, 0, n);
                const size_t wb = words.size() * 8, ob = (n + 1) * 8, need = wb + ob + n * 4;
                if (need > cap) {
                    if (d) (void)hipFree(d);
                    if (hipMalloc(reinterpret_cast<void **>(&d), need) != hipSuccess) throw Error("hipMalloc");
                    cap = need;
                }
                if (hipMemcpy(d, words.data(), wb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d + wb, b.offsets.data(), ob, hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(d + wb + ob, bad.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess)
                    throw Error("hipMemcpy");
                reads += n;
                bases += nb;
            }
            if (d) (void)hipFree(d);
        }
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("%llu %llu %.4f\n", (unsigned long long)reads, (unsigned long long)bases, s);
        mc_destroy(ctx);
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
