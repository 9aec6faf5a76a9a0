// What the tools of the `metacherchant` CLI keep on the device themselves: HIP's host API only, no device code.  Memory that grows
// (DevArray, PinnedStage), a file of whole reads read by the host or by the device (ReadsIn: the classifiers, seq-cov, fmt-visualizer,
// environment-assembler-finder) and one side of such reads joined on the device (SideStore: triple-reads-classifier, fmt-visualizer).
#pragma once
#include <algorithm>
#include <memory>

#include <hip/hip_runtime_api.h>

#include "cli.h"
#include "whole_reads_source.h"

namespace mch {

inline void hip_check(hipError_t e, const char *what)
{
    if (e != hipSuccess) throw Error(std::string(what) + ": " + hipGetErrorString(e));
}

// device memory of the tool's own, grown by doubling
struct DevArray {
    char *p = nullptr;
    size_t cap = 0, size = 0;
    DevArray() = default;
    DevArray(const DevArray &) = delete;
    DevArray &operator=(const DevArray &) = delete;
    ~DevArray() { if (p) (void)hipFree(p); }
    void reserve(size_t bytes)
    {
        if (bytes <= cap) return;
        const size_t nc = std::max(bytes, 2 * cap);
        char *q = nullptr;
        hip_check(hipMalloc(reinterpret_cast<void **>(&q), nc), "hipMalloc");
        if (size) hip_check(hipMemcpy(q, p, size, hipMemcpyDeviceToDevice), "hipMemcpy");
        if (p) (void)hipFree(p);
        p = q;
        cap = nc;
    }
    void put(size_t at, const void *h, size_t bytes)  // host bytes to [at, at + bytes)
    {
        reserve(at + bytes);
        if (bytes) hip_check(hipMemcpy(p + at, h, bytes, hipMemcpyHostToDevice), "hipMemcpy");
        size = std::max(size, at + bytes);
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = size = 0;
    }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// a file of whole reads, read one way or the other
struct ReadsIn {
    std::unique_ptr<DnaQReader> host;
    std::unique_ptr<WholeReadsSource> gpu;
    mc_ctx *ctx;
    ReadsIn(const Options &o, mc_ctx *c, const std::string &path) : ctx(c)
    {
        if (parse_on_gpu(o, path)) gpu.reset(new WholeReadsSource(ctx, o.device, path));
        else host.reset(new DnaQReader(path));
    }
    size_t read(DnaQBatch &b, size_t max_reads, uint64_t max_bases = ~0ull) { return gpu ? gpu->read(b, max_reads, max_bases) : host->read(b, max_reads); }
};

// page-locked host memory that grows: where the rendered text comes down
struct PinnedStage {
    uint8_t *p = nullptr;
    size_t cap = 0;
    PinnedStage() = default;
    PinnedStage(const PinnedStage &) = delete;
    PinnedStage &operator=(const PinnedStage &) = delete;
    ~PinnedStage() { if (p) (void)hipHostFree(p); }
    void reserve(size_t bytes)
    {
        if (bytes <= cap) return;
        const size_t nc = std::max(bytes, 2 * cap);
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        hip_check(hipHostMalloc(reinterpret_cast<void **>(&p), nc), "hipHostMalloc");
        cap = nc;
    }
};

// findReadWithCorrection's one low-quality position of each of the first n reads: -1 for none, -2 for several (mc_classify_reads)
inline std::vector<int32_t> bad_positions(const DnaQBatch &b, size_t n)
{
    return low_quality_positions(b, 0, n);
}

// one side of the pairs on the device, in mc_classify_reads' layout: words (the pad word included), offsets, bad positions
struct SideStore {
    DevArray words, offsets, bad;
    uint64_t n_reads = 0, n_bases = 0, carry = 0;  // carry: the partly filled last word, written again with the next batch
    void add(const DnaQBatch &b, size_t n, bool correction)
    {
        if (n_reads == 0) {
            const uint64_t z = 0;
            offsets.put(0, &z, 8);
        }
        const uint64_t nb = b.offsets[n], end = n_bases + nb, w0 = n_bases / 32;
        std::vector<uint64_t> w((end + 31) / 32 - w0 + 1, 0);
        w[0] = carry;
        for (uint64_t i = 0; i < nb; i++) {
            const uint64_t g = n_bases + i;
            w[g / 32 - w0] |= (uint64_t)(b.codes[i] & 3) << (62 - 2 * (g & 31));
        }
        words.put(w0 * 8, w.data(), w.size() * 8);
        carry = end % 32 ? w[end / 32 - w0] : 0;
        std::vector<uint64_t> off(n);
        for (size_t i = 0; i < n; i++) off[i] = n_bases + b.offsets[i + 1];
        offsets.put((n_reads + 1) * 8, off.data(), n * 8);
        if (correction) {
            const std::vector<int32_t> bp = bad_positions(b, n);
            bad.put(n_reads * 4, bp.data(), n * 4);
        }
        n_reads += n;
        n_bases = end;
    }
    // --parse gpu: the first n reads of a batch's device view, joined behind what is here on the device (mc_reads_append_dev).  A store
    // is filled one way or the other, never both (the host's way keeps the last word here).
    void add_dev(mc_ctx *ctx, const std::vector<WholeSegment> &segs, const DnaQBatch &b, size_t n, bool correction)
    {
        if (n_reads == 0 && words.size == 0) {
            const uint64_t z = 0;
            words.put(0, &z, 8);
            offsets.put(0, &z, 8);
        }
        const uint64_t end = n_bases + b.offsets[n];
        words.reserve(((end + 31) / 32 + 1) * 8);
        offsets.reserve((n_reads + n + 1) * 8);
        if (correction) bad.reserve((n_reads + n) * 4);
        uint64_t at_reads = n_reads, at_bases = n_bases;
        for (const WholeSegment &g : segs) {
            if (g.first >= n) break;  // (pairs end with the shorter file)
            const uint64_t m = std::min<uint64_t>(g.n_reads, n - g.first);
            MC_CHECK(ctx, mc_reads_append_dev(ctx, g.d_words, g.d_offsets, m, words.as<uint64_t>(), at_bases, offsets.as<uint64_t>() + at_reads));
            if (correction && m) hip_check(hipMemcpy(bad.p + at_reads * 4, g.d_bad_pos, m * 4, hipMemcpyDeviceToDevice), "hipMemcpy");
            at_bases += b.offsets[g.first + m] - b.offsets[g.first];
            at_reads += m;
        }
        if (at_reads != n_reads + n || at_bases != end) throw Error("internal: a batch's device view does not cover it");
        words.size = ((end + 31) / 32 + 1) * 8;
        offsets.size = (n_reads + n + 1) * 8;
        if (correction) bad.size = (n_reads + n) * 4;
        n_reads += n;
        n_bases = end;
    }
};

}  // namespace mch
