// mc_unitigs (include/mcgpu.h) as a Compactor of picture.h: what `metacherchant --compact gpu` hands to Environment::create_picture,
// and what mc_unitigs_bench times.  picture.{h,cpp} themselves stay free of the library (mc_hosttest builds them without it).
#pragma once
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "picture.h"
#include "mcgpu.h"

namespace mch {

// device_ms: where the call's device time goes (NULL: nowhere).  The context must outlive the compactor.
inline Compactor gpu_compactor(mc_ctx *ctx, double *device_ms = nullptr)
{
    return [ctx, device_ms](int k, const std::vector<kmer_t> &kmers, const std::vector<uint8_t> &cls, UnitigsResult &out) {
        const size_t n = kmers.size();
        std::vector<uint64_t> hi(k > 32 ? n : 0), lo(n);  // (one word a k-mer to k = 32: mc_unitigs takes no high words there)
        for (size_t i = 0; i < n; i++) lo[i] = (uint64_t)kmers[i];
        for (size_t i = 0; i < hi.size(); i++) hi[i] = (uint64_t)(kmers[i] >> 64);
        mc_unitigs_result r{};
        if (mc_unitigs(ctx, hi.empty() ? nullptr : hi.data(), lo.data(), cls.data(), n, &r) != MC_OK) throw Error(std::string(mc_last_error(ctx)));
        const uint64_t n_nbr = std::accumulate(r.deg, r.deg + r.n_nodes, (uint64_t)0);
        out.deg.assign(r.deg, r.deg + r.n_nodes);
        out.nbr.assign(r.nbr, r.nbr + n_nbr);
        out.first.assign(r.first, r.first + r.n_unitigs);
        out.last_rc.assign(r.last_rc, r.last_rc + r.n_unitigs);
        out.base_offsets.assign(r.base_offsets, r.base_offsets + r.n_unitigs + 1);
        out.bases.assign(r.bases, r.bases + r.base_offsets[r.n_unitigs] / 32);
        out.irregular.assign(r.irregular, r.irregular + r.n_irregular);
        if (device_ms) *device_ms = r.device_ms;
        mc_unitigs_free(&r);
    };
}

}  // namespace mch
