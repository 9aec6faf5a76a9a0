// mc_env_join (include/mcgpu.h) as a Joiner of multi.h: what `metacherchant --tool environment-finder-multi --join gpu` hands to
// environment_finder_multi_packed.  multi.{h,cpp} themselves stay free of the library (mc_hosttest builds them without it).
#pragma once
#include <string>
#include <vector>

#include "multi.h"
#include "mcgpu.h"

namespace mch {

// device_ms: where the call's device time goes (NULL: nowhere).  The context must outlive the joiner.
inline Joiner gpu_joiner(mc_ctx *ctx, double *device_ms = nullptr)
{
    return [ctx, device_ms](const EnvJoinInput &in, EnvJoinResult &out) {
        const size_t n = in.entries.size(), n_rec = in.rec_kmers.size(), G = in.n_graphs();
        const bool wide = in.k > 32;  // (one word a k-mer to k = 32: mc_env_join takes no high words there)
        std::vector<uint64_t> hi(wide ? n : 0), lo(n), rec_hi(wide ? n_rec : 0), rec_lo(n_rec);
        for (size_t i = 0; i < n; i++) lo[i] = (uint64_t)in.entries[i];
        for (size_t i = 0; i < hi.size(); i++) hi[i] = (uint64_t)(in.entries[i] >> 64);
        for (size_t i = 0; i < n_rec; i++) rec_lo[i] = (uint64_t)in.rec_kmers[i];
        for (size_t i = 0; i < rec_hi.size(); i++) rec_hi[i] = (uint64_t)(in.rec_kmers[i] >> 64);
        mc_env_join_result r{};
        if (mc_env_join(ctx, wide ? hi.data() : nullptr, lo.data(), n, wide ? rec_hi.data() : nullptr, rec_lo.data(), in.rec_depth.data(),
                        in.graph_offsets.data(), (uint32_t)G, in.gene_len ? in.gene_words.data() : nullptr, in.gene_len, &r) != MC_OK)
            throw Error(std::string(mc_last_error(ctx)));
        out.member.assign(r.member, r.member + n);
        out.is_gene.assign(r.is_gene, r.is_gene + n);
        out.kc.assign(r.kc, r.kc + n);
        out.diff.assign(r.diff, r.diff + G * G);
        out.diff_alt.assign(r.diff_alt, r.diff_alt + G * G);
        out.uni.assign(r.uni, r.uni + G * G);
        if (device_ms) *device_ms = r.device_ms;
        mc_env_join_free(&r);
    };
}

}  // namespace mch
