// libmcgpu.so, the reads-classifier unit: per-read k-mer coverage of a read set in the table (include/mcgpu.h
// mc_classify_reads*; src/algo/ReadsFinderInGraph.java, src/algo/PairFinder.java).  context.h lists the other units.
//
// One wave per read, its windows over the lanes: every lane extracts its window's k-mer from the packed read, keys it
// (kmer_device.h key_of) and looks it up (table_get), then the wave sums the coverages with cross-lane shuffles.  A probe
// is one 16-byte slot read at a random place in the table: the kernel is bound by how many of them HBM serves, and a wave
// has up to 64 of them in flight.  DESIGN.md "Reads-classifier" has the roofline.
#include "context.h"
#include "classify.h"

namespace {

constexpr int CL_THREADS = 256;

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// base i (0 = first) of an oriented k-mer set to code b
__device__ __forceinline__ void set_base(Kmer &v, int k, int i, uint32_t b)
{
    const int sh = 2 * (k - 1 - i);
    if (sh >= 64) v.hi = (v.hi & ~(3ull << (sh - 64))) | ((uint64_t)b << (sh - 64));
    else v.lo = (v.lo & ~(3ull << sh)) | ((uint64_t)b << sh);
}

// getWithZero (itmo!/structures/map/BigLong2ShortHashMap.java): the saturated count, 0 when absent
template <int MODE>
__device__ __forceinline__ uint32_t cov_of(const TableView &t, const Kmer &v, int k)
{
    const int c = table_get(t, (uint64_t)key_of<MODE>(v, k));
    return c > 0 ? (uint32_t)c : 0u;
}

template <int MODE>
__global__ void __launch_bounds__(CL_THREADS) k_classify(const uint64_t *__restrict__ words, const uint64_t *__restrict__ offsets,
                                                         uint64_t n_reads, const int32_t *__restrict__ bad_pos, int k, TableView t,
                                                         double thr, double z, int correction, mc_read_cov *__restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t r = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < n_reads; r += n_waves) {
        const uint64_t b = offsets[r];
        const uint32_t len = (uint32_t)(offsets[r + 1] - b);  // (a Java int: reads are shorter than 2^31 bases)
        mc_read_cov rec{0, 0, 0, 0, 0};
        if (len >= (uint32_t)k) {
            const uint32_t nwin = len - (uint32_t)k + 1;
            // findReadWithCorrection's one low-quality position p: the windows lo_w .. hi_w cover it
            int32_t p = correction && bad_pos ? bad_pos[r] : -1;
            if (p >= (int32_t)len) p = -1;  // (not a position of this read: the caller's mistake, read as "none")
            const uint32_t lo_w = p >= 0 ? (uint32_t)max(p - (k - 1), 0) : 1, hi_w = p >= 0 ? min((uint32_t)p, nwin - 1) : 0;
            uint32_t s = 0, cv = 0, rs = 0, rc = 0, lastc = 0;
            for (uint32_t w = lane; w < nwin; w += 64) {
                const uint32_t c = cov_of<MODE>(t, extract_kmer(words, b + w, k), k);
                s += c;
                cv += c > 0;
                if (w == nwin - 1) lastc = c;
                if (w >= lo_w && w <= hi_w) { rs += c; rc += c > 0; }
            }
            s = wave_sum_u32(s);
            cv = wave_sum_u32(cv);
            lastc = wave_sum_u32(lastc);  // (one lane holds it)
            rec.sum = (int32_t)s;
            rec.covered = (int32_t)cv;
            rec.last = (int16_t)lastc;
            // findRead on the read as given (step -1), or -- findReadWithCorrection's one low-quality position -- on the four
            // substitutions at p (steps 0 .. 3) until one passes: the windows that cover p (at most k <= 63: one a lane) are looked
            // up again and take the place of their old coverages in the sums; the threshold is then the reference's constant 0.9.
            // (One call of the verdict: its double-precision exp and sqrt are inlined once.)
            if (p >= 0) { rs = wave_sum_u32(rs); rc = wave_sum_u32(rc); }
            const uint32_t w = lo_w + lane;
            const bool mine = p >= 0 && w <= hi_w;
            Kmer v{0, 0};
            if (mine) v = extract_kmer(words, b + w, k);
            for (int step = p >= 0 ? 0 : -1;; step++) {
                uint32_t vs = s, vc = cv, vl = lastc;
                if (step >= 0) {
                    uint32_t c = 0;
                    if (mine) {
                        Kmer u = v;
                        set_base(u, k, p - (int32_t)w, (uint32_t)step);
                        c = cov_of<MODE>(t, u, k);
                    }
                    vs = s - rs + wave_sum_u32(c);
                    vc = cv - rc + wave_sum_u32(c > 0);
                    if (hi_w == nwin - 1) vl = wave_sum_u32(w == hi_w ? c : 0u);
                }
                rec.found = classify_verdict((int32_t)vs, (int32_t)vc, (int32_t)vl, (int32_t)len, k, step >= 0 ? 0.9 : thr, z);
                if (rec.found || step < 0 || step == 3) break;
            }
        }
        if (lane == 0) out[r] = rec;
    }
}

}  // namespace

int mc_classify_reads_dev(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_read_offsets, uint64_t n_reads, const int32_t *d_bad_pos,
                          int found_pct, double z, int flags, mc_read_cov *d_out)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->finalized) return fail(c, MC_ESTATE, "mc_classify_reads: call mc_finalize_counts first");
    if (n_reads && (!d_words || !d_read_offsets || !d_out)) return fail(c, MC_EINVAL, "mc_classify_reads: null pointer");
    if (found_pct < 0 || found_pct > 100) return fail(c, MC_EINVAL, "mc_classify_reads: found_pct %d is outside 0 .. 100", found_pct);
    if (n_reads == 0) return MC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // (hash keys in minimizer bins: a window's key does not say where it lives -- the table moves to hash-prefix regions, once)
    if (int brc = by_key_ready(c)) return brc;
    if (int mrc = materialize(c)) return mrc;  // (an empty table that was never written)
    const double thr = (double)found_pct / 100;  // ReadsClassifier.java:178
    const int corr = (flags & MC_CLASSIFY_CORRECTION) ? 1 : 0;
    const dim3 grid(grid_for(n_reads * 64, CL_THREADS, 1 << 18)), block(CL_THREADS);
    const int k = c->cfg.k;
    if (c->cfg.key_mode == MC_KEY_PACKED)
        hipLaunchKernelGGL(k_classify<KEY_PACKED>, grid, block, 0, c->stream, d_words, d_read_offsets, n_reads, d_bad_pos, k, c->view(), thr, z, corr, d_out);
    else if (c->cfg.key_mode == MC_KEY_POLY)
        hipLaunchKernelGGL(k_classify<KEY_POLY>, grid, block, 0, c->stream, d_words, d_read_offsets, n_reads, d_bad_pos, k, c->view(), thr, z, corr, d_out);
    else
        hipLaunchKernelGGL(k_classify<KEY_FNV1A>, grid, block, 0, c->stream, d_words, d_read_offsets, n_reads, d_bad_pos, k, c->view(), thr, z, corr, d_out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MC_OK;
}

int mc_classify_reads(mc_ctx *c, const uint64_t *words, const uint64_t *read_offsets, uint64_t n_reads, const int32_t *bad_pos, int found_pct,
                      double z, int flags, mc_read_cov *out)
{
    if (!c) return MC_EINVAL;
    if (n_reads && (!words || !read_offsets || !out)) return fail(c, MC_EINVAL, "mc_classify_reads: null pointer");
    if (n_reads == 0) return mc_classify_reads_dev(c, nullptr, nullptr, 0, nullptr, found_pct, z, flags, nullptr);
    const uint64_t n_words = (read_offsets[n_reads] + 31) / 32 + 1;
    DevBuf<uint64_t> dw, doff;
    DevBuf<int32_t> dbad;
    DevBuf<mc_read_cov> dout;
    {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(c, hipSetDevice(c->cfg.device));
        HIPCHK(c, dw.alloc(n_words));
        HIPCHK(c, doff.alloc(n_reads + 1));
        HIPCHK(c, dout.alloc(n_reads));
        HIPCHK(c, hipMemcpy(dw.p, words, n_words * 8, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(doff.p, read_offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice));
        if (bad_pos) {
            HIPCHK(c, dbad.alloc(n_reads));
            HIPCHK(c, hipMemcpy(dbad.p, bad_pos, n_reads * 4, hipMemcpyHostToDevice));
        }
    }
    int rc = mc_classify_reads_dev(c, dw.p, doff.p, n_reads, dbad.p, found_pct, z, flags, dout.p);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipMemcpy(out, dout.p, n_reads * sizeof(mc_read_cov), hipMemcpyDeviceToHost));
    return MC_OK;
}
