// libmcgpu.so, the reads-classifier unit: per-read k-mer coverage of a read set in the table (include/mcgpu.h
// mc_classify_reads*; src/algo/ReadsFinderInGraph.java, src/algo/PairFinder.java).  context.h lists the other units.
//
// One wave per read, its windows over the lanes: every lane extracts its window's k-mer from the packed read, keys it
// (kmer_device.h key_of) and looks it up (table_get), then the wave sums the coverages with cross-lane shuffles.  A probe
// is one 16-byte slot read at a random place in the table: the kernel is bound by how many of them HBM serves, and a wave
// has up to 64 of them in flight.  DESIGN.md "Reads-classifier" has the roofline.
//
// k_triple_classes, the triple-reads-classifier's classes (mc_triple_classes*): one thread a pair, the rules of classify.h.
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

constexpr int TC_THREADS = 256;

// one thread a pair: the two mates' classes at this pass (prev1 == NULL: pass 1; else pass 2 with the pass-1 classes of the mates' last
// copies).  (A last index out of range -- the caller's mistake -- reads as NOT_FOUND rather than outside the array.)
__global__ void __launch_bounds__(TC_THREADS) k_triple_classes(const mc_read_cov *__restrict__ cov1, const mc_read_cov *__restrict__ cov2,
                                                               const uint64_t *__restrict__ off1, const uint64_t *__restrict__ off2, uint64_t n,
                                                               int k, double half, const uint8_t *__restrict__ prev1,
                                                               const uint8_t *__restrict__ prev2, const uint32_t *__restrict__ last1,
                                                               const uint32_t *__restrict__ last2, uint8_t *__restrict__ cls1,
                                                               uint8_t *__restrict__ cls2)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int32_t len1 = (int32_t)(off1[i + 1] - off1[i]), len2 = (int32_t)(off2[i + 1] - off2[i]);
        const mc_read_cov a = cov1[i], b = cov2[i];
        const bool f1 = a.found != 0;
        const bool f2 = len2 == 0 ? !f1 : b.found != 0;  // TripleFinder.java:44-46, TripleFinder2.java:54-56
        const double w1 = triple_width(a.covered, a.last, len1, k), w2 = triple_width(b.covered, b.last, len2, k);
        if (!prev1) {
            cls1[i] = triple_class_pass1(f1, w1, half);
            cls2[i] = triple_class_pass1(f2, w2, half);
        } else {
            const uint32_t j1 = last1[i], j2 = last2[i];
            cls1[i] = triple_class_pass2(f1, j1 < n ? prev1[j1] : (uint8_t)CLASS_NOT_FOUND, w1, half);
            cls2[i] = triple_class_pass2(f2, j2 < n ? prev2[j2] : (uint8_t)CLASS_NOT_FOUND, w2, half);
        }
    }
}

}  // namespace

int mc_triple_classes_dev(mc_ctx *c, const mc_read_cov *d_cov1, const mc_read_cov *d_cov2, const uint64_t *d_offsets1, const uint64_t *d_offsets2,
                          uint64_t n_pairs, int half_pct, const uint8_t *d_prev1, const uint8_t *d_prev2, const uint32_t *d_last1,
                          const uint32_t *d_last2, uint8_t *d_class1, uint8_t *d_class2)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (half_pct < 0 || half_pct > 100) return fail(c, MC_EINVAL, "mc_triple_classes: half_pct %d is outside 0 .. 100", half_pct);
    const int n_prev = !!d_prev1 + !!d_prev2 + !!d_last1 + !!d_last2;
    if (n_prev != 0 && n_prev != 4) return fail(c, MC_EINVAL, "mc_triple_classes: pass 2 needs both sides' classes and last copies");
    if (n_pairs && (!d_cov1 || !d_cov2 || !d_offsets1 || !d_offsets2 || !d_class1 || !d_class2))
        return fail(c, MC_EINVAL, "mc_triple_classes: null pointer");
    if (n_pairs == 0) return MC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const double half = (double)half_pct / 100;  // TripleReadsClassifier.java:203,229
    hipLaunchKernelGGL(k_triple_classes, dim3(grid_for(n_pairs, TC_THREADS, 1 << 16)), dim3(TC_THREADS), 0, c->stream, d_cov1, d_cov2, d_offsets1,
                       d_offsets2, n_pairs, c->cfg.k, half, d_prev1, d_prev2, d_last1, d_last2, d_class1, d_class2);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MC_OK;
}

int mc_triple_classes(mc_ctx *c, const mc_read_cov *cov1, const mc_read_cov *cov2, const uint64_t *offsets1, const uint64_t *offsets2, uint64_t n_pairs,
                      int half_pct, const uint8_t *prev1, const uint8_t *prev2, const uint32_t *last1, const uint32_t *last2, uint8_t *class1,
                      uint8_t *class2)
{
    if (!c) return MC_EINVAL;
    const bool pass2 = prev1 || prev2 || last1 || last2;
    if (n_pairs && (!cov1 || !cov2 || !offsets1 || !offsets2 || !class1 || !class2 || (pass2 && !(prev1 && prev2 && last1 && last2))))
        return fail(c, MC_EINVAL, "mc_triple_classes: null pointer");
    if (n_pairs == 0) return mc_triple_classes_dev(c, nullptr, nullptr, nullptr, nullptr, 0, half_pct, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    HostStage st(c);
    const mc_read_cov *dc1 = st.in(cov1, n_pairs), *dc2 = st.in(cov2, n_pairs);
    const uint64_t *do1 = st.in(offsets1, n_pairs + 1), *do2 = st.in(offsets2, n_pairs + 1);
    const uint8_t *dp1 = st.in(prev1, n_pairs), *dp2 = st.in(prev2, n_pairs);  // (pass 2: all four, checked above; else none)
    const uint32_t *dl1 = st.in(last1, n_pairs), *dl2 = st.in(last2, n_pairs);
    uint8_t *dk1 = st.out<uint8_t>(n_pairs), *dk2 = st.out<uint8_t>(n_pairs);
    if (int rc = st.staged()) return rc;
    if (int rc = mc_triple_classes_dev(c, dc1, dc2, do1, do2, n_pairs, half_pct, dp1, dp2, dl1, dl2, dk1, dk2)) return rc;
    if (int rc = st.back(class1, dk1, n_pairs)) return rc;
    return st.back(class2, dk2, n_pairs);
}

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
    for_key_mode(c->cfg.key_mode, [&](auto mode) {
        hipLaunchKernelGGL(k_classify<mode()>, grid, block, 0, c->stream, d_words, d_read_offsets, n_reads, d_bad_pos, k, c->view(), thr, z, corr, d_out);
    });
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
    HostStage st(c);
    const uint64_t *dw = st.in(words, packed_words(read_offsets, n_reads)), *doff = st.in(read_offsets, n_reads + 1);
    const int32_t *dbad = st.in(bad_pos, n_reads);
    mc_read_cov *dout = st.out<mc_read_cov>(n_reads);
    if (int rc = st.staged()) return rc;
    if (int rc = mc_classify_reads_dev(c, dw, doff, n_reads, dbad, found_pct, z, flags, dout)) return rc;
    return st.back(out, dout, n_reads);
}
