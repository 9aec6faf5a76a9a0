// libmcgpu.so, the presence unit: which of up to four tables hold each of a list of oriented k-mers (include/mcgpu.h
// mc_kmer_presence*; BigLong2ShortHashMap.contains as src/tools/RecipientVisualiser.java:157-169 asks it of four maps a k-mer).
// context.h lists the other units.
//
// A thread takes one k-mer.  It is keyed once, with the key functions the walk uses for its neighbours (kmer_device.h key_of);
// the home slots of all NT tables are loaded before any of them is looked at, so a lane has NT independent 16-byte reads at random
// places in flight (multi_table.h home_slots, shared with seq_cov.hip); only a table whose home slot holds another key is probed
// further, in a second pass; one byte is stored.  The
// call is bound by the launch and by the latency of those reads, not by bandwidth (10^4 .. 10^6 k-mers a call: 16 .. 64 bytes each).
// DESIGN.md "presence" has the measurement, tests/test_presence_kernel_resources.py holds the kernels to their registers.
#include "multi_table.h"

namespace {

constexpr int PR_THREADS = 256;

// a table's scalars stay kernel arguments: everything below is unrolled, so nothing indexes them
template <int NT>
struct ArgsOf {
    const Tables<NT> &tv;
    __device__ __forceinline__ uint32_t shift(int t) const { return tv.t[t].shift; }
    __device__ __forceinline__ uint32_t n_regions(int t) const { return tv.t[t].n_regions; }
};

template <int MODE, int NT>
__global__ void __launch_bounds__(PR_THREADS) k_presence(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint64_t n, int k,
                                                         Tables<NT> tv, uint8_t *__restrict__ mask)
{
    const uint64_t i = (uint64_t)blockIdx.x * PR_THREADS + threadIdx.x;
    if (i >= n) return;
    const Kmer v{hi ? hi[i] : 0, lo[i]};
    const uint64_t key = (uint64_t)key_of<MODE>(v, k);
    uint32_t m = 0;
    uint64_t at[NT];
    const uint32_t behind = home_slots<MODE>(tv, bin_tables<MODE>(tv), key, k, ArgsOf<NT>{tv}, at, [&](int t, bool there, uint32_t) { if (there) m |= 1u << t; });  // (a key counted 0 times is present)
    if (behind) {
#pragma unroll
        for (int t = 0; t < NT; t++) {  // (unrolled: the tables' arguments stay scalar registers, nothing is indexed)
            if (!(behind >> t & 1)) continue;
            const bool in = get_behind_home<MODE, false>(tv.t[t].slots, tv.t[t].empty_cnt, tv.t[t].rmask, tv.t[t].n_regions, key, at[t]);
            m |= (in ? 1u : 0u) << t;
        }
    }
    mask[i] = (uint8_t)m;
}

constexpr char API[] = "mc_kmer_presence";

}  // namespace

int mc_kmer_presence_dev(mc_ctx *const *tables, uint32_t n_tables, const uint64_t *d_hi, const uint64_t *d_lo, uint64_t n, uint8_t *d_mask)
{
    if (int rc = check_tables(API, MC_PRESENCE_MAX_TABLES, tables, n_tables)) return rc;
    mc_ctx *c = tables[0];
    TablesLock lock(tables, n_tables);
    if (int rc = tables_agree(API, tables, n_tables)) return rc;
    if (n && (!d_lo || !d_mask || (!d_hi && c->cfg.k > 32))) return fail(c, MC_EINVAL, "%s: null pointer", API);
    if ((n + PR_THREADS - 1) / PR_THREADS >= (1ull << 31)) return fail(c, MC_EINVAL, "%s: %llu k-mers in one call", API, (unsigned long long)n);
    if (n == 0) return MC_OK;
    if (int rc = prepare_tables(API, c, lock)) return rc;
    for_key_mode_and_tables(c->cfg.key_mode, n_tables, [&](auto mode, auto nt) {
        hipLaunchKernelGGL((k_presence<mode(), nt()>), dim3((uint32_t)((n + PR_THREADS - 1) / PR_THREADS)), dim3(PR_THREADS), 0, c->stream, d_hi, d_lo, n,
                           c->cfg.k, tables_view<nt()>(tables), d_mask);
    });
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MC_OK;
}

int mc_kmer_presence(mc_ctx *const *tables, uint32_t n_tables, const uint64_t *hi, const uint64_t *lo, uint64_t n, uint8_t *mask)
{
    if (int rc = check_tables(API, MC_PRESENCE_MAX_TABLES, tables, n_tables)) return rc;
    mc_ctx *c = tables[0];
    if (n == 0 || !lo || !mask || (!hi && c->cfg.k > 32))  // (nothing to copy: the device form checks the rest and says what is wrong)
        return mc_kmer_presence_dev(tables, n_tables, nullptr, nullptr, n, nullptr);
    HostStage st(c);
    const uint64_t *dlo = st.in(lo, n), *dhi = st.in(hi, n);
    uint8_t *dmask = st.out<uint8_t>(n);
    if (int rc = st.staged()) return rc;
    if (int rc = mc_kmer_presence_dev(tables, n_tables, dhi, dlo, n, dmask)) return rc;
    return st.back(mask, dmask, n);
}
