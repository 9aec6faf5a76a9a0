// libmcgpu.so, the presence unit: which of up to four tables hold each of a list of oriented k-mers (include/mcgpu.h
// mc_kmer_presence*; BigLong2ShortHashMap.contains as src/tools/RecipientVisualiser.java:157-169 asks it of four maps a k-mer).
// context.h lists the other units.
//
// A thread takes one k-mer.  It is keyed once, with the key functions the walk uses for its neighbours (kmer_device.h key_of);
// the home slots of all NT tables are loaded before any of them is looked at, so a lane has NT independent 16-byte reads at random
// places in flight; only a table whose home slot holds another key is probed further, in a second pass; one byte is stored.  The
// call is bound by the launch and by the latency of those reads, not by bandwidth (10^4 .. 10^6 k-mers a call: 16 .. 64 bytes each).
// DESIGN.md "presence" has the measurement, tests/test_presence_kernel_resources.py holds the kernels to their registers.
#include "context.h"

namespace {

constexpr int PR_THREADS = 256;

template <int NT>
struct PresenceTables {
    TableView t[NT];
};

// table_get's probing rule (kmer_device.h) behind the home slot `s`, which the caller has found occupied by another key: is the
// key there?  (Scalars, not a TableView: one copy of these loops serves all the tables.)
__device__ __forceinline__ bool present_behind_home(const Slot *__restrict__ slots, uint32_t rmask, uint32_t n_regions, uint64_t key, uint64_t s)
{
    uint64_t base = s & ~(uint64_t)rmask;
    const uint64_t home = s & rmask;
    const uint32_t max_probes = rmask + 1 < TABLE_MAX_PROBES ? rmask + 1 : TABLE_MAX_PROBES;
    for (uint32_t hop = 0; hop < TABLE_CHAIN; hop++, base = next_region_base(base, rmask, n_regions), s = base | home)
    for (uint32_t probe = 0; probe < max_probes; probe++) {
        if (hop | probe) {
            const uint4 r = *reinterpret_cast<const uint4 *>(slots + s);
            const uint64_t cur = ((uint64_t)r.y << 32) | r.x;
            if (cur == key) return true;
            if (cur == EMPTY_KEY) return false;
        }
        s = base | ((s + 1) & rmask);
    }
    return false;
}

template <int MODE, int NT>
__global__ void __launch_bounds__(PR_THREADS) k_presence(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint64_t n, int k,
                                                         PresenceTables<NT> tv, uint8_t *__restrict__ mask)
{
    const uint64_t i = (uint64_t)blockIdx.x * PR_THREADS + threadIdx.x;
    if (i >= n) return;
    const Kmer v{hi ? hi[i] : 0, lo[i]};
    const uint64_t key = (uint64_t)key_of<MODE>(v, k);
    // slot_of (kmer_device.h) for NT tables of one k: the key's hash and its minimizer bin are worked out once
    uint32_t bins = 0;  // packed keys: the tables whose regions are minimizer bins (mm_k = k); hash keys never are, by_key_ready saw to it
#pragma unroll
    for (int t = 0; t < NT; t++) bins |= (MODE == KEY_PACKED && tv.t[t].mm_k != 0 ? 1u : 0u) << t;
    const uint64_t mix = fmix64(key);
    const uint64_t bin = bins ? sk_bin(sk_hmin_of_kmer(key, k)) : 0;
    const uint64_t home = sk_home(key);
    uint64_t at[NT];
    uint4 raw[NT];
#pragma unroll
    for (int t = 0; t < NT; t++)
        at[t] = !(bins >> t & 1) ? mix >> tv.t[t].shift : (((bin * tv.t[t].n_regions) >> 32) << MC_REGION_LG) | home;
#pragma unroll
    for (int t = 0; t < NT; t++) raw[t] = *reinterpret_cast<const uint4 *>(tv.t[t].slots + at[t]);
    uint32_t m = 0, behind = 0;  // behind: the tables whose home slot holds another key
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const uint64_t cur = ((uint64_t)raw[t].y << 32) | raw[t].x;
        if (cur == key && (MODE == KEY_PACKED || key != EMPTY_KEY)) m |= 1u << t;
        else if (cur != EMPTY_KEY || (MODE != KEY_PACKED && key == EMPTY_KEY)) behind |= 1u << t;  // (or the key is the free slot's mark)
    }
    if (behind) {
#pragma unroll
        for (int t = 0; t < NT; t++) {  // (unrolled: the tables' arguments stay scalar registers, nothing is indexed)
            if (!(behind >> t & 1)) continue;
            bool in;
            if (MODE != KEY_PACKED && key == EMPTY_KEY) in = *tv.t[t].empty_cnt != 0;  // (table_get: such a hash is counted beside the table)
            else in = present_behind_home(tv.t[t].slots, tv.t[t].rmask, tv.t[t].n_regions, key, at[t]);
            m |= (in ? 1u : 0u) << t;
        }
    }
    mask[i] = (uint8_t)m;
}

struct PresenceCall {
    hipStream_t stream;
    mc_ctx *const *tables;
    const uint64_t *d_hi, *d_lo;
    uint64_t n;
    uint8_t *d_mask;
};

template <int MODE, int NT>
void launch_presence(const PresenceCall &a)
{
    PresenceTables<NT> tv;
    for (int t = 0; t < NT; t++) tv.t[t] = a.tables[t]->view();
    hipLaunchKernelGGL((k_presence<MODE, NT>), dim3((uint32_t)((a.n + PR_THREADS - 1) / PR_THREADS)), dim3(PR_THREADS), 0, a.stream, a.d_hi, a.d_lo,
                       a.n, a.tables[0]->cfg.k, tv, a.d_mask);
}

template <int MODE>
void launch_presence_n(uint32_t n_tables, const PresenceCall &a)
{
    switch (n_tables) {
    case 1: launch_presence<MODE, 1>(a); break;
    case 2: launch_presence<MODE, 2>(a); break;
    case 3: launch_presence<MODE, 3>(a); break;
    default: launch_presence<MODE, 4>(a); break;
    }
}

// null contexts and their number; the message goes to tables[0] when there is one
int check_tables(mc_ctx *const *tables, uint32_t n_tables)
{
    if (!tables || n_tables == 0 || n_tables > MC_PRESENCE_MAX_TABLES) {
        mc_ctx *c0 = tables && n_tables ? tables[0] : nullptr;
        if (c0) {
            std::lock_guard<std::mutex> g(c0->mu);
            return fail(c0, MC_EINVAL, "mc_kmer_presence: %u tables (1 .. %d)", n_tables, MC_PRESENCE_MAX_TABLES);
        }
        return MC_EINVAL;
    }
    if (!tables[0]) return MC_EINVAL;
    for (uint32_t t = 1; t < n_tables; t++)
        if (!tables[t]) {
            std::lock_guard<std::mutex> g(tables[0]->mu);
            return fail(tables[0], MC_EINVAL, "mc_kmer_presence: table %u is null", t);
        }
    return MC_OK;
}

}  // namespace

int mc_kmer_presence_dev(mc_ctx *const *tables, uint32_t n_tables, const uint64_t *d_hi, const uint64_t *d_lo, uint64_t n, uint8_t *d_mask)
{
    if (int rc = check_tables(tables, n_tables)) return rc;
    mc_ctx *c = tables[0];
    TablesLock lock(tables, n_tables);
    for (uint32_t t = 1; t < n_tables; t++)
        if (tables[t]->cfg.k != c->cfg.k || tables[t]->cfg.key_mode != c->cfg.key_mode || tables[t]->cfg.device != c->cfg.device)
            return fail(c, MC_EINVAL, "mc_kmer_presence: table %u has k = %d, key mode %d, device %d; table 0 has %d, %d, %d", t, tables[t]->cfg.k,
                        tables[t]->cfg.key_mode, tables[t]->cfg.device, c->cfg.k, c->cfg.key_mode, c->cfg.device);
    for (uint32_t t = 0; t < n_tables; t++)
        if (!tables[t]->finalized) return fail(c, MC_ESTATE, "mc_kmer_presence: call mc_finalize_counts on table %u first", t);
    if (n && (!d_lo || !d_mask || (!d_hi && c->cfg.k > 32))) return fail(c, MC_EINVAL, "mc_kmer_presence: null pointer");
    if ((n + PR_THREADS - 1) / PR_THREADS >= (1ull << 31)) return fail(c, MC_EINVAL, "mc_kmer_presence: %llu k-mers in one call", (unsigned long long)n);
    if (n == 0) return MC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    for (mc_ctx *x : lock.distinct) {
        // (hash keys in minimizer bins: the table moves to hash-prefix regions, once; an empty table that was never written is filled)
        int rc = by_key_ready(x);
        if (!rc) rc = materialize(x);
        if (rc) return x == c ? rc : fail(c, rc, "mc_kmer_presence: %s", x->err.c_str());
        if (x != c) HIPCHK(c, hipStreamSynchronize(x->stream));  // (its own stream did that; the kernel runs on table 0's)
    }
    const PresenceCall a{c->stream, tables, d_hi, d_lo, n, d_mask};
    if (c->cfg.key_mode == MC_KEY_PACKED) launch_presence_n<KEY_PACKED>(n_tables, a);
    else if (c->cfg.key_mode == MC_KEY_POLY) launch_presence_n<KEY_POLY>(n_tables, a);
    else launch_presence_n<KEY_FNV1A>(n_tables, a);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MC_OK;
}

int mc_kmer_presence(mc_ctx *const *tables, uint32_t n_tables, const uint64_t *hi, const uint64_t *lo, uint64_t n, uint8_t *mask)
{
    if (int rc = check_tables(tables, n_tables)) return rc;
    mc_ctx *c = tables[0];
    if (n == 0 || !lo || !mask || (!hi && c->cfg.k > 32))  // (nothing to copy: the device form checks the rest and says what is wrong)
        return mc_kmer_presence_dev(tables, n_tables, nullptr, nullptr, n, nullptr);
    DevBuf<uint64_t> dhi, dlo;
    DevBuf<uint8_t> dmask;
    {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(c, hipSetDevice(c->cfg.device));
        HIPCHK(c, dlo.alloc(n));
        HIPCHK(c, dmask.alloc(n));
        HIPCHK(c, hipMemcpy(dlo.p, lo, n * 8, hipMemcpyHostToDevice));
        if (hi) {
            HIPCHK(c, dhi.alloc(n));
            HIPCHK(c, hipMemcpy(dhi.p, hi, n * 8, hipMemcpyHostToDevice));
        }
    }
    int rc = mc_kmer_presence_dev(tables, n_tables, dhi.p, dlo.p, n, dmask.p);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipMemcpy(mask, dmask.p, n, hipMemcpyDeviceToHost));
    return MC_OK;
}
