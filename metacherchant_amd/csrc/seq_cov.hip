// libmcgpu.so, the seq-cov unit: depth and breadth of every sequence's k-mers in up to four tables at once (include/mcgpu.h
// mc_seq_coverage*; src/tools/SequenceCoverage.java:162-185).  context.h lists the other units.
//
// The work is cut by base positions of the flattened store, not by sequences: a workgroup takes a tile of SC_TILE positions, each
// thread SC_ITEMS of them in a row, so a 5 Mbase contig and five million 1-base sequences both spread over the whole device.  One
// wave finds the sequence of the tile's first position by a 64-ary search in seq_offsets; a thread gallops from there to its own
// and then walks the boundaries.  A window is extracted and keyed once; its home slots in all NT tables are loaded before any
// of them is looked at (NT independent 16-byte reads at random places are in flight a lane, where k_classify has one), and only
// a window whose home slot holds another key goes on probing.  DESIGN.md "seq-cov" has the roofline.
//
// Sums: a thread adds what its windows of one sequence found in 32 bits (SC_ITEMS x 32767), a wave adds its lanes' runs of one
// sequence with a segmented scan (sequence numbers do not decrease along the lanes), the last lane of a run adds it to the
// tile's entry of that sequence in LDS (still 32 bits: SC_TILE x 32767 < 2^32, asserted below), and the tile gives every
// (sequence, table) it covered one 64-bit atomic add a number into d_out.  Integer adds: the same bits in any order.
#include "context.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_ITEMS = 8;                      // positions a thread
constexpr int SC_TILE = SC_THREADS * SC_ITEMS;   // positions a workgroup takes at a time
constexpr int SC_SEGS = 256;                     // sequences of a tile that have an entry in LDS; those behind go to d_out directly
static_assert((uint64_t)SC_TILE * 32767u < (1ull << 32), "a tile's depth must fit 32 bits");
// (Registers and occupancy: DESIGN.md "seq-cov" has the counts, tests/test_seq_cov_kernel_resources.py holds the kernels to them.)

struct SeqCovRare {
    const Slot *slots;
    const unsigned long long *empty_cnt;
    uint32_t rmask, n_regions, shift, pad;
};

template <int NT>
struct SeqCovTables {
    TableView t[NT];
};

// table_get's probing rule (kmer_device.h) behind the home slot `s`, which the caller has found occupied by another key;
// getWithZero: the saturated count, 0 when absent.  (Scalars, not a TableView: one copy of these loops serves all the tables.)
__device__ __forceinline__ uint32_t cov_behind_home(const Slot *__restrict__ slots, uint32_t rmask, uint32_t n_regions, uint64_t key, uint64_t s)
{
    uint64_t base = s & ~(uint64_t)rmask;
    const uint64_t home = s & rmask;
    const uint32_t max_probes = rmask + 1 < TABLE_MAX_PROBES ? rmask + 1 : TABLE_MAX_PROBES;
    for (uint32_t hop = 0; hop < TABLE_CHAIN; hop++, base = next_region_base(base, rmask, n_regions), s = base | home)
    for (uint32_t probe = 0; probe < max_probes; probe++) {
        if (hop | probe) {
            const uint4 r = *reinterpret_cast<const uint4 *>(slots + s);
            const uint64_t cur = ((uint64_t)r.y << 32) | r.x;
            if (cur == key) return r.z > 32767u ? 32767u : r.z;
            if (cur == EMPTY_KEY) return 0;
        }
        s = base | ((s + 1) & rmask);
    }
    return 0;
}

// the greatest s in [lo, hi) with offsets[s] <= p, given offsets[lo] <= p < offsets[hi]; the whole wave calls it with the same
// arguments and looks at 64 places a round
__device__ __forceinline__ uint64_t wave_find_seq(const uint64_t *__restrict__ offsets, uint64_t lo, uint64_t hi, uint64_t p, uint32_t lane)
{
    while (hi - lo > 1) {
        const uint64_t step = (hi - lo + 63) / 64;
        const uint64_t at = lo + (lane + 1) * step;
        const bool le = at < hi && offsets[at] <= p;
        const uint64_t c = (uint64_t)__popcll(__ballot(le));  // (sorted: the lanes below c)
        const uint64_t nlo = lo + c * step;
        hi = min(hi, nlo + step);
        lo = nlo;
    }
    return lo;
}

template <int MODE, int NT>
__global__ void __launch_bounds__(SC_THREADS) k_seq_cov(const uint64_t *__restrict__ words, const uint64_t *__restrict__ offsets,
                                                                      uint64_t n_seqs, uint64_t first, uint64_t end_all, int k, SeqCovTables<NT> tv,
                                                                      mc_seq_cov *__restrict__ out)
{
    __shared__ uint32_t s_acc[SC_SEGS][2 * NT];  // depth of table 0 .. NT-1, then breadth
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    unsigned long long *const out64 = reinterpret_cast<unsigned long long *>(out);  // (seq, table): depth, breadth
    // What only the rare paths need of a table waits in LDS, read by the table's number: the kernel arguments would hold four scalar
    // registers a table for the whole kernel (and indexing them would put them in scratch).
    __shared__ SeqCovRare s_rare[NT];
    uint32_t bins = 0;  // packed keys: the tables whose regions are minimizer bins (mm_k = k); hash keys never are, by_key_ready saw to it
#pragma unroll
    for (int t = 0; t < NT; t++) {
        bins |= (tv.t[t].mm_k != 0 ? 1u : 0u) << t;
        if (tid == (uint32_t)t) s_rare[t] = SeqCovRare{tv.t[t].slots, tv.t[t].empty_cnt, tv.t[t].rmask, tv.t[t].n_regions, tv.t[t].shift, 0};
    }

    const uint64_t p0 = first + (uint64_t)blockIdx.x * SC_TILE;  // (a tile a workgroup)
    const uint64_t p_end = min(p0 + SC_TILE, end_all);
    const uint64_t s0 = wave_find_seq(offsets, 0, n_seqs, p0, lane);
    for (uint32_t i = tid; i < SC_SEGS * 2 * NT; i += SC_THREADS) (&s_acc[0][0])[i] = 0;
    __syncthreads();

    // what this thread's windows of sequence s have found so far goes to the tile's entry of s (or, beyond SC_SEGS, to d_out)
    uint32_t acc[2 * NT];
#pragma unroll
    for (int i = 0; i < 2 * NT; i++) acc[i] = 0;
    auto flush = [&](uint64_t s) {
        uint32_t any = 0;  // (depth > 0 where breadth > 0)
#pragma unroll
        for (int t = 0; t < NT; t++) any |= acc[NT + t];
        if (!any) return;
        const uint64_t j = s - s0;
        if (j < SC_SEGS) {
#pragma unroll
            for (int i = 0; i < 2 * NT; i++) atomicAdd(&s_acc[j][i], acc[i]);
        } else {
#pragma unroll
            for (int i = 0; i < 2 * NT; i++) atomicAdd(&out64[(s * NT + (i % NT)) * 2 + i / NT], (unsigned long long)acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 2 * NT; i++) acc[i] = 0;
    };

    const uint64_t pt = p0 + (uint64_t)tid * SC_ITEMS;
    const bool active = pt < p_end;
    uint64_t s = s0;
    if (active) {
        // this thread's sequence: gallop from the tile's, then bisect
        uint64_t step = 1;
        while (s + step < n_seqs && offsets[s + step] <= pt) { s += step; step <<= 1; }
        uint64_t hi = min(s + step, n_seqs);
        while (hi - s > 1) {
            const uint64_t mid = s + (hi - s) / 2;
            if (offsets[mid] <= pt) s = mid; else hi = mid;
        }
        uint64_t seq_end = offsets[s + 1];
#pragma unroll 1
        for (int it = 0; it < SC_ITEMS; it++) {
            const uint64_t p = pt + it;
            if (p >= p_end) break;
            if (p >= seq_end) {
                flush(s);
                do seq_end = offsets[++s + 1]; while (p >= seq_end);  // (empty sequences in between; p < offsets[n_seqs])
            }
            if (p + k > seq_end) continue;  // no window starts here
            const uint64_t key = (uint64_t)key_of<MODE>(extract_kmer(words, p, k), k);
            // slot_of (kmer_device.h) for NT tables of one k: the key's hash and its minimizer bin are worked out once
            const uint64_t mix = fmix64(key);
            const uint64_t bin = MODE == KEY_PACKED && bins ? sk_bin(sk_hmin_of_kmer(key, k)) : 0;
            const uint64_t home = sk_home(key);
            uint64_t at[NT];
            uint4 raw[NT];
#pragma unroll
            for (int t = 0; t < NT; t++)
                at[t] = MODE != KEY_PACKED              ? mix >> tv.t[t].shift
                        : !(bins >> t & 1)              ? mix >> s_rare[t].shift  // (packed keys: the minimizer's constants want the scalar registers)
                                                        : (((bin * s_rare[t].n_regions) >> 32) << MC_REGION_LG) | home;
#pragma unroll
            for (int t = 0; t < NT; t++) raw[t] = *reinterpret_cast<const uint4 *>(tv.t[t].slots + at[t]);
            uint32_t behind = 0;  // the tables whose home slot holds another key
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const uint64_t cur = ((uint64_t)raw[t].y << 32) | raw[t].x;
                uint32_t c = 0;
                if (cur == key && (MODE == KEY_PACKED || key != EMPTY_KEY)) c = raw[t].z > 32767u ? 32767u : raw[t].z;
                else if (cur != EMPTY_KEY || (MODE != KEY_PACKED && key == EMPTY_KEY)) behind |= 1u << t;  // (or the key is the free slot's mark)
                acc[t] += c;
                acc[NT + t] += c > 0;
            }
            if (behind) {
#pragma unroll 1
                for (int t = 0; t < NT; t++) {
                    if (!(behind >> t & 1)) continue;
                    const SeqCovRare r = s_rare[t];
                    uint64_t s_home = at[0];  // (registers cannot be indexed: t is the same in every lane, so these are scalar selects)
#pragma unroll
                    for (int u = 1; u < NT; u++)
                        if (t == u) s_home = at[u];
                    uint32_t c;
                    if (MODE != KEY_PACKED && key == EMPTY_KEY) {  // (table_get: such a hash is counted beside the table)
                        const unsigned long long e = *r.empty_cnt;
                        c = e > 32767ull ? 32767u : (uint32_t)e;
                    } else {
                        c = cov_behind_home(r.slots, r.rmask, r.n_regions, key, s_home);
                    }
#pragma unroll
                    for (int u = 0; u < NT; u++)
                        if (t == u) { acc[u] += c; acc[NT + u] += c > 0; }
                }
            }
        }
    }
    // the lanes' last runs: sequence numbers do not decrease along the wave, so a segmented scan sums every run of equal ones
    // into its last lane.  (A run without an entry in LDS, whose number may not fit 32 bits either, goes straight to d_out and
    // leaves zeros; the lanes behind the tile's end carry zeros under a number of their own.)
    if (s - s0 >= SC_SEGS) flush(s);
    const uint32_t seg = active ? (uint32_t)min(s - s0, (uint64_t)SC_SEGS) : 0xFFFFFFFFu;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t oseg = __shfl_up(seg, o);
        const bool take = lane >= (uint32_t)o && oseg == seg;
#pragma unroll
        for (int i = 0; i < 2 * NT; i++) {
            const uint32_t v = __shfl_up(acc[i], o);
            if (take) acc[i] += v;
        }
    }
    const uint32_t nseg = __shfl_down(seg, 1);
    if (lane == 63 || nseg != seg) flush(s);
    __syncthreads();
    for (uint32_t i = tid; i < SC_SEGS * 2 * NT; i += SC_THREADS) {
        const uint32_t j = i / (2 * NT), f = i % (2 * NT);
        const uint32_t v = s_acc[j][f];
        if (v) atomicAdd(&out64[((s0 + j) * NT + (f % NT)) * 2 + f / NT], (unsigned long long)v);
    }
}

struct SeqCovCall {
    hipStream_t stream;
    mc_ctx *const *tables;
    const uint64_t *d_words, *d_offsets;
    uint64_t n_seqs, first, end_all;  // the store's positions: seq_offsets[0] .. seq_offsets[n_seqs]
    mc_seq_cov *d_out;
};

template <int MODE, int NT>
void launch_seq_cov(const SeqCovCall &a)
{
    SeqCovTables<NT> tv;
    for (int t = 0; t < NT; t++) tv.t[t] = a.tables[t]->view();
    const uint64_t n_tiles = (a.end_all - a.first + SC_TILE - 1) / SC_TILE;
    hipLaunchKernelGGL((k_seq_cov<MODE, NT>), dim3((uint32_t)n_tiles), dim3(SC_THREADS), 0, a.stream, a.d_words, a.d_offsets, a.n_seqs, a.first,
                       a.end_all, a.tables[0]->cfg.k, tv, a.d_out);
}

template <int MODE>
void launch_seq_cov_n(uint32_t n_tables, const SeqCovCall &a)
{
    switch (n_tables) {
    case 1: launch_seq_cov<MODE, 1>(a); break;
    case 2: launch_seq_cov<MODE, 2>(a); break;
    case 3: launch_seq_cov<MODE, 3>(a); break;
    default: launch_seq_cov<MODE, 4>(a); break;
    }
}

// null contexts, their number, and what they must share; the message goes to tables[0] when there is one
int check_tables(mc_ctx *const *tables, uint32_t n_tables)
{
    if (!tables || n_tables == 0 || n_tables > MC_SEQ_COV_MAX_TABLES) {
        mc_ctx *c0 = tables && n_tables ? tables[0] : nullptr;
        if (c0) {
            std::lock_guard<std::mutex> g(c0->mu);
            return fail(c0, MC_EINVAL, "mc_seq_coverage: %u tables (1 .. %d)", n_tables, MC_SEQ_COV_MAX_TABLES);
        }
        return MC_EINVAL;
    }
    if (!tables[0]) return MC_EINVAL;
    for (uint32_t t = 1; t < n_tables; t++)
        if (!tables[t]) {
            std::lock_guard<std::mutex> g(tables[0]->mu);
            return fail(tables[0], MC_EINVAL, "mc_seq_coverage: table %u is null", t);
        }
    return MC_OK;
}

}  // namespace

int mc_seq_coverage_dev(mc_ctx *const *tables, uint32_t n_tables, const uint64_t *d_words, const uint64_t *d_seq_offsets, uint64_t n_seqs,
                        mc_seq_cov *d_out)
{
    if (int rc = check_tables(tables, n_tables)) return rc;
    mc_ctx *c = tables[0];
    TablesLock lock(tables, n_tables);
    for (uint32_t t = 1; t < n_tables; t++)
        if (tables[t]->cfg.k != c->cfg.k || tables[t]->cfg.key_mode != c->cfg.key_mode || tables[t]->cfg.device != c->cfg.device)
            return fail(c, MC_EINVAL, "mc_seq_coverage: table %u has k = %d, key mode %d, device %d; table 0 has %d, %d, %d", t, tables[t]->cfg.k,
                        tables[t]->cfg.key_mode, tables[t]->cfg.device, c->cfg.k, c->cfg.key_mode, c->cfg.device);
    for (uint32_t t = 0; t < n_tables; t++)
        if (!tables[t]->finalized) return fail(c, MC_ESTATE, "mc_seq_coverage: call mc_finalize_counts on table %u first", t);
    if (n_seqs && (!d_words || !d_seq_offsets || !d_out)) return fail(c, MC_EINVAL, "mc_seq_coverage: null pointer");
    if (n_seqs == 0) return MC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    for (mc_ctx *x : lock.distinct) {
        // (hash keys in minimizer bins: the table moves to hash-prefix regions, once; an empty table that was never written is filled)
        int rc = by_key_ready(x);
        if (!rc) rc = materialize(x);
        if (rc) return x == c ? rc : fail(c, rc, "mc_seq_coverage: %s", x->err.c_str());
        if (x != c) HIPCHK(c, hipStreamSynchronize(x->stream));  // (its own stream did that; the kernel runs on table 0's)
    }
    // the store's first and last position size the grid (two words through the pinned scratch, as read_counters copies)
    unsigned long long *h = c->h_scratch;
    HIPCHK(c, hipMemcpyAsync(h, d_seq_offsets, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h + 1, d_seq_offsets + n_seqs, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const SeqCovCall a{c->stream, tables, d_words, d_seq_offsets, n_seqs, h[0], h[1], d_out};
    if (a.end_all < a.first || (a.end_all - a.first) / SC_TILE >= (1ull << 31))
        return fail(c, MC_EINVAL, "mc_seq_coverage: seq_offsets run from %llu to %llu", h[0], h[1]);
    HIPCHK(c, hipMemsetAsync(d_out, 0, n_seqs * n_tables * sizeof(mc_seq_cov), c->stream));
    if (a.end_all == a.first) return hipStreamSynchronize(c->stream) == hipSuccess ? MC_OK : fail(c, MC_EHIP, "mc_seq_coverage: the stream failed");  // (no bases: every number is 0)
    if (c->cfg.key_mode == MC_KEY_PACKED) launch_seq_cov_n<KEY_PACKED>(n_tables, a);
    else if (c->cfg.key_mode == MC_KEY_POLY) launch_seq_cov_n<KEY_POLY>(n_tables, a);
    else launch_seq_cov_n<KEY_FNV1A>(n_tables, a);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MC_OK;
}

int mc_seq_coverage(mc_ctx *const *tables, uint32_t n_tables, const uint64_t *words, const uint64_t *seq_offsets, uint64_t n_seqs, mc_seq_cov *out)
{
    if (int rc = check_tables(tables, n_tables)) return rc;
    mc_ctx *c = tables[0];
    if (n_seqs == 0 || !words || !seq_offsets || !out)  // (nothing to copy: the device form checks the rest and says what is wrong)
        return mc_seq_coverage_dev(tables, n_tables, nullptr, nullptr, n_seqs, nullptr);
    const uint64_t n_words = (seq_offsets[n_seqs] + 31) / 32 + 1;
    DevBuf<uint64_t> dw, doff;
    DevBuf<mc_seq_cov> dout;
    {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(c, hipSetDevice(c->cfg.device));
        HIPCHK(c, dw.alloc(n_words));
        HIPCHK(c, doff.alloc(n_seqs + 1));
        HIPCHK(c, dout.alloc(n_seqs * n_tables));
        HIPCHK(c, hipMemcpy(dw.p, words, n_words * 8, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(doff.p, seq_offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice));
    }
    int rc = mc_seq_coverage_dev(tables, n_tables, dw.p, doff.p, n_seqs, dout.p);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipMemcpy(out, dout.p, n_seqs * n_tables * sizeof(mc_seq_cov), hipMemcpyDeviceToHost));
    return MC_OK;
}
