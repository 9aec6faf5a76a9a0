// libmcgpu.so, the seq-cov unit: depth and breadth of every sequence's k-mers in up to four tables at once (include/mcgpu.h
// mc_seq_coverage*; src/tools/SequenceCoverage.java:162-185).  context.h lists the other units.
//
// The work is cut by base positions of the flattened store, not by sequences: a workgroup takes a tile of SC_TILE positions, each
// thread SC_ITEMS of them in a row, so a 5 Mbase contig and five million 1-base sequences both spread over the whole device.  One
// wave finds the sequence of the tile's first position by a 64-ary search in seq_offsets; a thread gallops from there to its own
// and then walks the boundaries.  A window is extracted and keyed once; its home slots in all NT tables are loaded before any
// of them is looked at (multi_table.h home_slots, shared with presence.hip; NT independent 16-byte reads at random places are in flight a lane, where k_classify has one), and only
// a window whose home slot holds another key goes on probing.  DESIGN.md "seq-cov" has the roofline.
//
// Sums: a thread adds what its windows of one sequence found in 32 bits (SC_ITEMS x 32767), a wave adds its lanes' runs of one
// sequence with a segmented scan (sequence numbers do not decrease along the lanes), the last lane of a run adds it to the
// tile's entry of that sequence in LDS (still 32 bits: SC_TILE x 32767 < 2^32, asserted below), and the tile gives every
// (sequence, table) it covered one 64-bit atomic add a number into d_out.  Integer adds: the same bits in any order.
#include "multi_table.h"

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

// a table's shift and n_regions for home_slots: hash keys read the shift from the kernel's arguments, packed keys both from LDS (the
// minimizer's constants want the scalar registers)
template <int MODE, int NT>
struct RareOf {
    const Tables<NT> &tv;
    const SeqCovRare *rare;
    __device__ __forceinline__ uint32_t shift(int t) const { return MODE != KEY_PACKED ? tv.t[t].shift : rare[t].shift; }
    __device__ __forceinline__ uint32_t n_regions(int t) const { return rare[t].n_regions; }
};

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
                                                                      uint64_t n_seqs, uint64_t first, uint64_t end_all, int k, Tables<NT> tv,
                                                                      mc_seq_cov *__restrict__ out)
{
    __shared__ uint32_t s_acc[SC_SEGS][2 * NT];  // depth of table 0 .. NT-1, then breadth
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    unsigned long long *const out64 = reinterpret_cast<unsigned long long *>(out);  // (seq, table): depth, breadth
    // What only the rare paths need of a table waits in LDS, read by the table's number: the kernel arguments would hold four scalar
    // registers a table for the whole kernel (and indexing them would put them in scratch).
    __shared__ SeqCovRare s_rare[NT];
    const uint32_t bins = bin_tables<MODE>(tv);
#pragma unroll
    for (int t = 0; t < NT; t++) {
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
            uint64_t at[NT];
    const uint32_t behind = home_slots<MODE>(tv, bins, key, k, RareOf<MODE, NT>{tv, s_rare}, at, [&](int t, bool there, uint32_t count) {
                const uint32_t c = !there ? 0 : count > 32767u ? 32767u : count;
                acc[t] += c;
                acc[NT + t] += c > 0;
            });
            if (behind) {
#pragma unroll 1
                for (int t = 0; t < NT; t++) {
                    if (!(behind >> t & 1)) continue;
                    const SeqCovRare r = s_rare[t];
                    uint64_t s_home = at[0];  // (registers cannot be indexed: t is the same in every lane, so these are scalar selects)
#pragma unroll
                    for (int u = 1; u < NT; u++)
                        if (t == u) s_home = at[u];
                    const uint32_t c = (uint32_t)max(get_behind_home<MODE, true>(r.slots, r.empty_cnt, r.rmask, r.n_regions, key, s_home), 0);
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

constexpr char API[] = "mc_seq_coverage";

}  // namespace

int mc_seq_coverage_dev(mc_ctx *const *tables, uint32_t n_tables, const uint64_t *d_words, const uint64_t *d_seq_offsets, uint64_t n_seqs,
                        mc_seq_cov *d_out)
{
    if (int rc = check_tables(API, MC_SEQ_COV_MAX_TABLES, tables, n_tables)) return rc;
    mc_ctx *c = tables[0];
    TablesLock lock(tables, n_tables);
    if (int rc = tables_agree(API, tables, n_tables)) return rc;
    if (n_seqs && (!d_words || !d_seq_offsets || !d_out)) return fail(c, MC_EINVAL, "%s: null pointer", API);
    if (n_seqs == 0) return MC_OK;
    if (int rc = prepare_tables(API, c, lock)) return rc;
    // the store's first and last position size the grid (two words through the pinned scratch, as read_counters copies)
    unsigned long long *h = c->h_scratch;
    HIPCHK(c, hipMemcpyAsync(h, d_seq_offsets, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h + 1, d_seq_offsets + n_seqs, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t first = h[0], end_all = h[1];  // the store's positions: seq_offsets[0] .. seq_offsets[n_seqs]
    if (end_all < first || (end_all - first) / SC_TILE >= (1ull << 31))
        return fail(c, MC_EINVAL, "%s: seq_offsets run from %llu to %llu", API, h[0], h[1]);
    HIPCHK(c, hipMemsetAsync(d_out, 0, n_seqs * n_tables * sizeof(mc_seq_cov), c->stream));
    if (end_all == first) return hipStreamSynchronize(c->stream) == hipSuccess ? MC_OK : fail(c, MC_EHIP, "%s: the stream failed", API);  // (no bases: every number is 0)
    const uint64_t n_tiles = (end_all - first + SC_TILE - 1) / SC_TILE;
    for_key_mode_and_tables(c->cfg.key_mode, n_tables, [&](auto mode, auto nt) {
        hipLaunchKernelGGL((k_seq_cov<mode(), nt()>), dim3((uint32_t)n_tiles), dim3(SC_THREADS), 0, c->stream, d_words, d_seq_offsets, n_seqs, first, end_all,
                           c->cfg.k, tables_view<nt()>(tables), d_out);
    });
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MC_OK;
}

int mc_seq_coverage(mc_ctx *const *tables, uint32_t n_tables, const uint64_t *words, const uint64_t *seq_offsets, uint64_t n_seqs, mc_seq_cov *out)
{
    if (int rc = check_tables(API, MC_SEQ_COV_MAX_TABLES, tables, n_tables)) return rc;
    mc_ctx *c = tables[0];
    if (n_seqs == 0 || !words || !seq_offsets || !out)  // (nothing to copy: the device form checks the rest and says what is wrong)
        return mc_seq_coverage_dev(tables, n_tables, nullptr, nullptr, n_seqs, nullptr);
    HostStage st(c);
    const uint64_t *dw = st.in(words, packed_words(seq_offsets, n_seqs)), *doff = st.in(seq_offsets, n_seqs + 1);
    mc_seq_cov *dout = st.out<mc_seq_cov>(n_seqs * n_tables);
    if (int rc = st.staged()) return rc;
    if (int rc = mc_seq_coverage_dev(tables, n_tables, dw, doff, n_seqs, dout)) return rc;
    return st.back(out, dout, n_seqs * n_tables);
}
