// libmcgpu.so, the reads-in-set unit: how many windows of every read are members of a small exact set of k-mers, and which reads
// that keeps (include/mcgpu.h mc_reads_in_set*; src/algo/ReadsFilter.java:47-68 over OneSequenceCalculator.java:150-152).
// context.h lists the other units.
//
// The set is a few hundred thousand k-mers out of the hundreds of millions in the reads: almost every window misses.  Two kernels
// and a small one:
//   k_rs_build   one thread a k-mer of the set: its canonical form (the smaller of the k-mer and its reverse complement as 2k-bit
//                numbers) goes into an open-addressing table in device memory -- one word a slot for k <= 32, two words above --
//                and sets three bits of one 64-bit word of a bit filter.  The table is at most half full.
//   k_rs_count   the work is cut by base positions of the flattened reads, as seq_cov.hip cuts it: a workgroup takes tiles of
//                RS_TILE positions, a thread RS_ITEMS of them in a row, and rolls the forward and the reverse k-mer along them one
//                base a step (the store is contiguous across reads: a window that straddles two reads is rolled through and not
//                counted).  The workgroup keeps the whole filter in LDS: a window whose three bits are not all set is no member
//                and costs one 8-byte LDS read.  A window that passes is looked up in the table, compared in full: the result
//                never rests on the filter.  Hits are rare, so a thread adds its count of a read to hits[] with one atomic add
//                when it leaves the read.
//   k_rs_keep    one thread a read: ReadsFilter's threshold.
// Without the filter (FILTER = false: MC_READS_IN_SET_WEAK_FILTER, or a set so large that the filter would pass most windows)
// every window goes to the table.  DESIGN.md "reads-in-set" has the sizes and the registers,
// tests/test_reads_in_set_kernel_resources.py holds the kernels to them.
#include "context.h"
#include "kmer_set.h"  // RsKey, rs_key, rs_hash, rs_home: shared with unitigs.hip

namespace {

constexpr int RS_THREADS = 1024;                  // one workgroup a CU: the filter takes most of its LDS
constexpr int RS_ITEMS = 32;                      // positions a thread
constexpr int RS_TILE = RS_THREADS * RS_ITEMS;    // positions a workgroup takes at a time
constexpr int RS_FILTER_WORDS_LG = 14;            // 2^14 words of 64 bits: 128 KB of a CU's 160 KB
constexpr int RS_FILTER_WORDS = 1 << RS_FILTER_WORDS_LG;
constexpr uint64_t RS_FILTER_MAX_SET = 1ull << 19;  // more k-mers than this: over a third of the windows would pass, no filter
constexpr int RS_BUILD_THREADS = 256;

__device__ __forceinline__ uint64_t rs_filter_bits(uint32_t h) { return (1ull << (h & 63)) | (1ull << ((h >> 6) & 63)) | (1ull << ((h >> 12) & 63)); }
__device__ __forceinline__ uint32_t rs_filter_word(uint32_t h) { return h >> (32 - RS_FILTER_WORDS_LG); }

// table: 2^lg_cap slots of one word (k <= 32) or two (above), all ones when the call starts; filter: RS_FILTER_WORDS words, zero
template <bool WIDE>
__global__ void __launch_bounds__(RS_BUILD_THREADS) k_rs_build(const uint64_t *__restrict__ set_hi, const uint64_t *__restrict__ set_lo, uint64_t n_set,
                                                               int k, unsigned long long *__restrict__ table, int lg_cap,
                                                               unsigned long long *__restrict__ filter)
{
    const uint64_t i = (uint64_t)blockIdx.x * RS_BUILD_THREADS + threadIdx.x;
    if (i >= n_set) return;
    Kmer v{WIDE ? set_hi[i] : 0, set_lo[i]};
    if (WIDE) v.hi &= ~0ull >> (128 - 2 * k);  // (bits above the k-mer are not the caller's to set: dropped)
    else if (k < 32) v.lo &= ~0ull >> (64 - 2 * k);
    const Kmer r = rc_kmer(v, k);
    const RsKey key = rs_key<WIDE>(v.hi, v.lo, r.hi, r.lo);
    const uint32_t h = rs_hash<WIDE>(key);
    if (filter) atomicOr(&filter[rs_filter_word(h)], (unsigned long long)rs_filter_bits(h));
    const uint64_t mask = (1ull << lg_cap) - 1;
    uint64_t s = rs_home(h, lg_cap);
    for (uint64_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {  // (at most half full: a free slot comes)
        unsigned long long *slot = table + (WIDE ? 2 * s : s);
        const unsigned long long was = atomicCAS(slot, (unsigned long long)RS_EMPTY, (unsigned long long)key.a);
        if (was != RS_EMPTY && was != key.a) continue;
        if (!WIDE) return;
        // the first word is this key's, written by this thread or by one with the same first word: whoever writes the second word
        // first has the slot, the other moves on.  Every thread that sets a first word goes straight on to the second, so no slot
        // is left half written when the kernel ends.
        const unsigned long long was_b = atomicCAS(slot + 1, (unsigned long long)RS_EMPTY, (unsigned long long)key.b);
        if (was_b == RS_EMPTY || was_b == key.b) return;
    }
}

template <bool WIDE>
__device__ __forceinline__ bool rs_in_table(const uint64_t *__restrict__ table, int lg_cap, const RsKey &key, uint32_t h)
{
    const uint64_t mask = (1ull << lg_cap) - 1;
    uint64_t s = rs_home(h, lg_cap);
    for (uint64_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {
        if (WIDE) {
            const ulonglong2 cur = *reinterpret_cast<const ulonglong2 *>(table + 2 * s);
            if (cur.x == key.a && cur.y == key.b) return true;
            if (cur.x == RS_EMPTY) return false;
        } else {
            const uint64_t cur = table[s];
            if (cur == key.a) return true;
            if (cur == RS_EMPTY) return false;
        }
    }
    return false;
}

// the greatest s in [lo, hi) with offsets[s] <= p, given offsets[lo] <= p < offsets[hi]; the whole wave calls it with the same
// arguments and looks at 64 places a round (as seq_cov.hip finds a tile's first sequence)
__device__ __forceinline__ uint64_t rs_wave_find_read(const uint64_t *__restrict__ offsets, uint64_t lo, uint64_t hi, uint64_t p, uint32_t lane)
{
    while (hi - lo > 1) {
        const uint64_t step = (hi - lo + 63) / 64;
        const uint64_t at = lo + (lane + 1) * step;
        const bool le = at < hi && offsets[at] <= p;
        const uint64_t c = (uint64_t)__popcll(__ballot(le));
        const uint64_t nlo = lo + c * step;
        hi = min(hi, nlo + step);
        lo = nlo;
    }
    return lo;
}

template <bool WIDE, bool FILTER>
__global__ void __launch_bounds__(RS_THREADS) k_rs_count(const uint64_t *__restrict__ words, const uint64_t *__restrict__ offsets, uint64_t n_reads,
                                                         uint64_t first, uint64_t end_all, uint64_t n_tiles, int k,
                                                         const uint64_t *__restrict__ table, int lg_cap, const uint64_t *__restrict__ filter,
                                                         uint32_t *__restrict__ hits)
{
    __shared__ uint64_t s_filter[FILTER ? RS_FILTER_WORDS : 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    if (FILTER) {
        for (uint32_t i = tid; i < RS_FILTER_WORDS / 2; i += RS_THREADS)
            reinterpret_cast<ulonglong2 *>(s_filter)[i] = reinterpret_cast<const ulonglong2 *>(filter)[i];
        __syncthreads();
    }
    const uint64_t kmask_lo = k >= 32 ? ~0ull : ~0ull >> (64 - 2 * k);          // the low word's bits of a k-mer
    const uint64_t kmask_hi = WIDE ? ~0ull >> (128 - 2 * k) : 0;                // k = 33 .. 63
    const int top = WIDE ? 2 * (k - 33) : 2 * (k - 1);                          // where the reverse k-mer takes a new base (hi or lo)

    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t p0 = first + tile * RS_TILE;
        const uint64_t p_end = min(p0 + RS_TILE, end_all);
        const uint64_t s0 = rs_wave_find_read(offsets, 0, n_reads, p0, lane);
        const uint64_t pt = p0 + (uint64_t)tid * RS_ITEMS;
        if (pt >= p_end || pt + k >= end_all) continue;  // (no window from pt on has a base behind it: none is tested)
        // this thread's read: gallop from the tile's, then bisect
        uint64_t s = s0, step = 1;
        while (s + step < n_reads && offsets[s + step] <= pt) { s += step; step <<= 1; }
        uint64_t hi = min(s + step, n_reads);
        while (hi - s > 1) {
            const uint64_t mid = s + (hi - s) / 2;
            if (offsets[mid] <= pt) s = mid; else hi = mid;
        }
        uint64_t read_end = offsets[s + 1];
        Kmer fw = extract_kmer(words, pt, k);  // (pt + k < end_all: all its words hold bases)
        Kmer rc = rc_kmer(fw, k);
        uint64_t w = words[(pt + k) >> 5];     // the word of the next base to come in
        uint32_t cnt = 0;
#pragma unroll 1
        for (int it = 0; it < RS_ITEMS; it++) {
            const uint64_t p = pt + it;
            if (p >= p_end) break;
            if (p >= read_end) {
                if (cnt) atomicAdd(&hits[s], cnt);
                cnt = 0;
                do read_end = offsets[++s + 1]; while (p >= read_end);  // (empty reads in between; p < offsets[n_reads])
            }
            // ReadsFilter.java:54: windows 0 .. L - k - 1 of a read, the last one never
            if (p + k < read_end) {
                const RsKey key = rs_key<WIDE>(fw.hi, fw.lo, rc.hi, rc.lo);
                const uint32_t h = rs_hash<WIDE>(key);
                bool maybe = true;
                if (FILTER) {
                    const uint64_t bits = rs_filter_bits(h);
                    maybe = (s_filter[rs_filter_word(h)] & bits) == bits;
                }
                if (maybe && rs_in_table<WIDE>(table, lg_cap, key, h)) cnt++;
            }
            // on to p + 1: base p + k comes in
            const uint64_t q = p + k;
            if (q >= end_all) break;  // (no base there, and no later window is tested)
            if ((q & 31) == 0) w = words[q >> 5];
            const uint64_t b = (w >> (62 - 2 * (q & 31))) & 3;
            if (WIDE) {
                fw.hi = ((fw.hi << 2) | (fw.lo >> 62)) & kmask_hi;
                fw.lo = (fw.lo << 2) | b;
                rc.lo = (rc.lo >> 2) | (rc.hi << 62);
                rc.hi = (rc.hi >> 2) | ((3 - b) << top);
            } else {
                fw.lo = ((fw.lo << 2) | b) & kmask_lo;
                rc.lo = (rc.lo >> 2) | ((3 - b) << top);
            }
        }
        if (cnt) atomicAdd(&hits[s], cnt);
    }
}

// ReadsFilter.java:50-52,58 in Java's int arithmetic: the product wraps, the division truncates
__global__ void __launch_bounds__(RS_BUILD_THREADS) k_rs_keep(const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ hits, uint64_t n_reads,
                                                              int k, int pct, uint8_t *__restrict__ keep)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        const int32_t len = (int32_t)(offsets[r + 1] - offsets[r]);
        const int32_t prod = (int32_t)((uint32_t)(len - k + 1) * (uint32_t)pct);
        const int32_t thr = max(1, prod / 100);
        keep[r] = len > k && (int64_t)hits[r] >= (int64_t)thr ? 1 : 0;
    }
}

constexpr char API[] = "mc_reads_in_set";

int check_args(mc_ctx *c, bool reads_ok, bool set_ok, uint64_t n_reads, uint64_t n_set, int pct)
{
    if (pct < 0 || pct > 100) return fail(c, MC_EINVAL, "%s: pct %d is outside 0 .. 100", API, pct);
    if (n_set >= (1ull << 31)) return fail(c, MC_EINVAL, "%s: %llu k-mers in the set (at most 2^31 - 1)", API, (unsigned long long)n_set);
    if ((n_reads && !reads_ok) || (n_reads && n_set && !set_ok)) return fail(c, MC_EINVAL, "%s: null pointer", API);
    return MC_OK;
}

}  // namespace

int mc_reads_in_set_dev(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_read_offsets, uint64_t n_reads, const uint64_t *d_set_hi,
                        const uint64_t *d_set_lo, uint64_t n_set, int pct, int flags, uint32_t *d_hits, uint8_t *d_keep)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    const int k = c->cfg.k;
    const bool wide = k > 32;
    if (int rc = check_args(c, d_words && d_read_offsets && d_hits && d_keep, d_set_lo && (d_set_hi || !wide), n_reads, n_set, pct)) return rc;
    if (n_reads == 0) return MC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // the store's first and last position size the grid (two words through the pinned scratch, as mc_seq_coverage copies them)
    unsigned long long *h = c->h_scratch;
    HIPCHK(c, hipMemcpyAsync(h, d_read_offsets, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h + 1, d_read_offsets + n_reads, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t first = h[0], end_all = h[1];
    if (end_all < first) return fail(c, MC_EINVAL, "%s: read_offsets run from %llu to %llu", API, h[0], h[1]);
    HIPCHK(c, hipMemsetAsync(d_hits, 0, n_reads * sizeof(uint32_t), c->stream));
    if (n_set == 0 || end_all == first) {  // (no member, or no base: every number is 0)
        HIPCHK(c, hipMemsetAsync(d_keep, 0, n_reads, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return MC_OK;
    }
    int lg_cap = 6;
    while ((1ull << lg_cap) < 2 * n_set) lg_cap++;  // (at most 32: n_set < 2^31)
    const uint64_t table_words = (1ull << lg_cap) * (wide ? 2 : 1);
    const bool use_filter = !(flags & MC_READS_IN_SET_WEAK_FILTER) && n_set <= RS_FILTER_MAX_SET;
    DevBuf<unsigned long long> table, filter;
    HIPCHK(c, table.alloc(table_words));
    HIPCHK(c, hipMemsetAsync(table.p, 0xff, table_words * 8, c->stream));
    if (use_filter) {
        HIPCHK(c, filter.alloc(RS_FILTER_WORDS));
        HIPCHK(c, hipMemsetAsync(filter.p, 0, RS_FILTER_WORDS * 8, c->stream));
    }
    const dim3 build_grid((uint32_t)((n_set + RS_BUILD_THREADS - 1) / RS_BUILD_THREADS));
    if (wide) hipLaunchKernelGGL(k_rs_build<true>, build_grid, dim3(RS_BUILD_THREADS), 0, c->stream, d_set_hi, d_set_lo, n_set, k, table.p, lg_cap, filter.p);
    else hipLaunchKernelGGL(k_rs_build<false>, build_grid, dim3(RS_BUILD_THREADS), 0, c->stream, d_set_hi, d_set_lo, n_set, k, table.p, lg_cap, filter.p);
    HIPCHK(c, hipGetLastError());
    const uint64_t n_tiles = (end_all - first + RS_TILE - 1) / RS_TILE;
    const dim3 grid(grid_for(n_tiles, 1, 512)), block(RS_THREADS);
    const uint64_t *tab = reinterpret_cast<const uint64_t *>(table.p), *fil = reinterpret_cast<const uint64_t *>(filter.p);
    auto launch = [&](auto w, auto f) {
        hipLaunchKernelGGL((k_rs_count<w(), f()>), grid, block, 0, c->stream, d_words, d_read_offsets, n_reads, first, end_all, n_tiles, k, tab, lg_cap, fil,
                           d_hits);
    };
    using T = std::true_type;
    using F = std::false_type;
    if (wide) { if (use_filter) launch(T(), T()); else launch(T(), F()); }
    else { if (use_filter) launch(F(), T()); else launch(F(), F()); }
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_rs_keep, dim3(grid_for(n_reads, RS_BUILD_THREADS, 1 << 16)), dim3(RS_BUILD_THREADS), 0, c->stream, d_read_offsets, d_hits, n_reads, k,
                       pct, d_keep);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MC_OK;
}

int mc_reads_in_set(mc_ctx *c, const uint64_t *words, const uint64_t *read_offsets, uint64_t n_reads, const uint64_t *set_hi, const uint64_t *set_lo,
                    uint64_t n_set, int pct, int flags, uint32_t *hits, uint8_t *keep)
{
    if (!c) return MC_EINVAL;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (int rc = check_args(c, words && read_offsets && hits && keep, set_lo && (set_hi || c->cfg.k <= 32), n_reads, n_set, pct)) return rc;
    }
    if (n_reads == 0) return MC_OK;
    HostStage st(c);
    const uint64_t *dw = st.in(words, packed_words(read_offsets, n_reads)), *doff = st.in(read_offsets, n_reads + 1);
    const uint64_t *dhi = c->cfg.k > 32 ? st.in(set_hi, n_set) : nullptr, *dlo = st.in(set_lo, n_set);
    uint32_t *dhits = st.out<uint32_t>(n_reads);
    uint8_t *dkeep = st.out<uint8_t>(n_reads);
    if (int rc = st.staged()) return rc;
    if (int rc = mc_reads_in_set_dev(c, dw, doff, n_reads, dhi, dlo, n_set, pct, flags, dhits, dkeep)) return rc;
    if (int rc = st.back(hits, dhits, n_reads)) return rc;
    return st.back(keep, dkeep, n_reads);
}
