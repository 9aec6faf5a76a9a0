// libmcgpu.so, the components unit: which k-mers of a table hang together (include/mcgpu.h mc_components*; the walks of
// src/tools/FMTVisualizer.java:113-139 through src/algo/KmerEnvCalculator.java, which reach exactly the connected component of their
// first k-mer and zero it).  context.h lists the other units.
//
// A vertex is a table slot whose key has a count above 0 and that some window of the given sequences holds; the hash key that is
// counted beside the table (the one that equals the free slot's mark) is the vertex behind the last slot.  Passes:
//   k_cc_first    a thread eight base positions in a row, the work cut by positions as seq_cov.hip cuts it: every window is keyed and
//                 located, and first[slot] becomes the smallest position of a window that holds the slot's key -- the slot's
//                 representative k-mer (a hash key has no bases of its own) and its first occurrence in scan order, in one word.
//   k_cc_union    a thread a claimed slot: the k-mer at first[slot] is rebuilt from the sequence words, its eight neighbours
//                 (StringUtils.allNeighbors) are located, and the two slots are united: find with path halving, the root with the
//                 greater index hooked under the smaller by compare-and-swap.  parent[x] <= x always, so no cycle can form, and a
//                 word that is read late still names an ancestor.  Every access to parent[] is an agent-scope atomic: a CU's L1 is
//                 not refreshed by other CUs' stores, and a root test on a stale line would retry its compare-and-swap for ever.
//   k_cc_flatten  parent[slot] = root; members and roots are counted.
//   k_cc_members, k_cc_rootmin, k_cc_roots   the claimed slots as a list (slot, first position); first[root] becomes the smallest
//                 position of the component; the roots with it.  The host sorts the roots by that position: the component numbers.
//   k_cc_number, k_cc_hist, k_cc_scatter     first[root] = number; members a component; every member to its place, the one whose
//                 window is the component's first to place 0.  Lanes of a wave that add to one counter share one atomic: one
//                 giant component is the usual case.
// Limit (hash keys): the first-seen k-mer of a key explores for it, include/mcgpu.h says what that means.
#include "context.h"

namespace {

constexpr int CC_THREADS = 256;
constexpr int CC_ITEMS = 8;                     // positions a thread
constexpr int CC_TILE = CC_THREADS * CC_ITEMS;  // positions a workgroup
constexpr unsigned long long CC_NONE = TABLE_NOWHERE;

// the greatest s in [lo, hi) with offsets[s] <= p, given offsets[lo] <= p < offsets[hi]; the whole wave calls it with the same
// arguments and looks at 64 places a round (as seq_cov.hip's)
__device__ __forceinline__ uint64_t cc_wave_find_seq(const uint64_t *__restrict__ offsets, uint64_t lo, uint64_t hi, uint64_t p, uint32_t lane)
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

template <int MODE>
__global__ void __launch_bounds__(CC_THREADS) k_cc_first(const uint64_t *__restrict__ words, const uint64_t *__restrict__ offsets, uint64_t n_seqs,
                                                         uint64_t first_pos, uint64_t end_all, int k, TableView t, unsigned long long n_slots,
                                                         unsigned long long *__restrict__ first)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint64_t p0 = first_pos + (uint64_t)blockIdx.x * CC_TILE;
    const uint64_t p_end = min(p0 + CC_TILE, end_all);
    uint64_t s = cc_wave_find_seq(offsets, 0, n_seqs, p0, lane);
    const uint64_t pt = p0 + (uint64_t)tid * CC_ITEMS;
    if (pt >= p_end) return;
    uint64_t step = 1;  // this thread's sequence: gallop from the tile's, then bisect
    while (s + step < n_seqs && offsets[s + step] <= pt) { s += step; step <<= 1; }
    uint64_t hi = min(s + step, n_seqs);
    while (hi - s > 1) {
        const uint64_t mid = s + (hi - s) / 2;
        if (offsets[mid] <= pt) s = mid; else hi = mid;
    }
    uint64_t seq_end = offsets[s + 1];
#pragma unroll 1
    for (int it = 0; it < CC_ITEMS; it++) {
        const uint64_t p = pt + it;
        if (p >= p_end) break;
        while (p >= seq_end) seq_end = offsets[++s + 1];  // (empty sequences in between; p < offsets[n_seqs])
        if (p + k > seq_end) continue;                     // no window starts here
        const uint64_t key = (uint64_t)key_of<MODE>(extract_kmer(words, p, k), k);
        uint32_t count;
        const unsigned long long at = table_locate<MODE>(t, key, n_slots, &count);
        if (at == CC_NONE) continue;
        // (a plain read first: the windows of a repeated k-mer do not all pay for an atomic.  A stale value is too great, never too small.)
        if (first[at] > p) atomicMin(&first[at], (unsigned long long)p);
    }
}

template <class I>
__device__ __forceinline__ I cc_load(const I *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class I>
__device__ __forceinline__ void cc_store(I *p, I v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x, halving the path on the way (a non-root never becomes a root again, so these stores never meet a hooking)
template <class I>
__device__ __forceinline__ I cc_find(I *parent, I x)
{
    I p = cc_load(parent + x);
    while (p != x) {
        const I g = cc_load(parent + p);
        if (g != p) cc_store(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

template <class I>
__device__ __forceinline__ void cc_unite(I *parent, I a, I b)
{
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a > b) { const I x = a; a = b; b = x; }
        if (atomicCAS(parent + b, b, a) == b) return;  // (else b was hooked meanwhile: again from where the two are now)
    }
}

// arr[c] += 1 for every lane that wants it; lanes of one c share one atomic.  Returns what arr[c] was before this lane's own add.
// Every lane of the wave must call it.
__device__ __forceinline__ unsigned long long cc_wave_claim(unsigned long long *arr, unsigned long long c, bool want)
{
    const uint32_t lane = threadIdx.x & 63;
    unsigned long long res = 0;
    unsigned long long todo = __ballot(want);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned long long lc = __shfl(c, leader);
        const bool mine = want && c == lc;
        const unsigned long long same = __ballot(mine);
        unsigned long long b = 0;
        if (lane == (uint32_t)leader) b = atomicAdd(arr + lc, (unsigned long long)__popcll(same));
        b = __shfl(b, leader);
        if (mine) {
            res = b + (unsigned long long)__popcll(same & ((1ull << lane) - 1));
            want = false;
        }
        todo &= ~same;
    }
    return res;
}

template <class I>
__global__ void __launch_bounds__(CC_THREADS) k_cc_init(I *__restrict__ parent, unsigned long long n)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i < n) parent[i] = (I)i;
}

template <int MODE, class I>
__global__ void __launch_bounds__(CC_THREADS) k_cc_union(const uint64_t *__restrict__ words, int k, TableView t, unsigned long long n_slots,
                                                         const unsigned long long *__restrict__ first, I *parent)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i > n_slots) return;
    const unsigned long long p = first[i];
    if (p == CC_NONE) return;
    const Kmer v = extract_kmer(words, p, k);
#pragma unroll 1
    for (int j = 0; j < 8; j++) {
        const uint64_t key = (uint64_t)key_of<MODE>(neighbour(v, k, 0, j), k);
        uint32_t count;
        const unsigned long long at = table_locate<MODE>(t, key, n_slots, &count);
        if (at == CC_NONE || at == i || first[at] == CC_NONE) continue;  // (a key that no window holds is no vertex)
        cc_unite(parent, (I)i, (I)at);
    }
}

// ctr: [0] members, [1] roots, [2] members listed, [3] roots listed
template <class I>
__global__ void __launch_bounds__(CC_THREADS) k_cc_flatten(const unsigned long long *__restrict__ first, I *parent, unsigned long long n_slots,
                                                           unsigned long long *ctr)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * CC_THREADS + threadIdx.x;
    unsigned long long member = 0, root = 0;
    if (i <= n_slots && first[i] != CC_NONE) {
        I r = (I)i, p;
        while ((p = cc_load(parent + r)) != r) r = p;  // (nothing is hooked in this launch: the roots stand)
        cc_store(parent + i, r);
        member = 1;
        root = r == (I)i;
    }
    wave_add_ull(ctr, member);
    wave_add_ull(ctr + 1, root);
}

template <class I>
__global__ void __launch_bounds__(CC_THREADS) k_cc_members(const unsigned long long *__restrict__ first, unsigned long long n_slots, unsigned long long *ctr,
                                                           I *__restrict__ m_slot, unsigned long long *__restrict__ m_pos)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * CC_THREADS + threadIdx.x;
    const unsigned long long p = i <= n_slots ? first[i] : CC_NONE;
    const unsigned long long at = cc_wave_claim(ctr, 2, p != CC_NONE);  // (one add a wave)
    if (p == CC_NONE) return;
    m_slot[at] = (I)i;
    m_pos[at] = p;
}

template <class I>
__global__ void __launch_bounds__(CC_THREADS) k_cc_rootmin(const I *__restrict__ parent, const I *__restrict__ m_slot, const unsigned long long *__restrict__ m_pos,
                                                           unsigned long long n, unsigned long long *first)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= n) return;
    const I s = m_slot[i], r = parent[s];
    if (r != s) atomicMin(first + r, m_pos[i]);
}

template <class I>
__global__ void __launch_bounds__(CC_THREADS) k_cc_roots(const I *__restrict__ parent, const I *__restrict__ m_slot, unsigned long long n,
                                                         const unsigned long long *__restrict__ first, unsigned long long *ctr,
                                                         unsigned long long *__restrict__ r_pos, unsigned long long *__restrict__ r_slot)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * CC_THREADS + threadIdx.x;
    const I s = i < n ? m_slot[i] : 0;
    const bool root = i < n && parent[s] == s;
    const unsigned long long at = cc_wave_claim(ctr, 3, root);  // (one add a wave)
    if (!root) return;
    r_pos[at] = first[s];
    r_slot[at] = s;
}

// component c (the c-th root by first position): its number into first[root]; the sequence and the offset of its first window
__global__ void __launch_bounds__(CC_THREADS) k_cc_number(const unsigned long long *__restrict__ c_pos, const unsigned long long *__restrict__ c_slot,
                                                          unsigned long long n_comp, const uint64_t *__restrict__ offsets, uint64_t n_seqs,
                                                          unsigned long long *__restrict__ first, uint64_t *__restrict__ seed_seq, uint64_t *__restrict__ seed_pos)
{
    const unsigned long long c = (unsigned long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (c >= n_comp) return;
    first[c_slot[c]] = c;
    const uint64_t p = c_pos[c];
    uint64_t lo = 0, hi = n_seqs;  // the greatest s with offsets[s] <= p: the empty sequences in front of p's share its offset
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= p) lo = mid; else hi = mid;
    }
    seed_seq[c] = lo;
    seed_pos[c] = p - offsets[lo];
}

template <class I>
__global__ void __launch_bounds__(CC_THREADS) k_cc_hist(const I *__restrict__ parent, const I *__restrict__ m_slot, const unsigned long long *__restrict__ m_pos,
                                                        unsigned long long n, const unsigned long long *__restrict__ first,
                                                        const unsigned long long *__restrict__ c_pos, unsigned long long *hist)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * CC_THREADS + threadIdx.x;
    const bool live = i < n;
    unsigned long long c = 0;
    bool seed = false;
    if (live) {
        c = first[parent[m_slot[i]]];
        seed = m_pos[i] == c_pos[c];
    }
    cc_wave_claim(hist, c, live && !seed);  // (the seed's place is the component's first, whoever else comes: it is added on the host)
}

template <class I>
__global__ void __launch_bounds__(CC_THREADS) k_cc_scatter(const uint64_t *__restrict__ words, int k, TableView t, unsigned long long n_slots,
                                                           const I *__restrict__ parent, const I *__restrict__ m_slot,
                                                           const unsigned long long *__restrict__ m_pos, unsigned long long n,
                                                           const unsigned long long *__restrict__ first, const unsigned long long *__restrict__ c_pos,
                                                           const unsigned long long *__restrict__ c_off, unsigned long long *cursor,
                                                           uint64_t *__restrict__ out_hi, uint64_t *__restrict__ out_lo, int16_t *__restrict__ out_cov)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * CC_THREADS + threadIdx.x;
    const bool live = i < n;
    unsigned long long c = 0, p = 0;
    I s = 0;
    bool seed = false;
    if (live) {
        s = m_slot[i];
        p = m_pos[i];
        c = first[parent[s]];
        seed = p == c_pos[c];
    }
    const unsigned long long rank = cc_wave_claim(cursor, c, live && !seed);
    if (!live) return;
    const unsigned long long at = c_off[c] + (seed ? 0 : 1 + rank);
    const Kmer v = extract_kmer(words, p, k);
    const unsigned long long count = (unsigned long long)s == n_slots ? *t.empty_cnt : t.slots[s].count;
    out_hi[at] = v.hi;
    out_lo[at] = v.lo;
    out_cov[at] = (int16_t)(count > 32767ull ? 32767 : (int)count);
}

constexpr char API[] = "mc_components";

template <class T>
T *host_array(uint64_t n) { return static_cast<T *>(calloc(std::max<uint64_t>(n, 1), sizeof(T))); }

int empty_result(mc_ctx *c, mc_components_result *out)
{
    out->comp_offsets = host_array<uint64_t>(1);
    if (!out->comp_offsets) return fail(c, MC_ENOMEM, "%s: no host memory", API);
    return MC_OK;
}

uint32_t blocks(unsigned long long n) { return (uint32_t)((n + CC_THREADS - 1) / CC_THREADS); }

template <class I>
int run_components(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_off, uint64_t n_seqs, uint64_t first_pos, uint64_t end_all, mc_components_result *out)
{
    const unsigned long long n_slots = c->n_slots(), n_v = n_slots + 1;  // (the vertex behind the last slot: the key counted beside the table)
    const int k = c->cfg.k;
    const TableView t = c->view();
    hipStream_t st = c->stream;
    DevBuf<unsigned long long> first, ctr;
    DevBuf<I> parent;
    HIPCHK(c, first.alloc(n_v));
    HIPCHK(c, parent.alloc(n_v));
    HIPCHK(c, ctr.alloc(4));
    HIPCHK(c, hipMemsetAsync(ctr.p, 0, 4 * sizeof(unsigned long long), st));
    const uint64_t n_tiles = (end_all - first_pos + CC_TILE - 1) / CC_TILE;
    const dim3 gv(blocks(n_v)), bt(CC_THREADS);
    double ms = 0;
    if (int rc = timed(c, &ms, [&] {
            (void)hipMemsetAsync(first.p, 0xFF, n_v * sizeof(unsigned long long), st);
            hipLaunchKernelGGL(k_cc_init<I>, gv, bt, 0, st, parent.p, n_v);
            for_key_mode(c->cfg.key_mode, [&](auto mode) {
                hipLaunchKernelGGL(k_cc_first<mode()>, dim3((uint32_t)n_tiles), bt, 0, st, d_words, d_off, n_seqs, first_pos, end_all, k, t, n_slots, first.p);
                hipLaunchKernelGGL((k_cc_union<mode(), I>), gv, bt, 0, st, d_words, k, t, n_slots, first.p, parent.p);
            });
            hipLaunchKernelGGL(k_cc_flatten<I>, gv, bt, 0, st, first.p, parent.p, n_slots, ctr.p);
        }))
        return rc;
    unsigned long long *h = c->h_scratch;
    HIPCHK(c, hipMemcpyAsync(h, ctr.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const unsigned long long n_members = h[0], n_comp = h[1];
    if (n_members == 0) {
        out->device_ms = ms;
        return empty_result(c, out);
    }

    DevBuf<I> m_slot;
    DevBuf<unsigned long long> m_pos, r_pos, r_slot;
    HIPCHK(c, m_slot.alloc(n_members));
    HIPCHK(c, m_pos.alloc(n_members));
    HIPCHK(c, r_pos.alloc(n_comp));
    HIPCHK(c, r_slot.alloc(n_comp));
    const dim3 gm(blocks(n_members)), gc(blocks(n_comp));
    if (int rc = timed(c, &ms, [&] {
            hipLaunchKernelGGL(k_cc_members<I>, gv, bt, 0, st, first.p, n_slots, ctr.p, m_slot.p, m_pos.p);
            hipLaunchKernelGGL(k_cc_rootmin<I>, gm, bt, 0, st, parent.p, m_slot.p, m_pos.p, n_members, first.p);
            hipLaunchKernelGGL(k_cc_roots<I>, gm, bt, 0, st, parent.p, m_slot.p, n_members, first.p, ctr.p, r_pos.p, r_slot.p);
        }))
        return rc;
    // the roots by their components' first positions (distinct: a window holds one key): the reference's comp<N>
    std::vector<std::pair<unsigned long long, unsigned long long>> roots(n_comp);
    {
        std::vector<unsigned long long> hp(n_comp), hs(n_comp);
        HIPCHK(c, hipMemcpy(hp.data(), r_pos.p, n_comp * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(hs.data(), r_slot.p, n_comp * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (unsigned long long i = 0; i < n_comp; i++) roots[i] = {hp[i], hs[i]};
        std::sort(roots.begin(), roots.end());
        for (unsigned long long i = 0; i < n_comp; i++) { hp[i] = roots[i].first; hs[i] = roots[i].second; }
        HIPCHK(c, hipMemcpy(r_pos.p, hp.data(), n_comp * sizeof(unsigned long long), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(r_slot.p, hs.data(), n_comp * sizeof(unsigned long long), hipMemcpyHostToDevice));
    }
    DevBuf<unsigned long long> hist, c_off;
    DevBuf<uint64_t> seed_seq, seed_pos, o_hi, o_lo;
    DevBuf<int16_t> o_cov;
    HIPCHK(c, hist.alloc(n_comp));
    HIPCHK(c, c_off.alloc(n_comp + 1));
    HIPCHK(c, seed_seq.alloc(n_comp));
    HIPCHK(c, seed_pos.alloc(n_comp));
    HIPCHK(c, o_hi.alloc(n_members));
    HIPCHK(c, o_lo.alloc(n_members));
    HIPCHK(c, o_cov.alloc(n_members));
    if (int rc = timed(c, &ms, [&] {
            (void)hipMemsetAsync(hist.p, 0, n_comp * sizeof(unsigned long long), st);
            hipLaunchKernelGGL(k_cc_number, gc, bt, 0, st, r_pos.p, r_slot.p, n_comp, d_off, n_seqs, first.p, seed_seq.p, seed_pos.p);
            hipLaunchKernelGGL(k_cc_hist<I>, gm, bt, 0, st, parent.p, m_slot.p, m_pos.p, n_members, first.p, r_pos.p, hist.p);
        }))
        return rc;
    out->n_components = n_comp;
    out->n_kmers = n_members;
    out->comp_offsets = host_array<uint64_t>(n_comp + 1);
    out->seed_seq = host_array<uint64_t>(n_comp);
    out->seed_pos = host_array<uint64_t>(n_comp);
    out->hi = host_array<uint64_t>(n_members);
    out->lo = host_array<uint64_t>(n_members);
    out->cov = host_array<int16_t>(n_members);
    if (!out->comp_offsets || !out->seed_seq || !out->seed_pos || !out->hi || !out->lo || !out->cov) return fail(c, MC_ENOMEM, "%s: no host memory", API);
    {
        std::vector<unsigned long long> hh(n_comp);
        HIPCHK(c, hipMemcpy(hh.data(), hist.p, n_comp * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        uint64_t run = 0;
        for (unsigned long long i = 0; i < n_comp; i++) {
            out->comp_offsets[i] = run;
            run += hh[i] + 1;  // (and the seed)
        }
        out->comp_offsets[n_comp] = run;
        if (run != n_members) return fail(c, MC_EHIP, "%s: %llu members in %llu places", API, n_members, (unsigned long long)run);
        HIPCHK(c, hipMemcpy(c_off.p, out->comp_offsets, (n_comp + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    if (int rc = timed(c, &ms, [&] {
            (void)hipMemsetAsync(hist.p, 0, n_comp * sizeof(unsigned long long), st);  // (now the cursors)
            hipLaunchKernelGGL(k_cc_scatter<I>, gm, bt, 0, st, d_words, k, t, n_slots, parent.p, m_slot.p, m_pos.p, n_members, first.p, r_pos.p, c_off.p,
                               hist.p, o_hi.p, o_lo.p, o_cov.p);
        }))
        return rc;
    HIPCHK(c, hipMemcpy(out->seed_seq, seed_seq.p, n_comp * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out->seed_pos, seed_pos.p, n_comp * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out->hi, o_hi.p, n_members * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out->lo, o_lo.p, n_members * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out->cov, o_cov.p, n_members * sizeof(int16_t), hipMemcpyDeviceToHost));
    out->device_ms = ms;
    return MC_OK;
}

}  // namespace

void mc_components_free(mc_components_result *r)
{
    if (!r) return;
    free(r->comp_offsets); free(r->seed_seq); free(r->seed_pos); free(r->hi); free(r->lo); free(r->cov);
    *r = mc_components_result{};
}

int mc_components_dev(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_seq_offsets, uint64_t n_seqs, mc_components_result *out)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!out) return fail(c, MC_EINVAL, "%s: null pointer", API);
    *out = mc_components_result{};
    if (!c->finalized) return fail(c, MC_ESTATE, "%s: call mc_finalize_counts first", API);
    if (n_seqs && (!d_words || !d_seq_offsets)) return fail(c, MC_EINVAL, "%s: null pointer", API);
    if (n_seqs == 0) return empty_result(c, out);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // (hash keys in minimizer bins: a window's key does not say where it lives -- the table moves to hash-prefix regions, once)
    if (int rc = by_key_ready(c)) return rc;
    if (int rc = materialize(c)) return rc;  // (an empty table that was never written)
    unsigned long long *h = c->h_scratch;
    HIPCHK(c, hipMemcpyAsync(h, d_seq_offsets, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h + 1, d_seq_offsets + n_seqs, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t first_pos = h[0], end_all = h[1];
    if (end_all < first_pos || (end_all - first_pos) / CC_TILE >= (1ull << 31) || c->n_slots() / CC_THREADS >= (1ull << 31) - 1)
        return fail(c, MC_EINVAL, "%s: seq_offsets run from %llu to %llu", API, h[0], h[1]);
    if (end_all == first_pos) return empty_result(c, out);  // (no bases)
    // parents are slot numbers: 32 bits while the table, with the vertex behind it, has fewer than 2^32 of them
    const int rc = c->n_slots() + 1 < (1ull << 32) ? run_components<unsigned int>(c, d_words, d_seq_offsets, n_seqs, first_pos, end_all, out)
                                                   : run_components<unsigned long long>(c, d_words, d_seq_offsets, n_seqs, first_pos, end_all, out);
    if (rc) mc_components_free(out);
    return rc;
}

int mc_components(mc_ctx *c, const uint64_t *words, const uint64_t *seq_offsets, uint64_t n_seqs, mc_components_result *out)
{
    if (!c) return MC_EINVAL;
    if (n_seqs == 0 || !words || !seq_offsets || !out)  // (nothing to copy: the device form checks the rest and says what is wrong)
        return mc_components_dev(c, nullptr, nullptr, n_seqs, out);
    HostStage st(c);
    const uint64_t *dw = st.in(words, packed_words(seq_offsets, n_seqs)), *doff = st.in(seq_offsets, n_seqs + 1);
    if (int rc = st.staged()) return rc;
    return mc_components_dev(c, dw, doff, n_seqs, out);
}
