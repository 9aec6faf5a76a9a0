// libmcgpu.so, the unitigs unit: the state that the reference's unitig compaction ends in, by link analysis instead of merges
// (include/mcgpu.h mc_unitigs*; src/algo/OneSequenceCalculator.java:387-451 initializeStructures + doMerge, which
// csrc/host/picture.cpp make_picture restates).  context.h lists the other units.
//
// n entries make N = 2n nodes: node 2e spells entry e's k-mer, node 2e + 1 its reverse complement.  One thread a node (or an
// entry) in every kernel, no LDS, and nothing that depends on the order in which threads run:
//   k_ut_build   an entry's canonical k-mer goes into an open-addressing table (kmer_set.h's keys: one word a slot for k <= 32, two
//                above, at most half full); val[slot] = the node that spells the canonical form.  A key that is there already
//                raises the duplicate flag.
//   k_ut_nbrs    a node's neighbours: the four successor strings of node p ^ 1 looked up, the hits turned into node ids (both nodes
//                of a palindrome), sorted by a fixed network of five: deg[p], and the list padded to five in a scratch array.
//   k_ut_link    link[p] = q where neighbours(p) = {q}, neighbours(q) = {p} and the classes agree, with a mark on an irregular link.
//   k_ut_rank0 / k_ut_jump   chains of oriented nodes: prev(a) = link[a] ^ 1, next(a) = link[a ^ 1].  Pointer jumping towards the head
//                over ceil(log2 N) rounds, two buffers in turn: every node learns its head, its distance from it and whether a
//                link up to there is irregular.  A node whose pointer does not rest on a head after that is on a cycle.
//   k_ut_chains  a chain is irregular when a node or its twin (the same entries read backwards) saw a mark or a cycle; the tail
//                of a regular chain of m >= 2 whose head is smaller than the twin's head gives that head m and last_rc.
//   k_ut_heads   the listed heads in node order (hipCUB scans give their ordinals and their first words).
//   k_ut_bases   every node of a listed chain ORs its last base into the unitig's words at rank + k - 1, the head its whole k-mer.
//                Unitigs start on word boundaries, and OR is commutative: the words are the same whoever comes first.
//   k_ut_pack / k_ut_scatter   the neighbours lists one after another, and the irregular entries, by scanned offsets.
// DESIGN.md 3.12 has the sizes and the registers, tests/test_unitigs_kernel_resources.py holds the kernels to no scratch.
#include "context.h"
#include "kmer_set.h"

#include <hipcub/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace {

constexpr int UT_THREADS = 256;
constexpr uint32_t UT_NONE = ~0u;         // no link, no neighbour
constexpr uint32_t UT_IRR = 1u << 31;     // on a link: it is irregular (node ids are below 2^31)

template <bool WIDE>
__device__ __forceinline__ Kmer ut_entry(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint64_t e, int k)
{
    Kmer v{WIDE ? hi[e] : 0, lo[e]};
    if (WIDE) v.hi &= ~0ull >> (128 - 2 * k);  // (bits above the k-mer are not the caller's to set: dropped)
    else if (k < 32) v.lo &= ~0ull >> (64 - 2 * k);
    return v;
}

template <bool WIDE>
__device__ __forceinline__ bool ut_le(const Kmer &a, const Kmer &b)  // the order rs_key takes its smaller k-mer by
{
    return WIDE ? (a.hi < b.hi || (a.hi == b.hi && a.lo <= b.lo)) : a.lo <= b.lo;
}

// table: 2^lg_cap slots of one word (k <= 32) or two (above), all ones when the call starts; val: a word a slot
template <bool WIDE>
__global__ void __launch_bounds__(UT_THREADS) k_ut_build(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint32_t n, int k,
                                                         unsigned long long *__restrict__ table, uint32_t *__restrict__ val, int lg_cap,
                                                         uint32_t *__restrict__ dup)
{
    const uint32_t e = blockIdx.x * UT_THREADS + threadIdx.x;
    if (e >= n) return;
    const Kmer v = ut_entry<WIDE>(hi, lo, e, k);
    const Kmer r = rc_kmer(v, k);
    const RsKey key = rs_key<WIDE>(v.hi, v.lo, r.hi, r.lo);
    const bool fw = ut_le<WIDE>(v, r);
    const uint64_t mask = (1ull << lg_cap) - 1;
    uint64_t s = rs_home(rs_hash<WIDE>(key), lg_cap);
    for (uint64_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {  // (at most half full: a free slot comes)
        unsigned long long *slot = table + (WIDE ? 2 * s : s);
        const unsigned long long was = atomicCAS(slot, (unsigned long long)RS_EMPTY, (unsigned long long)key.a);
        if (was != RS_EMPTY && was != key.a) continue;
        if (!WIDE) {
            if (was == key.a) atomicOr(dup, 1u);  // (another entry's k-mer, or its reverse complement)
            else val[s] = 2 * e + (fw ? 0 : 1);
            return;
        }
        // (reads_in_set.hip k_rs_build: whoever writes the second word first has the slot)
        const unsigned long long was_b = atomicCAS(slot + 1, (unsigned long long)RS_EMPTY, (unsigned long long)key.b);
        if (was_b == RS_EMPTY) { val[s] = 2 * e + (fw ? 0 : 1); return; }
        if (was_b == key.b) { atomicOr(dup, 1u); return; }
    }
}

// the slot of a key, or all ones
template <bool WIDE>
__device__ __forceinline__ uint64_t ut_find(const uint64_t *__restrict__ table, int lg_cap, const RsKey &key)
{
    const uint64_t mask = (1ull << lg_cap) - 1;
    uint64_t s = rs_home(rs_hash<WIDE>(key), lg_cap);
    for (uint64_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {
        if (WIDE) {
            const ulonglong2 cur = *reinterpret_cast<const ulonglong2 *>(table + 2 * s);
            if (cur.x == key.a && cur.y == key.b) return s;
            if (cur.x == RS_EMPTY) return ~0ull;
        } else {
            const uint64_t cur = table[s];
            if (cur == key.a) return s;
            if (cur == RS_EMPTY) return ~0ull;
        }
    }
    return ~0ull;
}

__device__ __forceinline__ void ut_order(uint32_t &a, uint32_t &b)
{
    const uint32_t lo = min(a, b), hi = max(a, b);
    a = lo;
    b = hi;
}

// pad: N words for each of the five places of a list (place i of node p at pad[i * N + p]); places past deg[p] are not written
template <bool WIDE>
__global__ void __launch_bounds__(UT_THREADS) k_ut_nbrs(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint32_t n_nodes, int k,
                                                        const uint64_t *__restrict__ table, const uint32_t *__restrict__ val, int lg_cap,
                                                        uint8_t *__restrict__ deg, uint32_t *__restrict__ pad)
{
    const uint32_t p = blockIdx.x * UT_THREADS + threadIdx.x;
    if (p >= n_nodes) return;
    const Kmer v = ut_entry<WIDE>(hi, lo, p >> 1, k);
    const Kmer x = (p & 1) ? v : rc_kmer(v, k);  // node p ^ 1
    const uint64_t kmask_lo = k >= 32 ? ~0ull : ~0ull >> (64 - 2 * k);
    const uint64_t kmask_hi = WIDE ? ~0ull >> (128 - 2 * k) : 0;
    Kmer s0;  // x's last k - 1 bases and an A
    s0.hi = WIDE ? ((x.hi << 2) | (x.lo >> 62)) & kmask_hi : 0;
    s0.lo = (x.lo << 2) & kmask_lo;
    uint32_t r0 = UT_NONE, r1 = UT_NONE, r2 = UT_NONE, r3 = UT_NONE, r4 = UT_NONE;
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) {
        const Kmer s{s0.hi, s0.lo | c};
        const Kmer rs = rc_kmer(s, k);
        const uint64_t at = ut_find<WIDE>(table, lg_cap, rs_key<WIDE>(s.hi, s.lo, rs.hi, rs.lo));
        uint32_t node = UT_NONE;
        if (at != ~0ull) {
            const uint32_t w = val[at];  // spells the smaller of s and rs
            if (s.hi == rs.hi && s.lo == rs.lo) { node = w; r4 = w ^ 1; }  // (a palindrome: at most one of the four, by its first base)
            else node = ut_le<WIDE>(s, rs) ? w : (w ^ 1);
        }
        if (c == 0) r0 = node; else if (c == 1) r1 = node; else if (c == 2) r2 = node; else r3 = node;
    }
    // nine exchanges sort five (absent places are all ones and go last)
    ut_order(r0, r1); ut_order(r3, r4); ut_order(r2, r4); ut_order(r2, r3); ut_order(r1, r4);
    ut_order(r0, r3); ut_order(r0, r2); ut_order(r1, r3); ut_order(r1, r2);
    const uint32_t d = (r0 != UT_NONE) + (r1 != UT_NONE) + (r2 != UT_NONE) + (r3 != UT_NONE) + (r4 != UT_NONE);
    deg[p] = (uint8_t)d;
    const uint64_t N = n_nodes;
    if (d > 0) pad[p] = r0;
    if (d > 1) pad[N + p] = r1;
    if (d > 2) pad[2 * N + p] = r2;
    if (d > 3) pad[3 * N + p] = r3;
    if (d > 4) pad[4 * N + p] = r4;
}

// (A k-mer that is its own reverse complement is spelled by both its nodes: whatever it follows has two neighbours, and what follows it
// follows both.  It never links, so a link needs no look at it.)
__global__ void __launch_bounds__(UT_THREADS) k_ut_link(uint32_t n_nodes, const uint8_t *__restrict__ cls, const uint8_t *__restrict__ deg,
                                                        const uint32_t *__restrict__ pad, uint32_t *__restrict__ link)
{
    const uint32_t p = blockIdx.x * UT_THREADS + threadIdx.x;
    if (p >= n_nodes) return;
    uint32_t l = UT_NONE;
    if (deg[p] == 1) {
        const uint32_t q = pad[p];
        // (q's one neighbour is p: q's prefix is the suffix of p ^ 1, so p's prefix is the suffix of q ^ 1)
        if (deg[q] == 1 && cls[p >> 1] == cls[q >> 1]) l = q | (q == p || q == (p ^ 1) ? UT_IRR : 0);
    }
    link[p] = l;
}

// A node's state while the chains are ranked, one word: the node its pointer rests on (31 bits), whether a link from there to here
// is irregular (bit 31), and the number of links in between (the high word).
__device__ __forceinline__ uint64_t ut_state(uint32_t at, bool irr, uint32_t dist) { return ((uint64_t)dist << 32) | (irr ? UT_IRR : 0) | at; }

__global__ void __launch_bounds__(UT_THREADS) k_ut_rank0(uint32_t n_nodes, const uint32_t *__restrict__ link, uint64_t *__restrict__ state)
{
    const uint32_t a = blockIdx.x * UT_THREADS + threadIdx.x;
    if (a >= n_nodes) return;
    const uint32_t l = link[a], l2 = link[a ^ 1];
    const bool irr = (l != UT_NONE && (l & UT_IRR)) || (l2 != UT_NONE && (l2 & UT_IRR));  // (the entry's own two links)
    const uint32_t prev = l == UT_NONE ? a : ((l & ~UT_IRR) ^ 1);
    // (prev == a with a link: a self-loop, which carries the mark; it rests on itself as a head does)
    state[a] = ut_state(prev, irr, prev == a ? 0 : 1);
}

__global__ void __launch_bounds__(UT_THREADS) k_ut_jump(uint32_t n_nodes, const uint64_t *__restrict__ from, uint64_t *__restrict__ to)
{
    const uint32_t a = blockIdx.x * UT_THREADS + threadIdx.x;
    if (a >= n_nodes) return;
    const uint64_t s = from[a];
    const uint64_t t = from[(uint32_t)s & ~UT_IRR];
    // (a head rests on itself at distance 0: nothing is added twice.  On a cycle the distances wrap and are never used.)
    to[a] = ut_state((uint32_t)t & ~UT_IRR, ((uint32_t)s | (uint32_t)t) & UT_IRR, (uint32_t)(s >> 32) + (uint32_t)(t >> 32));
}

// ulen, last_rc: per node, zero when the call starts; irr: per entry
__global__ void __launch_bounds__(UT_THREADS) k_ut_chains(uint32_t n_nodes, const uint32_t *__restrict__ link, const uint64_t *__restrict__ state,
                                                          uint8_t *__restrict__ regular, uint8_t *__restrict__ irr, uint32_t *__restrict__ ulen,
                                                          uint32_t *__restrict__ last_rc)
{
    const uint32_t a = blockIdx.x * UT_THREADS + threadIdx.x;
    if (a >= n_nodes) return;
    const uint64_t s = state[a], t = state[a ^ 1];
    const uint32_t head = (uint32_t)s & ~UT_IRR;
    const bool cycle = link[head] != UT_NONE;  // (or a self-loop, marked anyway)
    const bool bad = cycle || (((uint32_t)s | (uint32_t)t) & UT_IRR);
    regular[a] = !bad;
    if (!(a & 1)) irr[a >> 1] = bad;
    const uint32_t rank = (uint32_t)(s >> 32);
    if (!bad && link[a ^ 1] == UT_NONE && rank >= 1 && head < (a ^ 1)) {  // the tail of a chain that is listed from this end
        ulen[head] = rank + 1;
        last_rc[head] = a ^ 1;
    }
}

// What the scans read: the i-th term of one of four sums over per-node or per-entry arrays, 0 behind the last (the total lands there).
// (Sums are signed words: rocPRIM's scan-state kernels for them are then not the ones last_copy.hip's select instantiates, and every
// kernel of the library stays in one code object, as the resources tests ask.)
typedef long long ut_sum;
struct UtTerm {
    enum Mode { DEG, IRR, HEADS, WORDS };
    const uint8_t *bytes;
    const uint32_t *ulen;
    uint64_t n;
    int mode, k;
    __host__ __device__ ut_sum operator()(uint64_t i) const
    {
        if (i >= n) return 0;
        if (mode == DEG || mode == IRR) return bytes[i];
        const uint32_t m = ulen[i];
        if (m == 0) return 0;
        return mode == HEADS ? 1 : (ut_sum)(((uint64_t)m + (uint64_t)k - 1 + 31) / 32);
    }
};

__global__ void __launch_bounds__(UT_THREADS) k_ut_heads(uint32_t n_nodes, const uint32_t *__restrict__ ulen, const uint32_t *__restrict__ last_rc,
                                                         const ut_sum *__restrict__ ordinal, const ut_sum *__restrict__ word,
                                                         uint32_t *__restrict__ out_first, uint32_t *__restrict__ out_last_rc,
                                                         uint64_t *__restrict__ out_base_offsets)
{
    const uint32_t a = blockIdx.x * UT_THREADS + threadIdx.x;
    if (a >= n_nodes || ulen[a] == 0) return;
    const uint64_t u = (uint64_t)ordinal[a];
    out_first[u] = a;
    out_last_rc[u] = last_rc[a];
    out_base_offsets[u] = (uint64_t)word[a] * 32;
}

// bases: zero when the call starts
template <bool WIDE>
__global__ void __launch_bounds__(UT_THREADS) k_ut_bases(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint32_t n_nodes, int k,
                                                         const uint8_t *__restrict__ regular, const uint64_t *__restrict__ state,
                                                         const uint32_t *__restrict__ ulen, const ut_sum *__restrict__ word,
                                                         unsigned long long *__restrict__ bases)
{
    const uint32_t a = blockIdx.x * UT_THREADS + threadIdx.x;
    if (a >= n_nodes || !regular[a]) return;
    const uint64_t s = state[a];
    const uint32_t head = (uint32_t)s & ~UT_IRR, rank = (uint32_t)(s >> 32);
    if (ulen[head] == 0) return;  // (a chain of one entry, or listed from its other end)
    unsigned long long *w = bases + word[head];
    const Kmer v = ut_entry<WIDE>(hi, lo, a >> 1, k);
    if (a == head) {  // the whole k-mer, its first base at the top of the unitig's first word
        const Kmer x = (a & 1) ? rc_kmer(v, k) : v;
        if (k <= 32) atomicOr(w, (unsigned long long)(x.lo << (64 - 2 * k)));
        else {
            const int sh = 128 - 2 * k;  // 2 .. 62
            atomicOr(w, (unsigned long long)((x.hi << sh) | (x.lo >> (64 - sh))));
            atomicOr(w + 1, (unsigned long long)(x.lo << sh));
        }
        return;
    }
    // the node's last base: the entry's, or the complement of the entry's first
    const uint64_t b = (a & 1) ? 3 - base_at(v, k, 0) : (v.lo & 3);
    const uint64_t at = (uint64_t)rank + (uint64_t)k - 1;
    atomicOr(w + (at >> 5), (unsigned long long)(b << (62 - 2 * (at & 31))));
}

__global__ void __launch_bounds__(UT_THREADS) k_ut_pack(uint32_t n_nodes, const uint8_t *__restrict__ deg, const uint32_t *__restrict__ pad,
                                                        const ut_sum *__restrict__ at, uint32_t *__restrict__ nbr)
{
    const uint32_t p = blockIdx.x * UT_THREADS + threadIdx.x;
    if (p >= n_nodes) return;
    const uint32_t d = deg[p];
    const uint64_t o = (uint64_t)at[p], N = n_nodes;
    for (uint32_t i = 0; i < d; i++) nbr[o + i] = pad[i * N + p];
}

__global__ void __launch_bounds__(UT_THREADS) k_ut_scatter(uint32_t n, const uint8_t *__restrict__ irr, const ut_sum *__restrict__ at,
                                                           uint32_t *__restrict__ out)
{
    const uint32_t e = blockIdx.x * UT_THREADS + threadIdx.x;
    if (e < n && irr[e]) out[at[e]] = e;
}

constexpr char API[] = "mc_unitigs";

template <class T>
T *host_array(uint64_t n) { return static_cast<T *>(calloc(std::max<uint64_t>(n, 1), sizeof(T))); }

uint32_t blocks(uint64_t n) { return (uint32_t)((n + UT_THREADS - 1) / UT_THREADS); }

// out[i] = the sum of the terms before i, for i = 0 .. term.n (the total last)
int scan(mc_ctx *c, const UtTerm &term, ut_sum *out, DevBuf<char> &temp, size_t &temp_bytes)
{
    const auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), term);
    size_t need = 0;
    HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, out, (int)(term.n + 1), c->stream));
    if (need > temp_bytes || !temp.p) {
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (an earlier scan may still read the block)
        HIPCHK(c, temp.alloc(need));
        temp_bytes = need;
    }
    HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(temp.p, need, in, out, (int)(term.n + 1), c->stream));
    return MC_OK;
}

template <bool WIDE>
int run_unitigs(mc_ctx *c, const uint64_t *d_hi, const uint64_t *d_lo, const uint8_t *d_cls, uint32_t n, mc_unitigs_result *out)
{
    const int k = c->cfg.k;
    const uint32_t N = 2 * n;
    hipStream_t st = c->stream;
    int lg_cap = 6;
    while ((1ull << lg_cap) < 2 * (uint64_t)n) lg_cap++;  // (at most 31: n < 2^30)
    const uint64_t cap = 1ull << lg_cap, table_words = cap * (WIDE ? 2 : 1);
    DevBuf<unsigned long long> table;
    DevBuf<uint32_t> val, dup, pad, link, ulen, last_rc;
    DevBuf<uint8_t> deg, regular, irr;
    DevBuf<uint64_t> state_a, state_b;
    DevBuf<ut_sum> nbr_at, irr_at, ordinal, word;
    DevBuf<char> temp;
    size_t temp_bytes = 0;
    HIPCHK(c, table.alloc(table_words));
    HIPCHK(c, val.alloc(cap));
    HIPCHK(c, dup.alloc(1));
    HIPCHK(c, deg.alloc(N));
    HIPCHK(c, pad.alloc(5ull * N));
    HIPCHK(c, link.alloc(N));
    const uint64_t *tab = reinterpret_cast<const uint64_t *>(table.p);
    const dim3 gn(blocks(n)), gN(blocks(N)), bt(UT_THREADS);
    double ms_set = 0, ms_lists = 0, ms_ranks = 0, ms_chains = 0, ms_order = 0, ms_output = 0;  // (MC_UNITIGS_STATS=1 prints them)
    if (int rc = timed(c, &ms_set, [&] {
            (void)hipMemsetAsync(table.p, 0xff, table_words * 8, st);
            (void)hipMemsetAsync(dup.p, 0, 4, st);
            hipLaunchKernelGGL(k_ut_build<WIDE>, gn, bt, 0, st, d_hi, d_lo, n, k, table.p, val.p, lg_cap, dup.p);
        }))
        return rc;
    uint32_t *h_dup = reinterpret_cast<uint32_t *>(c->h_scratch);
    HIPCHK(c, hipMemcpyAsync(h_dup, dup.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (*h_dup) return fail(c, MC_EINVAL, "%s: two entries are the same k-mer or each other's reverse complement", API);

    HIPCHK(c, state_a.alloc(N));
    HIPCHK(c, state_b.alloc(N));
    HIPCHK(c, regular.alloc(N));
    HIPCHK(c, irr.alloc(n));
    HIPCHK(c, ulen.alloc(N));
    HIPCHK(c, last_rc.alloc(N));
    int rounds = 0;
    while ((1ull << rounds) < N) rounds++;
    uint64_t *from = state_a.p, *to = state_b.p;
    if (int rc = timed(c, &ms_lists, [&] {
            hipLaunchKernelGGL(k_ut_nbrs<WIDE>, gN, bt, 0, st, d_hi, d_lo, N, k, tab, val.p, lg_cap, deg.p, pad.p);
            hipLaunchKernelGGL(k_ut_link, gN, bt, 0, st, N, d_cls, deg.p, pad.p, link.p);
        }))
        return rc;
    if (int rc = timed(c, &ms_ranks, [&] {
            hipLaunchKernelGGL(k_ut_rank0, gN, bt, 0, st, N, link.p, from);
            for (int r = 0; r < rounds; r++) {
                hipLaunchKernelGGL(k_ut_jump, gN, bt, 0, st, N, from, to);
                std::swap(from, to);
            }
        }))
        return rc;
    if (int rc = timed(c, &ms_chains, [&] {
            (void)hipMemsetAsync(ulen.p, 0, (uint64_t)N * 4, st);
            (void)hipMemsetAsync(last_rc.p, 0, (uint64_t)N * 4, st);
            hipLaunchKernelGGL(k_ut_chains, gN, bt, 0, st, N, link.p, from, regular.p, irr.p, ulen.p, last_rc.p);
        }))
        return rc;
    table.reset();
    val.reset();

    HIPCHK(c, nbr_at.alloc((uint64_t)N + 1));
    HIPCHK(c, irr_at.alloc((uint64_t)n + 1));
    HIPCHK(c, ordinal.alloc((uint64_t)N + 1));
    HIPCHK(c, word.alloc((uint64_t)N + 1));
    HIPCHK(c, hipEventRecord(c->ev0, st));
    if (int rc = scan(c, UtTerm{deg.p, nullptr, N, UtTerm::DEG, k}, nbr_at.p, temp, temp_bytes)) return rc;
    if (int rc = scan(c, UtTerm{irr.p, nullptr, n, UtTerm::IRR, k}, irr_at.p, temp, temp_bytes)) return rc;
    if (int rc = scan(c, UtTerm{nullptr, ulen.p, N, UtTerm::HEADS, k}, ordinal.p, temp, temp_bytes)) return rc;
    if (int rc = scan(c, UtTerm{nullptr, ulen.p, N, UtTerm::WORDS, k}, word.p, temp, temp_bytes)) return rc;
    unsigned long long *h = c->h_scratch;
    HIPCHK(c, hipMemcpyAsync(h, nbr_at.p + N, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h + 1, irr_at.p + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h + 2, ordinal.p + N, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h + 3, word.p + N, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipEventRecord(c->ev1, st));
    HIPCHK(c, hipStreamSynchronize(st));
    {
        float scan_ms = 0;
        HIPCHK(c, hipEventElapsedTime(&scan_ms, c->ev0, c->ev1));
        ms_order = scan_ms;
    }
    const uint64_t n_nbr = h[0], n_irr = h[1], n_uni = h[2], n_words = h[3];  // (never negative)

    DevBuf<uint32_t> nbr, irregular, o_first, o_last_rc;
    DevBuf<uint64_t> o_off;
    DevBuf<unsigned long long> bases;
    HIPCHK(c, nbr.alloc(n_nbr));
    HIPCHK(c, irregular.alloc(n_irr));
    HIPCHK(c, o_first.alloc(n_uni));
    HIPCHK(c, o_last_rc.alloc(n_uni));
    HIPCHK(c, o_off.alloc(n_uni + 1));
    HIPCHK(c, bases.alloc(n_words));
    if (int rc = timed(c, &ms_output, [&] {
            (void)hipMemsetAsync(bases.p, 0, std::max<uint64_t>(n_words, 1) * 8, st);
            hipLaunchKernelGGL(k_ut_pack, gN, bt, 0, st, N, deg.p, pad.p, nbr_at.p, nbr.p);
            hipLaunchKernelGGL(k_ut_scatter, gn, bt, 0, st, n, irr.p, irr_at.p, irregular.p);
            hipLaunchKernelGGL(k_ut_heads, gN, bt, 0, st, N, ulen.p, last_rc.p, ordinal.p, word.p, o_first.p, o_last_rc.p, o_off.p);
            hipLaunchKernelGGL(k_ut_bases<WIDE>, gN, bt, 0, st, d_hi, d_lo, N, k, regular.p, from, ulen.p, word.p, bases.p);
        }))
        return rc;

    out->n_nodes = N;
    out->n_unitigs = n_uni;
    out->n_irregular = n_irr;
    out->deg = host_array<uint8_t>(N);
    out->nbr = host_array<uint32_t>(n_nbr);
    out->first = host_array<uint32_t>(n_uni);
    out->last_rc = host_array<uint32_t>(n_uni);
    out->base_offsets = host_array<uint64_t>(n_uni + 1);
    out->bases = host_array<uint64_t>(n_words);
    out->irregular = host_array<uint32_t>(n_irr);
    if (!out->deg || !out->nbr || !out->first || !out->last_rc || !out->base_offsets || !out->bases || !out->irregular)
        return fail(c, MC_ENOMEM, "%s: no host memory", API);
    HIPCHK(c, hipMemcpy(out->deg, deg.p, N, hipMemcpyDeviceToHost));
    if (n_nbr) HIPCHK(c, hipMemcpy(out->nbr, nbr.p, n_nbr * 4, hipMemcpyDeviceToHost));
    if (n_irr) HIPCHK(c, hipMemcpy(out->irregular, irregular.p, n_irr * 4, hipMemcpyDeviceToHost));
    if (n_uni) {
        HIPCHK(c, hipMemcpy(out->first, o_first.p, n_uni * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(out->last_rc, o_last_rc.p, n_uni * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(out->base_offsets, o_off.p, n_uni * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(out->bases, bases.p, n_words * 8, hipMemcpyDeviceToHost));
    }
    out->base_offsets[n_uni] = n_words * 32;
    out->device_ms = ms_set + ms_lists + ms_ranks + ms_chains + ms_order + ms_output;
    if (c->sw.unitigs_stats)
        fprintf(stderr, "mc_unitigs: n=%u k=%d set_ms=%.3f lists_ms=%.3f ranks_ms=%.3f rounds=%d chains_ms=%.3f order_ms=%.3f output_ms=%.3f\n", n, k, ms_set,
                ms_lists, ms_ranks, rounds, ms_chains, ms_order, ms_output);
    return MC_OK;
}

}  // namespace

void mc_unitigs_free(mc_unitigs_result *r)
{
    if (!r) return;
    free(r->deg); free(r->nbr); free(r->first); free(r->last_rc); free(r->base_offsets); free(r->bases); free(r->irregular);
    *r = mc_unitigs_result{};
}

int mc_unitigs_dev(mc_ctx *c, const uint64_t *d_hi, const uint64_t *d_lo, const uint8_t *d_cls, uint64_t n, mc_unitigs_result *out)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!out) return fail(c, MC_EINVAL, "%s: null pointer", API);
    *out = mc_unitigs_result{};
    const bool wide = c->cfg.k > 32;
    if (n >= (1ull << 30)) return fail(c, MC_EINVAL, "%s: %llu entries (at most 2^30 - 1)", API, (unsigned long long)n);
    if (n && (!d_lo || !d_cls || (wide && !d_hi))) return fail(c, MC_EINVAL, "%s: null pointer", API);
    if (n == 0) {
        out->base_offsets = host_array<uint64_t>(1);
        if (!out->base_offsets) return fail(c, MC_ENOMEM, "%s: no host memory", API);
        return MC_OK;
    }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const int rc = wide ? run_unitigs<true>(c, d_hi, d_lo, d_cls, (uint32_t)n, out) : run_unitigs<false>(c, d_hi, d_lo, d_cls, (uint32_t)n, out);
    if (rc) mc_unitigs_free(out);
    return rc;
}

int mc_unitigs(mc_ctx *c, const uint64_t *hi, const uint64_t *lo, const uint8_t *cls, uint64_t n, mc_unitigs_result *out)
{
    if (!c) return MC_EINVAL;
    const bool wide = c->cfg.k > 32;
    if (n == 0 || n >= (1ull << 30) || !lo || !cls || !out || (wide && !hi))  // (nothing to copy: the device form says what is wrong)
        return mc_unitigs_dev(c, nullptr, nullptr, nullptr, n, out);
    HostStage st(c);
    const uint64_t *dhi = wide ? st.in(hi, n) : nullptr, *dlo = st.in(lo, n);
    const uint8_t *dcls = st.in(cls, n);
    if (int rc = st.staged()) {
        *out = mc_unitigs_result{};
        return rc;
    }
    return mc_unitigs_dev(c, dhi, dlo, dcls, n, out);
}
