// libmcgpu.so, the walk-order unit: the order in which KmerEnvCalculator.runBfs pops the k-mers of every component for the first
// time, and which of them it pops more than once (include/mcgpu.h mc_walk_order*; src/algo/KmerEnvCalculator.java:60-76, which
// csrc/host/tool_visualisers.cpp replay_component_walk restates with the whole queue).  context.h lists the other units.
//
// The reference's queue has no visited set: a k-mer is queued once for every shortest path that reaches it.  What the subgraph
// needs of that queue is the order of the FIRST pops and whether there was a SECOND one, and both follow from a queue that keeps
// at most two entries a member (DESIGN.md 3.18 has the argument).  An entry is (member, orientation); positions count from the
// component's seed at 0; first[t] is the position of t's first entry (all ones: none yet), cnt[t] the entries it has (0, 1, 2).
// A level is the run of entries that the level before pushed.  One level:
//   candidates  entry i of the level (position p) and slot j of its eight neighbours (A, G, C, T, left before right) give the
//               candidate (key = 8 i + j, target t) when t is a member of the same component and first[t] >= p;
//   two mins    per target the smallest key, then the smallest of the others;
//   keep        a candidate stays when it is one of those two and the target has room for it (2 - cnt[t]);
//   scan        the kept candidates get the positions behind the level in key order; those that are a target's first entry
//               also get the next places of `order`;
//   update      first[] and cnt[] of the targets, by the thread of the smallest key alone.
// Kernels:
//   k_wo_build    the index: an open-addressing table of 2^lg_cap >= 2n words, a slot holds a MEMBER NUMBER (all ones: free)
//                 and a probe compares through hi / lo against the k-mer and its reverse complement (trim_paths.hip's layout,
//                 kmer_set.h's canonical key for the hash).  A slot that holds the same k-mer in either orientation raises the
//                 duplicate flag.
//   k_wo_adj      a member's eight neighbours in its stored orientation, 32 bytes: member number | orientation bit, or all ones.
//                 A hit outside the member's own slice is no neighbour.  The reverse complement's list is this one read
//                 backwards with the bits flipped.
//   k_wo_init     every seed: entry 0, first 0, cnt 1, place 0 of order.
//   k_wo_narrow   a workgroup a component, taken from a work list by an atomic counter; levels of at most w entries (a thread
//                 an entry) loop inside the kernel with the two mins in an LDS table of WO_SLOTS targets and the scan over the
//                 workgroup.  A component whose level is wider is put on the wide list and left.
//   k_wo_min<1|2>, k_wo_keep, k_wo_scatter   one level of one component across the grid: the mins are 64-bit words a member in
//                 device memory (a key can pass 2^32), the keep pass leaves a mask word an entry and a sum a block, the scatter
//                 pass adds the sums in front of its block, writes the entries and resets the mins.  The last block writes the
//                 component's new level; the host reads it (one round trip a wide level).
// first[] / cnt[] of a component are written by one workgroup at a time inside k_wo_narrow, and across workgroups only with a
// kernel boundary in between; the mins of the wide path are agent-scope atomics.
// Device memory a member beside the caller's arrays: index 8 - 16, adjacency 32, first 4, cnt 1, queue 8, order 4, twice 1
// (58 - 66); once a level is wide also the mins 16 and, for the widest level so far, 4 an entry.
#include "context.h"
#include "kmer_set.h"

namespace {

constexpr int WO_THREADS = 256;
constexpr uint32_t WO_W = 256;            // entries of a level that k_wo_narrow takes: a thread an entry
constexpr uint32_t WO_SLOTS = 4096;       // its LDS table: 8 WO_W candidates at the most, so at most half full
constexpr int WO_SLOT_BITS = 12;
constexpr int WO_WIDE_K = 33;             // from this k on a k-mer is two words
constexpr uint32_t WO_NONE = ~0u;         // a free slot, no neighbour, no first entry
constexpr uint32_t WO_RC = 1u << 31;      // on an entry or a neighbour: the member's reverse complement (members are below 2^30)
constexpr unsigned long long WO_NOKEY = ~0ull;

struct WoLevel {  // a component between two launches: its current level [s, e), the places of `order` that are filled
    uint32_t s, e, nf, pad;
};

template <bool WIDE>
__device__ __forceinline__ Kmer wo_entry(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint64_t e, int k)
{
    Kmer v{WIDE ? hi[e] : 0, lo[e]};
    if (WIDE) v.hi &= ~0ull >> (128 - 2 * k);  // (bits above the k-mer are dropped, as ut_entry does)
    else if (k < 32) v.lo &= ~0ull >> (64 - 2 * k);
    return v;
}

template <bool WIDE>
__device__ __forceinline__ bool wo_same(const Kmer &a, const Kmer &b) { return a.lo == b.lo && (!WIDE || a.hi == b.hi); }

template <bool WIDE>
__device__ __forceinline__ uint64_t wo_home(const Kmer &v, const Kmer &r, int lg_cap)
{
    return rs_home(rs_hash<WIDE>(rs_key<WIDE>(v.hi, v.lo, r.hi, r.lo)), lg_cap);
}

// index: 2^lg_cap words, all ones when the call starts
template <bool WIDE>
__global__ void __launch_bounds__(WO_THREADS) k_wo_build(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint32_t n, int k,
                                                         uint32_t *__restrict__ index, int lg_cap, uint32_t *__restrict__ dup)
{
    const uint32_t e = blockIdx.x * WO_THREADS + threadIdx.x;
    if (e >= n) return;
    const Kmer v = wo_entry<WIDE>(hi, lo, e, k);
    const Kmer r = rc_kmer(v, k);
    const uint64_t mask = (1ull << lg_cap) - 1;
    uint64_t s = wo_home<WIDE>(v, r, lg_cap);
    for (uint64_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {  // (at most half full: a free slot comes)
        const uint32_t was = atomicCAS(index + s, WO_NONE, e);
        if (was == WO_NONE) return;
        const Kmer u = wo_entry<WIDE>(hi, lo, was, k);
        if (wo_same<WIDE>(u, v) || wo_same<WIDE>(u, r)) {
            atomicOr(dup, 1u);
            return;
        }
    }
}

// the member that is k-mer x or its reverse complement, with WO_RC when it is stored the other way round; or all ones
template <bool WIDE>
__device__ __forceinline__ uint32_t wo_find(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, int k,
                                            const uint32_t *__restrict__ index, int lg_cap, const Kmer &x)
{
    const Kmer r = rc_kmer(x, k);
    const uint64_t mask = (1ull << lg_cap) - 1;
    uint64_t s = wo_home<WIDE>(x, r, lg_cap);
    for (uint64_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {
        const uint32_t e = index[s];
        if (e == WO_NONE) return WO_NONE;
        const Kmer u = wo_entry<WIDE>(hi, lo, e, k);
        if (wo_same<WIDE>(u, x)) return e;  // (a palindrome is found here: no bit)
        if (wo_same<WIDE>(u, r)) return e | WO_RC;
    }
    return WO_NONE;
}

// adj: eight words a member
template <bool WIDE>
__global__ void __launch_bounds__(WO_THREADS) k_wo_adj(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint32_t n, int k,
                                                       const uint32_t *__restrict__ index, int lg_cap, const uint64_t *__restrict__ comp_off,
                                                       uint32_t n_comp, uint4 *__restrict__ adj)
{
    const uint32_t i = blockIdx.x * WO_THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t c = 0, c_hi = n_comp;  // the greatest c with comp_off[c] <= i
    while (c_hi - c > 1) {
        const uint32_t mid = c + (c_hi - c) / 2;
        if (comp_off[mid] <= i) c = mid; else c_hi = mid;
    }
    const uint32_t a = (uint32_t)comp_off[c], b = (uint32_t)comp_off[c + 1];
    const Kmer v = wo_entry<WIDE>(hi, lo, i, k);
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t t = wo_find<WIDE>(hi, lo, k, index, lg_cap, neighbour(v, k, 0, j));
        const uint32_t m = t & ~WO_RC;
        w[j] = t != WO_NONE && m >= a && m < b ? t : WO_NONE;  // (another component's k-mer is no neighbour)
    }
    adj[2 * (uint64_t)i] = make_uint4(w[0], w[1], w[2], w[3]);
    adj[2 * (uint64_t)i + 1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// first: all ones, cnt: zero when the launch starts
__global__ void __launch_bounds__(WO_THREADS) k_wo_init(const uint64_t *__restrict__ comp_off, uint32_t n_comp, uint32_t *__restrict__ first,
                                                        uint8_t *__restrict__ cnt, uint32_t *__restrict__ queue, uint32_t *__restrict__ order,
                                                        WoLevel *__restrict__ level)
{
    const uint32_t c = blockIdx.x * WO_THREADS + threadIdx.x;
    if (c >= n_comp) return;
    const uint64_t a = comp_off[c];
    first[a] = 0;
    cnt[a] = 1;
    queue[2 * a] = (uint32_t)a;
    order[a] = 0;
    level[c] = WoLevel{0, 1, 1, 0};
}

// the eight neighbours of an entry in slot order
__device__ __forceinline__ void wo_neighbours(const uint4 *__restrict__ adj, uint32_t ent, uint32_t (&w)[8])
{
    const uint32_t m = ent & ~WO_RC;
    const uint4 x = adj[2 * (uint64_t)m], y = adj[2 * (uint64_t)m + 1];
    const uint32_t raw[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
    const bool rc = ent & WO_RC;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t back = raw[7 - j];  // (the left neighbour by c of rc(v) is the reverse complement of v's right one by 3 - c)
        w[j] = rc ? (back == WO_NONE ? WO_NONE : back ^ WO_RC) : raw[j];
    }
}

// a workgroup's exclusive scan of one word a thread (two 16-bit counts in it); *total: the sum
__device__ __forceinline__ uint32_t wo_block_scan(uint32_t v, uint32_t *wave_sum, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d);
        if (lane >= (uint32_t)d) inc += up;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t x = 0; x < WO_THREADS / 64; x++) {
        const uint32_t ws = wave_sum[x];
        if (x < wave) before += ws;
        all += ws;
    }
    __syncthreads();  // (wave_sum is free again)
    *total = all;
    return before + inc - v;
}

// The eight tests of a candidate mask are lane masks in scalar registers; re-made from the vector register in every phase of a level
// instead of kept across its barriers, they fit without scalar spills.
#define WO_FROM_VGPR(x) asm volatile("" : "+v"(x))

// work: n_work components; ctr: [0] the next place of work, [1] the places of wide that are taken; levels: summed over the launch
__global__ void __launch_bounds__(WO_THREADS) k_wo_narrow(const uint4 *__restrict__ adj, const uint64_t *__restrict__ comp_off, uint32_t *first,
                                                          uint8_t *cnt, uint32_t *queue, uint32_t *order, WoLevel *level,
                                                          const uint32_t *__restrict__ work, uint32_t n_work, uint32_t *ctr, uint32_t *wide,
                                                          unsigned long long *levels, uint32_t w_max)
{
    __shared__ uint32_t h_key[WO_SLOTS], h_m1[WO_SLOTS], h_m2[WO_SLOTS];
    __shared__ uint32_t wave_sum[WO_THREADS / 64];
    __shared__ uint32_t s_item;
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < WO_SLOTS; i += WO_THREADS) { h_key[i] = WO_NONE; h_m1[i] = WO_NONE; h_m2[i] = WO_NONE; }
    for (;;) {
        __syncthreads();
        if (tid == 0) s_item = atomicAdd(ctr, 1u);
        __syncthreads();
        const uint32_t item = s_item;
        if (item >= n_work) return;
        const uint32_t c = work[item];
        const uint64_t a = comp_off[c];
        const uint32_t room_q = 2 * (uint32_t)(comp_off[c + 1] - a);  // the component's part of queue
        uint32_t *q = queue + 2 * a;
        const WoLevel lv = level[c];
        uint32_t s = lv.s, e = lv.e, nf = lv.nf, done = 0;
        while (e > s && e - s <= w_max) {
            const uint32_t p = s + tid;
            uint32_t t[8], slot[8], cand = 0;
            if (p < e) {
                wo_neighbours(adj, q[p], t);
#pragma unroll
                for (int j = 0; j < 8; j++)
                    if (t[j] != WO_NONE && first[t[j] & ~WO_RC] >= p) cand |= 1u << j;
            }
#pragma unroll
            for (int j = 0; j < 8; j++) {
                slot[j] = 0;
                if (!(cand >> j & 1)) continue;
                const uint32_t m = t[j] & ~WO_RC;
                uint32_t h = (m * 0x9e3779b1u) >> (32 - WO_SLOT_BITS);
                for (uint32_t probe = 0; probe < WO_SLOTS; probe++, h = (h + 1) & (WO_SLOTS - 1)) {  // (at most half full)
                    const uint32_t was = atomicCAS(&h_key[h], WO_NONE, m);
                    if (was == WO_NONE || was == m) break;
                }
                slot[j] = h;
                atomicMin(&h_m1[h], tid * 8 + j);
            }
            __syncthreads();
            WO_FROM_VGPR(cand);
#pragma unroll
            for (int j = 0; j < 8; j++)
                if ((cand >> j & 1) && h_m1[slot[j]] != tid * 8 + j) atomicMin(&h_m2[slot[j]], tid * 8 + j);
            __syncthreads();
            WO_FROM_VGPR(cand);
            // keep: the candidate stays; lead: it is its target's smallest key and stays (it writes first[] and cnt[]);
            // fresh: the target had no entry; pair: the second smallest stays too
            uint32_t keep = 0, lead = 0, fresh = 0, pair = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (!(cand >> j & 1)) continue;
                const uint32_t key = tid * 8 + j, m1 = h_m1[slot[j]], m2 = h_m2[slot[j]];
                const uint32_t had = cnt[t[j] & ~WO_RC];
                if (key == m1 && had < 2) {
                    keep |= 1u << j;
                    lead |= 1u << j;
                    if (had == 0) fresh |= 1u << j;
                    if (had == 0 && m2 != WO_NONE) pair |= 1u << j;
                } else if (key == m2 && had == 0) keep |= 1u << j;
            }
            uint32_t total;
            uint32_t at = wo_block_scan(__popc(keep) | (__popc(fresh) << 16), wave_sum, &total);  // (its barriers: every cnt[] and min is read)
            uint32_t at_q = e + (at & 0xffff), at_o = nf + (at >> 16);
            WO_FROM_VGPR(cand);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (!(cand >> j & 1)) continue;
                h_key[slot[j]] = WO_NONE;  // (every candidate of a target writes the same)
                h_m1[slot[j]] = WO_NONE;
                h_m2[slot[j]] = WO_NONE;
                if (!(keep >> j & 1)) continue;
                const uint32_t m = t[j] & ~WO_RC;
                if (at_q < room_q) q[at_q] = t[j];  // (always: a member has at most two entries)
                if (lead >> j & 1) {
                    cnt[m] = (uint8_t)((fresh >> j & 1 ? 1 : 2) + (pair >> j & 1));
                    if (fresh >> j & 1) {
                        first[m] = at_q;
                        order[a + at_o++] = m - (uint32_t)a;
                    }
                }
                at_q++;
            }
            s = e;
            e += total & 0xffff;
            nf += total >> 16;
            done++;
            __syncthreads();  // (the next level reads q, first[], cnt[] and the table)
        }
        if (tid == 0) {
            level[c] = WoLevel{s, e, nf, 0};
            if (e > s) wide[atomicAdd(ctr + 1, 1u)] = c;
            atomicAdd(levels, (unsigned long long)done);
        }
    }
}

// ------------------------------------------------------------------ one level of one component across the grid

// PASS 1: min1[t] = the smallest key; PASS 2: min2[t] = the smallest of the others.  q, first, min1, min2: the component's own parts
// are reached through member numbers of the whole call; q is the component's queue.
template <int PASS>
__global__ void __launch_bounds__(WO_THREADS) k_wo_min(const uint4 *__restrict__ adj, const uint32_t *__restrict__ first, const uint32_t *__restrict__ q,
                                                       uint32_t s, uint32_t n_level, unsigned long long *min1, unsigned long long *min2)
{
    const uint32_t i = blockIdx.x * WO_THREADS + threadIdx.x;
    if (i >= n_level) return;
    const uint32_t p = s + i;
    uint32_t t[8];
    wo_neighbours(adj, q[p], t);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (t[j] == WO_NONE) continue;
        const uint32_t m = t[j] & ~WO_RC;
        if (first[m] < p) continue;
        const unsigned long long key = 8ull * i + j;
        if (PASS == 1) atomicMin(min1 + m, key);
        else if (__hip_atomic_load(min1 + m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != key) atomicMin(min2 + m, key);
    }
}

// mask: a word an entry of the level (keep, lead, fresh, pair: a byte each); sums: a word a block (kept | fresh << 32)
__global__ void __launch_bounds__(WO_THREADS) k_wo_keep(const uint4 *__restrict__ adj, const uint32_t *__restrict__ first, const uint8_t *__restrict__ cnt,
                                                        const uint32_t *__restrict__ q, uint32_t s, uint32_t n_level,
                                                        const unsigned long long *__restrict__ min1, const unsigned long long *__restrict__ min2,
                                                        uint32_t *__restrict__ mask, unsigned long long *__restrict__ sums)
{
    __shared__ uint32_t wave_sum[WO_THREADS / 64];
    const uint32_t i = blockIdx.x * WO_THREADS + threadIdx.x;
    uint32_t keep = 0, lead = 0, fresh = 0, pair = 0;
    if (i < n_level) {
        const uint32_t p = s + i;
        uint32_t t[8];
        wo_neighbours(adj, q[p], t);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (t[j] == WO_NONE) continue;
            const uint32_t m = t[j] & ~WO_RC;
            if (first[m] < p) continue;
            const unsigned long long key = 8ull * i + j, m1 = min1[m], m2 = min2[m];
            const uint32_t had = cnt[m];
            if (key == m1 && had < 2) {
                keep |= 1u << j;
                lead |= 1u << j;
                if (had == 0) fresh |= 1u << j;
                if (had == 0 && m2 != WO_NOKEY) pair |= 1u << j;
            } else if (key == m2 && had == 0) keep |= 1u << j;
        }
        mask[i] = keep | (lead << 8) | (fresh << 16) | (pair << 24);
    }
    uint32_t total;
    wo_block_scan(__popc(keep) | (__popc(fresh) << 16), wave_sum, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = (unsigned long long)(total & 0xffff) | ((unsigned long long)(total >> 16) << 32);
}

// the level's kept candidates to their places; min1 / min2 of every neighbour back to all ones; the last block: the component's new level
__global__ void __launch_bounds__(WO_THREADS) k_wo_scatter(const uint4 *__restrict__ adj, uint32_t *__restrict__ first, uint8_t *__restrict__ cnt,
                                                           uint32_t *__restrict__ q, uint32_t room_q, uint32_t *__restrict__ order, uint32_t a,
                                                           WoLevel was, const uint32_t *__restrict__ mask, const unsigned long long *__restrict__ sums,
                                                           unsigned long long *__restrict__ min1, unsigned long long *__restrict__ min2,
                                                           WoLevel *__restrict__ level)
{
    __shared__ uint32_t wave_sum[WO_THREADS / 64];
    __shared__ unsigned long long part[WO_THREADS / 64];
    const uint32_t tid = threadIdx.x, i = blockIdx.x * WO_THREADS + tid, n_level = was.e - was.s;
    unsigned long long front = 0;  // the sums of the blocks in front
    for (uint32_t b = tid; b < blockIdx.x; b += WO_THREADS) front += sums[b];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) front += __shfl_xor(front, d);
    if ((tid & 63) == 0) part[tid >> 6] = front;
    __syncthreads();
    front = 0;
#pragma unroll
    for (uint32_t x = 0; x < WO_THREADS / 64; x++) front += part[x];
    const uint32_t mk = i < n_level ? mask[i] : 0;
    const uint32_t keep = mk & 0xff, lead = mk >> 8 & 0xff, fresh = mk >> 16 & 0xff, pair = mk >> 24;
    uint32_t total;
    const uint32_t at = wo_block_scan(__popc(keep) | (__popc(fresh) << 16), wave_sum, &total);
    if (i < n_level) {
        uint32_t at_q = was.e + (uint32_t)front + (at & 0xffff), at_o = was.nf + (uint32_t)(front >> 32) + (at >> 16);
        uint32_t t[8];
        wo_neighbours(adj, q[was.s + i], t);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (t[j] == WO_NONE) continue;
            const uint32_t m = t[j] & ~WO_RC;
            min1[m] = WO_NOKEY;  // (whoever has m as a neighbour writes the same)
            min2[m] = WO_NOKEY;
            if (!(keep >> j & 1)) continue;
            if (at_q < room_q) q[at_q] = t[j];  // (always: a member has at most two entries)
            if (lead >> j & 1) {
                cnt[m] = (uint8_t)((fresh >> j & 1 ? 1 : 2) + (pair >> j & 1));
                if (fresh >> j & 1) {
                    first[m] = at_q;
                    order[a + at_o++] = m - a;
                }
            }
            at_q++;
        }
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0)
        *level = WoLevel{was.e, was.e + (uint32_t)front + (total & 0xffff), was.nf + (uint32_t)(front >> 32) + (total >> 16), 0};
}

__global__ void __launch_bounds__(WO_THREADS) k_wo_twice(const uint8_t *__restrict__ cnt, uint32_t n, uint8_t *__restrict__ twice)
{
    const uint32_t i = blockIdx.x * WO_THREADS + threadIdx.x;
    if (i < n) twice[i] = cnt[i] >= 2;
}

constexpr char API[] = "mc_walk_order";

uint32_t blocks(uint64_t n) { return (uint32_t)((n + WO_THREADS - 1) / WO_THREADS); }

template <class T>
T *host_array(uint64_t n) { return static_cast<T *>(calloc(std::max<uint64_t>(n, 1), sizeof(T))); }

template <bool WIDE>
int run_walk_order(mc_ctx *c, const uint64_t *d_hi, const uint64_t *d_lo, const uint64_t *d_off, const std::vector<uint64_t> &off, uint32_t flags,
                   mc_walk_order_result *out)
{
    const int k = c->cfg.k;
    hipStream_t st = c->stream;
    const uint32_t n_comp = (uint32_t)(off.size() - 1), n = (uint32_t)off.back();
    const uint32_t w_max = (flags & MC_WALK_ORDER_WIDE_ONLY) ? 0 : (flags & MC_WALK_ORDER_NARROW_8) ? 8 : WO_W;
    int lg_cap = 6;
    while ((1ull << lg_cap) < 2 * (uint64_t)n) lg_cap++;  // (at most 31: n < 2^30)
    const uint64_t cap = 1ull << lg_cap;
    const dim3 gn(blocks(n)), gc(blocks(n_comp)), bt(WO_THREADS);
    DevBuf<uint32_t> index, first, queue, order, work, wide, ctr, mask;
    DevBuf<uint4> adj;
    DevBuf<uint8_t> cnt, twice;
    DevBuf<WoLevel> level;
    DevBuf<unsigned long long> levels, min1, min2, sums;
    HIPCHK(c, index.alloc(cap));
    HIPCHK(c, ctr.alloc(2));
    HIPCHK(c, adj.alloc(2ull * n));
    uint32_t *h_word = reinterpret_cast<uint32_t *>(c->h_scratch);

    HIPCHK(c, hipEventRecord(c->ev0, st));
    HIPCHK(c, hipMemsetAsync(index.p, 0xff, cap * 4, st));
    HIPCHK(c, hipMemsetAsync(ctr.p, 0, 8, st));
    hipLaunchKernelGGL(k_wo_build<WIDE>, gn, bt, 0, st, d_hi, d_lo, n, k, index.p, lg_cap, ctr.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_word, ctr.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (*h_word) return fail(c, MC_EINVAL, "%s: two members are the same k-mer or each other's reverse complement", API);
    hipLaunchKernelGGL(k_wo_adj<WIDE>, gn, bt, 0, st, d_hi, d_lo, n, k, index.p, lg_cap, d_off, n_comp, adj.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    index.reset();  // (the walk reads the adjacency alone)

    HIPCHK(c, first.alloc(n));
    HIPCHK(c, cnt.alloc(n));
    HIPCHK(c, twice.alloc(n));
    HIPCHK(c, queue.alloc(2ull * n));
    HIPCHK(c, order.alloc(n));
    HIPCHK(c, level.alloc(n_comp));
    HIPCHK(c, work.alloc(n_comp));
    HIPCHK(c, wide.alloc(n_comp));
    HIPCHK(c, levels.alloc(1));
    HIPCHK(c, hipMemsetAsync(first.p, 0xff, (uint64_t)n * 4, st));
    HIPCHK(c, hipMemsetAsync(cnt.p, 0, n, st));
    HIPCHK(c, hipMemsetAsync(order.p, 0, (uint64_t)n * 4, st));
    HIPCHK(c, hipMemsetAsync(levels.p, 0, 8, st));
    hipLaunchKernelGGL(k_wo_init, gc, bt, 0, st, d_off, n_comp, first.p, cnt.p, queue.p, order.p, level.p);
    HIPCHK(c, hipGetLastError());

    // every component is narrow at its seed; from then on the two paths hand the components to each other
    std::vector<uint32_t> todo(n_comp), wide_now;
    for (uint32_t i = 0; i < n_comp; i++) todo[i] = i;
    if (w_max == 0) wide_now.swap(todo);
    uint64_t wide_levels = 0, mask_cap = 0, sums_cap = 0;
    while (!todo.empty() || !wide_now.empty()) {
        if (!todo.empty()) {
            HIPCHK(c, hipMemcpyAsync(work.p, todo.data(), todo.size() * 4, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemsetAsync(ctr.p, 0, 8, st));
            const uint32_t grid = (uint32_t)std::min<uint64_t>(todo.size(), 256 * 3);  // (three workgroups' LDS fit a CU)
            hipLaunchKernelGGL(k_wo_narrow, dim3(grid), bt, 0, st, adj.p, d_off, first.p, cnt.p, queue.p, order.p, level.p, work.p, (uint32_t)todo.size(),
                               ctr.p, wide.p, levels.p, w_max);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(h_word, ctr.p + 1, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));  // (todo has gone up)
            wide_now.resize(*h_word);
            if (!wide_now.empty()) HIPCHK(c, hipMemcpy(wide_now.data(), wide.p, wide_now.size() * 4, hipMemcpyDeviceToHost));
            std::sort(wide_now.begin(), wide_now.end());
            todo.clear();
        }
        for (const uint32_t comp : wide_now) {
            if (!min1.p) {
                HIPCHK(c, min1.alloc(n));
                HIPCHK(c, min2.alloc(n));
                HIPCHK(c, hipMemsetAsync(min1.p, 0xff, (uint64_t)n * 8, st));
                HIPCHK(c, hipMemsetAsync(min2.p, 0xff, (uint64_t)n * 8, st));
            }
            const uint32_t a = (uint32_t)off[comp], room_q = 2 * (uint32_t)(off[comp + 1] - off[comp]);
            WoLevel *h_level = reinterpret_cast<WoLevel *>(c->h_scratch);
            HIPCHK(c, hipMemcpyAsync(h_level, level.p + comp, sizeof(WoLevel), hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            WoLevel lv = *h_level;
            while (lv.e > lv.s && lv.e - lv.s > w_max) {
                const uint32_t n_level = lv.e - lv.s, n_blocks = blocks(n_level);
                if (n_level > mask_cap) {
                    mask_cap = std::max<uint64_t>(n_level, 2 * mask_cap);
                    HIPCHK(c, mask.alloc(mask_cap));
                }
                if (n_blocks > sums_cap) {
                    sums_cap = std::max<uint64_t>(n_blocks, 2 * sums_cap);
                    HIPCHK(c, sums.alloc(sums_cap));
                }
                uint32_t *q = queue.p + 2ull * a;
                const dim3 gl(n_blocks);
                hipLaunchKernelGGL(k_wo_min<1>, gl, bt, 0, st, adj.p, first.p, q, lv.s, n_level, min1.p, min2.p);
                hipLaunchKernelGGL(k_wo_min<2>, gl, bt, 0, st, adj.p, first.p, q, lv.s, n_level, min1.p, min2.p);
                hipLaunchKernelGGL(k_wo_keep, gl, bt, 0, st, adj.p, first.p, cnt.p, q, lv.s, n_level, min1.p, min2.p, mask.p, sums.p);
                hipLaunchKernelGGL(k_wo_scatter, gl, bt, 0, st, adj.p, first.p, cnt.p, q, room_q, order.p, a, lv, mask.p, sums.p, min1.p, min2.p,
                                   level.p + comp);
                HIPCHK(c, hipGetLastError());
                HIPCHK(c, hipMemcpyAsync(h_level, level.p + comp, sizeof(WoLevel), hipMemcpyDeviceToHost, st));
                HIPCHK(c, hipStreamSynchronize(st));
                lv = *h_level;
                wide_levels++;
            }
            if (lv.e > lv.s) todo.push_back(comp);
        }
        wide_now.clear();
    }
    hipLaunchKernelGGL(k_wo_twice, gn, bt, 0, st, cnt.p, n, twice.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev1, st));
    HIPCHK(c, hipStreamSynchronize(st));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));

    out->n_components = n_comp;
    out->n_kmers = n;
    out->reached = host_array<uint64_t>(n_comp);
    out->order = host_array<uint32_t>(n);
    out->twice = host_array<uint8_t>(n);
    if (!out->reached || !out->order || !out->twice) return fail(c, MC_ENOMEM, "%s: no host memory", API);
    std::vector<WoLevel> lv(n_comp);
    unsigned long long n_levels = 0;
    HIPCHK(c, hipMemcpy(lv.data(), level.p, (uint64_t)n_comp * sizeof(WoLevel), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&n_levels, levels.p, 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out->order, order.p, (uint64_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out->twice, twice.p, n, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n_comp; i++) {
        out->reached[i] = lv[i].nf;
        out->queue_entries += lv[i].e;
    }
    out->levels = n_levels + wide_levels;
    out->wide_levels = wide_levels;
    out->device_ms = ms;
    return MC_OK;
}

}  // namespace

void mc_walk_order_free(mc_walk_order_result *r)
{
    if (!r) return;
    free(r->reached); free(r->order); free(r->twice);
    *r = mc_walk_order_result{};
}

int mc_walk_order_dev(mc_ctx *c, const uint64_t *d_hi, const uint64_t *d_lo, const uint64_t *d_comp_offsets, uint64_t n_components, uint32_t flags,
                      mc_walk_order_result *out)
{
    if (!c) return MC_EINVAL;
    static_assert(WO_WIDE_K == 33, "one word holds 32 bases");
    static_assert(8 * WO_W <= WO_SLOTS / 2 && (1u << WO_SLOT_BITS) == WO_SLOTS && WO_W <= WO_THREADS, "the LDS table holds a level's candidates half full");
    std::lock_guard<std::mutex> g(c->mu);
    if (!out) return fail(c, MC_EINVAL, "%s: null pointer", API);
    *out = mc_walk_order_result{};
    const bool wide = c->cfg.k >= WO_WIDE_K;
    if (flags & ~(MC_WALK_ORDER_WIDE_ONLY | MC_WALK_ORDER_NARROW_8)) return fail(c, MC_EINVAL, "%s: flags %u", API, flags);
    if (n_components >= (1ull << 30)) return fail(c, MC_EINVAL, "%s: %llu components (fewer than 2^30 k-mers)", API, (unsigned long long)n_components);
    if (n_components == 0) return MC_OK;
    if (!d_lo || !d_comp_offsets || (wide && !d_hi)) return fail(c, MC_EINVAL, "%s: null pointer", API);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    std::vector<uint64_t> off(n_components + 1);
    HIPCHK(c, hipMemcpy(off.data(), d_comp_offsets, (n_components + 1) * 8, hipMemcpyDeviceToHost));
    if (off.back() >= (1ull << 30)) return fail(c, MC_EINVAL, "%s: %llu k-mers (fewer than 2^30)", API, (unsigned long long)off.back());
    if (off[0] != 0) return fail(c, MC_EINVAL, "%s: comp_offsets starts at %llu", API, (unsigned long long)off[0]);
    for (uint64_t i = 0; i < n_components; i++)
        if (off[i + 1] <= off[i] || off[i + 1] > off.back())
            return fail(c, MC_EINVAL, "%s: comp_offsets[%llu] = %llu, then %llu (ascending strictly up to the number of k-mers)", API, (unsigned long long)i,
                        (unsigned long long)off[i], (unsigned long long)off[i + 1]);
    const int rc = wide ? run_walk_order<true>(c, d_hi, d_lo, d_comp_offsets, off, flags, out) : run_walk_order<false>(c, d_hi, d_lo, d_comp_offsets, off, flags, out);
    if (rc) mc_walk_order_free(out);
    return rc;
}

int mc_walk_order(mc_ctx *c, const uint64_t *hi, const uint64_t *lo, const uint64_t *comp_offsets, uint64_t n_components, uint32_t flags,
                  mc_walk_order_result *out)
{
    if (!c) return MC_EINVAL;
    const bool wide = c->cfg.k >= WO_WIDE_K;
    // (nothing to copy, or nothing that may be read: the device form says what is wrong)
    if (!out || n_components == 0 || n_components >= (1ull << 30) || (flags & ~(MC_WALK_ORDER_WIDE_ONLY | MC_WALK_ORDER_NARROW_8)) || !lo || !comp_offsets ||
        (wide && !hi))
        return mc_walk_order_dev(c, nullptr, nullptr, nullptr, n_components, flags, out);
    *out = mc_walk_order_result{};
    const uint64_t n = comp_offsets[n_components];
    bool ok = comp_offsets[0] == 0 && n < (1ull << 30);
    for (uint64_t i = 0; ok && i < n_components; i++) ok = comp_offsets[i + 1] > comp_offsets[i] && comp_offsets[i + 1] <= n;
    HostStage st(c);
    const uint64_t *doff = st.in(comp_offsets, n_components + 1);
    if (!ok) {  // (hi and lo are not read: the device form names the fault in comp_offsets)
        if (int rc = st.staged()) return rc;
        return mc_walk_order_dev(c, reinterpret_cast<const uint64_t *>(doff), reinterpret_cast<const uint64_t *>(doff), doff, n_components, flags, out);
    }
    const uint64_t *dhi = wide ? st.in(hi, n) : nullptr, *dlo = st.in(lo, n);
    if (int rc = st.staged()) return rc;
    return mc_walk_order_dev(c, dhi, dlo, doff, n_components, flags, out);
}
