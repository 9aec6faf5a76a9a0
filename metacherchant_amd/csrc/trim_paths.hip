// libmcgpu.so, the trim unit: which k-mers of one BFS pass runTrimPaths keeps (include/mcgpu.h mc_trim_paths*;
// src/algo/OneSequenceCalculator.java:241-262, which csrc/host/envfinder.cpp Environment::add_pass restates as a reverse walk).
// context.h lists the other units.
//
// kept[i] = 1 iff entry i reaches a `last` entry through steps inside the set: right neighbours for dir = +1, left ones for
// dir = -1, all eight for dir = 0.  The answer is a set, so nothing below depends on the order in which threads run.
//
// The index.  An open-addressing table of 2^lg_cap >= 2n words (at least 64), linear probing.  A slot holds an ENTRY NUMBER
// (all ones: free), and a probe compares through hi / lo: the k-mers are oriented, and an oriented k-mer can be any word, all
// ones included (T^32 at k = 32), so no word of a k-mer can mark a free slot as kmer_set.h's canonical keys do.  kmer_set.h lends
// its hash, given the oriented words.
//   k_tp_build    an entry claims the first free slot of its probe sequence; a slot that holds an entry with the same k-mer raises
//                 the duplicate flag.
// dir = +1 / -1 (successors = the up to four neighbours on that side that are entries):
//   k_tp_succ     the four look-ups of an entry, succ[c * n + i]; and its first state: KEPT when it is `last`, else OPEN.
//   k_tp_classify an OPEN entry looks at the stops of its successors (a PASS successor's stop is where its pointer rests, any other
//                 successor is its own stop): a KEPT stop makes it KEPT; DEAD stops, unrested PASS stops (closed cycles of entries
//                 with one way on) and itself are ways that lead nowhere and are dropped; of what is left, none makes it DEAD,
//                 one stop (by however many arms: arms that rejoin count once) makes it PASS pointing there, two or more leave it OPEN.
//                 States are read from one buffer and written to the other.
//   k_tp_jump     pointer jumping of the PASS entries over ceil(log2 n) rounds, two buffers in turn as k_ut_jump does: a pointer
//                 then rests on a stop that is not PASS, or the entry is on or leads into a closed cycle of PASS entries.
//   classify and jump alternate ("a phase") until a classify changes nothing: what is still OPEN then has every way on ending in
//   OPEN entries or cycles, and is not kept.
//   k_tp_kept     KEPT, or PASS resting on KEPT.
// dir = 0 (the relation is symmetric: kept iff the connected component holds a `last`):
//   k_tp_unite    an entry and each of its right neighbours in the set are united (the left ones are somebody's right ones):
//                 components.hip's lock-free union-find over entry numbers, parent[x] <= x, every access an agent-scope atomic.
//   k_tp_mark     a `last` entry marks its root;  k_tp_kept0  kept[i] = mark[root(i)].
//
// Launches and host round trips do not grow with the length of a path.  They grow with log2 n (the jump rounds of a phase) times the
// number of phases, one round trip a phase; a phase ends every fork whose arms but one are dead, every bubble, and every fork next
// to a KEPT stop, so the number of phases is the depth of what is left of the fork graph after that (2 for a chain, 3 for a chain
// with dead side arms or bubbles).  No workgroup waits for another; every loop is bounded by n (probes by the table's size, 4n at
// the most).
// Device memory per entry, beside the caller's arrays: the index 8 - 16 bytes; dir +-1: succ 16, two states 16 (48 at the most);
// dir 0: parent 4, mark 1.
// Code paths change at one constant: k <= 32 reads lo alone (hi may be NULL), k > 32 reads both words (TP_WIDE_K = 33).
// The kernels use no LDS and no scratch memory: tests/test_trim_paths_kernel_resources.py.
#include "context.h"
#include "kmer_set.h"

namespace {

constexpr int TP_THREADS = 256;
constexpr int TP_WIDE_K = 33;             // from this k on an entry is two words
constexpr uint32_t TP_NONE = ~0u;         // a free slot, no successor (entry numbers are below 2^31)
enum : uint32_t { TP_DEAD = 0, TP_KEPT = 1, TP_PASS = 2, TP_OPEN = 3 };

// an entry's state, one word: where its pointer rests (itself unless it is PASS) and its kind above
__device__ __forceinline__ uint64_t tp_state(uint32_t kind, uint32_t at) { return ((uint64_t)kind << 32) | at; }
__device__ __forceinline__ uint32_t tp_kind(uint64_t s) { return (uint32_t)(s >> 32); }

template <bool WIDE>
__device__ __forceinline__ Kmer tp_entry(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint64_t e, int k)
{
    Kmer v{WIDE ? hi[e] : 0, lo[e]};
    if (WIDE) v.hi &= ~0ull >> (128 - 2 * k);  // (bits above the k-mer are dropped, as ut_entry does)
    else if (k < 32) v.lo &= ~0ull >> (64 - 2 * k);
    return v;
}

template <bool WIDE>
__device__ __forceinline__ uint64_t tp_home(const Kmer &v, int lg_cap)
{
    return rs_home(rs_hash<WIDE>(RsKey{v.lo, v.hi}), lg_cap);
}

template <bool WIDE>
__device__ __forceinline__ bool tp_same(const Kmer &a, const Kmer &b) { return a.lo == b.lo && (!WIDE || a.hi == b.hi); }

// index: 2^lg_cap words, all ones when the call starts
template <bool WIDE>
__global__ void __launch_bounds__(TP_THREADS) k_tp_build(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint32_t n, int k,
                                                         uint32_t *__restrict__ index, int lg_cap, uint32_t *__restrict__ dup)
{
    const uint32_t e = blockIdx.x * TP_THREADS + threadIdx.x;
    if (e >= n) return;
    const Kmer v = tp_entry<WIDE>(hi, lo, e, k);
    const uint64_t mask = (1ull << lg_cap) - 1;
    uint64_t s = tp_home<WIDE>(v, lg_cap);
    for (uint64_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {  // (at most half full: a free slot comes)
        const uint32_t was = atomicCAS(index + s, TP_NONE, e);
        if (was == TP_NONE) return;
        if (tp_same<WIDE>(tp_entry<WIDE>(hi, lo, was, k), v)) {
            atomicOr(dup, 1u);
            return;
        }
    }
}

// the entry that is k-mer x, or all ones
template <bool WIDE>
__device__ __forceinline__ uint32_t tp_find(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, int k,
                                            const uint32_t *__restrict__ index, int lg_cap, const Kmer &x)
{
    const uint64_t mask = (1ull << lg_cap) - 1;
    uint64_t s = tp_home<WIDE>(x, lg_cap);
    for (uint64_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {
        const uint32_t e = index[s];
        if (e == TP_NONE) return TP_NONE;
        if (tp_same<WIDE>(tp_entry<WIDE>(hi, lo, e, k), x)) return e;
    }
    return TP_NONE;
}

// StringUtils' neighbour of v with base c: on the right ((v << 2) & mask) | c, on the left (c << 2(k - 1)) | (v >> 2)
template <bool WIDE, bool RIGHT>
__device__ __forceinline__ Kmer tp_neighbour(const Kmer &v, int k, uint64_t c)
{
    Kmer s;
    if (RIGHT) {
        s.hi = WIDE ? ((v.hi << 2) | (v.lo >> 62)) & (~0ull >> (128 - 2 * k)) : 0;
        s.lo = ((v.lo << 2) | c) & (WIDE || k >= 32 ? ~0ull : ~0ull >> (64 - 2 * k));
    } else {
        s.hi = WIDE ? (v.hi >> 2) | (c << (2 * (k - 1) - 64)) : 0;
        s.lo = WIDE ? (v.lo >> 2) | (v.hi << 62) : (v.lo >> 2) | (c << (2 * (k - 1)));
    }
    return s;
}

// succ: n words for each of the four bases; state: the first one
template <bool WIDE, bool RIGHT>
__global__ void __launch_bounds__(TP_THREADS) k_tp_succ(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, const uint8_t *__restrict__ last,
                                                        uint32_t n, int k, const uint32_t *__restrict__ index, int lg_cap,
                                                        uint32_t *__restrict__ succ, uint64_t *__restrict__ state)
{
    const uint32_t i = blockIdx.x * TP_THREADS + threadIdx.x;
    if (i >= n) return;
    const Kmer v = tp_entry<WIDE>(hi, lo, i, k);
#pragma unroll
    for (uint32_t c = 0; c < 4; c++)
        succ[(uint64_t)c * n + i] = tp_find<WIDE>(hi, lo, k, index, lg_cap, tp_neighbour<WIDE, RIGHT>(v, k, c));
    state[i] = tp_state(last[i] ? TP_KEPT : TP_OPEN, i);
}

// changed: bit 0 an entry left OPEN, bit 1 it became PASS (only then is there anything to jump)
__global__ void __launch_bounds__(TP_THREADS) k_tp_classify(uint32_t n, const uint32_t *__restrict__ succ, const uint64_t *__restrict__ from,
                                                            uint64_t *__restrict__ to, uint32_t *__restrict__ changed)
{
    const uint32_t i = blockIdx.x * TP_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = from[i];
    if (tp_kind(s) != TP_OPEN) {
        to[i] = s;
        return;
    }
    bool kept = false;
    uint32_t a = TP_NONE, b = TP_NONE;  // two different OPEN stops, as far as there are
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) {
        const uint32_t j = succ[(uint64_t)c * n + i];
        if (j == TP_NONE) continue;
        const uint64_t sj = from[j];
        const uint32_t t = tp_kind(sj) == TP_PASS ? (uint32_t)sj : j;
        const uint32_t kt = tp_kind(t == j ? sj : from[t]);
        if (kt == TP_KEPT) kept = true;
        else if (kt == TP_OPEN && t != i) {
            if (a == TP_NONE || a == t) a = t;
            else b = t;
        }
    }
    const uint64_t now = kept ? tp_state(TP_KEPT, i) : a == TP_NONE ? tp_state(TP_DEAD, i) : b == TP_NONE ? tp_state(TP_PASS, a) : s;
    to[i] = now;
    if (now != s) atomicOr(changed, tp_kind(now) == TP_PASS ? 3u : 1u);
}

__global__ void __launch_bounds__(TP_THREADS) k_tp_jump(uint32_t n, const uint64_t *__restrict__ from, uint64_t *__restrict__ to)
{
    const uint32_t i = blockIdx.x * TP_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = from[i];
    uint64_t now = s;
    if (tp_kind(s) == TP_PASS) {
        const uint64_t t = from[(uint32_t)s];
        if (tp_kind(t) == TP_PASS) now = t;  // (the same kind, t's pointer)
    }
    to[i] = now;
}

__global__ void __launch_bounds__(TP_THREADS) k_tp_kept(uint32_t n, const uint64_t *__restrict__ state, uint8_t *__restrict__ kept)
{
    const uint32_t i = blockIdx.x * TP_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = state[i];
    const uint32_t kind = tp_kind(s);
    kept[i] = kind == TP_KEPT || (kind == TP_PASS && tp_kind(state[(uint32_t)s]) == TP_KEPT);
}

__device__ __forceinline__ uint32_t tp_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void tp_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x, halving the path on the way (components.hip cc_find); a path only descends, so it has fewer than n steps
__device__ __forceinline__ uint32_t tp_root(uint32_t *parent, uint32_t x, uint32_t n)
{
    uint32_t p = tp_load(parent + x);
    for (uint32_t step = 0; step < n && p != x; step++) {
        const uint32_t g = tp_load(parent + p);
        if (g != p) tp_store(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

// parent[i] = i when the launch starts
template <bool WIDE>
__global__ void __launch_bounds__(TP_THREADS) k_tp_unite(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint32_t n, int k,
                                                         const uint32_t *__restrict__ index, int lg_cap, uint32_t *__restrict__ parent)
{
    const uint32_t i = blockIdx.x * TP_THREADS + threadIdx.x;
    if (i >= n) return;
    const Kmer v = tp_entry<WIDE>(hi, lo, i, k);
    for (uint32_t c = 0; c < 4; c++) {
        const uint32_t j = tp_find<WIDE>(hi, lo, k, index, lg_cap, tp_neighbour<WIDE, true>(v, k, c));
        if (j == TP_NONE || j == i) continue;
        uint32_t a = i, b = j;
        for (uint32_t tries = 0; tries <= n; tries++) {  // (a failed hook means another one was made: fewer than n in all)
            a = tp_root(parent, a, n);
            b = tp_root(parent, b, n);
            if (a == b) break;
            if (a > b) { const uint32_t x = a; a = b; b = x; }
            if (atomicCAS(parent + b, b, a) == b) break;
        }
    }
}

// mark: zero when the launch starts
__global__ void __launch_bounds__(TP_THREADS) k_tp_mark(uint32_t n, const uint8_t *__restrict__ last, uint32_t *__restrict__ parent,
                                                        uint8_t *__restrict__ mark)
{
    const uint32_t i = blockIdx.x * TP_THREADS + threadIdx.x;
    if (i < n && last[i]) mark[tp_root(parent, i, n)] = 1;
}

__global__ void __launch_bounds__(TP_THREADS) k_tp_kept0(uint32_t n, uint32_t *__restrict__ parent, const uint8_t *__restrict__ mark,
                                                         uint8_t *__restrict__ kept)
{
    const uint32_t i = blockIdx.x * TP_THREADS + threadIdx.x;
    if (i < n) kept[i] = mark[tp_root(parent, i, n)];
}

__global__ void __launch_bounds__(TP_THREADS) k_tp_iota(uint32_t n, uint32_t *__restrict__ parent)
{
    const uint32_t i = blockIdx.x * TP_THREADS + threadIdx.x;
    if (i < n) parent[i] = i;
}

constexpr char API[] = "mc_trim_paths";

uint32_t blocks(uint64_t n) { return (uint32_t)((n + TP_THREADS - 1) / TP_THREADS); }

template <bool WIDE>
int run_trim(mc_ctx *c, const uint64_t *d_hi, const uint64_t *d_lo, const uint8_t *d_last, uint32_t n, int dir, uint8_t *d_kept, double *device_ms)
{
    const int k = c->cfg.k;
    hipStream_t st = c->stream;
    int lg_cap = 6;
    while ((1ull << lg_cap) < 2 * (uint64_t)n) lg_cap++;  // (at most 32: n < 2^31)
    const uint64_t cap = 1ull << lg_cap;
    const dim3 gn(blocks(n)), bt(TP_THREADS);
    DevBuf<uint32_t> index, flags, succ, parent;
    DevBuf<uint64_t> state_a, state_b;
    DevBuf<uint8_t> mark;
    HIPCHK(c, index.alloc(cap));
    HIPCHK(c, flags.alloc(1));
    uint32_t *h_flag = reinterpret_cast<uint32_t *>(c->h_scratch);

    HIPCHK(c, hipEventRecord(c->ev0, st));
    HIPCHK(c, hipMemsetAsync(index.p, 0xff, cap * 4, st));
    HIPCHK(c, hipMemsetAsync(flags.p, 0, 4, st));
    hipLaunchKernelGGL(k_tp_build<WIDE>, gn, bt, 0, st, d_hi, d_lo, n, k, index.p, lg_cap, flags.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_flag, flags.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (*h_flag) return fail(c, MC_EINVAL, "%s: two entries are the same oriented k-mer", API);

    if (dir == 0) {
        HIPCHK(c, parent.alloc(n));
        HIPCHK(c, mark.alloc(n));
        HIPCHK(c, hipMemsetAsync(mark.p, 0, n, st));
        hipLaunchKernelGGL(k_tp_iota, gn, bt, 0, st, n, parent.p);
        hipLaunchKernelGGL(k_tp_unite<WIDE>, gn, bt, 0, st, d_hi, d_lo, n, k, index.p, lg_cap, parent.p);
        hipLaunchKernelGGL(k_tp_mark, gn, bt, 0, st, n, d_last, parent.p, mark.p);
        hipLaunchKernelGGL(k_tp_kept0, gn, bt, 0, st, n, parent.p, mark.p, d_kept);
    } else {
        HIPCHK(c, succ.alloc(4ull * n));
        HIPCHK(c, state_a.alloc(n));
        HIPCHK(c, state_b.alloc(n));
        uint64_t *from = state_a.p, *to = state_b.p;
        if (dir > 0) hipLaunchKernelGGL((k_tp_succ<WIDE, true>), gn, bt, 0, st, d_hi, d_lo, d_last, n, k, index.p, lg_cap, succ.p, from);
        else hipLaunchKernelGGL((k_tp_succ<WIDE, false>), gn, bt, 0, st, d_hi, d_lo, d_last, n, k, index.p, lg_cap, succ.p, from);
        int rounds = 0;
        while ((1ull << rounds) < n) rounds++;
        for (uint64_t phase = 0; phase <= n; phase++) {  // (every phase but the last takes an entry out of OPEN)
            HIPCHK(c, hipMemsetAsync(flags.p, 0, 4, st));
            hipLaunchKernelGGL(k_tp_classify, gn, bt, 0, st, n, succ.p, from, to, flags.p);
            std::swap(from, to);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(h_flag, flags.p, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            if (!*h_flag) break;
            if (!(*h_flag & 2)) continue;
            for (int r = 0; r < rounds; r++) {
                hipLaunchKernelGGL(k_tp_jump, gn, bt, 0, st, n, from, to);
                std::swap(from, to);
            }
        }
        hipLaunchKernelGGL(k_tp_kept, gn, bt, 0, st, n, from, d_kept);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev1, st));
    HIPCHK(c, hipStreamSynchronize(st));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (device_ms) *device_ms = ms;
    return MC_OK;
}

}  // namespace

int mc_trim_paths_dev(mc_ctx *c, const uint64_t *d_hi, const uint64_t *d_lo, const uint8_t *d_last, uint64_t n, int dir, uint8_t *d_kept,
                      double *device_ms)
{
    if (!c) return MC_EINVAL;
    static_assert(TP_WIDE_K == 33, "one word holds 32 bases");
    std::lock_guard<std::mutex> g(c->mu);
    if (device_ms) *device_ms = 0;
    const bool wide = c->cfg.k >= TP_WIDE_K;
    if (dir < -1 || dir > 1) return fail(c, MC_EINVAL, "%s: dir %d (-1, 0 or +1)", API, dir);
    if (n >= (1ull << 31)) return fail(c, MC_EINVAL, "%s: %llu entries (at most 2^31 - 1)", API, (unsigned long long)n);
    if (n && (!d_lo || !d_last || !d_kept || (wide && !d_hi))) return fail(c, MC_EINVAL, "%s: null pointer", API);
    if (n == 0) return MC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return wide ? run_trim<true>(c, d_hi, d_lo, d_last, (uint32_t)n, dir, d_kept, device_ms)
                : run_trim<false>(c, d_hi, d_lo, d_last, (uint32_t)n, dir, d_kept, device_ms);
}

int mc_trim_paths(mc_ctx *c, const uint64_t *hi, const uint64_t *lo, const uint8_t *last, uint64_t n, int dir, uint8_t *kept, double *device_ms)
{
    if (!c) return MC_EINVAL;
    const bool wide = c->cfg.k >= TP_WIDE_K;
    if (n == 0 || n >= (1ull << 31) || dir < -1 || dir > 1 || !lo || !last || !kept || (wide && !hi))  // (nothing to copy: the device form says what is wrong)
        return mc_trim_paths_dev(c, nullptr, nullptr, nullptr, n, dir, nullptr, device_ms);
    HostStage st(c);
    const uint64_t *dhi = wide ? st.in(hi, n) : nullptr, *dlo = st.in(lo, n);
    const uint8_t *dlast = st.in(last, n);
    uint8_t *dkept = st.out<uint8_t>(n);
    if (int rc = st.staged()) return rc;
    if (int rc = mc_trim_paths_dev(c, dhi, dlo, dlast, n, dir, dkept, device_ms)) return rc;
    return st.back(kept, dkept, n);
}
