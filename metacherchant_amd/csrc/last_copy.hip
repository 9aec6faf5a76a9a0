// libmcgpu.so, the last-copy unit: for every read of a read set, the greatest index of a read with exactly the same bases
// (include/mcgpu.h mc_reads_last_copy*).  The triple-reads-classifier needs it: the reference keys its pass-1 verdicts by a read's
// bases (src/algo/TripleFinder.java:46-57, a Map<String, FindResult> whose last writer wins) and looks every read up by its bases
// in pass 2 (src/algo/TripleFinder2.java:60-76).  context.h lists the other units.
//
// Three steps a round, all on the context's stream:
//   k_lc_fingerprint  one wave a read: lanes take 32-base chunks at any bit alignment, mix each with its position, the wave
//                     sums them, and the length is folded in: a 64-bit fingerprint;
//   radix sort        (fingerprint, index) pairs, stably (hipCUB): equal fingerprints form runs, indices ascending within a run;
//   k_lc_resolve      one thread a sorted position: the run's end by a galloping search, then the read against the run's last
//                     member word by word.  Equal bases: that member is the answer.  Different bases (a fingerprint collision):
//                     the read stays open for the next round.
// Every read with the bases of its run's last member is resolved; every copy of an open read is open too (copies share every
// fingerprint, so they sat in the same run and differed from the same member), so the next round -- a fresh seed over the open
// reads only -- still sees all of them.  Each round closes at least the last member of every run: the loop ends, and no answer
// ever rests on a fingerprint alone.  DESIGN.md "Triple-reads-classifier" has the roofline.
#include "context.h"  // (first: hip_runtime.h picks hipCUB's backend)

#include <hipcub/device/device_radix_sort.hpp>
#include <hipcub/device/device_select.hpp>

namespace {

constexpr int LC_THREADS = 256;
constexpr uint32_t LC_OPEN = 0xffffffffu;  // last[r] of a read not resolved yet

__device__ __forceinline__ uint64_t mix64(uint64_t x)  // the finaliser of splitmix64
{
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// nb (1 .. 32) bases from base p on, left-aligned in 64 bits, the bits behind them zero
__device__ __forceinline__ uint64_t chunk_at(const uint64_t *__restrict__ words, uint64_t p, uint32_t nb)
{
    const uint64_t wi = p >> 5;
    const int off = 2 * (int)(p & 31);
    const uint64_t w0 = words[wi];
    const uint64_t a = off ? ((w0 << off) | (words[wi + 1] >> (64 - off))) : w0;  // (wi + 1 is at worst the pad word)
    return nb >= 32 ? a : a & ~(~0ull >> (2 * nb));
}

// reads active[i] (i < m; active == NULL: read i) -> fp[i], idx[i]
__global__ void __launch_bounds__(LC_THREADS) k_lc_fingerprint(const uint64_t *__restrict__ words, const uint64_t *__restrict__ offsets,
                                                               const uint32_t *__restrict__ active, uint32_t m, uint64_t seed, int weak,
                                                               uint64_t *__restrict__ fp, uint32_t *__restrict__ idx)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < m; i += n_waves) {
        const uint32_t r = active ? active[i] : (uint32_t)i;
        const uint64_t b = offsets[r], len = offsets[r + 1] - b;
        uint64_t h = 0;
        for (uint64_t c = lane; 32 * c < len; c += 64)
            h += mix64(chunk_at(words, b + 32 * c, (uint32_t)min(len - 32 * c, (uint64_t)32)) ^ mix64(seed + c + 1));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o);
        h = mix64(h ^ mix64(len ^ (seed << 32) ^ 0x5851f42d4c957f2dull));
        if (weak) h &= 15;  // (MC_LAST_COPY_WEAK_FP: 16 fingerprints in all, so distinct reads share them)
        if (lane == 0) {
            fp[i] = h;
            idx[i] = r;
        }
    }
}

__device__ bool same_bases(const uint64_t *__restrict__ words, const uint64_t *__restrict__ offsets, uint32_t r, uint32_t j)
{
    const uint64_t br = offsets[r], bj = offsets[j], len = offsets[r + 1] - br;
    if (offsets[j + 1] - bj != len) return false;
    for (uint64_t c = 0; c < len; c += 32) {
        const uint32_t nb = (uint32_t)min(len - c, (uint64_t)32);
        if (chunk_at(words, br + c, nb) != chunk_at(words, bj + c, nb)) return false;
    }
    return true;
}

// sorted position p: the end e of its run of equal fingerprints; last[idx[p]] = idx[e] when the bases agree.  *n_open counts the rest.
__global__ void __launch_bounds__(LC_THREADS) k_lc_resolve(const uint64_t *__restrict__ words, const uint64_t *__restrict__ offsets,
                                                           const uint64_t *__restrict__ fp, const uint32_t *__restrict__ idx, uint32_t m,
                                                           uint32_t *__restrict__ last, uint32_t *__restrict__ n_open)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < m; base += stride) {  // (whole waves a step: the ballot below)
        const uint64_t p = base + threadIdx.x;
        bool open = false;
        if (p < m) {
            const uint64_t f = fp[p];
            uint64_t lo = p, step = 1;  // fp[lo] == f throughout; gallop, then bisect (lo, hi)
            while (lo + step < m && fp[lo + step] == f) {
                lo += step;
                step <<= 1;
            }
            uint64_t hi = min(lo + step, (uint64_t)m);
            while (hi - lo > 1) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (fp[mid] == f) lo = mid;
                else hi = mid;
            }
            const uint32_t r = idx[p], j = idx[lo];
            if (lo == p || same_bases(words, offsets, r, j)) last[r] = j;
            else open = true;
        }
        const uint64_t b = __ballot(open);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_open, (uint32_t)__popcll(b));
    }
}

struct IsOpen {
    const uint32_t *last;
    __device__ bool operator()(uint32_t r) const { return last[r] == LC_OPEN; }
};

}  // namespace

int mc_reads_last_copy_dev(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_read_offsets, uint64_t n_reads, int flags, uint32_t *d_last)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (n_reads >= (1ull << 32)) return fail(c, MC_EINVAL, "mc_reads_last_copy: %llu reads (at most 2^32 - 1)", (unsigned long long)n_reads);
    if (n_reads && (!d_words || !d_read_offsets || !d_last)) return fail(c, MC_EINVAL, "mc_reads_last_copy: null pointer");
    if (n_reads == 0) return MC_OK;
    if (n_reads > (uint64_t)INT32_MAX) return fail(c, MC_EINVAL, "mc_reads_last_copy: %llu reads in one sort (at most 2^31 - 1)", (unsigned long long)n_reads);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const uint32_t n = (uint32_t)n_reads;
    DevBuf<uint64_t> fp, fp_s;
    DevBuf<uint32_t> idx, idx_s, active, counters;  // counters: the open reads of this round, the survivors of the selection
    HIPCHK(c, fp.alloc(n));
    HIPCHK(c, fp_s.alloc(n));
    HIPCHK(c, idx.alloc(n));
    HIPCHK(c, idx_s.alloc(n));
    HIPCHK(c, active.alloc(n));
    HIPCHK(c, counters.alloc(2));
    size_t sort_bytes = 0, select_bytes = 0;
    HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, fp.p, fp_s.p, idx.p, idx_s.p, (int)n, 0, 64, c->stream));
    HIPCHK(c, hipcub::DeviceSelect::If(nullptr, select_bytes, idx.p, active.p, counters.p + 1, (int)n, IsOpen{d_last}, c->stream));
    DevBuf<uint8_t> temp;
    HIPCHK(c, temp.alloc(std::max(sort_bytes, select_bytes)));
    HIPCHK(c, hipMemsetAsync(d_last, 0xff, (size_t)n * 4, c->stream));
    const bool weak = (flags & MC_LAST_COPY_WEAK_FP) != 0;
    uint32_t m = n;
    for (uint32_t round = 0; m > 0; round++) {
        const bool weak_round = weak && round == 0;  // (later rounds are full-width: they only ever see collisions)
        hipLaunchKernelGGL(k_lc_fingerprint, dim3(grid_for((uint64_t)m * 64, LC_THREADS, 1 << 18)), dim3(LC_THREADS), 0, c->stream, d_words,
                           d_read_offsets, round ? active.p : nullptr, m, 0x9e3779b97f4a7c15ull * (round + 1), weak_round ? 1 : 0, fp.p, idx.p);
        HIPCHK(c, hipGetLastError());
        size_t bytes = sort_bytes;
        HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(temp.p, bytes, fp.p, fp_s.p, idx.p, idx_s.p, (int)m, 0, weak_round ? 4 : 64, c->stream));
        HIPCHK(c, hipMemsetAsync(counters.p, 0, 4, c->stream));
        hipLaunchKernelGGL(k_lc_resolve, dim3(grid_for(m, LC_THREADS, 1 << 16)), dim3(LC_THREADS), 0, c->stream, d_words, d_read_offsets,
                           fp_s.p, idx_s.p, m, d_last, counters.p);
        HIPCHK(c, hipGetLastError());
        uint32_t n_open = 0;
        HIPCHK(c, hipMemcpyAsync(&n_open, counters.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (n_open == 0) break;
        // the open reads, in ascending order (idx holds this round's reads in the order they came, ascending), for the next round
        bytes = select_bytes;
        HIPCHK(c, hipcub::DeviceSelect::If(temp.p, bytes, idx.p, active.p, counters.p + 1, (int)m, IsOpen{d_last}, c->stream));
        HIPCHK(c, hipMemcpyAsync(&m, counters.p + 1, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return MC_OK;
}

int mc_reads_last_copy(mc_ctx *c, const uint64_t *words, const uint64_t *read_offsets, uint64_t n_reads, int flags, uint32_t *last)
{
    if (!c) return MC_EINVAL;
    if (n_reads >= (1ull << 32)) return fail(c, MC_EINVAL, "mc_reads_last_copy: %llu reads (at most 2^32 - 1)", (unsigned long long)n_reads);
    if (n_reads && (!words || !read_offsets || !last)) return fail(c, MC_EINVAL, "mc_reads_last_copy: null pointer");
    if (n_reads == 0) return MC_OK;
    HostStage st(c);
    const uint64_t *dw = st.in(words, packed_words(read_offsets, n_reads)), *doff = st.in(read_offsets, n_reads + 1);
    uint32_t *dlast = st.out<uint32_t>(n_reads);
    if (int rc = st.staged()) return rc;
    if (int rc = mc_reads_last_copy_dev(c, dw, doff, n_reads, flags, dlast)) return rc;
    return st.back(last, dlast, n_reads);
}
