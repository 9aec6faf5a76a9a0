// What the tokeniser's kernels share (csrc/tokenizer.h: the counting policy, csrc/whole_reads.hip: whole reads with their
// qualities): base codes, the workgroup scan, a wave's line spans, the FASTQ record of a wave and the WavePacker.  Device
// functions only -- every kernel stays in the one unit that launches it.
#pragma once
#include "device_types.h"

namespace mc {
namespace tok {

constexpr uint32_t SCAN_TILE = 4096;                    // elements per workgroup of the generic scan
enum { TOK_BAD_CHAR = 1, TOK_BAD_STRUCTURE = 2, TOK_BAD_QUALITY = 4 };

__device__ __forceinline__ int base_code(uint8_t c)
{   // A0 G1 C2 T3 (itmo!/dna/DnaTools.java:31), either case; -1: not a base
    switch (c | 0x20) {
    case 'a': return 0;
    case 'g': return 1;
    case 'c': return 2;
    case 't': return 3;
    default: return -1;
    }
}

// ---- a scan of 32-bit counts into 64-bit offsets: tile sums, one workgroup over the sums, tiles again
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *lds_wave, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if ((int)lane >= o) x += y;
    }
    if (lane == 63) lds_wave[wv] = x;
    __syncthreads();
    uint32_t before = 0, tot = 0;
    for (uint32_t i = 0; i < nw; i++) {
        const uint32_t c = lds_wave[i];
        if (i < wv) before += c;
        tot += c;
    }
    __syncthreads();
    *total = tot;
    return before + x - v;
}

// ---- a wave at a time: lines and records are short (a read), so a WAVE takes one -- its lanes read 64 bytes in a row
// and a ballot tells every lane which of them hold a base that stays.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ uint64_t lanes_below() { return (1ull << (threadIdx.x & 63)) - 1; }
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src)
{
    return (uint64_t)(uint32_t)__shfl((int)(uint32_t)v, src) | (uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src) << 32;
}

// Lines first .. first + N - 1 (N <= 4) of the text: lane i < N ends up with [s, e) of line first + i -- the '\n' and one
// trailing '\r' excluded -- and the line's first byte (0 for an empty line).
__device__ __forceinline__ void wave_line_spans(const uint8_t *__restrict__ t, uint64_t n, const unsigned long long *__restrict__ nl, uint64_t n_nl,
                                                uint64_t first, int N, uint64_t *s, uint64_t *e, uint8_t *c0)
{
    const int lane = threadIdx.x & 63;
    uint64_t v = 0;  // lane i <= N: the position of the newline in front of line first + i  (-1: the start of the text)
    if (lane <= N) {
        const uint64_t j = first + (uint64_t)lane;
        v = j == 0 ? ~0ull : j - 1 < n_nl ? nl[j - 1] : n;
    }
    const uint64_t nxt = shfl64(v, lane < 63 ? lane + 1 : 63);
    uint64_t ss = v + 1, ee = nxt;
    uint8_t first_byte = 0;
    if (lane < N) {
        if (ee > n) ee = n;  // (only the line after the last newline)
        if (ss > ee) ss = ee;
        if (ee > ss && t[ee - 1] == '\r') ee--;
        if (ee > ss) first_byte = t[ss];
    }
    *s = ss;
    *e = ee;
    *c0 = first_byte;
}

// The bases a wave keeps go out through 65 words of LDS of its own: lanes OR their two bits in, and a flush stores the
// words that lie wholly inside what the wave wrote since the last flush and ORs the two at the ends into the output
// (which starts zeroed), where a neighbouring read may have bits too.
constexpr uint32_t WP_WORDS = 65;
struct WavePacker {
    uint64_t *lds, *words;
    uint64_t base0, at;  // output bases [base0, at) are in the LDS words
    __device__ __forceinline__ void init(uint64_t *l, uint64_t *w)
    {
        lds = l;
        words = w;
        base0 = at = 0;
        for (uint32_t i = threadIdx.x & 63; i < WP_WORDS; i += 64) lds[i] = 0;
        wave_sync();
    }
    __device__ __forceinline__ void open(uint64_t b) { base0 = at = b; }
    __device__ __forceinline__ void flush()
    {
        wave_sync();
        const uint64_t w0 = base0 >> 5, nw = at > base0 ? ((at + 31) >> 5) - w0 : 0;
        for (uint64_t i = threadIdx.x & 63; i < nw; i += 64) {
            const uint64_t v = lds[i], W = w0 + i;
            if (W * 32 >= base0 && W * 32 + 32 <= at) words[W] = v;
            else if (v) atomicOr(reinterpret_cast<unsigned long long *>(&words[W]), (unsigned long long)v);
            lds[i] = 0;
        }
        wave_sync();
        base0 = at;
    }
    // every lane of the wave calls this; `good` lanes hold a base (code 0..3); returns where the lane's base went
    __device__ __forceinline__ uint64_t put(bool good, int code)
    {
        if (at - (base0 & ~31ull) + 64 > (uint64_t)WP_WORDS * 32) flush();
        const uint64_t gm = __ballot(good);
        const uint64_t b = at + (uint64_t)__popcll(gm & lanes_below());
        if (good && code) atomicOr(reinterpret_cast<unsigned long long *>(&lds[(b >> 5) - (base0 >> 5)]), (unsigned long long)code << (62 - 2 * (b & 31)));
        at += (uint64_t)__popcll(gm);
        return b;
    }
};

__device__ __forceinline__ uint64_t wave_index() { return ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; }
__device__ __forceinline__ uint64_t wave_count() { return ((uint64_t)gridDim.x * blockDim.x) >> 6; }

// ---- FASTQ: a wave per record (lines 4r .. 4r + 3)
struct FqRecord {
    uint64_t s1, s3;  // where the bases and the qualities start
    uint64_t len;
    bool ok;
};
__device__ __forceinline__ FqRecord fq_record(const uint8_t *__restrict__ t, uint64_t n, const unsigned long long *__restrict__ nl, uint64_t n_nl, uint64_t r)
{
    uint64_t s, e;
    uint8_t c0;
    wave_line_spans(t, n, nl, n_nl, 4 * r, 4, &s, &e, &c0);
    const uint64_t len = e - s;
    FqRecord R;
    R.s1 = shfl64(s, 1);
    R.s3 = shfl64(s, 3);
    R.len = shfl64(len, 1);
    const uint64_t len3 = shfl64(len, 3);
    const int m0 = __shfl((int)c0, 0), m2 = __shfl((int)c0, 2);
    R.ok = m0 == '@' && m2 == '+' && R.len == len3 && R.len <= 0xFFFFFFF0ull;
    return R;
}

}  // namespace tok
}  // namespace mc
