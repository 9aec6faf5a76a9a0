// Read pointers (Slot::aux): their 32-bit code, which needs nothing of HIP.  kmer_device.h includes it for the kernels; mc_hosttest
// (csrc/host/hosttest.cpp `pointers`) includes it alone and prints the values, which pins tests/read_pointers.py's restatement to
// this code.
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)  // a host compiler that has not seen the HIP headers (kmer_hash.h: the same words)
#define MC_READ_PTR_OWN_WORDS                  // (taken back at the end of this file: HIP headers included later define their own)
#define __host__
#define __device__
#define __forceinline__ inline __attribute__((always_inline))
#endif

namespace mc {

// The context keeps the packed bases of every read it was given (the "read store", mcgpu.hip) and a slot remembers WHERE one
// occurrence of its key sits in it.  The BFS uses that only to GUESS the next vertices of a linear stretch -- the bases that follow
// the occurrence in its read are the path a walker will most likely take -- and looks every guess up, so a missing, stale or wrong
// pointer can cost time but never change a result.  32 bits: 0 = none; v = aux - 1 < 2^31: the occurrence starts at base v of the
// store, exactly (14 M reads of 150 bases).  Beyond that the value names a GRANULE of the store and the reader matches the k-mer
// against every offset of it (+ slack, see ptr_advance and ptr_advance_long), in tiers, so that a store a few times the exact range
// still gets fine pointers:
//   v in [2^31,            2^31 + 2^30)            granules of   4 bases   positions 2.1 G ..   6.4 G
//   v in [2^31 + 2^30,     2^31 + 2^30 + 2^29)     granules of  16 bases             6.4 G ..  15.0 G
//   v in [2^31 + 3 * 2^29, 2^32 - 2)               granules of  64 bases            15.0 G ..  49 G   (beyond: no pointer)
// (one tier of 64-base granules from 2^31 on, as it was, made the walk over 50 M reads twice as long as over 10 M.)
constexpr uint64_t PTR_EXACT_END = 1ull << 31;
constexpr uint32_t PTR_SLACK = 16;        // what ptr_advance leaves a window behind its granule: j <= 15
constexpr uint32_t PTR_SLACK_LONG = 32;   // ... and ptr_advance_long in the 64-base tier: j <= 31 (in the finer tiers it names the granule j bases on)
constexpr uint32_t PTR_LONG_WINDOWS = 32; // windows of a long record (count_long.h SKL_MAX_WINDOWS)
constexpr uint32_t PTR_T1_LG = 2, PTR_T2_LG = 4, PTR_T3_LG = 6;  // (a hop looks at 512 bases around a pointer: 64 + PTR_SLACK_LONG candidate offsets is what fits)
constexpr uint64_t PTR_T1_N = 1ull << 30, PTR_T2_N = 1ull << 29, PTR_T3_N = (1ull << 29) - 2;
constexpr uint64_t PTR_T1_POS = PTR_EXACT_END, PTR_T2_POS = PTR_T1_POS + (PTR_T1_N << PTR_T1_LG), PTR_T3_POS = PTR_T2_POS + (PTR_T2_N << PTR_T2_LG);
__host__ __device__ __forceinline__ uint32_t ptr_encode(uint64_t pos)
{
    if (pos < PTR_EXACT_END) return (uint32_t)pos + 1u;
    uint64_t v;
    if (pos < PTR_T2_POS) v = PTR_EXACT_END + ((pos - PTR_T1_POS) >> PTR_T1_LG);
    else if (pos < PTR_T3_POS) v = PTR_EXACT_END + PTR_T1_N + ((pos - PTR_T2_POS) >> PTR_T2_LG);
    else {
        const uint64_t g = (pos - PTR_T3_POS) >> PTR_T3_LG;
        if (g >= PTR_T3_N) return 0u;
        v = PTR_EXACT_END + PTR_T1_N + PTR_T2_N + g;
    }
    return (uint32_t)v + 1u;
}
// first base of the range the occurrence starts in; *span = number of candidate offsets
__host__ __device__ __forceinline__ uint64_t ptr_decode(uint32_t aux, uint32_t *span)
{
    const uint64_t v = (uint64_t)aux - 1;
    if (v < PTR_EXACT_END) { *span = 1; return v; }
    const uint64_t w = v - PTR_EXACT_END;
    if (w < PTR_T1_N) { *span = (1u << PTR_T1_LG) + PTR_SLACK; return PTR_T1_POS + (w << PTR_T1_LG); }
    if (w < PTR_T1_N + PTR_T2_N) { *span = (1u << PTR_T2_LG) + PTR_SLACK; return PTR_T2_POS + ((w - PTR_T1_N) << PTR_T2_LG); }
    *span = (1u << PTR_T3_LG) + PTR_SLACK_LONG;
    return PTR_T3_POS + ((w - PTR_T1_N - PTR_T2_N) << PTR_T3_LG);
}
// pointer of the window j <= 15 bases after the window a pointer names (windows of one super-k-mer record)
__host__ __device__ __forceinline__ uint32_t ptr_advance(uint32_t aux, uint32_t j)
{
    if (aux == 0) return 0;
    const uint64_t v = (uint64_t)aux - 1;
    if (v + 16 < PTR_EXACT_END) return aux + j;
    if (v < PTR_EXACT_END) return ptr_encode(v + j);  // (the last exact positions: window j may lie in the first granule)
    return aux;  // (a granule: the reader's range has PTR_SLACK to spare)
}
// pointer of the window j <= 31 bases behind the one `aux` names (windows of one long record, count_long.h).  Where aux names a
// granule, the window it stands for starts at one of the granule's bases, o, and window j at o + j: the granule that holds the
// granule's first base + j is the window's own or the one before (4- and 16-base tiers: o + j less that granule's start is at
// most 6 and 30, within granule + PTR_SLACK), and in the 64-base tier it is the same granule and o + j <= 94 -- what
// PTR_SLACK_LONG is for.
__host__ __device__ __forceinline__ uint32_t ptr_advance_long(uint32_t aux, uint32_t j)
{
    if (aux == 0) return 0;
    const uint64_t v = (uint64_t)aux - 1;
    if (v + PTR_LONG_WINDOWS < PTR_EXACT_END) return aux + j;
    uint32_t span;
    return ptr_encode(ptr_decode(aux, &span) + j);
}

}  // namespace mc

#ifdef MC_READ_PTR_OWN_WORDS
#undef MC_READ_PTR_OWN_WORDS
#undef __host__
#undef __device__
#undef __forceinline__
#endif
