// The placement arithmetic of a key that needs nothing of HIP: fmix64, the reverse complement of a packed k-mer, and the minimizer
// order and bin of kmer_device.h "Minimizer bins".  kmer_device.h includes it for the kernels; mc_hosttest (csrc/host/hosttest.cpp
// `placement`) includes it alone and prints the values, which pins tests/crowded_tables.py's restatement to this code.
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)  // a host compiler that has not seen the HIP headers: the words mean nothing to it
#define MC_KMER_HASH_OWN_WORDS                 // (taken back at the end of this file: HIP headers included later define their own)
#define __host__
#define __device__
#define __forceinline__ inline __attribute__((always_inline))
#endif

namespace mc {

__host__ __device__ constexpr __forceinline__ uint64_t fmix64(uint64_t x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// itmo!/utils/KmerUtils.java:12-22 reverseComplement(kmer, k): reverse the 2-bit groups,
// complement, right-align.  v_bfrev reverses single bits, so swap the bits of each pair back.
__host__ __device__ __forceinline__ uint64_t rc_packed(uint64_t x, int k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint64_t r = __brevll(x);
#else
    uint64_t r = x;
    r = ((r & 0x5555555555555555ull) << 1) | ((r >> 1) & 0x5555555555555555ull);
    r = ((r & 0x3333333333333333ull) << 2) | ((r >> 2) & 0x3333333333333333ull);
    r = ((r & 0x0f0f0f0f0f0f0f0full) << 4) | ((r >> 4) & 0x0f0f0f0f0f0f0f0full);
    r = ((r & 0x00ff00ff00ff00ffull) << 8) | ((r >> 8) & 0x00ff00ff00ff00ffull);
    r = ((r & 0x0000ffff0000ffffull) << 16) | ((r >> 16) & 0x0000ffff0000ffffull);
    r = (r << 32) | (r >> 32);
#endif
    r = ((r & 0x5555555555555555ull) << 1) | ((r >> 1) & 0x5555555555555555ull);
    return (~r) >> (64 - 2 * k);
}

// (what the names mean: kmer_device.h "Minimizer bins")
constexpr int SK_M = 15;
constexpr int SK_MIN_K = 23;  // shorter k-mers: runs too short to pay; regions from fmix64(key) as for hash keys
constexpr uint32_t SK_MMASK = (1u << (2 * SK_M)) - 1;
constexpr uint32_t SK_NONE = 0xFFFFFFFFu;  // "no window here" in arrays of minimizer hashes

__host__ __device__ __forceinline__ uint32_t sk_order(uint32_t canon_mmer)
{  // a bijection of 32-bit words: random-looking total order of the SK_M-mers (ties impossible below 2^30).  It never gives
   // SK_NONE for an SK_M-mer: the one word it maps there is 0xCCFF8DF3, and canonical 15-mers are below 2^30 (round 3 tested
   // every hash against it: two of the thirteen instructions a base position costs the extraction kernel)
    uint32_t x = canon_mmer * 0x9E3779B1u;
    x ^= x >> 15;
    return x;
}
static_assert(SK_M == 15, "sk_order's image of the SK_M-mers must not hold SK_NONE: check again for another SK_M");
__host__ __device__ __forceinline__ uint32_t sk_bin(uint32_t hmin)
{  // the minimum of many hashes is small: mix again before taking top bits as a bin number
    uint32_t x = hmin;
    x ^= x >> 16; x *= 0x7FEB352Du;
    x ^= x >> 15; x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}
__host__ __device__ __forceinline__ uint32_t sk_rc_mmer(uint32_t x)
{
    return (uint32_t)rc_packed((uint64_t)x, SK_M);
}
// smallest sk_order over the canonical SK_M-mers of a k-mer (either strand gives the same value)
__host__ __device__ inline uint32_t sk_hmin_of_kmer(uint64_t fw, int k)
{
    uint32_t best = SK_NONE;
    for (int i = 0; i + SK_M <= k; i++) {
        const uint32_t f = (uint32_t)(fw >> (2 * (k - SK_M - i))) & SK_MMASK, r = sk_rc_mmer(f);
        const uint32_t h = sk_order(f < r ? f : r);
        best = h < best ? h : best;
    }
    return best;
}

// The hash of a super-k-mer record's three words of bases (count_pipeline.h k_p3_dedup): its top 16 bits are the record's fingerprint
// in the merge kernel's record table, its low bits the record's home place there.  `mc_hosttest dedup-tags` prints it, which pins
// tests/dedup_leaves.py's restatement to this code.
__host__ __device__ __forceinline__ uint32_t dd_hash(uint32_t y, uint32_t z, uint32_t w)
{
    uint32_t h = (y ^ (z * 0x9E3779B1u));
    h = (h ^ (h >> 15)) * 0x85EBCA6Bu;
    h ^= w * 0xC2B2AE35u;
    h = (h ^ (h >> 13)) * 0x27D4EB2Fu;
    return h ^ (h >> 16);
}

}  // namespace mc

#ifdef MC_KMER_HASH_OWN_WORDS
#undef MC_KMER_HASH_OWN_WORDS
#undef __host__
#undef __device__
#undef __forceinline__
#endif
