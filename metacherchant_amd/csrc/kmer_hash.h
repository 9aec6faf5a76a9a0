// The placement arithmetic of a key that needs nothing of HIP: fmix64, the reverse complement of a packed k-mer, the polynomial key of
// a k-mer of up to 64 bases, the minimizer order and bin of kmer_device.h "Minimizer bins", the home slot inside a bin, and the bin words
// and the record hash of long records (count_long.h).  kmer_device.h includes it for the kernels; mc_hosttest (csrc/host/hosttest.cpp
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

struct Kmer {  // oriented k-mer, 2k bits right-aligned in 128, first base most significant
    uint64_t hi, lo;
};

__host__ __device__ __forceinline__ uint32_t base_at(const Kmer &v, int k, int i)
{  // i-th base, 0 = first
    const int sh = 2 * (k - 1 - i);
    return (uint32_t)((sh >= 64 ? (v.hi >> (sh - 64)) : (v.lo >> sh)) & 3);
}

// src/utils/PolynomialHash.java:19-28
__host__ __device__ inline int64_t key_poly_plain(const Kmer &v, int k, bool *flipped = nullptr)
{
    uint64_t fw = 1, rc = 1;
    for (int i = 0; i < k; i++) {
        fw = fw * 5 + base_at(v, k, i);
        rc = rc * 5 + (3u ^ base_at(v, k, k - 1 - i));
    }
    const int64_t a = (int64_t)fw, b = (int64_t)rc;
    if (flipped) *flipped = b < a;
    return a < b ? a : b;  // Math.min on signed longs
}

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

// ... of a k-mer of up to 64 bases (hi:lo, right-aligned).  Hash keys say nothing about their bases: where such keys live in
// minimizer bins (k > 32 with polynomial keys, count_pipeline.h "long records") every look-up brings the k-mer itself.
__host__ __device__ inline uint32_t sk_hmin_of_kmer2(const Kmer &v, int k, bool two = false)
{   // two: the word made of the TWO smallest values, as a multiset (skl_word2 below) -- tables with mm_k < 0
    // (the bases are taken from the k-mer's END -- two bits off the bottom of hi:lo a step --: the set of SK_M-mers is the same from
    // either side, and base_at's two variable 64-bit shifts a base were a third of what a look-up of the walk computed)
    uint64_t lo = v.lo, hi = v.hi;
    uint32_t f = 0, r = 0, best = SK_NONE, second = SK_NONE;
    for (int i = 0; i < k; i++) {
        const uint32_t b = (uint32_t)lo & 3u;
        lo = (lo >> 2) | (hi << 62);
        hi >>= 2;
        f = (f >> 2) | (b << (2 * (SK_M - 1)));   // the SK_M-mer that STARTS at this base, first base on top
        r = ((r << 2) | (3u - b)) & SK_MMASK;     // ... and its reverse complement
        if (i >= SK_M - 1) {
            const uint32_t h = sk_order(f < r ? f : r);
            const uint32_t t = h > best ? h : best;
            best = h < best ? h : best;
            second = t < second ? t : second;
        }
    }
    return two ? best ^ (second * 0x85EBCA6Bu) : best;
}

// home slot inside a minimizer-bin region: 12 well-mixed bits of the key, cheaper than fmix64 (the
// merge kernel of the counting pipeline computes it once per k-mer occurrence)
#ifndef MC_REGION_LG
#define MC_REGION_LG 12   // log2 of the slots of a table region = of the merge kernel's LDS image (tuning builds override it)
#endif
__host__ __device__ __forceinline__ uint32_t sk_home_mix(uint64_t key)
{   // (the home slot is the top MC_REGION_LG bits; the merge kernel takes two more bits below them for its pointer rule)
    uint32_t x = (uint32_t)key * 0x9E3779B1u + (uint32_t)(key >> 32) * 0x85EBCA6Bu;
    x ^= x >> 15; x *= 0xC2B2AE35u;
    return x;
}
__host__ __device__ __forceinline__ uint32_t sk_home(uint64_t key) { return sk_home_mix(key) >> (32 - MC_REGION_LG); }

// Long records (count_long.h).  The bin word of a hash key's minimizer: sk_bin with its low byte cleared (see the record's second word)
__host__ __device__ __forceinline__ uint32_t skl_bin(uint32_t hmin) { return sk_bin(hmin) & 0xFFFFFF00u; }
// ... and the word made of a window's two smallest sk_order values (count_long.h "TWO SMALLEST")
__host__ __device__ __forceinline__ uint32_t skl_word2(uint32_t lo, uint32_t hi) { return lo ^ (hi * 0x85EBCA6Bu); }
// The hash of a long record's six words of bases and its window count (count_long.h k_p3_long): its top 16 bits are the record's
// fingerprint in the merge kernel's table of equal records, its low 10 bits the record's home slot there.  `mc_hosttest long-tags`
// prints it, which pins tests/long_loci.py's restatement to this code.
__host__ __device__ __forceinline__ uint32_t skl_rec_hash(uint32_t z0, uint32_t w0, uint32_t x1, uint32_t y1, uint32_t z1, uint32_t w1, uint32_t n_windows)
{
    uint32_t h = z0 * 0x9E3779B1u ^ w0;
    h = (h ^ (h >> 15)) * 0x85EBCA6Bu ^ x1;
    h = (h ^ (h >> 13)) * 0xC2B2AE35u ^ y1;
    h = (h ^ (h >> 16)) * 0x27D4EB2Fu ^ z1;
    h = (h ^ (h >> 15)) * 0x165667B1u ^ w1 ^ n_windows;
    h ^= h >> 16;
    return h;
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
