// What reads_in_set.hip, unitigs.hip and env_join.hip share: the key of a canonical k-mer in an exact open-addressing set built for one call, its
// hash and its home slot.  The tables themselves (what a slot holds beside the key, how it is built and probed) stay in the units.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

constexpr uint64_t RS_EMPTY = ~0ull;  // no canonical k-mer's word (see RsKey)

// A canonical k-mer as the table holds it.  k <= 32: the k-mer itself in `a` (all ones is never canonical: its reverse
// complement is 0).  k > 32: the 2k <= 126 bits as two words that can never be all ones either: a = hi : top bit of lo (at most 63
// bits), b = lo without its top bit.  Each word then has its own "empty" mark, and the build needs no 128-bit atomic.
struct RsKey {
    uint64_t a, b;
};

// (the four words by value: a choice between two structs by reference is a choice between two addresses, and puts both in scratch)
template <bool WIDE>
__device__ __forceinline__ RsKey rs_key(uint64_t fw_hi, uint64_t fw_lo, uint64_t rc_hi, uint64_t rc_lo)
{
    if (!WIDE) return RsKey{min(fw_lo, rc_lo), 0};
    const bool f = fw_hi < rc_hi || (fw_hi == rc_hi && fw_lo <= rc_lo);
    const uint64_t hi = f ? fw_hi : rc_hi, lo = f ? fw_lo : rc_lo;
    return RsKey{(hi << 1) | (lo >> 63), lo & ~(1ull << 63)};
}

// 32 mixed bits of a key: reads_in_set.hip's filter takes all of them (14 for the word, 3 x 6 for the bits), a table the top bits
// of a multiple
template <bool WIDE>
__device__ __forceinline__ uint32_t rs_hash(const RsKey &key)
{
    uint32_t h = (uint32_t)key.a ^ ((uint32_t)(key.a >> 32) * 0x85ebca6bu);
    if (WIDE) h ^= ((uint32_t)key.b * 0xc2b2ae35u) ^ ((uint32_t)(key.b >> 32) * 0x27d4eb2fu);
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    return h ^ (h >> 16);
}

__device__ __forceinline__ uint64_t rs_home(uint32_t h, int lg_cap) { return (uint64_t)((h * 0x9e3779b1u) >> (32 - lg_cap)); }
