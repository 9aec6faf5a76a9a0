// Plain types and constants of the kernel headers that host code of more than one unit needs: the context (context.h) holds
// the key join's and the walk's device-side state, and the group layer sizes the tokeniser's buffers.  No kernels: every header
// that defines one is included by exactly one .hip file.
#pragma once
#include "kmer_device.h"

namespace mc {

// ---- the key join (dup_check.h)

// level-1 stream: keys[((b * nseg) + seg) * cap + i], counts[b * nseg + seg]; the last segment of every bucket takes the keys
// that enter the table outside the merge kernel (the drain of handed-on occurrences, spilled records), by a global atomic
struct DupL1 {
    uint64_t *keys;    // nullptr: nobody collects
    uint32_t *counts;
    uint32_t nseg;
    uint64_t cap;
    uint32_t *lost;    // set when a segment overflows: the stream is then not used
};

// level 2's output (dup_check.h k_dup_scatter)
struct DupL2 {
    uint64_t *out_a, *out_b;   // buckets [0, split) in out_a, the others in out_b (the pipeline's two idle streams serve as one buffer)
    uint32_t split;
    uint32_t *counts;          // [(b << f2_lg | f) * slices + s]
    uint32_t f2_lg, slices;
    uint64_t cap;              // keys a segment holds
    uint32_t *lost;
    __host__ __device__ __forceinline__ uint64_t *bucket(uint32_t b) const
    {
        const uint64_t per = ((uint64_t)slices << f2_lg) * cap;
        return b < split ? out_a + (uint64_t)b * per : out_b + (uint64_t)(b - split) * per;
    }
};

// ---- the fix-up: the listed keys as a small set in global memory (qk: ~0 = free), per entry the sum of the key's counters, the
// lowest slot that holds it (the one exports count) and the number of slots
struct DupSet {
    unsigned long long *qk;
    unsigned long long *tot;
    unsigned long long *prim;
    uint64_t mask;               // slots - 1; 0 with qk == nullptr: no set
    unsigned long long *n_keys;  // distinct keys in the set
};

// (device code of the units that sweep the table: mcgpu.hip through dup_check.h, kmers_bin.hip)
__device__ __forceinline__ bool dup_set_find(const DupSet &q, uint64_t key, uint64_t *at)
{
    for (uint64_t s = fmix64(key) & q.mask;; s = (s + 1) & q.mask) {
        const unsigned long long v = q.qk[s];
        if (v == key) { *at = s; return true; }
        if (v == ~0ull) return false;
    }
}
// what a sweep that counts or lists KEYS (exports, "Hashtable size") asks about a slot: is it a listed key's second (third, ...) slot?
__device__ __forceinline__ bool dup_is_shadow(const DupSet &q, uint64_t key, uint64_t slot)
{
    if (!q.qk) return false;
    uint64_t s;
    return dup_set_find(q, key, &s) && q.prim[s] != slot;
}

// every slot of a listed key: (slot index, its own count, the set entry) noted, count added to the entry's sum
struct DupTwin { unsigned long long slot; uint32_t own, entry; };

// the look-ups of a walk that came back "absent", asked again by key (dup_check.h k_phantom_queries)
struct PhantomQ {
    unsigned long long *key, *hi, *lo;   // the hash that was asked for and the string that asked
    unsigned long long *n;               // how many (may pass cap: the caller then asks again with more room)
    uint64_t cap;
};

// ---- the walk (bfs_device.h)

struct BfsCtl {
    unsigned long long n;       // |distanceToKmer|
    unsigned long long lb, le;  // current frontier = entries [lb, le)
    unsigned long long c0;      // next candidate rank inside the frontier (wide path)
    unsigned long long lookups;
    unsigned long long rounds_narrow, rounds_slow, chunks_wide, scout_hops, scout_levels, scout_calls, scout_nf, scout_m0, slow_mismatch, slow_starved, slow_forced;
    unsigned long long tacc[8];  // MC_BFS_TIMING builds: 10 ns ticks per phase of a narrow round
    unsigned long long trace_n;  // MC_BFS_TRACE builds: records written to BfsState::trace so far
    long long level;            // distance of the frontier
    int status;
    int seeds_done;
};

struct ScoutBox;
struct BfsState {
    uint64_t *hi, *lo;  // distanceToKmer keys in insertion order
    int32_t *dist;
    int16_t *cov;
    uint32_t *flags;    // bit0: in lastKmers; bit1: seed window queued more than once.  Pre-zeroed.
    uint64_t dcap;
    uint64_t *vis;      // index of the arrays above: buckets of two (fingerprint << 32 | index) entries
    uint64_t bmask;     // number of buckets - 1
    BfsCtl *ctl;
    uint64_t *path;     // SCOUT_MAX_F * PATH_WORDS words: the predicted paths of the walkers (scout_run)
    ScoutBox *box;      // mailbox between this job's workgroup and its scouting companion (nullptr: none)
    uint32_t *trace;    // MC_BFS_TRACE builds: BFS_TRACE_RECORDS records of 8 words (nullptr: none)
    const uint64_t *seed_hi, *seed_lo;
    uint64_t n_seeds;
    int dir;
};

// ---- the tokeniser (tokenizer.h)

namespace tok {
constexpr int T_THREADS = 256;
constexpr uint32_t T_BYTES = 32;                        // bytes per thread of the newline passes
constexpr uint32_t T_TILE = T_THREADS * T_BYTES;        // 8192 bytes per workgroup
}  // namespace tok

}  // namespace mc
