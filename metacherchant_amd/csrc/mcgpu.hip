// libmcgpu.so -- MI355X (gfx950) k-mer counting + de Bruijn BFS behind the C ABI of include/mcgpu.h.
// Hand-written HIP for CDNA4: wave64, 16-byte table slots read with one dwordx4, memory-side
// 64-bit CAS / 32-bit add atomics, LDS-staged ordered compaction.  No MFMA: integer/hash work.
// This unit: the table, the key join, the counting pipeline and the context ABI (context.h lists the others).
//
// Reference lines each piece replaces are cited at the definitions (src/... and itmo!/... as in
// include/mcgpu.h).  Nothing in this file links or calls oracle/.
#include <unistd.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "context.h"
#include "count_pipeline.h"
#include "count_long.h"

TablePool g_table_pool;
ScratchPool g_scratch_pool;
thread_local std::string g_create_err;

// ------------------------------------------------------------------------------------------ kernels: table

__global__ void k_fill_empty(Slot *slots, uint64_t n)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint4 v;
        v.x = 0xFFFFFFFFu; v.y = 0xFFFFFFFFu; v.z = 0; v.w = 0;
        *reinterpret_cast<uint4 *>(slots + i) = v;
    }
}

// K2/K3: one wave per read, one lane per window; replaces the hot loop
// src/io/IOUtils.java:201-214 (ShortKmer.kmersOf + toLong + addAndBound) and
// src/io/LargeKIOUtils.java:41-54 (hasher.hash(dna, i, i+k) + addAndBound).
template <int MODE>
__global__ void __launch_bounds__(256) k_count_reads(const uint64_t *__restrict__ words,
                                                     const uint64_t *__restrict__ offsets, uint64_t r_begin,
                                                     uint64_t r_end, int k, TableView t, uint64_t ptr_base, uint32_t thr)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    unsigned long long n_new = 0;
    for (uint64_t r = r_begin + wave; r < r_end; r += n_waves) {
        const uint64_t b = offsets[r], e = offsets[r + 1];
        if (e - b < (uint64_t)k) continue;
        const uint64_t nwin = e - b - (uint64_t)k + 1;
        for (uint64_t w = lane; w < nwin; w += 64) {
            const Kmer v = extract_kmer(words, b + w, k);
            const uint64_t key = (uint64_t)key_of<MODE>(v, k);
            // (the inserter leaves its place in the read store; the occurrence ptr_pick names replaces it)
            n_new += table_add(t, key, 1u, ptr_base == ~0ull ? 0u : ptr_encode(ptr_base + b + w), nullptr, ptr_pick(key, thr >= 2 ? 1u : 0u, thr), ptr_pick_late(key, thr >= 2 ? 1u : 0u));
        }
    }
    wave_add_ull(t.n_used, n_new);
}

__global__ void k_add_keys(const int64_t *__restrict__ keys, uint64_t n, TableView t)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long n_new = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        n_new += table_add(t, (uint64_t)keys[i], 1u);
    wave_add_ull(t.n_used, n_new);
}

__global__ void k_add_pairs(const int64_t *__restrict__ keys, const int16_t *__restrict__ counts,
                            const uint32_t *__restrict__ hints, uint64_t n, TableView t)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long n_new = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (counts[i] > 0) n_new += table_add(t, (uint64_t)keys[i], (uint32_t)counts[i], hints ? hints[i] : 0u);
    wave_add_ull(t.n_used, n_new);
}

// the parked additions of TableView::ovf, once the table has been enlarged
// entry_leaf / leaf_state (may be null): an entry the merge kernels left (count_pipeline.h ovf_push) is skipped when its
// leaf was not committed -- that leaf is merged again and leaves its entries again
// region_of_leaf: hash keys in minimizer bins (count_long.h) -- the key does not say where it lives, the leaf it was handed on from
// does (one region a leaf; every entry of such a list comes from a leaf)
__global__ void k_add_parked(const uint4 *__restrict__ list, uint64_t n, TableView t, const uint32_t *__restrict__ entry_leaf = nullptr,
                             const uint32_t *__restrict__ leaf_state = nullptr, int region_of_leaf = 0, DupL1 d1 = DupL1{nullptr, nullptr, 0, 0, nullptr})
{   // d1: keys that are new to a table of hash keys in minimizer bins also go to the key streams of dup_check.h
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long n_new = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint32_t lf = 0xFFFFFFFFu;
        if (entry_leaf && leaf_state) {
            lf = entry_leaf[i];
            if (lf != 0xFFFFFFFFu && leaf_state[lf] == 0) continue;
        }
        const uint4 e = list[i];
        const uint64_t key = ((uint64_t)e.y << 32) | e.x;
        if (region_of_leaf && lf != 0xFFFFFFFFu) {
            const uint32_t fresh = table_add_at(t, ((uint64_t)lf << MC_REGION_LG) | sk_home(key), key, e.z, e.w);
            n_new += fresh;
            if (fresh) dup_l1_extra(d1, key);
        } else n_new += table_add(t, key, e.z, e.w);
    }
    wave_add_ull(t.n_used, n_new);
}

// table rebuild into a larger table (the reference's enlargeAndRehash,
// itmo!/structures/map/Long2ShortHashMap.java:191-214, done for the whole table at once)
__global__ void k_rehash(const Slot *__restrict__ old_slots, uint64_t n_old, TableView t)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long n_new = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_old; i += stride) {
        const uint4 raw = *reinterpret_cast<const uint4 *>(old_slots + i);
        const uint64_t key = ((uint64_t)raw.y << 32) | raw.x;
        if (key != EMPTY_KEY) n_new += table_add(t, key, raw.z, raw.w);
    }
    wave_add_ull(t.n_used, n_new);
}

// The solid table's regions (SOLID_REGION slots, 32 KB)
constexpr uint32_t SOLID_SB = 11, SOLID_REGION = 1u << SOLID_SB;
// (Round 3 also had k_build_solid_regions: a workgroup per solid region, fed from the counting regions whose hash prefix it
// shares.  It took every key to sit in its home counting region -- no longer so since additions that find their stretch full
// move on to the next region, kmer_device.h TABLE_CHAIN -- and lost the others: every solid table is now built
// by the sweep below, which asks no such thing.)

// K6: the solid table indexes by the key's own hash, so its regions draw from all over a counting table organised by
// minimizer bins (mc_ctx::mm_k) -- and from next door in one organised by hash prefixes, where a key may have been handed on.  The solid
// entries (a few % of the occurrences) therefore take the same route as the counting records:
// k_solid_emit sweeps the counting table and appends every entry with count >= min_cov to the level-1
// bucket of its solid slot (256 workgroups, each its own segment of every bucket), k_sk2_scatter
// splits the buckets into one leaf per solid region, k_solid_from_leaves assembles each region in
// LDS.  No fill pass, no global atomics.
__global__ void __launch_bounds__(PT_THREADS) k_solid_emit(const Slot *__restrict__ slots, uint64_t n_slots, int min_cov, uint32_t np1,
                                                            uint32_t *seg_counts, uint64_t cap, uint4 *out_recs, uint32_t *out_bins,
                                                            SkSpill sp)
{
    __shared__ SkCursors C;
    const uint32_t tid = threadIdx.x, n_buckets = np1;
    if (tid < PT_MAX_LEAVES2) { C.wcur[tid] = 0; C.cnt[tid] = 0; }
    __syncthreads();
    // Rows of 4 slots (64 bytes: one memory sector) are dealt to the workgroups (= segments) round-robin, as k_solid_emit_pairs
    // deals its rows: a table whose regions are hash prefixes is in the order of the very hash that picks the bucket here, and
    // whole tiles of it would put a bucket's entries into a few segments only (the segment capacities count on every segment
    // getting its share of every bucket).
    constexpr uint32_t WAVES = PT_THREADS / 64, ROW = 4, ROWS_PER_WAVE = 64 / ROW;
    const uint64_t n_rows = (n_slots + ROW - 1) / ROW;
    const uint32_t wave = tid >> 6, lane = tid & 63;
    for (uint64_t t0 = 0; t0 * WAVES * ROWS_PER_WAVE * gridDim.x < n_rows; t0 += PT_ITEMS) {
        uint4 raws[PT_ITEMS];
#pragma unroll
        for (int j = 0; j < PT_ITEMS; j++) {
            const uint64_t local = ((t0 + (uint64_t)j) * WAVES + wave) * ROWS_PER_WAVE + lane / ROW;  // this workgroup's row number
            const uint64_t i = (local * gridDim.x + blockIdx.x) * ROW + lane % ROW;
            raws[j] = i < n_slots ? *reinterpret_cast<const uint4 *>(slots + i) : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < PT_ITEMS; j++) {
            const uint64_t key = ((uint64_t)raws[j].y << 32) | raws[j].x;
            if (key == EMPTY_KEY) continue;
            const uint32_t c = raws[j].z > 32767u ? 32767u : raws[j].z;
            if ((int)c < min_cov) continue;
            raws[j].z = c;
            const uint32_t bin = (uint32_t)(fmix64(key) >> 32);
            sk_emit(C, mulhi32(bin, np1), raws[j], bin, cap, (uint64_t)blockIdx.x * cap, (uint64_t)PT_SEGMENTS * cap, out_recs, out_bins, sp);
        }
        __syncthreads();
        if (tid < n_buckets) { C.wcur[tid] += C.cnt[tid]; C.cnt[tid] = 0; }
        __syncthreads();
    }
    if (tid < n_buckets) seg_counts[(uint64_t)tid * PT_SEGMENTS + blockIdx.x] = min(C.wcur[tid], (uint32_t)cap);
}

// The same first step for solid entries that arrive as (key, count, hint) arrays -- the thresholded shards of the
// other ranks (mc_solid_from_pairs_dev) -- instead of sitting in this context's counting table.
__global__ void __launch_bounds__(PT_THREADS) k_solid_emit_pairs(const int64_t *__restrict__ keys, const int16_t *__restrict__ counts,
                                                                  const uint32_t *__restrict__ hints, uint64_t n, int min_cov, uint32_t np1,
                                                                  uint32_t *seg_counts, uint64_t cap, uint4 *out_recs, uint32_t *out_bins,
                                                                  SkSpill sp, unsigned long long *empty_cnt)
{
    __shared__ SkCursors C;
    const uint32_t tid = threadIdx.x, n_buckets = np1;
    if (tid < PT_MAX_LEAVES2) { C.wcur[tid] = 0; C.cnt[tid] = 0; }
    __syncthreads();
    // Rows of 8 entries (64 bytes of keys: one memory sector) are dealt to the workgroups (= segments) round-robin.  An
    // export comes in table order, which for hash-prefix tables is the order of the very hash that picks the bucket
    // -- one sorted run per gathered shard -- and short arrays must not land in a few segments either: the segment
    // capacities count on each segment getting its share of every bucket, to within a row per shard.
    constexpr uint32_t WAVES = PT_THREADS / 64, ROW = 8, ROWS_PER_WAVE = 64 / ROW;
    const uint64_t n_rows = (n + ROW - 1) / ROW;
    const uint32_t wave = tid >> 6, lane = tid & 63;
    for (uint64_t t0 = 0; t0 * WAVES * ROWS_PER_WAVE * gridDim.x < n_rows; t0 += PT_ITEMS) {
#pragma unroll
        for (int j = 0; j < PT_ITEMS; j++) {
            const uint64_t local = ((t0 + (uint64_t)j) * WAVES + wave) * ROWS_PER_WAVE + lane / ROW;  // this workgroup's row number
            const uint64_t i = (local * gridDim.x + blockIdx.x) * ROW + lane % ROW;
            if (i >= n) continue;
            const int c = counts[i];
            if (c < min_cov || c < 0) continue;
            const uint64_t key = (uint64_t)keys[i];
            if (key == EMPTY_KEY) { atomicAdd(empty_cnt, (unsigned long long)c); continue; }  // kept out of band, as in the counting table
            const uint4 rec = make_uint4((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)c, hints ? hints[i] : 0u);
            const uint32_t bin = (uint32_t)(fmix64(key) >> 32);
            sk_emit(C, mulhi32(bin, np1), rec, bin, cap, (uint64_t)blockIdx.x * cap, (uint64_t)PT_SEGMENTS * cap, out_recs, out_bins, sp);
        }
        __syncthreads();
        if (tid < n_buckets) { C.wcur[tid] += C.cnt[tid]; C.cnt[tid] = 0; }
        __syncthreads();
    }
    if (tid < n_buckets) seg_counts[(uint64_t)tid * PT_SEGMENTS + blockIdx.x] = min(C.wcur[tid], (uint32_t)cap);
}

// ... and for the solid list P3 left behind (count_pipeline.h P3Emit): nseg segments of (key, count, hint) records.
// Workgroup b takes segments b, b + gridDim.x, ...: a segment holds what one P3 workgroup saw, regions from all over
// the table, so every workgroup here feeds all buckets evenly.
__global__ void __launch_bounds__(PT_THREADS) k_solid_emit_list(const uint4 *__restrict__ list, const uint32_t *__restrict__ list_counts,
                                                                 uint32_t nseg, uint64_t list_segcap, uint32_t np1, uint32_t *seg_counts,
                                                                 uint64_t cap, uint4 *out_recs, uint32_t *out_bins, SkSpill sp)
{
    __shared__ SkCursors C;
    const uint32_t tid = threadIdx.x, n_buckets = np1;
    if (tid < PT_MAX_LEAVES2) { C.wcur[tid] = 0; C.cnt[tid] = 0; }
    __syncthreads();
    for (uint32_t sg = blockIdx.x; sg < nseg; sg += gridDim.x) {
        const uint32_t n = list_counts[sg];
        const uint4 *src = list + (uint64_t)sg * list_segcap;
        for (uint32_t i0 = 0; i0 < n; i0 += PT_TILE) {
            uint4 raws[PT_ITEMS];
#pragma unroll
            for (int j = 0; j < PT_ITEMS; j++) {
                const uint32_t i = i0 + tid + (uint32_t)j * PT_THREADS;
                raws[j] = i < n ? src[i] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < PT_ITEMS; j++) {
                const uint64_t key = ((uint64_t)raws[j].y << 32) | raws[j].x;
                if (key == EMPTY_KEY) continue;  // (padding of the last tile; the table never holds this key)
                const uint32_t bin = (uint32_t)(fmix64(key) >> 32);
                sk_emit(C, mulhi32(bin, np1), raws[j], bin, cap, (uint64_t)blockIdx.x * cap, (uint64_t)PT_SEGMENTS * cap, out_recs, out_bins, sp);
            }
            __syncthreads();
            if (tid < n_buckets) { C.wcur[tid] += C.cnt[tid]; C.cnt[tid] = 0; }
            __syncthreads();
        }
    }
    if (tid < n_buckets) seg_counts[(uint64_t)tid * PT_SEGMENTS + blockIdx.x] = min(C.wcur[tid], (uint32_t)cap);
}

__global__ void k_count_pairs(const int16_t *__restrict__ counts, const int64_t *__restrict__ keys, uint64_t n, int min_cov,
                              unsigned long long *out)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        m += counts[i] >= min_cov && counts[i] >= 0 && (uint64_t)keys[i] != EMPTY_KEY;
    wave_add_ull(out, m);
}

// one workgroup per solid region = one leaf (nseg segments of capacity seg_cap, as for k_p3_merge)
__global__ void __launch_bounds__(512) k_solid_from_leaves(const uint4 *__restrict__ leaf_recs, const uint32_t *__restrict__ seg_counts,
                                                           uint64_t seg_cap, uint32_t nseg, SolidView solid, uint32_t solid_lg)
{
    __shared__ Slot R[SOLID_REGION];
    __shared__ uint32_t overflow;
    const uint32_t tid = threadIdx.x;
    const uint64_t n_regions = 1ull << (solid_lg - SOLID_SB);
    for (uint64_t Q = blockIdx.x; Q < n_regions; Q += gridDim.x) {
        for (uint32_t i = tid; i < SOLID_REGION; i += 512) {
            R[i].key = EMPTY_KEY; R[i].count = 0; R[i].aux = 0;
        }
        if (tid == 0) overflow = 0;
        __syncthreads();
        for (uint32_t sgm = 0; sgm < nseg; sgm++) {
            const uint32_t n = min(seg_counts[Q * nseg + sgm], (uint32_t)seg_cap);
            const uint4 *recs = leaf_recs + (Q * nseg + sgm) * seg_cap;
            for (uint32_t i = tid; i < n; i += 512) {
                const uint4 raw = recs[i];
                const uint64_t key = ((uint64_t)raw.y << 32) | raw.x;
                uint32_t s = (uint32_t)(fmix64(key) >> (64 - solid_lg)) & (SOLID_REGION - 1);
                bool done = false;
                for (uint32_t probe = 0; probe < (SOLID_REGION < TABLE_MAX_PROBES ? SOLID_REGION : TABLE_MAX_PROBES); probe++) {  // (where a lookup gives the region up: kmer_device.h solid_probe_from)
                    if (atomicCAS(reinterpret_cast<unsigned long long *>(&R[s].key), (unsigned long long)EMPTY_KEY,
                                  (unsigned long long)key) == EMPTY_KEY) {
                        R[s].count = raw.z;
                        R[s].aux = raw.w;
                        done = true;
                        break;
                    }
                    s = (s + 1) & (SOLID_REGION - 1);
                }
                if (!done) atomicExch(&overflow, 1u);
            }
        }
        __syncthreads();
        if (overflow && tid == 0) atomicExch(solid.fatal, 1u);
        uint4 *dst = reinterpret_cast<uint4 *>(solid.slots + Q * SOLID_REGION);
        const uint4 *src = reinterpret_cast<const uint4 *>(R);
        for (uint32_t i = tid; i < SOLID_REGION; i += 512) dst[i] = src[i];
        __syncthreads();
    }
}

// windows = sum over reads of max(0, len - k + 1); also checks that the offsets never decrease
__global__ void k_reads_summary(const uint64_t *__restrict__ offsets, uint64_t n_reads, uint64_t k,
                                unsigned long long *out /* [0] windows, [1] violations; ends != 0: [2] first offset, [3] last offset */, int ends = 0)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long w = 0, bad = 0;
    // two reads a thread and step (three offsets, the middle one shared): half the loads of a read a thread
    for (uint64_t i = 2 * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x); i < n_reads; i += 2 * stride) {
        const uint64_t a = offsets[i], b = offsets[i + 1];
        if (b < a) bad++;
        else if (b - a >= k) w += b - a - k + 1;
        if (i + 1 < n_reads) {
            const uint64_t c2 = offsets[i + 2];
            if (c2 < b) bad++;
            else if (c2 - b >= k) w += c2 - b - k + 1;
        }
    }
    // one pair of atomics a WORKGROUP, at most 512 of them: atomics on one address take their turns at ~7 ns each, and a pair per
    // wave of 2048 workgroups (16 000 of them) was 120 us for 10 M reads -- four times what reading the offsets takes
    __shared__ unsigned long long part[2][4];
    for (int o = 32; o > 0; o >>= 1) { w += __shfl_down(w, o); bad += __shfl_down(bad, o); }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = w; part[1][threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tw = 0, tb = 0;
        for (unsigned i = 0; i < (blockDim.x + 63) / 64 && i < 4; i++) { tw += part[0][i]; tb += part[1][i]; }
        if (tw) atomicAdd(out, tw);
        if (tb) atomicAdd(out + 1, tb);
    }
    if (ends && blockIdx.x == 0 && threadIdx.x == 0) { out[2] = offsets[0]; out[3] = offsets[n_reads]; }
}

// K4: BigLong2ShortHashMap.get for a batch of keys
__global__ void k_get(const int64_t *__restrict__ keys, uint64_t n, int16_t *__restrict__ out, TableView t)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = (int16_t)table_get(t, (uint64_t)keys[i]);
}

// ... for a table of hash keys in minimizer bins (count_long.h), where a bare key does not say which region it lives in: the
// QUERIES go into a small set (qk: key, ~0 = free; qi: the first query that asked for it), the whole table is swept once and
// every slot whose key is in the set answers, queries that repeat a key copy the answer.  A sweep per call -- 20 GB in 5 ms --
// instead of a rebuild of the table that would end the long-record form for good (and cannot be afforded where the table is
// half the device's memory).
__global__ void k_getq_build(const int64_t *__restrict__ keys, uint64_t n, unsigned long long *qk, uint32_t *qi, uint64_t mask)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t key = (uint64_t)keys[i];
        if (key == EMPTY_KEY) continue;
        for (uint64_t s = fmix64(key) & mask;; s = (s + 1) & mask) {
            const unsigned long long old = atomicCAS(&qk[s], ~0ull, (unsigned long long)key);
            if (old == ~0ull) { qi[s] = (uint32_t)i; break; }
            if (old == key) break;
        }
    }
}
__global__ void k_getq_sweep(const Slot *__restrict__ slots, uint64_t n_slots, const unsigned long long *__restrict__ qk, const uint32_t *__restrict__ qi,
                             uint64_t mask, int16_t *__restrict__ out)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride) {
        const uint4 raw = *reinterpret_cast<const uint4 *>(slots + i);
        const uint64_t key = ((uint64_t)raw.y << 32) | raw.x;
        if (key == EMPTY_KEY) continue;
        for (uint64_t s = fmix64(key) & mask;; s = (s + 1) & mask) {
            const unsigned long long q = qk[s];
            if (q == ~0ull) break;
            if (q == key) { out[qi[s]] = (int16_t)(raw.z > 32767u ? 32767u : raw.z); break; }
        }
    }
}
__global__ void k_getq_finish(const int64_t *__restrict__ keys, uint64_t n, const unsigned long long *__restrict__ qk, const uint32_t *__restrict__ qi,
                              uint64_t mask, int16_t *__restrict__ out, const unsigned long long *__restrict__ empty_cnt)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t key = (uint64_t)keys[i];
        if (key == EMPTY_KEY) {
            const unsigned long long c = *empty_cnt;
            out[i] = (int16_t)(c == 0 ? -1 : (c > 32767ull ? 32767 : (int)c));
            continue;
        }
        for (uint64_t s = fmix64(key) & mask;; s = (s + 1) & mask)
            if (qk[s] == key) {
                if (qi[s] != (uint32_t)i) out[i] = out[qi[s]];  // (the first query for this key got the answer)
                break;
            }
    }
}

// K6: (key, count) pairs with count >= min_cov; with keys == nullptr only counts them.
constexpr int EXP_THREADS = 256, EXP_ITEMS = 8, EXP_TILE = EXP_THREADS * EXP_ITEMS;

__global__ void __launch_bounds__(EXP_THREADS) k_export(const Slot *__restrict__ slots, uint64_t n_slots, int min_cov,
                                                        int64_t *__restrict__ keys, int16_t *__restrict__ counts,
                                                        uint32_t *__restrict__ hints, uint64_t cap, unsigned long long *cursor,
                                                        DupSet dq = DupSet{nullptr, nullptr, nullptr, 0, nullptr})
{
    // dq: hash keys in minimizer bins -- a key that two k-mers brought to two regions is counted / listed at its first slot only
    // (dup_check.h; every slot of it holds the sum of its counters)
    // A tile of slots is compacted in LDS (one LDS cursor update per wave and row), takes ONE slice of the output
    // with a single global atomic and leaves in coalesced stores: a global atomic per wave and row would put
    // n_slots / 64 updates on one address, which alone costs ~10 ns each.
    __shared__ uint4 buf[EXP_TILE];
    __shared__ uint32_t lcur;
    __shared__ unsigned long long gbase;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    unsigned long long counted = 0;
    const uint64_t n_tiles = (n_slots + EXP_TILE - 1) / EXP_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint4 raws[EXP_ITEMS];
#pragma unroll
        for (int j = 0; j < EXP_ITEMS; j++) {
            const uint64_t i = tile * EXP_TILE + (uint64_t)j * EXP_THREADS + tid;
            raws[j] = i < n_slots ? *reinterpret_cast<const uint4 *>(slots + i) : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0);
        }
        if (!keys) {
#pragma unroll
            for (int j = 0; j < EXP_ITEMS; j++) {
                const uint64_t key = ((uint64_t)raws[j].y << 32) | raws[j].x;
                const int c = raws[j].z > 32767u ? 32767 : (int)raws[j].z;
                counted += key != EMPTY_KEY && c >= min_cov && !dup_is_shadow(dq, key, tile * EXP_TILE + (uint64_t)j * EXP_THREADS + tid) ? 1u : 0u;
            }
            continue;
        }
        if (tid == 0) lcur = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < EXP_ITEMS; j++) {
            const uint64_t key = ((uint64_t)raws[j].y << 32) | raws[j].x;
            const int c = raws[j].z > 32767u ? 32767 : (int)raws[j].z;
            const bool take = key != EMPTY_KEY && c >= min_cov && !dup_is_shadow(dq, key, tile * EXP_TILE + (uint64_t)j * EXP_THREADS + tid);
            const unsigned long long m = __ballot(take);
            if (!m) continue;
            uint32_t base = 0;
            const int leader = __ffsll((long long)m) - 1;
            if ((int)lane == leader) base = atomicAdd(&lcur, (uint32_t)__popcll(m));
            base = __shfl(base, leader);
            if (take) buf[base + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = make_uint4(raws[j].x, raws[j].y, (uint32_t)c, raws[j].w);
        }
        __syncthreads();
        const uint32_t n_out = lcur;
        if (tid == 0 && n_out) gbase = atomicAdd(cursor, (unsigned long long)n_out);
        __syncthreads();
        for (uint32_t i = tid; i < n_out; i += EXP_THREADS) {
            const unsigned long long pos = gbase + i;
            if (pos < cap) {
                const uint4 e = buf[i];
                keys[pos] = (int64_t)(((uint64_t)e.y << 32) | e.x);
                counts[pos] = (int16_t)e.z;
                if (hints) hints[pos] = e.w;
            }
        }
        __syncthreads();
    }
    if (!keys) wave_add_ull(cursor, counted);
}

// K6 from the solid list the merge kernel left (count_pipeline.h P3Emit): a segment takes its slice of the output
// with one atomic and is copied over -- 0.8 GB read instead of a sweep of the table.
__global__ void __launch_bounds__(256) k_export_list(const uint4 *__restrict__ list, const uint32_t *__restrict__ list_counts, uint32_t nseg,
                                                     uint64_t list_segcap, int64_t *__restrict__ keys, int16_t *__restrict__ counts,
                                                     uint32_t *__restrict__ hints, uint64_t cap, unsigned long long *cursor)
{
    __shared__ unsigned long long gbase;
    for (uint32_t sg = blockIdx.x; sg < nseg; sg += gridDim.x) {
        const uint32_t n = list_counts[sg];
        if (threadIdx.x == 0 && n) gbase = atomicAdd(cursor, (unsigned long long)n);
        __syncthreads();
        const uint4 *src = list + (uint64_t)sg * list_segcap;
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
            const unsigned long long pos = gbase + i;
            if (pos < cap) {
                const uint4 e = src[i];
                keys[pos] = (int64_t)(((uint64_t)e.y << 32) | e.x);
                counts[pos] = (int16_t)e.z;
                if (hints) hints[pos] = e.w;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ kernels: synthetic reads

constexpr uint64_t ERR_STREAM = 0xE44044E44044E440ull;

__host__ __device__ __forceinline__ uint32_t synth_read_base(uint64_t gseed, uint64_t n_contigs, uint64_t contig_len,
                                                             uint64_t rseed, uint64_t r, uint32_t L, uint32_t err,
                                                             uint32_t j)
{
    const uint64_t x0 = splitmix(rseed, 2 * r), x1 = splitmix(rseed, 2 * r + 1);
    const uint64_t contig = (x0 >> 33) % n_contigs;
    const bool strand = x0 & 1;
    const uint64_t start = x1 % (contig_len - L + 1);
    const uint64_t g = contig * contig_len + start + (strand ? (uint64_t)(L - 1 - j) : (uint64_t)j);
    uint32_t b = (uint32_t)(splitmix(gseed, g) & 3);
    if (strand) b ^= 3;
    if (err) {
        const uint64_t e = splitmix(rseed ^ ERR_STREAM, r * (uint64_t)L + j);
        if ((uint32_t)(e % 10000) < err) b = (b + 1 + (uint32_t)((e >> 40) % 3)) & 3;
    }
    return b;
}

// one thread per output word (32 bases)
__global__ void k_synth_reads(uint64_t gseed, uint64_t n_contigs, uint64_t contig_len, uint64_t rseed,
                              uint64_t first_read, uint64_t n_reads, uint32_t L, uint32_t err, uint64_t *words,
                              uint64_t n_words, uint64_t *offsets)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_bases = n_reads * (uint64_t)L;
    for (uint64_t w = tid; w < n_words; w += stride) {
        uint64_t v = 0;
        for (uint32_t i = 0; i < 32; i++) {
            const uint64_t p = w * 32 + i;
            if (p >= n_bases) break;
            const uint64_t r = p / L;
            const uint32_t j = (uint32_t)(p - r * L);
            v |= (uint64_t)synth_read_base(gseed, n_contigs, contig_len, rseed, first_read + r, L, err, j)
                 << (62 - 2 * i);
        }
        words[w] = v;
    }
    for (uint64_t r = tid; r <= n_reads; r += stride) offsets[r] = r * (uint64_t)L;
}

// ------------------------------------------------------------------------------------------ host: table management

// Number of regions for a table of at least `slots` slots.  Hash-prefix regions need a power of two; minimizer bins
// are numbered by multiplication (count_pipeline.h mulhi32), so those tables come in steps of 512 regions (2 M slots,
// 32 MB), of 1024 beyond 2^19 regions -- times 2^g beyond 2^20, where a leaf of the counting pipeline covers 2^g regions.
uint64_t regions_for(const mc_ctx *c, uint64_t slots)
{
    uint64_t want = std::max<uint64_t>((slots + (1ull << c->sb) - 1) >> c->sb, 1);
    uint64_t p2 = 1;
    while (p2 < want) p2 <<= 1;
    if (!c->mm_k || want <= 512) return p2;
    // up to 2^19 regions: 512 level-1 buckets of up to 1024 leaves, regions in steps of 512; up to 2^20: 1024 buckets, steps of
    // 1024; beyond: a leaf covers 2^g regions and the steps double with it
    uint64_t step = ((want + 511) / 512) * 512 <= (512ull << 10) ? 512 : 1024;
    while (((want + step - 1) / step) * step > (step << 10)) step <<= 1;
    return ((want + step - 1) / step) * step;
}

// Slots for `keys` distinct k-mers at load `load` in a minimizer-bin table: never more than the pipeline has leaves for
// (2^20, one region each) while the load stays under 0.6, and beyond that 2^g regions per leaf for the smallest g that
// keeps it there -- every doubling of g doubles the merge kernel's sweeps over a leaf's records.
static uint64_t mm_slots_for(const mc_ctx *c, double keys, double load)
{
    uint64_t want = (uint64_t)(keys / load);
    const uint64_t one_leaf_each = 1ull << (SK_LEAVES_LG + c->sb);
    if (c->mm_k && want > one_leaf_each) {
        uint64_t cap_slots = one_leaf_each;
        while (keys > 0.6 * (double)cap_slots) cap_slots <<= 1;
        want = std::min(want, cap_slots);
    }
    return want;
}

static int table_alloc(mc_ctx *c, uint64_t n_regions)
{
    if (n_regions < 1) n_regions = 1;
    if (n_regions > (1ull << 24)) return fail(c, MC_EOVERFLOW, "k-mer table would need %llu regions", (unsigned long long)n_regions);
    c->n_regions = n_regions;
    c->rb = 0;
    while ((2ull << c->rb) <= n_regions) c->rb++;
    {
        void *blk = nullptr;
        size_t got = 0;
        hipError_t e = g_table_pool.get(c->cfg.device, c->n_slots() * sizeof(Slot), &blk, &got);
        if (e == hipErrorOutOfMemory) {  // (idle scratch blocks are given back first)
            (void)hipGetLastError();
            g_scratch_pool.release(c->cfg.device);
            e = g_table_pool.get(c->cfg.device, c->n_slots() * sizeof(Slot), &blk, &got);
        }
        HIPCHK(c, e);
        c->slots = static_cast<Slot *>(blk);
        c->slots_bytes = got;
    }
    c->virgin = true;  // filled lazily: the partitioned pipeline writes every region itself
    c->st.table_slots = c->n_slots();
    c->st.table_bytes = c->n_slots() * sizeof(Slot);
    return MC_OK;
}

// the direct kernels, lookups and exports need real (EMPTY-initialised) slots
// The table is about to hold other counts (or to move: growing and rehashing give the old block back to the pool): results
// read before are void, and so is a walker's view of the ranks' tables (mc_shard_attach) -- it names this table's block
// and geometry as they were.  ADVICE r4: the attachment used to survive, and the next walk read a freed block.  The solid
// table built from the counts is stale with them.
static inline void counts_changed(mc_ctx *c)
{
    if (c->d_shards) { shard_detach_locked(c); c->shards_dropped = true; }
    c->finalized = false;
    c->dup.checked = false;
    c->dup.l2_valid = false;
    c->solid_cov = -1;
    c->solid_external = false;
}

int materialize(mc_ctx *c)
{
    if (!c->virgin) return MC_OK;
    hipLaunchKernelGGL(k_fill_empty, dim3(grid_for(c->n_slots(), 256)), dim3(256), 0, c->stream, c->slots,
                       c->n_slots());
    HIPCHK(c, hipGetLastError());
    c->virgin = false;
    return MC_OK;
}

int read_counters(mc_ctx *c, unsigned long long *n_used, uint32_t *fatal)
{
    unsigned long long *h = c->h_scratch;
    HIPCHK(c, hipMemcpyAsync(h, c->d_ctr, 9 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_used = h[0];
    *fatal = (uint32_t)h[8];
    return MC_OK;
}

// the table's block goes back to the pool
static void table_release(mc_ctx *c, Slot *slots, size_t bytes) { g_table_pool.put(c->cfg.device, slots, bytes); }

// What table_grow / to_hash_regions put aside while they move the keys: the old table comes back, with its counters, if
// anything fails before the move is complete (and goes to the pool when it is).
struct TableSwap {
    mc_ctx *c;
    Slot *old;
    size_t old_bytes;
    uint64_t old_regions;
    uint32_t old_rb;
    bool old_virgin;
    int old_mm;
    unsigned long long old_used = 0;
    bool have_used = false;  // old_used has been read (only then is it written back when the swap is abandoned)
    bool done = false;
    explicit TableSwap(mc_ctx *ctx) : c(ctx), old(ctx->slots), old_bytes(ctx->slots_bytes), old_regions(ctx->n_regions), old_rb(ctx->rb), old_virgin(ctx->virgin), old_mm(ctx->mm_k) {}
    ~TableSwap()
    {
        if (done) { table_release(c, old, old_bytes); return; }
        if (c->slots && c->slots != old) table_release(c, c->slots, c->slots_bytes);  // the half-filled new table
        c->slots = old; c->slots_bytes = old_bytes; c->n_regions = old_regions; c->rb = old_rb; c->virgin = old_virgin; c->mm_k = old_mm;
        if (have_used) (void)hipMemcpy(c->d_ctr, &old_used, sizeof old_used, hipMemcpyHostToDevice);  // (n_used as it was)
    }
};

// Hash keys in minimizer bins (count_long.h: polynomial keys, k > 32, counted as long records): nothing that has only the key
// can find it there, and such a table cannot be rebuilt with another number of bins either.  Everything that works by key --
// mc_get, key streams, the direct kernel, growing -- first moves the table to hash-prefix regions, for good (by_key_ready).
__global__ void k_ctr_add(unsigned long long *p, long long d) { if (threadIdx.x == 0 && blockIdx.x == 0) *p += (unsigned long long)d; }
// The slots of keys that sit in several regions (dup_check.h) get their own counts back: before the table takes more reads (the
// merge kernel adds to whichever slot a k-mer's bin holds) and before its keys move to hash-prefix regions (where equal keys meet
// and their counts add up by themselves).
int dup_unmerge(mc_ctx *c)
{
    mc_ctx::Dup &D = c->dup;
    if (!D.merged || !D.n_tw) { D.merged = false; return MC_OK; }
    hipLaunchKernelGGL(k_dup_apply, dim3((unsigned)((D.n_tw + 255) / 256)), dim3(256), 0, c->stream, c->slots, D.tw, D.n_tw, D.set, 0);
    HIPCHK(c, hipGetLastError());
    if (D.solid_delta) {
        hipLaunchKernelGGL(k_ctr_add, dim3(1), dim3(64), 0, c->stream, c->d_ctr + 6, -D.solid_delta);
        HIPCHK(c, hipGetLastError());
    }
    D.merged = false;
    D.solid_delta = 0;
    D.checked = false;
    return MC_OK;
}
// nothing is known about the table's keys any more (it is empty, or no longer in minimizer bins)
static void dup_forget(mc_ctx *c)
{
    mc_ctx::Dup &D = c->dup;
    D.merged = false; D.n_tw = 0; D.n_keys = 0; D.solid_delta = 0; D.checked = false; D.l1_armed = false; D.expected_keys = 0; D.l2_valid = false;
    c->st.dup_keys = 0;
    c->st.dup_unchecked = 0;
}
// why: what mc_stats.left_bins reports (include/mcgpu.h): 1 something came or asked by key (a key stream, mc_load_kmers, mc_shard_export, a
// copy of the solid k-mers), 2 a small batch took the direct kernel, 3 the long form declined a batch (nothing vouched for the table's
// size), 4 bins overflowed or the table had to grow, 5 more keys sat in several regions than the join's lists take
static int to_hash_regions(mc_ctx *c, int why = 1);
int by_key_ready(mc_ctx *c, int why) { return hash_bins(c) ? to_hash_regions(c, why) : MC_OK; }

int table_grow(mc_ctx *c, uint64_t new_regions)
{
    if (hash_bins(c) && c->virgin) {  // nothing to move: another empty table, still in minimizer bins
        table_release(c, c->slots, c->slots_bytes);
        c->slots = nullptr;
        int rc = table_alloc(c, new_regions);
        if (!rc) c->st.grows++;
        return rc;
    }
    if (hash_bins(c)) {
        int rc = to_hash_regions(c, 4);
        if (rc) return rc;
        new_regions = regions_for(c, new_regions << c->sb);  // (a power of two now)
        if (new_regions <= c->n_regions) return MC_OK;
    }
    TableSwap sw(c);
    HIPCHK(c, hipMemcpyAsync(&sw.old_used, c->d_ctr, sizeof sw.old_used, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    sw.have_used = true;
    const uint64_t old_n = c->n_slots();
    c->slots = nullptr;
    int rc = table_alloc(c, new_regions);
    if (rc) return rc;
    if (!sw.old_virgin) {  // (else: nothing to move)
        rc = materialize(c);
        if (rc) return rc;
        HIPCHK(c, hipMemsetAsync(c->d_ctr, 0, sizeof(unsigned long long), c->stream));  // n_used is recounted
        hipLaunchKernelGGL(k_rehash, dim3(grid_for(old_n, 256)), dim3(256), 0, c->stream, sw.old, old_n, c->view());
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    sw.done = true;
    c->st.grows++;
    return MC_OK;
}

// When the k-mers of a read set crowd into single minimizer bins -- a genome covered more than ~1500-fold: the error
// variants of one locus share its minimizer and outnumber a region's 4096 slots -- no number of regions helps.  The
// context then gives up minimizer bins for good: regions by the key's own hash, as for hash keys and short k-mers
// (reads take the per-window pipeline from here on), with everything counted so far moved over.
static int to_hash_regions(mc_ctx *c, int why)
{
    if (!c->mm_k) return MC_OK;
    if (hash_bins(c)) c->st.left_bins = (uint64_t)why;  // (the long-record form ends here for good, and only mc_stats.grows used to show it)
    if (int urc = dup_unmerge(c)) return urc;  // (equal keys meet in the new table: their own counts add up there)
    TableSwap sw(c);
    HIPCHK(c, hipMemcpyAsync(&sw.old_used, c->d_ctr, sizeof sw.old_used, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    sw.have_used = true;
    const unsigned long long used = sw.old_used;
    const uint64_t old_n = c->n_slots();
    c->mm_k = 0;
    c->slots = nullptr;
    int rc = table_alloc(c, regions_for(c, std::max<uint64_t>(old_n, 2 * used)));
    if (rc) return rc;
    if (!sw.old_virgin) {
        rc = materialize(c);
        if (rc) return rc;
        HIPCHK(c, hipMemsetAsync(c->d_ctr, 0, sizeof(unsigned long long), c->stream));  // n_used is recounted
        hipLaunchKernelGGL(k_rehash, dim3(grid_for(old_n, 256)), dim3(256), 0, c->stream, sw.old, old_n, c->view());
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    sw.done = true;
    dup_forget(c);
    c->solid_tracked = false;
    c->solid_list_fresh = false;
    c->solid_cov = -1;
    c->st.grows++;
    return MC_OK;
}

// Additions that found their region full were parked (TableView::ovf): enlarge the table -- twice as many regions
// split the bins that were crowded together -- and add them again, until none is left.
int drain_parked(mc_ctx *c)
{
    for (int attempt = 0;; attempt++) {
        unsigned long long n = 0;
        HIPCHK(c, hipMemcpyAsync(&n, c->d_ctr + 7, sizeof n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (n == 0) return MC_OK;
        if (int brc = by_key_ready(c)) return brc;  // (the parked additions are keys)
        if (n > mc_ctx::OVF_CAP || attempt >= 8)
            return fail(c, MC_EOVERFLOW, "k-mer table regions keep overflowing (%llu additions parked); pass a capacity_hint "
                        "(distinct k-mers), or set MC_SUPERKMERS=0 for read sets that cover a genome thousands of times", n);
        DevBuf<uint4> tmp;
        HIPCHK(c, tmp.alloc(n));
        HIPCHK(c, hipMemcpyAsync(tmp.p, c->d_ovf, n * sizeof(uint4), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_ctr + 7, 0, sizeof(unsigned long long), c->stream));
        // (minimizer bins: if two doublings did not make room, the crowd shares one bin)
        int rc = (c->mm_k && attempt >= 2) ? to_hash_regions(c, 4) : table_grow(c, c->n_regions * 2);
        if (rc) return rc;
        c->solid_tracked = false;  // (these additions were not watched for crossing the coverage threshold)
        c->solid_list_fresh = false;
        hipLaunchKernelGGL(k_add_parked, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, tmp.p, (uint64_t)n, c->view());
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
}

// Make room for `incoming` more key occurrences: returns how many of them may be inserted by the
// next launch without the load factor passing 0.85 even if every one is a new key.
static int table_reserve(mc_ctx *c, uint64_t incoming, uint64_t *allowed)
{
    int mrc = by_key_ready(c, 2);  // (what follows goes in by key: the direct kernel)
    if (!mrc) mrc = materialize(c);
    if (!mrc) mrc = drain_parked(c);  // (what the previous launch could not place)
    if (mrc) return mrc;
    unsigned long long used;
    uint32_t fatal;
    int rc = read_counters(c, &used, &fatal);
    if (rc) return rc;
    if (fatal) return fail(c, MC_EOVERFLOW, "a k-mer table region filled up (hash skew); table of %llu slots%s",
                           (unsigned long long)c->n_slots(), c->mm_k ? "; MC_SUPERKMERS=0 copes with read sets that cover a genome thousands of times" : "");
    c->n_used_host = used;
    const uint64_t max_launch = 1ull << 26;
    for (;;) {
        const uint64_t cap = c->n_slots();
        const uint64_t soft = (uint64_t)(0.70 * (double)cap), hard = (uint64_t)(0.85 * (double)cap);
        const uint64_t want = std::max<uint64_t>(1, std::min<uint64_t>(incoming, max_launch));
        if (used + want <= hard) {
            *allowed = want;
            return MC_OK;
        }
        const uint64_t room = hard > used ? hard - used : 0;
        if (used < soft && room >= cap / 16) {  // still worth a launch before rebuilding
            *allowed = room;
            return MC_OK;
        }
        rc = table_grow(c, c->n_regions * 2);
        if (rc) return rc;
    }
}

static void launch_count(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_off, uint64_t r0, uint64_t r1)
{
    const int block = 256;
    const int grid = grid_for((r1 - r0) * 64, block, 256 * 8);
    const TableView t = c->view();
    c->solid_tracked = false;
    c->solid_list_fresh = false;
    switch (c->cfg.key_mode) {
    case MC_KEY_PACKED:
        hipLaunchKernelGGL(k_count_reads<KEY_PACKED>, dim3(grid), dim3(block), 0, c->stream, d_words, d_off, r0, r1,
                           c->cfg.k, t, c->cur_ptr_base, (uint32_t)c->cov_hint);
        break;
    case MC_KEY_POLY:
        hipLaunchKernelGGL(k_count_reads<KEY_POLY>, dim3(grid), dim3(block), 0, c->stream, d_words, d_off, r0, r1,
                           c->cfg.k, t, c->cur_ptr_base, (uint32_t)c->cov_hint);
        break;
    default:
        hipLaunchKernelGGL(k_count_reads<KEY_FNV1A>, dim3(grid), dim3(block), 0, c->stream, d_words, d_off, r0, r1,
                           c->cfg.k, t, c->cur_ptr_base, (uint32_t)c->cov_hint);
    }
}

// hipMalloc that gives the pools' idle blocks back to the driver before it reports "out of memory"
hipError_t dev_malloc(mc_ctx *c, void **p, size_t bytes)
{
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        g_table_pool.release(c->cfg.device);
        g_scratch_pool.release(c->cfg.device);
        e = hipMalloc(p, bytes);
    }
    return e;
}

// ------------------------------------------------------------------------------------------ equal keys in different regions (dup_check.h)

// MC_DUP_CHECK=0: no join.  The one switch read on every call rather than at mc_create (switches.h): bench.py turns it off on a
// live context to measure the unchecked rate (config2.value_unchecked).
bool dup_check_on()
{
    const char *e = getenv("MC_DUP_CHECK");
    return !(e && !strcmp(e, "0"));
}

static int dup_small_bufs(mc_ctx *c)
{
    mc_ctx::Dup &D = c->dup;
    if (!D.flags) {
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&D.flags), 4 * sizeof(uint32_t)));
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&D.ctr), 4 * sizeof(unsigned long long)));
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&D.list), mc_ctx::Dup::LIST_CAP * sizeof(unsigned long long)));
        HIPCHK(c, hipMemsetAsync(D.flags, 0, 4 * sizeof(uint32_t), c->stream));
    }
    return MC_OK;
}

// Before the join takes tens of GB beside a table that fills half the device: blocks that sit idle in the process-wide pools go back
// to the driver when less than `need` + 6 GB is free (an allocation that only just fits leaves a later kernel launch nothing for its
// own bookkeeping: configs[2] at full size after other contexts of the process had left their blocks in the pools).
static void dup_make_room(mc_ctx *c, uint64_t need_bytes)
{
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); return; }
    if ((uint64_t)fr >= need_bytes + (6ull << 30)) return;
    (void)hipStreamSynchronize(c->stream);
    g_scratch_pool.release(c->cfg.device);
    g_table_pool.release(c->cfg.device);
}

// The key streams of the join go back to the scratch pool (mc_trim, or a result buffer that does not fit beside them: 84 GB at
// configs[2]'s full size): the next long run's merge kernel gets new ones, a walk's check by key sweeps the table instead.
static void dup_release_streams(mc_ctx *c)
{
    mc_ctx::Dup &D = c->dup;
    const int dev = c->cfg.device;
    (void)hipStreamSynchronize(c->stream);
    g_scratch_pool.put(dev, D.l1_keys, D.l1_words * 8); D.l1_keys = nullptr; D.l1_words = 0;
    g_scratch_pool.put(dev, D.l1_counts, D.l1_counts_cap * 4); D.l1_counts = nullptr; D.l1_counts_cap = 0;
    g_scratch_pool.put(dev, D.l2_own, D.l2_own_words * 8); D.l2_own = nullptr; D.l2_own_words = 0;
    D.l1_armed = false;
    if (D.l2.out_a && D.l2.out_a != reinterpret_cast<uint64_t *>(c->pipe.a_recs)) D.l2_valid = false;  // (streams borrowed from the pipeline stay)
}
// a result buffer for the caller: when the device is full, the join's streams and the pools' idle blocks make room
template <typename T>
static hipError_t alloc_result(mc_ctx *c, DevBuf<T> &b, size_t n)
{
    hipError_t e = b.alloc(n);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        dup_release_streams(c);
        g_scratch_pool.release(c->cfg.device);
        g_table_pool.release(c->cfg.device);
        e = b.alloc(n);
    }
    return e;
}

// capacity of a stream that is expected to take `mean` keys (they come hashed: Poisson, and a little more for the regions' unevenness)
static uint64_t dup_cap(double mean) { return (uint64_t)(mean * 1.12 + 7.0 * std::sqrt(mean) + 64.0); }

// The level-1 streams for a launch of k_p3_long with `grid` workgroups into a table that will hold about `keys` keys.  Not
// getting them is no error: the join then starts with a sweep of the table.
static void dup_arm(mc_ctx *c, double keys, uint32_t grid)
{
    mc_ctx::Dup &D = c->dup;
    D.l1_armed = false;
    if (!dup_check_on() || keys < 1.0) return;
    const std::string keep = c->err;
    if (dup_small_bufs(c)) { c->err = keep; (void)hipGetLastError(); return; }
    const uint32_t nseg = grid + 1;  // (the last one: keys that enter the table outside the merge kernel)
    uint64_t cap = dup_cap(keys / ((double)DUP_B1 * (double)grid));
    if (c->sw.dup_l1_scale != 1.0) cap = std::max<uint64_t>(4, (uint64_t)((double)cap * c->sw.dup_l1_scale));  // (tests: streams that overflow)
    if (D.l1_words < (uint64_t)DUP_B1 * nseg * cap) dup_make_room(c, (uint64_t)DUP_B1 * nseg * cap * 8);
    if (ensure_buf(c, &D.l1_keys, &D.l1_words, (uint64_t)DUP_B1 * nseg * cap) || ensure_buf(c, &D.l1_counts, &D.l1_counts_cap, (uint64_t)DUP_B1 * nseg)) {
        c->err = keep;
        (void)hipGetLastError();
        return;
    }
    if (hipMemsetAsync(D.l1_counts, 0, (uint64_t)DUP_B1 * nseg * sizeof(uint32_t), c->stream) != hipSuccess ||
        hipMemsetAsync(D.flags, 0, sizeof(uint32_t), c->stream) != hipSuccess) { (void)hipGetLastError(); return; }
    D.l1_nseg = nseg;
    D.l1_cap = cap;
    D.l1_armed = true;
}

// The listed keys' slots: one sweep of the table notes them, every one of them then holds the sum of its key's counters
// (dup_check.h); past what the lists take, the table gives up its minimizer bins instead -- equal keys meet in hash-prefix regions.
static int dup_fixup(mc_ctx *c, uint64_t n_listed)
{
    mc_ctx::Dup &D = c->dup;
    if (n_listed > mc_ctx::Dup::LIST_CAP) return to_hash_regions(c, 5);
    uint64_t want = 1024;
    while (want < 4 * n_listed) want <<= 1;
    if (want > D.set_slots) {
        if (D.set.qk) { (void)hipFree(D.set.qk); D.set.qk = nullptr; D.set_slots = 0; }
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&D.set.qk), want * 3 * sizeof(unsigned long long)));
        D.set_slots = want;
    }
    D.set.tot = D.set.qk + D.set_slots;
    D.set.prim = D.set.qk + 2 * D.set_slots;
    D.set.mask = D.set_slots - 1;
    D.set.n_keys = D.ctr + 1;
    const uint64_t tw_want = 8 * n_listed + 64;
    if (tw_want > D.tw_cap) {
        if (D.tw) { (void)hipFree(D.tw); D.tw = nullptr; D.tw_cap = 0; }
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&D.tw), tw_want * sizeof(DupTwin)));
        D.tw_cap = tw_want;
    }
    HIPCHK(c, hipMemsetAsync(D.set.qk, 0xFF, D.set_slots * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(D.set.tot, 0, D.set_slots * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(D.set.prim, 0xFF, D.set_slots * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(D.ctr + 1, 0, 2 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_dupq_build, dim3(grid_for(n_listed, 256)), dim3(256), 0, c->stream, D.list, n_listed, D.set);
    hipLaunchKernelGGL(k_dupq_sweep, dim3(grid_for(c->n_slots(), 256, 256 * 16)), dim3(256), 0, c->stream, c->slots, c->n_slots(), D.set, D.tw, D.ctr + 2, D.tw_cap);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_scratch + 20, D.ctr, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t n_keys = c->h_scratch[21], n_tw = c->h_scratch[22];
    if (n_tw > D.tw_cap) return to_hash_regions(c, 5);  // (a key in more slots than anybody planned for)
    D.n_keys = n_keys;
    D.n_tw = n_tw;
    D.solid_delta = 0;
    if (c->solid_tracked && c->cov_hint > 0 && n_tw) {  // d_ctr[6] counts KEYS at the threshold: once for a merged key, by its sum
        std::vector<DupTwin> tw(n_tw);
        std::vector<unsigned long long> tot(D.set_slots);
        HIPCHK(c, hipMemcpy(tw.data(), D.tw, n_tw * sizeof(DupTwin), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(tot.data(), D.set.tot, D.set_slots * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        std::map<uint32_t, int> own_solid;
        for (const DupTwin &t : tw) own_solid[t.entry] += t.own >= (uint32_t)c->cov_hint ? 1 : 0;
        for (const auto &e : own_solid) D.solid_delta += (tot[e.first] >= (unsigned long long)c->cov_hint ? 1 : 0) - e.second;
    }
    if (n_tw) {
        hipLaunchKernelGGL(k_dup_apply, dim3((unsigned)((n_tw + 255) / 256)), dim3(256), 0, c->stream, c->slots, D.tw, n_tw, D.set, 1);
        if (D.solid_delta) hipLaunchKernelGGL(k_ctr_add, dim3(1), dim3(64), 0, c->stream, c->d_ctr + 6, D.solid_delta);
        HIPCHK(c, hipGetLastError());
        c->solid_list_fresh = false;  // (the merge kernel listed these keys by their own counts, once a slot)
    }
    D.merged = true;
    return MC_OK;
}

// mc_finalize_counts: a table of hash keys in minimizer bins is joined by key (dup_check.h) unless that has been done for the
// table as it is.
int ensure_dups(mc_ctx *c)
{
    mc_ctx::Dup &D = c->dup;
    mc_ctx::Pipe &P = c->pipe;
    if (!hash_bins(c) || c->virgin) { dup_forget(c); return MC_OK; }
    if (D.checked) return MC_OK;
    if (!dup_check_on()) { D.checked = true; D.l1_armed = false; c->st.dup_unchecked = 1; return MC_OK; }
    c->st.dup_unchecked = 0;
    int rc = dup_unmerge(c);  // (only a table whose slots hold their own counts is joined: nothing has touched it since, but say so)
    if (rc) return rc;
    D.n_tw = 0; D.n_keys = 0;
    rc = dup_small_bufs(c);
    if (rc) return rc;
    unsigned long long n_used = 0;
    HIPCHK(c, hipMemcpyAsync(c->h_scratch + 20, c->d_ctr, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    if (D.l1_armed) HIPCHK(c, hipMemcpyAsync(c->h_scratch + 21, D.flags, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    n_used = c->h_scratch[20];
    bool have_l1 = D.l1_armed && (uint32_t)c->h_scratch[21] == 0;
    if (D.l1_armed && !have_l1 && c->sw.ingest_debug)
        fprintf(stderr, "[join] a segment of the merge kernel's key streams overflowed (the table holds %llu keys): the first level by a sweep\n", (unsigned long long)c->h_scratch[20]);
    D.l1_armed = false;  // (whatever happens next: the streams serve one join)
    if (n_used < 2) { D.checked = true; c->st.dup_keys = 0; return MC_OK; }
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    uint64_t n_listed = 0;
    for (int attempt = 0;; attempt++) {
        if (!have_l1) {  // level 1 by a sweep of the table: 1021 workgroups, each a segment of every bucket
            const uint32_t grid = 1021, nseg = grid + 1;  // (a region is 16 rows of the sweep, and a row's slots lie in 16 of the 256 buckets: not a multiple of 16)
            const uint64_t cap = dup_cap((double)n_used / ((double)DUP_B1 * grid));
            if (D.l1_words < (uint64_t)DUP_B1 * nseg * cap) dup_make_room(c, (uint64_t)DUP_B1 * nseg * cap * 8);
            rc = ensure_buf(c, &D.l1_keys, &D.l1_words, (uint64_t)DUP_B1 * nseg * cap);
            if (!rc) rc = ensure_buf(c, &D.l1_counts, &D.l1_counts_cap, (uint64_t)DUP_B1 * nseg);
            if (rc) return rc;
            HIPCHK(c, hipMemsetAsync(D.l1_counts, 0, (uint64_t)DUP_B1 * nseg * sizeof(uint32_t), c->stream));
            HIPCHK(c, hipMemsetAsync(D.flags, 0, sizeof(uint32_t), c->stream));
            D.l1_nseg = nseg;
            D.l1_cap = cap;
            hipLaunchKernelGGL(k_dup_sweep, dim3(grid), dim3(256), 0, c->stream, c->slots, c->n_slots(), DupL1{D.l1_keys, D.l1_counts, nseg, cap, D.flags});
            HIPCHK(c, hipGetLastError());
        }
        // level 2 into sub-buckets of ~1500 keys, every workgroup (bucket, slice of its segments) its own segment of each; the streams
        // borrow the pipeline's idle ones where those are large enough
        const uint32_t slices = std::max<uint32_t>(2u, (D.l1_nseg + DUP_MAX_SLICE_SEGS - 1) / DUP_MAX_SLICE_SEGS);
        if (slices > DUP_MAX_SLICES) return fail(c, MC_EINVAL, "internal: %u key-stream segments a bucket", D.l1_nseg);
        uint32_t f2_lg = 0;
        while (f2_lg < DUP_MAX_F2_LG && (double)n_used / ((double)DUP_B1 * (double)(1u << f2_lg)) > 1800.0) f2_lg++;
        const double per_sub = (double)n_used / ((double)DUP_B1 * (double)(1u << f2_lg));
        const uint64_t cap2 = dup_cap(per_sub / slices);
        const uint64_t per_bucket = ((uint64_t)slices << f2_lg) * cap2, need = per_bucket * DUP_B1;
        DupL2 l2{nullptr, nullptr, DUP_B1, nullptr, f2_lg, slices, cap2, D.flags + 1};
        {
            const uint64_t a_words = P.a_recs ? P.a_recs_cap * 2 : 0, b_words = P.b_recs ? P.b_recs_cap * 2 : 0;
            const uint64_t in_a = std::min<uint64_t>(a_words / per_bucket, DUP_B1);
            if (in_a + std::min<uint64_t>(b_words / per_bucket, DUP_B1) >= DUP_B1 && in_a > 0) {
                l2.out_a = reinterpret_cast<uint64_t *>(P.a_recs);
                l2.out_b = reinterpret_cast<uint64_t *>(P.b_recs);
                l2.split = (uint32_t)in_a;
                c->solid_list_fresh = false;  // (the solid list sat in a_recs)
            } else {
                if (D.l2_own_words < need) dup_make_room(c, need * 8);
                rc = ensure_buf(c, &D.l2_own, &D.l2_own_words, need);
                if (rc) return rc;
                l2.out_a = D.l2_own;
                l2.out_b = D.l2_own;
            }
        }
        const uint64_t n_cnt2 = ((uint64_t)DUP_B1 << f2_lg) * slices;
        rc = ensure_buf(c, &D.l2_counts, &D.l2_counts_cap, n_cnt2);
        if (rc) return rc;
        l2.counts = D.l2_counts;
        HIPCHK(c, hipMemsetAsync(D.flags + 1, 0, sizeof(uint32_t), c->stream));
        HIPCHK(c, hipMemsetAsync(D.ctr, 0, sizeof(unsigned long long), c->stream));
        const DupL1 l1{D.l1_keys, D.l1_counts, D.l1_nseg, D.l1_cap, D.flags};
        hipLaunchKernelGGL(k_dup_scatter, dim3(DUP_B1 * slices), dim3(DUP_THREADS), 0, c->stream, l1, l2);
        const DupOut lst{D.list, D.ctr, mc_ctx::Dup::LIST_CAP};
        // (an LDS set of 2^13 32-bit fingerprints, 32 KB, five workgroups a CU -- or, for sub-buckets beyond 4 500 keys, i.e. a table of
        // more than 1.2 G keys, of 2^15 in a workgroup of 1024 threads; beyond 19 600 keys a sub-bucket goes through the set in passes)
        if (per_sub <= 4500.0) hipLaunchKernelGGL((k_dup_find<13, 256>), dim3(std::min<uint32_t>(DUP_B1 << f2_lg, 256u * 40u)), dim3(256), 0, c->stream, l2, lst);
        else hipLaunchKernelGGL((k_dup_find<15, 1024>), dim3(std::min<uint32_t>(DUP_B1 << f2_lg, 256u * 8u)), dim3(1024), 0, c->stream, l2, lst);
        HIPCHK(c, hipGetLastError());
        D.l2 = l2;
        HIPCHK(c, hipMemcpyAsync(c->h_scratch + 20, D.ctr, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->h_scratch + 21, D.flags, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        uint32_t fl[2];
        memcpy(fl, c->h_scratch + 21, sizeof fl);
        if (!fl[0] && !fl[1]) {
            n_listed = c->h_scratch[20];
            if (c->sw.ingest_debug) fprintf(stderr, "[join] %llu keys, level 1 by %s, %u slices, f2_lg %u, cap2 %llu, k_dup_find<%s>, %llu listed\n", n_used,
                                                   have_l1 ? "merge streams" : "sweep", slices, f2_lg, (unsigned long long)cap2, per_sub <= 4500.0 ? "13, 256" : "15, 1024",
                                                   (unsigned long long)n_listed);
            break;
        }
        // a stream overflowed (the merge kernel's were sized by a hint that fell short, or the keys are far from evenly spread): once
        // more from a sweep, whose streams are sized by the number of keys the table holds
        if (attempt >= 1 || !have_l1)
            return fail(c, MC_EOVERFLOW, "internal: the key streams of the duplicate-key join overflowed (%llu keys)", n_used);
        if (c->sw.ingest_debug) fprintf(stderr, "[join] the merge kernel's key streams overflowed (sized for %.0f keys, the table holds %llu): once more from a sweep\n",
                                               c->cfg.capacity_hint ? (double)c->cfg.capacity_hint : D.expected_keys, n_used);
        have_l1 = false;
    }
    if (n_listed) {
        rc = dup_fixup(c, n_listed);
        if (rc) return rc;
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->st.dup_ms += ms;
    c->st.dup_checks++;
    c->st.dup_keys = D.n_keys;
    D.checked = true;
    D.l2_valid = hash_bins(c);  // (the streams of level 2 hold the table's keys by key until the pipeline takes its buffers back)
    return MC_OK;
}

// What a function of the counting driver (from here to add_records_binned, and the run-cutting loops behind it) may return
// besides MC_OK and the negative MC_* errors.  Each function's comment lists the ones it returns; a caller handles each by name,
// and none leaves through the C ABI (abi_result).
enum RunOutcome : int {
    RUN_LOST_RECORDS = 1,      // the streams lost records and nothing was merged: the caller counts the batch another way
    RUN_NOT_BINNED = 2,        // the table's level-1 buckets are not unions of the fine ones: the caller takes the flat stream
    RUN_BATCH_AGAIN = 3,       // the (empty) table was too small and has been replaced by one of the right size: the batch once more
    RUN_NOT_LONG = 4,          // not as long records: the caller takes the per-window form
    RUN_BEYOND_LEAF_BITS = 5,  // the wanted table is beyond the reach of the records' ten leaf bits: the first level again, two arrays
    RUN_RESPLIT = 6,           // the run must be cut again: the table has left its minimizer bins under it and takes one record a window now
};
static const char *const RUN_OUTCOME_NAMES[] = {"ok", "lost records", "not binned", "batch again", "not as long records", "beyond the leaf bits", "cut the run again"};

// a driver result on its way out through the C ABI: every outcome has been handled by then
static int abi_result(mc_ctx *c, int rc)
{
    return rc > 0 ? fail(c, MC_EINVAL, "internal: the counting driver's outcome %d (%s) was left unhandled", rc, rc <= RUN_RESPLIT ? RUN_OUTCOME_NAMES[rc] : "unknown") : rc;
}

struct PipePlan {
    uint32_t b1 = 0, b2 = 1, g = 0;  // b1 level-1 buckets of b2 leaves each (counts, not bits); a leaf covers 2^g regions
    uint64_t np1 = 0, n_leaves = 0, cap1 = 0, cap2 = 0, spill_cap = 0, wb = 0;
    uint32_t nseg1 = PT_SEGMENTS;  // segments of every level-1 bucket = workgroups of the level-1 kernel
    uint32_t pieces = 1;           // one key a window: the reads go through P1 / P2 in this many pieces (cap1, cap2: per piece); P3 sees `pieces` segments per leaf
    bool sk = false;  // the streams hold super-k-mer records; capacities are in records
    // compact: the streams hold 16-byte units and no pointer arrays (count_pipeline.h k_sk1w_extract<false, true>, k_sk2_scatter_compact):
    // every level-1 segment = workgroup took chunk_tiles consecutive tiles, the first of them at base position pos0
    bool compact = false;
    uint32_t chunk_tiles = 0;
    uint64_t pos0 = 0;
    bool guessed = false;  // no capacity hint vouches for the table's size: pipe_finish merges a sample of the leaves first
    // vleaf: compact records written before the table's size is known (a first batch without a hint): their leaf field holds the TEN
    // bits of the bin word below the level-1 bucket's -- 2^10 leaves a bucket whatever the table --, the table is then given a power
    // of two of regions (pipe_resize_by_sample) and the second level drops the bits it does not need
    bool vleaf = false;
    bool lng = false;      // long records (count_long.h): two 16-byte words a record in every stream
    // listed: there is no first level -- the records lie in the caller's buffer (in_recs / in_ptrs) in pieces that are in level-1 bucket
    // order already (the binned exchange), and the second level reads segment sg of a bucket from pipe.skb_seg_start[bucket * nseg1 + sg]
    bool listed = false;
    const uint4 *in_recs = nullptr;
    const uint32_t *in_ptrs = nullptr;
    SpillView sp{};
    SkSpill sks{};
    // What the caller of pipe_finish has done already, and what it can do afterwards:
    double ms1 = 0;           // time of the level-1 scatter that filled the a_* buckets, where the caller waited for it
    // p1_pending: the caller recorded ev_t[0], enqueued P1 and did not wait: P2 and P3 follow on the stream at once and
    // the host hears of all three together (a host round trip between two kernels leaves the device idle for tens of us)
    bool p1_pending = false;
    bool p2_done = false;     // the caller ran P2 itself, piece by piece behind P1 (ms2 = its time)
    double ms2 = 0;
    bool may_rerun = false;   // the caller can run the batch again (RUN_BATCH_AGAIN)
};

// What a caller asks of pipe_prepare
struct PipeRequest {
    uint64_t n_records = 0;        // != 0: the key occurrences travel as (an estimated) n_records super-k-mer records
    uint32_t nseg1 = PT_SEGMENTS;  // PipePlan::nseg1
    uint32_t pieces = 1;           // PipePlan::pieces
    // compact_tiles != 0: the caller's level-1 kernel is k_sk1w_extract over this many tiles in one piece and can write the compact
    // form: taken up when the rest of the run allows it (a second level through the staged kernel, one region per leaf, segments
    // short enough for 22-bit positions)
    uint64_t compact_tiles = 0;
    bool lng = false;              // PipePlan::lng
    // listed: PipePlan::listed -- no first-level streams (the solid list alone may want pipe.a_recs), the caller has filled
    // pipe.seg_counts1 (np1 x nseg1 fill levels) and pipe.skb_seg_start already
    bool listed = false;
    // level2_only: the level-1 scatter has run and the table has since been replaced by one of another size (pipe_resize_by_sample):
    // the plan of the second level and of the merge is made again for it; level 1 (buckets, segments, their fill levels, the
    // spill list) stays as it is -- the caller has checked that the new table splits into the same level-1 buckets
    bool level2_only = false;
};

// first_read[t] for every tile (count_pipeline.h): by the reads where they are short, by a search per tile otherwise
static void launch_tile_first(mc_ctx *c, const uint64_t *offs, uint64_t nr, uint64_t n_tiles, uint32_t *out, uint32_t tile_size)
{
    if (nr && n_tiles <= 8 * nr)  // (a read spans a few tiles at most on average: its thread's loop is short)
        hipLaunchKernelGGL(k_tile_first_read_by_reads, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, c->stream, offs, nr, n_tiles, out, tile_size);
    else
        hipLaunchKernelGGL(k_tile_first_read, dim3((unsigned)((n_tiles + 255) / 256)), dim3(256), 0, c->stream, offs, nr, n_tiles, out, tile_size);
}

// the control words of a pipeline run, cleared in one launch (flags: 4 words + the 64-bit spill counter behind them)
__global__ void __launch_bounds__(256) k_pipe_reset(uint32_t *seg_counts1, uint64_t n1, uint32_t *cursors2, uint64_t n2, uint32_t *leaf_state,
                                                    uint32_t *leaf_new, uint64_t n_leaves, uint32_t *flags)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x, stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = t; i < n1; i += stride) seg_counts1[i] = 0;
    for (uint64_t i = t; i < n2; i += stride) cursors2[i] = 0;
    for (uint64_t i = t; i < n_leaves; i += stride) { leaf_state[i] = 0; leaf_new[i] = 0; }
    if (flags && t < 6) flags[t] = 0;
}

// How a table of c->n_regions regions splits into level-1 buckets and leaves (records: the super-k-mer pipeline; else keys): *n_leaves
// leaves of 2^*g regions each, *np1 level-1 buckets.  Returns what is wrong, or null.
static const char *plan_levels(const mc_ctx *c, bool records, uint64_t *n_leaves_out, uint32_t *g_out, uint64_t *np1_out)
{
    // leaves: the regions themselves up to 2^20 of them (2^18 when keys travel, not records), else 2^g regions per leaf;
    // level-1 buckets: up to 512, each of m2 <= 1024 (512) leaves (regions_for made the numbers divide)
    uint64_t n_leaves = c->n_regions;
    uint32_t g = 0;
    // (2^20 leaves at most in either form: a leaf that covers 2^g regions is swept 2^(g+1) times by the merge kernel -- with 2^18
    // leaves the 137 GB table of configs[2] had g = 3, and two thirds of that run were those sweeps)
    const uint32_t max_b2 = records ? PT_MAX_LEAVES2 : PT_MAX_BUCKETS_KEYS;  // (super-k-mer records: k_sk2_scatter; keys: k_p2_scatter)
    const uint32_t max_b1_big = records ? PT_MAX_BUCKETS1_SK : PT_MAX_BUCKETS_KEYS;  // (1024 level-1 buckets only when 512 do not do)
    while (n_leaves > (uint64_t)max_b1_big * max_b2) { n_leaves >>= 1; g++; }
    if ((n_leaves << g) != c->n_regions) return "the table's regions do not split into leaves";
    if (n_leaves < 4) return "partitioned counting needs at least 4 table regions";
    // (512 level-1 buckets while 512 x max_b2 leaves do, then 1024, then -- super-k-mer records only -- 2048)
    uint64_t np1 = PT_MAX_BUCKETS;
    while (np1 < max_b1_big && n_leaves > np1 * max_b2) np1 *= 2;
    np1 = std::min<uint64_t>(n_leaves, np1);
    while (n_leaves % np1) np1--;  // (a power of two, or 512 dividing a multiple of 512)
    if (n_leaves / np1 > max_b2) return "the leaves do not fit two scatter levels";
    *n_leaves_out = n_leaves; *g_out = g; *np1_out = np1;
    return nullptr;
}

// Makes sure the table can take a batch of wb key occurrences: with a capacity hint that still holds the table was sized for
// it; without one assume every eighth occurrence is a new key at most.  Either way the merge kernel
// reports regions that would overflow and the table is grown then.
static int pipe_reserve(mc_ctx *c, uint64_t wb, bool *hint_holds_out)
{
    unsigned long long used;
    uint32_t fatal;
    int rc = read_counters(c, &used, &fatal);
    if (rc) return rc;
    if (fatal) return fail(c, MC_EOVERFLOW, "a k-mer table region filled up (hash skew)");
    c->n_used_host = used;
    const bool hint_holds = c->cfg.capacity_hint && used < c->cfg.capacity_hint;
    if (!hint_holds && c->n_slots() < wb / 4) {
        const uint64_t want = regions_for(c, (uint64_t)(((double)used + (double)wb / 8.0) / 0.5));
        if (want > c->n_regions) {
            rc = table_grow(c, want);
            if (rc) return rc;
        }
    }
    *hint_holds_out = hint_holds;
    return MC_OK;
}

// Table capacity check, scratch buffers and cursors for one run of the partitioned pipeline over
// `wb` key occurrences, as `rq` asks.  Returns MC_OK or an error, no outcome.
static int pipe_prepare(mc_ctx *c, uint64_t wb, PipePlan *pl, const PipeRequest &rq)
{
    const uint64_t n_records = rq.n_records, compact_tiles = rq.compact_tiles;
    const uint32_t nseg1 = rq.nseg1;
    uint32_t pieces = rq.pieces;
    const bool lng = rq.lng, listed = rq.listed, level2_only = rq.level2_only;
    pl->lng = lng;
    pl->listed = listed;
    const uint64_t rw = lng ? 2 : 1;  // 16-byte words a record
    pl->nseg1 = nseg1;
    pl->pieces = pieces;
    mc_ctx::Pipe &P = c->pipe;
    c->solid_list_fresh = false;  // the pipeline buffers are about to be reused
    c->dup.l2_valid = false;      // (... and with them what the key join left there)
    if (!level2_only) {
        bool hint_holds;
        int rc = pipe_reserve(c, wb, &hint_holds);
        if (rc) return rc;
        pl->guessed = !hint_holds;
    }
    uint64_t n_leaves, np1;
    uint32_t g;
    if (const char *why = plan_levels(c, n_records != 0, &n_leaves, &g, &np1)) return fail(c, MC_EINVAL, "internal: %s (%llu table regions)", why, (unsigned long long)c->n_regions);
    pl->b1 = (uint32_t)np1;               // level-1 buckets
    pl->b2 = (uint32_t)(n_leaves / np1);  // leaves per bucket; 1: the level-1 buckets already are the leaves, no P2
    pl->g = g;
    pl->wb = wb;
    pl->np1 = np1;
    pl->n_leaves = n_leaves;
    pl->sk = n_records != 0;
    if (pl->b2 <= 1) pl->pieces = pieces = 1;  // (no second level to overlap with)
    if (!level2_only) {
        const uint64_t chunk = (compact_tiles + nseg1 - 1) / std::max<uint32_t>(nseg1, 1);
        // (not where pipe_resize_by_sample may replace the table between the two levels: the leaf numbers inside the records
        // are those of the table the first level saw)
        pl->compact = compact_tiles && c->sw.sk_compact && pl->sk && pl->b2 > 1 && pl->b2 <= (1u << (32 - SKC_REL_BITS)) && g == 0 &&
                      chunk * p1w_tile(false) <= (1ull << SKC_REL_BITS) && !(pl->guessed && c->virgin);
        // ... unless the table can be given a power of two of regions once the batch's size is known: 512 buckets of 2 .. 1024 leaves
        pl->vleaf = false;
        if (!pl->compact && !lng && c->sw.sk_vleaf && !c->no_vleaf && compact_tiles && c->sw.sk_compact && pl->sk && g == 0 && chunk * p1w_tile(false) <= (1ull << SKC_REL_BITS) &&
            pl->guessed && c->virgin && c->mm_k > 0 && np1 == PT_MAX_BUCKETS && c->n_regions <= (uint64_t)PT_MAX_BUCKETS * 1024) {
            uint64_t r2 = 2 * PT_MAX_BUCKETS;
            while (r2 < c->n_regions) r2 *= 2;
            if (r2 != c->n_regions) {  // (a virgin table: nothing to move)
                table_release(c, c->slots, c->slots_bytes);
                c->slots = nullptr;
                int rc = table_alloc(c, r2);
                if (rc) return rc;
                n_leaves = r2;
                pl->b2 = (uint32_t)(n_leaves / np1);
                pl->n_leaves = n_leaves;
            }
            pl->compact = pl->vleaf = true;
        }
        // (long records keep the leaf in their second word: 32 bits of position)
        // (... and the bin word, so the table may still be replaced between the levels: a virgin table without a hint qualifies)
        if (lng) pl->compact = compact_tiles && pl->sk && pl->b2 > 1 && pl->b2 <= 1024 && g == 0 && chunk * P1L_TILE < (1ull << 32) &&
                               !(pl->guessed && !c->virgin);
        pl->chunk_tiles = pl->compact ? (uint32_t)chunk : 0;
        if (listed) pl->compact = true;  // (the listed second level leaves the pointer in the record's first word too: no pointer arrays behind it)
    }
    const uint64_t units = (pl->sk ? n_records : wb) / pieces + (pieces > 1 ? 1024 : 0);  // records in the streams (of one piece)
    // (long records into 2^20 leaves and more -- configs[2] at full size, where the table leaves the streams 130 GB --: tighter streams)
    const bool tight = lng && n_leaves >= (1ull << 20);
    pl->cap1 = (uint64_t)((double)units / (double)pl->np1 / (double)nseg1 * (tight ? 1.12 : 1.25)) + (pl->sk ? 64 : 256);  // per segment
    const double mean_leaf = (double)units / (double)pl->n_leaves;
    // (records of one locus come in clumps -- one per read covering it -- so leaves vary more than Poisson)
    const double sig2 = pl->sk ? (tight ? 12.0 : 32.0) : 8.0;
    pl->cap2 = (uint64_t)(mean_leaf * 1.15 + sig2 * std::sqrt(mean_leaf) + 64.0);  // (a spilled record also costs the solid list, P3Emit)
    pl->spill_cap = pl->sk ? std::max<uint64_t>(units / 16, 1u << 16) : std::max<uint64_t>(wb / 64, 1u << 20);
    if ((!listed && pl->np1 * nseg1 * pl->cap1 >= 0xFFFFFFFFull) || (uint64_t)pl->b2 * pl->cap2 * pieces >= 0xFFFFFFFFull)
        return fail(c, MC_EINVAL, "internal: partitioned batch too large for 32-bit bucket indices");
    // (np1, n_leaves as computed above)
    int rc;
    uint64_t dummy;
#define ENSURE(ptr, capvar, need) do { rc = ensure_buf(c, &(ptr), &(capvar), (need)); if (rc) return rc; } while (0)
    if (pl->sk) {
        if (!level2_only && !listed) ENSURE(P.a_recs, P.a_recs_cap, np1 * nseg1 * pl->cap1 * rw);
        if (listed && c->want_list) ENSURE(P.a_recs, P.a_recs_cap, units + units / 4);  // (the solid list's room, as a first level would have left it)
        // (long records into a table nothing vouches for: the second level's buffer first serves as the sample's scratch set, 64 MB)
        if (pl->b2 > 1) ENSURE(P.b_recs, P.b_recs_cap, std::max<uint64_t>(n_leaves * pl->cap2 * rw, lng && pl->guessed ? (1ull << 22) : 0));
        if (!level2_only) ENSURE(P.spill_recs, P.spill_recs_cap, pl->spill_cap * rw);
    } else {
        { uint64_t cap = P.a_cap; ENSURE(P.a_keys, cap, np1 * nseg1 * pl->cap1); P.a_cap = cap; }
        { uint64_t cap = P.b_cap; ENSURE(P.b_keys, cap, n_leaves * pl->cap2 * pieces); P.b_cap = cap; }
        { uint64_t cap = P.spill_cap; ENSURE(P.spill_keys, cap, pl->spill_cap); dummy = P.spill_cap; ENSURE(P.spill_hints, dummy, pl->spill_cap); P.spill_cap = cap; }
    }
    if (!pl->compact && !lng) {  // (the compact form keeps the read pointers inside the records)
        if (!level2_only && !listed) ENSURE(P.a_hints, P.a_hints_cap, np1 * nseg1 * pl->cap1 * pieces);
        ENSURE(P.b_hints, P.b_hints_cap, n_leaves * pl->cap2 * pieces);
    }
    if (!level2_only) ENSURE(P.seg_counts1, P.segs1_cap, np1 * nseg1 * pieces);
    ENSURE(P.cursors2, P.cursors2_cap, n_leaves * pieces);
    { uint64_t cap = P.leaves_cap; ENSURE(P.leaf_state, cap, n_leaves); dummy = P.leaves_cap; ENSURE(P.leaf_new, dummy, n_leaves); P.leaves_cap = cap; }
#undef ENSURE
    if (!P.flags) {  // four flags and, behind them, the spill counter: cleared by one fill, read by one copy
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&P.flags), 4 * sizeof(uint32_t) + sizeof(unsigned long long)));
        P.spill_count = reinterpret_cast<unsigned long long *>(P.flags + 4);
    }
    // (one launch clears all five: a fill each, 10 us apart, was 60 us in front of every run)
    hipLaunchKernelGGL(k_pipe_reset, dim3(256), dim3(256), 0, c->stream, P.seg_counts1, level2_only || listed ? 0 : np1 * nseg1 * pieces, P.cursors2, n_leaves * pieces,
                       P.leaf_state, P.leaf_new, n_leaves, level2_only ? nullptr : P.flags);
    HIPCHK(c, hipGetLastError());
    pl->sp = SpillView{P.spill_keys, P.spill_hints, P.spill_count, pl->spill_cap, P.flags};
    pl->sks = SkSpill{P.spill_recs, P.spill_count, pl->spill_cap, P.flags};
    return MC_OK;
}

// The occurrences the merge kernels handed on (count_pipeline.h ovf_push: no room within their stretch of the region) go
// into the table through the direct kernel, which follows the table's region chain; entries of leaves that were not
// committed are dropped (those leaves are merged again).  Only after a launch that has been over EVERY leaf: the regions
// behind must hold valid slots.  *n_parked (may be null): how many there were.
static int pipe_drain_handed_on(mc_ctx *c, uint64_t n_listed, bool lng = false)
{
    mc_ctx::Pipe &P = c->pipe;
    const uint64_t n = std::min<uint64_t>(n_listed, mc_ctx::OVF_CAP);
    if (n == 0) return MC_OK;
    // The direct kernel parks what IT cannot place (no room in the whole chain: a table far too small) in the same list:
    // the entries are moved aside first and the list starts again from 0 -- read and appended to in one launch, the
    // additions parked by the drain itself were wiped with the list's counter (15 000 of 21 M keys lost in a soak case with a
    // capacity hint a quarter of what the reads held).
    int rc = ensure_buf(c, &c->d_ovf_tmp, &c->ovf_tmp_cap, (uint64_t)mc_ctx::OVF_CAP);
    if (!rc) rc = ensure_buf(c, &c->d_ovf_leaf_tmp, &c->ovf_leaf_tmp_cap, (uint64_t)mc_ctx::OVF_CAP);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_ovf_tmp, c->d_ovf, n * sizeof(uint4), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_ovf_leaf_tmp, c->d_ovf_leaf, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_ctr + 7, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_add_parked, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, c->d_ovf_tmp, n, c->view(), c->d_ovf_leaf_tmp, P.leaf_state,
                       lng && hash_bins(c) ? 1 : 0, lng && hash_bins(c) ? c->dup_l1_view() : DupL1{nullptr, nullptr, 0, 0, nullptr});
    HIPCHK(c, hipGetLastError());
    c->solid_tracked = false;  // (these additions were not watched for crossing the coverage threshold)
    c->solid_list_fresh = false;
    c->st.spill_keys += n;
    // what the drain parked: into a table of twice the regions, until nothing is left (pipe_finish sees the new size)
    for (int attempt = 0;; attempt++) {
        unsigned long long m = 0;
        HIPCHK(c, hipMemcpyAsync(c->h_scratch + 29, c->d_ctr + 7, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        m = c->h_scratch[29];
        if (m == 0) return MC_OK;
        if (m > mc_ctx::OVF_CAP || attempt >= 6)
            return fail(c, MC_EOVERFLOW, "k-mer table regions keep overflowing (%llu additions parked); pass a capacity_hint (distinct k-mers)", m);
        HIPCHK(c, hipMemcpyAsync(c->d_ovf_tmp, c->d_ovf, m * sizeof(uint4), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_ctr + 7, 0, sizeof(unsigned long long), c->stream));
        rc = table_grow(c, c->n_regions * 2);
        if (rc) return rc;
        hipLaunchKernelGGL(k_add_parked, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, c->d_ovf_tmp, (uint64_t)m, c->view());
        HIPCHK(c, hipGetLastError());
    }
}

// Nothing vouches for the table's size (no capacity hint) and it holds nothing yet: the level-1 scatter has just run, and
// its first bucket is a fair sample of the batch -- 1 / np1 of the minimizer bins, whatever the table's size.  Its
// distinct k-mers are counted into a scratch set, the table is replaced by one of the size they call for, and the second
// level and the merge are planned for that table: the batch is scattered once (before, the merge of 1024 leaves told the
// size, and then everything ran again: 31 ms of counting on configs[1] against 19 with a hint).
// Outcomes: RUN_BEYOND_LEAF_BITS (pl.vleaf only), RUN_NOT_LONG (pl.lng only).
static int pipe_resize_by_sample(mc_ctx *c, PipePlan &pl, uint64_t n_records)
{
    mc_ctx::Pipe &P = c->pipe;
    if (!(pl.sk && pl.guessed && c->virgin && pl.b2 > 1 && c->mm_k)) return MC_OK;
    constexpr uint64_t SET_SLOTS = 1ull << 23;  // 64 MB of P.b_recs, which the second level has not touched yet
    if (P.b_recs_cap * sizeof(uint4) < SET_SLOTS * 8) return MC_OK;
    uint64_t *set = reinterpret_cast<uint64_t *>(P.b_recs);
    HIPCHK(c, hipMemsetAsync(set, 0xFF, SET_SLOTS * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_ctr + 2, 0, sizeof(unsigned long long), c->stream));
    if (pl.lng)
        hipLaunchKernelGGL(k_skl_sample_distinct, dim3(pl.nseg1), dim3(256), 0, c->stream, P.a_recs, P.seg_counts1, pl.cap1, c->cfg.k, set, SET_SLOTS - 1,
                           c->d_ctr + 2);
    else
        hipLaunchKernelGGL(k_sk_sample_distinct, dim3(pl.nseg1), dim3(256), 0, c->stream, P.a_recs, P.seg_counts1, pl.cap1, c->cfg.k, set, SET_SLOTS - 1,
                           c->d_ctr + 2);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_scratch + 24, c->d_ctr + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_scratch + 25, P.flags, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint32_t fl[4];
    memcpy(fl, c->h_scratch + 25, sizeof fl);
    if (fl[0]) return MC_OK;  // (records were lost: pipe_finish sees the flag too and the batch is counted another way)
    const double est = (double)c->h_scratch[24] * (double)pl.np1 * 1.1 + 1024.0;
    c->dup.expected_keys = est;  // (what the key streams of dup_check.h are sized by in a context without a hint)
    if (est > 0.45 * (double)SET_SLOTS * (double)pl.np1) return MC_OK;  // (the scratch set was too full to count in: the old way)
    uint64_t want = regions_for(c, mm_slots_for(c, est, 0.36));
    if (pl.vleaf) {
        // a power of two of regions: the smaller of the two around `want` while it keeps the table under load 0.45 (0.36 x 1.25),
        // else the larger (load 0.23 at least); beyond 2^19 regions the records' ten leaf bits do not reach: the caller runs the
        // first level again in the two-array form
        uint64_t p2 = 2 * PT_MAX_BUCKETS;
        while (p2 * 2 <= want) p2 *= 2;
        if (est > 0.45 * (double)(p2 << c->sb)) p2 *= 2;
        uint64_t reach = (uint64_t)PT_MAX_BUCKETS * 1024;
        reach = std::min<uint64_t>(reach, c->sw.sk_vleaf_max_regions);  // (tests: the way back at a small size)
        if (p2 > reach) return RUN_BEYOND_LEAF_BITS;
        want = p2;
    }
    if (pl.lng && est > 0.40 * (double)(want << c->sb)) return RUN_NOT_LONG;  // (hash keys need their bins roomy, mc_create: the caller takes the per-window form)
    if (pl.lng && want <= c->n_regions) { pl.guessed = false; return MC_OK; }  // (the table it was created with holds the batch)
    if (c->sw.ingest_debug) fprintf(stderr, "[count] first bucket: %llu distinct k-mers, %.0f M expected in all; table of %llu regions, %llu wanted\n",
                     (unsigned long long)c->h_scratch[24], est / 1e6, (unsigned long long)c->n_regions, (unsigned long long)want);
    if (want != c->n_regions) {
        // the new table must split into the level-1 buckets the records are in
        if (want % pl.np1 || want / pl.np1 > PT_MAX_LEAVES2 || want / pl.np1 < 2) return MC_OK;
        table_release(c, c->slots, c->slots_bytes);
        c->slots = nullptr;
        int rc = table_alloc(c, want);
        if (rc) return rc;
        c->st.grows++;
        HIPCHK(c, hipMemsetAsync(c->d_ctr + 6, 0, sizeof(unsigned long long), c->stream));  // keys at the coverage threshold: none yet
        PipePlan p2 = pl;
        PipeRequest rq;
        rq.n_records = n_records;
        rq.nseg1 = pl.nseg1;
        rq.lng = pl.lng;
        rq.level2_only = true;
        rc = pipe_prepare(c, pl.wb, &p2, rq);
        if (rc) return rc;
        if (p2.np1 != pl.np1 || p2.cap1 != pl.cap1 || p2.g != 0) return fail(c, MC_EINVAL, "internal: the resized table does not keep the level-1 buckets");
        pl = p2;
    } else {
        // (the scratch set sat in the second level's buffer: nothing of it is read before it is written)
    }
    pl.guessed = false;  // the table was sized by what the batch holds
    return MC_OK;
}

constexpr uint32_t P3_MAX_GRID = 256 * 2 * 4 * (D2_THREADS < P3_THREADS ? P3_THREADS / D2_THREADS : 1);  // workgroups of a merge launch at most

// One run of pipe_finish, as its stages (below, in the order they run) leave it to one another.  The plan goes with it: a stage that
// times level 1 or runs level 2 says so there (p1_pending, p2_done, ms1, ms2).
struct PipeRun {
    PipePlan &pl;
    // P3 reads the leaves: P2's output (one segment each), or P1's buckets directly when there is no second level
    const void *lk = nullptr;
    const uint32_t *lh = nullptr, *lc = nullptr;  // (lh null: the compact form, the pointers sit in the records)
    uint64_t lcap = 0;
    uint32_t lseg = 0;
    int p3_grid = 0;
    P3Emit emit{};
    bool virgin0 = false;           // the table held nothing before this run
    uint32_t flags[3] = {0, 0, 0};  // read back: records were lost, a region overflowed, a segment of the solid list overflowed
    unsigned long long n_spill = 0, n_handed_on = 0;
    double ms3 = 0, ms4 = 0;  // the merge, the spill drain
};

// Which merge kernel takes the leaves and with which template arguments: the debug line and the launch both go by this.
struct MergeChoice {
    bool lng, dedup;            // k_p3_long<long_k>, k_p3_dedup<virgin, one_gpu, k31>, or neither: k_p3_merge
    bool virgin, one_gpu, k31;
    bool general_behind;        // k_p3_merge right behind k_p3_dedup
    int long_k;
};
static MergeChoice merge_choice(const mc_ctx *c, const PipeRun &R, int virgin)
{
    const int k = c->cfg.k;
    MergeChoice m{};
    m.lng = R.pl.lng;
    // super-k-mer records, one region and one segment per leaf: the merge kernel that merges identical records first
    // (count_pipeline.h k_p3_dedup; MC_P3_DEDUP=0: the general kernel)
    m.dedup = !m.lng && R.pl.sk && R.pl.g == 0 && R.lseg == 1 && c->sw.p3_dedup;
    m.virgin = virgin;
    m.one_gpu = c->ptr_tries == 1 && (R.emit.recs == nullptr || !(c->solid_tracked && c->cov_hint > 0));
    m.k31 = m.virgin && m.one_gpu && k == 31;
    // (k_p3_dedup leaves the leaves of more than DD_MAX_CAP records alone: where the capacity allows such leaves, the general
    // kernel follows at once and takes what is left -- it skips the merged ones, ~20 us when that is all of them)
    m.general_behind = m.dedup && R.lcap > DD_MAX_CAP;
    // (built for the k-mer lengths people run -- constant shifts, trip counts and powers of 5 --, and for any other from the argument)
    m.long_k = k == 63 || k == 55 || k == 47 || k == 41 ? k : 0;
    return m;
}

// the merge kernel over the first `leaves` leaves
static void launch_merge(mc_ctx *c, const PipeRun &R, uint32_t leaves, int grid, int virgin)
{
    mc_ctx::Pipe &P = c->pipe;
    const PipePlan &pl = R.pl;
    const int k = c->cfg.k;
    const MergeChoice m = merge_choice(c, R, virgin);
#define P3_ARGS R.lk, R.lh, R.lc, R.lcap, R.lseg, leaves, pl.g, c->view(), virgin, P.leaf_state, P.leaf_new, P.flags + 1, \
                (uint32_t)(c->solid_tracked ? c->cov_hint : 0), c->d_ctr + 6, k, R.emit, c->ptr_tries, P.flags
#define P3D_ARGS static_cast<const uint4 *>(R.lk), R.lh, R.lc, R.lcap, leaves, c->view(), P.leaf_state, P.leaf_new, P.flags + 1, \
                 (uint32_t)(c->solid_tracked ? c->cov_hint : 0), c->d_ctr + 6, k, R.emit, c->ptr_tries, P.flags
#define P3L_ARGS static_cast<const uint4 *>(R.lk), R.lc, R.lcap, leaves, c->view(), virgin, P.leaf_state, P.leaf_new, P.flags + 1, \
                 (uint32_t)(c->solid_tracked ? c->cov_hint : 0), c->d_ctr + 6, k, R.emit, P.flags, c->dup_l1_view()
    if (c->sw.ingest_debug) {  // (every run of the merge stage: which kernel takes the leaves)
        char name[64];
        if (m.lng) snprintf(name, sizeof name, "k_p3_long");
        else if (m.dedup) snprintf(name, sizeof name, "k_p3_dedup<%d, %d, %d>", m.virgin ? 1 : 0, m.one_gpu ? 1 : 0, m.k31 ? 1 : 0);
        else snprintf(name, sizeof name, "k_p3_merge<%s>", pl.sk ? "true" : "false");
        fprintf(stderr, "[count] merge: %s over %u leaves, lcap %llu, ptr_tries %u, general kernel behind it: %s\n", name, leaves,
                (unsigned long long)R.lcap, c->ptr_tries, m.general_behind ? "yes" : "no");
    }
    if (m.lng) {
        if (m.long_k == 63) hipLaunchKernelGGL(k_p3_long<63>, dim3(grid), dim3(P3_THREADS), 0, c->stream, P3L_ARGS);
        else if (m.long_k == 55) hipLaunchKernelGGL(k_p3_long<55>, dim3(grid), dim3(P3_THREADS), 0, c->stream, P3L_ARGS);
        else if (m.long_k == 47) hipLaunchKernelGGL(k_p3_long<47>, dim3(grid), dim3(P3_THREADS), 0, c->stream, P3L_ARGS);
        else if (m.long_k == 41) hipLaunchKernelGGL(k_p3_long<41>, dim3(grid), dim3(P3_THREADS), 0, c->stream, P3L_ARGS);
        else hipLaunchKernelGGL(k_p3_long<0>, dim3(grid), dim3(P3_THREADS), 0, c->stream, P3L_ARGS);
    } else if (m.dedup) {
        if (m.k31) hipLaunchKernelGGL((k_p3_dedup<true, true, true>), dim3(grid), dim3(D2_THREADS), 0, c->stream, P3D_ARGS);
        else if (m.virgin && m.one_gpu) hipLaunchKernelGGL((k_p3_dedup<true, true>), dim3(grid), dim3(D2_THREADS), 0, c->stream, P3D_ARGS);
        else if (m.virgin) hipLaunchKernelGGL((k_p3_dedup<true, false>), dim3(grid), dim3(D2_THREADS), 0, c->stream, P3D_ARGS);
        else if (m.one_gpu) hipLaunchKernelGGL((k_p3_dedup<false, true>), dim3(grid), dim3(D2_THREADS), 0, c->stream, P3D_ARGS);
        else hipLaunchKernelGGL((k_p3_dedup<false, false>), dim3(grid), dim3(D2_THREADS), 0, c->stream, P3D_ARGS);
        if (m.general_behind) hipLaunchKernelGGL(k_p3_merge<true>, dim3(grid), dim3(P3_THREADS), 0, c->stream, P3_ARGS);
    } else if (pl.sk) {
        hipLaunchKernelGGL(k_p3_merge<true>, dim3(grid), dim3(P3_THREADS), 0, c->stream, P3_ARGS);
    } else {
        hipLaunchKernelGGL(k_p3_merge<false>, dim3(grid), dim3(P3_THREADS), 0, c->stream, P3_ARGS);
    }
#undef P3_ARGS
#undef P3D_ARGS
#undef P3L_ARGS
}
static void launch_merge_all(mc_ctx *c, const PipeRun &R) { launch_merge(c, R, (uint32_t)R.pl.n_leaves, R.p3_grid, c->virgin ? 1 : 0); }

// the second scatter level: the level-1 buckets (or the caller's listed records) into their leaves
static void launch_level2(mc_ctx *c, const PipePlan &pl)
{
    mc_ctx::Pipe &P = c->pipe;
    const uint64_t np1 = pl.np1;
    static bool told = false;  // (once a process)
    if (c->sw.ingest_debug && !told) {  // (where the streams lie: the second level's time differs between processes that differ in nothing else)
        told = true;
        fprintf(stderr, "[count] level-1 stream %p (%llu records a segment), level-2 stream %p (%llu a leaf), table %p\n", (void *)P.a_recs,
                (unsigned long long)pl.cap1, (void *)P.b_recs, (unsigned long long)pl.cap2, (void *)c->slots);
    }
    if (pl.lng)
        hipLaunchKernelGGL((k_sk2_scatter_compact<2, 2>), dim3((unsigned)np1), dim3(PT_THREADS), 0, c->stream, P.a_recs, pl.cap1,
                           P.seg_counts1, (uint32_t)np1, pl.b2, P.cursors2, pl.cap2, P.b_recs, pl.sks, pl.nseg1, c->cur_ptr_base, pl.pos0,
                           (uint64_t)pl.chunk_tiles * P1L_TILE);
    else if (pl.sk && pl.compact && !pl.listed)
        hipLaunchKernelGGL(k_sk2_scatter_compact<MC_SK2C_ITEMS>, dim3((unsigned)np1), dim3(PT_THREADS), 0, c->stream, P.a_recs, pl.cap1,
                           P.seg_counts1, (uint32_t)np1, pl.b2, P.cursors2, pl.cap2, P.b_recs, pl.sks, pl.nseg1, c->cur_ptr_base, pl.pos0,
                           (uint64_t)pl.chunk_tiles * p1w_tile(false), pl.vleaf ? 10u - (uint32_t)__builtin_ctz(pl.b2) : 0u);
    else if (pl.listed)
        hipLaunchKernelGGL((k_sk2_scatter_staged<MC_SK2_ITEMS, true, false>), dim3((unsigned)np1), dim3(PT_THREADS), 0, c->stream, pl.in_recs, pl.in_ptrs, (uint64_t)0,
                           P.seg_counts1, (uint32_t)np1, pl.b1, pl.b2, P.cursors2, pl.cap2, P.b_recs, nullptr, pl.sks, pl.nseg1, P.skb_seg_start, nullptr);
    else if (pl.sk)
        hipLaunchKernelGGL(k_sk2_scatter_staged<MC_SK2_ITEMS>, dim3((unsigned)np1), dim3(PT_THREADS), 0, c->stream, P.a_recs, P.a_hints, pl.cap1,
                           P.seg_counts1, (uint32_t)np1, pl.b1, pl.b2, P.cursors2, pl.cap2, P.b_recs, P.b_hints, pl.sks, pl.nseg1);
    else
        hipLaunchKernelGGL(k_p2_scatter, dim3((unsigned)np1), dim3(PT_THREADS), 0, c->stream, P.a_keys, P.a_hints, pl.cap1,
                           P.seg_counts1, (uint32_t)np1, pl.b1, pl.b2, P.cursors2, pl.cap2, P.b_keys, P.b_hints, pl.sp, c->mm_k);
}

// How many distinct keys the batch holds, judged by the first sample_leaves leaves as the merge kernel left them (a table that held
// nothing before).  MC_OK: the table holds the batch.  Outcomes: RUN_BATCH_AGAIN, the table has been replaced by one that does.
static int resize_for_batch(mc_ctx *c, const PipePlan &pl, uint64_t sample_leaves)
{
    mc_ctx::Pipe &P = c->pipe;
    std::vector<uint32_t> st(sample_leaves), nw(sample_leaves);
    HIPCHK(c, hipMemcpy(st.data(), P.leaf_state, sample_leaves * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(nw.data(), P.leaf_new, sample_leaves * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint64_t merged = 0, added = 0;
    for (uint64_t i = 0; i < sample_leaves; i++)
        if (st[i]) { merged++; added += nw[i]; }
    {   // occurrences the merged leaves handed on to the next region (ovf_push) are keys too, nearly all of them new
        unsigned long long ho = 0;
        HIPCHK(c, hipMemcpy(&ho, c->d_ctr + 7, sizeof ho, hipMemcpyDeviceToHost));
        added += std::min<uint64_t>(ho, mc_ctx::OVF_CAP);
        if (ho > mc_ctx::OVF_CAP) added += (uint64_t)((double)(ho - mc_ctx::OVF_CAP));
    }
    // (the leaves that overflowed hold more than the average: at least a full leaf each)
    const uint64_t per_full = (uint64_t)REGION_SLOTS << pl.g;
    const double est = ((double)added + (double)(sample_leaves - merged) * (double)per_full * 1.5) * ((double)pl.n_leaves / (double)sample_leaves) * 1.1 + 1024.0;
    const double load = c->mm_k ? 0.36 : 0.6;
    if (merged == sample_leaves && est <= (c->mm_k ? 0.5 : 0.7) * (double)c->n_slots()) return MC_OK;  // it fits: carry on
    uint64_t want = regions_for(c, c->mm_k ? mm_slots_for(c, est, load) : (uint64_t)(est / load));
    if (want <= c->n_regions) want = regions_for(c, c->n_slots() * 2);
    if (c->sw.ingest_debug) fprintf(stderr, "[count] table too small: %llu of %llu sampled leaves merged, %llu keys in them: %.0f M keys expected; new table %.1f GB\n",
                     (unsigned long long)merged, (unsigned long long)sample_leaves, (unsigned long long)added, est / 1e6, (double)(want << c->sb) * 16 / 1e9);
    table_release(c, c->slots, c->slots_bytes);
    c->slots = nullptr;
    int r = table_alloc(c, want);  // (fresh device memory comes zeroed by the driver at ~30 GB/s: 0.7 s for 22 GB, once)
    if (r) return r;
    c->st.grows++;
    HIPCHK(c, hipMemsetAsync(c->d_ctr + 6, 0, 2 * sizeof(unsigned long long), c->stream));  // keys at the coverage threshold: none yet; nothing handed on
    return RUN_BATCH_AGAIN;
}

// What the run has timed goes into the statistics; finished: it counted the batch (else it ends early, and the caller goes on with it)
static void book_run(mc_ctx *c, const PipeRun &R, bool finished)
{
    c->st.p1_ms += R.pl.ms1;
    c->st.p2_ms += R.pl.ms2;
    c->st.p3_ms += R.ms3;
    c->st.count_ms += R.pl.ms1 + R.pl.ms2 + R.ms3 + R.ms4;
    c->st.count_total_ms += R.pl.ms1 + R.pl.ms2 + R.ms3 + R.ms4;
    if (!finished) return;
    c->st.spill_keys += R.n_spill;
    c->st.count_launches++;
    c->st.windows += R.pl.wb;
}

// Nothing vouches for the table's size (no capacity hint): the second level, then the merge of 1024 leaves first -- the bin word is
// a mixed hash, any range of leaves is a fair sample -- to see what they hold.  Costs a host round trip; a whole merge into a
// table that turns out too small costs seven times the run.  Outcomes: RUN_LOST_RECORDS, RUN_BATCH_AGAIN (times booked).
static int merge_sample(mc_ctx *c, PipeRun &R)
{
    mc_ctx::Pipe &P = c->pipe;
    const uint64_t K = 1024;
    HIPCHK(c, hipEventRecord(c->ev_t[1], c->stream));
    launch_level2(c, R.pl);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_t[2], c->stream));
    launch_merge(c, R, (uint32_t)K, (int)K, 1);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(R.flags, P.flags, sizeof R.flags, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float f = 0;
    if (R.pl.p1_pending) { HIPCHK(c, hipEventElapsedTime(&f, c->ev_t[0], c->ev_t[1])); R.pl.ms1 = f; R.pl.p1_pending = false; }
    HIPCHK(c, hipEventElapsedTime(&f, c->ev_t[1], c->ev_t[2]));
    R.pl.ms2 += f;
    R.pl.p2_done = true;
    if (R.flags[0]) return RUN_LOST_RECORDS;  // (nothing was merged)
    const int rc = resize_for_batch(c, R.pl, K);
    if (rc == RUN_BATCH_AGAIN) book_run(c, R, false);  // (level 1 and level 2: the sample's merge is not timed)
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(P.flags + 1, 0, sizeof(uint32_t), c->stream));
    return MC_OK;
}

// P2 (where the run has one and it has not run yet) and the first P3 back to back.  The capacities of the streams are estimates
// (and a few heavy keys can fill a bucket's spill list alone): P3 looks at the "records lost" flag itself and merges nothing when
// it is set, so that the caller can still count the batch another way.  Outcomes: RUN_LOST_RECORDS.
static int scatter_and_merge(mc_ctx *c, PipeRun &R)
{
    mc_ctx::Pipe &P = c->pipe;
    const bool level2 = R.pl.b2 > 1 && !R.pl.p2_done;
    HIPCHK(c, hipEventRecord(c->ev_t[1], c->stream));
    if (level2) {
        launch_level2(c, R.pl);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(c->ev_t[2], c->stream));
    launch_merge_all(c, R);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_t[3], c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_scratch + 16, P.flags, 4 * sizeof(uint32_t) + sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_scratch + 19, c->d_ctr + 7, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(R.flags, c->h_scratch + 16, sizeof R.flags);
    R.n_spill = c->h_scratch[18];
    R.n_handed_on = c->h_scratch[19];
    float f = 0;
    if (R.pl.p1_pending) { HIPCHK(c, hipEventElapsedTime(&f, c->ev_t[0], c->ev_t[1])); R.pl.ms1 = f; }
    if (level2) { HIPCHK(c, hipEventElapsedTime(&f, c->ev_t[1], c->ev_t[2])); R.pl.ms2 += f; }
    if (R.flags[0]) return RUN_LOST_RECORDS;  // (nothing was merged)
    HIPCHK(c, hipEventElapsedTime(&f, c->ev_t[2], c->ev_t[3]));
    R.ms3 += f;
    c->virgin = false;
    return MC_OK;
}
// Minimizer bins that no number of regions can hold: regions by the key's hash from here on, and the leaves that were not merged
// go through the direct kernel, as many at a time as the table has room for.
static int add_unmerged_leaves(mc_ctx *c, const PipeRun &R)
{
    mc_ctx::Pipe &P = c->pipe;
    const PipePlan &pl = R.pl;
    const uint64_t n_leaves = pl.n_leaves;
    const uint32_t lseg = R.lseg;
    const int k = c->cfg.k;
    int rc = to_hash_regions(c, 4);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(P.leaf_new, 0, n_leaves * sizeof(uint32_t), c->stream));  // (n_used was recounted)
    std::vector<uint32_t> st(n_leaves), cnt(n_leaves * (uint64_t)lseg);
    HIPCHK(c, hipMemcpy(st.data(), P.leaf_state, n_leaves * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(cnt.data(), R.lc, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint32_t lo_leaf = 0;
    while (lo_leaf < n_leaves) {
        uint64_t allowed, need = 0;
        uint32_t hi_leaf = lo_leaf;
        rc = table_reserve(c, 1ull << 26, &allowed);
        if (rc) return rc;
        while (hi_leaf < n_leaves) {
            uint64_t w = 0;
            if (!st[hi_leaf])
                for (uint32_t sg = 0; sg < lseg; sg++) w += std::min<uint64_t>(cnt[(uint64_t)hi_leaf * lseg + sg], R.lcap) * (pl.lng ? SKL_MAX_WINDOWS : SK_MAX_WINDOWS);
            if (hi_leaf > lo_leaf && need + w > allowed) break;
            need += w;
            hi_leaf++;
        }
        if (need > allowed) {  // a single leaf above what one launch may add: make room for it
            rc = table_reserve(c, need, &allowed);
            if (rc) return rc;
            if (need > allowed) return fail(c, MC_EOVERFLOW, "internal: a leaf of %llu k-mer occurrences does not fit one launch", (unsigned long long)need);
        }
        if (need && pl.lng)
            hipLaunchKernelGGL(k_skl_add_unmerged, dim3(std::min<uint32_t>(hi_leaf - lo_leaf, 4096u)), dim3(256), 0, c->stream,
                               static_cast<const uint4 *>(R.lk), R.lc, R.lcap, lo_leaf, hi_leaf, P.leaf_state, k, c->view());
        else if (need)
            hipLaunchKernelGGL(k_sk_add_unmerged, dim3(std::min<uint32_t>(hi_leaf - lo_leaf, 4096u)), dim3(256), 0, c->stream,
                               static_cast<const uint4 *>(R.lk), R.lh, R.lc, R.lcap, lseg, lo_leaf, hi_leaf, P.leaf_state, k, c->view());
        HIPCHK(c, hipGetLastError());
        lo_leaf = hi_leaf;
    }
    return MC_OK;
}

// What the merge kernels handed on goes in, and while a region overflowed: a table of twice the regions and P3 again.
static int merge_until_no_overflow(mc_ctx *c, PipeRun &R)
{
    mc_ctx::Pipe &P = c->pipe;
    PipePlan &pl = R.pl;
    const uint64_t n_leaves = pl.n_leaves;
    int rc;
    for (int attempt = 0;; attempt++) {
        if (attempt > 0) {
            rc = timed(c, &R.ms3, [&] { launch_merge_all(c, R); });
            if (rc) return rc;
            c->virgin = false;
            HIPCHK(c, hipMemcpy(R.flags, P.flags, sizeof R.flags, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(&R.n_handed_on, c->d_ctr + 7, sizeof R.n_handed_on, hipMemcpyDeviceToHost));
        }
        if (R.flags[0]) return fail(c, MC_EOVERFLOW, "internal: spill list of the partitioned counting pipeline overflowed");
        // (every leaf has been merged or, where the hand-on list ran full, left as a valid region: the list can go in)
        const bool bins_before = hash_bins(c);
        rc = pipe_drain_handed_on(c, R.n_handed_on, pl.lng);
        if (rc) return rc;
        R.n_handed_on = 0;
        if (pl.lng && bins_before && !hash_bins(c))  // (the drain moved the table to hash-prefix regions: n_used was recounted, the merged leaves' keys included)
            HIPCHK(c, hipMemsetAsync(P.leaf_new, 0, n_leaves * sizeof(uint32_t), c->stream));
        if (!pl.lng && (n_leaves << pl.g) < c->n_regions) {  // (the drain doubled the table: a leaf covers more regions now; n_used was recounted)
            while ((n_leaves << pl.g) < c->n_regions) pl.g++;
            HIPCHK(c, hipMemsetAsync(P.leaf_new, 0, n_leaves * sizeof(uint32_t), c->stream));
        }
        if (R.flags[2]) R.emit.recs = nullptr;  // a segment of the solid list overflowed: the BFS set-up sweeps the table instead
        if (!R.flags[1]) return MC_OK;
        if (pl.lng || attempt >= 6 || pl.g >= 5) {
            // (long records: a table of hash keys in minimizer bins cannot be rebuilt with more bins -- it gives them up at the first leaf that fails)
            if (!(pl.sk && (c->mm_k || pl.lng)))
                return fail(c, MC_EOVERFLOW, "k-mer table regions keep overflowing; pass a capacity_hint (distinct k-mers)");
            R.emit.recs = nullptr;
            return add_unmerged_leaves(c, R);
        }
        rc = table_grow(c, c->n_regions * 2);
        if (rc) return rc;
        pl.g++;
        HIPCHK(c, hipMemsetAsync(P.flags + 1, 0, sizeof(uint32_t), c->stream));
        // the rebuild recounted n_used, keys of the leaves merged so far included
        HIPCHK(c, hipMemsetAsync(P.leaf_new, 0, n_leaves * sizeof(uint32_t), c->stream));
    }
}

// what did not fit its bucket goes through the direct kernel (n_spill: read with the flags, scatter_and_merge)
static int drain_spill(mc_ctx *c, PipeRun &R)
{
    mc_ctx::Pipe &P = c->pipe;
    const PipePlan &pl = R.pl;
    const unsigned long long n_spill = R.n_spill;
    const int k = c->cfg.k;
    const uint32_t thr = (uint32_t)(c->solid_tracked ? c->cov_hint : 0);
    int rc;
    uint64_t i = 0;
    if (n_spill && pl.lng && hash_bins(c)) {
        // (the table was sized by the hint that let this run take long records, and the direct path's usual preparations would
        // move it out of its minimizer bins: the few records that found no room in the streams go in as they are, each to its bin)
        rc = timed(c, &R.ms4, [&] {
            hipLaunchKernelGGL(k_skl_add_records, dim3(grid_for(n_spill, 256)), dim3(256), 0, c->stream, P.spill_recs, (uint64_t)n_spill, k, c->view(), thr, c->d_ctr + 6,
                               c->dup_l1_view());
        });
        if (rc) return rc;
        i = n_spill;
        unsigned long long parked = 0;  // what found no room in its bin's chain is a key without a leaf: only a by-key table takes it
        HIPCHK(c, hipMemcpy(&parked, c->d_ctr + 7, sizeof parked, hipMemcpyDeviceToHost));
        if (parked) { rc = drain_parked(c); if (rc) return rc; }
    }
    while (i < n_spill) {
        uint64_t allowed;
        rc = table_reserve(c, (n_spill - i) * (pl.lng ? SKL_MAX_WINDOWS : pl.sk ? SK_MAX_WINDOWS : 1), &allowed);
        if (rc) return rc;
        const uint64_t m = std::min<uint64_t>(pl.lng ? std::max<uint64_t>(allowed / SKL_MAX_WINDOWS, 1) : pl.sk ? std::max<uint64_t>(allowed / SK_MAX_WINDOWS, 1) : allowed, n_spill - i);
        rc = timed(c, &R.ms4, [&] {
            if (pl.lng)
                hipLaunchKernelGGL(k_skl_add_records, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, P.spill_recs + 2 * i, m, k, c->view(), thr, c->d_ctr + 6,
                                   DupL1{nullptr, nullptr, 0, 0, nullptr});  // (by key: the table is in hash-prefix regions by now)
            else if (pl.sk)
                hipLaunchKernelGGL(k_sk_add_records, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, P.spill_recs + i, (const uint32_t *)nullptr, m, k,
                                   c->view(), thr, c->d_ctr + 6);
            else
                hipLaunchKernelGGL(k_add_keys_hint, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, P.spill_keys + i,
                                   P.spill_hints + i, m, c->view(), thr, c->d_ctr + 6);
        });
        if (rc) return rc;
        i += m;
    }
    return MC_OK;
}

// P2, P3 (with the retry after growing the table), spill drain and bookkeeping of a run that pipe_prepare planned and whose level 1
// the caller has run or enqueued (PipePlan: ms1, p1_pending, p2_done, ms2, may_rerun).
// Outcomes: RUN_LOST_RECORDS (the streams overflowed even their spill list); RUN_BATCH_AGAIN (pl.may_rerun only).
static int pipe_finish(mc_ctx *c, PipePlan &pl)
{
    mc_ctx::Pipe &P = c->pipe;
    const bool level2 = pl.b2 > 1;
    PipeRun R{pl};
    R.virgin0 = c->virgin;
    R.emit = P3Emit{nullptr, nullptr, 0, P.flags + 2};
    R.lk = pl.sk ? (level2 ? (const void *)P.b_recs : (const void *)P.a_recs) : (level2 ? (const void *)P.b_keys : (const void *)P.a_keys);
    R.lh = pl.compact ? nullptr : (level2 ? P.b_hints : P.a_hints);
    R.lc = level2 ? P.cursors2 : P.seg_counts1;
    R.lcap = level2 ? pl.cap2 : pl.cap1;
    R.lseg = level2 ? pl.pieces : pl.nseg1;
    // The solid list (P3Emit): super-k-mer form with the leaves in b_recs, so that a_recs is free to take it, and a
    // threshold to track.  Each P3 workgroup owns a segment.
    R.p3_grid = (int)std::min<uint64_t>(pl.n_leaves, P3_MAX_GRID);
    if (pl.sk && level2 && c->mm_k && c->solid_tracked && c->cov_hint > 0 && c->want_list) {
        if (!P.emit_counts) HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&P.emit_counts), P3_MAX_GRID * sizeof(uint32_t)));
        HIPCHK(c, hipMemsetAsync(P.emit_counts, 0, P3_MAX_GRID * sizeof(uint32_t), c->stream));
        R.emit.recs = P.a_recs;
        R.emit.counts = P.emit_counts;
        R.emit.seg_cap = std::min<uint64_t>(P.a_recs_cap / (uint64_t)R.p3_grid, 0xFFFFFFF0ull);
    }
    // hash keys in minimizer bins: the merge kernel also leaves every key it writes back in the key streams of dup_check.h, sized
    // by what is known about the number of keys the table will hold
    if (pl.lng && hash_bins(c) && pl.g == 0)
        dup_arm(c, c->cfg.capacity_hint ? (double)c->cfg.capacity_hint : c->dup.expected_keys, (uint32_t)R.p3_grid);
    else
        c->dup.l1_armed = false;
    int rc = MC_OK;
    if (pl.may_rerun && R.virgin0 && pl.guessed && pl.n_leaves >= 8192 && level2 && !R.pl.p2_done) rc = merge_sample(c, R);
    if (!rc) rc = scatter_and_merge(c, R);
    if (rc) return rc;
    if (R.flags[1] && R.virgin0 && pl.may_rerun) {
        // The table held nothing before this run and is too small for it (no capacity hint, or a poor one).  Rebuilding it
        // by rehashing and merging the leaves that are left in two sweeps each costs 40 times the run (785 against 19 ms
        // on configs[1]); what the merged leaves added says how many distinct keys the batch holds, so: a fresh table of
        // the right size, and the caller runs the batch again.
        rc = resize_for_batch(c, pl, pl.n_leaves);
        if (rc != RUN_BATCH_AGAIN) return rc ? rc : fail(c, MC_EOVERFLOW, "internal: a leaf overflowed in a table that should hold the batch");
        book_run(c, R, false);
        return RUN_BATCH_AGAIN;
    }
    rc = merge_until_no_overflow(c, R);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sum_leaf_new, dim3(64), dim3(256), 0, c->stream, P.leaf_new, (uint32_t)pl.n_leaves, c->d_ctr);
    HIPCHK(c, hipGetLastError());
    rc = drain_spill(c, R);
    if (rc) return rc;
    if (R.emit.recs && !R.n_spill) {  // (spilled records went into the table behind P3's back)
        c->solid_list_fresh = true;
        c->solid_list_segs = (uint32_t)R.p3_grid;
        c->solid_list_segcap = R.emit.seg_cap;
    }
    book_run(c, R, true);
    return MC_OK;
}

static void launch_p1_reads(mc_ctx *c, const uint64_t *d_words, const uint64_t *offs, uint64_t nr, uint64_t base0,
                            uint64_t end_abs, uint64_t n_tiles_abs, const uint32_t *tile_first, uint32_t b1, uint32_t *cursors,
                            uint64_t cap, uint64_t *out_keys, uint32_t *out_hints, const SpillView &sp, int owners_mode,
                            const uint64_t *bases)
{   // owners_mode: 0 = hash-prefix buckets (counting), 1 = count per owner, 2 = scatter per owner at `bases`
    // counting mode: exactly PT_SEGMENTS workgroups, each owns one segment of every bucket
    const int grid = owners_mode == 0 ? PT_SEGMENTS
                                      : (int)std::min<uint64_t>(std::max<uint64_t>(n_tiles_abs - base0 / PT_TILE, 1), 256);
    const int k = c->cfg.k;
    // (owner modes: the kernel's mm_k chooses the owner rule -- 0: mc_key_owner, the key's own hash; k: the owner of the key's minimizer)
    const int p1_mm_k = owners_mode == 0 ? c->mm_k : (c->extract_by_minimizer ? k : 0);
#define P1_ARGS d_words, offs, nr, base0, end_abs, n_tiles_abs, tile_first, k, b1, cursors, cap, out_keys, out_hints, c->d_ctr + 1, sp, bases, p1_mm_k, c->cur_ptr_base
#define P1_LAUNCH(MODE)                                                                                                  \
    do {                                                                                                                 \
        if (owners_mode == 0)                                                                                            \
            hipLaunchKernelGGL((k_p1_extract_scatter<MODE, false, false>), dim3(grid), dim3(PT_THREADS), 0, c->stream, P1_ARGS); \
        else if (owners_mode == 1)                                                                                       \
            hipLaunchKernelGGL((k_p1_extract_scatter<MODE, true, true>), dim3(grid), dim3(PT_THREADS), 0, c->stream, P1_ARGS);   \
        else                                                                                                             \
            hipLaunchKernelGGL((k_p1_extract_scatter<MODE, true, false>), dim3(grid), dim3(PT_THREADS), 0, c->stream, P1_ARGS);  \
    } while (0)
    switch (c->cfg.key_mode) {
    case MC_KEY_PACKED: P1_LAUNCH(KEY_PACKED); break;
    case MC_KEY_POLY: P1_LAUNCH(KEY_POLY); break;
    default: P1_LAUNCH(KEY_FNV1A);
    }
#undef P1_LAUNCH
#undef P1_ARGS
}

// super-k-mer records expected from `nr` reads with `wb` windows: runs of windows sharing a minimizer average
// (w + 1) / 2 windows in random sequence (w = k - SK_M + 1 minimizer candidates per window); sequencing errors
// and the 16-window limit cut some short (x 1.5 covers 1-2 % errors), and every read ends one
static uint64_t sk_records_bound(const mc_ctx *c, uint64_t wb, uint64_t nr)
{
    return (uint64_t)((double)wb * 2.0 / (double)(c->cfg.k - SK_M + 2) * 1.5) + 2 * nr + 1024;
}

// One batch of reads [r0, r1) through the partitioned pipeline (count_pipeline.h).  wb = its windows,
// base0 / end_abs = read_offsets[r0] / read_offsets[r1].  Outcomes: RUN_BATCH_AGAIN, which add_reads_partitioned handles, and
// RUN_RESPLIT (nothing of the batch was counted), which it passes on to the loops that cut the runs.
static int add_reads_partitioned_once(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_off, uint64_t r0, uint64_t r1,
                                      uint64_t base0, uint64_t end_abs, uint64_t wb);
static uint64_t max_run_bases(const mc_ctx *c, double windows_per_base);
static int add_reads_partitioned(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_off, uint64_t r0, uint64_t r1,
                                 uint64_t base0, uint64_t end_abs, uint64_t wb)
{
    // RUN_BATCH_AGAIN from the pipeline is handled here: once more, into the table that replaced the empty one
    unsigned long long empty0 = 0;  // occurrences of the key that looks like a free slot (hash keys only): counted apart, by P1
    const bool hashed = c->cfg.key_mode != MC_KEY_PACKED;
    if (hashed) {
        HIPCHK(c, hipMemcpyAsync(&empty0, c->d_ctr + 1, sizeof empty0, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    for (int run = 0;; run++) {
        const int rc = add_reads_partitioned_once(c, d_words, d_off, r0, r1, base0, end_abs, wb);
        if (rc != RUN_BATCH_AGAIN) return rc;  // (MC_OK, an error or RUN_RESPLIT)
        if (run >= 8) return fail(c, MC_EOVERFLOW, "k-mer table regions keep overflowing; pass a capacity_hint (distinct k-mers)");  // (a rerun multiplies the table by 4.5 at least)
        if (hashed) {
            HIPCHK(c, hipMemcpyAsync(c->d_ctr + 1, &empty0, sizeof empty0, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    }
}
// the reads [r0, r1) through the direct kernel, as many at a time as the table has room for
static int count_batch_direct(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_off, uint64_t r0, uint64_t r1, uint64_t base0, uint64_t end_abs,
                              uint64_t wb)
{
    const uint64_t nr = r1 - r0;
    uint64_t r = r0;
    while (r < r1) {
        uint64_t allowed;
        int rc = table_reserve(c, wb, &allowed);
        if (rc) return rc;
        const uint64_t step = std::max<uint64_t>(1, std::min<uint64_t>(r1 - r, allowed / std::max<uint64_t>(1, (end_abs - base0) / nr + 1)));
        double ms = 0;
        rc = timed(c, &ms, [&] { launch_count(c, d_words, d_off, r, r + step); });
        if (rc) return rc;
        c->st.count_ms += ms;
        c->st.count_total_ms += ms;
        c->st.count_launches++;
        r += step;
    }
    c->st.windows += wb;
    return MC_OK;
}

// One run as long records (count_long.h).  Outcomes: RUN_NOT_LONG (the run does not qualify: the caller moves the table to
// hash-prefix regions and takes the per-window form), RUN_LOST_RECORDS (from pipe_finish, which may not ask for the batch again here).
static int add_reads_long(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_off, uint64_t r0, uint64_t r1, uint64_t base0, uint64_t end_abs,
                          uint64_t wb)
{
    mc_ctx::Pipe &P = c->pipe;
    const uint64_t nr = r1 - r0;
    if (c->cfg.key_mode != MC_KEY_POLY || c->cfg.k < SKL_MIN_K || c->cfg.k > SKL_MAX_K) return RUN_NOT_LONG;
    unsigned long long used;
    uint32_t fatal;
    int rc = dup_unmerge(c);  // (slots that hold their keys' sums get their own counts back: the merge kernel adds to whichever slot a bin holds)
    if (!rc) rc = read_counters(c, &used, &fatal);
    if (rc) return rc;
    // (only a table sized for what it will hold -- by a hint that still holds, or, holding nothing yet, by a sample of this batch: it cannot grow)
    if (fatal || !((c->cfg.capacity_hint && used < c->cfg.capacity_hint) || c->virgin)) return RUN_NOT_LONG;
    PipePlan pl;
    // (bin words of the two smallest hashes: runs two thirds as long -- 10.6 windows a record for 15.9 on configs[2]'s reads)
    const uint64_t n_records = c->mm_k < 0 ? sk_records_bound(c, wb, nr) * 8 / 5 : sk_records_bound(c, wb, nr);
    const uint64_t n_tiles_abs = (end_abs + P1L_TILE - 1) / P1L_TILE;
    PipeRequest rq;
    rq.n_records = n_records;
    rq.nseg1 = (uint32_t)P1W_SEGMENTS;
    rq.compact_tiles = n_tiles_abs - base0 / P1L_TILE;
    rq.lng = true;
    rc = pipe_prepare(c, wb, &pl, rq);
    if (rc) return rc;
    if (!pl.compact || !hash_bins(c)) return RUN_NOT_LONG;
    const uint64_t *offs = d_off + r0;
    rc = ensure_buf(c, &P.tile_first, &P.tiles1_cap, n_tiles_abs);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev_t[0], c->stream));  // (no wait here: pipe_finish enqueues the second level and the merge right behind)
    launch_tile_first(c, offs, nr, n_tiles_abs, P.tile_first, P1L_TILE);
    pl.pos0 = base0 / P1L_TILE * P1L_TILE;
    if (c->sw.ingest_debug)
        fprintf(stderr, "[count] long records: %u buckets x %u leaves, %u tiles a segment from base %llu, %llu records expected\n", pl.b1, pl.b2, pl.chunk_tiles,
                (unsigned long long)pl.pos0, (unsigned long long)n_records);
    const SklSpill sp{P.spill_recs, P.spill_count, pl.spill_cap, P.flags};
    hipLaunchKernelGGL(k_skl_extract, dim3(P1W_SEGMENTS), dim3(P1W_THREADS), 0, c->stream, d_words, offs, nr, base0, end_abs, n_tiles_abs, P.tile_first,
                       c->cfg.k, pl.b1, P.seg_counts1, pl.cap1, P.a_recs, sp, pl.chunk_tiles, c->mm_k < 0 ? 1u : 0u);
    HIPCHK(c, hipGetLastError());
    rc = pipe_resize_by_sample(c, pl, n_records);  // (no hint: the table is sized by what the first bucket holds; RUN_NOT_LONG: its bins would be too full)
    if (rc == RUN_BEYOND_LEAF_BITS) return fail(c, MC_EINVAL, "internal: long records have no leaf bits for a table to be beyond (PipePlan::vleaf)");
    if (rc) return rc;  // (an error or RUN_NOT_LONG)
    if (pl.guessed) return RUN_NOT_LONG;  // (no sample could be taken: nothing vouches for the table)
    c->st.long_runs++;
    pl.p1_pending = true;
    return pipe_finish(c, pl);  // (pl.may_rerun is not set: no RUN_BATCH_AGAIN)
}

static int add_reads_partitioned_once(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_off, uint64_t r0, uint64_t r1,
                                      uint64_t base0, uint64_t end_abs, uint64_t wb)
{
    mc_ctx::Pipe &P = c->pipe;
    PipePlan pl;
    const uint64_t nr = r1 - r0;
    if (hash_bins(c)) {
        int lrc = add_reads_long(c, d_words, d_off, r0, r1, base0, end_abs, wb);
        if (lrc == RUN_LOST_RECORDS) return count_batch_direct(c, d_words, d_off, r0, r1, base0, end_abs, wb);  // (nothing was merged)
        if (lrc != RUN_NOT_LONG) return lrc;  // (MC_OK or an error)
        lrc = to_hash_regions(c, 3);
        if (lrc) return lrc;
        // The run was cut for long records (2^34 bases); one record a window takes far less (39 M reads of 150 bases
        // at k = 63 pass the 32-bit bucket indices).  The caller cuts what is left again, for the table as it is now.
        if (end_abs - base0 > max_run_bases(c, (double)wb / (double)std::max<uint64_t>(end_abs - base0, 1))) return RUN_RESPLIT;
    }
    const uint64_t n_records = c->mm_k ? sk_records_bound(c, wb, nr) : 0;
    // One key per window (hash keys, short k): a large batch goes through the two scatter levels in pieces of ~2^30 windows
    // that REUSE the level-1 buffers, one after the other on the same stream, so that a run of twice the windows fits
    // the same scratch and the whole table is rewritten half as often (max_run_bases).
    // (only where the memory is needed: at 0.9 G windows two pieces cost 55 ms against 35 ms in one)
    // (super-k-mer records go in one piece)
    constexpr uint32_t sk_tile = p1w_tile(false);  // k_sk1w_extract<false, ..>, both forms
    PipeRequest rq;
    rq.n_records = n_records;
    rq.nseg1 = n_records ? (uint32_t)P1W_SEGMENTS : (uint32_t)PT_SEGMENTS;
    rq.pieces = n_records || wb < (3ull << 29) ? 1u : (uint32_t)std::min<uint64_t>(8, (wb + (1ull << 30) - 1) >> 30);
    rq.compact_tiles = n_records ? (end_abs + sk_tile - 1) / sk_tile - base0 / sk_tile : 0;
    int rc = pipe_prepare(c, wb, &pl, rq);
    if (rc) return rc;
    pl.may_rerun = true;
    const uint32_t pieces = pl.pieces;
    const uint64_t *offs = d_off + r0;
    // tiles are cut over the absolute base positions [0, end_abs); the ones before base0 hold no read of ours
    const uint32_t tile_size = pl.sk ? sk_tile : (uint32_t)PT_TILE;
    const uint64_t n_tiles_abs = (end_abs + tile_size - 1) / tile_size;
    rc = ensure_buf(c, &P.tile_first, &P.tiles1_cap, n_tiles_abs);
    if (rc) return rc;
    if (pieces > 1) {
        const uint64_t t_first = base0 / tile_size, per = (n_tiles_abs - t_first + pieces - 1) / pieces;
        // (the two levels alternate on one stream; an event behind every kernel books each level's time where it belongs --
        // round 3 booked both under the first level and reported k_p2_scatter: 0.0 for configs[2] at full size)
        for (uint32_t i = 0; i < 2 * pieces; i++)
            if (!c->ev_seq[i]) HIPCHK(c, hipEventCreate(&c->ev_seq[i]));
        HIPCHK(c, hipEventRecord(c->ev0, c->stream));
        launch_tile_first(c, offs, nr, n_tiles_abs, P.tile_first, tile_size);
        for (uint32_t pc = 0; pc < pieces; pc++) {
            const uint64_t lo_t = t_first + pc * per, hi_t = std::min<uint64_t>(n_tiles_abs, lo_t + per);
            if (lo_t < hi_t)
                launch_p1_reads(c, d_words, offs, nr, pc == 0 ? base0 : lo_t * tile_size, end_abs, hi_t, P.tile_first, pl.b1, P.seg_counts1, pl.cap1,
                                P.a_keys, P.a_hints, pl.sp, 0, nullptr);
            HIPCHK(c, hipEventRecord(c->ev_seq[2 * pc], c->stream));
            if (lo_t < hi_t)
                hipLaunchKernelGGL(k_p2_scatter, dim3((unsigned)pl.np1), dim3(PT_THREADS), 0, c->stream, P.a_keys, P.a_hints, pl.cap1, P.seg_counts1,
                                   (uint32_t)pl.np1, pl.b1, pl.b2, P.cursors2, pl.cap2, P.b_keys, P.b_hints, pl.sp, c->mm_k, pc, pieces);
            HIPCHK(c, hipEventRecord(c->ev_seq[2 * pc + 1], c->stream));
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventSynchronize(c->ev_seq[2 * pieces - 1]));
        for (uint32_t pc = 0; pc < pieces; pc++) {
            float f1 = 0, f2 = 0;
            HIPCHK(c, hipEventElapsedTime(&f1, pc ? c->ev_seq[2 * pc - 1] : c->ev0, c->ev_seq[2 * pc]));
            HIPCHK(c, hipEventElapsedTime(&f2, c->ev_seq[2 * pc], c->ev_seq[2 * pc + 1]));
            pl.ms1 += f1;
            pl.ms2 += f2;
        }
        pl.p2_done = true;
    } else {
        HIPCHK(c, hipEventRecord(c->ev_t[0], c->stream));  // (no wait here: pipe_finish enqueues P2 and P3 right behind)
        launch_tile_first(c, offs, nr, n_tiles_abs, P.tile_first, tile_size);
        if (pl.sk && pl.compact) {
            pl.pos0 = base0 / sk_tile * sk_tile;
            if (c->sw.ingest_debug)
                fprintf(stderr, "[count] compact records: %u buckets x %u leaves%s, %u tiles a segment from base %llu\n", pl.b1, pl.vleaf ? 1024u : pl.b2,
                        pl.vleaf ? " (whatever the table: it is sized behind the first level)" : "", pl.chunk_tiles, (unsigned long long)pl.pos0);
            hipLaunchKernelGGL((k_sk1w_extract<false, true>), dim3(P1W_SEGMENTS), dim3(P1W_THREADS), 0, c->stream, d_words, offs, nr, base0, end_abs,
                               n_tiles_abs, P.tile_first, c->cfg.k, pl.b1, P.seg_counts1, pl.cap1, P.a_recs, nullptr, pl.sks, c->cur_ptr_base,
                               pl.chunk_tiles, pl.vleaf ? 1024u : pl.b2);
        }
        else if (pl.sk)
            hipLaunchKernelGGL(k_sk1w_extract<false>, dim3(P1W_SEGMENTS), dim3(P1W_THREADS), 0, c->stream, d_words, offs, nr, base0, end_abs,
                               n_tiles_abs, P.tile_first, c->cfg.k, pl.b1, P.seg_counts1, pl.cap1, P.a_recs, P.a_hints, pl.sks, c->cur_ptr_base);
        else
            launch_p1_reads(c, d_words, offs, nr, base0, end_abs, n_tiles_abs, P.tile_first, pl.b1, P.seg_counts1, pl.cap1, P.a_keys,
                            P.a_hints, pl.sp, 0, nullptr);
        HIPCHK(c, hipGetLastError());
        rc = pipe_resize_by_sample(c, pl, n_records);  // (no long records here: no RUN_NOT_LONG)
        if (rc == RUN_BEYOND_LEAF_BITS && !c->no_vleaf) {  // (the batch wants a table beyond the reach of the records' leaf bits: once more, the two-array way)
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (c->sw.ingest_debug) fprintf(stderr, "[count] the batch wants a table beyond the reach of its records' ten leaf bits: the first level again, two arrays\n");
            c->no_vleaf = true;
            rc = add_reads_partitioned(c, d_words, d_off, r0, r1, base0, end_abs, wb);
            c->no_vleaf = false;
            return rc;
        }
        if (rc > 0) return fail(c, MC_EINVAL, "internal: the sample of the first bucket ended in '%s' where nothing asked for it", RUN_OUTCOME_NAMES[rc]);
        if (rc) return rc;
        pl.p1_pending = true;
    }
    rc = pipe_finish(c, pl);
    if (rc != RUN_LOST_RECORDS) return rc;  // (MC_OK, an error or RUN_BATCH_AGAIN)
    // (super-k-mer streams overflowed: unusually short runs) count this batch with the direct kernel instead
    return count_batch_direct(c, d_words, d_off, r0, r1, base0, end_abs, wb);
}

// A flat stream of keys (+ optional hints) through the partitioned pipeline: the keys a rank owns
// after the multi-GPU exchange.
static int add_keys_partitioned(mc_ctx *c, const uint64_t *d_keys, const uint32_t *d_hints, uint64_t n)
{
    mc_ctx::Pipe &P = c->pipe;
    PipePlan pl;
    int rc = by_key_ready(c);
    if (!rc) rc = pipe_prepare(c, n, &pl, PipeRequest());
    if (rc) return rc;
    rc = timed(c, &pl.ms1, [&] {
        hipLaunchKernelGGL(k_p1_keys_scatter, dim3(PT_SEGMENTS), dim3(PT_THREADS), 0, c->stream,
                           d_keys, d_hints, n, pl.b1, P.seg_counts1, pl.cap1, P.a_keys, P.a_hints, c->d_ctr + 1, pl.sp, c->mm_k);
    });
    if (rc) return rc;
    rc = pipe_finish(c, pl);
    if (rc != RUN_LOST_RECORDS) return rc;  // (MC_OK or an error: pl.may_rerun is not set)
    // (the streams overflowed: a few keys make up most of the batch) the direct kernel instead
    c->solid_tracked = false;
    c->solid_list_fresh = false;
    for (uint64_t i = 0; i < n;) {
        uint64_t allowed;
        rc = table_reserve(c, n - i, &allowed);
        if (rc) return rc;
        const uint64_t m = std::min<uint64_t>(allowed, n - i);
        if (d_hints)
            hipLaunchKernelGGL(k_add_keys_hint, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, d_keys + i, d_hints + i, m, c->view());
        else
            hipLaunchKernelGGL(k_add_keys, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, reinterpret_cast<const int64_t *>(d_keys) + i, m, c->view());
        HIPCHK(c, hipGetLastError());
        i += m;
    }
    return MC_OK;
}

// a stream of records through the direct kernel (what the partitioned runs fall back on when their streams overflow)
static int add_records_direct(mc_ctx *c, const uint4 *d_recs, const uint32_t *d_bins, uint64_t n)
{
    c->solid_tracked = false;
    c->solid_list_fresh = false;
    for (uint64_t i = 0; i < n;) {
        uint64_t allowed;
        int rc = table_reserve(c, (n - i) * SK_MAX_WINDOWS, &allowed);
        if (rc) return rc;
        const uint64_t m = std::min<uint64_t>(std::max<uint64_t>(allowed / SK_MAX_WINDOWS, 1), n - i);
        hipLaunchKernelGGL(k_sk_add_records, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, d_recs + i, d_bins + i, m, c->cfg.k, c->view(), 0u, c->d_ctr + 6);
        HIPCHK(c, hipGetLastError());
        i += m;
    }
    return MC_OK;
}

// A flat stream of super-k-mer records (+ bin words): what a rank owns after the multi-GPU exchange.
static int add_records_partitioned(mc_ctx *c, const uint4 *d_recs, const uint32_t *d_bins, uint64_t n)
{
    mc_ctx::Pipe &P = c->pipe;
    unsigned long long *sum = c->d_ctr + 2;
    HIPCHK(c, hipMemsetAsync(sum, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_sk_count_windows, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, d_recs, n, sum);
    HIPCHK(c, hipGetLastError());
    unsigned long long wb = 0;
    HIPCHK(c, hipMemcpy(&wb, sum, sizeof wb, hipMemcpyDeviceToHost));
    PipePlan pl;
    PipeRequest rq;
    rq.n_records = n;
    int rc = pipe_prepare(c, wb, &pl, rq);
    if (rc) return rc;
    rc = timed(c, &pl.ms1, [&] {
        hipLaunchKernelGGL(k_sk1_records, dim3(PT_SEGMENTS), dim3(PT_THREADS), 0, c->stream, d_recs, d_bins, n, pl.b1, P.seg_counts1,
                           pl.cap1, P.a_recs, P.a_hints, pl.sks);
    });
    if (rc) return rc;
    rc = pipe_finish(c, pl);
    if (rc != RUN_LOST_RECORDS) return rc;  // (MC_OK or an error: pl.may_rerun is not set)
    return add_records_direct(c, d_recs, d_bins, n);  // (the buckets overflowed)
}

// Records that arrive in level-1 bucket order already (the binned exchange, include/mcgpu.h mc_add_superkmers_binned_dev): part p of
// the buffer -- records part_off[p] .. part_off[p + 1] -- holds part_counts[p * fine + f] records of fine bucket f = mulhi32(bin word,
// fine), f ascending.  Where this table's level-1 buckets are unions of fine buckets the run starts at the second level, every part
// r = fine / np1 segments of every bucket.  Outcomes: RUN_NOT_BINNED where they are not (or the table has no second level, or the
// parts are too many): the caller counts the records as a flat stream.
static int add_records_binned(mc_ctx *c, const uint4 *d_recs, const uint32_t *d_ptrs, uint64_t n, uint64_t n_windows, uint32_t fine, uint32_t n_parts,
                              const uint64_t *part_off, const uint32_t *d_part_counts)
{
    mc_ctx::Pipe &P = c->pipe;
    {   // (the table may grow for the batch -- a context without a hint --: before the plan is looked at, as pipe_prepare would)
        bool hint_holds;
        int rc = pipe_reserve(c, n_windows, &hint_holds);
        if (rc) return rc;
    }
    uint64_t n_leaves, np1;
    uint32_t g;
    if (plan_levels(c, true, &n_leaves, &g, &np1)) return RUN_NOT_BINNED;
    if (n_leaves / np1 <= 1 || fine % np1 || n >= (1ull << 31)) return RUN_NOT_BINNED;
    const uint64_t r = fine / np1, nseg = (uint64_t)n_parts * r;
    if (nseg > (uint64_t)P1W_SEGMENTS || nseg == 0) return RUN_NOT_BINNED;
    int rc = ensure_buf(c, &P.seg_counts1, &P.segs1_cap, np1 * nseg);
    if (!rc) rc = ensure_buf(c, &P.skb_seg_start, &P.skb_seg_start_cap, np1 * nseg);
    if (!rc) rc = ensure_buf(c, &P.skb_small, &P.skb_small_cap, (uint64_t)P1W_SEGMENTS + 2 * PT_MAX_BUCKETS + 8);
    if (rc) return rc;
    // (the parts' starts go up through the context's pinned words; the kernel checks every part's counts against its length)
    std::vector<unsigned long long> po(part_off, part_off + n_parts + 1);
    po.push_back(0);  // [n_parts + 1]: the "counts do not add up" flag
    HIPCHK(c, hipMemcpyAsync(P.skb_small, po.data(), po.size() * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_skb_segments, dim3(n_parts), dim3(1024), 0, c->stream, P.skb_small, d_part_counts, fine, (uint32_t)r, (uint32_t)nseg, P.seg_counts1,
                       P.skb_seg_start, P.skb_small + n_parts + 1);
    HIPCHK(c, hipGetLastError());
    unsigned long long bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, P.skb_small + n_parts + 1, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (po must outlive its copy, and nothing may read by counts that do not add up)
    if (bad) return fail(c, MC_EINVAL, "mc_add_superkmers_binned_dev: the fine-bucket counts of %llu part(s) do not add up to the parts' lengths", bad);
    if (!c->want_list && (P.a_recs || P.a_hints)) {
        // This run has no first level: the extraction's first-level streams (a fifth of the table at configs[3]'s size) go back to the
        // pool, where the second level's buffer -- about as large -- is taken from; the next extraction gets them back from there.
        HIPCHK(c, hipStreamSynchronize(c->stream));
        g_scratch_pool.put(c->cfg.device, P.a_recs, P.a_recs_cap * sizeof(uint4));
        g_scratch_pool.put(c->cfg.device, P.a_hints, P.a_hints_cap * 4);
        P.a_recs = nullptr; P.a_recs_cap = 0; P.a_hints = nullptr; P.a_hints_cap = 0;
        c->solid_list_fresh = false;
    }
    PipePlan pl;
    PipeRequest rq;
    rq.n_records = n;
    rq.nseg1 = (uint32_t)nseg;
    rq.listed = true;
    rc = pipe_prepare(c, n_windows, &pl, rq);
    if (rc) return rc;
    if (pl.np1 != np1 || pl.b2 <= 1) return fail(c, MC_EINVAL, "internal: the plan of a binned run changed under it");
    pl.in_recs = d_recs;
    pl.in_ptrs = d_ptrs;
    rc = pipe_finish(c, pl);
    if (rc != RUN_LOST_RECORDS) return rc;  // (MC_OK or an error: pl.may_rerun is not set)
    return add_records_direct(c, d_recs, d_ptrs, n);  // (the leaves' streams overflowed)
}

// Appends the packed bases [first_off, last_off) of a batch (word-aligned copy from the batch's own buffer) to the read
// store and sets cur_ptr_base so that store position = cur_ptr_base + position in the batch.  in_place >= 0: the batch
// already sits in the store from word `in_place` on (mc_add_reads_packed uploads straight into it).
int rs_reserve(mc_ctx *c, uint64_t more_words)
{
    const uint64_t used = c->rs_words ? c->rs_end() / 32 : 0, need = std::max(c->rs_bases / 32 + more_words, used) + 2;  // (used: what must survive a move)
    if (need <= c->rs_cap_words) return MC_OK;
    uint64_t cap = std::max<uint64_t>(c->rs_cap_words * 2, std::max<uint64_t>(need, 1ull << 20));
    // (from the process-wide pool of large blocks, like the pipeline's scratch: a context's read store handed back with
    // hipFree is reclaimed lazily, and a later context's first launch waits for it)
    uint64_t *nw = nullptr;
    size_t got = 0;
    hipError_t e = g_scratch_pool.get(c->cfg.device, cap * 8, reinterpret_cast<void **>(&nw), &got);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        g_table_pool.release(c->cfg.device);
        g_scratch_pool.release(c->cfg.device);
        e = g_scratch_pool.get(c->cfg.device, cap * 8, reinterpret_cast<void **>(&nw), &got);
    }
    HIPCHK(c, e);
    cap = std::max<uint64_t>(cap, got / 8);
    if (used) HIPCHK(c, hipMemcpyAsync(nw, c->rs_words, used * 8, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    g_scratch_pool.put(c->cfg.device, c->rs_words, c->rs_cap_words * 8);
    c->rs_words = nw;
    c->rs_cap_words = cap;
    return MC_OK;
}
static int rs_append(mc_ctx *c, const uint64_t *d_words, uint64_t first_off, uint64_t last_off, int64_t in_place = -1, bool side = false)
{
    c->cur_ptr_base = ~0ull;
    if ((!c->rs_enabled && !c->rs_virtual) || last_off <= first_off) return MC_OK;
    const uint64_t w0 = first_off / 32, w1 = (last_off + 31) / 32;  // words [w0, w1) hold the batch (+ a pad word behind)
    uint64_t at = c->rs_bases / 32;
    if (c->rs_virtual) {
        // (the words themselves travel to the context that keeps the store: mc_read_store_import_dev there, at rs_bases as it is now)
    } else if (in_place >= 0) {
        at = (uint64_t)in_place;
    } else {
        int rc = rs_reserve(c, w1 - w0 + 1);
        if (rc) return rc;
        if (side) {
            // on the side stream: the counting kernels read the caller's buffer, the walk reads the store -- the copy runs
            // beside the kernels (0.25 ms for 10 M reads) and add_reads_dev_locked waits for it before it returns
            HIPCHK(c, hipEventRecord(c->ev_piece[7], c->stream));  // (what sits in the stream before may still write the store: rs_reserve's copy)
            HIPCHK(c, hipStreamWaitEvent(c->pipe_stream, c->ev_piece[7], 0));
            HIPCHK(c, hipMemcpyAsync(c->rs_words + at, d_words + w0, (w1 - w0 + 1) * 8, hipMemcpyDeviceToDevice, c->pipe_stream));
            c->rs_copy_pending = true;
        } else {
            HIPCHK(c, hipMemcpyAsync(c->rs_words + at, d_words + w0, (w1 - w0 + 1) * 8, hipMemcpyDeviceToDevice, c->stream));
        }
    }
    c->cur_ptr_base = at * 32 - w0 * 32;  // (mod 2^64: the kernels add a batch position >= w0 * 32)
    c->rs_bases = (at + (w1 - w0)) * 32;
    return MC_OK;
}

// Bases one run of the partitioned pipeline takes.  Positions are 64-bit throughout; what is 32-bit is the index of a
// record inside the scatter levels' arrays (pipe_prepare checks it): super-k-mer records are ~0.18 per window, so 2^34
// bases (114 M reads of 150 bp) stay far below 2^32 records, while one 8-byte key per window (k > 31, hash keys) costs
// scratch by the window -- those runs take what half the free memory holds, 2^31 to 2^33 bases.
// Every run reads and rewrites the whole table, so fewer, larger runs are what a large read set wants.
static uint64_t max_run_bases(const mc_ctx *c, double windows_per_base)
{   // windows_per_base: of the read set at hand (88 / 150 for 150-base reads at k = 63): the scratch is per window
    if (c->sw.max_run_bases) return std::max<uint64_t>(c->sw.max_run_bases, 1u << 20);
    if (c->mm_k) return 1ull << 34;
    // (tests: the per-window form's limit alone, so that a run cut for long records is too large for it)
    if (c->sw.max_run_bases_per_window) return c->sw.max_run_bases_per_window;
    // a key and a read pointer per window, in pieces (add_reads_partitioned): ~16.5 bytes of scratch per window.  Two
    // thirds of what the device has free may go there (the table is allocated already), between 2^31 and 2^33 bases: every
    // run reads and rewrites the whole table, so few, large runs (configs[2]: 2 instead of 4).
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = 0;
    fr += (c->pipe.a_cap + c->pipe.b_cap) * 12;  // (the scratch of the run before is ours to reuse)
    const double per_base = 16.5 * std::min(1.0, std::max(0.05, windows_per_base));
    return std::min<uint64_t>(1ull << 33, std::max<uint64_t>((1ull << 31) - (1ull << 24), (uint64_t)((double)fr * 0.66 / per_base)));
}

// counting with read offsets known on the host
static int add_reads_impl(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_off, const uint64_t *h_off,
                          uint64_t n_reads)
{
    const uint64_t k = (uint64_t)c->cfg.k;
    auto windows_of = [&](uint64_t a, uint64_t b) {
        uint64_t w = 0;
        for (uint64_t i = a; i < b; i++) {
            const uint64_t len = h_off[i + 1] - h_off[i];
            if (len >= k) w += len - k + 1;
        }
        return w;
    };
    const uint64_t total = windows_of(0, n_reads);
    const bool partition = c->sw.count_path == 2 || (c->sw.count_path == 0 && total >= (1ull << 22));
    if (partition) {
        uint64_t max_bases = max_run_bases(c, 1.0);
        uint64_t r = 0;
        while (r < n_reads) {
            uint64_t r1 = (uint64_t)(std::upper_bound(h_off + r, h_off + n_reads + 1, h_off[r] + max_bases) - h_off) - 1;
            if (r1 <= r) return fail(c, MC_EINVAL, "a single read of more than %llu bases is not supported", (unsigned long long)max_bases);
            if (r1 > n_reads) r1 = n_reads;
            const uint64_t wb = windows_of(r, r1);
            if (wb) {
                int rc = add_reads_partitioned(c, d_words, d_off, r, r1, h_off[r], h_off[r1], wb);
                if (rc == RUN_RESPLIT) { max_bases = max_run_bases(c, 1.0); continue; }  // (nothing of [r, r1) was counted)
                if (rc) return rc;
            }
            r = r1;
        }
        counts_changed(c);
        return MC_OK;
    }
    uint64_t r = 0;
    while (r < n_reads) {
        uint64_t allowed;
        const uint64_t remaining_bases = h_off[n_reads] - h_off[r];
        int rc = table_reserve(c, remaining_bases, &allowed);
        if (rc) return rc;
        // largest r1 with windows(r..r1) <= allowed (windows <= bases)
        uint64_t r1 = r;
        const uint64_t target = h_off[r] + allowed;
        r1 = (uint64_t)(std::upper_bound(h_off + r, h_off + n_reads + 1, target) - h_off) - 1;
        if (r1 <= r) r1 = r + 1;  // a single read longer than the allowance: fine, still < 0.85 + one read
        if (r1 > n_reads) r1 = n_reads;
        const uint64_t win = windows_of(r, r1);
        double ms = 0;
        rc = timed(c, &ms, [&] { launch_count(c, d_words, d_off, r, r1); });
        if (rc) return rc;
        c->st.count_ms += ms;
        c->st.count_total_ms += ms;
        c->st.count_launches++;
        c->st.windows += win;
        r = r1;
    }
    counts_changed(c);
    return MC_OK;
}

// ------------------------------------------------------------------------------------------ C ABI

extern "C" {

int mc_abi_version(void) { return MC_ABI_VERSION; }

const char *mc_last_error(const mc_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int mc_create(const mc_config *cfg, mc_ctx **out)
{
    if (!cfg || !out) return fail(nullptr, MC_EINVAL, "mc_create: null argument");
    *out = nullptr;
    if (cfg->key_mode < MC_KEY_PACKED || cfg->key_mode > MC_KEY_FNV1A)
        return fail(nullptr, MC_EINVAL, "mc_create: unknown key_mode %d", cfg->key_mode);
    const int kmax = cfg->key_mode == MC_KEY_PACKED ? 31 : 63;
    if (cfg->k < 1 || cfg->k > kmax)
        return fail(nullptr, MC_EINVAL, "mc_create: k=%d out of range 1..%d for key_mode %d", cfg->k, kmax,
                    cfg->key_mode);
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0)
        return fail(nullptr, MC_EHIP, "mc_create: no HIP device available (%s)",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= n_dev)
        return fail(nullptr, MC_EINVAL, "mc_create: device %d out of range (have %d)", cfg->device, n_dev);
    mc_ctx *c = new (std::nothrow) mc_ctx;
    if (!c) return fail(nullptr, MC_ENOMEM, "mc_create: out of host memory");
    c->cfg = *cfg;
#define CREATE_CHK(call)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            fail(nullptr, MC_EHIP, "mc_create: %s: %s", #call, hipGetErrorString(e_));            \
            mc_destroy(c);                                                                        \
            return e_ == hipErrorOutOfMemory ? MC_ENOMEM : MC_EHIP;                               \
        }                                                                                         \
    } while (0)
    CREATE_CHK(hipSetDevice(cfg->device));
    CREATE_CHK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    CREATE_CHK(hipEventCreate(&c->ev0));
    CREATE_CHK(hipEventCreate(&c->ev1));
    CREATE_CHK(hipStreamCreateWithFlags(&c->pipe_stream, hipStreamNonBlocking));
    for (auto &e : c->ev_piece) CREATE_CHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto &e : c->ev_t) CREATE_CHK(hipEventCreate(&e));
    CREATE_CHK(hipMalloc(reinterpret_cast<void **>(&c->d_ctr), 16 * sizeof(unsigned long long)));
    CREATE_CHK(hipHostMalloc(reinterpret_cast<void **>(&c->h_scratch), 32 * sizeof(unsigned long long), hipHostMallocDefault));
    c->d_fatal = reinterpret_cast<uint32_t *>(c->d_ctr + 8);  // (one copy brings the counters and the flag)
    CREATE_CHK(hipMalloc(reinterpret_cast<void **>(&c->d_ovf), mc_ctx::OVF_CAP * sizeof(uint4)));
    CREATE_CHK(hipMalloc(reinterpret_cast<void **>(&c->d_ovf_leaf), mc_ctx::OVF_CAP * sizeof(uint32_t)));
    CREATE_CHK(hipMemsetAsync(c->d_ctr, 0, 16 * sizeof(unsigned long long), c->stream));

#undef CREATE_CHK
    c->sw = read_switches();
    c->want_list = (cfg->flags & MC_FLAG_SOLID_LIST) != 0 || !c->sw.bfs_direct;
    // packed keys of at least SK_MIN_K bases: table regions = minimizer bins, reads counted as super-k-mers
    // (MC_SUPERKMERS=0 keeps the per-window pipeline: for A/B measurements)
    if (cfg->key_mode == MC_KEY_PACKED && cfg->k >= SK_MIN_K) c->mm_k = cfg->k;
    if (!c->sw.superkmers) c->mm_k = 0;
    c->sk_form = c->mm_k != 0;
    // polynomial keys of 33 .. 63 bases in a table sized by a capacity hint: minimizer bins too, reads counted as long records
    // (count_long.h; hash_bins() above says what such a table cannot do and what happens then).  MC_LONG_RECORDS=0: the per-window pipeline.
    if (cfg->key_mode == MC_KEY_POLY && cfg->k >= SKL_MIN_K && cfg->k <= SKL_MAX_K) {
        if (c->sw.long_records) c->mm_k = cfg->k;
    }
    uint64_t want_slots = 1ull << 22;  // 4 M slots = 64 MB to start with
    if (cfg->capacity_hint) {
        // Load factor the hint is turned into.  Hash-prefix tables: 0.7 (regions are probed in LDS, a fuller table
        // costs little).  Minimizer-bin tables fill less evenly (the k-mers of one locus share a bin) and both the merge
        // kernel's probe loops and the walk's lookups pay for every extra probe, while a sparser table only costs its
        // write-back: measured on the 10 M-read workload (364 M keys), count + BFS per step at load 0.60 / 0.51 / 0.43 /
        // 0.36: 39.1 / 31.5 / 29.2 / 28.6 ms.  So 0.25 up to 64 M keys, + 0.05 per doubling, 0.36 at most -- but never
        // more than 2^20 regions while the load stays under 0.6: beyond that a leaf of the counting pipeline covers two
        // regions and the merge kernel sweeps each leaf twice.
        double load = 0.7;
        if (c->mm_k) load = std::min(0.36, std::max(0.25, 0.25 + 0.05 * std::log2((double)cfg->capacity_hint / (double)(64u << 20))));
        want_slots = std::max<uint64_t>(want_slots, (uint64_t)((double)cfg->capacity_hint / load));
        if (c->mm_k) want_slots = std::max<uint64_t>(1ull << 22, mm_slots_for(c, (double)cfg->capacity_hint, load));
        // Long records need their bins roomy: at k = 63 a region holds the k-mers of four or five loci (each with the error variants
        // of the ~30 reads that cover it), and 2^21 regions -- one a leaf, all the merge kernel takes -- at load 0.53 (configs[2] at
        // full size: 4.6 G keys, 137 GB) leave a few per cent of them overfull, more than the hand-on list holds; such a table cannot
        // be rebuilt either.  A table that cannot be roomy takes its bin words from the TWO smallest hashes of a window (count_long.h
        // skl_word2: mm_k < 0 -- half again as many, smaller loci a region: even enough up to load ~0.55, scripts/bin_model.py);
        // beyond that, and with MC_LONG_BINS=1 (tuning runs; 2: two smallest for every table), the per-window pipeline.
        const bool crowded = hash_bins(c) && (double)cfg->capacity_hint > 0.40 * (double)want_slots;
        const bool two = hash_bins(c) && (c->sw.long_bins ? c->sw.long_bins == 2 : crowded);
        if (two && (double)cfg->capacity_hint <= 0.56 * (double)want_slots) c->mm_k = -cfg->k;
        else if (crowded) {
            c->mm_k = 0;
            want_slots = std::max<uint64_t>(1ull << 22, (uint64_t)((double)cfg->capacity_hint / 0.7));
        }
    }
    int rc = table_alloc(c, regions_for(c, want_slots));
    if (rc) {
        g_create_err = c->err;
        mc_destroy(c);
        return rc;
    }
    *out = c;
    return MC_OK;
}

void mc_destroy(mc_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    // Blocks go back to process-wide pools below and may be handed to another context at once (hipFree used to wait for the
    // device; a pool does not): everything this context still has queued must be done first -- on the caller's stream too
    // (mc_set_stream) and on the side stream of the pipeline.
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->own_stream && c->own_stream != c->stream) (void)hipStreamSynchronize(c->own_stream);
    if (c->pipe_stream) (void)hipStreamSynchronize(c->pipe_stream);
    for (auto &m : c->ipc_opened) (void)hipIpcCloseMemHandle(m.p);
    if (c->d_shards) (void)hipFree(c->d_shards);
    if (c->slots) table_release(c, c->slots, c->slots_bytes);
    if (c->solid) (void)hipFree(c->solid);
    c->pipe.release(c->cfg.device);
    {
        mc_ctx::Dup &D = c->dup;
        g_scratch_pool.put(c->cfg.device, D.l1_keys, D.l1_words * 8);
        g_scratch_pool.put(c->cfg.device, D.l1_counts, D.l1_counts_cap * 4);
        g_scratch_pool.put(c->cfg.device, D.l2_own, D.l2_own_words * 8);
        g_scratch_pool.put(c->cfg.device, D.l2_counts, D.l2_counts_cap * 4);
        if (D.flags) (void)hipFree(D.flags);
        if (D.ctr) (void)hipFree(D.ctr);
        if (D.list) (void)hipFree(D.list);
        if (D.set.qk) (void)hipFree(D.set.qk);
        if (D.tw) (void)hipFree(D.tw);
        if (D.pq_mem) (void)hipFree(D.pq_mem);
        if (D.pq_groups) (void)hipFree(D.pq_groups);
    }
    c->bfs_pool.clear();
    if (c->d_ctr) (void)hipFree(c->d_ctr);
    if (c->h_scratch) (void)hipHostFree(c->h_scratch);
    if (c->d_ovf) (void)hipFree(c->d_ovf);
    if (c->d_ovf_leaf) (void)hipFree(c->d_ovf_leaf);
    g_scratch_pool.put(c->cfg.device, c->d_ovf_tmp, c->ovf_tmp_cap * sizeof(uint4));
    if (c->d_ovf_leaf_tmp) (void)hipFree(c->d_ovf_leaf_tmp);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    g_scratch_pool.put(c->cfg.device, c->rs_words, c->rs_cap_words * 8);
    for (auto &e : c->ev_piece) if (e) (void)hipEventDestroy(e);
    for (auto &e : c->ev_seq) if (e) (void)hipEventDestroy(e);
    for (auto &e : c->ev_t) if (e) (void)hipEventDestroy(e);
    if (c->pipe_stream) { (void)hipStreamSynchronize(c->pipe_stream); (void)hipStreamDestroy(c->pipe_stream); }
    c->tok_pool.release();
    if (c->h_bfs_stage) (void)hipHostFree(c->h_bfs_stage);
    if (c->d_bfs_stage) (void)hipFree(c->d_bfs_stage);
    if (c->d_bfs_pack) (void)hipFree(c->d_bfs_pack);
    if (c->h_bfs_hdr) (void)hipHostFree(c->h_bfs_hdr);
    for (char *p : c->pin) if (p) (void)hipHostFree(p);
    for (hipStream_t st : c->pin_stream) if (st) (void)hipStreamDestroy(st);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int mc_clear(mc_ctx *c)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    c->virgin = true;
    if (c->d_shards) {  // (the tables an attachment describes are about to change; their mappings stay for the next attachment)
        for (auto &m : c->ipc_opened) m.in_use = false;
        (void)hipFree(c->d_shards);
        c->d_shards = nullptr; c->h_shards.clear(); c->shard_owner_mm_k = 0;
    }
    c->rs_bases = 0;  // (slots that pointed into the read store go with the table)
    c->rs_hi_bases = 0;
    HIPCHK(c, hipMemsetAsync(c->d_ctr, 0, 9 * sizeof(unsigned long long), c->stream));  // (counters and the fatal flag: one fill)
    c->n_used_host = 0;
    c->finalized = false;
    c->shards_dropped = false;
    c->solid_cov = -1; c->solid_external = false;
    c->solid_tracked = true;
    c->solid_list_fresh = false;
    dup_forget(c);
    return MC_OK;
}

int mc_set_coverage_hint(mc_ctx *c, int min_cov)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (min_cov < 0 || min_cov > 32767) return fail(c, MC_EINVAL, "mc_set_coverage_hint: min_cov must be in 0..32767");
    if (min_cov != c->cov_hint && !c->virgin) c->solid_tracked = false;  // keys already counted were not tracked at this threshold
    if (min_cov != c->cov_hint) c->solid_list_fresh = false;
    c->cov_hint = min_cov;
    return MC_OK;
}

int mc_set_read_pointers(mc_ctx *c, int mode)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    const int m = mode & 0xF;
    if (m > 2 || (mode & ~(0xF | MC_PTRS_ON_EVERY_RECORD))) return fail(c, MC_EINVAL, "mc_set_read_pointers: mode %d", mode);
    c->rs_enabled = m == 1;
    c->rs_virtual = m == 2;
    c->all_ptrs = (mode & MC_PTRS_ON_EVERY_RECORD) != 0;
    return MC_OK;
}

int mc_read_store_seek(mc_ctx *c, uint64_t at_bases, uint64_t reserve_bases)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (at_bases % 32) return fail(c, MC_EINVAL, "mc_read_store_seek: positions are whole words (multiples of 32 bases)");
    if (!c->rs_enabled && !c->rs_virtual) return fail(c, MC_ESTATE, "mc_read_store_seek: this context keeps no read pointers");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (c->rs_enabled) {
        c->rs_hi_bases = c->rs_end();  // (what lies below stays readable)
        c->rs_bases = at_bases;
        const uint64_t want = std::max(reserve_bases, at_bases) / 32 + 2;
        if (want > c->rs_cap_words) {
            int rc = rs_reserve(c, want - at_bases / 32);
            if (rc) return rc;
        }
    } else {
        c->rs_bases = at_bases;
    }
    return MC_OK;
}

uint64_t mc_read_store_tell(mc_ctx *c)
{
    if (!c) return 0;
    std::lock_guard<std::mutex> g(c->mu);
    return c->rs_bases;
}

int mc_read_store_import_dev(mc_ctx *c, const uint64_t *d_words, uint64_t n_words, uint64_t at_bases)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->rs_enabled) return fail(c, MC_ESTATE, "mc_read_store_import_dev: this context keeps no read store");
    if (at_bases % 32 || (!d_words && n_words)) return fail(c, MC_EINVAL, "mc_read_store_import_dev: bad argument");
    if (n_words == 0) return MC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const uint64_t at = at_bases / 32;
    if (at + n_words + 1 > c->rs_cap_words) {  // (mc_read_store_seek's reserve_bases is what makes this rare: a move copies the store)
        const uint64_t fill = c->rs_bases / 32;
        int rc = rs_reserve(c, at + n_words + 1 > fill ? at + n_words + 1 - fill : 0);
        if (rc) return rc;
    }
    HIPCHK(c, hipMemcpyAsync(c->rs_words + at, d_words, n_words * 8, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the caller's buffer may go as soon as this returns)
    c->rs_hi_bases = std::max(c->rs_hi_bases, (at + n_words) * 32);
    return MC_OK;
}

int mc_share_read_store(mc_ctx *c, mc_ctx *from)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (from == c) from = nullptr;
    if (from && from->cfg.device != c->cfg.device) return fail(c, MC_EINVAL, "mc_share_read_store: the contexts are on different devices");
    c->rs_from = from;
    return MC_OK;
}

int mc_set_stream(mc_ctx *c, void *hip_stream)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->own_stream;
    return MC_OK;
}

}  // extern "C"

// Host (pageable) memory to the device.  A plain hipMemcpy of pageable memory stages through one thread; a few
// threads each staging 8 MB pieces through their own pinned buffers and stream reach the link rate
// (scripts/microbench/hostreg.hip: 360 MB in 7-14 ms instead of 19 ms, or 176 ms for memory touched first here).
// fd >= 0: the bytes come from that file at file_off instead (pread straight into the pinned buffers: no page faults on
// a mapping).  Touches no state of the context but the pinned buffers (under their own lock), so the file reader can
// run it beside the kernels of the chunk before; returns a hipError_t-free verdict for the caller to report.
bool h2d_pinned(mc_ctx *c, void *dst, const void *src, size_t bytes, int fd, uint64_t file_off)
{
    constexpr size_t CHUNK = 8u << 20;
    constexpr int T = 8;  // staging threads, two pinned buffers each (mc_ctx::pin, pin_stream)
    std::lock_guard<std::mutex> g(c->pin_mu);
    if (hipSetDevice(c->cfg.device) != hipSuccess) return false;
    if (!c->pin[0]) {
        for (int i = 0; i < 2 * T; i++)
            if (hipHostMalloc(reinterpret_cast<void **>(&c->pin[i]), CHUNK) != hipSuccess) return false;
        for (int i = 0; i < T; i++)
            if (hipStreamCreateWithFlags(&c->pin_stream[i], hipStreamNonBlocking) != hipSuccess) return false;
    }
    const size_t n_chunks = (bytes + CHUNK - 1) / CHUNK;
    bool failed[T] = {};
    const int device = c->cfg.device;
    std::vector<std::thread> th;
    for (int t = 0; t < T && (size_t)t < n_chunks; t++)
        th.emplace_back([&, t] {
            if (hipSetDevice(device) != hipSuccess) { failed[t] = true; return; }
            hipEvent_t ev[2];
            if (hipEventCreateWithFlags(&ev[0], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) != hipSuccess) { failed[t] = true; return; }
            bool used[2] = {false, false};
            int flip = 0;
            for (size_t ch = (size_t)t; ch < n_chunks; ch += T) {
                const size_t off = ch * CHUNK, len = std::min(CHUNK, bytes - off);
                if (used[flip] && hipEventSynchronize(ev[flip]) != hipSuccess) failed[t] = true;
                if (fd >= 0) {
                    for (size_t got = 0; got < len;) {
                        const ssize_t r = pread(fd, c->pin[2 * t + flip] + got, len - got, (off_t)(file_off + off + got));
                        if (r <= 0) { failed[t] = true; break; }
                        got += (size_t)r;
                    }
                } else {
                    memcpy(c->pin[2 * t + flip], static_cast<const char *>(src) + off, len);
                }
                if (hipMemcpyAsync(static_cast<char *>(dst) + off, c->pin[2 * t + flip], len, hipMemcpyHostToDevice, c->pin_stream[t]) != hipSuccess ||
                    hipEventRecord(ev[flip], c->pin_stream[t]) != hipSuccess)
                    failed[t] = true;
                used[flip] = true;
                flip ^= 1;
            }
            if (hipStreamSynchronize(c->pin_stream[t]) != hipSuccess) failed[t] = true;
            (void)hipEventDestroy(ev[0]);
            (void)hipEventDestroy(ev[1]);
        });
    for (auto &x : th) x.join();
    for (int t = 0; t < T; t++)
        if (failed[t]) return false;
    return true;
}

int h2d_fast(mc_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (bytes < (32u << 20)) {
        HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return MC_OK;
    }
    if (!h2d_pinned(c, dst, src, bytes, -1, 0)) return fail(c, MC_EHIP, "host-to-device copy failed");
    return MC_OK;
}

extern "C" {

int mc_add_reads_packed(mc_ctx *c, const uint64_t *words, const uint64_t *off, uint64_t n_reads)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if ((!words || !off) && n_reads) return fail(c, MC_EINVAL, "mc_add_reads_packed: null pointer");
    if (n_reads == 0) return MC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const uint64_t n_bases = off[n_reads];
    if (n_bases < off[0]) return fail(c, MC_EINVAL, "mc_add_reads_packed: read_offsets not monotone");
    const uint64_t n_words = (n_bases + 31) / 32 + 1;
    const uint64_t w_begin = off[0] / 32;  // offsets need not start at 0
    DevBuf<uint64_t> dw, doff;
    uint64_t *dst = nullptr;
    int64_t in_store = -1;
    int rc;
    if (c->rs_enabled) {  // straight into the read store: the kernels read the batch from there
        rc = rs_reserve(c, n_words - w_begin);
        if (rc) return rc;
        in_store = (int64_t)(c->rs_bases / 32);
        dst = c->rs_words + in_store;
    } else {
        HIPCHK(c, dw.alloc(n_words - w_begin));
        dst = dw.p;
    }
    HIPCHK(c, doff.alloc(n_reads + 1));
    rc = h2d_fast(c, dst, words + w_begin, (n_words - w_begin) * 8);
    if (rc) return rc;
    if (w_begin == 0) {
        rc = h2d_fast(c, doff.p, off, (n_reads + 1) * 8);
    } else {
        std::vector<uint64_t> rel(off, off + n_reads + 1);
        for (auto &x : rel) x -= w_begin * 32;
        rc = h2d_fast(c, doff.p, rel.data(), (n_reads + 1) * 8);
    }
    if (rc) return rc;
    // (monotone offsets are checked on the device, with the window count: k_reads_summary)
    rc = add_reads_dev_locked(c, dst, doff.p, n_reads, n_bases - w_begin * 32, in_store);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return rc;
}

}  // extern "C"

// reads resident in HBM (the context's lock is held)
static int add_reads_dev_counted(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_off, uint64_t n_reads, uint64_t n_bases, int64_t in_store);
int add_reads_dev_locked(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_off, uint64_t n_reads, uint64_t n_bases, int64_t in_store)
{
    const int rc = abi_result(c, add_reads_dev_counted(c, d_words, d_off, n_reads, n_bases, in_store));  // (every caller is an entry point of the C ABI)
    if (c->rs_copy_pending) {  // the caller's buffer is his again when this returns, and later work on the stream may read the store
        c->rs_copy_pending = false;
        HIPCHK(c, hipStreamSynchronize(c->pipe_stream));
    }
    return rc;
}
static int add_reads_dev_counted(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_off, uint64_t n_reads, uint64_t n_bases, int64_t in_store)
{
    // summary on the device: total windows, monotone offsets, first and last offset
    unsigned long long *sum = c->d_ctr + 4;
    unsigned long long *sum4 = c->d_ctr + 10;  // windows, violations, first offset, last offset: one copy
    HIPCHK(c, hipMemsetAsync(sum4, 0, 2 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_reads_summary, dim3(grid_for((n_reads + 1) / 2, 256, 512)), dim3(256), 0, c->stream, d_off, n_reads,
                       (uint64_t)c->cfg.k, sum4, 1);
    HIPCHK(c, hipGetLastError());
    unsigned long long *hs = c->h_scratch + 20;
    HIPCHK(c, hipMemcpyAsync(hs, sum4, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t first_off = hs[2], last_off = hs[3];
    if (hs[1]) return fail(c, MC_EINVAL, "mc_add_reads_packed_dev: read_offsets not monotone");
    if (last_off != n_bases)
        return fail(c, MC_EINVAL, "mc_add_reads_packed_dev: read_offsets[n_reads]=%llu but n_bases=%llu",
                    (unsigned long long)last_off, (unsigned long long)n_bases);
    const uint64_t total = hs[0];
    {   // the batch joins the read store (the slots of its k-mers will point there)
        int rc = rs_append(c, d_words, first_off, last_off, in_store, true);
        if (rc) return rc;
        c->ptr_tries = 1;
    }
    const bool partition = c->sw.count_path == 2 || (c->sw.count_path == 0 && total >= (1ull << 22));
    const double wpb = last_off > first_off ? (double)total / (double)(last_off - first_off) : 1.0;  // windows per base
    if (partition && last_off - first_off < max_run_bases(c, wpb)) {  // one batch: no need for the offsets on the host
        int rc = total ? add_reads_partitioned(c, d_words, d_off, 0, n_reads, first_off, last_off, total) : MC_OK;
        if (rc != RUN_RESPLIT) {  // (RUN_RESPLIT: the long form declined and the batch is too large for one record a window: in runs, below)
            if (rc) return rc;
            counts_changed(c);
            return MC_OK;
        }
    }
    if (partition) {
        // several runs: cut at read boundaries found by bisection on the device's offsets (a few 8-byte copies), each
        // run's windows summed on the device -- the offsets of 100 M reads never travel to the host
        auto off_at = [&](uint64_t i, uint64_t *v) -> int {
            HIPCHK(c, hipMemcpyAsync(v, d_off + i, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            return MC_OK;
        };
        uint64_t r = 0, off_r = first_off;
        while (r < n_reads) {
            const uint64_t max_bases = max_run_bases(c, wpb), target = off_r + max_bases;
            uint64_t r1 = n_reads, off_r1 = last_off;
            if (last_off > target) {
                uint64_t lo = r, hi = n_reads;  // offsets[lo] <= target < offsets[hi]
                while (hi - lo > 1) {
                    const uint64_t mid = lo + (hi - lo) / 2;
                    uint64_t v;
                    int rc = off_at(mid, &v);
                    if (rc) return rc;
                    if (v <= target) lo = mid; else hi = mid;
                }
                r1 = lo;
                int rc = off_at(r1, &off_r1);
                if (rc) return rc;
            }
            if (r1 <= r) return fail(c, MC_EINVAL, "a single read of more than %llu bases is not supported", (unsigned long long)max_bases);
            HIPCHK(c, hipMemsetAsync(sum, 0, 2 * sizeof(unsigned long long), c->stream));
            hipLaunchKernelGGL(k_reads_summary, dim3(grid_for(r1 - r, 256, 512)), dim3(256), 0, c->stream, d_off + r, r1 - r, (uint64_t)c->cfg.k, sum);
            HIPCHK(c, hipGetLastError());
            unsigned long long wb = 0;
            HIPCHK(c, hipMemcpyAsync(&wb, sum, sizeof wb, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (wb) {
                int rc = add_reads_partitioned(c, d_words, d_off, r, r1, off_r, off_r1, wb);
                if (rc == RUN_RESPLIT) continue;  // (nothing of [r, r1) was counted; the next cut is made for the table as it is now)
                if (rc) return rc;
            }
            r = r1;
            off_r = off_r1;
        }
        counts_changed(c);
        return MC_OK;
    }
    // the launch planner of the direct kernel needs the offsets on the host (8 bytes per read, once per call)
    std::vector<uint64_t> h_off(n_reads + 1);
    HIPCHK(c, hipMemcpyAsync(h_off.data(), d_off, (n_reads + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return add_reads_impl(c, d_words, d_off, h_off.data(), n_reads);
}

extern "C" {

int mc_add_reads_packed_dev(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_off, uint64_t n_reads,
                            uint64_t n_bases)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if ((!d_words || !d_off) && n_reads) return fail(c, MC_EINVAL, "mc_add_reads_packed_dev: null pointer");
    if (n_reads == 0) return MC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return add_reads_dev_locked(c, d_words, d_off, n_reads, n_bases);
}

int mc_add_keys_dev(mc_ctx *c, const int64_t *d_keys, const uint32_t *d_hints, uint64_t n)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!d_keys && n) return fail(c, MC_EINVAL, "mc_add_keys_dev: null pointer");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const bool partition = c->sw.count_path == 2 || (c->sw.count_path == 0 && n >= (1ull << 22));
    if (partition) {
        const uint64_t max_batch = (1ull << 31) - (1ull << 24);
        for (uint64_t i = 0; i < n; i += max_batch) {
            const uint64_t m = std::min<uint64_t>(max_batch, n - i);
            int rc = add_keys_partitioned(c, reinterpret_cast<const uint64_t *>(d_keys) + i, d_hints ? d_hints + i : nullptr, m);
            if (rc) return abi_result(c, rc);
        }
    } else {
        c->solid_tracked = false;
        c->solid_list_fresh = false;
        uint64_t i = 0;
        while (i < n) {
            uint64_t allowed;
            int rc = table_reserve(c, n - i, &allowed);
            if (rc) return rc;
            const uint64_t m = std::min<uint64_t>(allowed, n - i);
            double ms = 0;
            rc = timed(c, &ms, [&] {
                if (d_hints)
                    hipLaunchKernelGGL(k_add_keys_hint, dim3(grid_for(m, 256)), dim3(256), 0, c->stream,
                                       reinterpret_cast<const uint64_t *>(d_keys) + i, d_hints + i, m, c->view());
                else
                    hipLaunchKernelGGL(k_add_keys, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, d_keys + i, m, c->view());
            });
            if (rc) return rc;
            c->st.count_ms += ms;
            c->st.count_total_ms += ms;
            c->st.count_launches++;
            c->st.windows += m;
            i += m;
        }
    }
    counts_changed(c);
    return MC_OK;
}

int mc_add_pairs_dev(mc_ctx *c, const int64_t *d_keys, const int16_t *d_counts, const uint32_t *d_hints, uint64_t n)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if ((!d_keys || !d_counts) && n) return fail(c, MC_EINVAL, "mc_add_pairs_dev: null pointer");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    c->solid_tracked = false;
    c->solid_list_fresh = false;
    uint64_t i = 0;
    while (i < n) {
        uint64_t allowed;
        int rc = table_reserve(c, n - i, &allowed);
        if (rc) return rc;
        const uint64_t m = std::min<uint64_t>(allowed, n - i);
        hipLaunchKernelGGL(k_add_pairs, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, d_keys + i, d_counts + i,
                           d_hints ? d_hints + i : nullptr, m, c->view());
        HIPCHK(c, hipGetLastError());
        i += m;
    }
    counts_changed(c);
    return MC_OK;
}

int mc_finalize_counts(mc_ctx *c, uint64_t *n_distinct)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    unsigned long long *h = c->h_scratch;
    {
        int rc = materialize(c);
        if (rc) return rc;
        // (one wait for all the counters: the parked additions' among them -- a wait of its own before, for a number that is 0
        // in every run that fits its table)
        HIPCHK(c, hipMemcpyAsync(h, c->d_ctr, 9 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const bool parked = h[7] != 0;
        if (parked) rc = drain_parked(c);
        // hash keys in minimizer bins: a key that different k-mers brought to different regions gets the sum of its counters
        // wherever it is read, and counts once (dup_check.h; src/io/LargeKIOUtils.java:46-49 has one counter a hash)
        const bool joins = hash_bins(c) && !c->virgin && !c->dup.checked;
        if (!rc) rc = ensure_dups(c);
        if (rc) return rc;
        if (parked || joins) {  // (the counters may have moved)
            HIPCHK(c, hipMemcpyAsync(h, c->d_ctr, 9 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    }
    const uint32_t fatal = (uint32_t)h[8];
    if (fatal) return fail(c, MC_EOVERFLOW, "a k-mer table region filled up (hash skew)");
    c->n_used_host = h[0];
    c->finalized = true;
    const uint64_t shadows = c->dup.merged ? c->dup.n_tw - c->dup.n_keys : 0;  // (slots beyond a key's first)
    if (n_distinct) *n_distinct = h[0] - shadows + (h[1] ? 1 : 0);
    return MC_OK;
}

int mc_get_dev(mc_ctx *c, const int64_t *d_keys, uint64_t n, int16_t *d_out)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->finalized) return fail(c, MC_ESTATE, "mc_get: call mc_finalize_counts first");
    if ((!d_keys || !d_out) && n) return fail(c, MC_EINVAL, "mc_get_dev: null pointer");
    if (n == 0) return MC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (hash_bins(c) && !c->virgin) {  // (hash keys in minimizer bins: one sweep of the table answers all the queries, k_getq_*)
        if (n >= (1ull << 31)) return fail(c, MC_EINVAL, "mc_get: at most 2^31 - 1 keys a call on this table");
        uint64_t qn = 1024;
        while (qn < 2 * n) qn <<= 1;
        DevBuf<unsigned long long> qk;
        DevBuf<uint32_t> qi;
        HIPCHK(c, qk.alloc(qn));
        HIPCHK(c, qi.alloc(qn));
        HIPCHK(c, hipMemsetAsync(qk.p, 0xFF, qn * sizeof(unsigned long long), c->stream));
        HIPCHK(c, hipMemsetAsync(d_out, 0xFF, n * sizeof(int16_t), c->stream));  // (-1: absent)
        hipLaunchKernelGGL(k_getq_build, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, d_keys, n, qk.p, qi.p, qn - 1);
        hipLaunchKernelGGL(k_getq_sweep, dim3(grid_for(c->n_slots(), 256, 256 * 16)), dim3(256), 0, c->stream, c->slots, c->n_slots(), qk.p, qi.p, qn - 1, d_out);
        hipLaunchKernelGGL(k_getq_finish, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, d_keys, n, qk.p, qi.p, qn - 1, d_out, c->d_ctr + 1);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return MC_OK;
    }
    if (int brc = by_key_ready(c)) return brc;
    hipLaunchKernelGGL(k_get, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, d_keys, n, d_out, c->view());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MC_OK;
}

int mc_get(mc_ctx *c, const int64_t *keys, uint64_t n, int16_t *out)
{
    if (!c) return MC_EINVAL;
    if ((!keys || !out) && n) return fail(c, MC_EINVAL, "mc_get: null pointer");
    if (n == 0) return MC_OK;
    DevBuf<int64_t> dk;
    DevBuf<int16_t> dout;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->finalized) return fail(c, MC_ESTATE, "mc_get: call mc_finalize_counts first");
        HIPCHK(c, hipSetDevice(c->cfg.device));
        HIPCHK(c, alloc_result(c, dk, n));
        HIPCHK(c, alloc_result(c, dout, n));
        HIPCHK(c, hipMemcpyAsync(dk.p, keys, n * 8, hipMemcpyHostToDevice, c->stream));
    }
    int rc = mc_get_dev(c, dk.p, n, dout.p);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipMemcpy(out, dout.p, n * 2, hipMemcpyDeviceToHost));
    return MC_OK;
}

int mc_kmer_keys(mc_ctx *c, const uint64_t *hi, const uint64_t *lo, uint64_t n, int64_t *out_keys)
{
    if (!c) return MC_EINVAL;
    if ((!lo || !out_keys) && n) return fail(c, MC_EINVAL, "mc_kmer_keys: null pointer");
    for (uint64_t i = 0; i < n; i++) {
        const Kmer v{hi ? hi[i] : 0, lo[i]};
        out_keys[i] = key_of_mode(v, c->cfg.k, c->cfg.key_mode);
    }
    return MC_OK;
}

uint32_t mc_key_owner(int64_t key, uint32_t n_owners)
{
    return n_owners ? (uint32_t)((fmix64((uint64_t)key) & 0xFFFFFFFFull) % n_owners) : 0;
}

int mc_extract_keys_dev(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_off, uint64_t n_reads, uint64_t n_bases,
                        uint32_t n_owners, int64_t *d_keys, uint32_t *d_hints, uint64_t cap, uint64_t *owner_offsets)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    struct ResetRule { mc_ctx *c; ~ResetRule() { c->extract_by_minimizer = false; } } reset_rule{c};  // (the group's choice holds for this call only)
    if (c->extract_by_minimizer && !(c->cfg.key_mode == MC_KEY_PACKED && c->cfg.k >= SK_MIN_K))
        return fail(c, MC_ESTATE, "internal: keys can only be dealt by minimizer where records are (packed keys, k >= %d)", SK_MIN_K);
    if (!owner_offsets || n_owners == 0 || n_owners > PT_MAX_BUCKETS)
        return fail(c, MC_EINVAL, "mc_extract_keys_dev: bad n_owners / owner_offsets");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    for (uint32_t o = 0; o <= n_owners; o++) owner_offsets[o] = 0;
    if (n_reads == 0) return MC_OK;
    mc_ctx::Pipe &P = c->pipe;
    uint64_t first_off = 0, last_off = 0;
    HIPCHK(c, hipMemcpyAsync(&first_off, d_off, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&last_off, d_off + n_reads, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (last_off != n_bases)
        return fail(c, MC_EINVAL, "mc_extract_keys_dev: read_offsets[n_reads]=%llu but n_bases=%llu",
                    (unsigned long long)last_off, (unsigned long long)n_bases);
    if (d_keys) {  // (the pass that writes the keys: their read pointers refer to this context's read store)
        const int64_t in_store = c->extract_in_store;  // (mc_group: tokenised on this device, in the store already)
        c->extract_in_store = -1;
        int rrc = rs_append(c, d_words, first_off, last_off, in_store);
        if (rrc) return rrc;
    } else {
        c->cur_ptr_base = ~0ull;
    }
    const uint64_t n_tiles_abs = (last_off + PT_TILE - 1) / PT_TILE;
    int rc = ensure_buf(c, &P.tile_first, &P.tiles1_cap, n_tiles_abs);
    if (rc) return rc;
    if (!P.cursors1) HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&P.cursors1), PT_MAX_BUCKETS * CURSOR1_STRIDE * sizeof(uint32_t)));
    DevBuf<uint64_t> d_bases;
    HIPCHK(c, d_bases.alloc(n_owners));
    const SpillView nosp{nullptr, nullptr, nullptr, 0, nullptr};
    // pass 1: how many keys every owner gets
    HIPCHK(c, hipMemsetAsync(P.cursors1, 0, PT_MAX_BUCKETS * CURSOR1_STRIDE * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_tile_first_read, dim3((unsigned)((n_tiles_abs + 255) / 256)), dim3(256), 0, c->stream, d_off, n_reads,
                       n_tiles_abs, P.tile_first);
    launch_p1_reads(c, d_words, d_off, n_reads, first_off, last_off, n_tiles_abs, P.tile_first, n_owners, P.cursors1, 0, nullptr,
                    nullptr, nosp, 1, nullptr);
    HIPCHK(c, hipGetLastError());
    std::vector<uint32_t> raw((size_t)n_owners * CURSOR1_STRIDE);
    HIPCHK(c, hipMemcpyAsync(raw.data(), P.cursors1, raw.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<uint64_t> bases(n_owners);
    for (uint32_t o = 0; o < n_owners; o++) {
        bases[o] = owner_offsets[o];
        owner_offsets[o + 1] = owner_offsets[o] + raw[(size_t)o * CURSOR1_STRIDE];
    }
    if (!d_keys) return MC_OK;
    if (owner_offsets[n_owners] > cap)
        return fail(c, MC_EINVAL, "mc_extract_keys_dev: %llu keys but capacity %llu",
                    (unsigned long long)owner_offsets[n_owners], (unsigned long long)cap);
    // pass 2: the same tiles again, now writing every owner's keys (and hints) into its packed range
    HIPCHK(c, hipMemcpyAsync(d_bases.p, bases.data(), n_owners * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(P.cursors1, 0, PT_MAX_BUCKETS * CURSOR1_STRIDE * sizeof(uint32_t), c->stream));
    launch_p1_reads(c, d_words, d_off, n_reads, first_off, last_off, n_tiles_abs, P.tile_first, n_owners, P.cursors1, 0,
                    reinterpret_cast<uint64_t *>(d_keys), d_hints, nosp, 2, d_bases.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MC_OK;
}

uint64_t mc_superkmer_capacity(mc_ctx *c, uint64_t n_windows, uint64_t n_reads)
{
    if (!c || !c->sk_form) return 0;
    return sk_records_bound(c, n_windows, n_reads);
}

int mc_extract_superkmers_dev(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_off, uint64_t n_reads, uint64_t n_bases,
                              uint32_t n_owners, uint64_t *d_recs, uint32_t *d_bins, uint64_t cap, uint64_t *owner_offsets)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->sk_form) return fail(c, MC_ESTATE, "mc_extract_superkmers_dev: this context does not count through super-k-mers (mc_superkmer_capacity() == 0)");
    if (!owner_offsets || !d_recs || !d_bins || n_owners == 0 || n_owners > PT_MAX_BUCKETS)
        return fail(c, MC_EINVAL, "mc_extract_superkmers_dev: bad argument");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    for (uint32_t o = 0; o <= n_owners; o++) owner_offsets[o] = 0;
    if (n_reads == 0) return MC_OK;
    mc_ctx::Pipe &P = c->pipe;
    uint64_t first_off = 0, last_off = 0;
    HIPCHK(c, hipMemcpyAsync(&first_off, d_off, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&last_off, d_off + n_reads, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (last_off != n_bases)
        return fail(c, MC_EINVAL, "mc_extract_superkmers_dev: read_offsets[n_reads]=%llu but n_bases=%llu",
                    (unsigned long long)last_off, (unsigned long long)n_bases);
    {
        const int64_t in_store = c->extract_in_store;  // (mc_group: tokenised on this device, in the store already)
        c->extract_in_store = -1;
        int rrc = rs_append(c, d_words, first_off, last_off, in_store);
        if (rrc) return rrc;
    }
    // The pieces go into pipe.a_recs, where the merge kernel may have left the list of solid k-mers (P3Emit): from here on
    // that list is gone, whether or not this rank then adds any record of its own (as pipe_prepare says for every run).
    c->solid_list_fresh = false;
    // windows <= bases: capacity of the (owner, segment) pieces from the same bound the caller sized its buffer with
    const uint64_t bound = sk_records_bound(c, n_bases - first_off, n_reads);
    const uint32_t nseg = P1W_SEGMENTS;
    constexpr uint32_t own_tile = p1w_tile(true);  // k_sk1w_extract<true>
    uint64_t seg_cap = (uint64_t)((double)bound / (double)n_owners / (double)nseg * 1.25) + 64;
    {   // a workgroup (= segment) takes whole tiles, one per wave and round: with few tiles some segments get more than others, or any at all
        const uint64_t n_waves = (uint64_t)nseg * P1W_WAVES;
        const uint64_t tiles = (last_off - first_off + own_tile - 1) / own_tile + 1, per_wg = (tiles + n_waves - 1) / n_waves * P1W_WAVES;
        const double per_tile = (double)bound / (double)std::max<uint64_t>(tiles - 1, 1);
        seg_cap = std::max<uint64_t>(seg_cap, (uint64_t)((double)per_wg * per_tile / (double)n_owners * 1.3) + 64);
    }
    if ((uint64_t)n_owners * nseg * seg_cap >= 0xFFFFFFFFull)
        return fail(c, MC_EINVAL, "mc_extract_superkmers_dev: batch too large (split the reads)");
    const uint64_t n_tiles_abs = (last_off + own_tile - 1) / own_tile;
    int rc = ensure_buf(c, &P.tile_first, &P.tiles1_cap, n_tiles_abs);
    if (!rc) rc = ensure_buf(c, &P.a_recs, &P.a_recs_cap, (uint64_t)n_owners * nseg * seg_cap);
    if (!rc) rc = ensure_buf(c, &P.a_hints, &P.a_hints_cap, (uint64_t)n_owners * nseg * seg_cap);
    if (!rc) rc = ensure_buf(c, &P.seg_counts1, &P.segs1_cap, (uint64_t)n_owners * nseg);
    if (rc) return rc;
    if (!P.flags) {  // four flags and, behind them, the spill counter: cleared by one fill, read by one copy
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&P.flags), 4 * sizeof(uint32_t) + sizeof(unsigned long long)));
        P.spill_count = reinterpret_cast<unsigned long long *>(P.flags + 4);
    }
    HIPCHK(c, hipMemsetAsync(P.flags, 0, 4 * sizeof(uint32_t) + sizeof(unsigned long long), c->stream));
    DevBuf<unsigned long long> d_piece, d_owner;
    HIPCHK(c, d_piece.alloc((uint64_t)n_owners * nseg));
    HIPCHK(c, d_owner.alloc(n_owners + 1));
    const SkSpill none{nullptr, P.spill_count, 0, P.flags};  // no spill list: an overflow is reported
    launch_tile_first(c, d_off, n_reads, n_tiles_abs, P.tile_first, own_tile);
    hipLaunchKernelGGL(k_sk1w_extract<true>, dim3(nseg), dim3(P1W_THREADS), 0, c->stream, d_words, d_off, n_reads, first_off,
                       last_off, n_tiles_abs, P.tile_first, c->cfg.k, n_owners, P.seg_counts1, seg_cap, P.a_recs, P.a_hints, none, c->cur_ptr_base);
    hipLaunchKernelGGL(k_sk_pack_offsets, dim3(1), dim3(1024), 0, c->stream, P.seg_counts1, n_owners, d_piece.p, d_owner.p, nseg);
    hipLaunchKernelGGL(k_sk_pack, dim3(std::min<uint32_t>(n_owners * nseg, 4096)), dim3(256), 0, c->stream, P.a_recs, P.a_hints,
                       P.seg_counts1, seg_cap, d_piece.p, n_owners * nseg, reinterpret_cast<uint4 *>(d_recs), d_bins, cap);
    HIPCHK(c, hipGetLastError());
    std::vector<unsigned long long> h_owner(n_owners + 1);
    uint32_t lost = 0;
    HIPCHK(c, hipMemcpyAsync(h_owner.data(), d_owner.p, (n_owners + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&lost, P.flags, sizeof lost, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (lost) return fail(c, MC_EOVERFLOW, "mc_extract_superkmers_dev: more super-k-mers than expected (unusually short runs); use mc_extract_keys_dev");
    if (h_owner[n_owners] > cap)
        return fail(c, MC_EINVAL, "mc_extract_superkmers_dev: %llu records but capacity %llu", h_owner[n_owners], (unsigned long long)cap);
    for (uint32_t o = 0; o <= n_owners; o++) owner_offsets[o] = h_owner[o];
    return MC_OK;
}

// fine buckets of a binned exchange for n_owners owners whose tables are laid out like this context's (0: no binned form), and the
// coarse buckets an owner's records are dealt to by the first level (*sub)
static uint32_t skb_fine_buckets(const mc_ctx *c, uint32_t n_owners, uint32_t *sub)
{
    if (!c->sw.exchange_binned || !c->sk_form || !c->mm_k || n_owners == 0 || n_owners > PT_MAX_BUCKETS) return 0;
    uint64_t n_leaves, np1;
    uint32_t g;
    if (plan_levels(c, true, &n_leaves, &g, &np1)) return 0;
    if (n_leaves / np1 <= 1 || (uint64_t)n_owners * np1 > SKB_MAX_CELLS) return 0;
    uint32_t sb = 1;  // about 512 first-level buckets in all (what k_sk1w_extract keeps open on one GPU), a power of two that divides np1
    while ((uint64_t)n_owners * sb * 2 <= PT_MAX_BUCKETS && np1 % (sb * 2) == 0) sb *= 2;
    if (np1 / sb > PT_MAX_LEAVES2 || (uint64_t)n_owners * sb > PT_MAX_BUCKETS1_SK) return 0;
    if (sub) *sub = sb;
    return (uint32_t)np1;
}

uint32_t mc_superkmer_fine_buckets(mc_ctx *c, uint32_t n_owners)
{
    if (!c) return 0;
    std::lock_guard<std::mutex> g(c->mu);
    return skb_fine_buckets(c, n_owners, nullptr);
}

int mc_extract_superkmers_binned_dev(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_off, uint64_t n_reads, uint64_t n_bases,
                                     uint32_t n_owners, uint32_t n_fine, uint64_t *d_recs, uint32_t *d_ptrs, uint64_t cap,
                                     uint32_t *d_fine_counts, uint64_t *owner_offsets, uint64_t *owner_windows)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->sk_form) return fail(c, MC_ESTATE, "mc_extract_superkmers_binned_dev: this context does not count through super-k-mers (mc_superkmer_capacity() == 0)");
    if (!owner_offsets || !owner_windows || !d_recs || !d_ptrs || !d_fine_counts || n_owners == 0 || n_owners > PT_MAX_BUCKETS)
        return fail(c, MC_EINVAL, "mc_extract_superkmers_binned_dev: bad argument");
    // the coarse buckets of the first level: a power of two that divides n_fine, about 512 buckets in all
    uint32_t sub = 1;
    while ((uint64_t)n_owners * sub * 2 <= PT_MAX_BUCKETS && n_fine % (sub * 2) == 0) sub *= 2;
    if (n_fine == 0 || (uint64_t)n_owners * n_fine > SKB_MAX_CELLS || n_fine / sub > PT_MAX_LEAVES2 || (uint64_t)n_owners * sub > PT_MAX_BUCKETS1_SK)
        return fail(c, MC_EINVAL, "mc_extract_superkmers_binned_dev: %u fine buckets for %u owners (mc_superkmer_fine_buckets says how many)", n_fine, n_owners);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    for (uint32_t o = 0; o <= n_owners; o++) owner_offsets[o] = 0;
    for (uint32_t o = 0; o < n_owners; o++) owner_windows[o] = 0;
    const uint64_t n_cells = (uint64_t)n_owners * n_fine;
    HIPCHK(c, hipMemsetAsync(d_fine_counts, 0, n_cells * sizeof(uint32_t), c->stream));
    if (n_reads == 0) return MC_OK;
    mc_ctx::Pipe &P = c->pipe;
    uint64_t first_off = 0, last_off = 0;
    HIPCHK(c, hipMemcpyAsync(&first_off, d_off, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&last_off, d_off + n_reads, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (last_off != n_bases)
        return fail(c, MC_EINVAL, "mc_extract_superkmers_binned_dev: read_offsets[n_reads]=%llu but n_bases=%llu",
                    (unsigned long long)last_off, (unsigned long long)n_bases);
    {
        const int64_t in_store = c->extract_in_store;  // (mc_group: tokenised on this device, in the store already)
        c->extract_in_store = -1;
        int rrc = rs_append(c, d_words, first_off, last_off, in_store);
        if (rrc) return rrc;
    }
    c->solid_list_fresh = false;  // (the pieces go into pipe.a_recs: mc_extract_superkmers_dev says what that ends)
    const uint64_t bound = sk_records_bound(c, n_bases - first_off, n_reads);
    const uint32_t nseg = P1W_SEGMENTS, n_buckets = n_owners * sub;
    constexpr uint32_t own_tile = p1w_tile(true);  // k_sk1w_extract<true, false, true>
    uint64_t seg_cap = (uint64_t)((double)bound / (double)n_buckets / (double)nseg * 1.25) + 64;
    {   // a workgroup (= segment) takes whole tiles, one per wave and round: with few tiles some segments get more than others, or any at all
        const uint64_t n_waves = (uint64_t)nseg * P1W_WAVES;
        const uint64_t tiles = (last_off - first_off + own_tile - 1) / own_tile + 1, per_wg = (tiles + n_waves - 1) / n_waves * P1W_WAVES;
        const double per_tile = (double)bound / (double)std::max<uint64_t>(tiles - 1, 1);
        seg_cap = std::max<uint64_t>(seg_cap, (uint64_t)((double)per_wg * per_tile / (double)n_buckets * 1.3) + 64);
    }
    if ((uint64_t)n_buckets * nseg * seg_cap >= 0xFFFFFFFFull)
        return fail(c, MC_EINVAL, "mc_extract_superkmers_binned_dev: batch too large (split the reads)");
    const uint64_t n_tiles_abs = (last_off + own_tile - 1) / own_tile;
    int rc = ensure_buf(c, &P.tile_first, &P.tiles1_cap, n_tiles_abs);
    if (!rc) rc = ensure_buf(c, &P.a_recs, &P.a_recs_cap, (uint64_t)n_buckets * nseg * seg_cap);
    if (!rc) rc = ensure_buf(c, &P.a_hints, &P.a_hints_cap, (uint64_t)n_buckets * nseg * seg_cap);
    if (!rc) rc = ensure_buf(c, &P.seg_counts1, &P.segs1_cap, (uint64_t)n_buckets * nseg);
    if (!rc) rc = ensure_buf(c, &P.skb_rows, &P.skb_rows_cap, (uint64_t)nseg * n_cells);
    if (!rc) rc = ensure_buf(c, &P.skb_cell_start, &P.skb_cell_start_cap, n_cells);
    if (!rc) rc = ensure_buf(c, &P.skb_small, &P.skb_small_cap, (uint64_t)P1W_SEGMENTS + 2 * PT_MAX_BUCKETS + 8);
    if (rc) return rc;
    if (!P.flags) {  // four flags and, behind them, the spill counter: cleared by one fill, read by one copy
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&P.flags), 4 * sizeof(uint32_t) + sizeof(unsigned long long)));
        P.spill_count = reinterpret_cast<unsigned long long *>(P.flags + 4);
    }
    HIPCHK(c, hipMemsetAsync(P.flags, 0, 4 * sizeof(uint32_t) + sizeof(unsigned long long), c->stream));
    unsigned long long *d_owner = P.skb_small, *d_win = P.skb_small + n_owners + 1;  // owner offsets (n_owners + 1), owner windows (n_owners)
    HIPCHK(c, hipMemsetAsync(d_win, 0, n_owners * sizeof(unsigned long long), c->stream));
    const SkSpill none{nullptr, P.spill_count, 0, P.flags};  // no spill list: an overflow is reported
    launch_tile_first(c, d_off, n_reads, n_tiles_abs, P.tile_first, own_tile);
    hipLaunchKernelGGL((k_sk1w_extract<true, false, true>), dim3(nseg), dim3(P1W_THREADS), 0, c->stream, d_words, d_off, n_reads, first_off,
                       last_off, n_tiles_abs, P.tile_first, c->cfg.k, n_owners, P.seg_counts1, seg_cap, P.a_recs, P.a_hints, none, c->cur_ptr_base,
                       0u, 0u, SkBinned{sub, n_fine, P.skb_rows, d_win});
    hipLaunchKernelGGL(k_skb_colsum, dim3((unsigned)((n_cells + 255) / 256), 16), dim3(256), 0, c->stream, P.skb_rows, nseg, (uint32_t)n_cells, d_fine_counts);
    hipLaunchKernelGGL(k_skb_offsets, dim3(1), dim3(1024), 0, c->stream, d_fine_counts, n_owners, n_fine, P.skb_cell_start, d_owner);
    // every (owner, coarse bucket)'s segments into the owner's fine buckets, at their exact places in the caller's buffer
    hipLaunchKernelGGL((k_sk2_scatter_staged<MC_SK2_ITEMS, false, true>), dim3(n_buckets), dim3(PT_THREADS), 0, c->stream, P.a_recs, P.a_hints, seg_cap,
                       P.seg_counts1, n_buckets, sub, n_fine / sub, nullptr, cap, reinterpret_cast<uint4 *>(d_recs), d_ptrs, none, nseg, nullptr, P.skb_cell_start);
    HIPCHK(c, hipGetLastError());
    std::vector<unsigned long long> h(2 * n_owners + 1);
    uint32_t lost = 0;
    HIPCHK(c, hipMemcpyAsync(h.data(), d_owner, (2 * n_owners + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&lost, P.flags, sizeof lost, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (lost) return fail(c, MC_EOVERFLOW, "mc_extract_superkmers_binned_dev: more super-k-mers than expected (unusually short runs); use mc_extract_keys_dev");
    if (h[n_owners] > cap)
        return fail(c, MC_EINVAL, "mc_extract_superkmers_binned_dev: %llu records but capacity %llu", h[n_owners], (unsigned long long)cap);
    for (uint32_t o = 0; o <= n_owners; o++) owner_offsets[o] = h[o];
    for (uint32_t o = 0; o < n_owners; o++) owner_windows[o] = h[n_owners + 1 + o];
    return MC_OK;
}

static int add_superkmers_locked(mc_ctx *c, const uint64_t *d_recs, const uint32_t *d_bins, uint64_t n);

int mc_add_superkmers_binned_dev(mc_ctx *c, const uint64_t *d_recs, const uint32_t *d_ptrs, uint64_t n, uint64_t n_windows, uint32_t n_fine,
                                 uint32_t n_parts, const uint64_t *part_offsets, const uint32_t *d_part_counts)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->sk_form) return fail(c, MC_ESTATE, "mc_add_superkmers_binned_dev: this context does not count through super-k-mers");
    if (n && (!d_recs || !d_ptrs || !part_offsets || !d_part_counts || n_parts == 0 || n_fine == 0)) return fail(c, MC_EINVAL, "mc_add_superkmers_binned_dev: bad argument");
    if (n) {
        bool ok = part_offsets[0] == 0 && part_offsets[n_parts] == n;
        for (uint32_t p = 0; p < n_parts && ok; p++) ok = part_offsets[p] <= part_offsets[p + 1];
        if (!ok) return fail(c, MC_EINVAL, "mc_add_superkmers_binned_dev: the parts must lie back to back over the %llu records", (unsigned long long)n);
    }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (n && c->mm_k) {
        c->ptr_tries = c->all_ptrs ? 1 : 16;  // (records of ranks that keep no read store carry no pointer)
        int rc = add_records_binned(c, reinterpret_cast<const uint4 *>(d_recs), d_ptrs, n, n_windows, n_fine, n_parts, part_offsets, d_part_counts);
        if (rc != RUN_NOT_BINNED) {
            if (rc) return abi_result(c, rc);
            c->st.binned_runs++;
            counts_changed(c);
            return MC_OK;
        }
    }
    return abi_result(c, add_superkmers_locked(c, d_recs, d_ptrs, n));  // (this table's buckets are not unions of the fine ones: records are records in any order)
}

int mc_add_superkmers_dev(mc_ctx *c, const uint64_t *d_recs, const uint32_t *d_bins, uint64_t n)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->sk_form) return fail(c, MC_ESTATE, "mc_add_superkmers_dev: this context does not count through super-k-mers");
    if ((!d_recs || !d_bins) && n) return fail(c, MC_EINVAL, "mc_add_superkmers_dev: null pointer");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return abi_result(c, add_superkmers_locked(c, d_recs, d_bins, n));
}

static int add_superkmers_locked(mc_ctx *c, const uint64_t *d_recs, const uint32_t *d_bins, uint64_t n)
{
    c->ptr_tries = c->all_ptrs ? 1 : 16;  // (records of ranks that keep no read store carry no pointer)
    if (!c->mm_k) {  // the context gave up minimizer bins (to_hash_regions): the records are expanded by the direct kernel
        int rc = add_records_direct(c, reinterpret_cast<const uint4 *>(d_recs), d_bins, n);
        if (rc) return rc;
        counts_changed(c);
        return MC_OK;
    }
    const uint64_t max_batch = 1ull << 28;  // records per pipeline run (32-bit bucket indices)
    for (uint64_t i = 0; i < n; i += max_batch) {
        const uint64_t m = std::min<uint64_t>(max_batch, n - i);
        int rc = add_records_partitioned(c, reinterpret_cast<const uint4 *>(d_recs) + i, d_bins + i, m);
        if (rc) return rc;
    }
    counts_changed(c);
    return MC_OK;
}

int mc_export_dev(mc_ctx *c, int min_cov, int64_t *d_keys, int16_t *d_counts, uint32_t *d_hints, uint64_t cap,
                  uint64_t *n_out)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->finalized) return fail(c, MC_ESTATE, "mc_export: call mc_finalize_counts first");
    if (!n_out) return fail(c, MC_EINVAL, "mc_export: n_out is null");
    if (d_keys && !d_counts) return fail(c, MC_EINVAL, "mc_export: counts is null");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    unsigned long long *cursor = c->d_ctr + 2;
    if (!d_keys && c->solid_tracked && c->cov_hint == min_cov && min_cov > 0 && !c->virgin) {
        cursor = c->d_ctr + 6;  // counting only, and k_p3_merge kept the number of keys at this threshold up to date
    } else if (d_keys && c->solid_list_fresh && c->solid_tracked && c->cov_hint == min_cov && min_cov > 0 && !c->virgin && c->mm_k) {
        // ... and listed them (the list stays: a BFS set-up on this context can still use it)
        HIPCHK(c, hipMemsetAsync(cursor, 0, sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL(k_export_list, dim3(std::min<uint32_t>(c->solid_list_segs, 2048u)), dim3(256), 0, c->stream, c->pipe.a_recs,
                           c->pipe.emit_counts, c->solid_list_segs, c->solid_list_segcap, d_keys, d_counts, d_hints, cap, cursor);
        HIPCHK(c, hipGetLastError());
        c->st.solid_list_builds++;
    } else {
        HIPCHK(c, hipMemsetAsync(cursor, 0, sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL(k_export, dim3(grid_for(c->n_slots(), 256)), dim3(256), 0, c->stream, c->slots, c->n_slots(),
                           min_cov, d_keys, d_counts, d_hints, cap, cursor, c->dup_filter());
        HIPCHK(c, hipGetLastError());
    }
    unsigned long long n = 0, empty_cnt = 0;
    HIPCHK(c, hipMemcpyAsync(&n, cursor, sizeof n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&empty_cnt, c->d_ctr + 1, sizeof empty_cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the key equal to EMPTY_KEY is counted out of band (hash modes only)
    const int ec = empty_cnt > 32767ull ? 32767 : (int)empty_cnt;
    if (empty_cnt && ec >= min_cov) {
        if (d_keys && n < cap) {
            const int64_t kk = (int64_t)EMPTY_KEY;
            const int16_t cc = (int16_t)ec;
            HIPCHK(c, hipMemcpy(d_keys + n, &kk, 8, hipMemcpyHostToDevice));
            HIPCHK(c, hipMemcpy(d_counts + n, &cc, 2, hipMemcpyHostToDevice));
            if (d_hints) HIPCHK(c, hipMemset(d_hints + n, 0, 4));
        }
        n++;
    }
    *n_out = n;
    if (d_keys && n > cap) return fail(c, MC_EINVAL, "mc_export: %llu pairs but capacity %llu", n, (unsigned long long)cap);
    return MC_OK;
}

int mc_export(mc_ctx *c, int min_cov, int64_t *keys, int16_t *counts, uint64_t cap, uint64_t *n_out)
{
    if (!c) return MC_EINVAL;
    if (!keys) return mc_export_dev(c, min_cov, nullptr, nullptr, nullptr, 0, n_out);
    DevBuf<int64_t> dk;
    DevBuf<int16_t> dc;
    {
        std::lock_guard<std::mutex> g(c->mu);
        HIPCHK(c, hipSetDevice(c->cfg.device));
        HIPCHK(c, alloc_result(c, dk, cap));
        HIPCHK(c, alloc_result(c, dc, cap));
    }
    int rc = mc_export_dev(c, min_cov, dk.p, dc.p, nullptr, cap, n_out);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipMemcpy(keys, dk.p, *n_out * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(counts, dc.p, *n_out * 2, hipMemcpyDeviceToHost));
    return MC_OK;
}

// ---- .kmers.bin (src/io/IOUtils.java:39-65 printKmers, :94-126 loadKmers, src/io/KmersLoadWorker.java:9-23)

int mc_save_kmers(mc_ctx *c, const char *bin_path, const char *stat_path, int threshold, uint64_t *n_total, uint64_t *n_written)
{
    if (!c) return MC_EINVAL;
    if (n_total) *n_total = 0;
    if (n_written) *n_written = 0;
    if (!bin_path) return fail(c, MC_EINVAL, "mc_save_kmers: null path");
    uint64_t n = 0;
    int rc = mc_export(c, 0, nullptr, nullptr, 0, &n);
    if (rc) return rc;
    std::vector<int64_t> keys(std::max<uint64_t>(n, 1));
    std::vector<int16_t> counts(std::max<uint64_t>(n, 1));
    if (n) {
        rc = mc_export(c, 0, keys.data(), counts.data(), n, &n);
        if (rc) return rc;
    }
    FILE *f = fopen(bin_path, "wb");
    if (!f) return fail(c, MC_EINVAL, "mc_save_kmers: cannot write %s", bin_path);
    std::vector<unsigned char> buf;
    buf.reserve(10u << 20);
    std::vector<uint64_t> hist(32768, 0);  // QuickQuantitativeStatistics<Short>: frequency -> number of such k-mers
    uint64_t good = 0;
    bool io_ok = true;
    for (uint64_t i = 0; i < n; i++) {
        const int16_t v = counts[i];
        hist[(size_t)v]++;
        if (v > threshold) {  // DataOutputStream.writeLong / writeShort: big-endian
            const uint64_t kk = (uint64_t)keys[i];
            for (int b = 7; b >= 0; b--) buf.push_back((unsigned char)(kk >> (8 * b)));
            buf.push_back((unsigned char)((uint16_t)v >> 8));
            buf.push_back((unsigned char)((uint16_t)v & 0xFF));
            good++;
            if (buf.size() >= (10u << 20)) { io_ok = io_ok && fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); }
        }
    }
    if (!buf.empty()) io_ok = io_ok && fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    io_ok = (fclose(f) == 0) && io_ok;
    if (!io_ok) return fail(c, MC_EINVAL, "mc_save_kmers: error writing %s", bin_path);
    if (stat_path) {
        FILE *sf = fopen(stat_path, "w");
        if (!sf) return fail(c, MC_EINVAL, "mc_save_kmers: cannot write %s", stat_path);
        fputs("# k-mer frequency\tnumber of such k-mers\n", sf);
        for (size_t v = 0; v < hist.size(); v++)
            if (hist[v]) fprintf(sf, "%zu\t%llu\n", v, (unsigned long long)hist[v]);
        fputs("\n", sf);  // (println of a string that already ends with a newline)
        if (fclose(sf) != 0) return fail(c, MC_EINVAL, "mc_save_kmers: error writing %s", stat_path);
    }
    if (n_total) *n_total = n;
    if (n_written) *n_written = good;
    return MC_OK;
}

int mc_load_kmers(mc_ctx *c, const char *path, int freq_threshold, uint64_t *n_records, uint64_t *n_added)
{
    if (!c) return MC_EINVAL;
    if (n_records) *n_records = 0;
    if (n_added) *n_added = 0;
    if (!path) return fail(c, MC_EINVAL, "mc_load_kmers: null path");
    FILE *f = fopen(path, "rb");
    if (!f) return fail(c, MC_EINVAL, "Failed to read from file %s", path);
    const size_t batch = 8u << 20;  // records per upload
    std::vector<unsigned char> raw(batch * 10);
    std::vector<int64_t> keys(batch);
    std::vector<int16_t> counts(batch);
    DevBuf<int64_t> dk;
    DevBuf<int16_t> dc;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (hipSetDevice(c->cfg.device) != hipSuccess || dk.alloc(batch) != hipSuccess || dc.alloc(batch) != hipSuccess) {
            fclose(f);
            return fail(c, MC_ENOMEM, "mc_load_kmers: device allocation failed");
        }
    }
    uint64_t total = 0, added = 0;
    int rc = MC_OK;
    for (;;) {
        const size_t got = fread(raw.data(), 1, raw.size(), f);
        if (got == 0) break;
        if (got % 10 != 0) { rc = fail(c, MC_EINVAL, "Can't load kmers from file %s: its length is not a multiple of the 10-byte record", path); break; }
        size_t m = 0;
        for (size_t i = 0; i < got; i += 10) {
            uint64_t kk = 0;
            for (int b = 0; b < 8; b++) kk = (kk << 8) | raw[i + b];
            const int16_t v = (int16_t)(((uint16_t)raw[i + 8] << 8) | raw[i + 9]);
            total++;
            if (v > freq_threshold) { keys[m] = (int64_t)kk; counts[m] = v; m++; }
        }
        if (m) {
            {
                std::lock_guard<std::mutex> g(c->mu);
                if (hipMemcpy(dk.p, keys.data(), m * 8, hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(dc.p, counts.data(), m * 2, hipMemcpyHostToDevice) != hipSuccess) {
                    rc = fail(c, MC_EHIP, "mc_load_kmers: upload failed");
                    break;
                }
            }
            rc = mc_add_pairs_dev(c, dk.p, dc.p, nullptr, m);
            if (rc) break;
            added += m;
        }
    }
    fclose(f);
    if (rc) return rc;
    if (n_records) *n_records = total;
    if (n_added) *n_added = added;
    return MC_OK;
}

int mc_get_stats(mc_ctx *c, mc_stats *out)
{
    if (!c || !out) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    c->st.dup_keys = c->dup.merged ? c->dup.n_keys : 0;
    *out = c->st;
    return MC_OK;
}

int mc_reset_stats(mc_ctx *c)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    const uint64_t slots = c->st.table_slots, bytes = c->st.table_bytes, left = c->st.left_bins, unchecked = c->st.dup_unchecked;
    c->st = mc_stats{};
    c->st.table_slots = slots;
    c->st.table_bytes = bytes;
    c->st.left_bins = left;  // (states of the table, not counters)
    c->st.dup_unchecked = unchecked;
    return MC_OK;
}

int mc_trim(mc_ctx *c)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    mc_ctx::Pipe &P = c->pipe;
    const int dev = c->cfg.device;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the blocks may be reused by another context at once: see mc_destroy)
    if (c->pipe_stream) HIPCHK(c, hipStreamSynchronize(c->pipe_stream));
    // (the list of solid k-mers sits in a_recs, its fill levels in emit_counts: they stay while the list is valid)
    uint4 *keep_recs = nullptr;
    uint64_t keep_cap = 0;
    uint32_t *keep_counts = nullptr;
    if (c->solid_list_fresh) {
        keep_recs = P.a_recs; keep_cap = P.a_recs_cap; keep_counts = P.emit_counts;
        P.a_recs = nullptr; P.a_recs_cap = 0; P.emit_counts = nullptr;
    }
    P.release(dev);
    P.a_recs = keep_recs; P.a_recs_cap = keep_cap; P.emit_counts = keep_counts;
    g_scratch_pool.put(dev, c->d_ovf_tmp, c->ovf_tmp_cap * sizeof(uint4));
    c->d_ovf_tmp = nullptr; c->ovf_tmp_cap = 0;
    dup_release_streams(c);
    g_scratch_pool.release(dev);
    g_table_pool.release(dev);
    return MC_OK;
}

int mc_synth_reads_dev(mc_ctx *c, uint64_t gseed, uint64_t n_contigs, uint64_t contig_len, uint64_t rseed,
                       uint64_t first_read, uint64_t n_reads, uint32_t L, uint32_t err, uint64_t *d_words,
                       uint64_t *d_off)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!d_words || !d_off || n_contigs == 0 || L == 0 || contig_len < L)
        return fail(c, MC_EINVAL, "mc_synth_reads_dev: bad argument");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const uint64_t n_words = (n_reads * (uint64_t)L + 31) / 32 + 1;
    hipLaunchKernelGGL(k_synth_reads, dim3(grid_for(n_words, 256)), dim3(256), 0, c->stream, gseed, n_contigs,
                       contig_len, rseed, first_read, n_reads, L, err, d_words, n_words, d_off);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MC_OK;
}

int mc_synth_genome(uint64_t gseed, uint64_t start, uint64_t n, uint8_t *codes)
{
    if (!codes && n) return MC_EINVAL;
    for (uint64_t i = 0; i < n; i++) codes[i] = (uint8_t)(splitmix(gseed, start + i) & 3);
    return MC_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ the walk's solid table and its checks

namespace {

struct PairSource { const int64_t *keys; const int16_t *counts; const uint32_t *hints; uint64_t n; };

// Builds the solid table for n entries with count >= min_cov, taken from the counting table or (pairs != nullptr)
// from arrays of (key, count, hint).
int solid_build(mc_ctx *c, uint64_t n, int min_cov, double *ms, const PairSource *pairs, bool from_list = false)
{
    c->n_solid = n;
    c->st.solid_kmers = n;
    constexpr uint64_t factor = 4;  // slots per solid key (load factor <= 1/4)
    uint32_t lg = c->sb;
    while (lg < 34 && (1ull << lg) < factor * n) lg++;
    if (lg < SOLID_SB + 1) lg = SOLID_SB + 1;
    if (!c->solid || lg != c->solid_lg) {
        if (c->solid) { (void)hipFree(c->solid); c->solid = nullptr; }
        HIPCHK(c, dev_malloc(c, reinterpret_cast<void **>(&c->solid), sizeof(Slot) << lg));
        c->solid_lg = lg;
    }
    // counting table organised by minimizer bins, or entries from outside: the solid entries are partitioned by
    // their own hash first
    const bool partitioned = true;
    mc_ctx::Pipe &P = c->pipe;
    const uint32_t q = lg - SOLID_SB, sb1 = std::min<uint32_t>(q, 9), sb2 = q - sb1;
    uint64_t scap1 = 0, scap2 = 0;
    int rc;
    if (partitioned) {
        const double m1 = (double)n / (double)(1ull << sb1) / (double)PT_SEGMENTS;
        const double m2 = (double)n / (double)(1ull << q);
        scap1 = (uint64_t)(m1 * 1.25 + 10.0 * std::sqrt(m1) + 64.0);
        scap1 += 64;  // rows of entries are dealt to the segments: one of them may bring a whole row more
        scap2 = (uint64_t)(m2 * 1.15 + 10.0 * std::sqrt(m2) + 64.0);
        const uint64_t need1 = (uint64_t)(1ull << sb1) * PT_SEGMENTS * scap1, need2 = sb2 ? (uint64_t)(1ull << q) * scap2 : 0;
        // The solid list sits in a_recs: the level-1 buckets then go to b_recs and the leaves, once the list has been
        // read, to a_recs -- which must not be reallocated for it (and a one-level build would have to read and
        // write a_recs at once): otherwise the table is swept as usual.
        if (from_list && (!sb2 || need2 > P.a_recs_cap)) from_list = false;  // (a_hints holds nothing of the list: it may grow, or come to be here -- compact runs do without it)
        uint4 **l1_recs = from_list ? &P.b_recs : &P.a_recs, **l2_recs = from_list ? &P.a_recs : &P.b_recs;
        uint32_t **l1_bins = from_list ? &P.b_hints : &P.a_hints, **l2_bins = from_list ? &P.a_hints : &P.b_hints;
        uint64_t *l1_recs_cap = from_list ? &P.b_recs_cap : &P.a_recs_cap, *l2_recs_cap = from_list ? &P.a_recs_cap : &P.b_recs_cap;
        uint64_t *l1_bins_cap = from_list ? &P.b_hints_cap : &P.a_hints_cap, *l2_bins_cap = from_list ? &P.a_hints_cap : &P.b_hints_cap;
        rc = ensure_buf(c, l1_recs, l1_recs_cap, need1);
        if (!rc) rc = ensure_buf(c, l1_bins, l1_bins_cap, need1);
        if (!rc) rc = ensure_buf(c, &P.seg_counts1, &P.segs1_cap, (uint64_t)(1ull << sb1) * PT_SEGMENTS);
        if (!rc && sb2) rc = ensure_buf(c, l2_recs, l2_recs_cap, need2);
        if (!rc && sb2) rc = ensure_buf(c, l2_bins, l2_bins_cap, need2);
        if (!rc && sb2) rc = ensure_buf(c, &P.solid_cursors, &P.solid_cursors_cap, 1ull << q);
        if (rc) return rc;
        if (!P.flags) {  // four flags and, behind them, the spill counter: cleared by one fill, read by one copy
            HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&P.flags), 4 * sizeof(uint32_t) + sizeof(unsigned long long)));
            P.spill_count = reinterpret_cast<unsigned long long *>(P.flags + 4);
        }
        HIPCHK(c, hipMemsetAsync(P.flags, 0, 4 * sizeof(uint32_t) + sizeof(unsigned long long), c->stream));
    }
    const bool list = partitioned && from_list && !pairs;
    uint4 *const r1 = list ? P.b_recs : P.a_recs, *const r2 = list ? P.a_recs : P.b_recs;
    uint32_t *const h1 = list ? P.b_hints : P.a_hints, *const h2 = list ? P.a_hints : P.b_hints;
    c->solid_list_fresh = false;  // (read below, then overwritten by the leaves)
    if (list) c->st.solid_list_builds++;
    rc = timed(c, ms, [&] {
        if (partitioned) {
            uint32_t *leaf_counts = P.solid_cursors;
            const SkSpill none{nullptr, P.spill_count, 0, P.flags};  // no spill list: an overflow is reported
            if (pairs)
                hipLaunchKernelGGL(k_solid_emit_pairs, dim3(PT_SEGMENTS), dim3(PT_THREADS), 0, c->stream, pairs->keys, pairs->counts,
                                   pairs->hints, pairs->n, min_cov, 1u << sb1, P.seg_counts1, scap1, r1, h1, none, c->d_ctr + 1);
            else if (list)
                hipLaunchKernelGGL(k_solid_emit_list, dim3(PT_SEGMENTS), dim3(PT_THREADS), 0, c->stream, P.a_recs, P.emit_counts,
                                   c->solid_list_segs, c->solid_list_segcap, 1u << sb1, P.seg_counts1, scap1, r1, h1, none);
            else
                hipLaunchKernelGGL(k_solid_emit, dim3(PT_SEGMENTS), dim3(PT_THREADS), 0, c->stream, c->slots, c->n_slots(), min_cov, 1u << sb1,
                                   P.seg_counts1, scap1, r1, h1, none);
            if (sb2)
                hipLaunchKernelGGL(k_sk2_scatter, dim3(1u << sb1), dim3(PT_THREADS), 0, c->stream, r1, h1, scap1,
                                   P.seg_counts1, 1u << sb1, 1u << sb1, 1u << sb2, leaf_counts, scap2, r2, h2, none, (uint32_t)PT_SEGMENTS, 1);
            hipLaunchKernelGGL(k_solid_from_leaves, dim3((unsigned)std::min<uint64_t>(1ull << q, 256 * 2 * 8)), dim3(512), 0, c->stream,
                               sb2 ? r2 : r1, sb2 ? leaf_counts : P.seg_counts1, sb2 ? scap2 : scap1,
                               sb2 ? 1u : (uint32_t)PT_SEGMENTS, c->solid_view(), lg);
        }
    });
    if (rc) return rc;
    uint32_t fatal = 0;
    HIPCHK(c, hipMemcpy(&fatal, c->d_fatal, sizeof fatal, hipMemcpyDeviceToHost));
    if (fatal) return fail(c, MC_EOVERFLOW, "a region of the solid k-mer table filled up (hash skew)");
    if (partitioned) {
        uint32_t lost = 0;
        HIPCHK(c, hipMemcpy(&lost, P.flags, sizeof lost, hipMemcpyDeviceToHost));
        if (lost) return fail(c, MC_EOVERFLOW, "internal: a bucket of the solid-table build overflowed (hash skew)");
    }
    c->solid_cov = min_cov;
    return MC_OK;
}

}  // namespace

// Builds (or reuses) the solid table for this threshold.
int ensure_solid(mc_ctx *c, int min_cov, double *ms)
{
    if (c->d_shards || (c->sw.bfs_direct && !c->solid_external)) {  // the walk looks its k-mers up in the counting table(s): nothing to build
        c->solid_is_table = true;
        c->solid_cov = min_cov;
        return MC_OK;
    }
    c->solid_is_table = false;
    if (c->solid_cov == min_cov && c->solid) return MC_OK;
    if (c->dup.merged && c->dup.n_tw)  // (a copy is built by key: the keys that sit in several regions meet in hash-prefix regions first)
        if (int brc = by_key_ready(c)) return brc;
    if (c->solid_external)
        return fail(c, MC_ESTATE, "this context's solid table came from mc_solid_from_pairs_dev at coverage %d; it serves that threshold only",
                    c->solid_external_cov);
    c->solid_cov = -1; c->solid_external = false;
    unsigned long long *cursor = c->d_ctr + 2;
    int rc;
    bool from_list = false;
    if (c->solid_tracked && c->cov_hint == min_cov && min_cov > 0 && !c->virgin) {
        cursor = c->d_ctr + 6;  // kept up to date by k_p3_merge
        from_list = c->solid_list_fresh && c->mm_k;  // ... which also listed those keys
    } else {
        HIPCHK(c, hipMemsetAsync(cursor, 0, sizeof(unsigned long long), c->stream));
        rc = timed(c, ms, [&] {
            hipLaunchKernelGGL(k_export, dim3(grid_for(c->n_slots(), 256)), dim3(256), 0, c->stream, c->slots,
                               c->n_slots(), min_cov, (int64_t *)nullptr, (int16_t *)nullptr, (uint32_t *)nullptr, (uint64_t)0, cursor);
        });
        if (rc) return rc;
        c->st.solid_sweeps++;
    }
    unsigned long long n = 0;
    HIPCHK(c, hipMemcpy(&n, cursor, sizeof n, hipMemcpyDeviceToHost));
    return solid_build(c, n, min_cov, ms, nullptr, from_list);
}

// After a walk over a table of hash keys in minimizer bins: every look-up of it that came back "absent" is asked again by key
// (dup_check.h, "Look-ups of k-mers that were never counted").  *redo: a key turned up that a string nobody counted had asked for;
// it has been given a slot in that string's bin, the table has been joined again, and the walks must be repeated.
int phantom_verify(mc_ctx *c, uint32_t n_jobs, std::vector<std::unique_ptr<BfsJobBuffers>> &B, const std::vector<BfsCtl> &ctl, bool *redo)
{
    *redo = false;
    mc_ctx::Dup &D = c->dup;
    if (!hash_bins(c) || !c->solid_is_table || c->d_shards || !dup_check_on() || !D.checked) return MC_OK;
    const bool by_streams = D.l2_valid;  // (else: the join's streams are gone -- mc_trim, a pipeline run since --: one sweep of the table instead)
    uint64_t cap = 64;
    for (uint32_t j = 0; j < n_jobs; j++) cap += ctl[j].n * (B[j]->S.dir == 0 ? 8 : 4) + B[j]->S.n_seeds;
    if (cap >= (1ull << 32)) return fail(c, MC_EOVERFLOW, "mc_bfs: %llu look-ups to check by key", (unsigned long long)cap);
    const uint64_t hit_cap = 4096;
    const uint64_t words = 3 * cap + (cap + 1) / 2 + hit_cap / 2 + 8;  // key, hi, lo; order (32-bit); hits (32-bit); two counters
    if (D.pq_cap < words) {
        if (D.pq_mem) (void)hipFree(D.pq_mem);
        D.pq_mem = nullptr; D.pq_cap = 0;
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&D.pq_mem), words * 2 * 8));
        D.pq_cap = words * 2;
    }
    uint64_t set_slots = 1024;  // (the sweep form: the queries as a set, 12 bytes an entry in the same block)
    while (set_slots < 2 * cap) set_slots <<= 1;
    const uint32_t G = by_streams ? DUP_B1 << D.l2.f2_lg : (uint32_t)std::min<uint64_t>(3 * set_slots, 0xFFFFFFF0ull);
    if (!by_streams && 3 * set_slots > 0xFFFFFFF0ull) return fail(c, MC_EOVERFLOW, "mc_bfs: %llu look-ups to check by key", (unsigned long long)cap);
    if (D.pq_groups_cap < G) {
        if (D.pq_groups) (void)hipFree(D.pq_groups);
        D.pq_groups = nullptr; D.pq_groups_cap = 0;
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&D.pq_groups), (uint64_t)G * sizeof(uint32_t)));
        D.pq_groups_cap = G;
    }
    unsigned long long *ctr = D.pq_mem;  // [0] queries, [1] hits
    PhantomQ q{D.pq_mem + 8, D.pq_mem + 8 + cap, D.pq_mem + 8 + 2 * cap, ctr, cap};
    uint32_t *next = reinterpret_cast<uint32_t *>(D.pq_mem + 8 + 3 * cap);
    uint32_t *hits = next + 2 * ((cap + 1) / 2);
    uint32_t *head = D.pq_groups;
    HIPCHK(c, hipMemsetAsync(ctr, 0, 2 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(head, 0xFF, (by_streams ? (uint64_t)G : 2 * set_slots) * sizeof(uint32_t), c->stream));  // (list heads, or the set's keys: ~0 = free)
    const SolidView t = c->solid_view();
    const int k = c->cfg.k;
    for (uint32_t j = 0; j < n_jobs; j++) {
        const BfsState &S = B[j]->S;
        const int nb = S.dir == 0 ? 8 : 4;
#define PQ_LAUNCH(MODE)                                                                                                                               \
        do {                                                                                                                                          \
            if (ctl[j].n) hipLaunchKernelGGL(k_phantom_queries<MODE>, dim3(grid_for(ctl[j].n * nb, 256)), dim3(256), 0, c->stream, S.hi, S.lo, (uint64_t)ctl[j].n, nb, S.dir, k, t, q); \
            if (S.n_seeds) hipLaunchKernelGGL(k_phantom_queries<MODE>, dim3(grid_for(S.n_seeds, 256)), dim3(256), 0, c->stream, S.seed_hi, S.seed_lo, (uint64_t)S.n_seeds, 0, S.dir, k, t, q); \
        } while (0)
        if (c->cfg.key_mode == MC_KEY_POLY) PQ_LAUNCH(KEY_POLY); else PQ_LAUNCH(KEY_FNV1A);
#undef PQ_LAUNCH
    }
    if (by_streams) {
        hipLaunchKernelGGL(k_pq_link, dim3(256), dim3(256), 0, c->stream, q.key, ctr, cap, D.l2.f2_lg, head, next);
        hipLaunchKernelGGL(k_pq_match, dim3(std::min<uint32_t>(G, 256u * 16u)), dim3(256), 0, c->stream, D.l2, head, next, q.key, hits, ctr + 1, hit_cap);
    } else {
        unsigned long long *qk = reinterpret_cast<unsigned long long *>(D.pq_groups);
        uint32_t *qidx = D.pq_groups + 2 * set_slots;
        hipLaunchKernelGGL(k_pq_set_build, dim3(256), dim3(256), 0, c->stream, q.key, ctr, cap, qk, qidx, set_slots - 1);
        hipLaunchKernelGGL(k_pq_sweep, dim3(grid_for(c->n_slots(), 256, 256 * 16)), dim3(256), 0, c->stream, c->slots, c->n_slots(), qk, qidx, set_slots - 1, hits, ctr + 1, hit_cap);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_scratch + 20, ctr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t n_hits = c->h_scratch[21];
    if (n_hits == 0) return MC_OK;
    // ---- a string nobody counted asked for a key the table holds: the key gets a slot in that string's bin and the join runs again
    int rc = dup_unmerge(c);
    if (rc) return rc;
    const uint64_t nh = std::min<uint64_t>(n_hits, hit_cap);
    hipLaunchKernelGGL(k_alias_insert, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, c->stream, hits, nh, q, c->view(), k);
    HIPCHK(c, hipGetLastError());
    rc = drain_parked(c);  // (no room in that bin's chain: the table gives up its bins, and every look-up is by key from then on)
    if (rc) return rc;
    D.checked = false; D.l1_armed = false; D.l2_valid = false;
    c->solid_tracked = false;  // (slots the merge kernel did not count)
    rc = ensure_dups(c);
    if (rc) return rc;
    *redo = true;
    return MC_OK;
}

extern "C" int mc_solid_from_pairs_dev(mc_ctx *c, const int64_t *d_keys, const int16_t *d_counts, const uint32_t *d_hints, uint64_t n,
                                       int min_cov, uint64_t *n_solid)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (n_solid) *n_solid = 0;
    if ((!d_keys || !d_counts) && n) return fail(c, MC_EINVAL, "mc_solid_from_pairs_dev: null pointer");
    if (min_cov < 0) return fail(c, MC_EINVAL, "mc_solid_from_pairs_dev: negative coverage threshold");
    if (!c->virgin) return fail(c, MC_ESTATE, "mc_solid_from_pairs_dev: the context holds counts; call mc_clear first");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    c->solid_cov = -1;
    c->solid_external = false;
    c->solid_is_table = false;
    unsigned long long *cursor = c->d_ctr + 2;
    HIPCHK(c, hipMemsetAsync(cursor, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_ctr + 1, 0, sizeof(unsigned long long), c->stream));  // the out-of-band count of EMPTY_KEY
    if (n) hipLaunchKernelGGL(k_count_pairs, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, d_counts, d_keys, n, min_cov, cursor);
    HIPCHK(c, hipGetLastError());
    unsigned long long m = 0;
    HIPCHK(c, hipMemcpyAsync(&m, cursor, sizeof m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const PairSource src{d_keys, d_counts, d_hints, n};
    double ms = 0;
    int rc = solid_build(c, m, min_cov, &ms, &src);
    if (rc) return rc;
    c->pending_solid_ms = ms;  // reported with the next BFS
    c->solid_external = true;
    c->solid_external_cov = min_cov;
    c->finalized = true;
    if (n_solid) *n_solid = m;
    return MC_OK;
}

