// The library's context and what more than one unit of it needs (host side; private to libmcgpu.so, not include/mcgpu.h).
//
// The library is seventeen units, each defining and launching its own kernels:
//   mcgpu.hip       the table, the key join, the counting pipeline, the context ABI, and the table work of the walk (solid table,
//                   the check of its "absent" look-ups)
//   reads_file.hip  the device tokeniser's driver, the upload pipeline that feeds it a file's chunks (tokenize_file_chunks: mc_group_add_reads_file
//                   runs on it too) and mc_add_reads_file; the host readers it falls back on are csrc/host/reads_io.cpp, linked into the library
//   walk.hip        the walk's driver and result pool, mc_bfs*, mc_shard_*
//   group.hip       mc_group_* (no kernels)
//   classify.hip    mc_classify_reads*: the reads-classifier's per-read coverage (classify.h: its verdict), and mc_triple_classes*
//   last_copy.hip   mc_reads_last_copy*: the last read with the same bases, for the triple-reads-classifier (hipCUB's radix sort)
//   seq_cov.hip     mc_seq_coverage*: depth and breadth of sequences of any length in up to four tables at once, cut by positions
//   presence.hip    mc_kmer_presence*: which of up to four tables hold each of a list of k-mers, one launch
//   reads_in_set.hip mc_reads_in_set*: every read's windows against a small exact set of k-mers behind a bit filter in LDS
//   components.hip  mc_components*: the connected components of the table's k-mers that a set of sequences holds (union-find over slots)
//   unitigs.hip     mc_unitigs*: what the reference's unitig compaction leaves of a set of k-mers, by link analysis and pointer jumping
//   env_join.hip    mc_env_join*: the join of several graph files' records on their k-mers for environment-finder-multi (members, KC, the two Jaccard tables' sums)
//   whole_reads.hip mc_tokenize_whole*: FASTA / FASTQ text into whole reads with their qualities (DnaQReader's policy) for the classifying tools,
//                   mc_reads_append_dev: slices of such results joined into one array of packed reads;
//                   tokenizer_device.h is what it shares with tokenizer.h, the newline pass and the scan come from reads_file.hip
//   trim_paths.hip  mc_trim_paths*: which k-mers of one BFS pass runTrimPaths keeps (those that reach a `last` one inside the pass), by an index of
//                   the pass's oriented k-mers, contraction with pointer jumping (dir +-1) or union-find (dir 0)
//   kmers_bin.hip   mc_kmers_encode_dev / mc_kmers_decode_dev: the table as .kmers.bin records and back, and mc_save_kmers_gpu / mc_load_kmers_gpu,
//                   which stream them to and from a file in chunks; the scan of the tile counts comes from reads_file.hip
//   render_fastq.hip mc_render_fastq*: the classifiers' FASTQ records as text, up to sixteen output streams a call, for --render gpu; the
//                   scan of the per-block counts comes from reads_file.hip
//   walk_order.hip  mc_walk_order*: the order in which runBfs pops every component's k-mers first and which it pops again, for the fmt-visualizer:
//                   a queue of at most two entries a member, level by level, narrow levels in one workgroup's LDS and wide ones across the grid
// multi_table.h is what seq_cov.hip and presence.hip share: one key's home slots in several tables, the probing behind them, and the
// host's checks of a list of contexts; kmer_set.h what reads_in_set.hip, unitigs.hip and env_join.hip share: the key and hash of a call's exact
// set (trim_paths.hip takes the hash alone).  A function below the "across units" line is what one unit lends another; everything else stays static in its unit.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mcgpu.h"
#include "kmer_device.h"
#include "device_types.h"
#include "switches.h"

using namespace mc;

// Device scratch of the tokeniser (csrc/tokenizer.h), kept between calls: a file is read in chunks of the same size,
// and hipMalloc / hipFree of gigabyte buffers cost milliseconds each.  Best fit with at most 2x slack; at most 48 idle
// blocks (the smallest goes first).
struct DevPool {
    std::vector<std::pair<void *, size_t>> idle;
    hipError_t get(size_t bytes, void **out, size_t *got)
    {
        bytes = std::max<size_t>((bytes + 255) / 256 * 256, 256);
        size_t best = idle.size();
        for (size_t i = 0; i < idle.size(); i++)
            if (idle[i].second >= bytes && idle[i].second <= 2 * bytes + (1u << 20) && (best == idle.size() || idle[i].second < idle[best].second)) best = i;
        if (best < idle.size()) {
            *out = idle[best].first;
            *got = idle[best].second;
            idle.erase(idle.begin() + (long)best);
            return hipSuccess;
        }
        *got = bytes;
        hipError_t e = hipMalloc(out, bytes);
        if (e == hipErrorOutOfMemory && !idle.empty()) {  // give the idle blocks back and try once more
            release();
            e = hipMalloc(out, bytes);
        }
        return e;
    }
    void put(void *p, size_t bytes)
    {
        idle.emplace_back(p, bytes);
        if (idle.size() > 48) {
            size_t small = 0;
            for (size_t i = 1; i < idle.size(); i++)
                if (idle[i].second < idle[small].second) small = i;
            (void)hipFree(idle[small].first);
            idle.erase(idle.begin() + (long)small);
        }
    }
    void release()
    {
        for (auto &b : idle) (void)hipFree(b.first);
        idle.clear();
    }
};
template <class T>
struct PoolBuf {  // RAII: a block of a DevPool
    T *p = nullptr;
    size_t bytes = 0;
    DevPool *pool = nullptr;
    PoolBuf() = default;
    PoolBuf(const PoolBuf &) = delete;
    PoolBuf &operator=(const PoolBuf &) = delete;
    ~PoolBuf() { if (p) pool->put(p, bytes); }
    hipError_t alloc(DevPool *pl, size_t n)
    {
        pool = pl;
        return pl->get(std::max<size_t>(n, 1) * sizeof(T), reinterpret_cast<void **>(&p), &bytes);
    }
};

// Table memory, kept across tables: fresh device memory comes zero-filled by the driver at ~30 GB/s (0.7 s for the 22 GB
// table of configs[1]), which a context without a capacity hint paid every time its table went to its real size.  A
// table that is given up goes here instead of back to the driver (the two largest idle blocks per device are kept) and the
// next table of about its size takes it; any allocation that fails for lack of memory empties the pool and tries again.
struct TablePool {
    std::mutex mu;
    std::map<int, DevPool> per_device;
    bool on = read_pool_switches().table_pool;
    hipError_t get(int dev, size_t bytes, void **out, size_t *got)
    {
        if (!on) { *got = bytes; return hipMalloc(out, bytes); }
        std::lock_guard<std::mutex> g(mu);
        return per_device[dev].get(bytes, out, got);
    }
    void put(int dev, void *p, size_t bytes)
    {
        if (!p) return;
        if (!on) { (void)hipFree(p); return; }
        std::lock_guard<std::mutex> g(mu);
        DevPool &P = per_device[dev];
        P.put(p, bytes);
        while (P.idle.size() > 2) {
            size_t small = 0;
            for (size_t i = 1; i < P.idle.size(); i++)
                if (P.idle[i].second < P.idle[small].second) small = i;
            (void)hipFree(P.idle[small].first);
            P.idle.erase(P.idle.begin() + (long)small);
        }
    }
    void release(int dev)
    {
        std::lock_guard<std::mutex> g(mu);
        per_device[dev].release();
    }
};
extern TablePool g_table_pool;

// The large scratch buffers of the counting pipeline (record and key streams: gigabytes per context), kept across contexts
// the same way: memory handed back with hipFree is reclaimed by the driver lazily and in bulk -- every third fresh context
// of a process that counted configs[1] stalled 1.5 - 4 s in its first launch while that happened.  Blocks of 64 MB or more
// go to this pool (DevPool's limits: best fit with at most 2x slack, 48 idle blocks); an allocation that fails for lack of
// memory empties both pools and tries again.
struct ScratchPool {
    static constexpr size_t MIN_BYTES = 64ull << 20;
    std::mutex mu;
    std::map<int, DevPool> per_device;
    bool on = read_pool_switches().scratch_pool;
    hipError_t get(int dev, size_t bytes, void **out, size_t *got)
    {
        if (!on || bytes < MIN_BYTES) { *got = bytes; return hipMalloc(out, std::max<size_t>(bytes, 1)); }
        std::lock_guard<std::mutex> g(mu);
        return per_device[dev].get(bytes, out, got);
    }
    void put(int dev, void *p, size_t bytes)
    {
        if (!p) return;
        if (!on || bytes < MIN_BYTES) { (void)hipFree(p); return; }
        std::lock_guard<std::mutex> g(mu);
        DevPool &P = per_device[dev];
        P.put(p, bytes);
        for (;;) {  // at most max_idle bytes stay idle (MC_SCRATCH_POOL_GB, default 64): the largest blocks go first
            size_t total = 0, big = 0;
            for (size_t i = 0; i < P.idle.size(); i++) {
                total += P.idle[i].second;
                if (P.idle[i].second > P.idle[big].second) big = i;
            }
            if (total <= max_idle || P.idle.empty()) break;
            (void)hipFree(P.idle[big].first);
            P.idle.erase(P.idle.begin() + (long)big);
        }
    }
    void release(int dev)
    {
        std::lock_guard<std::mutex> g(mu);
        per_device[dev].release();
    }
    size_t max_idle = read_pool_switches().scratch_idle_max;
};
extern ScratchPool g_scratch_pool;

// device buffers of one BFS job, kept in the context between calls
struct BfsJobBuffers {
    BfsState S{};
    uint64_t *d_seed_hi = nullptr, *d_seed_lo = nullptr;
    uint64_t seed_cap = 0;
    BfsJobBuffers() = default;
    BfsJobBuffers(const BfsJobBuffers &) = delete;
    BfsJobBuffers &operator=(const BfsJobBuffers &) = delete;
    void free_arrays()
    {
        (void)hipFree(S.hi); (void)hipFree(S.lo); (void)hipFree(S.dist); (void)hipFree(S.cov);
        (void)hipFree(S.flags); (void)hipFree(S.vis);
        S.hi = S.lo = nullptr; S.dist = nullptr; S.cov = nullptr; S.flags = nullptr; S.vis = nullptr;
    }
    ~BfsJobBuffers()
    {
        free_arrays();
        (void)hipFree(S.ctl);
        (void)hipFree(S.path);
        (void)hipFree(S.box);
        (void)hipFree(S.trace);
        (void)hipFree(d_seed_hi);
        (void)hipFree(d_seed_lo);
    }
};

struct mc_ctx {
    mc_config cfg{};
    mc_switches sw;  // the environment switches, read by mc_create (switches.h)
    std::mutex mu;
    std::string err;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // a side stream: the read store's copy of a batch (rs_append) and the walk's companions (mc_bfs_batch) run here
    hipStream_t pipe_stream = nullptr;
    hipEvent_t ev_piece[8] = {};
    hipEvent_t ev_seq[16] = {};  // behind every kernel of a per-window run in pieces (add_reads_partitioned_once)
    hipEvent_t ev_t[4] = {};  // P1 start, P1 end, P2 end, P3 end of a pipeline run enqueued without a host round trip in between
    // The read store: the packed bases of every read this context was given since the last mc_clear, batch after
    // batch (each starting on a word boundary).  Table slots point into it (read_ptr.h ptr_encode) and the BFS
    // reads its look-ahead from it.  rs_from: a BFS-only context (mc_solid_from_pairs_dev) borrows the store of the
    // context that counted this rank's reads (mc_share_read_store).
    uint64_t *rs_words = nullptr;
    uint64_t rs_cap_words = 0, rs_bases = 0;
    bool rs_enabled = true;
    // mc_set_read_pointers' other modes.  rs_virtual: this context keeps no store, but the reads it extracts or counts sit in ANOTHER
    // context's store (the walking rank's, mc_read_store_import_dev) from rs_bases on: their pointers are worked out as if they were
    // appended here, and only the bookkeeping is done.  all_ptrs: every record mc_add_superkmers*_dev is handed carries a pointer.
    // rs_hi_bases: how far the store is filled by imports (a real store; never below what rs_bases has reached).
    bool rs_virtual = false, all_ptrs = false;
    bool no_vleaf = false;  // (add_reads_partitioned: this batch's sample asked for a table beyond 2^19 regions; the first level runs again in the two-array form)
    uint64_t rs_hi_bases = 0;
    uint64_t rs_end() const { return std::max(rs_bases, rs_hi_bases); }
    mc_ctx *rs_from = nullptr;
    uint64_t cur_ptr_base = ~0ull;  // store position of base 0 of the batch being counted (~0: no pointers for it)
    uint32_t ptr_tries = 1;         // count_pipeline.h k_p3_merge: 16 while the records of other ranks (no pointers) are merged
    // The solid list P3 left in pipe.a_recs (count_pipeline.h P3Emit): valid for threshold cov_hint until anything
    // else touches the table or the pipeline buffers.
    bool solid_list_fresh = false;
    uint32_t solid_list_segs = 0;
    uint64_t solid_list_segcap = 0;

    // table
    Slot *slots = nullptr;
    size_t slots_bytes = 0;    // size of the block `slots` sits in (it may come from g_table_pool, a little larger than asked for)
    uint64_t n_regions = 0;    // regions of 2^sb slots: a power of two, or (minimizer-bin tables of >= 512 regions) any multiple of 512
    uint32_t rb = 0, sb = MC_REGION_LG;  // rb = log2(n_regions) when that is a power of two (else its floor)
    unsigned long long *d_ctr = nullptr;  // [0] n_used, [1] empty_cnt, [2] scratch counter, [3] solid n_used, [4..5] read summary, [6] keys with count >= cov_hint,
                                          // [7] parked additions, [8] the `fatal` flag (d_fatal points here), [10..13] read summary of a device batch
    unsigned long long *h_scratch = nullptr;  // 32 pinned words: where the small device-to-host copies land (a copy into pageable memory is staged)
    uint32_t *d_fatal = nullptr;
    uint64_t n_used_host = 0;
    bool finalized = false;

    // "solid" table (kmer_device.h): only the keys with count >= solid_cov, sparse.
    // Built lazily by mc_bfs_batch; the BFS never touches the counting table.
    Slot *solid = nullptr;
    uint32_t solid_lg = 0;
    int solid_cov = -1;  // -1: not built / stale
    bool solid_external = false;  // built by mc_solid_from_pairs_dev, not from this context's counting table
    bool solid_is_table = false;  // ... and does so now (solid_view)
    bool want_list = false;       // the merge kernel lists the solid keys (count_pipeline.h P3Emit): for exports, and for the copy
    int solid_external_cov = -1;
    double pending_solid_ms = 0;
    uint64_t n_solid = 0;
    // mc_set_coverage_hint: the merge kernel of the counting pipeline keeps d_ctr[6] = #keys with
    // count >= cov_hint, so ensure_solid needs no counting sweep.  Only additions that go through that
    // kernel maintain it; any other kind of addition clears solid_tracked until mc_clear.
    int cov_hint = 0;
    bool solid_tracked = true;

    mc_stats st{};
    std::vector<std::unique_ptr<BfsJobBuffers>> bfs_pool;

    char *pin[16] = {};                // pinned staging buffers of h2d_fast, made on first use
    DevPool tok_pool;                  // scratch of the device tokeniser
    int64_t extract_in_store = -1;     // mc_group: the reads the next mc_extract_*_dev call is given sit in the read store already, from this word on (consumed by that call)
    // Several GPUs: the walk of this context reads the counting tables of all ranks where they are (mc_shard_attach; mc_group
    // with peer access).  h_shards[i] describes rank i's table (this context's own among them), d_shards is the same array in
    // device memory, ipc_opened the mappings of other processes' tables this context holds.
    std::vector<ShardRef> h_shards;
    ShardRef *d_shards = nullptr;
    uint32_t shard_self = 0;
    bool shards_dropped = false;  // an attachment was dropped because the table changed: the next walk must not quietly read this rank's table alone
    int shard_owner_mm_k = 0;
    // A walker attaches the same tables step after step (bench.py: every step; the CLI: every batch of seeds): a mapping stays
    // open while its handle keeps coming (in_use: part of the current attachment) and is closed when it has not for a while.
    struct IpcMap { hipIpcMemHandle_t h; void *p; bool in_use; uint64_t addr, bytes; };  // (addr, bytes: the block in its owner's process -- a handle alone may be handed out again for another block)
    std::vector<IpcMap> ipc_opened;
    bool extract_by_minimizer = false; // mc_group: the next mc_extract_keys_dev call deals the keys to the owners of their minimizers (sk_owner), as the group's records are dealt (consumed by that call)
    uint4 *d_ovf_tmp = nullptr;        // pipe_drain_handed_on: the list moved aside while it is drained
    uint32_t *d_ovf_leaf_tmp = nullptr;
    uint64_t ovf_tmp_cap = 0, ovf_leaf_tmp_cap = 0;
    bool rs_copy_pending = false;      // a batch is on its way into the read store on pipe_stream (rs_append)
    // mc_bfs_batch: job states + seeds go up in one copy (pinned h_bfs_stage -> d_bfs_stage), results come back packed
    // (d_bfs_pack: a header block and the jobs' arrays back to back; h_bfs_hdr: the headers, pinned)
    char *h_bfs_stage = nullptr, *d_bfs_stage = nullptr, *d_bfs_pack = nullptr, *h_bfs_hdr = nullptr;
    uint64_t bfs_stage_cap = 0, bfs_pack_cap = 0, bfs_hdr_cap = 0;
    std::mutex pin_mu;                 // the pinned buffers serve one copy at a time
    hipStream_t pin_stream[8] = {};
    int mm_k = 0;        // != 0 (= k): regions are minimizer bins and reads are counted as super-k-mers (kmer_device.h)
    bool virgin = true;  // the table holds no key and its memory is not initialised yet
    bool sk_form = false;  // reads of this context can travel as super-k-mer records (set once; mm_k may be given up later)
    // scratch of the partitioned counting pipeline, kept between calls
    struct Pipe {
        uint64_t *a_keys = nullptr, *b_keys = nullptr, *spill_keys = nullptr;
        uint32_t *a_hints = nullptr, *b_hints = nullptr, *spill_hints = nullptr, *tile_first = nullptr;
        uint4 *a_recs = nullptr, *b_recs = nullptr, *spill_recs = nullptr;  // super-k-mer form (their bin words use a_hints / b_hints)
        uint64_t a_recs_cap = 0, b_recs_cap = 0, spill_recs_cap = 0;
        uint32_t *solid_cursors = nullptr;  // leaf fill levels of the solid-table build (minimizer-bin tables)
        uint64_t solid_cursors_cap = 0;
        uint32_t *emit_counts = nullptr;  // fill levels of the solid list's segments (one per P3 workgroup)
        uint32_t *cursors1 = nullptr, *seg_counts1 = nullptr, *cursors2 = nullptr, *leaf_state = nullptr, *leaf_new = nullptr, *flags = nullptr;  // cursors1: owner cursors (multi-GPU split); cursors2: leaf fill levels; flags: [0] spill lost, [1] any leaf failed, [2] a segment of the solid list overflowed
        unsigned long long *spill_count = nullptr;
        uint64_t a_cap = 0, b_cap = 0, spill_cap = 0, tiles1_cap = 0, leaves_cap = 0, segs1_cap = 0, a_hints_cap = 0, b_hints_cap = 0, cursors2_cap = 0;
        // the binned exchange (mc_extract_superkmers_binned_dev / mc_add_superkmers_binned_dev): every first-level workgroup's row of
        // (owner, fine bucket) counters; where every cell starts in the packed stream; where every listed segment of the second level starts
        uint32_t *skb_rows = nullptr;
        unsigned long long *skb_cell_start = nullptr, *skb_seg_start = nullptr, *skb_small = nullptr;  // skb_small: owner offsets / windows / part offsets / a flag
        uint64_t skb_rows_cap = 0, skb_cell_start_cap = 0, skb_seg_start_cap = 0, skb_small_cap = 0;
        void release(int dev)
        {   // (the large streams go to g_scratch_pool: ensure_buf took them from there)
            g_scratch_pool.put(dev, skb_rows, skb_rows_cap * 4); g_scratch_pool.put(dev, skb_cell_start, skb_cell_start_cap * 8);
            g_scratch_pool.put(dev, skb_seg_start, skb_seg_start_cap * 8); g_scratch_pool.put(dev, skb_small, skb_small_cap * 8);
            g_scratch_pool.put(dev, a_keys, a_cap * 8); g_scratch_pool.put(dev, b_keys, b_cap * 8); (void)hipFree(spill_keys);
            g_scratch_pool.put(dev, a_recs, a_recs_cap * sizeof(uint4)); g_scratch_pool.put(dev, b_recs, b_recs_cap * sizeof(uint4));
            (void)hipFree(spill_recs); (void)hipFree(solid_cursors); (void)hipFree(emit_counts);
            g_scratch_pool.put(dev, a_hints, a_hints_cap * 4); g_scratch_pool.put(dev, b_hints, b_hints_cap * 4); (void)hipFree(spill_hints); (void)hipFree(tile_first);
            (void)hipFree(cursors1); (void)hipFree(seg_counts1); (void)hipFree(cursors2); (void)hipFree(leaf_state); (void)hipFree(leaf_new); (void)hipFree(flags);
            // (spill_count lives behind flags, in the same allocation)
            *this = Pipe{};
        }
    } pipe;

    // Hash keys in minimizer bins: the join of the table's keys by key (dup_check.h) and what it found.
    struct Dup {
        // level 1: the merge kernel's (or the sweep's) key streams
        uint64_t *l1_keys = nullptr;
        uint64_t l1_words = 0;
        uint32_t *l1_counts = nullptr;
        uint64_t l1_counts_cap = 0;
        uint32_t l1_nseg = 0;
        uint64_t l1_cap = 0;
        bool l1_armed = false;       // the last long run's merge kernel collected into the streams (and nothing else has touched the table since)
        double expected_keys = 0;    // what the sample of the batch said the table will hold (a context without a hint)
        // levels 2 and 3
        uint64_t *l2_own = nullptr;  // where the pipeline's idle streams are too small to serve
        uint64_t l2_own_words = 0;
        uint32_t *l2_counts = nullptr;
        uint64_t l2_counts_cap = 0;
        uint32_t *flags = nullptr;            // [0] a level-1 segment overflowed, [1] a level-2 stream did
        unsigned long long *ctr = nullptr;    // [0] keys listed, [1] distinct keys in the set, [2] slots noted
        unsigned long long *list = nullptr;   // the listed keys (LIST_CAP)
        static constexpr uint64_t LIST_CAP = 1u << 16;
        // what the fix-up left: the set of keys held by more than one slot, their slots with their own counts
        DupSet set{nullptr, nullptr, nullptr, 0, nullptr};
        uint64_t set_slots = 0;
        DupTwin *tw = nullptr;
        uint64_t tw_cap = 0, n_tw = 0, n_keys = 0;
        bool merged = false;         // the noted slots hold their keys' sums now (else: their own counts)
        long long solid_delta = 0;   // what merging added to d_ctr[6] (keys at the coverage hint)
        bool checked = false;        // the table as it is has been joined
        DupL2 l2{nullptr, nullptr, 0, nullptr, 0, 0, 0, nullptr};  // the table's keys by key, as the last join left them (valid while l2_valid)
        bool l2_valid = false;
        // the check of a walk's "absent" look-ups by key (dup_check.h PhantomQ): queries, their order by sub-bucket, the hits
        unsigned long long *pq_mem = nullptr;
        uint64_t pq_cap = 0;
        uint32_t *pq_groups = nullptr;  // [G]: the first query of every sub-bucket's list
        uint64_t pq_groups_cap = 0;
    } dup;
    DupL1 dup_l1_view() const
    {
        if (!dup.l1_armed) return DupL1{nullptr, nullptr, 0, 0, nullptr};
        return DupL1{dup.l1_keys, dup.l1_counts, dup.l1_nseg, dup.l1_cap, dup.flags};
    }
    DupSet dup_filter() const { return dup.merged && dup.n_tw ? dup.set : DupSet{nullptr, nullptr, nullptr, 0, nullptr}; }

    uint64_t n_slots() const { return n_regions << sb; }
    SolidView solid_view() const
    {
        SolidView t;
        t.slots = solid;
        t.shift = 64 - solid_lg;
        t.rmask = (1u << 11) - 1;  // SOLID_REGION - 1
        t.mm_k = 0;
        t.n_regions = 0;
        if (solid_is_table) {  // the counting table itself
            t.slots = slots;
            t.shift = 64 - (rb + sb);
            t.rmask = (1u << sb) - 1;
            t.mm_k = mm_k;
            t.n_regions = (uint32_t)n_regions;
        }
        t.empty_cnt = d_ctr + 1;
        t.fatal = d_fatal;
        const mc_ctx *rs = rs_from ? rs_from : this;
        t.reads = rs->rs_end() && rs->rs_words ? rs->rs_words : nullptr;
        t.reads_bases = rs->rs_words ? rs->rs_end() : 0;
        t.shards = d_shards;
        t.n_shards = d_shards ? (uint32_t)h_shards.size() : 0u;
        t.owner_mm_k = shard_owner_mm_k;
        return t;
    }
    TableView view() const
    {
        TableView t;
        t.slots = slots;
        t.shift = 64 - (rb + sb);  // (hash-prefix regions: n_regions is a power of two)
        t.rmask = (1u << sb) - 1;
        t.n_regions = (uint32_t)n_regions;
        t.mm_k = mm_k;
        t.n_used = d_ctr;
        t.empty_cnt = d_ctr + 1;
        t.fatal = d_fatal;
        t.ovf = d_ovf;
        t.ovf_n = d_ctr + 7;
        t.ovf_cap = d_ovf ? OVF_CAP : 0;
        t.ovf_leaf = d_ovf_leaf;
        return t;
    }
    static constexpr uint64_t OVF_CAP = 1ull << 22;
    uint4 *d_ovf = nullptr;  // TableView::ovf
    uint32_t *d_ovf_leaf = nullptr;  // TableView::ovf_leaf
};

extern thread_local std::string g_create_err;  // what mc_create / mc_group_create failed of

inline int fail(mc_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_err = buf;
    return code;
}

#define HIPCHK(c, call)                                                                               \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail((c), e_ == hipErrorOutOfMemory ? MC_ENOMEM : MC_EHIP, "%s: %s (%s:%d)", #call, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                   \
    } while (0)

template <typename T>
struct DevBuf {  // RAII device buffer for temporaries
    T *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    void reset() { if (p) (void)hipFree(p); p = nullptr; }
    hipError_t alloc(size_t n) { reset(); return hipMalloc(reinterpret_cast<void **>(&p), std::max<size_t>(n, 1) * sizeof(T)); }
};

// The host form of a call: inputs go up into device buffers of its own and results come back, under the context's lock; in between
// (staged) the lock is free, for the device form takes it itself.  The first failure is kept, and everything after it is left out.
struct HostStage {
    mc_ctx *c;
    std::unique_lock<std::mutex> lock;
    std::vector<void *> bufs;
    int rc;
    explicit HostStage(mc_ctx *ctx) : c(ctx), lock(ctx->mu), rc(set_device()) {}
    HostStage(const HostStage &) = delete;
    HostStage &operator=(const HostStage &) = delete;
    ~HostStage()
    {
        if (lock.owns_lock()) lock.unlock();
        for (void *p : bufs) (void)hipFree(p);
    }
    template <typename T>
    T *out(uint64_t n)  // a device buffer of n elements
    {
        void *p = nullptr;
        if (!rc) rc = alloc(&p, std::max<uint64_t>(n, 1) * sizeof(T));
        return static_cast<T *>(p);
    }
    template <typename T>
    const T *in(const T *host, uint64_t n)  // ... holding the host's n elements; NULL for an optional input that is not given
    {
        T *p = host ? out<T>(n) : nullptr;
        if (p) rc = copy(p, host, n * sizeof(T), hipMemcpyHostToDevice);
        return p;
    }
    int staged()
    {
        lock.unlock();
        return rc;
    }
    template <typename T>
    int back(T *host, const T *dev, uint64_t n)  // after the device form: the result
    {
        if (!lock.owns_lock()) lock.lock();
        return copy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost);
    }

private:
    int set_device()
    {
        HIPCHK(c, hipSetDevice(c->cfg.device));
        return MC_OK;
    }
    int alloc(void **p, size_t bytes)
    {
        HIPCHK(c, hipMalloc(p, bytes));
        bufs.push_back(*p);
        return MC_OK;
    }
    int copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
    {
        HIPCHK(c, hipMemcpy(dst, src, bytes, kind));
        return MC_OK;
    }
};

// 64-bit words of n packed reads (32 bases a word), the pad word behind them included
inline uint64_t packed_words(const uint64_t *offsets, uint64_t n) { return (offsets[n] + 31) / 32 + 1; }

// f(the key mode as a constant: std::integral_constant<int, KEY_...>), for a kernel that is a template over it
template <typename F>
void for_key_mode(int key_mode, F &&f)
{
    if (key_mode == MC_KEY_PACKED) f(std::integral_constant<int, KEY_PACKED>());
    else if (key_mode == MC_KEY_POLY) f(std::integral_constant<int, KEY_POLY>());
    else f(std::integral_constant<int, KEY_FNV1A>());
}

// (calls that read several tables: mc_seq_coverage, mc_kmer_presence) every distinct context's mutex, taken in the order of their addresses (two calls that name the same contexts in different
// orders cannot wait for each other)
struct TablesLock {
    std::vector<mc_ctx *> distinct;
    TablesLock(mc_ctx *const *tables, uint32_t n_tables) : distinct(tables, tables + n_tables)
    {
        std::sort(distinct.begin(), distinct.end(), std::less<mc_ctx *>());
        distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
        for (mc_ctx *c : distinct) c->mu.lock();
    }
    ~TablesLock()
    {
        for (auto it = distinct.rbegin(); it != distinct.rend(); ++it) (*it)->mu.unlock();
    }
};

// a table of hash keys in minimizer bins (count_long.h): a bare key does not say which bin it is in (mcgpu.hip by_key_ready)
inline bool hash_bins(const mc_ctx *c) { return c->mm_k != 0 && c->cfg.key_mode != MC_KEY_PACKED; }

inline int grid_for(uint64_t work_items, int block, int max_blocks = 256 * 8)
{
    uint64_t g = (work_items + block - 1) / block;
    if (g < 1) g = 1;
    if (g > (uint64_t)max_blocks) g = max_blocks;
    return (int)g;
}

template <typename F>
int timed(mc_ctx *c, double *acc_ms, F &&launch)
{
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    launch();
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *acc_ms += ms;
    return MC_OK;
}

// ------------------------------------------------------------------------------------------ across units

// mcgpu.hip: the table, the key join, the counting pipeline, the read store
uint64_t regions_for(const mc_ctx *c, uint64_t slots);
int table_grow(mc_ctx *c, uint64_t new_regions);
int materialize(mc_ctx *c);
int read_counters(mc_ctx *c, unsigned long long *n_used, uint32_t *fatal);
int by_key_ready(mc_ctx *c, int why = 1);
int drain_parked(mc_ctx *c);
hipError_t dev_malloc(mc_ctx *c, void **p, size_t bytes);
bool dup_check_on();
int dup_unmerge(mc_ctx *c);
int ensure_dups(mc_ctx *c);
int rs_reserve(mc_ctx *c, uint64_t more_words);
int add_reads_dev_locked(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_off, uint64_t n_reads, uint64_t n_bases, int64_t in_store = -1);
bool h2d_pinned(mc_ctx *c, void *dst, const void *src, size_t bytes, int fd, uint64_t file_off);
int h2d_fast(mc_ctx *c, void *dst, const void *src, size_t bytes);
int ensure_solid(mc_ctx *c, int min_cov, double *ms);
int phantom_verify(mc_ctx *c, uint32_t n_jobs, std::vector<std::unique_ptr<BfsJobBuffers>> &B, const std::vector<BfsCtl> &ctl, bool *redo);

template <typename T>
int ensure_buf(mc_ctx *c, T **p, uint64_t *cap, uint64_t need)
{   // (blocks of 64 MB and more come from and go to g_scratch_pool: *cap may come out above `need`)
    if (*cap >= need && *p) return MC_OK;
    if (*p) {  // (a block that goes back to the pool may be handed out at once: what is queued on it must be done)
        (void)hipStreamSynchronize(c->stream);
        if (c->pipe_stream) (void)hipStreamSynchronize(c->pipe_stream);
        g_scratch_pool.put(c->cfg.device, *p, *cap * sizeof(T));
    }
    *p = nullptr;
    *cap = 0;
    const size_t bytes = std::max<uint64_t>(need, 1) * sizeof(T);
    size_t got = 0;
    hipError_t e = g_scratch_pool.get(c->cfg.device, bytes, reinterpret_cast<void **>(p), &got);
    if (e == hipErrorOutOfMemory) {  // (idle blocks are given back first)
        (void)hipGetLastError();
        g_table_pool.release(c->cfg.device);
        g_scratch_pool.release(c->cfg.device);
        e = g_scratch_pool.get(c->cfg.device, bytes, reinterpret_cast<void **>(p), &got);
    }
    if (e != hipSuccess) {
        size_t fr = 0, tot = 0;
        (void)hipMemGetInfo(&fr, &tot);
        *p = nullptr;
        return fail(c, e == hipErrorOutOfMemory ? MC_ENOMEM : MC_EHIP, "scratch of %.2f GB: %s (%.2f of %.2f GB free on the device)",
                    bytes / 1e9, hipGetErrorString(e), fr / 1e9, tot / 1e9);
    }
    *cap = std::max<uint64_t>(need, got / sizeof(T));
    return MC_OK;
}

// reads_file.hip: the device tokeniser
namespace mch { struct PlainReadsFile; struct PackedBatch; }
// The chunks of one file, tokenised into the read store back to back and counted together when the file ends: one run
// of the counting pipeline (which reads and rewrites the whole table) instead of one per 256 MB of text.
struct TokPending {
    PoolBuf<uint64_t> off;     // read offsets of all chunks so far (+ the end), relative to the first chunk's first base
    uint64_t off_cap = 0;
    uint64_t reads = 0, bases = 0;
    int64_t base_word = -1;    // where the first chunk starts in the read store
};
int tokenize_chunk_locked(mc_ctx *c, const mch::PlainReadsFile &f, const char *b, const char *e, uint8_t *d_text, uint64_t *n_reads_out,
                          bool *declined, TokPending *pend = nullptr);
// One mapped file through the tokeniser, chunk by chunk (host/reads_io.h plain_chunks), into the read store of c: the bytes of chunk
// i + 1 go up on a helper thread while chunk i is tokenised, the order of steps and the clean-up are written once, and the two callers
// -- mc_add_reads_file, mc_group_add_reads_file -- say what is theirs.  flush, host_batch and after_chunk run without c's lock (ctx_failed
// may run under it and takes none); each returns a code it has reported where its caller reports.
struct FileChunkOps {
    const char *who = "";                                // the function's name in front of the driver's own error texts
    std::function<int(TokPending &)> flush;              // what has gathered is counted: ahead of a declined chunk's host batches, and when the file ends
    uint64_t batch_reads = 0;                            // a declined chunk goes through the host parser in batches of so many reads ...
    std::function<int(mch::PackedBatch &)> host_batch;   // ... each handed to this
    std::function<int(size_t i, size_t n_chunks, TokPending &)> after_chunk;  // chunk i is done, its text still on the device
    std::function<int(int)> ctx_failed;                  // (optional) a failure whose text c->err holds -> the code to return (mc_group: the text goes to the group)
};
using FileCuts = std::vector<std::pair<const char *, const char *>>;  // (what plain_chunks gives)
int tokenize_file_chunks(mc_ctx *c, const mch::PlainReadsFile &f, const FileCuts &cuts, const FileChunkOps &ops, uint64_t *n_reads);
// ... and what whole_reads.hip takes from it: the scan of 32-bit counts into 64-bit offsets and the newline pass
int tok_scan(mc_ctx *c, const uint32_t *d_in, uint64_t n, unsigned long long *d_out, uint64_t *total);
struct TokNewlines {  // the newline positions and the pass's tile buffers: the caller keeps them until its own passes are done
    PoolBuf<uint32_t> tile_counts;
    PoolBuf<unsigned long long> tile_off, nl;
};
int tok_newlines(mc_ctx *c, const uint8_t *d_text, uint64_t n, TokNewlines *b, uint64_t *n_nl, bool *too_many);

// walk.hip: the walk over several ranks' tables
struct ShardWire {  // what a mc_shard_handle holds
    hipIpcMemHandle_t ipc;  // of the table's block (all zero: none could be made; the handle then only serves its own process)
    uint64_t addr, bytes;   // the table in the exporting process
    uint32_t shift, rmask, n_regions;
    int32_t mm_k;
    uint64_t empty;         // count of the key that equals EMPTY_KEY (hash modes)
    int32_t pid;
    int16_t device;
    uint8_t k, key_mode;
    uint64_t token;         // drawn once per process: ranks in separate PID namespaces can share a pid, and a foreign address must never be taken for a local one
    uint32_t magic, has_ipc;
};
static_assert(sizeof(ShardWire) == 128, "the wire format of a shard handle");
static_assert(sizeof(ShardWire) <= sizeof(mc_shard_handle), "mc_shard_handle is too small");
int shard_describe(mc_ctx *c, ShardWire *w, bool want_ipc);
void shard_detach_locked(mc_ctx *c);
int shard_attach_locked(mc_ctx *c, const ShardWire *w, uint32_t n, uint32_t self, int by_minimizer);
