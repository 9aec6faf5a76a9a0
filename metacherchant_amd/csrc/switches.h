// The library's environment switches (INTEGRATION.md lists them), read in one place.
//
// read_switches() fills an mc_switches from the environment: mc_create stores one in mc_ctx::sw, mc_group_create (group.hip) one in
// mc_group::sw (the group's own switches: MC_GROUP_*, MC_EXCHANGE_GATHER_READS).  A switch set after a context was created
// changes nothing for that context.  Two exceptions read elsewhere: the pools' switches, once per process
// (read_pool_switches: the pools outlive every context), and MC_DUP_CHECK, on every call (mcgpu.hip dup_check_on).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

struct mc_switches {
    // counting
    int count_path = 0;                       // MC_COUNT_PATH=direct|partition: 1 (atomics) | 2 (partitioned pipeline); 0 auto
    bool superkmers = true;                   // MC_SUPERKMERS=0: packed keys take the per-window pipeline (A/B measurements)
    bool long_records = true;                 // MC_LONG_RECORDS=0: polynomial keys of 33 .. 63 bases take the per-window pipeline
    int long_bins = 0;                        // MC_LONG_BINS: 0 unset (by how crowded the table is), 2 two smallest hashes, 1 any other value
    bool p3_dedup = true;                     // MC_P3_DEDUP=0: the general merge kernel instead of k_p3_dedup
    bool sk_compact = true;                   // MC_SK_COMPACT=0: super-k-mer records in the two-array form
    bool sk_vleaf = true;                     // MC_SK_VLEAF=0: no compact records before the table's size is known
    uint64_t sk_vleaf_max_regions = ~0ull;    // MC_SK_VLEAF_MAX_REGIONS: the reach of the records' leaf bits, made smaller (tests)
    double dup_l1_scale = 1.0;                // MC_DUP_L1_SCALE: the join's level-1 streams scaled (tests: streams that overflow)
    uint64_t max_run_bases = 0;               // MC_MAX_RUN_BASES: bases one pipeline run takes (0: by the form and the free memory)
    uint64_t max_run_bases_per_window = 0;    // MC_MAX_RUN_BASES_PER_WINDOW: the same for the per-window form alone (0: unset)
    bool exchange_binned = true;              // MC_EXCHANGE_BINNED=0: no binned form of the multi-GPU record exchange
    // reading files
    bool tokenizer_host = false;              // MC_TOKENIZER=host: every file through the host reader
    uint64_t tokenizer_chunk_bytes = 1ull << 28;  // MC_TOKENIZER_CHUNK_BYTES: chunks of the device tokeniser (64 B .. 1.5 GB)
    // the walk
    bool bfs_direct = true;                   // MC_BFS_DIRECT=0: the walk on a copy of the solid k-mers, not the counting table
    bool bfs_companion = true;                // MC_BFS_COMPANION=0: no scouts' kernel beside the walk's
    bool bfs_selfcheck = false;               // MC_BFS_SELFCHECK=1: every walk checked on the device
    std::string bfs_trace_dump;               // MC_BFS_TRACE_DUMP=<path>: the rounds' trace of a tuning build written there
    bool bfs_stats = false;                   // MC_BFS_STATS=1: walk statistics on stderr
    // diagnostics
    bool ingest_debug = false;                // MC_INGEST_DEBUG=1: what the counting and reading paths decided, on stderr
    bool unitigs_stats = false;               // MC_UNITIGS_STATS=1: device time of every pass of mc_unitigs on stderr, a line a call
    bool kmers_stats = false;                 // MC_KMERS_STATS=1: the stages of mc_save_kmers_gpu / mc_load_kmers_gpu on stderr, a line a call
    // the table as a file
    uint64_t kmers_chunk_records = 8ull << 20;  // MC_KMERS_CHUNK_RECORDS: records per staging chunk of mc_save_kmers_gpu / mc_load_kmers_gpu (64 at least)
    // mc_group
    bool group_gather_reads = true;           // MC_EXCHANGE_GATHER_READS=0: the other devices' records carry no pointers
    int group_transport = 0;                  // MC_GROUP_TRANSPORT=rccl|peer: 1 | 2; 0: as the config's flags say
    uint64_t group_batch_reads = 1ull << 24;  // MC_GROUP_BATCH_READS: reads per device and batch of a file (1024 at least)
    bool group_walk_gather = false;           // MC_GROUP_WALK=gather: the walk on gathered solid k-mers, not on every device's table
};

// MC_TOKENIZER_CHUNK_BYTES as it is spelt (NULL or empty: unset, mc_switches' default) -> the chunk size: for read_switches() below, for
// the CLI's WholeReadsSource (csrc/host/whole_reads_source.h: the far side of the ABI, it reads the environment itself), for `mc_hosttest cuts`
inline uint64_t tokenizer_chunk_bytes_of(const char *text)
{
    return std::min<uint64_t>(std::max<uint64_t>(text && *text ? strtoull(text, nullptr, 10) : mc_switches().tokenizer_chunk_bytes, 64), 3ull << 29);
}

inline mc_switches read_switches()
{
    auto off = [](const char *name) { const char *e = getenv(name); return e && !strcmp(e, "0"); };
    auto num = [](const char *name, uint64_t dflt) { const char *e = getenv(name); return e && *e ? strtoull(e, nullptr, 10) : dflt; };
    mc_switches s;
    if (const char *e = getenv("MC_COUNT_PATH")) s.count_path = !strcmp(e, "direct") ? 1 : !strcmp(e, "partition") ? 2 : 0;
    s.superkmers = !off("MC_SUPERKMERS");
    s.long_records = !off("MC_LONG_RECORDS");
    if (const char *e = getenv("MC_LONG_BINS")) s.long_bins = !strcmp(e, "2") ? 2 : 1;
    s.p3_dedup = !off("MC_P3_DEDUP");
    s.sk_compact = !off("MC_SK_COMPACT");
    s.sk_vleaf = !off("MC_SK_VLEAF");
    s.sk_vleaf_max_regions = num("MC_SK_VLEAF_MAX_REGIONS", ~0ull);
    if (const char *e = getenv("MC_DUP_L1_SCALE")) s.dup_l1_scale = atof(e);
    s.max_run_bases = num("MC_MAX_RUN_BASES", 0);
    if (const char *e = getenv("MC_MAX_RUN_BASES_PER_WINDOW")) if (*e) s.max_run_bases_per_window = std::max<uint64_t>(strtoull(e, nullptr, 10), 1u << 20);
    s.exchange_binned = !off("MC_EXCHANGE_BINNED");
    if (const char *e = getenv("MC_TOKENIZER")) s.tokenizer_host = !strcmp(e, "host");
    s.tokenizer_chunk_bytes = tokenizer_chunk_bytes_of(getenv("MC_TOKENIZER_CHUNK_BYTES"));
    if (const char *e = getenv("MC_BFS_DIRECT")) s.bfs_direct = strcmp(e, "0") != 0;
    s.bfs_companion = !off("MC_BFS_COMPANION");
    if (const char *e = getenv("MC_BFS_SELFCHECK")) s.bfs_selfcheck = *e && *e != '0';
    if (const char *e = getenv("MC_BFS_TRACE_DUMP")) s.bfs_trace_dump = e;
    s.bfs_stats = getenv("MC_BFS_STATS") != nullptr;
    s.ingest_debug = getenv("MC_INGEST_DEBUG") != nullptr;
    s.unitigs_stats = getenv("MC_UNITIGS_STATS") != nullptr;
    s.kmers_stats = getenv("MC_KMERS_STATS") != nullptr;
    s.kmers_chunk_records = std::max<uint64_t>(num("MC_KMERS_CHUNK_RECORDS", 8ull << 20), 64);
    s.group_gather_reads = !off("MC_EXCHANGE_GATHER_READS");
    if (const char *e = getenv("MC_GROUP_TRANSPORT")) s.group_transport = !strcmp(e, "rccl") ? 1 : !strcmp(e, "peer") ? 2 : 0;
    if (const char *e = getenv("MC_GROUP_BATCH_READS")) if (*e) s.group_batch_reads = std::max<uint64_t>(strtoull(e, nullptr, 10), 1024);
    if (const char *e = getenv("MC_GROUP_WALK")) s.group_walk_gather = !strcmp(e, "gather");
    return s;
}

// The process-wide pools of table and scratch memory (context.h TablePool, ScratchPool) read theirs once per process, when
// the library is loaded.
struct mc_pool_switches {
    bool table_pool = true;          // MC_TABLE_POOL=0: tables go back to the driver
    bool scratch_pool = true;        // MC_SCRATCH_POOL=0: pipeline scratch goes back to the driver
    size_t scratch_idle_max = (size_t)64e9;  // MC_SCRATCH_POOL_GB=<n>: idle scratch kept at most
};

inline mc_pool_switches read_pool_switches()
{
    mc_pool_switches s;
    const char *e = getenv("MC_TABLE_POOL");
    s.table_pool = !(e && !strcmp(e, "0"));
    e = getenv("MC_SCRATCH_POOL");
    s.scratch_pool = !(e && !strcmp(e, "0"));
    if ((e = getenv("MC_SCRATCH_POOL_GB"))) s.scratch_idle_max = (size_t)(atof(e) * 1e9);
    return s;
}
