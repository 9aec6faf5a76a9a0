/*
 * mcgpu.h -- C ABI of libmcgpu.so: the MI355X (gfx950) implementation of MetaCherchant's
 * environment-finder hot path (k-mer counting over the read set + coverage-thresholded
 * de Bruijn BFS from the seed sequences).
 *
 * This is the drop-in boundary.  The reference has no FFI: the seam is ordinary Java calls
 * inside one JVM, so each entry point below names the Java method whose body it replaces
 * (src/... = the reference's src/ tree, itmo!/x = ru/ifmo/genetics/x in
 * lib/itmo-assembler-src.jar).  INTEGRATION.md shows the JNI stub a maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative MC_E* code; the message is available
 *     from mc_last_error().  The library never calls exit() and no C++ exception crosses the ABI
 *     (the reference throws ExecutionFailedException, itmo!/utils/tool/Tool.java:450-462).
 *   - plain pointers and sizes only.  Functions ending in _dev take pointers to device (HBM)
 *     memory of the context's device; all others take host pointers.  Work runs on the context's own
 *     HIP stream (or the one given to mc_set_stream) and every call returns with its results complete;
 *     device buffers a caller passes in must not have writes pending on OTHER streams (a memset, a
 *     copy, a collective's result): synchronise those first, or share the stream.
 *   - a context is not re-entrant for mutation (mc_add_*, mc_finalize_counts).  After
 *     mc_finalize_counts, mc_get* and mc_bfs are read-only on the table; calls on ONE context
 *     are serialised internally, several contexts may be used from several threads.
 *
 * Data layout of reads ("2-bit packed"):
 *   base code A=0 G=1 C=2 T=3 (itmo!/dna/DnaTools.java:31 -- note: not ACGT order);
 *   base i of the concatenated read set lives in words[i >> 5], bits (63 - 2*(i & 31)) .. (62 - 2*(i & 31))
 *   (first base = most significant, itmo!/utils/KmerUtils.java:24-39);
 *   read r covers bases [read_offsets[r], read_offsets[r+1]); read_offsets has n_reads + 1 entries;
 *   words[] must hold ceil(n_bases / 32) + 1 entries (one readable pad word).
 *   Reads must be pure ACGT: the N policy of the readers (FASTA records with N dropped, FASTQ
 *   split at phred < 1, itmo!/io/readers/FastaReader.java:54-76,
 *   itmo!/io/readers/FastaReaderFromXQSourceTrunc.java:61-95) is applied by the caller
 *   (metacherchant_amd's host reader does it) before packing.
 */
#ifndef MCGPU_H
#define MCGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MC_ABI_VERSION 14

/* error codes */
#define MC_OK 0
#define MC_EINVAL (-1)    /* bad argument */
#define MC_ENOMEM (-2)    /* host or device allocation failed */
#define MC_EHIP (-3)      /* HIP runtime error (message has the HIP error string) */
#define MC_ESTATE (-4)    /* call not allowed in this state (e.g. mc_get before mc_finalize_counts) */
#define MC_EOVERFLOW (-5) /* an internal capacity was exceeded and could not be grown */
#define MC_ENOSEED (-6)   /* no seed k-mer reaches min_cov: the reference's "fail"
                             (src/algo/OneSequenceCalculator.java:193-196) */
#define MC_ECHECK (-7)    /* debugging only: MC_BFS_SELFCHECK=1 was set and a finished walk broke an invariant of
                             runBfs (no duplicate vertices, coverages as in the table, queue order, every vertex
                             has a parent); the message lists what */

/* Key modes, chosen exactly as src/tools/EnvironmentFinderMain.java:128-136,157-169:
 * k <= 31 and !forcehash -> PACKED (key = min(fw, rc) of the 2-bit packed k-mer as signed long,
 * itmo!/dna/kmers/ShortKmer.java:54-56); otherwise a 64-bit strand-symmetric hash of the k-mer
 * (src/utils/PolynomialHash.java:19-28 default, src/utils/FNV1AHash.java:33-42 with --hash fnv1a);
 * colliding k-mers share a counter, as in the reference (src/io/LargeKIOUtils.java:46-49 adds the HASH of every window to the
 * map).  That holds for every internal form of the table: where hash keys are kept in minimizer bins of the k-mers' bases
 * (mc_get below), mc_finalize_counts joins the table's keys by key (csrc/dup_check.h), gives a key that two different k-mers
 * brought to two regions the SUM of its counters wherever it is read, and counts and exports it once (mc_stats.dup_keys,
 * dup_ms).  Environment MC_DUP_CHECK=0 skips the join (measurements only: a colliding pair -- expected n^2 / 2^65 of them among n
 * keys -- then keeps two counters, "Hashtable size" counts it twice, an export lists it twice; mc_stats.dup_unchecked says so). */
enum { MC_KEY_PACKED = 0, MC_KEY_POLY = 1, MC_KEY_FNV1A = 2 };

/* mc_config.flags.  MC_FLAG_SOLID_LIST: the k-mers at or above the coverage hint will be exported (a shard of a
 * multi-GPU run, mc_export_dev): the counting pass then lists them as it goes, which saves the export a table sweep. */
#define MC_FLAG_SOLID_LIST 1
/* MC_FLAG_GROUP_RCCL (mc_group_create only): the buckets travel between the devices through RCCL -- one communicator per
 * device inside the process (ncclCommInitAll), the exchange as grouped ncclSend / ncclRecv over xGMI -- instead of
 * peer-to-peer copies; the environment variable MC_GROUP_TRANSPORT=rccl|peer says the same.  librccl is loaded on demand. */
#define MC_FLAG_GROUP_RCCL 4

typedef struct mc_ctx mc_ctx;

typedef struct {
    int32_t k;              /* 1..31 for MC_KEY_PACKED, 1..63 for the hash modes */
    int32_t key_mode;       /* MC_KEY_* */
    int32_t device;         /* HIP device ordinal */
    int32_t flags;          /* MC_FLAG_* */
    uint64_t capacity_hint; /* expected number of distinct keys; 0 = start small and grow */
} mc_config;

/* Tool lifetime: one context = one k-mer table = the BigLong2ShortHashMap created by
 * src/io/IOUtils.java:220-221 / src/io/LargeKIOUtils.java:60-61. */
int mc_create(const mc_config *cfg, mc_ctx **out);
void mc_destroy(mc_ctx *ctx);
/* ctx may be NULL: returns the message of the last failed mc_create on this thread. */
const char *mc_last_error(const mc_ctx *ctx);
int mc_abi_version(void);

/* Empties the table (keeps its allocation): a fresh BigLong2ShortHashMap without paying hipMalloc again. */
int mc_clear(mc_ctx *ctx);

/* Optional: tells the context which --coverage the BFS will use (minOccurences,
 * src/tools/EnvironmentFinderMain.java:61-65, known before the reads are loaded).  Counting then
 * keeps the number of k-mers with count >= min_cov up to date as it goes, which saves mc_bfs* one
 * sweep over the table.  Results never depend on it; 0 turns it off. */
int mc_set_coverage_hint(mc_ctx *ctx, int min_cov);

/* Read pointers.  A context keeps the packed bases of every read it counts (its "read store", until mc_clear) and each
 * table slot remembers where one occurrence of its k-mer sits in it: the BFS reads its look-ahead from there (the bases
 * that follow an occurrence are the path the walk will most likely take; every guess is looked up, so results never
 * depend on it).  mc_set_read_pointers(ctx, 0) turns both off for the reads added from then on -- for the ranks of a
 * sharded run whose reads the BFS rank cannot see.  mc_share_read_store(ctx, from): a BFS-only context built by
 * mc_solid_from_pairs_dev reads the store of `from`, the context of the same device that counted (or extracted) this
 * rank's reads and whose pointers the pairs carry; `from` must outlive the BFS calls on ctx (NULL detaches). */
int mc_set_read_pointers(mc_ctx *ctx, int mode);
int mc_share_read_store(mc_ctx *ctx, mc_ctx *from);
/* ... and for the ranks of a sharded run whose reads the BFS rank CAN see, because they are brought to it: with pointers from the
 * walking rank's reads alone -- one read in eight at 8 GPUs -- the walk of 8 x configs[1] took 146 ms instead of 7.9 (its look-ahead
 * had a 3.75-fold read set to follow).  mc_set_read_pointers' mode: 0 no pointers; 1 this context's own store (the default); 2 a
 * store kept by another context: this one keeps nothing, but works out the pointers of the reads it extracts or counts as if
 * they were appended to a store at mc_read_store_tell() -- the caller copies the words there (mc_read_store_import_dev on the
 * context that keeps the store, at that position).  | MC_PTRS_ON_EVERY_RECORD: every record this context will be handed by
 * mc_add_superkmers*_dev / mc_add_keys_dev carries a pointer (the merge kernel need not wait for a later copy that has one).
 *   mc_read_store_seek    the next reads go (mode 1) or are deemed to go (mode 2) to position at_bases, a multiple of 32: ranks
 *                         that share one store take disjoint stretches of it; reserve_bases (mode 1): room up to there
 *   mc_read_store_tell    where the next reads will go
 *   mc_read_store_import_dev  n_words packed words (32 bases each, as in mc_add_reads_packed_dev, with their pad word) of another
 *                         rank's reads to position at_bases of this context's store */
#define MC_PTRS_ON_EVERY_RECORD 0x10
int mc_read_store_seek(mc_ctx *ctx, uint64_t at_bases, uint64_t reserve_bases);
uint64_t mc_read_store_tell(mc_ctx *ctx);
int mc_read_store_import_dev(mc_ctx *ctx, const uint64_t *d_words, uint64_t n_words, uint64_t at_bases);

/* Use the caller's HIP stream (a hipStream_t passed as void*) for all work of this context
 * instead of the context's own stream.  NULL restores the own stream. */
int mc_set_stream(mc_ctx *ctx, void *hip_stream);

/* ---- counting: replaces ReadsLoadWorker.process (src/io/IOUtils.java:201-214,
 * src/io/LargeKIOUtils.java:41-54): for every window of every read, addAndBound(key, 1).
 * May be called repeatedly (one call per batch / file); the result does not depend on call or
 * read order.  Reads shorter than k contribute nothing. */
int mc_add_reads_packed(mc_ctx *ctx, const uint64_t *words, const uint64_t *read_offsets, uint64_t n_reads);
int mc_add_reads_packed_dev(mc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_read_offsets,
                            uint64_t n_reads, uint64_t n_bases);

/* One input file of --reads: ReadsWorker.run / ReadersUtils.readDnaLazyTrunc (src/io/ReadsWorker.java:29-41,
 * itmo!/io/ReadersUtils.java:27-53,104-121): format by extension (.fasta .fa .fn .fna / .fastq .fq, optionally
 * .gz or .bz2; .binq), FASTA records with N dropped whole, FASTQ and BINQ reads split where phred < 1 (quality
 * offset sniffed on the first 1000 records); every read (piece) is counted as by mc_add_reads_packed.  *n_reads (may be NULL) = reads
 * added ("N reads added").  Errors carry the reference's messages ("Can't detect file format for file ...").
 * Uncompressed FASTA / FASTQ text is tokenised on the device (csrc/tokenizer.h: the bytes cross the link in 256 MB
 * chunks, each tokenised and counted while the next one is copied); what the device declines, and every compressed
 * or .binq file, is parsed by the host (environment: MC_TOKENIZER=host parses every file on the host). */
int mc_add_reads_file(mc_ctx *ctx, const char *path, uint64_t *n_reads);

/* End of loadReads (src/io/IOUtils.java:217-248): waits for all queued counting work;
 * *n_distinct = hm.size() ("Hashtable size: N kmers", src/tools/EnvironmentFinderMain.java:137). */
int mc_finalize_counts(mc_ctx *ctx, uint64_t *n_distinct);

/* BigLong2ShortHashMap.get (itmo!/structures/map/BigLong2ShortHashMap.java:74-77 ->
 * Long2ShortHashMap.java:160-175): out[i] = count saturated at 32767
 * (itmo!/utils/NumUtils.java:21-26), or -1 when the key is absent.  Key 0 is legal.
 * A context with polynomial-hash keys of 33 .. 63 bases keeps its table in minimizer bins of the k-mers' BASES while reads
 * are counted into a table whose size something vouches for -- a capacity_hint that still holds, or, for the first batch into
 * an empty table, a sample of that batch -- (csrc/count_long.h), where a bare key does not say which region it lives in: mc_get
 * then answers all n queries with ONE sweep of the table (cost: the table's size, not n), and the first key stream
 * (mc_add_keys_dev, mc_add_pairs_dev, mc_load_kmers), mc_shard_export or batch that takes the direct kernel moves every key to
 * hash-prefix regions first, once and for good (a rebuild of the table: mc_stats.grows counts it), after which reads take the
 * per-window pipeline.  Results are the same either way: mc_finalize_counts has merged the counters of colliding k-mers (above). */
int mc_get(mc_ctx *ctx, const int64_t *keys, uint64_t n, int16_t *out);
int mc_get_dev(mc_ctx *ctx, const int64_t *d_keys, uint64_t n, int16_t *d_out);

/* getKmerKey (src/algo/OneSequenceCalculator.java:89-96) for packed oriented k-mers:
 * k-mer i is the 2k-bit number (hi[i] << 64 | lo[i]), first base most significant
 * (hi may be NULL when k <= 32).  Host pointers. */
int mc_kmer_keys(mc_ctx *ctx, const uint64_t *hi, const uint64_t *lo, uint64_t n, int64_t *out_keys);

/* ---- BFS: replaces OneSequenceCalculator.runBfs up to (not including) runTrimPaths
 * (src/algo/OneSequenceCalculator.java:154-214) with TerminationMode.allowsAddition
 * (src/algo/TerminationMode.java:31-47).
 *
 * Seeds are the k-windows of the seed sequences in file order (then Hi-C seeds when merging),
 * as oriented packed k-mers; the library looks their coverage up and queues those with
 * count >= min_cov (:159-192).  dir: -1 left neighbours, +1 right, 0 all eight interleaved
 * L(A) R(A) L(G) R(G) L(C) R(C) L(T) R(T) (src/utils/StringUtils.java:8-32).
 * max_kmers / max_radius: < 0 = unset (at least one must be set, EnvironmentFinderMain.java:171-175).
 *
 * The result lists the entries of distanceToKmer in insertion order (= BFS discovery order, seeds
 * first, duplicates once): the oriented k-mer, its distance, reads.get(key) and whether the vertex
 * is in lastKmers (needed by runTrimPaths, :241-262, which the host applies, or mc_trim_paths below).  Arrays are
 * malloc()ed by the library; release with mc_bfs_result_free. */
typedef struct {
    uint64_t n;
    uint64_t *hi, *lo; /* oriented k-mers (hi all zero when k <= 32) */
    int32_t *dist;
    int16_t *cov;
    uint8_t *last;
    uint64_t levels;     /* largest distance assigned */
    uint64_t lookups;    /* table lookups issued (speculative ones included) */
    uint64_t rounds;     /* memory round trips on the critical path (speculation rounds + wide chunks) */
    double device_ms;    /* device time of the BFS kernels of the whole batch, HIP events */
} mc_bfs_result;

int mc_bfs(mc_ctx *ctx, const uint64_t *seed_hi, const uint64_t *seed_lo, uint64_t n_seeds, int dir,
           int min_cov, int64_t max_kmers, int64_t max_radius, mc_bfs_result *out);
void mc_bfs_result_free(mc_bfs_result *r);

/* Several independent BFS passes in ONE launch, one workgroup each: the two passes of
 * buildEnvironment with --bothdirs False (runBfs(-1); runBfs(+1), OneSequenceCalculator.java:137-144)
 * and the one-calculator-per-seed-sequence thread pool of EnvironmentFinderMain.java:218-225.
 * out[] has n_jobs entries; a job whose seeds all fail the threshold returns out[j].n == 0
 * (mc_bfs returns MC_ENOSEED for that). */
typedef struct {
    const uint64_t *seed_hi; /* may be NULL when k <= 32 */
    const uint64_t *seed_lo;
    uint64_t n_seeds;
    int32_t dir;
} mc_bfs_job;
int mc_bfs_batch(mc_ctx *ctx, const mc_bfs_job *jobs, uint32_t n_jobs, int min_cov, int64_t max_kmers,
                 int64_t max_radius, mc_bfs_result *out);

/* ---- table export / import: (key, count) pairs with count >= min_cov, unordered.
 * Also the record content of the reference's .kmers.bin (src/io/KmersLoadWorker.java:9,20-23)
 * and the payload of the multi-GPU gather.  With keys == NULL only *n_out is computed. */
int mc_export(mc_ctx *ctx, int min_cov, int64_t *keys, int16_t *counts, uint64_t cap, uint64_t *n_out);
/* d_hints (may be NULL): the 32-bit read pointer stored with each key -- where one of its occurrences sits in the
 * read store of the context that extracted it, used only to steer the BFS's look-ahead (never part of a result);
 * carry it along with the pairs so that a table rebuilt elsewhere walks as fast as the one that counted the reads
 * (mc_share_read_store). */
int mc_export_dev(mc_ctx *ctx, int min_cov, int64_t *d_keys, int16_t *d_counts, uint32_t *d_hints, uint64_t cap,
                  uint64_t *n_out);
/* table[key] = min(32767, table[key] + count) for each pair (saturating adds commute). */
int mc_add_pairs_dev(mc_ctx *ctx, const int64_t *d_keys, const int16_t *d_counts, const uint32_t *d_hints, uint64_t n);
/* The BFS side of the multi-GPU gather: turns an empty (new or cleared) context into a BFS-only one whose graph
 * is the given pairs with count >= min_cov -- the concatenated mc_export_dev output of every rank, owners being
 * disjoint so no key comes twice; entries with a smaller (or negative: padding) count are skipped.  The pairs go
 * straight into the BFS's own table; the counting table stays empty, so mc_get / mc_export on this context see
 * nothing and mc_bfs* accepts this min_cov only, until mc_clear.  *n_solid (may be NULL) = vertices kept.
 * What the reference does instead: the BFS reads the one shared map (src/algo/OneSequenceCalculator.java:203-204). */
int mc_solid_from_pairs_dev(mc_ctx *ctx, const int64_t *d_keys, const int16_t *d_counts, const uint32_t *d_hints, uint64_t n,
                            int min_cov, uint64_t *n_solid);

/* ---- multi-GPU building blocks (device pointers).  The read set is split across ranks; each
 * rank turns its reads into keys bucketed by owner rank, ranks exchange buckets (RCCL
 * all-to-all, done by the caller), and each rank counts the keys it owns. */
/* owner of a key among n_owners ranks; pure function, same on every rank */
uint32_t mc_key_owner(int64_t key, uint32_t n_owners);
/* Writes the keys of all windows grouped by owner into d_keys (capacity = total windows):
 * owner o's keys are d_keys[owner_offsets[o] .. owner_offsets[o+1]); owner_offsets (host,
 * n_owners + 1 entries) is filled on return.  d_hints (may be NULL, same capacity) receives the
 * speculation hint of every occurrence at the same index.  With d_keys == NULL only the offsets are
 * computed.  n_owners <= 512. */
int mc_extract_keys_dev(mc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_read_offsets, uint64_t n_reads,
                        uint64_t n_bases, uint32_t n_owners, int64_t *d_keys, uint32_t *d_hints, uint64_t keys_cap,
                        uint64_t *owner_offsets);
/* addAndBound(key, 1) for each key; d_hints may be NULL */
int mc_add_keys_dev(mc_ctx *ctx, const int64_t *d_keys, const uint32_t *d_hints, uint64_t n);

/* The same split in the compact form the counting pipeline uses itself when keys are packed k-mers
 * of at least 23 bases: one 16-byte "super-k-mer" record per run of up to 16 consecutive windows of a
 * read that share their minimizer (two uint64 per record; layout in csrc/count_pipeline.h) plus one
 * 32-bit word per record (d_bins: the read pointer of the record's first window, 0 when the context keeps no read
 * store) -- about a seventh of the bytes of the key form.  All windows of a record have the same owner.
 *   mc_superkmer_capacity   records to provide room for, given the windows and reads of a batch;
 *                           0 when this context does not use the form (then use the key form above)
 *   mc_extract_superkmers_dev  as mc_extract_keys_dev; MC_EOVERFLOW when the reads yield more records
 *                           than mc_superkmer_capacity allows for (fall back to the key form)
 *   mc_add_superkmers_dev   addAndBound(key, 1) for every window of every record */
uint64_t mc_superkmer_capacity(mc_ctx *ctx, uint64_t n_windows, uint64_t n_reads);
int mc_extract_superkmers_dev(mc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_read_offsets, uint64_t n_reads,
                              uint64_t n_bases, uint32_t n_owners, uint64_t *d_records, uint32_t *d_bins,
                              uint64_t records_cap, uint64_t *owner_offsets);
int mc_add_superkmers_dev(mc_ctx *ctx, const uint64_t *d_records, const uint32_t *d_bins, uint64_t n);
/* The binned form of the same exchange: the sender also does the first level of the OWNER's counting run, so that the owner's run
 * starts at its second level (the owner's pass that dealt flat received records to its level-1 buckets was 4.5 of the 14.4 ms a
 * rank of 8 x configs[1] counted for; the sender's packing pass does the ordering instead).  Owner o's records
 * d_records[owner_offsets[o] .. owner_offsets[o + 1]) come in the order of n_fine "fine buckets" of the records' bin words;
 * d_fine_counts (device, n_owners x n_fine, written here) says how many records every (owner, fine bucket) cell holds, and
 * owner_windows (host, n_owners) how many k-mer windows every owner's records hold.  What travels to owner o: its records, its
 * pointers (if any) and its row of n_fine counts.
 *   mc_superkmer_fine_buckets  the n_fine to extract with for n_owners owners whose tables are laid out like this context's (the
 *                           level-1 buckets of its counting run: a function of the table's size); 0: no binned form here
 *                           (tables without a second level, more than 16384 / n_owners buckets, MC_EXCHANGE_BINNED=0) -- use the flat form
 *   mc_add_superkmers_binned_dev  what an owner received: n records in n_parts parts lying back to back (part p = records
 *                           part_offsets[p] .. part_offsets[p + 1], part_offsets on the host, n_parts + 1 entries; a part is what one
 *                           rank sent of one chunk), part p in the order of its d_part_counts[p * n_fine ..] (device) fine buckets;
 *                           n_windows = the windows of all records (the senders' owner_windows, summed).  Same result as
 *                           mc_add_superkmers_dev on the same records; counts that do not add up to a part's length are MC_EINVAL.
 *                           Where this context's level-1 buckets are not unions of the fine buckets (its table grew to another
 *                           bucket count), or the parts are more than 1024 x np1 / n_fine, the records are counted as a flat stream. */
uint32_t mc_superkmer_fine_buckets(mc_ctx *ctx, uint32_t n_owners);
int mc_extract_superkmers_binned_dev(mc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_read_offsets, uint64_t n_reads,
                                     uint64_t n_bases, uint32_t n_owners, uint32_t n_fine, uint64_t *d_records, uint32_t *d_bins,
                                     uint64_t records_cap, uint32_t *d_fine_counts, uint64_t *owner_offsets, uint64_t *owner_windows);
int mc_add_superkmers_binned_dev(mc_ctx *ctx, const uint64_t *d_records, const uint32_t *d_bins, uint64_t n, uint64_t n_windows,
                                 uint32_t n_fine, uint32_t n_parts, const uint64_t *part_offsets, const uint32_t *d_part_counts);

/* ---- the walk over several ranks' tables where they are.  After the exchange every rank's counting table holds the k-mers it
 * owns; instead of gathering the ones at or above --coverage into a second table on the rank that walks (mc_export_dev ->
 * mc_solid_from_pairs_dev: at configs[3]'s size that copy does not fit beside the rank's own table), the walking context
 * is given every rank's table and looks a k-mer up in its owner's, through peer access (contexts of one process) or an
 * IPC mapping (one process per GPU).  What the reference does: P threads read the one shared map,
 * src/algo/OneSequenceCalculator.java:203-204.
 *   mc_shard_export  after mc_finalize_counts: an opaque, fixed-size description of this context's table (geometry, an IPC
 *                    handle of its memory) to be sent to the walking rank by any means (an all-gather of 128 bytes).  The
 *                    table must stay as it is -- no counting, no mc_clear, no mc_destroy -- until the walker has detached.
 *   mc_shard_attach  on the walking context (which has counted its own share and keeps the read store the walk reads its
 *                    look-ahead from): shards[i] = rank i's handle, shards[self] its own.  by_minimizer != 0: the exchange
 *                    dealt super-k-mer records (mc_extract_superkmers_dev), so a k-mer is owned by the owner of its
 *                    minimizer; 0: it dealt keys (mc_key_owner).  From here on mc_bfs / mc_bfs_batch on this context walk the
 *                    union of the tables, any --coverage; results equal a single context's.  mc_get / mc_export still see
 *                    this context's own shard only.
 *                    An attachment names every table's block and geometry AS THEY WERE: any call that changes this context's
 *                    counts afterwards (mc_add_*, which may also move the table) drops it, and mc_bfs then fails with
 *                    MC_ESTATE until the tables are exported and attached again (or mc_shard_detach says one table is meant).
 *   mc_shard_detach  gives the mappings up (mc_clear and mc_destroy do so too). */
typedef struct { unsigned char bytes[128]; } mc_shard_handle;
int mc_shard_export(mc_ctx *ctx, mc_shard_handle *out);
int mc_shard_attach(mc_ctx *ctx, const mc_shard_handle *shards, uint32_t n_shards, uint32_t self, int by_minimizer);
int mc_shard_detach(mc_ctx *ctx);

/* ---- several GPUs of one node as ONE table, for a host that is one process (the native `metacherchant --devices 0,1,...`).
 * A context per device and one host thread per device; reads are dealt to the devices in equal contiguous shares, every
 * device buckets its share by owner (mc_extract_superkmers_dev / mc_extract_keys_dev), the buckets travel as peer-to-peer
 * copies over xGMI -- every (source, destination) pair at once -- and every device counts what it owns
 * (mc_add_superkmers_dev / mc_add_keys_dev); the walk runs on the first device and reads every device's table in place
 * (mc_shard_attach; without peer access between all devices, or with MC_GROUP_WALK=gather, the k-mers at or above the
 * threshold are gathered on the first device instead: mc_export_dev -> mc_solid_from_pairs_dev).  Results equal a single context's.
 * `cfg->device` is ignored; capacity_hint is the whole job's.  A device may be named more than once (shares of one GPU).
 * Replaces the same Java as the single-context calls: the P threads over one shared map of src/io/IOUtils.java:283-315 and
 * the work list of src/io/ReadsDispatcher.java:34-53.  ctx may be NULL in mc_group_last_error after a failed create. */
typedef struct mc_group mc_group;
int mc_group_create(const mc_config *cfg, const int32_t *devices, uint32_t n_devices, mc_group **out);
void mc_group_destroy(mc_group *g);
const char *mc_group_last_error(const mc_group *g);
int mc_group_set_coverage_hint(mc_group *g, int min_cov);
int mc_group_add_reads_packed(mc_group *g, const uint64_t *words, const uint64_t *read_offsets, uint64_t n_reads);
int mc_group_add_reads_file(mc_group *g, const char *path, uint64_t *n_reads);
int mc_group_finalize_counts(mc_group *g, uint64_t *n_distinct);
int mc_group_bfs_batch(mc_group *g, const mc_bfs_job *jobs, uint32_t n_jobs, int min_cov, int64_t max_kmers,
                       int64_t max_radius, mc_bfs_result *out);

/* ---- the table as a file: `kmer-counter`'s <name>.kmers.bin and <name>.stat.txt (src/tools/KmersCounter.java:87-121).
 * mc_save_kmers = IOUtils.printKmers (src/io/IOUtils.java:39-65): one 10-byte record per key with count >
 * threshold -- big-endian int64 key, big-endian int16 count (saturated) -- in table order (the reference's order
 * is its map's iteration order; nothing reads it), and the frequency histogram of ALL keys
 * ("# k-mer frequency<TAB>number of such k-mers", ascending, a blank line at the end); stat_path may be NULL.
 * Call after mc_finalize_counts.  *n_total = keys in the table, *n_written = records written.
 * mc_load_kmers = IOUtils.loadKmers (:94-126, src/io/KmersLoadWorker.java:9-23): addAndBound(key, count) for
 * every record with count > freq_threshold; *n_records = records read, *n_added = records added. */
int mc_save_kmers(mc_ctx *ctx, const char *bin_path, const char *stat_path, int threshold, uint64_t *n_total,
                  uint64_t *n_written);
int mc_load_kmers(mc_ctx *ctx, const char *path, int freq_threshold, uint64_t *n_records, uint64_t *n_added);

/* ... and the same on the device (csrc/kmers_bin.hip; src/io/IOUtils.java:39-65,94-126, src/io/KmersLoadWorker.java:9-23).
 * mc_kmers_encode_dev: the records of printKmers in device memory.  Call after mc_finalize_counts (else MC_ESTATE).  A key of the table
 * is what mc_export lists at min_cov 0; its value is its count saturated at 32767; d_hist (32768 bins, zeroed by the call; may be
 * NULL) takes the histogram of ALL keys; a key with value > threshold becomes a record.  Records come in ascending order of their
 * table slots, the key equal to the free-slot mark (hash modes; counted out of band) last: the bytes are a function of the table, two
 * calls give the same ones.  *n_total = keys, *n_written = records.  d_bytes == NULL only counts (and fills d_hist).  d_bytes must be
 * 16-byte aligned and hold 10 * n_written bytes: a smaller cap_bytes is MC_EINVAL (the message names both numbers, the counts are
 * still returned) and nothing is stored.
 * mc_kmers_decode_dev: KmersLoadWorker's filter on the device: of the n_records records at d_bytes (16-byte aligned) those with
 * count > freq_threshold (a signed compare: count bytes 80 00 are -32768) go to d_keys (8-byte aligned) / d_counts (4-byte aligned),
 * n_records entries each, in any order; *n_kept = how many.  The table is not touched: mc_add_pairs_dev takes the result.
 * mc_save_kmers_gpu / mc_load_kmers_gpu: mc_save_kmers / mc_load_kmers with these kernels, their contract, files and messages.  The
 * save sweeps the table once for the counts, then encodes chunks of whole table tiles -- at most MC_KMERS_CHUNK_RECORDS records, 2048 at
 * least -- into two staging buffers in turn; each is copied into pinned memory and written by a writer thread while the next one is
 * encoded, so the extra memory is two chunks on either side, whatever the table's size.  The file has the records in slot order.  The
 * load checks the file's length first (nothing is added from a file that is no whole number of records), then a reader thread
 * brings chunk i + 1 to the device while chunk i is decoded and added.  (environment: MC_KMERS_CHUNK_RECORDS, default 8 Mi, 64 at least.) */
int mc_kmers_encode_dev(mc_ctx *ctx, int threshold, uint8_t *d_bytes, uint64_t cap_bytes, uint64_t *d_hist, uint64_t *n_total,
                        uint64_t *n_written);
int mc_kmers_decode_dev(mc_ctx *ctx, const uint8_t *d_bytes, uint64_t n_records, int freq_threshold, int64_t *d_keys, int16_t *d_counts,
                        uint64_t *n_kept);
int mc_save_kmers_gpu(mc_ctx *ctx, const char *bin_path, const char *stat_path, int threshold, uint64_t *n_total, uint64_t *n_written);
int mc_load_kmers_gpu(mc_ctx *ctx, const char *path, int freq_threshold, uint64_t *n_records, uint64_t *n_added);

/* ---- reads-classifier: per-read k-mer coverage of a second read set in this table (src/tools/ReadsClassifier.java:154-200,
 * src/algo/PairFinder.java:32-57, src/algo/ReadsFinderInGraph.java:37-161).
 * Reads come in the packed layout above, but whole: the caller turns N / n / . into base code 0 (A) -- what
 * itmo!/dna/DnaQBuilder.java:45 does -- and does not split them.  For every read of length L >= k, with
 * cov[i] = getWithZero(key of window i) (the count saturated at 32767, 0 when absent; ReadsFinderInGraph.java:63-88):
 *   sum = sum of cov[i] (a Java int: it wraps), covered = #{i : cov[i] > 0}, last = cov[L - k];
 *   found = findRead (:37-49,95-103): !(width < found_pct / 100.0) && (width == 1 || (width != 0 && |width - theory| <= std))
 *           with cov_mean = (sum + last (k - 1)) / L, width = (covered + [last > 0] (k - 1)) / L, theory = 1 - e^-cov_mean,
 *           std = z sqrt(e^-cov_mean (1 - e^-cov_mean) / L), all in double.
 * A read shorter than k is not found and its numbers are 0.
 * flags & MC_CLASSIFY_CORRECTION: findReadWithCorrection (:121-161).  d_bad_pos[r] is the only position of read r whose phred is
 * below 10, -1 when there is none, -2 when there are several (d_bad_pos may be NULL: no read has one).  A read with exactly one
 * such position p is found when one of the four reads with base p set to 0..3 passes findRead with the threshold 0.9 -- a
 * constant in the reference, whatever found_pct says; only the <= k windows that cover p are looked up again.  sum / covered /
 * last stay those of the read as given.
 * The table is read as mc_get reads it: call after mc_finalize_counts.  A table of hash keys still in minimizer bins (mc_get
 * above) is moved to hash-prefix regions first, once and for good (the cost of one table rebuild); nothing is ever swept per call.
 * Errors: MC_ESTATE before mc_finalize_counts; MC_EINVAL for null pointers or found_pct outside 0 .. 100.
 * mc_classify_reads takes host pointers (words: ceil(n_bases / 32) + 1 entries as above), mc_classify_reads_dev device ones. */
typedef struct {
    int32_t sum;     /* sum of the windows' coverages (int32 wrap-around, as the reference's int) */
    int32_t covered; /* windows with coverage > 0 */
    int16_t last;    /* coverage of the last window */
    uint8_t found;   /* the verdict (with the correction when asked for) */
    uint8_t pad;
} mc_read_cov;
#define MC_CLASSIFY_CORRECTION 1
int mc_classify_reads_dev(mc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_read_offsets, uint64_t n_reads,
                          const int32_t *d_bad_pos, int found_pct, double z, int flags, mc_read_cov *d_out);
int mc_classify_reads(mc_ctx *ctx, const uint64_t *words, const uint64_t *read_offsets, uint64_t n_reads,
                      const int32_t *bad_pos, int found_pct, double z, int flags, mc_read_cov *out);

/* ---- triple-reads-classifier: found / half-found / not found with two k (src/tools/TripleReadsClassifier.java:164-270,
 * src/algo/TripleFinder.java:32-67, src/algo/TripleFinder2.java:45-110).
 * The reference keeps pass 1's class of a read in a map keyed by the read's bases (read.toString(): N printed as A, no qualities;
 * one map a mate) and looks every read up by its bases in pass 2: a read's pass-1 class is that of the LAST read of its side with
 * the same bases.  It runs pairs on a thread pool, so "last" is only defined at -p 1; here it is the greatest input index.
 *
 * mc_reads_last_copy: for every read r, last[r] = the greatest index j of a read with exactly the same bases (same length, same
 * codes); j >= r.  Reads in the layout of mc_classify_reads (N is code 0: exactly the reference's key).  Needs no table (any
 * context, before or after mc_finalize_counts).  A 64-bit fingerprint a read, a stable radix sort of (fingerprint, index), then
 * every read is compared base for base with the last member of its run of equal fingerprints: the result never rests on a
 * fingerprint alone.  flags & MC_LAST_COPY_WEAK_FP (tests only): the first round keeps 4 bits of the fingerprint, so distinct reads
 * share one and the collision path runs.  Errors: MC_EINVAL for null pointers or n_reads >= 2^31 (one sort).
 * mc_reads_last_copy takes host pointers, mc_reads_last_copy_dev device ones. */
#define MC_LAST_COPY_WEAK_FP 1
int mc_reads_last_copy_dev(mc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_read_offsets, uint64_t n_reads,
                           int flags, uint32_t *d_last);
int mc_reads_last_copy(mc_ctx *ctx, const uint64_t *words, const uint64_t *read_offsets, uint64_t n_reads,
                       int flags, uint32_t *last);

/* mc_triple_classes: the classes of n_pairs pairs at this context's k, one byte a read, from the two mates' mc_read_cov (what
 * mc_classify_reads gave at this k, with or without the correction) and their lengths (offsets1 / offsets2: n_pairs + 1 each).
 * found_i = cov_i.found, except found_2 = !found_1 when mate 2 is empty (TripleFinder.java:44-46);
 * width = (covered + [last > 0] (k - 1)) / len, 0 when len < k (getWidth, :70-76: the read as given, without the correction);
 * half = half_pct / 100.0.
 *   Pass 1 (prev1 == prev2 == NULL): FOUND if found, else HALF_FOUND if width >= half, else NOT_FOUND (TripleFinder.java:48-61).
 *   Pass 2 (prev_s: pass 1's classes of side s, last_s: mc_reads_last_copy of side s): c1 = prev_s[last_s[i]];
 *     FOUND if found && c1 == FOUND, else HALF_FOUND if found || c1 == FOUND || (width >= half && c1 == HALF_FOUND), else NOT_FOUND
 *     (TripleFinder2.java:58-76).
 * Needs no table.  Errors: MC_EINVAL for null pointers, half_pct outside 0 .. 100, or only some of the pass-2 arrays. */
#define MC_CLASS_NOT_FOUND 0
#define MC_CLASS_HALF_FOUND 1
#define MC_CLASS_FOUND 2
int mc_triple_classes_dev(mc_ctx *ctx, const mc_read_cov *d_cov1, const mc_read_cov *d_cov2, const uint64_t *d_offsets1,
                          const uint64_t *d_offsets2, uint64_t n_pairs, int half_pct, const uint8_t *d_prev1, const uint8_t *d_prev2,
                          const uint32_t *d_last1, const uint32_t *d_last2, uint8_t *d_class1, uint8_t *d_class2);
int mc_triple_classes(mc_ctx *ctx, const mc_read_cov *cov1, const mc_read_cov *cov2, const uint64_t *offsets1, const uint64_t *offsets2,
                      uint64_t n_pairs, int half_pct, const uint8_t *prev1, const uint8_t *prev2, const uint32_t *last1,
                      const uint32_t *last2, uint8_t *class1, uint8_t *class2);

/* ---- seq-cov: depth and breadth of every sequence's k-mers in up to four tables at once (src/tools/SequenceCoverage.java:162-185).
 * Sequences come in the layout of mc_classify_reads (whole, N as code 0, the pad word); they may be reads, genes or contigs of any
 * length: the work is cut by base positions, not by sequences.  For sequence s of length L and table t, with
 * cov[i] = getWithZero(key of window i) as mc_classify_reads defines it (the saturated count, 0 when absent; the contexts' key mode):
 *   out[s * n_tables + t].depth = sum of cov[i] (64 bits: it does not wrap), .breadth = #{i : cov[i] > 0}, over i = 0 .. L - k;
 * both 0 when L < k.  (No "last window" extension: that is findRead's.)  A window is keyed once and looked up in all n_tables tables.
 * tables: n_tables contexts (1 .. MC_SEQ_COV_MAX_TABLES) with the same k, key mode and device, each after mc_finalize_counts; the
 * same context may be named more than once.  A table of hash keys still in minimizer bins is moved to hash-prefix regions first, as
 * mc_classify_reads does.  The kernel runs on tables[0]'s stream, and messages go to tables[0]'s last error.
 * Errors: MC_EINVAL for null pointers, n_tables of 0 or above MC_SEQ_COV_MAX_TABLES, or contexts that differ in k, key mode or
 * device; MC_ESTATE when a context is not finalized.  n_seqs == 0 is MC_OK after these checks.  out is not written on an error.
 * mc_seq_coverage takes host pointers (words: ceil(n_bases / 32) + 1 entries), mc_seq_coverage_dev device ones (d_out: n_seqs *
 * n_tables entries, zeroed by the call). */
typedef struct {
    uint64_t depth;   /* sum of the windows' coverages */
    uint64_t breadth; /* windows with coverage > 0 */
} mc_seq_cov;
#define MC_SEQ_COV_MAX_TABLES 4
int mc_seq_coverage_dev(mc_ctx *const *tables, uint32_t n_tables, const uint64_t *d_words, const uint64_t *d_seq_offsets,
                        uint64_t n_seqs, mc_seq_cov *d_out);
int mc_seq_coverage(mc_ctx *const *tables, uint32_t n_tables, const uint64_t *words, const uint64_t *seq_offsets, uint64_t n_seqs,
                    mc_seq_cov *out);

/* ---- presence: which of up to four tables hold each of n k-mers (BigLong2ShortHashMap.contains, as the recipient-visualiser asks
 * it of its four class tables for every k-mer of an environment, src/tools/RecipientVisualiser.java:157-169).
 * K-mers come as oriented packed k-mers in the layout of mc_bfs_result and mc_kmer_keys (hi may be NULL when k <= 32).
 * mask[i] bit t is set exactly when tables[t] contains the key of k-mer i -- where mc_get would not answer -1; the key is the
 * contexts' own (getKmerKey: the canonical packed k-mer, or the polynomial / FNV-1a hash, colliding hash keys sharing a counter as
 * everywhere else), so a k-mer and its reverse complement get the same mask; key 0 (poly-A) is legal.  The k-mer is keyed once
 * and looked up in all n_tables tables, in one launch.
 * tables: n_tables contexts (1 .. MC_PRESENCE_MAX_TABLES) with the same k, key mode and device, each after mc_finalize_counts; the
 * same context may be named more than once.  A table of hash keys still in minimizer bins is moved to hash-prefix regions first, as
 * mc_classify_reads does.  The kernel runs on tables[0]'s stream, and messages go to tables[0]'s last error.
 * Errors: MC_EINVAL for null pointers, n_tables of 0 or above MC_PRESENCE_MAX_TABLES, or contexts that differ in k, key mode or
 * device; MC_ESTATE when a context is not finalized.  n == 0 is MC_OK after these checks.  mask is not written on an error.
 * mc_kmer_presence takes host pointers, mc_kmer_presence_dev device ones. */
#define MC_PRESENCE_MAX_TABLES 4
int mc_kmer_presence_dev(mc_ctx *const *tables, uint32_t n_tables, const uint64_t *d_hi, const uint64_t *d_lo, uint64_t n,
                         uint8_t *d_mask);
int mc_kmer_presence(mc_ctx *const *tables, uint32_t n_tables, const uint64_t *hi, const uint64_t *lo, uint64_t n, uint8_t *mask);

/* ---- reads in a set: how many windows of every read are k-mers of a small exact set, and which reads that keeps -- the
 * environment-assembler-finder's filter of the reads by an environment (src/algo/ReadsFilter.java:47-68; membership is
 * subgraph.containsKey(normalizeDna(kmer)), src/algo/OneSequenceCalculator.java:150-152: a test on the k-mer's bases, not on its
 * table key, so hash keys and their collisions play no part here).
 * Reads come in the layout of mc_classify_reads (whole, N as code 0, the pad word).  The set is n_set oriented packed k-mers in the
 * layout of mc_bfs_result and mc_kmer_presence (hi may be NULL when k <= 32, and is not read then), in any orientation, duplicates
 * allowed: the call canonicalises them, a k-mer and its reverse complement are one member.  k is the context's; its key mode and its
 * table play no part (any context, before or after mc_finalize_counts).  For read r of length L:
 *   hits[r] = #{i in 0 .. L - k - 1 : window i is a member} -- the reference's loop is `i < len - k`: the last window is never
 *             tested; there is no early exit in hits;
 *   keep[r] = hits[r] >= max(1, (L - k + 1) * pct / 100), in Java's int arithmetic (the division truncates).
 * A read with L <= k has no tested window: hits 0, keep 0.  pct = 100 therefore keeps no read at all.
 * The set becomes an open-addressing table of canonical k-mers in device memory (one word a slot for k <= 32, two above, at most
 * half full) and a bit filter that every workgroup holds in LDS; a window that the filter passes is compared with the table's
 * k-mer in full, so the result never rests on the filter.  flags & MC_READS_IN_SET_WEAK_FILTER (tests only): no filter, every
 * window goes to the table (as it does for sets of more than 2^19 k-mers).
 * Errors: MC_EINVAL for null pointers (hi at k <= 32 excepted), pct outside 0 .. 100, or n_set >= 2^31.  n_reads == 0 is MC_OK;
 * n_set == 0 is MC_OK with every output 0.  Outputs are not written on an error.
 * mc_reads_in_set takes host pointers, mc_reads_in_set_dev device ones (d_hits: 4 bytes a read, d_keep: one). */
#define MC_READS_IN_SET_WEAK_FILTER 1
int mc_reads_in_set_dev(mc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_read_offsets, uint64_t n_reads,
                        const uint64_t *d_set_hi, const uint64_t *d_set_lo, uint64_t n_set, int pct, int flags,
                        uint32_t *d_hits, uint8_t *d_keep);
int mc_reads_in_set(mc_ctx *ctx, const uint64_t *words, const uint64_t *read_offsets, uint64_t n_reads,
                    const uint64_t *set_hi, const uint64_t *set_lo, uint64_t n_set, int pct, int flags,
                    uint32_t *hits, uint8_t *keep);

/* ---- components: which k-mers of the table hang together -- what the fmt-visualizer's walks reach (src/tools/FMTVisualizer.java:
 * 113-139 starts src/algo/KmerEnvCalculator.java's runBfs at every window whose count is still above 0; the walk has no visited set
 * but zeroes every k-mer it pops, so it reaches exactly the connected component of its first k-mer, and the scan's seeds are the
 * first windows of the components in scan order).
 * Sequences come in the layout of mc_classify_reads (whole, N as code 0, the pad word).
 *   vertex     a key of the table with get > 0 that at least one window of the sequences holds (a counted k-mer that no window
 *              of the sequences holds is in no component);
 *   edge       between the keys of two k-mers that are StringUtils.allNeighbors of each other;
 *   numbering  components by the scan position (sequence, then offset) of their first window: the reference's comp<N>;
 *   members    of component c: entries comp_offsets[c] .. comp_offsets[c + 1] - 1 of hi / lo / cov.  Member 0 is the seed window's
 *              k-mer in the read's orientation; the order of the others is unspecified (it may differ from call to call).
 * The table is only read (a table of hash keys still in minimizer bins is moved to hash-prefix regions first, as mc_classify_reads
 * does; every mc_get answer stays what it was).
 * Work: one sweep of the windows (first[slot] = the smallest scan position of a window that holds the slot's key), one sweep of the
 * table with eight look-ups a claimed slot and a lock-free union-find over slot numbers (32-bit parents below 2^32 slots), two
 * more sweeps to list the members; the roots are sorted on the host.  12 or 16 bytes of device memory a table slot while it runs.
 * Limit, hash keys only: the k-mer of a key's first window explores for the key.  The reference's walk also steps onto a string
 * that was never read but whose hash is a key, and goes on from THAT string's neighbours.  Results equal the reference's exactly when
 * no two distinct canonical k-mers among the members and their neighbours share a key; for packed keys (k <= 31) always.
 * Errors: MC_EINVAL for null pointers, MC_ESTATE before mc_finalize_counts; n_seqs == 0 (or no bases) is MC_OK with an empty
 * result (comp_offsets = {0}).  *out is zeroed on an error.  Free a result with mc_components_free (NULL and zeroed results are
 * fine).  mc_components takes host pointers, mc_components_dev device ones; the result is on the host in both. */
typedef struct {
    uint64_t n_components, n_kmers;
    uint64_t *comp_offsets;        /* n_components + 1: members of component c are [comp_offsets[c], comp_offsets[c+1]) */
    uint64_t *seed_seq, *seed_pos; /* per component: sequence index and base offset of its first window in scan order */
    uint64_t *hi, *lo;             /* per member: one oriented k-mer that holds the key (hi all zero when k <= 32) */
    int16_t  *cov;                 /* per member: what mc_get answers for its key */
    double device_ms;              /* summed device time of the passes (HIP events) */
} mc_components_result;  /* (not mc_components: C has one name space for typedefs and functions) */
int mc_components_dev(mc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_seq_offsets, uint64_t n_seqs, mc_components_result *out);
int mc_components(mc_ctx *ctx, const uint64_t *words, const uint64_t *seq_offsets, uint64_t n_seqs, mc_components_result *out);
void mc_components_free(mc_components_result *r);

/* ---- unitigs: the state that the reference's unitig compaction ends in (initializeStructures + doMerge of
 * src/algo/OneSequenceCalculator.java:387-451, SeqEnvCalculator and KmerEnvCalculator alike), from link analysis.
 * Input: n oriented packed k-mers in the layout of mc_kmer_presence (hi may be NULL when k <= 32) in the subgraph's iteration order,
 * and a merge class for each (the caller folds colour and is_gene into it).  Entry e makes node 2e (the k-mer as given) and node
 * 2e + 1 (its reverse complement).  k is the context's; its key mode and its table play no part.
 *   neighbours(p)  the nodes whose (k-1)-prefix is the (k-1)-suffix of node p ^ 1, ascending: deg[p] of them (at most 5: four
 *                  successor strings, of which one may be a palindrome that both its nodes spell), in nbr one list after another;
 *   link p -- q    neighbours(p) = {q}, neighbours(q) = {p}, and the classes of their entries are equal: what doMerge merges.  A node
 *                  has at most one, so links tie entries into chains, open or closed;
 *   irregular      a closed chain, or one with a link where q == p (a hairpin) or q == p ^ 1 (a self-loop).  (An entry that is its own
 *                  reverse complement has no link: both its nodes spell it, so whatever it follows has two neighbours.)  Only there
 *                  does the loop's result depend on its scan order: the entries of such chains are listed in `irregular`,
 *                  ascending, and left to the caller;
 *   unitig         a regular chain of m >= 2 entries, oriented nodes a_1 -> ... -> a_m spelling S (m + k - 1 bases).  The loop leaves
 *                  a_1 alive with label S and rc = a_m ^ 1, a_m ^ 1 alive with label rc(S) and rc = a_1, every other node of the chain
 *                  deleted, no neighbours list changed.  A chain is listed once, read from that end where first < last_rc, by
 *                  ascending first; bases holds S from base_offsets[u] on, packed as reads are, every unitig starting a new word.
 * Nodes of entries that are in no unitig and not irregular stay as they are.  The result is a function of the input alone.
 * Errors: MC_EINVAL for null pointers (hi at k <= 32 excepted), n >= 2^30, or two entries that are the same k-mer or each other's
 * reverse complement.  n == 0 is MC_OK with an empty result (base_offsets = {0}).  *out is zeroed on an error.  Free a result with
 * mc_unitigs_free (NULL and zeroed results are fine).  mc_unitigs takes host pointers, mc_unitigs_dev device ones; the result is on
 * the host in both. */
typedef struct {
    uint64_t n_nodes;                 /* 2 * n */
    uint8_t  *deg;                    /* per node: length of its neighbours list */
    uint32_t *nbr;                    /* the lists one after another in node order, each ascending */
    uint64_t n_unitigs;               /* regular chains of >= 2 entries, by ascending `first` */
    uint32_t *first, *last_rc;        /* a_1 and a_m ^ 1 */
    uint64_t *base_offsets;           /* n_unitigs + 1, in bases, each a multiple of 32 */
    uint64_t *bases;                  /* S of every unitig, packed as reads are (A0 G1 C2 T3, first base most significant) */
    uint64_t n_irregular;
    uint32_t *irregular;              /* entries of irregular chains, ascending; untouched by the call */
    double device_ms;                 /* summed device time of the passes (HIP events) */
} mc_unitigs_result;  /* (not mc_unitigs: C has one name space for typedefs and functions) */
int mc_unitigs_dev(mc_ctx *ctx, const uint64_t *d_hi, const uint64_t *d_lo, const uint8_t *d_cls, uint64_t n, mc_unitigs_result *out);
int mc_unitigs(mc_ctx *ctx, const uint64_t *hi, const uint64_t *lo, const uint8_t *cls, uint64_t n, mc_unitigs_result *out);
void mc_unitigs_free(mc_unitigs_result *r);

/* ---- the trim: which entries of one BFS pass runTrimPaths keeps (src/algo/OneSequenceCalculator.java:241-262: the walk from every
 * lastKmers vertex through getNeighborsByDir(-dir) inside distanceToKmer, and retainAll of what it visited).  k is the context's; its
 * key mode and its table play no part, and the call is allowed before mc_finalize_counts.
 * Input: the result of one pass as mc_bfs_result holds it: n distinct oriented packed k-mers (hi may be NULL when k <= 32; bits above
 * the k-mer are dropped), last[i] (0, or anything else for 1), and the pass's dir in -1, 0, +1.
 * Neighbours are StringUtils', on oriented strings with no canonical form: the left neighbour of x with base c is
 * (c << 2(k-1)) | (x >> 2), the right one ((x << 2) & mask) | c.  x and its reverse complement are two unrelated entries.
 * Output: kept[i] = 1 iff the walk visits entry i, 0 otherwise.  That is:
 *   dir = +1   i reaches a `last` entry through right-neighbour steps inside the set (no step is a way too: a `last` entry is kept);
 *   dir = -1   the same through left-neighbour steps;
 *   dir =  0   through any of the eight neighbours: i's connected component holds a `last` entry.
 * With no `last` entry nothing is kept.  The result is a set, a function of the input alone.  The order-dependent half of the trim,
 * retainAll's removals from the replayed HashMap, stays with the caller (csrc/host/envfinder.cpp Environment::add_pass takes the mask).
 * Errors: MC_EINVAL for null pointers (hi at k <= 32 and device_ms excepted), dir outside -1..1, n >= 2^31, or two entries that are the
 * same oriented k-mer (distanceToKmer is a map).  n == 0 is MC_OK.  *device_ms (may be NULL): the device time of the call, HIP events.
 * mc_trim_paths takes host pointers, mc_trim_paths_dev device ones, kept included. */
int mc_trim_paths(mc_ctx *ctx, const uint64_t *hi, const uint64_t *lo, const uint8_t *last, uint64_t n, int dir, uint8_t *kept,
                  double *device_ms);
int mc_trim_paths_dev(mc_ctx *ctx, const uint64_t *d_hi, const uint64_t *d_lo, const uint8_t *d_last, uint64_t n, int dir,
                      uint8_t *d_kept, double *device_ms);

/* ---- the walk order: what the fmt-visualizer's subgraph takes from KmerEnvCalculator.runBfs (src/algo/KmerEnvCalculator.java:60-76),
 * for every component of one mc_components result at once.  k is the context's; its key mode and its table play no part, and the call
 * is allowed before mc_finalize_counts.
 * Input: mc_components_result's hi / lo / comp_offsets as they are: n = comp_offsets[n_components] oriented packed k-mers (hi may be
 * NULL when k <= 32; bits above the k-mer are dropped), component c's members comp_offsets[c] .. comp_offsets[c + 1] - 1, the first of
 * them its seed in the read's orientation.  A component is walked against its own members only.
 * The rule: the queue starts as [seed]; popping x appends, for the eight allNeighbors of x (A, G, C, T, the left neighbour before the
 * right one), every y whose canonical form is a member that has not been popped yet (x itself counts as not yet popped), then puts
 * (canonical(x), count) and zeroes the count.  The queue has no visited set, so its length is not bounded by n; the call keeps at most
 * two entries a member, which gives the same first pops in the same order and the same answer to "popped again" (DESIGN.md 3.18).
 * Output: reached[c] members of component c are popped (all of them when the slice is connected); order[comp_offsets[c] + i],
 * i < reached[c], is the member (relative to the slice) that is popped for the first time as the i-th, member 0 first, the places
 * behind them are 0; twice[m] = 1 iff member m is popped more than once, so that its put value ends as 0.  levels, queue_entries
 * (of the bounded queue) and wide_levels (levels that took the grid-wide kernels) are summed over the components; device_ms is the
 * device time of the call (HIP events).  The result is a function of the input alone, whatever the flags.
 * Errors: MC_EINVAL for null pointers (hi at k <= 32 excepted), unknown flags, n >= 2^30 (decided before hi and lo are read),
 * comp_offsets that does not start at 0 or does not ascend strictly, or two members anywhere in the call that are the same k-mer or each
 * other's reverse complement.  n_components == 0 is MC_OK with a zeroed result.  *out is zeroed on an error.  Free a result with
 * mc_walk_order_free (NULL and zeroed results are allowed).  Device memory: at most 66 bytes a member, 90 once a level takes the wide path.
 * mc_walk_order takes host pointers, mc_walk_order_dev device ones; the result's arrays are the library's host memory in both. */
#define MC_WALK_ORDER_WIDE_ONLY 1u   /* tests only: every level by the grid-wide kernels */
#define MC_WALK_ORDER_NARROW_8  2u   /* tests only: W = 8, so small inputs cross between the two paths many times */
typedef struct {
    uint64_t n_components, n_kmers;
    uint64_t *reached;   /* per component: members the walk pops */
    uint32_t *order;     /* per component slice: the first reached[c] entries are member numbers (relative to the slice) in first-pop order */
    uint8_t *twice;      /* per member: 1 iff popped more than once */
    uint64_t levels, queue_entries, wide_levels;
    double device_ms;
} mc_walk_order_result;
int mc_walk_order(mc_ctx *ctx, const uint64_t *hi, const uint64_t *lo, const uint64_t *comp_offsets, uint64_t n_components, uint32_t flags,
                  mc_walk_order_result *out);
int mc_walk_order_dev(mc_ctx *ctx, const uint64_t *d_hi, const uint64_t *d_lo, const uint64_t *d_comp_offsets, uint64_t n_components,
                      uint32_t flags, mc_walk_order_result *out);
void mc_walk_order_free(mc_walk_order_result *r);

/* ---- the environment join: what environment-finder-multi takes from several graph.txt files at once (initializeStructures of
 * src/algo/MultiSequenceCalculator.java:51-100, the KC column of src/io/writers/GFAWriterMulti.java, printProbability of
 * src/tools/EnvironmentFinderMultiMain.java:104-170).  k is the context's; its key mode and its table play no part.
 * Input:
 *   entries  n oriented packed k-mers in the layout of mc_kmer_presence (hi may be NULL when k <= 32).  No two may be the same k-mer or
 *            each other's reverse complement;
 *   records  the lines of n_graphs graph files (1 to 64) one graph after another: an oriented k-mer as the file spells it (rec_hi may
 *            be NULL when k <= 32) and its depth; graph g's records are graph_offsets[g] .. graph_offsets[g + 1] - 1 (graph_offsets[0]
 *            is 0; a graph may be empty).  Every record's k-mer or its reverse complement must be an entry, and a graph must not hold
 *            the same oriented k-mer twice (it may hold a k-mer and its reverse complement as two records);
 *   the gene gene_len bases packed as reads are (A0 G1 C2 T3, first base most significant, 32 a word; NULL when gene_len is 0).  A gene
 *            shorter than k has no window.
 * Output, per entry e:
 *   member[e]   bit g is set when graph g holds the entry's k-mer in either orientation (MultiNode.addGraph);
 *   is_gene[e]  1 when a window of the gene is the entry's k-mer or its reverse complement;
 *   kc[e]       the sum over g of the depth of graph g's record that is the entry's k-mer as given.  A record of the reverse
 *               complement adds nothing (GFAWriterMulti looks up the normalised window only).
 * Output, three n_graphs x n_graphs matrices (row i, column j at i * n_graphs + j) of sums modulo 2^32 over every oriented k-mer x that
 * some record spells, where H is the set of graphs holding x (in that orientation) and d_g their depths as unsigned words:
 *   i in H, j in H       diff and diff_alt += |d_i - d_j|, uni += max(d_i, d_j)   (i == j: uni += d_i)
 *   i in H, j not in H   diff, diff_alt and uni += d_i
 *   i not in H, j in H   diff and uni += d_j
 * -- printProbability's three sums for the pair (i, j).
 * Errors: MC_EINVAL for null pointers (hi and rec_hi at k <= 32 excepted), n_graphs == 0 or > 64, n >= 2^30, graph_offsets that
 * decrease, and the three conditions above.  n == 0 without records is MC_OK with empty arrays and zero matrices.  *out is zeroed on an
 * error.  Free a result with mc_env_join_free (NULL and zeroed results are fine).  mc_env_join takes host pointers, mc_env_join_dev
 * device ones; the result is on the host in both. */
typedef struct {
    uint64_t n;                       /* entries */
    uint32_t n_graphs;
    uint64_t *member;                 /* n */
    uint8_t  *is_gene;                /* n */
    int64_t  *kc;                     /* n */
    uint32_t *diff, *diff_alt, *uni;  /* n_graphs * n_graphs each */
    double device_ms;                 /* summed device time of the passes (HIP events) */
} mc_env_join_result;  /* (not mc_env_join: C has one name space for typedefs and functions) */
int mc_env_join_dev(mc_ctx *ctx, const uint64_t *d_hi, const uint64_t *d_lo, uint64_t n, const uint64_t *d_rec_hi, const uint64_t *d_rec_lo,
                    const int32_t *d_rec_depth, const uint64_t *d_graph_offsets, uint32_t n_graphs, const uint64_t *d_gene, uint64_t gene_len,
                    mc_env_join_result *out);
int mc_env_join(mc_ctx *ctx, const uint64_t *hi, const uint64_t *lo, uint64_t n, const uint64_t *rec_hi, const uint64_t *rec_lo,
                const int32_t *rec_depth, const uint64_t *graph_offsets, uint32_t n_graphs, const uint64_t *gene, uint64_t gene_len,
                mc_env_join_result *out);
void mc_env_join_free(mc_env_join_result *r);

/* ---- whole reads with their qualities, tokenised on the device: what the classifying tools read their -r files with, ready for
 * mc_classify_reads_dev, mc_reads_last_copy_dev, mc_seq_coverage_dev, mc_reads_in_set_dev and mc_components_dev.  The policy is that
 * of readDnaQLazy (itmo!/io/ReadersUtils.java:185-215) -- reads are neither split nor dropped, unlike mc_add_reads_file's:
 *   FASTQ (itmo!/io/readers/FastqReader.java:53-82): records of four lines, `@...`, bases, `+...`, qualities; one trailing '\r' comes
 *          off every line.  N, n and . give base 0 with phred 0 (itmo!/dna/DnaQBuilder.java:45 unsafeAppendUnknown), any other base its
 *          code (A0 G1 C2 T3, either case) and phred (quality char - phred_offset) & 63 (DnaQ.phredAt reads 6 bits).  A read of length 0
 *          is a read.  phred_offset is 33 or 64 and the caller's to find (ReadersUtils.java:63-77 determineQualityFormat: 64 unless, in
 *          the first 1000 records, a base that is not N n . has a quality char below 64 or above 126);
 *   FASTA (FastaWithNsReader.readNextDataLine): a line that starts with '>' or ';' ends the record before it, the other lines are
 *          concatenated, text in front of the first header is a record, empty records give nothing; phred 20
 *          (ReadersUtils.DEFAULT_PHRED_FOR_FASTA) and 0 at N n .
 * text holds n_bytes of a file, a whole number of records (host memory; mc_tokenize_whole_dev: device memory of at least
 * mc_whole_text_bytes(n_bytes) bytes, whose bytes behind the text are overwritten, and last_byte = text[n_bytes - 1]).  Any context
 * will do: its table plays no part, as with mc_reads_last_copy.  The result is device memory throughout:
 *   d_words    the bases packed as mc_classify_reads_dev takes them, ceil(n_bases / 32) + 1 words, unknown bases as base 0;
 *   d_offsets  n_reads + 1 base positions in d_words, d_offsets[0] == 0;
 *   d_bad_pos  per read mc_classify_reads' bad_pos: the one position with phred < 10, -1 for none, -2 for several
 *              (src/algo/PairFinder.java findReadWithCorrection).  An N counts, in FASTA as well;
 *   d_codes, d_phred  with MC_WHOLE_CODES / MC_WHOLE_PHRED in flags: a byte a base, the code and the phred (what a DnaQ holds); else NULL.
 * declined = 1 (and all else zero, nothing allocated): the text holds something whose outcome the host reader defines -- a byte that is
 * no base and not N n ., a quality char outside [phred_offset, 126], bases and qualities of different length, a line count that is
 * no multiple of four, a record whose first line does not start with '@' or whose third does not start with '+', a read of 2^31 - 16
 * bases or more.  Read that text with the host parser, which gives the reference's message or its laxer reading.
 * Two calls on the same text give the same bytes.  n_bytes == 0 gives no reads (d_offsets holds the one 0).
 * Errors: MC_EINVAL for null pointers, a format or phred_offset that is none of the above, unknown flags.  *out is zeroed on an error.
 * mc_whole_reads_to_host copies the arrays of a result to host memory: every pointer that is not NULL is filled, sized as above.
 * Free a result with mc_whole_reads_free (NULL and zeroed results are fine). */
#define MC_WHOLE_FASTA 0
#define MC_WHOLE_FASTQ 1
#define MC_WHOLE_CODES 1u  /* flags: also a byte a base with the code */
#define MC_WHOLE_PHRED 2u  /* flags: also a byte a base with the phred */
typedef struct {
    int declined;
    uint64_t n_reads, n_bases;
    uint64_t *d_words;
    uint64_t *d_offsets;
    int32_t  *d_bad_pos;
    uint8_t  *d_codes, *d_phred;
    double device_ms;  /* from the first pass to the last on the context's stream (HIP events; the scans' totals are waited for in between) */
} mc_whole_reads;
int mc_tokenize_whole(mc_ctx *ctx, const char *text, uint64_t n_bytes, int format, int phred_offset, uint32_t flags, mc_whole_reads *out);
int mc_tokenize_whole_dev(mc_ctx *ctx, uint8_t *d_text, uint64_t n_bytes, int last_byte, int format, int phred_offset, uint32_t flags,
                          mc_whole_reads *out);
uint64_t mc_whole_text_bytes(uint64_t n_bytes);
int mc_whole_reads_to_host(mc_ctx *ctx, const mc_whole_reads *r, uint64_t *words, uint64_t *offsets, int32_t *bad_pos, uint8_t *codes, uint8_t *phred);
void mc_whole_reads_free(mc_ctx *ctx, mc_whole_reads *r);
/* Joins device views of packed reads into one: the n_reads reads of d_words / d_offsets (n_reads + 1 base positions in d_words; the
 * first need not be 0, so a slice of a mc_whole_reads result will do; d_words has its pad word) go behind the dst_bases bases that
 * d_dst_words already holds, shifted into place.  d_dst_words needs ceil((dst_bases + the new bases) / 32) + 1 words; when dst_bases
 * is no multiple of 32, the word the old reads end in must be zero behind them (it is after an earlier call; zero the first word
 * before the first).  The pad word behind the result is zeroed.  d_dst_offsets points at the destination's entry for the first new
 * read: entries 0 .. n_reads are written, entry 0 being dst_bases.  For the calls that want all reads in one array
 * (mc_reads_last_copy_dev over all pairs, mc_components_dev) when the reads come a chunk at a time.  Any context will do. */
int mc_reads_append_dev(mc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_offsets, uint64_t n_reads, uint64_t *d_dst_words,
                        uint64_t dst_bases, uint64_t *d_dst_offsets);

/* ---- the classifiers' FASTQ records as text, rendered on the device (csrc/render_fastq.hip): the body of
 * WritersUtils.writeDnaQsToFastqFile (itmo!/io/writers/FastqDedicatedWriter.java:39-60 with Illumina.getPhredChar), which
 * ReadsClassifier.java:186-199 and TripleReadsClassifier.java:243-262 call once per output file.
 * A record is "@<n>\n<bases>\n+\n<quals>\n": <n> in decimal, counting from 1 per file; a base is "AGCT"[code] (an N is base 0 and
 * prints as A); a quality is phred + 64.  It has 2 len + digits(n) + 6 bytes.
 * Input: n_sides (1 or 2) sides of n_reads reads each (mate 1, mate 2).  A side's words are packed as mc_classify_reads_dev takes them,
 * phred holds a byte a base at the same base positions, offsets n_reads + 1 base positions (the first need not be 0: a slice of a
 * mc_whole_reads result will do), stream a byte a read: the output stream of the read (below n_streams <= MC_RENDER_MAX_STREAMS), or
 * MC_RENDER_SKIP for none.  Inside a stream the records come in item order, item = n_sides * read + side: read 0 side 0, read 0 side 1,
 * read 1 side 0, ... -- so one stream may take records of both sides.  first_number (host memory, n_streams entries): the first record
 * of stream t in this call is @first_number[t], the next one more, so a file continues over calls; MC_RENDER_UNNUMBERED makes the
 * stream's records start at the '\n' behind the number (2 len + 5 bytes), for lists whose numbers the caller knows later.
 * Output: d_text (16-byte aligned, `capacity` bytes) holds the streams one after another: stream t is out->bytes[t] bytes from
 * out->start[t] on, a multiple of 16, and out->records[t] records.  Bytes between the streams and behind the last are not written.
 * mc_render_fastq_bound(n_bases, n_items) is a capacity that always suffices (2 n_bases + 26 n_items + 256, rounded up to 16; host
 * only); a smaller capacity than the call needs is MC_EOVERFLOW, decided before anything is written to d_text.  No byte at or behind
 * `capacity` is written, whatever the inputs hold.  Two calls on the same input give the same bytes.
 * Data errors are the reference's: the call returns MC_OK with out->error set, the text is then unspecified.  MC_RENDER_EMPTY: a
 * selected read of length 0 ("Empty DnaQ!"); MC_RENDER_QUALITY: a phred above 62 (getPhredChar's "Invalid quality code byte"),
 * out->error_value the byte.  error_side / error_read name the offending item with the lowest item index (and its first such base).
 * Errors: MC_EINVAL for null pointers, n_sides not 1 or 2, n_streams 0 or above MC_RENDER_MAX_STREAMS, n_sides * n_reads >= 2^40,
 * d_text not 16-byte aligned, and a stream byte that is neither below n_streams nor MC_RENDER_SKIP (found on the device: out->error is
 * MC_RENDER_STREAM, error_side / error_read / error_value say where and what).  n_reads == 0 is MC_OK with no bytes.
 * mc_render_fastq takes host pointers and gives the text in host memory, mc_render_fastq_dev device ones (first_number and out are
 * host memory in both).  Any context will do: its table plays no part. */
#define MC_RENDER_MAX_STREAMS 16
#define MC_RENDER_SKIP 0xFF
#define MC_RENDER_UNNUMBERED (~0ull)
#define MC_RENDER_EMPTY 1
#define MC_RENDER_QUALITY 2
#define MC_RENDER_STREAM 3
typedef struct {
    const uint64_t *words;
    const uint8_t *phred;
    const uint64_t *offsets;
    const uint8_t *stream;
} mc_render_side;
typedef struct {
    uint64_t start[MC_RENDER_MAX_STREAMS], bytes[MC_RENDER_MAX_STREAMS], records[MC_RENDER_MAX_STREAMS];
    int32_t error;        /* 0, or MC_RENDER_EMPTY / MC_RENDER_QUALITY / MC_RENDER_STREAM */
    uint32_t error_side;
    uint64_t error_read;
    uint32_t error_value;
    double device_ms;     /* from the first pass to the last on the context's stream (HIP events; the scans' totals are waited for in between) */
} mc_render_result;
int mc_render_fastq_dev(mc_ctx *ctx, const mc_render_side *sides, uint32_t n_sides, uint64_t n_reads, uint32_t n_streams,
                        const uint64_t *first_number, uint8_t *d_text, uint64_t capacity, mc_render_result *out);
int mc_render_fastq(mc_ctx *ctx, const mc_render_side *sides, uint32_t n_sides, uint64_t n_reads, uint32_t n_streams,
                    const uint64_t *first_number, uint8_t *text, uint64_t capacity, mc_render_result *out);
uint64_t mc_render_fastq_bound(uint64_t n_bases, uint64_t n_items);

/* ---- measurement */
typedef struct {
    uint64_t windows;       /* k-mer occurrences counted so far */
    uint64_t count_launches; /* counting passes: launches of the direct kernel, or runs of the partitioned pipeline */
    double count_ms;         /* their summed device time (HIP events on the context's stream) */
    double count_total_ms;   /* device time of all counting-phase kernels */
    uint64_t table_slots;    /* current table capacity (slots) */
    uint64_t table_bytes;
    uint64_t grows;          /* number of table rebuilds */
    double p1_ms, p2_ms, p3_ms; /* partitioned pipeline: extract+scatter / scatter / merge kernels */
    uint64_t spill_keys;     /* keys that did not fit their bucket and took the direct kernel */
    uint64_t solid_kmers;    /* k-mers with count >= min_cov found by the last BFS set-up */
    uint64_t solid_sweeps;   /* table sweeps BFS set-ups needed to count them (0 with mc_set_coverage_hint) */
    uint64_t solid_list_builds; /* BFS set-ups and exports that took their entries from the list the merge kernel left, without sweeping the table */
    uint64_t long_runs;      /* pipeline runs that took long records (polynomial keys, k > 32, a capacity hint: csrc/count_long.h) */
    uint64_t dup_keys;       /* hash keys in minimizer bins: keys that different k-mers brought to more than one region, as the last
                                mc_finalize_counts found them (their counters are merged; 0 once the table has moved to hash-prefix regions) */
    uint64_t dup_checks;     /* joins of the table's keys by key that found that out (csrc/dup_check.h), ... */
    double dup_ms;           /* ... and their summed device time */
    uint64_t dup_unchecked;  /* 1: MC_DUP_CHECK=0 skipped the join for the table as it is now */
    uint64_t left_bins;      /* hash keys of 33 .. 63 bases: 0 while the table is in minimizer bins (reads travel as long records), else why
                                it moved to hash-prefix regions for good (reads take one record a window from then on, ~3 x the counting
                                time): 1 something came or asked by key (mc_add_keys_dev, mc_add_pairs_dev, mc_load_kmers, mc_shard_export,
                                a copy of the solid k-mers), 2 a batch of under 2^22 windows took the direct kernel, 3 nothing vouched for
                                the table's size when a batch came (no capacity_hint that still holds, and the table not empty), 4 bins
                                overflowed or the table had to grow, 5 more keys in several regions than the join's lists take */
    uint64_t binned_runs;    /* mc_add_superkmers_binned_dev calls whose run started at the second level (the others counted a flat stream) */
} mc_stats;
int mc_get_stats(mc_ctx *ctx, mc_stats *out);
int mc_reset_stats(mc_ctx *ctx);
/* Gives the counting pipeline's scratch (the record / key streams of the last run: about 1.3 bytes per base counted) and
 * the idle blocks of the process-wide pools back to the driver -- and, on a context that counted hash keys as long records, the
 * key streams of mc_finalize_counts' join (8 bytes a key, twice: 84 GB for configs[2]'s 4.58 G keys; a walk's check of its
 * look-ups by key then sweeps the table instead) --; the table, the read store and the list of solid k-mers
 * stay.  For callers that need the device's memory between counting and what follows (the next counting call allocates
 * its scratch again).  No counterpart in the reference: the JVM's collector does this for BigLong2ShortHashMap's
 * transient arrays (itmo!/structures/map/BigLong2ShortHashMap.java:46-70). */
int mc_trim(mc_ctx *ctx);
/* ... of a group: counts and bytes summed over its devices, times the largest of any device (they work side by side) */
int mc_group_get_stats(mc_group *g, mc_stats *out);

/* ---- synthetic workload of SURVEY.md section 8(d) (spec: DESIGN.md "Synthetic workload"),
 * generated straight into HBM so that benchmarks start with the reads resident.
 * Reads r = first_read .. first_read + n_reads - 1 of fixed length read_len drawn from
 * n_contigs contigs of contig_len bases; err_per_10k = substitution rate in 1/10000.
 * d_words needs ceil(n_reads*read_len/32) + 1 words, d_read_offsets n_reads + 1. */
int mc_synth_reads_dev(mc_ctx *ctx, uint64_t genome_seed, uint64_t n_contigs, uint64_t contig_len,
                       uint64_t read_seed, uint64_t first_read, uint64_t n_reads, uint32_t read_len,
                       uint32_t err_per_10k, uint64_t *d_words, uint64_t *d_read_offsets);
/* bases [start, start + n) of the synthetic genome as codes 0..3 (host buffer) */
int mc_synth_genome(uint64_t genome_seed, uint64_t start, uint64_t n, uint8_t *codes);

#ifdef __cplusplus
}
#endif
#endif /* MCGPU_H */
