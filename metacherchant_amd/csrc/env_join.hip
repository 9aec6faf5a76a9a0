// libmcgpu.so, the environment join: what environment-finder-multi needs of several graph.txt files at once (include/mcgpu.h
// mc_env_join*; src/algo/MultiSequenceCalculator.java:51-100, src/io/writers/GFAWriterMulti.java, EnvironmentFinderMultiMain.java:104-170,
// which csrc/host/multi.cpp environment_finder_multi restates on strings and env_join_host on packed keys).  context.h lists the
// other units.
//
// n entries make 2n oriented rows: row 2e is entry e's k-mer as given, row 2e + 1 its reverse complement.  A row has a 64-bit mask of
// the graphs that hold it (`holder`) and one depth a graph (`depth`, G words a row; a word is read only where the mask says so).
//   k_ej_build    an entry's canonical k-mer goes into an open-addressing table (kmer_set.h's keys, at most half full); val[slot] = the
//                 row that spells the canonical form.  A key that is there already raises the duplicate flag.  (unitigs.hip k_ut_build)
//   k_ej_records  one thread a record: its graph by bisection of graph_offsets, its row by a look-up, then an atomic OR of the graph's
//                 bit into the row's mask -- the old value shows a second record of that k-mer in that graph -- and the depth stored.
//   k_ej_gene     one thread a window of the gene: is_gene of the entry it hits.
//   k_ej_pairs    one thread a row, rows dealt to workgroups in a grid-stride loop: member and kc of the entry (the even row writes them),
//                 and the row's terms of diff / diff_alt / uni into G x G x 3 counters in LDS; at the end one global atomic add for every
//                 counter that is not zero.  SMALL (G <= 8): every thread walks all G x G pairs, a wave sums its 64 terms through
//                 shuffles and one lane adds to LDS.  Otherwise a thread walks only i in H and adds to LDS itself (48 KB at G = 64).
// Sums are modulo 2^32 and kc is a sum of at most 64 words: nothing depends on the order in which threads run.
// DESIGN.md 3.13 has the sizes and the registers, tests/test_env_join_kernel_resources.py holds the kernels to no scratch.
#include "context.h"
#include "kmer_set.h"

namespace {

constexpr int EJ_THREADS = 256;
constexpr uint32_t EJ_MAX_GRAPHS = 64;
constexpr uint32_t EJ_SMALL_GRAPHS = 8;
constexpr uint32_t EJ_DUP_ENTRY = 1, EJ_MISS = 2, EJ_DUP_RECORD = 4;  // the flags word

template <bool WIDE>
__device__ __forceinline__ Kmer ej_kmer(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint64_t e, int k)
{
    Kmer v{WIDE ? hi[e] : 0, lo[e]};
    if (WIDE) v.hi &= ~0ull >> (128 - 2 * k);  // (bits above the k-mer are not the caller's to set: dropped)
    else if (k < 32) v.lo &= ~0ull >> (64 - 2 * k);
    return v;
}

template <bool WIDE>
__device__ __forceinline__ bool ej_le(const Kmer &a, const Kmer &b)  // the order rs_key takes its smaller k-mer by
{
    return WIDE ? (a.hi < b.hi || (a.hi == b.hi && a.lo <= b.lo)) : a.lo <= b.lo;
}

// table: 2^lg_cap slots of one word (k <= 32) or two (above), all ones when the call starts; val: a word a slot
template <bool WIDE>
__global__ void __launch_bounds__(EJ_THREADS) k_ej_build(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, uint32_t n, int k,
                                                         unsigned long long *__restrict__ table, uint32_t *__restrict__ val, int lg_cap,
                                                         uint32_t *__restrict__ flags)
{
    const uint32_t e = blockIdx.x * EJ_THREADS + threadIdx.x;
    if (e >= n) return;
    const Kmer v = ej_kmer<WIDE>(hi, lo, e, k);
    const Kmer r = rc_kmer(v, k);
    const RsKey key = rs_key<WIDE>(v.hi, v.lo, r.hi, r.lo);
    const bool fw = ej_le<WIDE>(v, r);
    const uint64_t mask = (1ull << lg_cap) - 1;
    uint64_t s = rs_home(rs_hash<WIDE>(key), lg_cap);
    for (uint64_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {  // (at most half full: a free slot comes)
        unsigned long long *slot = table + (WIDE ? 2 * s : s);
        const unsigned long long was = atomicCAS(slot, (unsigned long long)RS_EMPTY, (unsigned long long)key.a);
        if (was != RS_EMPTY && was != key.a) continue;
        if (!WIDE) {
            if (was == key.a) atomicOr(flags, EJ_DUP_ENTRY);  // (another entry's k-mer, or its reverse complement)
            else val[s] = 2 * e + (fw ? 0 : 1);
            return;
        }
        // (reads_in_set.hip k_rs_build: whoever writes the second word first has the slot)
        const unsigned long long was_b = atomicCAS(slot + 1, (unsigned long long)RS_EMPTY, (unsigned long long)key.b);
        if (was_b == RS_EMPTY) { val[s] = 2 * e + (fw ? 0 : 1); return; }
        if (was_b == key.b) { atomicOr(flags, EJ_DUP_ENTRY); return; }
    }
}

// the row that spells v, or all ones when neither v nor its reverse complement is an entry
template <bool WIDE>
__device__ __forceinline__ uint32_t ej_row(const uint64_t *__restrict__ table, const uint32_t *__restrict__ val, int lg_cap, const Kmer &v, int k)
{
    const Kmer r = rc_kmer(v, k);
    const RsKey key = rs_key<WIDE>(v.hi, v.lo, r.hi, r.lo);
    const uint64_t mask = (1ull << lg_cap) - 1;
    uint64_t s = rs_home(rs_hash<WIDE>(key), lg_cap);
    for (uint64_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {
        if (WIDE) {
            const ulonglong2 cur = *reinterpret_cast<const ulonglong2 *>(table + 2 * s);
            if (cur.x == key.a && cur.y == key.b) break;
            if (cur.x == RS_EMPTY) return ~0u;
        } else {
            const uint64_t cur = table[s];
            if (cur == key.a) break;
            if (cur == RS_EMPTY) return ~0u;
        }
        if (probe == mask) return ~0u;
    }
    const uint32_t w = val[s];  // spells the smaller of v and r (a k-mer that is its own reverse complement: the entry as given)
    return ej_le<WIDE>(v, r) ? w : (w ^ 1);
}

// holder: a word a row, zero when the call starts; depth: G words a row
template <bool WIDE>
__global__ void __launch_bounds__(EJ_THREADS) k_ej_records(const uint64_t *__restrict__ rec_hi, const uint64_t *__restrict__ rec_lo,
                                                           const int32_t *__restrict__ rec_depth, const uint64_t *__restrict__ graph_offsets,
                                                           uint32_t G, uint64_t n_rec, int k, const uint64_t *__restrict__ table,
                                                           const uint32_t *__restrict__ val, int lg_cap, unsigned long long *__restrict__ holder,
                                                           int32_t *__restrict__ depth, uint32_t *__restrict__ flags)
{
    const uint64_t r = (uint64_t)blockIdx.x * EJ_THREADS + threadIdx.x;
    if (r >= n_rec) return;
    uint32_t a = 0, b = G;  // the graph: the last g with graph_offsets[g] <= r (empty graphs before it are passed over)
    while (b - a > 1) {
        const uint32_t m = (a + b) / 2;
        if (graph_offsets[m] <= r) a = m; else b = m;
    }
    const uint32_t row = ej_row<WIDE>(table, val, lg_cap, ej_kmer<WIDE>(rec_hi, rec_lo, r, k), k);
    if (row == ~0u) { atomicOr(flags, EJ_MISS); return; }
    const unsigned long long bit = 1ull << a;
    if (atomicOr(holder + row, bit) & bit) atomicOr(flags, EJ_DUP_RECORD);
    depth[(uint64_t)row * G + a] = rec_depth[r];  // (a second record of the row in this graph ends the call: which depth stays is not read)
}

// gene: packed as reads are, gene_len bases; is_gene: zero when the call starts
template <bool WIDE>
__global__ void __launch_bounds__(EJ_THREADS) k_ej_gene(const uint64_t *__restrict__ gene, uint64_t n_windows, int k,
                                                        const uint64_t *__restrict__ table, const uint32_t *__restrict__ val, int lg_cap,
                                                        uint8_t *__restrict__ is_gene)
{
    const uint64_t w = (uint64_t)blockIdx.x * EJ_THREADS + threadIdx.x;
    if (w >= n_windows) return;
    Kmer v{0, 0};
    for (int i = 0; i < k; i++) {
        const uint64_t at = w + (uint64_t)i;
        const uint64_t code = (gene[at >> 5] >> (62 - 2 * (at & 31))) & 3;
        if (WIDE) v.hi = (v.hi << 2) | (v.lo >> 62);
        v.lo = (v.lo << 2) | code;
    }
    if (WIDE) v.hi &= ~0ull >> (128 - 2 * k);
    else if (k < 32) v.lo &= ~0ull >> (64 - 2 * k);
    const uint32_t row = ej_row<WIDE>(table, val, lg_cap, v, k);
    if (row != ~0u) is_gene[row >> 1] = 1;
}

// |v - w| as the host's int arithmetic gives it, as an unsigned word
__device__ __forceinline__ uint32_t ej_absdiff(int32_t v, int32_t w)
{
    const int32_t d = (int32_t)((uint32_t)v - (uint32_t)w);
    return d < 0 ? 0u - (uint32_t)d : (uint32_t)d;
}

__device__ __forceinline__ uint32_t ej_wave_sum(uint32_t x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// mats: diff, diff_alt, uni one after another, G x G words each (row i, column j at i * G + j), zero when the call starts
template <bool SMALL>
__global__ void __launch_bounds__(EJ_THREADS) k_ej_pairs(uint32_t n_rows, uint32_t G, const unsigned long long *__restrict__ holder,
                                                         const int32_t *__restrict__ depth, unsigned long long *__restrict__ member,
                                                         long long *__restrict__ kc, uint32_t *__restrict__ mats)
{
    constexpr uint32_t MAXG = SMALL ? EJ_SMALL_GRAPHS : EJ_MAX_GRAPHS;
    __shared__ uint32_t acc[3 * MAXG * MAXG];
    const uint32_t GG = G * G;
    for (uint32_t i = threadIdx.x; i < 3 * GG; i += EJ_THREADS) acc[i] = 0;
    __syncthreads();
    // (whole blocks of rows, so that every lane of a wave is in the loop when the wave sums)
    for (uint64_t base = (uint64_t)blockIdx.x * EJ_THREADS; base < n_rows; base += (uint64_t)gridDim.x * EJ_THREADS) {
        const uint64_t row = base + threadIdx.x;
        const bool live = row < n_rows;
        const unsigned long long H = live ? holder[row] : 0;
        const int32_t *d = depth + row * G;  // (read only where H has a bit)
        if (live && !(row & 1)) {
            long long sum = 0;
            for (unsigned long long m = H; m; m &= m - 1) sum += d[__ffsll((long long)m) - 1];
            kc[row >> 1] = sum;
            member[row >> 1] = H | holder[row + 1];
        }
        if (SMALL) {
            for (uint32_t i = 0; i < G; i++) {
                const bool in_i = (H >> i) & 1;
                const int32_t di = in_i ? d[i] : 0;
                for (uint32_t j = 0; j < G; j++) {
                    const bool in_j = (H >> j) & 1;
                    const int32_t dj = in_j ? d[j] : 0;
                    uint32_t t_diff = 0, t_alt = 0, t_uni = 0;
                    if (in_i && in_j) { t_diff = t_alt = ej_absdiff(di, dj); t_uni = (uint32_t)max(di, dj); }
                    else if (in_i) t_diff = t_alt = t_uni = (uint32_t)di;
                    else if (in_j) t_diff = t_uni = (uint32_t)dj;
                    t_diff = ej_wave_sum(t_diff);
                    t_alt = ej_wave_sum(t_alt);
                    t_uni = ej_wave_sum(t_uni);
                    if ((threadIdx.x & 63) == 0) {
                        if (t_diff) atomicAdd(&acc[i * G + j], t_diff);
                        if (t_alt) atomicAdd(&acc[GG + i * G + j], t_alt);
                        if (t_uni) atomicAdd(&acc[2 * GG + i * G + j], t_uni);
                    }
                }
            }
        } else {
            for (unsigned long long m = H; m; m &= m - 1) {
                const uint32_t i = (uint32_t)__ffsll((long long)m) - 1;
                const int32_t di = d[i];
                for (uint32_t j = 0; j < G; j++) {
                    if ((H >> j) & 1) {
                        const int32_t dj = d[j];
                        const uint32_t a = ej_absdiff(di, dj);
                        if (a) { atomicAdd(&acc[i * G + j], a); atomicAdd(&acc[GG + i * G + j], a); }
                        atomicAdd(&acc[2 * GG + i * G + j], (uint32_t)max(di, dj));
                    } else if (di) {
                        const uint32_t u = (uint32_t)di;
                        atomicAdd(&acc[i * G + j], u);
                        atomicAdd(&acc[GG + i * G + j], u);
                        atomicAdd(&acc[2 * GG + i * G + j], u);
                        atomicAdd(&acc[j * G + i], u);  // (seen from j, which does not hold the k-mer: diff and uni only)
                        atomicAdd(&acc[2 * GG + j * G + i], u);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 3 * GG; i += EJ_THREADS)
        if (acc[i]) atomicAdd(mats + i, acc[i]);
}

constexpr char API[] = "mc_env_join";

template <class T>
T *host_array(uint64_t n) { return static_cast<T *>(calloc(std::max<uint64_t>(n, 1), sizeof(T))); }

uint32_t blocks(uint64_t n) { return (uint32_t)((n + EJ_THREADS - 1) / EJ_THREADS); }

int alloc_result(mc_ctx *c, uint64_t n, uint32_t G, mc_env_join_result *out)
{
    out->n = n;
    out->n_graphs = G;
    out->member = host_array<uint64_t>(n);
    out->is_gene = host_array<uint8_t>(n);
    out->kc = host_array<int64_t>(n);
    out->diff = host_array<uint32_t>((uint64_t)G * G);
    out->diff_alt = host_array<uint32_t>((uint64_t)G * G);
    out->uni = host_array<uint32_t>((uint64_t)G * G);
    if (!out->member || !out->is_gene || !out->kc || !out->diff || !out->diff_alt || !out->uni) return fail(c, MC_ENOMEM, "%s: no host memory", API);
    return MC_OK;
}

template <bool WIDE>
int run_env_join(mc_ctx *c, const uint64_t *d_hi, const uint64_t *d_lo, uint32_t n, const uint64_t *d_rec_hi, const uint64_t *d_rec_lo,
                 const int32_t *d_rec_depth, const uint64_t *d_graph_offsets, uint32_t G, uint64_t n_rec, const uint64_t *d_gene, uint64_t gene_len,
                 mc_env_join_result *out)
{
    const int k = c->cfg.k;
    const uint32_t N = 2 * n;
    hipStream_t st = c->stream;
    int lg_cap = 6;
    while ((1ull << lg_cap) < 2 * (uint64_t)n) lg_cap++;  // (at most 31: n < 2^30)
    const uint64_t cap = 1ull << lg_cap, table_words = cap * (WIDE ? 2 : 1), GG = (uint64_t)G * G;
    DevBuf<unsigned long long> table, holder, member;
    DevBuf<uint32_t> val, flags, mats;
    DevBuf<int32_t> depth;
    DevBuf<uint8_t> is_gene;
    DevBuf<long long> kc;
    HIPCHK(c, table.alloc(table_words));
    HIPCHK(c, val.alloc(cap));
    HIPCHK(c, flags.alloc(1));
    const uint64_t *tab = reinterpret_cast<const uint64_t *>(table.p);
    const dim3 bt(EJ_THREADS);
    double ms_set = 0, ms_records = 0, ms_pairs = 0;
    if (int rc = timed(c, &ms_set, [&] {
            (void)hipMemsetAsync(table.p, 0xff, table_words * 8, st);
            (void)hipMemsetAsync(flags.p, 0, 4, st);
            hipLaunchKernelGGL(k_ej_build<WIDE>, dim3(blocks(n)), bt, 0, st, d_hi, d_lo, n, k, table.p, val.p, lg_cap, flags.p);
        }))
        return rc;
    uint32_t *h_flags = reinterpret_cast<uint32_t *>(c->h_scratch);
    HIPCHK(c, hipMemcpyAsync(h_flags, flags.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (*h_flags & EJ_DUP_ENTRY) return fail(c, MC_EINVAL, "%s: two entries are the same k-mer or each other's reverse complement", API);

    HIPCHK(c, holder.alloc(N));
    HIPCHK(c, depth.alloc((uint64_t)N * G));
    HIPCHK(c, is_gene.alloc(n));
    const uint64_t n_windows = gene_len >= (uint64_t)k ? gene_len - (uint64_t)k + 1 : 0;
    if (int rc = timed(c, &ms_records, [&] {
            (void)hipMemsetAsync(holder.p, 0, (uint64_t)N * 8, st);
            (void)hipMemsetAsync(is_gene.p, 0, n, st);
            if (n_rec)
                hipLaunchKernelGGL(k_ej_records<WIDE>, dim3(blocks(n_rec)), bt, 0, st, d_rec_hi, d_rec_lo, d_rec_depth, d_graph_offsets, G, n_rec, k, tab,
                                   val.p, lg_cap, holder.p, depth.p, flags.p);
            if (n_windows) hipLaunchKernelGGL(k_ej_gene<WIDE>, dim3(blocks(n_windows)), bt, 0, st, d_gene, n_windows, k, tab, val.p, lg_cap, is_gene.p);
        }))
        return rc;
    HIPCHK(c, hipMemcpyAsync(h_flags, flags.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (*h_flags & EJ_MISS) return fail(c, MC_EINVAL, "%s: a record's k-mer is no entry, and neither is its reverse complement", API);
    if (*h_flags & EJ_DUP_RECORD) return fail(c, MC_EINVAL, "%s: a graph holds the same oriented k-mer twice", API);
    table.reset();
    val.reset();

    HIPCHK(c, member.alloc(n));
    HIPCHK(c, kc.alloc(n));
    HIPCHK(c, mats.alloc(3 * GG));
    // (every workgroup ends with up to 3 G^2 global adds: few workgroups where that is many)
    const uint32_t grid = std::min<uint32_t>(blocks(N), G <= EJ_SMALL_GRAPHS ? 2048 : 512);
    if (int rc = timed(c, &ms_pairs, [&] {
            (void)hipMemsetAsync(mats.p, 0, 3 * GG * 4, st);
            if (G <= EJ_SMALL_GRAPHS) hipLaunchKernelGGL(k_ej_pairs<true>, dim3(grid), bt, 0, st, N, G, holder.p, depth.p, member.p, kc.p, mats.p);
            else hipLaunchKernelGGL(k_ej_pairs<false>, dim3(grid), bt, 0, st, N, G, holder.p, depth.p, member.p, kc.p, mats.p);
        }))
        return rc;

    if (int rc = alloc_result(c, n, G, out)) return rc;
    HIPCHK(c, hipMemcpy(out->member, member.p, (uint64_t)n * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out->is_gene, is_gene.p, n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out->kc, kc.p, (uint64_t)n * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out->diff, mats.p, GG * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out->diff_alt, mats.p + GG, GG * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out->uni, mats.p + 2 * GG, GG * 4, hipMemcpyDeviceToHost));
    out->device_ms = ms_set + ms_records + ms_pairs;
    return MC_OK;
}

// what both forms refuse before anything is copied or launched (graph_offsets is not read here)
int check_args(mc_ctx *c, const uint64_t *hi, const uint64_t *lo, uint64_t n, const uint64_t *graph_offsets, uint32_t n_graphs, const uint64_t *gene,
               uint64_t gene_len, mc_env_join_result *out)
{
    if (!out) return fail(c, MC_EINVAL, "%s: null pointer", API);
    *out = mc_env_join_result{};
    if (n_graphs == 0 || n_graphs > EJ_MAX_GRAPHS) return fail(c, MC_EINVAL, "%s: %u graphs (1 to %u)", API, n_graphs, EJ_MAX_GRAPHS);
    if (n >= (1ull << 30)) return fail(c, MC_EINVAL, "%s: %llu entries (at most 2^30 - 1)", API, (unsigned long long)n);
    if (!graph_offsets || (gene_len && !gene) || (n && (!lo || (c->cfg.k > 32 && !hi)))) return fail(c, MC_EINVAL, "%s: null pointer", API);
    return MC_OK;
}

// the records' part, once graph_offsets is on the host
int check_records(mc_ctx *c, const uint64_t *offsets, uint32_t n_graphs, const uint64_t *rec_hi, const uint64_t *rec_lo, const int32_t *rec_depth, uint64_t n)
{
    for (uint32_t g = 0; g < n_graphs; g++)
        if (offsets[g] > offsets[g + 1]) return fail(c, MC_EINVAL, "%s: graph_offsets decrease", API);
    if (offsets[0] != 0) return fail(c, MC_EINVAL, "%s: graph_offsets start at %llu, not 0", API, (unsigned long long)offsets[0]);
    const uint64_t n_rec = offsets[n_graphs];
    if (n_rec >= (1ull << 40)) return fail(c, MC_EINVAL, "%s: %llu records", API, (unsigned long long)n_rec);
    if (n_rec && (!rec_lo || !rec_depth || (c->cfg.k > 32 && !rec_hi))) return fail(c, MC_EINVAL, "%s: null pointer", API);
    if (n_rec && n == 0) return fail(c, MC_EINVAL, "%s: a record's k-mer is no entry, and neither is its reverse complement", API);
    return MC_OK;
}

}  // namespace

void mc_env_join_free(mc_env_join_result *r)
{
    if (!r) return;
    free(r->member); free(r->is_gene); free(r->kc); free(r->diff); free(r->diff_alt); free(r->uni);
    *r = mc_env_join_result{};
}

int mc_env_join_dev(mc_ctx *c, const uint64_t *d_hi, const uint64_t *d_lo, uint64_t n, const uint64_t *d_rec_hi, const uint64_t *d_rec_lo,
                    const int32_t *d_rec_depth, const uint64_t *d_graph_offsets, uint32_t n_graphs, const uint64_t *d_gene, uint64_t gene_len,
                    mc_env_join_result *out)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (int rc = check_args(c, d_hi, d_lo, n, d_graph_offsets, n_graphs, d_gene, gene_len, out)) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    uint64_t offsets[EJ_MAX_GRAPHS + 1];
    HIPCHK(c, hipMemcpy(offsets, d_graph_offsets, ((uint64_t)n_graphs + 1) * 8, hipMemcpyDeviceToHost));
    if (int rc = check_records(c, offsets, n_graphs, d_rec_hi, d_rec_lo, d_rec_depth, n)) return rc;
    int rc;
    if (n == 0) rc = alloc_result(c, 0, n_graphs, out);
    else if (c->cfg.k > 32)
        rc = run_env_join<true>(c, d_hi, d_lo, (uint32_t)n, d_rec_hi, d_rec_lo, d_rec_depth, d_graph_offsets, n_graphs, offsets[n_graphs], d_gene, gene_len, out);
    else
        rc = run_env_join<false>(c, d_hi, d_lo, (uint32_t)n, d_rec_hi, d_rec_lo, d_rec_depth, d_graph_offsets, n_graphs, offsets[n_graphs], d_gene, gene_len, out);
    if (rc) mc_env_join_free(out);
    return rc;
}

int mc_env_join(mc_ctx *c, const uint64_t *hi, const uint64_t *lo, uint64_t n, const uint64_t *rec_hi, const uint64_t *rec_lo, const int32_t *rec_depth,
                const uint64_t *graph_offsets, uint32_t n_graphs, const uint64_t *gene, uint64_t gene_len, mc_env_join_result *out)
{
    if (!c) return MC_EINVAL;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (int rc = check_args(c, hi, lo, n, graph_offsets, n_graphs, gene, gene_len, out)) return rc;
        if (int rc = check_records(c, graph_offsets, n_graphs, rec_hi, rec_lo, rec_depth, n)) return rc;
    }
    const bool wide = c->cfg.k > 32;
    const uint64_t n_rec = graph_offsets[n_graphs];
    HostStage st(c);
    const uint64_t *dhi = wide && n ? st.in(hi, n) : nullptr, *dlo = n ? st.in(lo, n) : nullptr;
    const uint64_t *drhi = wide && n_rec ? st.in(rec_hi, n_rec) : nullptr, *drlo = n_rec ? st.in(rec_lo, n_rec) : nullptr;
    const int32_t *drd = n_rec ? st.in(rec_depth, n_rec) : nullptr;
    const uint64_t *doff = st.in(graph_offsets, (uint64_t)n_graphs + 1);
    const uint64_t *dgene = gene_len ? st.in(gene, (gene_len + 31) / 32) : nullptr;
    if (int rc = st.staged()) {
        *out = mc_env_join_result{};
        return rc;
    }
    return mc_env_join_dev(c, dhi, dlo, n, drhi, drlo, drd, doff, n_graphs, dgene, gene_len, out);
}
