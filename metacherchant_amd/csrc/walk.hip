// libmcgpu.so, the walk: the host driver of csrc/bfs_device.h (mc_bfs_batch, mc_bfs), its result pool, and the walk over
// several ranks' tables where they are (mc_shard_*).  The table work a walk needs -- the solid table, the check of its
// "absent" look-ups -- launches the counting unit's kernels and lives there (context.h).
#include <unistd.h>

#include <array>
#include <chrono>
#include <cstring>

#include "context.h"
#include "bfs_device.h"

extern "C" {

// The arrays of a BFS result are page-locked host memory from a process-wide pool (a block serves again once
// mc_bfs_result_free has returned it): the copies from the device run at the link rate without a staging pass, and a
// reused block costs no page faults -- 0.4 ms of a 29 ms step for two passes of 10^5 k-mers.  A 64-byte header in front
// of every array says what it is; pageable memory takes over when page-locked memory cannot be had.
namespace {
struct ResHeader {
    uint64_t kind;   // 1: page-locked block of the pool, 2: malloc
    uint64_t bytes;  // of the whole block
    uint64_t pad[6];
};
static_assert(sizeof(ResHeader) == 64, "arrays stay 64-byte aligned");
struct ResPool {
    std::mutex mu;
    std::vector<std::pair<void *, size_t>> idle;
    size_t idle_bytes = 0;
} g_res_pool;

void *res_alloc(size_t bytes)
{
    size_t want = 64 + std::max<size_t>(bytes, 1);
    want = (want + 4095) / 4096 * 4096;
    void *blk = nullptr;
    size_t got = 0;
    {
        std::lock_guard<std::mutex> g(g_res_pool.mu);
        size_t best = g_res_pool.idle.size();
        for (size_t i = 0; i < g_res_pool.idle.size(); i++) {
            const size_t b = g_res_pool.idle[i].second;
            if (b >= want && b <= 2 * want + (64u << 10) && (best == g_res_pool.idle.size() || b < g_res_pool.idle[best].second)) best = i;
        }
        if (best < g_res_pool.idle.size()) {
            blk = g_res_pool.idle[best].first;
            got = g_res_pool.idle[best].second;
            g_res_pool.idle_bytes -= got;
            g_res_pool.idle.erase(g_res_pool.idle.begin() + (long)best);
        }
    }
    uint64_t kind = 1;
    if (!blk) {
        got = want;
        if (hipHostMalloc(&blk, got) != hipSuccess) {
            (void)hipGetLastError();
            blk = malloc(got);
            kind = 2;
            if (!blk) return nullptr;
        }
    }
    ResHeader *h = static_cast<ResHeader *>(blk);
    h->kind = kind;
    h->bytes = got;
    return static_cast<char *>(blk) + 64;
}

void res_free(void *p)
{
    if (!p) return;
    ResHeader *h = reinterpret_cast<ResHeader *>(static_cast<char *>(p) - 64);
    if (h->kind == 2) { free(h); return; }
    std::lock_guard<std::mutex> g(g_res_pool.mu);
    if (g_res_pool.idle.size() >= 64 || g_res_pool.idle_bytes + h->bytes > (512u << 20)) {
        (void)hipHostFree(h);
        return;
    }
    g_res_pool.idle_bytes += h->bytes;
    g_res_pool.idle.emplace_back(h, (size_t)h->bytes);
}
}  // namespace

void mc_bfs_result_free(mc_bfs_result *r)
{
    if (!r) return;
    res_free(r->hi);  // (one block holds all five arrays: mc_bfs_batch)
    memset(r, 0, sizeof *r);
}

namespace {

int bfs_alloc(mc_ctx *c, BfsState &S, uint64_t dcap)
{
    S.dcap = dcap;
    uint64_t vcap = 1024;
    while (vcap < 4 * dcap) vcap <<= 1;
    S.bmask = vcap / 2 - 1;
    HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&S.hi), dcap * 8));
    HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&S.lo), dcap * 8));
    HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&S.dist), dcap * 4));
    HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&S.cov), dcap * 2));
    HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&S.flags), dcap * 4));
    HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&S.vis), vcap * 8));
    HIPCHK(c, hipMemsetAsync(S.vis, 0xFF, vcap * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(S.flags, 0, dcap * 4, c->stream));
    return MC_OK;
}

}  // namespace

// What mc_bfs_batch used to do with 4 fills per job before the launch and 5 + 2 copies per job behind it (each a
// launch of its own, 10-25 us apart: 0.7 ms of a 9 ms walk on two jobs) is one kernel either side.
// k_bfs_reset: blockIdx.y = job.  full: index emptied, flags and control block cleared (a fresh run); always: the mailbox.
__global__ void __launch_bounds__(256) k_bfs_reset(const BfsState *__restrict__ states, int full)
{
    const BfsState S = states[blockIdx.y];
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x, stride = (uint64_t)gridDim.x * 256;
    if (full) {
        uint4 *vis = reinterpret_cast<uint4 *>(S.vis);  // (bmask + 1 buckets of 16 bytes)
        for (uint64_t i = t; i <= S.bmask; i += stride) vis[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
        for (uint64_t i = t; i < S.dcap; i += stride) S.flags[i] = 0;
        uint32_t *ctl = reinterpret_cast<uint32_t *>(S.ctl);
        for (uint64_t i = t; i < sizeof(BfsCtl) / 4; i += stride) ctl[i] = 0;
    }
    if (S.box) {
        uint32_t *box = reinterpret_cast<uint32_t *>(S.box);
        for (uint64_t i = t; i < sizeof(ScoutBox) / 4; i += stride) box[i] = 0;
    }
}

// the header of a job's packed results
struct BfsPackHdr {
    BfsCtl ctl;
    ScoutBox box;
    unsigned long long offset;  // of the job's arrays in the data block: hi[n] lo[n] dist[n] cov[n] last[n], each padded to 8 bytes
    unsigned long long levels;  // max distance
};
__host__ __device__ inline uint64_t bfs_pack_bytes(uint64_t n) { return 16 * n + ((4 * n + 7) & ~7ull) + ((2 * n + 7) & ~7ull) + ((n + 7) & ~7ull); }

// k_bfs_pack: blockIdx.y = job.  Control block and mailbox into the job's header, its arrays (the first ctl.n entries)
// into the data block behind the arrays of the jobs before it; `last` from bit 0 of the flags; the largest distance.
__global__ void __launch_bounds__(256) k_bfs_pack(const BfsState *__restrict__ states, uint32_t n_jobs, BfsPackHdr *hdr, char *data, uint64_t data_cap)
{
    (void)n_jobs;
    const uint32_t j = blockIdx.y;
    const BfsState S = states[j];
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x, stride = (uint64_t)gridDim.x * 256;
    unsigned long long off = 0;
    for (uint32_t i = 0; i < j; i++) off += bfs_pack_bytes(ctl_ld(&states[i].ctl->n));
    const uint64_t n = ctl_ld(&S.ctl->n);
    if (blockIdx.x == 0) {
        uint32_t *h = reinterpret_cast<uint32_t *>(&hdr[j]);
        const uint32_t *ctl = reinterpret_cast<const uint32_t *>(S.ctl), *box = reinterpret_cast<const uint32_t *>(S.box);
        for (uint32_t i = threadIdx.x; i < sizeof(BfsCtl) / 4; i += 256) h[i] = __hip_atomic_load(&ctl[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (uint32_t i = threadIdx.x; i < sizeof(ScoutBox) / 4; i += 256)
            h[sizeof(BfsCtl) / 4 + i] = box ? __hip_atomic_load(&box[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        if (threadIdx.x == 0) hdr[j].offset = off;
    }
    if (off + bfs_pack_bytes(n) > data_cap) return;  // (the host sizes the block from the jobs' capacities: cannot happen)
    uint64_t *hi = reinterpret_cast<uint64_t *>(data + off), *lo = hi + n;
    int32_t *dist = reinterpret_cast<int32_t *>(lo + n);
    int16_t *cov = reinterpret_cast<int16_t *>(reinterpret_cast<char *>(dist) + ((4 * n + 7) & ~7ull));
    uint8_t *last = reinterpret_cast<uint8_t *>(reinterpret_cast<char *>(cov) + ((2 * n + 7) & ~7ull));
    unsigned long long mx = 0;
    for (uint64_t i = t; i < n; i += stride) {
        hi[i] = S.hi[i];
        lo[i] = S.lo[i];
        const int32_t d = S.dist[i];
        dist[i] = d;
        cov[i] = S.cov[i];
        last[i] = (uint8_t)(S.flags[i] & 1u);
        mx = max(mx, (unsigned long long)(uint32_t)d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned long long)__shfl_down(mx, o));
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&hdr[j].levels, mx);
}

namespace {

// MC_BFS_SELFCHECK: the finished walks of a batch against the invariants of k_bfs_check; *report names what was found
int bfs_selfcheck(mc_ctx *c, uint32_t n_jobs, const std::vector<BfsCtl> &ctl, int min_cov, int64_t max_kmers, int64_t max_radius,
                  std::string *report)
{
    const SolidView t = c->solid_view();
    BfsCheck *d_out = nullptr;
    HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&d_out), sizeof(BfsCheck)));
    for (uint32_t j = 0; j < n_jobs; j++) {
        const BfsState &S = c->bfs_pool[j]->S;
        const uint64_t n = ctl[j].n;
        if (n == 0) continue;
        uint64_t cap = 1024;
        while (cap < 4 * n) cap <<= 1;
        uint32_t *d_set = nullptr;
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&d_set), cap * 4));
        HIPCHK(c, hipMemsetAsync(d_set, 0xFF, cap * 4, c->stream));
        HIPCHK(c, hipMemsetAsync(d_out, 0, sizeof(BfsCheck), c->stream));
        const unsigned grid = (unsigned)std::min<uint64_t>(grid_for(n, 256), 4096);
        hipLaunchKernelGGL(k_bfs_check_index, dim3(grid), dim3(256), 0, c->stream, S, n, d_set, (uint32_t)(cap - 1), d_out);
        switch (c->cfg.key_mode) {
        case MC_KEY_PACKED:
            hipLaunchKernelGGL(k_bfs_check<KEY_PACKED>, dim3(grid), dim3(256), 0, c->stream, S, n, t, c->cfg.k, min_cov, (long long)max_kmers,
                               (long long)max_radius, d_set, (uint32_t)(cap - 1), d_out);
            break;
        case MC_KEY_POLY:
            hipLaunchKernelGGL(k_bfs_check<KEY_POLY>, dim3(grid), dim3(256), 0, c->stream, S, n, t, c->cfg.k, min_cov, (long long)max_kmers,
                               (long long)max_radius, d_set, (uint32_t)(cap - 1), d_out);
            break;
        default:
            hipLaunchKernelGGL(k_bfs_check<KEY_FNV1A>, dim3(grid), dim3(256), 0, c->stream, S, n, t, c->cfg.k, min_cov, (long long)max_kmers,
                               (long long)max_radius, d_set, (uint32_t)(cap - 1), d_out);
        }
        HIPCHK(c, hipGetLastError());
        BfsCheck h;
        HIPCHK(c, hipMemcpyAsync(&h, d_out, sizeof h, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        (void)hipFree(d_set);
        if (h.dup | h.cov | h.order | h.orphan | h.open) {
            char buf[256];
            snprintf(buf, sizeof buf, "job %u (dir %d, n %llu): %llu duplicate, %llu wrong coverage, %llu out of order, %llu without parent, %llu solid neighbours left out;",
                     j, S.dir, (unsigned long long)n, h.dup, h.cov, h.order, h.orphan, h.open);
            *report += buf;
            static const char *kind[] = {"?", "dup", "cov", "order", "orphan", "open"};
            for (uint32_t i = 0; i < std::min<uint32_t>(h.n_first, 16); i++) {
                snprintf(buf, sizeof buf, " [%s entry %u other %u dist %u]", kind[std::min<uint32_t>(h.first[i][0], 5)], h.first[i][1], h.first[i][2], h.first[i][3]);
                *report += buf;
            }
        }
    }
    (void)hipFree(d_out);
    return MC_OK;
}

// the rounds' trace of every job (MC_BFS_TRACE builds; nothing otherwise), oldest record first, as text
void bfs_trace_dump(mc_ctx *c, uint32_t n_jobs, const std::vector<BfsCtl> &ctl, const char *path, const std::string &why)
{
    FILE *f = fopen(path, "a");
    if (!f) return;
    if (!why.empty()) fprintf(f, "# %s\n", why.c_str());
    for (uint32_t j = 0; j < n_jobs; j++) {
        const BfsState &S = c->bfs_pool[j]->S;
        fprintf(f, "# job %u dir %d n %llu level %lld status %d rounds_narrow %llu slow %llu trace records %llu\n", j, S.dir, ctl[j].n, ctl[j].level, ctl[j].status,
                ctl[j].rounds_narrow, ctl[j].rounds_slow, ctl[j].trace_n);
        if (!S.trace || !ctl[j].trace_n) continue;
        std::vector<uint32_t> ring((size_t)BFS_TRACE_RECORDS * 8);
        if (hipMemcpy(ring.data(), S.trace, ring.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) continue;
        const unsigned long long tn = ctl[j].trace_n, first = tn > BFS_TRACE_RECORDS ? tn - BFS_TRACE_RECORDS : 0;
        for (unsigned long long r = first; r < tn; r++) {
            const uint32_t *w = &ring[(size_t)(r & (BFS_TRACE_RECORDS - 1)) * 8];
            const uint32_t kind = w[0] >> 24;
            if (kind == 8)
                fprintf(f, "%llu companion seq %u F %u team %u stopped %u levels %u %u budget %u stuck %u %u iters %u\n", r, w[0] & 0xFFFFFF, w[1] & 0xFF, (w[1] >> 8) & 0xFF,
                        (w[1] >> 16) & 1, w[2], w[3], w[4], w[5] & 0xFF, (w[5] >> 8) & 0xFF, w[6]);
            else
                fprintf(f, "%llu %s round %u n %u F %u H %u %s %u force_slow %u comp %u level %u pend %u %s %u seq %u open %u resp %08x %s %u %u\n", r,
                        kind == 1 ? "fast" : kind == 2 ? "slow" : "root_bad", w[0] & 0xFFFFFF, w[1], w[2] & 0xFF, (w[2] >> 8) & 0xFF, kind == 2 ? "n_new" : "J", (w[2] >> 16) & 0xFF,
                        (w[2] >> 24) & 1, (w[2] >> 25) & 1, w[3], w[4] & 0xFFFF, kind == 2 ? "F_next" : "bad_lvl", w[4] >> 16, w[5] & 0x7FFFFFFF, w[5] >> 31, w[6],
                        kind == 2 ? "n_after" : "plen0/ppos0", kind == 2 ? w[7] : w[7] & 0xFFFF, kind == 2 ? 0u : w[7] >> 16);
        }
    }
    fclose(f);
}

void launch_bfs(mc_ctx *c, hipStream_t stream, const BfsState *d_states, uint32_t n_jobs, int min_cov, int64_t max_kmers,
                int64_t max_radius, unsigned long long max_rounds, int companions)
{
    const SolidView t = c->solid_view();
    // companions: the scouts' kernel beside the walk's, on the side stream -- behind what the main stream has enqueued so far (the
    // mailboxes' reset), and the main stream takes nothing up behind the walk before the scouts have left (they leave when the walk
    // sets `quit`, which it does on every way out)
    hipStream_t side = companions && c->pipe_stream ? c->pipe_stream : nullptr;
    if (companions && !side) companions = 0;
    if (side) {
        if (hipEventRecord(c->ev_piece[0], stream) != hipSuccess || hipStreamWaitEvent(side, c->ev_piece[0], 0) != hipSuccess) { side = nullptr; companions = 0; }
    }
    // (SH: the walk over several ranks' tables, every look-up through its key's owner; the one-table kernel carries none of that)
#define BFS_LAUNCH(MODE)                                                                                                          \
    do {                                                                                                                          \
        if (t.n_shards > 1) {                                                                                                     \
            if (side) hipLaunchKernelGGL((k_bfs_scout<MODE, true>), dim3(n_jobs), dim3(BFS_THREADS), 0, side, d_states, t, c->cfg.k, min_cov); \
            hipLaunchKernelGGL((k_bfs<MODE, true>), dim3(n_jobs), dim3(BFS_THREADS), 0, stream, d_states, t, c->cfg.k, min_cov,    \
                               (long long)max_kmers, (long long)max_radius, max_rounds, companions);                              \
        } else {                                                                                                                  \
            if (side) hipLaunchKernelGGL((k_bfs_scout<MODE, false>), dim3(n_jobs), dim3(BFS_THREADS), 0, side, d_states, t, c->cfg.k, min_cov); \
            hipLaunchKernelGGL((k_bfs<MODE, false>), dim3(n_jobs), dim3(BFS_THREADS), 0, stream, d_states, t, c->cfg.k, min_cov,   \
                               (long long)max_kmers, (long long)max_radius, max_rounds, companions);                              \
        }                                                                                                                         \
    } while (0)
    switch (c->cfg.key_mode) {
    case MC_KEY_PACKED: BFS_LAUNCH(KEY_PACKED); break;
    case MC_KEY_POLY: BFS_LAUNCH(KEY_POLY); break;
    default: BFS_LAUNCH(KEY_FNV1A);
    }
#undef BFS_LAUNCH
    if (side) {
        (void)hipEventRecord(c->ev_piece[1], side);
        (void)hipStreamWaitEvent(stream, c->ev_piece[1], 0);
    }
}


}  // namespace

int mc_bfs_batch(mc_ctx *c, const mc_bfs_job *jobs, uint32_t n_jobs, int min_cov, int64_t max_kmers,
                 int64_t max_radius, mc_bfs_result *out)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!out || !jobs || n_jobs == 0) return fail(c, MC_EINVAL, "mc_bfs: null argument");
    memset(out, 0, sizeof(mc_bfs_result) * n_jobs);
    if (!c->finalized) return fail(c, MC_ESTATE, "mc_bfs: call mc_finalize_counts first");
    if (c->shards_dropped)
        return fail(c, MC_ESTATE, "mc_bfs: the table changed after mc_shard_attach, which dropped the attachment: export and attach the ranks' tables again (or mc_shard_detach to walk this table alone)");
    if (max_kmers < 0 && max_radius < 0)
        return fail(c, MC_EINVAL, "At least one of --maxkmers and --maxradius parameters should be set");
    if (min_cov < 0)
        return fail(c, MC_EINVAL, "mc_bfs: negative coverage threshold (absent k-mers read as -1 and would pass)");
    if (n_jobs > 4096) return fail(c, MC_EINVAL, "mc_bfs: too many jobs in one batch");
    for (uint32_t j = 0; j < n_jobs; j++) {
        if (jobs[j].dir < -1 || jobs[j].dir > 1) return fail(c, MC_EINVAL, "mc_bfs: dir must be -1, 0 or +1");
        if (jobs[j].n_seeds && !jobs[j].seed_lo) return fail(c, MC_EINVAL, "mc_bfs: seed_lo is null");
        if (c->cfg.k > 32 && jobs[j].n_seeds && !jobs[j].seed_hi)
            return fail(c, MC_EINVAL, "mc_bfs: seed_hi is null with k > 32");
        if (max_kmers >= (int64_t)0x3FFFF000ll || jobs[j].n_seeds >= 0x3FFFF000ull)
            return fail(c, MC_EINVAL, "mc_bfs: more than 2^30 vertices requested");
    }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    double total_ms = c->pending_solid_ms;
    c->pending_solid_ms = 0;
    {
        int rc = ensure_solid(c, min_cov, &total_ms);
        // (hash keys in minimizer bins: the join of mc_finalize_counts, should anything have skipped it)
        if (!rc && hash_bins(c) && c->solid_is_table && !c->d_shards && dup_check_on() && !c->dup.checked) {
            c->dup.l1_armed = false;
            rc = ensure_dups(c);
            if (!rc) rc = ensure_solid(c, min_cov, &total_ms);
        }
        if (rc) return rc;
    }

    while (c->bfs_pool.size() < n_jobs) c->bfs_pool.emplace_back(new BfsJobBuffers);
    auto &B = c->bfs_pool;
    // ---- one upload: the job states, then every job's seeds (lo, hi)
    uint64_t stage_bytes = ((uint64_t)n_jobs * sizeof(BfsState) + 63) & ~63ull, pack_bytes = 0;
    std::vector<uint64_t> seed_at(n_jobs);
    for (uint32_t j = 0; j < n_jobs; j++) {
        seed_at[j] = stage_bytes;
        stage_bytes += 2 * std::max<uint64_t>(jobs[j].n_seeds, 1) * 8;
    }
    if (c->bfs_stage_cap < stage_bytes) {
        if (c->h_bfs_stage) (void)hipHostFree(c->h_bfs_stage);
        if (c->d_bfs_stage) (void)hipFree(c->d_bfs_stage);
        c->h_bfs_stage = c->d_bfs_stage = nullptr;
        c->bfs_stage_cap = 0;
        const uint64_t cap = std::max<uint64_t>(stage_bytes * 2, 1u << 16);
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&c->h_bfs_stage), cap, hipHostMallocDefault));
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&c->d_bfs_stage), cap));
        c->bfs_stage_cap = cap;
    }
    for (uint32_t j = 0; j < n_jobs; j++) {
        BfsJobBuffers &J = *B[j];
        BfsState &S = J.S;
        const uint64_t ns = jobs[j].n_seeds;
        uint64_t *h_lo = reinterpret_cast<uint64_t *>(c->h_bfs_stage + seed_at[j]), *h_hi = h_lo + std::max<uint64_t>(ns, 1);
        if (ns) memcpy(h_lo, jobs[j].seed_lo, ns * 8);
        if (ns && jobs[j].seed_hi) memcpy(h_hi, jobs[j].seed_hi, ns * 8);
        const uint64_t dcap = max_kmers >= 0 ? std::max<uint64_t>((uint64_t)max_kmers, ns) + 2 * BFS_THREADS
                                             : std::max<uint64_t>(1ull << 20, ns + 2 * BFS_THREADS);
        if (S.dcap < dcap || S.dcap > 4 * dcap || !S.hi) {
            J.free_arrays();
            int rc = bfs_alloc(c, S, dcap);
            if (rc) return rc;
        }  // (reused arrays: k_bfs_reset empties the index and clears the flags)
        if (!S.ctl) HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&S.ctl), sizeof(BfsCtl)));
        if (!S.path) HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&S.path), (size_t)SCOUT_MAX_F * PATH_WORDS * 8));
        if (!S.box) HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&S.box), sizeof(ScoutBox)));
#ifdef MC_BFS_TRACE
        if (!S.trace) HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&S.trace), (size_t)BFS_TRACE_RECORDS * 32));
#endif
        uint64_t *d_lo = reinterpret_cast<uint64_t *>(c->d_bfs_stage + seed_at[j]);
        S.seed_hi = jobs[j].seed_hi ? d_lo + std::max<uint64_t>(ns, 1) : nullptr;
        S.seed_lo = d_lo;
        S.n_seeds = ns;
        S.dir = jobs[j].dir;
    }
    BfsState *const d_states = reinterpret_cast<BfsState *>(c->d_bfs_stage);
    BfsState *const h_states = reinterpret_cast<BfsState *>(c->h_bfs_stage);
    std::vector<BfsCtl> ctl(n_jobs);
    const unsigned long long max_rounds = 1ull << 17;  // bounds one launch; unfinished jobs are relaunched
    std::vector<std::array<unsigned long long, 4>> box_e(n_jobs, std::array<unsigned long long, 4>{0, 0, 0, 0});
    std::vector<unsigned long long> box_iters(n_jobs, 0), box_hops(n_jobs, 0), box_levels(n_jobs, 0), box_calls(n_jobs, 0), box_nf(n_jobs, 0), box_m0(n_jobs, 0);
    const uint64_t hdr_bytes = (uint64_t)n_jobs * sizeof(BfsPackHdr);
    BfsPackHdr *h_hdr = nullptr;
    for (int pass = 0;; pass++) {  // (a pass more where the check of the walk's look-ups by key gave the table a slot: phantom_verify)
    for (int launch = 0;; launch++) {
        for (uint32_t j = 0; j < n_jobs; j++) h_states[j] = B[j]->S;
        // (first launch: states and seeds; later ones, after a job's arrays grew: the states)
        HIPCHK(c, hipMemcpyAsync(c->d_bfs_stage, c->h_bfs_stage, launch == 0 ? stage_bytes : (uint64_t)n_jobs * sizeof(BfsState), hipMemcpyHostToDevice, c->stream));
        // Few jobs: each gets a second workgroup that scouts ahead while the first verifies (bfs_device.h ScoutBox).  The
        // pair must be on the chip together to gain anything (it is correct either way), so not for large batches.
        const int companions = c->sw.bfs_companion && n_jobs <= 64 && c->solid_view().reads != nullptr ? 1 : 0;
        hipLaunchKernelGGL(k_bfs_reset, dim3(n_jobs <= 8 ? 64 : 8, n_jobs), dim3(256), 0, c->stream, d_states, launch == 0 ? 1 : 0);
        HIPCHK(c, hipGetLastError());
        pack_bytes = 0;
        for (uint32_t j = 0; j < n_jobs; j++) pack_bytes += bfs_pack_bytes(B[j]->S.dcap);
        if (c->bfs_pack_cap < hdr_bytes + pack_bytes) {
            if (c->d_bfs_pack) (void)hipFree(c->d_bfs_pack);
            c->d_bfs_pack = nullptr;
            c->bfs_pack_cap = 0;
            HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&c->d_bfs_pack), hdr_bytes + pack_bytes));
            c->bfs_pack_cap = hdr_bytes + pack_bytes;
        }
        if (c->bfs_hdr_cap < hdr_bytes) {
            if (c->h_bfs_hdr) (void)hipHostFree(c->h_bfs_hdr);
            c->h_bfs_hdr = nullptr;
            c->bfs_hdr_cap = 0;
            HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&c->h_bfs_hdr), hdr_bytes * 2, hipHostMallocDefault));
            c->bfs_hdr_cap = hdr_bytes * 2;
        }
        // (the walk, the packing of its results and the copy of their headers are enqueued together: one wait)
        HIPCHK(c, hipEventRecord(c->ev0, c->stream));
        launch_bfs(c, c->stream, d_states, n_jobs, min_cov, max_kmers, max_radius, max_rounds, companions);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->ev1, c->stream));
        int rc;
        // ---- the results packed on the device: headers (control block, mailbox, offset, levels), then the jobs' arrays
        h_hdr = reinterpret_cast<BfsPackHdr *>(c->h_bfs_hdr);
        HIPCHK(c, hipMemsetAsync(c->d_bfs_pack, 0, hdr_bytes, c->stream));
        hipLaunchKernelGGL(k_bfs_pack, dim3(n_jobs <= 8 ? 64 : 8, n_jobs), dim3(256), 0, c->stream, d_states, n_jobs,
                           reinterpret_cast<BfsPackHdr *>(c->d_bfs_pack), c->d_bfs_pack + hdr_bytes, pack_bytes);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(h_hdr, c->d_bfs_pack, hdr_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        {
            float ms = 0;
            HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
            total_ms += ms;
        }
        for (uint32_t j = 0; j < n_jobs; j++) {
            ctl[j] = h_hdr[j].ctl;
            if (!companions) continue;
            const ScoutBox &hb = h_hdr[j].box;
            box_iters[j] += hb.iters; box_e[j][0] += hb.e_stuck; box_e[j][1] += hb.e_nc0; box_e[j][2] += hb.e_budget; box_e[j][3] += hb.e_stop; box_hops[j] += hb.hops; box_levels[j] += hb.levels; box_calls[j] += hb.calls; box_nf[j] += hb.nf; box_m0[j] += hb.m0;
        }
        bool all_done = true;
        for (uint32_t j = 0; j < n_jobs; j++) {
            if (ctl[j].status == BFS_DONE) continue;
            all_done = false;
            if (ctl[j].status != BFS_NEED_GROW) continue;
            // grow distanceToKmer and its index (only reachable without --maxkmers)
            BfsState &S = B[j]->S;
            BfsState N = S;
            N.hi = N.lo = nullptr; N.dist = nullptr; N.cov = nullptr; N.flags = nullptr; N.vis = nullptr;  // (ctl and path stay)
            rc = bfs_alloc(c, N, S.dcap * 2);
            if (rc) return rc;
            const uint64_t n = ctl[j].n;
            HIPCHK(c, hipMemcpyAsync(N.hi, S.hi, n * 8, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(N.lo, S.lo, n * 8, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(N.dist, S.dist, n * 4, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(N.cov, S.cov, n * 2, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(N.flags, S.flags, n * 4, hipMemcpyDeviceToDevice, c->stream));
            if (n) {
                hipLaunchKernelGGL(k_vis_rebuild, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, N, n);
                HIPCHK(c, hipGetLastError());
            }
            const int running = BFS_RUNNING;
            HIPCHK(c, hipMemcpyAsync(&S.ctl->status, &running, sizeof running, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            B[j]->free_arrays();
            S = N;
        }
        if (all_done) break;
    }
    bool redo = false;
    if (int vrc = phantom_verify(c, n_jobs, B, ctl, &redo)) return vrc;
    if (!redo) break;
    if (pass >= 8) return fail(c, MC_EOVERFLOW, "mc_bfs: the walk keeps finding keys that strings nobody counted ask for");
    }

    int ret = MC_OK;
    {   // debug: every walk checked on the device (bfs_device.h k_bfs_check); the rounds' trace of a tuning build written out
        const std::string &dump = c->sw.bfs_trace_dump;
        std::string report;
        if (c->sw.bfs_selfcheck) {
            int rc = bfs_selfcheck(c, n_jobs, ctl, min_cov, max_kmers, max_radius, &report);
            if (rc) return rc;
        }
        if (!report.empty() || !dump.empty()) bfs_trace_dump(c, n_jobs, ctl, dump.empty() ? "/dev/stderr" : dump.c_str(), report);
        if (!report.empty()) return fail(c, MC_ECHECK, "mc_bfs: self-check failed: %s", report.c_str());
    }
    for (uint32_t j = 0; j < n_jobs; j++) {
        const uint64_t n = ctl[j].n;
        mc_bfs_result *o = &out[j];
        o->lookups = ctl[j].lookups;
        // (a scout hop: the read, then its k-mers; the members of a companion's team hop side by side)
        o->rounds = ctl[j].rounds_narrow + ctl[j].chunks_wide + 2 * (ctl[j].scout_hops + box_iters[j]);
        o->device_ms = total_ms;
        {
            const bool stats = c->sw.bfs_stats;
            if (stats) fprintf(stderr, "[bfs job %u] slow rounds: after a partly verified round %llu, first level mismatch %llu, nothing predicted %llu; companion runs ended: stuck %llu, no candidates %llu, budget %llu, aborted %llu\n",
                               j, ctl[j].slow_forced, ctl[j].slow_mismatch, ctl[j].slow_starved, box_e[j][0], box_e[j][1], box_e[j][2], box_e[j][3]);
            if (stats)
                fprintf(stderr, "[bfs job %u] n=%llu level=%lld rounds_narrow=%llu (slow %llu) chunks_wide=%llu scout calls=%llu hops=%llu (team hops %llu) levels=%llu notfound=%llu m0=%llu lookups=%llu\n", j,
                        ctl[j].n, ctl[j].level, ctl[j].rounds_narrow, ctl[j].rounds_slow, ctl[j].chunks_wide, ctl[j].scout_calls + box_calls[j], ctl[j].scout_hops + box_hops[j], box_iters[j],
                        ctl[j].scout_levels + box_levels[j], ctl[j].scout_nf + box_nf[j], ctl[j].scout_m0 + box_m0[j], ctl[j].lookups);
        }
#ifdef MC_BFS_TIMING
        {
            const double r_ = 0.01 / std::max(1ull, ctl[j].rounds_narrow);
            fprintf(stderr, "[bfs job %u] rounds_narrow=%llu (slow %llu) chunks_wide=%llu levels~%lld  us/round: gen+issue %.2f table %.2f vis+check %.2f accept %.2f publish %.2f (%.2f %.2f)\n",
                    j, ctl[j].rounds_narrow, ctl[j].rounds_slow, ctl[j].chunks_wide, ctl[j].level, ctl[j].tacc[0] * r_,
                    ctl[j].tacc[1] * r_, ctl[j].tacc[2] * r_, ctl[j].tacc[3] * r_, ctl[j].tacc[4] * r_, ctl[j].tacc[5] * r_,
                    ctl[j].tacc[6] * r_);
        }
#endif
        if (n == 0) continue;  // the reference's "fail": no seed k-mer passes (out[j].n == 0)
        // one block per job (mc_bfs_result_free releases it through `hi`), laid out as k_bfs_pack wrote it
        char *blk = static_cast<char *>(res_alloc(bfs_pack_bytes(n)));
        if (!blk) {
            ret = fail(c, MC_ENOMEM, "mc_bfs: out of host memory");
            break;
        }
        o->n = n;
        o->hi = reinterpret_cast<uint64_t *>(blk);
        o->lo = o->hi + n;
        o->dist = reinterpret_cast<int32_t *>(o->lo + n);
        o->cov = reinterpret_cast<int16_t *>(reinterpret_cast<char *>(o->dist) + ((4 * n + 7) & ~7ull));
        o->last = reinterpret_cast<uint8_t *>(reinterpret_cast<char *>(o->cov) + ((2 * n + 7) & ~7ull));
        o->levels = h_hdr[j].levels;
        const hipError_t e = hipMemcpyAsync(blk, c->d_bfs_pack + hdr_bytes + h_hdr[j].offset, bfs_pack_bytes(n), hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) {
            ret = fail(c, MC_EHIP, "mc_bfs: %s", hipGetErrorString(e));
            break;
        }
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess && ret == MC_OK) ret = fail(c, MC_EHIP, "mc_bfs: copying the results failed");
    if (ret != MC_OK)
        for (uint32_t j = 0; j < n_jobs; j++) mc_bfs_result_free(&out[j]);
    return ret;
}

int mc_bfs(mc_ctx *c, const uint64_t *seed_hi, const uint64_t *seed_lo, uint64_t n_seeds, int dir, int min_cov,
           int64_t max_kmers, int64_t max_radius, mc_bfs_result *out)
{
    if (!c) return MC_EINVAL;
    if (!out) return fail(c, MC_EINVAL, "mc_bfs: out is null");
    mc_bfs_job job{seed_hi, seed_lo, n_seeds, dir};
    int rc = mc_bfs_batch(c, &job, 1, min_cov, max_kmers, max_radius, out);
    if (rc) return rc;
    if (out->n == 0) return fail(c, MC_ENOSEED, "Could not find any k-mers of the target gene in the input");
    return MC_OK;
}

}  // extern "C"


// ---- the walk over several ranks' tables where they are (include/mcgpu.h mc_shard_*) -------------------------------------
namespace {
uint64_t process_token()
{
    static const uint64_t tok = [] {
        uint64_t v = 0;
        if (FILE *f = fopen("/dev/urandom", "rb")) { if (fread(&v, sizeof v, 1, f) != 1) v = 0; fclose(f); }
        v ^= ((uint64_t)getpid() << 32) ^ (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count() ^ (uint64_t)(uintptr_t)&v;
        return v ? v : 1;
    }();
    return tok;
}
constexpr uint32_t SHARD_MAGIC = 0x4D435348u;  // "MCSH"
}  // namespace

// this context's counting table, ready to be read by another walker: initialised, nothing parked, counters read
int shard_describe(mc_ctx *c, ShardWire *w, bool want_ipc)
{
    memset(w, 0, sizeof *w);
    if (!c->finalized) return fail(c, MC_ESTATE, "mc_shard_export: call mc_finalize_counts first");
    if (c->solid_external) return fail(c, MC_ESTATE, "mc_shard_export: a BFS-only context has no counting table to share");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc = by_key_ready(c);  // (the walkers of other ranks come with keys)
    if (!rc) rc = materialize(c);  // (a rank that owns nothing of the batch still offers a valid, empty table)
    if (rc) return rc;
    unsigned long long *h = c->h_scratch;
    HIPCHK(c, hipMemcpyAsync(h, c->d_ctr, 9 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const TableView t = c->view();
    w->addr = (uint64_t)(uintptr_t)c->slots;
    w->bytes = c->n_slots() * sizeof(Slot);
    w->shift = t.shift; w->rmask = t.rmask; w->n_regions = t.n_regions; w->mm_k = t.mm_k;
    w->empty = h[1];
    w->pid = (int32_t)getpid(); w->device = (int16_t)c->cfg.device; w->k = (uint8_t)c->cfg.k; w->key_mode = (uint8_t)c->cfg.key_mode;
    w->token = process_token();
    w->magic = SHARD_MAGIC;
    if (want_ipc) {
        const hipError_t e = hipIpcGetMemHandle(&w->ipc, c->slots);
        w->has_ipc = e == hipSuccess;
        if (e != hipSuccess) (void)hipGetLastError();  // (the handle still serves this process)
    }
    return MC_OK;
}

void shard_detach_locked(mc_ctx *c)
{
    (void)hipSetDevice(c->cfg.device);
    for (auto &m : c->ipc_opened) m.in_use = false;  // (closed when the next attachments do not ask for them: shard_attach_locked)
    if (c->d_shards) (void)hipFree(c->d_shards);
    c->d_shards = nullptr;
    c->h_shards.clear();
    c->shard_owner_mm_k = 0;
}

int shard_attach_locked(mc_ctx *c, const ShardWire *w, uint32_t n, uint32_t self, int by_minimizer)
{
    shard_detach_locked(c);
    c->shards_dropped = false;
    if (!c->finalized) return fail(c, MC_ESTATE, "mc_shard_attach: call mc_finalize_counts first");
    if (n == 0 || n > 512 || self >= n) return fail(c, MC_EINVAL, "mc_shard_attach: bad number of shards / own index");
    if (by_minimizer && !(c->cfg.key_mode == MC_KEY_PACKED && c->cfg.k >= SK_MIN_K))
        return fail(c, MC_EINVAL, "mc_shard_attach: keys are dealt by minimizer only where reads travel as super-k-mer records (packed keys, k >= %d)", SK_MIN_K);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    std::vector<ShardRef> refs(n);
    for (uint32_t i = 0; i < n; i++) {
        const ShardWire &x = w[i];
        if (x.magic != SHARD_MAGIC) return fail(c, MC_EINVAL, "mc_shard_attach: shard %u is not a handle of mc_shard_export", i);
        if (x.k != c->cfg.k || x.key_mode != c->cfg.key_mode) return fail(c, MC_EINVAL, "mc_shard_attach: shard %u was counted with k = %d, key mode %d", i, x.k, x.key_mode);
        Slot *slots = nullptr;
        if (i == self) {
            if (x.addr != (uint64_t)(uintptr_t)c->slots || x.token != process_token())
                return fail(c, MC_EINVAL, "mc_shard_attach: shard %u is not this context's table as it is now (export again after counting)", i);
            slots = c->slots;
        } else if (x.token == process_token()) {  // another context of this process: its pointer, through peer access when it is another device's
            slots = reinterpret_cast<Slot *>((uintptr_t)x.addr);
            if (x.device != c->cfg.device) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, c->cfg.device, x.device) != hipSuccess || !can)
                    return fail(c, MC_EHIP, "mc_shard_attach: GPU %d cannot read GPU %d's memory (no peer access)", c->cfg.device, x.device);
                const hipError_t e = hipDeviceEnablePeerAccess(x.device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(c, MC_EHIP, "mc_shard_attach: hipDeviceEnablePeerAccess: %s", hipGetErrorString(e));
                (void)hipGetLastError();
            }
        } else {
            if (!x.has_ipc) { shard_detach_locked(c); return fail(c, MC_EHIP, "mc_shard_attach: shard %u comes from another process without an IPC handle", i); }
            void *p = nullptr;
            for (auto &m : c->ipc_opened)  // (the same table as last time: its mapping is still there)
                if (!m.in_use && memcmp(&m.h, &x.ipc, sizeof x.ipc) == 0 && m.addr == x.addr && m.bytes == x.bytes) { p = m.p; m.in_use = true; break; }
            if (!p) {
                const hipError_t e = hipIpcOpenMemHandle(&p, x.ipc, hipIpcMemLazyEnablePeerAccess);
                if (e != hipSuccess) { shard_detach_locked(c); return fail(c, MC_EHIP, "mc_shard_attach: hipIpcOpenMemHandle (shard %u): %s", i, hipGetErrorString(e)); }
                c->ipc_opened.push_back(mc_ctx::IpcMap{x.ipc, p, true, x.addr, x.bytes});
            }
            slots = static_cast<Slot *>(p);
        }
        refs[i].slots = slots; refs[i].shift = x.shift; refs[i].rmask = x.rmask; refs[i].n_regions = x.n_regions; refs[i].mm_k = x.mm_k;
        refs[i].empty = x.empty;
    }
    if (hipMalloc(reinterpret_cast<void **>(&c->d_shards), n * sizeof(ShardRef)) != hipSuccess) { shard_detach_locked(c); return fail(c, MC_ENOMEM, "mc_shard_attach: out of device memory"); }
    if (hipMemcpy(c->d_shards, refs.data(), n * sizeof(ShardRef), hipMemcpyHostToDevice) != hipSuccess) { shard_detach_locked(c); return fail(c, MC_EHIP, "mc_shard_attach: upload failed"); }
    // Mappings nobody asked for this time are closed at once (kept until twice as many had gathered, a peer's table
    // that had been replaced -- grown, or given back to the driver -- stayed pinned through its mapping, up to 137 GB each).
    {
        std::vector<mc_ctx::IpcMap> keep;
        for (auto &m : c->ipc_opened) { if (m.in_use) keep.push_back(m); else (void)hipIpcCloseMemHandle(m.p); }
        c->ipc_opened.swap(keep);
    }
    c->h_shards = refs;
    c->shard_self = self;
    c->shard_owner_mm_k = by_minimizer ? c->cfg.k : 0;
    return MC_OK;
}

extern "C" {

int mc_shard_export(mc_ctx *c, mc_shard_handle *out)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!out) return fail(c, MC_EINVAL, "mc_shard_export: out is null");
    ShardWire w;
    const int rc = shard_describe(c, &w, true);
    if (rc) return rc;
    memset(out, 0, sizeof *out);
    memcpy(out, &w, sizeof w);
    return MC_OK;
}

int mc_shard_attach(mc_ctx *c, const mc_shard_handle *shards, uint32_t n_shards, uint32_t self, int by_minimizer)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!shards) return fail(c, MC_EINVAL, "mc_shard_attach: shards is null");
    if (n_shards == 0 || n_shards > 512) return fail(c, MC_EINVAL, "mc_shard_attach: bad number of shards / own index");  // (before anything is sized by it)
    std::vector<ShardWire> w(n_shards);
    for (uint32_t i = 0; i < n_shards; i++) memcpy(&w[i], &shards[i], sizeof(ShardWire));
    return shard_attach_locked(c, w.data(), n_shards, self, by_minimizer);
}

int mc_shard_detach(mc_ctx *c)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    shard_detach_locked(c);
    c->shards_dropped = false;
    return MC_OK;
}

}  // extern "C"
