// libmcgpu.so, several GPUs as one table: mc_group_*.  This unit launches no kernels; it drives the contexts of its devices
// through the counting, tokeniser and walk units (context.h).
#include <dlfcn.h>

#include <chrono>
#include <cstring>
#include <thread>

#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
// librccl is loaded at run time (RcclApi below); without its headers the library still builds, from the few declarations
// of <rccl/rccl.h> the transport uses
typedef struct ncclComm *ncclComm_t;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclUint8 = 1 } ncclDataType_t;
#endif

#include "context.h"
#include "host/reads_io.h"

// mc_group: the native counterpart of metacherchant_amd/distributed.py, for a host that is one
// process: a context per device, one host thread per device for the work, and the exchange as peer-to-peer copies --
// every (source, destination) pair at once, so that all xGMI links of a GPU are busy together, which is what an
// all-to-all over RCCL's grouped send / recv does too.  Reads are dealt to the devices in equal contiguous shares, every
// device turns its share into super-k-mer records (keys for k < 23 / hash keys) bucketed by owner, the buckets travel,
// every device counts what it owns (disjoint key sets).  For the BFS the shards' k-mers at or above the threshold are
// gathered on the first device into a BFS-only context that borrows that device's read store (read pointers refer to the
// first device's reads: the others keep none).  What the reference does instead: P threads over one shared map
// (src/io/IOUtils.java:283-315, src/io/ReadsDispatcher.java:34-53).

// RCCL, loaded when a group asks for it (MC_GROUP_TRANSPORT=rccl / MC_FLAG_GROUP_RCCL): the library is large and a process
// that counts on one GPU, or moves its buckets with peer copies, never needs it.  Types and constants from <rccl/rccl.h>.
struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    bool load(std::string *why)
    {
        if (lib) return true;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (lib) break;
        }
        if (!lib) { *why = std::string("librccl.so.1 cannot be loaded: ") + dlerror(); return false; }
#define RCCL_SYM(field, sym) field = reinterpret_cast<decltype(field)>(dlsym(lib, sym)); if (!field) { *why = std::string("librccl has no ") + sym; return false; }
        RCCL_SYM(CommInitAll, "ncclCommInitAll") RCCL_SYM(CommDestroy, "ncclCommDestroy") RCCL_SYM(GroupStart, "ncclGroupStart")
        RCCL_SYM(GroupEnd, "ncclGroupEnd") RCCL_SYM(Send, "ncclSend") RCCL_SYM(Recv, "ncclRecv") RCCL_SYM(GetErrorString, "ncclGetErrorString")
#undef RCCL_SYM
        return true;
    }
};
static RcclApi g_rccl;

struct mc_group {
    std::vector<mc_ctx *> ctx;  // one per device, in the order given
    mc_ctx *solid = nullptr;    // BFS-only context on the first device (n > 1)
    int solid_cov = -1;
    bool dirty = true;          // counts changed since the shards were gathered
    mc_config cfg{};
    std::string err;
    std::mutex mu;
    // how the buckets travel between the devices: peer-to-peer copies (every pair at once), or RCCL -- one communicator per
    // device in this process (ncclCommInitAll), the exchange as grouped ncclSend / ncclRecv, which is what an all-to-all is
    bool use_rccl = false;
    std::vector<ncclComm_t> comm;
    bool peer_all = true;       // every pair of distinct devices has peer access (else HIP stages those copies through the host)
    bool gather_reads = false;  // every device's reads are brought to the first device's store, and every record carries a pointer into it
    mc_switches sw;             // the environment switches, read by mc_group_create (switches.h)
};

namespace {

int gfail(mc_group *g, int code, const std::string &msg)
{
    if (g) g->err = msg;
    return code;
}

// runs f(rank) on one thread per rank; returns the first non-zero result
template <typename F>
int per_rank(size_t n, F &&f)
{
    std::vector<int> rc(n, 0);
    std::vector<std::thread> th;
    auto guarded = [&](size_t r) {  // (an exception must not leave a thread: std::terminate)
        try { rc[r] = f(r); } catch (const std::bad_alloc &) { rc[r] = MC_ENOMEM; } catch (...) { rc[r] = MC_EINVAL; }
    };
    for (size_t r = 1; r < n; r++) th.emplace_back([&, r] { guarded(r); });
    guarded(0);
    for (auto &t : th) t.join();
    for (int x : rc) if (x) return x;
    return MC_OK;
}

// bytes from a buffer of src's device to one of dst's (the same device: a plain device copy)
hipError_t peer_copy(void *d, const mc_ctx *dst, const void *s, const mc_ctx *src, size_t bytes, hipStream_t st)
{
    if (bytes == 0) return hipSuccess;
    if (dst->cfg.device == src->cfg.device) return hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, st);
    return hipMemcpyPeerAsync(d, dst->cfg.device, s, src->cfg.device, bytes, st);
}

}  // namespace

extern "C" {

const char *mc_group_last_error(const mc_group *g) { return g ? g->err.c_str() : g_create_err.c_str(); }

void mc_group_destroy(mc_group *g)
{
    if (!g) return;
    for (ncclComm_t cm : g->comm) if (cm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(cm);
    if (g->solid) mc_destroy(g->solid);
    for (mc_ctx *c : g->ctx) mc_destroy(c);
    delete g;
}

int mc_group_create(const mc_config *cfg, const int32_t *devices, uint32_t n_devices, mc_group **out)
{
    if (!cfg || !devices || !out || n_devices == 0 || n_devices > 64) return fail(nullptr, MC_EINVAL, "mc_group_create: bad argument");
    *out = nullptr;
    mc_group *g = new (std::nothrow) mc_group;
    if (!g) return fail(nullptr, MC_ENOMEM, "mc_group_create: out of host memory");
    g->cfg = *cfg;
    g->sw = read_switches();
    for (uint32_t r = 0; r < n_devices; r++) {
        mc_config c = *cfg;
        c.device = devices[r];
        c.capacity_hint = cfg->capacity_hint ? cfg->capacity_hint / n_devices + (1u << 20) : 0;  // owners hold equal shares of the keys
        if (n_devices > 1) c.flags |= MC_FLAG_SOLID_LIST;                                           // its solid k-mers will be exported
        mc_ctx *x = nullptr;
        const int rc = mc_create(&c, &x);
        if (rc) { mc_group_destroy(g); return rc; }
        g->ctx.push_back(x);
        // The BFS device reads its look-ahead from ITS store: the other devices' reads are brought there (group_import_reads; a file's
        // reads are tokenised there in the first place) and every device works its pointers out as if its reads sat in that store
        // -- a walk that had only the first device's reads to follow took 20 times as long at 8 devices (include/mcgpu.h
        // mc_set_read_pointers).  MC_EXCHANGE_GATHER_READS=0: the other devices' records carry no pointers.
        g->gather_reads = g->sw.group_gather_reads && n_devices > 1;
        if (n_devices > 1) (void)mc_set_read_pointers(x, g->gather_reads ? ((r == 0 ? 1 : 2) | MC_PTRS_ON_EVERY_RECORD) : (r == 0 ? 1 : 0));
    }
    // peer access between every pair of different devices (already enabled: fine).  A pair without it still works -- HIP
    // stages such copies through the host -- but at a fraction of the xGMI rate: say so once.
    for (uint32_t a = 0; a < n_devices; a++)
        for (uint32_t b = 0; b < n_devices; b++) {
            if (devices[a] == devices[b]) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, devices[a], devices[b]) != hipSuccess) can = 0;
            bool ok = false;
            if (can && hipSetDevice(devices[a]) == hipSuccess) {
                const hipError_t e = hipDeviceEnablePeerAccess(devices[b], 0);
                ok = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
            }
            (void)hipGetLastError();
            if (!ok && g->peer_all) {
                g->peer_all = false;
                fprintf(stderr, "WARN: no peer access from GPU %d to GPU %d: the exchange between them is staged through the host\n", devices[a], devices[b]);
            }
        }
    {   // transport of the exchange
        g->use_rccl = ((cfg->flags & MC_FLAG_GROUP_RCCL) != 0 || g->sw.group_transport == 1) && g->sw.group_transport != 2;
        if (g->use_rccl && n_devices > 1) {
            for (uint32_t a = 0; a < n_devices; a++)
                for (uint32_t b = a + 1; b < n_devices; b++)
                    if (devices[a] == devices[b]) { mc_group_destroy(g); return fail(nullptr, MC_EINVAL, "mc_group_create: RCCL wants every rank on a GPU of its own (GPU %d is named twice); use the peer-copy transport for shares of one GPU", devices[a]); }
            std::string why;
            if (!g_rccl.load(&why)) { mc_group_destroy(g); return fail(nullptr, MC_EINVAL, "mc_group_create: %s", why.c_str()); }
            g->comm.assign(n_devices, nullptr);
            std::vector<int> devs(devices, devices + n_devices);
            const ncclResult_t r = g_rccl.CommInitAll(g->comm.data(), (int)n_devices, devs.data());
            if (r != ncclSuccess) { mc_group_destroy(g); return fail(nullptr, MC_EHIP, "mc_group_create: ncclCommInitAll: %s", g_rccl.GetErrorString(r)); }
        } else {
            g->use_rccl = false;
        }
    }
    if (n_devices > 1) {
        mc_config c = *cfg;
        c.device = devices[0];
        c.capacity_hint = 1u << 20;
        c.flags = 0;
        const int rc = mc_create(&c, &g->solid);
        if (rc) { mc_group_destroy(g); return rc; }
    }
    *out = g;
    return MC_OK;
}

int mc_group_set_coverage_hint(mc_group *g, int min_cov)
{
    if (!g) return MC_EINVAL;
    for (mc_ctx *c : g->ctx) {
        const int rc = mc_set_coverage_hint(c, min_cov);
        if (rc) return gfail(g, rc, mc_last_error(c));
    }
    return MC_OK;
}

namespace {
// what one device brings to an exchange: its share of the reads (device pointers) and, filled on the way, what it sends and receives
struct GroupRank {
    DevBuf<uint64_t> dw, doff, send, recv;   // reads uploaded here (host batches); what goes out (records: 2 words each, or keys) and what came in
    DevBuf<uint32_t> send_p, recv_p;         // the read pointers that travel with them
    DevBuf<uint32_t> fc, recv_fc;            // binned records: a row of fine-bucket counts for every owner; the rows every source sent me
    std::vector<uint64_t> owner_off;         // owner o's piece of `send` = [owner_off[o], owner_off[o + 1])
    std::vector<uint64_t> owner_win;         // binned records: the windows of owner o's piece
    uint64_t n_recv = 0;
    const uint64_t *d_words = nullptr, *d_off = nullptr;  // the share: d_off[0 .. n_reads] index bases of d_words
    uint64_t n_reads = 0, n_bases = 0, windows = 0;       // n_bases = d_off[n_reads]; windows: k-mer occurrences, or an upper bound
    int64_t in_store = -1;                                // >= 0: the share sits in this device's read store from that word on
};

// n_words packed words of device `from`'s reads to word `at_word` of the first device's read store (where that device's pointers lead)
int group_import_reads(mc_group *g, size_t from, const uint64_t *src, uint64_t n_words, uint64_t at_word)
{
    mc_ctx *c0 = g->ctx[0];
    std::lock_guard<std::mutex> g0(c0->mu);
    if (hipSetDevice(c0->cfg.device) != hipSuccess) return MC_EHIP;
    if (at_word + n_words + 1 > c0->rs_cap_words) {
        const uint64_t fill = c0->rs_bases / 32;
        int rc = rs_reserve(c0, at_word + n_words + 1 > fill ? at_word + n_words + 1 - fill : 0);
        if (rc) return rc;
    }
    if (peer_copy(c0->rs_words + at_word, c0, src, g->ctx[from], n_words * 8, c0->stream) != hipSuccess || hipStreamSynchronize(c0->stream) != hipSuccess) return MC_EHIP;
    c0->rs_hi_bases = std::max(c0->rs_hi_bases, (at_word + n_words) * 32);
    return MC_OK;
}

// every device: its share -> records (keys) bucketed by owner; the exchange; every device counts what it owns
int group_exchange_count(mc_group *g, std::vector<GroupRank> &R)
{
    const size_t W = g->ctx.size();
    const bool sk = g->ctx[0]->sk_form;
    bool sk_batch = sk;  // this batch travels as super-k-mer records (false: as keys)
    // the binned form of the record exchange (include/mcgpu.h mc_extract_superkmers_binned_dev) where every device's table is laid
    // out for the same level-1 buckets: the sender orders an owner's records by them, and the owner's run starts at its second level
    uint32_t fine = 0;
    if (sk) {
        fine = mc_superkmer_fine_buckets(g->ctx[0], (uint32_t)W);
        for (size_t r = 1; r < W && fine; r++) if (mc_superkmer_fine_buckets(g->ctx[r], (uint32_t)W) != fine) fine = 0;
    }
    auto extract = [&](size_t r, bool as_records) -> int {
        mc_ctx *c = g->ctx[r];
        GroupRank &X = R[r];
        X.owner_off.assign(W + 1, 0);
        X.owner_win.assign(W, 0);
        if (hipSetDevice(c->cfg.device) != hipSuccess) return MC_EHIP;
        if (as_records && fine && X.fc.alloc((uint64_t)W * fine) != hipSuccess) return MC_ENOMEM;
        if (X.n_reads == 0 || X.windows == 0) {  // (a rank without reads still sends its rows: zeros)
            if (as_records && fine && (hipMemsetAsync(X.fc.p, 0, (uint64_t)W * fine * 4, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)) return MC_EHIP;
            return MC_OK;
        }
        X.send.reset();
        X.send_p.reset();
        c->extract_in_store = X.in_store;
        if (as_records) {
            const uint64_t cap = mc_superkmer_capacity(c, X.windows, X.n_reads);
            if (X.send.alloc(cap * 2) != hipSuccess || X.send_p.alloc(cap) != hipSuccess) return MC_ENOMEM;
            if (fine)
                return mc_extract_superkmers_binned_dev(c, X.d_words, X.d_off, X.n_reads, X.n_bases, (uint32_t)W, fine, X.send.p, X.send_p.p, cap, X.fc.p,
                                                        X.owner_off.data(), X.owner_win.data());
            return mc_extract_superkmers_dev(c, X.d_words, X.d_off, X.n_reads, X.n_bases, (uint32_t)W, X.send.p, X.send_p.p, cap, X.owner_off.data());
        }
        if (X.send.alloc(X.windows) != hipSuccess || X.send_p.alloc(X.windows) != hipSuccess) return MC_ENOMEM;
        // A group that deals super-k-mer records deals by minimizer (sk_owner), and the owner of a k-mer must not depend on the
        // form a batch travels in: one batch as keys dealt by the key's own hash would split a k-mer's count over two shards
        // -- each under the threshold, perhaps, and the k-mer gone from the graph.
        c->extract_by_minimizer = sk;
        return mc_extract_keys_dev(c, X.d_words, X.d_off, X.n_reads, X.n_bases, (uint32_t)W, reinterpret_cast<int64_t *>(X.send.p), X.send_p.p, X.windows,
                                   X.owner_off.data());
    };
    std::vector<uint64_t> fill(W, 0);  // (where every device's reads go, or are deemed to go, in the shared store: a second extraction starts there again)
    if (g->gather_reads) for (size_t r = 0; r < W; r++) fill[r] = mc_read_store_tell(g->ctx[r]);
    int rc = per_rank(W, [&](size_t r) -> int { return extract(r, sk); });
    if (rc == MC_EOVERFLOW && sk) {
        if (g->gather_reads) for (size_t r = 0; r < W; r++) (void)mc_read_store_seek(g->ctx[r], fill[r], 0);
        // an owner's piece overflowed (reads of low complexity share one minimizer, hence one owner): this batch travels as
        // keys instead, on every rank alike -- one record per window, counted per owner first and then packed (no piece to
        // overflow), and dealt to the SAME owners: those of the keys' minimizers
        sk_batch = false;
        for (mc_ctx *c : g->ctx) c->err.clear();
        if (g->sw.ingest_debug) fprintf(stderr, "[ingest] group: an owner's piece of the record form overflowed; this batch travels as keys, dealt by minimizer\n");
        rc = per_rank(W, [&](size_t r) -> int { return extract(r, false); });
    }
    if (rc) {
        for (mc_ctx *c : g->ctx) if (!c->err.empty()) return gfail(g, rc, c->err);
        return gfail(g, rc, "mc_group_add_reads_packed: extraction failed");
    }
    // ---- the exchange: owner d receives its piece of every rank's output, all pairs at once
    const size_t unit = sk_batch ? 16 : 8;
    const bool binned = sk_batch && fine != 0;
    if (g->use_rccl) {
        // RCCL: every device's receive buffer first, then ONE group of sends and receives over all pairs (what an all-to-all
        // with per-pair counts is), each communicator's calls on its own context's stream
        rc = per_rank(W, [&](size_t d) -> int {
            mc_ctx *c = g->ctx[d];
            if (hipSetDevice(c->cfg.device) != hipSuccess) return MC_EHIP;
            uint64_t total = 0;
            for (size_t r = 0; r < W; r++) total += R[r].owner_off[d + 1] - R[r].owner_off[d];
            R[d].n_recv = total;
            if (binned && R[d].recv_fc.alloc((uint64_t)W * fine) != hipSuccess) return MC_ENOMEM;
            if (total == 0) return MC_OK;
            return R[d].recv.alloc(total * (sk_batch ? 2 : 1)) == hipSuccess && R[d].recv_p.alloc(total) == hipSuccess ? MC_OK : MC_ENOMEM;
        });
        if (rc) return gfail(g, rc, "mc_group_add_reads_packed: no room for the received buckets");
        struct Zero { size_t d; uint64_t at, m; };
        std::vector<Zero> ptr_zero;
        ncclResult_t nr = g_rccl.GroupStart();
        std::vector<uint64_t> at(W, 0);
        for (size_t r = 0; r < W && nr == ncclSuccess; r++)       // source
            for (size_t d = 0; d < W && nr == ncclSuccess; d++) {  // owner
                const uint64_t o0 = R[r].owner_off[d], m = R[r].owner_off[d + 1] - o0;
                if (binned) {  // source r's row of counts for owner d
                    nr = g_rccl.Send(R[r].fc.p + d * fine, (size_t)fine * 4, ncclUint8, (int)d, g->comm[r], g->ctx[r]->stream);
                    if (nr == ncclSuccess) nr = g_rccl.Recv(R[d].recv_fc.p + r * fine, (size_t)fine * 4, ncclUint8, (int)r, g->comm[d], g->ctx[d]->stream);
                    if (nr != ncclSuccess) break;
                }
                if (m == 0) continue;
                nr = g_rccl.Send(reinterpret_cast<const char *>(R[r].send.p) + o0 * unit, m * unit, ncclUint8, (int)d, g->comm[r], g->ctx[r]->stream);
                if (nr == ncclSuccess) nr = g_rccl.Recv(reinterpret_cast<char *>(R[d].recv.p) + at[d] * unit, m * unit, ncclUint8, (int)r, g->comm[d], g->ctx[d]->stream);
                // (read pointers lead into the FIRST device's read store, the one the walk reads: the other devices keep none, and the
                // zeros they used to send -- a fifth of their bytes -- are filled in where they arrive)
                if (r == 0 || g->gather_reads) {  // (gather_reads: every device's reads are in that store, every record brings its pointer)
                    if (nr == ncclSuccess) nr = g_rccl.Send(R[r].send_p.p + o0, m * 4, ncclUint8, (int)d, g->comm[r], g->ctx[r]->stream);
                    if (nr == ncclSuccess) nr = g_rccl.Recv(R[d].recv_p.p + at[d], m * 4, ncclUint8, (int)r, g->comm[d], g->ctx[d]->stream);
                } else {
                    ptr_zero.push_back({d, at[d], m});
                }
                at[d] += m;
            }
        const ncclResult_t ne = g_rccl.GroupEnd();
        if (nr == ncclSuccess) nr = ne;
        for (const Zero &z : ptr_zero) {
            if (hipSetDevice(g->ctx[z.d]->cfg.device) != hipSuccess || hipMemsetAsync(R[z.d].recv_p.p + z.at, 0, z.m * 4, g->ctx[z.d]->stream) != hipSuccess)
                return gfail(g, MC_EHIP, "mc_group_add_reads_packed: clearing the pointers of pointer-less records failed");
        }
        if (nr != ncclSuccess) return gfail(g, MC_EHIP, std::string("mc_group_add_reads_packed: RCCL exchange: ") + g_rccl.GetErrorString(nr));
        rc = per_rank(W, [&](size_t d) -> int {
            mc_ctx *c = g->ctx[d];
            if (hipSetDevice(c->cfg.device) != hipSuccess) return MC_EHIP;
            return hipStreamSynchronize(c->stream) == hipSuccess ? MC_OK : MC_EHIP;
        });
        if (rc) return gfail(g, rc, "mc_group_add_reads_packed: the RCCL exchange failed");
    } else
    rc = per_rank(W, [&](size_t d) -> int {
        mc_ctx *c = g->ctx[d];
        if (hipSetDevice(c->cfg.device) != hipSuccess) return MC_EHIP;
        uint64_t total = 0;
        for (size_t r = 0; r < W; r++) total += R[r].owner_off[d + 1] - R[r].owner_off[d];
        R[d].n_recv = total;
        if (total == 0) return MC_OK;
        if (R[d].recv.alloc(total * (sk_batch ? 2 : 1)) != hipSuccess || R[d].recv_p.alloc(total) != hipSuccess) return MC_ENOMEM;
        if (binned && R[d].recv_fc.alloc((uint64_t)W * fine) != hipSuccess) return MC_ENOMEM;
        uint64_t at = 0;
        for (size_t r = 0; r < W; r++) {
            const uint64_t o0 = R[r].owner_off[d], m = R[r].owner_off[d + 1] - o0;
            if (binned && peer_copy(R[d].recv_fc.p + r * fine, c, R[r].fc.p + d * fine, g->ctx[r], (size_t)fine * 4, c->stream) != hipSuccess) return MC_EHIP;
            // (pointers: from the first device only -- they lead into its read store; the others' would be zeros)
            if (peer_copy(reinterpret_cast<char *>(R[d].recv.p) + at * unit, c, reinterpret_cast<const char *>(R[r].send.p) + o0 * unit, g->ctx[r], m * unit, c->stream) != hipSuccess ||
                (r == 0 || g->gather_reads ? peer_copy(R[d].recv_p.p + at, c, R[r].send_p.p + o0, g->ctx[r], m * 4, c->stream)
                        : (m ? hipMemsetAsync(R[d].recv_p.p + at, 0, m * 4, c->stream) : hipSuccess)) != hipSuccess)
                return MC_EHIP;
            at += m;
        }
        return hipStreamSynchronize(c->stream) == hipSuccess ? MC_OK : MC_EHIP;
    });
    if (rc) return gfail(g, rc, "mc_group_add_reads_packed: the exchange between the devices failed");
    // ---- every device counts what it owns
    rc = per_rank(W, [&](size_t d) -> int {
        if (R[d].n_recv == 0) return MC_OK;
        if (binned) {  // every source's piece is a part, in the order the pieces were received
            std::vector<uint64_t> part_off(W + 1, 0);
            uint64_t windows = 0;
            for (size_t r = 0; r < W; r++) {
                part_off[r + 1] = part_off[r] + (R[r].owner_off[d + 1] - R[r].owner_off[d]);
                windows += R[r].owner_win[d];
            }
            return mc_add_superkmers_binned_dev(g->ctx[d], R[d].recv.p, R[d].recv_p.p, R[d].n_recv, windows, fine, (uint32_t)W, part_off.data(), R[d].recv_fc.p);
        }
        return sk_batch ? mc_add_superkmers_dev(g->ctx[d], R[d].recv.p, R[d].recv_p.p, R[d].n_recv)
                  : mc_add_keys_dev(g->ctx[d], reinterpret_cast<const int64_t *>(R[d].recv.p), R[d].recv_p.p, R[d].n_recv);
    });
    if (rc) {
        for (mc_ctx *c : g->ctx) if (!c->err.empty()) return gfail(g, rc, c->err);
        return gfail(g, rc, "mc_group_add_reads_packed: counting failed");
    }
    return MC_OK;
}
}  // namespace

namespace {
// a batch of packed reads in host memory: shares up to the devices, exchange, count (the caller holds the group's lock)
int group_add_host_batch(mc_group *g, const uint64_t *words, const uint64_t *off, uint64_t n_reads)
{
    const size_t W = g->ctx.size();
    const int k = g->cfg.k;
    std::vector<GroupRank> R(W);
    int rc = per_rank(W, [&](size_t r) -> int {
        mc_ctx *c = g->ctx[r];
        const uint64_t a = n_reads * r / W, b = n_reads * (r + 1) / W;
        if (a == b) return MC_OK;
        if (hipSetDevice(c->cfg.device) != hipSuccess) return MC_EHIP;
        const uint64_t w0 = off[a] / 32, w1 = (off[b] + 31) / 32 + 1, nb = off[b] - w0 * 32;
        std::vector<uint64_t> rel(off + a, off + b + 1);
        uint64_t windows = 0;
        for (uint64_t i = 0; i < b - a; i++) {
            const uint64_t len = rel[i + 1] - rel[i];
            if (len >= (uint64_t)k) windows += len - (uint64_t)k + 1;
        }
        for (auto &x : rel) x -= w0 * 32;
        if (R[r].dw.alloc(w1 - w0) != hipSuccess || R[r].doff.alloc(b - a + 1) != hipSuccess) return MC_ENOMEM;
        // (through the context's pinned staging buffers: a pageable copy runs at a third of the link's rate)
        if (h2d_fast(c, R[r].dw.p, words + w0, (w1 - w0) * 8) != MC_OK || h2d_fast(c, R[r].doff.p, rel.data(), (b - a + 1) * 8) != MC_OK) return MC_EHIP;
        R[r].d_words = R[r].dw.p; R[r].d_off = R[r].doff.p;
        R[r].n_reads = b - a; R[r].n_bases = nb; R[r].windows = windows;
        return MC_OK;
    });
    if (rc) {
        for (mc_ctx *c : g->ctx) if (!c->err.empty()) return gfail(g, rc, c->err);
        return gfail(g, rc, "mc_group_add_reads_packed: the reads did not reach the devices");
    }
    uint64_t end_word = 0;
    if (g->gather_reads) {
        // the shares one behind the other in the first device's store: its own where its extraction will append it, the others'
        // copied there from their devices; every other device is told where its share sits (its pointers lead there)
        mc_ctx *c0 = g->ctx[0];
        uint64_t at = 0;
        {
            std::lock_guard<std::mutex> g0(c0->mu);
            at = c0->rs_end() / 32;
        }
        std::vector<uint64_t> pos(W + 1, at);
        for (size_t r = 0; r < W; r++) pos[r + 1] = pos[r] + (R[r].n_reads ? (R[r].n_bases + 31) / 32 + 1 : 0);
        end_word = pos[W];
        if ((rc = mc_read_store_seek(c0, pos[0] * 32, end_word * 32 + 64)) != MC_OK) return gfail(g, rc, c0->err);
        rc = per_rank(W, [&](size_t r) -> int {
            if (r == 0 || R[r].n_reads == 0) return MC_OK;
            int x = group_import_reads(g, r, R[r].dw.p, (R[r].n_bases + 31) / 32 + 1, pos[r]);
            return x ? x : mc_read_store_seek(g->ctx[r], pos[r] * 32, 0);
        });
        if (rc) {
            for (mc_ctx *c : g->ctx) if (!c->err.empty()) return gfail(g, rc, c->err);
            return gfail(g, rc, "mc_group_add_reads_packed: the reads did not reach the first device's store");
        }
    }
    rc = group_exchange_count(g, R);
    if (g->gather_reads && rc == MC_OK && (rc = mc_read_store_seek(g->ctx[0], end_word * 32, 0)) != MC_OK) return gfail(g, rc, g->ctx[0]->err);  // (the next batch goes behind all of them)
    return rc;
}
}  // namespace

int mc_group_add_reads_packed(mc_group *g, const uint64_t *words, const uint64_t *off, uint64_t n_reads)
{
    if (!g) return MC_EINVAL;
    std::lock_guard<std::mutex> lk(g->mu);
    if ((!words || !off) && n_reads) return gfail(g, MC_EINVAL, "mc_group_add_reads_packed: null pointer");
    if (n_reads == 0) return MC_OK;
    g->dirty = true;
    if (g->ctx.size() == 1) {
        const int rc = mc_add_reads_packed(g->ctx[0], words, off, n_reads);
        return rc ? gfail(g, rc, mc_last_error(g->ctx[0])) : MC_OK;
    }
    return group_add_host_batch(g, words, off, n_reads);
}

int mc_group_add_reads_file(mc_group *g, const char *path, uint64_t *n_reads)
{
    if (!g) return MC_EINVAL;
    if (n_reads) *n_reads = 0;
    if (!path) return gfail(g, MC_EINVAL, "mc_group_add_reads_file: null path");
    if (g->ctx.size() == 1) {
        const int rc = mc_add_reads_file(g->ctx[0], path, n_reads);
        return rc ? gfail(g, rc, mc_last_error(g->ctx[0])) : MC_OK;
    }
    try {
        // Batches of 2^24 reads per device (2.5 G bases of 150-base reads: 0.6 GB of host memory per device): every batch is
        // one exchange and one counting run on every device, and a counting run rewrites the device's whole table -- with
        // 2^20 reads a batch, as before, a billion reads meant 119 rewrites of a 100 GB-class table per device.
        const uint64_t per_dev = g->sw.group_batch_reads;
        int rc = MC_OK;
        // Uncompressed FASTA / FASTQ: tokenised on the FIRST device (csrc/tokenizer.h, chunk i + 1 crossing PCIe while chunk i
        // is tokenised), into its read store -- the one the walk reads --; when W x per_dev reads have gathered, or the file
        // ends, the other devices fetch their shares of the packed reads from it (device to device) and the batch is exchanged
        // and counted.  A chunk the device declines goes through the host reader like any other file.
        mch::PlainReadsFile f;
        if (!g->sw.tokenizer_host && g->ctx[0]->rs_enabled && mch::map_plain_reads(path, &f)) {
            std::lock_guard<std::mutex> lk(g->mu);
            g->dirty = true;
            mc_ctx *c0 = g->ctx[0];
            const size_t W = g->ctx.size();
            const auto cuts = mch::plain_chunks(f, g->sw.tokenizer_chunk_bytes);
            uint64_t total = 0, n_flushes = 0;
            // the reads gathered in `pend` so far: shares to the devices, exchange, count; the store then ends behind them
            auto flush = [&](TokPending &P) -> int {
                if (P.reads == 0) { P.base_word = -1; P.bases = 0; return MC_OK; }
                n_flushes++;
                const uint64_t n = P.reads, base_word = (uint64_t)P.base_word;
                std::vector<uint64_t> cut_off(W + 1, 0);  // base offset (relative to the batch) of every share's first read
                {
                    std::lock_guard<std::mutex> g0(c0->mu);
                    if (hipSetDevice(c0->cfg.device) != hipSuccess) return gfail(g, MC_EHIP, "mc_group_add_reads_file: hipSetDevice");
                    for (size_t r = 0; r <= W; r++)
                        if (hipMemcpyAsync(&cut_off[r], P.off.p + n * r / W, 8, hipMemcpyDeviceToHost, c0->stream) != hipSuccess) return gfail(g, MC_EHIP, "mc_group_add_reads_file: copy failed");
                    if (hipStreamSynchronize(c0->stream) != hipSuccess) return gfail(g, MC_EHIP, "mc_group_add_reads_file: copy failed");
                }
                std::vector<GroupRank> R(W);
                int frc = per_rank(W, [&](size_t r) -> int {
                    mc_ctx *c = g->ctx[r];
                    const uint64_t a = n * r / W, b = n * (r + 1) / W;
                    if (a == b) return MC_OK;
                    GroupRank &X = R[r];
                    X.n_reads = b - a;
                    X.n_bases = cut_off[r + 1];
                    X.windows = cut_off[r + 1] - cut_off[r];  // (an upper bound: a window per base)
                    if (r == 0) {  // in place: the share is where the walk will read it
                        X.d_words = c0->rs_words + base_word;
                        X.d_off = P.off.p;
                        X.in_store = (int64_t)base_word;
                        return MC_OK;
                    }
                    // the words [w0, w1] of the share and its offsets come over; d_words is handed on as if it held the batch from
                    // its first word (the offsets stay relative to the batch: nothing below w0 is looked at)
                    if (hipSetDevice(c->cfg.device) != hipSuccess) return MC_EHIP;
                    // (with 512 words before the share's first: the extract kernels load whole tiles, up to 8191 bases ahead of it)
                    const uint64_t w0 = std::max<uint64_t>(cut_off[r] / 32, 512) - 512, w1 = (cut_off[r + 1] + 31) / 32 + 1;
                    if (X.dw.alloc(w1 - w0) != hipSuccess || X.doff.alloc(b - a + 1) != hipSuccess) return MC_ENOMEM;
                    if (peer_copy(X.dw.p, c, c0->rs_words + base_word + w0, c0, (w1 - w0) * 8, c->stream) != hipSuccess ||
                        peer_copy(X.doff.p, c, P.off.p + a, c0, (b - a + 1) * 8, c->stream) != hipSuccess ||
                        hipStreamSynchronize(c->stream) != hipSuccess)
                        return MC_EHIP;
                    X.d_words = X.dw.p - w0;
                    X.d_off = X.doff.p;
                    // (the share sits in the first device's store: batch position p is store position base_word * 32 + p, which is
                    // what this device's pointers come to when its -- deemed -- fill stands at the share's first word)
                    if (g->gather_reads) return mc_read_store_seek(c, (base_word + cut_off[r] / 32) * 32, 0);
                    return MC_OK;
                });
                if (frc) return gfail(g, frc, "mc_group_add_reads_file: the shares did not reach the devices");
                frc = group_exchange_count(g, R);
                {   // the batch's reads stay in the first device's store, whoever counted them
                    std::lock_guard<std::mutex> g0(c0->mu);
                    c0->rs_bases = std::max<uint64_t>(c0->rs_bases, (base_word + (P.bases + 31) / 32) * 32);
                }
                P.reads = P.bases = 0;
                P.base_word = -1;
                return frc;
            };
            FileChunkOps ops;
            ops.who = "mc_group_add_reads_file";
            ops.flush = flush;
            ops.batch_reads = W * per_dev;
            ops.host_batch = [&](mch::PackedBatch &b) { return b.n_reads() ? group_add_host_batch(g, b.words.data(), b.offsets.data(), b.n_reads()) : MC_OK; };
            ops.after_chunk = [&](size_t, size_t, TokPending &P) { return P.reads >= W * per_dev ? flush(P) : MC_OK; };
            ops.ctx_failed = [&](int code) { return gfail(g, code, c0->err); };
            rc = tokenize_file_chunks(c0, f, cuts, ops, &total);
            if (rc != MC_OK) return rc;
            if (g->sw.ingest_debug)
                fprintf(stderr, "[ingest] group: %zu chunk(s) tokenised on device %d, %llu reads in %llu exchange(s) over %zu devices\n", cuts.size(), c0->cfg.device,
                        (unsigned long long)total, (unsigned long long)n_flushes, W);
            if (n_reads) *n_reads = total;
            return MC_OK;
        }
        const uint64_t n = mch::load_reads_file(path, g->ctx.size() * per_dev, [&](mch::PackedBatch &b) {
            if (rc == MC_OK) rc = mc_group_add_reads_packed(g, b.words.data(), b.offsets.data(), b.n_reads());
        });
        if (rc != MC_OK) return rc;
        if (n_reads) *n_reads = n;
        return MC_OK;
    } catch (const mch::Error &e) {
        return gfail(g, MC_EINVAL, e.what());
    } catch (const std::bad_alloc &) {
        return gfail(g, MC_ENOMEM, "mc_group_add_reads_file: out of host memory");
    }
}

int mc_group_finalize_counts(mc_group *g, uint64_t *n_distinct)
{
    if (!g) return MC_EINVAL;
    uint64_t total = 0;
    for (mc_ctx *c : g->ctx) {
        uint64_t n = 0;
        const int rc = mc_finalize_counts(c, &n);
        if (rc) return gfail(g, rc, mc_last_error(c));
        total += n;  // owners are disjoint
    }
    if (n_distinct) *n_distinct = total;
    return MC_OK;
}

int mc_group_get_stats(mc_group *g, mc_stats *out)
{
    if (!g || !out) return MC_EINVAL;
    mc_stats t{};
    for (mc_ctx *c : g->ctx) {
        mc_stats s{};
        const int rc = mc_get_stats(c, &s);
        if (rc) return gfail(g, rc, mc_last_error(c));
        t.windows += s.windows; t.count_launches += s.count_launches; t.table_slots += s.table_slots; t.table_bytes += s.table_bytes;
        t.grows += s.grows; t.spill_keys += s.spill_keys; t.solid_kmers += s.solid_kmers; t.solid_sweeps += s.solid_sweeps;
        t.solid_list_builds += s.solid_list_builds;
        t.long_runs += s.long_runs;
        t.binned_runs += s.binned_runs;
        t.dup_keys += s.dup_keys; t.dup_checks += s.dup_checks; t.dup_ms = std::max(t.dup_ms, s.dup_ms); t.dup_unchecked |= s.dup_unchecked;
        t.left_bins = std::max(t.left_bins, s.left_bins);
        t.count_ms = std::max(t.count_ms, s.count_ms); t.count_total_ms = std::max(t.count_total_ms, s.count_total_ms);
        t.p1_ms = std::max(t.p1_ms, s.p1_ms); t.p2_ms = std::max(t.p2_ms, s.p2_ms); t.p3_ms = std::max(t.p3_ms, s.p3_ms);
    }
    *out = t;
    return MC_OK;
}

int mc_group_bfs_batch(mc_group *g, const mc_bfs_job *jobs, uint32_t n_jobs, int min_cov, int64_t max_kmers, int64_t max_radius,
                       mc_bfs_result *out)
{
    if (!g) return MC_EINVAL;
    std::lock_guard<std::mutex> lk(g->mu);
    const size_t W = g->ctx.size();
    if (W == 1) {
        const int rc = mc_bfs_batch(g->ctx[0], jobs, n_jobs, min_cov, max_kmers, max_radius, out);
        return rc ? gfail(g, rc, mc_last_error(g->ctx[0])) : MC_OK;
    }
    // ---- the walk reads every device's counting table where it is (round 4): the first context gets the other tables' addresses
    // (peer access; the same device for shares of one GPU) and looks a k-mer up in its owner's table.  No export, no copy of
    // the solid k-mers, no second table -- and what made configs[3] impossible: 5 G gathered solid k-mers do not fit beside
    // rank 0's counting table.  MC_GROUP_WALK=gather keeps round 3's way (and a group without peer
    // access between all its devices has no other).
    if (!g->sw.group_walk_gather && g->peer_all) {
        mc_ctx *c0 = g->ctx[0];
        const bool dbg = g->sw.ingest_debug;
        const auto t_0 = std::chrono::steady_clock::now();
        if (g->dirty || !c0->d_shards) {
            std::vector<ShardWire> w(W);
            int grc = per_rank(W, [&](size_t r) -> int {
                std::lock_guard<std::mutex> cl(g->ctx[r]->mu);
                return shard_describe(g->ctx[r], &w[r], false);
            });
            if (grc) {
                for (mc_ctx *c : g->ctx) if (!c->err.empty()) return gfail(g, grc, c->err);
                return gfail(g, grc, "mc_group_bfs_batch: a device's table could not be shared");
            }
            std::lock_guard<std::mutex> cl(c0->mu);
            grc = shard_attach_locked(c0, w.data(), (uint32_t)W, 0, c0->sk_form ? 1 : 0);
            if (grc) return gfail(g, grc, c0->err);
            g->dirty = false;
            g->solid_cov = -1;
        }
        const auto t_1 = std::chrono::steady_clock::now();
        const int rc = mc_bfs_batch(c0, jobs, n_jobs, min_cov, max_kmers, max_radius, out);
        if (dbg) fprintf(stderr, "[walk] group: tables described and attached in %.2f ms, %u walk(s) in %.2f ms\n", std::chrono::duration<double, std::milli>(t_1 - t_0).count(),
                         n_jobs, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_1).count());
        return rc ? gfail(g, rc, mc_last_error(c0)) : MC_OK;
    }
    if (g->dirty || g->solid_cov != min_cov) {
        // ---- gather: every shard's (key, count, pointer) with count >= min_cov, side by side on the first device.  The
        // shards are exported on all devices at once; the copies are then issued on the first device's stream with that
        // device current, and waited for once.
        std::vector<uint64_t> n(W, 0);
        struct Shard { DevBuf<int64_t> k; DevBuf<int16_t> c; DevBuf<uint32_t> p; uint64_t got = 0; };
        std::vector<Shard> sh(W);
        int grc = per_rank(W, [&](size_t r) -> int {
            mc_ctx *c = g->ctx[r];
            if (hipSetDevice(c->cfg.device) != hipSuccess) return MC_EHIP;
            int rc = mc_export_dev(c, min_cov, nullptr, nullptr, nullptr, 0, &n[r]);
            if (rc || n[r] == 0) return rc;
            if (sh[r].k.alloc(n[r]) != hipSuccess || sh[r].c.alloc(n[r]) != hipSuccess || sh[r].p.alloc(n[r]) != hipSuccess) return MC_ENOMEM;
            return mc_export_dev(c, min_cov, sh[r].k.p, sh[r].c.p, sh[r].p.p, n[r], &sh[r].got);
        });
        if (grc) {
            for (mc_ctx *c : g->ctx) if (!c->err.empty()) return gfail(g, grc, c->err);
            return gfail(g, grc, "mc_group_bfs_batch: exporting the shards failed");
        }
        uint64_t total = 0;
        for (size_t r = 0; r < W; r++) total += sh[r].got;
        mc_ctx *c0 = g->ctx[0];
        if (hipSetDevice(c0->cfg.device) != hipSuccess) return gfail(g, MC_EHIP, "hipSetDevice failed");
        DevBuf<int64_t> all_k;
        DevBuf<int16_t> all_c;
        DevBuf<uint32_t> all_p;
        if (all_k.alloc(total) != hipSuccess || all_c.alloc(total) != hipSuccess || all_p.alloc(total) != hipSuccess)
            return gfail(g, MC_ENOMEM, "mc_group_bfs_batch: no room for the gathered shards");
        uint64_t at = 0;
        for (size_t r = 0; r < W; r++) {
            const uint64_t got = sh[r].got;
            if (got == 0) continue;
            if (peer_copy(all_k.p + at, c0, sh[r].k.p, g->ctx[r], got * 8, c0->stream) != hipSuccess || peer_copy(all_c.p + at, c0, sh[r].c.p, g->ctx[r], got * 2, c0->stream) != hipSuccess ||
                peer_copy(all_p.p + at, c0, sh[r].p.p, g->ctx[r], got * 4, c0->stream) != hipSuccess)
                return gfail(g, MC_EHIP, "mc_group_bfs_batch: gathering the shards failed (peer copy)");
            at += got;
        }
        if (hipStreamSynchronize(c0->stream) != hipSuccess) return gfail(g, MC_EHIP, "mc_group_bfs_batch: gathering the shards failed (peer copy)");
        if (hipSetDevice(c0->cfg.device) != hipSuccess) return gfail(g, MC_EHIP, "hipSetDevice failed");
        int rc = mc_clear(g->solid);
        if (!rc) rc = mc_share_read_store(g->solid, c0);
        uint64_t kept = 0;
        if (!rc) rc = mc_solid_from_pairs_dev(g->solid, all_k.p, all_c.p, all_p.p, at, min_cov, &kept);
        if (rc) return gfail(g, rc, mc_last_error(g->solid));
        g->solid_cov = min_cov;
        g->dirty = false;
    }
    const int rc = mc_bfs_batch(g->solid, jobs, n_jobs, min_cov, max_kmers, max_radius, out);
    return rc ? gfail(g, rc, mc_last_error(g->solid)) : MC_OK;
}

}  // extern "C"
