// libmcgpu.so, the .kmers.bin unit: the table as 10-byte records on the device (include/mcgpu.h mc_kmers_encode_dev, mc_kmers_decode_dev)
// and streamed to and from a file (mc_save_kmers_gpu, mc_load_kmers_gpu; src/io/IOUtils.java:39-65 printKmers, :94-126 loadKmers,
// src/io/KmersLoadWorker.java:9-23).  mcgpu.hip's mc_save_kmers / mc_load_kmers are the host loops these are compared with.
// context.h lists the other units.
//
// A record is the int64 key big-endian, then the int16 value big-endian.  What counts as a key of the table is what k_export (mcgpu.hip)
// counts at min_cov = 0: a slot whose key is not EMPTY_KEY and which is not a shadow slot of the key join (device_types.h dup_is_shadow);
// its value is min(count, 32767); every key adds one to hist[value]; it becomes a record when value > threshold.  The key that equals
// EMPTY_KEY is counted out of band (d_ctr[1], hash modes): its histogram entry is added by the count sweep, its record is appended by
// the host behind the last slot's, as mc_export_dev appends its pair.
//
// The encoder.  A TILE is 2048 consecutive slots (32 KB), a wave of the workgroup owns 512 consecutive ones of them as 8 rows of 64.
//   k_kb_count   sweep 1: per tile the number of records, and the histogram.  Values 1 and 2 (nearly all of a real table) are counted
//                by ballots into two wave-uniform registers and reach LDS once per wave at the end; other values below KB_HIST_LDS go
//                to the workgroup's LDS bins (4 KB, flushed once: small enough for eight workgroups to share a CU), the rare ones above straight
//                to the 64-bit global bins.
//   (tok_scan)   the exclusive scan of the tile counts, reads_file.hip's: tile_off[t] = records before tile t.  With it the host knows
//                how many bytes any range of tiles produces, and the file path cuts its chunks by that.
//   k_kb_write   sweep 2 over a range of tiles: a tile's records are compacted in slot order (a count per wave and row in LDS and a scan
//                of those 32 counts: an LDS cursor, as k_export has it, would order the waves by arrival) and laid out in LDS as the
//                bytes of the file, shifted by two bytes when the slice starts in the middle of a dword of the output.  The slice
//                then leaves as whole dwords, 256 B a wave instruction; only a first or last halfword that shares its dword with the
//                neighbouring slice is a 16-bit store, so two tiles never store to one dword with a dword store.  An empty tile stores
//                nothing.  The output is a function of the table alone: two calls give the same bytes.
// The decoder.
//   k_kb_decode  a tile of 2048 records comes into LDS as 16-byte loads, a lane decodes eight of them (halfword reads, one 64-bit
//                byte swap), the ones with count > freq_threshold (signed) are compacted in LDS, the tile takes its slice of the
//                output with one global atomic, keys leave as 8-byte stores and counts as dwords (first / last halfword as above).
//                The order of the tiles in the output is the order of their atomics: free, addAndBound commutes.
// No loop depends on another workgroup; every index is bounded by the tile or checked against the buffer's size.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <condition_variable>
#include <thread>

#include "context.h"

namespace {

constexpr int KB_THREADS = 256, KB_WAVES = KB_THREADS / 64, KB_ROWS = 8;
constexpr int KB_WAVE_SLOTS = KB_ROWS * 64, KB_TILE = KB_THREADS * KB_ROWS;  // slots (records, in the decoder) of a wave and of a tile
constexpr int KB_RECORD = 10;                                                // bytes
constexpr int KB_HIST_LDS = 1024;                                            // bins kept in LDS
constexpr int KB_HIST_BINS = 32768;
constexpr int KB_MAX_GRID = 2048;
static_assert(KB_WAVES * KB_ROWS == 32, "the scan of a tile's counts is half a wave wide");

struct KbItem {
    uint64_t key;
    int value;
    bool live;
};

// slot `at` as the exports see it
__device__ __forceinline__ KbItem kb_item(const Slot *__restrict__ slots, uint64_t n_slots, uint64_t at, const DupSet &dq)
{
    KbItem it{EMPTY_KEY, 0, false};
    if (at < n_slots) {
        const uint4 raw = *reinterpret_cast<const uint4 *>(slots + at);
        it.key = ((uint64_t)raw.y << 32) | raw.x;
        it.value = raw.z > 32767u ? 32767 : (int)raw.z;
        it.live = it.key != EMPTY_KEY && !dup_is_shadow(dq, it.key, at);
    }
    return it;
}

// exclusive scan of the 32 counts of a tile (row j of wave w at w * KB_ROWS + j) by every wave on its own; *total: their sum
__device__ __forceinline__ uint32_t kb_scan32(const uint32_t *cnt, uint32_t lane, uint32_t *total)
{
    const uint32_t own = lane < 32 ? cnt[lane] : 0u;
    uint32_t incl = own;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
        const uint32_t below = __shfl_up(incl, o);
        if ((int)lane >= o) incl += below;
    }
    *total = __shfl(incl, 31);
    return incl - own;
}

// hist == nullptr: no histogram.  n_live += keys in the slots.  (A workgroup's LDS bins are 32-bit: it sees n_slots / gridDim.x slots.)
__global__ void __launch_bounds__(KB_THREADS) k_kb_count(const Slot *__restrict__ slots, uint64_t n_slots, int threshold, DupSet dq,
                                                         uint32_t *__restrict__ tile_counts, unsigned long long *hist,
                                                         unsigned long long *n_live, const unsigned long long *__restrict__ empty_cnt)
{
    __shared__ uint32_t lhist[KB_HIST_LDS];
    __shared__ uint32_t wrecs[KB_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (uint32_t i = tid; i < KB_HIST_LDS; i += KB_THREADS) lhist[i] = 0;
    __syncthreads();
    unsigned long long live = 0;
    uint32_t ones = 0, twos = 0;  // the same in every lane of the wave
    const uint64_t n_tiles = (n_slots + KB_TILE - 1) / KB_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        KbItem it[KB_ROWS];
#pragma unroll
        for (int j = 0; j < KB_ROWS; j++) it[j] = kb_item(slots, n_slots, tile * KB_TILE + w * KB_WAVE_SLOTS + j * 64 + lane, dq);
        uint32_t recs = 0;
#pragma unroll
        for (int j = 0; j < KB_ROWS; j++) {
            live += it[j].live ? 1u : 0u;
            recs += (uint32_t)__popcll(__ballot(it[j].live && it[j].value > threshold));
            if (hist) {
                ones += (uint32_t)__popcll(__ballot(it[j].live && it[j].value == 1));
                twos += (uint32_t)__popcll(__ballot(it[j].live && it[j].value == 2));
                if (it[j].live && it[j].value != 1 && it[j].value != 2) {
                    if (it[j].value < KB_HIST_LDS) atomicAdd(&lhist[it[j].value], 1u);
                    else atomicAdd(hist + it[j].value, 1ull);
                }
            }
        }
        if (lane == 0) wrecs[w] = recs;
        __syncthreads();
        if (tid == 0) {
            uint32_t sum = 0;
#pragma unroll
            for (int x = 0; x < KB_WAVES; x++) sum += wrecs[x];
            tile_counts[tile] = sum;
        }
        __syncthreads();
    }
    if (hist) {
        if (lane == 0) {
            if (ones) atomicAdd(&lhist[1], ones);
            if (twos) atomicAdd(&lhist[2], twos);
        }
        __syncthreads();
        for (uint32_t i = tid; i < KB_HIST_LDS; i += KB_THREADS)
            if (lhist[i]) atomicAdd(hist + i, (unsigned long long)lhist[i]);
        if (blockIdx.x == 0 && tid == 0) {  // the key that equals EMPTY_KEY
            const unsigned long long ec = *empty_cnt;
            if (ec) atomicAdd(hist + (ec > 32767ull ? 32767ull : ec), 1ull);
        }
    }
    wave_add_ull(n_live, live);
}

// the tiles [tile_begin, tile_end); rec_base = tile_off[tile_begin]: `out` starts with the first record of tile_begin.  out_bytes: the
// buffer's size, a multiple of 2 (the host has checked that the records fit; no store goes beyond it whatever the table holds)
__global__ void __launch_bounds__(KB_THREADS) k_kb_write(const Slot *__restrict__ slots, uint64_t n_slots, int threshold, DupSet dq,
                                                         const unsigned long long *__restrict__ tile_off, uint64_t tile_begin, uint64_t tile_end,
                                                         unsigned long long rec_base, uint8_t *__restrict__ out, uint64_t out_bytes)
{
    __shared__ __attribute__((aligned(16))) uint8_t img[KB_TILE * KB_RECORD + 4];  // the slice as it will be in the file, behind 0 or 2 bytes
    __shared__ uint32_t cnt[KB_WAVES * KB_ROWS];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (uint64_t tile = tile_begin + blockIdx.x; tile < tile_end; tile += gridDim.x) {
        KbItem it[KB_ROWS];
#pragma unroll
        for (int j = 0; j < KB_ROWS; j++) it[j] = kb_item(slots, n_slots, tile * KB_TILE + w * KB_WAVE_SLOTS + j * 64 + lane, dq);
        unsigned long long m[KB_ROWS];
#pragma unroll
        for (int j = 0; j < KB_ROWS; j++) {
            m[j] = __ballot(it[j].live && it[j].value > threshold);
            if (lane == 0) cnt[w * KB_ROWS + j] = (uint32_t)__popcll(m[j]);
        }
        __syncthreads();
        uint32_t n;
        const uint32_t before = kb_scan32(cnt, lane, &n);
        if (n) {  // (the same in every wave)
            const uint64_t byte0 = (uint64_t)KB_RECORD * (tile_off[tile] - rec_base);
            const uint32_t pad = (uint32_t)byte0 & 2u;
#pragma unroll
            for (int j = 0; j < KB_ROWS; j++) {
                const uint32_t base = __shfl(before, (int)(w * KB_ROWS + j));
                if (it[j].live && it[j].value > threshold) {
                    const uint32_t i = base + (uint32_t)__popcll(m[j] & ((1ull << lane) - 1));
                    const uint64_t be = __builtin_bswap64(it[j].key);
                    uint16_t *p = reinterpret_cast<uint16_t *>(img + pad + KB_RECORD * i);
                    p[0] = (uint16_t)be;
                    p[1] = (uint16_t)(be >> 16);
                    p[2] = (uint16_t)(be >> 32);
                    p[3] = (uint16_t)(be >> 48);
                    p[4] = __builtin_bswap16((uint16_t)it[j].value);
                }
            }
            __syncthreads();
            const uint32_t len = pad + KB_RECORD * n, n_dw = (len + 3) >> 2;
            const uint64_t dw0 = (byte0 - pad) >> 2;  // the output's dword that holds the slice's first byte
            const uint32_t *src = reinterpret_cast<const uint32_t *>(img);
            for (uint32_t d = tid; d < n_dw; d += KB_THREADS) {
                const uint32_t v = src[d];
                const uint64_t at = (dw0 + d) << 2;
                if (d == 0 && pad) {  // the dword's low half is the slice before
                    if (at + 4 <= out_bytes) *reinterpret_cast<uint16_t *>(out + at + 2) = (uint16_t)(v >> 16);
                } else if (d == n_dw - 1 && (len & 2u)) {  // its high half the slice behind
                    if (at + 2 <= out_bytes) *reinterpret_cast<uint16_t *>(out + at) = (uint16_t)v;
                } else if (at + 4 <= out_bytes) {
                    *reinterpret_cast<uint32_t *>(out + at) = v;
                }
            }
        }
        __syncthreads();  // (img and cnt serve the next tile)
    }
}

// in: n_records records, 16-byte aligned; keys 8-byte, counts 4-byte aligned, n_records entries each; *cursor: 0 before, the number kept after
__global__ void __launch_bounds__(KB_THREADS) k_kb_decode(const uint8_t *__restrict__ in, uint64_t n_records, int freq_threshold,
                                                          int64_t *__restrict__ keys, int16_t *__restrict__ counts, unsigned long long *cursor)
{
    // the tile's records; then, in the same bytes, the kept keys [0, 16 KB) and their counts behind 0 or 1 halfword
    constexpr uint32_t COUNTS_AT = KB_TILE * 8;
    __shared__ __attribute__((aligned(16))) uint8_t img[KB_TILE * KB_RECORD + 16];
    __shared__ uint32_t cnt[KB_WAVES * KB_ROWS];
    __shared__ unsigned long long gbase_s;
    static_assert(COUNTS_AT + (KB_TILE + 1) * 2 <= sizeof img, "keys and counts fit where the records were");
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint64_t n_tiles = (n_records + KB_TILE - 1) / KB_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t rec0 = tile * KB_TILE;
        const uint32_t n_rec = (uint32_t)(n_records - rec0 < (uint64_t)KB_TILE ? n_records - rec0 : (uint64_t)KB_TILE);
        const uint8_t *src = in + rec0 * KB_RECORD;  // (16-byte aligned: a tile is 20480 bytes)
        const uint32_t n_bytes = n_rec * KB_RECORD, n16 = n_bytes >> 4;
        for (uint32_t q = tid; q < n16; q += KB_THREADS) reinterpret_cast<uint4 *>(img)[q] = reinterpret_cast<const uint4 *>(src)[q];
        if (tid < ((n_bytes & 15u) >> 1))  // (the input ends inside a 16-byte group)
            reinterpret_cast<uint16_t *>(img)[n16 * 8 + tid] = reinterpret_cast<const uint16_t *>(src)[n16 * 8 + tid];
        __syncthreads();
        uint64_t key[KB_ROWS];
        int16_t val[KB_ROWS];
        unsigned long long m[KB_ROWS];
#pragma unroll
        for (int j = 0; j < KB_ROWS; j++) {
            const uint32_t r = w * KB_WAVE_SLOTS + j * 64 + lane;
            bool take = false;
            key[j] = 0;
            val[j] = 0;
            if (r < n_rec) {
                const uint16_t *p = reinterpret_cast<const uint16_t *>(img + KB_RECORD * r);
                const uint64_t be = (uint64_t)p[0] | ((uint64_t)p[1] << 16) | ((uint64_t)p[2] << 32) | ((uint64_t)p[3] << 48);
                key[j] = __builtin_bswap64(be);
                val[j] = (int16_t)__builtin_bswap16(p[4]);
                take = (int)val[j] > freq_threshold;
            }
            m[j] = __ballot(take);
            if (lane == 0) cnt[w * KB_ROWS + j] = (uint32_t)__popcll(m[j]);
        }
        __syncthreads();  // (the records are read: their bytes are free)
        uint32_t n;
        const uint32_t before = kb_scan32(cnt, lane, &n);
        if (tid == 0 && n) gbase_s = atomicAdd(cursor, (unsigned long long)n);
        __syncthreads();
        if (n) {  // (the same in every wave)
            const unsigned long long gbase = gbase_s;
            const uint32_t odd = (uint32_t)gbase & 1u;  // the slice of the counts starts in the middle of a dword
            uint64_t *lkeys = reinterpret_cast<uint64_t *>(img);
            uint16_t *lcounts = reinterpret_cast<uint16_t *>(img + COUNTS_AT);
#pragma unroll
            for (int j = 0; j < KB_ROWS; j++) {
                const uint32_t base = __shfl(before, (int)(w * KB_ROWS + j));
                if ((m[j] >> lane) & 1ull) {
                    const uint32_t i = base + (uint32_t)__popcll(m[j] & ((1ull << lane) - 1));
                    lkeys[i] = key[j];
                    lcounts[odd + i] = (uint16_t)val[j];
                }
            }
            __syncthreads();
            for (uint32_t i = tid; i < n; i += KB_THREADS) keys[gbase + i] = (int64_t)lkeys[i];
            const uint32_t len = odd + n, n_dw = (len + 1) >> 1;  // halfwords, dwords
            int16_t *dst = counts + (gbase - odd);
            const uint32_t *srcw = reinterpret_cast<const uint32_t *>(lcounts);
            for (uint32_t d = tid; d < n_dw; d += KB_THREADS) {
                const uint32_t v = srcw[d];
                if (d == 0 && odd) dst[1] = (int16_t)(v >> 16);
                else if (d == n_dw - 1 && (len & 1u)) dst[2 * d] = (int16_t)v;
                else *reinterpret_cast<uint32_t *>(dst + 2 * d) = v;
            }
        }
        __syncthreads();  // (img, cnt and gbase_s serve the next tile)
    }
}

// ------------------------------------------------------------------------------------------ host

// what sweep 1 left (the caller holds c->mu and has set the device)
struct KbSweep {
    DevBuf<uint32_t> tile_counts;
    DevBuf<unsigned long long> tile_off;
    uint64_t n_tiles = 0;
    uint64_t n_live = 0, n_recs = 0;  // keys and records of the slots (the key that equals EMPTY_KEY not among them)
    unsigned long long empty_cnt = 0;
    float count_ms = 0;
    int empty_value() const { return empty_cnt > 32767ull ? 32767 : (int)empty_cnt; }
    uint64_t total() const { return n_live + (empty_cnt ? 1 : 0); }
    bool empty_record(int threshold) const { return empty_cnt && empty_value() > threshold; }
    uint64_t written(int threshold) const { return n_recs + (empty_record(threshold) ? 1 : 0); }
    void empty_bytes(unsigned char *rec) const
    {
        for (int b = 0; b < 8; b++) rec[b] = (unsigned char)(EMPTY_KEY >> (8 * (7 - b)));
        rec[8] = (unsigned char)((uint16_t)empty_value() >> 8);
        rec[9] = (unsigned char)((uint16_t)empty_value() & 0xFF);
    }
};

uint32_t kb_grid(uint64_t tiles) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(tiles, 1), KB_MAX_GRID); }

// d_hist: 32768 bins (zeroed here), or NULL
int kb_count(mc_ctx *c, int threshold, unsigned long long *d_hist, KbSweep *S)
{
    const uint64_t n_slots = c->slots ? c->n_slots() : 0;
    S->n_tiles = (n_slots + KB_TILE - 1) / KB_TILE;
    HIPCHK(c, S->tile_counts.alloc(S->n_tiles));
    HIPCHK(c, S->tile_off.alloc(S->n_tiles + 1));
    unsigned long long *n_live = c->d_ctr + 2;
    HIPCHK(c, hipMemsetAsync(n_live, 0, sizeof(unsigned long long), c->stream));
    if (d_hist) HIPCHK(c, hipMemsetAsync(d_hist, 0, KB_HIST_BINS * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    // (no tile: one workgroup still adds the out-of-band key to the histogram)
    hipLaunchKernelGGL(k_kb_count, dim3(kb_grid(S->n_tiles)), dim3(KB_THREADS), 0, c->stream, c->slots, n_slots, threshold, c->dup_filter(),
                       S->tile_counts.p, d_hist, n_live, c->d_ctr + 1);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    if (S->n_tiles) {
        int rc = tok_scan(c, S->tile_counts.p, S->n_tiles, S->tile_off.p, &S->n_recs);
        if (rc) return rc;
    }
    unsigned long long *h = c->h_scratch;
    HIPCHK(c, hipMemcpyAsync(h, n_live, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h + 1, c->d_ctr + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    S->n_live = h[0];
    S->empty_cnt = h[1];
    HIPCHK(c, hipEventElapsedTime(&S->count_ms, c->ev0, c->ev1));
    return MC_OK;
}

// sweep 2 over [tile_begin, tile_end) into d_out, enqueued on the context's stream; rec_base = tile_off[tile_begin]
int kb_write(mc_ctx *c, int threshold, const KbSweep &S, uint64_t tile_begin, uint64_t tile_end, uint64_t rec_base, uint8_t *d_out, uint64_t out_bytes)
{
    if (tile_end <= tile_begin) return MC_OK;
    hipLaunchKernelGGL(k_kb_write, dim3(kb_grid(tile_end - tile_begin)), dim3(KB_THREADS), 0, c->stream, c->slots, c->n_slots(), threshold,
                       c->dup_filter(), S.tile_off.p, tile_begin, tile_end, (unsigned long long)rec_base, d_out, out_bytes);
    HIPCHK(c, hipGetLastError());
    return MC_OK;
}

int kb_decode(mc_ctx *c, const uint8_t *d_bytes, uint64_t n_records, int freq_threshold, int64_t *d_keys, int16_t *d_counts, uint64_t *n_kept, float *ms)
{
    unsigned long long *cursor = c->d_ctr + 2;
    HIPCHK(c, hipMemsetAsync(cursor, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    hipLaunchKernelGGL(k_kb_decode, dim3(kb_grid((n_records + KB_TILE - 1) / KB_TILE)), dim3(KB_THREADS), 0, c->stream, d_bytes, n_records,
                       freq_threshold, d_keys, d_counts, cursor);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_scratch, cursor, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_kept = c->h_scratch[0];
    if (ms) HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return MC_OK;
}

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct PinnedBuf {  // RAII page-locked host memory
    char *p = nullptr;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t bytes) { return hipHostMalloc(reinterpret_cast<void **>(&p), std::max<size_t>(bytes, 1)); }
};

// The save's writer: the caller fills the two staging slots in turn (a copy into host[b] is enqueued, done[b] recorded behind it),
// this thread waits for a slot's copy and writes it to the file, then hands the slot back.
struct KbWriter {
    int fd = -1, device = 0;
    char *host[2] = {};
    hipEvent_t done[2] = {};
    std::mutex mu;
    std::condition_variable cv;
    bool queued[2] = {false, false};
    size_t bytes[2] = {};
    bool quit = false, failed = false;
    double file_ms = 0;
    std::thread th;

    void start() { th = std::thread([this] { run(); }); }
    void run()
    {
        if (hipSetDevice(device) != hipSuccess) failed = true;
        for (int b = 0;; b ^= 1) {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return queued[b] || quit; });
            if (!queued[b]) return;
            lk.unlock();
            bool ok = !failed && hipEventSynchronize(done[b]) == hipSuccess;
            const auto t0 = std::chrono::steady_clock::now();
            for (size_t at = 0; ok && at < bytes[b];) {
                const ssize_t r = write(fd, host[b] + at, bytes[b] - at);
                if (r <= 0) ok = false;
                else at += (size_t)r;
            }
            lk.lock();
            file_ms += ms_since(t0);
            if (!ok) failed = true;
            queued[b] = false;
            cv.notify_all();
        }
    }
    void wait_free(int b)  // until slot b has been written
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !queued[b]; });
    }
    void submit(int b, size_t n)
    {
        std::lock_guard<std::mutex> lk(mu);
        bytes[b] = n;
        queued[b] = true;
        cv.notify_all();
    }
    void finish()  // what is queued is written first
    {
        if (!th.joinable()) return;
        {
            std::lock_guard<std::mutex> lk(mu);
            quit = true;
            cv.notify_all();
        }
        th.join();
    }
    ~KbWriter() { finish(); }
};

// the events and the side stream of a save
struct KbSaveHip {
    hipStream_t copy_stream = nullptr;
    hipEvent_t k0[2] = {}, k1[2] = {}, c0[2] = {}, c1[2] = {};  // before and behind a slot's kernel, before and behind its copy
    ~KbSaveHip()
    {
        for (int b = 0; b < 2; b++) {
            if (k0[b]) (void)hipEventDestroy(k0[b]);
            if (k1[b]) (void)hipEventDestroy(k1[b]);
            if (c0[b]) (void)hipEventDestroy(c0[b]);
            if (c1[b]) (void)hipEventDestroy(c1[b]);
        }
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
    }
    hipError_t create()
    {
        hipError_t e = hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking);
        for (int b = 0; b < 2 && e == hipSuccess; b++) {
            e = hipEventCreate(&k0[b]);
            if (e == hipSuccess) e = hipEventCreate(&k1[b]);
            if (e == hipSuccess) e = hipEventCreate(&c0[b]);
            if (e == hipSuccess) e = hipEventCreate(&c1[b]);
        }
        return e;
    }
};

// the text of <name>.stat.txt as mc_save_kmers writes it
int kb_write_stat(mc_ctx *c, const char *stat_path, const std::vector<unsigned long long> &hist)
{
    FILE *sf = fopen(stat_path, "w");
    if (!sf) return fail(c, MC_EINVAL, "mc_save_kmers: cannot write %s", stat_path);
    fputs("# k-mer frequency\tnumber of such k-mers\n", sf);
    for (size_t v = 0; v < hist.size(); v++)
        if (hist[v]) fprintf(sf, "%zu\t%llu\n", v, hist[v]);
    fputs("\n", sf);  // (println of a string that already ends with a newline)
    if (fclose(sf) != 0) return fail(c, MC_EINVAL, "mc_save_kmers: error writing %s", stat_path);
    return MC_OK;
}

struct Fd {  // RAII file descriptor
    int fd = -1;
    ~Fd() { if (fd >= 0) (void)close(fd); }
};

}  // namespace

int mc_kmers_encode_dev(mc_ctx *c, int threshold, uint8_t *d_bytes, uint64_t cap_bytes, uint64_t *d_hist, uint64_t *n_total, uint64_t *n_written)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (n_total) *n_total = 0;
    if (n_written) *n_written = 0;
    if (!c->finalized) return fail(c, MC_ESTATE, "mc_kmers_encode: call mc_finalize_counts first");
    if (reinterpret_cast<uintptr_t>(d_bytes) & 15) return fail(c, MC_EINVAL, "mc_kmers_encode: d_bytes is not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_hist) & 7) return fail(c, MC_EINVAL, "mc_kmers_encode: d_hist is not 8-byte aligned");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    KbSweep S;
    int rc = kb_count(c, threshold, reinterpret_cast<unsigned long long *>(d_hist), &S);
    if (rc) return rc;
    const uint64_t written = S.written(threshold);
    if (n_total) *n_total = S.total();
    if (n_written) *n_written = written;
    if (!d_bytes) return MC_OK;
    if (written * KB_RECORD > cap_bytes)
        return fail(c, MC_EINVAL, "mc_kmers_encode: %llu bytes of records but capacity %llu", (unsigned long long)(written * KB_RECORD),
                    (unsigned long long)cap_bytes);
    rc = kb_write(c, threshold, S, 0, S.n_tiles, 0, d_bytes, cap_bytes & ~1ull);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (S.empty_record(threshold)) {  // the last record, as mc_export_dev appends its pair
        unsigned char rec[KB_RECORD];
        S.empty_bytes(rec);
        HIPCHK(c, hipMemcpy(d_bytes + S.n_recs * KB_RECORD, rec, KB_RECORD, hipMemcpyHostToDevice));
    }
    return MC_OK;
}

int mc_kmers_decode_dev(mc_ctx *c, const uint8_t *d_bytes, uint64_t n_records, int freq_threshold, int64_t *d_keys, int16_t *d_counts,
                        uint64_t *n_kept)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (n_kept) *n_kept = 0;
    if (n_records == 0) return MC_OK;
    if (!d_bytes || !d_keys || !d_counts) return fail(c, MC_EINVAL, "mc_kmers_decode: null pointer");
    if (reinterpret_cast<uintptr_t>(d_bytes) & 15) return fail(c, MC_EINVAL, "mc_kmers_decode: d_bytes is not 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_keys) & 7) || (reinterpret_cast<uintptr_t>(d_counts) & 3))
        return fail(c, MC_EINVAL, "mc_kmers_decode: d_keys is not 8-byte or d_counts not 4-byte aligned");
    if (n_records > (~0ull >> 1) / KB_RECORD) return fail(c, MC_EINVAL, "mc_kmers_decode: %llu records", (unsigned long long)n_records);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    uint64_t kept = 0;
    int rc = kb_decode(c, d_bytes, n_records, freq_threshold, d_keys, d_counts, &kept, nullptr);
    if (rc) return rc;
    if (n_kept) *n_kept = kept;
    return MC_OK;
}

int mc_save_kmers_gpu(mc_ctx *c, const char *bin_path, const char *stat_path, int threshold, uint64_t *n_total, uint64_t *n_written)
{
    if (!c) return MC_EINVAL;
    if (n_total) *n_total = 0;
    if (n_written) *n_written = 0;
    if (!bin_path) return fail(c, MC_EINVAL, "mc_save_kmers: null path");
    std::lock_guard<std::mutex> g(c->mu);  // (for the whole save: the table must not move between the sweeps)
    if (!c->finalized) return fail(c, MC_ESTATE, "mc_export: call mc_finalize_counts first");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const auto t_start = std::chrono::steady_clock::now();
    DevBuf<unsigned long long> d_hist;
    HIPCHK(c, d_hist.alloc(KB_HIST_BINS));
    KbSweep S;
    int rc = kb_count(c, threshold, d_hist.p, &S);
    if (rc) return rc;
    std::vector<unsigned long long> hist(KB_HIST_BINS), off(S.n_tiles + 1);
    HIPCHK(c, hipMemcpy(hist.data(), d_hist.p, hist.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (S.n_tiles) HIPCHK(c, hipMemcpy(off.data(), S.tile_off.p, S.n_tiles * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    off[S.n_tiles] = S.n_recs;

    Fd out;
    out.fd = open(bin_path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (out.fd < 0) return fail(c, MC_EINVAL, "mc_save_kmers: cannot write %s", bin_path);
    // a chunk is whole tiles, so never less than one tile's records
    const uint64_t chunk = std::max<uint64_t>(c->sw.kmers_chunk_records, KB_TILE);
    const uint64_t stage_bytes = (std::min<uint64_t>(chunk, std::max<uint64_t>(S.n_recs, 1)) * KB_RECORD + 15) & ~15ull;
    DevBuf<uint8_t> stage[2];
    PinnedBuf host[2];
    KbSaveHip H;
    KbWriter W;
    float write_ms = 0, copy_ms = 0;
    uint32_t n_chunks = 0;
    if (S.n_recs) {
        for (int b = 0; b < 2; b++) {
            HIPCHK(c, stage[b].alloc(stage_bytes));
            HIPCHK(c, host[b].alloc(stage_bytes));
        }
        HIPCHK(c, H.create());
        W.fd = out.fd;
        W.device = c->cfg.device;
        for (int b = 0; b < 2; b++) { W.host[b] = host[b].p; W.done[b] = H.c1[b]; }
        W.start();
        bool used[2] = {false, false};
        auto reap = [&](int b) {  // slot b is written: its kernel's and its copy's device time
            W.wait_free(b);
            if (!used[b]) return;
            float k = 0, cp = 0;
            if (hipEventElapsedTime(&k, H.k0[b], H.k1[b]) == hipSuccess) write_ms += k;  // (figures for MC_KMERS_STATS: no reason to fail a save)
            if (hipEventElapsedTime(&cp, H.c0[b], H.c1[b]) == hipSuccess) copy_ms += cp;
            used[b] = false;
        };
        for (uint64_t t0 = 0; t0 < S.n_tiles && !rc;) {
            // the longest run of tiles from t0 with at most `chunk` records
            const uint64_t t1 = (uint64_t)(std::upper_bound(off.begin() + (long)t0, off.end(), off[t0] + chunk) - off.begin()) - 1;
            const uint64_t n_bytes = (off[t1] - off[t0]) * KB_RECORD;
            if (n_bytes) {
                const int b = (int)(n_chunks & 1);
                reap(b);
                HIPCHK(c, hipEventRecord(H.k0[b], c->stream));
                rc = kb_write(c, threshold, S, t0, t1, off[t0], stage[b].p, stage_bytes);
                if (rc) break;
                HIPCHK(c, hipEventRecord(H.k1[b], c->stream));
                HIPCHK(c, hipStreamWaitEvent(H.copy_stream, H.k1[b], 0));
                HIPCHK(c, hipEventRecord(H.c0[b], H.copy_stream));
                HIPCHK(c, hipMemcpyAsync(host[b].p, stage[b].p, n_bytes, hipMemcpyDeviceToHost, H.copy_stream));
                HIPCHK(c, hipEventRecord(H.c1[b], H.copy_stream));
                used[b] = true;
                W.submit(b, n_bytes);
                n_chunks++;
            }
            t0 = t1;
        }
        for (int b = 0; b < 2; b++) reap(b);
        W.finish();
        (void)hipStreamSynchronize(H.copy_stream);
        if (rc) return rc;
    }
    bool io_ok = !W.failed;
    if (io_ok && S.empty_record(threshold)) {
        unsigned char rec[KB_RECORD];
        S.empty_bytes(rec);
        io_ok = write(out.fd, rec, KB_RECORD) == KB_RECORD;
    }
    const int closed = close(out.fd);
    out.fd = -1;
    if (!io_ok || closed != 0) return fail(c, MC_EINVAL, "mc_save_kmers: error writing %s", bin_path);
    if (stat_path) {
        rc = kb_write_stat(c, stat_path, hist);
        if (rc) return rc;
    }
    if (n_total) *n_total = S.total();
    if (n_written) *n_written = S.written(threshold);
    if (c->sw.kmers_stats)
        fprintf(stderr, "mc_save_kmers_gpu: slots %llu records %llu chunks %u count_ms %.3f write_ms %.3f copy_ms %.3f file_ms %.3f total_ms %.3f extra_device_bytes %llu\n",
                (unsigned long long)(c->slots ? c->n_slots() : 0), (unsigned long long)S.written(threshold), n_chunks, S.count_ms, write_ms,
                copy_ms, W.file_ms, ms_since(t_start),
                (unsigned long long)((S.n_recs ? 2 * stage_bytes : 0) + S.n_tiles * 12 + 8 + KB_HIST_BINS * 8));
    return MC_OK;
}

int mc_load_kmers_gpu(mc_ctx *c, const char *path, int freq_threshold, uint64_t *n_records, uint64_t *n_added)
{
    if (!c) return MC_EINVAL;
    if (n_records) *n_records = 0;
    if (n_added) *n_added = 0;
    if (!path) return fail(c, MC_EINVAL, "mc_load_kmers: null path");
    const auto t_start = std::chrono::steady_clock::now();
    Fd in;
    in.fd = open(path, O_RDONLY);
    struct stat sb;
    if (in.fd < 0 || fstat(in.fd, &sb) != 0 || !S_ISREG(sb.st_mode)) return fail(c, MC_EINVAL, "Failed to read from file %s", path);
    const uint64_t size = (uint64_t)sb.st_size;
    if (size % KB_RECORD != 0)
        return fail(c, MC_EINVAL, "Can't load kmers from file %s: its length is not a multiple of the 10-byte record", path);
    const uint64_t total = size / KB_RECORD;
    if (total == 0) return MC_OK;
    const uint64_t chunk = std::min<uint64_t>(c->sw.kmers_chunk_records, total);
    const uint64_t n_chunks = (total + chunk - 1) / chunk;
    DevBuf<uint8_t> raw[2];
    DevBuf<int64_t> dk;
    DevBuf<int16_t> dc;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (hipSetDevice(c->cfg.device) != hipSuccess || raw[0].alloc(chunk * KB_RECORD + 16) != hipSuccess ||
            (n_chunks > 1 && raw[1].alloc(chunk * KB_RECORD + 16) != hipSuccess) || dk.alloc(chunk) != hipSuccess || dc.alloc(chunk + 2) != hipSuccess)
            return fail(c, MC_ENOMEM, "mc_load_kmers: device allocation failed");
    }
    // the reader: chunk i + 1 comes from the file into the other buffer while chunk i is decoded and added
    struct Fetch {
        std::thread th;
        bool ok = true;
        double ms = 0;
        ~Fetch() { if (th.joinable()) th.join(); }
    } F;
    double fetch_ms = 0, add_ms = 0;
    float decode_ms = 0;
    auto records_of = [&](uint64_t i) { return std::min<uint64_t>(chunk, total - i * chunk); };
    auto fetch = [&](uint64_t i) {
        F.th = std::thread([&F, c, dst = raw[i & 1].p, bytes = records_of(i) * KB_RECORD, fd = in.fd, at = i * chunk * KB_RECORD] {
            const auto t0 = std::chrono::steady_clock::now();
            F.ok = h2d_pinned(c, dst, nullptr, bytes, fd, at);
            F.ms = ms_since(t0);
        });
    };
    fetch(0);
    uint64_t added = 0;
    for (uint64_t i = 0; i < n_chunks; i++) {
        F.th.join();
        fetch_ms += F.ms;
        if (!F.ok) return fail(c, MC_EHIP, "mc_load_kmers: reading %s or its upload failed", path);
        if (i + 1 < n_chunks) fetch(i + 1);
        uint64_t kept = 0;
        {
            std::lock_guard<std::mutex> g(c->mu);
            HIPCHK(c, hipSetDevice(c->cfg.device));
            float ms = 0;
            int rc = kb_decode(c, raw[i & 1].p, records_of(i), freq_threshold, dk.p, dc.p, &kept, &ms);
            if (rc) return rc;
            decode_ms += ms;
        }
        if (kept) {  // (mc_add_pairs_dev takes the context's lock itself)
            const auto t0 = std::chrono::steady_clock::now();
            int rc = mc_add_pairs_dev(c, dk.p, dc.p, nullptr, kept);
            if (rc) return rc;
            add_ms += ms_since(t0);
            added += kept;
        }
    }
    if (n_records) *n_records = total;
    if (n_added) *n_added = added;
    if (c->sw.kmers_stats)
        fprintf(stderr, "mc_load_kmers_gpu: records %llu chunks %llu fetch_ms %.3f decode_ms %.3f add_ms %.3f total_ms %.3f extra_device_bytes %llu\n",
                (unsigned long long)total, (unsigned long long)n_chunks, fetch_ms, decode_ms, add_ms, ms_since(t_start),
                (unsigned long long)((n_chunks > 1 ? 2 : 1) * (chunk * KB_RECORD + 16) + chunk * 10 + 4));
    return MC_OK;
}
