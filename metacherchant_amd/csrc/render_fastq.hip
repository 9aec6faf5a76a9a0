// libmcgpu.so, the FASTQ rendering unit: the classifiers' output records as text on the device (include/mcgpu.h mc_render_fastq_dev,
// mc_render_fastq, mc_render_fastq_bound; itmo!/io/writers/FastqDedicatedWriter.java:39-60).  csrc/host/fastq_out.h FastqOut::put is the
// host loop these are compared with.  context.h lists the other units.
//
// An ITEM is one read of one side, item j = n_sides * read + side; a stream takes its items in item order.  A record's length depends
// on the digits of its number, so on its rank in its stream: two scans.  A BLOCK is 256 consecutive items, a lane an item.
//   k_rf_count    per block and stream the number of selected items, by ballots; a stream byte that names no stream and a selected
//                 read of length 0 are noted here (an atomic minimum over the item index: the lowest one wins).
//   (tok_scan)    reads_file.hip's scan over the counts, stream by stream: ranks.
//   k_rf_measure  per item its number and its place among the block's bytes of its stream, per block and stream the bytes (64-bit).
//   k_rf_scan64   the exclusive scan of those sums (one workgroup: 16 entries per block of 256 items).
//   k_rf_bounds   where every stream starts in the two scans: 34 numbers for the host, which lays the streams out (each on a 16-byte
//                 boundary) and compares with the capacity before anything is written.
//   k_rf_emit     a wave a record, on the output's dword grid: a lane builds the dword at 4 d from the record's header (held a byte
//                 a lane, read with a shuffle), two words of packed bases, and the phreds.  A dword that lies inside the record
//                 leaves as a dword store, 256 B a wave instruction; a first or last dword shared with the neighbouring record is
//                 written byte by byte by each record's owner.  So every byte has one writer and two calls give the same bytes.
//                 A phred above 62 is noted here, the first of the record, again by an atomic minimum over the item index.
// No loop depends on another workgroup; every store is checked against the capacity, whatever the inputs hold.
#include "context.h"

namespace {

constexpr int RF_THREADS = 256, RF_WAVES = RF_THREADS / 64;
constexpr int RF_BLOCK = RF_THREADS;  // items of a block
constexpr int RF_MAX_GRID = 4096;
constexpr uint32_t RF_NONE = 0xFFFFFFFFu;          // an item that is in no stream
constexpr int RF_S = MC_RENDER_MAX_STREAMS;
constexpr int RF_SMALL = 2 * (RF_S + 1) + 2;       // k_rf_bounds' numbers, then the two error keys
constexpr int RF_ERR_STREAM = 2 * (RF_S + 1), RF_ERR_DATA = RF_ERR_STREAM + 1;
static_assert(RF_SMALL <= 64, "the small results come down through h_scratch-sized staging");

struct RfArgs {
    mc_render_side side[2];
    uint32_t n_sides, n_streams;
    uint64_t n_items, n_blocks;
};
struct RfStreams {
    unsigned long long first[RF_S], start[RF_S];
};

__device__ const unsigned long long RF_P10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull,
                                                  1000000000ull, 10000000000ull, 100000000000ull, 1000000000000ull, 10000000000000ull,
                                                  100000000000000ull, 1000000000000000ull, 10000000000000000ull, 100000000000000000ull,
                                                  1000000000000000000ull, 10000000000000000000ull};

__device__ __forceinline__ uint32_t rf_digits(unsigned long long n)
{
    uint32_t d = 1;
#pragma unroll
    for (int i = 1; i < 20; i++) d += n >= RF_P10[i] ? 1u : 0u;
    return d;
}

struct RfItem {
    uint32_t s;      // its stream, RF_NONE for none; `raw` the byte as given
    uint32_t raw, sd;
    uint64_t read, o0, len;
};

// item j as every pass sees it
__device__ __forceinline__ RfItem rf_item(const RfArgs &A, uint64_t j)
{
    RfItem it;
    it.sd = A.n_sides == 2 ? (uint32_t)(j & 1) : 0u;
    it.read = A.n_sides == 2 ? j >> 1 : j;
    const uint8_t *st = it.sd ? A.side[1].stream : A.side[0].stream;
    const uint64_t *off = it.sd ? A.side[1].offsets : A.side[0].offsets;
    it.raw = st[it.read];
    it.s = it.raw < A.n_streams ? it.raw : RF_NONE;
    it.o0 = 0;
    it.len = 0;
    if (it.s != RF_NONE) {
        const uint64_t a = off[it.read], b = off[it.read + 1];
        it.o0 = a;
        it.len = b > a ? b - a : 0;
    }
    return it;
}

__device__ __forceinline__ unsigned long long rf_key(uint64_t j, uint32_t kind, uint32_t value)
{
    return ((unsigned long long)j << 16) | (kind << 8) | (value & 0xFFu);
}

__global__ void __launch_bounds__(RF_THREADS) k_rf_count(RfArgs A, uint32_t *__restrict__ counts, unsigned long long *small)
{
    __shared__ uint32_t wc[RF_WAVES][RF_S];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (uint64_t b = blockIdx.x; b < A.n_blocks; b += gridDim.x) {
        const uint64_t j = b * RF_BLOCK + tid;
        uint32_t s = RF_NONE;
        if (j < A.n_items) {
            const RfItem it = rf_item(A, j);
            s = it.s;
            if (s == RF_NONE && it.raw != MC_RENDER_SKIP) atomicMin(small + RF_ERR_STREAM, rf_key(j, MC_RENDER_STREAM, it.raw));
            if (s != RF_NONE && it.len == 0) atomicMin(small + RF_ERR_DATA, rf_key(j, MC_RENDER_EMPTY, 0));
        }
        for (uint32_t t = 0; t < A.n_streams; t++) {
            const uint32_t n = (uint32_t)__popcll(__ballot(s == t));
            if (lane == 0) wc[w][t] = n;
        }
        __syncthreads();
        if (tid < A.n_streams) {
            uint32_t sum = 0;
#pragma unroll
            for (int x = 0; x < RF_WAVES; x++) sum += wc[x][tid];
            counts[(uint64_t)tid * A.n_blocks + b] = sum;
        }
        __syncthreads();  // (wc serves the next block)
    }
}

// rank_off: the scan of k_rf_count's counts.  number[j]: the record's number (first_number + rank); place[j]: the bytes of its stream
// that the block's items before it give; sums[t * n_blocks + b]: the bytes of stream t in block b
__global__ void __launch_bounds__(RF_THREADS) k_rf_measure(RfArgs A, RfStreams F, const unsigned long long *__restrict__ rank_off,
                                                           unsigned long long *__restrict__ number, unsigned long long *__restrict__ place,
                                                           unsigned long long *__restrict__ sums)
{
    __shared__ uint32_t wc[RF_WAVES][RF_S];
    __shared__ unsigned long long wb[RF_WAVES][RF_S];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (uint64_t b = blockIdx.x; b < A.n_blocks; b += gridDim.x) {
        const uint64_t j = b * RF_BLOCK + tid;
        RfItem it{RF_NONE, 0, 0, 0, 0, 0};
        if (j < A.n_items) it = rf_item(A, j);
        const uint32_t s = it.s;
        uint32_t in_wave = 0;
        for (uint32_t t = 0; t < A.n_streams; t++) {
            const unsigned long long m = __ballot(s == t);
            if (lane == 0) wc[w][t] = (uint32_t)__popcll(m);
            if (s == t) in_wave = (uint32_t)__popcll(m & ((1ull << lane) - 1));
        }
        __syncthreads();
        unsigned long long bytes = 0;
        if (s != RF_NONE) {
            unsigned long long rank = rank_off[(uint64_t)s * A.n_blocks + b] - rank_off[(uint64_t)s * A.n_blocks] + in_wave;
            for (uint32_t x = 0; x < w; x++) rank += wc[x][s];
            const unsigned long long first = F.first[s], n = first + rank;
            number[j] = n;
            bytes = 2 * it.len + (first == MC_RENDER_UNNUMBERED ? 5u : rf_digits(n) + 6u);
        }
        unsigned long long before = 0;
        for (uint32_t t = 0; t < A.n_streams; t++) {
            if (__ballot(s == t) == 0) {  // (the same in every lane)
                if (lane == 0) wb[w][t] = 0;
                continue;
            }
            const unsigned long long own = s == t ? bytes : 0;
            unsigned long long incl = own;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long below = __shfl_up(incl, o);
                if ((int)lane >= o) incl += below;
            }
            if (s == t) before = incl - own;
            if (lane == 63) wb[w][t] = incl;
        }
        __syncthreads();
        if (s != RF_NONE) {
            for (uint32_t x = 0; x < w; x++) before += wb[x][s];
            place[j] = before;
        }
        if (tid < A.n_streams) {
            unsigned long long sum = 0;
#pragma unroll
            for (int x = 0; x < RF_WAVES; x++) sum += wb[x][tid];
            sums[(uint64_t)tid * A.n_blocks + b] = sum;
        }
        __syncthreads();  // (wc and wb serve the next block)
    }
}

// v[0, m) becomes its exclusive scan, v[m] the total (one workgroup)
__global__ void __launch_bounds__(1024) k_rf_scan64(unsigned long long *v, uint64_t m)
{
    __shared__ unsigned long long part[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned long long carry = 0;  // the same in every thread
    for (uint64_t base = 0; base < m; base += 1024) {
        const uint64_t at = base + tid;
        const unsigned long long own = at < m ? v[at] : 0;
        unsigned long long incl = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long below = __shfl_up(incl, o);
            if ((int)lane >= o) incl += below;
        }
        if (lane == 63) part[w] = incl;
        __syncthreads();
        unsigned long long before = 0, total = 0;
#pragma unroll
        for (uint32_t x = 0; x < 16; x++) {
            const unsigned long long p = part[x];
            if (x < w) before += p;
            total += p;
        }
        if (at < m) v[at] = carry + before + incl - own;
        carry += total;
        __syncthreads();  // (part serves the next round)
    }
    if (tid == 0) v[m] = carry;
}

// small[t] = rank_off[t * n_blocks], small[17 + t] = byte_off[t * n_blocks] (t = n_streams: the bytes' total)
__global__ void k_rf_bounds(const unsigned long long *__restrict__ rank_off, const unsigned long long *__restrict__ byte_off, uint64_t n_blocks,
                            uint32_t n_streams, unsigned long long *small)
{
    const uint32_t t = threadIdx.x;
    if (t < n_streams) small[t] = rank_off[(uint64_t)t * n_blocks];
    if (t <= n_streams) small[RF_S + 1 + t] = byte_off[(uint64_t)t * n_blocks];
}

__global__ void __launch_bounds__(RF_THREADS) k_rf_emit(RfArgs A, RfStreams F, const unsigned long long *__restrict__ byte_off,
                                                        const unsigned long long *__restrict__ number, const unsigned long long *__restrict__ place,
                                                        uint8_t *__restrict__ text, uint64_t capacity, unsigned long long *small)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * RF_WAVES + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * RF_WAVES;
    for (uint64_t j = wave0; j < A.n_items; j += n_waves) {  // (everything up to the dword loop is the same in every lane)
        const RfItem it = rf_item(A, j);
        if (it.s == RF_NONE) continue;
        const uint64_t *words = it.sd ? A.side[1].words : A.side[0].words;
        const uint8_t *phred = it.sd ? A.side[1].phred : A.side[0].phred;
        const bool numbered = F.first[it.s] != MC_RENDER_UNNUMBERED;
        const unsigned long long n = number[j];
        const uint32_t dg = rf_digits(n);
        const int64_t hlen = numbered ? dg + 2 : 1, len = (int64_t)it.len;
        // the header, a byte a lane: '@', the digits, '\n'
        uint32_t hb = '\n';
        if (numbered) {
            if (lane == 0) hb = '@';
            else if (lane <= dg) {
                const unsigned long long p = RF_P10[dg - lane];
                hb = '0' + (n >> 32 ? (uint32_t)((n / p) % 10) : ((uint32_t)n / (uint32_t)p) % 10);  // (n < 2^32: p is too)
            }
        }
        const uint64_t row = (uint64_t)it.s * A.n_blocks;
        const uint64_t pos = F.start[it.s] + (byte_off[row + j / RF_BLOCK] - byte_off[row]) + place[j];
        const int64_t total = hlen + 2 * len + 4, q0 = hlen + len + 3;  // q0: where the qualities start
        const uint64_t d_first = pos >> 2, d_last = (pos + (uint64_t)total - 1) >> 2;
        unsigned long long bad = ~0ull;  // (position << 8) | byte of the first phred above 62 this lane met
        for (uint64_t d0 = d_first; d0 <= d_last; d0 += 64) {
            const uint64_t d = d0 + lane;
            const int64_t r0 = (int64_t)(d << 2) - (int64_t)pos;  // the dword's first byte in the record (-3 at least)
            const bool live = d <= d_last;
            // the two words that hold the dword's bases
            const int64_t pb = (int64_t)it.o0 + (r0 - hlen);
            uint64_t wa = 0, wbb = 0, wi = 0;
            if (live && len > 0 && r0 + 3 >= hlen && r0 < hlen + len) {
                const int64_t q = pb < (int64_t)it.o0 ? (int64_t)it.o0 : pb;
                wi = (uint64_t)q >> 5;
                wa = words[wi];
                wbb = words[wi + 1];  // (the pad word, at the end)
            }
            uint32_t v = 0, inside = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int64_t r = r0 + k;
                uint32_t h = 0;
                if (d0 == d_first) h = (uint32_t)__shfl((int)hb, (int)(r < 0 ? 0 : r > 63 ? 63 : r));  // (every lane of the wave is here)
                uint32_t c = '\n';
                if (!live || r < 0 || r >= total) {
                    continue;
                } else if (r < hlen) {
                    c = h;
                } else if (r < hlen + len) {
                    const uint32_t rel = (uint32_t)((uint64_t)(pb + k) - (wi << 5));  // 0 .. 34
                    const uint32_t code = (uint32_t)((rel < 32 ? wa >> (62 - 2 * rel) : wbb >> (62 - 2 * (rel - 32))) & 3u);
                    c = (0x54434741u >> (8 * code)) & 0xFFu;  // "AGCT"
                } else if (r < q0) {
                    c = r == hlen + len + 1 ? '+' : '\n';
                } else if (r < total - 1) {
                    const uint32_t q = phred[it.o0 + (uint64_t)(r - q0)];
                    if (q > 62) {
                        const unsigned long long key = ((unsigned long long)(r - q0) << 8) | q;
                        bad = key < bad ? key : bad;
                    }
                    c = (q + 64) & 0xFFu;
                }
                v |= c << (8 * k);
                inside |= 1u << k;
            }
            const uint64_t at = d << 2;
            if (inside == 15u) {
                if (at + 4 <= capacity) *reinterpret_cast<uint32_t *>(text + at) = v;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (((inside >> k) & 1u) && at + k < capacity) text[at + k] = (uint8_t)(v >> (8 * k));
            }
        }
        if (__ballot(bad != ~0ull)) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long other = __shfl_xor(bad, o);
                bad = other < bad ? other : bad;
            }
            if (lane == 0) atomicMin(small + RF_ERR_DATA, rf_key(j, MC_RENDER_QUALITY, (uint32_t)bad & 0xFFu));
        }
    }
}

// ------------------------------------------------------------------------------------------ host

void rf_note_error(unsigned long long key, mc_render_result *out, uint32_t n_sides)
{
    const uint64_t j = key >> 16;
    out->error = (int32_t)((key >> 8) & 0xFF);
    out->error_value = (uint32_t)(key & 0xFF);
    out->error_side = n_sides == 2 ? (uint32_t)(j & 1) : 0u;
    out->error_read = n_sides == 2 ? j >> 1 : j;
}

int rf_check_args(mc_ctx *c, const mc_render_side *sides, uint32_t n_sides, uint64_t n_reads, uint32_t n_streams, const uint64_t *first_number,
                  const uint8_t *text, mc_render_result *out)
{
    if (!sides || !first_number || !text || !out) return fail(c, MC_EINVAL, "mc_render_fastq: null pointer");
    if (n_sides != 1 && n_sides != 2) return fail(c, MC_EINVAL, "mc_render_fastq: %u sides (1 or 2)", n_sides);
    if (n_streams == 0 || n_streams > MC_RENDER_MAX_STREAMS)
        return fail(c, MC_EINVAL, "mc_render_fastq: %u streams (1 .. %d)", n_streams, MC_RENDER_MAX_STREAMS);
    for (uint32_t s = 0; s < n_sides; s++)
        if (!sides[s].words || !sides[s].phred || !sides[s].offsets || !sides[s].stream) return fail(c, MC_EINVAL, "mc_render_fastq: null pointer");
    if (n_reads >= (1ull << 40) / n_sides) return fail(c, MC_EINVAL, "mc_render_fastq: %llu reads", (unsigned long long)n_reads);
    return MC_OK;
}

// the passes (the caller holds c->mu, has set the device and checked the arguments; d_text may be NULL when n_reads is 0)
int rf_render(mc_ctx *c, const mc_render_side *sides, uint32_t n_sides, uint64_t n_reads, uint32_t n_streams, const uint64_t *first_number,
              uint8_t *d_text, uint64_t capacity, mc_render_result *out)
{
    RfArgs A{};
    for (uint32_t s = 0; s < n_sides; s++) A.side[s] = sides[s];
    A.n_sides = n_sides;
    A.n_streams = n_streams;
    A.n_items = n_reads * n_sides;
    A.n_blocks = (A.n_items + RF_BLOCK - 1) / RF_BLOCK;
    if (A.n_items == 0) return MC_OK;
    RfStreams F{};
    for (uint32_t t = 0; t < n_streams; t++) F.first[t] = first_number[t];
    const uint64_t cells = A.n_blocks * n_streams;
    PoolBuf<uint32_t> counts;
    PoolBuf<unsigned long long> rank_off, byte_off, number, place, small;
    HIPCHK(c, counts.alloc(&c->tok_pool, cells));
    HIPCHK(c, rank_off.alloc(&c->tok_pool, cells));
    HIPCHK(c, byte_off.alloc(&c->tok_pool, cells + 1));
    HIPCHK(c, number.alloc(&c->tok_pool, A.n_items));
    HIPCHK(c, place.alloc(&c->tok_pool, A.n_items));
    HIPCHK(c, small.alloc(&c->tok_pool, RF_SMALL));
    const dim3 grid((unsigned)std::min<uint64_t>(A.n_blocks, RF_MAX_GRID)), block(RF_THREADS);
    HIPCHK(c, hipMemsetAsync(small.p + RF_ERR_STREAM, 0xFF, 2 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    hipLaunchKernelGGL(k_rf_count, grid, block, 0, c->stream, A, counts.p, small.p);
    HIPCHK(c, hipGetLastError());
    uint64_t n_records = 0;
    int rc = tok_scan(c, counts.p, cells, rank_off.p, &n_records);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rf_measure, grid, block, 0, c->stream, A, F, rank_off.p, number.p, place.p, byte_off.p);
    hipLaunchKernelGGL(k_rf_scan64, dim3(1), dim3(1024), 0, c->stream, byte_off.p, cells);
    hipLaunchKernelGGL(k_rf_bounds, dim3(1), dim3(64), 0, c->stream, rank_off.p, byte_off.p, A.n_blocks, n_streams, small.p);
    HIPCHK(c, hipGetLastError());
    unsigned long long h[RF_SMALL];
    HIPCHK(c, hipMemcpyAsync(h, small.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h[RF_ERR_STREAM] != ~0ull) {
        rf_note_error(h[RF_ERR_STREAM], out, n_sides);
        return fail(c, MC_EINVAL, "mc_render_fastq: read %llu of side %u has the stream byte %u, and there are %u streams",
                    (unsigned long long)out->error_read, out->error_side, out->error_value, n_streams);
    }
    uint64_t end = 0;
    for (uint32_t t = 0; t < n_streams; t++) {
        out->records[t] = (t + 1 < n_streams ? h[t + 1] : n_records) - h[t];
        out->bytes[t] = h[RF_S + 1 + t + 1] - h[RF_S + 1 + t];
        out->start[t] = F.start[t] = (end + 15) & ~15ull;
        end = out->start[t] + out->bytes[t];
    }
    if (end > capacity) {  // (nothing is written yet)
        for (uint32_t t = 0; t < n_streams; t++) out->start[t] = out->bytes[t] = out->records[t] = 0;
        return fail(c, MC_EOVERFLOW, "mc_render_fastq: %llu bytes of text but capacity %llu", (unsigned long long)end, (unsigned long long)capacity);
    }
    const uint64_t emit_blocks = std::min<uint64_t>((A.n_items + RF_WAVES - 1) / RF_WAVES, RF_MAX_GRID);
    hipLaunchKernelGGL(k_rf_emit, dim3((unsigned)emit_blocks), block, 0, c->stream, A, F, byte_off.p, number.p, place.p, d_text, capacity, small.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipMemcpyAsync(h, small.p + RF_ERR_DATA, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h[0] != ~0ull) rf_note_error(h[0], out, n_sides);
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    out->device_ms = ms;
    return MC_OK;
}

}  // namespace

uint64_t mc_render_fastq_bound(uint64_t n_bases, uint64_t n_items)
{
    return (2 * n_bases + 26 * n_items + 16 * MC_RENDER_MAX_STREAMS + 15) & ~15ull;
}

int mc_render_fastq_dev(mc_ctx *c, const mc_render_side *sides, uint32_t n_sides, uint64_t n_reads, uint32_t n_streams,
                        const uint64_t *first_number, uint8_t *d_text, uint64_t capacity, mc_render_result *out)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (out) *out = mc_render_result{};
    int rc = rf_check_args(c, sides, n_sides, n_reads, n_streams, first_number, d_text, out);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(d_text) & 15) return fail(c, MC_EINVAL, "mc_render_fastq: d_text is not 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return rf_render(c, sides, n_sides, n_reads, n_streams, first_number, d_text, capacity, out);
}

int mc_render_fastq(mc_ctx *c, const mc_render_side *sides, uint32_t n_sides, uint64_t n_reads, uint32_t n_streams, const uint64_t *first_number,
                    uint8_t *text, uint64_t capacity, mc_render_result *out)
{
    if (!c) return MC_EINVAL;
    if (out) *out = mc_render_result{};
    int rc = rf_check_args(c, sides, n_sides, n_reads, n_streams, first_number, text, out);
    if (rc) return rc;
    mc_render_side dev[2] = {};
    uint64_t n_bases = 0;
    HostStage st(c);
    for (uint32_t s = 0; s < n_sides; s++) {
        const uint64_t last = sides[s].offsets[n_reads], from = sides[s].offsets[0];
        if (last < from) return fail(c, MC_EINVAL, "mc_render_fastq: the offsets of side %u decrease", s);
        n_bases += last - from;
        dev[s].words = st.in(sides[s].words, (last + 31) / 32 + 1);
        dev[s].phred = st.in(sides[s].phred, std::max<uint64_t>(last, 1));
        dev[s].offsets = st.in(sides[s].offsets, n_reads + 1);
        dev[s].stream = st.in(sides[s].stream, std::max<uint64_t>(n_reads, 1));
    }
    // (a larger capacity than any input needs buys nothing on the device)
    const uint64_t cap = std::min<uint64_t>(capacity, mc_render_fastq_bound(n_bases, n_reads * n_sides));
    uint8_t *d_text = st.out<uint8_t>(cap);
    if (st.rc) return st.rc;
    rc = rf_render(c, dev, n_sides, n_reads, n_streams, first_number, d_text, cap, out);
    if (rc) return rc;
    for (uint32_t t = 0; t < n_streams; t++)
        if (out->bytes[t]) {
            rc = st.back(text + out->start[t], d_text + out->start[t], out->bytes[t]);
            if (rc) return rc;
        }
    return MC_OK;
}
