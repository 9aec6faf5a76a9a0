// libmcgpu.so: whole reads with their qualities, tokenised on the device (include/mcgpu.h mc_tokenize_whole) -- what the classifying
// tools read their -r files with.  The counting tokeniser (csrc/tokenizer.h) drops FASTA records with N and splits FASTQ reads where
// phred < 1; this one keeps DnaQReader's policy (csrc/host/reads_io.cpp, restating itmo!/io/ReadersUtils.java:185-215 readDnaQLazy,
// itmo!/io/readers/FastqReader.java:53-82, FastaWithNsReader, itmo!/dna/DnaQBuilder.java:32-45):
//   FASTQ  records of four lines; N n . give base 0 with phred 0, any other base its code and (quality char - offset) & 63; a read
//          of length 0 is a read;
//   FASTA  a line that starts with '>' or ';' ends the record before it, the other lines are concatenated, text in front of the
//          first header is a record, empty records give nothing; phred 20, and 0 at N n .;
//   bad_pos  the one position with phred < 10 (-1 none, -2 several): an N counts, in FASTA as well.
// Passes: (1) newline positions (tok_newlines of reads_file.hip); (2) a wave a record (FASTQ) or a line (FASTA) checks every byte and
// measures; (3) scans give every record / line its place; (4) a wave a record / line packs the bases through a WavePacker, stores a
// byte a base with the code and one with the phred -- 64 lanes, 64 bytes in a row -- and finds the low-quality position from the
// ballots over its 64-lane stretches.  Every output byte has one writer (the words' end bits are ORed in), so nothing depends on the
// order the waves run in.  A byte that is no base, a quality char outside [offset, 126], lengths that differ, a line count that is no
// multiple of four, a record that does not start with '@' or whose third line does not start with '+', a read of 2^31 bases: a flag
// goes up, nothing is allocated, and the caller reads that text with the host parser, which defines what happens then.
// mc_reads_append_dev joins slices of such results into one array, for the calls that want all reads at once (k_wr_append_*).
#include "context.h"
#include "tokenizer_device.h"

namespace mc {
namespace tok {

constexpr uint64_t WR_MAX_READ = 0x7FFFFFF0ull;  // bad_pos is an int32

// one base of a whole read: its code, and its phred through *ph.  fastq == false: every known base has phred 20
__device__ __forceinline__ int whole_base(uint8_t c, uint8_t q, bool fastq, int offset, int *ph, uint32_t *bad)
{
    if (c == 'N' || c == 'n' || c == '.') {  // DnaQBuilder.unsafeAppendUnknown (the quality char is not looked at)
        *ph = 0;
        return 0;
    }
    const int code = base_code(c);
    if (code < 0) {
        *bad |= TOK_BAD_CHAR;
        *ph = 63;
        return 0;
    }
    if (!fastq) {
        *ph = 20;  // ReadersUtils.DEFAULT_PHRED_FOR_FASTA
        return code;
    }
    if ((int)q < offset || q > 126) *bad |= TOK_BAD_QUALITY;
    *ph = ((int)q - offset) & 63;  // (DnaQ keeps the phred in 6 bits of a byte: DnaQ.phredAt)
    return code;
}

// the low-quality positions of a stretch of 64, folded into a wave-uniform (count, first position)
__device__ __forceinline__ void low_fold(bool low, uint64_t at, uint32_t *n_low, uint64_t *first)
{
    const uint64_t lm = __ballot(low);
    if (lm) {
        if (*n_low == 0) *first = at + (uint64_t)__builtin_ctzll(lm);
        *n_low += (uint32_t)__popcll(lm);
    }
}

// ---- FASTQ, pass 2: every record's shape and bytes checked, its length
__global__ void __launch_bounds__(T_THREADS) k_wq_records(const uint8_t *__restrict__ t, uint64_t n, const unsigned long long *__restrict__ nl, uint64_t n_nl,
                                                         uint64_t n_rec, int offset, uint32_t *rec_len, uint32_t *flags)
{
    const int lane = threadIdx.x & 63;
    uint32_t bad = 0;
    for (uint64_t r = wave_index(); r < n_rec; r += wave_count()) {
        const FqRecord R = fq_record(t, n, nl, n_nl, r);
        const bool ok = R.ok && R.len <= WR_MAX_READ;
        if (!ok) bad |= TOK_BAD_STRUCTURE;
        else
            for (uint64_t q = lane; q < R.len; q += 64) {
                int ph;
                (void)whole_base(t[R.s1 + q], t[R.s3 + q], true, offset, &ph, &bad);
            }
        if (lane == 0) rec_len[r] = ok ? (uint32_t)R.len : 0u;
    }
    if (bad) atomicOr(flags, bad);
}

// pass 4: record r is read r.  Its offset, its bases packed, a byte a base of codes and phreds, its low-quality position
__global__ void __launch_bounds__(T_THREADS) k_wq_emit(const uint8_t *__restrict__ t, uint64_t n, const unsigned long long *__restrict__ nl, uint64_t n_nl,
                                                      uint64_t n_rec, int offset, const unsigned long long *__restrict__ base_at, uint64_t total_bases,
                                                      uint64_t *offsets, uint64_t *words, int32_t *bad_pos, uint8_t *codes, uint8_t *phred)
{
    __shared__ uint64_t lds[T_THREADS / 64][WP_WORDS];
    const int lane = threadIdx.x & 63;
    WavePacker wp;
    wp.init(lds[threadIdx.x >> 6], words);
    uint32_t dummy = 0;
    for (uint64_t r = wave_index(); r < n_rec; r += wave_count()) {
        const FqRecord R = fq_record(t, n, nl, n_nl, r);
        const uint64_t b0 = base_at[r];
        uint32_t n_low = 0;
        uint64_t first = 0;
        wp.open(b0);
        for (uint64_t q = 0; q < R.len; q += 64) {
            const bool in = q + lane < R.len;
            int code = 0, ph = 63;
            if (in) code = whole_base(t[R.s1 + q + lane], t[R.s3 + q + lane], true, offset, &ph, &dummy);
            (void)wp.put(in, code);
            if (in && codes) codes[b0 + q + lane] = (uint8_t)code;
            if (in && phred) phred[b0 + q + lane] = (uint8_t)ph;
            low_fold(in && ph < 10, q, &n_low, &first);
        }
        if (R.len) wp.flush();
        if (lane == 0) {
            offsets[r] = b0;
            bad_pos[r] = n_low == 0 ? -1 : n_low == 1 ? (int32_t)first : -2;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[n_rec] = total_bases;
}

// ---- FASTA, pass 2: a wave a line -- is it a header, how long is it, how many of its bases are N n . and where is the first
__global__ void __launch_bounds__(T_THREADS) k_wa_lines(const uint8_t *__restrict__ t, uint64_t n, const unsigned long long *__restrict__ nl, uint64_t n_nl,
                                                       uint64_t n_lines, uint32_t *line_hdr, uint32_t *line_len, uint32_t *line_low, uint32_t *line_lowpos,
                                                       uint32_t *flags)
{
    const int lane = threadIdx.x & 63;
    uint32_t bad = 0;
    for (uint64_t j = wave_index(); j < n_lines; j += wave_count()) {
        uint64_t s, e;
        uint8_t c0;
        wave_line_spans(t, n, nl, n_nl, j, 1, &s, &e, &c0);
        s = shfl64(s, 0);
        e = shfl64(e, 0);
        c0 = (uint8_t)__shfl((int)c0, 0);
        const bool hdr = e > s && (c0 == '>' || c0 == ';');
        uint64_t len = hdr ? 0 : e - s, first = 0;
        uint32_t n_low = 0;
        if (len > WR_MAX_READ) {
            bad |= TOK_BAD_STRUCTURE;
            len = 0;
        }
        for (uint64_t q = 0; q < len; q += 64) {
            const bool in = q + lane < len;
            int ph = 63;
            if (in) (void)whole_base(t[s + q + lane], 0, false, 0, &ph, &bad);
            low_fold(in && ph < 10, q, &n_low, &first);
        }
        if (lane == 0) {
            line_hdr[j] = hdr ? 1u : 0u;
            line_len[j] = (uint32_t)len;
            line_low[j] = n_low;
            line_lowpos[j] = (uint32_t)first;
        }
    }
    if (bad) atomicOr(flags, bad);
}

// pass 3a: per record (rec = headers at or before the line): its length, the line that opens it, its N n .  Sums and a minimum:
// the order of the lines plays no part
__global__ void k_wa_records(const unsigned long long *__restrict__ hdr_before, const uint32_t *__restrict__ line_hdr, const uint32_t *__restrict__ line_len,
                             const uint32_t *__restrict__ line_low, uint64_t n_lines, unsigned long long *rec_len, uint32_t *rec_first, uint32_t *rec_low)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_lines; j += stride) {
        const uint32_t len = line_len[j];
        if (len == 0) continue;
        const uint64_t rec = hdr_before[j] + line_hdr[j];  // (exclusive scan + own flag; a header line has len 0 anyway)
        atomicAdd(&rec_len[rec], (unsigned long long)len);
        atomicMin(&rec_first[rec], (uint32_t)j);
        if (line_low[j]) atomicAdd(&rec_low[rec], line_low[j]);
    }
}

__global__ void k_wa_rec_keep(const unsigned long long *__restrict__ rec_len, uint64_t n_rec, uint32_t *rec_keep, uint32_t *flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += stride) {
        rec_keep[r] = rec_len[r] ? 1u : 0u;
        if (rec_len[r] > WR_MAX_READ) atomicOr(flags, (uint32_t)TOK_BAD_STRUCTURE);
    }
}

// pass 3b: where in its record the first N n . of a line is; the least of them is the record's
__global__ void k_wa_lowpos(const unsigned long long *__restrict__ hdr_before, const uint32_t *__restrict__ line_hdr, const uint32_t *__restrict__ line_low,
                            const uint32_t *__restrict__ line_lowpos, const unsigned long long *__restrict__ out_off, const uint32_t *__restrict__ rec_first,
                            uint64_t n_lines, uint32_t *rec_lowpos)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_lines; j += stride) {
        if (line_low[j] == 0) continue;
        const uint64_t rec = hdr_before[j] + line_hdr[j];
        atomicMin(&rec_lowpos[rec], (uint32_t)(out_off[j] + line_lowpos[j] - out_off[rec_first[rec]]));
    }
}

// pass 3c: the reads' offsets and low-quality positions
__global__ void k_wa_reads(const uint32_t *__restrict__ rec_keep, const unsigned long long *__restrict__ rec_out, const uint32_t *__restrict__ rec_first,
                           const unsigned long long *__restrict__ out_off, const uint32_t *__restrict__ rec_low, const uint32_t *__restrict__ rec_lowpos,
                           uint64_t n_rec, uint64_t n_reads, uint64_t total_bases, uint64_t *offsets, int32_t *bad_pos)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += stride) {
        if (!rec_keep[r]) continue;
        const uint64_t o = rec_out[r];
        offsets[o] = out_off[rec_first[r]];
        bad_pos[o] = rec_low[r] == 0 ? -1 : rec_low[r] == 1 ? (int32_t)rec_lowpos[r] : -2;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[n_reads] = total_bases;
}

// pass 4: a wave a line packs it and stores its codes and phreds
__global__ void __launch_bounds__(T_THREADS) k_wa_pack(const uint8_t *__restrict__ t, uint64_t n, const unsigned long long *__restrict__ nl, uint64_t n_nl,
                                                      uint64_t n_lines, const uint32_t *__restrict__ line_len, const unsigned long long *__restrict__ out_off,
                                                      uint64_t *words, uint8_t *codes, uint8_t *phred)
{
    __shared__ uint64_t lds[T_THREADS / 64][WP_WORDS];
    const int lane = threadIdx.x & 63;
    WavePacker wp;
    wp.init(lds[threadIdx.x >> 6], words);
    uint32_t dummy = 0;
    for (uint64_t j = wave_index(); j < n_lines; j += wave_count()) {
        const uint32_t len = line_len[j];
        if (len == 0) continue;
        uint64_t s, e;
        uint8_t c0;
        wave_line_spans(t, n, nl, n_nl, j, 1, &s, &e, &c0);
        s = shfl64(s, 0);
        const uint64_t b0 = out_off[j];
        wp.open(b0);
        for (uint32_t q = 0; q < len; q += 64) {
            const bool in = q + lane < len;
            int code = 0, ph = 63;
            if (in) code = whole_base(t[s + q + lane], 0, false, 0, &ph, &dummy);
            (void)wp.put(in, code);
            if (in && codes) codes[b0 + q + lane] = (uint8_t)code;
            if (in && phred) phred[b0 + q + lane] = (uint8_t)ph;
        }
        wp.flush();
    }
}

// ---- joining device views: n_bases bases of a packed set, from base src0 on, behind dst0 bases of another.  A thread a word of
// the destination: 32 bases from the source's two words under it, cut to what is the new reads', shifted to their place.  A word
// that starts with new bases is stored whole (its tail zero, the pad word too); the one the old reads end in is ORed into.
__global__ void k_wr_append_words(const uint64_t *__restrict__ src, uint64_t src0, uint64_t n_bases, uint64_t *dst, uint64_t dst0)
{
    const uint64_t w_first = dst0 >> 5, w_end = ((dst0 + n_bases + 31) >> 5) + 1, dst_end = dst0 + n_bases;  // (+ 1: the pad word)
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = w_first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < w_end; w += stride) {
        const uint64_t lo = max(w * 32, dst0), hi = min(w * 32 + 32, dst_end);
        uint64_t v = 0;
        if (hi > lo) {
            const uint64_t sp = lo - dst0 + src0, wi = sp >> 5;
            const uint32_t sh = 2 * (uint32_t)(sp & 31), cnt = (uint32_t)(hi - lo);
            v = src[wi] << sh;
            if (sh) v |= src[wi + 1] >> (64 - sh);  // (the source has its pad word)
            if (cnt < 32) v &= ~(~0ull >> (2 * cnt));
            v >>= 2 * (uint32_t)(lo - w * 32);
        }
        if (lo == w * 32 || hi <= lo) dst[w] = v;
        else dst[w] |= v;  // (one thread a word, and what was there is from launches before this one)
    }
}

__global__ void k_wr_append_offsets(const uint64_t *__restrict__ src_off, uint64_t n_reads, uint64_t src0, uint64_t dst0, uint64_t *dst_off)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n_reads; r += stride) dst_off[r] = src_off[r] - src0 + dst0;
}

}  // namespace tok
}  // namespace mc

extern "C" int mc_reads_append_dev(mc_ctx *c, const uint64_t *d_words, const uint64_t *d_offsets, uint64_t n_reads, uint64_t *d_dst_words,
                                   uint64_t dst_bases, uint64_t *d_dst_offsets)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (n_reads && (!d_words || !d_offsets)) return fail(c, MC_EINVAL, "mc_reads_append_dev: null pointer");
    if (!d_dst_words || !d_dst_offsets) return fail(c, MC_EINVAL, "mc_reads_append_dev: null pointer");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    unsigned long long *h = c->h_scratch;
    h[0] = h[1] = 0;
    if (n_reads) {
        HIPCHK(c, hipMemcpyAsync(h, d_offsets, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(h + 1, d_offsets + n_reads, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    const uint64_t src0 = h[0], src_end = h[1];
    if (src_end < src0) return fail(c, MC_EINVAL, "mc_reads_append_dev: read_offsets run from %llu to %llu", h[0], h[1]);
    const uint64_t n_bases = src_end - src0, n_words = ((dst_bases + n_bases + 31) >> 5) + 1 - (dst_bases >> 5);
    if (n_bases)  // (no new base: the words stay as they are, the old reads' last word and pad word with them)
        hipLaunchKernelGGL(tok::k_wr_append_words, dim3(grid_for(n_words, 256, 1 << 16)), dim3(256), 0, c->stream, d_words, src0, n_bases, d_dst_words, dst_bases);
    if (n_reads)
        hipLaunchKernelGGL(tok::k_wr_append_offsets, dim3(grid_for(n_reads + 1, 256, 1 << 16)), dim3(256), 0, c->stream, d_offsets, n_reads, src0, dst_bases,
                           d_dst_offsets);
    else
        HIPCHK(c, hipMemcpyAsync(d_dst_offsets, &dst_bases, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MC_OK;
}

static const char *const WR_API = "mc_tokenize_whole";

extern "C" void mc_whole_reads_free(mc_ctx *c, mc_whole_reads *r)
{
    if (!r) return;
    if (c) (void)hipSetDevice(c->cfg.device);
    for (void *p : {(void *)r->d_words, (void *)r->d_offsets, (void *)r->d_bad_pos, (void *)r->d_codes, (void *)r->d_phred})
        if (p) (void)hipFree(p);
    *r = mc_whole_reads{};
}

extern "C" int mc_whole_reads_to_host(mc_ctx *c, const mc_whole_reads *r, uint64_t *words, uint64_t *offsets, int32_t *bad_pos, uint8_t *codes, uint8_t *phred)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (!r || r->declined || !r->d_offsets) return fail(c, MC_EINVAL, "mc_whole_reads_to_host: no result");
    if ((codes && !r->d_codes) || (phred && !r->d_phred)) return fail(c, MC_EINVAL, "mc_whole_reads_to_host: the result was made without that array");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (words) HIPCHK(c, hipMemcpy(words, r->d_words, ((r->n_bases + 31) / 32 + 1) * 8, hipMemcpyDeviceToHost));
    if (offsets) HIPCHK(c, hipMemcpy(offsets, r->d_offsets, (r->n_reads + 1) * 8, hipMemcpyDeviceToHost));
    if (bad_pos && r->n_reads) HIPCHK(c, hipMemcpy(bad_pos, r->d_bad_pos, r->n_reads * 4, hipMemcpyDeviceToHost));
    if (codes && r->n_bases) HIPCHK(c, hipMemcpy(codes, r->d_codes, r->n_bases, hipMemcpyDeviceToHost));
    if (phred && r->n_bases) HIPCHK(c, hipMemcpy(phred, r->d_phred, r->n_bases, hipMemcpyDeviceToHost));
    return MC_OK;
}

// the result's arrays for n_reads reads of n_bases bases, the words zeroed
static int wr_alloc(mc_ctx *c, uint64_t n_reads, uint64_t n_bases, uint32_t flags, mc_whole_reads *out)
{
    const uint64_t n_words = (n_bases + 31) / 32 + 1;
    HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&out->d_words), n_words * 8));
    HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&out->d_offsets), (n_reads + 1) * 8));
    HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&out->d_bad_pos), std::max<uint64_t>(n_reads, 1) * 4));
    if (flags & MC_WHOLE_CODES) HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&out->d_codes), std::max<uint64_t>(n_bases, 1)));
    if (flags & MC_WHOLE_PHRED) HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&out->d_phred), std::max<uint64_t>(n_bases, 1)));
    HIPCHK(c, hipMemsetAsync(out->d_words, 0, n_words * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(out->d_offsets, 0, 8, c->stream));  // (no reads: the one offset)
    out->n_reads = n_reads;
    out->n_bases = n_bases;
    return MC_OK;
}

// d_text: n bytes of text (a whole number of records) in a buffer padded with room for whole tiles of the newline pass; last: its
// last byte.  The context's lock is held.  Declined: *out stays zero but for `declined`.
static int whole_chunk_locked(mc_ctx *c, uint8_t *d_text, uint64_t n, char last, int format, int offset, uint32_t want, mc_whole_reads *out)
{
    const uint64_t n_padded = (n + tok::T_TILE - 1) / tok::T_TILE * tok::T_TILE;
    if (n_padded > n) HIPCHK(c, hipMemsetAsync(d_text + n, 0, n_padded - n, c->stream));
    PoolBuf<uint32_t> flags;
    HIPCHK(c, flags.alloc(&c->tok_pool, 1));
    HIPCHK(c, hipMemsetAsync(flags.p, 0, 4, c->stream));
    auto decline = [&] {
        out->declined = 1;
        return MC_OK;
    };
    auto read_flags = [&](uint32_t *fl) -> int {
        HIPCHK(c, hipMemcpyAsync(fl, flags.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return MC_OK;
    };
    TokNewlines nlb;
    PoolBuf<unsigned long long> &nl = nlb.nl;
    uint64_t n_nl = 0;
    bool too_many = false;
    int rc = tok_newlines(c, d_text, n, &nlb, &n_nl, &too_many);
    if (rc) return rc;
    if (too_many) return decline();
    const uint64_t n_lines = n_nl + (last != '\n' ? 1 : 0);
    if (n_lines >= 0xFFFFFFF0ull) return decline();
    uint32_t fl = 0;
    if (format == MC_WHOLE_FASTQ) {
        if (n_lines % 4) return decline();
        const uint64_t n_rec = n_lines / 4;
        PoolBuf<uint32_t> rec_len;
        PoolBuf<unsigned long long> base_at;
        HIPCHK(c, rec_len.alloc(&c->tok_pool, n_rec));
        HIPCHK(c, base_at.alloc(&c->tok_pool, n_rec));
        const int g = grid_for(n_rec, 4, 1 << 14);  // a wave per record
        hipLaunchKernelGGL(tok::k_wq_records, dim3(g), dim3(tok::T_THREADS), 0, c->stream, d_text, n, nl.p, n_nl, n_rec, offset, rec_len.p, flags.p);
        HIPCHK(c, hipGetLastError());
        uint64_t n_bases = 0;
        rc = tok_scan(c, rec_len.p, n_rec, base_at.p, &n_bases);
        if (rc) return rc;
        rc = read_flags(&fl);
        if (rc) return rc;
        if (fl) return decline();
        rc = wr_alloc(c, n_rec, n_bases, want, out);
        if (rc) return rc;
        hipLaunchKernelGGL(tok::k_wq_emit, dim3(g), dim3(tok::T_THREADS), 0, c->stream, d_text, n, nl.p, n_nl, n_rec, offset, base_at.p, n_bases, out->d_offsets,
                           out->d_words, out->d_bad_pos, out->d_codes, out->d_phred);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return MC_OK;
    }
    PoolBuf<uint32_t> line_hdr, line_len, line_low, line_lowpos, rec_first, rec_low, rec_lowpos, rec_keep;
    PoolBuf<unsigned long long> hdr_before, rec_len, out_off, rec_out;
    HIPCHK(c, line_hdr.alloc(&c->tok_pool, n_lines));
    HIPCHK(c, line_len.alloc(&c->tok_pool, n_lines));
    HIPCHK(c, line_low.alloc(&c->tok_pool, n_lines));
    HIPCHK(c, line_lowpos.alloc(&c->tok_pool, n_lines));
    HIPCHK(c, hdr_before.alloc(&c->tok_pool, n_lines));
    HIPCHK(c, out_off.alloc(&c->tok_pool, n_lines));
    const int gw = grid_for(n_lines, 4, 1 << 14), gt = grid_for(n_lines, 256, 1 << 16);
    hipLaunchKernelGGL(tok::k_wa_lines, dim3(gw), dim3(tok::T_THREADS), 0, c->stream, d_text, n, nl.p, n_nl, n_lines, line_hdr.p, line_len.p, line_low.p,
                       line_lowpos.p, flags.p);
    HIPCHK(c, hipGetLastError());
    uint64_t n_hdr = 0, n_bases = 0, n_reads = 0;
    rc = tok_scan(c, line_hdr.p, n_lines, hdr_before.p, &n_hdr);
    if (rc) return rc;
    rc = read_flags(&fl);
    if (rc) return rc;
    if (fl) return decline();
    const uint64_t n_rec = n_hdr + 1;  // (record 0: the lines in front of the first header)
    HIPCHK(c, rec_len.alloc(&c->tok_pool, n_rec));
    HIPCHK(c, rec_first.alloc(&c->tok_pool, n_rec));
    HIPCHK(c, rec_low.alloc(&c->tok_pool, n_rec));
    HIPCHK(c, rec_lowpos.alloc(&c->tok_pool, n_rec));
    HIPCHK(c, rec_keep.alloc(&c->tok_pool, n_rec));
    HIPCHK(c, rec_out.alloc(&c->tok_pool, n_rec));
    HIPCHK(c, hipMemsetAsync(rec_len.p, 0, n_rec * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(rec_first.p, 0xFF, n_rec * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(rec_low.p, 0, n_rec * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(rec_lowpos.p, 0xFF, n_rec * 4, c->stream));
    const int gr = grid_for(n_rec, 256, 1 << 16);
    hipLaunchKernelGGL(tok::k_wa_records, dim3(gt), dim3(256), 0, c->stream, hdr_before.p, line_hdr.p, line_len.p, line_low.p, n_lines, rec_len.p, rec_first.p,
                       rec_low.p);
    hipLaunchKernelGGL(tok::k_wa_rec_keep, dim3(gr), dim3(256), 0, c->stream, rec_len.p, n_rec, rec_keep.p, flags.p);
    HIPCHK(c, hipGetLastError());
    rc = tok_scan(c, line_len.p, n_lines, out_off.p, &n_bases);
    if (rc) return rc;
    rc = tok_scan(c, rec_keep.p, n_rec, rec_out.p, &n_reads);
    if (rc) return rc;
    rc = read_flags(&fl);
    if (rc) return rc;
    if (fl) return decline();
    hipLaunchKernelGGL(tok::k_wa_lowpos, dim3(gt), dim3(256), 0, c->stream, hdr_before.p, line_hdr.p, line_low.p, line_lowpos.p, out_off.p, rec_first.p, n_lines,
                       rec_lowpos.p);
    HIPCHK(c, hipGetLastError());
    rc = wr_alloc(c, n_reads, n_bases, want, out);
    if (rc) return rc;
    hipLaunchKernelGGL(tok::k_wa_reads, dim3(gr), dim3(256), 0, c->stream, rec_keep.p, rec_out.p, rec_first.p, out_off.p, rec_low.p, rec_lowpos.p, n_rec, n_reads,
                       n_bases, out->d_offsets, out->d_bad_pos);
    hipLaunchKernelGGL(tok::k_wa_pack, dim3(gw), dim3(tok::T_THREADS), 0, c->stream, d_text, n, nl.p, n_nl, n_lines, line_len.p, out_off.p, out->d_words,
                       out->d_codes, out->d_phred);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MC_OK;
}

static int wr_check(mc_ctx *c, const void *text, uint64_t n_bytes, int format, int phred_offset, uint32_t flags, mc_whole_reads *out)
{
    if (!out) return fail(c, MC_EINVAL, "%s: null pointer", WR_API);
    *out = mc_whole_reads{};
    if (n_bytes && !text) return fail(c, MC_EINVAL, "%s: null pointer", WR_API);
    if (format != MC_WHOLE_FASTA && format != MC_WHOLE_FASTQ) return fail(c, MC_EINVAL, "%s: format %d (MC_WHOLE_FASTA or MC_WHOLE_FASTQ)", WR_API, format);
    if (format == MC_WHOLE_FASTQ && phred_offset != 33 && phred_offset != 64) return fail(c, MC_EINVAL, "%s: phred offset %d (33 or 64)", WR_API, phred_offset);
    if (flags & ~(uint32_t)(MC_WHOLE_CODES | MC_WHOLE_PHRED)) return fail(c, MC_EINVAL, "%s: unknown flags 0x%x", WR_API, flags);
    return MC_OK;
}

// events around the passes (they wait for their scans' totals in between: the time on the stream, not a sum of kernel times)
static int wr_timed(mc_ctx *c, uint8_t *d_text, uint64_t n_bytes, char last, int format, int phred_offset, uint32_t flags, mc_whole_reads *out)
{
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    int rc = n_bytes ? whole_chunk_locked(c, d_text, n_bytes, last, format, phred_offset, flags, out) : wr_alloc(c, 0, 0, flags, out);
    if (rc == MC_OK && !out->declined) {
        HIPCHK(c, hipEventRecord(c->ev1, c->stream));
        HIPCHK(c, hipEventSynchronize(c->ev1));
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        out->device_ms = ms;
    }
    return rc;
}

extern "C" uint64_t mc_whole_text_bytes(uint64_t n_bytes) { return std::max<uint64_t>((n_bytes + tok::T_TILE - 1) / tok::T_TILE, 1) * tok::T_TILE; }

extern "C" int mc_tokenize_whole_dev(mc_ctx *c, uint8_t *d_text, uint64_t n_bytes, int last_byte, int format, int phred_offset, uint32_t flags,
                                     mc_whole_reads *out)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (int rc = wr_check(c, d_text, n_bytes, format, phred_offset, flags, out)) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc = wr_timed(c, d_text, n_bytes, (char)last_byte, format, phred_offset, flags, out);
    if (rc) mc_whole_reads_free(c, out);
    return rc;
}

extern "C" int mc_tokenize_whole(mc_ctx *c, const char *text, uint64_t n_bytes, int format, int phred_offset, uint32_t flags, mc_whole_reads *out)
{
    if (!c) return MC_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (int rc = wr_check(c, text, n_bytes, format, phred_offset, flags, out)) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    PoolBuf<uint8_t> d_text;
    if (n_bytes) {
        HIPCHK(c, d_text.alloc(&c->tok_pool, mc_whole_text_bytes(n_bytes)));
        if (int rc = h2d_fast(c, d_text.p, text, n_bytes)) return rc;
    }
    int rc = wr_timed(c, d_text.p, n_bytes, n_bytes ? text[n_bytes - 1] : '\n', format, phred_offset, flags, out);
    if (rc) mc_whole_reads_free(c, out);
    return rc;
}
