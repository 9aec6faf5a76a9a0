// f1: uncompressed FASTA / FASTQ text -> 2-bit packed reads ON THE GPU.
//
// The reference parses inside its dispatcher's lock, one thread for the whole file (src/io/ReadsDispatcher.java:34-53 ->
// itmo!/io/readers/FastaReader.java:54-104, FastqReader.java:53-82, FastaReaderFromXQSourceTrunc.java:61-95); the host
// reader of csrc/host/reads_io.cpp does it on all cores (~5 Gbases/s).  Here the file's bytes go to HBM as they are and
// a handful of data-parallel passes do the rest, with the reference's policy:
//   FASTA  a line that starts with '>' or ';' ends the record before it; the other lines of a record are concatenated
//          (a trailing '\r' comes off); a record with an N / n anywhere is dropped whole; empty records give nothing;
//   FASTQ  records of four lines (@id, bases, +, qualities); a base that is N n . or has phred < 1 (quality char minus
//          offset, 6 bits) ends a piece and is dropped, every non-empty piece is a read.
// Passes: (1) newline positions (count per tile, scan, write); (2) a wave per line (FASTA) or per record (FASTQ)
// classifies it and measures what it keeps; (3) scans turn the measures into read numbers and base offsets; (4) a wave
// per line / record packs the bases that stay, through LDS words of its own.  Anything out of the ordinary -- a byte that
// is no base, a FASTQ record whose lines do not look like one, a quality char outside [offset, 126] -- raises a flag and
// the CALLER reads the file with the host parser instead, which reproduces the reference's behaviour (and messages) in
// those cases.  Nothing here decides a result differently from the host reader: tests compare the tables.
#pragma once
#include "tokenizer_device.h"

namespace mc {
namespace tok {

__global__ void __launch_bounds__(T_THREADS) k_scan_sums(const uint32_t *__restrict__ in, uint64_t n, unsigned long long *tile_sums)
{
    __shared__ uint32_t lw[T_THREADS / 64];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
    uint32_t s = 0;
    for (uint32_t i = threadIdx.x; i < SCAN_TILE; i += T_THREADS) s += base + i < n ? in[base + i] : 0u;
    uint32_t tot;
    (void)block_excl_scan(s, lw, &tot);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = tot;
}

// exclusive scan of `m` 64-bit values in place by ONE workgroup; total -> *total
__global__ void __launch_bounds__(1024) k_scan_one(unsigned long long *v, uint64_t m, unsigned long long *total)
{
    __shared__ unsigned long long part[1024];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint64_t b = 0; b < m; b += 1024) {
        const uint64_t i = b + threadIdx.x;
        const unsigned long long x = i < m ? v[i] : 0ull;
        part[threadIdx.x] = x;
        __syncthreads();
        for (uint32_t o = 1; o < 1024; o <<= 1) {  // Hillis-Steele
            const unsigned long long y = threadIdx.x >= o ? part[threadIdx.x - o] : 0ull;
            __syncthreads();
            part[threadIdx.x] += y;
            __syncthreads();
        }
        if (i < m) v[i] = carry + part[threadIdx.x] - x;
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ void __launch_bounds__(T_THREADS) k_scan_apply(const uint32_t *__restrict__ in, uint64_t n, const unsigned long long *__restrict__ tile_off,
                                                         unsigned long long *out)
{
    __shared__ uint32_t lw[T_THREADS / 64];
    constexpr uint32_t PER = SCAN_TILE / T_THREADS;  // consecutive elements per thread
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * PER;
    uint32_t vals[PER], s = 0;
#pragma unroll
    for (uint32_t i = 0; i < PER; i++) { vals[i] = base + i < n ? in[base + i] : 0u; s += vals[i]; }
    uint32_t tot;
    uint64_t at = tile_off[blockIdx.x] + block_excl_scan(s, lw, &tot);
#pragma unroll
    for (uint32_t i = 0; i < PER; i++) {
        if (base + i < n) out[base + i] = at;
        at += vals[i];
    }
}

// ---- pass 1: where the newlines are.  The text buffer is padded with zero bytes to a whole number of tiles, so a
// thread takes its 32 bytes as two 16-byte loads (a wave reads 2 KB in a row).
__device__ __forceinline__ uint32_t nl_bits4(uint32_t v)
{   // bit i set when byte i of v is '\n' (exact: no borrow between bytes)
    const uint32_t x = v ^ 0x0A0A0A0Au;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu) >> 7;  // 1 at bit 8i for a zero byte i
    return (z | z >> 7 | z >> 14 | z >> 21) & 0xFu;
}
__device__ __forceinline__ uint32_t nl_bits32(const uint8_t *__restrict__ t, uint64_t base)
{
    const uint4 a = *reinterpret_cast<const uint4 *>(t + base), b = *reinterpret_cast<const uint4 *>(t + base + 16);
    return nl_bits4(a.x) | nl_bits4(a.y) << 4 | nl_bits4(a.z) << 8 | nl_bits4(a.w) << 12 | nl_bits4(b.x) << 16 | nl_bits4(b.y) << 20 |
           nl_bits4(b.z) << 24 | nl_bits4(b.w) << 28;
}

__global__ void __launch_bounds__(T_THREADS) k_nl_count(const uint8_t *__restrict__ t, uint32_t *tile_counts)
{
    __shared__ uint32_t lw[T_THREADS / 64];
    const uint64_t base = (uint64_t)blockIdx.x * T_TILE + (uint64_t)threadIdx.x * T_BYTES;
    uint32_t tot;
    (void)block_excl_scan((uint32_t)__popc(nl_bits32(t, base)), lw, &tot);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(T_THREADS) k_nl_write(const uint8_t *__restrict__ t, const unsigned long long *__restrict__ tile_off, unsigned long long *nl)
{
    __shared__ uint32_t lw[T_THREADS / 64];
    const uint64_t base = (uint64_t)blockIdx.x * T_TILE + (uint64_t)threadIdx.x * T_BYTES;
    uint32_t mask = nl_bits32(t, base);
    uint32_t tot;
    uint64_t at = tile_off[blockIdx.x] + block_excl_scan((uint32_t)__popc(mask), lw, &tot);
    for (; mask; mask &= mask - 1) nl[at++] = base + (uint32_t)__builtin_ctz(mask);
}


// ---- FASTA, pass 2: a wave per line
__global__ void __launch_bounds__(T_THREADS) k_fa_lines(const uint8_t *__restrict__ t, uint64_t n, const unsigned long long *__restrict__ nl, uint64_t n_nl,
                                                       uint64_t n_lines, uint32_t *line_hdr, uint32_t *line_len, uint8_t *line_n, uint32_t *flags)
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
        bool has_n = false;
        if (!hdr) {
            for (uint64_t i = s + lane; i < e; i += 64) {
                const uint8_t c = t[i];
                if (c == 'N' || c == 'n') has_n = true;
                else if (base_code(c) < 0) bad |= TOK_BAD_CHAR;
            }
            has_n = __ballot(has_n) != 0;
            if (e - s > 0xFFFFFFF0ull) bad |= TOK_BAD_STRUCTURE;  // (a line of 4 G bases: not for this path)
        }
        if (lane == 0) {
            line_hdr[j] = hdr ? 1u : 0u;
            line_len[j] = hdr ? 0u : (uint32_t)(e - s);
            line_n[j] = has_n ? 1 : 0;
        }
    }
    if (bad) atomicOr(flags, bad);
}

// pass 3a: per record (rec = headers at or before the line): does it hold an N, how long is it, which line opens it
__global__ void k_fa_records(const unsigned long long *__restrict__ hdr_before, const uint32_t *__restrict__ line_hdr, const uint32_t *__restrict__ line_len,
                             const uint8_t *__restrict__ line_n, uint64_t n_lines, uint8_t *rec_n, unsigned long long *rec_len, uint32_t *rec_first)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_lines; j += stride) {
        const uint32_t len = line_len[j];
        if (len == 0) continue;
        const uint64_t rec = hdr_before[j] + line_hdr[j];  // (exclusive scan + own flag; a header line has len 0 anyway)
        if (line_n[j]) rec_n[rec] = 1;
        atomicAdd(&rec_len[rec], (unsigned long long)len);
        atomicMin(&rec_first[rec], (uint32_t)j);
    }
}

// pass 3b: what a line contributes once the records with N are gone
__global__ void k_fa_keep(const unsigned long long *__restrict__ hdr_before, const uint32_t *__restrict__ line_hdr, const uint32_t *__restrict__ line_len,
                          uint64_t n_lines, const uint8_t *__restrict__ rec_n, uint32_t *keep_len)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_lines; j += stride) {
        const uint64_t rec = hdr_before[j] + line_hdr[j];
        keep_len[j] = rec_n[rec] ? 0u : line_len[j];
    }
}

__global__ void k_fa_rec_keep(const uint8_t *__restrict__ rec_n, const unsigned long long *__restrict__ rec_len, uint64_t n_rec, uint32_t *rec_keep)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += stride) rec_keep[r] = !rec_n[r] && rec_len[r] ? 1u : 0u;
}

__global__ void k_fa_offsets(const uint32_t *__restrict__ rec_keep, const unsigned long long *__restrict__ rec_out, const uint32_t *__restrict__ rec_first,
                             const unsigned long long *__restrict__ out_off, uint64_t n_rec, uint64_t n_reads, uint64_t total_bases, uint64_t *offsets,
                             uint64_t dst_base)
{   // dst_base: where this chunk's first base goes in the output (the chunks of a file are packed back to back)
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += stride)
        if (rec_keep[r]) offsets[rec_out[r]] = dst_base + out_off[rec_first[r]];
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[n_reads] = dst_base + total_bases;
}

// pass 4: a wave per line packs it
__global__ void __launch_bounds__(T_THREADS) k_fa_pack(const uint8_t *__restrict__ t, uint64_t n, const unsigned long long *__restrict__ nl, uint64_t n_nl,
                                                      uint64_t n_lines, const uint32_t *__restrict__ keep_len, const unsigned long long *__restrict__ out_off,
                                                      uint64_t *words, uint32_t *flags, uint64_t dst_base)
{
    __shared__ uint64_t lds[T_THREADS / 64][WP_WORDS];
    const int lane = threadIdx.x & 63;
    WavePacker wp;
    wp.init(lds[threadIdx.x >> 6], words);
    uint32_t bad = 0;
    for (uint64_t j = wave_index(); j < n_lines; j += wave_count()) {
        const uint32_t len = keep_len[j];
        if (len == 0) continue;
        uint64_t s, e;
        uint8_t c0;
        wave_line_spans(t, n, nl, n_nl, j, 1, &s, &e, &c0);
        s = shfl64(s, 0);
        wp.open(dst_base + out_off[j]);
        for (uint32_t q = 0; q < len; q += 64) {
            const bool in = q + lane < len;
            const int c = in ? base_code(t[s + q + lane]) : -1;
            if (in && c < 0) bad |= TOK_BAD_CHAR;
            (void)wp.put(in && c >= 0, c);
        }
        wp.flush();
    }
    if (bad) atomicOr(flags, bad);
}

// ---- FASTQ: a wave per record (lines 4r .. 4r + 3)
__device__ __forceinline__ bool fq_bad_base(uint8_t c, uint8_t q, int offset, uint32_t *flags_acc)
{
    if (c == 'N' || c == 'n' || c == '.') return true;
    if (base_code(c) < 0) { *flags_acc |= TOK_BAD_CHAR; return true; }
    if ((int)q < offset || q > 126) { *flags_acc |= TOK_BAD_QUALITY; return true; }
    return (((int)q - offset) & 63) < 1;  // the phred lives in 6 bits (DnaQBuilder.java:32-35): 64 wraps to 0
}


// pass 2: structure, pieces and kept bases of every record
__global__ void __launch_bounds__(T_THREADS) k_fq_records(const uint8_t *__restrict__ t, uint64_t n, const unsigned long long *__restrict__ nl, uint64_t n_nl,
                                                         uint64_t n_rec, int offset, uint32_t *rec_pieces, uint32_t *rec_bases, uint32_t *flags)
{
    const int lane = threadIdx.x & 63;
    uint32_t bad = 0;
    for (uint64_t r = wave_index(); r < n_rec; r += wave_count()) {
        const FqRecord R = fq_record(t, n, nl, n_nl, r);
        uint32_t pieces = 0, bases = 0;
        if (!R.ok) {
            bad |= TOK_BAD_STRUCTURE;
        } else {
            uint64_t carry = 0;  // was the base in front of this stretch of 64 a good one
            for (uint64_t q = 0; q < R.len; q += 64) {
                const bool in = q + lane < R.len;
                const bool good = in && !fq_bad_base(t[R.s1 + q + lane], t[R.s3 + q + lane], offset, &bad);
                const uint64_t gm = __ballot(good);
                pieces += (uint32_t)__popcll(gm & ~(gm << 1 | carry));
                bases += (uint32_t)__popcll(gm);
                carry = gm >> 63;
            }
        }
        if (lane == 0) {
            rec_pieces[r] = pieces;
            rec_bases[r] = bases;
        }
    }
    if (bad) atomicOr(flags, bad);
}

// pass 4: the read offset of every piece, and its bases packed
__global__ void __launch_bounds__(T_THREADS) k_fq_emit(const uint8_t *__restrict__ t, uint64_t n, const unsigned long long *__restrict__ nl, uint64_t n_nl,
                                                      uint64_t n_rec, int offset, const unsigned long long *__restrict__ piece_at,
                                                      const unsigned long long *__restrict__ base_at, const uint32_t *__restrict__ rec_bases, uint64_t n_reads,
                                                      uint64_t total_bases, uint64_t *offsets, uint64_t *words, uint64_t dst_base)
{
    __shared__ uint64_t lds[T_THREADS / 64][WP_WORDS];
    const int lane = threadIdx.x & 63;
    WavePacker wp;
    wp.init(lds[threadIdx.x >> 6], words);
    uint32_t dummy = 0;
    for (uint64_t r = wave_index(); r < n_rec; r += wave_count()) {
        if (rec_bases[r] == 0) continue;
        const FqRecord R = fq_record(t, n, nl, n_nl, r);
        uint64_t p = piece_at[r], carry = 0;
        wp.open(dst_base + base_at[r]);
        for (uint64_t q = 0; q < R.len; q += 64) {
            const bool in = q + lane < R.len;
            const uint8_t c = in ? t[R.s1 + q + lane] : 0;
            const bool good = in && !fq_bad_base(c, t[R.s3 + q + lane], offset, &dummy);
            const uint64_t gm = __ballot(good);
            const uint64_t starts = gm & ~(gm << 1 | carry);
            const uint64_t b = wp.put(good, good ? base_code(c) : 0);
            if (starts >> lane & 1) offsets[p + (uint64_t)__popcll(starts & lanes_below())] = b;
            p += (uint64_t)__popcll(starts);
            carry = gm >> 63;
        }
        wp.flush();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[n_reads] = dst_base + total_bases;
}

}  // namespace tok
}  // namespace mc
