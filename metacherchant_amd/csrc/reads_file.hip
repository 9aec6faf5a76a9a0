// libmcgpu.so, f1 on the device: csrc/tokenizer.h driven over the chunks of an uncompressed FASTA / FASTQ file, and
// mc_add_reads_file.
#include <chrono>
#include <thread>

#include "context.h"
#include "tokenizer.h"
#include "host/reads_io.h"

// exclusive scan of n 32-bit counts into 64-bit offsets; *total on the host
int tok_scan(mc_ctx *c, const uint32_t *d_in, uint64_t n, unsigned long long *d_out, uint64_t *total)
{
    const uint64_t m = std::max<uint64_t>((n + tok::SCAN_TILE - 1) / tok::SCAN_TILE, 1);
    PoolBuf<unsigned long long> sums;
    HIPCHK(c, sums.alloc(&c->tok_pool, m + 1));
    hipLaunchKernelGGL(tok::k_scan_sums, dim3((unsigned)m), dim3(tok::T_THREADS), 0, c->stream, d_in, n, sums.p);
    hipLaunchKernelGGL(tok::k_scan_one, dim3(1), dim3(1024), 0, c->stream, sums.p, m, sums.p + m);
    hipLaunchKernelGGL(tok::k_scan_apply, dim3((unsigned)m), dim3(tok::T_THREADS), 0, c->stream, d_in, n, sums.p, d_out);
    HIPCHK(c, hipGetLastError());
    unsigned long long t = 0;
    HIPCHK(c, hipMemcpyAsync(&t, sums.p + m, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *total = t;
    return MC_OK;
}

// pass 1 of both tokenisers: the positions of the n_nl newlines of d_text[0, n), which is padded with zero bytes to whole tiles
int tok_newlines(mc_ctx *c, const uint8_t *d_text, uint64_t n, TokNewlines *b, uint64_t *n_nl, bool *too_many)
{
    *too_many = false;
    *n_nl = 0;
    const uint64_t n_tiles = (n + tok::T_TILE - 1) / tok::T_TILE;
    if (n_tiles > 0x7FFFFFFFull) { *too_many = true; return MC_OK; }
    HIPCHK(c, b->tile_counts.alloc(&c->tok_pool, n_tiles));
    HIPCHK(c, b->tile_off.alloc(&c->tok_pool, n_tiles));
    hipLaunchKernelGGL(tok::k_nl_count, dim3((unsigned)n_tiles), dim3(tok::T_THREADS), 0, c->stream, d_text, b->tile_counts.p);
    int rc = tok_scan(c, b->tile_counts.p, n_tiles, b->tile_off.p, n_nl);
    if (rc) return rc;
    HIPCHK(c, b->nl.alloc(&c->tok_pool, *n_nl));
    hipLaunchKernelGGL(tok::k_nl_write, dim3((unsigned)n_tiles), dim3(tok::T_THREADS), 0, c->stream, d_text, b->tile_off.p, b->nl.p);
    HIPCHK(c, hipGetLastError());
    return MC_OK;
}

static int tok_flush_locked(mc_ctx *c, TokPending &P)
{
    if (P.reads == 0) { P.base_word = -1; P.bases = 0; return MC_OK; }
    if ((uint64_t)P.base_word != c->rs_bases / 32)  // (the chunks sit behind the store's end until they are counted)
        return fail(c, MC_ESTATE, "mc_add_reads_file: the context took other reads while a file was being read");
    int rc = add_reads_dev_locked(c, c->rs_words + P.base_word, P.off.p, P.reads, P.bases, P.base_word);
    if (!rc) HIPCHK(c, hipStreamSynchronize(c->stream));
    P.reads = P.bases = 0;
    P.base_word = -1;
    return rc;
}

// Text bytes [b, e) of a mapped file (a whole number of records) -> packed reads in HBM -> counted.  *declined: the
// device saw something the host parser has to deal with; nothing was added.  The context's lock is held.
int tokenize_chunk_locked(mc_ctx *c, const mch::PlainReadsFile &f, const char *b, const char *e, uint8_t *d_text, uint64_t *n_reads_out,
                          bool *declined, TokPending *pend)
{
    *declined = false;
    *n_reads_out = 0;
    const uint64_t n = (uint64_t)(e - b);
    if (n == 0) return MC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const bool dbg = c->sw.ingest_debug;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t1 = now();
    struct { uint8_t *p; } text{d_text};  // (padded with zero bytes to whole tiles of the newline passes: tok_text_bytes)
    {
        const uint64_t n_padded = (n + tok::T_TILE - 1) / tok::T_TILE * tok::T_TILE;
        if (n_padded > n) HIPCHK(c, hipMemsetAsync(text.p + n, 0, n_padded - n, c->stream));
    }
    int rc = MC_OK;
    PoolBuf<uint32_t> flags;
    HIPCHK(c, flags.alloc(&c->tok_pool, 1));
    HIPCHK(c, hipMemsetAsync(flags.p, 0, 4, c->stream));
    // pass 1: newline positions
    TokNewlines nlb;  // (as before: the pass's buffers live as long as this call, and nothing waits for the pass here)
    PoolBuf<unsigned long long> &nl = nlb.nl;
    uint64_t n_nl = 0;
    bool too_many = false;
    rc = tok_newlines(c, text.p, n, &nlb, &n_nl, &too_many);
    if (rc) return rc;
    if (too_many) { *declined = true; return MC_OK; }
    const uint64_t n_lines = n_nl + (e[-1] != '\n' ? 1 : 0);
    if (n_lines >= 0xFFFFFFF0ull) { *declined = true; return MC_OK; }

    auto read_flags = [&](uint32_t *out) -> int {
        HIPCHK(c, hipMemcpyAsync(out, flags.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return MC_OK;
    };
    // where the packed words go: straight into the read store when the context keeps one
    PoolBuf<uint64_t> own_words;
    PoolBuf<uint64_t> offsets;
    uint64_t *dst = nullptr;
    int64_t in_store = -1;
    uint64_t dst_base = 0;  // this chunk's first base in `dst` (deferred counting: behind the chunks before it)
    uint64_t *off_out = nullptr;
    const bool defer = pend != nullptr && c->rs_enabled;
    auto reserve_words = [&](uint64_t total_bases, uint64_t n_reads_chunk) -> int {
        const uint64_t n_words = (total_bases + 31) / 32 + 1;
        if (defer) {
            if (pend->base_word < 0) { pend->base_word = (int64_t)(c->rs_bases / 32); pend->bases = 0; pend->reads = 0; }
            if ((uint64_t)pend->base_word != c->rs_bases / 32)
                return fail(c, MC_ESTATE, "mc_add_reads_file: the context took other reads while a file was being read");
            dst_base = pend->bases;
            // (the caller reserved the store for the whole file: no reallocation may move the chunks packed so far)
            if ((uint64_t)pend->base_word + (dst_base + total_bases + 31) / 32 + 2 > c->rs_cap_words)
                return fail(c, MC_EINVAL, "internal: the read store was not reserved for the whole file");
            dst = c->rs_words + pend->base_word;
            in_store = pend->base_word;
            const uint64_t first_new = (dst_base + 31) / 32;  // words before it hold bases of earlier chunks
            HIPCHK(c, hipMemsetAsync(dst + first_new, 0, ((dst_base + total_bases + 31) / 32 + 1 - first_new) * 8, c->stream));
            const uint64_t need = pend->reads + n_reads_chunk + 1;
            if (need > pend->off_cap) {
                PoolBuf<uint64_t> bigger;
                const uint64_t cap = std::max<uint64_t>(need * 2, 1u << 20);
                HIPCHK(c, bigger.alloc(&c->tok_pool, cap));
                if (pend->reads) HIPCHK(c, hipMemcpyAsync(bigger.p, pend->off.p, (pend->reads + 1) * 8, hipMemcpyDeviceToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                std::swap(pend->off.p, bigger.p);
                std::swap(pend->off.bytes, bigger.bytes);
                std::swap(pend->off.pool, bigger.pool);
                pend->off_cap = cap;
            }
            off_out = pend->off.p + pend->reads;
            return MC_OK;
        }
        if (c->rs_enabled) {
            int r = rs_reserve(c, n_words);
            if (r) return r;
            in_store = (int64_t)(c->rs_bases / 32);
            dst = c->rs_words + in_store;
        } else {
            HIPCHK(c, own_words.alloc(&c->tok_pool, n_words));
            dst = own_words.p;
        }
        HIPCHK(c, hipMemsetAsync(dst, 0, n_words * 8, c->stream));
        return MC_OK;
    };
    uint64_t n_reads = 0, total_bases = 0;
    uint32_t fl = 0;
    if (!f.fastq) {
        PoolBuf<uint32_t> line_hdr, line_len, keep_len, rec_first, rec_keep;
        PoolBuf<uint8_t> line_n, rec_n;
        PoolBuf<unsigned long long> hdr_before, rec_len, out_off, rec_out;
        HIPCHK(c, line_hdr.alloc(&c->tok_pool, n_lines));
        HIPCHK(c, line_len.alloc(&c->tok_pool, n_lines));
        HIPCHK(c, line_n.alloc(&c->tok_pool, n_lines));
        HIPCHK(c, hdr_before.alloc(&c->tok_pool, n_lines));
        hipLaunchKernelGGL(tok::k_fa_lines, dim3(grid_for(n_lines, 4, 1 << 14)), dim3(tok::T_THREADS), 0, c->stream, text.p, n, nl.p, n_nl, n_lines, line_hdr.p,
                           line_len.p, line_n.p, flags.p);
        uint64_t n_hdr = 0;
        rc = tok_scan(c, line_hdr.p, n_lines, hdr_before.p, &n_hdr);
        if (rc) return rc;
        rc = read_flags(&fl);
        if (rc) return rc;
        if (fl) { *declined = true; return MC_OK; }
        const uint64_t n_rec = n_hdr + 1;  // (record 0: the lines in front of the first header)
        HIPCHK(c, rec_n.alloc(&c->tok_pool, n_rec));
        HIPCHK(c, rec_len.alloc(&c->tok_pool, n_rec));
        HIPCHK(c, rec_first.alloc(&c->tok_pool, n_rec));
        HIPCHK(c, rec_keep.alloc(&c->tok_pool, n_rec));
        HIPCHK(c, rec_out.alloc(&c->tok_pool, n_rec));
        HIPCHK(c, keep_len.alloc(&c->tok_pool, n_lines));
        HIPCHK(c, out_off.alloc(&c->tok_pool, n_lines));
        HIPCHK(c, hipMemsetAsync(rec_n.p, 0, n_rec, c->stream));
        HIPCHK(c, hipMemsetAsync(rec_len.p, 0, n_rec * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(rec_first.p, 0xFF, n_rec * 4, c->stream));
        const int g = grid_for(n_lines, 256, 1 << 16);
        hipLaunchKernelGGL(tok::k_fa_records, dim3(g), dim3(256), 0, c->stream, hdr_before.p, line_hdr.p, line_len.p, line_n.p, n_lines, rec_n.p, rec_len.p,
                           rec_first.p);
        hipLaunchKernelGGL(tok::k_fa_keep, dim3(g), dim3(256), 0, c->stream, hdr_before.p, line_hdr.p, line_len.p, n_lines, rec_n.p, keep_len.p);
        hipLaunchKernelGGL(tok::k_fa_rec_keep, dim3(grid_for(n_rec, 256, 1 << 16)), dim3(256), 0, c->stream, rec_n.p, rec_len.p, n_rec, rec_keep.p);
        rc = tok_scan(c, keep_len.p, n_lines, out_off.p, &total_bases);
        if (rc) return rc;
        rc = tok_scan(c, rec_keep.p, n_rec, rec_out.p, &n_reads);
        if (rc) return rc;
        if (n_reads) {
            rc = reserve_words(total_bases, n_reads);
            if (rc) return rc;
            if (!off_out) { HIPCHK(c, offsets.alloc(&c->tok_pool, n_reads + 1)); off_out = offsets.p; }
            hipLaunchKernelGGL(tok::k_fa_offsets, dim3(grid_for(n_rec, 256, 1 << 16)), dim3(256), 0, c->stream, rec_keep.p, rec_out.p, rec_first.p, out_off.p,
                               n_rec, n_reads, total_bases, off_out, dst_base);
            hipLaunchKernelGGL(tok::k_fa_pack, dim3(grid_for(n_lines, 4, 1 << 14)), dim3(tok::T_THREADS), 0, c->stream, text.p, n, nl.p, n_nl,
                               n_lines, keep_len.p, out_off.p, dst, flags.p, dst_base);
            HIPCHK(c, hipGetLastError());
        }
    } else {
        if (n_lines % 4) { *declined = true; return MC_OK; }
        const uint64_t n_rec = n_lines / 4;
        PoolBuf<uint32_t> rec_pieces, rec_bases;
        PoolBuf<unsigned long long> piece_at, base_at;
        HIPCHK(c, rec_pieces.alloc(&c->tok_pool, n_rec));
        HIPCHK(c, rec_bases.alloc(&c->tok_pool, n_rec));
        HIPCHK(c, piece_at.alloc(&c->tok_pool, n_rec));
        HIPCHK(c, base_at.alloc(&c->tok_pool, n_rec));
        const int g = grid_for(n_rec, 4, 1 << 14);  // a wave per record
        hipLaunchKernelGGL(tok::k_fq_records, dim3(g), dim3(tok::T_THREADS), 0, c->stream, text.p, n, nl.p, n_nl, n_rec, f.offset, rec_pieces.p, rec_bases.p,
                           flags.p);
        rc = tok_scan(c, rec_pieces.p, n_rec, piece_at.p, &n_reads);
        if (rc) return rc;
        rc = tok_scan(c, rec_bases.p, n_rec, base_at.p, &total_bases);
        if (rc) return rc;
        rc = read_flags(&fl);
        if (rc) return rc;
        if (fl) { *declined = true; return MC_OK; }
        if (n_reads) {
            rc = reserve_words(total_bases, n_reads);
            if (rc) return rc;
            if (!off_out) { HIPCHK(c, offsets.alloc(&c->tok_pool, n_reads + 1)); off_out = offsets.p; }
            hipLaunchKernelGGL(tok::k_fq_emit, dim3(g), dim3(tok::T_THREADS), 0, c->stream, text.p, n, nl.p, n_nl, n_rec, f.offset, piece_at.p, base_at.p,
                               rec_bases.p, n_reads, total_bases, off_out, dst, dst_base);
            HIPCHK(c, hipGetLastError());
        }
    }
    rc = read_flags(&fl);
    if (rc) return rc;
    if (fl) { *declined = true; return MC_OK; }  // (cannot happen after the line pass; the read store was not advanced)
    const double t2 = now();
    if (n_reads && defer) {  // counted with the rest of the file (tok_flush_locked)
        pend->reads += n_reads;
        pend->bases += total_bases;
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (the text buffer goes back to its pool)
    } else if (n_reads) {
        rc = add_reads_dev_locked(c, dst, off_out, n_reads, total_bases, in_store);
        if (rc) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (dbg)
        fprintf(stderr, "[ingest] device tokeniser: %.1f MB text, %llu lines, %llu reads, %llu bases: tokenise %.3f s, count %.3f s\n", n / 1e6,
                (unsigned long long)n_lines, (unsigned long long)n_reads, (unsigned long long)total_bases, t2 - t1, now() - t2);
    *n_reads_out = n_reads;
    return MC_OK;
}

namespace {
// The two uploads of a file in flight and the reads its chunks have gathered, with the context whose pool their blocks come from:
// whichever way the driver below is left (the host parser may throw), the helper threads are joined and the blocks go back under
// that context's lock.
struct FileInFlight {
    struct Upload { PoolBuf<uint8_t> text; std::thread th; bool ok = true; };
    mc_ctx *c;
    std::unique_ptr<Upload> cur, nxt;
    std::unique_ptr<TokPending> pend{new TokPending};
    explicit FileInFlight(mc_ctx *ctx) : c(ctx) {}
    ~FileInFlight()
    {
        release(cur);
        release(nxt);
        std::lock_guard<std::mutex> g(c->mu);
        pend.reset();
    }
    // the bytes [b, e) of f start on their way into a block of u's own
    int start(std::unique_ptr<Upload> &u, const mch::PlainReadsFile &f, const char *b, const char *e)
    {
        u.reset(new Upload);
        const uint64_t n = (uint64_t)(e - b);
        {
            std::lock_guard<std::mutex> g(c->mu);
            HIPCHK(c, hipSetDevice(c->cfg.device));
            HIPCHK(c, u->text.alloc(&c->tok_pool, (n + tok::T_TILE - 1) / tok::T_TILE * tok::T_TILE));
        }
        Upload *up = u.get();
        mc_ctx *ctx = c;
        up->th = std::thread([ctx, up, b, n, &f] { up->ok = h2d_pinned(ctx, up->text.p, b, n, f.fd, (uint64_t)(b - f.p)); });
        return MC_OK;
    }
    void release(std::unique_ptr<Upload> &u)
    {
        if (!u) return;
        if (u->th.joinable()) u->th.join();
        std::lock_guard<std::mutex> g(c->mu);
        u.reset();
    }
};
}  // namespace

// Chunks of 256 MB: the bytes of chunk i + 1 cross the link (a helper thread, pinned staging buffers) while the kernels tokenise
// chunk i.  The context's lock is taken per step, never around the host parser or the caller's flush, host_batch and after_chunk.
int tokenize_file_chunks(mc_ctx *c, const mch::PlainReadsFile &f, const FileCuts &cuts, const FileChunkOps &ops, uint64_t *n_reads)
{
    auto own = [&](int rc) { return rc != MC_OK && ops.ctx_failed ? ops.ctx_failed(rc) : rc; };
    if (c->rs_enabled) {  // the read store grows once, not chunk by chunk (FASTA: a base a byte at most; FASTQ: half that)
        std::lock_guard<std::mutex> g(c->mu);
        const int r = [&]() -> int {
            HIPCHK(c, hipSetDevice(c->cfg.device));
            return rs_reserve(c, (f.fastq ? f.n / 2 : f.n) / 32 + 2 * cuts.size() + 2);
        }();
        if (r) return own(r);
    }
    FileInFlight fl(c);
    uint64_t total = 0;
    int rc = cuts.empty() ? MC_OK : own(fl.start(fl.cur, f, cuts[0].first, cuts[0].second));
    for (size_t i = 0; i < cuts.size() && rc == MC_OK; i++) {
        fl.cur->th.join();
        if (!fl.cur->ok) {
            std::lock_guard<std::mutex> g(c->mu);
            rc = own(fail(c, MC_EHIP, "%s: host-to-device copy failed", ops.who));
            break;
        }
        if (i + 1 < cuts.size() && (rc = own(fl.start(fl.nxt, f, cuts[i + 1].first, cuts[i + 1].second))) != MC_OK) break;
        uint64_t got = 0;
        bool declined = false;
        {
            std::lock_guard<std::mutex> g(c->mu);
            rc = own(tokenize_chunk_locked(c, f, cuts[i].first, cuts[i].second, fl.cur->text.p, &got, &declined, fl.pend.get()));
        }
        if (rc != MC_OK) break;
        if (declined) {  // (what was gathered goes first: the host's batches are appended behind what is counted)
            if ((rc = ops.flush(*fl.pend)) != MC_OK) break;
            got = mch::parse_plain_range(f, cuts[i].first, cuts[i].second, ops.batch_reads, [&](mch::PackedBatch &b) {
                if (rc == MC_OK) rc = ops.host_batch(b);
            });
            if (rc != MC_OK) break;
        }
        total += got;
        if ((rc = ops.after_chunk(i, cuts.size(), *fl.pend)) != MC_OK) break;
        fl.release(fl.cur);
        fl.cur = std::move(fl.nxt);
    }
    if (rc == MC_OK) rc = ops.flush(*fl.pend);  // (no upload is left by now)
    if (rc == MC_OK) *n_reads = total;
    return rc;
}

extern "C" int mc_add_reads_file(mc_ctx *c, const char *path, uint64_t *n_reads)
{
    if (!c) return MC_EINVAL;
    if (n_reads) *n_reads = 0;
    if (!path) return fail(c, MC_EINVAL, "mc_add_reads_file: null path");
    try {
        int rc = MC_OK;
        auto add_batch = [c](mch::PackedBatch &b) { return mc_add_reads_packed(c, b.words.data(), b.offsets.data(), b.n_reads()); };
        // Uncompressed FASTA / FASTQ: the bytes go to the device in chunks cut at record starts and are tokenised there
        // (csrc/tokenizer.h); a chunk the device declines goes through the host parser, as does any other kind of file
        // (MC_TOKENIZER=host: every file).  Host batches hold 2^20 reads; the context's lock is taken per batch / chunk.
        mch::PlainReadsFile f;
        if (!c->sw.tokenizer_host && mch::map_plain_reads(path, &f)) {
            const bool dbg = c->sw.ingest_debug;
            auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
            const double t_begin = now();
            const auto cuts = mch::plain_chunks(f, c->sw.tokenizer_chunk_bytes);
            FileChunkOps ops;
            ops.who = "mc_add_reads_file";
            ops.flush = [c](TokPending &P) { std::lock_guard<std::mutex> g(c->mu); return tok_flush_locked(c, P); };
            ops.batch_reads = 1u << 20;
            ops.host_batch = add_batch;
            ops.after_chunk = [&](size_t i, size_t n_chunks, TokPending &) -> int {
                if (i != 0 || n_chunks == 1) return MC_OK;
                // No capacity hint that still holds: the first chunk says how many distinct k-mers a byte of this file
                // brings, the file's size says how many chunks follow -- the table goes to its final size now, with one
                // chunk's keys to move, instead of being rebuilt every other chunk (10 M reads with 1 % errors in six
                // chunks: 110 ms of counting against ~45).  An over-estimate (the later chunks repeat k-mers of the first)
                // costs memory, bounded by a third of what the device has free.
                std::lock_guard<std::mutex> g(c->mu);
                unsigned long long used = 0;
                uint32_t fatal = 0;
                int r = read_counters(c, &used, &fatal);
                if (r != MC_OK) return r;
                const bool hint_holds = c->cfg.capacity_hint && used < c->cfg.capacity_hint;
                if (!hint_holds && used) {
                    const double scale = (double)f.n / (double)(cuts[0].second - cuts[0].first);
                    const double load = c->mm_k ? 0.36 : 0.6;
                    size_t fr = 0, tot = 0;
                    if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = 0;
                    uint64_t want_slots = (uint64_t)((double)used * scale / load);
                    want_slots = std::min<uint64_t>(want_slots, fr / 3 / sizeof(Slot));
                    const uint64_t want = regions_for(c, want_slots);
                    if (want > c->n_regions && want_slots > c->n_slots()) {
                        if (dbg) fprintf(stderr, "[ingest] %llu distinct k-mers after %.0f MB of %.0f MB: table to %.1f GB\n", used,
                                         (cuts[0].second - cuts[0].first) / 1e6, f.n / 1e6, (double)(want << c->sb) * sizeof(Slot) / 1e9);
                        r = table_grow(c, want);
                        if (r != MC_OK) return r;
                        c->solid_list_fresh = false;
                    }
                }
                return MC_OK;
            };
            uint64_t total = 0;
            rc = tokenize_file_chunks(c, f, cuts, ops, &total);
            if (rc != MC_OK) return rc;
            if (dbg) fprintf(stderr, "[ingest] device tokeniser: %zu chunk(s), %.1f MB in %.3f s\n", cuts.size(), f.n / 1e6, now() - t_begin);
            if (n_reads) *n_reads = total;
            return MC_OK;
        }
        const uint64_t n = mch::load_reads_file(path, 1u << 20, [&](mch::PackedBatch &b) { if (rc == MC_OK) rc = add_batch(b); });
        if (rc != MC_OK) return rc;
        if (n_reads) *n_reads = n;
        return MC_OK;
    } catch (const mch::Error &e) {
        std::lock_guard<std::mutex> g(c->mu);
        return fail(c, MC_EINVAL, "%s", e.what());
    } catch (const std::bad_alloc &) {
        std::lock_guard<std::mutex> g(c->mu);
        return fail(c, MC_ENOMEM, "mc_add_reads_file: out of host memory");
    }
}

