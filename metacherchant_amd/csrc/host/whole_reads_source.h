// WholeReadsSource: DnaQReader's contract -- read(batch, max_reads) appends exactly min(max_reads, what is left) whole reads in file
// order -- with the reads tokenised on the device (include/mcgpu.h mc_tokenize_whole_dev), for --parse gpu.  An uncompressed FASTA /
// FASTQ file is mapped and cut at record starts into chunks of MC_TOKENIZER_CHUNK_BYTES; the bytes of chunk i + 1 go up on a helper
// thread while chunk i is tokenised.  Beside the DnaQBatch (its codes and phreds are two copies from the device, for the writers) the
// source gives a device view of the batch just delivered: segments of packed words, offsets and low-quality positions that go straight
// into the _dev entry points -- a segment is a slice of one chunk's result, its offsets absolute base positions in its words.  A chunk
// the device declines is read by DnaQReader's own record functions over that range of memory (the same reads, the same messages) and
// its segments are packed here and copied up; a compressed file, or an empty one, goes to DnaQReader whole in the same way.
// (Not part of reads_io.cpp, which stays free of HIP for mc_hosttest and the library.)
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../switches.h"
#include "mcgpu.h"
#include "reads_io.h"

namespace mch {

struct WholeSegment {
    const uint64_t *d_words, *d_offsets;  // n_reads + 1 offsets: base positions in d_words (the first need not be 0)
    const int32_t *d_bad_pos;             // mc_classify_reads' bad_pos of the n_reads reads
    uint64_t first, n_reads;              // reads first .. first + n_reads - 1 of the batch just delivered
    const uint8_t *d_phred = nullptr;     // a phred a base at the base positions of d_offsets (NULL: the source was not asked for bytes)
};

class WholeReadsSource {
public:
    // want_bytes: read() also fills the batch's codes and phreds (else only its offsets)
    WholeReadsSource(mc_ctx *ctx, int device, const std::string &path, bool want_bytes = true)
        : ctx_(ctx), device_(device), path_(path), want_bytes_(want_bytes), host_(new DnaQReader(path))
    {
        debug_ = getenv("MC_INGEST_DEBUG") != nullptr;
        fastq_ = host_->fastq();
        offset_ = host_->phred_offset();
        compressed_ = host_->compressed();
        if (!compressed_ && map_file()) {
            cuts_ = plain_chunks(file_, tokenizer_chunk_bytes_of(getenv("MC_TOKENIZER_CHUNK_BYTES")));
            host_.reset();  // (its part is done: the format and the quality offset)
        }
    }
    WholeReadsSource(const WholeReadsSource &) = delete;
    WholeReadsSource &operator=(const WholeReadsSource &) = delete;
    ~WholeReadsSource()
    {
        for (Upload &u : up_) {
            if (u.th.joinable()) u.th.join();
            if (u.d_text) (void)hipFree(u.d_text);
        }
        release(true);
        if (debug_)
            fprintf(stderr, "[ingest] whole reads: %s: %zu chunk(s) on the device, %zu declined, %llu reads\n", path_.c_str(), n_device_, n_declined_,
                    (unsigned long long)delivered_);
    }
    bool compressed() const { return compressed_; }
    bool on_device() const { return !host_; }  // false: the whole file goes through DnaQReader (compressed, or not to be mapped)

    // max_bases: the batch also ends with the read that takes it to max_bases or beyond (it then holds fewer than max_reads reads
    // although the file goes on; a read is never cut)
    size_t read(DnaQBatch &b, size_t max_reads, uint64_t max_bases = ~0ull)
    {
        if (b.offsets.empty()) b.offsets.assign(1, 0);
        release(false);
        size_t got = 0;
        uint64_t bases = 0;
        while (got < max_reads && bases < max_bases) {
            if (!cur_ || cur_->pos == cur_->n_reads) {
                if (!advance()) break;
                continue;
            }
            const std::vector<uint64_t> &off = cur_->on_host ? cur_->host.offsets : cur_->h_off;
            uint64_t take = std::min<uint64_t>(max_reads - got, cur_->n_reads - cur_->pos);
            if (max_bases != ~0ull && off[cur_->pos + take] - off[cur_->pos] > max_bases - bases)  // up to and with the read that crosses the bound
                take = (uint64_t)(std::lower_bound(off.begin() + (long)cur_->pos, off.begin() + (long)(cur_->pos + take), off[cur_->pos] + (max_bases - bases)) -
                                  (off.begin() + (long)cur_->pos));
            take = std::max<uint64_t>(take, 1);
            bases += off[cur_->pos + take] - off[cur_->pos];
            deliver(b, got, take);
            got += take;
        }
        delivered_ += got;
        return got;
    }
    // the device view of the batch the last read() delivered, in order; it holds until the next read()
    const std::vector<WholeSegment> &segments() const { return segs_; }

private:
    // The file mapped as it is.  (Not map_plain_reads: that one also reads the first records with the counting path's parser and gives
    // up on shapes DnaQReader takes -- a blank line, a '+' for an '@'.  Here such a chunk is declined on the device and read by
    // DnaQReader's functions; the format and the quality offset are DnaQReader's already.)  false: empty, or not to be mapped
    bool map_file()
    {
        file_.fd = open(path_.c_str(), O_RDONLY);
        struct stat st;
        if (file_.fd < 0 || fstat(file_.fd, &st) != 0 || st.st_size <= 0) return false;
        void *mp = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, file_.fd, 0);
        if (mp == MAP_FAILED) return false;
        file_.p = static_cast<const char *>(mp);
        file_.n = (size_t)st.st_size;
        file_.fastq = fastq_;
        file_.offset = offset_;
        return true;
    }
    struct Chunk {  // one chunk's reads: on the device (res), or parsed here (host) when the device declined it
        mc_whole_reads res{};
        std::vector<uint64_t> h_off;
        DnaQBatch host;
        bool on_host = false;
        uint64_t n_reads = 0, pos = 0;
    };
    struct Upload {
        uint8_t *d_text = nullptr;
        uint64_t cap = 0;
        std::thread th;
        hipError_t err = hipSuccess;
    };
    static void check(hipError_t e, const char *what)
    {
        if (e != hipSuccess) throw Error(std::string(what) + ": " + hipGetErrorString(e));
    }
    void lib_check(int rc)
    {
        if (rc != MC_OK) throw Error(std::string("GPU error: ") + mc_last_error(ctx_));
    }
    void start_upload(size_t i)
    {
        Upload &u = up_[i & 1];
        const uint64_t n = (uint64_t)(cuts_[i].second - cuts_[i].first), need = mc_whole_text_bytes(n);
        check(hipSetDevice(device_), "hipSetDevice");
        if (u.cap < need) {
            if (u.d_text) (void)hipFree(u.d_text);
            u.d_text = nullptr;
            u.cap = 0;
            check(hipMalloc(reinterpret_cast<void **>(&u.d_text), need), "hipMalloc");
            u.cap = need;
        }
        const char *src = cuts_[i].first;
        const int device = device_;
        Upload *up = &u;
        u.th = std::thread([up, src, n, device] {
            up->err = hipSetDevice(device);
            if (up->err == hipSuccess) up->err = hipMemcpy(up->d_text, src, n, hipMemcpyHostToDevice);
        });
    }
    // the next chunk becomes the current one; false: the file is done
    bool advance()
    {
        if (host_) {  // the whole file through DnaQReader, a batch at a time
            std::unique_ptr<Chunk> c(new Chunk);
            c->on_host = true;
            c->host.clear();
            c->n_reads = host_->read(c->host, 1u << 16);
            if (c->n_reads == 0) return false;
            keep_.push_back(std::move(c));
            cur_ = keep_.back().get();
            return true;
        }
        if (next_ == cuts_.size()) return false;
        const size_t i = next_++;
        if (i == 0) start_upload(0);
        Upload &u = up_[i & 1];
        u.th.join();
        check(u.err, "hipMemcpy");
        if (i + 1 < cuts_.size()) start_upload(i + 1);
        std::unique_ptr<Chunk> c(new Chunk);
        const uint64_t n = (uint64_t)(cuts_[i].second - cuts_[i].first);
        lib_check(mc_tokenize_whole_dev(ctx_, u.d_text, n, cuts_[i].second[-1], fastq_ ? MC_WHOLE_FASTQ : MC_WHOLE_FASTA, offset_,
                                        want_bytes_ ? MC_WHOLE_CODES | MC_WHOLE_PHRED : 0, &c->res));
        if (c->res.declined) {
            n_declined_++;
            c->on_host = true;
            c->host.clear();
            DnaQReader part(cuts_[i].first, cuts_[i].second, fastq_, offset_);
            while (part.read(c->host, 1u << 16)) {}
            c->n_reads = c->host.n_reads();
        } else {
            n_device_++;
            c->n_reads = c->res.n_reads;
            c->h_off.resize(c->n_reads + 1);
            check(hipMemcpy(c->h_off.data(), c->res.d_offsets, (c->n_reads + 1) * 8, hipMemcpyDeviceToHost), "hipMemcpy");
        }
        keep_.push_back(std::move(c));
        cur_ = keep_.back().get();
        return true;
    }
    // reads pos .. pos + take - 1 of the current chunk: appended to b, and a segment of the view
    void deliver(DnaQBatch &b, uint64_t first, uint64_t take)
    {
        Chunk &c = *cur_;
        const uint64_t base = b.offsets.back();
        if (!c.on_host) {
            const uint64_t o0 = c.h_off[c.pos], o1 = c.h_off[c.pos + take];
            for (uint64_t r = 1; r <= take; r++) b.offsets.push_back(base + c.h_off[c.pos + r] - o0);
            if (want_bytes_ && o1 > o0) {
                const size_t at = b.codes.size();
                b.codes.resize(at + (o1 - o0));
                b.phred.resize(at + (o1 - o0));
                check(hipMemcpy(b.codes.data() + at, c.res.d_codes + o0, o1 - o0, hipMemcpyDeviceToHost), "hipMemcpy");
                check(hipMemcpy(b.phred.data() + at, c.res.d_phred + o0, o1 - o0, hipMemcpyDeviceToHost), "hipMemcpy");
            }
            segs_.push_back(WholeSegment{c.res.d_words, c.res.d_offsets + c.pos, c.res.d_bad_pos + c.pos, first, take, c.res.d_phred});
        } else {
            const DnaQBatch &h = c.host;
            const uint64_t o0 = h.offsets[c.pos], o1 = h.offsets[c.pos + take];
            for (uint64_t r = 1; r <= take; r++) b.offsets.push_back(base + h.offsets[c.pos + r] - o0);
            if (want_bytes_) {
                b.codes.insert(b.codes.end(), h.codes.begin() + (long)o0, h.codes.begin() + (long)o1);
                b.phred.insert(b.phred.end(), h.phred.begin() + (long)o0, h.phred.begin() + (long)o1);
            }
            // (the fall-back only: packed as classify_batch packs, then copied up)
            std::vector<uint64_t> words, off;
            pack_whole_reads(h, c.pos, take, words, &off);
            const std::vector<int32_t> bad = low_quality_positions(h, c.pos, take);
            check(hipSetDevice(device_), "hipSetDevice");
            char *d = nullptr;
            const size_t wb = words.size() * 8, ob = off.size() * 8, bb = std::max<size_t>(bad.size() * 4, 4), qb = want_bytes_ ? (size_t)(o1 - o0) : 0;
            check(hipMalloc(reinterpret_cast<void **>(&d), wb + ob + bb + std::max<size_t>(qb, 1)), "hipMalloc");
            owned_.push_back(d);
            check(hipMemcpy(d, words.data(), wb, hipMemcpyHostToDevice), "hipMemcpy");
            check(hipMemcpy(d + wb, off.data(), ob, hipMemcpyHostToDevice), "hipMemcpy");
            if (take) check(hipMemcpy(d + wb + ob, bad.data(), bad.size() * 4, hipMemcpyHostToDevice), "hipMemcpy");
            if (qb) check(hipMemcpy(d + wb + ob + bb, h.phred.data() + o0, qb, hipMemcpyHostToDevice), "hipMemcpy");  // (off starts at 0)
            segs_.push_back(WholeSegment{reinterpret_cast<uint64_t *>(d), reinterpret_cast<uint64_t *>(d + wb), reinterpret_cast<int32_t *>(d + wb + ob), first, take,
                                         want_bytes_ ? reinterpret_cast<uint8_t *>(d + wb + ob + bb) : nullptr});
        }
        c.pos += take;
    }
    // what the last batch's view held goes back; the chunk still being read stays
    void release(bool all)
    {
        segs_.clear();
        for (char *p : owned_) (void)hipFree(p);
        owned_.clear();
        std::vector<std::unique_ptr<Chunk>> stay;
        for (auto &c : keep_) {
            if (!all && c.get() == cur_ && c->pos < c->n_reads) { stay.push_back(std::move(c)); continue; }
            mc_whole_reads_free(ctx_, &c->res);
        }
        if (stay.empty()) cur_ = nullptr;
        keep_.swap(stay);
    }

    mc_ctx *ctx_;
    int device_;
    std::string path_;
    bool want_bytes_, debug_ = false, fastq_ = false, compressed_ = false;
    int offset_ = 0;
    std::unique_ptr<DnaQReader> host_;
    PlainReadsFile file_;
    std::vector<std::pair<const char *, const char *>> cuts_;
    size_t next_ = 0, n_device_ = 0, n_declined_ = 0;
    uint64_t delivered_ = 0;
    Upload up_[2];
    std::vector<std::unique_ptr<Chunk>> keep_;
    Chunk *cur_ = nullptr;
    std::vector<WholeSegment> segs_;
    std::vector<char *> owned_;
};

}  // namespace mch
