// See reads_io.h.  Every function restates the reference lines cited there.
#include "reads_io.h"

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>

namespace mch {

int code_of(char c)
{
    switch (c) {
    case 'A': case 'a': return 0;
    case 'G': case 'g': return 1;
    case 'C': case 'c': return 2;
    case 'T': case 't': return 3;
    default: return -1;
    }
}

void PackedBatch::clear()
{
    words.clear();
    offsets.assign(1, 0);
}

namespace {
struct CodeLut {  // A0 G1 C2 T3 (either case), 0xFF otherwise
    uint8_t v[256];
    CodeLut()
    {
        memset(v, 0xFF, sizeof v);
        v[(unsigned char)'A'] = v[(unsigned char)'a'] = 0;
        v[(unsigned char)'G'] = v[(unsigned char)'g'] = 1;
        v[(unsigned char)'C'] = v[(unsigned char)'c'] = 2;
        v[(unsigned char)'T'] = v[(unsigned char)'t'] = 3;
    }
};
const CodeLut CODE_LUT;
}  // namespace

void PackedBatch::add_read(const char *s, size_t n)
{
    if (offsets.empty()) offsets.assign(1, 0);
    uint64_t pos = offsets.back();
    words.resize((pos + n + 31) / 32, 0);
    // a word at a time: the open word is completed, then whole words of 32 bases, then the tail
    size_t i = 0;
    uint32_t bad = 0;
    uint64_t *w = words.data();
    while (i < n) {
        const uint32_t in_word = (uint32_t)(pos & 31), take = (uint32_t)std::min<size_t>(32 - in_word, n - i);
        uint64_t acc = 0;
        for (uint32_t j = 0; j < take; j++) {
            const uint8_t c = CODE_LUT.v[(unsigned char)s[i + j]];
            bad |= c;
            acc = (acc << 2) | (c & 3u);
        }
        w[pos >> 5] |= acc << (2 * (32 - in_word - take));
        pos += take;
        i += take;
    }
    if (bad & 0x80) {
        for (size_t q = 0; q < n; q++)
            if (code_of(s[q]) < 0)
                throw Error(std::string("read contains the character '") + s[q] +
                            "': IUPAC codes other than N are replaced at random by the reference "
                            "(itmo!/dna/DnaTools.java:66-117), which has no defined result; rejecting the input");
    }
    offsets.push_back(pos);
}

void PackedBatch::finish()
{
    if (offsets.empty()) offsets.assign(1, 0);
    words.resize((offsets.back() + 31) / 32 + 1, 0);
}

static bool ends_with(const std::string &s, const char *suf)
{
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

static std::string lower(std::string s)
{
    for (char &c : s) c = (char)tolower((unsigned char)c);
    return s;
}

// Bytes of a file, plain, gzip or bzip2 (itmo!/io/readers/FastaGZReader.java, FastqGZReader.java: the same readers
// over a java.util.zip.GZIPInputStream; FastaBZ2Reader.java:27, FastqBZ2Reader.java: over Hadoop's BZip2Codec
// stream; concatenated members / streams read on, as there).  bzip2 goes through the system's libbz2.so.1.0, loaded
// when the first .bz2 file is opened: its 1.0 ABI (bz_stream + BZ2_bzDecompress*) is declared here because the
// image ships the library without its header.
namespace {
enum Compression { COMP_NONE, COMP_GZ, COMP_BZ2 };

struct Bz2Api {
    struct Stream {
        char *next_in; unsigned avail_in, total_in_lo32, total_in_hi32;
        char *next_out; unsigned avail_out, total_out_lo32, total_out_hi32;
        void *state;
        void *(*bzalloc)(void *, int, int);
        void (*bzfree)(void *, void *);
        void *opaque;
    };
    int (*init)(Stream *, int, int) = nullptr;
    int (*run)(Stream *) = nullptr;
    int (*end)(Stream *) = nullptr;
    static const Bz2Api &get()
    {
        static const Bz2Api api = [] {
            Bz2Api a;
            void *h = dlopen("libbz2.so.1.0", RTLD_NOW | RTLD_GLOBAL);
            if (!h) h = dlopen("libbz2.so.1", RTLD_NOW | RTLD_GLOBAL);
            if (h) {
                a.init = (int (*)(Stream *, int, int))dlsym(h, "BZ2_bzDecompressInit");
                a.run = (int (*)(Stream *))dlsym(h, "BZ2_bzDecompress");
                a.end = (int (*)(Stream *))dlsym(h, "BZ2_bzDecompressEnd");
            }
            return a;
        }();
        if (!api.init || !api.run || !api.end) throw Error("bzip2 input needs libbz2.so.1.0, which could not be loaded");
        return api;
    }
};

class ByteSource {
public:
    ByteSource(const std::string &path, Compression comp) : comp_(comp)
    {
        if (comp_ == COMP_GZ) {
            g_ = gzopen(path.c_str(), "rb");
            if (!g_) throw Error("Failed to read from file " + path);
            gzbuffer(g_, 1u << 20);
        } else {
            f_ = fopen(path.c_str(), "rb");
            if (!f_) throw Error("Failed to read from file " + path);
            if (comp_ == COMP_BZ2) {
                bz_ = &Bz2Api::get();
                in_.resize(1u << 20);
                memset(&bs_, 0, sizeof bs_);
            }
        }
    }
    ~ByteSource()
    {
        if (g_) gzclose(g_);
        if (bz_open_) bz_->end(&bs_);
        if (f_) fclose(f_);
    }
    ByteSource(const ByteSource &) = delete;
    ByteSource &operator=(const ByteSource &) = delete;
    // up to n bytes; 0 at the end of the data
    size_t read(char *dst, size_t n)
    {
        if (comp_ == COMP_NONE) return fread(dst, 1, n, f_);
        if (comp_ == COMP_GZ) {
            const int got = gzread(g_, dst, (unsigned)std::min<size_t>(n, 1u << 30));
            if (got < 0) throw Error("Failed to decompress the input (corrupt gzip stream)");
            return (size_t)got;
        }
        size_t done = 0;
        while (done < n && !bz_eof_) {
            if (bs_.avail_in == 0) {
                bs_.next_in = in_.data();
                bs_.avail_in = (unsigned)fread(in_.data(), 1, in_.size(), f_);
                if (bs_.avail_in == 0) {
                    if (bz_open_) throw Error("Failed to decompress the input (truncated bzip2 stream)");
                    bz_eof_ = true;  // the file ends between two streams
                    break;
                }
            }
            if (!bz_open_) {
                if (bz_->init(&bs_, 0, 0) != 0) throw Error("Failed to decompress the input (bzip2 initialisation)");
                bz_open_ = true;
            }
            bs_.next_out = dst + done;
            bs_.avail_out = (unsigned)std::min<size_t>(n - done, 1u << 30);
            const unsigned before = bs_.avail_out;
            const int rc = bz_->run(&bs_);
            done += before - bs_.avail_out;
            if (rc == 4) {  // BZ_STREAM_END: another stream may follow
                bz_->end(&bs_);
                bz_open_ = false;
            } else if (rc != 0) {
                throw Error("Failed to decompress the input (corrupt bzip2 stream)");
            }
        }
        return done;
    }

private:
    Compression comp_;
    gzFile g_ = nullptr;
    FILE *f_ = nullptr;
    const Bz2Api *bz_ = nullptr;
    Bz2Api::Stream bs_;
    std::vector<char> in_;
    bool bz_open_ = false, bz_eof_ = false;
};

// Lines of such a file ('\n' ends a line, one trailing '\r' comes off)
class LineSource {
public:
    LineSource(const std::string &path, Compression comp) : src_(path, comp), buf_(1u << 20) {}
    bool getline(std::string &l)
    {
        l.clear();
        bool any = false;
        for (;;) {
            if (pos_ == len_) {
                len_ = src_.read(buf_.data(), buf_.size());
                pos_ = 0;
                if (len_ == 0) {
                    if (!any) return false;
                    break;
                }
            }
            any = true;
            const char *b = buf_.data() + pos_;
            const char *nl = (const char *)memchr(b, '\n', len_ - pos_);
            if (nl) {
                l.append(b, (size_t)(nl - b));
                pos_ += (size_t)(nl - b) + 1;
                break;
            }
            l.append(b, len_ - pos_);
            pos_ = len_;
        }
        if (!l.empty() && l.back() == '\r') l.pop_back();
        return true;
    }

private:
    ByteSource src_;
    std::vector<char> buf_;
    size_t pos_ = 0, len_ = 0;
};
}  // namespace

namespace {

// lines of a memory range (a chunk of a memory-mapped file)
class MemLines {
public:
    MemLines(const char *b, const char *e) : p_(b), end_(e) {}
    bool getline(std::string &l)
    {
        if (p_ >= end_) return false;
        const char *nl = static_cast<const char *>(memchr(p_, '\n', (size_t)(end_ - p_)));
        const char *stop = nl ? nl : end_;
        l.assign(p_, (size_t)(stop - p_));
        p_ = nl ? nl + 1 : end_;
        if (!l.empty() && l.back() == '\r') l.pop_back();
        return true;
    }

private:
    const char *p_, *end_;
};

// itmo!/io/readers/FastaReader.java:54-104: multi-line records concatenated, records with N / n dropped whole
template <class Src, class Emit>
void parse_fasta(Src &src, Emit &&emit)
{
    std::string line, sb;
    auto flush = [&] {
        if (!sb.empty() && sb.find('N') == std::string::npos && sb.find('n') == std::string::npos) emit(sb.data(), sb.size());
        sb.clear();
    };
    while (src.getline(line)) {
        if (!line.empty() && (line[0] == '>' || line[0] == ';')) {
            if (!sb.empty()) flush();
        } else if (sb.empty()) {
            sb.swap(line);  // (the usual single-line record is not copied again)
        } else {
            sb += line;
        }
    }
    flush();
}

// itmo!/io/readers/FastqReader.java:53-112 + FastaReaderFromXQSourceTrunc.java:61-95 + itmo!/io/ReadersUtils.java:57-77.
// Records: marker line ("@id" / "+id") + content line, twice; empty lines before a marker are skipped.
// offset < 0: the quality offset is sniffed on the first 1000 records (Illumina+64 unless a char < 64 shows up).
// strict: the first marker must be '@' and the second '+' (what the parallel reader relies on); returns false otherwise.
template <class Src, class Emit>
bool parse_fastq(Src &src, Emit &&emit, int offset, bool strict, int *sniffed = nullptr, size_t sniff_only = 0)
{
    char marker = 0;
    auto next_data = [&](std::string &out) -> bool {
        std::string l;
        for (;;) {
            if (!src.getline(l)) return false;
            if (!l.empty()) break;
        }
        if (l[0] != '@' && l[0] != '+') throw Error("Unknown structure of fastq file! Waiting \"@ID\" or \"+ID\" string");
        marker = l[0];
        if (!src.getline(out)) throw Error("Unexpected end of file. File is corrupted/Format mismatch.");
        return true;
    };
    std::vector<std::pair<std::string, std::string>> head;  // the records the offset is sniffed on
    auto process = [&](const std::string &d, const std::string &q) {
        // truncateByQuality(1): a base with phred < 1 (or N n .) ends the piece and is dropped; pieces go out straight
        // from the line
        size_t start = 0;
        const size_t n = d.size();
        for (size_t i = 0; i < n; i++) {
            const unsigned char c = (unsigned char)d[i];
            bool bad = c == 'N' || c == 'n' || c == '.';
            if (!bad) {
                const int qc = (unsigned char)q[i];
                if (qc < offset || qc > 126) throw Error("Invalid quality code char");
                bad = ((qc - offset) & 63) < 1;  // the phred lives in 6 bits of a byte (DnaQBuilder.java:32-35): 64 wraps to 0
            }
            if (bad) {
                if (i > start) emit(d.data() + start, i - start);
                start = i + 1;
            }
        }
        if (n > start) emit(d.data() + start, n - start);
    };
    auto sniff = [&] {
        offset = 64;
        for (const auto &r : head)
            for (size_t i = 0; i < r.first.size(); i++) {
                if (r.first[i] == 'N' || r.first[i] == 'n' || r.first[i] == '.') continue;
                const int qc = (unsigned char)r.second[i];
                if (qc < 64 || qc > 126) { offset = 33; return; }
            }
    };
    std::string d, q;
    while (next_data(d)) {
        if (strict && marker != '@') return false;
        if (!next_data(q)) throw Error("Unexpected end of file. File is corrupted/Format mismatch.");
        if (strict && marker != '+') return false;
        if (d.size() != q.size()) throw Error("Bad DnaQ record: length of chars and quality is not the same.");
        if (offset < 0) {
            head.emplace_back(d, q);
            if (head.size() == 1000) {
                sniff();
                if (sniff_only) { *sniffed = offset; return true; }
                for (const auto &r : head) process(r.first, r.second);
                head.clear();
            }
        } else {
            process(d, q);
        }
    }
    if (offset < 0) {
        sniff();
        if (sniff_only) { *sniffed = offset; return true; }
        for (const auto &r : head) process(r.first, r.second);
    }
    return true;
}

// itmo!/io/readers/BinqReader.java:52-86: records of a 4-byte big-endian length and that many bytes (phred << 2 | nuc);
// 0xFF bytes in front of a record are padding.  Pieces as in parse_fastq (FastaReaderFromXQSourceTrunc.java:61-95).
template <class Src, class Emit>
void parse_binq(Src &src, Emit &&emit, const std::string &file_name)
{
    std::vector<char> buf(1u << 20);
    size_t pos = 0, len = 0;
    auto next_byte = [&]() -> int {
        if (pos == len) {
            len = src.read(buf.data(), buf.size());
            pos = 0;
            if (len == 0) return -1;
        }
        return (unsigned char)buf[pos++];
    };
    std::string rec, piece;
    for (;;) {
        int b0 = next_byte();
        while (b0 == 255) b0 = next_byte();
        if (b0 < 0) return;
        const int b1 = next_byte(), b2 = next_byte(), b3 = next_byte();
        if (b1 < 0 || b2 < 0 || b3 < 0) throw Error("Unexpected end of file " + file_name);
        const size_t n = ((size_t)b0 << 24) + ((size_t)b1 << 16) + ((size_t)b2 << 8) + (size_t)b3;
        rec.resize(n);
        for (size_t got = 0; got < n;) {
            if (pos == len) {
                len = src.read(buf.data(), buf.size());
                pos = 0;
                if (len == 0) throw Error("Unexpected end of file " + file_name);
            }
            const size_t take = std::min(n - got, len - pos);
            memcpy(&rec[got], buf.data() + pos, take);
            got += take;
            pos += take;
        }
        piece.clear();
        for (size_t i = 0; i < n; i++) {
            const unsigned v = (unsigned char)rec[i];
            if ((v >> 2) < 1) {  // truncateByQuality(1)
                if (!piece.empty()) emit(piece.data(), piece.size());
                piece.clear();
            } else {
                piece.push_back("AGCT"[v & 3]);
            }
        }
        if (!piece.empty()) emit(piece.data(), piece.size());
    }
}

struct Mapped {  // a read-only memory map of a whole file
    const char *p = nullptr;
    size_t n = 0;
    int fd = -1;
    ~Mapped()
    {
        if (p && n) munmap(const_cast<char *>(p), n);
        if (fd >= 0) close(fd);
    }
};

size_t env_size(const char *name, size_t dflt)
{
    const char *e = getenv(name);
    return e && *e ? (size_t)strtoull(e, nullptr, 10) : dflt;
}

// Parallel ingest of an uncompressed file: cut at record starts, parse the chunks on all cores, hand the batches over
// in file order.  Returns false (nothing delivered) when the file is small, cannot be mapped, or does not have the
// plain structure the cutting relies on -- the caller then reads it serially, which defines the behaviour.
bool load_reads_parallel(const std::string &path, bool fastq, size_t max_reads, const std::function<void(PackedBatch &)> &sink,
                         uint64_t *delivered)
{
    const bool dbg = getenv("MC_INGEST_DEBUG") != nullptr;
    auto tnow = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = tnow();
    size_t n_threads = env_size("MC_INGEST_THREADS", std::min<size_t>(std::max(1u, std::thread::hardware_concurrency()), 128));
    const size_t min_chunk = std::max<size_t>(env_size("MC_INGEST_CHUNK_BYTES", 4u << 20), 64);
    if (n_threads < 2) return false;
    Mapped m;
    m.fd = open(path.c_str(), O_RDONLY);
    if (m.fd < 0) return false;
    struct stat st;
    if (fstat(m.fd, &st) != 0 || st.st_size < (off_t)(2 * min_chunk)) return false;
    m.n = (size_t)st.st_size;
    void *mp = mmap(nullptr, m.n, PROT_READ, MAP_PRIVATE, m.fd, 0);
    if (mp == MAP_FAILED) { m.n = 0; return false; }
    m.p = static_cast<const char *>(mp);
    n_threads = std::min(n_threads, m.n / min_chunk);
    const char *begin = m.p, *end = m.p + m.n;
    auto line_start_after = [&](const char *q) -> const char * {  // first line start at or after q
        if (q <= begin) return begin;
        const char *nl = static_cast<const char *>(memchr(q - 1, '\n', (size_t)(end - (q - 1))));
        return nl ? nl + 1 : end;
    };
    auto line_end = [&](const char *q) { const char *nl = static_cast<const char *>(memchr(q, '\n', (size_t)(end - q))); return nl ? nl : end; };
    auto next_line = [&](const char *q) { const char *e = line_end(q); return e < end ? e + 1 : end; };
    auto len_of = [&](const char *q) { const char *e = line_end(q); size_t l = (size_t)(e - q); if (l && q[l - 1] == '\r') l--; return l; };
    // record start at or after q: FASTA a header line; FASTQ '@' line whose third line starts with '+' and whose second
    // and fourth lines have the same length (a quality line that starts with '@' fails the '+' test)
    auto record_start = [&](const char *q) -> const char * {
        const char *l = line_start_after(q);
        for (int guard = 0; l < end && guard < 100000; guard++, l = next_line(l)) {
            if (!fastq) {
                if (*l == '>' || *l == ';') return l;
                continue;
            }
            if (*l != '@') continue;
            const char *l2 = next_line(l), *l3 = l2 < end ? next_line(l2) : end;
            if (l3 >= end || *l3 != '+') continue;
            const char *l4 = next_line(l3);
            if (l4 < end && len_of(l2) == len_of(l4)) return l;
        }
        return end;
    };
    std::vector<const char *> cut(n_threads + 1);
    cut[0] = begin;
    cut[n_threads] = end;
    for (size_t t = 1; t < n_threads; t++) cut[t] = std::max(cut[t - 1], record_start(begin + m.n / n_threads * t));
    int offset = -1;
    if (fastq) {  // the quality offset comes from the first 1000 records of the file
        MemLines src(begin, end);
        if (!parse_fastq(src, [](const char *, size_t) {}, -1, true, &offset, 1) || offset < 0) return false;
    }
    const double t_cut = tnow();
    struct Part { std::vector<PackedBatch> batches; uint64_t reads = 0; bool ok = true; };
    std::vector<Part> parts(n_threads);
    std::vector<std::thread> threads;
    for (size_t t = 0; t < n_threads; t++)
        threads.emplace_back([&, t] {
            Part &P = parts[t];
            try {
                PackedBatch batch;
                batch.clear();
                // room for the whole chunk up front: growing vectors map and unmap memory, which serialises the threads
                const size_t chunk_bytes = (size_t)(cut[t + 1] - cut[t]);
                batch.words.reserve(chunk_bytes / 32 + 16);
                batch.offsets.reserve(std::min<size_t>(max_reads, chunk_bytes / 64) + 16);
                auto emit = [&](const char *s, size_t n) {
                    batch.add_read(s, n);
                    P.reads++;
                    if (batch.n_reads() >= max_reads) {
                        batch.finish();
                        P.batches.push_back(std::move(batch));
                        batch = PackedBatch();
                        batch.clear();
                    }
                };
                MemLines src(cut[t], cut[t + 1]);
                if (fastq) P.ok = parse_fastq(src, emit, offset, true);
                else parse_fasta(src, emit);
                if (batch.n_reads() > 0) {
                    batch.finish();
                    P.batches.push_back(std::move(batch));
                }
            } catch (...) {
                P.ok = false;  // the serial reader will meet the same problem and report it
            }
        });
    for (auto &th : threads) th.join();
    const double t_parse = tnow();
    for (const Part &P : parts)
        if (!P.ok) return false;
    *delivered = 0;
    for (const Part &P : parts) *delivered += P.reads;
    // Every thread leaves a small batch; handing them over one by one would cost a device launch each.  They are
    // joined, in file order, into batches of up to max_reads reads: the pieces' words are shifted into place in
    // parallel (a piece starts wherever the previous one ended, not at a word boundary).
    std::vector<PackedBatch *> pieces;
    for (Part &P : parts)
        for (PackedBatch &b : P.batches)
            if (b.n_reads()) pieces.push_back(&b);
    size_t first = 0;
    while (first < pieces.size()) {
        size_t last = first;
        uint64_t reads = 0, bases = 0;
        std::vector<uint64_t> base_at;  // where each piece starts, in bases
        while (last < pieces.size() && (last == first || reads + pieces[last]->n_reads() <= max_reads)) {
            base_at.push_back(bases);
            reads += pieces[last]->n_reads();
            bases += pieces[last]->offsets.back();
            last++;
        }
        if (last - first == 1) {
            sink(*pieces[first]);
            first = last;
            continue;
        }
        const double t_m0 = tnow();
        PackedBatch out;
        out.words.assign((bases + 31) / 32 + 1, 0);
        out.offsets.resize(reads + 1);
        out.offsets[0] = 0;
        std::vector<uint64_t> read_at(last - first);
        {
            uint64_t r = 0;
            for (size_t i = first; i < last; i++) { read_at[i - first] = r; r += pieces[i]->n_reads(); }
        }
        std::vector<std::thread> mergers;
        const size_t n_merge = std::min<size_t>(last - first, n_threads);
        for (size_t w = 0; w < n_merge; w++)
            mergers.emplace_back([&, w] {
                for (size_t i = first + w; i < last; i += n_merge) {
                    const PackedBatch &b = *pieces[i];
                    const uint64_t at = base_at[i - first], n_src = (b.offsets.back() + 31) / 32;
                    const uint64_t dw = at / 32, sh = 2 * (at % 32);
                    // only the first and the last destination words of a piece can be shared with a neighbour
                    auto put = [&](uint64_t idx, uint64_t v) {
                        if (!v) return;
                        if (idx == dw || idx + 1 >= dw + n_src) __atomic_fetch_or(&out.words[idx], v, __ATOMIC_RELAXED);
                        else out.words[idx] |= v;
                    };
                    for (uint64_t j = 0; j < n_src; j++) {
                        const uint64_t v = b.words[j];
                        put(dw + j, sh ? (v >> sh) : v);
                        if (sh) put(dw + j + 1, v << (64 - sh));
                    }
                    const uint64_t r0 = read_at[i - first];
                    for (uint64_t r = 0; r < b.n_reads(); r++) out.offsets[r0 + r + 1] = at + b.offsets[r + 1];
                }
            });
        for (auto &th : mergers) th.join();
        const double t_m = tnow();
        sink(out);
        if (dbg) fprintf(stderr, "[ingest] merged %zu pieces (%llu reads) in %.3f s, sink %.3f s\n", last - first, (unsigned long long)reads, t_m - t_m0, tnow() - t_m);
        first = last;
    }
    if (dbg) fprintf(stderr, "[ingest] %zu threads: map+cut+sniff %.3f s, parse %.3f s, merge+sink %.3f s\n", n_threads, t_cut - t_begin, t_parse - t_cut, tnow() - t_parse);
    return true;
}

}  // namespace

namespace {
// itmo!/io/ReadersUtils.java:27-53 detectFileFormat on a lower-cased file name without its compression suffix
void reads_format_of(const std::string &name, bool *binq, bool *fastq, bool *fasta)
{
    *binq = ends_with(name, ".binq");
    *fastq = ends_with(name, ".fastq") || ends_with(name, ".fq");
    *fasta = ends_with(name, ".fasta") || ends_with(name, ".fa") || ends_with(name, ".fn") || ends_with(name, ".fna");
}
}  // namespace

PlainReadsFile::~PlainReadsFile()
{
    if (p && n) munmap(const_cast<char *>(p), n);
    if (fd >= 0) close(fd);
}

bool map_plain_reads(const std::string &path, PlainReadsFile *out)
{
    const size_t slash = path.find_last_of('/');
    const std::string name = lower(slash == std::string::npos ? path : path.substr(slash + 1));
    bool binq, fastq, fasta;
    reads_format_of(name, &binq, &fastq, &fasta);
    if (binq || (!fastq && !fasta)) return false;  // (a .gz / .bz2 name matches neither)
    out->fd = open(path.c_str(), O_RDONLY);
    if (out->fd < 0) return false;
    struct stat st;
    if (fstat(out->fd, &st) != 0 || st.st_size <= 0) return false;
    void *mp = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, out->fd, 0);
    if (mp == MAP_FAILED) return false;
    out->p = static_cast<const char *>(mp);
    out->n = (size_t)st.st_size;
    out->fastq = fastq;
    if (fastq) {
        MemLines src(out->p, out->p + out->n);
        int offset = -1;
        try {
            if (!parse_fastq(src, [](const char *, size_t) {}, -1, true, &offset, 1) || offset < 0) return false;
        } catch (const Error &) {
            return false;  // the serial reader meets the same problem and reports it
        }
        out->offset = offset;
    }
    return true;
}

const char *plain_record_start(const PlainReadsFile &f, const char *q)
{
    const char *begin = f.p, *end = f.p + f.n;
    auto line_end = [&](const char *s) { const char *nl = static_cast<const char *>(memchr(s, '\n', (size_t)(end - s))); return nl ? nl : end; };
    auto next_line = [&](const char *s) { const char *e = line_end(s); return e < end ? e + 1 : end; };
    auto len_of = [&](const char *s) { const char *e = line_end(s); size_t l = (size_t)(e - s); if (l && s[l - 1] == '\r') l--; return l; };
    const char *l = begin;
    if (q > begin) {
        const char *nl = static_cast<const char *>(memchr(q - 1, '\n', (size_t)(end - (q - 1))));
        l = nl ? nl + 1 : end;
    }
    for (; l < end; l = next_line(l)) {
        if (!f.fastq) {
            if (*l == '>' || *l == ';') return l;
            continue;
        }
        // an '@' line whose third line starts with '+' and whose second and fourth lines are equally long (a quality
        // line that starts with '@' fails the '+' test: the line two below it holds bases)
        if (*l != '@') continue;
        const char *l2 = next_line(l), *l3 = l2 < end ? next_line(l2) : end;
        if (l3 >= end || *l3 != '+') continue;
        const char *l4 = next_line(l3);
        if (l4 < end && len_of(l2) == len_of(l4)) return l;
    }
    return end;
}

std::vector<std::pair<const char *, const char *>> plain_chunks(const PlainReadsFile &f, uint64_t chunk_bytes)
{
    std::vector<std::pair<const char *, const char *>> cuts;
    for (const char *b = f.p, *end = f.p + f.n; b < end;) {
        const char *e = (uint64_t)(end - b) <= chunk_bytes + chunk_bytes / 4 ? end : plain_record_start(f, b + chunk_bytes);
        cuts.emplace_back(b, e);
        b = e;
    }
    return cuts;
}

uint64_t parse_plain_range(const PlainReadsFile &f, const char *b, const char *e, size_t max_reads, const std::function<void(PackedBatch &)> &sink)
{
    uint64_t delivered = 0;
    PackedBatch batch;
    batch.clear();
    auto emit = [&](const char *s, size_t n) {
        batch.add_read(s, n);
        delivered++;
        if (batch.n_reads() >= max_reads) {
            batch.finish();
            sink(batch);
            batch.clear();
        }
    };
    MemLines src(b, e);
    if (f.fastq) parse_fastq(src, emit, f.offset, false);
    else parse_fasta(src, emit);
    if (batch.n_reads() > 0) {
        batch.finish();
        sink(batch);
    }
    return delivered;
}

uint64_t load_reads_file(const std::string &path, size_t max_reads, const std::function<void(PackedBatch &)> &sink)
{
    // itmo!/io/ReadersUtils.java:27-53 detectFileFormat: a .gz and then a .bz2 suffix come off, then the format
    const size_t slash = path.find_last_of('/');
    const std::string full_name = lower(slash == std::string::npos ? path : path.substr(slash + 1));
    std::string name = full_name, suffix;
    Compression comp = COMP_NONE;
    if (ends_with(name, ".gz")) { comp = COMP_GZ; suffix = ".gz"; name.resize(name.size() - 3); }
    if (ends_with(name, ".bz2")) { comp = COMP_BZ2; suffix = ".bz2"; name.resize(name.size() - 4); }
    const bool binq = ends_with(name, ".binq");
    const bool fastq = ends_with(name, ".fastq") || ends_with(name, ".fq");
    const bool fasta = ends_with(name, ".fasta") || ends_with(name, ".fa") || ends_with(name, ".fn") || ends_with(name, ".fna");
    if (!binq && !fastq && !fasta) throw Error("Can't detect file format for file '" + name + "'");
    if (binq && comp != COMP_NONE) throw Error("Illegal format binq" + suffix);  // ReadersUtils.java:210-214

    uint64_t delivered = 0;
    if (comp == COMP_NONE && !binq && load_reads_parallel(path, fastq, max_reads, sink, &delivered)) return delivered;

    // the reference's readers are serial (one synchronized source per file, src/io/ReadsDispatcher.java:34-53)
    PackedBatch batch;
    batch.clear();
    auto emit = [&](const char *s, size_t n) {
        batch.add_read(s, n);
        delivered++;
        if (batch.n_reads() >= max_reads) {
            batch.finish();
            sink(batch);
            batch.clear();
        }
    };
    if (binq) {
        ByteSource src(path, COMP_NONE);
        parse_binq(src, emit, full_name);
    } else {
        LineSource src(path, comp);
        if (fasta) parse_fasta(src, emit);
        else parse_fastq(src, emit, -1, false);
    }
    if (batch.n_reads() > 0) {
        batch.finish();
        sink(batch);
    }
    return delivered;
}

// ------------------------------------------------------------------------------------------ whole reads with qualities

struct DnaQReader::Impl {
    std::string path;
    Compression comp = COMP_NONE;
    bool fastq = false;
    int offset = 64;
    std::unique_ptr<LineSource> src;  // the file's lines, or ...
    std::unique_ptr<MemLines> mem;    // ... those of a range of text in memory
    bool done = false;
    std::string line, data, qual;
    bool getline(std::string &l) { return mem ? mem->getline(l) : src->getline(l); }
    // FastqReader.readNextDataLine: empty lines skipped, a line starting with '@' or '+', then the content line
    bool fastq_line(std::string &out)
    {
        for (;;) {
            if (!getline(line)) return false;
            if (!line.empty()) break;
        }
        if (line[0] != '@' && line[0] != '+') throw Error("Unknown structure of fastq file! Waiting \"@ID\" or \"+ID\" string");
        if (!getline(out)) throw Error("Unexpected end of file. File is corrupted/Format mismatch.");
        return true;
    }
    bool fastq_record()
    {
        if (!fastq_line(data)) return false;
        if (!fastq_line(qual)) throw Error("Unexpected end of file. File is corrupted/Format mismatch.");
        if (data.size() != qual.size()) throw Error("Bad DnaQ record: length of chars and quality is not the same.");
        return true;
    }
    // FastaWithNsReader.readNextDataLine
    bool fasta_record()
    {
        data.clear();
        while (getline(line)) {
            if (!line.empty() && (line[0] == '>' || line[0] == ';')) {
                if (!data.empty()) return true;
            } else {
                data += line;
            }
        }
        return !data.empty();
    }
};

static bool unknown_base(char c) { return c == 'N' || c == 'n' || c == '.'; }

DnaQReader::DnaQReader(const std::string &path) : impl_(new Impl)
{
    Impl &I = *impl_;
    I.path = path;
    const size_t slash = path.find_last_of('/');
    std::string name = lower(slash == std::string::npos ? path : path.substr(slash + 1));
    if (ends_with(name, ".gz")) { I.comp = COMP_GZ; name.resize(name.size() - 3); }
    if (ends_with(name, ".bz2")) { I.comp = COMP_BZ2; name.resize(name.size() - 4); }
    bool binq, fasta;
    reads_format_of(name, &binq, &I.fastq, &fasta);
    if (binq) { delete impl_; throw Error("Illegal format binq: the reads-classifier reads FASTA and FASTQ files"); }
    if (!I.fastq && !fasta) { delete impl_; throw Error("Can't detect file format for file '" + name + "'"); }
    try {
        if (I.fastq) {  // ReadersUtils.determineQualityFormat: a pass over the first 1000 records with Illumina
            I.src.reset(new LineSource(path, I.comp));
            bool sanger = false;
            for (int r = 0; r < 1000 && !sanger && I.fastq_record(); r++)
                for (size_t i = 0; i < I.data.size(); i++)
                    if (!unknown_base(I.data[i]) && ((unsigned char)I.qual[i] < 64 || (unsigned char)I.qual[i] > 126)) { sanger = true; break; }
            I.offset = sanger ? 33 : 64;
        }
        I.src.reset(new LineSource(path, I.comp));
    } catch (...) {
        delete impl_;
        throw;
    }
}

DnaQReader::DnaQReader(const char *b, const char *e, bool fastq, int phred_offset) : impl_(new Impl)
{
    impl_->fastq = fastq;
    impl_->offset = phred_offset;
    impl_->mem.reset(new MemLines(b, e));
}

DnaQReader::~DnaQReader() { delete impl_; }

bool DnaQReader::fastq() const { return impl_->fastq; }
int DnaQReader::phred_offset() const { return impl_->offset; }
bool DnaQReader::compressed() const { return impl_->comp != COMP_NONE; }

size_t DnaQReader::read(DnaQBatch &b, size_t max_reads)
{
    Impl &I = *impl_;
    if (b.offsets.empty()) b.offsets.assign(1, 0);
    size_t got = 0;
    while (!I.done && got < max_reads) {
        if (!(I.fastq ? I.fastq_record() : I.fasta_record())) { I.done = true; break; }
        const size_t n = I.data.size();
        for (size_t i = 0; i < n; i++) {
            const char c = I.data[i];
            if (unknown_base(c)) {  // DnaQBuilder.unsafeAppendUnknown: base 0, phred 0
                b.codes.push_back(0);
                b.phred.push_back(0);
                continue;
            }
            const int code = code_of(c);
            if (code < 0)
                throw Error(std::string("read contains the character '") + c +
                            "': IUPAC codes other than N are replaced at random by the reference "
                            "(itmo!/dna/DnaTools.java:66-117), which has no defined result; rejecting the input");
            int ph = 20;  // ReadersUtils.DEFAULT_PHRED_FOR_FASTA
            if (I.fastq) {
                const int qc = (unsigned char)I.qual[i];
                if (qc < I.offset || qc > 126) throw Error("Invalid quality code char: \"" + std::string(1, (char)qc) + "\" char code = " + std::to_string(qc));
                ph = (qc - I.offset) & 63;  // (DnaQ keeps the phred in 6 bits of a byte: DnaQ.phredAt)
            }
            b.codes.push_back((uint8_t)code);
            b.phred.push_back((uint8_t)ph);
        }
        b.offsets.push_back(b.codes.size());
        got++;
    }
    return got;
}
}  // namespace mch
