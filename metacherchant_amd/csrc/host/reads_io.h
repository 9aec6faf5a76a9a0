// The host readers of read files (no HIP): packed reads batch by batch from FASTA / FASTQ / binq, plain, .gz or .bz2 (load_reads_file);
// an uncompressed file mapped for the device tokeniser, its chunks and the serial parser for a chunk the device declines; whole reads with
// their qualities (DnaQReader).  The one host unit libmcgpu.so links; java_replay.h, which says what the citations mean, includes it.
#pragma once
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace mch {

struct Error : std::runtime_error {  // plays ExecutionFailedException
    using std::runtime_error::runtime_error;
};

int code_of(char c);  // A0 G1 C2 T3 (case-insensitive), -1 otherwise

// ---- read ingest: itmo!/io/ReadersUtils.java:27-53,104-121 format by extension;
// FASTA: records with N/n dropped whole (itmo!/io/readers/FastaReader.java:54-76);
// FASTQ: split at phred < 1, offset sniffed on the first 1000 records
// (itmo!/io/readers/FastqReader.java:53-112, FastaReaderFromXQSourceTrunc.java:61-95, ReadersUtils.java:57-77).
struct PackedBatch {
    std::vector<uint64_t> words;    // 2-bit packed, layout of include/mcgpu.h, with the pad word
    std::vector<uint64_t> offsets;  // n_reads + 1
    uint64_t n_reads() const { return offsets.empty() ? 0 : offsets.size() - 1; }
    void clear();
    void add_read(const char *s, size_t n);  // pure ACGT (any case); throws Error otherwise
    void finish();                           // appends the pad word
};
// Calls sink(batch) for every max_reads reads; returns the number of reads (pieces) delivered.
uint64_t load_reads_file(const std::string &path, size_t max_reads, const std::function<void(PackedBatch &)> &sink);

// What the device tokeniser (csrc/tokenizer.h) needs from the host: an uncompressed FASTA / FASTQ file mapped, its format,
// the quality offset of its first 1000 records, record starts to cut it at, and this file's own parser for a byte range
// the device declined (a byte that is no base, a record out of shape: the serial parser defines what happens then).
struct PlainReadsFile {
    const char *p = nullptr;
    size_t n = 0;
    bool fastq = false;
    int offset = 0;  // FASTQ: 33 or 64
    int fd = -1;
    PlainReadsFile() = default;
    PlainReadsFile(const PlainReadsFile &) = delete;
    PlainReadsFile &operator=(const PlainReadsFile &) = delete;
    ~PlainReadsFile();
};
// false: compressed, binq, unknown suffix, empty or unmappable, or a FASTQ whose first 1000 records are not plain
// four-part records -- load_reads_file() is the reader for those
bool map_plain_reads(const std::string &path, PlainReadsFile *out);
// first record start at or after q (the end of the file when there is none)
const char *plain_record_start(const PlainReadsFile &f, const char *q);
// the serial parser over [b, e), which must begin at a record start; returns the reads delivered
uint64_t parse_plain_range(const PlainReadsFile &f, const char *b, const char *e, size_t max_reads, const std::function<void(PackedBatch &)> &sink);
// The chunks [b, e) a mapped file is read in, each a whole number of records: a chunk ends at the first record start at or
// after chunk_bytes from its beginning, and a rest of at most chunk_bytes + chunk_bytes / 4 stays whole.  The one statement of
// the cut rule (tests/tokenizer_cases.py cut_positions is its model).
std::vector<std::pair<const char *, const char *>> plain_chunks(const PlainReadsFile &f, uint64_t chunk_bytes);

// ---- whole reads with their qualities, the reads-classifier's -r files: itmo!/io/ReadersUtils.java:185-215 readDnaQLazy.
// FASTQ (itmo!/io/readers/FastqReader.java:70-80): N / n / . become base 0 (A) with phred 0 (itmo!/dna/DnaQBuilder.java:45),
// other bases take the phred of their quality char -- Illumina (+64) unless one of the first 1000 records has a char that is
// not (ReadersUtils.java:63-77), else Sanger (+33) -- kept as DnaQ.phredAt reads it back: in 6 bits.  FASTA (FastaWithNsReader):
// the lines between two '>' / ';' lines joined, empty records skipped, N / n / . as above, phred 20 for every other base.
// Reads are neither split nor dropped.  Plain, .gz or .bz2.
struct DnaQBatch {
    std::vector<uint8_t> codes;     // base codes A0 G1 C2 T3 (N -> 0)
    std::vector<uint8_t> phred;     // 0 .. 63
    std::vector<uint64_t> offsets;  // n_reads + 1
    uint64_t n_reads() const { return offsets.empty() ? 0 : offsets.size() - 1; }
    void clear() { codes.clear(); phred.clear(); offsets.assign(1, 0); }
};
// what a tool does with a batch before mc_classify_reads and its kin: reads first .. first + n - 1 packed 32 bases a word (the pad word
// included) with offsets that start at 0, and findReadWithCorrection's one low-quality position of each (phred < 10): -1 none, -2 several
inline void pack_whole_reads(const DnaQBatch &b, size_t first, size_t n, std::vector<uint64_t> &words, std::vector<uint64_t> *offsets)
{
    const uint64_t o0 = b.offsets[first], nb = b.offsets[first + n] - o0;
    words.assign((nb + 31) / 32 + 1, 0);
    for (uint64_t i = 0; i < nb; i++) words[i >> 5] |= (uint64_t)(b.codes[o0 + i] & 3) << (62 - 2 * (i & 31));
    if (offsets) {
        offsets->resize(n + 1);
        for (size_t r = 0; r <= n; r++) (*offsets)[r] = b.offsets[first + r] - o0;
    }
}
inline std::vector<int32_t> low_quality_positions(const DnaQBatch &b, size_t first, size_t n)
{
    std::vector<int32_t> bad(n, -1);
    for (size_t r = 0; r < n; r++)
        for (uint64_t i = b.offsets[first + r]; i < b.offsets[first + r + 1]; i++)
            if (b.phred[i] < 10) {
                if (bad[r] != -1) { bad[r] = -2; break; }
                bad[r] = (int32_t)(i - b.offsets[first + r]);
            }
    return bad;
}
class DnaQReader {
public:
    explicit DnaQReader(const std::string &path);  // throws Error on a file it cannot read or whose format it cannot tell
    // the same record functions over text in memory: [b, e) starts at a record start of a file of that format and quality offset
    // (a chunk of a mapped file that the device tokeniser declined: the same reads, the same messages)
    DnaQReader(const char *b, const char *e, bool fastq, int phred_offset);
    ~DnaQReader();
    bool fastq() const;
    int phred_offset() const;  // FASTQ: 33 or 64, as the first 1000 records say
    bool compressed() const;
    DnaQReader(const DnaQReader &) = delete;
    DnaQReader &operator=(const DnaQReader &) = delete;
    // appends up to max_reads records to b; returns how many (0: the file is done)
    size_t read(DnaQBatch &b, size_t max_reads);

private:
    struct Impl;
    Impl *impl_;
};

}  // namespace mch
