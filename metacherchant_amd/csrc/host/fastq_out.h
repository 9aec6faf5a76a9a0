// The classifiers' FASTQ writers (tool_classifiers.cpp) and what --render adds to them, free of HIP so that mc_hosttest runs them under the
// sanitizers: FastqOut (WritersUtils.writeDnaQsToFastqFile, itmo!/io/writers/FastqDedicatedWriter.java:39-60) with put_rendered for
// records that come as text, SideList with the body form for records whose numbers are not known yet, and render_ranges, which cuts
// a batch at the segments of its device view.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "envfinder.h"

namespace mch {

// MC_INGEST_DEBUG=1: the time spent in FastqOut::put / put_rendered (rendering a record and its fwrite, or the fwrite of a block),
// summed over the writers, for the log line "[ingest] FastqOut: ..." at the end of reads-classifier -- the share of the run that
// DESIGN.md 3.14 reports
inline const bool g_time_writers = getenv("MC_INGEST_DEBUG") != nullptr;
inline double g_fastq_out_s = 0;
inline unsigned long long g_fastq_out_n = 0;

struct FastqOut {
    FILE *f = nullptr;
    unsigned long long n = 0;
    std::string path, rec;
    explicit FastqOut(const std::string &p) : path(p)
    {
        f = fopen(p.c_str(), "wb");
        if (!f) throw Error("Failed to write to file " + p);
        setvbuf(f, nullptr, _IOFBF, 1 << 20);
    }
    FastqOut(const FastqOut &) = delete;
    FastqOut &operator=(const FastqOut &) = delete;
    ~FastqOut() { if (f) fclose(f); }
    void close()
    {
        if (f && (fclose(f) != 0)) { f = nullptr; throw Error("Failed to write to file " + path); }
        f = nullptr;
    }
    void put(const uint8_t *codes, const uint8_t *phred, size_t len)
    {
        if (len == 0) throw Error("Empty DnaQ!");
        const auto t0 = g_time_writers ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
        rec = "@" + std::to_string(++n) + "\n";
        const size_t at = rec.size();
        rec.resize(at + 2 * len + 4);
        char *b = &rec[at], *q = b + len + 3;
        for (size_t i = 0; i < len; i++) {
            b[i] = "AGCT"[codes[i] & 3];
            if (phred[i] > 62) throw Error("Invalid quality code byte: " + std::to_string(phred[i]));
            q[i] = (char)(phred[i] + 64);
        }
        b[len] = '\n'; b[len + 1] = '+'; b[len + 2] = '\n'; q[len] = '\n';
        if (fwrite(rec.data(), 1, rec.size(), f) != rec.size()) throw Error("Failed to write to file " + path);
        if (g_time_writers) { g_fastq_out_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); g_fastq_out_n++; }
    }
    // n_records records as they will be in the file, numbered from n + 1 on (mc_render_fastq with first_number = n + 1)
    void put_rendered(const uint8_t *bytes, size_t n_bytes, unsigned long long n_records)
    {
        const auto t0 = g_time_writers ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
        if (n_bytes && fwrite(bytes, 1, n_bytes, f) != n_bytes) throw Error("Failed to write to file " + path);
        n += n_records;
        if (g_time_writers) { g_fastq_out_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); g_fastq_out_n += n_records; }
    }
};

// records kept aside and appended to a FastqOut later: the "second only" halves of the _s files.  Two forms in one temporary file, each
// behind a 64-bit head: a read (its length, then bases and phreds), or a block of bodies (BODIES | the number of records, their
// lengths, then the records as mc_render_fastq gives them for MC_RENDER_UNNUMBERED: each starts at the '\n' behind its number and is
// 2 len + 5 bytes)
struct SideList {
    static constexpr uint64_t BODIES = 1ull << 63;
    FILE *f = tmpfile();
    unsigned long long n_bodies = 0;  // records that came in the body form
    SideList() { if (!f) throw Error("Failed to create a temporary file"); }
    SideList(const SideList &) = delete;
    SideList &operator=(const SideList &) = delete;
    ~SideList() { if (f) fclose(f); }
    void put(const uint8_t *codes, const uint8_t *phred, size_t len)
    {
        const uint64_t n = len;
        if (fwrite(&n, 8, 1, f) != 1 || fwrite(codes, 1, len, f) != len || fwrite(phred, 1, len, f) != len) throw Error("Failed to write a temporary file");
    }
    void put_bodies(const uint8_t *bytes, size_t n_bytes, const uint64_t *lens, size_t n_records)
    {
        if (n_records == 0) return;
        uint64_t sum = 0;
        for (size_t i = 0; i < n_records; i++) sum += 2 * lens[i] + 5;
        if (sum != n_bytes) throw Error("internal: the rendered bodies do not have their reads' lengths");
        const uint64_t head = BODIES | n_records;
        if (fwrite(&head, 8, 1, f) != 1 || fwrite(lens, 8, n_records, f) != n_records || fwrite(bytes, 1, n_bytes, f) != n_bytes)
            throw Error("Failed to write a temporary file");
        n_bodies += n_records;
    }
    void append_to(FastqOut &out)
    {
        rewind(f);
        std::vector<uint8_t> c, q;
        std::vector<uint64_t> lens;
        std::string block;
        uint64_t n = 0;
        while (fread(&n, 8, 1, f) == 1) {
            if (n & BODIES) {  // "@<n>" in front of every body, the block in one write
                const size_t m = (size_t)(n & ~BODIES);
                lens.resize(m);
                if (fread(lens.data(), 8, m, f) != m) throw Error("Failed to read a temporary file");
                uint64_t bytes = 0;
                for (uint64_t l : lens) bytes += 2 * l + 5;
                c.resize(bytes);
                if (fread(c.data(), 1, bytes, f) != bytes) throw Error("Failed to read a temporary file");
                block.clear();
                block.reserve(bytes + 21 * m);
                uint64_t at = 0;
                for (size_t i = 0; i < m; i++) {
                    block += '@';
                    block += std::to_string(out.n + 1 + i);
                    block.append(reinterpret_cast<const char *>(c.data()) + at, 2 * lens[i] + 5);
                    at += 2 * lens[i] + 5;
                }
                out.put_rendered(reinterpret_cast<const uint8_t *>(block.data()), block.size(), m);
                continue;
            }
            c.resize(n);
            q.resize(n);
            if (fread(c.data(), 1, n, f) != n || fread(q.data(), 1, n, f) != n) throw Error("Failed to read a temporary file");
            out.put(c.data(), q.data(), n);
        }
    }
};

// A batch of n reads whose device view is a list of segments per side ((first, n_reads) in batch order, covering 0 .. at least n on
// every side): the sub-ranges [a, b) of reads that lie in one segment on every side, cut at the union of the sides' segment
// boundaries, with the segment of every side.  Empty segments are passed over.
struct RenderRange {
    uint64_t a, b;
    size_t seg[2];
};
inline std::vector<RenderRange> render_ranges(const std::vector<std::pair<uint64_t, uint64_t>> *sides, int n_sides, uint64_t n)
{
    std::vector<RenderRange> out;
    size_t at[2] = {0, 0};
    for (uint64_t a = 0; a < n;) {
        uint64_t b = n;
        RenderRange r{a, 0, {0, 0}};
        for (int s = 0; s < n_sides; s++) {
            const auto &g = sides[s];
            while (at[s] < g.size() && g[at[s]].first + g[at[s]].second <= a) at[s]++;
            if (at[s] == g.size() || g[at[s]].first > a) throw Error("internal: a batch's device view does not cover it");
            b = std::min(b, g[at[s]].first + g[at[s]].second);
            r.seg[s] = at[s];
        }
        r.b = b;
        out.push_back(r);
        a = b;
    }
    return out;
}

}  // namespace mch
