// See envfinder.h.  Every function restates the reference lines cited there.
#include "envfinder.h"

#include <sys/stat.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <fstream>

namespace mch {

// ------------------------------------------------------------------------------------------ files

static void mkdirs(const std::string &dir)
{
    if (dir.empty()) return;
    std::string cur;
    for (size_t i = 0; i <= dir.size(); i++) {
        if (i == dir.size() || dir[i] == '/') {
            if (!cur.empty() && cur != "/") {
                if (mkdir(cur.c_str(), 0777) != 0 && errno != EEXIST)
                    throw Error("Could not create directory " + cur + ": " + strerror(errno));
            }
        }
        if (i < dir.size()) cur.push_back(dir[i]);
    }
}

void write_file(const std::string &path, const std::string &text)
{
    const size_t slash = path.find_last_of('/');
    if (slash != std::string::npos) mkdirs(path.substr(0, slash));
    std::ofstream f(path, std::ios::binary);
    if (!f) throw Error("Could not write " + path);
    f << text;
}

bool read_lines(const std::string &path, std::vector<std::string> *lines)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::string line;
    while (std::getline(f, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        lines->push_back(line);
    }
    return true;
}

// ------------------------------------------------------------------------------------------ seeds

static std::string dnaq_string(const std::string &s)
{
    std::string r;
    r.reserve(s.size());
    for (char c : s) {
        if (c == 'N' || c == 'n' || c == '.') {
            r.push_back('A');  // DnaQ: unknown -> nuc 0
        } else {
            const int code = code_of(c);
            if (code < 0) throw Error(std::string("Incorrect nucleotide char: \"") + c + "\"");
            r.push_back("AGCT"[code]);
        }
    }
    return r;
}

SeedFile read_seed_fasta(const std::string &path)
{
    std::vector<std::string> lines;
    if (!read_lines(path, &lines)) throw Error("cannot open " + path);
    SeedFile out;
    bool last_comment = true;
    std::string cur_comment, cur_dna;
    for (const std::string &line : lines) {
        if (!line.empty() && (line[0] == '>' || line[0] == ';')) {
            if (!last_comment) {
                out.dnas.push_back(dnaq_string(cur_dna));
                cur_dna.clear();
                cur_comment.clear();
            }
            cur_comment += line.substr(1);
            last_comment = true;
        } else {
            if (last_comment) {
                out.comments.push_back(cur_comment);
                cur_dna.clear();
                cur_comment.clear();
            }
            cur_dna += line;
            last_comment = false;
        }
    }
    if (!cur_comment.empty()) out.comments.push_back(cur_comment);
    if (!cur_dna.empty()) out.dnas.push_back(dnaq_string(cur_dna));
    return out;
}

// ------------------------------------------------------------------------------------------ Environment

Environment::Environment(int k, std::vector<std::string> gene_sequences) : k_(k), genes_(std::move(gene_sequences)), subgraph_(k)
{
    if (k < 1 || k > 63) throw Error("Environment: k must be in 1..63");
    // isGeneNode (:313-320) is `gene.contains(seq) || gene.contains(rc)` on k-long node labels: a lookup in the
    // set of the genes' k-windows.  Labels are upper-case ACGT, so windows holding anything else never match.
    for (const std::string &g : genes_) {
        kmer_t v = 0;
        int valid = 0;
        for (char c : g) {
            int code;
            switch (c) {
            case 'A': code = 0; break;
            case 'G': code = 1; break;
            case 'C': code = 2; break;
            case 'T': code = 3; break;
            default: code = -1;
            }
            if (code < 0) { valid = 0; continue; }
            v = ((v << 2) | (unsigned)code) & kmer_mask(k_);
            if (++valid >= k_) gene_kmers_.push_back(v);
        }
    }
    std::sort(gene_kmers_.begin(), gene_kmers_.end());
    gene_kmers_.erase(std::unique(gene_kmers_.begin(), gene_kmers_.end()), gene_kmers_.end());
}

// runTrimPaths (:241-262) on distanceToKmer `d`, the map of pass p's k-mers
void trim_pass(JavaKmerMap &d, const BfsPass &p, int k, const std::vector<uint8_t> *kept)
{
    if (kept) {
        for (size_t i = 0; i < p.kmers.size(); i++)  // keySet().retainAll(visitedKmers), the walk's answer given
            if (!(*kept)[i] && d.find_entry(p.kmers[i]) >= 0) d.remove(p.kmers[i]);
    } else {
        // runTrimPaths: reverse BFS from lastKmers through getNeighborsByDir(-dir) inside distanceToKmer
        std::vector<kmer_t> queue;
        std::vector<uint8_t> visited(d.n_entries(), 0);
        for (size_t i = 0; i < p.kmers.size(); i++) {
            const int e = d.find_entry(p.kmers[i]);
            if (p.last[i] && !visited[(size_t)e]) { visited[(size_t)e] = 1; queue.push_back(p.kmers[i]); }
        }
        const int dir = -p.dir;
        const int top = 2 * (k - 1);
        for (size_t head = 0; head < queue.size(); head++) {
            const kmer_t kmer = queue[head];
            for (unsigned c = 0; c < 4; c++) {  // A, G, C, T; dir 0 interleaves left and right
                kmer_t nb[2];
                int n = 0;
                if (dir != 1) nb[n++] = ((kmer_t)c << top) | (kmer >> 2);
                if (dir != -1) nb[n++] = ((kmer << 2) & kmer_mask(k)) | c;
                for (int j = 0; j < n; j++) {
                    const int e = d.find_entry(nb[j]);
                    if (e >= 0 && !visited[(size_t)e]) { visited[(size_t)e] = 1; queue.push_back(nb[j]); }
                }
            }
        }
        for (const kmer_t s : p.kmers) {  // keySet().retainAll(visitedKmers): no reordering
            const int e = d.find_entry(s);
            if (e >= 0 && !visited[(size_t)e]) d.remove(s);
        }
    }
}

void Environment::add_pass(const BfsPass &p, bool trim, const std::vector<uint8_t> *kept)
{
    if (kept && kept->size() != p.kmers.size()) throw Error("Environment::add_pass: the mask needs one byte a k-mer of the pass");
    JavaKmerMap d(k_);  // distanceToKmer
    std::vector<int16_t> cov;  // by entry of d
    cov.reserve(p.kmers.size());
    for (size_t i = 0; i < p.kmers.size(); i++) {
        const size_t e = (size_t)d.put(p.kmers[i], p.dist[i]);
        if (e >= cov.size()) cov.resize(e + 1);
        cov[e] = p.cov[i];
    }
    if (trim) trim_pass(d, p, k_, kept);
    d.for_each([&](kmer_t kmer, int, int e) { subgraph_.put(normalize128(kmer, k_), cov[(size_t)e]); });
    if (d.treeified()) d_treeified_ = true;  // (a removal from a treeified bin of distanceToKmer: runTrimPaths)
}

void Environment::add_puts(const std::vector<std::pair<kmer_t, int>> &puts)
{
    for (const auto &p : puts) subgraph_.put(normalize128(p.first, k_), p.second);
}

// (the fmt-visualizer's host replay; scripts/walk_order_bench.py times it)  KmerEnvCalculator.runBfs (:60-76) over one component: `canon` sorted, `count` beside it (zeroed here); the puts in pop order
// (cap: `--replay auto` gives up once the queue holds more entries than that, *abandoned says so; 0: no cap)
std::vector<std::pair<kmer_t, int>> replay_component_walk(int k, kmer_t seed, const std::vector<kmer_t> &canon, std::vector<int> &count,
                                                          size_t cap, bool *abandoned)
{
    const kmer_t kmask = ((kmer_t)1 << (2 * k)) - 1;
    const int top = 2 * (k - 1);
    auto at = [&](kmer_t v) -> int {
        const kmer_t c = normalize128(v, k);
        const auto it = std::lower_bound(canon.begin(), canon.end(), c);
        return it != canon.end() && *it == c ? (int)(it - canon.begin()) : -1;
    };
    std::vector<kmer_t> queue{seed};
    std::vector<std::pair<kmer_t, int>> puts;
    for (size_t head = 0; head < queue.size(); head++) {
        if (cap && queue.size() > cap) {
            *abandoned = true;
            return {};
        }
        const kmer_t kmer = queue[head];
        for (unsigned c = 0; c < 4; c++) {  // allNeighbors: A, G, C, T, the left neighbour before the right one
            const kmer_t nb[2] = {((kmer_t)c << top) | (kmer >> 2), ((kmer << 2) & kmask) | c};
            for (const kmer_t x : nb) {
                const int e = at(x);
                if (e >= 0 && count[(size_t)e] > 0) queue.push_back(x);
            }
        }
        const int e = at(kmer);  // (a member: it was queued with a count above 0)
        puts.emplace_back(kmer, count[(size_t)e]);
        count[(size_t)e] = 0;  // addAndBound(key, -get)
    }
    return puts;
}

static inline void append_uint(std::string &out, unsigned long long v)
{
    char buf[24];
    int n = 0;
    do { buf[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) out.push_back(buf[--n]);
}

std::string Environment::graph_txt() const
{
    std::string out;
    out.reserve(subgraph_.size() * (size_t)(k_ + 8));
    subgraph_.for_each([&](kmer_t key, int v, int) {
        for (int i = k_ - 1; i >= 0; i--) out.push_back("AGCT"[(unsigned)(key >> (2 * i)) & 3u]);
        out.push_back(' ');
        if (v < 0) { out.push_back('-'); append_uint(out, (unsigned long long)(-(long long)v)); }
        else append_uint(out, (unsigned long long)v);
        out.push_back('\n');
    });
    return out;
}

std::vector<kmer_t> Environment::kmers() const
{
    std::vector<kmer_t> out;
    out.reserve(subgraph_.size());
    subgraph_.for_each([&](kmer_t key, int, int) { out.push_back(key); });
    return out;
}

Environment::Colour Environment::colour_of_mask(unsigned mask)
{
    switch (mask & 15u) {
    case 0: return BLACK;
    case 1: return RED;
    case 2: return BLUE;
    case 4: return GREEN;
    case 8: return YELLOW;
    default: return GREY;
    }
}

const char *Environment::colour_name(Colour c)
{
    static const char *const names[] = {"RED", "GREEN", "BLUE", "GREY", "YELLOW", "BLACK"};
    return c < 0 ? "" : names[c];
}

void Environment::set_colours(const std::function<Colour(kmer_t)> &of)
{
    colours_.clear();
    colours_.reserve(subgraph_.size());
    subgraph_.for_each([&](kmer_t seq, int, int) { colours_.push_back(of(seq)); });
    coloured_ = true;
}

Environment::Outside Environment::outside_neighbours() const
{
    Outside o;
    const int top = 2 * (k_ - 1);
    uint32_t ordinal = 0;
    subgraph_.for_each([&](kmer_t kmer, int, int) {
        for (unsigned c = 0; c < 4; c++) {  // allNeighbors: left and right interleaved, A G C T
            const kmer_t nb[2] = {((kmer_t)c << top) | (kmer >> 2), ((kmer << 2) & kmer_mask(k_)) | c};
            for (const kmer_t x : nb)
                if (subgraph_.find_entry(normalize128(x, k_)) < 0) { o.kmers.push_back(x); o.of.push_back(ordinal); }
        }
        ordinal++;
    });
    return o;
}

size_t Environment::extensions(const Outside &o, const uint8_t *in_graph)
{
    size_t n = 0;
    for (size_t i = 0; i < o.of.size();) {  // (the entries of one k-mer lie together)
        size_t j = i, hits = 0;
        for (; j < o.of.size() && o.of[j] == o.of[i]; j++) hits += in_graph[j] != 0;
        n += hits == 1;
        i = j;
    }
    return n;
}

void Environment::create_picture(const Compactor *compact)
{
    std::vector<kmer_t> kmers;
    std::vector<uint8_t> cls;
    kmers.reserve(subgraph_.size());
    is_gene_.clear();
    subgraph_.for_each([&](kmer_t seq, int, int) {
        const kmer_t rc = reverse_complement128(seq, k_);
        const bool g = std::binary_search(gene_kmers_.begin(), gene_kmers_.end(), seq) ||
                       std::binary_search(gene_kmers_.begin(), gene_kmers_.end(), rc);
        const Colour col = coloured_ ? colours_[kmers.size()] : NO_COLOUR;
        kmers.push_back(seq);
        is_gene_.push_back(g);
        cls.push_back((uint8_t)(2 * (col + 1) + (g ? 1 : 0)));  // (doMerge: nodes of one colour and one is_gene; uncoloured nodes all have NO_COLOUR)
    });
    nodes_ = make_picture(k_, kmers, cls, compact);
}

std::string Environment::node_id(size_t i) const
{
    return std::to_string(std::min(i, (size_t)nodes_[i].rc) + 1) + (is_gene_[i / 2] ? "_start" : "");
}

std::string Environment::seqs_fasta(int chunk_length) const
{
    std::string out;
    for (size_t i = 0; i < nodes_.size(); i++) {
        const PictureNode &n = nodes_[i];
        if (n.deleted || !((int)i < n.rc) || (int)n.sequence.size() < chunk_length) continue;
        append_fasta_record(out, nodes_, i, node_id(i));
    }
    return out;
}

std::string Environment::graph_gfa() const
{
    std::string out;
    for (size_t i = 0; i < nodes_.size(); i++) {
        const PictureNode &n = nodes_[i];
        if (n.deleted || n.sequence.compare(nodes_[(size_t)n.rc].sequence) > 0) continue;
        long long coverage = 0;
        const std::string &s = n.sequence;
        kmer_t fw = 0, rc = 0;  // the window and its reverse complement, rolled along the label
        int last = 0;
        for (size_t p = 0; p < s.size(); p++) {
            const unsigned code = (unsigned)code_of(s[p]);
            fw = ((fw << 2) | code) & kmer_mask(k_);
            rc = (rc >> 2) | ((kmer_t)(3u - code) << (2 * (k_ - 1)));
            if (p + 1 < (size_t)k_) continue;
            const int e = subgraph_.find_entry(ascii_rank(fw) < ascii_rank(rc) ? fw : rc);
            if (e < 0) throw Error("graph_gfa: k-mer of a node label is not in the subgraph: " + s.substr(p + 1 - (size_t)k_, (size_t)k_));
            last = subgraph_.value_at(e);
            coverage += last;
        }
        coverage += (long long)last * (k_ - 1);
        out += "S\t" + node_id(i) + "\t" + s + "\tLN:i:" + std::to_string(s.size()) + "\tKC:i:" + std::to_string(coverage) +
               (coloured_ ? std::string("\tCL:Z:") + colour_name(colours_[i / 2]) : std::string(is_gene_[i / 2] ? "\tCL:Z:GREEN" : "")) + "\n";
    }
    for (size_t i = 0; i < nodes_.size(); i++) {
        const PictureNode &a = nodes_[i];
        if (a.deleted) continue;
        for (int jx : a.neighbors) {
            const PictureNode &b = nodes_[(size_t)jx];
            if (b.deleted) continue;
            out += "L\t" + node_id(i) + "\t" + (a.sequence.compare(nodes_[(size_t)a.rc].sequence) >= 0 ? "+" : "-") + "\t" +
                   node_id((size_t)jx) + "\t" + (b.sequence.compare(nodes_[(size_t)b.rc].sequence) <= 0 ? "+" : "-") + "\t" +
                   std::to_string(k_ - 1) + "M\n";
        }
    }
    return out;
}

std::string Environment::tsv_nodes() const
{
    std::string out = "id\tlength\tseq\n";
    for (size_t i = 0; i < nodes_.size(); i++) {
        const PictureNode &n = nodes_[i];
        if (n.deleted || n.sequence.compare(nodes_[(size_t)n.rc].sequence) > 0) continue;
        out += std::to_string(i + 1) + "\t" + std::to_string(n.sequence.size()) + "\t" + n.sequence + "\n";
    }
    return out;
}

std::string Environment::tsv_edges() const
{
    auto nid = [&](size_t i) {
        const size_t rc = (size_t)nodes_[i].rc;
        return (nodes_[i].sequence.compare(nodes_[rc].sequence) <= 0 ? std::to_string(i + 1) : "-" + std::to_string(rc + 1)) +
               (is_gene_[i / 2] ? "_start" : "");
    };
    std::string out = "source\ttarget\n";
    for (const PictureNode &a : nodes_) {
        if (a.deleted) continue;
        for (int jx : a.neighbors) {
            if (nodes_[(size_t)jx].deleted) continue;
            out += nid((size_t)a.rc) + "\t" + nid((size_t)jx) + "\tpp\n";
        }
    }
    return out;
}

void Environment::write_all(const std::string &out_prefix, int chunk_length, const Compactor *compact)
{
    const std::string g = graph_txt();
    write_file(out_prefix + "/graph.txt", g);
    write_file(out_prefix + "/env.txt", g);
    create_picture(compact);
    write_file(out_prefix + "/seqs.fasta", seqs_fasta(chunk_length));
    write_file(out_prefix + "/graph.gfa", graph_gfa());
    write_file(out_prefix + "/tsvs/edges.tsv", tsv_edges());
    write_file(out_prefix + "/tsvs/nodes.tsv", tsv_nodes());
}

// ------------------------------------------------------------------------------------------ cutReads<i>.fasta

CutReadsWriter::CutReadsWriter(const std::string &path, int file_index) : path_(path), f_(nullptr), index_(file_index)
{
    write_file(path, "");  // outputCutReads.getParentFile().mkdirs(); new PrintWriter(...)
    f_ = fopen(path.c_str(), "wb");
    if (!f_) throw Error("Could not write " + path);
}

CutReadsWriter::~CutReadsWriter()
{
    if (f_) fclose(f_);
}

void CutReadsWriter::flush()
{
    if (!buf_.empty() && fwrite(buf_.data(), 1, buf_.size(), f_) != buf_.size()) throw Error("Could not write " + path_);
    buf_.clear();
}

void CutReadsWriter::add(const uint8_t *codes, size_t n)
{
    kept_++;
    buf_.push_back('>');
    append_uint(buf_, (unsigned long long)index_);
    buf_.push_back('|');
    append_uint(buf_, kept_);
    buf_.push_back('\n');
    for (size_t i = 0; i < n; i++) buf_.push_back("AGCT"[codes[i] & 3]);
    buf_.push_back('\n');
    if (buf_.size() >= (1u << 20)) flush();
}

void CutReadsWriter::close()
{
    flush();
    FILE *f = f_;
    f_ = nullptr;
    if (fclose(f) != 0) throw Error("Could not write " + path_);
}

}  // namespace mch
