// See multi.h.  Every function restates the reference lines cited there.
#include "multi.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <unordered_map>

#include "envfinder.h"  // read_seed_fasta, read_lines, write_file

namespace mch {

namespace {

// |v - w| as int arithmetic gives it (wrapping where Java's would), as an unsigned word
inline uint32_t abs_diff_u32(int32_t v, int32_t w)
{
    const int32_t d = (int32_t)((uint32_t)v - (uint32_t)w);
    return d < 0 ? 0u - (uint32_t)d : (uint32_t)d;
}

// What either path knows once its join and its compaction are done: all that the tool's files are written from.
struct MultiPicture {
    int k = 0;
    size_t G = 0;
    std::vector<std::string> env_paths, log;  // (log: the lines so far)
    std::string comment, sequence;            // the gene's
    std::vector<PictureNode> nodes;           // entry e: nodes 2e and 2e + 1; a node's neighbours in the order of their last base, A G C T
    std::vector<uint8_t> is_gene;             // by entry
    std::vector<size_t> n_graphs;             // by entry: how many graphs hold it
    std::vector<long long> kc;                // by node, for the alive ones with index < rc: the depths of the label's windows in all graphs
    std::vector<uint32_t> diff, diff_alt, uni;  // G x G, row i column j at i * G + j: printProbability's sums, wrapping like Java's int
};

// The five texts and the closing log line.
MultiResult render_multi(const MultiPicture &P)
{
    MultiResult R;
    R.log = P.log;
    const std::vector<PictureNode> &nodes = P.nodes;
    const size_t N = nodes.size(), G = P.G;
    // MultiNode's label (MultiSequenceCalculator.java:141-160, GFAWriterMulti.java): the smaller id of the node and its reverse complement, from 1
    auto label = [&](size_t i) { return std::to_string(std::min(i, (size_t)nodes[i].rc) + 1) + (P.is_gene[i / 2] ? "_start" : ""); };

    // outputNodeSequences (MultiSequenceCalculator.java:141-160)
    for (size_t i = 0; i < N; i++)
        if (!nodes[i].deleted && (int)i < nodes[i].rc) append_fasta_record(R.seqs_fasta, nodes, i, label(i));

    // GFAWriterMulti (:37-146)
    auto color = [&](size_t i) -> std::string {
        if (P.is_gene[i / 2]) return "#00ff00";
        const size_t s = P.n_graphs[i / 2];
        if (G == 2) return s == 1 ? "#ff0000" : s == 2 ? "#0000ff" : "#000000";
        if (G == 3) {
            static const char *c3[] = {"#000000", "#ff0000", "#0000ff", "#ff00ff", "#ffff00", "#ffaa00", "#00ffff"};
            return s <= 6 ? c3[s] : "#000000";
        }
        const int v = (int)(256 * s / G);
        char buf[32];
        snprintf(buf, sizeof buf, "#%02X%02X%02X", v, v, v);
        return buf;
    };
    for (size_t i = 0; i < N; i++) {
        const PictureNode &nd = nodes[i];
        if (nd.deleted || !((int)i < nd.rc)) continue;
        const std::string col = color(i);
        R.graph_gfa += "S\t" + label(i) + "\t" + nd.sequence + "\tLN:i:" + std::to_string(nd.sequence.size()) + "\tKC:i:" + std::to_string(P.kc[i]) +
                       "\tCL:Z:" + col + "\tC2:Z:" + col + "\n";
    }
    for (size_t a = 0; a < N; a++) {
        if (nodes[a].deleted) continue;
        for (int j : nodes[a].neighbors)  // (to a deleted neighbour too, as the reference writes it)
            R.graph_gfa += "L\t" + label(a) + "\t" + ((int)a < nodes[a].rc ? "+" : "-") + "\t" + label((size_t)j) + "\t" +
                           (j > nodes[(size_t)j].rc ? "+" : "-") + "\t" + std::to_string(P.k - 1) + "M\n";
    }
    R.gene_fasta = ">" + P.comment + "\n" + P.sequence + "\n";

    // printProbability (EnvironmentFinderMultiMain.java:104-170): 32-bit sums (wrapping like Java's int), float division
    R.jacard_sym = "The[31mWarning! symmetric <<Jaccard distance>> (1 - AB/AUB):\n\n";
    R.jacard_alt = "The[31mWarning! alternative <<Jaccard distance>> (1 - AB/A):\n\n";
    for (size_t i = 0; i < G; i++) {
        R.jacard_sym += P.env_paths[i];
        R.jacard_alt += P.env_paths[i];
        for (size_t j = 0; j < G; j++) {
            const uint32_t diff = P.diff[i * G + j], diff_alt = P.diff_alt[i * G + j], uni = P.uni[i * G + j];
            const int inter = (int)(uni - diff), u = (int)uni, ua = (int)(uni - diff_alt);
            R.jacard_sym += java_format_6_2f(1.0f - (float)inter / (float)u) + " ";
            R.jacard_alt += java_format_6_2f(1.0f - (float)inter / (float)ua) + " ";
        }
        R.jacard_sym += "\n";
        R.jacard_alt += "\n";
    }
    R.log.push_back("INFO Finished processing!");
    return R;
}

// DeBruijnGraphUtils.loadGraph (:13-27): put(line, n, depth) for every "<kmer> <depth>" line of the file, the k-mer being the
// line's first n characters
template <typename Put>
void for_each_graph_line(const std::string &path, Put &&put)
{
    std::vector<std::string> lines;
    if (!read_lines(path, &lines)) throw Error("Couldn't load graph from file " + path);
    for (const std::string &line : lines) {
        if (line.empty()) continue;
        const size_t sp = line.find(' ');
        if (sp == std::string::npos || sp + 1 >= line.size()) throw Error("Couldn't load graph from file " + path + ": bad line '" + line + "'");
        size_t end = line.find(' ', sp + 1);
        const std::string num = line.substr(sp + 1, end == std::string::npos ? std::string::npos : end - sp - 1);
        char *stop = nullptr;
        const long v = strtol(num.c_str(), &stop, 10);
        if (num.empty() || *stop) throw Error("Couldn't load graph from file " + path + ": bad depth '" + num + "'");
        put(line, sp, (int)v);
    }
}

JavaHashMap load_graph(const std::string &path)
{
    JavaHashMap g;
    for_each_graph_line(path, [&](const std::string &line, size_t n, int depth) { g.put(line.substr(0, n), depth); });
    return g;
}

// k, from the first k-mer of the first graph; the reference's error when another k-mer has another length
int common_k(const std::vector<JavaHashMap> &graphs)
{
    int k = -1;
    graphs[0].for_each([&](const std::string &kmer, int) { if (k < 0) k = (int)kmer.size(); });
    if (k < 0) throw Error("The first environment is empty");  // (the reference fails with NoSuchElementException)
    for (const JavaHashMap &g : graphs)
        g.for_each([&](const std::string &kmer, int) {
            if ((int)kmer.size() != k)
                throw Error("K-mers of different lengths encountered: " + std::to_string(k) + " and " + std::to_string(kmer.size()));
        });
    return k;
}

// The picture's first fields, k known: the gene picked from the sequence file and the line that names it
void start_picture(MultiPicture &P, int k, const std::vector<std::string> &env_paths, const std::string &seq_path, int gene_id)
{
    P.k = k;
    P.G = env_paths.size();
    P.env_paths = env_paths;
    SeedFile sf;
    try {
        sf = read_seed_fasta(seq_path);
    } catch (const Error &) {
        throw Error("Could not load sequence file");
    }
    if (gene_id < 1 || (size_t)gene_id > sf.dnas.size() || (size_t)gene_id > sf.comments.size())
        throw Error("--geneid " + std::to_string(gene_id) + " is outside the sequences of " + seq_path);
    P.sequence = sf.dnas[(size_t)gene_id - 1];
    P.comment = sf.comments[(size_t)gene_id - 1];
    const std::string &s = P.sequence;
    P.log.push_back("INFO Combining environments for sequence " +
                    ((int)s.size() >= 2 * k ? s.substr(0, (size_t)k) + "..." + s.substr(s.size() - (size_t)k) + " (length=" + std::to_string(s.size()) + ")" : s));
}

}  // namespace

// ------------------------------------------------------------------------------------------ on k-mer strings

MultiResult environment_finder_multi(const std::vector<std::string> &env_paths, const std::string &seq_path, int gene_id)
{
    MultiPicture P;
    std::vector<JavaHashMap> graphs;
    for (const std::string &p : env_paths) graphs.push_back(load_graph(p));
    if (graphs.empty()) throw Error("Zero environments given");
    if (graphs.size() > 256) P.log.push_back("WARN Found more than 256 environments. Grayscale graph may be not accurate.");
    const int k = common_k(graphs);
    start_picture(P, k, env_paths, seq_path, gene_id);
    const size_t G = P.G;

    // initializeStructures (MultiSequenceCalculator.java:51-100)
    JavaHashMap by_kmer;  // value: node index, -1 = null
    for (const JavaHashMap &g : graphs)
        g.for_each([&](const std::string &kmer, int) {
            by_kmer.put(kmer, -1);
            by_kmer.put(reverse_complement(kmer), -1);
        });
    const size_t size = by_kmer.size();
    std::vector<PictureNode> &nodes = P.nodes;
    nodes.reserve(size);
    {
        std::vector<std::string> order;
        by_kmer.for_each([&](const std::string &kmer, int) { order.push_back(kmer); });
        for (const std::string &kmer : order) {
            const std::string rc = reverse_complement(kmer);
            if (kmer.compare(rc) > 0) continue;
            if (nodes.size() + 2 > size)
                throw Error("palindromic k-mer " + kmer + ": the reference fails here (ArrayIndexOutOfBoundsException)");
            P.is_gene.push_back(P.sequence.find(kmer) != std::string::npos || P.sequence.find(rc) != std::string::npos);
            const int a = (int)nodes.size();
            nodes.resize(nodes.size() + 2);
            nodes[(size_t)a].sequence = kmer;
            nodes[(size_t)a].rc = a + 1;
            nodes[(size_t)a + 1].sequence = rc;
            nodes[(size_t)a + 1].rc = a;
            by_kmer.put(kmer, a);
            by_kmer.put(rc, a + 1);
        }
    }
    const size_t N = nodes.size(), n = N / 2;
    // MultiNode.graphs of an entry's two nodes: one bit a graph, W words an entry (any number of graphs)
    const size_t W = (G + 63) / 64;
    std::vector<uint64_t> held(n * W, 0);
    for (size_t i = 0; i < G; i++)
        graphs[i].for_each([&](const std::string &kmer, int) { held[(size_t)by_kmer.get(kmer) / 2 * W + i / 64] |= 1ull << (i % 64); });
    P.n_graphs.assign(n, 0);
    for (size_t e = 0; e < n; e++)
        for (size_t w = 0; w < W; w++) P.n_graphs[e] += (size_t)__builtin_popcountll(held[e * W + w]);
    for (size_t i = 0; i < N; i++)
        for (const char c : {'A', 'G', 'C', 'T'}) {
            int nb;
            if (by_kmer.find(nodes[i].sequence.substr(1) + c, &nb) && nb >= 0) nodes[i ^ 1].neighbors.push_back(nb);
        }

    // doMerge (:102-139): nodes of one is_gene and one set of graphs
    merge_picture(nodes, k, [&](size_t e, size_t f) {
        return P.is_gene[e] == P.is_gene[f] && std::equal(held.begin() + (long)(e * W), held.begin() + (long)((e + 1) * W), held.begin() + (long)(f * W));
    });

    // KC (GFAWriterMulti.java): every window of a label, in every graph that holds it
    P.kc.assign(N, 0);
    for (size_t i = 0; i < N; i++) {
        const PictureNode &nd = nodes[i];
        if (nd.deleted || !((int)i < nd.rc)) continue;
        for (size_t p = 0; p + (size_t)k <= nd.sequence.size(); p++) {
            const std::string window = normalize_dna(nd.sequence.substr(p, (size_t)k));
            for (const JavaHashMap &g : graphs) {
                int c;
                if (g.find(window, &c)) P.kc[i] += c;
            }
        }
    }

    // printProbability's sums (EnvironmentFinderMultiMain.java:104-170)
    P.diff.assign(G * G, 0);
    P.diff_alt.assign(G * G, 0);
    P.uni.assign(G * G, 0);
    for (size_t i = 0; i < G; i++)
        for (size_t j = 0; j < G; j++) {
            uint32_t &diff = P.diff[i * G + j], &diff_alt = P.diff_alt[i * G + j], &uni = P.uni[i * G + j];
            graphs[i].for_each([&](const std::string &kmer, int v) {
                int w;
                if (!graphs[j].find(kmer, &w)) { diff += (uint32_t)v; diff_alt += (uint32_t)v; uni += (uint32_t)v; }
                else { diff += abs_diff_u32(v, w); diff_alt += abs_diff_u32(v, w); uni += (uint32_t)std::max(v, w); }
            });
            graphs[j].for_each([&](const std::string &kmer, int v) {
                int w;
                if (!graphs[i].find(kmer, &w)) { diff += (uint32_t)v; uni += (uint32_t)v; }
            });
        }
    return render_multi(P);
}

// ------------------------------------------------------------------------------------------ on packed k-mers

void env_join_host(const EnvJoinInput &in, EnvJoinResult &out)
{
    out = EnvJoinResult{};
    const int k = in.k;
    const size_t n = in.entries.size(), G = in.n_graphs();
    if (G == 0 || G > 64) throw Error("env_join_host: " + std::to_string(G) + " graphs (1 to 64)");
    if (n >= (1ull << 30)) throw Error("env_join_host: too many entries");
    if (in.graph_offsets[0] != 0 || in.graph_offsets[G] != in.rec_kmers.size() || in.rec_depth.size() != in.rec_kmers.size())
        throw Error("env_join_host: graph_offsets do not fit the records");
    std::unordered_map<kmer_t, uint32_t, KmerHash> row_of;  // both orientations of every entry
    row_of.reserve(4 * n);
    for (size_t e = 0; e < n; e++) {
        const kmer_t v = in.entries[e], r = reverse_complement128(v, k);
        const bool fresh = row_of.emplace(v, (uint32_t)(2 * e)).second && (r == v || row_of.emplace(r, (uint32_t)(2 * e + 1)).second);
        if (!fresh) throw Error("env_join_host: two entries are the same k-mer or each other's reverse complement");
    }
    std::vector<uint64_t> holder(2 * n, 0);
    std::vector<int32_t> depth(2 * n * G, 0);
    for (size_t g = 0; g < G; g++) {
        if (in.graph_offsets[g] > in.graph_offsets[g + 1]) throw Error("env_join_host: graph_offsets decrease");
        for (uint64_t r = in.graph_offsets[g]; r < in.graph_offsets[g + 1]; r++) {
            const auto it = row_of.find(in.rec_kmers[r]);
            if (it == row_of.end()) throw Error("env_join_host: a record's k-mer is no entry, and neither is its reverse complement");
            if (holder[it->second] >> g & 1) throw Error("env_join_host: a graph holds the same oriented k-mer twice");
            holder[it->second] |= 1ull << g;
            depth[(size_t)it->second * G + g] = in.rec_depth[r];
        }
    }
    out.member.assign(n, 0);
    out.is_gene.assign(n, 0);
    out.kc.assign(n, 0);
    out.diff.assign(G * G, 0);
    out.diff_alt.assign(G * G, 0);
    out.uni.assign(G * G, 0);
    {
        kmer_t v = 0;
        for (uint64_t i = 0; i < in.gene_len; i++) {
            v = ((v << 2) | ((in.gene_words[i >> 5] >> (62 - 2 * (i & 31))) & 3)) & kmer_mask(k);
            if (i + 1 < (uint64_t)k) continue;
            const auto it = row_of.find(v);
            if (it != row_of.end()) out.is_gene[it->second / 2] = 1;
        }
    }
    for (size_t row = 0; row < 2 * n; row++) {
        const uint64_t H = holder[row];
        const int32_t *d = depth.data() + row * G;
        out.member[row / 2] |= H;
        for (size_t i = 0; i < G; i++) {
            if (!(H >> i & 1)) continue;
            if (!(row & 1)) out.kc[row / 2] += d[i];
            for (size_t j = 0; j < G; j++) {
                if (H >> j & 1) {
                    out.diff[i * G + j] += abs_diff_u32(d[i], d[j]);
                    out.diff_alt[i * G + j] += abs_diff_u32(d[i], d[j]);
                    out.uni[i * G + j] += (uint32_t)std::max(d[i], d[j]);
                } else {
                    out.diff[i * G + j] += (uint32_t)d[i];
                    out.diff_alt[i * G + j] += (uint32_t)d[i];
                    out.uni[i * G + j] += (uint32_t)d[i];
                    out.diff[j * G + i] += (uint32_t)d[i];  // (seen from j, which does not hold the k-mer)
                    out.uni[j * G + i] += (uint32_t)d[i];
                }
            }
        }
    }
}

namespace {
struct PackedGraphFile {
    std::vector<kmer_t> kmers;  // line order
    std::vector<int> depths;
};

// loadGraph with the key packed; lengths: every key's length as it comes
PackedGraphFile load_graph_packed(const std::string &path, std::vector<size_t> *lengths)
{
    PackedGraphFile g;
    for_each_graph_line(path, [&](const std::string &line, size_t sp, int depth) {
        if (sp > 63) throw MultiUnpacked("k = " + std::to_string(sp) + " is above 63");
        if (sp == 0) throw MultiUnpacked("an empty k-mer in " + path);
        kmer_t key = 0;
        for (size_t i = 0; i < sp; i++) {
            unsigned code;
            switch (line[i]) {
            case 'A': code = 0; break;
            case 'G': code = 1; break;
            case 'C': code = 2; break;
            case 'T': code = 3; break;
            default: throw MultiUnpacked("a k-mer with a character outside upper-case ACGT in " + path + ": '" + line.substr(0, sp) + "'");
            }
            key = (key << 2) | code;
        }
        g.kmers.push_back(key);
        g.depths.push_back(depth);
        lengths->push_back(sp);
    });
    return g;
}
}  // namespace

MultiResult environment_finder_multi_packed(const std::vector<std::string> &env_paths, const std::string &seq_path, int gene_id, const Joiner &join,
                                            const Compactor &compact, size_t *n_entries)
{
    MultiPicture P;
    if (env_paths.size() > 64) throw MultiUnpacked(std::to_string(env_paths.size()) + " environments are more than 64");
    std::vector<PackedGraphFile> files;
    std::vector<size_t> lengths;
    for (const std::string &p : env_paths) files.push_back(load_graph_packed(p, &lengths));
    if (files.empty()) throw Error("Zero environments given");
    if (files[0].kmers.empty()) throw Error("The first environment is empty");
    if (std::adjacent_find(lengths.begin(), lengths.end(), std::not_equal_to<size_t>()) != lengths.end()) {
        // which two lengths the message names depends on the string maps' iteration order: theirs is asked (an error's path only)
        std::vector<JavaHashMap> graphs;
        for (const std::string &p : env_paths) graphs.push_back(load_graph(p));
        common_k(graphs);
    }
    const int k = (int)lengths[0];
    const size_t G = files.size();
    std::vector<JavaKmerMap> graphs;  // the last line of a k-mer wins; the iteration order is the HashMap's
    for (const PackedGraphFile &f : files) {
        graphs.emplace_back(k);
        for (size_t i = 0; i < f.kmers.size(); i++) graphs.back().put(f.kmers[i], f.depths[i]);
    }
    files.clear();
    start_picture(P, k, env_paths, seq_path, gene_id);

    // initializeStructures (MultiSequenceCalculator.java:51-100): the entries
    EnvJoinInput in;
    in.k = k;
    {
        JavaKmerMap by_kmer(k);
        for (const JavaKmerMap &g : graphs)
            g.for_each([&](kmer_t kmer, int, int) {
                by_kmer.put(kmer, -1);
                by_kmer.put(reverse_complement128(kmer, k), -1);
            });
        const size_t size = by_kmer.size();
        by_kmer.for_each([&](kmer_t kmer, int, int) {
            const kmer_t rc = reverse_complement128(kmer, k);
            if (ascii_rank(kmer) > ascii_rank(rc)) return;
            if (2 * in.entries.size() + 2 > size)
                throw Error("palindromic k-mer " + unpack_kmer128(kmer, k) + ": the reference fails here (ArrayIndexOutOfBoundsException)");
            in.entries.push_back(kmer);
        });
    }
    const size_t n = in.entries.size();
    if (n_entries) *n_entries = n;
    in.graph_offsets.push_back(0);
    for (const JavaKmerMap &g : graphs) {
        g.for_each([&](kmer_t kmer, int depth, int) {
            in.rec_kmers.push_back(kmer);
            in.rec_depth.push_back(depth);
        });
        in.graph_offsets.push_back(in.rec_kmers.size());
    }
    graphs.clear();
    in.gene_len = P.sequence.size();  // (upper-case ACGT: read_seed_fasta makes it so)
    in.gene_words.assign((P.sequence.size() + 31) / 32, 0);
    for (size_t i = 0; i < P.sequence.size(); i++) in.gene_words[i >> 5] |= (uint64_t)code_of(P.sequence[i]) << (62 - 2 * (i & 31));
    EnvJoinResult J;
    join(in, J);
    if (J.member.size() != n || J.is_gene.size() != n || J.kc.size() != n || J.diff.size() != G * G || J.diff_alt.size() != G * G || J.uni.size() != G * G)
        throw Error("environment_finder_multi_packed: the joiner's result does not fit the entries");
    in.rec_kmers.clear();
    in.rec_depth.clear();

    // doMerge (:102-139) merges nodes of one is_gene and one set of graphs: the merge class is the pair's dense rank
    std::vector<uint8_t> cls(n);
    {
        std::map<std::pair<uint8_t, uint64_t>, int> rank;
        for (size_t e = 0; e < n; e++) rank.emplace(std::make_pair(J.is_gene[e], J.member[e]), 0);
        if (rank.size() > 256) throw MultiUnpacked(std::to_string(rank.size()) + " merge classes (sets of graphs, with and without the gene) are more than 256");
        int next = 0;
        for (auto &kv : rank) kv.second = next++;
        for (size_t e = 0; e < n; e++) cls[e] = (uint8_t)rank[std::make_pair(J.is_gene[e], J.member[e])];
    }
    std::vector<uint8_t> irregular(n, 0);  // entries whose nodes the loop on labels merged
    const Compactor keep_irregular = [&](int kk, const std::vector<kmer_t> &kmers, const std::vector<uint8_t> &c, UnitigsResult &out) {
        compact(kk, kmers, c, out);
        for (const uint32_t e : out.irregular)
            if (e < n) irregular[e] = 1;
    };
    std::vector<PictureNode> &nodes = P.nodes;
    nodes = make_picture(k, in.entries, cls, &keep_irregular);
    const size_t N = nodes.size();
    auto node_kmer = [&](size_t i) { return (i & 1) ? reverse_complement128(in.entries[i / 2], k) : in.entries[i / 2]; };
    // the reference lists a node's neighbours in the order of their last base, A G C T: the codes' order
    for (PictureNode &nd : nodes)
        std::sort(nd.neighbors.begin(), nd.neighbors.end(),
                  [&](int a, int b) { return ((unsigned)node_kmer((size_t)a) & 3u) < ((unsigned)node_kmer((size_t)b) & 3u); });

    // KC: the joiner's sums over the entries that are a label's windows
    P.kc.assign(N, 0);
    std::unordered_map<kmer_t, uint32_t, KmerHash> entry_of;  // (only when the loop on labels merged something)
    for (size_t i = 0; i < N; i++) {
        const PictureNode &nd = nodes[i];
        if (nd.deleted || !((int)i < nd.rc)) continue;
        long long coverage = 0;
        if (!irregular[i / 2]) {
            // a unitig's windows are its chain's entries: next(a) is the one neighbour of a ^ 1, up to the node whose twin is rc
            size_t steps = 0;
            for (size_t a = i;; a = (size_t)nodes[a ^ 1].neighbors[0]) {
                coverage += J.kc[a / 2];
                if ((int)(a ^ 1) == nd.rc) break;
                if (nodes[a ^ 1].neighbors.size() != 1 || ++steps > N) throw Error("environment_finder_multi_packed: a merged node is no chain");
            }
        } else {
            if (entry_of.empty())
                for (size_t e = 0; e < n; e++) entry_of.emplace(in.entries[e], (uint32_t)e);
            kmer_t fw = 0, rc = 0;
            for (size_t p = 0; p < nd.sequence.size(); p++) {
                const unsigned code = (unsigned)code_of(nd.sequence[p]);
                fw = ((fw << 2) | code) & kmer_mask(k);
                rc = (rc >> 2) | ((kmer_t)(3u - code) << (2 * (k - 1)));
                if (p + 1 < (size_t)k) continue;
                const auto it = entry_of.find(ascii_rank(fw) < ascii_rank(rc) ? fw : rc);
                if (it != entry_of.end()) coverage += J.kc[it->second];
            }
        }
        P.kc[i] = coverage;
    }
    P.n_graphs.resize(n);
    for (size_t e = 0; e < n; e++) P.n_graphs[e] = (size_t)__builtin_popcountll(J.member[e]);
    P.is_gene = std::move(J.is_gene);
    P.diff = std::move(J.diff);
    P.diff_alt = std::move(J.diff_alt);
    P.uni = std::move(J.uni);
    return render_multi(P);
}

void write_multi(const MultiResult &r, const std::string &output_dir)
{
    write_file(output_dir + "/seqs.fasta", r.seqs_fasta);
    write_file(output_dir + "/graph.gfa", r.graph_gfa);
    write_file(output_dir + "/gene.fasta", r.gene_fasta);
    write_file(output_dir + "/Jacard_sym.txt", r.jacard_sym);
    write_file(output_dir + "/Jacard_alt.txt", r.jacard_alt);
}

}  // namespace mch
