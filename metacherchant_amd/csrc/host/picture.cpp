// See picture.h.  Every function restates the reference lines cited there.
#include "picture.h"

#include <algorithm>

namespace mch {

// ---- initializeStructures + doMerge

namespace {

void merge_nodes(std::vector<PictureNode> &nodes, int k, int first_plus, int second_minus)
{
    const int first_minus = nodes[(size_t)first_plus].rc, second_plus = nodes[(size_t)second_minus].rc;
    auto merge_labels = [&](const std::string &a, const std::string &b) {
        if (a.compare(a.size() - (size_t)(k - 1), (size_t)(k - 1), b, 0, (size_t)(k - 1)) != 0)
            throw Error("Labels should be merged, but can not: " + a + " and " + b);
        return a + b.substr((size_t)(k - 1));
    };
    const std::string new_seq = merge_labels(nodes[(size_t)second_plus].sequence, nodes[(size_t)first_plus].sequence);
    const std::string new_seq_rc = merge_labels(nodes[(size_t)first_minus].sequence, nodes[(size_t)second_minus].sequence);
    nodes[(size_t)second_plus].sequence = new_seq;
    nodes[(size_t)first_minus].sequence = new_seq_rc;
    nodes[(size_t)second_plus].rc = first_minus;
    nodes[(size_t)first_minus].rc = second_plus;
    nodes[(size_t)first_plus].deleted = true;
    nodes[(size_t)second_minus].deleted = true;
}

// doMerge over the nodes listed (ascending), pass after pass until nothing merges; same(e, f): the entries e and f are of one class
template <typename Same>
void merge_loop(std::vector<PictureNode> &nodes, int k, const Same &same, const std::vector<uint32_t> &scan)
{
    for (;;) {
        bool acted = false;
        for (const uint32_t i : scan) {
            if (!nodes[i].deleted && nodes[i].neighbors.size() == 1) {
                const int other = nodes[i].neighbors[0];
                if (nodes[(size_t)other].neighbors.size() != 1 || !same((size_t)i / 2, (size_t)other / 2)) continue;
                merge_nodes(nodes, k, (int)i, other);
                acted = true;
            }
        }
        if (!acted) break;
    }
}

std::vector<kmer_t> node_kmers(int k, const std::vector<kmer_t> &kmers)
{
    std::vector<kmer_t> packed;  // by node id
    packed.reserve(2 * kmers.size());
    for (const kmer_t seq : kmers) {
        packed.push_back(seq);
        packed.push_back(reverse_complement128(seq, k));
    }
    return packed;
}

// add(p, j) for every node j whose (k-1)-prefix is the (k-1)-suffix of node p ^ 1, p ascending and j ascending for each p
template <typename F>
void for_each_neighbour(int k, const std::vector<kmer_t> &packed, F &&add)
{
    // node ids by (k-1)-prefix, in node order: an open-addressing table of chains threaded through next[]
    const size_t n = packed.size();
    size_t cap = 16;
    while (cap < 2 * n) cap *= 2;
    struct Slot { kmer_t key; int head, tail; };
    std::vector<Slot> slots(cap, Slot{0, -1, -1});
    std::vector<int> next(n, -1);
    auto slot_of = [&](kmer_t key) {
        size_t i = KmerHash()(key) & (cap - 1);
        while (slots[i].head >= 0 && slots[i].key != key) i = (i + 1) & (cap - 1);
        return i;
    };
    for (size_t i = 0; i < n; i++) {
        Slot &sl = slots[slot_of(packed[i] >> 2)];
        if (sl.head < 0) { sl.key = packed[i] >> 2; sl.head = (int)i; } else next[(size_t)sl.tail] = (int)i;
        sl.tail = (int)i;
    }
    const kmer_t suffix_mask = kmer_mask(k - 1);
    for (size_t p = 0; p < n; p++)
        for (int j = slots[slot_of(packed[p ^ 1] & suffix_mask)].head; j >= 0; j = next[(size_t)j]) add(p, j);
}

}  // namespace

void unitigs_by_links(int k, const std::vector<kmer_t> &kmers, const std::vector<uint8_t> &cls, UnitigsResult &out)
{
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    out = UnitigsResult{};
    const size_t n = kmers.size(), N = 2 * n;
    if (cls.size() != n) throw Error("unitigs_by_links: one class an entry");
    if (n >= (1ull << 30)) throw Error("unitigs_by_links: too many entries");
    const std::vector<kmer_t> packed = node_kmers(k, kmers);
    {
        std::vector<kmer_t> canon(n);
        for (size_t e = 0; e < n; e++) canon[e] = std::min(packed[2 * e], packed[2 * e + 1]);
        std::sort(canon.begin(), canon.end());
        if (std::adjacent_find(canon.begin(), canon.end()) != canon.end())
            throw Error("unitigs_by_links: two entries are the same k-mer or each other's reverse complement");
    }
    out.deg.assign(N, 0);
    std::vector<uint64_t> at(N + 1, 0);
    for_each_neighbour(k, packed, [&](size_t p, int j) {
        out.deg[p]++;
        out.nbr.push_back((uint32_t)j);
    });
    for (size_t p = 0; p < N; p++) at[p + 1] = at[p] + out.deg[p];
    // links, and which of them are irregular
    std::vector<uint32_t> link(N, NONE);
    std::vector<uint8_t> mark(N, 0);
    for (size_t p = 0; p < N; p++) {
        if (out.deg[p] != 1) continue;
        const size_t q = out.nbr[at[p]];
        if (out.deg[q] != 1 || cls[p / 2] != cls[q / 2]) continue;
        link[p] = (uint32_t)q;
        mark[p] = q == p || q == (p ^ 1);  // (a k-mer that is its own reverse complement never links: both its nodes spell it)
    }
    // chains of oriented nodes from their heads: next(a) = link[a ^ 1]
    std::vector<uint8_t> seen(N, 0), irr(n, 0);
    std::vector<uint32_t> chain;
    for (size_t h = 0; h < N; h++) {
        if (link[h] != NONE) continue;
        chain.clear();
        bool bad = false;
        for (uint32_t a = (uint32_t)h;; a = link[a ^ 1]) {
            chain.push_back(a);
            seen[a] = 1;
            bad = bad || mark[a ^ 1];
            if (link[a ^ 1] == NONE) break;
        }
        const uint32_t last_rc = chain.back() ^ 1;
        if (bad) {
            for (const uint32_t a : chain) irr[a / 2] = 1;
            continue;
        }
        if (chain.size() < 2 || !(h < last_rc)) continue;  // (a chain is listed from that end where first < last_rc)
        out.first.push_back((uint32_t)h);
        out.last_rc.push_back(last_rc);
        const uint64_t base0 = out.bases.size() * 32, len = chain.size() + (size_t)k - 1;
        out.base_offsets.push_back(base0);
        out.bases.resize(out.bases.size() + (len + 31) / 32, 0);
        auto put = [&](uint64_t i, unsigned code) { out.bases[(base0 + i) >> 5] |= (uint64_t)code << (62 - 2 * ((base0 + i) & 31)); };
        for (int i = 0; i < k; i++) put((uint64_t)i, (unsigned)(packed[h] >> (2 * (k - 1 - i))) & 3u);
        for (size_t r = 1; r < chain.size(); r++) put(r + (size_t)k - 1, (unsigned)packed[chain[r]] & 3u);
    }
    out.base_offsets.push_back(out.bases.size() * 32);
    for (size_t a = 0; a < N; a++)  // what no head reaches lies on a cycle
        if (!seen[a]) irr[a / 2] = 1;
    for (size_t e = 0; e < n; e++)
        if (irr[e]) out.irregular.push_back((uint32_t)e);
}

std::vector<PictureNode> make_picture(int k, const std::vector<kmer_t> &kmers, const std::vector<uint8_t> &cls, const Compactor *compact)
{
    // initializeStructures
    const size_t N = 2 * kmers.size();
    const std::vector<kmer_t> packed = node_kmers(k, kmers);
    std::vector<PictureNode> nodes(N);
    for (size_t i = 0; i < N; i++) nodes[i].rc = (int)(i ^ 1);
    const auto same = [&](size_t e, size_t f) { return cls[e] == cls[f]; };
    std::vector<uint32_t> scan;
    if (!compact) {
        for (size_t i = 0; i < N; i++) nodes[i].sequence = unpack_kmer128(packed[i], k);
        for_each_neighbour(k, packed, [&](size_t p, int j) { nodes[p].neighbors.push_back(j); });
        scan.resize(N);
        for (size_t i = 0; i < N; i++) scan[i] = (uint32_t)i;
        merge_loop(nodes, k, same, scan);  // doMerge
        return nodes;
    }
    UnitigsResult r;
    (*compact)(k, kmers, cls, r);
    if (r.deg.size() != N || r.base_offsets.size() != r.first.size() + 1 || r.last_rc.size() != r.first.size())
        throw Error("make_picture: the compactor's result does not fit the k-mers");
    std::vector<uint64_t> at(N + 1, 0);
    for (size_t p = 0; p < N; p++) at[p + 1] = at[p] + r.deg[p];
    if (r.nbr.size() != at[N]) throw Error("make_picture: the compactor's neighbours lists do not fit their lengths");
    for (size_t p = 0; p < N; p++) nodes[p].neighbors.assign(r.nbr.begin() + (long)at[p], r.nbr.begin() + (long)at[p + 1]);
    for (size_t u = 0; u < r.first.size(); u++) {
        // the chain's nodes from a_1 on: next(a) is the one neighbour of a ^ 1.  All but a_1 and a_m ^ 1 are deleted.
        const uint32_t first = r.first[u], last_rc = r.last_rc[u];
        size_t m = 1;
        for (uint32_t a = first; (a ^ 1) != last_rc; m++) {
            if (r.deg[a ^ 1] != 1 || m > N) throw Error("make_picture: a unitig of the compactor's is no chain");
            nodes[a ^ 1].deleted = true;
            a = r.nbr[at[a ^ 1]];
            nodes[a].deleted = true;
        }
        const uint64_t base0 = r.base_offsets[u], len = m + (size_t)k - 1;
        if (base0 % 32 || (base0 + len + 31) / 32 > r.bases.size()) throw Error("make_picture: a unitig of the compactor's has no bases");
        std::string s(len, 'A');
        for (uint64_t i = 0; i < len; i++) s[i] = "AGCT"[(r.bases[(base0 + i) >> 5] >> (62 - 2 * ((base0 + i) & 31))) & 3];
        nodes[last_rc].sequence = reverse_complement(s);
        nodes[first].sequence = std::move(s);
        nodes[first].rc = (int)last_rc;
        nodes[last_rc].rc = (int)first;
    }
    for (size_t i = 0; i < N; i++)  // (a deleted node's label is never read: none is made)
        if (!nodes[i].deleted && nodes[i].sequence.empty()) nodes[i].sequence = unpack_kmer128(packed[i], k);
    for (const uint32_t e : r.irregular) {
        if (e >= kmers.size()) throw Error("make_picture: the compactor lists an entry that is not there");
        scan.push_back(2 * e);
        scan.push_back(2 * e + 1);
    }
    merge_loop(nodes, k, same, scan);
    return nodes;
}

void merge_picture(std::vector<PictureNode> &nodes, int k, const std::function<bool(size_t, size_t)> &same_class)
{
    std::vector<uint32_t> scan(nodes.size());
    for (size_t i = 0; i < scan.size(); i++) scan[i] = (uint32_t)i;
    merge_loop(nodes, k, same_class, scan);
}

void append_fasta_record(std::string &out, const std::vector<PictureNode> &nodes, size_t i, const std::string &label)
{
    const PictureNode &n = nodes[i];
    const auto min_id = [&](size_t j) { return (int)std::min(j, (size_t)nodes[j].rc) + 1; };
    std::vector<int> ids;
    for (const int j : n.neighbors) ids.push_back(min_id((size_t)j));
    for (const int j : nodes[(size_t)n.rc].neighbors) ids.push_back(min_id((size_t)j));
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    ids.erase(std::remove(ids.begin(), ids.end(), min_id(i)), ids.end());
    out += "> Id" + label + " Length:" + std::to_string(n.sequence.size()) + " Neighbors:[";
    for (size_t x = 0; x < ids.size(); x++) out += (x ? ", " : "") + std::to_string(ids[x]);
    out += "]\n" + n.sequence + "\n";
}

}  // namespace mch
