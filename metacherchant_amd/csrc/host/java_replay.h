// What the host side restates of the JDK and of the DNA alphabet, so that the output files come out byte-identical to the
// reference's: DNA strings and 2-bit packed k-mers, the iteration order of java.util.HashMap (tree bins included) and three of
// Java's number formats.  Nothing here knows a tool.
//
// Citations: src/... = reference src/; itmo!/x = ru/ifmo/genetics/x in lib/itmo-assembler-src.jar.
#pragma once
#include <cstdint>
#include <deque>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

#include "reads_io.h"  // Error, code_of

namespace mch {

// ---- DNA strings (itmo!/dna/DnaTools.java:31,46-64,131-145; src/utils/StringUtils.java:8-41)
std::string reverse_complement(const std::string &s);
std::string normalize_dna(const std::string &s);  // ASCII-lexicographic min of (s, rc(s))
std::vector<std::string> neighbors_by_dir(int dir, const std::string &kmer);  // A,G,C,T order; dir 0 interleaves L,R
void pack_kmer(const std::string &s, uint64_t *hi, uint64_t *lo);
std::string unpack_kmer(uint64_t hi, uint64_t lo, int k);

// ---- 2-bit packed k-mers (k <= 63): base i of the string is bits 2(k-1-i)+1..2(k-1-i), codes A0 G1 C2 T3,
// the layout of mc_bfs_result's hi/lo words (include/mcgpu.h)
typedef unsigned __int128 kmer_t;
kmer_t pack_kmer128(const std::string &s);
inline std::string unpack_kmer128(kmer_t v, int k) { return unpack_kmer((uint64_t)(v >> 64), (uint64_t)v, k); }
kmer_t reverse_complement128(kmer_t v, int k);
kmer_t normalize128(kmer_t v, int k);  // the packed form of normalize_dna(string)
inline uint64_t reverse_pairs64(uint64_t x)
{
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x);
}
// ASCII order is A < C < G < T, the codes are A0 G1 C2 T3: swapping the two bits of every code gives ranks
// whose numeric order is String.compareTo's
inline kmer_t ascii_rank(kmer_t v)
{
    const kmer_t m = ((kmer_t)0x5555555555555555ull << 64) | 0x5555555555555555ull;
    return ((v & m) << 1) | ((v >> 1) & m);
}
inline kmer_t kmer_mask(int bases) { return bases >= 64 ? ~(kmer_t)0 : (((kmer_t)1 << (2 * bases)) - 1); }

// ---- treeified bins of java.util.HashMap (JDK 8 HashMap.TreeNode).  A bin's iteration order is
// its nodes' next-chain, kept here as a vector of entry ids; the red-black tree over the same nodes decides where a new
// node is linked in: treeify() builds the tree in chain order and moves its root to the front (moveRootToFront),
// put() is putTreeVal (the new node goes right behind its tree parent, then balanceInsertion, then the root to the front).
// dir(x, p) = which way x goes below p: by the (signed) spread hash, then String.compareTo -- < 0 left, > 0 right.
class JavaTreeOrder {
public:
    explicit JavaTreeOrder(std::function<int(uint32_t, uint32_t)> dir) : dir_(std::move(dir)) {}
    void treeify(std::vector<uint32_t> &chain);
    void put(std::vector<uint32_t> &chain, uint32_t id);
    // removeTreeNode + balanceDeletion: the chain only loses `id` (with `movable` -- HashMap.remove; an iterator's remove, which
    // is what retainAll uses, passes false -- the root then moves to the front).  Returns true when the bin untreeifies (the tree
    // was too small BEFORE the removal) or is empty: the caller forgets the tree and keeps the chain as a plain list.
    bool remove(std::vector<uint32_t> &chain, uint32_t id, bool movable);
    void forget(const std::vector<uint32_t> &chain) { for (uint32_t id : chain) t_.erase(id); }

private:
    static constexpr uint32_t NIL = 0xFFFFFFFFu;
    struct Node { uint32_t parent = NIL, left = NIL, right = NIL; bool red = false; };
    uint32_t rotate_left(uint32_t root, uint32_t p);
    uint32_t rotate_right(uint32_t root, uint32_t p);
    uint32_t balance_insertion(uint32_t root, uint32_t x);
    uint32_t balance_deletion(uint32_t root, uint32_t x);
    static void root_to_front(std::vector<uint32_t> &chain, uint32_t root);
    std::function<int(uint32_t, uint32_t)> dir_;
    std::unordered_map<uint32_t, Node> t_;
};

// ---- java.util.HashMap<String,Integer> iteration order (JDK 8)
class JavaHashMap {
public:
    JavaHashMap();
    void put(const std::string &key, int value);  // new keys go to the tail of their bin; existing keep their place
    bool contains(const std::string &key) const { return index_.count(key) != 0; }
    int get(const std::string &key) const;         // throws if absent
    bool find(const std::string &key, int *value) const;
    void remove(const std::string &key, bool movable = false);
    size_t size() const { return size_; }
    // The order of a treeified bin is replayed node for node (JavaTreeOrder), removals included (removeTreeNode): nothing sets
    // the flag any more; it stays for callers that ask.
    bool treeified() const { return order_unknown_; }
    size_t bins_treeified() const { return n_treeified_; }  // bins that were treeified at some point (tests)
    template <typename F>
    void for_each(F &&f) const
    {
        for (const auto &bin : bins_)
            for (uint32_t e : bin) f(entries_[e].key, entries_[e].value);
    }

private:
    struct Entry { std::string key; int value; uint32_t hash; };
    void resize();
    int tree_dir(uint32_t x, uint32_t p) const;
    std::deque<Entry> entries_;
    std::vector<std::vector<uint32_t>> bins_;  // (a treeified bin's vector is its next-chain)
    std::vector<char> is_tree_;
    std::unordered_map<std::string, uint32_t> index_;
    JavaTreeOrder tree_;
    size_t cap_ = 16, size_ = 0, n_treeified_ = 0;
    bool order_unknown_ = false;
};

// java.util.HashMap<String, Integer> over k-mer strings held packed: the same bins, resize points, in-bin
// order and treeify detection as JavaHashMap, with String.hashCode() evaluated on the characters the
// packed key stands for.  Entries are chained per bin the way the JDK chains them.
class JavaKmerMap {
public:
    explicit JavaKmerMap(int k);
    int put(kmer_t key, int value);   // entry index; an existing key keeps its place and gets the value
    int find_entry(kmer_t key) const;  // -1 when absent
    int value_at(int e) const { return entries_[(size_t)e].value; }
    void remove(kmer_t key, bool movable = false);
    size_t size() const { return size_; }
    size_t n_entries() const { return entries_.size(); }  // removed ones included: bound of the entry indices
    bool treeified() const { return order_unknown_; }  // (see JavaHashMap::treeified)
    size_t bins_treeified() const { return n_treeified_; }
    template <typename F>
    void for_each(F &&f) const  // f(key, value, entry index) in HashMap iteration order
    {
        for (uint32_t h : head_)
            for (uint32_t e = h; e != NIL; e = entries_[e].next) f(entries_[e].key, entries_[e].value, (int)e);
    }

private:
    static constexpr uint32_t NIL = 0xFFFFFFFFu;
    struct Entry { kmer_t key; int value; uint32_t hash, next; };
    uint32_t hash_of(kmer_t key) const;
    void resize();
    int tree_dir(uint32_t x, uint32_t p) const;
    void relink(size_t bin, const std::vector<uint32_t> &chain);  // head_/tail_/next of a bin from its chain
    int k_;
    std::vector<Entry> entries_;
    std::vector<uint32_t> head_, tail_;
    std::unordered_map<size_t, std::vector<uint32_t>> tree_bins_;  // treeified bins: their next-chains
    JavaTreeOrder tree_;
    size_t cap_ = 16, size_ = 0, n_treeified_ = 0;
    bool order_unknown_ = false;
};

// ---- number formats
// String.format("%.2f", x) for a double: HALF_UP on the shortest decimal that reads back as x (Java's FormattedFloatingDecimal)
std::string java_format_2f(double x);
// Double.toString as JDK 19 and later document it: the shortest decimal that reads back as x, at least one digit after the point,
// plain notation for 10^-3 <= |x| < 10^7 and d.dddE[-]n outside it (seq-cov's columns, src/tools/SequenceCoverage.java:184)
std::string java_double_to_string(double x);
std::string java_format_6_2f(float x);  // String.format("%6.2f", x)

}  // namespace mch
