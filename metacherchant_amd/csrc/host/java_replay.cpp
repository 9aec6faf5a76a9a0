// See java_replay.h.  Every function restates the reference lines cited there.
#include "java_replay.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

namespace mch {

// ------------------------------------------------------------------------------------------ DNA strings

static inline char complement_char(char c)
{
    switch (c) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'T': return 'A';
    default: throw Error(std::string("Incorrect nucleotide char: \"") + c + "\"");
    }
}

std::string reverse_complement(const std::string &s)
{
    std::string r(s.size(), 'A');
    for (size_t i = 0; i < s.size(); i++) r[i] = complement_char(s[s.size() - 1 - i]);
    return r;
}

std::string normalize_dna(const std::string &s)
{
    std::string rc = reverse_complement(s);
    return s.compare(rc) < 0 ? s : rc;  // String.compareTo on ASCII
}

std::vector<std::string> neighbors_by_dir(int dir, const std::string &kmer)
{
    static const char NUC[4] = {'A', 'G', 'C', 'T'};  // DnaTools.NUCLEOTIDES
    std::vector<std::string> out;
    const std::string head = kmer.substr(0, kmer.size() - 1), tail = kmer.substr(1);
    if (dir == -1) {
        for (char c : NUC) out.push_back(std::string(1, c) + head);
    } else if (dir == 1) {
        for (char c : NUC) out.push_back(tail + c);
    } else {
        for (char c : NUC) {
            out.push_back(std::string(1, c) + head);
            out.push_back(tail + c);
        }
    }
    return out;
}

void pack_kmer(const std::string &s, uint64_t *hi, uint64_t *lo)
{
    unsigned __int128 v = 0;
    for (char c : s) {
        const int code = code_of(c);
        if (code < 0) throw Error(std::string("Incorrect nucleotide char: \"") + c + "\"");
        v = (v << 2) | (unsigned)code;
    }
    *hi = (uint64_t)(v >> 64);
    *lo = (uint64_t)v;
}

std::string unpack_kmer(uint64_t hi, uint64_t lo, int k)
{
    const unsigned __int128 v = ((unsigned __int128)hi << 64) | lo;
    std::string s((size_t)k, 'A');
    for (int i = 0; i < k; i++) s[(size_t)i] = "AGCT"[(unsigned)(v >> (2 * (k - 1 - i))) & 3u];
    return s;
}

// ---- packed k-mers

kmer_t pack_kmer128(const std::string &s)
{
    uint64_t hi, lo;
    pack_kmer(s, &hi, &lo);
    return ((kmer_t)hi << 64) | lo;
}

kmer_t reverse_complement128(kmer_t v, int k)
{
    // complement is 3 - code (A0<->T3, G1<->C2); then the 2-bit groups in reverse order
    const kmer_t c = ~v;
    const kmer_t r = ((kmer_t)reverse_pairs64((uint64_t)c) << 64) | reverse_pairs64((uint64_t)(c >> 64));
    return r >> (128 - 2 * k);
}

kmer_t normalize128(kmer_t v, int k)
{
    const kmer_t rc = reverse_complement128(v, k);
    return ascii_rank(v) < ascii_rank(rc) ? v : rc;
}

// ------------------------------------------------------------------------------------------ JavaTreeOrder
// java.util.HashMap.TreeNode (JDK 8): treeify, putTreeVal, balanceInsertion, rotateLeft / rotateRight, moveRootToFront.

uint32_t JavaTreeOrder::rotate_left(uint32_t root, uint32_t p)
{
    if (p == NIL) return root;
    const uint32_t r = t_[p].right;
    if (r == NIL) return root;
    const uint32_t rl = t_[p].right = t_[r].left;
    if (rl != NIL) t_[rl].parent = p;
    const uint32_t pp = t_[r].parent = t_[p].parent;
    if (pp == NIL) { root = r; t_[r].red = false; }
    else if (t_[pp].left == p) t_[pp].left = r;
    else t_[pp].right = r;
    t_[r].left = p;
    t_[p].parent = r;
    return root;
}

uint32_t JavaTreeOrder::rotate_right(uint32_t root, uint32_t p)
{
    if (p == NIL) return root;
    const uint32_t l = t_[p].left;
    if (l == NIL) return root;
    const uint32_t lr = t_[p].left = t_[l].right;
    if (lr != NIL) t_[lr].parent = p;
    const uint32_t pp = t_[l].parent = t_[p].parent;
    if (pp == NIL) { root = l; t_[l].red = false; }
    else if (t_[pp].right == p) t_[pp].right = l;
    else t_[pp].left = l;
    t_[l].right = p;
    t_[p].parent = l;
    return root;
}

uint32_t JavaTreeOrder::balance_insertion(uint32_t root, uint32_t x)
{
    t_[x].red = true;
    for (;;) {
        uint32_t xp = t_[x].parent;
        if (xp == NIL) { t_[x].red = false; return x; }
        uint32_t xpp = t_[xp].parent;
        if (!t_[xp].red || xpp == NIL) return root;
        const uint32_t xppl = t_[xpp].left;
        if (xp == xppl) {
            const uint32_t xppr = t_[xpp].right;
            if (xppr != NIL && t_[xppr].red) {
                t_[xppr].red = false; t_[xp].red = false; t_[xpp].red = true; x = xpp;
            } else {
                if (x == t_[xp].right) {
                    x = xp;
                    root = rotate_left(root, x);
                    xp = t_[x].parent;
                    xpp = xp == NIL ? NIL : t_[xp].parent;
                }
                if (xp != NIL) {
                    t_[xp].red = false;
                    if (xpp != NIL) { t_[xpp].red = true; root = rotate_right(root, xpp); }
                }
            }
        } else {
            if (xppl != NIL && t_[xppl].red) {
                t_[xppl].red = false; t_[xp].red = false; t_[xpp].red = true; x = xpp;
            } else {
                if (x == t_[xp].left) {
                    x = xp;
                    root = rotate_right(root, x);
                    xp = t_[x].parent;
                    xpp = xp == NIL ? NIL : t_[xp].parent;
                }
                if (xp != NIL) {
                    t_[xp].red = false;
                    if (xpp != NIL) { t_[xpp].red = true; root = rotate_left(root, xpp); }
                }
            }
        }
    }
}

void JavaTreeOrder::root_to_front(std::vector<uint32_t> &chain, uint32_t root)
{   // moveRootToFront: the root leaves its place in the chain and becomes its head
    if (chain.empty() || chain[0] == root) return;
    chain.erase(std::find(chain.begin(), chain.end(), root));
    chain.insert(chain.begin(), root);
}

void JavaTreeOrder::treeify(std::vector<uint32_t> &chain)
{
    uint32_t root = NIL;
    for (uint32_t x : chain) {
        t_[x] = Node{};
        if (root == NIL) { root = x; continue; }
        for (uint32_t p = root;;) {
            const int d = dir_(x, p);
            const uint32_t xp = p;
            p = d <= 0 ? t_[p].left : t_[p].right;
            if (p == NIL) {
                t_[x].parent = xp;
                if (d <= 0) t_[xp].left = x; else t_[xp].right = x;
                root = balance_insertion(root, x);
                break;
            }
        }
    }
    root_to_front(chain, root);
}

void JavaTreeOrder::put(std::vector<uint32_t> &chain, uint32_t id)
{   // putTreeVal for a key known to be absent
    uint32_t root = chain[0];
    while (t_[root].parent != NIL) root = t_[root].parent;
    for (uint32_t p = root;;) {
        const int d = dir_(id, p);
        const uint32_t xp = p;
        p = d <= 0 ? t_[p].left : t_[p].right;
        if (p == NIL) {
            t_[id] = Node{};
            t_[id].parent = xp;
            if (d <= 0) t_[xp].left = id; else t_[xp].right = id;
            chain.insert(std::find(chain.begin(), chain.end(), xp) + 1, id);  // xp.next = x
            root_to_front(chain, balance_insertion(root, id));
            return;
        }
    }
}

uint32_t JavaTreeOrder::balance_deletion(uint32_t root, uint32_t x)
{   // HashMap.TreeNode.balanceDeletion (JDK 8)
    auto red = [&](uint32_t n) { return n != NIL && t_[n].red; };
    for (;;) {
        if (x == NIL || x == root) return root;
        uint32_t xp = t_[x].parent;
        if (xp == NIL) { t_[x].red = false; return x; }
        if (t_[x].red) { t_[x].red = false; return root; }
        uint32_t xpl = t_[xp].left;
        if (xpl == x) {
            uint32_t xpr = t_[xp].right;
            if (red(xpr)) {
                t_[xpr].red = false; t_[xp].red = true;
                root = rotate_left(root, xp);
                xp = t_[x].parent;
                xpr = xp == NIL ? NIL : t_[xp].right;
            }
            if (xpr == NIL) { x = xp; continue; }
            uint32_t sl = t_[xpr].left, sr = t_[xpr].right;
            if (!red(sr) && !red(sl)) { t_[xpr].red = true; x = xp; continue; }
            if (!red(sr)) {
                if (sl != NIL) t_[sl].red = false;
                t_[xpr].red = true;
                root = rotate_right(root, xpr);
                xp = t_[x].parent;
                xpr = xp == NIL ? NIL : t_[xp].right;
            }
            if (xpr != NIL) {
                t_[xpr].red = xp == NIL ? false : t_[xp].red;
                sr = t_[xpr].right;
                if (sr != NIL) t_[sr].red = false;
            }
            if (xp != NIL) { t_[xp].red = false; root = rotate_left(root, xp); }
            x = root;
        } else {  // symmetric
            if (red(xpl)) {
                t_[xpl].red = false; t_[xp].red = true;
                root = rotate_right(root, xp);
                xp = t_[x].parent;
                xpl = xp == NIL ? NIL : t_[xp].left;
            }
            if (xpl == NIL) { x = xp; continue; }
            uint32_t sl = t_[xpl].left, sr = t_[xpl].right;
            if (!red(sl) && !red(sr)) { t_[xpl].red = true; x = xp; continue; }
            if (!red(sl)) {
                if (sr != NIL) t_[sr].red = false;
                t_[xpl].red = true;
                root = rotate_left(root, xpl);
                xp = t_[x].parent;
                xpl = xp == NIL ? NIL : t_[xp].left;
            }
            if (xpl != NIL) {
                t_[xpl].red = xp == NIL ? false : t_[xp].red;
                sl = t_[xpl].left;
                if (sl != NIL) t_[sl].red = false;
            }
            if (xp != NIL) { t_[xp].red = false; root = rotate_right(root, xp); }
            x = root;
        }
    }
}

bool JavaTreeOrder::remove(std::vector<uint32_t> &chain, uint32_t p, bool movable)
{   // HashMap.TreeNode.removeTreeNode (JDK 8)
    uint32_t root = chain[0];  // ("first" as it was before the node left the chain)
    chain.erase(std::find(chain.begin(), chain.end(), p));
    if (chain.empty()) { t_.erase(p); return true; }
    while (t_[root].parent != NIL) root = t_[root].parent;
    {
        const uint32_t rl = t_[root].left;
        if (t_[root].right == NIL || rl == NIL || t_[rl].left == NIL) { t_.erase(p); return true; }  // too small: untreeify
    }
    const uint32_t pl = t_[p].left, pr = t_[p].right;
    uint32_t replacement;
    if (pl != NIL && pr != NIL) {
        uint32_t s = pr;
        while (t_[s].left != NIL) s = t_[s].left;  // the successor
        std::swap(t_[s].red, t_[p].red);
        const uint32_t sr = t_[s].right, pp = t_[p].parent;
        if (s == pr) {  // p was s's direct parent
            t_[p].parent = s;
            t_[s].right = p;
        } else {
            const uint32_t sp = t_[s].parent;
            t_[p].parent = sp;
            if (sp != NIL) { if (s == t_[sp].left) t_[sp].left = p; else t_[sp].right = p; }
            t_[s].right = pr;
            if (pr != NIL) t_[pr].parent = s;
        }
        t_[p].left = NIL;
        t_[p].right = sr;
        if (sr != NIL) t_[sr].parent = p;
        t_[s].left = pl;
        if (pl != NIL) t_[pl].parent = s;
        t_[s].parent = pp;
        if (pp == NIL) root = s;
        else if (p == t_[pp].left) t_[pp].left = s;
        else t_[pp].right = s;
        replacement = sr != NIL ? sr : p;
    } else if (pl != NIL) replacement = pl;
    else if (pr != NIL) replacement = pr;
    else replacement = p;
    if (replacement != p) {
        const uint32_t pp = t_[replacement].parent = t_[p].parent;
        if (pp == NIL) root = replacement;
        else if (p == t_[pp].left) t_[pp].left = replacement;
        else t_[pp].right = replacement;
        t_[p].left = t_[p].right = t_[p].parent = NIL;
    }
    const uint32_t r = t_[p].red ? root : balance_deletion(root, replacement);
    if (replacement == p) {  // detach
        const uint32_t pp = t_[p].parent;
        t_[p].parent = NIL;
        if (pp != NIL) {
            if (p == t_[pp].left) t_[pp].left = NIL;
            else if (p == t_[pp].right) t_[pp].right = NIL;
        }
    }
    t_.erase(p);
    if (movable) root_to_front(chain, r);
    return false;
}

// ------------------------------------------------------------------------------------------ JavaHashMap

static uint32_t java_string_hash(const std::string &s)
{
    uint32_t h = 0;
    for (unsigned char c : s) h = 31u * h + c;
    return h;
}

JavaHashMap::JavaHashMap() : bins_(16), is_tree_(16, 0), tree_([this](uint32_t x, uint32_t p) { return tree_dir(x, p); }) {}

int JavaHashMap::tree_dir(uint32_t x, uint32_t p) const
{   // TreeNode order: the (signed) spread hash, then String.compareTo (distinct keys never compare equal)
    const int32_t h = (int32_t)entries_[x].hash, ph = (int32_t)entries_[p].hash;
    if (ph > h) return -1;
    if (ph < h) return 1;
    return entries_[x].key < entries_[p].key ? -1 : 1;
}

void JavaHashMap::put(const std::string &key, int value)
{
    auto it = index_.find(key);
    if (it != index_.end()) {
        entries_[it->second].value = value;
        return;
    }
    uint32_t h = java_string_hash(key);
    h ^= h >> 16;
    const uint32_t e = (uint32_t)entries_.size();
    entries_.push_back(Entry{key, value, h});
    index_.emplace(key, e);
    const size_t b = h & (cap_ - 1);
    auto &bin = bins_[b];
    if (is_tree_[b]) {
        tree_.put(bin, e);
    } else {
        bin.push_back(e);
        if (bin.size() >= 9) {  // a 9th node: treeifyBin (or a resize while the table is smaller than 64)
            if (cap_ >= 64) { tree_.treeify(bin); is_tree_[b] = 1; n_treeified_++; } else resize();
        }
    }
    size_++;
    if ((double)size_ > 0.75 * (double)cap_) resize();
}

void JavaHashMap::resize()
{
    const size_t ocap = cap_, ncap = cap_ * 2;
    std::vector<std::vector<uint32_t>> nb(ncap);
    std::vector<char> nt(ncap, 0);
    for (size_t j = 0; j < ocap; j++) {
        const auto &bin = bins_[j];
        for (uint32_t e : bin) nb[entries_[e].hash & (ncap - 1)].push_back(e);  // lo/hi split keeps relative order
        if (!is_tree_[j]) continue;
        // TreeNode.split: halves of <= 6 nodes become plain lists again; the others stay trees, rebuilt (treeify: the
        // root moves to the front) only when the bin really split
        auto &lo = nb[j], &hi = nb[j + ocap];
        const bool both = !lo.empty() && !hi.empty();
        for (auto *half : {&lo, &hi}) {
            if (half->empty()) continue;
            const size_t at = half == &lo ? j : j + ocap;
            if (half->size() <= 6) tree_.forget(*half);
            else { nt[at] = 1; if (both) tree_.treeify(*half); }
        }
    }
    cap_ = ncap;
    bins_.swap(nb);
    is_tree_.swap(nt);
}

int JavaHashMap::get(const std::string &key) const
{
    auto it = index_.find(key);
    if (it == index_.end()) throw Error("JavaHashMap::get: missing key " + key);
    return entries_[it->second].value;
}

bool JavaHashMap::find(const std::string &key, int *value) const
{
    auto it = index_.find(key);
    if (it == index_.end()) return false;
    *value = entries_[it->second].value;
    return true;
}

void JavaHashMap::remove(const std::string &key, bool movable)
{   // (movable: HashMap.remove(key) passes true, an iterator's remove -- retainAll -- false)
    auto it = index_.find(key);
    if (it == index_.end()) return;
    const size_t b = entries_[it->second].hash & (cap_ - 1);
    auto &bin = bins_[b];
    if (is_tree_[b]) {  // TreeNode.removeTreeNode
        if (tree_.remove(bin, it->second, movable)) { tree_.forget(bin); is_tree_[b] = 0; }
    } else {
        bin.erase(std::find(bin.begin(), bin.end(), it->second));
    }
    index_.erase(it);
    size_--;
}

// ---- JavaKmerMap

JavaKmerMap::JavaKmerMap(int k) : k_(k), head_(16, NIL), tail_(16, NIL), tree_([this](uint32_t x, uint32_t p) { return tree_dir(x, p); }) {}

int JavaKmerMap::tree_dir(uint32_t x, uint32_t p) const
{   // TreeNode order: the (signed) spread hash, then String.compareTo on the characters the packed keys stand for
    const int32_t h = (int32_t)entries_[x].hash, ph = (int32_t)entries_[p].hash;
    if (ph > h) return -1;
    if (ph < h) return 1;
    return unpack_kmer128(entries_[x].key, k_) < unpack_kmer128(entries_[p].key, k_) ? -1 : 1;
}

void JavaKmerMap::relink(size_t b, const std::vector<uint32_t> &chain)
{
    head_[b] = chain.empty() ? NIL : chain.front();
    tail_[b] = chain.empty() ? NIL : chain.back();
    for (size_t i = 0; i < chain.size(); i++) entries_[chain[i]].next = i + 1 < chain.size() ? chain[i + 1] : NIL;
}

uint32_t JavaKmerMap::hash_of(kmer_t key) const
{
    uint32_t h = 0;  // String.hashCode() of the k characters, then HashMap.hash()'s spread
    for (int i = k_ - 1; i >= 0; i--) h = 31u * h + (uint32_t)(unsigned char)"AGCT"[(unsigned)(key >> (2 * i)) & 3u];
    return h ^ (h >> 16);
}

int JavaKmerMap::find_entry(kmer_t key) const
{
    const uint32_t h = hash_of(key);
    for (uint32_t e = head_[h & (cap_ - 1)]; e != NIL; e = entries_[e].next)
        if (entries_[e].key == key) return (int)e;
    return -1;
}

int JavaKmerMap::put(kmer_t key, int value)
{
    const uint32_t h = hash_of(key);
    const size_t b = h & (cap_ - 1);
    size_t len = 0;
    for (uint32_t e = head_[b]; e != NIL; e = entries_[e].next, len++)
        if (entries_[e].key == key) {
            entries_[e].value = value;
            return (int)e;
        }
    const uint32_t e = (uint32_t)entries_.size();
    entries_.push_back(Entry{key, value, h, NIL});
    auto tb = tree_bins_.find(b);
    if (tb != tree_bins_.end()) {  // a treeified bin: putTreeVal decides where the node goes
        tree_.put(tb->second, e);
        relink(b, tb->second);
    } else {
        if (tail_[b] == NIL) head_[b] = e; else entries_[tail_[b]].next = e;
        tail_[b] = e;
        if (len + 1 >= 9) {  // a 9th node: treeifyBin (or a resize while the table is smaller than 64)
            if (cap_ >= 64) {
                std::vector<uint32_t> chain;
                for (uint32_t x = head_[b]; x != NIL; x = entries_[x].next) chain.push_back(x);
                tree_.treeify(chain);
                relink(b, chain);
                tree_bins_.emplace(b, std::move(chain));
                n_treeified_++;
            } else {
                resize();
            }
        }
    }
    size_++;
    if ((double)size_ > 0.75 * (double)cap_) resize();
    return (int)e;
}

void JavaKmerMap::resize()
{
    const size_t ncap = cap_ * 2;
    std::vector<uint32_t> nh(ncap, NIL), nt(ncap, NIL);
    for (uint32_t h : head_)
        for (uint32_t e = h, nx; e != NIL; e = nx) {  // lo/hi split keeps relative order
            nx = entries_[e].next;
            const size_t b = entries_[e].hash & (ncap - 1);
            entries_[e].next = NIL;
            if (nt[b] == NIL) nh[b] = e; else entries_[nt[b]].next = e;
            nt[b] = e;
        }
    const size_t ocap = cap_;
    cap_ = ncap;
    head_.swap(nh);
    tail_.swap(nt);
    // TreeNode.split for the bins that were trees: halves of <= 6 nodes are plain lists again (in chain order, as linked
    // above); the others stay trees, rebuilt (the root moves to the front) only when the bin really split
    std::unordered_map<size_t, std::vector<uint32_t>> old;
    old.swap(tree_bins_);
    for (auto &kv : old) {
        std::vector<uint32_t> lo, hi;
        for (uint32_t e : kv.second) ((entries_[e].hash & ocap) ? hi : lo).push_back(e);
        const bool both = !lo.empty() && !hi.empty();
        for (int side = 0; side < 2; side++) {
            std::vector<uint32_t> &half = side ? hi : lo;
            if (half.empty()) continue;
            const size_t at = kv.first + (side ? ocap : 0);
            if (half.size() <= 6) { tree_.forget(half); continue; }
            if (both) { tree_.treeify(half); relink(at, half); }
            tree_bins_.emplace(at, std::move(half));
        }
    }
}

void JavaKmerMap::remove(kmer_t key, bool movable)
{   // (movable: HashMap.remove(key) passes true, an iterator's remove -- runTrimPaths' retainAll -- false)
    const size_t b = hash_of(key) & (cap_ - 1);
    auto tb = tree_bins_.find(b);
    if (tb != tree_bins_.end()) {  // TreeNode.removeTreeNode
        std::vector<uint32_t> &chain = tb->second;
        for (size_t i = 0; i < chain.size(); i++)
            if (entries_[chain[i]].key == key) {
                const bool plain = tree_.remove(chain, chain[i], movable);
                relink(b, chain);
                if (plain) { tree_.forget(chain); tree_bins_.erase(tb); }
                size_--;
                return;
            }
        return;
    }
    uint32_t prev = NIL;
    for (uint32_t e = head_[b]; e != NIL; prev = e, e = entries_[e].next)
        if (entries_[e].key == key) {
            if (prev == NIL) head_[b] = entries_[e].next; else entries_[prev].next = entries_[e].next;
            if (tail_[b] == e) tail_[b] = prev;
            size_--;
            return;
        }
}

// ------------------------------------------------------------------------------------------ number formats

std::string java_format_2f(double x)
{
    if (x != x) return "NaN";
    if (std::isinf(x)) return x > 0 ? "Infinity" : "-Infinity";
    // the shortest decimal that reads back as x (Double.toString's digits), then HALF_UP to two places
    char buf[64];
    for (int prec = 1; prec <= 17; prec++) {
        snprintf(buf, sizeof buf, "%.*e", prec - 1, x < 0 ? -x : x);
        if (strtod(buf, nullptr) == (x < 0 ? -x : x)) break;
    }
    std::string m = buf;  // d.ddddde[+-]XX
    const size_t e = m.find('e');
    const int exp10 = atoi(m.c_str() + e + 1);
    std::string digits;
    for (size_t i = 0; i < e; i++)
        if (m[i] != '.') digits.push_back(m[i]);
    // value = 0.digits x 10^(exp10 + 1): integer part and two decimals, the third decides
    const int point = exp10 + 1;  // digits before the decimal point
    std::string ip, fp;
    if (point <= 0) { ip = "0"; fp = std::string((size_t)-point, '0') + digits; }
    else if ((size_t)point >= digits.size()) { ip = digits + std::string((size_t)point - digits.size(), '0'); }
    else { ip = digits.substr(0, (size_t)point); fp = digits.substr((size_t)point); }
    while (fp.size() < 3) fp.push_back('0');
    std::string out = ip + fp.substr(0, 2);
    if (fp[2] >= '5') {
        int i = (int)out.size() - 1;
        while (i >= 0 && out[(size_t)i] == '9') out[(size_t)i--] = '0';
        if (i >= 0) out[(size_t)i]++; else out.insert(out.begin(), '1');
    }
    std::string body = out.substr(0, out.size() - 2) + "." + out.substr(out.size() - 2);
    return std::signbit(x) ? "-" + body : body;
}

std::string java_double_to_string(double x)
{
    if (x != x) return "NaN";
    if (std::isinf(x)) return x > 0 ? "Infinity" : "-Infinity";
    const std::string sign = std::signbit(x) ? "-" : "";
    if (x == 0) return sign + "0.0";
    const double a = x < 0 ? -x : x;
    // the shortest decimal that reads back as x, as in java_format_2f
    char buf[64];
    for (int prec = 1; prec <= 17; prec++) {
        snprintf(buf, sizeof buf, "%.*e", prec - 1, a);
        if (strtod(buf, nullptr) == a) break;
    }
    const std::string m = buf;  // d.ddddde[+-]XX
    const size_t e = m.find('e');
    const int exp10 = atoi(m.c_str() + e + 1);  // value = d.ddd x 10^exp10
    std::string digits;
    for (size_t i = 0; i < e; i++)
        if (m[i] != '.') digits.push_back(m[i]);
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    if (a >= 1e-3 && a < 1e7) {  // plain notation, at least one digit on either side of the point
        const int point = exp10 + 1;  // digits before the point
        if (point <= 0) return sign + "0." + std::string((size_t)-point, '0') + digits;
        if ((size_t)point >= digits.size()) return sign + digits + std::string((size_t)point - digits.size(), '0') + ".0";
        return sign + digits.substr(0, (size_t)point) + "." + digits.substr((size_t)point);
    }
    return sign + digits.substr(0, 1) + "." + (digits.size() > 1 ? digits.substr(1) : "0") + "E" + std::to_string(exp10);
}

std::string java_format_6_2f(float x)
{
    std::string body;
    if (x != x) {
        body = "NaN";
    } else if (x == std::numeric_limits<float>::infinity() || x == -std::numeric_limits<float>::infinity()) {
        body = x > 0 ? "Infinity" : "-Infinity";
    } else {
        // the exact decimal value of the float, rounded HALF_UP to two places
        char buf[512];
        snprintf(buf, sizeof buf, "%.160f", (double)(x < 0 ? -x : x));
        std::string d = buf;
        const size_t dot = d.find('.');
        std::string ip = d.substr(0, dot), fp = d.substr(dot + 1);
        bool up = fp[2] >= '5';
        std::string digits = ip + fp.substr(0, 2);
        if (up) {
            int i = (int)digits.size() - 1;
            while (i >= 0 && digits[(size_t)i] == '9') digits[(size_t)i--] = '0';
            if (i >= 0) digits[(size_t)i]++; else digits.insert(digits.begin(), '1');
        }
        body = digits.substr(0, digits.size() - 2) + "." + digits.substr(digits.size() - 2);
        if (std::signbit(x)) body = "-" + body;  // (Java prints -0.00 for negative values that round to zero)
    }
    if (body.size() < 6) body.insert(0, 6 - body.size(), ' ');
    return body;
}

}  // namespace mch
