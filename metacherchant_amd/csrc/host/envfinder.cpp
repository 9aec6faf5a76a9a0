// See envfinder.h.  Every function restates the reference lines cited there.
#include "envfinder.h"

#include <sys/stat.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <cmath>
#include <functional>
#include <limits>
#include <set>

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

static bool read_lines(const std::string &path, std::vector<std::string> *lines)
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

// ------------------------------------------------------------------------------------------ Environment

// ---- packed k-mers

kmer_t pack_kmer128(const std::string &s)
{
    uint64_t hi, lo;
    pack_kmer(s, &hi, &lo);
    return ((kmer_t)hi << 64) | lo;
}

static inline uint64_t reverse_pairs64(uint64_t x)
{
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x);
}

kmer_t reverse_complement128(kmer_t v, int k)
{
    // complement is 3 - code (A0<->T3, G1<->C2); then the 2-bit groups in reverse order
    const kmer_t c = ~v;
    const kmer_t r = ((kmer_t)reverse_pairs64((uint64_t)c) << 64) | reverse_pairs64((uint64_t)(c >> 64));
    return r >> (128 - 2 * k);
}

// ASCII order is A < C < G < T, the codes are A0 G1 C2 T3: swapping the two bits of every code gives ranks
// whose numeric order is String.compareTo's
static inline kmer_t ascii_rank(kmer_t v)
{
    const kmer_t m = ((kmer_t)0x5555555555555555ull << 64) | 0x5555555555555555ull;
    return ((v & m) << 1) | ((v >> 1) & m);
}

kmer_t normalize128(kmer_t v, int k)
{
    const kmer_t rc = reverse_complement128(v, k);
    return ascii_rank(v) < ascii_rank(rc) ? v : rc;
}

static inline kmer_t kmer_mask(int bases) { return bases >= 64 ? ~(kmer_t)0 : (((kmer_t)1 << (2 * bases)) - 1); }

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

// ---- Environment

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

// doMerge over the nodes listed (ascending), pass after pass until nothing merges
void merge_loop(std::vector<PictureNode> &nodes, int k, const std::vector<uint8_t> &cls, const std::vector<uint32_t> &scan)
{
    for (;;) {
        bool acted = false;
        for (const uint32_t i : scan) {
            if (!nodes[i].deleted && nodes[i].neighbors.size() == 1) {
                const int other = nodes[i].neighbors[0];
                if (nodes[(size_t)other].neighbors.size() != 1 || cls[i / 2] != cls[(size_t)other / 2]) continue;
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
        uint64_t h = (uint64_t)key ^ ((uint64_t)(key >> 64) * 0x9E3779B97F4A7C15ull);
        h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull; h ^= h >> 33;
        size_t i = (size_t)h & (cap - 1);
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
    std::vector<uint32_t> scan;
    if (!compact) {
        for (size_t i = 0; i < N; i++) nodes[i].sequence = unpack_kmer128(packed[i], k);
        for_each_neighbour(k, packed, [&](size_t p, int j) { nodes[p].neighbors.push_back(j); });
        scan.resize(N);
        for (size_t i = 0; i < N; i++) scan[i] = (uint32_t)i;
        merge_loop(nodes, k, cls, scan);  // doMerge
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
    merge_loop(nodes, k, cls, scan);
    return nodes;
}

void Environment::create_picture(const Compactor *compact)
{
    std::vector<kmer_t> kmers;
    std::vector<uint8_t> cls, gene;
    kmers.reserve(subgraph_.size());
    subgraph_.for_each([&](kmer_t seq, int, int) {
        const kmer_t rc = reverse_complement128(seq, k_);
        const bool g = std::binary_search(gene_kmers_.begin(), gene_kmers_.end(), seq) ||
                       std::binary_search(gene_kmers_.begin(), gene_kmers_.end(), rc);
        const Colour col = coloured_ ? colours_[kmers.size()] : NO_COLOUR;
        kmers.push_back(seq);
        gene.push_back(g);
        cls.push_back((uint8_t)(2 * (col + 1) + (g ? 1 : 0)));  // (doMerge: nodes of one colour and one is_gene; uncoloured nodes all have NO_COLOUR)
    });
    std::vector<PictureNode> made = make_picture(k_, kmers, cls, compact);
    nodes_.clear();
    nodes_.reserve(made.size());
    for (size_t i = 0; i < made.size(); i++) {
        PictureNode &m = made[i];
        nodes_.push_back(Node{std::move(m.sequence), (int)i, gene[i / 2] != 0, m.deleted, m.rc, std::move(m.neighbors),
                              coloured_ ? colours_[i / 2] : NO_COLOUR});
    }
}

std::string Environment::node_id(const Node &n) const
{
    return std::to_string(std::min(nodes_[(size_t)n.rc].id, n.id) + 1) + (n.is_gene ? "_start" : "");
}

std::string Environment::seqs_fasta(int chunk_length) const
{
    std::string out;
    for (const Node &n : nodes_) {
        const Node &rc = nodes_[(size_t)n.rc];
        if (n.deleted || !(n.id < rc.id) || (int)n.sequence.size() < chunk_length) continue;
        std::set<int> ids;
        for (int j : n.neighbors) ids.insert(std::min(nodes_[(size_t)j].id, nodes_[(size_t)nodes_[(size_t)j].rc].id) + 1);
        for (int j : rc.neighbors) ids.insert(std::min(nodes_[(size_t)j].id, nodes_[(size_t)nodes_[(size_t)j].rc].id) + 1);
        ids.erase(std::min(n.id, rc.id) + 1);
        out += "> Id" + node_id(n) + " Length:" + std::to_string(n.sequence.size()) + " Neighbors:[";
        bool first = true;
        for (int x : ids) {
            if (!first) out += ", ";
            out += std::to_string(x);
            first = false;
        }
        out += "]\n" + n.sequence + "\n";
    }
    return out;
}

std::string Environment::graph_gfa() const
{
    std::string out;
    for (const Node &n : nodes_) {
        if (n.deleted || n.sequence.compare(nodes_[(size_t)n.rc].sequence) > 0) continue;
        long long coverage = 0;
        const std::string &s = n.sequence;
        kmer_t fw = 0, rc = 0;  // the window and its reverse complement, rolled along the label
        int last = 0;
        for (size_t i = 0; i < s.size(); i++) {
            const unsigned code = (unsigned)code_of(s[i]);
            fw = ((fw << 2) | code) & kmer_mask(k_);
            rc = (rc >> 2) | ((kmer_t)(3u - code) << (2 * (k_ - 1)));
            if (i + 1 < (size_t)k_) continue;
            const int e = subgraph_.find_entry(ascii_rank(fw) < ascii_rank(rc) ? fw : rc);
            if (e < 0) throw Error("graph_gfa: k-mer of a node label is not in the subgraph: " + s.substr(i + 1 - (size_t)k_, (size_t)k_));
            last = subgraph_.value_at(e);
            coverage += last;
        }
        coverage += (long long)last * (k_ - 1);
        out += "S\t" + node_id(n) + "\t" + s + "\tLN:i:" + std::to_string(s.size()) + "\tKC:i:" + std::to_string(coverage) +
               (coloured_ ? std::string("\tCL:Z:") + colour_name(n.colour) : std::string(n.is_gene ? "\tCL:Z:GREEN" : "")) + "\n";
    }
    for (const Node &i : nodes_) {
        if (i.deleted) continue;
        for (int jx : i.neighbors) {
            const Node &j = nodes_[(size_t)jx];
            if (j.deleted) continue;
            out += "L\t" + node_id(i) + "\t" + (i.sequence.compare(nodes_[(size_t)i.rc].sequence) >= 0 ? "+" : "-") + "\t" +
                   node_id(j) + "\t" + (j.sequence.compare(nodes_[(size_t)j.rc].sequence) <= 0 ? "+" : "-") + "\t" +
                   std::to_string(k_ - 1) + "M\n";
        }
    }
    return out;
}

std::string Environment::tsv_nodes() const
{
    std::string out = "id\tlength\tseq\n";
    for (size_t i = 0; i < nodes_.size(); i++) {
        const Node &n = nodes_[i];
        if (n.deleted || n.sequence.compare(nodes_[(size_t)n.rc].sequence) > 0) continue;
        out += std::to_string(i + 1) + "\t" + std::to_string(n.sequence.size()) + "\t" + n.sequence + "\n";
    }
    return out;
}

std::string Environment::tsv_edges() const
{
    auto nid = [&](const Node &n) {
        const Node &rc = nodes_[(size_t)n.rc];
        return (n.sequence.compare(rc.sequence) <= 0 ? std::to_string(n.id + 1) : "-" + std::to_string(rc.id + 1)) +
               (n.is_gene ? "_start" : "");
    };
    std::string out = "source\ttarget\n";
    for (const Node &i : nodes_) {
        if (i.deleted) continue;
        for (int jx : i.neighbors) {
            const Node &j = nodes_[(size_t)jx];
            if (j.deleted) continue;
            out += nid(nodes_[(size_t)i.rc]) + "\t" + nid(j) + "\tpp\n";
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

// ------------------------------------------------------------------------------------------ environment-finder-multi

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

namespace {
// DeBruijnGraphUtils.loadGraph (:13-27)
JavaHashMap load_graph(const std::string &path)
{
    std::vector<std::string> lines;
    if (!read_lines(path, &lines)) throw Error("Couldn't load graph from file " + path);
    JavaHashMap g;
    for (const std::string &line : lines) {
        if (line.empty()) continue;
        const size_t sp = line.find(' ');
        if (sp == std::string::npos || sp + 1 >= line.size()) throw Error("Couldn't load graph from file " + path + ": bad line '" + line + "'");
        size_t end = line.find(' ', sp + 1);
        const std::string num = line.substr(sp + 1, end == std::string::npos ? std::string::npos : end - sp - 1);
        char *stop = nullptr;
        const long v = strtol(num.c_str(), &stop, 10);
        if (num.empty() || *stop) throw Error("Couldn't load graph from file " + path + ": bad depth '" + num + "'");
        g.put(line.substr(0, sp), (int)v);
    }
    return g;
}

struct MultiNode {  // src/algo/MultiNode.java:9-29 (rc and neighbours as indices into the node array)
    std::string sequence;
    int id;
    bool is_gene, deleted = false;
    int rc;
    std::vector<int> neighbors;
    std::set<int> graphs;
};
}  // namespace

MultiResult environment_finder_multi(const std::vector<std::string> &env_paths, const std::string &seq_path, int gene_id)
{
    MultiResult R;
    std::vector<JavaHashMap> graphs;
    for (const std::string &p : env_paths) graphs.push_back(load_graph(p));
    if (graphs.empty()) throw Error("Zero environments given");
    if (graphs.size() > 256) R.log.push_back("WARN Found more than 256 environments. Grayscale graph may be not accurate.");
    int k = -1;
    graphs[0].for_each([&](const std::string &kmer, int) { if (k < 0) k = (int)kmer.size(); });
    if (k < 0) throw Error("The first environment is empty");  // (the reference fails with NoSuchElementException)
    for (const JavaHashMap &g : graphs)
        g.for_each([&](const std::string &kmer, int) {
            if ((int)kmer.size() != k)
                throw Error("K-mers of different lengths encountered: " + std::to_string(k) + " and " + std::to_string(kmer.size()));
        });
    SeedFile sf;
    try {
        sf = read_seed_fasta(seq_path);
    } catch (const Error &) {
        throw Error("Could not load sequence file");
    }
    if (gene_id < 1 || (size_t)gene_id > sf.dnas.size() || (size_t)gene_id > sf.comments.size())
        throw Error("--geneid " + std::to_string(gene_id) + " is outside the sequences of " + seq_path);
    const std::string sequence = sf.dnas[(size_t)gene_id - 1], comment = sf.comments[(size_t)gene_id - 1];
    R.log.push_back("INFO Combining environments for sequence " +
                    ((int)sequence.size() >= 2 * k ? sequence.substr(0, (size_t)k) + "..." + sequence.substr(sequence.size() - (size_t)k) +
                                                         " (length=" + std::to_string(sequence.size()) + ")"
                                                   : sequence));

    // initializeStructures (MultiSequenceCalculator.java:51-100)
    JavaHashMap by_kmer;  // value: node index, -1 = null
    for (const JavaHashMap &g : graphs)
        g.for_each([&](const std::string &kmer, int) {
            by_kmer.put(kmer, -1);
            by_kmer.put(reverse_complement(kmer), -1);
        });
    const size_t size = by_kmer.size();
    std::vector<MultiNode> nodes;
    nodes.reserve(size);
    {
        std::vector<std::string> order;
        by_kmer.for_each([&](const std::string &kmer, int) { order.push_back(kmer); });
        for (const std::string &kmer : order) {
            const std::string rc = reverse_complement(kmer);
            if (kmer.compare(rc) > 0) continue;
            if (nodes.size() + 2 > size)
                throw Error("palindromic k-mer " + kmer + ": the reference fails here (ArrayIndexOutOfBoundsException)");
            const bool is_gene = sequence.find(kmer) != std::string::npos || sequence.find(rc) != std::string::npos;
            const int a = (int)nodes.size();
            MultiNode na, nb;
            na.sequence = kmer; na.id = a; na.is_gene = is_gene; na.rc = a + 1;
            nb.sequence = rc; nb.id = a + 1; nb.is_gene = is_gene; nb.rc = a;
            nodes.push_back(na);
            nodes.push_back(nb);
            by_kmer.put(kmer, a);
            by_kmer.put(rc, a + 1);
        }
    }
    for (size_t i = 0; i < graphs.size(); i++)
        graphs[i].for_each([&](const std::string &kmer, int) {
            const int n = by_kmer.get(kmer);
            nodes[(size_t)n].graphs.insert((int)i);
            nodes[(size_t)nodes[(size_t)n].rc].graphs.insert((int)i);
        });
    for (size_t i = 0; i < nodes.size(); i++)
        for (const char c : {'A', 'G', 'C', 'T'}) {
            int nb;
            if (by_kmer.find(nodes[i].sequence.substr(1) + c, &nb) && nb >= 0) nodes[(size_t)nodes[i].rc].neighbors.push_back(nb);
        }

    // doMerge (:102-139)
    auto merge_labels = [&](const std::string &a, const std::string &b) {
        if (a.substr(a.size() - (size_t)(k - 1)) != b.substr(0, (size_t)(k - 1)))
            throw Error("Labels should be merged, but can not: " + a + " and " + b);
        return a + b.substr((size_t)(k - 1));
    };
    for (;;) {
        bool acted = false;
        for (size_t i = 0; i < nodes.size(); i++) {
            if (nodes[i].deleted || nodes[i].neighbors.size() != 1) continue;
            const size_t o = (size_t)nodes[i].neighbors[0];
            if (nodes[o].neighbors.size() != 1 || nodes[i].is_gene != nodes[o].is_gene || nodes[i].graphs != nodes[o].graphs) continue;
            const size_t first_minus = (size_t)nodes[i].rc, second_plus = (size_t)nodes[o].rc;
            const std::string new_seq = merge_labels(nodes[second_plus].sequence, nodes[i].sequence);
            const std::string new_rc = merge_labels(nodes[first_minus].sequence, nodes[o].sequence);
            nodes[second_plus].sequence = new_seq;
            nodes[first_minus].sequence = new_rc;
            nodes[second_plus].rc = (int)first_minus;
            nodes[first_minus].rc = (int)second_plus;
            nodes[i].deleted = nodes[o].deleted = true;
            acted = true;
        }
        if (!acted) break;
    }
    auto min_id = [&](const MultiNode &n) { return std::min(n.id, nodes[(size_t)n.rc].id) + 1; };
    auto label = [&](const MultiNode &n) { return std::to_string(min_id(n)) + (n.is_gene ? "_start" : ""); };

    // outputNodeSequences (:141-160)
    for (const MultiNode &n : nodes) {
        const MultiNode &rc = nodes[(size_t)n.rc];
        if (n.deleted || !(n.id < rc.id)) continue;
        std::set<int> ids;
        for (int j : n.neighbors) ids.insert(min_id(nodes[(size_t)j]));
        for (int j : rc.neighbors) ids.insert(min_id(nodes[(size_t)j]));
        ids.erase(min_id(n));
        R.seqs_fasta += "> Id" + label(n) + " Length:" + std::to_string(n.sequence.size()) + " Neighbors:[";
        bool first = true;
        for (int x : ids) {
            if (!first) R.seqs_fasta += ", ";
            R.seqs_fasta += std::to_string(x);
            first = false;
        }
        R.seqs_fasta += "]\n" + n.sequence + "\n";
    }

    // GFAWriterMulti (:37-146)
    const size_t G = graphs.size();
    auto color = [&](const MultiNode &n) -> std::string {
        if (n.is_gene) return "#00ff00";
        const size_t s = n.graphs.size();
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
    for (const MultiNode &n : nodes) {
        if (n.deleted || !(n.id < nodes[(size_t)n.rc].id)) continue;
        long long coverage = 0;
        for (const JavaHashMap &g : graphs)
            for (size_t i = 0; i + (size_t)k <= n.sequence.size(); i++) {
                int c;
                if (g.find(normalize_dna(n.sequence.substr(i, (size_t)k)), &c)) coverage += c;
            }
        const std::string col = color(n);
        R.graph_gfa += "S\t" + label(n) + "\t" + n.sequence + "\tLN:i:" + std::to_string(n.sequence.size()) + "\tKC:i:" +
                       std::to_string(coverage) + "\tCL:Z:" + col + "\tC2:Z:" + col + "\n";
    }
    for (const MultiNode &a : nodes) {
        if (a.deleted) continue;
        for (int j : a.neighbors) {
            const MultiNode &b = nodes[(size_t)j];
            R.graph_gfa += "L\t" + label(a) + "\t" + (a.id < nodes[(size_t)a.rc].id ? "+" : "-") + "\t" + label(b) + "\t" +
                           (b.id > nodes[(size_t)b.rc].id ? "+" : "-") + "\t" + std::to_string(k - 1) + "M\n";
        }
    }
    R.gene_fasta = ">" + comment + "\n" + sequence + "\n";

    // printProbability (EnvironmentFinderMultiMain.java:104-170): 32-bit sums (wrapping like Java's int), float division
    R.jacard_sym = "The[31mWarning! symmetric <<Jaccard distance>> (1 - AB/AUB):\n\n";
    R.jacard_alt = "The[31mWarning! alternative <<Jaccard distance>> (1 - AB/A):\n\n";
    for (size_t i = 0; i < G; i++) {
        R.jacard_sym += env_paths[i];
        R.jacard_alt += env_paths[i];
        for (size_t j = 0; j < G; j++) {
            uint32_t diff = 0, diff_alt = 0, uni = 0;  // (unsigned: wraps like Java's int without undefined behaviour)
            graphs[i].for_each([&](const std::string &kmer, int v) {
                int w;
                if (!graphs[j].find(kmer, &w)) { diff += (uint32_t)v; diff_alt += (uint32_t)v; uni += (uint32_t)v; }
                else { diff += (uint32_t)std::abs(v - w); diff_alt += (uint32_t)std::abs(v - w); uni += (uint32_t)std::max(v, w); }
            });
            graphs[j].for_each([&](const std::string &kmer, int v) {
                int w;
                if (!graphs[i].find(kmer, &w)) { diff += (uint32_t)v; uni += (uint32_t)v; }
            });
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

// ---- the packed path

namespace {
struct KmerHash {
    size_t operator()(kmer_t key) const
    {
        uint64_t h = (uint64_t)key ^ ((uint64_t)(key >> 64) * 0x9E3779B97F4A7C15ull);
        h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull; h ^= h >> 33;
        return (size_t)h;
    }
};

// |v - w| as int arithmetic gives it (wrapping where Java's would), as an unsigned word
inline uint32_t abs_diff_u32(int32_t v, int32_t w)
{
    const int32_t d = (int32_t)((uint32_t)v - (uint32_t)w);
    return d < 0 ? 0u - (uint32_t)d : (uint32_t)d;
}
}  // namespace

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

// DeBruijnGraphUtils.loadGraph (:13-27) with the key packed; lengths: every key's length as it comes
PackedGraphFile load_graph_packed(const std::string &path, std::vector<size_t> *lengths)
{
    std::vector<std::string> lines;
    if (!read_lines(path, &lines)) throw Error("Couldn't load graph from file " + path);
    PackedGraphFile g;
    for (const std::string &line : lines) {
        if (line.empty()) continue;
        const size_t sp = line.find(' ');
        if (sp == std::string::npos || sp + 1 >= line.size()) throw Error("Couldn't load graph from file " + path + ": bad line '" + line + "'");
        size_t end = line.find(' ', sp + 1);
        const std::string num = line.substr(sp + 1, end == std::string::npos ? std::string::npos : end - sp - 1);
        char *stop = nullptr;
        const long v = strtol(num.c_str(), &stop, 10);
        if (num.empty() || *stop) throw Error("Couldn't load graph from file " + path + ": bad depth '" + num + "'");
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
        g.depths.push_back((int)v);
        lengths->push_back(sp);
    }
    return g;
}
}  // namespace

MultiResult environment_finder_multi_packed(const std::vector<std::string> &env_paths, const std::string &seq_path, int gene_id, const Joiner &join,
                                            const Compactor &compact, size_t *n_entries)
{
    MultiResult R;
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
        int k0 = -1;
        graphs[0].for_each([&](const std::string &kmer, int) { if (k0 < 0) k0 = (int)kmer.size(); });
        for (const JavaHashMap &g : graphs)
            g.for_each([&](const std::string &kmer, int) {
                if ((int)kmer.size() != k0)
                    throw Error("K-mers of different lengths encountered: " + std::to_string(k0) + " and " + std::to_string(kmer.size()));
            });
    }
    const int k = (int)lengths[0];
    const size_t G = files.size();
    std::vector<JavaKmerMap> graphs;  // the last line of a k-mer wins; the iteration order is the HashMap's
    for (const PackedGraphFile &f : files) {
        graphs.emplace_back(k);
        for (size_t i = 0; i < f.kmers.size(); i++) graphs.back().put(f.kmers[i], f.depths[i]);
    }
    files.clear();
    SeedFile sf;
    try {
        sf = read_seed_fasta(seq_path);
    } catch (const Error &) {
        throw Error("Could not load sequence file");
    }
    if (gene_id < 1 || (size_t)gene_id > sf.dnas.size() || (size_t)gene_id > sf.comments.size())
        throw Error("--geneid " + std::to_string(gene_id) + " is outside the sequences of " + seq_path);
    const std::string sequence = sf.dnas[(size_t)gene_id - 1], comment = sf.comments[(size_t)gene_id - 1];
    R.log.push_back("INFO Combining environments for sequence " +
                    ((int)sequence.size() >= 2 * k ? sequence.substr(0, (size_t)k) + "..." + sequence.substr(sequence.size() - (size_t)k) +
                                                         " (length=" + std::to_string(sequence.size()) + ")"
                                                   : sequence));

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
    in.gene_len = sequence.size();  // (upper-case ACGT: read_seed_fasta makes it so)
    in.gene_words.assign((sequence.size() + 31) / 32, 0);
    for (size_t i = 0; i < sequence.size(); i++) in.gene_words[i >> 5] |= (uint64_t)code_of(sequence[i]) << (62 - 2 * (i & 31));
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
    std::vector<PictureNode> nodes = make_picture(k, in.entries, cls, &keep_irregular);
    const size_t N = nodes.size();
    auto node_kmer = [&](size_t i) { return (i & 1) ? reverse_complement128(in.entries[i / 2], k) : in.entries[i / 2]; };
    // the reference lists a node's neighbours in the order of their last base, A G C T: the codes' order
    for (PictureNode &nd : nodes)
        std::sort(nd.neighbors.begin(), nd.neighbors.end(),
                  [&](int a, int b) { return ((unsigned)node_kmer((size_t)a) & 3u) < ((unsigned)node_kmer((size_t)b) & 3u); });
    auto min_id = [&](size_t i) { return (int)std::min(i, (size_t)nodes[i].rc) + 1; };
    auto label = [&](size_t i) { return std::to_string(min_id(i)) + (J.is_gene[i / 2] ? "_start" : ""); };

    // outputNodeSequences (:141-160)
    for (size_t i = 0; i < N; i++) {
        const PictureNode &nd = nodes[i];
        if (nd.deleted || !((int)i < nd.rc)) continue;
        std::set<int> ids;
        for (int j : nd.neighbors) ids.insert(min_id((size_t)j));
        for (int j : nodes[(size_t)nd.rc].neighbors) ids.insert(min_id((size_t)j));
        ids.erase(min_id(i));
        R.seqs_fasta += "> Id" + label(i) + " Length:" + std::to_string(nd.sequence.size()) + " Neighbors:[";
        bool first = true;
        for (int x : ids) {
            if (!first) R.seqs_fasta += ", ";
            R.seqs_fasta += std::to_string(x);
            first = false;
        }
        R.seqs_fasta += "]\n" + nd.sequence + "\n";
    }

    // GFAWriterMulti (:37-146)
    auto color = [&](size_t i) -> std::string {
        if (J.is_gene[i / 2]) return "#00ff00";
        const size_t s = (size_t)__builtin_popcountll(J.member[i / 2]);
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
        const std::string col = color(i);
        R.graph_gfa += "S\t" + label(i) + "\t" + nd.sequence + "\tLN:i:" + std::to_string(nd.sequence.size()) + "\tKC:i:" + std::to_string(coverage) +
                       "\tCL:Z:" + col + "\tC2:Z:" + col + "\n";
    }
    for (size_t a = 0; a < N; a++) {
        if (nodes[a].deleted) continue;
        for (int j : nodes[a].neighbors)
            R.graph_gfa += "L\t" + label(a) + "\t" + ((int)a < nodes[a].rc ? "+" : "-") + "\t" + label((size_t)j) + "\t" +
                           (j > nodes[(size_t)j].rc ? "+" : "-") + "\t" + std::to_string(k - 1) + "M\n";
    }
    R.gene_fasta = ">" + comment + "\n" + sequence + "\n";

    // printProbability (EnvironmentFinderMultiMain.java:104-170): 32-bit sums (wrapping like Java's int), float division
    R.jacard_sym = "The[31mWarning! symmetric <<Jaccard distance>> (1 - AB/AUB):\n\n";
    R.jacard_alt = "The[31mWarning! alternative <<Jaccard distance>> (1 - AB/A):\n\n";
    for (size_t i = 0; i < G; i++) {
        R.jacard_sym += env_paths[i];
        R.jacard_alt += env_paths[i];
        for (size_t j = 0; j < G; j++) {
            const uint32_t diff = J.diff[i * G + j], diff_alt = J.diff_alt[i * G + j], uni = J.uni[i * G + j];
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

void write_multi(const MultiResult &r, const std::string &output_dir)
{
    write_file(output_dir + "/seqs.fasta", r.seqs_fasta);
    write_file(output_dir + "/graph.gfa", r.graph_gfa);
    write_file(output_dir + "/gene.fasta", r.gene_fasta);
    write_file(output_dir + "/Jacard_sym.txt", r.jacard_sym);
    write_file(output_dir + "/Jacard_alt.txt", r.jacard_alt);
}

}  // namespace mch
