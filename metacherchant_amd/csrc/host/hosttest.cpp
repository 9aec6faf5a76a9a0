// mc_hosttest -- CPU-only driver of the host logic (no GPU, no libmcgpu): takes BFS passes from
// a dump file instead of mc_bfs_batch and writes the environment files, so that tests/ can compare
// the C++ host side with the Python restatement in oracle/host_oracle.py.
//
// dump format (text): k chunk_length trim n_genes / gene strings / n_passes / per pass: dir n /
// n lines "kmer dist cov last".  Also: `mc_hosttest seeds <fasta>` and `mc_hosttest reads <file>`
// print what the seed reader / read ingest deliver; `fmt` and `dtoa` print Java's number formats.
// `mc_hosttest colour <dump> <out_dir> <name>`: one sequence of the recipient-visualiser.  dump: k / the sequence / n / n lines
// "kmer dist cov mask" (its walk, in insertion order, with every k-mer's class mask) / m / m k-mers the graph holds beside them;
// writes <out_dir>/<name>_seqs.fasta and <name>.gfa and prints the "Extending endings" line.
// `mc_hosttest kmers <dump>`: the subgraph's keys of an `env` dump, one a line, as Environment::kmers lists them.
// `mc_hosttest cutreads <reads file> <keep> <out.fasta> <index>`: the reads whose character in <keep> (one '0' / '1' a read) is '1'
// through CutReadsWriter.
// `mc_hosttest unitigs <file>`: unitig compaction both ways.  file: k n / n lines "kmer class" (oriented k-mers in node order).  Prints
// the link analysis ("U first last_rc bases" a unitig, "I entry" an irregular entry), then the node state of the reference's loop
// ("O id deleted rc label neighbours") and of the link analysis with the loop over the irregular entries ("N ..."); a deleted node's
// label and rc print as "-" (they depend on the loop's scan order and are never read).
// `mc_hosttest multi-packed <out_dir> <seq> <gene_id> <env>...`: what `multi` writes and prints, through environment_finder_multi_packed with
// env_join_host and unitigs_by_links, and "ENTRIES <n>" behind the log lines.  An input the packed path cannot represent ends with
// "unpacked: <reason>" on stderr and status 3.
// `mc_hosttest dnaq <file>`: what DnaQReader delivers.  "fastq <0|1> offset <n>" (the quality offset it found; 0 for FASTA), then a line a
// read: "R <length>\t<bases, N as A>\t<phreds as chars from '!'>".  `mc_hosttest dnaq-range <file> <chunk>`: the same lines from the file
// cut at record starts every <chunk> bytes, each piece read by DnaQReader over a range of memory.  An error ends both with status 1 after
// the reads before it.
// `mc_hosttest cuts <file> [<chunk>]`: the chunks the device tokeniser's drivers read the file in (reads_io.h plain_chunks), a line "b e" a
// chunk, byte offsets in the file.  <chunk>: MC_TOKENIZER_CHUNK_BYTES as it would be spelt; left out: the switch's default.
// `mc_hosttest render-host <out_dir>`: what --render adds to the host's writers (csrc/host/fastq_out.h), on designed reads (read i has
// i % 7 + 1 bases, base j the code (i + j) % 4 and the phred (3 i + 5 j) % 63).  <out_dir>/a.fastq: reads 0 .. 4 through FastqOut::put, 5 .. 9
// as one block through put_rendered, 10 .. 11 through put again.  <out_dir>/b.fastq: reads 8 and 9 through put, then a SideList that took
// read 0 as a read, 1 .. 4 as a block of bodies, 5 as a read, 6 .. 7 as bodies.  Prints "a <records> b <records>", then render_ranges of
// two designed covers, a line "R a b seg0 seg1" a range, and "E <message>" for a cover that ends before the batch does.
// `mc_hosttest streams`: which output stream the classifiers give each read of a pair (csrc/host/classifier_streams.h), for every input.
// "P found1 found2 len1 len2 st1 st2 counter" for reads-classifier's paired rule (lengths 0 and 3), "S found1 len1 st1 st2 counter"
// for its single-end rule (called with a found flag and a length for the second side that it must ignore), "T class1 class2 len1 len2
// st1 st2" for the triple rule; a stream prints as its number, MC_RENDER_SKIP as 255, a counter as its PAIR_* number.
// `mc_hosttest placement <k>`: where the table puts a key (csrc/kmer_hash.h, the functions the kernels compile).  Reads hexadecimal
// 64-bit words from stdin, one a line, and prints for each "fmix64 sk_order sk_bin sk_hmin_of_kmer": the hash of the word as a key, the
// order and the bin of its low 32 bits, and the smallest order among the SK_M-mers of the word as a packed k-mer of k bases.
// `mc_hosttest placement <k> poly`, k from 15 to 63: the same for a polynomial key in minimizer bins (csrc/count_long.h).  Reads a k-mer a
// line as two hexadecimal words "hi lo" (2k bits right-aligned in 128, first base on top) and prints "key hmin bin word2 bin2 home": the
// polynomial key, then under the smallest-hash rule sk_hmin_of_kmer2 and skl_bin of it, under the two-smallest rule the word of the two
// smallest and skl_bin of it, and sk_home(key), the key's home slot inside its bin.
// `mc_hosttest pointers <pos>...`: the code of a read pointer (csrc/read_ptr.h, the functions the kernels compile).  For every store
// position (decimal) one line: ptr_encode(pos), ptr_decode of that code and its span (0 0 for no pointer), ptr_advance(code, j) for
// j = 0 .. 15 and ptr_advance_long(code, j) for j = 0 .. 31.
// `mc_hosttest dedup-tags <file>`: where the merge kernel's record table puts a super-k-mer record (csrc/kmer_hash.h dd_hash, the function
// the kernel compiles).  file: a record a line as two hexadecimal 64-bit words "lo hi" (csrc/count_pipeline.h has the layout).  Prints for
// each "hash tag place": dd_hash of the record's three words of bases, the tag (hash & 0xFFFF0000) | 0x8000 and the home place hash & 1023.
// `mc_hosttest long-tags <file>`: where k_p3_long's table of equal records puts a long record (csrc/kmer_hash.h skl_rec_hash, the function
// the kernel compiles).  file: a record a line as "windows X0 X1 X2", the window count in decimal and the three words of bases in
// hexadecimal (csrc/count_long.h has the layout).  Prints for each "hash tag slot": the hash, hash >> 16 and hash & 1023.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <map>

#include "../kmer_hash.h"
#include "../read_ptr.h"
#include "../switches.h"
#include "classifier_streams.h"
#include "envfinder.h"
#include "fastq_out.h"

using namespace mch;

int main(int argc, char **argv)
{
    try {
        if (argc == 3 && std::string(argv[1]) == "seeds") {
            const SeedFile s = read_seed_fasta(argv[2]);
            printf("%zu %zu\n", s.dnas.size(), s.comments.size());
            for (const auto &d : s.dnas) printf("D %s\n", d.c_str());
            for (const auto &c : s.comments) printf("C %s\n", c.c_str());
            return 0;
        }
        if (argc == 3 && std::string(argv[1]) == "reads") {
            const uint64_t n = load_reads_file(argv[2], 1000, [&](PackedBatch &b) {
                for (uint64_t r = 0; r < b.n_reads(); r++) {
                    std::string s;
                    for (uint64_t p = b.offsets[r]; p < b.offsets[r + 1]; p++)
                        s.push_back("AGCT"[(b.words[p >> 5] >> (62 - 2 * (p & 31))) & 3]);
                    printf("%s\n", s.c_str());
                }
            });
            fprintf(stderr, "%llu reads\n", (unsigned long long)n);
            return 0;
        }
        if (argc == 3 && std::string(argv[1]) == "fmt") {  // String.format("%6.2f", (float) x)
            fputs(java_format_6_2f(strtof(argv[2], nullptr)).c_str(), stdout);
            return 0;
        }
        if (argc == 3 && std::string(argv[1]) == "dtoa") {  // Double.toString of every double of the file (hex bit patterns, one a line)
            std::ifstream f(argv[2]);
            if (!f) throw Error("cannot open the file of doubles");
            std::string out;
            for (std::string line; std::getline(f, line);) {
                if (line.empty()) continue;
                const uint64_t bits = strtoull(line.c_str(), nullptr, 16);
                double x;
                memcpy(&x, &bits, 8);
                out += java_double_to_string(x);
                out.push_back('\n');
            }
            fwrite(out.data(), 1, out.size(), stdout);
            return 0;
        }
        if (argc == 3 && std::string(argv[1]) == "hashmap") {  // put every k-mer string of the file ("-kmer": remove it as an iterator does, "~kmer": as HashMap.remove does), print both maps' orders
            std::ifstream f(argv[2]);
            if (!f) throw Error("cannot open key file");
            std::vector<std::string> ops;
            for (std::string line; std::getline(f, line);) if (!line.empty()) ops.push_back(line);
            const int k = (int)(ops.empty() ? 1 : ops[0].size() - (ops[0][0] == '-' || ops[0][0] == '~'));
            JavaHashMap hm;
            JavaKmerMap km(k);
            int v = 0;
            for (const std::string &op : ops) {
                if (op[0] == '-' || op[0] == '~') { hm.remove(op.substr(1), op[0] == '~'); km.remove(pack_kmer128(op.substr(1)), op[0] == '~'); }
                else { hm.put(op, v); km.put(pack_kmer128(op), v); v++; }
            }
            printf("S %zu %zu %d\n", hm.size(), hm.bins_treeified(), hm.treeified() ? 1 : 0);
            hm.for_each([](const std::string &key, int val) { printf("s %s %d\n", key.c_str(), val); });
            printf("K %zu %zu %d\n", km.size(), km.bins_treeified(), km.treeified() ? 1 : 0);
            km.for_each([&](kmer_t key, int val, int) { printf("k %s %d\n", unpack_kmer128(key, k).c_str(), val); });
            return 0;
        }
        if (argc >= 6 && std::string(argv[1]) == "multi") {  // multi <out_dir> <seq.fasta> <gene_id> <env>...
            const MultiResult r = environment_finder_multi(std::vector<std::string>(argv + 5, argv + argc), argv[3], atoi(argv[4]));
            write_multi(r, argv[2]);
            for (const auto &l : r.log) printf("%s\n", l.c_str());
            return 0;
        }
        if (argc >= 6 && std::string(argv[1]) == "multi-packed") {  // the same files on packed k-mers: env_join_host + unitigs_by_links
            size_t n = 0;
            const MultiResult r = environment_finder_multi_packed(std::vector<std::string>(argv + 5, argv + argc), argv[3], atoi(argv[4]), env_join_host,
                                                                  unitigs_by_links, &n);
            write_multi(r, argv[2]);
            for (const auto &l : r.log) printf("%s\n", l.c_str());
            printf("ENTRIES %zu\n", n);
            return 0;
        }
        if (argc == 5 && std::string(argv[1]) == "colour") {
            std::ifstream f(argv[2]);
            if (!f) throw Error("cannot open dump");
            int k;
            std::string sequence;
            size_t n, m;
            f >> k >> sequence >> n;
            Environment env(k, {sequence});
            BfsPass pass;
            std::map<kmer_t, unsigned> mask_of;
            for (size_t i = 0; i < n; i++) {
                int d, c;
                unsigned mask;
                std::string kmer;
                f >> kmer >> d >> c >> mask;
                pass.kmers.push_back(pack_kmer128(kmer));
                pass.dist.push_back(d); pass.cov.push_back((int16_t)c); pass.last.push_back(0);
                mask_of[normalize128(pass.kmers.back(), k)] = mask;
            }
            env.add_pass(pass, false);
            std::map<kmer_t, int> graph;
            f >> m;
            for (size_t i = 0; i < m; i++) {
                std::string kmer;
                f >> kmer;
                graph[normalize128(pack_kmer128(kmer), k)] = 1;
            }
            const Environment::Outside o = env.outside_neighbours();
            std::vector<uint8_t> in_graph(o.kmers.size());
            for (size_t i = 0; i < o.kmers.size(); i++) in_graph[i] = graph.count(normalize128(o.kmers[i], k)) != 0;
            printf("Extending endings by %zu kmers\n", Environment::extensions(o, in_graph.data()));
            env.set_colours([&](kmer_t s) { return Environment::colour_of_mask(mask_of.at(s)); });
            env.create_picture();
            write_file(std::string(argv[3]) + "/" + argv[4] + "_seqs.fasta", env.seqs_fasta(0));
            write_file(std::string(argv[3]) + "/" + argv[4] + ".gfa", env.graph_gfa());
            return 0;
        }
        if (argc == 6 && std::string(argv[1]) == "cutreads") {
            const std::string keep = argv[3];
            CutReadsWriter out(argv[4], atoi(argv[5]));
            DnaQReader reader(argv[2]);
            DnaQBatch b;
            b.clear();
            while (reader.read(b, 1000)) {}
            if (keep.size() != b.n_reads()) throw Error("one character of <keep> a read");
            for (size_t r = 0; r < b.n_reads(); r++)
                if (keep[r] == '1') out.add(b.codes.data() + b.offsets[r], (size_t)(b.offsets[r + 1] - b.offsets[r]));
            out.close();
            printf("%llu\n", (unsigned long long)out.kept());
            return 0;
        }
        if ((argc == 3 && std::string(argv[1]) == "dnaq") || (argc == 4 && std::string(argv[1]) == "dnaq-range")) {
            DnaQReader reader(argv[2]);
            printf("fastq %d offset %d\n", reader.fastq() ? 1 : 0, reader.fastq() ? reader.phred_offset() : 0);
            DnaQBatch b;
            auto print = [&] {
                std::string s, q;
                for (size_t r = 0; r < b.n_reads(); r++) {
                    s.clear();
                    q.clear();
                    for (uint64_t i = b.offsets[r]; i < b.offsets[r + 1]; i++) {
                        s.push_back("AGCT"[b.codes[i] & 3]);
                        q.push_back((char)(33 + b.phred[i]));
                    }
                    printf("R %zu\t%s\t%s\n", s.size(), s.c_str(), q.c_str());
                }
                fflush(stdout);  // (what was read before an error is printed)
            };
            auto read_some = [&](DnaQReader &r) {  // (the whole reads in front of the one that throws are printed)
                try {
                    return r.read(b, 7);
                } catch (...) {
                    print();
                    throw;
                }
            };
            if (argc == 3) {
                for (;;) {
                    b.clear();
                    const size_t got = read_some(reader);
                    print();
                    if (got == 0) break;
                }
                return 0;
            }
            // the file cut at record starts every <chunk> bytes, each piece through the reader over a range of memory
            const uint64_t chunk = strtoull(argv[3], nullptr, 10);
            PlainReadsFile f;
            if (!map_plain_reads(argv[2], &f)) throw Error("dnaq-range: not a plain FASTA / FASTQ file");
            for (const auto &cut : plain_chunks(f, chunk)) {
                DnaQReader part(cut.first, cut.second, reader.fastq(), reader.phred_offset());
                for (;;) {
                    b.clear();
                    const size_t got = read_some(part);
                    print();
                    if (got == 0) break;
                }
            }
            return 0;
        }
        if ((argc == 3 || argc == 4) && std::string(argv[1]) == "cuts") {
            PlainReadsFile f;
            if (!map_plain_reads(argv[2], &f)) throw Error("cuts: not a plain FASTA / FASTQ file");
            for (const auto &cut : plain_chunks(f, tokenizer_chunk_bytes_of(argc == 4 ? argv[3] : nullptr))) printf("%td %td\n", cut.first - f.p, cut.second - f.p);
            return 0;
        }
        if (argc == 3 && std::string(argv[1]) == "render-host") {
            auto read = [](size_t i, std::vector<uint8_t> &c, std::vector<uint8_t> &q) {
                c.resize(i % 7 + 1);
                q.resize(c.size());
                for (size_t j = 0; j < c.size(); j++) { c[j] = (uint8_t)((i + j) % 4); q[j] = (uint8_t)((3 * i + 5 * j) % 63); }
            };
            // reads [a, b) as text: numbered from `first` on, or (first == 0) as unnumbered bodies with their lengths
            auto text = [&](size_t a, size_t b, unsigned long long first, std::vector<uint64_t> *lens) {
                std::string t;
                std::vector<uint8_t> c, q;
                for (size_t i = a; i < b; i++) {
                    read(i, c, q);
                    if (first) t += "@" + std::to_string(first + (i - a));
                    t += '\n';
                    for (uint8_t x : c) t += "AGCT"[x];
                    t += "\n+\n";
                    for (uint8_t x : q) t += (char)(x + 64);
                    t += '\n';
                    if (lens) lens->push_back(c.size());
                }
                return t;
            };
            const std::string dir = argv[2];
            std::vector<uint8_t> c, q;
            FastqOut a(dir + "/a.fastq"), b(dir + "/b.fastq");
            for (size_t i = 0; i < 5; i++) { read(i, c, q); a.put(c.data(), q.data(), c.size()); }
            const std::string block = text(5, 10, a.n + 1, nullptr);
            a.put_rendered(reinterpret_cast<const uint8_t *>(block.data()), block.size(), 5);
            a.put_rendered(nullptr, 0, 0);
            for (size_t i = 10; i < 12; i++) { read(i, c, q); a.put(c.data(), q.data(), c.size()); }
            SideList list;
            auto bodies = [&](size_t from, size_t to) {
                std::vector<uint64_t> lens;
                const std::string t = text(from, to, 0, &lens);
                list.put_bodies(reinterpret_cast<const uint8_t *>(t.data()), t.size(), lens.data(), lens.size());
            };
            read(0, c, q);
            list.put(c.data(), q.data(), c.size());
            bodies(1, 5);
            read(5, c, q);
            list.put(c.data(), q.data(), c.size());
            bodies(6, 8);
            bodies(8, 8);
            for (size_t i = 8; i < 10; i++) { read(i, c, q); b.put(c.data(), q.data(), c.size()); }
            list.append_to(b);
            a.close();
            b.close();
            printf("a %llu b %llu\n", a.n, b.n);
            typedef std::vector<std::pair<uint64_t, uint64_t>> Cover;
            const Cover two[2] = {{{0, 5}, {5, 0}, {5, 7}, {12, 30}}, {{0, 3}, {3, 3}, {6, 20}, {26, 10}}}, one[1] = {{{0, 4}, {4, 4}, {8, 1}}};
            for (const RenderRange &r : render_ranges(two, 2, 30)) printf("R %llu %llu %zu %zu\n", (unsigned long long)r.a, (unsigned long long)r.b, r.seg[0], r.seg[1]);
            for (const RenderRange &r : render_ranges(one, 1, 9)) printf("R %llu %llu %zu 0\n", (unsigned long long)r.a, (unsigned long long)r.b, r.seg[0]);
            printf("R none %zu\n", render_ranges(one, 1, 0).size());
            try {
                (void)render_ranges(one, 1, 10);
            } catch (const Error &e) {
                printf("E %s\n", e.what());
            }
            try {
                std::vector<uint64_t> lens(1, 3);
                list.put_bodies(reinterpret_cast<const uint8_t *>("x"), 1, lens.data(), 1);
            } catch (const Error &e) {
                printf("E %s\n", e.what());
            }
            return 0;
        }
        if (argc == 2 && std::string(argv[1]) == "streams") {
            const size_t lens[2] = {0, 3};
            for (int f1 = 0; f1 < 2; f1++)
                for (int f2 = 0; f2 < 2; f2++)
                    for (size_t l1 : lens)
                        for (size_t l2 : lens) {
                            const ClassifiedPair p = classifier_streams(f1 != 0, f2 != 0, l1, l2, true);
                            printf("P %d %d %zu %zu %u %u %d\n", f1, f2, l1, l2, p.st[0], p.st[1], p.counter);
                        }
            for (int f1 = 0; f1 < 2; f1++)
                for (size_t l1 : lens) {
                    const ClassifiedPair p = classifier_streams(f1 != 0, true, l1, 3, false);
                    printf("S %d %zu %u %u %d\n", f1, l1, p.st[0], p.st[1], p.counter);
                }
            for (unsigned c1 = 0; c1 < 3; c1++)
                for (unsigned c2 = 0; c2 < 3; c2++)
                    for (size_t l1 : lens)
                        for (size_t l2 : lens) {
                            const TripleStreams t = triple_streams((uint8_t)c1, (uint8_t)c2, l1, l2);
                            printf("T %u %u %zu %zu %u %u\n", c1, c2, l1, l2, t.st[0], t.st[1]);
                        }
            return 0;
        }
        if (argc == 3 && std::string(argv[1]) == "placement") {
            const int k = atoi(argv[2]);
            if (k < mc::SK_M || k > 32) throw Error("placement: k from 15 to 32");
            unsigned long long w;
            while (scanf("%llx", &w) == 1)
                printf("%llx %x %x %x\n", (unsigned long long)mc::fmix64(w), mc::sk_order((uint32_t)w), mc::sk_bin((uint32_t)w),
                       mc::sk_hmin_of_kmer(k < 32 ? w & ((1ull << (2 * k)) - 1) : w, k));
            return 0;
        }
        if (argc == 4 && std::string(argv[1]) == "placement" && std::string(argv[3]) == "poly") {
            const int k = atoi(argv[2]);
            if (k < mc::SK_M || k > 63) throw Error("placement poly: k from 15 to 63");
            unsigned long long hi, lo;
            while (scanf("%llx %llx", &hi, &lo) == 2) {
                const mc::Kmer v{hi, lo};
                const uint64_t key = (uint64_t)mc::key_poly_plain(v, k);
                const uint32_t h1 = mc::sk_hmin_of_kmer2(v, k, false), h2 = mc::sk_hmin_of_kmer2(v, k, true);
                printf("%llx %x %x %x %x %u\n", (unsigned long long)key, h1, mc::skl_bin(h1), h2, mc::skl_bin(h2), mc::sk_home(key));
            }
            return 0;
        }
        if (argc == 3 && std::string(argv[1]) == "long-tags") {
            FILE *f = fopen(argv[2], "r");
            if (!f) throw Error("cannot open the records file");
            unsigned nw;
            unsigned long long x0, x1, x2;
            while (fscanf(f, "%u %llx %llx %llx", &nw, &x0, &x1, &x2) == 4) {
                const uint32_t h = mc::skl_rec_hash((uint32_t)x0, (uint32_t)(x0 >> 32), (uint32_t)x1, (uint32_t)(x1 >> 32), (uint32_t)x2, (uint32_t)(x2 >> 32), nw);
                printf("%x %x %u\n", h, h >> 16, h & 1023u);
            }
            fclose(f);
            return 0;
        }
        if (argc == 3 && std::string(argv[1]) == "dedup-tags") {
            FILE *f = fopen(argv[2], "r");
            if (!f) throw Error("cannot open the records file");
            unsigned long long lo, hi;
            while (fscanf(f, "%llx %llx", &lo, &hi) == 2) {
                const uint32_t h = mc::dd_hash((uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
                printf("%x %x %u\n", h, (h & 0xFFFF0000u) | 0x8000u, h & 1023u);
            }
            fclose(f);
            return 0;
        }
        if (argc >= 3 && std::string(argv[1]) == "pointers") {
            for (int a = 2; a < argc; a++) {
                const uint64_t pos = strtoull(argv[a], nullptr, 10);
                const uint32_t code = mc::ptr_encode(pos);
                uint32_t span = 0;
                const uint64_t lo = code ? mc::ptr_decode(code, &span) : 0;
                printf("%u %llu %u", code, (unsigned long long)lo, span);
                for (uint32_t j = 0; j < 16; j++) printf(" %u", mc::ptr_advance(code, j));
                for (uint32_t j = 0; j < mc::PTR_LONG_WINDOWS; j++) printf(" %u", mc::ptr_advance_long(code, j));
                printf("\n");
            }
            return 0;
        }
        if (argc == 3 && std::string(argv[1]) == "unitigs") {
            std::ifstream f(argv[2]);
            if (!f) throw Error("cannot open the k-mer file");
            int k;
            size_t n;
            f >> k >> n;
            std::vector<kmer_t> kmers(n);
            std::vector<uint8_t> cls(n);
            for (size_t i = 0; i < n; i++) {
                std::string kmer;
                int c;
                f >> kmer >> c;
                if ((int)kmer.size() != k) throw Error("a k-mer of the file is not k long");
                kmers[i] = pack_kmer128(kmer);
                cls[i] = (uint8_t)c;
            }
            UnitigsResult r;
            unitigs_by_links(k, kmers, cls, r);
            for (size_t u = 0; u < r.first.size(); u++) {
                std::string bases;  // (whole words: the padding prints as A)
                for (uint64_t i = r.base_offsets[u]; i < r.base_offsets[u + 1]; i++) bases.push_back("AGCT"[(r.bases[i >> 5] >> (62 - 2 * (i & 31))) & 3]);
                printf("U %u %u %s\n", r.first[u], r.last_rc[u], bases.c_str());
            }
            for (const uint32_t e : r.irregular) printf("I %u\n", e);
            const Compactor by_links = unitigs_by_links;
            for (int way = 0; way < 2; way++) {
                const std::vector<PictureNode> nodes = make_picture(k, kmers, cls, way ? &by_links : nullptr);
                for (size_t i = 0; i < nodes.size(); i++) {
                    const PictureNode &nd = nodes[i];
                    std::string nb;
                    for (const int j : nd.neighbors) nb += (nb.empty() ? "" : ",") + std::to_string(j);
                    printf("%c %zu %d %s %s [%s]\n", way ? 'N' : 'O', i, nd.deleted ? 1 : 0, nd.deleted ? "-" : std::to_string(nd.rc).c_str(),
                           nd.deleted ? "-" : nd.sequence.c_str(), nb.c_str());
                }
            }
            return 0;
        }
        const bool list_kmers = argc == 3 && std::string(argv[1]) == "kmers";
        if (!list_kmers && (argc != 4 || std::string(argv[1]) != "env")) {
            fprintf(stderr, "usage: mc_hosttest env <dump> <out_prefix> | kmers <dump> | unitigs <k-mers> | placement <k> [poly] | pointers <pos>... | dedup-tags <records> | long-tags <records> | cutreads <reads> <keep> <out.fasta> <index> | dnaq <reads> | dnaq-range <reads> <chunk> | cuts <reads> [<chunk>] | render-host <out_dir> | streams | colour <dump> <out_dir> <name> | seeds <fasta> | reads <file> | fmt <float> | dtoa <hex doubles> | hashmap <keys> | multi <out_dir> <seq> <gene_id> <env>... | multi-packed <out_dir> <seq> <gene_id> <env>...\n");
            return 2;
        }
        std::ifstream f(argv[2]);
        if (!f) throw Error("cannot open dump");
        int k, chunk, trim, n_genes;
        f >> k >> chunk >> trim >> n_genes;
        std::vector<std::string> genes((size_t)n_genes);
        for (auto &g : genes) f >> g;
        int n_passes;
        f >> n_passes;
        Environment env(k, genes);
        for (int p = 0; p < n_passes; p++) {
            BfsPass pass;
            size_t n;
            f >> pass.dir >> n;
            pass.kmers.resize(n); pass.dist.resize(n); pass.cov.resize(n); pass.last.resize(n);
            for (size_t i = 0; i < n; i++) {
                int d, c, l;
                std::string kmer;
                f >> kmer >> d >> c >> l;
                pass.kmers[i] = pack_kmer128(kmer);
                pass.dist[i] = d; pass.cov[i] = (int16_t)c; pass.last[i] = (uint8_t)l;
            }
            env.add_pass(pass, trim != 0);
        }
        if (list_kmers) {
            for (const kmer_t v : env.kmers()) printf("%s\n", unpack_kmer128(v, k).c_str());
            return 0;
        }
        env.write_all(argv[3], chunk);
        return 0;
    } catch (const MultiUnpacked &e) {
        fprintf(stderr, "unpacked: %s\n", e.what());
        return 3;
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
