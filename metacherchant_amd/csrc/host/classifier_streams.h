// Which output stream each read of a pair goes to in the two classifiers (tool_classifiers.cpp): the one place that holds the rule, for
// --render gpu (the stream bytes of mc_render_fastq) and --render host (the FastqOut or SideList the stream names) alike.  Free of
// HIP, like fastq_out.h, so that mc_hosttest prints both rules for every input (`mc_hosttest streams`).
#pragma once
#include <cstddef>
#include <cstdint>

#include "mcgpu.h"

namespace mch {

// reads-classifier's eight streams: the four pair files, the heads of the two _s files (the "first only" pairs) and their tails (the
// "second only" pairs, kept aside and numbered behind the heads when the run ends)
constexpr uint8_t FOUND_1 = 0, FOUND_2 = 1, NF_1 = 2, NF_2 = 3, FOUND_S = 4, NF_S = 5, FOUND_S_TAIL = 6, NF_S_TAIL = 7, CLASSIFIER_STREAMS = 8;
// ... and the four counters of its FoundStats (ReadsClassifier.java:203-260)
enum { PAIR_BOTH, PAIR_FIRST_ONLY, PAIR_SECOND_ONLY, PAIR_NEITHER };

struct ClassifiedPair {
    uint8_t st[2];  // the stream of each side, MC_RENDER_SKIP for none
    int counter;    // PAIR_*
};

// PairFinder.run (src/algo/PairFinder.java:32-57) and the files of ReadsClassifier.java:154-200: found_{1,2} and not_found_{1,2} take
// every read of their pairs (an empty one fails the writer), the _s files only reads of length > 0.  A single-end read is paired
// with an empty one.
inline ClassifiedPair classifier_streams(bool found1, bool found2, size_t len1, size_t len2, bool paired)
{
    if (!paired) len2 = 0;
    if (len2 == 0) found2 = !found1;
    if (found1 && found2) return {{FOUND_1, FOUND_2}, PAIR_BOTH};
    constexpr uint8_t SKIP = MC_RENDER_SKIP;
    if (found1) return {{len1 ? FOUND_S : SKIP, len2 ? NF_S : SKIP}, PAIR_FIRST_ONLY};
    if (found2) return {{len1 ? NF_S_TAIL : SKIP, len2 ? FOUND_S_TAIL : SKIP}, PAIR_SECOND_ONLY};
    return {{NF_1, NF_2}, PAIR_NEITHER};
}

struct TripleStreams {
    uint8_t st[2];
};

// triple-reads-classifier's nine streams (TripleReadsClassifier.java:248-267): 2 * class + side, the pair files of a pair whose mates
// share a class -- found_{1,2} take every read, the others only reads of length > 0 -- and 6 + class, the _s files, for the mates of a
// mixed pair that have a length
inline TripleStreams triple_streams(uint8_t class1, uint8_t class2, size_t len1, size_t len2)
{
    const uint8_t cls[2] = {class1, class2};
    const size_t len[2] = {len1, len2};
    TripleStreams r{{MC_RENDER_SKIP, MC_RENDER_SKIP}};
    for (int s = 0; s < 2; s++) {
        if (class1 == class2) {
            if (len[s] || class1 == MC_CLASS_FOUND) r.st[s] = (uint8_t)(2 * class1 + s);
        } else if (len[s]) {
            r.st[s] = (uint8_t)(6 + cls[s]);
        }
    }
    return r;
}

}  // namespace mch
