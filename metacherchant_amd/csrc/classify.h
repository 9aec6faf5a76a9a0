// The verdict of the reads-classifier on one read (src/algo/ReadsFinderInGraph.java:37-49,95-103), from the three numbers
// the kernel reduces a read to, and the triple-reads-classifier's width and class rules.  One copy for the kernels
// (csrc/classify.hip) and for host code: it compiles as HIP and as plain C++.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MC_CLASSIFY_HD __host__ __device__
#else
#define MC_CLASSIFY_HD
#endif

namespace mc {

// sum: the windows' coverages summed as a Java int; covered: windows with coverage > 0; last: the last window's coverage;
// len: the read's length (>= k); thr: the breadth threshold (found_threshold / 100, or 0.9 under correction); z: 1 or 1.96.
MC_CLASSIFY_HD inline bool classify_verdict(int32_t sum, int32_t covered, int32_t last, int32_t len, int k, double thr, double z)
{
    // (int arithmetic as in Java: the sums wrap, then one conversion to double)
    const int32_t total = (int32_t)((uint32_t)sum + (uint32_t)last * (uint32_t)(k - 1));
    const int32_t breadth = (int32_t)((uint32_t)covered + (last > 0 ? (uint32_t)(k - 1) : 0u));
    const double cov_mean = (double)total / len;
    const double width = (double)breadth / len;
    const double theory_width = 1.0 - exp(-cov_mean);
    const double std_dev = z * sqrt(exp(-cov_mean) * (1 - exp(-cov_mean)) / len);
    return !(width < thr) && (width == 1 || (width != 0 && -std_dev <= width - theory_width && width - theory_width <= std_dev));
}

// the classes of the triple-reads-classifier (include/mcgpu.h MC_CLASS_*: TripleReadsClassifier.FindResult)
enum : uint8_t { CLASS_NOT_FOUND = 0, CLASS_HALF_FOUND = 1, CLASS_FOUND = 2 };

// getWidth (src/algo/TripleFinder.java:70-76, TripleFinder2.java:113-119): the breadth of the read as given, 0 when len < k
MC_CLASSIFY_HD inline double triple_width(int32_t covered, int32_t last, int32_t len, int k)
{
    if (len < k) return 0;
    return (double)(int32_t)((uint32_t)covered + (last > 0 ? (uint32_t)(k - 1) : 0u)) / len;
}

// pass 1 (TripleFinder.java:48-61): found, else half found when the width reaches half (half_threshold / 100)
MC_CLASSIFY_HD inline uint8_t triple_class_pass1(bool found, double width, double half)
{
    return found ? CLASS_FOUND : width >= half ? CLASS_HALF_FOUND : CLASS_NOT_FOUND;
}

// pass 2 (TripleFinder2.java:58-76): f the verdict at k2, c1 the pass-1 class of the read's bases
MC_CLASSIFY_HD inline uint8_t triple_class_pass2(bool f, uint8_t c1, double width, double half)
{
    if (f && c1 == CLASS_FOUND) return CLASS_FOUND;
    if (f || c1 == CLASS_FOUND || (width >= half && c1 == CLASS_HALF_FOUND)) return CLASS_HALF_FOUND;
    return CLASS_NOT_FOUND;
}

}  // namespace mc
