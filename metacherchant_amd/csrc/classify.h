// The verdict of the reads-classifier on one read (src/algo/ReadsFinderInGraph.java:37-49,95-103), from the three numbers
// the kernel reduces a read to.  One function for the kernel (csrc/classify.hip) and for host code: it compiles as HIP and as
// plain C++.
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

}  // namespace mc
