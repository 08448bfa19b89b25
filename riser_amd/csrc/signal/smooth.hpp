// The output pass of MAD normalisation by one workgroup of THREADS threads: y = (x - med) / denom and the reference's sequential
// in-place smoothing of {|y| > lim} (riser/preprocess.py:128-147; the retraining script's copy is riser/retrain/preprocess.py:18-33),
// in T, one rounding per operation.  The outliers are fixed before any update, they are rewritten in ascending order, and each
// replacement needs the one before it: every thread writes the elements that are no outliers, and the first element of a run of
// outliers walks its run.  NaN is no outlier, +-inf is one, and a NaN replacement passes the clip.  With a zero denom every element
// off the median is +-inf, a run can span the whole read and one lane walks it: rare (more than half of the samples equal) and
// accepted.  Input edges (tests/test_float_edges.py): a NaN med or denom (a NaN sample, or an infinite median: radix_select.hpp)
// makes every y NaN, no element is an outlier and the row is NaN; an infinite sample beside a finite med and denom is an outlier,
// (prev + inf) / 2 clips to +-lim and index 0 / n - 1 copy their neighbour unclipped; an infinite denom (an overflowing 1.4826 *
// mad) gives +-0.0 and, with an infinite MAD, NaN off the median; subnormal y are kept, nothing is flushed.
#pragma once

#include "float_arith.hpp"

namespace rs {

// x(j): sample j of the read (0 <= j < n); o: the output row.  med is the read's median, so a lone sample (n == 1) deviates by 0
// or NaN and is no outlier: x(1) is read only where n >= 2
template <class T, int THREADS, class XF>
__device__ __forceinline__ void smooth_write(XF x, int n, T med, T denom, T lim, T* o, int tid) {
    typedef Arith<T> A;
    auto yv = [&](int j) -> T { return A::div(A::sub(x(j), med), denom); };
    auto is_out = [&](int j) { return A::abs(yv(j)) > lim; };         // :129; false for NaN
    for (int i = tid; i < n; i += THREADS) {
        if (!is_out(i)) {
            o[i] = yv(i);
            continue;
        }
        if (i > 0 && is_out(i - 1)) continue;                         // inside a run: its head writes it
        T prev = i > 0 ? yv(i - 1) : (T)0;
        int j = i;
        do {
            T nv;
            if (j == 0) {
                nv = yv(1);                                           // :132 (not clipped)
            } else if (j == n - 1) {
                nv = prev;                                            // :134 (not clipped)
            } else {
                nv = A::div(A::add(prev, yv(j + 1)), (T)2);           // :136
                nv = nv > lim ? lim : (nv < -lim ? -lim : nv);        // :141-147; NaN passes
            }
            o[j] = nv;
            prev = nv;
            ++j;
        } while (j < n && is_out(j));
    }
}

}  // namespace rs
