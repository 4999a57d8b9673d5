// fp64 pieces shared by the heads that solve small symmetric systems from fp64 moments (K25 ridge.hip, K28 logreg.hip,
// K32 spectral.hip): the packed-triangle index maps and the Cholesky-Crout factorisation in LDS.
#pragma once
#include "common.h"

namespace gae {

__host__ __device__ inline int64_t tri(int64_t w) { return w * (w + 1) / 2; }
// entry (i, j), i <= j, of a packed upper triangle of order W (rows one after another)
__device__ __forceinline__ int64_t upper_at(int i, int j, int W) { return int64_t(i) * W - int64_t(i) * (i - 1) / 2 + (j - i); }

// Cholesky-Crout of rows 0 .. d - 1 of a matrix held row by row in LDS (row i at Lm + row_at(i), entries 0 .. min(i, d - 1)),
// column by column; thread r of the block owns row j + r, so the block holds at least D threads.  Rows d .. D - 1 are
// right-hand sides carried along (forward substitution).  The factor's diagonal goes to dg[]; Lm's own diagonal keeps its
// value.  Returns 0, or LAPACK style the 1-based index of the first pivot that is <= 0 or not finite -- the same value
// in every thread.  Every thread of the block calls; the data is in place (a barrier) before the call.
template <class RowAt>
__device__ __forceinline__ int cholesky_crout(double *Lm, double *dg, int d, int D, int tid, RowAt row_at)
{
    for (int j = 0; j < d; ++j) {
        const int i = j + tid;
        const bool on = i < D;
        const double *rj = Lm + row_at(j);
        double *ri = Lm + row_at(on ? i : j);
        double piv = rj[j], s = ri[j];
        for (int k = 0; k < j; ++k) {
            const double ljk = rj[k];
            piv -= ljk * ljk;
            s -= ri[k] * ljk;
        }
        if (!(piv > 0.0 && piv <= DBL_MAX)) return j + 1;          // the same value in every thread
        const double ljj = sqrt(piv);
        if (i == j) dg[j] = ljj;                                   // rj[j] keeps its value: others may still read it
        else if (on) ri[j] = s / ljj;
        __syncthreads();
    }
    return 0;
}

} // namespace gae
