// What the clipping loops of the batch fits share (fitmanyclip.hip: the rms rule; fitmanymad.hip: the median / MAD rule): the
// starting weights, the coefficients as stored, the weighted residual of a point on them and the head of the result block.  The
// loops themselves stay in their kernels, each tuned to its register limit.  After a fit L.rho is free and gets (double)(T) x in
// the caller's node order, the very values eval_point (evalmany.hip) loads from `coef`; the factor tables and window_sum are
// those of evalcore.hpp on the grid in the CALLER's order, so r has the bits of splpak_residuals_many_* before its rounding.
#pragma once
#include "fitmanydev.hpp"
#include "evalcore.hpp"

namespace splpak {
namespace fitmanydev {

// eval_point of evalmany.hip (value pattern) with the window rows read from cf in LDS: the coefficients as stored, widened
template <int D, typename T>
__device__ inline double eval_from_lds(const Grid &g, const T *__restrict__ x, const double *cf)
{
    double b[D][4];
    int base = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double xd = (double)x[d];
        const int ws = eval_table<true>(g, d, xd, 0, b[d]);
        base += ws * g.colstride[d];
    }
    const int s1 = D > 1 ? g.colstride[1] : 0;
    return window_sum<D>(b, [&](int k1, int, int, double (&c)[4]) {
        const double *p = cf + base + k1 * s1;
        c[0] = p[0]; c[1] = p[1]; c[2] = p[2]; c[3] = p[3];
    });
}

// t = w r of point i (w != 0), each operation rounded on its own
template <int D, typename T>
__device__ inline double weighted_residual(const Grid &g, const T *__restrict__ xd, int l1xdat, const T *__restrict__ yd, long long i,
                                           double w, const double *cf)
{
#pragma clang fp contract(off)
    const double f = eval_from_lds<D, T>(g, xd + i * l1xdat, cf);
    const double r = (double)yd[i] - f;
    return w * r;
}

// The starting weights of a clipping loop into `wout` (the caller's, or 1 per point).  The first-weight decision is taken here,
// from wdata, and never again: it is returned.  (The opening barrier of the first fit orders these stores before its loads.)
template <typename T, int NT>
__device__ inline bool starting_weights(const T *__restrict__ wdata, T *wout, long long p0, long long np)
{
    const int tid = threadIdx.x;
    const bool weighted = first_weight_counts(wdata, p0);
    for (long long p = tid; p < np; p += NT) wout[p0 + p] = weighted ? wdata[p0 + p] : (T)1;
    return weighted;
}

// The coefficients as stored, after a fit: L.x rounded to T, into L.rho in the caller's node order; ends with a barrier
template <int D, typename T, int NT>
__device__ inline void coefficients_as_stored(const Grid &g, const Lds &L, int n)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += NT) {
        int in[D], refnode = 0;
        node_of<D>(g, i, in);
#pragma unroll
        for (int d = 0; d < D; ++d) refnode += in[d] * g.refstride[d];
        L.rho[refnode] = (double)(T)L.x[i];
    }
    __syncthreads();
}

// The result block of a loop kernel up to the rule's own slots: the FM_* slots of the LAST fit, FM_SPARE = the fits the
// problem ran; one thread calls it
__device__ inline void store_loop_outcome(const FitOutcome &o, int fits, double *res)
{
    store_outcome(o, res);
    res[FM_SPARE] = (double)fits;
}

}  // namespace fitmanydev
}  // namespace splpak
