// What the grid routes share (evalgrid.hip: one nderiv pattern; evalgridderivs.hip: value, gradient and Hessian
// planes; integrategrid.hip: integrals over the cells of a tensor grid): the shape of a call as the kernels see it, the
// workgroup size, the per-thread scratch and the tile kernel of evalgrid.hip on prepared tables.
#pragma once
#include "evalcore.hpp"
#include "evalscratch.hpp"

namespace splpak {

constexpr int GRID_NT = 256;

struct GridShape {
    long long npts[MAXD];      // outputs per dimension
    long long off[MAXD + 1];   // first table entry of every dimension (prefix of npts)
    long long ntile[MAXD];     // tiles per dimension
};

// per-thread scratch of the grid routes (evalgrid.hip): tile counters | factors | window starts of the last call
DevScratch<1> &eval_grid_scratch();

// outputs of a workgroup tile of eval_grid_kernel in dimension d < MAXD (1 beyond ndim)
int eval_grid_tile(int ndim, int d);

// eval_grid_kernel on prepared tables: entry gs.off[d] + i (window start wst[], four factors fac[4 *]) belongs to output
// position i < gs.npts[d] of dimension d; out[i0 + npts[0] (i1 + ...)] = the contraction of the coefficient window with the
// factors.  gs.npts (1 beyond ndim) and gs.off are the caller's, gs.ntile is set here; hipErrorInvalidValue from 2^31 tiles on.
// TC / TO: storage of the coefficients / outputs (double-double, float-float, float-double); stats: two tile counters or null.
template <typename TC, typename TO>
hipError_t launch_eval_grid_tables(const Grid &g, GridShape &gs, const double *fac, const int *wst, const TC *coef, TO *out,
                                   unsigned long long *stats, hipStream_t st);

}  // namespace splpak
