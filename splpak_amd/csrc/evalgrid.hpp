// What the grid routes share (evalgrid.hip: one nderiv pattern; evalgridderivs.hip: value, gradient and Hessian
// planes; integrategrid.hip: integrals over the cells of a tensor grid; fitgrid.hip: the residual of the grid fit): the
// shape of a call as the kernels see it and the one function that fills it (grid_shape), the workgroup size, the per-thread
// scratch (its end-of-use guard: ScratchUse, evalscratch.hpp), the tile kernel of evalgrid.hip on prepared tables and
// the slab size its callers may give it (eval_grid_slab).
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

// The shape of a call from the counts of its ndim dimensions: npts (1 beyond ndim), off (the prefix of npts; from ndim on the
// table length, which is gs.off[MAXD]) and ntile = 1 (a launcher sets its own).  False: a count below 1, the empty product.
template <typename N>
inline bool grid_shape(int ndim, const N *counts, GridShape &gs)
{
    long long ntab = 0;
    for (int d = 0; d < MAXD; ++d) {
        const long long n = d < ndim ? (long long)counts[d] : 1;
        if (n <= 0) return false;
        gs.npts[d] = n;
        gs.off[d] = ntab;
        gs.ntile[d] = 1;
        if (d < ndim) ntab += n;
    }
    gs.off[MAXD] = ntab;
    return true;
}

// per-thread scratch of the grid routes (evalgrid.hip): tile counters | factors | window starts of the last call
DevScratch<1> &eval_grid_scratch();

// outputs of a workgroup tile of eval_grid_kernel in dimension d < MAXD (1 beyond ndim)
int eval_grid_tile(int ndim, int d);

// The positions of the last dimension a slab of launch_eval_grid_tables may hold: the most that `cap` doubles allow at `row`
// doubles per position (row >= 1) and that keep the slab below the 2^31 tiles of a launch.  npts: the positions of the
// dimensions below the last (ndim - 1 of them).  qmax may be 0, where a single position is above the cap: what then is the
// caller's.  False: no slab can be launched (the tiles of one position alone are beyond 2^31 - 1, or their count overflows).
bool eval_grid_slab(int ndim, const long long *npts, long long row, long long cap, long long &qmax);

// eval_grid_kernel on prepared tables: entry gs.off[d] + i (window start wst[], four factors fac[4 *]) belongs to output
// position i < gs.npts[d] of dimension d; out[i0 + npts[0] (i1 + ...)] = the contraction of the coefficient window with the
// factors.  gs.npts (1 beyond ndim) and gs.off are the caller's, gs.ntile is set here; hipErrorInvalidValue from 2^31 tiles on.
// TC / TO: storage of the coefficients / outputs (double-double, float-float, float-double); stats: two tile counters or null.
template <typename TC, typename TO>
hipError_t launch_eval_grid_tables(const Grid &g, GridShape &gs, const double *fac, const int *wst, const TC *coef, TO *out,
                                   unsigned long long *stats, hipStream_t st);

}  // namespace splpak
