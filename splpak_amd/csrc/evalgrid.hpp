// What the two grid routes share (evalgrid.hip: one nderiv pattern; evalgridderivs.hip: value, gradient and Hessian
// planes): the shape of a call as the kernels see it, the workgroup size and the per-thread scratch.
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

}  // namespace splpak
