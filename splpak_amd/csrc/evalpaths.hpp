// What the dispatchers of eval.hip call in the files of the sorted evaluation paths.  Every path takes the dimension count
// from the grid, keeps its own per-thread scratch (evalscratch.hpp) and returns the bits of the direct kernel.  chunk =
// queries sorted per pass (0 = default).
#pragma once
#include "evalcore.hpp"
#include "evaltile.hpp"
#include "kernels.hpp"

namespace splpak {

// evalsort.hip -- regions of the grid (run path and region sort); false when the binned paths do not apply
bool make_regions(const Grid &g, Regions &rg);
// order == 0: one nderiv pattern (nd) -> out[nq]; order 1 / 2 (double only): value + gradient (+ Hessian) -> out[nq][ldout].
// The error of a failed scratch allocation is returned as it is (hipErrorOutOfMemory: the caller takes the direct kernel).
template <typename T>
hipError_t eval_sort(const Grid &g, const Regions &rg, long long nq, const T *xq, int ldxq, const NDeriv &nd, const T *coef, T *out,
                     long long chunk, hipStream_t st, int order, int ldout);
void eval_sort_shutdown();

// evalruns.hip -- hipErrorNotSupported = not for this grid / batch, take the region sort; hipErrorOutOfMemory = no room
template <typename T>
hipError_t eval_runs(const Grid &g, const Regions &rg, long long nq, const T *xq, int ldxq, const NDeriv &nd, const T *coef, T *out,
                     long long chunk, hipStream_t st);
void eval_runs_shutdown();

// evalregion.hip -- hipErrorNotSupported = not for this grid, or no room for its scratch: take the run path (decided before
// anything is launched).  nfields > 1: field k's coefficients at coef + k*ldcoef, its results to out + k*ldout, ONE sort of the
// queries for all of them
template <typename T>
hipError_t eval_persistent(const Grid &g, long long nq, const T *xq, int ldxq, const NDeriv &nd, const T *coef, T *out, hipStream_t st,
                           int nfields = 1, long long ldcoef = 0, long long ldout = 0);
void eval_persistent_shutdown();

}  // namespace splpak
