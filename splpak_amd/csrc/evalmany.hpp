// A batch of small fits evaluated at each problem's own points (evalmany.hip; the entries: evalmanyapi.hip).  Problem k owns
// the global indices offsets[k] .. offsets[k+1]-1; an array of points (xq / xdata, ydata, wdata, out, resid) is addressed at
// the global index minus `base` (0 for the caller's device arrays, offsets[0] for the staged span of a host entry); problem
// k's coefficients are at coef + k*ldcoef.
#pragma once
#include "kernels.hpp"

namespace splpak {

constexpr int EVALMANY_THREADS = 256;             // eval_many: a thread per query
constexpr long long EVALMANY_BLOCKS = 256LL * 32; // .. in at most that many workgroups (launch_eval's cap): a sweep; the rest is strided
constexpr int RESMANY_WAVES = 256 * 32;           // residuals_many: a one-wave workgroup per problem, at most that many; the rest is strided

// host counters of the calling thread's last call of either family (splpak_debug_eval_many_stats)
extern thread_local long long t_eval_many_stats[8];

// offsets_dev: the device copy of a call's offsets (manyhost.hpp: many_offsets_upload).

// out[i - base] for every query i of offsets[0] .. offsets[nbatch]-1: the bits of launch_eval's direct kernel on query i with
// the coefficients of the problem that owns i.  nq = offsets[nbatch] - offsets[0] > 0; one launch.
template <typename T>
hipError_t launch_eval_many(const Grid &g, int nbatch, const long long *offsets_dev, long long first, long long nq, long long base,
                            const T *xq, int ldxq, const int *nderiv, const T *coef, long long ldcoef, T *out, hipStream_t st);

// out[i - base] = a^T Z a for every query i, a the window row launch_eval_many contracts with the coefficients, Z from the half
// stencil of the owner's covariance at cov + k*ldcov (splpak_fit_many_cov_*); g.ndim is 1 or 2; one launch.
template <typename T>
hipError_t launch_eval_many_var(const Grid &g, int nbatch, const long long *offsets_dev, long long first, long long nq, long long base,
                                const T *xq, int ldxq, const int *nderiv, const T *cov, long long ldcov, T *out, hipStream_t st);

// resid[i - base] = (T)(y_i - f_i) and stats[4k .. 4k+3] = {points counted, sum (w r)^2, max |w r|, first local index of the max}
// of every problem (either may be null); one launch, a wave per problem.
template <typename T>
hipError_t launch_residuals_many(const Grid &g, int nbatch, const long long *offsets_dev, long long base, const T *xdata, int l1xdat,
                                 const T *ydata, const T *wdata, const T *coef, long long ldcoef, T *resid, double *stats, hipStream_t st);

// stats[4k .. 4k+3] = {points counted, median, MAD, 0} of values[offsets[k] - base .. offsets[k+1] - base) where wsel (may be
// null: all) is not 0 (madmany.hip; the definitions: include/splpak_hip.h, splpak_mad_many_*); one launch, a wave per problem.
template <typename T>
hipError_t launch_mad_many(int nbatch, const long long *offsets_dev, long long base, const T *values, const T *wsel, double *stats,
                           hipStream_t st);

}  // namespace splpak
