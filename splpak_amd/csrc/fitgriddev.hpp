// What the two grid fits share on the device (fitgrid.hip owns all of it; fitgridw.hip, the fit with a weight per sample, uses
// it): the layout of a call's scratch, the unit of a spread launch, the passes below the last dimension, the solves along
// the axes, the residual norm's sums, the refinement rule and the final store.
#pragma once
#include "fitgrid.hpp"
#include "evalgrid.hpp"

#include <limits>

namespace splpak {

struct SpreadArgs {
    long long inner, np, outer;      // in[i + inner (c + np o)], c = a coordinate of this axis; out[i + inner (j + nod o)]
    long long pa, pb;                // the table positions of this launch
    int nod, nbk, nblk;              // nodes, nodes per block, blocks
    int cont;                        // the running sums continue from `out` (a later slab)
    const double *G;                 // [np][4] w^2 * window values, table order
    const int *ws;                   // [np] window starts, table order
    const long long *idx;            // [np] original index of a table position
    const long long *start;          // [nod - 2]
    // the residual pass alone: in = the samples, indexed by original index; sub = A C of the slab, indexed by p - pa
    const double *w2s;               // [np] squared weights of this axis, table order
    const double *w2lo[MAXD];        // squared weights of the dimensions below, original order
    long long nlo[MAXD];
    int nlow;
};

constexpr long long SPREAD_WAVE_FORM = 128;      // lane positions from which a pass takes the wave form
constexpr int SPREAD_BATCH = 8;                  // samples a thread asks for at a time, one batch ahead of their use

// Everything a call keeps on the device, carved out of one buffer (offsets in doubles).
struct Layout {
    long long off[MAXD + 1];      // table entries of every axis (prefix of npts)
    long long offn[MAXD + 1];     // prefix of nodes
    long long offs[MAXD + 1];     // prefix of nodes - 2
    long long G, fac, w2o, w2s, idx, start, chol, wsS, wstE;      // tables
    long long tables;                                             // doubles of tables (uploaded in one copy)
    long long small, X, R, A, B, sq, rows, part, AC, stageV, stageC, extra, total;      // extra: the caller's own
    long long szA, szB, q, nslab;  // table positions of the last dimension per slab; slabs
};

struct Device {
    const FitGridHost &h;
    Layout L;
    double *base = nullptr;
    hipStream_t st;
    int D, last;
    Device(const FitGridHost &hh, hipStream_t s) : h(hh), st(s), D(hh.g.ndim), last(hh.g.ndim - 1) {}
    double *at(long long o) const { return base + o; }
};

// The scratch of the grid fits (per thread) and the counters of fit_grid_stats.
DevScratch<1> &fit_grid_scratch();
extern thread_local long long t_fit_grid_stats[8];

// The scratch of the call (with `extra` doubles of the caller's own at L.extra) and its tables on the device; resets the
// counters; 0 or a status.  Synchronises dv.st.
int device_begin(Device &dv, bool refine, long long stage_values_bytes, long long stage_coef_bytes, long long extra);
// the launch of the pass of dimension d over the whole axis, with the tables of the call (G: w^2 * window values)
SpreadArgs spread_args(const Device &dv, int d);
int fit_grid_node_block(long long inner, long long outer, int nod);
// one pass of doubles without the residual's extras
hipError_t launch_spread_plain(const SpreadArgs &a, const double *in, double *out, hipStream_t st);
// the passes below the last dimension: cur (the last dimension's result) -> dst[ncol]; tables: [4 sum npts] in the layout
// of Layout::G instead of it, or null
hipError_t spread_rest(const Device &dv, const double *cur, double *dst, const double *tables);
// Layout::AC = A x at the table positions pa .. pb - 1 of the last dimension (a slab: at most Layout::q of them)
hipError_t eval_slab(const Device &dv, const double *x, long long pa, long long pb);
// small[2] = the sum of Layout::sq[inner][nod], the sums a residual pass keeps per (lane position, window start)
hipError_t residual_norm(const Device &dv, long long inner, int nod);
const char *fit_grid_xtrap_message();
// x[ncol] <- (N_1^-1 x ... x N_D^-1) x with the factors at Layout::chol
hipError_t solve_all(const Device &dv, double *x);
template <typename T>
hipError_t launch_fit_store(const double *x, T *coef, int n, hipStream_t st);      // coef[i] = (T)x[i]

// The fit's own refinement rule (planfit.hip refinement_advance): stop when the estimated remaining error is below tol, go
// on while the corrections contract, fail (107) when that leaves an estimate above the parity bar.
struct RefineRule {
    static constexpr double tol = 1e-11;
    int steps = 0;
    double last_rel = 0.0, prev_rel = std::numeric_limits<double>::infinity(), ratio = 0.0;
    bool converged = false;
    // after step `it` (from 0): am = |correction|_inf, |coef|_inf.  True: the loop ends.
    __host__ __device__ bool advance(int it, const double *am)
    {
        ++steps;
        last_rel = am[1] > 0.0 ? am[0] / am[1] : 0.0;
        if (am[0] != am[0] || am[1] != am[1]) last_rel = std::numeric_limits<double>::quiet_NaN();
        if (!(last_rel == last_rel)) return true;
        if (last_rel <= tol) { converged = true; return true; }
        if (it >= 1) {
            ratio = last_rel / prev_rel;
            if (ratio < 0.9 && last_rel * ratio / (1.0 - ratio) <= tol) { converged = true; return true; }
            if (ratio >= 0.9) { converged = last_rel <= 1e-10; return true; }
        }
        prev_rel = last_rel;
        return false;
    }
    // the estimate that decides 107 where the loop ended without converging
    __host__ __device__ double estimate() const { return steps >= 2 && ratio > 0.0 && ratio < 1.0 ? last_rel * ratio / (1.0 - ratio) : last_rel; }
};

}  // namespace splpak
