// The fit of samples given on a tensor-product grid of points (fitgrid.hip), as the entries of fitgridapi.hip drive it:
// the host tables of a call (one per axis, shared by all fields), then the device passes field by field.
#pragma once
#include "kernels.hpp"

#include <vector>

namespace splpak {

// What the host keeps of one axis.  "Table order" = the coordinates ordered by (window start, original index): the
// contributions to a node are a contiguous range of it.
struct FitGridAxis {
    long long n = 0;                  // coordinates
    int nod = 0;                      // nodes
    std::vector<int> ws;              // [n] window start, original order
    std::vector<double> b;            // [n][4] general-form window values (window_table), original order
    std::vector<double> w2;           // [n] squared weight, original order
    std::vector<long long> order;     // [n] original index of table position p
    std::vector<long long> start;     // [nod - 2] first table position whose window start is >= s (start[nod - 3] = n)
    std::vector<double> nrm;          // [nod][4] N = A^T W^2 A, lower band: N(j, j - k) at 4 j + k
    std::vector<double> chol;         // [nod][4] its Cholesky factor in the same layout
    double minpiv = 0.0;              // smallest pivot (the diagonal entry before the square root)
    bool spd = true;                  // every pivot positive and at least nod * eps * (largest diagonal entry of N)
    long long nonzero = 0;            // coordinates with a non-zero weight
};

struct FitGridHost {
    Grid g;
    long long npts[MAXD] = {1, 1, 1, 1};
    long long nsamp = 1;              // prod npts
    FitGridAxis ax[MAXD];
    double seconds = 0.0;             // spent on the tables and factors
};

// The host part: tables, normal matrices, factors, the xtrap rule.  axes / waxes (may be null): the axes back to back,
// widened to double.  0; SPLPAK_E_UNSUPPORTED (xtrap != 0 and the constraint rows are not separable: set_error says so);
// 107 (an axis whose normal matrix is not numerically positive definite); SPLPAK_E_NOMEM.  Touches no device.
int fit_grid_host(const Grid &g, const int64_t *npts, const double *axes, const double *waxes, double xtrap, FitGridHost &h);

// The normal matrices and factors of h again for other axis weights, given SQUARED, one per axis coordinate (the axes back
// to back); the window values and the table order stay.  0; 107 as fit_grid_host.
int fit_grid_host_reweight(FitGridHost &h, const double *w2axes);

// The device part.  Field k's samples at values + k*ldv, its coefficients to coef + k*ldcoef; `on_host`: both are host
// arrays and are staged field by field (the words between the fields are neither read nor written), else device arrays.
// info: 10 per field or null.  0; 107 (the refinement missed 1e-10); SPLPAK_E_NOMEM; SPLPAK_E_NODEVICE.
// Synchronises st (once per refinement step and at the end of every field).
template <typename T>
int fit_grid_device(const FitGridHost &h, int nfields, const T *values, long long ldv, T *coef, long long ldcoef, double *info,
                    bool on_host, hipStream_t st);

// One stage alone, host arrays, one field: 0: out[ncol] = the spread of in[nsamp]; 1: out[ncol] = the solves of in[ncol]
int fit_grid_stage(const FitGridHost &h, int stage, const double *in, double *out);

// host counters of the calling thread's last fit_grid_device / fit_grid_stage: slabs of a residual pass [0], doubles of
// residual scratch held [1], spread launches [2], solve launches [3], refinement steps of the last field [4], 0 [5..7]
void fit_grid_stats(long long out8[8]);

// ---- fitgridw.hip: a weight per sample (splpak_fit_grid_weighted_*)
// h: the tables of fit_grid_host WITHOUT axis weights and with xtrap = 0 (changed: the factors become those of the
// preconditioner of the last weight set); axes: the host copy the tables were made from (the xtrap rule counts from it).
// Field k's weights at weights + k*ldw in the layout of its samples, ldw = 0: one set for all fields.  Status as the header
// gives it; synchronises st.
template <typename T>
int fit_grid_weighted_device(FitGridHost &h, const double *axes, double xtrap, int nfields, const T *values, long long ldv,
                             const T *weights, long long ldw, T *coef, long long ldcoef, double *info, bool on_host, hipStream_t st);
// One stage alone, host arrays, one field (the header: right-hand side, operator, preconditioner, marginals and diagonal)
int fit_grid_weighted_stage(FitGridHost &h, const double *axes, int stage, const double *weights, const double *in, double *out);
void fit_grid_weighted_stats(long long out8[8]);

}  // namespace splpak
