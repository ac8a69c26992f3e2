// The evaluation entries of the C ABI (include/splpak_hip.h): point, derivative and grid evaluation on host and device
// pointers, the evaluation mode, and the host-only / synthetic-data helpers that need no plan.
//
// Every entry family has ONE ladder of argument checks (point_validate for the value and the derivative entries,
// fields_validate, grid_validate, integrate_validate, grid_derivs_validate), one device form and one host form that stages its
// arrays through the device (staged_call: one block of results or several, a stride apart); the extern "C" functions forward
// to them.  The three grid ladders share their opening and close (grid_open, grid_close: GridCheck) and differ in the middle;
// what a failed ladder zeroes is zeroed by zero_results.
// Where two entries of a family have always answered differently, the difference is a named parameter of the ladder.
#include "plan.hpp"
#include "basis.hpp"
#include "manyhost.hpp"

#include <cstdio>
#include <vector>

using namespace splpak;

// returns 0/101/102/103/104 exactly like splde's checks (:1166-1194)
static int eval_validate(int32_t ndim, const int32_t *nderiv, const double *xmin, const double *xmax,
                         const int32_t *nodes, Grid &g)
{
    int v = build_grid(ndim, nodes, xmin, xmax, g, nullptr);
    if (v != 0) return v;
    if (nderiv)
        for (int d = 0; d < ndim; ++d)
            if (nderiv[d] < 0 || nderiv[d] > 2) v = 104;
    return v;
}

// A host entry after its checks: in (n_in) and coef (ncol) go to the device, launch(in, coef, out) runs on the null stream and
// leaves nplanes blocks of n results back to back (cleared first when `clear`); block k comes back to out + k * ldout, so that
// the caller's words between the blocks keep their contents.  status(e) turns what the copies and the launch returned into
// the entry's status (staged_status: rc when all went well); a staging buffer that cannot be had is SPLPAK_E_NOMEM.
template <typename T, typename F, typename S>
static int32_t staged_call(const T *in, size_t n_in, const T *coef, size_t ncol, T *out, size_t n, int nplanes, long long ldout, bool clear,
                           F &&launch, S &&status)
{
    CallStage stage;
    T *din = nullptr, *dc = nullptr, *dout = nullptr;
    if (!stage.get(&din, n_in) || !stage.get(&dc, ncol) || !stage.get(&dout, n * (size_t)nplanes)) return SPLPAK_E_NOMEM;
    hipError_t e = hipMemcpy(din, in, sizeof(T) * n_in, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dc, coef, sizeof(T) * ncol, hipMemcpyHostToDevice);
    if (e == hipSuccess && clear) e = hipMemset(dout, 0, sizeof(T) * n * (size_t)nplanes);
    if (e == hipSuccess) e = launch((const T *)din, (const T *)dc, dout);
    for (int k = 0; k < nplanes && e == hipSuccess; ++k)
        e = hipMemcpy(out + (long long)k * ldout, dout + (size_t)k * n, sizeof(T) * n, hipMemcpyDeviceToHost);
    return status(e);
}

static auto staged_status(const char *what, int rc)
{
    return [=](hipError_t e) -> int32_t { return hip_ok(e, what) ? rc : SPLPAK_E_NODEVICE; };
}

// The results a failed ladder zeroes (101 / 102 / 103) before its entry returns: n in each of nplanes blocks ld apart, on the
// host or, `dev`, by memsets queued on st.
template <typename T>
static void zero_results(T *out, long long n, int nplanes, long long ld, bool dev, hipStream_t st)
{
    if (!out || n <= 0) return;
    for (int k = 0; k < nplanes; ++k) {
        T *p = out + (long long)k * ld;
        if (dev) (void)hipMemsetAsync(p, 0, sizeof(T) * (size_t)n, st);
        else for (long long i = 0; i < n; ++i) p[i] = (T)0;
    }
}

// the grid arguments every ladder starts with: the null checks, ndim in 1 .. MAXD, the limits widened to double.
// zero_101: how many outputs to zero on ndim < 1.  Only splpak_eval_dev_f64 and splpak_eval_derivs_dev_f64 (all of them: they
// took their 101 from the grid check, which zeroes) and the grid entries (the one output of the empty product) have ever done so.
template <typename T>
static bool grid_args(int32_t ndim, const T *xmin_t, const T *xmax_t, const int32_t *nodes, long long zero_101,
                      double (&xmin)[MAXD], double (&xmax)[MAXD], int &rc, long long &zero_n)
{
    zero_n = 0;
    if (!nodes || !xmin_t || !xmax_t) { set_error("null argument"); rc = SPLPAK_E_BADARG; return false; }
    if (ndim < 1) { rc = 101; zero_n = zero_101; return false; }
    if (ndim > MAXD) { rc = SPLPAK_E_UNSUPPORTED; return false; }
    for (int d = 0; d < ndim; ++d) { xmin[d] = (double)xmin_t[d]; xmax[d] = (double)xmax_t[d]; }
    return true;
}

// ---- evaluation at a list of points: one nderiv pattern (the value entries: ldout 1) or, `derivs`, value + gradient
// (+ Hessian) of order 1 / 2 (the derivative entries: no nderiv) ----
static int derivs_nout(int ndim, int order) { return 1 + ndim + (order == 2 ? ndim * (ndim + 1) / 2 : 0); }

// The checks of a point entry before it touches a device.  True: the caller goes on to compute and returns rc (0 or 104)
// afterwards; false: rc is the status to return and zero_n the outputs to zero first (102 / 103: all nq * ldout of them).
// A bad nderiv (104) does not end the ladder: the call is evaluated with the orders clamped, as splde's callers get it.
// The derivative entries check order, ldxq and ldout BEFORE they look at nq; the value entries look at ldxq only when
// there are queries, after the null checks.
template <typename T>
static bool point_validate(bool derivs, int32_t ndim, int64_t nq, const T *xq, int32_t ldxq, const int32_t *nderiv, int32_t order, const T *coef,
                           const T *xmin_t, const T *xmax_t, const int32_t *nodes, const T *out, int32_t ldout, bool zero_101, Grid &g,
                           int &rc, long long &zero_n)
{
    const long long nzero = ldout > 0 ? (long long)nq * ldout : 0;
    double xmin[MAXD], xmax[MAXD];
    if (!grid_args(ndim, xmin_t, xmax_t, nodes, zero_101 ? nzero : 0, xmin, xmax, rc, zero_n)) return false;
    rc = eval_validate(ndim, nderiv, xmin, xmax, nodes, g);
    if (rc != 0 && rc != 104) {
        if (rc > 0) zero_n = nzero;
        return false;
    }
    if (derivs) {
        if (order < 1 || order > 2) { set_error("order must be 1 (gradient) or 2 (gradient and Hessian)"); rc = SPLPAK_E_BADARG; return false; }
        if (ldxq < ndim || ldout < derivs_nout(ndim, order)) { set_error("ldxq or ldout too small"); rc = SPLPAK_E_BADARG; return false; }
    }
    if (nq <= 0) return false;
    if (!xq || !coef || !out) { set_error("null argument"); rc = SPLPAK_E_BADARG; return false; }
    if (ldxq < ndim) { set_error("ldxq smaller than ndim"); rc = SPLPAK_E_BADARG; return false; }
    if (int r = device_ready()) { rc = r; return false; }
    return true;
}

template <typename T>
static int32_t eval_dev(bool derivs, int32_t ndim, int64_t nq, const T *xq_dev, int32_t ldxq, const int32_t *nderiv, int32_t order, const T *coef_dev,
                        const T *xmin, const T *xmax, const int32_t *nodes, T *out_dev, int32_t ldout, void *stream, bool zero_101)
{
    Grid g;
    int rc = 0;
    long long zero_n = 0;
    if (!point_validate(derivs, ndim, nq, xq_dev, ldxq, nderiv, order, coef_dev, xmin, xmax, nodes, out_dev, ldout, zero_101, g, rc, zero_n)) {
        if (zero_n > 0 && out_dev) (void)hipMemsetAsync(out_dev, 0, sizeof(T) * (size_t)zero_n, (hipStream_t)stream);
        return rc;
    }
    SPLPAK_HIP_TRY(!derivs ? launch_eval<T>(g, nq, xq_dev, ldxq, nderiv, coef_dev, out_dev, (hipStream_t)stream)
                              : launch_eval_derivs<T>(g, nq, xq_dev, ldxq, order, coef_dev, out_dev, ldout, (hipStream_t)stream),
                   SPLPAK_E_NODEVICE);
    return rc;
}

template <typename T>
static int32_t eval_host(bool derivs, int32_t ndim, int64_t nq, const T *xq, int32_t ldxq, const int32_t *nderiv, int32_t order, const T *coef,
                         const T *xmin, const T *xmax, const int32_t *nodes, T *out, int32_t ldout)
{
    Grid g;
    int rc = 0;
    long long zero_n = 0;
    if (!point_validate(derivs, ndim, nq, xq, ldxq, nderiv, order, coef, xmin, xmax, nodes, out, ldout, /*zero_101=*/false, g, rc, zero_n)) {
        if (out) for (long long i = 0; i < zero_n; ++i) out[i] = (T)0;
        return rc;
    }
    return staged_call<T>(xq, (size_t)nq * ldxq, coef, (size_t)g.ncol, out, (size_t)nq * ldout, 1, 0, derivs,
                          [&](const T *dq, const T *dc, T *dout) {
                              return !derivs ? launch_eval<T>(g, nq, dq, ldxq, nderiv, dc, dout, nullptr)
                                                : launch_eval_derivs<T>(g, nq, dq, ldxq, order, dc, dout, ldout, nullptr);
                          },
                          staged_status("evaluation", rc));
}

extern "C" {

int32_t splpak_eval_f64(int32_t ndim, int64_t nq, const double *xq, int32_t ldxq, const int32_t *nderiv, const double *coef,
                        const double *xmin, const double *xmax, const int32_t *nodes, double *out)
{
    return eval_host<double>(false, ndim, nq, xq, ldxq, nderiv, 0, coef, xmin, xmax, nodes, out, 1);
}

int32_t splpak_eval_f32(int32_t ndim, int64_t nq, const float *xq, int32_t ldxq, const int32_t *nderiv, const float *coef,
                        const float *xmin, const float *xmax, const int32_t *nodes, float *out)
{
    return eval_host<float>(false, ndim, nq, xq, ldxq, nderiv, 0, coef, xmin, xmax, nodes, out, 1);
}

int32_t splpak_eval_dev_f64(int32_t ndim, int64_t nq, const double *xq_dev, int32_t ldxq, const int32_t *nderiv, const double *coef_dev,
                            const double *xmin, const double *xmax, const int32_t *nodes, double *out_dev, void *stream)
{
    return eval_dev<double>(false, ndim, nq, xq_dev, ldxq, nderiv, 0, coef_dev, xmin, xmax, nodes, out_dev, 1, stream, /*zero_101=*/true);
}

int32_t splpak_eval_dev_f32(int32_t ndim, int64_t nq, const float *xq_dev, int32_t ldxq, const int32_t *nderiv, const float *coef_dev,
                            const float *xmin, const float *xmax, const int32_t *nodes, float *out_dev, void *stream)
{
    return eval_dev<float>(false, ndim, nq, xq_dev, ldxq, nderiv, 0, coef_dev, xmin, xmax, nodes, out_dev, 1, stream, /*zero_101=*/false);
}

int32_t splpak_eval_derivs_f64(int32_t ndim, int64_t nq, const double *xq, int32_t ldxq, int32_t order, const double *coef,
                               const double *xmin, const double *xmax, const int32_t *nodes, double *out, int32_t ldout)
{
    return eval_host<double>(true, ndim, nq, xq, ldxq, nullptr, order, coef, xmin, xmax, nodes, out, ldout);
}

int32_t splpak_eval_derivs_f32(int32_t ndim, int64_t nq, const float *xq, int32_t ldxq, int32_t order, const float *coef,
                               const float *xmin, const float *xmax, const int32_t *nodes, float *out, int32_t ldout)
{
    return eval_host<float>(true, ndim, nq, xq, ldxq, nullptr, order, coef, xmin, xmax, nodes, out, ldout);
}

int32_t splpak_eval_derivs_dev_f64(int32_t ndim, int64_t nq, const double *xq_dev, int32_t ldxq, int32_t order, const double *coef_dev,
                                   const double *xmin, const double *xmax, const int32_t *nodes, double *out_dev, int32_t ldout,
                                   void *stream)
{
    return eval_dev<double>(true, ndim, nq, xq_dev, ldxq, nullptr, order, coef_dev, xmin, xmax, nodes, out_dev, ldout, stream, /*zero_101=*/true);
}

}  // extern "C"

// ---- several coefficient sets at the same points (eval.hip launch_eval_fields): field k's coefficients at coef + k*ldcoef,
// its nq results at out + k*ldout, one nderiv pattern for all ----
// The checks of a fields entry before it touches a device, in the order the header gives.  True: the caller goes on to compute and
// returns rc (0 or 104) afterwards; false: rc is the status to return and `zero` says whether the nq results of every field are
// zeroed first (101 / 102 / 103; the words between the fields stay as they are).
template <typename T>
static bool fields_validate(int32_t ndim, int64_t nq, const T *xq, int32_t ldxq, const int32_t *nderiv, int32_t nfields, const T *coef,
                            int64_t ldcoef, const T *xmin_t, const T *xmax_t, const int32_t *nodes, const T *out, int64_t ldout, Grid &g,
                            int &rc, bool &zero)
{
    zero = false;
    if (!nodes || !xmin_t || !xmax_t) { set_error("null argument"); rc = SPLPAK_E_BADARG; return false; }
    if (nfields < 1 || nq < 0 || ldout < nq) { set_error("nfields < 1, nq < 0 or ldout smaller than nq"); rc = SPLPAK_E_BADARG; return false; }
    double xmin[MAXD], xmax[MAXD];
    long long zero_n = 0;
    if (!grid_args(ndim, xmin_t, xmax_t, nodes, 1, xmin, xmax, rc, zero_n)) { zero = zero_n > 0; return false; }
    rc = eval_validate(ndim, nderiv, xmin, xmax, nodes, g);
    if (rc != 0 && rc != 104) {
        zero = rc > 0;
        return false;
    }
    if (ldxq < ndim || ldcoef < g.ncol) { set_error("ldxq smaller than ndim or ldcoef smaller than the number of coefficients"); rc = SPLPAK_E_BADARG; return false; }
    if (nq == 0) return false;
    if (!xq || !coef || !out) { set_error("null argument"); rc = SPLPAK_E_BADARG; return false; }
    if (int r = device_ready()) { rc = r; return false; }
    return true;
}

template <typename T>
static int32_t eval_fields_dev(int32_t ndim, int64_t nq, const T *xq_dev, int32_t ldxq, const int32_t *nderiv, int32_t nfields, const T *coef_dev,
                               int64_t ldcoef, const T *xmin, const T *xmax, const int32_t *nodes, T *out_dev, int64_t ldout, void *stream)
{
    Grid g;
    int rc = 0;
    bool zero = false;
    if (!fields_validate(ndim, nq, xq_dev, ldxq, nderiv, nfields, coef_dev, ldcoef, xmin, xmax, nodes, out_dev, ldout, g, rc, zero)) {
        if (zero) zero_results(out_dev, nq, nfields, ldout, true, (hipStream_t)stream);
        return rc;
    }
    SPLPAK_HIP_TRY(launch_eval_fields<T>(g, nq, xq_dev, ldxq, nderiv, nfields, coef_dev, ldcoef, out_dev, ldout, (hipStream_t)stream),
                   SPLPAK_E_NODEVICE);
    return rc;
}

// the host form: the coefficients of all fields go to the device with the caller's ldcoef in one copy, the results are packed
// there (nq apart) and come back field by field
template <typename T>
static int32_t eval_fields_host(int32_t ndim, int64_t nq, const T *xq, int32_t ldxq, const int32_t *nderiv, int32_t nfields, const T *coef,
                                int64_t ldcoef, const T *xmin, const T *xmax, const int32_t *nodes, T *out, int64_t ldout)
{
    Grid g;
    int rc = 0;
    bool zero = false;
    if (!fields_validate(ndim, nq, xq, ldxq, nderiv, nfields, coef, ldcoef, xmin, xmax, nodes, out, ldout, g, rc, zero)) {
        if (zero) zero_results(out, nq, nfields, ldout, false, nullptr);
        return rc;
    }
    return staged_call<T>(xq, (size_t)nq * ldxq, coef, coef_block_len(nfields, ldcoef, g.ncol), out, (size_t)nq, nfields, ldout, false,
                          [&](const T *dq, const T *dc, T *dout) {
                              return launch_eval_fields<T>(g, nq, dq, ldxq, nderiv, nfields, dc, ldcoef, dout, nq, nullptr);
                          },
                          staged_status("evaluation of several fields", rc));
}

extern "C" {

int32_t splpak_eval_fields_f64(int32_t ndim, int64_t nq, const double *xq, int32_t ldxq, const int32_t *nderiv, int32_t nfields,
                               const double *coef, int64_t ldcoef, const double *xmin, const double *xmax, const int32_t *nodes,
                               double *out, int64_t ldout)
{
    return eval_fields_host<double>(ndim, nq, xq, ldxq, nderiv, nfields, coef, ldcoef, xmin, xmax, nodes, out, ldout);
}

int32_t splpak_eval_fields_f32(int32_t ndim, int64_t nq, const float *xq, int32_t ldxq, const int32_t *nderiv, int32_t nfields,
                               const float *coef, int64_t ldcoef, const float *xmin, const float *xmax, const int32_t *nodes,
                               float *out, int64_t ldout)
{
    return eval_fields_host<float>(ndim, nq, xq, ldxq, nderiv, nfields, coef, ldcoef, xmin, xmax, nodes, out, ldout);
}

int32_t splpak_eval_fields_dev_f64(int32_t ndim, int64_t nq, const double *xq_dev, int32_t ldxq, const int32_t *nderiv, int32_t nfields,
                                   const double *coef_dev, int64_t ldcoef, const double *xmin, const double *xmax, const int32_t *nodes,
                                   double *out_dev, int64_t ldout, void *stream)
{
    return eval_fields_dev<double>(ndim, nq, xq_dev, ldxq, nderiv, nfields, coef_dev, ldcoef, xmin, xmax, nodes, out_dev, ldout, stream);
}

int32_t splpak_eval_fields_dev_f32(int32_t ndim, int64_t nq, const float *xq_dev, int32_t ldxq, const int32_t *nderiv, int32_t nfields,
                                   const float *coef_dev, int64_t ldcoef, const float *xmin, const float *xmax, const int32_t *nodes,
                                   float *out_dev, int64_t ldout, void *stream)
{
    return eval_fields_dev<float>(ndim, nq, xq_dev, ldxq, nderiv, nfields, coef_dev, ldcoef, xmin, xmax, nodes, out_dev, ldout, stream);
}

// host-side counters of the calling thread's last fields call (no device is asked)
int32_t splpak_debug_eval_fields_stats(int64_t out3[3])
{
    if (!out3) { set_error("null argument"); return SPLPAK_E_BADARG; }
    long long v[3];
    eval_fields_stats(v);
    for (int j = 0; j < 3; ++j) out3[j] = v[j];
    return 0;
}

}  // extern "C"

// ---- evaluation on a tensor-product grid of points (evalgrid.hip) ----
// outputs and table entries of a grid call; false: a negative count or a product beyond int64
static bool grid_counts(int32_t ndim, const int64_t *npts, long long &nout, long long &ntab)
{
    nout = 1;
    ntab = 0;
    bool zero = false;
    for (int d = 0; d < ndim; ++d) {
        if (npts[d] < 0) return false;
        zero = zero || npts[d] == 0;
        if (__builtin_add_overflow(ntab, (long long)npts[d], &ntab)) return false;
    }
    if (zero) { nout = 0; return true; }
    for (int d = 0; d < ndim; ++d)
        if (__builtin_mul_overflow(nout, (long long)npts[d], &nout)) return false;
    return true;
}

// What the ladder of a grid family (grid_validate, integrate_validate, grid_derivs_validate) leaves to its entries.  Every
// ladder is grid_open, the family's own checks, grid_close, in the order of eval_host / splpak_eval_dev_f64.
struct GridCheck {
    Grid g;
    double xmin[MAXD], xmax[MAXD];
    long long nout = 0;         // results (of one plane)
    long long ntab = 0;         // axis entries
    int rc = 0;                 // the status to return when the ladder ends the call; 0 or 104 when the entry goes on to compute
    long long zero_n = 0;       // results to zero first (101: the empty product, one output; 102 / 103: all of them) ..
    int zero_planes = 1;        // .. in that many planes
};

// The opening: the null checks, ndim, the limits widened, the counts.  bad_counts: the family's text for a negative count
// or a product beyond int64.
template <typename T>
static bool grid_open(int32_t ndim, const int64_t *counts, const T *xmin_t, const T *xmax_t, const int32_t *nodes, const T *out,
                      const char *bad_counts, GridCheck &c)
{
    if (!counts) { set_error("null argument"); c.rc = SPLPAK_E_BADARG; return false; }
    if (!grid_args(ndim, xmin_t, xmax_t, nodes, out ? 1 : 0, c.xmin, c.xmax, c.rc, c.zero_n)) return false;
    if (!grid_counts(ndim, counts, c.nout, c.ntab)) { set_error(bad_counts); c.rc = SPLPAK_E_BADARG; return false; }
    return true;
}

// The close: 102 / 103 (the results of all `planes` planes are zeroed) and 104 (which does not end the ladder), the empty
// product, the data pointers, the device.  True: the entry goes on to compute.
template <typename T>
static bool grid_close(int32_t ndim, const int32_t *nderiv, const int32_t *nodes, const T *axes, const T *coef, const T *out, int planes,
                       GridCheck &c)
{
    c.rc = eval_validate(ndim, nderiv, c.xmin, c.xmax, nodes, c.g);
    if (c.rc != 0 && c.rc != 104) {
        if (c.rc > 0 && out) { c.zero_n = c.nout; c.zero_planes = planes; }
        return false;
    }
    if (c.nout == 0) return false;
    if (!axes || !coef || !out) { set_error("null argument"); c.rc = SPLPAK_E_BADARG; return false; }
    if (int r = device_ready()) { c.rc = r; return false; }
    return true;
}

template <typename T>
static bool grid_validate(int32_t ndim, const int64_t *npts, const T *axes, const int32_t *nderiv, const T *coef,
                          const T *xmin, const T *xmax, const int32_t *nodes, const T *out, GridCheck &c)
{
    return grid_open(ndim, npts, xmin, xmax, nodes, out, "negative npts, or an output count beyond int64", c) &&
           grid_close(ndim, nderiv, nodes, axes, coef, out, 1, c);
}

template <typename T>
static int32_t eval_grid_dev(int32_t ndim, const int64_t *npts, const T *axes_dev, const int32_t *nderiv, const T *coef_dev,
                             const T *xmin, const T *xmax, const int32_t *nodes, T *out_dev, void *stream)
{
    GridCheck c;
    if (!grid_validate(ndim, npts, axes_dev, nderiv, coef_dev, xmin, xmax, nodes, out_dev, c)) {
        zero_results(out_dev, c.zero_n, 1, 0, true, (hipStream_t)stream);
        return c.rc;
    }
    SPLPAK_HIP_TRY(launch_eval_grid<T>(c.g, npts, axes_dev, nderiv, coef_dev, out_dev, (hipStream_t)stream), SPLPAK_E_NODEVICE);
    return c.rc;
}

template <typename T>
static int32_t eval_grid_host(int32_t ndim, const int64_t *npts, const T *axes, const int32_t *nderiv, const T *coef,
                              const T *xmin, const T *xmax, const int32_t *nodes, T *out)
{
    GridCheck c;
    if (!grid_validate(ndim, npts, axes, nderiv, coef, xmin, xmax, nodes, out, c)) {
        zero_results(out, c.zero_n, 1, 0, false, nullptr);
        return c.rc;
    }
    return staged_call<T>(axes, (size_t)c.ntab, coef, (size_t)c.g.ncol, out, (size_t)c.nout, 1, 0, false,
                          [&](const T *da, const T *dc, T *dout) { return launch_eval_grid<T>(c.g, npts, da, nderiv, dc, dout, nullptr); },
                          staged_status("grid evaluation", c.rc));
}

extern "C" {

int32_t splpak_eval_grid_f64(int32_t ndim, const int64_t *npts, const double *axes, const int32_t *nderiv,
                             const double *coef, const double *xmin, const double *xmax, const int32_t *nodes, double *out)
{
    return eval_grid_host<double>(ndim, npts, axes, nderiv, coef, xmin, xmax, nodes, out);
}

int32_t splpak_eval_grid_f32(int32_t ndim, const int64_t *npts, const float *axes, const int32_t *nderiv,
                             const float *coef, const float *xmin, const float *xmax, const int32_t *nodes, float *out)
{
    return eval_grid_host<float>(ndim, npts, axes, nderiv, coef, xmin, xmax, nodes, out);
}

int32_t splpak_eval_grid_dev_f64(int32_t ndim, const int64_t *npts, const double *axes_dev, const int32_t *nderiv,
                                 const double *coef_dev, const double *xmin, const double *xmax, const int32_t *nodes,
                                 double *out_dev, void *stream)
{
    return eval_grid_dev<double>(ndim, npts, axes_dev, nderiv, coef_dev, xmin, xmax, nodes, out_dev, stream);
}

int32_t splpak_eval_grid_dev_f32(int32_t ndim, const int64_t *npts, const float *axes_dev, const int32_t *nderiv,
                                 const float *coef_dev, const float *xmin, const float *xmax, const int32_t *nodes,
                                 float *out_dev, void *stream)
{
    return eval_grid_dev<float>(ndim, npts, axes_dev, nderiv, coef_dev, xmin, xmax, nodes, out_dev, stream);
}

int64_t splpak_eval_grid_scratch_bytes(int32_t ndim, const int64_t *npts)
{
    long long nout = 0, ntab = 0;
    if (!npts || ndim < 1 || ndim > MAXD || !grid_counts(ndim, npts, nout, ntab)) { set_error("bad grid shape"); return SPLPAK_E_BADARG; }
    return nout == 0 ? 0 : eval_grid_scratch_bytes(ntab);
}

int32_t splpak_debug_eval_grid_stats(int64_t out2[2])
{
    if (!out2) { set_error("null argument"); return SPLPAK_E_BADARG; }
    out2[0] = out2[1] = 0;
    if (int r = device_ready()) return r;
    long long v[2];
    SPLPAK_HIP_TRY(eval_grid_stats(v), SPLPAK_E_NODEVICE);
    out2[0] = v[0];
    out2[1] = v[1];
    return 0;
}

}  // extern "C"

// ---- integrals over the cells of a tensor grid (integrategrid.hip) ----
// The ladder of grid_validate with ncell in place of npts and the mode check beside the count check; no nderiv, hence no 104.
// c.ntab: the axis entries (ncell[d] + 1 edges of an integrated dimension, ncell[d] coordinates of an evaluated one).
template <typename T>
static bool integrate_validate(int32_t ndim, const int64_t *ncell, const int32_t *mode, const T *axes, const T *coef, const T *xmin,
                               const T *xmax, const int32_t *nodes, const T *out, GridCheck &c)
{
    const char *bad = "negative ncell, a mode outside 0 and 1, or an output count beyond int64";
    if (!grid_open(ndim, ncell, xmin, xmax, nodes, out, bad, c)) return false;
    for (int d = 0; d < ndim; ++d) {
        const int m = mode ? mode[d] : 1;
        if ((m != 0 && m != 1) || __builtin_add_overflow(c.ntab, (long long)m, &c.ntab)) { set_error(bad); c.rc = SPLPAK_E_BADARG; return false; }
    }
    return grid_close(ndim, nullptr, nodes, axes, coef, out, 1, c);
}

static int32_t integrate_status(hipError_t e)
{
    if (e == hipSuccess) return 0;
    (void)hip_ok(e, "integration on a grid");
    return e == hipErrorOutOfMemory ? SPLPAK_E_NOMEM : SPLPAK_E_NODEVICE;
}

template <typename T>
static int32_t integrate_grid_dev(int32_t ndim, const int64_t *ncell, const int32_t *mode, const T *axes_dev, const T *coef_dev,
                                  const T *xmin, const T *xmax, const int32_t *nodes, T *out_dev, void *stream)
{
    GridCheck c;
    if (!integrate_validate(ndim, ncell, mode, axes_dev, coef_dev, xmin, xmax, nodes, out_dev, c)) {
        zero_results(out_dev, c.zero_n, 1, 0, true, (hipStream_t)stream);
        return c.rc;
    }
    return integrate_status(launch_integrate_grid<T>(c.g, ncell, mode, axes_dev, coef_dev, out_dev, (hipStream_t)stream));
}

template <typename T>
static int32_t integrate_grid_host(int32_t ndim, const int64_t *ncell, const int32_t *mode, const T *axes, const T *coef,
                                   const T *xmin, const T *xmax, const int32_t *nodes, T *out)
{
    GridCheck c;
    if (!integrate_validate(ndim, ncell, mode, axes, coef, xmin, xmax, nodes, out, c)) {
        zero_results(out, c.zero_n, 1, 0, false, nullptr);
        return c.rc;
    }
    return staged_call<T>(axes, (size_t)c.ntab, coef, (size_t)c.g.ncol, out, (size_t)c.nout, 1, 0, false,
                          [&](const T *da, const T *dc, T *dout) { return launch_integrate_grid<T>(c.g, ncell, mode, da, dc, dout, nullptr); },
                          integrate_status);
}

extern "C" {

int32_t splpak_integrate_grid_f64(int32_t ndim, const int64_t *ncell, const int32_t *mode, const double *axes, const double *coef,
                                  const double *xmin, const double *xmax, const int32_t *nodes, double *out)
{
    return integrate_grid_host<double>(ndim, ncell, mode, axes, coef, xmin, xmax, nodes, out);
}

int32_t splpak_integrate_grid_f32(int32_t ndim, const int64_t *ncell, const int32_t *mode, const float *axes, const float *coef,
                                  const float *xmin, const float *xmax, const int32_t *nodes, float *out)
{
    return integrate_grid_host<float>(ndim, ncell, mode, axes, coef, xmin, xmax, nodes, out);
}

int32_t splpak_integrate_grid_dev_f64(int32_t ndim, const int64_t *ncell, const int32_t *mode, const double *axes_dev,
                                      const double *coef_dev, const double *xmin, const double *xmax, const int32_t *nodes,
                                      double *out_dev, void *stream)
{
    return integrate_grid_dev<double>(ndim, ncell, mode, axes_dev, coef_dev, xmin, xmax, nodes, out_dev, stream);
}

int32_t splpak_integrate_grid_dev_f32(int32_t ndim, const int64_t *ncell, const int32_t *mode, const float *axes_dev,
                                      const float *coef_dev, const float *xmin, const float *xmax, const int32_t *nodes,
                                      float *out_dev, void *stream)
{
    return integrate_grid_dev<float>(ndim, ncell, mode, axes_dev, coef_dev, xmin, xmax, nodes, out_dev, stream);
}

// host-side counters of the calling thread's last integrate call (no device is asked, nothing is waited for)
int32_t splpak_debug_integrate_grid_stats(int64_t out8[8])
{
    if (!out8) { set_error("null argument"); return SPLPAK_E_BADARG; }
    long long v[8];
    integrate_grid_stats(v);
    for (int j = 0; j < 8; ++j) out8[j] = v[j];
    return 0;
}

}  // extern "C"

// ---- value, gradient and Hessian planes on a tensor-product grid of points (evalgridderivs.hip) ----
// The checks of a grid-derivatives entry before it touches a device: the ladder of grid_validate with the order and ldout
// checks between the shape and the 102 / 103 checks.  True: the caller goes on to compute; false: c.rc is the status to
// return, and c.zero_n results are zeroed first -- of out[0] alone (101) or of every plane (102 / 103).
template <typename T>
static bool grid_derivs_validate(int32_t ndim, const int64_t *npts, const T *axes, int32_t order, const T *coef, const T *xmin,
                                 const T *xmax, const int32_t *nodes, const T *out, int64_t ldout, GridCheck &c)
{
    if (!grid_open(ndim, npts, xmin, xmax, nodes, out, "negative npts, or an output count beyond int64", c)) return false;
    if (order < 1 || order > 2) { set_error("order must be 1 (gradient) or 2 (gradient and Hessian)"); c.rc = SPLPAK_E_BADARG; return false; }
    long long total = 0;
    if (ldout < c.nout || __builtin_mul_overflow((long long)derivs_nout(ndim, order), (long long)ldout, &total)) {
        set_error("ldout smaller than the number of grid points, or the planes beyond int64");
        c.rc = SPLPAK_E_BADARG;
        return false;
    }
    return grid_close(ndim, nullptr, nodes, axes, coef, out, derivs_nout(ndim, order), c);
}

template <typename T>
static int32_t eval_grid_derivs_dev(int32_t ndim, const int64_t *npts, const T *axes_dev, int32_t order, const T *coef_dev, const T *xmin,
                                    const T *xmax, const int32_t *nodes, T *out_dev, int64_t ldout, void *stream)
{
    GridCheck c;
    if (!grid_derivs_validate(ndim, npts, axes_dev, order, coef_dev, xmin, xmax, nodes, out_dev, ldout, c)) {
        zero_results(out_dev, c.zero_n, c.zero_planes, ldout, true, (hipStream_t)stream);
        return c.rc;
    }
    SPLPAK_HIP_TRY(launch_eval_grid_derivs<T>(c.g, npts, axes_dev, order, coef_dev, out_dev, ldout, (hipStream_t)stream), SPLPAK_E_NODEVICE);
    return c.rc;
}

// the host form: the planes are packed on the device (prod npts apart) and come back one by one
template <typename T>
static int32_t eval_grid_derivs_host(int32_t ndim, const int64_t *npts, const T *axes, int32_t order, const T *coef, const T *xmin,
                                     const T *xmax, const int32_t *nodes, T *out, int64_t ldout)
{
    GridCheck c;
    if (!grid_derivs_validate(ndim, npts, axes, order, coef, xmin, xmax, nodes, out, ldout, c)) {
        zero_results(out, c.zero_n, c.zero_planes, ldout, false, nullptr);
        return c.rc;
    }
    return staged_call<T>(axes, (size_t)c.ntab, coef, (size_t)c.g.ncol, out, (size_t)c.nout, derivs_nout(ndim, order), ldout, false,
                          [&](const T *da, const T *dc, T *dout) { return launch_eval_grid_derivs<T>(c.g, npts, da, order, dc, dout, c.nout, nullptr); },
                          staged_status("grid evaluation of derivatives", c.rc));
}

extern "C" {

int32_t splpak_eval_grid_derivs_f64(int32_t ndim, const int64_t *npts, const double *axes, int32_t order, const double *coef,
                                    const double *xmin, const double *xmax, const int32_t *nodes, double *out, int64_t ldout)
{
    return eval_grid_derivs_host<double>(ndim, npts, axes, order, coef, xmin, xmax, nodes, out, ldout);
}

int32_t splpak_eval_grid_derivs_f32(int32_t ndim, const int64_t *npts, const float *axes, int32_t order, const float *coef,
                                    const float *xmin, const float *xmax, const int32_t *nodes, float *out, int64_t ldout)
{
    return eval_grid_derivs_host<float>(ndim, npts, axes, order, coef, xmin, xmax, nodes, out, ldout);
}

int32_t splpak_eval_grid_derivs_dev_f64(int32_t ndim, const int64_t *npts, const double *axes_dev, int32_t order, const double *coef_dev,
                                        const double *xmin, const double *xmax, const int32_t *nodes, double *out_dev, int64_t ldout,
                                        void *stream)
{
    return eval_grid_derivs_dev<double>(ndim, npts, axes_dev, order, coef_dev, xmin, xmax, nodes, out_dev, ldout, stream);
}

int32_t splpak_eval_grid_derivs_dev_f32(int32_t ndim, const int64_t *npts, const float *axes_dev, int32_t order, const float *coef_dev,
                                        const float *xmin, const float *xmax, const int32_t *nodes, float *out_dev, int64_t ldout,
                                        void *stream)
{
    return eval_grid_derivs_dev<float>(ndim, npts, axes_dev, order, coef_dev, xmin, xmax, nodes, out_dev, ldout, stream);
}

int64_t splpak_eval_grid_derivs_scratch_bytes(int32_t ndim, const int64_t *npts, int32_t order)
{
    long long nout = 0, ntab = 0;
    if (!npts || ndim < 1 || ndim > MAXD || order < 1 || order > 2 || !grid_counts(ndim, npts, nout, ntab)) {
        set_error("bad grid shape or order");
        return SPLPAK_E_BADARG;
    }
    return nout == 0 ? 0 : eval_grid_derivs_scratch_bytes(ntab, order);
}

// host only
int32_t splpak_debug_eval_grid_derivs_tile(int32_t ndim, int32_t order, int32_t out4[4])
{
    int t[4];
    if (!out4 || !eval_grid_derivs_tile(ndim, order, t)) { set_error("bad ndim, order or pointer"); return SPLPAK_E_BADARG; }
    for (int d = 0; d < 4; ++d) out4[d] = t[d];
    return 0;
}

int32_t splpak_synth_points_f64(int32_t ndim, int64_t first_point, int64_t ndata, double *xdata_dev,
                                double *ydata_dev, double *wdata_dev, void *stream)
{
    if (ndim < 1 || ndim > MAXD) return SPLPAK_E_UNSUPPORTED;
    if (int r = device_ready()) return r;
    SPLPAK_HIP_TRY(launch_synth_points(ndim, first_point, ndata, xdata_dev, ydata_dev, wdata_dev, (hipStream_t)stream), SPLPAK_E_NODEVICE);
    return 0;
}

int32_t splpak_synth_queries_f64(int32_t ndim, int64_t ndata_before, int64_t first_query, int64_t nq,
                                 double *xq_dev, void *stream)
{
    if (ndim < 1 || ndim > MAXD) return SPLPAK_E_UNSUPPORTED;
    if (int r = device_ready()) return r;
    const long long skip = (long long)ndata_before * (ndim + 2) + (long long)first_query * ndim;
    SPLPAK_HIP_TRY(launch_synth_queries(ndim, skip, nq, xq_dev, (hipStream_t)stream), SPLPAK_E_NODEVICE);
    return 0;
}

int32_t splpak_set_eval_mode(int32_t mode, int64_t chunk)
{
    if (mode < 0 || mode > 2 || chunk < 0) { set_error("bad evaluation mode"); return SPLPAK_E_BADARG; }
    set_eval_mode(mode, chunk);
    return 0;
}

// host only: the 4-entry value table of a 1-D grid at n points, as the evaluation kernels select it and in the general form
int32_t splpak_debug_window_values(int32_t nodes, double xmin, double xmax, int64_t n, const double *x, int32_t *ws_out,
                                   double *used4, double *general4, int32_t *form_out)
{
    if (!x || !ws_out || !used4 || !general4 || !form_out || n < 0) { set_error("null argument"); return SPLPAK_E_BADARG; }
    Grid g;
    const int v = build_grid(1, &nodes, &xmin, &xmax, g, nullptr);
    if (v != 0) return v;
    for (int64_t i = 0; i < n; ++i) {
        int form = 0;
        ws_out[i] = window_table_selected(g, 0, x[i], used4 + 4 * i, form);
        form_out[i] = form;
        const int wg = window_table_value(g, 0, x[i], general4 + 4 * i);
        if (wg != ws_out[i]) { set_error("window starts of the two forms differ"); return SPLPAK_E_BADARG; }
    }
    return 0;
}

}  // extern "C"
