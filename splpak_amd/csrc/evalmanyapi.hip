// The entries of the batch evaluation at each problem's own points (include/splpak_hip.h): splpak_eval_many_*,
// splpak_eval_many_var_* (the prediction variance from the stencils of splpak_fit_many_cov_*),
// splpak_residuals_many_* and splpak_mad_many_* (madmany.hip) on host and device pointers, and their counters.  Each family has one ladder of checks, in the order
// the header gives, all on the host; then evalmany.hip.  The _dev entries only enqueue: the one thing they upload is the
// offsets, into the calling thread's scratch (manyhost.hpp: many_offsets_upload, held by a ScratchUse to the end of the
// call).  The host entries stage the span of the batch's points and (nbatch-1)*ldcoef + ncol coefficients through device
// memory of the call (manyhost.hpp: stage_span, stage_copy).
#include "plan.hpp"
#include "evalcore.hpp"
#include "evalmany.hpp"
#include "manyhost.hpp"

#include <vector>

using namespace splpak;

namespace {

// The rungs both ladders open with.  True: the grid is built (rc = 0); false: rc is the status, and `zero` says whether it is
// one of 101 / 102 / 103 (eval_many zeroes its results on these).  maxdim: the dimensions the family takes.
template <typename T>
bool many_open(int32_t ndim, int32_t nbatch, const int64_t *offsets, const T *xmin_t, const T *xmax_t, const int32_t *nodes, Grid &g, int &rc,
               bool &zero, int maxdim = MAXD)
{
    zero = false;
    if (!offsets || !nodes || !xmin_t || !xmax_t) { set_error("null argument"); rc = SPLPAK_E_BADARG; return false; }
    bool ok = nbatch >= 1;
    for (int k = 0; ok && k < nbatch; ++k) ok = offsets[k + 1] >= offsets[k];
    if (!ok) { set_error("nbatch < 1 or offsets that decrease"); rc = SPLPAK_E_BADARG; return false; }
    if (ndim < 1) { rc = 101; zero = true; return false; }
    if (ndim > maxdim) {
        set_error(maxdim == MAXD ? "more than 4 dimensions are not supported" : "splpak_eval_many_var_* takes 1-D and 2-D grids, as splpak_fit_many_cov_*");
        rc = SPLPAK_E_UNSUPPORTED;
        return false;
    }
    double xmin[MAXD], xmax[MAXD];
    for (int d = 0; d < ndim; ++d) { xmin[d] = (double)xmin_t[d]; xmax[d] = (double)xmax_t[d]; }
    rc = build_grid(ndim, nodes, xmin, xmax, g, nullptr);      // 102, 103
    if (rc != 0) {
        zero = rc > 0;
        if (rc == SPLPAK_E_UNSUPPORTED) set_error("more than 2^30 nodes is not supported");
        return false;
    }
    return true;
}

void many_counters(int family, long long npoints, int nbatch)
{
    t_eval_many_stats[2] = npoints;
    t_eval_many_stats[3] = nbatch;
    t_eval_many_stats[5] = family;
}

// ---- splpak_eval_many_* ----
template <typename T>
int32_t eval_many_entry(bool dev, int32_t ndim, int32_t nbatch, const int64_t *offsets, const T *xq, int32_t ldxq, const int32_t *nderiv,
                        const T *coef, int64_t ldcoef, const T *xmin, const T *xmax, const int32_t *nodes, T *out, hipStream_t st)
{
    for (int j = 0; j < 8; ++j) t_eval_many_stats[j] = 0;
    Grid g;
    int rc = 0;
    bool zero = false;
    if (!many_open(ndim, nbatch, offsets, xmin, xmax, nodes, g, rc, zero)) {
        if (zero && out) {
            const ManySpan sp = many_span(offsets, nbatch);
            if (dev) { if (sp.n > 0) (void)hipMemsetAsync(out + sp.lo, 0, sizeof(T) * (size_t)sp.n, st); }
            else for (long long i = 0; i < sp.n; ++i) out[sp.lo + i] = (T)0;
        }
        return rc;
    }
    if (ldxq < ndim || ldcoef < g.ncol) { set_error("ldxq smaller than ndim or ldcoef smaller than the number of coefficients"); return SPLPAK_E_BADARG; }
    if (nderiv)
        for (int d = 0; d < ndim; ++d)
            if (nderiv[d] < 0 || nderiv[d] > 2) rc = 104;      // reported; evaluated with the orders clamped
    const ManySpan sp = many_span(offsets, nbatch);
    const long long lo = sp.lo, nq = sp.n;
    many_counters(1, nq, nbatch);
    if (nq == 0) return rc;
    if (!xq || !coef || !out) { set_error("null argument"); return SPLPAK_E_BADARG; }
    if (int r = device_ready()) return r;

    const char *what = "evaluation of a batch of fits";
    const ScratchUse<1> use{t_many_offsets, st};
    const long long *off_dev = nullptr;
    if (dev) {
        hipError_t e = many_offsets_upload(offsets, nbatch, st, &off_dev);
        if (e == hipSuccess) e = launch_eval_many<T>(g, nbatch, off_dev, lo, nq, 0, xq, ldxq, nderiv, coef, ldcoef, out, st);
        return many_status(e, what, rc);
    }
    // the host form: the span of the batch's queries alone, the coefficient sets with the caller's ldcoef in one copy
    std::vector<T> res((size_t)nq);
    CallStage cs;
    const T *xs = nullptr, *cd = nullptr;
    T *od = nullptr;
    hipError_t e = stage_span<T>(cs, sp, xq, ldxq, nullptr, nullptr, &xs, nullptr, nullptr);
    if (e == hipSuccess) e = stage_copy(cs, coef, coef_block_len(nbatch, ldcoef, g.ncol), &cd);
    if (e == hipSuccess && !cs.get(&od, (size_t)nq)) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = many_offsets_upload(offsets, nbatch, nullptr, &off_dev);
    if (e == hipSuccess) e = launch_eval_many<T>(g, nbatch, off_dev, lo, nq, lo, xs, ldxq, nderiv, cd, ldcoef, od, nullptr);
    if (e == hipSuccess) e = hipMemcpy(res.data(), od, sizeof(T) * (size_t)nq, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        for (long long i = 0; i < nq; ++i) out[lo + i] = res[(size_t)i];
    return many_status(e, what, rc);
}

// ---- splpak_eval_many_var_* ----
// eval_many_entry with the half stencils of splpak_fit_many_cov_* in the place of the coefficients
template <typename T>
int32_t eval_many_var_entry(bool dev, int32_t ndim, int32_t nbatch, const int64_t *offsets, const T *xq, int32_t ldxq, const int32_t *nderiv,
                            const T *cov, int64_t ldcov, const T *xmin, const T *xmax, const int32_t *nodes, T *out, hipStream_t st)
{
    for (int j = 0; j < 8; ++j) t_eval_many_stats[j] = 0;
    Grid g;
    int rc = 0;
    bool zero = false;
    if (!many_open(ndim, nbatch, offsets, xmin, xmax, nodes, g, rc, zero, 2)) {
        if (zero && out) {
            const ManySpan sp = many_span(offsets, nbatch);
            if (dev) { if (sp.n > 0) (void)hipMemsetAsync(out + sp.lo, 0, sizeof(T) * (size_t)sp.n, st); }
            else for (long long i = 0; i < sp.n; ++i) out[sp.lo + i] = (T)0;
        }
        return rc;
    }
    const long long len = (long long)g.ncol * g.hstencil;
    if (ldxq < ndim || ldcov < len) { set_error("ldxq smaller than ndim or ldcov smaller than splpak_fit_many_cov_len"); return SPLPAK_E_BADARG; }
    if (nderiv)
        for (int d = 0; d < ndim; ++d)
            if (nderiv[d] < 0 || nderiv[d] > 2) rc = 104;      // reported; evaluated with the orders clamped
    const ManySpan sp = many_span(offsets, nbatch);
    const long long lo = sp.lo, nq = sp.n;
    many_counters(3, nq, nbatch);
    if (nq == 0) return rc;
    if (!xq || !cov || !out) { set_error("null argument"); return SPLPAK_E_BADARG; }
    if (int r = device_ready()) return r;

    const char *what = "prediction variance of a batch of fits";
    const ScratchUse<1> use{t_many_offsets, st};
    const long long *off_dev = nullptr;
    if (dev) {
        hipError_t e = many_offsets_upload(offsets, nbatch, st, &off_dev);
        if (e == hipSuccess) e = launch_eval_many_var<T>(g, nbatch, off_dev, lo, nq, 0, xq, ldxq, nderiv, cov, ldcov, out, st);
        return many_status(e, what, rc);
    }
    std::vector<T> res((size_t)nq);
    CallStage cs;
    const T *xs = nullptr, *cd = nullptr;
    T *od = nullptr;
    hipError_t e = stage_span<T>(cs, sp, xq, ldxq, nullptr, nullptr, &xs, nullptr, nullptr);
    if (e == hipSuccess) e = stage_copy(cs, cov, coef_block_len(nbatch, ldcov, len), &cd);
    if (e == hipSuccess && !cs.get(&od, (size_t)nq)) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = many_offsets_upload(offsets, nbatch, nullptr, &off_dev);
    if (e == hipSuccess) e = launch_eval_many_var<T>(g, nbatch, off_dev, lo, nq, lo, xs, ldxq, nderiv, cd, ldcov, od, nullptr);
    if (e == hipSuccess) e = hipMemcpy(res.data(), od, sizeof(T) * (size_t)nq, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        for (long long i = 0; i < nq; ++i) out[lo + i] = res[(size_t)i];
    return many_status(e, what, rc);
}

// ---- splpak_residuals_many_* ----
template <typename T>
int32_t residuals_many_entry(bool dev, int32_t ndim, int32_t nbatch, const int64_t *offsets, const T *xdata, int32_t l1xdat, const T *ydata,
                             const T *wdata, const T *coef, int64_t ldcoef, const T *xmin, const T *xmax, const int32_t *nodes, T *resid,
                             double *stats, hipStream_t st)
{
    for (int j = 0; j < 8; ++j) t_eval_many_stats[j] = 0;
    Grid g;
    int rc = 0;
    bool zero = false;
    if (!many_open(ndim, nbatch, offsets, xmin, xmax, nodes, g, rc, zero)) return rc;
    if (ldcoef < g.ncol) return 104;
    if (l1xdat < ndim || !xdata || !ydata || !coef || (!resid && !stats)) {
        set_error("l1xdat < ndim, a null pointer, or resid and stats both null");
        return SPLPAK_E_BADARG;
    }
    const ManySpan sp = many_span(offsets, nbatch);
    const long long lo = sp.lo, npt = sp.n;
    many_counters(2, npt, nbatch);
    if (npt == 0 && !dev) {      // nothing for a device to do
        if (stats)
            for (int k = 0; k < nbatch; ++k) { stats[4 * (size_t)k] = stats[4 * (size_t)k + 1] = stats[4 * (size_t)k + 2] = 0.0; stats[4 * (size_t)k + 3] = -1.0; }
        return 0;
    }
    if (npt == 0 && !stats) return 0;
    if (int r = device_ready()) return r;

    const char *what = "residuals of a batch of fits";
    const ScratchUse<1> use{t_many_offsets, st};
    const long long *off_dev = nullptr;
    if (dev) {
        hipError_t e = many_offsets_upload(offsets, nbatch, st, &off_dev);
        if (e == hipSuccess) e = launch_residuals_many<T>(g, nbatch, off_dev, 0, xdata, l1xdat, ydata, wdata, coef, ldcoef, resid, stats, st);
        return many_status(e, what, 0);
    }
    std::vector<T> res(resid ? (size_t)npt : 0);
    CallStage cs;
    const T *xs = nullptr, *ys = nullptr, *wsd = nullptr, *cd = nullptr;
    T *rd = nullptr;
    double *sd = nullptr;
    hipError_t e = stage_span(cs, sp, xdata, l1xdat, ydata, wdata, &xs, &ys, &wsd);
    if (e == hipSuccess) e = stage_copy(cs, coef, coef_block_len(nbatch, ldcoef, g.ncol), &cd);
    if (e == hipSuccess && ((resid && !cs.get(&rd, (size_t)npt)) || (stats && !cs.get(&sd, 4 * (size_t)nbatch)))) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = many_offsets_upload(offsets, nbatch, nullptr, &off_dev);
    if (e == hipSuccess) e = launch_residuals_many<T>(g, nbatch, off_dev, lo, xs, l1xdat, ys, wsd, cd, ldcoef, rd, sd, nullptr);
    if (e == hipSuccess && resid) e = hipMemcpy(res.data(), rd, sizeof(T) * (size_t)npt, hipMemcpyDeviceToHost);
    if (e == hipSuccess && stats) e = hipMemcpy(stats, sd, sizeof(double) * 4 * (size_t)nbatch, hipMemcpyDeviceToHost);
    if (e == hipSuccess && resid)
        for (long long i = 0; i < npt; ++i) resid[lo + i] = res[(size_t)i];
    return many_status(e, what, 0);
}

// ---- splpak_mad_many_* ----
template <typename T>
int32_t mad_many_entry(bool dev, int32_t nbatch, const int64_t *offsets, const T *values, const T *wsel, double *stats, hipStream_t st)
{
    for (int j = 0; j < 8; ++j) t_eval_many_stats[j] = 0;
    bool ok = offsets && nbatch >= 1;
    for (int k = 0; ok && k < nbatch; ++k) ok = offsets[k + 1] >= offsets[k];
    if (!ok || !values || !stats) {
        set_error("offsets null, nbatch < 1, offsets that decrease, or values or stats null");
        return SPLPAK_E_BADARG;
    }
    const ManySpan sp = many_span(offsets, nbatch);
    many_counters(4, sp.n, nbatch);
    if (sp.n == 0 && !dev) {      // nothing for a device to do
        for (size_t j = 0; j < 4 * (size_t)nbatch; ++j) stats[j] = 0.0;
        return 0;
    }
    if (int r = device_ready()) return r;

    const char *what = "medians of a batch of segments";
    const ScratchUse<1> use{t_many_offsets, st};
    const long long *off_dev = nullptr;
    if (dev) {
        hipError_t e = many_offsets_upload(offsets, nbatch, st, &off_dev);
        if (e == hipSuccess) e = launch_mad_many<T>(nbatch, off_dev, 0, values, wsel, stats, st);
        return many_status(e, what, 0);
    }
    CallStage cs;
    const T *vs = nullptr, *wsd = nullptr;
    double *sd = nullptr;
    hipError_t e = stage_copy(cs, values + sp.lo, (size_t)sp.n, &vs);
    if (e == hipSuccess && wsel) e = stage_copy(cs, wsel + sp.lo, (size_t)sp.n, &wsd);
    if (e == hipSuccess && !cs.get(&sd, 4 * (size_t)nbatch)) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = many_offsets_upload(offsets, nbatch, nullptr, &off_dev);
    if (e == hipSuccess) e = launch_mad_many<T>(nbatch, off_dev, sp.lo, vs, wsd, sd, nullptr);
    if (e == hipSuccess) e = hipMemcpy(stats, sd, sizeof(double) * 4 * (size_t)nbatch, hipMemcpyDeviceToHost);
    return many_status(e, what, 0);
}

}  // namespace

extern "C" {

int32_t splpak_mad_many_f64(int32_t nbatch, const int64_t *offsets, const double *values, const double *wsel, double *stats)
{
    return mad_many_entry<double>(false, nbatch, offsets, values, wsel, stats, nullptr);
}

int32_t splpak_mad_many_f32(int32_t nbatch, const int64_t *offsets, const float *values, const float *wsel, double *stats)
{
    return mad_many_entry<float>(false, nbatch, offsets, values, wsel, stats, nullptr);
}

int32_t splpak_mad_many_dev_f64(int32_t nbatch, const int64_t *offsets, const double *values_dev, const double *wsel_dev, double *stats_dev,
                                void *stream)
{
    return mad_many_entry<double>(true, nbatch, offsets, values_dev, wsel_dev, stats_dev, (hipStream_t)stream);
}

int32_t splpak_mad_many_dev_f32(int32_t nbatch, const int64_t *offsets, const float *values_dev, const float *wsel_dev, double *stats_dev,
                                void *stream)
{
    return mad_many_entry<float>(true, nbatch, offsets, values_dev, wsel_dev, stats_dev, (hipStream_t)stream);
}

int32_t splpak_eval_many_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xq, int32_t ldxq, const int32_t *nderiv,
                             const double *coef, int64_t ldcoef, const double *xmin, const double *xmax, const int32_t *nodes, double *out)
{
    return eval_many_entry<double>(false, ndim, nbatch, offsets, xq, ldxq, nderiv, coef, ldcoef, xmin, xmax, nodes, out, nullptr);
}

int32_t splpak_eval_many_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xq, int32_t ldxq, const int32_t *nderiv,
                             const float *coef, int64_t ldcoef, const float *xmin, const float *xmax, const int32_t *nodes, float *out)
{
    return eval_many_entry<float>(false, ndim, nbatch, offsets, xq, ldxq, nderiv, coef, ldcoef, xmin, xmax, nodes, out, nullptr);
}

int32_t splpak_eval_many_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xq_dev, int32_t ldxq, const int32_t *nderiv,
                                 const double *coef_dev, int64_t ldcoef, const double *xmin, const double *xmax, const int32_t *nodes,
                                 double *out_dev, void *stream)
{
    return eval_many_entry<double>(true, ndim, nbatch, offsets, xq_dev, ldxq, nderiv, coef_dev, ldcoef, xmin, xmax, nodes, out_dev,
                                   (hipStream_t)stream);
}

int32_t splpak_eval_many_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xq_dev, int32_t ldxq, const int32_t *nderiv,
                                 const float *coef_dev, int64_t ldcoef, const float *xmin, const float *xmax, const int32_t *nodes,
                                 float *out_dev, void *stream)
{
    return eval_many_entry<float>(true, ndim, nbatch, offsets, xq_dev, ldxq, nderiv, coef_dev, ldcoef, xmin, xmax, nodes, out_dev,
                                  (hipStream_t)stream);
}

int32_t splpak_eval_many_var_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xq, int32_t ldxq, const int32_t *nderiv,
                                 const double *cov, int64_t ldcov, const double *xmin, const double *xmax, const int32_t *nodes, double *out)
{
    return eval_many_var_entry<double>(false, ndim, nbatch, offsets, xq, ldxq, nderiv, cov, ldcov, xmin, xmax, nodes, out, nullptr);
}

int32_t splpak_eval_many_var_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xq, int32_t ldxq, const int32_t *nderiv,
                                 const float *cov, int64_t ldcov, const float *xmin, const float *xmax, const int32_t *nodes, float *out)
{
    return eval_many_var_entry<float>(false, ndim, nbatch, offsets, xq, ldxq, nderiv, cov, ldcov, xmin, xmax, nodes, out, nullptr);
}

int32_t splpak_eval_many_var_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xq_dev, int32_t ldxq,
                                     const int32_t *nderiv, const double *cov_dev, int64_t ldcov, const double *xmin, const double *xmax,
                                     const int32_t *nodes, double *out_dev, void *stream)
{
    return eval_many_var_entry<double>(true, ndim, nbatch, offsets, xq_dev, ldxq, nderiv, cov_dev, ldcov, xmin, xmax, nodes, out_dev,
                                       (hipStream_t)stream);
}

int32_t splpak_eval_many_var_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xq_dev, int32_t ldxq,
                                     const int32_t *nderiv, const float *cov_dev, int64_t ldcov, const float *xmin, const float *xmax,
                                     const int32_t *nodes, float *out_dev, void *stream)
{
    return eval_many_var_entry<float>(true, ndim, nbatch, offsets, xq_dev, ldxq, nderiv, cov_dev, ldcov, xmin, xmax, nodes, out_dev,
                                      (hipStream_t)stream);
}

int32_t splpak_residuals_many_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xdata, int32_t l1xdat, const double *ydata,
                                  const double *wdata, const double *coef, int64_t ldcoef, const double *xmin, const double *xmax,
                                  const int32_t *nodes, double *resid, double *stats)
{
    return residuals_many_entry<double>(false, ndim, nbatch, offsets, xdata, l1xdat, ydata, wdata, coef, ldcoef, xmin, xmax, nodes, resid, stats,
                                        nullptr);
}

int32_t splpak_residuals_many_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xdata, int32_t l1xdat, const float *ydata,
                                  const float *wdata, const float *coef, int64_t ldcoef, const float *xmin, const float *xmax,
                                  const int32_t *nodes, float *resid, double *stats)
{
    return residuals_many_entry<float>(false, ndim, nbatch, offsets, xdata, l1xdat, ydata, wdata, coef, ldcoef, xmin, xmax, nodes, resid, stats,
                                       nullptr);
}

int32_t splpak_residuals_many_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xdata_dev, int32_t l1xdat,
                                      const double *ydata_dev, const double *wdata_dev, const double *coef_dev, int64_t ldcoef,
                                      const double *xmin, const double *xmax, const int32_t *nodes, double *resid_dev, double *stats_dev,
                                      void *stream)
{
    return residuals_many_entry<double>(true, ndim, nbatch, offsets, xdata_dev, l1xdat, ydata_dev, wdata_dev, coef_dev, ldcoef, xmin, xmax, nodes,
                                        resid_dev, stats_dev, (hipStream_t)stream);
}

int32_t splpak_residuals_many_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xdata_dev, int32_t l1xdat,
                                      const float *ydata_dev, const float *wdata_dev, const float *coef_dev, int64_t ldcoef, const float *xmin,
                                      const float *xmax, const int32_t *nodes, float *resid_dev, double *stats_dev, void *stream)
{
    return residuals_many_entry<float>(true, ndim, nbatch, offsets, xdata_dev, l1xdat, ydata_dev, wdata_dev, coef_dev, ldcoef, xmin, xmax, nodes,
                                       resid_dev, stats_dev, (hipStream_t)stream);
}

// host counters of the calling thread's last call of either family (no device is asked, nothing is waited for)
int32_t splpak_debug_eval_many_stats(int64_t out8[8])
{
    if (!out8) { set_error("null argument"); return SPLPAK_E_BADARG; }
    for (int j = 0; j < 8; ++j) out8[j] = t_eval_many_stats[j];
    return 0;
}

}  // extern "C"
