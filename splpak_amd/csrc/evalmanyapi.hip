// The entries of the batch evaluation at each problem's own points (include/splpak_hip.h): splpak_eval_many_* and
// splpak_residuals_many_* on host and device pointers, and their counters.  Each family has one ladder of checks, in the order
// the header gives, all on the host; then evalmany.hip.  The _dev entries only enqueue: the one thing they upload is the
// offsets, into the calling thread's scratch (eval_many_offsets).  The host entries stage the span of the batch's points and
// (nbatch-1)*ldcoef + ncol coefficients through device memory of the call.
#include "plan.hpp"
#include "evalcore.hpp"
#include "evalmany.hpp"

#include <vector>

using namespace splpak;

namespace {

// device memory of one host call, released with it
struct CallStage {
    std::vector<void *> held;
    ~CallStage() { for (void *p : held) (void)hipFree(p); }
    template <typename U> bool get(U **out, size_t count)
    {
        void *q = nullptr;
        if (hip_malloc_retry(&q, (count ? count : 1) * sizeof(U)) != hipSuccess) {
            (void)hipGetLastError();
            set_error("the device copies of the batch could not be allocated");
            return false;
        }
        held.push_back(q);
        *out = static_cast<U *>(q);
        return true;
    }
};

// The rungs both ladders open with.  True: the grid is built (rc = 0); false: rc is the status, and `zero` says whether it is
// one of 101 / 102 / 103 (eval_many zeroes its results on these).
template <typename T>
bool many_open(int32_t ndim, int32_t nbatch, const int64_t *offsets, const T *xmin_t, const T *xmax_t, const int32_t *nodes, Grid &g, int &rc,
               bool &zero)
{
    zero = false;
    if (!offsets || !nodes || !xmin_t || !xmax_t) { set_error("null argument"); rc = SPLPAK_E_BADARG; return false; }
    bool ok = nbatch >= 1;
    for (int k = 0; ok && k < nbatch; ++k) ok = offsets[k + 1] >= offsets[k];
    if (!ok) { set_error("nbatch < 1 or offsets that decrease"); rc = SPLPAK_E_BADARG; return false; }
    if (ndim < 1) { rc = 101; zero = true; return false; }
    if (ndim > MAXD) { set_error("more than 4 dimensions are not supported"); rc = SPLPAK_E_UNSUPPORTED; return false; }
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

int32_t many_status(hipError_t e, const char *what, int rc)
{
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        set_error("the device copy of the offsets could not be allocated");
        return SPLPAK_E_NOMEM;
    }
    return hip_ok(e, what) ? rc : SPLPAK_E_NODEVICE;
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
            const long long lo = offsets[0], n = offsets[nbatch] - lo;
            if (dev) { if (n > 0) (void)hipMemsetAsync(out + lo, 0, sizeof(T) * (size_t)n, st); }
            else for (long long i = 0; i < n; ++i) out[lo + i] = (T)0;
        }
        return rc;
    }
    if (ldxq < ndim || ldcoef < g.ncol) { set_error("ldxq smaller than ndim or ldcoef smaller than the number of coefficients"); return SPLPAK_E_BADARG; }
    if (nderiv)
        for (int d = 0; d < ndim; ++d)
            if (nderiv[d] < 0 || nderiv[d] > 2) rc = 104;      // reported; evaluated with the orders clamped
    const long long lo = offsets[0], nq = offsets[nbatch] - lo;
    many_counters(1, nq, nbatch);
    if (nq == 0) return rc;
    if (!xq || !coef || !out) { set_error("null argument"); return SPLPAK_E_BADARG; }
    if (int r = device_ready()) return r;

    const long long *off_dev = nullptr;
    if (dev) {
        hipError_t e = eval_many_offsets(offsets, nbatch, st, &off_dev);
        if (e == hipSuccess) e = launch_eval_many<T>(g, nbatch, off_dev, lo, nq, 0, xq, ldxq, nderiv, coef, ldcoef, out, st);
        eval_many_offsets_used(st);
        return many_status(e, "evaluation of a batch of fits", rc);
    }
    // the host form: the span of the batch's queries alone, the coefficient sets with the caller's ldcoef in one copy
    const size_t ncoef = (size_t)(nbatch - 1) * (size_t)ldcoef + (size_t)g.ncol;
    std::vector<T> res((size_t)nq);
    CallStage cs;
    T *xs = nullptr, *cd = nullptr, *od = nullptr;
    if (!cs.get(&xs, (size_t)nq * (size_t)ldxq) || !cs.get(&cd, ncoef) || !cs.get(&od, (size_t)nq)) return SPLPAK_E_NOMEM;
    hipError_t e = hipMemcpy(xs, xq + lo * ldxq, sizeof(T) * (size_t)nq * (size_t)ldxq, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(cd, coef, sizeof(T) * ncoef, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = eval_many_offsets(offsets, nbatch, nullptr, &off_dev);
    if (e == hipSuccess) e = launch_eval_many<T>(g, nbatch, off_dev, lo, nq, lo, (const T *)xs, ldxq, nderiv, (const T *)cd, ldcoef, od, nullptr);
    eval_many_offsets_used(nullptr);
    if (e == hipSuccess) e = hipMemcpy(res.data(), od, sizeof(T) * (size_t)nq, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        for (long long i = 0; i < nq; ++i) out[lo + i] = res[(size_t)i];
    return many_status(e, "evaluation of a batch of fits", rc);
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
    const long long lo = offsets[0], npt = offsets[nbatch] - lo;
    many_counters(2, npt, nbatch);
    if (npt == 0 && !dev) {      // nothing for a device to do
        if (stats)
            for (int k = 0; k < nbatch; ++k) { stats[4 * (size_t)k] = stats[4 * (size_t)k + 1] = stats[4 * (size_t)k + 2] = 0.0; stats[4 * (size_t)k + 3] = -1.0; }
        return 0;
    }
    if (npt == 0 && !stats) return 0;
    if (int r = device_ready()) return r;

    const long long *off_dev = nullptr;
    if (dev) {
        hipError_t e = eval_many_offsets(offsets, nbatch, st, &off_dev);
        if (e == hipSuccess) e = launch_residuals_many<T>(g, nbatch, off_dev, 0, xdata, l1xdat, ydata, wdata, coef, ldcoef, resid, stats, st);
        eval_many_offsets_used(st);
        return many_status(e, "residuals of a batch of fits", 0);
    }
    const size_t ncoef = (size_t)(nbatch - 1) * (size_t)ldcoef + (size_t)g.ncol;
    std::vector<T> res(resid ? (size_t)npt : 0);
    CallStage cs;
    T *xs = nullptr, *ys = nullptr, *wsd = nullptr, *cd = nullptr, *rd = nullptr;
    double *sd = nullptr;
    if (!cs.get(&xs, (size_t)npt * (size_t)l1xdat) || !cs.get(&ys, (size_t)npt) || (wdata && !cs.get(&wsd, (size_t)npt)) || !cs.get(&cd, ncoef) ||
        (resid && !cs.get(&rd, (size_t)npt)) || (stats && !cs.get(&sd, 4 * (size_t)nbatch)))
        return SPLPAK_E_NOMEM;
    hipError_t e = hipMemcpy(xs, xdata + lo * l1xdat, sizeof(T) * (size_t)npt * (size_t)l1xdat, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ys, ydata + lo, sizeof(T) * (size_t)npt, hipMemcpyHostToDevice);
    if (e == hipSuccess && wdata) e = hipMemcpy(wsd, wdata + lo, sizeof(T) * (size_t)npt, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(cd, coef, sizeof(T) * ncoef, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = eval_many_offsets(offsets, nbatch, nullptr, &off_dev);
    if (e == hipSuccess)
        e = launch_residuals_many<T>(g, nbatch, off_dev, lo, (const T *)xs, l1xdat, (const T *)ys, (const T *)wsd, (const T *)cd, ldcoef, rd, sd, nullptr);
    eval_many_offsets_used(nullptr);
    if (e == hipSuccess && resid) e = hipMemcpy(res.data(), rd, sizeof(T) * (size_t)npt, hipMemcpyDeviceToHost);
    if (e == hipSuccess && stats) e = hipMemcpy(stats, sd, sizeof(double) * 4 * (size_t)nbatch, hipMemcpyDeviceToHost);
    if (e == hipSuccess && resid)
        for (long long i = 0; i < npt; ++i) resid[lo + i] = res[(size_t)i];
    return many_status(e, "residuals of a batch of fits", 0);
}

}  // namespace

extern "C" {

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
