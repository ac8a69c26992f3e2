// The entries of the grid fit with a weight per sample (include/splpak_hip.h): splpak_fit_grid_weighted_* on host and device
// pointers and the two debug entries.  The ladder of splpak_fit_grid_* (fit_grid_validate) with `weights` among its null
// checks and `ldw` behind it, the host tables of fitgrid.hip without axis weights, then fitgridw.hip.
#include "fitgridentry.hpp"

#include <new>
#include <vector>

using namespace splpak;

// the ladder, then the axes on the host (dev: one synchronisation of the stream) and their tables; 0: h and ax are ready.
// On 107 (an axis that is rank deficient whatever the weights) the coefficients of every field are zeroed where asked.
template <typename T>
static int weighted_prepare(bool dev, int32_t ndim, const int64_t *npts, const T *axes, int32_t nfields, const void *values, int64_t ldv,
                            const void *weights, int64_t ldw, const T *xmin, const T *xmax, const int32_t *nodes, T *coef, int64_t ldcoef,
                            bool zero_on_107, hipStream_t st, FitGridHost &h, std::vector<double> &ax)
{
    Grid g;
    long long nsamp = 1, ntab = 0;
    int rc = 0;
    if (!fit_grid_validate<T>(ndim, npts, axes, nfields, weights ? values : nullptr, ldv, xmin, xmax, nodes, coef, ldcoef, g, nsamp, ntab, rc))
        return rc;
    if (ldw != 0 && ldw < nsamp) {
        set_error("ldw is neither 0 (one weight array for all fields) nor at least the product of npts");
        return SPLPAK_E_BADARG;
    }
    ax.resize((size_t)ntab);
    if (dev) {
        if (int r = device_ready()) return r;
        std::vector<T> tmp((size_t)ntab);
        SPLPAK_HIP_TRY(hipMemcpyAsync(tmp.data(), axes, sizeof(T) * (size_t)ntab, hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
        for (long long i = 0; i < ntab; ++i) ax[(size_t)i] = (double)tmp[(size_t)i];
    } else {
        for (long long i = 0; i < ntab; ++i) ax[(size_t)i] = (double)axes[i];
    }
    rc = fit_grid_host(g, npts, ax.data(), nullptr, 0.0, h);
    if (rc == 107 && zero_on_107) {
        for (int32_t k = 0; k < nfields; ++k) {
            T *ck = coef + (long long)k * ldcoef;
            if (dev) (void)hipMemsetAsync(ck, 0, sizeof(T) * (size_t)g.ncol, st);
            else for (int i = 0; i < g.ncol; ++i) ck[i] = (T)0;
        }
    }
    return rc;
}

template <typename T>
static int32_t weighted_entry(bool dev, int32_t ndim, const int64_t *npts, const T *axes, int32_t nfields, const T *values, int64_t ldv,
                              const T *weights, int64_t ldw, const T *xmin, const T *xmax, const int32_t *nodes, double xtrap, T *coef,
                              int64_t ldcoef, double *info, hipStream_t st)
{
    try {
        FitGridHost h;
        std::vector<double> ax;
        if (int r = weighted_prepare<T>(dev, ndim, npts, axes, nfields, values, ldv, weights, ldw, xmin, xmax, nodes, coef, ldcoef, true, st, h, ax))
            return r;
        if (!dev)
            if (int r = device_ready()) return r;
        return fit_grid_weighted_device<T>(h, ax.data(), xtrap, nfields, values, ldv, weights, ldw, coef, ldcoef, info, !dev, st);
    } catch (const std::bad_alloc &) {
        set_error("the host copies of the axes could not be allocated");
        return SPLPAK_E_NOMEM;
    }
}

extern "C" {

int32_t splpak_fit_grid_weighted_f64(int32_t ndim, const int64_t *npts, const double *axes, int32_t nfields, const double *values,
                                     int64_t ldv, const double *weights, int64_t ldw, const double *xmin, const double *xmax,
                                     const int32_t *nodes, double xtrap, double *coef, int64_t ldcoef, double *info)
{
    return weighted_entry<double>(false, ndim, npts, axes, nfields, values, ldv, weights, ldw, xmin, xmax, nodes, xtrap, coef, ldcoef, info,
                                  nullptr);
}

int32_t splpak_fit_grid_weighted_f32(int32_t ndim, const int64_t *npts, const float *axes, int32_t nfields, const float *values, int64_t ldv,
                                     const float *weights, int64_t ldw, const float *xmin, const float *xmax, const int32_t *nodes,
                                     float xtrap, float *coef, int64_t ldcoef, double *info)
{
    return weighted_entry<float>(false, ndim, npts, axes, nfields, values, ldv, weights, ldw, xmin, xmax, nodes, (double)xtrap, coef, ldcoef,
                                 info, nullptr);
}

int32_t splpak_fit_grid_weighted_dev_f64(int32_t ndim, const int64_t *npts, const double *axes_dev, int32_t nfields, const double *values_dev,
                                         int64_t ldv, const double *weights_dev, int64_t ldw, const double *xmin, const double *xmax,
                                         const int32_t *nodes, double xtrap, double *coef_dev, int64_t ldcoef, double *info, void *stream)
{
    return weighted_entry<double>(true, ndim, npts, axes_dev, nfields, values_dev, ldv, weights_dev, ldw, xmin, xmax, nodes, xtrap, coef_dev,
                                  ldcoef, info, (hipStream_t)stream);
}

int32_t splpak_fit_grid_weighted_dev_f32(int32_t ndim, const int64_t *npts, const float *axes_dev, int32_t nfields, const float *values_dev,
                                         int64_t ldv, const float *weights_dev, int64_t ldw, const float *xmin, const float *xmax,
                                         const int32_t *nodes, float xtrap, float *coef_dev, int64_t ldcoef, double *info, void *stream)
{
    return weighted_entry<float>(true, ndim, npts, axes_dev, nfields, values_dev, ldv, weights_dev, ldw, xmin, xmax, nodes, (double)xtrap,
                                 coef_dev, ldcoef, info, (hipStream_t)stream);
}

// one stage alone (host arrays, one field, no xtrap rule): the checks of splpak_fit_grid_weighted_f64 with ldv = ldw = prod npts
// and ldcoef = ncol, then SPLPAK_E_BADARG for another stage
int32_t splpak_debug_fit_grid_weighted_stage_f64(int32_t stage, int32_t ndim, const int64_t *npts, const double *axes, const double *weights,
                                                 const double *xmin, const double *xmax, const int32_t *nodes, const double *in, double *out)
{
    try {
        FitGridHost h;
        std::vector<double> ax;
        // (stage 3 reads no `in`; `out` is checked as the coefficients are, and is no coefficient array to zero on 107)
        const void *in_checked = stage == 3 ? (const void *)weights : (const void *)in;
        if (int r = weighted_prepare<double>(false, ndim, npts, axes, 1, in_checked, INT64_MAX, weights, 0, xmin, xmax, nodes, out, INT64_MAX,
                                             false, nullptr, h, ax))
            return r;
        if (stage < 0 || stage > 3) {
            set_error("stage must be 0 (right-hand side), 1 (operator), 2 (preconditioner) or 3 (marginals and diagonal)");
            return SPLPAK_E_BADARG;
        }
        if (int r = device_ready()) return r;
        return fit_grid_weighted_stage(h, ax.data(), stage, weights, in, out);
    } catch (const std::bad_alloc &) {
        set_error("the host copies of the axes could not be allocated");
        return SPLPAK_E_NOMEM;
    }
}

// host counters of the calling thread's last weighted grid fit (no device is asked, nothing is waited for)
int32_t splpak_debug_fit_grid_weighted_stats(int64_t out8[8])
{
    if (!out8) { set_error("null argument"); return SPLPAK_E_BADARG; }
    long long v[8];
    fit_grid_weighted_stats(v);
    for (int j = 0; j < 8; ++j) out8[j] = v[j];
    return 0;
}

}  // extern "C"
