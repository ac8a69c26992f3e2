// The grid-fit entries of the C ABI (include/splpak_hip.h): splpak_fit_grid_* on host and device pointers and the two debug
// entries.  One ladder of argument checks (fit_grid_validate, fitgridentry.hpp), one host part (fitgrid.hip fit_grid_host), one device part.
#include "fitgridentry.hpp"

#include <new>
#include <vector>

using namespace splpak;

// dev: axes, waxes, values and coef are device arrays (the axes come to the host: one synchronisation of the stream)
template <typename T>
static int32_t fit_grid_entry(bool dev, int32_t ndim, const int64_t *npts, const T *axes, const T *waxes, int32_t nfields, const T *values,
                              int64_t ldv, const T *xmin, const T *xmax, const int32_t *nodes, double xtrap, T *coef, int64_t ldcoef,
                              double *info, hipStream_t st)
{
    Grid g;
    long long nsamp = 1, ntab = 0;
    int rc = 0;
    if (!fit_grid_validate<T>(ndim, npts, axes, nfields, values, ldv, xmin, xmax, nodes, coef, ldcoef, g, nsamp, ntab, rc)) return rc;
    try {
        std::vector<double> ax((size_t)ntab), wx(waxes ? (size_t)ntab : 0);
        if (dev) {
            if (int r = device_ready()) return r;
            std::vector<T> tmp((size_t)ntab * (waxes ? 2 : 1));
            SPLPAK_HIP_TRY(hipMemcpyAsync(tmp.data(), axes, sizeof(T) * (size_t)ntab, hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
            if (waxes) SPLPAK_HIP_TRY(hipMemcpyAsync(tmp.data() + ntab, waxes, sizeof(T) * (size_t)ntab, hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
            SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
            for (long long i = 0; i < ntab; ++i) ax[(size_t)i] = (double)tmp[(size_t)i];
            for (long long i = 0; waxes && i < ntab; ++i) wx[(size_t)i] = (double)tmp[(size_t)(ntab + i)];
        } else {
            for (long long i = 0; i < ntab; ++i) ax[(size_t)i] = (double)axes[i];
            for (long long i = 0; waxes && i < ntab; ++i) wx[(size_t)i] = (double)waxes[i];
        }
        FitGridHost h;
        rc = fit_grid_host(g, npts, ax.data(), waxes ? wx.data() : nullptr, xtrap, h);
        if (rc == 107) {      // the coefficients of every field zeroed; the words between the fields stay
            for (int32_t k = 0; k < nfields; ++k) {
                T *ck = coef + (long long)k * ldcoef;
                if (dev) (void)hipMemsetAsync(ck, 0, sizeof(T) * (size_t)g.ncol, st);
                else for (int i = 0; i < g.ncol; ++i) ck[i] = (T)0;
            }
        }
        if (rc != 0) return rc;
        if (!dev)
            if (int r = device_ready()) return r;
        return fit_grid_device<T>(h, nfields, values, ldv, coef, ldcoef, info, !dev, st);
    } catch (const std::bad_alloc &) {
        set_error("the host copies of the axes could not be allocated");
        return SPLPAK_E_NOMEM;
    }
}

extern "C" {

int32_t splpak_fit_grid_f64(int32_t ndim, const int64_t *npts, const double *axes, const double *waxes, int32_t nfields,
                            const double *values, int64_t ldv, const double *xmin, const double *xmax, const int32_t *nodes,
                            double xtrap, double *coef, int64_t ldcoef, double *info)
{
    return fit_grid_entry<double>(false, ndim, npts, axes, waxes, nfields, values, ldv, xmin, xmax, nodes, xtrap, coef, ldcoef, info, nullptr);
}

int32_t splpak_fit_grid_f32(int32_t ndim, const int64_t *npts, const float *axes, const float *waxes, int32_t nfields,
                            const float *values, int64_t ldv, const float *xmin, const float *xmax, const int32_t *nodes,
                            float xtrap, float *coef, int64_t ldcoef, double *info)
{
    return fit_grid_entry<float>(false, ndim, npts, axes, waxes, nfields, values, ldv, xmin, xmax, nodes, (double)xtrap, coef, ldcoef, info, nullptr);
}

int32_t splpak_fit_grid_dev_f64(int32_t ndim, const int64_t *npts, const double *axes_dev, const double *waxes_dev, int32_t nfields,
                                const double *values_dev, int64_t ldv, const double *xmin, const double *xmax, const int32_t *nodes,
                                double xtrap, double *coef_dev, int64_t ldcoef, double *info, void *stream)
{
    return fit_grid_entry<double>(true, ndim, npts, axes_dev, waxes_dev, nfields, values_dev, ldv, xmin, xmax, nodes, xtrap, coef_dev, ldcoef,
                                  info, (hipStream_t)stream);
}

int32_t splpak_fit_grid_dev_f32(int32_t ndim, const int64_t *npts, const float *axes_dev, const float *waxes_dev, int32_t nfields,
                                const float *values_dev, int64_t ldv, const float *xmin, const float *xmax, const int32_t *nodes,
                                float xtrap, float *coef_dev, int64_t ldcoef, double *info, void *stream)
{
    return fit_grid_entry<float>(true, ndim, npts, axes_dev, waxes_dev, nfields, values_dev, ldv, xmin, xmax, nodes, (double)xtrap, coef_dev,
                                 ldcoef, info, (hipStream_t)stream);
}

// one stage of the device part alone (host arrays, one field, no xtrap rule): the checks of splpak_fit_grid_f64 with ldv = prod npts
// and ldcoef = ncol, then SPLPAK_E_BADARG for another stage
int32_t splpak_debug_fit_grid_stage_f64(int32_t stage, int32_t ndim, const int64_t *npts, const double *axes, const double *waxes,
                                        const double *xmin, const double *xmax, const int32_t *nodes, const double *in, double *out)
{
    Grid g;
    long long nsamp = 1, ntab = 0;
    int rc = 0;
    if (!fit_grid_validate<double>(ndim, npts, axes, 1, in, INT64_MAX, xmin, xmax, nodes, out, INT64_MAX, g, nsamp, ntab, rc)) return rc;
    if (stage < 0 || stage > 1) { set_error("stage must be 0 (spread) or 1 (solves)"); return SPLPAK_E_BADARG; }
    FitGridHost h;
    rc = fit_grid_host(g, npts, axes, waxes, 0.0, h);
    if (rc != 0) return rc;
    if (int r = device_ready()) return r;
    return fit_grid_stage(h, stage, in, out);
}

// host counters of the calling thread's last grid fit (no device is asked, nothing is waited for)
int32_t splpak_debug_fit_grid_stats(int64_t out8[8])
{
    if (!out8) { set_error("null argument"); return SPLPAK_E_BADARG; }
    long long v[8];
    fit_grid_stats(v);
    for (int j = 0; j < 8; ++j) out8[j] = v[j];
    return 0;
}

}  // extern "C"
