// The entries of the batch of small fits (include/splpak_hip.h): splpak_fit_many_* on host and device pointers, the LDS
// rule and the counters.  The ladder, the launch and the scatter of the results: fitmanyentry.hpp, which the clipped entries
// (fitmanyclipapi.hip) share.
#include "fitmanyentry.hpp"

using namespace splpak;

extern "C" {

int32_t splpak_fit_many_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xdata, int32_t l1xdat, const double *ydata,
                            const double *wdata, const double *xmin, const double *xmax, const int32_t *nodes, double xtrap, double *coef,
                            int64_t ldcoef, int32_t *status, double *info)
{
    return fit_many_entry<double>(false, ndim, nbatch, offsets, xdata, l1xdat, ydata, wdata, xmin, xmax, nodes, xtrap, coef, ldcoef, status, info,
                                  nullptr);
}

int32_t splpak_fit_many_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xdata, int32_t l1xdat, const float *ydata,
                            const float *wdata, const float *xmin, const float *xmax, const int32_t *nodes, float xtrap, float *coef,
                            int64_t ldcoef, int32_t *status, double *info)
{
    return fit_many_entry<float>(false, ndim, nbatch, offsets, xdata, l1xdat, ydata, wdata, xmin, xmax, nodes, (double)xtrap, coef, ldcoef, status,
                                 info, nullptr);
}

int32_t splpak_fit_many_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xdata_dev, int32_t l1xdat,
                                const double *ydata_dev, const double *wdata_dev, const double *xmin, const double *xmax, const int32_t *nodes,
                                double xtrap, double *coef_dev, int64_t ldcoef, int32_t *status, double *info, void *stream)
{
    return fit_many_entry<double>(true, ndim, nbatch, offsets, xdata_dev, l1xdat, ydata_dev, wdata_dev, xmin, xmax, nodes, xtrap, coef_dev, ldcoef,
                                  status, info, (hipStream_t)stream);
}

int32_t splpak_fit_many_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xdata_dev, int32_t l1xdat,
                                const float *ydata_dev, const float *wdata_dev, const float *xmin, const float *xmax, const int32_t *nodes,
                                float xtrap, float *coef_dev, int64_t ldcoef, int32_t *status, double *info, void *stream)
{
    return fit_many_entry<float>(true, ndim, nbatch, offsets, xdata_dev, l1xdat, ydata_dev, wdata_dev, xmin, xmax, nodes, (double)xtrap, coef_dev,
                                 ldcoef, status, info, (hipStream_t)stream);
}

// the LDS bytes a problem of this grid takes (host only); SPLPAK_E_BADARG for a shape the ladder rejects
int64_t splpak_fit_many_lds_bytes(int32_t ndim, const int32_t *nodes)
{
    if (!nodes || ndim < 1 || ndim > 2) { set_error("nodes is null or ndim is not 1 or 2"); return SPLPAK_E_BADARG; }
    for (int d = 0; d < ndim; ++d)
        if (nodes[d] < 4) { set_error("fewer than 4 nodes in a dimension"); return SPLPAK_E_BADARG; }
    for (int d = 0; d < ndim; ++d)
        if (nodes[d] > (1 << 20)) return INT64_MAX / 2;      // (far beyond any budget; keeps the products below within int64)
    return fit_many_shape(ndim, nodes).bytes;
}

// host counters of the calling thread's last splpak_fit_many_* call (no device is asked, nothing is waited for)
int32_t splpak_debug_fit_many_stats(int64_t out8[8])
{
    if (!out8) { set_error("null argument"); return SPLPAK_E_BADARG; }
    for (int j = 0; j < 8; ++j) out8[j] = t_fit_many_stats[j];
    return 0;
}

}  // extern "C"
