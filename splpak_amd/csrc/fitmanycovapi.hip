// The entries of the batch fits with the covariance of their coefficients (include/splpak_hip.h): splpak_fit_many_cov_* on
// host and device pointers, and the length rule of `cov`.  The ladder of splpak_fit_many_* with ldcov on its 104 rung and cov
// among the null data pointers, the launch (fitmanycov.hip) and the scatter of the results: fitmanyentry.hpp.
#include "fitmanyentry.hpp"

using namespace splpak;

extern "C" {

int32_t splpak_fit_many_cov_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xdata, int32_t l1xdat, const double *ydata,
                                const double *wdata, const double *xmin, const double *xmax, const int32_t *nodes, double xtrap, double *coef,
                                int64_t ldcoef, double *cov, int64_t ldcov, int32_t *status, double *info)
{
    const CovSpec<double> spec{cov, ldcov};
    return fit_many_entry<double>(false, ndim, nbatch, offsets, xdata, l1xdat, ydata, wdata, xmin, xmax, nodes, xtrap, coef, ldcoef, status, info,
                                  nullptr, nullptr, &spec);
}

int32_t splpak_fit_many_cov_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xdata, int32_t l1xdat, const float *ydata,
                                const float *wdata, const float *xmin, const float *xmax, const int32_t *nodes, float xtrap, float *coef,
                                int64_t ldcoef, float *cov, int64_t ldcov, int32_t *status, double *info)
{
    const CovSpec<float> spec{cov, ldcov};
    return fit_many_entry<float>(false, ndim, nbatch, offsets, xdata, l1xdat, ydata, wdata, xmin, xmax, nodes, (double)xtrap, coef, ldcoef, status,
                                 info, nullptr, nullptr, &spec);
}

int32_t splpak_fit_many_cov_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xdata_dev, int32_t l1xdat,
                                    const double *ydata_dev, const double *wdata_dev, const double *xmin, const double *xmax,
                                    const int32_t *nodes, double xtrap, double *coef_dev, int64_t ldcoef, double *cov_dev, int64_t ldcov,
                                    int32_t *status, double *info, void *stream)
{
    const CovSpec<double> spec{cov_dev, ldcov};
    return fit_many_entry<double>(true, ndim, nbatch, offsets, xdata_dev, l1xdat, ydata_dev, wdata_dev, xmin, xmax, nodes, xtrap, coef_dev, ldcoef,
                                  status, info, (hipStream_t)stream, nullptr, &spec);
}

int32_t splpak_fit_many_cov_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xdata_dev, int32_t l1xdat,
                                    const float *ydata_dev, const float *wdata_dev, const float *xmin, const float *xmax, const int32_t *nodes,
                                    float xtrap, float *coef_dev, int64_t ldcoef, float *cov_dev, int64_t ldcov, int32_t *status, double *info,
                                    void *stream)
{
    const CovSpec<float> spec{cov_dev, ldcov};
    return fit_many_entry<float>(true, ndim, nbatch, offsets, xdata_dev, l1xdat, ydata_dev, wdata_dev, xmin, xmax, nodes, (double)xtrap, coef_dev,
                                 ldcoef, status, info, (hipStream_t)stream, nullptr, &spec);
}

// the words of one problem's cov, ncol (7^ndim + 1) / 2 (host only); the refusals of splpak_fit_many_lds_bytes
int64_t splpak_fit_many_cov_len(int32_t ndim, const int32_t *nodes)
{
    if (!nodes || ndim < 1 || ndim > 2) { set_error("nodes is null or ndim is not 1 or 2"); return SPLPAK_E_BADARG; }
    for (int d = 0; d < ndim; ++d)
        if (nodes[d] < 4) { set_error("fewer than 4 nodes in a dimension"); return SPLPAK_E_BADARG; }
    for (int d = 0; d < ndim; ++d)
        if (nodes[d] > (1 << 20)) return INT64_MAX / 2;      // (as splpak_fit_many_lds_bytes: the product below stays within int64)
    return fit_many_cov_len(ndim, (long long)nodes[0] * (ndim == 2 ? nodes[1] : 1));
}

}  // extern "C"
