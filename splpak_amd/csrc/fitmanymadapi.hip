// The entries of the robustly clipped batch fits (include/splpak_hip.h): splpak_fit_many_clip_mad_* on host and device
// pointers.  The ladder of splpak_fit_many_clip_* (any regrow is valid), the launch (fitmanymad.hip) and the scatter of the
// results, six clip numbers per problem: fitmanyentry.hpp.
#include "fitmanyentry.hpp"

using namespace splpak;

extern "C" {

int32_t splpak_fit_many_clip_mad_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xdata, int32_t l1xdat,
                                 const double *ydata, const double *wdata, const double *xmin, const double *xmax, const int32_t *nodes,
                                 double xtrap, double klo, double khi, int32_t maxpass, int32_t regrow, double *wout, double *coef, int64_t ldcoef,
                                 int32_t *status, double *info, double *clip)
{
    const ClipSpec<double> spec{klo, khi, maxpass, wout, clip, 6, true, regrow};
    return fit_many_entry<double>(false, ndim, nbatch, offsets, xdata, l1xdat, ydata, wdata, xmin, xmax, nodes, xtrap, coef, ldcoef, status, info,
                                  nullptr, &spec);
}

int32_t splpak_fit_many_clip_mad_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xdata, int32_t l1xdat, const float *ydata,
                                 const float *wdata, const float *xmin, const float *xmax, const int32_t *nodes, float xtrap, float klo,
                                 float khi, int32_t maxpass, int32_t regrow, float *wout, float *coef, int64_t ldcoef, int32_t *status, double *info,
                                 double *clip)
{
    const ClipSpec<float> spec{(double)klo, (double)khi, maxpass, wout, clip, 6, true, regrow};
    return fit_many_entry<float>(false, ndim, nbatch, offsets, xdata, l1xdat, ydata, wdata, xmin, xmax, nodes, (double)xtrap, coef, ldcoef, status,
                                 info, nullptr, &spec);
}

int32_t splpak_fit_many_clip_mad_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xdata_dev, int32_t l1xdat,
                                     const double *ydata_dev, const double *wdata_dev, const double *xmin, const double *xmax,
                                     const int32_t *nodes, double xtrap, double klo, double khi, int32_t maxpass, int32_t regrow, double *wout_dev,
                                     double *coef_dev, int64_t ldcoef, int32_t *status, double *info, double *clip, void *stream)
{
    const ClipSpec<double> spec{klo, khi, maxpass, wout_dev, clip, 6, true, regrow};
    return fit_many_entry<double>(true, ndim, nbatch, offsets, xdata_dev, l1xdat, ydata_dev, wdata_dev, xmin, xmax, nodes, xtrap, coef_dev, ldcoef,
                                  status, info, (hipStream_t)stream, &spec);
}

int32_t splpak_fit_many_clip_mad_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xdata_dev, int32_t l1xdat,
                                     const float *ydata_dev, const float *wdata_dev, const float *xmin, const float *xmax,
                                     const int32_t *nodes, float xtrap, float klo, float khi, int32_t maxpass, int32_t regrow, float *wout_dev,
                                     float *coef_dev, int64_t ldcoef, int32_t *status, double *info, double *clip, void *stream)
{
    const ClipSpec<float> spec{(double)klo, (double)khi, maxpass, wout_dev, clip, 6, true, regrow};
    return fit_many_entry<float>(true, ndim, nbatch, offsets, xdata_dev, l1xdat, ydata_dev, wdata_dev, xmin, xmax, nodes, (double)xtrap, coef_dev,
                                 ldcoef, status, info, (hipStream_t)stream, &spec);
}

}  // extern "C"
