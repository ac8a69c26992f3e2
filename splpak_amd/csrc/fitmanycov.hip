// The batch of small fits with the covariance of its coefficients: splpak_fit_many_cov_* (include/splpak_hip.h).  The kernel
// is fit_many_kernel (fitmany.hip) with phase 6 of fit_problem switched on (fitmanydev.hpp: selected_inverse): the workgroup
// that fitted a problem turns the band factor it still holds in LDS into the band of N^-1, in place, and writes the half
// stencil of every node to `cov`.  The LDS map, the workgroup shapes and the launch are those of the plain fit.  Then the
// entries on host and device pointers and the length rule of `cov`: the call of splpak_fit_many_* (fitmanyentry.hpp) with
// ldcov on its 104 rung and cov among the null data pointers, staged and scattered like coef.
#include "fitmanydev.hpp"
#include "fitmanyentry.hpp"

namespace splpak {

namespace {

using namespace fitmanydev;

// (The one-wave 1-D kernel is asked to keep the four waves per SIMD of fit_many_kernel, which has 125 VGPRs: left alone it takes
// 129, one allocation step past the 128 that four waves allow, and a quarter fewer problems are in flight.)
template <int D, typename T, int NT>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(D == 1 && NT == 64 ? 4 : 1)))
fit_many_cov_kernel(FitManyArgs a, const T *__restrict__ xd, const T *__restrict__ yd, const T *__restrict__ wd, T *__restrict__ coef,
                    T *__restrict__ cov, long long ldcov)
{
    extern __shared__ double fit_many_cov_lds[];
    const Lds L = carve(fit_many_cov_lds, a.sh);

    for (int r = blockIdx.x; r < a.nrun; r += gridDim.x) {
        const Problem p = problem_of(a, r);
        const bool weighted = first_weight_counts(wd, p.p0);
        const FitOutcome o = fit_problem<D, T, NT, const T *__restrict__, true>(a, L, xd, yd, wd, weighted, p.p0, p.np, coef + p.slot() * a.ldcoef,
                                                                                cov + p.slot() * ldcov);
        if (threadIdx.x == 0) store_outcome(o, a.result + (long long)r * FM_RESULT);
    }
}

// the launch of fit_many_launch (fitmany.hip) with the selected inverse: cov of a problem at its coefficients' slot times ldcov
template <typename T>
int fit_many_cov_launch(const FitManyArgs &a, const T *xdata, const T *ydata, const T *wdata, T *coef, T *cov, long long ldcov, hipStream_t st,
                        double *seconds)
{
    // the 2-D phase gives a lane of one wave to every entry of a column: hb + 1 <= 64 (the LDS rule admits 40 at the most)
    if (a.g.ndim == 2 && a.sh.hb + 1 > 64) { set_error("the band is wider than a wave: no covariance for this grid"); return SPLPAK_E_UNSUPPORTED; }
    return many_timed_launch(a.sh, st, seconds, [&](int cus, unsigned *blocks) {
        return many_shape_ladder(a.sh, [&](auto D, auto NT) {
            return many_launch(fit_many_cov_kernel<D(), T, NT()>, NT(), (size_t)a.sh.bytes, a.nrun, cus, st, blocks, a, xdata, ydata, wdata, coef,
                               cov, ldcov);
        });
    });
}

template <typename T>
int32_t fit_many_cov_call(bool dev, const FitManyIn<T> &in, T *coef, int64_t ldcoef, T *cov, int64_t ldcov, int32_t *status, double *info,
                          void *stream)
{
    FitManyCall<T> c{in, dev, (hipStream_t)stream, coef, ldcoef, status, info, "a batch of fits with their covariance"};
    c.has_cov = true;
    c.cov = cov;
    c.ldcov = ldcov;
    return fit_many_entry(c, [](const FitManyArgs &a, const T *xd, const T *yd, const T *wd, T *, T *cd, T *cvd, long long ldcvd, hipStream_t st,
                                double *seconds) { return fit_many_cov_launch<T>(a, xd, yd, wd, cd, cvd, ldcvd, st, seconds); });
}

}  // namespace

}  // namespace splpak

using namespace splpak;

extern "C" {

int32_t splpak_fit_many_cov_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xdata, int32_t l1xdat, const double *ydata,
                                const double *wdata, const double *xmin, const double *xmax, const int32_t *nodes, double xtrap, double *coef,
                                int64_t ldcoef, double *cov, int64_t ldcov, int32_t *status, double *info)
{
    return fit_many_cov_call<double>(false, {ndim, nbatch, offsets, xdata, l1xdat, ydata, wdata, xmin, xmax, nodes, xtrap}, coef, ldcoef, cov, ldcov,
                                     status, info, nullptr);
}

int32_t splpak_fit_many_cov_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xdata, int32_t l1xdat, const float *ydata,
                                const float *wdata, const float *xmin, const float *xmax, const int32_t *nodes, float xtrap, float *coef,
                                int64_t ldcoef, float *cov, int64_t ldcov, int32_t *status, double *info)
{
    return fit_many_cov_call<float>(false, {ndim, nbatch, offsets, xdata, l1xdat, ydata, wdata, xmin, xmax, nodes, xtrap}, coef, ldcoef, cov, ldcov,
                                    status, info, nullptr);
}

int32_t splpak_fit_many_cov_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xdata_dev, int32_t l1xdat,
                                    const double *ydata_dev, const double *wdata_dev, const double *xmin, const double *xmax,
                                    const int32_t *nodes, double xtrap, double *coef_dev, int64_t ldcoef, double *cov_dev, int64_t ldcov,
                                    int32_t *status, double *info, void *stream)
{
    return fit_many_cov_call<double>(true, {ndim, nbatch, offsets, xdata_dev, l1xdat, ydata_dev, wdata_dev, xmin, xmax, nodes, xtrap}, coef_dev,
                                     ldcoef, cov_dev, ldcov, status, info, stream);
}

int32_t splpak_fit_many_cov_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xdata_dev, int32_t l1xdat,
                                    const float *ydata_dev, const float *wdata_dev, const float *xmin, const float *xmax, const int32_t *nodes,
                                    float xtrap, float *coef_dev, int64_t ldcoef, float *cov_dev, int64_t ldcov, int32_t *status, double *info,
                                    void *stream)
{
    return fit_many_cov_call<float>(true, {ndim, nbatch, offsets, xdata_dev, l1xdat, ydata_dev, wdata_dev, xmin, xmax, nodes, xtrap}, coef_dev,
                                    ldcoef, cov_dev, ldcov, status, info, stream);
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
