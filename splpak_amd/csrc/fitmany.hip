// Many small independent fits on one node grid: splpak_fit_many_* (include/splpak_hip.h) on host and device pointers, the
// LDS rule and the counters.  One workgroup takes a problem from its points to its coefficients (fitmanydev.hpp: fit_problem,
// its phases and its LDS); a batch is ONE launch whose workgroups stride over the problems.  The host side of a call:
// fitmanyentry.hpp.
#include "fitmanydev.hpp"
#include "fitmanyentry.hpp"

namespace splpak {

thread_local long long t_fit_many_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

namespace {

using namespace fitmanydev;

template <int D, typename T, int NT>
__global__ void __launch_bounds__(NT)
fit_many_kernel(FitManyArgs a, const T *__restrict__ xd, const T *__restrict__ yd, const T *__restrict__ wd, T *__restrict__ coef)
{
    extern __shared__ double fit_many_lds[];
    const Lds L = carve(fit_many_lds, a.sh);

    for (int r = blockIdx.x; r < a.nrun; r += gridDim.x) {
        const Problem p = problem_of(a, r);
        const bool weighted = first_weight_counts(wd, p.p0);
        T *out = coef + p.slot() * a.ldcoef;
        const FitOutcome o = fit_problem<D, T, NT, const T *__restrict__>(a, L, xd, yd, wd, weighted, p.p0, p.np, out);
        if (threadIdx.x == 0) store_outcome(o, a.result + (long long)r * FM_RESULT);
    }
}

// the device part on device arrays: one launch.  0 or SPLPAK_E_*; *seconds = the launch's device time
template <typename T>
int fit_many_launch(const FitManyArgs &a, const T *xdata, const T *ydata, const T *wdata, T *coef, hipStream_t st, double *seconds)
{
    return many_timed_launch(a.sh, st, seconds, [&](int cus, unsigned *blocks) {
        return many_shape_ladder(a.sh, [&](auto D, auto NT) {
            return many_launch(fit_many_kernel<D(), T, NT()>, NT(), (size_t)a.sh.bytes, a.nrun, cus, st, blocks, a, xdata, ydata, wdata, coef);
        });
    });
}

template <typename T>
int32_t fit_many_call(bool dev, const FitManyIn<T> &in, T *coef, int64_t ldcoef, int32_t *status, double *info, void *stream)
{
    const FitManyCall<T> c{in, dev, (hipStream_t)stream, coef, ldcoef, status, info, "a batch of fits"};
    return fit_many_entry(c, [](const FitManyArgs &a, const T *xd, const T *yd, const T *wd, T *, T *cd, T *, long long, hipStream_t st,
                                double *seconds) { return fit_many_launch<T>(a, xd, yd, wd, cd, st, seconds); });
}

}  // namespace

}  // namespace splpak

using namespace splpak;

extern "C" {

int32_t splpak_fit_many_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xdata, int32_t l1xdat, const double *ydata,
                            const double *wdata, const double *xmin, const double *xmax, const int32_t *nodes, double xtrap, double *coef,
                            int64_t ldcoef, int32_t *status, double *info)
{
    return fit_many_call<double>(false, {ndim, nbatch, offsets, xdata, l1xdat, ydata, wdata, xmin, xmax, nodes, xtrap}, coef, ldcoef, status, info,
                                 nullptr);
}

int32_t splpak_fit_many_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xdata, int32_t l1xdat, const float *ydata,
                            const float *wdata, const float *xmin, const float *xmax, const int32_t *nodes, float xtrap, float *coef,
                            int64_t ldcoef, int32_t *status, double *info)
{
    return fit_many_call<float>(false, {ndim, nbatch, offsets, xdata, l1xdat, ydata, wdata, xmin, xmax, nodes, xtrap}, coef, ldcoef, status, info,
                                nullptr);
}

int32_t splpak_fit_many_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xdata_dev, int32_t l1xdat,
                                const double *ydata_dev, const double *wdata_dev, const double *xmin, const double *xmax, const int32_t *nodes,
                                double xtrap, double *coef_dev, int64_t ldcoef, int32_t *status, double *info, void *stream)
{
    return fit_many_call<double>(true, {ndim, nbatch, offsets, xdata_dev, l1xdat, ydata_dev, wdata_dev, xmin, xmax, nodes, xtrap}, coef_dev, ldcoef,
                                 status, info, stream);
}

int32_t splpak_fit_many_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xdata_dev, int32_t l1xdat,
                                const float *ydata_dev, const float *wdata_dev, const float *xmin, const float *xmax, const int32_t *nodes,
                                float xtrap, float *coef_dev, int64_t ldcoef, int32_t *status, double *info, void *stream)
{
    return fit_many_call<float>(true, {ndim, nbatch, offsets, xdata_dev, l1xdat, ydata_dev, wdata_dev, xmin, xmax, nodes, xtrap}, coef_dev, ldcoef,
                                status, info, stream);
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
