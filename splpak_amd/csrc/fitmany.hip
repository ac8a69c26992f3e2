// Many small independent fits on one node grid: splpak_fit_many_* (include/splpak_hip.h).  One workgroup takes a problem
// from its points to its coefficients (fitmanydev.hpp: fit_problem, its phases and its LDS); a batch is ONE launch whose
// workgroups stride over the problems.
#include "fitmanydev.hpp"
#include "../../include/splpak_hip.h"

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
        const int k = a.plist[r];
        const long long p0 = a.offsets[k] - a.base, np = a.offsets[k + 1] - a.offsets[k];
        const bool weighted = wd != nullptr && (double)wd[p0] >= 0.0;      // :581-588, :796
        T *out = coef + (long long)(a.compact ? r : k) * a.ldcoef;
        const FitOutcome o = fit_problem<D, T, NT, const T *__restrict__>(a, L, xd, yd, wd, weighted, p0, np, out);
        if (threadIdx.x == 0) store_outcome(o, a.result + (long long)r * FM_RESULT);
    }
}

// one shape of the launch: as many workgroups as fit on the device at once, or one per problem if that is fewer
template <int D, typename T, int NT>
hipError_t launch_shape(const FitManyArgs &a, const T *xdata, const T *ydata, const T *wdata, T *coef, int cus, hipStream_t st, unsigned *blocks)
{
    const size_t lds = (size_t)a.sh.bytes;
    *blocks = many_blocks(fit_many_kernel<D, T, NT>, NT, lds, a.nrun, cus);
    hipLaunchKernelGGL((fit_many_kernel<D, T, NT>), dim3(*blocks), dim3(NT), lds, st, a, xdata, ydata, wdata, coef);
    return hipGetLastError();
}

}  // namespace

template <typename T>
int fit_many_launch(const FitManyArgs &a, const T *xdata, const T *ydata, const T *wdata, T *coef, hipStream_t st, double *seconds)
{
    // A grid of at most FITMANY_SMALL_NCOL nodes has no work for more than one wave (a thread per band row): its workgroups are
    // one wave, so that four times as many problems are in flight on a CU.  The shape depends on the grid alone.
    const bool small = a.sh.ncol <= FITMANY_SMALL_NCOL;
    return many_timed_launch(a.sh, st, seconds, [&](int cus, unsigned *blocks) {
        if (a.g.ndim == 1 && small) return launch_shape<1, T, 64>(a, xdata, ydata, wdata, coef, cus, st, blocks);
        if (a.g.ndim == 1) return launch_shape<1, T, FITMANY_THREADS>(a, xdata, ydata, wdata, coef, cus, st, blocks);
        if (small) return launch_shape<2, T, 64>(a, xdata, ydata, wdata, coef, cus, st, blocks);
        return launch_shape<2, T, FITMANY_THREADS>(a, xdata, ydata, wdata, coef, cus, st, blocks);
    });
}

template int fit_many_launch<double>(const FitManyArgs &, const double *, const double *, const double *, double *, hipStream_t, double *);
template int fit_many_launch<float>(const FitManyArgs &, const float *, const float *, const float *, float *, hipStream_t, double *);

}  // namespace splpak
