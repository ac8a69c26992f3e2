// The batch of small fits with the covariance of its coefficients: splpak_fit_many_cov_* (include/splpak_hip.h).  The kernel
// is fit_many_kernel (fitmany.hip) with phase 6 of fit_problem switched on (fitmanydev.hpp: selected_inverse): the workgroup
// that fitted a problem turns the band factor it still holds in LDS into the band of N^-1, in place, and writes the half
// stencil of every node to `cov`.  The LDS map, the workgroup shapes and the launch are those of the plain fit.
#include "fitmanydev.hpp"
#include "../../include/splpak_hip.h"

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
        const int k = a.plist[r];
        const long long p0 = a.offsets[k] - a.base, np = a.offsets[k + 1] - a.offsets[k];
        const bool weighted = wd != nullptr && (double)wd[p0] >= 0.0;      // :581-588, :796
        const long long slot = a.compact ? r : k;
        const FitOutcome o = fit_problem<D, T, NT, const T *__restrict__, true>(a, L, xd, yd, wd, weighted, p0, np, coef + slot * a.ldcoef,
                                                                                cov + slot * ldcov);
        if (threadIdx.x == 0) store_outcome(o, a.result + (long long)r * FM_RESULT);
    }
}

template <int D, typename T, int NT>
hipError_t launch_shape(const FitManyArgs &a, const T *xdata, const T *ydata, const T *wdata, T *coef, T *cov, long long ldcov, int cus,
                        hipStream_t st, unsigned *blocks)
{
    const size_t lds = (size_t)a.sh.bytes;
    *blocks = many_blocks(fit_many_cov_kernel<D, T, NT>, NT, lds, a.nrun, cus);
    hipLaunchKernelGGL((fit_many_cov_kernel<D, T, NT>), dim3(*blocks), dim3(NT), lds, st, a, xdata, ydata, wdata, coef, cov, ldcov);
    return hipGetLastError();
}

}  // namespace

template <typename T>
int fit_many_cov_launch(const FitManyArgs &a, const T *xdata, const T *ydata, const T *wdata, T *coef, T *cov, long long ldcov, hipStream_t st,
                        double *seconds)
{
    // the 2-D phase gives a lane of one wave to every entry of a column: hb + 1 <= 64 (the LDS rule admits 40 at the most)
    if (a.g.ndim == 2 && a.sh.hb + 1 > 64) { set_error("the band is wider than a wave: no covariance for this grid"); return SPLPAK_E_UNSUPPORTED; }
    const bool small = a.sh.ncol <= FITMANY_SMALL_NCOL;      // the shapes of fit_many_launch
    return many_timed_launch(a.sh, st, seconds, [&](int cus, unsigned *blocks) {
        if (a.g.ndim == 1 && small) return launch_shape<1, T, 64>(a, xdata, ydata, wdata, coef, cov, ldcov, cus, st, blocks);
        if (a.g.ndim == 1) return launch_shape<1, T, FITMANY_THREADS>(a, xdata, ydata, wdata, coef, cov, ldcov, cus, st, blocks);
        if (small) return launch_shape<2, T, 64>(a, xdata, ydata, wdata, coef, cov, ldcov, cus, st, blocks);
        return launch_shape<2, T, FITMANY_THREADS>(a, xdata, ydata, wdata, coef, cov, ldcov, cus, st, blocks);
    });
}

template int fit_many_cov_launch<double>(const FitManyArgs &, const double *, const double *, const double *, double *, double *, long long,
                                         hipStream_t, double *);
template int fit_many_cov_launch<float>(const FitManyArgs &, const float *, const float *, const float *, float *, float *, long long, hipStream_t,
                                        double *);

}  // namespace splpak
