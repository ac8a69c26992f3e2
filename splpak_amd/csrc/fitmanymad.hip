// Robustly clipped batch fits: splpak_fit_many_clip_mad_* (include/splpak_hip.h states the rule).  The sibling of
// fitmanyclip.hip: the workgroup that owns a problem runs the whole loop on it -- fit (fitmanydev.hpp: fit_problem), weighted
// residuals, their median and MAD, decide, fit again -- until a pass changes no weight between zero and non-zero, the scale
// is 0 or the pass limit is reached, and then moves on to its next problem: one launch for the batch, the launch shapes of
// fit_many_kernel, no work queue.  The bits are those of the loop splpak_fit_many_* -> splpak_residuals_many_* -> t = w0 resid
// -> splpak_mad_many_* -> the rule on the host -> splpak_fit_many_* ...:
//   the fit        fit_problem on the weights in `wout`, exactly as fit_many_kernel runs it;
//   t              formed ONCE per pass for every point with w0 != 0 (fitmanyresid.hpp: the residual of
//                  splpak_residuals_many_*, on the coefficients as stored) and kept as a double per point in a.t, the calling
//                  thread's device scratch (10^3 points: 8 KB, which stays in L2);
//   med, MAD       madselect.hpp on those doubles over the points with wout != 0: 8 sweeps each, one more where an even count
//                  needs the next key above; |t - med| is formed on the fly.  The histogram sits at the head of the stage area,
//                  free between two fits: no LDS beyond the fit's;
//   the weights    written to `wout` in the decide step and read back by the next fit's stage_chunk; a.t likewise goes from its
//                  writer to other threads of the workgroup: global round trips inside the workgroup, ordered by barriers.
//                  `wout` and a.t are therefore plain pointers here, and w0 is read again from `wdata` (never written).
// No floating-point atomics; the selection's counts are integers.
#include "fitmanyresid.hpp"
#include "madselect.hpp"

namespace splpak {

namespace {

using namespace fitmanydev;
using namespace madselect;

// every operation of the rule below is rounded on its own (the fit and the factor tables come from the headers above)
#pragma clang fp contract(off)

constexpr double MAD_TO_SIGMA = 1.482602218505602;

static_assert(MEDIAN_LDS_WORDS * 4 <= FITMANY_CHUNK * 6 * 8, "the selection's words fit the stage area of a 1-D fit");

// The waves per SIMD of fit_many_kernel are asked for, as fit_many_clip_kernel does.
template <int D, typename T, int NT>
__global__ void __launch_bounds__(NT, D == 2 ? 2 : 4)
fit_many_mad_kernel(FitManyMadArgs a, const T *__restrict__ xd, const T *__restrict__ yd, const T *__restrict__ wdata, T *wout,
                    T *__restrict__ coef)
{
    extern __shared__ double fit_many_mad_lds[];
    const Lds L = carve(fit_many_mad_lds, a.f.sh);
    const Grid &g = a.f.g;
    const int tid = threadIdx.x, n = a.f.sh.ncol, l1xdat = a.f.l1xdat;
    unsigned *sel = reinterpret_cast<unsigned *>(L.stage);

    for (int r = blockIdx.x; r < a.f.nrun; r += gridDim.x) {
        const int k = a.f.plist[r];
        const long long p0 = a.f.offsets[k] - a.f.base, np = a.f.offsets[k + 1] - a.f.offsets[k];
        // the starting weights; the first-weight decision is taken here, from wdata, and never again
        const bool weighted = wdata != nullptr && (double)wdata[p0] >= 0.0;
        for (long long p = tid; p < np; p += NT) wout[p0 + p] = weighted ? wdata[p0 + p] : (T)1;
        T *out = coef + (long long)(a.f.compact ? r : k) * a.f.ldcoef;
        double *tp = a.t + (p0 - a.tbase);

        FitOutcome o;
        int fits = 0, passes = 0;
        double nout = 0.0, returned = 0.0, s = 0.0, med = 0.0;
        for (int j = 0;; ++j) {
            // (its opening barrier orders the stores to wout before its loads of them)
            o = fit_problem<D, T, NT, const T *>(a.f, L, xd, yd, wout, true, p0, np, out);
            ++fits;
            if (o.fail || j == a.maxpass) break;

            // the coefficients as stored: rounded to T, in the caller's node order
            for (int i = tid; i < n; i += NT) {
                int in[D], refnode = 0;
                node_of<D>(g, i, in);
#pragma unroll
                for (int d = 0; d < D; ++d) refnode += in[d] * g.refstride[d];
                L.rho[refnode] = (double)(T)L.x[i];
            }
            __syncthreads();

            // t of every point with w0 != 0 (a point of weight 0 is selected out, never multiplied), and the points counted
            int cnt_mine = 0;
            for (long long p = tid; p < np; p += NT) {
                const long long i = p0 + p;
                const double w0 = weighted ? (double)wdata[i] : 1.0;
                if (w0 == 0.0) continue;
                tp[p] = weighted_residual<D, T>(a.gref, xd, l1xdat, yd, i, w0, L.rho);
                cnt_mine += (double)wout[i] != 0.0 ? 1 : 0;
            }
            // (its barriers also order the stores to tp before the selection's loads)
            const unsigned cnt = (unsigned)block_reduce<false, NT>((double)cnt_mine, L.stage);
            // (nothing counted, all weights 0 under xtrap != 0: med = MAD = 0 as splpak_mad_many_* says, and the loop stops on s == 0)
            med = cnt == 0 ? 0.0 : select_median<NT>(sel, np, cnt, [&](long long p, unsigned long long &key) {
                if ((double)wout[p0 + p] == 0.0) return false;
                key = median_key(tp[p] + 0.0);
                return true;
            });
            const double mad = cnt == 0 ? 0.0 : select_median<NT>(sel, np, cnt, [&](long long p, unsigned long long &key) {
                if ((double)wout[p0 + p] == 0.0) return false;
                const double kv = tp[p] + 0.0;
                key = median_key(fabs(kv - med));
                return true;
            });
            s = MAD_TO_SIGMA * mad;
            ++passes;
            if (s == 0.0) break;

            // decide
            const double hi = a.khi * s, lo = a.klo * s;
            int changed = 0, back = 0, zeros = 0;
            for (long long p = tid; p < np; p += NT) {
                const long long i = p0 + p;
                const double w0 = weighted ? (double)wdata[i] : 1.0;
                if (w0 == 0.0) continue;
                const bool was = (double)wout[i] != 0.0;
                bool now = was;
                if (was || a.regrow) {
                    const double e = (tp[p] + 0.0) - med;
                    now = !(e > hi || -e > lo);
                    wout[i] = now ? (T)w0 : (T)0;
                }
                changed += now != was ? 1 : 0;
                back += now && !was ? 1 : 0;
                zeros += now ? 0 : 1;
            }
            const double nchanged = block_reduce<false, NT>((double)changed, L.stage);
            returned += block_reduce<false, NT>((double)back, L.stage);
            nout = block_reduce<false, NT>((double)zeros, L.stage);
            if (nchanged == 0.0) break;
        }

        if (tid == 0) {
            double *res = a.f.result + (long long)r * FMM_RESULT;
            store_outcome(o, res);
            res[FM_SPARE] = (double)fits;
            res[FMM_PASSES] = (double)passes;
            res[FMM_OUT] = nout;
            res[FMM_COUNTED] = o.rows;
            res[FMM_S] = s;
            res[FMM_MED] = med;
            res[FMM_RETURNED] = returned;
        }
    }
}

template <int D, typename T, int NT>
hipError_t launch_shape(const FitManyMadArgs &a, const T *xdata, const T *ydata, const T *wdata, T *wout, T *coef, int cus, hipStream_t st,
                        unsigned *blocks)
{
    const size_t lds = (size_t)a.f.sh.bytes;
    *blocks = many_blocks(fit_many_mad_kernel<D, T, NT>, NT, lds, a.f.nrun, cus);
    hipLaunchKernelGGL((fit_many_mad_kernel<D, T, NT>), dim3(*blocks), dim3(NT), lds, st, a, xdata, ydata, wdata, wout, coef);
    return hipGetLastError();
}

}  // namespace

template <typename T>
int fit_many_mad_launch(const FitManyMadArgs &a, const T *xdata, const T *ydata, const T *wdata, T *wout, T *coef, hipStream_t st,
                        double *seconds)
{
    const bool small = a.f.sh.ncol <= FITMANY_SMALL_NCOL;      // fit_many_launch's shapes
    return many_timed_launch(a.f.sh, st, seconds, [&](int cus, unsigned *blocks) {
        if (a.f.g.ndim == 1 && small) return launch_shape<1, T, 64>(a, xdata, ydata, wdata, wout, coef, cus, st, blocks);
        if (a.f.g.ndim == 1) return launch_shape<1, T, FITMANY_THREADS>(a, xdata, ydata, wdata, wout, coef, cus, st, blocks);
        if (small) return launch_shape<2, T, 64>(a, xdata, ydata, wdata, wout, coef, cus, st, blocks);
        return launch_shape<2, T, FITMANY_THREADS>(a, xdata, ydata, wdata, wout, coef, cus, st, blocks);
    });
}

template int fit_many_mad_launch<double>(const FitManyMadArgs &, const double *, const double *, const double *, double *, double *,
                                         hipStream_t, double *);
template int fit_many_mad_launch<float>(const FitManyMadArgs &, const float *, const float *, const float *, float *, float *, hipStream_t,
                                        double *);

}  // namespace splpak
