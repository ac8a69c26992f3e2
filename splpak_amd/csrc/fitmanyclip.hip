// Sigma-clipped batch fits: splpak_fit_many_clip_* (include/splpak_hip.h states the rule).  The workgroup that owns a problem
// runs the whole loop on it -- fit (fitmanydev.hpp: fit_problem), residuals, reject, fit again -- until a pass rejects nothing
// or the pass limit is reached, and then moves on to its next problem: one launch for the batch, the launch shapes of
// fit_many_kernel, no work queue, no atomics.  The bits are those of the loop splpak_fit_many_* -> splpak_residuals_many_* ->
// the rule on the host -> splpak_fit_many_* ...:
//   the fit        fit_problem on the weights in `wout`, exactly as fit_many_kernel runs it;
//   the residuals  the factor tables and window_sum of evalcore.hpp on the grid in the CALLER's order (the fit's own grid is
//                  reordered, which would change the order of the 2-D sum), the window rows read from LDS: after a fit L.rho is
//                  free and gets (double)(T) x in the caller's node order, the very values eval_point loads from `coef`;
//   S              all threads form t*t of a staged chunk of 128 points, then lane l of wave 0 adds entries l and l + 64 of
//                  every chunk in ascending order -- p = l, l + 64, l + 128, .. as residuals_many_kernel's one wave adds them --
//                  and the 64 lane sums go through wave_sum's butterfly: the same order whatever the workgroup size;
//   the mask       written to `wout` in the reject step and read back by the next fit's stage_chunk: a global round trip inside
//                  the workgroup, ordered by the barrier fit_problem opens with.  `wout` is therefore a plain pointer here and the
//                  first-weight decision is taken once, from `wdata`, before the loop.
// r is formed twice per pass (the reject step needs v first).
// Then the entries on host and device pointers: the call of splpak_fit_many_* (fitmanyentry.hpp) with the four clip conditions
// in its second SPLPAK_E_BADARG group, `wout` beside the span and four clip numbers per problem.
#include "fitmanyresid.hpp"
#include "fitmanyentry.hpp"

namespace splpak {

// The result block of a problem: the FM_* slots of the LAST fit, FM_SPARE = the fits the problem ran, then the four clip numbers.
enum { FMC_PASSES = FM_RESULT, FMC_REJECTED, FMC_COUNTED, FMC_V, FMC_RESULT };

struct FitManyClipArgs {
    FitManyArgs f;                 // f.result: [nrun][FMC_RESULT]
    Grid gref;                     // the caller's order (build_grid without reorder): the residuals are evaluated in it
    double klo2, khi2;             // klo^2, khi^2, formed once in double
    int maxpass;
};

namespace {

using namespace fitmanydev;

// every operation of the rule below is rounded on its own (the fit and the factor tables come from the headers above)
#pragma clang fp contract(off)

// The waves per SIMD of fit_many_kernel are asked for (2-D: 2, 1-D: 4): the loop's state beside the fit's would otherwise take
// 258 registers in the 2-D 256-thread shape (one workgroup per CU instead of two) and 158 in 1-D (3 waves per SIMD instead of
// 4).  The compiler spills 2 registers (2-D) and 17 to 30 (1-D) for it; measured, 1-D: 10^5 problems in 64 ms instead of 80.
template <int D, typename T, int NT>
__global__ void __launch_bounds__(NT, D == 2 ? 2 : 4)
fit_many_clip_kernel(FitManyClipArgs a, const T *__restrict__ xd, const T *__restrict__ yd, const T *__restrict__ wdata, T *wout,
                     T *__restrict__ coef)
{
    extern __shared__ double fit_many_clip_lds[];
    const Lds L = carve(fit_many_clip_lds, a.f.sh);
    const Grid &g = a.f.g;
    const int tid = threadIdx.x, n = a.f.sh.ncol, l1xdat = a.f.l1xdat;

    for (int r = blockIdx.x; r < a.f.nrun; r += gridDim.x) {
        const Problem pr = problem_of(a.f, r);
        const long long p0 = pr.p0, np = pr.np;
        starting_weights<T, NT>(wdata, wout, p0, np);
        T *out = coef + pr.slot() * a.f.ldcoef;

        FitOutcome o;
        int fits = 0, passes = 0;
        double rejected = 0.0, v = 0.0;
        for (int j = 0;; ++j) {
            // (its opening barrier orders the stores to wout before its loads of them)
            o = fit_problem<D, T, NT, const T *>(a.f, L, xd, yd, wout, true, p0, np, out);
            ++fits;
            if (o.fail || j == a.maxpass) break;

            coefficients_as_stored<D, T, NT>(g, L, n);

            // cnt and S over the points of non-zero weight
            double acc = 0.0;
            int cnt = 0;
            for (long long c0 = 0; c0 < np; c0 += FITMANY_CHUNK) {
                const int cntc = (int)(np - c0 < FITMANY_CHUNK ? np - c0 : FITMANY_CHUNK);
                for (int t = tid; t < FITMANY_CHUNK; t += NT) {
                    double tt = 0.0;
                    int counted = 0;
                    if (t < cntc) {
                        const long long i = p0 + c0 + t;
                        const double w = (double)wout[i];
                        if (w != 0.0) {      // a point of weight 0 is selected out, never multiplied
                            const double tw = weighted_residual<D, T>(a.gref, xd, l1xdat, yd, i, w, L.rho);
                            tt = tw * tw;
                            counted = 1;
                        }
                    }
                    L.stage[t] = tt;
                    L.addr[t] = counted;
                }
                __syncthreads();
                if (tid < 64) {
                    for (int e = tid; e < FITMANY_CHUNK; e += 64)
                        if (L.addr[e]) { acc = acc + L.stage[e]; ++cnt; }
                }
                __syncthreads();
            }
            if (tid < 64) {
                const double s = wave_sum(acc);
#pragma unroll
                for (int q = 32; q > 0; q >>= 1) cnt += __shfl_xor(cnt, q, 64);
                if (tid == 0) { L.scal[1] = s; L.scal[2] = (double)cnt; }
            }
            __syncthreads();
            v = L.scal[1] / L.scal[2];
            ++passes;

            // reject; rejected points never return
            const double hi = a.khi2 * v, lo = a.klo2 * v;
            int nrej = 0;
            for (long long p = tid; p < np; p += NT) {
                const long long i = p0 + p;
                const double w = (double)wout[i];
                if (w == 0.0) continue;
                const double tw = weighted_residual<D, T>(a.gref, xd, l1xdat, yd, i, w, L.rho);
                const double tt = tw * tw;
                if ((tw > 0.0 && tt > hi) || (tw < 0.0 && tt > lo)) { wout[i] = (T)0; ++nrej; }
            }
            const double rej = block_reduce<false, NT>((double)nrej, L.stage);
            rejected += rej;
            if (rej == 0.0) break;
        }

        if (tid == 0) {
            double *res = a.f.result + (long long)r * FMC_RESULT;
            store_loop_outcome(o, fits, res);
            res[FMC_PASSES] = (double)passes;
            res[FMC_REJECTED] = rejected;
            res[FMC_COUNTED] = o.rows;
            res[FMC_V] = v;
        }
    }
}

// the launch of fit_many_launch (fitmany.hip) on the loop's kernel: wout gets the weights each problem ended with
template <typename T>
int fit_many_clip_launch(const FitManyClipArgs &a, const T *xdata, const T *ydata, const T *wdata, T *wout, T *coef, hipStream_t st,
                         double *seconds)
{
    return many_timed_launch(a.f.sh, st, seconds, [&](int cus, unsigned *blocks) {
        return many_shape_ladder(a.f.sh, [&](auto D, auto NT) {
            return many_launch(fit_many_clip_kernel<D(), T, NT()>, NT(), (size_t)a.f.sh.bytes, a.f.nrun, cus, st, blocks, a, xdata, ydata, wdata,
                               wout, coef);
        });
    });
}

template <typename T>
int32_t fit_many_clip_call(bool dev, const FitManyIn<T> &in, double klo, double khi, int32_t maxpass, T *wout, T *coef, int64_t ldcoef,
                           int32_t *status, double *info, double *clip, void *stream)
{
    FitManyCall<T> c{in, dev, (hipStream_t)stream, coef, ldcoef, status, info, "a batch of clipped fits"};
    c.has_wout = true;
    c.wout = wout;
    c.nextra = FMC_RESULT - FM_RESULT;
    c.extra = clip;
    c.refusal = clip_refusal(wout, in.wdata, maxpass, klo, khi);
    return fit_many_entry(c, [&](const FitManyArgs &f, const T *xd, const T *yd, const T *wd, T *wo, T *cd, T *, long long, hipStream_t st,
                                 double *seconds) {
        FitManyClipArgs a{};
        a.f = f;
        // the residuals are evaluated on the grid in the caller's order (it was valid in the checks)
        if (int r = fit_many_grid(in, false, a.gref)) return r;
        a.klo2 = klo * klo;
        a.khi2 = khi * khi;
        a.maxpass = maxpass;
        return fit_many_clip_launch<T>(a, xd, yd, wd, wo, cd, st, seconds);
    });
}

}  // namespace

}  // namespace splpak

using namespace splpak;

extern "C" {

int32_t splpak_fit_many_clip_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xdata, int32_t l1xdat,
                                 const double *ydata, const double *wdata, const double *xmin, const double *xmax, const int32_t *nodes,
                                 double xtrap, double klo, double khi, int32_t maxpass, double *wout, double *coef, int64_t ldcoef,
                                 int32_t *status, double *info, double *clip)
{
    return fit_many_clip_call<double>(false, {ndim, nbatch, offsets, xdata, l1xdat, ydata, wdata, xmin, xmax, nodes, xtrap}, klo, khi, maxpass, wout,
                                      coef, ldcoef, status, info, clip, nullptr);
}

int32_t splpak_fit_many_clip_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xdata, int32_t l1xdat, const float *ydata,
                                 const float *wdata, const float *xmin, const float *xmax, const int32_t *nodes, float xtrap, float klo,
                                 float khi, int32_t maxpass, float *wout, float *coef, int64_t ldcoef, int32_t *status, double *info,
                                 double *clip)
{
    return fit_many_clip_call<float>(false, {ndim, nbatch, offsets, xdata, l1xdat, ydata, wdata, xmin, xmax, nodes, xtrap}, klo, khi, maxpass, wout,
                                     coef, ldcoef, status, info, clip, nullptr);
}

int32_t splpak_fit_many_clip_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xdata_dev, int32_t l1xdat,
                                     const double *ydata_dev, const double *wdata_dev, const double *xmin, const double *xmax,
                                     const int32_t *nodes, double xtrap, double klo, double khi, int32_t maxpass, double *wout_dev,
                                     double *coef_dev, int64_t ldcoef, int32_t *status, double *info, double *clip, void *stream)
{
    return fit_many_clip_call<double>(true, {ndim, nbatch, offsets, xdata_dev, l1xdat, ydata_dev, wdata_dev, xmin, xmax, nodes, xtrap}, klo, khi,
                                      maxpass, wout_dev, coef_dev, ldcoef, status, info, clip, stream);
}

int32_t splpak_fit_many_clip_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xdata_dev, int32_t l1xdat,
                                     const float *ydata_dev, const float *wdata_dev, const float *xmin, const float *xmax,
                                     const int32_t *nodes, float xtrap, float klo, float khi, int32_t maxpass, float *wout_dev,
                                     float *coef_dev, int64_t ldcoef, int32_t *status, double *info, double *clip, void *stream)
{
    return fit_many_clip_call<float>(true, {ndim, nbatch, offsets, xdata_dev, l1xdat, ydata_dev, wdata_dev, xmin, xmax, nodes, xtrap}, klo, khi,
                                     maxpass, wout_dev, coef_dev, ldcoef, status, info, clip, stream);
}

}  // extern "C"
