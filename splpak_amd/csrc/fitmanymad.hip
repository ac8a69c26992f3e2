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
// Then the entries on host and device pointers: the call of splpak_fit_many_clip_* (any regrow is valid) with six clip numbers
// per problem; the residuals' scratch is begun, and counted in the call's allocations, here.
#include "fitmanyresid.hpp"
#include "madselect.hpp"
#include "fitmanyentry.hpp"

namespace splpak {

// The result block of a problem: the FM_* slots of the LAST fit, FM_SPARE = the fits the problem ran, then the six clip numbers.
enum { FMM_PASSES = FM_RESULT, FMM_OUT, FMM_COUNTED, FMM_S, FMM_MED, FMM_RETURNED, FMM_RESULT };

struct FitManyMadArgs {
    FitManyArgs f;                 // f.result: [nrun][FMM_RESULT]
    Grid gref;                     // the caller's order (build_grid without reorder): the residuals are evaluated in it
    double klo, khi;
    int maxpass, regrow;
    double *t;                     // the weighted residuals of a pass, one per point of the batch's span (the calling thread's scratch)
    long long tbase;               // point i of the arrays (global index minus f.base) has t[i - tbase]
};

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
        const Problem pr = problem_of(a.f, r);
        const long long p0 = pr.p0, np = pr.np;
        const bool weighted = starting_weights<T, NT>(wdata, wout, p0, np);
        T *out = coef + pr.slot() * a.f.ldcoef;
        double *tp = a.t + (p0 - a.tbase);

        FitOutcome o;
        int fits = 0, passes = 0;
        double nout = 0.0, returned = 0.0, s = 0.0, med = 0.0;
        for (int j = 0;; ++j) {
            // (its opening barrier orders the stores to wout before its loads of them)
            o = fit_problem<D, T, NT, const T *>(a.f, L, xd, yd, wout, true, p0, np, out);
            ++fits;
            if (o.fail || j == a.maxpass) break;

            coefficients_as_stored<D, T, NT>(g, L, n);

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
            store_loop_outcome(o, fits, res);
            res[FMM_PASSES] = (double)passes;
            res[FMM_OUT] = nout;
            res[FMM_COUNTED] = o.rows;
            res[FMM_S] = s;
            res[FMM_MED] = med;
            res[FMM_RETURNED] = returned;
        }
    }
}

// the launch of fit_many_launch (fitmany.hip) on the loop's kernel: wout gets the weights each problem ended with
template <typename T>
int fit_many_mad_launch(const FitManyMadArgs &a, const T *xdata, const T *ydata, const T *wdata, T *wout, T *coef, hipStream_t st,
                        double *seconds)
{
    return many_timed_launch(a.f.sh, st, seconds, [&](int cus, unsigned *blocks) {
        return many_shape_ladder(a.f.sh, [&](auto D, auto NT) {
            return many_launch(fit_many_mad_kernel<D(), T, NT()>, NT(), (size_t)a.f.sh.bytes, a.f.nrun, cus, st, blocks, a, xdata, ydata, wdata,
                               wout, coef);
        });
    });
}

template <typename T>
int32_t fit_many_mad_call(bool dev, const FitManyIn<T> &in, double klo, double khi, int32_t maxpass, int32_t regrow, T *wout, T *coef,
                          int64_t ldcoef, int32_t *status, double *info, double *clip, void *stream)
{
    FitManyCall<T> c{in, dev, (hipStream_t)stream, coef, ldcoef, status, info, "a batch of clipped fits"};
    c.has_wout = true;
    c.wout = wout;
    c.nextra = FMM_RESULT - FM_RESULT;
    c.extra = clip;
    c.refusal = clip_refusal(wout, in.wdata, maxpass, klo, khi);
    return fit_many_entry(c, [&](const FitManyArgs &f, const T *xd, const T *yd, const T *wd, T *wo, T *cd, T *, long long, hipStream_t st,
                                 double *seconds) {
        // the residuals of the span's points in the calling thread's scratch, held to the end of the launch (which waits for it)
        const ManySpan sp = many_span(in.offsets, in.nbatch);
        const size_t need_t[1] = {sizeof(double) * (size_t)sp.n};
        const long long allocs_before = t_fit_many_mad_t.allocs;
        const ScratchUse<1> use_t{t_fit_many_mad_t, st};
        const hipError_t e = scratch_begin(t_fit_many_mad_t, need_t, st);
        t_fit_many_stats[6] += t_fit_many_mad_t.allocs - allocs_before;
        if (e != hipSuccess) return (int)many_status(e, c.what, 0);
        FitManyMadArgs a{};
        a.f = f;
        if (int r = fit_many_grid(in, false, a.gref)) return r;
        a.klo = klo;
        a.khi = khi;
        a.maxpass = maxpass;
        a.regrow = regrow != 0;
        a.t = t_fit_many_mad_t.as<double>(0);
        a.tbase = sp.lo - f.base;
        return fit_many_mad_launch<T>(a, xd, yd, wd, wo, cd, st, seconds);
    });
}

}  // namespace

}  // namespace splpak

using namespace splpak;

extern "C" {

int32_t splpak_fit_many_clip_mad_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xdata, int32_t l1xdat,
                                     const double *ydata, const double *wdata, const double *xmin, const double *xmax, const int32_t *nodes,
                                     double xtrap, double klo, double khi, int32_t maxpass, int32_t regrow, double *wout, double *coef,
                                     int64_t ldcoef, int32_t *status, double *info, double *clip)
{
    return fit_many_mad_call<double>(false, {ndim, nbatch, offsets, xdata, l1xdat, ydata, wdata, xmin, xmax, nodes, xtrap}, klo, khi, maxpass, regrow,
                                     wout, coef, ldcoef, status, info, clip, nullptr);
}

int32_t splpak_fit_many_clip_mad_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xdata, int32_t l1xdat,
                                     const float *ydata, const float *wdata, const float *xmin, const float *xmax, const int32_t *nodes,
                                     float xtrap, float klo, float khi, int32_t maxpass, int32_t regrow, float *wout, float *coef, int64_t ldcoef,
                                     int32_t *status, double *info, double *clip)
{
    return fit_many_mad_call<float>(false, {ndim, nbatch, offsets, xdata, l1xdat, ydata, wdata, xmin, xmax, nodes, xtrap}, klo, khi, maxpass, regrow,
                                    wout, coef, ldcoef, status, info, clip, nullptr);
}

int32_t splpak_fit_many_clip_mad_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets, const double *xdata_dev, int32_t l1xdat,
                                         const double *ydata_dev, const double *wdata_dev, const double *xmin, const double *xmax,
                                         const int32_t *nodes, double xtrap, double klo, double khi, int32_t maxpass, int32_t regrow,
                                         double *wout_dev, double *coef_dev, int64_t ldcoef, int32_t *status, double *info, double *clip,
                                         void *stream)
{
    return fit_many_mad_call<double>(true, {ndim, nbatch, offsets, xdata_dev, l1xdat, ydata_dev, wdata_dev, xmin, xmax, nodes, xtrap}, klo, khi,
                                     maxpass, regrow, wout_dev, coef_dev, ldcoef, status, info, clip, stream);
}

int32_t splpak_fit_many_clip_mad_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets, const float *xdata_dev, int32_t l1xdat,
                                         const float *ydata_dev, const float *wdata_dev, const float *xmin, const float *xmax,
                                         const int32_t *nodes, float xtrap, float klo, float khi, int32_t maxpass, int32_t regrow,
                                         float *wout_dev, float *coef_dev, int64_t ldcoef, int32_t *status, double *info, double *clip,
                                         void *stream)
{
    return fit_many_mad_call<float>(true, {ndim, nbatch, offsets, xdata_dev, l1xdat, ydata_dev, wdata_dev, xmin, xmax, nodes, xtrap}, klo, khi,
                                    maxpass, regrow, wout_dev, coef_dev, ldcoef, status, info, clip, stream);
}

}  // extern "C"
