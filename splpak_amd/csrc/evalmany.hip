// A batch of small fits at each problem's own points: the evaluation side of fitmany.hip.
//
// eval_many       one thread per query over the concatenated list of all problems' queries, so that 10^5 problems of 8 queries
//                 and 4 problems of 10^6 are balanced alike.  A thread finds the problem that owns its query in the uploaded
//                 offsets: a wave looks up the owner of its first query once (a uniform search); if its last query has the same
//                 owner -- the common case -- every lane takes that coefficient base, otherwise each lane searches between the
//                 owners of the wave's first and last query.  Problems without queries own no index and are never found.  From
//                 there on the thread is eval.hip's direct kernel: the factor tables of eval_table<VAL>, window_sum over rows
//                 loaded by load_window_row from ITS problem's coefficients.  Nothing is shared between problems, and how the
//                 owner was found does not enter the arithmetic: the bits are those of splpak_eval_* on that problem alone.
// residuals_many  one wave per problem, the waves stride over the problems.  The wave walks its problem's points 64 at a time:
//                 reads x, y, w once, evaluates (the value pattern of the above), writes the residual and keeps, per lane, the
//                 sum of (w r)^2 over ITS points in ascending order, the largest |w r| and where it was first seen.  The lane
//                 sums are combined by wave_sum's butterfly, the maxima by the same butterfly on (value, index) pairs.  Every
//                 multiplication and addition of the statistics is rounded on its own (contraction off), so the four numbers of
//                 a problem are a fixed sequence of IEEE double operations on its own data: no atomics, no dependence on the
//                 batch, the position or the launch shape.  A problem of very many points is walked by its one wave.
//
// eval_many_var  eval_many's sweep and owner search (wave_owners, lane_owner) with, per query, the quadratic form a^T Z a of its
//                 window row in the half stencil of its problem's covariance (var_point): 4 (1-D) or 16 (2-D) stencil rows of
//                 the problem's `cov`, 10 or 136 words of them, read from global memory once each.
//
// The coefficient sets are not staged in LDS: a 16-node set is 128 bytes and a wave's gathers stay in L1 / L2.
//
// The file also holds the per-thread device scratch of the batch entries' tables (manyhost.hpp).
#include "evalcore.hpp"
#include "manyhost.hpp"
#include "evalmany.hpp"

#include <climits>

namespace splpak {

thread_local long long t_eval_many_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

namespace {

// v of the wave's first active lane, in a scalar register
__device__ inline long long wave_uniform(long long v)
{
    const int lo = __builtin_amdgcn_readfirstlane((int)v), hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
    return ((long long)hi << 32) | (long long)(unsigned)lo;
}

// the problem k with offsets[k] <= i < offsets[k+1], given offsets[lo] <= i < offsets[hi] (problems without points own no i)
__device__ inline int owner_of(const long long *__restrict__ offsets, long long i, int lo, int hi)
{
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// eval_kernel's body (eval.hip) for the point at x[0 .. D-1 of a row], on the coefficient set cf
template <int D, typename T, bool VAL>
__device__ inline double eval_point(const Grid &g, const T *__restrict__ x, const NDeriv &nd, const T *__restrict__ cf)
{
    double b[D][4];
    int base = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double xd = (double)x[d];
        const int ws = eval_table<VAL>(g, d, xd, nd.v[d], b[d]);
        base += ws * g.colstride[d];
    }
    const int s1 = D > 1 ? g.colstride[1] : 0, s2 = D > 2 ? g.colstride[2] : 0, s3 = D > 3 ? g.colstride[3] : 0;
    return window_sum<D>(b, [&](int k1, int k2, int k3, double (&c)[4]) {
        const long long idx = base + k1 * s1 + k2 * s2 + k3 * s3;
        load_window_row(cf + idx, c);
    });
}

// The owners of a wave's queries i0 .. i1 (consecutive, i0 in a scalar register): the wave looks up the owner of i0 once; where
// i1 has the same owner every lane takes it, otherwise lane_owner searches between the two.
struct WaveOwners {
    int k0;
    bool one_owner;
};
__device__ inline WaveOwners wave_owners(const long long *__restrict__ offsets, int nbatch, long long i0, long long i1)
{
    const int k0 = owner_of(offsets, i0, 0, nbatch);
    return {k0, offsets[k0 + 1] > i1};
}
__device__ inline int lane_owner(const long long *__restrict__ offsets, int nbatch, const WaveOwners &w, long long i, long long i1)
{
    if (w.one_owner) return w.k0;
    const int k1 = owner_of(offsets, i1, w.k0, nbatch);
    return owner_of(offsets, i, w.k0, k1 + 1);
}

template <int D, typename T, bool VAL>
__global__ void __launch_bounds__(EVALMANY_THREADS)
eval_many_kernel(Grid g, int nbatch, const long long *__restrict__ offsets, long long first, long long nq, long long base,
                 const T *__restrict__ xq, int ldxq, NDeriv nd, const T *__restrict__ coef, long long ldcoef, T *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * EVALMANY_THREADS;
    // jw: the wave's first query of this sweep, counted from `first`
    for (long long jw = wave_uniform((long long)blockIdx.x * EVALMANY_THREADS + (threadIdx.x - lane)); jw < nq; jw += stride) {
        const long long i0 = first + jw, i1 = first + (jw + 63 < nq ? jw + 63 : nq - 1);
        const WaveOwners w = wave_owners(offsets, nbatch, i0, i1);
        const long long j = jw + lane;
        if (j < nq) {
            const long long i = first + j;
            const int k = lane_owner(offsets, nbatch, w, i, i1);
            const double sum = eval_point<D, T, VAL>(g, xq + (i - base) * ldxq, nd, coef + (long long)k * ldcoef);
            out[i - base] = (T)sum;
        }
    }
}

// a^T Z a for the window row a of the point at x (the products of the factors eval_point contracts the coefficients with) and
// the half stencil cv of its problem: cv[p * HST + code] = Z(p, p + o) (include/splpak_hip.h, splpak_fit_many_cov_*).  The
// window entries are numbered e = q0 (+ 4 q1), dimension 0 fastest, node p_e = base + q0 (+ q1 nodes[0]).  Order of the sum,
// part of the contract: acc = 0; for e = 0 .. 4^D - 1: r = (0.5 a_e) Z(p_e, p_e), then r = fma(a_f, Z(p_e, p_f), r) for
// f = 0 .. e - 1 ascending, then acc = fma(a_e, r, acc); the result is 2 acc.  Every symmetric pair is read once (p_f < p_e: the
// lower triangle the stencil holds).
template <int D, typename T, bool VAL>
__device__ inline double var_point(const Grid &g, const T *__restrict__ x, const NDeriv &nd, const T *__restrict__ cv)
{
    constexpr int HST = D == 1 ? 4 : 25, NB = D == 1 ? 4 : 16;
    double b[D][4];
    int base = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const int ws = eval_table<VAL>(g, d, (double)x[d], nd.v[d], b[d]);
        base += ws * g.colstride[d];
    }
    const int s1 = D > 1 ? g.colstride[1] : 0;
    double a[NB];
#pragma unroll
    for (int e = 0; e < NB; ++e) a[e] = D == 1 ? b[0][e] : b[0][e & 3] * b[D - 1][e >> 2];
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < NB; ++e) {
        const int e0 = e & 3, e1 = e >> 2;
        const T *row = cv + (long long)(base + e0 + e1 * s1) * HST;
        double r = (0.5 * a[e]) * (double)row[HST - 1];
#pragma unroll
        for (int f = 0; f < e; ++f) {
            const int code = D == 1 ? (f - e) + 3 : ((f & 3) - e0 + 3) + 7 * ((f >> 2) - e1 + 3);
            r = fma(a[f], (double)row[code], r);
        }
        acc = fma(a[e], r, acc);
    }
    return 2.0 * acc;
}

template <int D, typename T, bool VAL>
__global__ void __launch_bounds__(EVALMANY_THREADS)
eval_many_var_kernel(Grid g, int nbatch, const long long *__restrict__ offsets, long long first, long long nq, long long base,
                     const T *__restrict__ xq, int ldxq, NDeriv nd, const T *__restrict__ cov, long long ldcov, T *__restrict__ out)
{
    // eval_many_kernel's sweep and owner search
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * EVALMANY_THREADS;
    for (long long jw = wave_uniform((long long)blockIdx.x * EVALMANY_THREADS + (threadIdx.x - lane)); jw < nq; jw += stride) {
        const long long i0 = first + jw, i1 = first + (jw + 63 < nq ? jw + 63 : nq - 1);
        const WaveOwners w = wave_owners(offsets, nbatch, i0, i1);
        const long long j = jw + lane;
        if (j < nq) {
            const long long i = first + j;
            const int k = lane_owner(offsets, nbatch, w, i, i1);
            const double v = var_point<D, T, VAL>(g, xq + (i - base) * ldxq, nd, cov + (long long)k * ldcov);
            out[i - base] = (T)v;
        }
    }
}

template <int D, typename T>
__global__ void __launch_bounds__(64)
residuals_many_kernel(Grid g, int nbatch, const long long *__restrict__ offsets, long long base, const T *__restrict__ xd, int l1xdat,
                      const T *__restrict__ yd, const T *__restrict__ wd, const T *__restrict__ coef, long long ldcoef,
                      T *__restrict__ resid, double *__restrict__ stats)
{
    const int lane = threadIdx.x;
    const NDeriv nd{};
    for (int k = blockIdx.x; k < nbatch; k += gridDim.x) {
        const long long p0 = offsets[k] - base, np = offsets[k + 1] - offsets[k];
        const bool weighted = wd != nullptr && np > 0 && !((double)wd[p0] < 0.0);    // (fitmany.hip: a negative first weight = no weights; a NaN is not negative)
        const T *cf = coef + (long long)k * ldcoef;
        double acc = 0.0, mx = -1.0;
        long long mp = LLONG_MAX;
        int cnt = 0;
        for (long long p = lane; p < np; p += 64) {
            const long long i = p0 + p;
            const double f = eval_point<D, T, true>(g, xd + i * l1xdat, nd, cf);
            {
#pragma clang fp contract(off)
                const double r = (double)yd[i] - f;
                if (resid) resid[i] = (T)r;
                const double w = weighted ? (double)wd[i] : 1.0;
                if (w != 0.0) {      // a point of weight 0 is selected out, never multiplied
                    const double t = w * r;
                    const double tt = t * t;
                    acc = acc + tt;
                    const double at = fabs(t);
                    if (at > mx) { mx = at; mp = p; }
                    ++cnt;
                }
            }
        }
        if (stats == nullptr) continue;
        const double s = wave_sum(acc);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double omx = __shfl_xor(mx, o, 64);
            const long long omp = __shfl_xor(mp, o, 64);
            const bool take = omx > mx || (omx == mx && omp < mp);
            mx = take ? omx : mx;
            mp = take ? omp : mp;
            cnt += __shfl_xor(cnt, o, 64);
        }
        if (lane == 0) {
            double *sk = stats + 4LL * k;
            sk[0] = (double)cnt;
            sk[1] = cnt > 0 ? s : 0.0;
            sk[2] = cnt > 0 ? mx : 0.0;
            sk[3] = cnt > 0 ? (double)mp : -1.0;
        }
    }
}

}  // namespace

// the per-thread scratch of the batch entries (manyhost.hpp)
thread_local DevScratch<1> t_many_offsets;
thread_local DevScratch<2> t_fit_many_tables;
thread_local DevScratch<1> t_fit_many_mad_t;

void many_scratch_shutdown()
{
    t_many_offsets.release();
    t_fit_many_tables.release();
    t_fit_many_mad_t.release();
}

template <typename T>
hipError_t launch_eval_many(const Grid &g, int nbatch, const long long *offsets_dev, long long first, long long nq, long long base,
                            const T *xq, int ldxq, const int *nderiv, const T *coef, long long ldcoef, T *out, hipStream_t st)
{
    if (nq <= 0) return hipSuccess;
    const NDeriv nd = clamp_nderiv(nderiv, g.ndim);
    long long blocks = (nq + EVALMANY_THREADS - 1) / EVALMANY_THREADS;
    if (blocks > EVALMANY_BLOCKS) blocks = EVALMANY_BLOCKS;      // grid-stride the rest
    const dim3 gr((unsigned)blocks), bl(EVALMANY_THREADS);
    const bool plain = value_only(nd);
    DISPATCH_D(g.ndim, hipLaunchKernelGGL((plain ? eval_many_kernel<D, T, true> : eval_many_kernel<D, T, false>), gr, bl, 0, st, g, nbatch,
                                          offsets_dev, first, nq, base, xq, ldxq, nd, coef, ldcoef, out));
    t_eval_many_stats[0] = blocks;
    t_eval_many_stats[1] = 1;
    t_eval_many_stats[4] = blocks * EVALMANY_THREADS;
    return hipGetLastError();
}
template hipError_t launch_eval_many<double>(const Grid &, int, const long long *, long long, long long, long long, const double *, int,
                                             const int *, const double *, long long, double *, hipStream_t);
template hipError_t launch_eval_many<float>(const Grid &, int, const long long *, long long, long long, long long, const float *, int,
                                            const int *, const float *, long long, float *, hipStream_t);

template <typename T>
hipError_t launch_eval_many_var(const Grid &g, int nbatch, const long long *offsets_dev, long long first, long long nq, long long base,
                                const T *xq, int ldxq, const int *nderiv, const T *cov, long long ldcov, T *out, hipStream_t st)
{
    if (nq <= 0) return hipSuccess;
    const NDeriv nd = clamp_nderiv(nderiv, g.ndim);
    long long blocks = (nq + EVALMANY_THREADS - 1) / EVALMANY_THREADS;
    if (blocks > EVALMANY_BLOCKS) blocks = EVALMANY_BLOCKS;      // grid-stride the rest
    const dim3 gr((unsigned)blocks), bl(EVALMANY_THREADS);
    const bool plain = value_only(nd);
    if (g.ndim == 1)
        hipLaunchKernelGGL((plain ? eval_many_var_kernel<1, T, true> : eval_many_var_kernel<1, T, false>), gr, bl, 0, st, g, nbatch, offsets_dev,
                           first, nq, base, xq, ldxq, nd, cov, ldcov, out);
    else
        hipLaunchKernelGGL((plain ? eval_many_var_kernel<2, T, true> : eval_many_var_kernel<2, T, false>), gr, bl, 0, st, g, nbatch, offsets_dev,
                           first, nq, base, xq, ldxq, nd, cov, ldcov, out);
    t_eval_many_stats[0] = blocks;
    t_eval_many_stats[1] = 1;
    t_eval_many_stats[4] = blocks * EVALMANY_THREADS;
    return hipGetLastError();
}
template hipError_t launch_eval_many_var<double>(const Grid &, int, const long long *, long long, long long, long long, const double *, int,
                                                 const int *, const double *, long long, double *, hipStream_t);
template hipError_t launch_eval_many_var<float>(const Grid &, int, const long long *, long long, long long, long long, const float *, int,
                                                const int *, const float *, long long, float *, hipStream_t);

template <typename T>
hipError_t launch_residuals_many(const Grid &g, int nbatch, const long long *offsets_dev, long long base, const T *xdata, int l1xdat,
                                 const T *ydata, const T *wdata, const T *coef, long long ldcoef, T *resid, double *stats, hipStream_t st)
{
    if (nbatch < 1) return hipSuccess;
    const int blocks = nbatch < RESMANY_WAVES ? nbatch : RESMANY_WAVES;      // the waves stride over the rest
    const dim3 gr((unsigned)blocks), bl(64);
    DISPATCH_D(g.ndim, hipLaunchKernelGGL((residuals_many_kernel<D, T>), gr, bl, 0, st, g, nbatch, offsets_dev, base, xdata, l1xdat, ydata,
                                          wdata, coef, ldcoef, resid, stats));
    t_eval_many_stats[0] = blocks;
    t_eval_many_stats[1] = 1;
    return hipGetLastError();
}
template hipError_t launch_residuals_many<double>(const Grid &, int, const long long *, long long, const double *, int, const double *,
                                                  const double *, const double *, long long, double *, double *, hipStream_t);
template hipError_t launch_residuals_many<float>(const Grid &, int, const long long *, long long, const float *, int, const float *,
                                                 const float *, const float *, long long, float *, double *, hipStream_t);

}  // namespace splpak
