// Batched spline / partial-derivative evaluation: one thread per query.
//
// Replaces a loop of scalar splde/splfe calls (src/splpak.F90:1089-1240,
// :1258-1275).  Per query the reference calls bascmp 4^ndim times and recomputes
// every 1-D factor 4^(ndim-1) times; here each thread builds the separable
// 4 x ndim table once (basis.hpp) and walks the 4^ndim window with the same
// summation order as the reference's odometer (dimension 1 fastest, :1228-1232),
// so results differ from the reference only by FMA contraction.
//
// HBM roofline: 8*(ndim+1) algorithmic bytes per query (ndim coordinates in, one
// value out).  Paths with identical arithmetic: the direct kernels of this file gather
// the coefficients from global memory (L2-bound for scattered queries); the sorted
// paths sort large batches by grid region and gather from LDS -- the persistent region
// path (evalregion.hip), the run path (evalruns.hip) and the region sort (evalsort.hip),
// tried in that order by the dispatchers at the end of this file.
#include "evalpaths.hpp"
#include "manyhost.hpp"

namespace splpak {

// ---- direct path: one thread per query, coefficient gathers from global memory (L2) -------------
template <int D, typename T, bool VAL>
__global__ void __launch_bounds__(256)
eval_kernel(Grid g, long long nq, const T *__restrict__ xq, int ldxq, NDeriv nd,
            const T *__restrict__ coef, T *__restrict__ out)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += stride) {
        double b[D][4];
        int base = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double x = (double)xq[i * ldxq + d];
            const int ws = eval_table<VAL>(g, d, x, nd.v[d], b[d]);
            base += ws * g.colstride[d];
        }
        const int s1 = D > 1 ? g.colstride[1] : 0, s2 = D > 2 ? g.colstride[2] : 0, s3 = D > 3 ? g.colstride[3] : 0;
        const double sum = window_sum<D>(b, [&](int k1, int k2, int k3, double (&c)[4]) {
            const long long idx = base + k1 * s1 + k2 * s2 + k3 * s3;
            load_window_row(coef + idx, c);
        });
        out[i] = (T)sum;
    }
}

// Several coefficient sets at the same queries (splpak_eval_fields_*): field k's coefficients at coef + k*ldcoef, its results at
// out + k*ldout.  A thread reads its coordinates and builds its factor table once, then sums the window once per field with
// eval_kernel's row loads and window_sum's arithmetic -- nothing is shared between the fields, so every field has the bits of
// its own eval_kernel call.  Up to 3-D two fields at a time: their sums are independent, so the gathers of one are in flight
// while the other is multiplied.  4-D one at a time: beside the 32 registers of its table a pair of 256-coefficient windows
// takes the whole register file (256 VGPRs, one wave per SIMD, against the 70 of eval_kernel).
template <int D, typename T, bool VAL>
__global__ void __launch_bounds__(256)
eval_fields_kernel(Grid g, long long nq, const T *__restrict__ xq, int ldxq, NDeriv nd, int nfields, const T *__restrict__ coef,
                   long long ldcoef, T *__restrict__ out, long long ldout)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += stride) {
        double b[D][4];
        int base = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double x = (double)xq[i * ldxq + d];
            const int ws = eval_table<VAL>(g, d, x, nd.v[d], b[d]);
            base += ws * g.colstride[d];
        }
        const int s1 = D > 1 ? g.colstride[1] : 0, s2 = D > 2 ? g.colstride[2] : 0, s3 = D > 3 ? g.colstride[3] : 0;
        auto field = [&](const T *__restrict__ cf) {
            return window_sum<D>(b, [&](int k1, int k2, int k3, double (&c)[4]) {
                const long long idx = base + k1 * s1 + k2 * s2 + k3 * s3;
                load_window_row(cf + idx, c);
            });
        };
        int k = 0;
        for (; D < 4 && k + 1 < nfields; k += 2) {
            const T *c0 = coef + (long long)k * ldcoef;
            const double sum0 = field(c0), sum1 = field(c0 + ldcoef);
            out[(long long)k * ldout + i] = (T)sum0;
            out[(long long)(k + 1) * ldout + i] = (T)sum1;
        }
        for (; k < nfields; ++k) out[(long long)k * ldout + i] = (T)field(coef + (long long)k * ldcoef);      // (up to 3-D: the odd one)
    }
}

template <int D, int ORDER, typename T>
__global__ void __launch_bounds__(256)
eval_derivs_kernel(Grid g, long long nq, const T *__restrict__ xq, int ldxq, const T *__restrict__ coef,
                   T *__restrict__ out, int ldout)
{
    constexpr int NOUT = 1 + D + (ORDER == 2 ? D * (D + 1) / 2 : 0);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += stride) {
        double b[ORDER + 1][D][4];
        int base = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double x = (double)xq[i * ldxq + d];
            int ws = 0;
#pragma unroll
            for (int a = 0; a <= ORDER; ++a) ws = window_table(g, d, x, a, b[a][d]);
            base += ws * g.colstride[d];
        }
        double acc[NOUT];
        derivs_accumulate<D, ORDER>(b, [&](const int (&k)[D], double (&c)[4]) {
            int off = 0;
#pragma unroll
            for (int d = 1; d < D; ++d) off += k[d] * g.colstride[d];
            if constexpr (sizeof(T) == 8) {
                typedef double d2v __attribute__((ext_vector_type(2), aligned(8)));
                const d2v lo2 = *reinterpret_cast<const d2v *>(coef + base + off);
                const d2v hi2 = *reinterpret_cast<const d2v *>(coef + base + off + 2);
                c[0] = lo2[0]; c[1] = lo2[1]; c[2] = hi2[0]; c[3] = hi2[1];
            } else {
#pragma unroll
                for (int k0 = 0; k0 < 4; ++k0) c[k0] = (double)coef[base + off + k0];
            }
        }, acc);
#pragma unroll
        for (int j = 0; j < NOUT; ++j) out[i * ldout + j] = (T)acc[j];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
static thread_local int g_eval_mode = 0;             // 0 auto, 1 direct, 2 binned
static thread_local long long g_eval_chunk = 0;      // queries per chunk of the run path and the region sort, 0 = default

void set_eval_mode(int mode, long long chunk)
{
    g_eval_mode = mode;
    g_eval_chunk = chunk;
}

// the calling thread's last fields call: route (0 none yet, 1 direct fields kernel, 2 shared sort, 3 one launch_eval per field),
// place passes launched, evaluation-kernel launches
static thread_local long long g_fields_stats[3] = {0, 0, 0};

void eval_fields_stats(long long out3[3])
{
    for (int j = 0; j < 3; ++j) out3[j] = g_fields_stats[j];
}

void eval_scratch_shutdown()
{
    eval_persistent_shutdown();
    eval_runs_shutdown();
    eval_sort_shutdown();
    many_scratch_shutdown();
}

// The sorted paths, fastest first: the persistent region path, the run path, the region sort.  hipErrorNotSupported of a
// path = not for this grid / batch (or, persistent path, no room for its scratch): the next one is tried.
// order == 0: one nderiv pattern (nd) -> out[nq]; order 1 / 2: value + gradient (+ Hessian) -> out[nq][ldout] (region sort only)
template <typename T>
static hipError_t eval_binned(const Grid &g, const Regions &rg, long long nq, const T *xq, int ldxq, const NDeriv &nd, const T *coef,
                              T *out, hipStream_t st, int order = 0, int ldout = 1)
{
    if (order == 0 && g.ndim >= 3) {
        hipError_t e = eval_persistent<T>(g, nq, xq, ldxq, nd, coef, out, st);
        if (e != hipErrorNotSupported) return e;
        e = eval_runs<T>(g, rg, nq, xq, ldxq, nd, coef, out, g_eval_chunk, st);
        if (e != hipErrorNotSupported) return e;
    }
    return eval_sort<T>(g, rg, nq, xq, ldxq, nd, coef, out, g_eval_chunk, st, order, ldout);
}

// large batches on grids whose coefficients are far beyond the L1 (auto), or forced.  auto: 2-D windows are 4 rows (4-5 L2
// lines) and the direct kernel wins; from 3-D on (16+ rows) the sort pays for itself once the batch is large
static bool want_binned(const Grid &g, long long nq)
{
    return g_eval_mode == 2 || (g_eval_mode == 0 && g.ndim >= 3 && nq >= (1LL << 20) && g.ncol > 32768);
}

template <typename T>
hipError_t launch_eval_derivs(const Grid &g, long long nq, const T *xq, int ldxq, int order, const T *coef, T *out, int ldout,
                              hipStream_t st)
{
    if (nq <= 0) return hipSuccess;
    if constexpr (sizeof(T) == 8) {
        // same rule as the single-pattern evaluation: large batches on 3-D / 4-D grids go through the region sort
        Regions rg;
        if (make_regions(g, rg) && want_binned(g, nq)) {
            const hipError_t e = eval_binned<T>(g, rg, nq, xq, ldxq, NDeriv{}, coef, out, st, order, ldout);
            if (e != hipErrorOutOfMemory) return e;
            (void)hipGetLastError();
        }
    }
    long long blocks = (nq + 255) / 256;
    if (blocks > 256LL * 32) blocks = 256LL * 32;
    dim3 gr((unsigned)blocks), bl(256);
#define SPLPAK_DERIVS(DD) \
    hipLaunchKernelGGL((order == 1 ? eval_derivs_kernel<DD, 1, T> : eval_derivs_kernel<DD, 2, T>), gr, bl, 0, st, g, nq, xq, ldxq, coef, out, ldout);
    switch (g.ndim) {
    case 1: SPLPAK_DERIVS(1) break;
    case 2: SPLPAK_DERIVS(2) break;
    case 3: SPLPAK_DERIVS(3) break;
    default: SPLPAK_DERIVS(4) break;
    }
#undef SPLPAK_DERIVS
    return hipGetLastError();
}
template hipError_t launch_eval_derivs<double>(const Grid &, long long, const double *, int, int, const double *, double *, int, hipStream_t);
template hipError_t launch_eval_derivs<float>(const Grid &, long long, const float *, int, int, const float *, float *, int, hipStream_t);

template <typename T>
hipError_t launch_eval(const Grid &g, long long nq, const T *xq, int ldxq, const int *nderiv, const T *coef, T *out, hipStream_t st)
{
    if (nq <= 0) return hipSuccess;
    const NDeriv nd = clamp_nderiv(nderiv, g.ndim);
    {
        // binned path (both storage kinds: the REAL32 entry points widen their inputs in the sort passes and the tile fill,
        // same arithmetic as their direct kernel)
        Regions rg;
        if (make_regions(g, rg) && want_binned(g, nq)) {
            const hipError_t e = eval_binned<T>(g, rg, nq, xq, ldxq, nd, coef, out, st);
            // no room for the sort scratch: the binned path is an optimisation, fall through to the direct one
            if (e != hipErrorOutOfMemory) return e;
            (void)hipGetLastError();
        }
    }
    const int threads = 256;
    long long blocks = (nq + threads - 1) / threads;
    if (blocks > 256LL * 32) blocks = 256LL * 32;   // grid-stride the rest
    dim3 gr((unsigned)blocks), bl(threads);
    const bool plain = value_only(nd);
#define SPLPAK_EVAL(DD) \
    hipLaunchKernelGGL((plain ? eval_kernel<DD, T, true> : eval_kernel<DD, T, false>), gr, bl, 0, st, g, nq, xq, ldxq, nd, coef, out);
    switch (g.ndim) {
    case 1: SPLPAK_EVAL(1) break;
    case 2: SPLPAK_EVAL(2) break;
    case 3: SPLPAK_EVAL(3) break;
    default: SPLPAK_EVAL(4) break;
    }
#undef SPLPAK_EVAL
    return hipGetLastError();
}
template hipError_t launch_eval<double>(const Grid &, long long, const double *, int, const int *, const double *, double *, hipStream_t);
template hipError_t launch_eval<float>(const Grid &, long long, const float *, int, const int *, const float *, float *, hipStream_t);

// Several fields at the same queries.  One field: launch_eval itself.  A batch launch_eval would sort: the persistent region
// path sorts it once for all fields; where that path does not apply (2-D, too many regions, no room for its scratch -- it says so
// before it launches anything) every field takes launch_eval on its own, so that the run path and the region sort serve those
// grids as they do for one field.  Everything else: the direct fields kernel.
template <typename T>
hipError_t launch_eval_fields(const Grid &g, long long nq, const T *xq, int ldxq, const int *nderiv, int nfields, const T *coef,
                              long long ldcoef, T *out, long long ldout, hipStream_t st)
{
    long long (&stats)[3] = g_fields_stats;
    stats[0] = stats[1] = stats[2] = 0;
    if (nq <= 0 || nfields < 1) return hipSuccess;
    // (route 3 counts the launch_eval calls; what these sort and launch is theirs)
    auto per_field = [&]() {
        stats[0] = 3;
        for (int k = 0; k < nfields; ++k) {
            const hipError_t e = launch_eval<T>(g, nq, xq, ldxq, nderiv, coef + (long long)k * ldcoef, out + (long long)k * ldout, st);
            if (e != hipSuccess) return e;
            ++stats[2];
        }
        return hipSuccess;
    };
    if (nfields == 1) return per_field();
    const NDeriv nd = clamp_nderiv(nderiv, g.ndim);
    if (want_binned(g, nq)) {
        Regions rg;
        if (make_regions(g, rg)) {
            const hipError_t e = eval_persistent<T>(g, nq, xq, ldxq, nd, coef, out, st, nfields, ldcoef, ldout);
            if (e != hipErrorNotSupported) {
                stats[0] = 2;
                stats[1] = 1;
                stats[2] = nfields;
                return e;
            }
        }
        return per_field();
    }
    const int threads = 256;
    long long blocks = (nq + threads - 1) / threads;
    if (blocks > 256LL * 32) blocks = 256LL * 32;   // grid-stride the rest
    dim3 gr((unsigned)blocks), bl(threads);
    const bool plain = value_only(nd);
#define SPLPAK_EVAL_FIELDS(DD) \
    hipLaunchKernelGGL((plain ? eval_fields_kernel<DD, T, true> : eval_fields_kernel<DD, T, false>), gr, bl, 0, st, g, nq, xq, ldxq, nd, nfields, \
                       coef, ldcoef, out, ldout);
    switch (g.ndim) {
    case 1: SPLPAK_EVAL_FIELDS(1) break;
    case 2: SPLPAK_EVAL_FIELDS(2) break;
    case 3: SPLPAK_EVAL_FIELDS(3) break;
    default: SPLPAK_EVAL_FIELDS(4) break;
    }
#undef SPLPAK_EVAL_FIELDS
    stats[0] = 1;
    stats[2] = 1;
    return hipGetLastError();
}
template hipError_t launch_eval_fields<double>(const Grid &, long long, const double *, int, const int *, int, const double *, long long, double *,
                                               long long, hipStream_t);
template hipError_t launch_eval_fields<float>(const Grid &, long long, const float *, int, const int *, int, const float *, long long, float *,
                                              long long, hipStream_t);

}  // namespace splpak
