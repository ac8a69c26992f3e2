// Evaluation on a tensor-product grid of points: out[i0 + n0 (i1 + n1 (i2 + ...))] = spline (or one partial
// derivative) at (axes_1[i0], axes_2[i1], ...), what a loop of splfe / splde calls over a regular sample
// computes (src/splpak.F90:1089-1240, :1258-1275).
//
// The point route (eval.hip and the sorted paths behind it) takes the Cartesian product as a query list: 8 ndim bytes in per output, a sort
// by region although a grid is ordered, and the same ndim factor tables once per output.  Here:
//
//   grid_table_kernel   one thread per AXIS coordinate: window start + the four factors of that coordinate,
//                       by the device functions of the direct kernel (eval_table / window_table, evalcore.hpp).
//                       sum_d n_d entries of 36 bytes.
//   eval_grid_kernel    a workgroup owns a box of outputs (GTile).  From the tables it takes the range of
//                       window starts its box touches per dimension, stages that coefficient box (range + 3
//                       nodes per dimension) in LDS and contracts ONE DIMENSION AT A TIME: dimension 1 with its
//                       four factors for every output position along dimension 1 and every coefficient row of the
//                       box, then those partial sums with dimension 2, and so on (sum factorisation: neighbouring
//                       outputs share window rows, so a partial sum is formed once per tile instead of once per
//                       output).  The last contraction stores to global memory, consecutive lanes along dimension 1.
//                       A tile whose box and partial sums do not fit the LDS budget (coarse output grids whose
//                       windows do not overlap, unsorted axes, points far outside) takes the GENERAL form: every
//                       output gathers its window from global memory as the direct kernel does, with the factors
//                       from the tables.  Which form a tile takes depends on the tables alone.
//
// Rounding: a partial sum is exactly one of window_sum's intermediates (the row starts c0 b0 and adds k = 1..3 by
// fma; every later dimension starts at 0.0 and adds k = 0..3 by fma, in order), which depends only on the output
// coordinates contracted so far and on the coefficient row.  Sharing it between outputs changes no bit: both forms
// return the values of eval_kernel.
//
// HBM traffic by construction: 8 bytes per output (4 for REAL32) + the coefficient boxes (each coefficient is
// read by the tiles whose boxes hold it, from L2 after the first) + the tables.  Output counts are 64-bit;
// coefficient indices stay int as in Grid.
#include "evalgrid.hpp"
#include <climits>

namespace splpak {

// Outputs of a workgroup per dimension and its LDS budget in doubles.  Powers of two: the stage loops decode
// their items with shifts.  Dimension 1 is the lane direction (64 outputs = one 512-byte store per wave and
// item; 16 in 4-D, where a wider tile's first partial sums -- T0 x R1 R2 R3 -- would not fit).
// Budgets: 160 KB of LDS per CU; 3-D takes 42 KB + 3 KB of tables (three workgroups per CU), 4-D 58 KB + 1 KB
// (two).  With R the box extent (window-start range + 3):
//   3-D  64 x 8 x 8:   R1, R2 <= 6 (up to 3 cells per 8 outputs) and R0 <= 85 fit: 64*36 + max(R0*36, 64*8*6)
//   4-D  16 x 4 x 4 x 4: R1..R3 <= 6 fit: 16*216 + max(R0*216, 16*4*36) with R0 <= 18
template <int D> struct GTile;
template <> struct GTile<1> { static constexpr int T[4] = {256, 1, 1, 1}; static constexpr int LDS = 1; };
template <> struct GTile<2> { static constexpr int T[4] = {64, 16, 1, 1}; static constexpr int LDS = 4096; };
template <> struct GTile<3> { static constexpr int T[4] = {64, 8, 8, 1}; static constexpr int LDS = 5376; };
template <> struct GTile<4> { static constexpr int T[4] = {16, 4, 4, 4}; static constexpr int LDS = 7424; };
// ---- table pass ---------------------------------------------------------------------------------------------------
template <typename T, bool VAL>
__global__ void __launch_bounds__(256)
grid_table_kernel(Grid g, GridShape gs, NDeriv nd, const T *__restrict__ axes, double *__restrict__ fac, int *__restrict__ wst)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    // (no early return: eval_table<true> votes over the wave)
    const bool live = i < gs.off[g.ndim];
    int d = 0;
    for (int e = 1; e < g.ndim; ++e) d = (live && i >= gs.off[e]) ? e : d;
    const double x = live ? (double)axes[i] : g.xmin[0];      // REAL32: widened first, as eval_kernel does
    double b[4];
    const int ws = eval_table<VAL>(g, d, x, nd.v[d], b);
    if (live) {
        wst[i] = ws;
#pragma unroll
        for (int k = 0; k < 4; ++k) fac[4 * i + k] = b[k];
    }
}

// ---- tile kernel --------------------------------------------------------------------------------------------------
template <int D> constexpr int gtile_tab(int d) { int s = 0; for (int e = 0; e < d; ++e) s += GTile<D>::T[e]; return s; }
template <int D> constexpr int gtile_outputs() { int s = 1; for (int e = 0; e < D; ++e) s *= GTile<D>::T[e]; return s; }

// Contraction of dimension DD >= 1.  in[i0 + TX (m + M (j + R h))]: m = the output positions of dimensions 1 .. DD-1
// (M of them), j = the box row of dimension DD, h = the box rows of the dimensions above (H of them).  Item
// (m, i, h), i = output position of dimension DD, becomes dst[i0 + TX item] -- or, in the last dimension, the output.
template <int D, int DD, typename T>          // T: the output type
__device__ inline void grid_stage(const double *__restrict__ in, double *__restrict__ dst, int R, int H, const int *tw,
                                  const double (*tb)[4], int a, const long long (&o0)[D], const GridShape &gs,
                                  T *__restrict__ out)
{
    using GT = GTile<D>;
    constexpr int TX = GT::T[0], TD = GT::T[DD], TAB = gtile_tab<D>(DD);
    constexpr int M = []() { int s = 1; for (int e = 1; e < DD; ++e) s *= GTile<D>::T[e]; return s; }();
    constexpr bool LAST = DD == D - 1;
    const int i0 = threadIdx.x % TX;
    const int items = M * TD * H;
    for (int item = threadIdx.x / TX; item < items; item += GRID_NT / TX) {
        const int m = item % M, i = (item / M) % TD, h = item / (M * TD);
        const int w = tw[TAB + i] - a;
        const double *__restrict__ p = in + i0 + TX * (m + M * (w + R * h));
        const double *bk = tb[TAB + i];
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) sum = fma(p[k * TX * M], bk[k], sum);
        if constexpr (!LAST) {
            dst[i0 + TX * item] = sum;
        } else {
            // h = 0; m = i1 + T1 (i2 + ...) over the dimensions 1 .. D-2
            long long idx = o0[D - 1] + i;
            bool ok = idx < gs.npts[D - 1] && o0[0] + i0 < gs.npts[0];
            int rem = m;
            long long lo = 0, mul = 1;
#pragma unroll
            for (int e = 1; e < D - 1; ++e) {
                const long long c = o0[e] + rem % GT::T[e];
                rem /= GT::T[e];
                ok = ok && c < gs.npts[e];
                lo += c * mul;
                mul *= gs.npts[e];
            }
            idx = lo + idx * mul;                       // over the dimensions 1 .. D-1
            if (ok) out[o0[0] + i0 + gs.npts[0] * idx] = (T)sum;
        }
    }
}

// TC: storage type of the coefficients, TO: of the outputs (the grid entries: the same; the integrals of integrategrid.hip:
// REAL32 coefficients, double piece values)
template <int D, typename TC, typename TO>
__global__ void __launch_bounds__(GRID_NT)
eval_grid_kernel(Grid g, GridShape gs, const double *__restrict__ fac, const int *__restrict__ wst,
                 const TC *__restrict__ coef, TO *__restrict__ out, unsigned long long *__restrict__ stats)
{
    using GT = GTile<D>;
    constexpr int TX = GT::T[0], NTAB = gtile_tab<D>(D);
    __shared__ double lds[GT::LDS];
    __shared__ __attribute__((aligned(16))) double tb[NTAB][4];
    __shared__ int tw[NTAB];
    __shared__ int s_lo[MAXD], s_hi[MAXD];
    const int tid = threadIdx.x;
    long long o0[D];                            // first output of the tile per dimension
    {
        long long t = blockIdx.x;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            o0[d] = (t % gs.ntile[d]) * GT::T[d];
            t /= gs.ntile[d];
        }
    }
    if (tid < MAXD) { s_lo[tid] = INT_MAX; s_hi[tid] = INT_MIN; }
    __syncthreads();
    // the tile's slices of the tables; positions past the end of an axis repeat its last entry (their outputs are
    // never stored), so that the ranges below are those of real points
    for (int e = tid; e < NTAB; e += GRID_NT) {
        int d = 0;
#pragma unroll
        for (int f = 1; f < D; ++f) d = e >= gtile_tab<D>(f) ? f : d;
        int l = e;
#pragma unroll
        for (int f = 1; f < D; ++f) l = d == f ? e - gtile_tab<D>(f) : l;
        long long i = o0[d] + l;
        i = i < gs.npts[d] ? i : gs.npts[d] - 1;
        const long long src = gs.off[d] + i;
        const int w = wst[src];
        tw[e] = w;
#pragma unroll
        for (int k = 0; k < 4; ++k) tb[e][k] = fac[4 * src + k];
        atomicMin(&s_lo[d], w);
        atomicMax(&s_hi[d], w);
    }
    __syncthreads();
    int a[D], R[D];                             // first node and extent of the coefficient box (a + R <= nodes: ws <= nodes - 4)
#pragma unroll
    for (int d = 0; d < D; ++d) {
        a[d] = s_lo[d];
        R[d] = s_hi[d] - s_lo[d] + 4;
    }
    // LDS plan: box [0, B) | first partial sums S0 at PA; the second ones (S1) overlay the box, which is dead by then,
    // the third ones (S2, 4-D) overlay S0.
    bool fits = D >= 2;
    int PA = 0;
    if constexpr (D >= 2) {
        long long H0 = 1;
#pragma unroll
        for (int d = 1; d < D; ++d) H0 *= R[d];
        const long long B = H0 * R[0], S0 = TX * H0;
        long long S1 = 0, S2 = 0;
        if constexpr (D >= 3) S1 = (long long)TX * GT::T[1] * (H0 / R[1]);
        if constexpr (D >= 4) S2 = (long long)TX * GT::T[1] * GT::T[2] * R[3];
        const long long pa = B > S1 ? B : S1;
        fits = pa + (S0 > S2 ? S0 : S2) <= GT::LDS;
        PA = (int)pa;
    }
    if (tid == 0 && stats) atomicAdd(&stats[fits ? 0 : 1], 1ULL);
    if (fits) {
        if constexpr (D >= 2) {
            int H0 = 1;
#pragma unroll
            for (int d = 1; d < D; ++d) H0 *= R[d];
            const int B = H0 * R[0];
            for (int e = tid; e < B; e += GRID_NT) {
                int rem = e, idx = 0;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    idx += (a[d] + rem % R[d]) * g.colstride[d];
                    rem /= R[d];
                }
                lds[e] = (double)coef[idx];
            }
            __syncthreads();
            double *bufA = lds + PA, *bufB = lds;
            {   // dimension 1: the window row, exactly as window_sum's row()
                const int i0 = tid % TX;
                const double *c0 = lds + (tw[i0] - a[0]);
                const double b0 = tb[i0][0], b1 = tb[i0][1], b2 = tb[i0][2], b3 = tb[i0][3];
                for (int h = tid / TX; h < H0; h += GRID_NT / TX) {
                    const double *c = c0 + R[0] * h;
                    double t = c[0] * b0;
                    t = fma(c[1], b1, t);
                    t = fma(c[2], b2, t);
                    t = fma(c[3], b3, t);
                    bufA[i0 + TX * h] = t;
                }
            }
            __syncthreads();
            if constexpr (D == 2) {
                grid_stage<D, 1, TO>(bufA, nullptr, R[1], 1, tw, tb, a[1], o0, gs, out);
            } else if constexpr (D == 3) {
                grid_stage<D, 1, TO>(bufA, bufB, R[1], R[2], tw, tb, a[1], o0, gs, out);
                __syncthreads();
                grid_stage<D, 2, TO>(bufB, nullptr, R[2], 1, tw, tb, a[2], o0, gs, out);
            } else {
                grid_stage<D, 1, TO>(bufA, bufB, R[1], R[2] * R[3], tw, tb, a[1], o0, gs, out);
                __syncthreads();
                grid_stage<D, 2, TO>(bufB, bufA, R[2], R[3], tw, tb, a[2], o0, gs, out);
                __syncthreads();
                grid_stage<D, 3, TO>(bufA, nullptr, R[3], 1, tw, tb, a[3], o0, gs, out);
            }
        }
        return;
    }
    // general form: the plain window_sum gather of eval_kernel, factors from the tables
    const int s1 = D > 1 ? g.colstride[1] : 0, s2 = D > 2 ? g.colstride[2] : 0, s3 = D > 3 ? g.colstride[3] : 0;
    for (int o = tid; o < gtile_outputs<D>(); o += GRID_NT) {
        double b[D][4];
        int base = 0, rem = o;
        long long idx = 0, mul = 1;
        bool ok = true;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int l = rem % GT::T[d];
            rem /= GT::T[d];
            const long long c = o0[d] + l;
            ok = ok && c < gs.npts[d];
            idx += c * mul;
            mul *= gs.npts[d];
            const int e = gtile_tab<D>(d) + l;
            base += tw[e] * g.colstride[d];
#pragma unroll
            for (int k = 0; k < 4; ++k) b[d][k] = tb[e][k];
        }
        if (!ok) continue;
        const double sum = window_sum<D>(b, [&](int k1, int k2, int k3, double (&c)[4]) {
            const long long ci = base + k1 * s1 + k2 * s2 + k3 * s3;
            load_window_row(coef + ci, c);
        });
        out[idx] = (TO)sum;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// per-thread scratch (evalscratch.hpp): tile counters | factors [ntab][4] | window starts [ntab] of the last call
// (evalgridderivs.hip: factors [ntab][order + 1][4])
static thread_local DevScratch<1> g_gscratch;

DevScratch<1> &eval_grid_scratch() { return g_gscratch; }

long long eval_grid_scratch_bytes(long long ntab) { return 40 * ntab + 16; }      // 32 (factors) + 4 (start), rounded; counters

void eval_grid_scratch_shutdown() { g_gscratch.release(); }

hipError_t eval_grid_stats(long long out2[2])
{
    DevScratch<1> &s = g_gscratch;
    out2[0] = out2[1] = 0;
    if (!s.buf[0] || !s.used) return hipSuccess;
    if (hipError_t e = hipEventSynchronize(s.last); e != hipSuccess) return e;
    unsigned long long v[2];
    if (hipError_t e = hipMemcpy(v, s.buf[0], sizeof v, hipMemcpyDeviceToHost); e != hipSuccess) return e;
    out2[0] = (long long)v[0];
    out2[1] = (long long)v[1];
    return hipSuccess;
}

int eval_grid_tile(int ndim, int d) { return ndim == 1 ? GTile<1>::T[d] : ndim == 2 ? GTile<2>::T[d] : ndim == 3 ? GTile<3>::T[d] : GTile<4>::T[d]; }

bool eval_grid_slab(int ndim, const long long *npts, long long row, long long cap, long long &qmax)
{
    const int last = ndim - 1;
    long long row_tiles = 1;      // tiles of one tile layer of the last dimension
    for (int d = 0; d < last; ++d) {
        const long long t = eval_grid_tile(ndim, d);
        if (__builtin_mul_overflow(row_tiles, (npts[d] + t - 1) / t, &row_tiles)) return false;
    }
    if (row_tiles > 0x7fffffffLL) return false;
    const long long qtiles = (0x7fffffffLL / row_tiles) * eval_grid_tile(ndim, last);
    qmax = cap / row;
    qmax = qmax < qtiles ? qmax : qtiles;
    return true;
}

// the tile kernel on prepared tables: gs.npts and gs.off are the caller's, the tile counts are set here
template <typename TC, typename TO>
hipError_t launch_eval_grid_tables(const Grid &g, GridShape &gs, const double *fac, const int *wst, const TC *coef, TO *out,
                                   unsigned long long *stats, hipStream_t st)
{
    long long ntiles = 1;
    for (int d = 0; d < MAXD; ++d) {
        const int t = eval_grid_tile(g.ndim, d);
        gs.ntile[d] = (gs.npts[d] + t - 1) / t;
        if (__builtin_mul_overflow(ntiles, gs.ntile[d], &ntiles)) return hipErrorInvalidValue;
    }
    if (ntiles > 0x7fffffffLL) return hipErrorInvalidValue;
    dim3 gr((unsigned)ntiles), bl(GRID_NT);
    switch (g.ndim) {
    case 1: hipLaunchKernelGGL((eval_grid_kernel<1, TC, TO>), gr, bl, 0, st, g, gs, fac, wst, coef, out, stats); break;
    case 2: hipLaunchKernelGGL((eval_grid_kernel<2, TC, TO>), gr, bl, 0, st, g, gs, fac, wst, coef, out, stats); break;
    case 3: hipLaunchKernelGGL((eval_grid_kernel<3, TC, TO>), gr, bl, 0, st, g, gs, fac, wst, coef, out, stats); break;
    default: hipLaunchKernelGGL((eval_grid_kernel<4, TC, TO>), gr, bl, 0, st, g, gs, fac, wst, coef, out, stats); break;
    }
    return hipGetLastError();
}
template hipError_t launch_eval_grid_tables<double, double>(const Grid &, GridShape &, const double *, const int *, const double *, double *, unsigned long long *, hipStream_t);
template hipError_t launch_eval_grid_tables<float, float>(const Grid &, GridShape &, const double *, const int *, const float *, float *, unsigned long long *, hipStream_t);
template hipError_t launch_eval_grid_tables<float, double>(const Grid &, GridShape &, const double *, const int *, const float *, double *, unsigned long long *, hipStream_t);

template <typename T>
hipError_t launch_eval_grid(const Grid &g, const int64_t *npts, const T *axes, const int *nderiv, const T *coef, T *out, hipStream_t st)
{
    GridShape gs;
    if (!grid_shape(g.ndim, npts, gs)) return hipSuccess;
    const long long ntab = gs.off[MAXD];
    const NDeriv nd = clamp_nderiv(nderiv, g.ndim);
    DevScratch<1> &s = g_gscratch;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const size_t need[1] = {(size_t)eval_grid_scratch_bytes(ntab)};
    if (hipError_t e = s.ensure(dev, need, /*may_release_plan=*/true); e != hipSuccess) return e;
    if (hipError_t e = s.wait_on(st); e != hipSuccess) return e;
    const ScratchUse<1> use{s, st};                         // (also after a refused tile count: the table kernel is queued)
    unsigned long long *stats = s.as<unsigned long long>(0);
    double *fac = reinterpret_cast<double *>(stats + 2);
    int *wst = reinterpret_cast<int *>(fac + 4 * ntab);
    if (hipError_t e = hipMemsetAsync(stats, 0, 16, st); e != hipSuccess) return e;
    {
        dim3 gr((unsigned)((ntab + 255) / 256)), bl(256);
        hipLaunchKernelGGL((value_only(nd) ? grid_table_kernel<T, true> : grid_table_kernel<T, false>), gr, bl, 0, st, g, gs, nd, axes, fac, wst);
    }
    return launch_eval_grid_tables<T, T>(g, gs, fac, wst, coef, out, stats, st);
}
template hipError_t launch_eval_grid<double>(const Grid &, const int64_t *, const double *, const int *, const double *, double *, hipStream_t);
template hipError_t launch_eval_grid<float>(const Grid &, const int64_t *, const float *, const int *, const float *, float *, hipStream_t);

}  // namespace splpak
