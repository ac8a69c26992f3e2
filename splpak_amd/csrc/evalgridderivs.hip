// Value, gradient and (order 2) Hessian on a tensor-product grid of points, in PLANES: out[e ldout + idx] is entry e of
// splpak_eval_derivs_* (f, df/dx_1 .. df/dx_D, then the upper triangle of the Hessian row by row) at grid point
// idx = i0 + n0 (i1 + n1 (i2 + ...)), the ordering of evalgrid.hip.  What a loop of splpak_eval_grid_* calls over the
// 1 + D (+ D (D + 1) / 2) nderiv patterns computes, in one pass: one table pass, one coefficient box per tile, and the
// partial sums the patterns share formed once.
//
//   grid_derivs_table_kernel   one thread per AXIS coordinate: window start + the factor quadruples of derivative order
//                              0 .. ORDER, all by window_table (the general form, as every nderiv != 0 call gets them).
//   eval_grid_derivs_kernel    the plan of eval_grid_kernel -- range of window starts per dimension, coefficient box in
//                              LDS, one dimension contracted at a time, lanes along dimension 1 -- with one buffer per
//                              PATTERN SO FAR: after the dimensions 1 .. m a buffer exists for every (a_1 .. a_m) with
//                              a_1 + .. + a_m <= ORDER, and the buffer (a_1 .. a_m, a) is built from (a_1 .. a_m) with the
//                              order-a factors of dimension m + 1.  Buffers after dimension m (gd_nsets):
//                                  ORDER 1:  2  3  4  5        ORDER 2:  3  6  10  15
//                              against (patterns) x (dimensions) stage passes and as many box loads for the loop of calls.
//                              A tile whose box and buffers do not fit the budget takes the GENERAL form: every output
//                              gathers its window rows from global memory once and all planes accumulate from them.
//
// Rounding: every partial sum is formed as window_sum forms it (the row starts c0 b0 and adds k = 1..3 by fma; every later
// dimension starts at 0.0 and adds k = 0..3 by fma, in order) with the factor table of its plane's pattern.  Plane e >= 1
// therefore has the bits of splpak_eval_grid_* called with entry e's nderiv, on both forms; plane 0 has that summation on
// the order-0 general-form tables (splpak_eval_grid_* with nderiv == NULL takes the closed-form value tables: equal to
// rounding, not to the bit).
#include "evalgrid.hpp"
#include <climits>

namespace splpak {

// ---- derivative patterns ------------------------------------------------------------------------------------------
// The patterns of total order <= `order` over m dimensions, numbered as the entries of splpak_eval_derivs_* with ndim = m:
// 0 the value, 1 + d the first derivative in dimension d, then (order 2) the pairs d <= f row by row.
__host__ __device__ constexpr int gd_nsets(int m, int order) { return 1 + m + (order == 2 ? m * (m + 1) / 2 : 0); }
__host__ __device__ constexpr int gd_total(int m, int j) { return j == 0 ? 0 : (j <= m ? 1 : 2); }
__host__ __device__ constexpr int gd_pair(int m, int d, int f)
{
    int e = 1 + m;
    for (int r = 0; r < d; ++r) e += m - r;
    return e + (f - d);
}
// pattern j over m dimensions, continued with order a in dimension m + 1: its number over m + 1 dimensions
__host__ __device__ constexpr int gd_child(int m, int j, int a)
{
    if (a == 2) return gd_pair(m + 1, m, m);                 // j = 0
    if (a == 1) return j == 0 ? 1 + m : gd_pair(m + 1, j - 1, m);
    if (j <= m) return j;
    for (int d = 0; d < m; ++d)
        for (int f = d; f < m; ++f)
            if (gd_pair(m, d, f) == j) return gd_pair(m + 1, d, f);
    return -1;
}

// ---- tiles --------------------------------------------------------------------------------------------------------
// Outputs of a workgroup per dimension and its LDS budget in doubles, per (dimensions, order).  Several buffers per
// stage do not fit the tiles of evalgrid.hip; these keep box, buffers and tables below 64 KB (two workgroups per CU
// and more).  With R the box extent (window-start range + 3) and n_s = gd_nsets(s + 1, ORDER):
//   box  prod R | S0 = n_0 T0 R1 R2 R3 | S1 = n_1 T0 T1 R2 R3 | S2 = n_2 T0 T1 T2 R3;  max(box, S1) + max(S0, S2) <= LDS
//   3-D order 1   64 x 4 x 4      R1 = R2 = 5:       3840 + 3200
//   3-D order 2   32 x 4 x 4      R1 = 6, R2 = 5:    3840 + 2880
//   4-D order 1   8 x 4 x 4 x 4   R1 = R2 = R3 = 6:  3456 + 3456
//   4-D order 2   8 x 2 x 4 x 4   R1 = 5, R2 = R3 = 6: 3456 + 4320
// which regular axes of about four (3-D) / two (4-D) points per cell stay within.
template <int D, int O> struct GDTile;
template <int O> struct GDTile<1, O> { static constexpr int T[4] = {256, 1, 1, 1}; static constexpr int LDS = 1; };
template <int O> struct GDTile<2, O> { static constexpr int T[4] = {64, 16, 1, 1}; static constexpr int LDS = 4096; };
template <> struct GDTile<3, 1> { static constexpr int T[4] = {64, 4, 4, 1}; static constexpr int LDS = 7040; };
template <> struct GDTile<3, 2> { static constexpr int T[4] = {32, 4, 4, 1}; static constexpr int LDS = 6720; };
template <> struct GDTile<4, 1> { static constexpr int T[4] = {8, 4, 4, 4}; static constexpr int LDS = 6912; };
template <> struct GDTile<4, 2> { static constexpr int T[4] = {8, 2, 4, 4}; static constexpr int LDS = 7776; };

template <int D, int O> constexpr int gdtile_tab(int d) { int s = 0; for (int e = 0; e < d; ++e) s += GDTile<D, O>::T[e]; return s; }
template <int D, int O> constexpr int gdtile_outputs() { int s = 1; for (int e = 0; e < D; ++e) s *= GDTile<D, O>::T[e]; return s; }

bool eval_grid_derivs_tile(int ndim, int order, int out4[4])
{
    if (ndim < 1 || ndim > MAXD || order < 1 || order > 2) return false;
    const int *t = ndim == 1 ? GDTile<1, 1>::T : ndim == 2 ? GDTile<2, 1>::T
                 : ndim == 3 ? (order == 1 ? GDTile<3, 1>::T : GDTile<3, 2>::T)
                             : (order == 1 ? GDTile<4, 1>::T : GDTile<4, 2>::T);
    for (int d = 0; d < MAXD; ++d) out4[d] = d < ndim ? t[d] : 1;
    return true;
}

// ---- table pass ---------------------------------------------------------------------------------------------------
// fac[(O + 1) i + a][0..3]: the factors of derivative order a at axis coordinate i
template <typename T, int O>
__global__ void __launch_bounds__(256)
grid_derivs_table_kernel(Grid g, GridShape gs, const T *__restrict__ axes, double *__restrict__ fac, int *__restrict__ wst)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    // (no early return, as grid_table_kernel)
    const bool live = i < gs.off[g.ndim];
    int d = 0;
    for (int e = 1; e < g.ndim; ++e) d = (live && i >= gs.off[e]) ? e : d;
    const double x = live ? (double)axes[i] : g.xmin[0];      // REAL32: widened first, as eval_kernel does
#pragma unroll
    for (int a = 0; a <= O; ++a) {
        double b[4];
        const int ws = window_table(g, d, x, a, b);
        if (live) {
            if (a == 0) wst[i] = ws;
#pragma unroll
            for (int k = 0; k < 4; ++k) fac[4 * ((O + 1) * i + a) + k] = b[k];
        }
    }
}

// ---- tile kernel --------------------------------------------------------------------------------------------------
// Contraction of dimension DD >= 1, for every pattern over the dimensions 0 .. DD-1 (buffers `insz` apart in `in`) and
// every order a that keeps the total within O.  Layout of one buffer as in grid_stage (evalgrid.hip):
// in[i0 + TX (m + M (j + R h))] -> dst[i0 + TX item], item = (m, i, h); the last dimension stores plane `child` of the output.
template <int D, int O, int DD, typename T>
__device__ inline void grid_derivs_stage(const double *__restrict__ in, double *__restrict__ dst, int R, int H, const int *tw,
                                         const double (*tb)[4], int a0, const long long (&o0)[D], const GridShape &gs,
                                         T *__restrict__ out, long long ldout)
{
    using GT = GDTile<D, O>;
    constexpr int TX = GT::T[0], TD = GT::T[DD], TAB = gdtile_tab<D, O>(DD), NTAB = gdtile_tab<D, O>(D);
    constexpr int M = []() { int s = 1; for (int e = 1; e < DD; ++e) s *= GDTile<D, O>::T[e]; return s; }();
    constexpr bool LAST = DD == D - 1;
    constexpr int NP = gd_nsets(DD, O);
    const int i0 = threadIdx.x % TX;
    const int items = M * TD * H;
    const int insz = TX * M * R * H, outsz = TX * items;
    for (int item = threadIdx.x / TX; item < items; item += GRID_NT / TX) {
        const int m = item % M, i = (item / M) % TD, h = item / (M * TD);
        const int w = tw[TAB + i] - a0;
        const double *__restrict__ p = in + i0 + TX * (m + M * (w + R * h));
        long long pos = 0;
        bool ok = true;
        if constexpr (LAST) {
            // h = 0; m = i1 + T1 (i2 + ...) over the dimensions 1 .. D-2
            long long idx = o0[D - 1] + i;
            ok = idx < gs.npts[D - 1] && o0[0] + i0 < gs.npts[0];
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
            pos = o0[0] + i0 + gs.npts[0] * idx;
        }
#pragma unroll
        for (int pj = 0; pj < NP; ++pj) {
            double c[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = p[pj * insz + k * TX * M];
#pragma unroll
            for (int a = 0; a <= O; ++a) {
                if (a + gd_total(DD, pj) > O) continue;
                const double *bk = tb[a * NTAB + TAB + i];
                double sum = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) sum = fma(c[k], bk[k], sum);
                const int child = gd_child(DD, pj, a);
                if constexpr (!LAST) {
                    dst[child * outsz + i0 + TX * item] = sum;
                } else {
                    if (ok) out[child * ldout + pos] = (T)sum;
                }
            }
        }
    }
}

// general form, one output: the window rows gathered once, every level keeps one accumulator per pattern so far.
// acc = the patterns over the dimensions 0 .. L of the rows with window indices k[L + 1 ..]; fac(a, d, k) = factor table.
template <int D, int O, int L, typename F, typename L4>
__device__ inline void grid_derivs_gather(F &&fac, L4 &&load4, int (&k)[4], double (&acc)[gd_nsets(L + 1, O)])
{
    if constexpr (L == 0) {
        double c[4];
        load4(k[1], k[2], k[3], c);
#pragma unroll
        for (int a = 0; a <= O; ++a) {
            double t = c[0] * fac(a, 0, 0);
            t = fma(c[1], fac(a, 0, 1), t);
            t = fma(c[2], fac(a, 0, 2), t);
            t = fma(c[3], fac(a, 0, 3), t);
            acc[a] = t;
        }
    } else {
        constexpr int NP = gd_nsets(L, O);
#pragma unroll
        for (int j = 0; j < gd_nsets(L + 1, O); ++j) acc[j] = 0.0;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            k[L] = kk;
            double low[NP];
            grid_derivs_gather<D, O, L - 1>(fac, load4, k, low);
#pragma unroll
            for (int pj = 0; pj < NP; ++pj)
#pragma unroll
                for (int a = 0; a <= O; ++a) {
                    if (a + gd_total(L, pj) > O) continue;
                    const int child = gd_child(L, pj, a);
                    acc[child] = fma(low[pj], fac(a, L, kk), acc[child]);
                }
        }
    }
}

template <int D, int O, typename T>
__global__ void __launch_bounds__(GRID_NT)
eval_grid_derivs_kernel(Grid g, GridShape gs, const double *__restrict__ fac, const int *__restrict__ wst,
                        const T *__restrict__ coef, T *__restrict__ out, long long ldout, unsigned long long *__restrict__ stats)
{
    using GT = GDTile<D, O>;
    constexpr int TX = GT::T[0], NTAB = gdtile_tab<D, O>(D);
    __shared__ double lds[GT::LDS];
    __shared__ __attribute__((aligned(16))) double tb[(O + 1) * NTAB][4];      // [a][table entry][k]
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
    // the tile's slices of the tables; positions past the end of an axis repeat its last entry (never stored)
    for (int e = tid; e < NTAB; e += GRID_NT) {
        int d = 0;
#pragma unroll
        for (int f = 1; f < D; ++f) d = e >= gdtile_tab<D, O>(f) ? f : d;
        int l = e;
#pragma unroll
        for (int f = 1; f < D; ++f) l = d == f ? e - gdtile_tab<D, O>(f) : l;
        long long i = o0[d] + l;
        i = i < gs.npts[d] ? i : gs.npts[d] - 1;
        const long long src = gs.off[d] + i;
        const int w = wst[src];
        tw[e] = w;
#pragma unroll
        for (int a = 0; a <= O; ++a)
#pragma unroll
            for (int k = 0; k < 4; ++k) tb[a * NTAB + e][k] = fac[4 * ((O + 1) * src + a) + k];
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
    // LDS plan as eval_grid_kernel: box [0, B) | S0 at PA; S1 overlays the box, S2 (4-D) overlays S0
    bool fits = D >= 2;
    int PA = 0;
    if constexpr (D >= 2) {
        long long H0 = 1;
#pragma unroll
        for (int d = 1; d < D; ++d) H0 *= R[d];
        const long long B = H0 * R[0], S0 = (long long)gd_nsets(1, O) * TX * H0;
        long long S1 = 0, S2 = 0;
        if constexpr (D >= 3) S1 = (long long)gd_nsets(2, O) * TX * GT::T[1] * (H0 / R[1]);
        if constexpr (D >= 4) S2 = (long long)gd_nsets(3, O) * TX * GT::T[1] * GT::T[2] * R[3];
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
            {   // dimension 1: the window row, exactly as window_sum's row(), once per derivative order
                const int i0 = tid % TX;
                const double *c0 = lds + (tw[i0] - a[0]);
                const int sz = TX * H0;
                for (int h = tid / TX; h < H0; h += GRID_NT / TX) {
                    const double *c = c0 + R[0] * h;
                    const double c_0 = c[0], c_1 = c[1], c_2 = c[2], c_3 = c[3];
#pragma unroll
                    for (int o = 0; o <= O; ++o) {
                        const double *b = tb[o * NTAB + i0];
                        double t = c_0 * b[0];
                        t = fma(c_1, b[1], t);
                        t = fma(c_2, b[2], t);
                        t = fma(c_3, b[3], t);
                        bufA[o * sz + i0 + TX * h] = t;
                    }
                }
            }
            __syncthreads();
            if constexpr (D == 2) {
                grid_derivs_stage<D, O, 1, T>(bufA, nullptr, R[1], 1, tw, tb, a[1], o0, gs, out, ldout);
            } else if constexpr (D == 3) {
                grid_derivs_stage<D, O, 1, T>(bufA, bufB, R[1], R[2], tw, tb, a[1], o0, gs, out, ldout);
                __syncthreads();
                grid_derivs_stage<D, O, 2, T>(bufB, nullptr, R[2], 1, tw, tb, a[2], o0, gs, out, ldout);
            } else {
                grid_derivs_stage<D, O, 1, T>(bufA, bufB, R[1], R[2] * R[3], tw, tb, a[1], o0, gs, out, ldout);
                __syncthreads();
                grid_derivs_stage<D, O, 2, T>(bufB, bufA, R[2], R[3], tw, tb, a[2], o0, gs, out, ldout);
                __syncthreads();
                grid_derivs_stage<D, O, 3, T>(bufA, nullptr, R[3], 1, tw, tb, a[3], o0, gs, out, ldout);
            }
        }
        return;
    }
    // general form: the gather of eval_grid_kernel's general form, all planes from the same rows
    const int s1 = D > 1 ? g.colstride[1] : 0, s2 = D > 2 ? g.colstride[2] : 0, s3 = D > 3 ? g.colstride[3] : 0;
    for (int o = tid; o < gdtile_outputs<D, O>(); o += GRID_NT) {
        int te[D];
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
            te[d] = gdtile_tab<D, O>(d) + l;
            base += tw[te[d]] * g.colstride[d];
        }
        if (!ok) continue;
        double acc[gd_nsets(D, O)];
        int k[4] = {0, 0, 0, 0};
        grid_derivs_gather<D, O, D - 1>(
            [&](int o_, int d, int kk) { return tb[o_ * NTAB + te[d]][kk]; },
            [&](int k1, int k2, int k3, double (&c)[4]) {
                const long long ci = base + k1 * s1 + k2 * s2 + k3 * s3;
                load_window_row(coef + ci, c);
            },
            k, acc);
#pragma unroll
        for (int e = 0; e < gd_nsets(D, O); ++e) out[e * ldout + idx] = (T)acc[e];
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// tile counters | factors [ntab][order + 1][4] | window starts [ntab], in the scratch evalgrid.hip keeps per thread
long long eval_grid_derivs_scratch_bytes(long long ntab, int order) { return (32LL * (order + 1) + 8) * ntab + 16; }

template <int D, int O, typename T>
static void launch_tiles(unsigned ntiles, hipStream_t st, const Grid &g, const GridShape &gs, const double *fac, const int *wst,
                         const T *coef, T *out, long long ldout, unsigned long long *stats)
{
    hipLaunchKernelGGL((eval_grid_derivs_kernel<D, O, T>), dim3(ntiles), dim3(GRID_NT), 0, st, g, gs, fac, wst, coef, out, ldout, stats);
}

template <int O, typename T>
static hipError_t launch_order(const Grid &g, const GridShape &gs, long long ntab, long long ntiles, const T *axes, const T *coef,
                               T *out, long long ldout, unsigned long long *stats, hipStream_t st)
{
    double *fac = reinterpret_cast<double *>(stats + 2);
    int *wst = reinterpret_cast<int *>(fac + 4 * (O + 1) * ntab);
    {
        dim3 gr((unsigned)((ntab + 255) / 256)), bl(256);
        hipLaunchKernelGGL((grid_derivs_table_kernel<T, O>), gr, bl, 0, st, g, gs, axes, fac, wst);
    }
    switch (g.ndim) {
    case 1: launch_tiles<1, O, T>((unsigned)ntiles, st, g, gs, fac, wst, coef, out, ldout, stats); break;
    case 2: launch_tiles<2, O, T>((unsigned)ntiles, st, g, gs, fac, wst, coef, out, ldout, stats); break;
    case 3: launch_tiles<3, O, T>((unsigned)ntiles, st, g, gs, fac, wst, coef, out, ldout, stats); break;
    default: launch_tiles<4, O, T>((unsigned)ntiles, st, g, gs, fac, wst, coef, out, ldout, stats); break;
    }
    return hipGetLastError();
}

template <typename T>
hipError_t launch_eval_grid_derivs(const Grid &g, const int64_t *npts, const T *axes, int order, const T *coef, T *out, long long ldout,
                                   hipStream_t st)
{
    GridShape gs;
    int tile[4];
    if (!eval_grid_derivs_tile(g.ndim, order, tile)) return hipErrorInvalidValue;
    if (!grid_shape(g.ndim, npts, gs)) return hipSuccess;
    const long long ntab = gs.off[MAXD];
    long long ntiles = 1;
    for (int d = 0; d < MAXD; ++d) {
        gs.ntile[d] = (gs.npts[d] + tile[d] - 1) / tile[d];
        ntiles *= gs.ntile[d];
    }
    if (ntiles > 0x7fffffffLL) return hipErrorInvalidValue;
    DevScratch<1> &s = eval_grid_scratch();
    int dev = 0;
    (void)hipGetDevice(&dev);
    const size_t need[1] = {(size_t)eval_grid_derivs_scratch_bytes(ntab, order)};
    if (hipError_t e = s.ensure(dev, need, /*may_release_plan=*/true); e != hipSuccess) return e;
    if (hipError_t e = s.wait_on(st); e != hipSuccess) return e;
    const ScratchUse<1> use{s, st};
    unsigned long long *stats = s.as<unsigned long long>(0);
    if (hipError_t e = hipMemsetAsync(stats, 0, 16, st); e != hipSuccess) return e;
    return order == 1 ? launch_order<1, T>(g, gs, ntab, ntiles, axes, coef, out, ldout, stats, st)
                      : launch_order<2, T>(g, gs, ntab, ntiles, axes, coef, out, ldout, stats, st);
}
template hipError_t launch_eval_grid_derivs<double>(const Grid &, const int64_t *, const double *, int, const double *, double *, long long, hipStream_t);
template hipError_t launch_eval_grid_derivs<float>(const Grid &, const int64_t *, const float *, int, const float *, float *, long long, hipStream_t);

}  // namespace splpak
