// The grid fit with a weight per sample (splpak_fit_grid_weighted_*): masks, dead pixels, a variance map.  The rows are
// diag(w) (A_D x ... x A_1), the normal matrix N = A^T diag(w^2) A is no Kronecker product any more, and the fit is a
// preconditioned conjugate-gradient iteration on it whose every part is a pass of fitgrid.hip (fitgriddev.hpp):
//
//   operator        N p: A p by the tile kernel of evalgrid.hip into the slab scratch, then the spread passes A^T -- the first
//                   one (the last dimension, the one that reads the sample tensor) by fitw_spread_kernel below, which loads the
//                   sample's weight and multiplies by its square on the way in; the later passes are the unit-weight passes of
//                   fit_spread_kernel on the tables of a call without axis weights;
//   right-hand side A^T (w^2 o y) and the residual A^T (w^2 o (y - A x)) with the sums of w^2 r^2: the same kernel, other modes;
//   preconditioner  M = N^_D x ... x N^_1, N^_d = A_d^T diag(m_d / S^((D-1)/D)) A_d with m_d the marginals of w^2 and S their
//                   total: the separable solve of fitgrid.hip (solve_all) on factors made from them.  prod_d m_d(i_d) / S^(D-1)
//                   IS w^2 where the weights are separable: the iteration then ends in one or two steps;
//   diag(N)         (A o A)^T w^2, and the nearest-node histogram of the xtrap rule (K_D^T x ... x K_1^T) w: the same spread on
//                   tables of squared window values and of indicators of the nearest node.
//
// A sample whose weight is 0 is selected out, never multiplied: its value may be NaN or Inf.
//
// Summation order.  The marginals: level by level from the last dimension down; a workgroup owns 256 lane positions x 32
// coordinates; a lane position's 32 terms are added in order, then the groups of 32 in order (the tensor the next level
// reduces); a coordinate's terms are added over the 64 lanes of a wave as a tree, over the 4 waves in order, then over the
// workgroups in order.  The spread: as fitgrid.hip gives it, the term being w^2 y (or w^2 u, w^2 (y - u), w^2, w), rounded
// before it meets the window value.  The dot products of the iteration: cgkernels.hpp.  No sum depends on the node block,
// the slabs, the number of fields or the entry; there are no floating-point atomics.
#include "fitgriddev.hpp"
#include "cgkernels.hpp"
#include "../../include/splpak_hip.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>

namespace splpak {

namespace {

// ---- the first spread pass with a weight per sample ------------------------------------------------------------------
enum { W_RHS = 0, W_OP = 1, W_RES = 2, W_SQ = 3, W_ONE = 4 };      // the term: w^2 y, sgn w^2 u, w^2 (y - u), w^2, w

// fit_spread_kernel's walk (fitgrid.hip: lane positions, node blocks, table order, the nodes of the window in registers, the
// slab continuation) for the pass of the LAST dimension, outer = 1.  wt[] is indexed as the samples are.  Per sample a wave
// asks for the weight and, by mode, the value and the evaluated fit: up to three requests where the unit-weight pass has
// two.  They are issued one batch ahead as there, 2 x 3 x SPREAD_BATCH = 48 in flight at most, below the 63 a wave can count.
template <typename TI, int MODE, bool UNI>
__global__ void __launch_bounds__(256)
fitw_spread_kernel(SpreadArgs a, double sgn, const TI *__restrict__ in, const TI *__restrict__ wt, const double *__restrict__ sub,
                   double *__restrict__ out, double *__restrict__ sq)
{
    constexpr bool Y = MODE == W_RHS || MODE == W_RES, U = MODE == W_OP || MODE == W_RES, RES = MODE == W_RES;
    long long i, o;
    int jb;
    if constexpr (UNI) {
        const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const long long W = (long long)blockIdx.x * 4 + wv;
        const long long lp = (W / a.nblk) * 64 + (threadIdx.x & 63);
        jb = (int)(W % a.nblk);
        i = lp % a.inner;
        o = lp / a.inner;
        if (o >= a.outer) return;
    } else {
        const long long t = (long long)blockIdx.x * 256 + threadIdx.x, r = t / a.inner;
        i = t % a.inner;
        jb = (int)(r % a.nblk);
        o = r / a.nblk;
        if (o >= a.outer) return;
    }
    const int j0 = jb * a.nbk, j1 = j0 + a.nbk < a.nod ? j0 + a.nbk : a.nod;
    const int s0 = j0 - 3 > 0 ? j0 - 3 : 0, s1 = j1 < a.nod - 3 ? j1 : a.nod - 3;
    long long p0 = a.start[s0], p1 = a.start[s1];
    p0 = p0 > a.pa ? p0 : a.pa;
    p1 = p1 < a.pb ? p1 : a.pb;
    double *__restrict__ ob = out + i;
    const TI *__restrict__ vin = Y ? in + i : nullptr;
    const TI *__restrict__ wv_ = wt + i;
    const double *__restrict__ sb = U ? sub + i : nullptr;
    auto init = [&](int j) { return (a.cont && j >= j0 && j < j1) ? ob[a.inner * j] : 0.0; };
    int cur = j0 - 3;
    double a0 = init(cur), a1 = init(cur + 1), a2 = init(cur + 2), a3 = init(cur + 3);
    auto advance = [&](int s) {
        while (cur < s) {
            if (cur >= j0) ob[a.inner * cur] = a0;
            a0 = a1; a1 = a2; a2 = a3;
            a3 = init(cur + 4);
            ++cur;
        }
    };
    double e2 = 0.0;      // residual pass: the running sum of the window start es
    int es = -1;
    auto owner_flush = [&](int s) {
        if (es >= j0 && es < j1) sq[i + a.inner * es] = e2;
        es = s;
        e2 = (s >= j0 && s < j1) ? sq[i + a.inner * s] : 0.0;
    };
    constexpr int NY = Y ? SPREAD_BATCH : 1, NU = U ? SPREAD_BATCH : 1;
    double wc[SPREAD_BATCH] = {}, wn[SPREAD_BATCH] = {}, yc[NY] = {}, yn[NY] = {}, uc[NU] = {}, un[NU] = {};
    auto fetch = [&](long long p, double (&w)[SPREAD_BATCH], double (&y)[NY], double (&u)[NU]) {
#pragma unroll
        for (int k = 0; k < SPREAD_BATCH; ++k) {
            const long long q = p + k;
            if (q < p1) {
                const long long at = a.inner * a.idx[q];
                w[k] = (double)wv_[at];
                if constexpr (Y) y[k] = (double)vin[at];
                if constexpr (U) u[k] = sb[a.inner * (q - a.pa)];
            }
        }
    };
    fetch(p0, wc, yc, uc);
    for (long long p = p0; p < p1; p += SPREAD_BATCH) {
        fetch(p + SPREAD_BATCH, wn, yn, un);
#pragma unroll
        for (int k = 0; k < SPREAD_BATCH; ++k) {
            const long long q = p + k;
            if (q < p1) {
                const int s = a.ws[q];
                const double g0 = a.G[4 * q], g1 = a.G[4 * q + 1], g2 = a.G[4 * q + 2], g3 = a.G[4 * q + 3];
                const double w = wc[k], w2 = w * w;
                const bool on = w != 0.0;      // a select: what a masked sample holds never meets the sums
                double r = 0.0, t;
                if constexpr (MODE == W_RHS) t = on ? w2 * yc[k] : 0.0;
                else if constexpr (MODE == W_OP) t = on ? sgn * (w2 * uc[k]) : 0.0;
                else if constexpr (MODE == W_RES) { r = on ? yc[k] - uc[k] : 0.0; t = on ? w2 * r : 0.0; }
                else if constexpr (MODE == W_SQ) t = w2;
                else t = w;
                advance(s);
                a0 = fma(g0, t, a0);
                a1 = fma(g1, t, a1);
                a2 = fma(g2, t, a2);
                a3 = fma(g3, t, a3);
                if constexpr (RES) {
                    if (s != es) owner_flush(s);
                    e2 = fma(t, r, e2);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < SPREAD_BATCH; ++k) {
            wc[k] = wn[k];
            if constexpr (Y) yc[k] = yn[k];
            if constexpr (U) uc[k] = un[k];
        }
    }
    advance(j1);
    if constexpr (RES) owner_flush(-1);
}

// the launch shape of fitgrid.hip's launch_spread
template <typename TI, int MODE>
hipError_t launch_wspread(const SpreadArgs &a, double sgn, const TI *in, const TI *wt, const double *sub, double *out, double *sq,
                          hipStream_t st)
{
    if (a.outer != 1) return hipErrorInvalidValue;
    const long long lanes = a.inner;
    long long units = 0, blocks = 0;
    if (lanes > (1LL << 60)) return hipErrorInvalidValue;
    const bool uni = lanes >= SPREAD_WAVE_FORM;
    if (__builtin_mul_overflow(uni ? (lanes + 63) >> 6 : lanes, (long long)a.nblk, &units)) return hipErrorInvalidValue;
    blocks = uni ? (units + 3) / 4 : (units + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (uni) hipLaunchKernelGGL((fitw_spread_kernel<TI, MODE, true>), dim3((unsigned)blocks), dim3(256), 0, st, a, sgn, in, wt, sub, out, sq);
    else hipLaunchKernelGGL((fitw_spread_kernel<TI, MODE, false>), dim3((unsigned)blocks), dim3(256), 0, st, a, sgn, in, wt, sub, out, sq);
    ++t_fit_grid_stats[2];
    return hipGetLastError();
}

// ---- the marginal pass -------------------------------------------------------------------------------------------------
constexpr int MARG_ROWS = 32;

// One level: v[i + inner c], c < n (FIRST: the weights, squared here, counted and tested; else the tensor the level above
// left).  Workgroup (x, y) owns the lane positions 256 x .. and the coordinates 32 y ..:
//   pcol[y][i]   = the sum over its coordinates, in order          (the next level adds the y in order: the reduced tensor)
//   prow[c][x]   = the sum over its lane positions: a tree over the lanes of a wave, then the 4 waves in order
//   pcnt[0 | 1][workgroup] = weights that are not 0 | that are negative or not finite
// Every load is issued whether its element exists or not (from a clamped address), all 32 before the first use.
template <typename TI, bool FIRST>
__global__ void __launch_bounds__(256)
fitw_marginal_kernel(const TI *__restrict__ v, long long inner, long long n, long long nx, double *__restrict__ pcol,
                     double *__restrict__ prow, double *__restrict__ pcnt, long long nwg)
{
    __shared__ double red[MARG_ROWS + 2][4];
    const long long x = blockIdx.x % nx, y = blockIdx.x / nx;
    const long long i = x * 256 + threadIdx.x, c0 = y * MARG_ROWS;
    const bool live = i < inner;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const TI *__restrict__ col = v + (live ? i : inner - 1);
    double t[MARG_ROWS];
#pragma unroll
    for (int k = 0; k < MARG_ROWS; ++k) {
        const long long c = c0 + k < n ? c0 + k : n - 1;
        t[k] = (double)col[inner * c];
    }
    double acc = 0.0, nz = 0.0, bad = 0.0;
#pragma unroll
    for (int k = 0; k < MARG_ROWS; ++k) {
        const bool have = live && c0 + k < n;
        double w = have ? t[k] : 0.0;
        if constexpr (FIRST) {
            nz += w != 0.0 ? 1.0 : 0.0;
            bad += (w >= 0.0 && w <= std::numeric_limits<double>::max()) ? 0.0 : 1.0;      // (a NaN fails both)
            w = w * w;
        }
        acc += w;
        for (int o2 = 32; o2 > 0; o2 >>= 1) w += __shfl_down(w, o2);
        if (lane == 0) red[k][wv] = w;
    }
    if (live) pcol[y * inner + i] = acc;
    if constexpr (FIRST) {
        for (int o2 = 32; o2 > 0; o2 >>= 1) {
            nz += __shfl_down(nz, o2);
            bad += __shfl_down(bad, o2);
        }
        if (lane == 0) { red[MARG_ROWS][wv] = nz; red[MARG_ROWS + 1][wv] = bad; }
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < MARG_ROWS + (FIRST ? 2 : 0)) {
        const double s = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
        if (k < MARG_ROWS) {
            if (c0 + k < n) prow[(c0 + k) * nx + x] = s;
        } else {
            pcnt[(k - MARG_ROWS) * nwg + blockIdx.x] = s;
        }
    }
}

// out[c] = prow[c][0] + prow[c][1] + ..: the marginal of coordinate c
__global__ void __launch_bounds__(256)
fitw_marginal_rows_kernel(const double *__restrict__ prow, long long n, long long nx, double *__restrict__ out)
{
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    double acc = 0.0;
    for (long long x = 0; x < nx; ++x) acc += prow[c * nx + x];
    out[c] = acc;
}

// out[i] = pcol[0][i] + pcol[1][i] + ..: the tensor without its last dimension
__global__ void __launch_bounds__(256)
fitw_marginal_cols_kernel(const double *__restrict__ pcol, long long inner, long long ny, double *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= inner) return;
    double acc = 0.0;
    for (long long y = 0; y < ny; ++y) acc += pcol[y * inner + i];
    out[i] = acc;
}

thread_local long long t_wstats[8];

// What the weighted fit keeps behind Layout::extra (offsets in doubles from there).
struct WLayout {
    long long G2, K, marg, pcol, prow, pcnt, WA, WB, r, z, p, q, x, sc, partial, hist, pqh, stageW, total;
    long long nwg;      // workgroups of the first marginal level
    int maxit;
};

bool plan_wlayout(const FitGridHost &h, bool xtrap, long long stage_weights_bytes, int maxit, WLayout &W)
{
    const int D = h.g.ndim;
    long long ntab = 0;
    for (int d = 0; d < D; ++d) ntab += h.ax[d].n;
    long long o = 0;
    auto take = [&](long long n) { const long long at = o; o += (n + 7) & ~7LL; return at; };
    W.G2 = take(4 * ntab);
    W.K = take(xtrap ? 4 * ntab : 0);
    W.marg = take(ntab + 3);
    long long pcol = 0, prow = 0, wa = 0, wb = 0;
    W.nwg = 0;
    for (int d = D - 1, k = 0; d >= 0; --d, ++k) {
        long long inner = 1;
        for (int e = 0; e < d; ++e) inner *= h.npts[e];      // (prod npts fits int64: the entry checked it)
        const long long n = h.npts[d], nx = (inner + 255) / 256, ny = (n + MARG_ROWS - 1) / MARG_ROWS;
        long long a = 0, b = 0, wg = 0;
        if (__builtin_mul_overflow(ny, inner, &a) || __builtin_mul_overflow(n, nx, &b) || __builtin_mul_overflow(nx, ny, &wg)) return false;
        if (wg > 0x7fffffffLL) return false;
        pcol = std::max(pcol, a);
        prow = std::max(prow, b);
        (k % 2 == 0 ? wa : wb) = std::max(k % 2 == 0 ? wa : wb, inner);
        if (d == D - 1) W.nwg = wg;
    }
    if (pcol > (1LL << 56) || prow > (1LL << 56)) return false;
    W.pcol = take(pcol); W.prow = take(prow); W.pcnt = take(2 * W.nwg); W.WA = take(wa); W.WB = take(wb);
    const long long ncol = h.g.ncol;
    W.r = take(ncol); W.z = take(ncol); W.p = take(ncol); W.q = take(ncol); W.x = take(ncol);
    W.sc = take(S_COUNT); W.partial = take(DOT_BLOCKS);
    W.hist = take(maxit + 8); W.pqh = take(maxit + 8);
    W.stageW = take((stage_weights_bytes + 7) / 8);
    W.total = o;
    W.maxit = maxit;
    return o < (1LL << 58);
}

const char *BAD_WEIGHT = "a weight is negative or not finite";

// One call on the device.  TI: the storage of the samples and of the weights.
template <typename TI>
struct WFit {
    FitGridHost &h;
    Device dv;
    WLayout W;
    hipStream_t st;
    bool xtrap;
    std::vector<double> marg;      // the last analysis on the host: the D marginals, S, non-zero weights, bad weights
    double minpiv = 0.0;
    bool outside = false;          // xtrap: a coordinate outside the counting range (decided with the rule, after the weights)
    int cg_iters = 0, cg_solves = 0;

    WFit(FitGridHost &hh, hipStream_t s, bool xt) : h(hh), dv(hh, s), st(s), xtrap(xt) {}
    double *w(long long o) const { return dv.at(dv.L.extra + o); }
    long long ntab() const { return dv.L.off[dv.D]; }

    // the scratch, the tables of fitgrid.hip (unit axis weights) and the two tables of this file
    int begin(const double *axes, long long stage_values_bytes, long long stage_coef_bytes, long long stage_weights_bytes)
    {
        const int maxit = (int)option_ll("SPLPAK_FIT_GRID_WEIGHTED_MAXIT", 1000, 1, 1000000);
        if (!plan_wlayout(h, xtrap, stage_weights_bytes, maxit, W)) {
            set_error("the weighted grid fit's intermediates are beyond what can be addressed");
            return SPLPAK_E_NOMEM;
        }
        if (int r = device_begin(dv, true, stage_values_bytes, stage_coef_bytes, W.total)) return r;
        for (int k = 0; k < 8; ++k) t_wstats[k] = 0;
        // squared window values and, for the xtrap rule, the indicator of the nearest node, both in table order
        const long long nt = ntab();
        std::vector<double> img((size_t)(W.K - W.G2 + (xtrap ? 4 * nt : 0)), 0.0);
        long long off = 0;
        for (int d = 0; d < dv.D; ++d) {
            const FitGridAxis &a = h.ax[d];
            for (long long p = 0; p < a.n; ++p) {
                const long long i = a.order[(size_t)p];
                for (int c = 0; c < 4; ++c) {
                    const double b = a.b[(size_t)i * 4 + c];
                    img[(size_t)(4 * (off + p) + c)] = b * b;
                }
                if (xtrap) {
                    // the nearest-node count of the reference (:894-902), as fit_grid_host_run takes it
                    const double t = h.g.ref_dxin[d] * (axes[off + i] - h.g.ref_xmin[d]) + 0.5;
                    const int k = (t >= 2.0e9) ? 2000000000 : (t <= -2.0e9 ? -2000000000 : (int)t);
                    const int c = k - a.ws[(size_t)i];
                    // (a counted node outside the coordinate's own window: never, by window_table; refused like the others)
                    if (!(t == t) || k < 0 || k > a.nod - 1 || c < 0 || c > 3) outside = true;
                    else img[(size_t)(W.K - W.G2 + 4 * (off + p) + c)] = 1.0;
                }
            }
            off += a.n;
        }
        SPLPAK_HIP_TRY(hipMemcpyAsync(w(W.G2), img.data(), sizeof(double) * img.size(), hipMemcpyHostToDevice, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
        return 0;
    }

    // ---- the passes
    // dst[ncol] = the spread of the term of MODE over the whole tensor in one launch; tables: null, or others than Layout::G
    template <int MODE>
    hipError_t spread_once(const TI *values, const TI *wt, double *dst, const double *tables)
    {
        double *out = dv.last == 0 ? dst : dv.at(dv.L.A);
        SpreadArgs a = spread_args(dv, dv.last);
        if (tables) a.G = tables + 4 * dv.L.off[dv.last];
        if (hipError_t e = launch_wspread<TI, MODE>(a, 1.0, values, wt, nullptr, out, nullptr, st); e != hipSuccess) return e;
        return spread_rest(dv, out, dst, tables);
    }

    // dst[ncol] = sgn N x (W_OP), or A^T (w^2 o (values - A x)) with small[2] = sum w^2 r^2 (W_RES); slab by slab
    template <int MODE>
    hipError_t spread_slabs(const TI *values, const TI *wt, const double *x, double sgn, double *dst)
    {
        const Layout &L = dv.L;
        double *out = dv.last == 0 ? dst : dv.at(L.A);
        SpreadArgs a = spread_args(dv, dv.last);
        if constexpr (MODE == W_RES)
            if (hipError_t e = hipMemsetAsync(dv.at(L.sq), 0, sizeof(double) * (size_t)(a.inner * a.nod), st); e != hipSuccess) return e;
        for (long long pa = 0, k = 0; pa < a.np; pa += L.q, ++k) {
            const long long pb = pa + L.q < a.np ? pa + L.q : a.np;
            if (hipError_t e = eval_slab(dv, x, pa, pb); e != hipSuccess) return e;
            a.pa = pa;
            a.pb = pb;
            a.cont = k > 0;
            if (hipError_t e = launch_wspread<TI, MODE>(a, sgn, values, wt, dv.at(L.AC), out, dv.at(L.sq), st); e != hipSuccess) return e;
        }
        if constexpr (MODE == W_RES)
            if (hipError_t e = residual_norm(dv, a.inner, a.nod); e != hipSuccess) return e;
        return spread_rest(dv, out, dst, nullptr);
    }

    // the marginals of wt^2, their total, the counts -> marg (one synchronisation)
    int analyse(const TI *wt)
    {
        const long long nt = ntab();
        double *mg = w(W.marg);
        const double *src = nullptr;      // the tensor of the level (the first reads wt)
        for (int d = dv.last, k = 0; d >= 0; --d, ++k) {
            long long inner = 1;
            for (int e = 0; e < d; ++e) inner *= h.npts[e];
            const long long n = h.npts[d], nx = (inner + 255) / 256, ny = (n + MARG_ROWS - 1) / MARG_ROWS;
            double *next = w(k % 2 == 0 ? W.WA : W.WB);
            if (d == dv.last)
                hipLaunchKernelGGL((fitw_marginal_kernel<TI, true>), dim3((unsigned)(nx * ny)), dim3(256), 0, st, wt, inner, n, nx, w(W.pcol),
                                   w(W.prow), w(W.pcnt), W.nwg);
            else
                hipLaunchKernelGGL((fitw_marginal_kernel<double, false>), dim3((unsigned)(nx * ny)), dim3(256), 0, st, src, inner, n, nx,
                                   w(W.pcol), w(W.prow), (double *)nullptr, 0LL);
            hipLaunchKernelGGL(fitw_marginal_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double *)w(W.prow), n, nx,
                               mg + dv.L.off[d]);
            hipLaunchKernelGGL(fitw_marginal_cols_kernel, dim3((unsigned)nx), dim3(256), 0, st, (const double *)w(W.pcol), inner, ny, next);
            SPLPAK_HIP_TRY(hipGetLastError(), SPLPAK_E_NODEVICE);
            src = next;
        }
        // the level of dimension 1 leaves a tensor of one entry: the total
        SPLPAK_HIP_TRY(hipMemcpyAsync(mg + nt, src, sizeof(double), hipMemcpyDeviceToDevice, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(launch_sum_fixed(w(W.pcnt), W.nwg, mg + nt + 1, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(launch_sum_fixed(w(W.pcnt) + W.nwg, W.nwg, mg + nt + 2, st), SPLPAK_E_NODEVICE);
        marg.resize((size_t)nt + 3);
        SPLPAK_HIP_TRY(hipMemcpyAsync(marg.data(), mg, sizeof(double) * marg.size(), hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
        ++t_wstats[7];
        return 0;
    }
    double total() const { return marg[(size_t)ntab()]; }
    double nonzero() const { return marg[(size_t)ntab() + 1]; }
    bool bad_weight() const { return marg[(size_t)ntab() + 2] != 0.0; }

    // the reference's rule node by node (:879-907) on the histogram of wt; 0 or SPLPAK_E_UNSUPPORTED
    int xtrap_rule(const TI *wt)
    {
        const int ncol = h.g.ncol;
        if (outside) {
            set_error(fit_grid_xtrap_message());
            return SPLPAK_E_UNSUPPORTED;
        }
        SPLPAK_HIP_TRY(spread_once<W_ONE>(nullptr, wt, w(W.z), w(W.K)), SPLPAK_E_NODEVICE);
        std::vector<double> hist((size_t)ncol);
        SPLPAK_HIP_TRY(hipMemcpyAsync(hist.data(), w(W.z), sizeof(double) * (size_t)ncol, hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
        double tot = 0.0, cells = 1.0;
        for (int j = 0; j < ncol; ++j) tot += hist[(size_t)j];
        for (int d = 0; d < dv.D; ++d) cells *= (double)(h.ax[d].nod - 1);
        const double need = 0.75 * tot / cells;
        for (int j = 0; j < ncol; ++j) {
            double ef = 1.0;
            int rem = j;
            for (int d = 0; d < dv.D; ++d) {
                const int jd = rem % h.ax[d].nod;
                rem /= h.ax[d].nod;
                if (jd == 0 || jd == h.ax[d].nod - 1) ef *= 0.5;
            }
            if (!(hist[(size_t)j] / ef >= need)) {
                set_error(fit_grid_xtrap_message());
                return SPLPAK_E_UNSUPPORTED;
            }
        }
        return 0;
    }

    // the preconditioner of the analysed weights: factors on the host, uploaded; then diag(N) > 0.  0 or 107
    int precondition(const TI *wt)
    {
        const long long nt = ntab();
        const double S = total();
        if (!(S > 0.0)) {
            set_error("every weight is zero");
            return 107;
        }
        const double scale = std::pow(S, (double)(dv.D - 1) / (double)dv.D);
        std::vector<double> w2((size_t)nt);
        for (long long i = 0; i < nt; ++i) w2[(size_t)i] = marg[(size_t)i] / scale;
        if (int r = fit_grid_host_reweight(h, w2.data())) return r;
        std::vector<double> chol;
        minpiv = std::numeric_limits<double>::infinity();
        for (int d = 0; d < dv.D; ++d) {
            const FitGridAxis &a = h.ax[d];
            minpiv = std::min(minpiv, a.minpiv);
            for (long long j = 0; j < 4LL * a.nod; ++j)      // (the reciprocal of the diagonal, as fitgrid.hip uploads it)
                chol.push_back(j % 4 == 0 ? 1.0 / a.chol[(size_t)j] : a.chol[(size_t)j]);
        }
        // (pageable memory: the copy has left `chol` when the call returns)
        SPLPAK_HIP_TRY(hipMemcpyAsync(dv.at(dv.L.chol), chol.data(), sizeof(double) * chol.size(), hipMemcpyHostToDevice, st), SPLPAK_E_NODEVICE);
        const int ncol = h.g.ncol;
        SPLPAK_HIP_TRY(spread_once<W_SQ>(nullptr, wt, w(W.q), w(W.G2)), SPLPAK_E_NODEVICE);
        std::vector<double> diag((size_t)ncol);
        SPLPAK_HIP_TRY(hipMemcpyAsync(diag.data(), w(W.q), sizeof(double) * (size_t)ncol, hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
        for (int j = 0; j < ncol; ++j)
            if (!(diag[(size_t)j] > 0.0)) {
                char buf[200];
                snprintf(buf, sizeof buf, "coefficient %d has no sample of non-zero weight in its support: diag(N) is not positive there", j);
                set_error(buf);
                return 107;
            }
        return 0;
    }

    hipError_t dot(const double *a, const double *b, double sign, int slot, double *hist)
    {
        hipLaunchKernelGGL(dot_partial_kernel, dim3(DOT_BLOCKS), dim3(256), 0, st, (long long)h.g.ncol, a, b, w(W.partial));
        hipLaunchKernelGGL(dot_finish_kernel, dim3(1), dim3(DOT_BLOCKS), 0, st, (const double *)w(W.partial), sign, w(W.sc), slot, hist);
        return hipGetLastError();
    }

    // W.x = N^-1 W.r (approximately): pcg.hip's pcg_solve on this operator and this preconditioner, from a zero start until
    // the preconditioned residual norm has fallen by tol; the scalars stay on the device, read back every 5 iterations.
    // 0: converged; 1: the iteration cap (W.x holds the iterate reached); 107: a breakdown; else SPLPAK_E_*.
    // The count is that of the first iterate within tol: up to 4 more have run when the read-back sees it.
    int cg_solve(const TI *wt, double tol)
    {
        const long long n = h.g.ncol;
        const dim3 gr((unsigned)((n + 255) / 256)), bl(256);
        const size_t nb = sizeof(double) * (size_t)n;
        double *r = w(W.r), *z = w(W.z), *p = w(W.p), *q = w(W.q), *x = w(W.x), *sc = w(W.sc), *hist = w(W.hist), *pqh = w(W.pqh);
        SPLPAK_HIP_TRY(hipMemsetAsync(x, 0, nb, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipMemcpyAsync(z, r, nb, hipMemcpyDeviceToDevice, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(solve_all(dv, z), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipMemcpyAsync(p, z, nb, hipMemcpyDeviceToDevice, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(dot(r, z, 1.0, S_RZ, hist), SPLPAK_E_NODEVICE);
        const int check = 5, maxit = W.maxit;
        std::vector<double> hh((size_t)maxit + 8, 0.0), hp((size_t)maxit + 8, 0.0);
        double rz0 = 0.0;
        int it = 0, read_from = 0, status = 1, count = 0;
        while (it < maxit && status == 1) {
            const int upto = std::min(maxit, it + check);
            for (; it < upto; ++it) {
                SPLPAK_HIP_TRY((spread_slabs<W_OP>(nullptr, wt, p, -1.0, q)), SPLPAK_E_NODEVICE);      // q = -N p
                SPLPAK_HIP_TRY(dot(p, q, -1.0, S_PQ, pqh + it), SPLPAK_E_NODEVICE);
                hipLaunchKernelGGL(update_xr_kernel, gr, bl, 0, st, n, (const double *)sc, x, r, (const double *)p, (const double *)q);
                SPLPAK_HIP_TRY(hipMemcpyAsync(z, r, nb, hipMemcpyDeviceToDevice, st), SPLPAK_E_NODEVICE);
                SPLPAK_HIP_TRY(solve_all(dv, z), SPLPAK_E_NODEVICE);
                SPLPAK_HIP_TRY(dot(r, z, 1.0, S_RZNEW, hist + it + 1), SPLPAK_E_NODEVICE);
                hipLaunchKernelGGL(update_p_kernel, gr, bl, 0, st, n, (const double *)sc, p, (const double *)z);
                hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(1), 0, st, sc);
                SPLPAK_HIP_TRY(hipGetLastError(), SPLPAK_E_NODEVICE);
            }
            const int first = read_from;
            read_from = it + 1;
            SPLPAK_HIP_TRY(hipMemcpyAsync(hh.data() + first, hist + first, sizeof(double) * (size_t)(it - first + 1), hipMemcpyDeviceToHost, st),
                           SPLPAK_E_NODEVICE);
            SPLPAK_HIP_TRY(hipMemcpyAsync(hp.data(), pqh, sizeof(double) * (size_t)it, hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
            SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
            if (first == 0) {
                rz0 = hh[0];
                if (rz0 == 0.0) { status = 0; count = 0; break; }      // a zero right-hand side: x = 0
                if (!(rz0 > 0.0) || !std::isfinite(rz0)) { status = 107; break; }
            }
            for (int k = std::max(1, first); k <= it; ++k) {
                const double pq = hp[(size_t)k - 1], v2 = hh[(size_t)k];
                count = k;
                if (!(pq > 0.0) || !std::isfinite(pq) || !(v2 >= 0.0) || !std::isfinite(v2)) { status = 107; break; }
                if (std::sqrt(v2 / rz0) <= tol) { status = 0; break; }
            }
        }
        cg_iters += count;
        cg_solves += 1;
        return status;
    }
};

const char *BREAKDOWN = "weighted grid fit: the conjugate-gradient iteration of field %d broke down (p^T N p <= 0 or a scalar that is not finite)";

template <typename T>
int weighted_run(FitGridHost &h, const double *axes, double xtrap, int nfields, const T *values, long long ldv, const T *weights,
                 long long ldw, T *coef, long long ldcoef, double *info, bool on_host, hipStream_t st)
{
    const int nominal = (int)option_ll("SPLPAK_FIT_GRID_REFINE", 4, 0, 1000000);
    const int hard = nominal == 0 ? 0 : (nominal > 30 ? nominal : 30);
    const int ncol = h.g.ncol;
    const size_t nb = sizeof(double) * (size_t)ncol;
    WFit<T> f(h, st, xtrap != 0.0);
    const ScratchUse<1> use{fit_grid_scratch(), st};
    const long long vbytes = on_host ? (long long)sizeof(T) * h.nsamp : 0;
    if (int r = f.begin(axes, vbytes, on_host ? (long long)sizeof(T) * ncol : 0, vbytes)) return r;
    const Layout &L = f.dv.L;
    const WLayout &W = f.W;
    double *X = f.dv.at(L.X), *small = f.dv.at(L.small);
    T *sw = reinterpret_cast<T *>(f.w(W.stageW));
    const int nsets = ldw == 0 ? 1 : nfields;
    auto weights_of = [&](int s, const T *&wk) -> int {      // the weights of set s on the device
        wk = weights + (long long)s * ldw;
        if (on_host) {
            SPLPAK_HIP_TRY(hipMemcpyAsync(sw, wk, sizeof(T) * (size_t)h.nsamp, hipMemcpyHostToDevice, st), SPLPAK_E_NODEVICE);
            wk = sw;
        }
        return 0;
    };
    // every weight set is analysed before any coefficient is written: what is refused leaves `coef` untouched
    std::vector<std::vector<double>> margs((size_t)nsets);
    const T *wk = nullptr;
    for (int s = 0; s < nsets; ++s) {
        if (int r = weights_of(s, wk)) return r;
        if (int r = f.analyse(wk)) return r;
        if (f.bad_weight()) {
            set_error(BAD_WEIGHT);
            return SPLPAK_E_BADARG;
        }
        if (xtrap != 0.0)
            if (int r = f.xtrap_rule(wk)) return r;
        margs[(size_t)s] = f.marg;
    }
    int status = 0, set_status = 0;
    for (int k = 0; k < nfields; ++k) {
        const auto t0 = std::chrono::steady_clock::now();
        const T *vk = values + (long long)k * ldv;
        T *ck = coef + (long long)k * ldcoef;
        if (k == 0 || ldw != 0) {
            if (nsets > 1)
                if (int r = weights_of(k, wk)) return r;
            f.marg = margs[(size_t)(ldw == 0 ? 0 : k)];
            set_status = f.precondition(wk);
            if (set_status != 0 && set_status != 107) return set_status;
        }
        if (on_host) {
            T *sv = reinterpret_cast<T *>(f.dv.at(L.stageV));
            SPLPAK_HIP_TRY(hipMemcpyAsync(sv, vk, sizeof(T) * (size_t)h.nsamp, hipMemcpyHostToDevice, st), SPLPAK_E_NODEVICE);
            vk = sv;
        }
        f.cg_iters = f.cg_solves = 0;
        RefineRule rule;
        double ssq = 0.0;
        int fs = set_status;      // of this field: 0 or 107
        if (fs == 0) {
            SPLPAK_HIP_TRY((f.template spread_once<W_RHS>(vk, wk, f.w(W.r), nullptr)), SPLPAK_E_NODEVICE);
            const int rc = f.cg_solve(wk, 1e-11);
            if (rc != 0 && rc != 1 && rc != 107) return rc;
            if (rc == 107) fs = 107;
            SPLPAK_HIP_TRY(hipMemcpyAsync(X, f.w(W.x), nb, hipMemcpyDeviceToDevice, st), SPLPAK_E_NODEVICE);
        }
        rule.converged = hard == 0;
        for (int it = 0; fs == 0 && it < hard && !rule.converged; ++it) {
            SPLPAK_HIP_TRY((f.template spread_slabs<W_RES>(vk, wk, X, 1.0, f.w(W.r))), SPLPAK_E_NODEVICE);
            const int rc = f.cg_solve(wk, 1e-3);
            if (rc != 0 && rc != 1 && rc != 107) return rc;
            if (rc == 107) { fs = 107; break; }
            SPLPAK_HIP_TRY(launch_axpy_absmax(ncol, X, f.w(W.x), small, st), SPLPAK_E_NODEVICE);
            double am[3];
            SPLPAK_HIP_TRY(hipMemcpyAsync(am, small, sizeof am, hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
            SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
            ssq = am[2];
            if (rule.advance(it, am)) break;
        }
        if (fs == 107 && set_status == 0) {
            char buf[200];
            snprintf(buf, sizeof buf, BREAKDOWN, k);
            set_error(buf);
        }
        if (fs == 0 && !rule.converged) {
            const double est = rule.estimate();
            if (!(est <= 1e-10)) {      // the coefficients as they stand
                char buf[200];
                snprintf(buf, sizeof buf, "weighted grid fit: the refinement of field %d left an estimated error of %.2e after %d steps", k, est,
                         rule.steps);
                set_error(buf);
                status = 107;
            }
        }
        if (fs == 107) {
            status = 107;
            SPLPAK_HIP_TRY(hipMemsetAsync(X, 0, nb, st), SPLPAK_E_NODEVICE);
        }
        if (on_host) {
            T *sc = reinterpret_cast<T *>(f.dv.at(L.stageC));
            SPLPAK_HIP_TRY(launch_fit_store<T>(X, sc, ncol, st), SPLPAK_E_NODEVICE);
            SPLPAK_HIP_TRY(hipMemcpyAsync(ck, sc, sizeof(T) * (size_t)ncol, hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
        } else {
            SPLPAK_HIP_TRY(launch_fit_store<T>(X, ck, ncol, st), SPLPAK_E_NODEVICE);
        }
        SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
        t_wstats[4] = rule.steps;
        t_wstats[5] = f.cg_iters;
        t_wstats[6] = f.cg_solves;
        if (info) {
            double *o = info + 10 * (long long)k;
            o[0] = f.nonzero(); o[1] = 0.0; o[2] = rule.steps; o[3] = rule.last_rel; o[4] = f.minpiv; o[5] = h.seconds; o[6] = 0.0;
            o[7] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            o[8] = rule.steps > 0 ? std::sqrt(ssq) : 0.0;
            o[9] = 0.0;
        }
    }
    t_wstats[0] = L.nslab;
    t_wstats[1] = L.stageV - L.AC;
    t_wstats[2] = t_fit_grid_stats[2];
    t_wstats[3] = t_fit_grid_stats[3];
    return status;
}

}  // namespace

void fit_grid_weighted_stats(long long out8[8])
{
    for (int k = 0; k < 8; ++k) out8[k] = t_wstats[k];
}

template <typename T>
int fit_grid_weighted_device(FitGridHost &h, const double *axes, double xtrap, int nfields, const T *values, long long ldv,
                             const T *weights, long long ldw, T *coef, long long ldcoef, double *info, bool on_host, hipStream_t st)
{
    try {
        return weighted_run<T>(h, axes, xtrap, nfields, values, ldv, weights, ldw, coef, ldcoef, info, on_host, st);
    } catch (const std::bad_alloc &) {
        set_error("the host tables of the weighted grid fit could not be allocated");
        return SPLPAK_E_NOMEM;
    }
}
template int fit_grid_weighted_device<double>(FitGridHost &, const double *, double, int, const double *, long long, const double *,
                                              long long, double *, long long, double *, bool, hipStream_t);
template int fit_grid_weighted_device<float>(FitGridHost &, const double *, double, int, const float *, long long, const float *, long long,
                                             float *, long long, double *, bool, hipStream_t);

int fit_grid_weighted_stage(FitGridHost &h, const double *axes, int stage, const double *weights, const double *in, double *out)
{
    try {
        const int ncol = h.g.ncol;
        const long long nin = stage == 0 ? h.nsamp : (stage == 3 ? 0 : ncol);
        WFit<double> f(h, nullptr, false);
        const ScratchUse<1> use{fit_grid_scratch(), nullptr};
        if (int r = f.begin(axes, 8 * nin, 0, 8 * h.nsamp)) return r;
        double *sv = f.dv.at(f.dv.L.stageV), *sw = f.w(f.W.stageW), *res = f.w(f.W.r);
        SPLPAK_HIP_TRY(hipMemcpy(sw, weights, sizeof(double) * (size_t)h.nsamp, hipMemcpyHostToDevice), SPLPAK_E_NODEVICE);
        if (nin > 0) SPLPAK_HIP_TRY(hipMemcpy(sv, in, sizeof(double) * (size_t)nin, hipMemcpyHostToDevice), SPLPAK_E_NODEVICE);
        if (stage == 0) {
            SPLPAK_HIP_TRY((f.spread_once<W_RHS>(sv, sw, res, nullptr)), SPLPAK_E_NODEVICE);
        } else if (stage == 1) {
            SPLPAK_HIP_TRY((f.spread_slabs<W_OP>(nullptr, sw, sv, 1.0, res)), SPLPAK_E_NODEVICE);
        } else {
            if (int r = f.analyse(sw)) return r;
            if (f.bad_weight()) {
                set_error(BAD_WEIGHT);
                return SPLPAK_E_BADARG;
            }
            if (int r = f.precondition(sw)) return r;      // (leaves diag(N) in W.q)
            if (stage == 2) {
                res = sv;
                SPLPAK_HIP_TRY(solve_all(f.dv, res), SPLPAK_E_NODEVICE);
            } else {
                const long long nt = f.ntab();
                for (long long i = 0; i < nt; ++i) out[i] = f.marg[(size_t)i];
                out += nt;
                res = f.w(f.W.q);
            }
        }
        SPLPAK_HIP_TRY(hipMemcpy(out, res, sizeof(double) * (size_t)ncol, hipMemcpyDeviceToHost), SPLPAK_E_NODEVICE);
        t_wstats[0] = f.dv.L.nslab;
        t_wstats[1] = f.dv.L.stageV - f.dv.L.AC;
        t_wstats[2] = t_fit_grid_stats[2];
        t_wstats[3] = t_fit_grid_stats[3];
        return 0;
    } catch (const std::bad_alloc &) {
        set_error("the host tables of the weighted grid fit could not be allocated");
        return SPLPAK_E_NOMEM;
    }
}

}  // namespace splpak
