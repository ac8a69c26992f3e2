// Least-squares fit of samples given on a tensor-product grid of points: values[i0 + n0 (i1 + n1 (...))] at
// (axes_1[i0], axes_2[i1], ...), weights w = prod_d waxes_d[i_d].  With no constraint rows the rows of splcw's system are
// (W_1 A_1) x ... x (W_D A_D), A_d the n_d x nodes_d matrix of the four window values per axis coordinate, and the solution is
//
//     C = (P_1 x ... x P_D) Y,    P_d = (A_d^T W_d^2 A_d)^-1 A_d^T W_d^2
//
// Host, once per call (fit_grid_host): per axis the window start and the four GENERAL-FORM values of every coordinate
// (window_table, basis.hpp), the 7-band N_d = A_d^T W_d^2 A_d and its Cholesky factor, the nearest-node histogram of the
// xtrap rule, and the TABLE ORDER of the axis: its coordinates ordered by (window start, original index).  A node j receives
// terms from the coordinates whose window start is j - 3 .. j: a contiguous range of the table order.
//
// Device, per field:
//   fit_spread_kernel   T = (A_1^T W_1^2 x ... x A_D^T W_D^2) Y one dimension at a time, the SLOWEST FIRST: the pass over the
//                       full sample tensor reads `values` once, consecutive lanes along dimension 1.  A thread owns one lane
//                       position and a block of nodes; it walks the table range of its block once, keeps the four nodes of
//                       the current window in registers and stores a node when the window has moved past it.  Neighbouring
//                       node blocks re-read three window starts' worth of samples.  Every pass shrinks the tensor by
//                       n_d / nodes_d; the last one (dimension 1, lanes along the node blocks) is small.
//   fit_solve_kernel    C = (N_1^-1 x ... x N_D^-1) T: band forward and back substitution with the uploaded factors, one
//                       thread per line of the prod nodes tensor, dimension by dimension.
//   refinement          R = Y - A C: A C by the tile kernel of evalgrid.hip on the same general-form tables (double) into a
//                       scratch, the subtraction fused into the first spread pass; solve; add.  The scratch is capped (option
//                       fit_grid_scratch_mb); larger calls go in slabs of consecutive TABLE POSITIONS of the last dimension.
//
// Summation order (the definition the header gives).  The entry of T for node j of the dimension being spread is
//     acc = 0.0;  for p in table order over the coordinates with window start j - 3 .. j:  acc = fma(g, y, acc)
// with g = waxes^2 * (window value of node j at that coordinate), rounded once on the host, and y the sample (first pass;
// REAL32 widened; a refinement step: y - (A C), one subtraction in double) or the previous pass's result.  It is a function
// of the axis alone: the node block of a launch, the number of fields, the slabs (a slab stores its running sums and the next
// one loads them: plain sequential accumulation) and the entry form change no bit.  No floating-point atomics; every sum has
// one owner.  The residual norm follows the same rule: per (lane position, window start s) the terms w^2 r^2 of the
// coordinates with that window start in table order, then fixed-order sums over s, over blocks of 4096 lanes and over the blocks.
#include "fitgriddev.hpp"
#include "../../include/splpak_hip.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>

namespace splpak {

// ---- host part -----------------------------------------------------------------------------------------------------
static const char *XTRAP_MESSAGE =
    "the sample has data-sparse nodes (or coordinates outside the counting range): constraint rows are not separable; "
    "list the points and use the point fit, or pass xtrap = 0";

const char *fit_grid_xtrap_message() { return XTRAP_MESSAGE; }

// a.nrm -> a.chol, a.minpiv, a.spd: band Cholesky, half-width 3; the rank test on the pivot before its square root
static void band_cholesky(FitGridAxis &a)
{
    const int nod = a.nod;
    double maxdiag = 0.0;
    for (int j = 0; j < nod; ++j) maxdiag = std::max(maxdiag, a.nrm[(size_t)j * 4]);
    const double floor_piv = (double)nod * std::numeric_limits<double>::epsilon() * maxdiag;
    a.minpiv = std::numeric_limits<double>::infinity();
    a.spd = true;
    auto L = [&](int r, int c) -> double & { return a.chol[(size_t)r * 4 + (r - c)]; };
    for (int j = 0; j < nod && a.spd; ++j) {
        const int lo = j - 3 > 0 ? j - 3 : 0;
        for (int m = lo; m < j; ++m) {
            double v = a.nrm[(size_t)j * 4 + (j - m)];
            for (int q = lo; q < m; ++q) v -= L(j, q) * L(m, q);
            L(j, m) = v / L(m, m);
        }
        double piv = a.nrm[(size_t)j * 4];
        for (int q = lo; q < j; ++q) piv -= L(j, q) * L(j, q);
        a.spd = piv > 0.0 && piv >= floor_piv;      // (false for a NaN)
        if (!(a.minpiv <= piv)) a.minpiv = piv;
        L(j, j) = a.spd ? std::sqrt(piv) : 1.0;
    }
}

// 0, or 107 with the message that names the first axis whose normal matrix failed the pivot test
static int axes_spd(const FitGridHost &h)
{
    for (int d = 0; d < h.g.ndim; ++d)
        if (!h.ax[d].spd) {
            char buf[200];
            snprintf(buf, sizeof buf, "the normal matrix of axis %d is not positive definite (too few distinct coordinates with a non-zero weight?)", d + 1);
            set_error(buf);
            return 107;
        }
    return 0;
}

static int fit_grid_host_run(const Grid &g, const int64_t *npts, const double *axes, const double *waxes, double xtrap, FitGridHost &h)
{
    const auto t0 = std::chrono::steady_clock::now();
    h.g = g;
    h.nsamp = 1;
    const int D = g.ndim;
    long long off = 0;
    double rule_lhs = 1.0, totlwt = 1.0, cells = 1.0;
    bool separable = true;
    for (int d = 0; d < D; ++d) {
        FitGridAxis &a = h.ax[d];
        const long long n = npts[d];
        const int nod = g.nodes[d];
        const double *x = axes + off, *w = waxes ? waxes + off : nullptr;
        off += n;
        h.npts[d] = n;
        h.nsamp *= n;
        a.n = n;
        a.nod = nod;
        a.ws.resize((size_t)n);
        a.b.resize((size_t)n * 4);
        a.w2.resize((size_t)n);
        a.order.resize((size_t)n);
        a.start.assign((size_t)nod - 2, 0);
        a.nrm.assign((size_t)nod * 4, 0.0);
        a.chol.assign((size_t)nod * 4, 0.0);
        a.nonzero = 0;
        std::vector<double> hist(xtrap != 0.0 ? (size_t)nod : 0, 0.0);
        for (long long i = 0; i < n; ++i) {
            double *b = &a.b[(size_t)i * 4];
            const int ws = window_table(g, d, x[i], 0, b);
            const double wi = w ? w[i] : 1.0, w2 = wi * wi;
            a.ws[(size_t)i] = ws;
            a.w2[(size_t)i] = w2;
            a.nonzero += wi != 0.0 ? 1 : 0;
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c <= r; ++c) a.nrm[(size_t)(ws + r) * 4 + (r - c)] += w2 * b[r] * b[c];
            if (xtrap != 0.0) {
                // the nearest-node count of the reference (:894-902), per axis; `int` truncates toward zero
                const double t = g.ref_dxin[d] * (x[i] - g.ref_xmin[d]) + 0.5;
                const int k = (t >= 2.0e9) ? 2000000000 : (t <= -2.0e9 ? -2000000000 : (int)t);
                if (!(t == t) || k < 0 || k > nod - 1 || !(wi >= 0.0)) separable = false;
                else hist[(size_t)k] += wi;
            }
        }
        // table order: a counting sort by window start (0 .. nod - 4), stable in the original index
        {
            std::vector<long long> cnt((size_t)nod - 2, 0);
            for (long long i = 0; i < n; ++i) ++cnt[(size_t)a.ws[(size_t)i]];
            long long run = 0;
            for (int s = 0; s < nod - 2; ++s) {
                a.start[(size_t)s] = run;
                run += cnt[(size_t)s];
            }
            std::vector<long long> cur(a.start);
            for (long long i = 0; i < n; ++i) a.order[(size_t)cur[(size_t)a.ws[(size_t)i]]++] = i;
        }
        band_cholesky(a);
        if (xtrap != 0.0 && separable) {
            double sum = 0.0, least = std::numeric_limits<double>::infinity();
            for (int j = 0; j < nod; ++j) {
                sum += hist[(size_t)j];
                least = std::min(least, hist[(size_t)j] / ((j == 0 || j == nod - 1) ? 0.5 : 1.0));
            }
            rule_lhs *= least;
            totlwt *= sum;
            cells *= (double)(nod - 1);
        }
    }
    h.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (xtrap != 0.0 && !(separable && rule_lhs >= 0.75 * totlwt / cells)) {
        set_error(XTRAP_MESSAGE);
        return SPLPAK_E_UNSUPPORTED;
    }
    return axes_spd(h);
}

// (Placed on a 64-byte boundary: the per-coordinate loop of fit_grid_host_run, inlined here, takes 15 ns an iteration, and the
// same instructions starting 48 bytes into a line, where a change elsewhere in the library had moved them, took 4 % longer
// over the two 4096-point axes of an image.)
__attribute__((aligned(64)))
int fit_grid_host(const Grid &g, const int64_t *npts, const double *axes, const double *waxes, double xtrap, FitGridHost &h)
{
    try {
        return fit_grid_host_run(g, npts, axes, waxes, xtrap, h);
    } catch (const std::bad_alloc &) {
        set_error("the host tables of the grid fit could not be allocated");
        return SPLPAK_E_NOMEM;
    }
}

// The factors again for other axis weights, given SQUARED (fitgridw.hip: the scaled marginals of a weight map); the window
// values and the table order stay.  N_d is summed in the order fit_grid_host_run sums it.
int fit_grid_host_reweight(FitGridHost &h, const double *w2axes)
{
    const auto t0 = std::chrono::steady_clock::now();
    long long off = 0;
    for (int d = 0; d < h.g.ndim; ++d) {
        FitGridAxis &a = h.ax[d];
        a.nrm.assign((size_t)a.nod * 4, 0.0);
        a.chol.assign((size_t)a.nod * 4, 0.0);
        a.nonzero = 0;
        for (long long i = 0; i < a.n; ++i) {
            const double *b = &a.b[(size_t)i * 4];
            const double w2 = w2axes[off + i];
            const int ws = a.ws[(size_t)i];
            a.w2[(size_t)i] = w2;
            a.nonzero += w2 != 0.0 ? 1 : 0;
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c <= r; ++c) a.nrm[(size_t)(ws + r) * 4 + (r - c)] += w2 * b[r] * b[c];
        }
        off += a.n;
        band_cholesky(a);
    }
    h.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return axes_spd(h);
}

// ---- spread ----------------------------------------------------------------------------------------------------------
// The lane positions of a pass are its (i, o) pairs, i fastest: inner * outer of them.  UNI (from SPREAD_WAVE_FORM lane
// positions on): a wave owns 64 consecutive ones and ONE node block, so the walk over the table is the same in every lane
// (scalar loads of the table entries, no divergence); where `inner` is short the lanes run on into o (the pass of dimension 1:
// along o alone, every lane walking a row of its own).  Otherwise (1-D, toy sizes) one thread per (i, node block, o).
template <typename TI, bool RES, bool UNI>
__global__ void __launch_bounds__(256)
fit_spread_kernel(SpreadArgs a, const TI *__restrict__ in, const double *__restrict__ sub, double *__restrict__ out,
                  double *__restrict__ sq)
{
    long long i, o;
    int jb;
    if constexpr (UNI) {
        const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        // node blocks fastest: the waves that re-read each other's samples run side by side (one workgroup when there are 4 blocks)
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
    double *__restrict__ ob = out + i + a.inner * ((long long)a.nod * o);
    const TI *__restrict__ vin = RES ? in + i : in + i + a.inner * (a.np * o);
    const double *__restrict__ sb = RES ? sub + i : nullptr;
    auto init = [&](int j) { return (a.cont && j >= j0 && j < j1) ? ob[a.inner * j] : 0.0; };
    int cur = j0 - 3;
    double a0 = init(cur), a1 = init(cur + 1), a2 = init(cur + 2), a3 = init(cur + 3);
    // the window moves on to start s: the nodes it leaves are complete
    auto advance = [&](int s) {
        while (cur < s) {
            if (cur >= j0) ob[a.inner * cur] = a0;
            a0 = a1; a1 = a2; a2 = a3;
            a3 = init(cur + 4);
            ++cur;
        }
    };
    double wl2 = 1.0, e2 = 0.0;      // residual pass: the lane's weight; the running sum of the window start es
    int es = -1;
    if constexpr (RES) {
        long long rem = i;
        for (int e = 0; e < a.nlow; ++e) {
            wl2 *= a.w2lo[e][rem % a.nlo[e]];
            rem /= a.nlo[e];
        }
    }
    auto owner_flush = [&](int s) {      // the sum of window start es is complete; s is next (-1: none)
        if (es >= j0 && es < j1) sq[i + a.inner * es] = e2;
        es = s;
        e2 = (s >= j0 && s < j1) ? sq[i + a.inner * s] : 0.0;
    };
    // The samples of a batch are asked for one batch ahead of their use, so that a wave keeps up to 2 SPREAD_BATCH loads in
    // flight: with four (and nothing ahead) the first pass of a 512^3 volume waited for memory 38 times per wave and ran at
    // 3.2 TB/s of `values`, the same time for REAL32 samples of half the bytes.  The table entries are read at the use.
    double yc[SPREAD_BATCH] = {}, yn[SPREAD_BATCH] = {}, uc[RES ? SPREAD_BATCH : 1] = {}, un[RES ? SPREAD_BATCH : 1] = {};
    auto fetch = [&](long long p, double (&y)[SPREAD_BATCH], double (&u)[RES ? SPREAD_BATCH : 1]) {
#pragma unroll
        for (int k = 0; k < SPREAD_BATCH; ++k) {
            const long long q = p + k;
            if (q < p1) {
                y[k] = (double)vin[a.inner * a.idx[q]];
                if constexpr (RES) u[k] = sb[a.inner * (q - a.pa)];
            }
        }
    };
    fetch(p0, yc, uc);
    for (long long p = p0; p < p1; p += SPREAD_BATCH) {
        fetch(p + SPREAD_BATCH, yn, un);
#pragma unroll
        for (int k = 0; k < SPREAD_BATCH; ++k) {
            const long long q = p + k;
            if (q < p1) {
                const int s = a.ws[q];
                const double g0 = a.G[4 * q], g1 = a.G[4 * q + 1], g2 = a.G[4 * q + 2], g3 = a.G[4 * q + 3];
                double y = yc[k];
                if constexpr (RES) y -= uc[k];
                advance(s);
                a0 = fma(g0, y, a0);
                a1 = fma(g1, y, a1);
                a2 = fma(g2, y, a2);
                a3 = fma(g3, y, a3);
                if constexpr (RES) {
                    if (s != es) owner_flush(s);
                    e2 = fma((wl2 * a.w2s[q]) * y, y, e2);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < SPREAD_BATCH; ++k) {
            yc[k] = yn[k];
            if constexpr (RES) uc[k] = un[k];
        }
    }
    advance(j1);
    if constexpr (RES) owner_flush(-1);
}

template <typename TI, bool RES>
static hipError_t launch_spread(const SpreadArgs &a, const TI *in, const double *sub, double *out, double *sq, hipStream_t st)
{
    long long lanes = 0, units = 0, blocks = 0;
    if (__builtin_mul_overflow(a.inner, a.outer, &lanes) || lanes > (1LL << 60)) return hipErrorInvalidValue;
    const bool uni = lanes >= SPREAD_WAVE_FORM;
    if (__builtin_mul_overflow(uni ? (lanes + 63) >> 6 : lanes, (long long)a.nblk, &units)) return hipErrorInvalidValue;
    blocks = uni ? (units + 3) / 4 : (units + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (uni) hipLaunchKernelGGL((fit_spread_kernel<TI, RES, true>), dim3((unsigned)blocks), dim3(256), 0, st, a, in, sub, out, sq);
    else hipLaunchKernelGGL((fit_spread_kernel<TI, RES, false>), dim3((unsigned)blocks), dim3(256), 0, st, a, in, sub, out, sq);
    return hipGetLastError();
}

hipError_t launch_spread_plain(const SpreadArgs &a, const double *in, double *out, hipStream_t st)
{
    return launch_spread<double, false>(a, in, nullptr, out, nullptr, st);
}

// Nodes per block: the largest of 64, 32, .. that still gives the pass 8192 waves (32 per CU: a wave's walk is a chain of
// memory waits, so what hides them is waves); a pass that misses that even with one node per block takes 1, and one of fewer
// than 2048 waves in all, where nothing matters, 4.  No bit of the result depends on it, which the diagnostic option
// fit_grid_node_block (1 .. 64) lets a test show.
int fit_grid_node_block(long long inner, long long outer, int nod)
{
    const long long forced = option_ll("SPLPAK_FIT_GRID_NODE_BLOCK", 0, 0, 64);
    if (forced > 0) return (int)forced;
    const double per_block = (double)inner * (double)outer / 64.0;      // waves per node block
    for (int nbk = 64; nbk > 1; nbk >>= 1)
        if (per_block * (double)((nod + nbk - 1) / nbk) >= 8192.0) return nbk;
    return per_block * (double)nod >= 2048.0 ? 1 : 4;
}

// ---- solve -----------------------------------------------------------------------------------------------------------
// x[i + inner (j + nod o)], j = 0 .. nod - 1: one line per thread, L L^T x = t in place.  L(j, j - k) at chol[4 j + k] for
// k = 1 .. 3, the RECIPROCAL of L(j, j) at chol[4 j] (formed once on the host).  The recurrence is a chain of dependent
// operations; what the line contributes is loaded SOLVE_CH entries ahead of it, so that a thread waits for memory once per
// chunk and not once per entry.
constexpr int SOLVE_CH = 8;

// One step of L z = t at row j: l = the row's four entries (the reciprocal of the diagonal first), s = t[j], z1 .. z3 the
// three results before it.  Returns z[j].  (The step of the backward sweep stays written out in both kernels: as a function
// of this kind the chunked kernel compiled its row tests to other branches.)
__device__ inline double band_forward(const double *l, double s, double z1, double z2, double z3)
{
    s = fma(-l[1], z1, s);
    s = fma(-l[2], z2, s);
    s = fma(-l[3], z3, s);
    return s * l[0];
}

__global__ void __launch_bounds__(256)
fit_solve_kernel(const double *__restrict__ chol, int nod, long long inner, long long lines, double *__restrict__ x)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= lines) return;
    double *__restrict__ v = x + t % inner + inner * ((long long)nod * (t / inner));
    double r[SOLVE_CH];
    double z1 = 0.0, z2 = 0.0, z3 = 0.0;
    for (int j0 = 0; j0 < nod; j0 += SOLVE_CH) {
#pragma unroll
        for (int k = 0; k < SOLVE_CH; ++k)
            if (j0 + k < nod) r[k] = v[inner * (j0 + k)];
#pragma unroll
        for (int k = 0; k < SOLVE_CH; ++k) {
            if (j0 + k < nod) {
                const double s = band_forward(chol + 4 * (long long)(j0 + k), r[k], z1, z2, z3);
                r[k] = s;
                z3 = z2; z2 = z1; z1 = s;
            }
        }
#pragma unroll
        for (int k = 0; k < SOLVE_CH; ++k)
            if (j0 + k < nod) v[inner * (j0 + k)] = r[k];
    }
    z1 = z2 = z3 = 0.0;
    for (int j0 = ((nod - 1) / SOLVE_CH) * SOLVE_CH; j0 >= 0; j0 -= SOLVE_CH) {
#pragma unroll
        for (int k = 0; k < SOLVE_CH; ++k)
            if (j0 + k < nod) r[k] = v[inner * (j0 + k)];
#pragma unroll
        for (int k = SOLVE_CH - 1; k >= 0; --k) {
            const int j = j0 + k;
            if (j < nod) {
                const double *l = chol + 4 * (long long)j;
                double s = r[k];
                if (j + 1 < nod) s = fma(-l[4 + 1], z1, s);
                if (j + 2 < nod) s = fma(-l[8 + 2], z2, s);
                if (j + 3 < nod) s = fma(-l[12 + 3], z3, s);
                s *= l[0];
                r[k] = s;
                z3 = z2; z2 = z1; z1 = s;
            }
        }
#pragma unroll
        for (int k = 0; k < SOLVE_CH; ++k)
            if (j0 + k < nod) v[inner * (j0 + k)] = r[k];
    }
}

// The same recurrences, the same operations in the same order, for a line of at most NR entries held in registers: one wait
// for memory per line instead of one per chunk and sweep (64^3 nodes have 4096 lines per dimension -- 64 waves, each a
// chain of 128 dependent steps: the chunked form took 40 us per dimension there, of which the arithmetic is a tenth).
template <int NR>
__global__ void __launch_bounds__(256)
fit_solve_reg_kernel(const double *__restrict__ chol, int nod, long long inner, long long lines, double *__restrict__ x)
{
    // the factor in LDS: read from global memory at every step (scalar loads, as many as the scalar registers hold at a
    // time) the chain waited for them, 33 us for 128 steps
    __shared__ double sl[4 * NR];
    for (int e = threadIdx.x; e < 4 * nod; e += 256) sl[e] = chol[e];
    __syncthreads();
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= lines) return;
    double *__restrict__ v = x + t % inner + inner * ((long long)nod * (t / inner));
    double r[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k)
        if (k < nod) r[k] = v[inner * k];
    double z1 = 0.0, z2 = 0.0, z3 = 0.0;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        if (k < nod) {
            const double s = band_forward(sl + 4 * k, r[k], z1, z2, z3);
            r[k] = s;
            z3 = z2; z2 = z1; z1 = s;
        }
    }
    z1 = z2 = z3 = 0.0;
#pragma unroll
    for (int k = NR - 1; k >= 0; --k) {
        if (k < nod) {
            const double *l = sl + 4 * k;
            double s = r[k];
            if (k + 1 < nod) s = fma(-l[4 + 1], z1, s);
            if (k + 2 < nod) s = fma(-l[8 + 2], z2, s);
            if (k + 3 < nod) s = fma(-l[12 + 3], z3, s);
            s *= l[0];
            r[k] = s;
            z3 = z2; z2 = z1; z1 = s;
        }
    }
#pragma unroll
    for (int k = 0; k < NR; ++k)
        if (k < nod) v[inner * k] = r[k];
}

// ---- the residual norm's fixed-order sums, the final store ---------------------------------------------------------------
__global__ void __launch_bounds__(256)
fit_ssq_rows_kernel(const double *__restrict__ sq, long long inner, int nod, double *__restrict__ rows)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= inner) return;
    double acc = 0.0;
    for (int s = 0; s < nod; ++s) acc += sq[i + inner * s];
    rows[i] = acc;
}

// part[b] = the sum of v[4096 b .. 4096 (b + 1)): thread t adds its 16 entries t, t + 256, .. in order, then a tree
__global__ void __launch_bounds__(256)
fit_block_sum_kernel(const double *__restrict__ v, long long n, double *__restrict__ part)
{
    __shared__ double red[256];
    const long long base = (long long)blockIdx.x * 4096;
    double acc = 0.0;
    for (int k = 0; k < 16; ++k) {
        const long long i = base + threadIdx.x + 256 * k;
        acc += i < n ? v[i] : 0.0;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

template <typename T>
__global__ void __launch_bounds__(256)
fit_store_kernel(const double *__restrict__ x, T *__restrict__ coef, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) coef[i] = (T)x[i];      // REAL32: the one rounding
}

template <typename T>
hipError_t launch_fit_store(const double *x, T *coef, int n, hipStream_t st)
{
    hipLaunchKernelGGL((fit_store_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, coef, n);
    return hipGetLastError();
}
template hipError_t launch_fit_store<double>(const double *, double *, int, hipStream_t);
template hipError_t launch_fit_store<float>(const double *, float *, int, hipStream_t);

// ---- device side of a call -------------------------------------------------------------------------------------------
static thread_local DevScratch<1> g_fscratch;

DevScratch<1> &fit_grid_scratch() { return g_fscratch; }
thread_local long long t_fit_grid_stats[8];

void fit_grid_stats(long long out8[8])
{
    for (int k = 0; k < 8; ++k) out8[k] = t_fit_grid_stats[k];
}

void fit_grid_scratch_shutdown() { g_fscratch.release(); }

// sizes; false: beyond what can be addressed
static bool plan_layout(const FitGridHost &h, bool refine, long long stage_values_bytes, long long stage_coef_bytes, long long extra, Layout &L)
{
    const int D = h.g.ndim, last = D - 1;
    long long ntab = 0, nn = 0, ns = 0;
    for (int d = 0; d <= MAXD; ++d) {
        L.off[d] = ntab; L.offn[d] = nn; L.offs[d] = ns;
        if (d < D) { ntab += h.ax[d].n; nn += h.ax[d].nod; ns += h.ax[d].nod - 2; }
    }
    if (ntab > (1LL << 55)) return false;
    long long o = 0;
    auto take = [&](long long n) { const long long at = o; o += n; return at; };
    L.G = take(4 * ntab); L.fac = take(4 * ntab); L.w2o = take(ntab); L.w2s = take(ntab); L.idx = take(ntab);
    L.start = take(ns); L.chol = take(4 * nn);
    L.wsS = take((ntab + 1) / 2); L.wstE = take((ntab + 1) / 2);
    L.tables = o;
    L.small = take(8);
    L.X = take(h.g.ncol); L.R = take(h.g.ncol);
    // the spread passes, slowest dimension first: pass d writes prod_{e<d} npts_e * nodes_d * prod_{e>d} nodes_e
    L.szA = L.szB = 0;
    bool big = false;
    int k = 0;
    for (int d = last; d >= 1; --d, ++k) {
        long long sz = 1;
        for (int e = 0; e < D; ++e) big = big || __builtin_mul_overflow(sz, e < d ? h.npts[e] : (long long)h.ax[e].nod, &sz);
        (k % 2 == 0 ? L.szA : L.szB) = std::max(k % 2 == 0 ? L.szA : L.szB, sz);
    }
    if (big || L.szA > (1LL << 58) || L.szB > (1LL << 58)) return false;
    L.A = take(L.szA); L.B = take(L.szB);
    L.sq = L.rows = L.part = L.AC = o;
    L.q = 0; L.nslab = 0;
    if (refine) {
        long long row = 1;      // samples per position of the last dimension
        for (int e = 0; e < last; ++e) row *= h.npts[e];      // (prod npts fits int64: the entry checked it)
        long long sq = 0, q = 0;
        if (__builtin_mul_overflow(row, (long long)h.ax[last].nod, &sq) || sq > (1LL << 58)) return false;
        const long long cap = option_ll("SPLPAK_FIT_GRID_SCRATCH_MB", 256, 1, 1LL << 40) * (1LL << 17);
        if (!eval_grid_slab(D, h.npts, row, cap, q)) return false;
        q = q < 1 ? 1 : q;      // a single position above the cap goes whole
        q = q > h.npts[last] ? h.npts[last] : q;
        long long ac = 0;
        if (__builtin_mul_overflow(row, q, &ac) || ac > (1LL << 58)) return false;
        L.q = q;
        L.nslab = (h.npts[last] + q - 1) / q;
        L.sq = take(sq); L.rows = take(row); L.part = take((row + 4095) / 4096); L.AC = take(ac);
    }
    L.stageV = take((stage_values_bytes + 7) / 8);
    L.stageC = take((stage_coef_bytes + 7) / 8);
    if (extra < 0 || extra > (1LL << 58)) return false;
    L.extra = take(extra);
    L.total = o;
    return o < (1LL << 59);
}

// the tables of the call, as the kernels read them, in one host image
static void fill_tables(const FitGridHost &h, const Layout &L, std::vector<double> &img)
{
    img.assign((size_t)L.tables, 0.0);
    int *wsS = reinterpret_cast<int *>(&img[(size_t)L.wsS]), *wstE = reinterpret_cast<int *>(&img[(size_t)L.wstE]);
    long long *idx = reinterpret_cast<long long *>(&img[(size_t)L.idx]), *start = reinterpret_cast<long long *>(&img[(size_t)L.start]);
    const int D = h.g.ndim;
    for (int d = 0; d < D; ++d) {
        const FitGridAxis &a = h.ax[d];
        const long long o = L.off[d];
        for (long long p = 0; p < a.n; ++p) {
            const long long i = a.order[(size_t)p];
            // the evaluation tables: the last dimension in table order (a slab is a range of it), the others as given
            const long long ie = d == D - 1 ? i : p;
            for (int c = 0; c < 4; ++c) {
                img[(size_t)(L.G + 4 * (o + p) + c)] = a.w2[(size_t)i] * a.b[(size_t)i * 4 + c];
                img[(size_t)(L.fac + 4 * (o + p) + c)] = a.b[(size_t)ie * 4 + c];
            }
            wstE[o + p] = a.ws[(size_t)ie];
            wsS[o + p] = a.ws[(size_t)i];
            img[(size_t)(L.w2o + o + p)] = a.w2[(size_t)p];
            img[(size_t)(L.w2s + o + p)] = a.w2[(size_t)i];
            idx[o + p] = i;
        }
        for (int s = 0; s < a.nod - 2; ++s) start[L.offs[d] + s] = a.start[(size_t)s];
        for (long long j = 0; j < 4LL * a.nod; ++j)      // (the kernel multiplies by the reciprocal of the diagonal)
            img[(size_t)(L.chol + 4 * L.offn[d] + j)] = j % 4 == 0 ? 1.0 / a.chol[(size_t)j] : a.chol[(size_t)j];
    }
}

SpreadArgs spread_args(const Device &dv, int d)
{
    const FitGridHost &h = dv.h;
    const Layout &L = dv.L;
    SpreadArgs a;
    memset(&a, 0, sizeof a);
    a.inner = a.outer = 1;
    for (int e = 0; e < d; ++e) a.inner *= h.npts[e];
    for (int e = d + 1; e < dv.D; ++e) a.outer *= h.ax[e].nod;
    a.np = h.ax[d].n;
    a.pa = 0;
    a.pb = a.np;
    a.nod = h.ax[d].nod;
    a.nbk = fit_grid_node_block(a.inner, a.outer, a.nod);
    a.nblk = (a.nod + a.nbk - 1) / a.nbk;
    a.G = dv.at(L.G) + 4 * L.off[d];
    a.ws = reinterpret_cast<const int *>(dv.at(L.wsS)) + L.off[d];
    a.idx = reinterpret_cast<const long long *>(dv.at(L.idx)) + L.off[d];
    a.start = reinterpret_cast<const long long *>(dv.at(L.start)) + L.offs[d];
    a.w2s = dv.at(L.w2s) + L.off[d];
    a.nlow = d;
    for (int e = 0; e < MAXD; ++e) {
        a.nlo[e] = e < d ? h.npts[e] : 1;
        a.w2lo[e] = dv.at(L.w2o) + L.off[e < dv.D ? e : 0];
    }
    return a;
}

// the passes below the last dimension: cur (the last dimension's result) -> dst[ncol]
hipError_t spread_rest(const Device &dv, const double *cur, double *dst, const double *tables)
{
    const Layout &L = dv.L;
    int k = 1;
    for (int d = dv.last - 1; d >= 0; --d, ++k) {
        double *out = d == 0 ? dst : dv.at(k % 2 == 0 ? L.A : L.B);
        SpreadArgs a = spread_args(dv, d);
        if (tables) a.G = tables + 4 * L.off[d];
        if (hipError_t e = launch_spread<double, false>(a, cur, nullptr, out, nullptr, dv.st); e != hipSuccess) return e;
        ++t_fit_grid_stats[2];
        cur = out;
    }
    return hipSuccess;
}

// dst[ncol] = the spread of the samples
template <typename TI>
static hipError_t spread_values(const Device &dv, const TI *values, double *dst)
{
    double *out = dv.last == 0 ? dst : dv.at(dv.L.A);
    const SpreadArgs a = spread_args(dv, dv.last);
    if (hipError_t e = launch_spread<TI, false>(a, values, nullptr, out, nullptr, dv.st); e != hipSuccess) return e;
    ++t_fit_grid_stats[2];
    return spread_rest(dv, out, dst, nullptr);
}

// small[2] = the sum of sq[inner][nod], the per-(lane position, window start) sums of a residual pass, in the header's order
hipError_t residual_norm(const Device &dv, long long inner, int nod)
{
    const Layout &L = dv.L;
    const long long nb = (inner + 255) / 256, np = (inner + 4095) / 4096;
    if (nb > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fit_ssq_rows_kernel, dim3((unsigned)nb), dim3(256), 0, dv.st, dv.at(L.sq), inner, nod, dv.at(L.rows));
    hipLaunchKernelGGL(fit_block_sum_kernel, dim3((unsigned)np), dim3(256), 0, dv.st, dv.at(L.rows), inner, dv.at(L.part));
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    return launch_sum_fixed(dv.at(L.part), np, dv.at(L.small) + 2, dv.st);
}

// Layout::AC = A x at the table positions pa .. pb - 1 of the last dimension (a slab: at most Layout::q of them)
hipError_t eval_slab(const Device &dv, const double *x, long long pa, long long pb)
{
    const FitGridHost &h = dv.h;
    const Layout &L = dv.L;
    GridShape s;      // (its table offsets are Layout::off: the prefix of npts)
    if (!grid_shape(dv.D, h.npts, s)) return hipErrorInvalidValue;
    s.npts[dv.last] = pb - pa;
    s.off[dv.last] += pa;
    const int *wst = reinterpret_cast<const int *>(dv.at(L.wstE));
    return launch_eval_grid_tables<double, double>(h.g, s, dv.at(L.fac), wst, x, dv.at(L.AC), nullptr, dv.st);
}

// dst[ncol] = the spread of values - A x, slab by slab; small[2] = the sum of the squared weighted residuals
template <typename TI>
static hipError_t spread_residual(const Device &dv, const TI *values, const double *x, double *dst)
{
    const Layout &L = dv.L;
    const int last = dv.last;
    double *out = last == 0 ? dst : dv.at(L.A);
    SpreadArgs a = spread_args(dv, last);
    if (hipError_t e = hipMemsetAsync(dv.at(L.sq), 0, sizeof(double) * (size_t)(a.inner * a.nod), dv.st); e != hipSuccess) return e;
    for (long long pa = 0, k = 0; pa < a.np; pa += L.q, ++k) {
        const long long pb = pa + L.q < a.np ? pa + L.q : a.np;
        if (hipError_t e = eval_slab(dv, x, pa, pb); e != hipSuccess) return e;
        a.pa = pa;
        a.pb = pb;
        a.cont = k > 0;
        if (hipError_t e = launch_spread<TI, true>(a, values, dv.at(L.AC), out, dv.at(L.sq), dv.st); e != hipSuccess) return e;
        ++t_fit_grid_stats[2];
    }
    if (hipError_t e = residual_norm(dv, a.inner, a.nod); e != hipSuccess) return e;
    return spread_rest(dv, out, dst, nullptr);
}

// x[ncol] <- (N_1^-1 x ... x N_D^-1) x
hipError_t solve_all(const Device &dv, double *x)
{
    const FitGridHost &h = dv.h;
    long long inner = 1;
    for (int d = 0; d < dv.D; ++d) {
        const int nod = h.ax[d].nod;
        const long long lines = h.g.ncol / nod;
        const dim3 gr((unsigned)((lines + 255) / 256)), bl(256);
        const double *chol = dv.at(dv.L.chol) + 4 * dv.L.offn[d];
        if (nod <= 16) hipLaunchKernelGGL(fit_solve_reg_kernel<16>, gr, bl, 0, dv.st, chol, nod, inner, lines, x);
        else if (nod <= 64) hipLaunchKernelGGL(fit_solve_reg_kernel<64>, gr, bl, 0, dv.st, chol, nod, inner, lines, x);
        else hipLaunchKernelGGL(fit_solve_kernel, gr, bl, 0, dv.st, chol, nod, inner, lines, x);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        ++t_fit_grid_stats[3];
        inner *= nod;
    }
    return hipSuccess;
}

// the scratch of the call and its tables on the device; 0 or a status
int device_begin(Device &dv, bool refine, long long stage_values_bytes, long long stage_coef_bytes, long long extra)
{
    for (int k = 0; k < 8; ++k) t_fit_grid_stats[k] = 0;
    if (!plan_layout(dv.h, refine, stage_values_bytes, stage_coef_bytes, extra, dv.L)) {
        set_error("the grid fit's intermediates are beyond what can be addressed");
        return SPLPAK_E_NOMEM;
    }
    int dev = 0;
    (void)hipGetDevice(&dev);
    const size_t need[1] = {(size_t)dv.L.total * 8};
    if (hipError_t e = g_fscratch.ensure(dev, need, /*may_release_plan=*/true); e != hipSuccess) {
        char buf[160];
        snprintf(buf, sizeof buf, "hipMalloc of %.3f GB for the grid fit failed: %s", (double)need[0] / 1e9, hipGetErrorString(e));
        set_error(buf);
        (void)hipGetLastError();
        return SPLPAK_E_NOMEM;
    }
    dv.base = g_fscratch.as<double>(0);
    SPLPAK_HIP_TRY(g_fscratch.wait_on(dv.st), SPLPAK_E_NODEVICE);
    std::vector<double> img;
    fill_tables(dv.h, dv.L, img);
    // (pageable memory: the copy has left `img` when the call returns)
    SPLPAK_HIP_TRY(hipMemcpyAsync(dv.base, img.data(), sizeof(double) * img.size(), hipMemcpyHostToDevice, dv.st), SPLPAK_E_NODEVICE);
    SPLPAK_HIP_TRY(hipStreamSynchronize(dv.st), SPLPAK_E_NODEVICE);
    if (refine) {
        t_fit_grid_stats[0] = dv.L.nslab;
        t_fit_grid_stats[1] = dv.L.stageV - dv.L.AC;      // the doubles of A C
    }
    return 0;
}

template <typename T>
static int fit_grid_device_run(const FitGridHost &h, int nfields, const T *values, long long ldv, T *coef, long long ldcoef, double *info,
                               bool on_host, hipStream_t st)
{
    const int nominal = (int)option_ll("SPLPAK_FIT_GRID_REFINE", 4, 0, 1000000);
    const int hard = nominal == 0 ? 0 : (nominal > 30 ? nominal : 30);
    const int ncol = h.g.ncol;
    Device dv(h, st);
    const ScratchUse<1> use{g_fscratch, st};
    if (int r = device_begin(dv, hard > 0, on_host ? (long long)sizeof(T) * h.nsamp : 0, on_host ? (long long)sizeof(T) * ncol : 0, 0)) return r;
    const Layout &L = dv.L;
    double *X = dv.at(L.X), *R = dv.at(L.R), *small = dv.at(L.small);
    int status = 0;
    for (int k = 0; k < nfields; ++k) {
        const auto t0 = std::chrono::steady_clock::now();
        const T *vk = values + (long long)k * ldv;
        T *ck = coef + (long long)k * ldcoef;
        if (on_host) {
            T *sv = reinterpret_cast<T *>(dv.at(L.stageV));
            SPLPAK_HIP_TRY(hipMemcpyAsync(sv, vk, sizeof(T) * (size_t)h.nsamp, hipMemcpyHostToDevice, st), SPLPAK_E_NODEVICE);
            vk = sv;
        }
        SPLPAK_HIP_TRY(spread_values<T>(dv, vk, X), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(solve_all(dv, X), SPLPAK_E_NODEVICE);
        // the fit's own rule (planfit.hip refinement_advance): stop when the estimated remaining error is below tol, go on
        // while the corrections contract, fail (107) when that leaves an estimate above the parity bar
        RefineRule rule;
        double ssq = 0.0;
        rule.converged = hard == 0;
        for (int it = 0; it < hard && !rule.converged; ++it) {
            SPLPAK_HIP_TRY(spread_residual<T>(dv, vk, X, R), SPLPAK_E_NODEVICE);
            SPLPAK_HIP_TRY(solve_all(dv, R), SPLPAK_E_NODEVICE);
            SPLPAK_HIP_TRY(launch_axpy_absmax(ncol, X, R, small, st), SPLPAK_E_NODEVICE);
            double am[3];
            SPLPAK_HIP_TRY(hipMemcpyAsync(am, small, sizeof am, hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
            SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
            ssq = am[2];
            if (rule.advance(it, am)) break;
        }
        const int steps = rule.steps;
        const double last_rel = rule.last_rel;
        if (!rule.converged) {
            const double est = rule.estimate();
            if (!(est <= 1e-10)) {
                char buf[200];
                snprintf(buf, sizeof buf, "grid fit: the refinement of field %d left an estimated error of %.2e after %d steps", k, est, steps);
                set_error(buf);
                status = 107;
            }
        }
        if (on_host) {
            T *sc = reinterpret_cast<T *>(dv.at(L.stageC));
            hipLaunchKernelGGL((fit_store_kernel<T>), dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, st, X, sc, ncol);
            SPLPAK_HIP_TRY(hipGetLastError(), SPLPAK_E_NODEVICE);
            SPLPAK_HIP_TRY(hipMemcpyAsync(ck, sc, sizeof(T) * (size_t)ncol, hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
        } else {
            hipLaunchKernelGGL((fit_store_kernel<T>), dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, st, X, ck, ncol);
            SPLPAK_HIP_TRY(hipGetLastError(), SPLPAK_E_NODEVICE);
        }
        SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
        t_fit_grid_stats[4] = steps;
        if (info) {
            double *f = info + 10 * (long long)k;
            double rows = 1.0, minpiv = std::numeric_limits<double>::infinity();
            for (int d = 0; d < dv.D; ++d) {
                rows *= (double)h.ax[d].nonzero;
                minpiv = std::min(minpiv, h.ax[d].minpiv);
            }
            f[0] = rows; f[1] = 0.0; f[2] = steps; f[3] = last_rel; f[4] = minpiv; f[5] = h.seconds; f[6] = 0.0;
            f[7] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            f[8] = steps > 0 ? std::sqrt(ssq) : 0.0;
            f[9] = 0.0;
        }
    }
    return status;
}

template <typename T>
int fit_grid_device(const FitGridHost &h, int nfields, const T *values, long long ldv, T *coef, long long ldcoef, double *info,
                    bool on_host, hipStream_t st)
{
    try {
        return fit_grid_device_run<T>(h, nfields, values, ldv, coef, ldcoef, info, on_host, st);
    } catch (const std::bad_alloc &) {
        set_error("the host image of the grid fit's tables could not be allocated");
        return SPLPAK_E_NOMEM;
    }
}
template int fit_grid_device<double>(const FitGridHost &, int, const double *, long long, double *, long long, double *, bool, hipStream_t);
template int fit_grid_device<float>(const FitGridHost &, int, const float *, long long, float *, long long, double *, bool, hipStream_t);

int fit_grid_stage(const FitGridHost &h, int stage, const double *in, double *out)
{
    try {
        const int ncol = h.g.ncol;
        const long long nin = stage == 0 ? h.nsamp : ncol;
        Device dv(h, nullptr);
        const ScratchUse<1> use{g_fscratch, nullptr};
        if (int r = device_begin(dv, false, 8 * nin, 0, 0)) return r;
        double *X = dv.at(dv.L.X), *sv = dv.at(dv.L.stageV);
        if (stage == 0) {
            SPLPAK_HIP_TRY(hipMemcpy(sv, in, sizeof(double) * (size_t)nin, hipMemcpyHostToDevice), SPLPAK_E_NODEVICE);
            SPLPAK_HIP_TRY(spread_values<double>(dv, sv, X), SPLPAK_E_NODEVICE);
        } else {
            SPLPAK_HIP_TRY(hipMemcpy(X, in, sizeof(double) * (size_t)nin, hipMemcpyHostToDevice), SPLPAK_E_NODEVICE);
            SPLPAK_HIP_TRY(solve_all(dv, X), SPLPAK_E_NODEVICE);
        }
        SPLPAK_HIP_TRY(hipMemcpy(out, X, sizeof(double) * (size_t)ncol, hipMemcpyDeviceToHost), SPLPAK_E_NODEVICE);
        return 0;
    } catch (const std::bad_alloc &) {
        set_error("the host image of the grid fit's tables could not be allocated");
        return SPLPAK_E_NOMEM;
    }
}

}  // namespace splpak
