// Integrals of the fit over the cells of a tensor grid: out[j0 + n0 (j1 + ...)] = the integral over cell j_d of every
// INTEGRATED dimension (axis: n_d + 1 edges, cell j from e[j] to e[j+1]) at coordinate j_d of every EVALUATED dimension
// (axis: n_d coordinates).  One box, the cell means of a finite-volume mesh and projections (a 3-D fit integrated along z
// onto an x-y image) are all shapes of this call.
//
// What splfe returns is the global sum over all basis products (the window rule never drops a non-zero term), per dimension
// a cubic on every node cell [xmin + k dx, xmin + (k+1) dx] and a straight line below xmin and above xmax.  So a cell is cut
// at the node lines into PIECES, each inside one of the nodes + 1 regions k = -1 .. nodes - 1, and two-point Gauss-Legendre
// on a piece is exact.  A piece is then a table entry of the kind eval_grid_kernel consumes: the window start of its region
// and four factors  sign h (B(m - h/sqrt 3) + B(m + h/sqrt 3)),  m the midpoint and h the half length of the piece:
//
//   piece_count_kernel   one thread per cell of an axis: pieces = k(hi) - k(lo) + 1 (a coordinate of an evaluated axis: 1)
//   piece_scan_kernel    exclusive scan per axis, one workgroup each: first piece of every cell, the total behind the last
//   piece_table_kernel   one thread per piece (per coordinate of an evaluated axis: eval_table<true>, as grid_table_kernel)
//   eval_grid_kernel     (evalgrid.hip, unchanged) the N-D contraction: integrals of all piece products, in double
//   piece_sum_kernel     one launch per integrated dimension, dimension 1 first: [inner][pieces][outer] -> [inner][cells][outer],
//                        one thread per result adds the pieces of its cell in ascending order; the last launch stores T
//
// Summation order (the definition the header gives): every output is the sum over its pieces in ascending piece order,
// dimension 1 innermost, one accumulator per dimension, plain additions.  It does not depend on the slabs.
//
// Bytes by construction: the piece products 8 prod P_d written and read once, 8 prod_{e <= d} n_e prod_{e > d} P_e after the
// reduction of dimension d (written, and read by the next), sizeof(T) per output, the coefficient boxes and the tables
// (36 bytes per piece).  The intermediate (piece products + the first reduction's result) is capped by the option
// integrate_scratch_mb; larger calls go in slabs of consecutive cells of the last dimension.
#include "evalgrid.hpp"
#include "pieces.hpp"

#include <algorithm>
#include <new>
#include <vector>

namespace splpak {

struct IntShape {
    long long ncell[MAXD];     // outputs per dimension (1 beyond ndim)
    long long aoff[MAXD];      // first axis entry of every dimension (ncell + 1 edges or ncell coordinates)
    long long soff[MAXD];      // first entry of every dimension in the piece starts (ncell + 1 each)
    int mode[MAXD];            // 1: integrated, 0: evaluated
};

// ---- count and scan ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256)
piece_count_kernel(Grid g, IntShape is, long long nst, const T *__restrict__ axes, long long *__restrict__ starts)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nst) return;
    int d = 0;
    for (int e = 1; e < g.ndim; ++e) d = i >= is.soff[e] ? e : d;
    const long long j = i - is.soff[d];
    long long n = 0;                                       // the entry behind the last cell: the scan leaves the total there
    if (j < is.ncell[d]) {
        n = 1;
        if (is.mode[d]) {
            const double e0 = (double)axes[is.aoff[d] + j], e1 = (double)axes[is.aoff[d] + j + 1];      // REAL32: widened first
            const bool fwd = e0 <= e1;
            const int klo = piece_region(g, d, fwd ? e0 : e1), khi = piece_region(g, d, fwd ? e1 : e0);
            n = khi > klo ? khi - klo + 1 : 1;             // (a NaN edge: one piece)
        }
    }
    starts[i] = n;
}

__global__ void __launch_bounds__(1024)
piece_scan_kernel(IntShape is, long long *__restrict__ starts)
{
    __shared__ long long wsum[16];
    const int d = blockIdx.x;
    long long *s = starts + is.soff[d];
    const long long n = is.ncell[d] + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;
    for (long long base = 0; base < n; base += 1024) {
        const long long i = base + threadIdx.x;
        const long long v = i < n ? s[i] : 0;
        long long inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        long long before = 0, total = 0;
        for (int w = 0; w < 16; ++w) {
            const long long t = wsum[w];
            before += w < wave ? t : 0;
            total += t;
        }
        if (i < n) s[i] = carry + before + inc - v;
        carry += total;
        __syncthreads();
    }
}

// ---- piece table ---------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256)
piece_table_kernel(Grid g, IntShape is, GridShape gs, const T *__restrict__ axes, const long long *__restrict__ starts,
                   double *__restrict__ fac, int *__restrict__ wst)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    // (no early return: eval_table<true> votes over the wave)
    const bool live = i < gs.off[g.ndim];
    int d = 0;
    for (int e = 1; e < g.ndim; ++e) d = (live && i >= gs.off[e]) ? e : d;
    const long long p = live ? i - gs.off[d] : 0;
    const bool point = live && is.mode[d] == 0;
    // Threads of integrated axes take part in the vote with a dummy coordinate (any finite one does: xmin of dimension 1
    // against dimension d's grid); piece_factors below overwrites what they get.
    const double x = point ? (double)axes[is.aoff[d] + p] : g.xmin[0];
    double b[4];
    int ws = eval_table<true>(g, d, x, 0, b);
    if (live && !point) {
        const long long *s = starts + is.soff[d];
        long long ja = 0, jb = is.ncell[d] - 1;            // the cell of piece p: the last j with s[j] <= p
        while (ja < jb) {
            const long long mid = (ja + jb + 1) >> 1;
            if (s[mid] <= p) ja = mid;
            else jb = mid - 1;
        }
        const long long q = p - s[ja], n = s[ja + 1] - s[ja];
        const T *e = axes + is.aoff[d] + ja;
        ws = piece_factors(g, d, (double)e[0], (double)e[1], (int)q, (int)n, b);
    }
    if (live) {
        wst[i] = ws;
#pragma unroll
        for (int k = 0; k < 4; ++k) fac[4 * i + k] = b[k];
    }
}

// ---- sum of the pieces of one dimension ----------------------------------------------------------------------------
// in[i + inner (p + np o)], p = pieces of this launch -> out[i + inner (j + ncell o)]: cell j owns the pieces s[j] - pbase ..
// s[j+1] - pbase.  Lanes run along `inner` (dimension 1 itself: along the cells).
template <typename TO>
__global__ void __launch_bounds__(256)
piece_sum_kernel(const double *__restrict__ in, TO *__restrict__ out, const long long *__restrict__ s, long long pbase,
                 long long inner, long long ncell, long long np, long long total)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long long i = t % inner, j = (t / inner) % ncell, o = t / (inner * ncell);
    const long long p0 = s[j] - pbase, p1 = s[j + 1] - pbase;
    const double *v = in + i + inner * (np * o);
    double acc = 0.0;
    for (long long p = p0; p < p1; ++p) acc += v[inner * p];
    out[t] = (TO)acc;
}

// ---- host side -----------------------------------------------------------------------------------------------------
static thread_local long long t_stats[8];

void integrate_grid_stats(long long out8[8])
{
    for (int k = 0; k < 8; ++k) out8[k] = t_stats[k];
}

template <typename TO>
static hipError_t launch_piece_sum(const double *in, TO *out, const long long *s, long long pbase, long long inner, long long ncell,
                                   long long np, long long outer, hipStream_t st)
{
    const long long total = inner * ncell * outer, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((piece_sum_kernel<TO>), dim3((unsigned)blocks), dim3(256), 0, st, in, out, s, pbase, inner, ncell, np, total);
    return hipGetLastError();
}

template <typename T>
static hipError_t integrate_grid_run(const Grid &g, const int64_t *ncell, const int *mode, const T *axes, const T *coef, T *out, hipStream_t st)
{
    const int D = g.ndim, L = D - 1;
    for (int k = 0; k < 8; ++k) t_stats[k] = 0;
    IntShape is;
    long long nax = 0, nst = 0;
    int nint = 0, first = -1;                               // integrated dimensions, the first of them
    for (int d = 0; d < MAXD; ++d) {
        const long long n = d < D ? ncell[d] : 1;
        if (n <= 0) return hipSuccess;
        is.ncell[d] = n;
        is.mode[d] = d < D ? (mode ? mode[d] : 1) : 0;
        is.aoff[d] = nax;
        is.soff[d] = nst;
        if (d < D) {
            nax += n + is.mode[d];
            nst += n + 1;
            if (is.mode[d] && first < 0) first = d;
            nint += is.mode[d];
        }
    }
    if (nint == 0) {                                        // values only: straight to out in T, the bits of the grid entries
        t_stats[0] = 1;
        for (int d = 0; d < D; ++d) t_stats[2 + d] = is.ncell[d];
        return launch_eval_grid<T>(g, ncell, axes, nullptr, coef, out, st);
    }
    DevScratch<1> &s = eval_grid_scratch();
    int dev = 0;
    (void)hipGetDevice(&dev);
    // scratch: tile counters | piece starts | factors | intermediate A | B | window starts
    const size_t need1[1] = {(size_t)(16 + 8 * nst)};
    if (hipError_t e = s.ensure(dev, need1, /*may_release_plan=*/true); e != hipSuccess) return e;
    if (hipError_t e = s.wait_on(st); e != hipSuccess) return e;
    const ScratchUse<1> use{s, st};
    auto count_pass = [&]() {
        long long *starts = reinterpret_cast<long long *>(s.as<unsigned long long>(0) + 2);
        hipLaunchKernelGGL((piece_count_kernel<T>), dim3((unsigned)((nst + 255) / 256)), dim3(256), 0, st, g, is, nst, axes, starts);
        hipLaunchKernelGGL(piece_scan_kernel, dim3((unsigned)D), dim3(1024), 0, st, is, starts);
        return hipGetLastError();
    };
    if (nst > 0x7fffffffLL * 256) return hipErrorInvalidValue;
    if (hipError_t e = count_pass(); e != hipSuccess) return e;
    std::vector<long long> hs((size_t)nst);
    if (hipError_t e = hipMemcpyAsync(hs.data(), s.as<unsigned long long>(0) + 2, 8 * (size_t)nst, hipMemcpyDeviceToHost, st); e != hipSuccess) return e;
    if (hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return e;      // the one wait: the piece counts size the launches

    long long P[MAXD] = {1, 1, 1, 1};                       // pieces per dimension (every cell has at least one)
    for (int d = 0; d < D; ++d) {
        P[d] = hs[(size_t)(is.soff[d] + is.ncell[d])];
        t_stats[2 + d] = P[d];
    }
    GridShape full;
    if (!grid_shape(D, P, full)) return hipErrorInvalidValue;      // (a scan that lost its counts: P >= ncell >= 1)
    const long long ntab = full.off[MAXD];
    // doubles per piece of the last dimension: the piece products (A) and, with two or more integrated dimensions, the result
    // of the first reduction (B); later results fit the buffer two steps back
    long long rowA = 1, rowB = 0, row_out = 1;
    bool big = false;
    for (int d = 0; d < L; ++d) {
        big = big || __builtin_mul_overflow(rowA, P[d], &rowA);
        row_out *= is.ncell[d];                             // (the product of all ncell fits int64: the entry checked it)
    }
    if (!big && nint >= 2) rowB = rowA / P[first] * is.ncell[first];
    long long row = 0;
    big = big || __builtin_add_overflow(rowA, rowB, &row) || row > (1LL << 59);
    if (big) return hipErrorOutOfMemory;
    const long long cap = option_ll("SPLPAK_INTEGRATE_SCRATCH_MB", 256, 1, 1LL << 40) * (1LL << 17);      // 2^20 / 8
    long long qmax = 0;                                     // pieces of the last dimension per slab
    if (!eval_grid_slab(D, P, row, cap, qmax)) return hipErrorOutOfMemory;
    // slabs of consecutive cells of the last dimension; a single cell above the cap goes whole
    const long long *SL = hs.data() + is.soff[L];
    const long long nl = is.ncell[L];
    std::vector<long long> cut{0};
    long long qbig = 0;
    while (cut.back() < nl) {
        const long long c0 = cut.back();
        long long c1 = (std::upper_bound(SL + c0, SL + nl + 1, SL[c0] + qmax) - SL) - 1;      // the last c1 with SL[c1] - SL[c0] <= qmax
        c1 = c1 > c0 ? c1 : c0 + 1;
        qbig = std::max(qbig, SL[c1] - SL[c0]);
        cut.push_back(c1);
    }
    long long na = 0, nb = 0, words = 0;
    if (__builtin_mul_overflow(rowA, qbig, &na) || __builtin_mul_overflow(rowB, qbig, &nb) || na > (1LL << 59) || nb > (1LL << 59) ||
        ntab > (1LL << 55))
        return hipErrorOutOfMemory;
    long long qfit = 0;                                     // a single cell above the cap: does its slab still fit a launch?
    if (!eval_grid_slab(D, P, 1, qbig, qfit) || qfit < qbig) return hipErrorInvalidValue;
    words = 2 + nst + 4 * ntab + na + nb + (ntab + 1) / 2;
    const size_t need2[1] = {(size_t)words * 8};
    const bool regrow = need2[0] > s.bytes[0];
    if (hipError_t e = s.ensure(dev, need2, /*may_release_plan=*/true); e != hipSuccess) return hipErrorOutOfMemory;
    if (regrow) {                                           // the new buffer has no piece starts yet: the same pass again
        if (hipError_t e = count_pass(); e != hipSuccess) return e;
    }
    unsigned long long *stats = s.as<unsigned long long>(0);
    long long *starts = reinterpret_cast<long long *>(stats + 2);
    double *fac = reinterpret_cast<double *>(starts + nst);
    double *A = fac + 4 * ntab, *B = A + na;
    int *wst = reinterpret_cast<int *>(B + nb);
    if (hipError_t e = hipMemsetAsync(stats, 0, 16, st); e != hipSuccess) return e;
    if ((ntab + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((piece_table_kernel<T>), dim3((unsigned)((ntab + 255) / 256)), dim3(256), 0, st, g, is, full, axes, starts, fac, wst);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    t_stats[0] = (long long)cut.size() - 1;
    t_stats[1] = na + nb;
    for (size_t k = 0; k + 1 < cut.size(); ++k) {
        const long long c0 = cut[k], c1 = cut[k + 1];
        GridShape gs = full;
        gs.npts[L] = SL[c1] - SL[c0];
        gs.off[L] = full.off[L] + SL[c0];
        if (hipError_t e = launch_eval_grid_tables<T, double>(g, gs, fac, wst, coef, A, stats, st); e != hipSuccess) return e;
        long long dims[MAXD];
        for (int d = 0; d < MAXD; ++d) dims[d] = gs.npts[d];
        const double *cur = A;
        int left = nint;
        for (int d = 0; d < D; ++d) {
            if (!is.mode[d]) continue;
            long long inner = 1, outer = 1;
            for (int e = 0; e < d; ++e) inner *= dims[e];
            for (int e = d + 1; e < D; ++e) outer *= dims[e];
            const long long nc = d == L ? c1 - c0 : is.ncell[d];
            const long long *sd = starts + is.soff[d] + (d == L ? c0 : 0);
            const long long pbase = d == L ? SL[c0] : 0;
            hipError_t e;
            if (--left == 0) {
                e = launch_piece_sum<T>(cur, out + c0 * row_out, sd, pbase, inner, nc, dims[d], outer, st);
            } else {
                double *dst = cur == A ? B : A;
                e = launch_piece_sum<double>(cur, dst, sd, pbase, inner, nc, dims[d], outer, st);
                cur = dst;
            }
            if (e != hipSuccess) return e;
            dims[d] = nc;
            ++t_stats[6];
        }
    }
    return hipSuccess;
}

// the host lists (piece starts, slab cuts) are sized by the caller's ncell: a failed allocation must not unwind through the C entries
template <typename T>
hipError_t launch_integrate_grid(const Grid &g, const int64_t *ncell, const int *mode, const T *axes, const T *coef, T *out, hipStream_t st)
{
    try {
        return integrate_grid_run<T>(g, ncell, mode, axes, coef, out, st);
    } catch (const std::bad_alloc &) {
        return hipErrorOutOfMemory;
    }
}
template hipError_t launch_integrate_grid<double>(const Grid &, const int64_t *, const int *, const double *, const double *, double *, hipStream_t);
template hipError_t launch_integrate_grid<float>(const Grid &, const int64_t *, const int *, const float *, const float *, float *, hipStream_t);

}  // namespace splpak
