// Refinement residual and backward error, from the rows (not from the assembled normal equations).
//
//   rho = A^T W (W y - W A x) - C^T C x for iterative refinement, with the owner-gathers structure of the assembly
//   (gram.hip, constraints.hip): data rows splcw :788-855, constraint rows :921-1046.
//
// No floating-point atomics: every sum has ONE owner and a fixed order, so every refinement residual is bitwise
// reproducible from run to run.  (The backward error ends in an atomic maximum, which no order changes.)
//
// launch_residual, in launch order:
//   residual_wave_kernel (1-D .. 3-D), residual_cell4_kernel (4-D)
//                          per-cell share of A^T W (W y - W A x)
//   constraint_dots_kernel t = C x on the data-sparse nodes (with constraints)
//   rho_gather_kernel      per node: the shares of the cells that contain it, minus C^T t
//   sum_fixed_kernel       the sum of squared row residuals, when asked for (sums.hip)
// 3-D plans run the data rows tile by tile instead (rows3tile.hip), 4-D plans the whole pass (rowsop.hip): for them this form stays
// behind SPLPAK_ROWS_TILES=0 / SPLPAK_RESIDUAL_CELLS=1.
// Backward error:
//   backward_denominators_kernel, backward_error_kernel
#include "assemble_dev.hpp"

namespace splpak {

namespace {

// column of local basis index c (base-4 digits, dim 0 fastest) in a window whose
// first node has column `colbase`
template <int D>
__device__ inline int local_col(const Grid &g, int colbase, int c)
{
    int col = colbase;
#pragma unroll
    for (int d = 0; d < D; ++d) col += ((c >> (2 * d)) & 3) * g.colstride[d];
    return col;
}

// per-cell share of rho = A^T W (W y - W A x): rcell[cell][c] (plain stores; empty cells are skipped by the gather).
// 1-D .. 3-D grids (NB = 4^D <= 64): ONE WAVE per cell, four cells per workgroup, no workgroup barriers (round 3: the
// workgroup-per-cell form of rounds 1-2 spent 1.67 ms per pass at C3 -- 227 000 workgroups of 256 threads for 44 points
// each, staged through five __syncthreads -- for 0.4 GB of points; four passes per fit).
//   phase 1  lane = point:  the D window tables (parked in the wave's LDS slice), t = (w b) . x against the cell's 4^D
//            coefficients (LDS broadcast reads), e = w y - t
//   phase 2  lane = (window function c, point group):  racc_c += (w b)_c * e  over the points
// Sums in a fixed order: reproducible bits.
template <int D>
__global__ void __launch_bounds__(256)
residual_wave_kernel(Grid g, const int *__restrict__ offset, const double *__restrict__ xs,
                     const double *__restrict__ ys, const double *__restrict__ ws, long long cap,
                     const double *__restrict__ xvec, double *__restrict__ rcell, double *__restrict__ ssq)
{
    static_assert(D >= 1 && D <= 3, "one lane per window function");
    constexpr int NB = 1 << (2 * D), G = 64 / NB, PCH = 64, LDT = 4 * D + 1;
    __shared__ double s_tab[4][PCH * LDT];
    __shared__ double s_we[4][PCH];
    __shared__ double s_wt[4][PCH];
    __shared__ double s_x[4][NB];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int cell = blockIdx.x * 4 + wave;
    if (cell >= g.ncell) return;
    const long long beg = offset[cell], end = offset[cell + 1];
    if (beg == end) return;
    double *tab = s_tab[wave], *we = s_we[wave], *sw = s_wt[wave], *xl = s_x[wave];
    int colbase = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) colbase += ((cell / g.cellstride[d]) % g.cells[d]) * g.colstride[d];
    if (lane < NB) xl[lane] = xvec[local_col<D>(g, colbase, lane)];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int c = lane % NB, grp = lane / NB;
    double racc = 0.0, e2 = 0.0;
    for (long long p0 = beg; p0 < end; p0 += PCH) {
        const int np = (int)((end - p0 < PCH) ? (end - p0) : PCH);
        if (lane < np) {
            double b[D][4];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                window_table_value(g, d, xs[(long long)d * cap + p0 + lane], b[d]);
#pragma unroll
                for (int k = 0; k < 4; ++k) tab[lane * LDT + 4 * d + k] = b[d][k];
            }
            // t = (w b) . x with the row entries rounded exactly as the Gram kernel rounds them, ((w b0) b1) b2: the
            // refinement iterates with the operator whose Gram matrix was factored.  (Measured at C3: the contraction
            // factor is the same 2.2e-4 with the factorised window sum -- it is set by the Gram sums and the
            // factorisation, not by the rounding of the row entries; the consistent form costs nothing measurable.)
            const double wv = ws[p0 + lane];
            double t = 0.0;
            if constexpr (D == 1) {
#pragma unroll
                for (int k0 = 0; k0 < 4; ++k0) t = fma(wv * b[0][k0], xl[k0], t);
            } else {
                double u[4][4];
#pragma unroll
                for (int k1 = 0; k1 < 4; ++k1)
#pragma unroll
                    for (int k0 = 0; k0 < 4; ++k0) u[k1][k0] = (wv * b[0][k0]) * b[1][k1];
                if constexpr (D == 2) {
#pragma unroll
                    for (int k1 = 0; k1 < 4; ++k1)
#pragma unroll
                        for (int k0 = 0; k0 < 4; ++k0) t = fma(u[k1][k0], xl[k0 + 4 * k1], t);
                } else {
#pragma unroll
                    for (int k2 = 0; k2 < 4; ++k2)
#pragma unroll
                        for (int k1 = 0; k1 < 4; ++k1)
#pragma unroll
                            for (int k0 = 0; k0 < 4; ++k0) t = fma(u[k1][k0] * b[2][k2], xl[k0 + 4 * k1 + 16 * k2], t);
                }
            }
            const double e = (ys ? wv * ys[p0 + lane] : 0.0) - t; // row residual  w y - (w b) . x  (ys == NULL: -(w b) . x, the rows as an operator)
            we[lane] = e;
            sw[lane] = wv;
            e2 = fma(e, e, e2);
        } else {                                                  // zero rows pad the last group of the loop below
#pragma unroll
            for (int k = 0; k < 4 * D; ++k) tab[lane * LDT + k] = 0.0;
            we[lane] = 0.0;
            sw[lane] = 0.0;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // four points per trip, their LDS words asked for together (one point per trip waited out the LDS latency for each:
        // 5 us of a wave's time per cell at C3, as in the Gram kernel's right-hand side before round 5); the padding rows
        // add +0.0, the order of the sum is the points' order as before
        const int ntrip = (np + 4 * G - 1) / (4 * G);
        for (int it = 0; it < ntrip; ++it) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p = grp + G * (4 * it + k);
                double prod = sw[p] * tab[p * LDT + (c & 3)];
#pragma unroll
                for (int d = 1; d < D; ++d) prod *= tab[p * LDT + 4 * d + ((c >> (2 * d)) & 3)];
                racc = fma(prod, we[p], racc);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int o = NB; o < 64; o <<= 1) racc += __shfl_xor(racc, o, 64);
    if (lane < NB) rcell[(long long)cell * NB + lane] = racc;
    if (ssq) {
        e2 = wave_sum(e2);
        if (lane == 0) ssq[cell] = e2;
    }
}

// The 4-D form of the same share (256 window functions), one workgroup of four waves per cell (round 3: the staged form of
// rounds 1-2, which built the full 16 x 256 row image of a chunk in LDS, took 7.5 ms per pass at 16^4 / 10^7 points):
//   phase 1  wave k3, lane = point: b3[k3] * (factorised window sum of the slab k3 of the cell's coefficients) -> 4 partials
//   phase 2  thread = window function: racc_c += (w b)_c * e over the points
template <int D>
__global__ void __launch_bounds__(256)
residual_cell4_kernel(Grid g, const int *__restrict__ offset, const double *__restrict__ xs,
                      const double *__restrict__ ys, const double *__restrict__ ws, long long cap,
                      const double *__restrict__ xvec, double *__restrict__ rcell, double *__restrict__ ssq)
{
    static_assert(D == 4, "256 window functions");
    constexpr int NB = 256, PCH = 64, LDT = 4 * D + 1;
    __shared__ double tab[PCH * LDT];
    __shared__ double sw[PCH], sy[PCH], se[PCH];
    __shared__ double part[4][PCH];
    __shared__ double xl[NB];
    const int cell = blockIdx.x;
    const long long beg = offset[cell], end = offset[cell + 1];
    if (beg == end) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int colbase = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) colbase += ((cell / g.cellstride[d]) % g.cells[d]) * g.colstride[d];
    xl[tid] = xvec[local_col<D>(g, colbase, tid)];
    double racc = 0.0, e2 = 0.0;
    for (long long p0 = beg; p0 < end; p0 += PCH) {
        const int np = (int)((end - p0 < PCH) ? (end - p0) : PCH);
        if (tid < np) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                double b[4];
                window_table_value(g, d, xs[(long long)d * cap + p0 + tid], b);
#pragma unroll
                for (int k = 0; k < 4; ++k) tab[tid * LDT + 4 * d + k] = b[k];
            }
            sw[tid] = ws[p0 + tid];
            sy[tid] = ys ? ys[p0 + tid] : 0.0;      // (ys == NULL: the rows as an operator, rho = -N x: pcg.hip)
        }
        __syncthreads();
        if (lane < np) {                        // slab k3 = wave of the window sum of point `lane`
            const double *__restrict__ tb = tab + lane * LDT;
            double r3 = 0.0;
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2) {
                double r2 = 0.0;
#pragma unroll
                for (int k1 = 0; k1 < 4; ++k1) {
                    double r = 0.0;
#pragma unroll
                    for (int k0 = 0; k0 < 4; ++k0) r = fma(tb[k0], xl[k0 + 4 * k1 + 16 * k2 + 64 * wave], r);
                    r2 = fma(tb[4 + k1], r, r2);
                }
                r3 = fma(tb[8 + k2], r2, r3);
            }
            part[wave][lane] = tb[12 + wave] * r3;
        }
        __syncthreads();
        if (tid < np) {
            const double t = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
            const double e = sw[tid] * sy[tid] - sw[tid] * t;      // row residual  w y - (w b) . x
            se[tid] = e;
            e2 = fma(e, e, e2);
        }
        __syncthreads();
        for (int p = 0; p < np; ++p) {
            const double *__restrict__ tb = tab + p * LDT;
            const double prod = (((sw[p] * tb[tid & 3]) * tb[4 + ((tid >> 2) & 3)]) * tb[8 + ((tid >> 4) & 3)]) * tb[12 + (tid >> 6)];
            racc = fma(prod, se[p], racc);
        }
        __syncthreads();
    }
    rcell[(long long)cell * NB + tid] = racc;
    if (ssq && wave == 0) {
        e2 = wave_sum(e2);
        if (lane == 0) ssq[cell] = e2;
    }
}

// residual mode, step 1: t[n][pair] = row(n, pair) . x for every sparse node (0 otherwise); one wave per node
template <int D>
__global__ void __launch_bounds__(256)
constraint_dots_kernel(Grid g, const double *__restrict__ dcw, const unsigned char *__restrict__ spf, const double *__restrict__ ctab,
                       const double *__restrict__ xvec, double *__restrict__ tbuf, double *__restrict__ ssq)
{
    constexpr int NE = (D == 1) ? 3 : (D == 2) ? 9 : (D == 3) ? 27 : 81;
    constexpr int NP = D * (D + 1) / 2;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int node = blockIdx.x * 4 + wave;
    if (node >= g.ncol) return;
    int nn[D];
#pragma unroll
    for (int d = 0; d < D; ++d) nn[d] = (node / g.colstride[d]) % g.nodes[d];
    SparseNode sn;
    sn.sparse = spf[node] != 0;
    sn.dcwght = dcw[node];
    double *__restrict__ out = tbuf + (long long)node * NP;
    if (!sn.sparse) {
        if (lane < NP) out[lane] = 0.0;
        return;
    }
    int pair = 0;
    double e2 = 0.0;
    for (int idm = 0; idm < D; ++idm)
        for (int jdm = idm; jdm < D; ++jdm, ++pair) {
            int nder[D];
            const double rowwt = constraint_pattern<D>(g, nn, idm, jdm, sn.dcwght, nder);
            double t = 0.0;
            for (int je = lane; je < NE; je += 64) {
                int offj[D], tt = je, col = 0;
                bool ok = true;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    offj[d] = tt % 3 - 1;
                    tt /= 3;
                    const int ib = nn[d] + offj[d];
                    ok = ok && ib >= 0 && ib <= g.nodes[d] - 1;
                    col += ib * g.colstride[d];
                }
                if (ok) t += constraint_entry<D>(g, ctab, nn, offj, nder, rowwt) * xvec[col];
            }
            t = wave_sum(t);
            if (lane == 0) out[pair] = t;
            e2 += t * t;                         // constraint rows have rhs 0
        }
    if (ssq && lane == 0) ssq[node] = e2;      // the node's share of the squared constraint residuals (summed in a fixed order later)
}

// rho[i] = sum over the cells that contain node i of their share (CellRange order)
//          - sum over sparse neighbours n and their rows of row(n,pair)[i] * t[n][pair]   (tbuf != NULL)
template <int D>
__global__ void __launch_bounds__(256)
rho_gather_kernel(Grid g, const int *__restrict__ offset, const double *__restrict__ rcell,
                  const double *__restrict__ dcw, const unsigned char *__restrict__ spf, const double *__restrict__ ctab,
                  const double *__restrict__ tbuf, double *__restrict__ rho)
{
    constexpr int NB = 1 << (2 * D);
    const int node = blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= g.ncol) return;
    int in[D];
#pragma unroll
    for (int d = 0; d < D; ++d) in[d] = (node / g.colstride[d]) % g.nodes[d];
    const CellRange<D> cr(g, in);
    double acc = 0.0;
    for (int e = 0; e < cr.total; ++e) {
        int cell, r;
        cr.get(g, in, e, cell, r);
        if (offset[cell] != offset[cell + 1]) acc += rcell[(long long)cell * NB + r];
    }
    if (tbuf) acc = constraint_term<D>(g, in, dcw, spf, ctab, tbuf, acc);
    rho[node] = acc;
}

// Componentwise backward error of the returned coefficients with respect to the rows:
//   omega = max_i |rho_i| / ((|N| |x|)_i + |r_i|),   rho = A^T W (W y - W A x) - C^T C x  (from the rows),
// N = the assembled normal equations (half stencil, both triangles visited), r = A^T W^2 y.  The
// denominator is the size of the terms whose sum rho_i is (the basis functions are non-negative, so
// |A|^T |A| = N on the data rows): omega is at rounding level exactly when x minimises the
// least-squares functional to working precision, whatever the grading of the constraint weights.
// (Thread per node on purpose: neighbouring threads walk neighbouring rows code by code, so every 128-byte line of nst that
// is fetched serves 16 iterations of the same wave from the L1.  A wave per node with the lanes over the codes -- coalesced
// for the node's own row -- reads every line of the transposed part for ONE entry: 3.0 instead of 1.3 ms at 64^3, round 3.)
// den[i] = (|N| |x|)_i + |rhs_i| from the half stencil: sum over code < centre of |N(i, jl) x_jl| (jl = i + off(code), the entry
// of row i) and |N(ju, i) x_ju| (ju = i - off(code), the entry of row ju at the same code), code ascending.
// A thread per row that walked its 171 codes touched a new 64-byte sector of another row at every step (N(ju, i) of
// consecutive codes lie in consecutive ROWS): 45 M sector fetches, 1.2 ms at 64^3 -- and beside another kernel it starved
// that one.  Here a workgroup owns 256 consecutive rows and stages, for the seven codes of one (o_1, .., o_{D-1}) at a time
// (they differ in the offset along dimension 0 only), the 7-double pieces of its own rows and of the 256 + 6 rows
// i0 - base - 3 .. that hold the transposed entries, and the two windows of x: every fetched sector is used whole.  Same terms
// in the same order per row.
template <int D>
__global__ void __launch_bounds__(256)
backward_denominators_kernel(Grid g, const double *__restrict__ nst, const double *__restrict__ xvec,
                             const double *__restrict__ rhs, double *__restrict__ den)
{
    constexpr int TR = 256, HALO = TR + 6;
    __shared__ double HA[TR * 7], HB[HALO * 7], xa[HALO], xb[HALO];
    const int tid = threadIdx.x;
    const long long i0 = (long long)blockIdx.x * TR;
    const long long i = i0 + tid;
    const bool live = i < g.ncol;
    const int centre = g.hstencil - 1;
    int in[D];
#pragma unroll
    for (int d = 0; d < D; ++d) in[d] = live ? (int)((i / g.colstride[d]) % g.nodes[d]) : 0;
    double s = live ? fabs(nst[i * g.hstencil + centre] * xvec[i]) + fabs(rhs[i]) : 0.0;
    const int ngroups = centre / 7 + 1;
    for (int gi = 0; gi < ngroups; ++gi) {
        const int c0 = 7 * gi, nk = gi + 1 < ngroups ? 7 : centre - c0;      // (the last group: the codes below the centre)
        int oh[D], t = gi;
        long long base = 0;
        oh[0] = 0;
#pragma unroll
        for (int d = 1; d < D; ++d) {
            oh[d] = t % 7 - 3;
            t /= 7;
            base += (long long)oh[d] * g.colstride[d];
        }
        __syncthreads();
        for (int e = tid; e < TR * 7; e += 256) {
            const long long r = i0 + e / 7;
            const int k = e % 7;
            HA[e] = (r < g.ncol && k < nk) ? nst[r * g.hstencil + c0 + k] : 0.0;
        }
        for (int e = tid; e < HALO * 7; e += 256) {
            const long long r = i0 - base - 3 + e / 7;
            const int k = e % 7;
            HB[e] = (r >= 0 && r < g.ncol && k < nk) ? nst[r * g.hstencil + c0 + k] : 0.0;
        }
        for (int e = tid; e < HALO; e += 256) {
            const long long ra = i0 + base - 3 + e, rb = i0 - base - 3 + e;
            xa[e] = (ra >= 0 && ra < g.ncol) ? xvec[ra] : 0.0;
            xb[e] = (rb >= 0 && rb < g.ncol) ? xvec[rb] : 0.0;
        }
        __syncthreads();
        if (!live) continue;
        bool okh_l = true, okh_u = true;                // the higher dimensions' share of the two in-grid tests
#pragma unroll
        for (int d = 1; d < D; ++d) {
            okh_l = okh_l && in[d] + oh[d] >= 0 && in[d] + oh[d] <= g.nodes[d] - 1;
            okh_u = okh_u && in[d] - oh[d] >= 0 && in[d] - oh[d] <= g.nodes[d] - 1;
        }
        for (int k = 0; k < nk; ++k) {
            const int ox = k - 3;
            const bool okl = okh_l && in[0] + ox >= 0 && in[0] + ox <= g.nodes[0] - 1;
            const bool oku = okh_u && in[0] - ox >= 0 && in[0] - ox <= g.nodes[0] - 1;
            if (okl) s += fabs(HA[tid * 7 + k] * xa[tid + ox + 3]);                     // N(i, jl), jl = i + base + ox < i
            if (oku) s += fabs(HB[(tid - ox + 3) * 7 + k] * xb[tid - ox + 3]);          // N(ju, i), ju = i - base - ox > i
        }
    }
    if (live) den[i] = s;
}

__global__ void __launch_bounds__(256)
backward_error_kernel(int ncol, const double *__restrict__ den, const double *__restrict__ rho, unsigned long long *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double om = 0.0;
    if (i < ncol) {
        const double s = den[i];
        om = s > 0.0 ? fabs(rho[i]) / s : fabs(rho[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) om = fmax(om, __shfl_xor(om, o, 64));
    if ((threadIdx.x & 63) == 0 && om > 0.0) atomicMax(out, (unsigned long long)__double_as_longlong(om));
}

}  // namespace


template <int D>
static void residual_cells(const Grid &g, const SortScratch &s, const double *xvec, double *rcell, double *e2c, hipStream_t st)
{
    if constexpr (D <= 3) {
        hipLaunchKernelGGL(residual_wave_kernel<D>, dim3((unsigned)((g.ncell + 3) / 4)), dim3(256), 0, st, g,
                           s.offset, s.xs, s.ys, s.ws, s.cap, xvec, rcell, e2c);
    } else {
        hipLaunchKernelGGL(residual_cell4_kernel<D>, dim3((unsigned)g.ncell), dim3(256), 0, st, g,
                           s.offset, s.xs, s.ys, s.ws, s.cap, xvec, rcell, e2c);
    }
}

hipError_t launch_residual(const Grid &g, const SortScratch &s, const double *xvec, double *rcell,
                           const double *dcw, const unsigned char *spf, const double *ctab, bool constraints,
                           double *tbuf, double *rho, double *ssq, double *e2buf, hipStream_t st)
{
    dim3 gn((unsigned)((g.ncol + 3) / 4)), bl(256);
    // sum of squared row residuals (ssq != NULL): every cell and every data-sparse node leaves its share in e2buf
    // ([ncell] + [ncol]), one workgroup adds them in a fixed order -- no floating-point atomics, reproducible bits
    double *e2c = (ssq && e2buf) ? e2buf : nullptr, *e2n = e2c ? e2buf + g.ncell : nullptr;
    if (e2c) {
        hipError_t e = hipMemsetAsync(e2buf, 0, sizeof(double) * ((size_t)g.ncell + (size_t)g.ncol), st);
        if (e != hipSuccess) return e;
    }
    DISPATCH_D(g.ndim, {
        residual_cells<D>(g, s, xvec, rcell, e2c, st);
        if (constraints)
            hipLaunchKernelGGL(constraint_dots_kernel<D>, gn, bl, 0, st, g, dcw, spf, ctab, xvec, tbuf, e2n);
        hipLaunchKernelGGL(rho_gather_kernel<D>, dim3((unsigned)((g.ncol + 255) / 256)), bl, 0, st, g,
                           s.offset, rcell, dcw, spf, ctab, constraints ? tbuf : nullptr, rho);
    });
    if (e2c) return launch_sum_fixed(e2buf, (long long)g.ncell + g.ncol, ssq, st);
    return hipGetLastError();
}


hipError_t launch_constraint_dots(const Grid &g, const double *dcw, const unsigned char *spf, const double *ctab, const double *xvec,
                                  double *tbuf, double *e2nodes, hipStream_t st)
{
    dim3 gn((unsigned)((g.ncol + 3) / 4)), bl(256);
    DISPATCH_D(g.ndim, hipLaunchKernelGGL(constraint_dots_kernel<D>, gn, bl, 0, st, g, dcw, spf, ctab, xvec, tbuf, e2nodes));
    return hipGetLastError();
}

hipError_t launch_backward_denominators(const Grid &g, const double *nst, const double *xvec, const double *rhs, double *den, hipStream_t st)
{
    dim3 gr((unsigned)((g.ncol + 255) / 256)), bl(256);           // (256 rows per workgroup: the kernel's tile)
    DISPATCH_D(g.ndim, hipLaunchKernelGGL(backward_denominators_kernel<D>, gr, bl, 0, st, g, nst, xvec, rhs, den));
    return hipGetLastError();
}

hipError_t launch_backward_error(const Grid &g, const double *den, const double *rho, double *out, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(out, 0, sizeof(double), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(backward_error_kernel, dim3((unsigned)((g.ncol + 255) / 256)), dim3(256), 0, st, g.ncol, den, rho,
                       reinterpret_cast<unsigned long long *>(out));
    return hipGetLastError();
}

}  // namespace splpak
