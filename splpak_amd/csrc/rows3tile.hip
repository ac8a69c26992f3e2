// The rows of a 3-D fit applied to a vector, tile by tile: rho = A^T W (W y - W A x) - C^T C x, the pass that the refinement runs
// once per step and the fit once more at its end (with the sum of squared row residuals).  The 3-D form of rowsop.hip's data rows.
//
// The cell-by-cell form (residual.hip: residual_wave_kernel, rho_gather_kernel) runs one wave per cell -- 227 000 waves of ~44 points
// at 64^3 / 1e7 points --, builds every window table with one lane per point, walks the points serially in the transposed product
// with five LDS reads per point and window function, writes a 64-double share per cell (116 MB) and gathers the shares back 8
// bytes at a time from 64 different cells per node: 0.86 + 0.26 ms per pass for 0.4 GB of points
// (profiles/solve_refine_kernel_stats_before.csv).  Here:
//
//   data rows   a workgroup owns a TILE of 3 x 3 x 3 cells: the 6 x 6 x 6 coefficients it touches sit in LDS once, the point ranges
//       of its cells are read once.  Each of its four waves takes every fourth cell (points of a cell in their sorted order, sixteen
//       per trip): lanes = (point, dimension) for the window tables, then both products of the trip on the f64 matrix pipe -- the
//       16 x 4 window of coefficients W[(k1, k2)][k0] times the points' factors b0 in ONE step, and its transpose, the points four
//       per step --, adds the cell's 64 shares into ITS OWN LDS image of the tile's nodes, and the four images are added in a fixed
//       order into the tile's partial sums: 16 MB instead of 116 MB, coalesced, no atomics -- the bits do not depend on the schedule.
//   constraint rows   constraint_dots_kernel of residual.hip, as in the cell-by-cell form (launch_constraint_dots).
//   gather   node i adds the <= 8 tile partials that hold it (tile order, dimension 0 fastest) and subtracts the constraint term
//       (constraint_term, assemble_dev.hpp: the loop of rho_gather_kernel).
//
// Rounding: a row's window sum is taken factor by factor, b1 (sum_k2 b2 (sum_k0 b0 x)), and the residual is weighted afterwards,
// where the cell-by-cell form rounds the row entries as the Gram kernel does, ((w b0) b1) b2: last-bit differences in rho, none
// in the refinement's contraction (the comment in residual_wave_kernel).
#include "assemble_dev.hpp"
#include "plan.hpp"

namespace splpak {

namespace {

#ifndef SPLPAK_TILE3_SHAPE
#define SPLPAK_TILE3_SHAPE 3, 3, 3            // measured at 64^3, 1e7 points (tile kernel + gather, us per pass): 4,4,4 515 + 117; 4,4,2 485 + 119; 3,3,3 329 + 119;
#endif                                       // also 2,2,2 379 + 128; 2,3,3 352 + 121; 3,3,2 341 + 120; 3,3,4 324 + 118; 4,3,3 467 + 118
constexpr int TCS[3] = {SPLPAK_TILE3_SHAPE};                         // cells per tile, by dimension
constexpr int TBS[3] = {TCS[0] + 3, TCS[1] + 3, TCS[2] + 3};          // nodes per tile, by dimension
constexpr int TST[3] = {1, TBS[0], TBS[0] * TBS[1]};                  // strides of the tile's node image
constexpr int TB3 = TBS[0] * TBS[1] * TBS[2];                         // nodes of a tile
constexpr int NCT = TCS[0] * TCS[1] * TCS[2];                         // cells of a tile
constexpr int PCHUNK = 16;               // points per trip of a wave
constexpr int TLD = 13;                  // 12 table values per point + 1 (bank spread)
static_assert(NCT <= 256, "a thread per cell looks up the point ranges");

// partial[tile][TB3]: the tile's share of A^T W (W y - W A x) on its nodes; esq != NULL: esq[tile] = the sum of the squared row
// residuals of the tile's points (the fit's `reserr`), in a fixed order.  ys == NULL: y = 0, the rows as an operator.
__global__ void __launch_bounds__(256)
rows3_tile_kernel(Grid g, int nt0, int nt1, const int *__restrict__ offset, const double *__restrict__ xs,
                  const double *__restrict__ ys, const double *__restrict__ ws, long long cap, const double *__restrict__ xvec,
                  double *__restrict__ partial, double *__restrict__ esq)
{
    __shared__ double pt[TB3];
    __shared__ double acc[4][TB3];
    __shared__ double tab[4][PCHUNK * TLD];
    __shared__ double swe[4][PCHUNK];
    __shared__ int cbeg[NCT], cend[NCT], clb[NCT];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (known to be uniform: the walk over the cells below stays in scalar registers)
    int t = blockIdx.x;
    int cb[3];
    cb[0] = (t % nt0) * TCS[0]; t /= nt0;
    cb[1] = (t % nt1) * TCS[1]; t /= nt1;
    cb[2] = t * TCS[2];
    for (int idx = tid; idx < TB3; idx += 256) {
        int r = idx, col = 0;
        bool ok = true;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int nd = cb[d] + r % TBS[d];
            r /= TBS[d];
            ok = ok && nd < g.nodes[d];
            col += nd * g.colstride[d];
        }
        pt[idx] = ok ? xvec[col] : 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) acc[w][idx] = 0.0;
    }
    // the point ranges of the tile's cells, looked up once (rowsop.hip: asked for cell by cell they were two dependent global
    // round trips per cell that nothing hid)
    if (tid < NCT) {
        int r = tid, cell = 0, lb = 0, mul = 1;
        bool ok = true;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int a = r % TCS[d];
            r /= TCS[d];
            ok = ok && cb[d] + a < g.cells[d];
            cell += (cb[d] + a) * g.cellstride[d];
            lb += a * mul;
            mul *= TBS[d];
        }
        cbeg[tid] = ok ? offset[cell] : 0;
        cend[tid] = ok ? offset[cell + 1] : 0;
        clb[tid] = lb;
    }
    __syncthreads();
    double *__restrict__ mytab = tab[wave];
    double *__restrict__ mywe = swe[wave];
    double *__restrict__ myacc = acc[wave];
    const int pi = lane & 15, sl = lane >> 4;                              // staging: (point, dimension); the fourth quarter of the wave has no dimension
    const int l15 = lane & 15, g4 = lane >> 4;                             // the matrix products' lane coordinates
    const bool hasdim = sl < 3;
    const int sd = hasdim ? sl : 0;
    auto sld = [&](const int *q) { return __builtin_amdgcn_readfirstlane(*q); };
    auto next_cell = [&](int lc) { while (lc < NCT && sld(&cbeg[lc]) == sld(&cend[lc])) lc += 4; return lc; };
    // this lane's dimension of the grid, as dimension 0 of a copy: the table code below then reads registers, not the argument block
    Grid gl = g;
    gl.nodes[0] = g.nodes[sd]; gl.xmin[0] = g.xmin[sd]; gl.dx[0] = g.dx[sd]; gl.dxin[0] = g.dxin[sd];
    // (Measured, not taken up: __launch_bounds__(256, 6) -- 78 registers without the accumulation file, six waves per SIMD instead
    //  of five -- 309 instead of 329 us per pass, 0.06 ms of a 233 ms fit.)
    // the chunk after the current one is loaded while the current one is worked on
    double xpre = 0.0, wpre = 0.0, ypre = 0.0;
    auto issue = [&](int lc, int p0) {
        if (lc >= NCT) return;
        if (hasdim && p0 + pi < sld(&cend[lc])) {
            xpre = xs[(long long)sd * cap + p0 + pi];
            if (sl == 0) {
                wpre = ws[p0 + pi];
                ypre = ys ? ys[p0 + pi] : 0.0;
            }
        }
    };
    int lc = next_cell(wave);
    int p0 = lc < NCT ? sld(&cbeg[lc]) : 0;
    issue(lc, p0);
    d4_t racc = {0.0, 0.0, 0.0, 0.0};
    double esum = 0.0;
    double cw = 0.0;
    bool cell_new = true;
    while (lc < NCT) {
        const int end = sld(&cend[lc]), lbase = sld(&clb[lc]);
        const int np = end - p0 < PCHUNK ? end - p0 : PCHUNK;
        const double xcur = xpre, wcur = wpre, ycur = ypre;
        int lcn = lc, p0n = p0 + PCHUNK;
        if (p0n >= end) {
            lcn = next_cell(lc + 4);
            p0n = lcn < NCT ? sld(&cbeg[lcn]) : 0;
        }
        issue(lcn, p0n);
        if (hasdim) {   // window tables: lane = (point pi, dimension sl); zero rows pad the trip
            double b[4] = {0.0, 0.0, 0.0, 0.0};
            int form;
            if (pi < np) window_table_selected(gl, 0, xcur, b, form);      // (the closed forms of the evaluation kernels, as in rowsop.hip)
#pragma unroll
            for (int k = 0; k < 4; ++k) mytab[pi * TLD + 4 * sl + k] = b[k];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // Both products of a trip on the matrix pipe (v_mfma_f64_16x16x4_f64: A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col =
        // lane & 15], result rows (lane >> 4) + 4 r in register r), over the cell's window of coefficients as W[m][k0], m = k1 + 4 k2.
        if (cell_new)                     // the window's entry this lane feeds the forward product with: W[m = l15][k0 = g4]
            cw = pt[lbase + g4 + TST[1] * (l15 & 3) + TST[2] * (l15 >> 2)];
        {   // forward: T = W B0, B0[k0][q] = b0 of point q (K = k0: one step), then s_q = sum_k1 b1_q[k1] sum_k2 b2_q[k2] T[k1 + 4 k2][q]
            const double *__restrict__ tb = mytab + l15 * TLD;
            d4_t T = {0.0, 0.0, 0.0, 0.0};
            T = __builtin_amdgcn_mfma_f64_16x16x4f64(cw, tb[g4], T, 0, 0, 0);
            // this lane: rows m = g4 + 4 r of point l15, i.e. k1 = g4, k2 = r
            double r3 = T[0] * tb[8];
            r3 = fma(T[1], tb[9], r3);
            r3 = fma(T[2], tb[10], r3);
            r3 = fma(T[3], tb[11], r3);
            const double part = tb[4 + g4] * r3;
            const double q0 = __shfl(part, l15, 64), q1 = __shfl(part, l15 + 16, 64), q2 = __shfl(part, l15 + 32, 64), q3 = __shfl(part, l15 + 48, 64);
            const double tsum = ((q0 + q1) + q2) + q3;
            if (g4 == 0) {
                double we = 0.0;
                if (l15 < np) {
                    const double e = wcur * ycur - wcur * tsum;      // row residual w y - (w b) . x  (y = 0: the rows as an operator)
                    we = wcur * e;
                    esum = fma(e, e, esum);
                }
                mywe[l15] = we;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        {   // transposed: G[m][k0] += sum_q (we_q b1_q[k1] b2_q[k2]) b0_q[k0]  (K = the points, four per step, in their order); the
            // result's columns k0 = 0 .. 3 are real, the B operand of the others is zero
            const int nsteps = (np + 3) >> 2;
            const double *__restrict__ tq0 = mytab + g4 * TLD;
            const double *__restrict__ we0 = mywe + g4;
            const int ia = 4 + (l15 & 3), ja = 8 + (l15 >> 2), ib = l15 & 3;
            const bool realcol = l15 < 4;
#pragma unroll
            for (int s4 = 0; s4 < PCHUNK / 4; ++s4) {      // (unrolled: the steps' LDS addresses differ by constants)
                if (s4 < nsteps) {
                    const double *__restrict__ tq = tq0 + 4 * s4 * TLD;
                    const double a = (we0[4 * s4] * tq[ia]) * tq[ja];
                    const double b = realcol ? tq[ib] : 0.0;
                    racc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, racc, 0, 0, 0);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        cell_new = lcn != lc;
        if (cell_new) {                   // the cell is done: its 64 shares (k0 = l15 < 4, k1 = g4, k2 = register) into this wave's image of the tile
            if (l15 < 4) {
                const int li = lbase + l15 + TST[1] * g4;
#pragma unroll
                for (int j = 0; j < 4; ++j) myacc[li + TST[2] * j] += racc[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) racc[j] = 0.0;
        }
        lc = lcn;
        p0 = p0n;
    }
    if (esq) {                            // lanes 0 .. 15 of every wave hold shares: a fixed tree over them, then the waves in order
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) esum += __shfl_down(esum, o, 64);
        if (lane == 0) swe[wave][0] = esum;
    }
    __syncthreads();
    if (esq && tid == 0) esq[blockIdx.x] = ((swe[0][0] + swe[1][0]) + swe[2][0]) + swe[3][0];
    double *__restrict__ out = partial + (long long)blockIdx.x * TB3;
    for (int idx = tid; idx < TB3; idx += 256) out[idx] = ((acc[0][idx] + acc[1][idx]) + acc[2][idx]) + acc[3][idx];
}

// rho[i] = sum of the tile partials that hold node i (tile order, dimension 0 fastest)
//          - sum over sparse neighbours n and their rows of row(n,pair)[i] * t[n][pair]   (tbuf != NULL)
__global__ void __launch_bounds__(256)
rows3_gather_kernel(Grid g, int nt0, int nt1, int nt2, const double *__restrict__ partial, const double *__restrict__ dcw,
                    const unsigned char *__restrict__ spf, const double *__restrict__ ctab, const double *__restrict__ tbuf,
                    double *__restrict__ rho)
{
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= g.ncol) return;
    const int nt[3] = {nt0, nt1, nt2};
    int tlo[3], tcnt[3], in[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        in[d] = (node / g.colstride[d]) % g.nodes[d];
        // tiles t with TCS t <= in <= TCS t + TBS - 1
        int lo = in[d] - (TBS[d] - 1);
        lo = lo <= 0 ? 0 : (lo + TCS[d] - 1) / TCS[d];
        int hi = in[d] / TCS[d];
        if (hi > nt[d] - 1) hi = nt[d] - 1;
        tlo[d] = lo;
        tcnt[d] = hi - lo + 1;
    }
    double acc = 0.0;
    for (int e2 = 0; e2 < tcnt[2]; ++e2)
        for (int e1 = 0; e1 < tcnt[1]; ++e1)
            for (int e0 = 0; e0 < tcnt[0]; ++e0) {
                const int t0 = tlo[0] + e0, t1 = tlo[1] + e1, t2 = tlo[2] + e2;
                const long long tile = ((long long)t2 * nt1 + t1) * nt0 + t0;
                const int li = (in[0] - TCS[0] * t0) + TST[1] * (in[1] - TCS[1] * t1) + TST[2] * (in[2] - TCS[2] * t2);
                acc += partial[tile * TB3 + li];
            }
    if (tbuf) acc = constraint_term<3>(g, in, dcw, spf, ctab, tbuf, acc);
    rho[node] = acc;
}

}  // namespace

// the tiles of a 3-D grid -> doubles of r->partial the passes need
long long rows3_tiles(const Grid &g, Rows3Tiles *r)
{
    r->ntiles = 1;
    for (int d = 0; d < 3; ++d) {
        r->nt[d] = (g.cells[d] + TCS[d] - 1) / TCS[d];
        r->ntiles *= r->nt[d];
    }
    return r->ntiles * TB3;
}

// rho = A^T W (W y - W A x) [- C^T C x]   (rows.ys == NULL: y = 0); tbuf: [ncol][6] scratch of the constraint rows' dot products.
// e2tiles [ntiles], e2nodes [ncol] (both or none): the shares of the sum of squared row residuals, data rows by tile, constraint rows by node
hipError_t rows3_apply(const Grid &g, const Rows3Tiles &r, const SortScratch &rows, const double *xvec, const double *dcw,
                       const unsigned char *spf, const double *ctab, bool constraints, double *tbuf, double *rho, hipStream_t st,
                       double *e2tiles, double *e2nodes)
{
    hipLaunchKernelGGL(rows3_tile_kernel, dim3((unsigned)r.ntiles), dim3(256), 0, st, g, r.nt[0], r.nt[1], (const int *)rows.offset,
                       (const double *)rows.xs, (const double *)rows.ys, (const double *)rows.ws, rows.cap, xvec, r.partial, e2tiles);
    if (constraints) {
        const hipError_t e = launch_constraint_dots(g, dcw, spf, ctab, xvec, tbuf, e2nodes, st);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(rows3_gather_kernel, dim3((unsigned)((g.ncol + 255) / 256)), dim3(256), 0, st, g, r.nt[0], r.nt[1], r.nt[2],
                       (const double *)r.partial, dcw, spf, ctab, constraints ? (const double *)tbuf : (const double *)nullptr, rho);
    return hipGetLastError();
}

// The same pass with the sum of the squared row residuals into ssq[0]: e2buf [ncell + ncol] takes the shares -- tiles first, nodes
// from ncell on -- and one workgroup adds them in a fixed order (as rowsop_residual).
hipError_t rows3_residual(const Grid &g, const Rows3Tiles &r, const SortScratch &rows, const double *xvec, const double *dcw,
                          const unsigned char *spf, const double *ctab, bool constraints, double *tbuf, double *rho, double *ssq,
                          double *e2buf, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(e2buf, 0, sizeof(double) * ((size_t)g.ncell + (size_t)g.ncol), st);
    if (e != hipSuccess) return e;
    e = rows3_apply(g, r, rows, xvec, dcw, spf, ctab, constraints, tbuf, rho, st, e2buf, constraints ? e2buf + g.ncell : nullptr);
    if (e != hipSuccess) return e;
    return launch_sum_fixed(e2buf, (long long)g.ncell + g.ncol, ssq, st);
}

}  // namespace splpak
