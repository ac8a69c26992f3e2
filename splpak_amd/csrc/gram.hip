// Normal equations of the data rows: per-cell Gram blocks, gathered per node.
//
// Every row of the reference's least-squares matrix (splcw :788-855) has its non-zeros inside one 4-wide window of nodes
// per dimension, so with the points binned by window (binpoints.hip)
// every cell contributes ONE dense 4^ndim x 4^ndim Gram block B^T W^2 B to the
// normal equations N = A^T A, r = A^T b, stored as a half stencil
// nst[ncol][(7^ndim+1)/2] (row i, columns i+offset with offset tuple in
// [-3,3]^ndim, lower triangle only).
//
// No floating-point atomics on this path: every sum has ONE owner and a fixed order, so the normal
// equations and the sparse-area histogram are bitwise reproducible from
// run to run, and the assembly runs at streaming rates instead of the rate of
// scattered 8-byte atomics (round 1: 3.8 GB of them at 64^3, 19.8 ms).  The one exception: a point so far outside the grid
// that its histogram address is no node of its window (:899) is added to the histogram with an atomic -- a single add.
//
// Per slab of cells (launch_gram), in launch order:
//   the cell kernel        per cell: the 4^d x 4^d Gram block (packed lower triangle), B^T W^2 y and the
//                          cell's share of the nearest-node histogram (:886-907) are written with
//                          plain stores into a scratch image (the not-yet-used band storage)
//     gram_wave_kernel     2-D and 3-D, the default: one wave per cell on the f64 matrix cores
//     gram_mfma4_kernel    4-D, the default: ten waves per cell on the f64 matrix cores
//     gram_block_kernel    1-D, and every dimension under the A/B route SPLPAK_GRAM_VALU: point tables staged in LDS,
//                          register-tiled rank-1 updates
//   stencil_gather_kernel  one wave per node: sums the <= 4^d blocks that contain the node, in a
//                          fixed order, into its stencil row, right-hand side and histogram entry
// and once at the end
//   hist_total_kernel      totlwt (:906), the sum of the histogram in a fixed order (sums.hip)
// Also here, for the compiler's sake (see the comment above it): constraint_table_kernel, once per plan.
#include "assemble_dev.hpp"

namespace splpak {

namespace {

// nearest-node histogram slot of a point INSIDE its cell's window (local index, dim 0 fastest), or -1
// when the reference's address (:894-902) is not a node of the window: a coordinate so far outside
// the grid that its dimension is skipped in the Horner address (the :899 quirk).  x is in the plan's
// internal dimension order; per dimension the arithmetic is the reference's.
template <int D>
__device__ inline int nearest_slot(const Grid &g, const double *x)
{
#pragma clang fp contract(off)
    int slot = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double t = g.dxin[d] * (x[d] - g.xmin[d]) + 0.5;
        const int inidim = (t >= 2.0e9) ? 2000000000 : (t <= -2.0e9 ? -2000000000 : (int)t);
        if (inidim < 0 || inidim > g.nodes[d] - 1) return -1;
        int lo, hi;
        const int l = inidim - window_start(g, d, x[d], lo, hi);
        if (l < 0 || l > 3) return -1;
        slot += l << (2 * d);
    }
    return slot;
}

// Per-cell staging of gram_block_kernel: for `np` points
// starting at sorted position `p0`, fill bw[p*LDB + c] = w * ((b0*b1)*b2...) --
// the row of the weighted least-squares matrix restricted to the cell's window
// (:833-837) -- and wy[p] = w*y (:806).  hslot != NULL: also the point's histogram slot
// (nearest_slot; points whose address lies outside the window are added to `hist` directly).
template <int D, int NB, int LDB, int NT>
__device__ inline void stage_points(const Grid &g, const double *__restrict__ xs,
                                    const double *__restrict__ ys,
                                    const double *__restrict__ ws, long long cap, long long p0,
                                    int np, double *tab /*[PCH][D][4]*/, double *bw, double *wy,
                                    double *wt, int *hslot, double *__restrict__ hist)
{
    const int tid = threadIdx.x;
    for (int p = tid; p < np; p += NT) {
        const double wv = ws[p0 + p];
        double xv[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            double b[4];
            xv[d] = xs[(long long)d * cap + p0 + p];
            window_table(g, d, xv[d], 0, b);
#pragma unroll
            for (int k = 0; k < 4; ++k) tab[(p * D + d) * 4 + k] = b[k];
        }
        wy[p] = ys ? wv * ys[p0 + p] : 0.0;      // (ys == NULL: the rows applied to a vector, residual pass as operator -- pcg.hip)
        wt[p] = wv;
        if (hslot) {
            const int sl = nearest_slot<D>(g, xv);
            hslot[p] = sl;
            if (sl < 0) {                       // rare: far outside the grid (:899); the only atomic left
                double xr[MAXD] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int d = 0; d < D; ++d) xr[g.perm[d]] = xv[d];
                atomicAdd(&hist[nearest_node_address(g, xr)], wv);       // :905
            }
        }
    }
    __syncthreads();
    for (int idx = tid; idx < np * NB; idx += NT) {
        const int p = idx / NB, c = idx % NB;
        double prod = tab[(p * D + 0) * 4 + (c & 3)];
#pragma unroll
        for (int d = 1; d < D; ++d) prod *= tab[(p * D + d) * 4 + ((c >> (2 * d)) & 3)];
        bw[p * LDB + c] = wt[p] * prod;
    }
    __syncthreads();
}

template <int D>
struct GramCfg;
template <> struct GramCfg<1> { static constexpr int NB = 4,   TR = 1, TC = 1, NTY = 4,  NTX = 4,  NT = 64,   PCH = 64,  WPE = 1; };
template <> struct GramCfg<2> { static constexpr int NB = 16,  TR = 1, TC = 1, NTY = 16, NTX = 16, NT = 256,  PCH = 128, WPE = 1; };
template <> struct GramCfg<3> { static constexpr int NB = 64,  TR = 4, TC = 4, NTY = 16, NTX = 16, NT = 256,  PCH = 64,  WPE = 4; };
template <> struct GramCfg<4> { static constexpr int NB = 256, TR = 4, TC = 4, NTY = 64, NTX = 16, NT = 1024, PCH = 16,  WPE = 1; };

// scratch image of the per-cell blocks: [ncell][TRI] packed lower triangles (row-major: entry (r,c),
// c <= r, at r(r+1)/2 + c), then [ncell][NB] right-hand sides, then [ncell][NB] histogram shares
__host__ __device__ inline long long gram_tri(int nb) { return (long long)nb * (nb + 1) / 2; }

template <int D>
__global__ void __launch_bounds__(GramCfg<D>::NT, GramCfg<D>::WPE)
gram_block_kernel(Grid g, const int *__restrict__ offset, const double *__restrict__ xs,
                  const double *__restrict__ ys, const double *__restrict__ ws, long long cap,
                  double *__restrict__ blk, double *__restrict__ rblk, double *__restrict__ hblk,
                  double *__restrict__ hist, int cell0)
{
    using C = GramCfg<D>;
    constexpr int NB = C::NB, TR = C::TR, TC = C::TC, NT = C::NT, PCH = C::PCH;
    constexpr int CW = C::NTX * TC;            // columns handled by this workgroup
    constexpr long long TRI = (long long)NB * (NB + 1) / 2;
    const int cell = cell0 + blockIdx.x;       // the scratch image holds the cells of one slab, from cell0 on
    const int cpass = blockIdx.y;
    const long long beg = offset[cell], end = offset[cell + 1];
    if (beg == end) return;                    // the gather skips empty cells

    // (the point image doubles as the staging area of the packed triangle on the way out: at least TRI entries when
    // one column pass covers the block)
    constexpr int BWN = (C::NTX * TC >= NB && TRI > (long long)PCH * NB) ? (int)TRI : PCH * NB;
    __shared__ double tab[PCH * D * 4];
    __shared__ double bw[BWN];
    __shared__ double wy[PCH];
    __shared__ double wt[PCH];
    __shared__ int hslot[PCH];

    const int tid = threadIdx.x;
    const int ty = tid / C::NTX, tx = tid % C::NTX;
    const int r0 = ty * TR, c0 = cpass * CW + tx * TC;
    const bool tile_on = (tid < C::NTY * C::NTX) && (r0 + TR - 1 >= c0);
    const bool vec_on = (cpass == 0) && (tid < NB);
    const bool hist_on = hblk != nullptr && cpass == 0;

    double acc[TR][TC];
#pragma unroll
    for (int i = 0; i < TR; ++i)
#pragma unroll
        for (int j = 0; j < TC; ++j) acc[i][j] = 0.0;
    double racc = 0.0, hacc = 0.0;

    for (long long p0 = beg; p0 < end; p0 += PCH) {
        const int np = (int)((end - p0 < PCH) ? (end - p0) : PCH);
        stage_points<D, NB, NB, NT>(g, xs, ys, ws, cap, p0, np, tab, bw, wy, wt, hist_on ? hslot : nullptr, hist);
        if (tile_on) {
            for (int p = 0; p < np; ++p) {
                double a[TR], b[TC];
#pragma unroll
                for (int i = 0; i < TR; ++i) a[i] = bw[p * NB + r0 + i];
#pragma unroll
                for (int j = 0; j < TC; ++j) b[j] = bw[p * NB + c0 + j];
#pragma unroll
                for (int i = 0; i < TR; ++i)
#pragma unroll
                    for (int j = 0; j < TC; ++j) acc[i][j] += a[i] * b[j];
            }
        }
        if (vec_on) {
            for (int p = 0; p < np; ++p) racc += bw[p * NB + tid] * wy[p];
            if (hist_on)
                for (int p = 0; p < np; ++p) hacc += (hslot[p] == tid) ? wt[p] : 0.0;       // :905, in storage order
        }
        __syncthreads();
    }

    double *__restrict__ out = blk + (long long)(cell - cell0) * TRI;
    if constexpr (TRI <= (long long)BWN) {
        // the packed triangle is assembled in LDS (the point image is no longer needed) and leaves with
        // consecutive lanes on consecutive addresses (the 4x4 register tiles written directly put 8 bytes
        // every 32; same kernel time at 64^3 -- the kernel is bound by its per-cell phases, not by the
        // stores -- but a quarter of the write requests)
        if (tile_on) {
#pragma unroll
            for (int i = 0; i < TR; ++i) {
                const int r = r0 + i;
#pragma unroll
                for (int j = 0; j < TC; ++j) {
                    const int c = c0 + j;
                    if (c <= r) bw[r * (r + 1) / 2 + c] = acc[i][j];
                }
            }
        }
        __syncthreads();
        for (int e = tid; e < (int)TRI; e += NT) out[e] = bw[e];
    } else if (tile_on) {
#pragma unroll
        for (int i = 0; i < TR; ++i) {
            const int r = r0 + i;
#pragma unroll
            for (int j = 0; j < TC; ++j) {
                const int c = c0 + j;
                if (c <= r) out[(long long)r * (r + 1) / 2 + c] = acc[i][j];
            }
        }
    }
    if (vec_on) {
        rblk[(long long)(cell - cell0) * NB + tid] = racc;
        if (hist_on) hblk[(long long)(cell - cell0) * NB + tid] = hacc;
    }
}

// The same per-cell blocks for 2-D and 3-D grids (NB = 16 / 64) on the f64 matrix cores, ONE WAVE per cell, no workgroup
// barriers (round 3).  The block is B^T B with B = the cell's weighted rows (points x NB), i.e. a product
// with K = points: per 4 points one v_mfma_f64_16x16x4_f64 per 16 x 16 tile of the lower triangle (10 tiles at NB = 64).
// The operands are never staged: lane (l15, q) of k-step s needs
// B[p = 4 s + q][16 m + l15] = (w_p b0[l15 & 3] b1[l15 >> 2]) * b2[m] -- three table reads from the wave's LDS slice and
// one multiplication per tile block.  The result tiles have consecutive lanes on consecutive entries of a packed row
// (first MFMA operand = the row block), so they leave with plain coalesced stores.  The workgroup-per-cell form above
// read 8 LDS values per 16 FMAs, used 136 of its 256 threads in the triangle and passed five barriers per cell: 3.56 ms
// at C3 for 0.65 ms of matrix-pipe time.
// Round 5 (in-kernel clock stamps per wave, C3: 5.1 us loads + tables, 4.1 us products, 5.1 us right-hand side, 1.5 us stores):
//  - the right-hand side B^T (w^2 y) is summed from the matrix operands the lanes hold anyway (one multiply-add per row
//    block and step, the four lanes of an entry added at the end); as a loop over the points with lane = window function it
//    read five LDS words per point behind the LDS latency and cost as much as the blocks;
//  - the histogram share of a point is one LDS atomic of lane = point onto its nearest node's word of the wave's LDS row (the
//    lanes of one instruction that meet on a word are served one after the other by the LDS unit, the same way every run);
//  - a wave owns a RUN of up to GW_RUN consecutive cells (fewer on a small grid: launch_gram) and loads the points of the next cell before the products of the current
//    one, so that the two dependent round trips (offsets, then points) are paid once per run, not once per cell.
constexpr int GW_RUN = 8;
template <int D>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
gram_wave_kernel(Grid g, const int *__restrict__ offset, const double *__restrict__ xs,
                 const double *__restrict__ ys, const double *__restrict__ ws, long long cap,
                 double *__restrict__ blk, double *__restrict__ rblk, double *__restrict__ hblk,
                 double *__restrict__ hist, int cell0, int ncells, int run)
{
    static_assert(D == 2 || D == 3, "16 or 64 window functions");
    static_assert(GW_RUN + 1 <= 64, "the offsets of a run sit in one register of the wave");
    constexpr int NB = 1 << (2 * D), MT = NB / 16, NTILE = MT * (MT + 1) / 2, PCH = 64, LDT = 4 * D + 1;
    constexpr long long TRI = (long long)NB * (NB + 1) / 2;
    __shared__ double s_tab[4][PCH * LDT];
    __shared__ double s_w[4][PCH];
    __shared__ double s_wy[4][PCH];
    __shared__ double s_hist[4][NB];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, q = lane >> 4;
    const int first = (blockIdx.x * 4 + wave) * run;
    if (first >= ncells) return;
    const int ncl = ncells - first < run ? ncells - first : run;
    double *tab = s_tab[wave], *sw = s_w[wave], *swy = s_wy[wave], *sh = s_hist[wave];
    const bool hist_on = hblk != nullptr;
    const int offv = offset[cell0 + first + (lane <= ncl ? lane : ncl)];
    // the points of a chunk, lane = point (zeros beyond np: zero rows pad the last k-step)
    struct Pts { double x[D], y, w; };
    auto fetch = [&](long long p0, int np) {
        Pts t;
#pragma unroll
        for (int d = 0; d < D; ++d) t.x[d] = 0.0;
        t.y = 0.0;
        t.w = 0.0;
        if (lane < np) {
            t.w = ws[p0 + lane];
#pragma unroll
            for (int d = 0; d < D; ++d) t.x[d] = xs[(long long)d * cap + p0 + lane];
            t.y = ys[p0 + lane];
        }
        return t;
    };
    long long beg = __builtin_amdgcn_readlane(offv, 0), end = __builtin_amdgcn_readlane(offv, 1);
    Pts pre = fetch(beg, (int)(end - beg < PCH ? end - beg : PCH));
    for (int ci = 0; ci < ncl; ++ci) {
        const int rel = first + ci;
        long long nbeg = end, nend = end;
        if (ci + 1 < ncl) nend = __builtin_amdgcn_readlane(offv, ci + 2);
        if (beg == end) {                          // an empty cell leaves a zero block: the gather reads every block unconditionally
            double *__restrict__ z = blk + (long long)rel * TRI;
            for (int e = lane; e < (int)TRI; e += 64) z[e] = 0.0;
            if (lane < NB) {
                rblk[(long long)rel * NB + lane] = 0.0;
                if (hblk) hblk[(long long)rel * NB + lane] = 0.0;
            }
            if (ci + 1 < ncl) pre = fetch(nbeg, (int)(nend - nbeg < PCH ? nend - nbeg : PCH));
            beg = nbeg;
            end = nend;
            continue;
        }
        if (hist_on && lane < NB) sh[lane] = 0.0;
        d4_t acc[NTILE];
        double racc[MT];
#pragma unroll
        for (int t = 0; t < NTILE; ++t) acc[t] = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int m = 0; m < MT; ++m) racc[m] = 0.0;
        for (long long p0 = beg; p0 < end; p0 += PCH) {
            const int np = (int)((end - p0 < PCH) ? (end - p0) : PCH);
            const Pts cur = (p0 == beg) ? pre : fetch(p0, np);
            // ---- lane = point: window tables, weight, w^2 y, histogram share
            {
                double b[D][4];
#pragma unroll
                for (int d = 0; d < D; ++d)
#pragma unroll
                    for (int k = 0; k < 4; ++k) b[d][k] = 0.0;
                if (lane < np) {
#pragma unroll
                    for (int d = 0; d < D; ++d) window_table_value(g, d, cur.x[d], b[d]);   // (the bits of window_table(.., 0, ..), see basis.hpp)
                    if (hist_on) {
                        const int sl = nearest_slot<D>(g, cur.x);
                        if (sl >= 0)
                            __builtin_amdgcn_ds_atomic_fadd_f64((__attribute__((address_space(3))) double *)(sh + sl), cur.w);      // :905
                        else {                              // rare: far outside the grid (:899); the only global atomic left
                            double xr[MAXD] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                            for (int d = 0; d < D; ++d) xr[g.perm[d]] = cur.x[d];
                            atomicAdd(&hist[nearest_node_address(g, xr)], cur.w);       // :905
                        }
                    }
                }
#pragma unroll
                for (int d = 0; d < D; ++d)
#pragma unroll
                    for (int k = 0; k < 4; ++k) tab[lane * LDT + 4 * d + k] = b[d][k];
                sw[lane] = cur.w;
                swy[lane] = cur.w * cur.y;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // the next cell's first chunk is on its way while this one is multiplied
            if (p0 + PCH >= end && ci + 1 < ncl) pre = fetch(nbeg, (int)(nend - nbeg < PCH ? nend - nbeg : PCH));
            // ---- matrix cores: K = the chunk's points, four per step
            const int nsteps = (np + 3) >> 2;
            // (the LDS words of step s + 1 are asked for before the products of step s are issued)
            struct Ops { double w, t0, t1, t2[MT], wy; };
            auto lds_ops = [&](int s4) {
                const int p = 4 * s4 + q;
                Ops o;
                o.w = sw[p];
                o.t0 = tab[p * LDT + (l15 & 3)];
                o.t1 = tab[p * LDT + 4 + (l15 >> 2)];
                if constexpr (D == 3) {
#pragma unroll
                    for (int m = 0; m < MT; ++m) o.t2[m] = tab[p * LDT + 8 + m];
                }
                o.wy = swy[p];
                return o;
            };
            Ops nx = lds_ops(0);
            for (int s4 = 0; s4 < nsteps; ++s4) {
                const Ops o = nx;
                nx = lds_ops(s4 + 1 < nsteps ? s4 + 1 : s4);
                const double u = (o.w * o.t0) * o.t1;
                double op[MT];
                if constexpr (D == 2) op[0] = u;
                else {
#pragma unroll
                    for (int m = 0; m < MT; ++m) op[m] = u * o.t2[m];
                }
                int t = 0;
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int n = m; n < MT; ++n, ++t)
                        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(op[n], op[m], acc[t], 0, 0, 0);
                // right-hand side: this lane's entries B[4 s + q][16 m + l15] times w^2 y of its point, summed over the steps;
                // the four q of an entry meet after the last chunk
#pragma unroll
                for (int m = 0; m < MT; ++m) racc[m] += op[m] * o.wy;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        // packed lower triangle: tile (m, n), register v of lane (l15, q) = entry (r, c) = (16 n + q + 4 v, 16 m + l15)
        double *__restrict__ out = blk + (long long)rel * TRI;
        {
            int t = 0;
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = m; n < MT; ++n, ++t)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int r = 16 * n + q + 4 * v, c = 16 * m + l15;
                        if (c <= r) out[r * (r + 1) / 2 + c] = acc[t][v];
                    }
        }
        // right-hand side: entry 16 m + l15 = the sum over q of the lanes (l15, q) -> through LDS to lane = entry
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            double r = racc[m];
            r += __shfl_xor(r, 16, 64);
            r += __shfl_xor(r, 32, 64);
            if (q == 0) sw[16 * m + l15] = r;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane < NB) {
            rblk[(long long)rel * NB + lane] = sw[lane];
            if (hist_on) hblk[(long long)rel * NB + lane] = sh[lane];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        beg = nbeg;
        end = nend;
    }
}

// The 4-D blocks (256 window functions: 136 tiles of 16 x 16 in the lower triangle) on the matrix cores: one workgroup of TEN
// waves per cell, a wave per 64 x 64 super-block (I, J), J <= I, of the 256 x 256 block -- 16 accumulator tiles with static
// indices, as in the trailing-update kernels (the four diagonal super-blocks compute 6 tiles they do not store: 160 MFMAs per
// 4 points for 136 useful).  Operands as in gram_wave_kernel, with the fourth dimension's factor on top:
// B[p][c] = (((w b0[c0]) b1[c1]) b2[c2]) b3[c3], c = c0 + 4 c1 + 16 c2 + 64 c3: tile block m = (c2, c3) = (m & 3, m >> 2), so a
// super-block (I, J) needs t[j] = u b2[j] once and t[j] b3[I], t[j] b3[J] per step.  Round 3: the workgroup-per-cell VALU form
// took 73.8 ms at 16^4 / 10^7 points (a third of the fit) for ~11 ms of matrix-pipe time.
template <int D>
__global__ void __launch_bounds__(640)
gram_mfma4_kernel(Grid g, const int *__restrict__ offset, const double *__restrict__ xs,
                  const double *__restrict__ ys, const double *__restrict__ ws, long long cap,
                  double *__restrict__ blk, double *__restrict__ rblk, double *__restrict__ hblk,
                  double *__restrict__ hist, int cell0)
{
    static_assert(D == 4, "256 window functions");
    constexpr int NB = 256, PCH = 64, LDT = 4 * D + 1;
    constexpr long long TRI = (long long)NB * (NB + 1) / 2;
    __shared__ double tab[PCH * LDT];
    __shared__ double sw[PCH], swy[PCH];
    __shared__ int sslot[PCH];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, q = lane >> 4;
    const int cell = cell0 + blockIdx.x;
    const long long beg = offset[cell], end = offset[cell + 1];
    if (beg == end) return;                    // the gather skips empty cells
    const bool hist_on = hblk != nullptr;
    // super-block of this wave: (0,0) (1,0) (1,1) (2,0) (2,1) (2,2) (3,0) (3,1) (3,2) (3,3)
    int sbI = 0, sbJ = wave;
    while (sbJ > sbI) { sbJ -= sbI + 1; ++sbI; }

    d4_t acc[4][4];                            // [column tile mi of J][row tile ni of I]
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = d4_t{0.0, 0.0, 0.0, 0.0};
    double racc = 0.0, hacc = 0.0;
    for (long long p0 = beg; p0 < end; p0 += PCH) {
        const int np = (int)((end - p0 < PCH) ? (end - p0) : PCH);
        if (tid < PCH) {                       // lane = point: window tables, weight, w^2 y, histogram slot (zero rows beyond np)
            double b[D][4], wv = 0.0, wyv = 0.0;
            int sl = -2;
#pragma unroll
            for (int d = 0; d < D; ++d)
#pragma unroll
                for (int k = 0; k < 4; ++k) b[d][k] = 0.0;
            if (tid < np) {
                double xv[D];
                wv = ws[p0 + tid];
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    xv[d] = xs[(long long)d * cap + p0 + tid];
                    window_table(g, d, xv[d], 0, b[d]);         // (the value form costs this kernel registers it does not have: +4.7 ms at 16^4)
                }
                wyv = wv * ys[p0 + tid];
                if (hist_on) {
                    sl = nearest_slot<D>(g, xv);
                    if (sl < 0) {                       // rare: far outside the grid (:899); the only atomic left
                        double xr[MAXD] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                        for (int d = 0; d < D; ++d) xr[g.perm[d]] = xv[d];
                        atomicAdd(&hist[nearest_node_address(g, xr)], wv);       // :905
                    }
                }
            }
#pragma unroll
            for (int d = 0; d < D; ++d)
#pragma unroll
                for (int k = 0; k < 4; ++k) tab[tid * LDT + 4 * d + k] = b[d][k];
            sw[tid] = wv;
            swy[tid] = wyv;
            sslot[tid] = sl;
        }
        __syncthreads();
        const int nsteps = (np + 3) >> 2;
        for (int s4 = 0; s4 < nsteps; ++s4) {
            const int p = 4 * s4 + q;
            const double u = (sw[p] * tab[p * LDT + (l15 & 3)]) * tab[p * LDT + 4 + (l15 >> 2)];
            const double bI = tab[p * LDT + 12 + sbI], bJ = tab[p * LDT + 12 + sbJ];
            double orow[4], ocol[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double t = u * tab[p * LDT + 8 + j];
                orow[j] = t * bI;
                ocol[j] = t * bJ;
            }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(orow[ni], ocol[mi], acc[mi][ni], 0, 0, 0);
        }
        // right-hand side and histogram shares: thread = window function, points in storage order
        if (tid < NB) {
            for (int p = 0; p < np; ++p) {
                double prod = tab[p * LDT + (tid & 3)];
#pragma unroll
                for (int d = 1; d < D; ++d) prod *= tab[p * LDT + 4 * d + ((tid >> (2 * d)) & 3)];
                racc += (sw[p] * prod) * swy[p];
                if (hist_on) hacc += (sslot[p] == tid) ? sw[p] : 0.0;       // :905
            }
        }
        __syncthreads();
    }
    // packed lower triangle: tile (m, n) = (4 J + mi, 4 I + ni), register v of lane (l15, q) = entry (r, c) = (16 n + q + 4 v, 16 m + l15)
    double *__restrict__ out = blk + (long long)blockIdx.x * TRI;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int m = 4 * sbJ + mi, n = 4 * sbI + ni;
            if (m > n) continue;               // (above the diagonal of a diagonal super-block)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int r = 16 * n + q + 4 * v, c = 16 * m + l15;
                if (c <= r) out[(long long)r * (r + 1) / 2 + c] = acc[mi][ni][v];
            }
        }
    if (tid < NB) {
        rblk[(long long)blockIdx.x * NB + tid] = racc;
        if (hist_on) hblk[(long long)blockIdx.x * NB + tid] = hacc;
    }
}

// One wave per node i: stencil row nst[i][*], rhs[i] and the node's histogram entry as the sums of
// the per-cell blocks, cell after cell in CellRange order.  Entry (r, c) of a block, c <= r, belongs
// to column offset c - r (digit-wise), i.e. stencil code sum_d (c_d - r_d + 3) 7^d; for one cell the
// lanes c = 0..r hit distinct codes, so the wave accumulates in an LDS row without conflicts.
// ZEROED: the blocks of empty cells were written as zeros (gram_wave_kernel), so no cell's point count is looked up and the
// rows of a batch do not wait for a first round of loads (round 3: two dependent round trips per batch of 8 cells -> one).
template <int D, bool ZEROED = false>
__global__ void __launch_bounds__(256)
stencil_gather_kernel(Grid g, const int *__restrict__ offset, const double *__restrict__ blk,
                      const double *__restrict__ rblk, const double *__restrict__ hblk,
                      double *__restrict__ nst, double *__restrict__ rhs, double *__restrict__ hist,
                      int cell0, int cell1, int node0, int node1)
{
    constexpr int NB = 1 << (2 * D);
    constexpr long long TRI = (long long)NB * (NB + 1) / 2;
    constexpr int HS = (D == 1) ? 4 : (D == 2) ? 25 : (D == 3) ? 172 : 1201;
    __shared__ double sacc[4][HS];
    __shared__ double stmp[4][128];
    // (the wave index as a SCALAR: node, cell walk, row and block addresses below are then scalar arithmetic -- as vector
    //  code with a division per dimension and cell, and seven integer operations per lane for the stencil code, the kernel ran
    //  at the same 10.7 ns per node whether its blocks came from HBM or from the Infinity Cache: issue-bound, round 5)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    // the cells [cell0, cell1) of the current slab (whole hyper-rows of the slowest dimension) touch the
    // nodes [node0, node1); with one slab that is everything.  Sums of successive slabs add up in nst
    // (zero on entry), in slab order: still one owner and a fixed order per entry.
    const int node = node0 + blockIdx.x * 4 + wave;
    if (node >= node1) return;                 // whole waves leave; no workgroup barrier below
    double *acc = sacc[wave];
    for (int e = lane; e < HS; e += 64) acc[e] = 0.0;
    int in[D];
#pragma unroll
    for (int d = 0; d < D; ++d) in[d] = (node / g.colstride[d]) % g.nodes[d];
    const CellRange<D> cr(g, in);
    double racc = 0.0, hacc = 0.0;
    // Cells in batches of GB, three phases per batch so that no load waits for a decision that needs an
    // earlier load of the same batch: (1) the cells' point counts, (2) the block rows of the non-empty ones
    // (predicated, never a branch), (3) the LDS accumulation in cell order.  A cell at a time made every
    // wave wait out two dependent memory round trips per cell (3.4 ms at 64^3).
    constexpr int GB = (D <= 3) ? 8 : 4;
    constexpr int NCH = (NB + 63) / 64;              // 64-column chunks of a block row
    // stencil code of entry (r, c) = K(c) - K(r) + centre with K(v) = sum_d v_d 7^d over the 2-bit digits of v: K(c) once per
    // lane, K(r) with the row
    int kc[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const int c = lane + 64 * ch;
        int k = 0, m7 = 1;
#pragma unroll
        for (int d = 0; d < D; ++d) { k += ((c >> (2 * d)) & 3) * m7; m7 *= 7; }
        kc[ch] = k + (HS - 1);
    }
    if constexpr (D == 3 && ZEROED) {
        // 3-D: the walk as three nested loops with the row address carried along a row of cells (next cell: + TRI, one row up
        // in the triangle: - r) -- a dozen scalar instructions per cell.  The generic walk below spends ~140 (64-bit products
        // for every address, the counters' carries, the slab tests): the kernel took 1.8 ms of its 2.9 ms at 64^3 with every
        // load, LDS access and store removed (round 5).  Same cells in the same order.
        // Right-hand side and histogram shares: lane = cell, two gathers for the node instead of two one-lane loads per cell
        {
            double rv = 0.0, hv = 0.0;
            if (lane < cr.total) {
                int cell, r;
                cr.get(g, in, lane, cell, r);
                if (cell >= cell0 && cell < cell1) {
                    const long long cb = (long long)(cell - cell0);
                    rv = rblk[cb * NB + r];
                    if (hblk) hv = hblk[cb * NB + r];
                }
            }
            // summed cell after cell, as the generic walk does (the bits of rounds 1-4: a butterfly over the lanes moved the
            // second refinement correction of config 3 from 2.3e-8 to 3.9e-8 and the stopping rule's estimate across its 1e-11)
            double *tmp = stmp[wave];
            tmp[lane] = rv;
            tmp[64 + lane] = hv;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int e = 0; e < cr.total; ++e) {
                racc += tmp[e];
                hacc += tmp[64 + e];
            }
        }
        const int nx = cr.cnt[0], ny = cr.cnt[1], nz = cr.cnt[2];
        const int rx0 = in[0] - cr.lo[0];
        for (int iz = 0; iz < nz; ++iz) {
            const int cz = cr.lo[2] + iz;
            const int cellz = cz * g.cellstride[2];
            const bool zok = cellz >= cell0 && cellz < cell1;       // (a slab = whole hyper-rows of the slowest dimension)
            if (!zok) continue;
            for (int iy = 0; iy < ny; iy += 2) {
                double v[2][4];
                int rs[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const bool yok = iy + h < ny;
                    const int cy = cr.lo[1] + (yok ? iy + h : iy);
                    const int cell = cellz + cy * g.cellstride[1] + cr.lo[0];
                    int r = ((in[2] - cz) << 4) + ((in[1] - cy) << 2) + rx0;
                    rs[h] = yok ? r : -1;
                    long long off = (long long)(cell - cell0) * TRI + (long long)r * (r + 1) / 2;
#pragma unroll
                    for (int xi = 0; xi < 4; ++xi) {
                        const bool ok = yok && xi < nx;
                        v[h][xi] = (ok && lane <= r) ? blk[off + lane] : 0.0;
                        off += TRI - r;
                        r -= 1;
                    }
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    int r = rs[h];
                    if (r < 0) continue;
                    int k = (in[2] - cz) * 49 + ((r >> 2) & 3) * 7 + rx0;
#pragma unroll
                    for (int xi = 0; xi < 4; ++xi) {
                        if (xi < nx && lane <= r) acc[kc[0] - k] += v[h][xi];
                        r -= 1;
                        k -= 1;
                    }
                }
            }
        }
    } else {
    // the cells in CellRange order (dimension 0 fastest) by counters, not by divisions
    int ix[D];
#pragma unroll
    for (int d = 0; d < D; ++d) ix[d] = 0;
    for (int e0 = 0; e0 < cr.total; e0 += GB) {
        int cl[GB], rr[GB], kr[GB], o0[GB], o1[GB];
#pragma unroll
        for (int u = 0; u < GB; ++u) {
            int cell = 0, r = 0, k = 0;
            const bool have = e0 + u < cr.total;
            if (have) {
                int m7 = 1;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const int wsd = cr.lo[d] + ix[d];
                    cell += wsd * g.cellstride[d];
                    r += (in[d] - wsd) << (2 * d);
                    k += (in[d] - wsd) * m7;
                    m7 *= 7;
                }
                bool carry = true;
#pragma unroll
                for (int d = 0; d < D; ++d)
                    if (carry) {
                        if (++ix[d] < cr.cnt[d]) carry = false;
                        else ix[d] = 0;
                    }
            }
            kr[u] = k;
            const bool ok = have && cell >= cell0 && cell < cell1;
            cl[u] = ok ? cell : cell0;               // a harmless cell for the lookups below
            rr[u] = ok ? r : -1;
            if (!ZEROED) {
                o0[u] = offset[cl[u]];
                o1[u] = offset[cl[u] + 1];
            } else
                o0[u] = 0, o1[u] = 1;
        }
        double v[GB][NCH], rv[GB], hv[GB];
#pragma unroll
        for (int u = 0; u < GB; ++u) {
            if (o0[u] == o1[u]) rr[u] = -1;          // empty cell: its block was never written
            const int r = rr[u];
            const long long cb = (long long)(cl[u] - cell0);
            const double *__restrict__ row = blk + cb * TRI + (long long)(r < 0 ? 0 : r) * ((r < 0 ? 0 : r) + 1) / 2;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                const int c = lane + 64 * ch;
                v[u][ch] = (c <= r) ? row[c] : 0.0;
            }
            rv[u] = (lane == 0 && r >= 0) ? rblk[cb * NB + r] : 0.0;
            hv[u] = (lane == 0 && r >= 0 && hblk) ? hblk[cb * NB + r] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < GB; ++u) {
            const int r = rr[u];
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                const int c = lane + 64 * ch;
                if (c <= r) acc[kc[ch] - kr[u]] += v[u][ch];
            }
            racc += rv[u];
            hacc += hv[u];
        }
    }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    double *__restrict__ out = nst + (long long)node * g.hstencil;
    for (int e = lane; e < HS; e += 64) out[e] += acc[e];
    if (lane == 0) {
        rhs[node] += racc;
        if (hblk) {
            int refnode = 0;                   // the histogram is kept in the caller's dimension order
#pragma unroll
            for (int d = 0; d < D; ++d) refnode += in[d] * g.refstride[d];
            hist[refnode] += hacc;             // on top of the out-of-window points added by gram_block_kernel
        }
    }
}

// The table of the constraint rows' factors (constraints.hip) is built in THIS translation unit.  The compiler specialises
// basis_1d (basis.hpp) per translation unit on the derivative orders it is asked for there: beside constraint_table_kernel, which
// asks for all three, the Gram kernels keep the code they were tuned with.  Alone they only ask for order 0, and
// gram_block_kernel and gram_mfma4_kernel come out with other instructions (the same bits): the 1-D Gram stage then took 6.30
// instead of 6.12 ms at 2e6 points and 64 nodes, the VALU form 1.10 instead of 1.09 ms at 32^3 and 2e6 points, gram_mfma4_kernel
// the same 9.5 ms at 16^4 (medians of three alternating runs of six fits each).
//
// The factors depend on the grid alone: constraint_table_kernel tabulates them once per plan,
//   ctab[9 * (nodes_0 + .. + nodes_{d-1}) + (n * 3 + o + 1) * 3 + nder],
// and the row kernels multiply table entries instead of evaluating 3 piecewise cubics per entry (round 3: the constraint
// rows took 2.7 ms per fit at 64^3).  Same values, same order of the product: identical bits.  ctab == NULL: evaluate.
__global__ void __launch_bounds__(256)
constraint_table_kernel(Grid g, double *__restrict__ ctab)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x, base = 0;
    for (int d = 0; d < g.ndim; ++d) {
        const int cnt = 9 * g.nodes[d];
        if (t < cnt) {
            const int nder = t % 3, o = (t / 3) % 3 - 1, n = t / 9;
            ctab[base + t] = constraint_factor(g, d, n, o, nder);
            return;
        }
        t -= cnt;
        base += cnt;
    }
}

}  // namespace

long long constraint_table_doubles(const Grid &g)
{
    long long n = 0;
    for (int d = 0; d < g.ndim; ++d) n += 9LL * g.nodes[d];
    return n;
}

hipError_t launch_constraint_table(const Grid &g, double *ctab, hipStream_t st)
{
    const long long n = constraint_table_doubles(g);
    hipLaunchKernelGGL(constraint_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g, ctab);
    return hipGetLastError();
}

long long gram_scratch_doubles(const Grid &g)
{
    return (long long)g.ncell * (gram_tri(g.nb) + 2LL * g.nb);
}

long long gram_scratch_min_doubles(const Grid &g)
{   // one hyper-row of cells along the slowest dimension
    return (long long)g.cellstride[g.ndim - 1] * (gram_tri(g.nb) + 2LL * g.nb);
}


// cells per wave of gram_wave_kernel in a slab of ncells cells: GW_RUN where that still leaves four rounds of waves for the chip
// (two per SIMD), fewer on a small grid; 0: the slab goes to a kernel that does not work in runs
static int gram_run(int ndim, int ncells)
{
    if ((ndim != 2 && ndim != 3) || splpak::opt_get("SPLPAK_GRAM_VALU") != nullptr) return 0;      // A/B switch: the workgroup-per-cell form
    const int run = (int)(ncells / (4LL * 2048));
    return run < 1 ? 1 : run > GW_RUN ? GW_RUN : run;
}

bool gram_shape(const Grid &g, long long scratch_doubles, GramShape *out)
{
    const long long per_cell = gram_tri(g.nb) + 2LL * g.nb;
    const int hrow = g.cellstride[g.ndim - 1];              // cells per hyper-row
    const int nhrow = g.cells[g.ndim - 1];
    long long fit_rows = scratch_doubles / (per_cell * hrow);
    if (fit_rows < 1) return false;
    if (fit_rows > nhrow) fit_rows = nhrow;
    out->rows = (int)fit_rows;
    out->nslab = (nhrow + out->rows - 1) / out->rows;
    out->cells = out->rows * hrow;
    out->last_cells = (nhrow - (out->nslab - 1) * out->rows) * hrow;
    out->run = gram_run(g.ndim, out->cells);
    out->last_run = gram_run(g.ndim, out->last_cells);
    return true;
}

// run: gram_run of the slab.  -> true when the blocks of empty cells were written as zeros (the gather then reads every block
// unconditionally)
template <int D>
static bool gram_cells(const Grid &g, const SortScratch &s, double *blk, double *rblk, double *hblk, double *hist, int cell0,
                       int ncells, int run, hipStream_t st)
{
    const bool old_form = splpak::opt_get("SPLPAK_GRAM_VALU") != nullptr;       // A/B switch: the workgroup-per-cell form
    if constexpr (D == 2 || D == 3) {
        if (run > 0) {
            hipLaunchKernelGGL(gram_wave_kernel<D>, dim3((unsigned)((ncells + 4 * run - 1) / (4 * run))), dim3(256), 0, st, g, s.offset,
                               s.xs, s.ys, s.ws, s.cap, blk, rblk, hblk, hist, cell0, ncells, run);
            return true;
        }
    }
    if constexpr (D == 4) {
        if (!old_form) {
            hipLaunchKernelGGL(gram_mfma4_kernel<D>, dim3((unsigned)ncells), dim3(640), 0, st, g, s.offset,
                               s.xs, s.ys, s.ws, s.cap, blk, rblk, hblk, hist, cell0);
            return false;                      // (empty cells write nothing: a 263 KB zero block each would be too much)
        }
    }
    using C = GramCfg<D>;
    dim3 gr((unsigned)ncells, (unsigned)(C::NB / (C::NTX * C::TC)));
    hipLaunchKernelGGL(gram_block_kernel<D>, gr, dim3(C::NT), 0, st, g, s.offset, s.xs, s.ys, s.ws, s.cap, blk,
                       rblk, hblk, hist, cell0);
    return false;
}

hipError_t launch_gram(const Grid &g, const SortScratch &s, double *scratch, long long scratch_doubles, bool smooth,
                       double *nst, double *rhs, double *hist, double *scalH, hipStream_t st, GramShape *shape)
{
    // The per-cell blocks are produced and gathered slab by slab: as many whole hyper-rows of cells (along
    // the slowest dimension) as the scratch holds -- all of them at 64^3 (3.9 GB), two or three slabs of
    // the 189 GB that the 29^4 cells of the 4-D 32^4 grid would need at once.
    GramShape sh;
    if (!gram_shape(g, scratch_doubles, &sh)) return hipErrorInvalidValue;
    if (shape) *shape = sh;
    const int hrow = g.cellstride[g.ndim - 1];              // cells per hyper-row
    const int nhrow = g.cells[g.ndim - 1];
    const int nstride = g.colstride[g.ndim - 1];            // nodes per hyper-row of nodes
    for (int h0 = 0; h0 < nhrow; h0 += sh.rows) {
        const int h1 = (h0 + sh.rows < nhrow) ? h0 + sh.rows : nhrow;
        const int cell0 = h0 * hrow, cell1 = h1 * hrow, ncells = cell1 - cell0;
        const int run = h1 < nhrow ? sh.run : sh.last_run;
        const int node0 = h0 * nstride, node1 = (h1 + 3) * nstride;     // window starts h0..h1-1 touch nodes h0..h1+2
        double *blk = scratch;
        double *rblk = blk + (long long)ncells * gram_tri(g.nb);
        double *hblk = smooth ? rblk + (long long)ncells * g.nb : nullptr;
        DISPATCH_D(g.ndim, {
            const bool zeroed = gram_cells<D>(g, s, blk, rblk, hblk, hist, cell0, ncells, run, st);
            const dim3 gg((unsigned)((node1 - node0 + 3) / 4));
            if (zeroed)
                hipLaunchKernelGGL((stencil_gather_kernel<D, true>), gg, dim3(256), 0, st, g, s.offset, blk, rblk, hblk,
                                   nst, rhs, hist, cell0, cell1, node0, node1);
            else
                hipLaunchKernelGGL((stencil_gather_kernel<D, false>), gg, dim3(256), 0, st, g, s.offset, blk, rblk, hblk,
                                   nst, rhs, hist, cell0, cell1, node0, node1);
        });
    }
    if (smooth) return launch_hist_total(g, hist, scalH, st);
    return hipGetLastError();
}

}  // namespace splpak
