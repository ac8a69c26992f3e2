// What more than one stage of the assembly uses on the device, and grid_for of their launchers (binpoints.hip, gram.hip, constraints.hip, residual.hip,
// sums.hip, expand.hip).  Everything lives in an anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "basis.hpp"
#include "kernels.hpp"

namespace splpak {
namespace {


// Cells whose window contains node `in`: window starts ws_d in [max(in_d - 3, 0), min(in_d, cells_d - 1)],
// enumerated with dimension 0 fastest -- THE fixed summation order of every gather (stencil_gather_kernel, rho_gather_kernel).
template <int D>
struct CellRange {
    int lo[D], cnt[D], total;
    __device__ CellRange(const Grid &g, const int *in)
    {
        total = 1;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            lo[d] = in[d] - 3 > 0 ? in[d] - 3 : 0;
            const int hi = in[d] < g.cells[d] - 1 ? in[d] : g.cells[d] - 1;
            cnt[d] = hi - lo[d] + 1;
            total *= cnt[d];
        }
    }
    // e-th cell: its linear index, and the node's local basis index r inside that cell's window
    __device__ void get(const Grid &g, const int *in, int e, int &cell, int &r) const
    {
        cell = 0;
        r = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int wsd = lo[d] + e % cnt[d];
            e /= cnt[d];
            cell += wsd * g.cellstride[d];
            r += (in[d] - wsd) << (2 * d);
        }
    }
};

// a node's "data sparse" flag and constraint weight (sparse_node: constraints.hip)
struct SparseNode {
    bool sparse;
    double dcwght;
};

// The derivative-constraint rows (what they are: the head of constraints.hip), as constraints.hip adds them to the normal
// equations and residual.hip applies them to a vector.
// derivative orders and weight of constraint row `pair` (idm <= jdm enumerated row by row) of node `in`
template <int D>
__device__ inline double constraint_pattern(const Grid &g, const int *in, int idm, int jdm, double dcwght, int *nder)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int d = 0; d < D; ++d) nder[d] = 0;
    bool boundary = true;
    double rowwt = 2.0 * dcwght;                                  // :983
    if (jdm == idm) {
        rowwt = dcwght;
        nder[jdm] = 2;
        if (in[idm] != 0 && in[idm] != g.nodes[idm] - 1) boundary = false;
    }
    if (boundary) { nder[idm] = 1; nder[jdm] = 1; }                // :998-999
    return rowwt;
}

// one dimension's factor of a constraint-row entry: derivative `nder` of the basis function of node n + o at node n
__device__ inline double constraint_factor(const Grid &g, int d, int n, int o, int nder)
{
#pragma clang fp contract(off)
    const int ib = n + o;
    if (ib < 0 || ib > g.nodes[d] - 1) return 0.0;
    const double xnode = g.xmin[d] + (double)n * g.dx[d];         // :943
    const double xb = g.xmin[d] + (double)ib * g.dx[d];
    return basis_1d(basis_kind(ib, g.nodes[d]), nder, xnode, xb, g.dxin[d]);
}

// entry of the constraint row of node n (coordinates nn) at node j = nn + off (off_d in [-1,1]); 0 outside the grid
template <int D>
__device__ inline double constraint_entry(const Grid &g, const double *__restrict__ ctab, const int *nn, const int *off,
                                          const int *nder, double rowwt)
{
#pragma clang fp contract(off)
    double basm = 1.0;
    int base = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const int ib = nn[d] + off[d];
        if (ib < 0 || ib > g.nodes[d] - 1) return 0.0;
        basm *= ctab ? ctab[base + (nn[d] * 3 + off[d] + 1) * 3 + nder[d]] : constraint_factor(g, d, nn[d], off[d], nder[d]);
        base += 9 * g.nodes[d];
    }
    return rowwt * basm;                                          // :1011
}

// acc - (C^T t)_i for node i (coordinates in): over the data-sparse neighbours n of i (3^D offsets, dimension 0 fastest) and their rows,
// row(n, pair)[i] * t[n][pair] with t = C x from constraint_dots_kernel (tbuf: [ncol][D (D + 1) / 2]) -- the constraint term of the
// residual passes' gathers (residual.hip rho_gather_kernel, rows3tile.hip rows3_gather_kernel), one order of the subtractions
template <int D>
__device__ inline double constraint_term(const Grid &g, const int *in, const double *__restrict__ dcw, const unsigned char *__restrict__ spf,
                                         const double *__restrict__ ctab, const double *__restrict__ tbuf, double acc)
{
    constexpr int NE = (D == 1) ? 3 : (D == 2) ? 9 : (D == 3) ? 27 : 81;
    constexpr int NP = D * (D + 1) / 2;
    for (int ne = 0; ne < NE; ++ne) {
        int nn[D], offi[D], t = ne, ncol_n = 0;
        bool ok = true;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int o = t % 3 - 1;
            t /= 3;
            nn[d] = in[d] + o;
            offi[d] = -o;
            ok = ok && nn[d] >= 0 && nn[d] <= g.nodes[d] - 1;
            ncol_n += nn[d] * g.colstride[d];
        }
        if (!ok) continue;
        if (spf[ncol_n] == 0) continue;
        SparseNode sn;
        sn.sparse = true;
        sn.dcwght = dcw[ncol_n];
        int pair = 0;
        for (int idm = 0; idm < D; ++idm)
            for (int jdm = idm; jdm < D; ++jdm, ++pair) {
                int nder[D];
                const double rowwt = constraint_pattern<D>(g, nn, idm, jdm, sn.dcwght, nder);
                const double ci = constraint_entry<D>(g, ctab, nn, offi, nder, rowwt);
                if (ci != 0.0) acc -= ci * tbuf[(long long)ncol_n * NP + pair];
            }
    }
    return acc;
}

// workgroups of `threads` for a grid-stride loop over n items
inline unsigned grid_for(long long n, int threads, long long maxblocks = 256LL * 16)
{
    long long b = (n + threads - 1) / threads;
    if (b < 1) b = 1;
    if (b > maxblocks) b = maxblocks;
    return (unsigned)b;
}

}  // namespace
}  // namespace splpak
