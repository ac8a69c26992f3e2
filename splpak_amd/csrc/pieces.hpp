// The pieces of a cell of an integrated axis (integrategrid.hip): the region of a coordinate, and the table entry of a piece
// -- the window start of its region and the four factors of two-point Gauss-Legendre over it.  Host and device, as basis.hpp.
#pragma once
#include "basis.hpp"

namespace splpak {

// region of x in dimension d: -1 below xmin (and for a NaN), k in node cell k, nodes - 1 from xmax on.  Saturating: the
// conversion is reached only with 0 <= t < nodes - 1.
__host__ __device__ inline int piece_region(const Grid &g, int d, double x)
{
#pragma clang fp contract(off)
    const double t = g.dxin[d] * (x - g.xmin[d]);
    const int last = g.nodes[d] - 1;
    if (!(t >= 0.0)) return -1;
    return t >= (double)last ? last : (int)t;
}

// Piece q of the n pieces of the cell e0 .. e1: its bounds are the breakpoints xmin + k dx, computed as the node coordinates
// are (basis.hpp, :246) and clamped into [lo, hi], so that neighbours share one computed bound and the pieces tile the cell.
// The window start comes from the REGION, not from the quadrature points: a piece one ulp wide next to a breakpoint has one window.
__host__ __device__ inline int piece_factors(const Grid &g, int d, double e0, double e1, int q, int n, double (&b)[4])
{
#pragma clang fp contract(off)
    const bool fwd = e0 <= e1;
    const double lo = fwd ? e0 : e1, hi = fwd ? e1 : e0;
    const int nod = g.nodes[d];
    int r = piece_region(g, d, lo) + q;
    r = r < nod - 1 ? r : nod - 1;
    const double xa = q == 0 ? lo : fmin(fmax(g.xmin[d] + (double)r * g.dx[d], lo), hi);
    const double xb = q == n - 1 ? hi : fmin(fmax(g.xmin[d] + (double)(r + 1) * g.dx[d], lo), hi);
    const double m = 0.5 * (xa + xb), h = 0.5 * (xb - xa);
    const double off = h * 0.57735026918962576451;        // 1 / sqrt(3)
    const double x1 = m - off, x2 = m + off;
    const double w = fwd ? h : -h;
    int ws = r - 1;
    ws = ws > 0 ? ws : 0;
    ws = ws < nod - 4 ? ws : nod - 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ib = ws + k;
        const double xn = g.xmin[d] + (double)ib * g.dx[d];      // :246
        const int kind = basis_kind(ib, nod);
        b[k] = w * (basis_1d(kind, 0, x1, xn, g.dxin[d]) + basis_1d(kind, 0, x2, xn, g.dxin[d]));
    }
    return ws;
}

}  // namespace splpak
