// Device functions every evaluation kernel shares: the per-dimension factor table of a coordinate and the
// factorised sum over the 4^D window.  One definition, so that the direct, the sorted and the grid kernels
// (eval.hip, evalgrid.hip) return identical bits for the same point.
#pragma once
#include "basis.hpp"

namespace splpak {

struct NDeriv { int v[MAXD]; };

// Sum of the 4^D window products, factorised: the innermost dimension is contracted with its four
// factors first, then the partial sums with the factors of the next dimension, and so on -- 64 + 16 + 4
// fused multiply-adds in 3-D instead of the 64 * 3 multiplications of the plain triple product (the
// reference forms every product basm = prod_d bas1_d and adds coef*basm, :1215-1236; the two orders
// differ by rounding only).  load4(k1, k2, k3, c) delivers the 4 coefficients of the window row
// (k0 = 0..3).  Shared by the direct and the binned kernels so that both produce bit-identical values.
template <int D, typename L4>
__device__ inline double window_sum(const double (&b)[D][4], L4 &&load4)
{
    auto row = [&](int k1, int k2, int k3) {
        double c[4];
        load4(k1, k2, k3, c);
        double t = c[0] * b[0][0];
        t = fma(c[1], b[0][1], t);
        t = fma(c[2], b[0][2], t);
        t = fma(c[3], b[0][3], t);
        return t;
    };
    if constexpr (D == 1) {
        return row(0, 0, 0);
    } else if constexpr (D == 2) {
        double sum = 0.0;
#pragma unroll
        for (int k1 = 0; k1 < 4; ++k1) sum = fma(row(k1, 0, 0), b[1][k1], sum);
        return sum;
    } else if constexpr (D == 3) {
        double sum = 0.0;
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2) {
            double r = 0.0;
#pragma unroll
            for (int k1 = 0; k1 < 4; ++k1) r = fma(row(k1, k2, 0), b[1][k1], r);
            sum = fma(r, b[2][k2], sum);
        }
        return sum;
    } else {
        double sum = 0.0;
        for (int k3 = 0; k3 < 4; ++k3) {
            double q = 0.0;
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2) {
                double r = 0.0;
#pragma unroll
                for (int k1 = 0; k1 < 4; ++k1) r = fma(row(k1, k2, k3), b[1][k1], r);
                q = fma(r, b[2][k2], q);
            }
            sum = fma(q, b[3][k3], sum);
        }
        return sum;
    }
}

// the 4-entry factor table of dimension d: the branch-free value form when no derivative is asked for
template <bool VAL>
__device__ inline int eval_table(const Grid &g, int d, double x, int nder, double (&b)[4])
{
    if constexpr (VAL) {
        int lo, hi, it;
        bool interior;
        double u, t;
        const int ws = window_start_frac(g, d, x, lo, hi, interior, u, t, it);
        // every lane computes the closed form of an interior window (16 operations); a wave that holds queries whose window
        // in this dimension is NOT interior also computes, for those lanes, the form of a window next to an end of the grid
        // (the first / last three cells: end functions put into the closed form, window_values_near) and, if it holds
        // queries OUTSIDE the grid (or the grid has fewer than 8 nodes), the general form for these.  Which form a query
        // gets depends on the query alone.
        window_values_interior(u, b);
        if (__builtin_amdgcn_ballot_w64(!interior) != 0) {
            const int nod = g.nodes[d];
            const bool near = !interior && nod >= 8 && t >= 0.0 && it <= nod - 2;
            double bn[4];
            window_values_near(t, it, nod, b, bn);
            if (__builtin_amdgcn_ballot_w64(!interior && !near) != 0) {
                double bg[4];
                window_values<false>(g, d, x, ws, lo, hi, bg);
#pragma unroll
                for (int k = 0; k < 4; ++k) bn[k] = near ? bn[k] : bg[k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) b[k] = interior ? b[k] : bn[k];
        }
        return ws;
    } else {
        return window_table(g, d, x, nder, b);
    }
}

}  // namespace splpak
