// Device functions every evaluation kernel shares: the per-dimension factor table of a coordinate and the
// factorised sum over the 4^D window.  One definition, so that the direct, the sorted and the grid kernels
// (eval.hip, evalsort.hip, evalruns.hip, evalregion.hip, evalgrid.hip) return identical bits for the same point.
#pragma once
#include "basis.hpp"

namespace splpak {

struct NDeriv { int v[MAXD]; };
// the pattern a call evaluates: orders outside 0 .. 2 are clamped (the entries report them as 104), dimensions beyond ndim are 0
inline NDeriv clamp_nderiv(const int *nderiv, int ndim)
{
    NDeriv nd;
    for (int d = 0; d < MAXD; ++d) {
        const int v = (nderiv && d < ndim) ? nderiv[d] : 0;
        nd.v[d] = v < 0 ? 0 : (v > 2 ? 2 : v);
    }
    return nd;
}
// no derivative in any dimension: the kernels take the branch-free value form of the factor tables (eval_table<true>)
inline bool value_only(const NDeriv &nd)
{
    bool v = true;
    for (int d = 0; d < MAXD; ++d) v = v && nd.v[d] == 0;
    return v;
}

// The 4 coefficients of a window row (k0 = 0..3 from p on), widened to double.  They are contiguous: two 16-byte loads
// (REAL32: one) instead of four 8-byte ones (the gathering kernels are bound by gather instructions / L2 lines, not bytes).
// The load4 of window_sum in the direct, the fields and the grid kernels' general form.
template <typename T>
__device__ inline void load_window_row(const T *p, double (&c)[4])
{
    if constexpr (sizeof(T) == 8) {
        typedef double d2v __attribute__((ext_vector_type(2), aligned(8)));
        const d2v lo = *reinterpret_cast<const d2v *>(p);
        const d2v hi = *reinterpret_cast<const d2v *>(p + 2);
        c[0] = lo[0]; c[1] = lo[1]; c[2] = hi[0]; c[3] = hi[1];
    } else {
        typedef float f4v __attribute__((ext_vector_type(4), aligned(4)));
        const f4v v = *reinterpret_cast<const f4v *>(p);
        c[0] = v[0]; c[1] = v[1]; c[2] = v[2]; c[3] = v[3];
    }
}

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


// ---- fused value + gradient (+ Hessian) ------------------------------------------------------------
// all derivative patterns of total order <= ORDER from ONE pass over the window, instead
// of one splde call (:1089-1240) per pattern.  Output per query, ldout apart:
//   [ f, df/dx_1 .. df/dx_D, (ORDER 2:) d2f/dx_1dx_1, d2f/dx_1dx_2, .., d2f/dx_1dx_D, d2f/dx_2dx_2, .. ]
// Each entry is the reference's sum  sum_window coef * prod_d bas1(nderiv_d; x_d)  for its nderiv
// pattern; the 1-D factors come from the same window_table as everywhere else.
// acc[*] for one query from its factor tables b[a][d][k] (a = derivative order) and a loader of window
// rows: load4(k, c) delivers the 4 coefficients (k_0 = 0..3) of the row with window indices k[1..D-1].
// Shared by the direct and the binned kernel: identical bits.
template <int D, int ORDER, typename L4>
__device__ inline void derivs_accumulate(const double (&b)[ORDER + 1][D][4], L4 &&load4,
                                         double (&acc)[1 + D + (ORDER == 2 ? D * (D + 1) / 2 : 0)])
{
    constexpr int NOUT = 1 + D + (ORDER == 2 ? D * (D + 1) / 2 : 0);
#pragma unroll
    for (int j = 0; j < NOUT; ++j) acc[j] = 0.0;
    // window rows (k_0 = 0..3 contiguous): contract dimension 1 with its value / first / second
    // derivative factors first, then combine with the factors of the other dimensions
    constexpr int NROW = D == 1 ? 1 : (D == 2 ? 4 : (D == 3 ? 16 : 64));
    for (int e = 0; e < NROW; ++e) {
        int k[D];
        k[0] = 0;
#pragma unroll
        for (int d = 1; d < D; ++d) k[d] = (e >> (2 * (d - 1))) & 3;
        double c[4];
        load4(k, c);
        double r[ORDER + 1];                  // r[a] = sum_k0 c[k0] * (a-th derivative factor of dim 1)
#pragma unroll
        for (int a = 0; a <= ORDER; ++a) {
            double t = 0.0;
#pragma unroll
            for (int k0 = 0; k0 < 4; ++k0) t = fma(c[k0], b[a][0][k0], t);
            r[a] = t;
        }
        double v0[D], v1[D], pex[D];          // dims >= 1: pex[d] = prod_{f >= 1, f != d} v0[f]
        double full = 1.0;                    // prod_{f >= 1} v0[f]
        v0[0] = v1[0] = pex[0] = 1.0;
#pragma unroll
        for (int d = 1; d < D; ++d) {
            v0[d] = b[0][d][k[d]];
            v1[d] = b[1][d][k[d]];
            full *= v0[d];
        }
#pragma unroll
        for (int d = 1; d < D; ++d) {
            double pd = 1.0;
#pragma unroll
            for (int f = 1; f < D; ++f)
                if (f != d) pd *= v0[f];
            pex[d] = pd;
        }
        acc[0] = fma(r[0], full, acc[0]);
        acc[1] = fma(r[1], full, acc[1]);
#pragma unroll
        for (int d = 1; d < D; ++d) acc[1 + d] = fma(r[0], v1[d] * pex[d], acc[1 + d]);
        if constexpr (ORDER == 2) {
            int j = 1 + D;
#pragma unroll
            for (int d = 0; d < D; ++d)
#pragma unroll
                for (int f = d; f < D; ++f) {
                    double term;
                    if (d == 0 && f == 0) {
                        term = r[2] * full;
                    } else if (d == 0) {
                        term = r[1] * (v1[f] * pex[f]);
                    } else if (f == d) {
                        term = r[0] * (b[2][d][k[d]] * pex[d]);
                    } else {
                        double pdf = 1.0;
#pragma unroll
                        for (int h = 1; h < D; ++h)
                            if (h != d && h != f) pdf *= v0[h];
                        term = r[0] * (v1[d] * v1[f] * pdf);
                    }
                    acc[j] += term;
                    ++j;
                }
        }
    }
}

}  // namespace splpak
