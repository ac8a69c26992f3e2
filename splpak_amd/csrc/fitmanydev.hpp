// One small fit on the LDS of its workgroup: the device side the batch kernels share (fitmany.hip and fitmanycov.hip call
// fit_problem once per problem; fitmanyclip.hip and fitmanymad.hip once per pass of their clipping loops), and problem_of,
// with which each of them opens a problem.  The LDS map is that of fitmany.hpp.
//
// Phases of a problem, all on the workgroup's own LDS:
//   1 assemble   the points are staged FITMANY_CHUNK at a time: a thread per point computes the window tables of basis.hpp,
//                w, w y and the nearest-node address; then the OWNER of band row i (thread i mod 256) walks the staged points
//                in index order and adds the entries of its row, its right-hand side and its histogram word.
//   2 sparse     (xtrap != 0) the 0.75 rule per node, dcwght, and C^T C of the derivative-constraint rows into the band,
//                row by row, from the row patterns of assemble_dev.hpp (what constraints.hip adds for the single fit).
//   3 factor     right-looking Cholesky of the band in place, with the pivot test of the point fit (chol_device.hpp): a pivot
//                that is not positive fails.  (The floor of the grid fit, ncol * eps * the largest diagonal entry, has no place
//                here: a constraint row puts 1e13 on the diagonal beside the 1 of a node that only data rows reach.)
//   4 solve      forward and backward substitution (1-D: one thread with the last three unknowns in registers; 2-D: wave 0,
//                one lane per band entry of the row, summed by the fixed butterfly of wave_sum).
//   5 refine     RefineRule of fitgriddev.hpp: the gradient A^T W (W y - W A x) - C^T C x is recomputed from the rows
//                (points staged again, owners walk them in index order), solved, added.
//   6 inverse    (splpak_fit_many_cov_* alone: fitmanycov.hip) the band of N^-1 from the factor, in place, and its half stencils
//                to global memory (selected_inverse below).
// Determinism: every sum has one owner and a fixed order -- the point order of the problem, the neighbour order of a node,
// the lane tree of a reduction -- none of which depends on the batch, the position in it or the workgroup.  No atomics.
#pragma once
#include "fitmany.hpp"
#include "fitgriddev.hpp"
#include "assemble_dev.hpp"

#include <cmath>

namespace splpak {
namespace fitmanydev {

struct Lds {
    double *band, *rhs, *x, *rho, *dcw, *stage, *scal;
    int *ws, *addr;
    unsigned char *spf;
};

__device__ inline Lds carve(double *base, const FitManyShape &sh)
{
    Lds L;
    L.band = base + sh.band;
    L.rhs = base + sh.rhs;
    L.x = base + sh.x;
    L.rho = base + sh.rho;
    L.dcw = base + sh.dcw;
    L.stage = base + sh.stage;
    L.scal = base + sh.scal;
    L.ws = reinterpret_cast<int *>(base + sh.doubles);
    L.addr = L.ws + FITMANY_CHUNK * sh.ndim;
    L.spf = reinterpret_cast<unsigned char *>(L.addr + FITMANY_CHUNK);
    return L;
}

// max that keeps a NaN
__device__ inline double nanmax(double a, double b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }

// sum / max of v over the NT threads of the workgroup in every thread: a fixed tree through `red` (the stage: 256 doubles at least)
template <bool MAX, int NT>
__device__ inline double block_reduce(double v, double *red)
{
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = MAX ? nanmax(red[t], red[t + s]) : red[t] + red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

template <int D>
__device__ inline void node_of(const Grid &g, int i, int *in)
{
    if (D == 1) in[0] = i;
    else { in[0] = i % g.nodes[0]; in[1] = i / g.nodes[0]; }
}

// A thread per staged point: window tables, w and w y (RES: the row's residual w y - w A x), histogram address.
// A point of weight 0 gets window starts no row matches.  WP: the weights' pointer type -- `const T *__restrict__` where the
// kernel never writes them, a plain `const T *` where it does (the clipping loop).
template <int D, typename T, bool RES, int NT, typename WP>
__device__ inline void stage_chunk(const FitManyArgs &a, const Lds &L, const T *__restrict__ xd, const T *__restrict__ yd,
                                   WP wd, bool weighted, long long p0, int cnt, int &nrows, double &ssq)
{
    for (int t = threadIdx.x; t < FITMANY_CHUNK; t += NT) {
        double *sb = L.stage + t * (4 * D + 2);
        if (t >= cnt) {      // the padding of the owners' walk
#pragma unroll
            for (int d = 0; d < D; ++d) L.ws[t * D + d] = -1000000;
            sb[4 * D] = 0.0;
            L.addr[t] = -1;
            continue;
        }
        const long long p = p0 + t;
        const double w = weighted ? (double)wd[p] : 1.0;
        if (w == 0.0) {
#pragma unroll
            for (int d = 0; d < D; ++d) L.ws[t * D + d] = -1000000;
            sb[4 * D] = 0.0;
            sb[4 * D + 1] = 0.0;
            L.addr[t] = -1;
            continue;
        }
        double xr[D];
#pragma unroll
        for (int d = 0; d < D; ++d) xr[d] = (double)xd[p * a.l1xdat + d];
        const double y = (double)yd[p];
        int ws[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double xv = (D == 2 && a.g.perm[d] == 1) ? xr[D - 1] : xr[0];
            ws[d] = window_table(a.g, d, xv, 0, sb + 4 * d);
            L.ws[t * D + d] = ws[d];
        }
        sb[4 * D] = w;
        if (!RES) {
            sb[4 * D + 1] = w * y;
            L.addr[t] = a.xtrap != 0.0 ? nearest_node_address(a.g, xr) : -1;
            ++nrows;
        } else {
            double acc = 0.0;
            if (D == 1) {
#pragma unroll
                for (int q = 0; q < 4; ++q) acc += (w * sb[q]) * L.x[ws[0] + q];
            } else {
                const int n0 = a.g.nodes[0];
                for (int q1 = 0; q1 < 4; ++q1)
#pragma unroll
                    for (int q0 = 0; q0 < 4; ++q0) acc += (w * (sb[q0] * sb[4 + q1])) * L.x[(ws[0] + q0) + (ws[D - 1] + q1) * n0];
            }
            const double e = w * y - acc;
            sb[4 * D + 1] = e;
            ssq += e * e;
        }
    }
}

// The owner of row i walks the staged points in order.  !RES: its band row, right-hand side and histogram word (thread 0 also
// the total of the bumps); RES: its entry of the gradient.  The window starts and addresses of FITMANY_WALK points are read
// together before any of them is looked at: a walk that asks for one point's words at a time waits a whole LDS round trip per
// point, with only ncol of the 256 threads at work (the stage pads a chunk to a multiple of FITMANY_WALK with points no row meets).
template <int D, bool RES, int NT>
__device__ inline void owner_chunk(const FitManyArgs &a, const Lds &L, int cnt, double &tot)
{
    const int n0 = a.g.nodes[0], ld = a.sh.ld, ncol = a.sh.ncol;
    const int cntw = (cnt + FITMANY_WALK - 1) / FITMANY_WALK * FITMANY_WALK;
    for (int i = threadIdx.x; i < ncol; i += NT) {
        int in[D];
        node_of<D>(a.g, i, in);
        double *row = L.band + (long long)i * ld;
        double acc = RES ? L.rho[i] : L.rhs[i];
        double h = RES ? 0.0 : L.dcw[i];
        for (int pb = 0; pb < cntw; pb += FITMANY_WALK) {
            int r0v[FITMANY_WALK], r1v[FITMANY_WALK], adv[FITMANY_WALK];
#pragma unroll
            for (int u = 0; u < FITMANY_WALK; ++u) {
                r0v[u] = in[0] - L.ws[(pb + u) * D];
                r1v[u] = D == 2 ? in[D - 1] - L.ws[(pb + u) * D + D - 1] : 0;
                adv[u] = RES ? -1 : L.addr[pb + u];
            }
#pragma unroll
            for (int u = 0; u < FITMANY_WALK; ++u) {
                const double *sb = L.stage + (pb + u) * (4 * D + 2);
                if (!RES) {
                    if (adv[u] == i) h += sb[4 * D];
                    if (i == 0 && adv[u] >= 0) tot += sb[4 * D];
                }
                const int r0 = r0v[u], r1 = r1v[u];
                if ((unsigned)r0 > 3u || (unsigned)r1 > 3u) continue;
                const double w = sb[4 * D];
                const double ai = w * (D == 2 ? sb[r0] * sb[4 + r1] : sb[r0]);
                acc += ai * sb[4 * D + 1];
                if (!RES) {
                    if (D == 1) {
                        for (int q0 = 0; q0 <= r0; ++q0) row[r0 - q0] += ai * (w * sb[q0]);
                    } else {
                        for (int q1 = 0; q1 <= r1; ++q1) {
                            const int q0end = q1 == r1 ? r0 : 3;
                            for (int q0 = 0; q0 <= q0end; ++q0) row[(r0 - q0) + n0 * (r1 - q1)] += ai * (w * (sb[q0] * sb[4 + q1]));
                        }
                    }
                }
            }
        }
        if (RES) L.rho[i] = acc;
        else { L.rhs[i] = acc; L.dcw[i] = h; }
    }
}

// The derivative-constraint rows of the data-sparse nodes around row i, neighbours and rows in a fixed order.
// !RES: band row i += (C^T C)(i, j <= i);  RES: rho[i] -= (C^T C x)_i, and ssq += (C x)^2 of the rows of node i itself.
template <int D, bool RES, int NT>
__device__ inline void constraint_rows(const FitManyArgs &a, const Lds &L, double &ssq)
{
    constexpr int NE = D == 1 ? 3 : 9;
    const Grid &g = a.g;
    const int ld = a.sh.ld, ncol = a.sh.ncol;
    for (int i = threadIdx.x; i < ncol; i += NT) {
        int in[D];
        node_of<D>(g, i, in);
        double *row = L.band + (long long)i * ld;
        double acc = 0.0;
        for (int ne = 0; ne < NE; ++ne) {
            int nn[D], offi[D], t = ne, nl = 0;
            bool ok = true;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int o = t % 3 - 1;
                t /= 3;
                nn[d] = in[d] + o;
                offi[d] = -o;
                ok = ok && nn[d] >= 0 && nn[d] <= g.nodes[d] - 1;
                nl += nn[d] * g.colstride[d];
            }
            if (!ok || !L.spf[nl]) continue;
            const double dcwght = L.dcw[nl];
            for (int idm = 0; idm < D; ++idm)
                for (int jdm = idm; jdm < D; ++jdm) {
                    int nder[D];
                    const double rowwt = constraint_pattern<D>(g, nn, idm, jdm, dcwght, nder);
                    const double ci = constraint_entry<D>(g, nullptr, nn, offi, nder, rowwt);
                    if (!RES && ci == 0.0) continue;
                    double dot = 0.0;
                    for (int je = 0; je < NE; ++je) {
                        int offj[D], tt = je, jl = 0;
#pragma unroll
                        for (int d = 0; d < D; ++d) {
                            offj[d] = tt % 3 - 1;
                            tt /= 3;
                            jl += (nn[d] + offj[d]) * g.colstride[d];
                        }
                        const double cj = constraint_entry<D>(g, nullptr, nn, offj, nder, rowwt);      // 0 outside the grid
                        if (cj == 0.0) continue;
                        if (RES) dot += cj * L.x[jl];
                        else if (jl <= i) row[i - jl] += ci * cj;
                    }
                    if (RES) {
                        acc += ci * dot;
                        if (nl == i) ssq += dot * dot;
                    }
                }
        }
        if (RES) L.rho[i] -= acc;
    }
}

// v <- N^-1 v with the factor in the band; every thread of the workgroup calls it
template <int D>
__device__ inline void band_solve(const Lds &L, const FitManyShape &sh, double *v)
{
    const int n = sh.ncol, ld = sh.ld, hb = sh.hb;
    __syncthreads();
    if (D == 1) {
        if (threadIdx.x == 0) {
            double x1 = 0.0, x2 = 0.0, x3 = 0.0;
            for (int i = 0; i < n; ++i) {
                const double *r = L.band + (long long)i * 4;
                const double xi = (((v[i] - r[1] * x1) - r[2] * x2) - r[3] * x3) / r[0];
                v[i] = xi;
                x3 = x2; x2 = x1; x1 = xi;
            }
            x1 = x2 = x3 = 0.0;      // x[i + 1], x[i + 2], x[i + 3]
            for (int i = n - 1; i >= 0; --i) {
                const double l1 = i + 1 < n ? L.band[(long long)(i + 1) * 4 + 1] : 0.0;
                const double l2 = i + 2 < n ? L.band[(long long)(i + 2) * 4 + 2] : 0.0;
                const double l3 = i + 3 < n ? L.band[(long long)(i + 3) * 4 + 3] : 0.0;
                const double xi = (((v[i] - l1 * x1) - l2 * x2) - l3 * x3) / L.band[(long long)i * 4];
                v[i] = xi;
                x3 = x2; x2 = x1; x1 = xi;
            }
        }
        __syncthreads();
        return;
    }
    const int lane = threadIdx.x & 63;
    for (int i = 0; i < n; ++i) {
        if (threadIdx.x < 64) {
            double s = 0.0;
            for (int k = lane + 1; k <= hb; k += 64)
                if (i - k >= 0) s += L.band[(long long)i * ld + k] * v[i - k];
            s = wave_sum(s);
            if (lane == 0) v[i] = (v[i] - s) / L.band[(long long)i * ld];
        }
        __syncthreads();
    }
    for (int i = n - 1; i >= 0; --i) {
        if (threadIdx.x < 64) {
            double s = 0.0;
            for (int k = lane + 1; k <= hb; k += 64)
                if (i + k < n) s += L.band[(long long)(i + k) * ld + k] * v[i + k];
            s = wave_sum(s);
            if (lane == 0) v[i] = (v[i] - s) / L.band[(long long)i * ld];
        }
        __syncthreads();
    }
}

// What fit_problem leaves in registers, the same in every thread of the workgroup.
struct FitOutcome {
    double rows, crows, minpiv, ssq;
    RefineRule rule;
    bool fail;
};

// The FM_* block of a problem (fitmany.hpp) from its outcome; one thread calls it
__device__ inline void store_outcome(const FitOutcome &o, double *res)
{
    res[FM_ROWS] = o.rows;
    res[FM_CROWS] = o.crows;
    res[FM_STEPS] = (double)o.rule.steps;
    res[FM_LASTREL] = o.rule.last_rel;
    res[FM_MINPIV] = o.minpiv;
    res[FM_RESERR] = sqrt(o.ssq);
    res[FM_STATUS] = o.fail ? 107.0 : 0.0;
    res[FM_SPARE] = 0.0;
}

// Run r of a launch: problem k of the batch, its np points from p0 on in the device arrays, and the slot of its coefficients
// (and covariance): r where the problems that run lie back to back (the host entries), k otherwise.  (The slot is formed
// where it is used, after the first-weight decision: formed with the rest, the kernels come out scheduled differently.)
struct Problem {
    int k;
    long long p0, np;
    int r, compact;
    __device__ long long slot() const { return compact ? r : k; }
};

__device__ inline Problem problem_of(const FitManyArgs &a, int r)
{
    const int k = a.plist[r];
    return {k, a.offsets[k] - a.base, a.offsets[k + 1] - a.offsets[k], r, a.compact};
}

// the first-weight decision of a problem (:581-588, :796): weights are given and the first of them is not negative
// (a NaN is not negative: the weights count, and the problem ends in 107 instead of being fitted without them)
template <typename T>
__device__ inline bool first_weight_counts(const T *__restrict__ wd, long long p0)
{
    return wd != nullptr && !((double)wd[p0] < 0.0);
}

// 6 selected inverse (splpak_fit_many_cov_*): the entries of Z = N^-1 inside the band, by Takahashi's recurrence on the factor,
// in place.  The band holds L (L L^T = N) as band[i * ld + k] = L(i, i - k); column i of Z, for i = ncol-1 .. 0 and
// m = min(hb, ncol-1-i), is
//     Z(j, i) = -(sum_{k = i+1 .. i+m} Z(j, k) L(k, i)) / L(i, i)                      j = i+1 .. i+m
//     Z(i, i) = (1 / L(i, i) - sum_{k = i+1 .. i+m} Z(k, i) L(k, i)) / L(i, i)
// where Z(j, k) = Z(k, j) lies in a column after i, which the band already holds: Z(j, k) at band[max * ld + |j - k|].  Column i
// of Z goes where column i of L was, so that column is copied out first: 1-D into registers, 2-D into the stage.
//   1-D  (hb = 3) one thread, with the six entries of the live 3 x 3 block of Z in registers, as the 1-D solve keeps its last
//        three unknowns: the chain per column is three fused sums, a division, a fourth sum and a division.
//   2-D  lane t of wave 0 owns Z(i + t, i): it walks k in ascending order, then the diagonal's sum over the lanes is the fixed
//        butterfly of wave_sum (hb + 1 <= 40 lanes are live: a grid inside the LDS rule has min(nodes) <= 12).  The stage is two
//        buffers of 64: while column i is worked from one, the same lanes copy column i - 1 of L, which nobody writes before
//        step i - 1, into the other -- one barrier per column.
// Every sum has one owner and a fixed order; no atomics.  Then the half stencil of every node goes to global memory in the
// caller's node order: cov[i * hst + code] = Z(i, i + o), code = sum_d (o_d + 3) 7^d <= centre, 0 where i + o is outside the
// grid (include/splpak_hip.h) -- all zeros where the fit failed.  Every thread of the workgroup calls it, after fit_problem.
template <int D, typename T, int NT>
__device__ inline void selected_inverse(const FitManyArgs &a, const Lds &L, bool fail, T *__restrict__ cov)
{
    const Grid &g = a.g;
    const int tid = threadIdx.x, n = a.sh.ncol, ld = a.sh.ld, hb = a.sh.hb;
    constexpr int HST = D == 1 ? 4 : 25;
    if (fail) {
        for (long long e = tid; e < (long long)n * HST; e += NT) cov[e] = (T)0;
        return;
    }
    __syncthreads();
    if constexpr (D == 1) {
        if (tid == 0) {
            double *b = L.band;
            // the block of Z on rows / columns i+1 .. i+3 (0 beyond the grid)
            double z11 = 0.0, z21 = 0.0, z31 = 0.0, z22 = 0.0, z32 = 0.0, z33 = 0.0;
            double l0 = b[(long long)(n - 1) * 4], l1 = 0.0, l2 = 0.0, l3 = 0.0;
            for (int i = n - 1; i >= 0; --i) {
                // column i - 1 of L, read before column i of Z is stored (the two never share a word)
                double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
                if (i > 0) {
                    m0 = b[(long long)(i - 1) * 4];
                    m1 = b[(long long)i * 4 + 1];
                    m2 = i + 1 < n ? b[(long long)(i + 1) * 4 + 2] : 0.0;
                    m3 = i + 2 < n ? b[(long long)(i + 2) * 4 + 3] : 0.0;
                }
                const double r = 1.0 / l0;
                const double y1 = -(((z11 * l1) + z21 * l2) + z31 * l3) * r;
                const double y2 = -(((z21 * l1) + z22 * l2) + z32 * l3) * r;
                const double y3 = -(((z31 * l1) + z32 * l2) + z33 * l3) * r;
                const double y0 = (r - (((y1 * l1) + y2 * l2) + y3 * l3)) * r;
                b[(long long)i * 4] = y0;
                if (i + 1 < n) b[(long long)(i + 1) * 4 + 1] = y1;
                if (i + 2 < n) b[(long long)(i + 2) * 4 + 2] = y2;
                if (i + 3 < n) b[(long long)(i + 3) * 4 + 3] = y3;
                z33 = z22; z32 = z21; z22 = z11;
                z11 = y0; z21 = y1; z31 = y2;
                l0 = m0; l1 = m1; l2 = m2; l3 = m3;
            }
        }
    } else {
        double *buf = L.stage;      // [2][64]
        if (tid < 64) buf[((n - 1) & 1) * 64 + tid] = tid == 0 ? L.band[(long long)(n - 1) * ld] : 0.0;
        __syncthreads();
        for (int i = n - 1; i >= 0; --i) {
            if (tid < 64) {
                const int m = hb < n - 1 - i ? hb : n - 1 - i;
                const double *lc = buf + (i & 1) * 64;      // lc[t] = L(i + t, i), t = 0 .. m
                const double r = 1.0 / lc[0];
                const int j = i + tid;
                double z = 0.0;
                if (tid >= 1 && tid <= m) {
                    double s = 0.0;
                    for (int k = i + 1; k <= i + m; ++k) {
                        const int hi = k > j ? k : j, lo = k > j ? j : k;
                        s += L.band[(long long)hi * ld + (hi - lo)] * lc[k - i];
                    }
                    z = -s * r;
                }
                // column i - 1 of L into the other buffer (rows i - 1 .. i - 1 + min(hb, n - i))
                if (i > 0) {
                    const int mp = hb < n - i ? hb : n - i;
                    buf[((i - 1) & 1) * 64 + tid] = tid <= mp ? L.band[(long long)(i - 1 + tid) * ld + tid] : 0.0;
                }
                const double sd = wave_sum(tid >= 1 && tid <= m ? z * lc[tid] : 0.0);
                if (tid == 0) L.band[(long long)i * ld] = (r - sd) * r;
                else if (tid <= m) L.band[(long long)j * ld + tid] = z;
            }
            __syncthreads();
        }
    }
    __syncthreads();

    for (long long e = tid; e < (long long)n * HST; e += NT) {
        const int iref = (int)(e / HST), code = (int)(e % HST);
        double v = 0.0;
        if constexpr (D == 1) {
            const int j = iref - 3 + code;     // o = code - 3 <= 0
            if (j >= 0) v = L.band[(long long)iref * 4 + (iref - j)];
        } else {
            // the caller's node (r0, r1) and its neighbour at o; internal dimension d is the caller's perm[d]
            const int n0r = g.ref_nodes[0], n1r = g.ref_nodes[1];
            int ir[2], jr[2];
            ir[0] = iref % n0r; ir[1] = iref / n0r;
            jr[0] = ir[0] + code % 7 - 3; jr[1] = ir[1] + code / 7 - 3;
            if (jr[0] >= 0 && jr[0] < n0r && jr[1] >= 0 && jr[1] < n1r) {
                const int ii = ir[g.perm[0]] * g.colstride[0] + ir[g.perm[1]] * g.colstride[1];
                const int jj = jr[g.perm[0]] * g.colstride[0] + jr[g.perm[1]] * g.colstride[1];
                const int hi = ii > jj ? ii : jj, lo = ii > jj ? jj : ii;
                v = L.band[(long long)hi * ld + (hi - lo)];
            }
        }
        cov[e] = (T)v;
    }
}

// One problem from its points (the np points from p0 on of xd, yd and, where `weighted`, wd) to its coefficients: zeroing,
// phases 1 to 5, and the store of the ncol coefficients (0 where the fit failed) to `out` in the caller's node order.  Every
// thread of the workgroup calls it; L.x keeps the coefficients in the internal order, and L.rho and the stage are free on return.
// COV (off in fit_many_kernel and fit_many_clip_kernel, whose code it does not touch): phase 6 after the store, into `cov`.
template <int D, typename T, int NT, typename WP, bool COV = false>
__device__ inline FitOutcome fit_problem(const FitManyArgs &a, const Lds &L, const T *__restrict__ xd, const T *__restrict__ yd, WP wd,
                                         bool weighted, long long p0, long long np, T *__restrict__ out, T *__restrict__ cov = nullptr)
{
    const Grid &g = a.g;
    const int tid = threadIdx.x, n = a.sh.ncol, ld = a.sh.ld, hb = a.sh.hb;
    const bool sparse_rule = a.xtrap != 0.0;
    __syncthreads();
    for (long long e = tid; e < (long long)n * ld; e += NT) L.band[e] = 0.0;
    for (int i = tid; i < n; i += NT) { L.rhs[i] = 0.0; L.dcw[i] = 0.0; L.spf[i] = 0; }
    __syncthreads();

    // 1 assemble
    int nrows = 0;
    double tot = 0.0, unused = 0.0;
    for (long long c0 = 0; c0 < np; c0 += FITMANY_CHUNK) {
        const int cnt = (int)(np - c0 < FITMANY_CHUNK ? np - c0 : FITMANY_CHUNK);
        stage_chunk<D, T, false, NT, WP>(a, L, xd, yd, wd, weighted, p0 + c0, cnt, nrows, unused);
        __syncthreads();
        owner_chunk<D, false, NT>(a, L, cnt, tot);
        __syncthreads();
    }
    FitOutcome o;
    o.rows = block_reduce<false, NT>((double)nrows, L.stage);

    // 2 the data-sparse nodes and their constraint rows (:862-1046)
    o.crows = 0.0;
    if (sparse_rule) {
        if (tid == 0) L.scal[0] = tot;
        __syncthreads();
        const double totlwt = L.scal[0];
        int nsparse = 0;
        for (int i = tid; i < n; i += NT) {
#pragma clang fp contract(off)
            int in[D];
            node_of<D>(g, i, in);
            long long nrect = 1;
            int refnode = 0;
#pragma unroll
            for (int d = 0; d < D; ++d) { nrect *= (g.nodes[d] - 1); refnode += in[d] * g.refstride[d]; }
            double expect = totlwt / (double)nrect;                          // :910
#pragma unroll
            for (int d = 0; d < D; ++d)
                if (in[d] == 0 || in[d] == g.nodes[d] - 1) expect = 0.5 * expect;      // :928
            const double have = L.dcw[refnode];
            const bool sp = have < 0.75 * expect;                            // :696, :936
            L.rho[i] = sp ? a.xtrap * (expect - have) : 0.0;                 // :938, :960
            L.spf[i] = sp ? 1 : 0;
            nsparse += sp ? 1 : 0;
        }
        __syncthreads();
        for (int i = tid; i < n; i += NT) L.dcw[i] = L.rho[i];
        __syncthreads();
        constraint_rows<D, false, NT>(a, L, unused);
        o.crows = block_reduce<false, NT>((double)nsparse, L.stage) * (double)(D * (D + 1) / 2);
    }
    __syncthreads();

    // 3 factor
    o.minpiv = INFINITY;
    bool ok = true;
    for (int j = 0; j < n; ++j) {
        const double piv = L.band[(long long)j * ld];
        ok = piv > 0.0;                          // (false for a NaN)
        if (!(o.minpiv <= piv)) o.minpiv = piv;
        if (!ok) break;                          // the same in every thread
        const double l = sqrt(piv);
        const int m = hb < n - 1 - j ? hb : n - 1 - j;
        for (int t = tid; t < m; t += NT) L.band[(long long)(j + 1 + t) * ld + (t + 1)] /= l;
        __syncthreads();
        if (tid == 0) L.band[(long long)j * ld] = l;
        for (int e = tid; e < m * m; e += NT) {
            const int ra = e / m + 1, rb = e % m + 1;      // rows j + ra >= j + rb
            if (rb <= ra)
                L.band[(long long)(j + ra) * ld + (ra - rb)] -= L.band[(long long)(j + ra) * ld + ra] * L.band[(long long)(j + rb) * ld + rb];
        }
        __syncthreads();
    }

    // 4 solve, 5 refine
    o.ssq = 0.0;
    o.fail = !ok;
    if (ok) {
        for (int i = tid; i < n; i += NT) L.x[i] = L.rhs[i];
        band_solve<D>(L, a.sh, L.x);
        for (int it = 0; it < FITMANY_MAX_STEPS; ++it) {
            for (int i = tid; i < n; i += NT) L.rho[i] = 0.0;
            __syncthreads();
            double ssqp = 0.0;
            int nr = 0;
            for (long long c0 = 0; c0 < np; c0 += FITMANY_CHUNK) {
                const int cnt = (int)(np - c0 < FITMANY_CHUNK ? np - c0 : FITMANY_CHUNK);
                stage_chunk<D, T, true, NT, WP>(a, L, xd, yd, wd, weighted, p0 + c0, cnt, nr, ssqp);
                __syncthreads();
                owner_chunk<D, true, NT>(a, L, cnt, unused);
                __syncthreads();
            }
            if (sparse_rule) constraint_rows<D, true, NT>(a, L, ssqp);
            o.ssq = block_reduce<false, NT>(ssqp, L.stage);
            band_solve<D>(L, a.sh, L.rho);
            double m0 = 0.0, m1 = 0.0;
            for (int i = tid; i < n; i += NT) {
                const double dx = L.rho[i], xn = L.x[i] + dx;
                L.x[i] = xn;
                m0 = nanmax(m0, fabs(dx));
                m1 = nanmax(m1, fabs(xn));
            }
            double am[2];
            am[0] = block_reduce<true, NT>(m0, L.stage);
            am[1] = block_reduce<true, NT>(m1, L.stage);
            if (o.rule.advance(it, am)) break;
        }
        o.fail = !o.rule.converged && !(o.rule.estimate() <= 1e-10);
    }

    for (int i = tid; i < n; i += NT) {
        int in[D], refnode = 0;
        node_of<D>(g, i, in);
#pragma unroll
        for (int d = 0; d < D; ++d) refnode += in[d] * g.refstride[d];
        out[refnode] = o.fail ? (T)0 : (T)L.x[i];
    }
    if constexpr (COV) selected_inverse<D, T, NT>(a, L, o.fail, cov);
    return o;
}

}  // namespace fitmanydev
}  // namespace splpak
