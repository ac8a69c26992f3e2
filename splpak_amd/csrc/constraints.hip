// Derivative-constraint rows (:921-1046).  A data-sparse node n (histogram below spcrit = 0.75 of the
// expected weight, :936) emits D(D+1)/2 rows, one per pair idm <= jdm, whose entries sit on the 3^D
// nodes around n:  row(n, pair)[j] = rowwt * prod_d bas1(nderiv_d; x_n; node j).  (The pattern, the factors and the
// entries themselves: assemble_dev.hpp -- the refinement residual applies the same rows.)
//
// No floating-point atomics: every stencil row has ONE owner, which adds the contributions of its sparse neighbours in a
// fixed order.
//
//   (once per plan: constraint_table_kernel, the per-dimension factors of the entries -- in gram.hip, see there)
// per fit, in launch order
//   sparse_mark_kernel       which nodes are data sparse, and their constraint weight (:923-960)
//   constraint_rows_kernel   nst += C^T C, gathered per stencil row from the <= 3^d sparse neighbours
//   count_sparse_kernel      the number of constraint rows -> scal_out[SC_NROWS_CONS]
#include "assemble_dev.hpp"

namespace splpak {

namespace {

template <int D>
__device__ inline SparseNode sparse_node(const Grid &g, const int *in, const double *__restrict__ hist,
                                         double totlwt, double xtrap)
{
#pragma clang fp contract(off)
    long long nrect = 1;
#pragma unroll
    for (int d = 0; d < D; ++d) nrect *= (g.nodes[d] - 1);
    const double wtprrc = totlwt / (double)nrect;                 // :910
    double expect = wtprrc;
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (in[d] == 0 || in[d] == g.nodes[d] - 1) expect = 0.5 * expect;     // :928
    int refnode = 0;                                              // the histogram is in the caller's order
#pragma unroll
    for (int d = 0; d < D; ++d) refnode += in[d] * g.refstride[d];
    const double have = hist[refnode];
    SparseNode s;
    s.sparse = have < 0.75 * expect;                              // spcrit, :696, :936
    s.dcwght = xtrap * (expect - have);                           // :938, :960
    return s;
}


// Pre-pass: which nodes are data sparse, and their constraint weight -- once per fit (the histogram is
// final), so that the row gathers below look a neighbour up with one byte instead of re-deriving it
template <int D>
__global__ void __launch_bounds__(256)
sparse_mark_kernel(Grid g, const double *__restrict__ hist, const double *__restrict__ scal, double xtrap,
                   double *__restrict__ dcw, unsigned char *__restrict__ spf)
{
    const int node = blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= g.ncol) return;
    int in[D];
#pragma unroll
    for (int d = 0; d < D; ++d) in[d] = (node / g.colstride[d]) % g.nodes[d];
    const SparseNode sn = sparse_node<D>(g, in, hist, scal[SC_TOTLWT], xtrap);
    dcw[node] = sn.dcwght;
    spf[node] = sn.sparse ? 1 : 0;
}

// rows of the constraint system: ndim (ndim + 1) / 2 per data-sparse node (:974-1000) -> scal_out[SC_NROWS_CONS]
__global__ void __launch_bounds__(1024)
count_sparse_kernel(const unsigned char *__restrict__ spf, int ncol, int rows_per_node, double *__restrict__ scal_out)
{
    __shared__ int red[16];
    int c = 0;
    for (int i = threadIdx.x; i < ncol; i += 1024) c += spf[i] != 0 ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int v = 0; v < 16; ++v) t += red[v];
        scal_out[SC_NROWS_CONS] += (double)t * (double)rows_per_node;
    }
}

// One wave per stencil row i: nst[i][code(j - i)] += sum over the sparse nodes n within one node of
// both i and j, and over n's rows, of row[i] * row[j] -- neighbours and rows in a fixed order, the
// row's owner adds with plain read-modify-writes.  Also counts the rows (scal_out[SC_NROWS_CONS]).
template <int D>
__global__ void __launch_bounds__(256)
constraint_rows_kernel(Grid g, const double *__restrict__ dcw, const unsigned char *__restrict__ spf, const double *__restrict__ ctab,
                       double *__restrict__ nst, double *__restrict__ scal_out)
{
    constexpr int NE = (D == 1) ? 3 : (D == 2) ? 9 : (D == 3) ? 27 : 81;
    constexpr int HS = (D == 1) ? 4 : (D == 2) ? 25 : (D == 3) ? 172 : 1201;
    __shared__ double sacc[4][HS];
    __shared__ double sct[4][D * 27], sdn[4][NE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int node = blockIdx.x * 4 + wave;
    if (node >= g.ncol) return;
    double *acc = sacc[wave];
    int in[D];
#pragma unroll
    for (int d = 0; d < D; ++d) in[d] = (node / g.colstride[d]) % g.nodes[d];
    // lanes look the 3^D neighbours up in parallel: sparse[r] = which of the neighbours 64 r .. 64 r + 63 are data sparse.  Most
    // rows of a well-covered grid leave here; the others walk the SET bits only (the walk used to re-read the flag of every
    // neighbour, one dependent load after the other: 27 of them for 1.6 sparse neighbours at C3)
    unsigned long long sparse[(NE + 63) / 64];
#pragma unroll
    for (int r = 0; r < (NE + 63) / 64; ++r) {
        const int ne = lane + 64 * r;
        bool mine = false;
        if (ne < NE) {
            int t = ne, col = 0;
            bool ok = true;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int nd_ = in[d] + t % 3 - 1;
                t /= 3;
                ok = ok && nd_ >= 0 && nd_ <= g.nodes[d] - 1;
                col += nd_ * g.colstride[d];
            }
            mine = ok && spf[col] != 0;
        }
        sparse[r] = __builtin_amdgcn_ballot_w64(mine);
    }
    {
        unsigned long long anyb = 0;
#pragma unroll
        for (int r = 0; r < (NE + 63) / 64; ++r) anyb |= sparse[r];
        if (anyb == 0) return;
    }
    for (int e = lane; e < HS; e += 64) acc[e] = 0.0;
    // The factors this row can meet -- nodes in[d] - 1 .. in[d] + 1 of every dimension, 27 D of them -- and the weights of the 3^D
    // neighbours go to LDS first: the walk below then multiplies LDS words instead of chasing three dependent table loads per
    // entry through L2 (round 5: 1.84 ms of a 9.7 ms assembly at 64^3 for 17 000 data-sparse nodes).  Same values, same order.
    double *ct = sct[wave], *dn = sdn[wave];
    {
        for (int e = lane; e < D * 27; e += 64) {
            const int d = e / 27, r = e % 27, n = in[d] + r / 9 - 1;
            int base = 0;
            for (int q = 0; q < d; ++q) base += 9 * g.nodes[q];
            double v = 0.0;
            if (n >= 0 && n <= g.nodes[d] - 1) v = ctab ? ctab[base + n * 9 + r % 9] : constraint_factor(g, d, n, (r % 9) / 3 - 1, r % 3);
            ct[e] = v;
        }
        for (int ne = lane; ne < NE; ne += 64) {
            int t = ne, col = 0;
#pragma unroll
            for (int d = 0; d < D; ++d) { col += (in[d] + t % 3 - 1) * g.colstride[d]; t /= 3; }
            dn[ne] = ((sparse[ne >> 6] >> (ne & 63)) & 1ull) ? dcw[col] : 0.0;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    // entry of the constraint row of node nn at nn + off, from the LDS copy (constraint_entry's product, factor by factor)
    auto entry = [&](const int *nn, const int *off, const int *nder, double rowwt) -> double {
#pragma clang fp contract(off)
        double basm = 1.0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int ib = nn[d] + off[d];
            if (ib < 0 || ib > g.nodes[d] - 1) return 0.0;
            basm *= ct[d * 27 + (nn[d] - in[d] + 1) * 9 + (off[d] + 1) * 3 + nder[d]];
        }
        return rowwt * basm;
    };
    bool any = false;
    for (int ne = 0; ne < NE; ++ne) {            // neighbour n = i + offn, offn_d in [-1,1], dim 0 fastest
        if (!((sparse[ne >> 6] >> (ne & 63)) & 1ull)) continue;        // (in the grid and data sparse)
        int nn[D], offi[D], t = ne;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int o = t % 3 - 1;
            t /= 3;
            nn[d] = in[d] + o;
            offi[d] = -o;                        // i = n + offi
        }
        SparseNode sn;
        sn.sparse = true;
        sn.dcwght = dn[ne];
        any = true;
        // (the rows are counted by count_sparse_kernel: one f64 atomicAdd per data-sparse node on ONE word -- a compare-and-swap
        //  loop on this build -- serialised 17 000 of them at config 3 and 177 000 at 4-D 28^4)
        for (int idm = 0; idm < D; ++idm)
            for (int jdm = idm; jdm < D; ++jdm) {
                int nder[D];
                const double rowwt = constraint_pattern<D>(g, nn, idm, jdm, sn.dcwght, nder);
                const double ci = entry(nn, offi, nder, rowwt);
                if (ci == 0.0) continue;         // wave-uniform
                for (int je = lane; je < NE; je += 64) {
                    int offj[D], tt = je, code = 0, m7 = 1;
                    bool lower = true, decided = false;
#pragma unroll
                    for (int d = 0; d < D; ++d) { offj[d] = tt % 3 - 1; tt /= 3; }
                    // column j = n + offj must not exceed row i = n + offi in the linear order
                    // (highest dimension most significant)
#pragma unroll
                    for (int d = D - 1; d >= 0; --d) {
                        if (!decided && offj[d] != offi[d]) { lower = offj[d] < offi[d]; decided = true; }
                    }
#pragma unroll
                    for (int d = 0; d < D; ++d) { code += (offj[d] - offi[d] + 3) * m7; m7 *= 7; }
                    if (!lower) continue;
                    const double cj = entry(nn, offj, nder, rowwt);
                    if (cj != 0.0) acc[code] += ci * cj;
                }
            }
    }
    if (!any) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    double *__restrict__ out = nst + (long long)node * g.hstencil;
    for (int e = lane; e < HS; e += 64)
        if (acc[e] != 0.0) out[e] += acc[e];
}

}  // namespace



hipError_t launch_sparse_mark(const Grid &g, const double *hist, const double *scal, double xtrap, double *dcw,
                              unsigned char *spf, hipStream_t st)
{
    DISPATCH_D(g.ndim, hipLaunchKernelGGL(sparse_mark_kernel<D>, dim3((unsigned)((g.ncol + 255) / 256)), dim3(256), 0, st,
                                          g, hist, scal, xtrap, dcw, spf));
    return hipGetLastError();
}

hipError_t launch_count_sparse(const Grid &g, const unsigned char *spf, double *scal_out, hipStream_t st)
{
    hipLaunchKernelGGL(count_sparse_kernel, dim3(1), dim3(1024), 0, st, spf, g.ncol, g.ndim * (g.ndim + 1) / 2, scal_out);
    return hipGetLastError();
}

hipError_t launch_constraint_rows(const Grid &g, const double *dcw, const unsigned char *spf, const double *ctab, double *nst,
                                  double *scal_out, hipStream_t st)
{
    dim3 gr((unsigned)((g.ncol + 3) / 4)), bl(256);
    DISPATCH_D(g.ndim, hipLaunchKernelGGL(constraint_rows_kernel<D>, gr, bl, 0, st, g, dcw, spf, ctab, nst, scal_out));
    return launch_count_sparse(g, spf, scal_out, st);
}

}  // namespace splpak
