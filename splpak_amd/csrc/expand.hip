// Leaving the assembly: the half stencil of the normal equations into the band storage of the Cholesky factorisation
// (expand_kernel, then pad_diag_kernel: 1 on the diagonal of the padding), and the solution from the plan's internal
// dimension order into the caller's (to_reference_order_kernel).
#include "assemble_dev.hpp"

namespace splpak {

namespace {

template <int D>
__global__ void __launch_bounds__(256)
expand_kernel(Grid g, const double *__restrict__ nst, double *__restrict__ ab, long long lda, DistMap dm)
{
    const long long total = (long long)g.ncol * g.hstencil;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int i = (int)(t / g.hstencil);
        int code = (int)(t % g.hstencil);
        int j = i;
        bool ok = true;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int o = (code % 7) - 3;
            code /= 7;
            const int id = (i / g.colstride[d]) % g.nodes[d];
            const int jd = id + o;
            if (jd < 0 || jd > g.nodes[d] - 1) ok = false;
            j += o * g.colstride[d];
        }
        if (!ok) continue;
        const int J = j / NBLK;                 // block column of the entry: stored here only if this rank owns it
        if (!dm_owned(dm, J)) continue;
        ab[dm_shift(dm, J) + (long long)i + (long long)j * lda] = nst[t];
    }
}

__global__ void pad_diag_kernel(double *ab, long long lda, int n, int npad, DistMap dm)
{
    const int i = n + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < npad && dm_owned(dm, i / NBLK)) ab[dm_shift(dm, i / NBLK) + (long long)i + (long long)i * lda] = 1.0;
}

}  // namespace

__global__ void __launch_bounds__(256)
to_reference_order_kernel(Grid g, const double *__restrict__ xvec, double *__restrict__ coef)
{
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= g.ncol) return;
    int ref = 0;
    for (int d = 0; d < g.ndim; ++d) ref += ((col / g.colstride[d]) % g.nodes[d]) * g.refstride[d];
    coef[ref] = xvec[col];
}

hipError_t launch_to_reference_order(const Grid &g, const double *xvec, double *coef, hipStream_t st)
{
    bool identity = true;
    for (int d = 0; d < g.ndim; ++d) identity = identity && g.perm[d] == d;
    if (identity) return hipMemcpyAsync(coef, xvec, sizeof(double) * (size_t)g.ncol, hipMemcpyDeviceToDevice, st);
    hipLaunchKernelGGL(to_reference_order_kernel, dim3((g.ncol + 255) / 256), dim3(256), 0, st, g, xvec, coef);
    return hipGetLastError();
}

hipError_t launch_expand(const Grid &g, const double *nst, const Band &b, const DistMap &dm, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(b.ab, 0, b.bytes, st);
    if (e != hipSuccess) return e;
    const long long total = (long long)g.ncol * g.hstencil;
    dim3 gr(grid_for(total, 256, 256LL * 64)), bl(256);
    DISPATCH_D(g.ndim, hipLaunchKernelGGL(expand_kernel<D>, gr, bl, 0, st, g, nst, b.ab, b.lda, dm));
    if (b.npad > b.n)
        hipLaunchKernelGGL(pad_diag_kernel, dim3((b.npad - b.n + 255) / 256), dim3(256), 0, st, b.ab,
                           b.lda, b.n, b.npad, dm);
    return hipGetLastError();
}

}  // namespace splpak
