// The vector kernels of a conjugate-gradient iteration whose scalars stay on the device (pcg.hip: the point fit's
// iteration; fitgridw.hip: the weighted grid fit's): fixed-order dot products in two steps, the two updates, the slots of
// the scalars.  Internal linkage: every file that includes this compiles kernels of its own.
#pragma once
#include "common.hpp"

namespace splpak {

namespace {

constexpr int DOT_BLOCKS = 512;

// partial[b] = sum over block b's contiguous chunk of a[i] * b[i] (fixed order: reproducible)
__global__ void __launch_bounds__(256)
dot_partial_kernel(long long n, const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ partial)
{
    __shared__ double red[256];
    const long long chunk = (n + gridDim.x - 1) / gridDim.x;
    const long long beg = (long long)blockIdx.x * chunk, end = beg + chunk < n ? beg + chunk : n;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    long long i = beg + threadIdx.x;
    for (; i + 768 < end; i += 1024) {
        s0 = fma(a[i], b[i], s0);
        s1 = fma(a[i + 256], b[i + 256], s1);
        s2 = fma(a[i + 512], b[i + 512], s2);
        s3 = fma(a[i + 768], b[i + 768], s3);
    }
    for (; i < end; i += 256) s0 = fma(a[i], b[i], s0);
    red[threadIdx.x] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// sc[slot] = sign * sum(partial); hist != NULL: also hist[0] = that value
__global__ void __launch_bounds__(DOT_BLOCKS)
dot_finish_kernel(const double *__restrict__ partial, double sign, double *__restrict__ sc, int slot, double *__restrict__ hist)
{
    __shared__ double red[DOT_BLOCKS];
    red[threadIdx.x] = partial[threadIdx.x];
    __syncthreads();
    for (int o = DOT_BLOCKS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double v = sign * red[0];
        sc[slot] = v;
        if (hist) hist[0] = v;
    }
}

enum { S_RZ = 0, S_PQ = 1, S_RZNEW = 2, S_COUNT = 8 };

// alpha = rz / pq;  x += alpha p;  r += alpha nq   (nq = -N p, the residual pass's sign)
__global__ void __launch_bounds__(256)
update_xr_kernel(long long n, const double *__restrict__ sc, double *__restrict__ x, double *__restrict__ r,
                 const double *__restrict__ pv, const double *__restrict__ nq)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double pq = sc[S_PQ];
    const double alpha = pq > 0.0 ? sc[S_RZ] / pq : 0.0;
    x[i] = fma(alpha, pv[i], x[i]);
    r[i] = fma(alpha, nq[i], r[i]);
}

// beta = rz_new / rz;  p = z + beta p
__global__ void __launch_bounds__(256)
update_p_kernel(long long n, const double *__restrict__ sc, double *__restrict__ pv, const double *__restrict__ z)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double rz = sc[S_RZ];
    const double beta = rz > 0.0 ? sc[S_RZNEW] / rz : 0.0;
    pv[i] = fma(beta, pv[i], z[i]);
}

__global__ void advance_kernel(double *__restrict__ sc) { sc[S_RZ] = sc[S_RZNEW]; }

}  // namespace

}  // namespace splpak
