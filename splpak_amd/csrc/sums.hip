// Sums of a vector in a fixed order, by one workgroup: the histogram's total at the end of the Gram stage (gram.hip) and the
// sum of squared row residuals at the end of a residual pass (residual.hip).  No floating-point atomics: thread t adds the
// entries t, t + 1024, .., then a tree over the threads -- the same bits from run to run.
#include "kernels.hpp"

namespace splpak {

namespace {

// sum of v[t], v[t + nt], v[t + 2 nt], .. below n, eight loads in flight (eight partial sums, combined in a fixed order):
// the single-workgroup reductions below were bound by one dependent load + add per element (round 3)
__device__ inline double strided_sum8(const double *__restrict__ v, long long n, int t, int nt)
{
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    long long i = t;
    for (; i + 7LL * nt < n; i += 8LL * nt) {
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] += v[i + (long long)u * nt];
    }
    for (int u = 0; i < n; i += nt, ++u) a[u] += v[i];
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

// totlwt (:906) = the sum of the histogram (every counted point is in it), in a fixed order
__global__ void __launch_bounds__(1024)
hist_total_kernel(const double *__restrict__ hist, int n, double *__restrict__ scal)
{
    __shared__ double part[1024];
    const int t = threadIdx.x;
    const double s = strided_sum8(hist, n, t, 1024);
    part[t] = s;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (t < o) part[t] += part[t + o];
        __syncthreads();
    }
    if (t == 0) scal[SC_TOTLWT] = part[0];
}

}  // namespace

// out[0] = sum of v[0 .. n) in a fixed order: thread t sums the entries t, t + 1024, ..; then a tree over the threads
__global__ void __launch_bounds__(1024)
sum_fixed_kernel(const double *__restrict__ v, long long n, double *__restrict__ out)
{
    __shared__ double red[1024];
    red[threadIdx.x] = strided_sum8(v, n, (int)threadIdx.x, 1024);
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

hipError_t launch_hist_total(const Grid &g, const double *hist, double *scal, hipStream_t st)
{
    hipLaunchKernelGGL(hist_total_kernel, dim3(1), dim3(1024), 0, st, hist, g.ncol, scal);
    return hipGetLastError();
}

hipError_t launch_sum_fixed(const double *v, long long n, double *out, hipStream_t st)
{
    hipLaunchKernelGGL(sum_fixed_kernel, dim3(1), dim3(1024), 0, st, v, n, out);
    return hipGetLastError();
}

}  // namespace splpak
