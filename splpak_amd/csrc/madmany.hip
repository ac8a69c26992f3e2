// The median and the MAD of every problem's segment in one launch: splpak_mad_many_* (include/splpak_hip.h states the
// definitions; the entries: evalmanyapi.hip).  In the evalmany.hip family: one wave per problem, the waves stride over the
// problems, as residuals_many_kernel.  The wave counts its problem's selected values, then runs the selection of madselect.hpp
// twice on the caller's array -- on the keys of (double) v + 0.0, and on those of |k - med| formed on the fly -- with the
// histogram in 1 KB of LDS.  Nothing is written but stats, and no scratch is used.  The result is an order statistic of the
// multiset of the counted values: it does not depend on the batch, the position, the wave or the order of the values.
#include "evalmany.hpp"
#include "madselect.hpp"

namespace splpak {

namespace {

using namespace madselect;

// every operation below is rounded on its own
#pragma clang fp contract(off)

template <typename T>
__global__ void __launch_bounds__(64)
mad_many_kernel(int nbatch, const long long *__restrict__ offsets, long long base, const T *__restrict__ values, const T *__restrict__ wsel,
                double *__restrict__ stats)
{
    __shared__ unsigned long long sel64[MEDIAN_LDS_WORDS / 2];
    unsigned *sel = reinterpret_cast<unsigned *>(sel64);
    const int lane = threadIdx.x;
    for (int k = blockIdx.x; k < nbatch; k += gridDim.x) {
        const long long p0 = offsets[k] - base, np = offsets[k + 1] - offsets[k];
        const T *v = values + p0, *w = wsel ? wsel + p0 : nullptr;
        unsigned cnt = 0;
        if (w) {
            for (long long p = lane; p < np; p += 64) cnt += (double)w[p] != 0.0 ? 1u : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        } else {
            cnt = (unsigned)np;
        }
        double med = 0.0, mad = 0.0;
        if (cnt > 0) {      // (the same in every lane)
            med = select_median<64>(sel, np, cnt, [&](long long p, unsigned long long &key) {
                if (w && (double)w[p] == 0.0) return false;
                key = median_key((double)v[p] + 0.0);
                return true;
            });
            mad = select_median<64>(sel, np, cnt, [&](long long p, unsigned long long &key) {
                if (w && (double)w[p] == 0.0) return false;
                const double kv = (double)v[p] + 0.0;
                key = median_key(fabs(kv - med));
                return true;
            });
        }
        if (lane == 0) {
            double *sk = stats + 4LL * k;
            sk[0] = (double)cnt;
            sk[1] = med;
            sk[2] = mad;
            sk[3] = 0.0;
        }
    }
}

}  // namespace

template <typename T>
hipError_t launch_mad_many(int nbatch, const long long *offsets_dev, long long base, const T *values, const T *wsel, double *stats,
                           hipStream_t st)
{
    if (nbatch < 1) return hipSuccess;
    const int blocks = nbatch < RESMANY_WAVES ? nbatch : RESMANY_WAVES;      // the waves stride over the rest
    hipLaunchKernelGGL((mad_many_kernel<T>), dim3((unsigned)blocks), dim3(64), 0, st, nbatch, offsets_dev, base, values, wsel, stats);
    t_eval_many_stats[0] = blocks;
    t_eval_many_stats[1] = 1;
    return hipGetLastError();
}
template hipError_t launch_mad_many<double>(int, const long long *, long long, const double *, const double *, double *, hipStream_t);
template hipError_t launch_mad_many<float>(int, const long long *, long long, const float *, const float *, double *, hipStream_t);

}  // namespace splpak
