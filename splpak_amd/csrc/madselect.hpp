// The exact median of a problem's counted values on the LDS of its workgroup: what splpak_mad_many_* (madmany.hip) and the
// robust clipping loop (fitmanymad.hip) share.  include/splpak_hip.h (splpak_mad_many_*) states the definitions.
//
// A double is mapped to a 64-bit key whose unsigned order is the order of the doubles (median_key; -0 has become +0 before).
// The key of rank r is found most significant byte first: 8 sweeps over the problem's values, each counting the byte below
// the prefix found so far into a 256-bin histogram of integers in LDS (LDS atomic adds: a count does not depend on the order
// of its additions); wave 0 then scans the histogram -- four bins per lane, a shuffle scan over the lanes -- and publishes the
// bin that holds the rank, the rank inside it and the bin's count.  After the last byte the bin holds the copies of ONE key,
// so for an even count the upper middle is the same key when the bin holds a further copy, and otherwise the smallest key
// above it: one more sweep with an LDS integer minimum.  The result is an order statistic of the multiset: nothing of it
// depends on which thread saw which value.  No floating-point atomics.
//
// LDS: MEDIAN_LDS_WORDS 4-byte words at an 8-byte boundary (the fused kernel lends the head of its stage area).
#pragma once
#include "common.hpp"

namespace splpak {
namespace madselect {

constexpr int MEDIAN_LDS_WORDS = 264;      // 256 bins, the three published words, one spare, a 64-bit minimum

// ascending doubles (no NaN) <-> ascending unsigned keys
__device__ inline unsigned long long median_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__device__ inline double median_value(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k;
    return __longlong_as_double((long long)b);
}

// The key of rank r (0-based, r < the number of counted values) among the values p = 0 .. np-1 for which key_at(p, key) is
// true, in every thread of the workgroup of NT threads; *above = the counted copies of that key beyond rank r.
template <int NT, typename F>
__device__ inline unsigned long long select_rank(unsigned *lds, long long np, unsigned r, F &&key_at, unsigned *above)
{
    const int tid = threadIdx.x;
    unsigned long long prefix = 0;
    unsigned eq = 0;
    for (int b = 7; b >= 0; --b) {
        const int sh = 8 * b;
        __syncthreads();
        for (int i = tid; i < 256; i += NT) lds[i] = 0;
        __syncthreads();
        for (long long p = tid; p < np; p += NT) {
            unsigned long long k;
            if (key_at(p, k) && (b == 7 || (k >> (sh + 8)) == prefix)) atomicAdd(&lds[(unsigned)(k >> sh) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {
            unsigned c[4], sum = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { c[q] = lds[4 * tid + q]; sum += c[q]; }
            unsigned incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned up = __shfl_up(incl, o, 64);
                if (tid >= o) incl += up;
            }
            unsigned before = incl - sum;
            if (before <= r && r < incl) {      // one lane
                int q = 0;
                while (r >= before + c[q]) { before += c[q]; ++q; }      // (q < 4: r < incl)
                lds[256] = (unsigned)(4 * tid + q);
                lds[257] = r - before;
                lds[258] = c[q];
            }
        }
        __syncthreads();
        prefix = (prefix << 8) | lds[256];
        r = lds[257];
        eq = lds[258];
    }
    *above = eq - 1 - r;
    return prefix;
}

// The median of the cnt >= 1 counted values, numpy.median's bits: the middle one for odd cnt, else half the sum of the two
// middle ones (one addition, one multiplication by 0.5, each rounded on its own).  The same in every thread.
template <int NT, typename F>
__device__ inline double select_median(unsigned *lds, long long np, unsigned cnt, F &&key_at)
{
#pragma clang fp contract(off)
    unsigned above = 0;
    const unsigned long long k1 = select_rank<NT>(lds, np, (cnt - 1) / 2, key_at, &above);
    if (cnt & 1u) return median_value(k1);
    unsigned long long k2 = k1;
    if (above == 0) {      // the upper middle is the smallest key above k1 (there is one: rank cnt/2 exists)
        unsigned long long *mn = reinterpret_cast<unsigned long long *>(lds + 260);
        __syncthreads();
        if (threadIdx.x == 0) *mn = ~0ULL;
        __syncthreads();
        unsigned long long mine = ~0ULL;
        for (long long p = threadIdx.x; p < np; p += NT) {
            unsigned long long k;
            if (key_at(p, k) && k > k1 && k < mine) mine = k;
        }
        if (mine != ~0ULL) atomicMin(mn, mine);
        __syncthreads();
        k2 = *mn;
    }
    const double sum = median_value(k1) + median_value(k2);
    return 0.5 * sum;
}

}  // namespace madselect
}  // namespace splpak
