// What the LDS-tile kernels of the sorted evaluation paths share (evalsort.hip, evalruns.hip, evalregion.hip): the
// coefficient tile of a region and its LDS strides, the regions of a grid, the records the sort passes write, and the
// device helpers that place, fill and read a tile.  One definition each, so that a change of tile shape or of the way a
// window row is read is made once.  The arithmetic per query stays eval_table + window_sum (evalcore.hpp): identical bits
// on every path.
#pragma once
#include "basis.hpp"
#include "evalcore.hpp"
#include <type_traits>

namespace splpak {

// The tile of a region of the region sort and the run path: a box of window starts whose coefficients (box + 3 nodes per
// dimension, 4096 doubles = 32 KB) fit in LDS.
template <int D> struct TileShape;
template <> struct TileShape<2> { static constexpr int T[4] = {64, 64, 1, 1}; };
template <> struct TileShape<3> { static constexpr int T[4] = {16, 16, 16, 1}; };
// 4-D: 8 x 8 x 8 x 16 coefficients (64 KB) serve 5 x 5 x 5 x 13 window starts -- 648 regions at 32^4 instead of the 1 296 of an
// 8^4 tile (round 3): half the bins in the sort passes, 2.6 x the window starts per tile fill
template <> struct TileShape<4> { static constexpr int T[4] = {8, 8, 8, 16}; };
// LDS strides of the tile dimensions.  4-D: padded (8 -> 67 -> 539 instead of 64 -> 512) so that the tile offset of a window
// start, taken mod 32 doubles = its LDS bank class for ds_read_b64, is uniform over the 5 x 5 x 5 x 13 starts of a region (50-52
// per class; the dense strides give 20 classes, five of them double: SQ_LDS_BANK_CONFLICT was 80 % of SQ_LDS_IDX_ACTIVE and
// the LDS pipe 90 % of the evaluation pass, round 3).  The evaluation pass then deals its queries to the lanes BY CLASS
// (eval_binned_kernel), which makes every window read conflict free.
template <int D> struct TileStride { static constexpr int S[4] = {1, TileShape<D>::T[0], TileShape<D>::T[0] * TileShape<D>::T[1],
                                                                  TileShape<D>::T[0] * TileShape<D>::T[1] * TileShape<D>::T[2]}; };
template <> struct TileStride<4> { static constexpr int S[4] = {1, 8, 67, 539}; };
template <> struct TileStride<3> { static constexpr int S[4] = {1, 17, 274, 274 * 16}; };     // 13^3 starts: 67-70 per class (dense: 26 classes)
template <int D> constexpr int tile_elems() { return TileStride<D>::S[D - 1] * TileShape<D>::T[D - 1]; }
template <int D> constexpr int tile_cells() { return TileShape<D>::T[0] * TileShape<D>::T[1] * TileShape<D>::T[2] * TileShape<D>::T[3]; }
constexpr int EVAL_QPW = 2048;         // queries per workgroup in pass C
constexpr int EVAL_WG = 1024;          // threads per workgroup in pass C (value path): 16 waves share one 32 KB tile (A/B: 256 -> 512 threads +3 %, 1024 +5 %)

struct Regions { int nreg[MAXD]; int nbins; };

// A sorted query is ONE record of D + 1 doubles: its coordinates and, in the low half of the last word, its position in the
// caller's batch (round 3: coordinate planes + a separate permutation made pass B issue D + 1 scattered 8-byte stores per
// query -- 99 B of HBM writes for the 36-byte payload of a 4-D query, runs of 1.6 queries per workgroup and region; a record
// is one 32- / 40-byte store and one load in pass C).
typedef double rec2u_t __attribute__((ext_vector_type(2), aligned(8)));     // 40-byte records: 8-byte aligned pieces
typedef double rec2a_t __attribute__((ext_vector_type(2), aligned(16)));    // 32-byte records: aligned 16-byte pieces
template <int D>
__device__ inline void store_record(double *__restrict__ dst, const double (&x)[D], int idx)
{
    using rec2_t = typename std::conditional<(D + 1) % 2 == 0, rec2a_t, rec2u_t>::type;
    double v[D + 1];
#pragma unroll
    for (int d = 0; d < D; ++d) v[d] = x[d];
    v[D] = __longlong_as_double((long long)idx);
    constexpr int N = D + 1;
#pragma unroll
    for (int k = 0; k + 1 < N; k += 2) {
        rec2_t t;
        t[0] = v[k]; t[1] = v[k + 1];
        *reinterpret_cast<rec2_t *>(dst + k) = t;
    }
    if constexpr (N % 2 == 1) dst[N - 1] = v[N - 1];
}
template <int D>
__device__ inline int load_record(const double *__restrict__ src, double (&x)[D])
{
    constexpr int N = D + 1;
    using rec2_t = typename std::conditional<(D + 1) % 2 == 0, rec2a_t, rec2u_t>::type;
    double v[N];
#pragma unroll
    for (int k = 0; k + 1 < N; k += 2) {
        const rec2_t t = *reinterpret_cast<const rec2_t *>(src + k);
        v[k] = t[0]; v[k + 1] = t[1];
    }
    if constexpr (N % 2 == 1) v[N - 1] = src[N - 1];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = v[d];
    return (int)__double_as_longlong(v[D]);
}

template <int D>
__device__ inline int region_of(const Grid &g, const Regions &rg, const double *__restrict__ x)
{
    int r = 0, m = 1;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        int lo, hi;
        const int ws = window_start(g, d, x[d], lo, hi);
        r += (ws / (TileShape<D>::T[d] - 3)) * m;
        m *= rg.nreg[d];
    }
    return r;
}

// The four coefficients of a window row from a tile in LDS: four ds_read_b64 (2 LDS cycles each, 64 banks) instead of the
// two ds_read2_b64 the compiler would merge them into (8 cycles each, 32 banks) -- volatile keeps them apart.
__device__ __forceinline__ void lds_row4(const double *tile, int offset, double (&c)[4])
{
    typedef const volatile __attribute__((address_space(3))) double *lds_cvd;
    lds_cvd q = (lds_cvd)tile + offset;
    c[0] = q[0]; c[1] = q[1]; c[2] = q[2]; c[3] = q[3];
}

// The origin of a region's tile, the tile fill and the evaluation of a query from the tile stay written out in the five
// kernels (eval_binned_kernel is the commented copy): as __forceinline__ helpers -- regions by reference, by value, through
// accessors -- each changed the instruction streams of all of them, and eval_binned_kernel<4> sits at exactly 64 registers.
}  // namespace splpak
