// Many small independent fits on one node grid (include/splpak_hip.h: splpak_fit_many_* and the variants named after it):
// what every variant's file (fitmany*.hip: its kernel, its launch and its entries) shares with the host side of a call
// (fitmanyentry.hpp) and the device side of one fit (fitmanydev.hpp) -- the LDS map of a problem, the arguments and the result
// block of a kernel, the workgroup shapes and the one timed launch.
#pragma once
#include "common.hpp"
#include "../../include/splpak_hip.h"

#include <type_traits>

namespace splpak {

constexpr int FITMANY_THREADS = 256;            // threads of a workgroup: one workgroup per problem
constexpr int FITMANY_SMALL_NCOL = 64;          // grids of up to this many nodes run in workgroups of one wave (64 threads)
constexpr int FITMANY_CHUNK = 128;              // points staged in LDS at a time
constexpr int FITMANY_WALK = 8;                 // staged points whose words an owner reads together (divides FITMANY_CHUNK)
constexpr long long FITMANY_LDS_BUDGET = 65536; // bytes of LDS a workgroup may ask for (no launch of the library asks for more)
constexpr int FITMANY_MAX_STEPS = 30;           // refinement steps at the most (RefineRule decides earlier)

// The LDS of one workgroup, for a grid in the internal order (smaller dimension fastest), offsets in doubles from the start:
//   band    [ncol][hb + 1]   row i holds N(i, i - o) at o = 0 .. hb, later the Cholesky factor
//   rhs     [ncol]           A^T W^2 y
//   x       [ncol]           the coefficients
//   rho     [ncol]           the residual's gradient, then the correction
//   dcw     [ncol]           the nearest-node histogram (caller's node order), then the constraint weights (internal order)
//   stage   [CHUNK][4 D + 2] per staged point: D window tables, w, w y (or the row's residual); the reductions reuse it
//   scal    [16]
// then, in 4-byte words, ws [CHUNK][D] (window starts), addr [CHUNK] (histogram address) and ncol bytes of sparse flags.
struct FitManyShape {
    int ndim, ncol, hb, ld;                     // ld = hb + 1
    long long band, rhs, x, rho, dcw, stage, scal, doubles;
    long long bytes;
};

inline FitManyShape fit_many_shape(int ndim, const int *nodes)
{
    FitManyShape s{};
    s.ndim = ndim;
    int n0 = nodes[0], n1 = 1;
    if (ndim == 2) { n0 = nodes[0] < nodes[1] ? nodes[0] : nodes[1]; n1 = nodes[0] < nodes[1] ? nodes[1] : nodes[0]; }
    const long long ncol = (long long)n0 * n1;
    s.hb = ndim == 2 ? 3 * n0 + 3 : 3;
    s.ld = s.hb + 1;
    s.ncol = (int)(ncol < (1LL << 30) ? ncol : (1LL << 30));
    s.band = 0;
    s.rhs = ncol * s.ld;
    s.x = s.rhs + ncol;
    s.rho = s.x + ncol;
    s.dcw = s.rho + ncol;
    s.stage = s.dcw + ncol;
    s.scal = s.stage + (long long)FITMANY_CHUNK * (4 * ndim + 2);
    s.doubles = s.scal + 16;
    s.bytes = 8 * s.doubles + 4LL * FITMANY_CHUNK * (ndim + 1) + ((ncol + 3) / 4) * 4;
    return s;
}

// Words of one problem's `cov` (splpak_fit_many_cov_*): the half stencil of (7^ndim + 1) / 2 slots of every node
inline long long fit_many_cov_len(int ndim, long long ncol) { return ncol * (ndim == 2 ? 25 : 4); }

// What the kernel leaves per problem that ran (doubles).
enum { FM_ROWS = 0, FM_CROWS, FM_STEPS, FM_LASTREL, FM_MINPIV, FM_RESERR, FM_STATUS, FM_SPARE, FM_RESULT };

struct FitManyArgs {
    Grid g;                        // internal order (build_grid with reorder)
    FitManyShape sh;
    int nrun;                      // problems sent to the device
    const int *plist;              // [nrun] their numbers in the batch
    const long long *offsets;      // [nbatch + 1]
    long long base;                // point number of xdata[0] (the host entries upload the span of the batch alone)
    int l1xdat;
    double xtrap;
    long long ldcoef;
    int compact;                   // coef of run r at r * ldcoef (host entries) instead of plist[r] * ldcoef
    double *result;                // [nrun][FM_RESULT + what the variant's kernel adds]
};

extern thread_local long long t_fit_many_stats[8];

// workgroups of a batch launch: as many as fit on the device at once, or one per problem if that is fewer
template <typename K>
unsigned many_blocks(K kernel, int threads, size_t lds, int nrun, int cus)
{
    int occ = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, threads, lds) != hipSuccess || occ < 1) {
        (void)hipGetLastError();
        occ = 1;
    }
    const long long most = (long long)cus * occ;
    return (unsigned)(nrun < 1 ? 1 : ((long long)nrun < most ? (long long)nrun : most));
}

// one shape of a batch launch: many_blocks workgroups of NT threads with `lds` bytes each, on st
template <typename K, typename... A>
hipError_t many_launch(K kernel, int NT, size_t lds, int nrun, int cus, hipStream_t st, unsigned *blocks, A... args)
{
    *blocks = many_blocks(kernel, NT, lds, nrun, cus);
    hipLaunchKernelGGL(kernel, dim3(*blocks), dim3(NT), lds, st, args...);
    return hipGetLastError();
}

// The workgroup shapes of the batch kernels: f(dimension D, threads NT), both as integral constants.  A grid of at most
// FITMANY_SMALL_NCOL nodes has no work for more than one wave (a thread per band row): its workgroups are one wave, so that
// four times as many problems are in flight on a CU.  The shape depends on the grid alone.
template <typename F>
auto many_shape_ladder(const FitManyShape &sh, F &&f)
{
    using std::integral_constant;
    const bool small = sh.ncol <= FITMANY_SMALL_NCOL;
    if (sh.ndim == 1 && small) return f(integral_constant<int, 1>{}, integral_constant<int, 64>{});
    if (sh.ndim == 1) return f(integral_constant<int, 1>{}, integral_constant<int, FITMANY_THREADS>{});
    if (small) return f(integral_constant<int, 2>{}, integral_constant<int, 64>{});
    return f(integral_constant<int, 2>{}, integral_constant<int, FITMANY_THREADS>{});
}

// The one launch of a batch between two events: launch(cus, &blocks) enqueues it on st; st is synchronised once.  Fills
// t_fit_many_stats[0 .. 2] and *seconds (the launch's device time).  0 or SPLPAK_E_NODEVICE.
template <typename F>
int many_timed_launch(const FitManyShape &sh, hipStream_t st, double *seconds, F &&launch)
{
    int dev = 0;
    hipDeviceProp_t prop;
    SPLPAK_HIP_TRY(hipGetDevice(&dev), SPLPAK_E_NODEVICE);
    SPLPAK_HIP_TRY(hipGetDeviceProperties(&prop, dev), SPLPAK_E_NODEVICE);
    unsigned blocks = 1;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    SPLPAK_HIP_TRY(hipEventCreate(&e0), SPLPAK_E_NODEVICE);
    if (!hip_ok(hipEventCreate(&e1), "hipEventCreate")) { (void)hipEventDestroy(e0); return SPLPAK_E_NODEVICE; }
    hipError_t rc = hipEventRecord(e0, st);
    if (rc == hipSuccess) rc = launch(prop.multiProcessorCount, &blocks);
    if (rc == hipSuccess) rc = hipEventRecord(e1, st);
    if (rc == hipSuccess) rc = hipStreamSynchronize(st);
    float ms = 0.0f;
    if (rc == hipSuccess) rc = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (!hip_ok(rc, "the launch of the batch of fits")) return SPLPAK_E_NODEVICE;
    *seconds = (double)ms * 1e-3;
    t_fit_many_stats[0] = blocks;
    t_fit_many_stats[1] = (long long)sh.bytes;
    t_fit_many_stats[2] = 1;
    return 0;
}

}  // namespace splpak
