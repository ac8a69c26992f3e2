// Kernels of the nested-dissection multifrontal factorisation and of its tree solves (ndchol.hip, ndtop.hip), with one host
// launcher each: the drivers launch through these only.  Also the batched Cholesky of independent 256 x 256 blocks (pcg.hip).
#include "ndstate.hpp"
#include "chol_device.hpp"
#include <hip/hip_ext.h>
#include <cmath>
#include <type_traits>

namespace splpak {
namespace nd {

// job of the flat workgroup / item index `b`: first[j] <= b < first[j + 1] (first = the wg0 / item0 / tile0 field)
template <typename J, typename F>
__device__ __forceinline__ int find_job(const J *__restrict__ jobs, int njobs, int b, F &&first)
{
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first(jobs[mid]) <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Schur buffers come in two forms (round 5).  Square (lds > 0): element (r, c) at S[r + c lds].  PACKED (lds < 0, L = -lds =
// hp + 16): only the 64-column tile columns of the lower triangle, tile column c stored from its diagonal tile down with the
// leading dimension L - 64 c -- half the bytes; a tile is still an ordinary column-major 64 x 64 matrix.
// tile (ti, tj), ti >= tj -> its first element; ld: leading dimension inside its tile column
__device__ __forceinline__ double *schur_tile(double *S, long long lds, int ti, int tj, long long &ld)
{
    if (lds >= 0) {
        ld = lds;
        return S + (long long)(ti * 64) + (long long)(tj * 64) * lds;
    }
    const long long L = -lds;
    ld = L - 64 * tj;
    return S + 64 * L * tj - 2048LL * tj * (tj - 1) + (long long)(ti - tj) * 64;
}
// column c -> p with p[r] = element (r, c), r >= 64 (c / 64)
__device__ __forceinline__ double *schur_col(double *S, long long lds, int c)
{
    if (lds >= 0) return S + (long long)c * lds;
    const long long L = -lds;
    const int tj = c >> 6;
    return S + 64 * L * tj - 2048LL * tj * (tj - 1) + (long long)(c & 63) * (L - 64 * tj) - 64 * tj;
}

// item -> (tj, ti) of a trapezoid of 64-row tiles stored column by column: column tj holds ti = tj .. nr-1
__device__ __forceinline__ void trapezoid_decode(int it, int nr, int &tj, int &ti)
{
    const double b = 2.0 * nr + 1.0;
    int c = (int)((b - sqrt(b * b - 8.0 * (double)it)) * 0.5);
    if (c < 0) c = 0;
    while (c > 0 && (long long)c * nr - (long long)c * (c - 1) / 2 > it) --c;
    while ((long long)(c + 1) * nr - (long long)(c + 1) * c / 2 <= it) ++c;
    tj = c;
    ti = c + it - (int)((long long)c * nr - (long long)c * (c - 1) / 2);
}

// ---------------------------------------------------------------------------------------------------------
template <int NW>
__global__ void __launch_bounds__(64 * NW)
nd_potrf_kernel(const PotrfJob *__restrict__ jobs, int *__restrict__ info, double *__restrict__ minpiv)
{
    const PotrfJob j = jobs[blockIdx.x];
    potrf_strip_body<NW>(j.A, j.ld, j.k0, info, minpiv, j.inv16, j.ncols);
}

__global__ void __launch_bounds__(64)
nd_trsm_kernel(const TrsmJob *__restrict__ jobs, int njobs)
{
    constexpr int KREG = 6;                     // parked blocks in registers (chol_device.hpp: trsm_rows): 18 KB of LDS per wave, 8 waves per CU
    __shared__ double xs[(NBLK - 16 - 16 * KREG) * 16];
    const int b = blockIdx.x;
    const int ji = find_job(jobs, njobs, b, [](const TrsmJob &t) { return t.wg0; });
    const TrsmJob j = jobs[ji];
    const int r0 = (b - j.wg0) * 16;
    if (r0 >= j.nrows) return;
    __builtin_amdgcn_s_setprio(3);
    trsm_rows<false, KREG>(j.L, j.X, j.ld, j.ld, j.inv16, nullptr, r0, xs, j.ncb);
}

__global__ void __launch_bounds__(64)
nd_trinv_kernel(const TrinvJob *__restrict__ jobs)
{
    constexpr int KREG = 6;                     // (as in nd_trsm_kernel)
    __shared__ double xs[(NBLK - 16 - 16 * KREG) * 16];
    const TrinvJob j = jobs[blockIdx.y];
    trsm_rows<true, KREG>(j.L, j.dinv, j.ld, NBLK, j.inv16, j.dinvt, blockIdx.x * 16, xs);
}

// Panel-major order of the n x n lower trapezoid of tiles: panels of four tile columns, row by row inside a panel -- the four
// consecutive items of a row share their row operand, and the four column operands of a panel (2 MB at K = 1024) stay in the
// L2 while the panel is walked.  u = index in that order -> (tj, ti).
__device__ __forceinline__ void panel_decode(int u, int n, int &tj, int &ti)
{
    int c0 = 0;
    for (;;) {
        const int m = n - c0, w = m < 4 ? m : 4;
        const int sz = w * (w + 1) / 2 + (m - w) * w;
        if (u < sz) break;
        u -= sz;
        c0 += 4;
    }
    const int m = n - c0, w = m < 4 ? m : 4, tri = w * (w + 1) / 2;
    if (u < tri) {
        int i = 0;
        while (u >= i + 1) { u -= i + 1; ++i; }
        ti = c0 + i;
        tj = c0 + u;
    } else {
        u -= tri;
        ti = c0 + w + u / w;
        tj = c0 + u % w;
    }
}

// (XCC, shader engine, CU) of the CU this wave runs on, as a 12-bit index
__device__ inline unsigned nd_cu_index()
{
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    return ((xcc & 0xfu) << 8) | ((hw >> 8) & 0xffu);
}

// bitmap of the CUs a CU-masked stream runs on (discovery: many short workgroups on that stream)
__global__ void __launch_bounds__(64)
nd_whoami_kernel(unsigned *__restrict__ map)
{
    if (threadIdx.x == 0) {
        const unsigned i = nd_cu_index();
        atomicOr(&map[i >> 5], 1u << (i & 31));
    }
    __builtin_amdgcn_s_sleep(64);
}

// The trailing update of the multifrontal factorisation: one wave = one 64x64 item of C -= P_i P_j^T, in the
// register-streaming form of bandchol.hip's syrk64_kernel (operands loaded in MFMA fragment shape ahead of
// their use, 16 independent v_mfma_f64_16x16x4_f64 accumulators that start as the C tile; no LDS, no barriers).
// The operands wait in a rotating queue of SD slots, one k-step each: the MFMAs of k-step s read slot s % SD, and the slot
// is refilled with k-step s + SD right behind them.  That the queue stays in flight is a property of the ASSEMBLY, not
// of this source: the wait in front of a k-step must be a counted vmcnt(N) that leaves the younger slots' loads pending
// (vmcnt(27) ... vmcnt(24) at SD = 4: three refills of 8 loads).  It is, because the operands are addressed as global
// memory, A is negated by the MFMA and the prologue is retired in front of the loop (below); until then every wait was
// vmcnt(0) and the queue was drained once per SD k-steps (DESIGN 4a "The queue that never was").  After a change here,
// read the loop in `make asm` again.
// P and C have their own base pointers and leading dimensions: P is a block column of a front's panel (kb
// consecutive 256-column blocks of it per pass: K = 256 kb, the C tile is read and written once per pass),
// C the panel right of it or the front's Schur buffer.  SCHUR only names the instantiation: the Schur-buffer
// passes (K up to 1024, ~85 % of the flops of a large fit, one launch at a time) are the roofline kernel of
// bench.py, the panel updates (K = 256, on the chain) are listed separately by the profilers.
// queue != NULL: items are taken from an atomic counter and a wave that finds itself on a CU reserved for the
// diagonal-block factorisations (resmap) steps aside -- the launch carries `margin` spare waves for that.
// SPLIT = 1: a wave computes a whole 64 x 64 item.  SPLIT = 4 / 16: four / sixteen waves share an item (one 16-column slice of
// it each, or one 16 x 16 tile each) -- for launches of a few hundred items, which otherwise leave most of the chip's 1 024
// SIMDs idle while one wave per item works through its 1 024 MFMAs of 64 cycles each (27 us per K = 256, measured 30-57 us
// per launch at BASELINE config 2).  Every element sees the same sequence of operations: bitwise the same result.
// A front's LAST Schur pass (job.pm != NULL) does not store its tile: it adds it into the parent through the child -> parent
// map (extend-add).  That tail fetches the map first and then the parent's entries in batches of 4 N or 8 N per lane -- loads,
// ONE wait, adds, stores, global addressing -- because a wave issues no MFMA while it waits: with one read-modify-write at a
// time (64 per lane, each a full round trip to cold lines) the final passes of the deep stages, which nothing overlaps, ran
// a third longer (DESIGN 4a "The serialised tail").
template <int SD, int WPS, bool SCHUR, int SPLIT = 1, int WGW = 1>
__global__ void __launch_bounds__(64 * WGW, WPS)
nd_syrk_kernel(const SyrkJob *__restrict__ jobs, int njobs, int nitems, int margin, const unsigned *__restrict__ resmap,
               int *__restrict__ queue, int full_diag, int xmode)
{
    // xmode (Schur passes, one wave per item): XCD-aware item map.  The launch's items are cut into eight contiguous slices,
    // one per XCD (workgroups are dealt to the XCDs round robin: blockIdx & 7; with an item queue the XCC id register and
    // one counter per slice, a drained XCD steals from the next), and a front's items are walked in PANEL-major order
    // (panel_decode): operands are then fetched into ONE L2 and reused there instead of streaming through all eight.
    // WGW = 4: four waves per workgroup take four CONSECUTIVE items -- items are stored tile column by tile column, so the
    // four share their column operand, which then comes from the CU's L1 three times out of four (less operand traffic
    // = less power = a higher clock in the long power-limited Schur launches; round 2 measured +7 % for the band's bulk
    // update in sustained runs)
    constexpr int M = SPLIT == 1 ? 4 : 1, N = SPLIT == 16 ? 1 : 4;
    int b = blockIdx.x;
    const bool xm = SCHUR && SPLIT == 1 && WGW == 1 && xmode != 0;
    if (xm && !queue) {
        const int chunk = (nitems + 7) >> 3, loc = b >> 3;
        b = (b & 7) * chunk + loc;
        if (loc >= chunk) return;
    }
    if (queue) {
        if constexpr (WGW == 1) {
            const unsigned ci = nd_cu_index();
            if (resmap[ci >> 5] & (1u << (ci & 31))) {
                int e = 0;
                if (threadIdx.x == 0) e = atomicAdd(&queue[1], 1);
                e = __builtin_amdgcn_readfirstlane(e);
                if (e < margin) {
                    __builtin_amdgcn_s_sleep(127);       // do not drain the grid through this CU
                    __builtin_amdgcn_s_sleep(127);
                    return;
                }
            }
            if (xm) {
                const int chunk = (nitems + 7) >> 3, x0 = (int)((ci >> 8) & 7u);
                int t = -1;
                if (threadIdx.x == 0) {
                    for (int k = 0; k < 8 && t < 0; ++k) {
                        const int y = (x0 + k) & 7, lim = nitems - y * chunk < chunk ? nitems - y * chunk : chunk;
                        if (lim <= 0) continue;
                        const int e = atomicAdd(&queue[2 + y], 1);
                        if (e < lim) t = y * chunk + e;
                    }
                }
                b = __builtin_amdgcn_readfirstlane(t);
                if (b < 0) return;
            } else {
                if (threadIdx.x == 0) b = atomicAdd(&queue[0], 1);
                b = __builtin_amdgcn_readfirstlane(b);
            }
        } else {
            __shared__ int s_b[2];
            if (threadIdx.x == 0) {
                int skip = 0;
                const unsigned ci = nd_cu_index();
                if (resmap[ci >> 5] & (1u << (ci & 31))) skip = atomicAdd(&queue[1], 1) < margin ? 1 : 0;
                s_b[1] = skip;
                s_b[0] = skip ? 0 : atomicAdd(&queue[0], 1);
            }
            __syncthreads();
            if (s_b[1]) {
                __builtin_amdgcn_s_sleep(127);
                __builtin_amdgcn_s_sleep(127);
                return;
            }
            b = s_b[0];
        }
    }
    if constexpr (WGW > 1) b = b * WGW + (int)(threadIdx.x >> 6);
    if (b >= nitems) return;
    const int sub = SPLIT == 1 ? 0 : b % SPLIT;
    if (SPLIT > 1) b /= SPLIT;
    const int m0 = SPLIT == 1 ? 0 : (SPLIT == 4 ? sub : sub >> 2), n0 = SPLIT == 16 ? (sub & 3) : 0;
    const int ji = find_job(jobs, njobs, b, [](const SyrkJob &t) { return t.item0; });
    const SyrkJob j = jobs[ji];
    int tj, ti;
    if (!SCHUR && j.zinit < 0) {                     // rectangle: tile rows rb .. nr-1 of the tile columns 0 .. nc-1
        const int rb = -j.zinit, per = j.nr - rb, it = b - j.item0;
        tj = it / per;
        ti = rb + it - tj * per;
    } else if (xm && j.nc == j.nr)
        panel_decode(b - j.item0, j.nr, tj, ti);
    else
        trapezoid_decode(b - j.item0, j.nr, tj, ti);
    if (tj >= j.nc || ti >= j.nr) return;
    const bool diag = ti == tj;
    if (SPLIT == 16 && diag && n0 < m0) return;      // a 16 x 16 tile above the diagonal
    const int lane = threadIdx.x & 63, l15 = lane & 15, q = lane >> 4;
    // Operands and the C tile are addressed as GLOBAL memory.  The pointers come out of a job struct read from memory, so the
    // compiler would otherwise use flat accesses, and with a flat access pending it cannot count its waits: every wait becomes
    // vmcnt(0) lgkmcnt(0) and the operand queue below is drained at each of them (DESIGN 4a "The queue that never was").
    // COUNTED = false keeps the earlier form (flat accesses, A negated as it is loaded, no stated wait) for the one instantiation
    // whose registers do not take the new one without spilling more: <16, 2, true, 4, 1>, one launch per fit at 64^3.
    constexpr bool COUNTED = !(SCHUR && SPLIT == 4);
    typedef __attribute__((address_space(1))) double gdouble;
    typedef __attribute__((address_space(1))) const int gint;
    typedef typename std::conditional<COUNTED, __attribute__((address_space(1))) const double, const double>::type opnd_t;
    typedef typename std::conditional<COUNTED, gdouble, double>::type ctile_t;
    opnd_t *__restrict__ pJ = (opnd_t *)(j.P + (long long)(tj * 64 + 16 * m0 + l15) + (long long)q * j.ldp);
    opnd_t *__restrict__ pI = (opnd_t *)(j.P + (long long)(ti * 64 + 16 * n0 + l15) + (long long)q * j.ldp);
    long long ldc;
    ctile_t *__restrict__ C = (ctile_t *)schur_tile(j.C, j.ldc, ti, tj, ldc);
    const long long ldp = j.ldp;
    // SPLIT = 4 (80 loads in flight, 256 registers): the operand address is written as a wave-uniform base (tile, k-step) plus
    // one 32-bit byte offset per lane (row in the tile, column in the k-step: 3 ldp + 15 doubles at the most) instead of a 64-bit
    // pointer per lane and operand -- with that the panel form takes 212 registers and no scratch (it had 256 and 28 bytes)
    constexpr bool SBASE = COUNTED && SPLIT == 4;
    typedef __attribute__((address_space(1))) const char gcchar;
    auto uniform = [](const double *p) {
        const unsigned long long a = (unsigned long long)p;
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
        return (gcchar *)(((unsigned long long)hi << 32) | lo);
    };
    gcchar *bJ = uniform(j.P + (tj * 64 + 16 * m0)), *bI = uniform(j.P + (ti * 64 + 16 * n0));
    const unsigned lob = ((unsigned)l15 + (unsigned)q * (unsigned)ldp) * 8u;
    d4_t acc[M][N];
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int n = 0; n < N; ++n)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                acc[m][n][v] = (SCHUR && j.zinit) ? 0.0 : __builtin_nontemporal_load(&C[((n0 + n) * 16 + l15) + (long long)((m0 + m) * 16 + q + 4 * v) * ldc]);
    const bool skipu = diag && !full_diag;
    double qa[SD][M], qb[SD][N];
    auto fetch = [&](int slot, int step) {
        const long long off = (long long)(4 * step) * ldp;
        if constexpr (SBASE) {
#pragma unroll
            for (int m = 0; m < M; ++m) qa[slot][m] = *(opnd_t *)(bJ + (off + 16 * m) * 8 + lob);
#pragma unroll
            for (int n = 0; n < N; ++n) qb[slot][n] = *(opnd_t *)(bI + (off + 16 * n) * 8 + lob);
        } else {
            // A is negated by the MFMA (neg:[1,0,0]), not here: a negation at the load is a VALU instruction the compiler sinks
            // to the use, behind a wait for the load
#pragma unroll
            for (int m = 0; m < M; ++m) qa[slot][m] = COUNTED ? pJ[off + 16 * m] : -pJ[off + 16 * m];
#pragma unroll
            for (int n = 0; n < N; ++n) qb[slot][n] = pI[off + 16 * n];
        }
    };
#pragma unroll
    for (int d = 0; d < SD; ++d) fetch(d, d);
    // the prologue is retired here, stated: the scheduler issues it in no particular order (slot 0 last), and a loop header that
    // inherits its pending loads makes the wait in front of the first k-step -- which both paths into the loop share -- a
    // vmcnt(0) for every trip.  With nothing pending at entry the waits inside the loop are counted.
    if constexpr (COUNTED) __builtin_amdgcn_s_waitcnt(0x0f70);      // gfx9 encoding of vmcnt(0) alone
    constexpr int NSTEP = NBLK / 4;
    static_assert(NSTEP % SD == 0, "queue depth must divide the k-steps");
    const int last = j.kb * NSTEP - 1;               // last k-step of the pass
#pragma unroll 1
    for (int h = 0; h < j.kb; ++h) {                 // one 256-column block per trip: the unrolled body of K = 256
        const int base = h * NSTEP;
        const int kend = (h == j.kb - 1) ? j.ksl : NSTEP;      // the columns beyond are identity padding: zero in these rows
        for (int ks = 0; ks < NSTEP; ks += SD) {
            if (ks >= kend) break;
#pragma unroll
            for (int d = 0; d < SD; ++d) {
#pragma unroll
                for (int m = 0; m < M; ++m)
#pragma unroll
                    for (int n = 0; n < N; ++n) {
                        // (a diagonal item stores its lower triangle only: the 6 of its 16 tiles above the diagonal are skipped --
                        // 1 % of the items of the root, 12 % of those of a front of 16 tile rows; wave-uniform branch)
                        if (SPLIT == 1 && skipu && m > n) continue;
                        acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(qa[d][m], qb[d][n], acc[m][n], 0, 0, COUNTED ? 1 : 0);      // blgp = 1: neg:[1,0,0], -a b
                    }
                if (ks + d + SD < NSTEP) fetch(d, base + ks + d + SD);
                else {                               // the first steps of the next block (clamped: re-reads in the last one)
                    const int nx = base + ks + d + SD;
                    fetch(d, nx < last ? nx : last);
                }
            }
        }
    }
    if (SCHUR && j.pm) {
        // the front's last pass: its Schur complement goes straight into the parent (extend-add), every entry once --
        // the parent's entries of THIS child are touched by no other wave of the launch (the map is injective, the
        // launch holds children of one slot only), so plain read-modify-writes are safe and the order of the sums is
        // fixed: child of slot 0, then child of slot 1.  For the same reason no two of a wave's targets coincide, so the
        // parent's entries are fetched in BATCHES (the 4 N entries of one m, or of two): all map lookups first, then per batch
        // every load, one wait, the adds, every store -- a handful of memory round trips per item instead of one per entry,
        // which the wave would sit through without issuing an MFMA.  The operand queue is dead here: its registers hold the
        // batch.  Targets are addressed as global memory (one 64-bit address per column, panel or Schur buffer), and an
        // entry without a target (padding: -1; above the diagonal of a diagonal item) is neither loaded nor stored.
        constexpr int BM = M < 2 ? M : 2;            // m's per batch
        gint *pm = (gint *)j.pm;
        const int hl = j.h - 1;
        int prow[N], pcol[M][4];
#pragma unroll
        for (int n = 0; n < N; ++n) {
            const int r = ti * 64 + (n0 + n) * 16 + l15, t = pm[r < hl ? r : hl];
            prow[n] = r < j.h ? t : -1;
        }
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int c = tj * 64 + (m0 + m) * 16 + q + 4 * v, t = pm[c < hl ? c : hl];
                pcol[m][v] = c < j.h ? t : -1;
            }
#pragma unroll
        for (int mb = 0; mb < M; mb += BM) {
            gdouble *colp[BM][4];
            double t[BM][4][N];
            auto live = [&](int m, int v, int n) {
                return pcol[m][v] >= 0 && prow[n] >= 0 && !(diag && (n0 + n) * 16 + l15 < (m0 + m) * 16 + q + 4 * v);
            };
#pragma unroll
            for (int e = 0; e < BM; ++e)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int pc = pcol[mb + e][v];
                    colp[e][v] = (gdouble *)(pc < j.wpp ? j.Pp + (long long)pc * j.ldpp : schur_col(j.Sp, j.ldsp, pc - j.wpp) - j.wpp);
                }
#pragma unroll
            for (int e = 0; e < BM; ++e)
#pragma unroll
                for (int v = 0; v < 4; ++v)
#pragma unroll
                    for (int n = 0; n < N; ++n)
                        if (live(mb + e, v, n)) t[e][v][n] = colp[e][v][prow[n]];
            // the batch's one wait, stated: left to the compiler every guarded add gets a vmcnt(0) of its own (a lane that skips
            // one must not skip the wait of the next), which also waits for the store issued just before it
            __builtin_amdgcn_s_waitcnt(0x0f70);      // gfx9 encoding of vmcnt(0) alone
#pragma unroll
            for (int e = 0; e < BM; ++e)
#pragma unroll
                for (int v = 0; v < 4; ++v)
#pragma unroll
                    for (int n = 0; n < N; ++n)
                        if (live(mb + e, v, n)) colp[e][v][prow[n]] = t[e][v][n] + acc[mb + e][n][v];
        }
        return;
    }
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int n = 0; n < N; ++n) {
            const int r = (n0 + n) * 16 + l15;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int c = (m0 + m) * 16 + q + 4 * v;
                if (!diag || r >= c) __builtin_nontemporal_store(acc[m][n][v], &C[r + (long long)c * ldc]);
            }
        }
}

// half stencil -> panels: entry (i, j) of N, j <= i in the natural order, belongs to the front that owns the
// earlier eliminated of the two nodes, at the row of the other one (own row, or border row found by bisection
// of the front's ascending border positions)
template <int D>
__global__ void __launch_bounds__(256)
nd_assemble_kernel(Grid g, const double *__restrict__ nst, const int *__restrict__ pos, const int *__restrict__ front_of,
                   const FrontDev *__restrict__ fd, const int *__restrict__ bpos, double *__restrict__ factor,
                   const TopColDev *__restrict__ topcol)
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
        const int pi = pos[i], pj = pos[j];
        const int c = pi < pj ? i : j;
        const int pc = pi < pj ? pi : pj, pr = pi < pj ? pj : pi;
        const FrontDev f = fd[front_of[c]];
        const int col = pc - f.own0;
        int row;
        if (pr < f.own0 + f.w) row = pr - f.own0;
        else {
            const int *__restrict__ bp = bpos + f.bofs;
            int lo = 0, hi = f.h - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (bp[mid] < pr) lo = mid + 1;
                else hi = mid;
            }
            row = f.wp + lo;
        }
        if (f.top >= 0) {                        // a front distributed by block columns: this rank's columns only
            const int J = col >> 8;
            const TopColDev tc = topcol[f.top + J];
            if (tc.off >= 0) factor[tc.off + (row - (J << 8)) + (long long)(col & 255) * tc.ld] = nst[t];
        } else if (f.panel_off >= 0)
            factor[f.panel_off + row + (long long)col * f.ld] = nst[t];
    }
}

// The panels of ONE STAGE from scratch (round 5): a workgroup per panel column writes the column's zeros and then its entries of
// N -- the FULL stencil of the column's node, those neighbours that are eliminated later (own rows below the diagonal, border
// rows by bisection, as above); a padding column gets its unit diagonal.  Replaces, per stage, the clearing of the whole factor
// arena (14 GB at 64^3: 2.2 ms of memset that either ran before the assembly or shared the memory system with it) and
// nd_assemble_kernel's pass over all of N: the stages whose panels are alive when the factorisation starts are written
// behind the assembly (2.4 GB at 64^3), every later stage when its buffers come alive -- on the update stream at the start of
// the first stage that adds into them, beside that stage's diagonal blocks and panel solves.
template <int D>
__global__ void __launch_bounds__(256)
nd_init_kernel(Grid g, const double *__restrict__ nst, const int *__restrict__ pos, const int *__restrict__ ipos,
               const FrontDev *__restrict__ fd, const int *__restrict__ bpos, double *__restrict__ factor,
               const InitJob *__restrict__ jobs, int njobs)
{
    constexpr int NE = (D == 1) ? 7 : (D == 2) ? 49 : (D == 3) ? 343 : 2401;
    const int b = blockIdx.x;
    const int ji = find_job(jobs, njobs, b, [](const InitJob &t) { return t.col0; });
    const InitJob jb = jobs[ji];
    const FrontDev f = fd[jb.front];
    const int col = b - jb.col0;
    if (col >= f.wp || f.panel_off < 0) return;
    double *__restrict__ cp = factor + f.panel_off + (long long)col * f.ld;
    {
        double *z = cp;
        long long n = f.ld;
        if (reinterpret_cast<unsigned long long>(z) & 8) {
            if (threadIdx.x == 0) z[0] = 0.0;
            ++z, --n;
        }
        d2_t *__restrict__ z2 = reinterpret_cast<d2_t *>(z);
        for (long long i = threadIdx.x; i < (n >> 1); i += 256) __builtin_nontemporal_store((d2_t){0.0, 0.0}, z2 + i);
        if ((n & 1) && threadIdx.x == 0) z[n - 1] = 0.0;
    }
    __syncthreads();                              // (the zeros of the other waves have arrived before an entry goes on top)
    if (col >= f.w) {
        if (threadIdx.x == 0) cp[col] = 1.0;
        return;
    }
    const int pc = f.own0 + col, c = ipos[pc];
    int cd[D];
#pragma unroll
    for (int d = 0; d < D; ++d) cd[d] = (c / g.colstride[d]) % g.nodes[d];
    for (int e = threadIdx.x; e < NE; e += 256) {
        int j = c, code = e, t = e;
        bool ok = true;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int o = (t % 7) - 3;
            t /= 7;
            const int jd = cd[d] + o;
            if (jd < 0 || jd > g.nodes[d] - 1) ok = false;
            j += o * g.colstride[d];
        }
        if (!ok) continue;
        const int pj = pos[j];
        if (pj < pc) continue;                    // that entry lives in the column of j
        // N(c, j): the half stencil keeps it in the row of the larger natural index, code of (smaller - larger)
        const double v = j <= c ? nst[(long long)c * g.hstencil + code] : nst[(long long)j * g.hstencil + (NE - 1 - code)];
        int row;
        if (pj < f.own0 + f.w) row = pj - f.own0;
        else {
            const int *__restrict__ bp = bpos + f.bofs;
            int lo = 0, hi = f.h - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (bp[mid] < pj) lo = mid + 1;
                else hi = mid;
            }
            row = f.wp + lo;
        }
        cp[row] = v;
    }
}

// extend-add into a distributed front (see PullJob): workgroup = 64 x 64 tile of the child's columns [c0, c1), rows >= c0
__global__ void __launch_bounds__(256)
nd_pull_add_kernel(const PullJob *__restrict__ jobs, int njobs)
{
    __shared__ int pr[64], pc[64];
    const int b = blockIdx.x;
    const int ji = find_job(jobs, njobs, b, [](const PullJob &t) { return t.tile0; });
    const PullJob j = jobs[ji];
    const int lt = b - j.tile0;
    const int tj = lt / j.ntr, ti = lt - tj * j.ntr;
    if (tj >= j.ntc) return;
    const int rbase = (j.c0 >> 6) << 6;
    const int r0 = rbase + ti * 64, cc0 = j.c0 + tj * 64;
    if (r0 + 63 < cc0) return;                   // the tile lies above the diagonal
    const int tid = threadIdx.x;
    if (tid < 64) {
        const int r = r0 + tid;
        pr[tid] = r < j.h ? j.pm[r] : -1;
    } else if (tid < 128) {
        const int c = cc0 + tid - 64;
        pc[tid - 64] = c < j.c1 ? j.pm[c] : -1;
    }
    __syncthreads();
    const int rl = tid & 63;
    const int prow = pr[rl];
    if (prow < 0) return;
    const int r = r0 + rl;
#pragma unroll 4
    for (int u = 0; u < 16; ++u) {
        const int cl = (tid >> 6) + 4 * u;
        const int pcol = pc[cl];
        const int c = cc0 + cl;
        if (pcol < 0 || r < c) continue;
        const double v = j.src[(long long)r + (long long)c * j.lds];
        j.dst[(long long)(prow - j.row0) + (long long)(pcol - j.row0) * j.ldd] += v;
    }
}

__global__ void __launch_bounds__(256)
nd_pad_diag_kernel(const long long *__restrict__ where, int n, double *__restrict__ factor)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) factor[where[i]] = 1.0;
}

// Schur buffer of a child -> its parent: workgroup = one 64x64 tile of the child's lower triangle
__global__ void __launch_bounds__(256)
nd_extend_add_kernel(const AddJob *__restrict__ jobs, int njobs)
{
    __shared__ int pr[64], pc[64];
    const int b = blockIdx.x;
    const int ji = find_job(jobs, njobs, b, [](const AddJob &t) { return t.tile0; });
    const AddJob j = jobs[ji];
    int tj, ti;
    trapezoid_decode(b - j.tile0, j.nt, tj, ti);
    if (tj >= j.nt || ti >= j.nt) return;
    const int tid = threadIdx.x;
    if (tid < 64) {
        const int r = ti * 64 + tid;
        pr[tid] = r < j.h ? j.pm[r] : -1;
    } else if (tid < 128) {
        const int c = tj * 64 + tid - 64;
        pc[tid - 64] = c < j.h ? j.pm[c] : -1;
    }
    __syncthreads();
    const int r = tid & 63;
    const int prow = pr[r];
    if (prow < 0) return;
    long long lds;
    const double *__restrict__ S = schur_tile(const_cast<double *>(j.S), j.lds, ti, tj, lds) + r;
#pragma unroll 4
    for (int u = 0; u < 16; ++u) {
        const int c = (tid >> 6) + 4 * u;
        const int pcol = pc[c];
        if (pcol < 0 || (ti == tj && r < c)) continue;
        const double v = S[(long long)c * lds];
        double *dst = pcol < j.wpp ? j.P + prow + (long long)pcol * j.ldp : schur_col(j.Sp, j.ldsp, pcol - j.wpp) + (prow - j.wpp);
        *dst += v;
    }
}

// zeroes the lower-triangle 64x64 tiles of Schur buffers (what the updates and the extend-add read): half the bytes of a
// memset of the square buffers
__global__ void __launch_bounds__(256)
nd_zero_kernel(const ZeroJob *__restrict__ jobs, int njobs)
{
    const int b = blockIdx.x;
    const int ji = find_job(jobs, njobs, b, [](const ZeroJob &t) { return t.tile0; });
    const ZeroJob j = jobs[ji];
    int tj, ti;
    trapezoid_decode(b - j.tile0, j.nt, tj, ti);
    if (tj >= j.nt || ti >= j.nt) return;
    long long lds;
    double *__restrict__ S = schur_tile(j.S, j.lds, ti, tj, lds);
    const int r2 = (threadIdx.x & 31) * 2, c0 = threadIdx.x >> 5;
#pragma unroll
    for (int u = 0; u < 8; ++u) *reinterpret_cast<d2_t *>(S + r2 + (long long)(c0 + 8 * u) * lds) = (d2_t){0.0, 0.0};
}

// The early clear of the panels, beside the binning of the points.  Not a memset of the runtime: that one spreads its workgroups
// over every CU until it is done (2.2 ms for 12 GB), and the binning's scatter kernel -- one workgroup takes a whole CU: 144 KB
// of LDS, 16 waves of 128 registers -- then only starts where a CU has drained: round 5 saw its workgroups run on the even
// XCDs first and on the odd ones 450 us later (1.15 ms instead of 0.42 ms alone).  A few resident workgroups write as fast and
// leave the other CUs whole.
__global__ void __launch_bounds__(1024)
nd_clear_kernel(double *__restrict__ p, long long n)
{
    if (n > 0 && (reinterpret_cast<unsigned long long>(p) & 8)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) p[0] = 0.0;
        ++p, --n;
    }
    d2_t *__restrict__ q = reinterpret_cast<d2_t *>(p);
    const long long n2 = n >> 1, step = (long long)gridDim.x * 1024 * 4;
    for (long long i = (long long)blockIdx.x * 4096 + threadIdx.x; i < n2; i += step) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + 1024 * u < n2) __builtin_nontemporal_store((d2_t){0.0, 0.0}, q + i + 1024 * u);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) p[n - 1] = 0.0;
}

// distributed factorisation: the lower-triangle tiles of a Schur buffer <-> a contiguous image (tile after tile, column-major
// inside a tile), so that the join sums half the bytes of the square buffer
template <bool PACK>
__global__ void __launch_bounds__(256)
nd_tripack_kernel(double *__restrict__ S, long long lds, int nt, double *__restrict__ img)
{
    int tj, ti;
    trapezoid_decode(blockIdx.x, nt, tj, ti);
    if (tj >= nt || ti >= nt) return;
    double *__restrict__ T = S + (long long)(ti * 64) + (long long)(tj * 64) * lds;
    double *__restrict__ I = img + (long long)blockIdx.x * 4096;
    const int r2 = (threadIdx.x & 31) * 2, c0 = threadIdx.x >> 5;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int c = c0 + 8 * u;
        if (PACK) *reinterpret_cast<d2_t *>(I + r2 + 64 * c) = *reinterpret_cast<const d2_t *>(T + r2 + (long long)c * lds);
        else *reinterpret_cast<d2_t *>(T + r2 + (long long)c * lds) = *reinterpret_cast<const d2_t *>(I + r2 + 64 * c);
    }
}

// distributed factorisation: the pivot status is made collective (a rank must not leave the fit alone)
__global__ void nd_flag_kernel(const int *__restrict__ info, double *__restrict__ flag, int phase)
{
    if (phase == 0) flag[0] = info[0] != 0 ? 1.0 : 0.0;
}
__global__ void nd_unflag_kernel(int *__restrict__ info, const double *__restrict__ flag)
{
    if (flag[0] != 0.0 && info[0] == 0) info[0] = 0x7fffffff;        // another rank's subtree failed
}

// ---- solves ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
nd_gather_kernel(long long n, const int *__restrict__ rowsrc, const double *__restrict__ b, double *__restrict__ V)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int s = rowsrc[i];
        V[i] = s >= 0 ? b[s] : 0.0;
    }
}

__global__ void __launch_bounds__(256)
nd_scatter_kernel(long long n, const int *__restrict__ rowsrc, const double *__restrict__ V, double *__restrict__ x)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int s = rowsrc[i];
        if (s >= 0) x[s] = V[i];
    }
}

// forward: parent rows += the child's border updates; backward: the child's border values = parent rows
template <bool TAKE>
__global__ void __launch_bounds__(256)
nd_map_kernel(const MapJob *__restrict__ jobs)
{
    const MapJob j = jobs[blockIdx.y];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < j.h; i += gridDim.x * blockDim.x) {
        const int r = j.pm[i];
        if (TAKE) j.child[i] = j.par[r];
        else j.par[r] += j.child[i];
    }
}

// out = M v for row-major 256x256 blocks; grid (16, jobs) x 256 threads: a wave dots 4 rows
__global__ void __launch_bounds__(256)
nd_mv_kernel(const MvJob *__restrict__ jobs)
{
    const MvJob j = jobs[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * 16 + wave * 4;
    double vv[4], s[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) vv[u] = j.v[lane + 64 * u];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s[i] = 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) s[i] += j.M[(r0 + i) * NBLK + lane + 64 * u] * vv[u];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = wave_sum(s[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) j.out[r0 + i] = s[i];
    }
}

// v[rows below] -= L[rows, block] y: workgroup = 64 rows x 256 columns, 512 threads = 32 row pairs x 16 column groups
__global__ void __launch_bounds__(512)
nd_fwd_kernel(const FwdJob *__restrict__ jobs, int njobs)
{
    __shared__ double sy[NBLK];
    __shared__ double part[16][64];
    const int b = blockIdx.x;
    const int ji = find_job(jobs, njobs, b, [](const FwdJob &t) { return t.wg0; });
    const FwdJob j = jobs[ji];
    const int wg = b - j.wg0;
    if (wg * 64 >= j.nrows) return;
    const int tid = threadIdx.x;
    if (tid < NBLK) sy[tid] = j.y[tid];
    __syncthreads();
    const int rp = tid & 31, cg = tid >> 5;
    const int r = wg * 64 + 2 * rp;
    const double *__restrict__ Lr = j.L + r + (long long)(cg * 16) * j.ld;
    // a column group at or beyond the block's real columns loads nothing: its sixteen columns are identity padding (zero here, below
    // the diagonal) against y entries that are exactly zero -- every product it left out was +0.0 added to +0.0: the same bits
    const bool real = cg * 16 < j.ncols;
    double s0 = 0.0, s1 = 0.0;
    if (real) {
        d2_t l[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) l[c] = *reinterpret_cast<const d2_t *>(Lr + (long long)c * j.ld);
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const double yv = sy[cg * 16 + c];
            s0 += l[c][0] * yv;
            s1 += l[c][1] * yv;
        }
    }
    part[cg][2 * rp] = s0;
    part[cg][2 * rp + 1] = s1;
    __syncthreads();
    if (tid < 64) {
        double s = 0.0;
#pragma unroll
        for (int g = 0; g < 16; ++g) s += part[g][tid];
        j.v[wg * 64 + tid] -= s;
    }
}

// part[split][c] = sum over the rows of the split of L[r, c] x[r]; workgroup = (16 columns, split), a wave takes 4 columns
__global__ void __launch_bounds__(256)
nd_dot_kernel(const DotJob *__restrict__ jobs, int njobs)
{
    const int b = blockIdx.x;
    const int ji = find_job(jobs, njobs, b, [](const DotJob &t) { return t.wg0; });
    const DotJob j = jobs[ji];
    const int lw = b - j.wg0;
    const int cg = lw & 15, split = lw >> 4;
    if (split >= j.nsplit) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = cg * 16 + wave * 4;
    const int rbeg = split * j.rps;
    const int rend = rbeg + j.rps < j.nrows ? rbeg + j.rps : j.nrows;
    if (c0 >= j.ncols) {      // four columns of identity padding: nothing to read, and nd_bwd_kernel reads every entry of `part`
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) j.part[(long long)split * NBLK + c0 + c] = 0.0;
        }
        return;
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const double *__restrict__ Lc = j.L + lane + (long long)c0 * j.ld;
    // four row groups (20 loads) in flight per round: the rolled loop paid one memory round trip per 64 rows, 16 in a row
    // for a split of 1 024 -- the launch sits on the chain of every backward step.  Same order of the sums.
    int r = rbeg;
    for (; r + 192 < rend; r += 256) {
        double xr[4], l[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            xr[t] = j.x[r + 64 * t + lane];
#pragma unroll
            for (int c = 0; c < 4; ++c) l[t][c] = Lc[r + 64 * t + (long long)c * j.ld];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] += l[t][c] * xr[t];
    }
    for (; r < rend; r += 64) {
        const double xr = j.x[r + lane];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] += Lc[r + (long long)c * j.ld] * xr;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = wave_sum(acc[c]);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) j.part[(long long)split * NBLK + c0 + c] = acc[c];
    }
}

// x_k = Linv_k^T (y_k - sum_split part[split]); grid (16, jobs) x 256 threads
__global__ void __launch_bounds__(256)
nd_bwd_kernel(const BwdJob *__restrict__ jobs)
{
    const BwdJob j = jobs[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * 16 + wave * 4;
    // the 16 matrix entries are in flight while the partial dots are summed; the four columns of a split are loaded together
    // (the sums keep their order: split after split) -- the launch sits on the chain of every backward step
    double vv[4], s[4], mt[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int u = 0; u < 4; ++u) mt[i][u] = j.Mt[(r0 + i) * NBLK + lane + 64 * u];
#pragma unroll
    for (int u = 0; u < 4; ++u) vv[u] = j.y[lane + 64 * u];
    int sp = 0;
    for (; sp + 1 < j.nsplit; sp += 2) {
        double p0[4], p1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            p0[u] = j.part[(long long)sp * NBLK + lane + 64 * u];
            p1[u] = j.part[(long long)(sp + 1) * NBLK + lane + 64 * u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) vv[u] = (vv[u] - p0[u]) - p1[u];
    }
    if (sp < j.nsplit) {
#pragma unroll
        for (int u = 0; u < 4; ++u) vv[u] -= j.part[(long long)sp * NBLK + lane + 64 * u];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s[i] = 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) s[i] += mt[i][u] * vv[u];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = wave_sum(s[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) j.x[r0 + i] = s[i];
    }
}

// ---- solves of R right-hand sides in one sweep (nd_solve_many) -----------------------------------------------
// The kernels above with the vectors of slot r in copy r of V, Y and part (BatchVec): a thread loads its piece of L or of a
// block inverse ONCE and multiplies it by the R vectors one after another, every vector in the order of operations of the single
// kernel -- the bits of R single solves for one reading of the factor.
__device__ __forceinline__ double *batch_at(double *base, long long stride, int r, const double *job, const double *base0)
{
    return base + (long long)r * stride + (job - base0);
}

__global__ void __launch_bounds__(256)
nd_gather_many_kernel(long long n, const int *__restrict__ rowsrc, BatchPtrs b, BatchVec w)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int s = rowsrc[i];
        (w.V + (long long)blockIdx.y * w.vstride)[i] = s >= 0 ? b.p[blockIdx.y][s] : 0.0;
    }
}

__global__ void __launch_bounds__(256)
nd_scatter_many_kernel(long long n, const int *__restrict__ rowsrc, BatchVec w, BatchPtrs x)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int s = rowsrc[i];
        if (s >= 0) x.p[blockIdx.y][s] = (w.V + (long long)blockIdx.y * w.vstride)[i];
    }
}

// grid (8, jobs, R)
template <bool TAKE>
__global__ void __launch_bounds__(256)
nd_map_many_kernel(const MapJob *__restrict__ jobs, BatchVec w)
{
    const MapJob j = jobs[blockIdx.y];
    double *child = batch_at(w.V, w.vstride, blockIdx.z, j.child, w.V0);
    double *par = batch_at(w.V, w.vstride, blockIdx.z, j.par, w.V0);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < j.h; i += gridDim.x * blockDim.x) {
        const int r = j.pm[i];
        if (TAKE) child[i] = par[r];
        else par[r] += child[i];
    }
}

template <int R>
__global__ void __launch_bounds__(256)
nd_mv_many_kernel(const MvJob *__restrict__ jobs, BatchVec w)
{
    const MvJob j = jobs[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * 16 + wave * 4;
    double m[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int u = 0; u < 4; ++u) m[i][u] = j.M[(r0 + i) * NBLK + lane + 64 * u];
#pragma unroll
    for (int f = 0; f < R; ++f) {
        const double *__restrict__ v = batch_at(w.V, w.vstride, f, j.v, w.V0);
        double *__restrict__ out = batch_at(w.Y, w.vstride, f, j.out, w.Y0);
        double vv[4], s[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) vv[u] = v[lane + 64 * u];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            s[i] = 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) s[i] += m[i][u] * vv[u];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = wave_sum(s[i]);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) out[r0 + i] = s[i];
        }
    }
}

// The R vectors y in LDS (R x 256 doubles); the column groups' partial sums of up to four right-hand sides at a time (4 x 16 x 64
// doubles: 48 KiB with the vectors at R = 8, where one round over all eight would take 80), L in registers across the rounds.
template <int R>
__global__ void __launch_bounds__(512)
nd_fwd_many_kernel(const FwdJob *__restrict__ jobs, int njobs, BatchVec w)
{
    constexpr int RC = R < 4 ? R : 4;
    __shared__ double sy[R][NBLK];
    __shared__ double part[RC][16][64];
    const int b = blockIdx.x;
    const int ji = find_job(jobs, njobs, b, [](const FwdJob &t) { return t.wg0; });
    const FwdJob j = jobs[ji];
    const int wg = b - j.wg0;
    if (wg * 64 >= j.nrows) return;
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = tid; i < R * NBLK; i += 512) sy[i >> 8][i & 255] = batch_at(w.Y, w.vstride, i >> 8, j.y, w.Y0)[i & 255];
    const int rp = tid & 31, cg = tid >> 5;
    const int r = wg * 64 + 2 * rp;
    const double *__restrict__ Lr = j.L + r + (long long)(cg * 16) * j.ld;
    const bool real = cg * 16 < j.ncols;      // (as in nd_fwd_kernel: a group of padding columns loads nothing and adds +0.0)
    d2_t l[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) l[c] = real ? *reinterpret_cast<const d2_t *>(Lr + (long long)c * j.ld) : d2_t{0.0, 0.0};
    __syncthreads();
#pragma unroll
    for (int f0 = 0; f0 < R; f0 += RC) {
        const int nf = R - f0 < RC ? R - f0 : RC;
#pragma unroll
        for (int ff = 0; ff < RC; ++ff) {
            if (ff < nf) {
                double s0 = 0.0, s1 = 0.0;
                if (real) {
#pragma unroll
                    for (int c = 0; c < 16; ++c) {
                        const double yv = sy[f0 + ff][cg * 16 + c];
                        s0 += l[c][0] * yv;
                        s1 += l[c][1] * yv;
                    }
                }
                part[ff][cg][2 * rp] = s0;
                part[ff][cg][2 * rp + 1] = s1;
            }
        }
        __syncthreads();
        if (tid < 64 * nf) {
            const int ff = tid >> 6, t = tid & 63;
            double s = 0.0;
#pragma unroll
            for (int g = 0; g < 16; ++g) s += part[ff][g][t];
            batch_at(w.V, w.vstride, f0 + ff, j.v, w.V0)[wg * 64 + t] -= s;
        }
        if (f0 + RC < R) __syncthreads();
    }
}

template <int R>
__global__ void __launch_bounds__(256)
nd_dot_many_kernel(const DotJob *__restrict__ jobs, int njobs, BatchVec w)
{
    const int b = blockIdx.x;
    const int ji = find_job(jobs, njobs, b, [](const DotJob &t) { return t.wg0; });
    const DotJob j = jobs[ji];
    const int lw = b - j.wg0;
    const int cg = lw & 15, split = lw >> 4;
    if (split >= j.nsplit) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = cg * 16 + wave * 4;
    const int rbeg = split * j.rps;
    const int rend = rbeg + j.rps < j.nrows ? rbeg + j.rps : j.nrows;
    if (c0 >= j.ncols) {      // (as in nd_dot_kernel: padding columns are not read, their entries of every `part` are 0.0)
        if (lane == 0) {
#pragma unroll
            for (int f = 0; f < R; ++f) {
                double *__restrict__ pp = batch_at(w.part, w.pstride, f, j.part, w.part0);
#pragma unroll
                for (int c = 0; c < 4; ++c) pp[(long long)split * NBLK + c0 + c] = 0.0;
            }
        }
        return;
    }
    double acc[R][4];
#pragma unroll
    for (int f = 0; f < R; ++f)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[f][c] = 0.0;
    const double *__restrict__ Lc = j.L + lane + (long long)c0 * j.ld;
    const double *__restrict__ x0 = batch_at(w.V, w.vstride, 0, j.x, w.V0);
    int r = rbeg;
    for (; r + 192 < rend; r += 256) {
        double l[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c) l[t][c] = Lc[r + 64 * t + (long long)c * j.ld];
#pragma unroll
        for (int f = 0; f < R; ++f) {
            double xr[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) xr[t] = x0[(long long)f * w.vstride + r + 64 * t + lane];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[f][c] += l[t][c] * xr[t];
        }
    }
    for (; r < rend; r += 64) {
        double l[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) l[c] = Lc[r + (long long)c * j.ld];
#pragma unroll
        for (int f = 0; f < R; ++f) {
            const double xr = x0[(long long)f * w.vstride + r + lane];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[f][c] += l[c] * xr;
        }
    }
#pragma unroll
    for (int f = 0; f < R; ++f) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[f][c] = wave_sum(acc[f][c]);
        if (lane == 0) {
            double *__restrict__ pp = batch_at(w.part, w.pstride, f, j.part, w.part0);
#pragma unroll
            for (int c = 0; c < 4; ++c) pp[(long long)split * NBLK + c0 + c] = acc[f][c];
        }
    }
}

template <int R>
__global__ void __launch_bounds__(256)
nd_bwd_many_kernel(const BwdJob *__restrict__ jobs, BatchVec w)
{
    const BwdJob j = jobs[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * 16 + wave * 4;
    double mt[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int u = 0; u < 4; ++u) mt[i][u] = j.Mt[(r0 + i) * NBLK + lane + 64 * u];
#pragma unroll
    for (int f = 0; f < R; ++f) {
        const double *__restrict__ y = batch_at(w.Y, w.vstride, f, j.y, w.Y0);
        const double *__restrict__ part = batch_at(w.part, w.pstride, f, j.part, w.part0);
        double *__restrict__ x = batch_at(w.V, w.vstride, f, j.x, w.V0);
        double vv[4], s[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) vv[u] = y[lane + 64 * u];
        int sp = 0;
        for (; sp + 1 < j.nsplit; sp += 2) {
            double p0[4], p1[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                p0[u] = part[(long long)sp * NBLK + lane + 64 * u];
                p1[u] = part[(long long)(sp + 1) * NBLK + lane + 64 * u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) vv[u] = (vv[u] - p0[u]) - p1[u];
        }
        if (sp < j.nsplit) {
#pragma unroll
            for (int u = 0; u < 4; ++u) vv[u] -= part[(long long)sp * NBLK + lane + 64 * u];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            s[i] = 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) s[i] += mt[i][u] * vv[u];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = wave_sum(s[i]);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) x[r0 + i] = s[i];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// launchers.  Diagonal blocks: a workgroup per job, 8 waves each (SPLPAK_ND_POTRF_WAVES = 4: the band path's form, 16)
static void potrf_dispatch(int waves, const PotrfJob *jobs, unsigned n, hipStream_t st, int *info_dev, double *minpiv_dev)
{
    if (waves == 4) hipLaunchKernelGGL(nd_potrf_kernel<4>, dim3(n), dim3(256), 0, st, jobs, info_dev, minpiv_dev);
    else if (waves == 8) hipLaunchKernelGGL(nd_potrf_kernel<8>, dim3(n), dim3(512), 0, st, jobs, info_dev, minpiv_dev);
    else hipLaunchKernelGGL(nd_potrf_kernel<16>, dim3(n), dim3(1024), 0, st, jobs, info_dev, minpiv_dev);
}

// a launch over the jobs [l.first, l.first + l.count) of a table whose kernel finds its job by bisection of blockIdx.x
template <typename J> static void launch_jobs(void (*kernel)(const J *, int), unsigned threads, const JobTable<J> &tab, const Launch &l, hipStream_t st)
{
    if (l.count && l.grid) hipLaunchKernelGGL(kernel, dim3(l.grid), dim3(threads), 0, st, (const J *)(tab.dev + l.first), l.count);
}
// ... whose kernel takes job blockIdx.y, with gx workgroups per job
template <typename J> static void launch_each(void (*kernel)(const J *), unsigned gx, unsigned threads, const J *jobs, unsigned njobs, hipStream_t st)
{
    if (njobs) hipLaunchKernelGGL(kernel, dim3(gx, njobs), dim3(threads), 0, st, jobs);
}

void launch_potrf(const NdState *s, const JobTable<PotrfJob> &tab, const Launch &l, hipStream_t st, int *info_dev, double *minpiv_dev)
{
    if (l.count) potrf_dispatch(s->potrf_waves, tab.dev + l.first, l.grid, st, info_dev, minpiv_dev);
}
void launch_trsm(const JobTable<TrsmJob> &tab, const Launch &l, hipStream_t st) { launch_jobs(nd_trsm_kernel, 64, tab, l, st); }
void launch_trinv(const TrinvJob *jobs_dev, int n, hipStream_t st) { launch_each(nd_trinv_kernel, NBLK / 16, 64, jobs_dev, (unsigned)n, st); }

void launch_syrk(NdState *s, const JobTable<SyrkJob> &tab, const Launch &l, hipStream_t st, CholStats *stats, bool timing, bool schur,
                 bool pinned, int &qnext)
{
    if (l.count == 0 || l.grid == 0) return;
    hipEvent_t a = nullptr, b = nullptr;
    if (timing && schur) {
        const size_t i = (size_t)stats->syrk_launches;
        while (s->ev.evA.size() <= i) {
            s->ev.evA.push_back(nd_event(s, true));
            s->ev.evB.push_back(nd_event(s, true));
        }
        a = s->ev.evA[i];
        b = s->ev.evB[i];
        stats->syrk_launches += 1;
        stats->syrk_flop += l.flop;
    }
    if (stats) {
        stats->total_flop += l.flop;
        if (schur) {
            stats->bulk_launches += 1;
            stats->bulk_flop += l.flop;
        }
    }
    // A small launch (split over several waves per item) does without the item queue: its waves are gone in microseconds, so
    // they need not keep off the reserved CUs -- and the queue costs it dearly: 2 048 placeholder workgroups plus one atomic
    // per workgroup on ONE word made the 10-item update of the root's next diagonal block a 60-75 us launch, on the chain of
    // every one of the root's 48 steps (round 3, tools/last_fit_trace.py).
    const bool small_launch = (int)l.grid <= s->small_grid && !s->small_queue;
    int *queue = nullptr;
    int margin = 0;
    if (pinned && s->nres > 0 && qnext < s->nqueues && !small_launch) {
        queue = s->queues + ND_QSTRIDE * (qnext++);
        margin = 256 * s->nres;
    }
    const SyrkJob *jobs = tab.dev + l.first;
    // SD = 4 k-steps of operand look-ahead, two waves per SIMD (246 registers).  The measurement that chose it -- at 64^3
    // against the 16-deep queue / one wave per SIMD form the band's bulk update uses, 257.6 against 282.2 ms per
    // factorisation -- compared two forms that both drained their queue at every wait (vmcnt(0), see nd_syrk_kernel): it
    // showed that two waves per SIMD hide a drained queue better than one, not what a queue of either depth is worth.
    // What stands of it: a queue carried across the block loop of a K = 1024 pass has to live in registers, and 16 slots
    // beside 128 accumulator registers leave room for one wave only.  SD has not been retuned with the queue working.
    // Launches of a few hundred items leave most SIMDs idle while one wave per item works through its MFMAs: they are split
    // over 4 / 16 waves per item (SPLIT above; same arithmetic order, bitwise the same result)
    // (beside a bulk update that fills every wave slot -- `pinned` -- the waves of this launch are placed as slots retire,
    // ~37 per us at 64^3: sixteen waves per item then wait longer than they save; four per item there)
    int split = (int)l.grid * 4 <= s->small_grid ? 16 : ((int)l.grid <= s->small_grid ? 4 : 1);
    if (pinned && split > 4) split = 4;
    const int nit = (int)l.grid * split;
    const bool wg4 = split == 1 && (s->wg4 >= 2 || (s->wg4 == 1 && schur));
    unsigned gx = wg4 ? (l.grid + 3) / 4 : l.grid * (unsigned)split;
    if (s->xmode && schur && split == 1 && !wg4 && !queue) gx = (gx + 7u) / 8u * 8u;      // eight equal slices
    const dim3 grid(gx + (unsigned)margin);
    // operand look-ahead in k-steps: a split wave issues 1 (4) MFMA per step, so 4 steps cover 256 (1 024) cycles -- less than
    // one memory round trip: 77 us per K = 256 launch of the root's look-ahead block.  32 (16) steps in flight instead
    // (as measured then, fetched as a batch and drained once per 32 (16) steps; in flight throughout only with counted waits).
#define ND_SD(SPL) ((SPL) == 16 ? 32 : ((SPL) == 4 ? 16 : 4))
#define ND_SYRK_GO(SCH, SPL, WW)                                                                                               \
    do {                                                                                                                       \
        if (SCH) hipExtLaunchKernelGGL((nd_syrk_kernel<ND_SD(SPL), 2, SCH, SPL, WW>), grid, dim3(64 * WW), 0, st, a, b, 0, jobs, l.count, nit, margin,  \
                                       (const unsigned *)s->resmap, queue, s->full_diag, s->xmode);                            \
        else hipLaunchKernelGGL((nd_syrk_kernel<ND_SD(SPL), 2, SCH, SPL, WW>), grid, dim3(64 * WW), 0, st, jobs, l.count, nit, margin,   \
                                (const unsigned *)s->resmap, queue, s->full_diag, s->xmode);                                  \
    } while (0)
    if (schur) {
        if (split == 16) ND_SYRK_GO(true, 16, 1); else if (split == 4) ND_SYRK_GO(true, 4, 1); else if (wg4) ND_SYRK_GO(true, 1, 4); else ND_SYRK_GO(true, 1, 1);
    } else {
        if (split == 16) ND_SYRK_GO(false, 16, 1); else if (split == 4) ND_SYRK_GO(false, 4, 1); else if (wg4) ND_SYRK_GO(false, 1, 4); else ND_SYRK_GO(false, 1, 1);
    }
#undef ND_SYRK_GO
#undef ND_SD
}

void launch_add(const JobTable<AddJob> &tab, const Launch &l, hipStream_t st) { launch_jobs(nd_extend_add_kernel, 256, tab, l, st); }
void launch_pull(const JobTable<PullJob> &tab, const Launch &l, hipStream_t st) { launch_jobs(nd_pull_add_kernel, 256, tab, l, st); }
void launch_zero(const JobTable<ZeroJob> &tab, const Launch &l, hipStream_t st) { launch_jobs(nd_zero_kernel, 256, tab, l, st); }
void launch_fwd(const JobTable<FwdJob> &tab, const Launch &l, hipStream_t st) { launch_jobs(nd_fwd_kernel, 512, tab, l, st); }
void launch_dot(const JobTable<DotJob> &tab, const Launch &l, hipStream_t st) { launch_jobs(nd_dot_kernel, 256, tab, l, st); }
void launch_mv(const JobTable<MvJob> &tab, const Launch &l, hipStream_t st) { launch_each(nd_mv_kernel, 16, 256, (const MvJob *)(tab.dev + l.first), l.grid, st); }
void launch_bwd(const JobTable<BwdJob> &tab, const Launch &l, hipStream_t st) { launch_each(nd_bwd_kernel, 16, 256, (const BwdJob *)(tab.dev + l.first), l.grid, st); }
void launch_map(const JobTable<MapJob> &tab, const Launch &l, bool take, hipStream_t st)
{
    launch_each(take ? nd_map_kernel<true> : nd_map_kernel<false>, 8, 256, (const MapJob *)(tab.dev + l.first), l.grid, st);
}

void launch_init(const NdState *s, const Grid &g, const double *nst, const Launch &l, hipStream_t st)
{
    if (!l.count) return;
    DISPATCH_D(g.ndim, hipLaunchKernelGGL(nd_init_kernel<D>, dim3(l.grid), dim3(256), 0, st, g, nst, (const int *)s->pos, (const int *)s->ipos, (const FrontDev *)s->fdev,
                                          (const int *)s->bpos, s->factor, (const InitJob *)(s->fac.init.dev + l.first), l.count));
}

void launch_assemble(const NdState *s, const Grid &g, const double *nst, hipStream_t st)
{
    const long long total = (long long)g.ncol * g.hstencil;
    long long blocks = (total + 255) / 256;
    if (blocks > 256LL * 64) blocks = 256LL * 64;
    DISPATCH_D(g.ndim, hipLaunchKernelGGL(nd_assemble_kernel<D>, dim3((unsigned)blocks), dim3(256), 0, st, g, nst, (const int *)s->pos, (const int *)s->front_of,
                                          (const FrontDev *)s->fdev, (const int *)s->bpos, s->factor, (const TopColDev *)s->top.topcol_dev));
    if (s->npad > 0)
        hipLaunchKernelGGL(nd_pad_diag_kernel, dim3((unsigned)((s->npad + 255) / 256)), dim3(256), 0, st, (const long long *)s->padwhere, s->npad, s->factor);
}

void launch_clear(int wgs, double *p, long long n, hipStream_t st) { hipLaunchKernelGGL(nd_clear_kernel, dim3((unsigned)wgs), dim3(1024), 0, st, p, n); }
// lower-triangle tiles of a square Schur buffer -> image (pack), or back
void launch_tripack(bool pack, double *S, long long lds, int nt, double *img, hipStream_t st)
{
    hipLaunchKernelGGL(pack ? nd_tripack_kernel<true> : nd_tripack_kernel<false>, dim3((unsigned)trapezoid_items(nt, nt)), dim3(256), 0, st, S, lds, nt, img);
}
void launch_flag(const int *info, double *flag, hipStream_t st) { hipLaunchKernelGGL(nd_flag_kernel, dim3(1), dim3(1), 0, st, info, flag, 0); }
void launch_unflag(int *info, const double *flag, hipStream_t st) { hipLaunchKernelGGL(nd_unflag_kernel, dim3(1), dim3(1), 0, st, info, flag); }
void launch_whoami(unsigned wgs, unsigned *map, hipStream_t st) { hipLaunchKernelGGL(nd_whoami_kernel, dim3(wgs), dim3(64), 0, st, map); }
void launch_gather(long long n, const int *rowsrc, const double *b, double *V, hipStream_t st) { hipLaunchKernelGGL(nd_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, rowsrc, b, V); }
void launch_scatter(long long n, const int *rowsrc, const double *V, double *x, hipStream_t st) { hipLaunchKernelGGL(nd_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, rowsrc, V, x); }

// the forms for R right-hand sides: the grids of the single launches (gather, scatter and map: a grid dimension over the slots)
#define ND_MANY(R, GO)                                                                                                         \
    switch (R) {                                                                                                               \
    case 2: GO(2); break; case 3: GO(3); break; case 4: GO(4); break; case 5: GO(5); break;                                    \
    case 6: GO(6); break; case 7: GO(7); break; case 8: GO(8); break;                                                          \
    default: break;                                                                                                            \
    }
void launch_gather_many(long long n, const int *rowsrc, const BatchPtrs &b, const BatchVec &w, int R, hipStream_t st)
{
    hipLaunchKernelGGL(nd_gather_many_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)R), dim3(256), 0, st, n, rowsrc, b, w);
}
void launch_scatter_many(long long n, const int *rowsrc, const BatchPtrs &x, const BatchVec &w, int R, hipStream_t st)
{
    hipLaunchKernelGGL(nd_scatter_many_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)R), dim3(256), 0, st, n, rowsrc, w, x);
}
void launch_map_many(const JobTable<MapJob> &tab, const Launch &l, bool take, const BatchVec &w, int R, hipStream_t st)
{
    if (!l.grid) return;
    hipLaunchKernelGGL(take ? nd_map_many_kernel<true> : nd_map_many_kernel<false>, dim3(8, l.grid, (unsigned)R), dim3(256), 0, st, (const MapJob *)(tab.dev + l.first), w);
}
void launch_mv_many(const JobTable<MvJob> &tab, const Launch &l, const BatchVec &w, int R, hipStream_t st)
{
    if (!l.grid) return;
#define GO(N) hipLaunchKernelGGL(nd_mv_many_kernel<N>, dim3(16, l.grid), dim3(256), 0, st, (const MvJob *)(tab.dev + l.first), w)
    ND_MANY(R, GO)
#undef GO
}
void launch_bwd_many(const JobTable<BwdJob> &tab, const Launch &l, const BatchVec &w, int R, hipStream_t st)
{
    if (!l.grid) return;
#define GO(N) hipLaunchKernelGGL(nd_bwd_many_kernel<N>, dim3(16, l.grid), dim3(256), 0, st, (const BwdJob *)(tab.dev + l.first), w)
    ND_MANY(R, GO)
#undef GO
}
void launch_fwd_many(const JobTable<FwdJob> &tab, const Launch &l, const BatchVec &w, int R, hipStream_t st)
{
    if (!l.count || !l.grid) return;
#define GO(N) hipLaunchKernelGGL(nd_fwd_many_kernel<N>, dim3(l.grid), dim3(512), 0, st, (const FwdJob *)(tab.dev + l.first), l.count, w)
    ND_MANY(R, GO)
#undef GO
}
void launch_dot_many(const JobTable<DotJob> &tab, const Launch &l, const BatchVec &w, int R, hipStream_t st)
{
    if (!l.count || !l.grid) return;
#define GO(N) hipLaunchKernelGGL(nd_dot_many_kernel<N>, dim3(l.grid), dim3(256), 0, st, (const DotJob *)(tab.dev + l.first), l.count, w)
    ND_MANY(R, GO)
#undef GO
}
#undef ND_MANY

}  // namespace nd

using nd::PotrfJob;
using nd::TrinvJob;

// ---- batched Cholesky of independent dense 256 x 256 blocks (the block-Jacobi component of the iterative solve, pcg.hip) ----------
// The diagonal-block kernels of the fronts on blocks that belong to no front: `blocks` holds nb column-major 256 x 256 matrices (lower
// triangle read, L written in place), inv16 nb x 16 leaf inverses of 16 x 16, dinv / dinvt the inverse of L row-major and its
// transpose.  The job tables live in device memory the caller provides (block_chol_job_bytes) and are written once per plan.
size_t block_chol_job_bytes(int nb) { return (size_t)nb * (sizeof(PotrfJob) + sizeof(TrinvJob)) + 256; }

hipError_t block_chol_prepare(void *jobs_dev, int nb, double *blocks, double *inv16, double *dinv, double *dinvt, const int *ncols_host)
{
    std::vector<PotrfJob> pj((size_t)nb);
    std::vector<TrinvJob> tj((size_t)nb);
    for (int b = 0; b < nb; ++b) {
        double *A = blocks + (size_t)b * NBLK * NBLK, *iv = inv16 + (size_t)b * 16 * 256;
        pj[(size_t)b] = PotrfJob{A, iv, NBLK, b * NBLK, ncols_host ? ncols_host[b] : NBLK};
        tj[(size_t)b] = TrinvJob{A, iv, dinv + (size_t)b * NBLK * NBLK, dinvt + (size_t)b * NBLK * NBLK, NBLK};
    }
    char *base = static_cast<char *>(jobs_dev);
    hipError_t e = hipMemcpy(base, pj.data(), sizeof(PotrfJob) * (size_t)nb, hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    const size_t off = ((sizeof(PotrfJob) * (size_t)nb + 255) / 256) * 256;
    return hipMemcpy(base + off, tj.data(), sizeof(TrinvJob) * (size_t)nb, hipMemcpyHostToDevice);
}

hipError_t block_chol_run(const void *jobs_dev, int nb, int *info_dev, double *minpiv_dev, hipStream_t st)
{
    const char *base = static_cast<const char *>(jobs_dev);
    const size_t off = ((sizeof(PotrfJob) * (size_t)nb + 255) / 256) * 256;
    nd::potrf_dispatch(8, reinterpret_cast<const PotrfJob *>(base), (unsigned)nb, st, info_dev, minpiv_dev);
    nd::launch_trinv(reinterpret_cast<const TrinvJob *>(base + off), nb, st);
    return hipGetLastError();
}

}  // namespace splpak
