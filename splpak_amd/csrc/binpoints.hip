// Binning of the data points by window: the first stage of the assembly on the GPU.
//
// The reference builds one dense row per data point and streams it through a
// dense Householder solver (splcw :788-855 -> suprls :1375-1695), O(ncol^2) work
// per row.  Each row has at most 4^ndim non-zeros, all inside one 4-wide window
// of nodes per dimension, so here the points are sorted by window ("cell") first: cell-ordered SoA copies of the
// coordinates, values and weights, the original index of every sorted point and the offsets of the cells (SortScratch).
// Points of zero weight are counted and not placed (:799, :891).  Inside a cell the points stand in ascending original
// index: the per-cell sums of gram.hip and residual.hip are taken in storage order, so this order is what makes a fit
// reproducible bit for bit.
//
// No floating-point atomics that could change a bit: the counts are integers, and the number of data rows is added to the
// fit's scalars as an integer-valued double, exact in any order.
//
// The default, a stable partition without global atomics (the long comment above SP_NT), in launch order:
//   sp_count_kernel        window key per point, per-block counts per bin
//   sp_colsum_kernel / sp_chunkscan_kernel / sp_binscan_kernel / sp_blockbase_kernel
//                          bin bases, and where every block's points of every bin start
//   sp_scatter_kernel      one level (a bin per cell): the points go to their sorted places; two levels: records sorted by bin
//   sp_bin2_kernel         two levels only (more cells than bins): a workgroup per bin sorts its records by cell
// The A/B route SPLPAK_BIN_ATOMIC (the form of rounds 1-4, also taken by grids of too many cells for the partition):
//   keys_kernel            window key per point + per-cell counts (integer atomics only)
//   scan_partials/segments exclusive scan of the counts (two launches over 256 segments)
//   scatter_kernel         counting-sort scatter into cell-ordered SoA copies (+ original index)
//   cell_order_kernel      orders the points INSIDE every cell by original index: the scatter's
//                          cursor order is not reproducible, the per-cell sums must be
// The refit:
//   regather_values_kernel new values on the points of the last binning
// HBM roofline: 8*(ndim+1+[weighted]) algorithmic bytes per point and streaming pass.
#include "assemble_dev.hpp"

namespace splpak {

namespace {

// ---------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(256)
keys_kernel(Grid g, long long m, const double *__restrict__ x, int ldx,
            const double *__restrict__ w, int *__restrict__ key, int *__restrict__ count,
            double *__restrict__ scal)
{
    double lrows = 0.0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        const double wv = w ? w[i] : 1.0;
        int k = g.ncell;                       // zero weight: ignored (:799, :891)
        if (wv != 0.0) {
            k = 0;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                int lo, hi;
                k += window_start(g, d, x[i * ldx + g.perm[d]], lo, hi) * g.cellstride[d];
            }
            lrows += 1.0;
        }
        key[i] = k;
        atomicAdd(&count[k], 1);
    }
    lrows = wave_sum(lrows);
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wv_id = threadIdx.x >> 6;
    if (lane == 0) red[wv_id] = lrows;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double b = red[0] + red[1] + red[2] + red[3];
        if (b != 0.0) atomicAdd(&scal[SC_NROWS_DATA], b);      // integer-valued: exact in any order
    }
}

// exclusive scan of count[0..n) into offset[0..n] in two launches over SCAN_SEG segments (round 3: one workgroup walking
// 227 000 cells took 0.35 ms per fit at 64^3): segment sums, then every workgroup scans its own segment on top of the
// sum of the segments before it
constexpr int SCAN_SEG = 256;
__global__ void __launch_bounds__(256)
scan_partials_kernel(const int *__restrict__ count, int *__restrict__ part, int n)
{
    __shared__ int red[4];
    const int per = (n + SCAN_SEG - 1) / SCAN_SEG;
    const int lo = blockIdx.x * per, hi = (lo + per < n) ? lo + per : n;
    int s = 0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) s += count[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void __launch_bounds__(256)
scan_segments_kernel(const int *__restrict__ count, const int *__restrict__ part, int *__restrict__ offset, int n)
{
    __shared__ int sc[256];
    __shared__ int sbase;
    const int t = threadIdx.x;
    {   // sum of the segments before this one
        int v = (t < (int)blockIdx.x) ? part[t] : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((t & 63) == 0) sc[t >> 6] = v;
        __syncthreads();
        if (t == 0) sbase = sc[0] + sc[1] + sc[2] + sc[3];
        __syncthreads();
    }
    const int per = (n + SCAN_SEG - 1) / SCAN_SEG;
    const int lo = blockIdx.x * per, hi = (lo + per < n) ? lo + per : n;
    const int chunk = (per + 255) / 256;                  // consecutive entries per thread
    const int a = lo + t * chunk, b = (a + chunk < hi) ? a + chunk : hi;
    int s = 0;
    for (int i = a; i < b; ++i) s += count[i];
    __syncthreads();
    sc[t] = s;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {         // Hillis-Steele inclusive scan
        const int v = (t >= o) ? sc[t - o] : 0;
        __syncthreads();
        sc[t] += v;
        __syncthreads();
    }
    int run = sbase + sc[t] - s;
    for (int i = a; i < b; ++i) { offset[i] = run; run += count[i]; }
    if (blockIdx.x == SCAN_SEG - 1 && t == 255) offset[n] = sbase + sc[255];
}

template <int D>
__global__ void __launch_bounds__(256)
scatter_kernel(Grid g, long long m, const double *__restrict__ x, int ldx,
               const double *__restrict__ y, const double *__restrict__ w,
               const int *__restrict__ key, const int *__restrict__ offset,
               int *__restrict__ cursor, double *__restrict__ xs, double *__restrict__ ys,
               double *__restrict__ ws, int *__restrict__ idx, long long cap)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        const int k = key[i];
        if (k >= g.ncell) continue;
        const long long pos = (long long)offset[k] + atomicAdd(&cursor[k], 1);
#pragma unroll
        for (int d = 0; d < D; ++d) xs[(long long)d * cap + pos] = x[i * ldx + g.perm[d]];
        ys[pos] = y[i];
        ws[pos] = w ? w[i] : 1.0;
        idx[pos] = (int)i;
    }
}

// Orders the points inside every cell by original index.  The scatter places them in the order in
// which its atomic cursor was served, which differs from run to run; the per-cell sums of the Gram
// and residual kernels are taken in storage order, so this is what makes the whole fit reproducible
// bit for bit.  One workgroup per cell.  Cells of up to ORDER_CAP points are permuted through an image
// in LDS.  Larger cells (round 4; up to ORDER_BIG_CAP points): the rank of every point is counted against
// the cell's original indices streamed through LDS in chunks of 1 024, the ordered indices are parked in
// `ordtmp` (SortScratch::ordtmp, or the key array, dead once the scatter has run) and the cell's image is rebuilt from the caller's
// arrays.  Cells beyond ORDER_BIG_CAP (65 536 points in ONE window of the grid) keep the scatter's order:
// their sums are correct, only not reproducible from run to run.
constexpr int ORDER_CAP = 1024;
constexpr int ORDER_BIG_CAP = 1 << 16;
template <int D>
__global__ void __launch_bounds__(256)
cell_order_kernel(Grid g, const int *__restrict__ offset, double *__restrict__ xs, double *__restrict__ ys,
                  double *__restrict__ ws, int *__restrict__ idx, long long cap, const double *__restrict__ x, int ldx,
                  const double *__restrict__ y, const double *__restrict__ w, int *__restrict__ ordtmp)
{
    __shared__ int sidx[ORDER_CAP];
    __shared__ double sv[ORDER_CAP * (D + 2)];
    const int cell = blockIdx.x;
    const long long beg = offset[cell];
    const int n = (int)(offset[cell + 1] - beg);
    if (n < 2 || n > ORDER_BIG_CAP) return;
    const int tid = threadIdx.x;
    if (n > ORDER_CAP) {
        for (int t0 = 0; t0 < n; t0 += ORDER_CAP) {           // a tile of 1 024 points: four per thread
            int me[4], rank[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int p = t0 + tid + 256 * u;
                me[u] = p < n ? idx[beg + p] : 0x7fffffff;
                rank[u] = 0;
            }
            for (int c0 = 0; c0 < n; c0 += ORDER_CAP) {
                __syncthreads();
                for (int p = tid; p < ORDER_CAP; p += 256) sidx[p] = c0 + p < n ? idx[beg + c0 + p] : 0x7fffffff;
                __syncthreads();
                const int cn = n - c0 < ORDER_CAP ? n - c0 : ORDER_CAP;
                for (int q = 0; q < cn; ++q) {
                    const int v = sidx[q];
#pragma unroll
                    for (int u = 0; u < 4; ++u) rank[u] += v < me[u] ? 1 : 0;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (t0 + tid + 256 * u < n) ordtmp[beg + rank[u]] = me[u];
        }
        __syncthreads();                                      // (the workgroup's own global writes are visible to it)
        for (int p = tid; p < n; p += 256) {
            const int i = ordtmp[beg + p];
            idx[beg + p] = i;
#pragma unroll
            for (int d = 0; d < D; ++d) xs[(long long)d * cap + beg + p] = x[(long long)i * ldx + g.perm[d]];
            ys[beg + p] = y[i];
            ws[beg + p] = w ? w[i] : 1.0;
        }
        return;
    }
    for (int p = tid; p < n; p += 256) {
        sidx[p] = idx[beg + p];
#pragma unroll
        for (int d = 0; d < D; ++d) sv[d * ORDER_CAP + p] = xs[(long long)d * cap + beg + p];
        sv[D * ORDER_CAP + p] = ys[beg + p];
        sv[(D + 1) * ORDER_CAP + p] = ws[beg + p];
    }
    __syncthreads();
    for (int p = tid; p < n; p += 256) {
        const int me = sidx[p];
        int rank = 0;
        for (int q = 0; q < n; ++q) rank += sidx[q] < me;
        const long long pos = beg + rank;
#pragma unroll
        for (int d = 0; d < D; ++d) xs[(long long)d * cap + pos] = sv[d * ORDER_CAP + p];
        ys[pos] = sv[D * ORDER_CAP + p];
        ws[pos] = sv[(D + 1) * ORDER_CAP + p];
        idx[pos] = me;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Stable partition of the points by window (round 5).  keys_kernel / scatter_kernel above bin with one global
// integer atomic per point and pass -- on the cell's counter, then on its cursor -- and scatter (ndim + 3) separate 8-byte
// words per point; the cursor's order is not reproducible, so cell_order_kernel re-sorts every cell by original index:
// 3.6 ms for the 1e7 points of BASELINE config 3 (0.04 of the HBM roofline), 0.42 of config 2's 2.0 ms (269 points on each of
// only 3 721 counters).  Here a counting sort WITHOUT global atomics that is stable by construction -- the points of a cell
// end up in ascending original index, which is exactly the order cell_order_kernel produced: the same bits downstream.
//
//   A block = SP_Q consecutive points, its 16 waves own 512 consecutive points each.
//   sp_count:    window key of every point (kept in `key`), bin = key / cpt (one level: cpt = 1, bin = cell; the last bin holds
//                the zero-weight points, :799); per-wave bin counts in LDS (16-bit halves of words, LDS atomics -- counting is
//                order-free), block totals -> row [block][bin] of the count matrix.
//   sp_colsum / sp_binscan / sp_blockbase: bin bases (exclusive scan of the bin totals) and, in place of every count, where that
//                block's points of that bin start: bins in order, blocks in order inside a bin.
//   sp_scatter:  the per-wave counts again, turned into exclusive prefixes over the waves; then every wave walks its 8 passes
//                of 64 points in order: a point's rank among the EARLIER lanes with its bin comes from the ballots of the
//                bin's bits (12 ballots: the lanes whose bin matches, below the own one), its wave's running count of the bin
//                from LDS -- the lowest lane of every group adds the group's size to it.  One level: the point goes straight
//                to its sorted place (SoA planes).  Two levels (more cells than bins: 64^3 has 226 981): a RECORD (coordinates,
//                y, w, index, cell) goes to the tile-sorted intermediate image, and
//   sp_bin2:     one workgroup per tile of cpt cells sorts the tile's records (contiguous: ~2 800 at config 3) by cell with the
//                same machinery -- per-wave counts, prefixes over waves and sub-blocks, ballot ranks -- writes their sorted
//                places and the offsets of its cells.
// Every count has one writer or is a sum; no order depends on timing: bitwise reproducible without a second sort.
constexpr int SP_NT = 1024, SP_NW = SP_NT / 64, SP_BITS = 12;
// doubles of a record: ndim coordinates, y, w, (index, cell) -- rounded up to an even count: records move as 16-byte words (a
// scattered store costs this chip ~7 cycles per lane and instruction whatever its width)
__host__ __device__ constexpr int sp_rec(int d) { return (d + 3 + 1) & ~1; }
static_assert(SP_NB == 1 << SP_BITS && SP_Q == SP_NW * 512, "bins / block shape");

template <int D>
__device__ inline int sp_cell_key(const Grid &g, const double *__restrict__ x, int ldx, const double *__restrict__ w, long long i)
{
    const double wv = w ? w[i] : 1.0;
    if (wv == 0.0) return g.ncell;             // zero weight: ignored (:799, :891)
    int k = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        int lo, hi;
        k += window_start(g, d, x[i * ldx + g.perm[d]], lo, hi) * g.cellstride[d];
    }
    return k;
}

// lanes of the wave whose `bin` equals this lane's (all lanes take part; inactive ones pass bin = -1 and are matched with nobody real)
__device__ inline unsigned long long sp_match(int bin, int bits)
{
    unsigned long long m = ~0ull;
    for (int b = 0; b < bits; ++b) {
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(((bin >> b) & 1) != 0);
        m &= ((bin >> b) & 1) ? bal : ~bal;
    }
    return m;
}

// per-wave bin counts of a block of up to SP_Q items: whist[wave][bin / 2], two 16-bit counts per word; nb bins in use.
// keyv[j]: the bin of the wave's item j * 64 + lane (-1: none)
template <int NBW>
__device__ inline void sp_wave_counts(unsigned (*whist)[NBW], int nb, const int (&binv)[8])
{
    const int tid = threadIdx.x, wave = tid >> 6;
    const int nw = (nb + 1) >> 1;
    for (int v = 0; v < SP_NW; ++v)
        for (int e = tid; e < nw; e += SP_NT) whist[v][e] = 0u;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (binv[j] >= 0) atomicAdd(&whist[wave][binv[j] >> 1], 1u << (16 * (binv[j] & 1)));
    __syncthreads();
}

// first level, counts: a block only needs its TOTALS per bin -- one histogram for all waves (16 KB of LDS: several workgroups
// per CU; with per-wave counts, 128 KB, the kernel ran one workgroup per CU at 0.38 ms for the 1e7 points of config 3)
template <int D>
__global__ void __launch_bounds__(SP_NT)
sp_count_kernel(Grid g, long long m, const double *__restrict__ x, int ldx, const double *__restrict__ w, int cpt,
                int *__restrict__ key, int *__restrict__ cntm)
{
    __shared__ int hist[SP_NB];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long base = (long long)blockIdx.x * SP_Q;
    const int n = (int)(m - base < SP_Q ? m - base : SP_Q);
    for (int b = tid; b < SP_NB; b += SP_NT) hist[b] = 0;
    __syncthreads();
    // (all loads of a thread's 8 points in flight together: one dependent round trip per point made this pass latency bound)
    double xv[8][D], wv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int p = wave * 512 + j * 64 + lane;
        const long long i = base + (p < n ? p : 0);
        wv[j] = p < n ? (w ? w[i] : 1.0) : 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) xv[j][d] = x[i * ldx + g.perm[d]];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int p = wave * 512 + j * 64 + lane;
        if (p < n) {
            int k = g.ncell;                       // zero weight: ignored (:799, :891)
            if (wv[j] != 0.0) {
                k = 0;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    int lo, hi;
                    k += window_start(g, d, xv[j][d], lo, hi) * g.cellstride[d];
                }
            }
            key[base + p] = k;
            atomicAdd(&hist[k < g.ncell ? k / cpt : SP_NB - 1], 1);
        }
    }
    __syncthreads();
    int *__restrict__ row = cntm + (long long)blockIdx.x * SP_NB;
    for (int b = tid; b < SP_NB; b += SP_NT) row[b] = hist[b];
    // (the number of data rows -- the points of non-zero weight -- is the base of the last bin: sp_binscan_kernel adds it to the
    //  fit's scalars, no f64 atomic per block.  What this kernel's 0.25-0.3 ms per 1e7 points are, measured by taking its parts
    //  out: 0.23 ms are the loads of the coordinates and weights themselves -- 1.4 TB/s, although all 32 of a thread are in
    //  flight together --, the key stores, LDS atomics and the row together 0.04)
}

// Count matrix [block][bin] -> in place: where the block's points of the bin start (bins in order, blocks in order inside a
// bin), and binbase = exclusive scan of the bin totals.  Four small launches: sums over chunks of SP_ROWS blocks, per bin the
// exclusive prefix over the chunks + its total, the scan of the totals, and the walk down every chunk.
constexpr int SP_ROWS = 16;        // blocks per chunk of the column sums
__global__ void __launch_bounds__(256)
sp_colsum_kernel(int nblk, const int *__restrict__ cntm, int *__restrict__ part)
{
    const int bin = blockIdx.x * 256 + threadIdx.x, ch = blockIdx.y;
    const int b0 = ch * SP_ROWS, b1 = b0 + SP_ROWS < nblk ? b0 + SP_ROWS : nblk;
    int v[SP_ROWS];
#pragma unroll
    for (int r = 0; r < SP_ROWS; ++r) v[r] = b0 + r < b1 ? cntm[(long long)(b0 + r) * SP_NB + bin] : 0;
    int s = 0;
#pragma unroll
    for (int r = 0; r < SP_ROWS; ++r) s += v[r];
    part[(long long)ch * SP_NB + bin] = s;
}
__global__ void __launch_bounds__(256)
sp_chunkscan_kernel(int nchunk, int *__restrict__ part, int *__restrict__ tot)
{
    const int bin = blockIdx.x * 256 + threadIdx.x;
    int run = 0, c = 0;
    for (; c + 8 <= nchunk; c += 8) {             // eight loads in flight (a dependent load per chunk: 1 us each)
        int v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = part[(long long)(c + u) * SP_NB + bin];
#pragma unroll
        for (int u = 0; u < 8; ++u) { part[(long long)(c + u) * SP_NB + bin] = run; run += v[u]; }
    }
    for (; c < nchunk; ++c) {
        const int v = part[(long long)c * SP_NB + bin];
        part[(long long)c * SP_NB + bin] = run;
        run += v;
    }
    tot[bin] = run;
}
__global__ void __launch_bounds__(1024)
sp_binscan_kernel(const int *__restrict__ tot, int *__restrict__ binbase, double *__restrict__ scal)
{
    __shared__ int sc[1024];
    const int t = threadIdx.x;
    int v[4], sum = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) { v[u] = tot[4 * t + u]; sum += v[u]; }
    sc[t] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int a = t >= o ? sc[t - o] : 0;
        __syncthreads();
        sc[t] += a;
        __syncthreads();
    }
    int run = sc[t] - sum;
#pragma unroll
    for (int u = 0; u < 4; ++u) { binbase[4 * t + u] = run; run += v[u]; }
    if (t == 1023) {
        binbase[SP_NB] = run;
        const int nvalid = run - v[3];              // everything below the last bin (which holds the zero-weight points)
        if (nvalid) atomicAdd(&scal[SC_NROWS_DATA], (double)nvalid);      // integer-valued: exact in any order
    }
}
__global__ void __launch_bounds__(256)
sp_blockbase_kernel(int nblk, int *__restrict__ cntm, const int *__restrict__ part, const int *__restrict__ binbase)
{
    const int bin = blockIdx.x * 256 + threadIdx.x, ch = blockIdx.y;
    const int b0 = ch * SP_ROWS, b1 = b0 + SP_ROWS < nblk ? b0 + SP_ROWS : nblk;
    int v[SP_ROWS];
#pragma unroll
    for (int r = 0; r < SP_ROWS; ++r) v[r] = b0 + r < b1 ? cntm[(long long)(b0 + r) * SP_NB + bin] : 0;
    int run = binbase[bin] + part[(long long)ch * SP_NB + bin];
#pragma unroll
    for (int r = 0; r < SP_ROWS; ++r) {
        if (b0 + r < b1) cntm[(long long)(b0 + r) * SP_NB + bin] = run;
        run += v[r];
    }
}

// the stable places of a block's items: place(j, pos) is called once per item j * 64 + lane of the wave with binv[j] >= 0, pos =
// bbase[bin] + items of the bin before it in the block.  whist: the per-wave counts (sp_wave_counts), turned into running
// exclusive prefixes here.
template <int NBW>
__device__ inline void sp_wave_prefix(unsigned (*whist)[NBW], int nb)
{
    for (int b2 = threadIdx.x; b2 < ((nb + 1) >> 1); b2 += SP_NT) {         // exclusive prefixes over the waves, both halves of a word at once
        unsigned run = 0;
#pragma unroll
        for (int v = 0; v < SP_NW; ++v) {
            const unsigned c = whist[v][b2];
            whist[v][b2] = run;
            run += c;
        }
    }
    __syncthreads();
}
// (passes J0 .. J1 - 1 of the wave: a caller that has to LOAD what it places splits the eight passes in two, so that the loads of
//  four passes are in flight together without their registers exceeding the budget)
template <int J0, int J1, int NBW, typename Place>
__device__ inline void sp_places(unsigned (*whist)[NBW], const int *bbase, int bits, const int (&binv)[8], Place &&place)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int j = J0; j < J1; ++j) {
        const int bin = binv[j];
        const unsigned long long mm = sp_match(bin, bits + 1);          // (+ 1: bit `bits` tells -1 from every real bin)
        if (bin >= 0) {
            const unsigned wv = whist[wave][bin >> 1];
            const int before = (int)((wv >> (16 * (bin & 1))) & 0xffffu) + __builtin_popcountll(mm & lt);
            place(j, bbase[bin] + before);
        }
        __builtin_amdgcn_wave_barrier();                               // (every lane has read its running count)
        if (bin >= 0 && (mm & lt) == 0) atomicAdd(&whist[wave][bin >> 1], (unsigned)__builtin_popcountll(mm) << (16 * (bin & 1)));
        __builtin_amdgcn_wave_barrier();
    }
}
template <int NBW, typename Place>
__device__ inline void sp_stable_places(unsigned (*whist)[NBW], const int *bbase, int nb, int bits, const int (&binv)[8], Place &&place)
{
    sp_wave_prefix(whist, nb);
    sp_places<0, 8>(whist, bbase, bits, binv, place);
}

// RECORD of a point on its way through the tile-sorted image: ndim coordinates (internal order), y, w, (index, cell)
template <int D>
__global__ void __launch_bounds__(SP_NT)
sp_scatter_kernel(Grid g, long long m, const double *__restrict__ x, int ldx, const double *__restrict__ y, const double *__restrict__ w,
                  int cpt, int nb, const int *__restrict__ key, const int *__restrict__ cntm, double *__restrict__ rec,
                  double *__restrict__ xs, double *__restrict__ ys, double *__restrict__ ws, int *__restrict__ idx, long long cap)
{
    __shared__ unsigned whist[SP_NW][SP_NB / 2];
    __shared__ int bbase[SP_NB];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long base = (long long)blockIdx.x * SP_Q;
    const int n = (int)(m - base < SP_Q ? m - base : SP_Q);
    for (int b = tid; b < nb; b += SP_NT) bbase[b] = cntm[(long long)blockIdx.x * SP_NB + b];
    // the wave's 8 x 64 points, all loads of a thread in flight together (the walk below is LDS and stores only)
    int kk[8], binv[8];
    double xv[8][D], yv[8], wv[8];
    // (UNCONDITIONAL loads, the index clamped for the tail of the last block: loads under `valid ? load : 0` wait for the key and
    //  then for each other -- eight serialised round trips per wave, 0.82 of this kernel's 1.05 ms per 1e7 points, found by taking
    //  the rest of the kernel out)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int p = wave * 512 + j * 64 + lane;
        const long long i = base + (p < n ? p : 0);
        kk[j] = key[i];
#pragma unroll
        for (int d = 0; d < D; ++d) xv[j][d] = x[i * ldx + g.perm[d]];
        yv[j] = y[i];
        wv[j] = w ? w[i] : 1.0;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int p = wave * 512 + j * 64 + lane;
        if (p >= n) kk[j] = -1;
        const bool ok = kk[j] >= 0 && kk[j] < g.ncell;
        binv[j] = ok ? kk[j] / cpt : -1;                                // zero weight: neither counted nor placed here
    }
    sp_wave_counts(whist, nb, binv);
    sp_stable_places(whist, bbase, nb, SP_BITS, binv, [&](int j, int pos) {
        const int i = (int)(base + wave * 512 + j * 64 + lane);
        if (rec) {
            constexpr int R = sp_rec(D);
            double v[R];
#pragma unroll
            for (int d = 0; d < D; ++d) v[d] = xv[j][d];
            v[D] = yv[j];
            v[D + 1] = wv[j];
            v[D + 2] = __hiloint2double(kk[j], i);                       // (low word: index, high word: cell)
#pragma unroll
            for (int e = D + 3; e < R; ++e) v[e] = 0.0;
            d2_t *__restrict__ r = reinterpret_cast<d2_t *>(rec + (long long)pos * R);
#pragma unroll
            for (int e = 0; e < R / 2; ++e) r[e] = (d2_t){v[2 * e], v[2 * e + 1]};
        } else {
#pragma unroll
            for (int d = 0; d < D; ++d) xs[(long long)d * cap + pos] = xv[j][d];
            ys[pos] = yv[j];
            ws[pos] = wv[j];
            idx[pos] = i;
        }
    });
}

// second level: workgroup = tile of cpt cells; its records (binbase[tile] .. binbase[tile + 1]) -> sorted places by cell.
// NB2: capacity in cells of a tile (256; SP_NB for grids beyond ~1e6 cells).  A tile of at most SP_STAGE records (config 3: ~2 500)
// is assembled in LDS -- planes of coordinates, y, w, index in sorted order -- and leaves with consecutive stores; larger tiles
// (clustered data) are walked in sub-blocks of SP_Q records and scattered straight into place.
constexpr int SP_STAGE = 2816;      // (x 52 bytes in 4-D + the counters: 157 KB of the 160 KB LDS)
template <int D, int NB2>
__global__ void __launch_bounds__(SP_NT)
sp_bin2_kernel(Grid g, int cpt, int ntile, const int *__restrict__ binbase, const double *__restrict__ rec, int *__restrict__ offset,
               double *__restrict__ xs, double *__restrict__ ys, double *__restrict__ ws, int *__restrict__ idx, long long cap)
{
    constexpr int R = sp_rec(D);
    __shared__ unsigned whist[SP_NW][NB2 / 2];
    __shared__ int bbase[NB2], btot[NB2];                             // [local cell]: where its next sub-block's records start / totals
    __shared__ double stage[NB2 <= 256 ? SP_STAGE * (D + 2) : 1];
    __shared__ int stidx[NB2 <= 256 ? SP_STAGE : 1];
    const int tile = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tb = binbase[tile], te = binbase[tile + 1];
    const int c0 = tile * cpt, nc = min(cpt, g.ncell - c0);
    int bits = 1;
    while ((1 << bits) < nc) ++bits;
    auto cell_at = [&](int q) { return __double2hiint(rec[(long long)q * R + D + 2]) - c0; };       // local cell of record q
    // cell totals of the whole tile, then their exclusive prefix = the cells' offsets
    for (int b = tid; b < nc; b += SP_NT) btot[b] = 0;
    __syncthreads();
    for (int q = tb + tid; q < te; q += SP_NT) atomicAdd(&btot[cell_at(q)], 1);
    __syncthreads();
    if (tid < 64) {                                                    // exclusive scan over the nc cells by one wave
        int carry = tb;
        for (int b0 = 0; b0 < nc; b0 += 64) {
            const int v = b0 + lane < nc ? btot[b0 + lane] : 0;
            int inc = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(inc, o, 64);
                if (lane >= o) inc += t;
            }
            if (b0 + lane < nc) bbase[b0 + lane] = carry + inc - v;
            carry += __shfl(inc, 63, 64);
        }
    }
    __syncthreads();
    for (int b = tid; b < nc; b += SP_NT) offset[c0 + b] = bbase[b];
    if (tile == ntile - 1 && tid == 0) offset[g.ncell] = te;
    const bool staged = NB2 <= 256 && te - tb <= SP_STAGE;
    for (int sb0 = 0; sb0 < te - tb; sb0 += SP_Q) {
        const int n = min(SP_Q, te - tb - sb0);
        int binv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int p = wave * 512 + j * 64 + lane;
            const int c = cell_at(tb + sb0 + (p < n ? p : 0));          // (unconditional load, index clamped)
            binv[j] = p < n ? c : -1;
        }
        sp_wave_counts(whist, nc, binv);
        // (the sub-block's totals, for the next sub-block's bases -- taken before the counts become prefixes)
        for (int b = tid; b < nc; b += SP_NT) {
            unsigned t = 0;
            for (int v = 0; v < SP_NW; ++v) t += (whist[v][b >> 1] >> (16 * (b & 1))) & 0xffffu;
            btot[b] = (int)t;
        }
        __syncthreads();
        sp_wave_prefix(whist, nc);
        // (the records of four passes are loaded together, UNCONDITIONALLY -- index clamped --: a load per pass inside the walk was
        //  a dependent memory round trip per pass and wave)
        d2_t rv[4][R / 2];
        auto preload = [&](int j0) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int p = wave * 512 + (j0 + jj) * 64 + lane;
                const d2_t *__restrict__ r = reinterpret_cast<const d2_t *>(rec + (long long)(tb + sb0 + (p < n ? p : 0)) * R);
#pragma unroll
                for (int e = 0; e < R / 2; ++e) rv[jj][e] = r[e];
            }
        };
        auto place = [&](int j, int pos) {
            double v[R];
#pragma unroll
            for (int e = 0; e < R / 2; ++e) { v[2 * e] = rv[j & 3][e][0]; v[2 * e + 1] = rv[j & 3][e][1]; }
            if (staged) {
                const int l = pos - tb;
#pragma unroll
                for (int d = 0; d < D + 2; ++d) stage[d * SP_STAGE + l] = v[d];
                stidx[l] = __double2loint(v[D + 2]);
            } else {
#pragma unroll
                for (int d = 0; d < D; ++d) xs[(long long)d * cap + pos] = v[d];
                ys[pos] = v[D];
                ws[pos] = v[D + 1];
                idx[pos] = __double2loint(v[D + 2]);
            }
        };
        preload(0);
        sp_places<0, 4>(whist, bbase, bits, binv, place);
        preload(4);
        sp_places<4, 8>(whist, bbase, bits, binv, place);
        __syncthreads();
        for (int b = tid; b < nc; b += SP_NT) bbase[b] += btot[b];
        __syncthreads();
    }
    if (staged) {
        const int n = te - tb;
        for (int e = tid; e < n; e += SP_NT) {
#pragma unroll
            for (int d = 0; d < D; ++d) xs[(long long)d * cap + tb + e] = stage[d * SP_STAGE + e];
            ys[tb + e] = stage[D * SP_STAGE + e];
            ws[tb + e] = stage[(D + 1) * SP_STAGE + e];
            idx[tb + e] = stidx[e];
        }
    }
}

}  // namespace

// cells per bin of the stable partition's first level (1: the bins ARE the cells); 0: the grid has too many cells for it
static int sp_cells_per_bin(const Grid &g)
{
    const long long cpt = ((long long)g.ncell + SP_NB - 2) / (SP_NB - 1);
    return cpt <= SP_NB - 1 ? (int)(cpt < 1 ? 1 : cpt) : 0;
}

long long bin_record_doubles(const Grid &g, long long max_ndata)
{
    const int cpt = sp_cells_per_bin(g);
    return cpt > 1 ? max_ndata * (long long)sp_rec(g.ndim) : 0;
}

int bin_route(const Grid &g, const SortScratch &s, int *cpt_out)
{
    const bool old_form = splpak::opt_get("SPLPAK_BIN_ATOMIC") != nullptr;      // A/B switch: rounds 1-4 (global atomics + in-cell re-sort)
    const int cpt = sp_cells_per_bin(g);
    if (cpt_out) *cpt_out = cpt;
    if (old_form || cpt <= 0 || !s.cntm || !s.binbase || !s.sppart || (cpt > 1 && !s.rec)) return 0;
    return cpt == 1 ? 1 : cpt <= 256 ? 2 : 3;
}

hipError_t launch_bin_points(const Grid &g, long long m, const double *x, int ldx, const double *y,
                             const double *w, const SortScratch &s, double *scal, hipStream_t st)
{
    int cpt = 0;
    const int route = bin_route(g, s, &cpt);
    if (route != 0) {
        if (m <= 0) return hipMemsetAsync(s.offset, 0, sizeof(int) * (size_t)(g.ncell + 2), st);
        const int nblk = (int)((m + SP_Q - 1) / SP_Q), nchunk = (nblk + SP_ROWS - 1) / SP_ROWS;
        double *rec = cpt > 1 ? s.rec : nullptr;
        const int ntile = (g.ncell + cpt - 1) / cpt;                   // bins in use (one level: the cells)
        int *tot = s.binbase + SP_NB + 8;
        DISPATCH_D(g.ndim, hipLaunchKernelGGL(sp_count_kernel<D>, dim3((unsigned)nblk), dim3(SP_NT), 0, st, g, m, x, ldx, w, cpt, s.key, s.cntm));
        hipLaunchKernelGGL(sp_colsum_kernel, dim3(SP_NB / 256, (unsigned)nchunk), dim3(256), 0, st, nblk, s.cntm, s.sppart);
        hipLaunchKernelGGL(sp_chunkscan_kernel, dim3(SP_NB / 256), dim3(256), 0, st, nchunk, s.sppart, tot);
        hipLaunchKernelGGL(sp_binscan_kernel, dim3(1), dim3(1024), 0, st, tot, s.binbase, scal);
        hipLaunchKernelGGL(sp_blockbase_kernel, dim3(SP_NB / 256, (unsigned)nchunk), dim3(256), 0, st, nblk, s.cntm, s.sppart, s.binbase);
        DISPATCH_D(g.ndim, hipLaunchKernelGGL(sp_scatter_kernel<D>, dim3((unsigned)nblk), dim3(SP_NT), 0, st, g, m, x, ldx, y, w, cpt, ntile, s.key,
                                              s.cntm, rec, s.xs, s.ys, s.ws, s.idx, s.cap));
        if (route == 1)    // the bins are the cells: their bases are the offsets (bins ncell .. SP_NB - 2 are empty)
            return hipMemcpyAsync(s.offset, s.binbase, sizeof(int) * (size_t)(g.ncell + 1), hipMemcpyDeviceToDevice, st);
        if (route == 2) {
            DISPATCH_D(g.ndim, hipLaunchKernelGGL((sp_bin2_kernel<D, 256>), dim3((unsigned)ntile), dim3(SP_NT), 0, st, g, cpt, ntile, s.binbase,
                                                  rec, s.offset, s.xs, s.ys, s.ws, s.idx, s.cap));
        } else {
            DISPATCH_D(g.ndim, hipLaunchKernelGGL((sp_bin2_kernel<D, SP_NB>), dim3((unsigned)ntile), dim3(SP_NT), 0, st, g, cpt, ntile, s.binbase,
                                                  rec, s.offset, s.xs, s.ys, s.ws, s.idx, s.cap));
        }
        return hipGetLastError();
    }
    hipError_t e = hipMemsetAsync(s.count, 0, sizeof(int) * (size_t)(g.ncell + 2), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(s.cursor, 0, sizeof(int) * (size_t)(g.ncell + 1), st);
    if (e != hipSuccess) return e;
    if (m > 0) {
        dim3 gr(grid_for(m, 256)), bl(256);
        DISPATCH_D(g.ndim, hipLaunchKernelGGL(keys_kernel<D>, gr, bl, 0, st, g, m, x, ldx, w, s.key, s.count, scal));
    }
    hipLaunchKernelGGL(scan_partials_kernel, dim3(SCAN_SEG), dim3(256), 0, st, s.count, s.scanpart, g.ncell + 1);
    hipLaunchKernelGGL(scan_segments_kernel, dim3(SCAN_SEG), dim3(256), 0, st, s.count, s.scanpart, s.offset, g.ncell + 1);
    if (m > 0) {
        dim3 gr(grid_for(m, 256)), bl(256);
        DISPATCH_D(g.ndim, hipLaunchKernelGGL(scatter_kernel<D>, gr, bl, 0, st, g, m, x, ldx, y, w,
                                              s.key, s.offset, s.cursor, s.xs, s.ys, s.ws, s.idx, s.cap));
        DISPATCH_D(g.ndim, hipLaunchKernelGGL(cell_order_kernel<D>, dim3((unsigned)g.ncell), dim3(256), 0, st, g,
                                              s.offset, s.xs, s.ys, s.ws, s.idx, s.cap, x, ldx, y, w, s.ordtmp ? s.ordtmp : s.key));
    }
    return hipGetLastError();
}

// New values on the points of the last binning (the refit): ys_out[pos] = y[idx[pos]].  The stores and the reads of idx are
// consecutive per wave; the reads of y are the scattered side -- the points of a cell are ordered by original index, so a wave
// mostly walks ascending addresses -- and four of them per thread are in flight together (the kernel does nothing but wait for
// them).  The binning placed offset[ncell] points (a zero-weight point is counted, not placed): the positions behind them hold
// no point, their idx is not read, and they are given 0; no weight ever reads them.
__global__ void __launch_bounds__(256)
regather_values_kernel(long long n, const int *__restrict__ placed, const int *__restrict__ idx, const double *__restrict__ y,
                       double *__restrict__ ys)
{
    const long long np = min((long long)*placed, n);
    const long long tile = 4LL * blockDim.x, stride = (long long)gridDim.x * tile;
    for (long long p0 = (long long)blockIdx.x * tile + threadIdx.x; p0 < n; p0 += stride) {
        long long src[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long pos = p0 + (long long)u * blockDim.x;
            src[u] = pos < np ? (long long)idx[pos] : -1;
        }
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = y[src[u] < 0 ? 0 : src[u]];      // (unconditional loads: four in flight)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long pos = p0 + (long long)u * blockDim.x;
            if (pos < n) ys[pos] = src[u] < 0 ? 0.0 : v[u];
        }
    }
}

hipError_t launch_regather_values(const Grid &g, const SortScratch &s, long long n, const double *y, double *ys_out, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    if (n > s.cap) return hipErrorInvalidValue;
    hipLaunchKernelGGL(regather_values_kernel, dim3(grid_for(n, 1024, 2048)), dim3(256), 0, st, n, s.offset + g.ncell,
                       s.idx, y, ys_out);
    return hipGetLastError();
}

}  // namespace splpak
