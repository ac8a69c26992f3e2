// Region sort: the first of the sorted evaluation paths and the one every grid of up to BIN_MAX regions can take
// (2-D grids, grids of more than 256 regions, the fused derivative evaluation).
//
// Random queries make every window row a separate 128-byte L2 line (~19 lines = 2.4 KB of L2
// traffic per 3-D query, for 512 useful bytes): the direct kernel sits at the L2 gather ceiling.
// The binned path sorts a chunk of queries by REGION -- a box of window starts whose
// coefficients (box + 3 nodes per dimension, 4096 doubles = 32 KB) fit in LDS -- and evaluates
// every region's queries from an LDS copy of its coefficients: the gathers become LDS reads, the
// global traffic per query is its coordinates, a permutation index and the result.
//   pass A  bin_count_kernel    region histogram of the chunk + per-workgroup region counts
//           bin_scan_kernel     offsets and workgroups per region
//           bin_wgbase_kernel   where every pass-B workgroup's runs start (prefix over workgroups)
//   pass B  bin_scatter_kernel  coordinates + original index copied into region order
//   pass C  eval_binned_kernel  one workgroup per (region, 2048 queries)
// The arithmetic per query is window_table + window_sum exactly as in the direct kernel, so both
// paths return identical bits; only the order in which queries are processed differs.
#include "evalpaths.hpp"
#include "evalscratch.hpp"

namespace splpak {

constexpr int BIN_MAX = 2048;          // regions per grid handled by the LDS histograms

template <int D> struct ScatterShape { static constexpr int QPT = D == 4 ? 4 : 8; };   // queries per thread in passes A and B

// Pass A.  Workgroup w counts the SAME 256*QPT queries that workgroup w of pass B will place, and
// leaves its per-region counts in row w of `cnt`; the column-wise prefix of that matrix
// (bin_wgbase_kernel) then tells every pass-B workgroup where each of its runs starts.  No workgroup
// ever waits on a global atomic (round 2: 2 050 workgroups taking turns on 125 cursor words cost 42 of
// the 80 us of pass B), and the sorted order is a function of the input alone.
template <int D, typename T>
__global__ void __launch_bounds__(256)
bin_count_kernel(Grid g, Regions rg, int n, const T *__restrict__ xq, int ldxq, int *__restrict__ cnt, int ldw)
{
    constexpr int QPT = ScatterShape<D>::QPT;
    __shared__ int lh[BIN_MAX];
    for (int b = threadIdx.x; b < rg.nbins; b += 256) lh[b] = 0;
    __syncthreads();
    const int base = blockIdx.x * (256 * QPT);
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        const int i = base + j * 256 + threadIdx.x;
        if (i < n) {
            double x[D];
#pragma unroll
            for (int d = 0; d < D; ++d) x[d] = (double)xq[(long long)i * ldxq + d];
            atomicAdd(&lh[region_of<D>(g, rg, x)], 1);
        }
    }
    __syncthreads();
    (void)ldw;
    for (int b = threadIdx.x; b < rg.nbins; b += 256) cnt[(long long)blockIdx.x * rg.nbins + b] = lh[b];   // row = this workgroup, consecutive regions: coalesced
}

// The count matrix is cnt[workgroup][region] (round 3: the transposed layout made every workgroup of pass A write, and of
// pass B read, one 4-byte word per 32-byte sector -- 680 MB of traffic each for the 85 MB matrix of a 4-D batch: 1 296
// regions x 16 384 workgroups; profiles/r03_eval_pmc.json).  Column sums and prefixes over a row-major matrix: a thread
// owns a region (consecutive threads = consecutive regions = coalesced rows), workgroups own chunks of BIN_ROWS rows.
constexpr int BIN_ROWS = 128;
// part[c][b] = sum of cnt[w][b] over the rows w of chunk c; grid (ceil(nbins / 256), nchunk)
__global__ void __launch_bounds__(256)
bin_colsum_kernel(int nwg, int nbins, const int *__restrict__ cnt, int *__restrict__ part)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nbins) return;
    const int w0 = blockIdx.y * BIN_ROWS, w1 = (w0 + BIN_ROWS < nwg) ? w0 + BIN_ROWS : nwg;
    int sum = 0;
    for (int w = w0; w < w1; ++w) sum += cnt[(long long)w * nbins + b];
    part[(long long)blockIdx.y * nbins + b] = sum;
}
// hist[b] = sum_c part[c][b];  part[c][b] <- sum_{c' < c} part[c'][b]   (thread = region)
__global__ void __launch_bounds__(256)
bin_total_kernel(int nchunk, int nbins, int *__restrict__ part, int *__restrict__ hist)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nbins) return;
    int run = 0;
    for (int c = 0; c < nchunk; ++c) {
        const int v = part[(long long)c * nbins + b];
        part[(long long)c * nbins + b] = run;
        run += v;
    }
    hist[b] = run;
}
// cnt[w][b] <- off[b] + (queries of region b in the workgroups before w): first sorted position of workgroup w's run
__global__ void __launch_bounds__(256)
bin_wgbase_kernel(int nwg, int nbins, const int *__restrict__ off, const int *__restrict__ part, int *__restrict__ cnt)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nbins) return;
    const int w0 = blockIdx.y * BIN_ROWS, w1 = (w0 + BIN_ROWS < nwg) ? w0 + BIN_ROWS : nwg;
    int run = off[b] + part[(long long)blockIdx.y * nbins + b];
    for (int w = w0; w < w1; ++w) {
        const int c = cnt[(long long)w * nbins + b];
        cnt[(long long)w * nbins + b] = run;
        run += c;
    }
}

// ints: hist[nbins] | off[nbins+1] | cursor[nbins] | wgoff[nbins+1]
__global__ void __launch_bounds__(256)
bin_scan_kernel(int nbins, const int *__restrict__ hist, int *__restrict__ off, int *__restrict__ cursor,
                int *__restrict__ wgoff)
{
    __shared__ int sq[256], sw[256];
    const int per = (nbins + 255) / 256;
    const int b0 = threadIdx.x * per;
    int q = 0, w = 0;
    for (int b = b0; b < b0 + per && b < nbins; ++b) {
        q += hist[b];
        w += (hist[b] + EVAL_QPW - 1) / EVAL_QPW;
    }
    sq[threadIdx.x] = q;
    sw[threadIdx.x] = w;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
        const int aq = threadIdx.x >= s ? sq[threadIdx.x - s] : 0;
        const int aw = threadIdx.x >= s ? sw[threadIdx.x - s] : 0;
        __syncthreads();
        sq[threadIdx.x] += aq;
        sw[threadIdx.x] += aw;
        __syncthreads();
    }
    q = sq[threadIdx.x] - q;          // exclusive
    w = sw[threadIdx.x] - w;
    for (int b = b0; b < b0 + per && b < nbins; ++b) {
        off[b] = q;
        cursor[b] = q;
        wgoff[b] = w;
        q += hist[b];
        w += (hist[b] + EVAL_QPW - 1) / EVAL_QPW;
    }
    if (threadIdx.x == 255) {
        off[nbins] = sq[255];
        wgoff[nbins] = sw[255];
    }
}

// Pass B.  The workgroup sorts its queries by region in LDS first, so that the copy to global
// memory walks every region's run with consecutive lanes on consecutive addresses (the
// straightforward per-query scatter issued one 8-byte store request per coordinate and was
// bound by the request rate, not by bytes).
template <int D, typename T>
__global__ void __launch_bounds__(256)
bin_scatter_kernel(Grid g, Regions rg, int n, const T *__restrict__ xq, int ldxq,
                   const int *__restrict__ wgbase, int ldw, double *__restrict__ xs)
{
    constexpr int QPT = ScatterShape<D>::QPT, QPW = 256 * QPT;
    __shared__ double sx[QPW * D];
    __shared__ int sidx[QPW];
    __shared__ unsigned short srid[QPW];
    extern __shared__ int lds_bins[];          // lh[nbins] | lbase[nbins]: sized by the launch, not by BIN_MAX
    int *lh = lds_bins, *lbase = lds_bins + rg.nbins;
    __shared__ int sscan[256];
    for (int b = threadIdx.x; b < rg.nbins; b += 256) lh[b] = 0;
    __syncthreads();
    const int base = blockIdx.x * QPW;
    int rid[QPT], rank[QPT];
    double xr[QPT][D];
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        const int i = base + j * 256 + threadIdx.x;
        rid[j] = -1;
        rank[j] = 0;
        if (i < n) {
#pragma unroll
            for (int d = 0; d < D; ++d) xr[j][d] = (double)xq[(long long)i * ldxq + d];
            rid[j] = region_of<D>(g, rg, xr[j]);
            rank[j] = atomicAdd(&lh[rid[j]], 1);
        }
    }
    __syncthreads();
    // exclusive scan of the local counts; lh[b] <- local start, lbase[b] <- global start - local start
    const int per = (rg.nbins + 255) / 256;
    const int b0 = threadIdx.x * per;
    int q = 0;
    for (int b = b0; b < b0 + per && b < rg.nbins; ++b) q += lh[b];
    sscan[threadIdx.x] = q;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
        const int aq = threadIdx.x >= s ? sscan[threadIdx.x - s] : 0;
        __syncthreads();
        sscan[threadIdx.x] += aq;
        __syncthreads();
    }
    q = sscan[threadIdx.x] - q;
    for (int b = b0; b < b0 + per && b < rg.nbins; ++b) {
        const int c = lh[b];
        lh[b] = q;
        lbase[b] = wgbase[(long long)blockIdx.x * rg.nbins + b] - q;
        q += c;
    }
    const int total = sscan[255];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        if (rid[j] < 0) continue;
        const int i = base + j * 256 + threadIdx.x;
        const int lp = lh[rid[j]] + rank[j];
#pragma unroll
        for (int d = 0; d < D; ++d) sx[d * QPW + lp] = xr[j][d];
        sidx[lp] = i;
        srid[lp] = (unsigned short)rid[j];
    }
    __syncthreads();
    // copy-out: consecutive lanes walk a region's run, one record each (consecutive 32- / 40-byte pieces)
    for (int lp = threadIdx.x; lp < total; lp += 256) {
        const long long gpos = lp + lbase[srid[lp]];
        double x[D];
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = sx[d * QPW + lp];
        store_record<D>(xs + gpos * (D + 1), x, sidx[lp]);
    }
}

// T = storage type of the coefficients and the results (double, or float for the REAL32 entry points: widened when the
// tile is filled / narrowed when a result is stored; the sorted coordinates are always double, the arithmetic too)
// (8 waves per SIMD: two of these 16-wave workgroups per CU need <= 64 registers -- the 4-D instantiation came out at 65 and
// ran ONE workgroup per CU until round 3)
template <int D, bool VAL, typename T>
__global__ void __launch_bounds__(EVAL_WG, 8)
eval_binned_kernel(Grid g, Regions rg, NDeriv nd, const T *__restrict__ coef,
                   const double *__restrict__ xs,
                   const int *__restrict__ off, const int *__restrict__ wgoff, T *__restrict__ out)
{
    constexpr int TILE_ELEMS = tile_elems<D>();
    __shared__ double tile[TILE_ELEMS];
    using TS = TileShape<D>;
    const int wg = blockIdx.x;
    if (wg >= wgoff[rg.nbins]) return;
    int lo = 0, hi = rg.nbins;               // wgoff[lo] <= wg < wgoff[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (wgoff[mid] <= wg) lo = mid; else hi = mid;
    }
    const int r = lo;                         // wgoff[r] <= wg < wgoff[r+1]: a non-empty region
    const int part = wg - wgoff[r];
    int a[D];                                  // first node of the region's tile
    {
        int rr = r;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            a[d] = (rr % rg.nreg[d]) * (TS::T[d] - 3);
            rr /= rg.nreg[d];
        }
    }
    using TT = TileStride<D>;
    __shared__ int s_cnt[32], s_off[32], s_fre[33];
    constexpr bool DEAL = D == 4;             // queries dealt to the lanes by LDS bank class (below; 3-D: 403 -> 476 us, the class sort costs more than the conflicts)
    __shared__ unsigned short s_list[DEAL ? EVAL_QPW : 1], s_ovf[DEAL ? EVAL_QPW : 1];
    if (DEAL && threadIdx.x < 32) s_cnt[threadIdx.x] = 0;
    for (int e = threadIdx.x; e < tile_cells<D>(); e += EVAL_WG) {
        int rem = e, idx = 0, te = 0;
        bool ok = true;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int l = rem % TS::T[d];
            rem /= TS::T[d];
            const int node = a[d] + l;
            ok = ok && node < g.nodes[d];
            idx += node * g.colstride[d];
            te += l * TT::S[d];
        }
        tile[te] = ok ? (double)coef[idx] : 0.0;
    }
    __syncthreads();
    const int qb = off[r] + part * EVAL_QPW;
    const int qe = min(off[r + 1], qb + EVAL_QPW);
    constexpr int t1 = TT::S[1], t2 = TT::S[2], t3 = TT::S[3];
    auto evaluate = [&](const double (&x)[D], int p) {
        double b[D][4];
        int base = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int ws = eval_table<VAL>(g, d, x[d], nd.v[d], b[d]);
            base += (ws - a[d]) * TT::S[d];
        }
        const double sum = window_sum<D>(b, [&](int k1, int k2, int k3, double (&c)[4]) {
            lds_row4(tile, base + k1 * t1 + k2 * t2 + k3 * t3, c);
        });
        out[p] = (T)sum;
    };
    if constexpr (DEAL) {
        // Queries dealt to the lanes by bank class: lane h of every 32-lane half takes the queries whose tile offset is
        // h mod 32 (counting sort of the workgroup's <= 2 048 queries by that class in LDS).  The 64 window rows of a query are
        // read at the same constant offsets from its base by every lane, so lanes with distinct base classes never meet on a
        // bank: 2 LDS cycles per read instead of the ~10 of random windows.  Same arithmetic per query: identical bits.
        // A class holds 64 +- 8 of the 2 048 queries; every lane has exactly two rounds (64 slots per class = one per
        // half-wave and round), so what a class holds beyond 64 goes to the free slots of the short classes -- those few
        // lanes meet the lane of their own class on a bank (one extra LDS cycle), nobody idles.
        static_assert(EVAL_QPW == 2 * EVAL_WG && EVAL_WG == 32 * 32, "two rounds of 32 half-waves x 32 classes");
        const int nq = qe - qb;
        int key[2] = {-1, -1}, rk[2] = {0, 0};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int jj = (int)threadIdx.x + u * EVAL_WG;
            if (jj < nq) {
                double x[D];
                (void)load_record<D>(xs + (long long)(qb + jj) * (D + 1), x);
                int base = 0;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    int lo, hi;
                    base += (window_start(g, d, x[d], lo, hi) - a[d]) * TT::S[d];
                }
                key[u] = base & 31;
                rk[u] = atomicAdd(&s_cnt[key[u]], 1);
            }
        }
        __syncthreads();
        if (threadIdx.x < 32) {             // exclusive scans over the 32 classes: surplus (beyond 64) and free slots
            const int n = s_cnt[threadIdx.x];
            const int sur = n > 64 ? n - 64 : 0, fre = n < 64 ? 64 - n : 0;
            int is = sur, ifr = fre;
#pragma unroll
            for (int o = 1; o < 32; o <<= 1) {
                const int ts = __shfl_up(is, o, 32), tf = __shfl_up(ifr, o, 32);
                if ((int)threadIdx.x >= o) { is += ts; ifr += tf; }
            }
            s_off[threadIdx.x] = is - sur;          // first surplus position of the class
            s_fre[threadIdx.x] = ifr - fre;         // first surplus entry its free slots take
            if (threadIdx.x == 31) s_fre[32] = is;  // surplus entries in all
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u)
            if (key[u] >= 0) {
                const unsigned short id = (unsigned short)((int)threadIdx.x + u * EVAL_WG);
                if (rk[u] < 64) s_list[key[u] * 64 + rk[u]] = id;
                else s_ovf[s_off[key[u]] + rk[u] - 64] = id;
            }
        __syncthreads();
        const int h = threadIdx.x & 31, w = threadIdx.x >> 5;
        const int n_h = s_cnt[h], nsur = s_fre[32];
        int jq[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int slot = w + 32 * u;
            int id = -1;
            if (slot < n_h) id = s_list[h * 64 + slot];           // (slot < 64 always)
            else {
                const int e = s_fre[h] + (slot - n_h);
                if (e < nsur) id = s_ovf[e];
            }
            jq[u] = id;
        }
        double x0[D], x1[D];
        int p0 = 0, p1 = 0;
        if (jq[0] >= 0) p0 = load_record<D>(xs + (long long)(qb + jq[0]) * (D + 1), x0);
        if (jq[1] >= 0) p1 = load_record<D>(xs + (long long)(qb + jq[1]) * (D + 1), x1);
        if (jq[0] >= 0) evaluate(x0, p0);
        if (jq[1] >= 0) evaluate(x1, p1);
        return;
    }
    // the coordinates (and the destination) of the NEXT round are in flight while the current one is
    // evaluated: a round's global loads would otherwise be exposed once per round
    int j = qb + threadIdx.x;
    double xn[D];
    int pn = 0;
    if (j < qe) pn = load_record<D>(xs + (long long)j * (D + 1), xn);
    while (j < qe) {
        double x[D];
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = xn[d];
        const int p = pn;
        const int jn = j + EVAL_WG;
        if (jn < qe) pn = load_record<D>(xs + (long long)jn * (D + 1), xn);
        evaluate(x, p);
        j = jn;
    }
}

// binned form (pass C of the region sort, see eval_binned_kernel): the window rows come from the LDS tile
template <int D, int ORDER>
__global__ void __launch_bounds__(256)
eval_derivs_binned_kernel(Grid g, Regions rg, const double *__restrict__ coef, const double *__restrict__ xs,
                          const int *__restrict__ off,
                          const int *__restrict__ wgoff, double *__restrict__ out, int ldout)
{
    constexpr int NOUT = 1 + D + (ORDER == 2 ? D * (D + 1) / 2 : 0);
    constexpr int TILE_ELEMS = tile_cells<D>();          // (dense strides here: the padded ones belong to eval_binned_kernel)
    __shared__ double tile[TILE_ELEMS];
    using TS = TileShape<D>;
    const int wg = blockIdx.x;
    if (wg >= wgoff[rg.nbins]) return;
    int lo = 0, hi = rg.nbins;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (wgoff[mid] <= wg) lo = mid; else hi = mid;
    }
    const int r = lo, part = wg - wgoff[r];
    int a[D];                                  // (origin and fill as in eval_binned_kernel, dense strides)
    {
        int rr = r;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            a[d] = (rr % rg.nreg[d]) * (TS::T[d] - 3);
            rr /= rg.nreg[d];
        }
    }
    for (int e = threadIdx.x; e < TILE_ELEMS; e += 256) {
        int rem = e, idx = 0;
        bool ok = true;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int l = rem % TS::T[d];
            rem /= TS::T[d];
            const int node = a[d] + l;
            ok = ok && node < g.nodes[d];
            idx += node * g.colstride[d];
        }
        tile[e] = ok ? coef[idx] : 0.0;
    }
    __syncthreads();
    const int qb = off[r] + part * EVAL_QPW;
    const int qe = min(off[r + 1], qb + EVAL_QPW);
    int tstr[D];
    {
        int m = 1;
#pragma unroll
        for (int d = 0; d < D; ++d) { tstr[d] = m; m *= TS::T[d]; }
    }
    for (int j = qb + threadIdx.x; j < qe; j += 256) {
        double b[ORDER + 1][D][4];
        int base = 0;
        double xr[D];
        const long long p = load_record<D>(xs + (long long)j * (D + 1), xr);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double x = xr[d];
            int ws = 0;
#pragma unroll
            for (int aa = 0; aa <= ORDER; ++aa) ws = window_table(g, d, x, aa, b[aa][d]);
            base += (ws - a[d]) * tstr[d];
        }
        double acc[NOUT];
        derivs_accumulate<D, ORDER>(b, [&](const int (&k)[D], double (&c)[4]) {
            int o = base;
#pragma unroll
            for (int d = 1; d < D; ++d) o += k[d] * tstr[d];
            lds_row4(tile, o, c);
        }, acc);
#pragma unroll
        for (int jj = 0; jj < NOUT; ++jj) out[p * ldout + jj] = acc[jj];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
// regions of the grid (tiles of TileShape<ndim>); false when the binned paths do not apply
bool make_regions(const Grid &g, Regions &rg)
{
    const int *T = g.ndim == 2 ? TileShape<2>::T : g.ndim == 3 ? TileShape<3>::T : g.ndim == 4 ? TileShape<4>::T : nullptr;
    if (!T) return false;
    long long nb = 1;
    for (int d = 0; d < MAXD; ++d) rg.nreg[d] = 1;
    for (int d = 0; d < g.ndim; ++d) {
        const int R = T[d] - 3;
        rg.nreg[d] = (g.nodes[d] - 3 + R - 1) / R;
        nb *= rg.nreg[d];
    }
    rg.nbins = (int)nb;
    return nb >= 1 && nb <= BIN_MAX;
}

// sorted records of a chunk ((D + 1) doubles each) | hist, off, cursor, wgoff | per-workgroup region counts / run bases
static thread_local DevScratch<3> g_sort;

void eval_sort_shutdown() { g_sort.release(); }

// order == 0: one nderiv pattern (nd) -> out[nq]; order 1 / 2: value + gradient (+ Hessian) -> out[nq][ldout]
template <int D, typename T>
static hipError_t eval_sort_d(const Grid &g, const Regions &rg, long long nq, const T *xq, int ldxq, const NDeriv &nd,
                              const T *coef, T *out, long long chunk, hipStream_t st, int order, int ldout)
{
    // default chunk: 2^24 queries (measured best at 64^3: large enough that the ~8 000 evaluation
    // workgroups of a chunk keep every CU full to the end; chunks small enough to stay in the Infinity
    // Cache were not faster -- the passes are bound by instructions, not by HBM)
    if (chunk <= 0) chunk = 1LL << 24;
    if (chunk > (1LL << 28)) chunk = 1LL << 28;
    if (chunk > nq) chunk = nq;
    int dev = 0;
    (void)hipGetDevice(&dev);
    // row length of the count matrix for THIS chunk and dimension count, and what it needs for THIS grid's regions:
    // the scratch is regrown when a later grid has more regions than the one it was sized for (round-2 advice:
    // a 40^3 spline followed by a 64^3 one wrote past the allocation)
    const int ldw = (int)(chunk / (256 * ScatterShape<D>::QPT) + 2);
    const long long cnt_need = (long long)ldw * rg.nbins + (long long)(ldw / BIN_ROWS + 2) * rg.nbins;     // count matrix + chunk sums
    const size_t need[3] = {sizeof(double) * (size_t)chunk * (D + 1), sizeof(int) * (4 * BIN_MAX + 8), sizeof(int) * (size_t)cnt_need};
    DevScratch<3> &s = g_sort;
    if (const hipError_t e = s.ensure(dev, need, /*may_release_plan=*/true); e != hipSuccess) return e;
    (void)s.wait_on(st);
    double *xs = s.as<double>(0);
    int *cnt = s.as<int>(2);
    int *hist = s.as<int>(1), *off = hist + BIN_MAX, *cursor = off + BIN_MAX + 1, *wgoff = cursor + BIN_MAX;
    const bool plain = value_only(nd);
    for (long long c0 = 0; c0 < nq; c0 += chunk) {
        const int n = (int)(nq - c0 < chunk ? nq - c0 : chunk);
        const T *xc = xq + c0 * ldxq;
        const unsigned nbs = (unsigned)((n + 256 * ScatterShape<D>::QPT - 1) / (256 * ScatterShape<D>::QPT));
        hipLaunchKernelGGL((bin_count_kernel<D, T>), dim3(nbs), dim3(256), 0, st, g, rg, n, xc, ldxq, cnt, ldw);
        int *part = cnt + (long long)ldw * rg.nbins;
        const unsigned nchunk = (nbs + BIN_ROWS - 1) / BIN_ROWS, nbg = (unsigned)((rg.nbins + 255) / 256);
        hipLaunchKernelGGL(bin_colsum_kernel, dim3(nbg, nchunk), dim3(256), 0, st, (int)nbs, rg.nbins, (const int *)cnt, part);
        hipLaunchKernelGGL(bin_total_kernel, dim3(nbg), dim3(256), 0, st, (int)nchunk, rg.nbins, part, hist);
        hipLaunchKernelGGL(bin_scan_kernel, dim3(1), dim3(256), 0, st, rg.nbins, (const int *)hist, off, cursor, wgoff);
        hipLaunchKernelGGL(bin_wgbase_kernel, dim3(nbg, nchunk), dim3(256), 0, st, (int)nbs, rg.nbins, (const int *)off, (const int *)part, cnt);
        hipLaunchKernelGGL((bin_scatter_kernel<D, T>), dim3(nbs), dim3(256), 2 * sizeof(int) * rg.nbins, st, g, rg, n, xc, ldxq,
                           (const int *)cnt, ldw, xs);
        const unsigned nw = (unsigned)(n / EVAL_QPW + rg.nbins + 1);
        if constexpr (sizeof(T) == 8) {
            if (order == 1 || order == 2)
                hipLaunchKernelGGL((order == 1 ? eval_derivs_binned_kernel<D, 1> : eval_derivs_binned_kernel<D, 2>), dim3(nw), dim3(256), 0, st,
                                   g, rg, coef, (const double *)xs, (const int *)off, (const int *)wgoff, out + c0 * ldout, ldout);
        }
        if (order == 0)
            hipLaunchKernelGGL((plain ? eval_binned_kernel<D, true, T> : eval_binned_kernel<D, false, T>), dim3(nw), dim3(EVAL_WG), 0, st,
                               g, rg, nd, coef, (const double *)xs, (const int *)off, (const int *)wgoff, out + c0);
    }
    (void)s.mark_used(st);
    return hipGetLastError();
}

template <typename T>
hipError_t eval_sort(const Grid &g, const Regions &rg, long long nq, const T *xq, int ldxq, const NDeriv &nd, const T *coef, T *out,
                     long long chunk, hipStream_t st, int order, int ldout)
{
    switch (g.ndim) {
    case 2: return eval_sort_d<2, T>(g, rg, nq, xq, ldxq, nd, coef, out, chunk, st, order, ldout);
    case 3: return eval_sort_d<3, T>(g, rg, nq, xq, ldxq, nd, coef, out, chunk, st, order, ldout);
    case 4: return eval_sort_d<4, T>(g, rg, nq, xq, ldxq, nd, coef, out, chunk, st, order, ldout);
    default: return hipErrorNotSupported;
    }
}
template hipError_t eval_sort<double>(const Grid &, const Regions &, long long, const double *, int, const NDeriv &, const double *, double *,
                                      long long, hipStream_t, int, int);
template hipError_t eval_sort<float>(const Grid &, const Regions &, long long, const float *, int, const NDeriv &, const float *, float *,
                                     long long, hipStream_t, int, int);

}  // namespace splpak
