// Run path (3-D / 4-D value and single-pattern evaluation; round 3).
// The region sort (evalsort.hip) moves every query three times (count, place, evaluate) and spends a tenth of its time on the
// prefixes in between.  Here the place pass stops at what it has in LDS anyway: every workgroup writes ITS 2 048 queries,
// sorted by region, as one contiguous image (64 KB of records, fully coalesced) and leaves the starts of its runs in a row
// of `starts`; the evaluation workgroup (region r, group k) walks the runs (w, r) of the ~nbins workgroups of its
// group.  No count pass, no prefix kernels, no global order: 24 + 32 bytes per query in the place pass, 32 + 8 in the
// evaluation pass.  Same arithmetic per query as everywhere else: identical bits.
#include "evalpaths.hpp"
#include "evalscratch.hpp"

namespace splpak {

constexpr int RUN_QPW = 2048;          // queries per place-pass workgroup

// RUN_NT threads per workgroup: 62 KB of LDS allow two workgroups per CU, i.e. 16 waves with 512 threads each (8 with 256:
// too few for a pass that waits on memory)
constexpr int RUN_NT = 512;
template <int D, typename T>
__global__ void __launch_bounds__(RUN_NT)
run_place_kernel(Grid g, Regions rg, int n, const T *__restrict__ xq, int ldxq, double *__restrict__ img,
                 int *__restrict__ starts)
{
    constexpr int NT = RUN_NT, NW = NT / 64, QPT = RUN_QPW / NT, QPW = RUN_QPW;
    __shared__ double sx[QPW * D];
    __shared__ int sidx[QPW];
    extern __shared__ int lds_bins[];          // lstart[nbins + 1] | lcount[nbins]
    int *lst = lds_bins, *lcn = lds_bins + rg.nbins + 1;
    __shared__ int sscan[NW];
    for (int b = threadIdx.x; b < rg.nbins; b += NT) lcn[b] = 0;
    __syncthreads();
    const int base = blockIdx.x * QPW;
    int rid[QPT], rank[QPT];
    double xr[QPT][D];
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        const int i = base + j * NT + threadIdx.x;
        rid[j] = -1;
        rank[j] = 0;
        if (i < n) {
#pragma unroll
            for (int d = 0; d < D; ++d) xr[j][d] = (double)xq[(long long)i * ldxq + d];
            rid[j] = region_of<D>(g, rg, xr[j]);
            rank[j] = atomicAdd(&lcn[rid[j]], 1);
        }
    }
    __syncthreads();
    const int per = (rg.nbins + NT - 1) / NT;
    const int b0 = threadIdx.x * per;
    int q = 0;
    for (int b = b0; b < b0 + per && b < rg.nbins; ++b) q += lcn[b];
    // exclusive scan over the threads: within the waves by shuffles, then the wave totals (two barriers instead of the sixteen
    // of a Hillis-Steele scan in LDS: a third of this workgroup's time)
    int incl = q;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if ((int)(threadIdx.x & 63) >= o) incl += t;
    }
    if ((threadIdx.x & 63) == 63) sscan[threadIdx.x >> 6] = incl;
    __syncthreads();
    int woff = 0;
    for (int v = 0; v < (int)(threadIdx.x >> 6); ++v) woff += sscan[v];
    int total = 0;
#pragma unroll
    for (int v = 0; v < NW; ++v) total += sscan[v];
    q = woff + incl - q;
    for (int b = b0; b < b0 + per && b < rg.nbins; ++b) {
        lst[b] = q;
        q += lcn[b];
    }
    if (threadIdx.x == 0) lst[rg.nbins] = total;
    __syncthreads();
    for (int b = threadIdx.x; b <= rg.nbins; b += NT) starts[(long long)blockIdx.x * (rg.nbins + 1) + b] = lst[b];
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        if (rid[j] < 0) continue;
        const int lp = lst[rid[j]] + rank[j];
#pragma unroll
        for (int d = 0; d < D; ++d) sx[d * QPW + lp] = xr[j][d];
        sidx[lp] = base + j * NT + threadIdx.x;
    }
    __syncthreads();
    for (int lp = threadIdx.x; lp < total; lp += NT) {         // the sorted image: consecutive lanes, consecutive records
        double x[D];
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = sx[d * QPW + lp];
        store_record<D>(img + ((long long)blockIdx.x * QPW + lp) * (D + 1), x, sidx[lp]);
    }
}

// grp = place-pass workgroups per evaluation workgroup (<= RUN_GROUP_MAX): chosen by the host so that a region's queries in a
// group are ~2 000 (3-D 64^3: 128 x 16.4; 4-D 32^4: 615 x 3.2).
constexpr int RUN_GROUP_MAX = 1024;
template <int D, bool VAL, typename T>
__global__ void __launch_bounds__(EVAL_WG, 8)
eval_runs_kernel(Grid g, Regions rg, NDeriv nd, const T *__restrict__ coef, const double *__restrict__ img,
                 const int *__restrict__ starts, int nwg, int grp, T *__restrict__ out)
{
    constexpr bool DEAL = D == 4;             // queries dealt to the lanes by LDS bank class (see eval_binned_kernel)
    static_assert(EVAL_WG == 1024 && RUN_GROUP_MAX <= EVAL_WG, "one place-pass workgroup per thread in the prefix");
    __shared__ double tile[tile_elems<D>()];
    __shared__ int pre[RUN_GROUP_MAX + 1];
    __shared__ unsigned short rst[RUN_GROUP_MAX];
    __shared__ int wsum[16];
    __shared__ int s_cnt[32], s_sur[33], s_fre[33];
    __shared__ unsigned short s_list[DEAL ? EVAL_QPW : 1];      // [class][64 slots] (two of these workgroups share a CU's LDS: 79 KB each)
    using TS = TileShape<D>;
    using TT = TileStride<D>;
    const int r = blockIdx.x % rg.nbins, k = blockIdx.x / rg.nbins;
    const int w0 = k * grp;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // this region's runs in the group's workgroups: start inside the workgroup's image, inclusive prefix of the lengths
    {
        int c = 0, st = 0;
        if (tid < grp && w0 + tid < nwg) {
            const int *__restrict__ row = starts + (long long)(w0 + tid) * (rg.nbins + 1) + r;
            st = row[0];
            c = row[1] - st;
        }
        if (tid < grp) rst[tid] = (unsigned short)st;
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int woff = 0;
        for (int v = 0; v < wave; ++v) woff += wsum[v];
        if (tid < grp) pre[tid + 1] = woff + incl;
        if (tid == 0) pre[0] = 0;
    }
    __syncthreads();
    const int total = pre[grp];
    if (total == 0) return;
    int a[D];                                  // first node of the region's tile; origin, fill and `evaluate` as in eval_binned_kernel (evalsort.hip)
    {
        int rr = r;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            a[d] = (rr % rg.nreg[d]) * (TS::T[d] - 3);
            rr /= rg.nreg[d];
        }
    }
    for (int e = tid; e < tile_cells<D>(); e += EVAL_WG) {
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
    constexpr int t1 = TT::S[1], t2 = TT::S[2], t3 = TT::S[3];
    auto locate = [&](int qi) -> const double * {      // record qi of the group's queries of this region
        int lo = 0, hi = grp;                          // pre[lo] <= qi < pre[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (pre[mid] <= qi) lo = mid; else hi = mid;
        }
        return img + ((long long)(w0 + lo) * RUN_QPW + rst[lo] + (qi - pre[lo])) * (D + 1);
    };
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
        // batches of <= 2 048 queries, dealt to the lanes by the bank class of their tile offset (eval_binned_kernel has the
        // reasoning): 64 slots per class = two rounds per lane; what a class holds beyond 64 fills the free slots of the
        // short classes
        for (int q0 = 0; q0 < total; q0 += EVAL_QPW) {
            const int nqb = total - q0 < EVAL_QPW ? total - q0 : EVAL_QPW;
            if (tid < 32) s_cnt[tid] = 0;
            __syncthreads();
            int key[2] = {-1, -1}, rk[2] = {0, 0};
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int jj = tid + u * EVAL_WG;
                if (jj < nqb) {
                    double x[D];
                    (void)load_record<D>(locate(q0 + jj), x);
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
            if (tid < 32) {             // exclusive scans over the 32 classes: surplus (beyond 64) and free slots
                const int n = s_cnt[tid];
                const int sur = n > 64 ? n - 64 : 0, fre = n < 64 ? 64 - n : 0;
                int is = sur, ifr = fre;
#pragma unroll
                for (int o = 1; o < 32; o <<= 1) {
                    const int ts = __shfl_up(is, o, 32), tf = __shfl_up(ifr, o, 32);
                    if (tid >= o) { is += ts; ifr += tf; }
                }
                s_sur[tid] = is - sur;
                s_fre[tid] = ifr - fre;
                if (tid == 31) { s_sur[32] = is; s_fre[32] = ifr; }
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (key[u] >= 0) {
                    const unsigned short id = (unsigned short)(tid + u * EVAL_WG);
                    if (rk[u] < 64) s_list[key[u] * 64 + rk[u]] = id;
                    else {                               // surplus entry e takes the e-th free slot (classes in order)
                        const int e = s_sur[key[u]] + rk[u] - 64;
                        int lo = 0, hi = 32;             // s_fre[lo] <= e < s_fre[hi]
                        while (hi - lo > 1) {
                            const int mid = (lo + hi) >> 1;
                            if (s_fre[mid] <= e) lo = mid; else hi = mid;
                        }
                        s_list[lo * 64 + s_cnt[lo] + (e - s_fre[lo])] = id;
                    }
                }
            __syncthreads();
            const int h = tid & 31, w = tid >> 5;
            const int n_h = s_cnt[h], nsur = s_sur[32];
            int filled = n_h < 64 ? n_h : 64;           // own entries + the surplus entries that took this class's free slots
            if (n_h < 64) {
                int ex = nsur - s_fre[h];
                ex = ex < 0 ? 0 : (ex > 64 - n_h ? 64 - n_h : ex);
                filled += ex;
            }
            int jq[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int slot = w + 32 * u;
                jq[u] = slot < filled ? (int)s_list[h * 64 + slot] : -1;
            }
            double x0[D], x1[D];
            int p0 = 0, p1 = 0;
            if (jq[0] >= 0) p0 = load_record<D>(locate(q0 + jq[0]), x0);
            if (jq[1] >= 0) p1 = load_record<D>(locate(q0 + jq[1]), x1);
            if (jq[0] >= 0) evaluate(x0, p0);
            if (jq[1] >= 0) evaluate(x1, p1);
            __syncthreads();
        }
    } else {
        int qi = tid;
        double xn[D];
        int pn = 0;
        if (qi < total) pn = load_record<D>(locate(qi), xn);
        while (qi < total) {
            double x[D];
#pragma unroll
            for (int d = 0; d < D; ++d) x[d] = xn[d];
            const int p = pn;
            const int qn = qi + EVAL_WG;
            if (qn < total) pn = load_record<D>(locate(qn), xn);
            evaluate(x, p);
            qi = qn;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
// per-workgroup sorted images of a chunk | starts of their runs
static thread_local DevScratch<2> g_runs;

void eval_runs_shutdown() { g_runs.release(); }

template <int D, typename T>
static hipError_t eval_runs_d(const Grid &g, const Regions &rg, long long nq, const T *xq, int ldxq, const NDeriv &nd,
                              const T *coef, T *out, long long chunk, hipStream_t st)
{
    // (runs of RUN_QPW / nbins records: 16 at 64^3, 3 at 4-D 32^4; with more regions than that the evaluation pass would
    // gather single records and its groups outgrow the prefix)
    // Measured at 4-D 32^4 (648 regions, runs of 3 records = one 128-byte line): place 0.30 ms instead of count + prefixes +
    // place 0.70, but the evaluation pass 1.30 instead of 0.82 ms (fragments, a 10-step search per record, twice with the class
    // dealing) -- 1.09 against 1.18e10 evals/s: the sort stays for grids of more than 256 regions.
    if (rg.nbins > RUN_GROUP_MAX || rg.nbins > 256) return hipErrorNotSupported;
    // place-pass workgroups per evaluation workgroup: ~1 950 queries of a region (two rounds of 1 024 threads; the 4-D
    // class dealing works in batches of 2 048)
    int grp = (int)(0.95 * rg.nbins + 0.5);
    if (D == 3 && grp < 128) grp = 128;
    if (grp < 32) grp = 32;
    if (grp > RUN_GROUP_MAX) grp = RUN_GROUP_MAX;
    if (chunk <= 0) chunk = 1LL << 24;
    if (chunk > (1LL << 26)) chunk = 1LL << 26;
    if (chunk > nq) chunk = nq;
    const long long nwg_max = (chunk + RUN_QPW - 1) / RUN_QPW;
    const size_t need[2] = {sizeof(double) * (size_t)(nwg_max * RUN_QPW * (D + 1)), sizeof(int) * (size_t)(nwg_max * (rg.nbins + 1))};
    DevScratch<2> &s = g_runs;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (s.ensure(dev, need, /*may_release_plan=*/true) != hipSuccess) { (void)hipGetLastError(); return hipErrorOutOfMemory; }
    (void)s.wait_on(st);
    double *img = s.as<double>(0);
    int *starts = s.as<int>(1);
    const bool plain = value_only(nd);
    for (long long c0 = 0; c0 < nq; c0 += chunk) {
        const int n = (int)(nq - c0 < chunk ? nq - c0 : chunk);
        const T *xc = xq + c0 * ldxq;
        const unsigned nwg = (unsigned)((n + RUN_QPW - 1) / RUN_QPW);
        hipLaunchKernelGGL((run_place_kernel<D, T>), dim3(nwg), dim3(RUN_NT), sizeof(int) * (2 * rg.nbins + 1), st, g, rg, n, xc, ldxq,
                           img, starts);
        const unsigned ngroups = (nwg + (unsigned)grp - 1) / (unsigned)grp;
        hipLaunchKernelGGL((plain ? eval_runs_kernel<D, true, T> : eval_runs_kernel<D, false, T>), dim3(ngroups * (unsigned)rg.nbins),
                           dim3(EVAL_WG), 0, st, g, rg, nd, coef, (const double *)img, (const int *)starts, (int)nwg, grp, out + c0);
    }
    (void)s.mark_used(st);
    return hipGetLastError();
}

template <typename T>
hipError_t eval_runs(const Grid &g, const Regions &rg, long long nq, const T *xq, int ldxq, const NDeriv &nd, const T *coef, T *out,
                     long long chunk, hipStream_t st)
{
    if (g.ndim == 3) return eval_runs_d<3, T>(g, rg, nq, xq, ldxq, nd, coef, out, chunk, st);
    if (g.ndim == 4) return eval_runs_d<4, T>(g, rg, nq, xq, ldxq, nd, coef, out, chunk, st);
    return hipErrorNotSupported;
}
template hipError_t eval_runs<double>(const Grid &, const Regions &, long long, const double *, int, const NDeriv &, const double *, double *,
                                      long long, hipStream_t);
template hipError_t eval_runs<float>(const Grid &, const Regions &, long long, const float *, int, const NDeriv &, const float *, float *,
                                     long long, hipStream_t);

}  // namespace splpak
