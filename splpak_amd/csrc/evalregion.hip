// Persistent region path (round 4; 4-D: round 5, see pr_eval4_kernel).
// The run path (evalruns.hip) moves every query twice through HBM as a 32-byte record and writes its 8-byte result into a sector that
// other regions' workgroups fill at other times: 149 B per query by the counters for 32 algorithmic ones.  Here:
//
//   pr_place_kernel   a workgroup reads 8 192 queries, bins them by (region, interior or not) in LDS and writes their
//                     coordinates as D planes in that order (staged through LDS: consecutive stores), their LOCAL indices
//                     (16 bit) and the starts of the runs.  24 B read, 26 B written per 3-D query.
//   pr_eval_kernel    PERSISTENT: one workgroup of 16 waves per CU.  A workgroup holds the coefficient tile of ONE region in
//                     LDS; its waves, each an independent worker, take chunks of that region's runs (two levels: the
//                     workgroup takes superchunks from the region's counter in global memory, its waves take chunks from
//                     a counter in LDS) and walk them as one stream (four runs in flight, so the lanes the tail of one run
//                     leaves idle start the next ones: no barrier, no prefix, no search), the boundary runs first, then
//                     the interior ones, whose lanes all take the 16-operation closed form of the basis table.  When a
//                     region is used up the workgroup moves to the one with the most work left per workgroup there.
//                     The coordinates of element i + 1 are requested before the window of element i is read.  Results go
//                     to the SAME sorted places: consecutive lanes, consecutive words.  24 B read, 8 B written.
//   pr_unsort_kernel  per place-pass workgroup: sorted results + local indices -> the caller's order, through LDS.  10 B read,
//                     8 B written.
//
// By construction 100 B of HBM traffic per 3-D query, every byte of it in consecutive runs of at least 200 B.  (The first
// form of this path sorted only the 16-bit indices and let the evaluation pass gather the coordinates and scatter the results
// through the L2 of "its" XCD: 60 B by construction, but the windows of 8 192 workers do not stay in a 4 MB L2 -- 108 B
// fetched and 124 B written per query by the counters, every 8-byte result a read-for-ownership and an eviction of a line.)
// Arithmetic per query: eval_table + window_sum as everywhere else -- identical bits.  Used for 3-D grids of at most 64 regions
// of 16 (or 8) window starts per dimension: 64^3 nodes give 4 x 4 x 4 regions with tiles of 19^3 coefficients (55 KB).
#include "evalpaths.hpp"
#include "evalscratch.hpp"

namespace splpak {

struct PRegions { int nreg[MAXD]; int sper[MAXD]; int text[MAXD]; int tstr[MAXD]; int nbins; int telems; int tcells; int deal; };

constexpr int PR_Q = 8192;         // queries per place-pass workgroup (16-bit local indices; half a coordinate plane of them = 32 KB of LDS)
constexpr int PR_NT = 1024;        // threads of a place-pass workgroup
constexpr int PR_EW = 1024;        // threads of an evaluation workgroup: 16 waves = 4 per SIMD, ONE workgroup per CU (two of 640 threads
                                   // never shared a CU: 10 waves go to the SIMDs as 3,3,2,2 and two such sets can need 6 x 88 registers
                                   // on one SIMD -- the second workgroup of every CU only started when the first had ended)
constexpr int PR_WPE = 4;          // waves per SIMD the evaluation kernel is compiled for (128 registers; it takes 88)
// place-pass shape by dimension count.  MAXBINS: most regions of a grid; NCLS: LDS slot classes the queries of a bin are dealt
// by (3-D: the 16 sixteen-byte slots of ds_read_b128; 4-D: 32 eight-byte slots, ds_read_b64); JMAX: rounds of the deal.
// 2 MAXBINS JMAX = 2 PR_NT: every thread of the place pass prefixes two (bin, round) counters.
template <int D> struct PRCfg { static constexpr int MAXBINS = 64, NCLS = 16, JMAX = 16; };
template <> struct PRCfg<4> { static constexpr int MAXBINS = 256, NCLS = 32, JMAX = 4; };
constexpr int PR_MAXBINS = 256;    // (scratch sizes: the largest of them)

template <int D, typename T>
__global__ void __launch_bounds__(PR_NT)
pr_place_kernel(Grid g, PRegions rg, long long nq, const T *__restrict__ xq, int ldxq, unsigned short *__restrict__ sidx,
                int *__restrict__ starts, T *__restrict__ xs, unsigned char *__restrict__ scls)
{
    // bins: 2 per region -- [2 r] the queries whose windows are interior ones in every dimension (closed-form basis table,
    // eval_table), [2 r + 1] the others (end functions / clipped windows in some dimension): the evaluation pass walks the
    // interior runs first and the others afterwards, so that its waves are homogeneous (a wave with one non-interior lane
    // pays the general table for that dimension)
    // Inside a bin the queries are DEALT by the LDS slot class of their window (the 16-byte slot, mod 16, of the address the
    // evaluation pass reads the window from: ds_read_b128 serves 16 lanes per cycle from 16 slots): first the first query of
    // every class, then the second of every class, ... -- neighbouring lanes of the evaluation pass then read from
    // different slots where a random order has ~3 of 16 lanes on the busiest one (SQ_LDS_BANK_CONFLICT was 70 % of that
    // pass's LDS cycles, and the LDS its bottleneck).  A query's rank within its (bin, class) is its ROUND; it marks its
    // class in the round's mask, the rounds' populations (popcounts) are prefixed over bins x rounds, and its place is the
    // start of its round + the number of classes below its own in that round (class order inside a round: 16 consecutive
    // queries then straddle two rounds with fewer repeats than in the order the counters would give, 8.4 against 9.8 LDS
    // cycles per read in a simulation of 64^3).  Ranks beyond JMAX - 1 (clustered queries) share the last round, in counter order.
    constexpr int QPT = PR_Q / PR_NT, NB2 = 2 * PRCfg<D>::MAXBINS, HALF = PR_Q / 2, NCLS = PRCfg<D>::NCLS, JMAX = PRCfg<D>::JMAX, NKEY = NB2 * JMAX;
    static_assert(NKEY == 2 * PR_NT, "the prefix below gives every thread two (bin, round) counters");
    constexpr int TAB_BYTES = NB2 * NCLS * 4 + 2 * NKEY * 4;
    constexpr int SB_BYTES = HALF * (int)sizeof(T) > TAB_BYTES ? HALF * (int)sizeof(T) : TAB_BYTES;
    __shared__ unsigned short ssort[PR_Q];
    // 4-D: the LDS slot class of every query's window (tile offset mod 32) travels with the image as a plane of bytes -- the
    // evaluation pass deals its chunks to the lanes by it (pr_eval4_kernel); runs of ~16 queries are too short to be dealt here
    __shared__ __attribute__((aligned(16))) unsigned char scl[D == 4 ? PR_Q : 4];
    __shared__ __attribute__((aligned(16))) unsigned char sbuf[SB_BYTES];      // the counters, then the staging half plane
    T *splane = reinterpret_cast<T *>(sbuf);
    int *ccnt = reinterpret_cast<int *>(sbuf);                                   // [bin][class]: queries so far
    unsigned *dmask = reinterpret_cast<unsigned *>(sbuf + NB2 * NCLS * 4);       // [bin][round]: the classes present (last round: a counter)
    int *rstart = reinterpret_cast<int *>(sbuf + NB2 * NCLS * 4 + NKEY * 4);     // [bin][round]: where the round starts in the image
    __shared__ int lst[NB2 + 1];
    __shared__ int wsum[PR_NT / 64];
    __shared__ unsigned char rtab[D][256];         // region index of a window start, per dimension (window starts < 256: host check)
    const int tid = threadIdx.x;
    const int nb2 = 2 * rg.nbins;
    for (int e = tid; e < D * 256; e += PR_NT) {
        const int d = e >> 8, ws = e & 255;
        const int rd = ws / rg.sper[d];
        rtab[d][ws] = (unsigned char)(rd < rg.nreg[d] - 1 ? rd : rg.nreg[d] - 1);
    }
    for (int e = tid; e < TAB_BYTES / 4; e += PR_NT) reinterpret_cast<int *>(sbuf)[e] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * PR_Q;
    int rid[QPT], rank[QPT];                       // rid: bin * JMAX + round; rank: within the last round, or -1 - class
    unsigned long long clsw = 0;                   // (4-D) the classes of this thread's queries, 8 bits each
    T xr[QPT][D];
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        const long long i = base + j * PR_NT + tid;
        rid[j] = -1;
        rank[j] = 0;
        if (i < nq) {
            int r = 0, m = 1, tb = 0;
            bool inter = true;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                int lo, hi;
                bool in_d;
                xr[j][d] = __builtin_nontemporal_load(xq + i * ldxq + d);
                const int ws = window_start_value(g, d, (double)xr[j][d], lo, hi, in_d);
                inter = inter && in_d;
                const int rd = (int)rtab[d][ws];
                r += rd * m;
                m *= rg.nreg[d];
                tb += (ws - rd * rg.sper[d]) * rg.tstr[d];          // the window's first entry in the region's tile
            }
            // (3-D tiles: an odd start reads the second copy of the tile, rg.telems entries further and one entry down)
            const int ta = (rg.telems > 0 && (tb & 1)) ? rg.telems + tb - 1 : tb;
            const int cls = rg.telems > 0 ? (ta >> 1) & (NCLS - 1) : tb & (NCLS - 1);
            if constexpr (D == 4) clsw |= (unsigned long long)cls << (8 * j);
            const int bin = 2 * r + (inter ? 0 : 1);
            int round = atomicAdd(&ccnt[bin * NCLS + cls], 1);
            if (!rg.deal) round = JMAX - 1;
            if (round < JMAX - 1) {
                atomicOr(&dmask[bin * JMAX + round], 1u << cls);
                rid[j] = bin * JMAX + round;
                rank[j] = -1 - cls;                                  // (place: by the mask)
            } else {
                rid[j] = bin * JMAX + JMAX - 1;
                rank[j] = (int)atomicAdd(&dmask[rid[j]], 1u);        // (place: by this counter)
            }
        }
    }
    __syncthreads();
    {
        // exclusive prefix over the NKEY = 2 PR_NT (bin, round) counters, in place
        // (two neighbouring rounds of one bin: the odd one may be the bin's last round, which holds a count, not a mask)
        const unsigned m0 = dmask[2 * tid], m1 = dmask[2 * tid + 1];
        const int c0 = __builtin_popcount(m0), c1 = ((2 * tid + 1) % JMAX == JMAX - 1) ? (int)m1 : __builtin_popcount(m1);
        int incl = c0 + c1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if ((tid & 63) >= o) incl += t;
        }
        if ((tid & 63) == 63) wsum[tid >> 6] = incl;
        __syncthreads();
        int before = 0;
        for (int w = 0; w < (tid >> 6); ++w) before += wsum[w];
        const int excl = before + incl - (c0 + c1);
        rstart[2 * tid] = excl;
        rstart[2 * tid + 1] = excl + c0;
        if (tid == PR_NT - 1) lst[NB2] = excl + c0 + c1;
    }
    __syncthreads();
    for (int e = tid; e < NB2; e += PR_NT) lst[e] = rstart[e * JMAX];
    int lp[QPT];
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        lp[j] = -1;
        if (rid[j] >= 0) {
            lp[j] = rstart[rid[j]] + (rank[j] >= 0 ? rank[j] : __builtin_popcount(dmask[rid[j]] & ((1u << (-1 - rank[j])) - 1u)));
            ssort[lp[j]] = (unsigned short)(j * PR_NT + tid);
            if constexpr (D == 4) scl[lp[j]] = (unsigned char)(clsw >> (8 * j));
        }
    }
    __syncthreads();                               // (the counters give way to the staging buffer; lst is complete)
    const int total = lst[NB2];
    // the coordinates go to their sorted places in the workgroup's image (D planes of PR_Q entries: the evaluation pass reads
    // them with consecutive lanes on consecutive entries), half a plane at a time through LDS so that the stores are
    // consecutive (straight scattered 8-byte stores into the image: 1.03 ms per 5e7 queries instead of 0.25 without them)
    if constexpr (D == 4) {
        // 4-D: the image holds RECORDS of the four coordinates (32 bytes) instead of planes -- the evaluation pass takes its
        // elements in an order dealt by LDS bank class, i.e. scattered over a chunk, and a scattered element then costs one
        // sector instead of four lines (measured with planes: 2.8 of the pass's 5 ms per 1e8 queries went into these loads).
        // Staged through LDS a quarter of the image at a time.
        constexpr int PIECE = PR_Q / 4;
        static_assert(PIECE * 4 * (int)sizeof(T) <= SB_BYTES, "a quarter of the records fits the staging buffer");
        T *__restrict__ dstr = xs + (long long)blockIdx.x * PR_Q * D;
#pragma unroll
        for (int pc = 0; pc < 4; ++pc) {
            if (pc > 0) __syncthreads();
#pragma unroll
            for (int j = 0; j < QPT; ++j) {
                const int l = lp[j] - pc * PIECE;
                if (lp[j] >= 0 && l >= 0 && l < PIECE) {
#pragma unroll
                    for (int d = 0; d < D; ++d) splane[l * D + d] = xr[j][d];
                }
            }
            __syncthreads();
            const int nrec = total - pc * PIECE < PIECE ? total - pc * PIECE : PIECE;
            for (int e = tid; e < nrec * D; e += PR_NT) __builtin_nontemporal_store(splane[e], dstr + (long long)pc * PIECE * D + e);
        }
    } else {
#pragma unroll
    for (int d = 0; d < D; ++d) {
        T *__restrict__ dstp = xs + ((long long)blockIdx.x * D + d) * PR_Q;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            if (d + hf > 0) __syncthreads();
#pragma unroll
            for (int j = 0; j < QPT; ++j) {
                const int l = lp[j] - hf * HALF;
                if (lp[j] >= 0 && l >= 0 && l < HALF) splane[l] = xr[j][d];
            }
            __syncthreads();
            for (int e = tid; e < HALF && hf * HALF + e < total; e += PR_NT) __builtin_nontemporal_store(splane[e], dstp + hf * HALF + e);
        }
    }
    }
    for (int e = tid; e <= nb2; e += PR_NT) starts[(long long)blockIdx.x * (nb2 + 1) + e] = lst[e];
    unsigned *__restrict__ dst = reinterpret_cast<unsigned *>(sidx + base);
    for (int e = tid; 2 * e < total; e += PR_NT) {
        const unsigned lo = ssort[2 * e], hi = 2 * e + 1 < total ? ssort[2 * e + 1] : 0u;
        dst[e] = lo | (hi << 16);
    }
    if constexpr (D == 4) {
        static_assert(QPT <= 8, "eight class bytes per thread");
        unsigned *__restrict__ dc = reinterpret_cast<unsigned *>(scls + base);
        const unsigned *sc4 = reinterpret_cast<const unsigned *>(scl);
        for (int e = tid; 4 * e < total; e += PR_NT) dc[e] = sc4[e];          // (the bytes beyond `total` in the last word are never read)
    }
}

template <int D, int SPER> struct PTile {            // tile of a region: SPER window starts + 3 per dimension, compile-time LDS strides
    static constexpr int TE = SPER + 3;
    // 3-D: the rows of a window are read as two 16-byte halves (ds_read_b128: 16 lanes per LDS cycle, 16-byte slots -- a
    // random set of 16 slots out of 16 collides less than 32 out of 32, and half as many instructions), which must be
    // 16-byte aligned: even strides, and a SECOND copy of the tile one entry further for the windows with an odd start
    static constexpr bool W128 = D == 3;
    static constexpr int S1 = W128 ? ((TE + 1) & ~1) : (TE | 1);      // (else) odd row stride: the window rows of a lane spread over the LDS banks
    static constexpr int S2 = W128 ? S1 * TE : S1 * TE + 1;
    static constexpr int S3 = S2 * TE + 1;
    static constexpr int stride(int d) { return d == 0 ? 1 : (d == 1 ? S1 : (d == 2 ? S2 : S3)); }
    static constexpr int COPY = ((D == 1 ? TE : (D == 2 ? S1 * TE : (D == 3 ? S2 * TE : S3 * TE))) + 8 + 1) & ~1;
    static constexpr int ELEMS = W128 ? 2 * COPY : COPY;
};

template <int D, int SPER, bool VAL, typename T>
__global__ void __launch_bounds__(PR_EW, PR_WPE)
pr_eval_kernel(Grid g, PRegions rg, NDeriv nd, const T *__restrict__ coef, const T *__restrict__ xs,
               const int *__restrict__ starts, int nwg_all, int c0, int *__restrict__ queue, T *__restrict__ outs)
{
    using PT = PTile<D, SPER>;
    __shared__ __attribute__((aligned(16))) double pr_tile[PT::ELEMS];
    __shared__ int s_region, s_next, s_done, s_base[8], s_ready[8];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int t1 = D > 1 ? PT::S1 : 0, t2 = D > 2 ? PT::S2 : 0, t3 = D > 3 ? PT::S3 : 0;
    // Work distribution.  A workgroup holds the tile of ONE region; its waves, each on its own, take chunks of that region's
    // runs (c0 place-pass workgroups of interior runs, 4 c0 of the others; take_chunk below) until the region is used up, then
    // the workgroup moves to the region with the most work left per workgroup already there.
    // Why per wave: the SIMD issues from its oldest wave first, so the waves of a workgroup given equal shares finish one
    // after the other -- with a workgroup-wide barrier per work item the first wave waited 28-42 % of its life at barriers
    // (in-kernel clocks) while the last ones ran alone on their SIMDs with nothing to hide their latencies behind.
    //   queue[r]          SUPERCHUNKS (SC chunks) of region r taken (may overshoot by one per workgroup)
    //   queue[nbins + r]  workgroups at region r
    const int nbins = rg.nbins;
    const int c1 = 4 * c0;
    const int nch0 = (nwg_all + c0 - 1) / c0, nch1 = (nwg_all + c1 - 1) / c1;
    // lane L of a wave: cost of region L (window starts it covers, those with a boundary window in some dimension 2.5-fold)
    // and whether it has boundary windows at all (regions without them have no chunks of the second kind)
    double cost_l = 0.0;
    bool edge_l = false;
    if (lane < nbins) {
        double vol = 1.0, inter = 1.0;
        int rr = lane;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int rd = rr % rg.nreg[d], S = g.nodes[d] - 3;
            rr /= rg.nreg[d];
            const int lo = rd * rg.sper[d], hi = min(S, lo + rg.sper[d]);
            const int ilo = max(lo, 2), ihi = min(hi, g.nodes[d] - 5);
            vol *= hi - lo;
            inter *= max(0, ihi - ilo);
        }
        cost_l = vol + 1.5 * (vol - inter);
        edge_l = inter < vol;
    }
    const unsigned long long edge_mask = __builtin_amdgcn_ballot_w64(edge_l);
    if (wave == 0) {
        // the first region of this workgroup: workgroups are dealt to the regions in proportion to the costs
        double cum = cost_l;
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) {
            const double up = __shfl_up(cum, sft);
            if (lane >= sft) cum += up;
        }
        const double total = __shfl(cum, 63);
        const double target = ((double)blockIdx.x + 0.5) * total / (double)gridDim.x;
        int r0 = __builtin_popcountll(__builtin_amdgcn_ballot_w64(cum <= target));
        if (r0 > nbins - 1) r0 = nbins - 1;
        if (lane == 0) {
            atomicAdd(queue + nbins + r0, 1);
            s_region = r0;
        }
    }
    __syncthreads();
    int a[D];                                        // first node of the current region's tile (origin and fill: cf. eval_binned_kernel, evalsort.hip)
    for (;;) {
    const int r = __builtin_amdgcn_readfirstlane(s_region);
    if (r < 0) break;
    {
        int rr = r;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            a[d] = (rr % rg.nreg[d]) * rg.sper[d];
            rr /= rg.nreg[d];
        }
        for (int e = tid; e < rg.tcells; e += PR_EW) {
            int rem = e, idx = 0, te = 0;
            bool ok = true;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int l = rem % rg.text[d];
                rem /= rg.text[d];
                const int node = a[d] + l;
                ok = ok && node < g.nodes[d];
                idx += node * g.colstride[d];
                te += l * PT::stride(d);
            }
            const double cv = ok ? (double)coef[idx] : 0.0;
            pr_tile[te] = cv;
            if (PT::W128 && te > 0) pr_tile[PT::COPY + te - 1] = cv;      // the copy for odd window starts: entry i holds tile entry i + 1
        }
    }
    constexpr int SC = 16;                           // chunks of a superchunk
    const int nedge = ((edge_mask >> r) & 1ull) ? nch1 : 0;      // chunks of boundary runs come first
    const int ntot = nedge + nch0, nsc = (ntot + SC - 1) / SC;
    if (tid == 0) {
        const int b0 = atomicAdd(queue + r, 1);
        s_next = 0;
        s_done = b0 >= nsc ? 1 : 0;
        s_base[0] = b0 < nsc ? b0 : -1;
        s_ready[0] = 1;
        for (int k = 1; k < 8; ++k) s_ready[k] = 0;
    }
    __syncthreads();
    constexpr int NR = 4;
    const int nb1 = 2 * nbins + 1;
    // A wave's stream of runs goes on across its chunks (the first form drained the lanes and paid two memory round trips
    // at the start of every chunk: a sixth of a wave's life by the in-kernel clocks).
    // Chunks are handed out in two levels: the region's counter in global memory counts SUPERCHUNKS of SC chunks (an atomic
    // add on one address from all XCDs took ~0.4 us of that address's time: with one per chunk and wave the 64 counters were
    // the bottleneck at 2 place-pass workgroups per chunk and cost 10 us per chunk at 8); inside the workgroup the waves
    // take chunk numbers from a counter in LDS.  Superchunk k of the workgroup is published (s_base, s_ready = k + 1) by the
    // wave that took its chunk SC/2 of superchunk k - 1: half a superchunk ahead of its first use.
    auto take_chunk = [&]() -> int {
        int v = 0;
        if (lane == 0) v = atomicAdd(&s_next, 1);
        v = __builtin_amdgcn_readfirstlane(v);
        const int k = v / SC, o = v % SC;
        for (;;) {
            if (__hip_atomic_load(&s_ready[k & 7], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == k + 1) break;
            if (__hip_atomic_load(&s_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return -1;       // (set after every valid superchunk was published)
            __builtin_amdgcn_s_sleep(4);
        }
        const int b = __hip_atomic_load(&s_base[k & 7], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (o == SC / 2) {
            // this wave publishes superchunk k + 1, whatever happens to its own chunk: the waves that hold numbers of it wait for that
            int nb = -1;
            if (b >= 0) {
                int t = 0;
                if (lane == 0) t = atomicAdd(queue + r, 1);
                t = __builtin_amdgcn_readfirstlane(t);
                if (t < nsc) nb = t;
            }
            if (lane == 0) {
                __hip_atomic_store(&s_base[(k + 1) & 7], nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (nb < 0) __hip_atomic_store(&s_done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_store(&s_ready[(k + 1) & 7], k + 2, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        if (b < 0) return -1;
        const int c = b * SC + o;
        return c < ntot ? c : -1;
    };
    {
        bool more = true;
        int pw = 0, pend = 0, pcol = 0;              // the run whose descriptor is asked for next, the end of its chunk, its column
        int rst[NR], rlen[NR], rwa[NR];              // runs in flight: first element, length, place-pass workgroup (< 0: none)
        int qv = 0, qw = -1;                         // the run after them, as loaded (lanes 0 and 1; made uniform when it moves up)
        // (a VECTOR load, lanes 0 and 1 fetching the two words: as a scalar load -- the address is uniform -- it counts on
        //  lgkmcnt, and the lgkmcnt(0) waits of the window reads then wait for IT: a trip to L2 in front of every window.
        //  The loaded register is only looked at when the run moves up, several runs later: reading it into scalars at once
        //  was a full memory round trip at every run boundary)
        auto fetch_run = [&](int &v, int &w) {
            if (pw == pend && more) {
                const int c = take_chunk();
                if (c < 0)
                    more = false;
                else {
                    const int ph = c < nedge ? 1 : 0;
                    pw = ph ? c * c1 : (c - nedge) * c0;
                    pend = pw + (ph ? c1 : c0);
                    pend = pend < nwg_all ? pend : nwg_all;
                    pcol = 2 * r + ph;
                }
            }
            v = 0;
            w = -1;
            if (pw < pend) {
                v = starts[(long long)pw * nb1 + pcol + (lane & 1)];
                w = pw;
                ++pw;
            }
        };
        {
            int fv[NR];
#pragma unroll
            for (int j = 0; j < NR; ++j) fetch_run(fv[j], rwa[j]);
            fetch_run(qv, qw);
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                rst[j] = __builtin_amdgcn_readlane(fv[j], 0);
                rlen[j] = __builtin_amdgcn_readlane(fv[j], 1) - rst[j];
            }
        }
        // this lane's next element of the stream, relative to the start of run 0.  Not simply the lane number: ds_read_b128
        // serves the lanes in four fixed sets of 16 per half wave ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}); each set takes 16
        // CONSECUTIVE elements of the stream, which the place pass dealt so that neighbours read different LDS slots
        int pos;
        {
            const int m = lane & 31;
            pos = (lane & 32) + (m < 4 ? m : (m < 12 ? m + 12 : (m < 16 ? m - 8 : (m < 20 ? m + 8 : (m < 28 ? m - 12 : m)))));
        }
        // locates the lane's next element (drops the runs every lane has passed) and requests its coordinates
        auto next_element = [&](bool &act, long long &oq, T (&xn)[D]) {
            while (rwa[0] >= 0 && __builtin_amdgcn_ballot_w64(pos < rlen[0]) == 0) {
                pos -= rlen[0];
#pragma unroll
                for (int j = 0; j + 1 < NR; ++j) { rst[j] = rst[j + 1]; rlen[j] = rlen[j + 1]; rwa[j] = rwa[j + 1]; }
                rst[NR - 1] = __builtin_amdgcn_readlane(qv, 0);
                rlen[NR - 1] = __builtin_amdgcn_readlane(qv, 1) - rst[NR - 1];
                rwa[NR - 1] = qw;
                fetch_run(qv, qw);
            }
            act = false;
            int off = 0, wa = 0, rel = pos;
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const bool here = !act && rel < rlen[j];
                if (here) { off = rst[j] + rel; wa = rwa[j]; }
                act = act || here;
                rel -= rlen[j];
            }
            if (act) {
                oq = (long long)wa * PR_Q + off;
#pragma unroll
                for (int d = 0; d < D; ++d) xn[d] = __builtin_nontemporal_load(xs + ((long long)wa * D + d) * PR_Q + off);
                pos += 64;
            }
        };
        // the coordinates of element i + 1 are requested between the basis tables and the window sum of element i: they
        // arrive while the window is read from LDS (without this the two memory round trips and the LDS phase of a wave simply
        // added up: 0.5 + 0.5 ms of a 1.2 ms pass per 5e7 queries, measured by leaving either out)
        bool act = false;
        long long oq = 0;
        T xc[D];
#pragma unroll
        for (int d = 0; d < D; ++d) xc[d] = (T)0;
        next_element(act, oq, xc);
        while (__builtin_amdgcn_ballot_w64(act) != 0) {
            double b[D][4];
            int base = 0;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int ws = eval_table<VAL>(g, d, (double)xc[d], nd.v[d], b[d]);
                base += (ws - a[d]) * PT::stride(d);
            }
            if (!act) base = 0;
            const bool act_c = act;
            const long long oq_c = oq;
            next_element(act, oq, xc);
            double sum;
            if constexpr (D == 3) {
                // window_sum<3> with the LDS reads written as inline assembly, one k2 plane (16 reads, 32 registers) at a time:
                // left to the compiler, all 64 reads of a window are issued up front (128 registers: 2 waves per SIMD, or
                // spills), and behind a function call the coordinates requested above would be waited for at the call (the
                // compiler drains every counter there).  Same operations in the same order as window_sum<3>: identical bits.
                // an odd window start reads the second copy of the tile, one entry down: every address is 16-byte aligned
                const unsigned la = (unsigned)(size_t)(const __attribute__((address_space(3))) double *)pr_tile +
                                    (unsigned)((base & 1) ? PT::COPY + base - 1 : base) * 8u;
                sum = 0.0;
                // (the reads need the window starts only and would move above the basis tables, which then spill: the first
                //  read names the tables as operands it does not use)
                asm volatile("; tables ready %0 %1 %2 %3 %4 %5" :: "v"(b[0][0]), "v"(b[0][3]), "v"(b[1][0]), "v"(b[1][3]), "v"(b[2][0]), "v"(b[2][3]));
                __builtin_amdgcn_sched_barrier(0);
                typedef double d2v __attribute__((ext_vector_type(2)));
#pragma unroll
                for (int k2 = 0; k2 < 4; ++k2) {
                    d2v c[4][2];
                    // (the first read of a plane names the running sum as an operand it does not use: the multiply-adds of the
                    //  plane before stay in front of it)
                    asm volatile("ds_read_b128 %0, %1 offset:%2 ; after %3" : "=v"(c[0][0]) : "v"(la), "n"((k2 * t2) * 8), "v"(sum));
#pragma unroll
                    for (int k1 = 0; k1 < 4; ++k1)
#pragma unroll
                        for (int h = (k1 == 0 ? 1 : 0); h < 2; ++h)
                            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(c[k1][h]) : "v"(la), "n"((k1 * t1 + k2 * t2 + 2 * h) * 8));
                    // (the values pass through the wait as in/out operands: what uses them stays behind it)
                    asm volatile("s_waitcnt lgkmcnt(0)"
                                 : "+v"(c[0][0]), "+v"(c[0][1]), "+v"(c[1][0]), "+v"(c[1][1]), "+v"(c[2][0]), "+v"(c[2][1]), "+v"(c[3][0]), "+v"(c[3][1])
                                 :: "memory");
                    double rr = 0.0;
#pragma unroll
                    for (int k1 = 0; k1 < 4; ++k1) {
                        double t = c[k1][0].x * b[0][0];
                        t = fma(c[k1][0].y, b[0][1], t);
                        t = fma(c[k1][1].x, b[0][2], t);
                        t = fma(c[k1][1].y, b[0][3], t);
                        rr = fma(t, b[1][k1], rr);
                    }
                    sum = fma(rr, b[2][k2], sum);
                    __builtin_amdgcn_sched_barrier(0);          // (the multiply-adds of a plane stay in front of the next plane's reads)
                }
            } else {
                sum = window_sum<D>(b, [&](int k1, int k2, int k3, double (&c)[4]) {
                    lds_row4(pr_tile, base + k1 * t1 + k2 * t2 + k3 * t3, c);
                });
            }
            if (act_c) __builtin_nontemporal_store((T)sum, outs + oq_c);
        }
    }      // chunks
    __syncthreads();                                 // every wave is done with the tile
    if (wave == 0) {
        // the next region: the one with the most chunks left per workgroup that would then be there
        int left = 0, there = 0;
        if (lane < nbins) {
            const int taken = __hip_atomic_load(queue + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            there = __hip_atomic_load(queue + nbins + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            left = (nch0 + (((edge_mask >> lane) & 1ull) ? nch1 : 0) + SC - 1) / SC - taken;
        }
        const float score = left > 0 ? (float)left / (float)(there + 1) : 0.0f;
        unsigned long long key = ((unsigned long long)__float_as_uint(score) << 32) | (unsigned)lane;
#pragma unroll
        for (int sft = 32; sft > 0; sft >>= 1) {
            const unsigned long long o = __shfl_xor(key, sft);
            key = o > key ? o : key;
        }
        if (lane == 0) {
            const int rn = (key >> 32) != 0 ? (int)(key & 63u) : -1;
            atomicSub(queue + nbins + r, 1);
            if (rn >= 0) atomicAdd(queue + nbins + rn, 1);
            s_region = rn;
        }
    }
    __syncthreads();
    }      // regions
}

// ---- persistent region path, 4-D (round 5) --------------------------------------------------------------------------------
// BASELINE config 5's evaluation half (4-D 32^4, 1e8 queries) ran the three-pass global region sort of round 3: seven launches
// per 2^24 queries, 287 B of fabric traffic per query for 40 algorithmic ones, the tile of a region (64 KB) loaded once per
// 2 048 queries: 8.07 ms per 1e8 queries.  Here the 3-D scheme above: pr_place_kernel<4> (regions of 8 window starts per
// dimension: 32^4 nodes give 4^4 = 256 regions, two bins each; the image holds 32-byte RECORDS of the coordinates and a byte
// per query with the LDS bank class of its window), this kernel, pr_unsort_kernel -- 32 + 35, 35 + 8 and 10 + 8 bytes per query:
// 6.2 ms per 1e8 queries (place 1.45, this kernel 4.4, unsort 0.33).
//   One persistent workgroup of 12 waves per CU (3 per SIMD: 168 registers, no spills; 16 waves left 128 and spilled in the round
//   loop) holds the tile of ONE region in LDS: (8 + 3)^4 coefficients with odd strides = 118 KB.  Its waves, each on its own,
//   take CHUNKS of the region's runs -- c0 consecutive place-pass workgroups of one bin -- from the region's counter (the number
//   of the next chunk is requested before the current one is worked on).  A chunk's run descriptors sit one per lane; a prefix
//   over the lanes makes the chunk ONE stream of elements, element e of which is found by a six-step search over the lanes'
//   prefixes -- runs of a 4-D place-pass workgroup are ~16 queries long (8 192 queries over 512 bins), too short for the 3-D
//   kernel's four-runs-in-flight walk.
//   What the counters and A/B builds showed, step by step (tools/eval4_bench.py, per 1e8 queries):
//   * elements in stream order: 5.3 ms in this kernel, the LDS pipe busy for 4.7 of them, 69 % of its cycles bank conflicts
//     (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE): the 256 window reads of a query (ds_read_b64: two groups of 32 lanes, 64 banks
//     of 4 bytes) all have the bank class of its tile offset mod 32, and 32 random classes per group collide 2-4 ways.
//   * so a wave DEALS every 256 elements of its chunk to its lanes by class, as round 3's region kernel dealt a workgroup's
//     2 048 queries: a counting sort in the wave's own LDS gives lanes h and h + 32 the elements of class h, two per round; what
//     a class holds beyond its 2 R slots goes to the free slots of short classes (conflicts: 69 % -> 43 % of the LDS cycles).
//   * dealt elements are scattered over the chunk: with coordinate PLANES every element cost four lines (2.8 ms); records: one
//     sector.  The 64 results of a round go to ~60 different lines: stored from the round they cost 1.2-1.4 ms (plain or
//     non-temporal stores alike); they are parked in the wave's LDS by element and leave in stream order, consecutive lanes on
//     consecutive slots.
//   * with the window reads taken out the kernel takes 2.3 ms (914 vector instructions per query: 340 multiply-adds, the
//     basis tables -- 45 % of the queries of a 32^4 grid have a window next to an end in some dimension --, two element
//     searches), with them 4.4: the reads do not overlap the arithmetic.  Software-pipelining them in units of 8 with
//     s_waitcnt lgkmcnt(8) broke: the compiler reloads fields of the by-value Grid argument with s_load inside the loop, which
//     count on lgkmcnt and return out of order (wrong values on a 20^4 grid), and the registers of a second buffer spilled.
//   * interleaving TWO elements per lane (one element's next 8 reads in flight while the other's are multiplied, waits of
//     lgkmcnt(0) only): 6.26 against 6.21 ms -- the reads are not waited for, the LDS pipe itself is the limit (its 2 cycles per
//     read become ~3.5 with the conflicts left, plus the deal's own traffic).  "Pure rounds + a mixed round for the surplus"
//     would cut the conflicts but adds a quarter more rounds of arithmetic at deals of 256: not built.
//   A workgroup whose region is used up moves to the region with the most chunks left.  No spinning anywhere: counters,
//   barriers, and loops every wave leaves when its region has no chunk left.
// Arithmetic per query: eval_table + window_sum<4> as everywhere else -- identical bits.
constexpr int PR4_EW = 768;        // threads of a 4-D evaluation workgroup: 12 waves = 3 per SIMD (168 registers each), one workgroup per CU
template <int SPER, bool VAL, typename T>
__global__ void __launch_bounds__(PR4_EW, 3)
pr_eval4_kernel(Grid g, PRegions rg, NDeriv nd, const T *__restrict__ coef, const T *__restrict__ xs, const unsigned char *__restrict__ scls,
                const int *__restrict__ starts, int nwg_all, int c0, int *__restrict__ queue, T *__restrict__ outs)
{
    constexpr int D = 4, PR_EW = PR4_EW, NWAVE = PR_EW / 64, SUB = 256, RMAX = SUB / 64, CAPMAX = 2 * RMAX;
    using PT = PTile<D, SPER>;
    __shared__ __attribute__((aligned(16))) double pr_tile[PT::ELEMS];
    __shared__ double w_res[NWAVE][SUB];             // results of a deal, by element: they leave in stream order (consecutive stores)
    __shared__ unsigned short w_list[NWAVE][32][CAPMAX], w_ovf[NWAVE][SUB];
    __shared__ int w_cnt[NWAVE][32];
    __shared__ int s_region;
    const int tid = threadIdx.x, lane = tid & 63, hcl = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int t1 = PT::S1, t2 = PT::S2, t3 = PT::S3;
    const int nbins = rg.nbins, nb1 = 2 * nbins + 1;
    const int nch = (nwg_all + c0 - 1) / c0;         // chunks per bin
    unsigned short (*list)[CAPMAX] = w_list[wave];
    unsigned short *ovf = w_ovf[wave];
    double *res = w_res[wave];
    int *cnt = w_cnt[wave];
    if (lane < 32) cnt[lane] = 0;
    // does region r hold windows that are not interior ones (its second bin is non-empty)?
    auto has_edge = [&](int r) {
        bool edge = false;
        int rr = r;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int rd = rr % rg.nreg[d], S = g.nodes[d] - 3;
            rr /= rg.nreg[d];
            const int lo = rd * rg.sper[d], hi = min(S, lo + rg.sper[d]);
            edge = edge || lo < 2 || hi > g.nodes[d] - 5;
        }
        return edge;
    };
    if (tid == 0) {
        // first region: workgroup b starts at region b mod nbins (more workgroups than regions: they share from the start)
        const int r0 = (int)(blockIdx.x % (unsigned)nbins);
        atomicAdd(queue + nbins + r0, 1);
        s_region = r0;
    }
    __syncthreads();
    int a[D];
    for (;;) {
        const int r = __builtin_amdgcn_readfirstlane(s_region);
        if (r < 0) break;
        {
            int rr = r;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                a[d] = (rr % rg.nreg[d]) * rg.sper[d];
                rr /= rg.nreg[d];
            }
            for (int e = tid; e < rg.tcells; e += PR_EW) {
                int rem = e, idx = 0, te = 0;
                bool ok = true;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const int l = rem % rg.text[d];
                    rem /= rg.text[d];
                    const int node = a[d] + l;
                    ok = ok && node < g.nodes[d];
                    idx += node * g.colstride[d];
                    te += l * PT::stride(d);
                }
                pr_tile[te] = ok ? (double)coef[idx] : 0.0;
            }
        }
        __syncthreads();
        const int nedge = has_edge(r) ? nch : 0;     // chunks of boundary runs come first (the costlier ones: no long tail)
        const int ntot = nedge + nch;
        auto take = [&]() {
            int v = 0;
            if (lane == 0) v = atomicAdd(queue + r, 1);
            return v;                                // (lane 0's register; made uniform when it is looked at)
        };
        int cnext = take();
        for (;;) {
            const int c = __builtin_amdgcn_readfirstlane(cnext);
            if (c >= ntot) break;
            cnext = take();                          // the next chunk's number travels while this chunk is worked on
            const int ph = c < nedge ? 1 : 0, cc = ph ? c : c - nedge;
            const int w0 = cc * c0, nw = min(c0, nwg_all - w0), col = 2 * r + ph;
            // one run per lane (c0 <= 64): start in its workgroup's image, inclusive prefix of the lengths
            int st_l = 0, len_l = 0;
            if (lane < nw) {
                const int *sp = starts + (long long)(w0 + lane) * nb1 + col;
                st_l = sp[0];
                len_l = sp[1] - st_l;
            }
            int pre = len_l;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(pre, o, 64);
                if (lane >= o) pre += t;
            }
            const int total = __builtin_amdgcn_readlane(pre, 63);
            const int excl = pre - len_l;
            // element e of the chunk -> its slot in the images (every lane takes part: the prefixes are read across the lanes)
            auto locate = [&](int e) -> unsigned {
                int lo = 0, hi = 63;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const int mid = (lo + hi) >> 1;
                    const int v = __shfl(pre, mid, 64);
                    if (v <= e) lo = mid + 1; else hi = mid;
                }
                const int off = __shfl(st_l, lo, 64) + (e - __shfl(excl, lo, 64));
                return (unsigned)(w0 + lo) * (unsigned)PR_Q + (unsigned)off;
            };
            auto request = [&](unsigned oq, bool act, T (&x)[D]) {
                // (records of the four coordinates: one or two 16-byte loads)
                typedef T rec4 __attribute__((ext_vector_type(4)));
                rec4 v = {(T)0, (T)0, (T)0, (T)0};
                if (act) v = __builtin_nontemporal_load(reinterpret_cast<const rec4 *>(xs) + oq);
                x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; x[3] = v[3];
            };
            for (int E0 = 0; E0 < total; E0 += SUB) {
                const int n = min(SUB, total - E0), R = (n + 63) >> 6, cap = 2 * R;
                // ---- deal the n elements to the lanes by class
                int ck[RMAX], rk[RMAX];
                unsigned oqk[RMAX];                  // (kept: the results are stored to these slots at the end of the deal)
#pragma unroll
                for (int k = 0; k < RMAX; ++k) {
                    const int i = k * 64 + lane;
                    const bool valid = k < R && i < n;
                    oqk[k] = locate(valid ? E0 + i : 0);
                    ck[k] = valid ? (int)scls[oqk[k]] : -1;
                }
#pragma unroll
                for (int k = 0; k < RMAX; ++k) rk[k] = ck[k] >= 0 ? atomicAdd(&cnt[ck[k]], 1) : 0;
                __builtin_amdgcn_wave_barrier();
                const int n_h = __hip_atomic_load(&cnt[hcl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                const int sur = n_h > cap ? n_h - cap : 0, fre = n_h < cap ? cap - n_h : 0;
                int is = sur, ifr = fre;
#pragma unroll
                for (int o = 1; o < 32; o <<= 1) {
                    const int ts = __shfl_up(is, o, 32), tf = __shfl_up(ifr, o, 32);
                    if (hcl >= o) { is += ts; ifr += tf; }
                }
                const int sur0 = is - sur, fre0 = ifr - fre, nsur = __shfl(is, 31, 32);
#pragma unroll
                for (int k = 0; k < RMAX; ++k) {
                    const int so = __shfl(sur0, ck[k] >= 0 ? ck[k] : 0, 32);
                    if (ck[k] >= 0) {
                        const unsigned short i = (unsigned short)(k * 64 + lane);
                        if (rk[k] < cap) list[ck[k]][rk[k]] = i;
                        else ovf[so + rk[k] - cap] = i;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                if (lane < 32) cnt[lane] = 0;         // (for the next deal; every lane has read its class's count)
                // lanes h and h + 32 walk the slots of class h (even / odd ones); a slot beyond the class's own elements takes
                // one of the surplus elements of the long classes, if any is left
                auto slot_element = [&](int t) -> int {
                    const int sl = 2 * t + half;
                    if (t >= R) return -1;
                    if (sl < n_h) return (int)list[hcl][sl];
                    const int f = fre0 + (sl - n_h);
                    return f < nsur ? (int)ovf[f] : -1;
                };
                int inext = slot_element(0);
                unsigned oq = locate(E0 + (inext >= 0 ? inext : 0));
                bool act = inext >= 0;
                T xc[D];
                request(oq, act, xc);
                for (int t = 0; t < R; ++t) {
                    double b[D][4];
                    int base = 0;
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        const int ws = eval_table<VAL>(g, d, (double)xc[d], nd.v[d], b[d]);
                        base += (ws - a[d]) * PT::stride(d);
                    }
                    if (!act) base = 0;
                    const bool act_c = act;
                    const int i_c = inext;
                    inext = slot_element(t + 1);
                    oq = locate(E0 + (inext >= 0 ? inext : 0));
                    act = inext >= 0;
                    request(oq, act, xc);
                    // window_sum<4> with the LDS reads as inline assembly, one (k2, k3) plane -- 16 ds_read_b64, 32 registers --
                    // at a time: left to the compiler the 256 reads of a window are hoisted and spill (450 registers to scratch
                    // in the first build of this kernel).  Same operations in the same order as window_sum<4>: identical bits.
                    // The k3 loop stays rolled (the plane's offsets are immediates on top of a base that advances by t3).
                    unsigned la = (unsigned)(size_t)(const __attribute__((address_space(3))) double *)pr_tile + (unsigned)base * 8u;
                    double sum = 0.0;
                    asm volatile("; tables ready %0 %1 %2 %3" :: "v"(b[0][0]), "v"(b[1][0]), "v"(b[2][0]), "v"(b[3][0]));
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
                    for (int k3 = 0; k3 < 4; ++k3) {
                        const double b3 = k3 == 0 ? b[3][0] : (k3 == 1 ? b[3][1] : (k3 == 2 ? b[3][2] : b[3][3]));
                        double q = 0.0;
#pragma unroll
                        for (int k2 = 0; k2 < 4; ++k2) {
                            double c[4][4];
                            asm volatile("ds_read_b64 %0, %1 offset:%2 ; after %3" : "=v"(c[0][0]) : "v"(la), "n"((k2 * t2) * 8), "v"(q));
#pragma unroll
                            for (int k1 = 0; k1 < 4; ++k1)
#pragma unroll
                                for (int k0 = (k1 == 0 ? 1 : 0); k0 < 4; ++k0)
                                    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(c[k1][k0]) : "v"(la), "n"((k0 + k1 * t1 + k2 * t2) * 8));
                            asm volatile("s_waitcnt lgkmcnt(0)"
                                         : "+v"(c[0][0]), "+v"(c[0][1]), "+v"(c[0][2]), "+v"(c[0][3]), "+v"(c[1][0]), "+v"(c[1][1]), "+v"(c[1][2]), "+v"(c[1][3]),
                                           "+v"(c[2][0]), "+v"(c[2][1]), "+v"(c[2][2]), "+v"(c[2][3]), "+v"(c[3][0]), "+v"(c[3][1]), "+v"(c[3][2]), "+v"(c[3][3])
                                         :: "memory");
                            double rr = 0.0;
#pragma unroll
                            for (int k1 = 0; k1 < 4; ++k1) {
                                double tt = c[k1][0] * b[0][0];
                                tt = fma(c[k1][1], b[0][1], tt);
                                tt = fma(c[k1][2], b[0][2], tt);
                                tt = fma(c[k1][3], b[0][3], tt);
                                rr = fma(tt, b[1][k1], rr);
                            }
                            q = fma(rr, b[2][k2], q);
                            __builtin_amdgcn_sched_barrier(0);      // (the multiply-adds of a plane stay in front of the next plane's reads)
                        }
                        sum = fma(q, b3, sum);
                        la += (unsigned)(t3 * 8);
                    }
                    // (the 64 results of a round belong to ~60 different lines of the images: stored from here they cost 1.2-1.4
                    //  of the pass's 4.5 ms per 1e8 queries, plain or non-temporal; they go through the wave's LDS instead)
                    if (act_c) res[i_c] = sum;
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int k = 0; k < RMAX; ++k)
                    if (ck[k] >= 0) __builtin_nontemporal_store((T)res[k * 64 + lane], outs + oqk[k]);
                __builtin_amdgcn_wave_barrier();     // (the lists are rewritten by the next deal)
            }
        }
        __syncthreads();                             // every wave is done with the tile
        if (tid < 64) {
            // the next region: the one with the most chunks left per workgroup that would then be there
            unsigned long long key = 0;
            for (int q0 = 0; q0 < nbins; q0 += 64) {
                const int q = q0 + lane;
                if (q < nbins) {
                    const int taken = __hip_atomic_load(queue + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const int there = __hip_atomic_load(queue + nbins + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const int left = (has_edge(q) ? 2 * nch : nch) - taken;
                    const float score = left > 0 ? (float)left / (float)(there + 1) : 0.0f;
                    const unsigned long long k = ((unsigned long long)__float_as_uint(score) << 32) | (unsigned)q;
                    key = k > key ? k : key;
                }
            }
#pragma unroll
            for (int sft = 32; sft > 0; sft >>= 1) {
                const unsigned long long o = __shfl_xor(key, sft);
                key = o > key ? o : key;
            }
            if (lane == 0) {
                const int rn = (key >> 32) != 0 ? (int)(key & 0xffffffffu) : -1;
                atomicSub(queue + nbins + r, 1);
                if (rn >= 0) atomicAdd(queue + nbins + rn, 1);
                s_region = rn;
            }
        }
        __syncthreads();
    }
}

// results of a place-pass workgroup's queries, from the sorted order of its image back to the caller's order: staged through
// LDS, so that both the read and the write are consecutive
template <typename T>
__global__ void __launch_bounds__(PR_NT)
pr_unsort_kernel(long long nq, const unsigned short *__restrict__ sidx, const int *__restrict__ starts, int nb1, const T *__restrict__ outs,
                 T *__restrict__ out)
{
    __shared__ T lv[PR_Q];
    const long long base = (long long)blockIdx.x * PR_Q;
    const int total = starts[(long long)blockIdx.x * nb1 + nb1 - 1];
    for (int p = threadIdx.x; p < total; p += PR_NT) lv[sidx[base + p]] = __builtin_nontemporal_load(outs + base + p);
    __syncthreads();
    const long long left = nq - base;
    const int n = left < PR_Q ? (int)left : PR_Q;
    // (every query of the workgroup has a region: total == n)
    for (int j = threadIdx.x; j < n; j += PR_NT) __builtin_nontemporal_store(lv[j], out + base + j);
}

// persistent region path: regions of the grid, or false when it does not apply (more than 64 regions / tiles beyond 64 KB)
template <int D>
static bool make_pregions(const Grid &g, PRegions &rg, int sper)
{
    rg.nbins = 1;
    rg.tcells = 1;
    for (int d = 0; d < MAXD; ++d) { rg.nreg[d] = 1; rg.sper[d] = 1; rg.text[d] = 1; rg.tstr[d] = 0; }
    for (int d = 0; d < D; ++d) {
        const int S = g.nodes[d] - 3;                // window starts 0 .. nodes - 4
        if (g.nodes[d] < 8 || S > 256) return false;
        rg.sper[d] = sper;
        rg.nreg[d] = (S + sper - 1) / sper;
        rg.text[d] = sper + 3;
        rg.nbins *= rg.nreg[d];
        rg.tcells *= rg.text[d];
    }
    if (rg.nbins < 8 || rg.nbins > PRCfg<D>::MAXBINS) return false;
    // (4-D: the runs of a place-pass workgroup hold ~16 queries for 32 slot classes -- nothing to deal)
    rg.deal = D == 3;
    // what the place pass needs to know of the evaluation pass's LDS tile: its strides and the distance of its second copy
    if constexpr (D == 4) {
        if (sper != 8) return false;                 // (a tile of 19^4 coefficients is 1 MB)
        using PT = PTile<D, 8>;
        for (int d = 0; d < D; ++d) rg.tstr[d] = PT::stride(d);
        rg.telems = 0;
    } else if (sper == 16) { using PT = PTile<D, 16>; for (int d = 0; d < D; ++d) rg.tstr[d] = PT::stride(d); rg.telems = PT::W128 ? PT::COPY : 0; }
    else { using PT = PTile<D, 8>; for (int d = 0; d < D; ++d) rg.tstr[d] = PT::stride(d); rg.telems = PT::W128 ? PT::COPY : 0; }
    return true;
}

// local indices | (4-D) LDS slot class of every sorted query | run starts | sorted coordinates [workgroup][D][PR_Q] (4-D: records)
// | sorted results | the regions' chunk counters
enum { P_SIDX, P_SCLS, P_STARTS, P_XS, P_OUTS, P_CLAIM, P_COUNT };
static thread_local DevScratch<P_COUNT> g_pscratch;
static thread_local int g_pscratch_ncu = 0;         // compute units of the device the scratch is on (0: not asked yet)

void eval_persistent_shutdown() { g_pscratch.release(); }

// nfields coefficient sets (ldcoef apart) at the same queries, results ldout apart: the place pass runs ONCE, then every field
// takes the evaluation and the unsort pass in stream order (an evaluation pass consumes the chunk counters: cleared per field)
template <int D, typename T>
static hipError_t eval_persistent_d(const Grid &g, long long nq, const T *xq, int ldxq, const NDeriv &nd, const T *coef, T *out, hipStream_t st,
                                    int nfields, long long ldcoef, long long ldout)
{
    // regions of 16 window starts per dimension (tiles of 19^3 = 55 KB: 64^3 nodes give 4 x 4 x 4 regions), of 8 for smaller grids
    PRegions rg;
    int sper = D == 4 ? 8 : 16;
    if (!make_pregions<D>(g, rg, sper)) {
        sper = 8;
        if (D == 4 || !make_pregions<D>(g, rg, sper)) return hipErrorNotSupported;
    }
    const long long nwg_ll = (nq + PR_Q - 1) / PR_Q;
    if (nwg_ll > 0x3fffffffLL / (2 * rg.nbins + 1)) return hipErrorNotSupported;
    const int nwg = (int)nwg_ll;
    if (nwg_ll * PR_Q > 0xffffffffLL) return hipErrorNotSupported;          // (32-bit query indices in the evaluation kernel)
    const size_t need_q = (size_t)nwg_ll * PR_Q;
    size_t need[P_COUNT];
    need[P_SIDX] = sizeof(unsigned short) * need_q;
    need[P_SCLS] = need_q + 16;
    need[P_STARTS] = sizeof(int) * (size_t)nwg_ll * (2 * rg.nbins + 1);
    need[P_XS] = sizeof(T) * need_q * D;
    need[P_OUTS] = sizeof(T) * need_q;
    need[P_CLAIM] = sizeof(int) * 2 * PR_MAXBINS;
    DevScratch<P_COUNT> &s = g_pscratch;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (s.dev != dev) g_pscratch_ncu = 0;
    // (no room: the other paths need less -- no retry at the expense of the cached plan)
    if (s.ensure(dev, need, /*may_release_plan=*/false) != hipSuccess) { (void)hipGetLastError(); return hipErrorNotSupported; }
    (void)s.wait_on(st);
    unsigned short *sidx = s.as<unsigned short>(P_SIDX);
    unsigned char *scls = s.as<unsigned char>(P_SCLS);
    int *starts = s.as<int>(P_STARTS), *claim = s.as<int>(P_CLAIM);
    T *xs = s.as<T>(P_XS), *outs = s.as<T>(P_OUTS);
    const bool plain = value_only(nd);
    hipError_t e = hipMemsetAsync(claim, 0, sizeof(int) * 2 * PR_MAXBINS, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((pr_place_kernel<D, T>), dim3((unsigned)nwg), dim3(PR_NT), 0, st, g, rg, nq, xq, ldxq, sidx, starts, xs, scls);
    // persistent workers: one workgroup per CU
    if (g_pscratch_ncu <= 0) {
        int v = 0;
        g_pscratch_ncu = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
    }
    const dim3 grid((unsigned)g_pscratch_ncu);
    for (int k = 0; k < nfields; ++k) {
        const T *coefk = coef + (long long)k * ldcoef;
        if (k > 0) {
            e = hipMemsetAsync(claim, 0, sizeof(int) * 2 * PR_MAXBINS, st);
            if (e != hipSuccess) break;
        }
        if constexpr (D == 4) {
            // chunks of 32 place-pass workgroups of one bin: ~500 queries (a chunk's runs sit one per lane: at most 64)
            const int c0 = 32;
            hipLaunchKernelGGL((plain ? pr_eval4_kernel<8, true, T> : pr_eval4_kernel<8, false, T>), grid, dim3(PR4_EW), 0, st, g, rg, nd, coefk,
                               (const T *)xs, (const unsigned char *)scls, (const int *)starts, nwg, c0, claim, outs);
        } else {
            // (chunks of 4 place-pass workgroups of interior runs, 16 of boundary runs: ~400 queries; the waves of a workgroup
            //  take them from a counter in LDS, so small chunks cost nothing and keep the tails short)
            const int c0 = 4;
            hipLaunchKernelGGL((sper == 16 ? (plain ? pr_eval_kernel<D, 16, true, T> : pr_eval_kernel<D, 16, false, T>)
                                           : (plain ? pr_eval_kernel<D, 8, true, T> : pr_eval_kernel<D, 8, false, T>)),
                               grid, dim3(PR_EW), 0, st, g, rg, nd, coefk, (const T *)xs, (const int *)starts, nwg, c0, claim, outs);
        }
        hipLaunchKernelGGL((pr_unsort_kernel<T>), dim3((unsigned)nwg), dim3(PR_NT), 0, st, nq, (const unsigned short *)sidx, (const int *)starts,
                           2 * rg.nbins + 1, (const T *)outs, out + (long long)k * ldout);
    }
    (void)s.mark_used(st);
    return e != hipSuccess ? e : hipGetLastError();
}

template <typename T>
hipError_t eval_persistent(const Grid &g, long long nq, const T *xq, int ldxq, const NDeriv &nd, const T *coef, T *out, hipStream_t st,
                           int nfields, long long ldcoef, long long ldout)
{
    if (g.ndim == 3) return eval_persistent_d<3, T>(g, nq, xq, ldxq, nd, coef, out, st, nfields, ldcoef, ldout);
    if (g.ndim == 4) return eval_persistent_d<4, T>(g, nq, xq, ldxq, nd, coef, out, st, nfields, ldcoef, ldout);
    return hipErrorNotSupported;
}
template hipError_t eval_persistent<double>(const Grid &, long long, const double *, int, const NDeriv &, const double *, double *, hipStream_t, int,
                                            long long, long long);
template hipError_t eval_persistent<float>(const Grid &, long long, const float *, int, const NDeriv &, const float *, float *, hipStream_t, int,
                                           long long, long long);

}  // namespace splpak
