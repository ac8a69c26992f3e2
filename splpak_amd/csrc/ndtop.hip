// The top of the nested-dissection tree in a ONE-PROCESS MULTI-GPU fit (round 4).
//
// splpak_mplan_* / splpak_fit_multi_f64 (what a Fortran caller reaches through `set_gpus(n)`) give every GPU a plan and a
// host thread.  When the grid takes the nested-dissection factorisation -- the replacement of suprls' triangularisation and
// back-substitution, src/splpak.F90:1375-1695 -- it is distributed like this (ndtree.hpp NdPartition):
//
//   * below tree depth dcut = ceil(log2 ranks) every subtree belongs to ONE rank, which stores and eliminates it with the
//     single-GPU machinery of ndchol.hip (its panels, Schur arenas and block inverses exist on that GPU only);
//   * a front above (a "top front") is one square lower-triangular matrix [own | border] cut into block columns of 256 that
//     are dealt to the ranks.  Per block step k: owner(k) factors the diagonal block and solves the panel below it, every
//     other rank copies the solved panel over xGMI (hipMemcpyPeerAsync, straight out of the owner's block column: it is
//     final) and updates the block columns IT owns; owner(k+1) updates block column k+1 first, on its chain stream, and
//     factors it while everybody's bulk update by panel k is still running (one block column of look-ahead, as in dist.hip);
//   * a child's Schur complement is PULLED by the owners of the parent's block columns (nd_pull_add_kernel reads the child's
//     columns through the peer mapping, lower triangle only, slot 0 before slot 1), after a barrier that says the child is final;
//   * the solves walk the subtrees locally and the top fronts step by step, the front's vector travelling from owner to owner.
//
// Every element sees the same operations in the same order as in the single-GPU factorisation (the update of a tile by block
// k is the same K = 256 MFMA sequence whether it runs alone or as one trip of a K = 1024 pass), so the coefficients are
// bitwise those of the single-GPU nested-dissection fit.
//
// Host-side protocol: a rank's thread walks the global sequence of top steps in order and only ever waits for flags of
// EARLIER steps (set by their owners when they enqueue them, generation-stamped so that nothing is reset between fits), so
// the walk cannot deadlock; every wait watches the fit's abort flag.
#include "ndstate.hpp"
#include <thread>

namespace splpak {
namespace nd {

namespace {

inline NdState *rank_state(NdGroup *g, int r) { return static_cast<NdState *>(g->st[(size_t)r]); }
inline std::atomic<int> &grp_abort(NdGroup *g) { return g->abort ? *g->abort : g->own_abort; }

template <typename F>
bool nd_wait(NdGroup *g, F &&ready)
{
    while (!ready()) {
        if (grp_abort(g).load(std::memory_order_relaxed)) return false;
        std::this_thread::yield();
    }
    return true;
}

#define NTRY(expr)                                            \
    do {                                                      \
        hipError_t e_ = (expr);                               \
        if (e_ != hipSuccess) { grp_abort(g).store(1); return e_; } \
    } while (0)

// the one map job `job` of a table (-1: none)
inline void top_map(const JobTable<MapJob> &tab, int job, bool take, hipStream_t st) { if (job >= 0) launch_map(tab, Launch{job, 1, 1, 0}, take, st); }

}  // namespace

// Factorisation of the top fronts (after every rank has eliminated its subtrees).
hipError_t nd_top_factor(NdState *s, hipStream_t st, int *info_dev, double *minpiv_dev, CholStats *stats, bool timing)
{
    NdGroup *g = s->grp;
    NdTree &t = s->t;
    const NdPartition &pt = s->top.pt;
    const int me = s->mrank, gen = s->top.fgen;
    hipStream_t sP = s->str.sP, sU = s->str.sU, sC = s->str.sCopy;
    int qnext = 1 << 30;
    // the subtrees' Schur complements are final and visible, on every rank
    for (hipStream_t q : {sP, sU, s->str.sR, st})
        if (q) NTRY(hipStreamSynchronize(q));
    if (!g->bar.wait(grp_abort(g))) return hipErrorUnknown;
    int pslot_step[3] = {-1, -1, -1};
    int d_prev = -1;
    for (size_t ti = 0; ti < pt.top.size(); ++ti) {
        const NdFront &f = t.fr[(size_t)pt.top[ti]];
        if (d_prev >= 0 && f.depth != d_prev) {      // the fronts of the depth below are complete everywhere before their parents pull
            for (hipStream_t q : {sP, sU, sC}) NTRY(hipStreamSynchronize(q));
            if (!g->bar.wait(grp_abort(g))) return hipErrorUnknown;
        }
        d_prev = f.depth;
        for (int sl = 0; sl < 2; ++sl) {             // extend-add: the child of slot 0, then the child of slot 1
            const Launch &lp = s->top.l_pull[sl][ti];
            launch_pull(s->top.pull, lp, sU);
        }
        NTRY(hipEventRecord(s->top.evAdd[ti], sU));
        const int s0 = pt.seq0[ti];
        // block column k is complete on the chain stream: factor its diagonal block, solve its panel, post it
        auto factor_column = [&](int k) -> hipError_t {
            const int sq = s0 + k;
            launch_potrf(s, s->top.potrf, s->top.potrf.l[0][(size_t)sq], sP, info_dev, minpiv_dev);
            launch_trsm(s->top.trsm, s->top.trsm.l[0][(size_t)sq], sP);
            const hipError_t e = hipEventRecord(s->top.evReady[(size_t)sq], sP);
            g->posted[(size_t)sq].store(gen, std::memory_order_release);
            return e;
        };
        if (top_owner(pt, 0) == me) {
            NTRY(hipStreamWaitEvent(sP, s->top.evAdd[ti], 0));
            NTRY(factor_column(0));
        }
        for (int k = 0; k < f.nsteps; ++k) {
            const int sq = s0 + k, o = top_owner(pt, k);
            const Launch &lc = s->top.chain.l[0][(size_t)sq], &lb = s->top.bulk.l[0][(size_t)sq];
            const bool have_updates = (lc.count && lc.grid) || (lb.count && lb.grid);
            bool arrived = false;
            if (o == me) NTRY(hipStreamWaitEvent(sU, s->top.evReady[(size_t)sq], 0));
            else if (have_updates) {
                if (!nd_wait(g, [&] { return g->posted[(size_t)sq].load(std::memory_order_acquire) == gen; })) return hipErrorUnknown;
                NdState *ro = rank_state(g, o);
                NTRY(hipStreamWaitEvent(sC, ro->top.evReady[(size_t)sq], 0));
                const int ps = s->top.rslot[(size_t)sq];
                const int prev = pslot_step[ps];          // the receive buffer was last read by the updates by that step's panel
                if (prev >= 0) {
                    NTRY(hipStreamWaitEvent(sC, s->top.evBulk[(size_t)prev], 0));
                    NTRY(hipStreamWaitEvent(sC, s->top.evCol[(size_t)prev], 0));
                }
                pslot_step[ps] = sq;
                const TopColDev &ck = top_col(ro, ti, k);
                const long long rows = (long long)f.fp - (long long)k * 256;
                if (rows > 256)                           // rows below the diagonal block of column 0 .. the last row of column 255: one range
                    NTRY(hipMemcpyPeerAsync(s->top.pbuf[ps], s->device, ro->factor + ck.off + 256, ro->device, sizeof(double) * (size_t)(255 * ck.ld + rows - 256), sC));
                NTRY(hipEventRecord(s->top.evArr[(size_t)sq], sC));
                NTRY(hipStreamWaitEvent(sU, s->top.evArr[(size_t)sq], 0));
                arrived = true;
            }
            if (lc.count) {                               // the chain: the owner of block column k + 1 updates it first, then factors it
                if (o != me && arrived) NTRY(hipStreamWaitEvent(sP, s->top.evArr[(size_t)sq], 0));
                if (k >= 1) NTRY(hipStreamWaitEvent(sP, s->top.evBulk[(size_t)(sq - 1)], 0));      // the earlier updates of that column
                else NTRY(hipStreamWaitEvent(sP, s->top.evAdd[ti], 0));
                launch_syrk(s, s->top.chain, lc, sP, stats, timing, false, false, qnext);
                NTRY(hipEventRecord(s->top.evCol[(size_t)sq], sP));
                NTRY(factor_column(k + 1));
            } else
                NTRY(hipEventRecord(s->top.evCol[(size_t)sq], sU));
            launch_syrk(s, s->top.bulk, lb, sU, stats, timing, true, false, qnext);
            NTRY(hipEventRecord(s->top.evBulk[(size_t)sq], sU));
        }
    }
    for (hipStream_t q : {sP, sU, sC}) NTRY(hipStreamSynchronize(q));
    if (!g->bar.wait(grp_abort(g))) return hipErrorUnknown;      // nobody's block columns are still being read
    launch_trinv(s->top.trinv.dev, (int)s->top.trinv.host.size(), st);
    return hipGetLastError();
}

// pivot status of a distributed factorisation: a failure anywhere is a failure everywhere (every rank takes the same way out)
hipError_t nd_top_pivots(NdState *s, hipStream_t st, int *info_dev, double *minpiv_dev)
{
    NdGroup *g = s->grp;
    const int me = s->mrank;
    int hi = 0;
    double hp = 0.0;
    NTRY(hipMemcpyAsync(&hi, info_dev, sizeof(int), hipMemcpyDeviceToHost, st));
    NTRY(hipMemcpyAsync(&hp, minpiv_dev, sizeof(double), hipMemcpyDeviceToHost, st));
    NTRY(hipStreamSynchronize(st));
    g->h_info[(size_t)me] = hi;
    g->h_minpiv[(size_t)me] = hp;
    if (!g->bar.wait(grp_abort(g))) return hipErrorUnknown;
    int info = 0;
    double piv = hp;
    for (int r = 0; r < g->R; ++r) {
        const int v = g->h_info[(size_t)r];
        const double q = g->h_minpiv[(size_t)r];
        if (v != 0 && (info == 0 || v < info)) info = v;
        if (q < piv || !(q == q)) piv = q;
    }
    if (!g->bar.wait(grp_abort(g))) return hipErrorUnknown;      // everybody has read the table
    NTRY(hipMemcpyAsync(info_dev, &info, sizeof(int), hipMemcpyHostToDevice, st));
    NTRY(hipMemcpyAsync(minpiv_dev, &piv, sizeof(double), hipMemcpyHostToDevice, st));
    NTRY(hipStreamSynchronize(st));
    return hipSuccess;
}

// Forward sweep over the top fronts (this rank's subtrees are done on `st`).
hipError_t nd_top_forward(NdState *s, hipStream_t st)
{
    NdGroup *g = s->grp;
    NdTree &t = s->t;
    const NdPartition &pt = s->top.pt;
    const int me = s->mrank, gen = s->top.sgen;
    NTRY(hipEventRecord(s->top.evSub, st));
    g->subdone[(size_t)me].store(gen, std::memory_order_release);
    for (size_t ti = 0; ti < pt.top.size(); ++ti) {
        const NdFront &f = t.fr[(size_t)pt.top[ti]];
        const int s0 = pt.seq0[ti];
        double *Vf = s->V + f.vofs;
        for (int k = 0; k < f.nsteps; ++k) {
            if (top_owner(pt, k) != me) continue;
            const int sq = s0 + k;
            if (k == 0) {                                 // the children's border updates, slot 0 then slot 1
                for (int sl = 0; sl < 2; ++sl) {
                    const int cid = f.child[sl];
                    if (cid < 0) continue;
                    const NdFront &c = t.fr[(size_t)cid];
                    int q;
                    hipEvent_t ev;
                    if (pt.owner[(size_t)cid] >= 0) {
                        q = pt.owner[(size_t)cid];
                        if (!nd_wait(g, [&] { return g->subdone[(size_t)q].load(std::memory_order_acquire) == gen; })) return hipErrorUnknown;
                        ev = rank_state(g, q)->top.evSub;
                    } else {
                        const int sc = pt.seq0[(size_t)pt.top_index[(size_t)cid]] + c.nsteps - 1;
                        q = top_owner(pt, c.nsteps - 1);
                        if (!nd_wait(g, [&] { return g->fposted[(size_t)sc].load(std::memory_order_acquire) == gen; })) return hipErrorUnknown;
                        ev = rank_state(g, q)->top.evSF[(size_t)sc];
                    }
                    NdState *rq = rank_state(g, q);
                    if (q != me) NTRY(hipStreamWaitEvent(st, ev, 0));
                    if (c.h > 0) {
                        NTRY(hipMemcpyPeerAsync(s->top.stagev, s->device, rq->V + c.vofs + c.wp, rq->device, sizeof(double) * (size_t)c.h, st));
                        top_map(s->top.mapf, s->top.l_mapf[sl][ti], false, st);
                    }
                }
            } else if (top_owner(pt, k - 1) != me) {      // the rows the earlier steps have updated
                const int q = top_owner(pt, k - 1);
                if (!nd_wait(g, [&] { return g->fposted[(size_t)(sq - 1)].load(std::memory_order_acquire) == gen; })) return hipErrorUnknown;
                NdState *rq = rank_state(g, q);
                NTRY(hipStreamWaitEvent(st, rq->top.evSF[(size_t)(sq - 1)], 0));
                NTRY(hipMemcpyPeerAsync(Vf + k * 256, s->device, rq->V + f.vofs + k * 256, rq->device, sizeof(double) * (size_t)(f.fp - k * 256), st));
            }
            launch_mv(s->top.mv, s->top.mv.l[0][(size_t)sq], st);
            launch_fwd(s->top.fwd, s->top.fwd.l[0][(size_t)sq], st);
            NTRY(hipEventRecord(s->top.evSF[(size_t)sq], st));
            g->fposted[(size_t)sq].store(gen, std::memory_order_release);
        }
    }
    return hipGetLastError();
}

// Backward sweep over the top fronts, root first; then this rank's subtree roots take their border values.
hipError_t nd_top_backward(NdState *s, hipStream_t st)
{
    NdGroup *g = s->grp;
    NdTree &t = s->t;
    const NdPartition &pt = s->top.pt;
    const int me = s->mrank, gen = s->top.sgen;
    // the whole vector of a parent front, from the rank that ended its backward sweep, into the staging buffer
    auto pull_parent = [&](int pid) -> hipError_t {
        const NdFront &P = t.fr[(size_t)pid];
        const int sp = pt.seq0[(size_t)pt.top_index[(size_t)pid]], q = top_owner(pt, 0);
        if (!nd_wait(g, [&] { return g->bposted[(size_t)sp].load(std::memory_order_acquire) == gen; })) return hipErrorUnknown;
        NdState *rq = rank_state(g, q);
        if (q != me) NTRY(hipStreamWaitEvent(st, rq->top.evSB[(size_t)sp], 0));
        NTRY(hipMemcpyPeerAsync(s->top.stagev, s->device, rq->V + P.vofs, rq->device, sizeof(double) * (size_t)P.fp, st));
        return hipSuccess;
    };
    for (size_t tr = pt.top.size(); tr-- > 0;) {
        const size_t ti = tr;
        const NdFront &f = t.fr[(size_t)pt.top[ti]];
        const int s0 = pt.seq0[ti];
        double *Vf = s->V + f.vofs;
        for (int k = f.nsteps - 1; k >= 0; --k) {
            if (top_owner(pt, k) != me) continue;
            const int sq = s0 + k;
            if (k == f.nsteps - 1) {
                if (f.parent >= 0 && f.h > 0) {
                    NTRY(pull_parent(f.parent));
                    top_map(s->top.mapb, s->top.l_mapb[ti], true, st);
                }
            } else if (top_owner(pt, k + 1) != me) {
                const int q = top_owner(pt, k + 1);
                if (!nd_wait(g, [&] { return g->bposted[(size_t)(sq + 1)].load(std::memory_order_acquire) == gen; })) return hipErrorUnknown;
                NdState *rq = rank_state(g, q);
                NTRY(hipStreamWaitEvent(st, rq->top.evSB[(size_t)(sq + 1)], 0));
                NTRY(hipMemcpyPeerAsync(Vf + (k + 1) * 256, s->device, rq->V + f.vofs + (k + 1) * 256, rq->device,
                                        sizeof(double) * (size_t)(f.fp - (k + 1) * 256), st));
            }
            launch_dot(s->top.dot, s->top.dot.l[0][(size_t)sq], st);
            launch_bwd(s->top.bwd, s->top.bwd.l[0][(size_t)sq], st);
            NTRY(hipEventRecord(s->top.evSB[(size_t)sq], st));
            g->bposted[(size_t)sq].store(gen, std::memory_order_release);
        }
    }
    for (size_t i = 0; i < s->top.subroots.size(); ++i) {
        const NdFront &c = t.fr[(size_t)s->top.subroots[i]];
        if (c.parent < 0 || c.h == 0) continue;
        NTRY(pull_parent(c.parent));
        top_map(s->top.maps, s->top.l_maps[i], true, st);
    }
    return hipGetLastError();
}

#undef NTRY

}  // namespace nd

using nd::NdState;
using nd::rank_state;

NdGroup *nd_group_create(int R, int chunk, std::atomic<int> *abort)
{
    NdGroup *g = new NdGroup();
    g->R = R < 1 ? 1 : R;
    g->chunk = chunk < 1 ? 1 : chunk;
    g->abort = abort;
    g->st.assign((size_t)g->R, nullptr);
    g->bar.n = g->R;
    g->h_info.assign((size_t)g->R, 0);
    g->h_minpiv.assign((size_t)g->R, 0.0);
    return g;
}

void nd_group_destroy(NdGroup *g) { delete g; }

// Before the rank threads of a fit start (single-threaded).  The progress flags of the top phase are compared with each
// rank's private generation counters; a fit that was abandoned while the ranks stood at different points (one had entered
// nd_factor / nd_solve, another had not) used to leave them apart for good, and the next fit on the same plan then spun in
// nd_wait (round-4 advice).  Every fit now starts all ranks from ONE group-wide base, far above anything a fit adds.
void nd_group_reset(NdGroup *g)
{
    if (!g) return;
    g->bar.reset();
    g->gen += 4096;                         // (a fit enters nd_factor once and nd_solve at most 1 + 30 times)
    for (void *q : g->st)
        if (q) {
            NdState *s = static_cast<NdState *>(q);
            s->top.fgen = g->gen;
            s->top.sgen = g->gen;
        }
}

int nd_group_finalize(NdGroup *g)
{
    if (!g || g->R <= 1) return 0;
    for (void *q : g->st)
        if (!q || !static_cast<NdState *>(q)->mdist) { set_error("nested dissection: a rank of the multi-GPU fit has no plan"); return SPLPAK_E_BADARG; }
    g->nseq = rank_state(g, 0)->top.pt.nseq;
    auto mk = [](size_t n) {
        std::unique_ptr<std::atomic<int>[]> a(new std::atomic<int>[n]);
        for (size_t i = 0; i < n; ++i) a[i].store(-1);
        return a;
    };
    g->posted = mk((size_t)g->nseq + 1);
    g->fposted = mk((size_t)g->nseq + 1);
    g->bposted = mk((size_t)g->nseq + 1);
    g->subdone = mk((size_t)g->R);
    int cur = 0;
    (void)hipGetDevice(&cur);
    int rc = 0;
    for (int r = 0; r < g->R && rc == 0; ++r) {
        NdState *s = rank_state(g, r);
        (void)hipSetDevice(s->device);
        if (!nd_build_top_jobs(s)) rc = SPLPAK_E_NOMEM;
    }
    (void)hipSetDevice(cur);
    g->finalized = rc == 0;
    return rc;
}

}  // namespace splpak
