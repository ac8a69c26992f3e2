// Nested-dissection multifrontal Cholesky of the normal equations on gfx950.
//
// Replaces, for large 3-D / 4-D grids, the band factorisation of bandchol.hip -- and through it the dense
// row-streaming Householder triangularisation + back-substitution of suprls (src/splpak.F90:1375-1695, called
// from splcw :849, :1025, :1052) -- by a factorisation in the nested-dissection order of ndtree.hpp: 1.2e13
// flop and 14 GB of factor at 64^3 nodes instead of 4.1e13 / 26.9 GB, 2.7e14 flop at 24^4 instead of 6.2e14.
// The refinement against the rows (planfit.hip) is unchanged, so the result is the same minimiser.
//
// Every front is a dense column-major PANEL (rows: own | border, columns: own, padded to 256 with identity)
// and, while it is being eliminated, a dense Schur buffer S (border x border):
//
//     for the 256-column blocks k of the panel:   potrf(k) -> panel solve of all rows below -> update of the
//         panel columns right of k (chain stream) ;  S -= L21_k L21_k^T (second stream, beside the chain of k+1)
//     then S is added into the parent's panel / Schur buffer through the monotone child -> parent row map.
//
// Fronts of one tree depth are processed TOGETHER: every launch is a batch over job tables built once per plan
// (potrf: a workgroup per front; panel solve: a wave per 16 rows; updates: a wave per 64x64x256 item on the f64
// matrix cores, the register-streaming form of bandchol.hip's trailing update).  The two children of a parent
// add their Schur complements in two launches (slot 0, then slot 1), so every sum has a fixed order: the
// factor is bitwise reproducible from run to run.
//
// Solves walk the tree with per-front local vectors: forward bottom-up (gather the right-hand side, add the
// children's border updates, y_k = Linv_k v_k and v_below -= L_below,k y_k per block), backward top-down (border
// values from the parent, x_k = Linv_k^T (y_k - L_below,k^T x_below)), with explicit inverses of the 256x256
// diagonal blocks as in bandchol.hip.
#include "ndstate.hpp"
#include <cstdlib>

namespace splpak {
namespace nd {

// The panels start from zero (14 GB at 64^3: 2.2 ms of memset).  Only the head of the arena is busy during the assembly -- the
// per-cell Gram blocks live there until the stencil gather has read them -- so the rest is cleared on the second stream
// while the points are binned and the blocks computed, and nd_assemble clears the head.
hipError_t nd_prefit(splpak_plan *p, hipStream_t st, void *user)
{
    NdState *s = static_cast<NdState *>(user);
    s->tail_pending = false;
    if (s->sch.staged_init && !s->dist) return hipSuccess;         // (nothing to clear: nd_init_kernel writes every panel column whole)
    if (!s->str.sU || !s->ev.evPre || splpak::opt_get("SPLPAK_ND_NO_EARLY_CLEAR")) return hipSuccess;
    long long head = 0;
    if (p->gscratch == s->factor) head = p->gscratch_doubles < s->factor_doubles ? p->gscratch_doubles : s->factor_doubles;
    else if (p->gscratch >= s->factor && p->gscratch < s->factor + s->factor_doubles) return hipSuccess;     // (not laid out that way)
    if (head >= s->factor_doubles) return hipSuccess;
    hipError_t e = hipEventRecord(s->ev.evPre, st);                 // the previous fit's solves have read the factor by now
    if (e == hipSuccess) e = hipStreamWaitEvent(s->str.sU, s->ev.evPre, 0);
    const int clear_wgs = splpak::opt_get("SPLPAK_ND_CLEAR_WGS") ? atoi(splpak::opt_get("SPLPAK_ND_CLEAR_WGS")) : 128;
    if (e == hipSuccess) {
        if (clear_wgs > 0) {
            launch_clear(clear_wgs, s->factor + head, s->factor_doubles - head, s->str.sU);
            e = hipGetLastError();
        } else
            e = hipMemsetAsync(s->factor + head, 0, sizeof(double) * (size_t)(s->factor_doubles - head), s->str.sU);
    }
    if (e == hipSuccess) e = hipEventRecord(s->ev.evTail, s->str.sU);
    if (e != hipSuccess) return e;
    s->tail_pending = true;
    s->head_doubles = head;
    return hipSuccess;
}

hipError_t nd_assemble(splpak_plan *p, hipStream_t st, void *user)
{
    NdState *s = static_cast<NdState *>(user);
    hipError_t e = hipSuccess;
    if (s->sch.staged_init && !s->dist) {             // the stages whose panels are alive when the first stage starts; the others in nd_factor
        if (!s->sch.istarts.empty())
            for (int x : s->sch.istarts[0]) launch_init(s, p->g, p->nst, s->fac.init.l[(size_t)x][0], st);
        return hipGetLastError();
    }
    if (s->tail_pending) {
        if (s->head_doubles > 0) e = hipMemsetAsync(s->factor, 0, sizeof(double) * (size_t)s->head_doubles, st);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, s->ev.evTail, 0);
        s->tail_pending = false;
    } else
        e = hipMemsetAsync(s->factor, 0, sizeof(double) * (size_t)s->factor_doubles, st);
    if (e != hipSuccess) return e;
    launch_assemble(s, p->g, p->nst, st);
    return hipGetLastError();
}

namespace {

// one call of nd_factor
struct FactorRun {
    splpak_plan *p;
    NdState *s;
    hipStream_t st, sP, sU, sR;         // the plan's stream; chain, updates, reserved CUs as chosen for this call (SPLPAK_NO_LOOKAHEAD: all = st; sR NULL: no pinning)
    int *info_dev;
    double *minpiv_dev;
    CholStats *stats;
    bool timing;
    int pin_rounds;                     // potrf goes to the reserved CUs while a stage has at most this many diagonal blocks per step per reserved CU
    int qnext = 0;                      // next unused item queue
    int la_evt = -1;                    // step whose next-diagonal-block update is marked by evW (look-ahead inside a group)
    bool joined = false, comm_failed = false;       // joined: (dist) the subtrees' Schur complements are summed
    void syrk(const JobTable<SyrkJob> &tab, const Launch &l, hipStream_t q, bool schur, bool pinned) { launch_syrk(s, tab, l, q, stats, timing, schur, pinned, qnext); }
    void begin();                       // (the pieces of nd_factor) the waits on the previous fit, the first zeroing, the queue reset, the dist memsets
    void dist_join();
    void potrf_step(const Launch &lp, int k, hipStream_t sC, bool reserved, hipEvent_t after);
    void stage_prep(int i);
    void chain_step(int stg, int k, bool pinned, bool pin_potrf, int prep);
    void root_stage(int stg);
    void run_stage(int i);              // prep early or deferred, the chain loop, evF or the separate extend-adds
    hipError_t end();                   // the top phase, zeroing for the next fit, the block inverses, the pivot exchange, timing read-back
};

// stream `to` waits for what stream `from` has been given so far
void hop(hipEvent_t e, hipStream_t from, hipStream_t to) { (void)hipEventRecord(e, from); (void)hipStreamWaitEvent(to, e, 0); }

// the Schur buffers of stage x are zeroed (lower-triangle tiles) when they come alive: at the start of the first stage
// that adds into them, on the update stream -- whatever used their place in the arena before was last touched there
void zero_block(NdState *s, int x, hipStream_t q) { launch_zero(s->fac.zero, s->fac.zero.l[(size_t)x][0], q); }

void ensure_events(NdState *s, int steps)
{
    for (auto *v : {&s->ev.evT, &s->ev.evI, &s->ev.evW})
        while ((int)v->size() < steps) v->push_back(nd_event(s));
}

void FactorRun::begin()
{
    NdTree &t = s->t;
    if (timing) {
        if (!s->ev.f0) { s->ev.f0 = nd_event(s, true); s->ev.f1 = nd_event(s, true); }
        (void)hipEventRecord(s->ev.f0, st);
    }
    if (s->used && s->ev.evDone) (void)hipStreamWaitEvent(st, s->ev.evDone, 0);
    if (s->zlast_valid) (void)hipStreamWaitEvent(st, s->ev.evZlast, 0);
    if (!s->s_clean && !s->sch.sc.st.empty())  // first fit, or the previous one was abandoned (otherwise the previous fit left them zeroed: evZlast)
        for (int x : s->sch.starts[0]) zero_block(s, x, st);
    s->s_clean = false;
    if (s->queues) (void)hipMemsetAsync(s->queues, 0, sizeof(int) * ND_QSTRIDE * (size_t)s->nqueues, st);
    if (s->dist && s->sh.rank != 0)        // the fronts the subtrees' Schur complements are summed in: their entries of N come from rank 0 alone
        for (int id : t.by_depth[(size_t)(s->sh.dcut - 1)]) {
            const NdFront &f = t.fr[(size_t)id];
            (void)hipMemsetAsync(s->factor + s->poff[(size_t)id], 0, sizeof(double) * (size_t)(f.ld * f.wp), st);
        }
    (void)hipEventRecord(s->ev.ev0, st);
    for (hipStream_t q : {sP, sU})
        if (q != st) (void)hipStreamWaitEvent(q, s->ev.ev0, 0);
    if (sR) (void)hipStreamWaitEvent(sR, s->ev.ev0, 0);
}

// every rank has eliminated its subtrees: sum what they left in the fronts of depth dcut - 1 (panel and Schur buffer)
void FactorRun::dist_join()
{
    NdTree &t = s->t;
    joined = true;
    for (hipStream_t q : {sP, sU, sR})
        if (q) (void)hipStreamSynchronize(q);
    // (square Schur buffers: their lower-triangle tiles only, packed into a scratch image; the square buffer if that could
    //  not be had.  Buffers in the packed form are summed where they lie.)
    double *scratch = s->sh.join_scratch;
    long long scap = s->sh.join_scratch_doubles;
    if (!s->sch.sc.packed) {   // every rank must sum windows of the same size: the scratch image only if ALL ranks have the scratch for it
        const double mine_missing = scratch ? 0.0 : 1.0;
        double any_missing = 0.0;
        (void)hipMemcpyAsync(s->part + 1, &mine_missing, sizeof(double), hipMemcpyHostToDevice, st);
        if (plan_allreduce(p, s->part + 1, 1, st) != 0) comm_failed = true;
        (void)hipMemcpyAsync(&any_missing, s->part + 1, sizeof(double), hipMemcpyDeviceToHost, st);
        (void)hipStreamSynchronize(st);
        if (any_missing != 0.0) scap = 0;
    }
    for (int id : t.by_depth[(size_t)(s->sh.dcut - 1)]) {
        const NdFront &f = t.fr[(size_t)id];
        if (plan_allreduce(p, s->factor + s->poff[(size_t)id], f.ld * (long long)f.wp, st) != 0) comm_failed = true;
        if (f.hp == 0) continue;
        const int nt = f.hp / 64;
        const long long tiles = trapezoid_items(nt, nt);
        if (s->sch.sc.packed) {
            if (plan_allreduce(p, s_ptr(s, id), nd_schur_doubles(f, true), st) != 0) comm_failed = true;
        } else if (tiles * 4096 <= scap) {
            launch_tripack(true, s_ptr(s, id), f.lds, nt, scratch, st);
            if (plan_allreduce(p, scratch, tiles * 4096, st) != 0) comm_failed = true;
            launch_tripack(false, s_ptr(s, id), f.lds, nt, scratch, st);
        } else if (plan_allreduce(p, s_ptr(s, id), f.lds * (long long)f.hp, st) != 0)
            comm_failed = true;
    }
    (void)hipStreamSynchronize(st);
}

// The diagonal blocks of step k, behind the chain stream sC.  reserved: on the reserved CUs -- two event hops, chain -> reserved
// CUs -> chain; `after` != NULL: they were complete at that event already (the reserved CUs need not wait for the chain).
void FactorRun::potrf_step(const Launch &lp, int k, hipStream_t sC, bool reserved, hipEvent_t after)
{
    if (!reserved) { launch_potrf(s, s->fac.potrf, lp, sC, info_dev, minpiv_dev); return; }
    if (after) (void)hipStreamWaitEvent(sR, after, 0);
    else hop(s->ev.evR0, sC, sR);
    launch_potrf(s, s->fac.potrf, lp, sR, info_dev, minpiv_dev);
    hop(s->ev.evI[(size_t)k], sR, sC);
}

// What comes alive with stage i: the Schur buffers are zeroed, the panels written (zeros + entries), on the update
// stream.  2.6 .. 3.5 GB of stores per stage at 64^3: beside the stage's FIRST diagonal blocks they made those 0.93 ms
// instead of 0.3 -- so they are launched behind the first block step of the chain (beside its panel update), when the
// update stream has nothing to do before that anyway (round 5)
void FactorRun::stage_prep(int i)
{
    for (int x : s->sch.starts[(size_t)i]) zero_block(s, x, sU);
    if (s->sch.staged_init && !s->dist)
        for (int x : s->sch.istarts[(size_t)i]) {
            launch_init(s, p->g, p->nst, s->fac.init.l[(size_t)x][0], sU);
            if (s->sch.sc.st[(size_t)x].dep < 0 && sU != sP) (void)hipEventRecord(s->ev.evP[(size_t)x], sU);
        }
}

// one block step of a stage's chain: potrf (on the reserved CUs when pinned) -> panel solve -> panel update, on the
// chain stream; the Schur passes that become ready go to the update stream
// (pin_potrf: the diagonal blocks go to the reserved CUs -- only once a Schur pass of the stage is running beside the chain:
//  before the first one the chip is idle, and 16 blocks on 8 reserved CUs are two rounds of 140 us where one would do)
// prep >= 0: the deferred stage_prep of that stage is launched on the update stream behind this step's panel solve
void FactorRun::chain_step(int stg, int k, bool pinned, bool pin_potrf, int prep)
{
    FactorTables &F = s->fac;
    const size_t S = (size_t)stg, K = (size_t)k;
    hipStream_t sC = sP;
    const Launch &ls = F.schur.l[S][K], &lf0 = F.fin[0].l[S][K], &lf1 = F.fin[1].l[S][K];
    const bool ahead = pinned && k > 0 && la_evt == k - 1;    // these diagonal blocks were updated before the rest of step k - 1
    potrf_step(F.potrf.l[S][K], k, sC, pinned && (pin_potrf || ahead), ahead ? s->ev.evW[(size_t)(k - 1)] : nullptr);
    launch_trsm(F.trsm, F.trsm.l[S][K], sC);
    if (prep >= 0) {
        hop(s->ev.evU, sC, sU);
        stage_prep(prep);
    }
    if ((ls.count || lf0.count || lf1.count) && sU != sC) hop(s->ev.evT[K], sC, sU);
    syrk(F.upd, F.upd.l[S][K], sC, false, pinned);
    if (s->sch.chain_la[S] && F.updr.l[S][K].count) {      // the rest of the in-group update, behind the next diagonal block
        if (pinned) {
            (void)hipEventRecord(s->ev.evW[K], sC);
            la_evt = k;
        }
        syrk(F.updr, F.updr.l[S][K], sC, false, pinned);
    }
    syrk(F.updo, F.updo.l[S][K], sC, false, pinned);     // the group's outer panel pass
    syrk(F.schur, ls, sU, true, pinned);
    syrk(F.fin[0], lf0, sU, true, pinned);      // final passes, fused with the extend-add:
    syrk(F.fin[1], lf1, sU, true, pinned);      // children of slot 0, then of slot 1
}

// the root: no Schur buffer to hide its chain behind, hence the look-ahead split
void FactorRun::root_stage(int stg)
{
    FactorTables &F = s->fac;
    const size_t S = (size_t)stg;
    const int steps = (int)F.potrf.l[S].size();
    ensure_events(s, steps);
    const bool pinned = sR != nullptr && s->nres > 0 && steps > 0 && (int)F.potrf.l[S][0].grid <= pin_rounds * s->nres;
    const bool la = s->sch.lookahead[S] != 0, la2 = s->sch.lookahead[S] == 2;
    for (int k = 0; k < steps; ++k) {
        if (!la) { chain_step(stg, k, pinned, true, -1); continue; }
        const size_t K = (size_t)k;
        const Launch &ltb = F.trsmb.l[S][K], &lur = F.updr.l[S][K];
        potrf_step(F.potrf.l[S][K], k, sP, pinned, nullptr);
        if (ltb.count) {            // the panel rows beyond the next diagonal block are solved beside the chain
            if (sU != sP) {
                if (!pinned) (void)hipEventRecord(s->ev.evI[K], sP);
                (void)hipStreamWaitEvent(sU, s->ev.evI[K], 0);
            }
            launch_trsm(F.trsmb, ltb, sU);
        }
        // everything of step k - 1 that is not the next diagonal block ran beside the chain; the panel rows this step
        // solves and the block it updates were last written there.  (la2: block column k was completed on the chain by step
        // k - 1 -- which waited for the trailing pass of step k - 2 --, so the whole panel is solved here, beside the trailing
        // pass of step k - 1; only the update of block column k + 1 below has to wait for that pass)
        if (!la2 && k > 0 && sU != sP) (void)hipStreamWaitEvent(sP, s->ev.evW[K - 1], 0);
        launch_trsm(F.trsm, F.trsm.l[S][K], sP);
        if (lur.count && sU != sP) hop(s->ev.evT[K], sP, sU);
        if (la2 && k > 0 && sU != sP) (void)hipStreamWaitEvent(sP, s->ev.evW[K - 1], 0);
        syrk(F.upd, F.upd.l[S][K], sP, false, pinned);
        syrk(F.updr, lur, sU, false, pinned);
        if (sU != sP) (void)hipEventRecord(s->ev.evW[K], sU);
    }
    if (sU != sP) hop(s->ev.evU, sU, sP);
}

// Stage i of the schedule (children before parents).  A rank of a one-process multi-GPU fit eliminates its subtrees here
// and the fronts above them in the top phase, together with the other ranks (ndtop.hip).
void FactorRun::run_stage(int i)
{
    FactorTables &F = s->fac;
    const NdStage &S = s->sch.sc.st[(size_t)i];
    if (s->dist && !joined && S.depth <= s->sh.dcut - 1) dist_join();
    auto passes = [&](int k) { return F.schur.l[(size_t)i][(size_t)k].count || F.fin[0].l[(size_t)i][(size_t)k].count || F.fin[1].l[(size_t)i][(size_t)k].count; };
    const int steps = (int)F.potrf.l[(size_t)i].size();
    const bool prep_late = splpak::opt_get("SPLPAK_ND_PREP_EARLY") == nullptr;
    const bool defer = prep_late && i > 0 && i != s->sch.root_stage && sU != sP && steps >= 2 && !passes(0);      // (see stage_prep)
    if (i > 0) {
        if (!defer) stage_prep(i);
        if (s->sch.staged_init && !s->dist && S.dep < 0 && sU != sP) (void)hipStreamWaitEvent(sP, s->ev.evP[(size_t)i], 0);   // (its panels were written one stage ago)
    }
    // the fronts' children have added their Schur complements (their last passes run on the update stream)
    if (s->sch.fused && S.dep >= 0 && sU != sP) (void)hipStreamWaitEvent(sP, s->ev.evF[(size_t)S.dep], 0);
    la_evt = -1;
    if (i == s->sch.root_stage) { root_stage(i); return; }
    ensure_events(s, steps);
    // (a stage with look-ahead inside its groups uses the reserved CUs whatever the number of rounds: its diagonal blocks are
    //  factored beside the rest of the previous step's update)
    const bool pinned = sR != nullptr && s->nres > 0 && steps > 0 && ((int)F.potrf.l[(size_t)i][0].grid <= pin_rounds * s->nres || s->sch.chain_la[(size_t)i]);
    const bool unpin_first = splpak::opt_get("SPLPAK_ND_PIN_FIRST") == nullptr;
    bool pass_running = !unpin_first;
    for (int k = 0; k < steps; ++k) {
        chain_step(i, k, pinned, pass_running, k == 0 && defer ? i : -1);        // (the deferred prep: behind the first diagonal blocks and panel solve of the chain)
        if (passes(k)) pass_running = true;
    }
    if (s->sch.fused) (void)hipEventRecord(s->ev.evF[(size_t)i], sU);     // (stream order: the stage's last passes are behind it)
    else {                  // separate extend-add launches: the stage's passes, then slot 0, then slot 1
        if (sU != sP) hop(s->ev.evU, sU, sP);
        for (int sl = 0; sl < 2; ++sl) launch_add(F.add, F.add.l[(size_t)i][(size_t)sl], sP);
        (void)hipEventRecord(s->ev.evE[(size_t)i], sP);       // (the arena blocks of this stage are reused on the update stream)
        if (sU != sP) (void)hipStreamWaitEvent(sU, s->ev.evE[(size_t)i], 0);
    }
}

hipError_t FactorRun::end()
{
    if (s->dist && !joined && s->sh.dcut >= 1) dist_join();
    hipError_t top_err = hipSuccess;
    if (s->mdist) {
        ++s->top.fgen;
        top_err = nd_top_factor(s, st, info_dev, minpiv_dev, stats, timing);
    }
    // what is alive when the first stage starts is zeroed for the NEXT fit here, beside the tail of this one (waited for
    // through evZlast; multi-GPU: after the top phase, the other ranks have pulled the subtree roots' Schur complements)
    if (top_err == hipSuccess && !s->sch.sc.st.empty())
        for (int x : s->sch.starts[0]) zero_block(s, x, sU);
    // inverses of all diagonal blocks (the solves' operands)
    launch_trinv(s->fac.trinv.dev, s->fac.ntrinv, sP);
    (void)hipEventRecord(s->ev.evJ, sP);
    if (sP != st) (void)hipStreamWaitEvent(st, s->ev.evJ, 0);
    if (s->mdist && top_err == hipSuccess) top_err = nd_top_pivots(s, st, info_dev, minpiv_dev);
    if (s->dist) {      // (a failed pivot poisons the fronts above it with NaN, so every rank fails anyway; this makes it explicit)
        launch_flag(info_dev, s->part, st);
        if (plan_allreduce(p, s->part, 1, st) != 0) comm_failed = true;
        launch_unflag(info_dev, s->part, st);
    }
    if (sU != st) {                                   // (the zero launches for the next fit may still be running: it waits for them)
        (void)hipEventRecord(s->ev.evZlast, sU);
        s->zlast_valid = true;
    }
    s->s_clean = true;
    (void)hipEventRecord(s->ev.evDone, st);
    s->used = true;
    hipError_t err = hipGetLastError();
    if (timing) {
        (void)hipEventRecord(s->ev.f1, st);
        (void)hipEventSynchronize(s->ev.f1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, s->ev.f0, s->ev.f1);
        stats->factor_ms = ms;
        for (size_t i = 0; i < (size_t)stats->syrk_launches; ++i) {
            if (hipEventElapsedTime(&ms, s->ev.evA[i], s->ev.evB[i]) == hipSuccess) stats->syrk_ms += ms;
            else (void)hipGetLastError();
        }
    }
    if (err != hipSuccess || top_err != hipSuccess) s->s_clean = false;
    if (comm_failed) return hipErrorUnknown;
    return top_err != hipSuccess ? top_err : err;
}

}  // namespace

hipError_t nd_factor(splpak_plan *p, int *info_dev, double *minpiv_dev, hipStream_t st, void *user)
{
    NdState *s = static_cast<NdState *>(user);
    const bool timing = p->stats.enabled;
    p->stats = CholStats{};
    p->stats.enabled = timing;
    const bool serial = splpak::opt_get("SPLPAK_NO_LOOKAHEAD") != nullptr;
    FactorRun r{p, s, st, s->str.sP, s->str.sU, s->str.sR, info_dev, minpiv_dev, &p->stats, timing};
    if (serial) r.sP = r.sU = st;
    if (serial || splpak::opt_get("SPLPAK_NO_PANEL_CU")) r.sR = nullptr;
    // (round 5: 1 -- two rounds of 140 us on the reserved CUs lose against one round on the whole chip beside the pass:
    //  219.3 against 220.7 ms at 64^3)
    r.pin_rounds = splpak::opt_get("SPLPAK_ND_PIN_ROUNDS") ? atoi(splpak::opt_get("SPLPAK_ND_PIN_ROUNDS")) : 1;
    r.begin();
    for (int i = 0; i < (int)s->sch.sc.st.size(); ++i) r.run_stage(i);
    return r.end();
}

hipError_t nd_solve(splpak_plan *p, double *x, double *tmp, hipStream_t st, void *user)
{
    (void)tmp;
    NdState *s = static_cast<NdState *>(user);
    NdTree &t = s->t;
    SolveTables &T = s->sol;
    const long long n = t.vec_doubles;
    launch_gather(n, s->rowsrc, x, s->V, st);
    bool comm_failed = false;
    if (s->dist && s->sh.rank != 0)        // the right-hand side of the fronts the subtrees report into comes from rank 0 alone
        for (int id : t.by_depth[(size_t)(s->sh.dcut - 1)]) {
            const NdFront &f = t.fr[(size_t)id];
            (void)hipMemsetAsync(s->V + f.vofs, 0, sizeof(double) * (size_t)f.fp, st);
        }
    // (one-process multi-GPU fit: the subtrees here, the fronts above them step by step with the other ranks -- ndtop.hip)
    const int dlow = s->mdist ? s->top.pt.dcut : 0;
    if (s->mdist) ++s->top.sgen;
    // forward, bottom-up
    for (int d = t.maxdepth; d >= dlow; --d) {
        if (d < t.maxdepth)
            for (int sl = 0; sl < 2; ++sl) launch_map(T.map, T.map.l[(size_t)(d + 1)][(size_t)sl], false, st);
        if (s->dist && d == s->sh.dcut - 1)        // the subtrees' updates of these fronts' vectors, summed over the ranks
            for (int id : t.by_depth[(size_t)d]) {
                const NdFront &f = t.fr[(size_t)id];
                if (plan_allreduce(p, s->V + f.vofs, f.fp, st) != 0) comm_failed = true;
            }
        const int steps = (int)T.mv.l[(size_t)d].size();
        for (int k = 0; k < steps; ++k) {
            launch_mv(T.mv, T.mv.l[(size_t)d][(size_t)k], st);
            launch_fwd(T.fwd, T.fwd.l[(size_t)d][(size_t)k], st);
        }
    }
    if (s->mdist) {
        hipError_t e = nd_top_forward(s, st);
        if (e == hipSuccess) e = nd_top_backward(s, st);
        if (e != hipSuccess) return e;
    }
    // backward, top-down
    for (int d = dlow; d <= t.maxdepth; ++d) {
        if (d >= 1 && d > dlow) launch_map(T.map, T.map.l[(size_t)d][2], true, st);
        const int steps = (int)T.mv.l[(size_t)d].size();
        for (int k = steps - 1; k >= 0; --k) {
            launch_dot(T.dot, T.dot.l[(size_t)d][(size_t)k], st);
            launch_bwd(T.bwd, T.bwd.l[(size_t)d][(size_t)k], st);
        }
    }
    if (s->dist || s->mdist) {
        // every rank reports the variables of its own subtrees (rank 0 also those of the top of the tree); the sum is the solution
        (void)hipMemsetAsync(x, 0, sizeof(double) * (size_t)p->g.ncol, st);
        launch_scatter(n, s->sh.rowsrc_out, s->V, x, st);
        if (plan_allreduce(p, x, p->g.ncol, st) != 0) comm_failed = true;
    } else
        launch_scatter(n, s->rowsrc, s->V, x, st);
    if (comm_failed) return hipErrorUnknown;
    return hipGetLastError();
}

// The batch copies of V, Y and part for nd_solve_many, allocated at the first call (a batched refit): true when the plan's solver
// is the single-GPU nested dissection and they exist.  An allocation that fails is not an error of the caller's: it is tried
// once, the error is cleared, and the plan solves one right-hand side at a time from then on.
bool nd_batch_ready(splpak_plan *p)
{
    NdState *s = p && p->fn_code == 4 && p->solve_fn == nd_solve ? static_cast<NdState *>(p->fn_user) : nullptr;
    if (!s || s->dist || s->mdist) return false;
    if (s->bV || s->batch_tried) return s->bV != nullptr;
    s->batch_tried = true;
    const size_t vec = (size_t)s->t.vec_doubles, bytes = sizeof(double) * (size_t)ND_BATCH_MAX * (2 * vec + (size_t)s->part_cap);
    void *q = nullptr;
    if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
    s->owned.push_back(q);
    s->owned_bytes += bytes;
    s->bV = static_cast<double *>(q);
    s->bY = s->bV + (size_t)ND_BATCH_MAX * vec;
    s->bpart = s->bY + (size_t)ND_BATCH_MAX * vec;
    return true;
}

// x[r] <- N^-1 x[r] for R right-hand sides in ONE sweep of the tree: the depth loop of nd_solve with one launch where it has one,
// every launch over the R copies of the vectors (slot r = x[r], whatever field that is).  Each x[r] receives the bits nd_solve
// gives it.  R = 1 is nd_solve.  Single-GPU plans only, after nd_batch_ready.
hipError_t nd_solve_many(splpak_plan *p, int R, double *const *x, hipStream_t st)
{
    NdState *s = static_cast<NdState *>(p->fn_user);
    if (R == 1) return nd_solve(p, x[0], nullptr, st, s);
    if (R < 2 || R > ND_BATCH_MAX || !s->bV || s->dist || s->mdist) return hipErrorInvalidValue;
    NdTree &t = s->t;
    SolveTables &T = s->sol;
    const long long n = t.vec_doubles;
    const BatchVec w{s->bV, s->bY, s->bpart, n, s->part_cap, s->V, s->Y, s->part};
    BatchPtrs b{};
    for (int r = 0; r < R; ++r) b.p[r] = x[r];
    launch_gather_many(n, s->rowsrc, b, w, R, st);
    // forward, bottom-up
    for (int d = t.maxdepth; d >= 0; --d) {
        if (d < t.maxdepth)
            for (int sl = 0; sl < 2; ++sl) launch_map_many(T.map, T.map.l[(size_t)(d + 1)][(size_t)sl], false, w, R, st);
        const int steps = (int)T.mv.l[(size_t)d].size();
        for (int k = 0; k < steps; ++k) {
            launch_mv_many(T.mv, T.mv.l[(size_t)d][(size_t)k], w, R, st);
            launch_fwd_many(T.fwd, T.fwd.l[(size_t)d][(size_t)k], w, R, st);
        }
    }
    // backward, top-down
    for (int d = 0; d <= t.maxdepth; ++d) {
        if (d >= 1) launch_map_many(T.map, T.map.l[(size_t)d][2], true, w, R, st);
        const int steps = (int)T.mv.l[(size_t)d].size();
        for (int k = steps - 1; k >= 0; --k) {
            launch_dot_many(T.dot, T.dot.l[(size_t)d][(size_t)k], w, R, st);
            launch_bwd_many(T.bwd, T.bwd.l[(size_t)d][(size_t)k], w, R, st);
        }
    }
    launch_scatter_many(n, s->rowsrc, b, w, R, st);
    return hipGetLastError();
}

}  // namespace nd
}  // namespace splpak
