// Job tables of the nested-dissection factorisation (ndstate.hpp), built once per plan on the host (again when a sharded fit's
// ranks become known): the order of the jobs and of their items defines the order of every sum, so it is part of the result.
#include "ndstate.hpp"
#include <algorithm>

namespace splpak {
namespace nd {

namespace {

// The jobs of front `id` in block step k of stage `stg`, into the open launches of the factor tables (with the flops of the
// outer panel pass, the Schur pass and the fused final passes).  two_level: block k updates only the columns of its own group
// of schur_kb blocks, the columns beyond receive one outer pass per group.
void front_step_jobs(NdState *s, int stg, int id, int k, bool two_level)
{
    NdTree &t = s->t;
    FactorTables &F = s->fac;
    const NdFront &f = t.fr[(size_t)id];
    const bool la = s->sch.lookahead[(size_t)stg] != 0, la2 = s->sch.lookahead[(size_t)stg] == 2, cla = s->sch.chain_la[(size_t)stg] != 0;
    const int schur_kb = s->sch.schur_kb;
    // groups of panel blocks that share a Schur pass (and the outer panel pass): schur_kb blocks each, the same boundaries for every
    // front of a stage.  (Round 5 tried a RAMP of smaller first groups -- 2, then 4 blocks -- so that the first pass of a stage would
    // not wait for a chain of four block steps: -1.2 ms of 225 at 64^3, paid for with slower K = 512 passes; it made the group
    // boundaries differ between the fronts of one stage, which the look-ahead inside the groups did not allow for -- a front whose
    // group ended at step k - 1 could have its block k factored while the outer pass was still writing it (round-5 advice).  The
    // switch is gone.)
    const int g0 = (k / schur_kb) * schur_kb, gend = std::min(g0 + schur_kb, f.nsteps) - 1;
    double *panel = s->factor + s->poff[(size_t)id];
    double *diag = panel + (long long)k * 256 + (long long)k * 256 * f.ld;
    double *below = diag + 256;
    const int nrows = f.fp - (k + 1) * 256;
    double *i16 = s->inv16 + (long long)(s->lblk[(size_t)id] + k) * 4096;
    const int ncols = std::max(1, std::min(256, f.w - k * 256));     // real columns of block k (w > 256 (nsteps - 1) by construction)
    F.potrf.push(PotrfJob{diag, i16, f.ld, f.own0 + k * 256, ncols});
    const int nc = (f.wp - (k + 1) * 256) / 64, nr = nrows / 64;
    if (nrows > 0) {
        // with look-ahead (the root) only the rows of the NEXT diagonal block are solved on the chain, the rest beside it
        const int ntop = (la && !la2 && nc > 0) ? std::min(nrows, 256) : nrows;
        F.trsm.push(TrsmJob{diag, below, i16, f.ld, ntop, 0, (ncols + 15) / 16, 0}, ntop / 16);
        if (nrows > ntop) F.trsmb.push(TrsmJob{diag, below + ntop, i16, f.ld, nrows - ntop, 0, (ncols + 15) / 16, 0}, (nrows - ntop) / 16);
    }
    if (nc > 0) {
        // panel columns right of block k: rows and columns relative to row (k+1)*256.  With look-ahead only the next
        // DIAGONAL BLOCK (4 x 4 tiles) is updated on the chain; the rows below it in that block column (a rectangle
        // of tiles) and the columns beyond (a trapezoid) are one launch beside the chain
        const SyrkJob proto{below, below + (long long)256 * f.ld, f.ld, f.ld, 0, 0, 0, 1, 64, 0, nullptr, nullptr, nullptr, 0, 0, 0, 0};
        auto trapezoid = [&](JobTable<SyrkJob> &tab, int c, int r) {
            SyrkJob a = proto;
            a.nc = c; a.nr = r;
            tab.push(a, trapezoid_items(c, r));
        };
        // the next block column split in three: its diagonal block | the rows below it (a rectangle) | the nin - 4 columns beyond
        auto split = [&](JobTable<SyrkJob> &rect_tab, int nin) {
            const int n4 = std::min(nin, 4);
            trapezoid(F.upd, n4, std::min(nr, 4));
            if (nr > 4) {
                SyrkJob r = proto;
                r.nc = n4; r.nr = nr; r.zinit = -4;
                rect_tab.push(r, (long long)n4 * (nr - 4));
            }
            if (nin > 4) {
                SyrkJob t2 = proto;
                t2.P = below + 256;
                t2.C = below + (long long)256 * f.ld + 256 + (long long)256 * f.ld;
                t2.nc = nin - 4; t2.nr = nr - 4;
                F.updr.push(t2, trapezoid_items(nin - 4, nr - 4));
            }
        };
        if (!la && two_level) {
            // TWO-LEVEL blocking of the panel (round 3): block k updates only the columns of its own group of
            // schur_kb blocks here (K = 256); the columns beyond the group receive all of the group's blocks in ONE
            // pass of K = 256 kb when its last block is solved -- the same sums in the same order (the accumulators
            // start as the tile and subtract block after block), a quarter of the read-modify-writes, and launches
            // that run at the rate of the Schur passes instead of 34 TFLOP/s (rocprofv3, 64^3)
            const int nc_in = std::min(nc, (gend - k) * 4);
            // (look-ahead inside the group: the next diagonal block first, the rest of the group's columns behind it)
            if (nc_in > 0 && cla) split(F.updr, nc_in);
            else if (nc_in > 0) trapezoid(F.upd, nc_in, nr);
            if (k == gend) {             // nc > 0: columns remain beyond the group
                SyrkJob o = proto;
                o.P = panel + (long long)(k + 1) * 256 + (long long)g0 * 256 * f.ld;
                o.kb = k - g0 + 1;
                o.nc = nc; o.nr = nr;
                F.updo.push(o, trapezoid_items(nc, nr));
                F.updo.cur.flop += 2.0 * 64 * 64 * 256.0 * o.kb * (double)trapezoid_items(nc, nr);
            }
        } else if (!la)
            trapezoid(F.upd, nc, nr);
        else                             // the rows below the next diagonal block: on the chain too (la2), or beside it
            split(la2 ? F.upd : F.updr, nc);
    }
    // Schur buffer: one pass per group of up to schur_kb panel blocks, launched when the group's last block is solved
    const int ns = f.hp / 64;
    if (ns > 0 && k == gend) {
        const int kb = k - g0 + 1;
        // (the last block of a front holds ncols real columns: the k-loop stops behind them, in chunks of 16 columns)
        const int ksl = (k == f.nsteps - 1) ? 4 * ((ncols + 15) / 16) : 64;
        // (the ns diagonal items skip the 6 of their 16 tiles above the diagonal)
        const double jitems = (double)trapezoid_items(ns, ns) - (s->full_diag ? 0.0 : 0.375 * ns);
        const double jflop = 2.0 * 64 * 64 * (256.0 * (kb - 1) + 4.0 * ksl) * jitems;
        // (a subtree root of a multi-GPU fit keeps its Schur complement: the owners of the parent's block columns pull it)
        const bool boundary = s->mdist && f.depth == s->top.pt.dcut;
        if (s->sch.fused && k == f.nsteps - 1 && f.parent >= 0 && !boundary) {
            // the front's last pass carries its Schur complement into the parent itself
            const NdFront &pf = t.fr[(size_t)f.parent];
            const int leaf = s->sch.needs[(size_t)id] ? 0 : 1;       // no children, one pass: the buffer is never materialised
            F.fin[f.slot].push(SyrkJob{panel + f.wp + (long long)g0 * 256 * f.ld, s_ptr(s, id), f.ld, s_ld(s, id), ns, ns, 0, kb, ksl, leaf, s->pmap + f.bofs,
                                       s->factor + s->poff[(size_t)f.parent], s_ptr(s, f.parent), pf.ld, s_ld(s, f.parent), pf.wp, f.h},
                               trapezoid_items(ns, ns));
            F.fin[f.slot].cur.flop += jflop;
        } else {
            F.schur.push(SyrkJob{panel + f.wp + (long long)g0 * 256 * f.ld, s_ptr(s, id), f.ld, s_ld(s, id), ns, ns, 0, kb, ksl, 0, nullptr, nullptr, nullptr, 0, 0, 0, 0},
                         trapezoid_items(ns, ns));
            F.schur.cur.flop += jflop;
        }
    }
}

// the launches a stage has one of: zeroing of its Schur buffers, its panels, its separate extend-adds
bool stage_jobs(NdState *s, int stg)
{
    NdTree &t = s->t;
    FactorTables &F = s->fac;
    const std::vector<int> &ids = s->sch.sc.st[(size_t)stg].ids;
    // lower-triangle tiles of the stage's Schur buffers
    F.zero.open();
    for (int id : ids) {
        const NdFront &f = t.fr[(size_t)id];
        if (f.hp == 0 || !s->sch.needs[(size_t)id]) continue;       // (a leaf's buffer is never materialised: fused last pass)
        const int nt = f.hp / 64;
        F.zero.push(ZeroJob{s_ptr(s, id), s_ld(s, id), nt, 0}, trapezoid_items(nt, nt));
    }
    if (!F.zero.close((size_t)stg, 0)) return false;
    // panel columns of the stage's fronts
    F.init.open();
    for (int id : ids)
        if (s->poff[(size_t)id] >= 0) F.init.push(InitJob{id, 0}, t.fr[(size_t)id].wp);
    if (!F.init.close((size_t)stg, 0)) return false;
    // separate extend-add launches (SPLPAK_ND_NO_FUSE): children of this stage -> their parents
    if (s->sch.sc.st[(size_t)stg].depth >= 1 && !s->sch.fused)
        for (int sl = 0; sl < 2; ++sl) {
            F.add.open();
            for (int id : ids) {
                const NdFront &f = t.fr[(size_t)id];
                if (f.slot != sl || f.h == 0) continue;
                const NdFront &p = t.fr[(size_t)f.parent];
                const int nt = f.hp / 64;
                F.add.push(AddJob{s_ptr(s, id), s->pmap + f.bofs, s->factor + s->poff[(size_t)f.parent], s_ptr(s, f.parent), s_ld(s, id), p.ld,
                                  s_ld(s, f.parent), f.h, nt, p.wp, 0},
                           trapezoid_items(nt, nt));
            }
            if (!F.add.close((size_t)stg, (size_t)sl)) return false;
        }
    return true;
}

// Job tables of the FACTORISATION: one set of launches per stage of the schedule and block step.
bool nd_build_factor_jobs(NdState *s)
{
    NdTree &t = s->t;
    FactorTables &F = s->fac;
    const int nstage = (int)s->sch.sc.st.size();
    JobTable<SyrkJob> *const syrk[] = {&F.upd, &F.updr, &F.updo, &F.schur, &F.fin[0], &F.fin[1]};
    s->sch.lookahead.assign((size_t)nstage, 0);
    s->sch.chain_la.assign((size_t)nstage, 0);
    for_each_table(F, [&](auto &tab) { tab.l.assign((size_t)nstage, {}); });
    const bool two_level = splpak::opt_get("SPLPAK_ND_NO_OUTER") == nullptr;
    // (Schur buffer passes: groups of up to schur_kb panel blocks (K = 1024: the C tiles are read and written once per
    // group; measured at 64^3: 257.6 ms per factorisation against 262.4 with K = 512 and 270.9 with K = 256; groups that
    // ramp up 1, 2, 4, 4, .. so that the first pass of a depth starts earlier made no difference))
    for (int stg = 0; stg < nstage; ++stg) {
        const std::vector<int> &ids = s->sch.sc.st[(size_t)stg].ids;
        int steps = 0;
        for (int id : ids) steps = std::max(steps, t.fr[(size_t)id].nsteps);
        bool any_schur = false;
        for (int id : ids) any_schur = any_schur || t.fr[(size_t)id].hp > 0;
        const bool la = !any_schur && steps >= 4 && !splpak::opt_get("SPLPAK_ND_NO_ROOT_LOOKAHEAD");
        // 2: the WHOLE next block column is updated on the chain (its diagonal block and the rows below it), so that the next
        // panel solve runs beside the trailing pass of this step instead of behind it (round 5); 1: only the next diagonal block
        // (round 4: the panel solve of every step, 50 us, waited for the trailing pass and was waited for by the next one)
        const bool la2 = la && !(splpak::opt_get("SPLPAK_ND_ROOT_LA") && atoi(splpak::opt_get("SPLPAK_ND_ROOT_LA")) == 1);
        const int cla_blocks = splpak::opt_get("SPLPAK_ND_CHAIN_LA") ? atoi(splpak::opt_get("SPLPAK_ND_CHAIN_LA")) : 8;   // (64^3: 219.2 ms with 8, 219.9 with 16, 221.0 with 64 or 0)
        const bool cla = !la && two_level && steps >= 2 && (int)ids.size() <= cla_blocks && !s->mdist;
        s->sch.chain_la[(size_t)stg] = cla ? 1 : 0;
        s->sch.lookahead[(size_t)stg] = la ? (la2 ? 2 : 1) : 0;
        for (int k = 0; k < steps; ++k) {
            F.potrf.open(); F.trsm.open(); F.trsmb.open();
            for (auto *tab : syrk) tab->open();
            for (int id : ids)
                if (k < t.fr[(size_t)id].nsteps) front_step_jobs(s, stg, id, k, two_level);
            const size_t S = (size_t)stg, K = (size_t)k;
            if (!F.potrf.close(S, K) || !F.trsm.close(S, K) || !F.trsmb.close(S, K)) return false;
            for (auto *tab : syrk)
                if (!tab->close(S, K)) return false;
            F.upd.l[S][K].flop = 2.0 * 64 * 64 * 256 * (double)F.upd.l[S][K].grid;
            F.updr.l[S][K].flop = 2.0 * 64 * 64 * 256 * (double)F.updr.l[S][K].grid;
        }
        if (!stage_jobs(s, stg)) return false;
    }
    for (size_t id = 0; id < t.fr.size(); ++id) {
        const NdFront &f = t.fr[id];
        if (!s->mine.empty() && !s->mine[id]) continue;
        for (int k = 0; k < f.nsteps; ++k) {
            const double *diag = s->factor + s->poff[id] + (long long)k * 256 + (long long)k * 256 * f.ld;
            const long long lb = s->lblk[id] + k;
            F.trinv.host.push_back(TrinvJob{diag, s->inv16 + lb * 4096, s->dinv + lb * 65536, s->dinvt + lb * 65536, f.ld});
        }
    }
    F.ntrinv = (int)F.trinv.host.size();
    return true;
}

// Real columns of block k of a front of own width w, as the solves' sweeps take them (FwdJob / DotJob, ndstate.hpp).
// A/B switch SPLPAK_ND_SOLVE_PADDED: all 256, the identity padding of the last block included, as before -- the same bits.
static int solve_block_cols(int w, int k)
{
    if (splpak::opt_get("SPLPAK_ND_SOLVE_PADDED")) return 256;
    return std::max(1, std::min(256, w - k * 256));
}

// Job tables of the SOLVES: per tree depth (all fronts of the depth, whatever their pipeline) and block step.
bool nd_build_solve_jobs(NdState *s)
{
    NdTree &t = s->t;
    SolveTables &T = s->sol;
    const int nd = t.maxdepth + 1;
    for_each_table(T, [&](auto &tab) { tab.l.assign((size_t)nd, {}); });
    long long part_max = 0;
    for (int d = 0; d < nd; ++d) {
        std::vector<int> ids;
        for (int id : t.by_depth[(size_t)d])
            if (s->mine.empty() || s->mine[(size_t)id]) ids.push_back(id);
        int steps = 0;
        for (int id : ids) steps = std::max(steps, t.fr[(size_t)id].nsteps);
        for (int k = 0; k < steps; ++k) {
            T.mv.open(); T.fwd.open(); T.dot.open(); T.bwd.open();
            long long partofs = 0;
            for (int id : ids) {
                const NdFront &f = t.fr[(size_t)id];
                if (k >= f.nsteps) continue;
                const double *below = s->factor + s->poff[(size_t)id] + (long long)k * 256 + (long long)k * 256 * f.ld + 256;
                const int nrows = f.fp - (k + 1) * 256;
                const int ncols = solve_block_cols(f.w, k);
                double *Vf = s->V + f.vofs, *Yf = s->Y + f.vofs;
                T.mv.push(MvJob{s->dinv + (long long)(s->lblk[(size_t)id] + k) * 65536, Vf + k * 256, Yf + k * 256});
                int nsplit = 0;
                double *partp = s->part + partofs;
                if (nrows > 0) {
                    T.fwd.push(FwdJob{below, Yf + k * 256, Vf + (k + 1) * 256, f.ld, nrows, ncols, 0}, nrows / 64);
                    nsplit = (nrows + DOT_RPS - 1) / DOT_RPS;
                    T.dot.push(DotJob{below, Vf + (k + 1) * 256, partp, f.ld, nrows, nsplit, DOT_RPS, ncols, 0}, 16 * nsplit);
                    partofs += (long long)nsplit * 256;
                }
                T.bwd.push(BwdJob{s->dinvt + (long long)(s->lblk[(size_t)id] + k) * 65536, Yf + k * 256, partp, Vf + k * 256, nsplit, 0});
            }
            part_max = std::max(part_max, partofs);
            const size_t D = (size_t)d, K = (size_t)k;
            if (!T.mv.close(D, K) || !T.fwd.close(D, K) || !T.dot.close(D, K) || !T.bwd.close(D, K)) return false;
        }
        // children at depth d <-> parents at depth d - 1 (border values of the sweeps)
        if (d >= 1) {
            for (int sl = 0; sl < 2; ++sl) {
                T.map.open();
                for (int id : ids) {
                    const NdFront &f = t.fr[(size_t)id];
                    if (f.slot != sl || f.h == 0) continue;
                    const NdFront &p = t.fr[(size_t)f.parent];
                    T.map.push(MapJob{s->V + f.vofs + f.wp, s->V + p.vofs, s->pmap + f.bofs, f.h, 0});
                }
                if (!T.map.close((size_t)d, (size_t)sl)) return false;
            }
            // backward: both slots at once = the two consecutive runs of map jobs
            const int first = T.map.l[(size_t)d][0].first, both = T.map.l[(size_t)d][0].count + T.map.l[(size_t)d][1].count;
            T.map.l[(size_t)d].push_back(Launch{first, both, (unsigned)both, 0});
        }
    }
    return part_max <= s->part_cap;
}

}  // namespace

// for the fronts in s->mine; SPLPAK_E_UNSUPPORTED: a launch too large (set_error has the message)
int nd_make_jobs(NdState *s)
{
    auto each = [&](auto &&f) { for_each_table(s->fac, f); for_each_table(s->sol, f); };
    each([](auto &tab) { tab.host.clear(); });
    if (!nd_build_factor_jobs(s) || !nd_build_solve_jobs(s)) return SPLPAK_E_UNSUPPORTED;
    bool ok = true;
    each([&](auto &tab) { nd_free_dev(s, &tab.dev); ok = ok && nd_upload(s, &tab.dev, tab.host); });      // (free: the superseded device tables)
    return ok ? 0 : SPLPAK_E_NOMEM;
}

// Job tables of the top phase of ONE rank.  Needs every rank's storage (the peers' addresses go into the pull jobs): called by
// nd_group_finalize after all plans of the group exist.  (No sentinels here: one job each, or a count the search never leaves.)
bool nd_build_top_jobs(NdState *s)
{
    NdGroup *g = s->grp;
    NdTree &t = s->t;
    Top &T = s->top;
    const NdPartition &pt = T.pt;
    const int me = s->mrank, nseq = pt.nseq;
    const size_t ntop = pt.top.size();
    for_each_table(T, [&](auto &tab) { tab.l.assign(1, std::vector<Launch>((size_t)nseq + 1)); });
    T.rslot.assign((size_t)nseq + 1, -1);
    for (int sl = 0; sl < 2; ++sl) {
        T.l_pull[sl].assign(ntop, Launch());
        T.l_mapf[sl].assign(ntop, -1);
    }
    T.l_mapb.assign(ntop, -1);
    bool ok = true;
    auto single = [&](auto &tab, size_t sq, auto job, long long n = 1) {      // a launch of one job
        tab.open();
        tab.push(job, n);
        ok = tab.close(0, sq, false) && ok;
    };
    int ncopied = 0;
    for (size_t ti = 0; ti < ntop; ++ti) {
        const int id = pt.top[ti];
        const NdFront &f = t.fr[(size_t)id];
        const int nb = top_nblocks(f);
        double *Vf = s->V + f.vofs, *Yf = s->Y + f.vofs;
        // ---- extend-add: the child's columns that map into my block columns
        for (int sl = 0; sl < 2; ++sl) {
            const int cid = f.child[sl];
            if (cid < 0) continue;
            const NdFront &c = t.fr[(size_t)cid];
            T.pull.open();
            const int *pm = t.pmap.data() + c.bofs;
            for (int J = 0; J < nb; ++J) {
                const TopColDev &tc = top_col(s, ti, J);
                if (tc.off < 0) continue;
                const int lo = J * 256, hi = lo + top_block_cols(f, J);
                const int c0 = (int)(std::lower_bound(pm, pm + c.h, lo) - pm), c1 = (int)(std::lower_bound(pm, pm + c.h, hi) - pm);
                if (c1 <= c0) continue;
                auto push = [&](const double *src, long long lds, int a, int b) {
                    const int rbase = (a >> 6) << 6;
                    const PullJob j{src, lds, s->pmap + c.bofs, s->factor + tc.off, tc.ld, a, b, c.h, lo, 0, (c.h - rbase + 63) / 64, (b - a + 63) / 64, 0};
                    T.pull.push(j, (long long)j.ntr * j.ntc);
                };
                if (pt.owner[(size_t)cid] >= 0) {               // a subtree root: its Schur buffer, on its owner
                    NdState *q = static_cast<NdState *>(g->st[(size_t)pt.owner[(size_t)cid]]);
                    push(s_ptr(q, cid), c.lds, c0, c1);
                } else {                                        // a top front: its columns beyond wp, block column by block column
                    const size_t tci = (size_t)pt.top_index[(size_t)cid];
                    int a = c0;
                    while (a < c1) {
                        const int Jc = (c.wp + a) / 256;
                        const int bnd = std::min(c1, (Jc + 1) * 256 - c.wp);
                        NdState *q = static_cast<NdState *>(g->st[(size_t)top_owner(pt, Jc)]);
                        const TopColDev &sc = top_col(q, tci, Jc);
                        // element (border row r, border column cc) of the child = base[(wp + r - 256 Jc) + (wp + cc - 256 Jc) ld]
                        push(q->factor + (sc.off + (long long)(c.wp - Jc * 256) * (1 + sc.ld)), sc.ld, a, bnd);
                        a = bnd;
                    }
                }
            }
            if (!T.pull.close(T.l_pull[sl][ti], false)) return false;
            // forward sweep: the child's border updates arrive in the staging vector
            T.l_mapf[sl][ti] = (int)T.mapf.host.size();
            T.mapf.host.push_back(MapJob{T.stagev, Vf, s->pmap + c.bofs, c.h, 0});
        }
        if (f.parent >= 0) {                                    // backward sweep: border values from the parent's vector (staged)
            T.l_mapb[ti] = (int)T.mapb.host.size();
            T.mapb.host.push_back(MapJob{Vf + f.wp, T.stagev, s->pmap + f.bofs, f.h, 0});
        }
        // ---- block steps
        for (int k = 0; k < f.nsteps; ++k) {
            const size_t sq = (size_t)(pt.seq0[ti] + k);
            const int o = top_owner(pt, k);
            const long long ldk = top_block_ld(f, k);
            const double *P = nullptr;
            if (o == me) P = s->factor + top_col(s, ti, k).off + 256;
            else {
                const int ps = ncopied % 3;
                ++ncopied;
                T.rslot[sq] = ps;
                P = T.pbuf[ps];
            }
            const int ncols = std::max(1, std::min(256, f.w - k * 256));
            const int ksl = (k == f.nsteps - 1) ? 4 * ((ncols + 15) / 16) : 64;
            const int nrows = f.fp - (k + 1) * 256;
            const int scols = solve_block_cols(f.w, k);
            if (o == me) {
                double *diag = s->factor + top_col(s, ti, k).off;
                const long long lb = T.toplblk[(size_t)T.tbase[ti] + (size_t)k];
                double *i16 = s->inv16 + lb * 4096;
                single(T.potrf, sq, PotrfJob{diag, i16, ldk, f.own0 + k * 256, ncols});
                T.trinv.host.push_back(TrinvJob{diag, i16, s->dinv + lb * 65536, s->dinvt + lb * 65536, ldk});
                single(T.mv, sq, MvJob{s->dinv + lb * 65536, Vf + k * 256, Yf + k * 256});
                int nsplit = 0;
                if (nrows > 0) {
                    single(T.trsm, sq, TrsmJob{diag, diag + 256, i16, ldk, nrows, 0, (ncols + 15) / 16, 0}, nrows / 16);
                    single(T.fwd, sq, FwdJob{diag + 256, Yf + k * 256, Vf + (k + 1) * 256, ldk, nrows, scols, 0}, nrows / 64);
                    nsplit = (nrows + DOT_RPS - 1) / DOT_RPS;
                    if ((long long)nsplit * 256 > s->part_cap) { set_error("nested dissection: partial-sum buffer too small"); return false; }
                    single(T.dot, sq, DotJob{diag + 256, Vf + (k + 1) * 256, s->part, ldk, nrows, nsplit, DOT_RPS, scols, 0}, 16 * nsplit);
                }
                single(T.bwd, sq, BwdJob{s->dinvt + lb * 65536, Yf + k * 256, s->part, Vf + k * 256, nsplit, 0});
            }
            // updates of my block columns right of k by panel k (rows and columns relative to the column's own diagonal block)
            auto push_col = [&](JobTable<SyrkJob> &tab, int J) {
                const TopColDev &cj = top_col(s, ti, J);
                const SyrkJob a{P + (long long)(J - k - 1) * 256, s->factor + cj.off, ldk, cj.ld, (top_block_cols(f, J) + 63) / 64, (f.fp - J * 256) / 64,
                                0, 1, ksl, 0, nullptr, nullptr, nullptr, 0, 0, 0, 0};
                tab.push(a, trapezoid_items(a.nc, a.nr));
            };
            const double iflop = 2.0 * 64 * 64 * 4.0 * ksl;
            if (k + 1 < f.nsteps && top_owner(pt, k + 1) == me) {               // the next block column: on the chain
                T.chain.open();
                push_col(T.chain, k + 1);
                if (!T.chain.close(0, sq, false)) return false;
                T.chain.l[0][sq].flop = iflop * (double)T.chain.l[0][sq].grid;
            }
            T.bulk.open();
            for (int J = (k + 1 < f.nsteps ? k + 2 : k + 1); J < nb; ++J)
                if (top_owner(pt, J) == me) push_col(T.bulk, J);
            if (!T.bulk.close(0, sq, false)) return false;
            T.bulk.l[0][sq].flop = iflop * (double)T.bulk.l[0][sq].grid;
        }
    }
    // my subtree roots take their border values from their (distributed) parents
    T.subroots.clear();
    T.l_maps.clear();
    for (int id : t.by_depth[(size_t)pt.dcut]) {
        if (pt.owner[(size_t)id] != me) continue;
        const NdFront &c = t.fr[(size_t)id];
        T.subroots.push_back(id);
        T.l_maps.push_back((int)T.maps.host.size());
        T.maps.host.push_back(MapJob{s->V + c.vofs + c.wp, T.stagev, s->pmap + c.bofs, c.h, 0});
    }
    for_each_table(T, [&](auto &tab) { ok = ok && nd_upload(s, &tab.dev, tab.host); });
    return ok;
}

}  // namespace nd
}  // namespace splpak
