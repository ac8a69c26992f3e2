// Installs the nested-dissection factorisation on a plan (ndstate.hpp): the tree, this rank's storage, the elimination
// schedule and its Schur arena, the job tables, streams and events; the ranks of a sharded fit; and takes it all down again.
#include "ndstate.hpp"
#include <algorithm>
#include <cstdlib>

namespace splpak {
namespace nd {

bool nd_alloc_bytes(NdState *s, void **ptr, size_t bytes)
{
    void *q = nullptr;
    if (hip_malloc_retry(&q, bytes) != hipSuccess) {
        (void)hipGetLastError();
        char buf[160];
        snprintf(buf, sizeof buf, "nested dissection: hipMalloc of %.3f GB failed", (double)bytes / 1e9);
        set_error(buf);
        return false;
    }
    s->owned.push_back(q);
    s->owned_bytes += bytes;
    *ptr = q;
    return true;
}

void nd_free_bytes(NdState *s, void **ptr)
{
    if (!*ptr) return;
    for (size_t i = 0; i < s->owned.size(); ++i)
        if (s->owned[i] == *ptr) { s->owned.erase(s->owned.begin() + (long)i); break; }
    (void)hipFree(*ptr);
    *ptr = nullptr;
}

namespace {

size_t nd_bytes(void *user) { return user ? static_cast<NdState *>(user)->owned_bytes : 0; }

void nd_destroy(void *user)
{
    NdState *s = static_cast<NdState *>(user);
    if (!s) return;
    (void)hipDeviceSynchronize();
    (void)hipSetDevice(s->device);
    for (hipStream_t q : {s->str.sP, s->str.sU, s->str.sR, s->str.sCopy}) if (q) (void)hipStreamDestroy(q);
    for (hipEvent_t e : s->ev.all) (void)hipEventDestroy(e);
    for (void *q : s->owned) (void)hipFree(q);
    delete s;
}

// sh.rowsrc_out: rowsrc with the rows of the fronts this rank does not report (report(front) false) taken out
template <typename F>
bool upload_rowsrc_out(NdState *s, F &&report)
{
    std::vector<int> out(s->rowsrc_host);
    for (size_t id = 0; id < s->t.fr.size(); ++id) {
        const NdFront &f = s->t.fr[id];
        if (!report(id))
            for (int r = 0; r < f.fp; ++r) out[(size_t)(f.vofs + r)] = -1;
    }
    nd_free_dev(s, &s->sh.rowsrc_out);
    return nd_upload(s, &s->sh.rowsrc_out, out);
}

// (Re)builds the elimination schedule for the fronts in s->mine and sizes the Schur arena for it.  cut < 0: chosen here --
// the level-by-level order (cut = 0: the largest batches) if its arena fits beside `other_bytes` of further allocations in the
// free device memory, otherwise the smallest cut that does (SPLPAK_ND_CUT overrides).
bool nd_make_schedule(NdState *s, int cut, size_t other_bytes)
{
    NdTree &t = s->t;
    const bool packed = !s->mdist && splpak::opt_get("SPLPAK_ND_SQUARE") == nullptr;
    const int dlow = s->mdist ? s->top.pt.dcut : 0;
    s->sch.needs.assign(t.fr.size(), 0);
    for (size_t id = 0; id < t.fr.size(); ++id) {
        const NdFront &f = t.fr[id];
        const bool boundary = s->mdist && f.depth == s->top.pt.dcut;
        s->sch.needs[id] = f.hp > 0 && !(s->sch.fused && f.child[0] < 0 && f.nsteps <= s->sch.schur_kb && !boundary) ? 1 : 0;
    }
    if (cut < 0) {
        cut = 0;
        if (const char *e = splpak::opt_get("SPLPAK_ND_CUT")) cut = std::max(0, std::min(t.maxdepth, atoi(e)));
        else if (!s->mdist) {
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); fr = 0; }
            const double room = (double)fr - (double)other_bytes - std::max(1.0e9, 0.03 * (double)tot);
            long long best = -1;
            int best_cut = 0;
            for (int c = 0; c <= std::min(t.maxdepth, 6); ++c) {
                nd_schedule(t, c, packed, &s->mine, &s->sch.needs, dlow, s->sch.sc);
                if (best < 0 || s->sch.sc.arena < best) { best = s->sch.sc.arena; best_cut = c; }
                if (fr == 0 || 8.0 * (double)s->sch.sc.arena <= room) { best_cut = c; break; }
            }
            cut = best_cut;         // (nothing fits: the smallest arena -- the allocation then fails with the byte counts in the message)
        }
    }
    // (the half-stages: single-GPU plans in the level-by-level order)
    const int halves = (cut == 0 && !s->mdist && !s->dist && splpak::opt_get("SPLPAK_ND_HALVES")) ? atoi(splpak::opt_get("SPLPAK_ND_HALVES")) : 0;
    nd_schedule(t, cut, packed, &s->mine, &s->sch.needs, dlow, s->sch.sc, halves);
    const int ns = (int)s->sch.sc.st.size();
    s->sch.starts.assign((size_t)std::max(ns, 1), {});
    s->sch.root_stage = -1;
    for (int i = 0; i < ns; ++i) {
        const NdStage &S = s->sch.sc.st[(size_t)i];
        s->sch.starts[(size_t)S.first].push_back(i);
        if (S.ids.size() == 1 && t.fr[(size_t)S.ids[0]].parent < 0 && !s->mdist) s->sch.root_stage = i;
    }
    s->sch.istarts.assign((size_t)std::max(ns, 1), {});
    for (int i = 0; i < ns; ++i) {
        const NdStage &S = s->sch.sc.st[(size_t)i];
        s->sch.istarts[(size_t)((S.first == i && i > 0) ? i - 1 : S.first)].push_back(i);
    }
    for (auto *v : {&s->ev.evF, &s->ev.evE, &s->ev.evP})
        while ((int)v->size() < ns + 1) v->push_back(nd_event(s));
    if (s->sch.sc.arena + 64 > s->sarena_doubles) {
        if (s->sarena) {
            (void)hipDeviceSynchronize();
            nd_free_dev(s, &s->sarena);
            s->owned_bytes -= sizeof(double) * (size_t)s->sarena_doubles;
        }
        s->sarena_doubles = 0;
        if (!nd_alloc(s, &s->sarena, (size_t)s->sch.sc.arena + 64)) return false;
        s->sarena_doubles = s->sch.sc.arena + 64;
    }
    return true;
}

// this rank's storage and tables: arenas, the elimination schedule for the memory that is left, index arrays, job tables.  0, or an SPLPAK_E_* code.
int attach_storage(NdState *s, splpak_plan *p)
{
    NdTree &t = s->t;
    const NdPartition &pt = s->top.pt;
    const int rank = s->mrank;
    // this rank's storage: panels and Schur buffers of the fronts it eliminates, then its block columns of the top fronts
    s->poff.assign(t.fr.size(), -1);
    s->lblk.assign(t.fr.size(), -1);
    for (size_t id = 0; id < t.fr.size(); ++id) {
        const NdFront &f = t.fr[id];
        if (!s->mine[id]) continue;
        s->poff[id] = s->factor_doubles;
        s->factor_doubles += f.ld * (long long)f.wp;
        s->lblk[id] = s->nblocks;
        s->nblocks += f.nsteps;
    }
    std::vector<long long> padwhere;
    long long max_fp = 0;
    if (s->mdist) {
        s->top.tbase.assign(pt.top.size(), 0);
        for (size_t ti = 0; ti < pt.top.size(); ++ti) {
            const NdFront &f = t.fr[(size_t)pt.top[ti]];
            s->top.tbase[ti] = (long long)s->top.topcol.size();
            max_fp = std::max(max_fp, (long long)f.fp);
            const int nb = top_nblocks(f);
            for (int J = 0; J < nb; ++J) {
                TopColDev tc{-1, top_block_ld(f, J)};
                int lb = -1;
                if (top_owner(pt, J) == rank) {
                    tc.off = s->factor_doubles;
                    s->factor_doubles += tc.ld * top_block_cols(f, J);
                    if (J < f.nsteps) lb = s->nblocks++;
                    for (int c = J * 256; c < J * 256 + top_block_cols(f, J); ++c)            // identity on the padding of the own columns
                        if (c >= f.w && c < f.wp) padwhere.push_back(tc.off + (long long)(c - J * 256) * (tc.ld + 1));
                }
                s->top.topcol.push_back(tc);
                s->top.toplblk.push_back(lb);
            }
        }
    }
    // Everything but the Schur arena first; the schedule is then chosen for the device memory that is left (the plan still
    // allocates its communication buffer -- half stencil, right-hand side, histogram, residual -- and two vectors after this)
    bool ok = nd_alloc(s, &s->factor, (size_t)s->factor_doubles + 64) && nd_alloc(s, &s->dinv, (size_t)s->nblocks * 65536) &&
              nd_alloc(s, &s->dinvt, (size_t)s->nblocks * 65536) && nd_alloc(s, &s->inv16, (size_t)s->nblocks * 4096) &&
              nd_alloc(s, &s->V, (size_t)t.vec_doubles) && nd_alloc(s, &s->Y, (size_t)t.vec_doubles) &&
              nd_alloc(s, &s->part, (size_t)(s->part_cap = t.vec_doubles / 4 + 256LL * (long long)t.fr.size() + 4096));
    if (ok) {
        const size_t later = sizeof(double) * ((size_t)p->g.ncol * (size_t)(p->g.hstencil + 8)) + sizeof(int) * 8 * (size_t)t.vec_doubles;
        ok = nd_make_schedule(s, -1, later);
        if (!ok) {
            char buf[320];
            snprintf(buf, sizeof buf, "nested dissection: the Schur arena of %.1f GB (packed lower triangles, schedule cut %d) does not fit beside %.1f GB of factor panels",
                     8e-9 * (double)s->sch.sc.arena, s->sch.sc.cut, 8e-9 * (double)s->factor_doubles);
            set_error(buf);
        }
    }
    if (ok && s->mdist) {
        for (int i = 0; i < 3 && ok; ++i) ok = nd_alloc(s, &s->top.pbuf[i], (size_t)pt.max_panel + 64);
        s->top.stagev_doubles = max_fp + 64;
        ok = ok && nd_alloc(s, &s->top.stagev, (size_t)s->top.stagev_doubles);
    }
    if (!ok) return SPLPAK_E_NOMEM;
    // tables
    std::vector<int> rowsrc((size_t)t.vec_doubles, -1);
    std::vector<FrontDev> fdev;
    for (size_t id = 0; id < t.fr.size(); ++id) {
        const NdFront &f = t.fr[id];
        for (int r = 0; r < f.w; ++r) rowsrc[(size_t)(f.vofs + r)] = t.ownvar[(size_t)(f.rofs + r)];
        if (s->poff[id] >= 0)
            for (int r = f.w; r < f.wp; ++r) padwhere.push_back(s->poff[id] + r + (long long)r * f.ld);
        const int ti = s->mdist ? pt.top_index[id] : -1;
        fdev.push_back(FrontDev{s->poff[id], f.ld, f.bofs, f.own0, f.w, f.wp, f.h, ti >= 0 ? (int)s->top.tbase[(size_t)ti] : -1, 0});
    }
    s->npad = (int)padwhere.size();
    {
        int maxpos = -1;
        for (int v : t.pos) maxpos = std::max(maxpos, v);
        std::vector<int> ipos((size_t)(maxpos + 1), -1);
        for (size_t i = 0; i < t.pos.size(); ++i)
            if (t.pos[i] >= 0) ipos[(size_t)t.pos[i]] = (int)i;
        if (!nd_upload(s, &s->ipos, ipos)) return SPLPAK_E_NOMEM;
    }
    s->sch.staged_init = !s->mdist && !(splpak::opt_get("SPLPAK_ND_STAGED_INIT") && atoi(splpak::opt_get("SPLPAK_ND_STAGED_INIT")) == 0);
    ok = nd_upload(s, &s->pos, t.pos) && nd_upload(s, &s->front_of, t.front_of) && nd_upload(s, &s->bpos, t.bpos) &&
         nd_upload(s, &s->pmap, t.pmap) && nd_upload(s, &s->rowsrc, rowsrc) && nd_upload(s, &s->padwhere, padwhere) &&
         nd_upload(s, &s->fdev, fdev) && nd_upload(s, &s->top.topcol_dev, s->top.topcol);
    if (!ok) return SPLPAK_E_NOMEM;
    s->rowsrc_host.swap(rowsrc);
    s->full_diag = splpak::opt_get("SPLPAK_ND_FULL_DIAG") != nullptr ? 1 : 0;      // (before the job tables: it enters their flop counts)
    // XCD-aware item map of the Schur passes: on (round 4) -- half the fabric traffic per launch for the same factor bits at
    // +0.2 .. 0.4 % time (SPLPAK_ND_XCD=0: the plain map)
    s->xmode = splpak::opt_get("SPLPAK_ND_XCD") ? atoi(splpak::opt_get("SPLPAK_ND_XCD")) : 1;
    if (const int rc = nd_make_jobs(s)) {
        if (rc == SPLPAK_E_UNSUPPORTED) set_error("nested dissection: job tables");
        return rc;
    }
    // what this rank reports into the solution: its subtrees' variables and the top fronts it ends the backward sweep of
    if (s->mdist && !upload_rowsrc_out(s, [&](size_t id) { return pt.owner[id] >= 0 ? pt.owner[id] == rank : top_owner(pt, 0) == rank; })) return SPLPAK_E_NOMEM;
    return 0;
}

// streams, events, item queues and the CUs reserved for the diagonal blocks.  0, or an SPLPAK_E_* code.
int attach_streams(NdState *s)
{
    NdTree &t = s->t;
    // the host copies of the big index arrays are no longer needed
    std::vector<int>().swap(t.ownvar);
    std::vector<int>().swap(t.bvar);
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    (void)hipStreamCreateWithPriority(&s->str.sP, hipStreamNonBlocking, hi);
    (void)hipStreamCreateWithFlags(&s->str.sU, hipStreamNonBlocking);
    for (hipEvent_t *e : {&s->ev.ev0, &s->ev.evJ, &s->ev.evU, &s->ev.evZlast, &s->ev.evDone, &s->ev.evPre, &s->ev.evTail, &s->ev.evR0}) *e = nd_event(s);
    // item queues of the update launches (two per step at most)
    s->nqueues = 8 * t.nblocks + 64;
    if (const char *e = splpak::opt_get("SPLPAK_ND_SMALL_GRID")) s->small_grid = atoi(e);
    if (const char *e = splpak::opt_get("SPLPAK_ND_WG4")) s->wg4 = atoi(e);
    s->small_queue = splpak::opt_get("SPLPAK_ND_SMALL_QUEUE") != nullptr;
    if (const char *e = splpak::opt_get("SPLPAK_ND_POTRF_WAVES")) s->potrf_waves = atoi(e);
    if (!nd_alloc(s, &s->queues, (size_t)ND_QSTRIDE * s->nqueues) || !nd_alloc(s, &s->resmap, (size_t)128)) return SPLPAK_E_NOMEM;
    (void)hipMemset(s->resmap, 0, 128 * sizeof(unsigned));
    // A few CUs are left to the diagonal-block factorisations of the upper tree levels: v_mfma_f64 runs on the same
    // pipes as f64 VALU code, and the latency-bound potrf workgroups ran 8x slower (1.26 ms instead of 0.16) beside
    // the update waves (rocprofv3, 64^3).  potrf is pinned to those CUs through a CU-masked stream; the update
    // waves are not masked, they step aside when they find themselves there (nd_syrk_kernel).  Only trees whose
    // upper levels are worth it (>= 8 block steps in the root) pay for the extra stream.
    const int want_res = splpak::opt_get("SPLPAK_ND_RES_CUS") ? atoi(splpak::opt_get("SPLPAK_ND_RES_CUS")) : 8;
    if (want_res > 0 && t.fr[(size_t)t.root].nsteps >= 8 && !splpak::opt_get("SPLPAK_NO_PANEL_CU")) {
        hipDeviceProp_t prop;
        (void)hipGetDeviceProperties(&prop, s->device);
        const int ncu = prop.multiProcessorCount;
        std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
        for (int i = 0; i < want_res && i < ncu; ++i) mask[(size_t)i / 32] |= 1u << (i % 32);
        if (hipExtStreamCreateWithCUMask(&s->str.sR, (uint32_t)mask.size(), mask.data()) == hipSuccess) {
            launch_whoami(64 * (unsigned)want_res, s->resmap, s->str.sR);
            unsigned hm[128];
            if (hipStreamSynchronize(s->str.sR) == hipSuccess && hipMemcpy(hm, s->resmap, sizeof hm, hipMemcpyDeviceToHost) == hipSuccess)
                for (unsigned wv : hm) s->nres += __builtin_popcount(wv);
            if (s->nres == 0 || s->nres > 2 * want_res) {      // the mask did not take: no pinning
                (void)hipStreamDestroy(s->str.sR);
                s->str.sR = nullptr;
                s->nres = 0;
                (void)hipMemset(s->resmap, 0, 128 * sizeof(unsigned));
            }
        } else {
            (void)hipGetLastError();
            s->str.sR = nullptr;
        }
    }
    if (s->mdist) {
        (void)hipStreamCreateWithPriority(&s->str.sCopy, hipStreamNonBlocking, hi);
        for (auto *v : {&s->top.evReady, &s->top.evArr, &s->top.evCol, &s->top.evBulk, &s->top.evSF, &s->top.evSB}) {
            v->assign((size_t)s->top.pt.nseq + 1, nullptr);
            for (hipEvent_t &e : *v) e = nd_event(s);
        }
        s->top.evAdd.assign(s->top.pt.top.size() + 1, nullptr);
        for (hipEvent_t &e : s->top.evAdd) e = nd_event(s);
        s->top.evSub = nd_event(s);
        s->top.evTop = nd_event(s);
        if (!s->str.sCopy || !s->top.evSub || !s->top.evTop) { set_error("nested dissection: stream creation failed"); (void)hipGetLastError(); return SPLPAK_E_NODEVICE; }
    }
    if (!s->str.sP || !s->str.sU) { set_error("nested dissection: stream creation failed"); (void)hipGetLastError(); return SPLPAK_E_NODEVICE; }
    return 0;
}

}  // namespace
}  // namespace nd

using namespace nd;

// Ownership of the fronts for `world` ranks and the job tables that follow from it (see NdState::dist).  Called when the
// sharded fit's ranks become known (splpak_plan_set_allreduce comes after the plan); SPLPAK_ND_DIST=0 opts out.
int nd_set_ranks(splpak_plan *p, int rank, int world)
{
    NdState *s = p && p->fn_code == 4 ? static_cast<NdState *>(p->fn_user) : nullptr;
    if (!s || s->mdist) return 0;
    NdTree &t = s->t;
    int dcut = 0;
    while ((1 << dcut) < world) ++dcut;
    const char *sw = splpak::opt_get("SPLPAK_ND_DIST");                  // 0 = every rank factors everything (round 2's form)
    // (the join sums front panels, Schur buffers and solve vectors that live outside the plan's communication buffer: only with a
    //  hook that declared it accepts any device pointer -- SPLPAK_AR_ANY_POINTER; round-3 advice)
    const bool want = world > 1 && p->ar != nullptr && (p->ar_flags & SPLPAK_AR_ANY_POINTER) != 0 && !(sw && atoi(sw) == 0) && dcut >= 1 &&
                      dcut <= t.maxdepth && (s->sch.sc.cut == 0 || s->dist);
    if (!want && !s->dist) return 0;
    (void)hipDeviceSynchronize();
    s->dist = want;
    s->sh.world = world;
    s->sh.rank = rank;
    s->sh.dcut = want ? dcut : 0;
    s->mine.assign(t.fr.size(), 1);
    if (want) {
        std::vector<int> slot_of(t.fr.size(), -1);          // index of the depth-dcut ancestor among the fronts of that depth
        const std::vector<int> &cut = t.by_depth[(size_t)dcut];
        for (size_t i = 0; i < cut.size(); ++i) slot_of[(size_t)cut[i]] = (int)i;
        for (int id = (int)t.fr.size() - 1; id >= 0; --id) {   // parents have larger ids than their children (postorder)
            const NdFront &f = t.fr[(size_t)id];
            if (f.depth > dcut) slot_of[(size_t)id] = slot_of[(size_t)f.parent];
            if (f.depth >= dcut) s->mine[(size_t)id] = (slot_of[(size_t)id] % world) == rank ? 1 : 0;
        }
    }
    if (!nd_make_schedule(s, want ? 0 : -1, 0)) return SPLPAK_E_NOMEM;
    if (const int rc = nd_make_jobs(s)) {
        if (rc == SPLPAK_E_UNSUPPORTED) set_error("nested dissection: job tables (ranks)");
        return rc;
    }
    if (!upload_rowsrc_out(s, [&](size_t id) { return want ? (t.fr[id].depth >= dcut ? s->mine[id] != 0 : rank == 0) : true; })) return SPLPAK_E_NOMEM;
    if (want && !s->sch.sc.packed) {
        long long need = 0;
        for (int id : t.by_depth[(size_t)(dcut - 1)]) {
            const long long nt = t.fr[(size_t)id].hp / 64;
            need = std::max(need, trapezoid_items(nt, nt) * 4096);
        }
        if (need > s->sh.join_scratch_doubles) {
            double *q = nullptr;
            if (hipMalloc(&q, sizeof(double) * (size_t)need) == hipSuccess) {      // (no room: the join sums the square buffers)
                s->owned.push_back(q);
                s->sh.join_scratch = q;
                s->sh.join_scratch_doubles = need;
            } else
                (void)hipGetLastError();
        }
    }
    s->s_clean = false;
    if (splpak::opt_get("SPLPAK_DEBUG")) {
        int nm = 0;
        for (char c : s->mine) nm += c;
        fprintf(stderr, "[splpak] nested dissection: rank %d of %d eliminates %d of %zu fronts (subtrees below depth %d)\n", rank, world, nm, t.fr.size(), dcut);
    }
    return 0;
}

bool nd_wanted_for(int ndim, const int *nodes, const double *xmin, const double *xmax)
{
    Grid g;
    if (build_grid(ndim, nodes, xmin, xmax, g, nullptr, splpak::opt_get("SPLPAK_NO_REORDER") == nullptr) != 0) return false;
    return nd_wanted(g);
}

// SPLPAK_ND: 0 = never, 1 = always; otherwise 2-D / 3-D grids of at least 4 096 columns and 4-D grids of at least 20 000.
// Measured on MI355X (tools/nd_crossover.sh, fit time band -> nested dissection): 2-D 48^2 2.08 -> 2.27 ms (band stays),
// 64^2 (BASELINE config 2) 3.29 -> 2.46, 90^2 5.7 -> 4.3, 128^2 10.4 -> 5.1, 256^2 41.5 -> 13.1; 3-D 16^3 4.3 -> 3.7, 20^3 6.6 ->
// 5.9, 24^3 11.4 -> 9.0, 32^3 26.3 -> 17.8, 40^3 67.7 -> 42.5, 48^3 166 -> 85, 64^3 831 -> 280; 4-D 8^4 10.9 -> 11.2 and 10^4
// 19.5 -> 20.3 (band stays), 12^4 41.9 -> 41.0, 16^4 239 -> 184, 24^4 10.5 s -> 4.9 s.
bool nd_wanted(const Grid &g)
{
    if (const char *e = splpak::opt_get("SPLPAK_ND")) return atoi(e) != 0;
    if (g.ndim == 2 || g.ndim == 3) return g.ncol >= 4096;
    return g.ndim == 4 && g.ncol >= 20000;
}

// Installs the nested-dissection factorisation on a single-GPU plan: builds the tree, allocates the arenas,
// uploads the tables.  Returns 0, or an SPLPAK_E_* code (the plan is then unusable).  *factor_arena /
// *factor_doubles: the factor storage, idle until the half stencil is assembled (the Gram scratch may live there).
int nd_attach(splpak_plan *p, double **factor_arena, long long *factor_doubles, NdGroup *grp, int rank)
{
    NdState *s = new NdState();
    (void)hipGetDevice(&s->device);
    p->fn_user = s;
    p->fn_destroy = nd_destroy;
    p->fn_bytes = nd_bytes;
    if (!nd_build(p->g, s->t, nd_default_split_min(p->g.ndim))) { set_error("nested dissection: inconsistent tree"); return SPLPAK_E_BADARG; }
    NdTree &t = s->t;
    // one-process multi-GPU fit: this plan is rank `rank` of the group
    s->grp = grp;
    s->mrank = rank;
    s->mdist = grp != nullptr && grp->R > 1;
    nd_partition(t, s->mdist ? grp->R : 1, s->mdist ? grp->chunk : 1, s->top.pt);
    if (s->mdist && s->top.pt.dcut < 1) s->mdist = false;                 // (a tree of one front: nothing to distribute)
    if (grp) {
        if (rank < 0 || rank >= grp->R) { set_error("nested dissection: bad rank"); return SPLPAK_E_BADARG; }
        grp->st[(size_t)rank] = s;
    }
    if (grp && grp->R > 1 && !s->mdist) { set_error("nested dissection: the tree of this grid has a single front; use one GPU"); return SPLPAK_E_UNSUPPORTED; }
    const NdPartition &pt = s->top.pt;
    s->mine.assign(t.fr.size(), 1);
    if (s->mdist)
        for (size_t id = 0; id < t.fr.size(); ++id) s->mine[id] = pt.owner[id] == rank ? 1 : 0;
    s->sch.fused = splpak::opt_get("SPLPAK_ND_NO_FUSE") == nullptr;
    if (const char *e = splpak::opt_get("SPLPAK_ND_KB")) s->sch.schur_kb = std::max(1, std::min(4, atoi(e)));
    if (const int rc = attach_storage(s, p)) return rc;
    if (const int rc = attach_streams(s)) return rc;
    p->expand_fn = nd_assemble;
    p->prefit_fn = nd_prefit;
    p->factor_fn = nd_factor;
    p->solve_fn = nd_solve;
    {
        char buf[256];
        snprintf(buf, sizeof buf, "; %zu fronts in %zu stages (schedule cut %d), %.1f GB of factor panels, %.1f GB Schur arena (%s)", t.fr.size(), s->sch.sc.st.size(),
                 s->sch.sc.cut, 8e-9 * (double)s->factor_doubles, 8e-9 * (double)s->sarena_doubles, s->sch.sc.packed ? "packed lower triangles" : "square buffers");
        s->desc = s->mdist ? "nested-dissection multifrontal Cholesky distributed over several GPUs: subtrees per GPU, top fronts by block columns (csrc/ndchol.hip, csrc/ndtop.hip)"
                           : "nested-dissection multifrontal Cholesky (csrc/ndtree.hip, csrc/ndchol.hip)";
        s->desc += buf;
    }
    p->fn_name = s->desc.c_str();
    p->fn_code = s->mdist ? 5 : 4;
    p->factor_flop = t.flop;                 // (what the iteration in front of this factorisation may spend is weighed against it, planfit.hip)
    if (factor_arena) *factor_arena = s->factor;
    if (factor_doubles) *factor_doubles = s->factor_doubles;
    if (splpak::opt_get("SPLPAK_DEBUG"))
        fprintf(stderr, "[splpak] nested dissection%s: %zu fronts, depth %d, factor %.2f GB, Schur arena %.2f GB (%s, %zu stages, cut %d), %.3e flop, %d reserved CUs\n",
                s->mdist ? " (one rank of a multi-GPU fit)" : "", t.fr.size(), t.maxdepth, 8e-9 * (double)s->factor_doubles, 8e-9 * (double)s->sarena_doubles,
                s->sch.sc.packed ? "packed" : "square", s->sch.sc.st.size(), s->sch.sc.cut, t.flop, s->nres);
    return 0;
}

}  // namespace splpak
