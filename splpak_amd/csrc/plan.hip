// The plan and its part of the C ABI (include/splpak_hip.h): creation and destruction, the communication buffer's layout, the setters
// and getters, the options, the error message and the device name.  The fit and the refit on a plan are in planfit.hip, the one-shot
// fit entries and shutdown in hostfit.hip, the debug-plan entries in plandebug.hip, the evaluation entries in evalapi.hip.
#include "plan.hpp"
#include "basis.hpp"

#include <cstring>
#include <limits>

namespace splpak {

static thread_local std::string g_err;

void set_error(const std::string &msg) { g_err = msg; }

bool hip_ok(hipError_t e, const char *what)
{
    if (e == hipSuccess) return true;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    (void)hipGetLastError();
    return false;
}

// reference-order validation shared by fit and evaluation (:716-750, :1166-1210).
// returns 0 or 101/102/103
int build_grid(int ndim, const int *nodes, const double *xmin, const double *xmax, Grid &g,
               long long *ncol_out, bool reorder)
{
    std::memset(&g, 0, sizeof(g));
    if (ndim < 1) return 101;
    if (ndim > MAXD) return SPLPAK_E_UNSUPPORTED;
    g.ndim = ndim;
    // checks in the reference's order (first failing dimension wins), reference-order copies
    long long rs = 1;
    int refstride_of[MAXD] = {0, 0, 0, 0};
    for (int d = 0; d < ndim; ++d) {
        if (nodes[d] < 4) return 102;
        const double xrng = xmax[d] - xmin[d];
        if (xrng == 0.0) return 103;
        g.ref_nodes[d] = nodes[d];
        g.ref_xmin[d] = xmin[d];
        g.ref_dxin[d] = 1.0 / (xrng / (double)(nodes[d] - 1));
        refstride_of[d] = (int)rs;
        rs *= nodes[d];
        if (rs > (1LL << 30)) { if (ncol_out) *ncol_out = rs; return SPLPAK_E_UNSUPPORTED; }
    }
    for (int d = 0; d < MAXD; ++d) g.perm[d] = d;
    if (reorder)        // ascending node counts, stable: identity for isotropic grids
        for (int i = 1; i < ndim; ++i)
            for (int j = i; j > 0 && nodes[g.perm[j]] < nodes[g.perm[j - 1]]; --j) std::swap(g.perm[j], g.perm[j - 1]);
    long long ncol = 1, ncell = 1, cs = 1, ls = 1;
    int nb = 1, h = 1, hb = 0;
    for (int d = 0; d < ndim; ++d) {
        const int r = g.perm[d];
        const int nod = nodes[r];
        const double xrng = xmax[r] - xmin[r];
        g.nodes[d] = nod;
        g.xmin[d] = xmin[r];
        g.dx[d] = xrng / (double)(nod - 1);        // :747
        g.dxin[d] = 1.0 / g.dx[d];                 // :748
        g.colstride[d] = (int)cs;
        g.refstride[d] = refstride_of[r];
        g.cells[d] = nod - 3;
        g.cellstride[d] = (int)ls;
        hb += 3 * (int)cs;
        cs *= nod;
        ls *= (nod - 3);
        ncol *= nod;
        ncell *= (nod - 3);
        nb *= 4;
        h *= 7;
    }
    for (int d = ndim; d < MAXD; ++d) {
        g.nodes[d] = 4; g.dx[d] = g.dxin[d] = 1.0; g.cells[d] = 1;
        g.ref_nodes[d] = 4; g.ref_dxin[d] = 1.0;
    }
    g.ncol = (int)ncol;
    g.ncell = (int)ncell;
    g.nb = nb;
    g.hstencil = (h + 1) / 2;
    g.halfbw = hb;
    if (ncol_out) *ncol_out = ncol;
    return 0;
}

// The communication buffer: three windows, each a vector and behind it the scalars that travel with it through one all-reduce --
// G: the half stencil (not in a rows-only plan's), rhs, scalG;  H: hist, scalH;  R: rho, scalR (residual sum of squares)
static long long comm_lenG(const Grid &g, bool rows_only) { return (rows_only ? 0 : (long long)g.ncol * g.hstencil) + g.ncol + SC_COUNT; }
static long long comm_lenH(const Grid &g) { return (long long)g.ncol + SC_COUNT; }
static long long comm_lenR(const Grid &g) { return ((g.ncol + NBLK - 1) / NBLK) * (long long)NBLK + SC_COUNT; }
static long long comm_len_of(const Grid &g, bool rows_only) { return comm_lenG(g, rows_only) + comm_lenH(g) + comm_lenR(g); }

bool band_alloc_inverses(splpak_plan *p, Band &b, size_t nblocks, bool sweeps)
{
    return dev_alloc(p, &b.dinv, nblocks * NBLK * NBLK) && dev_alloc(p, &b.dinvt, nblocks * NBLK * NBLK) &&
           dev_alloc(p, &b.inv64, nblocks * 4 * 64 * 64) &&
           (!sweeps || (dev_alloc(p, &b.mfwd, nblocks * NBLK * NBLK) && dev_alloc(p, &b.mbwd, nblocks * NBLK * NBLK)));
}

bool sort_scratch_alloc(splpak_plan *owner, const Grid &g, long long max_ndata, SortScratch *s)
{
    bool ok = true;
    s->cap = max_ndata;
    ok = ok && dev_alloc(owner, &s->key, (size_t)max_ndata);
    ok = ok && dev_alloc(owner, &s->count, (size_t)g.ncell + 2);
    ok = ok && dev_alloc(owner, &s->scanpart, (size_t)256);
    ok = ok && dev_alloc(owner, &s->offset, (size_t)g.ncell + 2);
    ok = ok && dev_alloc(owner, &s->cursor, (size_t)g.ncell + 2);
    ok = ok && dev_alloc(owner, &s->xs, (size_t)max_ndata * g.ndim);
    ok = ok && dev_alloc(owner, &s->ys, (size_t)max_ndata);
    ok = ok && dev_alloc(owner, &s->ws, (size_t)max_ndata);
    ok = ok && dev_alloc(owner, &s->idx, (size_t)max_ndata);
    {   // stable partition of the points (binpoints.hip sp_*): count matrix, bin bases, tile-sorted records for grids of more cells than bins
        const size_t nblk = (size_t)((max_ndata + SP_Q - 1) / SP_Q);
        ok = ok && dev_alloc(owner, &s->cntm, nblk * SP_NB);
        ok = ok && dev_alloc(owner, &s->binbase, (size_t)2 * SP_NB + 16);      // bin bases | bin totals
        ok = ok && dev_alloc(owner, &s->sppart, ((nblk + 15) / 16) * SP_NB);
        const long long rd = bin_record_doubles(g, max_ndata);
        if (rd > 0) ok = ok && dev_alloc(owner, &s->rec, (size_t)rd);
    }
    if (ok && bin_route(g, *s, nullptr) == 0) ok = dev_alloc(owner, &s->ordtmp, (size_t)max_ndata);      // the atomic route: the keys survive its re-sort
    return ok;
}

int device_ready()
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no usable HIP device: the splpak HIP path has no CPU fallback");
        (void)hipGetLastError();
        return SPLPAK_E_NODEVICE;
    }
    return 0;
}

}  // namespace splpak

using namespace splpak;

int splpak::plan_create_dist(int ndim, const int *nodes, const double *xmin, const double *xmax, double xtrap,
                             long long max_ndata, void *comm_buf_dev, long long comm_len, int R, int r, int c,
                             splpak_plan **plan, bool allow_nd, NdGroup *ndgrp)
{
    if (!plan || !nodes || !xmin || !xmax) { set_error("null argument"); return SPLPAK_E_BADARG; }
    *plan = nullptr;
    const Options snap = options_snapshot();        // the switches of this plan: process defaults over the environment, as of now
    OptionsScope opt_scope(&snap);
    Grid g;
    long long ncol = 0;
    const int v = build_grid(ndim, nodes, xmin, xmax, g, &ncol, splpak::opt_get("SPLPAK_NO_REORDER") == nullptr);
    if (v != 0) {
        if (v == SPLPAK_E_UNSUPPORTED) set_error("ndim > 4 or more than 2^30 nodes is not supported");
        return v;
    }
    if (max_ndata < 1) return 105;
    if (max_ndata > (int64_t)std::numeric_limits<int32_t>::max() - 1024) {
        // the binning (keys, per-cell offsets and cursors, the scan) is 32-bit
        set_error("max_ndata per plan (= per GPU) is limited to 2^31 - 1025 points; shard the points over more plans");
        return SPLPAK_E_UNSUPPORTED;
    }
    // How the least-squares problem is solved: SPLPAK_SOLVER = direct | pcg | pcg+direct names it; auto, an empty value or no value
    // leave the choice to the plan (below).  Anything else is a mistake the caller hears about, not a silent "auto".
    int mode = 0;
    bool named = false;
    if (const char *e = splpak::opt_get("SPLPAK_SOLVER")) {
        if (!std::strcmp(e, "direct")) mode = 1;
        else if (!std::strcmp(e, "pcg")) mode = 2;
        else if (!std::strcmp(e, "pcg+direct")) mode = 3;
        else if (*e && std::strcmp(e, "auto")) {
            set_error(std::string("SPLPAK_SOLVER=") + e + ": the accepted values are direct, pcg, pcg+direct and auto (the same as unset or empty)");
            return SPLPAK_E_BADARG;
        }
        named = mode != 0;
    }
    if (int r = device_ready()) return r;
    const char *rt = splpak::opt_get("SPLPAK_ROWS_TILES");
    const bool rows_tiles = !(rt && atoi(rt) == 0);      // 4-D: the passes over the rows go tile by tile (rowsop.hip) unless switched off

    splpak_plan *p = new splpak_plan();
    const auto give_up = [p](int rc) { splpak_plan_destroy(p); return rc; };      // every failure from here on
    p->opt = snap;
    p->g = g;
    p->xtrap = xtrap;
    p->max_ndata = max_ndata;
    bool ok = sort_scratch_alloc(p, g, max_ndata, &p->s);
    {   // per-cell shares of the residual passes of residual.hip: 1-D and 2-D grids; a 3-D or 4-D grid's passes go tile by tile
        // (rows3tile.hip, rowsop.hip) and leave this scratch out (1.45 GB at 32^4, 116 MB at 64^3) unless the A/B switches ask for
        // the cell-by-cell forms
        const bool tiled = g.ndim >= 3 && rows_tiles && !splpak::opt_get("SPLPAK_RESIDUAL_CELLS");
        if (!tiled) ok = ok && dev_alloc(p, &p->rcell, (size_t)g.ncell * g.nb);
        if (g.ndim == 3 && rows_tiles) ok = ok && dev_alloc(p, &p->rows3.partial, (size_t)rows3_tiles(g, &p->rows3));
    }
    ok = ok && dev_alloc(p, &p->tbuf, (size_t)g.ncol * (g.ndim * (g.ndim + 1) / 2));
    ok = ok && dev_alloc(p, &p->dcw, (size_t)g.ncol);
    ok = ok && dev_alloc(p, &p->ctab, (size_t)constraint_table_doubles(g));
    ok = ok && dev_alloc(p, &p->spf, (size_t)g.ncol);
    ok = ok && dev_alloc(p, &p->e2buf, (size_t)g.ncell + (size_t)g.ncol);
    // band: all of it (R = 1) or the block columns dealt to rank r of R
    band_bytes(g.ncol, g.halfbw, &p->band);
    (void)hipGetDevice(&p->device);
    p->dm = DistMap{R < 1 ? 1 : R, r, c < 1 ? 1 : c, p->band.lda + 1};
    for (int J = 0; J < p->band.nblk; ++J)
        if (dm_owned(p->dm, J)) p->own_blocks_host.push_back(J);
    p->nown = (int)p->own_blocks_host.size();
    if (p->dm.R > 1) p->band.bytes = (size_t)(p->nown > 0 ? p->nown : 1) * NBLK * (size_t)p->dm.ld * sizeof(double) + 4096;
    // Large 3-D / 4-D grids on one GPU: the nested-dissection multifrontal factorisation (ndchol.hip) instead of the
    // band.  It owns its storage; the factor arena stands in for the band as the home of the Gram scratch.
    // Several GPUs driven by one process (ndgrp): the same factorisation, distributed -- every rank keeps its own subtrees and
    // its block columns of the fronts above them (round 4; ndchol.hip, ndtop.hip).
    // How the least-squares problem is solved (round 6): a factorisation (band / nested dissection) whenever one fits the device;
    // the iteration of pcg.hip for the grids none fits (4-D from about 29^4 on one GPU) or by request -- SPLPAK_SOLVER =
    // direct | pcg | pcg+direct (the iteration first, the factorisation when it stagnates) | auto.
    if (p->dm.R > 1) mode = 1;                      // (the one-process multi-GPU plans distribute a factorisation)
    // Left to itself a LARGE 4-D grid (from 20^4 columns on: the factorisation takes seconds) tries the iteration first: where the
    // constraint rows are dense (>= 2 per column: config 5's density of points) or absent it answers in a fraction of the
    // factorisation's time (24^4: 0.5 s against 4.6 s, 28^4: ~1.4 s against 18 s); where it stagnates (1.2 .. 1.7 rows per column)
    // the attempt costs 0.6 .. 1.4 s before the factorisation takes over (tools/pcg/density_sweep.py).
    if (mode == 0 && g.ndim == 4 && g.ncol >= 160000) mode = 3;
    const bool auto_mode = !named && p->dm.R == 1;      // the plan chose: what does not fit or is not supported is replaced, not reported
    bool direct = mode != 2;
    const bool use_nd = direct && allow_nd && (p->dm.R == 1 || ndgrp != nullptr) && nd_wanted(g);
    if (use_nd && ok) {
        double *arena = nullptr;
        long long arena_doubles = 0;
        const int rc = nd_attach(p, &arena, &arena_doubles, p->dm.R > 1 ? ndgrp : nullptr, r);
        if (rc == SPLPAK_E_NOMEM && auto_mode && p->dm.R == 1) {
            // no factorisation of this grid fits the device: the iteration instead
            if (p->fn_destroy) p->fn_destroy(p->fn_user);
            p->fn_user = nullptr; p->fn_destroy = nullptr; p->fn_bytes = nullptr; p->fn_name = nullptr; p->fn_code = 0;
            p->factor_fn = nullptr; p->solve_fn = nullptr; p->expand_fn = nullptr; p->prefit_fn = nullptr;
            (void)hipGetLastError();
            direct = false;
        } else if (rc != 0) {
            return give_up(rc);
        } else {
            p->band.ab = arena;
            p->band.bytes = (size_t)arena_doubles * sizeof(double);
        }
    } else if (direct && ok) {
        const bool okb = dev_alloc(p, &p->band.ab, p->band.bytes / sizeof(double));
        if (!okb && auto_mode && p->dm.R == 1) direct = false;
        else ok = ok && okb;
    }
    if (!direct) { p->band.ab = nullptr; p->band.bytes = 0; }
    // Iteration-only plans of 4-D grids never assemble the normal equations (round 6): the iteration applies the ROWS, and the
    // right-hand side, the histogram and the backward-error denominators come from the rows too (rowsop.hip) -- no half stencil
    // (10 GB at 32^4, and its all-reduce in a sharded fit), no Gram scratch (8 GB), no Gram / gather / constraint-row kernels
    // (0.30 of the 0.32 s of config 5's assembly).  pcg_assemble = 1 keeps the assembled form (A/B).
    p->rows_only = !direct && g.ndim == 4 && rows_tiles && !splpak::opt_get("SPLPAK_PCG_ASSEMBLE");
    {
        // scratch of the per-cell Gram blocks: everything at once if <= 8 GB (or if the band storage, which is
        // idle until the gather is done, holds it); otherwise slabs of what there is (launch_gram)
        const long long full = p->rows_only ? 8 : gram_scratch_doubles(g), least = p->rows_only ? 8 : gram_scratch_min_doubles(g);
        long long want = full;
        const char *cap = splpak::opt_get("SPLPAK_GRAM_SCRATCH_MB");
        const long long budget = cap ? atoll(cap) * (1LL << 17) : (1LL << 30);      // doubles (default 8 GB)
        if (want > budget) want = budget > least ? budget : least;
        const long long band_doubles = (long long)(p->band.bytes / sizeof(double));
        if (band_doubles >= want && !cap) {
            p->gscratch = p->band.ab;
            p->gscratch_doubles = band_doubles < full ? band_doubles : full;
        } else {
            ok = ok && dev_alloc(p, &p->gscratch, (size_t)want);
            p->gscratch_doubles = want;
        }
    }
    const size_t nloc = (use_nd || !direct) ? 0 : (size_t)(p->nown > 0 ? p->nown : 1);      // (the band's block inverses: not with nested dissection)
    ok = ok && band_alloc_inverses(p, p->band, nloc, p->dm.R == 1);
    if (p->dm.R > 1) {
        ok = ok && dev_alloc(p, &p->own_blocks, nloc);
        if (ok && p->nown > 0 && !use_nd)
            ok = hip_ok(hipMemcpy(p->own_blocks, p->own_blocks_host.data(), sizeof(int) * (size_t)p->nown, hipMemcpyHostToDevice),
                        "hipMemcpy of the block list");
    }
    // communication buffer (rows-only plans: no half stencil in it -- right-hand side first)
    p->lenG = comm_lenG(g, p->rows_only);
    p->lenH = comm_lenH(g);
    p->lenR = comm_lenR(g);
    p->comm_len = comm_len_of(g, p->rows_only);
    if (comm_buf_dev) {
        if (comm_len < p->comm_len) { set_error("comm buffer too small"); return give_up(SPLPAK_E_BADARG); }
        p->comm = static_cast<double *>(comm_buf_dev);
    } else {
        ok = ok && dev_alloc(p, &p->comm, (size_t)p->comm_len);
        p->own_comm = true;
    }
    ok = ok && dev_alloc(p, &p->xvec, (size_t)p->band.npad);
    ok = ok && dev_alloc(p, &p->tmp, (size_t)p->band.npad);
    ok = ok && dev_alloc(p, &p->small, 8);
    ok = ok && dev_alloc(p, &p->info, 2);
    if (!ok) return give_up(SPLPAK_E_NOMEM);
    p->nst = p->rows_only ? nullptr : p->comm;
    p->scalG = p->comm + p->lenG - SC_COUNT;
    p->rhs = p->scalG - g.ncol;
    p->hist = p->comm + p->lenG;
    p->scalH = p->hist + g.ncol;
    p->rho = p->hist + p->lenH;
    if (!hip_ok(launch_constraint_table(g, p->ctab, nullptr), "constraint table") ||
        !hip_ok(hipStreamSynchronize(nullptr), "constraint table"))
        return give_up(SPLPAK_E_NODEVICE);
    if (const int rc = rowsop_create(g, !direct, &p->rowsop)) return give_up(rc);
    if (direct) twoend_attach(p);
    p->solver_mode = !direct ? 2 : (mode == 3 ? 3 : 0);
    if (!direct || mode == 3) {
        const int rc = pcg_attach(p, &p->pcg);
        if (rc != 0 && direct && auto_mode) {
            // the iteration in front of a factorisation the plan chose by itself (more than 512 nodes in a dimension, or no memory
            // for its tables): the factorisation alone -- fatal only where the iteration was asked for by name or is all there is
            if (splpak::opt_get("SPLPAK_DEBUG"))
                fprintf(stderr, "[splpak] the iteration could not be set up (status %d: %s): the factorisation alone\n", rc, g_err.c_str());
            p->pcg = nullptr;
            p->solver_mode = 0;
            (void)hipGetLastError();
            set_error("");
        } else if (rc != 0)
            return give_up(rc);
    }
    *plan = p;
    return 0;
}

static int unknown_option(const char *name) { set_error(std::string("unknown option: ") + (name ? name : "(null)")); return SPLPAK_E_BADARG; }

// s into the caller's buffer, cut to its length and always terminated (no buffer: nothing)
static void copy_out(char *buf, int32_t buflen, const char *s)
{
    if (!buf || buflen <= 0) return;
    std::strncpy(buf, s, (size_t)buflen - 1);
    buf[buflen - 1] = '\0';
}

extern "C" {

int64_t splpak_plan_comm_len(int32_t ndim, const int32_t *nodes)
{
    double xmin[MAXD] = {0, 0, 0, 0}, xmax[MAXD] = {1, 1, 1, 1};
    Grid g;
    if (!nodes || build_grid(ndim, nodes, xmin, xmax, g, nullptr) != 0) return -1;
    return comm_len_of(g, false);
}

int32_t splpak_plan_create(int32_t ndim, const int32_t *nodes, const double *xmin,
                           const double *xmax, double xtrap, int64_t max_ndata,
                           void *comm_buf_dev, int64_t comm_len, splpak_plan **plan)
{
    return plan_create_dist(ndim, nodes, xmin, xmax, xtrap, max_ndata, comm_buf_dev, comm_len, 1, 0, 1, plan, true);
}

void splpak_plan_destroy(splpak_plan *p)
{
    if (!p) return;
    if (p->fn_destroy) p->fn_destroy(p->fn_user);
    pcg_destroy(p->pcg);
    rowsop_destroy(p->rowsop);
    band_pipeline_destroy(p->band.pipe);
    for (hipEvent_t e : p->evStage) if (e) (void)hipEventDestroy(e);
    for (void *q : p->owned) (void)hipFree(q);
    std::free(p->ar_owned);
    delete p;
}

int32_t splpak_plan_set_allreduce_ex(splpak_plan *p, splpak_allreduce_fn fn, void *user, int32_t rank,
                                     int32_t world, int32_t flags)
{
    if (!p) { set_error("null plan"); return SPLPAK_E_BADARG; }
    p->ar = fn;
    p->ar_user = user;
    p->rank = rank;
    p->world = world < 1 ? 1 : world;
    p->ar_flags = flags;
    // (a failure here leaves the plan without usable job tables: it is remembered and every rank's next fit returns it
    //  through the first reduction's error flag -- round-3 advice: the status used to be dropped)
    p->setup_rc = nd_set_ranks(p, p->rank, p->world);
    return p->setup_rc;
}

void splpak_plan_set_allreduce(splpak_plan *p, splpak_allreduce_fn fn, void *user, int32_t rank,
                               int32_t world)
{
    // the hook of rounds 1-2: windows of the plan's communication buffer only -> the factorisation stays replicated
    (void)splpak_plan_set_allreduce_ex(p, fn, user, rank, world, 0);
}

void splpak_plan_set_refine(splpak_plan *p, int32_t max_steps, double tol)
{
    if (!p) return;
    p->max_refine = max_steps < 0 ? 0 : max_steps;
    p->max_refine_hard = p->max_refine == 0 ? 0 : (p->max_refine > 80 ? p->max_refine : 80);
    p->tol = tol;
}

void splpak_plan_enable_kernel_timing(splpak_plan *p, int32_t on)
{
    if (p) p->stats.enabled = on != 0;
}

void splpak_plan_kernel_timing(const splpak_plan *p, double *out7)
{
    if (!p || !out7) return;
    const CholStats &c = p->stats;
    const double v[7] = {c.syrk_launches, c.syrk_ms, c.syrk_flop, c.factor_ms, c.total_flop, c.bulk_launches, c.bulk_flop};
    for (int i = 0; i < 7; ++i) out7[i] = v[i];
}

void splpak_plan_stage_timing(const splpak_plan *p, double *out6)
{
    if (!p || !out6) return;
    for (int i = 0; i < 6; ++i) out6[i] = p->stage_ms[i];
}

int32_t splpak_set_default_option(const char *name, const char *value)
{
    return options_set_default(name, value) != 0 ? unknown_option(name) : 0;
}

int32_t splpak_plan_set_option(splpak_plan *p, const char *name, const char *value)
{
    if (!p) { set_error("null plan"); return SPLPAK_E_BADARG; }
    std::string canon;
    if (!option_canonical(name, canon)) return unknown_option(name);
    // what shapes the plan's storage and job tables was consumed when the plan was created
    static const char *const at_creation[] = {"SPLPAK_SOLVER", "SPLPAK_ND", "SPLPAK_ND_SPLIT", "SPLPAK_ND_CUT", "SPLPAK_ND_HALVES", "SPLPAK_ND_KB", "SPLPAK_ND_RES_CUS",
                                              "SPLPAK_NO_REORDER", "SPLPAK_GRAM_SCRATCH_MB", "SPLPAK_PCG_MAXIT", "SPLPAK_MPLAN_RCCL", "SPLPAK_RCCL_LIB"};
    for (const char *c : at_creation)
        if (canon == c) {
            set_error(canon + " shapes the plan and is read when it is created: set it with splpak_set_default_option (or the environment) before splpak_plan_create");
            return SPLPAK_E_UNSUPPORTED;
        }
    if (value) p->opt.kv[canon] = value; else p->opt.kv.erase(canon);
    return 0;
}

int32_t splpak_plan_get_option(const splpak_plan *p, const char *name, char *buf, int32_t buflen)
{
    if (!p) { set_error("null plan"); return SPLPAK_E_BADARG; }
    std::string canon;
    if (!option_canonical(name, canon)) return unknown_option(name);
    const char *v = p->opt.get(canon.c_str());
    copy_out(buf, buflen, v ? v : "");
    return v ? 1 : 0;
}

void splpak_plan_pcg_stats(const splpak_plan *p, double *out6)
{
    if (!out6) return;
    for (int i = 0; i < 6; ++i) out6[i] = 0.0;
    if (p && p->pcg) pcg_stats(p->pcg, out6);
}

const double *splpak_plan_hist_dev(const splpak_plan *p) { return p ? p->hist : nullptr; }

int64_t splpak_plan_device_bytes(const splpak_plan *p)
{
    if (!p) return 0;
    return (int64_t)(p->owned_bytes + (p->fn_bytes ? p->fn_bytes(p->fn_user) : 0) + pcg_bytes(p->pcg) + rowsop_bytes(p->rowsop));
}

int32_t splpak_plan_factorisation(const splpak_plan *p, char *buf, int32_t buflen)
{
    if (!p) return SPLPAK_E_BADARG;
    OptionsScope opt_scope(&p->opt);                  // (the narrow limit as the plan's fits see it)
    int code = 0;
    const char *what = "band Cholesky, four-stream look-ahead pipeline (csrc/bandchol.hip)";
    if (p->solver_mode == 2) { code = 6; what = "preconditioned conjugate gradients on the rows, separable preconditioner (csrc/pcg.hip); no factorisation"; }
    else if (p->fn_name) { code = p->fn_code; what = p->fn_name; }
    else if (p->dm.R > 1) { code = 3; what = "band Cholesky distributed over several GPUs by block columns (csrc/dist.hip)"; }
    else if (p->band.bw < narrow_band_limit()) { code = 1; what = "band Cholesky, narrow (chain-bound) form (csrc/bandchol.hip)"; }
    copy_out(buf, buflen, what);
    return code;
}

int32_t splpak_last_error_message(char *buf, int32_t buflen)
{
    copy_out(buf, buflen, g_err.c_str());
    return (int32_t)g_err.size();
}

int32_t splpak_device_name(char *buf, int32_t buflen)
{
    if (int r = device_ready()) return r;
    hipDeviceProp_t prop;
    int dev = 0;
    SPLPAK_HIP_TRY(hipGetDevice(&dev), SPLPAK_E_NODEVICE);
    SPLPAK_HIP_TRY(hipGetDeviceProperties(&prop, dev), SPLPAK_E_NODEVICE);
    copy_out(buf, buflen, prop.gcnArchName);
    return 0;
}

}  // extern "C"
