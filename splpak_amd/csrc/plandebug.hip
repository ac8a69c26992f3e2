// The debug entries of the C ABI (include/splpak_hip.h): one piece of a plan's fit alone, in the caller's (reference) column numbering --
// the assembled normal equations, the factorisation, the pass over the rows, the preconditioner --, the shape of the last Gram pass, and two
// that need no plan: the binning of a caller's points in the library's internal numbering, and the band Cholesky on a caller's matrix.
#include "plan.hpp"

#include <cstring>
#include <limits>

using namespace splpak;

// Where every entry of the plan's half stencil (internal dimension order, nst[i][code], code <= centre) lives in the half stencil
// of the caller's (reference) column numbering and dimension order: index into [ncol][hstencil], or -1 for a slot whose column lies
// outside the grid.  The two layouts hold the same entries of the symmetric N: an entry whose reference code lies above the centre
// is stored in the row of its column, at the mirrored offset.
static std::vector<long long> ref_stencil_map(const Grid &g)
{
    const int nd = g.ndim, hs = g.hstencil, centre = hs - 1;
    std::vector<long long> map((size_t)g.ncol * (size_t)hs, -1);
    int p7[MAXD];
    for (int d = 0, m = 1; d < MAXD; ++d, m *= 7) p7[d] = m;
    for (int i = 0; i < g.ncol; ++i) {
        int id[MAXD];
        long long iref = 0;
        for (int d = 0; d < nd; ++d) {
            id[d] = (i / g.colstride[d]) % g.nodes[d];
            iref += (long long)id[d] * g.refstride[d];
        }
        for (int c = 0; c < hs; ++c) {
            int cref = 0;
            long long jref = iref;
            bool in = true;
            for (int d = 0; d < nd; ++d) {
                const int o = (c / p7[d]) % 7 - 3;
                if (id[d] + o < 0 || id[d] + o >= g.nodes[d]) in = false;
                cref += (o + 3) * p7[g.perm[d]];
                jref += (long long)o * g.refstride[d];
            }
            if (!in) continue;
            map[(size_t)i * hs + c] = cref <= centre ? iref * hs + cref : jref * hs + (2 * centre - cref);
        }
    }
    return map;
}

static long long ref_column(const Grid &g, int i)
{
    long long r = 0;
    for (int d = 0; d < g.ndim; ++d) r += (long long)((i / g.colstride[d]) % g.nodes[d]) * g.refstride[d];
    return r;
}

extern "C" {

int32_t splpak_debug_plan_normal_equations(const splpak_plan *p, double *nst_ref, double *rhs)
{
    if (!p || !nst_ref || !rhs) { set_error("null argument"); return SPLPAK_E_BADARG; }
    if (p->rows_only || !p->nst) { set_error("the plan never assembles the normal equations (rows-only plan)"); return SPLPAK_E_UNSUPPORTED; }
    if (!p->ne_valid) {
        set_error("the plan's last fit did not assemble the normal equations (no fit yet, an iteration that answered without them, or a failure)");
        return SPLPAK_E_UNSUPPORTED;
    }
    if (int r = device_ready()) return r;
    const Grid &g = p->g;
    const size_t nst_n = (size_t)g.ncol * (size_t)g.hstencil;
    std::vector<double> h(nst_n), r((size_t)g.ncol);
    SPLPAK_HIP_TRY(hipMemcpy(h.data(), p->nst, sizeof(double) * nst_n, hipMemcpyDeviceToHost), SPLPAK_E_NODEVICE);
    SPLPAK_HIP_TRY(hipMemcpy(r.data(), p->rhs, sizeof(double) * (size_t)g.ncol, hipMemcpyDeviceToHost), SPLPAK_E_NODEVICE);
    const std::vector<long long> map = ref_stencil_map(g);
    std::memset(nst_ref, 0, sizeof(double) * nst_n);
    for (size_t t = 0; t < nst_n; ++t)
        if (map[t] >= 0) nst_ref[map[t]] = h[t];
    for (int i = 0; i < g.ncol; ++i) rhs[ref_column(g, i)] = r[(size_t)i];
    return 0;
}

int32_t splpak_debug_plan_solve(splpak_plan *p, const double *nst_ref, const double *b, double *x, double *minpiv)
{
    if (!p || !nst_ref || !b || !x) { set_error("null argument"); return SPLPAK_E_BADARG; }
    OptionsScope opt_scope(&p->opt);
    if (p->rows_only || !p->nst || p->solver_mode == 2 || !p->band.ab) { set_error("the plan has no factorisation"); return SPLPAK_E_UNSUPPORTED; }
    if (p->world > 1 || p->dm.R > 1) { set_error("not for a rank of a sharded or distributed fit"); return SPLPAK_E_UNSUPPORTED; }
    if (int r = device_ready()) return r;
    const Grid &g = p->g;
    const size_t nst_n = (size_t)g.ncol * (size_t)g.hstencil;
    const std::vector<long long> map = ref_stencil_map(g);
    std::vector<double> h(nst_n), v((size_t)p->band.npad, 0.0);
    for (size_t t = 0; t < nst_n; ++t) h[t] = map[t] >= 0 ? nst_ref[map[t]] : 0.0;
    for (int i = 0; i < g.ncol; ++i) v[(size_t)i] = b[ref_column(g, i)];
    hipStream_t st = nullptr;
    p->comm_failed = false;
    p->ne_valid = false;                  // (the half stencil now holds the caller's matrix)
    p->fit_valid = false;
    p->geom_valid = false;                // (and the factor storage its factor: nothing to refit)
    p->factor_valid = false;
    SPLPAK_HIP_TRY(hipMemcpy(p->nst, h.data(), sizeof(double) * nst_n, hipMemcpyHostToDevice), SPLPAK_E_NODEVICE);
    SPLPAK_HIP_TRY(hipMemcpy(p->xvec, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice), SPLPAK_E_NODEVICE);
    if (p->prefit_fn) SPLPAK_HIP_TRY(p->prefit_fn(p, st, p->fn_user), SPLPAK_E_NODEVICE);
    int hinfo = 0;
    double mp = 0.0;
    if (int r = plan_factor(p, st, &hinfo, &mp, nullptr, nullptr)) return r;
    if (minpiv) *minpiv = mp;
    if (hinfo != 0) {
        std::memset(x, 0, sizeof(double) * (size_t)g.ncol);
        set_error("normal equations not positive definite (suprls 34)");
        return 107;
    }
    if (int r = plan_factor_solve(p, p->xvec, st)) return r;
    SPLPAK_HIP_TRY(hipMemcpy(v.data(), p->xvec, sizeof(double) * (size_t)g.ncol, hipMemcpyDeviceToHost), SPLPAK_E_NODEVICE);
    for (int i = 0; i < g.ncol; ++i) x[ref_column(g, i)] = v[(size_t)i];
    return 0;
}

int32_t splpak_debug_plan_rows_gradient(splpak_plan *p, const double *coef, int32_t which, double *rho, double *den, double *ssq)
{
    if (!p || !coef || !rho || which < 0 || which > 2) { set_error("null argument, or `which` outside 0 .. 2"); return SPLPAK_E_BADARG; }
    OptionsScope opt_scope(&p->opt);
    if (p->world > 1 || p->dm.R > 1 || p->ar) { set_error("not for a rank of a sharded or distributed fit"); return SPLPAK_E_UNSUPPORTED; }
    if (!p->fit_valid) { set_error("the plan holds no rows: no completed fit (or a splpak_debug_plan_solve since)"); return SPLPAK_E_UNSUPPORTED; }
    if (int r = device_ready()) return r;
    const Grid &g = p->g;
    const Band &b = p->band;
    const bool smooth = p->xtrap != 0.0;
    hipStream_t st = nullptr;
    std::vector<double> v((size_t)b.npad, 0.0);
    for (int i = 0; i < g.ncol; ++i) v[(size_t)i] = coef[ref_column(g, i)];
    SPLPAK_HIP_TRY(hipMemcpy(p->xvec, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice), SPLPAK_E_NODEVICE);
    if (which == 1) {
        if (int r = plan_diagnostics_pass(p, p->fit_rows, st, nullptr)) return r;
    } else {
        SortScratch rows = p->s;
        if (which == 2) rows.ys = nullptr;              // the operator form of pcg_solve
        SPLPAK_HIP_TRY(hipMemsetAsync(p->rho, 0, sizeof(double) * (size_t)(b.npad + SC_COUNT), st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(plan_rows_residual(p, rows, p->xvec, smooth && p->rank == 0, p->rho, st), SPLPAK_E_NODEVICE);
    }
    SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
    SPLPAK_HIP_TRY(hipMemcpy(v.data(), p->rho, sizeof(double) * (size_t)g.ncol, hipMemcpyDeviceToHost), SPLPAK_E_NODEVICE);
    for (int i = 0; i < g.ncol; ++i) rho[ref_column(g, i)] = v[(size_t)i];
    if (den) {
        std::memset(den, 0, sizeof(double) * (size_t)g.ncol);
        if (which == 1) {
            SPLPAK_HIP_TRY(hipMemcpy(v.data(), p->tmp, sizeof(double) * (size_t)g.ncol, hipMemcpyDeviceToHost), SPLPAK_E_NODEVICE);
            for (int i = 0; i < g.ncol; ++i) den[ref_column(g, i)] = v[(size_t)i];
        }
    }
    if (ssq) {
        *ssq = 0.0;
        if (which == 1) SPLPAK_HIP_TRY(hipMemcpy(ssq, p->rho + b.npad, sizeof(double), hipMemcpyDeviceToHost), SPLPAK_E_NODEVICE);
    }
    return 0;
}

int32_t splpak_debug_plan_precondition(splpak_plan *p, int32_t part, const double *r, double *z)
{
    if (!p || !r || !z || part < 0 || part > 2) { set_error("null argument, or `part` outside 0 .. 2"); return SPLPAK_E_BADARG; }
    OptionsScope opt_scope(&p->opt);
    if (!p->pcg) { set_error("the plan has no iteration"); return SPLPAK_E_UNSUPPORTED; }
    if (!p->pcg_prepared) { set_error("the plan's last fit did not prepare the preconditioner (no fit yet, or one that went to the factorisation directly)"); return SPLPAK_E_UNSUPPORTED; }
    if (int rc = device_ready()) return rc;
    const Grid &g = p->g;
    std::vector<double> v((size_t)g.ncol), w((size_t)g.ncol);
    for (int i = 0; i < g.ncol; ++i) v[(size_t)i] = r[ref_column(g, i)];
    if (int rc = pcg_debug_precondition(p->pcg, part, v.data(), w.data())) return rc;
    for (int i = 0; i < g.ncol; ++i) z[ref_column(g, i)] = w[(size_t)i];
    return 0;
}

int32_t splpak_debug_plan_pcg_tables(const splpak_plan *p, int32_t dim, double *V, double *VT, int32_t *n_out)
{
    if (!p || !n_out) { set_error("null argument"); return SPLPAK_E_BADARG; }
    if (dim < 0 || dim >= p->g.ndim) { set_error("dimension outside the grid"); return SPLPAK_E_BADARG; }
    if (!p->pcg) { set_error("the plan has no iteration"); return SPLPAK_E_UNSUPPORTED; }
    int k = 0;
    while (p->g.perm[k] != dim) ++k;
    *n_out = p->g.nodes[k];
    if (!V && !VT) return 0;
    if (int rc = device_ready()) return rc;
    return pcg_debug_tables(p->pcg, k, V, VT);
}

int32_t splpak_debug_plan_pcg_diagonal(const splpak_plan *p, double *dinv)
{
    if (!p || !dinv) { set_error("null argument"); return SPLPAK_E_BADARG; }
    if (!p->pcg) { set_error("the plan has no iteration"); return SPLPAK_E_UNSUPPORTED; }
    if (!p->pcg_prepared) { set_error("the plan's last fit did not prepare the preconditioner"); return SPLPAK_E_UNSUPPORTED; }
    if (int rc = device_ready()) return rc;
    const Grid &g = p->g;
    std::vector<double> v((size_t)g.ncol);
    if (int rc = pcg_debug_diagonal(p->pcg, v.data())) return rc;
    for (int i = 0; i < g.ncol; ++i) dinv[ref_column(g, i)] = v[(size_t)i];
    return 0;
}

int32_t splpak_debug_plan_gram_shape(const splpak_plan *p, int32_t *out6)
{
    if (!p || !out6) { set_error("null argument"); return SPLPAK_E_BADARG; }
    if (!p->ne_valid || p->gshape.nslab < 1) {
        set_error("the plan's last fit did not assemble the normal equations: no Gram pass to describe");
        return SPLPAK_E_UNSUPPORTED;
    }
    const GramShape &s = p->gshape;
    const int v[6] = {s.nslab, s.rows, s.cells, s.run, s.last_cells, s.last_run};
    for (int i = 0; i < 6; ++i) out6[i] = v[i];
    return 0;
}

int32_t splpak_debug_bin_points(int32_t ndim, const int32_t *nodes, const double *xmin, const double *xmax, int64_t ndata,
                                const double *xdata, int32_t l1xdat, const double *ydata, const double *wdata, int32_t *perm,
                                int32_t *cells, int32_t *cellstride, int32_t *route, int32_t *cpt, int32_t *key, int32_t *offset,
                                int32_t *idx, double *xs, double *ys, double *ws, int64_t *placed, double *nrows_data)
{
    if (!nodes || !xmin || !xmax || !xdata || !ydata || !perm || !cells || !cellstride || !route || !cpt || !key || !offset || !idx ||
        !xs || !ys || !ws || !placed || !nrows_data) {
        set_error("null argument");
        return SPLPAK_E_BADARG;
    }
    if (ndata < 1 || ndata > (int64_t)std::numeric_limits<int32_t>::max() - 1024) { set_error("ndata outside 1 .. 2^31 - 1025"); return SPLPAK_E_BADARG; }
    Grid g;
    const int v = build_grid(ndim, nodes, xmin, xmax, g, nullptr, splpak::opt_get("SPLPAK_NO_REORDER") == nullptr);
    if (v != 0) {
        if (v == SPLPAK_E_UNSUPPORTED) set_error("ndim > 4 or more than 2^30 nodes is not supported");
        return v;
    }
    if (l1xdat < ndim) { set_error("l1xdat < ndim"); return SPLPAK_E_BADARG; }
    if (int r = device_ready()) return r;
    for (int d = 0; d < ndim; ++d) { perm[d] = g.perm[d]; cells[d] = g.cells[d]; cellstride[d] = g.cellstride[d]; }
    splpak_plan holder;
    SortScratch s{};
    double *dx = nullptr, *dy = nullptr, *dw = nullptr, *dscal = nullptr;
    const size_t m = (size_t)ndata;
    const bool ok = sort_scratch_alloc(&holder, g, ndata, &s) && dev_alloc(&holder, &dx, m * (size_t)l1xdat) && dev_alloc(&holder, &dy, m) &&
                    (!wdata || dev_alloc(&holder, &dw, m)) && dev_alloc(&holder, &dscal, (size_t)SC_COUNT);
    int rc = ok ? 0 : SPLPAK_E_NOMEM;
    if (ok) {
        *route = bin_route(g, s, cpt);
        double hscal[SC_COUNT];
        int np = 0;
        hipError_t e = hipMemcpy(dx, xdata, sizeof(double) * m * (size_t)l1xdat, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dy, ydata, sizeof(double) * m, hipMemcpyHostToDevice);
        if (e == hipSuccess && wdata) e = hipMemcpy(dw, wdata, sizeof(double) * m, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(dscal, 0, sizeof(double) * SC_COUNT);
        if (e == hipSuccess) e = launch_bin_points(g, ndata, dx, l1xdat, dy, dw, s, dscal, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e == hipSuccess) e = hipMemcpy(hscal, dscal, sizeof hscal, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(key, s.key, sizeof(int) * m, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(offset, s.offset, sizeof(int) * ((size_t)g.ncell + 1), hipMemcpyDeviceToHost);
        if (e == hipSuccess) np = offset[g.ncell];
        if (!hip_ok(e, "binning")) rc = SPLPAK_E_NODEVICE;
        else if (np < 0 || (int64_t)np > ndata) {
            set_error("the binning placed " + std::to_string(np) + " of " + std::to_string((long long)ndata) + " points");
            rc = SPLPAK_E_NODEVICE;
        } else {
            const size_t n = (size_t)np;
            e = hipMemcpy(idx, s.idx, sizeof(int) * n, hipMemcpyDeviceToHost);
            for (int d = 0; d < ndim && e == hipSuccess; ++d)
                e = hipMemcpy(xs + (size_t)d * m, s.xs + (size_t)d * (size_t)s.cap, sizeof(double) * n, hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(ys, s.ys, sizeof(double) * n, hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(ws, s.ws, sizeof(double) * n, hipMemcpyDeviceToHost);
            if (!hip_ok(e, "binning")) rc = SPLPAK_E_NODEVICE;
            *placed = np;
            *nrows_data = hscal[SC_NROWS_DATA];
        }
    }
    for (void *q : holder.owned) (void)hipFree(q);
    return rc;
}

int32_t splpak_debug_spd_band_solve_f64(int32_t n, int32_t halfbw, const double *a_lower,
                                        const double *bvec, double *x)
{
    if (n < 1 || halfbw < 0 || !a_lower || !bvec || !x) { set_error("bad argument"); return SPLPAK_E_BADARG; }
    if (int r = device_ready()) return r;
    if (splpak::opt_get("SPLPAK_DEBUG_TWOEND")) {          // the two-ended factorisation (twoend.hip) on the same input
        int hinfo = 0;
        const int rc = twoend_debug_solve(n, halfbw, a_lower, bvec, x, &hinfo);
        if (rc == 0) return hinfo != 0 ? 107 : 0;
        if (rc != 1) { set_error("two-ended band solve failed"); return rc; }
    }
    splpak_plan holder;
    Band b;
    band_bytes(n, halfbw, &b);
    double *dsmall = nullptr, *dx = nullptr, *dtmp = nullptr;
    int *dinfo = nullptr;
    bool ok = dev_alloc(&holder, &b.ab, b.bytes / sizeof(double)) &&
              band_alloc_inverses(&holder, b, (size_t)b.nblk, true) &&
              dev_alloc(&holder, &dsmall, 8) && dev_alloc(&holder, &dx, (size_t)b.npad) &&
              dev_alloc(&holder, &dtmp, (size_t)b.npad) && dev_alloc(&holder, &dinfo, 2);
    int rc = 0;
    if (!ok) rc = SPLPAK_E_NOMEM;
    if (ok) {
        std::vector<double> hb(b.bytes / sizeof(double), 0.0), hx((size_t)b.npad, 0.0);
        for (int j = 0; j < n; ++j)
            for (int i = j; i < n && i - j <= halfbw; ++i)
                hb[(size_t)i + (size_t)j * b.lda] = a_lower[(size_t)i + (size_t)j * n];
        for (int i = n; i < b.npad; ++i) hb[(size_t)i + (size_t)i * b.lda] = 1.0;
        for (int i = 0; i < n; ++i) hx[(size_t)i] = bvec[i];
        const double inf = std::numeric_limits<double>::infinity();
        hipError_t e = hipMemcpy(b.ab, hb.data(), b.bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dx, hx.data(), sizeof(double) * (size_t)b.npad, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dsmall + 2, &inf, sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(dinfo, 0, 2 * sizeof(int));
        if (e == hipSuccess) e = band_cholesky(b, dinfo, dsmall + 2, nullptr, nullptr);
        if (e == hipSuccess) e = band_solve(b, dx, dtmp, nullptr);
        int hinfo = 0;
        if (e == hipSuccess) e = hipMemcpy(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(hx.data(), dx, sizeof(double) * (size_t)b.npad, hipMemcpyDeviceToHost);
        if (!hip_ok(e, "band solve")) rc = SPLPAK_E_NODEVICE;
        else {
            for (int i = 0; i < n; ++i) x[i] = hx[(size_t)i];
            if (hinfo != 0) rc = 107;
        }
    }
    band_pipeline_destroy(b.pipe);
    for (void *q : holder.owned) (void)hipFree(q);
    return rc;
}

}  // extern "C"
