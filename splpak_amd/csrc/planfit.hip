// The fit and the refit on a plan (splpak_plan_fit_dev, splpak_plan_refit_dev): the assembly, the solve stage the two share, and
// the pieces of it that the debug-plan entries run alone (plan.hpp).
//
// The fit that the reference performs as "one dense row at a time through a dense
// Householder solver" (splcw :512-1060 -> suprls :1375-1695) is done here as
//   1. bin the points by 4-wide node window (counting sort),       binpoints.hip
//   2. per-window Gram blocks -> banded normal equations N, r,      gram.hip
//   3. derivative-constraint rows of data-sparse nodes -> N,        constraints.hip
//   4. blocked band Cholesky on the f64 matrix cores,               bandchol.hip
//   5. solve + iterative refinement with the residual recomputed FROM THE ROWS,
//      rho = A^T W (W y - W A x) - C^T C x, which brings the normal-equation
//      solution back to the accuracy of an orthogonal factorisation
//      (1e-13..2e-12 max-norm vs the reference).
// Multi-GPU: every rank runs 1-2 on its shard of the points; the
// histogram, then (N, r), then each refinement residual are sum-all-reduced
// through the caller's hook (RCCL via torch.distributed); 3 is applied by rank 0
// before the reduction so all ranks hold bit-identical normal equations; 4-5 are
// replicated.
#include "plan.hpp"

#include <cmath>
#include <cstdlib>
#include <limits>

using namespace splpak;

constexpr int REFIT_BATCH_MAX = nd::ND_BATCH_MAX;        // fields per sweep of a batched refit: the right-hand sides nd_solve_many carries

// SPLPAK_DEBUG_SUMS: sum and absolute sum of a device buffer, printed with a label (diagnosing the sharded fit)
static void debug_sum(const splpak_plan *p, const char *what, const double *buf, long long count, hipStream_t st)
{
    if (!splpak::opt_get("SPLPAK_DEBUG_SUMS")) return;
    std::vector<double> h((size_t)count);
    (void)hipStreamSynchronize(st);
    (void)hipMemcpy(h.data(), buf, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost);
    double s = 0.0, a = 0.0;
    for (double v : h) { s += v; a += std::fabs(v); }
    fprintf(stderr, "[splpak rank %d] %s: sum %.17g abs %.17g\n", p->rank, what, s, a);
}

int splpak::plan_allreduce(splpak_plan *p, double *buf, long long count, hipStream_t st)
{
    if (!p->ar || (p->world <= 1 && !(p->ar_flags & SPLPAK_AR_ALWAYS))) return 0;
    debug_sum(p, "before all-reduce", buf, count, st);
    // The buffer is complete before the hook sees it and the reduced values are in place before the fit goes on,
    // whatever the hook's own ordering is worth: the rehearsal of `bench.py --gpus 2` on ONE device over gloo summed
    // buffers the fit's kernels were still writing (round 3; a host synchronisation costs ~10 us, a fit issues
    // 3 + refinement steps of these)
    // (a hook that declares SPLPAK_AR_STREAM_ORDERED -- the native RCCL one: ncclAllReduce is enqueued on the stream it is
    //  handed -- is ordered with the fit's kernels by the stream itself: no host synchronisation on either side)
    const bool ordered = (p->ar_flags & SPLPAK_AR_STREAM_ORDERED) != 0;
    if (!ordered) SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
    const int r = p->ar(buf, count, (void *)st, p->ar_user);
    if (r != 0) { set_error("all-reduce callback failed"); p->comm_failed = true; return SPLPAK_E_COMM; }
    if (!ordered) SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
    debug_sum(p, "after  all-reduce", buf, count, st);
    return 0;
}

namespace splpak {

// a failure inside the factorisation / solve hooks: a communication failure is not a device fault (round-3 advice)
#define SPLPAK_HOOK_TRY(expr)                                                        \
    do {                                                                             \
        const hipError_t he_ = (expr);                                               \
        if (p->comm_failed) { (void)hipGetLastError(); return SPLPAK_E_COMM; }       \
        if (!::splpak::hip_ok(he_, #expr)) return SPLPAK_E_NODEVICE;                 \
    } while (0)

// The plan's factorisation of the half stencil in p->nst, as the fit runs it and as splpak_debug_plan_solve runs it alone:
// clear the pivot flag, expand into the factor storage, factor, read back the flag (0: positive definite) and the smallest
// pivot.  e0 / e1: events recorded around the expansion (NULL: none).
int plan_factor(splpak_plan *p, hipStream_t st, int *hinfo, double *minpiv, hipEvent_t e0, hipEvent_t e1)
{
    const double inf = std::numeric_limits<double>::infinity();
    SPLPAK_HIP_TRY(hipMemsetAsync(p->info, 0, 2 * sizeof(int), st), SPLPAK_E_NODEVICE);
    SPLPAK_HIP_TRY(hipMemcpyAsync(p->small + 2, &inf, sizeof(double), hipMemcpyHostToDevice, st), SPLPAK_E_NODEVICE);
    if (e0) (void)hipEventRecord(e0, st);
    SPLPAK_HIP_TRY(p->expand_fn ? p->expand_fn(p, st, p->fn_user) : launch_expand(p->g, p->nst, p->band, p->dm, st), SPLPAK_E_NODEVICE);
    if (e1) (void)hipEventRecord(e1, st);
    SPLPAK_HOOK_TRY(p->factor_fn ? p->factor_fn(p, p->info, p->small + 2, st, p->fn_user) : band_cholesky(p->band, p->info, p->small + 2, st, &p->stats));
    *hinfo = 0;
    *minpiv = 0.0;
    SPLPAK_HIP_TRY(hipMemcpyAsync(hinfo, p->info, sizeof(int), hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
    SPLPAK_HIP_TRY(hipMemcpyAsync(minpiv, p->small + 2, sizeof(double), hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
    SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
    return 0;
}

// v <- N^-1 v with the factor plan_factor left (v: b.npad doubles, internal order, zero padding)
int plan_factor_solve(splpak_plan *p, double *v, hipStream_t st)
{
    SPLPAK_HOOK_TRY(p->solve_fn ? p->solve_fn(p, v, p->tmp, st, p->fn_user) : band_solve(p->band, v, p->tmp, st));
    return 0;
}

// The pass over the rows a fit ends with, at the coefficients in p->xvec (internal order), as the fit runs it and as
// splpak_debug_plan_rows_gradient runs it alone: the backward error's denominators into p->tmp, then rho into p->rho and the sum of
// squared row residuals behind it (p->rho + npad).  rows_fit: the normal equations of this fit are not assembled.  e0: recorded
// before the residual pass (NULL: none).
int plan_diagnostics_pass(splpak_plan *p, bool rows_fit, hipStream_t st, hipEvent_t e0)
{
    const Grid &g = p->g;
    const Band &b = p->band;
    const bool smooth = p->xtrap != 0.0;
    double *scalR = p->rho + b.npad;
    // the backward error's denominators (|N| |x| + |rhs|: a pass over the half stencil) need the coefficients only; into the
    // solves' scratch vector.  (On a stream of their own beside the residual pass they gained nothing -- the two kernels
    // slowed each other down by what the overlap saved -- and one more stream per plan is not free: round 5)
    if (rows_fit) {
        // from the rows: |A|^T W^2 |A| |x| + |C|^T |C| |x| + |rhs| (this rank's points; the residual's all-reduce below does not
        // carry it -- a sharded rows-only fit normalises by its own shard's terms + the constraint rows on rank 0, a lower bound
        // of the sum, i.e. a pessimistic backward error)
        SPLPAK_HIP_TRY(rowsop_backward_denominators(g, p->rowsop, p->s, p->xvec, p->rhs, p->dcw, p->spf, p->ctab, smooth && p->rank == 0,
                                                    pcg_scratch(p->pcg, 0), pcg_scratch(p->pcg, 1), p->tmp, st), SPLPAK_E_NODEVICE);
    } else
        SPLPAK_HIP_TRY(launch_backward_denominators(g, p->nst, p->xvec, p->rhs, p->tmp, st), SPLPAK_E_NODEVICE);
    SPLPAK_HIP_TRY(hipMemsetAsync(p->rho, 0, sizeof(double) * (size_t)(b.npad + SC_COUNT), st), SPLPAK_E_NODEVICE);
    if (e0) (void)hipEventRecord(e0, st);
    if (p->rowsop && (!p->rcell || !splpak::opt_get("SPLPAK_RESIDUAL_CELLS")))      // (4-D: tile by tile, as the refinement's passes; 8.3 -> 1 ms at 32^4)
        SPLPAK_HIP_TRY(rowsop_residual(g, p->rowsop, p->s, p->xvec, p->dcw, p->spf, p->ctab, smooth && p->rank == 0, p->rho, scalR, p->e2buf, st),
                       SPLPAK_E_NODEVICE);
    else if (p->rows3.partial && (!p->rcell || !splpak::opt_get("SPLPAK_RESIDUAL_CELLS")))      // (3-D: the data rows tile by tile, likewise)
        SPLPAK_HIP_TRY(rows3_residual(g, p->rows3, p->s, p->xvec, p->dcw, p->spf, p->ctab, smooth && p->rank == 0, p->tbuf, p->rho, scalR,
                                      p->e2buf, st), SPLPAK_E_NODEVICE);
    else
        SPLPAK_HIP_TRY(launch_residual(g, p->s, p->xvec, p->rcell, p->dcw, p->spf, p->ctab, smooth && p->rank == 0,
                                       p->tbuf, p->rho, scalR, p->e2buf, st), SPLPAK_E_NODEVICE);
    return 0;
}

}  // namespace splpak

// kernel timing (splpak_plan_enable_kernel_timing): the stage events exist before the first stamp; stamp i on the fit's stream
static int plan_stage_events(splpak_plan *p)
{
    if (p->stats.enabled)
        for (hipEvent_t &e : p->evStage)
            if (!e) SPLPAK_HIP_TRY(hipEventCreate(&e), SPLPAK_E_NODEVICE);
    return 0;
}
static void stamp(splpak_plan *p, int i, hipStream_t st) { if (p->stats.enabled) (void)hipEventRecord(p->evStage[i], st); }

// A fit that ends as the reference's suprls failures do: zero coefficients, the message, 107 (:1053-1058)
static int fit_fails_107(const Grid &g, double *coef_dev, hipStream_t st, const char *msg)
{
    SPLPAK_HIP_TRY(hipMemsetAsync(coef_dev, 0, sizeof(double) * (size_t)g.ncol, st), SPLPAK_E_NODEVICE);
    SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
    set_error(msg);
    return 107;
}

// A 4-D plan with the iteration in front of a factorisation leaves the normal equations unassembled until the factorisation
// is going to need them (see splpak_plan_fit_dev); read under the plan's options
static bool plan_lazy_assembly(const splpak_plan *p)
{
    return !p->rows_only && p->pcg && p->solver_mode == 3 && p->rowsop && p->xtrap != 0.0 && p->world <= 1 && !p->ar &&
           pcg_boxes_from_rows(p->pcg) && !splpak::opt_get("SPLPAK_PCG_EAGER");
}

// The assembly a lazy fit left out: everything the eager order would have written; same kernels, same bits (the caller clears its rows_fit)
static int plan_assemble_lazy(splpak_plan *p, hipStream_t st)
{
    const Grid &g = p->g;
    const bool smooth = p->xtrap != 0.0;
    SPLPAK_HIP_TRY(hipMemsetAsync(p->comm, 0, sizeof(double) * (size_t)(p->lenG + p->lenH), st), SPLPAK_E_NODEVICE);
    SPLPAK_HIP_TRY(launch_gram(g, p->s, p->gscratch, p->gscratch_doubles, smooth, p->nst, p->rhs, p->hist, p->scalH, st, &p->gshape), SPLPAK_E_NODEVICE);
    // (the weights of the constraint rows again, from THIS histogram: the rows' one differs from it in the last bits)
    SPLPAK_HIP_TRY(launch_sparse_mark(g, p->hist, p->scalH, p->xtrap, p->dcw, p->spf, st), SPLPAK_E_NODEVICE);
    SPLPAK_HIP_TRY(launch_constraint_rows(g, p->dcw, p->spf, p->ctab, p->nst, p->scalG, st), SPLPAK_E_NODEVICE);
    p->fit_rows = false;                           // (here, not only on success: a refit after a 107 must not assemble again)
    p->ne_valid = true;
    p->factor_valid = false;                       // (the Gram scratch may be the factor storage)
    return 0;
}

// What the solve of a fit starts from: left by the assembly of splpak_plan_fit_dev, or taken from the plan by a refit
struct SolveStart {
    double rows_cons = 0, sumw2 = 0;
    bool rows_fit = false;        // the normal equations are not assembled (a rows-only plan, or a lazy one so far)
    bool refit = false;           // new values on the last fit's points: the solver follows what that fit left in the plan
    std::chrono::steady_clock::time_point t1;      // the end of the assembly (refit: the start of the field)
};

// Where a solve with refinement stands.  converged: the (estimated) remaining error is below tol, or the corrections sit at the
// rounding floor; diverged: they stopped contracting while still large.  A solve that is still contracting after the nominal number
// of steps goes on up to max_refine_hard; if even that leaves an estimated error above the parity bar the fit is reported as failed
// (107) instead of returning coefficients that silently miss it.
struct Refinement {
    int steps = 0;
    double last_rel = 0.0, ratio = 0.0;
    bool converged = false, diverged = false, stagnated = false;
    // estimated error left after the last step (exact 0 when it met the tolerance outright)
    double est_err() const { return steps >= 2 && ratio > 0.0 && ratio < 1.0 ? last_rel * ratio / (1.0 - ratio) : last_rel; }
};

// One step of the refinement's stopping rules, for the step `it` whose correction measured am = (max |dx|, max |x|): counts it,
// and decides.  true: the solve ends here (rf says how); false: it goes on, prev_rel carried to the next step.  Shared by the
// solve of one field (solve_and_refine) and the lock-step solve of several (refit_chunk_batched): the same rules, field by field.
static bool refinement_advance(const splpak_plan *p, Refinement &rf, double &prev_rel, int it, const double am[2])
{
    ++rf.steps;
    rf.last_rel = (am[1] > 0.0) ? am[0] / am[1] : 0.0;
    if (am[0] != am[0] || am[1] != am[1]) rf.last_rel = std::numeric_limits<double>::quiet_NaN();      // (NaN > 0 is false: not "no correction")
    if (splpak::opt_get("SPLPAK_DEBUG"))
        fprintf(stderr, "[splpak] refinement step %d: |dx|/|x| = %.3e\n", rf.steps, rf.last_rel);
    if (!(rf.last_rel == rf.last_rel)) return true;             // NaN
    if (rf.last_rel <= p->tol) { rf.converged = true; return true; }
    if (it >= 1) {
        // linear convergence: after this step the error is ~ dx * ratio / (1 - ratio); stop as soon
        // as that estimate is below the tolerance instead of paying for one more solve
        rf.ratio = rf.last_rel / prev_rel;
        if (rf.ratio < 0.9 && rf.last_rel * rf.ratio / (1.0 - rf.ratio) <= p->tol) { rf.converged = true; return true; }
        if (rf.ratio >= 0.9) {                                // stagnation: fine at the rounding floor, a failure if the
            rf.diverged = rf.last_rel > 1e-8;                 // corrections are still large; in between (1e-10 .. 1e-8) the
            rf.converged = !rf.diverged;                      // MEASURED backward error decides below (round-2 advice: the
            rf.stagnated = rf.converged && rf.last_rel > 1e-10;   // estimate alone let coefficients that miss the bar through)
            return true;
        }
        // 0.5 .. 0.9: an ill-conditioned grid whose corrections still shrink -- go on (up to max_refine_hard):
        // stopping here left 1-D grids of 2 000-3 000 nodes 1e-7 .. 1e-10 away from the converged solution
        // (randomized sweep, tools/fuzz_parity.py big)
    }
    prev_rel = rf.last_rel;
    if (it + 1 >= p->max_refine && it + 1 < p->max_refine_hard && splpak::opt_get("SPLPAK_DEBUG"))
        fprintf(stderr, "[splpak] still contracting after %d steps: continuing\n", it + 1);
    return false;
}

// Solve + refinement against the rows, around any solver of N z = v, from the right-hand side in p->rhs to the coefficients in
// p->xvec.  solve(v, first): v <- N^-1 v; 0, a status to return (negative, SPLPAK_E_COMM), or 1 = this solver gives up (the iteration)
template <typename Solve>
static int solve_and_refine(splpak_plan *p, hipStream_t st, Refinement &rf, Solve &&solve)
{
    const Grid &g = p->g;
    const Band &b = p->band;
    const bool smooth = p->xtrap != 0.0;                              // swght, :769
    rf = Refinement();
    rf.converged = p->max_refine == 0;
    double prev_rel = std::numeric_limits<double>::infinity();
    SPLPAK_HIP_TRY(hipMemsetAsync(p->xvec, 0, sizeof(double) * (size_t)b.npad, st), SPLPAK_E_NODEVICE);
    SPLPAK_HIP_TRY(hipMemcpyAsync(p->xvec, p->rhs, sizeof(double) * (size_t)g.ncol, hipMemcpyDeviceToDevice, st), SPLPAK_E_NODEVICE);
    stamp(p, 6, st);
    if (int r = solve(p->xvec, true)) return r;
    stamp(p, 7, st);
    for (int it = 0; it < p->max_refine_hard && !rf.converged; ++it) {
        // (the scalars behind rho travel with it through the all-reduce: zeroed too, or every collective doubles them)
        SPLPAK_HIP_TRY(hipMemsetAsync(p->rho, 0, sizeof(double) * (size_t)(b.npad + SC_COUNT), st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(plan_rows_residual(p, p->s, p->xvec, smooth && p->rank == 0, p->rho, st), SPLPAK_E_NODEVICE);
        if (int r = plan_allreduce(p, p->rho, p->lenR, st)) return r;
        if (int r = solve(p->rho, false)) return r;
        SPLPAK_HIP_TRY(launch_axpy_absmax(g.ncol, p->xvec, p->rho, p->small, st), SPLPAK_E_NODEVICE);
        double am[2];
        SPLPAK_HIP_TRY(hipMemcpyAsync(am, p->small, 2 * sizeof(double), hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
        if (refinement_advance(p, rf, prev_rel, it, am)) break;
    }
    return 0;
}

// Where a factorisation stands behind the iteration, the attempt is skipped in the regime in which it is known to stagnate or
// crawl (between 0 and ~1.6 constraint rows per column; it works with none and from ~1.7 on)
static bool iteration_worth_trying(const splpak_plan *p, double rows_cons)
{
    if (p->solver_mode != 3 || splpak::opt_get("SPLPAK_PCG_ALWAYS")) return true;
    const double rpc = rows_cons / (double)p->g.ncol;
    // (a factorisation of seconds -- 24^4: 4.5 s, 28^4: 18 s -- is worth a patient attempt where the iteration only crawls: 24^4 at
    //  1.5 / 1.4 / 1.33 rows per column 1.0 / 2.1 / 3.1 s; at 1.27 it gives up after 2.8 s.  45 TFLOP/s: what the factorisation sustains)
    const double fac_s = p->factor_flop / 45.0e12;
    const double lo = fac_s >= 10.0 ? 1.3 : (fac_s >= 1.0 ? 1.35 : 1.6);
    if (!(rows_cons > 0.0 && rpc < lo)) return true;
    if (splpak::opt_get("SPLPAK_DEBUG")) fprintf(stderr, "[splpak] %.2f constraint rows per column: the factorisation without an attempt of the iteration\n", rpc);
    return false;
}

// The iteration (pcg.hip) as the solver: a fit prepares the preconditioner first, a refit solves on the prepared one.  0 with
// `solved` set = it answered (rf: how), or not -- the factorisation is to take over --; else the status the fit returns, 107 included
// where the plan has no factorisation to turn to.
static int plan_iterate(splpak_plan *p, hipStream_t st, double *coef_dev, double *info, const SolveStart &a, bool rows_fit,
                        Refinement &rf, bool &solved)
{
    const bool smooth = p->xtrap != 0.0;
    if (a.refit) pcg_restart_counts(p->pcg);
    else {
        SPLPAK_HIP_TRY(pcg_prepare(p, p->pcg, a.sumw2, smooth, rows_fit, st), SPLPAK_E_NODEVICE);
        p->pcg_prepared = true;
        if (pcg_singular(p->pcg)) {
            // A box taken out of the ASSEMBLED normal equations -- a principal submatrix of N -- is not positive definite by the pivot
            // test of the factorisations: neither is N (a column without data and, with xtrap = 0, without a constraint row; the
            // reference's "system is singular", suprls 34 -> 107).  The iteration would still run to a minimiser with arbitrary
            // values on what the rows do not see: the factorisation gets to say 107, or the plan that has none says it here
            // (randomised sweep tools/pcg/fuzz_pcg.py: 1-D, 150 nodes, 361 points, xtrap = 0)
            if (p->solver_mode != 2) return 0;
            return fit_fails_107(p->g, coef_dev, st, "normal equations not positive definite (suprls 34): a block of them failed the pivot test");
        }
    }
    const double tol_first = splpak::opt_get("SPLPAK_PCG_TOL1") ? atof(splpak::opt_get("SPLPAK_PCG_TOL1")) : 1e-11;
    const double tol_next = splpak::opt_get("SPLPAK_PCG_TOL2") ? atof(splpak::opt_get("SPLPAK_PCG_TOL2")) : 1e-3;
    const int r = solve_and_refine(p, st, rf, [=](double *v, bool first) -> int { return pcg_solve(p, p->pcg, v, first ? tol_first : tol_next, smooth, st); });
    if (r != 0 && r != 1) return r;
    solved = r == 0 && rf.last_rel == rf.last_rel && !rf.diverged && (rf.converged || rf.est_err() <= 1e-10);
    if (!solved && p->solver_mode == 2) {
        double ps[6];
        pcg_stats(p->pcg, ps);
        char buf[320];
        snprintf(buf, sizeof buf, "the iterative solve did not converge (%.0f iterations in %.0f solves, last preconditioned residual %.1e, last correction %.1e) "
                 "and no factorisation of this grid fits the device: data too clustered for the separable preconditioner", ps[0], ps[1], ps[3], rf.last_rel);
        const int rc = fit_fails_107(p->g, coef_dev, st, buf);
        if (rc == 107 && info) { info[2] = rf.steps; info[3] = rf.last_rel; }
        return rc;
    }
    if (!solved && splpak::opt_get("SPLPAK_DEBUG")) fprintf(stderr, "[splpak] the iteration gave up: factorisation instead\n");
    return 0;
}

// Kernel timing: this fit's stage times from the stage events (the stream has been synchronised; the residual pass is timed where it runs)
static void plan_stage_times(splpak_plan *p, bool refit, bool factored)
{
    const int pairs[5][2] = {{0, 1}, {1, 2}, {2, 3}, {4, 5}, {6, 7}};
    const int slot[5] = {0, 1, 2, 3, 5};
    for (int i = 0; i < 5; ++i) {
        float ms = 0.f;
        // (a refit records the values gather + right-hand side as stage 1 and bins nothing; it expands only when it factors)
        if (refit && (slot[i] == 0 || slot[i] == 2 || (slot[i] == 3 && !factored))) p->stage_ms[slot[i]] = 0.0;
        else if (hipEventElapsedTime(&ms, p->evStage[pairs[i][0]], p->evStage[pairs[i][1]]) == hipSuccess) p->stage_ms[slot[i]] = ms;
        else (void)hipGetLastError();
    }
}

// The part of a fit that depends on the values: the solve of N z = A^T W^2 y -- by the iteration where the plan has it, by the
// factorisation otherwise or when the iteration gives up (a lazy plan assembles N first) --, the refinement against the rows, the
// diagnostics pass and the decisions that end in 107.  p->rhs holds the right-hand side, p->s the binned points.  A refit
// (a.refit) solves with what the last fit left: the held factor without factoring again, else the iteration on the prepared
// preconditioner, and the factorisation -- from the binned points, as the fit runs it -- when that gives up.
static int plan_solve_stage(splpak_plan *p, hipStream_t st, double *coef_dev, double *info, const SolveStart &a)
{
    const Grid &g = p->g;
    using clk = std::chrono::steady_clock;
    const bool stamps = p->stats.enabled;
    const bool lazy = plan_lazy_assembly(p);       // the normal equations are assembled only if the factorisation is going to run
    bool rows_fit = a.rows_fit;
    Refinement rf;

    // ---- decide: a refit takes the held factor, else the iteration if it answered the fit (its preconditioner is prepared)
    const bool held_factor = a.refit && p->factor_valid;
    const bool try_iteration = p->pcg && (a.refit ? !held_factor && p->pcg_prepared : iteration_worth_trying(p, a.rows_cons));
    if (lazy && rows_fit && !try_iteration && !held_factor) {
        if (int r = plan_assemble_lazy(p, st)) return r;
        rows_fit = false;
    }

    // ---- the iteration (pcg.hip), where the plan has it --------------------
    bool solved = false;
    if (try_iteration)
        if (int r = plan_iterate(p, st, coef_dev, info, a, rows_fit, rf, solved)) return r;

    // ---- factorisation, or the held factor; solve + refinement with it -----
    const bool factored = !held_factor && !solved;
    auto t2 = a.t1;
    if (held_factor) {
        if (info) info[4] = p->fit_minpiv;
    } else if (!solved) {
        if (lazy && rows_fit) {
            if (int r = plan_assemble_lazy(p, st)) return r;
            rows_fit = false;
        }
        int hinfo = 0;
        double minpiv = 0.0;
        p->factor_valid = false;
        if (int r = plan_factor(p, st, &hinfo, &minpiv, stamps ? p->evStage[4] : nullptr, stamps ? p->evStage[5] : nullptr)) return r;
        t2 = clk::now();
        if (info) {
            info[4] = minpiv;
            info[6] = std::chrono::duration<double>(t2 - a.t1).count();
        }
        p->factor_valid = hinfo == 0 && p->world <= 1 && !p->ar && p->dm.R == 1;
        p->fit_minpiv = minpiv;
        // not positive definite: the reference's "system is singular" (suprls 34 -> 107)
        if (hinfo != 0) return fit_fails_107(g, coef_dev, st, "normal equations not positive definite (suprls 34)");
    }
    if (!solved)
        if (int r = solve_and_refine(p, st, rf, [=](double *v, bool) -> int {
                if (a.refit) { ++p->rb.stats[1]; ++p->rb.stats[2]; }       // (splpak_debug_plan_refit_stats)
                return plan_factor_solve(p, v, st);
            })) return r;
    const double est_err = rf.est_err();
    const bool unconverged = !rf.converged && !rf.diverged && rf.last_rel == rf.last_rel && est_err > 1e-10;
    SPLPAK_HIP_TRY(launch_to_reference_order(g, p->xvec, coef_dev, st), SPLPAK_E_NODEVICE);   // internal -> caller's dimension order

    // ---- diagnostics: one more pass over the rows at the returned coefficients
    //  * residual norm ||rows * coef - rhs||_2 over data AND constraint rows: what the reference computes
    //    as `reserr` (suprls :1693) and then drops (splcw :690, :1052)
    //  * optimality residual: the gradient rho = A^T W (W y - W A x) - C^T C x of the least-squares functional,
    //    recomputed from the rows, as a componentwise backward error max_i |rho_i| / ((|N||x|)_i + |A^T W^2 y|_i)
    //    -- 0 at the minimiser the reference computes; a MEASURED statement about the returned
    //    coefficients (the refinement's stopping rule is an estimate)
    double ssq = 0.0, omega = 0.0;
    if (info || rf.stagnated) {
        hipEvent_t r0 = stamps ? p->evStage[8] : nullptr, r1 = stamps ? p->evStage[9] : nullptr;   // (created with the other stage events)
        if (int r = plan_diagnostics_pass(p, rows_fit, st, r0 && r1 ? r0 : nullptr)) return r;
        if (r0 && r1) {
            (void)hipEventRecord(r1, st);
            (void)hipEventSynchronize(r1);
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, r0, r1) == hipSuccess) p->stage_ms[4] = ms;
        }
        if (int r = plan_allreduce(p, p->rho, p->lenR, st)) return r;
        SPLPAK_HIP_TRY(launch_backward_error(g, p->tmp, p->rho, p->small + 3, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipMemcpyAsync(&ssq, p->rho + p->band.npad, sizeof(double), hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipMemcpyAsync(&omega, p->small + 3, sizeof(double), hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
    }
    SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
    auto t3 = clk::now();
    if (stamps) plan_stage_times(p, a.refit, factored);
    if (info) {
        info[2] = rf.steps;
        info[3] = rf.last_rel;
        info[7] = std::chrono::duration<double>(t3 - t2).count();
        info[8] = std::sqrt(ssq);
        info[9] = omega;
    }

    // ---- verdict: a correction that is still large means the factor did not precondition the problem
    // (numerically singular normal equations): the reference's "suprls failure"
    if (!(rf.last_rel == rf.last_rel) || rf.diverged) {
        set_error("iterative refinement diverged: numerically singular normal equations");
        return 107;
    }
    char buf[200];
    if (rf.stagnated && !(omega <= 1e-10)) {
        snprintf(buf, sizeof buf, "iterative refinement stagnated at corrections of %.2e with a backward error of %.1e > 1e-10", rf.last_rel, omega);
        set_error(buf);
        return 107;
    }
    if (unconverged) {
        snprintf(buf, sizeof buf, "iterative refinement did not converge in %d steps: last correction %.2e, contraction %.2f, "
                 "estimated error %.1e > 1e-10", rf.steps, rf.last_rel, rf.ratio, est_err);
        set_error(buf);
        return 107;
    }
    p->fit_valid = p->world <= 1 && !p->ar && p->dm.R == 1;
    p->fit_rows = rows_fit;
    return 0;
}

// The arguments of one splpak_plan_refit_dev
struct RefitCall {
    int nfields;
    const double *ydata_dev;
    long long ldy;
    double *coef_dev;
    long long ldcoef;
    double *info;
    const double *y(int k) const { return ydata_dev + (size_t)k * (size_t)ldy; }
    double *coef(int k) const { return coef_dev + (size_t)k * (size_t)ldcoef; }
    double *inf(int k) const { return info ? info + 10 * (size_t)k : nullptr; }
};

// The fields [k0, k1) of a refit one after another, each through the solve stage of a fit.  0, or the status the call returns:
// negative at once; 107 with the failing field's coefficients, every later field of the CALL zeroed and the plan still refit-able
static int refit_field_by_field(splpak_plan *p, const RefitCall &c, int k0, int k1, hipStream_t st)
{
    const Grid &g = p->g;
    const long long ndata = p->fit_ndata;
    for (int k = k0; k < k1; ++k) {
        double *inf = c.inf(k);
        if (inf) for (int i = 0; i < 10; ++i) inf[i] = 0.0;
        // the values and the right-hand side are being replaced: until the field is through, the plan describes no fit
        p->fit_valid = false;
        p->geom_valid = false;
        SolveStart a;
        a.rows_cons = p->fit_rows_cons;
        a.sumw2 = p->fit_sumw2;
        a.rows_fit = p->fit_rows;
        a.refit = true;
        a.t1 = std::chrono::steady_clock::now();
        stamp(p, 1, st);
        SPLPAK_HIP_TRY(launch_regather_values(g, p->s, ndata, c.y(k), p->s.ys, st), SPLPAK_E_NODEVICE);
        // A^T W^2 y: the refinement's pass over the rows at x = 0, without the constraint rows
        SPLPAK_HIP_TRY(hipMemsetAsync(p->xvec, 0, sizeof(double) * (size_t)p->band.npad, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipMemsetAsync(p->rhs, 0, sizeof(double) * (size_t)g.ncol, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(plan_rows_residual(p, p->s, p->xvec, false, p->rhs, st), SPLPAK_E_NODEVICE);
        stamp(p, 2, st);
        if (inf) { inf[0] = p->fit_rows_data; inf[1] = p->fit_rows_cons; }
        const int rc = plan_solve_stage(p, st, c.coef(k), inf, a);
        if (rc < 0) return rc;
        p->geom_valid = true;                  // (107 too: the points, N and the factor or preconditioner are those of the fit still)
        if (rc != 0) {
            for (int j = k + 1; j < c.nfields; ++j)
                SPLPAK_HIP_TRY(hipMemsetAsync(c.coef(j), 0, sizeof(double) * (size_t)g.ncol, st), SPLPAK_E_NODEVICE);
            SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
            return rc;
        }
    }
    return 0;
}

// Option refit_batch: fields per sweep of a batched refit, 1 .. 8 (clamped; default, and text that is no number: 8; 1: field by field)
static int refit_batch_option()
{
    const char *e = splpak::opt_get("SPLPAK_REFIT_BATCH");
    if (!e) return REFIT_BATCH_MAX;
    char *end = nullptr;
    const long v = std::strtol(e, &end, 10);
    while (end && (*end == ' ' || *end == '\t')) ++end;
    if (end == e || (end && *end)) return REFIT_BATCH_MAX;
    return v < 1 ? 1 : (v > REFIT_BATCH_MAX ? REFIT_BATCH_MAX : (int)v);
}

// doubles between the per-field copies of ys, and of the vectors (multiples of 32: every copy as aligned as the plan's own)
static size_t refit_ystride(const splpak_plan *p) { return ((size_t)p->s.cap + 31) / 32 * 32; }
static size_t refit_vstride(const splpak_plan *p) { return ((size_t)p->band.npad + SC_COUNT + 31) / 32 * 32; }

// The per-field copies a batched refit works in: REFIT_BATCH_MAX x (ys | xvec | rhs | rho) and the pairs of the corrections,
// allocated at the first batched refit and counted in splpak_plan_device_bytes.  No memory for them is no error: it is asked
// for once, and the plan refits field by field from then on.
static bool refit_buffers_ready(splpak_plan *p)
{
    splpak_plan::RefitBatch &rb = p->rb;
    if (rb.ys || rb.tried) return rb.ys != nullptr;
    rb.tried = true;
    const size_t sy = refit_ystride(p), sv = refit_vstride(p);
    const size_t bytes = sizeof(double) * ((size_t)REFIT_BATCH_MAX * (sy + 3 * sv) + 32);
    void *q = nullptr;
    if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
    p->owned.push_back(q);
    p->owned_bytes += bytes;
    rb.ys = static_cast<double *>(q);
    rb.x = rb.ys + (size_t)REFIT_BATCH_MAX * sy;
    rb.rhs = rb.x + (size_t)REFIT_BATCH_MAX * sv;
    rb.rho = rb.rhs + (size_t)REFIT_BATCH_MAX * sv;
    rb.small = rb.rho + (size_t)REFIT_BATCH_MAX * sv;
    return true;
}

// The fields [k0, k0 + n) of a refit, 2 <= n <= REFIT_BATCH_MAX, in lock-step on the held nested-dissection factor: every field has
// its own values, right-hand side, coefficients and residual; the row passes run field after field as the single refit launches
// them, and every solve is ONE sweep of the factor over the fields that are still refining (nd_solve_many).  A field leaves the
// sweeps when the rules of solve_and_refine end its solve, so every field gets the operations -- and the bits -- of its own
// single-field refit, info[0..4], [8], [9] included; info[7] is the chunk's share per field, [5] and [6] are 0.
// *redo: a field did not end in status 0 -- nothing of the chunk is reported, the caller runs it field by field.
// Returns 0 or a negative status.  After a chunk without redo the plan describes its last field.
static int refit_chunk_batched(splpak_plan *p, const RefitCall &c, int k0, int n, hipStream_t st, bool *redo)
{
    using clk = std::chrono::steady_clock;
    const Grid &g = p->g;
    const Band &b = p->band;
    const bool smooth = p->xtrap != 0.0;
    const bool stamps = p->stats.enabled;
    const long long ndata = p->fit_ndata;
    const size_t sy = refit_ystride(p), sv = refit_vstride(p), vbytes = sizeof(double) * (size_t)b.npad, cbytes = sizeof(double) * (size_t)g.ncol;
    splpak_plan::RefitBatch &rb = p->rb;
    struct KeepYs {                         // the diagnostics pass reads the values through p->s
        splpak_plan *p;
        double *ys;
        ~KeepYs() { p->s.ys = ys; }
    } keep{p, p->s.ys};
    SortScratch rows[REFIT_BATCH_MAX];
    double *x[REFIT_BATCH_MAX], *rhs[REFIT_BATCH_MAX], *rho[REFIT_BATCH_MAX];
    for (int i = 0; i < n; ++i) {
        rows[i] = p->s;
        rows[i].ys = rb.ys + (size_t)i * sy;
        x[i] = rb.x + (size_t)i * sv;
        rhs[i] = rb.rhs + (size_t)i * sv;
        rho[i] = rb.rho + (size_t)i * sv;
    }
    *redo = false;
    p->fit_valid = false;
    p->geom_valid = false;
    // ---- the values and A^T W^2 y of every field (the refinement's pass at x = 0, without the constraint rows)
    for (int i = 0; i < n; ++i) {
        if (i == n - 1) stamp(p, 1, st);
        SPLPAK_HIP_TRY(launch_regather_values(g, p->s, ndata, c.y(k0 + i), rows[i].ys, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipMemsetAsync(x[i], 0, vbytes, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipMemsetAsync(rhs[i], 0, cbytes, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(plan_rows_residual(p, rows[i], x[i], false, rhs[i], st), SPLPAK_E_NODEVICE);
        if (i == n - 1) stamp(p, 2, st);
    }
    const auto t2 = clk::now();
    // ---- the first solve: one sweep for all
    for (int i = 0; i < n; ++i) SPLPAK_HIP_TRY(hipMemcpyAsync(x[i], rhs[i], cbytes, hipMemcpyDeviceToDevice, st), SPLPAK_E_NODEVICE);
    stamp(p, 6, st);
    SPLPAK_HIP_TRY(nd::nd_solve_many(p, n, x, st), SPLPAK_E_NODEVICE);
    stamp(p, 7, st);
    rb.stats[1] += 1;
    rb.stats[2] += n;
    // ---- refinement in lock-step: the fields still refining share the sweep of every step
    Refinement rf[REFIT_BATCH_MAX];
    double prev_rel[REFIT_BATCH_MAX];
    bool active[REFIT_BATCH_MAX];
    for (int i = 0; i < n; ++i) {
        rf[i] = Refinement();
        rf[i].converged = p->max_refine == 0;
        prev_rel[i] = std::numeric_limits<double>::infinity();
        active[i] = !rf[i].converged;
    }
    for (int it = 0; it < p->max_refine_hard; ++it) {
        int act[REFIT_BATCH_MAX], na = 0;
        for (int i = 0; i < n; ++i)
            if (active[i]) act[na++] = i;
        if (na == 0) break;
        double *v[REFIT_BATCH_MAX];
        for (int a = 0; a < na; ++a) {
            const int i = act[a];
            SPLPAK_HIP_TRY(hipMemsetAsync(rho[i], 0, sizeof(double) * (size_t)(b.npad + SC_COUNT), st), SPLPAK_E_NODEVICE);
            SPLPAK_HIP_TRY(plan_rows_residual(p, rows[i], x[i], smooth && p->rank == 0, rho[i], st), SPLPAK_E_NODEVICE);
            v[a] = rho[i];
        }
        SPLPAK_HIP_TRY(nd::nd_solve_many(p, na, v, st), SPLPAK_E_NODEVICE);
        rb.stats[1] += 1;
        rb.stats[2] += na;
        for (int a = 0; a < na; ++a)
            SPLPAK_HIP_TRY(launch_axpy_absmax(g.ncol, x[act[a]], rho[act[a]], rb.small + 2 * a, st), SPLPAK_E_NODEVICE);
        double am[2 * REFIT_BATCH_MAX];
        SPLPAK_HIP_TRY(hipMemcpyAsync(am, rb.small, 2 * sizeof(double) * (size_t)na, hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
        for (int a = 0; a < na; ++a)
            if (refinement_advance(p, rf[act[a]], prev_rel[act[a]], it, am + 2 * a)) active[act[a]] = false;
    }
    // ---- coefficients out; the diagnostics pass of every field, with the plan's own vectors holding that field (the last
    // field's stay: the plan describes it)
    double ssq[REFIT_BATCH_MAX], omega[REFIT_BATCH_MAX];
    hipEvent_t r0 = stamps ? p->evStage[8] : nullptr, r1 = stamps ? p->evStage[9] : nullptr;
    for (int i = 0; i < n; ++i) {
        const bool last = i == n - 1;
        ssq[i] = omega[i] = 0.0;
        SPLPAK_HIP_TRY(launch_to_reference_order(g, x[i], c.coef(k0 + i), st), SPLPAK_E_NODEVICE);
        const bool diag = c.info || rf[i].stagnated;
        if (!diag && !last) continue;
        SPLPAK_HIP_TRY(hipMemcpyAsync(p->xvec, x[i], vbytes, hipMemcpyDeviceToDevice, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipMemcpyAsync(p->rhs, rhs[i], cbytes, hipMemcpyDeviceToDevice, st), SPLPAK_E_NODEVICE);
        if (last) SPLPAK_HIP_TRY(hipMemcpyAsync(keep.ys, rows[i].ys, sizeof(double) * (size_t)ndata, hipMemcpyDeviceToDevice, st), SPLPAK_E_NODEVICE);
        if (!diag) continue;
        p->s.ys = rows[i].ys;
        const bool timed = last && r0 && r1;
        if (int r = plan_diagnostics_pass(p, p->fit_rows, st, timed ? r0 : nullptr)) return r;
        if (timed) (void)hipEventRecord(r1, st);
        SPLPAK_HIP_TRY(launch_backward_error(g, p->tmp, p->rho, p->small + 3, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipMemcpyAsync(&ssq[i], p->rho + b.npad, sizeof(double), hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipMemcpyAsync(&omega[i], p->small + 3, sizeof(double), hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
    }
    SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
    const double share_s = std::chrono::duration<double>(clk::now() - t2).count() / (double)n;
    // ---- verdicts: those of the solve stage.  Any field that would not return 0 sends the chunk to the field-by-field loop
    for (int i = 0; i < n; ++i) {
        const Refinement &r = rf[i];
        const bool unconverged = !r.converged && !r.diverged && r.last_rel == r.last_rel && r.est_err() > 1e-10;
        if (!(r.last_rel == r.last_rel) || r.diverged || (r.stagnated && !(omega[i] <= 1e-10)) || unconverged) *redo = true;
    }
    if (*redo) return 0;
    if (stamps) {
        plan_stage_times(p, true, false);
        float ms = 0.f;
        if (c.info && hipEventElapsedTime(&ms, r0, r1) == hipSuccess) p->stage_ms[4] = ms;
        else (void)hipGetLastError();
    }
    for (int i = 0; i < n && c.info; ++i) {
        double *inf = c.inf(k0 + i);
        const double v[10] = {p->fit_rows_data, p->fit_rows_cons, (double)rf[i].steps, rf[i].last_rel, p->fit_minpiv, 0.0, 0.0, share_s, std::sqrt(ssq[i]), omega[i]};
        for (int q = 0; q < 10; ++q) inf[q] = v[q];
    }
    p->fit_valid = true;                   // (single rank, no hook: splpak_plan_refit_dev refused the others)
    p->geom_valid = true;
    return 0;
}

extern "C" {

int32_t splpak_plan_fit_dev(splpak_plan *p, const double *x, int32_t l1xdat, const double *y,
                            const double *w, int64_t ndata, double *coef_dev, void *stream,
                            double *info)
{
    if (!p || !coef_dev) { set_error("null argument"); return SPLPAK_E_BADARG; }
    OptionsScope opt_scope(&p->opt);                                  // every switch a fit reads comes from the plan's snapshot
    if (ndata < 1 && p->world <= 1) return 105;                       // :759-764
    // A failure of ONE rank's arguments must not leave the others waiting in a collective: with more
    // than one rank it is carried through the first reduction as a flag and every rank returns.
    int lerr = 0;
    if (ndata < 0) ndata = 0;
    if (ndata > 0 && (!x || !y)) { set_error("null data pointer"); lerr = SPLPAK_E_BADARG; }
    else if (ndata > p->max_ndata) { set_error("ndata exceeds the plan's max_ndata"); lerr = SPLPAK_E_BADARG; }
    else if (l1xdat < p->g.ndim) { set_error("l1xdat < ndim"); lerr = SPLPAK_E_BADARG; }
    if (lerr == 0 && p->setup_rc != 0) { set_error("the plan's rank set-up failed (splpak_plan_set_allreduce)"); lerr = p->setup_rc; }
    if (lerr != 0 && p->world <= 1) return lerr;
    if (lerr != 0) ndata = 0;
    p->comm_failed = false;
    p->ne_valid = false;
    p->fit_valid = false;
    p->pcg_prepared = false;
    p->geom_valid = false;
    p->factor_valid = false;
    if (p->pcg) pcg_forget_fit(p->pcg);
    hipStream_t st = (hipStream_t)stream;
    if (lerr == 0 && w && ndata > 0) {
        // a negative first weight means "no weights" (:796, :890), as in the host entry points: one value read back
        double w0 = 0.0;
        SPLPAK_HIP_TRY(hipMemcpyAsync(&w0, w, sizeof(double), hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
        if (w0 < 0.0) w = nullptr;
    }
    const Grid &g = p->g;
    const Band &b = p->band;
    const bool smooth = p->xtrap != 0.0;                              // swght, :769
    using clk = std::chrono::steady_clock;
    auto t0 = clk::now();
    if (info) for (int i = 0; i < 10; ++i) info[i] = 0.0;

    // ---- assembly -------------------------------------------------------
    if (int r = plan_stage_events(p)) return r;
    // A 4-D plan that has the iteration IN FRONT of a factorisation assembles the normal equations only when the factorisation is
    // going to need them (round 6): the iteration applies the rows, its boxes are built from the rows (bj_build_kernel), and whether
    // it is tried at all is known from the histogram -- so the fit starts as an iteration-only plan's does (3 ms) and falls back to
    // the assembly (62 ms at 24^4: 40 % of such a fit) where the iteration is not tried or gives up.  One rank, no reduction hook.
    const bool lazy = plan_lazy_assembly(p);
    {   // (lazy: the half stencil is cleared when -- if -- it is assembled)
        const long long skip = lazy ? (long long)(p->rhs - p->comm) : 0;
        SPLPAK_HIP_TRY(hipMemsetAsync(p->comm + skip, 0, sizeof(double) * (size_t)(p->lenG + p->lenH - skip), st), SPLPAK_E_NODEVICE);
    }
    // (after the memset: the early clear of the factor arena that prefit starts on another stream is ordered behind this point of
    //  `st`, and the two used to share the memory system -- 0.07 ms of clearing took 0.7 ms beside it)
    if (p->prefit_fn) SPLPAK_HIP_TRY(p->prefit_fn(p, st, p->fn_user), SPLPAK_E_NODEVICE);
    stamp(p, 0, st);
    SPLPAK_HIP_TRY(launch_bin_points(g, ndata, x, l1xdat, y, w, p->s, p->scalH, st), SPLPAK_E_NODEVICE);
    if (p->pcg) SPLPAK_HIP_TRY(pcg_sum_w2(p, st), SPLPAK_E_NODEVICE);       // (rides the histogram's all-reduce)
    stamp(p, 1, st);
    const bool rows_fit = p->rows_only || lazy;        // the normal equations are not assembled (yet)
    if (rows_fit) {
        // the histogram from the rows (tile by tile); the right-hand side follows below, when the reduced histogram has gone
        if (smooth) {
            SPLPAK_HIP_TRY(rowsop_histogram(g, p->rowsop, p->s, p->hist, st), SPLPAK_E_NODEVICE);
            SPLPAK_HIP_TRY(launch_hist_total(g, p->hist, p->scalH, st), SPLPAK_E_NODEVICE);
        }
        SPLPAK_HIP_TRY(hipMemsetAsync(p->xvec, 0, sizeof(double) * (size_t)b.npad, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(rowsop_apply(g, p->rowsop, p->s, p->xvec, p->dcw, p->spf, p->ctab, false, p->rhs, st), SPLPAK_E_NODEVICE);   // A^T W^2 y
    } else
        SPLPAK_HIP_TRY(launch_gram(g, p->s, p->gscratch, p->gscratch_doubles, smooth, p->nst, p->rhs, p->hist, p->scalH, st, &p->gshape), SPLPAK_E_NODEVICE);
    stamp(p, 2, st);
    double hs[2 * SC_COUNT];
    if (p->world > 1) {
        const double one = 1.0;
        if (lerr != 0)
            SPLPAK_HIP_TRY(hipMemcpyAsync(p->scalH + SC_ERRFLAG, &one, sizeof(double), hipMemcpyHostToDevice, st), SPLPAK_E_NODEVICE);
        if (int r = plan_allreduce(p, p->hist, p->lenH, st)) return r;
        SPLPAK_HIP_TRY(hipMemcpyAsync(hs + SC_COUNT, p->scalH, sizeof(double) * SC_COUNT, hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
        SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
        if (hs[SC_COUNT + SC_ERRFLAG] != 0.0) {
            if (lerr != 0) return lerr;
            set_error("another rank of the sharded fit rejected its arguments");
            return SPLPAK_E_COMM;
        }
    }
    if (smooth && (p->rank == 0 || p->pcg))      // (every rank of an iterating fit: the preconditioner's second moment)
        SPLPAK_HIP_TRY(launch_sparse_mark(g, p->hist, p->scalH, p->xtrap, p->dcw, p->spf, st), SPLPAK_E_NODEVICE);
    if (smooth && p->rank == 0) {
        if (rows_fit) SPLPAK_HIP_TRY(launch_count_sparse(g, p->spf, p->scalG, st), SPLPAK_E_NODEVICE);      // (the rows are only counted)
        else SPLPAK_HIP_TRY(launch_constraint_rows(g, p->dcw, p->spf, p->ctab, p->nst, p->scalG, st), SPLPAK_E_NODEVICE);
    }
    stamp(p, 3, st);
    if (int r = plan_allreduce(p, p->rows_only ? p->rhs : p->nst, p->lenG, st)) return r;
    p->ne_valid = !rows_fit;

    SPLPAK_HIP_TRY(hipMemcpyAsync(hs, p->scalG, sizeof(double) * SC_COUNT, hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
    // scalG and scalH are not adjacent (hist sits between): fetch scalH separately
    SPLPAK_HIP_TRY(hipMemcpyAsync(hs + SC_COUNT, p->scalH, sizeof(double) * SC_COUNT, hipMemcpyDeviceToHost, st), SPLPAK_E_NODEVICE);
    SPLPAK_HIP_TRY(hipStreamSynchronize(st), SPLPAK_E_NODEVICE);
    const double rows_data = hs[SC_COUNT + SC_NROWS_DATA];
    const double rows_cons = hs[SC_NROWS_CONS];
    SolveStart a;
    a.t1 = clk::now();
    if (info) {
        info[0] = rows_data;
        info[1] = rows_cons;
        info[5] = std::chrono::duration<double>(a.t1 - t0).count();
    }
    // suprls error 33 "array has too few rows" (:1650-1654) -> 107 (:1053-1058)
    if (rows_data + rows_cons < (double)g.ncol) {
        p->ne_valid = false;
        return fit_fails_107(g, coef_dev, st, "fewer rows than coefficients (suprls 33)");
    }
    a.rows_cons = rows_cons;
    a.sumw2 = hs[SC_COUNT + SC_SUMW2];
    a.rows_fit = rows_fit;
    const int rc = plan_solve_stage(p, st, coef_dev, info, a);
    if (rc != 0) p->ne_valid = false;      // (a failed fit: splpak_debug_plan_normal_equations and _gram_shape refuse, as the header says)
    // what a refit continues from (splpak_plan_refit_dev)
    p->geom_valid = rc == 0 && p->fit_valid;
    p->fit_ndata = ndata;
    p->fit_rows_data = rows_data;
    p->fit_rows_cons = rows_cons;
    p->fit_sumw2 = a.sumw2;
    return rc;
}

int32_t splpak_plan_refit_dev(splpak_plan *p, int32_t nfields, const double *ydata_dev, int64_t ldy, double *coef_dev, int64_t ldcoef,
                              void *stream, double *info)
{
    if (!p || !ydata_dev || !coef_dev) { set_error("null argument"); return SPLPAK_E_BADARG; }
    if (nfields < 1) { set_error("nfields < 1"); return SPLPAK_E_BADARG; }
    // nothing to refit: decided here, on the host, before any device work
    if (p->world > 1 || p->dm.R > 1 || p->ar) { set_error("nothing to refit: the plan is a rank of a sharded or multi-GPU fit"); return SPLPAK_E_UNSUPPORTED; }
    if (!p->geom_valid) {
        set_error("nothing to refit: the plan holds no successful fit (none yet, a failed one, or a splpak_debug_plan_solve since): fit first");
        return SPLPAK_E_UNSUPPORTED;
    }
    const Grid &g = p->g;
    const long long ndata = p->fit_ndata;
    if (ldy < ndata) { set_error("ldy < ndata of the last fit"); return SPLPAK_E_BADARG; }
    if (ldcoef < g.ncol) { set_error("ldcoef < number of coefficients"); return SPLPAK_E_BADARG; }
    OptionsScope opt_scope(&p->opt);
    hipStream_t st = (hipStream_t)stream;
    p->comm_failed = false;
    if (int r = plan_stage_events(p)) return r;
    const RefitCall c{nfields, ydata_dev, ldy, coef_dev, ldcoef, info};
    // Fields that can share the sweeps of a held nested-dissection factor go in chunks of up to `refit_batch`; everything else --
    // one field, the band factorisations, the iteration, refit_batch = 1, no memory for the copies -- field by field
    const int batch = refit_batch_option();
    const bool batched = nfields >= 2 && batch > 1 && p->factor_valid && nd::nd_batch_ready(p) && refit_buffers_ready(p);
    p->rb.stats[0] = batched ? 2 : 1;
    p->rb.stats[1] = p->rb.stats[2] = p->rb.stats[3] = 0;
    if (!batched) return refit_field_by_field(p, c, 0, nfields, st);
    for (int k0 = 0; k0 < nfields; k0 += batch) {
        const int n = nfields - k0 < batch ? nfields - k0 : batch;
        bool redo = n == 1;                    // (a last chunk of one field has nothing to share)
        if (!redo) {
            if (int rc = refit_chunk_batched(p, c, k0, n, st, &redo)) return rc;
            if (redo) p->rb.stats[3] += n;     // a field of the chunk did not end in 0: the chunk again, by the loop that owns the 107 semantics
        }
        if (redo)
            if (int rc = refit_field_by_field(p, c, k0, k0 + n, st)) return rc;
    }
    return 0;
}

int32_t splpak_debug_plan_refit_stats(const splpak_plan *p, int64_t out4[4])
{
    if (!p || !out4) { set_error("null argument"); return SPLPAK_E_BADARG; }
    for (int i = 0; i < 4; ++i) out4[i] = p->rb.stats[i];
    return 0;
}

}  // extern "C"
