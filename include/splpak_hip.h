/*
 * splpak_hip.h -- C ABI of the MI355X (gfx950) implementation of SPLPAK's
 * least-squares cubic-spline fit / evaluate hot path.
 *
 * This is the drop-in boundary: a Fortran `splpak_module` (splpak_amd/fortran/
 * splpak_module.F90) binds these symbols with ISO_C_BINDING and keeps the
 * reference's public surface (`splpak_type%initialize/evaluate/destroy`,
 * `splpak_wp`).  Citations are into the reference, /root/reference/src/splpak.F90.
 *
 * Conventions
 *   - status return (`int32_t`) is the reference's `ierror`:
 *       0, 101..107 for the fit (:674-686), 0, 101..104 for evaluation (:1155-1161).
 *     Infrastructure failures (no GPU, HIP error, out of memory) are NEGATIVE
 *     (SPLPAK_E_*) and `splpak_last_error_message` explains them.  Nothing is
 *     printed by the library: the Fortran layer prints the reference's messages
 *     (cfaerr, :399-407) so stdout ordering matches.
 *   - `xdata` is the reference's column-major `xdata(l1xdat, ndata)` (:537-550),
 *     i.e. point i is the `ndim` doubles at `xdata + i*l1xdat`.
 *   - `coef` is ordered with the leftmost node index fastest (:657-673).
 *   - pointers are HOST pointers in the one-shot entry points and DEVICE pointers
 *     (same GPU as the plan) in the `_dev` / plan entry points.
 *   - there is NO CPU fallback: without a usable HIP device every compute entry
 *     point fails with SPLPAK_E_NODEVICE.
 *   - sizes: every count and every distance that is `int64_t` here (nq, ndata, offsets[], npts[], ldcoef, ldout, ldy,
 *     ldv, ldw, ldcov) may reach and pass 2^31 and 2^32 elements, and so may the products the `int32_t` strides form
 *     with a 64-bit index (query i at xq + i*ldxq, point p at xdata + p*l1xdat, row i of the derivatives at
 *     out + i*ldout): caller memory is addressed with 64-bit offsets throughout.  tests/test_large_index.py runs the
 *     device entries at such sizes -- the REAL32 instances past 2^31 and 2^32 (the kernels are templates over the
 *     storage type; the *_f64 entries are not run that large), and past 2^31 alone: splpak_eval_derivs_dev_f64,
 *     splpak_plan_refit_dev, the residual array of splpak_residuals_many_*, splpak_mad_many_*, both clipped batch fits
 *     and the sample count of splpak_fit_grid_*.  splpak_plan_fit_dev is run past 2^32 words on the binning's routes 1
 *     and 2; the strided read of its route 3 (grids of more than 1 048 320 cells) is 64-bit by reading only.
 *     The limits that do exist are stated at their entries:
 *     max_ndata of a plan <= 2^31 - 1025, a problem of a batch < 2^31 points, a grid call's tiles < 2^31 per launch,
 *     coefficient indices (ncol) in `int`, and the persistent region path of the evaluation, which numbers queries
 *     with 32 bits and leaves batches of 2^32 queries or more to the next path (same bits).
 */
#ifndef SPLPAK_HIP_H
#define SPLPAK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPLPAK_E_NODEVICE   (-1)  /* no HIP device / HIP runtime failure        */
#define SPLPAK_E_NOMEM      (-2)  /* device allocation failed                   */
#define SPLPAK_E_BADARG     (-3)  /* null pointer / inconsistent plan argument  */
#define SPLPAK_E_UNSUPPORTED (-4) /* ndim > 4 (the reference documents 1..4, :1099) */
#define SPLPAK_E_COMM       (-5)  /* the all-reduce callback reported failure   */

#define SPLPAK_MAXDIM 4

/* ---------------------------------------------------------------------------
 * One-shot host entry points -- what `splpak_module` binds.
 * ------------------------------------------------------------------------- */

/* Replaces splcw (:512-513) and, with wdata == NULL, splcc (:421-422; the
 * reference passes the sentinel wdata=[-1], :440).  A non-NULL wdata whose first
 * element is negative is treated like NULL (:581-588, :796).
 * `nwrk` is only used for the reference's 106 check (:772-781); the GPU path does
 * not use the caller's `work` array, except that when `hist_out` != NULL and
 * xtrap != 0 it receives the sparse-area histogram the reference leaves in
 * work(1:ncol) (:879-907).  `info` (optional, 10 doubles) receives diagnostics:
 *   [0] data rows used, [1] constraint rows, [2] refinement steps taken,
 *   [3] |last correction|_inf / |coef|_inf, [4] min Cholesky pivot (0 when no factorisation ran: the iterative solve answered),
 *   [5] seconds in assembly, [6] seconds in factorisation, [7] seconds in solve+refine (a 4-D plan with the iterative solve in
 *       front of a factorisation assembles the normal equations only when the factorisation is going to run: that assembly,
 *       and an attempt of the iteration that gave up, are then counted in [6]),
 *   [8] residual norm ||rows*coef - rhs||_2 over data and constraint rows -- the `reserr` that the
 *       reference computes (suprls :1693) and drops (splcw :690, :1052),
 *   [9] measured optimality residual of the returned coefficients: the gradient
 *       rho = A^T W (W y - W A x) - C^T C x of the least-squares functional (data rows A, constraint rows C),
 *       recomputed from the rows, as the componentwise backward error
 *       max_i |rho_i| / ((|N| |x|)_i + |A^T W^2 y|_i), N = A^T W^2 A + C^T C; 0 at the minimiser the reference
 *       computes, ~1e-14 when the fit is converged, ~cond(N) eps for plain normal equations.
 *       Fits that never assemble N (iteration-only 4-D plans, and 4-D fits the iteration answers before the assembly) normalise
 *       by (|A|^T W^2 |A| |x| + |C|^T |C| |x|)_i + |A^T W^2 y|_i from the rows instead: entry by entry at least |N| |x|, so their
 *       info[9] is the smaller (more lenient) of the two measures for the same coefficients.
 * The band-Cholesky solution is refined against the rows until the estimated remaining error
 * |dx|/|x| is below 1e-11 (2 steps at 64^3: corrections 9e-5, 1e-8, then an estimated 2e-12); a solve that is still contracting after the nominal
 * number of steps continues (up to 30), and one that then still misses 1e-10, or whose corrections
 * stop contracting while above 1e-8, is reported as 107 ("suprls failure") with an explanatory
 * splpak_last_error_message -- never as a silent success.
 * Data that is not finite.  A NaN or a +-Inf in ydata, or in a weight that is counted -- not the 0 of a point that is skipped,
 * not a negative first weight (which means "no weights"; a NaN first weight is not negative: the weights count) --, ends that
 * fit in 107 with a message, by the pivot test of the factorisation or by the refinement rule, whose corrections are then not
 * finite: never in 0.  The reference returns 0 and coefficients that are all NaN for such data.  `coef` is zeroed where the
 * factorisation refused and holds the unrefined values, which are not finite, otherwise -- for the point fit; where an entry
 * below says what its own 107 leaves in `coef` (the refits, the grid fits, the batch fits), that statement holds.  The plan
 * (the cached one of the one-shot entries too) stays usable: the next fit has the bits it has on a fresh plan.  This holds for
 * splpak_fit_f64 / _f32, splpak_plan_fit_dev on every solver route, splpak_plan_refit_dev and splpak_refit_* (a refit's 107
 * leaves the fit resident), splpak_fit_multi_f64 (every rank ends; the message is that of rank 0), splpak_fit_grid_* and
 * splpak_fit_grid_weighted_* (a value under a non-zero weight; a weight that is not finite is SPLPAK_E_BADARG there), and per
 * problem for splpak_fit_many_* and splpak_fit_many_cov_* (status 107, its coef and cov zeroed, every other problem of the
 * batch the bits it has without it).  Coordinates that are not finite are not covered; the clipping entries and
 * splpak_mad_many_* keep their own statement (unspecified). */
int32_t splpak_fit_f64(int32_t ndim, const double *xdata, int32_t l1xdat,
                       const double *ydata, const double *wdata, int64_t ndata,
                       const double *xmin, const double *xmax, const int32_t *nodes,
                       double xtrap, double *coef, int64_t ncf, int64_t nwrk,
                       double *hist_out, double *info);

/* real32 twin (reference built with -DREAL32, :33-34).  Storage is f32, the
 * arithmetic is f64 (the arrays are widened when they are staged for upload), so it
 * is at least as accurate as the REAL32 reference. */
int32_t splpak_fit_f32(int32_t ndim, const float *xdata, int32_t l1xdat,
                       const float *ydata, const float *wdata, int64_t ndata,
                       const float *xmin, const float *xmax, const int32_t *nodes,
                       float xtrap, float *coef, int64_t ncf, int64_t nwrk,
                       float *hist_out, double *info);

/* New values on the points of the last one-shot fit: several fields sampled at the same points (the components of a
 * velocity, a time series on a fixed sensor layout, bootstrap replicas) cost one fit and one refit each instead of a fit each.
 * The reference has no counterpart: every splcw call starts from the points (:512-1060).
 * splpak_fit_token: the token of the calling thread's last successful splpak_fit_f64 / _f32 (every successful fit of the
 * process draws a fresh one); 0 if there was none, or after a multi-GPU fit. */
int64_t splpak_fit_token(void);
/* Field k is the `ndata` values at ydata + k*ldy, in the point order of that fit (ldy >= ndata); its coefficients go to
 * coef + k*ldcoef (ldcoef >= ncol).  The fields are solved with what the fit left on the device -- its factorisation, or its
 * iteration -- as splpak_plan_refit_dev describes: on a held nested-dissection factor in chunks of up to 8 fields that share
 * every sweep of the factor (every field the bits of its own single-field refit; a chunk with a failing field is run again
 * field by field), otherwise one after another; info (10 doubles per field, may be NULL) likewise.
 * Returns 0; 107 as the fit would (that field's coefficients as the fit would return them, the later fields zeroed);
 * SPLPAK_E_BADARG for a null pointer, nfields < 1, ldy < ndata or ldcoef < ncol; SPLPAK_E_UNSUPPORTED, with the message "the
 * fit is no longer resident: fit again", when `token` is not that of the fit the library still holds or `ndata` is not its
 * number of points: after another fit, splpak_shutdown, a release of the cached plan under memory pressure, with
 * SPLPAK_NO_PLAN_CACHE, or after a multi-GPU fit.  A refused call (either of those two statuses) and a 107 leave the fit resident
 * and the token good; a device failure (SPLPAK_E_NODEVICE, SPLPAK_E_NOMEM) releases it. */
int32_t splpak_refit_f64(int64_t token, int32_t nfields, const double *ydata, int64_t ldy, int64_t ndata,
                         double *coef, int64_t ldcoef, double *info);
/* the REAL32 twin: storage f32, arithmetic f64 (token of a splpak_fit_f32 or a splpak_fit_f64 alike) */
int32_t splpak_refit_f32(int64_t token, int32_t nfields, const float *ydata, int64_t ldy, int64_t ndata,
                         float *coef, int64_t ldcoef, double *info);

/* Replaces a loop of splde (:1089) calls; nderiv == NULL gives splfe (:1258).
 * Query i is the `ndim` doubles at xq + i*ldxq (ldxq >= ndim, else SPLPAK_E_BADARG).  Error semantics per query are
 * the reference's: 101/102/103 return without computing (out is set to 0),
 * 104 (nderiv outside 0..2) is reported but the values are still computed with
 * nderiv clamped to 0..2 (the reference computes on, :1190-1194). */
int32_t splpak_eval_f64(int32_t ndim, int64_t nq, const double *xq, int32_t ldxq,
                        const int32_t *nderiv, const double *coef,
                        const double *xmin, const double *xmax, const int32_t *nodes,
                        double *out);
int32_t splpak_eval_f32(int32_t ndim, int64_t nq, const float *xq, int32_t ldxq,
                        const int32_t *nderiv, const float *coef,
                        const float *xmin, const float *xmax, const int32_t *nodes,
                        float *out);

/* ---------------------------------------------------------------------------
 * Resident-data (device pointer) API: plans, used by bench.py, by batched
 * callers and by the multi-GPU fit.  All work is enqueued on `stream`
 * (a hipStream_t passed as void*, NULL = the default stream).
 * ------------------------------------------------------------------------- */

typedef struct splpak_plan splpak_plan;

/* Sum-all-reduce hook for the sharded fit.  Called by
 * splpak_plan_fit_dev with a device pointer; must sum `count` doubles in place
 * across all ranks ON `stream` (or synchronise itself) and return 0.  With
 * torch.distributed/RCCL this is `all_reduce(tensor_view)`.  NULL => single rank.
 * The pointer lies in the plan's communication buffer for the histogram, the normal
 * equations and the refinement residuals.  A hook installed with
 * splpak_plan_set_allreduce_ex(.., SPLPAK_AR_ANY_POINTER) is also handed front panels,
 * Schur buffers and solve vectors that live in the library's own device allocations
 * (the nested-dissection factorisation distributed by subtrees, csrc/ndattach.hip, csrc/ndchol.hip). */
typedef int32_t (*splpak_allreduce_fn)(void *dev_buf, int64_t count, void *stream, void *user);

/* Validates exactly like splcw (:716-781; 105/106 are checked at fit time) and
 * allocates every device buffer the fit of a grid needs (band factor, stencil
 * normal equations, sort scratch for up to `max_ndata` points per call).
 * `max_ndata` (points per call on THIS GPU) is limited to 2^31 - 1025 (32-bit binning offsets);
 * larger values return SPLPAK_E_UNSUPPORTED.
 * `comm_buf_dev`/`comm_len`: optional caller-owned device buffer (doubles) the
 * all-reduced quantities live in -- pass a torch tensor's data_ptr so the
 * callback can all-reduce views of it; NULL lets the plan allocate it.  It must be device memory
 * the kernels can read and write at full speed (hipMalloc / a torch CUDA tensor): the assembly writes
 * the half stencil, right-hand side and histogram into it with plain stores (every sum has one owner and
 * a fixed order since round 2; the only floating-point atomic left is the histogram bump of a point so far
 * outside the grid that its nearest-node address is not a node of its window, src/splpak.F90:899).
 * `splpak_plan_comm_len` tells the required length. */
int64_t splpak_plan_comm_len(int32_t ndim, const int32_t *nodes);
int32_t splpak_plan_create(int32_t ndim, const int32_t *nodes, const double *xmin,
                           const double *xmax, double xtrap, int64_t max_ndata,
                           void *comm_buf_dev, int64_t comm_len, splpak_plan **plan);
void    splpak_plan_destroy(splpak_plan *plan);
void    splpak_plan_set_allreduce(splpak_plan *plan, splpak_allreduce_fn fn, void *user,
                                  int32_t rank, int32_t world);
/* The same with the hook's capabilities declared (round 4).  flags = 0 is splpak_plan_set_allreduce: the hook is only
 * ever called with windows of the plan's communication buffer (histogram, normal equations, refinement residuals) and
 * the factorisation is replicated on every rank, as in rounds 1-2.  SPLPAK_AR_ANY_POINTER: the hook accepts ANY device
 * pointer of the calling process (ncclAllReduce does; splpak_plan_set_rccl installs such a hook; the Python shim wraps
 * foreign pointers through the CUDA array interface) -- the nested-dissection factorisation of a sharded fit is then
 * distributed by subtrees (csrc/ndattach.hip, csrc/ndchol.hip; SPLPAK_ND_DIST=0 turns that off) and sums front panels, Schur buffers and
 * solve vectors that live in the library's own allocations.  Returns 0 or a negative status (a failure while the
 * per-rank job tables are rebuilt; the plan's next fit returns it on every rank). */
#define SPLPAK_AR_ANY_POINTER 1
#define SPLPAK_AR_ALWAYS      2   /* call the hook with one rank too (smoke tests of a one-rank communicator) */
#define SPLPAK_AR_STREAM_ORDERED 4 /* the hook only ENQUEUES its work on the stream it is handed (ncclAllReduce): the library then
                                     does not synchronise the stream before and after the call */
int32_t splpak_plan_set_allreduce_ex(splpak_plan *plan, splpak_allreduce_fn fn, void *user,
                                     int32_t rank, int32_t world, int32_t flags);
/* tuning / test knobs: nominal refinement steps (default 4; 0 = none; a solve that still contracts goes on
 * up to max(steps, 30)) and the tolerance on the (estimated) remaining relative error |dx|/|x| after a
 * step (default 1e-11; the parity bar is 1e-10) */
/* A native RCCL hook (round 4): the plan's sum-all-reduce becomes ncclAllReduce(.., ncclDouble, ncclSum, comm, stream) on the
 * fit's stream, with SPLPAK_AR_ANY_POINTER declared -- what a C / Fortran process-per-GPU caller uses instead of the Python
 * callback.  `nccl_comm` is the caller's ncclComm_t (one per process, made on the GPU the plan lives on).  librccl is opened at
 * run time (an RCCL the process already carries is reused; SPLPAK_RCCL_LIB names another); SPLPAK_E_COMM if it cannot be.
 * For callers without RCCL headers the communicator can be made here: rank 0 draws the 128-byte ncclUniqueId
 * (splpak_rccl_unique_id) and passes it to the other processes by any means -- splpak_rccl_comm_create_from_file[_ex] does it
 * through a file (no MPI needed on one node) -- and every process calls splpak_rccl_comm_create with the CURRENT device set
 * to its GPU.  The id file (round 5): { "SPLPAKID", job tag, publish time, id } = 152 bytes.  Rank 0 removes whatever lies at
 * `path`, writes its file atomically and removes it again once ncclCommInitRank has returned (collective: every rank has the
 * id by then); the others wait up to timeout_s seconds (<= 0: 60) for a file that carries THEIR job's tag and is no older than
 * that wait -- a file left by another run is ignored (a stale id would hang ncclCommInitRank), and the call times out with
 * SPLPAK_E_COMM.  `job` names the run (any string all ranks of ONE run share and other runs do not); NULL / "" = the environment
 * variable SPLPAK_RCCL_JOB, else what the launcher exports (TORCHELASTIC_RUN_ID, MASTER_ADDR, MASTER_PORT, SLURM_JOB_ID, ...). */
int32_t splpak_plan_set_rccl(splpak_plan *plan, void *nccl_comm, int32_t rank, int32_t world);
int32_t splpak_rccl_unique_id(char *id128);
int32_t splpak_rccl_comm_create(const char *id128, int32_t rank, int32_t world, void **nccl_comm);
int32_t splpak_rccl_comm_create_from_file(const char *path, int32_t rank, int32_t world, double timeout_s, void **nccl_comm);
int32_t splpak_rccl_comm_create_from_file_ex(const char *path, const char *job, int32_t rank, int32_t world, double timeout_s, void **nccl_comm);
void    splpak_rccl_comm_destroy(void *nccl_comm);
void    splpak_plan_set_refine(splpak_plan *plan, int32_t max_steps, double tol);

/* The fit on resident data.  xdata_dev/ydata_dev/wdata_dev (wdata_dev may be
 * NULL; a negative first weight of this rank's points means no weights, as in splcw) hold THIS rank's `ndata` points (with more than one rank a rank may hold none: ndata = 0,
 * pointers ignored); coef_dev receives ncol coefficients (identical on every rank).  A rank whose
 * arguments are rejected still takes part in the first reduction, which carries an error flag: that
 * rank returns its status, the others SPLPAK_E_COMM -- nobody is left waiting in a collective.  Synchronises `stream` before returning (the error
 * flag and the refinement's convergence test are read back).  info as above.
 * Sizes: ndata <= the plan's max_ndata <= 2^31 - 1025 (32-bit binning offsets), but ndata*l1xdat may pass 2^31 and 2^32
 * words: point i is read at xdata_dev + i*l1xdat with a 64-bit i, and the result does not depend on l1xdat. */
int32_t splpak_plan_fit_dev(splpak_plan *plan, const double *xdata_dev, int32_t l1xdat,
                            const double *ydata_dev, const double *wdata_dev,
                            int64_t ndata, double *coef_dev, void *stream, double *info);
/* New values on the points of the plan's last fit.  Only the solve depends on ydata: the binned points, the histogram, the
 * data-sparse flags, the constraint rows, N = A^T W^2 A + C^T C, its factor and the iteration's preconditioner are functions of
 * xdata, wdata and the grid, and a successful single-rank fit leaves them in the plan.  Field k is the `ndata` values (of that
 * fit) at ydata_dev + k*ldy, in that fit's point order; its ncol coefficients go to coef_dev + k*ldcoef (k*ldy and k*ldcoef
 * beyond 2^31 and 2^32 words are supported, field by field and in batched sweeps).  For every field
 * the values are gathered into the binned order, A^T W^2 y is one pass over the rows, and the solve, the refinement against
 * the rows, the diagnostics and the decisions that end in 107 are the fit's own.  Two or more fields on a held factor of the
 * single-GPU nested dissection are solved in chunks of up to 8 fields that share every sweep of the factor (option
 * refit_batch: fields per sweep, 1 .. 8, default 8; 1 = field by field): the first solve and every refinement step read the
 * factor's panels once for all fields of the chunk that are still refining.  Every field's coefficients and its info [0..4],
 * [8], [9] are bit for bit those of its single-field refit; [7] is the chunk's solve time divided by its fields.  If any
 * field of a chunk does not end with status 0 the chunk's results are discarded and the chunk is run again field by field,
 * which decides what a 107 returns.  The per-field copies this needs (8 x (2 vectors of the solve + partial sums), 8 x
 * max_ndata values, 8 x 3 vectors) are allocated at the first such call and counted in splpak_plan_device_bytes; without the
 * memory for them the plan refits field by field.  Every other call processes the fields one after another.  The solver
 * follows what the fit left: a held factor is used as it is (no expansion, no factorisation); a fit the iteration answered is
 * iterated again on the prepared preconditioner, and if that gives up and the plan has a factorisation the normal equations
 * are assembled from the binned points and factored as the fit does -- the later fields then use the factor.
 * info (10 doubles per field, may be NULL) as for the fit: [0] [1] the fit's row counts, [2] [3] [7] [8] [9] measured for the
 * field, [4] the held factor's smallest pivot, [5] 0, [6] 0 unless the factorisation ran in this call.
 * Returns 0; 107 as the fit (that field's coefficients zeroed or returned as the fit would, the later fields zeroed; the plan
 * stays refit-able); SPLPAK_E_BADARG for a null pointer, nfields < 1, ldy < ndata or ldcoef < ncol; SPLPAK_E_UNSUPPORTED, with a
 * message naming the reason, when there is nothing to refit: no successful fit yet, a failed fit, a splpak_debug_plan_solve
 * since the fit, or a plan that is a rank of a sharded or multi-GPU fit (an all-reduce hook installed) -- decided on the host
 * before any device work.  Synchronises `stream` before returning.
 * After a successful refit splpak_debug_plan_rows_gradient and splpak_debug_plan_normal_equations describe the LAST FIELD: N is
 * the fit's, rhs and the values of the rows are the field's; after a refit that returned 107 the former refuses, as after a
 * failed fit.  splpak_plan_stage_timing after a refit: [1] is the values gather + right-hand side, [0] and [2] are 0, [3] is 0
 * unless the factorisation ran, [4] [5] as for the fit; after a batched refit [1] is the last field's gather + right-hand
 * side, [5] the last chunk's first sweep, [4] a residual pass, [0] [2] [3] are 0. */
int32_t splpak_plan_refit_dev(splpak_plan *plan, int32_t nfields, const double *ydata_dev, int64_t ldy,
                              double *coef_dev, int64_t ldcoef, void *stream, double *info);
/* How the plan's last splpak_plan_refit_dev went (host counters; diagnostics): out4[0] its route -- 0 none yet, 1 field by
 * field, 2 batched sweeps --, [1] the tree solves it launched (single and batched sweeps together; the solves of a band factor
 * count too), [2] the right-hand sides those solves carried in total, [3] the fields run again field by field because their
 * chunk did not end in 0.  SPLPAK_E_BADARG for a null argument. */
int32_t splpak_debug_plan_refit_stats(const splpak_plan *plan, int64_t out4[4]);
/* device pointer to the (all-reduced) sparse-area histogram of the last fit */
const double *splpak_plan_hist_dev(const splpak_plan *plan);
/* device memory the plan holds (bytes) */
int64_t splpak_plan_device_bytes(const splpak_plan *plan);
/* Which factorisation of the normal equations the plan uses in place of suprls' triangularisation
 * (src/splpak.F90:1516-1619): returns 0 band Cholesky (four-stream pipeline), 1 its narrow form, 2 two-ended band,
 * 3 band distributed over several GPUs, 4 nested-dissection multifrontal (2-D / 3-D grids of >= 4 096 columns, 4-D grids of
 * >= 20 000), 5 the same distributed over the GPUs of a one-process multi-GPU plan (subtrees per GPU, the fronts above them by
 * block columns; the description names the elimination schedule's cut -- chosen from the free device memory unless the option
 * nd_cut fixes it -- and run-to-run bit reproducibility of a large grid's coefficients is promised for the SAME cut: the order in
 * which two siblings with different numbers of block steps add into their parent follows the schedule), 6 NO factorisation: the iterative solve below (grids whose factor does not fit the device, or by request);
 * a description is copied into buf. */
int32_t splpak_plan_factorisation(const splpak_plan *plan, char *buf, int32_t buflen);
/* Options (round 6).  Every switch of the library is a named option; a plan takes a snapshot of them when it is created --
 * the process defaults set here over the SPLPAK_<NAME> variables of the environment -- and a fit reads nothing else (no getenv
 * on the fit path; the one-shot entry's cached plan is keyed by the snapshot).  `name` is "nd_kb", "ND_KB" or "SPLPAK_ND_KB";
 * `value` is the text the environment variable would hold, NULL removes the setting.  Returns 0, SPLPAK_E_BADARG for an
 * unknown name, and (plan_set_option) SPLPAK_E_UNSUPPORTED for an option that shapes the plan's storage or job tables and is
 * therefore consumed at creation (solver, nd, nd_split, nd_cut, nd_kb, nd_res_cus, no_reorder, gram_scratch_mb, pcg_maxit,
 * mplan_rccl, rccl_lib): set those as defaults before splpak_plan_create.  The documented options are listed in
 * INTEGRATION.md; the other names are A/B switches of the test suite and may disappear.
 * splpak_plan_get_option: 1 if set (value copied into buf), 0 if not. */
int32_t splpak_set_default_option(const char *name, const char *value);
int32_t splpak_plan_set_option(splpak_plan *plan, const char *name, const char *value);
int32_t splpak_plan_get_option(const splpak_plan *plan, const char *name, char *buf, int32_t buflen);

/* The iterative solve (round 6; csrc/pcg.hip): preconditioned conjugate gradients on the normal equations with the operator
 * applied from the rows (data rows :788-855, constraint rows :921-1046) and a separable preconditioner, inside the same
 * refinement against the rows as the factorisations.  It replaces suprls (:1375-1695) for the grids the reference accepts
 * (any grid, :512-534) and no factorisation fits: BASELINE config 5's 4-D 32^4 grid on one GPU.  Selected automatically when
 * the factor storage cannot be allocated and, in front of the factorisation, for 4-D grids of 160 000 columns or more; or with
 * the option solver = pcg (iteration only) / pcg+direct (iteration first, the factorisation when it stagnates) / direct.  A fit whose iteration stagnates and whose plan
 * has no factorisation returns 107 with an explanatory message.
 * out6: [0] iterations of the last fit over all its solves, [1] solves, [2] iterations of the last solve, [3] its final
 * preconditioned residual (relative), [4] [5] the preconditioner's two moments (density of w^2, mean squared constraint weight);
 * zeros for a plan without the iteration, and after a fit that did not iterate (it went to the factorisation without an
 * attempt, or failed before the solve): never the numbers of an earlier fit. */
void splpak_plan_pcg_stats(const splpak_plan *plan, double *out6);

/* Per-kernel accounting of the last splpak_plan_fit_dev call, measured with HIP
 * events on the stream the kernels ran on (bench.py's roofline object).  Every BULK
 * trailing-update launch carries a start/stop event pair in its dispatch (hipExtLaunchKernelGGL).
 * "Bulk" is, for the nested-dissection factorisation, every Schur-buffer pass of the fronts
 * (nd_syrk_kernel<4,2,true,..>, f64 MFMA, K up to 1024 per pass: ~73 % of the factorisation's flops at
 * 64^3; the panel updates of the chain are the instantiation <..,false,..>); for the band factorisation
 * the one launch per block step that updates the block columns beyond the next one (syrk64_kernel,
 * ~96 % of the flops):
 *   out[0] = number of timed bulk launches
 *   out[1] = total milliseconds in them
 *   out[2] = floating-point operations they performed (algorithmic: 2*64*64*K per 64x64 item)
 *   out[3] = milliseconds in the whole factorisation
 *   out[4] = floating-point operations of ALL trailing-update launches
 *   out[5] = number of bulk launches, out[6] = their floating-point operations
 * Timing is only collected when enabled. */
void    splpak_plan_enable_kernel_timing(splpak_plan *plan, int32_t on);
void    splpak_plan_kernel_timing(const splpak_plan *plan, double *out7);
/* milliseconds of the stages of the last fit around the factorisation (HIP events on the fit's stream, collected
 * with kernel timing enabled): out[0] binning (keys, scan, scatter, in-cell ordering), [1] Gram blocks + gather,
 * [2] constraint rows, [3] band memset + expansion, [4] one refinement-residual pass, [5] one solve (two sweeps) */
void    splpak_plan_stage_timing(const splpak_plan *plan, double *out6);

/* ---------------------------------------------------------------------------
 * Several GPUs of one node, driven from ONE process: what a Fortran caller reaches
 * through `splpak_type%set_gpus(n)`.  The points are sharded over the GPUs and the factorisation of the
 * normal equations is DISTRIBUTED WITH ITS MEMORY PARTITIONED:
 *   - grids that take the nested-dissection factorisation (2-D / 3-D grids of >= 4 096 columns, 4-D grids of
 *     >= 20 000; since round 4): the subtrees below tree depth ceil(log2 ngpus) are dealt to the GPUs, the
 *     fronts above them are cut into 256-column blocks dealt to the GPUs in chunks of `chunk` blocks; a solved
 *     panel is copied GPU-to-GPU (hipMemcpyPeerAsync over xGMI) by the owners of the columns it updates, a
 *     child's Schur complement is pulled by the owners of the parent's columns through the peer mapping
 *     (csrc/ndtop.hip).  64^3: 4.4-4.6 GB of factorisation per GPU on eight instead of 30 GB; the 4-D 32^4 grid
 *     of BASELINE config 5: 159-190 GB per GPU on eight (476 GB of panels do not fit one GPU).  This form needs
 *     peer access between every pair of distinct devices (kernels read the other GPUs' memory): without it the
 *     plan falls back to the distributed band below, or returns SPLPAK_E_UNSUPPORTED when that cannot hold the grid;
 *   - smaller grids (or SPLPAK_MPLAN_BAND=1): the BAND of the normal equations dealt by block columns (round 2),
 *     every GPU stores and updates only its own block columns, the solved panel of every block step travels
 *     GPU-to-GPU, the triangular sweeps hand the active window from owner to owner (copies only: no peer mapping needed).
 * The sums over the ranks (histogram, normal equations, residuals) are reduce-scatter + all-gather over point-to-point
 * copies in rank order (bitwise reproducible), or -- option mplan_rccl, round 5 -- one ncclAllReduce per rank thread (no group call) of a
 * communicator the plan makes over its devices (ncclCommInitAll; distinct devices only).
 * Results are those of the single-GPU fit (same kernels per tile: with all points on rank 0 the coefficients are
 * bit-identical to it).
 * `chunk` < 1 chooses it automatically (nested dissection: 1; band: about one chunk per GPU inside the band window, at most 8).
 * `devices`: NULL = devices 0..ngpus-1; entries may repeat -- with SPLPAK_VIRTUAL_GPUS=1 in the
 * environment every rank is placed on the current device, which runs the whole protocol on one GPU
 * (the 1-GPU test tier does that).
 * ------------------------------------------------------------------------- */
typedef struct splpak_mplan splpak_mplan;
int32_t splpak_mplan_create(int32_t ngpus, const int32_t *devices, int32_t chunk, int32_t ndim,
                            const int32_t *nodes, const double *xmin, const double *xmax, double xtrap,
                            int64_t max_ndata_per_gpu, splpak_mplan **mplan);
void    splpak_mplan_destroy(splpak_mplan *mplan);
/* device of a rank (for placing its shard) */
int32_t splpak_mplan_device(const splpak_mplan *mplan, int32_t rank);
/* which factorisation the plan's ranks use (codes of splpak_plan_factorisation: 3 distributed band, 5 distributed nested dissection) */
int32_t splpak_mplan_factorisation(const splpak_mplan *mplan, char *buf, int32_t buflen);
/* device memory a rank of the plan holds (bytes): its plan (binning scratch, normal equations, its part of the factor)
 * and its panel / staging buffers */
int64_t splpak_mplan_rank_bytes(const splpak_mplan *mplan, int32_t rank);
/* xdata_dev[r] / ydata_dev[r] / wdata_dev[r] (wdata_dev may be NULL = unweighted) are device pointers
 * on rank r's GPU holding ndata[r] points (0 allowed); coef_dev (ncol doubles) is on rank 0's GPU.
 * Blocks until the fit is complete.  Status and `info` as splpak_plan_fit_dev. */
int32_t splpak_mplan_fit_dev(splpak_mplan *mplan, const double *const *xdata_dev, int32_t l1xdat,
                             const double *const *ydata_dev, const double *const *wdata_dev,
                             const int64_t *ndata, double *coef_dev, double *info);
/* one-shot host entry: as splpak_fit_f64 on `ngpus` GPUs (contiguous shards of the points); ngpus <= 1
 * is splpak_fit_f64 itself.  SPLPAK_DIST_CHUNK sets the chunk (default 0 = automatic). */
int32_t splpak_fit_multi_f64(int32_t ngpus, int32_t ndim, const double *xdata, int32_t l1xdat,
                             const double *ydata, const double *wdata, int64_t ndata,
                             const double *xmin, const double *xmax, const int32_t *nodes,
                             double xtrap, double *coef, int64_t ncf, int64_t nwrk,
                             double *hist_out, double *info);

/* Batched evaluation on resident data (asynchronous on `stream`; no validation
 * beyond the reference's 101..104, which is done on the host from the small
 * arguments).  Sizes: nq and nq*ldxq beyond 2^31 and 2^32 are supported -- query i is read at xq_dev + i*ldxq with a
 * 64-bit i by the direct kernel and by every sorted path (their chunks start at xq_dev + c0*ldxq, c0 64-bit).  One limit:
 * the persistent region path numbers the queries of a call with 32 bits, so a call of more than 2^32 - 8192 queries
 * falls through to the run path or the region sort, which work through the batch in chunks and return the same bits. */
int32_t splpak_eval_dev_f64(int32_t ndim, int64_t nq, const double *xq_dev, int32_t ldxq,
                            const int32_t *nderiv /* host, may be NULL */,
                            const double *coef_dev, const double *xmin, const double *xmax,
                            const int32_t *nodes, double *out_dev, void *stream);

/* The same for REAL32 storage (queries, coefficients and results in single precision, arithmetic in double:
 * the batched counterpart of the -DREAL32 build of splfe / splde, src/splpak.F90:33-41). */
int32_t splpak_eval_dev_f32(int32_t ndim, int64_t nq, const float *xq_dev, int32_t ldxq,
                            const int32_t *nderiv /* host, may be NULL */,
                            const float *coef_dev, const float *xmin, const float *xmax,
                            const int32_t *nodes, float *out_dev, void *stream);

/* Value, gradient and (order 2) Hessian of the spline at a batch of points in one pass over the
 * window -- SURVEY 8f: what a caller otherwise obtains from 1 + ndim (+ ndim(ndim+1)/2) splde calls
 * (:1089-1240) per point.  order = 1 or 2.  Row i of `out` (ldout apart, ldout >= number of entries):
 *   [ f, df/dx_1 .. df/dx_ndim, (order 2:) d2f/dx_1dx_1, d2f/dx_1dx_2, .., d2f/dx_1dx_ndim, d2f/dx_2dx_2, .. ]
 * i.e. the upper triangle of the Hessian row by row.  Each entry equals splde with the matching nderiv.
 * Sizes: nq*ldout (and nq*ldxq) beyond 2^31 and 2^32 elements are supported, row i is addressed with a 64-bit i.
 * Status: 0, 101/102/103 as splde (`out` is zeroed), or a negative library status. */
int32_t splpak_eval_derivs_f64(int32_t ndim, int64_t nq, const double *xq, int32_t ldxq, int32_t order,
                               const double *coef, const double *xmin, const double *xmax,
                               const int32_t *nodes, double *out, int32_t ldout);
int32_t splpak_eval_derivs_f32(int32_t ndim, int64_t nq, const float *xq, int32_t ldxq, int32_t order,
                               const float *coef, const float *xmin, const float *xmax,
                               const int32_t *nodes, float *out, int32_t ldout);
/* the same on resident data (asynchronous on `stream`) */
int32_t splpak_eval_derivs_dev_f64(int32_t ndim, int64_t nq, const double *xq_dev, int32_t ldxq, int32_t order,
                                   const double *coef_dev, const double *xmin, const double *xmax,
                                   const int32_t *nodes, double *out_dev, int32_t ldout, void *stream);

/* Evaluation on a tensor-product grid of points: replaces the loop of splfe (:1258) / splde (:1089) calls over a
 * regular sample that resamples a fit into an image, a volume or a table.
 *   axes   the axis coordinates back to back: the npts[0] coordinates of dimension 1, then the npts[1] of
 *          dimension 2, ...; sum_d npts[d] values.  Any values: unsorted, repeated, outside [xmin, xmax] (the
 *          reference extrapolates through its window rule, :1201-1209, and so does this).
 *   out    prod_d npts[d] values, dimension 1 fastest -- out[i0 + npts[0]*(i1 + npts[1]*(i2 + ...))], the ordering
 *          `coef` uses (:227-228) -- each what splde (splfe when nderiv == NULL) returns at
 *          (axes_1[i0], axes_2[i1], ...): the very values splpak_eval_* computes for that point.
 * No query list is formed and nothing is sorted: 8 bytes of device memory traffic per output (4 for REAL32) and the
 * coefficients; output counts beyond 2^31 and 2^32 are fine in both tile forms (64-bit output indices; the limit is the
 * tile count of a launch, below 2^31: at 64 x 8 x 8 outputs per 3-D tile that is 8.8e12 outputs).
 * Status as splpak_eval_f64: 101/102/103 return without computing, `out` set to 0 (101 -- no dimensions, so no
 * shape: out[0] alone); 104 (nderiv outside 0..2) is reported but the values are computed with nderiv clamped to
 * 0..2 (:1190-1194).  SPLPAK_E_BADARG: a null pointer, a negative npts[d], a product of npts beyond int64;
 * SPLPAK_E_UNSUPPORTED: ndim > 4.  If any npts[d] is 0 the validation status is returned and nothing is written.
 * All of these are decided on the host before any device work. */
int32_t splpak_eval_grid_f64(int32_t ndim, const int64_t *npts, const double *axes, const int32_t *nderiv,
                             const double *coef, const double *xmin, const double *xmax, const int32_t *nodes,
                             double *out);
int32_t splpak_eval_grid_f32(int32_t ndim, const int64_t *npts, const float *axes, const int32_t *nderiv,
                             const float *coef, const float *xmin, const float *xmax, const int32_t *nodes,
                             float *out);
/* the same on resident data (asynchronous on `stream`); npts, nderiv, xmin, xmax and nodes are host arrays */
int32_t splpak_eval_grid_dev_f64(int32_t ndim, const int64_t *npts /* host */, const double *axes_dev,
                                 const int32_t *nderiv /* host, may be NULL */, const double *coef_dev,
                                 const double *xmin, const double *xmax, const int32_t *nodes,
                                 double *out_dev, void *stream);
int32_t splpak_eval_grid_dev_f32(int32_t ndim, const int64_t *npts /* host */, const float *axes_dev,
                                 const int32_t *nderiv /* host, may be NULL */, const float *coef_dev,
                                 const float *xmin, const float *xmax, const int32_t *nodes,
                                 float *out_dev, void *stream);
/* Device memory (bytes) a grid call of this shape keeps, per calling thread, until splpak_shutdown: the per-axis
 * factor tables, 40 bytes per axis coordinate.  0 when a count is 0; SPLPAK_E_BADARG for a shape the entries reject. */
int64_t splpak_eval_grid_scratch_bytes(int32_t ndim, const int64_t *npts);
/* Diagnostics: how many workgroup tiles of the calling thread's last grid call contracted a coefficient box staged in
 * LDS (out2[0]) and how many gathered every window from global memory (out2[1]: boxes beyond the LDS budget -- coarse
 * or unsorted axes -- and every 1-D call).  Waits for that call.  Both forms return the same values.  A
 * splpak_eval_grid_derivs_* call is a grid call too: after one, these are the counts of its tiles. */
int32_t splpak_debug_eval_grid_stats(int64_t out2[2]);

/* Value, gradient and (order 2) Hessian of the fit on a tensor-product grid of points in one pass: what a loop of
 * splpak_eval_grid_* calls over the 1 + ndim (+ ndim(ndim+1)/2) nderiv patterns returns -- normals of an iso-surface,
 * the velocity of a potential, strain, vorticity or curvature volumes on the sample splpak_eval_grid_* resamples to --
 * with one table pass, one staging of the coefficients per tile, and the partial sums the patterns share formed once.
 *   npts, axes  exactly as for splpak_eval_grid_*;  order  1 or 2;
 *   out    in PLANES: entry e of grid point idx is out[e*ldout + idx], ldout >= prod_d npts[d];
 *          idx = i0 + npts[0]*(i1 + npts[1]*(i2 + ...)) is the ordering of splpak_eval_grid_*, and e runs over the entries
 *          of splpak_eval_derivs_* in its order: f, df/dx_1 .. df/dx_ndim, (order 2:) the upper triangle of the Hessian
 *          row by row.  Each plane is a volume as splpak_eval_grid_* writes it.  The words between the planes,
 *          [prod npts, ldout), are neither read nor written.  As for splpak_eval_grid_*, prod npts and e*ldout beyond 2^31
 *          and 2^32 elements are supported; the tiles of one launch stay below 2^31 (larger shapes are refused).
 * Plane e >= 1 holds the very values (identical bits) of splpak_eval_grid_* called with entry e's nderiv pattern: the
 * same factor tables and the same order of summation, whichever outputs share a partial sum.  Plane 0 is summed in that
 * order on the GENERAL-form factor tables (what every nderiv != NULL call uses), whereas splpak_eval_grid_* with
 * nderiv == NULL takes the closed-form value tables: plane 0 agrees with it to rounding, not to the bit.  Plane 0 has the
 * same bits for order 1 and 2.
 * Status, decided on the host before any device work, the first failing check wins:
 *   SPLPAK_E_BADARG       npts, nodes, xmin or xmax null;
 *   101                   out[0] alone is set to 0 (if `out` is not null), as the grid entries do;
 *   SPLPAK_E_UNSUPPORTED  ndim > 4;
 *   SPLPAK_E_BADARG       a negative npts[d] or a product of npts beyond int64; then order outside 1..2; then
 *                         ldout < prod npts or (number of planes)*ldout beyond int64;
 *   102 / 103             the prod npts results of EVERY plane are set to 0 (if `out` is not null), the words between
 *                         the planes stay as they are;
 *   a count of 0          the status so far; nothing is written;
 *   SPLPAK_E_BADARG       axes, coef or out null.
 * There is no nderiv argument, hence no 104. */
int32_t splpak_eval_grid_derivs_f64(int32_t ndim, const int64_t *npts, const double *axes, int32_t order,
                                    const double *coef, const double *xmin, const double *xmax, const int32_t *nodes,
                                    double *out, int64_t ldout);
int32_t splpak_eval_grid_derivs_f32(int32_t ndim, const int64_t *npts, const float *axes, int32_t order,
                                    const float *coef, const float *xmin, const float *xmax, const int32_t *nodes,
                                    float *out, int64_t ldout);
/* the same on resident data (asynchronous on `stream`); npts, xmin, xmax and nodes are host arrays */
int32_t splpak_eval_grid_derivs_dev_f64(int32_t ndim, const int64_t *npts /* host */, const double *axes_dev, int32_t order,
                                        const double *coef_dev, const double *xmin, const double *xmax,
                                        const int32_t *nodes, double *out_dev, int64_t ldout, void *stream);
int32_t splpak_eval_grid_derivs_dev_f32(int32_t ndim, const int64_t *npts /* host */, const float *axes_dev, int32_t order,
                                        const float *coef_dev, const float *xmin, const float *xmax,
                                        const int32_t *nodes, float *out_dev, int64_t ldout, void *stream);
/* Device memory (bytes) such a call keeps per calling thread until splpak_shutdown: the two tile counters and, per axis
 * coordinate, a window start and order + 1 factor quadruples: 16 + (32*(order + 1) + 8) * sum_d npts[d].  It is the scratch of
 * splpak_eval_grid_*, grown on demand: a thread holds the larger of the two needs, not their sum.  0 when a count is 0;
 * SPLPAK_E_BADARG for a shape or an order the entries reject. */
int64_t splpak_eval_grid_derivs_scratch_bytes(int32_t ndim, const int64_t *npts, int32_t order);
/* Host only: the outputs per workgroup tile per dimension (1 beyond ndim) of a splpak_eval_grid_derivs_* call with this
 * ndim and order, so that the tiles splpak_debug_eval_grid_stats counts can be predicted.  Every (ndim, order) class runs
 * the fused tile kernel.  SPLPAK_E_BADARG: ndim outside 1..4, order outside 1..2 or a null pointer. */
int32_t splpak_debug_eval_grid_derivs_tile(int32_t ndim, int32_t order, int32_t out4[4]);

/* Definite integrals of the fit over the cells of a tensor grid: the total over a box (ncell = 1 everywhere), the cell
 * integrals of a finite-volume mesh (the mean is the caller's division by the cell volume: conservative remapping), a
 * projection (a 3-D fit integrated along z onto an x-y image, a column density).  Exact: the fit is one global piecewise
 * polynomial -- per dimension a cubic on every node cell [xmin + k*dx, xmin + (k+1)*dx], a straight line below xmin and
 * above xmax -- so every cell is cut at the node lines and each piece integrated by two-point Gauss-Legendre.
 *   mode   mode[d] = 1: dimension d is INTEGRATED, its axis holds ncell[d] + 1 edges and output index j is the cell from
 *          e[j] to e[j+1];  mode[d] = 0: dimension d is EVALUATED, its axis holds ncell[d] coordinates as for
 *          splpak_eval_grid_* (values only).  NULL: every dimension is integrated.
 *   axes   the axes back to back, as splpak_eval_grid_* takes them.  Edges may be anything: unsorted, repeated
 *          (e[j] == e[j+1] gives exactly 0), outside the grid (the integral of the linear extrapolation), reversed (the
 *          exact negation of the cell taken the other way round).  Non-finite edges may give non-finite results.
 *   out    prod_d ncell[d] values, dimension 1 fastest, in the ordering of splpak_eval_grid_*.
 * Summation order: a piece of a cell is its part inside one node cell (or below xmin, or above xmax).  The integral over
 * every product of pieces is formed by the contraction of splpak_eval_grid_*; each output is then the sum over its pieces
 * in ascending piece order, dimension 1 innermost, one accumulator per dimension, plain additions.  The bits therefore do
 * not depend on how a large call is cut into slabs (option integrate_scratch_mb: the cap of the double intermediate in
 * MB, default 256; larger calls go in slabs of consecutive cells of the last dimension, a single layer above the cap is
 * allocated whole).  REAL32: storage is float; edges and coefficients are widened first, every intermediate is double,
 * and there is one rounding at the final store.  With every mode 0 the values are the bits of splpak_eval_grid_* with
 * nderiv == NULL.
 * Status, decided on the host before any device work, in the order of splpak_eval_grid_* with ncell in place of npts:
 * 101/102/103 return without computing, `out` set to 0 (101: out[0] alone); SPLPAK_E_UNSUPPORTED: ndim > 4;
 * SPLPAK_E_BADARG: a null pointer, a negative ncell[d], a mode[d] outside 0 and 1, a product of ncell beyond int64.  If
 * any ncell[d] is 0 the validation status is returned and nothing is written.  There is no nderiv, hence no 104.
 * SPLPAK_E_NOMEM: the tables and the intermediate could not be allocated. */
int32_t splpak_integrate_grid_f64(int32_t ndim, const int64_t *ncell, const int32_t *mode, const double *axes,
                                  const double *coef, const double *xmin, const double *xmax, const int32_t *nodes,
                                  double *out);
int32_t splpak_integrate_grid_f32(int32_t ndim, const int64_t *ncell, const int32_t *mode, const float *axes,
                                  const float *coef, const float *xmin, const float *xmax, const int32_t *nodes,
                                  float *out);
/* the same on resident data; ncell, mode, xmin, xmax and nodes are host arrays.  NOT fully asynchronous: `stream` is
 * synchronised ONCE, after the pass that counts the pieces of every cell -- the counts are read back to size the tables
 * and the launches; everything after that is queued on `stream`.  (Hence not usable inside a stream capture.)  With
 * every mode 0 the call is splpak_eval_grid_dev_* and waits for nothing. */
int32_t splpak_integrate_grid_dev_f64(int32_t ndim, const int64_t *ncell /* host */, const int32_t *mode /* host, may be NULL */,
                                      const double *axes_dev, const double *coef_dev, const double *xmin, const double *xmax,
                                      const int32_t *nodes, double *out_dev, void *stream);
int32_t splpak_integrate_grid_dev_f32(int32_t ndim, const int64_t *ncell /* host */, const int32_t *mode /* host, may be NULL */,
                                      const float *axes_dev, const float *coef_dev, const float *xmin, const float *xmax,
                                      const int32_t *nodes, float *out_dev, void *stream);
/* Diagnostics, host counters of the calling thread's last splpak_integrate_grid_* call (nothing is waited for):
 * [0] slabs, [1] doubles of intermediate held (piece products and the first reduction's result), [2..5] table entries per
 * axis (the pieces; ncell[d] for an evaluated axis; 0 beyond ndim), [6] reduction launches, [7] 0.  The tables and the
 * intermediate live in the scratch of splpak_eval_grid_*, grown on demand and released by splpak_shutdown. */
int32_t splpak_debug_integrate_grid_stats(int64_t out8[8]);

/* The fit of samples given on a tensor-product grid of points: an image, a volume, a table -- the opposite direction of
 * splpak_eval_grid_*.  Returns the coefficients splcw returns for the listed Cartesian product with the weights
 * w(i0, i1, ..) = prod_d waxes_d[i_d], PROVIDED THAT FIT HAS NO CONSTRAINT ROWS: its rows are then (W_1 A_1) x ... x
 * (W_D A_D), A_d the npts[d] x nodes[d] matrix of the four window values per axis coordinate, and the solution is
 * C = (P_1 x ... x P_D) Y with P_d = (A_d^T W_d^2 A_d)^-1 A_d^T W_d^2: one streaming pass over the samples and D 7-band
 * solves along the axes of the coefficient tensor, instead of 8 (ndim + 1) bytes per sample, a sort and a factorisation.
 *   npts, axes  as for splpak_eval_grid_*: the axes back to back, in any order, repeats and values outside the box allowed;
 *   waxes       the same layout, one weight per axis coordinate; NULL: all 1 (there is no negative-first-weight sentinel);
 *   values      field k's prod npts samples at values + k*ldv, dimension 1 fastest (what splpak_eval_grid_* writes);
 *   coef        field k's ncol coefficients go to coef + k*ldcoef (the layout of splpak_refit_* and splpak_eval_fields_*).
 * The words between the fields are neither read nor written.  Sizes: k*ldv (weighted entries: k*ldw) and k*ldcoef beyond
 * 2^31 and 2^32 elements are supported, and so is a sample count prod npts beyond 2^31.
 * xtrap.  With xtrap == 0 the reference adds no constraint rows (:862).  With xtrap != 0 it adds them for data-sparse nodes
 * (:921-1046); this entry then answers only when there are none, which it decides from per-axis nearest-node histograms:
 * every coordinate must be counted in range -- k = int(dxin_d (x - xmin_d) + 0.5), truncated toward zero, in 0 .. nodes_d - 1
 * --, every weight non-negative, and with h_d(j) the sum of the weights of the coordinates with k == j and ef = 0.5 at the
 * two end nodes, 1 elsewhere:   prod_d min_j h_d(j) / ef(j)  >=  0.75 prod_d sum_j h_d(j) / prod_d (nodes_d - 1).
 * Otherwise SPLPAK_E_UNSUPPORTED with the message "the sample has data-sparse nodes (or coordinates outside the counting
 * range): constraint rows are not separable; list the points and use the point fit, or pass xtrap = 0" -- never a silent
 * fallback.  The products of per-axis sums round differently from the reference's running sums over the points: a sample
 * that sits exactly on the 0.75 threshold may be decided differently.
 * Summation order.  Per axis the coordinates are ordered by (window start, original index): the TABLE ORDER.  The spread
 * T = (A_1^T W_1^2 x ... x A_D^T W_D^2) Y is taken one dimension at a time, the last dimension first; the entry of node j
 * is  acc = 0;  acc = fma(g, y, acc)  over the coordinates whose window holds node j, in table order, with g = waxes^2 *
 * (general-form window value), rounded once.  The solves are band forward and back substitutions with the Cholesky factors
 * of N_d = A_d^T W_d^2 A_d (formed on the host, coordinates in their original order; the substitutions multiply by the
 * reciprocal of the diagonal, rounded once on the host), one line of the coefficient tensor at a time, dimension 1 first.  The bits of a
 * result therefore depend on the axes, the weights and the field alone: not on the launch shape, the number of fields, the
 * scratch cap, or the host / _dev entry.  There are no floating-point atomics.
 * Refinement against the samples, the fit's own rule: R = Y - A C (A C by the tile kernel of splpak_eval_grid_* in double,
 * into a scratch), spread, solve, add; stop when the estimated remaining error is below 1e-11, go on while the corrections
 * contract (up to 30 steps), 107 with a message -- the coefficients as they stand -- if that misses 1e-10.  A well-conditioned
 * sample costs three passes over the data: spread; evaluate and spread; stop.  Options (splpak_set_default_option or the
 * environment): fit_grid_refine = nominal steps (default 4; 0: none), fit_grid_scratch_mb = cap of the residual scratch in
 * MB (default 256; larger calls go in slabs of consecutive table positions of the last dimension, whose running sums
 * continue from slab to slab by plain sequential accumulation; a single position above the cap is allocated whole).
 * REAL32: storage is float; samples, axes and weights are widened on load, every intermediate is double, and there is one
 * rounding at the store of coef.
 * Status, decided on the host before any device work, the first failing check wins:
 *   SPLPAK_E_BADARG       npts, nodes, xmin or xmax null;
 *   101; SPLPAK_E_UNSUPPORTED (ndim > 4); 102, 103 as splcw;
 *   104                   ldcoef < ncol;
 *   105                   an npts[d] < 1;
 *   SPLPAK_E_BADARG       a product of npts beyond int64, nfields < 1, ldv < prod npts, axes, values or coef null;
 *   SPLPAK_E_UNSUPPORTED  the xtrap rule above;
 *   107                   an axis whose N_d is not numerically positive definite (a non-positive Cholesky pivot or one below
 *                         nodes_d * eps * the largest diagonal entry: too few distinct coordinates, all weights zero); the
 *                         coefficients of every field are set to 0.
 * On 101 .. 105 and the negative codes `coef` is untouched.  Then SPLPAK_E_NODEVICE / SPLPAK_E_NOMEM from the device part.
 * info (optional, 10 doubles per field): [0] data rows = prod_d (coordinates of axis d with a non-zero weight), [1] 0,
 * [2] refinement steps taken, [3] |last correction|_inf / |coef|_inf, [4] the smallest Cholesky pivot over the axes (the
 * diagonal entry before its square root), [5] seconds in the host tables and factors (of the call), [6] 0, [7] seconds on
 * the device (of the field), [8] ||W (A c - y)||_2 AS MEASURED IN THE LAST RESIDUAL PASS, i.e. for the coefficients before
 * the last correction was added (0 with refinement off), [9] 0. */
int32_t splpak_fit_grid_f64(int32_t ndim, const int64_t *npts, const double *axes, const double *waxes /* may be NULL */,
                            int32_t nfields, const double *values, int64_t ldv, const double *xmin, const double *xmax,
                            const int32_t *nodes, double xtrap, double *coef, int64_t ldcoef,
                            double *info /* 10 per field, may be NULL */);
int32_t splpak_fit_grid_f32(int32_t ndim, const int64_t *npts, const float *axes, const float *waxes /* may be NULL */,
                            int32_t nfields, const float *values, int64_t ldv, const float *xmin, const float *xmax,
                            const int32_t *nodes, float xtrap, float *coef, int64_t ldcoef,
                            double *info /* 10 per field, may be NULL */);
/* the same on resident data: axes, waxes, values and coef are device arrays; npts, xmin, xmax, nodes and info host arrays.
 * NOT asynchronous: the sum npts axis coordinates and weights are copied to the host for the tables and the status checks
 * (`stream` is synchronised once for that), and again after every refinement step and at the end of every field.  Hence
 * not usable inside a stream capture, like splpak_integrate_grid_dev_*.  On 107 the coefficients are zeroed on `stream`. */
int32_t splpak_fit_grid_dev_f64(int32_t ndim, const int64_t *npts /* host */, const double *axes_dev, const double *waxes_dev /* may be NULL */,
                                int32_t nfields, const double *values_dev, int64_t ldv, const double *xmin, const double *xmax,
                                const int32_t *nodes, double xtrap, double *coef_dev, int64_t ldcoef,
                                double *info /* host, 10 per field, may be NULL */, void *stream);
int32_t splpak_fit_grid_dev_f32(int32_t ndim, const int64_t *npts /* host */, const float *axes_dev, const float *waxes_dev /* may be NULL */,
                                int32_t nfields, const float *values_dev, int64_t ldv, const float *xmin, const float *xmax,
                                const int32_t *nodes, float xtrap, float *coef_dev, int64_t ldcoef,
                                double *info /* host, 10 per field, may be NULL */, void *stream);
/* Diagnostics.  One stage of the device part alone, host arrays, one field, no xtrap rule: stage 0: out[ncol] = T, the
 * spread of in[prod npts] = the samples; stage 1: out[ncol] = C from in[ncol] = T, the solves alone (no refinement).
 * Status as splpak_fit_grid_f64 (ldv = prod npts, ldcoef = ncol), then SPLPAK_E_BADARG for another stage. */
int32_t splpak_debug_fit_grid_stage_f64(int32_t stage, int32_t ndim, const int64_t *npts, const double *axes,
                                        const double *waxes /* may be NULL */, const double *xmin, const double *xmax,
                                        const int32_t *nodes, const double *in, double *out);
/* host counters of the calling thread's last splpak_fit_grid_* / stage call (nothing is waited for): [0] slabs of a residual
 * pass (0: refinement off), [1] doubles of residual scratch held, [2] spread launches, [3] solve launches, [4] refinement
 * steps of the last field, [5..7] 0.  The tables and intermediates live in a per-thread scratch released by splpak_shutdown. */
int32_t splpak_debug_fit_grid_stats(int64_t out8[8]);

/* The grid fit with a weight per sample: dead pixels, masked regions, NaN holes, a variance map -- weights that do not
 * factor over the axes (those that do belong to splpak_fit_grid_*, which needs no iteration).  Returns the coefficients
 * splcw returns for the listed samples OF NON-ZERO WEIGHT, provided that fit has no constraint rows: the contract of
 * splpak_fit_grid_*.
 *   weights  one per sample in the layout of `values`, a row weight as wdata of splcw is: the normal equations see its
 *            square.  Field k's weights at weights + k*ldw; ldw == 0: one array for all fields, analysed once per call;
 *            otherwise ldw >= prod npts.  A sample whose weight is exactly 0 is selected out, never multiplied: its value
 *            may be NaN or Inf.
 * Algorithm.  N = A^T diag(w^2) A with A = A_D x ... x A_1 is no Kronecker product.  N x = b is solved by preconditioned
 * conjugate gradients from a zero start: applying N is one tile pass of splpak_eval_grid_* into the slab scratch and the
 * spread passes of splpak_fit_grid_*, the first of which loads the sample's weight; the preconditioner is the separable
 * solve of splpak_fit_grid_* on M = N^_D x ... x N^_1, N^_d = A_d^T diag(m_d / S^((D-1)/D)) A_d, with m_d the marginals of
 * w^2 over the other dimensions and S their total (one pass over the weights).  For separable weights M = N and the
 * iteration ends in one or two steps.  The first solve goes to a relative preconditioned residual of 1e-11; then the
 * refinement rule of splpak_fit_grid_* unchanged, its residual A^T (w^2 o (y - A x)) taken from the samples and its
 * corrections solved to 1e-3.  The scalars of the iteration stay on the device and are read back every 5 iterations.
 * Options: fit_grid_refine, fit_grid_scratch_mb as for splpak_fit_grid_*; fit_grid_weighted_maxit = the cap of one solve's
 * iterations (default 1000): a solve that reaches it hands its iterate to the refinement rule, which decides.
 * xtrap != 0: answered only when no node is data sparse by the reference's rule node by node (:879-907): with h(j) the sum of
 * the weights of the samples whose nearest node is j (every coordinate counted in range as for splpak_fit_grid_*) and
 * ef(j) = 0.5 per dimension in which j is an end node, every h(j) / ef(j) >= 0.75 sum h / prod_d (nodes_d - 1).
 * Determinism.  The bits of a field's coefficients depend on the axes, the weights and the field alone: not on the node
 * block, the scratch cap (slabs), the number of fields, shared or per-field weights, or the host / _dev entry.  Every sum
 * has one owner and a fixed order (csrc/fitgridw.hip gives it); there are no floating-point atomics.
 * Status, the first failing check wins: the ladder of splpak_fit_grid_* with `weights` among its null checks, and
 * SPLPAK_E_BADARG also for an ldw that is neither 0 nor >= prod npts; 107 where an axis is rank deficient whatever the
 * weights.  Then, AFTER the pass over the weights (of every weight set of the call, before any coefficient is written):
 *   SPLPAK_E_BADARG       a weight that is negative or not finite ("a weight is negative or not finite");
 *   SPLPAK_E_UNSUPPORTED  the xtrap rule, with the message of splpak_fit_grid_*.
 * On these `coef` is untouched.  107 with THAT FIELD's coefficients zeroed, each with a message of its own -- the reference
 * says 107 for the same samples --: an N^_d that fails the pivot test of splpak_fit_grid_* (a singular M implies a singular
 * N); an entry of diag(N) that is not positive (a coefficient without a sample of non-zero weight in its support); a
 * breakdown of the iteration (p^T N p <= 0 or a scalar that is not finite).  107 with the coefficients as they stand where
 * the refinement rule misses 1e-10.
 * info as for splpak_fit_grid_*, except [0] = the count of non-zero weights, [4] = the smallest pivot of the
 * preconditioner's factors, [6] = [9] = 0. */
int32_t splpak_fit_grid_weighted_f64(int32_t ndim, const int64_t *npts, const double *axes, int32_t nfields, const double *values,
                                     int64_t ldv, const double *weights, int64_t ldw, const double *xmin, const double *xmax,
                                     const int32_t *nodes, double xtrap, double *coef, int64_t ldcoef,
                                     double *info /* 10 per field, may be NULL */);
int32_t splpak_fit_grid_weighted_f32(int32_t ndim, const int64_t *npts, const float *axes, int32_t nfields, const float *values,
                                     int64_t ldv, const float *weights, int64_t ldw, const float *xmin, const float *xmax,
                                     const int32_t *nodes, float xtrap, float *coef, int64_t ldcoef,
                                     double *info /* 10 per field, may be NULL */);
/* the same on resident data: axes, values, weights and coef are device arrays.  Not asynchronous, like splpak_fit_grid_dev_*:
 * `stream` is synchronised for the axes, after the pass over the weights, every 5 iterations and after every refinement step. */
int32_t splpak_fit_grid_weighted_dev_f64(int32_t ndim, const int64_t *npts /* host */, const double *axes_dev, int32_t nfields,
                                         const double *values_dev, int64_t ldv, const double *weights_dev, int64_t ldw,
                                         const double *xmin, const double *xmax, const int32_t *nodes, double xtrap, double *coef_dev,
                                         int64_t ldcoef, double *info /* host, 10 per field, may be NULL */, void *stream);
int32_t splpak_fit_grid_weighted_dev_f32(int32_t ndim, const int64_t *npts /* host */, const float *axes_dev, int32_t nfields,
                                         const float *values_dev, int64_t ldv, const float *weights_dev, int64_t ldw,
                                         const float *xmin, const float *xmax, const int32_t *nodes, float xtrap, float *coef_dev,
                                         int64_t ldcoef, double *info /* host, 10 per field, may be NULL */, void *stream);
/* Diagnostics.  One stage alone, host arrays, one field, no xtrap rule: stage 0: out[ncol] = A^T (w^2 o in[prod npts]), the
 * right-hand side; 1: out[ncol] = N in[ncol], the operator; 2: out[ncol] = M^-1 in[ncol], the preconditioner; 3:
 * out[sum npts + ncol] = the D marginals of w^2 (the axes back to back), then diag(N) (`in` is not read).  Status as
 * splpak_fit_grid_weighted_f64 (ldv = prod npts, ldw = 0, ldcoef = ncol; `out` is never zeroed), then SPLPAK_E_BADARG for
 * another stage; stages 2 and 3 also refuse a bad weight and return 107 as the fit does. */
int32_t splpak_debug_fit_grid_weighted_stage_f64(int32_t stage, int32_t ndim, const int64_t *npts, const double *axes,
                                                 const double *weights, const double *xmin, const double *xmax, const int32_t *nodes,
                                                 const double *in, double *out);
/* host counters of the calling thread's last splpak_fit_grid_weighted_* / stage call (nothing is waited for): [0] slabs of an
 * operator pass, [1] doubles of slab scratch held, [2] spread launches, [3] axis-solve launches, [4] refinement steps of the
 * last field, [5] conjugate-gradient iterations of the last field over all its solves (per solve: up to the first iterate
 * within the tolerance; up to 4 more have run when the read-back sees it), [6] solves of the last field, [7] weight analyses of
 * the call (1 with ldw == 0, nfields otherwise). */
int32_t splpak_debug_fit_grid_weighted_stats(int64_t out8[8]);

/* Many small independent fits on one node grid in one launch: a spline per spectrum, per detector row, per station time series,
 * per tile of an image, per bootstrap resample of the points.  Every problem has its own points, its own number of them, its
 * own values and weights; only ndim, nodes, xmin, xmax and xtrap are shared.  (splpak_refit_* is the route for many VALUE sets
 * on the SAME points.)
 *   offsets  nbatch + 1 of them: problem k owns the points offsets[k] .. offsets[k+1]-1 of xdata(l1xdat, *), ydata and wdata;
 *   coef     problem k's ncol coefficients go to coef + k*ldcoef, ldcoef >= ncol: the layout of splpak_refit_* and
 *            splpak_eval_fields_*.
 * Per problem: what splcw does for its points, or splcc when wdata == NULL.  A negative FIRST weight of a problem means "no
 * weights" for that problem (:581-588); a point of weight 0 contributes no row and no histogram bump (:891); the nearest-node
 * histogram, the 0.75 rule, dcwght and the derivative-constraint rows are the reference's (:862-1046), the first-derivative
 * rows at boundary nodes and the doubled mixed row in 2-D included; every problem has its own totlwt and its own sparse set.
 * There is no hist_out.
 * Algorithm.  One workgroup works on one problem from its points to its coefficients, all in its own LDS: the banded normal
 * equations A^T W^2 A + C^T C and A^T W^2 y (2-D: the smaller dimension fastest, whatever the caller's order), a Cholesky on the
 * band with the pivot test of splpak_fit_f64 (a pivot that is not positive fails), the solve, and the
 * refinement of splpak_fit_grid_* against the data and constraint rows: it stops at an estimated 1e-11, goes on for up to 30
 * steps while the corrections contract, and says 107 when that misses 1e-10.  The rows come from the window tables of the
 * single fit.  The batch is ONE launch whatever nbatch is; its workgroups stride over the problems when there are more
 * problems than workgroups.  A problem of very many points is still worked by its one workgroup, which walks all of them for
 * every band row: the entry is for many SMALL problems; splitting a large one is out of scope (use splpak_fit_*).
 * Shapes.  ndim 1 or 2, and a grid whose band, vectors and staging area fit in 64 KiB of LDS: splpak_fit_many_lds_bytes returns
 * the bytes, 8 ((hb + 5) ncol + 128 (4 ndim + 2) + 16) + 512 (ndim + 1) + ncol rounded up to 4, with hb = 3 in 1-D and
 * 3 min(nodes) + 3 in 2-D: 1-D grids up to 896 nodes; 2-D up to 12 x 12 (62 736 bytes; 12 x 11: 55 332; 13 x 12: 66 972, refused).
 * It needs no device and returns SPLPAK_E_BADARG for null nodes, ndim other than 1 or 2, or fewer than 4
 * nodes.
 * Determinism.  Every sum has one owner and a fixed order -- the owner of a band row walks the problem's points in index order
 * -- and there are no floating-point atomics.  The bits of problem k depend on its own points, values, weights and the grid
 * alone: not on nbatch, its position in the batch, its neighbours, the host / _dev entry, or the workgroup that ran it.
 * Sizes.  offsets[] (the points of the whole batch), p*l1xdat, k*ldcoef and, in the variants, k*ldcov and the index into wout
 * may pass 2^31 and 2^32: points, rows of coef and cov are addressed with 64-bit offsets (splpak_eval_many_*,
 * splpak_residuals_many_* and splpak_mad_many_* likewise).  The limits: nbatch is an int32_t and ONE problem has fewer than
 * 2^31 points.  splpak_fit_many_clip_mad_* keeps one double per point of the batch's span in device scratch.
 * Status.  Decided on the host before any device work, the first failing check wins, coef and status untouched:
 *   SPLPAK_E_BADARG (offsets, nodes, xmin or xmax null); 101; SPLPAK_E_UNSUPPORTED (ndim > 2); 102; 103; 104 (ldcoef < ncol);
 *   SPLPAK_E_BADARG (nbatch < 1, offsets that decrease, a problem of 2^31 points or more, l1xdat < ndim, xdata, ydata or coef
 *   null); SPLPAK_E_UNSUPPORTED (the LDS rule, with a message that says to loop the single fit: never a silent fallback).
 * Then per problem, status[k] (may be NULL) = 105 for a problem without points (its coefficients untouched; it is never sent
 * to the device), 107 where a pivot fails the test or the refinement rule fails (ITS coefficients set to 0; no other problem
 * is touched), otherwise 0.  Returns 0 when every problem ended in 0, otherwise the status of the lowest-numbered problem that
 * did not; SPLPAK_E_NODEVICE / SPLPAK_E_NOMEM from the device part.
 * info (10 per problem, may be NULL) as for splpak_fit_f64: [0] data rows, [1] constraint rows, [2] refinement steps, [3] last
 * correction, [4] smallest pivot, [5] [6] 0, [7] the launch's device seconds divided by the problems that ran, [8] reserr over
 * the data and constraint rows -- of the coefficients BEFORE the last correction, whose residuals the last refinement step
 * computed anyway (the correction is below 1e-8 of the coefficients and reserr is stationary at the minimiser) --, [9] 0: the
 * backward error needs |N| |x|, which the workgroup no longer holds once the band is factored.  All 0 for a problem of status
 * 105. */
int32_t splpak_fit_many_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets /* nbatch + 1 */, const double *xdata, int32_t l1xdat,
                            const double *ydata, const double *wdata /* may be NULL */, const double *xmin, const double *xmax,
                            const int32_t *nodes, double xtrap, double *coef, int64_t ldcoef, int32_t *status /* nbatch, may be NULL */,
                            double *info /* 10 per problem, may be NULL */);
/* REAL32 storage, arithmetic in double, one rounding at the store of coef */
int32_t splpak_fit_many_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets /* nbatch + 1 */, const float *xdata, int32_t l1xdat,
                            const float *ydata, const float *wdata /* may be NULL */, const float *xmin, const float *xmax,
                            const int32_t *nodes, float xtrap, float *coef, int64_t ldcoef, int32_t *status /* nbatch, may be NULL */,
                            double *info /* 10 per problem, may be NULL */);
/* the same on resident data: xdata, ydata, wdata and coef are device arrays; offsets, xmin, xmax, nodes, status and info are
 * host arrays.  Not asynchronous: `stream` is synchronised once, after the launch, for the statuses.  The offsets, the list of
 * the problems that run and their results go through the calling thread's scratch (released by splpak_shutdown): once that
 * holds the batch, no hipMalloc / hipFree: the call waits for `stream`, which waits for the thread's previous batch call where
 * that still uses the scratch, and not for other work of the device. */
int32_t splpak_fit_many_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets /* host */, const double *xdata_dev, int32_t l1xdat,
                                const double *ydata_dev, const double *wdata_dev /* may be NULL */, const double *xmin, const double *xmax,
                                const int32_t *nodes, double xtrap, double *coef_dev, int64_t ldcoef, int32_t *status /* host */,
                                double *info /* host */, void *stream);
int32_t splpak_fit_many_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets /* host */, const float *xdata_dev, int32_t l1xdat,
                                const float *ydata_dev, const float *wdata_dev /* may be NULL */, const float *xmin, const float *xmax,
                                const int32_t *nodes, float xtrap, float *coef_dev, int64_t ldcoef, int32_t *status /* host */,
                                double *info /* host */, void *stream);
int64_t splpak_fit_many_lds_bytes(int32_t ndim, const int32_t *nodes);
/* host counters of the calling thread's last splpak_fit_many_* call (nothing is waited for): [0] workgroups launched, [1] LDS
 * bytes per workgroup, [2] launches of the call, [3] problems sent to the device, [4] problems refused with 105, [5] the
 * largest number of refinement steps over the problems, [6] device allocations (hipMalloc) the call made: 0 for a _dev call
 * whose scratch was large enough, [7] 0.  After a splpak_fit_many_clip_* or splpak_fit_many_clip_mad_* call the same slots ([5] over the LAST fits), and
 * [7] the largest number of fits any problem ran. */
int32_t splpak_debug_fit_many_stats(int64_t out8[8]);

/* Sigma-clipped batch fits: the clipping loop splpak_fit_many_* -> splpak_residuals_many_* -> set the rejected weights to 0 ->
 * splpak_fit_many_* ..., run to its end for every problem in ONE launch.  The workgroup that owns a problem fits it, forms its
 * residuals, rejects, and fits again until a pass rejects nothing or maxpass passes have run; it then takes its next problem,
 * so a problem that settles after one pass costs one pass, whatever its neighbours need.  The arguments are those of
 * splpak_fit_many_* with, after xtrap, klo, khi (the thresholds below and above the fit, in units of the rms of the weighted
 * residuals), maxpass, and wout: the weights the problem ended with, addressed by the global point index like wdata -- the mask
 * is wout[i] == 0 where wdata[i] was not --; and, after info, clip (4 per problem, host, may be NULL).
 * The rule, per problem, is part of the contract; T is the storage type and all arithmetic is in double, every operation
 * rounded on its own (no contraction):
 *   1 start    w_i = 1 for every point when wdata == NULL or the problem's first weight is negative, else (double) wdata[i];
 *              wout[i] = (T) w_i.  The first-weight decision is taken once, from wdata, before any pass.
 *   2 fit      (pass j = 0, 1, ..) coefficients, status and info are exactly what splpak_fit_many_* returns for the problem with
 *              wout as its weights.  If that is 107: stop; the coefficients are 0 and wout stays as that fit saw it.
 *   3 limit    if j == maxpass: stop.
 *   4 resid    over the points with wout[i] != 0: cnt and S exactly as splpak_residuals_many_* defines them on the coefficients
 *              as stored (rounded to T, the caller's node order): r = (double) y - f, t = w r, tt = t t; lane l of 64 adds tt
 *              for p = l, l + 64, .. in ascending order, then the butterfly o = 32 .. 1.  v = S / cnt.
 *   5 reject   a counted point is rejected where (t > 0 and tt > khi^2 v) or (t < 0 and tt > klo^2 v); khi^2 and klo^2 are
 *              formed once in double (the _f32 entries widen klo and khi first).  No point rejected: stop.  Otherwise
 *              wout[i] = (T) 0 for the rejected points and step 2 with j + 1.  Rejected points never return.
 * The result is therefore bit for bit what that loop of the three entries gives with step 5 applied on the host (REAL32: where
 * no decision hinges on the rounding of resid to float, which the entry does not do).  klo >= 1 and khi >= 1 are required
 * (+inf switches a side off): the counted point of smallest tt then always survives, so a problem cannot clip itself empty; it
 * can still end in 107 by becoming rank-deficient at xtrap = 0.  The coefficients returned always belong to the wout returned.
 * maxpass = 0 is splpak_fit_many_* plus step 1.
 *   clip + 4k  [0] residual passes that ran, [1] points rejected in total, [2] points counted by the last fit, [3] v of the
 *              last residual pass (0 if none ran); all 0 for status 105.
 *   info       what splpak_fit_many_* reports for the LAST fit of the problem, slot for slot; [7] the launch's device seconds
 *              divided by the problems that ran.
 * Shapes: exactly those of splpak_fit_many_* (splpak_fit_many_lds_bytes is the rule; the loop needs no LDS beyond the fit's).
 * Status: the ladder of splpak_fit_many_* in its order, with, in the SPLPAK_E_BADARG group of the null data pointers: wout
 * null, wout == wdata, maxpass < 0, klo or khi below 1 or NaN.  wout overlapping wdata in part is the caller's fault and is not
 * detected.  A problem without points: 105, never sent to the device, coef and wout untouched.
 * Determinism as splpak_fit_many_*: the bits of problem k depend on its own points, values, weights, the grid and (klo, khi,
 * maxpass) alone: not on the batch, its position, the workgroup, or the host / _dev entry.  No atomics. */
int32_t splpak_fit_many_clip_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets /* nbatch + 1 */, const double *xdata,
                                 int32_t l1xdat, const double *ydata, const double *wdata /* may be NULL */, const double *xmin,
                                 const double *xmax, const int32_t *nodes, double xtrap, double klo, double khi, int32_t maxpass,
                                 double *wout, double *coef, int64_t ldcoef, int32_t *status /* nbatch, may be NULL */,
                                 double *info /* 10 per problem, may be NULL */, double *clip /* 4 per problem, may be NULL */);
/* REAL32 storage, arithmetic in double */
int32_t splpak_fit_many_clip_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets /* nbatch + 1 */, const float *xdata,
                                 int32_t l1xdat, const float *ydata, const float *wdata /* may be NULL */, const float *xmin,
                                 const float *xmax, const int32_t *nodes, float xtrap, float klo, float khi, int32_t maxpass,
                                 float *wout, float *coef, int64_t ldcoef, int32_t *status /* nbatch, may be NULL */,
                                 double *info /* 10 per problem, may be NULL */, double *clip /* 4 per problem, may be NULL */);
/* the same on resident data, like splpak_fit_many_dev_*: xdata, ydata, wdata, wout and coef are device arrays, the rest host
 * arrays.  One launch; `stream` is synchronised once, for the statuses; no hipMalloc / hipFree once the calling thread's
 * scratch holds the batch. */
int32_t splpak_fit_many_clip_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets /* host */, const double *xdata_dev,
                                     int32_t l1xdat, const double *ydata_dev, const double *wdata_dev /* may be NULL */,
                                     const double *xmin, const double *xmax, const int32_t *nodes, double xtrap, double klo, double khi,
                                     int32_t maxpass, double *wout_dev, double *coef_dev, int64_t ldcoef, int32_t *status /* host */,
                                     double *info /* host */, double *clip /* host */, void *stream);
int32_t splpak_fit_many_clip_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets /* host */, const float *xdata_dev,
                                     int32_t l1xdat, const float *ydata_dev, const float *wdata_dev /* may be NULL */,
                                     const float *xmin, const float *xmax, const int32_t *nodes, float xtrap, float klo, float khi,
                                     int32_t maxpass, float *wout_dev, float *coef_dev, int64_t ldcoef, int32_t *status /* host */,
                                     double *info /* host */, double *clip /* host */, void *stream);

/* Robustly clipped batch fits: the clipping loop on a median / MAD scale, with rejected points allowed to return, run to its end
 * for every problem in ONE launch.  The rms of splpak_fit_many_clip_* is inflated by the outliers it is meant to find, and a run
 * of neighbouring outliers drags the first fit so that good points beside it are rejected in pass 0 and, there, lost for good.
 * Here the centre is the median of the weighted residuals, the scale 1.4826 times their MAD, and with regrow != 0 every point
 * is judged again in every pass against its ORIGINAL weight.  The arguments are those of splpak_fit_many_clip_* with regrow
 * after maxpass and 6 numbers per problem in clip.
 * The rule, per problem, is part of the contract; T is the storage type and all arithmetic is in double, every operation
 * rounded on its own (no contraction):
 *   1 start    as step 1 of splpak_fit_many_clip_*: w0_i = 1 for every point when wdata == NULL or the problem's first weight is
 *              negative, else (double) wdata[i]; wout[i] = (T) w0_i.  The first-weight decision is taken once, from wdata.
 *   2 fit      (pass j = 0, 1, ..) exactly splpak_fit_many_* with wout as the weights.  If that is 107: stop; the coefficients
 *              are 0 and wout stays as that fit saw it.
 *   3 limit    if j == maxpass: stop.
 *   4 scale    t_i = w0_i r_i for every point with w0_i != 0, r_i = (double) y_i - f_i with f_i the window sum of
 *              splpak_eval_many_* on the coefficients as stored (rounded to T, the caller's node order): what the rms rule uses.
 *              med and MAD as splpak_mad_many_* defines them over the t_i of the points with wout[i] != 0.
 *              s = 1.482602218505602 MAD.  If s == 0: stop (an exact fit of more than half the points rejects nothing).
 *   5 decide   e_i = t_i - med; hi = khi s and lo = klo s, each formed once (the _f32 entries widen klo and khi first).  A
 *              candidate is out where e_i > hi or -e_i > lo.  The candidates are the points with wout[i] != 0 when
 *              regrow == 0, and the points with w0_i != 0 when regrow != 0.  wout[i] = (T) 0 for an out candidate, (T) w0_i for
 *              every other candidate.  If no weight changed between zero and non-zero: stop.  Otherwise step 2 with j + 1.
 * klo >= 1 and khi >= 1 are required (+inf switches a side off).  When s > 0 at least ceil(cnt / 2) of the counted points have
 * |e| <= MAD < s, so a pass keeps at least half and a problem cannot clip itself empty; it can still end in 107 by becoming
 * rank-deficient at xtrap = 0.  With regrow the loop may oscillate: maxpass bounds it, and clip[0] == maxpass shows it.  The
 * coefficients returned always belong to the wout returned.  maxpass = 0 is splpak_fit_many_* plus step 1.
 *   clip + 6k  [0] residual passes that ran, [1] points with w0 != 0 and wout == 0 at the end, [2] points counted by the last
 *              fit, [3] s of the last residual pass, [4] its med, [5] points returned in total (a weight that went from zero back
 *              to w0; 0 when regrow == 0); all 0 for status 105.
 *   info       as splpak_fit_many_clip_*: the LAST fit of the problem.
 * The result is bit for bit the loop splpak_fit_many_* -> splpak_residuals_many_* (resid) -> t = w0 resid on the host ->
 * splpak_mad_many_* with wsel = the current weights -> steps 4 and 5 on the host -> splpak_fit_many_* ... (REAL32: where no
 * decision hinges on the rounding of resid to float, which the entry does not do).
 * Shapes: exactly those of splpak_fit_many_* (splpak_fit_many_lds_bytes is the rule; the selection counts in the stage area of
 * the fit's LDS and needs no byte beyond it).  The t_i of a pass live in the calling thread's device scratch, a double per
 * point of the batch.
 * Status: the ladder of splpak_fit_many_clip_* in its order (wout null, wout == wdata, maxpass < 0, klo or khi below 1 or NaN
 * in the SPLPAK_E_BADARG group of the null data pointers; any regrow is valid).  A problem without points: 105, never sent to the
 * device, coef and wout untouched.
 * Determinism as splpak_fit_many_*: the bits of problem k depend on its own points, values, weights, the grid and (klo, khi,
 * maxpass, regrow) alone: not on the batch, its position, the workgroup, or the host / _dev entry.  No floating-point atomics
 * (the selection's integer counts: splpak_mad_many_*). */
int32_t splpak_fit_many_clip_mad_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets /* nbatch + 1 */, const double *xdata,
                                     int32_t l1xdat, const double *ydata, const double *wdata /* may be NULL */, const double *xmin,
                                     const double *xmax, const int32_t *nodes, double xtrap, double klo, double khi, int32_t maxpass,
                                     int32_t regrow, double *wout, double *coef, int64_t ldcoef, int32_t *status /* nbatch, may be NULL */,
                                     double *info /* 10 per problem, may be NULL */, double *clip /* 6 per problem, may be NULL */);
/* REAL32 storage, arithmetic in double */
int32_t splpak_fit_many_clip_mad_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets /* nbatch + 1 */, const float *xdata,
                                     int32_t l1xdat, const float *ydata, const float *wdata /* may be NULL */, const float *xmin,
                                     const float *xmax, const int32_t *nodes, float xtrap, float klo, float khi, int32_t maxpass,
                                     int32_t regrow, float *wout, float *coef, int64_t ldcoef, int32_t *status /* nbatch, may be NULL */,
                                     double *info /* 10 per problem, may be NULL */, double *clip /* 6 per problem, may be NULL */);
/* the same on resident data, like splpak_fit_many_clip_dev_*: xdata, ydata, wdata, wout and coef are device arrays, the rest
 * host arrays.  One launch; `stream` is synchronised once, for the statuses; no hipMalloc / hipFree once the calling thread's
 * scratch holds the batch. */
int32_t splpak_fit_many_clip_mad_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets /* host */, const double *xdata_dev,
                                         int32_t l1xdat, const double *ydata_dev, const double *wdata_dev /* may be NULL */,
                                         const double *xmin, const double *xmax, const int32_t *nodes, double xtrap, double klo,
                                         double khi, int32_t maxpass, int32_t regrow, double *wout_dev, double *coef_dev, int64_t ldcoef,
                                         int32_t *status /* host */, double *info /* host */, double *clip /* host */, void *stream);
int32_t splpak_fit_many_clip_mad_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets /* host */, const float *xdata_dev,
                                         int32_t l1xdat, const float *ydata_dev, const float *wdata_dev /* may be NULL */,
                                         const float *xmin, const float *xmax, const int32_t *nodes, float xtrap, float klo, float khi,
                                         int32_t maxpass, int32_t regrow, float *wout_dev, float *coef_dev, int64_t ldcoef,
                                         int32_t *status /* host */, double *info /* host */, double *clip /* host */, void *stream);

/* splpak_fit_many_* with the uncertainty of the fit: the entries of Z = (A^T W^2 A + C^T C)^-1, the inverse of the matrix the
 * fit factors, that a prediction variance a(x)^T Z a(x) can touch.  The arguments are those of splpak_fit_many_* with cov, ldcov
 * after ldcoef.
 *   Meaning.  With w_i = 1 / sigma_i (wdata holds the reciprocal standard deviations) and no constraint rows (xtrap == 0, or no
 *            data-sparse node: info[1] == 0), Z is the covariance of the coefficients.  With constraint rows, those rows act as
 *            unit-variance pseudo-observations and Z never understates: the sandwich covariance is Z - Z C^T C Z, which is no
 *            larger than Z (the sandwich form is not computed).  Where the weights are only relative, the caller scales Z by the
 *            reduced chi-square info[8]^2 / (info[0] + info[1] - ncol), which it forms itself.
 *   Layout.  Problem k's stencil is at cov + k*ldcov, ldcov >= splpak_fit_many_cov_len(ndim, nodes) = ncol * hst with
 *            hst = (7^ndim + 1) / 2: 4 words per node in 1-D, 25 in 2-D.  Entry [i*hst + code] = Z[i, i + o], where i is the
 *            coefficient's index in coef (the caller's node order, dimension 0 fastest), o_d in -3 .. 3 the offset of the column's
 *            node in dimension d, and code = sum_d (o_d + 3) 7^d <= the centre (7^ndim - 1) / 2, i.e. the column is not after the
 *            row: the lower half of the stencil, the diagonal in its last slot.  A cubic tensor B-spline row has a 4^ndim window,
 *            so every pair of coefficients a window holds is in it.  A slot whose column i + o lies outside the grid holds 0;
 *            words between the length and ldcov are not written.  (The internal band order, smaller dimension fastest, does not
 *            show.)
 *   Results. coef, status and info are bit for bit those of splpak_fit_many_* on the same problem.  A problem of status 107 gets
 *            cov = 0 as it gets coef = 0; a problem of status 105 has its cov untouched.
 * Algorithm.  The workgroup that fitted the problem still holds the band Cholesky factor L in LDS (refinement does not change
 * it).  Takahashi's recurrence forms the entries of Z inside the band from it, column by column from the last one up, in place:
 *   Z[j,i] = (delta_ij / L_ii - sum_{k=i+1..min(i+hb,ncol-1)} Z[j,k] L[k,i]) / L_ii,  j = i .. min(i+hb, ncol-1)
 * (the divisions by L_ii are multiplications by its reciprocal, formed once per column).  No LDS beyond the fit's:
 * splpak_fit_many_lds_bytes stays the rule, 12 x 12 nodes run.  1-D: one thread with the live 3 x 3 block in registers; 2-D: lane
 * t of one wave owns Z[i+t,i] and walks k in ascending order, the diagonal's sum is a fixed butterfly over the lanes.  Every sum
 * has one owner and a fixed order, there are no floating-point atomics: the bits of a problem's cov depend on its own points,
 * values, weights and the grid alone (not on nbatch, its position, the workgroup or the host / _dev entry).
 * Status: the ladder of splpak_fit_many_* in its order, with ldcov < the length on the 104 rung (beside ldcoef < ncol) and
 * cov == NULL in the last SPLPAK_E_BADARG group (beside coef == NULL).  The LDS rule is unchanged.
 * Not offered by the clipped entry: run splpak_fit_many_clip_* first and this entry with its wout as the weights. */
int32_t splpak_fit_many_cov_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets /* nbatch + 1 */, const double *xdata,
                                int32_t l1xdat, const double *ydata, const double *wdata /* may be NULL */, const double *xmin,
                                const double *xmax, const int32_t *nodes, double xtrap, double *coef, int64_t ldcoef, double *cov,
                                int64_t ldcov, int32_t *status /* nbatch, may be NULL */, double *info /* 10 per problem, may be NULL */);
/* REAL32 storage, arithmetic in double, one rounding at the store of coef and of cov */
int32_t splpak_fit_many_cov_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets /* nbatch + 1 */, const float *xdata, int32_t l1xdat,
                                const float *ydata, const float *wdata /* may be NULL */, const float *xmin, const float *xmax,
                                const int32_t *nodes, float xtrap, float *coef, int64_t ldcoef, float *cov, int64_t ldcov,
                                int32_t *status /* nbatch, may be NULL */, double *info /* 10 per problem, may be NULL */);
/* the same on resident data, like splpak_fit_many_dev_*: xdata, ydata, wdata, coef and cov are device arrays, the rest host
 * arrays.  One launch; `stream` is synchronised once, for the statuses; no hipMalloc / hipFree once the calling thread's scratch
 * holds the batch.  (The host entries stage cov, compact, through device memory of the call.) */
int32_t splpak_fit_many_cov_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets /* host */, const double *xdata_dev,
                                    int32_t l1xdat, const double *ydata_dev, const double *wdata_dev /* may be NULL */,
                                    const double *xmin, const double *xmax, const int32_t *nodes, double xtrap, double *coef_dev,
                                    int64_t ldcoef, double *cov_dev, int64_t ldcov, int32_t *status /* host */, double *info /* host */,
                                    void *stream);
int32_t splpak_fit_many_cov_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets /* host */, const float *xdata_dev,
                                    int32_t l1xdat, const float *ydata_dev, const float *wdata_dev /* may be NULL */, const float *xmin,
                                    const float *xmax, const int32_t *nodes, float xtrap, float *coef_dev, int64_t ldcoef,
                                    float *cov_dev, int64_t ldcov, int32_t *status /* host */, double *info /* host */, void *stream);
/* words of one problem's cov: ncol (7^ndim + 1) / 2.  Needs no device; SPLPAK_E_BADARG where splpak_fit_many_lds_bytes says it
 * (nodes null, ndim other than 1 or 2, fewer than 4 nodes). */
int64_t splpak_fit_many_cov_len(int32_t ndim, const int32_t *nodes);

/* The prediction variance of a batch of small fits at each problem's own points, one launch: the arguments of splpak_eval_many_*
 * with cov, ldcov (as splpak_fit_many_cov_* wrote them) in the place of coef, ldcoef.
 *   out[i] = a^T Z a, where a is the window row splpak_eval_many_* forms for query i with the same nderiv -- the 4^ndim products
 *   of its factor tables -- and Z comes from the stencil of the problem that owns i.  With a derivative pattern this is the
 *   variance of that derivative.  It is the variance, not its root, and it is not clamped (rounding may leave a tiny negative
 *   number where a row vanishes).  The _f32 entries read cov as float, widen it, sum in double and round once at the store.
 * ndim is 1 or 2 and any grid is accepted (there is no LDS rule).
 * Algorithm.  One thread per query over the concatenated list, the owner search of splpak_eval_many_*.  The window entries are
 * numbered e = q0 + 4 q1 (dimension 0 fastest); the order of the double sum is part of the contract: acc = 0; for e = 0 ..
 * 4^ndim - 1: r = (0.5 a_e) Z[p_e,p_e], then r = fma(a_f, Z[p_e,p_f], r) for f = 0 .. e-1 ascending, then acc = fma(a_e, r, acc);
 * out = 2 acc.  Every symmetric pair is read once, from the row of the later node: 4 words per node in 1-D (10 in all), 136
 * distinct words of 16 stencil rows in 2-D, from global memory.  The bits depend on the query and its problem's cov alone.
 * Status: the ladder of splpak_eval_many_* in its order with three changes: ndim > 2 gives SPLPAK_E_UNSUPPORTED where ndim > 4
 * does there; ldcov < splpak_fit_many_cov_len is where ldcoef < ncol is; cov null is where coef null is.  The zeroing of out on
 * 101 / 102 / 103 and the clamped 104 are the same. */
int32_t splpak_eval_many_var_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets /* nbatch + 1 */, const double *xq, int32_t ldxq,
                                 const int32_t *nderiv /* may be NULL */, const double *cov, int64_t ldcov, const double *xmin,
                                 const double *xmax, const int32_t *nodes, double *out);
int32_t splpak_eval_many_var_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets /* nbatch + 1 */, const float *xq, int32_t ldxq,
                                 const int32_t *nderiv /* may be NULL */, const float *cov, int64_t ldcov, const float *xmin,
                                 const float *xmax, const int32_t *nodes, float *out);
/* the same on resident data: xq, cov and out are device arrays.  Asynchronous on `stream` exactly as splpak_eval_many_dev_*: the
 * call only enqueues, and the one thing it uploads is `offsets`, into the calling thread's scratch. */
int32_t splpak_eval_many_var_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets /* host */, const double *xq_dev, int32_t ldxq,
                                     const int32_t *nderiv /* host, may be NULL */, const double *cov_dev, int64_t ldcov,
                                     const double *xmin, const double *xmax, const int32_t *nodes, double *out_dev, void *stream);
int32_t splpak_eval_many_var_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets /* host */, const float *xq_dev, int32_t ldxq,
                                     const int32_t *nderiv /* host, may be NULL */, const float *cov_dev, int64_t ldcov,
                                     const float *xmin, const float *xmax, const int32_t *nodes, float *out_dev, void *stream);

/* The evaluation side of splpak_fit_many_*: problem k's coefficients at problem k's own points, one launch whatever nbatch is
 * (a spline per spectrum resampled on its own abscissa).  splpak_eval_fields_* evaluates every set at ONE shared batch of points
 * and splpak_eval_* takes one set per call; a host loop of nbatch such calls is latency bound.  The layouts are those of
 * splpak_fit_many_*:
 *   offsets  nbatch + 1 of them: problem k owns the global indices offsets[k] .. offsets[k+1]-1 of xq(ldxq, *) and out;
 *            offsets[0] need not be 0;
 *   coef     problem k's ncol coefficients are at coef + k*ldcoef, ldcoef >= ncol, problems without queries included: exactly
 *            where splpak_fit_many_* (or splpak_refit_*) put them;
 *   nderiv   one pattern for all problems (NULL: values).
 * ndim is 1 to 4 and any grid is accepted (there is no LDS rule).  out[i] is the very value splpak_eval_* returns for query i
 * with the coefficients of the problem that owns i and the same nderiv (identical bits: the same factor table and the same sum
 * over the window; nothing is shared between problems).  Words of `out` outside [offsets[0], offsets[nbatch]), rows of xq
 * beyond ndim and words of `coef` between the sets are neither read nor written.
 * Algorithm.  One thread per query over the concatenated list, so 10^5 problems of 8 queries and 4 problems of 10^6 are balanced
 * alike.  A wave looks its first query's problem up in the uploaded offsets; where its last query has the same problem (the
 * common case) all its lanes take that coefficient set, otherwise each lane searches between the two.  Problems without
 * queries, and runs of them, are stepped over.  How the problem was found does not enter the arithmetic.
 * Status, decided on the host before any device work, the first failing check wins:
 *   SPLPAK_E_BADARG       offsets, nodes, xmin or xmax null; then nbatch < 1 or offsets that decrease;
 *   101, then SPLPAK_E_UNSUPPORTED (ndim > 4), then 102 / 103 as splpak_eval_f64 -- on 101 / 102 / 103 the results
 *                         out[offsets[0] .. offsets[nbatch]) are set to 0 (if `out` is not null), on the others nothing is written;
 *   SPLPAK_E_BADARG       ldxq < ndim or ldcoef < ncol;
 *   no queries at all     0, or 104 for an nderiv outside 0..2; nothing is written and the data pointers are not looked at;
 *   SPLPAK_E_BADARG       xq, coef or out null.
 * 104 is reported but the values are computed with nderiv clamped to 0..2 (:1190-1194).
 * The host forms stage through the device: the span of the batch's queries alone and (nbatch-1)*ldcoef + ncol coefficients. */
int32_t splpak_eval_many_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets /* nbatch + 1 */, const double *xq, int32_t ldxq,
                             const int32_t *nderiv /* may be NULL */, const double *coef, int64_t ldcoef, const double *xmin,
                             const double *xmax, const int32_t *nodes, double *out);
/* REAL32 storage, arithmetic in double, as splpak_eval_f32 */
int32_t splpak_eval_many_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets /* nbatch + 1 */, const float *xq, int32_t ldxq,
                             const int32_t *nderiv /* may be NULL */, const float *coef, int64_t ldcoef, const float *xmin,
                             const float *xmax, const int32_t *nodes, float *out);
/* the same on resident data: xq, coef and out are device arrays; offsets, nderiv, xmin, xmax and nodes are host arrays.
 * Asynchronous on `stream`: the call only enqueues -- no read-back, no synchronisation of the stream, and once the calling
 * thread's scratch holds nbatch + 1 offsets no hipMalloc / hipFree.  The one thing it uploads is `offsets`, into that scratch
 * (released by splpak_shutdown); `offsets` has been read when the call returns. */
int32_t splpak_eval_many_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets /* host */, const double *xq_dev, int32_t ldxq,
                                 const int32_t *nderiv /* host, may be NULL */, const double *coef_dev, int64_t ldcoef,
                                 const double *xmin, const double *xmax, const int32_t *nodes, double *out_dev, void *stream);
int32_t splpak_eval_many_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets /* host */, const float *xq_dev, int32_t ldxq,
                                 const int32_t *nderiv /* host, may be NULL */, const float *coef_dev, int64_t ldcoef,
                                 const float *xmin, const float *xmax, const int32_t *nodes, float *out_dev, void *stream);

/* The residual pass of a clipping loop on a batch of small fits (fit_many -> residuals_many -> set the rejected weights to 0 ->
 * fit_many; splpak_fit_many_clip_* above runs that whole loop in one launch, with S as defined here): residuals at every
 * problem's own points and four numbers per problem, in one launch.  Layouts as above, with
 * xdata(l1xdat, *), ydata, wdata and resid addressed by the global index.  For point i, local index p = i - offsets[k], of
 * problem k:
 *   f_i      the double window sum splpak_eval_many_* forms for it (value pattern), before any rounding;
 *   r_i      (double) y_i - f_i;   resid[i] = (T) r_i, written for EVERY point, a weight of 0 included (a caller clips on it);
 *   w_i      1 for every point of the problem when wdata == NULL or the problem's FIRST weight is negative (as
 *            splpak_fit_many_*), else (double) wdata[i].  A point with w_i == 0 is selected out of the statistics and never
 *            multiplied: its value may be NaN.
 *   stats + 4k   [0] the points counted, [1] S = sum (w_i r_i)^2, [2] m = max |w_i r_i|, [3] the smallest local index p that
 *            attains m; [3] = -1 and [1] = [2] = 0 when nothing is counted.
 * The order of S is part of the contract: lane l of 64 starts from 0 and adds, for p = l, l + 64, l + 128, ... in ascending
 * order, the product t*t with t = w_i*r_i -- every multiplication and every addition rounded on its own, no contraction --, and
 * the 64 lane sums are combined by a butterfly: for o = 32, 16, .., 1 every lane adds the sum of lane (l xor o) to its own.
 * The bits of a problem's four numbers therefore depend on its own points, values, weights and coefficients alone: not on
 * nbatch, its position, its neighbours, the launch shape or the host / _dev entry.  There are no floating-point atomics.
 * Non-finite values among the counted points may give non-finite or unspecified [1..3].
 * Algorithm.  One wave per problem, the waves stride over the problems; the wave reads x, y and w once, evaluates, writes the
 * residual and keeps its lane accumulators.  A problem of very many points is walked by its one wave: the entry is for many
 * SMALL problems, as splpak_fit_many_* is.
 * resid or stats may be NULL, not both.  Status, decided on the host before any device work, the first failing check wins, and
 * on every one of them nothing is written:
 *   SPLPAK_E_BADARG (offsets, nodes, xmin or xmax null; nbatch < 1; offsets that decrease); 101; SPLPAK_E_UNSUPPORTED
 *   (ndim > 4); 102; 103; 104 (ldcoef < ncol, as splpak_fit_many_* says it); SPLPAK_E_BADARG (l1xdat < ndim; xdata, ydata or
 *   coef null; resid and stats both null).
 * A batch without points returns 0 with stats filled as for problems without points. */
int32_t splpak_residuals_many_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets /* nbatch + 1 */, const double *xdata,
                                  int32_t l1xdat, const double *ydata, const double *wdata /* may be NULL */, const double *coef,
                                  int64_t ldcoef, const double *xmin, const double *xmax, const int32_t *nodes,
                                  double *resid /* may be NULL */, double *stats /* 4 per problem, may be NULL */);
/* REAL32 storage: resid is float, the arithmetic and stats stay double */
int32_t splpak_residuals_many_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets /* nbatch + 1 */, const float *xdata,
                                  int32_t l1xdat, const float *ydata, const float *wdata /* may be NULL */, const float *coef,
                                  int64_t ldcoef, const float *xmin, const float *xmax, const int32_t *nodes,
                                  float *resid /* may be NULL */, double *stats /* 4 per problem, may be NULL */);
/* the same on resident data: xdata, ydata, wdata, coef, resid and stats are device arrays; offsets, xmin, xmax and nodes are host
 * arrays.  Asynchronous on `stream` exactly as splpak_eval_many_dev_*: stats stays in the caller's device memory. */
int32_t splpak_residuals_many_dev_f64(int32_t ndim, int32_t nbatch, const int64_t *offsets /* host */, const double *xdata_dev,
                                      int32_t l1xdat, const double *ydata_dev, const double *wdata_dev /* may be NULL */,
                                      const double *coef_dev, int64_t ldcoef, const double *xmin, const double *xmax,
                                      const int32_t *nodes, double *resid_dev /* may be NULL */, double *stats_dev /* may be NULL */,
                                      void *stream);
int32_t splpak_residuals_many_dev_f32(int32_t ndim, int32_t nbatch, const int64_t *offsets /* host */, const float *xdata_dev,
                                      int32_t l1xdat, const float *ydata_dev, const float *wdata_dev /* may be NULL */,
                                      const float *coef_dev, int64_t ldcoef, const float *xmin, const float *xmax,
                                      const int32_t *nodes, float *resid_dev /* may be NULL */, double *stats_dev /* may be NULL */,
                                      void *stream);
/* Robust batch clipping, the selection: the median and the MAD (median of the absolute deviations from the median) of every
 * problem's segment of `values`, in one launch.  values is addressed by the global point index (problem k owns
 * offsets[k] .. offsets[k+1]-1), wsel likewise and may be NULL: a point is counted where wsel[i] != 0, every point when wsel is
 * NULL.  A value under a zero of wsel is never read as a number and may be NaN.  Definitions, all in double, part of the
 * contract:
 *   key      k_i = (double) values[i] + 0.0, so -0 counts as +0;
 *   sort     the cnt counted keys ascending into s[0 .. cnt);
 *   med      s[(cnt-1)/2] for odd cnt, else 0.5 (s[cnt/2 - 1] + s[cnt/2]): one addition, one multiplication, each rounded on its
 *            own -- the bits of numpy.median;
 *   MAD      d_i = |k_i - med| (one rounded subtraction), and the same median over the d_i;
 *   stats + 4k   [0] cnt, [1] med, [2] MAD, [3] 0; all 0 when nothing is counted.
 * A NaN among the counted values gives unspecified med and MAD.
 * Determinism: med and MAD are exact order statistics.  Their bits depend on the multiset of the problem's counted values alone:
 * not on the order of the values, nbatch, the problem's position, its neighbours, the launch shape or the host / _dev entry.
 * There are no floating-point atomics; the counts of the selection are integers added with LDS atomics, whose result does not
 * depend on the order.
 * Algorithm.  One wave per problem, the waves stride over the problems.  A double is mapped to a 64-bit key of the same order
 * and the key of the middle rank is found most significant byte first: 8 sweeps over the problem's values with a 256-bin
 * histogram in LDS (16 sweeps for med and MAD, one more each where an even count needs the next key above).  No scratch: the
 * values are read from the caller's array and widened on load.  The entry is for many SMALL problems.
 * Status, decided on the host before any device work, nothing written on a failure: SPLPAK_E_BADARG for offsets null,
 * nbatch < 1, offsets that decrease, values null, stats null.  A batch without points returns 0 with zeros. */
int32_t splpak_mad_many_f64(int32_t nbatch, const int64_t *offsets /* nbatch + 1 */, const double *values,
                            const double *wsel /* may be NULL */, double *stats /* 4 per problem */);
/* REAL32 storage: values and wsel are float, the keys and stats double */
int32_t splpak_mad_many_f32(int32_t nbatch, const int64_t *offsets /* nbatch + 1 */, const float *values,
                            const float *wsel /* may be NULL */, double *stats /* 4 per problem */);
/* the same on resident data: values, wsel and stats are device arrays, offsets a host array.  Asynchronous on `stream` exactly
 * as splpak_residuals_many_dev_*: stats stays in the caller's device memory. */
int32_t splpak_mad_many_dev_f64(int32_t nbatch, const int64_t *offsets /* host */, const double *values_dev,
                                const double *wsel_dev /* may be NULL */, double *stats_dev, void *stream);
int32_t splpak_mad_many_dev_f32(int32_t nbatch, const int64_t *offsets /* host */, const float *values_dev,
                                const float *wsel_dev /* may be NULL */, double *stats_dev, void *stream);
/* host counters of the calling thread's last splpak_eval_many_*, splpak_eval_many_var_* splpak_residuals_many_* or splpak_mad_many_* call (nothing is waited for):
 * [0] workgroups launched, [1] launches of the call, [2] queries / points sent, [3] problems, [4] eval_many: the queries one
 * sweep of the launch covers (the launch strides over the rest); residuals_many: 0 (a sweep covers [0] problems, one wave
 * each), [5] 1 for eval_many, 2 for residuals_many, 3 for eval_many_var (the other slots as eval_many), 4 for mad_many (the other slots as
 * residuals_many), [6] [7] 0.  All 0 after a call its ladder refused. */
int32_t splpak_debug_eval_many_stats(int64_t out8[8]);

/* Several coefficient sets at the same points in one call: the evaluation half of splpak_refit_* / splpak_plan_refit_dev
 * (the components of a velocity, a time series on fixed sensors, bootstrap replicas), which otherwise takes one
 * splpak_eval_* call per field -- each reading the coordinates, building the factor tables and, for a large batch on a
 * 3-D / 4-D grid, sorting the queries by grid region again.  Here all of that is done once.
 *   coef   field k has its ncol coefficients at coef + k*ldcoef, ldcoef >= ncol: the layout refit writes;
 *   out    its nq results go to out + k*ldout, ldout >= nq;
 *   nderiv one pattern for all fields (NULL: values).
 * out[k*ldout + i] is the very value splpak_eval_* returns for query i with field k's coefficients (identical bits: the
 * same factor table and the same sum over the window, field by field; no partial sum is shared between fields).  The
 * words of `coef` and `out` between the fields are neither read nor written.  Sizes: k*ldcoef, k*ldout and nq*ldxq
 * beyond 2^31 and 2^32 elements are supported on every route (the limits of splpak_eval_dev_* apply to nq).
 * Status, decided on the host before any device work, the first failing check wins:
 *   SPLPAK_E_BADARG       nodes, xmin or xmax null; then nfields < 1, nq < 0 or ldout < nq;
 *   101, then SPLPAK_E_UNSUPPORTED (ndim > 4), then 102 / 103 as splpak_eval_f64 -- on 101 / 102 / 103 the nq results of
 *                         every field are set to 0 (if `out` is not null), on the others nothing is written;
 *   SPLPAK_E_BADARG       ldxq < ndim or ldcoef < ncol;
 *   nq == 0               0, or 104 for an nderiv outside 0..2; nothing is written;
 *   SPLPAK_E_BADARG       xq, coef or out null.
 * 104 is reported but the values are computed with nderiv clamped to 0..2 (:1190-1194).
 * The host forms stage through the device: (nfields-1)*ldcoef + ncol coefficients go up, the results come back field by field. */
int32_t splpak_eval_fields_f64(int32_t ndim, int64_t nq, const double *xq, int32_t ldxq, const int32_t *nderiv,
                               int32_t nfields, const double *coef, int64_t ldcoef,
                               const double *xmin, const double *xmax, const int32_t *nodes,
                               double *out, int64_t ldout);
/* REAL32 storage, arithmetic in double, as splpak_eval_f32 */
int32_t splpak_eval_fields_f32(int32_t ndim, int64_t nq, const float *xq, int32_t ldxq, const int32_t *nderiv,
                               int32_t nfields, const float *coef, int64_t ldcoef,
                               const float *xmin, const float *xmax, const int32_t *nodes,
                               float *out, int64_t ldout);
/* the same on resident data (asynchronous on `stream`); nderiv, xmin, xmax and nodes are host arrays */
int32_t splpak_eval_fields_dev_f64(int32_t ndim, int64_t nq, const double *xq_dev, int32_t ldxq,
                                   const int32_t *nderiv /* host, may be NULL */,
                                   int32_t nfields, const double *coef_dev, int64_t ldcoef,
                                   const double *xmin, const double *xmax, const int32_t *nodes,
                                   double *out_dev, int64_t ldout, void *stream);
int32_t splpak_eval_fields_dev_f32(int32_t ndim, int64_t nq, const float *xq_dev, int32_t ldxq,
                                   const int32_t *nderiv /* host, may be NULL */,
                                   int32_t nfields, const float *coef_dev, int64_t ldcoef,
                                   const float *xmin, const float *xmax, const int32_t *nodes,
                                   float *out_dev, int64_t ldout, void *stream);
/* Diagnostics: host-side counters of the calling thread's last fields call (no device is asked, nothing is waited for).
 * out3[0] the route: 0 no call yet, 1 the direct fields kernel (one thread per query, every field's window summed from one
 *         factor table), 2 the shared sort (queries sorted by grid region once, every field evaluated from LDS tiles),
 *         3 one single-field evaluation per field (nfields == 1, and large batches on grids the shared sort does not
 *         take: 2-D, more than 64 (4-D: 256) regions, no room for its scratch);
 * out3[1] the sorting (place) passes it launched itself: 1 on route 2, else 0;
 * out3[2] the evaluation kernels it launched: 1 on route 1, nfields on route 2; on route 3 the single-field evaluations. */
int32_t splpak_debug_eval_fields_stats(int64_t out3[3]);

/* Device-side synthetic inputs of SURVEY 8d (Park-Miller stream, seed 42):
 * points first_point .. first_point+ndata-1; any of the outputs may be NULL.
 * xdata_dev is written with leading dimension ndim.  Queries continue the stream
 * after `ndata_before` data points. */
int32_t splpak_synth_points_f64(int32_t ndim, int64_t first_point, int64_t ndata,
                                double *xdata_dev, double *ydata_dev, double *wdata_dev,
                                void *stream);
int32_t splpak_synth_queries_f64(int32_t ndim, int64_t ndata_before, int64_t first_query,
                                 int64_t nq, double *xq_dev, void *stream);

/* Diagnostics: solve A x = b for a symmetric positive definite band matrix with
 * the library's blocked band Cholesky (no refinement).  `a_lower` is the dense
 * column-major n x n matrix on the HOST, of which only the lower triangle within
 * `halfbw` of the diagonal is read.  Returns 0, or 107 if a pivot is not
 * positive.  Exists so the factorisation kernels (f64 MFMA trailing update, panel
 * solve, band sweeps) can be tested in isolation against LAPACK. */
int32_t splpak_debug_spd_band_solve_f64(int32_t n, int32_t halfbw, const double *a_lower,
                                        const double *b, double *x);

/* Diagnostics: the normal equations the plan's last fit assembled (after the all-reduce of a sharded fit), in the caller's
 * column numbering and dimension order.  nst_ref: [ncol][(7^ndim + 1) / 2], row-major; slot `code` of row i holds N(i, i + o)
 * for the column offset o in [-3,3]^ndim with code = sum_d (o_d + 3) 7^d (dimension 0 fastest), only the slots with
 * code <= (7^ndim - 1) / 2; slots whose column lies outside the grid are 0.  rhs: [ncol], A^T W^2 y.  Returns 0,
 * SPLPAK_E_BADARG for a null argument, SPLPAK_E_UNSUPPORTED when there is nothing assembled to return (a rows-only plan, no
 * fit yet, a 4-D fit the iteration answered without assembling, a failed fit, or a splpak_debug_plan_solve since the fit). */
int32_t splpak_debug_plan_normal_equations(const splpak_plan *plan, double *nst_ref, double *rhs);

/* Diagnostics: how the Gram pass of the plan's last assembly was launched (csrc/gram.hip launch_gram).  The cells are worked slab
 * by slab, a slab being as many whole hyper-rows of cells along the slowest internal dimension as the Gram scratch holds
 * (SPLPAK_GRAM_SCRATCH_MB); in a 2-D or 3-D slab a wave owns a run of consecutive cells.  out6: [0] slabs, [1] hyper-rows per
 * slab, [2] cells and [3] run of every slab but the last, [4] cells and [5] run of the last slab (= [2], [3] with one slab).  A
 * run of 0: the grid's cell kernel does not work in runs (1-D, 4-D, SPLPAK_GRAM_VALU).  Returns 0, SPLPAK_E_BADARG for a null
 * argument, SPLPAK_E_UNSUPPORTED where splpak_debug_plan_normal_equations has nothing to return. */
int32_t splpak_debug_plan_gram_shape(const splpak_plan *plan, int32_t *out6);

/* Diagnostics: the binning of the data points by window (csrc/binpoints.hip launch_bin_points), the first stage of every
 * assembly, on its own: no plan, no factor storage, no normal equations -- the scratch of the binning alone, allocated as a plan
 * allocates it and released before the entry returns.  Everything comes back RAW, in the library's internal numbering, so that
 * no translation can hide a mistake.  Inputs on the host as for splpak_fit_f64 (xdata(l1xdat, ndata), wdata may be NULL; a
 * negative first weight has no special meaning here).  SPLPAK_BIN_ATOMIC and SPLPAK_NO_REORDER are read from the process
 * defaults / the environment.  Outputs (all required):
 *   perm, cells, cellstride [ndim]: internal dimension d is the caller's dimension perm[d]; windows per dimension and their strides;
 *   *route: 0 the atomic route (SPLPAK_BIN_ATOMIC, or a grid of more than 4095^2 cells), 1 the stable partition in one level, 2 in
 *           two levels with tiles of at most 256 cells, 3 with tiles of up to 4095 cells; *cpt: cells per tile (0: too many cells);
 *   key [ndata]: cell of every point, sum_d ws_d cellstride[d], ncell = prod cells for a point of zero weight (not placed);
 *           (on the atomic route too: scratch made for that route keeps its re-sort out of the key array);
 *   offset [ncell + 1]: first sorted position of every cell; *placed = offset[ncell];
 *   idx [ndata]: original index of the sorted points (the first *placed entries are set; likewise below);
 *   xs [ndim][ndata] (plane d, internal order, at xs + d * ndata), ys, ws [ndata]: the sorted copies;
 *   *nrows_data: the scalar the fit reports as its number of data rows.
 * Returns 0; 101/102/103 (grid checks); SPLPAK_E_BADARG for a null argument, ndata < 1 or l1xdat < ndim; SPLPAK_E_NOMEM;
 * SPLPAK_E_NODEVICE, with the message of the failing call, when a launch or a copy fails or the placed count is impossible. */
int32_t splpak_debug_bin_points(int32_t ndim, const int32_t *nodes, const double *xmin, const double *xmax, int64_t ndata,
                                const double *xdata, int32_t l1xdat, const double *ydata, const double *wdata, int32_t *perm,
                                int32_t *cells, int32_t *cellstride, int32_t *route, int32_t *cpt, int32_t *key, int32_t *offset,
                                int32_t *idx, double *xs, double *ys, double *ws, int64_t *placed, double *nrows_data);

/* Diagnostics: loads the caller's matrix (layout of splpak_debug_plan_normal_equations) into the plan and solves N x = b with
 * the plan's own factorisation, exactly as a fit runs it -- expansion into the factor storage, factorisation, one solve --
 * without iterative refinement.  b, x: [ncol] in the caller's column order; minpiv (may be NULL): the smallest pivot.
 * Returns 0; 107 if N is not positive definite (x = 0; the plan stays usable); SPLPAK_E_BADARG for a null argument;
 * SPLPAK_E_UNSUPPORTED for a plan without a factorisation (iteration only) or a rank of a sharded / distributed fit. */
int32_t splpak_debug_plan_solve(splpak_plan *plan, const double *nst_ref, const double *b, double *x, double *minpiv);

/* Diagnostics: the passes over the ROWS of the plan's last successful single-rank fit (its binned points, constraint weights and
 * data-sparse flags are still in the plan), evaluated at the caller's coefficients.  coef, rho, den: [ncol] on the host, in the
 * caller's column order.  rho = A^T W (W y - W A coef) - C^T C coef, computed by
 *   which = 0: the pass the refinement calls (and the iteration, as its operator), with y;
 *   which = 1: the diagnostics pass a fit ends with for info[8] / info[9] (tile form or cell by cell, honouring
 *              SPLPAK_RESIDUAL_CELLS); only this one also returns *ssq, the sum of squared row residuals (info[8]^2), and in den
 *              the backward error's denominators the fit would use (from the half stencil, or from the rows where the fit did
 *              not assemble the normal equations);
 *   which = 2: the operator form of the iteration, y = 0.
 * den and ssq may be NULL; for which = 0 and 2 they are set to 0.  The entry calls the functions the fit calls.  It overwrites only
 * scratch every fit rewrites.  Returns 0; SPLPAK_E_BADARG for a null plan, coef or rho or another `which`; SPLPAK_E_UNSUPPORTED when
 * there is no completed fit (none yet, a failed one, or a splpak_debug_plan_solve since) or the plan is a rank of a sharded /
 * multi-GPU fit. */
int32_t splpak_debug_plan_rows_gradient(splpak_plan *plan, const double *coef, int32_t which, double *rho, double *den, double *ssq);

/* Diagnostics: z = M^-1 r with the iteration's preconditioner as the plan's last fit prepared it; r, z: [ncol] on the host, in the
 * caller's column order.  part = 0: the whole of it, as the iteration applies it; 1: the separable part alone; 2: the block-Jacobi
 * boxes alone (zero when the fit dropped them or the plan has none).  Returns 0; SPLPAK_E_BADARG for a null argument or another
 * `part`; SPLPAK_E_UNSUPPORTED for a plan without the iteration or a last fit that never prepared it. */
int32_t splpak_debug_plan_precondition(splpak_plan *plan, int32_t part, const double *r, double *z);

/* Diagnostics: host copies of what the separable part multiplies by.  _pcg_tables: for dimension `dim` of the CALLER's dimension
 * order, *n_out = its node count n, V: [n][n] row-major (component i of eigenvector j at V[i * n + j]) and VT, the transposed copy
 * the kernels read in the other direction; V and VT may be NULL (a sizing call).  _pcg_diagonal: dinv [ncol], caller's column
 * order, the reciprocal diagonal in the eigenbasis as the last fit prepared it:
 *     separable part:  z = (kron_k V_k) (dinv * ((kron_k V_k^T) r)).
 * Return 0, SPLPAK_E_BADARG (null argument, dim outside the grid), SPLPAK_E_UNSUPPORTED (no iteration / never prepared). */
int32_t splpak_debug_plan_pcg_tables(const splpak_plan *plan, int32_t dim, double *V, double *VT, int32_t *n_out);
int32_t splpak_debug_plan_pcg_diagonal(const splpak_plan *plan, double *dinv);

/* Diagnostics (host only): the fronts of the nested-dissection elimination tree of a grid (as splpak_debug_nd_tree builds it),
 * in elimination order (postorder, the root last).  *nfronts: their number F.  With max_fronts < F nothing else is written (a
 * sizing call); otherwise per front depth (root 0), parent (-1 for the root), w (own variables) and h (border variables),
 * unpadded; per node in the caller's column numbering (either may be NULL): the front that owns it and its elimination position.
 * Returns 0, 101/102/103 (grid checks) or a negative SPLPAK_E_* code. */
int32_t splpak_debug_nd_fronts(int32_t ndim, const int32_t *nodes, int32_t split_min, int32_t *nfronts, int32_t max_fronts,
                               int32_t *depth, int32_t *parent, int32_t *w, int32_t *h, int32_t *front_of_node, int32_t *pos_of_node);

/* Diagnostics (host only, no device needed): builds the nested-dissection elimination tree the fit uses for
 * large 3-D / 4-D grids (csrc/ndtree.hpp; separators 3 nodes thick because the normal equations of the
 * window rule src/splpak.F90:821-827 couple nodes up to 3 apart) and reports its size.  split_min <= 0: the
 * library default; check != 0: verify the tree's invariants (slow on big grids).  out16:
 *   [0] fronts  [1] depth  [2] bytes of factor panels  [3] bytes of the two Schur arenas  [4] bytes of all Schur
 *   buffers of one fit  [5] flop of the blocked factorisation (padded)  [6] flop without padding  [7] largest
 *   separator  [8] largest border  [9] 256x256 diagonal blocks  [10] local vector length  [11] own rows (padded)
 *   [12] border rows (padded)  [13] bytes of the diagonal-block inverses.
 * Returns 0, 101/102/103 (grid checks) or a negative SPLPAK_E_* code. */
int32_t splpak_debug_nd_tree(int32_t ndim, const int32_t *nodes, int32_t split_min, int32_t check, double *out16);

/* Diagnostics (host only): the elimination schedule of the nested-dissection factorisation (csrc/ndtree.hpp NdSchedule, round 5)
 * and the Schur-buffer arena it needs.  cut = 0: one stage per tree depth (rounds 3-4); cut > 0: the fronts above depth `cut` one
 * by one in postorder, the subtrees below it one after the other.  packed != 0: Schur buffers as packed lower triangles.  The
 * schedule's invariants are verified (children before parents, live buffers disjoint).  out8: [0] stages, [1] bytes of the
 * arena (peak of the allocation), [2] bytes of all Schur buffers of one fit, [3] bytes of the factor panels, [4] cut, [5] depth. */
int32_t splpak_debug_nd_schedule(int32_t ndim, const int32_t *nodes, int32_t split_min, int32_t cut, int32_t packed, double *out8);

/* Diagnostics (host only): how the nested-dissection factorisation of a grid is distributed over `ngpus` GPUs by the
 * one-process multi-GPU fit (splpak_mplan_*, splpak_fit_multi_f64; csrc/ndtree.hpp NdPartition): the subtrees below tree
 * depth ceil(log2 ngpus) belong to one rank each, the fronts above are distributed by block columns (chunk < 1: 1).
 * out_per_rank8 (8 doubles per rank): [0] bytes of everything the factorisation keeps on that GPU = [1] panels of its
 * subtrees + [2] its Schur arenas + [3] its block columns of the top fronts + [4] block inverses + [5] receive buffers,
 * solve vectors and index tables; [6] padded flop of its subtrees, [7] of its share of the top fronts.
 * out8 (optional): [0] depth of the cut, [1] top fronts, [2] their block steps, [3] bytes of the largest panel that
 * travels, [4] bytes of the all-reduced normal equations every rank also holds, [5] fronts, [6] depth, [7] total flop. */
int32_t splpak_debug_nd_partition(int32_t ndim, const int32_t *nodes, int32_t split_min, int32_t ngpus, int32_t chunk,
                                  double *out_per_rank8, double *out8);

/* Diagnostics (host only): the four basis values of the window of x (1-D grid of `nodes` nodes on [xmin, xmax];
 * src/splpak.F90:206-389, window rule :1201-1209) for n points, (a) as the evaluation kernels compute them -- the closed
 * form of an interior window, the closed form with the end functions put in next to an end of the grid, the general
 * form elsewhere (csrc/basis.hpp; form_out: 0 / 1 / 2) -- and (b) in the general form throughout.  ws_out: first node of
 * the window.  used4 / general4: 4 values per point.  Returns 0, 102/103 (grid checks) or a negative SPLPAK_E_* code. */
int32_t splpak_debug_window_values(int32_t nodes, double xmin, double xmax, int64_t n, const double *x, int32_t *ws_out,
                                   double *used4, double *general4, int32_t *form_out);

/* Releases the calling thread's internal HIP streams, events, queues and evaluation scratch
 * (created lazily and kept for reuse).  Optional; plans stay valid. */
void splpak_shutdown(void);

/* Evaluation strategy of the calling thread (results are bit-identical either way):
 *   mode 0  automatic: batches of >= 2^20 queries on 3-D and 4-D grids of more than 32768 nodes
 *           take the binned path, everything else the direct one
 *   mode 1  direct: one thread per query, coefficients gathered from global memory
 *   mode 2  binned: queries are sorted by grid region, `chunk` queries at a time (0 = 2^24), and
 *           each region is evaluated from a copy of its coefficients in LDS; needs
 *           chunk*(8*ndim+4) bytes of device scratch, kept until splpak_shutdown
 * There is no counterpart in the reference (splde evaluates one point per call, :1089-1240). */
int32_t splpak_set_eval_mode(int32_t mode, int64_t chunk);

/* Human-readable text for the last negative status on this thread. */
int32_t splpak_last_error_message(char *buf, int32_t buflen);

/* Library / device identification: writes e.g. "gfx950:sramecc+:xnack-" */
int32_t splpak_device_name(char *buf, int32_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* SPLPAK_HIP_H */
