// The host side of a batch of small fits, the same for every variant of splpak_fit_many_* (fitmany*.hip): a variant fills a
// FitManyCall -- the caller's arguments and which outputs it adds to them -- and gives the one launch of its kernel;
// fit_many_entry runs the call in stages: the ladder of checks in the order the header gives, all on the host; the tables of
// the call; the staging of a host entry's arrays; the launch; the scatter of the results.  The tables -- offsets, problem list,
// results -- live in the calling thread's scratch (manyhost.hpp), each held by a ScratchUse to the end of the call: a _dev call
// whose scratch is large enough allocates and frees nothing.  The host entries stage the span of the batch's points and the
// compact coefficients through device memory of the call.
#pragma once
#include "plan.hpp"
#include "fitmany.hpp"
#include "manyhost.hpp"

#include <new>
#include <vector>

namespace splpak {

// What every entry takes before its outputs, in the order of the C arguments
template <typename T>
struct FitManyIn {
    int32_t ndim, nbatch;
    const int64_t *offsets;
    const T *xdata;
    int32_t l1xdat;
    const T *ydata, *wdata, *xmin, *xmax;
    const int32_t *nodes;
    double xtrap;
};

template <typename T>
struct FitManyCall {
    FitManyIn<T> in;
    bool dev;                          // the arrays of points, coefficients and weights are device memory, the call runs on st
    hipStream_t st;
    T *coef;
    int64_t ldcoef;
    int32_t *status;                   // may be null
    double *info;                      // may be null
    const char *what;                  // the call as an error text names it: "a batch of fits"
    // what a variant adds
    bool has_wout = false;             // a weight per point comes back in `wout`: staged and copied back like the span
    T *wout = nullptr;
    bool has_cov = false;              // `cov`, ldcov words per problem, beside `coef`: staged and scattered like it
    T *cov = nullptr;
    int64_t ldcov = 0;
    int nextra = 0;                    // doubles the kernel leaves per problem after the FM_* slots ..
    double *extra = nullptr;           // .. which go to extra[k * nextra ..] (may be null)
    const char *refusal = nullptr;     // the variant's own SPLPAK_E_BADARG, its rung after the shared one (null: none)
};

// The refusal of a clipping variant (FitManyCall::refusal), or null
template <typename T>
const char *clip_refusal(const T *wout, const T *wdata, int32_t maxpass, double klo, double khi)
{
    if (!wout || wout == wdata || maxpass < 0 || !(klo >= 1.0) || !(khi >= 1.0))
        return "wout null or the same array as wdata, maxpass < 0, or klo or khi below 1 (or NaN)";
    return nullptr;
}

// the node grid of a call, in the internal order (reorder) or the caller's; build_grid's status
template <typename T>
int fit_many_grid(const FitManyIn<T> &in, bool reorder, Grid &g)
{
    double xmin[MAXD] = {0, 0, 0, 0}, xmax[MAXD] = {0, 0, 0, 0};
    for (int d = 0; d < in.ndim; ++d) { xmin[d] = (double)in.xmin[d]; xmax[d] = (double)in.xmax[d]; }
    return build_grid(in.ndim, in.nodes, xmin, xmax, g, nullptr, reorder);
}

// Where the launch reads and writes: the caller's arrays (_dev) or their copies in the memory of the call
template <typename T>
struct FitManyDev {
    const T *xd, *yd, *wd;
    T *wo, *cd, *cvd;
    long long ldcov;
};

// What comes back from the device, on the host: the result blocks and, for a host entry, the compact outputs
template <typename T>
struct FitManyBack {
    size_t nres;                       // doubles of a result block
    std::vector<double> res;
    std::vector<T> ch, wh, covh;
};

// checks: the ladder; fills a.g and a.sh
template <typename T>
int32_t fit_many_checks(const FitManyCall<T> &c, FitManyArgs &a)
{
    const FitManyIn<T> &in = c.in;
    if (!in.offsets || !in.nodes || !in.xmin || !in.xmax) { set_error("null argument"); return SPLPAK_E_BADARG; }
    if (in.ndim < 1) return 101;
    if (in.ndim > 2) {
        set_error("splpak_fit_many_* fits 1-D and 2-D grids: loop splpak_fit_* over the problems instead");
        return SPLPAK_E_UNSUPPORTED;
    }
    if (int rc = fit_many_grid(in, true, a.g)) {      // 102, 103
        if (rc == SPLPAK_E_UNSUPPORTED) set_error("more than 2^30 nodes is not supported");
        return rc;
    }
    if (c.ldcoef < a.g.ncol || (c.has_cov && c.ldcov < fit_many_cov_len(in.ndim, a.g.ncol))) return 104;
    bool ok = in.nbatch >= 1 && in.l1xdat >= in.ndim && in.xdata && in.ydata && c.coef && (!c.has_cov || c.cov);
    for (int k = 0; ok && k < in.nbatch; ++k)
        ok = in.offsets[k + 1] >= in.offsets[k] && in.offsets[k + 1] - in.offsets[k] < (1LL << 31);
    if (!ok) {
        set_error("nbatch < 1, offsets that decrease, a problem of 2^31 points or more, l1xdat < ndim or a null pointer");      // (cov included)
        return SPLPAK_E_BADARG;
    }
    if (c.refusal) { set_error(c.refusal); return SPLPAK_E_BADARG; }
    a.sh = fit_many_shape(in.ndim, in.nodes);
    if (a.sh.bytes > FITMANY_LDS_BUDGET) {
        set_error("the grid needs more than 64 KiB of LDS per problem (splpak_fit_many_lds_bytes): loop splpak_fit_* over the problems instead");
        return SPLPAK_E_UNSUPPORTED;
    }
    return 0;
}

// tables: the problems that have points, in order; status 105 for the others, info and extra zeroed
template <typename T>
std::vector<int> fit_many_tables(const FitManyCall<T> &c)
{
    const FitManyIn<T> &in = c.in;
    const size_t nextra = (size_t)c.nextra;
    std::vector<int> plist;
    for (int k = 0; k < in.nbatch; ++k) {
        const bool empty = in.offsets[k + 1] == in.offsets[k];
        if (!empty) plist.push_back(k);
        if (c.status) c.status[k] = empty ? 105 : 0;
        if (c.info) for (int j = 0; j < 10; ++j) c.info[(size_t)k * 10 + j] = 0.0;
        if (c.extra) for (size_t j = 0; j < nextra; ++j) c.extra[(size_t)k * nextra + j] = 0.0;
    }
    return plist;
}

// staging: the tables of the call into the thread's scratch (the caller holds their ScratchUse); for a host entry the span of
// the batch's points alone and room for the outputs of the problems that run, back to back, in cs.  Completes a, fills d.
template <typename T>
hipError_t fit_many_stage(const FitManyCall<T> &c, const std::vector<int> &plist, ManySpan sp, const FitManyBack<T> &h, CallStage &cs,
                          FitManyArgs &a, FitManyDev<T> &d)
{
    const FitManyIn<T> &in = c.in;
    const size_t need[2] = {sizeof(int) * plist.size(), sizeof(double) * h.res.size()};
    hipError_t e = many_offsets_upload(in.offsets, in.nbatch, c.st, &a.offsets);
    if (e == hipSuccess) e = scratch_begin(t_fit_many_tables, need, c.st);
    // (pageable memory: the copy has left `plist` when the call returns)
    if (e == hipSuccess) e = hipMemcpyAsync(t_fit_many_tables.buf[0], plist.data(), need[0], hipMemcpyHostToDevice, c.st);
    a.nrun = (int)plist.size();
    a.plist = t_fit_many_tables.as<int>(0);
    a.result = t_fit_many_tables.as<double>(1);
    a.l1xdat = in.l1xdat;
    a.xtrap = in.xtrap;
    a.base = 0;
    a.ldcoef = c.ldcoef;
    a.compact = 0;
    d = {in.xdata, in.ydata, in.wdata, c.wout, c.coef, c.cov, c.ldcov};
    if (!c.dev) {
        if (e == hipSuccess) e = stage_span(cs, sp, in.xdata, in.l1xdat, in.ydata, in.wdata, &d.xd, &d.yd, &d.wd);
        if (e == hipSuccess && !cs.get(&d.cd, h.ch.size())) e = hipErrorOutOfMemory;
        if (e == hipSuccess && c.has_wout && !cs.get(&d.wo, h.wh.size())) e = hipErrorOutOfMemory;
        if (e == hipSuccess && c.has_cov && !cs.get(&d.cvd, h.covh.size())) e = hipErrorOutOfMemory;
        d.ldcov = fit_many_cov_len(in.ndim, a.g.ncol);
        a.base = sp.lo;
        a.ldcoef = a.g.ncol;
        a.compact = 1;
    }
    return e;
}

// scatter: the results back to the host and to the caller's status, info, extra and (a host entry) coef, cov and wout;
// t_fit_many_stats[5] and [7]; the status of the call
template <typename T>
int32_t fit_many_scatter(const FitManyCall<T> &c, const std::vector<int> &plist, ManySpan sp, FitManyBack<T> &h, const FitManyArgs &a,
                         const FitManyDev<T> &d, double seconds)
{
    const FitManyIn<T> &in = c.in;
    const int nrun = a.nrun, ncol = a.g.ncol;
    const long long covlen = fit_many_cov_len(in.ndim, ncol);
    const size_t nextra = (size_t)c.nextra;
    hipError_t e = hipMemcpyAsync(h.res.data(), a.result, sizeof(double) * h.res.size(), hipMemcpyDeviceToHost, c.st);
    if (e == hipSuccess && !c.dev) e = hipMemcpyAsync(h.ch.data(), d.cd, sizeof(T) * h.ch.size(), hipMemcpyDeviceToHost, c.st);
    if (e == hipSuccess && !h.covh.empty()) e = hipMemcpyAsync(h.covh.data(), d.cvd, sizeof(T) * h.covh.size(), hipMemcpyDeviceToHost, c.st);
    if (e == hipSuccess && !h.wh.empty()) e = hipMemcpyAsync(h.wh.data(), d.wo, sizeof(T) * h.wh.size(), hipMemcpyDeviceToHost, c.st);
    const hipError_t waited = hipStreamSynchronize(c.st);      // (also after a failed copy: the one before it may still write `res`)
    if (e == hipSuccess) e = waited;
    if (e != hipSuccess) return many_status(e, c.what, 0);
    long long maxsteps = 0, maxfits = 0;
    int first_failed = -1;
    for (int r = 0; r < nrun; ++r) {
        const int k = plist[(size_t)r];
        const double *v = h.res.data() + (size_t)r * h.nres;
        const int sk = v[FM_STATUS] != 0.0 ? 107 : 0;
        if (c.status) c.status[k] = sk;
        if (sk != 0 && first_failed < 0) first_failed = k;
        if ((long long)v[FM_STEPS] > maxsteps) maxsteps = (long long)v[FM_STEPS];
        if ((long long)v[FM_SPARE] > maxfits) maxfits = (long long)v[FM_SPARE];
        if (c.info) {
            double *ik = c.info + (size_t)k * 10;
            ik[0] = v[FM_ROWS];
            ik[1] = v[FM_CROWS];
            ik[2] = v[FM_STEPS];
            ik[3] = v[FM_LASTREL];
            ik[4] = v[FM_MINPIV];
            ik[7] = seconds / (double)nrun;
            ik[8] = v[FM_RESERR];
        }
        if (c.extra)
            for (size_t j = 0; j < nextra; ++j) c.extra[(size_t)k * nextra + j] = v[FM_RESULT + j];
        if (!c.dev) {
            T *ck = c.coef + (long long)k * c.ldcoef;
            for (int i = 0; i < ncol; ++i) ck[i] = h.ch[(size_t)r * (size_t)ncol + (size_t)i];
            if (c.has_cov) {
                T *vk = c.cov + (long long)k * c.ldcov;
                for (long long i = 0; i < covlen; ++i) vk[i] = h.covh[(size_t)r * (size_t)covlen + (size_t)i];
            }
        }
    }
    // (every point of the span belongs to a problem that ran)
    for (size_t i = 0; i < h.wh.size(); ++i) c.wout[(size_t)sp.lo + i] = h.wh[i];
    t_fit_many_stats[5] = maxsteps;
    t_fit_many_stats[7] = maxfits;
    int rc = 0;
    for (int k = 0; k < in.nbatch && rc == 0; ++k) {
        if (in.offsets[k + 1] == in.offsets[k]) rc = 105;
        else if (k == first_failed) rc = 107;
    }
    if (first_failed >= 0) {
        char buf[200];
        snprintf(buf, sizeof buf, "problem %d of the batch: a pivot failed the rank test or the refinement missed 1e-10 (too few points?)", first_failed);
        set_error(buf);
    }
    return rc;
}

// One call.  launch(a, xd, yd, wd, wo, cd, cvd, ldcov, st, &seconds) -> 0 or SPLPAK_E_* is the variant's kernel on the staged
// arrays (wo and cvd null where the call has none): one launch, synchronised, *seconds its device time.  Device scratch of its
// own it begins itself, adding the allocations to t_fit_many_stats[6].
template <typename T, typename Launch>
int32_t fit_many_entry(const FitManyCall<T> &c, Launch &&launch)
{
    for (int j = 0; j < 8; ++j) t_fit_many_stats[j] = 0;
    FitManyArgs a{};
    if (int32_t rc = fit_many_checks(c, a)) return rc;
    try {
        const std::vector<int> plist = fit_many_tables(c);
        const size_t nrun = plist.size(), ncol = (size_t)a.g.ncol;
        t_fit_many_stats[1] = a.sh.bytes;
        t_fit_many_stats[3] = (long long)nrun;
        t_fit_many_stats[4] = c.in.nbatch - (long long)nrun;
        if (nrun == 0) return 105;

        if (int r = device_ready()) return r;
        const ManySpan sp = many_span(c.in.offsets, c.in.nbatch);
        FitManyBack<T> h{FM_RESULT + (size_t)c.nextra, {}, {}, {}, {}};
        h.res.resize(nrun * h.nres);
        h.ch.resize(c.dev ? 0 : nrun * ncol);
        h.wh.resize(c.dev || !c.has_wout ? 0 : (size_t)sp.n);
        h.covh.resize(c.dev || !c.has_cov ? 0 : nrun * (size_t)fit_many_cov_len(c.in.ndim, a.g.ncol));
        const long long allocs_before = t_many_offsets.allocs + t_fit_many_tables.allocs;
        const ScratchUse<1> use_offsets{t_many_offsets, c.st};
        const ScratchUse<2> use_tables{t_fit_many_tables, c.st};
        CallStage cs;      // (the host entries alone)
        FitManyDev<T> d{};
        const hipError_t e = fit_many_stage(c, plist, sp, h, cs, a, d);
        t_fit_many_stats[6] = t_many_offsets.allocs + t_fit_many_tables.allocs - allocs_before + (long long)cs.held.size();
        if (e != hipSuccess) return many_status(e, c.what, 0);

        double seconds = 0.0;
        if (int r = launch(a, d.xd, d.yd, d.wd, d.wo, d.cd, d.cvd, d.ldcov, c.st, &seconds)) return r;

        return fit_many_scatter(c, plist, sp, h, a, d, seconds);
    } catch (const std::bad_alloc &) {
        set_error("the host tables of the batch of fits could not be allocated");
        return SPLPAK_E_NOMEM;
    }
}

}  // namespace splpak
