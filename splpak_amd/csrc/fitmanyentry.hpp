// The host side of a batch of small fits, shared by splpak_fit_many_* (fitmanyapi.hip), splpak_fit_many_clip_*
// (fitmanyclipapi.hip), splpak_fit_many_clip_mad_* (fitmanymadapi.hip) and splpak_fit_many_cov_* (fitmanycovapi.hip; its cov is staged and scattered like coef): the ladder of checks in the order the header gives, all on the host; then the one launch
// (fitmany.hip / fitmanyclip.hip / fitmanymad.hip) and the scatter of its results.  The tables of a call -- offsets, problem list, results --
// live in the calling thread's scratch (manyhost.hpp), each held by a ScratchUse to the end of the call: a _dev call whose
// scratch is large enough allocates and frees nothing.  The host entries stage the span of the batch's points and the compact
// coefficients through device memory of the call.
#pragma once
#include "plan.hpp"
#include "fitmany.hpp"
#include "manyhost.hpp"

#include <new>
#include <vector>

namespace splpak {

// What the clipped entries add to the arguments of splpak_fit_many_* (null: the plain fit)
template <typename T>
struct ClipSpec {
    double klo, khi;
    int32_t maxpass;
    T *wout;
    double *clip;      // nclip per problem, may be null
    int nclip = 4;     // the numbers after the FM_* slots of a problem's result block
    bool mad = false;  // the median / MAD rule of splpak_fit_many_clip_mad_* (6 clip numbers) instead of the rms rule
    int32_t regrow = 0;
};

// What the covariance entries (splpak_fit_many_cov_*) add (null: no covariance)
template <typename T>
struct CovSpec {
    T *cov;
    int64_t ldcov;
};

template <typename T>
int32_t fit_many_entry(bool dev, int32_t ndim, int32_t nbatch, const int64_t *offsets, const T *xdata, int32_t l1xdat, const T *ydata,
                       const T *wdata, const T *xmin_t, const T *xmax_t, const int32_t *nodes, double xtrap, T *coef, int64_t ldcoef,
                       int32_t *status, double *info, hipStream_t st, const ClipSpec<T> *clip = nullptr, const CovSpec<T> *covs = nullptr)
{
    for (int j = 0; j < 8; ++j) t_fit_many_stats[j] = 0;
    if (!offsets || !nodes || !xmin_t || !xmax_t) { set_error("null argument"); return SPLPAK_E_BADARG; }
    if (ndim < 1) return 101;
    if (ndim > 2) {
        set_error("splpak_fit_many_* fits 1-D and 2-D grids: loop splpak_fit_* over the problems instead");
        return SPLPAK_E_UNSUPPORTED;
    }
    double xmin[MAXD] = {0, 0, 0, 0}, xmax[MAXD] = {0, 0, 0, 0};
    for (int d = 0; d < ndim; ++d) { xmin[d] = (double)xmin_t[d]; xmax[d] = (double)xmax_t[d]; }
    FitManyClipArgs ca{};
    FitManyArgs &a = ca.f;
    if (int rc = build_grid(ndim, nodes, xmin, xmax, a.g, nullptr, true)) {      // 102, 103
        if (rc == SPLPAK_E_UNSUPPORTED) set_error("more than 2^30 nodes is not supported");
        return rc;
    }
    const long long covlen = fit_many_cov_len(ndim, a.g.ncol);
    if (ldcoef < a.g.ncol || (covs && covs->ldcov < covlen)) return 104;
    bool ok = nbatch >= 1 && l1xdat >= ndim && xdata && ydata && coef && (!covs || covs->cov);
    for (int k = 0; ok && k < nbatch; ++k) ok = offsets[k + 1] >= offsets[k] && offsets[k + 1] - offsets[k] < (1LL << 31);
    if (!ok) {
        set_error("nbatch < 1, offsets that decrease, a problem of 2^31 points or more, l1xdat < ndim or a null pointer");      // (cov included)
        return SPLPAK_E_BADARG;
    }
    if (clip && (!clip->wout || clip->wout == wdata || clip->maxpass < 0 || !(clip->klo >= 1.0) || !(clip->khi >= 1.0))) {
        set_error("wout null or the same array as wdata, maxpass < 0, or klo or khi below 1 (or NaN)");
        return SPLPAK_E_BADARG;
    }
    a.sh = fit_many_shape(ndim, nodes);
    if (a.sh.bytes > FITMANY_LDS_BUDGET) {
        set_error("the grid needs more than 64 KiB of LDS per problem (splpak_fit_many_lds_bytes): loop splpak_fit_* over the problems instead");
        return SPLPAK_E_UNSUPPORTED;
    }

    try {
        const int ncol = a.g.ncol;
        const size_t nclip = clip ? (size_t)clip->nclip : 0;
        const size_t nres = FM_RESULT + nclip;
        std::vector<int> plist;
        for (int k = 0; k < nbatch; ++k) {
            const bool empty = offsets[k + 1] == offsets[k];
            if (!empty) plist.push_back(k);
            if (status) status[k] = empty ? 105 : 0;
            if (info) for (int j = 0; j < 10; ++j) info[(size_t)k * 10 + j] = 0.0;
            if (clip && clip->clip) for (size_t j = 0; j < nclip; ++j) clip->clip[(size_t)k * nclip + j] = 0.0;
        }
        const int nrun = (int)plist.size();
        t_fit_many_stats[1] = a.sh.bytes;
        t_fit_many_stats[3] = nrun;
        t_fit_many_stats[4] = nbatch - nrun;
        if (nrun == 0) return 105;

        if (int r = device_ready()) return r;
        const char *what = clip ? "a batch of clipped fits" : (covs ? "a batch of fits with their covariance" : "a batch of fits");
        const ManySpan sp = many_span(offsets, nbatch);
        std::vector<double> res((size_t)nrun * nres);
        std::vector<T> ch(dev ? 0 : (size_t)nrun * (size_t)ncol);
        std::vector<T> wh(dev || !clip ? 0 : (size_t)sp.n);
        std::vector<T> covh(dev || !covs ? 0 : (size_t)nrun * (size_t)covlen);
        const bool mad = clip && clip->mad;
        const long long allocs_before = t_many_offsets.allocs + t_fit_many_tables.allocs + t_fit_many_mad_t.allocs;
        const ScratchUse<1> use_offsets{t_many_offsets, st};
        const ScratchUse<2> use_tables{t_fit_many_tables, st};
        struct MadUse {      // ScratchUse of the robust rule's residuals, for the calls that use them
            bool on;
            hipStream_t st;
            ~MadUse() { if (on && t_fit_many_mad_t.last) (void)t_fit_many_mad_t.mark_used(st); }
        } const use_t{mad, st};
        CallStage cs;      // (the host entries alone)
        const size_t need[2] = {sizeof(int) * (size_t)nrun, sizeof(double) * res.size()};
        hipError_t e = many_offsets_upload(offsets, nbatch, st, &a.offsets);
        if (e == hipSuccess) e = scratch_begin(t_fit_many_tables, need, st);
        const size_t need_t[1] = {sizeof(double) * (size_t)sp.n};
        if (e == hipSuccess && mad) e = scratch_begin(t_fit_many_mad_t, need_t, st);
        // (pageable memory: the copy has left `plist` when the call returns)
        if (e == hipSuccess) e = hipMemcpyAsync(t_fit_many_tables.buf[0], plist.data(), need[0], hipMemcpyHostToDevice, st);
        a.nrun = nrun;
        a.plist = t_fit_many_tables.as<int>(0);
        a.result = t_fit_many_tables.as<double>(1);
        a.l1xdat = l1xdat;
        a.xtrap = xtrap;
        a.base = 0;
        a.ldcoef = ldcoef;
        a.compact = 0;
        const T *xd = xdata, *yd = ydata, *wd = wdata;
        T *cd = coef, *wo = clip ? clip->wout : nullptr, *cvd = covs ? covs->cov : nullptr;
        long long ldcov = covs ? covs->ldcov : 0;
        if (!dev) {
            // the span of the batch's points alone, the coefficients of the problems that run back to back
            if (e == hipSuccess) e = stage_span(cs, sp, xdata, l1xdat, ydata, wdata, &xd, &yd, &wd);
            if (e == hipSuccess && !cs.get(&cd, ch.size())) e = hipErrorOutOfMemory;
            if (e == hipSuccess && clip && !cs.get(&wo, wh.size())) e = hipErrorOutOfMemory;
            if (e == hipSuccess && covs && !cs.get(&cvd, covh.size())) e = hipErrorOutOfMemory;
            ldcov = covlen;
            a.base = sp.lo;
            a.ldcoef = ncol;
            a.compact = 1;
        }
        t_fit_many_stats[6] = t_many_offsets.allocs + t_fit_many_tables.allocs + t_fit_many_mad_t.allocs - allocs_before + (long long)cs.held.size();
        if (e != hipSuccess) return many_status(e, what, 0);
        double seconds = 0.0;
        if (mad) {
            FitManyMadArgs ma{};
            ma.f = a;
            if (int r = build_grid(ndim, nodes, xmin, xmax, ma.gref, nullptr)) return r;
            ma.klo = clip->klo;
            ma.khi = clip->khi;
            ma.maxpass = clip->maxpass;
            ma.regrow = clip->regrow != 0;
            ma.t = t_fit_many_mad_t.as<double>(0);
            ma.tbase = sp.lo - a.base;
            if (int r = fit_many_mad_launch<T>(ma, xd, yd, wd, wo, cd, st, &seconds)) return r;
        } else if (clip) {
            // the residuals are evaluated on the grid in the caller's order (it was valid above)
            if (int r = build_grid(ndim, nodes, xmin, xmax, ca.gref, nullptr)) return r;
            ca.klo2 = clip->klo * clip->klo;
            ca.khi2 = clip->khi * clip->khi;
            ca.maxpass = clip->maxpass;
            if (int r = fit_many_clip_launch<T>(ca, xd, yd, wd, wo, cd, st, &seconds)) return r;
        } else if (covs) {
            if (int r = fit_many_cov_launch<T>(a, xd, yd, wd, cd, cvd, ldcov, st, &seconds)) return r;
        } else {
            if (int r = fit_many_launch<T>(a, xd, yd, wd, cd, st, &seconds)) return r;
        }

        e = hipMemcpyAsync(res.data(), a.result, sizeof(double) * res.size(), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && !dev) e = hipMemcpyAsync(ch.data(), cd, sizeof(T) * ch.size(), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && !covh.empty()) e = hipMemcpyAsync(covh.data(), cvd, sizeof(T) * covh.size(), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && !wh.empty()) e = hipMemcpyAsync(wh.data(), wo, sizeof(T) * wh.size(), hipMemcpyDeviceToHost, st);
        const hipError_t waited = hipStreamSynchronize(st);      // (also after a failed copy: the one before it may still write `res`)
        if (e == hipSuccess) e = waited;
        if (e != hipSuccess) return many_status(e, what, 0);
        long long maxsteps = 0, maxfits = 0;
        int first_failed = -1;
        for (int r = 0; r < nrun; ++r) {
            const int k = plist[(size_t)r];
            const double *v = res.data() + (size_t)r * nres;
            const int sk = v[FM_STATUS] != 0.0 ? 107 : 0;
            if (status) status[k] = sk;
            if (sk != 0 && first_failed < 0) first_failed = k;
            if ((long long)v[FM_STEPS] > maxsteps) maxsteps = (long long)v[FM_STEPS];
            if ((long long)v[FM_SPARE] > maxfits) maxfits = (long long)v[FM_SPARE];
            if (info) {
                double *ik = info + (size_t)k * 10;
                ik[0] = v[FM_ROWS];
                ik[1] = v[FM_CROWS];
                ik[2] = v[FM_STEPS];
                ik[3] = v[FM_LASTREL];
                ik[4] = v[FM_MINPIV];
                ik[7] = seconds / (double)nrun;
                ik[8] = v[FM_RESERR];
            }
            if (clip && clip->clip)
                for (size_t j = 0; j < nclip; ++j) clip->clip[(size_t)k * nclip + j] = v[FM_RESULT + j];
            if (!dev) {
                T *ck = coef + (long long)k * ldcoef;
                for (int i = 0; i < ncol; ++i) ck[i] = ch[(size_t)r * (size_t)ncol + (size_t)i];
                if (covs) {
                    T *vk = covs->cov + (long long)k * covs->ldcov;
                    for (long long i = 0; i < covlen; ++i) vk[i] = covh[(size_t)r * (size_t)covlen + (size_t)i];
                }
            }
        }
        // (every point of the span belongs to a problem that ran)
        for (size_t i = 0; i < wh.size(); ++i) clip->wout[(size_t)sp.lo + i] = wh[i];
        t_fit_many_stats[5] = maxsteps;
        t_fit_many_stats[7] = maxfits;
        int rc = 0;
        for (int k = 0; k < nbatch && rc == 0; ++k) {
            if (offsets[k + 1] == offsets[k]) rc = 105;
            else if (k == first_failed) rc = 107;
        }
        if (first_failed >= 0) {
            char buf[200];
            snprintf(buf, sizeof buf, "problem %d of the batch: a pivot failed the rank test or the refinement missed 1e-10 (too few points?)", first_failed);
            set_error(buf);
        }
        return rc;
    } catch (const std::bad_alloc &) {
        set_error("the host tables of the batch of fits could not be allocated");
        return SPLPAK_E_NOMEM;
    }
}

}  // namespace splpak
