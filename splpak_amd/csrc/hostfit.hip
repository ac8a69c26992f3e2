// The one-shot host entry points of the C ABI (include/splpak_hip.h): splpak_fit_f64 / _f32 on host arrays, the refit of their
// last fit by token, the plan they keep between calls, and splpak_shutdown.
#include "plan.hpp"

#include <cstring>

using namespace splpak;

// The one-shot entry keeps its plan (band factor storage, sort scratch, staging buffers: 28 GB at
// 64^3) between calls: a caller that fits the same grid again -- the reference's usage pattern is one
// `initialize` per data set -- pays the allocation once.  Released by splpak_shutdown(); disabled by
// SPLPAK_NO_PLAN_CACHE.  Calls from several threads are serialised.
extern "C" {
namespace {
struct HostFitCache {
    std::mutex mu;
    splpak_plan *plan = nullptr;
    int ndim = 0, nodes[MAXD] = {0, 0, 0, 0}, dev = -1;
    double xmin[MAXD] = {0, 0, 0, 0}, xmax[MAXD] = {0, 0, 0, 0}, xtrap = 0.0;
    double *dx = nullptr, *dy = nullptr, *dw = nullptr, *dc = nullptr;
    long long cap_x = 0, cap_y = 0, cap_w = 0, cap_c = 0;
    int64_t token = 0;            // of the successful fit the plan holds (splpak_fit_token / splpak_refit_*); 0: none
    long long ndata = 0;          // its points
    void release()
    {
        token = 0;
        for (double **q : {&dx, &dy, &dw, &dc}) { if (*q) (void)hipFree(*q); *q = nullptr; }
        cap_x = cap_y = cap_w = cap_c = 0;
        if (plan) splpak_plan_destroy(plan);
        plan = nullptr;
    }
};
HostFitCache g_hostfit;
std::atomic<int64_t> g_fit_tokens{0};              // every successful one-shot fit of the process draws a fresh token
thread_local int64_t t_fit_token = 0;              // of the calling thread's last successful one-shot fit
}  // namespace
}  // extern "C"

// An allocation failed: give back what the one-shot entry keeps between calls (round-2 advice).  Not while a one-shot
// fit is running (it holds the lock and has released its old plan itself).  true = something was released.
static thread_local bool t_in_fit_host = false;      // this thread holds g_hostfit.mu (try_lock on a mutex one owns is undefined)
struct InFit { InFit() { t_in_fit_host = true; } ~InFit() { t_in_fit_host = false; } };

bool splpak::release_cached_plan_for_memory()
{
    if (t_in_fit_host) return false;
    std::unique_lock<std::mutex> lock(g_hostfit.mu, std::try_to_lock);
    if (!lock.owns_lock() || !g_hostfit.plan) return false;
    g_hostfit.release();
    return true;
}

void splpak::hostfit_forget_token()
{
    t_fit_token = 0;
    if (t_in_fit_host) return;
    std::lock_guard<std::mutex> lock(g_hostfit.mu);
    g_hostfit.token = 0;
}

extern "C" {

int32_t splpak_fit_f64(int32_t ndim, const double *xdata, int32_t l1xdat, const double *ydata,
                       const double *wdata, int64_t ndata, const double *xmin, const double *xmax,
                       const int32_t *nodes, double xtrap, double *coef, int64_t ncf, int64_t nwrk,
                       double *hist_out, double *info)
{
    if (!nodes || !xmin || !xmax) { set_error("null argument"); return SPLPAK_E_BADARG; }
    Grid g;
    long long ncol = 0;
    const int v = build_grid(ndim, nodes, xmin, xmax, g, &ncol);       // 101, 102, 103
    if (v != 0) return v;
    if (ncol > ncf) return 104;                                        // :751-756
    if (ndata < 1) return 105;                                         // :759-764
    if (nwrk >= 0) {                                                   // :772-781
        const long long nwrk1 = (xtrap != 0.0) ? ncol + 1 : 1;
        if (nwrk - nwrk1 + 1 < 1) return 106;
    }
    if (!xdata || !ydata || !coef) { set_error("null argument"); return SPLPAK_E_BADARG; }
    if (l1xdat < ndim) { set_error("l1xdat < ndim"); return SPLPAK_E_BADARG; }
    if (wdata && wdata[0] < 0.0) wdata = nullptr;                      // :581-588, :796
    if (int r = device_ready()) return r;

    HostFitCache &hc = g_hostfit;
    std::lock_guard<std::mutex> lock(hc.mu);
    InFit in_fit;
    int dev = 0;
    (void)hipGetDevice(&dev);
    // the switches are part of the cache key as a whole (a plan keeps the snapshot it was created with)
    const Options cur = options_snapshot();
    hc.token = 0;                      // (whatever fit the plan held is being replaced)
    bool same = hc.plan && hc.dev == dev && hc.ndim == ndim && hc.xtrap == xtrap && hc.plan->max_ndata >= ndata && hc.plan->opt == cur;
    for (int d = 0; same && d < ndim; ++d)
        same = hc.nodes[d] == nodes[d] && hc.xmin[d] == xmin[d] && hc.xmax[d] == xmax[d];
    if (!same) {
        hc.release();
        int rc = splpak_plan_create(ndim, nodes, xmin, xmax, xtrap, ndata, nullptr, 0, &hc.plan);
        if (rc != 0) { hc.plan = nullptr; return rc; }
        hc.dev = dev;
        hc.ndim = ndim;
        hc.xtrap = xtrap;
        for (int d = 0; d < ndim; ++d) { hc.nodes[d] = nodes[d]; hc.xmin[d] = xmin[d]; hc.xmax[d] = xmax[d]; }
    }
    splpak_plan *p = hc.plan;
    auto grow = [&](double **q, long long &cap, long long need) {
        if (*q && cap >= need) return true;
        if (*q) (void)hipFree(*q);
        *q = nullptr;
        cap = 0;
        if (!hip_ok(hipMalloc((void **)q, sizeof(double) * (size_t)need), "hipMalloc of the staging buffers")) return false;
        cap = need;
        return true;
    };
    const bool ok = grow(&hc.dx, hc.cap_x, (long long)ndata * l1xdat) && grow(&hc.dy, hc.cap_y, ndata) &&
                    (!wdata || grow(&hc.dw, hc.cap_w, ndata)) && grow(&hc.dc, hc.cap_c, ncol);
    if (!ok) { hc.release(); return SPLPAK_E_NOMEM; }
    hipError_t e = hipMemcpy(hc.dx, xdata, sizeof(double) * (size_t)ndata * l1xdat, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(hc.dy, ydata, sizeof(double) * (size_t)ndata, hipMemcpyHostToDevice);
    if (e == hipSuccess && wdata) e = hipMemcpy(hc.dw, wdata, sizeof(double) * (size_t)ndata, hipMemcpyHostToDevice);
    if (!hip_ok(e, "hipMemcpy H2D")) { hc.release(); return SPLPAK_E_NODEVICE; }
    int rc = splpak_plan_fit_dev(p, hc.dx, l1xdat, hc.dy, wdata ? hc.dw : nullptr, ndata, hc.dc, nullptr, info);
    if (rc == 0 || rc == 107) {
        e = hipMemcpy(coef, hc.dc, sizeof(double) * (size_t)ncol, hipMemcpyDeviceToHost);
        if (e == hipSuccess && hist_out && xtrap != 0.0)
            e = hipMemcpy(hist_out, p->hist, sizeof(double) * (size_t)ncol, hipMemcpyDeviceToHost);
        if (!hip_ok(e, "hipMemcpy D2H")) rc = SPLPAK_E_NODEVICE;
    }
    if (rc < 0 || splpak::opt_get("SPLPAK_NO_PLAN_CACHE")) hc.release();
    if (rc == 0) {                     // (the token is drawn even when nothing stays resident: a refit then says so)
        t_fit_token = ++g_fit_tokens;
        if (hc.plan) { hc.token = t_fit_token; hc.ndata = ndata; }
    }
    return rc;
}

// New values on the points of the one-shot fit `token`: every field through the cache's staging buffers and the cached plan's
// refit.  real32: the caller's arrays are floats, widened and narrowed on the host as splpak_fit_f32 does.
static int32_t refit_host(int64_t token, int32_t nfields, const void *ydata, int64_t ldy, int64_t ndata, void *coef, int64_t ldcoef,
                          double *info, bool real32)
{
    if (!ydata || !coef) { set_error("null argument"); return SPLPAK_E_BADARG; }
    if (nfields < 1) { set_error("nfields < 1"); return SPLPAK_E_BADARG; }
    if (ndata < 1 || ldy < ndata) { set_error("ldy < ndata, or ndata < 1"); return SPLPAK_E_BADARG; }
    if (int r = device_ready()) return r;
    HostFitCache &hc = g_hostfit;
    std::lock_guard<std::mutex> lock(hc.mu);
    InFit in_fit;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (token == 0 || !hc.plan || hc.token != token || hc.ndata != ndata || hc.dev != dev || !hc.dy || !hc.dc || hc.cap_y < ndata) {
        set_error("the fit is no longer resident: fit again (another fit, splpak_shutdown, a release under memory pressure, "
                  "SPLPAK_NO_PLAN_CACHE or a multi-GPU fit since, or another ndata)");
        return SPLPAK_E_UNSUPPORTED;
    }
    splpak_plan *p = hc.plan;
    const long long ncol = p->g.ncol;
    if (ldcoef < ncol) { set_error("ldcoef < number of coefficients"); return SPLPAK_E_BADARG; }
    std::vector<double> wide;
    if (real32) wide.resize((size_t)(ndata > ncol ? ndata : ncol));
    // Several fields are staged in groups of up to 8, so that the plan's refit can solve them in shared sweeps (splpak_plan_refit_dev);
    // one field, or no memory for the group's staging, goes through the cache's own buffers one field at a time
    struct Staging {
        void *y = nullptr, *c = nullptr;
        ~Staging() { if (y) (void)hipFree(y); if (c) (void)hipFree(c); }
    } own;
    int group = 1;
    double *dy = hc.dy, *dc = hc.dc;
    if (nfields >= 2) {
        const int want = nfields < 8 ? nfields : 8;
        if (hipMalloc(&own.y, sizeof(double) * (size_t)want * (size_t)ndata) == hipSuccess &&
            hipMalloc(&own.c, sizeof(double) * (size_t)want * (size_t)ncol) == hipSuccess) {
            group = want;
            dy = static_cast<double *>(own.y);
            dc = static_cast<double *>(own.c);
        } else
            (void)hipGetLastError();
    }
    if (info) for (size_t i = 0; i < 10 * (size_t)nfields; ++i) info[i] = 0.0;      // (a field behind a 107 keeps these zeros)
    for (int k0 = 0; k0 < nfields; k0 += group) {
        const int n = nfields - k0 < group ? nfields - k0 : group;
        for (int i = 0; i < n; ++i) {
            const double *src = nullptr;
            if (real32) {
                const float *yf = static_cast<const float *>(ydata) + (size_t)(k0 + i) * (size_t)ldy;
                for (long long q = 0; q < ndata; ++q) wide[(size_t)q] = yf[q];
                src = wide.data();
            } else
                src = static_cast<const double *>(ydata) + (size_t)(k0 + i) * (size_t)ldy;
            if (!hip_ok(hipMemcpy(dy + (size_t)i * (size_t)ndata, src, sizeof(double) * (size_t)ndata, hipMemcpyHostToDevice), "hipMemcpy H2D")) { hc.release(); return SPLPAK_E_NODEVICE; }
        }
        int rc = splpak_plan_refit_dev(p, n, dy, ndata, dc, ncol, nullptr, info ? info + 10 * (size_t)k0 : nullptr);
        // (a refusal -- the plan's state or an argument -- leaves the resident fit as it was; a device failure does not)
        if (rc == SPLPAK_E_UNSUPPORTED || rc == SPLPAK_E_BADARG) return rc;
        if (rc < 0) { hc.release(); return rc; }
        for (int i = 0; i < n; ++i) {
            double *dst = real32 ? wide.data() : static_cast<double *>(coef) + (size_t)(k0 + i) * (size_t)ldcoef;
            if (!hip_ok(hipMemcpy(dst, dc + (size_t)i * (size_t)ncol, sizeof(double) * (size_t)ncol, hipMemcpyDeviceToHost), "hipMemcpy D2H")) { hc.release(); return SPLPAK_E_NODEVICE; }
            if (real32) {
                float *cf = static_cast<float *>(coef) + (size_t)(k0 + i) * (size_t)ldcoef;
                for (long long q = 0; q < ncol; ++q) cf[q] = (float)wide[(size_t)q];
            }
        }
        if (rc != 0) {                 // 107: the later fields are zeroed, as splpak_plan_refit_dev leaves them (those of this group it zeroed itself)
            for (int j = k0 + n; j < nfields; ++j) {
                if (real32) std::memset(static_cast<float *>(coef) + (size_t)j * (size_t)ldcoef, 0, sizeof(float) * (size_t)ncol);
                else std::memset(static_cast<double *>(coef) + (size_t)j * (size_t)ldcoef, 0, sizeof(double) * (size_t)ncol);
            }
            return rc;
        }
    }
    return 0;
}

int64_t splpak_fit_token(void) { return t_fit_token; }

int32_t splpak_refit_f64(int64_t token, int32_t nfields, const double *ydata, int64_t ldy, int64_t ndata, double *coef, int64_t ldcoef,
                         double *info)
{
    return refit_host(token, nfields, ydata, ldy, ndata, coef, ldcoef, info, false);
}

int32_t splpak_refit_f32(int64_t token, int32_t nfields, const float *ydata, int64_t ldy, int64_t ndata, float *coef, int64_t ldcoef,
                         double *info)
{
    return refit_host(token, nfields, ydata, ldy, ndata, coef, ldcoef, info, true);
}

int32_t splpak_fit_f32(int32_t ndim, const float *xdata, int32_t l1xdat, const float *ydata,
                       const float *wdata, int64_t ndata, const float *xmin, const float *xmax,
                       const int32_t *nodes, float xtrap, float *coef, int64_t ncf, int64_t nwrk,
                       float *hist_out, double *info)
{
    // REAL32 storage, f64 arithmetic: widen on the host (the arrays are small
    // next to the factorisation), run the f64 path, narrow the results.
    if (ndim < 1) return 101;
    if (ndim > MAXD) return SPLPAK_E_UNSUPPORTED;
    if (!nodes || !xmin || !xmax) { set_error("null argument"); return SPLPAK_E_BADARG; }
    double xmn[MAXD], xmx[MAXD];
    long long ncol = 1;
    for (int d = 0; d < ndim; ++d) { xmn[d] = xmin[d]; xmx[d] = xmax[d]; ncol *= nodes[d] > 0 ? nodes[d] : 1; }
    const bool have = xdata && ydata && coef && ndata >= 1 && ncol <= ncf;
    std::vector<double> X, Y, W, Cf, H;
    if (have) {
        X.assign(xdata, xdata + (size_t)ndata * l1xdat);
        Y.assign(ydata, ydata + (size_t)ndata);
        if (wdata && !(wdata[0] < 0.0f)) W.assign(wdata, wdata + (size_t)ndata);      // (as splpak_fit_f64: a NaN is not negative)
        Cf.resize((size_t)ncol);
        if (hist_out) H.resize((size_t)ncol);
    }
    const int rc = splpak_fit_f64(ndim, have ? X.data() : nullptr, l1xdat, have ? Y.data() : nullptr,
                                  W.empty() ? nullptr : W.data(), ndata, xmn, xmx, nodes, (double)xtrap,
                                  have ? Cf.data() : nullptr, ncf, nwrk, H.empty() ? nullptr : H.data(), info);
    if (have && (rc == 0 || rc == 107)) {
        for (long long i = 0; i < ncol; ++i) coef[i] = (float)Cf[(size_t)i];
        if (hist_out && xtrap != 0.0f)
            for (long long i = 0; i < ncol; ++i) hist_out[i] = (float)H[(size_t)i];
    }
    return rc;
}

void splpak_shutdown(void)
{
    {
        std::lock_guard<std::mutex> lock(g_hostfit.mu);
        g_hostfit.release();
    }
    eval_scratch_shutdown();
    eval_grid_scratch_shutdown();
    fit_grid_scratch_shutdown();
}

}  // extern "C"
