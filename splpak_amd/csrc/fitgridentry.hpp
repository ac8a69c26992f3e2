// What the entries of the two grid fits share (fitgridapi.hip, fitgridwapi.hip): the ladder of argument checks.
#pragma once
#include "plan.hpp"
#include "fitgrid.hpp"

namespace splpak {

// The checks before the axes are looked at, in the order the header gives.  True: go on; false: rc is the status to return.
template <typename T>
inline bool fit_grid_validate(int32_t ndim, const int64_t *npts, const void *axes, int32_t nfields, const void *values, int64_t ldv,
                              const T *xmin_t, const T *xmax_t, const int32_t *nodes, const void *coef, int64_t ldcoef, Grid &g,
                              long long &nsamp, long long &ntab, int &rc)
{
    nsamp = 1;
    ntab = 0;
    if (!npts || !nodes || !xmin_t || !xmax_t) { set_error("null argument"); rc = SPLPAK_E_BADARG; return false; }
    double xmin[MAXD] = {0, 0, 0, 0}, xmax[MAXD] = {0, 0, 0, 0};
    for (int d = 0; d < ndim && d < MAXD; ++d) { xmin[d] = (double)xmin_t[d]; xmax[d] = (double)xmax_t[d]; }
    rc = build_grid(ndim, nodes, xmin, xmax, g, nullptr);      // 101, SPLPAK_E_UNSUPPORTED (ndim > 4), 102, 103
    if (rc != 0) {
        if (rc == SPLPAK_E_UNSUPPORTED) set_error("ndim > 4 or more than 2^30 nodes is not supported");
        return false;
    }
    if (ldcoef < g.ncol) { rc = 104; return false; }
    for (int d = 0; d < ndim; ++d)
        if (npts[d] < 1) { rc = 105; return false; }
    bool ok = nfields >= 1 && axes && values && coef;
    for (int d = 0; ok && d < ndim; ++d)
        ok = !__builtin_mul_overflow(nsamp, (long long)npts[d], &nsamp) && !__builtin_add_overflow(ntab, (long long)npts[d], &ntab);
    if (!ok || ldv < nsamp) {
        set_error("a null pointer, nfields < 1, a product of npts beyond int64 or ldv smaller than it");
        rc = SPLPAK_E_BADARG;
        return false;
    }
    return true;
}

}  // namespace splpak
