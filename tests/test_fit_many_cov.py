"""The covariance of the coefficients of a batch of small fits (splpak_fit_many_cov_*, csrc/fitmanycov.hip and phase 6 of
csrc/fitmanydev.hpp): Z = (A^T W^2 A + C^T C)^-1 inside the band, as the half stencil of every node.

Yardstick.  The reference has no covariance.  The normal equations of the reference's rows come from Port.normal_equations
(oracle/binding.py: accumulated in long double), are made dense and inverted by a Cholesky written in np.longdouble (restricted
to the band, outside which every entry of the factor is zero; the inverse is formed by two substitutions on the identity, not by
the recurrence under test).  Bar, from the perturbation theory of Cholesky: with kappa_s = cond(D^-1 N D^-1), D = sqrt(diag N),
every stencil entry has |Z_ij - Zref_ij| <= 16 eps kappa_s sqrt(Zref_ii Zref_jj).  A case enters the parity only with
kappa_s <= 1e9, which a CPU test asserts for every listed case; the family left out by name is n130_x* (the wide hole, 4e11),
which is run for status 0 and a positive diagonal.

CPU tier: exports, splpak_fit_many_cov_len, the ladder rung by rung before any device call, the condition of every listed case,
and a numpy restatement of the in-place band recurrence on NumpyManyFit's factor against the yardstick.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from splpak_amd import capi
from tests.conftest import ROOT
from tests.test_fit_many import (E_BADARG, E_UNSUPPORTED, LDS_BUDGET, SINGULAR, NumpyManyFit, _values, lo_hi, pack,
                                 problem)

SYMBOLS = ("splpak_fit_many_cov_f64", "splpak_fit_many_cov_f32", "splpak_fit_many_cov_dev_f64", "splpak_fit_many_cov_dev_f32",
           "splpak_fit_many_cov_len")
EPS = float(np.finfo(np.float64).eps)
KAPPA_MAX = 1e9
SENT = 777.0
DP, IP, LP = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


# ---------------------------------------------------------------------------------------------------------------
# The problems: those of tests/test_fit_many.py, a 65-node grid (the first that runs in 256-thread workgroups) with 3 evenly
# placed points per cell like nmax, and the largest 2-D grid with 2 000 uniform points.
@functools.lru_cache(maxsize=None)
def cov_problem(name):
    if name == "n65":
        rng = np.random.default_rng(7501)
        x = ((np.repeat(np.arange(64), 3) + np.tile((np.arange(3) + 0.37) / 3, 64)) / 64).reshape(-1, 1)
        return dict(ndim=1, nodes=(65,), xtrap=1.0, x=x, y=_values(x, rng), w=None)
    if name == "g1212":
        rng = np.random.default_rng(7502)
        x = rng.uniform(0.0, 1.0, (2000, 2))
        return dict(ndim=2, nodes=(12, 12), xtrap=1.0, x=x, y=_values(x, rng), w=None)
    return problem(name)


# one batch per grid (and xtrap), the problems in a mixed order
BATCHES = {
    "n4": ["n4_x1"],
    "n4_xt0": ["n4_x1_xt0"],
    "n9": ["n9_wide_x17", "w_n9_wide", "n9_wide_x1", "n9_wide_x3"],
    "n65": ["n65"],
    "nmax": ["nmax_x1"],
    "g44": ["g44"],
    "g59": ["w_g59", "g59"],
    "g95": ["g95"],
    "gbox": ["gbox"],
    "g1211": ["g1211"],
    "g1212": ["g1212"],
}
PARITY_NAMES = [n for b in BATCHES.values() for n in b]
LEFT_OUT = ["n130_x1", "n130_x3"]


def hst_of(ndim):
    return (7 ** ndim + 1) // 2


def stencil_columns(ndim, nodes):
    """(col, inside): col[i, code] = the column i + o of slot `code` of node i in the caller's numbering (dimension 0 fastest),
    inside[i, code] whether it lies in the grid.  The layout of Port.normal_equations and of `cov`."""
    nodes = list(nodes)
    ncol, hst = int(np.prod(nodes)), hst_of(ndim)
    idx = np.arange(ncol)
    col = np.zeros((ncol, hst), dtype=np.int64)
    inside = np.ones((ncol, hst), dtype=bool)
    for code in range(hst):
        c, stride, rem = idx.copy(), 1, idx.copy()
        for d in range(ndim):
            o = (code // 7 ** d) % 7 - 3
            ind = rem % nodes[d]
            rem = rem // nodes[d]
            inside[:, code] &= (ind + o >= 0) & (ind + o < nodes[d])
            c = c + o * stride
            stride *= nodes[d]
        col[:, code] = c
    col[~inside] = 0
    return col, inside


def dense_from_stencil(ndim, nodes, S, dtype=np.longdouble):
    col, inside = stencil_columns(ndim, nodes)
    n = col.shape[0]
    M = np.zeros((n, n), dtype=dtype)
    rows = np.repeat(np.arange(n), col.shape[1]).reshape(col.shape)
    M[rows[inside], col[inside]] = S[inside]
    M[col[inside], rows[inside]] = S[inside]
    return M


def stencil_from_dense(ndim, nodes, M):
    col, inside = stencil_columns(ndim, nodes)
    rows = np.repeat(np.arange(col.shape[0]), col.shape[1]).reshape(col.shape)
    S = np.zeros(col.shape, dtype=M.dtype)
    S[inside] = M[rows[inside], col[inside]]
    return S


def longdouble_inverse(N, hb):
    """N^-1 of a symmetric positive definite matrix of half bandwidth hb, in np.longdouble: the Cholesky factor column by column
    (entries outside the band are exactly zero, so only the band is touched), then L Y = I and L^T Z = Y row by row."""
    A = np.array(N, dtype=np.longdouble)
    n = A.shape[0]
    for j in range(n):
        A[j, j] = np.sqrt(A[j, j])
        m = min(hb, n - 1 - j)
        if m:
            A[j + 1:j + 1 + m, j] /= A[j, j]
            c = A[j + 1:j + 1 + m, j]
            A[j + 1:j + 1 + m, j + 1:j + 1 + m] -= np.outer(c, c)
    L = np.tril(A)
    Y = np.eye(n, dtype=np.longdouble)
    for i in range(n):
        k0 = max(0, i - hb)
        if i > k0:
            Y[i] -= L[i, k0:i] @ Y[k0:i]
        Y[i] /= L[i, i]
    Z = Y
    for i in range(n - 1, -1, -1):
        k1 = min(n, i + hb + 1)
        if k1 > i + 1:
            Z[i] -= L[i + 1:k1, i] @ Z[i + 1:k1]
        Z[i] /= L[i, i]
    return Z


@functools.lru_cache(maxsize=None)
def _port():
    from oracle.binding import Port
    return Port()


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """dict(Z dense long double, S its half stencil in float64, zd = sqrt(diag Z) in float64, kappa) of a problem."""
    p = cov_problem(name)
    lo, hi = lo_hi(p)
    nd, nodes = p["ndim"], list(p["nodes"])
    w = p["w"]
    ne = _port().normal_equations(nd, p["x"], p["y"], w, lo, hi, nodes, p["xtrap"])
    N = dense_from_stencil(nd, nodes, ne["N"])
    hb = 3 if nd == 1 else 3 * nodes[0] + 3
    d = np.sqrt(np.diag(N).astype(np.float64))
    kappa = float(np.linalg.cond(N.astype(np.float64) / np.outer(d, d)))
    Z = longdouble_inverse(N, hb)
    return dict(Z=Z, S=stencil_from_dense(nd, nodes, Z).astype(np.float64), zd=np.sqrt(np.diag(Z).astype(np.float64)), kappa=kappa)


def worst_ratio(name, S):
    """max over the stencil entries of |Z_ij - Zref_ij| / (eps kappa_s sqrt(Zref_ii Zref_jj)); entries outside the grid must be 0."""
    p = cov_problem(name)
    y = yardstick(name)
    col, inside = stencil_columns(p["ndim"], p["nodes"])
    S = np.asarray(S, dtype=np.float64).reshape(col.shape)
    assert np.all(S[~inside] == 0.0), name
    scale = y["zd"][:, None] * y["zd"][col]
    return float(np.max(np.abs(S - y["S"])[inside] / (EPS * y["kappa"] * scale[inside])))


def check_cov(name, S, what):
    ratio = worst_ratio(name, S)
    print(f"{name} ({what}): kappa_s {yardstick(name)['kappa']:.2e}, worst |Z - Zref| / (eps kappa_s sqrt(Zii Zjj)) = {ratio:.3f} (bar 16)")
    assert ratio <= 16.0, (name, ratio)


# ---------------------------------------------------------------------------------------------------------------
# The recurrence in numpy
def band_selected_inverse(B, n, hb):
    """In place on the factor B[i, k] = L(i, i - k): B[j, j - i] = Z(j, i) for j = i .. min(i + hb, n - 1), column by column from
    the last one up (phase 6 of csrc/fitmanydev.hpp)."""
    for i in range(n - 1, -1, -1):
        m = min(hb, n - 1 - i)
        lc = np.array([B[i + t, t] for t in range(m + 1)])
        z = np.zeros(m + 1)
        for t in range(1, m + 1):
            j, s = i + t, 0.0
            for k in range(i + 1, i + m + 1):
                a, b = max(j, k), min(j, k)
                s += B[a, a - b] * lc[k - i]
            z[t] = -s / lc[0]
        z[0] = (1.0 / lc[0] - z[1:] @ lc[1:]) / lc[0]
        for t in range(m + 1):
            B[i + t, t] = z[t]
    return B


def stencil_from_band(fit, B):
    """The half stencil in the caller's node order from the band of Z in NumpyManyFit's internal order."""
    nd, nodes = fit.ndim, fit.ref_nodes
    col, inside = stencil_columns(nd, nodes)

    def internal(ref_index):
        ind, rem = [], ref_index
        for r in range(nd):
            ind.append(rem % nodes[r])
            rem = rem // nodes[r]
        return sum(ind[fit.perm[d]] * fit.stride[d] for d in range(nd))
    rows = np.repeat(np.arange(col.shape[0]), col.shape[1]).reshape(col.shape)
    ii, jj = internal(rows), internal(col)
    a, b = np.maximum(ii, jj), np.minimum(ii, jj)
    S = np.zeros(col.shape)
    S[inside] = B[a[inside], (a - b)[inside]]
    return S


# ---------------------------------------------------------------------------------------------------------------
# CPU tier
def test_symbols_exported_and_listed():
    lib = capi.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in capi.SYMBOLS, s


def test_cov_len_values_and_refusals():
    f = capi.fit_many_cov_len
    assert f(1, [4]) == 16 and f(1, [896]) == 3584 and f(2, [4, 4]) == 400 and f(2, [12, 12]) == 3600 and f(2, [5, 9]) == f(2, [9, 5]) == 1125
    assert f(2, [1000, 1000]) == 25000000      # no LDS rule and no device in it
    raw = capi.lib().splpak_fit_many_cov_len
    for bad in ((0, [4]), (3, [4, 4, 4]), (1, [3]), (2, [4, 3])):
        assert raw(bad[0], np.array(bad[1], dtype=np.int32).ctypes.data_as(IP)) == E_BADARG
        assert capi.lib().splpak_fit_many_lds_bytes(bad[0], np.array(bad[1], dtype=np.int32).ctypes.data_as(IP)) == E_BADARG
    assert raw(1, None) == E_BADARG


def _call(ndim=1, nbatch=1, offsets=(0, 8), x="ok", l1xdat=1, y="ok", xmin=(0.0, 0.0), xmax=(1.0, 1.0), nodes=(4, 4), ldcoef=16, coef="ok",
          ldcov=400, cov="ok"):
    """splpak_fit_many_cov_f64 on raw arguments -> (rc, coef, cov, status); "ok": a valid array, None: a null pointer."""
    keep = []

    def arr(v, dt, ty):
        if v is None:
            return None
        a = np.ascontiguousarray(v, dtype=dt)
        keep.append(a)
        return a.ctypes.data_as(ty)
    cf, cv = np.full(64, SENT), np.full(1024, SENT)
    st = np.full(8, -999, dtype=np.int32)
    xs = np.linspace(0.0, 1.0, 32)
    rc = capi.lib().splpak_fit_many_cov_f64(ndim, nbatch, arr(offsets, np.int64, LP), arr(xs if x == "ok" else x, np.float64, DP), l1xdat,
                                            arr(xs if y == "ok" else y, np.float64, DP), None, arr(xmin, np.float64, DP),
                                            arr(xmax, np.float64, DP), arr(nodes, np.int32, IP), 1.0,
                                            cf.ctypes.data_as(DP) if coef == "ok" else None, ldcoef,
                                            cv.ctypes.data_as(DP) if cov == "ok" else None, ldcov, st.ctypes.data_as(IP), None)
    return rc, cf, cv, st


def test_status_ladder_in_order_before_any_device_call():
    """The ladder of splpak_fit_many_* with ldcov < len on the 104 rung and cov == NULL in the last SPLPAK_E_BADARG group: every
    rung with later rungs failing too; coef, cov and status stay as they were.  No rung asks for a device."""
    big = (1000, 1000)      # 2-D, beyond the LDS rule; len = 25 000 000
    ok = dict(ndim=2, nodes=big, ldcoef=1000000, ldcov=25000000)
    ladder = [
        (E_BADARG, dict(offsets=None, ndim=0)),
        (E_BADARG, dict(nodes=None, ndim=0)),
        (E_BADARG, dict(xmin=None, ndim=0)),
        (E_BADARG, dict(xmax=None, ndim=0)),
        (101, dict(ndim=0, nodes=(3, 3), ldcoef=0, ldcov=0, nbatch=0)),
        (E_UNSUPPORTED, dict(ndim=3, nodes=(3, 3, 3), xmin=(0, 0, 0), xmax=(1, 1, 1), ldcoef=0, ldcov=0, nbatch=0)),
        (102, dict(ndim=2, nodes=(3, 4), xmax=(1.0, 0.0), ldcoef=0, ldcov=0, nbatch=0)),
        (103, dict(ndim=2, nodes=(4, 4), xmax=(1.0, 0.0), ldcoef=0, ldcov=0, nbatch=0)),
        (104, dict(ndim=2, nodes=big, ldcoef=999999, ldcov=25000000, nbatch=0)),
        (104, dict(ndim=2, nodes=big, ldcoef=1000000, ldcov=24999999, nbatch=0, cov=None)),
        (104, dict(ndim=1, ldcoef=4, ldcov=15, x=None)),
        (104, dict(ndim=2, ldcoef=16, ldcov=399, cov=None)),
        (E_BADARG, dict(nbatch=0, **ok)),
        (E_BADARG, dict(l1xdat=2, offsets=(0, 8, 4), nbatch=2, **ok)),
        (E_BADARG, dict(l1xdat=1, **ok)),
        (E_BADARG, dict(l1xdat=2, x=None, **ok)),
        (E_BADARG, dict(l1xdat=2, y=None, **ok)),
        (E_BADARG, dict(l1xdat=2, coef=None, **ok)),
        (E_BADARG, dict(l1xdat=2, cov=None, **ok)),
        (E_UNSUPPORTED, dict(l1xdat=2, **ok)),
    ]
    for want, kw in ladder:
        rc, cf, cv, st = _call(**kw)
        assert rc == want, (want, rc, kw)
        assert np.all(cf == SENT) and np.all(cv == SENT) and np.all(st == -999), kw
    assert "loop" in capi.last_error()
    # cov null on a grid inside the LDS rule, and a batch of empty problems alone: 105 each on the host, nothing written
    assert _call(cov=None, ldcov=16, ldcoef=4)[0] == E_BADARG
    rc, cf, cv, st = _call(nbatch=2, offsets=(5, 5, 5), ldcoef=4, ldcov=16)
    assert rc == 105 and list(st[:2]) == [105, 105] and np.all(cf == SENT) and np.all(cv == SENT)
    # the LDS rule is that of splpak_fit_many_*: 12 x 12 is admitted, 13 x 13 is not
    assert capi.fit_many_lds_bytes(2, [12, 12]) <= LDS_BUDGET
    assert _call(ndim=2, nodes=(12, 12), ldcoef=144, ldcov=3600, l1xdat=2, offsets=(0, 0))[0] == 105
    assert _call(ndim=2, nodes=(13, 13), ldcoef=169, ldcov=4225, l1xdat=2, offsets=(0, 0))[0] == E_UNSUPPORTED


@pytest.mark.parametrize("name", PARITY_NAMES)
def test_every_parity_case_is_well_enough_conditioned(name):
    """kappa_s <= 1e9 for every listed case, so that none drops out of the parity silently."""
    k = yardstick(name)["kappa"]
    print(f"{name}: kappa_s = {k:.3e}")
    assert k <= KAPPA_MAX


@pytest.mark.parametrize("name", PARITY_NAMES)
def test_numpy_band_recurrence_matches_the_long_double_inverse(name):
    """The algebra without a GPU: the in-place recurrence on NumpyManyFit's float64 factor, mapped to the caller's stencil."""
    fit = NumpyManyFit(cov_problem(name))
    B = fit.band()
    spd, _ = fit.cholesky(B)
    assert spd
    check_cov(name, stencil_from_band(fit, band_selected_inverse(B, fit.ncol, fit.hb)), "numpy recurrence")


def test_the_yardstick_inverts():
    """Zref N = I to long-double accuracy on the worst conditioned listed case."""
    name = "g1211"
    p = cov_problem(name)
    lo, hi = lo_hi(p)
    ne = _port().normal_equations(2, p["x"], p["y"], None, lo, hi, list(p["nodes"]), p["xtrap"])
    N = dense_from_stencil(2, p["nodes"], ne["N"])
    y = yardstick(name)
    r = np.max(np.abs((y["Z"] @ N - np.eye(N.shape[0])).astype(np.float64)))
    print(f"{name}: max |Zref N - I| = {r:.2e}, kappa_s {y['kappa']:.2e}")
    assert r <= 1e-9


# ---------------------------------------------------------------------------------------------------------------
# GPU tier
def _batch_args(names, empty_at=()):
    ps = [cov_problem(n) for n in names]
    off, x, y, w = pack(ps, empty_at)
    p0 = ps[0]
    lo, hi = lo_hi(p0)
    return (p0["ndim"], off, x, y, w, lo, hi, list(p0["nodes"]), p0["xtrap"])


@functools.lru_cache(maxsize=None)
def run_cov(key):
    """(coef, cov, rc, status, info, counters) of one of BATCHES through the host entry; computed once, nobody writes to it."""
    out = capi.fit_many_cov(*_batch_args(BATCHES[key]))
    return out + (capi.debug_fit_many_stats(),)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(BATCHES))
def test_cov_matches_the_long_double_inverse(key):
    coef, cov, rc, st, info, stats = run_cov(key)
    assert rc == 0 and not st.any()
    for k, name in enumerate(BATCHES[key]):
        check_cov(name, cov[k], "device")
    p = cov_problem(BATCHES[key][0])
    assert stats[1] == capi.fit_many_lds_bytes(p["ndim"], list(p["nodes"])) <= LDS_BUDGET and stats[2] == 1
    if key == "g1212":
        assert stats[1] == 62736      # the LDS of the plain fit: the phase added none


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(BATCHES))
def test_fit_results_are_those_of_fit_many_bit_for_bit(key):
    coef, cov, rc, st, info, stats = run_cov(key)
    c0, rc0, st0, info0 = capi.fit_many(*_batch_args(BATCHES[key]))
    stats0 = capi.debug_fit_many_stats()
    keep = [j for j in range(10) if j != 7]
    assert rc == rc0 and np.array_equal(st, st0) and np.array_equal(coef, c0) and np.array_equal(info[:, keep], info0[:, keep])
    assert stats[1] == stats0[1] and stats[0] == stats0[0]


@pytest.mark.gpu
def test_g59_and_g95_hold_the_same_inverse_under_the_node_permutation():
    """The internal order (smaller dimension fastest) does not show: Z of g95 is Z of g59 with the dimensions swapped."""
    a = dense_from_stencil(2, (5, 9), run_cov("g59")[1][1].reshape(45, 25), np.float64)
    b = dense_from_stencil(2, (9, 5), run_cov("g95")[1][0].reshape(45, 25), np.float64)
    perm = np.arange(45).reshape(9, 5).T.ravel()      # node (i0, i1) of g95 = node (i1, i0) of g59
    a = a[np.ix_(perm, perm)]
    d = np.sqrt(np.diag(a))
    # the stencil of a swapped offset is the same set of pairs: compare where both are stored
    both = (a != 0.0) & (b != 0.0)
    assert both.sum() >= 45 * 13
    # (each is within 16 eps kappa_s of the same yardstick)
    assert np.max(np.abs(a - b)[both] / np.outer(d, d)[both]) <= 32 * EPS * yardstick("g59")["kappa"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", LEFT_OUT)
def test_the_wide_hole_runs_with_a_positive_diagonal(name):
    """n130_x*: kappa_s about 4e11, outside the parity by name; status 0 and Z_ii > 0."""
    coef, cov, rc, st, info = capi.fit_many_cov(*_batch_args([name]))
    assert rc == 0 and st[0] == 0
    diag = cov[0].reshape(130, 4)[:, 3]
    assert np.all(np.isfinite(cov[0])) and np.all(diag > 0.0)


@pytest.mark.gpu
def test_status_105_keeps_cov_and_107_zeroes_it():
    good, bad = problem("n9_wide_x1"), problem(SINGULAR)
    off, x, y, _ = pack([bad, good], empty_at=(1,))
    ldcov, ldcoef = 36 + 5, 9 + 2
    cov = np.full((3, ldcov), SENT)
    coef = np.full((3, ldcoef), SENT)
    _, _, rc, st, info = capi.fit_many_cov(1, off, x, y, None, [0.0], [1.0], [9], 0.0, ldcoef=ldcoef, coef=coef, ldcov=ldcov, cov=cov)
    assert rc == 107 and list(st) == [107, 105, 0]
    assert np.all(cov[0, :36] == 0.0) and np.all(coef[0, :9] == 0.0)
    assert np.all(cov[1] == SENT) and np.all(coef[1] == SENT)
    assert np.all(cov[:, 36:] == SENT) and np.all(coef[:, 9:] == SENT)
    c1, v1, rc1, _, _ = capi.fit_many_cov(1, [0, good["y"].size], good["x"], good["y"], None, [0.0], [1.0], [9], 0.0)
    assert rc1 == 0 and np.array_equal(cov[2, :36], v1[0]) and np.array_equal(coef[2, :9], c1[0])
    assert np.all(v1[0].reshape(9, 4)[:, 3] > 0.0)


@pytest.mark.gpu
def test_cov_bits_do_not_depend_on_the_batch_the_position_or_the_entry():
    import torch
    names = ["n9_wide_x3", "n9_cell_x1", "n9_wide_x1", "n9_cell_x17"]
    ps = [problem(n) for n in names]
    off, x, y, _ = pack(ps)
    _, cov, rc, st, _ = capi.fit_many_cov(1, off, x, y, None, [0.0], [1.0], [9], 1.0)
    assert rc == 0
    assert np.array_equal(cov, capi.fit_many_cov(1, off, x, y, None, [0.0], [1.0], [9], 1.0)[1])
    for k, p in enumerate(ps):
        alone = capi.fit_many_cov(1, [0, p["y"].size], p["x"], p["y"], None, [0.0], [1.0], [9], 1.0)[1][0]
        assert np.array_equal(alone, cov[k]), names[k]
        s = cov[k].reshape(9, 4)
        assert np.all(s[0, :3] == 0.0) and np.all(s[1, :2] == 0.0) and s[2, 0] == 0.0 and np.all(s[3:] != 0.0)
    off2, x2, y2, _ = pack(ps[::-1], empty_at=(2,))
    v2 = capi.fit_many_cov(1, off2, x2, y2, None, [0.0], [1.0], [9], 1.0)[1]
    for k, row in enumerate([0, 1, 3, 4]):
        assert np.array_equal(v2[row], cov[len(ps) - 1 - k])
    # the _dev entry, with padded leading dimensions
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    cd = torch.full((len(ps), 12), SENT, dtype=torch.float64, device="cuda")
    vd = torch.full((len(ps), 40), SENT, dtype=torch.float64, device="cuda")
    rc, st, _ = capi.fit_many_cov_dev(1, off, xd, yd, None, [0.0], [1.0], [9], cd, vd, xtrap=1.0, ldcoef=12)
    out = vd.cpu().numpy()
    assert rc == 0 and np.array_equal(out[:, :36], cov) and np.all(out[:, 36:] == SENT)
    # two dimensions and weights, host against _dev, behind an empty problem
    p = problem("w_g59")
    args = (2, [0, 0, p["y"].size])
    v_h = capi.fit_many_cov(*args, p["x"], p["y"], p["w"], [0.0, 0.0], [1.0, 1.0], [5, 9], 0.0)[1]
    vd = torch.full((2, 1125), SENT, dtype=torch.float64, device="cuda")
    cd = torch.zeros((2, 45), dtype=torch.float64, device="cuda")
    rc, st, _ = capi.fit_many_cov_dev(*args, torch.from_numpy(p["x"]).cuda(), torch.from_numpy(p["y"]).cuda(), torch.from_numpy(p["w"]).cuda(),
                                      [0.0, 0.0], [1.0, 1.0], [5, 9], cd, vd)
    out = vd.cpu().numpy()
    assert rc == 105 and list(st) == [105, 0] and np.all(out[0] == SENT) and np.array_equal(out[1], v_h[1])
    assert np.array_equal(v_h[1], run_cov("g59")[1][0])
    _, inside = stencil_columns(2, (5, 9))
    assert np.all(out[1].reshape(45, 25)[~inside] == 0.0) and np.all(out[1].reshape(45, 25)[inside] != 0.0)


@pytest.mark.gpu
def test_f32_is_the_f64_entry_on_the_widened_inputs_rounded_once():
    for key in ("n9", "g59"):
        nd, off, x, y, w, lo, hi, nodes, xtrap = _batch_args(BATCHES[key])
        x32, y32, w32 = x.astype(np.float32), y.astype(np.float32), w.astype(np.float32)
        c32, v32, rc, st, _ = capi.fit_many_cov(nd, off, x32, y32, w32, lo, hi, nodes, xtrap, real32=True)
        c64, v64, rc64, _, _ = capi.fit_many_cov(nd, off, x32.astype(np.float64), y32.astype(np.float64), w32.astype(np.float64), lo, hi, nodes, xtrap)
        assert rc == rc64 == 0 and v32.dtype == np.float32
        assert np.array_equal(v32, v64.astype(np.float32)) and np.array_equal(c32, c64.astype(np.float32))


@pytest.mark.gpu
def test_fit_many_cov_dev_allocates_nothing_on_its_second_call():
    """The pattern of tests/test_stream_order.py: slot [6] of the counters is the device allocations of the call."""
    import torch
    capi.shutdown()      # (the scratch of earlier tests: the first call below has to allocate)
    nd, off, x, y, w, lo, hi, nodes, xtrap = _batch_args(BATCHES["n9"])
    xd, yd, wd = (torch.from_numpy(a).cuda() for a in (x, y, w))
    cd = torch.zeros((4, 9), dtype=torch.float64, device="cuda")
    vd = torch.zeros((4, 36), dtype=torch.float64, device="cuda")
    allocs, covs = [], []
    for _ in range(3):
        rc, st, _ = capi.fit_many_cov_dev(nd, off, xd, yd, wd, lo, hi, nodes, cd, vd, xtrap=xtrap)
        allocs.append(capi.debug_fit_many_stats()[6])
        covs.append(vd.cpu().numpy().copy())
        assert rc == 0
    print(f"device allocations of the three calls: {allocs}")
    assert allocs[0] > 0 and allocs[1] == 0 and allocs[2] == 0, allocs
    assert np.array_equal(covs[0], covs[1]) and np.array_equal(covs[0], run_cov("n9")[1])


FDIR = os.path.join(ROOT, "splpak_amd", "fortran")
PROG = os.path.join(FDIR, "build", "test_fit_many_cov")


@pytest.mark.gpu
def test_fortran_initialize_many_cov_and_variance_each():
    """initialize_many_cov / variance_each against a dense inverse of a 9-node problem formed in the program
    (fortran/test/test_fit_many_cov.f90)."""
    if not os.path.exists(PROG):
        if not os.path.exists("/opt/rocm/bin/amdflang"):
            pytest.skip("amdflang not available")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "splpak_amd", "csrc")])
        subprocess.check_call(["make", "-C", FDIR])
    r = subprocess.run([PROG], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS test_fit_many_cov" in r.stdout
