"""The grid fit with a weight per sample (splpak_fit_grid_weighted_*, csrc/fitgridw.hip): masks, dead pixels, a variance map.

The entry returns the coefficients splcw returns for the listed samples of non-zero weight, provided that fit has no
constraint rows.  Yardsticks: the unmodified reference on the listed samples (live through the `reference` fixture where
oracle/_ref is built, and its recorded coefficients in tests/golden/fit_grid_weighted_ref.npz, written by
tools/gen_fit_grid_weighted_golden.py from the same seeded inputs), the library's own point fit, the separable entry
splpak_fit_grid_*, and numpy for the stages that can be run alone.  Bar 1e-10 max-norm relative, the project's parity bar.

CPU tier: exports, the argument ladder (everything decided before any device call), and a numpy restatement of the algorithm
-- marginals, the Kronecker preconditioner, conjugate gradients to 1e-11, the refinement rule with corrections to 1e-3 --
against the recorded reference: the algebra, pinned without a GPU.  The GPU tier compares the library's iteration counts with
that restatement's.
"""
import functools

import numpy as np
import pytest

from splpak_amd import capi
from tests.conftest import load_golden, relmax
from tests.test_fit_grid import (BAR, HI, LO, LP, POINT_FIT_CASES, XTRAP_TEXT, _dx, apply_axes, axis_matrix, listed_points, random_axes,
                                 xtrap_case)

BAD_WEIGHT_TEXT = "a weight is negative or not finite"
SYMBOLS = ("splpak_fit_grid_weighted_f64", "splpak_fit_grid_weighted_f32", "splpak_fit_grid_weighted_dev_f64",
           "splpak_fit_grid_weighted_dev_f32", "splpak_debug_fit_grid_weighted_stage_f64", "splpak_debug_fit_grid_weighted_stats")


# ---------------------------------------------------------------------------------------------------------------
# The cases
W_PARITY_SHAPES = {"1d": ((40,), (9,)), "2d": ((46, 34), (12, 9)), "3d": ((22, 18, 20), (8, 7, 9)), "4d": ((10, 9, 8, 9), (5, 4, 4, 5))}


def separable(waxes):
    """prod_d waxes[d][i_d] in the layout of the values, (n_D, ..., n_1)."""
    return functools.reduce(np.multiply, np.meshgrid(*waxes[::-1], indexing="ij"))


def sample_weights(shape, waxes, seed, dead=0.15, lo=0.5, hi=2.0):
    """"separable in [0.5, 2] x 15 % dead x U[0.5, 2]": the product of the axis weights (None: 1), a uniform factor per sample
    and a mask, in the layout of the values, (n_D, ..., n_1)."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(lo, hi, shape[::-1])
    if waxes is not None:
        w = w * separable(waxes)
    return w * (rng.random(shape[::-1]) >= dead)


def weighted_case(name):
    """-> (ndim, axes, weights, values with NaN where the weight is 0, nodes, xtrap).  The four xtrap = 0 shapes of the issue on
    jittered-strata axes; "xtrap1": the xtrap_case() sample of test_fit_grid.py with weights U[0.9, 1.1] and nothing masked (the
    golden tool confirms that the reference adds no constraint rows there)."""
    if name == "xtrap1":
        ndim, axes, _, values, nodes = xtrap_case()
        shape = tuple(a.size for a in axes)
        return ndim, axes, sample_weights(shape, None, 5199, dead=0.0, lo=0.9, hi=1.1), values, nodes, 1.0
    shape, nodes = W_PARITY_SHAPES[name]
    ndim = len(shape)
    axes, waxes = random_axes(shape, nodes, 5100 + ndim)
    w = sample_weights(shape, waxes, 5110 + ndim)
    values = np.random.default_rng(5120 + ndim).standard_normal(shape[::-1])
    values[w == 0.0] = np.nan
    return ndim, axes, w, values, list(nodes), 0.0


def point_case(name):
    """The block-edge shapes of POINT_FIT_CASES (test_fit_grid.py) with a weight per sample."""
    shape, nodes, clustered = POINT_FIT_CASES[name]
    ndim = len(shape)
    axes, waxes = random_axes(shape, nodes, 4300 + ndim, clustered)
    w = sample_weights(shape, waxes, 5200 + ndim)
    values = np.random.default_rng(5201).standard_normal(shape[::-1])
    values[w == 0.0] = np.nan
    return ndim, axes, w, values, list(nodes)


def listed_nonzero(axes, weights, values):
    """The samples of non-zero weight as the point fit takes them: (x, y, w)."""
    x, _ = listed_points(axes)
    keep = weights.ravel() != 0.0
    return x[keep], values.ravel()[keep], weights.ravel()[keep]


# ---------------------------------------------------------------------------------------------------------------
# The algorithm in numpy
class NumpyWeightedFit:
    """The algorithm of csrc/fitgridw.hip on dense axis matrices: operator, marginals, preconditioner, conjugate gradients whose
    count is that of the first iterate within the tolerance, and the refinement rule of the grid fits."""

    def __init__(self, ndim, axes, weights, nodes):
        self.A = [axis_matrix(d, nodes[d], axes[d])[0] for d in range(ndim)]
        self.AT = [a.T for a in self.A]
        self.w2 = weights ** 2
        self.on = weights != 0.0
        self.shape = tuple(nodes[::-1])
        D = ndim
        S = self.w2.sum()
        self.marg = [self.w2.sum(axis=tuple(ax for ax in range(D) if ax != D - 1 - d)) for d in range(D)]
        self.Nhat = [(self.A[d].T * (self.marg[d] / S ** ((D - 1) / D))) @ self.A[d] for d in range(D)]
        self.Minv = [np.linalg.inv(n) for n in self.Nhat]
        self.iters = []

    def rhs(self, y):
        return apply_axes(self.AT, self.w2 * np.where(self.on, y, 0.0))

    def op(self, p):
        return apply_axes(self.AT, self.w2 * apply_axes(self.A, p))

    def residual(self, y, x):
        return apply_axes(self.AT, self.w2 * np.where(self.on, y - apply_axes(self.A, x), 0.0))

    def diag(self):
        return apply_axes([a.T ** 2 for a in self.A], self.w2)

    def precondition(self, r):
        return apply_axes(self.Minv, r)

    def cg(self, b, tol, maxit=1000):
        x = np.zeros(self.shape)
        r = b.copy()
        z = self.precondition(r)
        p = z.copy()
        rz = rz0 = np.vdot(r, z)
        k = 0
        while rz0 > 0.0 and k < maxit:
            q = self.op(p)
            alpha = rz / np.vdot(p, q)
            x += alpha * p
            r -= alpha * q
            z = self.precondition(r)
            rz_new = np.vdot(r, z)
            k += 1
            if np.sqrt(rz_new / rz0) <= tol:
                break
            p = z + (rz_new / rz) * p
            rz = rz_new
        self.iters.append(k)
        return x

    def fit(self, y):
        self.iters = []
        x = self.cg(self.rhs(y), 1e-11)
        prev = np.inf
        for it in range(30):
            dx = self.cg(self.residual(y, x), 1e-3)
            x += dx
            rel = np.max(np.abs(dx)) / np.max(np.abs(x))
            if rel <= 1e-11:
                break
            if it >= 1:
                ratio = rel / prev
                if ratio >= 0.9 or rel * ratio / (1.0 - ratio) <= 1e-11:
                    break
            prev = rel
        return x.ravel()


# ---------------------------------------------------------------------------------------------------------------
# CPU tier
def test_fit_grid_weighted_symbols_are_exported():
    L = capi.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS
    for f in (capi.fit_grid_weighted, capi.fit_grid_weighted_dev, capi.debug_fit_grid_weighted_stage, capi.debug_fit_grid_weighted_stats):
        assert callable(f)


def _raw(ndim, npts, nodes, xmin, xmax, coef, axes=None, values=None, weights=None, nfields=1, ldv=None, ldw=0, ldcoef=None, xtrap=0.0):
    """splpak_fit_grid_weighted_f64 with nothing between the test and the entry."""
    npts = np.asarray(npts, dtype=np.int64)
    nodes = np.asarray(nodes, dtype=np.int32)
    xmin = np.asarray(xmin, dtype=np.float64)
    xmax = np.asarray(xmax, dtype=np.float64)
    nsamp = int(np.prod(np.maximum(npts[:max(ndim, 0)], 1)))
    axes = np.full(max(int(np.sum(np.maximum(npts, 0))), 1), 0.3) if axes is None else axes
    values = np.ones(max(nsamp * nfields, 1)) if values is None else values
    weights = np.ones(max(nsamp * nfields, 1)) if weights is None else weights
    return capi.lib().splpak_fit_grid_weighted_f64(ndim, capi._p(npts, LP), capi._p(axes, capi._dp), nfields, capi._p(values, capi._dp),
                                                   nsamp if ldv is None else ldv, capi._p(weights, capi._dp), ldw,
                                                   capi._p(xmin, capi._dp), capi._p(xmax, capi._dp), capi._p(nodes, capi._ip),
                                                   float(xtrap), capi._p(coef, capi._dp), coef.size if ldcoef is None else ldcoef, None)


def test_fit_grid_weighted_status_ladder_without_gpu():
    """The ladder of splpak_fit_grid_* with `weights` among the null checks and `ldw` behind them; the first failing check wins and
    `coef` is untouched on every one of them."""
    coef = np.full(40, 7.0)
    L = capi.lib()
    npts = np.array([9, 8], dtype=np.int64)
    nodes = np.array([6, 5], dtype=np.int32)
    lo, hi = np.array(LO[:2]), np.array(HI[:2])
    ax, val, wts = np.full(17, 0.3), np.ones(72), np.ones(72)
    dp, ip = capi._dp, capi._ip

    def call(npts_=npts, nodes_=nodes, lo_=lo, hi_=hi, ax_=ax, val_=val, wts_=wts, coef_=coef, ndim=2, ldw=0):
        return L.splpak_fit_grid_weighted_f64(ndim, capi._p(npts_, LP), capi._p(ax_, dp), 1, capi._p(val_, dp), 72, capi._p(wts_, dp), ldw,
                                              capi._p(lo_, dp), capi._p(hi_, dp), capi._p(nodes_, ip), 0.0, capi._p(coef_, dp), 40, None)

    for kw in ({"npts_": None}, {"nodes_": None}, {"lo_": None}, {"hi_": None}):
        assert call(ndim=0, **kw) == capi.E_BADARG, kw
    assert _raw(0, [9, 8], [6, 3], LO[:2], [LO[0], HI[1]], coef, ldcoef=1) == 101
    assert _raw(5, [2] * 5, [3] * 5, [0] * 5, [0] * 5, coef, ldcoef=1) == capi.E_UNSUPPORTED
    assert _raw(2, [9, 0], [3, 5], LO[:2], [LO[0], HI[1]], coef, ldcoef=1) == 102
    assert _raw(2, [9, 0], [6, 5], LO[:2], [LO[0], HI[1]], coef, ldcoef=1) == 103
    assert _raw(2, [9, 0], [6, 5], LO[:2], HI[:2], coef, ldcoef=29, nfields=0) == 104
    assert _raw(2, [9, 0], [6, 5], LO[:2], HI[:2], coef, nfields=0, ldw=1) == 105          # before the BADARG group, ldw included
    assert _raw(2, [9, 8], [6, 5], LO[:2], HI[:2], coef, nfields=0) == capi.E_BADARG
    assert _raw(2, [9, 8], [6, 5], LO[:2], HI[:2], coef, ldv=71) == capi.E_BADARG
    assert _raw(2, [2 ** 40, 2 ** 40], [6, 5], LO[:2], HI[:2], coef, axes=np.zeros(1), ldv=2 ** 62) == capi.E_BADARG
    for kw in ({"ax_": None}, {"val_": None}, {"wts_": None}, {"coef_": None}):
        assert call(**kw) == capi.E_BADARG, kw
    # ldw: 0 or at least prod npts
    for ldw in (1, 71, -72):
        assert call(ldw=ldw) == capi.E_BADARG, ldw
        assert "ldw" in capi.last_error()
    assert np.all(coef == 7.0)
    assert L.splpak_debug_fit_grid_weighted_stats(None) == capi.E_BADARG
    # the stage entry shares the ladder (a null `weights` included) and then knows four stages
    out = np.full(30 + 17, 7.0)

    def stage(k, nodes_=nodes, wts_=wts):
        return L.splpak_debug_fit_grid_weighted_stage_f64(k, 2, capi._p(npts, LP), capi._p(ax, dp), capi._p(wts_, dp), capi._p(lo, dp),
                                                          capi._p(hi, dp), capi._p(nodes_, ip), capi._p(val, dp), capi._p(out, dp))

    assert stage(0, nodes_=np.array([6, 3], dtype=np.int32)) == 102
    assert stage(0, wts_=None) == capi.E_BADARG
    assert np.all(out == 7.0)


def test_fit_grid_weighted_rank_deficient_axis_is_107_without_gpu():
    """An axis with too few distinct coordinates is singular whatever the weights: 107 from the host tables, every field zeroed."""
    ax = np.concatenate([np.linspace(LO[d], HI[d], n) for d, n in enumerate((12, 4))])
    coef = np.full(2 * 33, 7.0)
    assert _raw(2, [12, 4], [5, 6], LO[:2], HI[:2], coef, axes=ax, nfields=2, ldcoef=33) == 107
    for k in range(2):
        assert np.all(coef[33 * k:33 * k + 30] == 0.0) and np.all(coef[33 * k + 30:33 * (k + 1)] == 7.0)
    assert "axis 2" in capi.last_error()


@pytest.mark.parametrize("name", ["1d", "2d", "3d", "4d", "xtrap1"])
def test_numpy_restatement_matches_recorded_reference(name):
    """The algebra without a GPU: marginal preconditioner, conjugate gradients, refinement -- against the reference's coefficients
    for the listed samples of non-zero weight."""
    ndim, axes, w, values, nodes, _ = weighted_case(name)
    gold = load_golden("fit_grid_weighted_ref")
    assert int(gold["ierror_" + name]) == 0
    f = NumpyWeightedFit(ndim, axes, w, nodes)
    c = f.fit(values)
    err = relmax(c, gold["coef_" + name])
    print(f"{name}: numpy restatement vs recorded reference {err:.2e}, CG iterations per solve {f.iters}")
    assert err <= BAR
    assert max(f.iters) < 35


# ---------------------------------------------------------------------------------------------------------------
# GPU tier
def _wfit(ndim, axes, w, values, nodes, **kw):
    c, rc, info = capi.fit_grid_weighted(ndim, axes, values, w, LO[:ndim], HI[:ndim], nodes, **kw)
    assert rc == 0, capi.last_error()
    return c, info


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1d", "2d", "3d", "4d", "xtrap1"])
def test_fit_grid_weighted_matches_reference(reference, name):
    """1. Parity with the unmodified reference on the listed samples of non-zero weight: its recorded coefficients, and the
    reference itself where oracle/_ref is built.  The masked samples hold NaN."""
    ndim, axes, w, values, nodes, xtrap = weighted_case(name)
    assert name == "xtrap1" or np.isnan(values).sum() == (w == 0.0).sum() > 0
    c, info = _wfit(ndim, axes, w, values, nodes, xtrap=xtrap)
    gold = load_golden("fit_grid_weighted_ref")
    assert int(gold["ierror_" + name]) == 0
    err = relmax(c, gold["coef_" + name])
    stats = capi.debug_fit_grid_weighted_stats()
    print(f"{name}: vs recorded reference {err:.2e}, refinement steps {info[0, 2]:.0f}, CG iterations {stats[5]} in {stats[6]} solves")
    assert err <= BAR
    assert info[0, 0] == np.count_nonzero(w) and info[0, 1] == 0 and info[0, 6] == 0 and info[0, 9] == 0
    if reference is not None:
        x, y, wl = listed_nonzero(axes, w, values)
        c_ref, rc, _ = reference.fit(ndim, x, y, wl, LO[:ndim], HI[:ndim], nodes, xtrap)
        assert rc == 0
        live = relmax(c, c_ref[:c.size])
        print(f"{name}: vs the live reference {live:.2e}")
        assert live <= BAR


# 2. The block-edge shapes of test_fit_grid.py.  The first pass of the weighted fit (fitw_spread_kernel) is the pass of the last
# dimension; its lane positions are prod_{e<D} npts_e, from 128 on in the wave form.  The marginal pass (fitw_marginal_kernel) works
# level by level from the last dimension down; a workgroup owns 256 lane positions x 32 coordinates.
#   3-D 70x19x21 -> 12x8x9 (and its clustered twin, whose axis 1 has window starts that jump from 0 to 3): first pass: 1330 lanes
#       = 20 waves + 50 lanes, 9 nodes = 2 node blocks + 1 node.  Marginals: level 3: 1330 lane positions = 5 workgroups + 50
#       lanes, 21 coordinates = one partial group; level 2: 70 lanes x 19; level 1: one lane x 70 = 2 groups + 6.
#   2-D 300x65 -> 40x9: first pass: 300 lanes = 4 waves + 44, 3 node blocks, the last of 1.  Marginals: level 2: 300 = 1 workgroup
#       + 44 lanes, 65 coordinates = 2 groups + 1; level 1: 300 coordinates = 9 groups + 12.
#   4-D 20x18x10x9 -> 6x5x4x4: first pass: 3600 lanes = 56 waves + 16, one node block of 4.  Marginals: four levels, 3600, 360, 20
#       and 1 lane positions.
#   2-D 300x30 -> 70x6: first pass: 300 lanes on 6 nodes = 2 node blocks (4 + 2); the preconditioner's solve of the 70-node axis
#       goes in chunks of 8.
# The thread form of the first pass (fewer than 128 lanes) is the 1-D case of test 1 (one lane), its marginals one lane x 40.
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(POINT_FIT_CASES))
def test_fit_grid_weighted_matches_the_point_fit(name):
    ndim, axes, w, values, nodes = point_case(name)
    c, info = _wfit(ndim, axes, w, values, nodes)
    x, y, wl = listed_nonzero(axes, w, values)
    c_pt, rc, _, _ = capi.fit(ndim, x, y, wl, LO[:ndim], HI[:ndim], nodes, 0.0)
    assert rc == 0
    err = relmax(c, c_pt)
    print(f"{name}: weighted grid fit vs point fit {err:.2e}, {info[0, 2]:.0f} refinement steps")
    assert err <= BAR


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(POINT_FIT_CASES))
def test_fit_grid_weighted_stages_alone(name):
    """3. Stages 0, 1 and 3 against numpy, entry by entry, within 1e-12 of the sum of the absolute values of their terms (at most
    ~1e4 terms at these shapes: n eps ~ 1e-12); stage 2 as test_fit_grid_solves_alone takes the solves: the normwise backward error
    of the Kronecker preconditioner."""
    ndim, axes, w, values, nodes = point_case(name)
    f = NumpyWeightedFit(ndim, axes, w, nodes)
    absA = [np.abs(a) for a in f.A]
    absAT = [a.T for a in absA]
    lim = 1e-12
    y = np.where(w != 0.0, values, 0.0)
    T, rc = capi.debug_fit_grid_weighted_stage(0, ndim, axes, w, values, LO[:ndim], HI[:ndim], nodes)      # (NaN where masked)
    assert rc == 0
    bound = lim * apply_axes(absAT, f.w2 * np.abs(y))
    r0 = np.max(np.abs(T.reshape(f.shape) - f.rhs(values)) / bound)
    p = np.random.default_rng(5300).standard_normal(f.shape)
    Np, rc = capi.debug_fit_grid_weighted_stage(1, ndim, axes, w, p, LO[:ndim], HI[:ndim], nodes)
    assert rc == 0
    bound = lim * apply_axes(absAT, f.w2 * apply_axes(absA, np.abs(p)))
    r1 = np.max(np.abs(Np.reshape(f.shape) - f.op(p)) / bound)
    out, rc = capi.debug_fit_grid_weighted_stage(3, ndim, axes, w, None, LO[:ndim], HI[:ndim], nodes)
    assert rc == 0
    ntab = sum(a.size for a in axes)
    marg = np.concatenate(f.marg)
    assert np.all(marg > 0.0)
    r3m = np.max(np.abs(out[:ntab] - marg) / (lim * marg))
    diag = f.diag()
    r3d = np.max(np.abs(out[ntab:].reshape(f.shape) - diag) / (lim * diag))
    print(f"{name}: worst error / bound: right-hand side {r0:.2e}, operator {r1:.2e}, marginals {r3m:.2e}, diagonal {r3d:.2e}")
    assert max(r0, r1, r3m, r3d) <= 1.0
    t = np.random.default_rng(5301).standard_normal(f.shape)
    c, rc = capi.debug_fit_grid_weighted_stage(2, ndim, axes, w, t, LO[:ndim], HI[:ndim], nodes)
    assert rc == 0
    c = c.reshape(f.shape)
    res = np.max(np.abs(apply_axes(f.Nhat, c) - t))
    norm = np.prod([np.max(np.sum(np.abs(n), axis=1)) for n in f.Nhat])
    scale = norm * np.max(np.abs(c)) + np.max(np.abs(t))
    print(f"{name}: preconditioner ||M c - t|| / scale = {res / scale:.2e}")
    assert res <= 1e-12 * scale


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1d", "2d", "3d", "4d"])
def test_fit_grid_weighted_separable_weights_as_a_full_array(name):
    """4. Weights that factor over the axes, given per sample: the preconditioner IS the normal matrix, the iteration ends in a
    step or two, and the result is that of splpak_fit_grid_* on the same axis weights."""
    shape, nodes = W_PARITY_SHAPES[name]
    ndim = len(shape)
    axes, waxes = random_axes(shape, nodes, 5400 + ndim)
    values = np.random.default_rng(5401).standard_normal(shape[::-1])
    w = separable(waxes)
    c, _ = _wfit(ndim, axes, w, values, list(nodes))
    stats = capi.debug_fit_grid_weighted_stats()
    c_sep, rc, _ = capi.fit_grid(ndim, axes, values, LO[:ndim], HI[:ndim], list(nodes), waxes=waxes)
    assert rc == 0
    err = relmax(c, c_sep)
    print(f"{name}: full-array separable weights vs fit_grid {err:.2e}, {stats[5]} CG iterations in {stats[6]} solves")
    assert err <= BAR
    assert stats[5] <= 4


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1d", "2d", "3d", "4d", "xtrap1"] + ["point_" + n for n in sorted(POINT_FIT_CASES)])
def test_fit_grid_weighted_iteration_count(name):
    """5. The library's conjugate-gradient iterations over all solves of the fit against the numpy restatement's for the same
    inputs: at most 1.5 x + 3.  Counts at a fixed tolerance move by a few with the summation order; a count far above the
    restatement's means the preconditioner or the operator is wrong, even where refinement still rescues the answer."""
    if name.startswith("point_"):
        ndim, axes, w, values, nodes = point_case(name[len("point_"):])
        xtrap = 0.0
    else:
        ndim, axes, w, values, nodes, xtrap = weighted_case(name)
    _wfit(ndim, axes, w, values, nodes, xtrap=xtrap)
    stats = capi.debug_fit_grid_weighted_stats()
    f = NumpyWeightedFit(ndim, axes, w, nodes)
    f.fit(values)
    print(f"{name}: CG iterations {stats[5]} in {stats[6]} solves; numpy {sum(f.iters)} in {len(f.iters)} solves {f.iters}")
    assert stats[5] <= 1.5 * sum(f.iters) + 3


@pytest.mark.gpu
def test_fit_grid_weighted_bits_do_not_depend_on_slabs_or_node_block():
    """6. 70x40x120 -> 9x8x12 with a slab scratch of 1 MB (2800 samples per position of the last dimension: 46 positions per
    slab, 3 slabs) against the default (one slab), and node blocks of 1 and 64: the same bits."""
    shape, nodes = (70, 40, 120), [9, 8, 12]
    axes, waxes = random_axes(shape, nodes, 5500)
    w = sample_weights(shape, waxes, 5501)
    values = np.random.default_rng(5502).standard_normal(shape[::-1])
    values[w == 0.0] = np.nan
    c0, i0 = _wfit(3, axes, w, values, nodes)
    s0 = capi.debug_fit_grid_weighted_stats()
    assert s0[0] == 1 and i0[0, 2] >= 1
    capi.set_default_option("fit_grid_scratch_mb", 1)
    try:
        c1, i1 = _wfit(3, axes, w, values, nodes)
        s1 = capi.debug_fit_grid_weighted_stats()
    finally:
        capi.set_default_option("fit_grid_scratch_mb", None)
    assert s1[0] > 1 and s1[1] <= 131072
    assert np.array_equal(c0, c1) and s0[4:7] == s1[4:7]
    assert np.array_equal(i0[0, [0, 2, 3, 4, 8]], i1[0, [0, 2, 3, 4, 8]])
    got = {}
    for nbk in (1, 64):
        capi.set_default_option("fit_grid_node_block", nbk)
        try:
            got[nbk] = _wfit(3, axes, w, values, nodes)
        finally:
            capi.set_default_option("fit_grid_node_block", None)
        assert np.array_equal(got[nbk][0], c0), nbk
        assert np.array_equal(got[nbk][1][0, [0, 2, 3, 4, 8]], i0[0, [0, 2, 3, 4, 8]]), nbk


@pytest.mark.gpu
def test_fit_grid_weighted_bits_do_not_depend_on_fields_or_entry():
    """6, continued.  Three fields in one call against three calls; one weight array for all fields (ldw = 0) against the same
    weights repeated per field (1 and 3 weight analyses); the _dev entry; REAL32 against the f64 entry on the widened inputs."""
    import torch
    shape, nodes = (70, 19, 21), [12, 8, 9]
    axes, waxes = random_axes(shape, nodes, 5600)
    axes = [a.astype(np.float32).astype(np.float64) for a in axes]
    w = sample_weights(shape, waxes, 5601).astype(np.float32).astype(np.float64)
    nsamp, ncol = int(np.prod(shape)), int(np.prod(nodes))
    ldv, ldc = nsamp + 5, ncol + 3
    rng = np.random.default_rng(5602)
    values = np.full(3 * ldv, np.nan)
    for k in range(3):
        v = (rng.standard_normal(nsamp) * 10.0 ** k).astype(np.float32).astype(np.float64)
        v[w.ravel() == 0.0] = np.nan
        values[k * ldv:k * ldv + nsamp] = v
    coef = np.full(3 * ldc, 7.0)
    c, rc, info = capi.fit_grid_weighted(3, axes, values, w, LO[:3], HI[:3], nodes, ldv=ldv, ldw=0, ldcoef=ldc, coef=coef)
    assert rc == 0 and c is coef and info.shape == (3, 10)
    assert capi.debug_fit_grid_weighted_stats()[7] == 1
    singles = []
    for k in range(3):
        c1, i1 = _wfit(3, axes, w, values[k * ldv:k * ldv + nsamp].reshape(shape[::-1]), nodes)
        singles.append(c1)
        assert np.array_equal(coef[k * ldc:k * ldc + ncol], c1), k
        assert np.array_equal(info[k, [0, 1, 2, 3, 4, 8]], i1[0, [0, 1, 2, 3, 4, 8]]), k
        assert np.all(coef[k * ldc + ncol:(k + 1) * ldc] == 7.0), k
    # the same weights per field, ldw apart
    ldw = nsamp + 2
    wrep = np.full(3 * ldw, np.nan)
    for k in range(3):
        wrep[k * ldw:k * ldw + nsamp] = w.ravel()
    c3, rc, _ = capi.fit_grid_weighted(3, axes, values, wrep, LO[:3], HI[:3], nodes, ldv=ldv, ldw=ldw, ldcoef=ldc)
    assert rc == 0 and capi.debug_fit_grid_weighted_stats()[7] == 3
    for k in range(3):
        assert np.array_equal(c3[k * ldc:k * ldc + ncol], singles[k]), k
    # the _dev form: the bits of the host form
    dev = torch.device("cuda")
    v0 = values[:nsamp]
    coef_d = torch.full((ncol + 2,), 7.0, dtype=torch.float64, device=dev)
    rc, info_d = capi.fit_grid_weighted_dev(3, shape, torch.from_numpy(np.concatenate(axes)).to(dev), torch.from_numpy(v0).to(dev),
                                            torch.from_numpy(w.ravel()).to(dev), LO[:3], HI[:3], nodes, coef_d)
    torch.cuda.synchronize()
    assert rc == 0
    got = coef_d.cpu().numpy()
    assert np.array_equal(got[:ncol], singles[0]) and np.all(got[ncol:] == 7.0)
    assert np.array_equal(info_d[0, [0, 2, 3, 4, 8]], info[0, [0, 2, 3, 4, 8]])
    # REAL32: float storage, double arithmetic, one rounding at the store
    c32, rc, _ = capi.fit_grid_weighted(3, axes, v0.reshape(shape[::-1]), w, LO[:3], HI[:3], nodes, real32=True)
    assert rc == 0 and c32.dtype == np.float32
    assert np.array_equal(c32, singles[0].astype(np.float32))
    coef_f = torch.zeros(ncol, dtype=torch.float32, device=dev)
    rc, _ = capi.fit_grid_weighted_dev(3, shape, torch.from_numpy(np.concatenate(axes).astype(np.float32)).to(dev),
                                       torch.from_numpy(v0.astype(np.float32)).to(dev),
                                       torch.from_numpy(w.ravel().astype(np.float32)).to(dev), LO[:3], HI[:3], nodes, coef_f)
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(coef_f.cpu().numpy(), c32)


def _cells_2d(axes, nodes):
    """The node cell (0 .. nodes_d - 2, clipped) of every coordinate of the two axes of the 46x34 -> 12x9 case."""
    return [np.clip(np.floor((axes[d] - LO[d]) / _dx(d, nodes[d])), 0, nodes[d] - 2).astype(int) for d in range(2)]


@pytest.mark.gpu
def test_fit_grid_weighted_singular_and_refused_inputs():
    """7. What the weights can break."""
    shape, nodes = W_PARITY_SHAPES["2d"]
    nodes = list(nodes)
    axes, _ = random_axes(shape, nodes, 5700)
    values = np.random.default_rng(5701).standard_normal(shape[::-1])
    cx, cy = _cells_2d(axes, nodes)

    def masked(ncell):
        w = np.random.default_rng(5702).uniform(0.5, 2.0, shape[::-1])
        w[np.ix_(cy < ncell, cx < ncell)] = 0.0
        v = values.copy()
        v[w == 0.0] = np.nan
        return w, v

    # every sample in the first two node cells of both dimensions masked: the corner coefficient has no sample (the oracle: 107)
    w, v = masked(2)
    c, rc, _ = capi.fit_grid_weighted(2, axes, v, w, LO[:2], HI[:2], nodes)
    assert rc == 107 and np.all(c == 0.0), capi.last_error()
    print("two corner cells masked:", capi.last_error())
    # only the first node cell: a fit like any other
    w, v = masked(1)
    c, _ = _wfit(2, axes, w, v, nodes)
    x, y, wl = listed_nonzero(axes, w, v)
    c_pt, rc, _, _ = capi.fit(2, x, y, wl, LO[:2], HI[:2], nodes, 0.0)
    assert rc == 0
    err = relmax(c, c_pt)
    print(f"one corner cell masked: vs point fit {err:.2e}")
    assert err <= BAR
    # an axis coordinate whose whole hyperplane is masked (its marginal is 0)
    w = np.random.default_rng(5703).uniform(0.5, 2.0, shape[::-1])
    w[:, 7] = 0.0
    w[11, :] = 0.0
    v = values.copy()
    v[w == 0.0] = np.inf
    c, _ = _wfit(2, axes, w, v, nodes)
    x, y, wl = listed_nonzero(axes, w, v)
    c_pt, rc, _, _ = capi.fit(2, x, y, wl, LO[:2], HI[:2], nodes, 0.0)
    assert rc == 0 and relmax(c, c_pt) <= BAR
    # one negative and one NaN weight: refused after the pass over the weights, coef untouched
    for bad in (-1.0, np.nan):
        w = np.ones(shape[::-1])
        w[13, 29] = bad
        coef = np.full(int(np.prod(nodes)), 7.0)
        with pytest.raises(capi.SplpakError, match=BAD_WEIGHT_TEXT):
            capi.fit_grid_weighted(2, axes, values, w, LO[:2], HI[:2], nodes, coef=coef)
        assert np.all(coef == 7.0)
    # xtrap = 1 and a masked block of 3x3 node cells: its inner nodes are data sparse
    w = np.ones(shape[::-1])
    w[np.ix_((cy >= 3) & (cy < 6), (cx >= 4) & (cx < 7))] = 0.0
    coef = np.full(int(np.prod(nodes)), 7.0)
    with pytest.raises(capi.SplpakError, match="constraint rows are not separable") as e:
        capi.fit_grid_weighted(2, axes, values, w, LO[:2], HI[:2], nodes, xtrap=1.0, coef=coef)
    assert XTRAP_TEXT in str(e.value) and "or pass xtrap = 0" in str(e.value)
    assert np.all(coef == 7.0)
    # ... and without the block the same call is answered
    c, rc, _ = capi.fit_grid_weighted(2, axes, values, np.ones(shape[::-1]), LO[:2], HI[:2], nodes, xtrap=1.0)
    assert rc == 0, capi.last_error()


@pytest.mark.gpu
def test_fit_grid_weighted_round_trip():
    """8. Known coefficients resampled on a 60x50 grid, 30 % of it masked with NaN, fitted back with 0/1 weights."""
    shape, nodes = (60, 50), [9, 8]
    axes, _ = random_axes(shape, nodes, 5800)
    coef = np.random.default_rng(5801).standard_normal(int(np.prod(nodes)))
    y, rc = capi.evaluate_grid(2, axes, None, coef, LO[:2], HI[:2], nodes)
    assert rc == 0
    w = (np.random.default_rng(5802).random(shape[::-1]) >= 0.3).astype(np.float64)
    y = np.where(w != 0.0, y, np.nan)
    c, info = _wfit(2, axes, w, y, nodes)
    err = relmax(c, coef)
    print(f"round trip {err:.2e}, residual {info[0, 8]:.2e}")
    assert err <= BAR
    assert info[0, 0] == np.count_nonzero(w)
