"""One plan fitted with CHANGING data against fresh plans (splpak_plan_fit_dev, the one-shot entries' cached plan).

A plan carries the binned points and their offsets, the histogram, the data-sparse flags, the half stencil, the Gram scratch, the
factor storage, the accumulators of the row counts, the preconditioner's tables, the batched refit's copies and the flags that
say what a refit or a debug entry may continue from (csrc/plan.hpp).  The rest of the suite reuses a plan only with the data it
was first fitted with; here a fit follows a fit of OTHER data -- fewer points, other cells occupied, other nodes data sparse, a
107, a refit or a debug solve in between -- and must give the bits of the same fit through a plan that has seen nothing else:
the sums of a fit have one owner and a fixed order (the suite asserts run-to-run bit equality elsewhere).  The fresh plan's
result is then pinned to the CPU oracle (Port.fit_banded) at the project's 1e-10.

All data sets lie inside the unit box, so the one floating-point atomic left, the histogram bump of a far-outside point, is never
taken.  CPU tier: the oracle's statuses and constraint-row counts of the data sets on every grid used (a stale flag or counter
cannot cancel when consecutive counts differ).  GPU tier: tests 1-7 below.
"""
import contextlib
import os

import numpy as np
import pytest

from splpak_amd import capi
from splpak_amd.synth import synth_points
from tests.conftest import relmax
from tests.test_normal_equations import synthetic_spd

COEF_TOL = 1e-10        # the project's bar: max-norm relative
INFO_EXACT = [0, 1, 2, 4, 8, 9]      # row counts, refinement steps, smallest pivot, reserr, backward error; [5..7] are times

# name -> (nodes, points)
GRIDS = {"2d16": ([16, 16], 3000), "3d8": ([8, 8, 8], 3000), "4d6": ([6, 6, 6, 6], 6000), "3d_9_17_13": ([9, 17, 13], 20000),
         # 1.52 constraint rows per column for `dense`: below the 1.6 under which a plan with the iteration in front of a
         # factorisation goes to the factorisation without an attempt (planfit.hip iteration_worth_trying); 3.8 and more for
         # `clustered`, `fewer` and `half_empty` (test_iteration_and_factorisation_alternate)
         "4d6_30k": ([6, 6, 6, 6], 30000)}
SEQUENCE = ["dense", "clustered", "fewer", "half_empty", "zero_w", "dense"]

# label -> (environment while the plan is created, factorisation code the plan must report; None: whatever stands behind the iteration)
SETUPS = {
    "band": ({"SPLPAK_SOLVER": "direct", "SPLPAK_ND": "0", "SPLPAK_NO_TWOEND": "1"}, 1),
    "band_pipeline": ({"SPLPAK_SOLVER": "direct", "SPLPAK_ND": "0", "SPLPAK_NO_TWOEND": "1", "SPLPAK_NARROW_BW": "1"}, 0),
    "twoend": ({"SPLPAK_SOLVER": "direct", "SPLPAK_ND": "0"}, 2),
    "nd": ({"SPLPAK_SOLVER": "direct", "SPLPAK_ND": "1"}, 4),
    "nd_cut2": ({"SPLPAK_SOLVER": "direct", "SPLPAK_ND": "1", "SPLPAK_ND_CUT": "2"}, 4),
    # the panels cleared as a whole and scattered into: the form most exposed to leftovers
    "nd_unstaged": ({"SPLPAK_SOLVER": "direct", "SPLPAK_ND": "1", "SPLPAK_ND_STAGED_INIT": "0"}, 4),
    "pcg+direct": ({"SPLPAK_SOLVER": "pcg+direct"}, None),
    "pcg": ({"SPLPAK_SOLVER": "pcg"}, 6),
}


def data_sets(grid):
    """name -> (x, y, w or None) of the grid's data sets, all inside the unit box."""
    nodes, m = GRIDS[grid]
    x, y, w = synth_points(len(nodes), m)
    k = m // 7
    w0 = w.copy()
    w0[2::3] = 0.0
    return {"dense": (x, y, w), "clustered": (x * x, y, None), "fewer": (x[:k].copy(), y[:k].copy(), w[:k].copy()),
            "half_empty": (0.5 * x, y, w), "zero_w": (x, y, w0)}


_data, _oracle = {}, {}


def _ds(grid, name):
    if grid not in _data:
        _data[grid] = data_sets(grid)
    return _data[grid][name]


def oracle_fit(port, grid, name, xtrap):
    """Port.fit_banded of a data set, computed once -> (coef, ierror, info)."""
    key = (grid, name, xtrap)
    if key not in _oracle:
        nodes, _ = GRIDS[grid]
        nd = len(nodes)
        x, y, w = _ds(grid, name)
        _oracle[key] = port.fit_banded(nd, x, y, w, [0.0] * nd, [1.0] * nd, nodes, xtrap)
    return _oracle[key]


# ---------------------------------------------------------------------------------------------------------------
# CPU tier
@pytest.mark.parametrize("grid", list(GRIDS))
def test_oracle_statuses_and_row_counts_of_the_data_sets(port, grid):
    """What the GPU tests rest on, by the banded CPU oracle: every data set returns 0 at xtrap = 1, consecutive data sets of the
    sequence differ in their constraint-row count, and at xtrap = 0 `half_empty` returns 107 while `dense` returns 0."""
    cons = []
    for name in SEQUENCE:
        _, ierr, info = oracle_fit(port, grid, name, 1.0)
        assert ierr == 0, (grid, name)
        cons.append(int(info[1]))
    print(f"{grid}: constraint rows along the sequence {dict(zip(SEQUENCE[:-1], cons))}")
    assert all(a != b for a, b in zip(cons, cons[1:])), cons
    c, ierr, info = oracle_fit(port, grid, "half_empty", 0.0)
    assert ierr == 107 and not c.any()
    _, ierr, info = oracle_fit(port, grid, "dense", 0.0)
    assert ierr == 0 and info[1] == 0
    if grid == "3d8":
        assert cons[:4] == [876, 1842, 1614, 2688]


# ---------------------------------------------------------------------------------------------------------------
# GPU tier
@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device=torch.device("cuda", 0))


class Reused:
    """One plan (created under the set-up's environment, which it keeps) and what goes through it."""

    def __init__(self, setup, grid, xtrap=1.0):
        env, code = SETUPS[setup]
        self.nodes, self.m = GRIDS[grid]
        self.nd = len(self.nodes)
        with _env(env):
            self.plan = capi.Plan(self.nd, self.nodes, [0.0] * self.nd, [1.0] * self.nd, xtrap, self.m)
        self.code = self.plan.factorisation()[0]
        if (code is not None and self.code != code) or (code is None and self.code == 6):
            self.plan.close()
            raise AssertionError(f"{setup} {self.nodes}: factorisation {self.code}, wanted {code}")

    def fit(self, x, y, w):
        """-> dict(ierr, coef, info, hist, ne: (N, rhs) as the fit assembled them, or None where the plan has nothing to return)"""
        import torch
        xt, yt, wt = _t(x), _t(y), (None if w is None else _t(w))
        coef = torch.full((self.plan.ncol,), 7.5, dtype=torch.float64, device=xt.device)
        ierr, info = self.plan.fit(xt, yt, wt, coef, torch.cuda.current_stream().cuda_stream)
        res = dict(ierr=ierr, coef=coef.cpu().numpy(), info=info, hist=self.plan.histogram())
        try:
            res["ne"] = self.plan.normal_equations()
        except capi.SplpakError as e:
            assert f"error {capi.E_UNSUPPORTED}:" in str(e), str(e)
            res["ne"] = None
        return res

    def refit(self, fields):
        """fields: (nfields, ndata of the last fit) -> dict(ierr, coef (nfields, ncol), info (nfields, 10))"""
        import torch
        yt = _t(fields)
        coef = torch.full((yt.shape[0], self.plan.ncol), 7.5, dtype=torch.float64, device=yt.device)
        ierr, info = self.plan.refit(yt, coef, torch.cuda.current_stream().cuda_stream)
        return dict(ierr=ierr, coef=coef.cpu().numpy(), info=info)

    def close(self):
        self.plan.close()


_fresh = {}


def fresh_fit(setup, grid, name, xtrap=1.0):
    """The data set alone through a plan of its own (same environment, same max_ndata), computed once."""
    key = (setup, grid, name, xtrap)
    if key not in _fresh:
        p = Reused(setup, grid, xtrap)
        try:
            _fresh[key] = p.fit(*_ds(grid, name))
        finally:
            p.close()
    return _fresh[key]


def assert_same_fit(got, want, label):
    assert got["ierr"] == want["ierr"], f"{label}: ierror {got['ierr']} against {want['ierr']}"
    for i in INFO_EXACT:
        assert np.array_equal(got["info"][..., i], want["info"][..., i], equal_nan=True), \
            f"{label}: info[{i}] {got['info'][..., i]} against {want['info'][..., i]}"
    if "hist" in want:
        bad = np.nonzero(got["hist"] != want["hist"])[0]
        assert bad.size == 0, f"{label}: {bad.size} histogram entries differ, first at {bad[:5]}"
    if "ne" in got and "ne" in want:
        assert (got["ne"] is None) == (want["ne"] is None), f"{label}: normal equations {'refused' if got['ne'] is None else 'returned'}, not so by the other plan"
        if got["ne"] is not None:
            for what, a, b in zip(("N", "rhs"), got["ne"], want["ne"]):
                bad = np.argwhere(a != b)
                assert bad.size == 0, f"{label}: {len(bad)} entries of the assembled {what} differ, first at {bad[:3].tolist()}"
    if not np.array_equal(got["coef"], want["coef"]):
        raise AssertionError(f"{label}: coefficients differ, max-norm relative {relmax(got['coef'], want['coef']):.3e}")


def assert_oracle(port, res, grid, name, xtrap, label):
    """The fresh plan's fit against Port.fit_banded: status, row counts, coefficients at the project's bar -> the error."""
    c, ierr, info = oracle_fit(port, grid, name, xtrap)
    assert res["ierr"] == ierr, f"{label}: ierror {res['ierr']}, the oracle's {ierr}"
    assert (res["info"][0], res["info"][1]) == (info[0], info[1]), f"{label}: rows {res['info'][:2]}, the oracle's {info[:2]}"
    if ierr != 0:
        assert not res["coef"].any(), label
        return 0.0
    err = relmax(res["coef"], c)
    assert err < COEF_TOL, f"{label}: {err:.2e} from the oracle"
    return err


SEQUENCE_CASES = [("band", "2d16"), ("band", "3d8"), ("band", "4d6"), ("band_pipeline", "3d_9_17_13"), ("twoend", "3d_9_17_13"),
                  ("nd", "3d8"), ("nd", "3d_9_17_13"), ("nd", "4d6"), ("nd_cut2", "3d_9_17_13"), ("nd_unstaged", "3d_9_17_13"),
                  ("pcg+direct", "4d6"), ("pcg", "4d6"), ("pcg", "3d8")]


@pytest.mark.gpu
@pytest.mark.parametrize("setup,grid", SEQUENCE_CASES, ids=[f"{s}-{g}" for s, g in SEQUENCE_CASES])
def test_sequence_matches_fresh_plans(port, setup, grid):
    """1. One plan at xtrap = 1 fits dense, clustered, fewer, half_empty, zero_w and dense again; every step has the status, the
    coefficients, info[0, 1, 2, 4, 8, 9] and the histogram of a fresh plan fitting that data set alone, bit for bit; the fresh
    plan's coefficients are within 1e-10 of Port.fit_banded with its row counts; the last step has the first step's bits.
    The iteration-only plans (code 6) are anchored to the oracle where the fresh plan returns 0; where it returns 107 (DESIGN 4c's
    stagnation regime) the reused plan must return 107 with zeroed coefficients too, and `dense` must return 0.
    Measured on an MI355X: every step of every set-up returns 0, the iteration-only plans included (6^4 with 6 000 points has 3.5
    to 9.4 constraint rows per column along the sequence, 8^3 with 3 000 points 1.7 to 5.3: outside the stagnation regime), so
    every step is anchored to the oracle; the fresh plans are 5e-16 ... 2e-13 from it.  pcg+direct on 6^4 reports code 2 (the
    two-ended band behind the iteration) and the iteration answers every step of this sequence:
    test_iteration_and_factorisation_alternate makes the factorisation take its turn."""
    p = Reused(setup, grid)
    steps, errs = [], []
    try:
        for k, name in enumerate(SEQUENCE):
            got = p.fit(*_ds(grid, name))
            want = fresh_fit(setup, grid, name)
            label = f"{setup} {grid} step {k} ({name})"
            assert_same_fit(got, want, label)
            if p.code == 6 and want["ierr"] == 107:
                assert not got["coef"].any() and not want["coef"].any(), label
                errs.append(float("nan"))
            else:
                errs.append(assert_oracle(port, want, grid, name, 1.0, label))
            steps.append(got)
    finally:
        p.close()
    print(f"{setup} {grid}: factorisation {p.code}; statuses {[s['ierr'] for s in steps]}; constraint rows {[int(s['info'][1]) for s in steps]}; "
          f"refinement steps {[int(s['info'][2]) for s in steps]}; fresh plan against the oracle {['%.1e' % e for e in errs]}")
    assert steps[0]["ierr"] == 0
    assert_same_fit(steps[-1], steps[0], f"{setup} {grid}: dense again against the first step")


FAILURE_CASES = [("band", "3d8"), ("twoend", "3d_9_17_13"), ("nd", "3d_9_17_13"), ("pcg+direct", "4d6"), ("pcg", "4d6"), ("pcg", "3d8")]


@pytest.mark.gpu
@pytest.mark.parametrize("setup,grid", FAILURE_CASES, ids=[f"{s}-{g}" for s, g in FAILURE_CASES])
def test_failure_in_the_middle(port, setup, grid):
    """2. A plan at xtrap = 0 fits dense, then half_empty (107, coefficients zero), then dense: the third fit equals the first and
    a fresh plan's bit for bit -- the assembled normal equations included --, and the fresh plan's is the oracle's.  After the
    failed fit the diagnostics entries refuse (include/splpak_hip.h: splpak_debug_plan_normal_equations, _rows_gradient): they
    must not describe the failed fit's leftovers, nor the first fit."""
    p = Reused(setup, grid, xtrap=0.0)
    try:
        first = p.fit(*_ds(grid, "dense"))
        failed = p.fit(*_ds(grid, "half_empty"))
        _refused(lambda: p.plan.rows_gradient(np.zeros(p.plan.ncol)))
        third = p.fit(*_ds(grid, "dense"))
    finally:
        p.close()
    want = fresh_fit(setup, grid, "dense", 0.0)
    print(f"{setup} {grid} xtrap 0: factorisation {p.code}; statuses {[first['ierr'], failed['ierr'], third['ierr']]}")
    assert failed["ierr"] == 107 and not failed["coef"].any()
    assert failed["ne"] is None, "splpak_debug_plan_normal_equations answered after a failed fit"
    assert (first["ne"] is None) == ((setup, grid) == ("pcg", "4d6"))       # (only the rows-only plan never assembles)
    assert_same_fit(failed, fresh_fit(setup, grid, "half_empty", 0.0), f"{setup} {grid}: the failed fit")
    assert first["ierr"] == 0
    assert_same_fit(first, want, f"{setup} {grid}: first fit")
    assert_same_fit(third, first, f"{setup} {grid}: dense after the 107 against the first fit")
    assert_same_fit(third, want, f"{setup} {grid}: dense after the 107 against a fresh plan")
    assert_oracle(port, want, grid, "dense", 0.0, f"{setup} {grid} xtrap 0")


EDGE_CASES = [("band", "2d16"), ("nd", "3d_9_17_13"), ("pcg+direct", "4d6")]


@pytest.mark.gpu
@pytest.mark.parametrize("setup,grid", EDGE_CASES, ids=[f"{s}-{g}" for s, g in EDGE_CASES])
def test_point_count_and_layout_edges(setup, grid):
    """3. Through one plan: ndata == max_ndata, then m // 7 points, then max_ndata again; l1xdat = ndim + 2 with 1e300 in the
    padding columns against l1xdat = ndim; weights absent, given, and with a negative first weight ("no weights").  Each equals
    the fresh plan's fit of the same points (the padded ones: of the unpadded)."""
    x, y, w = _ds(grid, "dense")
    xf, yf, wf = _ds(grid, "fewer")
    pad = lambda a: np.hstack([a, np.full((a.shape[0], 2), 1e300)])
    wneg = w.copy()
    wneg[0] = -1.0
    p = Reused(setup, grid)
    try:
        alone = []
        for wv in (None, wneg):
            q = Reused(setup, grid)
            try:
                alone.append(q.fit(x, y, wv))
            finally:
                q.close()
        want_now, want_neg = alone
        assert_same_fit(want_neg, want_now, f"{setup} {grid}: a negative first weight against no weights, fresh plans")
        seq = [("ndata == max_ndata", (x, y, w), fresh_fit(setup, grid, "dense")),
               ("m // 7 points", (xf, yf, wf), fresh_fit(setup, grid, "fewer")),
               ("max_ndata again", (x, y, w), fresh_fit(setup, grid, "dense")),
               ("m // 7 points, l1xdat = ndim + 2", (pad(xf), yf, wf), fresh_fit(setup, grid, "fewer")),
               ("l1xdat = ndim + 2", (pad(x), y, w), fresh_fit(setup, grid, "dense")),
               ("l1xdat = ndim", (x, y, w), fresh_fit(setup, grid, "dense")),
               ("no weights", (x, y, None), want_now),
               ("weights", (x, y, w), fresh_fit(setup, grid, "dense")),
               ("negative first weight", (x, y, wneg), want_neg)]
        for what, args, want in seq:
            got = p.fit(*args)
            assert want["ierr"] == 0
            assert_same_fit(got, want, f"{setup} {grid}: {what}")
    finally:
        p.close()
    assert not np.array_equal(want_now["coef"], fresh_fit(setup, grid, "dense")["coef"])


def _fields(x, y, which):
    """Three fields on the points x (which: 0 or 1, two different sets)."""
    s = x.sum(axis=1)
    if which == 0:
        return np.stack([np.cos(3.0 * s) + 0.25 * y, np.sin(2.0 * s), y * y])
    return np.stack([np.sin(5.0 * s) - 0.5 * y, np.cos(s) * y, 1.0 + s])


def _refused(call):
    with pytest.raises(capi.SplpakError) as ei:
        call()
    assert f"error {capi.E_UNSUPPORTED}:" in str(ei.value), str(ei.value)


REFIT_CASES = [("nd", "3d_9_17_13"), ("band", "3d8"), ("pcg+direct", "4d6")]


@pytest.mark.gpu
@pytest.mark.parametrize("setup,grid", REFIT_CASES, ids=[f"{s}-{g}" for s, g in REFIT_CASES])
def test_refits_in_between(setup, grid):
    """4. fit(dense), a refit of 3 fields (on nested dissection the batched route, so the per-field copies exist), fit(clustered),
    a refit of 3 other fields: the second fit and every field of the second refit equal a fresh plan doing fit(clustered) and that
    refit.  Then, at xtrap = 0: fit(dense), fit(half_empty) = 107, and a refit -- refused with SPLPAK_E_UNSUPPORTED as
    include/splpak_hip.h says, not answered from the first fit's state."""
    xd, yd, wd = _ds(grid, "dense")
    xc, yc, wc = _ds(grid, "clustered")
    p, q = Reused(setup, grid), Reused(setup, grid)
    try:
        assert p.fit(xd, yd, wd)["ierr"] == 0
        r0 = p.refit(_fields(xd, yd, 0))
        assert r0["ierr"] == 0
        if setup == "nd":
            assert p.plan.refit_stats()[0] == 2
        fit2 = p.fit(xc, yc, wc)
        r1 = p.refit(_fields(xc, yc, 1))
        want = q.fit(xc, yc, wc)
        w1 = q.refit(_fields(xc, yc, 1))
        routes = (p.plan.refit_stats()[0], q.plan.refit_stats()[0])
    finally:
        p.close()
        q.close()
    print(f"{setup} {grid}: factorisation {p.code}; refit routes {routes}; refit statuses {r0['ierr']}, {r1['ierr']}; steps {r1['info'][:, 2]}")
    assert_same_fit(fit2, want, f"{setup} {grid}: fit(clustered) after fit(dense) + refit")
    assert_same_fit(fit2, fresh_fit(setup, grid, "clustered"), f"{setup} {grid}: fit(clustered) against the fresh plan of test 1")
    assert w1["ierr"] == 0 and routes[0] == routes[1]
    assert_same_fit(r1, w1, f"{setup} {grid}: the second refit")
    p = Reused(setup, grid, xtrap=0.0)
    try:
        assert p.fit(xd, yd, wd)["ierr"] == 0
        xh, yh, wh = _ds(grid, "half_empty")
        assert p.fit(xh, yh, wh)["ierr"] == 107
        _refused(lambda: p.refit(_fields(xd, yd, 0)))
    finally:
        p.close()


DEBUG_CASES = [("band", "3d8"), ("band_pipeline", "3d_9_17_13"), ("twoend", "3d_9_17_13"), ("nd", "3d_9_17_13")]


@pytest.mark.gpu
@pytest.mark.parametrize("setup,grid", DEBUG_CASES, ids=[f"{s}-{g}" for s, g in DEBUG_CASES])
def test_debug_entries_in_between(setup, grid):
    """5. splpak_debug_plan_normal_equations and a splpak_debug_plan_solve of a synthetic SPD matrix between two fits of
    different data: the next fit equals a fresh plan's; a refit directly after the debug solve is refused (include/splpak_hip.h,
    splpak_plan_refit_dev)."""
    nodes, _ = GRIDS[grid]
    xd, yd, wd = _ds(grid, "dense")
    N = synthetic_spd(nodes, 7)
    b = np.random.default_rng(8).uniform(-1.0, 1.0, N.shape[0])
    p = Reused(setup, grid)
    try:
        assert_same_fit(p.fit(xd, yd, wd), fresh_fit(setup, grid, "dense"), f"{setup} {grid}: first fit")
        p.plan.normal_equations()
        x1, rc, mp = p.plan.debug_solve(N, b)
        assert rc == 0 and mp > 0
        _refused(lambda: p.refit(_fields(xd, yd, 0)))
        assert_same_fit(p.fit(*_ds(grid, "clustered")), fresh_fit(setup, grid, "clustered"), f"{setup} {grid}: fit(clustered) after the debug entries")
        p.plan.normal_equations()
        x2, rc, _ = p.plan.debug_solve(N, b)
        assert rc == 0 and np.array_equal(x1, x2)
        assert_same_fit(p.fit(*_ds(grid, "half_empty")), fresh_fit(setup, grid, "half_empty"), f"{setup} {grid}: fit(half_empty) after the debug solve")
        assert_same_fit(p.fit(xd, yd, wd), fresh_fit(setup, grid, "dense"), f"{setup} {grid}: fit(dense) at the end")
    finally:
        p.close()


@pytest.mark.gpu
def test_iteration_and_factorisation_alternate(port):
    """7. A 4-D plan with the iteration in front of a factorisation (pcg+direct) assembles the normal equations only when the
    factorisation is going to run (planfit.hip plan_lazy_assembly), and skips the iteration below 1.6 constraint rows per column.
    On 6^4 with 30 000 points `dense` (1.52) is factored -- assembled late, from the binned points -- while `clustered` and
    `fewer` are answered by the iteration from the rows alone: through one plan dense, clustered, dense, fewer, dense, with a
    refit of three fields after each of the first two.  Every fit and refit equals a fresh plan's bit for bit, which solver
    answered is asserted from info[4] (the factor's smallest pivot, 0 without a factorisation) and the iteration's counters, and
    after a fit the iteration answered splpak_debug_plan_normal_equations refuses instead of returning the previous fit's."""
    setup, grid = "pcg+direct", "4d6_30k"
    ncol = int(np.prod(GRIDS[grid][0]))
    p = Reused(setup, grid)
    how = []
    try:
        for k, name in enumerate(["dense", "clustered", "dense", "fewer", "dense"]):
            x, y, w = _ds(grid, name)
            got = p.fit(x, y, w)
            stats = p.plan.pcg_stats()
            factored = name == "dense"
            label = f"{setup} {grid} step {k} ({name})"
            how.append((got["ierr"], int(got["info"][1]), got["info"][4] != 0.0, stats["solves"]))
            assert got["ierr"] == 0, label
            assert (got["info"][4] != 0.0) == factored and (stats["solves"] == 0) == factored, f"{label}: {how[-1]}"
            assert (got["ne"] is not None) == factored, label
            want = fresh_fit(setup, grid, name)
            assert_same_fit(got, want, label)
            assert_oracle(port, want, grid, name, 1.0, label)
            if k < 2:
                fields = _fields(x, y, k)
                r = p.refit(fields)
                q = Reused(setup, grid)
                try:
                    assert_same_fit(q.fit(x, y, w), want, f"{label}: a second fresh plan")
                    assert_same_fit(r, q.refit(fields), f"{label}: refit of three fields")
                finally:
                    q.close()
                assert r["ierr"] == 0 and r["coef"].shape == (3, ncol)
    finally:
        p.close()
    print(f"{setup} {grid}: factorisation {p.code}; (status, constraint rows, factored, solves of the iteration) {how}")


def _one_shot(grid, name, real32=False):
    nodes, _ = GRIDS[grid]
    nd = len(nodes)
    x, y, w = _ds(grid, name)
    coef, ierr, hist, info = capi.fit(nd, x, y, w, [0.0] * nd, [1.0] * nd, nodes, 1.0, want_hist=True, real32=real32)
    return dict(ierr=ierr, coef=coef, info=info, hist=hist)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", ["3d8", "3d_9_17_13"])
def test_one_shot_cache(port, grid, monkeypatch):
    """6. The sequence through capi.fit (the plan the one-shot entry keeps, default solver choice), and again under
    SPLPAK_NO_PLAN_CACHE=1: every step has the same bits, info and histogram.  It starts with `fewer`, so the later `dense` exceeds
    the cached plan's max_ndata and forces a new plan.  A refit by token after the last step equals a refit through a fresh Plan.
    The REAL32 entry once: `dense` after `clustered` equals the same call after shutdown()."""
    for k in ("SPLPAK_SOLVER", "SPLPAK_ND", "SPLPAK_NO_PLAN_CACHE"):
        monkeypatch.delenv(k, raising=False)
    nodes, m = GRIDS[grid]
    nd, ncol = len(nodes), int(np.prod(nodes))
    seq = ["fewer"] + SEQUENCE
    capi.shutdown()
    try:
        cached = [_one_shot(grid, name) for name in seq]
        xd, yd, wd = _ds(grid, "dense")
        fields = _fields(xd, yd, 1)
        assert cached[-1]["ierr"] == 0 and capi.fit_token() != 0
        rc_coef, rc, rc_info = capi.refit(capi.fit_token(), fields, ncol)
        monkeypatch.setenv("SPLPAK_NO_PLAN_CACHE", "1")
        uncached = [_one_shot(grid, name) for name in seq]
        monkeypatch.delenv("SPLPAK_NO_PLAN_CACHE")
        for k, name in enumerate(seq):
            assert_same_fit(cached[k], uncached[k], f"one-shot {grid} step {k} ({name}): cached plan against no cache")
            assert_oracle(port, uncached[k], grid, name, 1.0, f"one-shot {grid} step {k} ({name})")
        print(f"one-shot {grid}: statuses {[s['ierr'] for s in cached]}; constraint rows {[int(s['info'][1]) for s in cached]}")
        p = capi.Plan(nd, nodes, [0.0] * nd, [1.0] * nd, 1.0, m)
        try:
            import torch
            coef = torch.zeros(ncol, dtype=torch.float64, device="cuda")
            ierr, info = p.fit(_t(xd), _t(yd), _t(wd), coef)
            assert_same_fit(cached[-1], dict(ierr=ierr, coef=coef.cpu().numpy(), info=info, hist=p.histogram()), f"one-shot {grid}: last step against a Plan")
            c2 = torch.zeros((3, ncol), dtype=torch.float64, device="cuda")
            ierr, info = p.refit(_t(fields), c2)
        finally:
            p.close()
        assert_same_fit(dict(ierr=rc, coef=rc_coef, info=rc_info), dict(ierr=ierr, coef=c2.cpu().numpy(), info=info), f"one-shot {grid}: refit by token")
        capi.shutdown()
        assert _one_shot(grid, "clustered", real32=True)["ierr"] == 0
        after = _one_shot(grid, "dense", real32=True)
        capi.shutdown()
        alone = _one_shot(grid, "dense", real32=True)
        assert alone["ierr"] == 0 and alone["coef"].dtype == np.float32
        assert_same_fit(after, alone, f"one-shot {grid} REAL32: dense after clustered against dense alone")
    finally:
        capi.shutdown()
