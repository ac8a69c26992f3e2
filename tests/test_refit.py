"""Refit: new values on the points of a plan's last fit (splpak_plan_refit_dev, splpak_refit_f64 / _f32; splpak_amd/csrc/planfit.hip, hostfit.hip).

Only the solve of a fit depends on ydata; the binned points, the constraint rows, N = A^T W^2 A + C^T C, its factor and the
iteration's preconditioner are kept by the plan.  What is checked, and against what:
  * the reference's goldens (tests/golden/*.npz) at the project's 1e-10 through every solver a plan can hold -- narrow and
    two-ended band, nested dissection, the tiled 4-D row operator, the iteration alone and in front of a factorisation;
  * a second field y2 = cos(3 sum_d x_d) + 0.25 y against a fit of its own (2e-10: both lie within 1e-10 of the same
    minimiser), against itself bit for bit, and against the dense oracle (tests/golden/refit_y2.npz, written by
    tools/gen_refit_golden.py from oracle Port.fit; a case missing from it fails the test);
  * the shapes the values gather can get wrong, the diagnostics, the statuses, and the one-shot entries.
"""
import contextlib
import os

import numpy as np
import pytest

from splpak_amd import capi
from splpak_amd.synth import synth_points
from tests.cases import CASES, make_inputs
from tests.conftest import GOLDEN, load_golden, relmax

pytestmark = pytest.mark.gpu

COEF_TOL = 1e-10        # the project's bar: max-norm relative
PAIR_TOL = 2e-10        # two results that each meet the bar against the same minimiser
EPS32 = float(np.finfo(np.float32).eps)

GOLDEN_CASES = ["c1_1d16", "1d_sparse", "2d16_zero_w", "2d16_outside", "2d32_cc_xt0", "3d8_cc_clust", "3d_aniso", "3d16",
                "2d64_c2grid", "4d6"]
ND_CASES = ("3d16", "2d64_c2grid")


def second_field(inp):
    return np.cos(3.0 * inp["xdata"].sum(axis=1)) + 0.25 * inp["ydata"]


_oracle_y2 = {}


def oracle_second_field(name):
    """Coefficients of y2 from the dense oracle (Port.fit, the way test_fit_fresh_inputs_vs_oracle obtains its reference), as
    tools/gen_refit_golden.py recorded them: the grids of 4 096 columns take the oracle the better part of an hour."""
    if not _oracle_y2:
        _oracle_y2.update(np.load(os.path.join(GOLDEN, "refit_y2.npz")))
    assert name in _oracle_y2, f"tests/golden/refit_y2.npz holds no '{name}': run tools/gen_refit_golden.py {name}"
    return _oracle_y2[name]


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


class Session:
    """One plan with its points on the device (a plan keeps the options it was created under)."""

    def __init__(self, inp, env=None, max_ndata=None, comm=False):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.st = torch.cuda.current_stream().cuda_stream
        self.inp = inp
        self.x = torch.tensor(np.ascontiguousarray(inp["xdata"], dtype=np.float64), device=self.dev)
        self.w = None if inp["wdata"] is None else torch.tensor(np.ascontiguousarray(inp["wdata"], dtype=np.float64), device=self.dev)
        self.ndata = self.x.shape[0]
        self.ncol = int(np.prod(inp["nodes"]))
        buf = None
        if comm:
            nodes = np.ascontiguousarray(inp["nodes"], dtype=np.int32)
            n = int(capi.lib().splpak_plan_comm_len(inp["ndim"], capi._p(nodes, capi._ip)))
            buf = torch.zeros(n, dtype=torch.float64, device=self.dev)
        with _env(env or {}):
            self.plan = capi.Plan(inp["ndim"], inp["nodes"], inp["xmin"], inp["xmax"], inp["xtrap"], max_ndata or self.ndata, comm=buf)

    def t(self, a):
        return self.torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device=self.dev)

    def fit(self, y, x=None, w=None):
        c = self.torch.zeros(self.ncol, dtype=self.torch.float64, device=self.dev)
        rc, info = self.plan.fit(self.x if x is None else x, self.t(y), self.w if x is None else w, c, self.st)
        return c.cpu().numpy(), rc, info

    def refit(self, y):
        c = self.torch.full((self.ncol,), 7.5, dtype=self.torch.float64, device=self.dev)
        rc, info = self.plan.refit(self.t(y), c, self.st)
        return c.cpu().numpy(), rc, info

    def close(self):
        self.plan.close()


def _refused(call, code):
    with pytest.raises(capi.SplpakError) as ei:
        call()
    assert f"error {code}:" in str(ei.value), str(ei.value)
    return str(ei.value)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_refit_golden_through_every_solver(name):
    """Fit y2, refit the case's own values (golden), refit y2 (the fit's coefficients, itself bit for bit, the oracle); the
    diagnostics of every refit."""
    gold = load_golden(name)
    inp = make_inputs(CASES[name])
    y, y2 = inp["ydata"], second_field(inp)
    s = Session(inp)
    try:
        c_fit2, rc, info_fit = s.fit(y2)
        assert rc == 0
        code = s.plan.factorisation()[0]
        if name in ND_CASES:
            assert code == 4
        held = info_fit[4] != 0.0                      # a factorisation ran in the fit: the refits use its factor
        c_y, rc, info_y = s.refit(y)
        assert rc == 0
        c_a, rc_a, info_a = s.refit(y2)
        c_b, rc_b, info_b = s.refit(y2)
        assert rc_a == 0 and rc_b == 0
        ref2 = oracle_second_field(name)
        print(f"{name}: factorisation code {code}; refit vs golden {relmax(c_y, gold['coef']):.2e}; refit of y2 vs its fit {relmax(c_a, c_fit2):.2e}, "
              f"vs the oracle {relmax(c_a, ref2):.2e}; steps {info_y[2]:.0f} / {info_a[2]:.0f}; backward error {info_y[9]:.1e} / {info_a[9]:.1e}; "
              f"reserr of y2 refit {info_a[8]:.12e} fit {info_fit[8]:.12e}")
        assert relmax(c_y, gold["coef"]) < COEF_TOL
        assert relmax(c_a, c_fit2) < PAIR_TOL
        assert np.array_equal(c_a, c_b)
        assert relmax(c_a, ref2) < COEF_TOL
        for info in (info_y, info_a, info_b):
            assert info[0] == info_fit[0] and info[1] == info_fit[1]
            assert info[9] < 1e-9
            assert info[5] == 0.0
            if held:
                assert info[6] == 0.0 and info[4] == info_fit[4]
        assert abs(info_a[8] - info_fit[8]) <= 1e-9 * info_fit[8]
        assert np.array_equal(info_a[[0, 1, 2, 3, 4, 8, 9]], info_b[[0, 1, 2, 3, 4, 8, 9]])
    finally:
        s.close()


@pytest.mark.parametrize("solver,env", [("pcg", {"SPLPAK_SOLVER": "pcg"}),
                                        ("pcg+direct", {"SPLPAK_SOLVER": "pcg+direct", "SPLPAK_PCG_ALWAYS": "1"})])
def test_refit_with_the_iteration(solver, env):
    """4d6 on a plan that iterates: alone (the golden at 1e-10 or the reference's 107, as tests/test_pcg.py accepts for the fit)
    and in front of a factorisation (must succeed: the iteration again on the prepared preconditioner, or the factorisation
    from the binned points when it gives up)."""
    name = "4d6"
    gold = load_golden(name)
    inp = make_inputs(CASES[name])
    s = Session(inp, env=env)
    try:
        if solver == "pcg":
            assert s.plan.factorisation()[0] == 6
        c2, rc, info_fit = s.fit(second_field(inp))
        if solver == "pcg":
            assert rc in (0, 107)
            if rc == 107:
                _refused(lambda: s.refit(inp["ydata"]), capi.E_UNSUPPORTED)
                return
        else:
            assert rc == 0
        c, rc, info = s.refit(inp["ydata"])
        ps = s.plan.pcg_stats()
        print(f"{solver}: refit status {rc}; fit answered by {'the iteration' if info_fit[4] == 0.0 else 'the factorisation'}, refit by "
              f"{'the iteration' if info[4] == 0.0 else 'the factorisation'}; {ps['iterations']} iterations in {ps['solves']} solves; "
              f"vs golden {relmax(c, gold['coef']):.2e}; backward error {info[9]:.1e}")
        if solver == "pcg":
            assert rc in (0, 107)
        else:
            assert rc == 0
        if rc == 0:
            assert relmax(c, gold["coef"]) < COEF_TOL and info[9] < 1e-9
            assert info[0] == info_fit[0] and info[1] == info_fit[1]
            if solver == "pcg":
                assert info[4] == 0.0 and info[6] == 0.0 and ps["iterations"] > 0
        else:
            assert "iterative solve did not converge" in capi.last_error()
            assert np.all(c == 0.0)
    finally:
        s.close()


def test_refit_factors_when_its_iteration_gives_up():
    """A fit the iteration answered, then a refit whose iteration cannot meet its tolerance (pcg_tol1 = -1 on the plan: no
    residual meets it, the solve ends at its iteration limit or in a breakdown): the normal equations are assembled from the binned points and factored as a fit does, and the next field uses the factor."""
    name = "4d6"
    gold = load_golden(name)
    inp = make_inputs(CASES[name])
    s = Session(inp, env={"SPLPAK_SOLVER": "pcg+direct", "SPLPAK_PCG_ALWAYS": "1"})
    try:
        c2, rc, info_fit = s.fit(second_field(inp))
        assert rc == 0 and info_fit[4] == 0.0 and info_fit[6] == 0.0        # (the iteration answers 4d6: tests/test_pcg.py)
        s.plan.set_option("pcg_tol1", "-1")
        c, rc, info = s.refit(inp["ydata"])
        s.plan.set_option("pcg_tol1", None)
        print(f"refit after the iteration gave up: vs golden {relmax(c, gold['coef']):.2e}, smallest pivot {info[4]:.3e}, {info[6]:.4f} s in the fallback")
        assert rc == 0 and relmax(c, gold["coef"]) < COEF_TOL and info[9] < 1e-9
        assert info[4] > 0.0 and info[6] > 0.0
        assert info[0] == info_fit[0] and info[1] == info_fit[1]
        cb, rc, info_b = s.refit(second_field(inp))
        assert rc == 0 and relmax(cb, c2) < PAIR_TOL
        assert info_b[6] == 0.0 and info_b[4] == info[4]
    finally:
        s.close()


def test_stage_timing_after_a_fit_and_a_refit():
    """include/splpak_hip.h on splpak_plan_stage_timing after a refit: [1] is the values gather + right-hand side, [0] and [2]
    are 0, [3] is 0 unless the factorisation ran, [4] [5] as for the fit.  On the band (2d16) and on nested dissection (3d16) with
    the held factor, and on 4d6 where the refit's iteration gives up and it factors.  Signs and zeros only, never durations."""
    def timing(s):
        t = s.plan.stage_timing()
        print({k: float(v) for k, v in t.items()})
        assert all(np.isfinite(v) and v >= 0.0 for v in t.values()), t
        return t

    for name in ("2d16", "3d16"):
        inp = make_inputs(CASES[name])
        s = Session(inp)
        try:
            s.plan.enable_kernel_timing()
            _, rc, info = s.fit(second_field(inp))
            assert rc == 0 and info[4] != 0.0                       # (a factorisation ran: the refit holds its factor)
            t = timing(s)
            assert t["bin_ms"] > 0.0 and t["gram_ms"] > 0.0 and t["expand_ms"] > 0.0 and t["solve_ms"] > 0.0, (name, t)
            _, rc, info = s.refit(inp["ydata"])
            assert rc == 0 and info[6] == 0.0
            t = timing(s)
            assert t["bin_ms"] == 0.0 and t["constraints_ms"] == 0.0 and t["expand_ms"] == 0.0, (name, t)
            assert t["gram_ms"] > 0.0 and t["solve_ms"] > 0.0, (name, t)
        finally:
            s.close()
    # the set-up of test_refit_factors_when_its_iteration_gives_up: the refit expands and factors
    inp = make_inputs(CASES["4d6"])
    s = Session(inp, env={"SPLPAK_SOLVER": "pcg+direct", "SPLPAK_PCG_ALWAYS": "1"})
    try:
        s.plan.enable_kernel_timing()
        _, rc, info_fit = s.fit(second_field(inp))
        assert rc == 0 and info_fit[4] == 0.0 and info_fit[6] == 0.0
        timing(s)
        s.plan.set_option("pcg_tol1", "-1")
        _, rc, info = s.refit(inp["ydata"])
        s.plan.set_option("pcg_tol1", None)
        assert rc == 0 and info[4] > 0.0 and info[6] > 0.0
        t = timing(s)
        assert t["expand_ms"] > 0.0, t
        assert t["bin_ms"] == 0.0 and t["constraints_ms"] == 0.0 and t["gram_ms"] > 0.0 and t["solve_ms"] > 0.0, t
    finally:
        s.close()


def _synth_case(nd, nodes, m, xtrap=1.0):
    x, y, w = synth_points(nd, m)
    return dict(ndim=nd, xdata=np.ascontiguousarray(x), ydata=y, wdata=np.ascontiguousarray(w), xmin=np.zeros(nd), xmax=np.ones(nd),
                nodes=np.array(nodes, dtype=np.int32), xtrap=xtrap)


@pytest.mark.parametrize("what,nodes,m,code", [("two-ended band", [40, 20], 6000, 2),
                                               # 67 x 67 = 4 489 cells: more than the binning's 4 095 bins, so idx comes out of its record path
                                               ("record path of the binning", [70, 70], 20000, 4)])
def test_refit_against_a_fresh_fit(what, nodes, m, code):
    inp = _synth_case(2, nodes, m)
    s = Session(inp)
    try:
        assert s.plan.factorisation()[0] == code
        c_fresh, rc, info_fresh = s.fit(inp["ydata"])
        assert rc == 0
        _, rc, _ = s.fit(second_field(inp))
        assert rc == 0
        c, rc, info = s.refit(inp["ydata"])
        print(f"{what}: refit vs a fresh fit {relmax(c, c_fresh):.2e}; reserr {info[8]:.12e} / {info_fresh[8]:.12e}")
        assert rc == 0 and relmax(c, c_fresh) < PAIR_TOL
        assert info[0] == info_fresh[0] and info[1] == info_fresh[1] and info[6] == 0.0 and info[9] < 1e-9
        assert abs(info[8] - info_fresh[8]) <= 1e-9 * info_fresh[8]
    finally:
        s.close()


def test_refit_on_a_plan_larger_than_the_fit():
    """max_ndata = 3 x ndata: the sorted arrays are addressed with the plan's capacity, the values with the fit's ndata."""
    name = "2d16_zero_w"
    gold = load_golden(name)
    inp = make_inputs(CASES[name])
    s = Session(inp, max_ndata=3 * inp["xdata"].shape[0])
    try:
        assert s.fit(second_field(inp))[1] == 0
        c, rc, info = s.refit(inp["ydata"])
        assert rc == 0 and relmax(c, gold["coef"]) < COEF_TOL and info[9] < 1e-9
    finally:
        s.close()


def test_refit_of_three_fields_with_padded_leading_dimensions():
    """nfields = 3, ldy = ndata + 7, ldcoef = ncol + 5: y, y2 and 2 y - y2.  The padding is untouched, every field is its
    single-field refit bit for bit, and the third is the same combination of the first two (linearity; 3e-10: the bar, three times)."""
    import torch
    name = "3d_aniso"
    inp = make_inputs(CASES[name])
    y, y2 = inp["ydata"], second_field(inp)
    fields = [y, y2, 2.0 * y - y2]
    s = Session(inp)
    try:
        assert s.fit(y2)[1] == 0
        single = []
        for f in fields:
            c, rc, _ = s.refit(f)
            assert rc == 0
            single.append(c)
        n, ncol = s.ndata, s.ncol
        Y = torch.full((3, n + 7), -11.25, dtype=torch.float64, device=s.dev)
        for k, f in enumerate(fields):
            Y[k, :n] = s.t(f)
        Cf = torch.full((3, ncol + 5), 3.5, dtype=torch.float64, device=s.dev)
        rc, info = s.plan.refit(Y[:, :n], Cf[:, :ncol], s.st)
        assert rc == 0 and info.shape == (3, 10)
        Yh, Ch = Y.cpu().numpy(), Cf.cpu().numpy()
        assert np.all(Yh[:, n:] == -11.25) and np.all(Ch[:, ncol:] == 3.5)
        for k in range(3):
            assert np.array_equal(Yh[k, :n], fields[k])
            assert np.array_equal(Ch[k, :ncol], single[k]), k
            assert info[k, 9] < 1e-9 and info[k, 6] == 0.0
        err = relmax(Ch[2, :ncol], 2.0 * Ch[0, :ncol] - Ch[1, :ncol])
        print(f"third field vs 2 c(y) - c(y2): {err:.2e}")
        assert err < 3e-10
    finally:
        s.close()


def test_refit_statuses():
    """Nothing to refit is SPLPAK_E_UNSUPPORTED with the reason named, a bad argument SPLPAK_E_BADARG; after each refused call
    a fit and a refit on the same plan work."""
    import torch
    name = "2d16"
    gold = load_golden(name)
    inp = make_inputs(CASES[name])
    y, y2 = inp["ydata"], second_field(inp)

    def works(s):
        assert s.fit(y2)[1] == 0
        c, rc, _ = s.refit(y)
        assert rc == 0 and relmax(c, gold["coef"]) < COEF_TOL

    s = Session(inp, comm=True)
    try:
        # before any fit
        assert "nothing to refit" in _refused(lambda: s.refit(y), capi.E_UNSUPPORTED)
        works(s)
        # bad arguments
        empty_y = torch.zeros((0, s.ndata), dtype=torch.float64, device=s.dev)
        empty_c = torch.zeros((0, s.ncol), dtype=torch.float64, device=s.dev)
        L, h = s.plan._L, s.plan._h
        c1 = torch.zeros(s.ncol, dtype=torch.float64, device=s.dev)
        yd = s.t(y)
        assert L.splpak_plan_refit_dev(h, 0, yd.data_ptr(), s.ndata, c1.data_ptr(), s.ncol, None, None) == capi.E_BADARG
        _refused(lambda: s.plan.refit(empty_y, empty_c, s.st), capi.E_BADARG)
        _refused(lambda: s.plan.refit(yd[:-1], c1, s.st), capi.E_BADARG)                    # ldy < ndata
        assert L.splpak_plan_refit_dev(h, 1, yd.data_ptr(), s.ndata, c1.data_ptr(), s.ncol - 1, None, None) == capi.E_BADARG
        assert L.splpak_plan_refit_dev(h, 1, None, s.ndata, c1.data_ptr(), s.ncol, None, None) == capi.E_BADARG
        works(s)
        # a splpak_debug_plan_solve since the fit: the factor storage holds another matrix's factor
        N, rhs = s.plan.normal_equations()
        assert s.plan.debug_solve(N, rhs)[1] == 0
        assert "nothing to refit" in _refused(lambda: s.refit(y), capi.E_UNSUPPORTED)
        works(s)
        # an all-reduce hook: the plan is a rank of a sharded fit
        s.plan.set_allreduce(lambda off, count: None, 0, 1)
        assert s.fit(y2)[1] == 0
        assert "sharded" in _refused(lambda: s.refit(y), capi.E_UNSUPPORTED)
        assert L.splpak_plan_set_allreduce_ex(h, capi.ALLREDUCE_FN(), None, 0, 1, 0) == 0
        works(s)
        # after a refit the rows diagnostics describe the last field: its gradient at its coefficients vanishes
        c, rc, info = s.refit(y)
        rho, den, ssq = s.plan.rows_gradient(c, which=1)
        assert np.max(np.abs(rho) / np.where(den > 0.0, den, 1.0)) < 1e-9 and abs(np.sqrt(ssq) - info[8]) <= 1e-12 * info[8]
    finally:
        s.close()


def test_refit_after_a_failed_fit_is_refused():
    """tests/test_pcg.py's singular inputs (xtrap = 0, nodes without data): the fit returns 107 and leaves nothing to refit."""
    rng = np.random.default_rng(3)
    nodes, m = [150], 361
    x = np.concatenate([0.45 * rng.random(m // 2), 0.55 + 0.45 * rng.random(m - m // 2)])[:, None]      # nothing in [0.45, 0.55]
    inp = dict(ndim=1, xdata=x, ydata=np.sin(3.0 * x[:, 0]), wdata=0.5 + rng.random(m), xmin=[0.0], xmax=[1.0], nodes=nodes, xtrap=0.0)
    s = Session(inp, max_ndata=4000)
    try:
        c, rc, _ = s.fit(inp["ydata"])
        assert rc == 107
        assert "nothing to refit" in _refused(lambda: s.refit(inp["ydata"]), capi.E_UNSUPPORTED)
        # the same plan with points everywhere: a fit and a refit
        xg = rng.random((4000, 1))
        wg = 0.5 + rng.random(4000)
        ya, yb = np.sin(3.0 * xg[:, 0]), np.cos(5.0 * xg[:, 0])
        ca, rc, _ = s.fit(ya, x=s.t(xg), w=s.t(wg))
        assert rc == 0
        assert s.fit(yb, x=s.t(xg), w=s.t(wg))[1] == 0
        c, rc, _ = s.refit(ya)
        assert rc == 0 and relmax(c, ca) < PAIR_TOL
    finally:
        s.close()


def _fit_one_shot(inp, y, real32=False):
    f = (lambda a: None if a is None else np.asarray(a, dtype=np.float32)) if real32 else (lambda a: a)
    return capi.fit(inp["ndim"], f(inp["xdata"]), f(y), f(inp["wdata"]), inp["xmin"], inp["xmax"], inp["nodes"], inp["xtrap"], real32=real32)


def test_one_shot_refit_and_its_token():
    name = "2d16"
    gold = load_golden(name)
    inp = make_inputs(CASES[name])
    ncol = int(np.prod(inp["nodes"]))
    _, rc, _, info_fit = _fit_one_shot(inp, second_field(inp))
    assert rc == 0
    tok = capi.fit_token()
    assert tok > 0
    c, rc, info = capi.refit(tok, inp["ydata"], ncol)
    assert rc == 0 and relmax(c, gold["coef"]) < COEF_TOL
    assert info[0] == info_fit[0] and info[1] == info_fit[1] and info[6] == 0.0 and info[9] < 1e-9
    # two fields with a padded coefficient array
    Y = np.stack([second_field(inp), inp["ydata"]])
    c2, rc, info2 = capi.refit(tok, Y, ncol, ldcoef=ncol + 3)
    assert rc == 0 and c2.shape == (2, ncol + 3) and np.array_equal(c2[1, :ncol], c) and np.all(c2[:, ncol:] == 0.0)
    # another ndata, bad arguments
    assert "no longer resident" in _refused(lambda: capi.refit(tok, inp["ydata"][:-1], ncol), capi.E_UNSUPPORTED)
    _refused(lambda: capi.refit(tok, inp["ydata"], ncol, ldcoef=ncol - 1), capi.E_BADARG)
    # a fit of another grid: the old token's fit is no longer resident
    other = make_inputs(CASES["2d8"])
    assert _fit_one_shot(other, other["ydata"])[1] == 0
    tok2 = capi.fit_token()
    assert tok2 > tok
    assert "no longer resident" in _refused(lambda: capi.refit(tok, inp["ydata"], ncol), capi.E_UNSUPPORTED)
    c8, rc, _ = capi.refit(tok2, other["ydata"], 64)
    assert rc == 0 and relmax(c8, load_golden("2d8")["coef"]) < COEF_TOL
    # shutdown releases the cached plan
    capi.shutdown()
    assert "no longer resident" in _refused(lambda: capi.refit(tok2, other["ydata"], 64), capi.E_UNSUPPORTED)


def test_one_shot_refit_real32():
    """REAL32 storage, f64 arithmetic: the refit of the case's values at the tolerance of test_fit_real32_vs_real32_reference."""
    name = "2d8"
    g32, g64 = load_golden(name + "_r32"), load_golden(name)
    inp = make_inputs(CASES[name])
    assert _fit_one_shot(inp, second_field(inp), real32=True)[1] == 0
    c, rc, _ = capi.refit(capi.fit_token(), np.asarray(inp["ydata"], dtype=np.float32), 64, real32=True)
    assert rc == 0 and c.dtype == np.float32
    err_gpu, err_ref = relmax(c, g64["coef"]), relmax(g32["coef"], g64["coef"])
    print(f"{name}: real32 refit error vs real64 golden: GPU {err_gpu:.2e}, REAL32 reference {err_ref:.2e}")
    assert err_gpu <= 1.5 * err_ref + 4 * EPS32
    assert relmax(c, g32["coef"]) <= 2.0 * err_ref + 4 * EPS32
