"""Refit of several fields in lock-step on a held nested-dissection factor (splpak_plan_refit_dev with nfields >= 2; planfit.hip
refit_chunk_batched, ndchol.hip nd_solve_many, ndkernels.hip nd_*_many_kernel).

The fields of a chunk (option refit_batch, 1 .. 8, default 8) share every sweep of the factor.  The contract is equality with the
field-by-field refit -- refit_batch = 1 on the same plan --, bit for bit: coefficients, info[0..4], [8], [9], the padding of ydata
and coef untouched.  What else is checked: the counters of splpak_debug_plan_refit_stats, the calls that stay field by field, a
failing field (its chunk is run again by the field-by-field loop), the plan's state after a batch, and the one-shot entries.
Grids: the smallest that take nested dissection -- 3d16 (4 096 columns), 2-D 70 x 70 (fronts that are no multiples of 256, the
binning's record path), 4-D 12^4 (20 736 columns, the tiled row operator).
"""
import numpy as np
import pytest

from splpak_amd import capi
from tests.cases import CASES, make_inputs
from tests.test_refit import Session, _refused, _synth_case, second_field

pytestmark = pytest.mark.gpu

INFO_EQUAL = [0, 1, 2, 3, 4, 8, 9]          # what a batched refit promises bit for bit ([7] is a time, [5] [6] are 0)
PAD_Y, PAD_C = -11.25, 3.5
TIGHT_TOL = 1e-17

ND_GRIDS = {
    "3d16": lambda: make_inputs(CASES["3d16"]),
    "2d70": lambda: _synth_case(2, [70, 70], 20000),
    "4d12": lambda: _synth_case(4, [12, 12, 12, 12], 60000),
}


def fields_of(inp, nfields, zero=1):
    """Field k = cos((3 + k) sum_d x_d) at the points; field `zero` is identically zero (it converges after one step)."""
    sx = inp["xdata"].sum(axis=1)
    F = np.stack([np.cos((3.0 + k) * sx) for k in range(nfields)])
    if zero is not None and zero < nfields:
        F[zero] = 0.0
    return F


@pytest.fixture(scope="module")
def sessions():
    """One plan per grid, fitted once (a refit needs a fit), shared by the tests that only refit."""
    made = {}

    def get(name):
        if name not in made:
            inp = ND_GRIDS[name]()
            s = Session(inp)
            assert s.plan.factorisation()[0] == 4, s.plan.factorisation()
            _, rc, info = s.fit(second_field(inp))
            assert rc == 0 and info[4] != 0.0          # a factorisation ran: refits hold its factor
            made[name] = s
        return made[name]

    yield get
    for s in made.values():
        s.close()


def refit_padded(s, F, batch):
    """One refit call of the fields F under refit_batch = `batch`, with padded leading dimensions -> (rc, coef (nfields, ncol),
    info, stats); asserts that the padding and the values are untouched."""
    import torch
    nf, n, ncol = F.shape[0], s.ndata, s.ncol
    Y = torch.full((nf, n + 7), PAD_Y, dtype=torch.float64, device=s.dev)
    Y[:, :n] = s.t(F)
    Cf = torch.full((nf, ncol + 5), PAD_C, dtype=torch.float64, device=s.dev)
    s.plan.set_option("refit_batch", str(batch))
    try:
        rc, info = s.plan.refit(Y[:, :n], Cf[:, :ncol], s.st)
    finally:
        s.plan.set_option("refit_batch", None)
    Yh, Ch = Y.cpu().numpy(), Cf.cpu().numpy()
    assert np.all(Yh[:, n:] == PAD_Y) and np.all(Ch[:, ncol:] == PAD_C)
    assert np.array_equal(Yh[:, :n], F, equal_nan=True)
    return rc, Ch[:, :ncol].copy(), info.copy(), s.plan.refit_stats()


def chunks_of(nfields, batch):
    return [range(k, min(k + batch, nfields)) for k in range(0, nfields, batch)]


@pytest.mark.parametrize("nfields", [2, 3, 8, 11])
@pytest.mark.parametrize("grid", sorted(ND_GRIDS))
def test_batched_refit_equals_field_by_field(sessions, grid, nfields):
    """refit_batch = 8 (11 fields: chunks of 8 + 3) and 3 (3, 3, 3, 2) against refit_batch = 1 on the same plan: equal bits, and
    the counters: one sweep per chunk for the first solve and one per refinement step of its slowest field, each carrying the
    fields still refining.  The zero field's first correction is 0: it leaves the sweeps after one step.  On 3d16 every other
    field meets the default tolerance (1e-11) with its first correction as well, so nothing would drop out of a sweep there: that
    grid refines to TIGHT_TOL, which only an exact zero meets at once (the others end by the estimate or at the rounding floor)."""
    s = sessions(grid)
    F = fields_of(s.inp, nfields)
    if grid == "3d16":
        s.plan.set_refine(4, TIGHT_TOL)
    try:
        _batched_against_field_by_field(s, grid, nfields, F)
    finally:
        s.plan.set_refine(4, 1e-11)          # (the plan's defaults, csrc/plan.hpp)


def _batched_against_field_by_field(s, grid, nfields, F):
    rc1, c1, info1, st1 = refit_padded(s, F, 1)
    assert rc1 == 0
    assert st1[0] == 1 and st1[1] == st1[2] and st1[3] == 0
    assert st1[2] == int(np.sum(1 + info1[:, 2]))
    print(f"{grid} x {nfields}: refinement steps per field {info1[:, 2].astype(int).tolist()}")
    assert len(set(info1[:, 2])) > 1, "the zero field should leave the sweeps before the others"
    assert info1[1, 2] == 1 and np.all(c1[1] == 0.0)
    for batch in (8, 3):
        rc, c, info, st = refit_padded(s, F, batch)
        assert rc == 0
        for k in range(nfields):
            assert np.array_equal(c[k], c1[k]), (grid, nfields, batch, k)
        assert np.array_equal(info[:, INFO_EQUAL], info1[:, INFO_EQUAL]), (grid, nfields, batch)
        assert np.all(info[:, 6] == 0.0) and np.all(info[:, 5] == 0.0)
        assert st[0] == 2 and st[3] == 0
        assert st[2] == int(np.sum(1 + info[:, 2]))
        assert st[1] == sum(1 + int(max(info[k, 2] for k in ch)) for ch in chunks_of(nfields, batch)), (st, info[:, 2])
        assert st[1] < st1[1]


def test_refit_batch_option_on_a_plan():
    """A process default set under either name is what a plan created afterwards reads back; the option does not shape storage, so
    a plan takes it per call as well."""
    for name in ("refit_batch", "SPLPAK_REFIT_BATCH"):
        capi.set_default_option(name, "4")
        try:
            plan = capi.Plan(2, [8, 8], [0.0, 0.0], [1.0, 1.0], 1.0, 100)
        finally:
            capi.set_default_option(name, None)
        try:
            assert plan.get_option("refit_batch") == "4"
            plan.set_option("refit_batch", "99")
            assert plan.get_option("SPLPAK_REFIT_BATCH") == "99"
            plan.set_option("refit_batch", None)
            assert plan.get_option("refit_batch") is None
        finally:
            plan.close()


def test_single_field_band_iteration_and_hook_stay_field_by_field(sessions):
    """Route 1, and the results of today's loop: one field on a nested-dissection plan; three fields on the band plan 2d16; a fit
    the iteration answered (4d6, SPLPAK_SOLVER=pcg); a plan with an all-reduce hook refuses as before."""
    s = sessions("3d16")
    F = fields_of(s.inp, 3, zero=None)
    c, rc, _ = s.refit(F[0])
    assert rc == 0 and s.plan.refit_stats()[0] == 1
    assert np.array_equal(c, refit_padded(s, F[:1], 8)[1][0]) and s.plan.refit_stats()[0] == 1

    for name, env in (("2d16", None), ("4d6", {"SPLPAK_SOLVER": "pcg"})):
        inp = make_inputs(CASES[name])
        t = Session(inp, env=env, comm=(name == "2d16"))
        try:
            assert t.plan.refit_stats() == [0, 0, 0, 0]
            _, rc, info_fit = t.fit(second_field(inp))
            if name == "4d6":
                assert t.plan.factorisation()[0] == 6
                assert rc in (0, 107)              # (as tests/test_refit.py accepts for the iteration alone)
                if rc == 107:
                    _refused(lambda: t.refit(F[0][:t.ndata]), capi.E_UNSUPPORTED)
                    continue
            else:
                assert rc == 0 and t.plan.factorisation()[0] != 4
            G = fields_of(inp, 3, zero=None)
            single = [t.refit(f) for f in G]
            rcb, cb, infob, stb = refit_padded(t, G, 8)
            assert stb[0] == 1 and stb[3] == 0, stb
            assert rcb == next((r for _, r, _ in single if r != 0), 0)      # (the first failing field ends the call)
            if rcb == 0:
                for k in range(3):
                    assert np.array_equal(cb[k], single[k][0]), (name, k)
                    assert np.array_equal(infob[k, INFO_EQUAL], single[k][2][INFO_EQUAL]), (name, k)
            if name == "2d16":
                assert rcb == 0
                assert stb[1] == stb[2] == int(np.sum(1 + infob[:, 2]))
                t.plan.set_allreduce(lambda off, count: None, 0, 1)
                assert t.fit(second_field(inp))[1] == 0
                assert "sharded" in _refused(lambda: refit_padded(t, G, 8), capi.E_UNSUPPORTED)
        finally:
            t.close()


def test_a_failing_field_sends_its_chunk_to_the_field_by_field_loop(sessions):
    """Three fields, the middle one holding a NaN (ordinary data): 107 with the outputs of the field-by-field call -- field 0 its
    single-field refit, the last field zeroed --, the three fields counted as run again, and the plan still refits."""
    s = sessions("3d16")
    F = fields_of(s.inp, 3, zero=None)
    c0, rc, _ = s.refit(F[0])
    assert rc == 0
    F[1, s.ndata // 2] = np.nan
    rc1, c1, info1, _ = refit_padded(s, F, 1)
    rc8, c8, info8, st8 = refit_padded(s, F, 8)
    assert rc1 == 107 and rc8 == 107
    assert np.array_equal(c8[0], c0)
    assert np.array_equal(c8, c1, equal_nan=True) and np.all(c8[2] == 0.0)
    assert np.array_equal(info8[:, INFO_EQUAL], info1[:, INFO_EQUAL], equal_nan=True)
    assert st8[0] == 2 and st8[3] == 3, st8
    good = fields_of(s.inp, 2, zero=None)
    rc, c, _, st = refit_padded(s, good, 8)
    assert rc == 0 and st[0] == 2 and st[3] == 0 and np.array_equal(c[0], c0)


def test_plan_state_after_a_batched_refit():
    """After a batched refit the plan describes the LAST field (rows gradient, reserr, normal equations), a single-field refit and
    a fresh fit give the bits they gave before, and the per-field copies are allocated once and counted."""
    inp = make_inputs(CASES["3d16"])
    s = Session(inp)
    try:
        y2 = second_field(inp)
        c_fit, rc, _ = s.fit(y2)
        assert rc == 0
        F = fields_of(inp, 4, zero=None)
        c_single, rc, _ = s.refit(F[0])
        assert rc == 0
        before = s.plan.device_bytes()
        rc, c, info, st = refit_padded(s, F, 8)
        assert rc == 0 and st[0] == 2
        after = s.plan.device_bytes()
        # 8 copies each of: the values (max_ndata), xvec / rhs / rho (>= ncol each), and V and Y of the tree solve (>= ncol each:
        # every variable has a row in its front's vector)
        assert after - before >= 8 * 8 * (s.ndata + 5 * s.ncol), (before, after)
        last = c[-1]
        rho, den, ssq = s.plan.rows_gradient(last, which=1)
        assert np.max(np.abs(rho) / np.where(den > 0.0, den, 1.0)) < 1e-9
        assert abs(np.sqrt(ssq) - info[-1, 8]) <= 1e-12 * info[-1, 8]
        N, rhs = s.plan.normal_equations()
        assert np.all(np.isfinite(N)) and np.all(np.isfinite(rhs)) and np.any(rhs != 0.0)
        s.plan.enable_kernel_timing()
        rc, c_again, _, _ = refit_padded(s, F, 8)
        t = s.plan.stage_timing()
        s.plan.enable_kernel_timing(False)
        assert rc == 0 and np.array_equal(c_again, c) and s.plan.device_bytes() == after
        # (signs and zeros only, never durations) the last field's gather + right-hand side, the first sweep, a residual pass
        assert t["bin_ms"] == 0.0 and t["constraints_ms"] == 0.0 and t["expand_ms"] == 0.0, t
        assert t["gram_ms"] > 0.0 and t["solve_ms"] > 0.0 and t["residual_pass_ms"] > 0.0, t
        c_single2, rc, _ = s.refit(F[0])
        assert rc == 0 and np.array_equal(c_single2, c_single) and np.array_equal(c_single2, c[0])
        c_fit2, rc, _ = s.fit(y2)
        assert rc == 0 and np.array_equal(c_fit2, c_fit)
    finally:
        s.close()


@pytest.mark.parametrize("real32", [False, True])
def test_one_shot_refit_of_four_fields(real32):
    """splpak_refit_f64 / _f32 with 4 fields on 3d16: the bits of the same fit + refit under a process default refit_batch = 1.
    (A batched chunk reports ONE time share for all its fields in info[7]; field by field every field has its own.)"""
    inp = make_inputs(CASES["3d16"])
    ncol = int(np.prod(inp["nodes"]))
    f = (lambda a: None if a is None else np.asarray(a, dtype=np.float32)) if real32 else (lambda a: a)
    F = fields_of(inp, 4, zero=None)

    def run():
        _, rc, _, _ = capi.fit(inp["ndim"], f(inp["xdata"]), f(second_field(inp)), f(inp["wdata"]), inp["xmin"], inp["xmax"], inp["nodes"],
                               inp["xtrap"], real32=real32)
        assert rc == 0
        return capi.refit(capi.fit_token(), f(F), ncol, real32=real32, ldcoef=ncol + 3)

    capi.shutdown()
    try:
        c8, rc8, info8 = run()
        capi.shutdown()
        capi.set_default_option("refit_batch", "1")
        c1, rc1, info1 = run()
    finally:
        capi.set_default_option("refit_batch", None)
        capi.shutdown()
    assert rc8 == 0 and rc1 == 0
    assert np.array_equal(c8, c1) and np.all(c8[:, ncol:] == 0.0)
    assert np.array_equal(info8[:, INFO_EQUAL], info1[:, INFO_EQUAL])
    assert len(set(info8[:, 7])) == 1 and len(set(info1[:, 7])) == 4
