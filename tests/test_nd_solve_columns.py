"""The tree solves read a block's REAL columns only (csrc/ndjobs.hip solve_block_cols; csrc/ndkernels.hip nd_fwd_kernel,
nd_dot_kernel and their _many forms).

A front's own width w is padded to a multiple of 256 with identity columns: zero below a unit diagonal, against vector entries
that are exactly zero.  The forward sweep's column groups and the backward sweep's waves that hold padding alone load nothing
and contribute +0.0 / store 0.0.  Every product left out was an exact zero added to a sum that began at +0.0, so the contract is
EQUAL BITS with the form that reads all 256 columns, which the switch nd_solve_padded keeps (SPLPAK_ND_SOLVE_PADDED).

CPU tier: the grids named here hold the widths the guard can go wrong at (found with capi.debug_nd_fronts).
GPU tier: splpak_debug_plan_solve of a synthetic SPD matrix, two right-hand sides one after the other on the same plan (stale
partial sums of the first would show in the second), and a batched refit of three fields (the _many kernels)."""
import numpy as np
import pytest

from splpak_amd import capi
from tests.cases import CASES, make_inputs
from tests.test_normal_equations import _plan, stencil_matvec, synthetic_spd
from tests.test_refit import Session, _synth_case, second_field
from tests.test_refit_batch import fields_of, refit_padded

PADDED = "SPLPAK_ND_SOLVE_PADDED"

# grid -> (w mod 256 of a front WITH rows below its own block (h > 0), what that is)
GRIDS = {
    (19, 19, 20): (1, "a last block with one real column (w = 513)"),
    (9, 17, 13): (105, "real columns that are no multiple of 16 (w = 105, 189)"),
    (4, 8, 8): (16, "exactly one column group (w = 16)"),
    (16, 16, 34): (0, "no padding at all (w = 768)"),
    (16, 16, 16): (32, "the golden 3d16: two blocks, 32 real columns in the second (w = 288)"),
}


def _widths(nodes):
    t = capi.debug_nd_fronts(list(nodes))
    return [int(w) for w, h in zip(t["w"], t["h"]) if h > 0]


def test_grids_hold_the_widths_they_are_named_for():
    for nodes, (rem, what) in GRIDS.items():
        ws = _widths(nodes)
        assert any(w % 256 == rem for w in ws), (nodes, what, sorted(set(ws)))
    assert any(w % 16 != 0 for w in _widths((9, 17, 13)))
    assert 513 in _widths((19, 19, 20)) and 768 in _widths((16, 16, 34)) and 16 in _widths((4, 8, 8))
    assert tuple(CASES["3d16"]["nodes"]) == (16, 16, 16) and 288 in _widths((16, 16, 16))


def _nd_plan(nodes, padded, monkeypatch):
    monkeypatch.setenv("SPLPAK_SOLVER", "direct")
    monkeypatch.setenv("SPLPAK_ND", "1")
    if padded:
        monkeypatch.setenv(PADDED, "1")
    try:
        plan = _plan(list(nodes))
    finally:
        monkeypatch.delenv("SPLPAK_ND")
        monkeypatch.delenv(PADDED, raising=False)
    assert plan.factorisation()[0] == 4, (nodes, plan.factorisation())
    assert plan.get_option("nd_solve_padded") == ("1" if padded else None)
    return plan


@pytest.mark.gpu
@pytest.mark.parametrize("nodes", list(GRIDS), ids=["x".join(map(str, n)) for n in GRIDS])
def test_real_columns_give_the_bits_of_all_columns(nodes, monkeypatch):
    N = synthetic_spd(list(nodes), seed=4242 + int(np.prod(nodes)))
    rng = np.random.default_rng(17)
    xs = [rng.uniform(-1.0, 1.0, N.shape[0]), rng.standard_normal(N.shape[0]) * 1e3]
    bs = [np.asarray(stencil_matvec(N, list(nodes), x), dtype=np.float64) for x in xs]
    got = {}
    for padded in (False, True):
        plan = _nd_plan(nodes, padded, monkeypatch)
        try:
            out = []
            for b in bs:                      # one after the other on the same plan
                x, rc, mp = plan.debug_solve(N, b)
                assert rc == 0 and mp > 0
                out.append(x)
            again, rc, _ = plan.debug_solve(N, bs[0])         # and the first once more, after the second
            assert rc == 0 and np.array_equal(again, out[0])
        finally:
            plan.close()
        got[padded] = out
    for k, x_true in enumerate(xs):
        err = float(np.max(np.abs(got[False][k] - x_true)) / np.max(np.abs(x_true)))
        print(f"{nodes} right-hand side {k}: forward error {err:.2e}")
        assert err <= 1e-12
        assert np.array_equal(got[False][k], got[True][k]), (nodes, k)


def _refit_inputs(name):
    return make_inputs(CASES["3d16"]) if name == "3d16" else _synth_case(3, [19, 19, 20], 20000)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["3d16", "3d19x19x20"])
def test_batched_refit_of_three_fields_gives_the_same_bits(name):
    inp = _refit_inputs(name)
    F = fields_of(inp, 3, zero=None)
    got = {}
    for padded in (False, True):
        s = Session(inp, env={"SPLPAK_ND": "1", "SPLPAK_SOLVER": "direct", **({PADDED: "1"} if padded else {})})
        try:
            assert s.plan.factorisation()[0] == 4
            c0, rc, info0 = s.fit(second_field(inp))
            assert rc == 0 and info0[4] != 0.0
            rc, c, info, st = refit_padded(s, F, 8)
            assert rc == 0 and st[0] == 2, st           # one sweep for the three fields: the _many kernels
            rc1, c1, _, _ = refit_padded(s, F, 1)
            assert rc1 == 0 and np.array_equal(c, c1)   # and the single kernels on the same factor
            got[padded] = (c0, c, info[:, [0, 1, 2, 3, 4, 8, 9]])
        finally:
            s.close()
    for a, b in zip(got[False], got[True]):
        assert np.array_equal(a, b), name
