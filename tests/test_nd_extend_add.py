"""The extend-add fused into a front's last Schur pass (csrc/ndkernels.hip, nd_syrk_kernel, the `SCHUR && j.pm` block): the
finished tile is added into the parent through the child -> parent map, the parent's entries fetched a batch at a time.

The yardstick is the same fit with SPLPAK_ND_NO_FUSE=1: the Schur complement is then stored and added by separate launches of
nd_extend_add_kernel, a kernel that shares no code with the block.  Every parent entry receives the same summands in the same
order either way, so the two fits agree bit for bit -- under square and packed destinations, the postorder schedule, K = 256
passes and without stream overlap.  The grids are the smallest whose fronts reach every branch of the block:

  3-D 20 x 14 x 17   odd extents: no front's height is a multiple of 64 (padding rows and columns with target -1), tiles straddle
                     the boundary between the parent's panel and its Schur buffer, diagonal items
  3-D 16 x 16 x 16   launches of few items: the instantiations where four / sixteen waves share an item
  2-D 48 x 37        fronts of a single block step, leaves whose Schur buffer is never materialised
  4-D 9 x 8 x 10 x 8 wide borders (1 920 rows), packed buffers; its host oracle is the slowest part of this file (seconds)

All four are accepted for nested dissection as they stand.  Against the host oracle (the banded CPU solve of the reference's
rows) the bar is the 1e-10 of tests/test_nd.py."""
import os

import numpy as np
import pytest

from splpak_amd import capi
from tests.conftest import relmax

COEF_TOL = 1e-10                                 # tests/test_nd.py

GRIDS = {"3d_odd": ([20, 14, 17], 60000), "3d16": ([16, 16, 16], 40000), "2d": ([48, 37], 50000), "4d": ([9, 8, 10, 8], 80000)}
VARIANTS = {"default": {}, "square": {"SPLPAK_ND_SQUARE": "1"}, "cut2": {"SPLPAK_ND_CUT": "2"}, "kb1": {"SPLPAK_ND_KB": "1"},
            "serial": {"SPLPAK_NO_LOOKAHEAD": "1"}}

_inputs, _fits, _oracle = {}, {}, {}


@pytest.fixture(autouse=True)
def _factorisation_only(monkeypatch):
    monkeypatch.setenv("SPLPAK_SOLVER", "direct")
    monkeypatch.setenv("SPLPAK_ND", "1")


def _inp(grid):
    if grid not in _inputs:
        from splpak_amd.synth import synth_points
        nodes, m = GRIDS[grid]
        nd = len(nodes)
        x, y, w = synth_points(nd, m)
        _inputs[grid] = dict(ndim=nd, xdata=x, ydata=y, wdata=w, xmin=[0.0] * nd, xmax=[1.0] * nd, nodes=nodes, xtrap=1.0)
    return _inputs[grid]


def _setenv(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    return old


def _restore(old):
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _fit(grid, variant, fused):
    """(coef, ierror, info) of one fit, computed once per (grid, variant, fused / separate extend-add)"""
    key = (grid, variant, fused)
    if key not in _fits:
        inp = _inp(grid)
        old = _setenv(dict(VARIANTS[variant], **({} if fused else {"SPLPAK_ND_NO_FUSE": "1"})))
        try:
            c, e, _, info = capi.fit(inp["ndim"], inp["xdata"], inp["ydata"], inp["wdata"], inp["xmin"], inp["xmax"], inp["nodes"],
                                     inp["xtrap"], want_hist=False)
        finally:
            _restore(old)
        c.setflags(write=False)
        _fits[key] = (c, e, info)
    return _fits[key]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_fused_extend_add_equals_separate_launches_bitwise(grid, variant):
    c, e, info = _fit(grid, variant, True)
    c0, e0, info0 = _fit(grid, variant, False)
    assert e == 0 and e0 == 0
    print(f"{grid} {variant}: optimality {info[9]:.1e}, refine steps {info[2]:.0f} (separate launches: {info0[2]:.0f}), "
          f"{'same bits' if np.array_equal(c, c0) else f'{relmax(c, c0):.1e} apart'}")
    assert np.array_equal(c, c0)
    assert info[9] < 1e-9
    assert info[2] == info0[2]


@pytest.mark.gpu
@pytest.mark.parametrize("grid", list(GRIDS))
def test_two_fits_on_one_plan_give_the_same_bits(grid):
    """The second fit starts from the arena as the first left it: the parents must be cleared again before the children add."""
    import torch
    inp = _inp(grid)
    dev = torch.device("cuda", 0)
    x, y, w = (torch.tensor(inp[k], dtype=torch.float64, device=dev) for k in ("xdata", "ydata", "wdata"))
    plan = capi.Plan(inp["ndim"], inp["nodes"], inp["xmin"], inp["xmax"], inp["xtrap"], x.shape[0])
    try:
        assert plan.factorisation()[0] == 4
        out = []
        for _ in range(2):
            coef = torch.zeros(plan.ncol, dtype=torch.float64, device=dev)
            ierr, info = plan.fit(x, y, w, coef)
            torch.cuda.synchronize()
            assert ierr == 0 and info[9] < 1e-9
            out.append(coef.cpu().numpy())
    finally:
        plan.close()
    assert np.array_equal(out[0], out[1])


@pytest.mark.gpu
@pytest.mark.parametrize("grid", list(GRIDS))
def test_fused_extend_add_matches_the_host_oracle(port, grid):
    inp = _inp(grid)
    if grid not in _oracle:
        _oracle[grid] = port.fit_banded(inp["ndim"], inp["xdata"], inp["ydata"], inp["wdata"], inp["xmin"], inp["xmax"], inp["nodes"],
                                        inp["xtrap"])
    c0, e0, i0 = _oracle[grid]
    c, e, info = _fit(grid, "default", True)
    assert e == 0 and e0 == 0
    print(f"{grid}: against the banded CPU solve {relmax(c, c0):.2e}; rows {info[0]:.0f}+{info[1]:.0f}")
    assert relmax(c, c0) < COEF_TOL
    assert info[0] == i0[0] and info[1] == i0[1]
