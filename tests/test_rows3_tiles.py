"""The 3-D rows pass tile by tile (csrc/rows3tile.hip): a workgroup owns a tile of 3 x 3 x 3 cells, its four waves take every fourth
cell in trips of sixteen points, both products of a trip run on the f64 matrix pipe, and a gather adds the <= 8 tile partials of
a node.  3-D plans take this form by default; rows_tiles = 0 (every pass) and residual_cells = 1 (the closing diagnostics pass)
keep the cell-by-cell form of csrc/residual.hip.

The method, the criterion and every bound are those of tests/test_rows_pass.py (_rows_case): splpak_debug_plan_rows_gradient for
which = 0, 1, 2 against the oracle's rows (exact histogram total) at two seeded vectors, at 0 and at the fitted coefficients,
|rho - rho_oracle|_i <= tol den_i with exact zeros where the rows have no term, tol = min(max(NE_TOL, (4^3 + busiest cell) 2^-53),
NE_CEIL), and the sum of squares within (rows + 4^3) 2^-52.

Shapes: the smallest at which the tile form can go wrong -- one cell; cell counts 4 x 5 x 6 (residues 1, 2, 0 modulo the tile
edge, 2 x 2 x 2 tiles); 2 x 9 x 8 cells (one tile in one dimension, three in the others, dimensions reordered by the plan).
Point sets: constructed cell by cell as that file constructs them, with an empty tile, empty cells inside a full tile, a cell
with exactly one trip of points (16), one with one more, cells with several trips, points on the upper boundary of the domain,
zero weights scattered and over one whole cell."""
import functools

import numpy as np
import pytest

from splpak_amd import capi
from tests import test_rows_pass as rp

TILE3 = 3                    # cells along a tile's edge (rows3tile.hip TCS), every dimension
TRIP = 16                    # points per trip of a wave (rows3tile.hip PCHUNK)
GRIDS = {"rows3_one_cell": [4, 4, 4], "rows3_7_8_9": [7, 8, 9], "rows3_5_12_11": [5, 12, 11]}
FULL_TILE = [TRIP, TRIP + 1, 0, 3 * TRIP + 2, 1, 0, 2 * TRIP, 5, TRIP - 1, 0, 70, 9]          # cycled over the cells of the first tile
FORMS = ({}, {"SPLPAK_ROWS_TILES": "0"}, {"SPLPAK_RESIDUAL_CELLS": "1"})


def _counts(nodes):
    """Points per window, dimension 0 fastest: the first tile full with empty cells inside, the tile next to it along dimension 0
    (where there is one) empty, a spread of 0 .. 22 elsewhere."""
    cells = [n - 3 for n in nodes]
    out, k_full = [], 0
    for j2 in range(cells[2]):
        for j1 in range(cells[1]):
            for j0 in range(cells[0]):
                tile = (j0 // TILE3, j1 // TILE3, j2 // TILE3)
                if tile == (0, 0, 0):
                    out.append(FULL_TILE[k_full % len(FULL_TILE)])
                    k_full += 1
                elif tile == (1, 0, 0):
                    out.append(0)
                else:
                    out.append((3 * j0 + 5 * j1 + 7 * j2) % 23)
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    nodes = GRIDS[name]
    counts = [40] if name == "rows3_one_cell" else _counts(nodes)
    inp = rp._cell_points(3, nodes, counts, 71 + sum(nodes))
    rng = np.random.default_rng(5 + sum(nodes))
    # points on the upper boundary of the domain, in one, two and all three dimensions (they belong to the last window)
    edge = np.array([[1.0, 0.3, 0.6], [0.4, 1.0, 1.0], [1.0, 1.0, 1.0], [0.2, 0.7, 1.0], [1.0, 1.0, 0.1]])
    x = np.vstack([inp["xdata"], edge])
    y = np.concatenate([inp["ydata"], np.cos(3.0 * edge.sum(axis=1)) + 0.25])
    w = np.concatenate([inp["wdata"], 0.5 + rng.random(edge.shape[0])])
    # zero weights: one point in ten, and every point of the window that holds (0.5, 0.5, 0.5)
    w[rng.random(w.size) < 0.1] = 0.0
    dx = 1.0 / (np.asarray(nodes) - 1)
    win = np.clip(np.floor(x / dx).astype(np.int64) - 1, 0, np.asarray(nodes) - 4)
    mid = np.clip(np.floor(0.5 / dx).astype(np.int64) - 1, 0, np.asarray(nodes) - 4)
    if name != "rows3_one_cell":
        w[np.all(win == mid, axis=1)] = 0.0
    return dict(inp, xdata=np.ascontiguousarray(x), ydata=y, wdata=w)


def _inputs(name):
    return _case(name) if name in GRIDS else _ORIGINAL_INPUTS(name)


_ORIGINAL_INPUTS = rp._inputs


def test_point_sets_hold_what_they_are_built_for():
    for name, nodes in GRIDS.items():
        inp = _case(name)
        assert 1000 * (name != "rows3_one_cell") <= inp["xdata"].shape[0] <= 6000
        assert np.any(inp["wdata"] == 0.0) and np.any(np.all(inp["xdata"] == 1.0, axis=1))
    order = rp._internal_order(GRIDS["rows3_7_8_9"])
    assert [(GRIDS["rows3_7_8_9"][d] - 3) % TILE3 for d in order] == [1, 2, 0]
    cells = [GRIDS["rows3_5_12_11"][d] - 3 for d in rp._internal_order(GRIDS["rows3_5_12_11"])]
    assert [-(-c // TILE3) for c in cells] == [1, 3, 3]
    assert all(n - 3 == 1 for n in GRIDS["rows3_one_cell"])
    nodes = GRIDS["rows3_7_8_9"]
    cnt = np.asarray(_counts(nodes)).reshape([n - 3 for n in nodes][::-1])          # [j2][j1][j0]
    first, beside = cnt[:TILE3, :TILE3, :TILE3], cnt[:TILE3, :TILE3, TILE3:2 * TILE3]
    assert beside.size > 0 and not beside.any()                                    # an empty tile
    assert {TRIP, TRIP + 1, 0} <= set(first.ravel().tolist()) and first.max() > 4 * TRIP      # one trip, one more, several; empty cells inside
    # the constructed windows hold those counts: exactly in the first two tiles, the five boundary points on top elsewhere
    got = rp._window_counts(_case("rows3_7_8_9")).reshape(cnt.shape)
    assert np.array_equal(got[:TILE3, :TILE3, :2 * TILE3], cnt[:TILE3, :TILE3, :2 * TILE3])
    assert np.all(got >= cnt) and got.sum() == cnt.sum() + 5


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRIDS))
def test_rows3_forms_match_oracle(port, name, monkeypatch):
    """The tile form (default) and the two switches back to the cell-by-cell form, each against the oracle by _rows_case's rules."""
    monkeypatch.setattr(rp, "_inputs", _inputs)
    rp._rows_case(port, name, monkeypatch, rp.SOLVERS_4D[:1], forms=FORMS)


@pytest.mark.gpu
def test_rows3_bits_do_not_depend_on_what_else_runs(monkeypatch):
    """Two passes at the same vector, one on an idle device and one behind and beside other work (matrix products queued on the
    stream the pass runs on, and on a second stream): identical bits, for every form of the pass -- no floating-point atomics."""
    import torch
    inp = _case("rows3_7_8_9")
    c = np.random.default_rng(9).uniform(-1.0, 1.0, int(np.prod(inp["nodes"])))
    plan, ierr, info, coef = rp._fit_plan(inp, {"SPLPAK_SOLVER": "direct"}, monkeypatch)
    try:
        assert ierr == 0
        torch.cuda.synchronize()
        idle = [plan.rows_gradient(c, which) for which in (0, 1, 2)]
        a = torch.rand(4096, 4096, dtype=torch.float64, device="cuda")
        side = torch.cuda.Stream()
        for which in (0, 1, 2):
            with torch.cuda.stream(side):
                for _ in range(4):
                    a @ a
            for _ in range(2):
                a @ a
            rho, den, ssq = plan.rows_gradient(c, which)
            assert np.array_equal(rho, idle[which][0]) and np.array_equal(den, idle[which][1]) and ssq == idle[which][2], which
        torch.cuda.synchronize()
    finally:
        plan.close()
