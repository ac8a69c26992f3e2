"""The binning of the points by window (csrc/binpoints.hip) on its own, at the grid sizes that switch its form.

launch_bin_points picks its kernels from the grid's number of cells: the stable partition in one level (up to 4 095 cells), in two
levels with tiles of up to 256 cells (sp_bin2_kernel<D, 256>, up to 1 048 320 cells) or of up to 4 095 cells
(sp_bin2_kernel<D, SP_NB>, up to 4 095^2 cells), and beyond that the atomic route (keys, a two-launch scan over 256 segments, a
scatter and a re-sort of every cell).  The fits of the rest of the suite stop at 707 281 cells and only see the consequences of
the sorted order.  Here splpak_debug_bin_points runs the binning alone -- no plan, no factor storage -- and returns everything raw
in the library's internal numbering; every array is held against plain numpy with array_equal, no tolerance.

Every grid has xmin = 0 and xmax = nodes - 1 per dimension, so dx = dxin = 1 and t = x exactly: the reference key
    it = trunc(x) saturated at +-2e9,  ws = clip(it - 1, 0, nodes - 4),  key = sum_d ws[perm[d]] * cellstride[d]
is exact for every representable x (on nodes, in (-1, 0), beyond +-2e9); a point of zero weight has key = ncell and is not placed.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from splpak_amd import capi
from tests.conftest import ROOT

SP_NB, SP_Q, SP_STAGE = 4096, 8192, 2816          # binpoints.hip: bins of a level, records per sub-block, records a tile stages in LDS

# name -> (nodes, route, cpt, weights, columns of padding in xdata).  route / cpt: what launch_bin_points must take on that grid --
# asserted, so that a later change of a threshold cannot quietly turn a case into a test of something else.
CASES = {
    "1d_one_level_limit": ([4098], 1, 1, "tenth", 0),                 # 4 095 cells
    "1d_two_levels_smallest": ([4099], 2, 2, None, 2),
    "2d_two_levels_smallest": ([90, 80], 2, 2, "tenth", 0),
    "1d_tiles256_limit": ([1048323], 2, 256, "tenth", 2),             # 1 048 320 = 4 095 * 256 cells
    "1d_tiles_nb_smallest": ([1048324], 3, 257, "tenth", 0),
    "2d_tiles_nb": ([1030, 1025], 3, 257, "positive", 2),
    "3d_tiles_nb": ([105, 104, 105], 3, 257, "tenth", 0),
    "4d_tiles_nb": ([35, 36, 35, 35], 3, 265, None, 0),
    "1d_tiles_nb_limit": ([16769028], 3, 4095, "tenth", 0),           # 4 095^2 cells
    "1d_atomic_fallback": ([16769030], 0, 0, "tenth", 0),
}
ATOMIC_CASES = ["1d_two_levels_smallest", "3d_tiles_nb"]              # once more under SPLPAK_BIN_ATOMIC=1, in a child process


def _grid(nodes):
    """(perm, cells, cellstride, ncell) as build_grid orders the dimensions: ascending node counts, stable."""
    nodes = np.asarray(nodes, dtype=np.int64)
    perm = np.argsort(nodes, kind="stable")
    cells = nodes[perm] - 3
    stride = np.concatenate([[1], np.cumprod(cells)[:-1]])
    return perm, cells, stride, int(np.prod(cells))


def reference_keys(nodes, x, w, perm, cellstride):
    nodes = np.asarray(nodes, dtype=np.int64)
    nd = nodes.size
    it = np.trunc(np.clip(x[:, :nd], -2.0e9, 2.0e9)).astype(np.int64)
    ws = np.clip(it - 1, 0, nodes - 4)
    key = np.zeros(x.shape[0], dtype=np.int64)
    for d in range(nd):
        key += ws[:, int(perm[d])] * int(cellstride[d])
    if w is not None:
        key[w == 0] = int(np.prod(nodes - 3))
    return key


def _points_of_cells(nodes, cell, rng):
    """One point inside every listed cell (internal linear index), caller's dimension order; every seventh one on a node."""
    perm, cells, stride, _ = _grid(nodes)
    nd = len(nodes)
    u = rng.random((cell.size, nd))
    u[::7] = 0.0
    x = np.zeros((cell.size, nd))
    for d in range(nd):
        x[:, perm[d]] = (cell // stride[d]) % cells[d] + 1.0 + u[:, d]
    return x


def _special_points(nodes):
    """Points of the clamped cells at both ends, outside the grid, beyond the saturation of the index and at +-1e300; every
    coordinate comes from the same list, so they all fall into corner cells."""
    nodes = np.asarray(nodes, dtype=np.float64)
    rel_lo = [-1.0e300, -2.5e9, -2.0e9, -5.5, -1.0, -0.5, 0.0, 0.25, 1.0, 1.75, 2.0, 2.5]                 # window starts 0 and 1
    rel_hi = [-4.0, -3.5, -3.0, -2.25, -2.0, -1.0, -0.5, 0.0, 0.5, 7.25, 2.0e9, 2.5e9, 1.0e300]          # relative to nodes - 1
    rows = []
    for j, v in enumerate(rel_lo):
        rows.append([v if (j + d) % 2 == 0 else (nodes[d] - 1) + rel_hi[(j + d) % len(rel_hi)] for d in range(nodes.size)])
    for j, v in enumerate(rel_hi):
        rows.append([(nodes[d] - 1) + v if (j + d) % 2 == 0 else rel_lo[(j + d) % len(rel_lo)] for d in range(nodes.size)])
    return np.array(rows)


def build_case(name):
    """-> (nodes, x, y, w, route, cpt, wanted): the points come from a wanted population per tile of max(cpt, 1) cells -- a
    background of ~150 000 points on random cells, reserved tiles with exact record counts -- in a seeded random order."""
    nodes, route, cpt, weights, pad = CASES[name]
    rng = np.random.default_rng(sum(nodes) + 7 * len(nodes))
    perm, cells, stride, ncell = _grid(nodes)
    ts = max(cpt, 1)
    ntile = (ncell + ts - 1) // ts
    special = _special_points(nodes)
    corner = set((reference_keys(nodes, special, None, perm, stride) // ts).tolist())
    # reserved tiles, away from the corner cells and from the short last tile: (records, where)
    plan = [(0, "empty"), (300, "last"), (SP_STAGE, "spread"), (SP_STAGE + 1, "spread"), (SP_Q, "spread"), (SP_Q + 1, "spread"),
            (20000, "one"), (3 * SP_Q + 5, "spread")]
    tiles, t = [], ntile // 3
    while len(tiles) < len(plan):
        if t not in corner and t != ntile - 1:
            tiles.append(t)
        t += 5
    assert t < ntile - 1
    bg = rng.integers(0, ncell, 150000)
    bg = bg[~np.isin(bg // ts, tiles)]
    parts, wanted = [], {}
    for (n, where), tile in zip(plan, tiles):
        c0, c1 = tile * ts, min((tile + 1) * ts, ncell)
        if where == "last":
            parts.append(np.full(n, c1 - 1))
        elif where == "one":
            parts.append(np.full(n, c0 + (c1 - c0) // 2))
        elif n:
            parts.append(rng.integers(c0, c1, n))
        wanted[tile] = n
    nres = sum(p.size for p in parts)
    parts += [bg, np.full(40, ncell - 1)]                      # (the last tile, short where ncell is no multiple of cpt, is not empty)
    if route == 0:                                             # the re-sort of the atomic route: a cell through LDS, one by rank counting
        parts += [np.full(700, 12345), np.full(1500, 7 * (ncell // 8))]
    xall = np.vstack([_points_of_cells(nodes, np.concatenate(parts), rng), special])
    m = xall.shape[0]
    # a seeded random order; the records of the reserved tiles keep away from the places whose weight will be zero, so that the
    # tiles hold the counts above among the PLACED points
    order = rng.permutation(m)
    if weights == "tenth":
        live = order[order % 10 != 0]
        order = np.concatenate([live[:nres], rng.permutation(np.concatenate([live[nres:], order[order % 10 == 0]]))])
    x = np.empty_like(xall)
    x[order] = xall
    if pad:
        x = np.ascontiguousarray(np.hstack([x, np.full((m, pad), 1.0e300)]))
    y = rng.standard_normal(m)
    w = None
    if weights is not None:
        w = 0.5 + rng.random(m)
        if weights == "tenth":
            w[::10] = 0.0
    return nodes, x, y, w, route, cpt, wanted


def check_binning(label, nodes, x, y, w, route, cpt, wanted=None):
    nd = len(nodes)
    out = capi.debug_bin_points(nodes, [0.0] * nd, [float(n - 1) for n in nodes], x, y, w)
    print(f"{label}: nodes {list(nodes)}, {x.shape[0]} points, route {out['route']}, cpt {out['cpt']}, placed {out['placed']}")
    perm, cells, stride, ncell = _grid(nodes)
    assert np.array_equal(out["perm"], perm), label
    assert np.array_equal(out["cells"], np.asarray(nodes)[out["perm"]] - 3), label
    assert np.array_equal(out["cellstride"], np.concatenate([[1], np.cumprod(out["cells"].astype(np.int64))[:-1]])), label
    assert (out["route"], out["cpt"]) == (route, cpt), label
    key = reference_keys(nodes, x, w, out["perm"], out["cellstride"])
    assert np.array_equal(out["key"], key), f"{label}: first wrong key at point {np.argmax(out['key'] != key)}"
    live = np.nonzero(key < ncell)[0]
    pop = np.bincount(key[live], minlength=ncell)
    offset = np.concatenate([[0], np.cumsum(pop)])
    assert np.array_equal(out["offset"], offset), f"{label}: first wrong offset at cell {np.argmax(out['offset'] != offset)}"
    assert out["offset"][ncell] == out["placed"] == live.size and out["nrows_data"] == float(live.size), label
    idx = live[np.argsort(key[live], kind="stable")]
    assert np.array_equal(out["idx"], idx), f"{label}: first wrong index at sorted position {np.argmax(out['idx'] != idx)}"
    for d in range(nd):
        assert np.array_equal(out["xs"][d], x[idx, out["perm"][d]]), (label, d)
    assert np.array_equal(out["ys"], y[idx]), label
    assert np.array_equal(out["ws"], np.ones(idx.size) if w is None else w[idx]), label
    if wanted is not None:                                     # the reserved tiles hold what the case names
        ts = max(cpt, 1)
        tpop = np.bincount(key[live] // ts, minlength=(ncell + ts - 1) // ts)
        for tile, n in wanted.items():
            assert tpop[tile] == n, (label, tile, n, tpop[tile])
    return out, pop


def _tile_pop(nodes, x, w, cpt):
    """placed records per tile of max(cpt, 1) cells"""
    perm, cells, stride, ncell = _grid(nodes)
    key = reference_keys(nodes, x, w, perm, stride)
    return np.bincount(key[key < ncell] // max(cpt, 1), minlength=(ncell + max(cpt, 1) - 1) // max(cpt, 1)), ncell


@pytest.mark.parametrize("name", list(CASES))
def test_cases_hold_the_tiles_they_name(name):
    """CPU: the inputs of every case contain what the second level can get wrong -- a tile without a record, one whose records all
    sit in its last cell, tiles of exactly SP_STAGE and SP_STAGE + 1 records (staged in LDS or not), of SP_Q and SP_Q + 1 (one
    sub-block or two), 20 000 records in one cell, more than three sub-blocks spread over many cells (the carry between
    sub-blocks), a last tile that is not empty -- counted among the points of non-zero weight."""
    nodes, x, y, w, route, cpt, wanted = build_case(name)
    tpop, ncell = _tile_pop(nodes, x, w, cpt)
    for tile, n in wanted.items():
        assert tpop[tile] == n, (name, tile)
    assert sorted(wanted.values()) == [0, 300, SP_STAGE, SP_STAGE + 1, SP_Q, SP_Q + 1, 20000, 3 * SP_Q + 5]
    assert tpop[-1] > 0 and 150000 <= x.shape[0] <= 300000
    if name in ("1d_tiles_nb_smallest", "2d_tiles_nb", "3d_tiles_nb", "4d_tiles_nb", "2d_two_levels_smallest"):
        assert ncell % cpt != 0                                # a short last tile
    if route == 0:                                             # cell_order_kernel does not order cells of more than 65 536 points
        perm, cells, stride, _ = _grid(nodes)
        assert np.bincount(reference_keys(nodes, x, None, perm, stride)).max() <= 65536


def test_bin_points_entry_rejects_bad_arguments_without_gpu():
    import ctypes as C
    L = capi.lib()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    nodes = np.array([8, 8], dtype=np.int32)
    lo, hi = np.zeros(2), np.full(2, 7.0)
    x, y = np.zeros((4, 2)), np.zeros(4)
    i = [np.zeros(64, dtype=np.int32) for _ in range(8)]
    d = [np.zeros(16) for _ in range(4)]
    placed = C.c_int64(0)

    def call(nd=2, nodes=nodes, lo=lo, x=x, y=y, m=4, ldx=2, key=i[5], rows=d[3], placed=C.byref(placed)):
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)
        return L.splpak_debug_bin_points(nd, p(nodes, ip), p(lo, dp), p(hi, dp), m, p(x, dp), ldx, p(y, dp), None, p(i[0], ip),
                                         p(i[1], ip), p(i[2], ip), p(i[3], ip), p(i[4], ip), p(key, ip), p(i[6], ip), p(i[7], ip),
                                         p(d[0], dp), p(d[1], dp), p(d[2], dp), placed, p(rows, dp))

    assert call(nodes=None) == capi.E_BADARG
    assert call(lo=None) == capi.E_BADARG
    assert call(x=None) == capi.E_BADARG
    assert call(y=None) == capi.E_BADARG
    assert call(key=None) == capi.E_BADARG
    assert call(rows=None) == capi.E_BADARG
    assert call(placed=None) == capi.E_BADARG
    assert call(m=0) == capi.E_BADARG
    assert call(m=2 ** 31) == capi.E_BADARG
    assert call(ldx=1) == capi.E_BADARG
    assert "l1xdat" in capi.last_error()
    assert call(nd=0) == 101
    assert call(nodes=np.array([8, 3], dtype=np.int32)) == 102
    assert L.splpak_debug_plan_gram_shape(None, i[0].ctypes.data_as(ip)) == capi.E_BADARG


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_sorted_order_matches_numpy(name):
    nodes, x, y, w, route, cpt, wanted = build_case(name)
    check_binning(name, nodes, x, y, w, route, cpt, wanted)


@pytest.mark.gpu
@pytest.mark.parametrize("nodes,route,cpt", [([4098], 1, 1), ([90, 80], 2, 2), ([105, 104, 105], 3, 257)])
@pytest.mark.parametrize("ndata", [1, SP_Q - 1, SP_Q, SP_Q + 1, 16 * SP_Q + 1])
def test_point_counts_at_the_block_edges(nodes, route, cpt, ndata):
    """One point; a block of SP_Q points less one, full, plus one; 16 blocks plus one point (a second chunk of the column sums)."""
    rng = np.random.default_rng(ndata + len(nodes))
    _, _, _, ncell = _grid(nodes)
    x = _points_of_cells(nodes, rng.integers(0, ncell, ndata), rng)
    w = 0.5 + rng.random(ndata)
    w[3::10] = 0.0
    check_binning(f"{ndata} points", nodes, x, rng.standard_normal(ndata), w, route, cpt)


@pytest.mark.gpu
@pytest.mark.parametrize("nodes,route,cpt", [([4098], 1, 1), ([90, 80], 2, 2), ([1030, 1025], 3, 257), ([16769030], 0, 0)])
def test_all_weights_zero_places_nothing(nodes, route, cpt):
    rng = np.random.default_rng(5)
    _, _, _, ncell = _grid(nodes)
    x = _points_of_cells(nodes, rng.integers(0, ncell, 20000), rng)
    out, _ = check_binning("all weights zero", nodes, x, rng.standard_normal(20000), np.zeros(20000), route, cpt)
    assert out["placed"] == 0 and not out["offset"].any()


def _atomic_child():
    for name in ATOMIC_CASES:
        nodes, x, y, w, _, cpt, wanted = build_case(name)
        check_binning(name + " SPLPAK_BIN_ATOMIC=1", nodes, x, y, w, 0, cpt, wanted)


@pytest.mark.gpu
def test_atomic_route_by_switch_matches_numpy():
    """The same two cases through the atomic route (SPLPAK_BIN_ATOMIC=1, read once per process: a child process), held against the
    same numpy reference: route 0, the grid's cpt."""
    code = "import sys; sys.path.insert(0, %r)\nfrom tests.test_binning import _atomic_child\n_atomic_child()\n" % ROOT
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SPLPAK_BIN_ATOMIC="1"), capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    assert r.stdout.count("route 0") == len(ATOMIC_CASES)
