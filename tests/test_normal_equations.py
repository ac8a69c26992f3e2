"""The assembled normal equations and each factorisation on their own, without iterative refinement.

Every fit refines against the ROWS (planfit.hip solve_and_refine), so an assembled N or a factor that is slightly wrong only
costs refinement steps: the coefficients still meet the parity bar.  These tests look at the two objects directly.

CPU tier: the oracle's normal equations (oracle/splpak_banded.c oracle_normal_equations, long double) against the oracle's
rows (rhs - N c is the rows' gradient at any c); the new diagnostic entries' argument checks; the fronts of the
nested-dissection tree (splpak_debug_nd_fronts).
GPU tier:
  A. what a fit assembled (splpak_debug_plan_normal_equations) against the oracle, entry by entry, with exact zeros where the
     oracle has no term at all (a contribution scattered into the wrong slot); the same on the grids where a wave of the Gram pass
     owns a run of 2, 3 or 8 cells (test_gram_runs_match_oracle);
  B. every factorisation alone (splpak_debug_plan_solve): synthetic SPD matrices with independent random entries on the 7^d
     pattern (forward error) and the fits' own N (backward error; and bitwise the coefficients of a fit without refinement);
  C. a matrix that is not positive definite at a chosen column: 107 from every factorisation, then the same plan solves again.
"""
import ctypes as C

import numpy as np
import pytest

from splpak_amd import capi
from splpak_amd.synth import synth_points
from tests.cases import CASES, make_inputs

NE_TOL = 1e-13          # |dN_ij| <= NE_TOL * absN_ij, |drhs_i| <= NE_TOL * absrhs_i
NE_CEIL = 1e-12         # never looser, whatever the points per cell
SPD_FWD_TOL = 1e-12     # synthetic SPD, Gershgorin condition bound <= 100: ||x - x*|| / ||x*||
BWD_TOL = 1e-13         # the fits' own N: ||b - N x|| / (||N|| ||x|| + ||b||)


# ---------------------------------------------------------------------------------------------------------------
# half stencils on the host (reference numbering: dimension 0 fastest, slot code = sum_d (o_d + 3) 7^d, code <= centre)
def _grid_index(nodes):
    nodes = [int(n) for n in nodes]
    ncol = int(np.prod(nodes))
    stride = np.cumprod([1] + nodes[:-1])
    multi = np.stack([(np.arange(ncol) // stride[d]) % nodes[d] for d in range(len(nodes))], axis=1)
    return ncol, stride, multi


def stencil_slots(nodes):
    """-> list of (code, offset o, rows i whose column i + o lies in the grid, those columns)."""
    nd = len(nodes)
    ncol, stride, multi = _grid_index(nodes)
    hst = (7 ** nd + 1) // 2
    out = []
    for code in range(hst):
        o = np.array([(code // 7 ** d) % 7 - 3 for d in range(nd)])
        t = multi + o
        ok = np.all((t >= 0) & (t < np.asarray(nodes)), axis=1)
        rows = np.nonzero(ok)[0]
        out.append((code, o, rows, rows + int(np.dot(o, stride))))
    return out


def stencil_to_sparse(N, nodes):
    """The symmetric matrix of a half stencil as scipy.sparse (csr)."""
    import scipy.sparse as sp
    ncol = N.shape[0]
    centre = N.shape[1] - 1
    r, c, v = [], [], []
    for code, _, rows, cols in stencil_slots(nodes):
        val = N[rows, code]
        r.append(rows); c.append(cols); v.append(val)
        if code != centre:
            r.append(cols); c.append(rows); v.append(val)
    return sp.csr_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(c))), shape=(ncol, ncol))


def stencil_matvec(N, nodes, x, dtype=np.longdouble, absolute=False):
    """N x (|N| |x| with absolute=True), accumulated in `dtype`."""
    centre = N.shape[1] - 1
    Nd = np.abs(N).astype(dtype) if absolute else N.astype(dtype)
    xd = np.abs(x).astype(dtype) if absolute else np.asarray(x).astype(dtype)
    y = np.zeros(N.shape[0], dtype=dtype)
    for code, _, rows, cols in stencil_slots(nodes):
        v = Nd[rows, code]
        np.add.at(y, rows, v * xd[cols])
        if code != centre:
            np.add.at(y, cols, v * xd[rows])
    return y


def stencil_norm_inf(N, nodes):
    return float(np.max(stencil_matvec(N, nodes, np.ones(N.shape[0]), dtype=np.float64, absolute=True)))


def synthetic_spd(nodes, seed):
    """Independent random values for every N(i, i+o) on the 7^d pattern (no tensor-product symmetry to hide a mirrored
    index behind); constant diagonal 1.03 x the largest off-diagonal row sum: Gershgorin condition bound <= 2.03 / 0.03."""
    rng = np.random.default_rng(seed)
    ncol = int(np.prod(nodes))
    hst = (7 ** len(nodes) + 1) // 2
    centre = hst - 1
    N = np.zeros((ncol, hst))
    rsum = np.zeros(ncol)
    for code, _, rows, cols in stencil_slots(nodes):
        if code == centre:
            continue
        v = rng.uniform(-1.0, 1.0, rows.size)
        N[rows, code] = v
        np.add.at(rsum, rows, np.abs(v))
        np.add.at(rsum, cols, np.abs(v))
    N[:, centre] = 1.03 * max(rsum.max(), 1.0)
    lo, hi = N[0, centre] - rsum.max(), N[0, centre] + rsum.max()
    assert hi / lo <= 100.0
    return N


# ---------------------------------------------------------------------------------------------------------------
# CPU tier
ORACLE_CASES = ["c1_1d16", "c1_1d16_xt0", "1d_sparse", "2d16_zero_w", "2d16_outside", "2d_aniso_box", "2d32_cc_xt0", "3d8_cc_clust",
                "3d_aniso", "4d5_cc", "4d4"]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_oracle_normal_equations_are_the_rows_gradient(port, name):
    """rhs - N c = A^T (b - A c) over the reference's rows, for any c: the long-double normal equations tied to the rows the
    rest of the suite already pins (oracle_rows_gradient), including their counts."""
    inp = make_inputs(CASES[name])
    a = [inp[k] for k in ("ndim", "xdata", "ydata", "wdata", "xmin", "xmax", "nodes", "xtrap")]
    ne = port.normal_equations(*a)
    worst = 0.0
    for seed in (1, 2):
        c = np.random.default_rng(seed).uniform(-1.0, 1.0, ne["rhs"].size)
        rho = port.rows_gradient_vec(*a, c)
        ref = ne["rhs"].astype(np.longdouble) - stencil_matvec(ne["N"], inp["nodes"], c)
        scale = ne["absrhs"] + stencil_matvec(ne["absN"], inp["nodes"], c, dtype=np.float64, absolute=True)
        err = np.abs(np.asarray(ref - rho, dtype=np.float64))
        worst = max(worst, float(np.max(err / np.where(scale > 0, scale, 1.0))))
        assert np.all(err[scale == 0] == 0)
    _, _, nrow, ncons = port.rows_gradient(*a, np.zeros(ne["rhs"].size))
    print(f"{name}: |rhs - N c - rho| / (|rhs| + |N||c|) <= {worst:.1e}; rows {ne['data_rows']} + {ne['constraint_rows']}")
    assert worst <= 1e-13
    assert (ne["data_rows"], ne["constraint_rows"]) == (nrow, ncons)
    assert np.all(ne["absN"] >= np.abs(ne["N"])) and np.all(ne["absrhs"] >= np.abs(ne["rhs"]))


def test_debug_plan_entries_reject_null_arguments_without_gpu():
    L = capi.lib()
    d = np.zeros(16)
    p = d.ctypes.data_as(C.POINTER(C.c_double))
    assert L.splpak_debug_plan_normal_equations(None, p, p) == capi.E_BADARG
    assert L.splpak_debug_plan_solve(None, p, p, p, p) == capi.E_BADARG
    nodes = np.array([8, 8, 8], dtype=np.int32)
    ip = nodes.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.splpak_debug_nd_fronts(3, ip, 0, None, 0, None, None, None, None, None, None) == capi.E_BADARG
    nf = np.zeros(1, dtype=np.int32)
    assert L.splpak_debug_nd_fronts(3, ip, 0, nf.ctypes.data_as(C.POINTER(C.c_int32)), 100, None, None, None, None, None, None) == capi.E_BADARG
    bad = np.array([3, 8], dtype=np.int32)
    assert L.splpak_debug_nd_fronts(2, bad.ctypes.data_as(C.POINTER(C.c_int32)), 0, nf.ctypes.data_as(C.POINTER(C.c_int32)), 0,
                                    None, None, None, None, None, None) == 102


# grids of the factorisation tests; the ND ones are chosen so that the tree has fronts with w mod 256 in {1, 255, 0} and
# borders with h mod 64 in {1, 63, 0} (padding of the diagonal blocks and of the border tiles at both ends)
ND_GRIDS = [[33], [40, 7], [64, 64], [32, 35], [16, 24], [9, 17, 13], [5, 30, 5], [8, 8, 8], [16, 16, 16], [9, 19, 19], [5, 17, 17],
            [24, 40, 24], [6, 6, 6, 6], [8, 9, 10, 11]]


@pytest.mark.parametrize("nodes", [[33], [40, 7], [64, 64], [9, 17, 13], [5, 30, 5], [24, 40, 24], [8, 9, 10, 11]])
@pytest.mark.parametrize("split", [0, 5, 11])
def test_nd_fronts_invariants(nodes, split):
    t = capi.debug_nd_fronts(nodes, split_min=split)
    ncol = int(np.prod(nodes))
    nf = t["depth"].size
    assert t["parent"][-1] == -1 and t["depth"][-1] == 0 and np.sum(t["parent"] == -1) == 1
    for f in range(nf - 1):
        par = t["parent"][f]
        assert f < par < nf and t["depth"][par] == t["depth"][f] - 1
    assert t["w"].sum() == ncol and np.all(t["w"] > 0) and np.all(t["h"] >= 0) and t["h"][-1] == 0
    # every node owned once; a front's own nodes are its w consecutive elimination positions, fronts in order
    assert np.all((t["front_of"] >= 0) & (t["front_of"] < nf))
    assert np.array_equal(np.bincount(t["front_of"], minlength=nf), t["w"])
    assert np.array_equal(np.sort(t["pos"]), np.arange(ncol))
    start = np.concatenate([[0], np.cumsum(t["w"])[:-1]])
    assert np.all(t["pos"] >= start[t["front_of"]]) and np.all(t["pos"] < (start + t["w"])[t["front_of"]])


def test_nd_grids_cover_the_padding_edges():
    w_seen, h_seen = set(), set()
    for nodes in ND_GRIDS:
        t = capi.debug_nd_fronts(nodes)
        w_seen |= {int(v) % 256 for v in t["w"] if v > 0}
        h_seen |= {int(v) % 64 for v in t["h"] if v > 0}
    assert {1, 255, 0} <= w_seen, w_seen
    assert {1, 63, 0} <= h_seen, h_seen


# ---------------------------------------------------------------------------------------------------------------
# GPU tier
def _tensors(inp):
    import torch
    dev = torch.device("cuda")
    x = torch.tensor(np.ascontiguousarray(inp["xdata"]), dtype=torch.float64, device=dev)
    y = torch.tensor(inp["ydata"], dtype=torch.float64, device=dev)
    w = None if inp["wdata"] is None else torch.tensor(inp["wdata"], dtype=torch.float64, device=dev)
    return x, y, w


def _plan(nodes, xmin=None, xmax=None, xtrap=1.0, max_ndata=1):
    nd = len(nodes)
    return capi.Plan(nd, list(nodes), [0.0] * nd if xmin is None else xmin, [1.0] * nd if xmax is None else xmax, xtrap, max_ndata)


def _fit_ne(inp, refine=None):
    """Fit through a Plan -> (ierror, info, coef, N, rhs, factorisation code)."""
    import torch
    x, y, w = _tensors(inp)
    plan = capi.Plan(inp["ndim"], inp["nodes"], inp["xmin"], inp["xmax"], inp["xtrap"], x.shape[0])
    try:
        if refine is not None:
            plan.set_refine(refine, 1e-11)
        coef = torch.zeros(plan.ncol, dtype=torch.float64, device=x.device)
        ierr, info = plan.fit(x, y, w, coef)
        torch.cuda.synchronize()
        N, rhs = plan.normal_equations()
        return ierr, info, coef.cpu().numpy(), N, rhs, plan.factorisation()[0], plan
    except Exception:
        plan.close()
        raise


def _compare_ne(label, inp, N, rhs, info, ne, tol=NE_TOL):
    assert (info[0], info[1]) == (ne["data_rows"], ne["constraint_rows"]), label
    dN = np.abs(N - ne["N"])
    dr = np.abs(rhs - ne["rhs"])
    zN, zr = ne["absN"] == 0, ne["absrhs"] == 0
    eN = float(np.max(np.where(zN, 0.0, dN / np.where(zN, 1.0, ne["absN"]))))
    er = float(np.max(np.where(zr, 0.0, dr / np.where(zr, 1.0, ne["absrhs"]))))
    print(f"{label}: |dN| / absN <= {eN:.2e}, |drhs| / absrhs <= {er:.2e} (bound {tol:.1e}); "
          f"{int(np.count_nonzero(zN))} structural zeros; rows {int(info[0])} + {int(info[1])}")
    assert np.all(N[zN] == 0), f"{label}: entries where the rows have no term: {np.argwhere(zN & (N != 0))[:5]}"
    assert np.all(rhs[zr] == 0), label
    assert eN <= tol and er <= tol, label


def _oracle_ne(port, inp):
    return port.normal_equations(inp["ndim"], inp["xdata"], inp["ydata"], inp["wdata"], inp["xmin"], inp["xmax"], inp["nodes"],
                                 inp["xtrap"])


def _seeded(nd, nodes, m, seed, xtrap=1.0, weighted=True, xmin=None, xmax=None):
    x, y, w = synth_points(nd, m)
    rng = np.random.default_rng(seed)
    x = np.ascontiguousarray(rng.permutation(x))
    xmin = np.zeros(nd) if xmin is None else np.asarray(xmin, dtype=np.float64)
    xmax = np.ones(nd) if xmax is None else np.asarray(xmax, dtype=np.float64)
    x = xmin + x * (xmax - xmin)
    return dict(ndim=nd, xdata=x, ydata=y, wdata=(w if weighted else None), xmin=xmin, xmax=xmax,
                nodes=np.array(nodes, dtype=np.int32), xtrap=float(xtrap))


def _extra_cases():
    out = {}
    # dimensions not in ascending node order (the plan permutes them: Grid::perm)
    out["perm_3d_12_5_8"] = _seeded(3, [12, 5, 8], 20000, 11, xmin=[-1.0, 0.0, 2.0], xmax=[1.0, 3.0, 2.5])
    out["perm_4d_7_4_6_5"] = _seeded(4, [7, 4, 6, 5], 20000, 12)
    out["perm_2d_30_9"] = _seeded(2, [30, 9], 8000, 13, weighted=False)
    # l1xdat > ndim: a column the fit must skip
    inp = _seeded(2, [10, 14], 5000, 14)
    inp["xdata"] = np.ascontiguousarray(np.hstack([inp["xdata"], np.full((inp["xdata"].shape[0], 1), 7.0)]))
    out["l1xdat_3_2d"] = inp
    # a negative first weight: unweighted (src/splpak.F90 splcw)
    inp = _seeded(3, [6, 7, 8], 8000, 15)
    inp["wdata"] = inp["wdata"].copy()
    inp["wdata"][0] = -1.0
    out["neg_first_weight"] = inp
    # a far-outside point
    inp = _seeded(2, [12, 12], 4000, 16)
    inp["xdata"] = inp["xdata"].copy()
    inp["xdata"][17] = [40.0, -25.0]
    out["far_outside"] = inp
    # cells of more than 1024 points
    out["big_cells_2d"] = _seeded(2, [5, 6], 60000, 17)
    out["big_cells_3d"] = _seeded(3, [4, 5, 4], 40000, 18)
    # 24^3 with 1e5 points
    out["3d24_1e5"] = _seeded(3, [24, 24, 24], 100000, 19)
    return out


EXTRA = _extra_cases()


def _busiest_cell(inp):
    nodes = np.asarray(inp["nodes"])
    x = inp["xdata"][:, :inp["ndim"]]
    dx = (inp["xmax"] - inp["xmin"]) / (nodes - 1)
    it = np.clip(np.floor((x - inp["xmin"]) / dx).astype(np.int64) - 1, 0, nodes - 4)
    key = np.ravel_multi_index(it.T, nodes - 3)
    return int(np.bincount(key).max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES) + list(EXTRA))
def test_assembly_matches_oracle(port, name, monkeypatch):
    monkeypatch.setenv("SPLPAK_SOLVER", "direct")
    inp = make_inputs(CASES[name]) if name in CASES else EXTRA[name]
    ierr, info, _, N, rhs, _, plan = _fit_ne(inp)
    plan.close()
    assert ierr == 0
    ne = _oracle_ne(port, inp)
    big = _busiest_cell(inp)
    tol = min(max(NE_TOL, big * 2.0 ** -53), NE_CEIL)
    _compare_ne(f"{name} (busiest cell {big} points)", inp, N, rhs, info, ne, tol)


ASSEMBLY_VARIANTS = [{"SPLPAK_GRAM_SCRATCH_MB": "1"}, {"SPLPAK_GRAM_SCRATCH_MB": "3"}, {"SPLPAK_GRAM_SCRATCH_MB": "8"},
                     {"SPLPAK_GRAM_VALU": "1"}, {"SPLPAK_BIN_ATOMIC": "1"}]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["2d16_zero_w", "3d8_cc_clust", "3d_aniso", "4d6", "perm_3d_12_5_8", "3d24_1e5"])
def test_assembly_variants_match_oracle(port, name, monkeypatch):
    """The slab-wise Gram scratch, the VALU Gram kernels and the atomic binning against the oracle, not only against each other."""
    monkeypatch.setenv("SPLPAK_SOLVER", "direct")
    inp = make_inputs(CASES[name]) if name in CASES else EXTRA[name]
    ne = _oracle_ne(port, inp)
    for env in ASSEMBLY_VARIANTS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ierr, info, _, N, rhs, _, plan = _fit_ne(inp)
        plan.close()
        for k in env:
            monkeypatch.delenv(k)
        assert ierr == 0
        _compare_ne(f"{name} {env}", inp, N, rhs, info, ne)


# ---- Gram passes in which a wave owns a RUN of consecutive cells (gram.hip gram_wave_kernel, 2-D and 3-D): launch_gram gives a
# wave min(8, cells of the slab / 8192) cells, so every grid above stays at run 1.  What exists only for runs -- the offsets of a
# run in one register, the next cell's first chunk fetched before the current cell's products, the empty-cell shortcut inside a
# run, a last wave with fewer cells than its run -- is reached by grid size here, and the run is asserted from the plan.
# name -> nodes, points, seed, run, whether the cell count leaves a short last run, xtrap, SPLPAK_GRAM_SCRATCH_MB, expected shape
GRAM_RUN_CASES = {
    "2d131_run2": dict(nodes=[131, 131], m=40000, seed=31, run=2, short=False),           # 16 384 cells = 2 * 8 192: no short run
    "2d184_run3": dict(nodes=[184, 184], m=75000, seed=32, run=3, short=True),            # 32 761 = 3 * 10 920 + 1
    "2d260_run8": dict(nodes=[260, 260], m=150000, seed=33, run=8, short=True),           # 66 049 = 32 * 2 064 + 1: one wave, one cell
    "3d29_run2": dict(nodes=[29, 29, 29], m=60000, seed=34, run=2, short=False),          # 17 576 cells = 2 * 8 788: no short run
    "3d44_run8": dict(nodes=[44, 44, 44], m=150000, seed=35, run=8, short=True),          # 68 921 = 8 * 8 615 + 1
    # slabs of 69 hyper-rows of 257 cells (23 MB of scratch / 345 408 bytes per hyper-row): run 2 where the whole grid takes 8
    "2d260_slabs_run2": dict(nodes=[260, 260], m=150000, seed=33, run=2, short=True, scratch_mb=23,
                             shape=dict(slabs=4, rows=69, cells=17733, run=2, last_cells=12850, last_run=1)),
    # no smoothing: the kernel without a histogram (hblk == nullptr); no cell may be empty, so only the busy-cell pattern applies
    "2d131_run2_xtrap0": dict(nodes=[131, 131], m=600000, seed=36, run=2, short=False, xtrap=0.0),
}


def _cell_keys(inp):
    """Cell of every point (dimension 0 fastest), with the library's own arithmetic (basis.hpp window_start)."""
    nodes = np.asarray(inp["nodes"], dtype=np.int64)
    dx = (inp["xmax"] - inp["xmin"]) / (nodes - 1).astype(np.float64)
    t = (1.0 / dx) * (inp["xdata"][:, :inp["ndim"]] - inp["xmin"])
    ws = np.clip(np.trunc(t).astype(np.int64) - 1, 0, nodes - 4)
    return np.ravel_multi_index(ws[:, ::-1].T, (nodes - 3)[::-1])


def _run_patterns(pop, slabs):
    """What the runs of the slabs [(first cell, cells, run)] contain, from the points per cell."""
    found = dict(busy_then_some=False, empty_then_some=False, first_empty=False, all_empty=False, short_last=False)
    for c0, n, run in slabs:
        nfull = n // run
        groups = [pop[c0:c0 + nfull * run].reshape(nfull, run)]
        if n % run:
            groups.append(pop[c0 + nfull * run:c0 + n][None, :])
            found["short_last"] = True
        for g in groups:
            if g.shape[1] > 1:
                found["busy_then_some"] |= bool(np.any((g[:, :-1] > 64) & (g[:, 1:] > 0)))
                found["empty_then_some"] |= bool(np.any((g[:, :-1] == 0) & (g[:, 1:] > 0)))
            found["first_empty"] |= bool(np.any((g[:, 0] == 0) & (g.max(axis=1) > 0)))
            found["all_empty"] |= bool(np.any(g.max(axis=1) == 0))
    return found


def _gram_run_inputs(name):
    """The seeded stream of synth_points, permuted, a third of it moved into a patch of 5 % of the box's side; then, in the middle of
    the first slab, the points of one whole run and of the first cell of another are taken out, and a cell of 70 points followed by one of 2
    is put in: every pattern a run can hold is there whatever the stream happens to give."""
    c = GRAM_RUN_CASES[name]
    nd, run = len(c["nodes"]), c["run"]
    inp = _seeded(nd, c["nodes"], c["m"], c["seed"], xtrap=c.get("xtrap", 1.0))
    x, y, w = inp["xdata"].copy(), inp["ydata"].copy(), inp["wdata"].copy()
    third = c["m"] // 3
    x[:third] = 0.3 + 0.05 * x[:third]
    inp.update(xdata=x, ydata=y, wdata=w)
    if c.get("xtrap", 1.0) == 0.0:
        return inp
    cells = np.asarray(c["nodes"]) - 3
    b = (c.get("shape", dict(cells=int(np.prod(cells))))["cells"] // run) // 2       # a run in the middle of the first slab ...
    while np.any(np.unravel_index(np.arange(b * run, (b + 4) * run), cells[::-1])[-1] < 2):
        b += 1                                                  # ... of interior cells along dimension 0
    key = _cell_keys(inp)
    keep = ~(((key >= b * run) & (key < (b + 1) * run)) | (key == (b + 2) * run))
    rng = np.random.default_rng(c["seed"] + 100)
    newc = np.concatenate([np.full(2, (b + 2) * run + 1), np.full(70, (b + 3) * run), np.full(2, (b + 3) * run + 1)])
    ws = np.stack(np.unravel_index(newc, cells[::-1])[::-1], axis=1)
    xn = (ws + 1.0 + rng.uniform(0.05, 0.95, ws.shape)) / (np.asarray(c["nodes"]) - 1.0)
    inp.update(xdata=np.ascontiguousarray(np.vstack([x[keep], xn])), ydata=np.concatenate([y[keep], np.sin(xn.sum(axis=1))]),
               wdata=np.concatenate([w[keep], rng.uniform(0.5, 1.5, newc.size)]))
    return inp


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRAM_RUN_CASES))
def test_gram_runs_match_oracle(port, name, monkeypatch):
    """The normal equations of grids on which a wave of the Gram pass owns 2, 3 or 8 cells, entry by entry against the oracle
    under the rule of test_assembly_matches_oracle, with exact zeros where the rows have no term.  The run (and with
    SPLPAK_GRAM_SCRATCH_MB the slabs) comes from splpak_debug_plan_gram_shape and must be what the case names; the points per
    cell are asserted to hold, inside a run: a cell of more than 64 points followed by a non-empty one (a second chunk while the
    next cell's prefetch is pending), an empty cell followed by a non-empty one, a run starting with an empty cell, a run of empty
    cells only, and -- where the cell count is no multiple of the run: not at 16 384 and 17 576 cells with run 2 -- the short
    last run.  xtrap = 0 allows no empty cell: that case is about the kernel without a histogram and rests on the fit returning 0.
    The oracle's own time is the long part: about 8 s for 44^3 on 16 threads, below 2 s for the others."""
    c = GRAM_RUN_CASES[name]
    monkeypatch.setenv("SPLPAK_SOLVER", "direct")
    inp = _gram_run_inputs(name)
    nd, ncell = inp["ndim"], int(np.prod(np.asarray(c["nodes"]) - 3))
    raw = capi.debug_bin_points(inp["nodes"], inp["xmin"], inp["xmax"], inp["xdata"], inp["ydata"], inp["wdata"])
    assert np.array_equal(raw["perm"], np.arange(nd))          # equal node counts: the internal cell order is the caller's
    key = _cell_keys(inp)
    pop = np.bincount(key[inp["wdata"] != 0], minlength=ncell)
    assert np.array_equal(np.diff(raw["offset"]), pop)
    if "scratch_mb" in c:
        monkeypatch.setenv("SPLPAK_GRAM_SCRATCH_MB", str(c["scratch_mb"]))
    ierr, info, _, N, rhs, _, plan = _fit_ne(inp)
    try:
        shape = plan.gram_shape()
    finally:
        plan.close()
    want = c.get("shape", dict(slabs=1, rows=int(c["nodes"][-1]) - 3, cells=ncell, run=c["run"], last_cells=ncell, last_run=c["run"]))
    slabs = [(i * shape["cells"], shape["cells"], shape["run"]) for i in range(shape["slabs"] - 1)]
    slabs.append(((shape["slabs"] - 1) * shape["cells"], shape["last_cells"], shape["last_run"]))
    found = _run_patterns(pop, slabs)
    empty = int(np.count_nonzero(pop == 0))
    print(f"{name}: {shape}; {inp['xdata'].shape[0]} points, {empty} of {ncell} cells empty, {int(np.count_nonzero(pop > 64))} of more "
          f"than 64 points; {found}")
    assert shape == want, name
    if c.get("xtrap", 1.0) == 0.0:
        assert empty == 0 and found["busy_then_some"], found
    else:
        assert found == dict(busy_then_some=True, empty_then_some=True, first_empty=True, all_empty=True, short_last=c["short"]), found
    assert ierr == 0
    ne = _oracle_ne(port, inp)
    big = _busiest_cell(inp)
    tol = min(max(NE_TOL, big * 2.0 ** -53), NE_CEIL)
    _compare_ne(f"{name} (run {shape['run']}, busiest cell {big} points)", inp, N, rhs, info, ne, tol)


@pytest.mark.gpu
def test_debug_plan_entries_refuse_what_there_is_not(monkeypatch):
    L = capi.lib()
    plan = _plan([8, 8])
    try:
        N = np.zeros((64, 25))
        r = np.zeros(64)
        dp = C.POINTER(C.c_double)
        assert L.splpak_debug_plan_normal_equations(plan._h, N.ctypes.data_as(dp), r.ctypes.data_as(dp)) == capi.E_UNSUPPORTED
        assert L.splpak_debug_plan_normal_equations(plan._h, None, r.ctypes.data_as(dp)) == capi.E_BADARG
        assert L.splpak_debug_plan_solve(plan._h, None, r.ctypes.data_as(dp), r.ctypes.data_as(dp), None) == capi.E_BADARG
    finally:
        plan.close()
    # an iteration-only 4-D plan never assembles and has no factorisation
    monkeypatch.setenv("SPLPAK_SOLVER", "pcg")
    inp = _seeded(4, [6, 6, 6, 6], 8000, 21)
    import torch
    x, y, w = _tensors(inp)
    plan = capi.Plan(4, inp["nodes"], inp["xmin"], inp["xmax"], 1.0, x.shape[0])
    try:
        assert plan.factorisation()[0] == 6
        coef = torch.zeros(plan.ncol, dtype=torch.float64, device=x.device)
        ierr, _ = plan.fit(x, y, w, coef)
        assert ierr == 0
        N = np.zeros((plan.ncol, (7 ** 4 + 1) // 2))
        r = np.zeros(plan.ncol)
        dp = C.POINTER(C.c_double)
        assert L.splpak_debug_plan_normal_equations(plan._h, N.ctypes.data_as(dp), r.ctypes.data_as(dp)) == capi.E_UNSUPPORTED
        assert L.splpak_debug_plan_solve(plan._h, N.ctypes.data_as(dp), r.ctypes.data_as(dp), r.ctypes.data_as(dp), None) == capi.E_UNSUPPORTED
    finally:
        plan.close()


# (label, environment, grids, factorisation code the plan must report)
FACTORISATIONS = [
    ("band", {"SPLPAK_ND": "0", "SPLPAK_NO_TWOEND": "1"}, [[200], [40, 7], [9, 17, 13], [6, 6, 6, 6]], 1),
    ("band_pipeline", {"SPLPAK_ND": "0", "SPLPAK_NO_TWOEND": "1", "SPLPAK_NARROW_BW": "1"}, [[64, 64], [9, 17, 13]], 0),
    ("twoend", {"SPLPAK_ND": "0"}, [[2000], [64, 64], [9, 17, 13], [5, 30, 5], [24, 40, 24]], 2),
    ("nd", {"SPLPAK_ND": "1"}, ND_GRIDS, 4),
    ("nd_split5", {"SPLPAK_ND": "1", "SPLPAK_ND_SPLIT": "5"}, [[9, 17, 13], [16, 16, 16], [64, 64]], 4),
    ("nd_split11", {"SPLPAK_ND": "1", "SPLPAK_ND_SPLIT": "11"}, [[9, 17, 13], [16, 16, 16], [8, 9, 10, 11]], 4),
] + [(f"nd_{k.lower()[10:]}_{v}", {"SPLPAK_ND": "1", k: v}, [[9, 17, 13], [24, 40, 24]], 4)
     for k, v in [("SPLPAK_ND_CUT", "0"), ("SPLPAK_ND_CUT", "2"), ("SPLPAK_ND_SQUARE", "1"), ("SPLPAK_ND_NO_FUSE", "1"),
                  ("SPLPAK_ND_NO_ROOT_LOOKAHEAD", "1"), ("SPLPAK_ND_HALVES", "0"), ("SPLPAK_ND_HALVES", "9"), ("SPLPAK_ND_FULL_DIAG", "1"),
                  ("SPLPAK_ND_SMALL_GRID", "0")]]


def _forced_plan(env, nodes, monkeypatch, code):
    monkeypatch.setenv("SPLPAK_SOLVER", "direct")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = _plan(nodes)
    for k in env:
        monkeypatch.delenv(k)
    got = plan.factorisation()[0]
    if got != code:
        plan.close()
        raise AssertionError(f"{nodes} {env}: factorisation {got}, wanted {code}")
    return plan


def _solve_synthetic(plan, nodes, seed):
    N = synthetic_spd(nodes, seed)
    xs = np.random.default_rng(seed + 1000).uniform(-1.0, 1.0, N.shape[0])
    b = np.asarray(stencil_matvec(N, nodes, xs), dtype=np.float64)
    x, rc, mp = plan.debug_solve(N, b)
    return rc, float(np.max(np.abs(x - xs)) / np.max(np.abs(xs))), mp


@pytest.mark.gpu
@pytest.mark.parametrize("label,env,grids,code", FACTORISATIONS, ids=[f[0] for f in FACTORISATIONS])
def test_factorisation_solves_synthetic_spd(label, env, grids, code, monkeypatch):
    worst = 0.0
    for nodes in grids:
        plan = _forced_plan(env, nodes, monkeypatch, code)
        try:
            rc, err, mp = _solve_synthetic(plan, nodes, seed=len(nodes) * 1000 + int(np.prod(nodes)) % 997)
        finally:
            plan.close()
        print(f"{label} {nodes}: forward error {err:.2e} (bound {SPD_FWD_TOL:.0e}), min pivot {mp:.3g}")
        assert rc == 0 and mp > 0
        assert err <= SPD_FWD_TOL, (label, nodes)
        worst = max(worst, err)
    print(f"{label}: worst forward error {worst:.2e}")


OWN_NE = [("band", {"SPLPAK_ND": "0", "SPLPAK_NO_TWOEND": "1"}, ["c1_1d16", "2d_aniso_box", "3d_aniso", "4d5_cc"], 1),
          ("twoend", {"SPLPAK_ND": "0"}, ["2d32", "3d12", "2d64_c2grid"], 2),
          ("nd", {"SPLPAK_ND": "1"}, ["2d32", "3d12", "3d16", "3d8_cc_clust", "4d6", "perm_3d_12_5_8", "3d24_1e5"], 4),
          ("nd_cut2", {"SPLPAK_ND": "1", "SPLPAK_ND_CUT": "2"}, ["3d16"], 4),
          ("nd_halves9", {"SPLPAK_ND": "1", "SPLPAK_ND_HALVES": "9"}, ["3d16"], 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("label,env,names,code", OWN_NE, ids=[f[0] for f in OWN_NE])
def test_factorisation_of_the_fits_own_normal_equations(label, env, names, code, monkeypatch):
    """Backward error of one solve with the fit's own N / rhs, and a fit without refinement returns exactly that solve."""
    monkeypatch.setenv("SPLPAK_SOLVER", "direct")
    for name in names:
        inp = make_inputs(CASES[name]) if name in CASES else EXTRA[name]
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ierr, info, coef, N, rhs, got, plan = _fit_ne(inp, refine=0)
        for k in env:
            monkeypatch.delenv(k)
        try:
            assert ierr == 0 and got == code, (name, got)
            x, rc, mp = plan.debug_solve(N, rhs)
        finally:
            plan.close()
        assert rc == 0
        res = np.asarray(rhs.astype(np.longdouble) - stencil_matvec(N, inp["nodes"], x), dtype=np.float64)
        bwd = float(np.max(np.abs(res)) / (stencil_norm_inf(N, inp["nodes"]) * np.max(np.abs(x)) + np.max(np.abs(rhs))))
        print(f"{label} {name}: backward error {bwd:.2e} (bound {BWD_TOL:.0e}); unrefined fit == debug solve: {np.array_equal(coef, x)}")
        assert bwd <= BWD_TOL, (label, name)
        assert np.array_equal(coef, x), (label, name)


def _indefinite_at(N, col):
    M = N.copy()
    M[col, -1] = -abs(M[col, -1])
    return M


def _check_107_then_good(plan, nodes, cols, label):
    N = synthetic_spd(nodes, 5)
    b = np.ones(N.shape[0])
    for where, col in cols:
        x, rc, _ = plan.debug_solve(_indefinite_at(N, int(col)), b)
        print(f"{label} {nodes}: negative pivot at column {int(col)} ({where}) -> {rc}")
        assert rc == 107 and not x.any(), (label, where)
    rc, err, _ = _solve_synthetic(plan, nodes, seed=6)
    print(f"{label} {nodes}: the same plan afterwards, forward error {err:.2e}")
    assert rc == 0 and err <= SPD_FWD_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("label,env,nodes,code", [("band", {"SPLPAK_ND": "0", "SPLPAK_NO_TWOEND": "1"}, [9, 17, 13], 1),
                                                  ("band_pipeline", {"SPLPAK_ND": "0", "SPLPAK_NO_TWOEND": "1", "SPLPAK_NARROW_BW": "1"}, [64, 64], 0),
                                                  ("twoend", {"SPLPAK_ND": "0"}, [24, 40, 24], 2)])
def test_band_not_positive_definite_is_107(label, env, nodes, code, monkeypatch):
    ncol = int(np.prod(nodes))
    plan = _forced_plan(env, nodes, monkeypatch, code)
    try:
        _check_107_then_good(plan, nodes, [("first", 0), ("middle", ncol // 2), ("last", ncol - 1)], label)
    finally:
        plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nodes", [[9, 17, 13], [40, 7], [6, 6, 6, 6]])
def test_nd_not_positive_definite_is_107(nodes, monkeypatch):
    t = capi.debug_nd_fronts(nodes)
    nf = t["depth"].size
    leaf = int(np.argmax(t["depth"]))
    mids = [f for f in range(nf) if 0 < t["depth"][f] < t["depth"].max()]
    cols = [("leaf front", np.nonzero(t["front_of"] == leaf)[0][0])]
    if mids:
        cols.append(("mid-level separator", np.nonzero(t["front_of"] == mids[len(mids) // 2])[0][-1]))
    root = np.nonzero(t["front_of"] == nf - 1)[0]
    cols.append(("first own column of the root", root[np.argmin(t["pos"][root])]))
    cols.append(("last own column of the root", root[np.argmax(t["pos"][root])]))
    plan = _forced_plan({"SPLPAK_ND": "1"}, nodes, monkeypatch, 4)
    try:
        _check_107_then_good(plan, nodes, cols, "nd")
    finally:
        plan.close()
