"""Nested-dissection multifrontal factorisation (csrc/ndtree.hip, csrc/ndchol.hip and the csrc/nd*.hip beside it).

CPU tier: the elimination tree is host code -- its invariants (every node owned once, every entry of the
7^d-stencil normal equations has a row in its column's front, monotone child -> parent maps) are checked
without a GPU, and so is what it promises for BASELINE's grids (flops, bytes).
GPU tier: the fit through that factorisation against the reference goldens, the band factorisation, the
independent banded CPU solve, and itself (bitwise run-to-run)."""
import os

import numpy as np
import pytest

from splpak_amd import capi
from tests.cases import CASES, make_inputs
from tests.conftest import load_golden, relmax

COEF_TOL = 1e-10


@pytest.mark.parametrize("nodes", [[8, 8, 8], [12, 12, 12], [16, 16, 16], [9, 17, 13], [64, 64], [40, 7], [6, 6, 6, 6],
                                   [8, 9, 10, 11], [33], [24, 24, 24], [5, 30, 5]])
def test_tree_invariants(nodes):
    t = capi.debug_nd_tree(nodes, check=True)
    n = int(np.prod(nodes))
    assert t["own_rows"] >= n and t["fronts"] >= 1
    assert t["flop_exact"] > 0


@pytest.mark.parametrize("split", [5, 6, 8, 11])
def test_tree_invariants_other_leaf_sizes(split):
    capi.debug_nd_tree([20, 20, 20], split_min=split, check=True)
    capi.debug_nd_tree([9, 9, 9, 9], split_min=split, check=True)


def test_tree_promises_for_the_baseline_grids():
    """BASELINE config 3 (64^3): at most a third of the band's n p^2 = 4.1e13 flop and under 20 GB of factor;
    4-D 24^4: under half of the band's 6.2e14 flop."""
    t = capi.debug_nd_tree([64, 64, 64], check=True)
    assert t["flop"] < 4.1e13 / 3 and t["factor_bytes"] < 20e9 and t["max_separator"] == 3 * 64 * 64
    t4 = capi.debug_nd_tree([24, 24, 24, 24], check=False)
    assert t4["flop"] < 6.2e14 / 2


@pytest.mark.parametrize("nodes", [[16, 16, 16], [9, 17, 13], [64, 64], [150, 130], [8, 9, 10, 11], [24, 40, 24], [5, 30, 5], [33]])
def test_schedule_invariants(nodes):
    """Round 5 (csrc/ndtree.hpp NdSchedule): for every cut depth the schedule eliminates children before parents and no two
    Schur buffers that are alive at the same time share a place in the arena (verified inside splpak_debug_nd_schedule);
    cut = 0 with square buffers is exactly the two depth-parity arenas of rounds 3-4, and packing halves it."""
    tree = capi.debug_nd_tree(nodes, check=False)
    level = capi.debug_nd_schedule(nodes, cut=0, packed=False)
    assert level["stages"] == int(tree["depth"]) + 1
    assert level["arena_bytes"] == tree["arena_bytes"]
    for cut in range(0, int(tree["depth"]) + 2):
        for packed in (False, True):
            sc = capi.debug_nd_schedule(nodes, cut=cut, packed=packed)
            assert sc["stages"] >= level["stages"] and sc["factor_bytes"] == tree["factor_bytes"]
            if packed and tree["arena_bytes"] > 0:          # (borders of a few tiles gain less than half: whole 64 x 64 tiles on the diagonal)
                sq = capi.debug_nd_schedule(nodes, cut=cut, packed=False)["arena_bytes"]
                assert sc["arena_bytes"] <= (0.62 if tree["max_border"] >= 2048 else 1.0) * sq + 4096


def test_schedule_makes_the_4d_28_grid_fit_one_gpu_and_says_why_32_does_not():
    """VERDICT r04 #1.  MI355X: 288 GiB = 309 GB of HBM.  With the level-by-level order of rounds 3-4 the 4-D 28^4 grid needed
    205 GB of panels + 326 GB of Schur arenas; in postorder with packed buffers the arena is ~60 GB and the fit runs on one GPU
    (tests/test_gpu_parity.py).  BASELINE config 5's own 32^4 grid: 476 GB of panels + ~131 GB of arena = twice the HBM; the
    GPU boxes of this pool give a job 322 GB of host memory (cgroup memory.max, tools/host_probe.py), less than the >= 330 GB an
    out-of-core factorisation would have to park there -- it stays an 8-GPU problem (test_multi_gpu_partition_of_the_4d_32_grid...)."""
    hbm = 288 * 2.0**30
    t28 = capi.debug_nd_tree([28] * 4, check=False)
    assert t28["factor_bytes"] + t28["arena_bytes"] > 1.5 * hbm
    best28 = min(capi.debug_nd_schedule([28] * 4, cut=c)["arena_bytes"] for c in range(0, 5))
    assert best28 < 66e9 and t28["factor_bytes"] + best28 + 20e9 < hbm
    t32 = capi.debug_nd_tree([32] * 4, check=False)
    best32 = min(capi.debug_nd_schedule([32] * 4, cut=c)["arena_bytes"] for c in range(0, 5))
    assert t32["factor_bytes"] > 1.5 * hbm and 120e9 < best32 < 140e9
    assert t32["factor_bytes"] + best32 - hbm > 290e9      # what would have to live in host memory: more than the box's cgroup allows with anything else
    # 64^3 (BASELINE configs 3 / 4): the level-by-level order stays (largest batches); packed buffers halve its arena
    assert capi.debug_nd_schedule([64] * 3, cut=0)["arena_bytes"] < 8.2e9


def test_tree_rejects_bad_grids_like_the_fit():
    with pytest.raises(capi.SplpakError):
        capi.debug_nd_tree([3, 8])


@pytest.fixture(autouse=True)
def _factorisation_only(monkeypatch):
    """These tests are about the FACTORISATION: since round 6 a large 4-D grid left to itself tries the iterative solve first
    (csrc/pcg.hip; tests/test_pcg.py) -- not here."""
    monkeypatch.setenv("SPLPAK_SOLVER", "direct")


# ---------------------------------------------------------------------------------------------------------------
def _fit_env(inp, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return capi.fit(inp["ndim"], inp["xdata"], inp["ydata"], inp["wdata"], inp["xmin"], inp["xmax"],
                        inp["nodes"], inp["xtrap"], want_hist=False)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


ND_GOLDENS = ["3d12", "3d16", "2d64_c2grid", "4d6", "3d8", "3d8_sparse", "3d8_cc_clust", "3d_aniso", "2d32", "2d16_outside",
              "2d_aniso_box", "4d5_cc", "c1_1d16", "4d4"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ND_GOLDENS)
def test_nd_fit_matches_golden_and_band(name):
    """The nested-dissection factorisation forced onto grids the reference covers (trees of 1 .. 127 fronts,
    1-D .. 4-D, constraint rows, zero weights): the golden at 1e-10, the band factorisation at 1e-12, the same
    row counts and residual norm."""
    gold = load_golden(name)
    inp = make_inputs(CASES[name])
    c_nd, e_nd, _, i_nd = _fit_env(inp, {"SPLPAK_ND": "1"})
    c_bd, e_bd, _, i_bd = _fit_env(inp, {"SPLPAK_ND": "0"})
    assert e_nd == 0 and e_bd == 0
    err = relmax(c_nd, gold["coef"])
    print(f"{name}: ND vs golden {err:.2e}, vs band {relmax(c_nd, c_bd):.2e}, steps {i_nd[2]:.0f}, optimality {i_nd[9]:.1e}")
    assert err < COEF_TOL
    assert relmax(c_nd, c_bd) < 1e-12
    assert i_nd[9] < 1e-9
    assert i_nd[0] == i_bd[0] and i_nd[1] == i_bd[1]
    assert abs(i_nd[8] - i_bd[8]) <= 1e-9 * max(i_bd[8], 1e-300)


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["5", "6", "11"])
def test_nd_other_leaf_sizes_match_golden(split):
    for name in ("3d12", "4d6", "2d32"):
        gold = load_golden(name)
        c, e, _, info = _fit_env(make_inputs(CASES[name]), {"SPLPAK_ND": "1", "SPLPAK_ND_SPLIT": split})
        assert e == 0 and relmax(c, gold["coef"]) < COEF_TOL, (name, split)


@pytest.mark.gpu
def test_nd_is_bitwise_reproducible_and_serial_equals_overlapped():
    """Every sum of the factorisation has one owner and a fixed order (children add into their parent slot 0
    first, then slot 1): two fits give identical bits, and so does the fit without stream overlap."""
    inp = make_inputs(CASES["3d16"])
    a = _fit_env(inp, {"SPLPAK_ND": "1"})[0]
    b = _fit_env(inp, {"SPLPAK_ND": "1"})[0]
    c = _fit_env(inp, {"SPLPAK_ND": "1", "SPLPAK_NO_LOOKAHEAD": "1"})[0]
    assert np.array_equal(a, b) and np.array_equal(a, c)


@pytest.mark.gpu
def test_nd_singular_system_is_107():
    """No smoothing rows and fewer points than coefficients in part of the grid: a pivot fails somewhere in the
    tree (or the row count already says so) -> 107 like the band path, never garbage with ierror 0."""
    from splpak_amd.synth import synth_points
    nd, nod = 3, 12
    x, y, w = synth_points(nd, 3000)
    x = x * 0.5                                  # an empty half of the box: columns without data
    c, e, _, info = _fit_env(dict(ndim=nd, xdata=x, ydata=y, wdata=w, xmin=[0.0] * nd, xmax=[1.0] * nd, nodes=[nod] * nd,
                                  xtrap=0.0), {"SPLPAK_ND": "1"})
    assert e == 107


@pytest.mark.gpu
@pytest.mark.parametrize("nod,m", [(24, 100000), (32, 150000)])
def test_nd_matches_banded_cpu_beyond_the_dense_oracle(port, nod, m):
    """24^3 / 32^3 with weights and derivative-constraint rows through the nested-dissection path, against the
    independent CPU solve of the reference's rows (oracle/splpak_banded.c, pinned to the goldens)."""
    from splpak_amd.synth import synth_points
    nd = 3
    x, y, w = synth_points(nd, m)
    lo, hi, nodes = [0.0] * nd, [1.0] * nd, [nod] * nd
    c0, e0, i0 = port.fit_banded(nd, x, y, w, lo, hi, nodes, 1.0)
    c1, e1, _, i1 = _fit_env(dict(ndim=nd, xdata=x, ydata=y, wdata=w, xmin=lo, xmax=hi, nodes=nodes, xtrap=1.0), {"SPLPAK_ND": "1"})
    assert e0 == e1 == 0
    print(f"{nod}^3 ND: vs banded CPU rel={relmax(c1, c0):.2e}; rows {i1[0]:.0f}+{i1[1]:.0f}; fit {i1[5] + i1[6] + i1[7]:.4f} s")
    assert relmax(c1, c0) < COEF_TOL
    assert i1[0] == i0[0] and i1[1] == i0[1]
    assert abs(i1[8] - i0[8]) <= 1e-9 * i0[8]


@pytest.mark.gpu
def test_nd_4d_24_random_spline_recovery():
    """4-D, 24^4 = 331 776 columns (BASELINE config 5's dimension count at the largest size whose fronts fit one
    288 GB GPU next to their Schur arenas: 76 + 132 GB; the 32^4 grid itself needs 476 GB of factor alone,
    tests/test_gpu_parity.py::test_grid_beyond_one_gpu_is_a_clean_error).  Data sampled from a spline of the grid
    with RANDOM coefficients, xtrap = 0: the fit is a projection and must give the coefficients back to 1e-10;
    fresh queries (also outside the box) agree; the measured optimality residual is at rounding level."""
    import time
    import torch
    capi.shutdown()
    torch.cuda.empty_cache()
    nd, nod, m = 4, 24, 4_000_000
    nodes, lo, hi = [nod] * nd, [0.0] * nd, [1.0] * nd
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    x = torch.empty((m, nd), dtype=torch.float64, device=dev)
    capi.synth_points_dev(nd, 0, m, x, None, None, st)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    ctrue = torch.randn(nod ** nd, dtype=torch.float64, device=dev, generator=gen)
    y = torch.empty(m, dtype=torch.float64, device=dev)
    capi.evaluate_dev(nd, x, None, ctrue, lo, hi, nodes, y, st)
    t0 = time.perf_counter()
    plan = capi.Plan(nd, nodes, lo, hi, 0.0, m)
    t1 = time.perf_counter()
    try:
        coef = torch.zeros(nod ** nd, dtype=torch.float64, device=dev)
        ierr, info = plan.fit(x, y, None, coef, st)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert ierr == 0
        err = float((coef - ctrue).abs().max() / ctrue.abs().max())
        print(f"24^4 projection: plan {t1 - t0:.1f} s, fit {t2 - t1:.2f} s (assembly {info[5]:.2f}, factorisation {info[6]:.2f}, "
              f"solve {info[7]:.2f}); coefficient error {err:.2e}, steps {info[2]:.0f}, optimality {info[9]:.1e}")
        assert info[0] == m
        assert err < COEF_TOL
        assert info[9] < 1e-9
        q = torch.rand((50000, nd), dtype=torch.float64, device=dev, generator=gen) * 1.2 - 0.1
        v1 = torch.empty(q.shape[0], dtype=torch.float64, device=dev)
        v2 = torch.empty_like(v1)
        capi.evaluate_dev(nd, q, None, coef, lo, hi, nodes, v1, st)
        capi.evaluate_dev(nd, q, None, ctrue, lo, hi, nodes, v2, st)
        torch.cuda.synchronize()
        assert float((v1 - v2).abs().max() / v2.abs().max()) < 1e-10
    finally:
        plan.close()


@pytest.mark.gpu
def test_nd_4d_28_the_largest_grid_one_gpu_holds(port):
    """BASELINE config 5's fit half (4-D, 1e7 points) at the largest grid ONE MI355X holds since round 5:
    28^4 = 614 656 columns, 1.1e15 flop, 205 GB of factor panels.  The level-by-level order of rounds 3-4 needed 326 GB of Schur
    arenas on top (refused); the postorder schedule with packed Schur buffers (csrc/ndtree.hpp NdSchedule) needs ~63 GB.
    (a) 1e7 points sampled from a spline with RANDOM coefficients, xtrap = 0: the fit is a projection, the coefficients come
    back to 1e-10 and the measured backward error is at rounding level; (b) the seeded WEIGHTED workload with xtrap = 1 and its
    ~1e6 derivative-constraint rows: the HOST-side componentwise backward error over the reference's rows
    (oracle_rows_gradient, src/splpak.F90:788-855, :862-1046) < 1e-12, row counts and reserr as the GPU reports them.
    Config 5's own 32^4 grid (476 GB of panels) stays refused on one GPU: test_gpu_parity.py::test_grid_beyond_one_gpu_is_a_clean_error."""
    import time
    import torch
    capi.shutdown()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if total < 300e9:
        pytest.skip(f"needs a 288 GiB device, this one has {total / 1e9:.0f} GB")
    # (a fresh box -- the driver's lease -- has 308 of 309 GB free; a busier one must not drop config 5's only full-pipeline
    #  factorised 4-D check silently: round-5 verdict)
    assert free >= 285e9, f"needs ~280 GB of free device memory, only {free / 1e9:.0f} of {total / 1e9:.0f} GB are free: something else holds the device"
    nd, nod, m = 4, 28, 10_000_000
    nodes, lo, hi = [nod] * nd, [0.0] * nd, [1.0] * nd
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    x = torch.empty((m, nd), dtype=torch.float64, device=dev)
    ys = torch.empty(m, dtype=torch.float64, device=dev)
    ws = torch.empty(m, dtype=torch.float64, device=dev)
    capi.synth_points_dev(nd, 0, m, x, ys, ws, st)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    ctrue = torch.randn(nod ** nd, dtype=torch.float64, device=dev, generator=gen)
    y = torch.empty(m, dtype=torch.float64, device=dev)
    capi.evaluate_dev(nd, x, None, ctrue, lo, hi, nodes, y, st)
    coef = torch.zeros(nod ** nd, dtype=torch.float64, device=dev)
    t0 = time.perf_counter()
    plan = capi.Plan(nd, nodes, lo, hi, 0.0, m)
    try:
        code, what = plan.factorisation()
        assert code == 4 and "packed" in what and "cut 0" not in what, what
        ierr, info = plan.fit(x, y, None, coef, st)
        torch.cuda.synchronize()
        err = float((coef - ctrue).abs().max() / ctrue.abs().max())
        print(f"28^4 projection: {what}; plan + fit {time.perf_counter() - t0:.1f} s (assembly {info[5]:.2f}, factorisation {info[6]:.2f}, "
              f"solve {info[7]:.2f}); coefficient error {err:.2e}, steps {info[2]:.0f}, backward error {info[9]:.1e}")
        assert ierr == 0 and info[0] == m
        assert err < COEF_TOL and info[9] < 1e-9
    finally:
        plan.close()
    del ctrue, y
    plan = capi.Plan(nd, nodes, lo, hi, 1.0, m)
    try:
        ierr, info = plan.fit(x, ys, ws, coef, st)
        torch.cuda.synchronize()
        c = coef.cpu().numpy()
    finally:
        plan.close()
    assert ierr == 0 and info[9] < 1e-9
    omega, reserr, nrow, ncons = port.rows_gradient(nd, x.cpu().numpy(), ys.cpu().numpy(), ws.cpu().numpy(), lo, hi, nodes, 1.0, c)
    print(f"28^4 weighted: host backward error {omega:.2e} (GPU's own: {info[9]:.2e}); rows {nrow}+{ncons} (GPU {info[0]:.0f}+{info[1]:.0f}); "
          f"reserr host {reserr:.9e} GPU {info[8]:.9e}")
    assert omega < 1e-12
    assert nrow == info[0] == m and ncons == info[1] and ncons > 100000
    assert abs(reserr - info[8]) <= 1e-9 * reserr
    # round 6: the iterative solve (csrc/pcg.hip) on the same rows, without any factorisation, agrees to 1e-10
    os.environ["SPLPAK_SOLVER"] = "pcg"
    try:
        plan = capi.Plan(nd, nodes, lo, hi, 1.0, m)
    finally:
        os.environ.pop("SPLPAK_SOLVER", None)
    try:
        assert plan.factorisation()[0] == 6
        t0 = time.perf_counter()
        ierr, info_it = plan.fit(x, ys, ws, coef, st)
        torch.cuda.synchronize()
        t_it = time.perf_counter() - t0
        ps = plan.pcg_stats()
        c_it = coef.cpu().numpy()
    finally:
        plan.close()
    err = float(np.abs(c_it - c).max() / np.abs(c).max())
    print(f"28^4 weighted, iteration alone: {t_it:.2f} s, {ps['iterations']} iterations in {ps['solves']} solves; {err:.2e} from the factorisation's coefficients; "
          f"backward error {info_it[9]:.1e}")
    # 28^4 with 1e7 points: 18.8 points per grid cell, 17 % of the nodes data sparse -- below the density of constraint rows at which
    # the separable preconditioner works (config 5's 32^4: 10.8 points per cell, 26 %).  Either outcome is
    # legitimate, a silently wrong answer is not: agreement at 1e-10, or the reference's 107 with the library's explanation.
    assert ierr in (0, 107)
    if ierr == 0:
        assert err < COEF_TOL and info_it[9] < 1e-9
        assert info_it[0] == info[0] and info_it[1] == info[1]
    else:
        assert "iterative solve did not converge" in capi.last_error() and not c_it.any()


@pytest.mark.gpu
def test_nd_pinned_queue_lookahead_variants_are_bitwise_equal():
    """32^3 (root separator 3 072 columns = 12 block steps): the diagonal blocks of the upper levels are factored on
    reserved CUs while the update waves take their items from a queue and step aside there, and the root's panel
    update is split for look-ahead.  The last Schur pass of every front adds its result into the parent itself.  None of that may
    change a bit: the same fit without reserved CUs, without the root look-ahead, with K = 256 Schur passes, with separate
    extend-add launches and entirely serial gives identical coefficients.  Round 5: so do the POSTORDER schedules (the fronts
    above depth SPLPAK_ND_CUT one by one, the subtrees below one after the other, Schur buffers reused along the way --
    csrc/ndtree.hpp NdSchedule) and square instead of packed Schur buffers (SPLPAK_ND_SQUARE); and so does the way the panels
    come to hold the normal equations: written column by column, zeros and entries, when their stage comes alive (nd_init_kernel)
    or cleared as a whole (by the runtime's memset or by resident workgroups) and scattered into."""
    from splpak_amd.synth import synth_points
    nd, nod, m = 3, 32, 200000
    x, y, w = synth_points(nd, m)
    inp = dict(ndim=nd, xdata=x, ydata=y, wdata=w, xmin=[0.0] * nd, xmax=[1.0] * nd, nodes=[nod] * nd, xtrap=1.0)
    ref, e, _, info = _fit_env(inp, {"SPLPAK_ND": "1"})
    assert e == 0 and info[9] < 1e-9
    for env in ({"SPLPAK_NO_PANEL_CU": "1"}, {"SPLPAK_ND_NO_ROOT_LOOKAHEAD": "1"}, {"SPLPAK_ND_KB": "1"}, {"SPLPAK_ND_NO_FUSE": "1"},
                {"SPLPAK_ND_CUT": "1"}, {"SPLPAK_ND_CUT": "2"}, {"SPLPAK_ND_CUT": "3", "SPLPAK_NO_LOOKAHEAD": "1"}, {"SPLPAK_ND_CUT": "4", "SPLPAK_ND_SQUARE": "1"},
                {"SPLPAK_ND_CUT": "6"}, {"SPLPAK_ND_CUT": "2", "SPLPAK_ND_NO_FUSE": "1"}, {"SPLPAK_ND_SQUARE": "1"}, {"SPLPAK_ND_NO_OUTER": "1"}, {"SPLPAK_ND_SMALL_GRID": "0"}, {"SPLPAK_ND_WG4": "2"}, {"SPLPAK_ND_POTRF_WAVES": "4"}, {"SPLPAK_ND_POTRF_WAVES": "16"}, {"SPLPAK_ND_SMALL_QUEUE": "1"}, {"SPLPAK_ND_FULL_DIAG": "1"}, {"SPLPAK_ND_XCD": "0"},
                {"SPLPAK_ND_NO_FUSE": "1", "SPLPAK_ND_SQUARE": "1", "SPLPAK_ND_KB": "2"},
                {"SPLPAK_NO_LOOKAHEAD": "1"}, {"SPLPAK_ND_RES_CUS": "3", "SPLPAK_ND_PIN_ROUNDS": "8"}, {"SPLPAK_ND_PIN_FIRST": "1", "SPLPAK_ND_PIN_ROUNDS": "2"}, {"SPLPAK_ND_PREP_EARLY": "1"}, {"SPLPAK_ND_CHAIN_LA": "0"}, {"SPLPAK_ND_CHAIN_LA": "64"},
                # the panels written stage by stage (nd_init_kernel, the default) | cleared as a whole, then scattered into
                {"SPLPAK_ND_STAGED_INIT": "0"}, {"SPLPAK_ND_STAGED_INIT": "0", "SPLPAK_ND_CLEAR_WGS": "0"}, {"SPLPAK_ND_STAGED_INIT": "0", "SPLPAK_ND_NO_EARLY_CLEAR": "1"},
                {"SPLPAK_ND_STAGED_INIT": "0", "SPLPAK_ND_CUT": "2"},
                # the root's look-ahead over the next diagonal block only (round 4)
                {"SPLPAK_ND_ROOT_LA": "1"},
                # round 6: the upper depths as two interleaved half-stages (the root's two subtrees); off
                {"SPLPAK_ND_HALVES": "0"}, {"SPLPAK_ND_HALVES": "1"}, {"SPLPAK_ND_HALVES": "9"}, {"SPLPAK_ND_HALVES": "2", "SPLPAK_NO_LOOKAHEAD": "1"},
                {"SPLPAK_ND_HALVES": "3", "SPLPAK_ND_NO_FUSE": "1"}, {"SPLPAK_ND_HALVES": "9", "SPLPAK_ND_SQUARE": "1"}):
        c, e, _, _ = _fit_env(inp, dict(env, SPLPAK_ND="1"))
        assert e == 0 and np.array_equal(c, ref), env


@pytest.mark.gpu
def test_nd_schedule_variants_on_an_anisotropic_grid():
    """Round-5 advice: the isotropic 32^3 grid of the variants test has no stage whose fronts differ in their number of block steps,
    so neither the look-ahead inside the chain's groups nor the order of the extend-adds under different schedule cuts was ever
    exercised with mixed fronts.  A 24 x 40 x 24 box has them.  Variants that only re-time the same operations must return the same
    bits; a different schedule CUT may add two siblings into their parent in the other order -- the header promises run-to-run
    reproducibility for the same cut only (include/splpak_hip.h) -- so across cuts the bar is rounding level, and the test says which
    it was."""
    from splpak_amd.synth import synth_points
    nd, nodes, m = 3, [24, 40, 24], 150000
    x, y, w = synth_points(nd, m)
    inp = dict(ndim=nd, xdata=x, ydata=y, wdata=w, xmin=[0.0] * nd, xmax=[1.0] * nd, nodes=nodes, xtrap=1.0)
    ref, e, _, info = _fit_env(inp, {"SPLPAK_ND": "1", "SPLPAK_ND_CUT": "0"})
    assert e == 0 and info[9] < 1e-9
    for env in ({"SPLPAK_ND_CHAIN_LA": "0"}, {"SPLPAK_ND_CHAIN_LA": "64"}, {"SPLPAK_NO_LOOKAHEAD": "1"}, {"SPLPAK_ND_KB": "2"}, {"SPLPAK_ND_NO_FUSE": "1"},
                {"SPLPAK_NO_PANEL_CU": "1"}, {"SPLPAK_ND_PREP_EARLY": "1"}, {"SPLPAK_ND_PIN_FIRST": "1", "SPLPAK_ND_PIN_ROUNDS": "2"},
                {"SPLPAK_ND_HALVES": "0"}, {"SPLPAK_ND_HALVES": "2"}, {"SPLPAK_ND_HALVES": "9"}):
        c, e, _, _ = _fit_env(inp, dict(env, SPLPAK_ND="1", SPLPAK_ND_CUT="0"))
        assert e == 0 and np.array_equal(c, ref), env
    again, e, _, _ = _fit_env(inp, {"SPLPAK_ND": "1", "SPLPAK_ND_CUT": "0", "SPLPAK_NO_PLAN_CACHE": "1"})
    assert e == 0 and np.array_equal(again, ref)
    for cut in ("1", "2", "4"):
        c, e, _, _ = _fit_env(inp, {"SPLPAK_ND": "1", "SPLPAK_ND_CUT": cut})
        assert e == 0
        d = relmax(c, ref)
        print(f"24 x 40 x 24, schedule cut {cut} against cut 0: {'same bits' if np.array_equal(c, ref) else f'{d:.1e} apart'}")
        assert d < 1e-12


def test_multi_gpu_partition_of_the_4d_32_grid_fits_eight_gpus():
    """BASELINE config 5's 4-D 32^4 grid does not fit one 288 GB GPU by any route (476 GB of panels); the
    one-process multi-GPU fit distributes the nested-dissection factorisation -- subtrees per GPU, the fronts above them by
    block columns (csrc/ndtree.hpp NdPartition).  Host-only: per rank, everything the factorisation keeps + the all-reduced
    normal equations + the Gram scratch + the binned points of its shard must stay below the GPU's memory."""
    ranks, summ = capi.debug_nd_partition([32] * 4, 8)
    assert summ["dcut"] == 3 and summ["top_fronts"] == 7
    hbm = 288e9
    points = 1.25e6 * (8 * 5 + 8 * 6 + 8)          # a shard of config 5's 1e7 points: caller's arrays + sorted copies + keys
    gram_scratch = 8.6e9                           # slabs of per-cell Gram blocks (plan.hip: at most 8 GiB)
    worst = 0.0
    for r in ranks:
        assert abs(r["bytes"] - (r["panel_bytes"] + r["schur_bytes"] + r["top_bytes"] + r["inverse_bytes"] + r["other_bytes"])) < 1.0
        total = r["bytes"] + summ["normal_eq_bytes"] * 1.3 + gram_scratch + points      # (x 1.3: reduction staging, residual shares)
        worst = max(worst, total)
    print(f"32^4 on 8 GPUs: {min(r['bytes'] for r in ranks) / 1e9:.0f} - {max(r['bytes'] for r in ranks) / 1e9:.0f} GB of factorisation "
          f"per GPU, {worst / 1e9:.0f} GB in all on the fullest; flop per GPU {max(r['flop_subtrees'] + r['flop_top'] for r in ranks):.2e}")
    assert worst < 0.9 * hbm
    # the work is spread: no rank does more than 1.3 x the mean
    fl = [r["flop_subtrees"] + r["flop_top"] for r in ranks]
    assert max(fl) < 1.3 * sum(fl) / len(fl)
    # on FOUR GPUs it does not fit (the test has teeth), on one rank the partition is the whole tree
    ranks4, _ = capi.debug_nd_partition([32] * 4, 4)
    assert max(r["bytes"] for r in ranks4) > hbm
    one, s1 = capi.debug_nd_partition([24] * 4, 1)
    tree = capi.debug_nd_tree([24] * 4, check=False)
    assert s1["dcut"] == 0 and s1["top_fronts"] == 0
    assert one[0]["panel_bytes"] == tree["factor_bytes"] and one[0]["schur_bytes"] == tree["arena_bytes"]


@pytest.mark.parametrize("nodes,R", [([64] * 3, 8), ([64] * 3, 3), ([24] * 4, 4), ([90, 90], 8)])
def test_multi_gpu_partition_memory_shrinks_with_the_ranks(nodes, R):
    ranks, summ = capi.debug_nd_partition(nodes, R)
    tree = capi.debug_nd_tree(nodes, check=False)
    whole = tree["factor_bytes"] + tree["arena_bytes"]
    fullest = max(r["panel_bytes"] + r["schur_bytes"] + r["top_bytes"] for r in ranks)
    assert fullest < 1.6 * whole / R + 3 * summ["max_panel_bytes"]
    assert abs(sum(r["flop_subtrees"] + r["flop_top"] for r in ranks) / tree["flop"] - 1.0) < 0.02
