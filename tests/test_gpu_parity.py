"""GPU: parity of the HIP path (through the C ABI) with the reference.

Checked against (a) golden vectors generated from the unmodified reference
(tests/golden/, oracle/gen_golden.py) and (b) the CPU oracle on fresh seeded
inputs.  Tolerance: 1e-10 max-norm relative on coefficients (BASELINE.json
north_star, real64); evaluation 1e-12 relative to the largest value.
"""
import os

import numpy as np
import pytest

from splpak_amd import capi
from tests.cases import CASES, make_inputs, make_queries, nderiv_patterns
from tests.conftest import ROOT, load_golden, relmax

pytestmark = pytest.mark.gpu

COEF_TOL = 1e-10
EVAL_TOL = 1e-12

ALL = list(CASES)


def test_device_is_gfx950():
    assert capi.device_name().startswith("gfx950")


# ---------------------------------------------------------------------------
# band Cholesky kernels in isolation (f64 MFMA trailing update, trsm, sweeps)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,halfbw", [(200, 199), (256, 40), (700, 699), (1000, 300), (1536, 257),
                                      (2048, 700)])
def test_band_cholesky_vs_lapack(n, halfbw):
    rng = np.random.default_rng(n + halfbw)
    i, j = np.indices((n, n))
    mask = np.abs(i - j) <= halfbw
    # asymmetric-looking random band made SPD by diagonal dominance
    a = rng.standard_normal((n, n)) * mask
    a = np.tril(a) + np.tril(a, -1).T
    a[np.diag_indices(n)] = np.abs(a).sum(axis=1) + 1.0 + rng.random(n)
    b = rng.standard_normal(n)
    x, rc = capi.debug_spd_band_solve(a, halfbw, b)
    assert rc == 0
    xref = np.linalg.solve(a, b)
    assert relmax(x, xref) < 1e-11
    # not positive definite -> 107
    a2 = a.copy()
    a2[n // 2, n // 2] = -1.0
    assert capi.debug_spd_band_solve(a2, halfbw, b)[1] == 107


@pytest.mark.parametrize("n,halfbw", [(1000, 50), (1024, 200), (2048, 255), (2100, 300), (3000, 257),
                                      (4096, 195), (5000, 700), (3300, 513)])
def test_two_ended_band_cholesky_vs_lapack(n, halfbw, monkeypatch):
    """The two-ended factorisation (csrc/twoend.hip: both ends eliminated at once, meeting in a separator of
    the band's width) on dense SPD band matrices: same answers as LAPACK and as the single chain; with and
    without padding columns, separators of 1..3 blocks, a failing pivot in either chain or in the separator."""
    rng = np.random.default_rng(7 * n + halfbw)
    i, j = np.indices((n, n))
    mask = np.abs(i - j) <= halfbw
    a = rng.standard_normal((n, n)) * mask
    a = np.tril(a) + np.tril(a, -1).T
    a[np.diag_indices(n)] = np.abs(a).sum(axis=1) + 1.0 + rng.random(n)
    b = rng.standard_normal(n)
    x1, rc1 = capi.debug_spd_band_solve(a, halfbw, b)
    monkeypatch.setenv("SPLPAK_DEBUG_TWOEND", "1")
    x2, rc2 = capi.debug_spd_band_solve(a, halfbw, b)
    assert rc1 == 0 and rc2 == 0
    xref = np.linalg.solve(a, b)
    assert relmax(x2, xref) < 1e-11
    assert relmax(x2, x1) < 1e-11
    for pos in (5, n // 2, n - 7):
        a2 = a.copy()
        a2[pos, pos] = -1.0
        assert capi.debug_spd_band_solve(a2, halfbw, b)[1] == 107


# ---------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_eval_matches_reference_golden(name):
    spec = CASES[name]
    gold = load_golden(name)
    inp = make_inputs(spec)
    q = make_queries(spec)
    for i, p in enumerate(nderiv_patterns(inp["ndim"])):
        v, ierr = capi.evaluate(inp["ndim"], q, p, gold["coef"], inp["xmin"], inp["xmax"], inp["nodes"])
        assert ierr == 0
        # scale: the size of the terms that are summed (|coef| * prod dxin^nderiv), so that
        # derivatives that cancel to ~0 (e.g. f'' of a fitted straight line) are judged fairly
        dxin = (np.array(spec["nodes"]) - 1) / (inp["xmax"] - inp["xmin"])
        scale = max(np.max(np.abs(gold["values"][i])),
                    np.max(np.abs(gold["coef"])) * float(np.prod(dxin ** np.array(p))))
        assert np.max(np.abs(v - gold["values"][i])) / scale < EVAL_TOL, (name, p)
    v0, ierr = capi.evaluate(inp["ndim"], q, None, gold["coef"], inp["xmin"], inp["xmax"], inp["nodes"])
    assert ierr == 0
    assert np.max(np.abs(v0 - gold["values"][0])) <= EVAL_TOL * max(np.max(np.abs(gold["values"][0])), 1e-300)


def test_eval_ragged_and_strided():
    gold = load_golden("3d8")
    inp = make_inputs(CASES["3d8"])
    q = make_queries(CASES["3d8"])
    # leading dimension larger than ndim (xq(ldxq, nq))
    qpad = np.zeros((q.shape[0], 5))
    qpad[:, :3] = q
    qpad[:, 3:] = 1e300
    v, _ = capi.evaluate(3, qpad, None, gold["coef"], inp["xmin"], inp["xmax"], inp["nodes"])
    assert np.max(np.abs(v - gold["values"][0])) <= EVAL_TOL * np.max(np.abs(gold["values"][0]))
    # a single query and an empty batch
    v1, _ = capi.evaluate(3, q[:1], None, gold["coef"], inp["xmin"], inp["xmax"], inp["nodes"])
    assert abs(v1[0] - gold["values"][0][0]) <= EVAL_TOL * np.max(np.abs(gold["values"][0]))
    v0, rc = capi.evaluate(3, np.zeros((0, 3)), None, gold["coef"], inp["xmin"], inp["xmax"], inp["nodes"])
    assert rc == 0 and v0.size == 0
    # nderiv out of range: 104, value still computed (clamped)
    v, rc = capi.evaluate(3, q, [3, 0, 0], gold["coef"], inp["xmin"], inp["xmax"], inp["nodes"])
    assert rc == 104 and np.all(np.isfinite(v))


R32 = ["2d8", "3d8", "4d4"]
EPS32 = float(np.finfo(np.float32).eps)


@pytest.mark.parametrize("name", R32)
def test_eval_real32_vs_real32_reference(name):
    """REAL32 evaluation against the reference compiled with -DREAL32 (src/splpak.F90:33-41;
    tests/golden/*_r32.npz, oracle/gen_golden.py --real32): same single-precision coefficients and
    queries, every nderiv pattern.  (a) the GPU's error against the real64 golden is no larger than
    the REAL32 reference's (x1.5), (b) both agree to single-precision rounding of the summed terms."""
    spec = CASES[name]
    g32, g64 = load_golden(name + "_r32"), load_golden(name)
    inp = make_inputs(spec)
    nd = inp["ndim"]
    q32 = make_queries(spec).astype(np.float32)
    dxin = (np.array(spec["nodes"]) - 1) / (inp["xmax"] - inp["xmin"])
    cmax = float(np.max(np.abs(g64["coef"])))
    for i, p in enumerate(nderiv_patterns(nd)):
        v, rc = capi.evaluate(nd, q32, p, g32["coef"], inp["xmin"], inp["xmax"], inp["nodes"], real32=True)
        assert rc == 0 and v.dtype == np.float32
        scale = max(float(np.max(np.abs(g64["values"][i]))), cmax * float(np.prod(dxin ** np.array(p))))
        err_gpu = np.max(np.abs(v.astype(np.float64) - g64["values"][i])) / scale
        err_ref = np.max(np.abs(g32["values"][i].astype(np.float64) - g64["values"][i])) / scale
        assert err_gpu <= 1.5 * err_ref + 4 * EPS32, (name, p, err_gpu, err_ref)
        # 4^d terms of size <= scale, each carrying a few single-precision roundings in the reference
        assert np.max(np.abs(v - g32["values"][i])) <= (4 ** nd) * 8 * EPS32 * scale, (name, p)


@pytest.mark.parametrize("name", R32)
def test_fit_real32_vs_real32_reference(name):
    """REAL32 fit (f32 storage, f64 arithmetic) on the inputs rounded to single precision: its error
    against the real64 golden must not exceed the REAL32 reference's own error (x1.5) -- the oracle of
    BASELINE config 5's real32-vs-real64 tolerance sweep."""
    spec = CASES[name]
    g32, g64 = load_golden(name + "_r32"), load_golden(name)
    inp = make_inputs(spec)
    f32 = lambda a: None if a is None else np.asarray(a, dtype=np.float32)
    coef, ierr, hist, _ = capi.fit(inp["ndim"], f32(inp["xdata"]), f32(inp["ydata"]), f32(inp["wdata"]),
                                   inp["xmin"], inp["xmax"], inp["nodes"], inp["xtrap"], real32=True,
                                   want_hist=True)
    assert ierr == 0 == int(g32["ierror"]) and coef.dtype == np.float32
    err_gpu = relmax(coef, g64["coef"])
    err_ref = relmax(g32["coef"], g64["coef"])
    print(f"{name}: real32 fit error vs real64 golden: GPU {err_gpu:.2e}, REAL32 reference {err_ref:.2e}")
    assert err_gpu <= 1.5 * err_ref + 4 * EPS32
    assert relmax(coef, g32["coef"]) <= 2.0 * err_ref + 4 * EPS32
    # the histogram is a sum of single-precision weights in the reference
    assert relmax(hist, g32["hist"]) <= 1e-4


@pytest.mark.parametrize("nodes", [(150, 70), (20, 17, 30), (12, 9, 8, 14), (64, 64)])
def test_eval_binned_path_is_bit_identical_to_direct(port, nodes):
    """The LDS-binned evaluation (queries sorted by grid region) must return the bits of the direct
    kernel, for every derivative pattern, with queries outside the grid, padded rows and a ragged
    last chunk; one pattern is also anchored to the reference algorithm (oracle)."""
    nd = len(nodes)
    rng = np.random.default_rng(nd * 1000 + nodes[0])
    coef = rng.standard_normal(int(np.prod(nodes)))
    lo = -1.0 + rng.random(nd)
    hi = lo + 1.0 + 3.0 * rng.random(nd)
    nq = 20011
    q = np.full((nq, nd + 1), 1e300)
    q[:, :nd] = lo + (hi - lo) * (-0.2 + 1.4 * rng.random((nq, nd)))     # ~30 % outside the grid
    q[:50, :nd] = lo + (hi - lo) * rng.integers(0, 2, (50, nd))            # corners / edges exactly
    try:
        for p in [None] + nderiv_patterns(nd):
            capi.set_eval_mode(capi.EVAL_DIRECT)
            vd, rc = capi.evaluate(nd, q, p, coef, lo, hi, nodes)
            assert rc == 0
            capi.set_eval_mode(capi.EVAL_BINNED, 4099)
            vb, rc = capi.evaluate(nd, q, p, coef, lo, hi, nodes)
            assert rc == 0
            assert np.array_equal(vd, vb), (nodes, p)
        capi.set_eval_mode(capi.EVAL_BINNED, 0)
        vb, _ = capi.evaluate(nd, q, None, coef, lo, hi, nodes)
        vo, _ = port.evaluate(nd, q[:2000], None, coef, lo, hi, nodes)
        assert np.max(np.abs(vb[:2000] - vo)) <= EVAL_TOL * np.max(np.abs(vo))
    finally:
        capi.set_eval_mode(capi.EVAL_AUTO)
    with pytest.raises(capi.SplpakError):
        capi.set_eval_mode(7)


@pytest.mark.parametrize("nodes", [(40, 40, 40), (20, 20, 20, 20)])
def test_eval_real32_binned_path_is_bit_identical_to_direct(nodes):
    """REAL32 storage (float queries, coefficients, results; double arithmetic) through the region sort: the bits of the
    REAL32 direct kernel, and the real64 values to single-precision rounding (BASELINE config 5's tolerance sweep runs
    its 1e8 queries through this path)."""
    import torch
    nd = len(nodes)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(17)
    nq = 400_000
    coef = torch.randn(int(np.prod(nodes)), dtype=torch.float64, device=dev, generator=gen)
    xq = torch.rand((nq, nd), dtype=torch.float64, device=dev, generator=gen) * 1.2 - 0.1
    c32, x32 = coef.float(), xq.float()
    lo, hi = [0.0] * nd, [1.0] * nd
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    try:
        for pat in (None, [1] + [0] * (nd - 1), [0] * (nd - 1) + [2]):
            for mode in (capi.EVAL_BINNED, capi.EVAL_DIRECT):
                capi.set_eval_mode(mode, 1 << 16)
                o = torch.empty(nq, dtype=torch.float32, device=dev)
                assert capi.evaluate_dev(nd, x32, pat, c32, lo, hi, nodes, o, st) == 0
                torch.cuda.synchronize()
                out[mode] = o
            assert torch.equal(out[capi.EVAL_BINNED], out[capi.EVAL_DIRECT]), (nodes, pat)
            o64 = torch.empty(nq, dtype=torch.float64, device=dev)
            capi.evaluate_dev(nd, x32.double(), pat, c32.double(), lo, hi, nodes, o64, st)
            torch.cuda.synchronize()
            scale = float(o64.abs().max())
            assert float((out[capi.EVAL_BINNED].double() - o64).abs().max()) <= 2e-7 * scale
    finally:
        capi.set_eval_mode(capi.EVAL_AUTO)


def test_eval_binned_scratch_regrows_for_a_grid_with_more_regions():
    """the binned path's per-workgroup count matrix was sized for the regions of whichever grid
    allocated it; a later grid with MORE regions and the same batch size wrote past it.  A 3-D 28^3 spline (8 regions),
    then 64^3 (125 regions), then a 4-D 24^4 one (625 regions) with the same number of queries and chunk, in one
    process: every batch must return the bits of the direct kernel."""
    rng = np.random.default_rng(321)
    nq = 300_000
    try:
        for nodes in ((28, 28, 28), (64, 64, 64), (24, 24, 24, 24), (16, 16, 16)):
            nd = len(nodes)
            coef = rng.standard_normal(int(np.prod(nodes)))
            q = -0.1 + 1.2 * rng.random((nq, nd))
            capi.set_eval_mode(capi.EVAL_BINNED, 1 << 17)
            vb, rc = capi.evaluate(nd, q, None, coef, [0.0] * nd, [1.0] * nd, nodes)
            assert rc == 0
            capi.set_eval_mode(capi.EVAL_DIRECT)
            vd, rc = capi.evaluate(nd, q, None, coef, [0.0] * nd, [1.0] * nd, nodes)
            assert rc == 0 and np.array_equal(vb, vd), nodes
    finally:
        capi.set_eval_mode(capi.EVAL_AUTO)


def test_eval_scratch_of_every_path_across_streams_regrowth_and_threads():
    """Every evaluation path keeps per-thread device scratch of its own (csrc/evalscratch.hpp): a call on another stream
    waits for the previous use, regrowing one path's scratch leaves the others' alone, and threads do not share it.
    One host thread, EVAL_BINNED forced, the calls alternating between two streams with no synchronisation in between;
    every call must return the bits of the direct kernel.  Which path takes a grid follows from the code:
      1. 2-D (20, 20): the region sort (2-D has no other path; one region).
      2. 3-D (7, 20, 20): make_pregions refuses nodes < 8; make_regions gives 1 x 2 x 2 = 4 <= 256 regions: the run path.
      3. 3-D (19, 19, 19): 16 window starts per dimension are ONE region at 16 per region (< 8 regions: refused) and
         2 x 2 x 2 = 8 at 8 per region: the persistent path.
      4. 4-D (19, 19, 19, 11): 2 x 2 x 2 x 1 = 8 regions of 8 window starts: the persistent 4-D path.
      5. the grid route on 9 x 10 x 11 points of (19, 19, 19), against the point route.
      6. case 1 with 40 000 queries in chunks of 4 099 (ten chunks, a ragged last one: these still fit the buffers of call
         1, which held 5 000 queries), then in ONE chunk, which regrows the sort scratch.
      7. cases 2 and 3 again: their scratch was not touched by the regrowth.
    At the end a second Python thread runs case 3 with scratch of its own."""
    import threading
    import torch
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2024)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]

    def make(nodes, nq):
        nd = len(nodes)
        coef = torch.randn(int(np.prod(nodes)), dtype=torch.float64, device=dev, generator=gen)
        xq = torch.rand((nq, nd), dtype=torch.float64, device=dev, generator=gen) * 1.2 - 0.1      # ~30 % outside the grid
        return nodes, coef, xq

    c1, c2, c3, c4 = make((20, 20), 5000), make((7, 20, 20), 5000), make((19, 19, 19), 5000), make((19, 19, 19, 11), 5000)
    c6 = (c1[0], c1[1], make(c1[0], 40_000)[2])
    axes = [torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * 1.2 - 0.1 for n in (9, 10, 11)]
    g2, g1, g0 = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    grid_points = torch.stack([g0, g1, g2], dim=-1).reshape(-1, 3).contiguous()
    torch.cuda.synchronize()
    pending = []          # (what, binned / grid result, direct result)
    turn = [0]

    def point(case, mode, chunk=0, stream=None):
        nodes, coef, xq = case
        nd = len(nodes)
        if stream is None:
            stream = streams[turn[0] % 2]
            turn[0] += 1
        out = torch.empty(xq.shape[0], dtype=torch.float64, device=dev)
        capi.set_eval_mode(mode, chunk)
        assert capi.evaluate_dev(nd, xq, None, coef, [0.0] * nd, [1.0] * nd, nodes, out, stream.cuda_stream) == 0
        return out

    def both(what, case, chunk=0):
        pending.append((what, point(case, capi.EVAL_BINNED, chunk), point(case, capi.EVAL_DIRECT)))

    try:
        both("1 sort", c1)
        both("2 runs", c2)
        both("3 persistent", c3)
        both("4 persistent 4-D", c4)
        gout = torch.empty(9 * 10 * 11, dtype=torch.float64, device=dev)
        st = streams[turn[0] % 2]
        turn[0] += 1
        assert capi.evaluate_grid_dev(3, [9, 10, 11], torch.cat(axes), None, c3[1], [0.0] * 3, [1.0] * 3, c3[0], gout, st.cuda_stream) == 0
        pending.append(("5 grid", gout, point((c3[0], c3[1], grid_points), capi.EVAL_DIRECT)))
        both("6 sort, chunks of 4099", c6, 4099)
        both("6 sort, regrown", c6)
        both("7 runs again", c2)
        both("7 persistent again", c3)
        torch.cuda.synchronize()
        for what, a, b in pending:
            assert torch.equal(a, b), what
        result = []

        def other_thread():
            try:
                torch.cuda.set_device(0)
                st2 = torch.cuda.Stream(device=dev)
                a = point(c3, capi.EVAL_BINNED, stream=st2)
                b = point(c3, capi.EVAL_DIRECT, stream=st2)
                st2.synchronize()
                result.append(bool(torch.equal(a, b)) and bool(torch.equal(a, pending[2][1])))
            except Exception as exc:          # (reported by the assertion below)
                result.append(exc)

        t = threading.Thread(target=other_thread)
        t.start()
        t.join()
        assert result == [True], result
        both("3 persistent, first thread again", c3)
        torch.cuda.synchronize()
        assert torch.equal(pending[-1][1], pending[-1][2])
    finally:
        capi.set_eval_mode(capi.EVAL_AUTO)


@pytest.mark.parametrize("nodes", [(64, 64, 64), (40, 33, 52), (20, 20, 20)])
def test_eval_persistent_path_clusters_ends_and_small_batches(port, nodes):
    """The persistent 3-D path of round 4 (place pass that DEALS the queries of a bin by LDS slot class / evaluation waves
    that take chunks from two-level counters / windows next to an end of the grid in the semi-closed form): batches that
    stress its bookkeeping -- every query in ONE cell (all in one (bin, class): the overflow round of the dealing), every
    query in the first / last three cells of some dimension (boundary runs only), queries outside the grid and on the
    nodes, and batches smaller than one place-pass workgroup -- return the bits of the direct kernel and the values of the
    reference algorithm (oracle)."""
    nd = 3
    rng = np.random.default_rng(nodes[0] * 7 + nodes[2])
    coef = rng.standard_normal(int(np.prod(nodes)))
    lo = np.array([-0.5, 1.0, 2.0])
    hi = lo + np.array([1.0, 2.5, 0.75])
    dx = (hi - lo) / (np.array(nodes) - 1)
    batches = {}
    n = 70_001
    one_cell = lo + dx * (np.array([5, 2, nodes[2] - 3]) + rng.random((n, 3)))                 # one cell, next to two ends
    batches["one cell"] = one_cell
    ends = lo + (hi - lo) * rng.random((n, 3))
    k = rng.integers(0, 3, n)
    side = rng.integers(0, 2, n)
    cell = rng.integers(0, 3, n) + rng.random(n)
    ends[np.arange(n), k] = np.where(side == 0, lo[k] + dx[k] * cell, hi[k] - dx[k] * cell)  # first / last three cells
    batches["ends"] = ends
    mixed = lo + (hi - lo) * (-0.3 + 1.6 * rng.random((n, 3)))                                 # ~60 % outside the grid
    mixed[:4000] = lo + dx * rng.integers(-1, np.array(nodes) + 1, (4000, 3))                 # on the nodes (and one step outside)
    batches["outside + nodes"] = mixed
    batches["tiny"] = lo + (hi - lo) * rng.random((37, 3))
    batches["one workgroup"] = lo + (hi - lo) * rng.random((8192, 3))
    try:
        for name, q in batches.items():
            capi.set_eval_mode(capi.EVAL_DIRECT)
            vd, rc = capi.evaluate(nd, q, None, coef, lo, hi, nodes)
            assert rc == 0
            capi.set_eval_mode(capi.EVAL_BINNED, 0)
            vb, rc = capi.evaluate(nd, q, None, coef, lo, hi, nodes)
            assert rc == 0
            assert np.array_equal(vd, vb), (nodes, name)
            m = min(len(q), 3000)
            vo, _ = port.evaluate(nd, q[:m], None, coef, lo, hi, nodes)
            assert np.max(np.abs(vb[:m] - vo)) <= EVAL_TOL * max(np.max(np.abs(vo)), np.max(np.abs(coef))), (nodes, name)
    finally:
        capi.set_eval_mode(capi.EVAL_AUTO)


@pytest.mark.parametrize("nodes", [(32, 32, 32, 32), (24, 20, 9, 27), (12, 35, 12, 8)])
def test_eval_persistent_4d_path_matches_the_direct_kernel(port, nodes):
    """The persistent 4-D path of round 5 (BASELINE config 5's evaluation half: place pass over 2 x 256 bins, one persistent
    workgroup per CU with the (8 + 3)^4 tile of a region in LDS, waves that take chunks of runs and find their elements by a
    search over the lanes' prefixes, unsort pass): scattered queries, every query in ONE cell (one bin: a single long run per
    place-pass workgroup), queries in the first / last three cells of some dimension (boundary bins only), outside the grid
    and on the nodes, batches below one place-pass workgroup and one query over a chunk boundary -- values and a derivative
    pattern return the bits of the direct kernel and the values of the reference algorithm (oracle); REAL32 storage too."""
    nd = 4
    rng = np.random.default_rng(nodes[0] * 7 + nodes[3])
    coef = rng.standard_normal(int(np.prod(nodes)))
    lo = np.array([-0.5, 1.0, 2.0, 0.0])
    hi = lo + np.array([1.0, 2.5, 0.75, 3.0])
    nn = np.array(nodes)
    dx = (hi - lo) / (nn - 1)
    batches = {}
    n = 300_001
    batches["scattered"] = lo + (hi - lo) * rng.random((n, nd))
    batches["one cell"] = lo + dx * (np.array([5, 2, nodes[2] - 3, 1]) + rng.random((n // 3, nd)))
    ends = lo + (hi - lo) * rng.random((n // 3, nd))
    k = rng.integers(0, nd, n // 3)
    side = rng.integers(0, 2, n // 3)
    cell = rng.integers(0, 3, n // 3) + rng.random(n // 3)
    ends[np.arange(n // 3), k] = np.where(side == 0, lo[k] + dx[k] * cell, hi[k] - dx[k] * cell)
    batches["ends"] = ends
    mixed = lo + (hi - lo) * (-0.3 + 1.6 * rng.random((n // 3, nd)))
    mixed[:4000] = lo + dx * rng.integers(-1, nn + 1, (4000, nd))
    batches["outside + nodes"] = mixed
    batches["tiny"] = lo + (hi - lo) * rng.random((37, nd))
    batches["one workgroup + 1"] = lo + (hi - lo) * rng.random((8193, nd))
    try:
        for name, q in batches.items():
            for pat in (None, [0, 1, 0, 2]):
                if pat is not None and name not in ("scattered", "outside + nodes"):
                    continue
                capi.set_eval_mode(capi.EVAL_DIRECT)
                vd, rc = capi.evaluate(nd, q, pat, coef, lo, hi, nodes)
                assert rc == 0
                capi.set_eval_mode(capi.EVAL_BINNED, 0)
                vb, rc = capi.evaluate(nd, q, pat, coef, lo, hi, nodes)
                assert rc == 0
                assert np.array_equal(vd, vb), (nodes, name, pat)
                m = min(len(q), 2000)
                vo, _ = port.evaluate(nd, q[:m], pat, coef, lo, hi, nodes)
                scale = max(np.max(np.abs(vo)), np.max(np.abs(coef)) * float(np.max(1.0 / dx)) ** sum(pat or [0]))
                assert np.max(np.abs(vb[:m] - vo)) <= EVAL_TOL * scale, (nodes, name, pat)
        q = batches["scattered"].astype(np.float32)
        c32 = coef.astype(np.float32)
        capi.set_eval_mode(capi.EVAL_DIRECT)
        v0, _ = capi.evaluate(nd, q, None, c32, lo, hi, nodes, real32=True)
        capi.set_eval_mode(capi.EVAL_BINNED, 0)
        v1, _ = capi.evaluate(nd, q, None, c32, lo, hi, nodes, real32=True)
        assert np.array_equal(v0, v1)
    finally:
        capi.set_eval_mode(capi.EVAL_AUTO)


def test_config5_evaluation_at_full_size_1e8_queries(port):
    """BASELINE config 5's evaluation half AT ITS OWN SIZE (round-5 verdict: only bench.py ran it, unchecked): 4-D 32^4
    coefficients, 1e8 scattered queries resident in HBM (the seeded query stream of splpak_amd.synth), splfe values and two splde
    derivative patterns, real64 and REAL32 storage.  The persistent region path (what the automatic choice takes at this size) must
    return the BITS of the one-thread-per-query kernel on the whole batch (src/splpak.F90:1089-1240 is the arithmetic of both),
    and the values of the reference algorithm (oracle port.evaluate) on a sample of 2 000 queries spread over the batch."""
    import torch
    capi.shutdown()
    torch.cuda.empty_cache()
    nd, nod, nq = 4, 32, 100_000_000
    nodes, lo, hi = [nod] * nd, [0.0] * nd, [1.0] * nd
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(2026)
    coef_h = rng.standard_normal(nod ** nd)
    coef = torch.from_numpy(coef_h).to(dev)
    q = torch.empty((nq, nd), dtype=torch.float64, device=dev)
    capi.synth_queries_dev(nd, 10_000_000, 0, nq, q, st)
    vd = torch.empty(nq, dtype=torch.float64, device=dev)
    vb = torch.empty(nq, dtype=torch.float64, device=dev)
    sample = np.linspace(0, nq - 1, 2000).astype(np.int64)
    qs = q[torch.from_numpy(sample).to(dev)].cpu().numpy()
    try:
        for pat in (None, [1, 0, 0, 0], [0, 2, 0, 1]):
            capi.set_eval_mode(capi.EVAL_DIRECT)
            capi.evaluate_dev(nd, q, pat, coef, lo, hi, nodes, vd, st)
            capi.set_eval_mode(capi.EVAL_BINNED, 0)
            capi.evaluate_dev(nd, q, pat, coef, lo, hi, nodes, vb, st)
            torch.cuda.synchronize()
            assert torch.equal(vd, vb), pat
            capi.set_eval_mode(capi.EVAL_AUTO)
            capi.evaluate_dev(nd, q, pat, coef, lo, hi, nodes, vb, st)
            torch.cuda.synchronize()
            assert torch.equal(vd, vb), pat
            vo, _ = port.evaluate(nd, qs, pat, coef_h, lo, hi, nodes)
            got = vd[torch.from_numpy(sample).to(dev)].cpu().numpy()
            scale = max(np.max(np.abs(vo)), np.max(np.abs(coef_h)) * 31.0 ** sum(pat or [0]))
            assert np.max(np.abs(got - vo)) <= EVAL_TOL * scale, pat
        del vd, vb
        # REAL32 storage (f64 arithmetic inside): the two paths agree bitwise, and with real64 to single-precision rounding of the inputs
        q32 = q.to(torch.float32)
        del q
        c32 = coef.to(torch.float32)
        v0 = torch.empty(nq, dtype=torch.float32, device=dev)
        v1 = torch.empty(nq, dtype=torch.float32, device=dev)
        for pat in (None, [0, 2, 0, 1]):
            capi.set_eval_mode(capi.EVAL_DIRECT)
            capi.evaluate_dev(nd, q32, pat, c32, lo, hi, nodes, v0, st)
            capi.set_eval_mode(capi.EVAL_BINNED, 0)
            capi.evaluate_dev(nd, q32, pat, c32, lo, hi, nodes, v1, st)
            torch.cuda.synchronize()
            assert torch.equal(v0, v1), pat
            vo, _ = port.evaluate(nd, qs.astype(np.float32).astype(np.float64), pat, coef_h.astype(np.float32).astype(np.float64), lo, hi, nodes)
            got = v0[torch.from_numpy(sample).to(dev)].cpu().numpy().astype(np.float64)
            scale = max(np.max(np.abs(vo)), np.max(np.abs(coef_h)) * 31.0 ** sum(pat or [0]))
            assert np.max(np.abs(got - vo)) <= 2e-6 * scale, pat
    finally:
        capi.set_eval_mode(capi.EVAL_AUTO)
        capi.shutdown()
        torch.cuda.empty_cache()


def test_eval_run_path_with_clustered_queries():
    """The 3-D run path (round 3: every place-pass workgroup leaves its own region-sorted image and the starts of its
    runs; the evaluation workgroups gather the runs of their region -- no global sort).  Scattered queries give runs of
    ~16; 90 % of these sit in one small box (one region: runs of ~1 800), the rest is scattered, a few lie outside the
    grid: every value must still be the direct kernel's, for values and a derivative pattern, over several chunks."""
    rng = np.random.default_rng(99)
    nodes, nq = (64, 64, 64), 300_001
    coef = rng.standard_normal(int(np.prod(nodes)))
    q = -0.05 + 1.1 * rng.random((nq, 3))
    hot = rng.random(nq) < 0.9
    q[hot] = 0.40 + 0.05 * rng.random((int(hot.sum()), 3))
    try:
        for pat in (None, [0, 1, 2]):
            capi.set_eval_mode(capi.EVAL_BINNED, 1 << 17)
            vb, rc = capi.evaluate(3, q, pat, coef, [0.0] * 3, [1.0] * 3, nodes)
            assert rc == 0
            capi.set_eval_mode(capi.EVAL_DIRECT)
            vd, rc = capi.evaluate(3, q, pat, coef, [0.0] * 3, [1.0] * 3, nodes)
            assert rc == 0 and np.array_equal(vb, vd), pat
    finally:
        capi.set_eval_mode(capi.EVAL_AUTO)


@pytest.mark.parametrize("nodes", [(20, 17, 30), (12, 9, 8, 14), (70, 40)])
def test_eval_derivs_binned_path_is_bit_identical_to_direct(nodes):
    """Value + gradient + Hessian through the region sort (LDS tiles) must return the bits of the direct
    kernel: queries outside the grid, padded rows, a ragged last chunk, both orders."""
    import torch
    nd = len(nodes)
    rng = np.random.default_rng(nd * 77 + nodes[0])
    dev = torch.device("cuda", 0)
    coef = torch.tensor(rng.standard_normal(int(np.prod(nodes))), device=dev)
    lo = -1.0 + rng.random(nd)
    hi = lo + 1.0 + 3.0 * rng.random(nd)
    nq = 30011
    q = np.full((nq, nd + 1), 1e300)
    q[:, :nd] = lo + (hi - lo) * (-0.2 + 1.4 * rng.random((nq, nd)))
    q[:50, :nd] = lo + (hi - lo) * rng.integers(0, 2, (50, nd))
    qd = torch.tensor(q, device=dev)
    try:
        for order in (1, 2):
            nout = capi.derivs_nout(nd, order)
            od = torch.full((nq, nout + 1), -7.0, dtype=torch.float64, device=dev)
            ob = torch.full((nq, nout + 1), -7.0, dtype=torch.float64, device=dev)
            capi.set_eval_mode(capi.EVAL_DIRECT)
            assert capi.evaluate_derivs_dev(nd, qd, order, coef, lo, hi, nodes, od) == 0
            capi.set_eval_mode(capi.EVAL_BINNED, 4099)
            assert capi.evaluate_derivs_dev(nd, qd, order, coef, lo, hi, nodes, ob) == 0
            torch.cuda.synchronize()
            assert torch.equal(od, ob), (nodes, order)
            assert bool((ob[:, nout] == -7.0).all())          # the padding column is not touched
    finally:
        capi.set_eval_mode(capi.EVAL_AUTO)


@pytest.mark.parametrize("name", ["c1_1d16", "2d16", "3d8", "3d_aniso", "4d6"])
def test_eval_derivs_matches_splde_patterns(port, name):
    """Fused value / gradient / Hessian evaluation: every output column equals splde with the
    matching nderiv pattern -- against the reference's golden values where they exist, the GPU's
    single-pattern path and the oracle otherwise."""
    spec = CASES[name]
    gold = load_golden(name)
    inp = make_inputs(spec)
    nd, nodes, lo, hi = inp["ndim"], inp["nodes"], inp["xmin"], inp["xmax"]
    q = make_queries(spec)
    coef = gold["coef"]
    dxin = (np.array(spec["nodes"]) - 1) / (hi - lo)
    cmax = np.max(np.abs(coef))
    for order in (1, 2):
        out, rc = capi.evaluate_derivs(nd, q, order, coef, lo, hi, nodes)
        assert rc == 0 and out.shape == (q.shape[0], capi.derivs_nout(nd, order))
        pats = [[0] * nd] + [[int(e == d) for e in range(nd)] for d in range(nd)]
        if order == 2:
            pats += [[int(e == d) + int(e == f) for e in range(nd)] for d in range(nd) for f in range(d, nd)]
        for j, p in enumerate(pats):
            ref, rc1 = capi.evaluate(nd, q, p, coef, lo, hi, nodes)
            scale = max(np.max(np.abs(ref)), cmax * float(np.prod(dxin ** np.array(p))))
            assert np.max(np.abs(out[:, j] - ref)) <= EVAL_TOL * scale, (name, order, p)
            vo, _ = port.evaluate(nd, q[:200], p, coef, lo, hi, nodes)
            assert np.max(np.abs(out[:200, j] - vo)) <= EVAL_TOL * scale, (name, order, p)
    # real32 twin and argument errors
    o32, rc = capi.evaluate_derivs(nd, q.astype(np.float32), 1, coef.astype(np.float32), lo, hi, nodes, real32=True)
    assert rc == 0 and o32.dtype == np.float32
    o64, _ = capi.evaluate_derivs(nd, q.astype(np.float32).astype(np.float64), 1,
                                  coef.astype(np.float32).astype(np.float64), lo, hi, nodes)
    assert np.max(np.abs(o32 - o64)) <= 2e-5 * max(np.max(np.abs(o64)), 1e-30)
    with pytest.raises(capi.SplpakError):
        capi.evaluate_derivs(nd, q, 3, coef, lo, hi, nodes)
    z, rc = capi.evaluate_derivs(nd, q, 1, coef, lo, lo, nodes)      # xmin == xmax: 103, zeros
    assert rc == 103 and not z.any()


# ---------------------------------------------------------------------------
# fit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_fit_matches_reference_golden(name):
    spec = CASES[name]
    gold = load_golden(name)
    inp = make_inputs(spec)
    coef, ierr, hist, info = capi.fit(inp["ndim"], inp["xdata"], inp["ydata"], inp["wdata"], inp["xmin"],
                                      inp["xmax"], inp["nodes"], inp["xtrap"], want_hist=True)
    assert ierr == 0 == int(gold["ierror"])
    err = relmax(coef, gold["coef"])
    print(f"{name}: rel={err:.2e} refine_steps={info[2]:.0f} last_corr={info[3]:.1e} minpiv={info[4]:.2e} "
          f"rows={info[0]:.0f}+{info[1]:.0f}")
    assert err < COEF_TOL
    if inp["xtrap"] != 0.0:
        assert relmax(hist, gold["hist"]) < 1e-12


def test_fit_fresh_inputs_vs_oracle(port):
    rng = np.random.default_rng(11)
    for nd, nodes, m in [(1, [9], 40), (2, [6, 11], 700), (3, [5, 4, 7], 900), (4, [4, 4, 5, 4], 1500)]:
        x = rng.random((m, nd)) * 1.2 - 0.1
        y = np.cos(x.sum(axis=1) * 2.0) + 0.05 * rng.standard_normal(m)
        w = rng.random(m)
        w[rng.random(m) < 0.1] = 0.0
        for wd, xtrap in [(w, 1.0), (None, 0.3)]:
            c0, e0, w0 = port.fit(nd, x, y, wd, [0.0] * nd, [1.0] * nd, nodes, xtrap)
            c1, e1, h1, _ = capi.fit(nd, x, y, wd, [0.0] * nd, [1.0] * nd, nodes, xtrap, want_hist=True)
            n = int(np.prod(nodes))
            assert e0 == e1 == 0
            assert relmax(c1[:n], c0[:n]) < COEF_TOL
            assert relmax(h1[:n], w0[:n]) < 1e-12


def test_fit_dimension_reordering_vs_oracle(port):
    """A plan orders the dimensions by node count internally (smallest fastest) to minimise the
    bandwidth; coefficients and the histogram must come back in the caller's order.  Descending
    and mixed node counts, a different box per dimension, points outside the box."""
    rng = np.random.default_rng(23)
    for nd, nodes in [(2, [11, 6]), (3, [9, 6, 4]), (3, [4, 8, 5]), (4, [6, 4, 5, 4])]:
        m = 1200
        lo = -1.0 + rng.random(nd)
        hi = lo + 0.5 + 2.0 * rng.random(nd)
        x = lo + (hi - lo) * (rng.random((m, nd)) * 1.2 - 0.1)
        y = np.cos(((x - lo) / (hi - lo) * np.arange(1, nd + 1)).sum(axis=1) * 2.0) + 0.05 * rng.standard_normal(m)
        w = 0.5 + rng.random(m)
        for xtrap in (1.0, 0.0):
            c0, e0, w0 = port.fit(nd, x, y, w, lo, hi, nodes, xtrap)
            c1, e1, h1, _ = capi.fit(nd, x, y, w, lo, hi, nodes, xtrap, want_hist=True)
            n = int(np.prod(nodes))
            assert e0 == e1 == 0, (nodes, xtrap, e0, e1)
            assert relmax(c1[:n], c0[:n]) < COEF_TOL, (nodes, xtrap)
            if xtrap != 0.0:
                assert relmax(h1[:n], w0[:n]) < 1e-12, (nodes, xtrap)
            q = lo + (hi - lo) * rng.random((500, nd))
            v1, _ = capi.evaluate(nd, q, None, c1, lo, hi, nodes)
            v0, _ = port.evaluate(nd, q, None, c0, lo, hi, nodes)
            assert np.max(np.abs(v1 - v0)) <= 1e-9 * np.max(np.abs(v0))


def test_fit_l1xdat_and_negative_first_weight(port):
    """xdata(l1xdat, ndata) with l1xdat > ndim (:521-525); wdata(1) < 0 means unweighted (:581-588)."""
    inp = make_inputs(CASES["2d8"])
    m = inp["xdata"].shape[0]
    xpad = np.full((m, 4), 1e300)
    xpad[:, :2] = inp["xdata"]
    c_ref = load_golden("2d8_cc")["coef"]
    w = inp["wdata"].copy()
    w[0] = -1.0
    coef, ierr, _, _ = capi.fit(2, xpad, inp["ydata"], w, inp["xmin"], inp["xmax"], inp["nodes"], 1.0)
    assert ierr == 0 and relmax(coef, c_ref) < COEF_TOL


def test_fit_error_codes():
    """107 conditions of the reference (:683-686)."""
    x = np.linspace(0, 1, 50).reshape(-1, 1)
    y = np.sin(x[:, 0])
    assert capi.fit(1, x, y, np.zeros(50), [0.0], [1.0], [10], 1.0)[1] == 107   # all-zero weights
    assert capi.fit(1, x, y, np.zeros(50), [0.0], [1.0], [10], 0.0)[1] == 107
    x5 = np.linspace(0.1, 0.9, 5).reshape(-1, 1)
    assert capi.fit(1, x5, np.sin(x5[:, 0]), None, [0.0], [1.0], [10], 0.0)[1] == 107  # too few rows
    c, rc, _, _ = capi.fit(1, x5, np.sin(x5[:, 0]), None, [0.0], [1.0], [10], 1.0)       # constraints regularise
    assert rc == 0 and np.all(np.isfinite(c))
    # enough rows but rank deficient (all data in one corner, no smoothing): not positive definite
    xc = np.random.default_rng(0).random((400, 2)) * 0.2
    assert capi.fit(2, xc, xc.sum(axis=1), None, [0.0, 0.0], [1.0, 1.0], [8, 8], 0.0)[1] == 107


def test_grid_beyond_one_gpu_is_a_clean_error(monkeypatch):
    """BASELINE config 5's 32^4 grid on ONE GPU: the nested-dissection factor panels alone are 476 GB (+ ~131 GB of Schur
    arena in the postorder schedule; the band factor would be 852 GB) against 309 GB of HBM, and the boxes' 322 GB host-memory
    cgroup cannot park the difference either: asked for a FACTORISATION (SPLPAK_SOLVER=direct) the plan must be refused with
    the library's out-of-memory status, not crash.  Left to itself the plan takes the iterative solve of round 6 and the fit
    runs (tests/test_pcg.py::test_config5_fit_4d_32_on_one_gpu)."""
    monkeypatch.setenv("SPLPAK_SOLVER", "direct")
    with pytest.raises(capi.SplpakError) as e:
        capi.Plan(4, [32] * 4, [0.0] * 4, [1.0] * 4, 1.0, 1000)
    assert "-2" in str(e.value) or "memory" in str(e.value).lower()
    # the host-pointer entry reports the same failure as a negative ierror
    x = np.random.default_rng(1).random((100, 4))
    with pytest.raises(capi.SplpakError):
        capi.fit(4, x, x.sum(axis=1), None, [0.0] * 4, [1.0] * 4, [32] * 4, 1.0)
    monkeypatch.delenv("SPLPAK_SOLVER")
    plan = capi.Plan(4, [32] * 4, [0.0] * 4, [1.0] * 4, 1.0, 1000)
    try:
        assert plan.factorisation()[0] == 6
    finally:
        plan.close()


def test_eval_4d_32_real32_vs_real64_sweep(port):
    """BASELINE config 5, evaluation half at full size: 4-D 32^4 coefficients, values and derivatives.
    real64 is anchored to the reference algorithm (oracle) on a sample; real32 (single-precision
    storage) is bounded by the single-precision rounding of its inputs -- the small-grid comparison
    with the REAL32 reference itself is test_eval_real32_vs_real32_reference."""
    nodes = [32] * 4
    rng = np.random.default_rng(5)
    coef = rng.standard_normal(32 ** 4)
    q = rng.random((200_000, 4))
    lo, hi = [0.0] * 4, [1.0] * 4
    for p, tol in ((None, 2e-6), ([1, 0, 0, 0], 2e-6), ([0, 2, 0, 1], 2e-6)):
        v64, rc = capi.evaluate(4, q, p, coef, lo, hi, nodes)
        assert rc == 0
        vo, _ = port.evaluate(4, q[:500], p, coef, lo, hi, nodes)
        scale64 = max(np.max(np.abs(vo)), np.max(np.abs(coef)) * 31.0 ** sum(p or [0]))
        assert np.max(np.abs(v64[:500] - vo)) <= EVAL_TOL * scale64, p
        v32, rc = capi.evaluate(4, q.astype(np.float32), p, coef.astype(np.float32), lo, hi, nodes, real32=True)
        assert rc == 0 and v32.dtype == np.float32
        # same inputs rounded to single, evaluated in double: isolates the storage rounding
        v64r, _ = capi.evaluate(4, q.astype(np.float32).astype(np.float64), p,
                                coef.astype(np.float32).astype(np.float64), lo, hi, nodes)
        scale = np.max(np.abs(v64))
        assert np.max(np.abs(v32 - v64r)) <= tol * scale, p
        assert np.max(np.abs(v64r - v64)) <= 1e-3 * scale, p        # input rounding amplified by 31/box derivatives


def test_reference_known_answer_linear_on_gpu():
    """test/splpak_test_linear.f90:65-89 through the HIP path: slope 2 within 1e-12."""
    inp = make_inputs(CASES["ref_linear"])
    coef, ierr, _, _ = capi.fit(1, inp["xdata"], inp["ydata"], inp["wdata"], inp["xmin"], inp["xmax"],
                                inp["nodes"], inp["xtrap"])
    assert ierr == 0
    v, ie = capi.evaluate(1, np.array([[0.0], [1.0]]), [1], coef, inp["xmin"], inp["xmax"], inp["nodes"])
    assert ie == 0 and np.all(np.abs(v - 2.0) <= 1e-12)
    xs = (np.arange(100) / 100.0).reshape(-1, 1)
    v, _ = capi.evaluate(1, xs, None, coef, inp["xmin"], inp["xmax"], inp["nodes"])
    assert np.max(np.abs(v - 2.0 * xs[:, 0])) <= 1e-1


def test_plan_reuse_gives_identical_fits():
    """A plan is reusable: consecutive fits through one plan (the bench.py pattern) must each be
    correct.  Regression test: the trailing-update item queues of the factorisation pipeline were
    once indexed past their allocation, which only broke the SECOND fit of a plan."""
    import torch
    spec = CASES["3d12"]
    gold = load_golden("3d12")
    inp = make_inputs(spec)
    dev = torch.device("cuda", 0)
    x = torch.tensor(inp["xdata"], device=dev)
    y = torch.tensor(inp["ydata"], device=dev)
    w = torch.tensor(inp["wdata"], device=dev)
    ncol = int(np.prod(inp["nodes"]))
    plan = capi.Plan(3, inp["nodes"], inp["xmin"], inp["xmax"], inp["xtrap"], x.shape[0])
    coefs = []
    for _ in range(3):
        coef = torch.zeros(ncol, dtype=torch.float64, device=dev)
        ierr, info = plan.fit(x, y, w, coef, torch.cuda.current_stream().cuda_stream)
        assert ierr == 0
        coefs.append(coef.cpu().numpy())
        assert relmax(coefs[-1], gold["coef"]) < COEF_TOL
    plan.close()
    assert np.array_equal(coefs[1], coefs[0]) and np.array_equal(coefs[2], coefs[0])


def test_large_grid_repeated_fit_properties():
    """Size-independent properties on a grid the dense reference cannot reach in test time
    (3-D 24^3 = 13 824 columns, 3e5 points): (a) data sampled from a function in the spline
    space (a plane; natural splines reproduce it, xtrap = 0) is recovered to 1e-10 at fresh
    points, also on a second fit through the same plan; (b) splcc == splcw with unit weights."""
    import torch
    from splpak_amd.synth import synth_points, synth_queries
    nd, nod, m = 3, 24, 300000
    x, _, _ = synth_points(nd, m)
    f = lambda p: 1.0 + 2.0 * p[:, 0] - 3.0 * p[:, 1] + 0.5 * p[:, 2]
    dev = torch.device("cuda", 0)
    xt = torch.tensor(x, device=dev)
    yt = torch.tensor(f(x), device=dev)
    wt = torch.ones(m, dtype=torch.float64, device=dev)
    plan = capi.Plan(nd, [nod] * nd, [0.0] * nd, [1.0] * nd, 0.0, m)
    q = synth_queries(nd, 2000, m) * 1.2 - 0.1            # also outside the grid: linear extrapolation
    res = []
    for wv in (None, wt, None):
        coef = torch.zeros(nod ** nd, dtype=torch.float64, device=dev)
        ierr, info = plan.fit(xt, yt, wv, coef, torch.cuda.current_stream().cuda_stream)
        assert ierr == 0
        c = coef.cpu().numpy()
        v, ie = capi.evaluate(nd, q, None, c, [0.0] * nd, [1.0] * nd, [nod] * nd)
        assert ie == 0 and np.max(np.abs(v - f(q))) < 1e-10
        res.append(c)
    assert relmax(res[1], res[0]) < 1e-11 and relmax(res[2], res[0]) < 1e-11
    plan.close()


def _fit_with_env(inp, env):
    """One-shot fit with environment switches of the factorisation pipeline (read at every call)."""
    import os
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return capi.fit(inp["ndim"], inp["xdata"], inp["ydata"], inp["wdata"], inp["xmin"], inp["xmax"],
                        inp["nodes"], inp["xtrap"])
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("name", ["3d12", "3d16", "2d64_c2grid", "4d6"])
def test_headline_pipeline_variants_match_golden(name):
    """BASELINE config 3 (64^3, block half-bandwidth 49) runs the factorisation with potrf PINNED to
    its reserved CU (taken when the band is >= 24 blocks wide).  Force that pipeline -- and the
    unpinned and the no-look-ahead forms -- on grids the reference covers: each must hold the golden
    at 1e-10 and they must agree with each other to 1e-13 (same arithmetic, different scheduling)."""
    gold = load_golden(name)
    inp = make_inputs(CASES[name])
    res = {}
    for label, env in (("pinned", {"SPLPAK_PIN_BW": "1"}), ("unpinned", {"SPLPAK_PIN_BW": "1000000"}),
                       ("serial", {"SPLPAK_NO_LOOKAHEAD": "1"})):
        env = dict(env, SPLPAK_ND="0")       # the BAND pipelines (3d16 and 2d64 take nested dissection by default since round 3)
        coef, ierr, _, info = _fit_with_env(inp, env)
        assert ierr == 0, (label, ierr)
        err = relmax(coef, gold["coef"])
        print(f"{name} [{label}]: rel={err:.2e} steps={info[2]:.0f} optimality={info[9]:.1e}")
        assert err < COEF_TOL, (label, err)
        assert info[9] < 1e-9, (label, info[9])
        res[label] = coef
    assert relmax(res["pinned"], res["unpinned"]) <= 1e-13
    assert relmax(res["serial"], res["unpinned"]) <= 1e-13
    _pipeline_variants_have_equal_bits(name, inp["ndim"], inp["xdata"], inp["ydata"], inp["wdata"], inp["xmin"], inp["xmax"],
                                       inp["nodes"], inp["xtrap"])


# the four-stream pipeline of csrc/bandchol.hip pinned, unpinned and on one stream.  (SPLPAK_NO_LOOKAHEAD=1 alone, the "serial" of
# the refined comparisons above, leaves the narrow limit at its default: on these grids that is the two-ended form on serial chains,
# another launch split, which tests/test_band_scheduling.py does not compare with the pipeline bit for bit either.)
PIPELINE_SCHEDULES = (("pinned", {"SPLPAK_PIN_BW": "1"}), ("unpinned", {"SPLPAK_NARROW_BW": "1", "SPLPAK_PIN_BW": "1000000"}),
                      ("serial", {"SPLPAK_NARROW_BW": "1", "SPLPAK_PIN_BW": "1000000", "SPLPAK_NO_LOOKAHEAD": "1"}))


def _pipeline_variants_have_equal_bits(what, nd, x, y, w, xmin, xmax, nodes, xtrap):
    """Fits WITHOUT refinement (the coefficients are the factorisation's one solve) under the three schedules of the pipeline:
    identical bits and smallest pivots -- tests/test_band_scheduling.py established no exception for this family."""
    import torch
    dev = torch.device("cuda", 0)
    xt = torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)
    yt = torch.tensor(y, dtype=torch.float64, device=dev)
    wt = None if w is None else torch.tensor(w, dtype=torch.float64, device=dev)
    res = {}
    for label, env in PIPELINE_SCHEDULES:
        env = dict(env, SPLPAK_ND="0", SPLPAK_SOLVER="direct", SPLPAK_NO_TWOEND="1")
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            plan = capi.Plan(nd, nodes, xmin, xmax, xtrap, xt.shape[0])
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        try:
            code, text = plan.factorisation()
            assert code == 0, (label, code, text)
            plan.set_refine(0, 1e-11)
            coef = torch.zeros(plan.ncol, dtype=torch.float64, device=dev)
            ierr, info = plan.fit(xt, yt, wt, coef)
            torch.cuda.synchronize()
            assert ierr == 0 and info[2] == 0 and info[4] > 0, (label, ierr, info)
            res[label] = (coef.cpu().numpy(), float(info[4]))
        finally:
            plan.close()
    for label in ("pinned", "serial"):
        same = np.array_equal(res[label][0], res["unpinned"][0])
        print(f"{what} without refinement [{label} / unpinned]: equal bits {same}, min pivot {res[label][1]!r} / {res['unpinned'][1]!r}")
        assert same and res[label][1] == res["unpinned"][1], (what, label, relmax(res[label][0], res["unpinned"][0]))


def test_pinned_pipeline_24cubed_property():
    """The pinned pipeline on the 24^3 grid (13 824 columns, band 8 blocks wide, 54 steps): data from
    the spline space is reproduced to 1e-10 (xtrap = 0) and matches the unpinned pipeline; without refinement
    pinned, unpinned and serial give identical bits."""
    import os
    import torch
    from splpak_amd.synth import synth_points, synth_queries
    nd, nod, m = 3, 24, 300000
    x, _, _ = synth_points(nd, m)
    f = lambda p: 1.0 + 2.0 * p[:, 0] - 3.0 * p[:, 1] + 0.5 * p[:, 2]
    q = synth_queries(nd, 2000, m) * 1.2 - 0.1
    out = {}
    for label, pin in (("pinned", "1"), ("unpinned", "1000000")):
        os.environ["SPLPAK_PIN_BW"] = pin
        os.environ["SPLPAK_ND"] = "0"          # this test is about the BAND pipelines (grids of this size default to nested dissection)
        try:
            c, ierr, _, info = capi.fit(nd, x, f(x), None, [0.0] * nd, [1.0] * nd, [nod] * nd, 0.0)
        finally:
            os.environ.pop("SPLPAK_PIN_BW", None)
            os.environ.pop("SPLPAK_ND", None)
        assert ierr == 0
        v, _ = capi.evaluate(nd, q, None, c, [0.0] * nd, [1.0] * nd, [nod] * nd)
        assert np.max(np.abs(v - f(q))) < 1e-10, label
        assert info[9] < 1e-9
        out[label] = c
    assert relmax(out["pinned"], out["unpinned"]) <= 1e-13
    _pipeline_variants_have_equal_bits("24^3", nd, x, f(x), None, [0.0] * nd, [1.0] * nd, [nod] * nd, 0.0)


def test_c3_full_size_properties():
    """BASELINE config 3 AT FULL SIZE through the code path bench.py times (3-D, 64^3 = 262 144 columns,
    10^7 points of the seeded stream; round 3: the nested-dissection multifrontal factorisation, 1 023 fronts).
    The dense reference cannot run this grid (550 GB of workspace), so parity is checked through
    size-independent properties:
      (a) data sampled from a spline of the grid with RANDOM coefficients (xtrap = 0, so the fit is a
          projection): the coefficients are recovered to 1e-10 max-norm;
      (b) splcc equals splcw with unit weights;
      (c) the measured optimality residual (info[9]) is at rounding level;
      (d) the band factorisation (round 2's path: pinned-potrf pipeline, band 49 blocks wide, SPLPAK_ND=0) gives the
          same coefficients to 1e-12."""
    import torch
    nd, nod, m = 3, 64, 10_000_000
    nodes, lo, hi = [nod] * nd, [0.0] * nd, [1.0] * nd
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    x = torch.empty((m, nd), dtype=torch.float64, device=dev)
    capi.synth_points_dev(nd, 0, m, x, None, None, st)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    ctrue = torch.randn(nod ** nd, dtype=torch.float64, device=dev, generator=gen)
    # a plane on top, so that the linear end functions (natural boundary) carry signal too
    y = torch.empty(m, dtype=torch.float64, device=dev)
    capi.evaluate_dev(nd, x, None, ctrue, lo, hi, nodes, y, st)
    plan = capi.Plan(nd, nodes, lo, hi, 0.0, m)
    try:
        coef = torch.zeros(nod ** nd, dtype=torch.float64, device=dev)
        ierr, info = plan.fit(x, y, None, coef, st)                       # splcc
        assert ierr == 0
        err = float((coef - ctrue).abs().max() / ctrue.abs().max())
        print(f"64^3 projection: coefficient error {err:.2e}, steps {info[2]:.0f}, last corr {info[3]:.1e}, "
              f"optimality {info[9]:.1e}, data rows {info[0]:.0f}")
        assert info[0] == m
        assert err < COEF_TOL
        assert info[9] < 1e-9
        w = torch.ones(m, dtype=torch.float64, device=dev)
        coefw = torch.zeros_like(coef)
        ierr, infow = plan.fit(x, y, w, coefw, st)                        # splcw, unit weights
        assert ierr == 0
        assert float((coefw - coef).abs().max() / coef.abs().max()) < 1e-11
        # fresh queries, also outside the grid: values of the fitted and the true spline agree
        q = torch.rand((100000, nd), dtype=torch.float64, device=dev, generator=gen) * 1.2 - 0.1
        v1 = torch.empty(q.shape[0], dtype=torch.float64, device=dev)
        v2 = torch.empty_like(v1)
        capi.evaluate_dev(nd, q, None, coef, lo, hi, nodes, v1, st)
        capi.evaluate_dev(nd, q, None, ctrue, lo, hi, nodes, v2, st)
        torch.cuda.synchronize()
        assert float((v1 - v2).abs().max() / v2.abs().max()) < 1e-10
        import os
        os.environ["SPLPAK_ND"] = "0"
        try:
            band = capi.Plan(nd, nodes, lo, hi, 0.0, m)
        finally:
            os.environ.pop("SPLPAK_ND", None)
        try:
            coefb = torch.zeros_like(coef)
            ierr, infob = band.fit(x, y, None, coefb, st)
            assert ierr == 0
            dband = float((coefb - coef).abs().max() / coef.abs().max())
            print(f"64^3: nested dissection vs band {dband:.2e}; factorisation {info[6]:.3f} s vs {infob[6]:.3f} s")
            assert dband < 1e-12
        finally:
            band.close()
    finally:
        plan.close()


@pytest.mark.parametrize("name,mb", [("3d12", 3), ("4d6", 8), ("2d32", 1), ("c1_1d16", 1)])
def test_gram_blocks_in_slabs_match_golden(name, mb, monkeypatch):
    """The per-cell Gram blocks are produced and gathered in slabs when the scratch cannot hold all of
    them (189 GB at the 4-D 32^4 grid): force a scratch of a few MB so that these grids take several
    slabs; the fit must hold the golden exactly as with one slab."""
    capi.lib().splpak_shutdown()                     # drop the cached plan of the one-shot entry
    monkeypatch.setenv("SPLPAK_GRAM_SCRATCH_MB", str(mb))
    gold = load_golden(name)
    inp = make_inputs(CASES[name])
    try:
        coef, ierr, hist, info = capi.fit(inp["ndim"], inp["xdata"], inp["ydata"], inp["wdata"], inp["xmin"],
                                          inp["xmax"], inp["nodes"], inp["xtrap"], want_hist=True)
    finally:
        capi.lib().splpak_shutdown()
    assert ierr == 0 and relmax(coef, gold["coef"]) < COEF_TOL
    assert relmax(hist, gold["hist"]) < 1e-12 and info[9] < 1e-9


@pytest.mark.parametrize("nod,m", [(24, 100000), (32, 150000)])
def test_fit_matches_banded_cpu_beyond_the_dense_oracle(port, nod, m):
    """Grids the dense reference algorithm cannot reach in test time (24^3 = 13 824, 32^3 = 32 768 columns),
    WITH weights and derivative-constraint rows: the GPU fit against the independent CPU solve of the
    reference's rows (oracle/splpak_banded.c, itself pinned to the reference goldens)."""
    from splpak_amd.synth import synth_points
    nd = 3
    x, y, w = synth_points(nd, m)
    lo, hi, nodes = [0.0] * nd, [1.0] * nd, [nod] * nd
    c0, e0, i0 = port.fit_banded(nd, x, y, w, lo, hi, nodes, 1.0)
    # the BAND factorisation (two-ended at these sizes); the nested-dissection path these grids take by default is
    # held to the same CPU solve in tests/test_nd.py
    c1, e1, _, i1 = _fit_with_env(dict(ndim=nd, xdata=x, ydata=y, wdata=w, xmin=lo, xmax=hi, nodes=nodes, xtrap=1.0), {"SPLPAK_ND": "0"})
    assert e0 == e1 == 0
    print(f"{nod}^3: GPU vs banded CPU rel={relmax(c1, c0):.2e}; rows {i1[0]:.0f}+{i1[1]:.0f}; reserr GPU {i1[8]:.6e} CPU {i0[8]:.6e}; "
          f"CPU {i0[5] + i0[6] + i0[7]:.1f} s on {i0[9]:.0f} threads")
    assert relmax(c1, c0) < COEF_TOL
    assert i1[0] == i0[0] and i1[1] == i0[1]
    assert abs(i1[8] - i0[8]) <= 1e-9 * i0[8]


def test_slowly_contracting_refinement_is_not_a_silent_success():
    """A solve whose refinement has not converged must not return ierror 0: with the
    nominal step count forced to 1 and an unreachable tolerance the loop continues while it
    contracts; with refinement switched off entirely the coefficients of an ill-conditioned grid
    miss the parity bar and the diagnostics show it."""
    import torch
    inp = make_inputs(CASES["2d32"])
    gold = load_golden("2d32")
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    x = torch.tensor(inp["xdata"], device=dev)
    y = torch.tensor(inp["ydata"], device=dev)
    w = torch.tensor(inp["wdata"], device=dev)
    plan = capi.Plan(2, inp["nodes"], inp["xmin"], inp["xmax"], inp["xtrap"], x.shape[0])
    try:
        coef = torch.zeros(32 * 32, dtype=torch.float64, device=dev)
        plan.set_refine(1, 1e-12)            # nominal 1 step: must go on by itself until converged
        ierr, info = plan.fit(x, y, w, coef, st)
        assert ierr == 0 and info[2] >= 2
        assert relmax(coef.cpu().numpy(), gold["coef"]) < COEF_TOL
        plan.set_refine(0, 1e-12)            # no refinement at all: plain normal equations (~6e-8)
        ierr, info0 = plan.fit(x, y, w, coef, st)
        assert ierr == 0 and info0[2] == 0
        assert info0[9] > 10 * info[9]       # the measured optimality residual exposes the unrefined solve
        plan.set_refine(4, 1e-12)
    finally:
        plan.close()


@pytest.mark.parametrize("name", ["c1_1d16", "2d16", "2d16_sparse", "3d8_cc_clust", "4d4"])
def test_residual_norm_matches_reference_algorithm(port, name):
    """info[8] = ||rows*coef - rhs||_2 over data and constraint rows: the `reserr` the reference
    computes in suprls (:1693) and drops in splcw (:690).  Checked against the oracle's value."""
    inp = make_inputs(CASES[name])
    _, ierr, _, info = capi.fit(inp["ndim"], inp["xdata"], inp["ydata"], inp["wdata"], inp["xmin"], inp["xmax"],
                                inp["nodes"], inp["xtrap"])
    _, e0, _ = port.fit(inp["ndim"], inp["xdata"], inp["ydata"], inp["wdata"], inp["xmin"], inp["xmax"],
                        inp["nodes"], inp["xtrap"])
    assert ierr == e0 == 0
    assert abs(info[8] - port.last_reserr) <= 1e-9 * max(port.last_reserr, 1e-300)


def test_fit_is_linear_in_ydata_and_idempotent():
    """Size-independent properties of the least-squares fit (same xdata, wdata, grid):
    coef(a*y1 + b*y2) = a*coef(y1) + b*coef(y2); and fitting data sampled FROM a spline of the
    grid with xtrap = 0 returns that spline (projection is idempotent)."""
    inp = make_inputs(CASES["3d8"])
    nd, x, w = inp["ndim"], inp["xdata"], inp["wdata"]
    rng = np.random.default_rng(5)
    y1, y2 = inp["ydata"], np.cos(7.0 * x.sum(axis=1)) + rng.standard_normal(x.shape[0])
    args = (inp["xmin"], inp["xmax"], inp["nodes"], inp["xtrap"])
    c1 = capi.fit(nd, x, y1, w, *args)[0]
    c2 = capi.fit(nd, x, y2, w, *args)[0]
    c12 = capi.fit(nd, x, 2.5 * y1 - 0.75 * y2, w, *args)[0]
    assert relmax(c12, 2.5 * c1 - 0.75 * c2) < 1e-10
    # idempotence: y := spline(c1) at the data points, no smoothing rows
    ys, _ = capi.evaluate(nd, x, None, c1, inp["xmin"], inp["xmax"], inp["nodes"])
    c3, ierr, _, _ = capi.fit(nd, x, ys, w, inp["xmin"], inp["xmax"], inp["nodes"], 0.0)
    assert ierr == 0 and relmax(c3, c1) < 1e-9


def test_ragged_and_degenerate_batches():
    """One point, all points in one cell, duplicated points, a huge batch of one repeated query."""
    lo, hi, nodes = [0.0, 0.0], [1.0, 1.0], [6, 6]
    # a single data point cannot determine 36 coefficients without smoothing rows ...
    assert capi.fit(2, np.array([[0.3, 0.4]]), np.array([1.0]), None, lo, hi, nodes, 0.0)[1] == 107
    # ... with them the fit exists; it must agree with the reference algorithm
    from oracle.binding import Port
    P = Port()
    x1 = np.array([[0.3, 0.4]])
    c, ierr, _, _ = capi.fit(2, x1, np.array([1.0]), None, lo, hi, nodes, 1.0)
    c0, e0, _ = P.fit(2, x1, np.array([1.0]), None, lo, hi, nodes, 1.0)
    assert ierr == e0 == 0 and relmax(c, c0[:36]) < 1e-10
    # many coincident points in a single window + a few elsewhere
    rng = np.random.default_rng(3)
    x = np.vstack([np.tile([[0.52, 0.47]], (500, 1)), rng.random((200, 2))])
    y = np.sin(3 * x[:, 0]) + x[:, 1]
    c, ierr, _, _ = capi.fit(2, x, y, None, lo, hi, nodes, 1.0)
    c0, e0, _ = P.fit(2, x, y, None, lo, hi, nodes, 1.0)
    assert ierr == e0 == 0 and relmax(c, c0[:36]) < 1e-10
    q = np.tile([[0.25, 0.75]], (100000, 1))
    v, rc = capi.evaluate(2, q, [1, 1], c, lo, hi, nodes)
    assert rc == 0 and np.all(v == v[0])


def test_c2_full_size_vs_banded_cpu(port):
    """BASELINE config 2 AT FULL SIZE (2-D, 64x64 nodes, 1e6 scattered points, equal weights = splcc, xtrap = 1)
    against the independent CPU solve of the reference's rows (oracle/splpak_banded.c, pinned to the goldens incl.
    this grid's 2d64_c2grid): coefficients at 1e-10, same row counts, same residual norm (VERDICT r02 #6b)."""
    from splpak_amd.synth import synth_points
    nd, m = 2, 1_000_000
    x, y, _ = synth_points(nd, m)
    lo, hi, nodes = [0.0] * nd, [1.0] * nd, [64, 64]
    c0, e0, i0 = port.fit_banded(nd, x, y, None, lo, hi, nodes, 1.0)
    c1, e1, _, i1 = capi.fit(nd, x, y, None, lo, hi, nodes, 1.0)
    assert e0 == e1 == 0
    print(f"C2 full size: GPU vs banded CPU rel={relmax(c1, c0):.2e}; rows {i1[0]:.0f}+{i1[1]:.0f}; reserr GPU {i1[8]:.9e} CPU {i0[8]:.9e}")
    assert relmax(c1, c0) < COEF_TOL
    assert i1[0] == i0[0] == m and i1[1] == i0[1]
    assert abs(i1[8] - i0[8]) <= 1e-9 * i0[8]
    assert i1[9] < 1e-9


def test_c3_full_size_weighted_optimality_on_the_host(port):
    """BASELINE config 3 AT FULL SIZE, WEIGHTED and with its derivative-constraint rows (1e7 points of the seeded
    stream, 64^3 nodes, xtrap = 1 -- the workload bench.py times): the coefficients the GPU returns are checked
    on the HOST against the reference's rows, independently of the GPU's own residual kernels
    (oracle_rows_gradient: rows generated as in src/splpak.F90:788-855 and :862-1046, never stored): the
    componentwise backward error max_i |A^T(b - A x)|_i / (|A|^T(|A||x| + |b|))_i is at rounding level, the row
    counts and the residual norm `reserr` agree with what the GPU reports (VERDICT r02 #6c)."""
    from splpak_amd.synth import synth_points
    nd, nod, m = 3, 64, 10_000_000
    x, y, w = synth_points(nd, m)
    lo, hi, nodes = [0.0] * nd, [1.0] * nd, [nod] * nd
    c, e, _, info = capi.fit(nd, x, y, w, lo, hi, nodes, 1.0)
    assert e == 0
    omega, reserr, nrow, ncons = port.rows_gradient(nd, x, y, w, lo, hi, nodes, 1.0, c)
    print(f"C3 weighted: host backward error {omega:.2e} (GPU's own: {info[9]:.2e}); rows {nrow}+{ncons} "
          f"(GPU {info[0]:.0f}+{info[1]:.0f}); reserr host {reserr:.9e} GPU {info[8]:.9e}")
    assert omega < 1e-12
    assert nrow == info[0] == m and ncons == info[1]
    assert abs(reserr - info[8]) <= 1e-9 * reserr
    # and the check has teeth: a coefficient off by 1e-7 (relative to the largest) is seen
    c2 = c.copy()
    c2[c.size // 2] += 1e-7 * np.abs(c).max()
    assert port.rows_gradient(nd, x, y, w, lo, hi, nodes, 1.0, c2)[0] > 1e-9


def _far_outside_case(nd, nodes, m, far_point, weighted, seed=11):
    rng = np.random.default_rng(seed)
    x = rng.random((m, nd))
    x = np.vstack([x, np.asarray(far_point, dtype=np.float64).reshape(1, nd)])
    y = np.cos(2.0 * x.sum(axis=1))
    w = (0.5 + rng.random(m + 1)) if weighted else None
    return x, y, w


FAR_CASES = [
    # SURVEY 8a3's own case (2-D 4x4: ONE window holds every node, the outlier's address 2 is a node of it)
    ("survey_2d4", 2, [4, 4], None, (5.0, 0.5), False),
    # grids with more than one window: the outlier's Horner address (its in-range dimensions alone, :899) is NOT a node of
    # the window the point is binned into -> the one f64 atomicAdd left in the assembly (gram.hip: stage_points, "far outside")
    ("2d8_wave", 2, [8, 8], 600, (5.0, 0.9), True),
    ("2d8_wave_both", 2, [8, 8], 600, (-7.0, 9.0), True),          # both dimensions skipped: address 0
    ("3d7_wave", 3, [7, 6, 8], 2500, (0.2, -4.0, 0.95), True),
    ("4d6_mfma4", 4, [6, 5, 6, 5], 5000, (0.9, 0.1, 7.5, 0.8), True),
    ("1d16_block", 1, [16], 300, (5.0,), True),
]


@pytest.mark.parametrize("name,nd,nodes,m,far,weighted", FAR_CASES)
def test_histogram_far_outside_point_on_gpu(port, name, nd, nodes, m, far, weighted):
    """SURVEY 8a3 / src/splpak.F90:886-907: a coordinate so far outside the grid that its nearest-node index is out of
    range executes the unlabelled `cycle` of the DIMENSION loop (:899) -- the point is still counted, at the Horner address
    of its remaining dimensions, and still adds to totlwt.  Through gram_wave_kernel (2-D / 3-D), gram_mfma4_kernel (4-D)
    and gram_block_kernel (1-D), whose only f64 atomicAdd this is; compared with the reference algorithm's work(1:ncol)."""
    if m is None:                                   # the survey's case verbatim: 36 in-range points + (5.0, 0.5)
        g = (np.arange(6) + 0.5) / 6.0
        xx, yy = np.meshgrid(g, g, indexing="ij")
        x = np.vstack([np.column_stack([xx.ravel(), yy.ravel()]), [far]])
        y, w = x[:, 0] + x[:, 1], None
    else:
        x, y, w = _far_outside_case(nd, nodes, m, far, weighted)
    lo, hi = [0.0] * nd, [1.0] * nd
    ncol = int(np.prod(nodes))
    c0, e0, work = port.fit(nd, x, y, w, lo, hi, nodes, 1.0)
    c1, e1, hist, info = capi.fit(nd, x, y, w, lo, hi, nodes, 1.0, want_hist=True)
    assert e0 == e1 == 0
    base = capi.fit(nd, x[:-1], y[:-1], None if w is None else w[:-1], lo, hi, nodes, 1.0, want_hist=True)[2]
    diff = hist - base
    bump = 1.0 if w is None else w[-1]
    print(f"{name}: outlier counted at 0-based address {int(np.argmax(np.abs(diff)))}, hist sum {hist.sum():.6f} "
          f"(reference {work[:ncol].sum():.6f}), coef rel {relmax(c1, c0[:ncol]):.1e}")
    assert np.count_nonzero(diff) == 1 and abs(diff.max() - bump) < 1e-12
    assert relmax(hist, work[:ncol]) < 1e-13
    assert int(np.argmax(diff)) == int(np.argmax(work[:ncol] - port.fit(nd, x[:-1], y[:-1], None if w is None else w[:-1],
                                                                        lo, hi, nodes, 1.0)[2][:ncol]))
    if m is None:
        assert hist.sum() == 37.0 and int(np.argmax(diff)) == 2
    assert relmax(c1, c0[:ncol]) < COEF_TOL


def test_histogram_far_outside_point_valu_gram_kernel():
    """The same through gram_block_kernel on 2-D / 4-D grids (SPLPAK_GRAM_VALU=1 is read once per process: a child process)."""
    import os
    import subprocess
    import sys
    code = r'''
import numpy as np, sys
sys.path.insert(0, %r)
from splpak_amd import capi
from tests.test_gpu_parity import _far_outside_case
for nd, nodes, m, far in [(2, [8, 8], 600, (5.0, 0.9)), (4, [6, 5, 6, 5], 5000, (0.9, 0.1, 7.5, 0.8))]:
    x, y, w = _far_outside_case(nd, nodes, m, far, True)
    lo, hi = [0.0] * nd, [1.0] * nd
    h = capi.fit(nd, x, y, w, lo, hi, nodes, 1.0, want_hist=True)[2]
    np.save(sys.argv[1] + "_%%d.npy" %% nd, h)
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        env = dict(os.environ, SPLPAK_GRAM_VALU="1")
        subprocess.check_call([sys.executable, "-c", code % root, os.path.join(td, "h")], env=env, cwd=root)
        for nd, nodes, m, far in [(2, [8, 8], 600, (5.0, 0.9)), (4, [6, 5, 6, 5], 5000, (0.9, 0.1, 7.5, 0.8))]:
            x, y, w = _far_outside_case(nd, nodes, m, far, True)
            lo, hi = [0.0] * nd, [1.0] * nd
            h_mfma = capi.fit(nd, x, y, w, lo, hi, nodes, 1.0, want_hist=True)[2]
            h_valu = np.load(os.path.join(td, f"h_{nd}.npy"))
            assert relmax(h_valu, h_mfma) < 1e-13 and abs(h_valu.sum() - w.sum()) < 1e-9


def test_cells_of_more_than_1024_points_are_ordered_too():
    """binpoints.hip cell_order_kernel: the per-cell sums follow the storage order of the binned points, and the scatter's
    atomic cursor hands out positions in a different order every run.  Cells of up to 1 024 points are re-ordered through
    LDS; larger ones (up to 65 536 points in one window) by the chunked rank count added in round 4.  2-D 5x5 nodes =
    4 windows, 30 000 points = 7 500 per window: four fits must agree bit for bit, coefficients AND histogram, and hold
    the reference algorithm's answer."""
    import torch
    nd, nodes, m = 2, [5, 5], 30000
    from splpak_amd.synth import synth_points
    x, y, w = synth_points(nd, m)
    lo, hi = [0.0] * nd, [1.0] * nd
    dev = torch.device("cuda", 0)
    xt, yt, wt = (torch.tensor(a, device=dev) for a in (x, y, w))
    coef = torch.zeros(25, dtype=torch.float64, device=dev)
    plan = capi.Plan(nd, nodes, lo, hi, 1.0, m)
    outs = []
    for _ in range(4):
        ierr, info = plan.fit(xt, yt, wt, coef, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert ierr == 0
        outs.append((coef.cpu().numpy().copy(), info[8]))
    plan.close()
    for c, r in outs[1:]:
        assert np.array_equal(c, outs[0][0]) and r == outs[0][1], "a cell of 7 500 points is summed in a run-dependent order"
    from oracle.binding import Port
    c0, e0, _ = Port().fit(nd, x, y, w, lo, hi, nodes, 1.0)
    assert e0 == 0 and relmax(outs[0][0], c0[:25]) < COEF_TOL


SP_CASES = ["1d_sparse", "2d64_c2grid", "3d16", "3d8_cc_clust", "2d16_zero_w", "4d6", "3d_cells", "2d_cluster", "2d_two_level"]


def _sp_case_args(case):
    rng = np.random.default_rng(3)
    if case in CASES:
        inp = make_inputs(CASES[case])
        return (inp["ndim"], inp["xdata"], inp["ydata"], inp["wdata"], inp["xmin"], inp["xmax"], inp["nodes"], inp["xtrap"])
    if case == "3d_cells":              # 64^3: 226 981 windows -> two levels, tiles of 56 cells, most of them nearly empty
        x = rng.random((300000, 3))
        return (3, x, np.sin(x.sum(axis=1)), 0.5 + rng.random(300000), [0.0] * 3, [1.0] * 3, [64] * 3, 1.0)
    if case == "2d_cluster":            # one level; 20 000 of 30 000 points in ONE window, a tenth of the weights zero
        x = rng.random((30000, 2))
        x[:20000] = 0.41 + 0.01 * rng.random((20000, 2))
        w = 0.5 + rng.random(30000)
        w[::10] = 0.0
        return (2, x, np.cos(3 * x[:, 0]) + x[:, 1], w, [0.0] * 2, [1.0] * 2, [20, 20], 1.0)
    # 2-D 90 x 80: 6 699 windows -> two levels with 2 cells per tile; a cluster of 30 000 in one tile
    x = rng.random((60000, 2))
    x[:30000] = [0.3, 0.6] + 0.004 * rng.random((30000, 2))
    return (2, x, np.cos(3 * x[:, 0]) + x[:, 1], None, [0.0] * 2, [1.0] * 2, [90, 80], 0.5)


def _sp_fit_twice(case):
    out = []
    for _ in range(2):
        c, e, h, info = capi.fit(*_sp_case_args(case), want_hist=True)
        out.append((c, h, info[8], e, info[0]))
    assert out[0][3] == 0 and np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    return dict(coef=out[0][0], hist=out[0][1], reserr=out[0][2], rows=out[0][4])


@pytest.fixture(scope="module")
def atomic_binning_results(tmp_path_factory):
    """Every case of SP_CASES through the binning of rounds 1-4 (SPLPAK_BIN_ATOMIC=1), in ONE child process: the switch is
    read once per process."""
    import subprocess
    import sys
    td = tmp_path_factory.mktemp("atomic_binning")
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from tests.test_gpu_parity import SP_CASES, _sp_fit_twice\n"
            "for case in SP_CASES:\n"
            "    np.savez(sys.argv[1] + '/' + case + '.npz', **_sp_fit_twice(case))\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code, str(td)], env=dict(os.environ, SPLPAK_BIN_ATOMIC="1"), capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-800:]
    return {case: dict(np.load(os.path.join(td, case + ".npz"))) for case in SP_CASES}


@pytest.mark.parametrize("case", SP_CASES)
def test_stable_partition_gives_the_bits_of_the_atomic_binning(case, atomic_binning_results):
    """Round 5 (binpoints.hip sp_*): the points are binned by a counting sort without global atomics that is stable by
    construction -- the points of a window end up in ascending original index, the order cell_order_kernel used to restore after
    the atomic scatter.  So every fit must return the SAME BITS through both forms (SPLPAK_BIN_ATOMIC=1 = rounds 1-4, in a child
    process: the switch is read once): goldens of one level (cells <= 4 095) and two levels (tiles of cells, then cells), zero
    weights (never placed), clustered data (one window holding 20 000 points: several sub-blocks of a tile), a grid of 230 000
    windows with 300 000 points, and repeated fits through one plan."""
    a, b = _sp_fit_twice(case), atomic_binning_results[case]
    assert a["rows"] == b["rows"]
    assert np.array_equal(a["coef"], b["coef"]) and np.array_equal(a["hist"], b["hist"]) and a["reserr"] == b["reserr"], case


def test_c4_workload_on_one_gpu_weighted_optimality_on_the_host(port):
    """BASELINE config 4's WORKLOAD -- 1e8 scattered weighted points of the seeded stream on the 64^3 grid -- on ONE GPU
    (the config shards it over 8; the multi-GPU path is covered in tests/test_dist.py): the returned coefficients are
    checked on the host against the reference's rows (oracle_rows_gradient over ALL 1e8 rows + the constraint rows, never
    stored): componentwise backward error at rounding level, row counts and reserr as the GPU reports them."""
    import torch
    nd, nod, m = 3, 64, 100_000_000
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    x = torch.empty((m, nd), dtype=torch.float64, device=dev)
    y = torch.empty(m, dtype=torch.float64, device=dev)
    w = torch.empty(m, dtype=torch.float64, device=dev)
    capi.synth_points_dev(nd, 0, m, x, y, w, st)
    lo, hi, nodes = [0.0] * nd, [1.0] * nd, [nod] * nd
    coef = torch.zeros(nod ** nd, dtype=torch.float64, device=dev)
    plan = capi.Plan(nd, nodes, lo, hi, 1.0, m)
    try:
        ierr, info = plan.fit(x, y, w, coef, st)
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert ierr == 0
    c = coef.cpu().numpy()
    xh, yh, wh = x.cpu().numpy(), y.cpu().numpy(), w.cpu().numpy()
    del x, y, w
    torch.cuda.empty_cache()
    omega, reserr, nrow, ncons = port.rows_gradient(nd, xh, yh, wh, lo, hi, nodes, 1.0, c)
    print(f"C4 workload on one GPU: {info[5] + info[6] + info[7]:.3f} s, host backward error {omega:.2e} (GPU's own {info[9]:.2e}); "
          f"rows {nrow}+{ncons}; reserr host {reserr:.9e} GPU {info[8]:.9e}")
    assert omega < 1e-12
    assert nrow == info[0] == m and ncons == info[1]
    assert abs(reserr - info[8]) <= 1e-9 * reserr
