"""Evaluation on a tensor-product grid of points (splpak_eval_grid_*, csrc/evalgrid.hip).

The yardstick on the GPU is the library's own direct kernel (splpak_eval_dev_* with EVAL_DIRECT on the Cartesian
product of the axes), which test_gpu_parity.py holds to the oracle and the goldens: the grid entries must return
EXACTLY its values (np.array_equal -- no tolerance), whichever form a tile takes (coefficient box in LDS contracted one
dimension at a time, or the plain gather), because a shared partial sum is one of window_sum's own intermediates.
Coefficients are seeded random normals; no fit is involved.

CPU tier: exports and the host-side argument checks, all of which return before any device call.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from splpak_amd import capi
from tests.conftest import relmax

LP = C.POINTER(C.c_int64)


# ---------------------------------------------------------------------------------------------------------------
# CPU tier
def _host_call(ndim, npts, nodes, xmin, xmax, out, axes=None, coef=None, nderiv=None):
    npts = np.asarray(npts, dtype=np.int64)
    nodes = np.asarray(nodes, dtype=np.int32)
    xmin = np.asarray(xmin, dtype=np.float64)
    xmax = np.asarray(xmax, dtype=np.float64)
    axes = np.full(max(int(np.sum(np.abs(npts))), 1), 0.3) if axes is None else axes
    coef = np.ones(max(int(np.prod(np.maximum(nodes, 1))), 1)) if coef is None else coef
    nd = None if nderiv is None else np.asarray(nderiv, dtype=np.int32)
    return capi.lib().splpak_eval_grid_f64(ndim, capi._p(npts, LP), capi._p(axes, capi._dp), capi._p(nd, capi._ip),
                                           capi._p(coef, capi._dp), capi._p(xmin, capi._dp), capi._p(xmax, capi._dp),
                                           capi._p(nodes, capi._ip), capi._p(out, capi._dp))


def test_grid_symbols_are_exported():
    L = capi.lib()
    for name in ("splpak_eval_grid_f64", "splpak_eval_grid_f32", "splpak_eval_grid_dev_f64", "splpak_eval_grid_dev_f32",
                 "splpak_eval_grid_scratch_bytes", "splpak_debug_eval_grid_stats"):
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS
    assert callable(capi.evaluate_grid) and callable(capi.evaluate_grid_dev)


def test_grid_validation_zeroes_out_without_gpu():
    """101/102/103 are decided on the host and zero `out` (:1166-1188); 101 has no shape, so one output."""
    out = np.full(12, 7.0)
    assert _host_call(0, [3, 4], [8, 8], [0, 0], [1, 1], out) == 101
    assert out[0] == 0.0 and np.all(out[1:] == 7.0)
    out = np.full(12, 7.0)
    assert _host_call(2, [3, 4], [8, 3], [0, 0], [1, 1], out) == 102
    assert np.all(out == 0.0)
    out = np.full(13, 7.0)
    assert _host_call(2, [3, 4], [8, 8], [0, 0.5], [1, 0.5], out) == 103
    assert np.all(out[:12] == 0.0) and out[12] == 7.0
    # the first failing check wins, as in the point entries
    assert _host_call(0, [3, 4], [8, 3], [0, 0], [1, 1], np.zeros(12)) == 101
    # the Python wrapper reports them too
    v, rc = capi.evaluate_grid(2, [np.zeros(3), np.zeros(4)], None, np.ones(24), [0, 0], [1, 1], [8, 3])
    assert rc == 102 and v.shape == (4, 3) and np.all(v == 0.0)


def test_grid_bad_shapes_without_gpu():
    out = np.full(12, 7.0)
    assert _host_call(2, [3, -4], [8, 8], [0, 0], [1, 1], out) == capi.E_BADARG
    assert _host_call(2, [2 ** 40, 2 ** 40], [8, 8], [0, 0], [1, 1], out, axes=np.zeros(1)) == capi.E_BADARG      # product beyond int64
    assert np.all(out == 7.0)
    assert _host_call(5, [2] * 5, [4] * 5, [0] * 5, [1] * 5, out) == capi.E_UNSUPPORTED
    assert np.all(out == 7.0)
    # a count of 0: the validation status, nothing written
    assert _host_call(2, [3, 0], [8, 8], [0, 0], [1, 1], out) == 0
    assert _host_call(2, [0, 4], [8, 8], [0, 0], [1, 1], out, nderiv=[0, 3]) == 104
    assert _host_call(2, [3, 0], [8, 3], [0, 0], [1, 1], out) == 102
    assert np.all(out == 7.0)
    # null pointers
    L = capi.lib()
    npts = np.array([3, 4], dtype=np.int64)
    assert L.splpak_eval_grid_f64(2, capi._p(npts, LP), None, None, None, None, None, None, None) == capi.E_BADARG
    nodes = np.array([8, 8], dtype=np.int32)
    lo, hi = np.zeros(2), np.ones(2)
    assert L.splpak_eval_grid_f64(2, None, None, None, None, capi._p(lo, capi._dp), capi._p(hi, capi._dp),
                                  capi._p(nodes, capi._ip), None) == capi.E_BADARG
    assert L.splpak_eval_grid_f64(2, capi._p(npts, LP), None, None, None, capi._p(lo, capi._dp), capi._p(hi, capi._dp),
                                  capi._p(nodes, capi._ip), capi._p(out, capi._dp)) == capi.E_BADARG
    assert np.all(out == 7.0)


def test_grid_scratch_bytes():
    """40 bytes per axis coordinate (four factors and the window start) and the two tile counters."""
    assert capi.eval_grid_scratch_bytes([512, 512, 512]) == 40 * 1536 + 16
    assert capi.eval_grid_scratch_bytes([7]) == 40 * 7 + 16
    assert capi.eval_grid_scratch_bytes([5, 0, 3]) == 0
    npts = np.array([3, -1], dtype=np.int64)
    assert capi.lib().splpak_eval_grid_scratch_bytes(2, capi._p(npts, LP)) == capi.E_BADARG
    assert capi.lib().splpak_eval_grid_scratch_bytes(5, capi._p(np.ones(5, dtype=np.int64), LP)) == capi.E_BADARG


# ---------------------------------------------------------------------------------------------------------------
# GPU tier
# Box of every case: bounds exact in single precision, so that the REAL32 entries see the same grid.
LO, HI = [-1.25, 0.0, 2.0, -0.5], [3.5, 1.0, 2.75, 0.25]


def _awkward_axes(seed, nodes, npts):
    """Unsorted axes with a tenth of the points outside the box on both sides, exact node positions, xmin, xmax and
    repeated values."""
    rng = np.random.default_rng(seed)
    axes = []
    for d, (nod, n) in enumerate(zip(nodes, npts)):
        lo, hi = LO[d], HI[d]
        w = hi - lo
        x = rng.uniform(lo, hi, n)
        k = n // 10
        if k:
            x[:k] = rng.uniform(lo - 0.3 * w, lo, k)
            x[k:2 * k] = rng.uniform(hi, hi + 0.3 * w, k)
        special = [lo, hi] + list(lo + (w / (nod - 1)) * rng.integers(0, nod, 4))
        for j, s in enumerate(special[:max(0, n - 2 * k - 1)]):
            x[2 * k + j] = s
        if n >= 8:
            x[-1] = x[-2] = x[2 * k]            # repeats
        rng.shuffle(x)
        axes.append(x)
    return axes


def _monotone_axes(nodes, npts):
    """Regular resampling axes that reach a little beyond the box on both sides."""
    return [np.linspace(LO[d] - 0.01 * (HI[d] - LO[d]), HI[d] + 0.01 * (HI[d] - LO[d]), n) for d, n in enumerate(npts)]


@functools.lru_cache(maxsize=None)
def _coef(nodes, real32=False):
    c = np.random.default_rng(sum(nodes) + len(nodes)).standard_normal(int(np.prod(nodes)))
    return c.astype(np.float32) if real32 else c


def _product(axes):
    """The Cartesian product as a query list, dimension 1 fastest (the ordering of `out`)."""
    mesh = np.meshgrid(*axes[::-1], indexing="ij")
    return np.stack([m.ravel() for m in mesh[::-1]], axis=1)


def _point_route(nodes, axes, nderiv, real32=False):
    """The yardstick: the direct kernel on the product query list."""
    import torch
    nd = len(nodes)
    dt = torch.float32 if real32 else torch.float64
    dev = torch.device("cuda", 0)
    q = torch.from_numpy(_product(axes)).to(dev).to(dt)
    coef = torch.from_numpy(_coef(tuple(nodes), real32)).to(dev)
    out = torch.empty(q.shape[0], dtype=dt, device=dev)
    capi.set_eval_mode(capi.EVAL_DIRECT)
    try:
        rc = capi.evaluate_dev(nd, q, nderiv, coef, LO[:nd], HI[:nd], nodes, out, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        capi.set_eval_mode(capi.EVAL_AUTO)
    return out.cpu().numpy(), rc


def _grid_route(nodes, axes, nderiv, real32=False, stream=None):
    """-> (values, ierror, (LDS tiles, general tiles))"""
    import torch
    nd = len(nodes)
    dt = torch.float32 if real32 else torch.float64
    dev = torch.device("cuda", 0)
    npts = [a.size for a in axes]
    a = torch.from_numpy(np.concatenate(axes)).to(dev).to(dt)
    coef = torch.from_numpy(_coef(tuple(nodes), real32)).to(dev)
    out = torch.full((int(np.prod(npts)),), float("nan"), dtype=dt, device=dev)
    torch.cuda.synchronize()
    if stream is None:
        rc = capi.evaluate_grid_dev(nd, npts, a, nderiv, coef, LO[:nd], HI[:nd], nodes, out, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    else:
        rc = capi.evaluate_grid_dev(nd, npts, a, nderiv, coef, LO[:nd], HI[:nd], nodes, out, stream.cuda_stream)
        stream.synchronize()
    return out.cpu().numpy(), rc, capi.debug_eval_grid_stats()


def _tiles(nd, npts):
    shape = {1: (256,), 2: (64, 16), 3: (64, 8, 8), 4: (16, 4, 4, 4)}[nd]
    return int(np.prod([-(-n // t) for n, t in zip(npts, shape)]))


SMALL = [
    # nodes, npts: partial tiles, more than one tile, unsorted axes with points outside the box
    ((16,), (257,)),
    ((5, 12), (70, 33)),                 # a dimension below 8 nodes: general form of the basis table
    ((12, 10, 8), (37, 29, 19)),
    ((12, 10, 8), (3, 50, 2)),           # coarse: the windows do not overlap
    ((12, 10, 8), (1, 1, 1)),
    ((6, 5, 7, 4), (9, 7, 5, 11)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("nodes,npts", SMALL, ids=lambda v: "x".join(map(str, v)))
def test_grid_equals_direct_kernel_small_shapes(nodes, npts):
    axes = _awkward_axes(len(nodes) * 100 + sum(npts), nodes, npts)
    want, rc0 = _point_route(nodes, axes, None)
    got, rc, stats = _grid_route(nodes, axes, None)
    assert rc == 0 and rc0 == 0
    assert sum(stats) == _tiles(len(nodes), npts)
    assert np.array_equal(got, want), np.max(np.abs(got - want))


@pytest.mark.gpu
def test_grid_1d_shuffled_with_a_tenth_outside():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(LO[0], HI[0], 205), rng.uniform(LO[0] - 2.0, LO[0], 26), rng.uniform(HI[0], HI[0] + 2.0, 26)])
    rng.shuffle(x)
    want, _ = _point_route((16,), [x], None)
    got, rc, stats = _grid_route((16,), [x], None)
    assert rc == 0 and stats == (0, 2)          # 1-D: every tile gathers
    assert np.array_equal(got, want)


TILED = [((24, 24, 24), (96, 96, 96)), ((12, 12, 12, 12), (24, 24, 24, 24))]


@pytest.mark.gpu
@pytest.mark.parametrize("real32", [False, True], ids=["real64", "real32"])
@pytest.mark.parametrize("nodes,npts", TILED, ids=["3d", "4d"])
def test_grid_tile_path_engages_and_equals_direct_kernel(nodes, npts, real32):
    """Monotone axes: every tile stages its coefficient box in LDS (no silent fall-back to the gather).  One axis
    reversed and one shuffled: the monotone result permuted accordingly, and the point route's values; the shuffled
    axis sends tiles to the general form, which must return the same values."""
    nd = len(nodes)
    axes = _monotone_axes(nodes, npts)
    if real32:
        axes = [a.astype(np.float32).astype(np.float64) for a in axes]
    want, _ = _point_route(nodes, axes, None, real32)
    got, rc, stats = _grid_route(nodes, axes, None, real32)
    assert rc == 0
    assert stats == (_tiles(nd, npts), 0), stats
    assert got.dtype == (np.float32 if real32 else np.float64)
    assert np.array_equal(got, want), np.max(np.abs(got - want))
    perm = np.random.default_rng(9).permutation(npts[1])
    axes2 = [axes[0][::-1].copy(), axes[1][perm]] + axes[2:]
    got2, rc2, stats2 = _grid_route(nodes, axes2, None, real32)
    assert rc2 == 0 and sum(stats2) == _tiles(nd, npts) and stats2[1] > 0
    mono = got.reshape(npts[::-1])
    assert np.array_equal(got2.reshape(npts[::-1]), mono[..., perm, ::-1])
    want2, _ = _point_route(nodes, axes2, None, real32)
    assert np.array_equal(got2, want2)


@pytest.mark.gpu
@pytest.mark.parametrize("nodes,npts,pat,monotone", [
    ((12, 10, 8), (37, 29, 19), [1, 0, 2], False),
    ((24, 24, 24), (96, 96, 96), [1, 0, 2], True),
    ((5, 12), (70, 33), [0, 2], False),
    ((6, 5, 7, 4), (9, 7, 5, 11), [2, 1, 0, 1], False),
    ((12, 12, 12, 12), (24, 24, 24, 24), [2, 1, 0, 1], True),
], ids=["3d", "3d-tiled", "2d", "4d", "4d-tiled"])
def test_grid_derivatives_equal_direct_kernel(nodes, npts, pat, monotone):
    axes = _monotone_axes(nodes, npts) if monotone else _awkward_axes(77, nodes, npts)
    want, _ = _point_route(nodes, axes, pat)
    got, rc, stats = _grid_route(nodes, axes, pat)
    assert rc == 0
    if monotone:                                # regular axes of about four / two points per cell: every tile fits the LDS budget
        assert stats == (_tiles(len(nodes), npts), 0), stats
    assert np.array_equal(got, want), np.max(np.abs(got - want))


@pytest.mark.gpu
def test_grid_nderiv_out_of_range_is_104_with_clamped_values():
    nodes, npts = (12, 10, 8), (37, 29, 19)
    axes = _awkward_axes(3, nodes, npts)
    ref, rc0 = _grid_route(nodes, axes, [2, 0, 0])[:2]
    got, rc = _grid_route(nodes, axes, [3, 0, 0])[:2]
    assert rc0 == 0 and rc == 104
    assert np.array_equal(got, ref)
    want, rcp = _point_route(nodes, axes, [3, 0, 0])
    assert rcp == 104 and np.array_equal(got, want)


@pytest.mark.gpu
def test_grid_host_entry_equals_device_entry():
    nodes, npts = (12, 10, 8), (37, 29, 19)
    axes = _awkward_axes(4, nodes, npts)
    dev, rc, _ = _grid_route(nodes, axes, [0, 1, 0])
    host, rch = capi.evaluate_grid(3, axes, [0, 1, 0], _coef(nodes), LO[:3], HI[:3], nodes)
    assert rc == 0 and rch == 0 and host.shape == npts[::-1]
    assert np.array_equal(host.ravel(), dev)
    h32, rc32 = capi.evaluate_grid(3, axes, None, _coef(nodes), LO[:3], HI[:3], nodes, real32=True)
    d32 = _grid_route(nodes, [a.astype(np.float32).astype(np.float64) for a in axes], None, real32=True)[0]
    assert rc32 == 0 and h32.dtype == np.float32 and np.array_equal(h32.ravel(), d32)


@pytest.mark.gpu
def test_grid_on_a_side_stream():
    """Asynchronous on the caller's stream: synchronising THAT stream alone is enough."""
    import torch
    nodes, npts = (24, 24, 24), (96, 96, 96)
    axes = _monotone_axes(nodes, npts)
    ref, _, stats = _grid_route(nodes, axes, None)
    assert stats[1] == 0
    side = torch.cuda.Stream()
    got, rc, _ = _grid_route(nodes, axes, None, stream=side)
    assert rc == 0 and np.array_equal(got, ref)


@pytest.mark.gpu
def test_grid_against_the_oracle(port):
    """One check against the reference algorithm itself (oracle port of splde) at the project's bar."""
    nodes, npts = (12, 10, 8), (37, 29, 19)
    axes = _awkward_axes(len(nodes) * 100 + sum(npts), nodes, npts)
    got, rc, _ = _grid_route(nodes, axes, None)
    vo, eo = port.evaluate(3, _product(axes), None, _coef(nodes), LO[:3], HI[:3], list(nodes))
    assert rc == 0 and eo == 0
    assert relmax(got, vo) <= 1e-10, relmax(got, vo)
