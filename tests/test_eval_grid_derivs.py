"""Value, gradient and Hessian planes on a tensor-product grid of points (splpak_eval_grid_derivs_*, csrc/evalgridderivs.hip).

The yardstick on the GPU is the library's own single-pattern grid route (splpak_eval_grid_dev_*, which test_eval_grid.py
holds bit for bit to the direct kernel): plane e >= 1 must be EXACTLY (np.array_equal) what that route returns under entry
e's nderiv, whichever form a tile takes, because every partial sum the planes share is one of window_sum's own
intermediates.  Plane 0 is summed in the same order on the general-form value tables, the single-pattern route with
nderiv None on the closed-form ones: the project's parity bar, relmax <= 1e-10 (the two table forms are pinned to 1e-12 of
each other by test_basis_table_forms_match_the_reference_basis).  Box, axes and coefficients are those of
test_eval_grid.py.

CPU tier: exports and the host-side argument checks, all of which return before any device call.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from splpak_amd import capi
from tests.conftest import relmax
from tests.test_eval_grid import HI, LO, _awkward_axes, _coef, _monotone_axes, _product

LP = C.POINTER(C.c_int64)
NAMES = ("splpak_eval_grid_derivs_f64", "splpak_eval_grid_derivs_f32", "splpak_eval_grid_derivs_dev_f64",
         "splpak_eval_grid_derivs_dev_f32", "splpak_eval_grid_derivs_scratch_bytes", "splpak_debug_eval_grid_derivs_tile")


def _nplanes(nd, order):
    return 1 + nd + (nd * (nd + 1) // 2 if order == 2 else 0)


def _patterns(nd, order):
    """The nderiv pattern of every plane: the entries of splpak_eval_derivs_* in their order."""
    pats = [[0] * nd]
    for d in range(nd):
        pats.append([int(e == d) for e in range(nd)])
    if order == 2:
        for d in range(nd):
            for f in range(d, nd):
                pats.append([int(e == d) + int(e == f) for e in range(nd)])
    assert len(pats) == _nplanes(nd, order)
    return pats


# ---------------------------------------------------------------------------------------------------------------
# CPU tier
def _host_call(ndim, npts, nodes, xmin, xmax, out, ldout, order=1, axes=None, coef=None):
    npts = np.asarray(npts, dtype=np.int64)
    nodes = np.asarray(nodes, dtype=np.int32)
    xmin = np.asarray(xmin, dtype=np.float64)
    xmax = np.asarray(xmax, dtype=np.float64)
    axes = np.full(max(int(np.sum(np.abs(npts))), 1), 0.3) if axes is None else axes
    coef = np.ones(max(int(np.prod(np.maximum(nodes, 1))), 1)) if coef is None else coef
    return capi.lib().splpak_eval_grid_derivs_f64(ndim, capi._p(npts, LP), capi._p(axes, capi._dp), order, capi._p(coef, capi._dp),
                                                  capi._p(xmin, capi._dp), capi._p(xmax, capi._dp), capi._p(nodes, capi._ip),
                                                  capi._p(out, capi._dp), ldout)


def test_grid_derivs_symbols_are_exported():
    L = capi.lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert callable(capi.evaluate_grid_derivs) and callable(capi.evaluate_grid_derivs_dev)


def test_grid_derivs_status_ladder_without_gpu():
    """Every status is decided on the host, the first failing check wins, in the order the header gives."""
    L = capi.lib()
    nan = float("nan")
    npts = np.array([3, 4], dtype=np.int64)
    nodes = np.array([8, 8], dtype=np.int32)
    lo, hi = np.zeros(2), np.ones(2)
    out = np.full(100, nan)
    # 1. npts, nodes, xmin or xmax null
    args = dict(npts=capi._p(npts, LP), lo=capi._p(lo, capi._dp), hi=capi._p(hi, capi._dp), nodes=capi._p(nodes, capi._ip))
    for missing in args:
        a = dict(args, **{missing: None})
        assert L.splpak_eval_grid_derivs_f64(0, a["npts"], None, 7, None, a["lo"], a["hi"], a["nodes"], capi._p(out, capi._dp), 0) == capi.E_BADARG, missing
    assert np.all(np.isnan(out))
    # 2. 101: out[0] alone, before the shape, the order and ldout are looked at
    assert _host_call(0, [3, -4], [8, 3], [0, 0], [1, 1], out, 0, order=7) == 101
    assert out[0] == 0.0 and np.all(np.isnan(out[1:]))
    out[:] = nan
    # 3. more than four dimensions, before the shape and the order
    assert _host_call(5, [2, 2, -2, 2, 2], [4] * 5, [0] * 5, [1] * 5, out, 0, order=0) == capi.E_UNSUPPORTED
    # 4. a negative count, a product beyond int64
    assert _host_call(2, [3, -4], [8, 3], [0, 0], [1, 1], out, 12) == capi.E_BADARG
    assert _host_call(2, [2 ** 40, 2 ** 40], [8, 3], [0, 0], [1, 1], out, 2 ** 62, axes=np.zeros(1)) == capi.E_BADARG
    # 5. order outside 1 .. 2: before 102 (which would zero the planes)
    for order in (0, 3, -1):
        assert _host_call(2, [3, 4], [8, 3], [0, 0], [1, 1], out, 12, order=order) == capi.E_BADARG
        assert _host_call(2, [3, 0], [8, 8], [0, 0], [1, 1], out, 12, order=order) == capi.E_BADARG      # also with a count of 0
    # 6. ldout smaller than the number of grid points, or the planes beyond int64: before 102
    assert _host_call(2, [3, 4], [8, 3], [0, 0], [1, 1], out, 11) == capi.E_BADARG
    assert _host_call(2, [3, 4], [8, 3], [0, 0], [1, 1], out, -1) == capi.E_BADARG
    assert _host_call(2, [3, 4], [8, 3], [0, 0], [1, 1], out, 2 ** 62, order=2) == capi.E_BADARG
    assert np.all(np.isnan(out))
    # 7. 102 / 103: the 12 results of every plane are zeroed, the words between the planes and behind the last stay
    for order, nodes_, hi_, rc in ((1, [8, 3], [1, 1], 102), (2, [8, 8], [1, 0.0], 103)):
        out[:] = nan
        npl = _nplanes(2, order)
        assert _host_call(2, [3, 4], nodes_, [0, 0], hi_, out, 15, order=order) == rc
        planes = out[:npl * 15].reshape(npl, 15)
        assert np.all(planes[:, :12] == 0.0) and np.all(np.isnan(planes[:, 12:])) and np.all(np.isnan(out[npl * 15:]))
    out[:] = nan
    npts3 = np.array([3, 4], dtype=np.int64)
    bad = np.array([8, 3], dtype=np.int32)
    assert L.splpak_eval_grid_derivs_f64(2, capi._p(npts3, LP), None, 1, None, capi._p(lo, capi._dp), capi._p(hi, capi._dp),
                                         capi._p(bad, capi._ip), None, 12) == 102                          # a null out is not written
    # 8. a count of 0: the status so far, nothing written
    assert _host_call(2, [3, 0], [8, 8], [0, 0], [1, 1], out, 0) == 0
    assert _host_call(2, [0, 4], [8, 8], [0, 0], [1, 1], out, 5, order=2) == 0
    assert _host_call(2, [3, 0], [8, 3], [0, 0], [1, 1], out, 0) == 102
    assert np.all(np.isnan(out))
    # 9. axes, coef or out null
    axes, coef = np.zeros(7), np.ones(64)
    full = [capi._p(axes, capi._dp), capi._p(coef, capi._dp), capi._p(out, capi._dp)]
    for j in range(3):
        p = list(full)
        p[j] = None
        assert L.splpak_eval_grid_derivs_f64(2, capi._p(npts, LP), p[0], 1, p[1], capi._p(lo, capi._dp), capi._p(hi, capi._dp),
                                             capi._p(nodes, capi._ip), p[2], 12) == capi.E_BADARG, j
    assert np.all(np.isnan(out))
    # the Python wrapper reports the reference's codes too
    v, rc = capi.evaluate_grid_derivs(2, [np.zeros(3), np.zeros(4)], 2, np.ones(24), [0, 0], [1, 1], [8, 3])
    assert rc == 102 and v.shape == (6, 4, 3) and np.all(v == 0.0)


def test_grid_derivs_scratch_bytes():
    """The two tile counters and, per axis coordinate, a window start and order + 1 factor quadruples (8 + 32 (order + 1))."""
    assert capi.eval_grid_derivs_scratch_bytes([512, 512, 512], 1) == 72 * 1536 + 16
    assert capi.eval_grid_derivs_scratch_bytes([512, 512, 512], 2) == 104 * 1536 + 16
    assert capi.eval_grid_derivs_scratch_bytes([7], 2) == 104 * 7 + 16
    assert capi.eval_grid_derivs_scratch_bytes([5, 0, 3], 1) == 0
    assert capi.eval_grid_scratch_bytes([512, 512, 512]) == 40 * 1536 + 16          # the single-pattern entry keeps its value
    f = capi.lib().splpak_eval_grid_derivs_scratch_bytes
    assert f(2, capi._p(np.array([3, -1], dtype=np.int64), LP), 1) == capi.E_BADARG
    assert f(5, capi._p(np.ones(5, dtype=np.int64), LP), 1) == capi.E_BADARG
    assert f(2, capi._p(np.array([3, 4], dtype=np.int64), LP), 0) == capi.E_BADARG
    assert f(2, capi._p(np.array([3, 4], dtype=np.int64), LP), 3) == capi.E_BADARG
    assert f(2, None, 1) == capi.E_BADARG


def test_grid_derivs_tile_entry():
    for nd in (1, 2, 3, 4):
        for order in (1, 2):
            t = capi.debug_eval_grid_derivs_tile(nd, order)
            assert len(t) == 4 and all(v >= 1 for v in t[:nd]) and all(v == 1 for v in t[nd:]), (nd, order, t)
    f = capi.lib().splpak_debug_eval_grid_derivs_tile
    v = np.zeros(4, dtype=np.int32)
    for nd, order in ((0, 1), (5, 1), (3, 0), (3, 3)):
        assert f(nd, order, capi._p(v, capi._ip)) == capi.E_BADARG
    assert f(3, 1, None) == capi.E_BADARG
    assert np.all(v == 0)


# ---------------------------------------------------------------------------------------------------------------
# GPU tier
def _tiles(nd, order, npts):
    shape = capi.debug_eval_grid_derivs_tile(nd, order)
    return int(np.prod([-(-n // t) for n, t in zip(npts, shape)]))


def _tensors(nodes, axes, real32):
    import torch
    dt = torch.float32 if real32 else torch.float64
    dev = torch.device("cuda", 0)
    a = torch.from_numpy(np.concatenate(axes)).to(dev).to(dt)
    coef = torch.from_numpy(_coef(tuple(nodes), real32)).to(dev)
    return a, coef, dt, dev


def _fused(nodes, axes, order, real32=False, stream=None, pad=0, guard=0):
    """-> (planes (nplanes, prod npts), ierror, (LDS tiles, general tiles), the whole NaN-prefilled buffer)"""
    import torch
    nd = len(nodes)
    npts = [a.size for a in axes]
    nout, npl = int(np.prod(npts)), _nplanes(nd, order)
    a, coef, dt, dev = _tensors(nodes, axes, real32)
    buf = torch.full((npl * (nout + pad) + guard,), float("nan"), dtype=dt, device=dev)
    out = buf[:npl * (nout + pad)].view(npl, nout + pad)
    torch.cuda.synchronize()
    if stream is None:
        rc = capi.evaluate_grid_derivs_dev(nd, npts, a, order, coef, LO[:nd], HI[:nd], nodes, out, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    else:
        rc = capi.evaluate_grid_derivs_dev(nd, npts, a, order, coef, LO[:nd], HI[:nd], nodes, out, stream.cuda_stream)
        stream.synchronize()
    stats = capi.debug_eval_grid_stats()
    whole = buf.cpu().numpy()
    return whole[:npl * (nout + pad)].reshape(npl, nout + pad)[:, :nout].copy(), rc, stats, whole


def _single(nodes, axes, nderiv, real32=False):
    """The yardstick: the single-pattern grid route."""
    import torch
    nd = len(nodes)
    npts = [a.size for a in axes]
    a, coef, dt, dev = _tensors(nodes, axes, real32)
    out = torch.full((int(np.prod(npts)),), float("nan"), dtype=dt, device=dev)
    rc = capi.evaluate_grid_dev(nd, npts, a, nderiv, coef, LO[:nd], HI[:nd], nodes, out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    return out.cpu().numpy()


def _axes(kind, nodes, npts, real32=False):
    if kind == "awkward":
        axes = _awkward_axes(len(nodes) * 100 + sum(npts), nodes, npts)
    else:
        axes = _monotone_axes(nodes, npts)
        if kind == "permuted":
            perm = np.random.default_rng(9).permutation(npts[1])
            axes = [axes[0][::-1].copy(), axes[1][perm]] + axes[2:]
    if real32:
        axes = [a.astype(np.float32).astype(np.float64) for a in axes]
    return axes


@functools.lru_cache(maxsize=None)
def _fused_cached(nodes, npts, kind, order, real32=False):
    got, rc, stats, _ = _fused(nodes, _axes(kind, nodes, npts, real32), order, real32)
    got.setflags(write=False)
    return got, rc, stats


def _check_against_single_route(nodes, npts, kind, order, real32=False):
    nd = len(nodes)
    axes = _axes(kind, nodes, npts, real32)
    got, rc, stats = _fused_cached(nodes, npts, kind, order, real32)
    assert rc == 0
    assert got.dtype == (np.float32 if real32 else np.float64)
    assert sum(stats) == _tiles(nd, order, npts), stats
    for e, pat in enumerate(_patterns(nd, order)):
        if e == 0:
            want = _single(nodes, axes, None, real32)
            # real64: the project's bar.  REAL32: each side is its double sum rounded to float32, and two sums 1e-10 apart
            # can round to neighbouring float32 numbers: one unit in the last place, 2^-23 = 1.2e-7 of the value
            assert relmax(got[0], want) <= (1.2e-7 if real32 else 1e-10), relmax(got[0], want)
        else:
            want = _single(nodes, axes, pat, real32)
            assert np.array_equal(got[e], want), (e, pat, np.max(np.abs(got[e] - want)))
    return stats


SMALL = [
    ((16,), (257,)),                     # 1-D: every tile gathers
    ((5, 12), (70, 33)),                 # a dimension below 8 nodes
    ((12, 10, 8), (37, 29, 19)),         # partial tiles
    ((12, 10, 8), (3, 50, 2)),           # coarse: the windows do not overlap
    ((12, 10, 8), (1, 1, 1)),            # a single point
    ((6, 5, 7, 4), (9, 7, 5, 11)),       # 4-D
]


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("nodes,npts", SMALL, ids=lambda v: "x".join(map(str, v)))
def test_grid_derivs_planes_equal_single_pattern_route_small_shapes(nodes, npts, order):
    _check_against_single_route(nodes, npts, "awkward", order)


@pytest.mark.gpu
@pytest.mark.parametrize("nodes,npts", SMALL, ids=lambda v: "x".join(map(str, v)))
def test_grid_derivs_value_plane_is_the_same_for_both_orders_small_shapes(nodes, npts):
    p1, p2 = _fused_cached(nodes, npts, "awkward", 1)[0], _fused_cached(nodes, npts, "awkward", 2)[0]
    assert np.array_equal(p1[0], p2[0])
    assert np.array_equal(p1[1:], p2[1:1 + len(nodes)])          # and so is the gradient


TILED = [((24, 24, 24), (96, 96, 96)), ((12, 12, 12, 12), (24, 24, 24, 24))]


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("real32", [False, True], ids=["real64", "real32"])
@pytest.mark.parametrize("nodes,npts", TILED, ids=["3d", "4d"])
def test_grid_derivs_tile_path_engages_and_equals_single_pattern_route(nodes, npts, real32, order):
    """Monotone axes of about four (3-D) / two (4-D) points per cell: every tile takes the LDS form."""
    stats = _check_against_single_route(nodes, npts, "monotone", order, real32)
    assert stats == (_tiles(len(nodes), order, npts), 0), stats
    if order == 2:
        assert np.array_equal(_fused_cached(nodes, npts, "monotone", 1, real32)[0][0], _fused_cached(nodes, npts, "monotone", 2, real32)[0][0])


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("real32", [False, True], ids=["real64", "real32"])
@pytest.mark.parametrize("nodes,npts", TILED, ids=["3d", "4d"])
def test_grid_derivs_general_form_equals_lds_form_bit_for_bit(nodes, npts, real32, order):
    """Axis 1 reversed and axis 2 shuffled send tiles to the general form: every plane, plane 0 included, is the monotone
    (all-LDS) result permuted accordingly."""
    nd = len(nodes)
    mono, rc, stats = _fused_cached(nodes, npts, "monotone", order, real32)
    got, rc2, stats2 = _fused_cached(nodes, npts, "permuted", order, real32)
    assert rc == 0 and rc2 == 0 and stats[1] == 0
    assert sum(stats2) == _tiles(nd, order, npts) and stats2[1] > 0, stats2
    perm = np.random.default_rng(9).permutation(npts[1])
    shape = (_nplanes(nd, order),) + tuple(npts[::-1])
    assert np.array_equal(got.reshape(shape), mono.reshape(shape)[..., perm, ::-1])


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 2])
def test_grid_derivs_padded_ldout_leaves_the_gaps_alone(order):
    nodes, npts = (12, 10, 8), (37, 29, 19)
    axes = _axes("awkward", nodes, npts)
    nout, npl = int(np.prod(npts)), _nplanes(3, order)
    got, rc, _, whole = _fused(nodes, axes, order, pad=5, guard=64)
    assert rc == 0
    assert np.array_equal(got, _fused_cached(nodes, npts, "awkward", order)[0])
    assert not np.any(np.isnan(got))
    assert np.all(np.isnan(whole[:npl * (nout + 5)].reshape(npl, nout + 5)[:, nout:]))
    assert np.all(np.isnan(whole[npl * (nout + 5):])) and whole.size == npl * (nout + 5) + 64


@pytest.mark.gpu
def test_grid_derivs_host_entry_equals_device_entry():
    nodes, npts = (12, 10, 8), (37, 29, 19)
    axes = _axes("awkward", nodes, npts)
    for order in (1, 2):
        host, rch = capi.evaluate_grid_derivs(3, axes, order, _coef(nodes), LO[:3], HI[:3], nodes)
        assert rch == 0 and host.shape == (_nplanes(3, order),) + npts[::-1]
        assert np.array_equal(host.reshape(host.shape[0], -1), _fused_cached(nodes, npts, "awkward", order)[0])
    h32, rc32 = capi.evaluate_grid_derivs(3, axes, 2, _coef(nodes), LO[:3], HI[:3], nodes, real32=True)
    d32 = _fused_cached(nodes, npts, "awkward", 2, True)[0]
    assert rc32 == 0 and h32.dtype == np.float32 and np.array_equal(h32.reshape(10, -1), d32)


@pytest.mark.gpu
@pytest.mark.parametrize("real32", [False, True], ids=["real64", "real32"])
def test_grid_derivs_host_entry_with_padded_ldout_leaves_the_gaps_alone(real32):
    """The host entries themselves (capi.evaluate_grid_derivs always passes a tight ldout): six planes ldout = points + 5 apart
    into a NaN-filled buffer equal the device entry's bit for bit; the words between and behind the planes stay NaN."""
    nodes, npts, order, pad, guard = (6, 5), (5, 3), 2, 5, 16
    axes = _axes("awkward", nodes, npts, real32)
    dt, rp = (np.float32, capi._fp) if real32 else (np.float64, capi._dp)
    nout, npl = int(np.prod(npts)), _nplanes(2, order)
    assert npl == 6
    n64 = np.asarray(npts, dtype=np.int64)
    cat, coef = np.concatenate(axes).astype(dt), _coef(nodes, real32)
    lo, hi, nod = np.asarray(LO[:2], dtype=dt), np.asarray(HI[:2], dtype=dt), np.asarray(nodes, dtype=np.int32)
    whole = np.full(npl * (nout + pad) + guard, np.nan, dtype=dt)
    fn = capi.lib().splpak_eval_grid_derivs_f32 if real32 else capi.lib().splpak_eval_grid_derivs_f64
    rc = fn(2, capi._p(n64, LP), capi._p(cat, rp), order, capi._p(coef, rp), capi._p(lo, rp), capi._p(hi, rp), capi._p(nod, capi._ip),
            capi._p(whole, rp), nout + pad)
    assert rc == 0
    planes = whole[:npl * (nout + pad)].reshape(npl, nout + pad)
    assert np.array_equal(planes[:, :nout], _fused_cached(nodes, npts, "awkward", order, real32)[0])
    assert np.all(np.isnan(planes[:, nout:]))
    assert np.all(np.isnan(whole[npl * (nout + pad):])) and whole.size == npl * (nout + pad) + guard


@pytest.mark.gpu
def test_grid_derivs_on_a_side_stream():
    """Asynchronous on the caller's stream: synchronising THAT stream alone is enough."""
    import torch
    nodes, npts = (24, 24, 24), (96, 96, 96)
    ref, _, stats = _fused_cached(nodes, npts, "monotone", 2)
    assert stats[1] == 0
    side = torch.cuda.Stream()
    got, rc, _, _ = _fused(nodes, _axes("monotone", nodes, npts), 2, stream=side)
    assert rc == 0 and np.array_equal(got, ref)


@pytest.mark.gpu
def test_grid_derivs_against_the_oracle(port):
    """One check against the reference algorithm itself (oracle port of splde), every plane at the project's bar."""
    nodes, npts = (12, 10, 8), (37, 29, 19)
    got, rc, _ = _fused_cached(nodes, npts, "awkward", 2)
    q = _product(_axes("awkward", nodes, npts))
    assert rc == 0
    for e, pat in enumerate(_patterns(3, 2)):
        vo, eo = port.evaluate(3, q, pat, _coef(nodes), LO[:3], HI[:3], list(nodes))
        assert eo == 0
        assert relmax(got[e], vo) <= 1e-10, (e, pat, relmax(got[e], vo))


@pytest.mark.gpu
def test_grid_derivs_against_the_point_entry():
    """The same planes from splpak_eval_derivs_dev_f64 on the Cartesian product as a query list."""
    import torch
    nodes, npts = (12, 10, 8), (37, 29, 19)
    got, rc, _ = _fused_cached(nodes, npts, "awkward", 2)
    dev = torch.device("cuda", 0)
    q = torch.from_numpy(_product(_axes("awkward", nodes, npts))).to(dev)
    coef = torch.from_numpy(_coef(nodes)).to(dev)
    out = torch.full((q.shape[0], 10), float("nan"), dtype=torch.float64, device=dev)
    rcp = capi.evaluate_derivs_dev(3, q, 2, coef, LO[:3], HI[:3], nodes, out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = out.cpu().numpy().T
    assert rc == 0 and rcp == 0
    for e in range(10):
        assert relmax(got[e], want[e]) <= 1e-10, (e, relmax(got[e], want[e]))
