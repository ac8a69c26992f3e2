"""Integrals of the fit over the cells of a tensor grid (splpak_integrate_grid_*, csrc/integrategrid.hip).

Yardstick on the GPU: the oracle's point evaluation (oracle.binding.Port().evaluate) under a quadrature built here in numpy --
every cell split at the node lines, two Gauss-Legendre points per piece and dimension, the oracle at the tensor of them, summed
with the product weights.  The fit is a cubic on every node cell and a straight line outside the grid, so the rule is exact;
on the CPU it agrees with the five-point rule to 7e-16 of the summed terms.  Error measure: S = max over the cells of
sum |w_q f(x_q)|, err = max_j |out_j - ref_j| / S, bar 1e-10 (the project's parity bar).  Coefficients are seeded random
normals; no fit is involved.

CPU tier: exports and the host-side argument checks, all of which return before any device call.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from splpak_amd import capi

LP = C.POINTER(C.c_int64)
BAR = 1e-10


# ---------------------------------------------------------------------------------------------------------------
# CPU tier
def _host_call(ndim, ncell, nodes, xmin, xmax, out, axes=None, coef=None, mode=None):
    ncell = np.asarray(ncell, dtype=np.int64)
    nodes = np.asarray(nodes, dtype=np.int32)
    xmin = np.asarray(xmin, dtype=np.float64)
    xmax = np.asarray(xmax, dtype=np.float64)
    axes = np.full(max(int(np.sum(np.abs(ncell) + 1)), 1), 0.3) if axes is None else axes
    coef = np.ones(max(int(np.prod(np.maximum(nodes, 1))), 1)) if coef is None else coef
    md = None if mode is None else np.asarray(mode, dtype=np.int32)
    return capi.lib().splpak_integrate_grid_f64(ndim, capi._p(ncell, LP), capi._p(md, capi._ip), capi._p(axes, capi._dp),
                                                capi._p(coef, capi._dp), capi._p(xmin, capi._dp), capi._p(xmax, capi._dp),
                                                capi._p(nodes, capi._ip), capi._p(out, capi._dp))


def test_integrate_symbols_are_exported():
    L = capi.lib()
    for name in ("splpak_integrate_grid_f64", "splpak_integrate_grid_f32", "splpak_integrate_grid_dev_f64",
                 "splpak_integrate_grid_dev_f32", "splpak_debug_integrate_grid_stats"):
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS
    assert callable(capi.integrate_grid) and callable(capi.integrate_grid_dev) and callable(capi.debug_integrate_grid_stats)


def test_integrate_validation_zeroes_out_without_gpu():
    """101/102/103 are decided on the host and zero `out`; 101 has no shape, so one output."""
    out = np.full(12, 7.0)
    assert _host_call(0, [3, 4], [8, 8], [0, 0], [1, 1], out) == 101
    assert out[0] == 0.0 and np.all(out[1:] == 7.0)
    out = np.full(12, 7.0)
    assert _host_call(2, [3, 4], [8, 3], [0, 0], [1, 1], out) == 102
    assert np.all(out == 0.0)
    out = np.full(13, 7.0)
    assert _host_call(2, [3, 4], [8, 8], [0, 0.5], [1, 0.5], out, mode=[1, 0]) == 103
    assert np.all(out[:12] == 0.0) and out[12] == 7.0
    # the first failing check wins, as in the grid entries
    assert _host_call(0, [3, 4], [8, 3], [0, 0], [1, 1], np.zeros(12)) == 101
    # the Python wrapper reports them too: 3 and 4 cells from 4 and 5 edges
    v, rc = capi.integrate_grid(2, [np.zeros(4), np.zeros(5)], None, np.ones(24), [0, 0], [1, 1], [8, 3])
    assert rc == 102 and v.shape == (4, 3) and np.all(v == 0.0)
    v, rc = capi.integrate_grid(2, [np.zeros(4), np.zeros(5)], [1, 0], np.ones(24), [0, 0], [1, 1], [8, 3])
    assert rc == 102 and v.shape == (5, 3)


def test_integrate_bad_shapes_without_gpu():
    out = np.full(12, 7.0)
    assert _host_call(2, [3, -4], [8, 8], [0, 0], [1, 1], out) == capi.E_BADARG
    assert _host_call(2, [2 ** 40, 2 ** 40], [8, 8], [0, 0], [1, 1], out, axes=np.zeros(1)) == capi.E_BADARG      # product beyond int64
    assert _host_call(2, [3, 4], [8, 8], [0, 0], [1, 1], out, mode=[1, 2]) == capi.E_BADARG
    assert _host_call(2, [3, 4], [8, 8], [0, 0], [1, 1], out, mode=[-1, 0]) == capi.E_BADARG
    assert np.all(out == 7.0)
    # a bad mode comes before 102 / 103, with the counts
    assert _host_call(2, [3, 4], [8, 3], [0, 0], [1, 1], out, mode=[1, 2]) == capi.E_BADARG
    assert np.all(out == 7.0)
    assert _host_call(5, [2] * 5, [4] * 5, [0] * 5, [1] * 5, out) == capi.E_UNSUPPORTED
    assert np.all(out == 7.0)
    # a count of 0: the validation status, nothing written
    assert _host_call(2, [3, 0], [8, 8], [0, 0], [1, 1], out) == 0
    assert _host_call(2, [0, 4], [8, 8], [0, 0], [1, 1], out, mode=[0, 1]) == 0
    assert _host_call(2, [3, 0], [8, 3], [0, 0], [1, 1], out) == 102
    assert np.all(out == 7.0)
    # null pointers
    L = capi.lib()
    ncell = np.array([3, 4], dtype=np.int64)
    assert L.splpak_integrate_grid_f64(2, capi._p(ncell, LP), None, None, None, None, None, None, None) == capi.E_BADARG
    nodes = np.array([8, 8], dtype=np.int32)
    lo, hi = np.zeros(2), np.ones(2)
    assert L.splpak_integrate_grid_f64(2, None, None, None, None, capi._p(lo, capi._dp), capi._p(hi, capi._dp),
                                       capi._p(nodes, capi._ip), None) == capi.E_BADARG
    assert L.splpak_integrate_grid_f64(2, capi._p(ncell, LP), None, None, None, capi._p(lo, capi._dp), capi._p(hi, capi._dp),
                                       capi._p(nodes, capi._ip), capi._p(out, capi._dp)) == capi.E_BADARG
    assert np.all(out == 7.0)
    assert L.splpak_debug_integrate_grid_stats(None) == capi.E_BADARG


# ---------------------------------------------------------------------------------------------------------------
# The yardstick
# Box of every case (that of test_eval_grid.py): bounds exact in single precision, so that the REAL32 entries see the same grid.
LO, HI = [-1.25, 0.0, 2.0, -0.5], [3.5, 1.0, 2.75, 0.25]
GAUSS = {2: ([-1.0 / np.sqrt(3.0), 1.0 / np.sqrt(3.0)], [1.0, 1.0]),
         5: np.polynomial.legendre.leggauss(5)}


def _breakpoints(d, nod):
    return LO[d] + np.arange(nod) * ((HI[d] - LO[d]) / (nod - 1))


def _pieces(d, nod, a, b):
    """Bounds of the pieces of the cell a .. b: cut at the node lines strictly inside it."""
    lo, hi = min(a, b), max(a, b)
    bp = _breakpoints(d, nod)
    return np.concatenate([[lo], bp[(bp > lo) & (bp < hi)], [hi]])


def _axis_rule(d, nod, axis, integrated, npt=2):
    """-> (points, matrix M of shape (outputs, points)): output j of the axis is sum_q M[j, q] f(.., x_q, ..)."""
    if not integrated:
        return np.asarray(axis, dtype=np.float64), np.eye(len(axis))
    t, w = GAUSS[npt]
    xs, rows, ws = [], [], []
    for j in range(len(axis) - 1):
        a, b = float(axis[j]), float(axis[j + 1])
        sign = 1.0 if b >= a else -1.0
        cuts = _pieces(d, nod, a, b)
        for u, v in zip(cuts[:-1], cuts[1:]):
            m, h = 0.5 * (u + v), 0.5 * (v - u)
            for tq, wq in zip(t, w):
                xs.append(m + h * tq)
                ws.append(sign * h * wq)
                rows.append(j)
    M = np.zeros((len(axis) - 1, len(xs)))
    M[rows, np.arange(len(xs))] = ws
    return np.array(xs), M


def _product(axes):
    """The Cartesian product as a query list, dimension 1 fastest (the ordering of `out`)."""
    mesh = np.meshgrid(*axes[::-1], indexing="ij")
    return np.stack([m.ravel() for m in mesh[::-1]], axis=1)


def _yardstick(port, nodes, axes, mode, coef, npt=2, limit=None):
    """-> (reference of shape ncell[::-1], S, oracle queries)"""
    nd = len(nodes)
    mode = [1] * nd if mode is None else mode
    rules = [_axis_rule(d, nodes[d], axes[d], mode[d] == 1, npt) for d in range(nd)]
    pts = [r[0] for r in rules]
    nq = int(np.prod([p.size for p in pts]))
    assert limit is None or nq <= limit, (nq, limit)
    f, eo = port.evaluate(nd, _product(pts), None, coef, LO[:nd], HI[:nd], list(nodes))
    assert eo == 0
    f = np.asarray(f).reshape([p.size for p in pts][::-1])         # C-ordered: the last index runs along dimension 1
    ref, mag = f, np.abs(f)
    for d in range(nd):                                            # dimension d is array axis nd - 1 - d
        M = rules[d][1]
        ax = nd - 1 - d
        ref = np.moveaxis(np.tensordot(ref, M, axes=([ax], [1])), -1, ax)
        mag = np.moveaxis(np.tensordot(mag, np.abs(M), axes=([ax], [1])), -1, ax)
    return ref, float(np.max(mag)), nq


@functools.lru_cache(maxsize=None)
def _coef(nodes, real32=False):
    c = np.random.default_rng(sum(nodes) + len(nodes)).standard_normal(int(np.prod(nodes)))
    return c.astype(np.float32) if real32 else c


def _rich_edges(rng, d, nod, n):
    """The first integrated axis of a case, n >= 9 cells.  Unsorted runs of cells, one run backwards; a tenth of the edges
    (at least one) outside the box on each side; cell 0 from 0.7 box lengths below xmin to 0.3 above xmax (nodes + 1 pieces);
    cell 2 empty (a repeated edge); cells 4 and 5 the same interval there and back; edges exactly on xmin, on xmax and on a
    node (on two nodes where there is room)."""
    lo, hi = LO[d], HI[d]
    w = hi - lo
    bp = _breakpoints(d, nod)
    k = max((n + 1) // 10, 1)
    x = np.sort(np.concatenate([rng.uniform(lo - 0.3 * w, lo, k), rng.uniform(hi, hi + 0.3 * w, k), rng.uniform(lo, hi, n + 1 - 2 * k)]))
    runs = np.array_split(x, 4)
    x = np.concatenate([runs[2], runs[0], runs[3][::-1], runs[1]])
    a, b = x[5], x[6]
    x[:7] = [lo - 0.7 * w, hi + 0.3 * w, x[2], x[2], a, b, a]
    special = [hi, bp[nod // 2], lo, bp[1]][:min(4, n - 6)]
    x[7 + rng.choice(n - 6, len(special), replace=False)] = special
    return x


def _span_edges(rng, d, nod, n):
    """A further integrated axis with n >= 8 cells: an edge outside the box on each side, xmin (twice: an empty cell on it),
    xmax and a node, the rest inside; ascending to the middle, then from the far end back down, so that the cell in the
    middle jumps over half the box and every cell behind it is reversed.  About n + 1.5 nodes pieces."""
    lo, hi = LO[d], HI[d]
    w = hi - lo
    x = np.sort(np.concatenate([[lo - 0.1 * w, lo, lo, _breakpoints(d, nod)[nod // 2], hi, hi + 0.1 * w], rng.uniform(lo, hi, n - 5)]))
    h = (n + 1) // 2
    return np.concatenate([x[:h], x[h:][::-1]])


def _end_edges(rng, d, nod, n):
    """A further integrated axis with few cells (the 4-D cases, where the oracle's load allows little more than a piece per
    cell): all at one end of the box, the upper end in dimensions 2 and 4 and the lower in dimension 3.  From xmax (xmin) a
    tenth outside, back across it into the last (first) node cell, an empty cell there, onto the node line, and off it."""
    lo, hi = LO[d], HI[d]
    w = hi - lo
    dx = w / (nod - 1)
    bp = _breakpoints(d, nod)
    end, s, node = (hi, -1.0, bp[nod - 2]) if d % 2 else (lo, 1.0, bp[1])
    t = end + s * dx * np.sort(rng.uniform(0.1, 0.9, 2))
    return np.array([end, end - s * 0.1 * w, t[1], t[1], node, t[0]][:n + 1])


def _points(rng, d, nod, n):
    """An evaluated axis: unsorted coordinates from a tenth below xmin to a tenth above xmax; first one above, xmin, a node,
    xmax and one below, as many of them as the axis has room for."""
    lo, hi = LO[d], HI[d]
    w = hi - lo
    x = rng.uniform(lo - 0.1 * w, hi + 0.1 * w, n)
    special = [hi + 0.1 * w, lo, _breakpoints(d, nod)[nod // 2], hi, lo - 0.1 * w][:n]
    x[:len(special)] = special
    return x


def _case_axes(seed, nodes, ncell, mode=None):
    """Which axis gets which edges depends on the shape alone, never on the seed."""
    mode = [1] * len(nodes) if mode is None else mode
    first = mode.index(1) if 1 in mode else -1
    axes = []
    for d, (nod, n, m) in enumerate(zip(nodes, ncell, mode)):
        rng = np.random.default_rng(seed + 7 * d)
        if not m:
            axes.append(_points(rng, d, nod, n))
        elif d == first:
            assert n >= 9
            axes.append(_rich_edges(rng, d, nod, n))
        else:
            assert 3 <= n
            axes.append(_span_edges(rng, d, nod, n) if n >= 8 else _end_edges(rng, d, nod, n))
    return axes


def _exact_cells(got, axes, mode):
    """On every integrated axis: an empty cell is 0, and a cell taken there and back is the exact negation.
    -> (empty cells, there-and-back pairs) checked per dimension"""
    nd = len(axes)
    seen = []
    for d, (e, m) in enumerate(zip(axes, mode)):
        if not m:
            seen.append((0, 0))
            continue
        g = np.moveaxis(got, nd - 1 - d, 0)
        empty = [j for j in range(e.size - 1) if e[j] == e[j + 1]]
        back = [j for j in range(e.size - 2) if e[j] == e[j + 2] and e[j] != e[j + 1]]
        for j in empty:
            assert np.all(g[j] == 0.0), (d, j)
        for j in back:
            assert np.array_equal(g[j + 1], -g[j]), (d, j)
        seen.append((len(empty), len(back)))
    return seen


# ---------------------------------------------------------------------------------------------------------------
# GPU tier
def _dev_route(nodes, axes, mode, real32=False, stream=None, coef=None):
    """-> (values of shape ncell[::-1], ierror, stats)"""
    import torch
    nd = len(nodes)
    dt = torch.float32 if real32 else torch.float64
    dev = torch.device("cuda", 0)
    md = [1] * nd if mode is None else mode
    ncell = [a.size - m for a, m in zip(axes, md)]
    a = torch.from_numpy(np.concatenate(axes)).to(dev).to(dt)
    c = torch.from_numpy(_coef(tuple(nodes), real32) if coef is None else coef).to(dev)
    out = torch.full((int(np.prod(ncell)),), float("nan"), dtype=dt, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream() if stream is None else stream
    rc = capi.integrate_grid_dev(nd, ncell, mode, a, c, LO[:nd], HI[:nd], nodes, out, st.cuda_stream)
    st.synchronize()
    return out.cpu().numpy().reshape(ncell[::-1]), rc, capi.debug_integrate_grid_stats()


def _err(got, ref, S):
    return float(np.max(np.abs(got - ref)) / S)


CASES = [
    # nodes, cells, mode, oracle queries allowed
    ((9,), (40,), None, 10 ** 5),
    ((8, 5), (70, 19), None, 10 ** 5),
    ((8, 6, 4), (70, 9, 11), None, 5 * 10 ** 5),          # crosses the 64 x 8 x 8 tile in every dimension
    ((4, 5, 4, 6), (18, 5, 3, 5), None, 10 ** 5),
    ((8, 6, 4), (70, 9, 11), [1, 0, 1], 5 * 10 ** 5),
    ((8, 6, 4), (70, 9, 11), [0, 1, 0], 5 * 10 ** 5),
    ((4, 5, 4, 6), (18, 5, 3, 5), [1, 1, 0, 1], 10 ** 5),
]


def _case_id(v):
    return "x".join(map(str, v)) if isinstance(v, (tuple, list)) else str(v)


@pytest.mark.gpu
@pytest.mark.parametrize("nodes,ncell,mode,limit", CASES, ids=_case_id)
def test_integrals_against_the_oracle_quadrature(port, nodes, ncell, mode, limit):
    axes = _case_axes(len(nodes) * 100 + sum(ncell), nodes, ncell, mode)
    ref, S, nq = _yardstick(port, nodes, axes, mode, _coef(nodes), limit=limit)
    got, rc, stats = _dev_route(nodes, axes, mode)
    assert rc == 0
    assert got.shape == ref.shape == tuple(ncell[::-1])
    err = _err(got, ref, S)
    print(f"integrate {_case_id(nodes)} cells {_case_id(ncell)} mode {mode}: err {err:.2e}, S {S:.3e}, {nq} oracle queries, "
          f"pieces {stats[2:6]}")
    assert err <= BAR, err
    md = [1] * len(nodes) if mode is None else mode
    seen = _exact_cells(got, axes, md)
    for d in range(len(nodes)):                            # every integrated axis has an empty cell, the first a there-and-back pair
        assert not md[d] or seen[d][0] >= 1, (d, seen)
    r = md.index(1)
    assert seen[r][1] >= 1 and axes[r][2] == axes[r][3] and axes[r][4] == axes[r][6]
    assert stats[2 + r] >= ncell[r] + nodes[r]             # its cell 0 alone has nodes + 1 pieces
    assert stats[6] == sum(md) * stats[0]


@pytest.mark.gpu
def test_edges_one_ulp_from_the_node_lines(port):
    """Cells that end one ulp below, on and one ulp above every node line, and cells one and two ulps wide across it: the
    window of a piece comes from its region, so a sliver next to a breakpoint adds (almost) nothing and nothing twice."""
    nodes = (9,)
    bp = _breakpoints(0, 9)
    e = []
    for b in bp:
        e += [b - 0.3, np.nextafter(b, -np.inf), b, np.nextafter(b, np.inf), np.nextafter(b, -np.inf), b + 0.3, b]
    axes = [np.array(e)]
    ref, S, nq = _yardstick(port, nodes, axes, None, _coef(nodes), limit=10 ** 5)
    got, rc, stats = _dev_route(nodes, axes, None)
    err = _err(got, ref, S)
    print(f"integrate 9 with edges one ulp from the node lines: err {err:.2e}, {nq} oracle queries, pieces {stats[2:6]}")
    assert rc == 0 and err <= BAR, err


@pytest.mark.gpu
def test_one_box_over_the_whole_grid(port):
    nodes = (12, 10, 9)
    axes = [np.array([LO[d], HI[d]]) for d in range(3)]
    ref, S, nq = _yardstick(port, nodes, axes, None, _coef(nodes), limit=5 * 10 ** 5)
    got, rc, stats = _dev_route(nodes, axes, None)
    err = _err(got, ref, S)
    print(f"integrate one box over {_case_id(nodes)}: err {err:.2e}, {nq} oracle queries, pieces {stats[2:6]}")
    assert rc == 0 and got.shape == (1, 1, 1) and err <= BAR, err
    # the same through the host entry, and taken the other way round in two dimensions: the same bits
    host, rch = capi.integrate_grid(3, axes, None, _coef(nodes), LO[:3], HI[:3], nodes)
    assert rch == 0 and np.array_equal(host, got)
    back, _, _ = _dev_route(nodes, [axes[0][::-1].copy(), axes[1], axes[2][::-1].copy()], None)
    assert np.array_equal(back, got)
    neg, _, _ = _dev_route(nodes, [axes[0], axes[1][::-1].copy(), axes[2]], None)
    assert np.array_equal(neg, -got)


@pytest.mark.gpu
@pytest.mark.parametrize("real32", [False, True], ids=["real64", "real32"])
def test_mode_all_zero_is_evaluate_grid_to_the_bit(real32):
    import torch
    nodes, npts = (8, 6, 4), (70, 9, 11)
    axes = _case_axes(11, nodes, npts, [0, 0, 0])
    if real32:
        axes = [a.astype(np.float32).astype(np.float64) for a in axes]
    got, rc, stats = _dev_route(nodes, axes, [0, 0, 0], real32)
    dev = torch.device("cuda", 0)
    dt = torch.float32 if real32 else torch.float64
    a = torch.from_numpy(np.concatenate(axes)).to(dev).to(dt)
    c = torch.from_numpy(_coef(nodes, real32)).to(dev)
    want = torch.full((int(np.prod(npts)),), float("nan"), dtype=dt, device=dev)
    rcw = capi.evaluate_grid_dev(3, list(npts), a, None, c, LO[:3], HI[:3], nodes, want, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and rcw == 0
    assert got.dtype == (np.float32 if real32 else np.float64)
    assert np.array_equal(got.ravel(), want.cpu().numpy())
    assert stats[:2] == (1, 0) and stats[2:5] == npts and stats[6] == 0


@pytest.mark.gpu
def test_real32_is_one_rounding_of_the_real64_entry():
    """Storage f32, edges and coefficients widened first, every intermediate double, one rounding at the final store."""
    nodes, ncell, mode = (8, 6, 4), (70, 9, 11), [1, 0, 1]
    axes = [a.astype(np.float32).astype(np.float64) for a in _case_axes(13, nodes, ncell, mode)]
    c32 = _coef(nodes, True)
    got, rc, _ = _dev_route(nodes, axes, mode, real32=True)
    wide, rcw, _ = _dev_route(nodes, axes, mode, coef=c32.astype(np.float64))
    assert rc == 0 and rcw == 0 and got.dtype == np.float32
    assert np.array_equal(got, wide.astype(np.float32))


@pytest.mark.gpu
def test_side_stream_equals_host_entry():
    import torch
    nodes, ncell, mode = (8, 6, 4), (70, 9, 11), [1, 1, 0]
    axes = _case_axes(17, nodes, ncell, mode)
    host, rch = capi.integrate_grid(3, axes, mode, _coef(nodes), LO[:3], HI[:3], nodes)
    side = torch.cuda.Stream()
    got, rc, _ = _dev_route(nodes, axes, mode, stream=side)
    assert rc == 0 and rch == 0 and host.shape == ncell[::-1]
    assert np.array_equal(got, host)
    h32, rc32 = capi.integrate_grid(3, axes, mode, _coef(nodes), LO[:3], HI[:3], nodes, real32=True)
    d32, _, _ = _dev_route(nodes, [a.astype(np.float32).astype(np.float64) for a in axes], mode, real32=True, stream=side)
    assert rc32 == 0 and h32.dtype == np.float32 and np.array_equal(h32, d32)


@pytest.mark.gpu
def test_slabs_do_not_change_the_bits():
    """Sorted edges strictly between the breakpoints: the pieces of an axis are its cells + the node lines inside its range."""
    nodes, ncell = (12, 10, 9), (60, 50, 40)
    rng = np.random.default_rng(23)
    axes, pieces = [], []
    for d, (nod, n) in enumerate(zip(nodes, ncell)):
        bp = _breakpoints(d, nod)
        w = HI[d] - LO[d]
        e = np.sort(rng.uniform(LO[d] - 0.05 * w, HI[d] + 0.05 * w, n + 1))
        assert np.min(np.abs(e[:, None] - bp[None, :])) > 1e-9 * w
        axes.append(e)
        pieces.append(n + int(np.sum((bp > e[0]) & (bp < e[-1]))))
    ref, rc, stats = _dev_route(nodes, axes, None)
    assert rc == 0 and stats[0] == 1 and stats[2:5] == tuple(pieces) and stats[5] == 0 and stats[6] == 3 and stats[7] == 0
    assert stats[1] == pieces[0] * pieces[1] * pieces[2] + ncell[0] * pieces[1] * pieces[2]
    capi.set_default_option("integrate_scratch_mb", "1")
    try:
        got, rc1, stats1 = _dev_route(nodes, axes, None)
    finally:
        capi.set_default_option("integrate_scratch_mb", None)
    assert rc1 == 0 and stats1[0] >= 2, stats1
    assert stats1[1] * 8 <= 1 << 20 and stats1[2:6] == stats[2:6] and stats1[6] == 3 * stats1[0]
    assert np.array_equal(got, ref)
