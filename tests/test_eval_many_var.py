"""The prediction variance of a batch of small fits at each problem's own points (splpak_eval_many_var_*; csrc/evalmany.hip,
csrc/evalmanyapi.hip): out[i] = a^T Z a with a the window row splpak_eval_many_* forms for query i and Z the half stencil
splpak_fit_many_cov_* wrote for the problem that owns i.

Yardstick: Zref of tests/test_fit_many_cov.py (the long-double inverse of the oracle's normal equations) and the rows a from the
oracle: column j of the row matrix is port.evaluate of the j-th unit coefficient vector, so a is the oracle's own factor table
product for the same nderiv.  Bar: with s = (sum_j |a_j| sqrt(Zref_jj))^2, |out - a^T Zref a| <= (16 eps kappa_s + 1e-14) s.
Where the stencil is arbitrary numbers (the tests of the owner search) the quadratic form is restated in long double from the
same stencil, bar 1e-12 sum |a_p| |Z_pq| |a_q| (136 terms of a few eps each, and rows that differ from the oracle's by rounding).

CPU tier: exports and the ladder rung by rung, every rung decided before any device call.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from splpak_amd import capi
from tests.test_eval_many import E_BADARG, E_UNSUPPORTED, SENT, _dev, _offsets, _queries, _stream, _zeroed_range_only
from tests.test_fit_many import lo_hi
from tests.test_fit_many_cov import (BATCHES, EPS, _batch_args, _port, cov_problem, dense_from_stencil, hst_of, run_cov,
                                     yardstick)
from tests.test_stream_order import _check_late, _Entry, clock, streams  # noqa: F401

SYMBOLS = ("splpak_eval_many_var_f64", "splpak_eval_many_var_f32", "splpak_eval_many_var_dev_f64", "splpak_eval_many_var_dev_f32")
DP, FP, IP, LP = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


# ---------------------------------------------------------------------------------------------------------------
# CPU tier
def test_symbols_exported_and_listed():
    lib = capi.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in capi.SYMBOLS, s


def _arr(v, dt, ty, keep):
    if v is None:
        return None
    a = np.ascontiguousarray(v, dtype=dt)
    keep.append(a)
    return a.ctypes.data_as(ty)


def _var_call(ndim=1, nbatch=3, offsets=(5, 13, 13, 20), xq="ok", ldxq=1, nderiv=None, cov="ok", ldcov=16, xmin=(0.0, 0.0), xmax=(1.0, 1.0),
              nodes=(4, 4), out="ok", real32=False):
    """splpak_eval_many_var_f64 / _f32 on raw arguments -> (rc, out); `out` has 40 entries holding SENT."""
    dt, rp = (np.float32, FP) if real32 else (np.float64, DP)
    keep = []
    o = np.full(40, SENT, dtype=dt)
    fn = capi.lib().splpak_eval_many_var_f32 if real32 else capi.lib().splpak_eval_many_var_f64
    rc = fn(ndim, nbatch, _arr(offsets, np.int64, LP, keep), _arr(np.linspace(0.0, 1.0, 80) if xq == "ok" else xq, dt, rp, keep), ldxq,
            _arr(nderiv, np.int32, IP, keep), _arr(np.ones(2048) if cov == "ok" else cov, dt, rp, keep), ldcov, _arr(xmin, dt, rp, keep),
            _arr(xmax, dt, rp, keep), _arr(nodes, np.int32, IP, keep), o.ctypes.data_as(rp) if out == "ok" else None)
    return rc, o


def test_ladder_in_order_before_any_device_call():
    """The ladder of splpak_eval_many_* with ndim > 2 refused where ndim > 4 is there, ldcov < len where ldcoef < ncol is and cov
    null where coef null is.  101 / 102 / 103 zero exactly [offsets[0], offsets[nbatch]); every other failure writes nothing."""
    late = dict(ldxq=0, ldcov=0, xq=None, cov=None)
    untouched = [
        (E_BADARG, dict(offsets=None, ndim=0)),
        (E_BADARG, dict(nodes=None, ndim=0)),
        (E_BADARG, dict(xmin=None, ndim=0)),
        (E_BADARG, dict(xmax=None, ndim=0)),
        (E_BADARG, dict(nbatch=0, ndim=0)),
        (E_BADARG, dict(offsets=(5, 13, 12, 20), ndim=0)),
        (E_BADARG, dict(offsets=(5, 13, 12, 20), ndim=2, nodes=(3, 3), **late)),
        (E_UNSUPPORTED, dict(ndim=3, nodes=(3,) * 3, xmin=(0,) * 3, xmax=(0,) * 3, **late)),
        (E_UNSUPPORTED, dict(ndim=5, nodes=(3,) * 5, xmin=(0,) * 5, xmax=(0,) * 5, **late)),
        (E_BADARG, dict(ldxq=0, cov=None)),
        (E_BADARG, dict(ndim=2, ldxq=1, ldcov=400, out=None)),
        (E_BADARG, dict(ldcov=15, xq=None)),
        (E_BADARG, dict(ndim=2, ldxq=2, ldcov=399, nderiv=[3, 0])),
        (E_BADARG, dict(xq=None)),
        (E_BADARG, dict(cov=None, nderiv=[3])),
        (E_BADARG, dict(out=None)),
    ]
    for want, kw in untouched:
        rc, o = _var_call(**kw)
        assert rc == want, (want, rc, kw)
        assert np.all(o == SENT), kw
    zeroed = [
        (101, dict(ndim=0, nodes=(3, 3), **late)),
        (102, dict(ndim=2, nodes=(3, 4), xmax=(1.0, 0.0), **late)),
        (102, dict(ndim=1, nodes=(3,), nderiv=[3], **late)),
        (103, dict(ndim=2, nodes=(4, 4), xmax=(1.0, 0.0), **late)),
    ]
    for want, kw in zeroed:
        rc, o = _var_call(**kw)
        assert rc == want, (want, rc, kw)
        assert _zeroed_range_only(o), (kw, o)
        assert _var_call(out=None, **kw)[0] == want      # a null `out` is not written
    rc, o = _var_call(ndim=2, nodes=(4, 4), xmax=(1.0, 0.0), real32=True, **late)
    assert rc == 103 and o.dtype == np.float32 and _zeroed_range_only(o)
    assert capi.debug_eval_many_stats() == (0,) * 8      # a refused call leaves no counters
    # no queries at all: 0, or 104 for an nderiv out of range; nothing is written, no data pointer is looked at
    for nder, want in ((None, 0), ([1], 0), ([3], 104)):
        assert _var_call(offsets=(5, 5, 5, 5), xq=None, cov=None, out=None, nderiv=nder)[0] == want
        rc, o = _var_call(offsets=(5, 5, 5, 5), nderiv=nder)
        assert rc == want and np.all(o == SENT)
    assert capi.debug_eval_many_stats() == (0, 0, 0, 3, 0, 3, 0, 0)
    assert _var_call(offsets=(5, 5, 5, 5), ldcov=15)[0] == E_BADARG      # the leading dimensions come before the empty batch


# ---------------------------------------------------------------------------------------------------------------
# The yardstick's rows
def oracle_rows(nd, nodes, lo, hi, q, pat):
    """A (nq, ncol): row i is the window row of query i, from port.evaluate of the unit coefficient vectors."""
    ncol = int(np.prod(nodes))
    A = np.zeros((q.shape[0], ncol))
    unit = np.zeros(ncol)
    for j in range(ncol):
        unit[j] = 1.0
        A[:, j], rc = _port().evaluate(nd, q, pat if pat is not None else [0] * nd, unit, lo, hi, list(nodes))
        assert rc == 0
        unit[j] = 0.0
    return A


def quadratic_forms(A, Z):
    """(a^T Z a, sum |a_p| |Z_pq| |a_q|) per row of A, in long double."""
    AL = A.astype(np.longdouble)
    return np.einsum("ij,ij->i", AL @ Z, AL), np.einsum("ij,ij->i", np.abs(AL) @ np.abs(Z), np.abs(AL)).astype(np.float64)


def problem_points(name):
    p = cov_problem(name)
    return np.ascontiguousarray(p["x"][:, :p["ndim"]])


# ---------------------------------------------------------------------------------------------------------------
# GPU tier
PATTERNS = {1: [None, [1]], 2: [None, [1, 0], [0, 2]]}


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["n9", "n65", "g59", "g1211"])
def test_variance_matches_the_long_double_inverse(key):
    """Every problem of the batch at its own points, values and one derivative pattern per dimension."""
    names = BATCHES[key]
    nd, off, x, y, w, lo, hi, nodes, xtrap = _batch_args(names)
    cov = run_cov(key)[1]
    q = np.ascontiguousarray(x[:, :nd])
    for pat in PATTERNS[nd]:
        out, rc = capi.evaluate_many_var(nd, off, q, pat, cov, lo, hi, nodes)
        assert rc == 0
        for k, name in enumerate(names):
            a, b = int(off[k]), int(off[k + 1])
            yk = yardstick(name)
            A = oracle_rows(nd, nodes, lo, hi, q[a:b], pat)
            want, _ = quadratic_forms(A, yk["Z"])
            s = (np.abs(A) @ yk["zd"]) ** 2
            bar = (16 * EPS * yk["kappa"] + 1e-14) * s
            err = np.abs(out[a:b] - want.astype(np.float64))
            print(f"{name}, nderiv {pat}: worst |out - a^T Zref a| / bar = {np.max(err / bar):.3e}, variance {out[a:b].min():.3e} .. {out[a:b].max():.3e}")
            assert np.all(err <= bar), (name, pat)
            if pat is None and key != "n9":      # (n9_wide has points beyond the box, where a row may vanish)
                assert np.all(out[a:b] > 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["g59", "w_g59"])
def test_trace_of_the_hat_matrix(name):
    """An identity that needs no oracle: at xtrap = 0, sum_i w_i^2 var(x_i) = trace(A Z A^T W^2) = ncol."""
    k = BATCHES["g59"].index(name)
    nd, off, x, y, w, lo, hi, nodes, xtrap = _batch_args(BATCHES["g59"])
    assert xtrap == 0.0
    out, rc = capi.evaluate_many_var(nd, off, x, None, run_cov("g59")[1], lo, hi, nodes)
    a, b = int(off[k]), int(off[k + 1])
    got = float(np.sum((w[a:b].astype(np.longdouble) ** 2) * out[a:b]))
    tol = (16 * EPS * yardstick(name)["kappa"] + 1e-14) * 45
    print(f"{name}: sum w^2 var = {got:.15f}, ncol 45, tolerance {tol:.2e}")
    assert rc == 0 and abs(got - 45.0) <= tol


def _random_cov(nodes, nbatch, gap=0, dt=np.float64):
    hst = hst_of(len(nodes))
    ln = int(np.prod(nodes)) * hst
    cv = np.full((nbatch, ln + gap), np.nan, dtype=dt)
    cv[:, :ln] = np.random.default_rng(4300 + sum(nodes)).standard_normal((nbatch, ln))
    return cv


def _check_against_restatement(nodes, sizes, pat, first=0, ldxq=None, gap=0, tail=3, variant="dense"):
    """One batch on the device with seeded random stencils (no two problems share one: a wrong owner gives a wrong value)
    against the long-double restatement problem by problem; the sentinel outside [offsets[0], offsets[nbatch])."""
    import torch
    from tests.test_eval_many import _box
    nd, ncol = len(nodes), int(np.prod(nodes))
    off = _offsets(sizes, first)
    n, total = int(off[-1]) - first, int(off[-1]) + tail
    ld = nd if ldxq is None else ldxq
    xq = np.full((total, ld), 1.0e30)
    xq[first:first + n, :nd] = _queries(tuple(nodes), n, variant)
    cv = _random_cov(nodes, len(sizes), gap)
    lo, hi = _box(nodes, variant)
    got = torch.full((total,), SENT, dtype=torch.float64, device="cuda")
    rc = capi.evaluate_many_var_dev(nd, off, _dev(xq), pat, _dev(cv), lo, hi, list(nodes), got, ldxq=ld, stream=_stream())
    stats = capi.debug_eval_many_stats()
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert rc == 0 and stats[1] == 1 and stats[2] == n and stats[3] == len(sizes) and stats[5] == 3, stats
    assert np.all(got[:first] == SENT) and np.all(got[first + n:] == SENT)
    A = oracle_rows(nd, nodes, lo, hi, xq[first:first + n, :nd], pat)
    owner = np.repeat(np.arange(len(sizes)), sizes)
    for k in np.unique(owner):
        Z = dense_from_stencil(nd, nodes, cv[k, :ncol * hst_of(nd)].reshape(ncol, -1))
        sel = np.flatnonzero(owner == k)
        want, mag = quadratic_forms(A[sel], Z)
        err = np.abs(got[first + sel] - want.astype(np.float64))
        assert np.all(err <= 1e-12 * mag), (k, float(np.max(err / mag)))
    return got, off, xq, cv


@pytest.mark.gpu
def test_segment_edges_of_waves_and_problems():
    """Problems that end one short of, on and one past a wave's and a workgroup's edge, empty problems alone and in runs,
    offsets[0] = 5, a padded xq and padded stencil rows (NaN in the gaps): the cases of tests/test_eval_many.py."""
    sizes = [0, 1, 63, 64, 65, 0, 0, 255, 256, 257, 1, 0, 513, 0]
    for pat in (None, [2]):
        _check_against_restatement((9,), sizes, pat, first=5, ldxq=3, gap=3)


@pytest.mark.gpu
def test_many_problems_per_wave():
    """600 problems of 0 .. 3 queries in 1-D and 200 in 2-D: a dozen and more problems in every wave, every lane searches."""
    _check_against_restatement((9,), [k % 4 for k in range(600)], None)
    _check_against_restatement((5, 9), [(k * 7) % 5 for k in range(200)], [0, 1], gap=2, variant="box")


@pytest.mark.gpu
def test_bits_do_not_depend_on_the_batch_the_position_or_the_entry():
    import torch
    nd, off, x, y, w, lo, hi, nodes, xtrap = _batch_args(BATCHES["g59"])
    cov = run_cov("g59")[1]
    out, rc = capi.evaluate_many_var(nd, off, x, None, cov, lo, hi, nodes)
    assert rc == 0 and np.array_equal(out, capi.evaluate_many_var(nd, off, x, None, cov, lo, hi, nodes)[0])
    n = int(off[1])
    for k in (0, 1):      # alone, and the two swapped behind an empty problem at offsets[0] = 3
        a, b = int(off[k]), int(off[k + 1])
        alone, rc = capi.evaluate_many_var(nd, [0, b - a], x[a:b], None, cov[k:k + 1], lo, hi, nodes)
        assert rc == 0 and np.array_equal(alone[:b - a], out[a:b])
    off2 = np.array([3, 3, 3 + n, 3 + 2 * n], dtype=np.int64)
    x2 = np.concatenate([np.zeros((3, 2)), x[n:], x[:n]])
    cov2 = np.stack([np.zeros_like(cov[0]), cov[1], cov[0]])
    out2, rc = capi.evaluate_many_var(nd, off2, x2, None, cov2, lo, hi, nodes)
    assert rc == 0 and np.array_equal(out2[3:3 + n], out[n:]) and np.array_equal(out2[3 + n:], out[:n]) and np.all(out2[:3] == 0.0)
    od = torch.full((out.size,), SENT, dtype=torch.float64, device="cuda")
    assert capi.evaluate_many_var_dev(nd, off, _dev(x), None, _dev(cov), lo, hi, nodes, od, stream=_stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(od.cpu().numpy(), out)
    # REAL32: cov read as float and widened, the sum in double, one rounding at the store
    x32, c32 = x.astype(np.float32), cov.astype(np.float32)
    o32, rc = capi.evaluate_many_var(nd, off, x32, [1, 0], c32, lo, hi, nodes, real32=True)
    o64, rc64 = capi.evaluate_many_var(nd, off, x32.astype(np.float64), [1, 0], c32.astype(np.float64), lo, hi, nodes)
    assert rc == rc64 == 0 and o32.dtype == np.float32 and np.array_equal(o32, o64.astype(np.float32))


@pytest.mark.gpu
def test_dev_entry_zeroes_its_range_on_102_and_103_and_reports_104():
    import torch
    off = _offsets([4, 0, 6], 5)
    q = _dev(np.linspace(0.0, 1.0, 20).reshape(-1, 1))
    cv = _dev(_random_cov((9,), 3))
    for want, kw in ((102, dict(nodes=[3])), (103, dict(hi=[0.0]))):
        out = torch.full((20,), SENT, dtype=torch.float64, device="cuda")
        rc = capi.evaluate_many_var_dev(1, off, q, None, cv, [0.0], kw.get("hi", [1.0]), kw.get("nodes", [9]), out, stream=_stream())
        torch.cuda.synchronize()
        assert rc == want and _zeroed_range_only(out.cpu().numpy(), 5, 15)
    out = torch.full((20,), SENT, dtype=torch.float64, device="cuda")
    clamped = torch.full((20,), SENT, dtype=torch.float64, device="cuda")
    assert capi.evaluate_many_var_dev(1, off, q, [3], cv, [0.0], [1.0], [9], out, stream=_stream()) == 104
    assert capi.evaluate_many_var_dev(1, off, q, [2], cv, [0.0], [1.0], [9], clamped, stream=_stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, clamped) and bool((out[:5] == SENT).all()) and bool((out[15:] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------
# stream order (the harness of tests/test_stream_order.py)
SO_NODES, SO_SIZES = (9,), [300, 0, 1000, 64, 700]


@functools.lru_cache(maxsize=None)
def _so_data(part):
    n = sum(SO_SIZES)
    return {"x": _queries(SO_NODES, 2 * n)[part * n:(part + 1) * n], "cov": np.random.default_rng(9300 + part).standard_normal((len(SO_SIZES), 36))}


@pytest.mark.gpu
def test_evaluate_many_var_dev_with_late_inputs_and_stream_only_read_back(clock, streams):
    """The entry only enqueues: called while its inputs are still being copied behind a delay on the same stream, it returns the
    values of the late inputs, read back by the stream alone."""
    off = _offsets(SO_SIZES)

    def call(t, stream):
        return (capi.evaluate_many_var_dev(1, off, t["x"], None, t["cov"], [0.0], [1.0], list(SO_NODES), t["out"], stream=stream),)
    _check_late(_Entry(call, {"out": (int(off[-1]),)}), dict(_so_data(0)), dict(_so_data(1)), streams, clock, "evaluate_many_var_dev")
