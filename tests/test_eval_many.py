"""A batch of small fits evaluated at each problem's own points, and its residual pass, in one launch
(splpak_eval_many_*, splpak_residuals_many_*; csrc/evalmany.hip, csrc/evalmanyapi.hip).

Yardsticks: the library's single entry splpak_eval_dev_* under EVAL_DIRECT, one call per problem with that problem's
coefficients (bit for bit: the batch entry promises the very value), the oracle's `port.evaluate` (1e-10, the project's parity
bar), and for the statistics a numpy restatement of the stated order of operations (bit for bit: every operation is an IEEE
double operation numpy also has).  Every problem's coefficients are seeded random normals: no two rows are equal, so a wrong
problem gives a wrong value.  Queries come from tests.cases.make_queries (beyond the box, xmin, xmax and exact node positions).

CPU tier: exports and both argument ladders rung by rung, every rung decided before any device call.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from splpak_amd import capi
from tests import cases
from tests.conftest import ROOT, relmax
from tests.test_fit_many import lo_hi, pack, problem
from tests.test_stream_order import (T_FLOOR_MS, _check_control, _check_late, _Entry, _yardsticks, clock,  # noqa: F401
                                     streams)

SYMBOLS = ("splpak_eval_many_f64", "splpak_eval_many_f32", "splpak_eval_many_dev_f64", "splpak_eval_many_dev_f32",
           "splpak_residuals_many_f64", "splpak_residuals_many_f32", "splpak_residuals_many_dev_f64", "splpak_residuals_many_dev_f32",
           "splpak_debug_eval_many_stats")
E_BADARG, E_UNSUPPORTED = -3, -4
SENT = 777.0
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


def _eval_call(ndim=1, nbatch=3, offsets=(5, 13, 13, 20), xq="ok", ldxq=1, nderiv=None, coef="ok", ldcoef=16, xmin=(0.0, 0.0), xmax=(1.0, 1.0),
               nodes=(4, 4), out="ok", real32=False):
    """splpak_eval_many_f64 / _f32 on raw arguments -> (rc, out); "ok": a valid array, None: a null pointer.  `out` has 40
    entries holding SENT."""
    dt, rp = (np.float32, FP) if real32 else (np.float64, DP)
    keep = []
    o = np.full(40, SENT, dtype=dt)
    fn = capi.lib().splpak_eval_many_f32 if real32 else capi.lib().splpak_eval_many_f64
    rc = fn(ndim, nbatch, _arr(offsets, np.int64, LP, keep), _arr(np.linspace(0.0, 1.0, 80) if xq == "ok" else xq, dt, rp, keep), ldxq,
            _arr(nderiv, np.int32, IP, keep), _arr(np.ones(64) if coef == "ok" else coef, dt, rp, keep), ldcoef, _arr(xmin, dt, rp, keep),
            _arr(xmax, dt, rp, keep), _arr(nodes, np.int32, IP, keep), o.ctypes.data_as(rp) if out == "ok" else None)
    return rc, o


def _res_call(ndim=1, nbatch=3, offsets=(5, 13, 13, 20), x="ok", l1xdat=1, y="ok", coef="ok", ldcoef=16, xmin=(0.0, 0.0), xmax=(1.0, 1.0),
              nodes=(4, 4), resid="ok", stats="ok", real32=False):
    """splpak_residuals_many_f64 / _f32 on raw arguments -> (rc, resid, stats), both holding SENT before the call."""
    dt, rp = (np.float32, FP) if real32 else (np.float64, DP)
    keep = []
    r, s = np.full(40, SENT, dtype=dt), np.full(16, SENT)
    fn = capi.lib().splpak_residuals_many_f32 if real32 else capi.lib().splpak_residuals_many_f64
    xs = np.linspace(0.0, 1.0, 80)
    rc = fn(ndim, nbatch, _arr(offsets, np.int64, LP, keep), _arr(xs if x == "ok" else x, dt, rp, keep), l1xdat,
            _arr(xs if y == "ok" else y, dt, rp, keep), None, _arr(np.ones(64) if coef == "ok" else coef, dt, rp, keep), ldcoef,
            _arr(xmin, dt, rp, keep), _arr(xmax, dt, rp, keep), _arr(nodes, np.int32, IP, keep), r.ctypes.data_as(rp) if resid == "ok" else None,
            s.ctypes.data_as(DP) if stats == "ok" else None)
    return rc, r, s


def _zeroed_range_only(o, lo=5, hi=20):
    return np.all(o[:lo] == SENT) and np.all(o[lo:hi] == 0.0) and np.all(o[hi:] == SENT)


def test_eval_many_ladder_in_order_before_any_device_call():
    """Every rung with later rungs failing too: the first failing check wins.  101 / 102 / 103 zero exactly
    [offsets[0], offsets[nbatch]); every other failure writes nothing.  No rung asks for a device."""
    late = dict(ldxq=0, ldcoef=0, xq=None, coef=None)      # rungs 3 and 5 fail as well
    untouched = [
        (E_BADARG, dict(offsets=None, ndim=0)),
        (E_BADARG, dict(nodes=None, ndim=0)),
        (E_BADARG, dict(xmin=None, ndim=0)),
        (E_BADARG, dict(xmax=None, ndim=0)),
        (E_BADARG, dict(nbatch=0, ndim=0)),
        (E_BADARG, dict(offsets=(5, 13, 12, 20), ndim=0)),
        (E_BADARG, dict(offsets=(5, 13, 12, 20), ndim=2, nodes=(3, 3), **late)),
        (E_UNSUPPORTED, dict(ndim=5, nodes=(3,) * 5, xmin=(0,) * 5, xmax=(0,) * 5, **late)),
        (E_BADARG, dict(ldxq=0, coef=None)),
        (E_BADARG, dict(ndim=2, ldxq=1, out=None)),
        (E_BADARG, dict(ldcoef=3, xq=None)),
        (E_BADARG, dict(ndim=2, ldxq=2, ldcoef=15, nderiv=[3, 0])),
        (E_BADARG, dict(xq=None)),
        (E_BADARG, dict(coef=None, nderiv=[3])),
        (E_BADARG, dict(out=None)),
    ]
    for want, kw in untouched:
        rc, o = _eval_call(**kw)
        assert rc == want, (want, rc, kw)
        assert np.all(o == SENT), kw
    zeroed = [
        (101, dict(ndim=0, nodes=(3, 3), **late)),
        (101, dict(ndim=-1, nodes=(3, 3), xmax=(0.0, 0.0), **late)),
        (102, dict(ndim=2, nodes=(3, 4), xmax=(1.0, 0.0), **late)),
        (102, dict(ndim=1, nodes=(3,), nderiv=[3], **late)),
        (103, dict(ndim=2, nodes=(4, 4), xmax=(1.0, 0.0), **late)),
        (103, dict(ndim=1, xmin=(1.0,), xmax=(1.0,), nderiv=[5], **late)),
    ]
    for want, kw in zeroed:
        rc, o = _eval_call(**kw)
        assert rc == want, (want, rc, kw)
        assert _zeroed_range_only(o), (kw, o)
        assert _eval_call(out=None, **kw)[0] == want      # a null `out` is not written
    # REAL32: the same ladder on float storage
    rc, o = _eval_call(ndim=2, nodes=(4, 4), xmax=(1.0, 0.0), real32=True, **late)
    assert rc == 103 and o.dtype == np.float32 and _zeroed_range_only(o)
    rc, o = _eval_call(ldcoef=3, real32=True)
    assert rc == E_BADARG and np.all(o == SENT)
    assert capi.debug_eval_many_stats() == (0,) * 8      # a refused call leaves no counters


def test_eval_many_empty_batch_without_gpu():
    """No queries at all: 0, or 104 for an nderiv out of range; nothing is written and no data pointer is looked at."""
    for off in ((5, 5, 5, 5), (0, 0, 0, 0)):
        for nder, want in ((None, 0), ([1], 0), ([3], 104), ([-1], 104)):
            for real32 in (False, True):
                rc, o = _eval_call(offsets=off, xq=None, coef=None, out=None, nderiv=nder, real32=real32)
                assert rc == want, (off, nder, rc)
                rc, o = _eval_call(offsets=off, nderiv=nder, real32=real32)
                assert rc == want and np.all(o == SENT)
    assert capi.debug_eval_many_stats() == (0, 0, 0, 3, 0, 1, 0, 0)
    # the leading dimensions are checked before the batch is found empty
    assert _eval_call(offsets=(5, 5, 5, 5), ldxq=0)[0] == E_BADARG
    assert _eval_call(offsets=(5, 5, 5, 5), ldcoef=3, nderiv=[3])[0] == E_BADARG


def test_residuals_many_ladder_in_order_before_any_device_call():
    """Every rung with later rungs failing too; a ladder failure never writes resid or stats."""
    late = dict(l1xdat=0, x=None, y=None, coef=None)      # rung 4 fails as well
    ladder = [
        (E_BADARG, dict(offsets=None, ndim=0)),
        (E_BADARG, dict(nodes=None, ndim=0)),
        (E_BADARG, dict(xmin=None, ndim=0)),
        (E_BADARG, dict(xmax=None, ndim=0)),
        (E_BADARG, dict(nbatch=0, ndim=0)),
        (E_BADARG, dict(offsets=(5, 13, 12, 20), ndim=0)),
        (101, dict(ndim=0, nodes=(3, 3), ldcoef=0, **late)),
        (E_UNSUPPORTED, dict(ndim=5, nodes=(3,) * 5, xmin=(0,) * 5, xmax=(0,) * 5, ldcoef=0, **late)),
        (102, dict(ndim=2, nodes=(3, 4), xmax=(1.0, 0.0), ldcoef=0, **late)),
        (103, dict(ndim=2, nodes=(4, 4), xmax=(1.0, 0.0), ldcoef=0, **late)),
        (104, dict(ndim=2, ldcoef=15, **late)),
        (104, dict(ldcoef=3, resid=None, stats=None)),
        (E_BADARG, dict(ndim=2, l1xdat=1)),
        (E_BADARG, dict(x=None)),
        (E_BADARG, dict(y=None)),
        (E_BADARG, dict(coef=None)),
        (E_BADARG, dict(resid=None, stats=None)),
    ]
    for want, kw in ladder:
        rc, r, s = _res_call(**kw)
        assert rc == want, (want, rc, kw)
        assert np.all(r == SENT) and np.all(s == SENT), kw
    rc, r, s = _res_call(ldcoef=3, real32=True)
    assert rc == 104 and r.dtype == np.float32 and np.all(r == SENT) and np.all(s == SENT)
    rc, r, s = _res_call(l1xdat=0, real32=True)
    assert rc == E_BADARG and np.all(r == SENT) and np.all(s == SENT)


def test_residuals_many_batch_without_points_without_gpu():
    """0, stats as for problems without points, resid untouched -- answered on the host."""
    for real32 in (False, True):
        rc, r, s = _res_call(offsets=(5, 5, 5, 5), real32=real32)
        assert rc == 0 and np.all(r == SENT)
        assert np.array_equal(s[:12].reshape(3, 4), np.tile([0.0, 0.0, 0.0, -1.0], (3, 1))) and np.all(s[12:] == SENT)
        assert _res_call(offsets=(5, 5, 5, 5), stats=None, real32=real32)[0] == 0
    assert capi.debug_eval_many_stats() == (0, 0, 0, 3, 0, 2, 0, 0)


# ---------------------------------------------------------------------------------------------------------------
# GPU tier: eval_many
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _spec(nodes, variant="dense"):
    return dict(ndim=len(nodes), nodes=list(nodes), m=1000 + sum(nodes), variant=variant)


def _box(nodes, variant="dense"):
    lo, hi = cases.domain(_spec(nodes, variant))
    return list(lo), list(hi)


@functools.lru_cache(maxsize=None)
def _queries(nodes, n, variant="dense"):
    """n queries of make_queries (a block of at least 64, repeated for a long list; nobody writes to them)."""
    block = cases.make_queries(_spec(nodes, variant), max(64, min(n, 1 << 16)))
    reps = -(-n // block.shape[0])
    return np.ascontiguousarray(np.tile(block, (reps, 1))[:n])


def _coefs(nodes, nbatch, seed=0):
    """(nbatch, ncol) seeded random normals: no two problems share a row."""
    return np.random.default_rng(4100 + 17 * seed + sum(nodes) + len(nodes)).standard_normal((nbatch, int(np.prod(nodes))))


def _offsets(sizes, first=0):
    return np.concatenate([[first], first + np.cumsum(sizes)]).astype(np.int64)


def _singles(nodes, lo, hi, off, q, coef, ncol, pat, out):
    """The yardstick: the single entry under EVAL_DIRECT per problem that has queries, on device tensors q (rows by global
    index), coef (nbatch, >= ncol), into out (by global index) -> the set of statuses."""
    import torch
    nd = len(nodes)
    rcs = set()
    capi.set_eval_mode(capi.EVAL_DIRECT)
    try:
        for k in range(off.size - 1):
            a, b = int(off[k]), int(off[k + 1])
            if b > a:
                rcs.add(capi.evaluate_dev(nd, q[a:b], pat, coef[k, :ncol], lo, hi, list(nodes), out[a:b], _stream()))
        torch.cuda.synchronize()
    finally:
        capi.set_eval_mode(capi.EVAL_AUTO)
    return rcs


def _many_vs_singles(nodes, sizes, pats, first=0, ldxq=None, gap=0, real32=False, variant="dense", tail=3, seed=0):
    """One batch on the device against the single entry, for every (pattern, status, pattern of the yardstick) of pats: equal bits
    inside [offsets[0], offsets[nbatch]), the sentinel outside.  -> the counters of the last call."""
    import torch
    nd, ncol = len(nodes), int(np.prod(nodes))
    dt = np.float32 if real32 else np.float64
    off = _offsets(sizes, first)
    n, total = int(off[-1]) - first, int(off[-1]) + tail
    ld = nd if ldxq is None else ldxq
    xq = np.full((total, ld), 1.0e30, dtype=dt)
    xq[first:first + n, :nd] = _queries(tuple(nodes), n, variant)
    cf = np.full((len(sizes), ncol + gap), np.nan, dtype=dt)
    cf[:, :ncol] = _coefs(nodes, len(sizes), seed)
    lo, hi = _box(nodes, variant)
    q, c = _dev(xq), _dev(cf)
    stats = None
    for pat, want_rc, ref_pat in pats:
        got = torch.full((total,), SENT, dtype=q.dtype, device=q.device)
        want = torch.full((total,), SENT, dtype=q.dtype, device=q.device)
        rc = capi.evaluate_many_dev(nd, off, q, pat, c, lo, hi, list(nodes), got, ldxq=ld, ldcoef=ncol + gap, stream=_stream())
        stats = capi.debug_eval_many_stats()
        torch.cuda.synchronize()
        assert rc == want_rc, (pat, rc)
        assert _singles(nodes, lo, hi, off, q, c, ncol, ref_pat, want) <= {0}
        assert stats[1] == 1 and stats[2] == n and stats[3] == len(sizes) and stats[5] == 1, stats
        assert got.dtype == (torch.float32 if real32 else torch.float64)
        assert bool(torch.isfinite(got[first:first + n]).all())
        assert torch.equal(got, want), (nodes, pat, int((got != want).sum()))
        assert bool((got[:first] == SENT).all()) and bool((got[first + n:] == SENT).all())
    return stats


@pytest.mark.gpu
def test_segment_edges_of_waves_and_problems():
    """1. Problems that end one short of, on and one past a wave's and a workgroup's edge, empty problems alone and in runs,
    offsets[0] = 5, a padded xq (1e30 in the unused rows) and padded coefficient rows (NaN in the gaps)."""
    sizes = [0, 1, 63, 64, 65, 0, 0, 255, 256, 257, 1, 0, 513, 0]
    pats = [(None, 0, None), ([1], 0, [1]), ([2], 0, [2]), ([3], 104, [2])]
    _many_vs_singles((9,), sizes, pats, first=5, ldxq=3, gap=3)


@pytest.mark.gpu
def test_many_problems_per_wave():
    """2. 3 000 problems of 0, 1, 2, 3 queries: some forty problems in every wave, every lane searches."""
    sizes = [k % 4 for k in range(3000)]
    _many_vs_singles((9,), sizes, [(None, 0, None)])


@pytest.mark.gpu
def test_beyond_one_sweep_of_the_launch():
    """3. 3 sweeps + 1 queries: a problem that straddles the first two sweeps, one that straddles the last two, a tail of problems
    of 100 queries; one launch of the same number of workgroups."""
    import torch
    nodes, lo, hi = (9,), [0.0], [1.0]
    big = 1 << 22
    q = _dev(_queries(nodes, big))
    out = torch.zeros(big, dtype=torch.float64, device="cuda")
    c = _dev(_coefs(nodes, 1))
    assert capi.evaluate_many_dev(1, [0, big], q, None, c, lo, hi, list(nodes), out, stream=_stream()) == 0
    torch.cuda.synchronize()
    large = capi.debug_eval_many_stats()
    sweep = large[4]
    assert large[1] == 1 and 0 < sweep < big, large
    del q, out
    n = 3 * sweep + 1
    sizes = [sweep + 1000, n - (sweep + 1000) - 5001] + [100] * 50 + [1]
    assert sum(sizes) == n and sizes[0] > sweep and sizes[0] + sizes[1] > 2 * sweep
    stats = _many_vs_singles(nodes, sizes, [(None, 0, None)], tail=0, seed=1)
    assert stats[0] == large[0] and stats[1] == 1 and stats[4] == sweep, (stats, large)


MIXED = {1: [2], 2: [0, 2], 3: [1, 0, 2], 4: [2, 1, 0, 1]}


@pytest.mark.gpu
@pytest.mark.parametrize("real32", [False, True], ids=["real64", "real32"])
@pytest.mark.parametrize("nodes", [(9,), (5, 9), (4, 5, 6), (4, 4, 4, 4)], ids=lambda v: "x".join(map(str, v)))
def test_every_dimension_and_storage(nodes, real32):
    """4. Ragged batches of 5 problems with an empty one on an anisotropic box whose bounds are exact in single precision;
    values and a mixed derivative pattern."""
    nd = len(nodes)
    _many_vs_singles(nodes, [130, 7, 0, 300, 64], [(None, 0, None), (MIXED[nd], 0, MIXED[nd])], first=2, gap=1, real32=real32,
                     variant="box")


@pytest.mark.gpu
def test_against_the_oracle(port):
    """5. One 2-D batch against port.evaluate, problem by problem: 1e-10, the bar test_gpu_parity.py holds the single entry to."""
    nodes, sizes = (5, 9), [200, 0, 33, 150]
    lo, hi = _box(nodes, "box")
    off = _offsets(sizes)
    q, cf = _queries(nodes, int(off[-1]), "box"), _coefs(nodes, len(sizes))
    for pat in (None, [1, 0], [0, 2]):
        got, rc = capi.evaluate_many(2, off, q, pat, cf, lo, hi, list(nodes))
        assert rc == 0
        for k in range(len(sizes)):
            a, b = int(off[k]), int(off[k + 1])
            if b > a:
                want, rc_ref = port.evaluate(2, q[a:b], pat if pat is not None else [0, 0], cf[k], lo, hi, list(nodes))
                err = relmax(got[a:b], want)
                print(f"problem {k}, nderiv {pat}: vs the oracle {err:.2e}")
                assert rc_ref == 0 and err <= 1e-10


@pytest.mark.gpu
def test_eval_many_bits_do_not_depend_on_the_batch_the_position_or_the_entry():
    """6. A problem alone, first, last and between different neighbours; the host entry and the _dev entry."""
    import torch
    nodes, lo, hi = (5, 9), [0.0, 0.0], [1.0, 1.0]
    ncol = 45
    cf = _coefs(nodes, 4)
    qs = [_queries(nodes, n)[::-1] if k % 2 else _queries(nodes, n) for k, n in enumerate((150, 64, 7, 200))]

    def run(order, empty_at=()):
        sizes, rows = [], []
        for i, k in enumerate(order):
            if i in empty_at:
                sizes.append(0)
            rows.append(len(sizes))
            sizes.append(qs[k].shape[0])
        off = _offsets(sizes, 3)
        x = np.zeros((int(off[-1]), 2))
        c = np.zeros((len(sizes), ncol))
        for k, r in zip(order, rows):
            x[off[r]:off[r + 1]] = qs[k]
            c[r] = cf[k]
        out, rc = capi.evaluate_many(2, off, x, None, c, lo, hi, list(nodes))
        assert rc == 0
        return {k: out[off[r]:off[r + 1]].copy() for k, r in zip(order, rows)}, (off, x, c, out)

    alone = {k: run([k])[0][k] for k in range(4)}
    for order, empty_at in (([0, 1, 2, 3], ()), ([3, 2, 1, 0], (2,)), ([2, 0, 3, 1], (0, 1)), ([1, 3, 0, 2], ())):
        got, (off, x, c, out) = run(order, empty_at)
        for k in order:
            assert np.array_equal(got[k], alone[k]), (order, k)
    # the _dev entry on the last batch
    od = torch.zeros(out.size, dtype=torch.float64, device="cuda")
    assert capi.evaluate_many_dev(2, off, _dev(x), None, _dev(c), lo, hi, list(nodes), od, stream=_stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(od.cpu().numpy()[3:], out[3:])


# ---------------------------------------------------------------------------------------------------------------
# GPU tier: residuals_many
def stats_in_numpy(y, f, w):
    """The four numbers of one problem in the stated order: 64 strided lane sums (the product and the sum rounded on their own),
    the butterfly 32 .. 1, the first index of the maximum.  y, f, w (or None) are doubles."""
    n = y.size
    if n == 0:
        return np.array([0.0, 0.0, 0.0, -1.0])
    wt = w if (w is not None and w[0] >= 0.0) else np.ones(n)
    counted = wt != 0.0
    if not counted.any():
        return np.array([0.0, 0.0, 0.0, -1.0])
    r = y - f
    t = np.zeros(n)
    t[counted] = wt[counted] * r[counted]
    rows = -(-n // 64)
    tt = np.zeros(rows * 64)
    tt[:n] = t * t            # (an uncounted point adds +0: no bit of a non-negative sum changes)
    lanes = np.zeros(64)
    for row in tt.reshape(rows, 64):
        lanes = lanes + row
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[np.arange(64) ^ o]
    at = np.where(counted, np.abs(t), -1.0)
    return np.array([float(counted.sum()), lanes[0], at.max(), float(np.argmax(at))])


def _fitted_batch():
    """(offsets, x, y, w, coef, problems) of the residual tests: the 1-D problems n9_wide_x1, w_n9_wide and a copy with a negative
    first weight around an empty one, fitted by fit_many."""
    a, b, c = dict(problem("n9_wide_x1")), dict(problem("w_n9_wide")), dict(problem("w_n9_wide"))
    c["w"] = c["w"].copy()
    c["w"][0] = -1.0
    ps = [a, b, c]
    off, x, y, w = pack(ps, empty_at=(1,))
    coef, rc, st, _ = capi.fit_many(1, off, x, y, w, [0.0], [1.0], [9], 1.0)
    assert rc == 105 and list(st) == [0, 105, 0, 0]
    return off, x, y, w, coef


def _check_residuals(nd, off, x, y, w, coef, lo, hi, nodes):
    """resid == y - evaluate_many bit for bit, stats == the numpy restatement bit for bit; -> (resid, stats)."""
    f, rc = capi.evaluate_many(nd, off, x, None, coef, lo, hi, list(nodes))
    assert rc == 0
    resid, stats, rc = capi.residuals_many(nd, off, x, y, w, coef, lo, hi, list(nodes))
    assert rc == 0
    a, b = int(off[0]), int(off[-1])
    assert np.array_equal(resid[a:b], (y - f[:y.size])[a:b])
    for k in range(off.size - 1):
        s, e = int(off[k]), int(off[k + 1])
        want = stats_in_numpy(y[s:e], f[s:e], None if w is None else w[s:e])
        assert np.array_equal(stats[k], want), (k, stats[k], want)
    return resid, stats


@pytest.mark.gpu
def test_residuals_and_statistics_f64():
    """7. 1-D and 2-D, without weights, with 15 % exact zero weights, an empty problem, a negative first weight."""
    off, x, y, w, coef = _fitted_batch()
    resid, stats = _check_residuals(1, off, x, y, w, coef, [0.0], [1.0], [9])
    n = off[1] - off[0]
    assert stats[0, 0] == n and list(stats[1]) == [0.0, 0.0, 0.0, -1.0]
    assert stats[2, 0] == np.count_nonzero(w[off[2]:off[3]]) < n and stats[3, 0] == n      # (the negative first weight: all count)
    assert np.all(stats[[0, 2, 3], 1] > 0.0)
    # a NaN value under a zero weight: the statistics stay finite (and the same), the residual is NaN at that point only
    zero = int(off[2]) + int(np.flatnonzero(w[off[2]:off[3]] == 0.0)[0])
    y2 = y.copy()
    y2[zero] = np.nan
    r2, s2, rc = capi.residuals_many(1, off, x, y2, w, coef, [0.0], [1.0], [9])
    assert rc == 0 and np.array_equal(s2, stats) and np.all(np.isfinite(s2))
    assert np.isnan(r2[zero]) and np.array_equal(np.delete(r2, zero), np.delete(resid, zero))
    # either output alone
    r3, none, rc = capi.residuals_many(1, off, x, y, w, coef, [0.0], [1.0], [9], want_stats=False)
    assert rc == 0 and none is None and np.array_equal(r3, resid)
    none, s3, rc = capi.residuals_many(1, off, x, y, w, coef, [0.0], [1.0], [9], want_resid=False)
    assert rc == 0 and none is None and np.array_equal(s3, stats)
    # two dimensions: g59 and w_g59 with an empty problem between them
    ps = [problem("g59"), problem("w_g59")]
    off, x, y, w = pack(ps, empty_at=(1,))
    coef, rc, st, _ = capi.fit_many(2, off, x, y, w, [0.0, 0.0], [1.0, 1.0], [5, 9], 0.0)
    assert rc == 105 and list(st) == [0, 105, 0]
    _, stats = _check_residuals(2, off, x, y, w, coef, [0.0, 0.0], [1.0, 1.0], [5, 9])
    assert stats[0, 0] == 2000 and stats[2, 0] == np.count_nonzero(ps[1]["w"])


@pytest.mark.gpu
def test_residuals_and_statistics_f32():
    """8. REAL32 storage: resid = float32(float64(y) - f) and the statistics of those doubles, f from the f64 entry on the
    widened inputs."""
    off, x, y, w, coef = _fitted_batch()
    x32, y32, w32, c32 = (a.astype(np.float32) for a in (x, y, w, coef))
    xw, yw, ww, cw = (a.astype(np.float64) for a in (x32, y32, w32, c32))
    f, rc = capi.evaluate_many(1, off, xw, None, cw, [0.0], [1.0], [9])
    assert rc == 0
    resid, stats, rc = capi.residuals_many(1, off, x32, y32, w32, c32, [0.0], [1.0], [9], real32=True)
    assert rc == 0 and resid.dtype == np.float32 and stats.dtype == np.float64
    assert np.array_equal(resid, (yw - f).astype(np.float32))
    for k in range(off.size - 1):
        s, e = int(off[k]), int(off[k + 1])
        assert np.array_equal(stats[k], stats_in_numpy(yw[s:e], f[s:e], ww[s:e])), k


@pytest.mark.gpu
def test_residuals_bits_do_not_depend_on_the_batch_the_position_or_the_entry():
    """9. Alone, first, last, between other neighbours, host and _dev entry; and 3 x (the workgroups of a large launch) + 1 copies
    of two alternating problems, every copy with the same bits, in one launch."""
    import torch
    a, b = dict(problem("n9_wide_x1")), dict(problem("w_n9_wide"))
    a["w"] = np.ones(a["y"].size)
    cf = capi.fit_many(1, *pack([a, b]), [0.0], [1.0], [9], 1.0)[0]

    def run(order, dev=False):
        off, x, y, w = pack([[a, b][k] for k in order])
        c = np.ascontiguousarray(cf[list(order)])
        if not dev:
            resid, stats, rc = capi.residuals_many(1, off, x, y, w, c, [0.0], [1.0], [9])
        else:
            rd = torch.full((y.size,), SENT, dtype=torch.float64, device="cuda")
            sd = torch.full((len(order), 4), SENT, dtype=torch.float64, device="cuda")
            rc = capi.residuals_many_dev(1, off, _dev(x), _dev(y), _dev(w), _dev(c), [0.0], [1.0], [9], rd, sd, stream=_stream())
            torch.cuda.synchronize()
            resid, stats = rd.cpu().numpy(), sd.cpu().numpy()
        assert rc == 0
        return off, resid, stats

    alone = [run([k]) for k in (0, 1)]
    for order in ([0, 1], [1, 0], [0, 0, 1, 0], [1, 0, 1, 1]):
        for dev in (False, True):
            off, resid, stats = run(order, dev=dev)
            for i, k in enumerate(order):
                assert np.array_equal(stats[i], alone[k][2][0]), (order, i, dev)
                assert np.array_equal(resid[off[i]:off[i + 1]], alone[k][1]), (order, i, dev)
    assert not np.array_equal(alone[0][2], alone[1][2])
    run([0, 1] * 8192)
    large = capi.debug_eval_many_stats()
    assert large[1] == 1 and large[5] == 2 and 1 <= large[0] < 16384, large
    ncopy = 3 * large[0] + 1
    order = ([0, 1] * ((ncopy + 1) // 2))[:ncopy]
    off, resid, stats = run(order)
    got = capi.debug_eval_many_stats()
    assert got[0] == large[0] and got[1] == 1 and got[3] == ncopy and got[2] == off[-1], got
    assert np.all(stats[0::2] == alone[0][2][0]) and np.all(stats[1::2] == alone[1][2][0])
    n = a["y"].size
    assert b["y"].size == n
    assert np.all(resid.reshape(ncopy, n)[0::2] == alone[0][1]) and np.all(resid.reshape(ncopy, n)[1::2] == alone[1][1])


@pytest.mark.gpu
def test_fit_then_residuals_end_to_end(port):
    """10. fit_many, then residuals_many on n130_x3 at xtrap = 1: sqrt(S) against a numpy sum over w (y - port.evaluate) of the same
    coefficients.  Both are sums of <= 1 800 positive terms in different orders: they agree to 1 800 x 2^-53 = 2e-13; bar 1e-12.
    (Not info[8]: that includes the constraint rows and belongs to the coefficients before the last correction.)"""
    p = problem("n130_x3")
    lo, hi = lo_hi(p)
    n = p["y"].size
    coef, rc, st, _ = capi.fit_many(1, [0, n], p["x"], p["y"], None, lo, hi, list(p["nodes"]), 1.0)
    assert rc == 0 and n <= 1800
    resid, stats, rc = capi.residuals_many(1, [0, n], p["x"], p["y"], None, coef, lo, hi, list(p["nodes"]))
    f, rc_ref = port.evaluate(1, p["x"], [0], coef[0], lo, hi, list(p["nodes"]))
    want = np.sqrt(np.sum((p["y"] - f) ** 2))
    got = np.sqrt(stats[0, 1])
    print(f"n130_x3: sqrt(S) {got:.17g}, numpy over the oracle's values {want:.17g}, relative {abs(got - want) / want:.2e}")
    assert rc == 0 and rc_ref == 0 and stats[0, 0] == n
    assert abs(got - want) <= 1e-12 * want
    assert stats[0, 2] == np.max(np.abs(resid)) and stats[0, 3] == np.argmax(np.abs(resid))


# ---------------------------------------------------------------------------------------------------------------
# GPU tier: stream order (the harness of tests/test_stream_order.py)
SO_NODES, SO_SIZES = (9,), [300, 0, 1000, 64, 700]


def _so_data(part):
    """Valid points, values, weights and coefficients of the batch SO_SIZES; part 0: the inputs, part 1: the decoy."""
    n = sum(SO_SIZES)
    rng = np.random.default_rng(9100 + part)
    x = _queries(SO_NODES, 2 * n)[part * n:(part + 1) * n]
    return {"x": x, "y": rng.standard_normal(n), "w": rng.uniform(0.5, 2.0, n), "coef": _coefs(SO_NODES, len(SO_SIZES), seed=5 + part)}


def _so_eval_entry(sizes=SO_SIZES):
    off = _offsets(sizes)

    def call(t, stream):
        return (capi.evaluate_many_dev(1, off, t["x"], None, t["coef"], [0.0], [1.0], list(SO_NODES), t["out"], stream=stream),)
    return _Entry(call, {"out": (int(off[-1]),)})


def _so_resid_entry(sizes=SO_SIZES):
    off = _offsets(sizes)

    def call(t, stream):
        return (capi.residuals_many_dev(1, off, t["x"], t["y"], t["w"], t["coef"], [0.0], [1.0], list(SO_NODES), t["resid"], t["stats"],
                                        stream=stream),)
    return _Entry(call, {"resid": (int(off[-1]),), "stats": (len(sizes), 4)})


def _eval_only(d):
    return {k: d[k] for k in ("x", "coef")}


@pytest.mark.gpu
def test_evaluate_many_dev_with_late_inputs_and_stream_only_read_back(clock, streams):
    _check_late(_so_eval_entry(), _eval_only(_so_data(0)), _eval_only(_so_data(1)), streams, clock, "evaluate_many_dev")


@pytest.mark.gpu
def test_residuals_many_dev_with_late_inputs_and_stream_only_read_back(clock, streams):
    _check_late(_so_resid_entry(), _so_data(0), _so_data(1), streams, clock, "residuals_many_dev")


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["evaluate_many_dev", "residuals_many_dev"])
def test_many_dev_control_reads_the_decoy_on_a_second_stream(family, clock, streams):
    if family == "evaluate_many_dev":
        _check_control(_so_eval_entry(), _eval_only(_so_data(0)), _eval_only(_so_data(1)), streams, clock, family + " (control)")
    else:
        _check_control(_so_resid_entry(), _so_data(0), _so_data(1), streams, clock, family + " (control)")


@pytest.mark.gpu
def test_back_to_back_calls_with_different_offsets_on_two_streams(clock, streams):
    """The offsets live in one per-thread scratch: the second call's upload waits for the first call's kernel (wait_on /
    mark_used), although that kernel sits behind a delay on another stream."""
    import torch
    data = _so_data(0)
    ea, eb = _so_resid_entry(SO_SIZES), _so_resid_entry(SO_SIZES[::-1])
    ya, _, _ = _yardsticks(ea, data, _so_data(1), "residuals_many_dev, offsets A")
    yb, _, _ = _yardsticks(eb, data, _so_data(1), "residuals_many_dev, offsets B")
    assert ya.differs(yb)
    t = {k: _dev(v) for k, v in data.items()}
    ta, tb = dict(t, **ea.outputs()), dict(t, **eb.outputs())
    pa, pb = ea.pinned(), eb.pinned()
    torch.cuda.synchronize()
    try:
        d = clock.delay(streams.S, T_FLOOR_MS)
        ha = ea.call(ta, streams.S.cuda_stream)
        hb = eb.call(tb, streams.S2.cuda_stream)
        for st, tt, pp in ((streams.S, ta, pa), (streams.S2, tb, pb)):
            with torch.cuda.stream(st):
                for k in pp:
                    pp[k].copy_(tt[k], non_blocking=True)
        streams.S.synchronize()
        streams.S2.synchronize()
    finally:
        torch.cuda.synchronize()
    d.check("back to back")
    assert ha == (0,) and hb == (0,)
    for k in pa:
        assert np.array_equal(pa[k].numpy(), ya.dev[k]), ("A", k)
        assert np.array_equal(pb[k].numpy(), yb.dev[k]), ("B", k)


# ---------------------------------------------------------------------------------------------------------------
FDIR = os.path.join(ROOT, "splpak_amd", "fortran")
PROG = os.path.join(FDIR, "build", "test_eval_many")


@pytest.mark.gpu
def test_fortran_evaluate_each_and_residuals_each():
    """12. initialize_many, then evaluate_each against evaluate per point and residuals_each's sums against a Fortran loop in
    the stated order (fortran/test/test_eval_many.f90)."""
    if not os.path.exists(PROG):
        if not os.path.exists("/opt/rocm/bin/amdflang"):
            pytest.skip("amdflang not available")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "splpak_amd", "csrc")])
        subprocess.check_call(["make", "-C", FDIR])
    r = subprocess.run([PROG], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS test_eval_many" in r.stdout
