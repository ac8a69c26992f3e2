"""Several coefficient sets at the same points in one call (splpak_eval_fields_*, csrc/eval.hip launch_eval_fields).

The yardstick on the GPU is the library's own single-field entry (splpak_eval_dev_* with EVAL_DIRECT), field by field, which
test_gpu_parity.py holds to the oracle and the goldens: a fields call must return EXACTLY its values (torch.equal /
np.array_equal -- no tolerance) on every route -- the direct fields kernel, the shared sort of the persistent region path,
the loop of single-field calls -- because every field goes through the same factor table and the same window sum.
Coefficients are seeded random normals; queries are seeded uniforms over the box widened by 30 % on each side with xmin, xmax
and exact node positions mixed in.  The box bounds are exact in single precision, so the REAL32 entries see the same grid.

CPU tier: exports and the host-side argument ladder, all of which returns before any device call.
"""
import functools

import numpy as np
import pytest

from splpak_amd import capi
from tests.cases import CASES, make_inputs, make_queries
from tests.conftest import load_golden

NAMES = ("splpak_eval_fields_f64", "splpak_eval_fields_f32", "splpak_eval_fields_dev_f64", "splpak_eval_fields_dev_f32",
         "splpak_debug_eval_fields_stats")


# ---------------------------------------------------------------------------------------------------------------
# CPU tier
def _arr(a, dt):
    return None if a is None else np.ascontiguousarray(a, dtype=dt)


def _host_call(ndim, nq, nfields, nodes, xmin, xmax, out, ldout, xq="default", coef="default", ldxq=None, ldcoef=None, nderiv=None):
    """splpak_eval_fields_f64 as C sees it: every pointer may be None, every count is passed as given."""
    nodes, xmin, xmax = _arr(nodes, np.int32), _arr(xmin, np.float64), _arr(xmax, np.float64)
    ncol = 1 if nodes is None else int(np.prod(np.maximum(nodes[:max(ndim, 1)], 1)))
    ldxq = max(ndim, 1) if ldxq is None else ldxq
    ldcoef = ncol if ldcoef is None else ldcoef
    if isinstance(xq, str):
        xq = np.full(max(nq, 1) * max(ldxq, ndim, 1), 0.3)
    if isinstance(coef, str):
        coef = np.ones(max(nfields, 1) * max(ldcoef, ncol))
    nd = _arr(nderiv, np.int32)
    return capi.lib().splpak_eval_fields_f64(ndim, nq, capi._p(xq, capi._dp), ldxq, capi._p(nd, capi._ip), nfields,
                                             capi._p(coef, capi._dp), ldcoef, capi._p(xmin, capi._dp), capi._p(xmax, capi._dp),
                                             capi._p(nodes, capi._ip), capi._p(out, capi._dp), ldout)


def test_fields_symbols_are_exported():
    L = capi.lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS
    assert callable(capi.evaluate_fields) and callable(capi.evaluate_fields_dev) and callable(capi.debug_eval_fields_stats)


def _zeroed_fields_only(out, nq=5, ldout=7, nfields=3):
    o = out.reshape(nfields, ldout)
    return bool(np.all(o[:, :nq] == 0.0) and np.all(o[:, nq:] == 7.0))


def test_fields_validation_zeroes_every_field_and_keeps_the_gaps_without_gpu():
    """101/102/103 are decided on the host and zero the nq results of every field (:1166-1188), not the words between them."""
    out = np.full(21, 7.0)
    assert _host_call(0, 5, 3, [8, 8], [0, 0], [1, 1], out, 7) == 101
    assert _zeroed_fields_only(out)
    out = np.full(21, 7.0)
    assert _host_call(2, 5, 3, [8, 3], [0, 0], [1, 1], out, 7) == 102
    assert _zeroed_fields_only(out)
    out = np.full(21, 7.0)
    assert _host_call(2, 5, 3, [8, 8], [0, 0.5], [1, 0.5], out, 7) == 103
    assert _zeroed_fields_only(out)
    # the first failing check wins
    out = np.full(21, 7.0)
    assert _host_call(0, 5, 3, [8, 3], [0, 0], [1, 1], out, 7) == 101
    assert _zeroed_fields_only(out)
    assert _host_call(2, 5, 3, [8, 3], [0, 0.5], [1, 0.5], np.zeros(21), 7) == 102
    # a null `out` is not written
    assert _host_call(2, 5, 3, [8, 3], [0, 0], [1, 1], None, 7) == 102
    # a bad count is reported before the grid is looked at, and before a bad leading dimension
    out = np.full(21, 7.0)
    assert _host_call(0, 5, 0, [8, 3], [0, 0], [1, 1], out, 7) == capi.E_BADARG
    assert _host_call(2, 5, 3, [8, 3], [0, 0], [1, 1], out, 7, ldxq=1) == 102
    assert _zeroed_fields_only(out)
    # the Python wrapper reports them too
    v, rc = capi.evaluate_fields(2, np.zeros((5, 2)), None, np.ones((3, 24)), [0, 0], [1, 1], [8, 3])
    assert rc == 102 and v.shape == (3, 5) and np.all(v == 0.0)


def test_fields_bad_arguments_without_gpu():
    out = np.full(21, 7.0)
    good = dict(nodes=[8, 8], xmin=[0, 0], xmax=[1, 1])
    assert _host_call(2, 5, 0, out=out, ldout=7, **good) == capi.E_BADARG          # nfields
    assert _host_call(2, -1, 3, out=out, ldout=7, **good) == capi.E_BADARG         # nq
    assert _host_call(2, 5, 3, out=out, ldout=4, **good) == capi.E_BADARG          # ldout < nq
    assert _host_call(2, 5, 3, out=out, ldout=7, ldcoef=63, **good) == capi.E_BADARG
    assert _host_call(2, 5, 3, out=out, ldout=7, ldxq=1, **good) == capi.E_BADARG
    assert _host_call(2, 5, 3, out=out, ldout=7, xq=None, **good) == capi.E_BADARG
    assert _host_call(2, 5, 3, out=out, ldout=7, coef=None, **good) == capi.E_BADARG
    assert _host_call(2, 5, 3, out=None, ldout=7, **good) == capi.E_BADARG
    assert _host_call(2, 5, 3, [8, 8], [0, 0], None, out, 7) == capi.E_BADARG
    assert _host_call(2, 5, 3, [8, 8], None, [1, 1], out, 7) == capi.E_BADARG
    assert _host_call(2, 5, 3, None, [0, 0], [1, 1], out, 7) == capi.E_BADARG
    assert _host_call(5, 5, 3, [4] * 5, [0] * 5, [1] * 5, out, 7) == capi.E_UNSUPPORTED
    assert np.all(out == 7.0)
    # the REAL32 host entry runs the same ladder
    o32 = np.full(21, 7.0, dtype=np.float32)
    lo, hi, nodes = np.zeros(2, dtype=np.float32), np.ones(2, dtype=np.float32), np.array([8, 8], dtype=np.int32)
    assert capi.lib().splpak_eval_fields_f32(2, 5, None, 2, None, 3, None, 64, capi._p(lo, capi._fp), capi._p(hi, capi._fp),
                                             capi._p(nodes, capi._ip), capi._p(o32, capi._fp), 7) == capi.E_BADARG
    assert np.all(o32 == 7.0)


def test_fields_empty_batch_without_gpu():
    out = np.full(21, 7.0)
    assert _host_call(2, 0, 3, [8, 8], [0, 0], [1, 1], out, 7) == 0
    assert _host_call(2, 0, 3, [8, 8], [0, 0], [1, 1], out, 0, nderiv=[0, 3]) == 104
    assert _host_call(2, 0, 3, [8, 8], [0, 0], [1, 1], out, 7, xq=None, coef=None) == 0        # nothing to read: no null check
    assert _host_call(2, 0, 3, [8, 3], [0, 0], [1, 1], out, 7) == 102
    assert np.all(out == 7.0)
    v, rc = capi.evaluate_fields(2, np.zeros((0, 2)), [0, 3], np.ones((3, 64)), [0, 0], [1, 1], [8, 8])
    assert rc == 104 and v.shape == (3, 0)


def test_fields_stats_need_no_device():
    assert capi.lib().splpak_debug_eval_fields_stats(None) == capi.E_BADARG
    s = capi.debug_eval_fields_stats()
    assert len(s) == 3 and s[0] in (0, 1, 2, 3)


# ---------------------------------------------------------------------------------------------------------------
# GPU tier
LO, HI = [-1.25, 0.0, 2.0, -0.5], [3.5, 1.0, 2.75, 0.25]
MAXF = 5
MIXED = {1: [2], 2: [0, 2], 3: [1, 0, 2], 4: [2, 1, 0, 1]}
OUT_OF_RANGE = {1: [3], 2: [-1, 2], 3: [1, 0, 5], 4: [4, 1, -2, 1]}          # clamped to 0..2: MIXED


@functools.lru_cache(maxsize=None)
def _coefs(nodes, real32=False, seed=0):
    c = np.random.default_rng(1000 * seed + sum(nodes) + len(nodes)).standard_normal((MAXF, int(np.prod(nodes))))
    return c.astype(np.float32) if real32 else c


@functools.lru_cache(maxsize=None)
def _queries(nodes, nq, real32=False):
    """(nq, ndim) queries over the box widened by 30 % on each side; xmin, xmax and exact node positions mixed in."""
    rng = np.random.default_rng(7 * nq + sum(nodes))
    cols = []
    for d, nod in enumerate(nodes):
        lo, hi = LO[d], HI[d]
        w = hi - lo
        x = rng.uniform(lo - 0.3 * w, hi + 0.3 * w, nq)
        special = [lo, hi] + list(lo + (w / (nod - 1)) * rng.integers(0, nod, 6))
        x[:len(special)] = special
        rng.shuffle(x)
        cols.append(x)
    q = np.stack(cols, axis=1)
    return np.ascontiguousarray(q.astype(np.float32) if real32 else q)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _single(nodes, nq, pat, real32=False, seed=0):
    """The yardstick, computed once per case: the single-field entry under EVAL_DIRECT for each of the MAXF fields
    -> ((MAXF, nq) tensor on the device, ierror)."""
    import torch
    nd = len(nodes)
    q = _dev(_queries(nodes, nq, real32))
    c = _dev(_coefs(nodes, real32, seed))
    out = torch.full((MAXF, nq), float("nan"), dtype=q.dtype, device=q.device)
    rcs = set()
    capi.set_eval_mode(capi.EVAL_DIRECT)
    try:
        for k in range(MAXF):
            rcs.add(capi.evaluate_dev(nd, q, None if pat is None else list(pat), c[k], LO[:nd], HI[:nd], list(nodes), out[k], _stream()))
        torch.cuda.synchronize()
    finally:
        capi.set_eval_mode(capi.EVAL_AUTO)
    assert len(rcs) == 1
    return out, rcs.pop()


def _fields(nodes, nq, nfields, pat, real32=False, seed=0, q=None, coef=None, out=None):
    """One fields call on the device -> (out tensor as given or (nfields, nq), ierror, stats)."""
    import torch
    nd = len(nodes)
    q = _dev(_queries(nodes, nq, real32)) if q is None else q
    coef = _dev(_coefs(nodes, real32, seed)[:nfields]) if coef is None else coef
    if out is None:
        out = torch.full((nfields, nq), float("nan"), dtype=q.dtype, device=q.device)
    torch.cuda.synchronize()
    rc = capi.evaluate_fields_dev(nd, q, pat, coef, LO[:nd], HI[:nd], list(nodes), out, _stream())
    torch.cuda.synchronize()
    return out, rc, capi.debug_eval_fields_stats()


DIRECT_GRIDS = [(16,), (9, 7), (8, 6, 5), (5, 4, 6, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("real32", [False, True], ids=["real64", "real32"])
@pytest.mark.parametrize("nfields", [1, 2, 3, 5])
@pytest.mark.parametrize("nodes", DIRECT_GRIDS, ids=lambda v: "x".join(map(str, v)))
def test_fields_direct_route_equals_single_field_entry(nodes, nfields, real32):
    """The pair loop (2), the pair and the odd tail (3, 5) and the forward to the single-field entry (1); plain values, a mixed
    derivative pattern, and a pattern out of range: 104 with the values of the clamped pattern."""
    import torch
    nd, nq = len(nodes), 1000
    for pat, want_rc, ref_pat in ((None, 0, None), (MIXED[nd], 0, MIXED[nd]), (OUT_OF_RANGE[nd], 104, MIXED[nd])):
        want, rc0 = _single(nodes, nq, None if ref_pat is None else tuple(ref_pat), real32)
        got, rc, stats = _fields(nodes, nq, nfields, pat, real32)
        assert rc0 == 0 and rc == want_rc
        assert stats == ((3, 0, 1) if nfields == 1 else (1, 0, 1)), stats
        assert got.dtype == (torch.float32 if real32 else torch.float64)
        assert torch.equal(got, want[:nfields]), (pat, float((got - want[:nfields]).abs().max()))
    # the single-field entry reports the out-of-range pattern the same way
    assert _single(nodes, nq, tuple(OUT_OF_RANGE[nd]), real32)[1] == 104


@pytest.mark.gpu
@pytest.mark.parametrize("nodes", [(9, 7), (5, 4, 6, 4)], ids=["2d", "4d"])
def test_fields_padded_queries_and_coefficients_are_not_read(nodes):
    """ldxq = ndim + 2 with 1e300 behind every query, ldcoef = ncol + 3 with NaN behind every field."""
    import torch
    nd, nq, nf = len(nodes), 1000, 3
    ncol = int(np.prod(nodes))
    want, _ = _single(nodes, nq, tuple(MIXED[nd]))
    qp = np.full((nq, nd + 2), 1e300)
    qp[:, :nd] = _queries(nodes, nq)
    cp = np.full((nf, ncol + 3), np.nan)
    cp[:, :ncol] = _coefs(nodes)[:nf]
    got, rc, stats = _fields(nodes, nq, nf, MIXED[nd], q=_dev(qp), coef=_dev(cp)[:, :ncol])
    assert rc == 0 and stats == (1, 0, 1)
    assert torch.equal(got, want[:nf])


@pytest.mark.gpu
@pytest.mark.parametrize("real32", [False, True], ids=["real64", "real32"])
def test_fields_gaps_of_out_survive_device_and_host_form(real32):
    """ldout = nq + 5: the five words behind every field keep their sentinel, through the device form and the host form."""
    import torch
    nodes, nq, nf, pad = (8, 6, 5), 1000, 3, 5
    dt = np.float32 if real32 else np.float64
    want, _ = _single(nodes, nq, None, real32)
    out = torch.full((nf, nq + pad), -3.5, dtype=want.dtype, device=want.device)
    got, rc, stats = _fields(nodes, nq, nf, None, real32, out=out[:, :nq])
    assert rc == 0 and stats == (1, 0, 1)
    assert torch.equal(out[:, :nq], want[:nf]) and bool((out[:, nq:] == -3.5).all())
    # host form, as C sees it
    q, c = _queries(nodes, nq, real32), np.ascontiguousarray(_coefs(nodes, real32)[:nf])
    lo, hi, nod = np.array(LO[:3], dtype=dt), np.array(HI[:3], dtype=dt), np.array(nodes, dtype=np.int32)
    h = np.full((nf, nq + pad), -3.5, dtype=dt)
    rp = capi._fp if real32 else capi._dp
    fn = capi.lib().splpak_eval_fields_f32 if real32 else capi.lib().splpak_eval_fields_f64
    assert fn(3, nq, capi._p(q, rp), 3, None, nf, capi._p(c, rp), c.shape[1], capi._p(lo, rp), capi._p(hi, rp), capi._p(nod, capi._ip),
              capi._p(h, rp), nq + pad) == 0
    assert np.array_equal(h[:, :nq], want[:nf].cpu().numpy()) and np.all(h[:, nq:] == -3.5)
    # and through the Python wrapper, with padded coefficients on the way
    v, rc = capi.evaluate_fields(3, q, None, c, LO[:3], HI[:3], nodes, real32=real32, ldcoef=c.shape[1] + 3, ldout=nq + pad)
    assert rc == 0 and v.dtype == dt and np.array_equal(v, want[:nf].cpu().numpy())


@pytest.mark.gpu
def test_fields_grid_stride_beyond_the_block_cap():
    """2^21 + 777 queries: more than the 8 192 blocks of 256 threads a launch is capped at."""
    import torch
    nodes, nq, nf = (9, 7), 2 ** 21 + 777, 3
    want, _ = _single(nodes, nq, None)
    got, rc, stats = _fields(nodes, nq, nf, None)
    assert rc == 0 and stats == (1, 0, 1)
    assert torch.equal(got, want[:nf])


NQ_SORT = 2 * 8192 + 77                           # three place-pass workgroups, the last one partial
SORT_GRIDS = [(12, 13, 12), (20, 21, 36), (12, 12, 12, 8)]       # tiles of 8 window starts, of 16, and the 4-D kernel


@pytest.mark.gpu
@pytest.mark.parametrize("real32", [False, True], ids=["real64", "real32"])
@pytest.mark.parametrize("mixed", [False, True], ids=["values", "derivs"])
@pytest.mark.parametrize("nodes", SORT_GRIDS, ids=lambda v: "x".join(map(str, v)))
def test_fields_shared_sort_places_once_and_equals_single_field_entry(nodes, mixed, real32):
    """EVAL_BINNED: one place pass, three evaluation passes; then a second call of the same thread with other coefficients and
    two fields, which shows that the regions' chunk counters are cleared per field and per call."""
    import torch
    nd = len(nodes)
    pat = MIXED[nd] if mixed else None
    key = None if pat is None else tuple(pat)
    want, _ = _single(nodes, NQ_SORT, key, real32)
    want2, _ = _single(nodes, NQ_SORT, key, real32, seed=1)
    ncol = int(np.prod(nodes))
    cp = np.full((2, ncol + 3), np.nan, dtype=np.float32 if real32 else np.float64)      # an odd distance between the fields
    cp[:, :ncol] = _coefs(nodes, real32, 1)[:2]
    capi.set_eval_mode(capi.EVAL_BINNED)
    try:
        got, rc, stats = _fields(nodes, NQ_SORT, 3, pat, real32)
        got2, rc2, stats2 = _fields(nodes, NQ_SORT, 2, pat, real32, coef=_dev(cp)[:, :ncol])
    finally:
        capi.set_eval_mode(capi.EVAL_AUTO)
    assert rc == 0 and stats == (2, 1, 3), stats
    assert torch.equal(got, want[:3]), float((got - want[:3]).abs().max())
    assert rc2 == 0 and stats2 == (2, 1, 2), stats2
    assert torch.equal(got2, want2[:2]), float((got2 - want2[:2]).abs().max())


@pytest.mark.gpu
def test_fields_per_field_loop_where_the_shared_sort_does_not_apply():
    """EVAL_BINNED on a 2-D grid: the persistent region path declines, every field takes the single-field dispatcher."""
    import torch
    nodes, nq = (40, 40), 3000
    want, _ = _single(nodes, nq, None)
    capi.set_eval_mode(capi.EVAL_BINNED)
    try:
        got, rc, stats = _fields(nodes, nq, 3, None)
    finally:
        capi.set_eval_mode(capi.EVAL_AUTO)
    assert rc == 0 and stats[0] == 3, stats
    assert torch.equal(got, want[:3])


@pytest.mark.gpu
def test_fields_against_the_reference_golden():
    """Golden 3d12: the first field at the bar of test_eval_matches_reference_golden (1e-12 of the largest value), the
    second -- the coefficients times -0.5 -- exactly -0.5 times the first (scaling by a power of two is exact)."""
    spec = CASES["3d12"]
    gold = load_golden("3d12")
    inp = make_inputs(spec)
    q = make_queries(spec)
    coefs = np.stack([gold["coef"], -0.5 * gold["coef"]])
    v, rc = capi.evaluate_fields(inp["ndim"], q, None, coefs, inp["xmin"], inp["xmax"], inp["nodes"])
    assert rc == 0 and v.shape == (2, q.shape[0])
    err = np.max(np.abs(v[0] - gold["values"][0]))
    tol = 1e-12 * max(np.max(np.abs(gold["values"][0])), 1e-300)
    print("golden 3d12: max error", err, "bar", tol)
    assert err <= tol
    assert np.array_equal(v[1], -0.5 * v[0])


@pytest.mark.gpu
def test_fields_evaluate_what_refit_wrote():
    """Plan.fit, then Plan.refit of two more fields into a (3, ncol + 8) tensor; evaluate_fields_dev straight on that tensor
    (its row stride is ldcoef): every row equals evaluate_dev on that row."""
    import torch
    nodes, m, nq = [12, 12, 12], 3000, 1000
    ncol = int(np.prod(nodes))
    rng = np.random.default_rng(12)
    dev = torch.device("cuda", 0)
    x = rng.uniform(0.0, 1.0, (m, 3))
    ys = np.stack([np.sin(3 * x[:, 0]) + x[:, 1] * x[:, 2], np.cos(2 * x[:, 1]) - x[:, 0], x[:, 0] * x[:, 1] + np.exp(-x[:, 2])])
    ys += 0.01 * rng.standard_normal(ys.shape)
    lo, hi = [0.0] * 3, [1.0] * 3
    plan = capi.Plan(3, nodes, lo, hi, 1.0, m)
    try:
        st = _stream()
        C3 = torch.full((3, ncol + 8), float("nan"), dtype=torch.float64, device=dev)
        xd, yd = _dev(x), _dev(ys)
        rc, _ = plan.fit(xd, yd[0], None, C3[0, :ncol], st)
        assert rc == 0
        rc, _ = plan.refit(yd[1:], C3[1:, :ncol], st)
        assert rc == 0
        torch.cuda.synchronize()
        q = _dev(rng.uniform(-0.1, 1.1, (nq, 3)))
        out = torch.full((3, nq), float("nan"), dtype=torch.float64, device=dev)
        assert capi.evaluate_fields_dev(3, q, None, C3[:, :ncol], lo, hi, nodes, out, st) == 0
        torch.cuda.synchronize()
        assert capi.debug_eval_fields_stats() == (1, 0, 1)
        for k in range(3):
            one = torch.full((nq,), float("nan"), dtype=torch.float64, device=dev)
            assert capi.evaluate_dev(3, q, None, C3[k, :ncol].contiguous(), lo, hi, nodes, one, st) == 0
            torch.cuda.synchronize()
            assert torch.equal(out[k], one), k
        assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0.1
        # the fitted fields are distinct functions
        assert not torch.equal(out[0], out[1]) and not torch.equal(out[1], out[2])
    finally:
        plan.close()
