"""Every device entry with an array, or an offset into an array, of 2^31 and 2^32 elements and more.

The C ABI takes such shapes by design (nq, offsets[], npts[] and every ld* but ldxq / l1xdat are int64_t), and the kernels behind
the entries index with 64-bit products; this file is what holds that.  The method is the same for every entry:

  1. The boundary is reached with MEMORY, not work: a large leading dimension or stride where the entry has one (torch.empty,
     only the words the entry reads are written, through a strided view), REAL32 storage where the element count itself must
     be large.  Both 2^31 and 2^32 are crossed (an `unsigned` index survives the first) wherever the test then holds at most
     40 GiB; where it would hold more, 2^31 alone, and the docstring says so.
  2. EVERY element is checked, on the device, against the entry itself below the boundary: the inputs are periodic (query rows
     repeat every 4 099 rows, the last axis of a grid repeats with a short period, the problems of a batch repeat every M
     problems), every entry promises bits that do not depend on the position, so the whole output is its first period tiled --
     one reshaped comparison of the bits.  The boundaries fall strictly inside a period (asserted), for batches inside a problem.
  3. The first period (or the compact twin of a call whose stride alone is large) is held to the oracle at the bars the
     sibling files hold: EVAL_TOL for real64 values, COEF_TOL for coefficients, and for REAL32 values the bar
     test_config5_evaluation_at_full_size_1e8_queries holds them to.  Three families are NOT anchored here: the variances, the
     residual statistics with the medians, and the clipped fits are compared with the library's own host entry on the first
     period alone -- a check that position and batch do not matter, no more; what those entries compute is held to the
     reference by test_eval_many_var.py, test_eval_many.py, test_mad_many.py, test_fit_many_clip.py and test_fit_many_clip_mad.py.
  4. Nothing else is touched: the padding of the outputs and a guard of 4 096 words behind them keep a sentinel, the inputs
     keep their checksum.
  5. A test computes the bytes it holds, skips (with that number) when less than that plus 8 GiB is free -- never on an idle
     MI355X -- and releases everything at its end; one test at a time holds memory.

The shapes are rebuilt by the CPU tier at the top, which asserts their premises without a device: where 2^31 and 2^32 are crossed,
that a period straddles them, the tile counts of the grid cases, and the bytes.
"""
import functools
import gc
import traceback

import numpy as np
import pytest

from splpak_amd import capi
from tests.test_gpu_parity import COEF_TOL, EVAL_TOL

GIB = 1 << 30
B31, B32 = 1 << 31, 1 << 32
PERIOD = 4099                     # rows of queries / points after which the inputs repeat
GUARD = 4096                      # words behind every output that must keep the sentinel
SENT = -1.5 * 2.0 ** 100          # the sentinel: exact in both storage kinds, no result comes near it
HEADROOM = 8 * GIB
MAX_BYTES = 40 * GIB
REAL32_EVAL_TOL = 2e-6            # REAL32 values against the oracle on the widened inputs (test_gpu_parity.py, config 5)
MIXED = {2: [1, 0], 3: [0, 2, 1], 4: [1, 0, 2, 1]}


# ---------------------------------------------------------------------------------------------------------------
# The shapes (pure arithmetic: the CPU tier and the GPU tests read the same numbers)
def crossing(boundary, ld, period_rows):
    """Where element `boundary` of an array of rows `ld` words apart lies: (row, column, offset inside its period of rows)."""
    return boundary // ld, boundary % ld, boundary % (ld * period_rows)


# splpak_eval_dev_f32: the queries 256 words apart
EVAL_NQ, EVAL_LDXQ = (1 << 24) + PERIOD, 256
EVAL_GRIDS = [((20, 20), "region sort"), ((7, 20, 20), "run path"), ((19, 19, 19), "persistent"), ((19, 19, 19, 11), "persistent 4-D")]
EVAL_BYTES = 4 * EVAL_NQ * EVAL_LDXQ + 2 * 4 * (EVAL_NQ + GUARD) + 3 * GIB          # xq, two outputs, the paths' scratch
# splpak_eval_derivs_dev_f64: the results 128 words apart (16 GiB of real64: 2^31 alone)
DERIVS_NODES, DERIVS_LDOUT = (20, 17, 30), 128
DERIVS_BYTES = 8 * (EVAL_NQ * DERIVS_LDOUT + GUARD) + 8 * EVAL_NQ * 3 + 3 * GIB
# splpak_eval_fields_dev_f32: five fields 2^30 + 7 results, or 2^30 + 5 coefficients, apart
FIELDS_NODES, FIELDS_NF, FIELDS_NQ = (20, 17, 30), 5, 50_000
FIELDS_LDOUT, FIELDS_LDCOEF = (1 << 30) + 7, (1 << 30) + 5
FIELDS_BYTES = 4 * ((FIELDS_NF - 1) * FIELDS_LDOUT + FIELDS_NQ + GUARD) + GIB
# splpak_eval_grid_dev_f32: the output count itself; the last axis repeats with period `p`
GRID_CASES = {
    "2d": dict(nodes=(40, 33), npts=(65_537, 65_539), p=7),
    "3d": dict(nodes=(20, 17, 30), npts=(1_627, 1_621, 1_630), p=7),
    "4d": dict(nodes=(12, 9, 8, 14), npts=(257, 255, 259, 254), p=5),
}
GRID_TILES = {2: (64, 16), 3: (64, 8, 8), 4: (16, 4, 4, 4)}          # GTile<D>::T of csrc/evalgrid.hip
# splpak_eval_grid_derivs_dev_f32: ten planes 2^29 + 3 apart
GDERIVS_NODES, GDERIVS_NPTS, GDERIVS_LDOUT = (20, 17, 30), (40, 37, 41), (1 << 29) + 3
GDERIVS_NPLANES = 10
GDERIVS_BYTES = 4 * ((GDERIVS_NPLANES - 1) * GDERIVS_LDOUT + int(np.prod(GDERIVS_NPTS)) + GUARD) + GIB
# splpak_fit_many_dev_f32 / splpak_fit_many_cov_dev_f32: 2^22 + 3 problems of 24 points, coefficients (covariances) 1 031 apart
MANY_NB, MANY_NP, MANY_NODES, MANY_LD, MANY_M = (1 << 22) + 3, 24, (8,), 1031, 7
MANY_BYTES = 4 * (MANY_NB * MANY_LD + GUARD) + 3 * 4 * MANY_NB * MANY_NP + GIB
# splpak_fit_many_dev_f32, 2-D: 5 x 9 nodes, the points 64 words apart
MANY2_NODES, MANY2_L1, MANY2_NP, MANY2_M = (5, 9), 64, 200, 7
MANY2_NB = (B32 // (MANY2_L1 * MANY2_NP)) + 2 * MANY2_M + 3
MANY2_BYTES = 4 * MANY2_NB * MANY2_NP * (MANY2_L1 + 1) + 4 * (MANY2_NB * 45 + GUARD) + GIB
# splpak_fit_grid_dev_f32 / splpak_fit_grid_weighted_dev_f32: five fields of samples (and weights) 2^30 + 7 apart
FITGRID_NF, FITGRID_LDV = 5, (1 << 30) + 7


def grid_elements(case):
    return int(np.prod([int(n) for n in case["npts"]], dtype=object))


def grid_bytes(case):
    return 4 * (grid_elements(case) + GUARD) + GIB


def grid_tiles(case):
    """(tiles of one tile layer of the last dimension, tiles of the launch) by the rule of eval_grid_slab / launch_eval_grid_tables."""
    t = GRID_TILES[len(case["npts"])]
    per = [-(-n // tt) for n, tt in zip(case["npts"], t)]
    return int(np.prod(per[:-1], dtype=object)), int(np.prod(per, dtype=object))


# ---------------------------------------------------------------------------------------------------------------
# CPU tier: the premises of the shapes
def test_shapes_strided_queries_cross_both_boundaries_inside_a_period():
    assert EVAL_NQ * EVAL_LDXQ == 4_296_016_640 > B32
    r31, c31, in31 = crossing(B31, EVAL_LDXQ, PERIOD)
    r32, c32, in32 = crossing(B32, EVAL_LDXQ, PERIOD)
    assert (r31, c31) == (1 << 23, 0) and (r32, c32) == (1 << 24, 0)          # rows from 2^23 on lie past 2^31, the last 4 099 past 2^32
    assert EVAL_NQ - r32 == PERIOD
    assert in31 != 0 and in32 != 0 and r31 % PERIOD != 0 and r32 % PERIOD != 0       # strictly inside a period of rows
    assert EVAL_BYTES <= MAX_BYTES
    # results 128 words apart: real64, 2^31 alone
    assert B31 < EVAL_NQ * DERIVS_LDOUT < B32
    r, c, inside = crossing(B31, DERIVS_LDOUT, PERIOD)
    assert (r, c) == (1 << 24, 0) and r < EVAL_NQ and inside != 0
    assert DERIVS_BYTES <= MAX_BYTES


def test_shapes_field_and_plane_strides_put_whole_fields_past_the_boundaries():
    nq = FIELDS_NQ
    for ld, n in ((FIELDS_LDOUT, nq), (FIELDS_LDCOEF, int(np.prod(FIELDS_NODES)))):
        first = [k * ld for k in range(FIELDS_NF)]
        assert first[1] + n < B31 < first[2] and first[3] + n < B32 < first[4]          # field 2 starts past 2^31, field 4 past 2^32
    assert FIELDS_BYTES <= MAX_BYTES
    first = [e * GDERIVS_LDOUT for e in range(GDERIVS_NPLANES)]
    n = int(np.prod(GDERIVS_NPTS))
    assert first[3] + n < B31 < first[4] and first[7] + n < B32 < first[8]              # plane 4 past 2^31, plane 8 past 2^32
    assert GDERIVS_BYTES <= MAX_BYTES
    first = [k * FITGRID_LDV for k in range(FITGRID_NF)]
    assert first[1] < B31 < first[2] and first[3] < B32 < first[4]


@pytest.mark.parametrize("name", sorted(GRID_CASES))
def test_shapes_grid_outputs_cross_both_boundaries_inside_a_period(name):
    case = GRID_CASES[name]
    n = grid_elements(case)
    assert n == {"2d": 4_295_229_443, "3d": 4_298_908_210, "4d": 4_311_285_510}[name] > B32
    rest = n // case["npts"][-1]
    period = rest * case["p"]
    for b in (B31, B32):
        assert b % period != 0 and b % rest != 0          # strictly inside a period, and inside a position of the last axis
        assert b + period < n or b == B32                 # whole periods follow the first boundary
    row_tiles, tiles = grid_tiles(case)
    assert row_tiles <= 0x7fffffff and tiles <= 0x7fffffff          # one launch, no slab
    assert grid_bytes(case) <= MAX_BYTES


def test_shapes_batches_of_small_fits_cross_both_boundaries_inside_a_problem():
    assert (1 << 22) * MANY_LD == 4_324_327_424 > B32
    for b in (B31, B32):
        k, c, inside = crossing(b, MANY_LD, MANY_M)
        assert k < MANY_NB and inside != 0
    assert MANY_BYTES <= MAX_BYTES
    # 2-D, points 64 words apart: p * l1xdat crosses inside a problem's own points
    per_problem = MANY2_NP * MANY2_L1
    assert MANY2_NB * per_problem > B32
    for b in (B31, B32):
        assert b % per_problem != 0 and b % (per_problem * MANY2_M) != 0
    assert MANY2_BYTES <= MAX_BYTES


# ---------------------------------------------------------------------------------------------------------------
# GPU tier: helpers
def big_memory(nbytes):
    """The memory discipline of this file: skip when `nbytes` + 8 GiB is not free; whatever the test held is released at its end,
    also after a failure (the frames of the traceback hold the tensors otherwise)."""
    def deco(fn):
        @functools.wraps(fn)
        def wrapper(*args, **kwargs):
            import torch
            need = nbytes(*args, **kwargs) if callable(nbytes) else nbytes
            capi.shutdown()
            gc.collect()
            torch.cuda.empty_cache()
            free = torch.cuda.mem_get_info()[0]
            if free < need + HEADROOM:
                pytest.skip(f"needs {need} bytes of device memory and 8 GiB of headroom, {free} are free")
            try:
                return fn(*args, **kwargs)
            except BaseException as e:
                traceback.clear_frames(e.__traceback__)
                raise
            finally:
                capi.set_eval_mode(capi.EVAL_AUTO)
                capi.shutdown()
                gc.collect()
                torch.cuda.empty_cache()
        return wrapper
    return deco


def _dev():
    import torch
    return torch.device("cuda", 0)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    import torch
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def tiled_mismatch(x, period, chunk=1 << 27):
    """x: (n, m) tensor, rows possibly strided.  True (a 0-d device tensor) where some row differs in a bit from the row `period`
    rows before it -- i.e. x is not its first `period` rows tiled.  Compared in pieces of about `chunk` elements."""
    import torch
    n, m = x.shape
    xb = _bits(x)
    first = xb[:period].clone()
    bad = torch.zeros((), dtype=torch.bool, device=x.device)
    k = n // period
    step = max(1, chunk // (period * m))
    body = xb[:k * period].unflatten(0, (k, period))
    for a in range(0, k, step):
        bad |= (body[a:a + step] != first).any()
    tail = n - k * period
    if tail:
        bad |= (xb[k * period:] != first[:tail]).any()
    return bad


def not_sentinel(flat, chunk=1 << 28):
    """True (0-d device tensor) where some word of the 1-D or 2-D tensor `flat` is not the sentinel."""
    import torch
    bad = torch.zeros((), dtype=torch.bool, device=flat.device)
    rows = max(1, chunk // max(int(flat.shape[-1]), 1)) if flat.dim() == 2 else chunk
    for a in range(0, int(flat.shape[0]), rows):
        bad |= (flat[a:a + rows] != SENT).any()
    return bad


def checksum(t):
    """Sum of the words of `t` as integers (0-d int64 device tensor)."""
    import torch
    return _bits(t).sum(dtype=torch.int64)


def query_period(nd, seed, dtype=np.float32):
    """4 099 query rows in [-0.1, 1.1]^nd, the corners of the box among them."""
    rng = np.random.default_rng(seed)
    q = rng.uniform(-0.1, 1.1, (PERIOD, nd))
    q[:16] = rng.integers(0, 2, (16, nd))
    return q.astype(dtype)


def eval_scale(vo, coef, nodes, pat):
    """The scale the evaluation bars of test_gpu_parity.py are relative to (unit box)."""
    d = float(np.prod((np.array(nodes, dtype=np.float64) - 1.0) ** np.array(pat if pat is not None else [0] * len(nodes))))
    return max(float(np.max(np.abs(vo))), float(np.max(np.abs(coef))) * d)


def derivs_patterns(nd, order):
    pats = [[0] * nd] + [[int(e == d) for e in range(nd)] for d in range(nd)]
    if order == 2:
        pats += [[int(e == d) + int(e == f) for e in range(nd)] for d in range(nd) for f in range(d, nd)]
    return pats


# ---------------------------------------------------------------------------------------------------------------
# splpak_eval_dev_f32
@pytest.mark.gpu
@big_memory(EVAL_BYTES)
def test_eval_dev_f32_queries_256_words_apart_past_2_32(port):
    """xq of (2^24 + 4 099) x 256 REAL32 words, 4 296 016 640 elements: the rows from 2^23 on lie past 2^31, the last 4 099 past
    2^32.  The four grids of test_eval_scratch_of_every_path_across_streams_regrowth_and_threads, so that the direct kernel and
    each sorted path (forced by EVAL_BINNED) reads the strided queries; values and one derivative pattern.  Every result must be
    the bits of the result 4 099 rows before it, the sorted path's the direct kernel's, the first 2 000 the oracle's."""
    import torch
    dev, st = _dev(), _stream()
    nq, ld = EVAL_NQ, EVAL_LDXQ
    qh = query_period(4, 3101)
    xq = torch.empty((nq, ld), dtype=torch.float32, device=dev)
    k = nq // PERIOD
    xq[:k * PERIOD, :4].unflatten(0, (k, PERIOD)).copy_(_to_dev(qh))
    xq[k * PERIOD:, :4].copy_(_to_dev(qh[:nq - k * PERIOD]))
    assert xq.stride() == (ld, 1) and xq.numel() > B32
    before = checksum(xq[:, :4])
    outs = [torch.full((nq + GUARD,), SENT, dtype=torch.float32, device=dev) for _ in range(2)]
    rng = np.random.default_rng(3102)
    for nodes, what in EVAL_GRIDS:
        nd = len(nodes)
        lo, hi = [0.0] * nd, [1.0] * nd
        ch = rng.standard_normal(int(np.prod(nodes))).astype(np.float32)
        coef = _to_dev(ch)
        for pat in (None, MIXED[nd]):
            for o, mode in zip(outs, (capi.EVAL_DIRECT, capi.EVAL_BINNED)):
                o.fill_(SENT)
                capi.set_eval_mode(mode, 0)
                # (the entry reads columns 0 .. nd-1 of the rows it is given: the 4-D queries serve every grid)
                assert capi.evaluate_dev(nd, xq, pat, coef, lo, hi, nodes, o, st) == 0
            bad = tiled_mismatch(outs[0][:nq].unsqueeze(1), PERIOD)
            same = torch.equal(_bits(outs[0]), _bits(outs[1]))
            guard = not_sentinel(outs[0][nq:]) | not_sentinel(outs[1][nq:])
            assert not bool(bad), (what, pat)
            assert same, (what, pat)
            assert not bool(guard), (what, pat)
            vo, _ = port.evaluate(nd, qh[:2000, :nd].astype(np.float64), pat, ch.astype(np.float64), lo, hi, nodes)
            got = outs[0][:2000].cpu().numpy().astype(np.float64)
            assert np.max(np.abs(got - vo)) <= REAL32_EVAL_TOL * eval_scale(vo, ch, nodes, pat), (what, pat)
    assert int(checksum(xq[:, :4])) == int(before)


# ---------------------------------------------------------------------------------------------------------------
# splpak_eval_derivs_dev_f64
@pytest.mark.gpu
@big_memory(DERIVS_BYTES)
def test_eval_derivs_dev_f64_results_128_words_apart_past_2_31(port):
    """Compact queries, `out` with ldout = 128 for 2^24 + 4 099 queries: 16 GiB of real64, so 2^31 alone is crossed (element 2^31
    is the value of query 2^24; both boundaries would take 32 GiB of real64 at this ldout).  Order 2 on (20, 17, 30), the direct
    kernel and the region sort.  Ten results per row, each the bits of the row 4 099 before; 118 sentinels behind them."""
    import torch
    dev, st = _dev(), _stream()
    nq, ld, nodes, nd = EVAL_NQ, DERIVS_LDOUT, DERIVS_NODES, 3
    nout = capi.derivs_nout(nd, 2)
    lo, hi = [0.0] * nd, [1.0] * nd
    qh = query_period(nd, 3201, np.float64)
    k = nq // PERIOD
    xq = torch.empty((nq, nd), dtype=torch.float64, device=dev)
    xq[:k * PERIOD].unflatten(0, (k, PERIOD)).copy_(_to_dev(qh))
    xq[k * PERIOD:].copy_(_to_dev(qh[:nq - k * PERIOD]))
    ch = np.random.default_rng(3202).standard_normal(int(np.prod(nodes)))
    coef = _to_dev(ch)
    before = checksum(xq) + checksum(coef)
    flat = torch.empty(nq * ld + GUARD, dtype=torch.float64, device=dev)
    out = flat[:nq * ld].view(nq, ld)
    assert flat.numel() > B31
    first = None
    for mode in (capi.EVAL_DIRECT, capi.EVAL_BINNED):
        flat.fill_(SENT)
        capi.set_eval_mode(mode, 0)
        assert capi.evaluate_derivs_dev(nd, xq, 2, coef, lo, hi, nodes, out, st) == 0
        bad = tiled_mismatch(out[:, :nout], PERIOD)
        pad = not_sentinel(out[:, nout:]) | not_sentinel(flat[nq * ld:])
        assert not bool(bad), mode
        assert not bool(pad), mode
        head = out[:PERIOD, :nout].clone()
        if first is None:
            first = head
        assert torch.equal(_bits(head), _bits(first))          # the region sort returns the direct kernel's bits
    got = first[:2000].cpu().numpy()
    for j, p in enumerate(derivs_patterns(nd, 2)):
        vo, _ = port.evaluate(nd, qh[:2000], p, ch, lo, hi, nodes)
        assert np.max(np.abs(got[:, j] - vo)) <= EVAL_TOL * eval_scale(vo, ch, nodes, p), p
    assert int(checksum(xq) + checksum(coef)) == int(before)


# ---------------------------------------------------------------------------------------------------------------
# splpak_eval_fields_dev_f32
def _fields_inputs():
    nodes, nd = FIELDS_NODES, 3
    rng = np.random.default_rng(3301)
    qh = rng.uniform(-0.1, 1.1, (FIELDS_NQ, nd)).astype(np.float32)
    ch = rng.standard_normal((FIELDS_NF, int(np.prod(nodes)))).astype(np.float32)
    return nodes, nd, qh, ch


def _fields_compact(port, xq, coef, qh, ch, nodes, pat):
    """The entry itself below the boundary: packed fields under the direct kernel, anchored to the oracle field by field."""
    import torch
    nd = len(nodes)
    lo, hi = [0.0] * nd, [1.0] * nd
    want = torch.full((FIELDS_NF, FIELDS_NQ), SENT, dtype=torch.float32, device=xq.device)
    capi.set_eval_mode(capi.EVAL_DIRECT)
    assert capi.evaluate_fields_dev(nd, xq, pat, coef, lo, hi, nodes, want, _stream()) == 0
    assert capi.debug_eval_fields_stats()[0] == 1
    got = want[:, :2000].cpu().numpy().astype(np.float64)
    for f in range(FIELDS_NF):
        vo, _ = port.evaluate(nd, qh[:2000].astype(np.float64), pat, ch[f].astype(np.float64), lo, hi, nodes)
        assert np.max(np.abs(got[f] - vo)) <= REAL32_EVAL_TOL * eval_scale(vo, ch[f], nodes, pat), (f, pat)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["ldout", "ldcoef"])
@big_memory(FIELDS_BYTES)
def test_eval_fields_dev_f32_fields_2_30_words_apart(port, which):
    """Five fields at 50 000 queries on (20, 17, 30).  "ldout": the results 2^30 + 7 apart, so field 2 starts past 2^31 and field 4
    past 2^32; "ldcoef": the coefficients 2^30 + 5 apart, likewise.  The direct fields kernel (route 1) and the shared sort of
    the persistent region path (route 2, EVAL_BINNED), the route asserted; values and a derivative pattern.  Every field must
    have the bits of the packed call; the words between the fields and behind the last keep the sentinel."""
    import torch
    dev, st = _dev(), _stream()
    nodes, nd, qh, ch = _fields_inputs()
    ncol, nf, nq = ch.shape[1], FIELDS_NF, FIELDS_NQ
    lo, hi = [0.0] * nd, [1.0] * nd
    xq, cpack = _to_dev(qh), _to_dev(ch)
    if which == "ldout":
        ld = FIELDS_LDOUT
        flat = torch.empty((nf - 1) * ld + nq + GUARD, dtype=torch.float32, device=dev)
        out = torch.as_strided(flat, (nf, nq), (ld, 1))
        coef = cpack
    else:
        ld = FIELDS_LDCOEF
        cflat = torch.empty((nf - 1) * ld + ncol, dtype=torch.float32, device=dev)
        coef = torch.as_strided(cflat, (nf, ncol), (ld, 1))
        coef.copy_(cpack)
        flat = torch.empty(nf * nq + GUARD, dtype=torch.float32, device=dev)
        out = flat[:nf * nq].view(nf, nq)
    assert (nf - 1) * ld > B32
    before = checksum(coef) + checksum(xq)
    for pat in (None, MIXED[nd]):
        want = _fields_compact(port, xq, cpack, qh, ch, nodes, pat)
        for mode, route in ((capi.EVAL_AUTO, 1), (capi.EVAL_BINNED, 2)):
            flat.fill_(SENT)
            capi.set_eval_mode(mode, 0)
            assert capi.evaluate_fields_dev(nd, xq, pat, coef, lo, hi, nodes, out, st) == 0
            assert capi.debug_eval_fields_stats()[0] == route
            same = torch.equal(_bits(out), _bits(want))
            out.fill_(SENT)          # what is left must be all sentinel: the gaps and the guard
            assert same, (pat, route)
            assert not bool(not_sentinel(flat)), (pat, route)
    assert int(checksum(coef) + checksum(xq)) == int(before)


# ---------------------------------------------------------------------------------------------------------------
# splpak_eval_grid_dev_f32
def _grid_axes(case, form, seed):
    """The axes of a grid case, back to back, REAL32.  All but the last: npts[d] ascending coordinates over [-0.02, 1.02]
    ("gather", 3-D: those of dimension 2 in turn from [-0.02, 0.1] and [0.9, 1.02], window starts 0 and 13 of the 17 nodes, so
    that the 8 of every tile span the grid and its coefficient box -- 17 x 4 rows, 64 x 68 first partial sums -- is beyond the
    LDS budget of 5 376 doubles).  The last: `p` coordinates inside one cell of the node grid, repeated."""
    rng = np.random.default_rng(seed)
    nodes, npts, p = case["nodes"], case["npts"], case["p"]
    axes = [np.linspace(-0.02, 1.02, n) for n in npts[:-1]]
    if form == "gather":
        m = npts[1]
        axes[1] = np.stack([np.linspace(-0.02, 0.1, (m + 1) // 2), np.linspace(0.9, 1.02, (m + 1) // 2)], axis=1).ravel()[:m]
    cell = 1.0 / (nodes[-1] - 1)
    base = (nodes[-1] // 2 + rng.uniform(0.05, 0.95, p)) * cell
    axes.append(np.tile(base, -(-npts[-1] // p))[:npts[-1]])
    return [a.astype(np.float32) for a in axes]


GRID_RUNS = [("2d", "lds", None), ("3d", "lds", None), ("3d", "lds", MIXED[3]), ("4d", "lds", None), ("3d", "gather", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,form,pat", GRID_RUNS, ids=[f"{n}-{f}-{'values' if p is None else 'derivs'}" for n, f, p in GRID_RUNS])
@big_memory(lambda port, name, form, pat: grid_bytes(GRID_CASES[name]))
def test_eval_grid_dev_f32_more_than_2_32_outputs(port, name, form, pat):
    """npts (65 537, 65 539), (1 627, 1 621, 1 630) and (257, 255, 259, 254): 4.3e9 REAL32 outputs, past 2^32.  The last axis
    repeats with a period of 7 (5) coordinates, so the output is its first 7 (5) positions of the last dimension tiled, and both
    boundaries fall inside a period.  "lds": sorted axes, the tiles stage their coefficient box in LDS (asserted); "gather":
    dimension 2 unsorted, every tile gathers from global memory (asserted).  2 000 outputs of the first period against the oracle."""
    import torch
    dev, st = _dev(), _stream()
    case = GRID_CASES[name]
    nodes, npts, p = case["nodes"], case["npts"], case["p"]
    nd = len(nodes)
    lo, hi = [0.0] * nd, [1.0] * nd
    n = grid_elements(case)
    rest = n // npts[-1]
    axes_h = _grid_axes(case, form, 3400 + nd)
    ch = np.random.default_rng(3401 + nd).standard_normal(int(np.prod(nodes))).astype(np.float32)
    axes, coef = _to_dev(np.concatenate(axes_h)), _to_dev(ch)
    before = checksum(axes) + checksum(coef)
    flat = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=dev)
    assert flat.numel() > B32
    assert capi.evaluate_grid_dev(nd, npts, axes, pat, coef, lo, hi, nodes, flat, st) == 0
    lds, general = capi.debug_eval_grid_stats()
    assert lds + general == grid_tiles(case)[1]
    assert (lds > 0 and general == 0) if form == "lds" else (general > 0 and lds == 0), (lds, general)
    bad = tiled_mismatch(flat[:n].view(npts[-1], rest), p)
    assert not bool(bad)
    assert not bool(not_sentinel(flat[n:]))
    # the first period against the oracle
    rng = np.random.default_rng(3402)
    idx = rng.integers(0, rest * p, 2000)
    idx[:4] = [0, npts[0] - 1, rest - 1, rest * p - 1]
    sub, rem = [], idx.copy()
    for d in range(nd):
        sub.append(rem % npts[d])
        rem = rem // npts[d]
    q = np.stack([axes_h[d][sub[d]] for d in range(nd)], axis=1).astype(np.float64)
    vo, _ = port.evaluate(nd, q, pat, ch.astype(np.float64), lo, hi, nodes)
    got = flat[_to_dev(idx)].cpu().numpy().astype(np.float64)
    assert np.max(np.abs(got - vo)) <= REAL32_EVAL_TOL * eval_scale(vo, ch, nodes, pat)
    assert int(checksum(axes) + checksum(coef)) == int(before)


# ---------------------------------------------------------------------------------------------------------------
# splpak_eval_grid_derivs_dev_f32
@pytest.mark.gpu
@big_memory(GDERIVS_BYTES)
def test_eval_grid_derivs_dev_f32_planes_2_29_words_apart(port):
    """3-D order 2, ten planes of (40, 37, 41) points with ldout = 2^29 + 3: plane 4 lies past 2^31, plane 8 past 2^32.  Every plane
    must have the bits of the packed call (ldout = the points of a plane), which is anchored to the oracle pattern by pattern;
    the words between the planes and behind the last keep the sentinel."""
    import torch
    dev, st = _dev(), _stream()
    nodes, npts, ld, nd = GDERIVS_NODES, GDERIVS_NPTS, GDERIVS_LDOUT, 3
    lo, hi = [0.0] * nd, [1.0] * nd
    npl, n = GDERIVS_NPLANES, int(np.prod(GDERIVS_NPTS))
    assert capi.derivs_nout(nd, 2) == npl
    rng = np.random.default_rng(3501)
    axes_h = [np.sort(rng.uniform(-0.05, 1.05, m)).astype(np.float32) for m in npts]
    ch = rng.standard_normal(int(np.prod(nodes))).astype(np.float32)
    axes, coef = _to_dev(np.concatenate(axes_h)), _to_dev(ch)
    before = checksum(axes) + checksum(coef)
    want = torch.full((npl, n), SENT, dtype=torch.float32, device=dev)
    assert capi.evaluate_grid_derivs_dev(nd, npts, axes, 2, coef, lo, hi, nodes, want, st) == 0
    idx = rng.integers(0, n, 2000)
    q = np.stack([axes_h[0][idx % npts[0]], axes_h[1][(idx // npts[0]) % npts[1]], axes_h[2][idx // (npts[0] * npts[1])]], axis=1).astype(np.float64)
    got = want[:, _to_dev(idx)].cpu().numpy().astype(np.float64)
    for e, pat in enumerate(derivs_patterns(nd, 2)):
        vo, _ = port.evaluate(nd, q, pat, ch.astype(np.float64), lo, hi, nodes)
        assert np.max(np.abs(got[e] - vo)) <= REAL32_EVAL_TOL * eval_scale(vo, ch, nodes, pat), pat
    flat = torch.full(((npl - 1) * ld + n + GUARD,), SENT, dtype=torch.float32, device=dev)
    out = torch.as_strided(flat, (npl, n), (ld, 1))
    assert (npl - 1) * ld > B32
    assert capi.evaluate_grid_derivs_dev(nd, npts, axes, 2, coef, lo, hi, nodes, out, st) == 0
    same = torch.equal(_bits(out), _bits(want))
    out.fill_(SENT)
    assert same
    assert not bool(not_sentinel(flat))
    assert int(checksum(axes) + checksum(coef)) == int(before)


# ---------------------------------------------------------------------------------------------------------------
# splpak_fit_many_dev_f32, splpak_fit_many_cov_dev_f32
def fill_tiled(dst, period):
    """dst (n, m), rows possibly strided, := the rows of `period` (P, m) over and over."""
    n, P = int(dst.shape[0]), int(period.shape[0])
    k = n // P
    if k:
        dst[:k * P].unflatten(0, (k, P)).copy_(period)
    if n > k * P:
        dst[k * P:].copy_(period[:n - k * P])


def _many_period(nd, nper, m, seed):
    """`m` problems of `nper` points each on the unit box, REAL32: the points on a jittered lattice (every cell of the node grids
    used here holds some), smooth values plus noise.  -> (x (m * nper, nd), y)."""
    rng = np.random.default_rng(seed)
    if nd == 1:
        u = ((np.arange(nper)[None, :] + rng.uniform(0.1, 0.9, (m, nper))) / nper).reshape(-1, 1)
    else:
        a, b = 10, nper // 10
        i, j = np.meshgrid(np.arange(a), np.arange(b), indexing="ij")
        u = np.stack([(i.ravel()[None, :] + rng.uniform(0.1, 0.9, (m, a * b))) / a, (j.ravel()[None, :] + rng.uniform(0.1, 0.9, (m, a * b))) / b],
                     axis=2).reshape(-1, 2)
    y = np.sin(3.0 * u[:, 0]) + 0.5 * np.cos(2.0 * u[:, -1]) + 0.05 * rng.standard_normal(u.shape[0])
    return u.astype(np.float32), y.astype(np.float32)


def _many_anchor(port, nd, nodes, xtrap, x32, y32, m, nper, with_cov=False):
    """The first period below the boundary: the real64 entry on the widened inputs -- every problem against the oracle at COEF_TOL --
    rounded once, which is what the REAL32 entry promises bit for bit (test_bits_do_not_depend_on_the_batch_the_position_or_the_entry,
    test_f32_is_the_f64_entry_on_the_widened_inputs_rounded_once).  -> (coef (m, ncol) float32, cov or None)."""
    lo, hi = [0.0] * nd, [1.0] * nd
    off = np.arange(m + 1, dtype=np.int64) * nper
    x64, y64 = x32.astype(np.float64), y32.astype(np.float64)
    cov = None
    if with_cov:
        c64, v64, rc, st, _ = capi.fit_many_cov(nd, off, x64, y64, None, lo, hi, list(nodes), xtrap)
        cov = v64.astype(np.float32)
    else:
        c64, rc, st, _ = capi.fit_many(nd, off, x64, y64, None, lo, hi, list(nodes), xtrap)
    assert rc == 0 and not st.any()
    for k in range(m):
        c_ref, rc_ref, _ = port.fit(nd, x64[k * nper:(k + 1) * nper], y64[k * nper:(k + 1) * nper], None, lo, hi, list(nodes), xtrap)
        assert rc_ref == 0
        err = float(np.max(np.abs(c64[k] - c_ref[:c64.shape[1]])) / np.max(np.abs(c_ref[:c64.shape[1]])))
        assert err < COEF_TOL, (k, err)
    return c64.astype(np.float32), cov


def _host_rows_tiled(a, m):
    """Rows of the host array `a` repeat with period m."""
    k = a.shape[0] // m
    return np.array_equal(a[:k * m].reshape(k, m, -1), np.broadcast_to(a[:m].reshape(1, m, -1), (k, m, a[:m].reshape(m, -1).shape[1]))) and \
        np.array_equal(a[k * m:], a[:a.shape[0] - k * m])


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["ldcoef", "ldcov"])
@big_memory(MANY_BYTES)
def test_fit_many_dev_f32_rows_1031_words_apart_past_2_32(port, which):
    """2^22 + 3 problems of 24 points on 8 nodes, seven different ones over and over.  "ldcoef": splpak_fit_many_dev_f32 with the
    coefficients 1 031 words apart ((2^22) 1 031 = 4 324 327 424: the rows from 2 082 913 on lie past 2^31, from 4 165 826 on past
    2^32); "ldcov": splpak_fit_many_cov_dev_f32 with the covariances that far apart.  Every row must have the bits of the row seven
    before it, the first seven those of the real64 entry rounded once, which meets the oracle at COEF_TOL; the 1 023 (999) words
    behind every row and the guard keep the sentinel."""
    import torch
    dev, st = _dev(), _stream()
    nb, nper, nodes, ld, m = MANY_NB, MANY_NP, MANY_NODES, MANY_LD, MANY_M
    ncol, xtrap = nodes[0], 1.0
    covlen = capi.fit_many_cov_len(1, list(nodes))
    xh, yh = _many_period(1, nper, m, 3601)
    want_c, want_v = _many_anchor(port, 1, nodes, xtrap, xh, yh, m, nper, with_cov=which == "ldcov")
    x = torch.empty((nb * nper, 1), dtype=torch.float32, device=dev)
    y = torch.empty((nb * nper, 1), dtype=torch.float32, device=dev)
    fill_tiled(x, _to_dev(xh))
    fill_tiled(y, _to_dev(yh.reshape(-1, 1)))
    before = checksum(x) + checksum(y)
    off = np.arange(nb + 1, dtype=np.int64) * nper
    flat = torch.full((nb * ld + GUARD,), SENT, dtype=torch.float32, device=dev)
    rows = flat[:nb * ld].view(nb, ld)
    assert nb * ld > B32
    if which == "ldcoef":
        rc, status, info = capi.fit_many_dev(1, off, x, y, None, [0.0], [1.0], list(nodes), flat, xtrap=xtrap, ldcoef=ld, stream=st)
        live, want = ncol, want_c
    else:
        cflat = torch.full((nb * ncol + GUARD,), SENT, dtype=torch.float32, device=dev)
        rc, status, info = capi.fit_many_cov_dev(1, off, x, y, None, [0.0], [1.0], list(nodes), cflat, flat, xtrap=xtrap, ldcov=ld, stream=st)
        live, want = covlen, want_v
        coef = cflat[:nb * ncol].view(nb, ncol)
        assert not bool(tiled_mismatch(coef, m)) and not bool(not_sentinel(cflat[nb * ncol:]))
        assert torch.equal(_bits(coef[:m]), _bits(_to_dev(want_c)))
    torch.cuda.synchronize()
    assert rc == 0 and not status.any()
    assert _host_rows_tiled(info, m)
    assert not bool(tiled_mismatch(rows[:, :live], m))
    assert torch.equal(_bits(rows[:m, :live]), _bits(_to_dev(want)))
    assert not bool(not_sentinel(rows[:, live:]))
    assert not bool(not_sentinel(flat[nb * ld:]))
    assert int(checksum(x) + checksum(y)) == int(before)


@pytest.mark.gpu
@big_memory(MANY2_BYTES)
def test_fit_many_dev_f32_points_64_words_apart_past_2_32(port):
    """2-D, 5 x 9 nodes, 200 points per problem with l1xdat = 64: xdata holds 4.3e9 words, `p * l1xdat` passes 2^31 at point 32 of
    problem 167 772 and 2^32 at point 64 of problem 335 544, both inside a problem's own points (the CPU tier asserts it).  Seven
    different problems over and over: every row of coefficients must have the bits of the row seven before it, the first seven
    those of the real64 entry on the packed points rounded once, which meets the oracle at COEF_TOL."""
    import torch
    dev, st = _dev(), _stream()
    nb, nper, nodes, l1, m = MANY2_NB, MANY2_NP, MANY2_NODES, MANY2_L1, MANY2_M
    ncol = int(np.prod(nodes))
    xh, yh = _many_period(2, nper, m, 3701)
    want, _ = _many_anchor(port, 2, nodes, 0.0, xh, yh, m, nper)
    x = torch.empty((nb * nper, l1), dtype=torch.float32, device=dev)
    y = torch.empty((nb * nper, 1), dtype=torch.float32, device=dev)
    fill_tiled(x[:, :2], _to_dev(xh))
    fill_tiled(y, _to_dev(yh.reshape(-1, 1)))
    assert x.numel() > B32 and x.stride() == (l1, 1)
    before = checksum(x[:, :2]) + checksum(y)
    off = np.arange(nb + 1, dtype=np.int64) * nper
    flat = torch.full((nb * ncol + GUARD,), SENT, dtype=torch.float32, device=dev)
    rc, status, info = capi.fit_many_dev(2, off, x, y, None, [0.0, 0.0], [1.0, 1.0], list(nodes), flat, xtrap=0.0, stream=st)
    torch.cuda.synchronize()
    assert rc == 0 and not status.any()
    assert _host_rows_tiled(info, m)
    coef = flat[:nb * ncol].view(nb, ncol)
    assert not bool(tiled_mismatch(coef, m))
    assert torch.equal(_bits(coef[:m]), _bits(_to_dev(want)))
    assert not bool(not_sentinel(flat[nb * ncol:]))
    assert int(checksum(x[:, :2]) + checksum(y)) == int(before)


# ---------------------------------------------------------------------------------------------------------------
# splpak_fit_grid_dev_f32, splpak_fit_grid_weighted_dev_f32
FITGRID_BYTES = {False: 4 * ((FITGRID_NF - 1) * FITGRID_LDV + 23 * 17) + GIB, True: 2 * 4 * ((FITGRID_NF - 1) * FITGRID_LDV + 23 * 17) + GIB}


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True], ids=["fit_grid", "fit_grid_weighted"])
@big_memory(lambda port, weighted: FITGRID_BYTES[weighted])
def test_fit_grid_dev_f32_fields_2_30_samples_apart(port, weighted):
    """Five fields on the "2d" parity shape of test_fit_grid.py (23 x 17 samples, 6 x 5 nodes) with ldv (weighted: and ldw, a weight
    array per field) = 2^30 + 7: field 2 starts past 2^31, field 4 past 2^32.  The coefficients must have the bits of the call with
    the fields packed; those are the real64 entry on the widened inputs rounded once (test_fit_grid_entry_forms_and_real32), which
    meets the oracle's fit of the listed samples at COEF_TOL field by field."""
    import torch
    from tests.test_fit_grid import HI, LO, listed_points, parity_case
    dev, st = _dev(), _stream()
    nd, axes, waxes, _, nodes = parity_case("2d")
    shape = tuple(a.size for a in axes)
    nsamp, ncol, nf, ld = int(np.prod(shape)), int(np.prod(nodes)), FITGRID_NF, FITGRID_LDV
    rng = np.random.default_rng(3801)
    a32 = [a.astype(np.float32) for a in axes]
    v32 = (rng.standard_normal((nf, nsamp)) * (10.0 ** np.arange(nf))[:, None]).astype(np.float32)
    x, wprod = listed_points([a.astype(np.float64) for a in a32], [w.astype(np.float32).astype(np.float64) for w in waxes])
    if weighted:
        w32 = rng.uniform(0.5, 2.0, (nf, nsamp)).astype(np.float32)
        w32[:, ::11] = 0.0          # masked samples
    else:
        wa32 = [w.astype(np.float32) for w in waxes]
        w32 = np.broadcast_to(wprod, (nf, nsamp))          # (for the oracle: the product of the axis weights)
    # below the boundary: packed fields, real64 on the widened inputs against the oracle, REAL32 = that rounded once
    a64, v64 = [a.astype(np.float64) for a in a32], v32.astype(np.float64)
    if weighted:
        c64, rc, _ = capi.fit_grid_weighted(nd, a64, v64.reshape((nf,) + shape[::-1]), w32.astype(np.float64).reshape((nf,) + shape[::-1]),
                                            LO[:nd], HI[:nd], nodes)
    else:
        c64, rc, _ = capi.fit_grid(nd, a64, v64.reshape((nf,) + shape[::-1]), LO[:nd], HI[:nd], nodes, waxes=[w.astype(np.float64) for w in wa32])
    assert rc == 0
    for k in range(nf):
        wk = np.asarray(w32[k], dtype=np.float64)
        keep = wk != 0.0
        c_ref, rc_ref, _ = port.fit(nd, x[keep], v64[k][keep], wk[keep], LO[:nd], HI[:nd], nodes, 0.0)
        assert rc_ref == 0
        err = float(np.max(np.abs(c64[k] - c_ref[:ncol])) / np.max(np.abs(c_ref[:ncol])))
        assert err < COEF_TOL, (k, err)
    want = _to_dev(c64.astype(np.float32))
    # past the boundary
    axes_d = _to_dev(np.concatenate(a32))
    vflat = torch.empty((nf - 1) * ld + nsamp, dtype=torch.float32, device=dev)
    vals = torch.as_strided(vflat, (nf, nsamp), (ld, 1))
    vals.copy_(_to_dev(v32))
    assert (nf - 1) * ld > B32
    cflat = torch.full((nf * ncol + GUARD,), SENT, dtype=torch.float32, device=dev)
    if weighted:
        wflat = torch.empty((nf - 1) * ld + nsamp, dtype=torch.float32, device=dev)
        wts = torch.as_strided(wflat, (nf, nsamp), (ld, 1))
        wts.copy_(_to_dev(np.ascontiguousarray(w32)))
        before = checksum(vals) + checksum(wts)
        rc, info = capi.fit_grid_weighted_dev(nd, shape, axes_d, vflat, wflat, LO[:nd], HI[:nd], nodes, cflat, nfields=nf, ldv=ld, ldw=ld, stream=st)
        after = lambda: checksum(vals) + checksum(wts)
    else:
        before = checksum(vals)
        rc, info = capi.fit_grid_dev(nd, shape, axes_d, vflat, LO[:nd], HI[:nd], nodes, cflat, waxes=_to_dev(np.concatenate(wa32)), nfields=nf,
                                     ldv=ld, stream=st)
        after = lambda: checksum(vals)
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(_bits(cflat[:nf * ncol].view(nf, ncol)), _bits(want))
    assert not bool(not_sentinel(cflat[nf * ncol:]))
    assert int(after()) == int(before)


# ---------------------------------------------------------------------------------------------------------------
# The ragged 1-D batch of splpak_eval_many_*, splpak_residuals_many_*, splpak_mad_many_*, splpak_fit_many_* and the clipped fits
RAGGED_SIZES = (1003, 0, 977, 1021, 0, 1009, 991, 1013, 986)          # one period: nine problems, two of them empty, 7 000 points
RAGGED_POINTS = sum(RAGGED_SIZES)
RAGGED_NODES = (16,)
TOTAL_32, TOTAL_31 = B32 + (1 << 20), B31 + (1 << 20)


def ragged_offsets(total):
    """offsets of the period's problems over and over up to `total` points (the last problem cut short)."""
    k = total // RAGGED_POINTS
    sizes = np.tile(np.array(RAGGED_SIZES, dtype=np.int64), k + 1)
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(np.searchsorted(off, total, side="left"))          # the first offset >= total
    off = off[:n + 1].copy()
    off[n] = total
    return off


def ragged_problem_at(boundary):
    """(problem of the period, first point, end) that holds point `boundary` of the period it falls into."""
    r = boundary % RAGGED_POINTS
    edges = np.concatenate([[0], np.cumsum(RAGGED_SIZES)])
    k = int(np.searchsorted(edges, r, side="right")) - 1
    return k, int(edges[k]), int(edges[k + 1])


def test_shapes_ragged_batch_crosses_both_boundaries_inside_a_problem():
    assert RAGGED_POINTS == 7000 and RAGGED_SIZES.count(0) == 2
    for b, total in ((B31, TOTAL_31), (B31, TOTAL_32), (B32, TOTAL_32)):
        k, lo, hi = ragged_problem_at(b)
        assert lo < b % RAGGED_POINTS < hi - 1 and RAGGED_SIZES[k] > 0          # strictly inside a problem's own segment
        assert b + RAGGED_POINTS < total                                         # whole periods follow the boundary
    off = ragged_offsets(10 * RAGGED_POINTS + 1500)
    assert off[-1] == 10 * RAGGED_POINTS + 1500 and np.all(np.diff(off) >= 0) and off.size == 10 * 9 + 3 + 1
    assert np.array_equal(np.diff(off)[:9], RAGGED_SIZES) and np.diff(off)[-1] == 1500 - 1003
    # bytes: queries and results (evaluation), points and values (statistics, fit), points, values and residuals / weights out
    nb = (TOTAL_32 // RAGGED_POINTS + 1) * 9
    assert 2 * 4 * (TOTAL_32 + GUARD) + 4 * nb * (16 + 64) + GIB <= MAX_BYTES
    assert 3 * 4 * (TOTAL_31 + GUARD) + 4 * nb * 16 + GIB <= MAX_BYTES


RAGGED_BYTES_32 = 2 * 4 * (TOTAL_32 + GUARD) + 4 * (TOTAL_32 // RAGGED_POINTS + 1) * 9 * (16 + 64 + 8) + GIB
CLIP_MAD_SCRATCH = 8 * TOTAL_31          # splpak_fit_many_clip_mad_* keeps a double per point of the batch in the library's scratch
RAGGED_BYTES_31 = 3 * 4 * (TOTAL_31 + GUARD) + 4 * (TOTAL_31 // RAGGED_POINTS + 1) * 9 * (16 + 8 + 8) + GIB


def _ragged_period(seed, outliers=False):
    """One period on the host, REAL32: x in [-0.02, 1.02] (a jittered lattice per problem), y smooth plus noise (outliers: 1 % of
    the points 50 noise widths off), coefficients and half-stencil "covariances" of the nine problems (random words: the
    evaluation entries contract whatever they are given)."""
    rng = np.random.default_rng(seed)
    xs = [(-0.02 + 1.04 * (np.arange(n) + rng.uniform(0.1, 0.9, n)) / max(n, 1)) for n in RAGGED_SIZES]
    x = np.concatenate(xs)
    y = np.sin(3.0 * x) + 0.25 * x ** 2 + 0.05 * rng.standard_normal(x.size)
    if outliers:
        hit = rng.choice(x.size, x.size // 100, replace=False)
        y[hit] += 2.5 * rng.choice([-1.0, 1.0], hit.size)
    coef = rng.standard_normal((len(RAGGED_SIZES), RAGGED_NODES[0]))
    cov = rng.standard_normal((len(RAGGED_SIZES), 4 * RAGGED_NODES[0]))
    return tuple(a.astype(np.float32) for a in (x, y, coef, cov))


def _ragged_device(total, xh, rows):
    """(offsets, number of problems, x tiled to `total` points (total, 1), the (9, m) host arrays of `rows` tiled to the problems)."""
    import torch
    off = ragged_offsets(total)
    nb = off.size - 1
    x = torch.empty((total, 1), dtype=torch.float32, device=_dev())
    fill_tiled(x, _to_dev(xh.reshape(-1, 1)))
    tiled = []
    for r in rows:
        t = torch.empty((nb, r.shape[1]), dtype=torch.float32, device=_dev())
        fill_tiled(t, _to_dev(r))
        tiled.append(t)
    return off, nb, x, tiled


@pytest.mark.gpu
@big_memory(RAGGED_BYTES_32)
def test_eval_many_and_var_dev_f32_2_32_queries(port):
    """1-D, 16 nodes, problems of about 1 000 queries, two empty ones in every nine, 2^32 + 2^20 queries in all: point 2^31 is
    query 668 of a problem of 1 021, point 2^32 query 295 of one of 1 013.  splpak_eval_many_dev_f32 (values and the first derivative) and
    splpak_eval_many_var_dev_f32: every result must have the bits of the one 7 000 queries before it; the first two problems
    against the oracle; the first period of the variances has the bits of the host entry on that period alone (position and batch
    do not matter; the variance itself is test_eval_many_var.py's)."""
    import torch
    st = _stream()
    xh, _, ch, vh = _ragged_period(3901)
    total = TOTAL_32
    off, nb, xq, (coef, cov) = _ragged_device(total, xh, [ch, vh])
    assert ragged_problem_at(B31) == (3, 1980, 3001) and ragged_problem_at(B32) == (7, 5001, 6014)
    before = checksum(xq) + checksum(coef) + checksum(cov)
    out = torch.empty(total + GUARD, dtype=torch.float32, device=_dev())
    lo, hi, nodes = [0.0], [1.0], list(RAGGED_NODES)
    m = len(RAGGED_SIZES)
    for pat in (None, [1]):
        out.fill_(SENT)
        assert capi.evaluate_many_dev(1, off, xq, pat, coef, lo, hi, nodes, out, stream=st) == 0
        assert not bool(tiled_mismatch(out[:total].unsqueeze(1), RAGGED_POINTS)), pat
        assert not bool(not_sentinel(out[total:])), pat
        got = out[:RAGGED_POINTS].cpu().numpy().astype(np.float64)
        for k in (0, 2):
            a, b = int(off[k]), int(off[k + 1])
            vo, _ = port.evaluate(1, xh[a:b].astype(np.float64).reshape(-1, 1), pat, ch[k].astype(np.float64), lo, hi, nodes)
            assert np.max(np.abs(got[a:b] - vo)) <= REAL32_EVAL_TOL * eval_scale(vo, ch[k], nodes, pat), (k, pat)
    out.fill_(SENT)
    assert capi.evaluate_many_var_dev(1, off, xq, None, cov, lo, hi, nodes, out, stream=st) == 0
    assert not bool(tiled_mismatch(out[:total].unsqueeze(1), RAGGED_POINTS))
    assert not bool(not_sentinel(out[total:]))
    want, rc = capi.evaluate_many_var(1, off[:m + 1], xh, None, vh, lo, hi, nodes, real32=True)
    assert rc == 0 and np.array_equal(out[:RAGGED_POINTS].cpu().numpy().view(np.int32), want.view(np.int32))
    assert int(checksum(xq) + checksum(coef) + checksum(cov)) == int(before)


def _stats_tiled(stats, nb):
    """The rows of the (nb, 4) device statistics repeat with the period's nine problems (the last, cut problem aside)."""
    whole = (nb - 1) // len(RAGGED_SIZES) * len(RAGGED_SIZES)
    return not bool(tiled_mismatch(stats[:whole], len(RAGGED_SIZES)))


@pytest.mark.gpu
@big_memory(RAGGED_BYTES_31)
def test_residuals_many_and_mad_many_dev_f32_residuals_past_2_31(port):
    """The ragged batch as points with values, 2^31 + 2^20 of them (x, y and the residuals are 8 GiB each; past 2^32 the three would
    be 48 GiB): splpak_residuals_many_dev_f32 with `resid` and statistics, then splpak_mad_many_dev_f32 on that residual array.
    Residuals and statistics repeat with the period; the first period of the residuals is y - the oracle's value, its statistics
    and medians have the bits of the host entries on that period alone."""
    import torch
    st = _stream()
    xh, yh, ch, _ = _ragged_period(3902)
    total = TOTAL_31
    off, nb, x, (coef,) = _ragged_device(total, xh, [ch])
    y = torch.empty((total, 1), dtype=torch.float32, device=_dev())
    fill_tiled(y, _to_dev(yh.reshape(-1, 1)))
    before = checksum(x) + checksum(y) + checksum(coef)
    resid = torch.full((total + GUARD,), SENT, dtype=torch.float32, device=_dev())
    stats = torch.full((nb + 1, 4), SENT, dtype=torch.float64, device=_dev())
    lo, hi, nodes, m = [0.0], [1.0], list(RAGGED_NODES), len(RAGGED_SIZES)
    assert capi.residuals_many_dev(1, off, x, y, None, coef, lo, hi, nodes, resid, stats, stream=st) == 0
    assert not bool(tiled_mismatch(resid[:total].unsqueeze(1), RAGGED_POINTS))
    assert not bool(not_sentinel(resid[total:])) and not bool(not_sentinel(stats[nb:]))
    assert _stats_tiled(stats, nb)
    r_h, s_h, rc = capi.residuals_many(1, off[:m + 1], xh, yh, None, ch, lo, hi, nodes, real32=True)
    assert rc == 0
    got = resid[:RAGGED_POINTS].cpu().numpy()
    assert np.array_equal(got.view(np.int32), r_h.view(np.int32)) and np.array_equal(stats[:m].cpu().numpy(), s_h)
    for k in (0, 2):
        a, b = int(off[k]), int(off[k + 1])
        vo, _ = port.evaluate(1, xh[a:b].astype(np.float64).reshape(-1, 1), None, ch[k].astype(np.float64), lo, hi, nodes)
        r_ref = yh[a:b].astype(np.float64) - vo
        assert np.max(np.abs(got[a:b] - r_ref)) <= REAL32_EVAL_TOL * max(np.max(np.abs(r_ref)), eval_scale(vo, ch[k], nodes, None)), k
    # the medians of the residual array the call above produced
    mstats = torch.full((nb + 1, 4), SENT, dtype=torch.float64, device=_dev())
    rsum = checksum(resid[:total])
    assert capi.mad_many_dev(off, resid, None, mstats, stream=st) == 0
    assert _stats_tiled(mstats, nb) and not bool(not_sentinel(mstats[nb:]))
    m_h, rc = capi.mad_many(off[:m + 1], got, None, real32=True)
    assert rc == 0 and np.array_equal(mstats[:m].cpu().numpy(), m_h)
    assert int(checksum(resid[:total])) == int(rsum)
    assert int(checksum(x) + checksum(y) + checksum(coef)) == int(before)


@pytest.mark.gpu
@big_memory(RAGGED_BYTES_32)
def test_residuals_many_dev_f32_statistics_alone_2_32_points():
    """The same batch with 2^32 + 2^20 points and `resid` NULL: the statistics of every problem repeat with the period, the first
    period's have the bits of the host entry on that period alone."""
    import torch
    st = _stream()
    xh, yh, ch, _ = _ragged_period(3903)
    total = TOTAL_32
    off, nb, x, (coef,) = _ragged_device(total, xh, [ch])
    y = torch.empty((total, 1), dtype=torch.float32, device=_dev())
    fill_tiled(y, _to_dev(yh.reshape(-1, 1)))
    before = checksum(x) + checksum(y) + checksum(coef)
    stats = torch.full((nb + 1, 4), SENT, dtype=torch.float64, device=_dev())
    lo, hi, nodes, m = [0.0], [1.0], list(RAGGED_NODES), len(RAGGED_SIZES)
    assert capi.residuals_many_dev(1, off, x, y, None, coef, lo, hi, nodes, None, stats, stream=st) == 0
    assert _stats_tiled(stats, nb) and not bool(not_sentinel(stats[nb:]))
    _, s_h, rc = capi.residuals_many(1, off[:m + 1], xh, yh, None, ch, lo, hi, nodes, real32=True, want_resid=False)
    assert rc == 0 and np.array_equal(stats[:m].cpu().numpy(), s_h)
    assert int(checksum(x) + checksum(y) + checksum(coef)) == int(before)


def _ragged_fit_anchor(port, xh, yh, xtrap):
    """The first period as a fit: the real64 entry on the widened points against the oracle problem by problem at COEF_TOL, rounded
    once (what the REAL32 entry promises).  -> coef (9, 16) float32, the empty problems' rows 0."""
    m, nodes = len(RAGGED_SIZES), list(RAGGED_NODES)
    off = ragged_offsets(RAGGED_POINTS)
    x64, y64 = xh.astype(np.float64).reshape(-1, 1), yh.astype(np.float64)
    c64, rc, st, _ = capi.fit_many(1, off, x64, y64, None, [0.0], [1.0], nodes, xtrap)
    assert rc == 105 and [int(s) for s in st] == [105 if n == 0 else 0 for n in RAGGED_SIZES]
    for k in range(m):
        a, b = int(off[k]), int(off[k + 1])
        if b > a:
            c_ref, rc_ref, _ = port.fit(1, x64[a:b], y64[a:b], None, [0.0], [1.0], nodes, xtrap)
            assert rc_ref == 0
            err = float(np.max(np.abs(c64[k] - c_ref[:16])) / np.max(np.abs(c_ref[:16])))
            assert err < COEF_TOL, (k, err)
    return c64.astype(np.float32)


@pytest.mark.gpu
@big_memory(RAGGED_BYTES_32)
def test_fit_many_dev_f32_2_32_points(port):
    """The ragged batch as a fit, 2^32 + 2^20 points: the coefficients of every problem must have the bits of the problem nine
    before it (the last, cut problem aside), the empty problems status 105 and untouched rows, the first nine the bits of the real64
    entry rounded once, which meets the oracle at COEF_TOL."""
    import torch
    st = _stream()
    xh, yh, _, _ = _ragged_period(3904)
    total, m, ncol = TOTAL_32, len(RAGGED_SIZES), RAGGED_NODES[0]
    want = _ragged_fit_anchor(port, xh, yh, 1.0)
    off, nb, x, _ = _ragged_device(total, xh, [])
    y = torch.empty((total, 1), dtype=torch.float32, device=_dev())
    fill_tiled(y, _to_dev(yh.reshape(-1, 1)))
    before = checksum(x) + checksum(y)
    flat = torch.full((nb * ncol + GUARD,), SENT, dtype=torch.float32, device=_dev())
    rc, status, info = capi.fit_many_dev(1, off, x, y, None, [0.0], [1.0], list(RAGGED_NODES), flat, xtrap=1.0, stream=st)
    torch.cuda.synchronize()
    whole = (nb - 1) // m * m
    assert rc == 105 and np.array_equal(status[:whole].reshape(-1, m), np.broadcast_to([105 if n == 0 else 0 for n in RAGGED_SIZES], (whole // m, m)))
    assert status[nb - 1] == 0
    coef = flat[:nb * ncol].view(nb, ncol)
    assert not bool(tiled_mismatch(coef[:whole], m))
    first = coef[:m].cpu().numpy()
    live = [k for k, n in enumerate(RAGGED_SIZES) if n > 0]
    assert np.array_equal(first[live].view(np.int32), want[live].view(np.int32))
    assert all(np.all(first[k] == np.float32(SENT)) for k in range(m) if k not in live)          # status 105 keeps its row
    assert not bool(not_sentinel(flat[nb * ncol:]))
    assert _host_rows_tiled(info[:whole][:, [0, 1, 2, 3, 4, 8]], m)
    assert int(checksum(x) + checksum(y)) == int(before)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["clip", "clip_mad"])
@big_memory(lambda entry: RAGGED_BYTES_31 + (CLIP_MAD_SCRATCH if entry == "clip_mad" else 0))
def test_fit_many_clip_dev_f32_points_past_2_31(entry):
    """The ragged batch with 1 % outliers, 2^31 + 2^20 points (x, y and wout are 8 GiB each; past 2^32 the three would be 48 GiB),
    through splpak_fit_many_clip_dev_f32 and splpak_fit_many_clip_mad_dev_f32: coefficients, clip counters and `wout` -- checked like
    an output, with its guard -- repeat with the period up to the last whole period; the first period, and the problems behind
    the last whole one (the very last is cut short, a problem of its own), have the bits of the host entry on those problems
    alone (which test_fit_many_clip.py and test_fit_many_clip_mad.py hold to the reference loop).  The robust entry keeps a
    double per point of the batch in the library's scratch: 16 GiB more, 40 GiB in all."""
    import torch
    st = _stream()
    xh, yh, _, _ = _ragged_period(3905, outliers=True)
    total, m, ncol = TOTAL_31, len(RAGGED_SIZES), RAGGED_NODES[0]
    off, nb, x, _ = _ragged_device(total, xh, [])
    y = torch.empty((total, 1), dtype=torch.float32, device=_dev())
    fill_tiled(y, _to_dev(yh.reshape(-1, 1)))
    before = checksum(x) + checksum(y)
    flat = torch.full((nb * ncol + GUARD,), SENT, dtype=torch.float32, device=_dev())
    wout = torch.full((total + GUARD,), SENT, dtype=torch.float32, device=_dev())
    fn_d, fn_h = (capi.fit_many_clip_dev, capi.fit_many_clip) if entry == "clip" else (capi.fit_many_clip_mad_dev, capi.fit_many_clip_mad)
    rc, status, info, clip = fn_d(1, off, x, y, None, [0.0], [1.0], list(RAGGED_NODES), flat, wout, xtrap=1.0, stream=st)
    torch.cuda.synchronize()
    whole = (nb - 1) // m * m
    assert rc == 105
    done = int(off[whole])          # the points of the whole periods
    assert done % RAGGED_POINTS == 0 and B31 + RAGGED_POINTS < done
    assert not bool(tiled_mismatch(wout[:done].unsqueeze(1), RAGGED_POINTS))
    assert not bool(not_sentinel(wout[total:])) and not bool(not_sentinel(flat[nb * ncol:]))
    coef = flat[:nb * ncol].view(nb, ncol)
    assert not bool(tiled_mismatch(coef[:whole], m))
    assert _host_rows_tiled(clip[:whole], m) and _host_rows_tiled(status[:whole].reshape(-1, 1), m)
    c_h, w_h, rc_h, st_h, _, clip_h = fn_h(1, off[:m + 1], xh, yh, None, [0.0], [1.0], list(RAGGED_NODES), 1.0, real32=True)
    assert rc_h == 105 and np.array_equal(st_h, status[:m]) and np.array_equal(clip_h, clip[:m])
    assert clip_h[:, 1].sum() > 0          # outliers were rejected
    live = [k for k, n in enumerate(RAGGED_SIZES) if n > 0]
    assert np.array_equal(coef[:m].cpu().numpy()[live].view(np.int32), np.ascontiguousarray(c_h[live]).view(np.int32))
    assert np.array_equal(wout[:RAGGED_POINTS].cpu().numpy().view(np.int32), w_h[:RAGGED_POINTS].view(np.int32))
    # the problems behind the last whole period, the cut one at the end: the host entry on them alone
    toff = off[whole:] - off[whole]
    nt = int(toff[-1])
    c_t, w_t, _, st_t, _, clip_t = fn_h(1, toff, xh[:nt], yh[:nt], None, [0.0], [1.0], list(RAGGED_NODES), 1.0, real32=True)
    assert np.array_equal(st_t, status[whole:]) and np.array_equal(clip_t, clip[whole:])
    ran = [k for k in range(nb - whole) if toff[k + 1] > toff[k]]
    assert np.array_equal(coef[whole:].cpu().numpy()[ran].view(np.int32), np.ascontiguousarray(c_t[ran]).view(np.int32))
    assert np.array_equal(wout[done:total].cpu().numpy().view(np.int32), w_t[:nt].view(np.int32))
    assert int(checksum(x) + checksum(y)) == int(before)


# ---------------------------------------------------------------------------------------------------------------
# splpak_plan_fit_dev, splpak_plan_refit_dev
PLAN_NPTS, PLAN_L1 = (1 << 25) + PERIOD, 128
PLAN_GRIDS = {"3d16": (16, 16, 16), "route1": (4098,), "route2": (90, 80)}          # nested dissection; tests/test_binning.py
# (Route 3 of the binning starts at 1 048 321 cells, so a grid that takes it has a factorisation of a million columns: too slow
#  for a test that every run of the suite repeats.  Its strided read of the points is therefore not run past 2^31 here.)
PLAN_BYTES = 8 * PLAN_NPTS * (PLAN_L1 + 3 + 1) + 12 * GIB          # the points 128 apart, their compact copy, the values; the plan
REFIT_LD, REFIT_NF = (1 << 30) + 3, 3
REFIT_BYTES = 8 * ((REFIT_NF - 1) * REFIT_LD + (1 << 17) + GUARD) + 2 * GIB          # (room for the points of 3d16 behind the last field)
INFO_EQUAL = [0, 1, 2, 3, 4, 8, 9]


def test_shapes_plan_points_and_refit_fields():
    assert PLAN_NPTS * PLAN_L1 == 4_295_491_968 > B32 and PLAN_NPTS < B31 - 1025          # max_ndata stays legal
    assert crossing(B31, PLAN_L1, 1)[:2] == (1 << 24, 0) and crossing(B32, PLAN_L1, 1)[:2] == (1 << 25, 0)
    assert PLAN_BYTES <= 48 * GIB          # 32 GiB of points + the plan
    first = [k * REFIT_LD for k in range(REFIT_NF)]
    assert first[1] + 20_000 < B31 < first[2] and first[2] + 20_000 < B32          # field 2 lies past 2^31; 2^32 would take 32 GiB more
    assert REFIT_BYTES <= MAX_BYTES


@pytest.mark.gpu
@pytest.mark.parametrize("grid", list(PLAN_GRIDS))
@big_memory(PLAN_BYTES)
def test_plan_fit_dev_points_128_words_apart_past_2_32(grid):
    """2^25 + 4 099 points with l1xdat = 128: 4 295 491 968 real64 words, the points from 2^24 on past 2^31, the last 4 099 past
    2^32 (32 GiB and the plan, the one case above 40 GiB).  16^3 nodes (nested dissection) and the grids
    test_binning.py names for the binning routes 1 and 2 (route 3 needs a grid of a million cells: see PLAN_GRIDS).  Coefficients and info [0..4], [8], [9] must be bit for bit those of a
    fresh plan fed the compact copy of the same points in the same order."""
    import torch
    dev, st = _dev(), _stream()
    nodes = PLAN_GRIDS[grid]
    nd, n, l1 = len(nodes), PLAN_NPTS, PLAN_L1
    ncol = int(np.prod(nodes))
    gen = torch.Generator(device=dev)
    gen.manual_seed(4001)
    xc = torch.rand((n, nd), dtype=torch.float64, device=dev, generator=gen)
    y = torch.sin(3.0 * xc[:, 0]) + 0.5 * torch.cos(2.0 * xc[:, -1]) + 0.05 * torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
    x = torch.empty((n, l1), dtype=torch.float64, device=dev)
    x[:, :nd].copy_(xc)
    assert x.numel() > B32 and x.stride() == (l1, 1)
    before = checksum(x[:, :nd]) + checksum(y)
    got = {}
    for which, pts in (("strided", x), ("compact", xc)):
        plan = capi.Plan(nd, list(nodes), [0.0] * nd, [1.0] * nd, 1.0, n)
        try:
            c = torch.full((ncol + GUARD,), SENT, dtype=torch.float64, device=dev)
            rc, info = plan.fit(pts, y, None, c, st)
            torch.cuda.synchronize()
            assert rc == 0, (which, rc)
            assert not bool(not_sentinel(c[ncol:]))
            got[which] = (c[:ncol].clone(), info.copy())
        finally:
            plan.close()
    assert torch.equal(_bits(got["strided"][0]), _bits(got["compact"][0]))
    assert np.array_equal(got["strided"][1][INFO_EQUAL], got["compact"][1][INFO_EQUAL])
    assert got["compact"][1][0] == n
    assert int(checksum(x[:, :nd]) + checksum(y)) == int(before)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["ldy", "ldcoef"])
@big_memory(REFIT_BYTES)
def test_plan_refit_dev_fields_2_30_words_apart(which):
    """Three fields on the points of 3d16 (nested dissection) with ldy = 2^30 + 3, then with ldcoef = 2^30 + 3: field 2 lies past
    2^31 (16 GiB of real64; past 2^32 would take five fields and 32 GiB, so 2^31 alone).  refit_batch 1 and 8.  Coefficients and
    info [0..4], [8], [9] must have the bits of the refit with packed fields, whose first two fields meet the recorded reference
    and the oracle's recorded coefficients at COEF_TOL as in test_refit.py."""
    import torch
    from tests.cases import CASES, make_inputs
    from tests.conftest import load_golden, relmax
    from tests.test_refit import Session, oracle_second_field, second_field
    inp = make_inputs(CASES["3d16"])
    s = Session(inp)
    try:
        assert s.plan.factorisation()[0] == 4
        _, rc, info = s.fit(second_field(inp))
        assert rc == 0 and info[4] != 0.0
        n, ncol, nf, ld = s.ndata, s.ncol, REFIT_NF, REFIT_LD
        F = np.stack([inp["ydata"], second_field(inp), np.cos(5.0 * inp["xdata"].sum(axis=1))])
        Yc = s.t(F)
        want = torch.full((nf, ncol), SENT, dtype=torch.float64, device=s.dev)
        s.plan.set_option("refit_batch", "1")
        rc, info0 = s.plan.refit(Yc, want, s.st)
        assert rc == 0
        wh = want.cpu().numpy()
        assert relmax(wh[0], load_golden("3d16")["coef"]) < COEF_TOL and relmax(wh[1], oracle_second_field("3d16")) < COEF_TOL
        if which == "ldy":
            yflat = torch.empty((nf - 1) * ld + n, dtype=torch.float64, device=s.dev)
            Y = torch.as_strided(yflat, (nf, n), (ld, 1))
            Y.copy_(Yc)
            cflat = torch.empty(nf * ncol + GUARD, dtype=torch.float64, device=s.dev)
            C = cflat[:nf * ncol].view(nf, ncol)
        else:
            Y = Yc
            cflat = torch.empty((nf - 1) * ld + ncol + GUARD, dtype=torch.float64, device=s.dev)
            C = torch.as_strided(cflat, (nf, ncol), (ld, 1))
        assert (nf - 1) * ld > B31
        before = checksum(Y)
        for batch in (1, 8):
            cflat.fill_(SENT)
            s.plan.set_option("refit_batch", str(batch))
            rc, info = s.plan.refit(Y, C, s.st)
            torch.cuda.synchronize()
            assert rc == 0 and s.plan.refit_stats()[0] == (1 if batch == 1 else 2)
            same = torch.equal(_bits(C), _bits(want))
            C.fill_(SENT)
            assert same, batch
            assert not bool(not_sentinel(cflat)), batch
            assert np.array_equal(info[:, INFO_EQUAL], info0[:, INFO_EQUAL]), batch
        assert int(checksum(Y)) == int(before)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------
# splpak_fit_grid_dev_f32: the sample count itself
SAMPLES_NPTS, SAMPLES_NODES, SAMPLES_P = (65_537, 32_771), (40, 9), 29
SAMPLES_BYTES = 4 * SAMPLES_NPTS[0] * SAMPLES_NPTS[1] + 9 * GIB          # the samples; the residual scratch of the refinement (8 GB cap)
EPS32_HALF = 2.0 ** -24          # one rounding to REAL32


def test_shapes_fit_grid_sample_count_crosses_2_31_inside_a_period():
    n1, n2 = SAMPLES_NPTS
    assert n1 * n2 == 2_147_713_027 > B31
    row, col = divmod(B31, n1)
    assert 0 < col < n1 and row % SAMPLES_P != 0 and row + 3 < n2          # inside a row, inside a period; rows follow (the shape ends 3.5 rows on)
    assert n2 % SAMPLES_P == 1 and n2 // SAMPLES_P == 1130          # coordinate 0 of the period occurs 1 131 times, the others 1 130
    assert SAMPLES_BYTES <= MAX_BYTES


def separable_reference(port, a1, a2, w2, nodes, v):
    """The least-squares coefficients of samples v (n2, n1) on the product of the axes a1 x a2, rows weighted by w2, in real64
    by two QR-based least-squares solves (the pseudo-inverse of a Kronecker product is the product of the pseudo-inverses); the
    basis values are the oracle's own evaluation of unit coefficient vectors.  -> coef (nodes[0] * nodes[1]), dimension 1 fastest."""
    def basis(x, nod):
        eye = np.eye(nod)
        return np.stack([port.evaluate(1, x.reshape(-1, 1), None, eye[k], [0.0], [1.0], [nod])[0] for k in range(nod)], axis=1)
    A1, A2 = basis(a1, nodes[0]), basis(a2, nodes[1])
    G = np.linalg.lstsq(A1, v.T, rcond=None)[0]                               # (nodes[0], n2)
    C = np.linalg.lstsq(w2[:, None] * A2, w2[:, None] * G.T, rcond=None)[0]   # (nodes[1], nodes[0])
    return C.ravel()


def _samples_period(seed, n1):
    """One period of the sample-count case, REAL32: ascending coordinates of dimension 1, 29 shuffled ones of dimension 2 (more
    than three in every cell of its 9 nodes), values of order 1."""
    rng = np.random.default_rng(seed)
    a1 = ((np.arange(n1) + rng.uniform(0.1, 0.9, n1)) / n1).astype(np.float32)
    a2 = ((np.arange(SAMPLES_P) + rng.uniform(0.1, 0.9, SAMPLES_P)) / SAMPLES_P).astype(np.float32)
    rng.shuffle(a2)
    g2, g1 = np.meshgrid(a2.astype(np.float64), a1.astype(np.float64), indexing="ij")
    v = (np.sin(3.0 * g1) + 0.5 * np.cos(2.0 * g2) + 0.05 * rng.standard_normal(g1.shape)).astype(np.float32)
    return a1, a2, v


def test_separable_reference_is_the_oracles_fit(port):
    """The yardstick of the sample-count case on a shape the oracle's dense fit takes: the same coefficients at COEF_TOL."""
    a1, a2, v = _samples_period(4101, 300)
    a1, a2, v = a1.astype(np.float64), a2.astype(np.float64), v.astype(np.float64)
    w2 = np.sqrt(np.r_[3.0, np.full(SAMPLES_P - 1, 2.0)])
    g2, g1 = np.meshgrid(a2, a1, indexing="ij")
    w = np.broadcast_to(w2[:, None], g1.shape)
    c_ref, rc, _ = port.fit(2, np.stack([g1.ravel(), g2.ravel()], axis=1), v.ravel(), w.ravel(), [0.0, 0.0], [1.0, 1.0], list(SAMPLES_NODES), 0.0)
    c = separable_reference(port, a1, a2, w2, SAMPLES_NODES, v)
    assert rc == 0 and np.max(np.abs(c - c_ref[:c.size])) / np.max(np.abs(c_ref[:c.size])) < COEF_TOL


@pytest.mark.gpu
@big_memory(SAMPLES_BYTES)
def test_fit_grid_dev_f32_more_than_2_31_samples(port):
    """npts (65 537, 32 771) = 2 147 713 027 REAL32 samples on nodes (40, 9): the sample count itself passes 2^31 (8 GiB; past 2^32
    would be the same test twice as large), inside row 32 767 of the values.  Dimension 2 repeats with a period of 29 coordinates,
    values included, so the fit is the fit of one period whose coordinates of dimension 2 are weighted by the root of how often
    they occur (1 131 times the first, 1 130 the others).  That fit, by the real64 host entry on the widened period, meets the
    separable least-squares reference at COEF_TOL; the REAL32 coefficients of the full call are that solution rounded once, so
    they differ from it by at most half a REAL32 unit in the last place plus COEF_TOL of the largest coefficient."""
    import time
    import torch
    dev, st = _dev(), _stream()
    (n1, n2), nodes, P = SAMPLES_NPTS, SAMPLES_NODES, SAMPLES_P
    ncol = int(np.prod(nodes))
    a1, a2, vp = _samples_period(4102, n1)
    count = np.array([len(range(j, n2, P)) for j in range(P)], dtype=np.float64)
    w2 = np.sqrt(count)
    a1w, a2w, vw = a1.astype(np.float64), a2.astype(np.float64), vp.astype(np.float64)
    c_ref = separable_reference(port, a1w, a2w, w2, nodes, vw)
    c_per, rc, _ = capi.fit_grid(2, [a1w, a2w], vw, [0.0, 0.0], [1.0, 1.0], list(nodes), waxes=[np.ones(n1), w2])
    cmax = float(np.max(np.abs(c_ref)))
    assert rc == 0 and np.max(np.abs(c_per - c_ref)) / cmax < COEF_TOL
    axes = _to_dev(np.concatenate([a1, np.tile(a2, -(-n2 // P))[:n2]]))
    vals = torch.empty((n2, n1), dtype=torch.float32, device=dev)
    fill_tiled(vals, _to_dev(vp))
    assert vals.numel() > B31
    before = checksum(vals) + checksum(axes)
    cflat = torch.full((ncol + GUARD,), SENT, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc, info = capi.fit_grid_dev(2, [n1, n2], axes, vals, [0.0, 0.0], [1.0, 1.0], list(nodes), cflat, stream=st)
    torch.cuda.synchronize()
    print(f"fit_grid_dev_f32 on {n1 * n2} samples: {time.perf_counter() - t0:.2f} s, refinement steps {info[0, 2]:.0f}")
    assert rc == 0 and info[0, 0] == n1 * n2
    got = cflat[:ncol].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - c_per) <= EPS32_HALF * np.abs(c_per) + COEF_TOL * cmax), float(np.max(np.abs(got - c_per)) / cmax)
    assert not bool(not_sentinel(cflat[ncol:]))
    assert int(checksum(vals) + checksum(axes)) == int(before)


# ---------------------------------------------------------------------------------------------------------------
def test_shapes_bytes_every_test_holds():
    """What each GPU test of this file asks big_memory for: at most 40 GiB, with the two exceptions named here."""
    held = {"eval_dev": EVAL_BYTES, "eval_derivs": DERIVS_BYTES, "eval_fields": FIELDS_BYTES, "eval_grid_derivs": GDERIVS_BYTES,
            "fit_many rows": MANY_BYTES, "fit_many 2-D": MANY2_BYTES, "fit_grid": FITGRID_BYTES[False], "fit_grid_weighted": FITGRID_BYTES[True],
            "ragged 2^32": RAGGED_BYTES_32, "ragged 2^31": RAGGED_BYTES_31, "fit_grid samples": SAMPLES_BYTES, "plan_refit": REFIT_BYTES}
    held.update({"eval_grid " + k: grid_bytes(c) for k, c in GRID_CASES.items()})
    for what, nbytes in held.items():
        assert 8 * GIB <= nbytes <= MAX_BYTES, (what, nbytes)
    # the robust clipped fit: x, y and wout are 12 bytes a point, the library's residual scratch 8 more -- 20 bytes a point is
    # 40 GiB at 2^31 points already, so this case cannot cross 2^31 below 40 GiB; the test's own tensors stay within it
    assert MAX_BYTES < RAGGED_BYTES_31 + CLIP_MAD_SCRATCH <= 42 * GIB
    # the plan's fit: 32 GiB of points 128 words apart, their packed copy, the values and the plan
    assert MAX_BYTES < PLAN_BYTES <= 48 * GIB
