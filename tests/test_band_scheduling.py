"""The band factorisations under every schedule they have: equal bits between the schedules of one form, idle and under load.

csrc/bandchol.hip runs one arithmetic under several schedules -- the four-stream look-ahead pipeline (band_cholesky: chain, column,
bulk and CU-masked stream, per-step events, item queues, potrf on a reserved CU), the narrow two-stream form (band_cholesky_narrow)
and, in csrc/twoend.hip, two narrow chains on two streams that meet in a separator and fork / join three times.  A missing or
misplaced hipStreamWaitEvent lets a trailing update read a block whose panel solve has not landed, only when the timing falls that
way; the slightly wrong factor then costs the fit a refinement step and nothing else.  This file takes the refinement away and
compares BITS: between the schedules of one form (part A), of every schedule against itself beside a bandwidth load and a
matrix-core load (part B), and of the band distributed over virtual GPUs run to run (part C).

Forms (FORMS; the environment holds at plan creation, the plan must report the code, its description is printed):

  family    label                          beyond SPLPAK_SOLVER=direct SPLPAK_ND=0                                             code
  pipeline  pipeline_unpinned              SPLPAK_NO_TWOEND=1 SPLPAK_NARROW_BW=1 SPLPAK_PIN_BW=1000000                          0
  pipeline  pipeline_pinned                SPLPAK_NO_TWOEND=1 SPLPAK_NARROW_BW=1 SPLPAK_PIN_BW=1                                0
  pipeline  pipeline_no_panel_cu           pipeline_unpinned + SPLPAK_NO_PANEL_CU=1                                             0
  pipeline  pipeline_serial                pipeline_unpinned + SPLPAK_NO_LOOKAHEAD=1                                            0
  pipeline  pipeline_pinned_no_panel_cu    pipeline_pinned + SPLPAK_NO_PANEL_CU=1                                               0
  narrow    narrow                         SPLPAK_NO_TWOEND=1                                                                   1
  narrow    narrow_serial                  SPLPAK_NO_TWOEND=1 SPLPAK_NO_LOOKAHEAD=1                                             1
  twoend    twoend                         (nothing more)                                                                       2
  twoend    twoend_serial                  SPLPAK_NO_LOOKAHEAD=1 (each chain on one stream; the two chains still on two)        2

Read from band_cholesky: the CU-masked stream and with it the item queues exist only where the band reaches SPLPAK_PIN_BW, so under
the unpinned environment SPLPAK_NO_PANEL_CU is never consulted and pipeline_no_panel_cu is the schedule of pipeline_unpinned.
pipeline_pinned_no_panel_cu is added for what the switch does change: the pin threshold reached, potrf on the chain's own stream,
no reserved CU, no item queues.  pipeline_pinned alone runs with item queues and the margin of spare waves.

Block geometry (NBLK = 256; the plan orders the dimensions by ascending node count, half bandwidth = 3 x the sum of the column
strides; nblk = block columns = steps, bw = block half-bandwidth, two-ended split top m + separator w + bottom nb).  The description
string of a plan names no block counts, so test_block_geometry restates band_bytes / te_split, holds the figures below and confirms
bw from the plans themselves: under SPLPAK_NARROW_BW=v a plan reports the pipeline (0) exactly when bw >= v.

  grid            columns  nblk  bw  two-ended m + w + nb   forms
  [2000]            2 000     8   1   4 + 1 + 3             all; b.bw <= 1: the block-tridiagonal branch of the narrow form
  [64, 64]          4 096    16   1   8 + 1 + 7             all; the same branch, no padding
  [9, 17, 13]       1 989     8   2   3 + 2 + 3             all; partial last block (197 columns of 256)
  [24, 40, 24]     23 040    90   8  41 + 8 + 41            all; NOT 12 blocks wide: the plan puts the 40 last (strides 1, 24, 576)
  [5, 9, 6]           270     2   1   -                     3d_aniso: pipeline and narrow only (two blocks cannot be split in three)
  [12, 12, 12]      1 728     7   2   3 + 2 + 2             3d12: all
  dense 3300/513    3 300    13   3   5 + 3 + 5             two-ended through splpak_debug_spd_band_solve_f64, SPLPAK_DEBUG_TWOEND=1

At bw = 8 a trailing window of [24, 40, 24] is 32 x 32 tiles of 64: the bulk launch spans seven block columns, topB and colU are
launches of their own, the pinned form draws its items from queues over 89 steps.

Part A (idle device, no refinement): synthetic_spd of every grid, two right-hand sides as tests/test_nd_solve_columns.py builds
them, plan.debug_solve.  Every form within SPD_FWD_TOL of the known solution for both; the first right-hand side solved again
after the second returns its bits; within a family np.array_equal solutions and equal minpiv.  Pipeline, narrow and two-ended are
different launch splits and are not compared with each other.  The same between the forms of a family on the fit's own normal
equations (unrefined fits of 3d_aniso, 3d12 and 24 x 40 x 24 with 200 000 points; the first form's solve is held to BWD_TOL).

EXCEPTIONS is empty: no pair of one family differed in any run.

Part B (tests/test_nd_operand_queue.py's method and constants): per form and grid of LOAD_GRIDS one plan without refinement, points
resident.  Reference = two identical fits on the idle device; ten idle fits are timed (wall clock around the stream's synchronise);
then ten fits beside (a) 1 GiB device-to-device copies on a side stream and ten beside (a) and (b) 4096 x 4096 f64 matrix products
on a second side stream, a piece of LOAD_FACTOR x the idle fit in front of each fit.  All twenty: ierr 0, the reference's bits and
its info[4].  A loaded fit is DISTURBED when it took longer than the slowest of the ten idle ones; at least NEED = 8 of the 10 of
each series must be, or the test fails ("the load did not reach the fits").  (info[4] is the smallest pivot over the padding's
unit diagonal too: on 9 x 17 x 13 and 3d12 it is 1 where the real pivots are larger.)

Streams share hardware queues (four per process by default), and which of them do is settled by the order in which the process
created them.  Two things were measured while this file was written and shaped the loop:
  - a synchronise of the fit's stream BEHIND the piece of load waits for the whole piece where that stream shares a queue with the
    copies: the fit then ran on an idle device at its idle time, and the undisturbed series failed the test as it should.  The
    coefficients are therefore cleared and the stream synchronised in FRONT of the piece;
  - with ONE side stream per kind of load the whole file saw, per test, one of two cases for all ten fits: the load beside the fit
    (9 x 17 x 13 narrow: 3.8 ms against 2.3 ms idle, the copies running on for 55 ms after the last fit), or the fit's first launch
    behind the whole piece (the same test in another process: 11.6 ms = idle + 22 copies, nothing left at the end) -- a fit that is
    late as a whole, not one whose streams are shifted against each other.  So the pieces take NRING = 4 side streams in turn, the
    copies of fit i on stream i mod 4, its products on stream (i + 2) mod 4: within one series the piece falls onto the queue of
    one of the plan's streams after the other, and that stream alone stalls behind it while the others run on -- the shift between
    panel, column, bulk and caller's stream that a missing wait needs.  The loaded times of one series now spread by a factor 3 to 5
    (TIMINGS), every one of them above the slowest idle fit.
No form on any of the three grids needed a larger piece than LOAD_FACTOR x its idle fit.

Part C: splpak_fit_multi_f64 on 2 and 3 virtual GPUs (code 3, csrc/dist.hip), 3d12.  That entry has no switch for the refinement,
so REFINED coefficients are compared run to run: the weaker form of the check -- a factor that differs between two runs can be
refined to the same coefficients.  Two idle fits equal, ten beside load (a) equal to them, all within 1e-10 of the golden.

TIMINGS of one run on an MI355X (57 tests in 44 s, the longest 4.0 s).  One copy of 1 GiB 0.42 ms, one 4096^3 f64 product 2.1 ms on
the idle device.  Columns: idle fits min .. max [ms]; copies and products in front of each loaded fit (the products are bounded
by NMM_MAX: 40 per fit); the ten fits beside the copies min .. max [ms]; the ten beside copies and products.  Every loaded fit of
every series was slower than the slowest idle fit of its plan, and had its bits.

  2d64         pipeline_unpinned              3.58 .. 3.60     35   8   5.3 .. 10.9      9.4 .. 34.5
  2d64         pipeline_pinned                4.35 .. 4.44     43   9   6.0 .. 32.6      23.2 .. 47.8
  2d64         pipeline_no_panel_cu           3.60 .. 3.64     35   8   5.1 .. 24.3      20.5 .. 38.9
  2d64         pipeline_serial                3.57 .. 3.59     35   8   5.1 .. 25.8      20.3 .. 39.0
  2d64         pipeline_pinned_no_panel_cu    3.61 .. 3.69     35   8   5.1 .. 25.8      20.6 .. 36.6
  2d64         narrow                         3.38 .. 3.42     33   7   4.9 .. 29.9      17.0 .. 41.3
  2d64         narrow_serial                  3.30 .. 3.31     32   7   4.9 .. 21.9      18.2 .. 34.8
  2d64         twoend                         2.38 .. 3.06     25   5   3.7 .. 18.5      13.4 .. 28.0
  2d64         twoend_serial                  3.06 .. 3.73     34   7   4.5 .. 30.8      19.9 .. 42.4
  3d_9_17_13   pipeline_unpinned              2.39 .. 2.47     24   5   3.9 .. 17.5      13.2 .. 26.4
  3d_9_17_13   pipeline_pinned                2.75 .. 3.06     30   7   4.4 .. 22.4      17.5 .. 34.7
  3d_9_17_13   pipeline_no_panel_cu           2.38 .. 2.45     24   5   4.0 .. 17.4      13.4 .. 26.1
  3d_9_17_13   pipeline_serial                2.83 .. 2.87     28   6   4.6 .. 20.3      15.7 .. 30.3
  3d_9_17_13   pipeline_pinned_no_panel_cu    2.36 .. 2.47     24   5   4.0 .. 21.4      13.3 .. 31.3
  3d_9_17_13   narrow                         2.25 .. 2.29     22   5   3.9 .. 14.8      13.3 .. 24.1
  3d_9_17_13   narrow_serial                  2.58 .. 2.61     25   6   4.3 .. 18.0      16.0 .. 28.3
  3d_9_17_13   twoend                         2.32 .. 2.79     24   5   3.8 .. 21.3      14.7 .. 29.8
  3d_9_17_13   twoend_serial                  2.50 .. 3.12     26   6   4.0 .. 19.4      15.9 .. 29.5
  3d_24_40_24  pipeline_unpinned             21.23 .. 21.52   206  40   29.9 .. 157.2    105.9 .. 223.9
  3d_24_40_24  pipeline_pinned               31.98 .. 33.04   315  40   39.6 .. 243.6    115.5 .. 310.5
  3d_24_40_24  pipeline_no_panel_cu          21.21 .. 21.43   205  40   29.5 .. 156.9    107.9 .. 222.1
  3d_24_40_24  pipeline_serial               32.10 .. 32.20   310  40   45.7 .. 285.7    122.7 .. 345.6
  3d_24_40_24  pipeline_pinned_no_panel_cu   21.21 .. 21.54   206  40   29.3 .. 157.8    106.3 .. 224.0
  3d_24_40_24  narrow                        23.07 .. 23.32   224  40   32.1 .. 203.1    103.5 .. 304.4
  3d_24_40_24  narrow_serial                 25.26 .. 25.33   244  40   38.8 .. 91.9     89.8 .. 219.3
  3d_24_40_24  twoend                        14.91 .. 16.75   146  30   22.6 .. 111.1    80.1 .. 161.9
  3d_24_40_24  twoend_serial                 22.34 .. 26.41   241  40   31.1 .. 185.0    107.0 .. 253.3
  3d12 on 2 virtual GPUs: idle 16.4, 15.3 ms; beside 148 copies each 73.6 .. 75.0 ms
  3d12 on 3 virtual GPUs: idle 19.2, 18.3 ms; beside 177 copies each 90.5 .. 92.4 ms
  One series in full (9 x 17 x 13 narrow beside the copies): 5.06 8.34 14.85 3.90 8.34 9.19 11.75 3.87 8.41 9.28 ms.
"""
import math
import os
import time

import numpy as np
import pytest

from splpak_amd import capi
from tests.cases import CASES, make_inputs
from tests.conftest import load_golden, relmax
from tests.test_nd_operand_queue import LOAD_BYTES, LOAD_FACTOR, NCOPY_MAX, NFITS
from tests.test_normal_equations import BWD_TOL, SPD_FWD_TOL, _fit_ne, _plan, _seeded, stencil_matvec, stencil_norm_inf, synthetic_spd
from tests.test_stream_order import BAND, DIRECT

NBLK = 256
NEED = 8                     # loaded fits of a series of NFITS that must have taken longer than the slowest idle fit
MM_N = 4096                  # load (b): f64 products of this order (tests/test_rows3_tiles.py)
NMM_MAX = 400                # products per test at the most, as NCOPY_MAX bounds the copies
NRING = 4                    # side streams the pieces of load take in turn: as many as a process has hardware queues by default

_PIPE = dict(BAND, SPLPAK_NARROW_BW="1")
_UNPINNED = dict(_PIPE, SPLPAK_PIN_BW="1000000")
_PINNED = dict(_PIPE, SPLPAK_PIN_BW="1")
_TWOEND = dict(DIRECT, SPLPAK_ND="0")
# label -> (family, environment at plan creation, code the plan must report)
FORMS = {
    "pipeline_unpinned": ("pipeline", _UNPINNED, 0),
    "pipeline_pinned": ("pipeline", _PINNED, 0),
    "pipeline_no_panel_cu": ("pipeline", dict(_UNPINNED, SPLPAK_NO_PANEL_CU="1"), 0),
    "pipeline_serial": ("pipeline", dict(_UNPINNED, SPLPAK_NO_LOOKAHEAD="1"), 0),
    "pipeline_pinned_no_panel_cu": ("pipeline", dict(_PINNED, SPLPAK_NO_PANEL_CU="1"), 0),
    "narrow": ("narrow", dict(BAND), 1),
    "narrow_serial": ("narrow", dict(BAND, SPLPAK_NO_LOOKAHEAD="1"), 1),
    "twoend": ("twoend", dict(_TWOEND), 2),
    "twoend_serial": ("twoend", dict(_TWOEND, SPLPAK_NO_LOOKAHEAD="1"), 2),
}
FAMILIES = ["pipeline", "narrow", "twoend"]
# (family, form, form) -> reason: a pair that differs in bits BY DESIGN; each of the two is then held to the tolerance on its own
EXCEPTIONS = {}

# grid -> (columns, nblk, bw, (m, w, nb) of the two-ended split or None)
GEOMETRY = {
    (2000,): (2000, 8, 1, (4, 1, 3)),
    (64, 64): (4096, 16, 1, (8, 1, 7)),
    (9, 17, 13): (1989, 8, 2, (3, 2, 3)),
    (24, 40, 24): (23040, 90, 8, (41, 8, 41)),
    (5, 9, 6): (270, 2, 1, None),
    (12, 12, 12): (1728, 7, 2, (3, 2, 2)),
}
SOLVE_GRIDS = [[2000], [64, 64], [9, 17, 13], [24, 40, 24]]
LOAD_GRIDS = {"2d64": ([64, 64], 40000), "3d_9_17_13": ([9, 17, 13], 20000), "3d_24_40_24": ([24, 40, 24], 200000)}
OWN_CASES = ["3d_aniso", "3d12", "3d_24_40_24"]


def band_geometry(nodes):
    """(columns, nblk, bw, two-ended split) as csrc/plan.hip build_grid, csrc/bandchol.hip band_bytes and csrc/twoend.hip te_split
    compute them."""
    s = sorted(int(n) for n in nodes)
    halfbw = 3 * int(np.sum(np.cumprod([1] + s[:-1])))
    ncol = int(np.prod(s))
    nblk = (ncol + NBLK - 1) // NBLK
    bw = max(1, (halfbw + NBLK - 1) // NBLK)
    if bw > nblk - 1:
        bw = max(nblk - 1, 0)
    split = None
    if bw >= 1 and nblk - bw >= 2:
        m = (nblk - bw + 1) // 2
        nb = nblk - bw - m
        if m >= 1 and nb >= 1:
            split = (m, bw, nb)
    return ncol, nblk, bw, split


def _admits(nodes, label):
    return FORMS[label][0] != "twoend" or band_geometry(nodes)[3] is not None


def _forms_of(nodes, family):
    return [k for k, f in FORMS.items() if f[0] == family and _admits(nodes, k)]


class _Env:
    """The environment of a form for the duration of a plan's creation (or of a one-shot call)."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _checked(plan, label, nodes):
    code, text = plan.factorisation()
    if code != FORMS[label][2]:
        plan.close()
        raise AssertionError(f"{label} {list(nodes)}: factorisation {code} ({text}), wanted {FORMS[label][2]}")
    print(f"{label} {list(nodes)}: code {code}, {text}")
    return plan


def _same_within(family, what, results):
    """results: {label: (array, scalar)} of one family -> every form against the first, bit for bit unless excepted."""
    labels = list(results)
    base = labels[0]
    for other in labels[1:]:
        same = np.array_equal(results[other][0], results[base][0]) and results[other][1] == results[base][1]
        key = (family, base, other)
        if key in EXCEPTIONS:
            print(f"{what}: {base} / {other} excepted ({EXCEPTIONS[key]}); equal bits: {same}")
            continue
        diff = np.nonzero(results[other][0] != results[base][0])[0]
        assert same, (f"{what}: {other} differs from {base} in {diff.size} of {results[base][0].size} entries, first at {diff[:1]}, "
                      f"relative difference {relmax(results[other][0], results[base][0]):.2e}; min pivot {results[other][1]!r} / "
                      f"{results[base][1]!r}")


# ---------------------------------------------------------------------------------------------------------------
# geometry
@pytest.mark.gpu
@pytest.mark.parametrize("nodes", [list(g) for g in GEOMETRY], ids=lambda g: "x".join(map(str, g)))
def test_block_geometry(nodes):
    """The figures of the docstring: band_geometry gives them, and the plans confirm bw (the pipeline exactly from
    SPLPAK_NARROW_BW <= bw) and whether the two-ended form takes the grid."""
    want = GEOMETRY[tuple(nodes)]
    assert band_geometry(nodes) == want
    ncol, nblk, bw, split = want
    for limit, code in ((bw, 0), (bw + 1, 1)):
        with _Env(dict(BAND, SPLPAK_NARROW_BW=str(limit))):
            plan = _plan(nodes)
        try:
            got, text = plan.factorisation()
            assert plan.ncol == ncol and got == code, (nodes, limit, got, text)
        finally:
            plan.close()
    with _Env(_TWOEND):
        plan = _plan(nodes)
    try:
        got, text = plan.factorisation()
    finally:
        plan.close()
    print(f"{nodes}: {ncol} columns, {nblk} block columns, band {bw} blocks wide, two-ended split {split}; default band plan: {got}, {text}")
    assert got == (2 if split else 1), (nodes, got, text)


# ---------------------------------------------------------------------------------------------------------------
# part A: synthetic SPD matrices through plan.debug_solve
_synthetic = {}


def _synthetic_case(nodes):
    """(N, [known solutions], [right-hand sides]), computed once per grid and read-only."""
    key = tuple(nodes)
    if key not in _synthetic:
        N = synthetic_spd(nodes, 4000 + len(nodes) * 100 + int(np.prod(nodes)) % 97)
        rng = np.random.default_rng(17)
        xs = [rng.uniform(-1.0, 1.0, N.shape[0]), rng.standard_normal(N.shape[0]) * 1e3]
        bs = [np.asarray(stencil_matvec(N, nodes, x), dtype=np.float64) for x in xs]
        for a in [N] + xs + bs:
            a.setflags(write=False)
        _synthetic[key] = (N, xs, bs)
    return _synthetic[key]


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("nodes", SOLVE_GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_forms_of_a_family_solve_to_equal_bits(nodes, family):
    N, xs, bs = _synthetic_case(nodes)
    results = {}
    for label in _forms_of(nodes, family):
        with _Env(FORMS[label][1]):
            plan = _checked(_plan(nodes), label, nodes)
        try:
            got = [plan.debug_solve(N, bs[k]) for k in (0, 1, 0)]
        finally:
            plan.close()
        for k, (x, rc, mp) in zip((0, 1), got):
            err = float(np.max(np.abs(x - xs[k])) / np.max(np.abs(xs[k])))
            print(f"{label} {nodes} right-hand side {k}: forward error {err:.2e} (bound {SPD_FWD_TOL:.0e}), min pivot {mp:.17g}")
            assert rc == 0 and mp > 0, (label, k, rc, mp)
            assert err <= SPD_FWD_TOL, (label, k, err)
        assert got[2][1] == 0 and np.array_equal(got[2][0], got[0][0]) and got[2][2] == got[0][2], \
            f"{label} {nodes}: the first right-hand side solved again after the second differs from its first solve"
        assert got[1][2] == got[0][2], (label, "min pivot of one matrix factored twice")
        results[label] = (np.concatenate([got[0][0], got[1][0]]), got[0][2])
    assert len(results) >= 2, (nodes, family)
    _same_within(family, f"synthetic {nodes}", results)


def _dense_band(n, halfbw):
    """The matrix of tests/test_gpu_parity.py::test_two_ended_band_cholesky_vs_lapack."""
    rng = np.random.default_rng(7 * n + halfbw)
    i, j = np.indices((n, n))
    a = rng.standard_normal((n, n)) * (np.abs(i - j) <= halfbw)
    a = np.tril(a) + np.tril(a, -1).T
    a[np.diag_indices(n)] = np.abs(a).sum(axis=1) + 1.0 + rng.random(n)
    return a, [rng.standard_normal(n), rng.uniform(-1.0, 1.0, n) * 1e3]


@pytest.mark.gpu
def test_two_ended_with_a_separator_of_three_blocks():
    """n = 3300, half bandwidth 513 (13 block columns with padding, split 5 + 3 + 5) from the parametrisation of
    test_two_ended_band_cholesky_vs_lapack, through the dense entry: the two chains' Schur complements meet in three blocks.
    Held to LAPACK at that test's 1e-11; chains on two streams each and on one, bit for bit."""
    n, halfbw = 3300, 513
    nblk, bw = (n + NBLK - 1) // NBLK, (halfbw + NBLK - 1) // NBLK
    m = (nblk - bw + 1) // 2
    assert (nblk, bw, m, nblk - bw - m) == (13, 3, 5, 5)
    a, bs = _dense_band(n, halfbw)
    ref = [np.linalg.solve(a, b) for b in bs]
    results = {}
    for label, env in (("twoend", {}), ("twoend_serial", {"SPLPAK_NO_LOOKAHEAD": "1"})):
        with _Env(dict(env, SPLPAK_DEBUG_TWOEND="1")):
            got = [capi.debug_spd_band_solve(a, halfbw, bs[k]) for k in (0, 1, 0)]
        for k, (x, rc) in zip((0, 1), got):
            err = relmax(x, ref[k])
            print(f"dense {n}/{halfbw} {label} right-hand side {k}: against LAPACK {err:.2e}")
            assert rc == 0 and err < 1e-11, (label, k, rc, err)
        assert np.array_equal(got[2][0], got[0][0]), label
        results[label] = (np.concatenate([got[0][0], got[1][0]]), 0)
    _same_within("twoend", f"dense {n}/{halfbw}", results)


def _own_case(name):
    return _seeded(3, [24, 40, 24], 200000, 41) if name == "3d_24_40_24" else make_inputs(CASES[name])


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", OWN_CASES)
def test_forms_of_a_family_fit_to_equal_bits(name, family):
    """Unrefined fits: the assembly in front of the factorisation, the coefficients being the factorisation's one solve
    (test_factorisation_of_the_fits_own_normal_equations)."""
    inp = _own_case(name)
    nodes = [int(v) for v in inp["nodes"]]
    labels = _forms_of(nodes, family)
    if not labels:
        assert band_geometry(nodes)[3] is None and family == "twoend"      # 3d_aniso: two block columns
        with _Env(_TWOEND):
            plan = _plan(nodes)
        try:
            assert plan.factorisation()[0] == 1
        finally:
            plan.close()
        return
    results = {}
    for label in labels:
        with _Env(FORMS[label][1]):
            ierr, info, coef, N, rhs, code, plan = _fit_ne(inp, refine=0)
        try:
            _checked(plan, label, nodes)
        finally:
            plan.close()
        assert ierr == 0 and info[2] == 0 and info[4] > 0, (label, ierr, info)
        if not results:
            res = np.asarray(rhs.astype(np.longdouble) - stencil_matvec(N, nodes, coef), dtype=np.float64)
            bwd = float(np.max(np.abs(res)) / (stencil_norm_inf(N, nodes) * np.max(np.abs(coef)) + np.max(np.abs(rhs))))
            print(f"{name} {label}: backward error of the unrefined fit {bwd:.2e} (bound {BWD_TOL:.0e}), min pivot {info[4]:.17g}")
            assert bwd <= BWD_TOL, (name, label, bwd)
        results[label] = (coef, float(info[4]))
    assert len(results) >= 2
    _same_within(family, f"unrefined fit {name}", results)


# ---------------------------------------------------------------------------------------------------------------
# part B: every form beside a load
@pytest.fixture(scope="module")
def load():
    """The two loads: (source, destination, seconds per copy on the idle device, matrix, seconds per product)."""
    import torch
    dev = torch.device("cuda", 0)
    src = torch.zeros(LOAD_BYTES // 8, dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    mat = torch.rand(MM_N, MM_N, dtype=torch.float64, device=dev)
    out = torch.empty_like(mat)
    dst.copy_(src)
    torch.matmul(mat, mat, out=out)
    secs = []
    for work in (lambda: dst.copy_(src), lambda: torch.matmul(mat, mat, out=out)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(4):
            work()
        b.record()
        b.synchronize()
        secs.append(a.elapsed_time(b) * 1e-3 / 4)
    print(f"load: one copy of {LOAD_BYTES >> 20} MiB {secs[0] * 1e3:.2f} ms, one {MM_N}^3 f64 product {secs[1] * 1e3:.2f} ms on the idle device")
    yield src, dst, secs[0], (mat, out), secs[1]
    del src, dst, mat, out
    torch.cuda.empty_cache()


_points = {}


def _resident(grid):
    if grid not in _points:
        import torch
        nodes, m = LOAD_GRIDS[grid]
        inp = _seeded(len(nodes), nodes, m, 43)
        dev = torch.device("cuda", 0)
        _points[grid] = tuple(torch.tensor(np.ascontiguousarray(inp[k]), dtype=torch.float64, device=dev) for k in ("xdata", "ydata", "wdata"))
    return _points[grid]


def _timed_fits(plan, pts, coef, nfits, before_each=None):
    """-> [(coefficients, ierr, info[4], seconds)]: the seconds are the fit's own, from its call to the end of its stream's work.
    Nothing is enqueued on the fit's stream between the load and the fit: where that stream shares a hardware queue with a load's
    stream, a synchronise behind the load would wait for the whole piece and leave the fit on an idle device (measured so: 22
    copies in front of a 3.4 ms fit, the fit at 3.4 ms and no copy left when the series ended)."""
    import torch
    x, y, w = pts
    out = []
    for _ in range(nfits):
        coef.zero_()
        torch.cuda.current_stream().synchronize()
        if before_each is not None:
            before_each()
        t0 = time.perf_counter()
        ierr, info = plan.fit(x, y, w, coef)
        torch.cuda.current_stream().synchronize()
        dt = time.perf_counter() - t0
        out.append((coef.cpu().numpy(), ierr, float(info[4]), dt))
    return out


def _ms(v):
    return " ".join(f"{t * 1e3:.2f}" for t in v)


@pytest.mark.gpu
@pytest.mark.parametrize("label", list(FORMS))
@pytest.mark.parametrize("grid", list(LOAD_GRIDS))
def test_fits_beside_a_load_keep_their_idle_bits(load, grid, label):
    import torch
    src, dst, t_copy, (mat, out), t_mm = load
    nodes = LOAD_GRIDS[grid][0]
    assert _admits(nodes, label)
    pts = _resident(grid)
    with _Env(FORMS[label][1]):
        plan = _checked(capi.Plan(len(nodes), nodes, [0.0] * len(nodes), [1.0] * len(nodes), 1.0, pts[0].shape[0]), label, nodes)
    ring = [torch.cuda.Stream() for _ in range(NRING)]
    turn = [0]
    try:
        plan.set_refine(0, 1e-11)
        coef = torch.zeros(plan.ncol, dtype=torch.float64, device=pts[0].device)
        ierr, _ = plan.fit(*pts, coef)                      # the plan's first fit creates its streams (and reads back the reserved CU)
        assert ierr == 0
        torch.cuda.synchronize()
        ref = _timed_fits(plan, pts, coef, 2)
        assert ref[0][1] == ref[1][1] == 0 and np.array_equal(ref[0][0], ref[1][0]) and ref[0][2] == ref[1][2] > 0, \
            f"{grid} {label}: two fits on the idle device differ"
        assert np.all(np.isfinite(ref[0][0])) and np.any(ref[0][0] != 0)
        idle = _timed_fits(plan, pts, coef, NFITS)
        t_idle = [r[3] for r in idle]
        t_fit = float(np.median(t_idle))
        ncopy = min(NCOPY_MAX // NFITS, max(2, math.ceil(LOAD_FACTOR * t_fit / t_copy)))
        nmm = min(NMM_MAX // NFITS, max(2, math.ceil(LOAD_FACTOR * t_fit / t_mm)))

        def load_a():                                         # the piece of fit i on stream i mod NRING
            turn[0] += 1
            with torch.cuda.stream(ring[turn[0] % NRING]):
                for _ in range(ncopy):
                    dst.copy_(src, non_blocking=True)

        def load_ab():                                        # ... and its products two streams further on
            load_a()
            with torch.cuda.stream(ring[(turn[0] + NRING // 2) % NRING]):
                for _ in range(nmm):
                    torch.matmul(mat, mat, out=out)

        series, left = {}, {}
        try:
            for what, piece in (("copies", load_a), ("copies and products", load_ab)):
                series[what] = _timed_fits(plan, pts, coef, NFITS, before_each=piece)
                t0 = time.perf_counter()
                for s in ring:
                    s.synchronize()
                left[what] = time.perf_counter() - t0          # load still running when the last fit ended
        finally:
            for s in ring:
                s.synchronize()
    finally:
        plan.close()
    print(f"{grid} {label}: idle fits {min(t_idle) * 1e3:.2f} .. {max(t_idle) * 1e3:.2f} ms; in front of each loaded fit {ncopy} copies "
          f"({t_copy * 1e3:.2f} ms each) and {nmm} products ({t_mm * 1e3:.2f} ms each)")
    for what, runs in series.items():
        print(f"{grid} {label}: beside the {what} [ms]: {_ms([r[3] for r in runs])}; the load ran on for {left[what] * 1e3:.0f} ms")
    for what, runs in [("idle", idle)] + list(series.items()):
        bad = [i for i, r in enumerate(runs) if not (r[1] == 0 and np.array_equal(r[0], ref[0][0]) and r[2] == ref[0][2])]
        assert not bad, (f"{grid} {label}: fits {bad} of the {what} series do not have the idle fit's status, bits and smallest pivot; first: "
                         f"ierr {runs[bad[0]][1]}, min pivot {runs[bad[0]][2]!r} against {ref[0][2]!r}, relative difference "
                         f"{relmax(runs[bad[0]][0], ref[0][0]):.2e}")
    for what, runs in series.items():
        disturbed = sum(r[3] > max(t_idle) for r in runs)
        assert disturbed >= NEED, (f"{grid} {label}: the load did not reach the fits: only {disturbed} of {NFITS} fits beside the {what} "
                                   f"took longer than the slowest idle fit ({max(t_idle) * 1e3:.2f} ms)")


# ---------------------------------------------------------------------------------------------------------------
# part C: the band distributed over virtual GPUs
@pytest.mark.gpu
@pytest.mark.parametrize("ngpus,chunk", [(2, 1), (3, 2)])
def test_distributed_band_run_to_run(load, ngpus, chunk, monkeypatch):
    import torch
    src, dst, t_copy = load[:3]
    monkeypatch.setenv("SPLPAK_VIRTUAL_GPUS", "1")
    monkeypatch.setenv("SPLPAK_DIST_CHUNK", str(chunk))
    inp = make_inputs(CASES["3d12"])
    gold = load_golden("3d12")
    m = inp["xdata"].shape[0]
    mpl = capi.MultiPlan(ngpus, inp["ndim"], inp["nodes"], inp["xmin"], inp["xmax"], inp["xtrap"], (m + ngpus - 1) // ngpus, chunk=chunk)
    try:
        code, text = mpl.factorisation()
    finally:
        mpl.close()
    print(f"3d12 on {ngpus} virtual GPUs (chunk {chunk}): code {code}, {text}")
    assert code == 3, (code, text)
    args = (inp["ndim"], inp["xdata"], inp["ydata"], inp["wdata"], inp["xmin"], inp["xmax"], inp["nodes"], inp["xtrap"])

    def fit():
        t0 = time.perf_counter()
        c, ierr, _, info = capi.fit_multi(ngpus, *args)
        return c, ierr, time.perf_counter() - t0

    fit()
    torch.cuda.synchronize()
    idle = [fit() for _ in range(2)]
    assert idle[0][1] == idle[1][1] == 0 and np.array_equal(idle[0][0], idle[1][0])
    assert relmax(idle[0][0], gold["coef"]) < 1e-10
    t_fit = min(r[2] for r in idle)
    ncopy = min(NCOPY_MAX // NFITS, max(2, math.ceil(LOAD_FACTOR * t_fit / t_copy)))
    side = torch.cuda.Stream()
    loaded = []
    try:
        for _ in range(NFITS):
            with torch.cuda.stream(side):
                for _ in range(ncopy):
                    dst.copy_(src, non_blocking=True)
            loaded.append(fit())
    finally:
        side.synchronize()
    print(f"3d12 x{ngpus}: idle {_ms([r[2] for r in idle])} ms; beside {ncopy} copies each [ms]: {_ms([r[2] for r in loaded])}")
    bad = [i for i, r in enumerate(loaded) if not (r[1] == 0 and np.array_equal(r[0], idle[0][0]))]
    assert not bad, (ngpus, bad)
