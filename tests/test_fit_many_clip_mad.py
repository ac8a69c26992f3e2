"""Robustly clipped batch fits in one launch (splpak_fit_many_clip_mad_*, csrc/fitmanymad.hip): the clipping loop of
tests/test_fit_many_clip.py on a median / MAD scale, with rejected points allowed to return (regrow).

Yardstick 1 is the loop of the existing entries with the rule of include/splpak_hip.h applied in numpy between them
(`loop_yardstick`: capi.fit_many -> capi.residuals_many -> t = w0 resid -> capi.mad_many with wsel = the current weights ->
decide -> ...; a problem is frozen once it stops).  In f64 the new entry must return its bits: coef, wout, status, clip, info
slots 0-4 and 8.  In f32 residuals_many rounds resid to float, which the fused entry does not do, so the helper asserts that no
decision of any pass lies within 1e-5 relative of its threshold and the test then asks for equal masks, identical coefficient
bits and equal counts.

Yardstick 2 is the unmodified reference run through the same rule with numpy.median (Reference.fit / Reference.evaluate) by
tools/gen_fit_many_clip_mad_golden.py, recorded in tests/golden/fit_many_clip_mad_ref.npz for regrow 0 and 1: same mask, same
number of passes, same number of returned points, coefficients within BAR = 1e-10 relative max-norm.  The generator refuses a
case with a decision within 1e-6 of its threshold.

CPU tier: exports, the argument ladder (decided before any device call), and the rule restated in numpy on NumpyManyFit against
the recorded masks and coefficients.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from splpak_amd import capi
from tests.conftest import ROOT, load_golden, relmax
from tests.test_fit_many import NumpyManyFit, largest_1d_nodes
from tests.test_fit_many_clip import NOISE, RAGGED, case, make, numpy_evaluate, pack, same_bits, smooth, start_weights
from tests.test_stream_order import NO_WINDOW, T_FLOOR_MS, clock, streams  # noqa: F401  (the fixtures of the stream-order tests)

BAR = 1e-10
SYMBOLS = ("splpak_fit_many_clip_mad_f64", "splpak_fit_many_clip_mad_f32", "splpak_fit_many_clip_mad_dev_f64",
           "splpak_fit_many_clip_mad_dev_f32")
E_BADARG, E_UNSUPPORTED = -3, -4
INFO_SLOTS = [0, 1, 2, 3, 4, 8]
KLO, KHI, MAXPASS = 2.5, 3.0, 8
MAD_TO_SIGMA = 1.482602218505602
GOLDEN_NAMES = ["c16", "c16_xt0", "c80w", "c65", "c56", "c1212", "first", "negfirst", "clean", "cluster", "drag"]
DRAG_SEED, DRAG_RUN = 9501, 7


@functools.lru_cache(maxsize=None)
def mad_case(name):
    """The cases of tests/test_fit_many_clip.py and `drag`: 1-D, 16 nodes, 300 points, and 7 points that are neighbours in x, each
    raised by 1.0 -- they drag the first fit towards them, and good points beside them are rejected in pass 0.  The points are
    permuted; p["raised"] lists the seven."""
    if name != "drag":
        return case(name)
    rng = np.random.default_rng(DRAG_SEED)
    n = 300
    x = np.sort(rng.uniform(0.0, 1.0, n))
    y = smooth(x.reshape(-1, 1)) + rng.uniform(-NOISE, NOISE, n)
    at = int(rng.integers(60, 220))
    y[at:at + DRAG_RUN] += 1.0
    order = rng.permutation(n)
    raised = np.nonzero((order >= at) & (order < at + DRAG_RUN))[0]
    return dict(ndim=1, nodes=(16,), xtrap=1.0, x=x[order].reshape(-1, 1), y=y[order], w=None, raised=raised)


def mad_stats(t):
    """(med, MAD) of splpak_mad_many_* over t (all counted): numpy.median on the keys t + 0.0."""
    if t.size == 0:
        return 0.0, 0.0
    k = np.asarray(t, dtype=np.float64) + 0.0
    med = np.median(k)
    return float(med), float(np.median(np.abs(k - med)))


def decide(t, med, s, klo, khi, margin=None, what=""):
    """Step 5 on the weighted residuals t of the candidates -> out (bool).  margin: assert that no decision lies within that
    relative distance of its threshold."""
    e = t - np.float64(med)
    hi, lo = np.float64(khi) * np.float64(s), np.float64(klo) * np.float64(s)
    out = (e > hi) | (-e > lo)
    if margin is not None:
        near = np.zeros(e.size, dtype=bool)
        if np.isfinite(hi):
            near |= np.abs(e - hi) <= margin * hi
        if np.isfinite(lo):
            near |= np.abs(-e - lo) <= margin * lo
        assert not near.any(), f"{what}: a decision within {margin:g} of its threshold"
    return out


def apply_rule(t_all, w0, w, klo, khi, regrow, margin=None, what=""):
    """Steps 4 and 5 for one problem: t_all at the points with w0 != 0 (in their order), the current weights w (changed in
    place).  -> (s, med, changed, returned)."""
    cand0 = np.nonzero(w0 != 0.0)[0]
    counted = w[cand0] != 0.0
    med, mad = mad_stats(t_all[counted])
    s = MAD_TO_SIGMA * mad
    if s == 0.0:
        return s, med, 0, 0
    sel = np.ones(cand0.size, dtype=bool) if regrow else counted
    out = decide(t_all[sel], med, s, klo, khi, margin, what)
    was = w[cand0[sel]] != 0.0
    w[cand0[sel]] = np.where(out, 0.0, w0[cand0[sel]])
    now = ~out
    return s, med, int((now != was).sum()), int((now & ~was).sum())


# ---------------------------------------------------------------------------------------------------------------
# The rule restated in numpy on NumpyManyFit (CPU tier; the generator runs the same rule on the reference)
def numpy_loop(p, klo, khi, maxpass, regrow, margin=None):
    """-> (coef, wout, status, passes, returned)."""
    w0 = start_weights(p)
    w = w0.copy()
    q0 = dict(p)
    q0["w"], q0["y"] = w0, np.where(w0 != 0.0, p["y"], 0.0)
    rows = NumpyManyFit(q0)      # the rows of every point with w0 != 0: t = w0 (y - f) for any coefficients
    passes = returned = 0
    for j in range(maxpass + 1):
        q = dict(p)
        q["w"] = w
        q["y"] = np.where(w != 0.0, p["y"], 0.0)
        f = rows if j == 0 else NumpyManyFit(q)
        c, status, _ = f.fit()
        if status != 0 or j == maxpass:
            break
        t_all = numpy_evaluate(rows, c)
        passes += 1
        s, med, changed, back = apply_rule(t_all, w0, w, klo, khi, regrow, margin, f"pass {j}")
        returned += back
        if s == 0.0 or changed == 0:
            break
    return c, w, status, passes, returned


# ---------------------------------------------------------------------------------------------------------------
# CPU tier
def test_symbols_exported():
    lib = capi.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in capi.SYMBOLS


def _call(ndim=1, nbatch=1, offsets=(0, 8), x="ok", l1xdat=1, y="ok", w=None, xmin=(0.0, 0.0), xmax=(1.0, 1.0), nodes=(4, 4), ldcoef=16,
          coef="ok", wout="ok", klo=3.0, khi=3.0, maxpass=3, regrow=0):
    """splpak_fit_many_clip_mad_f64 on raw arguments -> (rc, coef, wout, status, clip); "ok": a valid array, None: a null pointer,
    wout="wdata": the very array passed as wdata."""
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    keep = []

    def arr(v, dt, ty):
        if v is None:
            return None
        a = np.ascontiguousarray(v, dtype=dt)
        keep.append(a)
        return a.ctypes.data_as(ty)
    cf = np.full(64, 777.0)
    wo = np.full(32, 555.0)
    cl = np.full(48, 333.0)
    st = np.full(8, -999, dtype=np.int32)
    xs = np.linspace(0.0, 1.0, 32)
    wd = np.ones(32) if (w == "ok" or wout == "wdata") else None
    wd_p = arr(wd, np.float64, dp)
    wo_p = wd_p if wout == "wdata" else (wo.ctypes.data_as(dp) if wout == "ok" else None)
    rc = capi.lib().splpak_fit_many_clip_mad_f64(ndim, nbatch, arr(offsets, np.int64, lp), arr(xs if x == "ok" else x, np.float64, dp), l1xdat,
                                                 arr(xs if y == "ok" else y, np.float64, dp), wd_p, arr(xmin, np.float64, dp),
                                                 arr(xmax, np.float64, dp), arr(nodes, np.int32, ip), 1.0, klo, khi, maxpass, regrow, wo_p,
                                                 arr(cf, np.float64, dp) if coef is not None else None, ldcoef, st.ctypes.data_as(ip), None,
                                                 cl.ctypes.data_as(dp))
    return rc, cf, wo, st, cl


def test_status_ladder_in_order_before_any_device_call():
    """The ladder of splpak_fit_many_clip_* in its order, every rung with every LATER rung failing too, at both values of regrow
    (and a regrow that is neither 0 nor 1: any value is valid); coef, wout, status and clip stay as they were.  No rung asks for a
    device (the test runs where there is none)."""
    big = (1000, 1000)      # 2-D, beyond the LDS rule
    bad = dict(wout=None, maxpass=-1, klo=0.5, khi=float("nan"))      # every clip condition failing
    deep = dict(ndim=2, nodes=big, ldcoef=1000000, l1xdat=2)           # passes up to the LDS rule, which it fails
    ladder = [
        (E_BADARG, dict(offsets=None, ndim=0, **bad)),
        (E_BADARG, dict(nodes=None, ndim=0, **bad)),
        (E_BADARG, dict(xmin=None, ndim=0, **bad)),
        (E_BADARG, dict(xmax=None, ndim=0, **bad)),
        (101, dict(ndim=0, nodes=(3, 3), ldcoef=0, nbatch=0, **bad)),
        (E_UNSUPPORTED, dict(ndim=3, nodes=(3, 3, 3), xmin=(0, 0, 0), xmax=(1, 1, 1), ldcoef=0, nbatch=0, **bad)),
        (102, dict(ndim=2, nodes=(3, 4), xmax=(1.0, 0.0), ldcoef=0, nbatch=0, **bad)),
        (103, dict(ndim=2, nodes=(4, 4), xmax=(1.0, 0.0), ldcoef=0, nbatch=0, **bad)),
        (104, dict(ndim=2, nodes=big, ldcoef=999999, nbatch=0, **bad)),
        (E_BADARG, dict(deep, nbatch=0)),
        (E_BADARG, dict(deep, offsets=(0, 8, 4), nbatch=2)),
        (E_BADARG, dict(deep, l1xdat=1)),
        (E_BADARG, dict(deep, x=None)),
        (E_BADARG, dict(deep, y=None)),
        (E_BADARG, dict(deep, coef=None)),
        (E_BADARG, dict(deep, wout=None)),
        (E_BADARG, dict(deep, wout="wdata")),
        (E_BADARG, dict(deep, maxpass=-1)),
        (E_BADARG, dict(deep, klo=0.999)),
        (E_BADARG, dict(deep, khi=0.0)),
        (E_BADARG, dict(deep, klo=float("nan"))),
        (E_BADARG, dict(deep, khi=float("nan"))),
        (E_BADARG, dict(deep, khi=float("-inf"))),
        (E_UNSUPPORTED, dict(deep)),
        (E_UNSUPPORTED, dict(deep, klo=1.0, khi=float("inf"), maxpass=0, w="ok")),
    ]
    for regrow in (0, 1, -7):
        for want, kw in ladder:
            rc, cf, wo, st, cl = _call(regrow=regrow, **kw)
            assert rc == want, (want, rc, kw, regrow)
            assert np.all(cf == 777.0) and np.all(wo == 555.0) and np.all(st == -999) and np.all(cl == 333.0), kw
        # the clip conditions are what refuses a call that is otherwise admitted (a batch of empty problems, answered on the host)
        assert _call(nbatch=2, offsets=(5, 5, 5), regrow=regrow)[0] == 105
        for kw in (dict(wout=None), dict(wout="wdata"), dict(maxpass=-1), dict(klo=0.5), dict(khi=float("nan"))):
            rc, cf, wo, st, cl = _call(nbatch=2, offsets=(5, 5, 5), regrow=regrow, **kw)
            assert rc == E_BADARG and np.all(st == -999) and np.all(cl == 333.0), kw
            assert "wout" in capi.last_error()
    # problems without points: 105 each, coef and wout untouched, six clip numbers zeroed per problem and no more
    rc, cf, wo, st, cl = _call(nbatch=2, offsets=(5, 5, 5), regrow=1)
    assert rc == 105 and list(st[:2]) == [105, 105] and np.all(cf == 777.0) and np.all(wo == 555.0)
    assert np.all(cl[:12] == 0.0) and np.all(cl[12:] == 333.0)
    assert capi.debug_fit_many_stats()[2:5] == (0, 0, 2) and capi.debug_fit_many_stats()[7] == 0


@pytest.mark.parametrize("regrow", [0, 1])
@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_numpy_restatement_matches_recorded_reference(name, regrow):
    """The rule without a GPU: the fit of NumpyManyFit, its rows as the residuals, numpy.median; against the reference's run."""
    gold = load_golden("fit_many_clip_mad_ref")
    p = mad_case(name)
    c, w, status, passes, returned = numpy_loop(p, KLO, KHI, MAXPASS, regrow, margin=1e-9)
    key = f"{name}_g{regrow}"
    assert status == 0
    assert np.array_equal(w == 0.0, gold["mask_" + key]), name
    assert passes == int(gold["passes_" + key]) and returned == int(gold["returned_" + key])
    err = relmax(c, gold["coef_" + key])
    print(f"{key}: numpy rule vs the reference's run {err:.2e}, {passes} passes, {returned} returned")
    assert err <= BAR
    if name == "drag" and regrow:
        assert returned >= 10


# ---------------------------------------------------------------------------------------------------------------
# GPU tier
def loop_yardstick(ndim, off, x, y, w, lo, hi, nodes, xtrap, klo, khi, maxpass, regrow, real32=False, margin=None):
    """Yardstick 1: capi.fit_many -> capi.residuals_many -> t = w0 resid -> capi.mad_many -> steps 4 and 5 in numpy -> ..., each
    round on the batch of the problems that have not stopped (the bits of a problem do not depend on its batch).
    -> (coef, wout, status, info, clip) as capi.fit_many_clip_mad returns them; coefficient rows of problems without points are 0."""
    dt = np.float32 if real32 else np.float64
    off = np.asarray(off, dtype=np.int64)
    nb = off.size - 1
    ncol = int(np.prod(nodes))
    x = np.asarray(x, dtype=dt).reshape(y.size, -1)
    y = np.asarray(y, dtype=dt)
    w0 = np.zeros(y.size, dtype=dt)
    coef, status, info, clip = np.zeros((nb, ncol), dtype=dt), np.full(nb, 105, dtype=np.int32), np.zeros((nb, 10)), np.zeros((nb, 6))
    active = []
    for k in range(nb):
        s, e = off[k], off[k + 1]
        if e > s:
            active.append(k)
            w0[s:e] = 1.0 if (w is None or w[s] < 0.0) else np.asarray(w[s:e], dtype=dt)
    wout = w0.copy()
    j = 0
    while active:
        idx = np.concatenate([np.arange(off[k], off[k + 1]) for k in active])
        sub = np.concatenate([[0], np.cumsum([off[k + 1] - off[k] for k in active])]).astype(np.int64)
        c, _, st, inf = capi.fit_many(ndim, sub, x[idx], y[idx], wout[idx], lo, hi, nodes, xtrap, real32=real32)
        go = []
        for a, k in enumerate(active):
            coef[k], status[k], info[k] = c[a], st[a], inf[a]
            clip[k, 2] = inf[a, 0]
            if st[a] == 0 and j < maxpass:
                go.append((a, k))
        if not go:
            break
        # (the starting weights as the weights: resid does not depend on them, and every point is written)
        resid, _, rc = capi.residuals_many(ndim, sub, x[idx], y[idx], w0[idx], c, lo, hi, nodes, real32=real32, want_stats=False)
        assert rc == 0
        w0d, wd = w0[idx].astype(np.float64), wout[idx].astype(np.float64)
        with np.errstate(invalid="ignore"):
            t = np.where(w0d != 0.0, w0d * resid[:idx.size].astype(np.float64), np.nan)
        stats, rc = capi.mad_many(sub, t, wd)
        assert rc == 0
        active = []
        for a, k in go:
            sl = slice(sub[a], sub[a + 1])
            w0k, wk = w0d[sl], wd[sl].copy()
            cand0 = w0k != 0.0
            assert stats[a, 0] == np.count_nonzero(wk)
            med, s = stats[a, 1], MAD_TO_SIGMA * stats[a, 2]
            clip[k, 0] += 1
            clip[k, 3], clip[k, 4] = s, med
            if s == 0.0:
                continue
            sel = cand0 if regrow else wk != 0.0
            out = decide(t[sl][sel], med, s, dt(klo), dt(khi), margin, f"problem {k}, pass {j}")
            was = wk[sel] != 0.0
            wk[sel] = np.where(out, 0.0, w0k[sel])
            wout[idx[sl]] = wk.astype(dt)
            clip[k, 1] = np.count_nonzero(cand0 & (wk == 0.0))
            clip[k, 5] += np.count_nonzero(~out & ~was)
            if np.any(~out != was):
                active.append(k)
        j += 1
    return coef, wout, status, info, clip


def run_and_compare(problems, regrow, xtrap=None, klo=KLO, khi=KHI, maxpass=MAXPASS, empty_at=(), real32=False):
    """The entry on a packed batch against yardstick 1 -> (coef, wout, status, info, clip, offsets)."""
    p0 = problems[0]
    nd, nodes = p0["ndim"], list(p0["nodes"])
    xt = p0["xtrap"] if xtrap is None else xtrap
    off, x, y, w = pack(problems, empty_at)
    lo, hi = [0.0] * nd, [1.0] * nd
    if real32:
        x, y, w = x.astype(np.float32), y.astype(np.float32), (None if w is None else w.astype(np.float32))
    coef, wout, rc, st, info, clip = capi.fit_many_clip_mad(nd, off, x, y, w, lo, hi, nodes, xt, klo, khi, maxpass, regrow, real32=real32)
    want = loop_yardstick(nd, off, x, y, w, lo, hi, nodes, xt, klo, khi, maxpass, regrow, real32=real32, margin=1e-5 if real32 else None)
    for k in range(off.size - 1):
        print(f"problem {k}: {off[k + 1] - off[k]} points, status {st[k]}, clip {clip[k]}, constraint rows {info[k, 1]:.0f}")
    assert same_bits(st, want[2]), (st, want[2])
    assert np.array_equal(wout == 0.0, want[1] == 0.0)
    assert same_bits(coef, want[0])
    if not real32:
        assert same_bits(wout, want[1])
        assert same_bits(clip, want[4]), (clip, want[4])
        assert same_bits(info[:, INFO_SLOTS], want[3][:, INFO_SLOTS])
    else:
        assert same_bits(clip[:, [0, 1, 2, 5]], want[4][:, [0, 1, 2, 5]])
    bad = [int(s) for s in st if s != 0]
    assert rc == (bad[0] if bad else 0)
    return coef, wout, st, info, clip, off


@pytest.mark.gpu
@pytest.mark.parametrize("regrow", [0, 1])
@pytest.mark.parametrize("names", [("c16", "first", "clean", "cluster", "drag"), ("c16_xt0",), ("c80w",), ("c65",), ("c56",), ("c1212",),
                                   ("negfirst",)], ids=lambda n: "+".join(n))
def test_recorded_cases_match_the_loop_and_the_reference(names, regrow):
    """Both yardsticks on the recorded cases: the bits of the loop of the entries, and the reference's mask, number of passes,
    returned points and coefficients.  c1212 runs at the LDS limit."""
    gold = load_golden("fit_many_clip_mad_ref")
    coef, wout, st, info, clip, off = run_and_compare([mad_case(n) for n in names], regrow)
    for k, name in enumerate(names):
        key = f"{name}_g{regrow}"
        assert st[k] == 0
        assert np.array_equal(wout[off[k]:off[k + 1]] == 0.0, gold["mask_" + key]), name
        assert clip[k, 0] == int(gold["passes_" + key]) and clip[k, 5] == int(gold["returned_" + key])
        err = relmax(coef[k], gold["coef_" + key])
        print(f"{key}: vs the reference's run {err:.2e}")
        assert err <= BAR
        p = mad_case(name)
        if p["w"] is not None and p["w"][0] >= 0.0:      # user zeros stay zeros, NaN values under them are never touched
            assert np.all(wout[off[k]:off[k + 1]][p["w"] == 0.0] == 0.0) and np.all(np.isfinite(coef[k]))
            assert clip[k, 1] == np.count_nonzero((p["w"] != 0.0) & (wout[off[k]:off[k + 1]] == 0.0))
        if regrow == 0:
            assert clip[k, 5] == 0
    if "c1212" in names:
        assert capi.debug_fit_many_stats()[1] == capi.fit_many_lds_bytes(2, [12, 12])


@pytest.mark.gpu
def test_drag_points_return_with_regrow():
    """The run of seven raised neighbours: without regrow the good points rejected beside it in pass 0 are lost; with it they
    return and fewer points end rejected."""
    p = mad_case("drag")
    args = (1, [0, p["y"].size], p["x"], p["y"], None, [0.0], [1.0], [16], 1.0, KLO, KHI, MAXPASS)
    _, w0, _, _, _, clip0 = capi.fit_many_clip_mad(*args, 0)
    _, w1, _, _, _, clip1 = capi.fit_many_clip_mad(*args, 1)
    print(f"drag: regrow 0 {clip0[0]}, regrow 1 {clip1[0]}")
    assert clip1[0, 5] > 0 and clip1[0, 1] < clip0[0, 1] and clip0[0, 5] == 0
    assert np.all(w0[p["raised"]] == 0.0) and np.all(w1[p["raised"]] == 0.0)
    assert clip1[0, 1] == np.count_nonzero(w1 == 0.0) and clip0[0, 1] == np.count_nonzero(w0 == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("xtrap", [1.0, 0.0])
def test_ragged_batch_across_the_wave_and_chunk_borders(xtrap):
    """1, 63, 64, 65, 127, 128, 129 and 300 points with an empty problem among them; at xtrap = 0 the one-point problem is 107."""
    for regrow in (0, 1):
        coef, wout, st, info, clip, off = run_and_compare([case(n) for n in RAGGED], regrow, xtrap=xtrap, empty_at=(3,))
        assert st[3] == 105 and np.all(clip[3] == 0.0) and np.all(info[3] == 0.0) and np.all(coef[3] == 0.0)
        assert st[0] == (0 if xtrap else 107)
        assert clip[-1, 1] >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("real32", [False, True], ids=["f64", "f32"])
def test_weights_zeros_nan_and_a_negative_first_weight_among_weighted_neighbours(real32):
    a = dict(case("c16"))
    rng = np.random.default_rng(9301)
    a["w"] = rng.uniform(0.5, 2.0, a["y"].size)
    a["w"][rng.random(a["y"].size) < 0.1] = 0.0
    a["y"] = np.where(a["w"] == 0.0, np.nan, a["y"])
    for regrow in (0, 1):
        coef, wout, st, info, clip, off = run_and_compare([a, case("negfirst"), a], regrow, real32=real32)
        assert not st.any() and np.array_equal(coef[0], coef[2])
        assert np.all(wout[off[0]:off[1]][a["w"] == 0.0] == 0.0)
        # the problem of the negative first weight ran without weights: its wout holds ones and zeros alone, and it is the fit of w = None
        p = dict(case("negfirst"))
        p["w"] = None
        alone = run_and_compare([p], regrow, real32=real32)
        assert set(np.unique(wout[off[1]:off[2]])) <= {0.0, 1.0} and np.array_equal(alone[0][0], coef[1])
        assert np.array_equal(alone[1], wout[off[1]:off[2]])


@pytest.mark.gpu
def test_f32_recorded_case_with_returning_points():
    run_and_compare([mad_case("drag"), mad_case("c16")], 1, real32=True)


@pytest.mark.gpu
def test_largest_1d_grid_one_problem():
    """The LDS limit in 1-D, 3 points per cell: the selection needs no byte beyond the fit's."""
    nod, m = largest_1d_nodes(), 3
    rng = np.random.default_rng(9302)
    x = ((np.repeat(np.arange(nod - 1), m) + np.tile((np.arange(m) + 0.37) / m, nod - 1)) / (nod - 1)).reshape(-1, 1)
    y = smooth(x) + rng.uniform(-NOISE, NOISE, x.shape[0])
    y[rng.permutation(x.shape[0])[:12]] += np.tile([1.0, -1.0], 6)
    coef, wout, st, info, clip, off = run_and_compare([dict(ndim=1, nodes=(nod,), xtrap=1.0, x=x, y=y, w=None)], 1)
    assert st[0] == 0 and clip[0, 1] >= 12 and capi.debug_fit_many_stats()[1] == capi.fit_many_lds_bytes(1, [nod])


@pytest.mark.gpu
def test_pass_limit_and_thresholds_switched_off():
    p = case("c16")
    args = (1, [0, p["y"].size], p["x"], p["y"], None, [0.0], [1.0], [16], 1.0)
    # maxpass = 0: the bits of fit_many, wout = the starting weights
    c0, w0, rc0, st0, info0, clip0 = capi.fit_many_clip_mad(*args, KLO, KHI, 0, 1)
    cf, rcf, stf, infof = capi.fit_many(*args)
    assert same_bits(c0, cf) and np.all(w0 == 1.0) and np.all(clip0[0] == [0, 0, p["y"].size, 0, 0, 0])
    assert same_bits(info0[:, INFO_SLOTS], infof[:, INFO_SLOTS])
    capi.fit_many_clip_mad(*args, KLO, KHI, 0, 1)
    assert capi.debug_fit_many_stats()[7] == 1
    # maxpass = 1 stops before the loop settles: one residual pass, and the coefficients belong to the wout returned
    c1, w1, _, _, _, clip1 = capi.fit_many_clip_mad(*args, KLO, KHI, 1, 0)
    assert clip1[0, 0] == 1 and clip1[0, 1] > 0
    assert same_bits(c1, capi.fit_many(1, [0, p["y"].size], p["x"], p["y"], w1, [0.0], [1.0], [16], 1.0)[0])
    # both sides off: one residual pass, nothing rejected
    for regrow in (0, 1):
        ci, wi, _, _, _, clipi = capi.fit_many_clip_mad(*args, float("inf"), float("inf"), MAXPASS, regrow)
        assert clipi[0, 0] == 1 and clipi[0, 1] == 0 and clipi[0, 3] > 0 and np.all(wi == 1.0) and same_bits(ci, cf)
    run_and_compare([p], 1, klo=float("inf"), khi=2.0)


def exact_case():
    """33 of 41 values are exactly the cubic 0 (the one cubic a fit returns to the bit: its right-hand side is 0), 8 are raised
    by 5: once those are out the fit is exact on every counted point."""
    rng = np.random.default_rng(9305)
    x = rng.uniform(0.0, 1.0, (41, 1))
    y = np.zeros(41)
    y[rng.permutation(41)[:8]] = 5.0
    return dict(ndim=1, nodes=(4,), xtrap=0.0, x=x, y=y, w=None)


def test_numpy_rule_stops_on_the_exact_fit():
    """(CPU) the scenario of the GPU test below does what its docstring says."""
    p = exact_case()
    for regrow in (0, 1):
        c, w, status, passes, returned = numpy_loop(p, KLO, KHI, MAXPASS, regrow)
        assert status == 0 and 2 <= passes < MAXPASS and np.all(c == 0.0) and np.all(w[p["y"] != 0.0] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("regrow", [0, 1])
def test_an_exact_fit_of_more_than_half_the_points_stops_with_s_zero(regrow):
    """The raised points go, the next fit is exact on the counted points, the MAD of their residuals is 0: the loop stops on
    s == 0 with nothing further rejected, before the pass limit."""
    p = exact_case()
    coef, wout, st, info, clip, off = run_and_compare([p], regrow)
    assert st[0] == 0 and 2 <= clip[0, 0] < MAXPASS and clip[0, 3] == 0.0 and clip[0, 4] == 0.0 and np.all(coef == 0.0)
    assert np.all(wout[p["y"] != 0.0] == 0.0) and clip[0, 1] == np.count_nonzero(wout == 0.0)
    # and the degenerate start: every value on the cubic, s == 0 in pass 0
    q = dict(p)
    q["y"] = np.zeros(41)
    coef, wout, st, info, clip, off = run_and_compare([q], regrow)
    assert clip[0, 0] == 1 and clip[0, 3] == 0.0 and clip[0, 1] == 0 and np.all(wout == 1.0)


@pytest.mark.gpu
def test_a_failure_stays_local():
    """xtrap = 0: once its cluster is rejected nothing holds the functions inside the gap; 107, zero coefficients, and the
    neighbours keep their bits."""
    good, bad = case("c16_xt0"), case("gap")
    coef, wout, st, info, clip, off = run_and_compare([good, bad, good], 0, xtrap=0.0)
    assert list(st) == [0, 107, 0] and np.all(coef[1] == 0.0) and clip[1, 0] >= 1 and clip[1, 1] >= 24
    assert "problem 1" in capi.last_error()
    alone = capi.fit_many_clip_mad(1, [0, good["y"].size], good["x"], good["y"], None, [0.0], [1.0], [16], 0.0, KLO, KHI, MAXPASS, 0)
    assert same_bits(coef[0], alone[0][0]) and same_bits(coef[2], alone[0][0])
    run_and_compare([good, bad, good], 1, xtrap=0.0)


@pytest.mark.gpu
def test_bits_do_not_depend_on_the_batch_the_position_or_the_entry():
    import torch
    names = ["c16", "first", "clean", "cluster", "drag", "r65"]
    ps = [mad_case(n) for n in names]
    off, x, y, _ = pack(ps)
    lo, hi, nodes = [0.0], [1.0], [16]
    coef, wout, rc, st, info, clip = capi.fit_many_clip_mad(1, off, x, y, None, lo, hi, nodes, 1.0, KLO, KHI, MAXPASS, 1)
    assert rc == 0
    for k, p in enumerate(ps):      # alone
        c1, w1, _, _, i1, cl1 = capi.fit_many_clip_mad(1, [0, p["y"].size], p["x"], p["y"], None, lo, hi, nodes, 1.0, KLO, KHI, MAXPASS, 1)
        assert same_bits(c1[0], coef[k]) and same_bits(w1, wout[off[k]:off[k + 1]]) and same_bits(cl1[0], clip[k]), names[k]
        assert same_bits(i1[0, INFO_SLOTS], info[k, INFO_SLOTS])
    # permuted, with an empty problem, a first global index that is not 0 and ldcoef > ncol; rows of `coef` that are not written stay
    off2, x2, y2, _ = pack(ps[::-1], empty_at=(2,), first=37)
    cin = np.full((len(ps) + 1, 20), 7.0)
    win = np.full(y2.size, 5.0)
    c2, w2, rc2, st2, _, cl2 = capi.fit_many_clip_mad(1, off2, x2, y2, None, lo, hi, nodes, 1.0, KLO, KHI, MAXPASS, 1, ldcoef=20, coef=cin,
                                                      wout=win)
    assert rc2 == 105 and st2[2] == 105 and np.all(c2[2] == 7.0) and np.all(c2[:, 16:] == 7.0) and np.all(w2[:37] == 5.0)
    rows = [0, 1, 3, 4, 5, 6]
    for r, k in zip(rows, range(len(ps) - 1, -1, -1)):
        assert same_bits(c2[r, :16], coef[k]) and same_bits(w2[off2[r]:off2[r + 1]], wout[off[k]:off[k + 1]]) and same_bits(cl2[r], clip[k])
    # the _dev entry on the same layout
    xd, yd = torch.from_numpy(x2).cuda(), torch.from_numpy(y2).cuda()
    cd = torch.full((len(ps) + 1, 20), 7.0, dtype=torch.float64, device="cuda")
    wd = torch.full((y2.size,), 5.0, dtype=torch.float64, device="cuda")
    rc3, st3, info3, cl3 = capi.fit_many_clip_mad_dev(1, off2, xd, yd, None, lo, hi, nodes, cd, wd, 1.0, KLO, KHI, MAXPASS, 1, ldcoef=20)
    assert rc3 == 105 and same_bits(st3, st2) and same_bits(cl3, cl2)
    assert same_bits(cd.cpu().numpy(), c2) and same_bits(wd.cpu().numpy(), w2)
    # the scratch holds the batch now: the second _dev call allocates nothing; [7] is the largest number of fits of a problem
    rc4, _, _, cl4 = capi.fit_many_clip_mad_dev(1, off2, xd, yd, None, lo, hi, nodes, cd, wd, 1.0, KLO, KHI, MAXPASS, 1, ldcoef=20)
    stats = capi.debug_fit_many_stats()
    assert rc4 == 105 and same_bits(cl4, cl2) and stats[6] == 0 and stats[2] == 1 and stats[3] == len(ps) and stats[4] == 1
    assert stats[7] >= int(clip[:, 0].max()) and clip[:, 0].max() < MAXPASS
    # weighted, on the device, 2-D
    p = dict(case("c65"))
    p["w"] = np.random.default_rng(9303).uniform(0.5, 2.0, p["y"].size)
    c_h, w_h, _, _, _, cl_h = capi.fit_many_clip_mad(2, [0, p["y"].size], p["x"], p["y"], p["w"], [0.0, 0.0], [1.0, 1.0], [6, 5], 0.0, KLO, KHI,
                                                     MAXPASS, 1)
    cd = torch.zeros((1, 30), dtype=torch.float64, device="cuda")
    wd = torch.zeros(p["y"].size, dtype=torch.float64, device="cuda")
    _, _, _, cl_d = capi.fit_many_clip_mad_dev(2, [0, p["y"].size], torch.from_numpy(p["x"]).cuda(), torch.from_numpy(p["y"]).cuda(),
                                               torch.from_numpy(p["w"]).cuda(), [0.0, 0.0], [1.0, 1.0], [6, 5], cd, wd, 0.0, KLO, KHI, MAXPASS, 1)
    assert same_bits(cd.cpu().numpy(), c_h) and same_bits(wd.cpu().numpy(), w_h) and same_bits(cl_d, cl_h) and cl_h[0, 1] > 0


@pytest.mark.gpu
def test_striding_gives_every_copy_the_bits_of_its_original():
    """More problems than workgroups: 6 000 copies of a 20-point problem interleaved with 6 000 of a second one."""
    a = make(9404, (16,), 20, 1.0, tiers=((1.0, 1),))
    b = make(9402, (16,), 20, 1.0, tiers=())
    lo, hi, nodes = [0.0], [1.0], [16]
    one = [capi.fit_many_clip_mad(1, [0, 20], p["x"], p["y"], None, lo, hi, nodes, 1.0, KLO, KHI, MAXPASS, 1) for p in (a, b)]
    off, x, y, _ = pack([a, b] * 6000)
    coef, wout, rc, st, info, clip = capi.fit_many_clip_mad(1, off, x, y, None, lo, hi, nodes, 1.0, KLO, KHI, MAXPASS, 1)
    stats = capi.debug_fit_many_stats()
    assert rc == 0 and not st.any() and stats[0] < 12000 and stats[2] == 1 and stats[3] == 12000
    w = wout.reshape(12000, 20)
    for h in (0, 1):
        assert np.all(coef[h::2] == one[h][0][0]) and np.all(w[h::2] == one[h][1]) and np.all(clip[h::2] == one[h][5][0])
    assert one[0][5][0, 1] >= 1 and not np.array_equal(one[0][0], one[1][0])


@pytest.mark.gpu
def test_dev_entry_keeps_its_scratch_and_does_not_wait_for_other_streams(clock, streams):
    """A second _dev call allocates nothing (slot [6]), and so returns while a delay still runs on another stream."""
    import torch
    assert streams.concurrent, NO_WINDOW
    p = mad_case("drag")
    n = p["y"].size
    xd, yd = torch.from_numpy(p["x"]).cuda(), torch.from_numpy(p["y"]).cuda()
    cd = torch.zeros((1, 16), dtype=torch.float64, device="cuda")
    wd = torch.zeros(n, dtype=torch.float64, device="cuda")

    def call(stream):
        return capi.fit_many_clip_mad_dev(1, [0, n], xd, yd, None, [0.0], [1.0], [16], cd, wd, 1.0, KLO, KHI, MAXPASS, 1, stream=stream)
    capi.shutdown()                         # (the scratch of earlier tests: the first call below has to allocate)
    call(0)
    first = capi.debug_fit_many_stats()[6]
    torch.cuda.synchronize()
    want_c, want_w = cd.cpu().numpy().copy(), wd.cpu().numpy().copy()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc, _, _, want_clip = call(0)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    assert first > 0 and capi.debug_fit_many_stats()[6] == 0 and rc == 0
    cd.zero_()
    wd.zero_()
    torch.cuda.synchronize()
    try:
        d = clock.delay(streams.S, max(5.0 * ms, T_FLOOR_MS))
        rc, _, _, clip = call(streams.S2.cuda_stream)
        running = d.running()
    finally:
        streams.S.synchronize()
        streams.S2.synchronize()
    d.check("fit_many_clip_mad beside a delay")
    assert rc == 0 and capi.debug_fit_many_stats()[6] == 0
    assert same_bits(cd.cpu().numpy(), want_c) and same_bits(wd.cpu().numpy(), want_w) and same_bits(clip, want_clip)
    assert running, "fit_many_clip_mad_dev on S2 returned only when the delay on S had ended"


FDIR = os.path.join(ROOT, "splpak_amd", "fortran")
PROG = os.path.join(FDIR, "build", "test_fit_many_clip_mad")


@pytest.mark.gpu
def test_fortran_initialize_many_robust_matches_fit_many_clip_mad(tmp_path):
    """The Fortran method on the drag case, its results written to a file by the program, agrees with capi.fit_many_clip_mad to the
    bit.  (The program's own checks run on the way: PASS.)"""
    if not os.path.exists(PROG):
        if not os.path.exists("/opt/rocm/bin/amdflang"):
            pytest.skip("amdflang not available")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "splpak_amd", "csrc")])
        subprocess.check_call(["make", "-C", FDIR])
    p = mad_case("drag")
    n = p["y"].size
    inp, out = tmp_path / "points.bin", tmp_path / "results.bin"
    with open(inp, "wb") as f:
        f.write(np.int64(n).tobytes() + np.ascontiguousarray(p["x"][:, 0]).tobytes() + np.ascontiguousarray(p["y"]).tobytes())
    r = subprocess.run([PROG, str(inp), str(out)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS test_fit_many_clip_mad" in r.stdout
    got = np.fromfile(out, dtype=np.float64)
    off = np.array([0, n, n, 2 * n], dtype=np.int64)      # the program's batch: the case, an empty problem, the case again
    x2, y2 = np.concatenate([p["x"], p["x"]]), np.concatenate([p["y"], p["y"]])
    coef, wout, rc, st, info, clip = capi.fit_many_clip_mad(1, off, x2, y2, None, [0.0], [1.0], [16], 1.0, KLO, KHI, MAXPASS, 1,
                                                            coef=np.full((3, 16), -7.0))      # (the program's fill: the empty problem's row stays)
    stats, rc2 = capi.mad_many(off, y2)
    want = np.concatenate([coef.ravel(), wout, clip.ravel(), stats.ravel()])
    assert rc2 == 0 and got.size == want.size and np.array_equal(got, want)
