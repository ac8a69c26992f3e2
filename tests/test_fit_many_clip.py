"""Sigma-clipped batch fits in one launch (splpak_fit_many_clip_*, csrc/fitmanyclip.hip).

Yardstick 1 is the loop of the three existing entries with the rule of include/splpak_hip.h applied in numpy between them
(`loop_yardstick`: capi.fit_many -> capi.residuals_many -> reject -> ...; a problem is frozen once it stops).  In f64 the new
entry must return its bits: coef, wout, status, clip, info slots 0-4 and 8.  In f32 residuals_many rounds resid to float, so
the helper asserts that no decision of any pass lies within 1e-5 relative of its threshold (100 times the float rounding of
t*t) and the test then asks for equal masks and identical coefficient bits.

Yardstick 2 is the unmodified reference run through the same loop (Reference.fit / Reference.evaluate) by
tools/gen_fit_many_clip_golden.py, recorded in tests/golden/fit_many_clip_ref.npz: same mask, same number of passes,
coefficients within BAR = 1e-10 relative max-norm.  The generator refuses a case with a decision within 1e-6 of its threshold.

CPU tier: exports, the argument ladder (decided before any device call), and the loop restated in numpy on NumpyManyFit
against the recorded masks and coefficients.
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

BAR = 1e-10
SYMBOLS = ("splpak_fit_many_clip_f64", "splpak_fit_many_clip_f32", "splpak_fit_many_clip_dev_f64", "splpak_fit_many_clip_dev_f32")
E_BADARG, E_UNSUPPORTED = -3, -4
NOISE = 0.05      # half width of the uniform noise: rms 0.029, nothing of it beyond 1.74 rms
INFO_SLOTS = [0, 1, 2, 3, 4, 8]


# ---------------------------------------------------------------------------------------------------------------
# The problems: dict(ndim, nodes, xtrap, x (n, ndim), y, w or None) on the box [0, 1]^ndim, and the clip parameters beside them.
def smooth(x):
    return np.sin(3.0 * x[:, 0]) + (0.5 * np.cos(2.0 * x[:, -1]) if x.shape[1] > 1 else 0.25 * x[:, 0] ** 2)


def make(seed, nodes, n, xtrap, tiers=((1.0, 3), (0.3, 2), (0.1, 1)), first_outlier=False):
    """n points U[0, 1]^ndim, a smooth field plus uniform noise, and outliers in tiers (amplitude, how many of each sign): 20
    sigma, then smaller ones that a pass can reject only after the larger ones have gone."""
    rng = np.random.default_rng(seed)
    nd = len(nodes)
    x = rng.uniform(0.0, 1.0, (n, nd))
    y = smooth(x) + rng.uniform(-NOISE, NOISE, n)
    where = rng.permutation(np.arange(1, n))
    at = 0
    for amp, count in tiers:
        for sign in (1.0, -1.0):
            for _ in range(count):
                if at < where.size:
                    y[where[at]] += sign * amp
                    at += 1
    if first_outlier:
        y[0] += 1.0
    return dict(ndim=nd, nodes=tuple(nodes), xtrap=xtrap, x=x, y=y, w=None)


@functools.lru_cache(maxsize=None)
def case(name):
    """The recorded cases (yardstick 2) and the further problems of the GPU tier, by name."""
    if name == "c16":            # 1-D, a one-wave workgroup, 300 points in three chunks
        return make(9101, (16,), 300, 1.0)
    if name == "c16_xt0":
        p = dict(case("c16"))
        p["xtrap"] = 0.0
        return p
    if name == "c80w":           # 1-D, 256 threads; weights with user zeros (NaN values under them)
        p = make(9102, (80,), 1600, 1.0)
        rng = np.random.default_rng(9103)
        w = rng.uniform(0.5, 2.0, p["y"].size)
        zero = rng.random(w.size) < 0.1
        zero[0] = False
        w[zero] = 0.0
        p["y"] = p["y"].copy()
        p["y"][zero] = np.nan
        p["w"] = w
        return p
    if name == "c65":            # 2-D, one wave, the permutation active
        return make(9104, (6, 5), 400, 0.0)
    if name == "c56":            # .. and the other way round: the same points with the dimensions swapped
        p = dict(case("c65"))
        p["nodes"] = (5, 6)
        p["x"] = np.ascontiguousarray(p["x"][:, ::-1])
        return p
    if name == "c1212":          # the LDS limit
        return make(9105, (12, 12), 2500, 0.0)
    if name == "first":          # the FIRST point is the outlier: its weight becomes 0, not negative
        return make(9106, (16,), 200, 1.0, tiers=((1.0, 1),), first_outlier=True)
    if name == "negfirst":       # a negative first weight: no weights for this problem
        p = make(9107, (16,), 150, 1.0)
        w = np.random.default_rng(9108).uniform(0.5, 2.0, 150)
        w[0] = -1.0
        p["w"] = w
        return p
    if name == "clean":          # no outlier: one residual pass, nothing rejected
        return make(9109, (16,), 600, 1.0, tiers=())
    if name == "cluster":        # outliers of alternating sign are all the points nearest to node 5: rejected, the node turns data-sparse
        # (20 evenly spaced points nearest to every other node, 10 at the two ends: no node is data-sparse before the cluster goes)
        rng = np.random.default_rng(9110)
        x = np.concatenate([(max(j - 0.5, 0.0) + (min(j + 0.5, 15.0) - max(j - 0.5, 0.0)) * (np.arange(m) + 0.5) / m) / 15
                            for j, m in ((j, 10 if j in (0, 15) else 20) for j in range(16) if j != 5)])
        xc = (4.5 + (np.arange(18) + 0.5) / 18) / 15
        y = smooth(x.reshape(-1, 1)) + rng.uniform(-NOISE, NOISE, x.size)
        yc = smooth(xc.reshape(-1, 1)) + np.where(np.arange(18) % 2 == 0, 1.0, -1.0)
        order = rng.permutation(x.size + 18)
        return dict(ndim=1, nodes=(16,), xtrap=1.0, x=np.concatenate([x, xc])[order].reshape(-1, 1), y=np.concatenate([y, yc])[order], w=None)
    if name == "gap":            # .. are all the points of four cells: once rejected nothing holds the functions inside the gap
        rng = np.random.default_rng(9111)
        x = rng.uniform(0.0, 1.0, 900)
        x = x[(x < 4.0 / 15) | (x > 8.0 / 15)][:500]
        xc = (4.0 + 4.0 * (np.arange(24) + 0.5) / 24) / 15
        y = smooth(x.reshape(-1, 1)) + rng.uniform(-NOISE, NOISE, x.size)
        yc = smooth(xc.reshape(-1, 1)) + np.where(np.arange(24) % 2 == 0, 1.0, -1.0)
        order = rng.permutation(x.size + 24)
        return dict(ndim=1, nodes=(16,), xtrap=0.0, x=np.concatenate([x, xc])[order].reshape(-1, 1), y=np.concatenate([y, yc])[order], w=None)
    if name.startswith("r"):     # the ragged batch: "r<points>"
        n = int(name[1:])
        return make(9200 + n, (16,), n, 1.0, tiers=((1.0, 1), (0.3, 1)) if n >= 63 else ())
    raise KeyError(name)


KLO, KHI, MAXPASS = 2.5, 3.0, 8
GOLDEN_NAMES = ["c16", "c16_xt0", "c80w", "c65", "c56", "c1212", "first", "negfirst", "clean", "cluster"]
RAGGED = ["r1", "r63", "r64", "r65", "r127", "r128", "r129", "r300"]


def pack(problems, empty_at=(), first=0):
    """-> (offsets, x, y, w or None) of a batch whose first point has the global index `first`; an empty problem before every
    position listed in empty_at.  The arrays are `first` points longer at the front (never read)."""
    xs, ys, ws, off = [], [], [], [first]
    weighted = any(p["w"] is not None for p in problems)
    nd = problems[0]["ndim"]
    if first:
        xs.append(np.full((first, nd), 1e30))
        ys.append(np.full(first, np.nan))
        ws.append(np.full(first, np.nan))
    for k, p in enumerate(problems):
        if k in empty_at:
            off.append(off[-1])
        xs.append(p["x"])
        ys.append(p["y"])
        ws.append(p["w"] if p["w"] is not None else np.ones(p["y"].size))
        off.append(off[-1] + p["y"].size)
    return np.array(off, dtype=np.int64), np.concatenate(xs), np.concatenate(ys), (np.concatenate(ws) if weighted else None)


def start_weights(p):
    """Step 1 of the rule."""
    w = p["w"]
    return np.ones(p["y"].size) if w is None or w[0] < 0.0 else np.asarray(w, dtype=np.float64).copy()


def decide(t, v, klo, khi, margin=None, what=""):
    """Step 5 on the weighted residuals t of the counted points -> rejected (bool).  margin: assert that no decision lies within
    that relative distance of its threshold."""
    klo2, khi2 = np.float64(klo) * np.float64(klo), np.float64(khi) * np.float64(khi)
    tt = t * t
    with np.errstate(invalid="ignore"):
        thr = np.where(t > 0.0, khi2 * v, klo2 * v)
        rej = ((t > 0.0) & (tt > khi2 * v)) | ((t < 0.0) & (tt > klo2 * v))
        if margin is not None:
            fin = np.isfinite(thr) & (thr > 0.0) & (t != 0.0)
            near = np.abs(tt[fin] - thr[fin]) <= margin * thr[fin]
            assert not near.any(), f"{what}: a decision within {margin:g} of its threshold"
    return rej


# ---------------------------------------------------------------------------------------------------------------
# The loop restated in numpy on NumpyManyFit (CPU tier; the generator runs the same loop on the reference)
def numpy_evaluate(f, c):
    """t = w (y - f) at the points NumpyManyFit kept (non-zero weight), for coefficients c in the caller's order."""
    xv = np.zeros(f.ncol)
    for node in range(f.ncol):
        inn = [node % f.nod[0], node // f.nod[0]][:f.ndim]
        xv[node] = c[sum(inn[d] * f.refstride[d] for d in range(f.ndim))]
    return f.b - np.einsum("ij,ij->i", f.vals, xv[f.cols])


def numpy_loop(p, klo, khi, maxpass, margin=None):
    """-> (coef, wout, status, passes, rejected)."""
    w = start_weights(p)
    passes = rejected = 0
    for j in range(maxpass + 1):
        q = dict(p)
        q["w"] = w
        q["y"] = np.where(w != 0.0, p["y"], 0.0)
        f = NumpyManyFit(q)
        c, status, _ = f.fit()
        if status != 0 or j == maxpass:
            break
        t = numpy_evaluate(f, c)
        v = float(t @ t) / t.size
        passes += 1
        rej = decide(t, v, klo, khi, margin, f"pass {j}")
        if not rej.any():
            break
        idx = np.nonzero(w != 0.0)[0]
        w[idx[rej]] = 0.0
        rejected += int(rej.sum())
    return c, w, status, passes, rejected


# ---------------------------------------------------------------------------------------------------------------
# CPU tier
def test_symbols_exported():
    lib = capi.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in capi.SYMBOLS


def _call(ndim=1, nbatch=1, offsets=(0, 8), x="ok", l1xdat=1, y="ok", w=None, xmin=(0.0, 0.0), xmax=(1.0, 1.0), nodes=(4, 4), ldcoef=16,
          coef="ok", wout="ok", klo=3.0, khi=3.0, maxpass=3):
    """splpak_fit_many_clip_f64 on raw arguments -> (rc, coef, wout, status); "ok": a valid array, None: a null pointer,
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
    st = np.full(8, -999, dtype=np.int32)
    xs = np.linspace(0.0, 1.0, 32)
    wd = np.ones(32) if (w == "ok" or wout == "wdata") else None
    wd_p = arr(wd, np.float64, dp)
    wo_p = wd_p if wout == "wdata" else (wo.ctypes.data_as(dp) if wout == "ok" else None)
    rc = capi.lib().splpak_fit_many_clip_f64(ndim, nbatch, arr(offsets, np.int64, lp), arr(xs if x == "ok" else x, np.float64, dp), l1xdat,
                                             arr(xs if y == "ok" else y, np.float64, dp), wd_p, arr(xmin, np.float64, dp),
                                             arr(xmax, np.float64, dp), arr(nodes, np.int32, ip), 1.0, klo, khi, maxpass, wo_p,
                                             arr(cf, np.float64, dp) if coef is not None else None, ldcoef, st.ctypes.data_as(ip), None, None)
    return rc, cf, wo, st


def test_status_ladder_in_order_before_any_device_call():
    """The ladder of splpak_fit_many_* in its order, every rung with every LATER rung failing too, then the four clip conditions
    in the group of the null data pointers, before the LDS rule; coef, wout and status stay as they were.  No rung asks for a
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
    for want, kw in ladder:
        rc, cf, wo, st = _call(**kw)
        assert rc == want, (want, rc, kw)
        assert np.all(cf == 777.0) and np.all(wo == 555.0) and np.all(st == -999), kw
    # the clip conditions are what refuses a call that is otherwise admitted (a batch of empty problems, answered on the host)
    assert _call(nbatch=2, offsets=(5, 5, 5))[0] == 105
    for kw in (dict(wout=None), dict(wout="wdata"), dict(maxpass=-1), dict(klo=0.5), dict(khi=float("nan"))):
        rc, cf, wo, st = _call(nbatch=2, offsets=(5, 5, 5), **kw)
        assert rc == E_BADARG and np.all(st == -999), kw
        assert "wout" in capi.last_error()
    # problems without points: 105 each, coef and wout untouched, clip zeroed
    rc, cf, wo, st = _call(nbatch=2, offsets=(5, 5, 5))
    assert rc == 105 and list(st[:2]) == [105, 105] and np.all(cf == 777.0) and np.all(wo == 555.0)
    assert capi.debug_fit_many_stats()[2:5] == (0, 0, 2) and capi.debug_fit_many_stats()[7] == 0


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_numpy_restatement_matches_recorded_reference(name):
    """The loop without a GPU: the fit of NumpyManyFit, its rows as the residuals, the rule; against the reference's loop."""
    gold = load_golden("fit_many_clip_ref")
    p = case(name)
    c, w, status, passes, rejected = numpy_loop(p, KLO, KHI, MAXPASS, margin=1e-9)
    assert status == 0
    assert np.array_equal(w == 0.0, gold["mask_" + name]), name
    assert passes == int(gold["passes_" + name]) and rejected == int(gold["rejected_" + name])
    err = relmax(c, gold["coef_" + name])
    print(f"{name}: numpy loop vs the reference's loop {err:.2e}, {passes} passes, {rejected} rejected")
    assert err <= BAR


# ---------------------------------------------------------------------------------------------------------------
# GPU tier
def loop_yardstick(ndim, off, x, y, w, lo, hi, nodes, xtrap, klo, khi, maxpass, real32=False, margin=None):
    """Yardstick 1: capi.fit_many -> capi.residuals_many -> the rule in numpy -> ..., each round on the batch of the problems that
    have not stopped (the bits of a problem do not depend on its batch: tests/test_fit_many.py, tests/test_eval_many.py).
    -> (coef, wout, status, info, clip) as capi.fit_many_clip returns them; coefficient rows of problems without points are 0."""
    dt = np.float32 if real32 else np.float64
    off = np.asarray(off, dtype=np.int64)
    nb = off.size - 1
    ncol = int(np.prod(nodes))
    x = np.asarray(x, dtype=dt).reshape(y.size, -1)
    y = np.asarray(y, dtype=dt)
    wout = np.zeros(y.size, dtype=dt)
    coef, status, info, clip = np.zeros((nb, ncol), dtype=dt), np.full(nb, 105, dtype=np.int32), np.zeros((nb, 10)), np.zeros((nb, 4))
    active = []
    for k in range(nb):
        s, e = off[k], off[k + 1]
        if e > s:
            active.append(k)
            wout[s:e] = 1.0 if (w is None or w[s] < 0.0) else np.asarray(w[s:e], dtype=dt)
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
        resid, stats, rc = capi.residuals_many(ndim, sub, x[idx], y[idx], wout[idx], c, lo, hi, nodes, real32=real32)
        assert rc == 0
        active = []
        for a, k in go:
            sl = slice(sub[a], sub[a + 1])
            wk = wout[idx[sl]].astype(np.float64)
            counted = wk != 0.0
            assert counted.sum() == stats[a, 0]
            v = stats[a, 1] / stats[a, 0]
            t = wk[counted] * resid[sl][counted].astype(np.float64)
            rej = decide(t, v, dt(klo), dt(khi), margin, f"problem {k}, pass {j}")
            clip[k, 0] += 1
            clip[k, 1] += rej.sum()
            clip[k, 3] = v
            if rej.any():
                wout[idx[sl][counted][rej]] = 0.0
                active.append(k)
        j += 1
    return coef, wout, status, info, clip


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def run_and_compare(problems, xtrap=None, klo=KLO, khi=KHI, maxpass=MAXPASS, empty_at=(), real32=False):
    """The entry on a packed batch against yardstick 1 -> (coef, wout, status, info, clip, offsets)."""
    p0 = problems[0]
    nd, nodes = p0["ndim"], list(p0["nodes"])
    xt = p0["xtrap"] if xtrap is None else xtrap
    off, x, y, w = pack(problems, empty_at)
    lo, hi = [0.0] * nd, [1.0] * nd
    if real32:
        x, y, w = x.astype(np.float32), y.astype(np.float32), (None if w is None else w.astype(np.float32))
    coef, wout, rc, st, info, clip = capi.fit_many_clip(nd, off, x, y, w, lo, hi, nodes, xt, klo, khi, maxpass, real32=real32)
    want = loop_yardstick(nd, off, x, y, w, lo, hi, nodes, xt, klo, khi, maxpass, real32=real32, margin=1e-5 if real32 else None)
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
        assert same_bits(clip[:, :3], want[4][:, :3])
    bad = [int(s) for s in st if s != 0]
    assert rc == (bad[0] if bad else 0)
    return coef, wout, st, info, clip, off


@pytest.mark.gpu
@pytest.mark.parametrize("names", [("c16", "first", "clean", "cluster"), ("c16_xt0",), ("c80w",), ("c65",), ("c56",), ("c1212",), ("negfirst",)],
                         ids=lambda n: "+".join(n))
def test_recorded_cases_match_the_loop_and_the_reference(names):
    """Both yardsticks on the recorded cases: the bits of the loop of the existing entries, and the reference's mask, number of
    passes and coefficients."""
    gold = load_golden("fit_many_clip_ref")
    coef, wout, st, info, clip, off = run_and_compare([case(n) for n in names])
    for k, name in enumerate(names):
        assert st[k] == 0
        assert np.array_equal(wout[off[k]:off[k + 1]] == 0.0, gold["mask_" + name]), name
        assert clip[k, 0] == int(gold["passes_" + name]) and clip[k, 1] == int(gold["rejected_" + name])
        err = relmax(coef[k], gold["coef_" + name])
        print(f"{name}: vs the reference's loop {err:.2e}")
        assert err <= BAR
        p = case(name)
        if p["w"] is not None and p["w"][0] >= 0.0:      # user zeros stay zeros, NaN values under them are never touched
            assert np.all(wout[off[k]:off[k + 1]][p["w"] == 0.0] == 0.0) and np.all(np.isfinite(coef[k]))
    if "clean" in names:
        k = names.index("clean")
        assert clip[k, 0] == 1 and clip[k, 1] == 0 and np.all(wout[off[k]:off[k + 1]] == 1.0)
    if "first" in names:            # the first point is rejected: its weight is 0, and the others still count as weighted
        k = names.index("first")
        assert wout[off[k]] == 0.0 and clip[k, 1] >= 1
    if "cluster" in names:          # xtrap = 1: the node the cluster was nearest to turns data-sparse, constraint rows appear
        k = names.index("cluster")
        p = case("cluster")
        first_fit = capi.fit_many(1, [0, p["y"].size], p["x"], p["y"], None, [0.0], [1.0], [16], 1.0)[3][0]
        assert clip[k, 1] >= 18 and info[k, 1] > first_fit[1], (info[k, 1], first_fit[1])


@pytest.mark.gpu
def test_asymmetric_thresholds_and_swapped_dimensions():
    p = case("c16")
    _, w_a, _, _, _, clip_a = capi.fit_many_clip(1, [0, p["y"].size], p["x"], p["y"], None, [0.0], [1.0], [16], 1.0, 1.5, 6.0, MAXPASS)
    _, w_b, _, _, _, clip_b = capi.fit_many_clip(1, [0, p["y"].size], p["x"], p["y"], None, [0.0], [1.0], [16], 1.0, 6.0, 1.5, MAXPASS)
    r = p["y"] - smooth(p["x"])
    assert np.all(r[(w_a == 0.0) & (w_b != 0.0)] < 0.0) and np.all(r[(w_b == 0.0) & (w_a != 0.0)] > 0.0)
    assert ((w_a == 0.0) != (w_b == 0.0)).any()
    # 6 x 5 and 5 x 6: the same points with the dimensions swapped give the same mask and the transposed coefficients
    a, b = case("c65"), case("c56")
    ca, wa, _, _, _, cla = capi.fit_many_clip(2, [0, a["y"].size], a["x"], a["y"], None, [0.0, 0.0], [1.0, 1.0], [6, 5], 0.0, KLO, KHI, MAXPASS)
    cb, wb, _, _, _, clb = capi.fit_many_clip(2, [0, b["y"].size], b["x"], b["y"], None, [0.0, 0.0], [1.0, 1.0], [5, 6], 0.0, KLO, KHI, MAXPASS)
    assert np.array_equal(wa, wb) and np.array_equal(cla[:, :3], clb[:, :3])
    assert relmax(cb[0].reshape(6, 5), ca[0].reshape(5, 6).T) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("xtrap", [1.0, 0.0])
def test_ragged_batch_across_the_wave_and_chunk_borders(xtrap):
    """1, 63, 64, 65, 127, 128, 129 and 300 points with an empty problem among them; at xtrap = 0 the one-point problem is 107."""
    coef, wout, st, info, clip, off = run_and_compare([case(n) for n in RAGGED], xtrap=xtrap, empty_at=(3,))
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
    coef, wout, st, info, clip, off = run_and_compare([a, case("negfirst"), a], real32=real32)
    assert not st.any() and np.array_equal(coef[0], coef[2])
    # the problem of the negative first weight ran without weights: its wout holds ones and zeros alone, and it is the fit of w = None
    p = dict(case("negfirst"))
    p["w"] = None
    alone = run_and_compare([p], real32=real32)
    assert set(np.unique(wout[off[1]:off[2]])) <= {0.0, 1.0} and np.array_equal(alone[0][0], coef[1])
    assert np.array_equal(alone[1], wout[off[1]:off[2]])


@pytest.mark.gpu
def test_largest_1d_grid_one_problem():
    """The LDS limit in 1-D, 3 points per cell: the loop needs no byte beyond the fit's."""
    nod, m = largest_1d_nodes(), 3
    rng = np.random.default_rng(9302)
    x = ((np.repeat(np.arange(nod - 1), m) + np.tile((np.arange(m) + 0.37) / m, nod - 1)) / (nod - 1)).reshape(-1, 1)
    y = smooth(x) + rng.uniform(-NOISE, NOISE, x.shape[0])
    y[rng.permutation(x.shape[0])[:12]] += np.tile([1.0, -1.0], 6)
    coef, wout, st, info, clip, off = run_and_compare([dict(ndim=1, nodes=(nod,), xtrap=1.0, x=x, y=y, w=None)])
    assert st[0] == 0 and clip[0, 1] >= 12 and capi.debug_fit_many_stats()[1] == capi.fit_many_lds_bytes(1, [nod])


@pytest.mark.gpu
def test_pass_limit_and_thresholds_switched_off():
    p = case("c16")
    args = (1, [0, p["y"].size], p["x"], p["y"], None, [0.0], [1.0], [16], 1.0)
    full = capi.fit_many_clip(*args, KLO, KHI, MAXPASS)
    assert full[5][0, 0] >= 3, full[5]      # the data needs three passes at least
    # maxpass = 0: the bits of fit_many, wout = the starting weights
    c0, w0, rc0, st0, info0, clip0 = capi.fit_many_clip(*args, KLO, KHI, 0)
    cf, rcf, stf, infof = capi.fit_many(*args)
    assert same_bits(c0, cf) and np.all(w0 == 1.0) and np.all(clip0[0] == [0, 0, p["y"].size, 0])
    assert same_bits(info0[:, INFO_SLOTS], infof[:, INFO_SLOTS]) and capi.debug_fit_many_stats()[7] == 0
    capi.fit_many_clip(*args, KLO, KHI, 0)
    assert capi.debug_fit_many_stats()[7] == 1
    # maxpass = 1 stops before the loop settles: one residual pass, and the coefficients belong to the wout returned
    c1, w1, _, _, _, clip1 = capi.fit_many_clip(*args, KLO, KHI, 1)
    assert clip1[0, 0] == 1 and 0 < clip1[0, 1] < full[5][0, 1]
    assert same_bits(c1, capi.fit_many(1, [0, p["y"].size], p["x"], p["y"], w1, [0.0], [1.0], [16], 1.0)[0])
    assert capi.debug_fit_many_stats()[7] == 0      # (a plain fit_many call)
    # both sides off: one residual pass, nothing rejected
    ci, wi, _, _, _, clipi = capi.fit_many_clip(*args, float("inf"), float("inf"), MAXPASS)
    assert clipi[0, 0] == 1 and clipi[0, 1] == 0 and np.all(wi == 1.0) and same_bits(ci, cf)
    run_and_compare([p], klo=float("inf"), khi=2.0)


@pytest.mark.gpu
def test_a_failure_stays_local():
    """xtrap = 0: once its cluster is rejected nothing holds the functions inside the gap; 107, zero coefficients, and the
    neighbours keep their bits."""
    good, bad = case("c16_xt0"), case("gap")
    coef, wout, st, info, clip, off = run_and_compare([good, bad, good], xtrap=0.0)
    assert list(st) == [0, 107, 0] and np.all(coef[1] == 0.0) and clip[1, 0] >= 1 and clip[1, 1] >= 24
    assert "problem 1" in capi.last_error()
    alone = capi.fit_many_clip(1, [0, good["y"].size], good["x"], good["y"], None, [0.0], [1.0], [16], 0.0, KLO, KHI, MAXPASS)
    assert same_bits(coef[0], alone[0][0]) and same_bits(coef[2], alone[0][0])
    # the first fit of the failing problem was fine
    assert capi.fit_many(1, [0, bad["y"].size], bad["x"], bad["y"], None, [0.0], [1.0], [16], 0.0)[1] == 0


@pytest.mark.gpu
def test_bits_do_not_depend_on_the_batch_the_position_or_the_entry():
    import torch
    names = ["c16", "first", "clean", "cluster", "r65"]
    ps = [case(n) for n in names]
    off, x, y, _ = pack(ps)
    lo, hi, nodes = [0.0], [1.0], [16]
    coef, wout, rc, st, info, clip = capi.fit_many_clip(1, off, x, y, None, lo, hi, nodes, 1.0, KLO, KHI, MAXPASS)
    assert rc == 0
    for k, p in enumerate(ps):      # alone
        c1, w1, _, _, i1, cl1 = capi.fit_many_clip(1, [0, p["y"].size], p["x"], p["y"], None, lo, hi, nodes, 1.0, KLO, KHI, MAXPASS)
        assert same_bits(c1[0], coef[k]) and same_bits(w1, wout[off[k]:off[k + 1]]) and same_bits(cl1[0], clip[k]), names[k]
        assert same_bits(i1[0, INFO_SLOTS], info[k, INFO_SLOTS])
    # permuted, with an empty problem, a first global index that is not 0 and ldcoef > ncol; rows of `coef` that are not written stay
    off2, x2, y2, _ = pack(ps[::-1], empty_at=(2,), first=37)
    cin = np.full((len(ps) + 1, 20), 7.0)
    win = np.full(y2.size, 5.0)
    c2, w2, rc2, st2, _, cl2 = capi.fit_many_clip(1, off2, x2, y2, None, lo, hi, nodes, 1.0, KLO, KHI, MAXPASS, ldcoef=20, coef=cin, wout=win)
    assert rc2 == 105 and st2[2] == 105 and np.all(c2[2] == 7.0) and np.all(c2[:, 16:] == 7.0) and np.all(w2[:37] == 5.0)
    rows = [0, 1, 3, 4, 5]
    for r, k in zip(rows, range(len(ps) - 1, -1, -1)):
        assert same_bits(c2[r, :16], coef[k]) and same_bits(w2[off2[r]:off2[r + 1]], wout[off[k]:off[k + 1]]) and same_bits(cl2[r], clip[k])
    # the _dev entry on the same layout
    xd, yd = torch.from_numpy(x2).cuda(), torch.from_numpy(y2).cuda()
    cd = torch.full((len(ps) + 1, 20), 7.0, dtype=torch.float64, device="cuda")
    wd = torch.full((y2.size,), 5.0, dtype=torch.float64, device="cuda")
    rc3, st3, info3, cl3 = capi.fit_many_clip_dev(1, off2, xd, yd, None, lo, hi, nodes, cd, wd, 1.0, KLO, KHI, MAXPASS, ldcoef=20)
    assert rc3 == 105 and same_bits(st3, st2) and same_bits(cl3, cl2)
    assert same_bits(cd.cpu().numpy(), c2) and same_bits(wd.cpu().numpy(), w2)
    # the scratch holds the batch now: the second _dev call allocates nothing; [7] is the largest number of fits of a problem
    rc4, _, _, cl4 = capi.fit_many_clip_dev(1, off2, xd, yd, None, lo, hi, nodes, cd, wd, 1.0, KLO, KHI, MAXPASS, ldcoef=20)
    stats = capi.debug_fit_many_stats()
    assert rc4 == 105 and same_bits(cl4, cl2) and stats[6] == 0 and stats[2] == 1 and stats[3] == len(ps) and stats[4] == 1
    # (a problem that stops by rejecting nothing ran as many fits as residual passes; MAXPASS is not reached here)
    assert stats[7] == int(clip[:, 0].max()) and clip[:, 0].max() < MAXPASS
    # weighted, on the device, 2-D
    p = dict(case("c65"))
    p["w"] = np.random.default_rng(9303).uniform(0.5, 2.0, p["y"].size)
    c_h, w_h, _, _, _, cl_h = capi.fit_many_clip(2, [0, p["y"].size], p["x"], p["y"], p["w"], [0.0, 0.0], [1.0, 1.0], [6, 5], 0.0, KLO, KHI, MAXPASS)
    cd = torch.zeros((1, 30), dtype=torch.float64, device="cuda")
    wd = torch.zeros(p["y"].size, dtype=torch.float64, device="cuda")
    _, _, _, cl_d = capi.fit_many_clip_dev(2, [0, p["y"].size], torch.from_numpy(p["x"]).cuda(), torch.from_numpy(p["y"]).cuda(),
                                           torch.from_numpy(p["w"]).cuda(), [0.0, 0.0], [1.0, 1.0], [6, 5], cd, wd, 0.0, KLO, KHI, MAXPASS)
    assert same_bits(cd.cpu().numpy(), c_h) and same_bits(wd.cpu().numpy(), w_h) and same_bits(cl_d, cl_h) and cl_h[0, 1] > 0


@pytest.mark.gpu
def test_striding_gives_every_copy_the_bits_of_its_original():
    """More problems than workgroups: 6 000 copies of a 20-point problem interleaved with 6 000 of a second one."""
    a = make(9404, (16,), 20, 1.0, tiers=((1.0, 1),))      # (three passes, three points rejected)
    b = make(9402, (16,), 20, 1.0, tiers=())
    lo, hi, nodes = [0.0], [1.0], [16]
    one = [capi.fit_many_clip(1, [0, 20], p["x"], p["y"], None, lo, hi, nodes, 1.0, KLO, KHI, MAXPASS) for p in (a, b)]
    off, x, y, _ = pack([a, b] * 6000)
    coef, wout, rc, st, info, clip = capi.fit_many_clip(1, off, x, y, None, lo, hi, nodes, 1.0, KLO, KHI, MAXPASS)
    stats = capi.debug_fit_many_stats()
    assert rc == 0 and not st.any() and stats[0] < 12000 and stats[2] == 1 and stats[3] == 12000
    w = wout.reshape(12000, 20)
    for h in (0, 1):
        assert np.all(coef[h::2] == one[h][0][0]) and np.all(w[h::2] == one[h][1]) and np.all(clip[h::2] == one[h][5][0])
    assert one[0][5][0, 1] >= 1 and not np.array_equal(one[0][0], one[1][0])


FDIR = os.path.join(ROOT, "splpak_amd", "fortran")
PROG = os.path.join(FDIR, "build", "test_fit_many_clip")


@pytest.mark.gpu
def test_fortran_initialize_many_clipped_matches_fit_many_clip(tmp_path):
    """The Fortran method on the recorded 1-D case, its results written to a file by the program, agrees with capi.fit_many_clip to
    the bit.  (The program's own checks run on the way: PASS.)"""
    if not os.path.exists(PROG):
        if not os.path.exists("/opt/rocm/bin/amdflang"):
            pytest.skip("amdflang not available")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "splpak_amd", "csrc")])
        subprocess.check_call(["make", "-C", FDIR])
    p = case("c16")
    n = p["y"].size
    inp, out = tmp_path / "points.bin", tmp_path / "results.bin"
    with open(inp, "wb") as f:
        f.write(np.int64(n).tobytes() + np.ascontiguousarray(p["x"][:, 0]).tobytes() + np.ascontiguousarray(p["y"]).tobytes())
    r = subprocess.run([PROG, str(inp), str(out)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS test_fit_many_clip" in r.stdout
    got = np.fromfile(out, dtype=np.float64)
    off = np.array([0, n, n, 2 * n], dtype=np.int64)      # the program's batch: the case, an empty problem, the case again
    x2, y2 = np.concatenate([p["x"], p["x"]]), np.concatenate([p["y"], p["y"]])
    coef, wout, rc, st, info, clip = capi.fit_many_clip(1, off, x2, y2, None, [0.0], [1.0], [16], 1.0, KLO, KHI, MAXPASS,
                                                        coef=np.full((3, 16), -7.0))      # (the program's fill: the empty problem's row stays)
    want = np.concatenate([coef.ravel(), wout, clip.ravel()])
    assert got.size == want.size and np.array_equal(got, want)
