"""Many small independent fits on one node grid in one launch (splpak_fit_many_*, csrc/fitmany.hip).

Every problem of a batch gets what splcw (splcc without weights) does for its own points: yardsticks are the unmodified
reference, one Reference.fit per problem (live through the `reference` fixture where oracle/_ref is built and the problem is
small enough for its dense solver to take a few seconds at the most; its recorded coefficients in tests/golden/fit_many_ref.npz, written by
tools/gen_fit_many_golden.py from the same seeded inputs, always), and the library's own single fit.  Bar 1e-10 max-norm
relative per problem, the project's parity bar.

CPU tier: exports, the argument ladder (every rung decided before any device call), the LDS rule, and a numpy restatement of
the per-problem algorithm -- band normal equations with the constraint rows, Cholesky with the pivot test, the refinement rule --
against the recorded reference: the algebra, pinned without a GPU.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from splpak_amd import capi
from tests.conftest import ROOT, load_golden, relmax

BAR = 1e-10
LDS_BUDGET = 65536
SYMBOLS = ("splpak_fit_many_f64", "splpak_fit_many_f32", "splpak_fit_many_dev_f64", "splpak_fit_many_dev_f32",
           "splpak_fit_many_lds_bytes", "splpak_debug_fit_many_stats")
E_BADARG, E_UNSUPPORTED = -3, -4
# The live reference solves dense rows by Householder steps, ~2 ncol^2 flop per row.  Measured on one CPU core, by ncol^2 x points:
# 2.6e7 (12 x 11 nodes, 1 500 points) 0.02 s, 1.7e8 (130 nodes, 10 200 points) 0.08 s, 2.2e9 (896 nodes, 2 685 points) 2.7 s,
# 6.5e9 (896 nodes, 8 055 points) 7.5 s.  Live up to the third; the 3- and 17-fold problems of the largest 1-D grid (7.5 s and about
# 45 s) are judged by the recorded coefficients alone.
LIVE_WORK = 2.5e9


# ---------------------------------------------------------------------------------------------------------------
# The problems.  Every one is a dict(ndim, nodes, xtrap, x (n, l1xdat), y, w or None), on the box [0, 1]^ndim unless it has lo, hi.
def largest_1d_nodes():
    """The largest 1-D grid the LDS rule admits, from splpak_fit_many_lds_bytes."""
    lo, hi = 4, 1 << 16
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if capi.fit_many_lds_bytes(1, [mid]) <= LDS_BUDGET:
            lo = mid
        else:
            hi = mid
    return lo


def largest_square_nodes():
    """The largest near-square 2-D grid (n, n) or (n + 1, n) the LDS rule admits."""
    n = 4
    while capi.fit_many_lds_bytes(2, [n + 1, n + 1]) <= LDS_BUDGET:
        n += 1
    return (n + 1, n) if capi.fit_many_lds_bytes(2, [n + 1, n]) <= LDS_BUDGET else (n, n)


def _values(x, rng):
    """A smooth field plus noise at the points x (n, ndim)."""
    s = np.sin(3.0 * x[:, 0]) + (0.5 * np.cos(2.0 * x[:, -1]) if x.shape[1] > 1 else 0.25 * x[:, 0] ** 2)
    return s + 0.05 * rng.standard_normal(x.shape[0])


def _points_1d(base, mult, rng):
    """`mult` times the points of the base kind."""
    if base == "n4":
        x = np.linspace(0.0, 1.0, 8 * mult)
    elif base == "n9_wide":
        x = rng.uniform(-0.3, 1.3, 200 * mult)
    elif base == "n9_cell":
        x = rng.uniform(0.0, 0.124, 40 * mult)
    elif base == "n130":
        x = np.concatenate([rng.uniform(0.0, 0.2, 300 * mult), rng.uniform(0.7, 1.0, 300 * mult)])
    else:      # "nmax": 3 points per cell, evenly spaced inside it (none half way between two nodes)
        nod, m = largest_1d_nodes(), 3 * mult
        x = (np.repeat(np.arange(nod - 1), m) + np.tile((np.arange(m) + 0.37) / m, nod - 1)) / (nod - 1)
    return x.reshape(-1, 1)


NODES_1D = {"n4": 4, "n9_wide": 9, "n9_cell": 9, "n130": 130}
SEEDS = {"n4": 7101, "n9_wide": 7102, "n9_cell": 7103, "n130": 7104, "nmax": 7105}
MULTS = (1, 3, 17)


@functools.lru_cache(maxsize=None)
def problem(name):
    """The parity problems by name.  1-D: "<base>_x<mult>" at xtrap = 1 and "n4_x1_xt0"; 2-D: "g44", "g1211", "g59", "g95", "gbox" (its own box, l1xdat = 3);
    weighted: "w_n9_wide", "w_g59" (U[0.5, 2] with 15 % exact zeros)."""
    if name.startswith("w_"):
        p = dict(problem({"w_n9_wide": "n9_wide_x1", "w_g59": "g59"}[name]))
        rng = np.random.default_rng(7300 + len(name))
        w = rng.uniform(0.5, 2.0, p["y"].size)
        w[rng.random(w.size) < 0.15] = 0.0
        w[0] = max(w[0], 0.5)      # (a first weight that is not negative: the weights count)
        p["w"] = w
        return p
    if name == "n4_x1_xt0":
        p = dict(problem("n4_x1"))
        p["xtrap"] = 0.0
        return p
    if name == "gbox":
        # a box that is not the unit box, points beyond it and away from one corner, and a third, unused row of xdata (l1xdat = 3)
        rng = np.random.default_rng(7204)
        lo, hi = [-1.25, 2.0], [3.5, 2.75]
        u = rng.uniform(-0.04, 1.04, (900, 2))
        u = u[(u[:, 0] < 0.55) | (u[:, 1] < 0.6)]
        x = np.column_stack([lo[0] + u[:, 0] * (hi[0] - lo[0]), lo[1] + u[:, 1] * (hi[1] - lo[1]), np.full(u.shape[0], 1.0e30)])
        return dict(ndim=2, nodes=(7, 6), xtrap=1.0, x=x, y=_values(u, rng), w=None, lo=lo, hi=hi)
    if name.startswith("g"):
        if name == "g44":
            rng = np.random.default_rng(7201)
            nodes, x, xtrap = (4, 4), rng.uniform(0.0, 1.0, (6, 2)), 1.0
        elif name == "g1211":
            rng = np.random.default_rng(7202)
            nodes = (12, 11) if capi.fit_many_lds_bytes(2, [12, 11]) <= LDS_BUDGET else largest_square_nodes()
            x = np.column_stack([rng.uniform(0.0, 0.4, 1500), rng.uniform(0.0, 1.0, 1500)])
            xtrap = 1.0
        else:      # "g59" and "g95": the same points with the dimensions swapped
            rng = np.random.default_rng(7203)
            x = rng.uniform(0.0, 1.0, (2000, 2))
            y = _values(x, rng)
            if name == "g95":
                return dict(ndim=2, nodes=(9, 5), xtrap=0.0, x=np.ascontiguousarray(x[:, ::-1]), y=y, w=None)
            return dict(ndim=2, nodes=(5, 9), xtrap=0.0, x=x, y=y, w=None)
        return dict(ndim=2, nodes=nodes, xtrap=xtrap, x=x, y=_values(x, rng), w=None)
    base, mult = name.rsplit("_x", 1)
    rng = np.random.default_rng(SEEDS[base] + 10 * int(mult))
    x = _points_1d(base, int(mult), rng)
    nod = largest_1d_nodes() if base == "nmax" else NODES_1D[base]
    return dict(ndim=1, nodes=(nod,), xtrap=1.0, x=x, y=_values(x, rng), w=None)


BATCHES_1D = {b: [f"{b}_x{m}" for m in MULTS] for b in SEEDS}
PARITY_NAMES = [n for b in BATCHES_1D.values() for n in b] + ["n4_x1_xt0", "g44", "g1211", "g59", "g95", "gbox", "w_n9_wide", "w_g59"]
# the problem of 40 points in one cell at xtrap = 0: N is exactly singular, the reference says 107
SINGULAR = "n9_cell_x1"


def ref_nwrk(p):
    """Scratch for the reference: its default in oracle/binding.py is below suprls' ((n + 5) n + 2) / 2 for the 4-node grid."""
    n = int(np.prod(p["nodes"]))
    return n * (n + 1) + 8 * n + 64


def lo_hi(p):
    """The box of a problem: [0, 1]^ndim unless it names its own."""
    return list(p.get("lo", [0.0] * p["ndim"])), list(p.get("hi", [1.0] * p["ndim"]))


def listed(p):
    """(x, y, w) as the reference takes them: the points of non-zero weight."""
    if p["w"] is None:
        return p["x"], p["y"], None
    keep = p["w"] != 0.0
    return p["x"][keep], p["y"][keep], p["w"][keep]


def pack(problems, empty_at=()):
    """-> (offsets, x, y, w or None) of a batch; an empty problem before every position listed in empty_at."""
    xs, ys, ws, off = [], [], [], [0]
    weighted = any(p["w"] is not None for p in problems)
    for k, p in enumerate(problems):
        if k in empty_at:
            off.append(off[-1])
        xs.append(p["x"])
        ys.append(p["y"])
        ws.append(p["w"] if p["w"] is not None else np.ones(p["y"].size))
        off.append(off[-1] + p["y"].size)
    return np.array(off, dtype=np.int64), np.concatenate(xs), np.concatenate(ys), (np.concatenate(ws) if weighted else None)


# ---------------------------------------------------------------------------------------------------------------
# The algorithm in numpy
def basis_1d(kind, deriv, x, xb, s):
    """The 1-D basis function of the reference (bascmp :231-381): kind 1 left end, 2 interior, 3 right end."""
    b = 0.0
    if kind == 2:
        if deriv == 0:
            z = abs(s * (x - xb)) - 2.0
            if z < 0.0:
                b = -0.25 * z ** 3
                if z + 1.0 < 0.0:
                    b += (z + 1.0) ** 3
        elif deriv == 1:
            u = x - xb
            f = -s if u < 0.0 else s
            z = f * u - 2.0
            if z < 0.0:
                b = -0.75 * z * z
                if z + 1.0 < 0.0:
                    b += 3.0 * (z + 1.0) ** 2
                b *= f
        else:
            z = s * abs(x - xb) - 2.0
            if z < 0.0:
                b = -1.5 * z
                if z + 1.0 < 0.0:
                    b += 6.0 * (z + 1.0)
                b *= s * s
        return b
    f = -s if kind == 1 else s
    z = f * (x - xb) + 2.0
    if deriv == 0:
        if z > 0.0:
            if z < 2.0:
                b = 0.5 * z ** 3
                if z - 1.0 > 0.0:
                    b -= (z - 1.0) ** 3
            else:
                b = 3.0 * z - 3.0
    elif deriv == 1:
        if z > 0.0:
            if z < 2.0:
                b = 1.5 * z * z
                if z - 1.0 > 0.0:
                    b -= 3.0 * (z - 1.0) ** 2
                b *= f
            else:
                b = 3.0 * f
    else:
        if abs(z - 1.0) < 1.0:
            b = 3.0 * z
            if z - 1.0 > 0.0:
                b -= 6.0 * (z - 1.0)
            b *= f * f
    return b


def _kind(ib, nod):
    return 1 if ib <= 1 else (3 if ib >= nod - 2 else 2)


class NumpyManyFit:
    """What one workgroup of csrc/fitmany.hip does for one problem, in numpy: the rows of the reference (data rows in 4-wide
    windows, the 0.75 rule, the derivative-constraint rows), the band normal equations with the smaller dimension fastest,
    Cholesky with the pivot test of the point fit, the solve, and the refinement rule of the grid fits against the rows."""

    def __init__(self, p):
        self.ndim, self.xtrap = p["ndim"], p["xtrap"]
        nodes = list(p["nodes"])
        D = self.ndim
        # internal order: ascending node counts, stable
        self.perm = sorted(range(D), key=lambda d: nodes[d])
        self.ref_nodes = nodes
        self.nod = [nodes[r] for r in self.perm]
        self.refstride = [int(np.prod(nodes[:r])) for r in self.perm]
        self.stride = [1, self.nod[0]][:D]
        self.ncol = int(np.prod(nodes))
        self.hb = 3 * self.nod[0] + 3 if D == 2 else 3
        lo, hi = lo_hi(p)
        self.ref_lo = lo
        self.ref_dx = [(hi[r] - lo[r]) / (nodes[r] - 1) for r in range(D)]
        self.lo = [lo[r] for r in self.perm]
        self.dx = [self.ref_dx[r] for r in self.perm]
        x, y, w = p["x"], p["y"], p["w"]
        weighted = w is not None and w[0] >= 0.0
        wt = np.asarray(w, dtype=np.float64) if weighted else np.ones(y.size)
        keep = wt != 0.0
        self.x, self.y, self.w = x[keep], y[keep], wt[keep]
        self.rows_data = int(keep.sum())
        self._data_rows()
        self._constraint_rows()

    def _window(self, d, xv):
        nod, s = self.nod[d], 1.0 / self.dx[d]
        it = int(s * (xv - self.lo[d]))
        lo = min(max(it - 1, 0), nod - 2)
        hi = max(min(it + 2, nod - 1), 1)
        ws = min(max(it - 1, 0), nod - 4)
        b = [basis_1d(_kind(ws + k, nod), 0, xv, self.lo[d] + (ws + k) * self.dx[d], s) if lo <= ws + k <= hi else 0.0 for k in range(4)]
        return ws, b

    def _data_rows(self):
        D, m = self.ndim, self.y.size
        nb = 4 ** D
        self.cols = np.zeros((m, nb), dtype=np.int64)
        self.vals = np.zeros((m, nb))
        for i in range(m):
            tabs = [self._window(d, self.x[i, self.perm[d]]) for d in range(D)]
            for e in range(nb):
                q = [(e >> (2 * d)) & 3 for d in range(D)]
                self.cols[i, e] = sum((tabs[d][0] + q[d]) * self.stride[d] for d in range(D))
                self.vals[i, e] = self.w[i] * np.prod([tabs[d][1][q[d]] for d in range(D)])
        self.b = self.w * self.y

    def _constraint_rows(self):
        """Dense rows C (internal column order), from the histogram of nearest nodes (:862-1046)."""
        D = self.ndim
        self.C = np.zeros((0, self.ncol))
        if self.xtrap == 0.0:
            return
        hist = np.zeros(self.ncol)      # over the caller's node numbering, as the reference's work(1:ncol)
        tot = 0.0
        for i in range(self.y.size):
            # a coordinate out of range skips ITS dimension in the Horner address; the point still counts (:899)
            addr = 0
            for r in reversed(range(D)):
                t = int((1.0 / self.ref_dx[r]) * (self.x[i, r] - self.ref_lo[r]) + 0.5)
                if 0 <= t <= self.ref_nodes[r] - 1:
                    addr = self.ref_nodes[r] * addr + t
            hist[addr] += self.w[i]
            tot += self.w[i]
        nrect = np.prod([n - 1 for n in self.nod])
        rows = []
        for node in range(self.ncol):
            inn = [node % self.nod[0], node // self.nod[0]][:D]
            expect = tot / nrect
            for d in range(D):
                if inn[d] in (0, self.nod[d] - 1):
                    expect *= 0.5
            have = self._hist_at(hist, inn)
            if not have < 0.75 * expect:
                continue
            dcw = self.xtrap * (expect - have)
            for idm in range(D):
                for jdm in range(idm, D):
                    nder = [0] * D
                    boundary, rowwt = True, 2.0 * dcw
                    if jdm == idm:
                        rowwt = dcw
                        nder[jdm] = 2
                        boundary = inn[idm] in (0, self.nod[idm] - 1)
                    if boundary:
                        nder[idm] = nder[jdm] = 1
                    row = np.zeros(self.ncol)
                    for e in range(3 ** D):
                        off = [(e // 3 ** d) % 3 - 1 for d in range(D)]
                        ib = [inn[d] + off[d] for d in range(D)]
                        if any(not 0 <= ib[d] <= self.nod[d] - 1 for d in range(D)):
                            continue
                        v = rowwt
                        for d in range(D):
                            v *= basis_1d(_kind(ib[d], self.nod[d]), nder[d], self.lo[d] + inn[d] * self.dx[d], self.lo[d] + ib[d] * self.dx[d],
                                          1.0 / self.dx[d])
                        row[sum(ib[d] * self.stride[d] for d in range(D))] = v
                    rows.append(row)
        if rows:
            self.C = np.array(rows)

    def _hist_at(self, hist, inn):
        return hist[sum(inn[d] * self.refstride[d] for d in range(self.ndim))]

    def band(self):
        """N = A^T W^2 A + C^T C in band storage [ncol, hb + 1]: entry (i, i - o) at [i, o]."""
        n, hb = self.ncol, self.hb
        B = np.zeros((n, hb + 1))
        nb = self.cols.shape[1]
        for ea in range(nb):
            for eb in range(nb):
                i, j = self.cols[:, ea], self.cols[:, eb]
                m = j <= i
                np.add.at(B, (i[m], (i - j)[m]), (self.vals[:, ea] * self.vals[:, eb])[m])
        for row in self.C:
            nz = np.nonzero(row)[0]
            for i in nz:
                for j in nz[nz <= i]:
                    B[i, i - j] += row[i] * row[j]
        return B

    def cholesky(self, B):
        """In place; -> (spd, smallest pivot): a pivot that is not positive fails, the test of the point fit."""
        n, hb = self.ncol, self.hb
        minpiv = np.inf
        for j in range(n):
            piv = B[j, 0]
            minpiv = min(minpiv, piv)
            if not piv > 0.0:
                return False, minpiv
            l = np.sqrt(piv)
            m = min(hb, n - 1 - j)
            col = np.array([B[j + t, t] for t in range(1, m + 1)]) / l
            B[j, 0] = l
            for t in range(1, m + 1):
                B[j + t, t] = col[t - 1]
            for ra in range(1, m + 1):
                B[j + ra, ra - np.arange(1, ra + 1)] -= col[ra - 1] * col[:ra]
        return True, minpiv

    def solve(self, B, v):
        n, hb = self.ncol, self.hb
        v = v.copy()
        for i in range(n):
            k = np.arange(1, min(hb, i) + 1)
            v[i] = (v[i] - B[i, k] @ v[i - k]) / B[i, 0]
        for i in range(n - 1, -1, -1):
            k = np.arange(1, min(hb, n - 1 - i) + 1)
            v[i] = (v[i] - B[i + k, k] @ v[i + k]) / B[i, 0]
        return v

    def gradient(self, xv):
        """A^T W (W y - W A x) - C^T C x from the rows -> (rho, sum of squared row residuals)."""
        e = self.b - np.einsum("ij,ij->i", self.vals, xv[self.cols])
        rho = np.zeros(self.ncol)
        np.add.at(rho, self.cols.ravel(), (self.vals * e[:, None]).ravel())
        t = self.C @ xv
        return rho - self.C.T @ t, float(e @ e + t @ t)

    def fit(self):
        """-> (coef in the caller's column order or zeros, status 0 / 107, refinement steps)."""
        B = self.band()
        spd, self.minpiv = self.cholesky(B)
        if not spd:
            return np.zeros(self.ncol), 107, 0
        rhs = np.zeros(self.ncol)
        np.add.at(rhs, self.cols.ravel(), (self.vals * self.b[:, None]).ravel())
        xv = self.solve(B, rhs)
        steps, prev, ratio, last, converged = 0, np.inf, 0.0, 0.0, False
        for it in range(30):
            rho, self.ssq = self.gradient(xv)
            dxv = self.solve(B, rho)
            xv = xv + dxv
            steps += 1
            last = np.max(np.abs(dxv)) / np.max(np.abs(xv)) if np.max(np.abs(xv)) > 0 else 0.0
            if not np.isfinite(last):
                break
            if last <= 1e-11:
                converged = True
                break
            if it >= 1:
                ratio = last / prev
                if ratio < 0.9 and last * ratio / (1.0 - ratio) <= 1e-11:
                    converged = True
                    break
                if ratio >= 0.9:
                    converged = last <= 1e-10
                    break
            prev = last
        if not converged:
            est = last * ratio / (1.0 - ratio) if steps >= 2 and 0.0 < ratio < 1.0 else last
            if not est <= 1e-10:
                return np.zeros(self.ncol), 107, steps
        out = np.zeros(self.ncol)
        for node in range(self.ncol):
            inn = [node % self.nod[0], node // self.nod[0]][:self.ndim]
            out[sum(inn[d] * self.refstride[d] for d in range(self.ndim))] = xv[node]
        return out, 0, steps


# ---------------------------------------------------------------------------------------------------------------
# CPU tier
def test_symbols_exported():
    lib = capi.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def _call(ndim=1, nbatch=1, offsets=(0, 8), x="ok", l1xdat=1, y="ok", xmin=(0.0, 0.0), xmax=(1.0, 1.0), nodes=(4, 4), ldcoef=16, coef="ok",
          status="ok"):
    """splpak_fit_many_f64 on raw arguments -> (rc, coef, status); "ok": a valid array, None: a null pointer."""
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    keep = []

    def arr(v, dt, ty):
        if v is None:
            return None
        a = np.ascontiguousarray(v, dtype=dt)
        keep.append(a)
        return a.ctypes.data_as(ty)
    cf = np.full(64, 777.0)
    st = np.full(8, -999, dtype=np.int32)
    xs = np.linspace(0.0, 1.0, 32)
    rc = capi.lib().splpak_fit_many_f64(ndim, nbatch, arr(offsets, np.int64, lp), arr(xs if x == "ok" else x, np.float64, dp), l1xdat,
                                        arr(xs if y == "ok" else y, np.float64, dp), None, arr(xmin, np.float64, dp),
                                        arr(xmax, np.float64, dp), arr(nodes, np.int32, ip), 1.0,
                                        arr(cf if coef == "ok" else coef, np.float64, dp) if coef is not None else None, ldcoef,
                                        st.ctypes.data_as(ip) if status == "ok" else None, None)
    return rc, cf, st


def test_status_ladder_in_order_before_any_device_call():
    """Every rung with every LATER rung failing too: the first failing check wins; coef and status stay as they were.  No rung
    asks for a device (the test runs where there is none)."""
    big = (1000, 1000)      # 2-D, beyond the LDS rule
    ladder = [
        (E_BADARG, dict(offsets=None, ndim=0)),
        (E_BADARG, dict(nodes=None, ndim=0)),
        (E_BADARG, dict(xmin=None, ndim=0)),
        (E_BADARG, dict(xmax=None, ndim=0)),
        (101, dict(ndim=0, nodes=(3, 3), ldcoef=0, nbatch=0)),
        (E_UNSUPPORTED, dict(ndim=3, nodes=(3, 3, 3), xmin=(0, 0, 0), xmax=(1, 1, 1), ldcoef=0, nbatch=0)),
        (E_UNSUPPORTED, dict(ndim=4, nodes=(4, 4, 4, 4), xmin=(0,) * 4, xmax=(1,) * 4)),
        (102, dict(ndim=2, nodes=(3, 4), xmax=(1.0, 0.0), ldcoef=0, nbatch=0)),
        (103, dict(ndim=2, nodes=(4, 4), xmax=(1.0, 0.0), ldcoef=0, nbatch=0)),
        (104, dict(ndim=2, nodes=big, ldcoef=999999, nbatch=0)),
        (104, dict(ndim=1, ldcoef=3, x=None)),
        (E_BADARG, dict(ndim=2, nodes=big, ldcoef=1000000, nbatch=0)),
        (E_BADARG, dict(ndim=2, nodes=big, ldcoef=1000000, l1xdat=2, offsets=(0, 8, 4), nbatch=2)),
        (E_BADARG, dict(ndim=2, nodes=big, ldcoef=1000000, l1xdat=2, offsets=(0, 1 << 31))),
        (E_BADARG, dict(ndim=2, nodes=big, ldcoef=1000000, l1xdat=1)),
        (E_BADARG, dict(ndim=2, nodes=big, ldcoef=1000000, l1xdat=2, x=None)),
        (E_BADARG, dict(ndim=2, nodes=big, ldcoef=1000000, l1xdat=2, y=None)),
        (E_BADARG, dict(ndim=2, nodes=big, ldcoef=1000000, l1xdat=2, coef=None)),
        (E_UNSUPPORTED, dict(ndim=2, nodes=big, ldcoef=1000000, l1xdat=2)),
    ]
    for want, kw in ladder:
        rc, cf, st = _call(**kw)
        assert rc == want, (want, rc, kw)
        assert np.all(cf == 777.0) and np.all(st == -999), kw
    # a batch of empty problems alone is answered on the host as well: 105 each, coefficients untouched
    rc, cf, st = _call(nbatch=2, offsets=(5, 5, 5))
    assert rc == 105 and list(st[:2]) == [105, 105] and np.all(cf == 777.0)
    assert capi.debug_fit_many_stats()[2:5] == (0, 0, 2)
    rc, _, _ = _call(ndim=2, nodes=big, ldcoef=1000000, l1xdat=2)
    assert "loop" in capi.last_error()


def test_lds_bytes_rule():
    f = capi.fit_many_lds_bytes
    assert f(2, [5, 9]) == f(2, [9, 5])
    prev = 0
    for n in range(4, 40):      # monotone in the node counts
        assert f(1, [n]) > prev
        prev = f(1, [n])
        assert f(2, [n, 7]) < f(2, [n + 1, 7]) and f(2, [7, n]) < f(2, [7, n + 1])
    for bad in ((0, [4]), (3, [4, 4, 4]), (1, [3]), (2, [4, 3])):
        assert capi.lib().splpak_fit_many_lds_bytes(bad[0], np.array(bad[1], dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))) == E_BADARG
    # both sides of the frontier agree with the ladder's decision (decided on the host: the admitted side asks for a device
    # only after the ladder, so it is probed with a batch of empty problems)
    nmax = largest_1d_nodes()
    assert f(1, [nmax]) <= LDS_BUDGET < f(1, [nmax + 1])
    assert _call(nodes=(nmax,), ldcoef=nmax + 1, offsets=(0, 0))[0] == 105
    assert _call(nodes=(nmax + 1,), ldcoef=nmax + 1, offsets=(0, 0))[0] == E_UNSUPPORTED
    a, b = largest_square_nodes()
    assert f(2, [a, b]) <= LDS_BUDGET < f(2, [a + 1, b + 1])
    assert _call(ndim=2, nodes=(a, b), ldcoef=a * b, l1xdat=2, offsets=(0, 0))[0] == 105
    assert _call(ndim=2, nodes=(a + 1, b + 1), ldcoef=(a + 1) * (b + 1), l1xdat=2, offsets=(0, 0))[0] == E_UNSUPPORTED


@pytest.mark.parametrize("name", PARITY_NAMES)
def test_numpy_restatement_matches_recorded_reference(name):
    """The algebra without a GPU: band normal equations with the constraint rows, Cholesky, refinement."""
    gold = load_golden("fit_many_ref")
    p = problem(name)
    c, status, steps = NumpyManyFit(p).fit()
    assert status == 0 and int(gold["ierror_" + name]) == 0
    err = relmax(c, gold["coef_" + name])
    print(f"{name}: numpy restatement vs recorded reference {err:.2e}, refinement steps {steps}")
    assert err <= BAR


def test_numpy_restatement_says_107_where_the_reference_does():
    p = dict(problem(SINGULAR))
    p["xtrap"] = 0.0
    gold = load_golden("fit_many_ref")
    assert int(gold["ierror_singular"]) == 107
    assert NumpyManyFit(p).fit()[1] == 107
    three = dict(problem("n4_x1_xt0"))
    three["x"], three["y"] = three["x"][:3], three["y"][:3]
    assert int(gold["ierror_three"]) == 107
    assert NumpyManyFit(three).fit()[1] == 107


# ---------------------------------------------------------------------------------------------------------------
# GPU tier
def recorded(name):
    return load_golden("fit_many_ref")["coef_" + name]


def run_batch(names, empty_at=(), xtrap=None, **kw):
    ps = [problem(n) for n in names]
    off, x, y, w = pack(ps, empty_at)
    p0 = ps[0]
    lo, hi = lo_hi(p0)
    return capi.fit_many(p0["ndim"], off, x, y, w, lo, hi, list(p0["nodes"]), p0["xtrap"] if xtrap is None else xtrap, **kw)


def rows_of(names, empty_at):
    """Row of `coef` of every problem of a packed batch."""
    rows, k = [], 0
    for i in range(len(names)):
        if i in empty_at:
            k += 1
        rows.append(k)
        k += 1
    return rows


def check_parity(name, c, reference):
    err = relmax(c, recorded(name))
    print(f"{name}: vs recorded reference {err:.2e}")
    assert err <= BAR, name
    p = problem(name)
    x, y, w = listed(p)
    if reference is not None and float(np.prod(p["nodes"])) ** 2 * y.size <= LIVE_WORK:
        lo, hi = lo_hi(p)
        c_ref, rc, _ = reference.fit(p["ndim"], x, y, w, lo, hi, list(p["nodes"]), p["xtrap"], nwrk=ref_nwrk(p))
        assert rc == 0
        live = relmax(c, c_ref[:c.size])
        print(f"{name}: vs the live reference {live:.2e}")
        assert live <= BAR, name


def check_against_single_fit(name, c, st, info):
    """The library's own single fit: same status, same row counts, 1e-10."""
    p = problem(name)
    lo, hi = lo_hi(p)
    c1, rc1, _, info1 = capi.fit(p["ndim"], p["x"], p["y"], p["w"], lo, hi, list(p["nodes"]), p["xtrap"])
    assert rc1 == st == 0
    assert info1[0] == info[0] and info1[1] == info[1], (name, info1[:2], info[:2])
    d = relmax(c, c1)
    print(f"{name}: vs splpak_fit_f64 {d:.2e}, rows {info[0]:.0f} + {info[1]:.0f}, steps {info[2]:.0f}, reserr {info[8]:.3e} / {info1[8]:.3e}")
    assert d <= BAR
    assert abs(info[8] - info1[8]) <= 1e-5 * info1[8] + 1e-9 * np.max(np.abs(p["y"]))


@pytest.mark.gpu
@pytest.mark.parametrize("base", list(BATCHES_1D))
def test_1d_ragged_batch_matches_reference_and_single_fit(reference, base):
    """One call per grid: the 1-, 3- and 17-fold problems in shuffled order with an empty problem among them."""
    names = [BATCHES_1D[base][i] for i in (2, 0, 1)]
    coef, rc, st, info = run_batch(names, empty_at=(1,))
    rows = rows_of(names, (1,))
    assert rc == 105 and st[1] == 105 and np.all(coef[1] == 0.0) and np.all(info[1] == 0.0)
    for name, k in zip(names, rows):
        assert st[k] == 0, (name, st)
        check_parity(name, coef[k], reference)
        check_against_single_fit(name, coef[k], st[k], info[k])
    stats = capi.debug_fit_many_stats()
    assert stats[2] == 1 and stats[3] == 3 and stats[4] == 1 and stats[1] == capi.fit_many_lds_bytes(1, list(problem(names[0])["nodes"]))


@pytest.mark.gpu
def test_both_sides_of_the_one_wave_threshold(reference):
    """Grids of up to 64 nodes run in workgroups of one wave, larger ones in four: 64 and 65 nodes, 300 points with a hole, against
    the library's single fit and, where it is built, the reference."""
    rng = np.random.default_rng(7400)
    x = np.concatenate([rng.uniform(-0.05, 0.45, 150), rng.uniform(0.6, 1.05, 150)]).reshape(-1, 1)
    y = _values(x, rng)
    for nod in (64, 65):
        coef, rc, st, info = capi.fit_many(1, [0, 0, 300], x, y, None, [0.0], [1.0], [nod], 1.0)
        c1, rc1, _, info1 = capi.fit(1, x, y, None, [0.0], [1.0], [nod], 1.0)
        assert rc == 105 and list(st) == [105, 0] and rc1 == 0
        assert info[1, 0] == info1[0] == 300 and info[1, 1] == info1[1] > 0
        d = relmax(coef[1], c1)
        print(f"{nod} nodes: vs splpak_fit_f64 {d:.2e}, {capi.debug_fit_many_stats()}")
        assert d <= BAR
        if reference is not None:
            c_ref, rc_ref, _ = reference.fit(1, x, y, None, [0.0], [1.0], [nod], 1.0, nwrk=nod * (nod + 1) + 8 * nod + 64)
            live = relmax(coef[1], c_ref[:nod])
            print(f"{nod} nodes: vs the live reference {live:.2e}")
            assert rc_ref == 0 and live <= BAR


@pytest.mark.gpu
def test_1d_xtrap0_eight_points_fit_and_three_points_fail(reference):
    coef, rc, st, info = run_batch(["n4_x1_xt0"])
    assert rc == 0 and st[0] == 0 and info[0, 1] == 0
    check_parity("n4_x1_xt0", coef[0], reference)
    check_against_single_fit("n4_x1_xt0", coef[0], st[0], info[0])
    p = problem("n4_x1_xt0")
    coef, rc, st, _ = capi.fit_many(1, [0, 3], p["x"][:3], p["y"][:3], None, [0.0], [1.0], [4], 0.0)
    assert rc == 107 and st[0] == 107 and np.all(coef[0] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["g44", "g1211", "g59", "g95", "gbox"])
def test_2d_matches_reference_and_single_fit(reference, name):
    coef, rc, st, info = run_batch([name], empty_at=(0,))
    assert rc == 105 and list(st) == [105, 0]
    check_parity(name, coef[1], reference)
    check_against_single_fit(name, coef[1], st[1], info[1])
    if name in ("g1211", "gbox"):
        assert info[1, 1] > 0      # data-sparse nodes on a boundary and in a corner: constraint rows


@pytest.mark.gpu
def test_2d_swapped_dimensions_give_transposed_coefficients():
    a = run_batch(["g59"])[0][0].reshape(9, 5)      # (n2, n1), first dimension fastest
    b = run_batch(["g95"])[0][0].reshape(5, 9)
    assert relmax(b, a.T) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["w_n9_wide", "w_g59"])
def test_weights_with_exact_zeros(reference, name):
    """U[0.5, 2] with 15 % exact zeros: the fit of the listed points of non-zero weight."""
    p = problem(name)
    coef, rc, st, info = run_batch([name])
    assert rc == 0 and info[0, 0] == np.count_nonzero(p["w"])
    check_parity(name, coef[0], reference)
    x, y, w = listed(p)
    lo, hi = lo_hi(p)
    c2, rc2, st2, _ = capi.fit_many(p["ndim"], [0, y.size], x, y, w, lo, hi, list(p["nodes"]), p["xtrap"])
    assert rc2 == 0 and relmax(coef[0], c2[0]) <= BAR
    check_against_single_fit(name, coef[0], st[0], info[0])


@pytest.mark.gpu
def test_negative_first_weight_means_no_weights_for_that_problem_alone():
    a, b, c = dict(problem("w_n9_wide")), dict(problem("w_n9_wide")), dict(problem("w_n9_wide"))
    b["w"] = b["w"].copy()
    b["w"][0] = -1.0
    off, x, y, w = pack([a, b, c])
    coef, rc, st, info = capi.fit_many(1, off, x, y, w, [0.0], [1.0], [9], 1.0)
    assert rc == 0
    unweighted = dict(b)
    unweighted["w"] = None
    off1, x1, y1, _ = pack([unweighted])
    c_un = capi.fit_many(1, off1, x1, y1, None, [0.0], [1.0], [9], 1.0)[0][0]
    assert np.array_equal(coef[1], c_un) and info[1, 0] == y1.size
    alone = run_batch(["w_n9_wide"])[0][0]
    assert np.array_equal(coef[0], alone) and np.array_equal(coef[2], alone)
    assert not np.array_equal(coef[0], coef[1])


@pytest.mark.gpu
def test_a_failure_stays_local():
    good, bad = problem("n9_wide_x1"), problem(SINGULAR)
    off, x, y, _ = pack([good, bad, good])
    coef, rc, st, _ = capi.fit_many(1, off, x, y, None, [0.0], [1.0], [9], 0.0)
    assert rc == 107 and list(st) == [0, 107, 0]
    assert np.all(coef[1] == 0.0)
    alone = capi.fit_many(1, [0, good["y"].size], good["x"], good["y"], None, [0.0], [1.0], [9], 0.0)[0][0]
    assert np.array_equal(coef[0], coef[2]) and np.array_equal(coef[0], alone)
    assert "problem 1" in capi.last_error()


@pytest.mark.gpu
def test_bits_do_not_depend_on_the_batch_the_position_or_the_entry():
    import torch
    names = ["n9_wide_x3", "n9_cell_x1", "n9_wide_x1", "n9_cell_x17"]
    ps = [problem(n) for n in names]
    off, x, y, _ = pack(ps)
    coef, rc, st, _ = capi.fit_many(1, off, x, y, None, [0.0], [1.0], [9], 1.0)
    assert rc == 0
    again = capi.fit_many(1, off, x, y, None, [0.0], [1.0], [9], 1.0)[0]
    assert np.array_equal(coef, again)
    for k, p in enumerate(ps):
        alone = capi.fit_many(1, [0, p["y"].size], p["x"], p["y"], None, [0.0], [1.0], [9], 1.0)[0][0]
        assert np.array_equal(alone, coef[k]), names[k]
    off2, x2, y2, _ = pack(ps[::-1], empty_at=(2,))
    c2 = capi.fit_many(1, off2, x2, y2, None, [0.0], [1.0], [9], 1.0)[0]
    for k, row in enumerate(rows_of(names, (2,))):
        assert np.array_equal(c2[row], coef[len(ps) - 1 - k])
    # the _dev entry
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    cd = torch.zeros((len(ps), 9), dtype=torch.float64, device="cuda")
    rc, st, _ = capi.fit_many_dev(1, off, xd, yd, None, [0.0], [1.0], [9], cd, xtrap=1.0)
    assert rc == 0 and np.array_equal(cd.cpu().numpy(), coef)
    # REAL32 storage: the f64 entry on the widened inputs, rounded once
    x32, y32 = x.astype(np.float32), y.astype(np.float32)
    c32 = capi.fit_many(1, off, x32, y32, None, [0.0], [1.0], [9], 1.0, real32=True)[0]
    c64 = capi.fit_many(1, off, x32.astype(np.float64), y32.astype(np.float64), None, [0.0], [1.0], [9], 1.0)[0]
    assert c32.dtype == np.float32 and np.array_equal(c32, c64.astype(np.float32))
    # two dimensions, weights, the _dev entry with a padded ldcoef
    p = problem("w_g59")
    c_h = capi.fit_many(2, [0, 0, p["y"].size], p["x"], p["y"], p["w"], [0.0, 0.0], [1.0, 1.0], [5, 9], 0.0)[0]
    cd = torch.full((2, 50), 7.0, dtype=torch.float64, device="cuda")
    rc, st, _ = capi.fit_many_dev(2, [0, 0, p["y"].size], torch.from_numpy(p["x"]).cuda(), torch.from_numpy(p["y"]).cuda(),
                                  torch.from_numpy(p["w"]).cuda(), [0.0, 0.0], [1.0, 1.0], [5, 9], cd, ldcoef=50)
    out = cd.cpu().numpy()
    assert rc == 105 and list(st) == [105, 0] and np.all(out[0] == 7.0) and np.all(out[1, 45:] == 7.0)
    assert np.array_equal(out[1, :45], c_h[1])


@pytest.mark.gpu
def test_persistent_loop_gives_every_copy_the_same_bits():
    a, b = problem("n4_x1"), dict(problem("n4_x1"))
    xb = np.linspace(0.0, 1.0, 9).reshape(-1, 1)
    b["x"], b["y"] = xb, np.sin(3.0 * xb[:, 0])
    capi.fit_many(1, [0, 8], a["x"], a["y"], None, [0.0], [1.0], [4], 1.0)
    one = capi.debug_fit_many_stats()
    off, x, y, _ = pack([a, b] * 4096)
    capi.fit_many(1, off, x, y, None, [0.0], [1.0], [4], 1.0)
    wg = capi.debug_fit_many_stats()[0]      # what a large call launches
    assert one[0] == 1 and 1 <= wg < 8192
    ncopy = 3 * wg + 1
    off, x, y, _ = pack(([a, b] * ((ncopy + 1) // 2))[:ncopy])
    coef, rc, st, _ = capi.fit_many(1, off, x, y, None, [0.0], [1.0], [4], 1.0)
    stats = capi.debug_fit_many_stats()
    assert rc == 0 and not st.any()
    assert stats[0] == wg and stats[2] == one[2] == 1 and stats[3] == ncopy
    assert np.all(coef[0::2] == coef[0]) and np.all(coef[1::2] == coef[1]) and not np.array_equal(coef[0], coef[1])


FDIR = os.path.join(ROOT, "splpak_amd", "fortran")
PROG = os.path.join(FDIR, "build", "test_fit_many")


@pytest.mark.gpu
def test_fortran_initialize_many_matches_initialize():
    if not os.path.exists(PROG):
        if not os.path.exists("/opt/rocm/bin/amdflang"):
            pytest.skip("amdflang not available")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "splpak_amd", "csrc")])
        subprocess.check_call(["make", "-C", FDIR])
    r = subprocess.run([PROG], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS test_fit_many" in r.stdout
