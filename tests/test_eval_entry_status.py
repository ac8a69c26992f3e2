"""CPU: the argument ladder of the seven point / derivative evaluation entries of the C ABI, and (second half) of the
sixteen grid, grid-derivatives, integral and fields entries.

Every case returns before the library asks for a device, so the statuses, the error text of an argument
error and the elements of `out` a host entry zeroes are decided on the host.  The device entries get null
data pointers throughout (nothing is dereferenced).  EXPECTED was recorded from the library as it stood
before the entries moved out of plan.hip into evalapi.hip; the entries differ from one another in places
(where ndim > 4 is caught, whether ndim < 1 zeroes an output) and the table keeps those differences."""
import ctypes as C

import numpy as np
import pytest

from splpak_amd import capi

EVAL = ("splpak_eval_f64", "splpak_eval_f32", "splpak_eval_dev_f64", "splpak_eval_dev_f32")
DERIVS = ("splpak_eval_derivs_f64", "splpak_eval_derivs_f32", "splpak_eval_derivs_dev_f64")
NOUT = 8          # elements of the pre-filled output buffer

# name -> (entries it applies to, overrides of the base call).  Base: ndim 2, nodes 8 x 8 on [0, 1]^2, two queries,
# ldxq 2, nderiv (0, 0), order 1, ldout 3 = 1 + ndim; the host entries get valid arrays for everything not in `null`.
CASES = {
    "null_nodes": (EVAL + DERIVS, dict(null={"nodes"})),
    "null_xmin": (EVAL + DERIVS, dict(null={"xmin"})),
    "null_xmax": (EVAL + DERIVS, dict(null={"xmax"})),
    "ndim_0": (EVAL + DERIVS, dict(ndim=0)),
    "ndim_5": (EVAL + DERIVS, dict(ndim=5)),
    "nodes_3": (EVAL + DERIVS, dict(nodes0=3)),
    "xmax_le_xmin": (EVAL + DERIVS, dict(xmax1=0.0)),
    "nderiv_3_nq_0": (EVAL, dict(nderiv0=3, nq=0)),
    # (with a query list the host entries would go on to the device: the null xq stops them behind the 104)
    "nderiv_3_nq_1_null_xq": (EVAL, dict(nderiv0=3, nq=1, null={"xq"})),
    "nderiv_3_nodes_3": (EVAL, dict(nderiv0=3, nodes0=3)),
    "order_0": (DERIVS, dict(order=0, nq=1)),
    "order_3": (DERIVS, dict(order=3, nq=1)),
    "order_3_nq_0": (DERIVS, dict(order=3, nq=0)),
    "nq_0": (EVAL + DERIVS, dict(nq=0)),
    "nq_0_null_data": (EVAL + DERIVS, dict(nq=0, null={"xq", "coef", "out"})),
    "null_xq": (EVAL + DERIVS, dict(nq=1, null={"xq"})),
    "null_coef": (EVAL + DERIVS, dict(nq=1, null={"coef"})),
    "null_out": (EVAL + DERIVS, dict(nq=1, null={"out"})),
    "ldxq_1": (EVAL + DERIVS, dict(ldxq=1)),
    "ldxq_1_nq_0": (EVAL + DERIVS, dict(ldxq=1, nq=0)),
    "ldout_2": (DERIVS, dict(ldout=2)),
    "ldout_2_nodes_3": (DERIVS, dict(ldout=2, nodes0=3)),
    "ldout_0_nodes_3": (DERIVS, dict(ldout=0, nodes0=3)),
}


def _call(entry, ov):
    """One call -> (status, error text for an argument error else '', indices of `out` that were zeroed)."""
    L = capi.lib()
    f32, dev, der = entry.endswith("f32"), "_dev_" in entry, "derivs" in entry
    dt, rp = (np.float32, C.POINTER(C.c_float)) if f32 else (np.float64, C.POINTER(C.c_double))
    null = ov.get("null", set())
    ndim, nq, ldxq = ov.get("ndim", 2), ov.get("nq", 2), ov.get("ldxq", 2)
    nodes = np.full(8, 8, dtype=np.int32)
    nodes[0] = ov.get("nodes0", 8)
    xmin, xmax = np.zeros(8, dtype=dt), np.ones(8, dtype=dt)
    xmax[1] = ov.get("xmax1", 1.0)
    nderiv = np.zeros(8, dtype=np.int32)
    nderiv[0] = ov.get("nderiv0", 0)
    xq, coef = np.full(16, 0.5, dtype=dt), np.ones(64, dtype=dt)
    out = np.full(NOUT, 7.0, dtype=dt)
    ptr = lambda name, a, ty: None if name in null else a.ctypes.data_as(ty)
    data = lambda name, a: None if dev else ptr(name, a, rp)
    grid = (ptr("xmin", xmin, rp), ptr("xmax", xmax, rp), ptr("nodes", nodes, C.POINTER(C.c_int32)))
    if der:
        args = [ndim, nq, data("xq", xq), ldxq, ov.get("order", 1), data("coef", coef), *grid, data("out", out), ov.get("ldout", 3)]
    else:
        args = [ndim, nq, data("xq", xq), ldxq, nderiv.ctypes.data_as(C.POINTER(C.c_int32)), data("coef", coef), *grid, data("out", out)]
    if dev:
        args.append(None)          # stream
    rc = int(getattr(L, entry)(*args))
    msg = capi.last_error() if rc == capi.E_BADARG else ""
    return rc, msg, tuple(int(i) for i in np.flatnonzero(out == 0))


def observe():
    return {(name, entry): _call(entry, ov) for name, (entries, ov) in CASES.items() for entry in entries}


NULLARG, LDXQ, ORDER, LDBOTH = ("null argument", "ldxq smaller than ndim",
                                "order must be 1 (gradient) or 2 (gradient and Hessian)", "ldxq or ldout too small")
EXPECTED = {}     # filled below: (case, entry) -> (status, error text, zeroed indices)


def _expect(case, entries, rc, msg="", zeroed=()):
    for e in entries:
        EXPECTED[(case, e)] = (rc, msg, tuple(zeroed))


HOST_EVAL, DEV_EVAL = EVAL[:2], EVAL[2:]
HOST_DERIVS, DEV_DERIVS = DERIVS[:2], DERIVS[2:]
ALL = EVAL + DERIVS
_expect("null_nodes", ALL, capi.E_BADARG, NULLARG)
_expect("null_xmin", ALL, capi.E_BADARG, NULLARG)
_expect("null_xmax", ALL, capi.E_BADARG, NULLARG)
_expect("ndim_0", ALL, 101)
_expect("ndim_5", ALL, capi.E_UNSUPPORTED)
for _case, _rc in (("nodes_3", 102), ("xmax_le_xmin", 103)):
    _expect(_case, HOST_EVAL, _rc, zeroed=(0, 1))                      # nq outputs
    _expect(_case, HOST_DERIVS, _rc, zeroed=(0, 1, 2, 3, 4, 5))        # nq * ldout
    _expect(_case, DEV_EVAL + DEV_DERIVS, _rc)
_expect("nderiv_3_nq_0", EVAL, 104)
_expect("nderiv_3_nq_1_null_xq", EVAL, capi.E_BADARG, NULLARG)
_expect("nderiv_3_nodes_3", HOST_EVAL, 102, zeroed=(0, 1))
_expect("nderiv_3_nodes_3", DEV_EVAL, 102)
_expect("order_0", DERIVS, capi.E_BADARG, ORDER)
_expect("order_3", DERIVS, capi.E_BADARG, ORDER)
_expect("order_3_nq_0", DERIVS, capi.E_BADARG, ORDER)
_expect("nq_0", ALL, 0)
_expect("nq_0_null_data", ALL, 0)
_expect("null_xq", ALL, capi.E_BADARG, NULLARG)
_expect("null_coef", ALL, capi.E_BADARG, NULLARG)
_expect("null_out", ALL, capi.E_BADARG, NULLARG)
_expect("ldxq_1", HOST_EVAL, capi.E_BADARG, LDXQ)
_expect("ldxq_1", DEV_EVAL, capi.E_BADARG, NULLARG)                   # (their data pointers are null here, and that check comes first)
_expect("ldxq_1", DERIVS, capi.E_BADARG, LDBOTH)
_expect("ldxq_1_nq_0", EVAL, 0)                                        # the value entries look at ldxq only when there are queries,
_expect("ldxq_1_nq_0", DERIVS, capi.E_BADARG, LDBOTH)                  # the derivative entries before they look at nq
_expect("ldout_2", DERIVS, capi.E_BADARG, LDBOTH)
_expect("ldout_2_nodes_3", HOST_DERIVS, 102, zeroed=(0, 1, 2, 3))
_expect("ldout_2_nodes_3", DEV_DERIVS, 102)
_expect("ldout_0_nodes_3", DERIVS, 102)


def test_table_covers_every_case():
    assert set(EXPECTED) == {(name, e) for name, (entries, _) in CASES.items() for e in entries}


@pytest.mark.parametrize("entry", ALL)
def test_entry_ladder(entry):
    for name, (entries, ov) in CASES.items():
        if entry in entries:
            assert _call(entry, ov) == EXPECTED[(name, entry)], (name, entry)


# ---- the sixteen entries over a tensor grid of points and over several fields --------------------------------------------
# GRID_EXPECTED was recorded from the library as it stood before the three grid ladders of evalapi.hip got a shared opening
# and close.  The per-family tests (test_eval_grid.py, test_eval_grid_derivs.py, test_integrate_grid.py, test_eval_fields.py)
# pin what the Python wrappers can reach on the host form; here every rung is taken on the raw entries, host and device form,
# with the pairs that fix the order of neighbouring rungs.
def _four(stem):
    return (f"{stem}_f64", f"{stem}_f32", f"{stem}_dev_f64", f"{stem}_dev_f32")


GRID, GDER, INTG, FLDS = (_four("splpak_eval_grid"), _four("splpak_eval_grid_derivs"), _four("splpak_integrate_grid"),
                          _four("splpak_eval_fields"))
COUNTED = GRID + GDER + INTG      # the entries with a count array
GALL = COUNTED + FLDS
GNOUT = 40        # elements of the pre-filled output buffer

# Base: ndim 2, nodes 8 x 8 on [0, 1]^2.  Grid entries: 2 x 2 points (cells, all integrated), nderiv (0, 0), order 1 with
# ldout 6 = 4 points + 2.  Fields: two queries, ldxq 2, two fields, ldcoef 64, ldout 3 = 2 queries + 1.  `empty` sets the
# first count (nq) to 0, `ldout_low` sets ldout to one below the point count.
GRID_CASES = {
    "null_npts": (COUNTED, dict(null={"npts"})),
    "null_npts_ndim_0": (COUNTED, dict(null={"npts"}, ndim=0)),
    "null_nodes": (GALL, dict(null={"nodes"})),
    "null_xmin": (GALL, dict(null={"xmin"})),
    "null_nodes_ndim_0": (GALL, dict(null={"nodes"}, ndim=0)),
    "ndim_0": (GALL, dict(ndim=0)),
    "ndim_0_null_out": (GALL, dict(ndim=0, null={"out"})),
    "ndim_0_negative_count": (COUNTED, dict(ndim=0, npts0=-1)),
    "ndim_5": (GALL, dict(ndim=5)),
    "negative_count": (COUNTED, dict(npts0=-1)),
    "count_beyond_int64": (COUNTED, dict(npts0=1 << 62, npts1=4)),
    "negative_count_nodes_3": (COUNTED, dict(npts0=-1, nodes0=3)),
    "mode_2": (INTG, dict(mode0=2)),
    "mode_2_nodes_3": (INTG, dict(mode0=2, nodes0=3)),
    "order_0": (GDER, dict(order=0)),
    "order_3": (GDER, dict(order=3)),
    "order_3_negative_count": (GDER, dict(order=3, npts0=-1)),
    "order_3_nodes_3": (GDER, dict(order=3, nodes0=3)),
    "ldout_low": (GDER + FLDS, dict(ldout_low=True)),
    "ldout_low_order_3": (GDER, dict(ldout_low=True, order=3)),
    "ldout_low_nodes_3": (GDER + FLDS, dict(ldout_low=True, nodes0=3)),
    "nodes_3": (GALL, dict(nodes0=3)),
    "nodes_3_order_2": (GDER, dict(nodes0=3, order=2)),
    "xmax_le_xmin": (GALL, dict(xmax1=0.0)),
    "nodes_3_null_out": (GALL, dict(nodes0=3, null={"out"})),
    "nderiv_3_empty": (GRID + FLDS, dict(nderiv0=3, empty=True)),
    "nderiv_3_nodes_3": (GRID + FLDS, dict(nderiv0=3, nodes0=3)),
    "empty": (GALL, dict(empty=True)),
    "empty_null_data": (GALL, dict(empty=True, null={"axes", "coef", "out"})),
    "empty_nodes_3": (GALL, dict(empty=True, nodes0=3)),
    "null_axes": (GALL, dict(null={"axes"})),
    "null_coef": (GALL, dict(null={"coef"})),
    "null_out": (GALL, dict(null={"out"})),
}


def _grid_call(entry, ov):
    """One call -> (status, error text for an argument error else '', indices of `out` that were zeroed)."""
    L = capi.lib()
    f32, dev = entry.endswith("f32"), "_dev_" in entry
    fam = "F" if "fields" in entry else "I" if "integrate" in entry else "D" if "grid_derivs" in entry else "G"
    dt, rp = (np.float32, C.POINTER(C.c_float)) if f32 else (np.float64, C.POINTER(C.c_double))
    ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    null = ov.get("null", set())
    ndim = ov.get("ndim", 2)
    nodes = np.full(8, 8, dtype=np.int32)
    nodes[0] = ov.get("nodes0", 8)
    xmin, xmax = np.zeros(8, dtype=dt), np.ones(8, dtype=dt)
    xmax[1] = ov.get("xmax1", 1.0)
    nderiv = np.zeros(8, dtype=np.int32)
    nderiv[0] = ov.get("nderiv0", 0)
    mode = np.ones(8, dtype=np.int32)
    mode[0] = ov.get("mode0", 1)
    npts = np.full(8, 2, dtype=np.int64)
    npts[0] = 0 if ov.get("empty") else ov.get("npts0", 2)
    npts[1] = ov.get("npts1", 2)
    axes, coef = np.full(16, 0.5, dtype=dt), np.ones(128, dtype=dt)
    out = np.full(GNOUT, 7.0, dtype=dt)
    ptr = lambda name, a, ty: None if name in null else a.ctypes.data_as(ty)
    data = lambda name, a: None if dev else ptr(name, a, rp)
    grid = (ptr("xmin", xmin, rp), ptr("xmax", xmax, rp), ptr("nodes", nodes, ip))
    if fam == "F":
        nq = 0 if ov.get("empty") else 2
        args = [ndim, nq, data("axes", axes), 2, nderiv.ctypes.data_as(ip), 2, data("coef", coef), 64, *grid, data("out", out),
                1 if ov.get("ldout_low") else 3]
    elif fam == "G":
        args = [ndim, ptr("npts", npts, lp), data("axes", axes), nderiv.ctypes.data_as(ip), data("coef", coef), *grid, data("out", out)]
    elif fam == "I":
        args = [ndim, ptr("npts", npts, lp), mode.ctypes.data_as(ip), data("axes", axes), data("coef", coef), *grid, data("out", out)]
    else:
        args = [ndim, ptr("npts", npts, lp), data("axes", axes), ov.get("order", 1), data("coef", coef), *grid, data("out", out),
                3 if ov.get("ldout_low") else 6]
    if dev:
        args.append(None)          # stream
    rc = int(getattr(L, entry)(*args))
    msg = capi.last_error() if rc == capi.E_BADARG else ""
    return rc, msg, tuple(int(i) for i in np.flatnonzero(out == 0))


def grid_observe():
    return {(name, entry): _grid_call(entry, ov) for name, (entries, ov) in GRID_CASES.items() for entry in entries}


GRID_EXPECTED = {}     # filled below: (case, entry) -> (status, error text, zeroed indices)


def _gexpect(case, entries, rc, msg="", zeroed=()):
    for e in entries:
        GRID_EXPECTED[(case, e)] = (rc, msg, tuple(zeroed))


def _host(*families):
    return tuple(e for f in families for e in f[:2])


def _dev(*families):
    return tuple(e for f in families for e in f[2:])


BADCOUNT, BADCELL, LDPLANES, FIELDARGS = ("negative npts, or an output count beyond int64",
                                          "negative ncell, a mode outside 0 and 1, or an output count beyond int64",
                                          "ldout smaller than the number of grid points, or the planes beyond int64",
                                          "nfields < 1, nq < 0 or ldout smaller than nq")
POINTS = (0, 1, 2, 3)                                        # the 2 x 2 results
PLANES_3 = tuple(6 * e + i for e in range(3) for i in range(4))      # the results of the three planes of order 1, ldout 6: the gaps stay
PLANES_6 = tuple(6 * e + i for e in range(6) for i in range(4))
FIELDS_2 = (0, 1, 3, 4)                                      # the two results of both fields, ldout 3
for _case in ("null_npts", "null_npts_ndim_0"):             # the count array is looked at first
    _gexpect(_case, COUNTED, capi.E_BADARG, NULLARG)
for _case in ("null_nodes", "null_xmin", "null_nodes_ndim_0"):
    _gexpect(_case, GALL, capi.E_BADARG, NULLARG)
_gexpect("ndim_0", _host(GRID, GDER, INTG), 101, zeroed=(0,))         # the one output of the empty product
_gexpect("ndim_0", _host(FLDS), 101, zeroed=FIELDS_2)
_gexpect("ndim_0", _dev(GRID, GDER, INTG, FLDS), 101)
_gexpect("ndim_0_null_out", GALL, 101)
_gexpect("ndim_0_negative_count", _host(GRID, GDER, INTG), 101, zeroed=(0,))      # ndim comes before the counts
_gexpect("ndim_0_negative_count", _dev(GRID, GDER, INTG), 101)
_gexpect("ndim_5", GALL, capi.E_UNSUPPORTED)
for _case in ("negative_count", "count_beyond_int64", "negative_count_nodes_3"):      # the counts come before 102
    _gexpect(_case, GRID + GDER, capi.E_BADARG, BADCOUNT)
    _gexpect(_case, INTG, capi.E_BADARG, BADCELL)
_gexpect("mode_2", INTG, capi.E_BADARG, BADCELL)
_gexpect("mode_2_nodes_3", INTG, capi.E_BADARG, BADCELL)
_gexpect("order_0", GDER, capi.E_BADARG, ORDER)
_gexpect("order_3", GDER, capi.E_BADARG, ORDER)
_gexpect("order_3_negative_count", GDER, capi.E_BADARG, BADCOUNT)      # counts, then order, then ldout, then 102
_gexpect("order_3_nodes_3", GDER, capi.E_BADARG, ORDER)
_gexpect("ldout_low_order_3", GDER, capi.E_BADARG, ORDER)
for _case in ("ldout_low", "ldout_low_nodes_3"):
    _gexpect(_case, GDER, capi.E_BADARG, LDPLANES)
    _gexpect(_case, FLDS, capi.E_BADARG, FIELDARGS)
for _case, _rc in (("nodes_3", 102), ("xmax_le_xmin", 103)):
    _gexpect(_case, _host(GRID, INTG), _rc, zeroed=POINTS)
    _gexpect(_case, _host(GDER), _rc, zeroed=PLANES_3)
    _gexpect(_case, _host(FLDS), _rc, zeroed=FIELDS_2)
    _gexpect(_case, _dev(GRID, GDER, INTG, FLDS), _rc)
_gexpect("nodes_3_order_2", _host(GDER), 102, zeroed=PLANES_6)
_gexpect("nodes_3_order_2", _dev(GDER), 102)
_gexpect("nodes_3_null_out", GALL, 102)
_gexpect("nderiv_3_empty", GRID + FLDS, 104)
_gexpect("nderiv_3_nodes_3", _host(GRID), 102, zeroed=POINTS)
_gexpect("nderiv_3_nodes_3", _host(FLDS), 102, zeroed=FIELDS_2)
_gexpect("nderiv_3_nodes_3", _dev(GRID, FLDS), 102)
_gexpect("empty", GALL, 0)
_gexpect("empty_null_data", GALL, 0)
_gexpect("empty_nodes_3", GALL, 102)                         # 102 comes before the empty product; nothing to zero
for _case in ("null_axes", "null_coef", "null_out"):
    _gexpect(_case, GALL, capi.E_BADARG, NULLARG)


def test_grid_table_covers_every_case():
    assert set(GRID_EXPECTED) == {(name, e) for name, (entries, _) in GRID_CASES.items() for e in entries}


@pytest.mark.parametrize("entry", GALL)
def test_grid_entry_ladder(entry):
    for name, (entries, ov) in GRID_CASES.items():
        if entry in entries:
            assert _grid_call(entry, ov) == GRID_EXPECTED[(name, entry)], (name, entry)
