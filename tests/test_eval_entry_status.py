"""CPU: the argument ladder of the seven point / derivative evaluation entries of the C ABI.

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
