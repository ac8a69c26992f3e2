"""The operand queue of the nested-dissection update kernel (csrc/ndkernels.hip, nd_syrk_kernel) under slow loads.

The kernel keeps SD k-steps of operand loads in flight and waits, in front of each k-step's MFMAs, only for the loads that step
needs (a counted s_waitcnt vmcnt(N)).  A wait that is one load too lax feeds an MFMA the register contents of SD k-steps earlier.
On an idle device the loads of the older slots have long arrived when they are used, so such a wait passes every other suite;
it bites when loads are slow.  This file makes them slow: beside the fits, a second stream copies a buffer of 1 GiB device to
device back to back, which takes the memory system's bandwidth and stretches every load of the fit.

The reference bits of a grid come from one fit on the idle device without stream overlap (SPLPAK_NO_LOOKAHEAD=1).  Then ten fits
on one plan run on the default stream beside the copies, for the default configuration and for K = 256 passes (SPLPAK_ND_KB=1),
without the split launches (SPLPAK_ND_SMALL_GRID=0) and with four waves per workgroup (SPLPAK_ND_WG4=2).  Every one of them must
give the reference's bits: each element sees the same operations in the same order in all of these forms (tests/test_nd.py).

The grids are the smallest the existing suites establish for each path of the kernel:

  20 x 14 x 17, 60 000 points    partial last block of a pass, padded rows, diagonal items (tests/test_nd_extend_add.py)
  16 x 16 x 16, 40 000 points    launches of few items: four / sixteen waves share an item (SPLIT = 4 / 16)
  32 x 32 x 32, 200 000 points   K = 1024 passes, the item queue, the root's look-ahead (tests/test_nd.py)

The copies are bounded: in front of each of the ten fits, LOAD_FACTOR = 4 times what one fit takes on the idle device, NCOPY_MAX
at the most in all.  They are not enqueued in one piece in front of the first fit, because streams share hardware queues: where
one of the plan's streams falls onto the queue of the copy stream, its work waits behind every copy enqueued so far -- measured
with all copies in front (32^3, default configuration): the ten fits ended together with the last copy, so only the first of
them had run beside the load.  A piece per fit keeps every fit beside its own copies; where no queue is shared (SPLPAK_ND_WG4=2)
a fit beside the copies takes 1.3 to 3 times its idle time.  The figures are printed, not asserted."""
import math
import os
import time

import numpy as np
import pytest

from splpak_amd import capi

GRIDS = {"3d_odd": ([20, 14, 17], 60000), "3d16": ([16, 16, 16], 40000), "3d32": ([32, 32, 32], 200000)}
VARIANTS = {"default": {}, "kb1": {"SPLPAK_ND_KB": "1"}, "no_split": {"SPLPAK_ND_SMALL_GRID": "0"}, "wg4": {"SPLPAK_ND_WG4": "2"}}
NFITS = 10
LOAD_BYTES = 1 << 30
NCOPY_MAX = 4000
LOAD_FACTOR = 4.0

_inputs, _reference = {}, {}


@pytest.fixture(autouse=True)
def _factorisation_only(monkeypatch):
    monkeypatch.setenv("SPLPAK_SOLVER", "direct")
    monkeypatch.setenv("SPLPAK_ND", "1")


@pytest.fixture(scope="module")
def load():
    """(source, destination, seconds per copy on the idle device)"""
    import torch
    dev = torch.device("cuda", 0)
    src = torch.zeros(LOAD_BYTES // 8, dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(4):
        dst.copy_(src)
    b.record()
    b.synchronize()
    yield src, dst, a.elapsed_time(b) * 1e-3 / 4
    del src, dst
    torch.cuda.empty_cache()


def _inp(grid):
    if grid not in _inputs:
        import torch
        from splpak_amd.synth import synth_points
        nodes, m = GRIDS[grid]
        x, y, w = synth_points(3, m)
        dev = torch.device("cuda", 0)
        _inputs[grid] = tuple(torch.tensor(a, dtype=torch.float64, device=dev) for a in (x, y, w))
    return _inputs[grid]


def _setenv(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    return old


def _restore(old):
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _plan_fits(grid, env, nfits, before_each=None):
    """`nfits` fits on one plan on the default stream -> (list of coefficient arrays, seconds per fit).  `before_each` runs in
    front of each of them; a warm-up fit (streams, reserved CUs) comes before all that."""
    import torch
    x, y, w = _inp(grid)
    nodes = GRIDS[grid][0]
    old = _setenv(env)
    plan = None
    try:
        plan = capi.Plan(3, nodes, [0.0] * 3, [1.0] * 3, 1.0, x.shape[0])
        assert plan.factorisation()[0] == 4
        coef = torch.zeros(plan.ncol, dtype=torch.float64, device=x.device)
        out = []
        ierr, info = plan.fit(x, y, w, coef)             # the plan's first fit sets up streams and reserved CUs and waits for the device
        assert ierr == 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(nfits):
            if before_each is not None:
                before_each()
            coef.zero_()
            ierr, info = plan.fit(x, y, w, coef)
            torch.cuda.current_stream().synchronize()
            assert ierr == 0 and info[9] < 1e-9, (ierr, info[9])
            out.append(coef.cpu().numpy())
        dt = (time.perf_counter() - t0) / nfits
    finally:
        if plan is not None:
            plan.close()
        _restore(old)
    return out, dt


def _ref(grid):
    """(reference coefficients, seconds per fit on the idle device): serial streams, nothing else on the device"""
    if grid not in _reference:
        import torch
        torch.cuda.synchronize()
        out, dt = _plan_fits(grid, {"SPLPAK_NO_LOOKAHEAD": "1"}, 2)
        assert np.array_equal(out[0], out[1])
        out[0].setflags(write=False)
        _reference[grid] = (out[0], dt)
    return _reference[grid]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_fits_beside_a_bandwidth_load_keep_the_idle_bits(load, grid, variant):
    import torch
    src, dst, t_copy = load
    ref, t_fit = _ref(grid)
    ncopy = min(NCOPY_MAX // NFITS, max(2, math.ceil(LOAD_FACTOR * t_fit / t_copy)))
    side = torch.cuda.Stream()

    def more_load():
        with torch.cuda.stream(side):
            for _ in range(ncopy):
                dst.copy_(src, non_blocking=True)

    try:
        out, dt = _plan_fits(grid, VARIANTS[variant], NFITS, before_each=more_load)
    finally:
        side.synchronize()
    same = [np.array_equal(c, ref) for c in out]
    print(f"{grid} {variant}: {ncopy} copies of {LOAD_BYTES >> 20} MiB in front of each fit ({t_copy * 1e3:.2f} ms each idle), fit {t_fit * 1e3:.1f} ms "
          f"idle, {dt * 1e3:.1f} ms beside the copies; {sum(same)} of {NFITS} fits have the reference's bits")
    assert all(same), [i for i, s in enumerate(same) if not s]
