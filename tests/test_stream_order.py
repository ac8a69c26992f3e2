"""The device entries under stream-ordered use (include/splpak_hip.h: "all work is enqueued on `stream`", the fit and the refit
synchronise it before returning, the evaluation entries are asynchronous on it).

The fit side forks private, non-blocking streams from the caller's stream and joins them to it by events alone (ndattach.hip,
ndchol.hip, bandchol.hip, twoend.hip, rowsop.hip), and leaves some work running past the end of a call for the next call to
wait for (evZlast, evPre / evTail, evDone, the band pipeline's `done`, the DevScratch event of the grid fit).  The other tests
hand over inputs that were complete long before the call, pass the legacy default stream and wait for the whole device before
they look: a private stream that starts before the caller's stream has produced the inputs, or that is never joined to it, is
invisible to them.  Here:

  late inputs      the call's input tensors hold a DECOY (other valid inputs of the same shapes) when the call is made; the real
                   inputs arrive by device-to-device copies that sit on the side stream S behind a calibrated delay
                   (torch.cuda._sleep), and the entry is called on S at once.  Work that does not wait for S reads the decoy.
  stream-only      the outputs are copied to pinned host memory by a copy enqueued on the stream of the call, and only that
  read-back        stream is synchronised: work that was never joined to the caller's stream has nothing to wait for it.
  yardstick        the same entry, same options, on inputs complete beforehand, on the default stream, with device-wide waits:
                   the arrangement every other test anchors to the reference, the goldens and the oracle.  Compared bit for bit
                   (the library promises run-to-run identical bits; all points lie inside the box, so the one floating-point
                   atomic left, the histogram bump of a far-outside point, is not reachable).  The decoy's own yardstick must
                   differ from it.
  control          once per entry family the same late-input call is made on a SECOND stream while the delay and the copies
                   sit on S -- a caller's mistake, made on purpose.  It reads valid memory holding valid data and must return
                   the decoy's yardstick bit for bit: the window was open.
  T                five times the plain call's duration measured in the test, at least 20 ms; every delay is bracketed by two
                   events and must have lasted at least what was asked.

A pass is not a proof.  With the default of four hardware queues several streams of a process share a queue, and streams that
share a queue serialise: that can hide a missing wait, it cannot fake one.  (Measured on an MI355X: with four queues a private
stream of the nested-dissection and of the two-ended plan shared S's queue -- the fit controls returned the decoy's bits but
ended only when the delay had; with GPU_MAX_HW_QUEUES=16 they ended inside it, and every test here passed either way.)  The
control needs one stream that does NOT serialise behind S; the `streams` fixture finds one by a probe and the controls fail
where there is none.
"""
import functools
import threading

import numpy as np
import pytest

from splpak_amd import capi
from splpak_amd.synth import synth_points

M = 20_000                          # points of every Plan.fit here
INFO = [0, 1, 2, 3, 4, 8, 9]        # the entries of info that are no timings
T_FACTOR, T_FLOOR_MS = 5.0, 20.0
SENTINEL = 7.0                      # what an output holds before the call


# ---------------------------------------------------------------------------------------------------------------
# the harness
class _Delay:
    """A sleep of `ms` milliseconds enqueued on `stream`, between two timing events."""

    def __init__(self, stream, ms, cycles_per_ms):
        import torch
        self.ms = float(ms)
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            self.e0.record()
            torch.cuda._sleep(int(self.ms * cycles_per_ms * 1.05) + 1)       # (5 %: the calibration's own scatter)
            self.e1.record()

    def running(self):
        return not self.e1.query()

    def check(self, what):
        """After the stream has been synchronised: the delay lasted at least what was asked -- otherwise the test proves nothing."""
        got = self.e0.elapsed_time(self.e1)
        print(f"{what}: delay asked {self.ms:.2f} ms, achieved {got:.2f} ms")
        assert got >= self.ms, (what, got, self.ms)


class _Clock:
    """Cycles of torch.cuda._sleep per millisecond on this device, timed once with two events on a side stream."""

    def __init__(self):
        import torch
        st = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cycles, ms = 1_000_000, 0.0
        with torch.cuda.stream(st):
            torch.cuda._sleep(cycles)               # (the first launch loads the kernel)
        st.synchronize()
        for _ in range(10):
            with torch.cuda.stream(st):
                e0.record()
                torch.cuda._sleep(cycles)
                e1.record()
            st.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 10.0:
                break
            cycles *= 4
        assert ms >= 10.0, (cycles, ms)
        self.cycles_per_ms = cycles / ms
        print(f"torch.cuda._sleep: {cycles} cycles in {ms:.3f} ms = {self.cycles_per_ms:.0f} cycles per ms")

    def delay(self, stream, ms):
        return _Delay(stream, ms, self.cycles_per_ms)


@pytest.fixture(scope="module")
def clock():
    return _Clock()


class _Streams:
    pass


@pytest.fixture(scope="module")
def streams(clock):
    """S, and a second stream S2 on which a kernel completes while a delay sits on S (probed: up to three candidates, so four
    streams at the most).  `concurrent` is False where every candidate serialised behind S: the controls then fail."""
    import torch
    out = _Streams()
    out.S = torch.cuda.Stream()
    probe = torch.zeros(64, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    out.S2, out.concurrent = None, False
    for _ in range(3):
        cand = torch.cuda.Stream()
        d = clock.delay(out.S, T_FLOOR_MS)
        with torch.cuda.stream(cand):
            probe.add_(1.0)
        cand.synchronize()
        free = d.running()
        out.S.synchronize()
        if out.S2 is None or free:
            out.S2 = cand
        if free:
            out.concurrent = True
            break
    print(f"side streams: S2 runs beside a delay on S: {out.concurrent}")
    return out


NO_WINDOW = ("every candidate for the second stream serialised behind the delay on S (shared hardware queue): "
             "the control cannot show that the window was open")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _default_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class _Entry:
    """A device entry with its options fixed: call(t, stream) -> tuple of host results, on a dict `t` of device tensors -- the
    inputs under the names of the data dicts, the outputs under the names of `outs` (name -> shape, float64)."""

    def __init__(self, call, outs):
        self.call, self.outs = call, outs

    def outputs(self):
        import torch
        return {k: torch.full(tuple(s), SENTINEL, dtype=torch.float64, device="cuda") for k, s in self.outs.items()}

    def pinned(self):
        import torch
        return {k: torch.empty(tuple(s), dtype=torch.float64, pin_memory=True) for k, s in self.outs.items()}


class _Result:
    def __init__(self, dev, host):
        self.dev, self.host = dev, tuple(np.array(h) for h in host)

    def differs(self, other):
        """Names of what is not bit for bit the same."""
        bad = [k for k in self.dev if not np.array_equal(self.dev[k], other.dev[k])]
        return bad + [f"host[{i}]" for i, (a, b) in enumerate(zip(self.host, other.host)) if not np.array_equal(a, b)]


def _plain(entry, data):
    """The yardstick: inputs complete beforehand, the default stream, device-wide waits -> (result, milliseconds of the call)."""
    import torch
    t = {k: _dev(v) for k, v in data.items()}
    t.update(entry.outputs())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    host = entry.call(t, _default_stream())
    e1.record()
    torch.cuda.synchronize()
    return _Result({k: t[k].cpu().numpy() for k in entry.outs}, host), e0.elapsed_time(e1)


def _yardsticks(entry, data, decoy, what):
    """(yardstick of the inputs, yardstick of the decoy, T).  The decoy goes first, so that what a first call allocates is not
    in the measured duration."""
    yd, _ = _plain(entry, decoy)
    yi, ms = _plain(entry, data)
    T = max(T_FACTOR * ms, T_FLOOR_MS)
    print(f"{what}: plain call {ms:.3f} ms, T = {T:.2f} ms")
    assert yi.differs(yd), f"{what}: the decoy gives the same result as the inputs: it proves nothing"
    return yi, yd, T


def _late(entry, data, decoy, S, R, clock, T, before=None):
    """The inputs hold the decoy; delay(S, T), then the copies of the real inputs, on S; the entry on R (S itself; another
    stream in a control) at once; the outputs to pinned memory by copies on R; R alone is synchronised.
    -> (result, the delay, whether the delay was still running when R had finished).  S is synchronised before returning: by
    then the result is on the host.  before(t, S): more work for S between the copies and the call (synth_points_dev)."""
    import torch
    t = {k: _dev(decoy[k]) for k in data}
    stage = {k: _dev(data[k]) for k in data}
    t.update(entry.outputs())
    pinned = entry.pinned()                 # (everything is allocated before the delay: an allocation may synchronise)
    torch.cuda.synchronize()
    try:
        d = clock.delay(S, T)
        with torch.cuda.stream(S):
            for k in stage:
                t[k].copy_(stage[k], non_blocking=True)
        if before is not None:
            before(t, S)
        host = entry.call(t, R.cuda_stream)
        with torch.cuda.stream(R):
            for k in pinned:
                pinned[k].copy_(t[k], non_blocking=True)
        R.synchronize()
        early = d.running()
        res = _Result({k: pinned[k].numpy().copy() for k in pinned}, host)
    finally:
        S.synchronize()
        R.synchronize()
    return res, d, early


def _check_late(entry, data, decoy, streams, clock, what, before=None, yardsticks=None):
    yi, yd, T = _yardsticks(entry, data, decoy, what) if yardsticks is None else yardsticks
    got, d, _ = _late(entry, data, decoy, streams.S, streams.S, clock, T, before)
    d.check(what)
    assert not got.differs(yi), (what, got.differs(yi), "equals the decoy's" if not got.differs(yd) else "neither")


def _check_control(entry, data, decoy, streams, clock, what):
    """The call on S2 while the delay and the copies sit on S: it must return the decoy's yardstick.  (Whether it also ENDED
    inside the delay is only printed: a private stream of the library that shares a hardware queue with S finishes its part
    behind the delay, long after the inputs were read.)"""
    assert streams.concurrent, NO_WINDOW
    yi, yd, T = _yardsticks(entry, data, decoy, what)
    got, d, early = _late(entry, data, decoy, streams.S, streams.S2, clock, T)
    d.check(what)
    print(f"{what}: ended inside the delay: {early}")
    assert not got.differs(yd), (what, got.differs(yd), "equals the inputs'" if not got.differs(yi) else "neither")


# ---------------------------------------------------------------------------------------------------------------
# Plan.fit
@functools.lru_cache(maxsize=None)
def _points(nd, part):
    """Points part*M .. part*M + M - 1 of synth_points on the unit box (shared; nobody writes to them)."""
    return synth_points(nd, M, first_point=part * M)


def _fit_data(nd, part, weighted):
    x, y, w = _points(nd, part)
    return {"x": x, "y": y, "w": w} if weighted else {"x": x, "y": y}


DIRECT = {"SPLPAK_SOLVER": "direct"}
BAND = dict(DIRECT, SPLPAK_ND="0", SPLPAK_NO_TWOEND="1")
ND = dict(DIRECT, SPLPAK_ND="1")
# label -> (nodes, environment the plan is created under, the code plan.factorisation() must report)
ROUTES = {
    "band_narrow": ([9, 17, 13], BAND, 1),
    "band_pipeline": ([64, 64], dict(BAND, SPLPAK_NARROW_BW="1"), 0),
    "twoend": ([64, 64], dict(DIRECT, SPLPAK_ND="0"), 2),
    "nd_16": ([16, 16, 16], ND, 4),
    "nd": ([9, 17, 13], ND, 4),
    "nd_clear_all_early": ([9, 17, 13], dict(ND, SPLPAK_ND_STAGED_INIT="0"), 4),
    "nd_clear_all_late": ([9, 17, 13], dict(ND, SPLPAK_ND_STAGED_INIT="0", SPLPAK_ND_NO_EARLY_CLEAR="1"), 4),
    "nd_cut_2": ([9, 17, 13], dict(ND, SPLPAK_ND_CUT="2"), 4),
    "nd_halves_9": ([9, 17, 13], dict(ND, SPLPAK_ND_HALVES="9"), 4),
    "nd_one_stream": ([9, 17, 13], dict(ND, SPLPAK_NO_LOOKAHEAD="1"), 4),
    "nd_prep_early": ([9, 17, 13], dict(ND, SPLPAK_ND_PREP_EARLY="1"), 4),
    "pcg": ([6, 6, 6, 6], {"SPLPAK_SOLVER": "pcg"}, 6),
}


def _plan(label, monkeypatch, xtrap=1.0, scale=1.0):
    """The plan of ROUTES[label] on the box [0, scale]^nd."""
    nodes, env, code = ROUTES[label]
    nd = len(nodes)
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        plan = capi.Plan(nd, nodes, [0.0] * nd, [scale] * nd, xtrap, M)
    got = plan.factorisation()[0]
    if got != code:
        plan.close()
        raise AssertionError(f"{label} {nodes} {env}: factorisation {got}, wanted {code}")
    return plan


def _fit_entry(plan):
    def call(t, stream):
        rc, info = plan.fit(t["x"], t["y"], t.get("w"), t["coef"], stream)
        return rc, info[INFO]
    return _Entry(call, {"coef": (plan.ncol,)})


def _fits_ok(*results):
    return all(int(r.host[0]) == 0 for r in results)


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [True, False], ids=["weights", "no_weights"])
@pytest.mark.parametrize("label", list(ROUTES))
def test_fit_with_late_inputs_and_stream_only_read_back(label, weighted, monkeypatch, clock, streams):
    """A. With weights the fit reads w[0] back and synchronises the stream before any other work; only the unweighted call
    leaves its first kernels waiting behind the delay."""
    nd = len(ROUTES[label][0])
    data, decoy = _fit_data(nd, 0, weighted), _fit_data(nd, 1, weighted)
    plan = _plan(label, monkeypatch)
    try:
        entry = _fit_entry(plan)
        what = f"fit {label} {'weights' if weighted else 'no weights'}"
        ys = _yardsticks(entry, data, decoy, what)
        assert _fits_ok(ys[0], ys[1])
        _check_late(entry, data, decoy, streams, clock, what, yardsticks=ys)
    finally:
        plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("label", ["nd_16", "twoend"])
def test_fit_on_the_wrong_stream_reads_the_decoy(label, monkeypatch, clock, streams):
    """The control of A: once for the nested dissection, once for a band route."""
    nd = len(ROUTES[label][0])
    data, decoy = _fit_data(nd, 0, False), _fit_data(nd, 1, False)
    plan = _plan(label, monkeypatch)
    try:
        _check_control(_fit_entry(plan), data, decoy, streams, clock, f"control fit {label}")
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# B. a plan that moves between streams
MOVING = ["nd_16", "twoend", "pcg"]


def _four_steps(plan, nd, queues):
    """Fit data set 1, fit data set 2, refit a second field of data set 2, fit data set 1 again.  queues: None -- the default
    stream, a device-wide wait after every step; else the four streams of the steps -- nothing in between but the calls' own
    synchronisation, every result read back by a copy on the stream of its call.  -> [(coef, ierror, info)] per step."""
    import torch
    (x1, y1, _), (x2, y2, _), (_, y3, _) = _points(nd, 0), _points(nd, 1), _points(nd, 2)
    x1, y1, x2, y2, y3 = (_dev(a) for a in (x1, y1, x2, y2, y3))
    coefs = [torch.full((plan.ncol,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(4)]
    pinned = [torch.empty(plan.ncol, dtype=torch.float64, pin_memory=True) for _ in range(4)]
    steps = [lambda c, q: plan.fit(x1, y1, None, c, q), lambda c, q: plan.fit(x2, y2, None, c, q),
             lambda c, q: plan.refit(y3, c, q), lambda c, q: plan.fit(x1, y1, None, c, q)]
    torch.cuda.synchronize()
    host = []
    if queues is None:
        for step, c in zip(steps, coefs):
            host.append(step(c, _default_stream()))
            torch.cuda.synchronize()
        return [(c.cpu().numpy(), rc, info[INFO]) for c, (rc, info) in zip(coefs, host)]
    try:
        for step, c, p, q in zip(steps, coefs, pinned, queues):
            host.append(step(c, q.cuda_stream))
            with torch.cuda.stream(q):
                p.copy_(c, non_blocking=True)
    finally:
        for q in queues:
            q.synchronize()
    return [(p.numpy().copy(), rc, info[INFO]) for p, (rc, info) in zip(pinned, host)]


@pytest.mark.gpu
@pytest.mark.parametrize("label", MOVING)
def test_plan_moves_between_streams(label, monkeypatch, streams):
    """B. What evDone, evZlast, evTail, the band pipeline's `done` and the rows' side-stream events exist for: every step
    equals the same step on a fresh plan with device-wide waits."""
    import torch
    nd = len(ROUTES[label][0])
    fresh = _plan(label, monkeypatch)
    try:
        want = _four_steps(fresh, nd, None)
    finally:
        fresh.close()
    plan = _plan(label, monkeypatch)
    try:
        got = _four_steps(plan, nd, [streams.S, streams.S2, streams.S, torch.cuda.default_stream()])
    finally:
        plan.close()
    assert [w[1] for w in want] == [0, 0, 0, 0]
    assert not np.array_equal(want[0][0], want[1][0]) and not np.array_equal(want[1][0], want[2][0])
    assert np.array_equal(want[0][0], want[3][0])
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[1] == w[1] and np.array_equal(g[0], w[0]) and np.array_equal(g[2], w[2]), (label, "step", i + 1)


# ---------------------------------------------------------------------------------------------------------------
# C. the inputs belong to the caller again at return
def _fit_then_refit(plan, nd, nfields, S):
    """A weighted fit, then a refit of `nfields` fields whose first is the fit's own.  S None: the default stream with
    device-wide waits, nothing disturbed.  Else on S: when the fit has returned x, y and w are overwritten with other points by
    copies on S, and the refit is given the values from a tensor of its own.  -> (fit coef, refit coef, ierrors, infos)"""
    import torch
    x, y, w = (_dev(a) for a in _points(nd, 0))
    ys = np.stack([_points(nd, k)[1] for k in range(nfields)])
    keep = _dev(ys[0] if nfields == 1 else ys)
    other = [_dev(a) for a in _points(nd, 3)]
    c1 = torch.full((plan.ncol,), SENTINEL, dtype=torch.float64, device="cuda")
    c2 = torch.full((plan.ncol,) if nfields == 1 else (nfields, plan.ncol), SENTINEL, dtype=torch.float64, device="cuda")
    p1, p2 = (torch.empty(tuple(c.shape), dtype=torch.float64, pin_memory=True) for c in (c1, c2))
    torch.cuda.synchronize()
    if S is None:
        rc1, i1 = plan.fit(x, y, w, c1, _default_stream())
        torch.cuda.synchronize()
        rc2, i2 = plan.refit(keep, c2, _default_stream())
        torch.cuda.synchronize()
        return c1.cpu().numpy(), c2.cpu().numpy(), (rc1, rc2), (i1[INFO], i2[..., INFO])
    try:
        rc1, i1 = plan.fit(x, y, w, c1, S.cuda_stream)
        with torch.cuda.stream(S):
            p1.copy_(c1, non_blocking=True)
            for dst, src in zip((x, y, w), other):
                dst.copy_(src, non_blocking=True)
        rc2, i2 = plan.refit(keep, c2, S.cuda_stream)
        with torch.cuda.stream(S):
            p2.copy_(c2, non_blocking=True)
    finally:
        S.synchronize()
    return p1.numpy().copy(), p2.numpy().copy(), (rc1, rc2), (i1[INFO], i2[..., INFO])


@pytest.mark.gpu
@pytest.mark.parametrize("label,nfields", [("nd_16", 1), ("nd_16", 3), ("twoend", 1), ("pcg", 1)])
def test_inputs_belong_to_the_caller_at_return(label, nfields, monkeypatch, streams):
    """C. Three fields on the nested-dissection plan: the batched sweep (route 2 of splpak_debug_plan_refit_stats)."""
    nd = len(ROUTES[label][0])
    results = []
    for S in (None, streams.S):
        plan = _plan(label, monkeypatch)
        try:
            results.append(_fit_then_refit(plan, nd, nfields, S))
            route = plan.refit_stats()[0]
        finally:
            plan.close()
        assert route == (2 if nfields == 3 else 1), (label, nfields, route)
    want, got = results
    assert want[2] == (0, 0) and got[2] == (0, 0)
    assert np.array_equal(got[0], want[0]), (label, "fit")
    assert np.array_equal(got[1], want[1]), (label, "refit")
    assert np.array_equal(got[3][0], want[3][0]) and np.array_equal(got[3][1], want[3][1]), (label, "info")


# ---------------------------------------------------------------------------------------------------------------
# D. two plans, two host threads, two streams
@pytest.mark.gpu
def test_two_plans_two_threads_two_streams(monkeypatch, streams):
    """D. Each thread holds a plan of its own and a side stream of its own and runs three fits of different data."""
    import torch
    labels = ["nd_16", "twoend"]
    want = {}
    for label in labels:                    # the serial yardsticks, on a plan of their own
        nd = len(ROUTES[label][0])
        plan = _plan(label, monkeypatch)
        try:
            entry = _fit_entry(plan)
            want[label] = [_plain(entry, _fit_data(nd, part, True))[0] for part in range(3)]
        finally:
            plan.close()
        assert _fits_ok(*want[label])
    plans = [_plan(label, monkeypatch) for label in labels]
    barrier = threading.Barrier(2)
    got = {}

    def worker(label, plan, S):
        try:
            torch.cuda.set_device(0)
            nd = len(ROUTES[label][0])
            sets = [[_dev(a) for a in _points(nd, part)] for part in range(3)]
            coefs = [torch.full((plan.ncol,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(3)]
            pinned = [torch.empty(plan.ncol, dtype=torch.float64, pin_memory=True) for _ in range(3)]
            torch.cuda.synchronize()
            barrier.wait(timeout=60)
            host = []
            for (x, y, w), c, p in zip(sets, coefs, pinned):
                host.append(plan.fit(x, y, w, c, S.cuda_stream))
                with torch.cuda.stream(S):
                    p.copy_(c, non_blocking=True)
            S.synchronize()
            got[label] = [_Result({"coef": p.numpy().copy()}, (rc, info[INFO])) for p, (rc, info) in zip(pinned, host)]
        except Exception as exc:          # (reported by the assertion below)
            got[label] = exc
            barrier.abort()

    try:
        threads = [threading.Thread(target=worker, args=(label, plan, S))
                   for label, plan, S in zip(labels, plans, (streams.S, streams.S2))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        alive = [t.is_alive() for t in threads]
        torch.cuda.synchronize()
    finally:
        if not any(t.is_alive() for t in threads):
            for plan in plans:
                plan.close()
    assert alive == [False, False], alive
    for label in labels:
        assert isinstance(got.get(label), list), (label, got.get(label))
        for part, (g, w) in enumerate(zip(got[label], want[label])):
            assert not g.differs(w), (label, "fit", part, g.differs(w))


# ---------------------------------------------------------------------------------------------------------------
# E. the other device entries
GRID_NODES, GRID_NPTS = (12, 10, 8), (37, 29, 19)
UNIT3 = ([0.0] * 3, [1.0] * 3)


@functools.lru_cache(maxsize=None)
def _grid_data_cached(seed, weighted):
    """Unsorted axes, one coordinate per stratum of the unit interval, two fields of values; weighted: a weight per sample, a
    tenth of them zero."""
    rng = np.random.default_rng(seed)
    axes = []
    for n in GRID_NPTS:
        u = (np.arange(n) + rng.uniform(0.05, 0.95, n)) / n
        rng.shuffle(u)
        axes.append(u)
    nsamp = int(np.prod(GRID_NPTS))
    data = {"axes": np.concatenate(axes), "values": rng.standard_normal((2, nsamp))}
    if weighted:
        w = rng.uniform(0.5, 2.0, nsamp)
        w[rng.permutation(nsamp)[:nsamp // 10]] = 0.0
        data["weights"] = w
    return data


def _grid_data(seed, weighted):
    return dict(_grid_data_cached(seed, weighted))


def _grid_entry(weighted):
    ncol = int(np.prod(GRID_NODES))

    def call(t, stream):
        if weighted:
            rc, info = capi.fit_grid_weighted_dev(3, GRID_NPTS, t["axes"], t["values"], t["weights"], *UNIT3, list(GRID_NODES), t["coef"],
                                                  nfields=2, stream=stream)
        else:
            rc, info = capi.fit_grid_dev(3, GRID_NPTS, t["axes"], t["values"], *UNIT3, list(GRID_NODES), t["coef"], nfields=2, stream=stream)
        return rc, info[:, INFO]
    return _Entry(call, {"coef": (2, ncol)})


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True], ids=["fit_grid", "fit_grid_weighted"])
def test_grid_fit_with_late_inputs(weighted, clock, streams):
    entry = _grid_entry(weighted)
    data, decoy = _grid_data(11, weighted), _grid_data(12, weighted)
    ys = _yardsticks(entry, data, decoy, "fit_grid_weighted" if weighted else "fit_grid")
    assert _fits_ok(ys[0], ys[1])
    _check_late(entry, data, decoy, streams, clock, "fit_grid_weighted" if weighted else "fit_grid", yardsticks=ys)


@pytest.mark.gpu
def test_grid_fit_on_the_wrong_stream_reads_the_decoy(clock, streams):
    """The control of E."""
    _check_control(_grid_entry(False), _grid_data(11, False), _grid_data(12, False), streams, clock, "control fit_grid")


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True], ids=["fit_grid", "fit_grid_weighted"])
def test_grid_fits_back_to_back_on_alternating_streams(weighted, streams):
    """Two calls in a row on two streams with different data and no wait in between share the per-thread DevScratch: each
    must return its own yardstick."""
    import torch
    entry = _grid_entry(weighted)
    sets = [_grid_data(11, weighted), _grid_data(12, weighted)]
    want = [_plain(entry, d)[0] for d in sets]
    assert _fits_ok(*want) and want[0].differs(want[1])
    ts = []
    for d in sets:
        t = {k: _dev(v) for k, v in d.items()}
        t.update(entry.outputs())
        ts.append(t)
    pinned = [entry.pinned(), entry.pinned()]
    queues = [streams.S, streams.S2]
    torch.cuda.synchronize()
    host = []
    try:
        for t, p, q in zip(ts, pinned, queues):
            host.append(entry.call(t, q.cuda_stream))
            with torch.cuda.stream(q):
                p["coef"].copy_(t["coef"], non_blocking=True)
    finally:
        for q in queues:
            q.synchronize()
    for i in range(2):
        got = _Result({"coef": pinned[i]["coef"].numpy().copy()}, host[i])
        assert not got.differs(want[i]), ("call", i + 1, got.differs(want[i]))


MANY = {"1d": ((9,), 25, 120), "2d": ((5, 9), 150, 400)}        # nodes, the fewest and the most points of a problem
NBATCH = 300


@functools.lru_cache(maxsize=None)
def _many_offsets(name):
    _, lo, hi = MANY[name]
    sizes = np.random.default_rng(300 + len(name)).integers(lo, hi, NBATCH)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _many_data(name, seed):
    nd = len(MANY[name][0])
    n = int(_many_offsets(name)[-1])
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (n, nd))
    y = np.sin(3.0 * x + np.arange(1, nd + 1)).sum(axis=1) + 0.01 * (rng.uniform(0.0, 1.0, n) - 0.5)
    return {"x": x, "y": y, "w": rng.uniform(0.5, 1.5, n)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MANY))
def test_fit_many_with_late_inputs(name, clock, streams):
    nodes = MANY[name][0]
    nd = len(nodes)
    off = _many_offsets(name)

    def call(t, stream):
        rc, status, info = capi.fit_many_dev(nd, off, t["x"], t["y"], t["w"], [0.0] * nd, [1.0] * nd, list(nodes), t["coef"], xtrap=1.0,
                                             stream=stream)
        return rc, status, info[:, INFO]
    entry = _Entry(call, {"coef": (NBATCH, int(np.prod(nodes)))})
    data, decoy = _many_data(name, 21), _many_data(name, 22)
    ys = _yardsticks(entry, data, decoy, f"fit_many {name}")
    assert _fits_ok(ys[0], ys[1]) and not ys[0].host[1].any()
    _check_late(entry, data, decoy, streams, clock, f"fit_many {name}", yardsticks=ys)


def _eval_data(nodes, nq, nfields, seed):
    rng = np.random.default_rng(seed)
    ncol = int(np.prod(nodes))
    return {"q": rng.uniform(0.0, 1.0, (nq, len(nodes))), "coef": rng.standard_normal((nfields, ncol) if nfields else ncol)}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["direct", "binned"])
def test_evaluate_fields_with_late_inputs(mode, clock, streams):
    nodes, nq = (19, 19, 19), 5000
    routes = []

    def call(t, stream):
        capi.set_eval_mode(capi.EVAL_DIRECT if mode == "direct" else capi.EVAL_BINNED)
        rc = capi.evaluate_fields_dev(3, t["q"], None, t["coef"], *UNIT3, list(nodes), t["out"], stream)
        routes.append(capi.debug_eval_fields_stats()[0])        # (host counters: nothing is waited for)
        return (rc,)
    try:
        _check_late(_Entry(call, {"out": (3, nq)}), _eval_data(nodes, nq, 3, 31), _eval_data(nodes, nq, 3, 32), streams, clock,
                    f"evaluate_fields {mode}")
    finally:
        capi.set_eval_mode(capi.EVAL_AUTO)
    assert len(routes) == 3 and all((r == 1) == (mode == "direct") for r in routes), routes


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["direct", "binned"])
def test_evaluate_derivs_with_late_inputs(mode, clock, streams):
    nodes, nq = (20, 17, 30), 30_011

    def call(t, stream):
        if mode == "direct":
            capi.set_eval_mode(capi.EVAL_DIRECT)
        else:
            capi.set_eval_mode(capi.EVAL_BINNED, 4099)
        return (capi.evaluate_derivs_dev(3, t["q"], 2, t["coef"], *UNIT3, list(nodes), t["out"], stream),)
    try:
        _check_late(_Entry(call, {"out": (nq, capi.derivs_nout(3, 2))}), _eval_data(nodes, nq, 0, 41), _eval_data(nodes, nq, 0, 42),
                    streams, clock, f"evaluate_derivs {mode}")
    finally:
        capi.set_eval_mode(capi.EVAL_AUTO)


@pytest.mark.gpu
def test_synth_points_then_a_fit_on_the_same_stream(monkeypatch, clock, streams):
    """synth_points_dev followed, with no wait, by the fit that consumes its output: x, y and w hold other points until the
    generator, which sits behind the delay, has written them."""
    nd = 3
    plan = _plan("nd_16", monkeypatch)
    try:
        def call(t, stream):
            rc, info = plan.fit(t["x"], t["y"], t["w"], t["coef"], stream)
            return rc, info[INFO]

        def plain_call(t, stream):
            import torch
            capi.synth_points_dev(nd, 0, M, t["x"], t["y"], t["w"], stream)
            torch.cuda.synchronize()
            return call(t, stream)
        outs = {"coef": (plan.ncol,)}
        decoy = _fit_data(nd, 1, True)
        what = "synth_points + fit"
        yd, _ = _plain(_Entry(call, outs), decoy)
        yi, ms = _plain(_Entry(plain_call, outs), decoy)          # (the generator overwrites what it is given)
        T = max(T_FACTOR * ms, T_FLOOR_MS)
        print(f"{what}: plain calls {ms:.3f} ms, T = {T:.2f} ms")
        assert _fits_ok(yi, yd) and yi.differs(yd)
        # (nothing to stage: the "copies" put the decoy where it is already, and the generator follows them on S)
        got, d, _ = _late(_Entry(call, outs), decoy, decoy, streams.S, streams.S, clock, T,
                          before=lambda t, S: capi.synth_points_dev(nd, 0, M, t["x"], t["y"], t["w"], S.cuda_stream))
        d.check(what)
        assert not got.differs(yi), (what, got.differs(yi), "equals the decoy's" if not got.differs(yd) else "neither")
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# F. the batch entries and the per-thread scratch behind them (the offsets of all three families, fit_many's tables)
SMALL_NODES = (9,)
OFF_A = np.array([0, 40, 80, 120], dtype=np.int64)
OFF_B = np.array([0, 20, 100, 120], dtype=np.int64)        # the same total and nbatch as OFF_A: every index stays in bounds


def _small_batch(seed, keys):
    """120 points of a 1-D batch of 3 problems on 9 nodes, and a coefficient row per problem."""
    rng = np.random.default_rng(seed)
    n = int(OFF_A[-1])
    d = {"x": rng.uniform(0.0, 1.0, (n, 1)), "y": rng.standard_normal(n), "w": rng.uniform(0.5, 1.5, n),
         "coef": rng.standard_normal((3, SMALL_NODES[0]))}
    return {k: d[k] for k in keys}


def _eval_many_entry(off):
    def call(t, stream):
        return (capi.evaluate_many_dev(1, off, t["x"], None, t["coef"], [0.0], [1.0], list(SMALL_NODES), t["out"], stream=stream),)
    return _Entry(call, {"out": (int(off[-1]),)})


def _residuals_many_entry(off):
    def call(t, stream):
        return (capi.residuals_many_dev(1, off, t["x"], t["y"], t["w"], t["coef"], [0.0], [1.0], list(SMALL_NODES), t["resid"], t["stats"],
                                        stream=stream),)
    return _Entry(call, {"resid": (int(off[-1]),), "stats": (off.size - 1, 4)})


def _fit_many_entry(off, nodes=SMALL_NODES, counters=None):
    """counters: a list that receives debug_fit_many_stats() of every call."""
    nd, nbatch = len(nodes), off.size - 1

    def call(t, stream):
        rc, status, info = capi.fit_many_dev(nd, off, t["x"], t["y"], t["w"], [0.0] * nd, [1.0] * nd, list(nodes), t["coef"], xtrap=1.0,
                                             stream=stream)
        if counters is not None:
            counters.append(capi.debug_fit_many_stats())
        return rc, status, info[:, INFO]
    return _Entry(call, {"coef": (nbatch, int(np.prod(nodes)))})


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["evaluate_many", "residuals_many"])
def test_many_evaluation_with_late_inputs(family, clock, streams):
    """Both entries only enqueue; resid and stats of the residual pass are compared alike."""
    if family == "evaluate_many":
        entry, keys = _eval_many_entry(OFF_A), ("x", "coef")
    else:
        entry, keys = _residuals_many_entry(OFF_A), ("x", "y", "w", "coef")
    _check_late(entry, _small_batch(51, keys), _small_batch(52, keys), streams, clock, family)


@pytest.mark.gpu
@pytest.mark.parametrize("second", ["evaluate_many", "fit_many"])
def test_two_batches_share_the_offsets_scratch_across_streams(second, clock, streams):
    """evaluate_many_dev with OFF_A on S behind a delay, then with no wait a call with OFF_B on S2 (fit_many_dev may block until
    the delay ends): the second upload of the offsets has to wait for the first kernel.  Without the wait the first kernel reads
    OFF_B: the values of `swapped` below."""
    import torch
    first = _eval_many_entry(OFF_A)
    data_a = _small_batch(53, ("x", "coef"))
    if second == "evaluate_many":
        other, data_b = _eval_many_entry(OFF_B), _small_batch(54, ("x", "coef"))
    else:
        other, data_b = _fit_many_entry(OFF_B), _small_batch(54, ("x", "y", "w"))
    (want_a, ms), (want_b, _) = _plain(first, data_a), _plain(other, data_b)
    swapped, _ = _plain(_eval_many_entry(OFF_B), data_a)
    assert want_a.differs(swapped), "the first batch gives the same values under either offsets: the test proves nothing"
    if second == "evaluate_many":
        assert want_a.differs(want_b)
    else:
        assert _fits_ok(want_b) and not want_b.host[1].any()
    entries, ts, pinned = [first, other], [], []
    for e, d in zip(entries, (data_a, data_b)):
        t = {k: _dev(v) for k, v in d.items()}
        t.update(e.outputs())
        ts.append(t)
        pinned.append(e.pinned())
    queues = [streams.S, streams.S2]
    torch.cuda.synchronize()
    host = []
    try:
        d = clock.delay(streams.S, max(T_FACTOR * ms, T_FLOOR_MS))
        for e, t, p, q in zip(entries, ts, pinned, queues):
            host.append(e.call(t, q.cuda_stream))
            with torch.cuda.stream(q):
                for k in p:
                    p[k].copy_(t[k], non_blocking=True)
    finally:
        for q in queues:
            q.synchronize()
    d.check(f"offsets scratch, then {second}")
    for i, want in enumerate((want_a, want_b)):
        got = _Result({k: pinned[i][k].numpy().copy() for k in pinned[i]}, host[i])
        assert not got.differs(want), ("call", i + 1, got.differs(want))


@pytest.mark.gpu
def test_fit_many_scratch_regrows_and_is_kept():
    """3 problems, 300, 300 again, 3 again: the small batch gives the same bits before and after the scratch grew, and a call
    whose scratch is large enough makes no device allocation (slot [6] of the counters)."""
    capi.shutdown()                         # (the scratch of earlier tests: the first calls below have to allocate)
    counters = []
    small, big = _fit_many_entry(OFF_A, counters=counters), _fit_many_entry(_many_offsets("1d"), MANY["1d"][0], counters=counters)
    data_small, data_big = _small_batch(55, ("x", "y", "w")), _many_data("1d", 21)
    r1, _ = _plain(small, data_small)
    r2, _ = _plain(big, data_big)
    r2b, _ = _plain(big, data_big)
    r3, _ = _plain(small, data_small)
    assert _fits_ok(r1, r2, r2b, r3)
    assert not r3.differs(r1), r3.differs(r1)
    assert not r2b.differs(r2), r2b.differs(r2)
    allocs = [c[6] for c in counters]
    print(f"device allocations of the four calls: {allocs}")
    assert allocs[0] > 0 and allocs[1] > 0, allocs          # (the counter counts)
    assert allocs[2] == 0 and allocs[3] == 0, allocs


@pytest.mark.gpu
def test_fit_many_does_not_wait_for_other_streams(clock, streams):
    """With its scratch in place fit_many_dev frees nothing, so it returns while a delay still runs on another stream."""
    import torch
    assert streams.concurrent, NO_WINDOW
    entry, data = _fit_many_entry(OFF_A), _small_batch(56, ("x", "y", "w"))
    _plain(entry, data)                     # (the warm-up: what a first call allocates)
    want, ms = _plain(entry, data)
    assert _fits_ok(want)
    t = {k: _dev(v) for k, v in data.items()}
    t.update(entry.outputs())
    torch.cuda.synchronize()
    try:
        d = clock.delay(streams.S, max(T_FACTOR * ms, T_FLOOR_MS))
        host = entry.call(t, streams.S2.cuda_stream)
        running = d.running()
    finally:
        streams.S.synchronize()
        streams.S2.synchronize()
    d.check("fit_many beside a delay")
    got = _Result({"coef": t["coef"].cpu().numpy()}, host)
    assert not got.differs(want), got.differs(want)
    assert running, "fit_many_dev on S2 returned only when the delay on S had ended"
