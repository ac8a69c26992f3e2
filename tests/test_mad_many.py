"""The median and the MAD of every problem's segment in one launch (splpak_mad_many_*, csrc/madmany.hip, csrc/madselect.hpp).

The yardstick is numpy.median on the keys (double) v + 0.0 of the counted values, and again on |key - med|: the entry returns
exact order statistics, so bit equality is asked for, in f64 and in f32 storage (the float values widened to double are the
keys).  CPU tier: exports and the argument ladder, decided before any device call.
"""
import ctypes as C

import numpy as np
import pytest

from splpak_amd import capi
from tests.test_fit_many_clip import same_bits

SYMBOLS = ("splpak_mad_many_f64", "splpak_mad_many_f32", "splpak_mad_many_dev_f64", "splpak_mad_many_dev_f32")
E_BADARG = -3


def want_stats(off, values, wsel):
    """numpy's answer -> (nbatch, 4)."""
    off = np.asarray(off, dtype=np.int64)
    out = np.zeros((off.size - 1, 4))
    for k in range(off.size - 1):
        v = np.asarray(values[off[k]:off[k + 1]])
        if wsel is not None:
            v = v[np.asarray(wsel[off[k]:off[k + 1]]) != 0.0]
        if v.size:
            key = v.astype(np.float64) + 0.0
            med = np.median(key)
            out[k] = [v.size, med, np.median(np.abs(key - med)), 0.0]
    return out


def segments():
    """name -> values: the sizes around the wave and the sweep borders, mixed signs, and the special multisets."""
    rng = np.random.default_rng(9601)
    segs = {f"n{n}": rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n) for n in (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 300, 1000)}
    segs["equal"] = np.full(37, -2.5)                                                   # MAD 0
    segs["half_equal"] = rng.permutation(np.concatenate([np.full(60, 0.125), rng.standard_normal(40)]))
    # an even count whose two middle values are one tie, with further copies on both sides
    segs["tie"] = rng.permutation(np.concatenate([rng.uniform(-3.0, -1.0, 20), np.full(6, 0.75), rng.uniform(1.0, 3.0, 22)]))
    # .. and one whose middle pair straddles two different values, the lower one a tie
    segs["tie_edge"] = rng.permutation(np.concatenate([rng.uniform(-3.0, -1.0, 21), np.full(4, 0.75), rng.uniform(1.0, 3.0, 25)]))
    segs["zeros"] = rng.permutation(np.array([-0.0, 0.0, -0.0, 5e-324, -5e-324, 2.2e-308, -1e-310, 0.0, 1e-320, -0.0, -3e-315, 0.0]))
    segs["signed_zero"] = np.array([-0.0, -0.0, 0.0, -0.0])
    segs["negative"] = -np.abs(rng.standard_normal(90)) - 1e-3
    segs["two_far"] = np.array([-1e300, 1e300])
    return segs


def batch(names, segs, first=0):
    off = np.cumsum([first] + [segs[n].size for n in names]).astype(np.int64)
    vals = np.concatenate([np.full(first, np.nan)] + [segs[n] for n in names])
    return off, vals


def f32_values(v):
    """The segment in float storage: the denormal doubles become float denormals, so that every kind of value is still there."""
    v = np.asarray(v, dtype=np.float64)
    tiny = (np.abs(v) < 1e-300) & (v != 0.0)
    return np.where(tiny, np.sign(v) * 1.4e-45 * (1 + np.arange(v.size) % 5), v).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# CPU tier
def test_symbols_exported():
    lib = capi.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in capi.SYMBOLS


def test_status_ladder_before_any_device_call():
    """SPLPAK_E_BADARG for offsets null, nbatch < 1, offsets that decrease, values null, stats null: stats untouched; a batch
    without points returns 0 with zeros.  No rung asks for a device (the test runs where there is none)."""
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    vals = np.linspace(-1.0, 1.0, 16)
    fn = capi.lib().splpak_mad_many_f64

    def call(nbatch=2, offsets=(0, 8, 16), values=True, stats=True):
        off = None if offsets is None else np.asarray(offsets, dtype=np.int64)
        st = np.full(12, 333.0)
        rc = fn(nbatch, None if off is None else off.ctypes.data_as(lp), vals.ctypes.data_as(dp) if values else None, None,
                st.ctypes.data_as(dp) if stats else None)
        return rc, st
    for kw in (dict(offsets=None, nbatch=0, values=False), dict(nbatch=0, values=False), dict(nbatch=-1), dict(offsets=(0, 8, 4), values=False),
               dict(values=False, stats=False), dict(values=False), dict(stats=False)):
        rc, st = call(**kw)
        assert rc == E_BADARG and np.all(st == 333.0), kw
        assert "offsets" in capi.last_error()
    rc, st = call(offsets=(5, 5, 5))
    assert rc == 0 and np.all(st[:8] == 0.0) and np.all(st[8:] == 333.0)
    assert capi.debug_eval_many_stats()[2:6] == (0, 2, 0, 4)
    rc = capi.lib().splpak_mad_many_f32(1, None, None, None, None)
    assert rc == E_BADARG


# ---------------------------------------------------------------------------------------------------------------
# GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("real32", [False, True], ids=["f64", "f32"])
def test_ragged_batch_and_special_multisets_match_numpy_median(real32):
    segs = segments()
    if real32:
        segs["two_far"] = np.array([-3e38, 3e38])      # (the ends of the float range)
        segs = {n: f32_values(v) for n, v in segs.items()}
    names = list(segs)
    off, vals = batch(names, segs)
    stats, rc = capi.mad_many(off, vals, None, real32=real32)
    want = want_stats(off, vals.astype(np.float32) if real32 else vals, None)
    for k, n in enumerate(names):
        print(f"{n}: {stats[k]}")
        assert same_bits(stats[k], want[k]), (n, stats[k], want[k])
    assert rc == 0 and capi.debug_eval_many_stats()[5] == 4 and capi.debug_eval_many_stats()[3] == len(names)
    k = names.index("equal")
    assert stats[k, 2] == 0.0 and stats[k, 1] == -2.5
    assert stats[names.index("half_equal"), 2] == 0.0 and stats[names.index("n0"), 0] == 0.0
    z = stats[names.index("signed_zero")]
    assert z[1] == 0.0 and not np.signbit(z[1]) and not np.signbit(z[2])      # -0 counts as +0


@pytest.mark.gpu
@pytest.mark.parametrize("real32", [False, True], ids=["f64", "f32"])
def test_wsel_with_zeros_over_nan(real32):
    rng = np.random.default_rng(9602)
    dt = np.float32 if real32 else np.float64
    sizes = [1, 7, 64, 65, 200, 513, 3, 0, 40]
    off = np.cumsum([0] + sizes).astype(np.int64)
    vals = rng.standard_normal(off[-1]).astype(dt)
    wsel = rng.uniform(0.5, 2.0, off[-1]).astype(dt)
    wsel[rng.random(off[-1]) < 0.3] = 0.0
    wsel[off[2]:off[3]][1::2] = -0.0          # (a negative zero is a zero)
    wsel[off[6]:off[7]] = 0.0                 # nothing counted
    wsel[off[8]:off[9]][:] = 0.0
    wsel[off[8] + 5] = -1.0                   # (a negative weight counts: it is not 0)
    vals[wsel == 0.0] = np.nan
    stats, rc = capi.mad_many(off, vals, wsel, real32=real32)
    want = want_stats(off, vals, wsel)
    assert rc == 0 and same_bits(stats, want), (stats, want)
    assert np.all(stats[6] == 0.0) and stats[8, 0] == 1 and stats[8, 2] == 0.0


@pytest.mark.gpu
def test_bits_do_not_depend_on_the_batch_the_position_the_order_or_the_entry():
    import torch
    segs = segments()
    names = ["n300", "tie", "n65", "zeros", "n0", "n1000", "negative", "tie_edge"]
    off, vals = batch(names, segs)
    stats, rc = capi.mad_many(off, vals)
    assert rc == 0
    rng = np.random.default_rng(9603)
    for k, n in enumerate(names):      # alone, and alone with its values permuted
        one, _ = capi.mad_many([0, segs[n].size], segs[n])
        perm, _ = capi.mad_many([0, segs[n].size], rng.permutation(segs[n]))
        assert same_bits(one[0], stats[k]) and same_bits(perm[0], stats[k]), n
    # reversed, with a first global index that is not 0 (NaN in front, never read)
    off2, vals2 = batch(names[::-1], segs, first=41)
    stats2, rc2 = capi.mad_many(off2, vals2)
    assert rc2 == 0 and same_bits(stats2, stats[::-1])
    # the _dev entries on the same layout, f64 and f32, with and without wsel
    for dt in (torch.float64, torch.float32):
        vd = torch.from_numpy(vals2).to(dt).cuda()
        sd = torch.full((len(names), 4), 7.0, dtype=torch.float64, device="cuda")
        assert capi.mad_many_dev(off2, vd, None, sd) == 0
        host, _ = capi.mad_many(off2, vd.cpu().numpy(), None, real32=dt == torch.float32)
        assert same_bits(sd.cpu().numpy(), host)
        if dt == torch.float64:
            assert same_bits(host, stats2)
        wsel = torch.from_numpy((rng.random(vals2.size) < 0.7).astype(np.float64)).to(dt).cuda()
        sd.fill_(7.0)
        assert capi.mad_many_dev(off2, vd, wsel, sd) == 0
        host, _ = capi.mad_many(off2, vd.cpu().numpy(), wsel.cpu().numpy(), real32=dt == torch.float32)
        assert same_bits(sd.cpu().numpy(), host)
        assert same_bits(host, want_stats(off2, vd.cpu().numpy(), wsel.cpu().numpy()))
    # a batch without points on the device: zeros
    sd.fill_(7.0)
    assert capi.mad_many_dev(np.array([3, 3, 3]), vd, None, sd) == 0
    assert np.all(sd.cpu().numpy()[:2] == 0.0) and np.all(sd.cpu().numpy()[2:] == 7.0)


@pytest.mark.gpu
def test_striding_gives_every_copy_the_bits_of_its_original():
    """More problems than workgroups: 5 000 copies of a 30-value segment interleaved with 5 000 of a 21-value one."""
    rng = np.random.default_rng(9604)
    a, b = rng.standard_normal(30), rng.standard_normal(21)
    one = [capi.mad_many([0, v.size], v)[0][0] for v in (a, b)]
    vals = np.concatenate([np.concatenate([a, b])] * 5000)
    off = np.concatenate([[0], np.cumsum(np.tile([30, 21], 5000))]).astype(np.int64)
    stats, rc = capi.mad_many(off, vals)
    st = capi.debug_eval_many_stats()
    assert rc == 0 and st[0] < 10000 and st[1] == 1 and st[3] == 10000
    assert np.all(stats[0::2] == one[0]) and np.all(stats[1::2] == one[1])
    assert same_bits(np.stack(one), want_stats([0, 30, 51], np.concatenate([a, b]), None))
