"""The float64 reference of the observation kernels' tests (observe_cases.py) anchored
on what exists already -- the oracle's measures -- and the conditions its planted inputs
must meet, on the CPU.  test_observe_kernels_gpu.py holds the kernels to this reference.
"""
import math

import numpy as np
import pytest

import observe_cases as oc
import vector_cases as vc
from oracle import nsol_oracle as orc

ANCHOR_SHAPES = [(1031,), (6, 259), (7, 10, 13)]


def _close(got, want, rtol, label):
    print("%s: got %.17g want %.17g rel %.3g" % (label, got, want,
                                                 abs(got - want) / max(abs(want), 1e-300)))
    assert abs(got - want) <= rtol * abs(want), label


@pytest.mark.parametrize("shape", ANCHOR_SHAPES)
@pytest.mark.parametrize("spacing", oc.SPACINGS)
def test_reference_sums_reproduce_the_oracles_measures(shape, spacing):
    d = len(shape)
    x = oc.smooth_field(shape, np.float64)
    y = oc.reference_for(x, 1.0, np.float64)
    w = oc.weights(spacing)
    gamma = oc.median_gamma(x, 1.0, shape, w, d, np.float64)
    flags = oc.PAIR | oc.GRAD | oc.SQ | oc.HUBER
    s, terms = oc.observe_sums_ref(x, 1.0, y, 0.0, shape, w, gamma, flags, d, np.float64)
    D, _ = orc.flat_operators(shape, spacing[:d])
    xf, yf = x.reshape(-1), y.reshape(-1)
    _close(s[0], orc.sim_ssd(xf, yf), 1e-13, "SSD")
    _close(s[1], orc.sim_sad(xf, yf), 1e-13, "SAD")
    _close(s[5], orc.prior_tv(xf, D, d), 1e-13, "TV")
    _close(s[6], orc.prior_huber(xf, D, d, gamma), 1e-13, "Huber")
    _close(0.5 * s[7], orc.prior_tk1(xf, D), 1e-13, "TK1")
    _close(0.5 * s[8], orc.prior_tk0(xf), 1e-13, "TK0")
    # both Huber branches are taken by this gamma
    n2 = terms[7]
    assert 0.2 <= np.mean(n2 < gamma * gamma) <= 0.8


def test_sums_not_asked_for_are_exactly_zero_and_huber_alone_is_ignored():
    shape = (5, 7)
    x = oc.smooth_field(shape, np.float32)
    y = oc.reference_for(x, 1.0, np.float32)
    for flags in oc.FLAG_SETS:
        s, terms = oc.observe_sums_ref(x, 1.0, y, 0.25, shape, (1., 1., 1.), 0.5, flags, 2,
                                       np.float32)
        for k in range(oc.SUMS):
            asked = (flags & oc.GROUP[k]) == oc.GROUP[k]
            assert (terms[k] is not None) == asked, (flags, k)
            if not asked:
                assert s[k] == 0.0 and not np.signbit(s[k])
    s, _ = oc.observe_sums_ref(x, 1.0, y, 0.25, shape, (1., 1., 1.), 0.5, oc.HUBER, 2,
                               np.float32)
    assert not s.any()


def test_the_scale_is_rounded_to_the_element_type_first():
    """0.1 is no float32: T(x) * T(0.1) differs from the float64 product rounded once."""
    x = oc.smooth_field((259,), np.float32)
    got = oc.widen(x, 0.1, np.float32)
    assert np.array_equal(got, (x.astype(np.float32) * np.float32(0.1)).astype(np.float64))
    assert np.any(got != (x * 0.1).astype(np.float32).astype(np.float64))
    assert np.array_equal(oc.widen(x, 0.1, np.float64), x * 0.1)


@pytest.mark.parametrize("shape", ANCHOR_SHAPES)
def test_finalised_sums_give_the_oracles_psnr_and_ncc(shape):
    from nsol_amd.observer import finalise, reference_stats
    x = oc.smooth_field(shape, np.float64)
    y = oc.reference_for(x, 1.0, np.float64)
    xf, yf = x.reshape(-1), y.reshape(-1)
    n = xf.size
    ybar = math.fsum(yf) / n
    ref = reference_stats(math.fsum(yf), float(yf.max()), math.fsum((yf - ybar) ** 2), n)
    s, _ = oc.observe_sums_ref(x, 1.0, y, ref["mean"], shape, (1., 1., 1.), 1.0, oc.PAIR,
                               len(shape), np.float64)
    _close(finalise("PSNR", s, ref), orc.sim_psnr(xf, yf), 1e-13, "PSNR")
    _close(finalise("NCC", s, ref), orc.sim_ncc(xf, yf), 1e-12, "NCC")
    _close(finalise("MSE", s, ref), orc.sim_mse(xf, yf), 1e-13, "MSE")
    _close(finalise("MAE", s, ref), orc.sim_mae(xf, yf), 1e-13, "MAE")


def test_ncc_where_the_shift_to_the_iterates_own_mean_cancels():
    """mean(x) - ybar = 1000 std(x): finalise forms sum (x - xbar)^2 as S4 - 2 d S2' +
    n d^2 with d = xbar - ybar, three terms a factor (d / std)^2 = 10^6 above their sum,
    and sum (x - xbar)(y - ybar) as S3 - d cs with terms a factor d / std above theirs.
    Every term carries a few unit roundoffs (the sums themselves are exact here: fsum),
    so NCC from exact sums is good to about (d / std)^2 2^-53 = 1e-10 at worst and no
    better: the floor of any gate on a device NCC of such an iterate.  Measured with this
    input: relative error 4.5e-13, against 3.6e-16 for the same x without the offset
    (bound asserted: 16 (d / std)^2 2^-53 = 1.8e-9)."""
    from nsol_amd.observer import finalise, reference_stats
    shape = (7, 10, 13)
    rng = np.random.default_rng(5)
    y = rng.standard_normal(shape)
    x0 = 0.7 * y + 0.3 * rng.standard_normal(shape)
    x = x0 + 1000.0 * x0.std()
    xf, yf = x.reshape(-1), y.reshape(-1)
    n = xf.size
    ybar = math.fsum(yf) / n
    ref = reference_stats(math.fsum(yf), float(yf.max()), math.fsum((yf - ybar) ** 2), n)
    s, _ = oc.observe_sums_ref(x, 1.0, y, ref["mean"], shape, (1., 1., 1.), 1.0, oc.PAIR,
                               3, np.float64)
    ratio = (xf.mean() - ybar) / xf.std()
    assert 900.0 < ratio < 1100.0
    got, want = finalise("NCC", s, ref), orc.sim_ncc(xf, yf)
    rel = abs(got - want) / abs(want)
    print("NCC at (mean(x) - ybar) / std(x) = %.4g: got %.17g want %.17g, relative error "
          "%.3g of the float64 reference alone" % (ratio, got, want, rel))
    assert rel <= 16.0 * ratio * ratio * vc.U64
    # without the offset the same sums give NCC to the last places
    s0, _ = oc.observe_sums_ref(x0, 1.0, y, ref["mean"], shape, (1., 1., 1.), 1.0, oc.PAIR,
                                3, np.float64)
    _close(finalise("NCC", s0, ref), orc.sim_ncc(x0.reshape(-1), yf), 1e-13, "NCC, no offset")


HUBER_SHAPES = [s for s in oc.SHAPES if int(np.prod(s)) >= 35]


@pytest.mark.parametrize("shape", HUBER_SHAPES)
def test_the_huber_field_sits_on_both_branches_on_the_corner_and_on_zero(shape):
    x = oc.huber_field(shape)
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    sh = oc.huber_shares(x, shape)
    print(shape, sh)
    assert sh["below"] >= 0.2 and sh["above"] >= 0.2 and sh["on"] >= 1 and sh["zero"] >= 1
    # the two forms agree on the corner, so the side the corner is put on does not show
    g = oc.HUBER_GAMMA
    assert 2.0 * g * math.sqrt(g * g) - g * g == g * g


def test_the_cancelling_field_cancels():
    for ybar in (0.0, 1024.0):
        for dtype in (np.float32, np.float64):
            x, y = oc.cancelling_field((6, 259), dtype, ybar)
            _, t = oc.observe_sums_ref(x, 1.0, y, ybar, (6, 259), (1., 1., 1.), 1.0,
                                       oc.PAIR, 2, dtype)
            for k in oc.SIGNED:
                if k == 2 and ybar != 0.0:
                    continue
                assert abs(math.fsum(t[k])) <= 1e-3 * np.sum(np.abs(t[k])), (ybar, k)


def test_trip_counts_and_pitches():
    # two workgroups: 512 voxels per stride, whole steps of four strides
    assert oc.obs_trips(1, 2) == 4 and oc.obs_trips(2048, 2) == 4
    assert oc.obs_trips(2049, 2) == 8 and oc.obs_trips(4 * 6 * 259, 2) == 16
    # the library's default grid: the second unrolled step of 2048 * 256 * 4 + 5
    assert oc.obs_trips(2048 * 256 * 4, 2048) == 4
    assert oc.obs_trips(2048 * 256 * 4 + 5, 2048) == 8
    assert oc.pitches(259, np.float32) == (260, 262, 260)
    assert oc.pitches(64, np.float32) == (65, 67, 68)
    assert oc.pitches(64, np.float64) == (65, 67, 66)
    p = oc.pitched(np.arange(6.).reshape(2, 3), (2, 3), 5, -1.0)
    assert p.tolist() == [0, 1, 2, -1, -1, 3, 4, 5, -1, -1]


def test_closed_form_of_a_periodic_line_equals_the_sums_of_the_line_itself():
    rng = np.random.default_rng(9)
    px = vc.rounded(rng.standard_normal(17), np.float32)
    py = vc.rounded(rng.standard_normal(17), np.float32)
    for n in (17 * 5, 17 * 5 + 6, 17 * 5 + 1):
        reps = -(-n // 17)
        x, y = np.tile(px, reps)[:n], np.tile(py, reps)[:n]
        want, terms = oc.observe_sums_ref(x, 37.5, y, 0.25, (n,), (1.3, 1., 1.), 1.0,
                                          oc.PAIR | oc.GRAD | oc.SQ, 1, np.float32)
        got, mags = oc.periodic_sums(px, py, n, 37.5, 0.25, 1.3, np.float32)
        for k in range(oc.SUMS):
            assert got[k] == want[k], (n, k)
            if terms[k] is not None:
                assert mags[k] >= np.sum(np.abs(terms[k])) * (1 - 1e-15)
