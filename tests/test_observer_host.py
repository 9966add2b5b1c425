"""Device-mode observer (nsol_amd/observer.py), the parts that need no GPU:
recognition of the measure lambdas through the symbolic probe, the observation
points and the host finaliser of the board sums."""
import numpy as np
import pytest

from oracle import nsol_oracle as orc

SHAPE = (6, 7, 8)
N = int(np.prod(SHAPE))


def _ops(spacing=None):
    import nsol_amd.linear_operators as LO
    lo = LO.LinearOperators3D() if spacing is None else \
        LO.LinearOperators3D(spacing=spacing)
    grad, _ = lo.get_gradient_operators()
    return grad, (lambda x: grad(x.reshape(*SHAPE)).flatten())


def test_probe_recognises_the_measures_as_callers_write_them():
    from nsol_amd.observer import classify, probe_measure
    from nsol_amd.prior_measures import PriorMeasures
    from nsol_amd.similarity_measures import SimilarityMeasures
    x_ref = np.random.default_rng(0).random(N)
    _, D_1D = _ops(spacing=np.array([1.0, 2.0, 4.0]))
    expected = {"SSD": "board", "SAD": "board", "MAE": "board", "MSE": "board",
                "RMSE": "board", "PSNR": "board", "NCC": "board",
                "SSIM": "ssim", "MI": "histogram", "NMI": "histogram"}
    for m, cls in expected.items():
        fn = lambda x, m=m: SimilarityMeasures.similarity_measures[m](x, x_ref)
        d = probe_measure(fn, N)
        assert d is not None and d.kind == m and d.ref is x_ref, m
        assert d.shape == (N,)
        assert classify(d) == cls, m
    d = probe_measure(lambda x: SimilarityMeasures.structural_similarity(
        x.reshape(SHAPE), x_ref.reshape(SHAPE), win_size=5), N)
    assert d.kind == "SSIM" and d.shape == SHAPE and d.ssim["win_size"] == 5
    d = probe_measure(lambda x: SimilarityMeasures.shannon_entropy(x, bins=20), N)
    assert (d.kind, d.bins, classify(d)) == ("entropy", 20, "histogram")
    d = probe_measure(lambda x: SimilarityMeasures.dice_score(x, x_ref > 0.5), N)
    assert (d.kind, classify(d)) == ("Dice", "histogram")
    priors = {
        "TK0": lambda x: PriorMeasures.zeroth_order_tikhonov(x),
        "TK1": lambda x: PriorMeasures.first_order_tikhonov(x, D_1D),
        "TV": lambda x: PriorMeasures.total_variation(x, D_1D, 3),
        "Huber": lambda x: PriorMeasures.huber(x, D_1D, 3, gamma=0.2),
    }
    for m, fn in priors.items():
        d = probe_measure(fn, N)
        assert d is not None and d.kind == m and classify(d) == "board", m
        if m != "TK0":
            assert d.grad[0] == "grad" and tuple(d.grad[2]) == SHAPE
            assert tuple(d.grad[1].w[:3]) == (1.0, 0.5, 0.25)
    assert probe_measure(priors["Huber"], N).gamma == 0.2
    assert probe_measure(priors["TV"], N).gamma is None


def test_probe_sends_foreign_callables_to_the_host():
    from nsol_amd.observer import classify, probe_measure
    from nsol_amd.prior_measures import PriorMeasures
    from nsol_amd.similarity_measures import SimilarityMeasures
    x_ref = np.ones(N)
    _, D_1D = _ops()
    foreign = [
        lambda x: float(np.sum(np.asarray(x) ** 2)),                 # NumPy
        lambda x: SimilarityMeasures.SSD(2.0 * x, x_ref),            # arithmetic
        lambda x: orc.sim_ssd(x, x_ref),                             # foreign code
        lambda x: SimilarityMeasures.SSD(x, x_ref[:-1]),             # bad shape
        lambda x: PriorMeasures.total_variation(x, D_1D, 2),         # wrong dim
        lambda x: PriorMeasures.total_variation(x, lambda v: np.gradient(v), 3),
        lambda x: SimilarityMeasures.SSD(x_ref, x),                  # probe as ref
    ]
    for fn in foreign:
        d = probe_measure(fn, N)
        assert d is None and classify(d) == "host"


@pytest.mark.parametrize("iterations, every, points", [
    (10, 3, [0, 3, 6, 9, 10]), (9, 3, [0, 3, 6, 9]), (5, 1, [0, 1, 2, 3, 4, 5]),
    (4, 10, [0, 4]), (1, 1, [0, 1]), (0, 3, [0])])
def test_observation_points(iterations, every, points):
    from nsol_amd.observer import Observer, observation_points
    assert observation_points(iterations, every) == points
    o = Observer(keep_iterates=False, every=every)
    assert o.get_every() == every and not o.get_keep_iterates()
    with pytest.raises(ValueError):
        o.set_every(0)


def test_observer_defaults_keep_the_reference_api():
    from nsol_amd.observer import Observer
    o = Observer()
    assert o.get_keep_iterates() and o.get_every() == 1
    assert o.get_measure_classes() == {}
    o.add_x(np.zeros(3))
    o.add_x(np.ones(3))
    o.set_measures({"s": lambda x: float(np.sum(x))})
    o.compute_measures()
    assert list(o.get_measures()["s"]) == [0.0, 3.0]
    assert o.get_observed_iterations() == [0, 1]


def _sums(xs, y, grad):
    """The 9 sums of nsol_observe_* in NumPy float64."""
    ybar = y.mean()
    d = xs - y
    g = grad(xs.reshape(SHAPE)).reshape(3, -1)
    n2 = g[0] ** 2 + g[1] ** 2 + g[2] ** 2
    gm = 0.05
    hub = np.where(n2 < gm * gm, n2, 2 * gm * np.sqrt(n2) - gm * gm) / (2 * gm)
    return np.array([np.sum(d * d), np.sum(np.abs(d)), np.sum(xs),
                     np.sum((xs - ybar) * (y - ybar)), np.sum((xs - ybar) ** 2),
                     np.sum(np.sqrt(n2)), np.sum(hub), np.sum(n2),
                     np.sum(xs * xs)])


@pytest.mark.parametrize("offset", [0.0, 40.0])
def test_finaliser_matches_the_oracle(offset):
    """offset: the reference's mean far from x's -- NCC goes through the shift
    from the reference's mean to x's own."""
    from nsol_amd.observer import finalise, reference_stats
    rng = np.random.default_rng(3)
    xs = rng.standard_normal(N) * 2.0 + 1.0
    y = xs + rng.standard_normal(N) * 0.7 + offset
    spacing = np.array([1.0, 1.0, 1.0])
    D = lambda v: orc.grad(v.reshape(SHAPE), spacing).reshape(-1)
    s = _sums(xs, y, lambda v: orc.grad(v, spacing))
    ybar = y.sum() / N
    ref = reference_stats(float(y.sum()), float(y.max()),
                          float(np.sum((y - ybar) ** 2)), N)
    want = {"SSD": orc.sim_ssd(xs, y), "SAD": orc.sim_sad(xs, y),
            "MAE": orc.sim_mae(xs, y), "MSE": orc.sim_mse(xs, y),
            "RMSE": orc.sim_rmse(xs, y), "PSNR": orc.sim_psnr(xs, y),
            "NCC": orc.sim_ncc(xs, y), "TK0": orc.prior_tk0(xs),
            "TK1": orc.prior_tk1(xs, D), "TV": orc.prior_tv(xs, D, 3),
            "Huber": orc.prior_huber(xs, D, 3)}
    for kind, v in want.items():
        got = finalise(kind, s, ref)
        assert got == pytest.approx(v, rel=1e-12, abs=0), kind
