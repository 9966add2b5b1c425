"""Stacked TGV deconvolution on the GPU: k_tgv_primal_lin_stack through the C ABI, bit for
bit against the single entry on every member's arrays and against the NumPy restatement
(tgv_numpy.primal_step_lin), with an open and a finite box; access paths, guard bands,
members that do not see each other, what the entry declines; TGVPrimalDualLinearBatch and
TGVPrimalDualLinearSweep against the members' own runs on every blur path; launch counts
and groups.  (test_tgv_linear_stack_host.py asserts that the finite box is at work.)"""
import functools

import numpy as np
import pytest

from conftest import rel_l2
from device_arena import Arena
from nsol_amd import tgv_numpy as tg
from test_pd_linear_host import box_kernel, gaussian_kernel
from test_pd_weighted_host import mixed_weights
from test_tgv_linear_gpu import _solver as _case_solver
from test_tgv_linear_gpu import _device_operators, _problem
from test_tgv_stack_gpu import (ALPHAS, BOTH, ITERS, MEMBER_BETAS, SHAPES, SPACING, TAU,
                                THETA, X_SCALES, _as_f64, _bytes_of, _dims, _fn, _gate, _iw,
                                _member, _obs, _raw, _suffix)
from tgv_lin_stack_cases import OPEN, finite_box, lin_state, want_lin

pytestmark = pytest.mark.gpu

LIN_ARRAYS = ("p", "q", "x", "xbar", "w", "wbar", "g")
WRITTEN = ("x", "xbar", "w", "wbar")
READ = ("p", "q", "g")


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


# ---- the single entry on one member's arrays: what every stacked member must equal
@functools.lru_cache(maxsize=None)
def _single_lin(shape, dtype, m, box):
    import torch
    from nsol_amd.device import stream_ptr
    s = lin_state(shape, dtype, m)
    ar = Arena({k: s[k] for k in LIN_ARRAYS}, dtype)
    assert _fn("tgv_primal_lin", dtype)(
        *[ar.ptr(k) for k in LIN_ARRAYS], *_dims(shape), *_iw(len(shape)), TAU, THETA,
        box[0], box[1], stream_ptr()) == 0
    torch.cuda.synchronize()
    return {k: _raw(ar.t[k]) for k in LIN_ARRAYS}


def _stacked(shape, dtype, P, poison=None):
    """The members' arrays one after the other.  poison: the member whose g, p and q are
    NaN."""
    out = {}
    for k in LIN_ARRAYS:
        parts = [lin_state(shape, dtype, m)[k].reshape(-1).copy() for m in range(P)]
        if poison is not None and k in READ:
            parts[poison][:] = np.nan
        out[k] = np.concatenate(parts)
    return out


def _check(shape, dtype, P, box, offset=0, last=None, poison=None):
    import torch
    from nsol_amd import ops
    from nsol_amd.device import stream_ptr
    host = _stacked(shape, dtype, P, poison)
    ar = Arena(host, dtype, offset, last)
    before = ops.tgv_stack_launches(), ops.tgv_launches()
    assert _fn("tgv_stack_primal_lin", dtype)(
        *[ar.ptr(k) for k in LIN_ARRAYS], P, *_dims(shape), *_iw(len(shape)), TAU, THETA,
        box[0], box[1], stream_ptr()) == 0
    torch.cuda.synchronize()
    assert (ops.tgv_stack_launches(), ops.tgv_launches()) == (before[0] + 1, before[1])
    got = {k: _raw(ar.t[k]) for k in LIN_ARRAYS}
    label = "lin stack %r P=%d box=%r off=%d last=%s" % (shape, P, box, offset, last)
    for m in range(P):
        if m == poison:
            continue
        want = _single_lin(shape, dtype, m, box)
        for k in LIN_ARRAYS:                            # all seven arrays, member by member
            assert np.array_equal(_member(got[k], m, P), want[k]), (label, m, k)
    assert ar.guards_intact(), label
    if poison is None:
        for k in READ:                                  # the inputs are only read
            assert np.array_equal(got[k], _bytes_of(host[k], dtype)), (label, k)
        m = P - 1                                       # the last member, restated
        want = want_lin(shape, dtype, m, box)
        errs = [rel_l2(_as_f64(_member(got[k], m, P), dtype, v.shape), v, label + " " + k)
                for k, v in zip(WRITTEN, want)]
        print("%s %s: x %.3g xbar %.3g w %.3g wbar %.3g" % ((label, _suffix(dtype)) +
                                                           tuple(errs)))
        assert max(errs) <= _gate(dtype)


# ------------------------------------------------------------ 1. the stacked kernel
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", BOTH)
def test_the_entry_has_the_single_entrys_bits(nsol, shape, dtype):
    for box in (OPEN, finite_box(shape, dtype)):
        for P in (1, 2, 3):
            _check(shape, dtype, P, box)


def test_the_finite_box_changes_what_the_kernel_writes(nsol):
    """(the box is not ignored: the finite one moves a third of the voxels or more)"""
    shape, dtype = (6, 259), np.float32
    a = _single_lin(shape, dtype, 0, OPEN)["x"].view(dtype)
    b = _single_lin(shape, dtype, 0, finite_box(shape, dtype))["x"].view(dtype)
    assert np.mean(a != b) > 0.5


# ----------------------------------------------------- 2. access paths and isolation
@pytest.mark.parametrize("shape", [(259,), (6, 259), (3, 5, 7), (5, 4, 64)])
@pytest.mark.parametrize("dtype", BOTH)
def test_arrays_off_16_byte_alignment(nsol, shape, dtype):
    """Every base 4 and 8 bytes off alignment (float64: 8): the ragged kernels, or the
    element kernels for short rows, whatever the row length."""
    offsets = (1, 2) if dtype is np.float32 else (1,)
    for offset in offsets:
        assert (offset * np.dtype(dtype).itemsize) % 16 in (4, 8)
        for P in (2, 3):
            _check(shape, dtype, P, finite_box(shape, dtype), offset=offset)


@pytest.mark.parametrize("shape", [(259,), (6, 259), (3, 5, 7), (5, 4, 64)])
@pytest.mark.parametrize("dtype", BOTH)
def test_stacks_that_end_with_their_allocation(nsol, shape, dtype):
    """Every stacked array in turn ends exactly where the device allocation ends: the last
    rows of the LAST member's last component have nothing of the array behind them."""
    for last in LIN_ARRAYS:
        _check(shape, dtype, 3, finite_box(shape, dtype), last=last)


@pytest.mark.parametrize("shape", [(259,), (6, 259), (3, 5, 7), (5, 4, 64)])
@pytest.mark.parametrize("dtype", BOTH)
def test_a_member_of_nans_leaves_its_neighbours_alone(nsol, shape, dtype):
    """NaN throughout member 1's g, p and q: members 0 and 2 keep the bits of their clean
    run and the guard bands their sentinels."""
    _check(shape, dtype, 3, OPEN, poison=1)
    _check(shape, dtype, 3, finite_box(shape, dtype), poison=1, offset=1)


# ------------------------------------------------------------------------ 3. declines
@pytest.mark.parametrize("dtype", BOTH)
def test_the_entry_declines(nsol, dtype):
    import torch
    from nsol_amd import ops
    from nsol_amd.device import stream_ptr, to_device
    entry = _fn("tgv_stack_primal_lin", dtype)
    shape, P = (3, 4, 6), 2
    n = 3 * 4 * 6
    mk = lambda k: to_device(np.full(k * P * n, 0.25), dtype)
    p, q, x, xbar, w, wbar, g = mk(3), mk(6), mk(1), mk(1), mk(3), mk(3), mk(1)
    good = (p, q, x, xbar, w, wbar, g)
    ptr = lambda t: None if t is None else t.data_ptr()

    def call(a=good, members=P, dims=(3,) + shape, tau=0.3, theta=1., lo=-np.inf,
             hi=np.inf):
        return entry(*[ptr(t) for t in a], members, *dims, 1., 1., 1., tau, theta, lo, hi,
                     stream_ptr())

    before = ops.tgv_stack_launches(), ops.tgv_launches()
    for members in (0, 65536, -1):                       # declined, nothing launched
        assert call(members=members) == -2
    for dims in ((3, 1 << 11, 1 << 11, 1 << 10), (1, 1, 1, (1 << 31) + 1)):
        assert call(dims=dims) == -2
    for k in range(7):                                   # a missing pointer
        a = list(good)
        a[k] = None
        assert call(a) == -1, k
    for i in range(7):                                   # two arguments that alias
        for j in range(i):
            a = list(good)
            a[i] = a[j]
            assert call(a) == -1, (i, j)
    # ... or overlap only because the spans are `members` times as long
    assert call((p, q, x[:n], x[n:], w, wbar, g)) == -1
    assert call((p, q, x, xbar, w, wbar[:3 * n], wbar[3 * n:][:n])) == -1
    assert call(lo=1., hi=0.5) == -1 and call(lo=np.nan) == -1 and call(hi=np.nan) == -1
    for bad in (0., -1., np.inf, np.nan):
        assert call(tau=bad) == -1, bad
    assert call(theta=np.nan) == -1
    for dims in ((0,) + shape, (4,) + shape, (3, -1, 4, 6)):
        assert call(dims=dims) == -1, dims
    # an extent of 0: nothing to do, whatever else is passed
    for dims in ((3, 0, 4, 6), (3, 3, 0, 6), (1, 1, 1, 0)):
        assert call(dims=dims) == 0 and call((None,) * 7, dims=dims) == 0
    assert (ops.tgv_stack_launches(), ops.tgv_launches()) == before
    torch.cuda.synchronize()
    for t in good:
        assert torch.equal(t, torch.full_like(t, 0.25))
    # the good calls run, one count each
    assert call() == 0 and call(lo=0., hi=0.) == 0 and call(theta=0.) == 0
    assert call((p, q, x[:n], x[n:], w[:3 * n], wbar[:3 * n], g[:n]), members=1) == 0
    torch.cuda.synchronize()
    assert (ops.tgv_stack_launches(), ops.tgv_launches()) == (before[0] + 4, before[1])
    # the Python wrapper checks its operands before the library sees them
    iw = (1., 1., 1.)
    with pytest.raises(ValueError):
        ops.tgv_stack_primal_lin(p, q, x, xbar, w, wbar, g[:n], P, shape, iw, 0.3)
    with pytest.raises(ValueError):
        ops.tgv_stack_primal_lin(p, q[:3 * n], x, xbar, w, wbar, g, P, shape, iw, 0.3)
    with pytest.raises(ValueError):
        ops.tgv_stack_primal_lin(p, q, x, xbar, w, wbar, g, P, shape, iw, -1.)
    assert ops.tgv_stack_primal_lin(p, q, x, xbar, w, wbar, g, 0, shape, iw, 0.3) is False
    v = [t._version for t in (x, xbar, w, wbar)]
    assert ops.tgv_stack_primal_lin(p, q, x, xbar, w, wbar, g, P, shape, iw, 0.3) is True
    assert [t._version for t in (x, xbar, w, wbar)] == [k + 1 for k in v]


# --------------------------------------------------------------------------- 4. batch
@pytest.fixture
def data_side(monkeypatch):
    """Counts the launches of the data term's side: {"stacked": the calls of
    ops.pdl_stack_dual_data that the library took, "single": the calls of
    ops.pdl_dual_data}.  The library counts neither kernel: nsol_pdl_stack_launches and
    nsol_pdl_launches count the tile kernels k_pdl_stack / k_pdl alone -- which a TGV run
    never launches, so both stay where they are -- and every call of the wrapper is one
    launch."""
    from nsol_amd import ops
    calls = {"stacked": 0, "single": 0}
    real_stacked, real_single = ops.pdl_stack_dual_data, ops.pdl_dual_data

    def stacked(*a, **k):
        ok = real_stacked(*a, **k)
        calls["stacked"] += bool(ok)
        return ok

    def single(*a, **k):
        calls["single"] += 1
        return real_single(*a, **k)
    monkeypatch.setattr(ops, "pdl_stack_dual_data", stacked)
    monkeypatch.setattr(ops, "pdl_dual_data", single)
    return calls


def _tiles():
    """(the stacked, the single) tile kernels' launches: no TGV run moves them."""
    from nsol_amd import ops
    return ops.pdl_stack_launches(), ops.pdl_launches()


def _wrapped(op, shape):
    return lambda x: op(x.reshape(*shape)).flatten()


def _weights(shape, k):
    return mixed_weights(shape, k).flatten()


def _member_solver(nsol, shape, dtype, k, op, **kw):
    """Member k of a list: its own observation, alpha, beta and x_scale; the operator
    behind lambdas on the flat vector, as a caller writes it."""
    obs = _obs(shape, k)
    args = dict(A=_wrapped(op, shape), A_adj=_wrapped(op, shape), b=obs.flatten(),
                x0=obs.flatten(), dimension=len(shape), spacing=SPACING[:len(shape)],
                alpha=ALPHAS[k], beta=MEMBER_BETAS[k], iterations=ITERS,
                x_scale=X_SCALES[k], dtype=dtype)
    args.update(kw)
    return nsol.TGVPrimalDualLinearSolver(**args)


def _restated_member(solver, shape, k, taps, **kw):
    from scipy.ndimage import convolve
    obs = _obs(shape, k)
    blur = lambda x: convolve(np.asarray(x, np.float64).reshape(shape), taps, mode="wrap")
    return tg.iterate_linear(blur, blur, obs.reshape(-1) / X_SCALES[k], obs / X_SCALES[k],
                             ITERS, ALPHAS[k], MEMBER_BETAS[k], SPACING[:len(shape)],
                             A_norm2=solver.get_A_norm2(), **kw)


def _assert_members_are_own_runs(solvers, own, label):
    for k, (s, f) in enumerate(zip(solvers, own)):
        assert np.array_equal(s.get_x(), f.get_x()), (label, k)
        assert np.array_equal(s.get_w(), f.get_w()), (label, k)
        assert np.array_equal(s.get_x_device().cpu().numpy(),
                              f.get_x_device().cpu().numpy()), (label, k)
        assert s.get_iterations_done() == f.get_iterations_done(), (label, k)
        assert s.get_stop_reason() == f.get_stop_reason(), (label, k)
        assert s.get_execution() == f.get_execution(), (label, k)
        assert np.abs(s.get_w()).max() > 0, (label, k)


def _against(s, want, k, dtype, label):
    ex = rel_l2(s.get_x(), want["x"] * X_SCALES[k], label + " x")
    ew = rel_l2(s.get_w(), want["w"] * X_SCALES[k], label + " w")
    print("%s %s: x %.3g w %.3g" % (label, _suffix(dtype), ex, ew))
    assert ex <= _gate(dtype) and ew <= _gate(dtype)


BATCH_CASES = [
    # a stacked 1-D blur
    ((1031,), "gauss", dict(), 5),
    # two stacked passes
    ((37, 50), "gauss", dict(isotropic=True, data_loss="ell1", bounds=(0., np.inf)), 7),
    # 3-D, member by member; slices not on 16 bytes
    ((5, 7, 9), "box", dict(), 2 * 6 + 3)]


@pytest.mark.parametrize("shape, kernel, kw, launches", BATCH_CASES,
                         ids=lambda v: str(v).replace(" ", "") if isinstance(v, tuple)
                         else None)
@pytest.mark.parametrize("dtype", BOTH)
def test_batch_members_are_their_own_runs(nsol, data_side, shape, kernel, kw, launches,
                                          dtype):
    from nsol_amd import ops
    from nsol_amd.linear_operators import ConvolutionOperator
    from nsol_amd.tgv_linear_stack import launches_per_iteration
    P, d = 6, len(shape)
    taps = box_kernel(d) if kernel == "box" else gaussian_kernel(d, 1.)
    weighted = "bounds" in kw

    def make():
        return [_member_solver(nsol, shape, dtype, k, ConvolutionOperator(d, taps),
                               weights=_weights(shape, k) if weighted else None, **kw)
                for k in range(P)]
    own, solvers = make(), make()
    for f in own:
        before = ops.tgv_launches()
        f.run()
        assert ops.tgv_launches() - before == 2 * ITERS
    assert launches_per_iteration(solvers[0], P)[0] == launches
    if d == 3:
        assert (int(np.prod(shape)) * np.dtype(dtype).itemsize) % 16 != 0
    assert data_side == dict(stacked=0, single=P * ITERS)
    batch = nsol.TGVPrimalDualLinearBatch(solvers)
    before = ops.tgv_stack_launches(), ops.tgv_launches(), _tiles()
    batch.run()
    assert batch.get_execution() == ["stacked"] * P and batch.get_group_size() == P
    assert ops.tgv_stack_launches() - before[0] == 2 * ITERS
    assert data_side == dict(stacked=ITERS, single=P * ITERS)
    assert ops.tgv_launches() == before[1] and _tiles() == before[2]
    label = "batch %r %s" % (shape, kernel)
    _assert_members_are_own_runs(solvers, own, label)
    assert solvers[0].get_execution() == "fused"
    assert solvers[0].get_iterations_done() == ITERS
    assert solvers[0].get_stop_reason() == "iterations"
    X = batch.get_x_all_device().cpu().numpy()
    for k, f in enumerate(own):
        assert np.array_equal(X[k], f.get_x_device().cpu().numpy())
    k = P - 1                                           # the last member, restated
    want = _restated_member(
        solvers[k], shape, k, taps, data_loss=kw.get("data_loss", "ell2"),
        isotropic=kw.get("isotropic", False), bounds=kw.get("bounds"),
        weights=_weights(shape, k) if weighted else None)
    _against(solvers[k], want, k, dtype, label)
    if weighted:
        assert solvers[k].get_x().min() >= 0.


def test_batch_on_the_blur_epilogue_path(nsol, monkeypatch):
    """The one-pass blur's epilogue on and off: under each setting every member has the
    bits of its own run under that setting."""
    from nsol_amd import linear_operators as LO, ops
    shape, dtype, P = (20, 37, 64), np.float32, 6
    A, _ = LO.LinearOperators3D().get_gaussian_blurring_operators(np.diag([2.] * 3))
    ran = []
    real = ops.corr3_wrap_axpby

    def counted(*a, **k):
        out = real(*a, **k)
        ran.append(out is not None)
        return out
    monkeypatch.setattr(ops, "corr3_wrap_axpby", counted)
    make = lambda: [_member_solver(nsol, shape, dtype, k, A) for k in range(P)]
    last = {}
    for on in (True, False):
        monkeypatch.setattr(LO, "USE_BLUR_EPILOGUE", on)
        own, solvers = make(), make()
        for f in own:
            f.run()
        del ran[:]
        batch = nsol.TGVPrimalDualLinearBatch(solvers)
        batch.run()
        assert batch.get_execution() == ["stacked"] * P
        # the epilogue ran for every member in every iteration, or never
        assert ran == ([True] * (ITERS * P) if on else [])
        _assert_members_are_own_runs(solvers, own, "epilogue=%d" % on)
        last[on] = solvers[P - 1]
    want = _restated_member(last[True], shape, P - 1, A.kernel)
    for on in (True, False):
        _against(last[on], want, P - 1, dtype, "epilogue=%d %r" % (on, shape))


def test_mixed_input_stacks_what_agrees_and_runs_the_rest(nsol):
    """Solvers that differ in `isotropic` or in their bounds form stacks of their own; a
    tolerance, a blur-and-sample pair and a pair of opaque device callables run on their
    own.  All of them answer as after their own run()."""
    from nsol_amd import ops
    from nsol_amd.device import is_device_tensor
    shape, dtype = (5, 7), np.float64
    obs, _, _, _, _ = _problem(shape, False)
    A, At = _device_operators(shape, False)

    def opaque(op):
        def f(t):
            if not is_device_tensor(t):
                raise TypeError("device tensors only")
            return op(t.view(*shape)).reshape(-1)
        return f

    def build():
        mk = lambda **kw: _case_solver(nsol, shape, dtype, **kw)
        return [mk(alpha=0.1, beta=0.8), mk(iso=True), mk(bounds=(0.25, 0.85)),
                mk(alpha=0.5), mk(iso=True, beta=3.0), mk(bounds=(0.25, 0.85), alpha=0.7),
                mk(tolerance=1e-3, check_every=5), mk(sampled=True),
                mk(A=opaque(A), A_adj=opaque(At), A_norm2=1.)]
    solvers, own = build(), build()
    for f in own:
        f.run()
    batch = nsol.TGVPrimalDualLinearBatch(solvers)
    before = ops.tgv_stack_launches()
    batch.run()
    assert batch.get_execution() == ["stacked"] * 6 + ["sequential"] * 3
    assert batch.get_group_size() == 2
    assert ops.tgv_stack_launches() - before == 3 * 2 * 25          # three stacks of two
    assert [s.get_execution() for s in solvers] == ["fused"] * 8 + ["device"]
    _assert_members_are_own_runs(solvers, own, "mixed")
    assert len(solvers[6].get_changes()) == len(own[6].get_changes()) > 0
    # the stacks did not mix their members up: the three pairs differ from one another
    assert not np.array_equal(solvers[0].get_x(), solvers[3].get_x())
    assert not np.array_equal(solvers[0].get_x(), solvers[1].get_x())


# --------------------------------------------------------------------------- 5. sweep
@pytest.mark.parametrize("dtype, weighted", [(np.float64, False), (np.float32, True)])
def test_sweep_members_are_single_solvers(nsol, data_side, dtype, weighted):
    from nsol_amd import ops
    from nsol_amd.linear_operators import ConvolutionOperator
    from nsol_amd.observer import Observer, observation_points
    from nsol_amd.similarity_measures import SimilarityMeasures as sm
    shape = (16, 20, 24)
    obs, truth = _obs(shape).flatten(), _obs(shape, 99).flatten()
    op = ConvolutionOperator(3, gaussian_kernel(3, 1.))
    measures = {k: (lambda x, k=k: sm.similarity_measures[k](x, truth))
                for k in ("PSNR", "SSD")}
    kw = dict(A=_wrapped(op, shape), A_adj=_wrapped(op, shape), b=obs, x0=obs, dimension=3,
              spacing=SPACING, iterations=ITERS, x_scale=2.0, dtype=dtype, isotropic=True,
              bounds=(0., np.inf), weights=_weights(shape, 3) if weighted else None)
    grid = {"alpha": [0.1, 0.4], "beta": [0.8, 1.7, 3.0]}
    sweep = nsol.TGVPrimalDualLinearSweep(parameters=grid, **kw)
    sweep.set_measures(measures, every=10)
    before = ops.tgv_stack_launches(), ops.tgv_launches(), _tiles()
    sweep.run()
    assert sweep.get_execution() == "stacked" and sweep.get_group_size() == 6
    assert ops.tgv_stack_launches() - before[0] == 2 * ITERS
    assert data_side == dict(stacked=ITERS, single=0)
    assert ops.tgv_launches() == before[1] and _tiles() == before[2]
    members = [dict(alpha=a, beta=b) for a in grid["alpha"] for b in grid["beta"]]
    assert sweep.get_parameters() == members                 # product order
    assert sweep.get_iterations_done() == [ITERS] * 6
    assert sweep.get_observed_iterations() == observation_points(ITERS, 10)
    got = sweep.get_measures()
    X = sweep.get_x_all_device().cpu().numpy()
    for m, member in enumerate(members):
        s = nsol.TGVPrimalDualLinearSolver(**dict(kw, **member))
        o = Observer(keep_iterates=False, every=10)
        o.set_measures(measures)
        s.set_observer(o)
        s.run()
        o.compute_measures()
        assert np.array_equal(sweep.get_x(m), s.get_x()), member
        assert np.array_equal(sweep.get_w(m), s.get_w()), member
        assert np.array_equal(X[m], s.get_x_device().cpu().numpy())
        for name in measures:
            assert got[name].shape == (6, 4)
            assert np.array_equal(got[name][m], o.get_measures()[name]), (name, member)
    k, best = sweep.best("PSNR")
    assert k == int(np.argmax(got["PSNR"][:, -1])) and best == members[k]
    assert sweep.best("SSD", mode="min")[0] == int(np.argmin(got["SSD"][:, -1]))
    # alpha and beta both act: the members at the ends of either list differ
    last = got["PSNR"][:, -1]
    assert last[0] != last[3] and last[0] != last[2] and last[3] != last[5]


def test_sweep_with_a_tolerance_runs_sequentially(nsol):
    from nsol_amd import ops
    from nsol_amd.linear_operators import ConvolutionOperator
    shape, dtype = (16, 20, 24), np.float64
    obs = _obs(shape).flatten()
    op = ConvolutionOperator(3, gaussian_kernel(3, 1.))
    kw = dict(A=_wrapped(op, shape), A_adj=_wrapped(op, shape), b=obs, x0=obs, dimension=3,
              spacing=SPACING, iterations=40, x_scale=2.0, dtype=dtype, tolerance=1e-3,
              check_every=5)
    grid = {"beta": [0.8, 3.0], "alpha": [0.1, 0.4]}
    sweep = nsol.TGVPrimalDualLinearSweep(parameters=grid, **kw)
    before = ops.tgv_stack_launches()
    sweep.run()
    assert sweep.get_execution() == "sequential" and sweep.get_group_size() is None
    assert ops.tgv_stack_launches() == before
    members = sweep.get_parameters()
    assert members == [dict(beta=b, alpha=a) for b in grid["beta"] for a in grid["alpha"]]
    done = sweep.get_iterations_done()
    for m, member in enumerate(members):
        s = nsol.TGVPrimalDualLinearSolver(**dict(kw, **member))
        s.run()
        assert np.array_equal(sweep.get_x(m), s.get_x()), member
        assert np.array_equal(sweep.get_w(m), s.get_w()), member
        assert done[m] == s.get_iterations_done()


# ------------------------------------------------------- 6. launch counts and groups
def test_launch_counts_and_groups_that_leave_the_same_bits(nsol, data_side, monkeypatch):
    """Over a run of five members, per iteration and group: two launches of the stacked TGV
    kernels, one of the stacked update of r, none of the single TGV kernels.  (The data
    side's launches are counted at ops.pdl_stack_dual_data -- see data_side: the library's
    own nsol_pdl_stack_launches counts the tile kernel of PrimalDualLinearSolver's stack,
    which never runs here, and is asserted to stay where it is.)"""
    from nsol_amd import ops
    from nsol_amd.linear_operators import ConvolutionOperator
    shape, dtype, P = (37, 50), np.float32, 5
    taps = gaussian_kernel(2, 1.)
    n = 37 * 50
    # a member here owns x, xbar; w, wbar, p; q; r, g; its b~ and t = A xbar
    per_member = (2 + 3 * 2 + 3 + 2 + 2) * n * 4
    assert ops.tgv_lin_stack_group_size(1 << 20, n, 2, 4, own_data=True, with_t=True) == \
        ops.TGV_STACK_GROUP_BYTES // per_member
    runs = {}
    for name, budget in (("one", ops.TGV_STACK_GROUP_BYTES),
                         ("2 + 2 + 1", 2 * per_member + per_member // 2)):
        monkeypatch.setattr(ops, "TGV_STACK_GROUP_BYTES", budget)
        solvers = [_member_solver(nsol, shape, dtype, k, ConvolutionOperator(2, taps))
                   for k in range(P)]
        batch = nsol.TGVPrimalDualLinearBatch(solvers)
        before = ops.tgv_stack_launches(), data_side["stacked"], ops.tgv_launches(), \
            _tiles()
        batch.run()
        assert batch.get_execution() == ["stacked"] * P
        assert _tiles() == before[3] and data_side["single"] == 0
        runs[name] = ([(s.get_x(), s.get_w()) for s in solvers], batch.get_group_size(),
                      ops.tgv_stack_launches() - before[0],
                      data_side["stacked"] - before[1], ops.tgv_launches() - before[2])
    assert runs["one"][1:] == (5, 2 * ITERS, ITERS, 0)
    assert runs["2 + 2 + 1"][1:] == (2, 2 * ITERS * 3, ITERS * 3, 0)
    for (xa, wa), (xb, wb) in zip(runs["one"][0], runs["2 + 2 + 1"][0]):
        assert np.array_equal(xa, xb) and np.array_equal(wa, wb)
