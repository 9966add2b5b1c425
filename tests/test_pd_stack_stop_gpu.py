"""Stacked runs that stop member by member on a real MI355X: the member-mapped kernels
k_pd_stack / k_pd_stack_iso (nsol_pdm.hip) through ops.pd_stack_iter against the
stacked and single-run kernels, the per-member sums, and PrimalDualBatch /
PrimalDualSweep(stacked_stopping=True) against the float64 restatement of
test_pd_stop_host.py and against every member's own run()."""
import itertools

import numpy as np
import pytest

from test_pd_stop_host import K, pd_stop_denoise
from test_pd_weighted_host import mixed_weights

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-12     # identical non-negative float64 summands, another order
ITERS = 60

# The stacked kernels plan tiles of TX x 16 voxels (one row per lane at these sizes,
# 16 lanes along x; TX = 64 in float32, 32 in float64, also in the ragged form) and z
# chunks of 2 planes.  The last three shapes make one member span several workgroups:
#   (150,)       3 (float32) / 5 (float64) workgroups along x
#   (37, 150)    3 tiles along y times 3 / 5 along x
#   (5, 20, 70)  2 tiles along y, 2 / 3 along x, 3 z chunks (2 + 2 + 1 planes)
#   (260, 9)     17 tiles along y: the XCD map deals them in slabs of 3 to 8 XCDs,
#                24 workgroups, 7 of them without a tile (their partials are zeros)
SHAPES = [(37,), (9, 20), (7, 13), (5, 6, 8), (4, 5, 7),
          (150,), (37, 150), (5, 20, 70), (260, 9)]
_ids = lambda s: "x".join(map(str, s))


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


# ------------------------------------------------------------------ kernel level
SIGMA, TAU, THETA, GAMMA = 0.31, 0.27, 0.93, 0.05
W = (1.0, 1.0, 1.0)


def _flags(huber, l1, iso, wgt):
    from nsol_amd import ops
    return (ops.PD_REG_HUBER if huber else ops.PD_REG_TV) | \
        (ops.PD_DATA_L1 if l1 else ops.PD_DATA_L2) | \
        (ops.PD_REG_ISOTROPIC if iso else 0) | (ops.PD_DATA_WEIGHTED if wgt else 0)


class _State(object):
    """Random x, xbar, p, bt, wt of P members and their scalars, one per member."""

    def __init__(self, shape, dtype, P, seed):
        from nsol_amd.device import to_device
        rng = np.random.default_rng(seed)
        self.shape, self.P = shape, P
        self.n, self.dim = int(np.prod(shape)), len(shape)
        n, dim = self.n, self.dim
        dev = lambda a: to_device(np.ascontiguousarray(a), dtype)
        self.x = dev(rng.standard_normal(P * n))
        self.xbar = dev(rng.standard_normal(P * n))
        self.p = dev(rng.uniform(-1, 1, P * dim * n))
        self.bt = dev(rng.standard_normal(P * n))
        wt = rng.uniform(0, 3, P * n)
        wt[rng.random(P * n) < 0.3] = 0.0
        self.wt = dev(wt)
        self.lmbda = 20.0 / (1.0 + np.arange(P))
        self.sig = SIGMA * (1.0 + 0.1 * np.arange(P))
        self.tau = TAU * (1.0 - 0.05 * np.arange(P))
        self.theta = THETA - 0.02 * np.arange(P)

    def table(self, flags, has_p):
        from nsol_amd import ops
        col = lambda v: np.asarray(v).reshape(self.P, 1)
        return ops.pd_weighted_table(self.x, self.P, self.lmbda, col(self.sig),
                                     col(self.tau), col(self.theta), not has_p, GAMMA,
                                     flags)

    def member(self, t, m, comps=1):
        k = self.n * comps
        return t[m * k:(m + 1) * k]

    def single(self, m, flags, has_p, bt, wt):
        """Member m alone through the single-run kernels: (xbar_out, x, p_out)."""
        import torch
        from nsol_amd import ops
        x = self.member(self.x, m).clone()
        xb, pin = self.member(self.xbar, m), self.member(self.p, m, self.dim)
        xbo, po = torch.empty_like(x), torch.empty_like(pin)
        b1 = bt if bt.numel() == self.n else self.member(bt, m)
        huber = bool(flags & ops.PD_REG_HUBER)
        if wt is None:
            ops.pd_fused_iter(xb, xbo, x, b1, pin if has_p else None, po, self.shape, W,
                              self.sig[m], 1. + self.sig[m] * GAMMA if huber else 1.,
                              self.tau[m], self.tau[m] * self.lmbda[m], self.theta[m],
                              flags)
        else:
            w1 = wt if wt.numel() == self.n else self.member(wt, m)
            tab = ops.pd_weighted_table(x, 1, [self.lmbda[m]], [self.sig[m]],
                                        [self.tau[m]], [self.theta[m]], not has_p,
                                        GAMMA, flags)
            assert ops.pd_weighted_iter(xb, xbo, x, b1, w1, pin, po, 1, self.shape, W,
                                        tab, 0, flags)
        return xbo, x, po


def _imap(members):
    import torch
    return torch.tensor(list(members), dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_identity_map_writes_the_bits_of_the_stacked_kernels(nsol, shape, dtype):
    """{p zero, not} x {TV, Huber} x {l2, l1} x {anisotropic, isotropic} x
    {unweighted, weighted} x member strides {n, 0} of bt and wt: xbar_out, x and p_out
    of pd_stack_iter with the identity map are nsol_pd_batch_iter's /
    nsol_pd_weighted_iter's bit for bit, with rows and without."""
    import torch
    from nsol_amd import _lib, ops
    lib = _lib.load()
    P = 3
    st = _State(shape, dtype, P, sum(shape) + 3)
    n, dim = st.n, st.dim
    ndim, nz, ny, nx = ops.dims3(shape)
    batch_iter = getattr(lib, "nsol_pd_batch_iter_" +
                         ("f32" if dtype == np.float32 else "f64"))
    ws = ops.pd_stack_workspace(st.x, shape, P)
    ident = _imap(range(P))
    tabs = {}
    for has_p, huber, l1, iso, wgt, shared_bt, shared_wt in itertools.product(
            (False, True), repeat=7):
        if shared_wt and not wgt:
            continue
        flags = _flags(huber, l1, iso, wgt)
        label = (has_p, huber, l1, iso, wgt, shared_bt, shared_wt)
        if (flags, has_p) not in tabs:
            tabs[flags, has_p] = st.table(flags, has_p)
        tab = tabs[flags, has_p]
        bt = st.bt[:n] if shared_bt else st.bt
        wt = None if not wgt else st.wt[n:2 * n] if shared_wt else st.wt
        xr, xbr, pr = st.x.clone(), torch.empty_like(st.x), torch.empty_like(st.p)
        if wgt:
            assert ops.pd_weighted_iter(st.xbar, xbr, xr, bt, wt, st.p, pr, P, shape, W,
                                        tab, 0, flags)
        else:
            bt_all = bt.repeat(P) if shared_bt else bt      # k_pd_batch: own data only
            assert batch_iter(st.xbar.data_ptr(), xbr.data_ptr(), xr.data_ptr(),
                              bt_all.data_ptr(), st.p.data_ptr(), pr.data_ptr(), P, ndim,
                              nz, ny, nx, *W, tab.data_ptr(), 0, flags, None) == 0
        for with_rows in (False, True):
            xc, xbc, pc = st.x.clone(), torch.empty_like(st.x), torch.empty_like(st.p)
            rows = torch.zeros(4 * P, dtype=torch.float64, device="cuda")
            assert ops.pd_stack_iter(st.xbar, xbc, xc, bt, wt, st.p, pc, P, ident, P,
                                     shape, W, tab, 0, flags,
                                     ws=ws if with_rows else None,
                                     rows=rows if with_rows else None)
            for got, want in ((xc, xr), (xbc, xbr), (pc, pr)):
                assert torch.equal(got, want), (label, with_rows)
            if with_rows:
                assert bool((rows.view(P, 4)[:, 1] > 0).all()), label


SENTINEL = -777.25


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_subset_map_touches_its_members_only(nsol, shape, dtype):
    """Members {1, 2, 5} of 6: theirs are the single-run kernels' bits; every byte of
    the others' x, xbar, p and board rows is as it was."""
    import torch
    from nsol_amd import ops
    P, mapped = 6, [1, 2, 5]
    st = _State(shape, dtype, P, sum(shape) + 5)
    ws = ops.pd_stack_workspace(st.x, shape, P)
    dmap = _imap(mapped)
    for has_p, iso, wgt, with_rows in itertools.product((False, True), repeat=4):
        flags = _flags(True, False, iso, wgt)
        label = (has_p, iso, wgt, with_rows)
        tab = st.table(flags, has_p)
        wt = st.wt if wgt else None
        xc = st.x.clone()
        xbc = torch.full_like(st.x, SENTINEL)
        pc = torch.full_like(st.p, SENTINEL)
        rows = torch.full((P, 4), SENTINEL, dtype=torch.float64, device="cuda")
        assert ops.pd_stack_iter(st.xbar, xbc, xc, st.bt, wt, st.p, pc, P, dmap,
                                 len(mapped), shape, W, tab, 0, flags,
                                 ws=ws if with_rows else None,
                                 rows=rows.view(-1) if with_rows else None)
        for m in range(P):
            gx, gxb = st.member(xc, m), st.member(xbc, m)
            gp = st.member(pc, m, st.dim)
            if m in mapped:
                xbo, x1, po = st.single(m, flags, has_p, st.bt, wt)
                assert torch.equal(gx, x1) and torch.equal(gxb, xbo), (label, m)
                assert torch.equal(gp, po), (label, m)
                assert with_rows == bool((rows[m] != SENTINEL).all()), (label, m)
            else:
                assert torch.equal(gx, st.member(st.x, m)), (label, m)
                assert bool((gxb == SENTINEL).all()), (label, m)
                assert bool((gp == SENTINEL).all()), (label, m)
                assert bool((rows[m] == SENTINEL).all()), (label, m)


def _np_sums(x_old, x_new, p_old, p_new):
    f = lambda a: a.cpu().numpy().astype(np.float64)
    xo, xn, pn = f(x_old), f(x_new), f(p_new)
    po = np.zeros_like(pn) if p_old is None else f(p_old)
    return np.array([np.sum((xn - xo) ** 2), np.sum(xn ** 2),
                     np.sum((pn - po) ** 2), np.sum(pn ** 2)])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_every_member_gets_its_own_sums(nsol, shape, dtype):
    """The board row of every mapped member against nsol_pd_change_* on that member's
    arrays before and after, and against NumPy in float64, to 1e-12; two launches
    give the same bits.  The identity map and a map with a gap."""
    import torch
    from nsol_amd import ops
    P = 4
    st = _State(shape, dtype, P, sum(shape) + 9)
    n, dim = st.n, st.dim
    ws = ops.pd_stack_workspace(st.x, shape, P)
    ws1 = ops.pd_check_workspace(st.x, shape)
    worst = 0.0
    for mapped in (list(range(P)), [0, 2, 3]):
        dmap = _imap(mapped)
        for has_p, huber, iso, wgt in itertools.product((False, True), repeat=4):
            flags = _flags(huber, False, iso, wgt)
            label = (mapped, has_p, huber, iso, wgt)
            tab = st.table(flags, has_p)
            wt = st.wt if wgt else None
            out = []
            for _ in range(2):
                xc, xbc, pc = st.x.clone(), torch.empty_like(st.x), torch.empty_like(st.p)
                rows = torch.zeros((P, 4), dtype=torch.float64, device="cuda")
                assert ops.pd_stack_iter(st.xbar, xbc, xc, st.bt, wt, st.p, pc, P, dmap,
                                         len(mapped), shape, W, tab, 0, flags, ws=ws,
                                         rows=rows.view(-1))
                out.append((xc, pc, rows))
            assert torch.equal(out[0][2], out[1][2]), label      # the same bits twice
            xc, pc, rows = out[0]
            got = rows.cpu().numpy()
            second = torch.zeros(4, dtype=torch.float64, device="cuda")
            for m in mapped:
                x_old, x_new = st.member(st.x, m), st.member(xc, m)
                p_old = st.member(st.p, m, dim) if has_p else None
                p_new = st.member(pc, m, dim)
                ops.pd_change(x_old, x_new, p_old, p_new, ws1, second)
                change = second.cpu().numpy()
                want = _np_sums(x_old, x_new, p_old, p_new)
                assert np.all(np.isfinite(got[m])) and np.all(want > 0), (label, m)
                err = max(np.max(np.abs(got[m] - want) / want),
                          np.max(np.abs(got[m] - change) / want))
                worst = max(worst, err)
                assert err <= SUM_TOL, (label, m, err, got[m], want, change)
    print(shape, np.dtype(dtype).name, "worst relative error of a sum %.3g" % worst)


def test_entry_declines_and_refuses(nsol):
    """-2 for what nsol_pd_batch_iter declines, NSOL_EINVAL for what cannot be
    indexed, 0 and no launch for an empty map."""
    import torch
    from nsol_amd import _lib, ops
    lib = _lib.load()
    t, xx, tab0 = (torch.zeros(64, dtype=torch.float32, device="cuda") for _ in range(3))
    d, d2 = (torch.zeros(64, dtype=torch.float64, device="cuda") for _ in range(2))
    imap = _imap([0, 1])
    before = ops.pd_stack_launches()

    def call(members=2, nx=16, active=2, xo=None, bts=16, wt=None, wts=0, flags=0,
             dmap=imap, ws=None, wsd=0, rows=None, ny=1, ndim=1):
        u = torch.zeros(64, dtype=torch.float32, device="cuda")
        v = torch.zeros(64, dtype=torch.float32, device="cuda")
        return lib.nsol_pd_stack_iter_f32(
            t.data_ptr(), (u if xo is None else xo).data_ptr(), xx.data_ptr(),
            t.data_ptr(), bts, None if wt is None else wt.data_ptr(), wts,
            t.data_ptr(), v.data_ptr(), members, None if dmap is None else
            dmap.data_ptr(), active, ndim, 1, ny, nx, 1.0, 1.0, 1.0, tab0.data_ptr(), 0,
            flags, None if ws is None else ws.data_ptr(), wsd,
            None if rows is None else rows.data_ptr(), None)
    for members, nx in ((0, 16), (3, 1 << 30), (65536, 16)):
        assert call(members=members, nx=nx, active=0) == -2
    assert call(ny=2) == -2                                  # 1-D with two rows
    assert call(active=3) == -1                              # more than the members
    assert call(active=-1) == -1
    assert call(xo=t) == -1                                  # xbar_out is xbar_in
    assert call(bts=8) == -1                                 # neither 0 nor n
    assert call(dmap=None) == -1
    assert call(wt=t) == -1                                  # weights without the flag
    assert call(flags=ops.PD_DATA_WEIGHTED) == -1            # the flag without them
    assert call(flags=ops.PD_DATA_WEIGHTED, wt=t, wts=8) == -1
    assert call(rows=d2) == -1                               # rows without a workspace
    assert call(rows=d2, ws=d, wsd=7) == -1                  # 4 * active * 1 workgroup
    assert call(active=0) == 0 and call(active=0, dmap=None) == 0
    assert ops.pd_stack_launches() == before
    assert call(rows=d2, ws=d, wsd=8) == 0
    assert call() == 0
    assert ops.pd_stack_launches() == before + 2
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.pd_stack_workspace(t, (5, 6, 7, 8), 2)
    x = torch.zeros(60, dtype=torch.float64, device="cuda")
    p = torch.zeros(120, dtype=torch.float64, device="cuda")
    tab = ops.pd_weighted_table(x, 2, [1., 1.], [[.3], [.3]], [[.3], [.3]], [[1.], [1.]],
                                True, 0.05, 0)
    args = lambda **kw: dict(dict(xbar_in=x.clone(), xbar_out=x.clone(), x=x.clone(),
                                  bt=x, wt=None, p_in=p, p_out=p.clone(), members=2,
                                  map=imap, active=2, shape=(5, 6), w=W, tab=tab,
                                  iteration=0, flags=0), **kw)
    assert ops.pd_stack_iter(**args())
    for bad in (dict(map=imap.long()), dict(active=3), dict(map=imap[:1]),
                dict(p_out=p[:119]), dict(wt=x), dict(flags=ops.PD_DATA_WEIGHTED),
                dict(iteration=1), dict(bt=x[:31]), dict(rows=d[:8]),
                dict(rows=d[:7], ws=d), dict(shape=(5, 7))):
        with pytest.raises(ValueError):
            ops.pd_stack_iter(**args(**bad))


# -------------------------------------------------------------- the public runs
def _member_obs(shape, m):
    rng = np.random.default_rng(100 + m)
    return (50.0 + 30.0 * rng.standard_normal(shape)) * (1.0 + 0.25 * m)


def _member_weights(shape, m):
    return mixed_weights(shape, 7 + m)


def _solver(obs, reg, data, alg, alpha, L2, iso, weights, dtype, tolerance,
            iters=ITERS, check_every=K):
    """test_pd_stop_gpu's wiring on an observation and weights of the member's own:
    b = x0 = obs, x_scale = max(obs), as the restatement has them."""
    import nsol_amd.linear_operators as LO
    import nsol_amd.primal_dual_solver as pd
    from nsol_amd.proximal_operators import ProximalOperators as prox
    shape = obs.shape
    b = obs.flatten()
    xs = float(np.max(b))
    dim = len(shape)
    lo = {1: LO.LinearOperators1D, 2: LO.LinearOperators2D,
          3: LO.LinearOperators3D}[dim]()
    grad, grad_adj = lo.get_gradient_operators()
    Z = grad(b.reshape(shape)).shape
    D = lambda x: grad(x.reshape(*shape)).flatten()
    Da = lambda x: grad_adj(x.reshape(*Z)).flatten()
    if weights is None:
        f = prox.prox_ell1_denoising if data == "L1" else prox.prox_ell2_denoising
        pf = lambda x, tau: f(x, tau, x0=b, x_scale=xs)
    else:
        w = weights.flatten()
        f = prox.prox_ell1_denoising_weighted if data == "L1" else \
            prox.prox_ell2_denoising_weighted
        pf = lambda x, tau: f(x, tau, x0=b, weights=w, x_scale=xs)
    if not iso:
        pg = prox.prox_huber_conj if reg == "Huber" else prox.prox_tv_conj
    elif reg == "Huber":
        pg = lambda x, s: prox.prox_huber_conj_isotropic(x, s, dim)
    else:
        pg = lambda x, s: prox.prox_tv_conj_isotropic(x, s, dim)
    return pd.PrimalDualSolver(prox_f=pf, prox_g_conj=pg, B=D, B_conj=Da, L2=L2, x0=b,
                               alpha=alpha, iterations=iters, x_scale=xs, alg_type=alg,
                               dtype=dtype, tolerance=tolerance, check_every=check_every)


# Stacks: (shape, reg, data, iso, weighted, L2, members per group,
#          [(alpha, alg_type, tolerance, stops at)]), member m on _member_obs(shape, m).
# Chosen on the CPU from the restatement's max(r_x, r_p) at the checks 5, 10, ... 60,
# so that it keeps its 3 % margin at every check; "stops at" is the restatement's.
# In every stack one member retires at the first check, one never does (1e-300), the
# others at three or more other checks, and member 0 is not the last.
STACKS = {
    "2d-tv-l2-two-groups": (
        (24, 40), "TV", "L2", False, False, 8, 4,
        [(0.05, "ALG2", 1e-2, 20), (0.3, "ALG2", 1e-300, 60), (0.02, "ALG3", 0.1, 5),
         (0.1, "ALG2", 1e-2, 30), (0.6, "ALG3", 2e-2, 35),
         (0.05, "ALG2_AHMOD", 5e-2, 45), (0.15, "ALG2", 2e-2, 25)]),
    "2d-huber-l2-weighted": (
        (24, 40), "Huber", "L2", False, True, 8, 6,
        [(0.05, "ALG2", 1e-2, 15), (0.3, "ALG2", 1e-300, 60), (0.02, "ALG3", 0.2, 5),
         (0.1, "ALG2", 1e-3, 30), (0.6, "ALG3", 1e-2, 30), (0.15, "ALG2", 5e-3, 25)]),
    "3d-tv-l2-isotropic": (
        (9, 12, 21), "TV", "L2", True, False, 16, 6,
        [(0.05, "ALG2", 1e-2, 15), (0.3, "ALG2", 1e-300, 60), (0.02, "ALG3", 0.05, 5),
         (0.1, "ALG2", 1e-2, 30), (0.6, "ALG3", 2e-2, 35), (0.15, "ALG2", 1.5e-2, 35)]),
}
# Sweeps over alpha with one tolerance: (shape, reg, data, iso, weighted, L2,
#                                        tolerance, [(alpha, stops at)])
SWEEPS = {
    "2d-tv-l2": ((24, 40), "TV", "L2", False, False, 8, 2.5e-2,
                 [(0.02, 10), (0.05, 15), (0.1, 20), (0.2, 25), (0.4, 30)]),
    "3d-huber-l1-isotropic-weighted": (
        (9, 12, 21), "Huber", "L1", True, True, 16, 1e-2,
        [(0.2, 25), (0.4, 30), (0.6, 35), (0.9, 40)]),
}

_cache = {}


def _restated(shape, m, reg, data, alg, alpha, L2, iso, weighted, tolerance):
    """The float64 restatement for member m (computed once per session; it asserts its
    own 3 % margin at every check)."""
    key = (shape, m, reg, data, alg, alpha, L2, iso, weighted, tolerance)
    if key not in _cache:
        _cache[key] = pd_stop_denoise(
            _member_obs(shape, m), shape, reg, data, alg, alpha, L2, ITERS, tolerance,
            iso=iso, weights=_member_weights(shape, m) if weighted else None)
    return _cache[key]


def _make_stack(name, dtype, **kw):
    shape, reg, data, iso, weighted, L2, _, members = STACKS[name]
    return [_solver(_member_obs(shape, m), reg, data, alg, alpha, L2, iso,
                    _member_weights(shape, m) if weighted else None, dtype, tol, **kw)
            for m, (alpha, alg, tol, _) in enumerate(members)]


def _assert_as_its_own_run(got, one, ref, label):
    """A member of a stacked run against the restatement and its own run()."""
    one.run()
    print(label, "done", got.get_iterations_done(), got.get_stop_reason(),
          "restated", ref["done"], ref["reason"], "alone", one.get_iterations_done())
    assert got.get_iterations_done() == ref["done"] == one.get_iterations_done(), label
    assert got.get_stop_reason() == ref["reason"] == one.get_stop_reason(), label
    assert got.get_execution() == "fused" and one.get_execution() == "fused"
    assert np.array_equal(got.get_x(), one.get_x()), label
    a, b = got.get_changes(), one.get_changes()
    assert a.shape == b.shape == ref["changes"].shape, label
    assert np.array_equal(a[:, 0], b[:, 0]), label
    assert np.allclose(a[:, 1:], b[:, 1:], rtol=1e-12, atol=0), (label, a, b)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(STACKS))
def test_stack_members_stop_where_their_own_runs_stop(nsol, name, dtype, monkeypatch):
    from nsol_amd import PrimalDualBatch, ops
    shape, reg, data, iso, weighted, L2, group, members = STACKS[name]
    refs = [_restated(shape, m, reg, data, alg, alpha, L2, iso, weighted, tol)
            for m, (alpha, alg, tol, _) in enumerate(members)]
    # the cases are what the table says: the restatement alone, on the CPU
    assert [r["done"] for r in refs] == [c[3] for c in members]
    assert len(set(c[3] for c in members)) >= 5 and members[0][3] < ITERS
    assert 5 in [c[3] for c in members] and refs[1]["reason"] == "iterations"
    n, dim = int(np.prod(shape)), len(shape)
    # the byte budget of `group` members' state: x, two xbar, bt (and wt), two p
    monkeypatch.setattr(ops, "PD_BATCH_GROUP_BYTES", group * (
        (5 if weighted else 4) + 2 * dim) * n * np.dtype(dtype).itemsize)
    solvers = _make_stack(name, dtype)
    before = ops.pd_stack_launches(), ops.pd_batch_launches(), ops.pd_check_launches()
    batch = PrimalDualBatch(solvers, stacked_stopping=True)
    batch.run()
    assert batch.get_execution() == ["stacked"] * len(members)
    assert batch.get_group_size() == group
    # one launch per iteration and group, until the group's last member has stopped
    done = [r["done"] for r in refs]
    assert ops.pd_stack_launches() - before[0] == sum(
        max(done[a:a + group]) for a in range(0, len(done), group))
    assert (ops.pd_batch_launches(), ops.pd_check_launches()) == before[1:]
    for m, (got, one) in enumerate(zip(solvers, _make_stack(name, dtype))):
        _assert_as_its_own_run(got, one, refs[m], (name, m))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_sweep_members_stop_where_the_sequential_sweep_stops(nsol, name, dtype):
    from nsol_amd import ops
    from nsol_amd.parameter_sweep import PrimalDualSweep
    shape, reg, data, iso, weighted, L2, tol, members = SWEEPS[name]
    alphas = [a for a, _ in members]
    refs = [_restated(shape, 0, reg, data, "ALG2", a, L2, iso, weighted, tol)
            for a in alphas]
    assert [r["done"] for r in refs] == [k for _, k in members]
    obs = _member_obs(shape, 0)
    t = _solver(obs, reg, data, "ALG2", alphas[0], L2, iso,
                _member_weights(shape, 0) if weighted else None, dtype, tol)
    from nsol_amd.similarity_measures import SimilarityMeasures as SM
    truth = obs.flatten() * 0.9

    def sweep(stacked_stopping):
        s = PrimalDualSweep(t._prox_f, t._prox_g_conj, t._B, t._B_conj, L2, obs.flatten(),
                            {"alpha": alphas}, iterations=ITERS, x_scale=t.get_x_scale(),
                            dtype=dtype, tolerance=tol, check_every=K,
                            stacked_stopping=stacked_stopping)
        s.set_measures({"RMSE": lambda x: SM.similarity_measures["RMSE"](x, truth)},
                       every=4)
        s.run()
        return s
    before = ops.pd_stack_launches()
    got = sweep(True)
    assert ops.pd_stack_launches() - before == max(k for _, k in members)
    want = sweep(False)
    assert ops.pd_stack_launches() - before == max(k for _, k in members)
    assert got.get_execution() == "stacked" and want.get_execution() == "sequential"
    assert got.get_group_size() == len(members)
    assert got.get_iterations_done() == want.get_iterations_done() == \
        [r["done"] for r in refs]
    for m in range(len(members)):
        assert np.array_equal(got.get_x(m), want.get_x(m)), m
    assert bool((got.get_x_all_device() == want.get_x_all_device()).all())
    # the measures up to every member's stop, NaN behind it, as in the single runs
    a, b = got.get_measures()["RMSE"], want.get_measures()["RMSE"]
    assert got.get_observed_iterations() == want.get_observed_iterations()
    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
    assert np.isnan(a[0, -1]) and not np.isnan(a[0, 1])


def test_device_observers_of_stack_members_stop_with_them(nsol):
    from nsol_amd import PrimalDualBatch
    from nsol_amd.observer import Observer
    from nsol_amd.similarity_measures import SimilarityMeasures as SM
    name = "2d-tv-l2-two-groups"
    shape = STACKS[name][0]

    def make():
        out = _make_stack(name, np.float64)
        for m, s in enumerate(out):
            ref = _member_obs(shape, m).flatten()
            o = Observer(keep_iterates=False, every=4)
            o.set_measures({"RMSE": lambda x, r=ref: SM.similarity_measures["RMSE"](x, r)})
            s.set_observer(o)
        return out
    solvers = make()
    batch = PrimalDualBatch(solvers, stacked_stopping=True)
    batch.run()
    assert batch.get_execution() == ["stacked"] * len(solvers)
    for m, (got, one) in enumerate(zip(solvers, make())):
        one.run()
        assert got.get_iterations_done() == one.get_iterations_done() == \
            STACKS[name][7][m][3]
        assert np.array_equal(got.get_x(), one.get_x()), m
        og, oo = got.get_observer(), one.get_observer()
        og.compute_measures()
        oo.compute_measures()
        assert og.get_observed_iterations() == oo.get_observed_iterations()
        a, b = og.get_measures()["RMSE"], oo.get_measures()["RMSE"]
        assert np.array_equal(a, b, equal_nan=True), (m, a, b)
        assert np.isnan(a[-1]) == (got.get_iterations_done() < ITERS)


def test_launch_counters(nsol):
    from nsol_amd import PrimalDualBatch, ops
    name = "2d-huber-l2-weighted"
    members = STACKS[name][7]
    # a stack whose members have all retired launches nothing more
    solvers = [s for s, c in zip(_make_stack(name, np.float64), members) if c[3] < ITERS]
    before = ops.pd_stack_launches()
    batch = PrimalDualBatch(solvers, stacked_stopping=True)
    batch.run()
    assert batch.get_execution() == ["stacked"] * len(solvers)
    last = max(c[3] for c in members if c[3] < ITERS)
    assert ops.pd_stack_launches() - before == last < ITERS
    assert [s.get_iterations_done() for s in solvers] == \
        [c[3] for c in members if c[3] < ITERS]
    # the option off, and runs without a tolerance: not one member-mapped launch
    before = ops.pd_stack_launches()
    off = PrimalDualBatch(_make_stack(name, np.float64, iters=10))
    off.run()
    assert off.get_execution() == ["sequential"] * len(members)
    for flag in (False, True):
        plain = _make_stack(name, np.float64, iters=10)
        for s in plain:
            s.set_tolerance(None)
        b = PrimalDualBatch(plain, stacked_stopping=flag)
        b.run()
        assert b.get_execution() == ["stacked"] * len(members)
    assert ops.pd_stack_launches() == before
    # a stack of one stays sequential, and so does a mixed pair
    pair = _make_stack(name, np.float64, iters=10)[:2]
    pair[1].set_tolerance(None)
    b = PrimalDualBatch(pair, stacked_stopping=True)
    b.run()
    assert b.get_execution() == ["sequential"] * 2
    assert ops.pd_stack_launches() == before


def test_a_declined_geometry_falls_back_to_sequential(nsol, monkeypatch):
    from nsol_amd import PrimalDualBatch, ops
    from nsol_amd.parameter_sweep import PrimalDualSweep
    from nsol_amd.stacked_stopping import StackDevice
    name = "2d-tv-l2-two-groups"
    solvers = _make_stack(name, np.float32)[:4]
    seen = []

    def declined(*args, **kw):
        seen.append([s._x for s in solvers])
        return False
    monkeypatch.setattr(StackDevice, "iter", staticmethod(declined))
    before = ops.pd_stack_launches()
    batch = PrimalDualBatch(solvers, stacked_stopping=True)
    batch.run()
    assert len(seen) == 1 and all(x is None for x in seen[0])   # nothing written before
    assert batch.get_execution() == ["sequential"] * 4 and batch.get_group_size() is None
    assert ops.pd_stack_launches() == before
    for m, (got, one) in enumerate(zip(solvers, _make_stack(name, np.float32)[:4])):
        one.run()
        assert got.get_iterations_done() == one.get_iterations_done() == \
            STACKS[name][7][m][3]
        assert np.array_equal(got.get_x(), one.get_x()), m
        assert np.array_equal(got.get_changes(), one.get_changes()), m
    shape, reg, data, iso, weighted, L2, tol, members = SWEEPS["2d-tv-l2"]
    obs = _member_obs(shape, 0)
    t = _solver(obs, reg, data, "ALG2", 0.05, L2, iso, None, np.float32, tol)
    sw = PrimalDualSweep(t._prox_f, t._prox_g_conj, t._B, t._B_conj, L2, obs.flatten(),
                         {"alpha": [a for a, _ in members[:2]]}, iterations=ITERS,
                         x_scale=t.get_x_scale(), dtype=np.float32, tolerance=tol,
                         check_every=K, stacked_stopping=True)
    sw.run()
    assert sw.get_execution() == "sequential"
    assert sw.get_iterations_done() == [k for _, k in members[:2]]
    assert ops.pd_stack_launches() == before


def test_run_denoising_cli_slice_wise_tolerance(nsol, tmp_path, capsys, monkeypatch):
    """--slice-wise --tolerance: the slices stacked, and the file and the printed
    range of stopping iterations those of the stack forced sequential."""
    import re
    from nsol_amd import ops
    from nsol_amd.application import run_denoising
    vol = np.stack([_member_obs((24, 40), m) for m in range(5)])
    vol[3] = 0.0                                    # copied through
    src = str(tmp_path / "vol.npy")
    np.save(src, vol)
    outs = [str(tmp_path / f) for f in ("stacked.npy", "sequential.npy")]
    argv = lambda out: ["--observation", src, "--result", out, "--reconstruction-type",
                        "TVL2", "--iterations", "60", "--alpha", "0.05", "--dtype",
                        "float64", "--slice-wise", "--tolerance", "1e-2",
                        "--check-every", "5"]
    before = ops.pd_stack_launches()
    assert run_denoising.main(argv(outs[0])) == 0
    assert ops.pd_stack_launches() > before
    first = capsys.readouterr().out.splitlines()
    before = ops.pd_stack_launches()
    monkeypatch.setattr(ops, "PD_BATCH_MAX_VOXELS", 0)      # no solver has a key
    assert run_denoising.main(argv(outs[1])) == 0
    assert ops.pd_stack_launches() == before
    second = capsys.readouterr().out.splitlines()
    assert re.search(r"\(4 slices stacked, 1 copied through, 0 sequential\)$", first[0])
    assert re.search(r"\(0 slices stacked, 1 copied through, 4 sequential\)$", second[0])
    m = re.match(r"^  stopped after (\d+) to (\d+) of 60 iterations$", first[1])
    assert m and int(m.group(1)) <= int(m.group(2)) < 60, first[1]
    assert first[1] == second[1]
    assert open(outs[0], "rb").read() == open(outs[1], "rb").read()


def test_run_denoising_cli_alpha_sweep_tolerance(nsol, tmp_path, capsys):
    import re
    from nsol_amd.application import run_denoising
    shape, _, _, _, _, L2, tol, members = SWEEPS["2d-tv-l2"]
    src, out = str(tmp_path / "img.npy"), str(tmp_path / "out.npy")
    np.save(src, _member_obs(shape, 0))
    argv = ["--observation", src, "--result", out, "--reconstruction-type", "TVL2",
            "--iterations", str(ITERS), "--L2", str(L2), "--dtype", "float64",
            "--tolerance", str(tol), "--check-every", str(K), "--alpha"] + \
        [str(a) for a, _ in members]
    assert run_denoising.main(argv) == 0
    text = capsys.readouterr().out
    assert len(re.findall(r"\(stacked\)", text)) == len(members)
    assert [int(k) for k in re.findall(r"stopped after (\d+) of 60 iterations", text)] \
        == [k for _, k in members]
