"""The generalized Cauchy point of L-BFGS-B (nsol_amd/lbfgsb.py `_cauchy`) against
a plain float64 reference of Byrd, Lu, Nocedal & Zhu's algorithm CP: one loop
over all breakpoints sorted by (t, index), no windows, no prefix sums.

On the CPU the NumPy backend (tests/lbfgsb_numpy_backend.py) is held to the
reference; on the GPU every stage of the device search (nsol_lbfgsb.hip,
nsol_sort.hip) is held to the NumPy rule it implements, the whole device search
to the reference, and the other length-n primitives of DeviceBackend to the
NumPy backend.  The case catalogue reaches ties, clustered breakpoints that
overflow the device's breakpoint windows, the clamp of f'', searches that fix
every variable and searches without breakpoints."""
import numpy as np
import pytest

from conftest import rel_l2
from lbfgsb_numpy_backend import NumpyBackend

EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def setup_rule(x, g, lo, hi, iwhere, dtype):
    """Classification, d = -g on the moving variables and the breakpoints, all in
    the kernel's dtype (k_cauchy_setup); the sums in float64."""
    T = np.dtype(dtype).type
    x, g = np.asarray(x, T), np.asarray(g, T)
    has_lo, has_hi = bool(np.isfinite(lo)), bool(np.isfinite(hi))
    neg = -g
    inf = T(np.inf)
    tl = x - T(lo) if has_lo else np.full(x.size, inf)
    tu = T(hi) - x if has_hi else np.full(x.size, inf)
    iw = np.array(iwhere, np.int8)
    act = (iw != 3) & (iw != -1)
    xlower = has_lo & (tl <= 0)
    xupper = has_hi & (tu <= 0)
    new = np.zeros(x.size, np.int8)
    new[xlower & (neg <= 0)] = 1
    new[~xlower & xupper & (neg >= 0)] = 2
    new[~xlower & ~xupper & (np.abs(neg) <= 0)] = -3
    iw[act] = new[act]
    moving = (iw == 0) | (iw == -1)
    d = np.where(moving, neg, T(0)).astype(T)
    tbk = np.full(x.size, inf, T)
    bl = moving & has_lo & (neg < 0)
    bu = moving & ~bl & has_hi & (neg > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        tbk[bl] = tl[bl] / (-neg[bl])
        tbk[bu] = tu[bu] / neg[bu]
    unb = moving & ~bl & ~bu & (np.abs(neg) > 0)
    d64 = d.astype(np.float64)
    st = {"f1": -float(np.dot(d64, d64)),
          "nbreak": int(np.count_nonzero(bl | bu)),
          "bnded": not bool(np.any(unb)), "any_move": bool(np.any(moving))}
    return d, tbk, iw, st


def middle(cm):
    """M = [[-D, L'], [L, theta S'S]]^-1 from its definition (BLNZ 1995, (3.4))."""
    c = cm.col
    sy = cm.sy[:c, :c]
    ss = np.triu(cm.ss[:c, :c]) + np.triu(cm.ss[:c, :c], 1).T
    L = np.tril(sy, -1)
    K = np.block([[-np.diag(np.diag(sy)), L.T], [L, cm.theta * ss]])
    return np.linalg.inv(K)


def reference_cauchy(x, g, lo, hi, iwhere, ws, wy, cm, dtype):
    """Algorithm CP of L-BFGS-B (scipy's `cauchy`: the same recurrences, the same
    clamp of f'' and the same rule for the last breakpoint), ties taken in index
    order.  Inputs are rounded to `dtype` first; the walk is float64.  Returns
    (xcp, c, iwhere, info)."""
    T = np.dtype(dtype).type
    d, tbk, iw, st = setup_rule(x, g, lo, hi, iwhere, dtype)
    xT = np.asarray(x, T).astype(np.float64)
    d64 = d.astype(np.float64)
    n, col, theta = xT.size, cm.col, cm.theta
    Y = np.array([np.asarray(w, T) for w in wy], np.float64).reshape(col, n)
    S = np.array([np.asarray(w, T) for w in ws], np.float64).reshape(col, n)
    info = {"crossed": 0, "all_fixed": False, "clamped": 0, "gap": np.inf,
            "tsum": 0.0}
    if not st["any_move"]:
        return xT.copy(), np.zeros(2 * col), iw, info
    M = middle(cm) if col else np.zeros((0, 0))
    p = np.concatenate((Y.dot(d64), theta * S.dot(d64)))
    c = np.zeros(2 * col)
    f1 = st["f1"]
    f2 = -theta * f1
    f2_org = f2
    if col:
        f2 -= float(p.dot(M.dot(p)))
    dtm = -f1 / f2
    tsum = tj = 0.0
    nbreak, bnded = st["nbreak"], st["bnded"]
    nleft = nbreak
    fin = np.isfinite(tbk)
    order = np.lexsort((np.arange(n), tbk))[:nbreak]
    assert fin[order].all() and not fin[np.argsort(tbk)[nbreak:]].any()
    xcp = xT.copy()
    tb = tbk.astype(np.float64)
    all_fixed = False
    lo64, hi64 = float(T(lo)), float(T(hi))
    for ibp in order.tolist():
        tnew = float(tb[ibp])
        dt = tnew - tj
        info["gap"] = min(info["gap"], abs(dtm - dt) / max(abs(dtm), abs(dt), 1e-300))
        if dtm < dt:
            break
        tj = tnew
        tsum += dt
        nleft -= 1
        info["crossed"] += 1
        dibp = float(d64[ibp])
        if dibp > 0:
            zibp = hi64 - xT[ibp]
            xcp[ibp], iw[ibp] = hi64, 2
        else:
            zibp = lo64 - xT[ibp]
            xcp[ibp], iw[ibp] = lo64, 1
        if nleft == 0 and nbreak == n:
            dtm = dt
            all_fixed = True
            break
        dibp2 = dibp * dibp
        f1 = f1 + dt * f2 + dibp2 - theta * dibp * zibp
        f2 = f2 - theta * dibp2
        if col:
            c = c + dt * p
            wbp = np.concatenate((Y[:, ibp], theta * S[:, ibp]))
            v = M.dot(wbp)
            wmc, wmp, wmw = float(c.dot(v)), float(p.dot(v)), float(wbp.dot(v))
            p = p - dibp * wbp
            f1 += dibp * wmc
            f2 += 2.0 * dibp * wmp - dibp2 * wmw
        if f2 < EPS * f2_org:
            info["clamped"] += 1
        f2 = max(EPS * f2_org, f2)
        if nleft > 0:
            dtm = -f1 / f2
        elif bnded:
            f1 = f2 = dtm = 0.0
        else:
            dtm = -f1 / f2
    info["all_fixed"] = all_fixed
    if not all_fixed:
        if dtm <= 0.0:
            dtm = 0.0
        tsum += dtm
        moving = ~np.isin(np.arange(n), order[:info["crossed"]])
        xcp[moving] = xT[moving] + tsum * d64[moving]
    if col:
        c = c + dtm * p
    info["tsum"] = tsum
    return xcp, c, iw, info


# ---------------------------------------------------------------------------
# the case catalogue
# ---------------------------------------------------------------------------
def pairs(n, col, m, dtype, seed, hscale=1.0):
    """col stored pairs (s_k, y_k = H s_k), H diagonal and positive definite, in
    `dtype`, and the CompactMatrix built from them."""
    from nsol_amd.lbfgsb import CompactMatrix
    T = np.dtype(dtype).type
    rng = np.random.default_rng(1000 + seed)
    h = hscale * rng.uniform(0.5, 2.0, n)
    S = rng.standard_normal((col, n)).astype(T)
    Y = (S.astype(np.float64) * h).astype(T)
    S64, Y64 = S.astype(np.float64), Y.astype(np.float64)
    cm = CompactMatrix(m)
    cm.col = col
    if col:
        cm.ss[:col, :col] = S64.dot(S64.T)
        cm.sy[:col, :col] = S64.dot(Y64.T)          # sy[i, j] = s_i'y_j
        cm.theta = float(Y64[-1].dot(Y64[-1]) / S64[-1].dot(Y64[-1]))
        assert cm.form_t()
    else:
        cm.theta = hscale
    return list(S), list(Y), cm


def first_dtm(g, ws, wy, cm, dtype):
    """The minimiser along -g before any breakpoint (every variable moving)."""
    T = np.dtype(dtype).type
    d = -np.asarray(g, T).astype(np.float64)
    col, th = cm.col, cm.theta
    f1 = -d.dot(d)
    f2 = -th * f1
    if col:
        Y = np.array(wy, np.float64)
        S = np.array(ws, np.float64)
        p = np.concatenate((Y.dot(d), th * S.dot(d)))
        f2 -= p.dot(middle(cm).dot(p))
    return -f1 / f2


CASES = ("even", "tied", "clustered", "clustered_early", "ties_gt_cap", "clamp",
         "all_crossed", "no_breakpoints", "one_sided")
# the layouts whose breakpoints overflow a device window of OVERFLOW_CAP at
# OVERFLOW_N variables
OVERFLOW_CASES = ("tied", "clustered", "clustered_early", "ties_gt_cap")
OVERFLOW_N, OVERFLOW_CAP = 50000, 4096
# col per case: the clamp of f'' leaves f' at rounding level (dt_min = -f' / f'' is
# then decided by rounding): only its col = 0 form is exact enough to compare
COLS = [(name, col) for name in CASES for col in (0, 1, 10)
        if name != "clamp" or col == 0]


def xcp_tol(info):
    """float64 xcp: the recurrences for f' and f'' take one term per breakpoint
    crossed, which the device sums by prefix sums over windows, the reference one
    after the other.  Observed on an MI355X: at most 8e-14 without overflowing
    windows (up to 843 196 breakpoints crossed), 1.23e-12 for ties_gt_cap at col = 1
    in windows of 4 096 (the largest of all cases)."""
    return 2e-12


def err_xcp(xcp, xr, x, d, tsum, label):
    """|xcp - xr| relative to the size of what x + tsum d is formed from (a point
    near a bound is the difference of two larger numbers)."""
    scale = np.abs(np.asarray(x, np.float64)) + abs(tsum) * np.abs(
        np.asarray(d, np.float64))
    return rel_l2(scale + (np.asarray(xcp, np.float64) - xr), scale, label)




def make_case(name, n, col, dtype, seed=0, m=10):
    """(x, g, lo, hi, iwhere, ws, wy, cm) in `dtype` (x, g, ws, wy)."""
    T = np.dtype(dtype).type
    rng = np.random.default_rng(seed + 7 * n + 13 * col)
    col = min(col, n)
    hscale = {"tied": 1.6, "all_crossed": 0.01}.get(name, 1.0)
    ws, wy, cm = pairs(n, col, m, dtype, seed, hscale)
    lo, hi = 0.0, np.inf
    if name == "even":
        lo, hi = 0.0, 1.0
        x = rng.uniform(0.02, 0.98, n)
        g = 2.0 * rng.standard_normal(n)
    elif name == "tied":
        # t in {0.25, 0.5, 0.75}: thousands of equal breakpoints
        lo, hi = 0.0, 1.0
        x = rng.choice([0.25, 0.5, 0.75], n)
        g = rng.choice([-1.0, 1.0], n)
    elif name in ("clustered", "clustered_early", "ties_gt_cap"):
        g = np.ones(n)
        dtm = first_dtm(g, ws, wy, cm, dtype)
        t = rng.uniform(0.9, 1.0, n) * dtm
        if name == "clustered_early":
            k = max(1, n // 100)
            t[rng.choice(n, k, replace=False)] = rng.uniform(0.01, 0.02, k) * dtm
        elif name == "ties_gt_cap":
            t = rng.uniform(0.1, 1.4, n) * dtm
            t[rng.random(n) < 0.3] = float(T(0.5 * dtm))
        x = lo + t * g
    elif name == "clamp":
        # one variable whose |g| dwarfs the rest is crossed first: f'' drops below
        # eps * f''(0) and is clamped (the device hands it to the scalar rule)
        x = rng.uniform(0.1, 1.0, n)
        g = rng.uniform(0.5, 1.0, n) / 32.0
        j = n // 3
        x[j], g[j] = 0.5, 2.0 ** 30
    elif name == "all_crossed":
        lo, hi = 0.0, 1.0
        x = rng.uniform(0.05, 0.95, n)
        g = rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.0, n)
    elif name == "no_breakpoints":
        lo, hi = -np.inf, np.inf
        x = rng.standard_normal(n)
        g = rng.standard_normal(n)
    elif name == "one_sided":
        # lo = 0, hi = inf: the variables with g < 0 move up without a bound
        x = rng.uniform(0.1, 1.0, n)
        g = rng.standard_normal(n)
    else:
        raise ValueError(name)
    x, g = x.astype(T), g.astype(T)
    iw = NumpyBackend().init_where(x, lo, hi)
    return x, g, lo, hi, iw, ws, wy, cm


# ---------------------------------------------------------------------------
# CPU: the NumPy backend against the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,col", COLS)
def test_numpy_cauchy_matches_reference(name, col):
    from nsol_amd import lbfgsb
    for n in (1, 3, 4097, OVERFLOW_N if name in OVERFLOW_CASES else 20000):
        case = make_case(name, n, col, np.float64)
        x, g, lo, hi, iw0, ws, wy, cm = case
        xr, cr, iwr, info = reference_cauchy(*case, np.float64)
        assert info["gap"] > 1e-8, (name, n, info["gap"])
        xcp, c, iw = lbfgsb._cauchy(NumpyBackend(), x.copy(), g, lo, hi, iw0.copy(),
                                    list(ws), list(wy), cm, 1.0)
        d = setup_rule(x, g, lo, hi, iw0, np.float64)[0]
        assert err_xcp(xcp, xr, x, d, info["tsum"], "xcp n=%d" % n) <= xcp_tol(info)
        if cm.col:
            assert rel_l2(c, cr, "c n=%d" % n) <= 1e-10
        assert np.array_equal(iw, iwr)
        assert np.all(xcp >= lo) and np.all(xcp <= hi)


def test_catalogue_reaches_its_paths():
    """The cases are what their names say (at the sizes the GPU tests use)."""
    n = OVERFLOW_N
    info = {}
    for name in CASES:
        case = make_case(name, n, 0, np.float32)
        info[name] = reference_cauchy(*case, np.float32)
    d, tbk, _, st = setup_rule(*make_case("tied", n, 0, np.float32)[:5], np.float32)
    assert np.unique(tbk[np.isfinite(tbk)]).size == 3
    assert 0 < info["tied"][3]["crossed"] < st["nbreak"]
    for name in ("clustered", "all_crossed"):
        xr, _, iwr, inf_ = info[name]
        assert inf_["all_fixed"] and inf_["crossed"] == n
    # the closed form of the clustered layout at col = 0
    assert np.all(info["clustered"][0] == 0.0) and np.all(info["clustered"][2] == 1)
    assert 0 < info["ties_gt_cap"][3]["crossed"] < n
    _, tbk, _, _ = setup_rule(*make_case("ties_gt_cap", n, 0, np.float32)[:5],
                              np.float32)
    assert np.max(np.unique(tbk, return_counts=True)[1]) > OVERFLOW_CAP
    assert info["clamp"][3]["clamped"] >= 1
    d, tbk, _, st = setup_rule(*make_case("no_breakpoints", n, 0, np.float32)[:5],
                               np.float32)
    assert st["nbreak"] == 0 and not st["bnded"]
    d, tbk, _, st = setup_rule(*make_case("one_sided", n, 0, np.float32)[:5],
                               np.float32)
    assert st["nbreak"] > 0 and not st["bnded"]


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()                      # fails loudly if the .so is missing
    return nsol_amd


def _dev(a, dtype=None, offset=0):
    """Host array -> device tensor; offset > 0: a view that starts `offset`
    elements into its allocation (not 16-byte aligned)."""
    import torch
    a = np.asarray(a if dtype is None else np.asarray(a, dtype))
    t = torch.from_numpy(np.ascontiguousarray(a))
    if offset:
        buf = torch.empty(a.size + offset, dtype=t.dtype, device="cuda")
        v = buf[offset:]
        v.copy_(t)
        return v
    return t.cuda()


def _host(t):
    return t.cpu().numpy()


def _ulp_ok(got, ref, scale, k):
    """|got - ref| <= k ulp (float32) of max(|scale|, |ref|), element by element."""
    s = np.maximum(np.abs(scale), np.abs(ref)).astype(np.float32)
    return np.abs(got.astype(np.float64) - ref) <= k * np.spacing(s).astype(np.float64)


def _device_cauchy(case, dtype, capacity=None, offset=0):
    from nsol_amd import lbfgsb
    from nsol_amd.lbfgsb_device import DeviceBackend
    x, g, lo, hi, iw0, ws, wy, cm = case
    be = DeviceBackend()
    if capacity is not None:
        be.CAPACITY = capacity
    for k in list(lbfgsb.STATS):
        lbfgsb.STATS[k] = 0
    xcp, c, iw = lbfgsb._cauchy(
        be, _dev(x, dtype, offset), _dev(g, dtype, offset), lo, hi,
        _dev(iw0, None, offset), [_dev(w, dtype) for w in ws],
        [_dev(w, dtype) for w in wy], cm, 1.0)
    return _host(xcp), np.asarray(c, np.float64), _host(iw), dict(lbfgsb.STATS)


def _check_against_reference(case, dtype, got, label):
    x, g, lo, hi = case[:4]
    xcp, c, iw, stats = got
    xr, cr, iwr, info = reference_cauchy(*case, dtype)
    assert info["gap"] > 1e-8, (label, info["gap"])    # (the case decides clearly)
    # feasibility first, so that an infeasible Cauchy point names itself
    assert np.all(xcp >= lo), "%s: xcp < lo at %d variables (min %g)" % (
        label, int(np.sum(xcp < lo)), float(np.min(xcp)))
    assert np.all(xcp <= hi), "%s: xcp > hi" % label
    assert np.array_equal(iw, iwr), "%s: iwhere differs at %d variables" % (
        label, int(np.sum(iw != iwr)))
    d = setup_rule(*case[:5], dtype)[0].astype(np.float64)
    e = err_xcp(xcp, xr, np.asarray(x, dtype), d, info["tsum"], label + " xcp")
    if dtype == np.float64:
        assert e <= xcp_tol(info)
        if case[7].col:
            assert rel_l2(c, cr, label + " c") <= 1e-10
    else:
        # x + tsum * d is formed in float32: 4 ulp of the larger operand
        scale = np.maximum(np.abs(x.astype(np.float64)), np.abs(info["tsum"] * d))
        ok = _ulp_ok(xcp, xr, scale, 4)
        assert ok.all(), "%s: xcp off by > 4 ulp at %d variables" % (
            label, int(np.sum(~ok)))
        if case[7].col:
            assert rel_l2(c, cr, label + " c") <= 1e-6
    return info


DTYPES = [np.float32, np.float64]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name,col", COLS)
def test_device_cauchy_matches_reference(nsol, name, col, dtype):
    n = 4097 if name != "even" else 20000
    case = make_case(name, n, col, dtype, seed=1)
    _check_against_reference(case, dtype, _device_cauchy(case, dtype),
                             "%s n=%d col=%d" % (name, n, col))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_device_cauchy_with_twenty_stored_pairs(nsol, dtype):
    case = make_case("even", 20000, 20, dtype, seed=2, m=20)
    _check_against_reference(case, dtype, _device_cauchy(case, dtype), "m=20")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 3, 4097, 3 * 32768 + 5, (1 << 20) + 3])
def test_device_cauchy_sizes(nsol, n, dtype):
    col = {(1 << 20) + 3: 0, 3 * 32768 + 5: 1}.get(n, min(n, 10))
    case = make_case("even", n, col, dtype, seed=3)
    _check_against_reference(case, dtype, _device_cauchy(case, dtype), "n=%d" % n)
    if n == 4097:        # the set-up and finish on a view that is not 16-byte aligned
        _check_against_reference(case, dtype, _device_cauchy(case, dtype, offset=1),
                                 "n=%d unaligned" % n)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("col", [0, 1, 10])
@pytest.mark.parametrize("name", OVERFLOW_CASES)
def test_device_cauchy_overflowing_windows(nsol, name, col, dtype):
    """More breakpoints than a window holds: the window is shrunk, and the search
    must still cross every breakpoint before the minimiser."""
    case = make_case(name, OVERFLOW_N, col, dtype, seed=4)
    got = _device_cauchy(case, dtype, capacity=OVERFLOW_CAP)
    _check_against_reference(case, dtype, got, "%s col=%d" % (name, col))
    assert got[3]["window_shrinks"] > 0


@pytest.mark.gpu
def test_device_cauchy_overflow_at_product_size(nsol):
    """20 M float32 breakpoints in [0.9, 1.0] * dtm with the product's window
    capacity: every variable is fixed at its bound (xcp = lo, iwhere = 1)."""
    import torch
    from nsol_amd import lbfgsb
    from nsol_amd.lbfgsb import CompactMatrix
    from nsol_amd.lbfgsb_device import DeviceBackend
    n = 20000000
    be = DeviceBackend()
    assert n > min(be.CAPACITY, 1 << 24)
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = 0.9 + 0.1 * torch.rand(n, dtype=torch.float32, device="cuda", generator=gen)
    g = torch.ones(n, dtype=torch.float32, device="cuda")
    iw = be.init_where(x, 0.0, np.inf)
    cm = CompactMatrix(10)
    for k in list(lbfgsb.STATS):
        lbfgsb.STATS[k] = 0
    xcp, c, iw = lbfgsb._cauchy(be, x, g, 0.0, np.inf, iw, [], [], cm, 1.0)
    mn = float(xcp.min())
    assert mn >= 0.0, "xcp < lo: min %g" % mn
    assert int(torch.count_nonzero(xcp)) == 0
    assert bool(torch.all(iw == 1))
    assert lbfgsb.STATS["window_shrinks"] > 0
    assert lbfgsb.STATS["crossed"] == n


# ---- stage by stage -----------------------------------------------------------
BOUNDS = [(0.0, 1.0), (0.0, np.inf), (-np.inf, 1.0), (-np.inf, np.inf)]


def _setup_inputs(n, lo, hi, rng):
    """Variables inside, at each bound with g outward and inward, g == 0, and
    preset codes -1 and 3."""
    x = rng.uniform(0.05, 0.95, n)
    g = rng.standard_normal(n)
    k = rng.integers(0, 6, n)
    if np.isfinite(lo):
        x[k == 1] = lo
    if np.isfinite(hi):
        x[k == 2] = hi
    g[k == 3] = 0.0
    g[rng.random(n) < 0.1] = 0.0
    iw = NumpyBackend().init_where(x, lo, hi)
    iw[k == 4] = -1
    iw[k == 5] = 3
    return x, g, iw


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("bounds", BOUNDS, ids=["box", "lower", "upper", "free"])
@pytest.mark.parametrize("n,offset", [(4096, 0), (4099, 0), (4096, 1)])
def test_stage_cauchy_setup(nsol, bounds, n, offset, dtype):
    from nsol_amd.lbfgsb_device import DeviceBackend
    lo, hi = bounds
    x, g, iw0 = _setup_inputs(n, lo, hi, np.random.default_rng(n + offset))
    d, tbk, iw, st = DeviceBackend().cauchy_setup(
        _dev(x, dtype, offset), _dev(g, dtype, offset), lo, hi, _dev(iw0, None, offset))
    dr, tr, iwr, sr = setup_rule(x, g, lo, hi, iw0, dtype)
    assert np.array_equal(_host(iw), iwr)
    assert np.array_equal(_host(d), dr)
    # float32 tbk bit-equal: correctly rounded division under -ffp-contract=off
    # and no fast-math
    assert np.array_equal(_host(tbk), tr)
    assert abs(st["f1"] - sr["f1"]) <= 1e-12 * abs(sr["f1"])
    rel_l2(st["f1"], sr["f1"], "f1")
    assert (st["nbreak"], st["bnded"], st["any_move"]) == \
        (sr["nbreak"], sr["bnded"], sr["any_move"])


def _tie_runs(n, dtype, rng):
    """Breakpoints in long runs of equal values, some infinite."""
    vals = np.array([0.125, 0.25, 0.375, 0.5, 0.625, np.inf])
    t = vals[np.minimum(np.arange(n) * 6 // n + rng.integers(-1, 2, n), 5).clip(0)]
    return t.astype(dtype)


ALL = np.iinfo(np.int64).max


def _window_rule(t, t_done, i_done, t_hi, i_hi=ALL):
    i = np.arange(t.size)
    sel = ((t < t_hi) | ((t == t_hi) & (i <= i_hi))) & \
        ((t > t_done) | ((t == t_done) & (i > i_done)))
    idx = i[sel]
    return idx[np.lexsort((idx, t[idx]))]


def _select(tbk, t_done, i_done, t_hi, cap, extra=0, i_hi=ALL):
    import torch
    from nsol_amd import _lib
    from nsol_amd.device import stream_ptr
    from nsol_amd.lbfgsb_device import _fn
    buf = torch.full((cap + extra,), -7, dtype=torch.int64, device=tbk.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=tbk.device)
    _lib.check(_fn("select", tbk)(tbk.data_ptr(), tbk.numel(), float(t_done),
                                  int(i_done), float(t_hi), int(i_hi),
                                  buf.data_ptr(), cap,
                                  cnt.data_ptr(), stream_ptr()), "select")
    return buf, int(cnt.item())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n,offset", [(4099, 0), (3 * 32768 + 5, 0),
                                      ((1 << 20) + 3, 0), (3 * 32768 + 5, 1)])
def test_stage_select_sort_gather(nsol, n, offset, dtype):
    import torch
    from nsol_amd import _lib
    from nsol_amd.device import stream_ptr
    from nsol_amd.lbfgsb_device import _fn
    lib = _lib.load()
    rng = np.random.default_rng(n + offset)
    t = _tie_runs(n, dtype, rng)
    tbk = _dev(t, None, offset)
    from nsol_amd import ops
    ws, _ = ops._workspace(tbk.device)
    res = torch.empty(8, dtype=torch.float64, device="cuda")
    run = np.flatnonzero(t == dtype(0.25))
    mid = int(run[run.size // 2])
    # (t_done, i_done) inside a tie run; a window that ends inside one (i_hi)
    for t_done, i_done, t_hi, i_hi in (
            (-1.0, -1, 0.5, ALL), (0.25, mid, 0.5, ALL), (0.25, int(run[-1]), 0.625, ALL),
            (0.0, -1, 0.25, ALL), (0.625, n, 1.0, ALL), (0.0, -1, 0.25, mid),
            (0.25, int(run[run.size // 4]), 0.25, mid), (0.25, mid, 0.25, mid),
            (0.125, -1, 0.25, int(run[0]) - 1)):
        want = _window_rule(t, t_done, i_done, t_hi, i_hi)
        buf, count = _select(tbk, t_done, i_done, t_hi, max(want.size, 1), 64, i_hi)
        assert count == want.size
        if i_hi == ALL:
            _lib.check(_fn("count_window", tbk)(
                tbk.data_ptr(), n, float(t_done), i_done, float(t_hi), res.data_ptr(),
                ws.data_ptr(), stream_ptr()), "count_window")
            assert int(res[0].item()) == want.size
        got = _host(buf)
        assert np.all(got[want.size:] == -7)
        if count == 0:
            continue
        tmp = torch.empty(int(lib.nsol_lb_sort_tmp_bytes(count, t.itemsize)),
                          dtype=torch.uint8, device="cuda")
        _lib.check(_fn("sort_candidates", tbk)(tbk.data_ptr(), buf.data_ptr(), count,
                                               tmp.data_ptr(), tmp.numel(),
                                               stream_ptr()), "sort_candidates")
        got = _host(buf)
        assert np.array_equal(got[:count], want)
        assert np.all(got[count:] == -7)
        out = torch.empty(count, dtype=tbk.dtype, device="cuda")
        _lib.check(_fn("gather", tbk)(tbk.data_ptr(), buf.data_ptr(), count,
                                      out.data_ptr(), stream_ptr()), "gather")
        assert np.array_equal(_host(out), t[want])
    # more candidates than the buffer holds: the counter reports them all and
    # nothing is written past the capacity
    want = _window_rule(t, -1.0, -1, 0.5)
    cap = want.size // 3
    buf, count = _select(tbk, -1.0, -1, 0.5, cap, 4096)
    got = _host(buf)
    assert count == want.size
    assert np.all(got[cap:] == -7)
    assert np.unique(got[:cap]).size == cap and np.isin(got[:cap], want).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n,offset", [(4096, 0), (4099, 0), (4096, 1)])
def test_stage_cauchy_finish(nsol, n, offset, dtype):
    from nsol_amd.lbfgsb_device import DeviceBackend
    T = np.dtype(dtype).type
    rng = np.random.default_rng(n + 3 * offset)
    lo, hi = 0.0, 1.0
    x = rng.uniform(0.05, 0.95, n).astype(T)
    d = (rng.standard_normal(n) * (rng.random(n) < 0.9)).astype(T)
    tbk = _tie_runs(n, T, rng)
    iw0 = rng.choice([0, -1, -3], n).astype(np.int8)
    run = np.flatnonzero(tbk == T(0.25))
    t_done, i_done = float(T(0.25)), int(run[run.size // 2])   # inside a tie run
    tsum = 0.3125 + 1e-3 * np.pi
    xcp, iw = DeviceBackend().cauchy_finish(
        _dev(x, None, offset), _dev(d, None, offset), _dev(tbk, None, offset), lo, hi,
        _dev(iw0, None, offset), tsum, t_done, i_done, False)
    i = np.arange(n)
    fixed = np.isfinite(tbk) & ((tbk < T(t_done)) | ((tbk == T(t_done)) & (i <= i_done)))
    want = np.where(fixed, np.where(d > 0, T(hi), T(lo)), x + T(tsum) * d).astype(T)
    iwr = iw0.copy()
    iwr[fixed] = np.where(d[fixed] > 0, 2, 1)
    # float64 exact; float32: x + tsum d in float32, correctly rounded operations
    assert np.array_equal(_host(xcp), want)
    assert np.array_equal(_host(iw), iwr)
    assert 0 < fixed.sum() < n and (tbk[fixed] == T(t_done)).any()


# ---- the prefix-sum walk of a sorted window (nsol_lb_cauchy_walk_*) -----------
def walk_rule(t, dib, z, W, theta, tj, f1, f2, f2_org, dtm, p, c, M):
    """The candidate states of the breakpoints of one sorted window from NumPy
    prefix sums (the formulas of `cumsum_walk` in lbfgsb.py, over all K), and the
    event rule of nsol_lb_cauchy_walk_*: the first k whose minimiser lies before
    breakpoint k (stop) or whose f'' falls below eps f''(0) (clamp)."""
    dt = np.diff(np.concatenate(([tj], t)))
    dib2 = dib * dib
    inc2 = -theta * dib2
    inc1x = dib2 - theta * dib * z
    P_after = p - np.cumsum(dib[:, None] * W, axis=0)
    P_before = np.vstack((p, P_after[:-1]))
    C_after = c + np.cumsum(dt[:, None] * P_before, axis=0)
    if W.shape[1]:
        V = W.dot(M.T)
        inc2 = inc2 + 2.0 * dib * np.sum(P_before * V, axis=1) - \
            dib2 * np.sum(W * V, axis=1)
        inc1x = inc1x + dib * np.sum(C_after * V, axis=1)
    f2_after = f2 + np.cumsum(inc2)
    f2_before = np.concatenate(([f2], f2_after[:-1]))
    f1_after = f1 + np.cumsum(dt * f2_before + inc1x)
    dtm_after = -f1_after / f2_after
    dtm_before = np.concatenate(([dtm], dtm_after[:-1]))
    # what each prefix sum has added up so far, in magnitude: the scale of its
    # rounding whatever the order of the sums (f' at a stop is the small difference
    # of large partial sums)
    s1 = abs(f1) + np.cumsum(np.abs(dt * f2_before) + np.abs(inc1x))
    s2 = abs(f2) + np.cumsum(np.abs(inc2))
    sP = np.abs(p) + np.cumsum(np.abs(dib[:, None] * W), axis=0)
    sC = np.abs(c) + np.cumsum(np.abs(dt[:, None] * P_before), axis=0)
    return dict(s1=s1, s2=s2, sP=sP, sC=sC,
                dt=dt, f1=f1_after, f2=f2_after, f2_before=f2_before,
                dtm=dtm_after, dtm_before=dtm_before, P=P_after, C=C_after,
                stop=dtm_before < dt, clamp=f2_after < EPS * f2_org)


def _first(mask):
    return int(np.argmax(mask)) if mask.any() else mask.size


WALKS = [(1, 0, w) for w in ("stop0", "never")] + \
    [(1, 1, "never"), (7, 10, "middle"), (4097, 20, "stop0"), (4097, 20, "middle"),
     (4097, 20, "never"), (65537, 10, "middle"), (65537, 1, "never")] + \
    [(k, 0, w) for k in (4097, (1 << 20) - 5) for w in ("middle", "never", "clamp")] + \
    [((1 << 20) - 5, 1, w) for w in ("stop0", "middle")]


def walk_case(K, col, where, dtype):
    """Inputs of one sorted window whose walk ends as `where` says, and what
    walk_rule expects of it."""
    from nsol_amd.lbfgsb import middle_matrix
    T = np.dtype(dtype).type
    rng = np.random.default_rng(K + 31 * col)
    lo, hi = 0.0, 1.0
    # breakpoints with runs of equal values, in (t, index) order
    t = (np.round(rng.uniform(0.01, 1.0, K) * 4096) / 4096).astype(T)
    order = np.lexsort((np.arange(K), t))
    x = rng.uniform(0.05, 0.95, K).astype(T)
    d = (rng.choice([-1.0, 1.0], K) * rng.uniform(0.5, 1.0, K)).astype(T)
    ws, wy, cm = pairs(K, col, max(col, 1), dtype, K) if col else ([], [], None)
    theta = cm.theta if col else 1.3
    M = middle_matrix(cm) if col else np.zeros((0, 0))
    ts = t[order].astype(np.float64)
    dib = d[order].astype(np.float64)
    xs = x[order].astype(np.float64)
    z = np.where(dib > 0, hi - xs, lo - xs)
    W = np.concatenate([np.asarray(w, np.float64)[order][:, None] for w in wy] +
                       [theta * np.asarray(w, np.float64)[order][:, None] for w in ws],
                       axis=1) if col else np.zeros((K, 0))
    p = rng.standard_normal(2 * col) * 0.1
    c = rng.standard_normal(2 * col) * 0.01
    tj = 0.0
    # f'' stays well above the clamp unless the case asks for one; f' places the stop
    probe = walk_rule(ts, dib, z, W, theta, tj, 0.0, 0.0, 1.0, 1.0, p, c, M)
    cum2 = probe["f2"]                                     # cumsum of the f'' steps
    f2 = 2.0 * float(np.max(np.abs(cum2))) + 1.0
    f2_org = f2
    if where == "clamp":
        kc = K // 3
        f2 = f2_org = -0.5 * (cum2[kc - 1] + cum2[kc])      # f'' < 0 after kc
    r0 = walk_rule(ts, dib, z, W, theta, tj, 0.0, f2, f2_org, 1.0, p, c, M)
    # stop at k >= 1  <=>  f1 > B[k] = -F1[k-1] - dt[k] f2_before[k]   (F1: f1 = 0)
    B = np.concatenate(([np.inf], -r0["f1"][:-1] - r0["dt"][1:] * r0["f2_before"][1:]))
    dtm = 10.0 * max(ts[0] - tj, 1e-3)
    if where == "stop0":
        dtm = 0.5 * (ts[0] - tj)
        f1 = -1.0
    elif where == "middle":
        prev = np.minimum.accumulate(B)                     # min over j <= k
        with np.errstate(invalid="ignore"):             # (prev[0] = inf)
            lows = np.flatnonzero(B[1:] < prev[:-1] - 1e-6 * np.abs(prev[:-1])) + 1
        ks = int(lows[np.argmin(np.abs(lows - K // 2))])
        f1 = 0.5 * (B[ks] + prev[ks - 1])
    else:                                                    # never, clamp
        bmin = float(np.min(B[1:])) if K > 1 else 0.0
        f1 = bmin - abs(bmin) - 1.0
    r = walk_rule(ts, dib, z, W, theta, tj, f1, f2, f2_org, dtm, p, c, M)
    kstop, kclamp = _first(r["stop"]), _first(r["clamp"])
    kdone = min(K, kstop, kclamp)
    stopped = kstop < K and kstop <= kclamp
    clamp_at = kclamp if kclamp <= kdone and kclamp < K else -1
    # the case decides clearly: dt_min and dt apart by 1e-8 up to the stop
    kk = min(kdone + 1, K)
    gap = np.abs(r["dtm_before"][:kk] - r["dt"][:kk]) / np.maximum(
        np.maximum(np.abs(r["dtm_before"][:kk]), np.abs(r["dt"][:kk])), 1e-300)
    assert gap.min() > 1e-8
    want_kdone = {"stop0": 0, "never": K, "clamp": K // 3}.get(where)
    if want_kdone is not None:
        assert kdone == want_kdone
    else:
        assert 0 < kdone < K and stopped
    assert (clamp_at >= 0) == (where == "clamp")

    return dict(t=t, order=order, x=x, d=d, ws=ws, wy=wy, theta=theta, M=M, p=p, c=c,
                tj=tj, f1=f1, f2=f2, f2_org=f2_org, dtm=dtm, lo=lo, hi=hi, ts=ts, r=r,
                kdone=kdone, stopped=stopped, clamp_at=clamp_at)


def test_walk_cases_end_where_they_say():
    for K, col, where in WALKS:
        for dtype in DTYPES:
            walk_case(K, col, where, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("K,col,where", WALKS)
def test_stage_cauchy_walk(nsol, K, col, where, dtype):
    """One sorted window walked on the device against walk_rule, with the stop at
    k = 0, inside the window or nowhere, or a clamped f'' (handed back at its k);
    both forms of the column scans (sort_walk_by_key)."""
    import ctypes
    import torch
    from nsol_amd import _lib
    from nsol_amd.device import stream_ptr
    from nsol_amd.lbfgsb_device import _fn
    w = walk_case(K, col, where, dtype)
    t, order, x, d, ws, wy = (w[k] for k in ("t", "order", "x", "d", "ws", "wy"))
    theta, M, p, c, tj, f1, f2, f2_org, dtm, lo, hi, ts, r = (
        w[k] for k in ("theta", "M", "p", "c", "tj", "f1", "f2", "f2_org", "dtm", "lo",
                       "hi", "ts", "r"))
    kdone, stopped, clamp_at = w["kdone"], w["stopped"], w["clamp_at"]
    lib = _lib.load()
    tbk_d, d_d, x_d = _dev(t), _dev(d), _dev(x)
    idx = _dev(order.astype(np.int64))
    wy_d = [_dev(w) for w in wy]
    ws_d = [_dev(w) for w in ws]
    PW = ctypes.c_void_p * max(col, 1)
    wy_p, ws_p = PW(*[w.data_ptr() for w in wy_d]), PW(*[w.data_ptr() for w in ws_d])
    params = _dev(np.concatenate((p, c, M.reshape(-1)))) if col else None
    table = torch.empty(int(lib.nsol_lb_walk_table_doubles(K, col)), dtype=torch.float64,
                        device="cuda")
    tmp = torch.empty(int(lib.nsol_lb_walk_tmp_bytes(K)), dtype=torch.uint8,
                      device="cuda")
    event = torch.zeros(2, dtype=torch.int32, device="cuda")
    out = torch.empty(8 + 4 * max(col, 1), dtype=torch.float64, device="cuda")
    walk = _fn("cauchy_walk", tbk_d)
    j = kdone - 1
    for by_key in (1, 0):
        _lib.set_param("sort_walk_by_key", by_key)
        try:
            _lib.check(walk(
                tbk_d.data_ptr(), d_d.data_ptr(), x_d.data_ptr(), idx.data_ptr(), K,
                ctypes.cast(wy_p, ctypes.c_void_p), ctypes.cast(ws_p, ctypes.c_void_p),
                col, float(theta), lo, hi, tj, f1, f2, f2_org, dtm,
                None if params is None else params.data_ptr(), table.data_ptr(),
                tmp.data_ptr(), tmp.numel(), event.data_ptr(), out.data_ptr(),
                stream_ptr()), "cauchy_walk")
            o = _host(out)
        finally:
            _lib.set_param("sort_walk_by_key", 1)
        assert (int(o[0]), o[1] > 0.5, int(o[2])) == (kdone, stopped, clamp_at)
        if kdone == 0:
            assert (o[3], o[4], o[5], o[6], o[7]) == (0.0, -1.0, f1, f2, dtm)
            continue
        assert o[3] == ts[j] and int(o[4]) == int(order[j])
        tag = "by_key=%d " % by_key
        # each within 1e-12 of what its prefix sum added up (rel_l2 logs the plain
        # relative errors as well)
        for k_, name, sc in ((5, "f1", r["s1"][j]), (6, "f2", r["s2"][j])):
            rel_l2(o[k_], r[name][j], tag + name)
            assert abs(o[k_] - r[name][j]) <= 1e-12 * sc, name
        f1e, f2e = 1e-12 * r["s1"][j], 1e-12 * r["s2"][j]
        rel_l2(o[7], r["dtm"][j], tag + "dtm")
        assert abs(o[7] - r["dtm"][j]) <= (f1e + abs(r["dtm"][j]) * f2e) / \
            (abs(r["f2"][j]) - f2e) * 1.01, "dtm"
        if col:
            pd, cd = o[8:8 + 2 * col], o[8 + 2 * col:8 + 4 * col]
            rel_l2(pd, r["P"][j], tag + "p")
            rel_l2(cd, r["C"][j], tag + "c")
            assert np.all(np.abs(pd - r["P"][j]) <= 1e-12 * r["sP"][j]), "p"
            assert np.all(np.abs(cd - r["C"][j]) <= 1e-12 * r["sC"][j]), "c"


# ---- the other length-n primitives of DeviceBackend against NumpyBackend ------
def _ratio_ties(n, lo, rng):
    """x, d whose smallest feasible step ratio is shared by indices in different
    workgroups and grid-stride lanes (and by neighbours in one wave)."""
    x = rng.uniform(0.5, 0.8, n)                # every other ratio >= 0.2
    d = rng.uniform(-1.0, 1.0, n)
    k = np.unique(np.concatenate((np.linspace(0, n - 1, min(n, 5)).astype(np.int64),
                                  [n // 2 + 1, n - 2])).clip(0, n - 1))
    x[k], d[k] = lo + 0.125, -1.0              # ratio 0.125, the smallest
    return x, d, k


def _ratios(x, d, lo, hi, free=None):
    """The feasible step ratio of every variable (NumpyBackend.truncated_step's
    rule, in the dtype of x and d); inf where nothing limits the step."""
    msk = np.ones(x.size, bool) if free is None else free
    r = np.full(x.size, np.inf)
    dn = msk & (d < 0) & np.isfinite(lo)
    up = msk & (d > 0) & np.isfinite(hi)
    t2 = x.dtype.type(lo) - x if np.isfinite(lo) else None
    if t2 is not None:
        r[dn] = np.where(t2[dn] >= 0, 0.0, t2[dn] / d[dn])
    t2 = x.dtype.type(hi) - x if np.isfinite(hi) else None
    if t2 is not None:
        r[up] = np.where(t2[up] <= 0, 0.0, t2[up] / d[up])
    return r


def _check_ratio_min(be, x, d, lo, hi, iw=None):
    """DeviceBackend._ratio_min: the smallest ratio and, among ties, the smallest
    index (np.argmin's)."""
    free = None if iw is None else iw <= 0
    r = _ratios(x, d, lo, hi, free)
    k = int(np.argmin(r))
    got = be._ratio_min(_dev(x), _dev(d), lo, hi, None if iw is None else _dev(iw))
    if np.isfinite(r[k]):
        assert got == (float(r[k]), k)
    else:
        assert got[1] == -1
    return r, k


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [7, 4097, (1 << 20) + 3])
def test_device_primitives_match_numpy_backend(nsol, n, dtype):
    from nsol_amd.lbfgsb_device import DeviceBackend
    T = np.dtype(dtype).type
    tol = 1e-12 if dtype == np.float64 else 1e-6
    rng = np.random.default_rng(n)
    be, nb = DeviceBackend(), NumpyBackend()
    lo, hi = 0.0, 1.0
    x = rng.uniform(-0.2, 1.2, n).astype(T)
    g = rng.standard_normal(n).astype(T)
    iw = rng.choice(np.array([-1, 0, 0, 1, 2, 3], np.int8), n)
    free = iw <= 0
    X, G, IW = _dev(x), _dev(g), _dev(iw)
    for b in ((lo, hi), (lo, np.inf), (-np.inf, hi), (-np.inf, np.inf)):
        assert be.projgr(X, G, *b) == nb.projgr(x, g, *b)
    assert be.count_free(IW) == nb.count_free(iw)
    # sums: float64 over the dtype's values
    a, b_, c = (rng.standard_normal(n).astype(T) for _ in range(3))
    out, dd, dc = be.diff_dots(_dev(a), _dev(b_), _dev(c))
    diff = a - b_
    assert np.array_equal(_host(out), diff)
    d64 = diff.astype(np.float64)
    assert abs(dd - d64.dot(d64)) <= tol * d64.dot(d64)
    assert abs(dc - d64.dot(c.astype(np.float64))) <= tol * np.abs(d64).dot(np.abs(c))
    vecs = [rng.standard_normal(n).astype(T) for _ in range(5)]
    V = [_dev(w) for w in vecs]
    for mask, msk in ((None, np.ones(n, bool)), (IW, free)):
        got = be.dots(V, G, mask)
        for w, r in zip(vecs, got):
            w64, g64 = w.astype(np.float64)[msk], g.astype(np.float64)[msk]
            assert abs(r - w64.dot(g64)) <= tol * np.abs(w64).dot(np.abs(g64)) + 1e-300
    # combinations: float64 over the dtype's values, formed in the dtype
    ws, wy = vecs[:2], vecs[2:4]
    z = rng.uniform(0.0, 1.0, n).astype(T)
    cs, cy, theta = [0.3, -0.7], [1.1, 0.4], 1.7
    r = be.reduced_gradient(_dev(z), X, G, theta, V[:2], V[2:4], cs, cy, IW)
    f64 = lambda v: np.asarray(v, np.float64)
    want = nb.reduced_gradient(f64(z), f64(x), f64(g), theta, [f64(w) for w in ws],
                               [f64(w) for w in wy], cs, cy, iw)
    assert rel_l2(_host(r), want, "reduced_gradient") <= tol * 10
    assert np.all(_host(r)[~free] == 0)
    rr = want.astype(T)
    dv = be.subspace_direction(_dev(rr), V[:2], V[2:4], cy, cs, theta, IW)
    want = nb.subspace_direction(f64(rr), [f64(w) for w in ws], [f64(w) for w in wy],
                                 cy, cs, theta, iw)
    assert rel_l2(_host(dv), want, "subspace_direction") <= tol * 10
    assert np.all(_host(dv)[~free] == 0)
    # projection and the step ratios: the dtype's own arithmetic, exact
    xcp = rng.uniform(0.0, 1.0, n).astype(T)
    d = (0.5 * rng.standard_normal(n)).astype(T)
    for mask, m in ((IW, iw), (None, None)):
        xn, hit = be.project_step(_dev(xcp), _dev(d), lo, hi, mask)
        xw, hw = nb.project_step(xcp, d, lo, hi, m)
        assert np.array_equal(_host(xn), xw) and hit == hw
    for b in ((lo, hi), (lo, np.inf), (-np.inf, np.inf)):
        xr, dr, k = _ratio_ties(n, b[0] if np.isfinite(b[0]) else 0.0, rng)
        xr, dr = xr.astype(T), dr.astype(T)
        r, kmin = _check_ratio_min(be, xr, dr, *b)
        if np.isfinite(b[0]):
            assert kmin == k[0] and np.count_nonzero(r == r[kmin]) == k.size
        _check_ratio_min(be, xr, dr, *b, iw)
        for mask, m in ((IW, iw), (None, None)):
            got = _host(be.truncated_step(_dev(xr), _dev(dr), *b, mask))
            assert np.array_equal(got, nb.truncated_step(xr, dr, *b, m))
        assert be.max_step(_dev(xr), _dev(dr), *b, 1e10) == \
            nb.max_step(xr, dr, *b, 1e10)
        # x at the bound with d pointing out of the box: ratios of exactly 0, tied
        # at the later indices of the run
        x0 = xr.copy()
        if np.isfinite(b[0]):
            x0[k[1:]] = T(b[0])
            r, kmin = _check_ratio_min(be, x0, dr, *b)
            assert r[kmin] == 0.0 and kmin == k[min(1, k.size - 1)]
            _check_ratio_min(be, x0, dr, *b, iw)
        got = _host(be.truncated_step(_dev(x0), _dev(dr), *b, None))
        assert np.array_equal(got, nb.truncated_step(x0, dr, *b, None))
        assert be.max_step(_dev(x0), _dev(dr), *b, 1e10) == \
            nb.max_step(x0, dr, *b, 1e10)
