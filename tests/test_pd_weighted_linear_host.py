"""CPU side of the tests of the tile bodies' WGT and LIN forms (k_pd_w, k_pd_lin, k_pdl_stack)
and of the element-wise kernels beside them (k_prox_w, k_pdl_dual_data): the restatements
of nsol_amd/vector_numpy.py against the loops the suite already holds to the oracle and to
the L-BFGS-B minimiser, the mirror of the launch path with stacked members, the coverage of
pd_step_cases.catalogue_stack, the float32 gates against an np.float32 emulation (sound) and
against mutated references (teeth), the branch shares and the tie states.
"""
import numpy as np
import pytest

import pd_step_cases as pc
from nsol_amd import vector_numpy as vn
from test_pd_linear_host import blur, box_kernel, default_steps, pd_linear_restatement
from test_pd_steps_host import emulate
from test_pd_weighted_host import mixed_weights, pd_weighted_denoise

BOTH = pc.BOTH


# ============================================ 1. the restatements against the known loops
@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
@pytest.mark.parametrize("shape", [(61,), (7, 13), (4, 5, 9)])
def test_weighted_iterations_compose_to_the_weighted_loop(shape, iso):
    """pd_weighted_iteration, iterated under the oracle's schedule, against
    pd_weighted_denoise (test_pd_weighted_host.py): array_equal.  Both loops perform the same
    float64 operations in the same order -- the taps are scaled by w = 1 / h and multiplied,
    the data prox is the very same function -- so nothing may differ."""
    from oracle import nsol_oracle as orc
    d = len(shape)
    spacing = np.array(pc.SPACING[:d])
    w = tuple(1. / pc.SPACING[a] if a < d else 1. for a in range(3))
    rng = np.random.default_rng(21 + d)
    b = 50. + 30. * rng.standard_normal(shape)
    wt = mixed_weights(shape, 3)
    junk = b.copy()
    junk[wt == 0] = np.nan
    for reg in ("TV", "Huber"):
        for data in ("L2", "L1"):
            alpha = 0.05 if data == "L2" else 0.6
            xs, lmbda = float(np.max(b)), 1. / alpha
            want = pd_weighted_denoise(junk, wt, shape, reg, data, alpha, 6, 4.0, "ALG2",
                                       iso=iso, spacing=spacing, x_scale=xs, x0=b,
                                       scaled=True)
            sig, ta, th = orc.pd_schedule("ALG2", 4.0, lmbda, 6)
            x = b / xs
            xbar, p = x.copy(), None
            for n in range(6):
                hden = 1. + sig[n] * 0.05 if reg == "Huber" else 1.
                p, x, xbar = vn.pd_weighted_iteration(
                    xbar, x, junk / xs, wt, p, sig[n], hden, ta[n], ta[n] * lmbda, th[n], w,
                    data == "L1", np.float64, iso)
            assert np.all(np.isfinite(x))
            assert np.array_equal(x.reshape(-1), want), (reg, data)


@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
@pytest.mark.parametrize("shape", [(61,), (7, 13), (4, 5, 9)])
def test_linear_iterations_compose_to_the_linear_restatement(shape, iso):
    """pdl_dual_data and pd_lin_iteration around the blur of test_pd_linear_host.py, iterated,
    against pd_linear_restatement after every iteration (x, p and q): array_equal.  The
    operations and their order are the same; the loop there clips with np.clip where the
    kernel selects, which gives the same numbers and can differ in the sign of a zero
    only, which array_equal does not see (the tie states below do)."""
    d = len(shape)
    spacing = np.array(pc.SPACING[:d])
    w = tuple(1. / pc.SPACING[a] if a < d else 1. for a in range(3))
    rng = np.random.default_rng(31 + d)
    obs = 50. + 30. * rng.standard_normal(shape)
    wt = mixed_weights(shape, 4)
    kernel = box_kernel(d)
    xs, alpha = float(obs.max()), 0.05
    for reg in ("TV", "huber"):
        for data in ("ell2", "ell1"):
            for bounds in (None, (0.3, 0.9)):
                trace = []
                pd_linear_restatement(obs, kernel, shape, reg, data, alpha, 5, weights=wt,
                                      bounds=bounds, iso=iso, spacing=spacing, x_scale=xs,
                                      trace=trace)
                _, tau, sigma = default_steps(shape, kernel, spacing)
                lo, hi = (-np.inf, np.inf) if bounds is None else bounds
                hden = 1. + sigma * 0.05 if reg == "huber" else 1.
                bt = obs / xs
                x = bt.copy()
                xbar, p, q = x.copy(), None, np.zeros(shape)
                for n in range(5):
                    q = vn.pdl_dual_data(q, blur(xbar, kernel), bt, wt, sigma, 1. / alpha,
                                         data == "ell1")
                    g = blur(q, kernel, adjoint=True)
                    p, x, xbar = vn.pd_lin_iteration(xbar, x, g, p, sigma, hden, tau, 1.,
                                                     lo, hi, w, np.float64, iso)
                    label = (reg, data, bounds, n)
                    assert np.array_equal(x, trace[n][0]), label
                    # (the loop there keeps component a on array axis a, x last)
                    assert np.array_equal(p[::-1], trace[n][1]), label
                    assert np.array_equal(q, trace[n][2]), label


def test_box_in_rounds_towards_the_inside():
    f = np.float32
    up = lambda v: float(np.nextafter(f(v), f(np.inf)))
    dn = lambda v: float(np.nextafter(f(v), f(-np.inf)))
    assert vn.box_in(-0.46, 0.55, np.float64) == (-0.46, 0.55)
    lo, hi = vn.box_in(-0.46, 0.55, np.float32)
    assert -0.46 <= lo <= up(-0.46) and dn(0.55) <= hi <= 0.55
    assert lo == float(f(lo)) and hi == float(f(hi))
    assert float(f(-0.46)) < -0.46 and lo == up(float(f(-0.46)))      # nearest was outside
    assert float(f(0.55)) > 0.55 and hi == dn(float(f(0.55)))
    assert vn.box_in(0.25, 0.75, np.float32) == (0.25, 0.75)          # float32 numbers stay
    assert vn.box_in(-np.inf, np.inf, np.float32) == (-np.inf, np.inf)
    assert vn.box_in(0.1, 0.1, np.float32) == (float(f(0.1)),) * 2    # lo == hi: nearest
    # narrower than one spacing with no float32 inside: as rounded to nearest
    a = float(f(0.1))
    lo, hi = a + 1e-10, a + 2e-10
    assert vn.box_in(lo, hi, np.float32) == (a, a)
    assert not pc.box_holds_a_number((lo, hi), np.float32)
    assert pc.box_holds_a_number(pc.BOX, np.float32) and pc.box_holds_a_number(pc.BOX, np.float64)
    for box in pc.BOXES:
        assert float(f(box[0])) != box[0] or not np.isfinite(box[0])
        assert float(f(box[1])) != box[1] or not np.isfinite(box[1])


def test_lin_step_selects_as_the_kernel_does():
    x = np.array([-0., 0., -1., 2., 0.25])
    z = np.zeros(5)
    got = vn.pd_lin_step(x, z, z, 0.5, 0., 0.75)
    assert np.array_equal(got, [0., 0., 0., 0.75, 0.25])
    assert np.signbit(got[0]) and not np.signbit(got[1]) and not np.signbit(got[2])
    assert np.array_equal(vn.pd_lin_step(x, z, z, 0.5, 0.25, 0.25), [0.25] * 5)
    w = np.array([0., 1., 0., 2.])
    bt = np.array([np.nan, 1., np.inf, -1.])
    u = np.array([3., 3., -2., -2.])
    assert np.array_equal(vn.prox_data_w(u, bt, w, 0.5, False), [3., 3.5 / 1.5, -2., -1.5])
    assert np.array_equal(vn.prox_data_w(u, bt, w, 0.5, True), [3., 2.5, -2., -1.])
    got = vn.pdl_dual_data(u, None, bt, w, 0.5, 0., True)
    assert np.array_equal(got, [0., 0., 0., 0.]) and list(np.signbit(got)) == [0, 0, 0, 1]


# ============================================================ 2. the mirror with members
def test_the_mirror_with_members_on_plans_worked_out_by_hand():
    """pd_auto_rows_per_lane and pd_plan_grid with members, followed by hand."""
    F = pc.Form
    for dtype in BOTH:
        # 17 columns: ragged, 16 lanes, one tile along x; two rows per lane: TY = 32, two
        # tile rows; 2 * 32 pairs of planes = 64 < 512 alone: one row per lane, TY = 16,
        # three tile rows; z chunk: ceil(64 / ceil(4096 / 3)) = 1 -> 2, 32 chunks
        assert pc.plan((64, 33, 17), dtype).form == F("rag", 16, 1, 3, 1, 3, 32, 0)
        # 8 members: 16 * 32 = 512: two rows per lane; ceil(4096 / 16) = 256 -> chunks of 2
        assert pc.plan((64, 33, 17), dtype, members=8).form == F("rag", 16, 2, 3, 1, 2, 32, 0)
        assert pc.plan((64, 33, 17), dtype, members=7).form.RY == 1
        assert pc.plan((33, 17), dtype).form == F("rag", 16, 1, 2, 1, 3, 1, 0)
        assert pc.plan((33, 17), dtype, members=256).form == F("rag", 16, 2, 2, 1, 2, 1, 0)
        assert pc.plan((33, 17), dtype, members=255).form.RY == 1
        assert pc.plan((259,), dtype, members=4096).form.RY == 1           # 1-D: always one
    # 300 planes, 2 x 5 tiles of 256 x 4, 3 members: 30 tiles, ceil(4096 / 30) = 137 chunks
    # wanted, ceil(300 / 137) = 3 planes a chunk; alone: ceil(4096 / 10) = 410 -> 1 -> 2
    assert pc.plan((300, 17, 260), np.float32, members=3, ry=1).zchunk == 3
    assert pc.plan((300, 17, 260), np.float32, ry=1).zchunk == 2
    assert pc.plan((1000, 17, 260), np.float32, members=3, ry=1).zchunk == 8   # 1000 / 137
    assert pc.plan((1000, 17, 260), np.float32, ry=1).zchunk == 3              # 1000 / 410
    # the automatic rows: 2 x 3 tiles of 256 x 8, 3 members: 18 * 150 >= 512: two rows;
    # ceil(4096 / 18) = 228 chunks wanted, ceil(300 / 228) = 2 planes: 150 chunks
    assert pc.plan((300, 17, 260), np.float32, members=3).form == \
        pc.Form("vec", 64, 2, 3, 2, 3, 150, 0)


def _wanted_forms():
    forms = set()
    for kind in ("vec", "rag", "elem"):
        for LX in (64, 16) if kind != "elem" else (16,):
            forms.add((kind, LX, 1, 1))
            forms |= {(kind, LX, RY, ndim) for RY in (1, 2) for ndim in (2, 3)}
    return forms


@pytest.mark.parametrize("dtype", BOTH)
def test_the_stack_catalogue_reaches_every_form_without_knobs(dtype):
    VW = pc.vw(dtype)
    cases = pc.catalogue_stack(dtype)
    plans = {cs.name: pc.scase_plan(cs, dtype) for cs in cases}
    print("\n%-18s %-12s off members  form (%s)" % ("case", "shape", pc.suffix(dtype)))
    for cs in cases:
        print("%-18s %-12s %3d %7d  %s" % (cs.name, "x".join(map(str, cs.shape)), cs.offset,
                                           cs.members, tuple(plans[cs.name].form)))
    edged, every = set(), set()
    for cs in cases:
        pl = plans[cs.name]
        f, (ndim, nz, ny, nx) = pl.form, pc.dims3(cs.shape)
        every.add((f.kind, f.LX, f.RY, f.NDIM))
        ok = f.kind == "elem" or (f.ntx >= 2 and nx % pl.TX != 0)
        if ndim >= 2:
            ok = ok and f.nty >= 2 and ny % pl.TY != 0
        if ndim >= 3:
            ok = ok and f.nzc >= 2 and nz % pl.zchunk != 0
        if ok:
            edged.add((f.kind, f.LX, f.RY, f.NDIM))
        if f.kind == "elem":                        # single elements: short rows only
            assert nx < 2 * VW and f.LX == 16 and f.ntx == 1
        assert int(np.prod(cs.shape)) <= pc.MAX_VOXELS
    assert every == _wanted_forms() and len(every) == 25
    assert _wanted_forms() <= edged, sorted(_wanted_forms() - edged)
    # a stack whose form is not its member's: in 3-D and in 2-D
    for ndim in (2, 3):
        sw = [cs for cs in cases if cs.members > 1 and len(cs.shape) == ndim and
              pc.scase_plan(cs, dtype, 1).form.RY == 1 and plans[cs.name].form.RY == 2]
        assert sw, ndim
        assert any(alone.shape == cs.shape and alone.members == 1 for cs in sw
                   for alone in cases)
    assert plans["switch-3d-alone"].form[:6] == ("rag", 16, 1, 3, 1, 3)
    assert plans["switch-3d-stack"].form[:6] == ("rag", 16, 2, 3, 1, 2)
    rag = [cs for cs in cases if plans[cs.name].form.kind == "rag"]
    for LX in (64, 16):
        valid = {cs.shape[-1] % VW for cs in rag if plans[cs.name].form.LX == LX}
        assert set(range(1, VW)) <= valid, (LX, valid)
    assert any(-(-cs.shape[-1] // VW) == 64 and plans[cs.name].form.LX == 64 for cs in rag)
    for axis in range(3):
        assert any(pc.dims3(cs.shape)[1 + axis] == 1 and len(cs.shape) == 3 for cs in cases)
    assert any(cs.shape == (1, 1, 1) for cs in cases) and any(cs.shape == (1,) for cs in cases)
    slabbed = [plans[cs.name].form for cs in cases if plans[cs.name].form.slab]
    assert slabbed and all(f.nty >= 17 for f in slabbed)
    assert any(pc.blocks(f)[0] > pc.blocks(f)[1] for f in slabbed)
    assert {cs.offset for cs in cases} == {0, 1, 3}
    off = [cs for cs in cases if cs.offset and cs.shape[-1] % VW == 0]
    assert off and all(plans[cs.name].form.kind == "rag" for cs in off)
    for d in (1, 2, 3):
        assert any(cs.unit and len(cs.shape) == d for cs in cases)
        assert any(not cs.unit and len(cs.shape) == d for cs in cases)
    for name in pc.STACK_TIE_CASES:
        assert pc.scase_named(name, dtype).members == 1


def test_the_states_hold_what_they_promise():
    for dtype in BOTH:
        for cs in pc.catalogue_stack(dtype):
            st = pc.weights_state(cs.shape, dtype)
            wt, bt, n = st["wt"], st["bt"], int(np.prod(cs.shape))
            assert np.all(wt[~np.isfinite(bt)] == 0)
            assert wt.reshape(-1)[0] == 0 and wt.reshape(-1)[-1] == 0   # on every face
            pl = pc.scase_plan(cs, dtype)
            if pl.form.ntx >= 2:
                row = wt.reshape(-1, cs.shape[-1])[0]
                assert row[pl.TX - 1] == 0 and row[pl.TX] == 0
            if n >= pc.BRANCH_MIN_VOXELS:
                assert np.isnan(bt).any() and np.isposinf(bt).any() and np.isneginf(bt).any()
                assert np.any(wt == 1) and np.any((wt > 0) & (wt < 1)) and np.any(wt > 2)
            if cs.members > 1:
                a, b = pc.weights_state(cs.shape, dtype, 1), pc.lin_state(cs.shape, dtype, 1)
                assert not np.array_equal(a["wt"], wt) or n < 4
                assert not np.array_equal(b["g"], pc.lin_state(cs.shape, dtype)["g"])
                assert not np.array_equal(a["x"], st["x"])


# ========================================================= 3. an emulation in the type
def _kt(T, pn, w):
    d = pn.shape[0]
    kt = None
    for a in range(d):
        lo = vn.shifted(pn[a], d - 1 - a, False)
        term = pn[a] * (-T(w[a])) + lo * T(w[a])
        kt = term if kt is None else kt + term
    return kt


def emulate_primal(T, p, st, sc, w, form, arg, mut=None):
    """(x_new, xbar_new) of the WGT (form "wgt", arg = l1) or LIN (form "lin", arg = the
    caller's box) primal half on the dual field p in the arithmetic of type T, one NumPy
    operation per kernel operation, written from nsol_pd_fused_body.hpp and
    nsol_pd_weighted.hpp.  mut names a fault:
      tau_kt_plus_g     tau * kt + g
      box_nearest       the float32 box rounded to nearest, not inward
      selects_reversed  u > lo ? u : lo, then c < hi ? c : hi (the bound's zero, not u's)
      one_plus_tl       (u + t bt) / (1 + tl)
      w0_gives_bt       w == 0 returns bt"""
    f = lambda a: np.asarray(a, np.float64).astype(T)
    pn, x = f(p), f(st["x"])
    ta, th = T(sc.tau), T(sc.theta)
    kt = _kt(T, pn, w)
    with np.errstate(invalid="ignore", over="ignore"):
        if form == "lin":
            g = f(st["g"])
            lo, hi = (T(v) for v in vn.box_in(arg[0], arg[1], T))
            if mut == "box_nearest":
                lo, hi = T(arg[0]), T(arg[1])
            u = x - (ta * kt + g) if mut == "tau_kt_plus_g" else x - ta * (kt + g)
            if mut == "selects_reversed":
                cl = np.where(u > lo, u, lo)
                xn = np.where(cl < hi, cl, hi)
            else:
                cl = np.where(u < lo, lo, u)
                xn = np.where(cl > hi, hi, cl)
        else:
            bt, wt, tl = f(st["bt"]), f(st["wt"]), T(sc.tl)
            u = x - ta * kt
            t = tl * wt
            if arg:
                dd = u - bt
                r = bt + np.maximum(np.abs(dd) - t, T(0)) * np.sign(dd)
            else:
                r = (u + t * bt) / (T(1) + (tl if mut == "one_plus_tl" else t))
            xn = np.where(wt == 0, bt if mut == "w0_gives_bt" else u, r)
        xb = xn + th * (xn - x)
    assert xn.dtype == np.dtype(T) and xb.dtype == np.dtype(T)
    return xn.astype(np.float64), xb.astype(np.float64)


def emulate_prox_w(T, u, bt, wt, tl, l1):
    u, bt, wt, tl = (np.asarray(a, np.float64).astype(T) for a in (u, bt, wt, tl))
    with np.errstate(invalid="ignore", over="ignore"):
        t = tl * wt
        if l1:
            dd = u - bt
            r = bt + np.maximum(np.abs(dd) - t, T(0)) * np.sign(dd)
        else:
            r = (u + t * bt) / (T(1) + t)
    out = np.where(wt == 0, u, r)
    assert out.dtype == np.dtype(T)
    return out.astype(np.float64)


def emulate_dual_data(T, q, t, bt, wt, sigma, lmbda, l1, mut=None):
    """k_pdl_dual_data in type T; mut "c_plus_lmbda": (v c) / (c + lmbda)."""
    f = lambda a: np.asarray(a, np.float64).astype(T)
    q, bt, sg, lm = f(q), f(bt), T(sigma), T(lmbda)
    w = np.ones_like(q) if wt is None else f(wt)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = q + sg * (f(t) - bt) if t is not None else q - sg * bt
        cc = lm * w
        if l1:
            r = np.where(v < -cc, -cc, v)
            r = np.where(r > cc, cc, r)
        else:
            r = (v * cc) / (cc + (lm if mut == "c_plus_lmbda" else sg))
    out = np.where(w == 0, T(0), r)
    assert out.dtype == np.dtype(T)
    return out.astype(np.float64)


def _dual(T, cs, m, sc, huber, iso, has_p):
    st = pc.member_state(cs.shape, T, m)
    return emulate(T, st, sc, pc.scase_weights(cs), huber, False, iso, has_p)[0]


def _judge_primal(got, st, sc, w, dtype, form, arg, exact=False):
    """[(array, bad, ratio)] of (x_new, xbar_new) on the dual field got[0]."""
    primal = (lambda p: pc.lin_expected(p, st, sc, w, dtype, arg)) if form == "lin" else \
        (lambda p: pc.weighted_expected(p, st, sc, w, dtype, arg))
    return pc.judge(got, st, sc, w, dtype, False, False, False, True, exact, "xb", primal)


DD_LENGTHS = (1, 2, 3, 63, 64, 65, 1021, 2 * 512 + 37)


def elementwise_inputs(n, dtype):
    rng = np.random.default_rng(7000 + n)
    r = lambda s=1.: pc.rounded(s * rng.standard_normal(n), dtype)
    st = pc.weights_state((n,), dtype)
    return dict(q=r(), t=r(), u=r(), bt=st["bt"], wt=st["wt"])


def test_the_gates_are_sound_for_an_ieee_kernel():
    """Every case of catalogue_stack (member 0; a second member of every stack), emulated
    in np.float32 and judged as the GPU results are: inside the gate at every voxel; in
    float64 the emulation equals the restatement.  The worst ratios are printed."""
    worst = {}

    def take(key, out, label, dtype):
        for name, bad, ratio in out:
            assert not np.any(bad), (label, pc.suffix(dtype), key, name, ratio)
            if not pc.is64(dtype):
                k = "%s %s" % (key, name)
                worst[k] = max(worst.get(k, 0.), ratio)

    for dtype in BOTH:
        for k, cs in enumerate(pc.catalogue_stack(dtype)):
            w = pc.scase_weights(cs)
            for m in (0, 1) if cs.members > 1 else (0,):
                for c4 in range(4):
                    huber, iso, has_p = bool(c4 & 1), bool(c4 & 2), (c4 + k + m) % 2 == 0
                    p = _dual(dtype, cs, m, pc.RANDOM, huber, iso, has_p)
                    st = pc.lin_state(cs.shape, dtype, m)
                    for box in pc.BOXES if c4 == 0 else pc.BOXES[:1]:
                        got = (p,) + emulate_primal(dtype, p, st, pc.RANDOM, w, "lin", box)
                        take("lin", _judge_primal(got, st, pc.RANDOM, w, dtype, "lin", box),
                             cs.name, dtype)
                        if pc.box_holds_a_number(box, dtype):
                            assert np.all((got[1] >= box[0]) & (got[1] <= box[1]))
                    st = pc.weights_state(cs.shape, dtype, m)
                    for l1 in (False, True):
                        got = (p,) + emulate_primal(dtype, p, st, pc.WEIGHTED, w, "wgt", l1)
                        take("weighted %s" % ("l1" if l1 else "l2"),
                             _judge_primal(got, st, pc.WEIGHTED, w, dtype, "wgt", l1),
                             cs.name, dtype)
        for n in DD_LENGTHS + (2048 * 256 + 37,):
            a = elementwise_inputs(n, dtype)
            for l1 in (False, True):
                got = emulate_prox_w(dtype, a["u"], a["bt"], a["wt"], pc.TL, l1)
                want, R, S = pc.prox_w_expected(a["u"], a["bt"], a["wt"], pc.TL, l1, dtype)
                take("k_prox_w %s" % ("l1" if l1 else "l2"),
                     [("out",) + pc.excess(got, want, R, S, dtype)], n, dtype)
                zero = a["wt"] == 0
                assert np.array_equal(got[zero], a["u"][zero])
                for t in (a["t"], None):
                    for wt in (a["wt"], None):
                        bt = a["bt"] if wt is not None else np.where(
                            np.isfinite(a["bt"]), a["bt"], 0.5)
                        got = emulate_dual_data(dtype, a["q"], t, bt, wt, pc.DD_SIGMA,
                                                pc.DD_LMBDA, l1)
                        want, R, S = pc.dual_data_expected(a["q"], t, bt, wt, pc.DD_SIGMA,
                                                           pc.DD_LMBDA, l1, dtype)
                        take("k_pdl_dual_data %s" % ("l1" if l1 else "l2"),
                             [("q",) + pc.excess(got, want, R, S, dtype)], n, dtype)
    for key in sorted(worst):
        print("emulation / gate, worst err / (R u S): %-32s %.3f" % (key, worst[key]))
    assert worst and max(worst.values()) <= 1.


# ================================================================= 4. the gates have teeth
def _seam(cs, dtype):
    pl = pc.scase_plan(cs, dtype)
    return pl.TX if pl.form.ntx >= 2 else None


@pytest.mark.parametrize("dtype", BOTH)
def test_the_gates_refuse_mutated_references(dtype):
    """Each fault, written into the emulation, falls outside the gate (float64: differs) on
    at least one case where the unmutated emulation passes."""
    def failing(form, arg, mut, sc, state_of, exact=False, has_p=True, names=None):
        red = set()
        for cs in (pc.scase_named(n, dtype) for n in names or pc.STACK_TIE_CASES):
            w = pc.weights(cs.shape, True) if exact else pc.scase_weights(cs)
            st = state_of(cs)
            p = (emulate(dtype, dict(st, bt=st["x"]), sc, w, False, False, False, has_p)[0]
                 if exact else _dual(dtype, cs, 0, sc, False, False, has_p))
            got = (p,) + emulate_primal(dtype, p, st, sc, w, form, arg, mut)
            if any(np.any(bad) for _, bad, _ in
                   _judge_primal(got, st, sc, w, dtype, form, arg, exact)):
                red.add(cs.name)
        return red

    lin = lambda cs: pc.lin_state(cs.shape, dtype)
    wgt = lambda cs: pc.weights_state(cs.shape, dtype)
    assert failing("lin", pc.BOX, None, pc.RANDOM, lin) == set()
    assert failing("lin", pc.BOX, "tau_kt_plus_g", pc.RANDOM, lin)
    for l1 in (False, True):
        assert failing("wgt", l1, None, pc.WEIGHTED, wgt) == set()
        assert failing("wgt", l1, "w0_gives_bt", pc.WEIGHTED, wgt)
    assert failing("wgt", False, "one_plus_tl", pc.WEIGHTED, wgt)
    # the reversed selects hand back the bound's zero for u = -0.0 on lo = 0: the sign of a
    # zero is all that differs, and the tie state sees it
    tie = lambda cs: pc.lin_tie_state(cs.shape, dtype, _seam(cs, dtype), "zero")
    box = pc.LIN_TIE_BOXES["zero"]
    assert failing("lin", box, None, pc.TIE, tie, exact=True, has_p=False) == set()
    assert failing("lin", box, "selects_reversed", pc.TIE, tie, exact=True, has_p=False)
    if not pc.is64(dtype):
        # the box rounded to nearest moves a clipped x by one float32 spacing: far less than
        # R u S, so it is the rule that a u well outside the box must come back as box_in's
        # bound, bit for bit, that puts this mutant outside the gate -- and the iterates
        # leave the caller's box, which the GPU test asserts in double as well
        assert failing("lin", pc.BOX, "box_nearest", pc.RANDOM, lin)
        cs = pc.scase_named("unit-3d", dtype)
        p = _dual(dtype, cs, 0, pc.RANDOM, False, False, True)
        xn, _ = emulate_primal(dtype, p, lin(cs), pc.RANDOM, pc.scase_weights(cs), "lin",
                               pc.BOX, "box_nearest")
        assert np.any(xn < pc.BOX[0]) and np.any(xn > pc.BOX[1])
        xn, _ = emulate_primal(dtype, p, lin(cs), pc.RANDOM, pc.scase_weights(cs), "lin",
                               pc.BOX)
        assert np.all((xn >= pc.BOX[0]) & (xn <= pc.BOX[1]))
    a = elementwise_inputs(1021, dtype)
    args = (a["q"], a["t"], a["bt"], a["wt"], pc.DD_SIGMA, pc.DD_LMBDA, False)
    want, R, S = pc.dual_data_expected(*args, dtype)
    assert not np.any(pc.excess(emulate_dual_data(dtype, *args), want, R, S, dtype)[0])
    assert np.any(pc.excess(emulate_dual_data(dtype, *args, mut="c_plus_lmbda"), want, R, S,
                            dtype)[0])


# ================================================================== 5. the branch shares
def test_at_least_a_twentieth_of_every_case_takes_each_branch():
    lo = {}
    for dtype in BOTH:
        for cs in pc.catalogue_stack(dtype):
            if int(np.prod(cs.shape)) < pc.BRANCH_MIN_VOXELS:
                continue
            for k, f in pc.stack_branch_shares(cs, dtype).items():
                assert f >= 0.05, (cs.name, pc.suffix(dtype), k, f)
                lo[k] = min(lo.get(k, 1.), f)
    for k in sorted(lo):
        print("branch share, least: %-24s %5.1f %%" % (k, 100 * lo[k]))
    assert len(lo) == 6


# ===================================================================== 6. the tie states
@pytest.mark.parametrize("dtype", BOTH)
def test_the_tie_states_are_exact_in_the_emulation(dtype):
    up = lambda v: float(np.nextafter(dtype(v), dtype(np.inf)))
    for name in pc.STACK_TIE_CASES:
        cs = pc.scase_named(name, dtype)
        assert int(np.prod(cs.shape)) >= pc.BRANCH_MIN_VOXELS
        w, seam = pc.weights(cs.shape, True), _seam(cs, dtype)
        for kind, box in pc.LIN_TIE_BOXES.items():
            st = pc.lin_tie_state(cs.shape, dtype, seam, kind)
            u = (st["x"] - 0.5 * st["g"]).reshape(-1)
            for v in (box[0], box[1], up(box[0]), up(box[1])):
                assert np.any(u == v), (kind, v)
            assert np.any((u == 0) & np.signbit(u))
            assert np.any(u < box[0]) and np.any(u > box[1])
            p = emulate(dtype, dict(st, bt=st["x"]), pc.TIE, w, False, False, False, False)[0]
            assert not p.any()
            got = (p,) + emulate_primal(dtype, p, st, pc.TIE, w, "lin", box)
            for _, bad, _ in _judge_primal(got, st, pc.TIE, w, dtype, "lin", box, True):
                assert not np.any(bad), (name, kind, pc.first_bad(bad, cs.shape))
        st = pc.wgt_tie_state(cs.shape, dtype, seam)
        d, t = np.abs(st["x"] - st["bt"]).reshape(-1), (pc.TIE.tl * st["wt"]).reshape(-1)
        with np.errstate(invalid="ignore"):
            for wv in (0.5, 1., 2., 2. ** -20):
                on = st["wt"].reshape(-1) == wv
                assert np.any(on & (d == t)) and np.any(on & (d > t) & (d < t * (1 + 1e-6)))
                assert np.any(on & (d < t) & (d > t * (1 - 1e-6)))
        assert np.any(np.isnan(st["bt"]) & (st["wt"] == 0))
        p = emulate(dtype, dict(st, bt=st["x"]), pc.TIE, w, False, False, False, False)[0]
        got = (p,) + emulate_primal(dtype, p, st, pc.TIE, w, "wgt", True)
        for _, bad, _ in _judge_primal(got, st, pc.TIE, w, dtype, "wgt", True, True):
            assert not np.any(bad), (name, pc.first_bad(bad, cs.shape))
    for lmbda in (1., 0.):
        a = pc.dual_data_tie_state(259, dtype, lmbda)
        for t in (a["t"], None):
            got = emulate_dual_data(dtype, a["q"], t, a["bt"], a["wt"], pc.TIE.sigma, lmbda,
                                    True)
            want = vn.pdl_dual_data(a["q"], t, a["bt"], a["wt"], pc.TIE.sigma, lmbda, True,
                                    dtype)
            bad, _ = pc.excess(got, want, 0, 0., dtype, exact=True)
            assert not np.any(bad), (lmbda, t is None, np.argwhere(bad)[:3])
        cc = lmbda * a["wt"]
        assert np.any((a["q"] == cc) & (cc > 0)) or lmbda == 0
