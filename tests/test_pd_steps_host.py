"""CPU side of the one-iteration primal-dual kernels' tests: the restatement
(nsol_amd/vector_numpy.py: pd_dual_step, pd_primal_step, pd_iteration) against the oracle's
loop, the float32 gate of pd_step_cases.py against an np.float32 emulation (sound) and
against mutated references (teeth), the branch shares of the random states, and the
catalogue's coverage of the launch path's forms as the mirror pd_step_cases.plan sees them.
"""
import numpy as np
import pytest

import pd_step_cases as pc
from nsol_amd import vector_numpy as vn
from test_pd_isotropic_host import pd_iso_denoise

BOTH = pc.BOTH


# ===================================================== 1. restatement against the oracle
def _oracle_states(b, shape, reg, data, alpha, iterations, L2, spacing, iso):
    """The oracle's loop (oracle.nsol_oracle.primal_dual_denoise; iso: pd_iso_denoise of
    test_pd_isotropic_host.py) from the oracle's own functions, keeping the state
    (xbar, x, p) before every iteration; the caller checks its end against the loop it
    repeats."""
    from oracle import nsol_oracle as orc
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    x_scale, d, lmbda = float(np.max(b)), len(shape), 1. / float(alpha)
    sig, ta, th = orc.pd_schedule("ALG2", L2, lmbda, iterations)
    x = b / x_scale
    xbar, p, states = x.copy(), 0, []
    for n in range(iterations):
        states.append((xbar, x, p))
        q = p + sig[n] * orc.grad(xbar.reshape(shape), spacing).reshape(-1)
        if iso:
            p = vn.project_iso(q, d, 1. + sig[n] * 0.05 if reg == "Huber" else None)
        else:
            p = orc.prox_huber_conj(q, sig[n]) if reg == "Huber" else \
                orc.prox_tv_conj(q, sig[n])
        Zshape = (d * shape[0],) + tuple(shape[1:]) if d > 1 else shape
        u = x - ta[n] * orc.grad_adj(p.reshape(Zshape), spacing).reshape(-1)
        prox = orc.prox_ell2_denoising if data == "L2" else orc.prox_ell1_denoising
        xn = prox(u, ta[n] * lmbda, b, x_scale)
        xbar = xn + th[n] * (xn - x)
        x = xn
    states.append((xbar, x, p))
    return states, (sig, ta, th, lmbda, b / x_scale, x_scale)


@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
@pytest.mark.parametrize("shape", [(61,), (7, 13), (4, 5, 9)])
@pytest.mark.parametrize("spaced", [False, True])
def test_restatement_reproduces_the_oracles_next_state(shape, spaced, iso):
    """pd_iteration in float64 from the oracle's state before iteration 0 (p = None) and
    after iterations 0 and 3: the oracle's next state, array_equal.  The oracle scales the
    taps by w = 1 / h and multiplies, as the kernels do, so any spacing serves; 1 / h is
    handed to the restatement as the C ABI would get it."""
    from oracle import nsol_oracle as orc
    d = len(shape)
    spacing = np.array(pc.SPACING[:d]) if spaced else None
    w = tuple(1. / pc.SPACING[a] if spaced and a < d else 1. for a in range(3))
    rng = np.random.default_rng(11 + d)
    b = 50. + 30. * rng.standard_normal(shape)
    for reg in ("TV", "Huber"):
        for data in ("L2", "L1"):
            alpha = 0.05 if data == "L2" else 0.6
            states, (sig, ta, th, lmbda, bt, xs) = _oracle_states(
                b, shape, reg, data, alpha, 6, 4.0, spacing, iso)
            whole = (pd_iso_denoise(b, shape, reg, data, alpha, 6, 4.0, spacing=spacing)
                     if iso else orc.primal_dual_denoise(b, shape, reg, data, alpha, 6, 4.0,
                                                         spacing=spacing))
            assert np.array_equal(states[-1][1] * xs, whole), "the loop is not the oracle's"
            for n in (0, 1, 4):
                xbar, x, p = states[n]
                got = vn.pd_iteration(
                    xbar.reshape(shape), x.reshape(shape), bt.reshape(shape),
                    None if n == 0 else p.reshape((d,) + shape), sig[n],
                    1. + sig[n] * 0.05 if reg == "Huber" else 1., ta[n], ta[n] * lmbda,
                    th[n], w, data == "L1", np.float64, iso)
                nxbar, nx, np_ = states[n + 1]
                label = (reg, data, n)
                assert np.array_equal(got[0].reshape(-1), np_), label
                assert np.array_equal(got[1].reshape(-1), nx), label
                assert np.array_equal(got[2].reshape(-1), nxbar), label


# ========================================================= 2. an emulation in the type
def emulate(T, st, sc, w, huber, l1, iso, has_p=True, mut=None, TX=0, zc=0, bound=1.):
    """One iteration in the arithmetic of type T, one NumPy operation per kernel
    operation (NumPy does not contract), written from the kernels and not from
    vector_numpy.  mut names a fault:
      wrap        the neighbour beyond the last index wraps round
      halo_x      the new dual left of tile column x0 == TX is p_in's
      pzprev      the new dual below the first plane z == zc of the second chunk is p_in's
      theta       theta * (x - x_new)
      tau_for_tl  tau in the place of tl in the l1 prox
    bound: the clamp's bound."""
    f64 = np.dtype(T) == np.float64
    f = lambda a: np.asarray(a, np.float64).astype(T)
    xbar, x, bt, p_in = f(st["xbar"]), f(st["x"]), f(st["bt"]), f(st["p"])
    d = xbar.ndim
    sg, ta, tl, th = T(sc.sigma), T(sc.tau), T(sc.tl), T(sc.theta)
    wt = [T(w[a]) for a in range(d)]
    hden = sc.hden if huber else 1.0
    q = []
    for a in range(d):
        ax = d - 1 - a
        hi = np.roll(xbar, -1, ax) if mut == "wrap" else vn.shifted(xbar, ax, True)
        g = hi * wt[a] + xbar * (-wt[a])
        qa = (p_in[a] if has_p else np.zeros_like(xbar)) + sg * g
        if huber:
            qa = qa / T(hden) if f64 else qa * T(1. / hden)
        q.append(qa)
    if iso:
        s = q[0] * q[0]
        for a in range(1, d):
            s = s + q[a] * q[a]
        m = np.maximum(T(1), np.sqrt(s))
        pn = [qa / m for qa in q]
    else:
        pn = [np.minimum(np.maximum(qa, T(-bound)), T(bound)) for qa in q]
    kt = None
    for a in range(d):
        ax = d - 1 - a
        lo = vn.shifted(pn[a], ax, False)
        if mut == "halo_x" and a == 0:
            lo[..., TX] = p_in[0][..., TX - 1]
        if mut == "pzprev" and a == 2:
            lo[zc] = p_in[2][zc - 1]
        term = pn[a] * (-wt[a]) + lo * wt[a]
        kt = term if kt is None else kt + term
    u = x - ta * kt
    if l1:
        t = ta if mut == "tau_for_tl" else tl
        dd = u - bt
        xn = bt + np.maximum(np.abs(dd) - t, T(0)) * np.sign(dd)
    elif f64:
        xn = (u + tl * bt) / (1.0 + sc.tl)
    else:
        xn = (u + tl * bt) * T(1.0 / (1.0 + sc.tl))
    xb = xn + th * ((x - xn) if mut == "theta" else (xn - x))
    for a in pn + [xn, xb]:
        assert a.dtype == np.dtype(T)
    return (np.stack(pn).astype(np.float64), xn.astype(np.float64), xb.astype(np.float64))


def _flags():
    return [(iso, huber, l1, has_p) for iso in (False, True) for huber in (False, True)
            for l1 in (False, True) for has_p in (True, False)]


def test_the_gate_is_sound_for_an_ieee_kernel():
    """Every case of the catalogue, emulated in np.float32 and judged as the GPU results
    are: inside the gate at every element / voxel.  In float64 the emulation -- a second
    writing of the arithmetic -- equals the restatement.  The worst ratios are printed."""
    worst = {}
    for dtype in BOTH:
        for cs in pc.catalogue(dtype):
            st, w = pc.state(cs.shape, dtype), pc.case_weights(cs)
            for iso, huber, l1, has_p in _flags():
                got = emulate(dtype, st, pc.RANDOM, w, huber, l1, iso, has_p)
                for name, bad, ratio in pc.judge(got, st, pc.RANDOM, w, dtype, huber, l1,
                                                 iso, has_p):
                    key = ("%s %s %s" % (name, "iso" if iso and name == "p_out" else
                                         ("l1" if l1 else "l2") if name != "p_out" else
                                         "aniso", "huber" if huber and name == "p_out"
                                         else "")).strip()
                    assert not np.any(bad), (cs.name, pc.suffix(dtype), key,
                                             pc.first_bad(bad, cs.shape))
                    if not pc.is64(dtype):
                        worst[key] = max(worst.get(key, 0.), ratio)
    for key in sorted(worst):
        print("emulation / gate, worst err / (R u S): %-24s %.3f" % (key, worst[key]))
    assert worst and max(worst.values()) <= 1.


@pytest.mark.parametrize("dtype", BOTH)
def test_the_tie_states_are_exact_in_the_emulation(dtype):
    """Dual ties: p_out equal to the restatement for the clamp and the projection; primal
    ties (l1, p_in NULL): p_out == 0, x and xbar equal."""
    for name in pc.TIE_CASES:
        cs = pc.case_named(name, dtype)
        w = pc.weights(cs.shape, True)
        seam = pc.seam_of(cs, dtype)
        st = pc.dual_tie_state(cs.shape, dtype, seam)
        nz = np.count_nonzero(st["p"], axis=0)
        assert nz.max() == 1 and int(np.prod(cs.shape)) >= pc.BRANCH_MIN_VOXELS
        for v in pc.tie_values(dtype):
            assert np.all(np.any(st["p"].reshape(len(cs.shape), -1) == v, axis=1)), v
        for iso in (False, True):
            got = emulate(dtype, st, pc.TIE, w, False, False, iso)
            (_, bad, _), = pc.judge(got, st, pc.TIE, w, dtype, False, False, iso, True,
                                    exact=True, which="p")
            assert not np.any(bad), (name, iso, pc.first_bad(bad, cs.shape))
        st = pc.primal_tie_state(cs.shape, dtype, seam)
        d = (st["x"] - st["bt"]).reshape(-1)
        assert np.any(d == pc.TIE.tl) and np.any(d == -pc.TIE.tl) and np.any(d == 0)
        assert np.any((d > pc.TIE.tl) & (d < pc.TIE.tl + 1e-6))
        for iso in (False, True):
            got = emulate(dtype, st, pc.TIE, w, False, True, iso, has_p=False)
            assert not got[0].any()
            for _, bad, _ in pc.judge(got, st, pc.TIE, w, dtype, False, True, iso, False,
                                      exact=True):
                assert not np.any(bad), (name, iso, pc.first_bad(bad, cs.shape))


# ================================================================= 3. the gate has teeth
@pytest.mark.parametrize("dtype", BOTH)
def test_the_gate_refuses_mutated_references(dtype):
    """Each fault, written into the emulation, must fall outside the gate (float64: differ)
    where the unmutated emulation passes."""
    cs = pc.case_named("rag16-3d-ry2", dtype)
    pl = pc.case_plan(cs, dtype, False)
    assert pl.form.ntx >= 2 and pl.form.nzc >= 2 and pl.TX < cs.shape[-1]
    st, w, sc = pc.state(cs.shape, dtype), pc.case_weights(cs), pc.RANDOM

    def failing(mut, l1=False, iso=False):
        got = emulate(dtype, st, sc, w, True, l1, iso, True, mut, pl.TX, pl.zchunk)
        return {name for name, bad, _ in
                pc.judge(got, st, sc, w, dtype, True, l1, iso, True) if np.any(bad)}

    for iso in (False, True):
        for l1 in (False, True):
            assert failing(None, l1, iso) == set()
        assert "p_out" in failing("wrap", iso=iso)
        # the stale halo value is a fault of the primal half: p_out itself is right
        assert failing("halo_x", iso=iso) == {"x", "xbar_out"}
        assert failing("pzprev", iso=iso) == {"x", "xbar_out"}
        assert failing("theta", iso=iso) == {"xbar_out"}
        assert failing("tau_for_tl", l1=True, iso=iso) == {"x", "xbar_out"}
    # the clamp's bound one float32 ulp up or down, on the dual tie state
    tie = pc.dual_tie_state(cs.shape, dtype, pl.TX)
    wu = pc.weights(cs.shape, True)
    for bound in (1., float(np.nextafter(np.float32(1), np.float32(2))),
                  float(np.nextafter(np.float32(1), np.float32(0)))):
        got = emulate(dtype, tie, pc.TIE, wu, False, False, False, bound=bound)
        (_, bad, _), = pc.judge(got, tie, pc.TIE, wu, dtype, False, False, False, True,
                                exact=True, which="p")
        assert bool(np.any(bad)) == (bound != 1.), bound


# ================================================================== 4. the branch shares
def test_between_a_tenth_and_nine_tenths_of_every_case_take_each_branch():
    lo, hi = {}, {}
    for dtype in BOTH:
        for cs in pc.catalogue(dtype):
            if int(np.prod(cs.shape)) < pc.BRANCH_MIN_VOXELS:
                continue
            for huber in (False, True):
                for k, f in pc.branch_shares(cs, dtype, huber).items():
                    if len(cs.shape) == 1 and k == "outside the ball":
                        assert f == pc.branch_shares(cs, dtype, huber)["clamped"]
                    assert 0.1 <= f <= 0.9, (cs.name, pc.suffix(dtype), huber, k, f)
                    lo[k], hi[k] = min(lo.get(k, 1.), f), max(hi.get(k, 0.), f)
    for k in sorted(lo):
        print("branch share %-28s %5.1f %% .. %5.1f %%" % (k, 100 * lo[k], 100 * hi[k]))


# ===================================================================== 5. the catalogue
def _wanted_forms(iso):
    forms = set()
    for kind in ("vec", "rag", "elem"):
        for LX in (64, 16):
            forms.add((kind, LX, 1, 1))
            for ndim in (2, 3):
                for RY in (1, 2) if kind == "rag" or iso else (1, 2, 4):
                    forms.add((kind, LX, RY, ndim))
    return forms


@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
@pytest.mark.parametrize("dtype", BOTH)
def test_the_catalogue_reaches_every_form_at_its_edges(dtype, iso):
    VW = pc.vw(dtype)
    cases = pc.catalogue(dtype)
    plans = {cs.name: pc.case_plan(cs, dtype, iso) for cs in cases}
    print("\n%-18s %-14s off ry rag zc  form (%s, %s)" % (
        "case", "shape", pc.suffix(dtype), "iso" if iso else "aniso"))
    for cs in cases:
        print("%-18s %-14s %3d %2d %3d %2d  %s" % (
            cs.name, "x".join(map(str, cs.shape)), cs.offset, cs.ry, cs.rag, cs.zchunk,
            tuple(plans[cs.name].form)))
    edged = set()
    for cs in cases:
        pl = plans[cs.name]
        f, (ndim, nz, ny, nx) = pl.form, pc.dims3(cs.shape)
        ok = f.ntx >= 2 and nx % pl.TX != 0
        if ndim >= 2:
            ok = ok and f.nty >= 2 and ny % pl.TY != 0
        if ndim >= 3:
            ok = ok and f.nzc >= 2 and nz % pl.zchunk != 0
        if ok:
            edged.add((f.kind, f.LX, f.RY, f.NDIM))
    # every form that exists, each with partial last tiles and a shorter last chunk
    assert _wanted_forms(iso) <= edged, sorted(_wanted_forms(iso) - edged)
    every = {(pl.form.kind, pl.form.LX, pl.form.RY, pl.form.NDIM) for pl in plans.values()}
    assert every == _wanted_forms(iso)               # ... and the mirror knows no other
    if iso:
        assert not any(f[2] == 4 for f in every)
    # the LX 64 element form is reached with pd_rag = 0 only
    assert all(cs.rag == 0 for cs in cases
               if plans[cs.name].form[:2] == ("elem", 64))
    d3 = [cs for cs in cases if len(cs.shape) == 3]
    assert any(cs.zchunk == 1 and cs.shape[0] > 2 for cs in d3)
    assert any(plans[cs.name].form.nzc == 1 and cs.shape[0] > 2 for cs in d3)
    assert any(cs.shape[0] == 1 for cs in d3)
    # ragged rows: every count of valid elements in the last vector, and 64 vectors exactly
    rag = [cs for cs in cases if plans[cs.name].form.kind == "rag"]
    for LX in (64, 16):
        valid = {cs.shape[-1] % VW for cs in rag if plans[cs.name].form.LX == LX}
        assert set(range(1, VW)) <= valid, (LX, valid)
    assert any(-(-cs.shape[-1] // VW) == 64 and plans[cs.name].form.LX == 64 for cs in rag)
    for axis in range(3):                            # extents of 1 on every axis
        assert any(pc.dims3(cs.shape)[1 + axis] == 1 and len(cs.shape) == 3 for cs in cases)
    assert any(cs.shape == (1,) for cs in cases)
    # the slab map, with blocks that have no tile
    slabbed = [plans[cs.name].form for cs in cases if plans[cs.name].form.slab]
    assert slabbed and all(f.nty >= 16 for f in slabbed)
    assert any(pc.blocks(f)[0] > pc.blocks(f)[1] for f in slabbed)
    assert {cs.offset for cs in cases} == {0, 1, 3}
    assert {cs.ry for cs in cases} == {0, 1, 2, 4}
    assert {cs.rag for cs in cases} == {0, 1}
    assert any(cs.unit and len(cs.shape) == d for d in (1, 2, 3) for cs in cases)
    for d in (1, 2, 3):
        assert any(cs.unit and len(cs.shape) == d for cs in cases)
    assert all(int(np.prod(cs.shape)) <= pc.MAX_VOXELS for cs in cases)


def test_the_mirror_on_shapes_worked_out_by_hand():
    """pd_launch and pd_plan_grid followed by hand (nsol_pd_launch.hpp)."""
    F = pc.Form
    # 260 / 4 = 65 vectors >= 64: LX 64, TX 256; TY = 4: 17 tile rows, slab = ceil(17 / 8)
    assert pc.form((3, 67, 260), np.float32, ry=1) == F("vec", 64, 1, 3, 2, 17, 2, 3)
    assert pc.blocks(pc.form((3, 67, 260), np.float32, ry=1)) == (96, 68)
    # off alignment: ragged; pd_ry = 4 has no ragged form and falls to 2
    assert pc.form((3, 67, 260), np.float32, offset=1, ry=4) == \
        F("rag", 64, 2, 3, 2, 9, 2, 0)
    assert pc.form((3, 67, 260), np.float32, offset=1, rag=0) == \
        F("elem", 64, 1, 3, 5, 17, 2, 3)
    # float64: two elements per vector, offset 2 is aligned again
    assert pc.form((5, 9, 34), np.float64, offset=2, zchunk=1) == \
        F("vec", 16, 1, 3, 2, 1, 5, 0)
    assert pc.form((7,), np.float32) == F("elem", 16, 1, 1, 1, 1, 1, 0)
    assert pc.form((8,), np.float32, offset=3) == F("rag", 16, 1, 1, 1, 1, 1, 0)
    # the isotropic launcher takes pd_ry = 4 as `choose`
    assert pc.form((3, 19, 260), np.float32, ry=4, iso=True).RY == 1
    assert pc.form((3, 19, 260), np.float32, ry=4).RY == 4
    assert pc.form((511, 1, 17), np.float32, rag=0).RY == 2
