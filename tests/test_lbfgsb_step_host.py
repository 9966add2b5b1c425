"""What lbfgsb_step_cases.py claims, proved on the CPU:

  * every lattice case of the tables is exact: all terms lie on a dyadic grid fine enough
    that their magnitudes sum below 2^24 (float32) / 2^53 (the float64 reductions) grid
    steps, so any order of additions, with or without FMA, gives the same value; and the
    evaluation in float32 in the kernel's own order equals the float64 reference element
    for element, the sums equal math.fsum;
  * of the free variables at least a quarter end strictly inside the box, a tenth at each
    bound, and one at each bound exactly without being clipped;
  * the references agree with NumpyBackend (tests/lbfgsb_numpy_backend.py), and the
    projected-gradient rule with scipy's own: scipy.optimize exposes only setulb, so
    its projgr is observed through the pgtol stop at the starting point (its subsm cannot
    be called alone; test_host_logic.py holds NumpyBackend's iterates to scipy's);
  * every planted mistake (lbfgsb_step_cases.MISTAKES) changes the expected values at
    every (length, count, type) of the tables where the mistaken code would run at all
    (_applies names the exceptions), so the GPU module's equality gates would notice it.
"""
import math

import numpy as np
import pytest

import lbfgsb_step_cases as sc
from lbfgsb_numpy_backend import NumpyBackend

BOTH = [np.float32, np.float64]


# ---- the lattice -----------------------------------------------------------------------
def test_lattice_rows_coefficients_and_mask():
    n = 257 * 4 + 3
    L = sc.lattice(n)
    for a in [L.w(k) for k in range(sc.NW_ROWS)] + [L.xcp, L.x, L.g, L.r, L.y]:
        assert np.array_equal(a * 4, np.rint(a * 4)) and np.abs(a).max() <= 8.0
    assert L.x.min() > sc.LO and L.x.max() < sc.HI
    assert np.all((L.xcp[L.free] >= sc.LO) & (L.xcp[L.free] <= sc.HI))
    assert np.any(L.xcp[~L.free] > sc.HI) and L.xcp[1] == 8.0 and not L.free[1]
    assert set(np.unique(L.mask)) == {-128, -1, 0, 1, 2, 127}
    assert L.free[0] and L.mask[0] == 0          # where "< 0" and "<= 0" part
    assert 0.5 < L.free.mean() < 0.7
    for a, b in sc.fixed_runs(n):
        assert a % 16 == 0 and b - a == 16 and not L.free[a:b].any()
    assert len(sc.fixed_runs(n)) == 2
    for nw in set(sc.WCOMB_NW) | set(sc.STEP_NW) | {sc.BIG_NW}:
        for co in (sc.comb_coefs(nw),) + sc.step_coefs(nw) + (sc.box_coefs(nw, 1),):
            co = np.array(co)
            assert co.size == nw
            assert np.array_equal(co * 8, np.rint(co * 8)) and np.all(np.abs(co) <= 1)
    for v in (sc.LO, sc.HI, sc.STEP_SCALE, sc.COMB_SCALE) + sc.RB3 + sc.BCOEF:
        assert float(np.float32(v)) == v


def _on_grid(a, q):
    return np.array_equal(a / q, np.rint(a / q))


def _wcomb_f32(base, bcoef, w, wcoef, scale, n, box=None):
    """k_wcomb's order in float32 arithmetic (NumPy rounds every operation, no FMA)."""
    f = np.float32
    acc = np.zeros(n, f)
    for c, v in list(zip(bcoef, base)) + list(zip(wcoef, w)):
        acc = acc + f(c) * v.astype(f)
    acc = acc * f(scale)
    if box is not None:
        acc = np.where(acc < f(box[0]), f(box[0]), acc)
        acc = np.where(acc > f(box[1]), f(box[1]), acc)
    assert acc.dtype == f
    return acc.astype(np.float64)


def _step_f32(w, wcoef, r, rcoef, xcp, x, g, free, n):
    f = np.float32
    if r is None:
        rv = np.zeros(n, f)
        for c, v in list(zip(sc.RB3, (xcp, x, g))) + list(zip(rcoef, w)):
            rv = rv + f(c) * v.astype(f)
        rv = np.where(free, rv, f(0))
    else:
        rv = r.astype(f)
    acc = np.zeros(n, f) + f(1) * rv
    for c, v in zip(wcoef, w):
        acc = acc + f(c) * v.astype(f)
    acc = acc * f(sc.STEP_SCALE)
    v = xcp.astype(f) + acc
    v = np.where(v < f(sc.LO), f(sc.LO), v)
    v = np.where(v > f(sc.HI), f(sc.HI), v)
    xn = np.where(free, v, xcp.astype(f))
    d = f(1) * xn + f(-1) * x.astype(f)
    assert xn.dtype == f and d.dtype == f
    return xn.astype(np.float64), d.astype(np.float64)


def _sum_is_exact_in_any_order(terms, q=2.0 ** -14):
    assert _on_grid(terms, q)
    assert np.abs(terms).sum() / q < 2.0 ** 53


def test_wcomb_and_clip_cases_are_exact_in_float32_in_any_order():
    q = 1.0 / 16                                  # scale 2 times c v in Z / 32
    for n, nbase, nw, masked, _ in sc.wcomb_cases(np.float32):
        L = sc.lattice(n)
        base, bco, w, wco = sc.wcomb_args(n, nbase, nw)
        mask = L.mask if masked else None
        out, S = sc.wcomb_ref(n, base, bco, w, wco, sc.COMB_SCALE, mask, np.float32)
        assert _on_grid(out, q) and (S.max() if n else 0) / (q / 2) < 2.0 ** 24
        emu = _wcomb_f32(base, bco, w, wco, sc.COMB_SCALE, n)
        emu = np.where(L.free, emu, 0.0) if masked else emu
        assert np.array_equal(emu, out), (n, nbase, nw)
        out64, _ = sc.wcomb_ref(n, base, bco, w, wco, sc.COMB_SCALE, mask, np.float64)
        assert np.array_equal(out64, out)
    for n, nw, _ in sc.clip_cases(np.float32):
        L = sc.lattice(n)
        w, wco = [L.w(k) for k in range(nw)], sc.box_coefs(nw, 1)
        out, S = sc.wcomb_ref(n, [], [], w, wco, 1.0, None, np.float32, box=(sc.LO, sc.HI))
        assert _on_grid(out, 1.0 / 32) and S.max() * 32 < 2.0 ** 24
        assert np.array_equal(_wcomb_f32([], [], w, wco, 1.0, n, (sc.LO, sc.HI)), out)


@pytest.mark.parametrize("rin", [False, True])
def test_step_cases_are_exact_in_float32_in_any_order(rin):
    q = 1.0 / 128
    for n, nw, cap in sc.step_cases(np.float32):
        L = sc.lattice(n)
        ref = sc.step_expected(n, nw, np.float32, rin, grid_cap=cap)
        # S bounds every partial sum of xn; d = xn - x adds |x| <= 8
        assert _on_grid(ref["xn"], q) and _on_grid(ref["d"], q)
        assert (ref["S"].max() + 8.0) / q < 2.0 ** 24
        w, wc, rc = sc.step_args(n, nw)
        xn, d = _step_f32(w, wc, None if rin else L.r, rc, L.xcp, L.x, L.g, L.free, n)
        assert np.array_equal(xn, ref["xn"]) and np.array_equal(d, ref["d"]), (n, nw)
        ref64 = sc.step_expected(n, nw, np.float64, rin, grid_cap=cap)
        for key in ("xn", "d", "wd"):
            assert np.array_equal(ref64[key], ref[key])
        assert (ref64["hits"], ref64["dd"], ref64["gd"]) == (ref["hits"], ref["dd"], ref["gd"])
        # (the ratio is a quotient rounded to T: one expected value per type)
        assert abs(ref64["nratio"] - ref["nratio"]) <= 2.0 ** -23 * abs(ref64["nratio"])
        d = ref["d"]
        for terms in [d * d, d * L.g] + [wk * d for wk in w]:
            _sum_is_exact_in_any_order(terms)
        if n < sc.FSUM_BELOW:
            assert float(np.sum(d * w[0])) == math.fsum((d * w[0]).tolist())
            assert float(np.sum(d * d)) == ref["dd"]


def test_the_other_sums_are_exact_in_any_order():
    for n, _ in sc.plain_cases(np.float32):
        L = sc.lattice(n)
        for terms in (L.w(0) * L.y, (L.xcp - L.x) ** 2, (L.xcp - L.x) * L.g):
            _sum_is_exact_in_any_order(terms, 1.0 / 16)
        out, _, _ = sc.diff_dots_ref(L.xcp, L.x, L.g, np.float32)
        assert np.array_equal(out, L.xcp - L.x)


# ---- the shares ------------------------------------------------------------------------
def _hold_shares(sh, label):
    assert sh["inside"] >= 0.25, (label, sh)
    assert sh["at_lo"] >= 0.10 and sh["at_hi"] >= 0.10, (label, sh)
    assert sh["unclipped"] >= 1, (label, sh)


@pytest.mark.parametrize("rin", [False, True])
def test_step_cases_end_inside_and_at_both_bounds(rin):
    worst = {"inside": 1.0, "at_lo": 1.0, "at_hi": 1.0}
    for n, nw, cap in sc.step_cases(np.float32):
        if n < 1000:
            continue
        L = sc.lattice(n)
        ref = sc.step_expected(n, nw, np.float32, rin)
        sh = sc.shares(ref, L.xcp)
        _hold_shares(sh, (n, nw, rin))
        pre = L.xcp + ref["dsub"]
        assert L.free[sc.P_HI] and pre[sc.P_HI] == sc.HI and ref["xn"][sc.P_HI] == sc.HI
        assert L.free[sc.P_LO] and pre[sc.P_LO] == sc.LO and ref["xn"][sc.P_LO] == sc.LO
        worst = {k: min(worst[k], sh[k]) for k in worst}
    print("subspace step, r %s: smallest shares %r" % ("formed" if rin else "read", worst))


def test_clip_cases_end_inside_and_at_both_bounds():
    for n, nw, _ in sc.clip_cases(np.float32):
        if n < 1000:
            continue
        L = sc.lattice(n)
        w, wco = [L.w(k) for k in range(nw)], sc.box_coefs(nw, 1)
        out, _ = sc.wcomb_ref(n, [], [], w, wco, 1.0, None, np.float32, box=(sc.LO, sc.HI))
        pre, _ = sc.wcomb_ref(n, [], [], w, wco, 1.0, None, np.float32)
        sh = {"inside": np.mean((out > sc.LO) & (out < sc.HI)), "at_lo": np.mean(out == sc.LO),
              "at_hi": np.mean(out == sc.HI),
              "unclipped": int(((pre == sc.LO) | (pre == sc.HI)).sum())}
        _hold_shares(sh, (n, nw))


# ---- the references against NumpyBackend and scipy ---------------------------------------
def test_references_agree_with_the_numpy_backend():
    nb = NumpyBackend()
    for n in (7, 1031):
        L = sc.lattice(n)
        c = 5
        wy, ws = [L.w(k) for k in range(c)], [L.w(k) for k in range(c, 2 * c)]
        w = wy + ws
        wc, rc = sc.step_coefs(2 * c)
        theta = 4.0
        # reduced_gradient: wcomb with the bases (z, x, g)
        r = nb.reduced_gradient(L.xcp, L.x, L.g, theta, ws, wy, rc[c:], rc[:c], L.mask)
        got, _ = sc.wcomb_ref(n, [L.xcp, L.x, L.g], [-theta, theta, -1.0], w, rc, 1.0, L.mask,
                              np.float64)
        assert np.array_equal(got, r)
        dsub = nb.subspace_direction(r, ws, wy, wc[:c], wc[c:], theta, L.mask)
        got, _ = sc.wcomb_ref(n, [r], [1.0], w, wc, 1.0 / theta, L.mask, np.float64)
        assert np.array_equal(got, dsub)
        xn, hit = nb.project_step(L.xcp, dsub, sc.LO, sc.HI, L.mask)
        ref = sc.step_ref(w, wc, r, rc, L.xcp, L.x, L.g, L.mask, 1.0 / theta, sc.LO, sc.HI,
                          np.float64)
        assert np.array_equal(ref["xn"], xn) and (ref["hits"] > 0) == hit
        rin = sc.step_ref(w, wc, None, rc, L.xcp, L.x, L.g, L.mask, 1.0 / theta, sc.LO, sc.HI,
                          np.float64)
        # RB3 is (-theta, theta, -1) / ... only for theta = 1/2: compare at that theta
        r2 = nb.reduced_gradient(L.xcp, L.x, L.g, 0.5, ws, wy, rc[c:], rc[:c], L.mask)
        ref2 = sc.step_ref(w, wc, r2, rc, L.xcp, L.x, L.g, L.mask, 1.0 / theta, sc.LO, sc.HI,
                           np.float64)
        assert np.array_equal(rin["xn"], ref2["xn"]) and np.array_equal(rin["d"], ref2["d"])
        d, dd, gd = nb.diff_dots(xn, L.x, L.g)
        assert np.array_equal(ref["d"], d)
        assert ref["dd"] == dd and ref["gd"] == gd
        assert np.array_equal(ref["wd"], nb.dots(w, d))
        assert -ref["nratio"] == nb.max_step(L.x, d, sc.LO, sc.HI, 1e10)
        out, res, _ = sc.diff_dots_ref(L.xcp, L.x, L.g, np.float64)
        d2, dd2, gd2 = nb.diff_dots(L.xcp, L.x, L.g)
        assert np.array_equal(out, d2) and res == [dd2, gd2]
        row, _ = sc.mdots_ref(w, L.y, L.mask, np.float64)
        assert np.array_equal(row, nb.dots(w, L.y, L.mask))
        assert sc.mdot_ref(w[0], L.y, None, np.float64)[0] == nb.dot(w[0], L.y)
        assert sc.count_free_ref(L.mask) == nb.count_free(L.mask)
        x, g = sc.projgr_inputs(n)
        for lo, hi in ((sc.LO, sc.HI), (-np.inf, sc.HI), (sc.LO, np.inf), (-np.inf, np.inf)):
            assert sc.projgr_ref(x, g, lo, hi, np.float64) == nb.projgr(x, g, lo, hi)


def test_projgr_reference_is_scipys_rule():
    """scipy's L-BFGS-B stops at the starting point exactly when ITS projected-gradient
    norm is <= pgtol: just above the reference's value it does, just below it does not."""
    optimize = pytest.importorskip("scipy.optimize")
    n = 61
    x0, g0 = sc.projgr_inputs(n)
    x0 = np.clip(x0, sc.LO, sc.HI)               # scipy projects the starting point itself
    want = sc.projgr_ref(x0, g0, sc.LO, sc.HI, np.float64)
    assert want > 0
    centre = x0 - g0                             # gradient of 0.5 |x - centre|^2 at x0: g0

    def fun(x):
        return 0.5 * float(np.dot(x - centre, x - centre)), x - centre
    for gtol, stops in ((want * (1 + 1e-9), True), (want * (1 - 1e-9), False)):
        res = optimize.minimize(fun, x0, jac=True, method="L-BFGS-B",
                                bounds=[(sc.LO, sc.HI)] * n,
                                options={"gtol": gtol, "ftol": 0.0, "maxiter": 3})
        assert (res.nit == 0) == stops, (gtol, res.nit, res.message)


# ---- the planted mistakes ------------------------------------------------------------------
def _differs(a, b):
    if isinstance(a, np.ndarray):
        return not np.array_equal(a, b)
    return a != b


def _step_differs(good, bad):
    keys = ("xn", "d", "hits", "dd", "gd", "wd", "nratio")
    return [k for k in keys if _differs(good[k], bad[k])]


def _wcomb_applies(mistake, n, nbase, nw, masked, dtype):
    width = sc.vw(dtype)
    if mistake in ("coef_index", "swap_halves"):
        return nw >= 2
    if mistake == "drop_fourth":
        return nw >= 4
    if mistake == "scale_first":
        return nbase >= 1
    if mistake == "mask_lt":
        return masked and nbase + nw >= 1
    if mistake == "fixed_not_zeroed":
        # the vector form alone skips; a wholly fixed vector needs the runs of 16 (or the
        # pair 1 / 127 ... of one float64 vector)
        free = sc.lattice(n).free
        return masked and nbase + nw >= 1 and bool(sc._whole_fixed(free, width).any())
    if mistake == "tail_skipped":
        return True
    return False


@pytest.mark.parametrize("dtype", BOTH)
def test_planted_mistakes_change_wcomb_and_lincomb_clip(dtype):
    seen = set()
    for n, nbase, nw, masked, _ in sc.wcomb_cases(dtype):
        L = sc.lattice(n)
        base, bco, w, wco = sc.wcomb_args(n, nbase, nw)
        mask = L.mask if masked else None
        good, _ = sc.wcomb_ref(n, base, bco, w, wco, sc.COMB_SCALE, mask, dtype)
        for m in sc.MISTAKES:
            if not _wcomb_applies(m, n, nbase, nw, masked, dtype):
                continue
            bad, _ = sc.wcomb_ref(n, base, bco, w, wco, sc.COMB_SCALE, mask, dtype, mistake=m)
            assert not np.array_equal(good, bad), (m, n, nbase, nw, masked)
            seen.add(m)
    assert seen == {"coef_index", "drop_fourth", "swap_halves", "scale_first", "mask_lt",
                    "fixed_not_zeroed", "tail_skipped"}
    for n, nw, _ in sc.clip_cases(dtype):
        L = sc.lattice(n)
        w, wco = [L.w(k) for k in range(nw)], sc.box_coefs(nw, 1)
        good, _ = sc.wcomb_ref(n, [], [], w, wco, 1.0, None, dtype, box=(sc.LO, sc.HI))
        for m in ("coef_index", "drop_fourth", "swap_halves", "clip_swapped", "tail_skipped"):
            if not (m in ("clip_swapped", "tail_skipped") or
                    _wcomb_applies(m, n, 0, nw, False, dtype)):
                continue
            bad, _ = sc.wcomb_ref(n, [], [], w, wco, 1.0, None, dtype, box=(sc.LO, sc.HI),
                                  mistake=m)
            assert not np.array_equal(good, bad), (m, n, nw)


STEP_MISTAKES = ("coef_index", "drop_fourth", "swap_halves", "scale_first", "mask_lt",
                 "clip_swapped", "d_from_xcp", "ratio_free_only", "ratio_other_slot",
                 "tail_skipped")


@pytest.mark.parametrize("rin", [False, True])
@pytest.mark.parametrize("dtype", BOTH)
def test_planted_mistakes_change_the_subspace_step(dtype, rin):
    """Every mistake changes xn, d or the result row at every case the kernel takes; the
    two about the ratio change result[nw + 3] itself."""
    ran = 0
    for n, nw, cap in sc.step_cases(dtype):
        if not sc.vector_form(n, dtype):
            continue                               # declined: nothing runs
        good = sc.step_expected(n, nw, dtype, rin, grid_cap=cap)
        for m in STEP_MISTAKES:
            if m in ("coef_index", "swap_halves") and nw < 2:
                continue
            if m == "drop_fourth" and nw < 4:
                continue
            if m == "ratio_free_only" and n < 2:
                continue
            bad = sc.step_expected(n, nw, dtype, rin, mistake=m, grid_cap=cap)
            diff = _step_differs(good, bad)
            assert diff, (m, n, nw)
            if m.startswith("ratio_"):
                assert diff == ["nratio"], (m, n, nw, diff)
            ran += 1
    assert ran > 250


@pytest.mark.parametrize("dtype", BOTH)
def test_planted_mistakes_change_the_sums(dtype):
    for n, nvec, cap in sc.mdots_cases(dtype):
        L = sc.lattice(n)
        vecs = [L.w(k) for k in range(nvec)]
        good, _ = sc.mdots_ref(vecs, L.y, L.mask, dtype)
        assert np.all(good != sc.RES_FILL)
        for m in ("mask_lt", "tail_skipped", "second_launch"):
            if m == "second_launch" and nvec <= sc.DOTS_PER_LAUNCH:
                continue
            bad, _ = sc.mdots_ref(vecs, L.y, L.mask, dtype, mistake=m)
            assert not np.array_equal(good, bad), (m, n, nvec)
    for n, cap in sc.plain_cases(dtype):
        L = sc.lattice(n)
        for m in ("mask_lt", "tail_skipped"):
            assert sc.mdot_ref(L.w(0), L.y, L.mask, dtype)[0] != \
                sc.mdot_ref(L.w(0), L.y, L.mask, dtype, mistake=m)[0], (m, n)
        good = sc.diff_dots_ref(L.xcp, L.x, L.g, dtype)
        bad = sc.diff_dots_ref(L.xcp, L.x, L.g, dtype, mistake="tail_skipped")
        assert good[1][0] != bad[1][0] and good[1][1] != bad[1][1], n
        x, g = sc.projgr_inputs(n)
        assert sc.projgr_ref(x, g, sc.LO, sc.HI, dtype) == 7.5
        assert sc.projgr_ref(x, g, sc.LO, sc.HI, dtype, mistake="tail_skipped") < 7.5, n
    for n, cap in sc.plain_cases(dtype, 16):
        mask = sc.lattice_mask(n)
        for m in ("mask_lt", "tail_skipped"):
            if m == "tail_skipped" and n % 16 == 0 and not (mask[n - 16:] <= 0).any():
                continue
            if m == "tail_skipped" and n % 16 and mask[n - 1] > 0:
                continue
            assert sc.count_free_ref(mask) != sc.count_free_ref(mask, mistake=m), (m, n)


def test_projgr_plants_reach_every_branch():
    x, g = sc.projgr_inputs(1031)
    lo, hi = sc.LO, sc.HI
    for gsel in (g < 0, (g == 0) & ~np.signbit(g), (g == 0) & np.signbit(g), g > 0):
        for xsel in (x < lo, x == lo, (x > lo) & (x < hi), x == hi, x > hi):
            assert np.any(gsel[:24] & xsel[:24]) and np.any(gsel[-26:] & xsel[-26:])
    vals = [sc.projgr_ref(x, g, a, b, np.float32) for a in (lo, -np.inf) for b in (hi, np.inf)]
    assert vals == [7.5, 7.75, 8.0, 8.0]
