"""The WGT and LIN forms of the two tile bodies -- k_pd_w / k_pd_w_iso (csrc/nsol_pdw.hip),
k_pd_lin / k_pd_lin_iso (nsol_pdl.hip), k_pdl_stack / k_pdl_stack_iso (nsol_pdls.hip) -- and
the element-wise kernels beside them (k_prox_w, k_pdl_dual_data, k_pdl_dual_data_stack), ONE
call at a time through the C ABI, per voxel against the float64 restatement of
nsol_amd/vector_numpy.py (anchored by test_pd_weighted_linear_host.py): bit for bit in
float64, inside the gates derived in pd_step_cases.py in float32.

The launchers of these kernels take no knobs, so the shapes of pd_step_cases.catalogue_stack
(and the members of its stacks) choose the form; the host test asserts that they reach every
one.  All arrays live in a guard-band arena (device_arena.py), outputs hold a sentinel
before a call, inputs are compared with what they held, and each array in turn ends where
the allocation ends.
"""
import numpy as np
import pytest

import pd_step_cases as pc
import test_pd_steps_gpu as steps
from device_arena import Arena
from nsol_amd import vector_numpy as vn
from test_pd_weighted_linear_host import DD_LENGTHS, elementwise_inputs

pytestmark = pytest.mark.gpu

BOTH = pc.BOTH
FILL = steps.FILL
NAMES = [cs.name for cs in pc.catalogue_stack(np.float32)]
assert NAMES == [cs.name for cs in pc.catalogue_stack(np.float64)]
STACKS = [cs.name for cs in pc.catalogue_stack(np.float32) if cs.members > 1]
LIN_ARRAYS = ("xbar_in", "xbar_out", "x", "g", "p_in", "p_out")
WGT_ARRAYS = ("xbar_in", "xbar_out", "x", "bt", "wt", "p_in", "p_out")
_fn, _sync, _stream = steps._fn, steps._sync, steps._stream


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    before = set(steps.WORST)
    yield nsol_amd
    for key in sorted(set(steps.WORST) - before):
        print("GPU float32, worst err / (R u S): %-34s %.3f" % (key, steps.WORST[key]))


def _reg_flags(huber, iso):
    from nsol_amd import ops
    return (ops.PD_REG_HUBER if huber else 0) | (ops.PD_REG_ISOTROPIC if iso else 0)


def _wgt_flags(huber, l1, iso):
    from nsol_amd import ops
    return _reg_flags(huber, iso) | ops.PD_DATA_WEIGHTED | (ops.PD_DATA_L1 if l1 else 0)


def _member_scalars(m):
    """The weighted stack's members differ in lmbda, so every row of the table differs."""
    lmbda = pc.LMBDA * (1. + 0.25 * (m % 3))
    return lmbda, pc.Scalars(pc.SIGMA, pc.HDEN, pc.TAU, pc.TAU * lmbda, pc.THETA)


class Run(object):
    """One case on one kernel family with the states of its members (a single volume: one)."""

    def __init__(self, cs, dtype, iso, sts, scs=None, unit=None, lmbdas=None):
        M = len(sts)
        self.cs, self.dtype, self.iso, self.M, self.sts = cs, dtype, iso, M, sts
        self.w = pc.weights(cs.shape, cs.unit if unit is None else unit)
        self.scs = scs or [pc.RANDOM] * M
        self.lmbdas = lmbdas or [pc.LMBDA] * M
        self.plan = pc.scase_plan(cs, dtype, M)
        self.shape, self.d, self.dims = cs.shape, len(cs.shape), pc.dims3(cs.shape)
        self.n = int(np.prod(cs.shape))
        self.cx = [steps._Ctx("%s member %d of %d" % (cs.name, m, M), cs.shape, dtype, iso,
                              self.plan, sts[m], self.scs[m], self.w, cs.offset)
                   for m in range(M)]

    def cat(self, k):
        return np.stack([st[k] for st in self.sts])

    def fills(self):
        return np.full((self.M,) + self.shape, FILL), np.full((self.M, self.d) + self.shape, FILL)

    def outputs(self, ar, what, inputs):
        """The guards and the inputs after the call (bt may hold NaN), then (p, x, xbar)."""
        _sync()
        assert ar.guards_intact(), self.cx[0].label(what) + ": a guard band was written"
        for k, v in inputs.items():
            assert np.array_equal(ar.get(k, v.shape), v, equal_nan=True), \
                self.cx[0].label(what) + ": %s (an input) was written" % k
        shape, pshape = (self.M,) + self.shape, (self.M, self.d) + self.shape
        return ar.get("p_out", pshape), ar.get("x", shape), ar.get("xbar_out", shape)

    # ------------------------------------------------------------------- the calls
    def lin(self, box, huber, has_p, last=None, stacked=None):
        stacked = self.M > 1 if stacked is None else stacked
        fill, pfill = self.fills()
        inputs = dict(xbar_in=self.cat("xbar"), g=self.cat("g"), p_in=self.cat("p"))
        ar = Arena(dict(inputs, xbar_out=fill, x=self.cat("x"), p_out=pfill), self.dtype,
                   self.cs.offset, last)
        sc = self.scs[0]
        ptrs = [ar.ptr(k) for k in ("xbar_in", "xbar_out", "x", "g", "p_in", "p_out")]
        tail = (*self.dims, *self.w, sc.sigma, sc.hden if huber else 1.0, sc.tau, sc.theta,
                box[0], box[1], _reg_flags(huber, self.iso), int(has_p), _stream())
        if stacked:
            rc = _fn("pdl_stack_iter", self.dtype)(*ptrs, self.M, *tail)
        else:
            assert self.M == 1
            rc = _fn("pdl_iter", self.dtype)(*ptrs, *tail)
        what = "%s box=%r huber=%d has_p=%d last=%s" % (
            "pdl_stack_iter" if stacked else "pdl_iter", box, huber, has_p, last)
        assert rc == 0, self.cx[0].label(what)
        return self.outputs(ar, what, inputs), what

    def weighted(self, huber, l1, has_p, last=None, strides="nn", wt=None, bt=None):
        """strides: a letter each for bt and wt, "0" (the stack shares member 0's) or "n"."""
        from nsol_amd import ops
        fill, pfill = self.fills()
        share = lambda a, s: a[:1] if s == "0" else a
        inputs = dict(xbar_in=self.cat("xbar"), p_in=self.cat("p"),
                      bt=share(self.cat("bt") if bt is None else bt, strides[0]),
                      wt=share(self.cat("wt") if wt is None else wt, strides[1]))
        ar = Arena(dict(inputs, xbar_out=fill, x=self.cat("x"), p_out=pfill), self.dtype,
                   self.cs.offset, last)
        flags = _wgt_flags(huber, l1, self.iso)
        col = lambda k: [[getattr(sc, k)] for sc in self.scs]
        tab = ops.pd_weighted_table(ar.buf, self.M, self.lmbdas, col("sigma"), col("tau"),
                                    col("theta"), not has_p, pc.HUBER_GAMMA, flags)
        stride = lambda s: 0 if s == "0" else self.n
        rc = _fn("pd_weighted_iter", self.dtype)(
            ar.ptr("xbar_in"), ar.ptr("xbar_out"), ar.ptr("x"), ar.ptr("bt"),
            stride(strides[0]), ar.ptr("wt"), stride(strides[1]), ar.ptr("p_in"),
            ar.ptr("p_out"), self.M, *self.dims, *self.w, tab.data_ptr(), 0, flags, _stream())
        what = "pd_weighted_iter huber=%d l1=%d has_p=%d strides=%s last=%s" % (
            huber, l1, has_p, strides, last)
        assert rc == 0, self.cx[0].label(what)
        return self.outputs(ar, what, inputs), what

    # ------------------------------------------------------------------ the verdicts
    def judge_lin(self, got, what, box, huber, has_p, exact=False, members=None):
        for m in range(self.M) if members is None else members:
            cx, st = self.cx[m], self.sts[m]
            cx.judge(tuple(a[m] for a in got), what,
                     "k_pd_lin_iso" if self.iso else "k_pd_lin", huber, False, has_p, "pxb",
                     exact, lambda p: pc.lin_expected(p, st, cx.sc, self.w, self.dtype, box))
            if pc.box_holds_a_number(box, self.dtype):
                inside = (got[1][m] >= box[0]) & (got[1][m] <= box[1])
                assert np.all(inside), cx.label(what) + ": x leaves the caller's box at %s" % \
                    pc.first_bad(~inside, self.shape)

    def judge_weighted(self, got, what, huber, l1, has_p, exact=False, members=None,
                       sts=None):
        for m in range(self.M) if members is None else members:
            cx, st = self.cx[m], (sts or self.sts)[m]
            cx.judge(tuple(a[m] for a in got), what,
                     "k_pd_w%s %s" % ("_iso" if self.iso else "", "l1" if l1 else "l2"),
                     huber, False, has_p, "pxb", exact,
                     lambda p: pc.weighted_expected(p, st, cx.sc, self.w, self.dtype, l1))

    def same(self, got, want, what, m=0, k=0):
        """Member m of got against member k of want, bit for bit."""
        for a in range(self.d):
            self.cx[m].same(got[0][m][a], want[0][k][a], what, "p_out")
        self.cx[m].same(got[1][m], want[1][k], what, "x")
        self.cx[m].same(got[2][m], want[2][k], what, "xbar_out")


def _combos():
    return [(iso, huber, has_p) for iso in (False, True) for huber in (False, True)
            for has_p in (True, False)]


# ============================================================================ single entries
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_the_linear_iteration_per_voxel_in_every_form(nsol, name, dtype):
    """nsol_pdl_iter_* on the case's volume (of a stack: its member 0): {TV, Huber} x
    {anisotropic, isotropic} x {has_p 1, 0} on the box BOX -- the tie cases also on the
    one-sided and the infinite boxes --, p_out against pd_dual_step, x and xbar_out against
    pd_lin_primal_step of the call's own p_out, x inside the caller's box in double; then
    each array in turn at the end of the allocation."""
    cs = pc.scase_named(name, dtype)
    st = pc.lin_state(cs.shape, dtype)
    kept = {}
    for iso, huber, has_p in _combos():
        run = Run(cs, dtype, iso, [st])
        boxes = pc.BOXES if name in pc.STACK_TIE_CASES and huber == has_p else pc.BOXES[:1]
        for box in boxes:
            got, what = run.lin(box, huber, has_p)
            run.judge_lin(got, what, box, huber, has_p)
            if box is pc.BOX:
                kept[(iso, huber, has_p)] = got
    keys = sorted(kept)
    for k, last in enumerate(LIN_ARRAYS):
        iso, huber, has_p = keys[(3 * k + 1) % len(keys)]
        run = Run(cs, dtype, iso, [st])
        got, what = run.lin(pc.BOX, huber, has_p, last=last)
        run.same(got, kept[(iso, huber, has_p)], what)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_the_weighted_iteration_per_voxel_in_every_form(nsol, name, dtype):
    """nsol_pd_weighted_iter_* with one member: {TV, Huber} x {l2, l1} x {anisotropic,
    isotropic} x {p_is_zero}: judged as the linear one against pd_weighted_primal_step -- so
    no NaN or inf leaves a zero-weight voxel and its neighbours carry the restatement's
    values --; unit weights in float64 give nsol_pd_fused_iter_f64's bits; then each array
    in turn at the end of the allocation."""
    cs = pc.scase_named(name, dtype)
    st = pc.weights_state(cs.shape, dtype)
    kept = {}
    for iso, huber, has_p in _combos():
        run = Run(cs, dtype, iso, [st], [pc.WEIGHTED])
        for l1 in (False, True):
            got, what = run.weighted(huber, l1, has_p)
            run.judge_weighted(got, what, huber, l1, has_p)
            kept[(iso, huber, has_p, l1)] = got
    keys = sorted(kept)
    for k, last in enumerate(WGT_ARRAYS):
        iso, huber, has_p, l1 = keys[(5 * k + 2) % len(keys)]
        run = Run(cs, dtype, iso, [st], [pc.WEIGHTED])
        got, what = run.weighted(huber, l1, has_p, last=last)
        run.same(got, kept[(iso, huber, has_p, l1)], what)
    if pc.is64(dtype):
        plain = pc.member_state(cs.shape, dtype)
        ones = np.ones((1,) + cs.shape)
        for iso, huber, has_p in _combos()[::3]:
            run = Run(cs, dtype, iso, [plain], [pc.WEIGHTED])
            for l1 in (False, True):
                got, what = run.weighted(huber, l1, has_p, wt=ones)
                fused, _ = run.cx[0].fused(huber, l1, has_p)
                run.same(got, tuple(a[None] for a in fused), what + " against pd_fused_iter")


# ==================================================================================== stacks
def _stack_states(cs, dtype, M, form):
    state_of = pc.lin_state if form == "lin" else pc.weights_state
    return [state_of(cs.shape, dtype, m) for m in range(M)]


def _check_members_against_single(run, got, members, call):
    """Member m of the stack's outputs against the single entry on member m's arrays."""
    for m in members:
        one = Run(run.cs, run.dtype, run.iso, [run.sts[m]], [run.scs[m]],
                  lmbdas=[run.lmbdas[m]])
        alone, what = call(one, m)
        run.same(got, alone, what + " (member %d of the stack against the single entry)" % m,
                 m, 0)


@pytest.mark.parametrize("name", STACKS)
@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_the_stacks_of_the_catalogue_member_by_member(nsol, name, dtype):
    """The stacks whose member count chooses the form -- two rows per lane in 2-D, and the
    pairs where the stack takes two rows per lane and its member alone one --: every member
    of nsol_pdl_stack_iter_* and of nsol_pd_weighted_iter_* (own bt and wt, and a table
    row of its own), anisotropic and isotropic, against the restatement, and the first, a
    middle and the last member (all of them up to 8) bit for bit against the single entry on
    that member's arrays."""
    cs = pc.scase_named(name, dtype)
    M, k = cs.members, NAMES.index(name)
    picked = range(M) if M <= 8 else (0, M // 2, M - 1)
    ms = [_member_scalars(m) for m in range(M)]
    for iso in (False, True):
        k += iso
        huber, has_p, l1 = bool(k & 1), not k & 2, bool(k & 4) != bool(k & 1)
        run = Run(cs, dtype, iso, _stack_states(cs, dtype, M, "lin"))
        got, what = run.lin(pc.BOX, huber, has_p)
        run.judge_lin(got, what, pc.BOX, huber, has_p)
        _check_members_against_single(
            run, got, picked, lambda one, m: one.lin(pc.BOX, huber, has_p, stacked=False))
        run = Run(cs, dtype, iso, _stack_states(cs, dtype, M, "wgt"), [sc for _, sc in ms],
                  lmbdas=[lm for lm, _ in ms])
        got, what = run.weighted(huber, l1, has_p)
        run.judge_weighted(got, what, huber, l1, has_p)
        _check_members_against_single(run, got, picked,
                                      lambda one, m: one.weighted(huber, l1, has_p))


@pytest.mark.parametrize("M", [3, 8])
@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_stacks_of_3_and_8_members_are_their_members_runs(nsol, M, dtype):
    """On the tie cases' shapes and the form-switching pair: nsol_pdl_stack_iter_* and
    nsol_pd_weighted_iter_* with bt and wt at member strides 0 and n in all four
    combinations, member states and table rows that differ: every member's three outputs are
    the single entry's bits on that member's arrays -- so the forward difference at a
    member's last voxel and the backward one at its first see zeros, not the neighbouring
    member -- and lie inside the gates."""
    names = pc.STACK_TIE_CASES + (("switch-3d-alone",) if M == 8 else ("small-3d", "ones"))
    for k, name in enumerate(names):
        cs = pc.scase_named(name, dtype)
        for iso in (False, True):
            huber, has_p, l1 = bool((k + iso) & 1), not (k + M) & 2, bool((k + M + iso) & 1)
            run = Run(cs, dtype, iso, _stack_states(cs, dtype, M, "lin"))
            if name == "switch-3d-alone":
                assert run.plan.form.RY == 2 and pc.scase_plan(cs, dtype, 1).form.RY == 1
            got, what = run.lin(pc.BOX, huber, has_p)
            run.judge_lin(got, what, pc.BOX, huber, has_p)
            _check_members_against_single(
                run, got, range(M), lambda one, m: one.lin(pc.BOX, huber, has_p, stacked=False))
            ms = [_member_scalars(m) for m in range(M)]
            for strides in ("nn", "00", "0n", "n0"):
                # garbage under a zero weight needs bt and wt of the same member
                form = "wgt" if strides[0] == strides[1] else "plain"
                sts = [dict(pc.weights_state(cs.shape, dtype, m),
                            bt=(pc.weights_state if form == "wgt" else pc.member_state)(
                                cs.shape, dtype, m)["bt"]) for m in range(M)]
                seen = [dict(st, bt=sts[0 if strides[0] == "0" else m]["bt"],
                             wt=sts[0 if strides[1] == "0" else m]["wt"])
                        for m, st in enumerate(sts)]
                run = Run(cs, dtype, iso, sts, [sc for _, sc in ms],
                          lmbdas=[lm for lm, _ in ms])
                got, what = run.weighted(huber, l1, has_p, strides=strides)
                run.judge_weighted(got, what, huber, l1, has_p, sts=seen)
                for m in range(M):
                    one = Run(cs, dtype, iso, [seen[m]], [run.scs[m]], lmbdas=[run.lmbdas[m]])
                    alone, _ = one.weighted(huber, l1, has_p)
                    run.same(got, alone, what + " (member %d against the single entry)" % m,
                             m, 0)


# ==================================================================== element-wise kernels
def _judge_elements(got, want, R, S, dtype, kernel, label):
    bad, ratio = pc.excess(got, want, R, S, dtype)
    if not pc.is64(dtype):
        steps.WORST[kernel] = max(steps.WORST.get(kernel, 0.), ratio)
    assert not np.any(bad), "%s %s: %d elements %s, first at %d (worst err / bound %.3g)" % (
        kernel, label, np.count_nonzero(bad),
        "are not the restatement's bits" if pc.is64(dtype) else "outside the gate",
        np.argwhere(bad)[0][0], ratio)


def _elementwise_cases():
    return [(n, off) for n in DD_LENGTHS for off in ((0, 1, 3) if n in (3, 65, 1021) else (0,))]


@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_the_elementwise_kernels_per_element(nsol, dtype):
    """nsol_pdl_dual_data_* and nsol_prox_ell{1,2}_weighted_* at lengths 1 .. 2 * 512 + 37 and
    one past the grid cap of 2048 workgroups (a second trip of the stride loop), with t and
    wt given and NULL, on and off 16-byte alignment, per element; where the weight is zero
    the result is +0 (u itself for the prox) whatever bt holds.  (The stacked entry:
    test_the_stacked_dual_update_member_by_member.)"""
    s = _stream()
    for n, off in _elementwise_cases() + [(2048 * 256 + 37, 0)]:
        a = elementwise_inputs(n, dtype)
        clean = np.where(np.isfinite(a["bt"]), a["bt"], 0.5)
        for l1 in (False, True):
            ar = Arena(dict(out=np.full(n, FILL), u=a["u"], bt=a["bt"], wt=a["wt"]), dtype, off)
            rc = _fn("prox_ell1_weighted" if l1 else "prox_ell2_weighted", dtype)(
                ar.ptr("out"), ar.ptr("u"), ar.ptr("bt"), ar.ptr("wt"), pc.TL, n, s)
            assert rc == 0
            _sync()
            label = "n=%d offset=%d" % (n, off)
            assert ar.guards_intact(), label
            got = ar.get("out", (n,))
            want, R, S = pc.prox_w_expected(a["u"], a["bt"], a["wt"], pc.TL, l1, dtype)
            _judge_elements(got, want, R, S, dtype, "k_prox_w %s" % ("l1" if l1 else "l2"), label)
            for k in ("u", "bt", "wt"):
                assert np.array_equal(ar.get(k, (n,)), a[k], equal_nan=True), (label, k)
            for with_t in (True, False):
                for with_w in (True, False):
                    bt = a["bt"] if with_w else clean
                    ar = Arena(dict(q=a["q"], t=a["t"], bt=bt, wt=a["wt"]), dtype, off)
                    rc = _fn("pdl_dual_data", dtype)(
                        ar.ptr("q"), ar.ptr("t") if with_t else None, ar.ptr("bt"),
                        ar.ptr("wt") if with_w else None, pc.DD_SIGMA, pc.DD_LMBDA, int(l1),
                        n, s)
                    assert rc == 0
                    _sync()
                    label = "n=%d offset=%d t=%d wt=%d" % (n, off, with_t, with_w)
                    assert ar.guards_intact(), label
                    got = ar.get("q", (n,))
                    want, R, S = pc.dual_data_expected(
                        a["q"], a["t"] if with_t else None, bt, a["wt"] if with_w else None,
                        pc.DD_SIGMA, pc.DD_LMBDA, l1, dtype)
                    _judge_elements(got, want, R, S, dtype,
                                    "k_pdl_dual_data %s" % ("l1" if l1 else "l2"), label)
                    if with_w:
                        zero = a["wt"] == 0
                        assert not np.any(got[zero]) and not np.any(np.signbit(got[zero]))
                    for k, v in (("t", a["t"]), ("bt", bt), ("wt", a["wt"])):
                        assert np.array_equal(ar.get(k, (n,)), v, equal_nan=True), (label, k)


@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_the_stacked_dual_update_member_by_member(nsol, dtype):
    """nsol_pdl_stack_dual_data_* with 3 members, a lmbda each (one of them 0), at the
    lengths and offsets of the single entry, t and wt given and NULL in all four
    combinations, bt and wt at member strides 0 and n: every member per element against the
    restatement and bit for bit against the single entry on that member's arrays.  One
    length lies past the grid cap of 2048 workgroups along x -- the kernel has a stride loop
    of its own on a two-dimensional grid --, there with own arrays, l2 with t and wt given
    and l1 with both NULL."""
    s, M = _stream(), 3
    lmbdas = pc.rounded(np.array([pc.DD_LMBDA, 0.6, 0.]), dtype)
    past_cap = 2048 * 256 + 37
    for n, off in _elementwise_cases() + [(past_cap, 0)]:
        ins = [elementwise_inputs(n + 100000 * m, dtype) for m in range(M)]
        ins = [{k: v[:n] for k, v in a.items()} for a in ins]
        cat = lambda k: np.stack([a[k] for a in ins])
        for l1 in (False, True):
            for strides in ("nn", "00", "0n", "n0") if n in (3, 1021) and not off else ("nn",):
                for with_t, with_w in ((True, True), (False, True), (True, False),
                                       (False, False)):
                    if n == past_cap and (with_t, with_w) != (not l1, not l1):
                        continue
                    garbage = with_w and strides[0] == strides[1]
                    bts = [a["bt"] if garbage else np.where(np.isfinite(a["bt"]), a["bt"], 0.5)
                           for a in ins]
                    share = lambda arr, c: arr[:1] if c == "0" else arr
                    ar = Arena(dict(q=cat("q"), t=cat("t"), bt=share(np.stack(bts), strides[0]),
                                    wt=share(cat("wt"), strides[1]), lm=lmbdas), dtype, off)
                    rc = _fn("pdl_stack_dual_data", dtype)(
                        ar.ptr("q"), ar.ptr("t") if with_t else None, ar.ptr("bt"),
                        0 if strides[0] == "0" else n, ar.ptr("wt") if with_w else None,
                        0 if strides[1] == "0" else n, pc.DD_SIGMA, ar.ptr("lm"), int(l1), M,
                        n, s)
                    assert rc == 0
                    _sync()
                    label = "n=%d offset=%d strides=%s t=%d wt=%d" % (n, off, strides, with_t,
                                                                      with_w)
                    assert ar.guards_intact(), label
                    got = ar.get("q", (M, n))
                    for m in range(M):
                        bt = bts[0 if strides[0] == "0" else m]
                        wt = ins[0 if strides[1] == "0" else m]["wt"] if with_w else None
                        want, R, S = pc.dual_data_expected(
                            ins[m]["q"], ins[m]["t"] if with_t else None, bt, wt, pc.DD_SIGMA,
                            lmbdas[m], l1, dtype)
                        _judge_elements(got[m], want, R, S, dtype,
                                        "k_pdl_dual_data_stack %s" % ("l1" if l1 else "l2"),
                                        label + " member %d" % m)
                        # ... and the single entry's bits on that member's arrays
                        one = Arena(dict(q=ins[m]["q"], t=ins[m]["t"], bt=bt,
                                         wt=ins[m]["wt"] if wt is None else wt), dtype, off)
                        assert _fn("pdl_dual_data", dtype)(
                            one.ptr("q"), one.ptr("t") if with_t else None, one.ptr("bt"),
                            one.ptr("wt") if with_w else None, pc.DD_SIGMA, float(lmbdas[m]),
                            int(l1), n, s) == 0
                        _sync()
                        alone = one.get("q", (n,))
                        assert np.array_equal(got[m], alone) and \
                            np.array_equal(np.signbit(got[m]), np.signbit(alone)), label


# ================================================================================ tie states
@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_the_tie_states_come_out_exactly(nsol, dtype):
    """u on lo, on hi and one ulp either side, u = -0.0 on lo = 0, lo == hi; |u - bt| on and
    beside tl w for w in {0.5, 1, 2, 2^-20} and w = 0 over NaN; v on and beside +-c with
    lmbda 1 and 0: equal to the restatement in float32 as well, the sign of a zero
    included."""
    s = _stream()
    for name in pc.STACK_TIE_CASES:
        cs = pc.scase_named(name, dtype)
        pl = pc.scase_plan(cs, dtype)
        seam = pl.TX if pl.form.ntx >= 2 else None
        for iso in (False, True):
            for kind, box in pc.LIN_TIE_BOXES.items():
                st = pc.lin_tie_state(cs.shape, dtype, seam, kind)
                run = Run(cs, dtype, iso, [st], [pc.TIE], unit=True)
                got, what = run.lin(box, False, False)
                assert not got[0].any(), run.cx[0].label(what + ": p_out != 0")
                run.judge_lin(got, what + " (%s ties)" % kind, box, False, False, exact=True)
            st = pc.wgt_tie_state(cs.shape, dtype, seam)
            run = Run(cs, dtype, iso, [st], [pc.TIE], unit=True,
                      lmbdas=[pc.TIE.tl / pc.TIE.tau])
            got, what = run.weighted(False, True, False)
            run.judge_weighted(got, what + " (l1 ties)", False, True, False, exact=True)
    for lmbda in (1., 0.):
        for n, off in ((259, 0), (259, 1), (70, 3)):
            a = pc.dual_data_tie_state(n, dtype, lmbda)
            for with_t in (True, False):
                ar = Arena(dict(a), dtype, off)
                assert _fn("pdl_dual_data", dtype)(
                    ar.ptr("q"), ar.ptr("t") if with_t else None, ar.ptr("bt"), ar.ptr("wt"),
                    pc.TIE.sigma, lmbda, 1, n, s) == 0
                _sync()
                want = vn.pdl_dual_data(a["q"], a["t"] if with_t else None, a["bt"], a["wt"],
                                        pc.TIE.sigma, lmbda, True, dtype)
                bad, _ = pc.excess(ar.get("q", (n,)), want, 0, 0., dtype, exact=True)
                assert not np.any(bad) and ar.guards_intact(), (lmbda, n, off, with_t,
                                                                np.argwhere(bad)[:3])


# ================================================================================== refusals
@pytest.mark.parametrize("dtype", BOTH, ids=["f64", "f32"])
def test_the_entries_decline_and_write_nothing(nsol, dtype):
    from nsol_amd import ops
    shape, M = (3, 4, 5), 2
    n, s = 60, _stream()
    held = dict(xi=np.full(M * n, 0.25), xo=np.full(M * n, 0.25), x=np.full(M * n, 0.25),
                bt=np.full(M * n, 0.25), wt=np.full(M * n, 0.25), pi=np.full(3 * M * n, 0.25),
                po=np.full(3 * M * n, 0.25), q=np.full(M * n, 0.25), t=np.full(M * n, 0.25),
                lm=np.full(M, 0.25))
    ar = Arena(held, dtype)
    P = ar.ptr
    w, sc = (1., 1., 1.), pc.RANDOM
    tab = ops.pd_weighted_table(ar.buf, M, [1.25] * M, [[sc.sigma]] * M, [[sc.tau]] * M,
                                [[sc.theta]] * M, False, 0.05, ops.PD_DATA_WEIGHTED)

    def lin(xi="xi", xo="xo", pi="pi", po="po", lo=0., hi=1., flags=0, members=None,
            sigma=sc.sigma):
        tail = (3,) + shape + w + (sigma, 1.0, sc.tau, sc.theta, lo, hi, flags, 1, s)
        ptrs = (P(xi), P(xo), P("x"), P("bt"), P(pi), P(po))
        if members is None:
            return _fn("pdl_iter", dtype)(*ptrs, *tail)
        return _fn("pdl_stack_iter", dtype)(*ptrs, members, *tail)

    def wgt(xi="xi", xo="xo", pi="pi", po="po", wt="wt", bts=n, wts=n, members=M,
            flags=ops.PD_DATA_WEIGHTED):
        return _fn("pd_weighted_iter", dtype)(
            P(xi), P(xo), P("x"), P("bt"), bts, P(wt) if wt else None, wts, P(pi), P(po),
            members, 3, *shape, *w, tab.data_ptr(), 0, flags, s)

    def dd(t="t", sigma=0.3, lmbda=1., n_=n, members=None, bts=n, wts=n):
        if members is None:
            return _fn("pdl_dual_data", dtype)(P("q"), P(t), P("bt"), P("wt"), sigma, lmbda,
                                               0, n_, s)
        return _fn("pdl_stack_dual_data", dtype)(P("q"), P(t), P("bt"), bts, P("wt"), wts,
                                                 sigma, P("lm"), 0, members, n_, s)

    for members in (None, M):
        assert lin(xo="xi", members=members) == -1           # xbar_in == xbar_out
        assert lin(po="pi", members=members) == -1           # p_in == p_out
        assert lin(lo=1., hi=0.5, members=members) == -1     # lo > hi
        assert lin(lo=np.nan, members=members) == -1 and lin(hi=np.nan, members=members) == -1
        assert lin(flags=ops.PD_DATA_L1, members=members) == -1
        assert lin(flags=ops.PD_DATA_WEIGHTED, members=members) == -1
    assert lin(members=0) == -2 and lin(members=65536) == -2 and lin(members=-1) == -2
    assert lin(members=M, sigma=0.) == -1 and lin(members=M, sigma=-1.) == -1
    assert wgt(xo="xi") == -1 and wgt(po="pi") == -1
    assert wgt(flags=0) == -1 and wgt(flags=ops.PD_DATA_L1) == -1   # no weighted flag
    assert wgt(wt=None) == -1
    for stride in (1, n - 1, 2 * n, -n):
        assert wgt(bts=stride) == -1 and wgt(wts=stride) == -1, stride
    assert wgt(members=0) == -2 and wgt(members=65536) == -2
    for members in (None, M):
        assert dd(t="q", members=members) == -1              # q == t
        assert dd(sigma=0., members=members) == -1 and dd(sigma=-0.3, members=members) == -1
        assert dd(n_=-1, members=members) == -1
    assert dd(lmbda=-1e-9) == -1
    assert dd(members=0) == -2 and dd(members=65536) == -2
    for stride in (1, 2 * n):
        assert dd(members=M, bts=stride) == -1 and dd(members=M, wts=stride) == -1
    for name in ("prox_ell2_weighted", "prox_ell1_weighted"):
        f = _fn(name, dtype)
        assert f(P("xo"), P("x"), P("bt"), P("wt"), 0.5, -1, s) == -1
        assert f(P("xo"), P("x"), P("bt"), None, 0.5, n, s) == -1
        assert f(None, P("x"), P("bt"), P("wt"), 0.5, n, s) == -1
    _sync()
    assert ar.guards_intact()
    for k, v in held.items():
        assert np.array_equal(ar.get(k, v.shape), v), k
    # ... and the good calls run
    assert lin() == 0 and lin(members=M) == 0 and wgt() == 0 and dd() == 0 and \
        dd(members=M) == 0
    _sync()
    assert ar.guards_intact()
    for k in ("xo", "x", "po", "q"):
        assert not np.array_equal(ar.get(k, held[k].shape), held[k]), k
