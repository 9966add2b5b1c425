"""The one-pass periodic 3-D blur (nsol_corr3_wrap_*: k_blur3_dma of nsol_blur3_dma.hpp,
k_blur3_wrap / k_blur3_wrap_pp of nsol_conv.hip) against a float64 reference PER VOXEL,
with taps that differ on every axis, through nsol_amd.ops.  Needs a real MI355X.

Nothing here compares a kernel with another kernel.  Reference, tap sets, inputs, shapes
and the table of which entry point answers are blur3_cases.py; test_blur3_host.py shows on
the CPU that every planted mistake (tz / ty / tx swapped, taps reversed, the x wrap reading
the mirror neighbour, a seam row from the neighbouring plane, a tap off by 2^-12) breaks
the gate below on every (shape, tap kind, type) used here.

Gate, per voxel:  |got - ref| <= C u S,  u = 2^-24 / 2^-53, S the same expression in
float64 with every term replaced by its absolute value.  C counted from the arithmetic
(the library is built with -ffp-contract=off: only the explicit fma builtins fuse):
  plain, DMA          C = 3 ntaps + 3   three taps rounded to T per product; one fma per
                                        tap and pass (the packed float x pass: (ntaps + 1)
                                        / 2 fmas on each pair grid and one sum, no more);
                                        no (a + b) fold of the symmetric taps
  plain, register     C = 6 ntaps       `acc += w v`: a product and a sum per tap, 2 ntaps
                                        - 1 per pass, + 3
  axpby               C = 3 ntaps + 6   ca *, cb *, +;  S = |ca| S_blur + |cb| |io0|
  norms               out as plain
  lanczos_a / _a2     t as plain; q0 = c1 K'K y + c0 y + c2 y_prev against the float64
                      formula within C_LANCZOS eps M of test_lsmr_steps_gpu.py
  lanczos_b           C = 3 ntaps + 7   y_new = (ca A t + q0) + cy y on the kernel's own
                                        stored t and q0;  S = |ca| S(t) + |q0| + |cy| |y|
  lanczos_b2          the same with q0 formed in float64 from y, y_prev: its C_LANCZOS
                      eps M is added to the bound
  loss                C = 3 ntaps + 3 + grad_R(loss) (vector_cases.py) on S_blur + |b|:
                      r -> rho'(r^2) r is 1-Lipschitz for linear, soft_l1 and huber, so the
                      blur's error passes through unamplified, also across Huber's threshold
Sums (axpby's result, the two slots of norms, the board's 3 j + 1 .. 3 j + 3, the loss
cost): against math.fsum over what the kernel stored and against the float64 reference,
relative 3e-7 (float32) / 1e-12 (float64); sum |grad x|^2 is of the INPUT (forward
differences, zero behind the last voxel, one case with non-unit weights).  The device
coefficients coef[0..2], coef[4..5] against the host formulas.

Every call asserts blur3_cases.applies(): answered exactly where the table says so, and
on -2 the output still holds its fill.  The return code cannot tell WHICH kernel answered
a plain call with symmetric taps; but axpby and norms answer through k_blur3_dma alone,
and they are asserted on the same operands (so a DMA form that declined would show), and
the register kernels are asserted with asymmetric taps and with corr_blur3_dma = 0.

Instantiations reached (T = float32 / float64; tap counts 3 .. 17 unless noted):
  k_blur3_dma  ISO false  EPI 0 / 1 / 2  RAG false and true   gauss_aniso, sym_signed
               (EPI 1 float64: to 13; EPI 2 float64: to 13; EPI 2 RAG: to 15)
               ISO true   EPI 0 / 1 / 2  RAG false and true   iso32 in float32, 7 and 13
               (the same iso32 taps take ISO false in float64)
               ISO false  EPI 3 / 4 / 5 / 6, RAG false        5 .. 13 (float64: 9; EPI 2
               as the first lean half and EPI 6: 11)
  k_blur3_wrap            3, 15, 17 (float64: 13 too), aligned rows
  k_blur3_wrap_pp PP = 2  5 .. 13 (float64: 11), aligned;  PP = 1 RAGX: ragged rows
  z-chunk seams (corr_blur3_zchunk 1 and 4 at nz = 7) for every form
Left out on purpose: ISO true with EPI 3 .. 6 (the existing bit-for-bit parity tests run
exactly that, and the epilogues do not read the taps); the 3-GiB-plane and 2^31 limits
(shapes above 4e5 voxels); cauchy / arctan (the entry point declines them, tested in
test_gpu_parity.py).

Largest |got - ref| / (u S) observed on an MI355X (float32 / float64), against C = 18 at
3 taps .. 54 at 17 (register kernels 18 .. 102):
  plain      k_blur3_dma 6.27 / 5.91, RAG 6.52 / 5.90;  k_blur3_wrap 6.10 / 0,
             k_blur3_wrap_pp PP = 2 6.13 / 0, PP = 1 RAGX 7.53 / 0  (float64, contraction
             off: the register kernels round where NumPy rounds, in the same order)
  axpby      4.84 / 4.98, RAG 6.01 / 5.40                      (C + 3)
  norms      out 6.27 / 5.91, RAG 6.52 / 5.90
  lanczos_a  t 6.27 / 4.31;  q0 3.01 / 0 of 2 C_LANCZOS = 20
  lanczos_a2 t 6.27 / 4.31
  lanczos_b  y_new 4.57 / 4.57;  lanczos_b2 4.56 / 4.60       (C + 4)
  loss       linear 7.06 / 4.65, soft_l1 2.95 / 2.37, huber 3.63 / 2.93   (C + grad_R);
             cost: 1.3e-7 / 3.8e-16 from the float64 reference
Every sum met its gate: float32 at most 7.8e-8 from what was stored and 2.4e-7 from the
reference (axpby, 3 taps, (3, 5, 16): the 1e3 spikes carry the sum and their own rounding
to float32 is most of that), float64 3.5e-16 from both.
Value-only mutations of a scratch build the module was checked to notice: tz and ty
swapped in k_blur3_dma<ISO = false> (every staged, Lanczos and loss case failed; iso32 in
float32, ISO = true, passed), and the y taps reversed in k_blur3_wrap_pp (the asymmetric
cases at 5 .. 13 taps failed, float64 to 11; 3 / 15 / 17 taps, k_blur3_wrap, and the
symmetric sets passed): 159 of 209 tests failed, the 50 others do not run mutated code.
One disagreement between table and library came out of the first run: in float64,
nsol_corr3_wrap_axpby_* declines 15 taps as well as 17 (164864 bytes of LDS with the two
io tiles); the header said 17 only and now says both.
"""
import math

import numpy as np
import pytest

import blur3_cases as bc
import vector_cases as vc
from device_arena import Arena

pytestmark = pytest.mark.gpu

DT_IDS = {np.float32: "f32", np.float64: "f64"}
FILL = 777.0
SUM_GATE = {np.float32: 3e-7, np.float64: 1e-12}
COEF_TOL = {np.float32: 1e-6, np.float64: 1e-14}
W_UNIT, W_ANISO = (1.0, 1.0, 1.0), (1.0, 0.7, 1.3)          # (wx, wy, wz)
CA, CB = 0.8, -1.3
LOSS_F_SCALE = vc.COST_F_SCALE

_RATIOS = {}
_REF = {}


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()                      # fails loudly if the .so is missing
    yield nsol_amd
    for key in sorted(_RATIOS):
        print("largest |got - ref| / (u S): %-22s %-8s %.3g" % (key + (_RATIOS[key],)))


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """A failed assertion lets the next test run; a device error ends the session --
    nothing more is launched on a device that has faulted."""
    yield
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error, stopping: %s" % e, returncode=3)


def _ref(dtype, kind, ntaps, shape, salt=0):
    """(x, reference, S) once per (type, taps, shape); read-only."""
    key = (np.dtype(dtype).name, kind, ntaps, tuple(shape), salt)
    if key not in _REF:
        ts = bc.taps(kind, ntaps)
        x = bc.volume(shape, dtype, salt)
        got = (x, bc.reference(x, *ts), bc.magnitude(x, *ts))
        for a in got:
            a.setflags(write=False)
        _REF[key] = got
    return _REF[key]


def _hold(form, what, got, ref, S, C, dtype, extra=0.0):
    u = bc.unit(dtype)
    got = np.asarray(got, np.float64).reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    S = np.asarray(S, np.float64).reshape(-1)
    assert got.shape == ref.shape == S.shape
    assert np.all(np.isfinite(got)), "%s %s: not finite" % (form, what)
    err = np.abs(got - ref)
    bound = C * u * S + np.asarray(extra, np.float64).reshape(-1)
    pos = bound > 0
    ratio = float(np.max(err[pos] / (bound[pos] / C))) if pos.any() else 0.0
    key = (form, np.dtype(dtype).name)
    _RATIOS[key] = max(_RATIOS.get(key, 0.0), ratio)
    print("%s %s %s: largest |err| / (u S) %.3g of C = %d" % (form, what,
                                                             np.dtype(dtype).name, ratio, C))
    bad = err > bound
    assert not bad.any(), "%s %s: %d of %d voxels past %d u S, worst ratio %.3g, first at " \
        "%d (got %r, ref %r)" % (form, what, int(bad.sum()), bad.size, C, ratio,
                                 int(np.argmax(bad)), got[np.argmax(bad)], ref[np.argmax(bad)])


def _hold_sum(what, got, stored_terms, ref_terms, dtype):
    got = float(got)
    stored = math.fsum(np.asarray(stored_terms, np.float64).reshape(-1).tolist())
    ref = math.fsum(np.asarray(ref_terms, np.float64).reshape(-1).tolist())
    gate = SUM_GATE[dtype]
    print("%s %s: sum %.17g, of what was stored %.3g, of the reference %.3g (gate %g)" % (
        what, np.dtype(dtype).name, got, abs(got - stored) / abs(stored),
        abs(got - ref) / abs(ref), gate))
    assert abs(got - stored) <= gate * abs(stored), what
    assert abs(got - ref) <= gate * abs(ref), what


def _filled(a):
    return bool(np.all(a == FILL))


def _slot(k):
    import torch
    return torch.zeros(k, dtype=torch.float64, device="cuda")


class _Knobs(object):
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from nsol_amd import _lib
        for k, v in self.kw.items():
            _lib.set_param(k, v)

    def __exit__(self, *exc):
        from nsol_amd import _lib
        _lib.reset_params()


def _variants(dtype, ntaps):
    """(name, shape, offset, zchunk) of every run."""
    out = [(name, shape, off, 0) for name, (shape, off) in bc.shapes(dtype, ntaps).items()]
    tiles = bc.shapes(dtype, ntaps)["tiles"][0]
    return out + [("tiles-z%d" % zc, tiles, 0, zc) for zc in bc.ZCHUNKS]


def _C(kernel, ntaps):
    return bc.c_dma(ntaps) if kernel.startswith("dma") else bc.c_reg(ntaps)


# --------------------------------------------------------- plain, axpby, norms
def _run_plain_axpby_norms(dtype, kind, ntaps, dma):
    from nsol_amd import ops
    ts = bc.taps(kind, ntaps)
    sym = bc.is_symmetric(ts, dtype)
    assert sym == bc.SYMMETRIC[kind]
    for name, shape, off, zc in _variants(dtype, ntaps):
        label = "%s %s %d taps %s%s" % (kind, name, ntaps, shape, "" if dma else " dma=0")
        n = int(np.prod(shape))
        x, ref, S = _ref(dtype, kind, ntaps, shape)
        io0 = bc.rounded(np.random.default_rng(n + ntaps).standard_normal(n) * 3.0, dtype)
        w = W_ANISO if name in ("tiles", "rag1") else W_UNIT
        ar = Arena(dict(x=x, out=np.full(n, FILL), io=io0, nout=np.full(n, FILL)), dtype,
                   offset=off)
        args = dict(dma=dma)
        with _Knobs(corr_blur3_zchunk=zc, corr_blur3_dma=int(dma)):
            # plain
            want = bc.applies("plain", dtype, shape, ntaps, sym, off == 0, **args)
            got = ops.corr3_wrap(ar.t["x"], shape, *ts, out=ar.t["out"])
            assert (got is not None) == (want is not None), (label, want)
            if want is None:
                assert _filled(ar.get("out", n)), label
            else:
                _hold("plain " + want, label, ar.get("out", n), ref, S, _C(want, ntaps), dtype)
            # axpby
            want = bc.applies("axpby", dtype, shape, ntaps, sym, off == 0, **args)
            res = _slot(1)
            got = ops.corr3_wrap_axpby(ar.t["x"], ar.t["io"], shape, *ts, CA, CB, result=res)
            assert (got is not None) == (want is not None), (label, want)
            if want is None:
                assert np.array_equal(ar.get("io", n), io0) and float(res[0]) == 0.0, label
            else:
                ca, cb = (vc.c(v, dtype) for v in (CA, CB))
                want_io = ca * ref.reshape(-1) + cb * io0
                _hold("axpby " + want, label, ar.get("io", n), want_io,
                      abs(ca) * S.reshape(-1) + abs(cb) * np.abs(io0), bc.c_dma(ntaps) + 3,
                      dtype)
                _hold_sum("axpby result " + label, res[0], ar.get("io", n) ** 2, want_io ** 2,
                          dtype)
            # norms
            want = bc.applies("norms", dtype, shape, ntaps, sym, off == 0, **args)
            res = _slot(2)
            got = ops.corr3_wrap_norms(ar.t["x"], ar.t["nout"], shape, *ts, w, res)
            assert (got is not None) == (want is not None), (label, want)
            if want is None:
                assert _filled(ar.get("nout", n)) and float(res[0]) == 0.0, label
            else:
                _hold("norms " + want, label, ar.get("nout", n), ref, S, bc.c_dma(ntaps), dtype)
                _hold_sum("norms sum out^2 " + label, res[0], ar.get("nout", n) ** 2, ref ** 2,
                          dtype)
                g = bc.grad_sums(x, w)
                _hold_sum("norms sum |grad x|^2 " + label, res[1], g, g, dtype)
        assert ar.guards_intact(), label
        assert np.array_equal(ar.get("x", shape), x), label


DMA_CASES = [("gauss_aniso", n) for n in bc.NTAPS] + [("sym_signed", n) for n in bc.NTAPS] + \
    [("iso32", 7), ("iso32", 13)]


@pytest.mark.parametrize("dtype", bc.DTYPES, ids=lambda d: DT_IDS[d])
@pytest.mark.parametrize("kind,ntaps", DMA_CASES)
def test_staged_blur_per_voxel(nsol, kind, ntaps, dtype):
    """k_blur3_dma, EPI 0 / 1 / 2, ISO false (iso32 in float32: true), RAG both ways,
    every z-chunk seam; the short ragged rows fall to k_blur3_wrap_pp<.., 1, true>."""
    ts = bc.taps(kind, ntaps)
    assert bc.is_iso(ts, dtype) == (kind == "iso32" and dtype == np.float32)
    _run_plain_axpby_norms(dtype, kind, ntaps, True)


@pytest.mark.parametrize("dtype", bc.DTYPES, ids=lambda d: DT_IDS[d])
@pytest.mark.parametrize("ntaps", bc.NTAPS)
@pytest.mark.parametrize("kind", ["asym", "sym_signed"])
def test_register_blur_per_voxel(nsol, kind, ntaps, dtype):
    """k_blur3_wrap (3, 15, 17 taps), k_blur3_wrap_pp PP = 2 (aligned) and PP = 1 (ragged):
    asymmetric taps, and symmetric ones with the staged kernel switched off."""
    _run_plain_axpby_norms(dtype, kind, ntaps, kind == "asym")


# ---------------------------------------------------------------- Lanczos halves
def _ktk(y64):
    """(K'K y, its magnitude): forward differences with zero behind the last voxel, unit
    spacing -- test_lsmr_steps_gpu.py's reference of the same kernel arithmetic."""
    import test_lsmr_steps_gpu as ls
    ref, M = ls._ktk(y64, (1.0, 1.0, 1.0), 3)
    return ref, M, ls.C_LANCZOS


def _coef(lb, lo, hi):
    return [float(v) for v in lb.coef[lo:hi].cpu().double()]


def _lanczos_case(dtype, kind, ntaps, name, shape, off, zc, lean, ident):
    import torch
    from nsol_amd import ops
    ts = bc.taps(kind, ntaps)
    td = torch.float32 if dtype == np.float32 else torch.float64
    eps, tol = float(np.finfo(dtype).eps), COEF_TOL[dtype]
    label = "%s %s %d taps %s lean=%d ident=%d" % (kind, name, ntaps, shape, lean, ident)
    n = int(np.prod(shape))
    y, _, _ = _ref(dtype, kind, ntaps, shape)
    yp = bc.volume(shape, dtype, salt=1) * 0.5
    rg, ri = (0.0, 0.37) if ident else (0.37, 0.0)
    forms = ("lanczos_a2", "lanczos_b2") if lean else ("lanczos_a", "lanczos_b")
    want_a = bc.applies(forms[0], dtype, shape, ntaps, True, off == 0)
    want_b = bc.applies(forms[1], dtype, shape, ntaps, True, off == 0)
    ktk, Mktk, C_LZ = _ktk(y)
    ktk, Mktk = ktk.reshape(-1), Mktk.reshape(-1)
    yf, ypf = y.reshape(-1), yp.reshape(-1)
    for step, prev in ((0, None), (3, yp)):
        ar = Arena(dict(y=y, yp=yp, t=np.full(n, FILL), q0=np.full(n, FILL),
                        ynew=np.full(n, FILL)), dtype, offset=off)
        prev_t = None if prev is None else ar.t["yp"]
        lb = ops.LanczosBoard(ar.t["y"], 8, rg, ri)
        nb2 = math.fsum((yf * yf).tolist())
        beta, bprev = math.sqrt(nb2), math.sqrt(1.7 * nb2)
        lb.board[3 * step:3 * step + 1] = nb2
        if step == 0:
            lb.init()
            assert np.allclose(_coef(lb, 0, 3), [rg / beta, ri / beta, 0.0], rtol=tol, atol=0)
        else:
            lb.coef[0:3] = torch.tensor([rg / beta, ri / beta, -beta / bprev], dtype=td,
                                        device="cuda")
        c1, c0, c2 = _coef(lb, 0, 3)
        q0_ref = c1 * ktk + c0 * yf + (0.0 if prev is None else c2 * ypf)
        M_q0 = abs(c1) * Mktk + abs(c0) * np.abs(yf) + \
            (0.0 if prev is None else abs(c2) * np.abs(ypf))
        with _Knobs(corr_blur3_zchunk=zc):
            if lean:
                ok = ops.corr3_lanczos_a2(ar.t["y"], ar.t["t"], shape, *ts, lb, step)
            else:
                ok = ops.corr3_lanczos_a(ar.t["y"], prev_t, ar.t["t"], ar.t["q0"], shape, *ts,
                                         lb, step)
            assert ok == (want_a is not None), (label, want_a)
            if not ok:
                assert _filled(ar.get("t", n)) and _filled(ar.get("q0", n)), label
                assert float(lb.board[3 * step + 1]) == 0.0, label
                # (where a first half declines, so does its second half: the table)
                assert want_b is None, label
                if lean:
                    ok = ops.corr3_lanczos_b2(ar.t["yp"], ar.t["y"], None, ar.t["ynew"], shape,
                                              *ts, lb, step)
                else:
                    ok = ops.corr3_lanczos_b(ar.t["yp"], ar.t["q0"], ar.t["y"], ar.t["ynew"],
                                             shape, *ts, lb, step)
                assert not ok, label
                assert _filled(ar.get("ynew", n)) and ar.guards_intact(), label
                assert float(lb.board[3 * step + 3]) == 0.0, label
                continue
            t_st = ar.get("t", shape)
            _, ref, S = _ref(dtype, kind, ntaps, shape)
            _hold(forms[0] + " t", label, t_st, ref, S, bc.c_dma(ntaps), dtype)
            board = lb.board.cpu().numpy()
            _hold_sum("board |A y|^2 " + label, board[3 * step + 1], t_st ** 2, ref ** 2, dtype)
            g = bc.grad_sums(y)
            _hold_sum("board |grad y|^2 " + label, board[3 * step + 2], g, g, dtype)
            if not lean:
                q0_st = ar.get("q0", n)
                _hold("lanczos_a q0", label, q0_st, q0_ref, M_q0, 2 * C_LZ, dtype)
            else:
                assert _filled(ar.get("q0", n)), label
            alfa = (board[3 * step + 1] + rg * board[3 * step + 2]) / nb2 + ri
            ca, cy = _coef(lb, 4, 6)
            assert abs(ca - 1 / beta) <= tol / beta, label
            assert abs(cy + alfa / beta) <= tol * alfa / beta, label
            # second half, on what the first one stored
            tS = bc.magnitude(t_st, *ts).reshape(-1)
            tA = bc.reference(t_st, *ts).reshape(-1)
            if lean:
                ok = ops.corr3_lanczos_b2(ar.t["t"], ar.t["y"], prev_t, ar.t["ynew"], shape, *ts,
                                          lb, step)
                q0_use, q0_S, extra = q0_ref, M_q0, C_LZ * eps * M_q0
            else:
                ok = ops.corr3_lanczos_b(ar.t["t"], ar.t["q0"], ar.t["y"], ar.t["ynew"], shape,
                                         *ts, lb, step)
                q0_use, q0_S, extra = q0_st, np.abs(q0_st), 0.0
            assert ok == (want_b is not None), (label, want_b)
            assert ok, label                                # (the first half answered)
            ynew = ar.get("ynew", n)
            _hold(forms[1] + " y_new", label, ynew, ca * tA + q0_use + cy * yf,
                  abs(ca) * tS + q0_S + abs(cy) * np.abs(yf), bc.c_dma(ntaps) + 4,
                  dtype, extra=extra)
            board = lb.board.cpu().numpy()
            want_new = (ca * tA + q0_use + cy * yf) ** 2
            _hold_sum("board |y_new|^2 " + label, board[3 * step + 3], ynew ** 2, want_new, dtype)
            bn = math.sqrt(board[3 * step + 3])
            cnew = _coef(lb, 0, 3)
            assert np.allclose(cnew, [rg / bn, ri / bn, -bn / beta], rtol=10 * tol, atol=0), label
            if lean:
                # the last step of a solve: no vector stored, the same sum and coefficients
                lb.board[3 * step + 3] = 0.0
                lb.coef[0:3] = torch.tensor([c1, c0, c2], dtype=td, device="cuda")
                assert ops.corr3_lanczos_b2(ar.t["t"], ar.t["y"], prev_t, None, shape, *ts, lb,
                                            step)
                _hold_sum("board |y_new|^2, no vector " + label, lb.board[3 * step + 3],
                          ynew ** 2, want_new, dtype)
                assert _coef(lb, 0, 3) == cnew, label
                assert np.array_equal(ar.get("ynew", n), ynew), label
            assert np.array_equal(ar.get("t", shape), t_st), label
        assert ar.guards_intact(), label
        assert np.array_equal(ar.get("y", shape), y) and np.array_equal(ar.get("yp", shape), yp)


@pytest.mark.parametrize("dtype", bc.DTYPES, ids=lambda d: DT_IDS[d])
@pytest.mark.parametrize("ident", [False, True], ids=["rho_grad", "rho_ident"])
@pytest.mark.parametrize("lean", [False, True], ids=["q0", "lean"])
@pytest.mark.parametrize("ntaps", [5, 7, 9, 11, 13])
@pytest.mark.parametrize("kind", ["gauss_aniso", "sym_signed"])
def test_lanczos_halves_per_voxel(nsol, kind, ntaps, lean, ident, dtype):
    """EPI 3 / 4 and the lean pair EPI 2 / 6 with taps that differ per axis: step 0 without
    y_prev and step 3 with it, z-chunk seams, and -2 with nothing written on ragged rows
    and off the grid."""
    sh = bc.shapes(dtype, ntaps)
    runs = [("tiny",) + sh["tiny"] + (0,), ("tiles",) + sh["tiles"] + (0,)]
    runs += [("tiles-z%d" % zc,) + sh["tiles"] + (zc,) for zc in bc.ZCHUNKS]
    runs += [("rag1",) + sh["rag1"] + (0,), ("offgrid",) + sh["offgrid"] + (0,)]
    for name, shape, off, zc in runs:
        _lanczos_case(dtype, kind, ntaps, name, shape, off, zc, lean, ident)


def test_lanczos_halves_decline_outside_their_tap_counts(nsol):
    from nsol_amd import ops
    for dtype in bc.DTYPES:
        for ntaps in (3, 15, 17):
            shape = (3, 5, 16)
            n = int(np.prod(shape))
            ts = bc.taps("gauss_aniso", ntaps)
            y = bc.volume(shape, dtype)
            ar = Arena(dict(y=y, a=np.full(n, FILL), b=np.full(n, FILL), c=np.full(n, FILL)),
                       dtype)
            lb = ops.LanczosBoard(ar.t["y"], 2, 0.37, 0.0)
            for form in bc.FORMS[3:7]:
                assert bc.applies(form, dtype, shape, ntaps, True, True) is None
            assert not ops.corr3_lanczos_a(ar.t["y"], None, ar.t["a"], ar.t["b"], shape, *ts, lb, 0)
            assert not ops.corr3_lanczos_b(ar.t["y"], ar.t["a"], ar.t["b"], ar.t["c"], shape, *ts,
                                           lb, 0)
            assert not ops.corr3_lanczos_a2(ar.t["y"], ar.t["a"], shape, *ts, lb, 0)
            assert not ops.corr3_lanczos_b2(ar.t["y"], ar.t["a"], None, ar.t["c"], shape, *ts, lb,
                                            0)
            assert all(_filled(ar.get(k, n)) for k in "abc") and ar.guards_intact()


# -------------------------------------------------------------------------- loss
@pytest.mark.parametrize("dtype", bc.DTYPES, ids=lambda d: DT_IDS[d])
@pytest.mark.parametrize("lossname", ["linear", "soft_l1", "huber"])
@pytest.mark.parametrize("ntaps", [5, 7, 9, 11, 13])
@pytest.mark.parametrize("kind", ["gauss_aniso", "sym_signed"])
def test_loss_epilogue_per_voxel(nsol, kind, ntaps, lossname, dtype):
    """EPI 5: g = rho'(r^2) r for r = A x - b against nsol_amd.vector_numpy on the float64
    blur, with r = 0 (to the blur's rounding) and both sides of Huber's threshold planted,
    and the cost; -2 on ragged rows, off the grid and outside 5 .. 13 (9) taps."""
    from nsol_amd import ops
    from nsol_amd import vector_numpy as vn
    ts = bc.taps(kind, ntaps)
    u = bc.unit(dtype)
    sh = bc.shapes(dtype, ntaps)
    runs = [("tiny",) + sh["tiny"] + (0,), ("tiles",) + sh["tiles"] + (0,)]
    runs += [("tiles-z%d" % zc,) + sh["tiles"] + (zc,) for zc in bc.ZCHUNKS]
    runs += [("rag1",) + sh["rag1"] + (0,), ("offgrid",) + sh["offgrid"] + (0,)]
    thr = vn.HUBER_GAMMA * LOSS_F_SCALE
    for name, shape, off, zc in runs:
        label = "%s %s %s %d taps %s" % (lossname, kind, name, ntaps, shape)
        n = int(np.prod(shape))
        x, ref, S = _ref(dtype, kind, ntaps, shape)
        rng = np.random.default_rng(n + 7 * ntaps)
        # b on the other side of zero from A x: r = A x - b then cancels nothing, and the
        # cost can be held to the float64 reference at the sums' gate.  (With b = A x +
        # noise on these spiky inputs, |r| ~ 2 beside S ~ 1e3, the float32 cost is off by
        # up to 3.3e-5 on (3, 5, 16): every r within its per-voxel bound, 2 |g| e summed.)
        rf = ref.reshape(-1)
        b = -np.where(rf < 0, -1.0, 1.0) * np.abs(2.0 * rng.standard_normal(n))
        b[0:8] = ref.reshape(-1)[0:8]                                  # r = 0
        b[8:16] = ref.reshape(-1)[8:16] - thr                          # r = +threshold
        b[n - 8:] = ref.reshape(-1)[n - 8:] + thr * (1.0 + 4 * u)      # r just past -threshold
        b = bc.rounded(b, dtype)
        ar = Arena(dict(x=x, b=b), dtype, offset=off)
        want = bc.applies("loss", dtype, shape, ntaps, True, off == 0)
        slot = _slot(1)
        with _Knobs(corr_blur3_zchunk=zc):
            g = ops.corr3_wrap_loss(ar.t["x"], ar.t["b"], shape, *ts, lossname, LOSS_F_SCALE,
                                    slot)
        assert (g is not None) == (want is not None), (label, want)
        if g is not None:
            from nsol_amd.device import to_numpy
            rho, g_ref = vn.loss_terms(ref.reshape(-1), lossname, LOSS_F_SCALE, b, dtype)
            _hold("loss " + lossname, label, to_numpy(g, dtype).astype(np.float64), g_ref,
                  S.reshape(-1) + np.abs(b), bc.c_dma(ntaps) + vc.grad_R(lossname), dtype)
            cost = 0.5 * math.fsum(rho.tolist())
            got = float(slot[0])
            print("loss cost %s %s: rel. error %.3g" % (label, np.dtype(dtype).name,
                                                        abs(got - cost) / cost))
            assert abs(got - cost) <= SUM_GATE[dtype] * cost, label
        else:
            assert float(slot[0]) == 0.0, label
        assert ar.guards_intact(), label
        assert np.array_equal(ar.get("x", shape), x) and np.array_equal(ar.get("b", n), b)
