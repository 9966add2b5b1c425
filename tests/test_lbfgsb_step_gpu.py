"""The second half of an L-BFGS-B iteration on the device -- k_wcomb (nsol_lb_wcomb_*,
and nsol_lincomb_clip_* through its CLIP form), k_subspace_step (r read, and formed with
RIN), k_mdot, k_mdots, k_diff_dots, k_projgr, k_count_free -- each against the float64
reference of lbfgsb_step_cases.py, per element and per sum.

The C entries are called through ctypes so that every count is reachable.  On the lattice
inputs every output element and every sum must be EQUAL to the reference, in float32 and
float64 (test_lbfgsb_step_host.py proves the lattice exact in any order, and that each of
twelve planted mistakes would change the reference at every case run here).  Lengths: 1,
255, 256, 257 vectors of 16 bytes and the same plus 1, 2, 3 elements (the scalar
instantiations; the subspace step must decline those with -2 and touch nothing), with the
full count tables; two trips and part of a third with max_grid_blocks = 2; 256 * 257 + 3
vectors (k_final's own loop runs twice) and 1024 * 256 + 5 vectors (rgrid's cap) once per
kernel and type.  Inputs are views [:n] of longer allocations whose remainder is NaN;
every output has its fill before the call and sentinels around it, every result row
sentinels behind it, the workspace is refilled before every subspace step (so a ratio read
from the other NV's slot shows), every call is made twice and must give the same bits.

Further: each pointer in turn moved off the 16-byte grid by one element (the mask by one
byte), every EINVAL case of the launchers with the outputs untouched, all four
has_lo / has_hi combinations, lo == hi, masks of all fixed and all free variables, no
mask, diff_dots without c, the step ratio over ALL variables (-inf when nothing limits
the step), NaN / Inf at variables that are not free in every input of the masked kernels,
one pass through the DeviceBackend methods that wrap these entries, and one random-data
case per kernel, form and type with the gates counted in lbfgsb_step_cases.py.

MEASURED on the MI355X, random data (the gates come from the counts in
lbfgsb_step_cases.py, not from these): the largest |got - ref| / (C u S), float32 / float64
  wcomb                C = 29 (3 + 24 + 2)   0.122 / 0.095   (vector and scalar forms alike)
  lincomb_clip         C = 26                0.073 / 0     (the float64 reference adds in
                                             the kernel's order: the same bits)
  step xn, r read      C = 16 (NV = 12)      0.135 / 0.12;   C = 28 (NV = 24)  0.070 / 0.085
  step xn, r formed    C = 30 (NV = 12)      0.061 / 0.05;   C = 54 (NV = 24)  0.034 / 0.023
  step d, diff_dots    C = 1                 1.000 / 0 of u (|xn| + |x|), and equal to the
                                             difference of the stored values in T arithmetic
Every sum met both gates: at most 1e-3 of gram_cases.random_gate from math.fsum of what
was stored, and at most 0.015 of SUM_GATE (3e-7 / 1e-12 of the terms' magnitudes) from the
float64 reference (w[23]'d, r formed, float32; float64 sums: below 1e-3 of it).  hits, the
ratio, projgr and count_free were equal.  On the lattice everything was equal on the first
run, with one exception:
FINDING.  k_mdots zeroed only y at a variable that is not free and still multiplied: with
NaN / Inf stored there in vecs[k] the parent's library returned NaN for exactly those k
(test_nonfinite_values_at_fixed_variables, seen in the vector form with both types; the
scalar instantiation shares the code; k_mdot skips such a variable and was right).  It
selects both factors now; finite sums kept their bits (the existing fused-step and Gram tests pass).

Value-only mutations of a scratch build the module was checked to notice (never
committed): (1) k_wcomb's unrolled loop using wcoef[q + 2] for its fourth vector too: both
wcomb and both lincomb_clip lattice tests failed, and the pointer, bounds / masks,
non-finite, random and backend tests of both types (14 of 25); the subspace-step, mdots,
mdot / diff_dots / projgr, count_free and invalid-argument tests do not run that loop with
nw >= 4 and passed.  (2) subspace_step_impl reading the ratio back from the other NV's rows
of ws (the comparison nw > 12 turned round): all four subspace-step lattice tests failed,
and the bounds / masks, non-finite, random and backend tests (12 of 25); the tests of the
other kernels passed, as did the pointer test, where every subspace step is declined.
"""
import ctypes

import numpy as np
import pytest

import gram_cases as gc
import lbfgsb_step_cases as sc

pytestmark = pytest.mark.gpu

BOTH = [np.float32, np.float64]
IDS = {np.float32: "f32", np.float64: "f64"}
SLACK = 64                          # NaN elements behind (and before) every input
GUARD = 64                          # sentinels before and behind every output
SENTINEL = 4321.0
NAN, INF = float("nan"), float("inf")
NONFINITE = (NAN, INF, -INF)


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    yield nsol_amd
    _lib.reset_params()


def _td(dtype):
    import torch
    return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


def _fn(name, dtype=None):
    from nsol_amd import _lib
    full = "nsol_" + name + ("" if dtype is None else "_" + IDS[dtype])
    return getattr(_lib.load(), full)


def _stream():
    from nsol_amd.device import stream_ptr
    return stream_ptr()


def _sync():
    import torch
    torch.cuda.synchronize()


class _Grid(object):
    """max_grid_blocks for the length of a with-block (None: the library's default)."""

    def __init__(self, cap):
        self.cap = cap

    def __enter__(self):
        from nsol_amd import _lib
        if self.cap:
            _lib.set_param("max_grid_blocks", self.cap)

    def __exit__(self, *exc):
        from nsol_amd import _lib
        _lib.reset_params()


# ---- device arrays -------------------------------------------------------------------
def _dev(a, dtype, shift=0):
    """Device view of len(a) elements of T, `shift` elements off the 16-byte grid, NaN
    before and behind."""
    import torch
    a = np.asarray(a)
    host = np.full(SLACK + shift + a.size + SLACK, NAN, dtype=dtype)
    host[SLACK + shift:SLACK + shift + a.size] = a
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 16 == 0
    return t[SLACK + shift:SLACK + shift + a.size]


def _dev_mask(m, shift=0):
    """int8 view, 0 (free) around it."""
    import torch
    host = np.zeros(SLACK + shift + m.size + SLACK, dtype=np.int8)
    host[SLACK + shift:SLACK + shift + m.size] = m
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 16 == 0
    return t[SLACK + shift:SLACK + shift + m.size]


class _Rows(object):
    """Named rows of one 2-D allocation (one upload): views [:n], NaN behind; mask."""

    def __init__(self, dtype, n, rows, mask=None):
        import torch
        stride = (n + SLACK + 15) // 16 * 16
        host = np.full((len(rows), stride), NAN, dtype=dtype)
        for i, k in enumerate(rows):
            host[i, :n] = rows[k]
        self.t = torch.from_numpy(host).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.v = {k: self.t[i, :n] for i, k in enumerate(rows)}
        self.mask = None if mask is None else _dev_mask(mask)
        self.n, self.dtype = n, dtype

    def __getitem__(self, k):
        return self.v[k]

    def w(self, nw):
        return [self.v[k] for k in range(nw)]


def _lattice_rows(dtype, n, nw):
    L = sc.lattice(n)
    rows = {k: L.w(k) for k in range(nw)}
    rows.update(xcp=L.xcp, x=L.x, g=L.g, r=L.r, y=L.y)
    return L, _Rows(dtype, n, rows, L.mask)


class _Out(object):
    """An output of n elements of T holding FILL, sentinels around it."""

    def __init__(self, n, dtype, shift=0):
        import torch
        self.n, self.off, self.dtype = n, GUARD + shift, dtype
        self.buf = torch.full((GUARD + shift + n + GUARD,), SENTINEL, dtype=_td(dtype),
                              device="cuda")
        self.view = self.buf[self.off:self.off + n]
        self.view.fill_(sc.FILL)

    def ptr(self):
        return self.view.data_ptr()

    def get(self):
        """The raw values (T); the sentinels must be intact."""
        h = self.buf.cpu().numpy()
        assert np.all(h[:self.off] == SENTINEL) and np.all(h[self.off + self.n:] == SENTINEL), \
            "written outside the output"
        return h[self.off:self.off + self.n]

    def untouched(self):
        return bool(np.all(self.get() == np.dtype(self.dtype).type(sc.FILL)))


class _Row(object):
    """A result row of k doubles holding RES_FILL, the same behind it."""

    def __init__(self, k):
        import torch
        self.k = k
        self.buf = torch.full((k + 8,), sc.RES_FILL, dtype=torch.float64, device="cuda")

    def ptr(self):
        return self.buf.data_ptr()

    def get(self):
        h = self.buf.cpu().numpy()
        assert np.all(h[self.k:] == sc.RES_FILL), "result row written behind its end"
        return h[:self.k]

    def untouched(self):
        return bool(np.all(self.buf.cpu().numpy() == sc.RES_FILL))


_WS = {}


def _ws(fill=True):
    import torch
    if "ws" not in _WS:
        _WS["ws"] = torch.empty(int(_fn("lb_gram_ws_doubles")()), dtype=torch.float64,
                                device="cuda")
    if fill:
        _WS["ws"].fill_(sc.WS_FILL)
    return _WS["ws"]


def _ptrs(ts):
    return (ctypes.c_void_p * max(len(ts), 1))(*[t if t is None or isinstance(t, int)
                                                  else t.data_ptr() for t in ts])


def _dbl(v):
    return np.ascontiguousarray(list(v) if len(v) else [0.0], dtype=np.float64)


def _p(t):
    return None if t is None else t.data_ptr()


def _f64(a):
    return np.asarray(a).astype(np.float64)


# ---- one call of each entry: (rc, {name: raw array}) ----------------------------------
def run_wcomb(dtype, n, base, bco, w, wco, scale, mask, shift=0):
    out = _Out(n, dtype, shift)
    bc, wc = _dbl(bco), _dbl(wco)
    rc = _fn("lb_wcomb", dtype)(out.ptr(), n, _p(mask), float(scale), len(base), _ptrs(base),
                                bc.ctypes.data, len(w), _ptrs(w), wc.ctypes.data, _stream())
    _sync()
    return rc, {"out": out.get()}


def run_clip(dtype, n, w, wco, lo, hi, shift=0):
    out = _Out(n, dtype, shift)
    wc = _dbl(wco)
    rc = _fn("lincomb_clip", dtype)(out.ptr(), n, len(w), _ptrs(w), wc.ctypes.data, float(lo),
                                    float(hi), _stream())
    _sync()
    return rc, {"out": out.get()}


def run_step(dtype, n, w, wco, r, rco, xcp, x, g, mask, scale, lo, hi, shift_xn=0,
             shift_d=0, nw=None):
    """r None: nsol_lb_subspace_step_r_* with RB3 / rco."""
    nw = len(w) if nw is None else nw
    xn, d, row = _Out(n, dtype, shift_xn), _Out(n, dtype, shift_d), _Row(nw + 4)
    wc, rc3, rcw = _dbl(wco), _dbl(sc.RB3), _dbl(rco)
    ws = _ws()
    if r is None:
        rc = _fn("lb_subspace_step_r", dtype)(
            _ptrs(w), wc.ctypes.data, nw, rc3.ctypes.data, rcw.ctypes.data, _p(xcp), _p(x),
            _p(g), _p(mask), n, float(scale), float(lo), float(hi), xn.ptr(), d.ptr(),
            row.ptr(), ws.data_ptr(), _stream())
    else:
        rc = _fn("lb_subspace_step", dtype)(
            _ptrs(w), wc.ctypes.data, nw, _p(r), _p(xcp), _p(x), _p(g), _p(mask), n,
            float(scale), float(lo), float(hi), xn.ptr(), d.ptr(), row.ptr(), ws.data_ptr(),
            _stream())
    _sync()
    return rc, {"xn": xn.get(), "d": d.get(), "row": row.buf.cpu().numpy()[:nw + 4 + 8]}


def run_mdots(dtype, n, vecs, y, mask):
    row = _Row(len(vecs))
    rc = _fn("lb_mdots", dtype)(_ptrs(vecs), len(vecs), _p(y), _p(mask), n, row.ptr(),
                                _ws().data_ptr(), _stream())
    _sync()
    return rc, {"row": row.get()}


def run_mdot(dtype, n, a, b, mask):
    row = _Row(1)
    rc = _fn("lb_mdot", dtype)(_p(a), _p(b), _p(mask), n, row.ptr(), _ws().data_ptr(), _stream())
    _sync()
    return rc, {"row": row.get()}


def run_diff_dots(dtype, n, a, b, c, shift=0):
    out, row = _Out(n, dtype, shift), _Row(2)
    rc = _fn("lb_diff_dots", dtype)(_p(a), _p(b), _p(c), out.ptr(), n, row.ptr(),
                                    _ws().data_ptr(), _stream())
    _sync()
    return rc, {"out": out.get(), "row": row.get()}


def run_projgr(dtype, n, x, g, lo, hi):
    row = _Row(1)
    rc = _fn("lb_projgr", dtype)(_p(x), _p(g), n, float(lo), float(hi), row.ptr(),
                                 _ws().data_ptr(), _stream())
    _sync()
    return rc, {"row": row.get()}


def run_count_free(n, mask):
    row = _Row(1)
    rc = _fn("lb_count_free")(_p(mask), n, row.ptr(), _ws().data_ptr(), _stream())
    _sync()
    return rc, {"row": row.get()}


def _twice(run, *args, **kw):
    """The call made twice: the same return code and the same bits; the first answer."""
    rc, a = run(*args, **kw)
    rc2, b = run(*args, **kw)
    assert rc == rc2
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), "a second run gave other bits (%s)" % k
    return rc, a


def _step_row_equal(row, ref, nw, label):
    assert row[0] == ref["hits"], label
    assert row[1] == ref["dd"] and row[2] == ref["gd"], label
    assert np.array_equal(row[3:3 + nw], ref["wd"]), label
    assert row[3 + nw] == ref["nratio"], (label, row[3 + nw], ref["nratio"])
    assert np.all(row[nw + 4:] == sc.RES_FILL), label


# ---- the lattice tables: equality ------------------------------------------------------
@pytest.mark.parametrize("dtype", BOTH, ids=IDS.get)
def test_wcomb_equals_the_reference_on_the_lattice(nsol, dtype):
    """k_wcomb<T, VW> and <T, 1>: nbase 0..3, nw 0..40 (0, 1, 3 remainder trips, 4, 8, 40
    whole groups of four, 5, 39 both), masked with whole 16-byte vectors fixed, and without
    a mask; one workgroup making five trips (max_grid_blocks = 2 halved by wcomb_grid)."""
    rows, ran = None, 0
    for n, nbase, nw, masked, cap in sc.wcomb_cases(dtype):
        if rows is None or rows.n != n:
            L, rows = _lattice_rows(dtype, n, sc.MAXW_COMB if n < 5000 else sc.BIG_NW)
        base, bco, w, wco = sc.wcomb_args(n, nbase, nw)
        ref, _ = sc.wcomb_ref(n, base, bco, w, wco, sc.COMB_SCALE, L.mask if masked else None,
                              dtype)
        with _Grid(cap):
            rc, got = _twice(run_wcomb, dtype, n, [rows[k] for k in ("xcp", "x", "g")[:nbase]],
                             bco, rows.w(nw), wco, sc.COMB_SCALE, rows.mask if masked else None)
        assert rc == 0
        assert np.array_equal(_f64(got["out"]), ref), (n, nbase, nw, masked)
        ran += 1
    assert ran > 350
    # 41 stored vectors: EINVAL, nothing written
    out = _Out(16, dtype)
    rc = _fn("lb_wcomb", dtype)(out.ptr(), 16, None, 1.0, 0, _ptrs([]), _dbl([]).ctypes.data,
                                41, _ptrs([rows[0]] * 41), _dbl([1.0] * 41).ctypes.data,
                                _stream())
    _sync()
    assert rc == sc.EINVAL and out.untouched()


@pytest.mark.parametrize("dtype", BOTH, ids=IDS.get)
def test_lincomb_clip_equals_the_reference_on_the_lattice(nsol, dtype):
    rows = None
    for n, nw, cap in sc.clip_cases(dtype):
        if rows is None or rows.n != n:
            L, rows = _lattice_rows(dtype, n, sc.MAXW_COMB if n < 5000 else sc.BIG_NW)
        w, wco = [L.w(k) for k in range(nw)], sc.box_coefs(nw, 1)
        ref, _ = sc.wcomb_ref(n, [], [], w, wco, 1.0, None, dtype, box=(sc.LO, sc.HI))
        with _Grid(cap):
            rc, got = _twice(run_clip, dtype, n, rows.w(nw), wco, sc.LO, sc.HI)
        assert rc == 0
        assert np.array_equal(_f64(got["out"]), ref), (n, nw)


@pytest.mark.parametrize("rin", [False, True], ids=["r_read", "r_formed"])
@pytest.mark.parametrize("dtype", BOTH, ids=IDS.get)
def test_subspace_step_equals_the_reference_on_the_lattice(nsol, dtype, rin):
    """k_subspace_step<T, VW, 12 / 24, RIN>: nw on both sides of 12 and at 24; xn, d, the
    nw + 3 sums and the ratio (from the slot of the form that ran: ws holds WS_FILL where
    the kernel did not write).  A length that is no multiple of 16 bytes: -2, outputs and
    result row untouched.  nw = 25: -2."""
    rows, ran, declined = None, 0, 0
    for n, nw, cap in sc.step_cases(dtype):
        if rows is None or rows.n != n:
            L, rows = _lattice_rows(dtype, n, sc.MAXW_STEP + 1)
        _, wc, rc_ = sc.step_args(n, nw)
        label = (IDS[dtype], rin, n, nw)
        with _Grid(cap):
            rc, got = _twice(run_step, dtype, n, rows.w(nw), wc, None if rin else rows["r"], rc_,
                             rows["xcp"], rows["x"], rows["g"], rows.mask, sc.STEP_SCALE,
                             sc.LO, sc.HI)
        if not sc.vector_form(n, dtype):
            assert rc == sc.DECLINED, label
            fill = np.dtype(dtype).type(sc.FILL)
            assert np.all(got["xn"] == fill) and np.all(got["d"] == fill), label
            assert np.all(got["row"] == sc.RES_FILL), label
            declined += 1
            continue
        assert rc == 0, label
        ref = sc.step_expected(n, nw, dtype, rin, grid_cap=cap)
        assert np.array_equal(_f64(got["xn"]), ref["xn"]), label
        assert np.array_equal(_f64(got["d"]), ref["d"]), label
        _step_row_equal(got["row"], ref, nw, label)
        ran += 1
    assert ran > 30 and declined > 30
    n = 64
    L, rows = _lattice_rows(dtype, n, 25)
    rc, got = run_step(dtype, n, rows.w(25), [0.125] * 25, None if rin else rows["r"],
                       [0.125] * 25, rows["xcp"], rows["x"], rows["g"], rows.mask, 0.25,
                       sc.LO, sc.HI)
    assert rc == sc.DECLINED and np.all(got["row"] == sc.RES_FILL)
    assert np.all(got["xn"] == np.dtype(dtype).type(sc.FILL))


@pytest.mark.parametrize("dtype", BOTH, ids=IDS.get)
def test_mdots_equals_the_reference_on_the_lattice(nsol, dtype):
    """k_mdots<T, VW, 12>, <T, VW, 24>, <T, 1, 24>; 25 and 49 vectors take two and three
    launches that share ws and write result + 24 k."""
    rows = None
    for n, nvec, cap in sc.mdots_cases(dtype):
        if rows is None or rows.n != n:
            L, rows = _lattice_rows(dtype, n, sc.NW_ROWS if n < 5000 else sc.BIG_NW)
        ref, _ = sc.mdots_ref([L.w(k) for k in range(nvec)], L.y, L.mask, dtype)
        with _Grid(cap):
            rc, got = _twice(run_mdots, dtype, n, rows.w(nvec), rows["y"], rows.mask)
        assert rc == 0
        assert np.array_equal(got["row"], ref), (n, nvec)


@pytest.mark.parametrize("dtype", BOTH, ids=IDS.get)
def test_mdot_diff_dots_projgr_equal_the_reference_on_the_lattice(nsol, dtype):
    for n, cap in sc.plain_cases(dtype):
        L, rows = _lattice_rows(dtype, n, 1)
        px, pg = sc.projgr_inputs(n)
        dx, dg = _dev(px, dtype), _dev(pg, dtype)
        with _Grid(cap):
            for mask, dmask in ((L.mask, rows.mask), (None, None)):
                rc, got = _twice(run_mdot, dtype, n, rows[0], rows["y"], dmask)
                assert rc == 0 and got["row"][0] == sc.mdot_ref(L.w(0), L.y, mask, dtype)[0], n
            for c, dc in ((L.g, rows["g"]), (None, None)):
                rc, got = _twice(run_diff_dots, dtype, n, rows["xcp"], rows["x"], dc)
                out, res, _ = sc.diff_dots_ref(L.xcp, L.x, c, dtype)
                assert rc == 0 and np.array_equal(_f64(got["out"]), out), n
                assert list(got["row"]) == res, (n, c is None)
            for lo in (sc.LO, -INF):
                for hi in (sc.HI, INF):
                    rc, got = _twice(run_projgr, dtype, n, dx, dg, lo, hi)
                    assert rc == 0 and got["row"][0] == sc.projgr_ref(px, pg, lo, hi, dtype), \
                        (n, lo, hi)


def test_count_free_equals_the_reference(nsol):
    """k_count_free<16> (n a multiple of 16) and <1>."""
    forms = set()
    for n, cap in sc.plain_cases(np.float32, 16):
        mask = sc.lattice_mask(n)
        with _Grid(cap):
            rc, got = _twice(run_count_free, n, _dev_mask(mask))
        assert rc == 0 and got["row"][0] == sc.count_free_ref(mask), n
        forms.add(n % 16 == 0)
    assert forms == {True, False}
    for value, want in ((1, 0.0), (0, 1.0), (-128, 1.0), (127, 0.0)):
        m = np.full(16 * 257, value, np.int8)
        assert run_count_free(m.size, _dev_mask(m))[1]["row"][0] == want * m.size
    # one byte off the 16-byte grid: the scalar form, the same count
    mask = sc.lattice_mask(16 * 257)
    rc, got = run_count_free(mask.size, _dev_mask(mask, 1))
    assert rc == 0 and got["row"][0] == sc.count_free_ref(mask)


# ---- alignment -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", BOTH, ids=IDS.get)
def test_each_pointer_off_the_16_byte_grid(nsol, dtype):
    """n a multiple of 16 bytes, one array at a time moved by one element (the mask by one
    byte): the kernels with a scalar form give the same values; the subspace step returns
    -2 and leaves xn, d and the result row as they were."""
    n, nw, nbase = 256 * sc.vw(dtype), 5, 3
    L, rows = _lattice_rows(dtype, n, nw)
    base, bco, w, wco = sc.wcomb_args(n, nbase, nw)
    names = ("xcp", "x", "g")
    ref, _ = sc.wcomb_ref(n, base, bco, w, wco, sc.COMB_SCALE, L.mask, dtype)
    refc, _ = sc.wcomb_ref(n, [], [], w, sc.box_coefs(nw, 1), 1.0, None, dtype,
                           box=(sc.LO, sc.HI))
    _, swc, src = sc.step_args(n, nw)
    host = {k: getattr(L, k) for k in ("xcp", "x", "g", "r", "y")}
    host.update({k: L.w(k) for k in range(nw)})
    moved_mask = _dev_mask(L.mask, 1)
    assert moved_mask.data_ptr() % sc.vw(dtype) == 1
    for moved in list(host) + ["mask", "out", "out2"]:
        def arr(k):
            if k == moved:
                t = _dev(host[k], dtype, 1)
                assert t.data_ptr() % 16 == np.dtype(dtype).itemsize
                return t
            return rows[k]
        mask = moved_mask if moved == "mask" else rows.mask
        sh = 1 if moved == "out" else 0
        dw = [arr(k) for k in range(nw)]
        label = (IDS[dtype], moved)
        rc, got = run_wcomb(dtype, n, [arr(k) for k in names], bco, dw, wco, sc.COMB_SCALE,
                            mask, sh)
        assert rc == 0 and np.array_equal(_f64(got["out"]), ref), label
        rc, got = run_clip(dtype, n, dw, sc.box_coefs(nw, 1), sc.LO, sc.HI, sh)
        assert rc == 0 and np.array_equal(_f64(got["out"]), refc), label
        rc, got = run_mdots(dtype, n, dw, arr("y"), mask)
        assert rc == 0 and np.array_equal(got["row"], sc.mdots_ref(w, L.y, L.mask, dtype)[0]), \
            label
        rc, got = run_mdot(dtype, n, dw[0], arr("y"), mask)
        assert rc == 0 and got["row"][0] == sc.mdot_ref(w[0], L.y, L.mask, dtype)[0], label
        rc, got = run_diff_dots(dtype, n, arr("xcp"), arr("x"), arr("g"), sh)
        out, res, _ = sc.diff_dots_ref(L.xcp, L.x, L.g, dtype)
        assert rc == 0 and np.array_equal(_f64(got["out"]), out) and list(got["row"]) == res, \
            label
        rc, got = run_projgr(dtype, n, arr("x"), arr("g"), sc.LO, sc.HI)
        assert rc == 0 and got["row"][0] == sc.projgr_ref(L.x, L.g, sc.LO, sc.HI, dtype), label
        for rin in (False, True):
            if moved == "y" or (rin and moved == "r"):
                continue
            rc, got = run_step(dtype, n, dw, swc, None if rin else arr("r"), src, arr("xcp"),
                               arr("x"), arr("g"), mask, sc.STEP_SCALE, sc.LO, sc.HI,
                               shift_xn=sh, shift_d=1 if moved == "out2" else 0)
            fill = np.dtype(dtype).type(sc.FILL)
            if moved in ("out", "out2") or moved in host or moved == "mask":
                assert rc == sc.DECLINED, label + (rin,)
                assert np.all(got["xn"] == fill) and np.all(got["d"] == fill), label
                assert np.all(got["row"] == sc.RES_FILL), label


# ---- invalid arguments -----------------------------------------------------------------
def _expect_einval(fn, args, bad, outs, label, want=sc.EINVAL):
    """fn(*args) with args[i] replaced by v for every (i, v) of bad: `want`, and none of
    outs touched."""
    for i, v in bad:
        a = list(args)
        a[i] = v
        rc = fn(*a)
        _sync()
        assert rc == want, (label, i, v, rc)
        for o in outs:
            assert o.untouched(), (label, i, v)


@pytest.mark.parametrize("dtype", BOTH, ids=IDS.get)
def test_invalid_arguments_are_refused_and_nothing_is_written(nsol, dtype):
    n, nw = 64, 3
    L, rows = _lattice_rows(dtype, n, nw)
    out, out2, row = _Out(n, dtype), _Out(n, dtype), _Row(nw + 4)
    ws, st = _ws().data_ptr(), _stream()
    wp, wc = _ptrs(rows.w(nw)), _dbl([0.5] * nw)
    bp, bc = _ptrs([rows["xcp"], rows["x"], rows["g"]]), _dbl(sc.BCOEF)
    holed = _ptrs([rows[0], None, rows[2]])
    outs = [out, out2, row]
    _expect_einval(_fn("lb_wcomb", dtype),
                   [out.ptr(), n, _p(rows.mask), 1.0, 3, bp, bc.ctypes.data, nw, wp,
                    wc.ctypes.data, st],
                   [(1, 0), (1, -5), (0, None), (4, -1), (4, 4), (7, -1), (7, 41)], outs, "wcomb")
    _expect_einval(_fn("lincomb_clip", dtype),
                   [out.ptr(), n, nw, wp, wc.ctypes.data, sc.LO, sc.HI, st],
                   [(1, 0), (0, None), (2, 0), (2, 41), (3, None), (4, None), (3, holed),
                    (5, sc.HI + 1.0), (5, NAN), (6, NAN)], outs, "lincomb_clip")
    xcp, x, g, r = (_p(rows[k]) for k in ("xcp", "x", "g", "r"))
    step = [wp, wc.ctypes.data, nw, r, xcp, x, g, _p(rows.mask), n, 0.25, sc.LO, sc.HI,
            out.ptr(), out2.ptr(), row.ptr(), ws, st]
    _expect_einval(_fn("lb_subspace_step", dtype), step,
                   [(8, 0), (2, 0), (0, None), (1, None), (3, None), (4, None), (5, None),
                    (6, None), (12, None), (13, None), (14, None), (15, None), (0, holed)],
                   outs, "subspace_step")
    _expect_einval(_fn("lb_subspace_step", dtype), step, [(2, 25)], outs, "subspace_step",
                   sc.DECLINED)
    rb, rw = _dbl(sc.RB3), _dbl([0.25] * nw)
    stepr = [wp, wc.ctypes.data, nw, rb.ctypes.data, rw.ctypes.data, xcp, x, g,
             _p(rows.mask), n, 0.25, sc.LO, sc.HI, out.ptr(), out2.ptr(), row.ptr(), ws, st]
    _expect_einval(_fn("lb_subspace_step_r", dtype), stepr,
                   [(9, 0), (2, 0), (0, None), (1, None), (3, None), (4, None), (5, None),
                    (6, None), (7, None), (13, None), (14, None), (15, None), (16, None),
                    (0, holed)], outs, "subspace_step_r")
    _expect_einval(_fn("lb_mdots", dtype),
                   [wp, nw, _p(rows["y"]), _p(rows.mask), n, row.ptr(), ws, st],
                   [(0, None), (1, 0), (2, None), (4, 0), (5, None), (6, None), (0, holed)],
                   outs, "mdots")
    _expect_einval(_fn("lb_mdot", dtype),
                   [_p(rows[0]), _p(rows["y"]), _p(rows.mask), n, row.ptr(), ws, st],
                   [(3, 0), (0, None), (1, None), (4, None), (5, None)], outs, "mdot")
    _expect_einval(_fn("lb_diff_dots", dtype),
                   [xcp, x, g, out.ptr(), n, row.ptr(), ws, st],
                   [(0, None), (1, None), (3, None), (4, 0), (5, None), (6, None)], outs,
                   "diff_dots")
    _expect_einval(_fn("lb_projgr", dtype), [x, g, n, sc.LO, sc.HI, row.ptr(), ws, st],
                   [(2, 0), (0, None), (1, None), (5, None), (6, None)], outs, "projgr")
    _expect_einval(_fn("lb_count_free"), [_p(rows.mask), n, row.ptr(), ws, st],
                   [(1, -1), (2, None), (3, None), (0, None)], outs, "count_free")


# ---- beyond the tables -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", BOTH, ids=IDS.get)
def test_bounds_masks_and_the_ratio_over_all_variables(nsol, dtype):
    """All four has_lo / has_hi combinations, masks of all fixed and all free variables and
    no mask, at nw = 12 and 13 (the two forms keep the ratio in different slots of ws).
    The ratio is the minimum over ALL variables: with the lattice mask it comes from a
    variable that is not free (the reference over the free ones alone is another value);
    without bounds result[nw + 3] is -inf."""
    n = 257 * sc.vw(dtype)
    L, rows = _lattice_rows(dtype, n, 13)
    masks = {"lattice": L.mask, "fixed": np.full(n, 2, np.int8), "free": np.full(n, -1, np.int8),
             "none": None}
    dmask = {k: (None if m is None else _dev_mask(m)) for k, m in masks.items()}
    for nw in (12, 13):
        w, wc, rc_ = sc.step_args(n, nw)
        for lo in (sc.LO, -INF):
            for hi in (sc.HI, INF):
                for mk, mask in masks.items():
                    if mk != "lattice" and (lo, hi) not in ((sc.LO, sc.HI), (-INF, INF)):
                        continue
                    for rin in (False, True):
                        label = (IDS[dtype], nw, lo, hi, mk, rin)
                        ref = sc.step_ref(w, wc, None if rin else L.r, rc_, L.xcp, L.x, L.g, mask,
                                          sc.STEP_SCALE, lo, hi, dtype)
                        rc, got = _twice(run_step, dtype, n, rows.w(nw), wc,
                                         None if rin else rows["r"], rc_, rows["xcp"], rows["x"],
                                         rows["g"], dmask[mk], sc.STEP_SCALE, lo, hi)
                        assert rc == 0, label
                        assert np.array_equal(_f64(got["xn"]), ref["xn"]), label
                        assert np.array_equal(_f64(got["d"]), ref["d"]), label
                        _step_row_equal(got["row"], ref, nw, label)
                        if lo == -INF and hi == INF:
                            assert got["row"][nw + 3] == -INF and got["row"][0] == 0.0, label
                        if mk == "fixed":
                            assert np.array_equal(_f64(got["xn"]), L.xcp), label
                        if mk == "lattice" and (lo, hi) == (sc.LO, sc.HI):
                            free_only = sc.neg_ratio(L.x, ref["d"], lo, hi, dtype, L.free)
                            assert -free_only >= 1.0 > -got["row"][nw + 3] >= 0.0, label
    # wcomb: every variable fixed, every variable free
    base, bco, w, wco = sc.wcomb_args(n, 3, 13)
    for mk in ("fixed", "free"):
        ref, _ = sc.wcomb_ref(n, base, bco, w, wco, sc.COMB_SCALE, masks[mk], dtype)
        rc, got = _twice(run_wcomb, dtype, n, [rows[k] for k in ("xcp", "x", "g")], bco,
                         rows.w(13), wco, sc.COMB_SCALE, dmask[mk])
        assert rc == 0 and np.array_equal(_f64(got["out"]), ref), mk
        assert mk != "fixed" or not got["out"].any()
    # lincomb_clip: lo == hi, and one-sided boxes
    wco = sc.box_coefs(13, 1)
    for lo, hi in ((1.25, 1.25), (-INF, sc.HI), (sc.LO, INF), (-INF, INF)):
        ref, _ = sc.wcomb_ref(n, [], [], w, wco, 1.0, None, dtype, box=(lo, hi))
        rc, got = _twice(run_clip, dtype, n, rows.w(13), wco, lo, hi)
        assert rc == 0 and np.array_equal(_f64(got["out"]), ref), (lo, hi)
        assert lo != hi or np.all(got["out"] == 1.25)


# ---- non-finite values at variables that are not free ---------------------------------
def _fixed_spots(L, n):
    """A variable inside a wholly fixed run, one beside free ones, the last fixed one."""
    fixed = np.flatnonzero(~L.free)
    run = sc.fixed_runs(n)[0][0] + 3
    beside = int(fixed[(fixed > 40) & L.free[np.minimum(fixed + 1, n - 1)]][0])
    return [run, beside, int(fixed[-1])]


@pytest.mark.parametrize("dtype", BOTH, ids=IDS.get)
def test_nonfinite_values_at_fixed_variables(nsol, dtype):
    """NaN, +Inf, -Inf planted at three variables that are not free, as include/nsol_hip.h
    decides: wcomb's out is 0 there and clean elsewhere; mdot and mdots return the finite sum
    over the free variables (k_mdots multiplied such a value with a zeroed y before: NaN);
    the subspace step's xn and d show no trace of r or the stored vectors (the products
    w'd are plain sums over all variables and are NaN for exactly the planted vectors),
    and a non-finite xcp, x or g at a fixed variable stays in its own element of xn / d."""
    n, nw = 257 * sc.vw(dtype) * 2, 13
    L = sc.lattice(n)
    spots = _fixed_spots(L, n)
    host = {k: np.array(L.w(k)) for k in range(nw)}
    host.update(xcp=np.array(L.xcp), x=np.array(L.x), g=np.array(L.g), r=np.array(L.r),
                y=np.array(L.y))
    planted = (0, 3, 4, 12, "r", "y")
    for j, k in enumerate(planted):
        for s, spot in enumerate(spots):
            host[k][spot] = NONFINITE[(s + j) % 3]
    rows = _Rows(dtype, n, host, L.mask)
    w = [L.w(k) for k in range(nw)]
    # mdot, mdots
    ref, _ = sc.mdots_ref(w, L.y, L.mask, dtype)
    for label, vecs in (("vector", rows.w(nw)), ("scalar", rows.w(nw - 1) + [_dev(host[12], dtype, 1)])):
        rc, got = _twice(run_mdots, dtype, n, vecs, rows["y"], rows.mask)
        assert rc == 0 and np.array_equal(got["row"], ref), (label, got["row"], ref)
    rc, got = _twice(run_mdot, dtype, n, rows[0], rows["y"], rows.mask)
    assert rc == 0 and got["row"][0] == ref[0]
    # wcomb, with the base vectors planted too
    for k in ("xcp", "x", "g"):
        for s, spot in enumerate(spots):
            host[k][spot] = NONFINITE[s]
    rows3 = _Rows(dtype, n, host, L.mask)
    base, bco, _, wco = sc.wcomb_args(n, 3, nw)
    ref, _ = sc.wcomb_ref(n, base, bco, w, wco, sc.COMB_SCALE, L.mask, dtype)
    rc, got = _twice(run_wcomb, dtype, n, [rows3[k] for k in ("xcp", "x", "g")], bco,
                     rows3.w(nw), wco, sc.COMB_SCALE, rows3.mask)
    assert rc == 0 and np.array_equal(_f64(got["out"]), ref) and not got["out"][spots].any()
    # the subspace step: r and the stored vectors planted
    _, wc, rc_ = sc.step_args(n, nw)
    hit = np.array([k in planted for k in range(nw)])
    for rin in (False, True):
        ref = sc.step_expected(n, nw, dtype, rin)
        rc, got = _twice(run_step, dtype, n, rows.w(nw), wc, None if rin else rows["r"], rc_,
                         rows["xcp"], rows["x"], rows["g"], rows.mask, sc.STEP_SCALE, sc.LO,
                         sc.HI)
        assert rc == 0
        assert np.array_equal(_f64(got["xn"]), ref["xn"]), rin
        assert np.array_equal(_f64(got["d"]), ref["d"]), rin
        row = got["row"]
        assert (row[0], row[1], row[2]) == (ref["hits"], ref["dd"], ref["gd"]), rin
        assert np.array_equal(np.isnan(row[3:3 + nw]), hit), rin
        assert np.array_equal(row[3:3 + nw][~hit], ref["wd"][~hit]), rin
        assert row[3 + nw] == ref["nratio"], rin
        # xcp = +Inf, x = NaN, g = -Inf at three fixed variables: their own elements only
        rc, got = _twice(run_step, dtype, n, rows.w(nw), wc, None if rin else rows["r"], rc_,
                         rows3["xcp"], rows3["x"], rows3["g"], rows.mask, sc.STEP_SCALE,
                         sc.LO, sc.HI)
        assert rc == 0
        xn, d = _f64(got["xn"]), _f64(got["d"])
        clean = np.ones(n, bool)
        clean[spots] = False
        assert np.array_equal(xn[clean], ref["xn"][clean]), rin
        assert np.array_equal(d[clean], ref["d"][clean]), rin
        assert np.isnan(xn[spots[0]]) and xn[spots[1]] == INF and xn[spots[2]] == -INF, rin
        assert np.all(~np.isfinite(d[spots])), rin
        assert got["row"][0] == ref["hits"], rin


# ---- random data -----------------------------------------------------------------------
_WORST = {}


def _hold(kernel, dtype, got, ref, S, C, label):
    """|got - ref| <= C u S per element; the largest ratio is printed."""
    err = np.abs(_f64(got) - ref)
    gate = C * sc.unit(dtype) * S
    assert np.all(err[gate == 0] == 0), label
    ratio = float(np.max(err[gate > 0] / gate[gate > 0])) if np.any(gate > 0) else 0.0
    key = (kernel, IDS[dtype])
    _WORST[key] = max(_WORST.get(key, 0.0), ratio)
    print("lbfgsb_step %-16s %s: worst |got - ref| / (C u S) = %.3f  (C = %d)  %r"
          % (kernel, IDS[dtype], ratio, C, label))
    assert np.all(err <= gate), (label, ratio)


def _hold_sum(kernel, dtype, got, stored_terms, ref_terms, label):
    """got against math.fsum of what was stored (order-free bound) and against the float64
    reference (SUM_GATE of the reference terms' magnitudes)."""
    import math
    st = np.asarray(stored_terms, np.float64)
    exact = math.fsum(st.tolist())
    gate = gc.random_gate(float(np.abs(st).sum()), st.size)
    rt = np.asarray(ref_terms, np.float64)
    ref, mag = math.fsum(rt.tolist()), float(np.abs(rt).sum())
    a = abs(got - exact) / gate if gate else 0.0
    b = abs(got - ref) / (sc.SUM_GATE[dtype] * mag) if mag else 0.0
    for key, v in ((("sum/stored", kernel), a), (("sum/ref", kernel), b)):
        k = key + (IDS[dtype],)
        _WORST[k] = max(_WORST.get(k, 0.0), v)
    print("lbfgsb_step %-16s %s: sum error / gate: %.3g of what was stored, %.3g of the "
          "reference  %r" % (kernel, IDS[dtype], a, b, label))
    assert abs(got - exact) <= gate, (label, got, exact)
    assert abs(got - ref) <= sc.SUM_GATE[dtype] * mag, (label, got, ref)


RANDOM_NV = sc.TRIPS_NV                 # five workgroups; the scalar forms at + 1


@pytest.mark.parametrize("dtype", BOTH, ids=IDS.get)
def test_random_data_within_the_counted_bounds(nsol, dtype):
    """Normal data, one case per kernel, form and type (vector and scalar forms where there
    are two): the per-element gates C u S of lbfgsb_step_cases.py, the sums against fsum of
    what was stored and against the reference; hits, the ratio, projgr and the differences
    exactly."""
    for n in (RANDOM_NV * sc.vw(dtype), RANDOM_NV * sc.vw(dtype) + 1):
        D = sc.random_inputs(n, dtype)
        nw, nbase = sc.MAXW_STEP, 3
        host = {k: D["w"][k] for k in range(nw + 3)}
        host.update({k: D[k] for k in ("xcp", "x", "g", "r", "y")})
        rows = _Rows(dtype, n, host, D["mask"])
        w = [D["w"][k] for k in range(nw)]
        form = "vec" if sc.vector_form(n, dtype) else "scalar"
        # wcomb, lincomb_clip (27 vectors: three of them as base vectors)
        bco, wco = (-0.83, 0.83, -1.0), list(np.linspace(-0.7, 0.9, nw))
        base = [D["w"][nw + k] for k in range(3)]
        ref, S = sc.wcomb_ref(n, base, bco, w, wco, 0.3, D["mask"], dtype)
        rc, got = _twice(run_wcomb, dtype, n, [rows[nw + k] for k in range(3)], bco, rows.w(nw),
                         wco, 0.3, rows.mask)
        assert rc == 0
        _hold("wcomb " + form, dtype, got["out"], ref, S, sc.wcomb_count(nbase, nw), n)
        lo, hi = -0.75, 1.0
        ref, S = sc.wcomb_ref(n, [], [], w, wco, 1.0, None, dtype, box=(lo, hi))
        rc, got = _twice(run_clip, dtype, n, rows.w(nw), wco, lo, hi)
        assert rc == 0
        _hold("lincomb_clip " + form, dtype, got["out"], ref, S, sc.wcomb_count(0, nw), n)
        assert np.mean(_f64(got["out"]) == lo) > 0.1 and np.mean(_f64(got["out"]) == hi) > 0.1
        # mdot, mdots, diff_dots, projgr
        keep = D["mask"] <= 0
        rc, got = _twice(run_mdots, dtype, n, rows.w(nw), rows["y"], rows.mask)
        assert rc == 0
        for k in (0, 11, 12, 23):
            t = (w[k] * D["y"])[keep]
            _hold_sum("mdots " + form, dtype, got["row"][k], t, t, (n, k))
        rc, got = _twice(run_mdot, dtype, n, rows[0], rows["y"], rows.mask)
        t = (w[0] * D["y"])[keep]
        _hold_sum("mdot " + form, dtype, got["row"][0], t, t, n)
        rc, got = _twice(run_diff_dots, dtype, n, rows["xcp"], rows["x"], rows["g"])
        out, _, _ = sc.diff_dots_ref(D["xcp"], D["x"], D["g"], dtype)
        assert rc == 0 and np.array_equal(_f64(got["out"]), out), n
        exact = D["xcp"] - D["x"]
        _hold_sum("diff_dots " + form, dtype, got["row"][0], out * out, exact * exact, n)
        _hold_sum("diff_dots " + form, dtype, got["row"][1], out * D["g"], exact * D["g"], n)
        for lo_, hi_ in ((lo, hi), (-INF, hi), (lo, INF)):
            rc, got = _twice(run_projgr, dtype, n, rows["x"], rows["g"], lo_, hi_)
            assert rc == 0 and got["row"][0] == sc.projgr_ref(D["x"], D["g"], lo_, hi_, dtype), n
        if form == "scalar":
            continue
        # the subspace step: r read and formed, the NV = 12 and the NV = 24 instantiation
        for rin, nws in ((False, 12), (False, 24), (True, 12), (True, 24)):
            name = "step %s NV=%d" % ("r formed" if rin else "r read", nws)
            ws_, wd = w[:nws], rows.w(nws)
            wc = list(np.linspace(-0.45, 0.55, nws))
            rcf = list(np.linspace(0.35, -0.3, nws))
            ref = sc.step_ref(ws_, wc, None if rin else D["r"], rcf, D["xcp"], D["x"], D["g"],
                              D["mask"], 0.6, lo, hi, dtype)
            rc, got = _twice(run_step, dtype, n, wd, wc, None if rin else rows["r"], rcf,
                             rows["xcp"], rows["x"], rows["g"], rows.mask, 0.6, lo, hi)
            assert rc == 0
            xn, d, row = _f64(got["xn"]), _f64(got["d"]), got["row"]
            _hold(name + " xn", dtype, xn, ref["xn"], ref["S"], ref["C"], n)
            # d: one rounding of the difference of what was stored
            dT = (got["xn"] - D["x"].astype(dtype)).astype(np.float64)
            assert np.array_equal(d, dT), name
            _hold(name + " d", dtype, d, xn - D["x"], np.abs(xn) + np.abs(D["x"]), 1, n)
            free = ref["free"]
            assert 0.1 < np.mean(xn[free] == lo) and 0.1 < np.mean(xn[free] == hi)
            assert np.array_equal(xn[~free], D["xcp"][~free])
            own = sc.step_row(ws_, xn, d, D["x"], D["g"], free, lo, hi, dtype)
            assert row[0] == own["hits"], name
            assert row[3 + nws] == own["nratio"], (name, row[3 + nws], own["nratio"])
            rd = ref["d"]
            _hold_sum(name + " d'd", dtype, row[1], d * d, rd * rd, n)
            _hold_sum(name + " g'd", dtype, row[2], d * D["g"], rd * D["g"], n)
            for k in (0, nws // 2 - 1, nws - 1):
                _hold_sum(name + " w'd", dtype, row[3 + k], d * ws_[k], rd * ws_[k], (n, k))
    print("lbfgsb_step worst ratios %s: %r" % (IDS[dtype], sorted(
        (k, round(v, 3)) for k, v in _WORST.items() if k[-1] == IDS[dtype])))


# ---- the DeviceBackend methods that wrap these entries ---------------------------------
@pytest.mark.parametrize("dtype", BOTH, ids=IDS.get)
def test_one_pass_through_the_device_backend(nsol, dtype):
    """dots, reduced_gradient, subspace_direction, subspace_step with r and with rdef,
    diff_dots, projgr, count_free, project_step, truncated_step on the lattice: equal to
    the references (project_step and truncated_step: to NumpyBackend's rule)."""
    import torch
    from lbfgsb_numpy_backend import NumpyBackend
    from nsol_amd.lbfgsb_device import DeviceBackend
    be, nb = DeviceBackend(), NumpyBackend()
    n, c = 16 * 129, 6
    L, rows = _lattice_rows(dtype, n, 2 * c)
    wy, ws = rows.w(2 * c)[:c], rows.w(2 * c)[c:]
    hy, hs = [L.w(k) for k in range(c)], [L.w(k) for k in range(c, 2 * c)]
    w = hy + hs
    wc, rcf = sc.step_coefs(2 * c)
    theta = 4.0
    free = rows.mask
    assert be.dots(wy + ws, rows["y"], free) == list(sc.mdots_ref(w, L.y, L.mask, dtype)[0])
    assert be.dots(wy + ws, rows["y"]) == list(sc.mdots_ref(w, L.y, None, dtype)[0])
    r = be.reduced_gradient(rows["xcp"], rows["x"], rows["g"], theta, ws, wy, rcf[c:], rcf[:c],
                            free)
    r_ref, _ = sc.wcomb_ref(n, [L.xcp, L.x, L.g], [-theta, theta, -1.0], w, rcf, 1.0, L.mask,
                            dtype)
    assert np.array_equal(_f64(r.cpu().numpy()), r_ref)
    dsub = be.subspace_direction(r, ws, wy, wc[:c], wc[c:], theta, free)
    d_ref, _ = sc.wcomb_ref(n, [r_ref], [1.0], w, wc, 1.0 / theta, L.mask, dtype)
    assert np.array_equal(_f64(dsub.cpu().numpy()), d_ref)
    ref = sc.step_ref(w, wc, r_ref, rcf, L.xcp, L.x, L.g, L.mask, 1.0 / theta, sc.LO, sc.HI,
                      dtype)
    for rdef in (None, (rcf[:c], rcf[c:])):
        got = be.subspace_step(r if rdef is None else None, ws, wy, wc[:c], wc[c:], theta, free,
                               rows["xcp"], rows["x"], rows["g"], sc.LO, sc.HI, rdef=rdef)
        assert got is not None
        xn, hit, d, dd, gd, sd, yd, ratio = got
        assert np.array_equal(_f64(xn.cpu().numpy()), ref["xn"]), rdef is None
        assert np.array_equal(_f64(d.cpu().numpy()), ref["d"])
        assert hit == (ref["hits"] > 0) and (dd, gd) == (ref["dd"], ref["gd"])
        assert np.array_equal(yd, ref["wd"][:c]) and np.array_equal(sd, ref["wd"][c:])
        assert ratio == -ref["nratio"]
    out, dd, gd = be.diff_dots(rows["xcp"], rows["x"], rows["g"])
    o_ref, res, _ = sc.diff_dots_ref(L.xcp, L.x, L.g, dtype)
    assert np.array_equal(_f64(out.cpu().numpy()), o_ref) and [dd, gd] == res
    assert be.diff_dots(rows["xcp"], rows["x"])[2] == 0.0
    px, pg = sc.projgr_inputs(n)
    assert be.projgr(_dev(px, dtype), _dev(pg, dtype), sc.LO, sc.HI) == \
        sc.projgr_ref(px, pg, sc.LO, sc.HI, dtype)
    assert be.count_free(free) == int(sc.count_free_ref(L.mask))
    xn, hit = be.project_step(rows["xcp"], dsub, sc.LO, sc.HI, free)
    xn_ref, hit_ref = nb.project_step(L.xcp, d_ref, sc.LO, sc.HI, L.mask)
    assert np.array_equal(_f64(xn.cpu().numpy()), xn_ref) and hit == hit_ref
    # the truncated step from x (strictly inside the box) along a lattice direction
    xt = be.truncated_step(rows["x"], rows["y"], sc.LO, sc.HI, free)
    want = nb.truncated_step(sc.rounded(L.x, dtype), sc.rounded(L.y, dtype), sc.LO, sc.HI,
                             L.mask)
    err = np.abs(_f64(xt.cpu().numpy()) - want)
    assert np.all(err <= 4 * sc.unit(dtype) * (np.abs(L.x) + np.abs(L.y))), err.max()
    assert torch.cuda.is_available()
