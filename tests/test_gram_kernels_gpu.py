"""The masked Gram pass of the L-BFGS-B backend in all three forms -- k_masked_gram
(staged through registers), k_masked_gram_dma (staged by LDS-DMA), k_masked_gram_mfma (the
products on the matrix cores), closed by k_gram_final / k_gram2_final -- against the exact
integer reference of gram_cases.py: every matrix entry, every product W'Z b and every
element of the reduced gradient must be EQUAL, in float32 and float64, because the lattice
inputs make every sum exact in any order (test_gram_kernels_host.py proves that, and that
the faults these lengths aim at would change the reference).

The C entries are called through ctypes so that odd vector counts are reachable, at the
lengths where a triple-buffered, tiled kernel can go wrong (gram_cases.lengths), in five
modes (with and without the reduced gradient, a mask, r_out).  Which kernel took a call is
asserted through nsol_lb_gram_launches; a call no kernel of the form takes must return -2
and launch nothing.  The arrays are views [:n] of longer allocations whose remainder holds
NaN, r_out has sentinels behind its end, every call is made twice (same bits).  Non-finite
values at variables that are not free must leave no trace; at a free one, exactly the
entries of that vector.  One random-data case per form closes with a per-entry gate that
holds for any order of summation (gram_cases.random_gate).
"""
import ctypes
import functools
import math

import numpy as np
import pytest

import gram_cases as gc

pytestmark = pytest.mark.gpu

BOTH = [np.float32, np.float64]
FORMS = ["register", "dma", "mfma"]
SLACK = 4096                        # poisoned elements behind the longest array
SENTINEL = 12345.0
GUARD = 64                          # sentinels behind r_out[n]


@pytest.fixture(scope="module")
def nsol():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nsol_amd
    from nsol_amd import _lib
    _lib.load()
    return nsol_amd


def _suffix(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def _fn(name, dtype):
    from nsol_amd import _lib
    return getattr(_lib.load(), "nsol_%s_%s" % (name, _suffix(dtype)))


def _stream():
    from nsol_amd.device import stream_ptr
    return stream_ptr()


def _counters():
    from nsol_amd import ops
    return [ops.lb_gram_launches(f) for f in range(3)]


class _Device(object):
    """The 24 vectors, the three base vectors and the mask on the device: a clean master
    copy of the longest problem and a working copy, of which a call sees the views [:n];
    what lies behind n is NaN (mask: 0, free)."""

    def __init__(self, dtype):
        import torch
        from nsol_amd import _lib
        rows, mask = gc.lattice()
        self.dtype = dtype
        self.td = torch.float32 if dtype == np.float32 else torch.float64
        self.master = torch.empty((27, gc.NMAX), dtype=self.td, device="cuda")
        for k in range(27):
            self.master[k].copy_(torch.from_numpy(rows[k].astype(dtype)))
        self.mask_master = torch.from_numpy(np.array(mask)).cuda()
        self.work = torch.empty((27, gc.NMAX + SLACK), dtype=self.td, device="cuda")
        self.mask = torch.empty(gc.NMAX + SLACK, dtype=torch.int8, device="cuda")
        ws = int(_lib.load().nsol_lb_gram_ws_doubles())
        self.ws = torch.zeros(ws, dtype=torch.float64, device="cuda")
        self.res = [torch.empty(gc.MAXVEC * (gc.MAXVEC + 1) // 2 + gc.MAXVEC,
                                dtype=torch.float64, device="cuda") for _ in range(2)]
        self.r = [torch.empty(gc.NMAX + GUARD, dtype=self.td, device="cuda")
                  for _ in range(2)]
        assert self.work.data_ptr() % 16 == 0 and self.mask.data_ptr() % 16 == 0
        assert (gc.NMAX + SLACK) * self.work.element_size() % 16 == 0
        self.n = None

    def prepare(self, n, data=None, mask=None):
        """Lattice data (or data [27, n] / mask [n] given on the host) in [:n], poison
        behind."""
        import torch
        if data is None:
            self.work[:, :gc.NMAX].copy_(self.master)
        else:
            self.work[:, :n].copy_(torch.from_numpy(data))
        self.work[:, n:] = float("nan")
        if mask is None:
            self.mask[:gc.NMAX].copy_(self.mask_master)
        else:
            self.mask[:n].copy_(torch.from_numpy(mask))
        self.mask[n:] = 0
        self.n = n

    def plant(self, row, index, value):
        self.work[row, index] = value

    def call(self, nvec, mode, which=0, bcoef=gc.BCOEF3, wcoef=gc.WCOEF):
        """One call of the C entry; (rc, counter deltas)."""
        import torch
        rg, masked, want_r = gc.MODES[mode]
        n = self.n
        res, r = self.res[which], self.r[which]
        res.fill_(SENTINEL)
        r[:n + GUARD].fill_(SENTINEL)
        ptrs = (ctypes.c_void_p * nvec)(*[self.work[k].data_ptr() for k in range(nvec)])
        iw = self.mask.data_ptr() if masked else None
        torch.cuda.synchronize()
        before = _counters()
        if rg:
            base = (ctypes.c_void_p * 3)(*[self.work[gc.MAXVEC + k].data_ptr()
                                           for k in range(3)])
            bco = np.array(bcoef, dtype=np.float64)
            wco = np.array(wcoef[:nvec], dtype=np.float64)
            rc = _fn("lb_masked_gram_rgrad", self.dtype)(
                ptrs, nvec, iw, n, res.data_ptr(), self.ws.data_ptr(), base,
                bco.ctypes.data, wco.ctypes.data, r.data_ptr() if want_r else None,
                _stream())
        else:
            rc = _fn("lb_masked_gram", self.dtype)(
                ptrs, nvec, iw, n, res.data_ptr(), self.ws.data_ptr(), _stream())
        torch.cuda.synchronize()
        after = _counters()
        return rc, [a - b for a, b in zip(after, before)]

    def results(self, nvec, mode, which=0):
        """(pairs, W'Z b or None, r_out [n + GUARD] or None) on the host, as float64."""
        rg, _, want_r = gc.MODES[mode]
        npairs = nvec * (nvec + 1) // 2
        flat = self.res[which].cpu().numpy()
        used = npairs + (nvec if rg else 0)
        assert np.all(flat[used:] == SENTINEL), "result written behind its end"
        r = None
        if rg and want_r:
            r = self.r[which][:self.n + GUARD].cpu().numpy().astype(np.float64)
        return flat[:npairs], (flat[npairs:used] if rg else None), r


@functools.lru_cache(maxsize=1)
def _device(dtype):
    # one dtype's arrays at a time (the float64 set is about 1 GB)
    import torch
    torch.cuda.empty_cache()
    return _Device(dtype)


def _set_form(form):
    from nsol_amd import _lib
    for name, value in gc.FORM_KNOBS[form].items():
        _lib.set_param(name, value)


def _check_outcome(rc, delta, want_form, label):
    if want_form == gc.DECLINED:
        assert rc == -2 and delta == [0, 0, 0], label
        return False
    assert rc == 0, label
    assert delta == [int(f == want_form) for f in range(3)], label
    return True


def _run_plan(dev, form, dtype, cls):
    import torch
    calls = gc.plan(form, dtype, cls)
    assert calls
    ran, dev.n = 0, None                 # whatever an earlier test left in the arrays
    for n, nvec, mode, (want_form, tb) in calls:
        label = (form, _suffix(dtype), cls, n, nvec, mode)
        if dev.n != n:
            dev.prepare(n)
        rg, masked, want_r = gc.MODES[mode]
        rc, delta = dev.call(nvec, mode, 0)
        if not _check_outcome(rc, delta, want_form, label):
            assert torch.all(dev.res[0] == SENTINEL), label      # nothing written either
            continue
        ran += 1
        ref = gc.gram_ref(n, masked)
        pairs, wzb, r = dev.results(nvec, mode, 0)
        assert np.array_equal(pairs, ref.pairs(nvec).astype(np.float64)), label
        if rg:
            assert np.array_equal(wzb, ref.wzb[:nvec]), label
        if r is not None:
            assert np.array_equal(r[:n], ref.r(nvec)), label
            assert np.all(r[n:] == SENTINEL), label
        # again: the same bits
        rc, delta = dev.call(nvec, mode, 1)
        _check_outcome(rc, delta, want_form, label)
        assert torch.equal(dev.res[0], dev.res[1]), label
        if r is not None:
            assert torch.equal(dev.r[0][:n + GUARD], dev.r[1][:n + GUARD]), label
    return ran


@pytest.mark.parametrize("cls", gc.LENGTH_CLASSES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", BOTH)          # slowest: one dtype's arrays at a time
def test_gram_forms_equal_the_integer_reference(nsol, form, dtype, cls):
    """Every call of gram_cases.plan(form, dtype, length class): return code and launch
    counters as expected_form says, all entries, products and the reduced gradient equal
    to the reference, sentinels intact, a second run bit for bit the first."""
    dev = _device(dtype)
    _set_form(form)
    assert _run_plan(dev, form, dtype, cls) > 0


@pytest.mark.parametrize("dtype", BOTH)
def test_register_form_at_lengths_no_vector_load_divides(nsol, dtype):
    """n in {1, 5, 1023, 1025, 4097}: the element-wise tail of k_masked_gram's staging;
    with the reduced gradient asked for, declined."""
    dev = _device(dtype)
    _set_form("register")
    assert _run_plan(dev, "register", dtype, "ragged") > 0
    # the default knobs send these lengths to the same kernel
    _set_form("mfma")
    dev.prepare(1023)
    rc, delta = dev.call(7, "gram_masked")
    assert rc == 0 and delta == [1, 0, 0]
    pairs, _, _ = dev.results(7, "gram_masked")
    assert np.array_equal(pairs, gc.gram_ref(1023, True).pairs(7).astype(np.float64))


def _nonfinite_length(form, dtype, nvec):
    """A full tile and a partial one of the largest tile the form uses for nvec vectors
    (several tiles and a partial one for the smaller tile)."""
    ks = [gc.tile_voxels(tb, dtype) for rg in (False, True)
          for f, tb in [gc.expected_form(gc.FORM_KNOBS[form], dtype, nvec, 16, True, rg)]
          if tb]
    return gc.lengths(max(ks))["full_and_partial"]


NONFINITE = (float("nan"), float("inf"), float("-inf"))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", BOTH)
def test_nonfinite_values_at_variables_that_are_not_free_leave_no_trace(nsol, form, dtype):
    """NaN, +Inf and -Inf in two stored vectors of different pair blocks and in a base
    vector, at variables that are not free (the first, a middle one, one in the partial
    last tile): every result equals the clean reference and r_out is 0 there.

    Before the fix of k_masked_gram_dma this failed for that form alone, with and without
    the reduced gradient: it selected the a side of a product only, and a NaN on the b
    side or in the base vectors met the zero as fma(0, NaN)."""
    nvec = 10
    n = _nonfinite_length(form, dtype, nvec)
    dev = _device(dtype)
    _set_form(form)
    dev.prepare(n)
    _, mask = gc.lattice()
    bound = np.flatnonzero(mask[:n] > 0)
    spots = [int(bound[0]), int(bound[bound.size // 2]), int(bound[-1])]
    assert spots[2] >= n - 16, "no variable at a bound in the partial tile"
    for shift, row in enumerate((1, 6, gc.MAXVEC + 1)):     # blocks 0 / 1 (4 x 4), 0 / 2 (3 x 3)
        for s, spot in enumerate(spots):
            dev.plant(row, spot, NONFINITE[(s + shift) % 3])
    ref = gc.gram_ref(n, True)
    for mode in ("gram_masked", "rg_r", "rg_no_r"):
        rg = gc.MODES[mode][0]
        want_form, _ = gc.expected_form(gc.FORM_KNOBS[form], dtype, nvec, n, True, rg)
        rc, delta = dev.call(nvec, mode)
        label = (form, _suffix(dtype), mode)
        if not _check_outcome(rc, delta, want_form, label):
            assert form == "register" and rg
            continue
        pairs, wzb, r = dev.results(nvec, mode)
        assert np.array_equal(pairs, ref.pairs(nvec).astype(np.float64)), label
        if rg:
            assert np.array_equal(wzb, ref.wzb[:nvec]), label
        if r is not None:
            assert np.all(r[spots] == 0.0), label
            assert np.array_equal(r[:n], ref.r(nvec)), label
            assert np.all(r[n:] == SENTINEL), label


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", BOTH)
def test_a_nan_at_a_free_variable_reaches_its_own_entries_only(nsol, form, dtype):
    """NaN in vector 5 at one free variable (in the partial last tile): row / column 5 of
    the matrix and W'Z b[5] are NaN, every other entry equals the reference, and r_out is
    NaN at that variable only."""
    nvec, k = 10, 5
    n = _nonfinite_length(form, dtype, nvec)
    dev = _device(dtype)
    _set_form(form)
    dev.prepare(n)
    _, mask = gc.lattice()
    spot = int(np.flatnonzero(mask[:n] <= 0)[-1])
    assert spot >= n - 16
    dev.plant(k, spot, float("nan"))
    ref = gc.gram_ref(n, True)
    iu = np.triu_indices(nvec)
    hit = (iu[0] == k) | (iu[1] == k)
    for mode in ("gram_masked", "rg_r", "rg_no_r"):
        rg = gc.MODES[mode][0]
        want_form, _ = gc.expected_form(gc.FORM_KNOBS[form], dtype, nvec, n, True, rg)
        rc, delta = dev.call(nvec, mode)
        label = (form, _suffix(dtype), mode)
        if not _check_outcome(rc, delta, want_form, label):
            assert form == "register" and rg
            continue
        pairs, wzb, r = dev.results(nvec, mode)
        assert np.array_equal(np.isnan(pairs), hit), label
        assert np.array_equal(pairs[~hit], ref.pairs(nvec).astype(np.float64)[~hit]), label
        if rg:
            assert np.array_equal(np.isnan(wzb), np.arange(nvec) == k), label
            assert np.array_equal(np.delete(wzb, k), np.delete(ref.wzb[:nvec], k)), label
        if r is not None:
            want = ref.r(nvec)
            assert np.isnan(r[spot]) and np.isnan(r[:n]).sum() == 1, label
            assert np.array_equal(np.delete(r[:n], spot), np.delete(want, spot)), label
            assert np.all(r[n:] == SENTINEL), label


# ---- random data ---------------------------------------------------------------------
RANDOM_NVEC = 20
RANDOM_BCOEF = (-0.83, 0.83, -1.0)
RANDOM_WCOEF = tuple(np.linspace(-0.7, 0.9, RANDOM_NVEC))


@functools.lru_cache(maxsize=None)
def _random_case(dtype, n):
    """(data [27, n], mask [n], fsum of every pair's terms, sum of their magnitudes,
    number of free variables): computed once per (dtype, n), shared by the forms."""
    rng = np.random.default_rng(n)
    data = rng.standard_normal((27, n)).astype(dtype)
    mask = np.array(gc.lattice()[1][:n])
    keep = mask <= 0
    a = data[:RANDOM_NVEC, keep].astype(np.float64)      # the masked terms are exact zeros
    iu = np.triu_indices(RANDOM_NVEC)
    exact, mag = np.empty(iu[0].size), np.empty(iu[0].size)
    for e, (i, j) in enumerate(zip(*iu)):
        terms = a[i] * a[j]
        exact[e] = math.fsum(terms.tolist())
        mag[e] = np.abs(terms).sum()
    return data, mask, exact, mag, int(keep.sum())


@pytest.mark.parametrize("rg", [False, True])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", BOTH)
def test_random_data_within_the_bound_of_any_summation_order(nsol, form, dtype, rg):
    """Normal random data, 20 vectors, the fourth_partial length of the kernel that runs:
    per entry |got - fsum(terms)| <= (kept + 2) 2^-53 sum |terms|  (gram_cases.random_gate;
    scaled per entry, not by the largest of the matrix), and r_out bit for bit
    nsol_lb_wcomb_*'s."""
    import torch
    knobs = gc.FORM_KNOBS[form]
    want_form, tb = gc.expected_form(knobs, dtype, RANDOM_NVEC, 16, True, rg)
    n = gc.lengths(gc.tile_voxels(tb if tb else 2048, dtype))["fourth_partial"]
    assert gc.expected_form(knobs, dtype, RANDOM_NVEC, n, True, rg)[0] == want_form
    data, mask, exact, mag, kept = _random_case(dtype, n)
    dev = _device(dtype)
    _set_form(form)
    dev.prepare(n, data, mask)
    mode = "rg_r" if rg else "gram_masked"
    rc, delta = dev.call(RANDOM_NVEC, mode, 0, RANDOM_BCOEF, RANDOM_WCOEF)
    label = (form, _suffix(dtype), rg, n)
    if not _check_outcome(rc, delta, want_form, label):
        assert form == "register" and rg
        return
    pairs, wzb, r = dev.results(RANDOM_NVEC, mode)
    err = np.abs(pairs - exact)
    gate = gc.random_gate(mag, kept)
    worst = int(np.argmax(err / gate))
    print("gram random %s: worst |err| / gate = %.2e (entry %d)"
          % (label, err[worst] / gate[worst], worst))
    assert np.all(err <= gate), label
    if rg:
        assert np.all(np.isfinite(wzb)), label
        nv = RANDOM_NVEC
        ptrs = (ctypes.c_void_p * nv)(*[dev.work[k].data_ptr() for k in range(nv)])
        base = (ctypes.c_void_p * 3)(*[dev.work[gc.MAXVEC + k].data_ptr() for k in range(3)])
        bco = np.array(RANDOM_BCOEF, dtype=np.float64)
        wco = np.array(RANDOM_WCOEF, dtype=np.float64)
        out = dev.r[1]
        out[:n + GUARD].fill_(SENTINEL)
        rc = _fn("lb_wcomb", dtype)(out.data_ptr(), n, dev.mask.data_ptr(), 1.0, 3, base,
                                    bco.ctypes.data, nv, ptrs, wco.ctypes.data, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(dev.r[0][:n + GUARD], out[:n + GUARD]), label
        assert np.all(r[n:] == SENTINEL), label
