"""CPU checks of what test_blur3_gpu.py relies on (blur3_cases.py): the float64 reference
of the one-pass periodic blur, the tap sets, the table of answering entry points, and --
the point of the module -- that the per-voxel gate is SHARP: on every (shape, tap kind,
type) the GPU module uses, each planted mistake of a kernel breaks the bound at one or
more voxels.  If one did not, a kernel with that mistake would pass on the GPU."""
import numpy as np
import pytest
from scipy import ndimage

import blur3_cases as bc
from conftest import rel_l2
from oracle import nsol_oracle as orc

DT_IDS = {np.float32: "f32", np.float64: "f64"}
# (kind, tap counts) the GPU module runs
GPU_KINDS = (("gauss_aniso", bc.NTAPS), ("sym_signed", bc.NTAPS), ("asym", bc.NTAPS),
             ("iso32", (7, 13)))
KIND_NTAPS = [(k, n) for k, counts in GPU_KINDS for n in counts]


def _outer(tz, ty, tx):
    """The dense kernel whose scipy-convention convolution is the correlation with
    (tz, ty, tx): convolve correlates with the reversed kernel."""
    return np.einsum("i,j,k->ijk", tz[::-1], ty[::-1], tx[::-1])


@pytest.mark.parametrize("kind,ntaps", [("asym", 3), ("asym", 7), ("sym_signed", 5),
                                        ("gauss_aniso", 9), ("asym", 17)])
@pytest.mark.parametrize("shape", [(3, 5, 16), (4, 7, 9), (2, 3, 5)])
def test_reference_is_the_oracles_wrap_convolution(kind, ntaps, shape):
    """Also where R >= n: several periods ((2, 3, 5) at 17 taps: R = 8)."""
    tz, ty, tx = bc.taps(kind, ntaps)
    x = np.random.default_rng(3).standard_normal(shape)
    ref = bc.reference(x, tz, ty, tx)
    assert rel_l2(ref, orc.convolve_nd(x, _outer(tz, ty, tx), "wrap")) < 1e-13
    if shape == (4, 7, 9):
        assert rel_l2(ref, ndimage.convolve(x, _outer(tz, ty, tx), mode="wrap")) < 1e-13
        assert rel_l2(ref, ndimage.correlate1d(ndimage.correlate1d(ndimage.correlate1d(
            x, tx, 2, mode="wrap"), ty, 1, mode="wrap"), tz, 0, mode="wrap")) < 1e-13


def test_reference_index_arithmetic_by_hand():
    x = np.arange(24, dtype=np.float64).reshape(2, 3, 4) ** 2
    tz, ty, tx = np.array([1., 2., 4.]), np.array([0., 1., 0.]), np.array([0., 1., 0.])
    # nz = 2, R = 1: out[z] = 1 x[z - 1] + 2 x[z] + 4 x[z + 1] = 2 x[z] + 5 x[1 - z]
    assert np.array_equal(bc.reference(x, tz, ty, tx), 2 * x + 5 * x[::-1])
    tx = np.array([3., 0., 0., 0., 0., 0., 0.])           # R = 3: out[i] = 3 x[i - 3]
    assert np.array_equal(bc.reference(x, ty, ty, tx), 3 * np.roll(x, 3, axis=2))
    assert np.array_equal(bc.magnitude(-x, -tz, ty, -tx), bc.reference(x, tz, ty, tx))


@pytest.mark.parametrize("ntaps", bc.NTAPS)
def test_gaussian_tap_sets(ntaps):
    """Same count, symmetric, different per axis in both types, one-pass fusable; and the
    axis convention stated independently: array axis a takes its EXTENT from cov[a, a]
    and its VALUES from cov[2 - a, 2 - a] (coordinates stacked z, y, x)."""
    sets = [("gauss_aniso", bc.GAUSS_ANISO[ntaps])]
    if ntaps == 13:
        sets.append(("gauss_spacing", bc.GAUSS_SPACING_13))
    for kind, (cov, sp) in sets:
        A = bc.gaussian_operator(cov, sp)
        assert A._fusable3()
        ts = bc.taps(kind, ntaps)
        assert [t.size for t in ts] == [ntaps] * 3
        spacing = np.ones(3) if sp is None else sp
        k = np.arange(-(ntaps // 2), ntaps // 2 + 1, dtype=np.float64)
        for a in range(3):
            assert np.ceil(3 * np.sqrt(cov[a, a]) / spacing[a]) == ntaps // 2
            w = np.exp(-0.5 * k * k * spacing[2 - a] ** 2 / cov[2 - a, 2 - a])
            assert np.allclose(ts[a], w / w.sum(), rtol=1e-12, atol=1e-300)
        for dtype in bc.DTYPES:
            assert bc.is_symmetric(ts, dtype) and not bc.is_iso(ts, dtype)
            c = [t.astype(dtype) for t in ts]
            assert not np.array_equal(c[0], c[1]) and not np.array_equal(c[1], c[2])


@pytest.mark.parametrize("ntaps", bc.NTAPS)
def test_synthetic_tap_sets(ntaps):
    R = ntaps // 2
    ts = bc.taps("sym_signed", ntaps)
    for dtype in bc.DTYPES:
        assert bc.is_symmetric(ts, dtype) and not bc.is_iso(ts, dtype)
        c = [t.astype(dtype) for t in ts]
        assert not np.array_equal(c[0], c[1]) and not np.array_equal(c[1], c[2])
    for t in ts:
        assert t[0] < 0 and t[R] > 0 and abs(t.sum() - 1.0) > 1e-3
    ts = bc.taps("asym", ntaps)
    for dtype in bc.DTYPES:
        assert not any(bc.is_symmetric((t,), dtype) for t in ts)
        assert not bc.is_iso(ts, dtype)
    ts = bc.taps("iso32", ntaps)
    assert bc.is_symmetric(ts, np.float32) and bc.is_symmetric(ts, np.float64)
    assert bc.is_iso(ts, np.float32) and not bc.is_iso(ts, np.float64)
    assert not np.array_equal(ts[0], ts[1]) and not np.array_equal(ts[0], ts[2])
    assert bc.taps("asym", ntaps) is bc.taps("asym", ntaps)       # cached, unchanged


def test_applies_reproduces_the_documented_table():
    f32, f64 = np.float32, np.float64
    al, tiny = (7, 66, 68), (3, 5, 16)
    ap = bc.applies
    for dtype in (f32, f64):
        for n in (1, 2, 4, 16, 19):
            for form in bc.FORMS:
                assert ap(form, dtype, al, n, True, True) is None
        for n in bc.NTAPS:
            assert ap("plain", dtype, tiny, n, True, True) == "dma"
            # asymmetric taps: the register kernels for the plain form, -2 for the others
            pp2 = 5 <= n <= (13 if dtype == f32 else 11)
            assert ap("plain", dtype, tiny, n, False, True) == ("reg_pp2" if pp2 else "reg")
            assert ap("plain", dtype, tiny, n, True, True, dma=False) == \
                ("reg_pp2" if pp2 else "reg")
            for form in bc.FORMS[1:]:
                assert ap(form, dtype, tiny, n, False, True) is None
                assert ap(form, dtype, tiny, n, True, True, dma=False) is None
    # Lanczos / loss: 5 .. 13 in float, 5 .. 9 in double (the lean pair: 11)
    for form in ("lanczos_a", "lanczos_b", "loss"):
        assert [n for n in bc.NTAPS if ap(form, f32, tiny, n, True, True)] == [5, 7, 9, 11, 13]
        assert [n for n in bc.NTAPS if ap(form, f64, tiny, n, True, True)] == [5, 7, 9]
    for form in ("lanczos_a2", "lanczos_b2"):
        assert [n for n in bc.NTAPS if ap(form, f32, tiny, n, True, True)] == [5, 7, 9, 11, 13]
        assert [n for n in bc.NTAPS if ap(form, f64, tiny, n, True, True)] == [5, 7, 9, 11]
    assert [n for n in bc.NTAPS if ap("norms", f64, tiny, n, True, True)] == list(bc.NTAPS[:6])
    assert [n for n in bc.NTAPS if ap("norms", f32, tiny, n, True, True)] == list(bc.NTAPS)
    # (15 taps in double: 164864 bytes with the two io tiles, past the 160 KiB)
    assert [n for n in bc.NTAPS if ap("axpby", f64, tiny, n, True, True)] == list(bc.NTAPS[:6])
    assert bc.dma_lds(f64, 15, 1) == 164864 and bc.dma_lds(f64, 13, 1, True) == 158464
    assert bc.dma_lds(f32, 13, 0) == 7040 * 16                # the kernel's "110 KiB"
    assert [n for n in bc.NTAPS if ap("axpby", f32, tiny, n, True, True)] == list(bc.NTAPS)
    # ragged rows: DMA from (16 + 2 ceil(R / VEC)) VEC on
    assert [bc.dma_rag_bound(f32, n) for n in bc.NTAPS] == [72, 72, 72, 72, 80, 80, 80, 80]
    assert [bc.dma_rag_bound(f64, n) for n in bc.NTAPS] == [36, 36, 40, 40, 44, 44, 48, 48]
    for dtype in (f32, f64):
        for n in bc.NTAPS:
            b = bc.dma_rag_bound(dtype, n)
            assert ap("plain", dtype, (5, 9, b + 1), n, True, True) == "dma_rag"
            assert ap("axpby", dtype, (5, 9, b + 1), n, True, True) == \
                (None if dtype == f64 and n >= 15 else "dma_rag")
            assert ap("norms", dtype, (5, 9, b + 1), n, True, True) == \
                (None if n == 17 or (dtype == f64 and n >= 15) else "dma_rag")
            assert ap("plain", dtype, (5, 9, b), n, True, False) == "dma_rag"     # off grid
            assert ap("plain", dtype, (5, 9, b - bc.vec(dtype)), n, True, False) is None
            assert ap("plain", dtype, (5, 9, b + 1), n, True, True, dma_rag=False) == \
                ap("plain", dtype, (5, 9, b + 1), n, False, True)
            assert ap("axpby", dtype, (5, 9, b + 1), n, True, True, dma_rag=False) is None
            assert ap("axpby", dtype, (5, 9, b - 1), n, True, True) is None
            for form in bc.FORMS[3:]:                       # no ragged, no off-grid form
                assert ap(form, dtype, (5, 9, b + 1), n, True, True) is None
                assert ap(form, dtype, (5, 9, b), n, True, False) is None
    # below the DMA bound: the ragged register kernel from 2 ntaps + 2 VEC on, 5 .. 13 (11)
    assert ap("plain", f32, (5, 9, 45), 13, True, True) == "reg_pp1_rag"
    assert ap("plain", f32, (5, 9, 33), 13, True, True) is None              # < 34
    assert ap("plain", f32, (5, 9, 45), 15, True, True) is None
    assert ap("plain", f32, (5, 9, 45), 3, True, True) is None
    assert ap("plain", f32, (5, 9, 81), 15, False, True) is None
    assert ap("plain", f64, (5, 9, 31), 11, False, True) == "reg_pp1_rag"
    assert ap("plain", f64, (5, 9, 31), 13, True, True) is None
    assert ap("plain", f32, (5, 9, 80), 7, False, False) is None             # off grid, asym


def test_shapes_cross_what_they_claim():
    for dtype in bc.DTYPES:
        V = bc.vec(dtype)
        for ntaps in bc.NTAPS:
            sh = bc.shapes(dtype, ntaps)
            assert all(np.prod(s) < 4e5 for s, _ in sh.values())
            (nz, ny, nx), _ = sh["tiles"]
            assert ny > bc.DMA_ROWS and nx > bc.DMA_LANES * V and nx % V == 0
            assert sorted(sh["rag%d" % r][0][2] % V for r in range(1, V)) == list(range(1, V))
            assert any(sh["rag%d" % r][0][1] == 65 for r in range(1, V))
            for r in range(1, V):
                assert bc.applies("plain", dtype, sh["rag%d" % r][0], ntaps, True, True) == \
                    "dma_rag"
                assert sh["rag%d" % r][0][2] - r == bc.dma_rag_bound(dtype, ntaps)
            assert bc.applies("plain", dtype, sh["offgrid"][0], ntaps, True, False) == "dma_rag"
            if "ragreg" in sh:
                assert bc.applies("plain", dtype, sh["ragreg"][0], ntaps, True, True) == \
                    "reg_pp1_rag"
            assert ("ragreg" in sh) == (5 <= ntaps <= (13 if V == 4 else 11))
            if ntaps >= 13:
                assert ntaps // 2 > sh["tiny"][0][0] and ntaps // 2 > sh["tiny"][0][1]
        x = bc.volume((7, 66, 68), dtype)
        assert np.array_equal(x, bc.rounded(x, dtype))
        sites = bc.spike_sites((7, 66, 68), dtype)
        assert all(abs(x[s]) >= bc.SPIKE for s in sites)
        xs = sorted(s[2] for s in sites)
        assert 0 in xs and 67 in xs and 16 * V - 1 in xs and 16 * V in xs
        assert {63, 64} <= {s[1] for s in sites}
        sites = bc.spike_sites((5, 9, 83), dtype)
        assert {80 if V == 4 else 82, 82} <= {s[2] for s in sites}


@pytest.mark.parametrize("dtype", bc.DTYPES, ids=lambda d: DT_IDS[d])
@pytest.mark.parametrize("kind,ntaps", KIND_NTAPS)
def test_the_gate_is_sharp(kind, ntaps, dtype):
    """Every planted mistake breaks |got - ref| <= C u S somewhere, with the LARGER of the
    two constants (the register kernels'), on every shape of the GPU module.  The only
    combinations without a mistake to find: reversed taps where the taps are symmetric,
    and tz / ty / tx swapped where the three sets are one set in the working type (iso32
    in float32 -- the kernel is handed equal taps)."""
    ts = bc.taps(kind, ntaps)
    cast = tuple(bc.rounded(t, dtype) for t in ts)
    u, C = bc.unit(dtype), bc.c_reg(ntaps)
    for name, (shape, _) in bc.shapes(dtype, ntaps).items():
        x = bc.volume(shape, dtype)
        ref, S = bc.reference(x, *ts), bc.magnitude(x, *ts)
        # the reference itself, and the kernel's rounded taps, are inside the gate
        assert np.all(np.abs(bc.reference(x, *cast) - ref) <= 3 * u * S)
        for m in bc.MISTAKES:
            if m.startswith("swap") and bc.is_iso(ts, dtype):
                continue
            bad = bc.mistaken(m, x, *ts)
            if bad is None:
                assert m in ("reverse_x", "reverse_z") and bc.SYMMETRIC[kind]
                continue
            worst = float(np.max(np.abs(bad - ref) / (u * S)))
            assert worst > C, "%s %s %s: mistake %s moves no voxel past %d u S (%.3g)" % (
                kind, name, shape, m, C, worst)
