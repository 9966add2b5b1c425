"""What tests/gram_cases.py claims, proved on the CPU: the lattice reference is exact and
independent of the order of summation, its magnitude bounds hold, its entries tell the
vectors apart, every fault a Gram kernel can plausibly have (a lost group, a tile counted
twice, the mask or the data of the tile staged before, a shifted or ignored mask, swapped
slots) changes it at every tile size, and expected_form is the dispatch of
nsol_lbfgsb.hip written out by hand."""
import math

import numpy as np
import pytest

import gram_cases as gc

TILES = (256, 512, 1024, 2048)      # voxels per tile of the staged kernels (TB / sizeof T)
SMALL = 3 * 65536 + 4112            # crosses the reference's own chunks


def _int_gram(rows, keep):
    a = rows[:gc.MAXVEC].astype(np.int64) * keep.astype(np.int64)
    return np.einsum("im,jm->ij", a, a), a.dot(gc.b4_of(rows[gc.MAXVEC:]))


@pytest.mark.parametrize("masked", [True, False])
def test_reference_is_integer_arithmetic_in_any_order(masked):
    rows, mask = gc.lattice(SMALL)
    for n in (16, 4112, 65536, SMALL):
        ref = gc.gram_ref(n, masked, SMALL)
        keep = mask[:n] <= 0 if masked else np.ones(n, bool)
        g, w = _int_gram(rows[:, :n], keep)
        assert np.array_equal(ref.gram, g) and np.array_equal(ref.wzb4, w), n
        assert np.array_equal(ref.wzb * 4, w)
        a = rows[:gc.MAXVEC, :n].astype(np.float64) * keep
        assert np.array_equal(a.dot(a.T), g.astype(np.float64))
        assert np.array_equal(a[:, ::-1].dot(a[:, ::-1].T), g.astype(np.float64))
        assert np.array_equal(ref.pairs(5), g[:5, :5][np.triu_indices(5)])
    n = 4112
    ref = gc.gram_ref(n, masked, SMALL)
    keep = mask[:n] <= 0 if masked else np.ones(n, bool)
    a = rows[:gc.MAXVEC, :n].astype(np.float64) * keep
    b = gc.b4_of(rows[gc.MAXVEC:, :n]).astype(np.float64) / 4.0
    for i in range(gc.MAXVEC):
        assert math.fsum((a[i] * b).tolist()) == ref.wzb[i]
        for j in range(i, gc.MAXVEC):
            assert math.fsum((a[i] * a[j]).tolist()) == float(ref.gram[i, j])


@pytest.mark.parametrize("masked", [True, False])
def test_reduced_gradient_is_exact_in_float32_in_any_order(masked):
    rows, mask = gc.lattice(SMALL)
    n = 70000
    ref = gc.gram_ref(n, masked, SMALL)
    keep = mask[:n] <= 0 if masked else np.ones(n, bool)
    for nvec in (1, 7, 24, 12):                       # (12 after 24: the cache restarts)
        want = ref.r(nvec)
        terms = [(c, rows[gc.MAXVEC + k, :n]) for k, c in enumerate(gc.BCOEF3)] + \
                [(gc.WCOEF[k], rows[k, :n]) for k in range(nvec)]
        for dt, order in ((np.float32, 1), (np.float32, -1), (np.float64, 1)):
            acc = np.zeros(n, dt)
            for c, v in terms[::order]:
                acc = acc + dt(c) * v.astype(dt)      # the kernels' multiply, then add
            got = np.where(keep, acc, dt(0))
            assert got.dtype == dt
            assert np.array_equal(got.astype(np.float64), want), (nvec, dt, order)
        assert np.all(want[~keep] == 0)


def test_the_magnitude_bounds_of_the_docstring_hold():
    rows, mask = gc.lattice()
    assert rows.shape == (27, gc.NMAX) and mask.shape == (gc.NMAX,)
    assert rows.min() == -31 and rows.max() == 31 and not np.any(rows == 0)
    assert set(np.unique(mask)) == {-128, -1, 0, 1, 2, 127}
    free = float((mask <= 0).mean())
    assert 0.58 < free < 0.62
    assert all(abs(c) <= 1 and float(8 * c).is_integer() for c in gc.WCOEF)
    assert len(gc.WCOEF) == gc.MAXVEC and 0.0 in gc.WCOEF
    assert gc.NMAX == max(gc.lengths(max(TILES)).values())
    # the largest sum of absolute values any entry can reach, and the data's own
    assert 961 * gc.NMAX < 2 ** 53 and 31 * 310 * gc.NMAX < 2 ** 53
    ref = gc.gram_ref(gc.NMAX, False)
    assert int(np.abs(ref.gram).max()) == int(ref.gram.diagonal().max()) < 2 ** 53
    assert int(np.abs(ref.wzb4).max()) < 2 ** 53
    b4 = gc.b4_of(rows[gc.MAXVEC:])
    assert np.abs(b4).max() <= 310
    # r: the sum of the absolute values of its terms bounds every partial sum
    worst = np.abs(b4).astype(np.float64) / 4 + sum(
        abs(gc.WCOEF[k]) * np.abs(rows[k]).astype(np.float64) for k in range(gc.MAXVEC))
    assert worst.max() * 8 < 2 ** 24
    assert np.abs(ref.r(gc.MAXVEC)).max() * 8 < 2 ** 24


@pytest.mark.parametrize("k", TILES)
def test_entries_at_the_fourth_partial_lengths_tell_the_vectors_apart(k):
    n = gc.lengths(k)["fourth_partial"]
    assert n == 768 * k + 16
    for masked in (True, False):
        ref = gc.gram_ref(n, masked)
        pairs = ref.pairs(gc.MAXVEC)
        assert pairs.size == 300 and np.unique(pairs).size == 300
        assert np.unique(ref.wzb).size == gc.MAXVEC          # a swapped W'Z b slot shows
        assert not np.any(np.isin(ref.wzb, pairs.astype(np.float64)))


def _mutations(k):
    """(name, rows, keep, diagonal must change) of faulty evaluations at n = 3 k + 16:
    tiles 0 .. 2 full, tile 3 holds 16 voxels."""
    n = 3 * k + 16
    rows, mask = gc.lattice(SMALL)
    rows, keep = rows[:, :n], mask[:n] <= 0
    out = [("drop the last 16-voxel group", rows[:, :n - 16], keep[:n - 16], True)]
    twice = np.concatenate([np.arange(n), np.arange(k, 2 * k)])
    out.append(("count one tile twice", rows[:, twice], keep[twice], True))
    prev = keep.copy()
    prev[2 * k:3 * k] = keep[k:2 * k]
    out.append(("the previous tile's mask for a tile", rows, prev, False))
    prev = keep.copy()
    prev[3 * k:] = keep[2 * k:2 * k + 16]
    out.append(("the previous tile's mask for the partial tile", rows, prev, False))
    # the partial tile lands in a buffer that held a full one: what lies behind its end
    stale = np.concatenate([np.arange(n), np.arange(2 * k + 16, 3 * k)])
    out.append(("the previous tile's data behind the end", rows[:, stale], keep[stale], True))
    out.append(("the mask shifted by a 16-byte piece", rows, np.roll(keep, 16), False))
    out.append(("the mask shifted by a 1 KiB piece", rows, np.roll(keep, 1024), False))
    out.append(("the mask ignored", rows, np.ones(n, bool), True))
    return n, rows, keep, out


@pytest.mark.parametrize("k", TILES)
def test_every_simulated_fault_changes_the_reference(k):
    n, rows, keep, muts = _mutations(k)
    g, w = gc.gram_of(rows, keep)
    assert np.array_equal(g, gc.gram_ref(n, True, SMALL).gram)
    for name, mrows, mkeep, diagonal in muts:
        mg, mw = gc.gram_of(mrows, mkeep)
        assert not np.array_equal(mg, g), name
        assert not np.array_equal(mw, w), name
        # not one pair block of 3 x 3 or 4 x 4 entries survives, so every nvec sees it
        for e in (3, 4):
            for i in range(0, gc.MAXVEC, e):
                for j in range(i, gc.MAXVEC, e):
                    assert not np.array_equal(mg[i:i + e, j:j + e], g[i:i + e, j:j + e]), name
        assert np.all(mw != w) or not diagonal, name
        if diagonal:
            assert np.all(mg.diagonal() != g.diagonal()), name
    # two vectors swapped, two W'Z b slots of one block swapped (the long lengths, where
    # all 300 entries differ pairwise, show more: any slot taken for any other)
    full = gc.gram_ref(gc.lengths(k)["fourth_partial"], True)
    for ref_g, ref_w in ((g, w), (full.gram, full.wzb4)):
        for i in range(gc.MAXVEC):
            for j in range(i + 1, gc.MAXVEC):
                perm = np.arange(gc.MAXVEC)
                perm[[i, j]] = [j, i]
                lead = max(j + 1, 2)
                assert not np.array_equal(ref_g[np.ix_(perm, perm)][:lead, :lead],
                                          ref_g[:lead, :lead]), (i, j)
                assert ref_w[i] != ref_w[j], (i, j)


@pytest.mark.parametrize("k", TILES)
def test_the_mask_repeats_in_no_tile_and_no_staging_piece(k):
    """The mask of a tile is not the mask of the tile before it, nor of one of the three
    that shared its LDS buffer, nor of the tile a workgroup took before (256 tiles back);
    the same for 1 KiB staging pieces."""
    _, mask = gc.lattice()
    keep = mask <= 0
    for unit in (k, 1024):
        tiles = keep[:(gc.NMAX // unit) * unit].reshape(-1, unit)
        for back in (1, 2, 3, 256, 512, 768):
            if back >= tiles.shape[0]:
                continue
            differ = (tiles[back:] != tiles[:-back]).sum(axis=1)
            assert differ.min() > unit // 4, (unit, back)
    for period in (16, 64, 256, 512, 1024, 2048, 4096, 8192):
        assert 0.3 < (keep[period:] != keep[:-period]).mean() < 0.7, period


F32, F64 = np.float32, np.float64
REG, DMA, MFMA = (gc.FORM_KNOBS[f] for f in ("register", "dma", "mfma"))
# (knobs, dtype, nvec, n, masked, rg) -> (form, TB), by hand from masked_gram_impl (the
# dma knob, rg only staged), masked_gram_dma_launch (n % VEC, n % 16 with a mask, rows ->
# TB, LDS above 160 KiB declined) and masked_gram_mfma_dispatch (nb -> TB, no RG at nb 6)
DISPATCH = [
    ((MFMA, F32, 4, 4096, True, False), (2, 8192)),
    ((MFMA, F32, 5, 4096, True, False), (2, 4096)),
    ((MFMA, F32, 9, 4096, True, False), (2, 4096)),
    ((MFMA, F32, 13, 4096, True, False), (2, 2048)),
    ((MFMA, F64, 20, 4096, True, False), (2, 2048)),
    ((MFMA, F64, 24, 4096, False, False), (2, 2048)),
    ((MFMA, F32, 1, 16, True, True), (2, 4096)),
    ((MFMA, F32, 8, 4096, True, True), (2, 4096)),
    ((MFMA, F32, 9, 4096, True, True), (2, 2048)),
    ((MFMA, F64, 20, 4096, False, True), (2, 2048)),
    ((MFMA, F32, 21, 4096, True, True), (gc.DECLINED, 0)),      # mfma: nb 6; dma: LDS
    ((MFMA, F64, 24, 4096, True, True), (gc.DECLINED, 0)),
    ((MFMA, F32, 10, 4100, False, False), (2, 4096)),           # n % 4 == 0, no mask
    ((MFMA, F32, 10, 4100, True, False), (0, 4096)),            # n % 16 != 0 with a mask
    ((MFMA, F32, 10, 4100, True, True), (gc.DECLINED, 0)),
    ((MFMA, F64, 10, 4098, False, True), (2, 2048)),            # n % 2 == 0, no mask
    ((MFMA, F32, 10, 4098, False, False), (0, 4096)),
    ((MFMA, F64, 10, 4097, False, False), (0, 4096)),
    ((DMA, F32, 4, 4096, True, False), (1, 8192)),
    ((DMA, F32, 5, 4096, True, False), (1, 4096)),
    ((DMA, F64, 12, 4096, True, False), (1, 4096)),
    ((DMA, F32, 13, 4096, False, False), (1, 2048)),
    ((DMA, F64, 24, 4096, True, False), (1, 2048)),
    ((DMA, F32, 4, 4096, True, True), (1, 4096)),               # rows 7: never 8 KiB
    ((DMA, F32, 8, 4096, True, True), (1, 4096)),               # rows 11
    ((DMA, F64, 9, 4096, True, True), (1, 2048)),               # rows 15
    ((DMA, F32, 20, 4096, True, True), (1, 2048)),
    ((DMA, F32, 21, 4096, True, True), (gc.DECLINED, 0)),       # 27 rows: 164.8 KiB
    ((DMA, F64, 23, 4096, False, True), (gc.DECLINED, 0)),
    ((DMA, F32, 7, 1023, False, False), (0, 4096)),
    ((REG, F32, 7, 4096, True, False), (0, 4096)),
    ((REG, F64, 24, 4096, False, False), (0, 4096)),
    ((REG, F32, 7, 4096, True, True), (gc.DECLINED, 0)),        # rg only on staged kernels
    ((MFMA, F32, 25, 4096, True, False), (gc.EINVAL, 0)),
    ((DMA, F64, 25, 4096, True, True), (gc.EINVAL, 0)),
    ((REG, F32, 0, 4096, True, False), (gc.EINVAL, 0)),
]


def test_expected_form_is_the_dispatch_written_out_by_hand():
    assert len(DISPATCH) >= 30
    for args, want in DISPATCH:
        assert gc.expected_form(*args) == want, args
    # the default knobs are the MFMA form's
    assert gc.DEFAULT_KNOBS == gc.FORM_KNOBS["mfma"]
    from nsol_amd import _lib
    for name, value in gc.DEFAULT_KNOBS.items():
        assert _lib.PARAM_DEFAULTS[name] == value


def test_the_launch_counter_is_declared_bound_and_knows_its_forms():
    from nsol_amd import _lib, ops
    assert "nsol_lb_gram_launches" in _lib.declared_symbols()
    assert [ops.lb_gram_launches(f) for f in (-1, 3)] == [-1, -1]
    assert all(ops.lb_gram_launches(f) >= 0 for f in gc.FORM_INDEX.values())
    assert sorted(gc.FORM_INDEX.values()) == [0, 1, 2]


def test_every_case_has_an_outcome_and_the_plans_cover_what_they_claim():
    total = 0
    for form in gc.FORM_KNOBS:
        for dtype in (F32, F64):
            classes = gc.LENGTH_CLASSES + (("ragged",) if form == "register" else ())
            for cls in classes:
                calls = gc.plan(form, dtype, cls)
                total += len(calls)
                want = gc.NVEC_ALL if cls == "fourth_partial" else gc.NVEC_SHORT
                for mode in gc.MODES:
                    assert {c[1] for c in calls if c[2] == mode} == set(want)
                ran = {c[3][0] for c in calls}
                assert ran <= {gc.FORM_INDEX[form], gc.DECLINED}, (form, cls, ran)
                assert gc.FORM_INDEX[form] in ran
                assert max(c[0] for c in calls) <= gc.NMAX
                for n, nvec, mode, (f, tb) in calls:
                    rg, masked, _ = gc.MODES[mode]
                    if f == gc.DECLINED:
                        assert rg and (form == "register" or nvec > 20 or cls == "ragged")
                    elif cls != "ragged":
                        k = gc.tile_voxels(tb, dtype)
                        base = gc.lengths(k)[cls]
                        assert n in (base, gc.unmasked_twin(base, dtype))
                        assert masked is False or n == base
    assert total > 3000


def test_lengths_reach_the_tiles_the_table_names():
    for k in TILES:
        ls = gc.lengths(k)
        w = gc.WORKGROUPS
        tiles = {c: (-(-n // k), n % k) for c, n in ls.items()}
        assert tiles["one_partial"] == (1, 16) and tiles["one_full"] == (1, 0)
        assert tiles["full_and_partial"] == (2, 16)
        assert tiles["second_partial"] == (w + 1, 16)       # workgroup 0: tiles 0, 256
        assert tiles["third_partial"][0] == 2 * w + 1 and 0 < tiles["third_partial"][1] < k
        assert tiles["fourth_partial"] == (3 * w + 1, 16)   # buffer (3 mod 3) = 0 again
        assert tiles["steady"] == (4 * w + 3, 0)
        assert all(n % 16 == 0 for n in ls.values())
        for dt in (F32, F64):
            twin = gc.unmasked_twin(ls["fourth_partial"], dt)
            assert twin % 16 != 0 and twin % (16 // np.dtype(dt).itemsize) == 0
            assert (twin - 1) // 16 == (ls["fourth_partial"] - 1) // 16


def test_numpy_dot_stays_inside_the_random_data_gate():
    """The reference side of the random-data test alone: float64 np.dot against fsum."""
    rng = np.random.default_rng(5)
    n = 768 * 256 + 16
    _, mask = gc.lattice()
    keep = mask[:n] <= 0
    for dt in (F32, F64):
        v = rng.standard_normal((4, n)).astype(dt).astype(np.float64) * keep
        for i in range(4):
            for j in range(i, 4):
                terms = v[i] * v[j]
                want = math.fsum(terms.tolist())
                gate = gc.random_gate(float(np.abs(terms).sum()), int(keep.sum()))
                assert abs(float(v[i].dot(v[j])) - want) <= gate
                assert gate < 1e-9 * np.abs(terms).sum()
