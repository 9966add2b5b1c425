"""Host side of the shifted depth-3 form (k_pd_shift3): how nsol_pd_run_* cuts a run
into leading iterations and the shifted block (pure host functions of the C ABI, no GPU),
and the register budget of every compiled instantiation."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from nsol_amd import _lib
    return _lib.load()


def _parts(lib, n, min_iters):
    lead, m = ctypes.c_int(-1), ctypes.c_int(-1)
    taken = lib.nsol_pd_run_parts(n, min_iters, ctypes.byref(lead), ctypes.byref(m))
    return taken, lead.value, m.value


@pytest.mark.parametrize("threshold", [0, 1, 4, 5, 10, 48, 61, 200, 201])
def test_run_parts(lib, threshold):
    """N = 1 .. 200: the parts sum to N; the block is 3 m + 1 iterations with m >= 1
    behind at most two leading iterations; it is taken exactly when N has reached the
    threshold (and the four iterations of the shortest block); threshold 0 = never."""
    for n in range(1, 201):
        taken, lead, m = _parts(lib, n, threshold)
        want = threshold > 0 and n >= max(threshold, 4)
        assert taken == int(want), (n, threshold)
        if want:
            assert m >= 1 and 0 <= lead <= 2 and lead == (n - 1) % 3
            assert lead + 3 * m + 1 == n
        else:
            assert (lead, m) == (n, 0)


def test_block_engages_exactly_when_flags_shape_and_knobs_allow(lib):
    """nsol_pd_shift_min_iters is what the run loop asks (pointer alignment aside): the
    threshold for a 3-D volume of whole-vector contiguous rows the tuner handles, 0 for
    the isotropic and weighted flags, ragged or pitched rows, 1-D / 2-D, small volumes
    (unless pdk_shift is 1); pdk_shift 0: never; 1: from four iterations on."""
    from nsol_amd import _lib, ops
    TV, HUB, L1 = ops.PD_REG_TV, ops.PD_REG_HUBER, ops.PD_DATA_L1
    big, small = (256, 256, 256), (20, 30, 256)
    default = _lib.PARAM_DEFAULTS["pdk_shift_min_iters"]

    def mi(shape, flags=0, esize=4, ndim=3, pitch=0):
        return lib.nsol_pd_shift_min_iters(esize, ndim, shape[0], shape[1], shape[2],
                                           flags, pitch)

    def engages(shape, n, **kw):
        return _parts(lib, n, mi(shape, **kw))[0]
    try:
        for esize in (4, 8):
            for flags in (TV, HUB, TV | L1, HUB | L1):
                assert mi(big, flags, esize) == default
        assert engages(big, default) == 1 and engages(big, default - 1) == 0
        assert mi(big, ops.PD_REG_ISOTROPIC) == 0
        assert mi(big, ops.PD_DATA_WEIGHTED) == 0
        assert mi((256, 256, 258)) == 0                  # ragged rows (float)
        assert mi((256, 256, 257), esize=8) == 0         # ragged rows (double)
        assert mi(big, pitch=260) == 0                   # rows at a pitch
        assert mi((1, 4096, 4096), ndim=2) == 0
        assert mi(small) == 0                            # below the tuner's size
        assert mi((4, 2048, 2048)) == 0                  # fewer than 8 planes
        _lib.set_param("pdk_shift_min_iters", 10)
        assert mi(big) == 10
        _lib.set_param("pdk_shift", 1)
        _lib.set_param("pdk_min_kvox", 0)
        assert mi(big) == 4 and mi(small) == 4
        assert mi(small, ops.PD_REG_ISOTROPIC) == 0 and mi((20, 30, 258)) == 0
        _lib.set_param("pdk_nw", 16)                     # no such workgroup size: no footprint
        assert mi(small) == 0
        _lib.set_param("pdk_nw", 0)
        _lib.set_param("pdk_shift", 0)
        for shape in (big, small):
            assert mi(shape) == 0
            for n in range(1, 201):
                assert _parts(lib, n, mi(shape)) == (0, n, 0)
        _lib.set_param("pdk_shift", -1)
        _lib.set_param("pdk_enable", 0)
        assert mi(big) == 0
    finally:
        _lib.reset_params()
    assert lib.nsol_pd_shift_launches() >= 0


def test_shifted_instantiations_do_not_spill(tmp_path):
    """Every compiled k_pd_shift3: no scratch memory, and within the registers of the
    occupancy its __launch_bounds__ ask for (12 waves: three per SIMD, 168 VGPRs of the
    512; 8 waves: two per SIMD, 256)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "nsol_pdk.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17",
                    "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-S",
                    "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "nsol_amd", "csrc", "nsol_pdk.hip")],
                   check=True, stderr=subprocess.DEVNULL)
    seen = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S*k_pd_shift3\S*)(.*?)\.end_amdhsa_kernel",
                         out.read_text(), re.S):
        name, body = m.group(1), m.group(2)
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        waves = int(re.search(r"k_pd_shift3I[fd]Li\d+ELi(\d+)E", name).group(1))
        seen[name] = (waves, vgpr, scratch)
        assert scratch == 0, (name, scratch)
        assert vgpr <= {12: 168, 8: 256}[waves], (name, vgpr)
    # float and double x 12 and 8 waves x TV / Huber x l2 / l1 x unit / non-unit spacing
    assert len(seen) == 32, sorted(seen)
