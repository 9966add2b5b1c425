"""Build-time guard on the gfx950 ISA of the TGV unit (nsol_tgv.hip): no instantiation
spills to scratch memory, and the 3-D float32 whole-vector forms of k_tgv_primal_lin and
k_tgv_primal_w stay inside the 128 VGPRs DESIGN section 4i names as the unit's budget
(four waves per SIMD).  Reads the kernels' metadata only."""
import pytest

from test_isa_guards_pdw import _assembly, _by_kernel

KERNELS = ["k_tgv_dual", "k_tgv_primal", "k_tgv_primal_w", "k_tgv_primal_lin"]
# {float, double} x {16-byte vectors, ragged vectors, single elements} x {4 rows, 1 row}
# x {1-D, 2-D, 3-D}
FORMS = 2 * 3 * 2 * 3


@pytest.mark.parametrize("kernel,variants", [
    ("k_tgv_dual", 2), ("k_tgv_primal", 2), ("k_tgv_primal_w", 2), ("k_tgv_primal_lin", 1)])
def test_no_instantiation_of_the_unit_uses_scratch(tmp_path_factory, kernel, variants):
    scratch = _by_kernel(_assembly(tmp_path_factory, "tgv"), kernel,
                         "private_segment_fixed_size")
    # (variants: isotropic or not for the dual kernel, l2 or l1 for the two proxes)
    assert len(scratch) == FORMS * variants, (kernel, len(scratch))
    assert not any(scratch.values()), {n: p for n, p in scratch.items() if p}


@pytest.mark.parametrize("kernel,tail,count", [
    ("k_tgv_primal_lin", "ELi3ELb0EEE", 2),           # ROWS = 4 and 1
    ("k_tgv_primal_w", "ELi3ELb0ELb", 4),             # ... each l2 and l1
])
def test_the_3d_float32_vector_forms_fit_four_waves_per_simd(tmp_path_factory, kernel, tail,
                                                             count):
    """The counts are printed for DESIGN.md section 4j."""
    vgpr = _by_kernel(_assembly(tmp_path_factory, "tgv"), kernel, "vgpr_count")
    # T = float, VEC = 4, any ROWS, NDIM = 3, whole vectors
    form = {n: v for n, v in vgpr.items()
            if ("%sIfLi4ELi" % kernel) in n and tail in n}
    assert len(form) == count, (kernel, sorted(vgpr))
    print(kernel, "3-D float32 VEC-4: VGPRs", sorted(form.values()))
    assert max(form.values()) <= 128, form
