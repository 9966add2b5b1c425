"""Build-time guard on the gfx950 ISA of k_tgv_primal_lin_stack (nsol_tgv.hip), the
member-stacked LIN form of the TGV primal step: every instantiation is there, none spills
to scratch memory, and the 3-D float32 whole-vector forms stay inside the 128 VGPRs DESIGN
section 4i names as the unit's budget (four waves per SIMD).  Reads the kernels' metadata
only."""
from test_isa_guards_pdw import _assembly, _by_kernel
from test_isa_guards_tgv import FORMS

KERNEL = "k_tgv_primal_lin_stack"


def test_every_instantiation_is_there_and_none_uses_scratch(tmp_path_factory):
    scratch = _by_kernel(_assembly(tmp_path_factory, "tgv"), KERNEL,
                         "private_segment_fixed_size")
    # {float, double} x {16-byte vectors, ragged vectors, single elements} x {4 rows, 1
    # row} x {1-D, 2-D, 3-D}; the LIN form has no l1 variant
    assert FORMS == 36 and len(scratch) == FORMS, len(scratch)
    assert not any(scratch.values()), {n: p for n, p in scratch.items() if p}
    # one stacked form for every single one, by template arguments
    single = _by_kernel(_assembly(tmp_path_factory, "tgv"), "k_tgv_primal_lin",
                        "private_segment_fixed_size")
    args = lambda names, k: sorted(n.split("%d%sI" % (len(k), k))[1].split("EEv")[0]
                                   for n in names)
    assert args(scratch, KERNEL) == args(single, "k_tgv_primal_lin")


def test_the_3d_float32_vector_forms_fit_four_waves_per_simd(tmp_path_factory):
    """The counts are printed for DESIGN.md section 4l, beside the single kernel's."""
    text = _assembly(tmp_path_factory, "tgv")
    counts = {}
    for kernel in (KERNEL, "k_tgv_primal_lin"):
        vgpr = _by_kernel(text, kernel, "vgpr_count")
        # T = float, VEC = 4, ROWS = 4 and 1, NDIM = 3, whole vectors
        form = {n: v for n, v in vgpr.items()
                if ("%sIfLi4ELi" % kernel) in n and "ELi3ELb0EEE" in n}
        assert len(form) == 2, (kernel, sorted(vgpr))
        counts[kernel] = sorted(form.values())
        print(kernel, "3-D float32 VEC-4: VGPRs", counts[kernel])
    assert max(counts[KERNEL]) <= 128, counts
