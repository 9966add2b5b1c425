"""Build-time guard on the gfx950 ISA of the member-stacked kernels of the primal-dual
iteration with the data term behind a linear operator (nsol_pdls.hip): k_pdl_stack and
k_pdl_stack_iso have the forms of k_pd_batch and nothing more, none of them spills to
scratch memory, and the 3-D float32 two-rows form needs no more registers than the
weighted kernel's (the yardstick of the single-volume k_pd_lin).  Kernel metadata only."""
import pytest

from test_isa_guards_pdw import _assembly, _by_kernel, _tag

KERNELS = ["k_pdl_stack", "k_pdl_stack_iso"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_stacked_linear_kernels_have_the_stacks_forms_and_no_scratch(
        tmp_path_factory, kernel):
    scratch = _by_kernel(_assembly(tmp_path_factory, "pdls"), kernel,
                         "private_segment_fixed_size")
    # {float, double} x {16-byte vectors, ragged vectors, single elements} x
    # {64, 16 lanes along x} x {1-D, 2-D and 3-D with 1 or 2 rows per lane}
    assert len(scratch) == 2 * 3 * 2 * 5, len(scratch)
    assert not any(scratch.values()), {n: p for n, p in scratch.items() if p}
    batch = _by_kernel(_assembly(tmp_path_factory, "pdb"), "k_pd_batch",
                       "private_segment_fixed_size")
    assert len(batch) == len(scratch)
    args = lambda names, k: sorted(n.split(_tag(k))[1].split("EEv")[0] for n in names)
    assert len(set(args(scratch, kernel))) == len(scratch)
    assert args(scratch, kernel) == args(batch, "k_pd_batch")


def test_the_stacked_update_of_q_has_four_forms_and_no_scratch(tmp_path_factory):
    scratch = _by_kernel(_assembly(tmp_path_factory, "pdls"), "k_pdl_dual_data_stack",
                         "private_segment_fixed_size")
    assert len(scratch) == 2 * 2, sorted(scratch)        # {float, double} x {l2, l1}
    assert not any(scratch.values())


@pytest.mark.parametrize("kernel, weighted", [("k_pdl_stack", "k_pd_w"),
                                              ("k_pdl_stack_iso", "k_pd_w_iso")])
def test_the_3d_float32_two_rows_form_needs_no_more_registers_than_the_weighted(
        tmp_path_factory, kernel, weighted):
    def form(unit, name):
        vgpr = _by_kernel(_assembly(tmp_path_factory, unit), name, "vgpr_count")
        # T = float, VEC = 4, LX = 64, RY = 2, NDIM = 3, whole vectors
        hit = [v for n, v in vgpr.items()
               if ("%sIfLi4ELi64ELi2ELi3ELb0EEE" % name) in n]
        assert len(hit) == 1, (name, sorted(vgpr))
        return hit[0]
    lin, wgt = form("pdls", kernel), form("pdw", weighted)
    print(kernel, "3-D float32 two rows: VGPRs", lin, "--", weighted, wgt)
    assert lin <= wgt, (lin, wgt)
