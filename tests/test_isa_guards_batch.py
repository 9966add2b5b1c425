"""Build-time guard on the gfx950 ISA of the image-stacked primal-dual kernels
(nsol_pdb.hip): k_pd_batch and k_pd_batch_iso have the forms of k_pd_sweep and
nothing more, none of them spills to scratch memory, and the isotropic ones keep
the IEEE division of the projection."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ASM = {}


def _assembly(tmp_path_factory, unit="pdb"):
    if unit not in _ASM:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("hipcc not available")
        out = tmp_path_factory.mktemp("isa_" + unit) / ("nsol_%s.s" % unit)
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                        "-S", "--cuda-device-only", "-o", str(out),
                        os.path.join(ROOT, "nsol_amd", "csrc", "nsol_%s.hip" % unit)],
                       check=True, stderr=subprocess.DEVNULL)
        _ASM[unit] = out.read_text()
    return _ASM[unit]


def _by_kernel(text, kernel, field):
    names = re.findall(r"\.name:\s+(\S+)", text)
    vals = re.findall(r"\.%s:\s+(\d+)" % field, text)
    assert len(names) == len(vals)
    # (the mangled name carries the length of the template's own name, which tells
    # k_pd_batch from k_pd_batch_iso)
    tag = "%d%sI" % (len(kernel), kernel)
    return {n: int(p) for n, p in zip(names, vals) if tag in n}


@pytest.mark.parametrize("kernel", ["k_pd_batch", "k_pd_batch_iso"])
def test_the_stacked_kernels_have_the_sweeps_forms_and_no_scratch(tmp_path_factory,
                                                                  kernel):
    scratch = _by_kernel(_assembly(tmp_path_factory), kernel,
                         "private_segment_fixed_size")
    # {float, double} x {16-byte vectors, ragged vectors, single elements} x
    # {64, 16 lanes along x} x {1-D, 2-D and 3-D with 1 or 2 rows per lane}
    assert len(scratch) == 2 * 3 * 2 * 5, len(scratch)
    assert not any(scratch.values()), {n: p for n, p in scratch.items() if p}
    sweep = _by_kernel(_assembly(tmp_path_factory, "pds"), "k_pd_sweep",
                       "private_segment_fixed_size")
    assert len(sweep) == len(scratch)
    # the same template arguments, one for one
    args = lambda names, k: sorted(n.split("%d%sI" % (len(k), k))[1] for n in names)
    assert args(scratch, kernel) == args(sweep, "k_pd_sweep")


def test_the_isotropic_stacked_kernels_divide_in_ieee(tmp_path_factory):
    text = _assembly(tmp_path_factory)
    seen = 0
    for m in re.finditer(r"\.amdhsa_kernel (\S*14k_pd_batch_isoI\S*)", text):
        name = m.group(1)
        body = text[text.index("\n%s:" % name):]
        body = body[:body.index("s_endpgm")]
        fix = "v_div_fixup_f32" if "k_pd_batch_isoIfLi" in name else "v_div_fixup_f64"
        assert fix in body, name
        seen += 1
    assert seen == 2 * 3 * 2 * 5


def test_the_3d_float32_two_rows_forms_stay_under_256_registers(tmp_path_factory):
    """The member offset is uniform per workgroup: the stacked kernels need no more
    vector registers than two waves per SIMD allow (DESIGN.md section 4b records the
    counts next to k_pd_fused's and k_pd_fused_iso's)."""
    text = _assembly(tmp_path_factory)
    for kernel in ("k_pd_batch", "k_pd_batch_iso"):
        vgpr = _by_kernel(text, kernel, "vgpr_count")
        # T = float, VEC = 4, LX = 64, RY = 2, NDIM = 3, whole vectors
        form = [v for n, v in vgpr.items()
                if ("%sIfLi4ELi64ELi2ELi3ELb0EEE" % kernel) in n]
        assert len(form) == 1, (kernel, sorted(vgpr))
        print(kernel, "3-D float32 two rows: VGPRs", form[0])
        assert form[0] <= 256, (kernel, form[0])


def test_the_unit_issues_no_buffer_stores():
    src = open(os.path.join(ROOT, "nsol_amd", "csrc", "nsol_pdb.hip")).read()
    assert "buffer_store" not in src
