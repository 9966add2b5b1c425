"""Build-time guard on the gfx950 ISA of the weighted primal-dual kernels
(nsol_pdw.hip): k_pd_w and k_pd_w_iso have the forms of k_pd_batch and nothing
more, none of them spills to scratch memory, the 3-D float32 two-rows form fits two
waves per SIMD, and the float32 kernels keep the IEEE division of the weighted
l2 prox (nsol_pd_weighted.hpp)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ASM = {}
KERNELS = ["k_pd_w", "k_pd_w_iso"]


def _assembly(tmp_path_factory, unit="pdw"):
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


def _tag(kernel):
    # (the mangled name carries the length of the template's own name, which tells
    # k_pd_w from k_pd_w_iso)
    return "%d%sI" % (len(kernel), kernel)


def _by_kernel(text, kernel, field):
    names = re.findall(r"\.name:\s+(\S+)", text)
    vals = re.findall(r"\.%s:\s+(\d+)" % field, text)
    assert len(names) == len(vals)
    return {n: int(p) for n, p in zip(names, vals) if _tag(kernel) in n}


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_weighted_kernels_have_the_stacks_forms_and_no_scratch(tmp_path_factory,
                                                                   kernel):
    scratch = _by_kernel(_assembly(tmp_path_factory), kernel,
                         "private_segment_fixed_size")
    # {float, double} x {16-byte vectors, ragged vectors, single elements} x
    # {64, 16 lanes along x} x {1-D, 2-D and 3-D with 1 or 2 rows per lane}
    assert len(scratch) == 2 * 3 * 2 * 5, len(scratch)
    assert not any(scratch.values()), {n: p for n, p in scratch.items() if p}
    batch = _by_kernel(_assembly(tmp_path_factory, "pdb"), "k_pd_batch",
                       "private_segment_fixed_size")
    assert len(batch) == len(scratch)
    # the same template arguments (T, VEC, LX, RY, NDIM, RAG), one for one (what
    # follows them in the mangled name is the argument list, which has the weights)
    args = lambda names, k: sorted(n.split(_tag(k))[1].split("EEv")[0] for n in names)
    assert len(set(args(scratch, kernel))) == len(scratch)
    assert args(scratch, kernel) == args(batch, "k_pd_batch")


def test_the_3d_float32_two_rows_forms_stay_under_256_registers(tmp_path_factory):
    """One more row of weights per plane is held from the loads to the prox: the
    count is printed for DESIGN.md section 4c."""
    text = _assembly(tmp_path_factory)
    for kernel in KERNELS:
        vgpr = _by_kernel(text, kernel, "vgpr_count")
        # T = float, VEC = 4, LX = 64, RY = 2, NDIM = 3, whole vectors
        form = [v for n, v in vgpr.items()
                if ("%sIfLi4ELi64ELi2ELi3ELb0EEE" % kernel) in n]
        assert len(form) == 1, (kernel, sorted(vgpr))
        print(kernel, "3-D float32 two rows: VGPRs", form[0])
        assert form[0] <= 256, (kernel, form[0])


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_float32_kernels_divide_in_ieee(tmp_path_factory, kernel):
    """(u + t b) / (1 + t) has a denominator per voxel: a true division, not the
    product with a host-side reciprocal of the unweighted kernels.  The l2 and l1
    prox share a kernel (the loss is a uniform branch), so every float32 form
    holds the division."""
    text = _assembly(tmp_path_factory)
    seen = 0
    for m in re.finditer(r"\.amdhsa_kernel (\S*%sfLi\S*)" % _tag(kernel), text):
        name = m.group(1)
        body = text[text.index("\n%s:" % name):]
        body = body[:body.index(".amdhsa_kernel")]
        assert "v_div_fixup_f32" in body, name
        seen += 1
    assert seen == 3 * 2 * 5


def test_the_stand_alone_float32_l2_prox_divides_in_ieee(tmp_path_factory):
    text = _assembly(tmp_path_factory)
    # k_prox_w<float, false>: the l2 form
    names = [n for n in re.findall(r"\.amdhsa_kernel (\S+)", text)
             if "8k_prox_wIfLb0E" in n]
    assert len(names) == 1, names
    body = text[text.index("\n%s:" % names[0]):]
    body = body[:body.index(".amdhsa_kernel")]
    assert "v_div_fixup_f32" in body
