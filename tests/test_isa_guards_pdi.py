"""Build-time guard on the gfx950 ISA of the isotropic primal-dual kernels
(nsol_pdi.hip): k_pd_fused_iso carries a plane of state per lane plus the lower
halo's whole dual vectors; no instantiation may spill to scratch memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ASM = {}


def _assembly(tmp_path_factory, unit="pdi"):
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


def _scratch_by_kernel(text, kernel):
    names = re.findall(r"\.name:\s+(\S+)", text)
    scratch = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(names) == len(scratch)
    # (the mangled name carries the length of the template's own name)
    tag = "%d%sI" % (len(kernel), kernel)
    return {n: int(p) for n, p in zip(names, scratch) if tag in n}


def test_no_isotropic_instantiation_uses_scratch(tmp_path_factory):
    text = _assembly(tmp_path_factory)
    names = re.findall(r"\.name:\s+(\S+)", text)
    scratch = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(names) == len(scratch)
    fused = {n: int(p) for n, p in zip(names, scratch) if "k_pd_fused_iso" in n}
    # {float, double} x {16-byte vectors, ragged vectors, single elements} x
    # {64, 16 lanes along x} x {1-D, 2-D and 3-D with 1 or 2 rows per lane}
    assert len(fused) == 2 * 3 * 2 * 5, len(fused)
    assert not any(fused.values()), {n: p for n, p in fused.items() if p}
    rest = {n: int(p) for n, p in zip(names, scratch)
            if "k_dual_step_iso" in n or "k_prox_dual_project" in n}
    assert len(rest) == 12 and not any(rest.values()), rest


def test_isotropic_kernels_use_ieee_division_and_square_root(tmp_path_factory):
    """No approximate reciprocal stands in for the projection's division: the
    float kernels scale and fix up their quotient (v_div_fixup_f32), the double
    ones likewise; the stand-alone projection is the smallest place to look."""
    text = _assembly(tmp_path_factory)
    for m in re.finditer(r"\.amdhsa_kernel (\S*k_prox_dual_project\S*)", text):
        name = m.group(1)
        body = text[text.index("\n%s:" % name):]
        body = body[:body.index("s_endpgm")]
        fix = "v_div_fixup_f32" if "IfLi" in name else "v_div_fixup_f64"
        assert fix in body, name


def test_the_new_unit_issues_no_16_byte_buffer_stores():
    """k_pd_fused_iso stores with plain vector stores, as k_pd_fused does."""
    src = open(os.path.join(ROOT, "nsol_amd", "csrc", "nsol_pdi.hip")).read() + \
        open(os.path.join(ROOT, "nsol_amd", "csrc", "nsol_pd_iso_body.hpp")).read()
    assert "buffer_store" not in src


def test_the_stacked_kernel_has_the_isotropic_kernels_forms(tmp_path_factory):
    """The shared launch path (nsol_pd_launch.hpp) instantiates for k_pd_sweep what
    its launcher struct names and nothing more."""
    sweep = _scratch_by_kernel(_assembly(tmp_path_factory, "pds"), "k_pd_sweep")
    # {float, double} x {16-byte vectors, ragged vectors, single elements} x
    # {64, 16 lanes along x} x {1-D, 2-D and 3-D with 1 or 2 rows per lane}
    assert len(sweep) == 2 * 3 * 2 * 5, len(sweep)
    assert not any(sweep.values()), {n: p for n, p in sweep.items() if p}


def test_the_anisotropic_kernel_adds_four_rows_per_lane_where_rows_are_whole(
        tmp_path_factory):
    fused = _scratch_by_kernel(_assembly(tmp_path_factory, "pd"), "k_pd_fused")
    # the five (NDIM, RY) pairs above in every access form, and 4 rows per lane in
    # 2-D and 3-D for the two forms that are not ragged:
    # {float, double} x {64, 16 lanes} x (3 forms x 5 + 2 forms x 2)
    assert len(fused) == 2 * 2 * (3 * 5 + 2 * 2), len(fused)
    assert not any(fused.values()), {n: p for n, p in fused.items() if p}
    ry4 = [n for n in fused if re.search(r"k_pd_fusedI[fd]Li\d+ELi\d+ELi4E", n)]
    assert len(ry4) == 2 * 2 * 2 * 2, len(ry4)
    assert not [n for n in ry4 if re.search(r"ELi4ELi\dELb1EEE", n)], ry4
