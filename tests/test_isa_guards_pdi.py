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


def _assembly(tmp_path_factory):
    if "pdi" not in _ASM:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("hipcc not available")
        out = tmp_path_factory.mktemp("isa_pdi") / "nsol_pdi.s"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                        "-S", "--cuda-device-only", "-o", str(out),
                        os.path.join(ROOT, "nsol_amd", "csrc", "nsol_pdi.hip")],
                       check=True, stderr=subprocess.DEVNULL)
        _ASM["pdi"] = out.read_text()
    return _ASM["pdi"]


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
