"""run_deconvolution --solver PDL --psf FILE: the PSF reaches the solver as
(A, A.transpose()), the refusals, and one run end to end on the device."""
import numpy as np
import pytest

PSF = np.array([[0.00, 0.05, 0.10, 0.02],
                [0.02, 0.20, 0.30, 0.05],
                [0.01, 0.10, 0.12, 0.03]])


def _observation(shape=(16, 24)):
    rng = np.random.default_rng(0)
    return 1. + rng.random(shape)


def _files(tmp_path, psf=PSF, shape=(16, 24)):
    obs, out = tmp_path / "obs.npy", tmp_path / "out.npy"
    np.save(obs, _observation(shape))
    np.save(tmp_path / "psf.npy", psf)
    return str(obs), str(tmp_path / "psf.npy"), str(out)


@pytest.mark.parametrize("rtype", ["TVL2", "HuberL2", "TGVL2"])
def test_psf_reaches_the_solver_with_its_exact_transpose(rtype):
    from nsol_amd.application import run_deconvolution as rd
    from nsol_amd.linear_operators import ConvolutionOperator
    obs = _observation()
    s = rd.build_solver(obs, np.ones(2), 1.2, rtype, "PDL", psf=PSF, dtype=np.float64)
    assert s._execution == "fused"
    A, At = s._op, s._op_adj
    assert isinstance(A, ConvolutionOperator) and isinstance(At, ConvolutionOperator)
    assert A is not At and not A.separable
    np.testing.assert_array_equal(A.kernel, PSF)                 # taps as they are
    np.testing.assert_array_equal(At.kernel, np.pad(PSF[::-1, ::-1], [(0, 0), (1, 0)]))
    # Young's bound comes from A's kernel
    assert s._A_norm2 == pytest.approx(PSF.sum() ** 2)
    # without psf: the Gaussian of blur, and the same object twice
    g = rd.build_solver(obs, np.ones(2), 1.2, rtype, "PDL", dtype=np.float64)
    assert g._op is g._op_adj and g._op.separable


def test_psf_refusals_of_build_solver():
    from nsol_amd.application import run_deconvolution as rd
    obs = _observation()
    for solver in ("PD", "ADMM"):
        with pytest.raises(ValueError, match="PDL"):
            rd.build_solver(obs, np.ones(2), 1.2, "TVL2", solver, psf=PSF)
    with pytest.raises(ValueError, match="upsample"):
        rd.build_solver(obs, np.ones(2), 1.2, "TVL2", "PDL", psf=PSF, upsample=[2, 2])
    with pytest.raises(ValueError, match="axes"):
        rd.build_solver(obs, np.ones(2), 1.2, "TVL2", "PDL", psf=PSF[0])
    with pytest.raises(ValueError, match="finite"):
        rd.build_solver(obs, np.ones(2), 1.2, "TVL2", "PDL", psf=PSF * np.nan)


@pytest.mark.parametrize("extra,needle", [
    (["--solver", "PD"], "--psf is an option of --solver PDL"),
    (["--solver", "ADMM"], "--psf is an option of --solver PDL"),
    (["--solver", "PDL", "--upsample", "2", "2"], "--psf cannot be combined with --upsample"),
    (["--solver", "PDL", "--slice-wise"], "--psf does not go with --slice-wise"),
])
def test_psf_refusals_of_the_command_line(tmp_path, capsys, extra, needle):
    from nsol_amd.application import run_deconvolution as rd
    obs, psf, out = _files(tmp_path)
    with pytest.raises(SystemExit) as e:
        rd.parse_args(["--observation", obs, "--result", out, "--psf", psf] + extra)
    assert e.value.code == 2
    err = " ".join(capsys.readouterr().err.split())
    assert needle in err


def test_help_says_that_blur_is_ignored():
    from nsol_amd.application import run_deconvolution as rd
    text = " ".join(rd.build_parser().format_help().split())
    assert "--psf FILE" in text and "ignored when --psf is given" in text


def test_psf_with_the_wrong_number_of_axes_is_a_parser_error(tmp_path, capsys):
    from nsol_amd.application import run_deconvolution as rd
    obs, psf, out = _files(tmp_path, psf=PSF[1])
    with pytest.raises(SystemExit):
        rd.main(["--observation", obs, "--result", out, "--solver", "PDL", "--psf", psf])
    assert "the PSF has 1 axes, the observation 2" in capsys.readouterr().err


@pytest.mark.gpu
def test_psf_run_end_to_end(tmp_path):
    """The tool's result is the solver's own on the same wiring, and --blur does not
    enter it."""
    from nsol_amd.application import run_deconvolution as rd
    obs, psf, out = _files(tmp_path)
    common = ["--observation", obs, "--result", out, "--solver", "PDL", "--psf", psf,
              "--iterations", "12", "--alpha", "0.05", "--dtype", "float64"]
    assert rd.main(common) == 0
    first = np.load(out)
    assert rd.main(common + ["--blur", "3.5"]) == 0
    assert np.array_equal(np.load(out), first)
    s = rd.build_solver(_observation(), np.ones(2), 1.2, "TVL2", "PDL", alpha=0.05,
                        iterations=12, psf=PSF, dtype=np.float64)
    s.run()
    assert s.get_execution() == "fused"
    assert np.array_equal(first, s.get_x().reshape(first.shape))
