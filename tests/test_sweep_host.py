"""Host-side logic of the parameter sweep (nsol_amd/parameter_sweep.py): member
order, validation, group splitting, result naming, the declared C entry points.
No GPU."""
import itertools
import os

import pytest


def test_member_order_is_itertools_product_over_the_dictionary_as_given():
    from nsol_amd.parameter_sweep import member_parameters
    params = {"alg_type": ["ALG2", "ALG3"], "alpha": [0.3, 0.01, 0.1],
              "L2": [8, 12]}
    got = member_parameters(params)
    want = [dict(zip(params.keys(), v))
            for v in itertools.product(*params.values())]
    assert got == want
    assert len(got) == 12 and list(got[0].keys()) == ["alg_type", "alpha", "L2"]
    assert got[1] == {"alg_type": "ALG2", "alpha": 0.3, "L2": 12}


def test_unknown_key_and_empty_list_raise():
    from nsol_amd.parameter_sweep import member_parameters
    with pytest.raises(ValueError, match="rho"):
        member_parameters({"alpha": [0.1], "rho": [1.0]})
    with pytest.raises(ValueError, match="iterations"):
        member_parameters({"iterations": [10, 20]})
    with pytest.raises(ValueError, match="alpha"):
        member_parameters({"alpha": []})
    with pytest.raises(ValueError):
        member_parameters({})


def test_sweep_object_lists_its_members_without_a_device():
    import numpy as np
    from nsol_amd.parameter_sweep import PrimalDualSweep
    f = lambda x, t: x
    s = PrimalDualSweep(f, f, f, f, 8, np.zeros(16),
                        parameters={"alpha": [0.1, 0.2], "alg_type": ["ALG2"]})
    assert s.get_parameters() == [{"alpha": 0.1, "alg_type": "ALG2"},
                                  {"alpha": 0.2, "alg_type": "ALG2"}]
    assert s.get_execution() is None
    with pytest.raises(ValueError):
        s.set_measures({}, every=0)


@pytest.mark.parametrize("members,group", [(15, 4), (15, 15), (15, 64), (1, 1),
                                           (64, 16), (7, 1)])
def test_groups_cover_every_member_once(members, group):
    from nsol_amd import ops
    groups = ops.sweep_groups(members, group)
    seen = [m for a, b in groups for m in range(a, b)]
    assert seen == list(range(members))
    assert all(0 < b - a <= group for a, b in groups)
    assert len(groups) == -(-members // group)


def test_group_size_follows_the_byte_budget(monkeypatch):
    from nsol_amd import ops
    n, dim, es = 1 << 16, 2, 4
    per_member = (3 + 2 * dim) * n * es
    monkeypatch.setattr(ops, "PD_SWEEP_GROUP_BYTES", 5 * per_member + 1)
    assert ops.sweep_group_size(64, n, dim, es) == 5
    assert ops.sweep_group_size(3, n, dim, es) == 3
    monkeypatch.setattr(ops, "PD_SWEEP_GROUP_BYTES", 1)
    assert ops.sweep_group_size(64, n, dim, es) == 1     # never less than one
    # all members of a group within the kernel's 2^31 voxels
    monkeypatch.setattr(ops, "PD_SWEEP_GROUP_BYTES", 1 << 62)
    assert ops.sweep_group_size(4096, 1 << 21, 3, 4) == 1024


def test_result_dir_naming():
    from nsol_amd.application.run_denoising import member_result_path as mp
    assert mp("out", "a/b/img.npy", 0.03) == os.path.join("out", "img_alpha0.03.npy")
    assert mp("out", "vol.nii.gz", 1e-3) == os.path.join("out", "vol_alpha0.001.nii.gz")
    assert mp("d/e", "x.png", 1.0) == os.path.join("d/e", "x_alpha1.png")


def test_sweep_entry_points_are_declared():
    from nsol_amd import _lib
    decl = _lib.declared_symbols()
    for base in ("pd_sweep_iter", "pd_sweep_run"):
        for suf in ("f32", "f64"):
            assert "nsol_%s_%s" % (base, suf) in decl
    assert "nsol_pd_sweep_launches" in decl
    assert "nsol_pd_sweep_entry_bytes" in decl
    # the run entry: 5 state arrays + bt, members, geometry, 4 host schedules,
    # the table (host, device, bytes), final slot, stream
    assert len(decl["nsol_pd_sweep_run_f32"][1]) == 27
