"""Combo training (`egogen_amd.train_combo`, csrc/combo.hip): the parts that need no device.  The fixture
tests/golden/combo_train_ref.npz is what the reference's own `GAMMAPrimitiveComboTrainOP` computed on the CPU
(scripts/gen_combo_golden.py); tests/combo_ref.py restates the two losses in torch and is held to it here in float64, so that
the GPU tests can use it as the float64 truth and the float32 yardstick.

EGX_COMBO_TABLE=<file>: append the measured float32-vs-float64 distances of the restatement (profiles/combo_train.md)."""
import os
import re
import runpy

import numpy as np
import pytest
import torch

from tests import combo_ref
from tests.combo_ref import CASES, evaluated
from tests.helpers import load_golden, max_abs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("egx_cont6d_to_aa_backward", "egx_primitive_loss_forward", "egx_primitive_loss_backward", "egx_primitive_reseed")
RTOL = 5e-5     # the figure the predictor / regressor training tests use for restatement-vs-reference-class comparisons


def _table(line):
    path = os.environ.get("EGX_COMBO_TABLE")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def test_new_entries_are_declared_and_bound():
    from egogen_amd import _lib
    txt = open(os.path.join(ROOT, "include", "egogen_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"#define\s+EGX_PRIMITIVE_LOSS_WS_BYTES\s+4096\b", txt)
    assert os.path.exists(os.path.join(ROOT, "egogen_amd", "csrc", "combo.hip"))


def test_train_combo_imports_nothing_from_the_oracle_and_spells_no_library_gemm():
    for fn in ("egogen_amd/train_combo.py", "exp_GAMMAPrimitive/train_GAMMACombo.py"):
        src = open(os.path.join(ROOT, fn)).read()
        assert not re.search(r"^\s*(from|import)\s+(oracle|tests)\b", src, flags=re.M) and "oracle/" not in src, fn
        # as tests/test_lib_abi.py asks of the other training operators: products run through egx_gemm3
        assert not re.search(r"torch\.(addmm|mm|bmm|baddbmm|matmul|einsum|tensordot)\(|\.addmm_\(|F\.linear\(", src), fn


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_reproduces_the_reference_class(case):
    """Loss items [REC, KLD, REG, HPOSE] and the gradient norm of every predictor parameter, rtol 5e-5; the float32 evaluation of
    the same restatement is measured against float64 for the table."""
    g = load_golden("combo_train_ref.npz")
    items, grads, _ = evaluated(case, torch.float64)
    assert [str(k) for k in g["grad_keys"]] == list(grads.keys())
    np.testing.assert_allclose(items.numpy(), g[case + "_items"], rtol=RTOL)
    for k, n in zip(grads, g[case + "_grad_norm"]):
        assert abs(float(grads[k].norm()) - n) <= RTOL * max(n, 1e-6) + 1e-9, (k, float(grads[k].norm()), n)
    i32, g32, _ = evaluated(case, torch.float32)
    d_items = np.abs(i32.numpy() - items.numpy()) / np.abs(items.numpy())
    n64 = np.array([float(v.norm()) for v in grads.values()])
    n32 = np.array([float(v.norm()) for v in g32.values()])
    d_norm = float(np.max(np.abs(n32 - n64) / np.maximum(n64, 1e-12)))
    print(f"{case}: float32 restatement vs float64: items {d_items}, max rel grad-norm distance {d_norm:.3e}")
    _table(f"| cpu float32 restatement | {case} | items rel " + " ".join(f"{v:.2e}" for v in d_items) + f" | grad norm rel {d_norm:.2e} |")
    # the gradient heads as ONE group (the fixture is a float32 evaluation: float32's own distance is its bound)
    h64, h32 = (np.stack([np.resize(v[k].flatten()[:8].numpy(), 8) for k in grads]) for v in (grads, g32))
    assert max_abs(h64, g[case + "_grad_head"]) <= combo_ref.yardstick(h64, h32)
    if case == "one":   # :1025 and :733 as the generator read them from the class: Adam over the predictor, ft_regressor unused
        assert bool(g["optimizer_over_predictor_only"]) and int(g["ft_regressor_reads"]) == 0


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_recorded_primitives(case):
    """Y_rec / Xb_rec of each primitive and, for the rollouts, the seed X and the frame (R_curr, T_curr) the class derived from the
    GENERATED body.  The fixture is the class's float32 evaluation: it may be max(5e-5 relative, 3 x the float32 restatement's own
    distance) from the float64 restatement, the bound the GPU tests give the HIP path."""
    g = load_golden("combo_train_ref.npz")
    _, _, rec = evaluated(case, torch.float32)
    _, _, rec64 = evaluated(case, torch.float64)
    if case == "one":
        for k in ("Y_rec", "Xb_rec"):
            assert max_abs(rec64[k], g["one_" + k]) <= combo_ref.yardstick(rec64[k], rec[k]), k
        return
    assert len(rec["X"]) == g[case + "_X"].shape[0] == 3
    for i in range(3):
        for k in ("R_curr", "T_curr", "X", "Y_rec", "Xb_rec"):
            bound = combo_ref.yardstick(rec64[k][i], rec[k][i])
            err = max_abs(rec64[k][i], g[f"{case}_{k}"][i])
            print(f"{case} primitive {i} {k}: |fixture - float64| {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (k, i, err, bound)
    for i in range(3):       # and in float64 the frames stay rotations about z
        R = rec64["R_curr"][i]
        assert max_abs(R @ R.transpose(1, 2), torch.eye(3, dtype=torch.float64).expand_as(R)) < 1e-12
        assert max_abs(R[:, 2], torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(R.shape[0], 3)) == 0.0


def test_use_gt_transform_is_refused():
    from egogen_amd.train_combo import GAMMAPrimitiveComboTrainOP
    with pytest.raises(NotImplementedError, match="use_gt_transform"):
        GAMMAPrimitiveComboTrainOP({"modelconfig": {}}, {"modelconfig": {}}, {}, {"use_gt_transform": True, "log_dir": "unused"})


def test_driver_parses_the_yaml_and_fails_loudly_without_a_device(tmp_path, monkeypatch):
    """exp_GAMMAPrimitive/train_GAMMACombo.py on configs in the reference's layout (crowd_ppo/cfg_samp20/MPVAECombo_samp_2frame.yml
    naming the predictor's and the regressor's yml): everything is parsed, then the operator refuses to run without a device."""
    import yaml
    from egogen_amd import _lib
    from egogen_amd.models import PREDICTOR_CFG, REGRESSOR_CFG
    cfgdir = tmp_path / "crowd_ppo" / "cfg_samp20"
    os.makedirs(cfgdir)
    combo = {"modelconfig": {"predictor_config": "MPVAE_samp20_2frame_rollout", "regressor_config": "MoshRegressor_v3_male"},
             "lossconfig": dict(combo_ref.LOSS_CFG, use_cycle=False),
             "trainconfig": {"scheduled_sampling": False, "use_gt_transform": False, "ft_regressor": False, "use_Yproj_as_seed": False,
                             "max_rollout": 8, "learning_rate": 3e-4, "batch_size": 2, "num_epochs": 2, "num_epochs_fix": 1,
                             "saving_per_X_ep": 2, "dataset_path": str(tmp_path / "data"), "subsets": ["CMU"]}}
    for name, cfg in (("MPVAECombo_samp_2frame", combo), ("MPVAE_samp20_2frame_rollout", {"modelconfig": dict(PREDICTOR_CFG)}),
                      ("MoshRegressor_v3_male", {"modelconfig": dict(REGRESSOR_CFG, gender="male")})):
        with open(cfgdir / f"{name}.yml", "w") as fh:
            yaml.safe_dump(cfg, fh)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    mod = runpy.run_path(os.path.join(ROOT, "exp_GAMMAPrimitive", "train_GAMMACombo.py"), run_name="driver_under_test")
    with pytest.raises(_lib.EgxError, match="no CPU fallback"):
        mod["main"](["--cfg", "MPVAECombo_samp_2frame"])
    for name in ("MPVAECombo_samp_2frame", "MPVAE_samp20_2frame_rollout", "MoshRegressor_v3_male"):
        assert os.path.isdir(tmp_path / "results" / "exp_GAMMAPrimitive" / name / "checkpoints")
    with pytest.raises(FileNotFoundError):
        mod["main"](["--cfg", "no_such_config"])
    combo["trainconfig"]["use_gt_transform"] = True
    with open(cfgdir / "MPVAECombo_samp_2frame.yml", "w") as fh:
        yaml.safe_dump(combo, fh)
    with pytest.raises(NotImplementedError):
        mod["main"](["--cfg", "MPVAECombo_samp_2frame"])
