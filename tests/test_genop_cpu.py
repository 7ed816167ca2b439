"""CPU checks of the generation operator's specification (no GPU):

  1. tests/genop_ref.py::generate in float32 reproduces what the reference's own `GAMMAPrimitiveComboGenOP.generate` returned
     (tests/golden/genop_ref.npz, scripts/gen_genop_golden.py), and `_blend_params` is the reference's;
  2. tests/genop_ref.py::chain in float32, started from the reset state of tests/golden/env_step_ref.npz with the recorded z,
     reproduces every scene-independent quantity the reference's own `CrowdEnv.step` produced over consecutive steps - so the
     restatement, and with it the specification of the kernel egx_primitive_advance, is the reference's step;
  3. the pickle `generate_primitive_to_files` writes has the reference's keys, container types, dtypes and shapes (the operator
     driven through a CPU stand-in for the model).

Bars: the project's 1e-4 |ref| + 2e-5 (the `unit` / `m` floors of tests/test_env_reference_goldens.py); rotations are compared
as matrices."""
import json
import pickle
import types

import numpy as np
import pytest
import torch

from tests import genop_ref
from tests.helpers import load_golden, rebuild_state_dict, seeded_prior_state_dict

TOL, FLOOR = 1e-4, 2e-5


def _close(a, b, what):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    d = np.abs(a - b)
    bad = d > TOL * np.abs(b) + FLOOR
    assert not bad.any(), f"{what}: {int(bad.sum())} of {d.size} outside 1e-4 |ref| + {FLOOR:g}; worst |d| {d.max():.3e}"


def _aa_close(a, b, what):
    from oracle.rot import tgm_angle_axis_to_rotation_matrix as aa2R
    f = lambda x: torch.as_tensor(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, np.float32)).reshape(-1, 3)
    _close(aa2R(f(a)), aa2R(f(b)), what)


def _params_close(got, ref, what):
    """[...,93] body parameters: transl and pose entries directly, the global orientation as a matrix."""
    got, ref = np.asarray(got), np.asarray(ref)
    _close(got[..., :3], ref[..., :3], what + " transl")
    _aa_close(got[..., 3:6], ref[..., 3:6], what + " glorot")
    _close(got[..., 6:], ref[..., 6:], what + " pose")


@pytest.fixture(scope="module")
def gen_fixture():
    g = load_golden("genop_ref.npz")
    sd = rebuild_state_dict(g, [int(g["pred_seed"]), int(g["reg_seed"])], ["predictor.", "regressor."],
                            gains=[float(g["pred_gain"]), float(g["reg_gain"])])
    return g, sd


@pytest.mark.parametrize("tag,n_gens", [("gen3", -1), ("gen4", 4)])
def test_generate_restatement_matches_reference_execution(gen_fixture, tag, n_gens):
    g, sd = gen_fixture
    args = (sd, g[tag + "_data"], g[tag + "_bparams"], g[tag + "_betas"])
    Y, Yb = genop_ref.generate(*args, n_gens=n_gens, param_blending=True, t_his=2, z=g[tag + "_z"], dtype=torch.float32)
    _, Yb_nb = genop_ref.generate(*args, n_gens=n_gens, param_blending=False, t_his=2, z=g[tag + "_z"], dtype=torch.float32)
    assert Y.shape == g[tag + "_Y"].shape == (3 if n_gens < 0 else 4, 20, 201)
    _close(Y, g[tag + "_Y"], tag + " Y")
    _params_close(Yb, g[tag + "_Yb"], tag + " Yb")
    _params_close(Yb_nb, g[tag + "_Yb_noblend"], tag + " Yb without blending")
    # the seed frames pass through untouched, and blending changes frames 2 and 3 of the pose part only
    seed = np.tile(g[tag + "_data"][:2, :, :201], (1, max(n_gens, 1), 1))
    assert np.array_equal(Y[:, :2].numpy(), seed.transpose(1, 0, 2)) and np.array_equal(g[tag + "_Y"][:, :2], seed.transpose(1, 0, 2))
    ref, ref_nb = g[tag + "_Yb"], g[tag + "_Yb_noblend"]
    same = np.ones(20, bool)
    same[2:4] = False
    assert np.array_equal(ref[:, same], ref_nb[:, same]) and np.array_equal(ref[:, :, :6], ref_nb[:, :, :6])
    assert not np.array_equal(ref[:, 2:4, 6:], ref_nb[:, 2:4, 6:])


def test_blend_params_restatement_is_the_reference(gen_fixture):
    from oracle.env import blend_params
    g, _ = gen_fixture
    x = torch.as_tensor(g["blend_in"]).clone()
    out = blend_params(x, 2)
    assert out is x and np.array_equal(out.numpy(), g["blend_out"])


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,n", [("free", 3), ("pene", 2)])
def test_chain_restatement_is_the_reference_step(case, n):
    from egogen_amd import synth
    from oracle.smplx_lbs import BodyModel
    g = load_golden("env_step_ref.npz")
    pre = case + "_"
    assert int(g[pre + "n_steps"]) == n and int(g["body_model_seed"]) == 0
    sd = seeded_prior_state_dict(int(g["prior_seed"]), *[float(v) for v in g["prior_gains"]])
    rf = float(json.loads(str(g["cfg_json"]))["modelconfig"]["reproj_factor"])
    bm = BodyModel(synth.make_body_model(0), dtype=torch.float32)
    z = torch.as_tensor(g[pre + "z"][:n]).reshape(n, 1, 128)
    steps = genop_ref.chain(sd, bm, synth.marker_ids(), g[pre + "reset_state"][None, :, :201], g[pre + "reset_seed"][None],
                            g[pre + "reset_R0"].reshape(1, 3, 3), g[pre + "reset_T0"].reshape(1, 3), g[pre + "betas"].reshape(1, 10),
                            z, rf)
    for i, r in enumerate(steps):
        sp = f"{pre}s{i}_"
        _close(r["Y_gen"][:, 0], g[sp + "Y_gen"], sp + "Y_gen")
        _params_close(r["pred_params"][0], g[sp + "pred_params"], sp + "pred_params")
        _close(r["joints"][0], g[sp + "joints"], sp + "joints")
        _close(r["marker_b"][0], g[sp + "marker_b"], sp + "marker_b")
        _params_close(r["seed_params"][0], g[sp + "after_seed"], sp + "after_seed")
        _close(r["R0"][0], g[sp + "after_R0"], sp + "after_R0")
        _close(r["T0"][0].reshape(-1), g[sp + "after_T0"].reshape(-1), sp + "after_T0")
        _close(r["seed_markers"][0], g[sp + "after_state"][:, :201], sp + "marker seed")


# ----------------------------------------------------------------------------------------------------------------------
class _CpuPrior:
    """Stand-in for GAMMAPrimitiveCombo on the CPU: `sample_prior` through the oracle's networks."""

    def __init__(self, sd):
        self.sd = sd
        self.predictor = types.SimpleNamespace(z_dim=128)

    def sample_prior(self, X, betas, z=None):
        from oracle import nets
        return nets.sample_prior(self.sd, X, betas[None].repeat(18, 1, 1), z)


class _Batcher:
    amass_subset_name = ["synthetic"]

    def __init__(self, items):
        self.items, self.i = items, 0

    def next_sequence(self):
        self.i += 1
        return self.items[self.i - 1]


def test_generate_primitive_to_files_layout(gen_fixture, tmp_path):
    from egogen_amd.genop import GAMMAPrimitiveComboGenOP
    g, sd = gen_fixture
    op = GAMMAPrimitiveComboGenOP.__new__(GAMMAPrimitiveComboGenOP)      # the constructor needs a device
    op.dtype, op.device, op.t_his = torch.float32, torch.device("cpu"), 2
    op.predictorcfg = {"modelconfig": {"body_repr": "ssm2_67", "t_his": 2}}
    op.regressorcfg = {"modelconfig": {"gender": "male"}}
    op.testconfig = {"result_dir": str(tmp_path), "seed": 7}
    op.model = _CpuPrior(sd)
    genders = [str(x) for x in g["files_item_genders"]]
    assert genders == ["male", "female", "male"]
    items = [dict({k: g[f"files_item{i}_{k}"] for k in ("body_feature", "betas", "transf_rotmat", "transf_transl", "transl", "glorot",
                                                         "poses")}, gender=genders[i]) for i in range(3)]
    bg = _Batcher(items)
    path = op.generate_primitive_to_files(bg, n_seqs=2, n_gens=3, t_his=2)
    assert bg.i == 3                                                     # the female sequence was drawn and skipped
    import os
    assert os.path.relpath(path, str(tmp_path)) == str(g["files_relpath"])
    with open(path, "rb") as fh:
        res = pickle.load(fh)
    assert list(res.keys()) == [str(k) for k in g["files_keys"]]
    for k, v in res.items():
        assert type(v).__name__ == str(g[f"files_type_{k}"]), k
        ref = g[f"files_val_{k}"]
        if k == "gender":
            assert [str(x) for x in v] == [str(x) for x in ref]
            continue
        arr = v if isinstance(v, np.ndarray) else np.stack([np.asarray(x) for x in v])
        assert arr.shape == ref.shape, (k, arr.shape, ref.shape)
        assert str(arr.dtype if isinstance(v, np.ndarray) else np.asarray(v[0]).dtype) == str(g[f"files_dtype_{k}"]), k
        if k not in ("markers", "smplx_params"):
            assert np.array_equal(arr, ref), k                           # passed through from the batcher
    # the seed frames of every generated sequence are the sequence's first two frames
    assert np.array_equal(res["markers"][:, :, :2], np.broadcast_to(res["gt"][:, :, :2], res["markers"][:, :, :2].shape))
    assert np.array_equal(res["markers"][:, :, :2], g["files_val_markers"][:, :, :2])
    assert np.array_equal(res["smplx_params"][:, :, :2], g["files_val_smplx_params"][:, :, :2])


def test_generate_ppo_is_not_built():
    from egogen_amd.genop import GAMMAPrimitiveComboGenOP
    op = GAMMAPrimitiveComboGenOP.__new__(GAMMAPrimitiveComboGenOP)
    with pytest.raises(NotImplementedError, match="nothing in the reference calls it"):
        op.generate_ppo(None, None, None, None)
