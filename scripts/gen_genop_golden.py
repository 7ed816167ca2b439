#!/usr/bin/env python3
"""Execute the reference's own `GAMMAPrimitiveComboGenOP` (models/models_GAMMA_primitive.py:1099-1425) on the CPU and record
tests/golden/genop_ref.npz (data only: seeds, inputs and the class's outputs), in the manner of scripts/gen_combo_golden.py;
the stubs and the seeded fill of scripts/gen_goldens.py are imported.  Needs the reference tree (build container only).

Substitutions for pieces that are absent or unusable here - everything else executed is the reference's code:
  * `build_model` is bypassed (it loads checkpoints that do not exist here): `op.model` is the reference's
    `GAMMAPrimitiveCombo`, in eval mode, filled with seeded weights;
  * `torchgeometry.rotation_matrix_to_angle_axis` -> oracle.rot's restatement (torchgeometry is absent);
  * `torch.cuda.FloatTensor(...)` (:1221, :1388, :1390) -> `torch.FloatTensor(...)` on the CPU (gen_goldens.cuda_to_cpu), and its
    `device=` argument, which the CPU constructor rejects for a cuda device, is dropped;
  * `torch.randn` is captured while `generate_primitive_to_files` runs, so that the z it draws (:130) is part of the fixture;
  * `t_his = 2` is passed explicitly (the default None fails at :1212).

Recorded:
  gen3_*    generate with b = 3, given z, param_blending on and off (Y, Yb, Yb_noblend)
  gen4_*    generate with n_gens = 4 from b = 1, given z whose rows 0 and 2 are equal
  blend_*   _blend_params alone on a random [20,3,93]
  files_*   generate_primitive_to_files with a three-item batcher whose second item has the wrong gender: the batcher's items,
            the captured z, the output path below result_dir, and the pickle's keys, shapes, dtypes and arrays"""
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

from gen_goldens import OUT, REF, cuda_to_cpu, fill_module, install_env_stubs, install_stubs  # noqa: E402

PRED_SEED, REG_SEED, PRED_GAIN, REG_GAIN = 530, 531, 1.0, 0.3
PM = {"body_repr": "ssm2_67", "h_dim": 256, "z_dim": 128, "t_his": 2, "t_pred": 18, "use_drnn_mlp": True, "hdims_mlp": [512, 256],
      "residual": True}
RM = {"body_repr": "ssm2_67", "h_dim": 128, "n_blocks": 10, "n_recur": 3, "actfun": "relu", "use_cont": True, "gender": "male",
      "seq_len": 10}


def seed_inputs(bm, marker_ids, smplx_forward, n_t, nb, g):
    """A smooth walking-like start: xb[n_t,nb,93], betas[nb,10], markers[n_t,nb,201] (projected markers plus 3 mm of noise)."""
    xb = torch.zeros(n_t, nb, 93)
    step = torch.tensor([0.0, 0.02, 0.0]) + torch.randn(1, nb, 3, generator=g) * 0.004
    xb[:, :, :3] = torch.arange(n_t).view(n_t, 1, 1) * step + torch.tensor([0.0, 0.0, 0.9])
    xb[:, :, 3:69] = torch.randn(1, nb, 66, generator=g) * 0.08 + (torch.randn(n_t, nb, 66, generator=g) * 0.02).cumsum(0)
    xb[:, :, 69:] = torch.randn(1, nb, 24, generator=g) * 0.1
    betas = torch.randn(nb, 10, generator=g) * 0.5
    with torch.no_grad():
        v, _ = smplx_forward(bm, xb.reshape(n_t * nb, 93), betas.repeat(n_t, 1))
    markers = v[:, marker_ids].reshape(n_t, nb, 201) + torch.randn(n_t, nb, 201, generator=g) * 0.003
    return xb.contiguous(), betas.contiguous(), markers.contiguous()


class FakeBatcher:
    amass_subset_name = ["synthetic"]

    def __init__(self, items):
        self.items, self.i = items, 0

    def next_sequence(self):
        it = self.items[self.i]
        self.i += 1
        return it


def main():
    from egogen_amd import synth
    from oracle.rot import tgm_rotation_matrix_to_angle_axis
    from oracle.smplx_lbs import BodyModel, smplx_forward
    install_stubs()
    install_env_stubs()
    sys.modules["torchgeometry"].rotation_matrix_to_angle_axis = lambda m: tgm_rotation_matrix_to_angle_axis(m[:, :3, :3])
    sys.path.insert(0, REF)
    torch.set_num_threads(1)
    from models import models_GAMMA_primitive as mgp
    bm = BodyModel(synth.make_body_model(0))
    marker_ids = [int(v) for v in synth.marker_ids()]
    g = torch.Generator().manual_seed(532)
    ns = types.SimpleNamespace
    out = {"pred_seed": np.int64(PRED_SEED), "reg_seed": np.int64(REG_SEED), "pred_gain": np.float64(PRED_GAIN),
           "reg_gain": np.float64(REG_GAIN), "body_model_seed": np.int64(0)}

    with tempfile.TemporaryDirectory() as td, torch.no_grad():
        testconfig = {"gpu_index": 0, "result_dir": td, "seed": 7, "ckpt_dir": td}
        op = mgp.GAMMAPrimitiveComboGenOP(ns(modelconfig=PM, trainconfig={"save_dir": td}), ns(modelconfig=RM, trainconfig={"save_dir": td}),
                                          testconfig)
        assert op.device.type == "cpu"
        op.model = mgp.GAMMAPrimitiveCombo(PM, RM)            # build_model bypassed (see the docstring)
        op.model.predictor.eval()
        op.model.regressor.eval()
        fill_module(op.model.predictor, PRED_SEED, PRED_GAIN)
        fill_module(op.model.regressor, REG_SEED, REG_GAIN)
        sd = op.model.state_dict()
        out["state_dict_keys"] = np.array(list(sd.keys()))
        out["state_dict_shapes"] = np.array([str(tuple(v.shape)) for v in sd.values()])

        # ---- generate, b = 3 ----
        xb, betas, markers = seed_inputs(bm, marker_ids, smplx_forward, 2, 3, g)
        b1 = betas[:1].clone()                                  # the class takes ONE shape for the batch (:1220-1223)
        z = torch.randn(3, 128, generator=g)
        Y, Yb = op.generate(markers.clone(), xb.clone(), b1.clone(), n_gens=-1, to_numpy=True, param_blending=True, t_his=2, z=z.clone())
        _, Yb_nb = op.generate(markers.clone(), xb.clone(), b1.clone(), n_gens=-1, to_numpy=True, param_blending=False, t_his=2, z=z.clone())
        out.update(gen3_data=markers.numpy(), gen3_bparams=xb.numpy(), gen3_betas=b1.numpy(), gen3_z=z.numpy(), gen3_Y=Y, gen3_Yb=Yb,
                   gen3_Yb_noblend=Yb_nb)
        print("generate b=3", Y.shape, Yb.shape, "max|Y|", float(np.abs(Y).max()), "max|Yb|", float(np.abs(Yb).max()))

        # ---- generate, n_gens = 4 from b = 1 ----
        xb, betas, markers = seed_inputs(bm, marker_ids, smplx_forward, 2, 1, g)
        z = torch.randn(4, 128, generator=g)
        z[2] = z[0]
        Y, Yb = op.generate(markers.clone(), xb.clone(), betas.clone(), n_gens=4, to_numpy=True, param_blending=True, t_his=2, z=z.clone())
        _, Yb_nb = op.generate(markers.clone(), xb.clone(), betas.clone(), n_gens=4, to_numpy=True, param_blending=False, t_his=2, z=z.clone())
        out.update(gen4_data=markers.numpy(), gen4_bparams=xb.numpy(), gen4_betas=betas.numpy(), gen4_z=z.numpy(), gen4_Y=Y, gen4_Yb=Yb,
                   gen4_Yb_noblend=Yb_nb)
        assert np.array_equal(Y[0], Y[2]) and np.array_equal(Yb[0], Yb[2])
        print("generate n_gens=4", Y.shape, Yb.shape)

        # ---- _blend_params alone ----
        bp = torch.randn(20, 3, 93, generator=g)
        out["blend_in"] = bp.numpy().copy()
        res = op._blend_params(bp)
        assert res is bp                                        # in place
        out["blend_out"] = res.numpy().copy()

        # ---- generate_primitive_to_files: three items, the second of the wrong gender ----
        items = []
        for i, gender in enumerate(("male", "female", "male")):
            xb, betas, markers = seed_inputs(bm, marker_ids, smplx_forward, 10, 1, g)
            poses = torch.cat([xb[:, 0, 6:69], torch.zeros(10, 3)], dim=1)
            items.append({"body_feature": markers[:, 0].numpy().copy(), "betas": betas[0].numpy().copy(), "gender": gender,
                          "transf_rotmat": np.eye(3, dtype=np.float32)[None] * 1.0, "transf_transl": np.full((1, 1, 3), 0.1 * (i + 1), np.float32),
                          "transl": xb[:, 0, :3].numpy().copy(), "glorot": xb[:, 0, 3:6].numpy().copy(), "poses": poses.numpy().copy()})
        for i, it in enumerate(items):
            for k in ("body_feature", "betas", "transf_rotmat", "transf_transl", "transl", "glorot", "poses"):
                out[f"files_item{i}_{k}"] = it[k]
        out["files_item_genders"] = np.array([it["gender"] for it in items])
        zs = []
        real_randn = torch.randn

        def fake_randn(*a, **k):
            k.pop("device", None)
            e = real_randn(*a, generator=g, **k)
            zs.append(e.clone())
            return e
        real_ft = torch.FloatTensor
        torch.randn = fake_randn
        try:
            with cuda_to_cpu():
                torch.cuda.FloatTensor = lambda a, device=None: real_ft(np.asarray(a, np.float32))
                op.generate_primitive_to_files(FakeBatcher(items), n_seqs=2, n_gens=3, t_his=2)
        finally:
            torch.randn = real_randn
        assert len(zs) == 2
        out["files_z"] = torch.stack(zs).numpy()
        found = [os.path.join(dp, f) for dp, _, fs in os.walk(td) for f in fs]
        assert len(found) == 1, found
        out["files_relpath"] = np.array(os.path.relpath(found[0], td))
        with open(found[0], "rb") as fh:
            res = pickle.load(fh)
        out["files_keys"] = np.array(list(res.keys()))
        for k, v in res.items():
            out[f"files_type_{k}"] = np.array(type(v).__name__)
            if isinstance(v, np.ndarray):
                out[f"files_val_{k}"] = v
                out[f"files_dtype_{k}"] = np.array(str(v.dtype))
            elif k == "gender":
                out[f"files_val_{k}"] = np.array([str(x) for x in v])
            else:
                out[f"files_val_{k}"] = np.stack([np.asarray(x) for x in v])
                out[f"files_dtype_{k}"] = np.array(str(np.asarray(v[0]).dtype))
            print("pickle", k, type(v).__name__, out[f"files_val_{k}"].shape, out[f"files_val_{k}"].dtype)
        print("path", out["files_relpath"])

    # ---- conditioning: the float32 restatement against the fixture and against float64
    from tests import genop_ref
    from tests.helpers import rebuild_state_dict
    sd = rebuild_state_dict(out, [PRED_SEED, REG_SEED], ["predictor.", "regressor."], gains=[PRED_GAIN, REG_GAIN])
    for tag, n_gens in (("gen3", -1), ("gen4", 4)):
        args = (sd, out[tag + "_data"], out[tag + "_bparams"], out[tag + "_betas"])
        Y32, Yb32 = genop_ref.generate(*args, n_gens=n_gens, z=out[tag + "_z"], dtype=torch.float32)
        Y64, Yb64 = genop_ref.generate(*args, n_gens=n_gens, z=out[tag + "_z"], dtype=torch.float64)
        print(tag, "max|f32 restatement - fixture| Y", float((Y32 - torch.as_tensor(out[tag + "_Y"])).abs().max()),
              "Yb", float((Yb32 - torch.as_tensor(out[tag + "_Yb"])).abs().max()),
              "| max|f32 - f64| Y", float((Y32.double() - Y64).abs().max()), "Yb", float((Yb32.double() - Yb64).abs().max()))
    os.makedirs(OUT, exist_ok=True)
    f = os.path.join(OUT, "genop_ref.npz")
    np.savez_compressed(f, **out)
    print("genop_ref", os.path.getsize(f), "bytes")


if __name__ == "__main__":
    main()
