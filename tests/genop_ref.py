"""`GAMMAPrimitiveComboGenOP.generate` (motion/models/models_GAMMA_primitive.py:1166-1249) and the motion-only tail of
`CrowdEnv.step` (motion/crowd_ppo/crowd_env_2f.py:144-155, 238-265 without `_get_feature`) as plain torch on the CPU,
parametrised by dtype: the float64 truth and the float32 yardstick of tests/test_genop_{cpu,gpu}.py.  Built from the oracle's
pieces as they are (predictor, regressor, parameter blending, SMPL-X, canonical frame, torchgeometry's rotation formulas).

  * `generate`: pinned by tests/golden/genop_ref.npz where that fixture is present (scripts/gen_genop_golden.py records it from
    the reference's own class);
  * `advance`: the specification of the kernel egx_primitive_advance;
  * `chain`: sample_prior -> blend -> SMPL-X -> advance, primitive after primitive; pinned by the scene-independent quantities of
    tests/golden/env_step_ref.npz, which the reference's own `CrowdEnv.step` produced (tests/test_genop_cpu.py)."""
import numpy as np
import torch

from oracle import nets
from oracle.env import blend_params, get_new_coordinate, update_transl_glorot
from oracle.smplx_lbs import smplx_forward

T_HIS, T_PRED, T_ALL = 2, 18, 20


def _t(x, dtype, device="cpu"):
    return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).detach().to(device=device, dtype=dtype)


def cast_state_dict(sd, dtype):
    return {k: v.detach().clone().to(dtype) for k, v in sd.items()}


def generate(sd, data, bparams, betas, n_gens=-1, param_blending=True, t_his=T_HIS, z=None, dtype=torch.float32):
    """data[t,b,>=201], bparams[t,b,93], betas (10,) | (1,10) | (b,10), z[b',128] (b' = b * n_gens when n_gens > 0)
    -> Y[b',20,201], Yb[b',20,93] (:1211-1237; `z` is required here: the restatement draws nothing)."""
    sd = cast_state_dict(sd, dtype)
    X = _t(data, dtype)[:t_his, :, :201]
    Xb = _t(bparams, dtype)[:t_his]
    if n_gens > 0:
        X, Xb = X.repeat(1, n_gens, 1), Xb.repeat(1, n_gens, 1)
    nb = X.shape[1]
    bt = _t(betas, dtype).reshape(-1, 10)
    if bt.shape[0] == 1:
        bt = bt.repeat(nb, 1)
    elif n_gens > 0:
        bt = bt.repeat(n_gens, 1)
    Y_pred, Yb_pred = nets.sample_prior(sd, X, bt[None].repeat(T_ALL - t_his, 1, 1), _t(z, dtype))
    Y = torch.cat([X, Y_pred], dim=0)
    Yb = torch.cat([Xb, Yb_pred], dim=0).clone()
    if param_blending:
        Yb = blend_params(Yb, t_his)
    return Y.permute(1, 0, 2).contiguous(), Yb.permute(1, 0, 2).contiguous()


def advance(pred_params, Y_gen, X_seed, joints, markers_proj, delta_T, reproj_factor, R0, T0, dtype=torch.float32, device="cpu"):
    """The arithmetic of egx_primitive_advance.  pred_params[B,20,93], Y_gen[18,B,201], X_seed[2,B,201], joints[B,20,J,3],
    markers_proj[B,20,67,3], delta_T[B,3], R0[B,3,3], T0[B,3] -> dict: marker_b[B,20,67,3], pelvis[B,20,3], R / T (the frame the
    primitive was generated in), R_ / T_ (frame of body (b, 18)), R0 / T0 (updated), seed_params[B,2,93], seed_markers[B,2,201].
    `device`: where the torch ops run (the CPU for the tests; scripts/bench_genop.py times the same ops on the GPU)."""
    c = lambda x: _t(x, dtype, device)
    pp, Yg, X = c(pred_params), c(Y_gen), c(X_seed)
    J, mp, dT = c(joints), c(markers_proj), c(delta_T)
    R0, T0 = c(R0).reshape(-1, 3, 3), c(T0).reshape(-1, 1, 3)
    B = pp.shape[0]
    rf = reproj_factor
    pred_markers = torch.cat([X, Yg], dim=0).reshape(T_ALL, B, -1, 3).permute(1, 0, 2, 3)
    marker_b = rf * mp + (1 - rf) * pred_markers                                              # :151-152
    pelvis = J[:, :, 0]                                                                       # :144
    R_, T_ = get_new_coordinate(J[:, T_ALL - T_HIS])                                          # :241-245, T_[B,1,3]
    T0n = torch.einsum("bij,btj->bti", R0, T_) + T0                                           # :247
    R0n = torch.einsum("bij,bjk->bik", R0, R_)                                                # :248
    seed = pp[:, -T_HIS:]
    seed_new = update_transl_glorot(R_.repeat_interleave(T_HIS, 0), T_.repeat_interleave(T_HIS, 0), dT.repeat_interleave(T_HIS, 0),
                                    seed.reshape(B * T_HIS, -1)).reshape(B, T_HIS, -1)        # :250-257
    marker_seed = torch.einsum("bij,btpj->btpi", R_.permute(0, 2, 1), marker_b[:, -T_HIS:] - T_[..., None, :])   # :259
    return {"marker_b": marker_b, "pelvis": pelvis, "R": R0.clone(), "T": T0[:, 0].clone(), "R_": R_, "T_": T_[:, 0],
            "R0": R0n, "T0": T0n[:, 0], "seed_params": seed_new, "seed_markers": marker_seed.reshape(B, T_HIS, -1)}


def delta_T_of(bm, betas):
    """calc_calibrate_offset (baseops.py:494-534): joint 0 at zero pose / orientation / translation, [B,3]."""
    bt = _t(betas, bm.dtype).reshape(-1, 10)
    _, j = smplx_forward(bm, torch.zeros(bt.shape[0], 93, dtype=bm.dtype), bt)
    return j[:, 0]


def chain(sd, bm, marker_ids, X_seed, seed_params, R0, T0, betas, z, reproj_factor):
    """K = z.shape[0] primitives from one start, in bm's dtype.  X_seed[B,2,201], seed_params[B,2,93], R0[B,3,3], T0[B,3],
    betas[B,10], z[K,B,128] -> list of K dicts: `advance`'s outputs plus Y_gen, pred_params, joints, markers_proj."""
    dt = bm.dtype
    sd = cast_state_dict(sd, dt)
    mk = torch.as_tensor(np.asarray(marker_ids), dtype=torch.long)
    X = _t(X_seed, dt).permute(1, 0, 2)
    seed = _t(seed_params, dt)
    R0, T0, bt, z = _t(R0, dt).reshape(-1, 3, 3), _t(T0, dt).reshape(-1, 3), _t(betas, dt).reshape(-1, 10), _t(z, dt)
    B = bt.shape[0]
    dT = delta_T_of(bm, bt)
    out = []
    for k in range(z.shape[0]):
        Y_gen, Yb_gen = nets.sample_prior(sd, X, bt[None].repeat(T_PRED, 1, 1), z[k])
        Yb = blend_params(torch.cat([seed.permute(1, 0, 2), Yb_gen], dim=0).clone(), T_HIS)
        pp = Yb.permute(1, 0, 2).contiguous()
        v, j = smplx_forward(bm, pp.reshape(B * T_ALL, 93), bt.repeat_interleave(T_ALL, 0))
        joints = j.reshape(B, T_ALL, -1, 3)
        mproj = v[:, mk].reshape(B, T_ALL, -1, 3)
        r = advance(pp, Y_gen, X, joints, mproj, dT, reproj_factor, R0, T0, dt)
        r.update(Y_gen=Y_gen, pred_params=pp, joints=joints, markers_proj=mproj)
        out.append(r)
        X, seed, R0, T0 = r["seed_markers"].permute(1, 0, 2), r["seed_params"], r["R0"], r["T0"]
    return out
