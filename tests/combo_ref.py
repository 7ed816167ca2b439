"""Combo training loss (`GAMMAPrimitiveComboTrainOP.calc_loss_one` / `calc_loss_rollout`, motion/models/models_GAMMA_primitive.py
:773-835, :934-1013) as plain differentiable torch on the CPU, parametrised by dtype: the float64 truth and the float32
yardstick of tests/test_combo_train_{cpu,gpu}.py.  Built from the oracle's pieces as they are (predictor, regressor with its
6D tail, SMPL-X, canonical frame); pinned by tests/golden/combo_train_ref.npz, which scripts/gen_combo_golden.py records from
the reference's own class.

The one reading that differs from the letter of the reference: `get_new_coordinate` receives the FIRST FRAME of the
[t,b,J,3] slice the reference passes whole (:963, :968)."""
import torch

from oracle import nets
from oracle import train as otrain
from oracle.env import get_new_coordinate
from oracle.smplx_lbs import BodyModel, smplx_forward

LOSS_CFG = {"weight_rec": 1.0, "weight_td": 3.0, "weight_kld": 1.0, "weight_reg_hpose": 0.01, "annealing_kld": False,
            "robust_kld": True}
T_HIS, T_PRED = 2, 18
CASES = ("one", "roll", "roll_proj")       # calc_loss_one, calc_loss_rollout, calc_loss_rollout with use_Yproj_as_seed


def cast_state_dict(sd, dtype, requires_grad=True):
    return {k: v.detach().clone().to(dtype).requires_grad_(requires_grad and k.startswith("predictor.")) for k, v in sd.items()}


def combo_forward(sd, X, Y, betas, eps):
    """GAMMAPrimitiveCombo.forward (:324-332) -> Y_rec, mu, logvar, Xb_rec[t,b,93]."""
    Y_rec, mu, logvar = otrain.cvae_forward(sd, X, Y, eps, prefix="predictor.")
    nt, nb = Y_rec.shape[:2]
    Xb = nets.regressor_forward(sd, Y_rec.reshape(nt * nb, -1), betas.reshape(nt * nb, -1), prefix="regressor.")
    return Y_rec, mu, logvar, Xb.view(nt, nb, -1)


def smplx_parser(bm, marker_ids, Yb, betas):
    """_smplx_parser (:837-855) -> markers[t,b,201], joints[t,b,22,3], hand pose[t,b,24]."""
    nt, nb = Yb.shape[:2]
    v, j = smplx_forward(bm, Yb.reshape(nt * nb, -1), betas.reshape(nt * nb, -1))
    return v[:, marker_ids].reshape(nt, nb, -1), j[:, :22].reshape(nt, nb, 22, 3), Yb[..., 69:]


def loss_regressor(bm, marker_ids, x_ref, xb, betas, cfg=LOSS_CFG):
    x_pred, _, hpose = smplx_parser(bm, marker_ids, xb, betas)
    rec = otrain.loss_rec(x_ref, x_pred, cfg)
    hp = (hpose ** 2).mean()
    return rec + cfg["weight_reg_hpose"] * hp, (rec, hp)


def loss_marker(Y, Y_rec, mu, logvar, cfg=LOSS_CFG, scheduled_sampling=False, epoch=0, num_epochs=10):
    rec = otrain.loss_rec(Y, Y_rec, cfg)
    kld, w = otrain._kld(mu, logvar, cfg, epoch, num_epochs)
    return (rec + w * kld) if scheduled_sampling else w * kld, (rec, kld)


def loss_one(sd, bm, marker_ids, betas, markers, eps, cfg=LOSS_CFG, t_his=T_HIS):
    """calc_loss_one -> loss, items [REC, KLD, REG, HPOSE], record."""
    X, Y, betas_Y = markers[:t_his], markers[t_his:, :, :201], betas[t_his:]
    Y_rec, mu, logvar, Yb = combo_forward(sd, X, Y, betas_Y, eps)
    lm, im = loss_marker(Y, Y_rec, mu, logvar, cfg, False)
    lb, ib = loss_regressor(bm, marker_ids, Y, Yb, betas_Y, cfg)
    return lm + lb, torch.stack([v.detach() for v in im + ib]), {"Y_rec": Y_rec.detach(), "Xb_rec": Yb.detach()}


def loss_rollout(sd, bm, marker_ids, betas, markers, jts, eps_list, cfg=LOSS_CFG, use_Yproj_as_seed=False, max_rollout=8,
                 t_his=T_HIS, t_pred=T_PRED):
    """calc_loss_rollout (scheduled_sampling on) -> loss, items, record of every primitive."""
    n_t, n_b = betas.shape[:2]
    jts = jts.reshape(n_t, n_b, -1, 3)
    t, losses, infos = 0, [], []
    rec = {"Y_rec": [], "Xb_rec": [], "X": [], "R_curr": [], "T_curr": []}
    Y_rec = Yb = R_prev = T_prev = None
    while t < n_t:
        t_ub = t + 20
        if t_ub >= n_t:
            break
        betas_Y = betas[t + t_his:t_ub]
        mk = markers[t:t_ub]
        with torch.no_grad():
            if t == 0:
                X, Y = mk[:t_his], mk[t_his:]
                R_prev, T_prev = get_new_coordinate(jts[t])
            else:
                Y_proj, pred_jts, _ = smplx_parser(bm, marker_ids, Yb.detach(), betas_Y)
                R_, T_ = get_new_coordinate(pred_jts[-t_his:][0])
                R_curr = torch.einsum("bij,bjk->bik", R_prev, R_)
                T_curr = torch.einsum("bij,bpj->bpi", R_prev, T_) + T_prev
                Y_blend = Y_proj if use_Yproj_as_seed else Y_rec.detach()
                X_prev = Y_blend.reshape(t_pred, n_b, -1, 3)[-t_his:]
                X = torch.einsum("bij,tbpj->tbpi", R_.permute(0, 2, 1), X_prev - T_.unsqueeze(0)).reshape(t_his, n_b, -1)
                Yg = mk[t_his:].reshape(t_pred, n_b, -1, 3)
                Y = torch.einsum("bij,tbpj->tbpi", R_curr.permute(0, 2, 1), Yg - T_curr.unsqueeze(0)).reshape(t_pred, n_b, -1)
                R_prev, T_prev = R_curr, T_curr
        Y_rec, mu, logvar, Yb = combo_forward(sd, X, Y, betas_Y, eps_list[len(losses)])
        lm, im = loss_marker(Y, Y_rec, mu, logvar, cfg, True)
        if use_Yproj_as_seed:
            lb, ib = loss_regressor(bm, marker_ids, Y, Yb, betas_Y, cfg)
            lm = lm + lb
        else:
            with torch.no_grad():
                _, ib = loss_regressor(bm, marker_ids, Y, Yb, betas_Y, cfg)
        losses.append(lm)
        infos.append(torch.stack([v.detach() for v in im + ib]))
        for k, v in (("Y_rec", Y_rec), ("Xb_rec", Yb), ("X", X), ("R_curr", R_prev), ("T_curr", T_prev)):
            rec[k].append(v.detach())
        t += t_pred
        if len(losses) >= max_rollout:
            break
    return torch.stack(losses).mean(), torch.stack(infos).mean(0), rec


def predictor_grads(loss, sd):
    """d loss / d (every predictor parameter), in state-dict order; None-free (the encoder of y always takes part)."""
    keys = [k for k, v in sd.items() if v.requires_grad]
    return keys, torch.autograd.grad(loss, [sd[k] for k in keys], allow_unused=True)


def evaluate(g, sd, bmd, marker_ids, case, dtype):
    """One of the fixture's three cases ('one', 'roll', 'roll_proj') at `dtype` -> items, grads {key: tensor}, record."""
    bm = BodyModel(bmd, dtype)
    sdd = cast_state_dict(sd, dtype)
    t = lambda name: torch.from_numpy(g[name]).to(dtype)
    if case == "one":
        loss, items, rec = loss_one(sdd, bm, marker_ids, t("one_betas"), t("one_markers"), t("one_eps"))
    else:
        loss, items, rec = loss_rollout(sdd, bm, marker_ids, t("roll_betas"), t("roll_markers"), t("roll_jts"), list(t(case + "_eps")),
                                        use_Yproj_as_seed=(case == "roll_proj"))
    keys, grads = predictor_grads(loss, sdd)
    return items, {k: (gr if gr is not None else torch.zeros_like(sdd[k])) for k, gr in zip(keys, grads)}, rec


def yardstick(truth64, f32, rel=5e-5):
    """The bound a float32 evaluation (the HIP path, or the fixture, which the reference class computed in float32) may be from
    the float64 truth: max(rel x the group's largest magnitude, 3 x the distance of the float32 restatement on the same inputs)."""
    truth64, f32 = torch.as_tensor(truth64, dtype=torch.float64), torch.as_tensor(f32, dtype=torch.float64)
    return max(rel * float(truth64.abs().max()), 3.0 * float((f32 - truth64).abs().max()))


def fixture_world():
    """The fixture, the seeded state dict it names, the synthetic body and the SSM2-67 vertex ids."""
    from egogen_amd import synth
    from tests.helpers import load_golden, rebuild_state_dict
    g = load_golden("combo_train_ref.npz")
    sd = rebuild_state_dict(g, [int(g["pred_seed"]), int(g["reg_seed"])], ["predictor.", "regressor."],
                            gains=[float(g["pred_gain"]), float(g["reg_gain"])])
    return g, sd, synth.make_body_model(int(g["body_model_seed"])), [int(v) for v in synth.marker_ids()]


_CACHE = {}


def evaluated(case, dtype):
    """combo_ref.evaluate on the fixture's inputs, computed once per (case, dtype) and shared (never modified)."""
    key = (case, dtype)
    if key not in _CACHE:
        g, sd, bmd, mids = fixture_world()
        _CACHE[key] = evaluate(g, sd, bmd, mids, case, dtype)
    return _CACHE[key]
