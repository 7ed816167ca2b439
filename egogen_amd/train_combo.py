"""Combo training, the third stage of the motion prior: host-side mirror of `GAMMAPrimitiveComboTrainOP`
(models/models_GAMMA_primitive.py:713-1093).  The marker predictor is fine-tuned THROUGH the frozen body regressor and SMPL-X:
predicted markers -> regressor -> 6D-to-axis-angle tail -> body model -> L1 + temporal-difference loss against the target
markers, and (with `scheduled_sampling`) over a rollout whose next primitive is re-seeded from the body the model generated.

Same constructor arguments, loss definitions, optimiser / scheduler and checkpoint layout as the reference
(`<save_dir>/epoch-N.ckp` = {'epoch', 'model_state_dict' with `predictor.*` and `regressor.*` keys, 'optimizer_state_dict'}: the
file `GAMMAPrimitiveComboGenOP.build_model` and `setup_world` read).  What the reference does, quirks included:

  * Adam steps the predictor's parameters only (:1025); `ft_regressor` is read (:733) and never used.  The regressor is frozen,
    so its layers run through `fused_ops.FrozenLinearFn / FrozenResMLPFn`: input gradients only, no weight-gradient products.
  * `load_pretrained` takes the predictor's `epoch-300.ckp` and the regressor's `epoch-100.ckp` from the two configs' `save_dir`
    (:759-770); resume takes the newest `epoch-*.ckp` of the combo's own `save_dir` with optimiser state and epoch (:1031-1039).
  * without `scheduled_sampling` the marker loss is `weight_kld * kld` alone; REC is reported, not optimised (:810-813).
  * the rollout's regressor loss is evaluated under no_grad and left out of the loss unless `use_Yproj_as_seed` (:992-1000).
  * the re-seeding block evaluates the body of the PREVIOUS primitive's parameters with the NEXT window's betas (:966).

One reading differs from the letter of the reference: it hands `get_new_coordinate` the whole [t,b,J,3] slice (:963, :968),
which indexes the batch axis as if it were the joint axis and fails with an IndexError / shape error for general batch sizes;
here the FIRST FRAME of the slice is used, as the predictor's own rollout does (:457, :459).  `use_gt_transform`
(`calc_loss_rollout_UseGTTransform`, :858-930) is not implemented.  Any batch size is accepted (the reference fixes
`n_meshes = batch_size * t_pred` at construction).

The glue between the networks and the body model is three HIP kernel families (csrc/combo.hip) behind `fused_ops.Cont6dToAaFn`,
`PrimitiveLossFn` and `primitive_reseed`; `trainconfig['fused'] = False` spells the same step with torch ops instead (the
baseline those kernels are measured against).  The body model is one `BodyPoints` on the SSM2-67 vertex ids (the reference
evaluates SMPL-X twice per `_smplx_parser` call).  There is no CPU fallback."""
from __future__ import annotations

import glob
import logging
import os
import time
from typing import List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .fused_ops import (ACT_CODE, Cont6dToAaFn, FlatGrads, FrozenLinearFn, FrozenResMLPFn, PrimitiveLossFn, primitive_reseed)
from .models import GAMMAPrimitiveCombo
from .train_predictor import get_scheduler
from .train_regressor import cont6d_params_to_aa


def _section(cfg, name):
    """`cfg.modelconfig` of the reference's config objects, or cfg['modelconfig'] of a plain dict (a parsed yaml)."""
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


def _frame_torch(jts: torch.Tensor):
    """get_new_coordinate_torch (baseops.py:214-225) in torch ops: jts[b,J,3] -> R[b,3,3], T[b,1,3]."""
    x = (jts[:, 2] - jts[:, 1]) * jts.new_tensor([1.0, 1.0, 0.0])
    x = x / torch.norm(x, dim=-1, keepdim=True)
    z = jts.new_tensor([[0.0, 0.0, 1.0]]).repeat(x.shape[0], 1)
    y = torch.linalg.cross(z, x, dim=-1)
    y = y / torch.norm(y, dim=-1, keepdim=True)
    return torch.stack([x, y, z], dim=-1), jts[:, :1]


def _rot(M, x):
    """y[t,b,p,i] = sum_j M[b,i,j] x[t,b,p,j] as a broadcast multiply + sum (3-term dot products, no batched GEMM)."""
    return (M[None, :, None] * x.unsqueeze(-2)).sum(-1)


def _reseed_torch(seed_jts, X_prev, Yg, R_prev, T_prev):
    """`fused_ops.primitive_reseed` in torch ops (:959-984), the baseline that kernel is measured against: joints[b,J,3],
    X_prev[t_his,b,201], Yg[t_pred,b,201], R_prev[b,3,3], T_prev[b,1,3] -> X[t_his,b,201], Y[t_pred,b,201], R_curr, T_curr."""
    n_b = seed_jts.shape[0]
    R_, T_ = _frame_torch(seed_jts[:, :22])
    R_curr = (R_prev.unsqueeze(-1) * R_.unsqueeze(-3)).sum(-2)
    T_curr = (R_prev.unsqueeze(1) * T_.unsqueeze(-2)).sum(-1) + T_prev
    X = _rot(R_.transpose(1, 2), X_prev.reshape(X_prev.shape[0], n_b, -1, 3) - T_.unsqueeze(0)).reshape(X_prev.shape[0], n_b, -1)
    Y = _rot(R_curr.transpose(1, 2), Yg.reshape(Yg.shape[0], n_b, -1, 3) - T_curr.unsqueeze(0)).reshape(Yg.shape[0], n_b, -1)
    return X, Y, R_curr, T_curr


class GAMMAPrimitiveComboTrainOP:
    def __init__(self, predictorcfg, regressorcfg, lossconfig, trainconfig):
        if trainconfig.get("use_gt_transform", False):
            raise NotImplementedError("use_gt_transform (calc_loss_rollout_UseGTTransform, models_GAMMA_primitive.py:858-930) is "
                                      "not implemented; the shipped MPVAECombo configs do not set it")
        if not torch.cuda.is_available():
            raise _lib.EgxError("combo training needs a HIP device (no CPU fallback)")
        self.dtype = torch.float32
        self.device = torch.device("cuda", index=trainconfig.get("gpu_index", 0))
        self.predictorcfg, self.regressorcfg = predictorcfg, regressorcfg
        self.lossconfig, self.trainconfig = lossconfig, trainconfig
        os.makedirs(trainconfig["log_dir"], exist_ok=True)
        self.logger = logging.getLogger(trainconfig["log_dir"])
        if not self.logger.handlers:
            self.logger.addHandler(logging.FileHandler(os.path.join(trainconfig["log_dir"], "train.log")))
        self.logger.setLevel(logging.INFO)
        pm = _section(predictorcfg, "modelconfig")
        self.max_rollout = trainconfig.get("max_rollout", 1e8)
        self.t_his, self.t_pred = pm["t_his"], pm["t_pred"]
        self.use_scheduled_sampling = trainconfig.get("scheduled_sampling", False)
        self.use_gt_transform = False
        self.ft_regressor = trainconfig.get("ft_regressor", False)      # read and never used, as upstream (:733)
        self.use_Yproj_as_seed = trainconfig.get("use_Yproj_as_seed", False)
        self.fused = bool(trainconfig.get("fused", True))
        self.model = None

    # ---- model (:736-770) ---------------------------------------------------------------------------------------------
    def build_model(self, load_pretrained=False, body_model=None, markers=None):
        """`body_model` / `markers`: the SMPL-X tensors and SSM2 vertex ids; by default the ones the rest of the package uses
        (setup_world.load_body_model: the real SMPLX_<GENDER>.npz when present, else the synthetic body)."""
        from . import synth
        from .body_model import BodyPoints
        pm, rm = _section(self.predictorcfg, "modelconfig"), _section(self.regressorcfg, "modelconfig")
        self.model = GAMMAPrimitiveCombo(pm, rm).to(self.device)
        self.model.predictor.train()
        for p in self.model.regressor.parameters():      # frozen: Adam never sees them (:1025)
            p.requires_grad_(False)
        self.grads = FlatGrads(self.model.predictor)
        if body_model is None:
            from . import setup_world
            body_model, _ = setup_world.load_body_model(rm["gender"])
        if markers is None:
            markers = synth.marker_ids(body_model["v_template"].shape[0])
        self.markers = [int(v) for v in markers]
        with torch.cuda.device(self.device):             # the point set's tables are allocated on the current device
            self.points = BodyPoints(body_model, self.markers)
        if load_pretrained:
            self.trainconfig["resume_training"] = False
            ckpt = os.path.join(_section(self.predictorcfg, "trainconfig")["save_dir"], "epoch-300.ckp")
            self.model.predictor.load_state_dict(torch.load(ckpt, map_location=self.device)["model_state_dict"])
            self.logger.info("[INFO] --load pre-trained predictor: {}".format(ckpt))
            ckpt = os.path.join(_section(self.regressorcfg, "trainconfig")["save_dir"], "epoch-100.ckp")
            self.model.regressor.load_state_dict(torch.load(ckpt, map_location=self.device)["model_state_dict"])
            self.logger.info("[INFO] --load pre-trained regressor: {}".format(ckpt))
            self.model.mark_dirty()
            self.grads.attach()

    # ---- forward of GAMMAPrimitiveCombo (:324-332) ----------------------------------------------------------------------
    def _regressor_6d(self, marker_ref, betas):
        """MoshRegressor._forward (:240-259) on frozen weights: [n,201], [n,10] -> xb6[n,159]."""
        net = self.model.regressor.pnet
        relu = ACT_CODE["relu"]
        n = marker_ref.shape[0]
        xb = marker_ref.new_zeros(n, self.model.regressor.body_dim)
        for _ in range(3):
            h = FrozenLinearFn.apply(torch.cat([marker_ref, xb, betas], dim=-1), net.in_fc.weight, net.in_fc.bias, 0, 0.0, None)
            for blk in net.layers:
                h = FrozenResMLPFn.apply(h, blk.layers[0].weight, blk.layers[0].bias, blk.layers[1].weight, blk.layers[1].bias, relu, 0.01)
            if (n * xb.shape[1]) % 4 == 0:               # the fused residual pass works on float4s
                xb = FrozenLinearFn.apply(h, net.out_fc.weight, net.out_fc.bias, 0, 0.0, xb)
            else:
                xb = FrozenLinearFn.apply(h, net.out_fc.weight, net.out_fc.bias, 0, 0.0, None) + xb
        return xb

    def forward(self, X, Y, betas, eps=None, regressor_grad=True):
        """-> Y_rec[t_pred,b,201], mu, logvar, Xb_rec[t_pred,b,93] (axis-angle)."""
        Y_rec, mu, logvar = self.model.predictor.forward_train(X, Y, eps)
        nt, nb = Y_rec.shape[:2]
        with torch.set_grad_enabled(regressor_grad and torch.is_grad_enabled()):
            xb6 = self._regressor_6d(Y_rec.reshape(nt * nb, -1), betas.to(torch.float32).reshape(nt * nb, -1))
            xb = Cont6dToAaFn.apply(xb6) if self.fused else cont6d_params_to_aa(xb6)
        return Y_rec, mu, logvar, xb.view(nt, nb, -1)

    def _smplx_parser(self, Yb, betas):
        """:837-855 with ONE body evaluation: -> markers[t,b,201], joints[t,b,55,3] (the reference keeps the first 22), hand pose."""
        nt, nb = Yb.shape[:2]
        pts, jts = self.points(Yb.reshape(nt * nb, -1), betas.reshape(nt * nb, -1), want_joints=True)
        return pts.view(nt, nb, -1), jts.view(nt, nb, -1, 3), Yb[..., 69:]

    # ---- losses ---------------------------------------------------------------------------------------------------------
    def _calc_loss_rec(self, Y, Y_rec):
        """:773-784 -> weight_rec * rec + weight_td * td (a device scalar)."""
        w_rec, w_td = self.lossconfig["weight_rec"], self.lossconfig["weight_td"]
        if self.fused:
            return PrimitiveLossFn.apply(Y, Y_rec, w_rec, w_td)[0]
        loss_rec = F.l1_loss(Y, Y_rec)
        if Y.shape[0] < 2:
            return w_rec * loss_rec
        loss_td = F.l1_loss(Y_rec[1:] - Y_rec[:-1], Y[1:] - Y[:-1])
        return w_rec * loss_rec + w_td * loss_td

    def _loss_regressor(self, x_ref, xb, betas):
        x_pred, _, hpose = self._smplx_parser(xb, betas)
        loss_marker_rec = self._calc_loss_rec(x_ref, x_pred)
        loss_hpose = torch.mean(hpose ** 2)
        loss = loss_marker_rec + self.lossconfig["weight_reg_hpose"] * loss_hpose
        return loss, torch.stack([loss_marker_rec.detach(), loss_hpose.detach()])

    def _loss_marker(self, Y, Y_rec, mu, logvar, epoch):
        loss_rec = self._calc_loss_rec(Y, Y_rec)
        loss_kld = 0.5 * torch.mean(-1 - logvar + mu.pow(2) + logvar.exp())
        if self.lossconfig["robust_kld"]:
            loss_kld = torch.sqrt(1 + loss_kld ** 2) - 1
        weight_kld = self.lossconfig["weight_kld"]
        if self.lossconfig["annealing_kld"]:
            weight_kld = min(float(epoch) / (0.9 * self.trainconfig["num_epochs"]), 1.0) * self.lossconfig["weight_kld"]
        loss = loss_rec + weight_kld * loss_kld if self.use_scheduled_sampling else weight_kld * loss_kld
        return loss, torch.stack([loss_rec.detach(), loss_kld.detach()])

    def calc_loss_regressor(self, x_ref, x_ref_pred, xb, betas):
        """:787-794: L1 + td between the target markers x_ref[t,b,201] and the SMPL-X markers of the regressed body xb[t,b,93],
        plus weight_reg_hpose x mean square of the hand coefficients.  `x_ref_pred` is unused, as upstream."""
        loss, info = self._loss_regressor(x_ref, xb, betas)
        return loss, info.cpu().numpy()

    def calc_loss_marker(self, Y, Y_rec, mu, logvar, epoch):
        """:798-814."""
        loss, info = self._loss_marker(Y, Y_rec, mu, logvar, epoch)
        return loss, info.cpu().numpy()

    def calc_loss_one(self, data, epoch, eps: Optional[torch.Tensor] = None):
        """:817-835: data = [betas[20,b,10], markers[20,b,201], ...] -> loss, np.array([REC, KLD, REG, HPOSE]).  `eps`: the
        reparameterisation noise (tests inject it)."""
        betas, ref_markers = (d.to(self.device) for d in data[:2])
        X = ref_markers[:self.t_his]
        Y = ref_markers[self.t_his:, :, :67 * 3].contiguous()
        betas_Y = betas[self.t_his:]
        Y_rec, mu, logvar, Yb_rec = self.forward(X, Y, betas_Y, eps)
        loss_marker, info_m = self._loss_marker(Y, Y_rec, mu, logvar, epoch)
        loss_bparams, info_b = self._loss_regressor(Y, Yb_rec, betas_Y)
        return loss_marker + loss_bparams, torch.cat([info_m, info_b]).cpu().numpy()

    @torch.no_grad()
    def _reseed(self, Y_rec, Yb_rec, betas_Y, Yg, R_prev, T_prev):
        """The detached block of the rollout (:959-984): the body of the previous primitive's parameters (with the next window's
        betas, :966), its frame, and the seed and target markers in it -> X[t_his,b,201], Y[t_pred,b,201], R_curr, T_curr."""
        Y_proj, pred_jts, _ = self._smplx_parser(Yb_rec.detach(), betas_Y)
        Y_blend = Y_proj if self.use_Yproj_as_seed else Y_rec.detach()
        seed_jts = pred_jts[self.t_pred - self.t_his]                    # [b,55,3]: first frame of pred_jts[-t_his:]
        if self.fused:
            return primitive_reseed(seed_jts, Y_blend[-self.t_his:], Yg, R_prev, T_prev)[:4]
        return _reseed_torch(seed_jts, Y_blend[-self.t_his:], Yg, R_prev, T_prev)

    def calc_loss_rollout(self, data, epoch, eps_list: Optional[List[torch.Tensor]] = None):
        """:934-1013: windows of 20 frames advancing by t_pred, at most `max_rollout` of them.  Primitive k > 0 lives in the frame
        of the GENERATED body (first frame of the last t_his frames of primitive k-1: see the module docstring for that
        reading) and is seeded with Y_rec[-t_his:], or with the reprojected markers under `use_Yproj_as_seed`; everything in
        that block is detached.  -> mean loss over the primitives, np.array([REC, KLD, REG, HPOSE]) likewise."""
        betas, ref_markers, _, _, _, ref_jts = data
        betas, ref_markers = betas.to(self.device), ref_markers.to(self.device)
        if ref_markers.shape[-1] != 67 * 3:      # not sliced here, as upstream: a wider row would not fit the frames of k > 0
            raise ValueError("calc_loss_rollout takes marker rows of 67 x 3 = 201 values, got %d" % ref_markers.shape[-1])
        n_t, n_b = betas.shape[:2]
        ref_jts = ref_jts.view(n_t, n_b, -1, 3).to(self.device)
        t_his, t_pred = self.t_his, self.t_pred
        t, loss, loss_info = 0, [], []
        Y_rec = Yb_rec = R_curr = T_curr = None
        while t < n_t:
            t_ub = t + 20
            if t_ub >= n_t:
                break
            betas_Y = betas[t + t_his:t_ub]
            window = ref_markers[t:t_ub]
            if t == 0:                                                   # only the first primitive starts from the data
                X, Y = window[:t_his].detach(), window[t_his:].detach().contiguous()
                with torch.no_grad():
                    R_curr, T_curr = _frame_torch(ref_jts[t])
            else:
                X, Y, R_curr, T_curr = self._reseed(Y_rec, Yb_rec, betas_Y, window[t_his:], R_curr, T_curr)
            Y_rec, mu, logvar, Yb_rec = self.forward(X, Y, betas_Y, None if eps_list is None else eps_list[len(loss)],
                                                     regressor_grad=self.use_Yproj_as_seed)
            loss_marker, info_m = self._loss_marker(Y, Y_rec, mu, logvar, epoch)
            if not self.use_Yproj_as_seed:
                with torch.no_grad():
                    _, info_b = self._loss_regressor(Y, Yb_rec, betas_Y)
                loss_ = loss_marker
            else:
                loss_bparams, info_b = self._loss_regressor(Y, Yb_rec, betas_Y)
                loss_ = loss_marker + loss_bparams
            loss.append(loss_)
            loss_info.append(torch.cat([info_m, info_b]))
            t += t_pred
            if len(loss) >= self.max_rollout:
                break
        return torch.stack(loss).mean(), torch.stack(loss_info).mean(0).cpu().numpy()

    def step(self, optimizer, loss):
        """loss.backward() + optimizer.step() around the predictor's flat gradient buffer (:1061-1063)."""
        self.grads.zero()
        loss.backward(retain_graph=False)
        optimizer.step()

    # ---- training loop (:1018-1093) ---------------------------------------------------------------------------------------
    def train(self, batch_gen):
        tc = self.trainconfig
        if self.model is None:
            self.build_model(load_pretrained=not tc.get("resume_training", False))
        starting_epoch = 0
        optimizer = torch.optim.Adam(self.model.predictor.parameters(), lr=tc["learning_rate"])
        scheduler = get_scheduler(optimizer, policy="lambda", num_epochs_fix=tc["num_epochs_fix"], num_epochs=tc["num_epochs"])
        if tc.get("resume_training", False):
            ckp_list = sorted(glob.glob(os.path.join(tc["save_dir"], "epoch-*.ckp")), key=os.path.getmtime)
            if ckp_list:
                checkpoint = torch.load(ckp_list[-1], map_location=self.device)
                self.model.load_state_dict(checkpoint["model_state_dict"])
                optimizer.load_state_dict(checkpoint["optimizer_state_dict"])
                starting_epoch = checkpoint["epoch"]
                self.grads.attach()
                self.logger.info("[INFO] --resuming training from {}".format(ckp_list[-1]))
        gender = _section(self.regressorcfg, "modelconfig")["gender"]
        loss_names = ["REC", "KLD", "REG", "HPOSE"]
        history = []
        for epoch in range(starting_epoch, tc["num_epochs"]):
            epoch_losses, epoch_nsamples = 0, 0
            stime = time.time()
            while batch_gen.has_next_rec():
                data = batch_gen.next_batch_genderselection(batch_size=tc["batch_size"], gender=gender, batch_first=False)   # [t,b,d]
                if data is None:
                    continue
                if self.use_scheduled_sampling:
                    loss, items = self.calc_loss_rollout(data, epoch)
                else:
                    loss, items = self.calc_loss_one(data, epoch)
                self.step(optimizer, loss)
                epoch_losses = epoch_losses + items
                epoch_nsamples += 1
            batch_gen.reset()
            scheduler.step()
            epoch_losses = epoch_losses / max(epoch_nsamples, 1)
            info = "[epoch {:d}]:".format(epoch + 1) + "".join("{}={:f}, ".format(n, v) for n, v in zip(loss_names, np.atleast_1d(epoch_losses)))
            info += "time={:f}, lr={:f}".format(time.time() - stime, optimizer.param_groups[0]["lr"])
            self.logger.info(info)
            history.append(np.atleast_1d(epoch_losses))
            if (1 + epoch) % tc["saving_per_X_ep"] == 0:
                os.makedirs(tc["save_dir"], exist_ok=True)
                torch.save({"epoch": epoch + 1, "model_state_dict": self.model.state_dict(),
                            "optimizer_state_dict": optimizer.state_dict()}, os.path.join(tc["save_dir"], f"epoch-{epoch + 1}.ckp"))
            if tc.get("verbose", False):
                print(info)
        return history
