"""Fitting body parameters to points: the user-facing use of the gradient through the body model (`BodyPoints`) - refine what
the regressor returns, or recover xb from a marker clip (the optimisation the reference runs through `smplx` and torch autograd,
models/baseops.py:382 / models_GAMMA_primitive.py:617-633)."""
from __future__ import annotations

import numpy as np
import torch


def fit_markers(model, target: torch.Tensor, betas: torch.Tensor, xb0: torch.Tensor, steps: int = 150, lr: float = 0.02,
                weight_hpose: float = 0.0, frames_per_agent: int = 1, collision_model=None, penalty=None, weight_pene: float = 0.0):
    """Adam on a copy of xb0[B,93] so that `model(xb, betas)` [B,P,3] meets target[B,P,3].

    model: any callable (xb, betas) -> points: a `BodyPoints` on the device, or on the CPU a `MarkerBodyModel`
    (frames_per_agent != 1 is passed on as a third argument, which `BodyPoints` takes).
    loss: mean over the points of the squared distance + weight_hpose x mean square of the 24 hand coefficients xb[:, 69:].
    penalty: any callable points[B,Q,3] -> [B] (an `SdfPenalty` on the device, a torch callable on the CPU) evaluated on
    `collision_model(xb, betas)` - a second point model, typically a `BodyPoints` on `collision_vids`; None = the points of
    `model`.  weight_pene x its mean over the bodies is added to the loss (nothing is evaluated in the loop while weight_pene is 0).
    Returns (xb, history): history[i] is the mean point distance before step i and history[steps] the one after the last step;
    it is read back once at the end, so the loop never waits for the device.  When `penalty` is given, the penalty[B] of the
    returned xb follows as a third value."""
    if target.dim() != 3 or target.shape[-1] != 3 or xb0.dim() != 2 or xb0.shape[1] != 93 or target.shape[0] != xb0.shape[0]:
        raise ValueError(f"target must be [B,P,3] and xb0 [B,93], got {tuple(target.shape)} and {tuple(xb0.shape)}")
    if steps < 1:
        raise ValueError("steps must be positive")
    if penalty is None and (collision_model is not None or weight_pene):
        raise ValueError("collision_model / weight_pene need a penalty")
    bind = lambda m: (lambda x: m(x, betas)) if frames_per_agent == 1 else (lambda x: m(x, betas, frames_per_agent))
    call = bind(model)
    collide = None if collision_model is None else bind(collision_model)
    xb = xb0.detach().clone().requires_grad_(True)
    optimizer = torch.optim.Adam([xb], lr=lr)
    dist = []
    for _ in range(steps):
        optimizer.zero_grad(set_to_none=True)
        points = call(xb)
        d2 = ((points - target) ** 2).sum(-1)
        loss = d2.mean()
        if weight_hpose:
            loss = loss + weight_hpose * (xb[:, 69:] ** 2).mean()
        if weight_pene:
            loss = loss + weight_pene * penalty(points if collide is None else collide(xb)).mean()
        dist.append(d2.detach().sqrt().mean())
        loss.backward()
        optimizer.step()
    with torch.no_grad():
        points = call(xb)
        dist.append(((points - target) ** 2).sum(-1).sqrt().mean())
        final_pene = None if penalty is None else penalty(points if collide is None else collide(xb)).detach()
    history = torch.stack(dist).cpu().numpy().astype(np.float64)
    if penalty is None:
        return xb.detach(), history
    return xb.detach(), history, final_pene
