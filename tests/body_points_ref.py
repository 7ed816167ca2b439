"""Cases of the differentiable body points (shared by test_body_points_cpu.py and test_body_points_gpu.py).

Reference: torch autograd of `oracle/smplx_lbs.py::smplx_forward` in float64 on the CPU, with random cotangents for the points and
for the 55 joints.  Yardstick: the same in float32.  Per output group (translation, global orientation, body pose, hand
coefficients, betas) a gradient may be at most R = 3 times as far from the float64 one as the float32 oracle's is - the rule of
tests/precision_yardstick.py without its store term: the factor allows for a different summation order and nothing more.

No GPU needed to import; nothing here is a pytest fixture or setting.  A case is computed once and never modified.
"""
import functools
import math
import os

import numpy as np
import torch

from egogen_amd import synth
from oracle.smplx_lbs import BodyModel, smplx_forward

R = 3.0
GROUPS = ("transl", "glorot", "body_pose", "hands", "betas")
VARIANTS = ("both", "points", "joints")


@functools.lru_cache(maxsize=None)
def body(num_verts=640, seed=0):
    return synth.make_body_model(seed, num_verts=num_verts)


@functools.lru_cache(maxsize=None)
def oracle_body(num_verts, seed, dtype):
    return BodyModel(body(num_verts, seed), dtype)


def marker_vids(num_verts=640):
    return tuple(int(v) for v in synth.marker_ids(num_verts))


def fingertip_vid(num_verts=640):
    """The vertex with the largest weight on joint 39, a fingertip: the deepest chain of the tree."""
    return (int(np.argmax(body(num_verts)["lbs_weights"][:, 39])),)


def random_vids(num_verts=640, count=200, seed=11):
    """`count` random ids with repeats allowed, the first and the last vertex among them."""
    v = np.random.default_rng(seed).integers(0, num_verts, count)
    v[0], v[-1] = 0, num_verts - 1
    return tuple(int(x) for x in v)


def seeded_xb(B, seed):
    """0.4 randn, translation x 3; row 0 at the rest pose, row 1 with body joint 1 at (pi, 0, 0) and everything else zero, row 2
    with the global orientation (0, 0, 3), row 3 with the body pose x 3 (the rows that exist at this B)."""
    g = torch.Generator().manual_seed(seed)
    xb = 0.4 * torch.randn(B, 93, generator=g)
    xb[:, :3] *= 3
    xb[0, 3:] = 0
    if B > 1:
        xb[1] = 0
        xb[1, 6:9] = torch.tensor([math.pi, 0.0, 0.0])
    if B > 2:
        xb[2, 3:6] = torch.tensor([0.0, 0.0, 3.0])
    if B > 3:
        xb[3, 6:69] *= 3
    return xb, g


def groups(g_xb, g_betas):
    g_xb, g_betas = g_xb.detach().cpu().double(), g_betas.detach().cpu().double()
    return {"transl": g_xb[:, :3], "glorot": g_xb[:, 3:6], "body_pose": g_xb[:, 6:69], "hands": g_xb[:, 69:], "betas": g_betas}


class Case:
    """xb[B,93], betas[A,10] (B = A * fpa), cotangents, and the oracle's outputs and gradients in float64 and float32."""

    def __init__(self, B, fpa, vids, num_verts, seed):
        assert B % fpa == 0
        self.B, self.fpa, self.vids, self.num_verts = B, fpa, tuple(vids), num_verts
        self.name = f"B={B} fpa={fpa} P={len(vids)} V={num_verts}"
        self.xb, g = seeded_xb(B, seed)
        self.betas = torch.randn(B // fpa, 10, generator=g)
        self.g_points = torch.randn(B, len(vids), 3, generator=g)
        self.g_joints = torch.randn(B, 55, 3, generator=g)
        self.points64 = self.joints64 = None
        self.grad64, self.grad32 = {}, {}
        for dtype, store in ((torch.float64, self.grad64), (torch.float32, self.grad32)):
            xb = self.xb.clone().to(dtype).requires_grad_(True)
            betas = self.betas.clone().to(dtype).requires_grad_(True)
            verts, joints = smplx_forward(oracle_body(num_verts, 0, dtype), xb, betas.repeat_interleave(fpa, 0))
            points, joints = verts[:, list(self.vids)], joints[:, :55]
            if dtype == torch.float64:
                self.points64, self.joints64 = points.detach(), joints.detach()
            lp, lj = (points * self.g_points.to(dtype)).sum(), (joints * self.g_joints.to(dtype)).sum()
            for variant, loss in (("both", lp + lj), ("points", lp), ("joints", lj)):
                store[variant] = groups(*torch.autograd.grad(loss, (xb, betas), retain_graph=True))
        self.scale = {v: {k: float(self.grad64[v][k].abs().max()) for k in GROUPS} for v in VARIANTS}
        self.err32 = {v: {k: float((self.grad32[v][k] - self.grad64[v][k]).abs().max()) for k in GROUPS} for v in VARIANTS}

    def cotangents(self, variant):
        return (self.g_points if variant != "joints" else None), (self.g_joints if variant != "points" else None)

    def bound(self, variant, group):
        return R * self.err32[variant][group]

    def error(self, variant, g_xb, g_betas):
        got = groups(g_xb, g_betas)
        assert all(got[k].shape == self.grad64[variant][k].shape for k in GROUPS)
        return {k: float((got[k] - self.grad64[variant][k]).abs().max()) for k in GROUPS}


@functools.lru_cache(maxsize=None)
def case(B, fpa=1, vids=None, num_verts=640, seed=3):
    return Case(B, fpa, marker_vids(num_verts) if vids is None else vids, num_verts, seed)


# the batches of the forward and gradient tests: (B, frames_per_agent)
BATCHES = ((1, 1), (5, 1), (37, 1), (12, 4))


def table(c, variant, err):
    """Lines of text: every error next to its ratio to the float32 oracle's."""
    lines = [f"# egx_points_backward, {c.name}, cotangents: {variant} (MI355X)",
             "# group        max|f64|   |f32-f64|      bound        |hip-f64|     ratio"]
    for k in GROUPS:
        e32 = c.err32[variant][k]
        ratio = f"{err[k] / e32:7.2f} x" if e32 > 0 else ("   exact" if err[k] == 0 else "     inf")
        lines.append(f"{k:10s} {c.scale[variant][k]:10.3e} {e32:11.3e} {c.bound(variant, k):10.3e}   {err[k]:10.3e}  ({ratio})")
    return lines


def emit(lines, env="EGX_POINTS_TABLE"):
    """Print the table; append it to the file that the environment variable names, if it names one."""
    print("\n".join(lines))
    out = os.environ.get(env)
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


# ---------------------------------------------------------------------------------------------------------------------------
# the fitting setup: B = 8, generator seed 5
# ---------------------------------------------------------------------------------------------------------------------------
def fit_setup(dtype=torch.float32):
    """(betas, xt, xb0): targets come from xt (pose 0.3 randn, hands 0.5 randn, translation randn); the start is xt with
    + 0.05 randn on the translation and + 0.1 randn on the rotations, hands zeroed."""
    g = torch.Generator().manual_seed(5)
    B = 8
    xt = torch.zeros(B, 93)
    xt[:, :3] = torch.randn(B, 3, generator=g)
    xt[:, 3:69] = 0.3 * torch.randn(B, 66, generator=g)
    xt[:, 69:] = 0.5 * torch.randn(B, 24, generator=g)
    betas = torch.randn(B, 10, generator=g)
    xb0 = xt.clone()
    xb0[:, :3] += 0.05 * torch.randn(B, 3, generator=g)
    xb0[:, 3:69] += 0.1 * torch.randn(B, 66, generator=g)
    xb0[:, 69:] = 0
    return betas.to(dtype), xt.to(dtype), xb0.to(dtype)


def fit_on_cpu(dtype):
    """`fit_markers` with `MarkerBodyModel` on the CPU in `dtype`: (xb, history)."""
    from egogen_amd.fit import fit_markers
    from egogen_amd.train_regressor import MarkerBodyModel
    model = MarkerBodyModel(body(), marker_vids()).to(dtype)
    betas, xt, xb0 = fit_setup(dtype)
    with torch.no_grad():
        target = model(xt, betas)
    return fit_markers(model, target, betas, xb0, steps=150, lr=0.02)
