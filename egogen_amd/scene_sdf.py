"""The scene SDF as a differentiable operator: `calc_sdf` (crowd_ppo/utils.py:54-84) with the gradient torch autograd carries
through the reference's `F.grid_sample`, and a penetration penalty on arbitrary points (`SdfPenalty`) that chains behind
`BodyPoints`.  Value, gradient and penalty are HIP kernels (`egx_sdf_value_grad`, `egx_sdf_penalty_forward` /
`egx_sdf_penalty_backward`); everything runs on the current stream without a host synchronisation, and there is no CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .body_model import SdfScene, SdfSceneSet


def _require_device(t: torch.Tensor, scene: SdfScene, what: str):
    if not t.is_cuda:
        raise _lib.EgxError(f"{what} must be on the HIP device - the scene SDF operators have no CPU fallback")
    if t.device != scene.grid.device:
        raise _lib.EgxError(f"{what} is on {t.device}, the scene on {scene.grid.device}")


class _SdfFn(torch.autograd.Function):
    """calc_sdf values of contiguous fp32 device points [B,V,3] as one autograd node.  The forward is `egx_sdf_sample`, or one
    `egx_sdf_value_grad` launch when the gradient field is wanted as a second (non-differentiable) output; the backward is
    `egx_sdf_value_grad` with the cotangent.  Only the points are saved."""

    @staticmethod
    def forward(ctx, pts, scene, want_gradient):
        lib = _lib.load()
        B, V, _ = pts.shape
        val = torch.empty(B, V, dtype=torch.float32, device=pts.device)
        grad = None
        if want_gradient:
            grad = torch.empty(B, V, 3, dtype=torch.float32, device=pts.device)
            _lib.check(lib.egx_sdf_value_grad(C.byref(scene.desc), _lib.ptr(pts), B * V, None, _lib.ptr(val), _lib.ptr(grad),
                                              _lib.current_stream_ptr()), "egx_sdf_value_grad")
            ctx.mark_non_differentiable(grad)
        else:
            _lib.check(lib.egx_sdf_sample(C.byref(scene.desc), _lib.ptr(pts), B * V, _lib.ptr(val), _lib.current_stream_ptr()),
                       "egx_sdf_sample")
        ctx.save_for_backward(pts)
        ctx.scene = scene
        ctx.set_materialize_grads(False)
        return (val, grad) if want_gradient else val

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_val, g_grad=None):
        (pts,) = ctx.saved_tensors
        if g_val is None:
            return None, None, None
        B, V, _ = pts.shape
        g_val = g_val.to(dtype=torch.float32).contiguous()
        g_pts = torch.empty_like(pts)
        _lib.check(_lib.load().egx_sdf_value_grad(C.byref(ctx.scene.desc), _lib.ptr(pts), B * V, _lib.ptr(g_val), None,
                                                  _lib.ptr(g_pts), _lib.current_stream_ptr()), "egx_sdf_value_grad")
        return g_pts, None, None


def sdf_values(vertices: torch.Tensor, scene: SdfScene, return_gradient: bool = False):
    """The differentiable paths of `egogen_amd.utils.calc_sdf`: vertices[B,V,3] of any float dtype and layout on the scene's
    device -> values[B,V] fp32 (an autograd node when vertices require grad), or (values, gradient[B,V,3])."""
    _require_device(vertices, scene, "vertices")
    pts = vertices.to(dtype=torch.float32).contiguous()
    return _SdfFn.apply(pts, scene, bool(return_gradient))


class _PenaltyFn(torch.autograd.Function):
    """penalty[B] (and count[B]) of an `SdfPenalty` as one autograd node.  pts arrives as a contiguous fp32 device tensor; the
    backward recomputes everything from it."""

    @staticmethod
    def forward(ctx, pts, owner, agent_scene, fpa, want_count):
        B, P, _ = pts.shape
        pen = torch.empty(B, dtype=torch.float32, device=pts.device)
        cnt = torch.empty(B, dtype=torch.int32, device=pts.device) if want_count else None
        rc = _lib.load().egx_sdf_penalty_forward(*owner._field(agent_scene), _lib.ptr(pts), B, P, fpa, _lib.ptr(owner._weights(P, pts.device)),
                                                 owner.margin, owner.power, _lib.ptr(pen), _lib.ptr(cnt), _lib.current_stream_ptr())
        _lib.check(rc, "egx_sdf_penalty_forward")
        ctx.save_for_backward(pts)
        ctx.owner, ctx.agent_scene, ctx.fpa = owner, agent_scene, fpa
        ctx.set_materialize_grads(False)
        if want_count:
            ctx.mark_non_differentiable(cnt)
            return pen, cnt
        return pen

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_pen, g_cnt=None):
        (pts,) = ctx.saved_tensors
        if g_pen is None:
            return None, None, None, None, None
        B, P, _ = pts.shape
        owner = ctx.owner
        g_pen = g_pen.to(dtype=torch.float32).contiguous()
        g_pts = torch.empty_like(pts)
        rc = _lib.load().egx_sdf_penalty_backward(*owner._field(ctx.agent_scene), _lib.ptr(pts), B, P, ctx.fpa,
                                                  _lib.ptr(owner._weights(P, pts.device)), owner.margin, owner.power, _lib.ptr(g_pen),
                                                  _lib.ptr(g_pts), _lib.current_stream_ptr())
        _lib.check(rc, "egx_sdf_penalty_backward")
        return g_pts, None, None, None, None


class SdfPenalty:
    """Differentiable penetration penalty of points in a scene: penalty[b] = sum_p w_p * max(margin - calc_sdf(point_bp), 0)^power
    (calc_sdf < 0 inside geometry; power 2 is C1, power 1 a hinge), one fused HIP kernel forward and one backward.

    scene_or_set: an `SdfScene` (or an sdf dict), or an `SdfSceneSet` - then every call names the scene of each agent.
    weights: [P] per-point weights or None (= 1); a zero weight takes a point (a foot, say) out of penalty and count.
    The sum over a body is reduced in a fixed order, so results are bit-reproducible.  There is no CPU fallback."""

    def __init__(self, scene_or_set, weights=None, margin: float = 0.0, power: int = 2):
        if power not in (1, 2):
            raise ValueError("power must be 1 or 2")
        if not torch.cuda.is_available():
            raise _lib.EgxError("no HIP device visible - the SDF penalty has no CPU fallback")
        self.scene = scene_or_set if isinstance(scene_or_set, (SdfScene, SdfSceneSet)) else SdfScene(scene_or_set)
        self.is_set = isinstance(self.scene, SdfSceneSet)
        self.margin, self.power = float(margin), int(power)
        self.weights = None
        if weights is not None:
            w = torch.as_tensor(weights).detach().reshape(-1)
            self.weights = w.to(device=self._grid().device, dtype=torch.float32).contiguous()

    def _grid(self) -> torch.Tensor:
        return (self.scene.scenes[0] if self.is_set else self.scene).grid

    def _weights(self, P: int, device):
        if self.weights is not None and (self.weights.numel() != P or self.weights.device != device):
            raise ValueError(f"the penalty has {self.weights.numel()} weights on {self.weights.device}, the call {P} points per body on {device}")
        return self.weights

    def _field(self, agent_scene):
        """(sdf, scenes, agent_scene) of the C calls."""
        if self.is_set:
            return None, self.scene.handle, _lib.ptr(agent_scene)
        return C.byref(self.scene.desc), None, None

    def __call__(self, points: torch.Tensor, agent_scene=None, frames_per_agent: int = 1, want_count: bool = False):
        """points[B,P,3] -> penalty[B] fp32, or (penalty, count[B] int32) with count = #{p : w_p > 0 and calc_sdf < 0}.
        Differentiable in points.  With a scene set, body b lies in scene agent_scene[b // frames_per_agent]; an index outside the
        set gives penalty 0, count -1 and a zero gradient."""
        fpa = int(frames_per_agent)
        if points.dim() != 3 or points.shape[-1] != 3 or points.shape[0] == 0 or points.shape[1] == 0:
            raise ValueError(f"points must be a non-empty [B,P,3], got {tuple(points.shape)}")
        B = int(points.shape[0])
        if fpa < 1 or B % fpa:
            raise ValueError(f"B={B} is no multiple of frames_per_agent={frames_per_agent}")
        if not points.is_cuda or points.device != self._grid().device:
            raise _lib.EgxError("points must be on the scene's HIP device - the SDF penalty has no CPU fallback")
        if self.is_set:
            if agent_scene is None:
                raise ValueError("a scene-set penalty needs agent_scene [B / frames_per_agent]")
            agent_scene = torch.as_tensor(agent_scene).to(device=points.device, dtype=torch.int32).reshape(-1).contiguous()
            if agent_scene.numel() != B // fpa:
                raise ValueError(f"agent_scene must hold one scene index per agent ({B // fpa}), got {agent_scene.numel()}")
        elif agent_scene is not None:
            raise ValueError("agent_scene needs an SdfSceneSet")
        pts = points.to(dtype=torch.float32).contiguous()
        return _PenaltyFn.apply(pts, self, agent_scene, fpa, bool(want_count))


def collision_vids(bm, feet_vids, n: int = 1024) -> np.ndarray:
    """A deterministic, evenly strided subsample of the vertex ids that are not feet (crowd_env_2f.py:163-175 excludes the feet
    from the penetration count): at most n ids in ascending order, for a `BodyPoints` whose points feed an `SdfPenalty`.
    bm: a body-model dict (its `v_template` gives the vertex count) or anything with a vertex count `V`."""
    V = int(bm.V) if hasattr(bm, "V") else int(np.asarray(bm["v_template"]).shape[0])
    if n < 1:
        raise ValueError("n must be positive")
    feet = np.zeros(V, bool)
    feet[np.asarray(feet_vids, np.int64).reshape(-1)] = True
    rest = np.nonzero(~feet)[0]
    if rest.size == 0:
        raise ValueError("every vertex is a foot vertex")
    if rest.size > n:
        rest = rest[(np.arange(n, dtype=np.int64) * rest.size) // n]
    return rest.astype(np.int32)
