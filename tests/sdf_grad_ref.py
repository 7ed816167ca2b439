"""Cases of the differentiable scene SDF (shared by test_sdf_grad_cpu.py, test_sdf_grad_gpu.py and scripts/gen_sdf_grad_golden.py).

Three evaluations of calc_sdf (crowd_ppo/utils.py:54-84) and its derivative with respect to the points:
  * `closed_form`: numpy, in a chosen dtype - value as aten's grid_sampler_3d forms it, gradient along axis a = minus the bilinear
    combination (other two axes' weights) of the four corner differences along a, times scale * d_a / 2, and exactly 0 where the
    unclamped voxel coordinate is <= 0 or >= d_a - 1 (aten's clip_coordinates_set_grad);
  * `oracle_autograd` in float64: torch autograd of oracle/sdf.py::calc_sdf - the REFERENCE;
  * the same in float32 - the YARDSTICK: a device result may be at most R = 3 times as far from float64 as float32 is (the rule
    of tests/body_points_ref.py).

The interpolated field has kinks: cell faces (the gradient jumps), the hinge of the penalty, the border clamp.  A float32 and a
float64 evaluation that fall on different sides of one differ by a jump, not by rounding, so the inputs keep clear of them by
construction: interior points sit at a cell index plus a fraction from U[0.1, 0.9] (float32 and float64 `floor` agree - asserted,
never filtered), outside points lie well outside or are only compared for their exact zeros, face points use a setup where
world coordinates map to integer voxel coordinates exactly, and penalty points closer than 1e-4 to the hinge are redrawn.

No GPU needed to import; nothing here is a pytest fixture or setting.  A case is computed once and never modified.
"""
import functools

import numpy as np
import torch

from oracle.sdf import calc_sdf as oracle_calc_sdf
from tests import body_points_ref as bref

R = bref.R
CENTER = np.array([0.3, -0.2, 1.0], np.float32)
SCALE = 0.25
TABLE_ENV = "EGX_SDF_GRAD_TABLE"


# ---------------------------------------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------------------------------------
def sample_positions(dims, center, scale):
    """World position [d0,d1,d2,3] (float64) of every sample: center + ((2 i + 1) / d - 1) / scale."""
    ax = [np.asarray(center, np.float64)[a] + ((2 * np.arange(d) + 1) / d - 1) / scale for a, d in enumerate(dims)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1)


def box_field(dims, center, scale, box_center, half):
    """Stored grid (float32) = minus the signed distance to an axis-aligned box: calc_sdf is then negative inside the box."""
    q = np.abs(sample_positions(dims, center, scale) - np.asarray(box_center, np.float64)) - np.asarray(half, np.float64)
    sd = np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0)
    return (-sd).astype(np.float32)


def random_field(dims, seed, gain=1.0):
    return (gain * np.random.default_rng(seed).standard_normal(dims)).astype(np.float32)


def sdf_dict(grid, center=CENTER, scale=SCALE, dtype=torch.float32):
    """The reference's sdf_dict as torch tensors of one dtype (the float32 grid and centre, widened for float64)."""
    return {"sdf": torch.as_tensor(np.asarray(grid, np.float32)).to(dtype), "center": torch.as_tensor(np.asarray(center, np.float32)).to(dtype),
            "scale": torch.tensor(float(scale), dtype=dtype)}


# ---------------------------------------------------------------------------------------------------------------------------
# points
# ---------------------------------------------------------------------------------------------------------------------------
def voxel_coords(pts, dims, center, scale, dtype):
    """Unclamped voxel coordinates [n,3], every operation in `dtype` (aten: ((c + 1) * size - 1) / 2)."""
    dt = np.dtype(dtype).type
    n = (np.asarray(pts, dtype) - np.asarray(center, np.float32).astype(dtype)) * dt(scale)
    return ((n + dt(1)) * np.asarray(dims, dtype) - dt(1)) / dt(2)


def interior_points(dims, center, scale, n, rng):
    """(points float32 [n,3], cells int [n,3]): cell index + U[0.1, 0.9] per axis, mapped to world in float64."""
    d = np.asarray(dims)
    cells = np.stack([rng.integers(0, d[a] - 1, n) for a in range(3)], 1)
    p = cells + rng.uniform(0.1, 0.9, (n, 3))
    world = np.asarray(center, np.float32).astype(np.float64) + ((2 * p + 1) / d - 1) / scale
    return world.astype(np.float32), cells


def assert_floors_agree(pts, cells, dims, center, scale):
    """The precondition of every interior comparison: float32 and float64 put each point into the cell it was drawn in."""
    for dtype in (np.float32, np.float64):
        f = np.floor(voxel_coords(pts, dims, center, scale, dtype))
        assert np.array_equal(f, cells.astype(dtype)), f"{dtype.__name__} floor leaves the drawn cell for {(f != cells).any(1).sum()} points"


def outside_points(center, scale, n, rng):
    return (np.asarray(center, np.float32).astype(np.float64) + rng.uniform(-1.6, 1.6, (n, 3)) / scale).astype(np.float32)


# the face setup: centre 0, scale 0.5, d = 8 - world = (2 k + 1) / 4 - 2 is voxel coordinate k exactly, in float32 too
FACE_D, FACE_SCALE, FACE_CENTER = 8, 0.5, np.zeros(3, np.float32)


def face_points():
    """Points whose voxel coordinates are integers on one, two or three axes (the rest at +0.25 / +0.5), the last plane included."""
    rng = np.random.default_rng(21)
    k = rng.integers(0, FACE_D, (96, 3)).astype(np.float64)
    k[:8] = FACE_D - 1                                         # the far corner and, below, its edges and faces
    frac = rng.choice([0.0, 0.25, 0.5], (96, 3), p=[0.5, 0.25, 0.25])
    frac[0] = 0.0
    frac[k + frac > FACE_D - 1] = 0.0                          # stay inside the sample range
    pts = ((2 * (k + frac) + 1) / FACE_D - 1) / FACE_SCALE
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    assert np.array_equal(voxel_coords(pts.astype(np.float32), (FACE_D,) * 3, FACE_CENTER, FACE_SCALE, np.float32), (k + frac).astype(np.float32))
    return pts.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# the three evaluations
# ---------------------------------------------------------------------------------------------------------------------------
def closed_form(pts, grid, center, scale, dtype=np.float64):
    """(values [n], gradient [n,3]) of calc_sdf at pts [n,3], all arithmetic in `dtype`."""
    dt = np.dtype(dtype).type
    g = np.asarray(grid, np.float32).astype(dtype)
    dims = g.shape
    raw = voxel_coords(pts, dims, center, scale, dtype)
    top = np.asarray(dims, dtype) - dt(1)
    p = np.minimum(np.maximum(raw, dt(0)), top)
    i0f = np.floor(p)                                          # on a face: the upper cell
    w1, w0 = p - i0f, (i0f + dt(1)) - p
    i0 = i0f.astype(np.int64)
    inb = i0 + 1 < np.asarray(dims)
    i1 = np.where(inb, i0 + 1, i0)
    w1 = np.where(inb, w1, dt(0))                              # aten drops corners that fall off the grid
    idx, w = (i0, i1), (w0, w1)
    v = [[[g[idx[a][:, 0], idx[b][:, 1], idx[c][:, 2]] for c in range(2)] for b in range(2)] for a in range(2)]
    val = np.zeros(len(p), dtype)
    for a in range(2):
        for b in range(2):
            for c in range(2):
                val = val + v[a][b][c] * ((w[a][:, 0] * w[b][:, 1]) * w[c][:, 2])
    dx = sum((v[1][b][c] - v[0][b][c]) * (w[b][:, 1] * w[c][:, 2]) for b in range(2) for c in range(2))
    dy = sum((v[a][1][c] - v[a][0][c]) * (w[a][:, 0] * w[c][:, 2]) for a in range(2) for c in range(2))
    dz = sum((v[a][b][1] - v[a][b][0]) * (w[a][:, 0] * w[b][:, 1]) for a in range(2) for b in range(2))
    k = np.asarray(dims, dtype) * dt(0.5) * dt(scale)
    free = (raw > dt(0)) & (raw < top)
    grad = np.where(free, -np.stack([dx, dy, dz], 1) * k, dt(0))
    return -val, grad.astype(dtype)


def autograd_of(fn, pts, sd, cot, dtype):
    """(values [n], d sum(values * cot) / d pts [n,3]) as numpy, by torch autograd of fn(vertices[1,n,3], sd) in `dtype`."""
    v = torch.as_tensor(np.asarray(pts, np.float32)).to(dtype).reshape(1, -1, 3).requires_grad_(True)
    val = fn(v, sd).reshape(-1)
    (val * torch.as_tensor(np.asarray(cot)).to(dtype)).sum().backward()
    return val.detach().numpy(), v.grad.reshape(-1, 3).numpy()


def oracle_autograd(pts, grid, center, scale, cot, dtype):
    return autograd_of(oracle_calc_sdf, pts, sdf_dict(grid, center, scale, dtype), cot, dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# the gradient cases: the golden's (reference autograd recorded) and the oracle's
# ---------------------------------------------------------------------------------------------------------------------------
GOLDEN_CASES = (("r965", (9, 6, 5)), ("r33", (33, 33, 33)), ("box32", (32, 32, 32)))
N_INTERIOR, N_OUTSIDE = 600, 200


def golden_inputs(tag, dims):
    """Grid, points and cotangent of one golden case (scripts/gen_sdf_grad_golden.py records the reference's outputs for them)."""
    seed = [t for t, _ in GOLDEN_CASES].index(tag)
    rng = np.random.default_rng(100 + seed)
    grid = box_field(dims, CENTER, SCALE, (0.8, -0.5, 0.6), (1.1, 0.7, 0.9)) if tag.startswith("box") else random_field(dims, 200 + seed)
    inner, cells = interior_points(dims, CENTER, SCALE, N_INTERIOR, rng)
    assert_floors_agree(inner, cells, dims, CENTER, SCALE)
    pts = np.concatenate([inner, outside_points(CENTER, SCALE, N_OUTSIDE, rng)])
    cot = rng.standard_normal(len(pts)).astype(np.float32)
    return grid, pts, cot


class GradCase:
    """pts [n,3] with the first n_interior of them interior, cotangent, and (values, gradient) in float64 and float32."""

    def __init__(self, name, grid, center, scale, pts, cot, n_interior, f64, f32):
        self.name, self.grid, self.center, self.scale = name, grid, np.asarray(center, np.float32), float(scale)
        self.pts, self.cot, self.n_interior = pts, cot, n_interior
        (self.val64, self.grad64), (self.val32, self.grad32) = f64, f32
        inner = slice(0, n_interior)
        self.scale_ax = np.abs(self.grad64[inner]).max(0)
        self.err32 = np.abs(self.grad32[inner].astype(np.float64) - self.grad64[inner]).max(0)

    def sdf_dict(self):
        return sdf_dict(self.grid, self.center, self.scale)

    def error(self, grad):
        g = np.asarray(grad, np.float64).reshape(-1, 3)
        return np.abs(g[:self.n_interior] - self.grad64[:self.n_interior]).max(0)

    def clamped(self):
        """[n,3] bool: axes on which the border clamp holds the point in float32 AND float64 (their gradient is exactly 0)."""
        dims = self.grid.shape
        out = None
        for dtype in (np.float32, np.float64):
            raw = voxel_coords(self.pts, dims, self.center, self.scale, dtype)
            c = (raw <= 0) | (raw >= np.asarray(dims, dtype) - 1)
            out = c if out is None else out & c
        return out

    def table(self, err):
        lines = [f"# egx_sdf_value_grad, {self.name}, {self.n_interior} interior points (MI355X)",
                 "# axis   max|f64|   |f32-f64|      bound        |hip-f64|     ratio"]
        for a in range(3):
            ratio = f"{err[a] / self.err32[a]:7.2f} x" if self.err32[a] > 0 else ("   exact" if err[a] == 0 else "     inf")
            lines.append(f"{'xyz'[a]:4s} {self.scale_ax[a]:10.3e} {self.err32[a]:11.3e} {R * self.err32[a]:10.3e}   {err[a]:10.3e}  ({ratio})")
        return lines


@functools.lru_cache(maxsize=None)
def golden_case(tag):
    from tests.helpers import load_golden
    g = load_golden("calc_sdf_grad_ref.npz")
    grid, pts, cot = g[f"{tag}_sdf"], g[f"{tag}_pts"], g[f"{tag}_cot"]
    return GradCase(f"golden {tag} {'x'.join(map(str, grid.shape))}", grid, g["center"], float(g["scale"]), pts, cot, int(g["n_interior"]),
                    (g[f"{tag}_val64"], g[f"{tag}_grad64"]), (g[f"{tag}_val32"], g[f"{tag}_grad32"]))


@functools.lru_cache(maxsize=None)
def oracle_case(dims, seed=7, n=600):
    rng = np.random.default_rng(seed)
    grid = random_field(dims, seed + 50)
    inner, cells = interior_points(dims, CENTER, SCALE, n, rng)
    assert_floors_agree(inner, cells, dims, CENTER, SCALE)
    pts = np.concatenate([inner, outside_points(CENTER, SCALE, n // 3, rng)])
    cot = rng.standard_normal(len(pts)).astype(np.float32)
    f64 = oracle_autograd(pts, grid, CENTER, SCALE, cot, torch.float64)
    f32 = oracle_autograd(pts, grid, CENTER, SCALE, cot, torch.float32)
    return GradCase(f"oracle {'x'.join(map(str, dims))}", grid, CENTER, SCALE, pts, cot, n, f64, f32)


def emit(lines):
    bref.emit(lines, env=TABLE_ENV)


# ---------------------------------------------------------------------------------------------------------------------------
# the penalty
# ---------------------------------------------------------------------------------------------------------------------------
def torch_penalty(sd, margin=0.0, power=2, weights=None, fn=oracle_calc_sdf):
    """points [B,P,3] -> penalty [B] with torch ops in the dtype of `sd` (differentiable): the CPU counterpart of SdfPenalty."""
    def penalty(points):
        h = (margin - fn(points, sd)).clamp(min=0)
        t = h * h if power == 2 else h
        return (t if weights is None else weights.to(t.dtype) * t).sum(-1)
    return penalty


PENALTY_DIMS = (16, 16, 16)
PENALTY_SHAPES = ((1, 1), (5, 67), (37, 200), (2, 1024), (3, 1500))


@functools.lru_cache(maxsize=None)
def penalty_grid(seed=31):
    return random_field(PENALTY_DIMS, seed, gain=0.05)


def feet_weights(P):
    """[P] float32 in [0.5, 1.5] with every seventh point (the "feet") at zero."""
    w = np.random.default_rng(P).uniform(0.5, 1.5, P).astype(np.float32)
    w[3::7] = 0
    return w


class PenaltyCase:
    """Interior points [B,P,3] of the penalty grid, none within 1e-4 of the hinge (redrawn, not masked), a cotangent [B], and the
    oracle's penalty and gradient in float64 and float32."""

    def __init__(self, B, P, power, margin, feet, grid=None, seed=0):
        self.B, self.P, self.power, self.margin = B, P, power, margin
        self.grid = penalty_grid() if grid is None else grid
        self.weights = feet_weights(P) if feet else None
        self.name = f"B={B} P={P} power={power} margin={margin} weights={'feet' if feet else 'none'}"
        rng = np.random.default_rng([B, P, power, int(margin * 1000), int(feet), seed])
        dims = self.grid.shape
        pts, cells = interior_points(dims, CENTER, SCALE, B * P, rng)
        for _ in range(100):
            s64 = closed_form(pts, self.grid, CENTER, SCALE)[0]
            bad = np.nonzero(np.abs(margin - s64) < 1e-4)[0]
            if bad.size == 0:
                break
            pts[bad], cells[bad] = interior_points(dims, CENTER, SCALE, bad.size, rng)
        assert bad.size == 0
        assert_floors_agree(pts, cells, dims, CENTER, SCALE)
        self.pts = pts.reshape(B, P, 3)
        self.s64 = s64.reshape(B, P)
        self.g_pen = rng.standard_normal(B).astype(np.float32)
        for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
            w = None if self.weights is None else torch.as_tensor(self.weights)
            v = torch.as_tensor(self.pts).to(dtype).requires_grad_(True)
            pen = torch_penalty(sdf_dict(self.grid, dtype=dtype), margin, power, w)(v)
            (pen * torch.as_tensor(self.g_pen).to(dtype)).sum().backward()
            setattr(self, "pen" + tag, pen.detach().numpy())
            setattr(self, "grad" + tag, v.grad.numpy())
        self.err32_pen = float(np.abs(self.pen32.astype(np.float64) - self.pen64).max())
        self.err32_grad = float(np.abs(self.grad32.astype(np.float64) - self.grad64).max())
        wpos = np.ones(P, bool) if self.weights is None else self.weights > 0
        self.count = ((self.s64 < 0) & wpos).sum(1)

    def sdf_dict(self):
        return sdf_dict(self.grid)


@functools.lru_cache(maxsize=None)
def penalty_case(B, P, power, margin, feet):
    return PenaltyCase(B, P, power, margin, feet)


def penalty_table(rows):
    lines = ["# SdfPenalty against the float64 oracle (MI355X): forward and grad_pts, bound = 3 x |f32 - f64|",
             "# case                                                  |f32-f64| pen  |hip-f64| pen   ratio   |f32-f64| grad |hip-f64| grad   ratio"]
    ratio = lambda e, e32: f"{e / e32:6.2f} x" if e32 > 0 else (" exact" if e == 0 else "   inf")
    for name, e32p, ep, e32g, eg in rows:
        lines.append(f"{name:55s} {e32p:11.3e}   {ep:11.3e}  {ratio(ep, e32p)}   {e32g:11.3e}   {eg:11.3e}  {ratio(eg, e32g)}")
    return lines


# ---------------------------------------------------------------------------------------------------------------------------
# the chain body points -> penalty: float64 autograd of oracle body + oracle SDF
# ---------------------------------------------------------------------------------------------------------------------------
class ChainCase:
    """xb[B,93], betas[B,10], collision ids, a box scene, a cotangent [B]; gradients of sum(penalty * cotangent) with respect to
    xb and betas per group of body_points_ref.GROUPS, in float64 and float32."""

    def __init__(self, B=5, seed=3, margin=0.02, power=2):
        from oracle.smplx_lbs import smplx_forward
        self.B, self.margin, self.power = B, margin, power
        self.vids = bref.random_vids(640, 200, seed=11)
        self.xb, g = bref.seeded_xb(B, seed)
        self.xb[:, :3] = self.xb[:, :3] / 3 + torch.tensor([1.2, 0.0, 0.3])       # around the box, so that bodies reach into it
        self.betas = torch.randn(B, 10, generator=g)
        self.g_pen = torch.randn(B, generator=g)
        self.grid = fit_scene()["sdf"]
        self.grads, self.pen = {}, {}
        for dtype in (torch.float64, torch.float32):
            xb = self.xb.clone().to(dtype).requires_grad_(True)
            betas = self.betas.clone().to(dtype).requires_grad_(True)
            points = smplx_forward(bref.oracle_body(640, 0, dtype), xb, betas)[0][:, list(self.vids)]
            pen = torch_penalty(sdf_dict(self.grid, FIT_CENTER, FIT_SCALE, dtype), margin, power)(points)
            self.pen[dtype] = pen.detach()
            self.grads[dtype] = bref.groups(*torch.autograd.grad((pen * self.g_pen.to(dtype)).sum(), (xb, betas)))
        g64, g32 = self.grads[torch.float64], self.grads[torch.float32]
        self.scale = {k: float(g64[k].abs().max()) for k in bref.GROUPS}
        self.err32 = {k: float((g32[k] - g64[k]).abs().max()) for k in bref.GROUPS}

    def error(self, g_xb, g_betas):
        got = bref.groups(g_xb, g_betas)
        return {k: float((got[k] - self.grads[torch.float64][k]).abs().max()) for k in bref.GROUPS}

    def table(self, err):
        lines = [f"# BodyPoints -> SdfPenalty backward, B={self.B} P={len(self.vids)} (MI355X)",
                 "# group        max|f64|   |f32-f64|      bound        |hip-f64|     ratio"]
        for k in bref.GROUPS:
            e32 = self.err32[k]
            ratio = f"{err[k] / e32:7.2f} x" if e32 > 0 else ("   exact" if err[k] == 0 else "     inf")
            lines.append(f"{k:10s} {self.scale[k]:10.3e} {e32:11.3e} {R * e32:10.3e}   {err[k]:10.3e}  ({ratio})")
        return lines


@functools.lru_cache(maxsize=None)
def chain_case():
    return ChainCase()


# ---------------------------------------------------------------------------------------------------------------------------
# the scene-aware fit: the setup of body_points_ref.fit_setup next to a box
# ---------------------------------------------------------------------------------------------------------------------------
FIT_CENTER, FIT_SCALE, FIT_DIMS = np.array([0.0, 0.0, 1.0], np.float32), 0.25, (64, 64, 64)
FIT_MARGIN, FIT_POWER, FIT_WEIGHT, FIT_STEPS, FIT_LR = 0.02, 2, 1.0, 150, 0.02


@functools.lru_cache(maxsize=None)
def fit_scene():
    """64^3 grid, centre (0, 0, 1), scale 0.25, holding minus the signed distance to the unit box centred (1.5, 0, 0.5)."""
    return {"sdf": box_field(FIT_DIMS, FIT_CENTER, FIT_SCALE, (1.5, 0.0, 0.5), (0.5, 0.5, 0.5)), "center": FIT_CENTER, "scale": FIT_SCALE}


def fit_collision_vids():
    return bref.random_vids(640, 200, seed=11)


def fit_setup(dtype=torch.float32):
    """body_points_ref.fit_setup with the targets' translations moved to (1.5, 0, -0.45) + 0.35 randn (seed 9): around the box.
    The start keeps its offset from the target."""
    betas, xt, xb0 = bref.fit_setup(torch.float64)
    t = torch.tensor([1.5, 0.0, -0.45]) + 0.35 * torch.randn(8, 3, generator=torch.Generator().manual_seed(9))
    xb0[:, :3] += t.double() - xt[:, :3]
    xt[:, :3] = t.double()
    return betas.to(dtype), xt.to(dtype), xb0.to(dtype)


def cpu_fit_parts(dtype, steps=FIT_STEPS):
    """(marker model, collision model, penalty, target, betas, xb0) of the CPU fit in `dtype`, torch ops throughout."""
    from egogen_amd.train_regressor import MarkerBodyModel
    model = MarkerBodyModel(bref.body(), bref.marker_vids()).to(dtype)
    collide = MarkerBodyModel(bref.body(), fit_collision_vids()).to(dtype)
    betas, xt, xb0 = fit_setup(dtype)
    with torch.no_grad():
        target = model(xt, betas)
    penalty = torch_penalty(sdf_dict(fit_scene()["sdf"], FIT_CENTER, FIT_SCALE, dtype), FIT_MARGIN, FIT_POWER)
    return model, collide, penalty, target, betas, xb0


@functools.lru_cache(maxsize=None)
def fit_on_cpu(dtype, weight_pene, steps=FIT_STEPS):
    """`fit_markers` on the CPU in `dtype` with the penalty term weighted by weight_pene: (xb, history, final penalty [8])."""
    from egogen_amd.fit import fit_markers
    model, collide, penalty, target, betas, xb0 = cpu_fit_parts(dtype)
    return fit_markers(model, target, betas, xb0, steps=steps, lr=FIT_LR, collision_model=collide, penalty=penalty, weight_pene=weight_pene)


def adam_loop(model, collide, penalty, target, betas, xb0, steps, lr, weight_pene, b1=0.9, b2=0.999, eps=1e-8):
    """What fit_markers is specified to do, written out: loss = mean squared point distance + weight_pene x mean penalty of the
    collision points, Adam (Kingma & Ba, bias-corrected, torch's epsilon placement) by hand.  (xb, history, final penalty)."""
    xb = xb0.detach().clone()
    m, v = torch.zeros_like(xb), torch.zeros_like(xb)
    hist = []
    for t in range(1, steps + 1):
        x = xb.clone().requires_grad_(True)
        d2 = ((model(x, betas) - target) ** 2).sum(-1)
        loss = d2.mean() + weight_pene * penalty(collide(x, betas)).mean()
        hist.append(float(d2.detach().sqrt().mean()))
        (g,) = torch.autograd.grad(loss, x)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        xb = xb - (lr / (1 - b1 ** t)) * m / (v.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
    with torch.no_grad():
        hist.append(float(((model(xb, betas) - target) ** 2).sum(-1).sqrt().mean()))
        final = penalty(collide(xb, betas))
    return xb, np.asarray(hist, np.float64), final
