"""The differentiable scene SDF on the device (`calc_sdf` under autograd, `SdfPenalty`, the penalty term of `fit_markers`) against
torch autograd of the reference / the oracle in float64 (tests/sdf_grad_ref.py).

Values are held bit for bit to `egx_sdf_sample`.  Gradients and penalties are held to R = 3 times the distance of the float32
evaluation from the float64 one.  The tests print every error next to its ratio to the float32 one; EGX_SDF_GRAD_TABLE=<file>
appends the tables to a file (committed in profiles/sdf_grad.md)."""
import itertools

import numpy as np
import pytest
import torch

from tests import body_points_ref as bref
from tests import sdf_grad_ref as ref

pytestmark = pytest.mark.gpu


def _scene(grid, center=ref.CENTER, scale=ref.SCALE):
    from egogen_amd.body_model import SdfScene
    return SdfScene({"sdf": np.asarray(grid, np.float32), "center": np.asarray(center, np.float32), "scale": float(scale)})


class _row_major:
    """The scene without its tables for the duration of the block: the calls then gather from the row-major grid."""

    def __init__(self, scene):
        self.scene = scene

    def __enter__(self):
        self.saved = self.scene.desc.coarse_minmax
        self.scene.desc.coarse_minmax = None

    def __exit__(self, *exc):
        self.scene.desc.coarse_minmax = self.saved


# ---------------------------------------------------------------------------------------------------------------------------
# 1. values: bit-identical to calc_sdf, bricked and row-major
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(9, 6, 5), (16, 16, 16), (7, 5, 2)])
def test_values_are_those_of_calc_sdf_and_both_paths_agree_bit_for_bit(dims):
    from egogen_amd.utils import calc_sdf
    scene = _scene(ref.random_field(dims, 3))
    rng = np.random.default_rng(4)
    for n in (1, 255, 256, 257, 4 * 256 * 3 - 1, 4 * 256 * 3 + 1):
        pts = torch.as_tensor((ref.CENTER + rng.uniform(-1.3, 1.3, (1, n, 3)) / ref.SCALE).astype(np.float32)).cuda()
        plain = calc_sdf(pts, scene)
        val, grad = calc_sdf(pts, scene, return_gradient=True)
        with _row_major(scene):
            plain_rm = calc_sdf(pts, scene)
            val_rm, grad_rm = calc_sdf(pts, scene, return_gradient=True)
        assert val.shape == (1, n) and grad.shape == (1, n, 3) and val.dtype == grad.dtype == torch.float32
        assert torch.equal(val, plain) and torch.equal(val_rm, plain_rm) and torch.equal(plain, plain_rm), (dims, n)
        assert torch.equal(grad, grad_rm), (dims, n)
        assert torch.isfinite(grad).all() and (grad != 0).any()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. gradient: within three times the float32 evaluation, exact zeros outside, the face convention
# ---------------------------------------------------------------------------------------------------------------------------
def _device_grad(c, scene):
    from egogen_amd.utils import calc_sdf
    v = torch.as_tensor(c.pts).reshape(1, -1, 3).cuda().requires_grad_(True)
    val = calc_sdf(v, scene)
    val.backward(torch.as_tensor(c.cot).reshape(1, -1).cuda())
    return val.detach().cpu().numpy().reshape(-1), v.grad.cpu().numpy().reshape(-1, 3)


@pytest.mark.parametrize("name", ["golden r965", "golden r33", "golden box32", "oracle 16x16x16", "oracle 7x5x2"])
def test_gradient_within_three_times_the_float32_evaluation(name):
    kind, tag = name.split()
    c = ref.golden_case(tag) if kind == "golden" else ref.oracle_case(tuple(int(d) for d in tag.split("x")))
    scene = _scene(c.grid, c.center, c.scale)
    val, grad = _device_grad(c, scene)
    with _row_major(scene):
        val_rm, grad_rm = _device_grad(c, scene)
    assert np.array_equal(grad, grad_rm) and np.array_equal(val, val_rm)
    err = c.error(grad)
    ev, ev32 = np.abs(val - c.val64).max(), np.abs(c.val32.astype(np.float64) - c.val64).max()
    ref.emit(c.table(err) + [f"values: |f32-f64| {ev32:.3e}  |hip-f64| {ev:.3e}"])
    assert (err <= ref.R * c.err32).all(), (c.name, err, c.err32)
    assert ev <= ref.R * ev32
    held = c.clamped()
    assert held.any() and (grad[held] == 0).all()                       # the border clamp: exact zeros, compared with ==


def test_gradient_on_cell_faces_takes_the_upper_cell_and_vanishes_on_the_last_plane():
    from egogen_amd.utils import calc_sdf
    d = ref.FACE_D
    grid = ref.random_field((d, d, d), 5)
    scene = _scene(grid, ref.FACE_CENTER, ref.FACE_SCALE)
    pts = ref.face_points()
    val, grad = calc_sdf(torch.as_tensor(pts).reshape(1, -1, 3).cuda(), scene, return_gradient=True)
    val, grad = val.cpu().numpy().reshape(-1), grad.cpu().numpy().reshape(-1, 3).astype(np.float64)
    v64, g64 = ref.closed_form(pts, grid, ref.FACE_CENTER, ref.FACE_SCALE)
    v32, g32 = ref.closed_form(pts, grid, ref.FACE_CENTER, ref.FACE_SCALE, np.float32)
    e32 = np.abs(g32.astype(np.float64) - g64).max(0)
    err = np.abs(grad - g64).max(0)
    ref.emit([f"# faces, {d}^3, {len(pts)} points on integer voxel coordinates: gradient |f32-f64| {e32}, |hip-f64| {err}"])
    assert (err <= ref.R * e32).all(), (err, e32)
    assert np.abs(val - v64).max() <= 4 * np.finfo(np.float32).eps * np.abs(v64).max()
    vox = ref.voxel_coords(pts, (d,) * 3, ref.FACE_CENTER, ref.FACE_SCALE, np.float64)
    edge = (vox <= 0) | (vox >= d - 1)
    assert edge.any() and (grad[edge] == 0).all() and (g64[edge] == 0).all() and (grad[~edge] != 0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the autograd contract of calc_sdf
# ---------------------------------------------------------------------------------------------------------------------------
def test_calc_sdf_autograd_contract():
    from egogen_amd._lib import EgxError
    from egogen_amd.utils import calc_sdf
    c = ref.oracle_case((16, 16, 16))
    scene = _scene(c.grid)
    sd = c.sdf_dict()                                                   # the dict form goes through the same scene cache
    pts = torch.as_tensor(c.pts).reshape(4, -1, 3).cuda()
    cot = torch.as_tensor(c.cot).reshape(4, -1).cuda()
    plain = calc_sdf(pts, scene)
    val0, field = calc_sdf(pts, scene, return_gradient=True)
    assert plain.grad_fn is None and val0.grad_fn is None and not field.requires_grad

    v = pts.clone().requires_grad_(True)
    out = calc_sdf(v, sd)
    assert out.grad_fn is not None and torch.equal(out, plain)
    out.backward(cot)
    assert torch.equal(v.grad, cot.unsqueeze(-1) * field)

    with torch.no_grad():
        assert calc_sdf(v, scene).grad_fn is None
    assert calc_sdf(v.detach(), scene).grad_fn is None

    val1, field1 = calc_sdf(v, scene, return_gradient=True)             # values differentiable, the field a plain tensor
    assert val1.grad_fn is not None and not field1.requires_grad and torch.equal(field1, field)

    # any float dtype and layout: the gradient comes back in the input's own
    w = pts.double().transpose(0, 1).contiguous().transpose(0, 1).requires_grad_(True)
    assert not w.is_contiguous()
    calc_sdf(w, scene).backward(cot)
    assert w.grad.dtype == torch.float64 and w.grad.shape == w.shape and torch.equal(w.grad.float(), v.grad)

    (g,) = torch.autograd.grad(calc_sdf(v, scene).sum(), v, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        u = pts.clone().requires_grad_(True)
        out_s = calc_sdf(u, scene)
        out_s.backward(cot)
    side.synchronize()
    assert torch.equal(out_s, out) and torch.equal(u.grad, v.grad)

    empty = calc_sdf(torch.zeros(2, 0, 3, device="cuda"), scene, return_gradient=True)
    assert empty[0].shape == (2, 0) and empty[1].shape == (2, 0, 3)
    with pytest.raises(EgxError):
        calc_sdf(pts.cpu().requires_grad_(True), scene)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the penalty
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def penalty_scene():
    return _scene(ref.penalty_grid())


@pytest.mark.parametrize("B,P", ref.PENALTY_SHAPES)
def test_penalty_forward_backward_count(penalty_scene, B, P):
    from egogen_amd.scene_sdf import SdfPenalty
    from egogen_amd.utils import calc_sdf
    rows = []
    for power, margin, feet in itertools.product((1, 2), (0.0, 0.02), (False, True)):
        c = ref.penalty_case(B, P, power, margin, feet)
        op = SdfPenalty(penalty_scene, weights=c.weights, margin=margin, power=power)
        pts = torch.as_tensor(c.pts).cuda().requires_grad_(True)
        pen, cnt = op(pts, want_count=True)
        assert pen.shape == (B,) and pen.dtype == torch.float32 and cnt.shape == (B,) and cnt.dtype == torch.int32 and not cnt.requires_grad
        pen.backward(torch.as_tensor(c.g_pen).cuda())
        ep = float(np.abs(pen.detach().cpu().numpy().astype(np.float64) - c.pen64).max())
        eg = float(np.abs(pts.grad.cpu().numpy().astype(np.float64) - c.grad64).max())
        rows.append((c.name, c.err32_pen, ep, c.err32_grad, eg))
        print(ref.penalty_table(rows[-1:])[-1])
        assert ep <= ref.R * c.err32_pen, (c.name, ep, c.err32_pen)
        assert eg <= ref.R * c.err32_grad, (c.name, eg, c.err32_grad)
        w = torch.ones(P, device="cuda") if c.weights is None else torch.as_tensor(c.weights).cuda()
        inside = (calc_sdf(pts.detach(), penalty_scene) < 0) & (w > 0)
        assert torch.equal(cnt.long(), inside.sum(1))
        again = pts.detach().clone().requires_grad_(True)
        pen2, cnt2 = op(again, want_count=True)
        pen2.backward(torch.as_tensor(c.g_pen).cuda())
        assert torch.equal(pen2, pen) and torch.equal(cnt2, cnt) and torch.equal(again.grad, pts.grad)
        with _row_major(penalty_scene):
            other = pts.detach().clone().requires_grad_(True)
            pen3 = op(other)
            pen3.backward(torch.as_tensor(c.g_pen).cuda())
        assert torch.equal(pen3, pen) and torch.equal(other.grad, pts.grad)
    ref.emit(ref.penalty_table(rows))


def test_penalty_in_free_space_layouts_and_errors():
    from egogen_amd._lib import EgxError
    from egogen_amd.scene_sdf import SdfPenalty
    sc = ref.fit_scene()
    op = SdfPenalty(_scene(sc["sdf"], sc["center"], sc["scale"]), margin=0.02, power=2)
    g = torch.Generator().manual_seed(1)
    free = (torch.tensor([-2.0, 0.0, 1.0]) + torch.rand(6, 300, 3, generator=g) - 0.5).cuda().requires_grad_(True)   # >= 2 m from the box
    pen, cnt = op(free, want_count=True)
    pen.sum().backward()
    assert (pen == 0).all() and (cnt == 0).all() and (free.grad == 0).all()
    # a float64, non-contiguous batch that reaches into the box: the gradient comes back in its own dtype and layout
    deep = torch.tensor([1.5, 0.0, 0.5]) + 0.8 * (torch.rand(300, 6, 3, generator=g) - 0.5)
    a = deep.transpose(0, 1).double().cuda().requires_grad_(True)
    b = deep.transpose(0, 1).contiguous().cuda().requires_grad_(True)
    assert not a.is_contiguous()
    pa, pb = op(a), op(b)
    pa.sum().backward(), pb.sum().backward()
    assert (pa > 0).all() and torch.equal(pa, pb)
    assert a.grad.dtype == torch.float64 and a.grad.shape == a.shape and torch.equal(a.grad.float(), b.grad) and (b.grad != 0).any()
    (gg,) = torch.autograd.grad(op(b).sum(), b, create_graph=True)
    with pytest.raises(RuntimeError):
        gg.sum().backward()
    with pytest.raises(EgxError):
        op(deep)                                                        # a CPU tensor
    with pytest.raises(ValueError):
        op(b, agent_scene=torch.zeros(6, dtype=torch.int32))            # agent_scene needs a set
    with pytest.raises(ValueError):
        SdfPenalty(op.scene, weights=np.ones(5, np.float32))(b)         # five weights, 300 points
    with pytest.raises(ValueError):
        SdfPenalty(op.scene, power=3)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. scene sets
# ---------------------------------------------------------------------------------------------------------------------------
def test_penalty_over_a_scene_set_is_the_one_scene_call_per_body():
    from egogen_amd.body_model import SdfSceneSet
    from egogen_amd.scene_sdf import SdfPenalty
    centers = (ref.CENTER, ref.CENTER + np.float32(0.4), ref.CENTER - np.float32(0.3))
    scenes = [_scene(ref.random_field((16, 16, 16), 60 + i, gain=0.05), centers[i], ref.SCALE * (1 + 0.1 * i)) for i in range(3)]
    sset = SdfSceneSet(scenes)
    fpa, P = 4, 67
    agent_scene = torch.tensor([0, -1, 2, 3, 1], dtype=torch.int32)
    B = fpa * len(agent_scene)
    rng = np.random.default_rng(8)
    pts0 = torch.as_tensor((ref.CENTER + rng.uniform(-1.1, 1.1, (B, P, 3)) / ref.SCALE).astype(np.float32)).cuda()
    w = ref.feet_weights(P)
    g_pen = torch.as_tensor(rng.standard_normal(B).astype(np.float32)).cuda()
    op = SdfPenalty(sset, weights=w, margin=0.02, power=2)
    pts = pts0.clone().requires_grad_(True)
    pen, cnt = op(pts, agent_scene=agent_scene, frames_per_agent=fpa, want_count=True)
    pen.backward(g_pen)
    for a, s in enumerate(agent_scene.tolist()):
        rows = slice(a * fpa, (a + 1) * fpa)
        if 0 <= s < 3:
            one = pts0[rows].clone().requires_grad_(True)
            p1, c1 = SdfPenalty(scenes[s], weights=w, margin=0.02, power=2)(one, want_count=True)
            p1.backward(g_pen[rows])
            assert (p1 > 0).all() and (one.grad != 0).any()
            assert torch.equal(pen[rows], p1) and torch.equal(cnt[rows], c1) and torch.equal(pts.grad[rows], one.grad), (a, s)
        else:
            assert (pen[rows] == 0).all() and (cnt[rows] == -1).all() and (pts.grad[rows] == 0).all(), (a, s)
    with pytest.raises(ValueError):
        op(pts0)                                                        # a set needs agent_scene
    with pytest.raises(ValueError):
        op(pts0, agent_scene=agent_scene, frames_per_agent=2)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the chain body points -> penalty
# ---------------------------------------------------------------------------------------------------------------------------
def test_penalty_behind_body_points_reaches_xb_and_betas():
    from egogen_amd.body_model import BodyPoints
    from egogen_amd.scene_sdf import SdfPenalty
    c = ref.chain_case()
    sc = ref.fit_scene()
    op = SdfPenalty(_scene(sc["sdf"], sc["center"], sc["scale"]), margin=c.margin, power=c.power)
    bp = BodyPoints(bref.body(), c.vids)
    xb, betas = c.xb.cuda().requires_grad_(True), c.betas.cuda().requires_grad_(True)
    pen = op(bp(xb, betas))
    (pen * c.g_pen.cuda()).sum().backward()
    assert xb.grad.shape == (c.B, 93) and betas.grad.shape == (c.B, 10)
    err = c.error(xb.grad, betas.grad)
    p64, p32 = c.pen[torch.float64], c.pen[torch.float32].double()
    ep, ep32 = float((pen.detach().cpu().double() - p64).abs().max()), float((p32 - p64).abs().max())
    ref.emit(c.table(err) + [f"penalty: max {float(p64.max()):.3e}  |f32-f64| {ep32:.3e}  |hip-f64| {ep:.3e}"])
    assert float(p64.min()) > 0                                         # every body reaches into the box
    for k in bref.GROUPS:
        assert err[k] <= ref.R * c.err32[k], (k, err[k], c.err32[k])


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the scene-aware fit
# ---------------------------------------------------------------------------------------------------------------------------
def test_fit_markers_next_to_a_box_keeps_the_body_out_and_agrees_with_the_cpu_loop():
    """CPU float64 (torch-op body): without the term 3.2 mm marker distance and a mean penalty of 3.0e-2; with it 16 mm and 1.2e-4."""
    from egogen_amd.body_model import BodyPoints
    from egogen_amd.fit import fit_markers
    from egogen_amd.scene_sdf import SdfPenalty
    _, hist_off, pene_off = ref.fit_on_cpu(torch.float64, 0.0)
    _, hist64, pene64 = ref.fit_on_cpu(torch.float64, ref.FIT_WEIGHT)
    sc = ref.fit_scene()
    op = SdfPenalty(_scene(sc["sdf"], sc["center"], sc["scale"]), margin=ref.FIT_MARGIN, power=ref.FIT_POWER)
    markers, collide = BodyPoints(bref.body(), bref.marker_vids()), BodyPoints(bref.body(), ref.fit_collision_vids())
    betas, xt, xb0 = (t.cuda() for t in ref.fit_setup())
    target = markers(xt, betas)
    xb, hist, pene = fit_markers(markers, target, betas, xb0, steps=ref.FIT_STEPS, lr=ref.FIT_LR, collision_model=collide, penalty=op,
                                 weight_pene=ref.FIT_WEIGHT)
    assert xb.is_cuda and hist.shape == (ref.FIT_STEPS + 1,) and pene.shape == (8,) and not pene.requires_grad
    p, p64, p_off = float(pene.mean()), float(pene64.mean()), float(pene_off.mean())
    ref.emit(["# fit_markers next to the unit box, 8 bodies, 150 steps (MI355X against the CPU float64 loop)",
              f"without the term (cpu float64): distance {hist_off[-1] * 1e3:.3f} mm, mean penalty {p_off:.4e}",
              f"with the term    (cpu float64): distance {hist64[-1] * 1e3:.3f} mm, mean penalty {p64:.4e}",
              f"with the term    (hip):         distance {hist[-1] * 1e3:.3f} mm, mean penalty {p:.4e}",
              f"relative difference hip / cpu float64: distance {abs(hist[-1] - hist64[-1]) / hist64[-1]:.2e}, penalty {abs(p - p64) / p64:.2e}"])
    assert p <= 0.05 * p_off, (p, p_off)
    assert abs(hist[-1] - hist64[-1]) <= 0.01 * hist64[-1], (hist[-1], hist64[-1])
    assert abs(p - p64) <= 0.01 * p64, (p, p64)
