"""Differentiable body points on the device (`BodyPoints`: egx_points_forward / egx_points_backward) against torch autograd of the
oracle in float64 (tests/body_points_ref.py).

Positions are held to the project's 2e-5 m.  Gradients are held, per output group, to R = 3 times the distance of the float32
oracle from the float64 one.  Every gradient test prints max|hip - f64| per group next to its ratio to max|f32 - f64|;
EGX_POINTS_TABLE=<file> appends the tables to a file (committed in profiles/body_points.md)."""
import os

import numpy as np
import pytest
import torch

from tests import body_points_ref as ref
from tests.helpers import load_golden, max_abs, rebuild_state_dict

pytestmark = pytest.mark.gpu

POS_TOL = 2e-5


@pytest.fixture(scope="module")
def marker_points():
    from egogen_amd.body_model import BodyPoints
    return BodyPoints(ref.body(), ref.marker_vids())


def _hip_grads(bp, c, variant, xb=None, betas=None):
    """(grad_xb, grad_betas) of sum(points * g_points) + sum(joints55 * g_joints) with the cotangents of the variant."""
    xb = (c.xb.cuda() if xb is None else xb).requires_grad_(True)
    betas = (c.betas.cuda() if betas is None else betas).requires_grad_(True)
    gp, gj = c.cotangents(variant)
    points, joints = bp(xb, betas, c.fpa, want_joints=True)
    outs, cots = [], []
    if gp is not None:
        outs.append(points), cots.append(gp.cuda())
    if gj is not None:
        outs.append(joints), cots.append(gj.cuda())
    torch.autograd.backward(outs, cots)
    return xb.grad, betas.grad


def _check(c, variant, g_xb, g_betas):
    err = c.error(variant, g_xb, g_betas)
    ref.emit(ref.table(c, variant, err))
    for k, e in err.items():
        assert e <= c.bound(variant, k), (c.name, variant, k, e, c.bound(variant, k))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,fpa", ref.BATCHES)
def test_forward_matches_oracle_and_the_fused_lbs_markers(marker_points, B, fpa):
    from egogen_amd.body_model import BodyModelHandle
    c = ref.case(B, fpa)
    xb, betas = c.xb.cuda(), c.betas.cuda()
    points, joints = marker_points(xb, betas, fpa, want_joints=True)
    only = marker_points(xb, betas, fpa)
    assert points.shape == (B, 67, 3) and joints.shape == (B, 55, 3) and points.grad_fn is None
    assert torch.equal(only, points)
    ep, ej = max_abs(points.cpu().double(), c.points64), max_abs(joints.cpu().double(), c.joints64)
    print(f"forward {c.name}: max|points - f64| = {ep:.2e}, max|joints55 - f64| = {ej:.2e}")
    assert ep <= POS_TOL and ej <= POS_TOL
    h = BodyModelHandle(ref.body(), ref.marker_vids())
    markers = h.forward(xb, betas, fpa, want_joints=False, want_markers=True)["markers"]
    assert max_abs(points.cpu(), markers.cpu()) <= POS_TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 2. / 3. gradients
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ref.VARIANTS)
@pytest.mark.parametrize("B,fpa", ref.BATCHES)
def test_gradients_within_three_times_the_float32_oracle(marker_points, B, fpa, variant):
    """(12, 4) is the shared shape: betas.grad is [3,10], the oracle's with betas.repeat_interleave(4, 0)."""
    c = ref.case(B, fpa)
    g_xb, g_betas = _hip_grads(marker_points, c, variant)
    assert g_xb.shape == (B, 93) and g_betas.shape == (B // fpa, 10)
    _check(c, variant, g_xb, g_betas)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. point sets
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fingertip", "random200", "full1024"])
def test_point_sets(name):
    from egogen_amd.body_model import BodyPoints
    V = 2048 if name == "full1024" else 640
    vids = {"fingertip": ref.fingertip_vid, "random200": ref.random_vids,
            "full1024": lambda: ref.random_vids(2048, 1024, seed=12)}[name]()
    assert len(vids) == {"fingertip": 1, "random200": 200, "full1024": 1024}[name]
    assert name == "fingertip" or (0 in vids and V - 1 in vids and len(set(vids)) < len(vids))
    c = ref.case(2, 1, vids, V)
    bp = BodyPoints(ref.body(V), vids)
    assert bp.P == len(vids)
    points = bp(c.xb.cuda(), c.betas.cuda())
    assert max_abs(points.cpu().double(), c.points64) <= POS_TOL
    for variant in ref.VARIANTS:
        _check(c, variant, *_hip_grads(bp, c, variant))


def test_point_set_limits():
    from egogen_amd._lib import EgxError
    from egogen_amd.body_model import BodyPoints
    bm = ref.body()
    for vids in (list(range(640)) + list(range(385)), [3, 640], [3, -1]):
        with pytest.raises(EgxError):
            BodyPoints(bm, vids)
    with pytest.raises(ValueError):
        BodyPoints(bm, [])
    assert BodyPoints(bm, list(range(640)) + list(range(384))).P == 1024


# ---------------------------------------------------------------------------------------------------------------------------
# 5. / 6. reproducibility and the autograd contract
# ---------------------------------------------------------------------------------------------------------------------------
def test_backward_is_bit_reproducible(marker_points):
    c = ref.case(37)
    a, b = _hip_grads(marker_points, c, "both"), _hip_grads(marker_points, c, "both")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_autograd_contract(marker_points):
    c = ref.case(5)
    xb, betas = c.xb.cuda().requires_grad_(True), c.betas.cuda()
    points = marker_points(xb, betas)
    points.backward(c.g_points.cuda())
    assert betas.grad is None and xb.grad is not None
    with torch.no_grad():
        assert marker_points(xb, betas).grad_fn is None
    assert marker_points(xb.detach(), betas).grad_fn is None
    # second order: the backward is once-differentiable
    xb2 = c.xb.cuda().requires_grad_(True)
    (g,) = torch.autograd.grad((marker_points(xb2, betas) * c.g_points.cuda()).sum(), xb2, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    with pytest.raises(ValueError):
        marker_points(xb[:, :90], betas)
    with pytest.raises(ValueError):
        marker_points(xb, betas[:3])


def test_stream_and_layout_do_not_change_the_result(marker_points):
    c = ref.case(5)
    base = _hip_grads(marker_points, c, "both")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = _hip_grads(marker_points, c, "both")
    s.synchronize()
    assert torch.equal(base[0], other[0]) and torch.equal(base[1], other[1])
    # a non-contiguous float64 xb: the gradient comes back in its layout and dtype
    wide = torch.zeros(5, 2 * 93, dtype=torch.float64, device="cuda")
    wide[:, ::2] = c.xb.cuda().double()
    xb = wide[:, ::2].detach().requires_grad_(True)
    assert not xb.is_contiguous()
    betas = c.betas.cuda().requires_grad_(True)
    points, joints = marker_points(xb, betas, want_joints=True)
    torch.autograd.backward([points, joints], [c.g_points.cuda(), c.g_joints.cuda()])
    assert xb.grad.dtype == torch.float64 and torch.equal(xb.grad.float(), base[0]) and torch.equal(betas.grad, base[1])


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the gradient the reference's own class recorded, full-size body
# ---------------------------------------------------------------------------------------------------------------------------
MCFG = {"body_repr": "ssm2_67", "h_dim": 128, "n_blocks": 10, "n_recur": 3, "actfun": "relu", "use_cont": True, "gender": "male",
        "seq_len": 10}


def test_train_op_with_hip_body_matches_reference_golden(tmp_path):
    """The bounds tests/test_train_regressor.py holds the torch path to."""
    from egogen_amd import synth
    from egogen_amd.train_regressor import GAMMARegressorTrainOP, HipMarkerBodyModel
    g = load_golden("regressor_train_ref.npz")
    bmd, mids = synth.make_body_model(int(g["body_model_seed"])), [int(v) for v in synth.marker_ids()]
    tc = {"log_dir": str(tmp_path / "logs"), "save_dir": str(tmp_path / "ckpt"), "batch_size": 4}
    with pytest.raises(ValueError):
        GAMMARegressorTrainOP(MCFG, {"weight_reg_hpose": 0.01}, dict(tc, marker_body_model="triton")).build_model(bmd, mids)
    op = GAMMARegressorTrainOP(MCFG, {"weight_reg_hpose": 0.01}, dict(tc, marker_body_model="hip"))
    op.build_model(bmd, mids)
    assert isinstance(op.bm, HipMarkerBodyModel)
    x_ref, betas = torch.from_numpy(g["marker_ref"]).cuda(), torch.from_numpy(g["betas"]).cuda()
    xb_in = torch.from_numpy(g["xb_in"]).cuda().requires_grad_(True)
    loss_b, items_b = op.calc_loss(x_ref, xb_in, betas)
    np.testing.assert_allclose(items_b, g["loss_b_items"], rtol=2e-5)
    loss_b.backward()
    err = max_abs(xb_in.grad.cpu(), g["dloss_dxb"])
    print(f"calc_loss, hip body: max|d loss / d xb - reference| = {err:.2e}")
    assert err < 1e-6
    # the full step
    sd = rebuild_state_dict(g, [int(g["fill_seed"])], [""], gains=[float(g["fill_gain"])])
    op.model.load_state_dict(sd)
    op.grads.attach()
    xb = op.model(x_ref, betas)
    op.grads.zero()
    loss, items = op.calc_loss(x_ref, xb, betas)
    np.testing.assert_allclose(items, g["loss_items"], rtol=5e-5)
    np.testing.assert_allclose(float(loss), float(g["loss"]), rtol=5e-5)
    loss.backward()
    params = dict(op.model.named_parameters())
    for k, n in zip([str(k) for k in g["grad_keys"]], g["grad_norm"]):
        got = float(params[k].grad.detach().norm())
        assert abs(got - n) <= 5e-3 * max(n, 1e-6) + 1e-8, (k, got, n)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. fitting
# ---------------------------------------------------------------------------------------------------------------------------
def test_fit_markers_on_the_device_agrees_with_the_cpu_loop(marker_points):
    from egogen_amd.fit import fit_markers
    _, hist64 = ref.fit_on_cpu(torch.float64)
    betas, xt, xb0 = (t.cuda() for t in ref.fit_setup())
    target = marker_points(xt, betas)
    xb, hist = fit_markers(marker_points, target, betas, xb0, steps=150, lr=0.02)
    print(f"fit_markers (hip): {hist[0]:.4f} m -> {hist[-1]:.4f} m; cpu float64: {hist64[0]:.4f} m -> {hist64[-1]:.4f} m")
    assert xb.is_cuda and hist.shape == (151,)
    assert hist[-1] <= 0.1 * hist[0]
    assert abs(hist[-1] - hist64[-1]) <= 0.01 * hist64[-1], (hist[-1], hist64[-1])


# ---------------------------------------------------------------------------------------------------------------------------
# 9. the training loop of test_training_loop_fits_markers_and_writes_reference_checkpoint with the fused body
# ---------------------------------------------------------------------------------------------------------------------------
def test_training_loop_with_hip_body_fits_markers(tmp_path):
    from egogen_amd import synth
    from egogen_amd.models import MoshRegressor
    from egogen_amd.train_predictor import write_canonicalized_primitive
    from egogen_amd.train_regressor import BatchGeneratorAMASSCanonicalized, GAMMARegressorTrainOP, MarkerBodyModel
    bmd, mids = synth.make_body_model(0), [int(v) for v in synth.marker_ids()]
    mbm = MarkerBodyModel(bmd, mids)
    rng = np.random.default_rng(1)
    root = tmp_path / "data" / "locomotion"
    os.makedirs(root)
    T = 10
    for i in range(16):
        xb = np.zeros((T, 93), np.float32)
        xb[:, :3] = rng.normal(0, 0.05, (1, 3)) + np.cumsum(rng.normal(0, 0.01, (T, 3)), 0)
        xb[:, 3:69] = rng.normal(0, 0.1, (1, 66)) + np.cumsum(rng.normal(0, 0.01, (T, 66)), 0)
        betas = rng.normal(0, 0.5, 16)
        with torch.no_grad():
            mk = mbm(torch.from_numpy(xb), torch.from_numpy(np.tile(betas[:10], (T, 1)).astype(np.float32))).numpy()
        poses = np.zeros((T, 156))
        poses[:, :66] = xb[:, 3:69]
        write_canonicalized_primitive(str(root / f"subseq_{i:05d}.npz"), trans=xb[:, :3], poses=poses, betas=betas,
                                      gender="male" if i % 4 else "female", marker_ssm2_67=mk, joints=rng.normal(0, 0.3, (T, 22, 3)))
    gen = BatchGeneratorAMASSCanonicalized(str(tmp_path / "data"), ["locomotion"], sample_rate=1, body_repr="ssm2_67")
    gen.get_rec_list(shuffle_seed=0)
    torch.manual_seed(0)
    op = GAMMARegressorTrainOP(MCFG, {"weight_reg_hpose": 0.01},
                               {"log_dir": str(tmp_path / "logs"), "save_dir": str(tmp_path / "ckpt"), "batch_size": 4, "num_epochs": 12,
                                "num_epochs_fix": 6, "learning_rate": 1e-3, "saving_per_X_ep": 6, "resume_training": False,
                                "marker_body_model": "hip"})
    op.build_model(bmd, mids)
    hist = op.train(gen)
    assert len(hist) == 12 and hist[-1][0] < 0.6 * hist[0][0], [h[0] for h in hist]
    ck = torch.load(str(tmp_path / "ckpt" / "epoch-12.ckp"), map_location="cpu")
    assert set(ck.keys()) == {"epoch", "model_state_dict", "optimizer_state_dict"} and ck["epoch"] == 12
    MoshRegressor(MCFG).load_state_dict(ck["model_state_dict"])             # strict: the reference's key set
