"""Combo training on the device: the three kernel families of csrc/combo.hip in isolation, then `GAMMAPrimitiveComboTrainOP`
against the fixture the reference's own class produced (tests/golden/combo_train_ref.npz) and against the float64 restatement
(tests/combo_ref.py), then the training loop and the driver.

Every kernel is held to the float64 evaluation of the torch expression it replaces, within R = 3 times the distance of the
float32 torch evaluation of that expression from float64, per output group.  The operator may be max(5e-5 relative, 3 x the
float32 restatement's distance) from float64 (combo_ref.yardstick).  The tests print every figure before asserting;
EGX_COMBO_TABLE=<file> appends them to a file (committed in profiles/combo_train.md)."""
import os

import numpy as np
import pytest
import torch

from tests import combo_ref
from tests.helpers import load_golden, max_abs
from tests.combo_ref import CASES, evaluated, fixture_world

pytestmark = pytest.mark.gpu
R = 3.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def emit(line):
    print(line)
    path = os.environ.get("EGX_COMBO_TABLE")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def held(name, group, got, truth64, f32):
    """|got - truth64| <= R |f32 - truth64| (largest entry of the group), printed before it is asserted."""
    t = torch.as_tensor(truth64, dtype=torch.float64)
    err = float((torch.as_tensor(got).double().cpu() - t).abs().max())
    e32 = float((torch.as_tensor(f32).double() - t).abs().max())
    emit(f"| {name} | {group} | {e32:.3e} | {err:.3e} | {err / e32 if e32 > 0 else float(err > 0):.2f} |")
    assert err <= R * e32, (name, group, err, e32)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. egx_cont6d_to_aa_backward
# ---------------------------------------------------------------------------------------------------------------------------
def _rotations(n, seed):
    """n x 22 rotations with angles 1e-3 .. 3.0 rad (the range of rot2aa_ref.npz) about random axes, float64 [n*22,3,3]."""
    g = torch.Generator().manual_seed(seed)
    m = n * 22
    axis = torch.randn(m, 3, generator=g, dtype=torch.float64)
    axis = axis / axis.norm(dim=1, keepdim=True)
    k = max(m - m // 8, 1)
    theta = torch.cat([torch.logspace(-3, 0.45, k, dtype=torch.float64), torch.linspace(2.0, 3.0, m - k, dtype=torch.float64)])
    theta = theta[torch.randperm(m, generator=g)]
    K = torch.zeros(m, 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    s, c = torch.sin(theta).view(-1, 1, 1), torch.cos(theta).view(-1, 1, 1)
    return torch.eye(3, dtype=torch.float64) + s * K + (1 - c) * (K @ K)


def _cont6d_inputs(n, seed):
    """xb6[n,159] (float32): first column of each rotation times a positive scale, second column times a positive scale plus a
    multiple of the first (non-orthogonal), in the (3,2) layout of RotConverter.cont2rotmat; random pass-through columns."""
    g = torch.Generator().manual_seed(seed + 1)
    Rm = _rotations(n, seed)
    m = Rm.shape[0]
    s1 = torch.rand(m, 1, generator=g, dtype=torch.float64) * 2.5 + 0.2
    s2 = torch.rand(m, 1, generator=g, dtype=torch.float64) * 2.5 + 0.2
    mix = torch.randn(m, 1, generator=g, dtype=torch.float64) * 0.7
    a1, a2 = Rm[:, :, 0] * s1, Rm[:, :, 1] * s2 + mix * Rm[:, :, 0]
    x6 = torch.stack([a1, a2], dim=-1).reshape(n, 132)
    xb6 = torch.cat([torch.randn(n, 3, generator=g, dtype=torch.float64), x6, torch.randn(n, 24, generator=g, dtype=torch.float64)], 1)
    return xb6.float(), torch.randn(n, 93, generator=g).float(), Rm


def _branches(Rm):
    """Which of the four quaternion branches (and whether w < 0) each rotation takes in rotation_matrix_to_quaternion on R^T."""
    m00, m11, m22 = Rm[:, 0, 0], Rm[:, 1, 1], Rm[:, 2, 2]
    neg_z, x_big, xy_neg = m22 < 1e-6, m00 > m11, m00 < -m11
    br = torch.where(neg_z & x_big, 0, torch.where(neg_z, 1, torch.where(xy_neg, 2, 3)))
    w = torch.stack([Rm[:, 2, 1] - Rm[:, 1, 2], Rm[:, 0, 2] - Rm[:, 2, 0], Rm[:, 1, 0] - Rm[:, 0, 1], torch.ones_like(m00)], 1)
    return br, w.gather(1, br.view(-1, 1)).view(-1) < 0


def _torch_tail_grad(xb6, g_out, dtype):
    from egogen_amd.train_regressor import cont6d_params_to_aa
    x = xb6.detach().clone().to(dtype).requires_grad_(True)
    out = cont6d_params_to_aa(x)
    out.backward(g_out.to(dtype))
    return out.detach(), x.grad


@pytest.mark.parametrize("n", [1, 5, 300])
def test_cont6d_backward_within_three_times_float32(n):
    from egogen_amd.fused_ops import Cont6dToAaFn
    xb6, g_out, Rm = _cont6d_inputs(n, 40 + n)
    if n == 300:
        br, wneg = _branches(Rm)
        assert sorted(set(br.tolist())) == [0, 1, 2, 3] and bool(wneg.any()) and bool((~wneg).any())
    out64, g64 = _torch_tail_grad(xb6, g_out, torch.float64)
    out32, g32 = _torch_tail_grad(xb6, g_out, torch.float32)
    x = xb6.detach().cuda().requires_grad_(True)
    out = Cont6dToAaFn.apply(x)
    out.backward(g_out.cuda())
    got = x.grad.cpu()
    assert torch.isfinite(got).all()
    held(f"cont6d_to_aa_backward n={n}", "rotation columns", got[:, 3:135], g64[:, 3:135], g32[:, 3:135])
    # pass-through columns: the incoming gradient, bit for bit
    assert torch.equal(got[:, :3], g_out[:, :3]) and torch.equal(got[:, 135:], g_out[:, 69:])
    assert torch.isfinite(out).all() and out32.shape == out.shape and out64.shape == out.shape
    again = torch.empty_like(x.grad)
    from egogen_amd import _lib
    _lib.check(_lib.load().egx_cont6d_to_aa_backward(_lib.ptr(x.detach()), _lib.ptr(g_out.cuda()), n, _lib.ptr(again), None), "bwd")
    assert torch.equal(again, x.grad)                       # same bits on the same inputs


def test_cont6d_backward_is_finite_at_the_exact_identity():
    from egogen_amd.fused_ops import Cont6dToAaFn
    xb6 = torch.zeros(2, 159)
    xb6[:, 3:135] = torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0, 0.0]).repeat(22)      # (3,2): columns e1, e2
    xb6[1, 3:135] *= 2.5                                                          # a scaled identity is the identity too
    x = xb6.cuda().requires_grad_(True)
    out = Cont6dToAaFn.apply(x)
    assert float(out.detach()[:, 3:69].abs().max()) == 0.0
    out.backward(torch.ones(2, 93, device="cuda"))
    assert torch.isfinite(x.grad).all() and float(x.grad[:, 3:135].abs().max()) > 0
    # the limit of the float64 gradient along rotations that approach the identity (angle 1e-6: k = 2 to 1e-13)
    Rm = torch.eye(3, dtype=torch.float64).unsqueeze(0).clone()
    eps = 1e-6
    Rm[0, 0, 1], Rm[0, 1, 0] = -eps, eps
    near = torch.zeros(1, 159, dtype=torch.float64)
    near[0, 3:135] = torch.stack([Rm[0, :, 0], Rm[0, :, 1]], -1).reshape(6).repeat(22)
    _, g64 = _torch_tail_grad(near, torch.ones(1, 93, dtype=torch.float64), torch.float64)
    assert max_abs(x.grad[0].cpu(), g64[0]) < 1e-5


def test_cont6d_node_composes_behind_the_regressor(monkeypatch):
    """MoshRegressorTrain with its torch-op tail replaced by the node: the same output and, through torch.autograd, the same flat
    weight gradient as the select-based tail.  The tail is the last operation, so the network's forward is the same in both
    passes and no ReLU changes side; the two backward passes are one linear map applied to two cotangents that differ by the
    float32 rounding of the tail's own backward.  That rounding is below 1e-5 of the cotangent's size (the float32 torch tail is
    8.5e-6 from float64 on gradients of order one, test_cont6d_backward_within_three_times_float32), hence a relative L2 bound
    of 1e-5 on the whole buffer."""
    from egogen_amd import train_regressor as tr
    from egogen_amd.fused_ops import Cont6dToAaFn, FlatGrads
    from tests.helpers import seeded_prior_state_dict
    from egogen_amd.models import REGRESSOR_CFG
    model = tr.MoshRegressorTrain(REGRESSOR_CFG).cuda()
    model.load_state_dict({k[len("regressor."):]: v for k, v in seeded_prior_state_dict().items() if k.startswith("regressor.")})
    grads = FlatGrads(model)
    g = torch.Generator().manual_seed(9)
    markers, betas = (torch.randn(12, 67, 3, generator=g) * 0.4).cuda(), (torch.randn(12, 10, generator=g) * 0.5).cuda()
    cot = torch.randn(12, 93, generator=g).cuda()
    flats, outs = [], []
    for tail in (tr.cont6d_params_to_aa, Cont6dToAaFn.apply):
        monkeypatch.setattr(tr, "cont6d_params_to_aa", tail)
        grads.zero()
        out = model(markers, betas)
        (out * cot).sum().backward()
        flats.append(grads.flat.clone())
        outs.append(out.detach())
    assert max_abs(outs[0].cpu(), outs[1].cpu()) < 1e-5
    rel = float((flats[0] - flats[1]).norm() / flats[0].norm())
    emit(f"# regressor behind Cont6dToAaFn vs the torch tail: relative L2 of the flat gradient {rel:.3e}")
    assert float(flats[1].norm()) > 0 and rel <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------------
# 2. egx_primitive_loss_forward / _backward
# ---------------------------------------------------------------------------------------------------------------------------
W_REC, W_TD = 1.0, 3.0


def _loss_torch(Y, Yr, dtype, g=1.0):
    Y, Yr = Y.to(dtype), Yr.detach().clone().to(dtype).requires_grad_(True)
    rec = torch.nn.functional.l1_loss(Y, Yr)
    td = torch.nn.functional.l1_loss(Yr[1:] - Yr[:-1], Y[1:] - Y[:-1]) if Y.shape[0] > 1 else rec * 0
    loss = W_REC * rec + W_TD * td
    (loss * g).backward()
    return torch.stack([loss.detach(), rec.detach(), td.detach()]), Yr.grad


def _loss_hip(Y, Yr, g=1.0):
    from egogen_amd.fused_ops import PrimitiveLossFn
    Yd, Yrd = Y.cuda(), Yr.detach().cuda().requires_grad_(True)
    loss, items = PrimitiveLossFn.apply(Yd, Yrd, W_REC, W_TD)
    (loss * g).backward()
    assert float(loss) == float(items[0])
    return items.cpu(), Yrd.grad.cpu()


SHAPES = [(18, 3, 201), (2, 1, 3), (1, 2, 201), (18, 64, 201)]


@pytest.mark.parametrize("shape", SHAPES)
def test_primitive_loss_on_a_dyadic_grid_equals_float64(shape):
    """Inputs are multiples of 2^-10 below 4, so every difference is exact in float32 and float64 alike and the sums are exact
    in double: the value is the float64 one rounded once, the gradient the float64 one up to the rounding of its two scale
    factors.  Exact zeros of Y_rec - Y and of the td residual are placed on purpose (sign(0) = 0); no element is excluded."""
    T, b, D = shape
    g = torch.Generator().manual_seed(T * 1000 + b)
    Y = torch.randint(-2047, 2048, shape, generator=g).float() / 1024
    Yr = torch.randint(-2047, 2048, shape, generator=g).float() / 1024
    flat = torch.randperm(b * D, generator=g)
    zr = flat[: max(1, b * D // 7)]                          # zeros of Y_rec - Y in frame 0 (and in every third frame)
    Yr.view(T, -1)[::3, zr] = Y.view(T, -1)[::3, zr]
    if T > 1:                                                # zeros of the td residual: the same offset in two consecutive frames
        zt = flat[-max(1, b * D // 5):]
        for t in range(0, T - 1, 2):
            off = torch.randint(-1024, 1025, (zt.numel(),), generator=g).float() / 1024
            off[0] = 0.0                                     # one element where Y_rec - Y and the td residual vanish together
            Yr.view(T, -1)[t, zt] = Y.view(T, -1)[t, zt] + off
            Yr.view(T, -1)[t + 1, zt] = Y.view(T, -1)[t + 1, zt] + off
        D_res = (Yr[1:] - Yr[:-1]) - (Y[1:] - Y[:-1])
        assert int((D_res == 0).sum()) >= zt.numel()
    assert int((Yr == Y).sum()) >= zr.numel()
    gscale = 0.375                                           # dyadic: the incoming gradient is the same number in both formats
    items64, g64 = _loss_torch(Y, Yr, torch.float64, gscale)
    items, grad = _loss_hip(Y, Yr, gscale)
    emit(f"| primitive_loss dyadic {shape} | value | float64 {items64.tolist()} | hip {items.tolist()} | |")
    assert torch.equal(items, items64.float())               # rounded once
    if T == 1:
        assert float(items[2]) == 0.0 and float(items[0]) == float(items[1])
    # float64 gradient = a s1 + c k with a = g w_rec / N, c = g w_td / N_td; float32 rounds a, c (2^-24 relative each) and the sum
    N, Ntd = T * b * D, (T - 1) * b * D
    a, c = gscale * W_REC / N, (gscale * W_TD / Ntd if Ntd else 0.0)
    s1 = torch.sign(Yr - Y).double()
    k = torch.zeros(shape, dtype=torch.float64)
    if T > 1:
        sd = torch.sign((Yr[1:] - Yr[:-1]) - (Y[1:] - Y[:-1])).double()
        k[1:] += sd
        k[:-1] -= sd
    assert max_abs(g64, a * s1 + c * k) <= 1e-18
    bound = 2.0 ** -24 * (a * s1.abs() + c * k.abs() + g64.abs()) * 1.0000001
    excess = ((grad.double() - g64).abs() - bound).max()
    emit(f"| primitive_loss dyadic {shape} | gradient | max |hip - f64| {float((grad.double() - g64).abs().max()):.3e} | worst excess over "
         f"the rounding of the scale factors {float(excess):.3e} | |")
    assert float(excess) <= 0.0
    zero = (s1 == 0) & (k == 0)
    assert bool(zero.any()) and float(grad[zero].abs().max()) == 0.0
    items2, grad2 = _loss_hip(Y, Yr, gscale)
    assert torch.equal(items, items2) and torch.equal(grad, grad2)      # two calls, the same bits


@pytest.mark.parametrize("shape", SHAPES)
def test_primitive_loss_on_random_inputs_within_three_times_float32(shape):
    g = torch.Generator().manual_seed(shape[0] + 7 * shape[1])
    Y = torch.randn(shape, generator=g) * 0.6
    Yr = Y + torch.randn(shape, generator=g) * 0.05
    items64, g64 = _loss_torch(Y, Yr, torch.float64)
    items32, g32 = _loss_torch(Y, Yr, torch.float32)
    items, grad = _loss_hip(Y, Yr)
    for i, name in enumerate(("loss", "rec", "td")):
        held(f"primitive_loss random {shape}", name, items[i], items64[i], items32[i])
    held(f"primitive_loss random {shape}", "gradient", grad, g64, g32)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. egx_primitive_reseed
# ---------------------------------------------------------------------------------------------------------------------------
def _reseed_torch(joints, X_prev, Yg, R_prev, T_prev, dtype):
    from oracle.env import get_new_coordinate
    joints, X_prev, Yg, R_prev, T_prev = (t.to(dtype) for t in (joints, X_prev, Yg, R_prev, T_prev))
    t_his, b = X_prev.shape[:2]
    R_, T_ = get_new_coordinate(joints)
    R_curr = torch.einsum("bij,bjk->bik", R_prev, R_)
    T_curr = torch.einsum("bij,bpj->bpi", R_prev, T_) + T_prev
    X = torch.einsum("bij,tbpj->tbpi", R_.permute(0, 2, 1), X_prev.reshape(t_his, b, -1, 3) - T_.unsqueeze(0)).reshape(t_his, b, -1)
    Y = torch.einsum("bij,tbpj->tbpi", R_curr.permute(0, 2, 1), Yg.reshape(Yg.shape[0], b, -1, 3) - T_curr.unsqueeze(0)).reshape(Yg.shape[0], b, -1)
    return {"X": X, "Y": Y, "R_curr": R_curr, "T_curr": T_curr, "R_": R_, "T_": T_}


@pytest.mark.parametrize("b", [1, 3, 67])
def test_primitive_reseed_within_three_times_float32(b):
    from egogen_amd.fused_ops import primitive_reseed
    g = torch.Generator().manual_seed(70 + b)
    joints = torch.randn(b, 55, 3, generator=g) * 0.4 + torch.tensor([0.3, -0.2, 0.9])
    X_prev, Yg = torch.randn(2, b, 201, generator=g) * 0.5, torch.randn(18, b, 201, generator=g) * 0.8 + 1.5
    yaw = torch.rand(b, generator=g) * 6.28
    R_prev = torch.zeros(b, 3, 3)
    R_prev[:, 0, 0], R_prev[:, 0, 1], R_prev[:, 1, 0], R_prev[:, 1, 1], R_prev[:, 2, 2] = yaw.cos(), -yaw.sin(), yaw.sin(), yaw.cos(), 1.0
    T_prev = torch.randn(b, 1, 3, generator=g)
    ref64 = _reseed_torch(joints, X_prev, Yg, R_prev, T_prev, torch.float64)
    ref32 = _reseed_torch(joints, X_prev, Yg, R_prev, T_prev, torch.float32)
    out = primitive_reseed(*(t.cuda() for t in (joints, X_prev, Yg, R_prev, T_prev)))
    got = dict(zip(("X", "Y", "R_curr", "T_curr", "R_", "T_"), out))
    for k in ("R_", "T_", "R_curr", "T_curr", "X", "Y"):
        assert got[k].shape == ref32[k].shape, k
        held(f"primitive_reseed b={b}", k, got[k], ref64[k], ref32[k])
    assert torch.equal(got["T_"].cpu(), joints[:, :1])
    again = primitive_reseed(*(t.cuda() for t in (joints, X_prev, Yg, R_prev, T_prev)))
    assert all(torch.equal(u, v) for u, v in zip(out, again))


def test_primitive_reseed_frame_matches_the_reference_golden():
    """R_, T_ against CanonicalCoordinateExtractor.get_new_coordinate_torch's own outputs (canon_ref.npz), as egx_canonical_frame is
    held (tests/test_boundary_gpu.py); with identity R_prev and zero T_prev the current frame is that frame."""
    from egogen_amd.fused_ops import primitive_reseed
    g = load_golden("canon_ref.npz")
    j = torch.from_numpy(g["jts"]).cuda()
    B = j.shape[0]
    X_prev, Yg = torch.zeros(2, B, 201, device="cuda"), torch.zeros(18, B, 201, device="cuda")
    _, _, R_curr, T_curr, R_, T_ = primitive_reseed(j, X_prev, Yg, torch.eye(3, device="cuda").repeat(B, 1, 1), torch.zeros(B, 1, 3, device="cuda"))
    assert max_abs(R_.cpu(), g["R"]) < 1e-6 and max_abs(T_.cpu(), g["T"]) == 0.0
    assert torch.equal(R_curr, R_) and torch.equal(T_curr, T_)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the operator against the fixture and the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _op(tmp_path, g, sd, bmd, mids, **train_kw):
    from egogen_amd.models import PREDICTOR_CFG, REGRESSOR_CFG
    from egogen_amd.train_combo import GAMMAPrimitiveComboTrainOP
    tc = dict({"log_dir": str(tmp_path / "logs"), "save_dir": str(tmp_path / "ckpt"), "batch_size": 2, "num_epochs": 10, "max_rollout": 8,
               "learning_rate": 3e-4}, **train_kw)
    op = GAMMAPrimitiveComboTrainOP({"modelconfig": PREDICTOR_CFG}, {"modelconfig": dict(REGRESSOR_CFG, gender="male")},
                                    dict(combo_ref.LOSS_CFG), tc)
    op.build_model(body_model=bmd, markers=mids)
    op.model.load_state_dict(sd)
    op.grads.attach()
    return op


def _recorded(op, case):
    """Wrap the operator's `forward` and `_reseed` so that a call leaves Y_rec and Xb_rec (per primitive also the seed X and the
    frame R_curr, T_curr) behind, as scripts/gen_combo_golden.py wraps the reference class.  The frame of primitive 0 is what
    the first re-seeding is handed."""
    rec = {"Y_rec": [], "Xb_rec": []} if case == "one" else {"Y_rec": [], "Xb_rec": [], "X": [], "R_curr": [], "T_curr": []}
    forward, reseed = op.forward, op._reseed

    def forward_rec(X, Y, betas, eps=None, **kw):
        out = forward(X, Y, betas, eps, **kw)
        rec["Y_rec"].append(out[0].detach().cpu())
        rec["Xb_rec"].append(out[3].detach().cpu())
        if "X" in rec:
            rec["X"].append(X.detach().cpu())
        return out

    def reseed_rec(Y_rec, Yb_rec, betas_Y, Yg, R_prev, T_prev):
        if not rec["R_curr"]:
            rec["R_curr"].append(R_prev.cpu())
            rec["T_curr"].append(T_prev.cpu())
        out = reseed(Y_rec, Yb_rec, betas_Y, Yg, R_prev, T_prev)
        rec["R_curr"].append(out[2].cpu())
        rec["T_curr"].append(out[3].cpu())
        return out

    op.forward, op._reseed = forward_rec, reseed_rec
    return rec


def _run_case(op, g, case):
    dev = lambda name: torch.from_numpy(g[name]).cuda()
    rec = _recorded(op, case)
    op.grads.zero()
    if case == "one":
        loss, items = op.calc_loss_one([dev("one_betas"), dev("one_markers")], 0, eps=dev("one_eps"))
    else:
        loss, items = op.calc_loss_rollout([dev("roll_betas"), dev("roll_markers"), None, None, None, dev("roll_jts")], 0,
                                           eps_list=list(dev(case + "_eps")))
    loss.backward()
    grads = {k: p.grad.detach().cpu().clone() for k, p in op.model.named_parameters() if k.startswith("predictor.")}
    return items, grads, {k: (v[0] if case == "one" else torch.stack(v)) for k, v in rec.items()}


def _stack(rec, k):
    return torch.stack(list(rec[k])) if isinstance(rec[k], list) else rec[k]


def _heads(grads, keys):
    return np.stack([np.resize(grads[k].flatten()[:8].numpy(), 8) for k in keys])


@pytest.mark.parametrize("case", CASES)
def test_operator_matches_the_reference_class_and_float64(tmp_path, case):
    """calc_loss_one and both rollouts: Y_rec, Xb_rec, seeds and frames of every primitive, the four loss items, and per predictor
    parameter the gradient norm and head - the HIP path (fused, and the torch-op composition `fused=False`) may be
    max(5e-5 relative, 3 x the float32 restatement's distance) from the float64 restatement; so may the fixture (CPU test).
    The two legs are then held to each other, group by group, within that same bound."""
    g, sd, bmd, mids = fixture_world()
    items64, grads64, rec64 = evaluated(case, torch.float64)
    items32, grads32, rec32 = evaluated(case, torch.float32)
    keys = list(grads64.keys())
    n64, n32 = (np.array([float(v[k].norm()) for k in keys]) for v in (grads64, grads32))
    h64, h32 = _heads(grads64, keys), _heads(grads32, keys)
    groups = [k for k in ("Y_rec", "Xb_rec", "X", "R_curr", "T_curr") if k in rec64]
    bound_item = [combo_ref.yardstick(items64[i], items32[i]) for i in range(4)]
    bound_rec = {k: combo_ref.yardstick(_stack(rec64, k), _stack(rec32, k)) for k in groups}
    bound_norm = np.maximum(5e-5, R * np.abs(n32 - n64) / n64)                # relative, per parameter
    bound_head = combo_ref.yardstick(h64, h32)
    results = {}
    for fused in (True, False):
        op = _op(tmp_path / str(fused), g, sd, bmd, mids, scheduled_sampling=(case != "one"), use_Yproj_as_seed=(case == "roll_proj"),
                 fused=fused)
        items, grads, rec = _run_case(op, g, case)
        assert sorted(rec) == sorted(groups)
        tag = f"operator {case} {'fused' if fused else 'torch-op glue'}"
        assert all(p.grad is None for p in op.model.regressor.parameters())
        for i, name in enumerate(("REC", "KLD", "REG", "HPOSE")):
            err = abs(float(items[i]) - float(items64[i]))
            emit(f"| {tag} | {name} | {abs(float(items32[i]) - float(items64[i])):.3e} | {err:.3e} | bound {bound_item[i]:.3e} |")
            assert err <= bound_item[i], (tag, name, err, bound_item[i])
            # the fixture is within one bound of float64 too (CPU test), so this follows from the line above; it is kept as
            # the direct comparison with what the reference class computed
            assert abs(float(items[i]) - float(g[case + "_items"][i])) <= 2 * bound_item[i], (tag, name)
        for k in groups:
            t64 = _stack(rec64, k)
            err = max_abs(rec[k], t64)
            emit(f"| {tag} | {k} | {max_abs(_stack(rec32, k), t64):.3e} | {err:.3e} | bound {bound_rec[k]:.3e} |")
            assert err <= bound_rec[k], (tag, k, err, bound_rec[k])
        got_n, got_h = np.array([float(grads[k].norm()) for k in keys]), _heads(grads, keys)
        rel = np.abs(got_n - n64) / n64
        emit(f"| {tag} | gradient norms (max rel) | {(np.abs(n32 - n64) / n64).max():.3e} | {rel.max():.3e} | bound max(5e-5, 3 x f32) per parameter |")
        assert (rel <= bound_norm).all(), (tag, keys[int(np.argmax(rel / bound_norm))], rel.max())
        emit(f"| {tag} | gradient heads | {max_abs(h32, h64):.3e} | {max_abs(got_h, h64):.3e} | bound {bound_head:.3e} |")
        assert max_abs(got_h, h64) <= bound_head, tag
        results[fused] = (items, rec, got_n, got_h)
    # fused against the torch-op glue: every group above, within the same bound (one bound, not one per leg)
    (items_f, rec_f, n_f, h_f), (items_t, rec_t, n_t, h_t) = results[True], results[False]
    tag = f"operator {case} fused vs torch-op glue"
    for i, name in enumerate(("REC", "KLD", "REG", "HPOSE")):
        d = abs(float(items_f[i]) - float(items_t[i]))
        emit(f"| {tag} | {name} | | {d:.3e} | bound {bound_item[i]:.3e} |")
        assert d <= bound_item[i], (tag, name, d, bound_item[i])
    for k in groups:
        d = max_abs(rec_f[k], rec_t[k])
        emit(f"| {tag} | {k} | | {d:.3e} | bound {bound_rec[k]:.3e} |")
        assert d <= bound_rec[k], (tag, k, d, bound_rec[k])
    rel = np.abs(n_f - n_t) / n64
    emit(f"| {tag} | gradient norms (max rel) | | {rel.max():.3e} | bound max(5e-5, 3 x f32) per parameter |")
    assert (rel <= bound_norm).all(), (tag, keys[int(np.argmax(rel / bound_norm))], rel.max())
    emit(f"| {tag} | gradient heads | | {max_abs(h_f, h_t):.3e} | bound {bound_head:.3e} |")
    assert max_abs(h_f, h_t) <= bound_head, tag


def test_regressor_is_frozen_and_saved(tmp_path):
    """Adam visits the predictor only (:1025): after a step the regressor's parameters are bit-identical, none of them is in the
    optimiser, none has a gradient, and the predictor's have moved."""
    g, sd, bmd, mids = fixture_world()
    op = _op(tmp_path, g, sd, bmd, mids)
    before = {k: v.detach().clone() for k, v in op.model.state_dict().items()}
    opt = torch.optim.Adam(op.model.predictor.parameters(), lr=1e-3)
    dev = lambda name: torch.from_numpy(g[name]).cuda()
    loss, _ = op.calc_loss_one([dev("one_betas"), dev("one_markers")], 0, eps=dev("one_eps"))
    op.step(opt, loss)
    after = op.model.state_dict()
    reg_ids = {id(p) for p in op.model.regressor.parameters()}
    assert not any(id(p) in reg_ids for grp in opt.param_groups for p in grp["params"])
    assert all(p.grad is None and not p.requires_grad for p in op.model.regressor.parameters())
    assert all(torch.equal(before[k], after[k]) for k in before if k.startswith("regressor."))
    assert any(not torch.equal(before[k], after[k]) for k in before if k.startswith("predictor."))
    assert {k.split(".")[0] for k in after} == {"predictor", "regressor"}


# ---------------------------------------------------------------------------------------------------------------------------
# 5. training loop, checkpoint, resume, driver
# ---------------------------------------------------------------------------------------------------------------------------
def _write_primitives(root, n_files, T, seed):
    """Canonicalised primitive files whose markers and joints come from the body model itself (smooth small motions)."""
    from egogen_amd import synth
    from egogen_amd.train_predictor import write_canonicalized_primitive
    from oracle.smplx_lbs import BodyModel, smplx_forward
    bmd, mids = synth.make_body_model(0), [int(v) for v in synth.marker_ids()]
    bm = BodyModel(bmd)
    rng = np.random.default_rng(seed)
    os.makedirs(root)
    for i in range(n_files):
        xb = np.zeros((T, 93), np.float32)
        xb[:, :3] = np.array([0.0, 0.0, 0.9]) + np.arange(T)[:, None] * np.array([0.0, 0.015, 0.0]) + np.cumsum(rng.normal(0, 0.003, (T, 3)), 0)
        xb[:, 3:69] = rng.normal(0, 0.08, (1, 66)) + np.cumsum(rng.normal(0, 0.01, (T, 66)), 0)
        betas = rng.normal(0, 0.5, 16)
        with torch.no_grad():
            v, j = smplx_forward(bm, torch.from_numpy(xb), torch.from_numpy(np.tile(betas[:10], (T, 1)).astype(np.float32)))
        poses = np.zeros((T, 156))
        poses[:, :66] = xb[:, 3:69]
        write_canonicalized_primitive(os.path.join(root, f"subseq_{i:05d}.npz"), trans=xb[:, :3], poses=poses, betas=betas, gender="male",
                                      marker_ssm2_67=v[:, mids].numpy(), joints=j[:, :22].numpy())
    return bmd, mids


def _pretrained(tmp_path, names=("pred", "reg")):
    """epoch-300.ckp / epoch-100.ckp of the two earlier stages (seeded weights), where load_pretrained looks for them."""
    from tests.helpers import seeded_prior_state_dict
    sd = seeded_prior_state_dict(pred_gain=0.5, reg_gain=0.3)
    dirs = [str(tmp_path / n) for n in names]
    for d, prefix, ep in zip(dirs, ("predictor.", "regressor."), (300, 100)):
        os.makedirs(d, exist_ok=True)
        torch.save({"epoch": ep, "model_state_dict": {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}},
                   os.path.join(d, f"epoch-{ep}.ckp"))
    return dirs


def test_training_loop_lowers_reg_writes_reference_checkpoint_and_resumes(tmp_path):
    from egogen_amd.models import GAMMAPrimitiveCombo, PREDICTOR_CFG, REGRESSOR_CFG
    from egogen_amd.train_combo import GAMMAPrimitiveComboTrainOP
    from egogen_amd.train_regressor import BatchGeneratorAMASSCanonicalized
    bmd, mids = _write_primitives(str(tmp_path / "data" / "CMU"), 8, 20, seed=3)
    pdir, rdir = _pretrained(tmp_path)
    rcfg = dict(REGRESSOR_CFG, gender="male")

    def run(num_epochs, resume):
        gen = BatchGeneratorAMASSCanonicalized(str(tmp_path / "data"), ["CMU"], sample_rate=1, body_repr="ssm2_67")
        gen.get_rec_list(shuffle_seed=0)
        tc = {"log_dir": str(tmp_path / "logs"), "save_dir": str(tmp_path / "ckpt"), "batch_size": 4, "num_epochs": num_epochs,
              "num_epochs_fix": 3, "learning_rate": 1e-3, "saving_per_X_ep": 3, "resume_training": resume}
        op = GAMMAPrimitiveComboTrainOP({"modelconfig": PREDICTOR_CFG, "trainconfig": {"save_dir": pdir}},
                                        {"modelconfig": rcfg, "trainconfig": {"save_dir": rdir}}, dict(combo_ref.LOSS_CFG), tc)
        op.build_model(load_pretrained=not resume, body_model=bmd, markers=mids)
        torch.manual_seed(0)
        return op, op.train(gen)

    op, hist = run(6, False)
    reg = [h[2] for h in hist]
    emit(f"# training loop, 6 epochs of calc_loss_one on 8 synthetic primitives: REG {['%.4f' % v for v in reg]}")
    assert len(hist) == 6 and reg[-1] < reg[0], reg
    ck = torch.load(str(tmp_path / "ckpt" / "epoch-6.ckp"), map_location="cpu")
    assert set(ck.keys()) == {"epoch", "model_state_dict", "optimizer_state_dict"} and ck["epoch"] == 6
    assert {k.split(".")[0] for k in ck["model_state_dict"]} == {"predictor", "regressor"}
    combo = GAMMAPrimitiveCombo(PREDICTOR_CFG, REGRESSOR_CFG)
    combo.load_state_dict(ck["model_state_dict"])                        # strict: the rollout's module reads this layout
    Y, Yb = combo.cuda().sample_prior(torch.randn(2, 3, 201, device="cuda") * 0.3, torch.zeros(3, 10, device="cuda"))
    assert torch.isfinite(Y).all() and torch.isfinite(Yb).all()
    pre = torch.load(os.path.join(rdir, "epoch-100.ckp"), map_location="cpu")["model_state_dict"]
    assert all(torch.equal(ck["model_state_dict"]["regressor." + k], v) for k, v in pre.items())   # frozen through training
    assert os.path.getsize(str(tmp_path / "logs" / "train.log")) > 0
    op2, hist2 = run(8, True)                                            # resume: epochs 7 and 8 only, from the optimiser state
    assert len(hist2) == 2 and os.path.exists(str(tmp_path / "ckpt" / "epoch-6.ckp"))
    assert hist2[0][2] < reg[0]


def test_combo_training_driver_runs_from_a_yaml(tmp_path):
    """exp_GAMMAPrimitive/train_GAMMACombo.py end to end on configs in the reference's yaml layout."""
    import subprocess
    import sys
    import yaml
    from egogen_amd.models import PREDICTOR_CFG, REGRESSOR_CFG
    _write_primitives(str(tmp_path / "data" / "CMU"), 4, 20, seed=5)
    res = tmp_path / "results" / "exp_GAMMAPrimitive"
    _pretrained(res, names=(os.path.join("MPVAE_samp20_2frame_rollout", "checkpoints"), os.path.join("MoshRegressor_v3_male", "checkpoints")))
    cfgdir = tmp_path / "crowd_ppo" / "cfg_samp20"
    os.makedirs(cfgdir)
    combo = {"modelconfig": {"predictor_config": "MPVAE_samp20_2frame_rollout", "regressor_config": "MoshRegressor_v3_male"},
             "lossconfig": dict(combo_ref.LOSS_CFG, use_cycle=False),
             "trainconfig": {"scheduled_sampling": False, "use_gt_transform": False, "ft_regressor": False, "use_Yproj_as_seed": False,
                             "max_rollout": 8, "learning_rate": 3e-4, "batch_size": 2, "num_epochs": 2, "num_epochs_fix": 1,
                             "saving_per_X_ep": 2, "sample_rate": 1, "dataset_path": str(tmp_path / "data"), "subsets": ["CMU"]}}
    for name, cfg in (("MPVAECombo_samp_2frame", combo), ("MPVAE_samp20_2frame_rollout", {"modelconfig": dict(PREDICTOR_CFG)}),
                      ("MoshRegressor_v3_male", {"modelconfig": dict(REGRESSOR_CFG, gender="male")})):
        with open(cfgdir / f"{name}.yml", "w") as fh:
            yaml.safe_dump(cfg, fh)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "exp_GAMMAPrimitive", "train_GAMMACombo.py"), "--cfg", "MPVAECombo_samp_2frame"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[epoch 2]" in r.stdout and "REG=" in r.stdout
    ck = torch.load(str(res / "MPVAECombo_samp_2frame" / "checkpoints" / "epoch-2.ckp"), map_location="cpu")
    assert ck["epoch"] == 2 and "predictor.d_out.weight" in ck["model_state_dict"] and "regressor.pnet.in_fc.weight" in ck["model_state_dict"]
