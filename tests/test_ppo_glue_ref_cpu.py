"""The references and input builders of tests/ppo_glue_ref.py, held to torch itself on the CPU: a GPU test that compares a
kernel with them (test_ppo_glue_gpu.py) is only as good as they are.  The builder's guarantees are conditions, not measurements."""
import math
import warnings

import pytest
import torch

from tests import ppo_glue_ref as pg

F32, F64 = torch.float32, torch.float64


# ---------------------------------------------------------------------------------------------------------------------------
# references against torch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_clip,max_norm", [(11, 6, 0.1), (5, 5, 0.1), (3, 0, 0.1), (11, 6, 0.0), (1025, 1023, 0.1)])
def test_restated_optimiser_is_torch_adamw(n, n_clip, max_norm):
    p0, grads, o64, _, coefs = pg.adamw_case(n, n_clip, max_norm)
    ref = pg.torch_adamw_steps(p0, grads, n_clip, max_norm, F64, **pg.ADAMW)
    for k in ("p", "m", "v"):
        assert torch.allclose(o64[k], ref[k], rtol=1e-12, atol=0.0), (k, float((o64[k] - ref[k]).abs().max()))
    if n_clip and max_norm > 0:      # the gradients are scaled so that the second step alone is clipped, with room to spare
        assert coefs[0] == 1.0 and coefs[2] == 1.0 and coefs[1] < 0.5, coefs
    else:
        assert coefs == [1.0, 1.0, 1.0]


@pytest.mark.parametrize("n,n_clip", pg.ADAMW_CASES)
def test_adamw_cases_clip_the_second_step_only(n, n_clip):
    p0, grads, o64, o32, coefs = pg.adamw_case(n, n_clip)
    norms = [float(torch.linalg.vector_norm(g[:n_clip].double())) for g in grads]
    if n_clip:
        assert norms[0] < 0.5 * pg.MAX_NORM and norms[2] < 0.5 * pg.MAX_NORM and norms[1] > 2 * pg.MAX_NORM, norms
        assert coefs[1] == pytest.approx(pg.MAX_NORM / (norms[1] + 1e-6), rel=1e-14)
    for k in ("p", "m", "v"):
        assert o64[k].shape == o32[k].shape == (n,)


def test_gru_reference_is_torch_grucell():
    g = torch.Generator().manual_seed(0)
    M, K, H = 5, 7, 6
    cell = torch.nn.GRUCell(K, H).double()
    x, h = torch.randn(M, K, generator=g, dtype=F64), torch.randn(M, H, generator=g, dtype=F64)
    gi = (x @ cell.weight_ih.t() + cell.bias_ih).detach()
    gh = (h @ cell.weight_hh.t() + cell.bias_hh).detach()
    assert torch.allclose(pg.gru_gates(gi, gh, h), cell(x, h).detach(), rtol=1e-13, atol=1e-15)
    # zero previous state: h_prev = None is h_prev = 0 (gh is then the bias alone)
    gh0 = cell.bias_hh.detach().expand(M, 3 * H)
    assert torch.allclose(pg.gru_gates(gi, gh0, None), cell(x, torch.zeros(M, H, dtype=F64)).detach(), rtol=1e-13, atol=1e-15)
    # backward: the closed form of the kernel's comment against autograd through the reference
    dh = torch.randn(M, H, generator=g, dtype=F64)
    o = pg.gru_gates_bwd(gi, gh, h, dh)
    r = torch.sigmoid(gi[:, :H] + gh[:, :H]); z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    dan = dh * (1 - z) * (1 - n * n)
    dar, daz = dan * gh[:, 2 * H:] * r * (1 - r), dh * (h - n) * z * (1 - z)
    assert torch.allclose(o["dgi"], torch.cat([dar, daz, dan], 1), rtol=1e-12, atol=1e-15)
    assert torch.allclose(o["dgh"], torch.cat([dar, daz, dan * r], 1), rtol=1e-12, atol=1e-15)
    assert torch.allclose(o["dh_prev"], dh * z, rtol=1e-12, atol=1e-15)
    assert "dh_prev" not in pg.gru_gates_bwd(gi, gh, None, dh)


def test_saturated_gates_agree_in_both_precisions():
    gi, gh, hp, dh = pg.gru_saturated()
    assert float(gi.abs().max()) == 90.0
    h64, h32 = pg.gru_gates(gi.double(), gh.double(), hp.double()), pg.gru_gates(gi, gh, hp)
    assert torch.isfinite(h32).all() and torch.equal(h32.double(), h64)
    H = hp.shape[1]
    r = torch.sigmoid(gi[:, :H] + gh[:, :H]); z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    for gate in (r, z):      # sigmoid(-45) = 2.9e-20: saturated means within 1e-19 of 0 or 1, on both sides
        assert float(torch.minimum(gate, 1 - gate).max()) < 1e-19 and float(gate.min()) < 0.5 < float(gate.max())


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_activation_reference_is_torch(act):
    F = torch.nn.functional
    fn = {0: lambda z: z, 1: torch.tanh, 2: torch.relu, 3: lambda z: F.leaky_relu(z, pg.SLOPE)}[act]
    z, res, dy = (t[:33, :65].double() for t in pg.act_master())
    zz = z.clone().requires_grad_(True)
    out = fn(zz) + res
    out.backward(dy)
    f = pg.act_fwd(z, res, act)
    assert torch.equal(f["out"], out.detach()) and torch.equal(f["a"], fn(z))
    assert torch.equal(pg.act_fwd(z, None, act)["out"], fn(z))
    b = pg.act_bwd(dy, f["a"], act)
    # the saved outputs hold +0.0 and -0.0: torch's backward gives relu 0 and leaky relu `slope` there, and so must the reference
    a = f["a"]
    if act in (2, 3):
        zero = a == 0
        neg0 = zero & torch.signbit(a)
        assert int(zero.sum()) > 0 and int((zero & ~torch.signbit(a)).sum()) > 0
        assert act == 2 or int(neg0.sum()) > 0          # relu's output has no -0.0; leaky relu's has
        want = 0.0 if act == 2 else pg.SLOPE
        assert torch.equal(zz.grad[zero], dy[zero] * want)
    assert torch.allclose(b["g"], zz.grad, rtol=1e-13, atol=1e-15)
    assert torch.allclose(b["db"], zz.grad.sum(0), rtol=1e-13, atol=1e-15)


def test_loss_reference_gradient_at_the_clamp_edges_and_clip_branches():
    """The reference is torch autograd; this pins the facts the kernel's branches rely on: the clamp passes gradient AT +-2.5 and
    blocks it beyond, and a clipped ratio on the side that the minimum selects carries no policy gradient."""
    m = pg.build_loss_inputs(30)
    args = tuple(m[k].double() for k in ("mu", "logvar", "value", "act", "adv", "ret", "logp_old"))
    o = pg.ppo_loss_ref(*args, None, 0.37)
    for r in range(30):
        c = pg.lv_edge_columns(r)
        assert o["g_logvar"][r, c[0]] != 0 and o["g_logvar"][r, c[1]] != 0
        assert o["g_logvar"][r, c[2]] == 0 and o["g_logvar"][r, c[3]] == 0
        t, s = float(m["target"][r]), float(m["sign"][r])
        blocked = (t == 2.0 and s > 0) or (t == 0.5 and s < 0) or s == 0
        assert bool((o["g_mu"][r] == 0).all()) == blocked, (r, t, s)
    assert torch.equal(o["g_value"], 0.37 * pg.VF_COEF * -2.0 * (args[5] - args[2]))
    # the six terms are scale * sum over rows of the oracle's means
    lv = args[1].clamp(pg.MIN_LV, pg.MAX_LV)
    ent = (0.5 + 0.5 * math.log(2 * math.pi) + 0.5 * lv).sum(-1)
    assert torch.allclose(o["terms"][3], 0.37 * ent.sum(), rtol=1e-13)
    assert torch.allclose(o["terms"][4], 0.37 * (0.5 * args[0] ** 2).sum() / 128, rtol=1e-13)
    assert torch.allclose(o["terms"][0], o["terms"][1] + pg.VF_COEF * o["terms"][2] - pg.ENT_COEF * o["terms"][3], rtol=1e-12)


def test_posenc_argument_is_exact_in_fp32():
    x = torch.tensor([0.0, 1.0, 0.3, 1e-3, 0.999, 16.0, 7.3])
    k = 2.0 ** torch.arange(32, dtype=F64)
    assert torch.equal((x[:, None] * k.float()[None]).double(), x.double()[:, None] * k[None])
    o = pg.posenc_ref(x.double(), x.double())["posenc"]
    assert o.shape == (7, 128) and torch.equal(o[:, :64], o[:, 64:])
    assert torch.equal(o[:, 0], torch.sin(x.double())) and torch.equal(o[:, 63], torch.cos(x.double() * 2.0 ** 31))


def test_adv_stats_and_bookkeeping_references():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(257, generator=g, dtype=F64)
    assert torch.allclose(pg.adv_stats_ref(a), torch.stack([a.mean(), a.std()]), rtol=1e-13)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # torch warns that one value has no degrees of freedom left
        assert torch.isnan(pg.adv_stats_ref(a[:1])[1]) and torch.isnan(a[:1].std())
    A = 300
    rew, term = torch.randn(A, generator=g), (torch.rand(A, generator=g) < 0.3).int()
    ep_ret, ep_len = torch.randn(A, generator=g), torch.randint(0, 9, (A,), generator=g).float()
    r, l, sums, mag = pg.track_episode_ref(rew, term, ep_ret, ep_len)
    d = term.bool()
    assert torch.equal(r[~d], (ep_ret + rew)[~d]) and bool((r[d] == 0).all()) and bool((l[d] == 0).all())
    assert torch.equal(l[~d], ep_len[~d] + 1)
    assert float(sums[2]) == int(d.sum()) > 0 and float(sums[1]) == float((ep_len + 1)[d].sum())
    assert float(sums[0]) == float((ep_ret + rew)[d].double().sum()) and bool((mag >= sums.abs()).all())


def test_ulp32_is_the_spacing_of_fp32():
    x = torch.tensor([1.0, 1.5, 1.9999, 2.0, 0.0149, 1e4], dtype=F64)
    want = torch.tensor([2.0 ** -23, 2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -30, 2.0 ** -10], dtype=F64)
    assert torch.equal(pg.ulp32(x), want) and torch.equal(pg.ulp32(-x), want)
    assert pg.ulp32(x[4]).shape == () and float(pg.ulp32(x[4])) == 2.0 ** -30
    assert pg.ulp32(x.reshape(2, 3)).shape == (2, 3)


def test_gae_reference_on_a_hand_case():
    v = torch.tensor([[1.0], [2.0], [3.0]])
    rew, term = torch.tensor([[0.5], [0.25]]), torch.tensor([[0], [0]], dtype=torch.int32)
    o = pg.gae_ref(v, rew, term, 0.5, 0.5)
    d1 = 0.25 + 0.5 * 3.0 - 2.0
    d0 = 0.5 + 0.5 * 2.0 - 1.0 + 0.25 * d1
    assert o["adv"].flatten().tolist() == [d0, d1] and o["returns"].flatten().tolist() == [d0 + 1.0, d1 + 2.0]
    o = pg.gae_ref(v, rew, torch.tensor([[1], [0]], dtype=torch.int32), 0.5, 0.5)
    assert o["adv"].flatten().tolist() == [0.5 - 1.0, d1]


# ---------------------------------------------------------------------------------------------------------------------------
# the loss builder's guarantees
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [15, 2053])
def test_loss_builder_guarantees(n):
    m = pg.build_loss_inputs(n) if n != pg.LOSS_ROWS_MASTER else pg.loss_master()
    from oracle import ppo as oppo
    mu64, s64 = oppo.action_dist(m["mu"].double(), m["logvar"].double(), pg.MIN_LV, pg.MAX_LV)
    lp = oppo.log_prob(mu64, s64, m["act"].double())
    assert 1e2 <= float(lp.abs().min()) and float(lp.abs().max()) <= 1e3
    ratio = (lp - m["logp_old"].double()).exp()          # of the fp32 logp_old that the kernel reads
    assert float((ratio / m["target"] - 1).abs().max()) < 1e-4
    for edge in (1 - pg.EPS_CLIP, 1 + pg.EPS_CLIP):
        assert float((ratio / edge - 1).abs().min()) > 0.01
    # every (target ratio, sign of A) combination, under both ways of handing the advantage over, in fp32 and in float64
    for dtype in (F32, F64):
        for adv, stats in ((m["adv"], None), (m["adv_raw"], pg.LOSS_STATS)):
            A = pg.normalised_adv(adv.to(dtype), stats)
            assert torch.equal(torch.sign(A).float(), m["sign"])
            seen = {(float(t), float(s)) for t, s in zip(m["target"], torch.sign(A))}
            assert seen == {(t, s) for t in pg.TARGET_RATIOS for s in (1.0, -1.0, 0.0)}
    # both clamp edges and both outsides in every row, in both halves of the 128 dimensions over the rows
    lv = m["logvar"]
    assert bool(((lv == pg.MIN_LV).sum(1) >= 1).all()) and bool(((lv == pg.MAX_LV).sum(1) >= 1).all())
    assert bool(((lv < pg.MIN_LV).sum(1) >= 1).all()) and bool(((lv > pg.MAX_LV).sum(1) >= 1).all())
    cols = {c for r in range(n) for c in pg.lv_edge_columns(r)}
    assert min(cols) < 64 and (max(cols) >= 64 or n < 32)
    for r in range(min(n, 40)):
        assert lv[r, pg.lv_edge_columns(r)].tolist() == list(pg.LV_EDGE_VALUES)


# ---------------------------------------------------------------------------------------------------------------------------
# the fp32 yardstick's own error, for every group that test_ppo_glue_gpu.py holds to it: non-zero, or floored on purpose
# ---------------------------------------------------------------------------------------------------------------------------
def _nonzero(grp, exact=()):
    for g in grp.groups:
        if g in exact:
            assert grp.err32[g] == 0.0 and grp.bound(g) == pg.ULP * grp.scale[g], (grp.name, g)
        else:
            assert grp.err32[g] > 0 and grp.scale[g] > 0, (grp.name, g)
            assert grp.err32[g] < 1e-4 * grp.scale[g], (grp.name, g, grp.err32[g], grp.scale[g])   # fp32, not something coarser


def test_yardstick_of_the_loss():
    for n, with_stats, scale in ((1, True, 1.0), (2053, False, 0.37), (9, True, 1.0 / 9)):
        part, grp, t64, t32, tb = pg.loss_case(n, with_stats, scale)
        # g_value = -2 scale vf_coef (ret - v): fp32 is not exact on it either
        _nonzero(grp)
        assert part[0].shape == (n, 128) and t64.shape == (6,)
        for j, k in enumerate(pg.TERMS):
            # the derived bound of a sum covers what the fp32 reference itself loses on it, and is no blank cheque
            assert abs(float(t32[j] - t64[j])) <= tb[k], (n, k, float(t32[j] - t64[j]), tb[k])
            assert tb[k] <= 2e-3 * max(abs(float(t64[j])), scale * n), (n, k, tb[k], float(t64[j]))
    # rows are independent: the first rows of the master evaluated alone give the same gradients
    part, grp, *_ = pg.loss_case(5, True, 0.37)
    o = pg.ppo_loss_ref(*pg.cast(part, F64), pg.LOSS_STATS, 0.37)
    for k in ("g_mu", "g_logvar", "g_value"):       # up to the rounding of (1 / n) * (n * scale) in float64
        assert torch.allclose(o[k], grp.o64[k][:5], rtol=1e-14, atol=0.0)


def test_yardstick_of_the_elementwise_groups():
    for grp in pg.gru_groups():
        _nonzero(grp)
    z, res, dy = pg.act_master()
    for act in range(4):
        f = pg.Group(f"act_fwd {act}", lambda z_, r_: pg.act_fwd(z_, r_, act), (z, res))
        _nonzero(f, exact={0: ("a",), 1: (), 2: ("a",), 3: ()}[act])
        a32 = pg.act_fwd(z, None, act)["a"]
        b = pg.Group(f"act_bwd {act}", lambda d_, a_: {"g": pg.act_bwd(d_, a_, act)["g"]}, (dy, a32))
        _nonzero(b, exact=("g",) if act in (0, 2) else ())
    s = pg.Group("sample", pg.sample_action_ref, pg.sample_master())
    _nonzero(s, exact=("logvar",))
    p = pg.Group("posenc", pg.posenc_ref, pg.posenc_master())
    _nonzero(p)


@pytest.mark.parametrize("n,n_clip", pg.ADAMW_CASES)
def test_yardstick_of_the_optimiser(n, n_clip):
    _, _, o64, o32, _ = pg.adamw_case(n, n_clip)
    for k in ("p", "m", "v"):
        e = float((o32[k] - o64[k]).abs().max())
        assert e > 0 or n <= 3, (k, e)      # one to three elements: fp32 may be exact by chance, the bound is then one ulp
        assert e <= 1e-5 * float(o64[k].abs().max())
