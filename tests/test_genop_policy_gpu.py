"""The policy as the proposal distribution of the primitive search on the device: the two launches of csrc/genop_policy.hip against
the float64 / float32 restatement of tests/genop_policy_ref.py and against the environment's own step kernel, and
`generate_sequence_to_goal(policy=)` against its records.

Yardsticks.  state, dist, time and the sampled rows of the proposal: the project's `held()` rule, error against float64 at most 3 x
the float32 restatement's.  Rays: the floor the env tests use for egosensing (3.6e-4, tests/test_env_gpu.py), a ray whose float64 value
moves by more than that under a 1e-5 m shift of the eye left out, at most UNDECIDABLE_CAP of all rays.  Everything that is a copy or the
same device function on the same inputs: torch.equal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import genop_policy_ref as ref
from tests.genop_gpu_helpers import (CFG_RF, MAX_DEPTH, RAY_LEN, ROOT, UNDECIDABLE_CAP, W_TEST, _check_rays, _observe, _poly_dev, _vp, held,
                                     patched_loop, search_world, small_world)  # noqa: F401
from tests.helpers import seeded_prior_state_dict, seeded_vposer_state_dict

pytestmark = pytest.mark.gpu


# ---- observe against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,mode", ref.OBSERVE_CASES, ids=[f"{k}-N{n}-{m[1]}of{m[0]}" for k, n, m in ref.OBSERVE_CASES])
def test_observe_against_float64(kind, N, mode):
    fpr, first = mode
    poly = ref.polygon(kind)
    d = ref.observe_inputs(N, fpr, first, None if poly is None else poly[3])
    g = {k: v.cuda().contiguous() for k, v in d.items() if torch.is_tensor(v)}
    step = 15 if N == 5 else 4                   # above max_depth once: clamped
    got = _observe(g, fpr, first, N, g["choice"], 201, _poly_dev(poly), step, ref.B)
    t64 = ref.observe_case(d, poly, RAY_LEN, step, MAX_DEPTH, torch.float64)
    t32 = ref.observe_case(d, poly, RAY_LEN, step, MAX_DEPTH, torch.float32)
    group = f"{kind} N={N} frame {first} of {fpr}"
    assert torch.equal(got[0][..., :201].cpu(), torch.stack([d["x0"][::N], d["x1"][::N]], 1))          # the seed frames as they are
    for name, q in (("state", 0), ("dist", 2), ("time", 3)):
        held("observe " + name, group, got[q], t64[q], t32[q])
    if poly is None:
        assert torch.equal(got[1].cpu(), torch.ones(ref.B, 2, 32))
    else:
        _check_rays("observe egosensing", group, got[1], t64[1], ref.undecidable(d, poly, RAY_LEN))
        outside = 2 if kind == "square" else None
        if outside is not None:
            assert torch.equal(got[1][outside].cpu(), -torch.ones(2, 32))                             # a start outside its polygon
    if step > MAX_DEPTH:
        assert torch.equal(got[3].cpu(), torch.zeros(ref.B))
    if N > 1:        # NULL choice is candidate 0
        d0 = dict(d, choice=torch.zeros(ref.B, dtype=torch.int32))
        got0 = _observe(g, fpr, first, N, None, 201, _poly_dev(poly), step, ref.B)
        zero = _observe(g, fpr, first, N, torch.zeros(ref.B, dtype=torch.int32, device="cuda"), 201, _poly_dev(poly), step, ref.B)
        assert all(torch.equal(a, b_) for a, b_ in zip(got0, zero))
        held("observe dist, no choice", group, got0[2], ref.observe_case(d0, poly, RAY_LEN, step, MAX_DEPTH, torch.float64)[2],
             ref.observe_case(d0, poly, RAY_LEN, step, MAX_DEPTH, torch.float32)[2])


def test_observe_rows_do_not_depend_on_the_batch():
    """row i of every output from sequence i's inputs only: sequence 1 alone gives the bits it has in the batch of three"""
    poly = ref.polygon("two")
    N = 5
    d = ref.observe_inputs(N, 20, 18, poly[3])
    g = {k: v.cuda().contiguous() for k, v in d.items() if torch.is_tensor(v)}
    pd = _poly_dev(poly)
    full = _observe(g, 20, 18, N, g["choice"], 201, pd, 2, ref.B)
    one = lambda t, per: t[per:2 * per].contiguous()
    g1 = {"joints": one(g["joints"], N * 20), "R_prev": one(g["R_prev"], 1), "T_prev": one(g["T_prev"], 1), "R0": one(g["R0"], N),
          "T0": one(g["T0"], N), "x0": one(g["x0"], N), "x1": one(g["x1"], N), "goal": one(g["goal"], 1)}
    alone = _observe(g1, 20, 18, N, one(g["choice"], 1), 201, (pd[0], pd[1], one(pd[2], 1), pd[3]), 2, 1)
    for a, f in zip(alone, full):
        assert torch.equal(a[0], f[1])


def test_observe_argument_checks():
    from egogen_amd import _lib
    z = torch.zeros(4096, device="cuda")
    zi = torch.zeros(16, dtype=torch.int32, device="cuda")
    lib, st = _lib.load(), _lib.current_stream_ptr()

    def call(fpr=20, first=18, N=1, x_ld=201, edges=z, off=zi, idx=zi, S=1, ray=7.0, step=0, md=13, state=z):
        return lib.egx_primitive_observe(_vp(z), fpr, first, None, N, _vp(z), _vp(z), _vp(z), _vp(z), _vp(z), _vp(z), x_ld, _vp(z), _vp(edges),
                                         _vp(off), _vp(idx), S, ray, step, md, 1, _vp(state), _vp(z), _vp(z), _vp(z), st)
    for kw in ({"first": 19}, {"fpr": 1, "first": 0}, {"N": 0}, {"N": 257}, {"x_ld": 200}, {"off": None}, {"edges": None}, {"ray": 0.0}, {"step": -1},
               {"md": 0}, {"state": None}, {"S": 0}):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert not z.any()


# ---- observe against the environment -------------------------------------------------------------------------------------------
def test_observe_equals_the_env_step(small_world):
    """A VecCrowdEnv (A = 3, single-box SDF scene) after reset and one step: the launch on the env's own step buffers returns the env's
    observation bit for bit - the same device functions on the same inputs."""
    from egogen_amd import synth
    from egogen_amd.crowd_env import VecCrowdEnv
    from egogen_amd.models import GAMMAPrimitiveCombo, PREDICTOR_CFG, REGRESSOR_CFG, VPoserEncoder
    A = 3
    combo = GAMMAPrimitiveCombo(PREDICTOR_CFG, REGRESSOR_CFG)
    combo.load_state_dict(seeded_prior_state_dict())
    vp = VPoserEncoder()
    vp.load_state_dict(seeded_vposer_state_dict())
    scene = synth.make_sdf_scene(32)
    pairs = np.zeros((64, 2, 3), np.float32)
    pairs[:, :, :2] = np.random.default_rng(5).uniform(-3.0, 3.0, (64, 2, 2))
    # the seeded prior throws a body metres away in one step: a walkable polygon of 60 m with a 1.5 m pillar every 5 m (169 holes, 680
    # edges: the staged path) keeps every eye inside it and some wall within the rays' 7 m
    rings = [synth.rect_ring(np.array([-32.0, -32.0]), np.array([32.0, 32.0]), True)]
    rings += [synth.rect_ring(np.array([x, y]), np.array([x + 1.5, y + 1.5]), False) for x in np.arange(-30.0, 31.0, 5.0) for y in np.arange(-30.0, 31.0, 5.0)]
    env = VecCrowdEnv(A, small_world["handle"], combo.cuda().eval(), vp.cuda().eval(), scene_kind="sdf", sdf_dict=scene, rings=rings, pairs=pairs,
                      keep_rollout=True, seed=3)
    env.reset()
    env.step(torch.randn(A, 128, generator=torch.Generator().manual_seed(4)).cuda() * 0.5, auto_reset=False)
    torch.cuda.synchronize()
    assert env.steps.tolist() == [1] * A
    prev = env.prev_frame
    g = {"joints": env.joints, "R_prev": prev[:, :9].contiguous(), "T_prev": prev[:, 9:].contiguous(), "R0": env.R0, "T0": env.T0,
         "x0": env.state[:, 0], "x1": env.state[:, 1], "goal": env.wpath[:, 1].contiguous()}
    got = _observe(g, 20, 18, 1, None, 804, (env.edges, env.edge_off, env.scene_idx, 1), 1, A, ray_len=env.cfg["ray_len"],
                   max_depth=env.cfg["max_depth"])
    differ = [name for name, mine, theirs in zip(("state", "egosensing", "dist", "time"), got, (env.state, env.obs_ego, env.obs_dist, env.obs_time))
              if not torch.equal(mine, theirs)]
    assert not differ, (differ, (got[1] - env.obs_ego).abs().max().item(), (got[2] - env.obs_dist).abs().max().item())
    assert env.edges.shape == (680, 4) and float(env.obs_ego.max()) > -1.0 and float(env.obs_ego.min()) < 1.0      # inside, walls in sight


# ---- propose -------------------------------------------------------------------------------------------------------------------
def _propose(mu, logvar, eps, N, n_mean, n_policy, temperature, alias):
    from egogen_amd import _lib
    e = eps.clone()
    z = e if alias else torch.full_like(e, float("nan"))
    _lib.check(_lib.load().egx_policy_propose(_vp(mu), _vp(logvar), _vp(e), -2.5, 2.5, mu.shape[0], N, n_mean, n_policy, float(temperature),
                                              _vp(z), _lib.current_stream_ptr()), "egx_policy_propose")
    torch.cuda.synchronize()
    if not alias:
        assert torch.equal(e, eps)
    return z


@pytest.mark.parametrize("N", [1, 5, 256])
def test_propose(N):
    b = ref.B
    mu, logvar, eps = ref.propose_inputs(N)
    assert bool((logvar[0] < -2.5).all()) and bool((logvar[1] > 2.5).all())
    mu_d, lv_d, eps_d = mu.cuda(), logvar.cuda(), eps.cuda()
    pool = {"got": [], "t64": [], "t32": []}
    for n_mean in sorted({0, 1, N}):
        for n_policy in sorted({n_mean, N}):
            for temperature in (0.0, 1.0, 0.5):
                for alias in (False, True):
                    z = _propose(mu_d, lv_d, eps_d, N, n_mean, n_policy, temperature, alias).reshape(b, N, 128)
                    assert torch.equal(z[:, :n_mean], mu_d[:, None].expand(b, n_mean, 128)), (n_mean, n_policy, temperature, alias)
                    assert torch.equal(z[:, n_policy:], eps_d.reshape(b, N, 128)[:, n_policy:]), (n_mean, n_policy, temperature, alias)
                    if temperature == 0.0:
                        assert torch.equal(z[:, :n_policy], mu_d[:, None].expand(b, n_policy, 128))
                    elif n_policy > n_mean:
                        rows = lambda t: t.reshape(b, N, 128)[:, n_mean:n_policy]
                        pool["got"].append(z[:, n_mean:n_policy].cpu().reshape(-1))
                        pool["t64"].append(rows(ref.propose(mu, logvar, eps, -2.5, 2.5, N, n_mean, n_policy, temperature, torch.float64)).reshape(-1))
                        pool["t32"].append(rows(ref.propose(mu, logvar, eps, -2.5, 2.5, N, n_mean, n_policy, temperature, torch.float32)).reshape(-1))
    assert torch.equal(lv_d.cpu(), logvar)                  # logvar is only read: the clamp is not written back
    held("propose", f"N={N}", torch.cat(pool["got"]), torch.cat(pool["t64"]), torch.cat(pool["t32"]))


def test_propose_temperature_one_is_sample_action():
    """the arithmetic of egx_sample_action through the same device functions: at temperature 1 the same bits"""
    from egogen_amd import _lib
    mu, logvar, eps = (t.cuda() for t in ref.propose_inputs(1))
    z = _propose(mu, logvar, eps, 1, 0, 1, 1.0, False)
    act, lv = torch.empty_like(mu), logvar.clone()
    _lib.check(_lib.load().egx_sample_action(_vp(mu), _vp(lv), _vp(eps), -2.5, 2.5, 0, ref.B, _vp(act), None, _lib.current_stream_ptr()),
               "egx_sample_action")
    torch.cuda.synchronize()
    assert torch.equal(z, act)


def test_propose_argument_checks():
    from egogen_amd import _lib
    z = torch.zeros(2 * 128 + 4, device="cuda")
    lib, st = _lib.load(), _lib.current_stream_ptr()

    def call(N=2, n_mean=1, n_policy=2, t=1.0, mu=z, out=z, lo=-2.5, hi=2.5):
        return lib.egx_policy_propose(_vp(mu), _vp(z), _vp(z), lo, hi, 1, N, n_mean, n_policy, t, _vp(out), st)
    for kw in ({"N": 0}, {"N": 257}, {"n_mean": -1}, {"n_mean": 2, "n_policy": 1}, {"n_policy": 3}, {"t": -0.5}, {"t": float("nan")}, {"mu": None},
               {"out": None}, {"mu": z[1:]}, {"lo": 1.0, "hi": 0.0}):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert not z.any()


# ---- in the search -------------------------------------------------------------------------------------------------------------
class _Args:
    seed = 0; lr = 3e-4; gamma = 0.99; gae_lambda = 0.95; max_grad_norm = 0.1; vf_coef = 1.0; ent_coef = 0.01
    weight_kld = 0; rew_norm = False; eps_clip = 0.1; value_clip = 0; dual_clip = None; norm_adv = 1; recompute_adv = 0
    deterministic_eval = False


K, N = 3, 5


@pytest.fixture(scope="module")
def policy_world(search_world):
    """search_world with a seeded policy (non-trivial biases, some logvars outside the clamp), the room0 polygon, starts inside it and
    the single-box SDF scene."""
    from egogen_amd import setup_world as sw, synth
    from egogen_amd.body_model import SdfScene
    pol = sw.build_policy(_Args())
    with torch.no_grad():
        for p_ in pol.parameters():
            if p_.dim() == 1:
                p_.add_(0.05 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(p_.numel())).cuda())
        pol.actor.pnet.out_fc.weight.mul_(30.0)             # main_ppo's 0.01 head would give mu ~ 0: make the proposal matter
        pol.actor.pnet.out_fc.bias[128:160] += 4.0
        pol.actor.pnet.out_fc.bias[160:192] -= 4.0
    poly = ref.polygon("two")
    T0 = torch.zeros(3, 3)
    T0[:, :2] = torch.as_tensor(np.stack([poly[3][0], poly[3][2], poly[3][0] + [0.3, 0.2]]), dtype=torch.float32)
    w = dict(search_world)
    w.update(policy=pol, room0=ref.room0_edges(), T0=T0, scene=SdfScene(synth.make_sdf_scene(32)),
             z=torch.randn(K, 3 * N, 128, generator=torch.Generator().manual_seed(92)))
    return w


def _run(w, Kp, prop, **extra):
    zin = w["z"][:Kp].cuda()             # on the device already: the operator must not write the caller's tensor
    kw = dict(z=zin, reproj_factor=CFG_RF, weights=W_TEST, goal_thresh=0.0, to_numpy=False, T0=w["T0"], scene=w["scene"], policy=prop)
    kw.update(extra)
    with patched_loop(w["op"], "_search_loop", no_host_wait=True) as seen:
        res = w["op"].generate_sequence_to_goal(w["data"], w["bparams"], w["betas"], w["goal"] + w["T0"], Kp, N, **kw)
    assert seen.calls == [(Kp, 3, N)] and torch.equal(zin.cpu(), w["z"][:Kp])
    return res, seen.s


def _identities(w, res, s, prop, Kp):
    """what the records of a policy run must satisfy among themselves, bit for bit"""
    b = 3
    n_mean, n_policy = prop.counts(N)
    assert res.obs_state.shape == (Kp, b, 2, 402) and res.obs_egosensing.shape == (Kp, b, 2, 32) and res.obs_dist.shape == (Kp, b)
    assert res.policy_mu.shape == (Kp, b, 128) and res.policy_logvar.shape == (Kp, b, 128) and res.obs_time.shape == (Kp, b)
    assert (res.policy_n_mean, res.policy_n_policy, res.policy_temperature) == (n_mean, n_policy, prop.temperature)
    assert res.search["policy_ray_len"] == prop.ray_len and res.policy_max_depth == prop.max_depth
    for k in range(Kp):
        obs = {"state": res.obs_state[k].clone(), "egosensing": res.obs_egosensing[k].clone(), "dist": res.obs_dist[k].clone(),
               "time": res.obs_time[k].clone()}
        out = prop.runner.forward(obs, want_actor=True, want_critic=False)
        assert torch.equal(out["mu"], res.policy_mu[k]) and torch.equal(out["logvar"], res.policy_logvar[k]), k
        z = _propose(res.policy_mu[k], res.policy_logvar[k], w["z"][k].cuda(), N, n_mean, n_policy, prop.temperature, False)
        assert torch.equal(z, s["z"][k]), k
        rows = torch.arange(b, device="cuda") * N + res.choice[k].long()
        assert torch.equal(res.z[k], s["z"][k][rows]), k
        assert torch.equal(res.obs_time[k], torch.full((b,), 1.0 - np.float32(min(k, prop.max_depth)) / np.float32(prop.max_depth), device="cuda"))
    assert not torch.equal(s["z"][0].cpu(), w["z"][0])           # the candidates are the proposal's, not the draws


def test_search_with_policy(policy_world):
    from egogen_amd.proposal import PolicyProposal
    w, b = policy_world, 3
    h = w["handle"]
    prop = PolicyProposal(w["policy"], edges=w["room0"], max_depth=2)              # K = 3 primitives: the clamp of time acts at the last
    poly = (w["room0"], np.array([0, 89], np.int32), np.zeros(b, np.int32))
    pd = _poly_dev(poly)
    runs = {Kp: _run(w, Kp, prop) for Kp in range(1, K + 1)}
    res, s = runs[K]
    _identities(w, res, s, prop, K)
    goal = (w["goal"] + w["T0"]).cuda()
    # the first observation: the seed bodies in the seed's frame
    seed = w["bparams"].permute(1, 0, 2).contiguous().cuda()
    j0 = h.forward(seed.reshape(b * 2, 93), w["betas"].cuda(), 2, want_verts=False, want_markers=False)["joints"]
    R0 = torch.eye(3, device="cuda").repeat(b, 1, 1)
    x = w["data"].cuda()
    inputs = {0: (j0.reshape(b, 2, 127, 3), R0, w["T0"].cuda(), R0, w["T0"].cuda(), x[0], x[1])}
    for k in range(1, K):           # a run of k primitives is the prefix of the longer one: its loop state is what observation k was made from
        rk, sk = runs[k]
        for name in ("choice", "cost", "z", "markers", "obs_state", "policy_mu"):
            assert torch.equal(getattr(rk, name), getattr(res, name)[:k]), (name, k)
        J = sk["lbs_out"]["joints"].reshape(b, N, 20, 127, 3)[torch.arange(b), rk.choice[k - 1].long(), 18:20]
        cur = sk["xs"][k % 2]
        inputs[k] = (J, rk.rotmat[k - 1], rk.transl[k - 1], sk["R0"][::N].reshape(b, 3, 3), sk["T0"][::N], cur[0][::N], cur[1][::N])
    left_out = total = 0
    for k in range(K):
        j2, Rp, Tp, Rn, Tn, x0, x1 = (t.cpu() for t in inputs[k])
        g = {name: t.cuda().contiguous() for name, t in zip(("joints", "R_prev", "T_prev", "R0", "T0", "x0", "x1"), (j2, Rp, Tp, Rn, Tn, x0, x1))}
        direct = _observe(dict(g, goal=goal), 2, 0, 1, None, 201, pd, k, b, ray_len=prop.ray_len, max_depth=prop.max_depth)
        for mine, name in zip(direct, ("obs_state", "obs_egosensing", "obs_dist", "obs_time")):
            assert torch.equal(mine, getattr(res, name)[k]), (name, k)
        t64 = ref.observe(j2, Rp, Tp, Rn, Tn, x0, x1, goal.cpu(), poly, prop.ray_len, k, prop.max_depth, torch.float64)
        t32 = ref.observe(j2, Rp, Tp, Rn, Tn, x0, x1, goal.cpu(), poly, prop.ray_len, k, prop.max_depth, torch.float32)
        held("search obs_state", f"k={k}", res.obs_state[k], t64[0], t32[0])
        held("search obs_dist", f"k={k}", res.obs_dist[k], t64[2], t32[2])
        held("search obs_time", f"k={k}", res.obs_time[k], t64[3], t32[3])
        und = torch.zeros(b, 2, 32, dtype=torch.bool)
        for sx, sy in ((ref.SHIFT, 0.0), (-ref.SHIFT, 0.0), (0.0, ref.SHIFT), (0.0, -ref.SHIFT)):
            moved = ref.observe(j2, Rp, Tp, Rn, Tn, x0, x1, goal.cpu(), poly, prop.ray_len, k, prop.max_depth, torch.float64, (sx, sy))[1]
            und |= (moved.double() - t64[1].double()).abs() > ref.EGO_FLOOR
        keep = ~und
        left_out, total = left_out + int(und.sum()), total + und.numel()
        assert float((res.obs_egosensing[k].cpu().double() - t64[1].double()).abs()[keep].max()) <= ref.EGO_FLOOR, k
    assert left_out / total <= UNDECIDABLE_CAP, (left_out, total)
    assert float(res.obs_time[K - 1].max()) == 0.0 and float(res.obs_egosensing.min()) < 1.0
    res_np = w["op"].generate_sequence_to_goal(w["data"], w["bparams"], w["betas"], w["goal"] + w["T0"], K, N, z=w["z"], reproj_factor=CFG_RF,
                                               weights=W_TEST, goal_thresh=0.0, T0=w["T0"], scene=w["scene"], policy=prop)
    assert isinstance(res_np.policy_mu, np.ndarray) and np.array_equal(res_np.obs_egosensing, res.obs_egosensing.cpu().numpy())
    assert np.array_equal(res_np.z, res.z.cpu().numpy())


def test_search_zero_head_puts_its_bias_into_every_mean_row(policy_world):
    from egogen_amd.proposal import PolicyProposal
    w, b = policy_world, 3
    head = w["policy"].actor.pnet.out_fc
    keep = (head.weight.detach().clone(), head.bias.detach().clone())
    zstar = torch.randn(128, generator=torch.Generator().manual_seed(5)).cuda()
    try:
        with torch.no_grad():
            head.weight.zero_()
            head.bias.copy_(torch.cat([zstar, torch.full((128,), -2.5, device="cuda")]))
        prop = PolicyProposal(w["policy"], edges=w["room0"], n_mean=2)
        res, s = _run(w, K, prop)
        zs = s["z"].reshape(K, b, N, 128)
        assert torch.equal(zs[:, :, :2], zstar.expand(K, b, 2, 128)) and torch.equal(res.policy_mu, zstar.expand(K, b, 128))
        assert torch.equal(res.policy_logvar, torch.full((K, b, 128), -2.5, device="cuda"))
        assert torch.equal(zs[:, :, 4:], w["z"].cuda().reshape(K, b, N, 128)[:, :, 4:])              # n_policy = 5 - 1: the prior's row
        # every candidate the mean: equal costs, the lowest index wins
        res_all, s_all = _run(w, K, PolicyProposal(w["policy"], edges=w["room0"], n_mean=N, prior_fraction=0.0))
        assert torch.equal(s_all["z"], zstar.expand(K, b * N, 128))
        assert torch.equal(res_all.cost, res_all.cost[:, :, :1].expand(K, b, N)) and not res_all.choice.any()
    finally:
        with torch.no_grad():
            head.weight.copy_(keep[0])
            head.bias.copy_(keep[1])


def test_search_with_policy_and_groups_and_obstacles(policy_world):
    from egogen_amd import MovingObstacles
    from egogen_amd.proposal import PolicyProposal
    w = policy_world
    prop = PolicyProposal(w["policy"], edges=w["room0"], temperature=0.5, prior_fraction=0.4)
    res, s = _run(w, 2, prop, groups=[0, 1, 0])
    _identities(w, res, s, prop, 2)
    assert res.choice_trace.shape == (2, 2, 3) and torch.equal(res.choice, res.choice_trace[:, -1])
    free, _ = _run(w, 1, prop)       # somebody stands 0.7 m beside where sequence 0 would be at frame 10: 0.1 m clear of it, inside the margin
    at = (free.rotmat[0, 0] @ free.pelvis[0, 0, 10] + free.transl[0, 0])[:2].cpu().numpy() + [0.7, 0.0]
    res, s = _run(w, 2, prop, obstacles=MovingObstacles.from_tracks(np.tile(at[None, None], (1, 40, 1))))
    _identities(w, res, s, prop, 2)
    assert res.obstacle_term.shape == (2, 3, N) and float(res.obstacle_term[0, 0, int(free.choice[0, 0])]) > 0.0
    with pytest.raises(ValueError, match="policy= is the greedy search only"):
        _run(w, 2, prop, beam_width=2)


# ---- the untouched path --------------------------------------------------------------------------------------------------------
_UNTOUCHED = r"""
import sys, torch
sys.path.insert(0, {root!r})
from tests.genop_gpu_helpers import CFG_RF, W_TEST, V_SMALL, _combo, _op, _walkers
from tests.helpers import seeded_prior_state_dict
from egogen_amd import synth
from egogen_amd.body_model import BodyModelHandle
h = BodyModelHandle(synth.make_body_model(0, num_verts=V_SMALL), synth.marker_ids(V_SMALL), synth.feet_vids(V_SMALL))
op = _op(_combo(seeded_prior_state_dict()), h)
b, K, N = 3, 2, 4
pp, betas, g = _walkers(b, 78)
pp[:, :, 3:6] = torch.randn(b, 1, 3, generator=g) * 0.05
data = h.forward(pp.cuda().reshape(b * 20, 93), betas.cuda(), 20, want_verts=False)["markers"].reshape(b, 20, 201)[:, :2].permute(1, 0, 2).contiguous().cpu()
goal = torch.tensor([[0.5, 2.0, 0.9], [-1.0, 1.0, 0.9], [0.0, 3.0, 0.9]])
z = torch.randn(K, b * N, 128, generator=torch.Generator().manual_seed(3))
run = lambda **kw: op.generate_sequence_to_goal(data, pp[:, :2].permute(1, 0, 2).contiguous(), betas, goal, K, N, z=z, reproj_factor=CFG_RF,
                                                weights=W_TEST, goal_thresh=0.0, to_numpy=False, **kw)
assert "egogen_amd.proposal" not in sys.modules
before = run()
assert "egogen_amd.proposal" not in sys.modules
from egogen_amd.proposal import PolicyProposal
after = run(policy=None)
for k in ("markers", "params", "rotmat", "transl", "pelvis", "z", "R0", "T0", "choice", "status", "goal_dist", "cost", "cost_terms", "colliding", "n_valid"):
    assert torch.equal(getattr(before, k), getattr(after, k)), k
assert all(getattr(after, k) is None for k in after.POLICY_FIELDS) and "policy_mu" not in after.search
print("UNTOUCHED OK")
"""


def test_policy_none_is_the_search_as_it_was():
    """policy=None gives the outputs of a call made before egogen_amd.proposal was ever imported: one fresh process runs both"""
    r = subprocess.run([sys.executable, "-c", _UNTOUCHED.format(root=ROOT)], capture_output=True, text=True, cwd=ROOT, timeout=300,
                       env=dict(os.environ))
    assert r.returncode == 0 and "UNTOUCHED OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
