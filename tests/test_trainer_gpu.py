"""GPU tests of the PPO rollout glue (action sampling, GAE), the collector/trainer loop and the drop-in entry point."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import build_world, max_abs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Args:
    seed = 0; lr = 3e-4; gamma = 0.99; gae_lambda = 0.95; max_grad_norm = 0.1; vf_coef = 1.0; ent_coef = 0.01
    weight_kld = 0; rew_norm = False; eps_clip = 0.1; value_clip = 0; dual_clip = None; norm_adv = 1; recompute_adv = 0
    deterministic_eval = False


def test_gae_kernel_matches_oracle():
    import ctypes as C
    from egogen_amd import _lib
    from oracle import ppo as oppo
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    n, A = 7, 37
    v = torch.randn(n + 1, A, generator=g)
    rew = torch.randn(n, A, generator=g)
    term = (torch.rand(n, A, generator=g) < 0.2).to(torch.int32)
    ret, adv = torch.empty(n, A, device="cuda"), torch.empty(n, A, device="cuda")
    vc, rc_, tc = v.cuda(), rew.cuda(), term.cuda()
    _lib.check(lib.egx_gae(_lib.ptr(vc), _lib.ptr(rc_), _lib.ptr(tc), n, A, 0.99, 0.95, _lib.ptr(ret), _lib.ptr(adv),
                           _lib.current_stream_ptr()), "gae")
    oret, oadv = oppo.gae_returns(v[:n].T.numpy(), v[1:].T.numpy(), rew.T.numpy(), term.T.numpy().astype(bool),
                                  np.zeros((A, n), bool), 0.99, 0.95)
    assert max_abs(adv.cpu().T, oadv) < 1e-5 and max_abs(ret.cpu().T, oret) < 1e-5


def test_sample_action_kernel():
    import ctypes as C
    from egogen_amd import _lib
    from oracle import ppo as oppo
    lib = _lib.load()
    g = torch.Generator().manual_seed(1)
    n = 19
    mu, lv, eps = torch.randn(n, 128, generator=g), torch.randn(n, 128, generator=g) * 3, torch.randn(n, 128, generator=g)
    muc, lvc, epsc = mu.cuda(), lv.clone().cuda(), eps.cuda()
    act, logp = torch.empty(n, 128, device="cuda"), torch.empty(n, device="cuda")
    _lib.check(lib.egx_sample_action(_lib.ptr(muc), _lib.ptr(lvc), _lib.ptr(epsc), -2.5, 2.5, 0, n, _lib.ptr(act), _lib.ptr(logp),
                                     _lib.current_stream_ptr()), "sample")
    m, s = oppo.action_dist(mu, lv)
    ref_act = m + s * eps
    assert max_abs(lvc.cpu(), lv.clamp(-2.5, 2.5)) == 0
    assert max_abs(act.cpu(), ref_act) < 1e-5
    assert max_abs(logp.cpu(), oppo.log_prob(m, s, ref_act)) < 1e-3
    # deterministic eval: act = mu
    _lib.check(lib.egx_sample_action(_lib.ptr(muc), _lib.ptr(lvc), None, -2.5, 2.5, 1, n, _lib.ptr(act), _lib.ptr(logp),
                                     _lib.current_stream_ptr()), "sample")
    assert torch.equal(act, muc)


def _rollout_logp_vs_float64(policy, bb):
    """Rollout log-probabilities (policy forward + egx_sample_action on the packed images) against the oracle's restatement of
    the networks evaluated in FLOAT64 on the same observations and actions: (max |d logp|, max |logp|)."""
    from oracle import nets as onets, ppo as oppo
    P = {k: v.detach().cpu().double() for k, v in policy.state_dict().items() if not k.startswith("_actor_critic.")}
    obs = {k: v.detach().cpu().double() for k, v in bb.obs_flat().items()}
    mu, logvar = onets.policy_actor(P, onets.policy_base(P, obs))
    m_, s_ = oppo.action_dist(mu, logvar)
    lp = oppo.log_prob(m_, s_, bb.act.reshape(-1, 128).detach().cpu().double())
    return max_abs(lp, bb.logp_old.reshape(-1).cpu()), float(lp.abs().max())


@pytest.mark.parametrize("kind", ["sdf", "box"])
def test_collect_and_update_loop(kind):
    """Collector + trainer on the DEFAULT update path: minibatches of 32 rows = the hand-written chain replayed as HIP graphs
    (round 4 ran this loop at batch size 8, i.e. on the autograd-node fallback)."""
    from egogen_amd import setup_world as sw
    from egogen_amd.trainer import Collector, onpolicy_trainer
    w = build_world(V=1024, A=32, scene_kind=kind, sdf_res=32, n_pairs=64, n_scenes=4)
    env = w["env"]
    a = _Args()
    a.update_graph = True
    policy = sw.build_policy(a)
    before = policy.actor.pnet.out_fc.weight.clone()
    col = Collector(policy, env)
    res = onpolicy_trainer(policy, col, None, max_epoch=1, step_per_epoch=128, repeat_per_collect=1, episode_per_test=0,
                           batch_size=32, step_per_collect=64, verbose=False)
    assert res["train_step"] == 128 and res["gradient_step"] == 4
    assert policy.update_paths == {"chain+graph": 4}, policy.update_paths
    assert not torch.equal(before, policy.actor.pnet.out_fc.weight)
    for p in policy.parameters():
        assert torch.isfinite(p).all()
    b = col._batches[2]
    assert torch.isfinite(b.rew).all() and torch.isfinite(b.adv).all() and torch.isfinite(b.returns).all()
    # the rollout log-probs (packed images, default two-term arithmetic) against the torch modules in float64, before any
    # parameter change: 1e-4 RELATIVE is north_star's bar; the values are ~ -2e2, measured ~1e-4 absolute
    policy2 = sw.build_policy(_Args())
    col2 = Collector(policy2, env)
    bb = col2.collect(2)
    d, mag = _rollout_logp_vs_float64(policy2, bb)
    assert d <= 1e-4 * mag and d <= 2e-3, (d, mag)
    # and the update chain sees the same function: on its first minibatch (no step taken yet) mean(logp_old - logp) ~ 0
    policy2.process_fn(bb)
    policy2._ensure_flat_grads()
    assert policy2._flat_optimizer_ready()
    hs = policy2._train_handle(32)
    assert hs is not None
    log = torch.zeros(6, device="cuda")
    policy2._fwd_bwd(bb, torch.arange(32, device="cuda"), None, log)
    assert abs(float(log[5])) <= 2e-4, float(log[5])


def test_full_size_loop_on_the_default_update_path():
    """BASELINE configs[2] at its own size: 512 agents on the 64 random-box scenes, V = 10 475, 4 vector steps per collect,
    minibatch 256, two collect + update cycles.  Every minibatch must run the hand-written chain as replayed graphs, no episode
    may start in penetration, parameters stay finite, and the rollout log-probs agree with float64 torch before any step."""
    from egogen_amd import setup_world as sw, synth
    from egogen_amd.body_model import BodyModelHandle
    from egogen_amd.trainer import Collector
    bm, _ = sw.load_body_model("male", seed=0, num_verts=synth.NUM_VERTS)
    body = BodyModelHandle(bm, synth.marker_ids(synth.NUM_VERTS), synth.feet_vids(synth.NUM_VERTS))
    scene = sw.build_scene("box", seed=0)
    assert len(scene["box_scenes"]) == 64
    env = sw.build_env(512, scene, body, sw.build_motion_prior(seed=0), sw.build_vposer(seed=0), seed=0)
    a = _Args()
    a.update_graph = True
    policy = sw.build_policy(a)
    policy.train()
    col = Collector(policy, env)
    col.reset()
    first = None
    for cycle in range(2):
        batch = col.collect(4)
        env.check_finite()
        if first is None:
            first = _rollout_logp_vs_float64(policy, batch)
        policy.process_fn(batch)
        out = policy.learn(batch, 256, 1)
        assert len(out["loss"]) == 8 and np.isfinite(out["loss"]).all()
    assert policy.update_paths == {"chain+graph": 16}, policy.update_paths
    assert env.forced_accepts() == 0
    for p in policy.parameters():
        assert torch.isfinite(p).all()
    d, mag = first
    assert d <= 1e-4 * mag and d <= 2e-3, first


def test_recompute_adv_reads_current_weights_under_graph_replay():
    """--recompute-adv with a loss option (value_clip routes the minibatch through the autograd nodes, replayed as graphs):
    replayed graphs write the parameters by address, so from the third pass on the value pass of ppo_policy.py:185-186 used to
    read packed images that were a whole pass old.  Every recompute must equal a fresh critic evaluation of the CURRENT
    parameters (plain torch modules)."""
    from egogen_amd import setup_world as sw

    class A(_Args):
        value_clip = 1; recompute_adv = 1
        update_graph = True
    pol = sw.build_policy(A())
    b = _filled_batch(4, 32, 11, pol)
    b.term.zero_()
    b.rew.copy_(torch.randn(4, 32, generator=torch.Generator().manual_seed(3)))
    pol.process_fn(b)
    with torch.no_grad():     # ratio exactly 1 at the start: the early stop on approx_kl must not end the passes
        _, mu, sigma = pol._dist_params(b.obs_flat())
        b.logp_old.copy_(pol.log_prob(mu, sigma, b.act.reshape(-1, 128)).reshape(4, 32))
    seen, drift, prev = [], [], []
    inner = pol.process_fn

    def spy(batch):
        r = inner(batch)
        if getattr(pol, "_recomputing", False):
            with torch.no_grad():
                hx = pol.shared_net(batch.obs_flat(batch.n + 1))
                fresh = pol.critic(hx).flatten().reshape(batch.n + 1, batch.A)
            seen.append(max_abs(batch.values.cpu(), fresh.cpu()))
            if prev:
                drift.append(max_abs(fresh.cpu(), prev[-1]))
            prev.append(fresh.cpu().clone())
        return r
    pol.process_fn = spy
    for g in pol.optim.param_groups:   # small steps: the early stop on approx_kl (>= 0.02) must not end the passes
        g["lr"] = 1e-6
    pol.learn(b, 32, 4)
    assert len(seen) >= 2, seen            # pass 3 is the first one that used to read stale images
    assert any(k.endswith("+graph") for k in pol.update_paths), pol.update_paths
    # seen[0] (the first recompute was never stale) is the images-vs-fp32-modules yardstick; a stale image is off by a whole
    # pass of optimiser steps = `drift`
    assert min(drift) > 20 * max(seen[0], 1e-6), (seen, drift)
    assert max(seen) <= 3 * seen[0] + 2e-5, (seen, drift)


def test_main_ppo_entry_point_writes_reference_layout(tmp_path):
    """crowd_ppo/main_ppo.py drop-in: CLI, checkpoint_{epoch}.pth / policy.pth with {"model","optim"}, 48 state_dict keys,
    results/ directory tree and log/eval_results/*.pkl in the reference's format (utils.py:14-46)."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "crowd_ppo", "main_ppo.py"), "--training-num", "8", "--test-num", "4", "--epoch", "2",
           "--step-per-epoch", "32", "--step-per-collect", "16", "--batch-size", "8", "--num-verts", "1024", "--sdf-res", "32",
           "--scene", "single_box", "--logdir", str(tmp_path / "log"), "--save-interval", "1", "--save-rollout", "1"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Final reward:" in r.stdout
    run_dirs = []
    for dp, dn, fn in os.walk(tmp_path / "log" / "collision-avoidance" / "ppo" / "0"):
        if "checkpoint_1.pth" in fn:
            run_dirs.append(dp)
    assert len(run_dirs) == 1
    ck = torch.load(os.path.join(run_dirs[0], "checkpoint_2.pth"), map_location="cpu")
    assert set(ck.keys()) == {"model", "optim"} and len(ck["model"]) == 48
    assert os.path.exists(os.path.join(run_dirs[0], "policy.pth"))
    assert os.path.isdir(tmp_path / "results" / "crowd_ppo" / "MPVAEPolicy_samp_collision" / "collision_test" / "checkpoints")
    pk = sorted((tmp_path / "log" / "eval_results").glob("motion_*.pkl"))
    assert pk, "no rollout pickles written"
    d = pickle.load(open(pk[0], "rb"))
    assert set(d.keys()) >= {"motion", "wpath", "navmesh_path"} and d["wpath"].shape == (2, 3)
    mp = d["motion"][0]
    assert mp["blended_marker"].shape == (20, 67, 3) and mp["smplx_params"].shape == (1, 20, 93) and mp["betas"].shape == (10,)
    assert mp["transf_rotmat"].shape == (3, 3) and mp["transf_transl"].shape == (1, 3) and mp["pelvis_loc"].shape == (20, 3)
    assert mp["gender"] == "male" and mp["mp_type"] == "2-frame"
    # resume + watch with deterministic eval
    cmd2 = [sys.executable, os.path.join(ROOT, "crowd_ppo", "main_ppo.py"), "--watch", "--deterministic-eval", "--resume-path",
            os.path.join(run_dirs[0], "checkpoint_2.pth"), "--test-num", "4", "--num-verts", "1024", "--sdf-res", "32",
            "--scene", "single_box", "--logdir", str(tmp_path / "log2")]
    r2 = subprocess.run(cmd2, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-4000:]
    assert "Loaded agent from" in r2.stdout and "Final reward:" in r2.stdout


def test_graph_replayed_update_equals_eager():
    """The HIP-graph replay of (gather, forward, loss, backward, clip, AdamW) performs the same update as eager."""
    import copy
    from egogen_amd import setup_world as sw
    from egogen_amd.ppo_policy import RolloutBatch

    def make(graph):
        a = _Args()
        a.update_graph = graph
        return sw.build_policy(a)

    pe, pg = make(False), make(True)
    pg.load_state_dict(pe.state_dict())
    g = torch.Generator().manual_seed(0)
    b = RolloutBatch(2, 32, "cuda")
    b.state.copy_(torch.randn(b.state.shape, generator=g) * 0.3)
    b.ego.copy_(torch.rand(b.ego.shape, generator=g) * 2 - 1)
    b.dist.copy_(torch.rand(b.dist.shape, generator=g)); b.time.copy_(torch.rand(b.time.shape, generator=g))
    b.act.copy_(torch.randn(b.act.shape, generator=g)); b.adv.copy_(torch.randn(b.adv.shape, generator=g))
    b.returns.copy_(torch.randn(b.returns.shape, generator=g))
    with torch.no_grad():
        _, mu, sigma = pe._dist_params(b.obs_flat())
        b.logp_old.copy_(pe.log_prob(mu, sigma, b.act.reshape(-1, 128)).reshape(2, 32) + 0.05 * torch.randn(2, 32, generator=g).cuda())
    for pol in (pe, pg):
        pol._perm_gen.manual_seed(123)
    le = pe.learn(b, 16, 1)
    lg = pg.learn(b, 16, 1)
    assert not any(v.get("failed") for v in pg._graph_cache.values()), "graph capture fell back to eager"
    assert len(le["loss"]) == len(lg["loss"]) == 4
    np.testing.assert_allclose(le["loss"], lg["loss"], rtol=2e-4, atol=1e-5)
    ge, gg = pe._flat_grad, pg._flat_grad
    assert float((ge - gg).abs().max()) <= 1e-4 * float(ge.abs().max()) + 1e-9
    # second call replays the cached graph
    le2, lg2 = pe.learn(b, 16, 1), pg.learn(b, 16, 1)
    np.testing.assert_allclose(le2["loss"], lg2["loss"], rtol=5e-3, atol=1e-4)


def test_fused_update_ops_match_torch_autograd():
    """egx_ppo_loss / egx_gru_pointwise(_bwd) / egx_posenc as autograd nodes give the same loss and parameter gradients as the
    plain torch expression of ppo_policy.py:189-241 (which tests/test_ppo_cpu.py pins to the oracle restatement)."""
    from egogen_amd import models, setup_world as sw
    from egogen_amd.ppo_policy import RolloutBatch
    pol = sw.build_policy(_Args())
    g = torch.Generator().manual_seed(0)
    N = 48
    b = RolloutBatch(1, N, "cuda")
    b.state.copy_(torch.randn(b.state.shape, generator=g) * 0.3)
    b.ego.copy_(torch.rand(b.ego.shape, generator=g) * 2 - 1)
    b.dist.copy_(torch.rand(b.dist.shape, generator=g)); b.time.copy_(torch.rand(b.time.shape, generator=g))
    b.act.copy_(torch.randn(b.act.shape, generator=g) * 2.5)   # some ratios leave the clip range
    b.adv.copy_(torch.randn(b.adv.shape, generator=g)); b.returns.copy_(torch.randn(b.returns.shape, generator=g))
    # push some raw logvars outside [-2.5, 2.5] so the clamp mask is exercised
    with torch.no_grad():
        pol.actor.pnet.out_fc.bias[128:160] += 4.0
        pol.actor.pnet.out_fc.bias[160:192] -= 4.0
        _, mu, sigma = pol._dist_params(b.obs_flat())
        b.logp_old.copy_((pol.log_prob(mu, sigma, b.act.reshape(-1, 128)) + 0.2 * torch.randn(N, generator=g).cuda()).reshape(1, N))
    args = (b.obs_flat(), b.act.reshape(N, 128), b.adv.reshape(N), b.returns.reshape(N), b.logp_old.reshape(N))

    def grads(fused, fused_linear=False):
        models.FUSED_UPDATE_OPS = fused
        pol.use_fused_loss = fused
        pol.use_fused_linear = fused_linear
        pol.zero_grad(set_to_none=True)
        if fused_linear:  # LinearFn accumulates into the flat gradient views
            pol._ensure_flat_grads()
            pol._flat_grad.zero_()
        loss, terms = pol.minibatch_loss(*args)
        loss.backward()
        return float(loss), {k: float(v) for k, v in terms.items() if not k.startswith("_")}, torch.cat([p.grad.flatten() for p in pol.parameters()]).clone()

    try:
        l0, t0, g0 = grads(False)
        l1, t1, g1 = grads(True)
        l2, t2, g2 = grads(True, fused_linear=True)
    finally:
        models.FUSED_UPDATE_OPS = True
        pol.use_fused_linear = True
    assert abs(l0 - l2) <= 1e-4 * max(1.0, abs(l0))
    for k in ("loss/clip", "loss/vf", "loss/ent", "loss/kld", "approx_kl"):
        assert abs(t0[k] - t2[k]) <= 2e-4 * max(1.0, abs(t0[k])), k
    assert float((g0 - g2).abs().max()) <= 1e-3 * float(g0.abs().max())
    # log-probs are 128-term sums of magnitude ~1e2 feeding exp(): 1e-4 absolute on the loss is fp32 summation-order noise
    assert abs(l0 - l1) <= 1e-4 * max(1.0, abs(l0))
    for k in ("loss/clip", "loss/vf", "loss/ent", "loss/kld", "approx_kl"):
        assert abs(t0[k] - t1[k]) <= 2e-4 * max(1.0, abs(t0[k])), k
    assert float((g0 - g1).abs().max()) <= 1e-3 * float(g0.abs().max())
    # with externally supplied (global) advantage statistics, as in the data-parallel path
    gs = (torch.tensor(0.1, device="cuda"), torch.tensor(1.3, device="cuda"), torch.tensor(96.0, device="cuda"))
    models.FUSED_UPDATE_OPS = False; pol.use_fused_loss = False
    la, _ = pol.minibatch_loss(*args, gs)
    models.FUSED_UPDATE_OPS = True; pol.use_fused_loss = True
    lb, _ = pol.minibatch_loss(*args, gs)
    assert abs(float(la) - float(lb)) <= 1e-4 * max(1.0, abs(float(la)))


def test_main_crowd_eval_entry_point(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "crowd_ppo", "main_crowd_eval.py"), "--test-num", "4", "--num-verts", "1024", "--seed", "1"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Final reward:" in r.stdout
    pk = sorted((tmp_path / "log" / "eval_results" / "crowd-4human").glob("motion_crowd4_*.pkl"))
    assert pk
    d = pickle.load(open(pk[0], "rb"))
    assert d["motion"][0]["blended_marker"].shape == (20, 67, 3) and d["wpath"].shape == (2, 3)


def test_main_egobody_eval_entry_point(tmp_path):
    """crowd_ppo/main_egobody_eval.py drop-in: two people per scene, male and female pairs, ./egobody_tmp_res/<member>.pkl in
    the reference's layout with exactly max_depth primitives each (only max_depth terminates); flagged sequences are dropped
    unless --keep-invalid (random weights leave the walkable polygon at once)."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "crowd_ppo", "main_egobody_eval.py"), "--num-scenes", "5", "--num-verts", "1024",
           "--seed", "2", "--keep-invalid"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Final reward:" in r.stdout and "5 scene(s) written" in r.stdout
    pk = sorted((tmp_path / "egobody_tmp_res").glob("motion_s*_*.pkl"))
    assert len(pk) == 10
    genders = set()
    for f in pk:
        d = pickle.load(open(f, "rb"))
        assert len(d["motion"]) == 11 and d["wpath"].shape == (2, 3) and d["navmesh_path"].endswith("navmesh_tight.ply")
        mp = d["motion"][0]
        assert mp["blended_marker"].shape == (20, 67, 3) and mp["smplx_params"].shape == (1, 20, 93) and mp["betas"].shape == (10,)
        genders.add(mp["gender"])
    assert genders == {"male", "female"}
    a, b = (pickle.load(open(tmp_path / "egobody_tmp_res" / f"motion_s0_{k}.pkl", "rb")) for k in (0, 1))
    assert np.allclose(a["wpath"][0, :2], b["wpath"][1, :2], atol=1e-5) and a["motion"][0]["gender"] == b["motion"][0]["gender"]
    assert not np.array_equal(a["motion"][0]["betas"], b["motion"][0]["betas"])


def test_crowd_eval_bf16_policy_is_statistically_equivalent(tmp_path):
    """Config 5 (bf16 policy): per-episode statistics over 256 four-human scenes (1024 humans, SURVEY 8(d) C5: >= 256 scenes)
    against the fp32 policy, same seeds - statistical parity, not 1e-4: means, and the two-sample Kolmogorov-Smirnov distance of
    the reward and episode-length distributions (critical value at alpha = 0.001 for n = m = 1024: 1.95 sqrt(2 / n) = 0.086).
    EGX_C5_HIST=<file>: write both histograms (committed as profiles/r04_c5_histograms.txt)."""
    import json
    import re
    env = dict(os.environ, PYTHONPATH=ROOT)
    res, dist_ = {}, {}
    S = 256
    for dt in ("fp32", "bf16x2", "bf16"):
        wd = tmp_path / dt
        wd.mkdir()
        cmd = [sys.executable, os.path.join(ROOT, "crowd_ppo", "main_crowd_eval.py"), "--test-num", str(4 * S), "--num-verts", "1024",
               "--seed", "3", "--num-scenes", str(S), "--policy-dtype", dt]
        r = subprocess.run(cmd, cwd=wd, env=dict(env, EGX_CROWD_STATS=str(wd / "stats.json")), capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        m = re.search(r"Final reward: ([-0-9.eE+]+), length: ([-0-9.eE+]+)", r.stdout)
        assert m, r.stdout[-1000:]
        res[dt] = (float(m.group(1)), float(m.group(2)))
        assert ("bf16 operands" in r.stdout) == (dt == "bf16")
        st = json.load(open(wd / "stats.json"))
        assert st["scenes"] == S and st["humans_per_scene"] == 4 and len(st["reward"]) >= 4 * S
        dist_[dt] = (np.asarray(st["reward"][:4 * S]), np.asarray(st["length"][:4 * S]))

    def ks(a, b):
        grid = np.sort(np.concatenate([a, b]))
        return float(np.max(np.abs(np.searchsorted(np.sort(a), grid, side="right") / len(a) - np.searchsorted(np.sort(b), grid, side="right") / len(b))))

    lines = [f"# main_crowd_eval.py, {S} four-human scenes ({4 * S} episodes per policy arithmetic), seed 3, random-init policy"]
    r_edges = np.linspace(min(d[0].min() for d in dist_.values()), max(d[0].max() for d in dist_.values()), 13)
    l_edges = np.arange(0.5, 12.5)
    for dt, (rw, ln) in dist_.items():
        lines.append(f"{dt:>7s}  mean reward {rw.mean():8.4f}  mean length {ln.mean():6.3f}")
        lines.append("         reward hist  " + " ".join(f"{c:4d}" for c in np.histogram(rw, r_edges)[0]))
        lines.append("         length hist  " + " ".join(f"{c:4d}" for c in np.histogram(ln, l_edges)[0]))
    lines.append("         reward bin edges " + " ".join(f"{e:.2f}" for e in r_edges))
    crit = 1.95 * np.sqrt(2.0 / (4 * S))
    for dt in ("bf16x2", "bf16"):
        kr, kl = ks(dist_["fp32"][0], dist_[dt][0]), ks(dist_["fp32"][1], dist_[dt][1])
        lines.append(f"KS distance fp32 vs {dt}: reward {kr:.4f}, length {kl:.4f} (critical value alpha=0.001: {crit:.4f})")
        assert kr <= crit and kl <= crit, (dt, kr, kl, crit)
        (r32, l32), (r16, l16) = res["fp32"], res[dt]
        assert abs(l32 - l16) <= 0.25, res                                  # mean episode length (steps)
        assert abs(r32 - r16) <= 0.05 * max(1.0, abs(r32)), res             # mean episode reward
    print("\n".join(lines))
    out = os.environ.get("EGX_C5_HIST")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def test_update_glue_kernels():
    """egx_gather_rows / egx_adv_stats / egx_track_episode / egx_act_fwd / egx_act_bwd_colsum against torch."""
    from egogen_amd import _lib
    from egogen_amd.fused_ops import adv_stats, gather_rows
    import ctypes as C
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    N, n = 300, 77
    srcs = [torch.randn(N, w, generator=g).cuda() for w in (804, 64, 1, 1, 128, 1, 1, 1)]
    idx = torch.randperm(N, generator=g)[:n].cuda()
    out = gather_rows(idx, srcs)
    for s_, o in zip(srcs, out):
        assert torch.equal(o, s_.index_select(0, idx))
    adv = (torch.randn(256, generator=g) * 3 + 0.7).cuda()
    st = adv_stats(adv)
    assert abs(float(st[0]) - float(adv.mean())) < 1e-6 and abs(float(st[1]) - float(adv.std())) < 1e-5
    # episode bookkeeping
    A = 37
    rew = torch.randn(A, generator=g).cuda(); term = (torch.rand(A, generator=g) < 0.3).int().cuda()
    ep_ret = torch.randn(A, generator=g).cuda(); ep_len = torch.randint(0, 9, (A,), generator=g).float().cuda()
    done = torch.tensor([1.0, 2.0, 3.0]).cuda()
    r0, l0 = ep_ret.clone(), ep_len.clone()
    _lib.check(lib.egx_track_episode(_lib.ptr(rew), _lib.ptr(term), A, _lib.ptr(ep_ret), _lib.ptr(ep_len), _lib.ptr(done),
                                     _lib.current_stream_ptr()), "egx_track_episode")
    d = term.bool()
    assert torch.allclose(done, torch.tensor([1.0, 2.0, 3.0]).cuda() + torch.stack([((r0 + rew) * d).sum(), ((l0 + 1) * d).sum(), d.sum().float()]), atol=1e-5)
    assert torch.allclose(ep_ret, torch.where(d, torch.zeros_like(r0), r0 + rew)) and torch.allclose(ep_len, torch.where(d, torch.zeros_like(l0), l0 + 1))
    # activation forward / backward + bias gradient, all four activation codes, with and without residual
    M, W = 50, 72
    for act, fn in ((0, lambda z: z), (1, torch.tanh), (2, torch.relu), (3, lambda z: torch.nn.functional.leaky_relu(z, 0.01))):
        z = torch.randn(M, W, generator=g).cuda(); res = torch.randn(M, W, generator=g).cuda(); dy = torch.randn(M, W, generator=g).cuda()
        zz = z.clone().requires_grad_(True)
        ref = fn(zz) + res
        ref.backward(dy)
        a = z.clone(); outt = torch.empty_like(z)
        _lib.check(lib.egx_act_fwd(_lib.ptr(a), _lib.ptr(res), _lib.ptr(outt), M, W, act, 0.01, _lib.current_stream_ptr()), "egx_act_fwd")
        assert torch.allclose(outt, ref.detach(), atol=1e-6) and torch.allclose(a, fn(z), atol=1e-6)
        gbuf = torch.empty_like(z); db = torch.full((W,), 0.5).cuda()
        _lib.check(lib.egx_act_bwd_colsum(_lib.ptr(dy), _lib.ptr(a), _lib.ptr(gbuf), _lib.ptr(db), M, W, act, 0.01,
                                          _lib.current_stream_ptr()), "egx_act_bwd_colsum")
        assert torch.allclose(gbuf, zz.grad, atol=1e-5)
        assert torch.allclose(db, 0.5 + zz.grad.sum(0), atol=1e-4)


def test_flat_adamw_clip_matches_torch():
    """egx_adamw_clip_step (flat buffers, clip of the actor+critic prefix) against clip_grad_norm_ + torch.optim.AdamW
    over three steps, and the optimiser state_dict keeps torch's layout."""
    import copy
    from egogen_amd import setup_world as sw

    class _A(_Args):
        update_graph = False
    pol = sw.build_policy(_A())
    ref = sw.build_policy(_A())   # same seed -> identical initial parameters
    ref.use_flat_optimizer = False
    pol.use_flat_optimizer = True
    pol._ensure_flat_grads(); ref._ensure_flat_grads()
    assert pol._flat_optimizer_ready()
    g = torch.Generator().manual_seed(1)
    for step in range(3):
        for (pp, off, n), (rp, roff, _) in zip(pol._flat_layout(), ref._flat_layout()):  # padding stays zero
            gi = (torch.randn(n, generator=g) * (10.0 if step == 1 else 0.001)).cuda()  # clipped and unclipped steps
            pol._flat_grad[off:off + n].copy_(gi); ref._flat_grad[roff:roff + n].copy_(gi)
        pol._clip_and_step(); ref._clip_and_step()
        for (k, a), (_, b) in zip(pol.named_parameters(), ref.named_parameters()):
            assert torch.allclose(a, b, rtol=2e-6, atol=1e-8), (step, k, float((a - b).abs().max()))
    sd = pol.optim.state_dict()
    sr = ref.optim.state_dict()
    assert sd["state"].keys() == sr["state"].keys()
    for i in sd["state"]:
        assert set(sd["state"][i].keys()) == set(sr["state"][i].keys())
        assert float(sd["state"][i]["step"]) == float(sr["state"][i]["step"]) == 3.0
        a, b = sd["state"][i]["exp_avg_sq"], sr["state"][i]["exp_avg_sq"]
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-12), (i, float(((a - b).abs() / (b.abs() + 1e-12)).max()), float(b.abs().max()))
    # loading a torch-layout state back re-adopts it into the flat buffers
    pol.optim.load_state_dict(copy.deepcopy(sr))
    assert pol._flat_optimizer_ready()
    assert float(pol._step_t) == 3.0 and pol.optim.state[next(iter(pol.optim.param_groups[0]["params"]))]["exp_avg"].data_ptr() == pol._flat_m.data_ptr()


def _filled_batch(n_steps, A, seed, pol):
    from egogen_amd.ppo_policy import RolloutBatch
    g = torch.Generator().manual_seed(seed)
    b = RolloutBatch(n_steps, A, "cuda")
    b.state.copy_(torch.randn(b.state.shape, generator=g) * 0.3)
    b.ego.copy_(torch.rand(b.ego.shape, generator=g) * 2 - 1)
    b.dist.copy_(torch.rand(b.dist.shape, generator=g)); b.time.copy_(torch.rand(b.time.shape, generator=g))
    b.act.copy_(torch.randn(b.act.shape, generator=g) * 2.5)   # some ratios leave the clip range
    b.adv.copy_(torch.randn(b.adv.shape, generator=g)); b.returns.copy_(torch.randn(b.returns.shape, generator=g))
    with torch.no_grad():
        _, mu, sigma = pol._dist_params(b.obs_flat())
        lp = pol.log_prob(mu, sigma, b.act.reshape(-1, 128)) + 0.2 * torch.randn(n_steps * A, generator=g).cuda()
        b.logp_old.copy_(lp.reshape(n_steps, A))
    return b


def _assert_grads_close(name, got, ref):
    """Two fp32 evaluations of a leaky-relu network disagree about the side of the kink for the odd pre-activation within
    round-off of zero (about one element per ~1e6: expect one or two in a minibatch of this size).  One flipped mask bit changes
    one row of one weight gradient by ~1e-2 of the tensor's scale and, diluted, everything upstream of it by ~1e-3 (measured:
    every tensor not downstream of a flip agrees to 1e-7..3e-5 relative).  So the criterion is the error NORM - a wrong
    product, transposition or missing term is O(1) in it - plus a cap on any single entry."""
    scale = float(ref.abs().max()) + 1e-12
    d = got - ref
    rel_l2 = float(d.norm()) / (float(ref.norm()) + 1e-12)
    assert rel_l2 <= 1e-2 and float(d.abs().max()) <= 5e-2 * scale, (name, rel_l2, float(d.abs().max()) / scale)


def test_train_step_matches_torch_autograd():
    """csrc/update3.hip: the minibatch as a chain of hand-written launches (forward, clipped-PPO loss, backward: packed bf16x3
    products, fused epilogues, bias gradients through a row of ones) gives the loss terms and EVERY parameter gradient of the
    plain torch expression of ppo_policy.py:189-241."""
    from egogen_amd import models, setup_world as sw
    pol = sw.build_policy(_Args())
    with torch.no_grad():   # non-trivial biases; some raw logvars outside [-2.5, 2.5] so that the clamp mask is exercised
        for p_ in pol.parameters():
            if p_.dim() == 1:
                p_.add_(0.05 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(p_.numel())).cuda())
        pol.actor.pnet.out_fc.bias[128:160] += 4.0
        pol.actor.pnet.out_fc.bias[160:192] -= 4.0
    N = 96
    b = _filled_batch(1, N, 0, pol)
    pol._ensure_flat_grads()
    assert pol._flat_optimizer_ready()
    args = (b.obs_flat(), b.act.reshape(N, 128), b.adv.reshape(N), b.returns.reshape(N), b.logp_old.reshape(N))
    try:
        models.FUSED_UPDATE_OPS = False
        pol.use_fused_loss = False
        pol.zero_grad(set_to_none=True)
        loss, terms = pol.minibatch_loss(*args)
        loss.backward()
        ref = {n_: p_.grad.detach().clone() for n_, p_ in pol.named_parameters()}
        ref_terms = {k: float(v) for k, v in terms.items()}
    finally:
        models.FUSED_UPDATE_OPS = True
        pol.use_fused_loss = True
    pol._ensure_flat_grads()
    pol._flat_grad.fill_(7.0)   # the step WRITES every gradient: whatever was there must be gone
    idx = torch.arange(N, device="cuda")
    log = torch.zeros(6, device="cuda")
    hs = pol._train_handle(N)
    assert hs is not None, "the hand-written update step was not selected"
    pol._fwd_bwd(b, idx, None, log)
    torch.cuda.synchronize()
    log = log.cpu().tolist()
    for i, k in enumerate(("loss", "loss/clip", "loss/vf", "loss/ent", "loss/kld", "approx_kl")):
        assert abs(log[i] - ref_terms[k]) <= 2e-4 * max(1.0, abs(ref_terms[k])), (k, log[i], ref_terms[k])
    for n_, p_ in pol.named_parameters():
        if n_.startswith("_actor_critic."):
            continue
        _assert_grads_close(n_, p_.grad, ref[n_])
    # a second minibatch through the same handle (all buffers reused), other rows
    b2 = _filled_batch(1, N, 1, pol)
    args2 = (b2.obs_flat(), b2.act.reshape(N, 128), b2.adv.reshape(N), b2.returns.reshape(N), b2.logp_old.reshape(N))
    snap = pol._flat_grad.clone()
    pol._fwd_bwd(b2, idx, None, torch.zeros(6, device="cuda"))
    assert float((pol._flat_grad - snap).abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# P3 (crowd_ppo/ppo_policy.py:189-247) against the ORACLE: `oracle.nets.policy_*` + `oracle.ppo.ppo_loss`, differentiated by torch
# autograd in FLOAT64 - the truth - with the same oracle in float32 (the arithmetic of the reference's PyTorch-CPU path) as the
# yardstick of what fp32 costs.
# ---------------------------------------------------------------------------------------------------------------------------
_ORACLE_KEYS = ("loss", "loss/clip", "loss/vf", "loss/ent", "loss/kld")


def _oracle_p3(sd, obs, act, adv, ret, lpo, dtype):
    """Loss terms, every parameter gradient and the pre-activations of the eight 1152-wide layers (both networks), from the
    oracle restatement evaluated in `dtype` on the CPU."""
    from oracle import nets as onets, ppo as oppo
    c = lambda t: t.detach().cpu().to(dtype)
    P = {k: c(v).requires_grad_(True) for k, v in sd.items() if not k.startswith("_actor_critic.")}
    o = {k: c(v) for k, v in obs.items()}
    hx = onets.policy_base(P, o)
    mu, logvar = onets.policy_actor(P, hx)
    value = onets.policy_critic(P, hx)
    loss, terms = oppo.ppo_loss(mu, logvar, value, c(act), c(adv), c(ret), c(lpo), eps_clip=_Args.eps_clip, vf_coef=_Args.vf_coef,
                                ent_coef=_Args.ent_coef)
    loss.backward()
    # pre-activations z of every leaky-ReLU (models_policy_ppo.py:24-39): recomputed layer by layer, no gradient
    zs = []
    with torch.no_grad():
        for net in ("actor.pnet", "critic.vnet"):
            h = hx
            for b in range(2):
                t = h
                for k in range(2):
                    z = torch.nn.functional.linear(t, P[f"{net}.layers.{b}.layers.{k}.weight"], P[f"{net}.layers.{b}.layers.{k}.bias"])
                    zs.append(z)
                    t = torch.nn.functional.leaky_relu(z, 0.01)
                h = t + h
    out = {"loss": float(loss.detach()), **{k: float(v.detach()) for k, v in terms.items()}}
    return out, {k: v.grad.detach().double() for k, v in P.items()}, zs


def _build_policy_one_thread(a):
    """sw.build_policy with one host thread: its orthogonal init is a LAPACK QR whose last bits depend on the thread count, so
    otherwise the weights - and the figures the test below holds to fixed bounds - would change with the host's thread count."""
    from egogen_amd import setup_world as sw
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return sw.build_policy(a)
    finally:
        torch.set_num_threads(n)


def _unambiguous_rows(pol, n_rows, band, seed):
    """The first `n_rows` candidate transitions none of whose 9216 leaky-ReLU arguments lies within `band` x (rms of that
    layer's arguments) of zero IN FLOAT64.  Inside that band two correct evaluations in different arithmetic may take
    different sides of the kink, and each such element changes one row of one weight gradient by O(1) of that row - that is a
    property of the function at that point, not an error of either evaluation, so such transitions are excluded BY THIS
    CRITERION (the band is the mode's round-off, stated by the caller) instead of by a blanket tolerance."""
    n_cand = 8 * n_rows
    b = _filled_batch(1, n_cand, seed, pol)
    args = (b.obs_flat(), b.act.reshape(n_cand, 128), b.adv.reshape(n_cand), b.returns.reshape(n_cand), b.logp_old.reshape(n_cand))
    _, _, zs = _oracle_p3(pol.state_dict(), *args, torch.float64)
    ok = torch.ones(n_cand, dtype=torch.bool)
    for z in zs:
        ok &= (z.abs() >= band * z.pow(2).mean().sqrt()).all(dim=1)
    keep = torch.nonzero(ok).flatten()[:n_rows]
    assert keep.numel() == n_rows, f"only {int(ok.sum())} of {n_cand} candidate rows are unambiguous at band {band}"
    return b, keep.cuda(), float(1.0 - ok.float().mean())


# mode -> (band of the row selection as a multiple of the layer's rms argument, bound on chain error / fp32-yardstick error)
# f32: three bf16 terms per operand = 2^-24 per product: must sit within 3x of what fp32 itself costs (the review's bar).
# bf16x2 / bf16: 2^-17 / 2^-9 per operand - NOT fp32-equivalent by construction; their bound is north_star's 1e-4 relative
# (bf16x2) / a norm bound (bf16), and the table records how far from the yardstick they are.
_P3_MODES = {"f32": (1e-5, 3.0), "bf16x2": (2e-4, None), "bf16": (None, None)}


@pytest.mark.parametrize("mode", ["f32", "bf16x2", "bf16"])
def test_train_step_matches_oracle_fp64(mode):
    """csrc/update3.hip (`egx_policy_train_step`, 256-row minibatch = the training shape) against the float64 oracle of
    ppo_policy.py:189-247: loss terms and EVERY parameter gradient, with |oracle-fp32 - fp64| as the yardstick.
    EGX_P3_TABLE=<file>: append the per-parameter table (committed as profiles/r04_p3_yardstick.txt)."""
    a = _Args()
    a.update_precision = mode
    pol = _build_policy_one_thread(a)
    assert pol.update_precision == mode
    with torch.no_grad():   # non-trivial biases; some raw logvars outside [-2.5, 2.5] so that the clamp mask is exercised
        for p_ in pol.parameters():
            if p_.dim() == 1:
                p_.add_(0.05 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(p_.numel())).cuda())
        pol.actor.pnet.out_fc.bias[128:160] += 4.0
        pol.actor.pnet.out_fc.bias[160:192] -= 4.0
    N = 256
    band, ratio_bound = _P3_MODES[mode]
    if band is not None:
        b, idx, dropped = _unambiguous_rows(pol, N, band, seed=0)
    else:   # bf16 operands: every row has arguments inside the mode's round-off - nothing to select, norm criterion below
        b, idx, dropped = _filled_batch(1, N, 0, pol), torch.arange(N, device="cuda"), 0.0
    sel = lambda t: t.reshape((-1,) + tuple(t.shape[2:]))[idx.to(t.device)]
    obs = {k: v[idx] for k, v in b.obs_flat().items()}
    args = (obs, sel(b.act), sel(b.adv), sel(b.returns), sel(b.logp_old))
    t64, g64, _ = _oracle_p3(pol.state_dict(), *args, torch.float64)
    t32, g32, _ = _oracle_p3(pol.state_dict(), *args, torch.float32)
    # the chain, through GAMMAPPOPolicy._fwd_bwd exactly as learn() drives it
    pol._ensure_flat_grads()
    assert pol._flat_optimizer_ready()
    pol._flat_grad.fill_(7.0)
    log = torch.zeros(6, device="cuda")
    assert pol._train_handle(N) is not None, "the hand-written update step was not selected"
    assert pol._fwd_bwd(b, idx, None, log) == "chain"
    torch.cuda.synchronize()
    log = log.cpu().tolist()
    lines = [f"# mode {mode}: 256-row minibatch, rows with a leaky-ReLU argument within {band} x rms of 0 excluded ({dropped:.0%} of candidates)",
             f"# {'term':<46s} {'fp64':>13s} {'|fp32-fp64|':>12s} {'|chain-fp64|':>12s}"]
    for i, k in enumerate(_ORACLE_KEYS):
        e32, ech = abs(t32[k] - t64[k]), abs(log[i] - t64[k])
        lines.append(f"  {k:<46s} {t64[k]:13.6e} {e32:12.3e} {ech:12.3e}")
        tol = 3.0 * e32 + 2e-6 * max(1.0, abs(t64[k])) if mode == "f32" else (1e-4 if mode == "bf16x2" else 5e-3) * max(1.0, abs(t64[k]))
        assert ech <= tol, (k, log[i], t64[k], e32)
    lines.append(f"# {'parameter':<46s} {'||g64||':>10s} {'rel-L2 fp32':>12s} {'rel-L2 chain':>12s} {'ratio':>7s} {'max fp32':>10s} {'max chain':>10s}")
    worst = 0.0
    for n_, p_ in pol.named_parameters():
        if n_.startswith("_actor_critic."):
            continue
        ref = g64[n_].cuda()
        nrm = float(ref.norm()) + 1e-300
        e32 = (g32[n_].cuda() - ref)
        ech = (p_.grad.double() - ref)
        r32, rch = float(e32.norm()) / nrm, float(ech.norm()) / nrm
        scale = float(ref.abs().max()) + 1e-300
        m32, mch = float(e32.abs().max()) / scale, float(ech.abs().max()) / scale
        ratio = rch / max(r32, 1e-7)   # floor: a tensor fp32 gets right to the last bit does not make the bound 0
        worst = max(worst, ratio)
        lines.append(f"  {n_:<46s} {nrm:10.3e} {r32:12.3e} {rch:12.3e} {ratio:7.2f} {m32:10.2e} {mch:10.2e}")
        if mode == "f32":
            assert rch <= ratio_bound * max(r32, 1e-7), (n_, rch, r32)
            assert mch <= ratio_bound * max(m32, 2e-7), (n_, mch, m32)
        elif mode == "bf16x2":
            assert rch <= 1e-4 and mch <= 1e-4, (n_, rch, mch)          # north_star: 1e-4 relative
        else:
            # operands rounded to bf16 (2^-9 per element) through five layers forward and back, with leaky-ReLU sides decided
            # in that arithmetic: measured 0.5 - 4.2 % per tensor on MI355X (profiles/r04_p3_yardstick.txt); a wrong term,
            # a transposition or a missing skip gradient is O(1)
            assert rch <= 1e-1, (n_, rch)
    lines.append(f"# worst rel-L2 ratio chain / fp32-yardstick: {worst:.2f}")
    out = os.environ.get("EGX_P3_TABLE")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    print("\n".join(lines))


@pytest.mark.parametrize("mode", ["f32", "bf16x2"])
def test_train_step_gradients_on_all_rows_report(mode):
    """The same comparison WITHOUT the leaky-ReLU margin filter of the test above: the first 256 candidate transitions as they
    come - what a user's minibatch looks like.  A pre-activation within the arithmetic's round-off of zero takes the other side of
    the kink in ONE of two correct evaluations; each such element changes one row of one weight gradient by O(1) of that row, in
    the chain and in torch-fp32 alike, so the bound here is the fp32 yardstick's own size on the same rows (the chain may be at
    most 3x further from float64 than fp32 autograd is, plus 1e-4).  EGX_P3_TABLE=<file> appends the table
    (profiles/r05_p3_yardstick.txt: rel-L2 per parameter, unfiltered, next to the yardstick)."""
    from egogen_amd import setup_world as sw
    a = _Args()
    a.update_precision = mode
    pol = sw.build_policy(a)
    with torch.no_grad():
        for p_ in pol.parameters():
            if p_.dim() == 1:
                p_.add_(0.05 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(p_.numel())).cuda())
        pol.actor.pnet.out_fc.bias[128:160] += 4.0
        pol.actor.pnet.out_fc.bias[160:192] -= 4.0
    N = 256
    b = _filled_batch(1, 8 * N, 0, pol)       # the candidate pool of _unambiguous_rows (same seed): its FIRST 256 rows
    idx = torch.arange(N, device="cuda")
    sel = lambda t: t.reshape((-1,) + tuple(t.shape[2:]))[idx.to(t.device)]
    obs = {k: v[idx] for k, v in b.obs_flat().items()}
    args = (obs, sel(b.act), sel(b.adv), sel(b.returns), sel(b.logp_old))
    t64, g64, zs = _oracle_p3(pol.state_dict(), *args, torch.float64)
    t32, g32, _ = _oracle_p3(pol.state_dict(), *args, torch.float32)
    band = {"f32": 1e-5, "bf16x2": 2e-4}[mode]
    near = sum(int(((z.abs() / z.pow(2).mean().sqrt()) < band).sum()) for z in zs)
    pol._ensure_flat_grads()
    assert pol._flat_optimizer_ready()
    log = torch.zeros(6, device="cuda")
    assert pol._train_handle(N) is not None
    assert pol._fwd_bwd(b, idx, None, log) == "chain"
    torch.cuda.synchronize()
    lines = [f"# mode {mode}: the first 256 candidate rows, NO margin filter ({near} of {sum(z.numel() for z in zs)} leaky-ReLU arguments within "
             f"{band} x rms of zero)",
             f"# {'parameter':<46s} {'||g64||':>10s} {'rel-L2 fp32':>12s} {'rel-L2 chain':>12s} {'ratio':>7s}"]
    worst = 0.0
    for n_, p_ in pol.named_parameters():
        if n_.startswith("_actor_critic."):
            continue
        ref = g64[n_].cuda()
        nrm = float(ref.norm()) + 1e-300
        r32 = float((g32[n_].cuda() - ref).norm()) / nrm
        rch = float((p_.grad.double() - ref).norm()) / nrm
        worst = max(worst, rch)
        lines.append(f"  {n_:<46s} {nrm:10.3e} {r32:12.3e} {rch:12.3e} {rch / max(r32, 1e-7):7.2f}")
        assert rch <= 3.0 * r32 + (1e-4 if mode == "f32" else 2e-3), (n_, rch, r32)
    lines.append(f"# worst rel-L2 of the chain on unfiltered rows: {worst:.3e}")
    out = os.environ.get("EGX_P3_TABLE")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    print("\n".join(lines))


def test_learn_matches_oracle_fp64_parameters():
    """End to end: two passes of `learn()` (8 optimiser steps, replayed graphs) in every update mode against the same schedule
    done in float64 with the oracle's loss (torch AdamW + clip_grad_norm_ on float64 copies, the reference's optimiser calls,
    ppo_policy.py:243-247).  AdamW normalises each step to ~lr, so a gradient entry within round-off of zero moves its
    parameter by up to 2 lr per step in either arithmetic: the bound is that, plus the requirement that all but a small fraction of
    the parameters agree with float64 as closely as the autograd-node path on torch fp32 does."""
    import copy
    from egogen_amd import setup_world as sw
    from oracle import nets as onets, ppo as oppo
    n_steps, A, bs = 4, 64, 64
    base = sw.build_policy(_Args())
    sd0 = copy.deepcopy(base.state_dict())
    b = _filled_batch(n_steps, A, 3, base)
    N = n_steps * A
    # float64 reference of the schedule
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in sd0.items() if not k.startswith("_actor_critic.")}
    order = [k for k in P if not k.startswith("shared_net.")] + [k for k in P if k.startswith("shared_net.")]   # ActorCritic.parameters(): actor, critic, shared_net
    opt = torch.optim.AdamW([P[k] for k in order], lr=_Args.lr)
    wd = base.optim.param_groups[0]["weight_decay"]
    for g_ in opt.param_groups:
        g_["weight_decay"] = wd
    clip_keys = [k for k in order if not k.startswith("shared_net.")]
    pg = torch.Generator().manual_seed(11)
    flat = lambda t: t.reshape((N,) + tuple(t.shape[2:])).cpu().double()
    obs_all = {k: v.cpu().double() for k, v in b.obs_flat().items()}
    for _ in range(2):
        perm = torch.randperm(N, generator=pg)
        for s0 in range(0, N, bs):
            i = perm[s0:s0 + bs]
            o = {k: v[i] for k, v in obs_all.items()}
            hx = onets.policy_base(P, o)
            mu, lv = onets.policy_actor(P, hx)
            val = onets.policy_critic(P, hx)
            loss, _ = oppo.ppo_loss(mu, lv, val, flat(b.act)[i], flat(b.adv)[i], flat(b.returns)[i], flat(b.logp_old)[i],
                                    eps_clip=_Args.eps_clip, vf_coef=_Args.vf_coef, ent_coef=_Args.ent_coef)
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_([P[k] for k in clip_keys], _Args.max_grad_norm)
            opt.step()
    lr, steps = _Args.lr, 2 * (N // bs)
    frac = {}
    for mode, kw in (("autograd-nodes fp32", dict(train_step=False)), ("f32", {}), ("bf16x2", {}), ("bf16", {})):
        a = _Args()
        a.update_graph = True
        if "train_step" not in kw:
            a.update_precision = mode
        pol = sw.build_policy(a)
        if "train_step" in kw:
            pol.use_train_step = False
        pol.load_state_dict(sd0)
        pol._perm_gen.manual_seed(11)
        pol.learn(b, bs, 1)
        pol.learn(b, bs, 1)
        far, tot, dmax, err2, upd2 = 0, 0, 0.0, 0.0, 0.0
        for k, v in pol.state_dict().items():
            if k.startswith("_actor_critic."):
                continue
            d = (v.detach().cpu().double() - P[k].detach()).abs()
            dmax = max(dmax, float(d.max()))
            far += int((d > 2e-5).sum()); tot += d.numel()
            err2 += float((d * d).sum())
            upd2 += float(((P[k].detach() - sd0[k].cpu().double()) ** 2).sum())
        frac[mode] = (far / tot, (err2 / upd2) ** 0.5)
        assert dmax <= 2 * lr * steps * 1.01, (mode, dmax)
    # (fraction of parameters further than 2e-5 from the float64 schedule, ||theta - theta64|| / ||theta64 - theta0||)
    print("distance from the float64 schedule after 8 optimiser steps:", {k: ("%.4f" % a, "%.4f" % b) for k, (a, b) in frac.items()})
    out = os.environ.get("EGX_P3_TABLE")
    if out:
        with open(out, "a") as f:
            f.write("# learn() x 2 (8 optimiser steps, 64-row minibatches, replayed graphs) against the same schedule in float64:\n"
                    "# mode                   share of parameters > 2e-5 away   ||theta - theta64|| / ||theta64 - theta0||\n")
            for k, (a, b) in frac.items():
                f.write(f"  {k:<22s} {a:10.4f} {b:34.4f}\n")
            f.write("\n")
    yard = frac["autograd-nodes fp32"]
    # the hand-written chain in its fp32-equivalent mode is as close to float64 as torch fp32 autograd on library products is
    assert frac["f32"][0] <= 3 * yard[0] + 1e-4 and frac["f32"][1] <= 3 * yard[1] + 1e-4, frac
    # two bf16 terms per operand: every gradient within 1e-4 of float64 (test above) -> the same trajectory as fp32 up to the
    # AdamW sign noise both share; bf16 operands: a different (noisier) trajectory, bounded, reported
    assert frac["bf16x2"][0] <= 3 * yard[0] + 1e-4 and frac["bf16x2"][1] <= 3 * yard[1] + 1e-4, frac
    assert frac["bf16"][1] <= 0.5, frac


def test_ppo_options_of_main_ppo_run_through_the_policy():
    """--rew-norm / --value-clip / --dual-clip / --recompute-adv (main_ppo.py:54-67 -> ppo_policy.py:80-86,118-135,185-186,
    204-221): accepted like the reference class accepts them; the loss options route the minibatch through the torch expression
    (the hand-written chain implements the default loss only), reward normalisation rescales the critic's values for the GAE
    scan and the returns by the running standard deviation of the un-normalised returns."""
    from egogen_amd import setup_world as sw
    from oracle import ppo as oppo

    class A(_Args):
        rew_norm = True; value_clip = 1; dual_clip = 2.0; recompute_adv = 1
        update_graph = False
    pol = sw.build_policy(A())
    assert pol._rew_norm and pol._value_clip and pol._dual_clip == 2.0 and pol._recompute_adv
    b = _filled_batch(3, 32, 9, pol)
    b.term.copy_((torch.rand(3, 32, generator=torch.Generator().manual_seed(1)) < 0.2).int())
    b.rew.copy_(torch.randn(3, 32, generator=torch.Generator().manual_seed(2)))
    pol.ret_rms.update(np.array([0.0, 4.0, -4.0, 8.0]))          # some history: var = 19
    var0 = pol.ret_rms.var
    pol.process_fn(b)
    v = b.values.cpu().double().numpy() * np.sqrt(var0 + np.finfo(np.float32).eps)
    ret, adv = oppo.gae_returns(v[:3].T, v[1:].T, b.rew.cpu().numpy().T, b.term.cpu().numpy().T.astype(bool), np.zeros((32, 3), bool), 0.99, 0.95)
    np.testing.assert_allclose(b.adv.cpu().numpy().T, adv, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(b.returns.cpu().numpy().T, ret / np.sqrt(var0 + np.finfo(np.float32).eps), rtol=1e-5, atol=1e-5)
    assert pol.ret_rms.count == 4 + 96 and pol.ret_rms.var != var0
    before = torch.cat([q.detach().flatten() for q in pol.parameters()]).clone()
    out = pol.learn(b, 32, 2)                                      # repeat 2: the second pass recomputes the advantages
    assert len(out["loss"]) in (3, 6) and np.isfinite(out["loss"]).all()
    assert set(pol.update_paths) == {"autograd"} and not pol._train_handles, pol.update_paths
    assert float((torch.cat([q.detach().flatten() for q in pol.parameters()]) - before).abs().max()) > 0


def test_merged_last_minibatch_reads_current_weight_images():
    """Batch.split(merge_last=True): 160 transitions at batch size 64 = minibatches of 64 and 96 rows -> TWO train handles, the
    second created after the graphs of the first size were captured.  A captured (clip + AdamW + image refresh) graph refreshes
    the handles it knew at capture time only; the late handle must not forward through weights that are a step old: graph mode
    and eager mode perform the same launches on the same data, so their parameters must agree to the last bit."""
    from egogen_amd import setup_world as sw
    out = []
    for graph in (False, True):
        a = _Args()
        a.update_graph = graph
        pol = sw.build_policy(a)
        if out:
            pol.load_state_dict(out[0][2])
        sd0 = {k: v.clone() for k, v in pol.state_dict().items()}
        b = _filled_batch(5, 32, 4, pol)
        pol._perm_gen.manual_seed(5)
        losses = []
        for _ in range(3):
            losses += pol.learn(b, 64, 1)["loss"]
        assert set(pol._train_handles) == {64, 96}, pol._train_handles.keys()
        if graph:
            assert pol.update_paths.get("chain+graph", 0) >= 2 and pol.update_paths.get("chain", 0) >= 3, pol.update_paths
            assert not any(v.get("failed") for v in pol._graph_cache.values())
        out.append((losses, torch.cat([q.detach().flatten() for q in pol.parameters()]).clone(), sd0))
    np.testing.assert_allclose(out[1][0], out[0][0], rtol=1e-6, atol=1e-7)
    d = (out[1][1] - out[0][1]).abs()
    assert float(d.max()) <= 1e-7, (float(d.max()), int((d > 0).sum()))


def test_learn_with_train_step_equals_autograd_nodes():
    """GAMMAPPOPolicy.learn over a whole collect: the hand-written step (eager and as replayed HIP graphs) performs the same
    optimiser steps as the autograd-node path - losses of every minibatch and the parameters afterwards."""
    from egogen_amd import setup_world as sw

    def make(train_step, graph):
        a = _Args()
        a.update_graph = graph
        p = sw.build_policy(a)
        p.use_train_step = train_step
        return p

    ref, eager, graph = make(False, False), make(True, False), make(True, True)
    for p in (eager, graph):
        p.load_state_dict(ref.state_dict())
    b = _filled_batch(4, 64, 3, ref)
    out = []
    for p in (ref, eager, graph):
        p._perm_gen.manual_seed(11)
        l1 = p.learn(b, 64, 1)
        l2 = p.learn(b, 64, 1)   # second pass: replayed graphs, refreshed weight images
        out.append((l1["loss"] + l2["loss"], torch.cat([q.detach().flatten() for q in p.parameters()]).clone()))
    assert eager._train_handles and graph._train_handles and not ref._train_handles
    assert not any(v.get("failed") for v in graph._graph_cache.values()), "graph capture fell back to eager"
    for name, (losses, params) in zip(("eager", "graph"), out[1:]):
        np.testing.assert_allclose(losses, out[0][0], rtol=1e-3, atol=5e-5, err_msg=name)
        # AdamW's first steps move every parameter by ~lr whatever the size of its gradient, so round-off-level differences
        # of near-zero gradients show up as differences of up to 2 lr per step: bound by that, and require that nearly
        # all parameters agree far more closely
        d = (params - out[0][1]).abs()
        assert float(d.max()) <= 8 * 2 * 3e-4 and float((d > 2e-5).float().mean()) <= 0.02, (name, float(d.max()))
    # the rollout forward reads the images the update keeps current: same action means as a fresh runner on the same weights
    from egogen_amd.models import PolicyHipRunner
    obs = {k: v[:64] for k, v in b.obs_flat().items()}
    o1 = eager._runner.forward(obs)
    o2 = PolicyHipRunner(eager.shared_net, eager.actor, eager.critic).forward(obs)
    assert max_abs(o1["mu"].cpu(), o2["mu"].cpu()) <= 1e-6 and max_abs(o1["value"].cpu(), o2["value"].cpu()) <= 1e-6
    # ... and follows a load_state_dict between updates (torch-visible in-place edit of the weights: the runner asks the
    # owner of the adopted images to re-make them)
    sd = {k: (v * 1.05 if v.is_floating_point() else v) for k, v in ref.state_dict().items()}
    eager.load_state_dict(sd)
    ref.load_state_dict(sd)
    o3 = eager._runner.forward(obs)
    o4 = PolicyHipRunner(ref.shared_net, ref.actor, ref.critic).forward(obs)
    assert max_abs(o3["mu"].cpu(), o4["mu"].cpu()) <= 1e-6 and max_abs(o3["value"].cpu(), o4["value"].cpu()) <= 1e-6
    assert max_abs(o3["mu"].cpu(), o1["mu"].cpu()) > 1e-4          # the weights did change
