"""The head launch of the update's minibatch (`egx_update_head_kernel`, csrc/update3.hip), the device-side minibatch cursor and
learn()'s conditional weight-image refreshes, on a synthetic rollout of 4 x 24 = 96 rows.

The head launch computes the same values from the same inputs in the same order as the launches it replaces (row gather,
advantage statistics, input images, positional encoding), so everything downstream of it except the four loss sums (float
atomics) is held to `torch.equal` against the old launches (EGX_UPDATE_HEAD=0, read when a train handle is created).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

N_STEPS, AGENTS = 4, 24
N = N_STEPS * AGENTS
_SENT = -777.25          # exact in fp32
_SENT_IDX = 10 ** 12     # an index no rollout has: read as a row index it is clamped to the last row, and the gathered rows differ


class _Args:
    seed = 0; lr = 3e-4; gamma = 0.99; gae_lambda = 0.95; max_grad_norm = 0.1; vf_coef = 1.0; ent_coef = 0.01
    weight_kld = 0; rew_norm = False; eps_clip = 0.1; value_clip = 0; dual_clip = None; norm_adv = 1; recompute_adv = 0
    deterministic_eval = False


_STATE = {}


def _initial_state():
    """One initialisation (main_ppo's orthogonal init is a QR of every weight matrix: built once, shared by every policy here)."""
    if "sd" not in _STATE:
        from egogen_amd import setup_world as sw
        pol = sw.build_policy(_Args())
        with torch.no_grad():   # non-trivial biases, some logvars outside the clamp range
            for p_ in pol.parameters():
                if p_.dim() == 1:
                    p_.add_(0.05 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(p_.numel())).cuda())
            pol.actor.pnet.out_fc.bias[128:160] += 4.0
            pol.actor.pnet.out_fc.bias[160:192] -= 4.0
        _STATE["sd"] = {k: v.detach().clone() for k, v in pol.state_dict().items()}
    return _STATE["sd"]


def _new_policy(graph, prec, sd=None):
    """setup_world.build_policy without its initialisation: the weights come from `sd`."""
    from egogen_amd import setup_world as sw
    from egogen_amd.models import ActorCritic, GAMMAActor, GAMMACritic, GAMMAPolicyBase
    from egogen_amd.ppo_policy import GAMMAPPOPolicy
    a = _Args()
    pc = sw.POLICY_CFG
    actor, critic, shared = GAMMAActor(pc), GAMMACritic(pc), GAMMAPolicyBase(pc)
    ac = ActorCritic(actor, critic, shared)
    ac.to("cuda")
    optim = torch.optim.AdamW(ac.parameters(), lr=a.lr, weight_decay=0.01, **(dict(capturable=True, foreach=True) if graph else {}))
    pol = GAMMAPPOPolicy(actor, critic, shared, optim, None, discount_factor=a.gamma, gae_lambda=a.gae_lambda,
                         max_grad_norm=a.max_grad_norm, vf_coef=a.vf_coef, ent_coef=a.ent_coef, weight_kld=a.weight_kld,
                         reward_normalization=a.rew_norm, eps_clip=a.eps_clip, value_clip=a.value_clip, dual_clip=a.dual_clip,
                         advantage_normalization=a.norm_adv, recompute_advantage=a.recompute_adv,
                         deterministic_eval=a.deterministic_eval, seed=a.seed, use_update_graph=graph, update_precision=prec)
    pol.load_state_dict(_initial_state() if sd is None else sd)
    return pol


def _batch(n_steps=N_STEPS):
    """The synthetic rollout: built once per size from the initial weights and only ever read."""
    key = ("batch", n_steps)
    if key not in _STATE:
        from egogen_amd.ppo_policy import RolloutBatch
        pol = _new_policy(False, "f32")
        g = torch.Generator().manual_seed(11)
        b = RolloutBatch(n_steps, AGENTS, "cuda")
        b.state.copy_(torch.randn(b.state.shape, generator=g) * 0.3)
        b.ego.copy_(torch.rand(b.ego.shape, generator=g) * 2 - 1)
        b.dist.copy_(torch.rand(b.dist.shape, generator=g)); b.time.copy_(torch.rand(b.time.shape, generator=g))
        b.act.copy_(torch.randn(b.act.shape, generator=g) * 2.5)
        b.adv.copy_(torch.randn(b.adv.shape, generator=g)); b.returns.copy_(torch.randn(b.returns.shape, generator=g))
        b.mu.copy_(torch.randn(b.mu.shape, generator=g))
        with torch.no_grad():
            _, mu, sigma = pol._dist_params(b.obs_flat())
            lp = pol.log_prob(mu, sigma, b.act.reshape(-1, 128)) + 0.2 * torch.randn(n_steps * AGENTS, generator=g).cuda()
            b.logp_old.copy_(lp.reshape(n_steps, AGENTS))
        _STATE[key] = b
    return _STATE[key]


def _run_learn(monkeypatch, head, graph, prec, batch_size, perms=None, n_steps=N_STEPS):
    """One learn() pass; returns the policy, the logged terms and the flat gradient each optimiser step consumed."""
    monkeypatch.setenv("EGX_UPDATE_HEAD", "1" if head else "0")
    pol = _new_policy(graph, prec)
    if perms is not None:
        pol._perm_queue = [p.clone() for p in perms]
    grads = []
    pol._after_minibatch = lambda i: grads.append(pol._flat_grad.clone())
    stats = pol.learn(_batch(n_steps), batch_size, 1)
    torch.cuda.synchronize()
    for hs in pol._train_handles.values():
        assert hs["head"] == head
    return pol, stats, grads


def _assert_same_training(new, old, exact_steps=None):
    """`exact_steps`: the first so many optimiser steps are held to bit equality (None: all of them, and then the parameters and
    both moments after the last one as well)."""
    (pn, sn, gn), (po, so, go) = new, old
    assert pn.update_paths == po.update_paths, (pn.update_paths, po.update_paths)
    assert len(gn) == len(go) > 0
    if exact_steps is None:
        for name in ("_flat_p", "_flat_m", "_flat_v"):
            assert torch.equal(getattr(pn, name), getattr(po, name)), name
    for i in range(len(gn) if exact_steps is None else exact_steps):
        assert torch.equal(gn[i], go[i]), f"flat gradient of step {i}"
    for k in sn:   # the loss sums are float atomics: last bits only
        assert len(sn[k]) == len(so[k]) == len(gn)
        for a, b in zip(sn[k], so[k]):
            assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (k, sn[k], so[k])


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("prec", ["bf16x2", "f32"])
@pytest.mark.parametrize("batch_size", [32, 64])
def test_head_launch_trains_bit_for_bit_like_the_old_launches(monkeypatch, batch_size, prec, graph):
    """Minibatch 32: three optimiser steps (replayed graphs with `graph`).  Minibatch 64: 96 rows leave a ragged rest of 32 that
    Batch.split(merge_last=True) merges - the 96-row minibatch runs eagerly through the same entry with cursor 0."""
    new = _run_learn(monkeypatch, True, graph, prec, batch_size)
    old = _run_learn(monkeypatch, False, graph, prec, batch_size)
    want = {"chain+graph" if graph else "chain": 3} if batch_size == 32 else {"chain": 1}
    assert new[0].update_paths == want, new[0].update_paths
    _assert_same_training(new, old)


def test_replays_followed_by_a_ragged_eager_chain_minibatch(monkeypatch):
    """12 x 24 = 288 rows at minibatch 64: three replays, then the merged 96-row rest eagerly through a handle of its own size
    (created in mid-epoch), cursor 0 and its own index buffer."""
    new = _run_learn(monkeypatch, True, True, "bf16x2", 64, n_steps=12)
    old = _run_learn(monkeypatch, False, True, "bf16x2", 64, n_steps=12)
    assert new[0].update_paths == {"chain+graph": 3, "chain": 1}, new[0].update_paths
    assert set(new[0]._train_handles) == {64, 96}
    _assert_same_training(new, old)


def test_replays_followed_by_an_autograd_minibatch(monkeypatch):
    """5 x 24 = 120 rows at minibatch 32: two replays, then the merged 56-row rest - not a multiple of 32 rows, so it runs the
    autograd nodes, whose bias gradients are sums of float atomics (egx_act_bwd_colsum: four row blocks at 2 x 56 GRU rows) and
    not reproducible to the bit.  Bit equality is held up to the last replay; the log keeps the minibatch order across the two
    paths; after the autograd step the parameters can differ by what two AdamW steps of opposite sign move one (2 lr)."""
    new = _run_learn(monkeypatch, True, True, "bf16x2", 32, n_steps=5)
    old = _run_learn(monkeypatch, False, True, "bf16x2", 32, n_steps=5)
    assert new[0].update_paths == {"chain+graph": 2, "autograd": 1}, new[0].update_paths
    _assert_same_training(new, old, exact_steps=2)
    assert float((new[0]._flat_p - old[0]._flat_p).abs().max()) <= 2 * _Args.lr


def test_log_rows_land_in_minibatch_order(monkeypatch):
    """Rows 0 and N - 1 in the same (second) minibatch of an injected permutation; the three minibatches' losses differ by far
    more than the bound, so a log row in the wrong place fails."""
    g = torch.Generator().manual_seed(3)
    mid = torch.randperm(N - 2, generator=g) + 1
    perm = torch.cat([mid[:32], torch.tensor([0, N - 1]), mid[32:]])
    assert sorted(perm.tolist()) == list(range(N)) and {0, N - 1} <= set(perm[32:64].tolist())
    new = _run_learn(monkeypatch, True, True, "bf16x2", 32, perms=[perm])
    old = _run_learn(monkeypatch, False, True, "bf16x2", 32, perms=[perm])
    _assert_same_training(new, old)
    loss = new[1]["loss"]
    assert min(abs(loss[i] - loss[j]) for i in range(3) for j in range(i)) > 1e-3 * max(map(abs, loss)), loss
    (st,) = new[0]._graph_cache.values()
    dev_log = st["log"].cpu()
    for k in range(3):   # the device log's rows are the minibatches, in order
        assert abs(float(dev_log[k, 0]) - loss[k]) == 0.0, (k, dev_log[:, 0], loss)
    assert torch.equal(st["perm"].cpu(), perm)
    # the persistent buffers of the graphs hold exactly the epoch: N / 32 minibatches of indices, log rows and no more
    assert st["perm"].shape == (N,) and st["perm"].dtype == torch.long and st["log"].shape == (N // 32, 6) and st["rows"] == N // 32
    (hs,) = new[0]._train_handles.values()
    assert not {"state", "egosensing", "dist", "time"} & set(hs)   # no compact observation buffer exists with the head
    assert [tuple(hs[k].shape) for k in ("act", "adv", "ret", "logp_old")] == [(32, 128), (32, 1), (32, 1), (32, 1)]


def test_cursor_counts_the_replays_of_an_epoch(monkeypatch):
    monkeypatch.setenv("EGX_UPDATE_HEAD", "1")
    pol = _new_policy(True, "bf16x2")
    seen = []
    pol._after_minibatch = lambda i: seen.append(int(next(iter(pol._graph_cache.values()))["cursor"]))
    pol.learn(_batch(), 32, 1)
    (st,) = pol._graph_cache.values()
    assert seen == [1, 2, 3] and int(st["cursor"]) == 3, seen
    pol.learn(_batch(), 32, 2)   # two epochs: the cursor starts from zero in each
    if len(seen) == 9:
        assert seen[3:] == [1, 2, 3, 1, 2, 3], seen
    else:                        # the approximate-KL early stop ended the pass after its first epoch
        assert seen[3:] == [1, 2, 3], seen


class _Guarded:
    """`n` elements between `pad` sentinel elements."""

    def __init__(self, n, dtype=torch.float32, sent=_SENT, pad=64):
        self.buf = torch.full((n + 2 * pad,), sent, dtype=dtype, device="cuda")
        self.t, self.pad, self.n, self.sent = self.buf[pad:pad + n], pad, n, sent

    def check(self, what):
        assert bool((self.buf[:self.pad] == self.sent).all()), f"{what}: written in front"
        assert bool((self.buf[self.pad + self.n:] == self.sent).all()), f"{what}: written behind"


@pytest.mark.parametrize("cursor", [None, 0, 1, 2, 7])
def test_head_launch_alone(monkeypatch, cursor):
    """`egx_policy_train_head` on guarded buffers: the compact rows are rows perm[k n + r] of the rollout, the two statistics are
    the bits of egx_adv_stats on the gathered advantages, row k of the log is cleared and no other, and nothing is written in
    front of or behind the permutation, the log or a compact buffer.  A cursor past the end (7) is held at the last minibatch."""
    from egogen_amd import _lib
    from egogen_amd.fused_ops import adv_stats
    monkeypatch.setenv("EGX_UPDATE_HEAD", "1")
    n, rows = 32, 3
    if "head_pol" not in _STATE:
        pol = _new_policy(False, "bf16x2")
        pol._ensure_flat_grads()
        assert pol._flat_optimizer_ready()
        _STATE["head_pol"] = pol
    pol = _STATE["head_pol"]
    hs = pol._train_handle(n)
    assert hs is not None and hs["head"]
    b = _batch()
    k = 0 if cursor is None else min(cursor, rows - 1)
    perm_rows = rows if cursor is not None else 1
    perm = _Guarded(perm_rows * n, torch.long, _SENT_IDX)
    perm.t.copy_(torch.randperm(N, generator=torch.Generator().manual_seed(5))[:perm_rows * n])
    log, act_c, stats = _Guarded(perm_rows * 6), _Guarded(n * 128), _Guarded(2)
    adv_c, ret_c, lpo_c = _Guarded(n), _Guarded(n), _Guarded(n)
    log.t.fill_(3.5)
    cur = torch.tensor(cursor, dtype=torch.int32, device="cuda") if cursor is not None else None
    obs = b.obs_flat()
    hd = _lib.UpdateHead()
    hd.perm, hd.cursor, hd.max_cursor, hd.num_src_rows = perm.t.data_ptr(), (cur.data_ptr() if cur is not None else None), perm_rows - 1, N
    hd.state, hd.egosensing, hd.dist, hd.time = (obs[key].data_ptr() for key in ("state", "egosensing", "dist", "time"))
    hd.act, hd.adv, hd.ret, hd.logp_old = b.act.data_ptr(), b.adv.data_ptr(), b.returns.data_ptr(), b.logp_old.data_ptr()
    hd.act_c, hd.adv_c, hd.ret_c, hd.logp_old_c = act_c.t.data_ptr(), adv_c.t.data_ptr(), ret_c.t.data_ptr(), lpo_c.t.data_ptr()
    hd.stats, hd.compute_stats, hd.log = stats.t.data_ptr(), 1, log.t.data_ptr()
    _lib.check(_lib.load().egx_policy_train_head(hs["h"], C.byref(hd), _lib.current_stream_ptr()), "egx_policy_train_head")
    torch.cuda.synchronize()
    idx = perm.t[k * n:(k + 1) * n]
    assert torch.equal(act_c.t.view(n, 128), b.act.reshape(N, 128).index_select(0, idx))
    assert torch.equal(adv_c.t, b.adv.reshape(N).index_select(0, idx))
    assert torch.equal(ret_c.t, b.returns.reshape(N).index_select(0, idx))
    assert torch.equal(lpo_c.t, b.logp_old.reshape(N).index_select(0, idx))
    ref = adv_stats(b.adv.reshape(N).index_select(0, idx))
    assert torch.equal(stats.t.view(torch.int32), ref.view(torch.int32)), (stats.t, ref)
    want_log = torch.full((perm_rows, 6), 3.5, device="cuda")
    want_log[k] = 0.0
    assert torch.equal(log.t.view(perm_rows, 6), want_log)
    for what, gbuf in (("perm", perm), ("log", log), ("act", act_c), ("adv", adv_c), ("ret", ret_c), ("logp_old", lpo_c), ("stats", stats)):
        gbuf.check(what)


def test_refresh_only_when_something_changed(monkeypatch):
    """learn() re-makes the weight images at its top and bottom only when a parameter's version or a precision differs from what
    the last refresh saw; load_state_dict and a change of the rollout precision still reach the next forward."""
    from egogen_amd import _lib
    lib = _lib.load()
    monkeypatch.setenv("EGX_UPDATE_HEAD", "1")
    g = torch.Generator().manual_seed(21)
    obs = {"state": (torch.randn(32, 2, 402, generator=g) * 0.3).cuda(), "egosensing": (torch.rand(32, 2, 32, generator=g) * 2 - 1).cuda(),
           "dist": torch.rand(32, generator=g).cuda(), "time": torch.rand(32, generator=g).cuda()}

    def fresh_values(sd):
        return _new_policy(False, "bf16x2", sd=sd).values(obs).clone()

    pol = _new_policy(True, "bf16x2")
    assert lib.egx_policy_get_precision() == 0
    try:
        pol.values(obs)
        pol.learn(_batch(), 32, 1)
        assert pol.update_paths == {"chain+graph": 3}
        pol.values(obs)                # the rollout runner's own check sees the capture's restored snapshot (load_state_dict) once
        before = dict(pol.refresh_counts)
        pol.learn(_batch(), 32, 1)     # undisturbed: the replays' captured refreshes are the only ones
        assert pol.refresh_counts == before, (before, pol.refresh_counts)
        pol.values(obs)                # ... and the forward after it asks for none either
        assert pol.refresh_counts == before, (before, pol.refresh_counts)
        sd = {k: v.detach().clone() for k, v in pol.state_dict().items()}
        assert torch.equal(pol.values(obs), fresh_values(sd)), "images after replayed optimiser steps"
        # perturbed weights
        sd2 = {k: v + 0.01 * torch.randn(v.shape, generator=g).cuda() for k, v in sd.items()}
        pol.load_state_dict(sd2)
        assert torch.equal(pol.values(obs), fresh_values(sd2)), "images after load_state_dict"
        pol.learn(_batch(), 32, 1)     # ... and learn() after it runs on the loaded weights' images whether or not a forward came first
        # the rollout arithmetic changes: two planes, then back to three
        _lib.check(lib.egx_policy_set_precision(2), "egx_policy_set_precision")
        sd3 = {k: v.detach().clone() for k, v in pol.state_dict().items()}
        assert torch.equal(pol.values(obs), fresh_values(sd3)), "images after a change of the rollout precision"
        pol.learn(_batch(), 32, 1)
        _lib.check(lib.egx_policy_set_precision(0), "egx_policy_set_precision")
        sd4 = {k: v.detach().clone() for k, v in pol.state_dict().items()}
        assert torch.equal(pol.values(obs), fresh_values(sd4)), "images after the precision went back to three planes"
    finally:
        lib.egx_policy_set_precision(0)


def test_learn_refreshes_after_load_state_dict_without_a_forward(monkeypatch):
    """load_state_dict directly before learn(): the refresh at learn()'s top is the one that sees it."""
    monkeypatch.setenv("EGX_UPDATE_HEAD", "1")
    pol = _new_policy(True, "bf16x2")
    pol.learn(_batch(), 32, 1)
    sd = _initial_state()
    pol.load_state_dict(sd)
    for st in pol.optim.state.values():
        for v in st.values():
            if torch.is_tensor(v):
                v.zero_()
    top = pol.refresh_counts["learn_top"]
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(9))
    pol._perm_queue = [perm.clone()]
    pol.learn(_batch(), 32, 1)
    assert pol.refresh_counts["learn_top"] == top + 1
    ref = _new_policy(True, "bf16x2")
    ref._perm_queue = [perm.clone()]
    ref.learn(_batch(), 32, 1)
    assert torch.equal(pol._flat_p, ref._flat_p)
