"""The epilogues of egx_dense3_kernel / egx_gru3_kernel (csrc/dense3.hip, csrc/gru3.hip) request everything they read from memory as one batch
ahead of the reduction barrier and store everything after the last load.  A prefetch taken for the wrong element, a load or a
store outside the matrix, or a store that went missing shows at the smallest shapes with ragged tiles, so these tests drive the
three entry points built on the two kernels at such shapes:

  * results against the oracle, with the tolerances of the existing tests of the same entry points
    (test_nets_gpu.py: test_sample_prior_matches_oracle, test_policy_matches_reference_golden,
    test_policy_bf16_mode_is_close_to_fp32_and_restorable; test_trainer_gpu.py: test_train_step_matches_torch_autograd);
  * the rows of a small call equal the same rows of a larger call BIT FOR BIT (an element's arithmetic does not depend on how
    many rows the call has; an operand read from another row breaks this);
  * every fp32 output - and the entry point's whole workspace - lies between sentinel words that must survive, and no sentinel
    survives inside an output;
  * the same call twice gives the same bits.
"""
import numpy as np
import pytest
import torch

from tests.helpers import load_golden, max_abs, rebuild_state_dict

pytestmark = pytest.mark.gpu

_SENT = -777.25   # exact in fp32; no network output takes this value


class _Guarded:
    """An fp32 output of `shape` with `pad` sentinel words in front of it and behind it (the outputs are dense: no padding
    columns to guard inside them)."""

    def __init__(self, shape, pad=256):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * pad,), _SENT, dtype=torch.float32, device="cuda")
        self.t = self.buf[pad:pad + n].view(*shape)
        self.pad, self.n = pad, n

    def check(self, what, written=True):
        assert bool((self.buf[:self.pad] == _SENT).all()), f"{what}: written in front of the output"
        assert bool((self.buf[self.pad + self.n:] == _SENT).all()), f"{what}: written past the end of the output"
        if written:
            assert not bool((self.t == _SENT).any()), f"{what}: an element of the output was never stored"


class _GuardedWorkspace:
    """Stand-in for models._Workspace: a fresh buffer of exactly the size asked for per call (so nothing carries over between
    two calls either), between two guard pages."""
    PAD = 4096

    def __init__(self):
        self.last = None

    def get(self, nbytes, device):
        self.last = (torch.full((nbytes + 2 * self.PAD,), 0xA5, dtype=torch.uint8, device=device), nbytes)
        return self.last[0][self.PAD:self.PAD + nbytes]

    def check(self, what):
        buf, n = self.last
        assert bool((buf[:self.PAD] == 0xA5).all()) and bool((buf[self.PAD + n:] == 0xA5).all()), f"{what}: written outside the workspace"


# ---------------------------------------------------------------------------------------------------------------------------
# egx_sample_prior: A = 1 and A = 33 (ragged last row tile; the N = 201 output layer's ragged columns; the GRU cell's in-place
# gi running sum over all 18 steps), against A = 64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prior():
    from egogen_amd.models import GAMMAPrimitiveCombo, PREDICTOR_CFG, REGRESSOR_CFG
    from oracle import nets
    g1, g2 = load_golden("cvae_ref.npz"), load_golden("regressor_ref.npz")
    sd = {"predictor." + k: v for k, v in rebuild_state_dict(g1, [g1["fill_seed"]], [""]).items()}
    sd.update({"regressor." + k: v for k, v in rebuild_state_dict(g2, [g2["fill_seed"]], [""], gains=[float(g2["fill_gain"])]).items()})
    combo = GAMMAPrimitiveCombo(PREDICTOR_CFG, REGRESSOR_CFG)
    combo.load_state_dict(sd, strict=True)
    combo.cuda()
    combo._ws = _GuardedWorkspace()
    gen = torch.Generator().manual_seed(7)
    A = 64
    X = torch.randn(2, A, 201, generator=gen) * 0.3
    z = torch.randn(A, 128, generator=gen)
    betas = torch.randn(A, 10, generator=gen)
    dev = {"X": X.cuda(), "z": z.cuda(), "betas": betas.cuda()}

    def call(a):
        Y, Yb = _Guarded((18, a, 201)), _Guarded((18, a, 93))
        combo.sample_prior_into(dev["X"][0, :a], dev["X"][1, :a], 201, dev["betas"][:a].contiguous(), dev["z"][:a].contiguous(), Y.t, Yb.t)
        torch.cuda.synchronize()
        Y.check(f"sample_prior A={a} Y"); Yb.check(f"sample_prior A={a} Yb"); combo._ws.check(f"sample_prior A={a}")
        return Y.t.clone(), Yb.t.clone()

    Yo, Ybo = nets.sample_prior(sd, X[:, :33], betas[None, :33].repeat(18, 1, 1), z[:33])   # rows are independent: row 0 serves A = 1
    return {"call": call, "big": call(64), "Yo": Yo, "Ybo": Ybo}


@pytest.mark.parametrize("A", [1, 33])
def test_sample_prior_small_batches(prior, A):
    from oracle.rot import tgm_angle_axis_to_rotation_matrix as aa2R
    Y, Yb = prior["call"](A)
    Yo, Ybo = prior["Yo"][:, :A], prior["Ybo"][:, :A]
    # tolerances of test_sample_prior_matches_oracle (rotations compared as matrices: axis-angle is discontinuous at pi)
    assert max_abs(Y.cpu(), Yo) < 1e-4 * max(1.0, float(Yo.abs().max()))
    assert max_abs(Yb.cpu()[..., :3], Ybo[..., :3]) < 2e-4 * max(1.0, float(Ybo[..., :3].abs().max()))
    assert max_abs(aa2R(Yb.cpu()[..., 3:69].reshape(-1, 3)), aa2R(Ybo[..., 3:69].reshape(-1, 3))) < 2e-4
    assert max_abs(Yb.cpu()[..., 69:], Ybo[..., 69:]) < 2e-4 * max(1.0, float(Ybo[..., 69:].abs().max()))
    # the same agents inside a 64-agent call: the same bits
    Y64, Yb64 = prior["big"]
    assert torch.equal(Y, Y64[:, :A]) and torch.equal(Yb, Yb64[:, :A])
    # and the same call again
    Y2, Yb2 = prior["call"](A)
    assert torch.equal(Y, Y2) and torch.equal(Yb, Yb2)


# ---------------------------------------------------------------------------------------------------------------------------
# egx_policy_forward at n = 33: three arithmetic modes x (actor, critic, both) = single, pair and triple launches, the N = 1 head
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def policy():
    from egogen_amd.models import ActorCritic, GAMMAActor, GAMMACritic, GAMMAPolicyBase, POLICY_CFG, PolicyHipRunner
    from oracle import nets
    g = load_golden("policy_ref.npz")
    sd = rebuild_state_dict(g, g["fill_seeds"], ["shared_net.", "actor.", "critic."], gains=[1.0, 1.4, 1.4])
    ac = ActorCritic(GAMMAActor(POLICY_CFG), GAMMACritic(POLICY_CFG), GAMMAPolicyBase(POLICY_CFG))
    ac.load_state_dict(sd, strict=True)
    ac.cuda()
    run = PolicyHipRunner(ac.shared_net, ac.actor, ac.critic)
    run._ws = _GuardedWorkspace()
    gen = torch.Generator().manual_seed(1)
    n = 64
    obs = {"state": torch.randn(n, 2, 402, generator=gen) * 0.3, "egosensing": torch.rand(n, 2, 32, generator=gen) * 2 - 1,
           "dist": torch.rand(n, generator=gen), "time": torch.rand(n, generator=gen)}
    o33 = {k: v[:33] for k, v in obs.items()}
    hx = nets.policy_base(sd, o33)
    mu, logvar = nets.policy_actor(sd, hx)
    ref = {"mu": mu, "logvar": logvar, "value": nets.policy_critic(sd, hx).reshape(-1)}
    return {"run": run, "obs": {k: v.cuda() for k, v in obs.items()}, "ref": ref}


def _policy_call(policy, n, actor, critic):
    out, guards = {}, {}
    if actor:
        guards["mu"], guards["logvar"] = _Guarded((n, 128)), _Guarded((n, 128))
    if critic:
        guards["value"] = _Guarded((n,))
    out = {k: gd.t for k, gd in guards.items()}
    policy["run"].forward({k: v[:n].contiguous() for k, v in policy["obs"].items()}, want_actor=actor, want_critic=critic, out=out)
    torch.cuda.synchronize()
    for k, gd in guards.items():
        gd.check(f"policy_forward n={n} {k}")
    policy["run"]._ws.check(f"policy_forward n={n}")
    return {k: gd.t.clone() for k, gd in guards.items()}


@pytest.mark.parametrize("heads", ["actor", "critic", "both"])
@pytest.mark.parametrize("prec", [0, 2, 1])
def test_policy_forward_small_batch(policy, prec, heads):
    from egogen_amd import _lib
    lib = _lib.load()
    actor, critic = heads != "critic", heads != "actor"
    try:
        _lib.check(lib.egx_policy_set_precision(prec), "egx_policy_set_precision")
        out = _policy_call(policy, 33, actor, critic)
        again = _policy_call(policy, 33, actor, critic)
        big = _policy_call(policy, 64, actor, critic)
    finally:
        _lib.check(lib.egx_policy_set_precision(0), "egx_policy_set_precision")
    assert set(out) == ({"mu", "logvar"} if actor else set()) | ({"value"} if critic else set())
    for k, v in out.items():
        ref = policy["ref"][k]
        if prec != 1:
            # test_policy_matches_reference_golden: 1e-4 relative in the fp32-equivalent and the two-term arithmetic
            err = max_abs(v.cpu(), ref) / max(1.0, float(ref.abs().max()))
            assert err < 1e-4, (k, err)
        else:
            # test_policy_bf16_mode_is_close_to_fp32_and_restorable: operands rounded to bf16 - within bf16 round-off on average
            err = float((v.cpu() - ref).abs().mean()) / (float(ref.abs().mean()) + 1e-6)
            assert err < 3e-2, (k, err)
        assert torch.equal(v, again[k]), k
        assert torch.equal(v, big[k][:33]), k


# ---------------------------------------------------------------------------------------------------------------------------
# egx_policy_train_step at n = 32 and n = 64 in both update arithmetics: residual, saved activation, act' of a saved
# activation, the weight-gradient launches' n_split / bias_out, both GRU-backward launches
# ---------------------------------------------------------------------------------------------------------------------------
_POLICIES = {}


def _train_policy(mode):
    from tests.test_trainer_gpu import _Args, _build_policy_one_thread
    if mode not in _POLICIES:
        a = _Args()
        a.update_precision = mode
        pol = _build_policy_one_thread(a)
        assert pol.update_precision == mode
        with torch.no_grad():   # as test_train_step_matches_torch_autograd: non-trivial biases, some logvars outside the clamp range
            for p_ in pol.parameters():
                if p_.dim() == 1:
                    p_.add_(0.05 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(p_.numel())).cuda())
            pol.actor.pnet.out_fc.bias[128:160] += 4.0
            pol.actor.pnet.out_fc.bias[160:192] -= 4.0
        _POLICIES[mode] = pol
    return _POLICIES[mode]


@pytest.mark.parametrize("N", [32, 64])
@pytest.mark.parametrize("mode", ["f32", "bf16x2"])
def test_train_step_small_minibatches(mode, N):
    """The yardstick of test_train_step_matches_torch_autograd: loss terms and every parameter gradient of the plain torch
    expression, with that test's bounds (2e-4 on the terms, _assert_grads_close on the gradients)."""
    from egogen_amd import models
    from tests.test_trainer_gpu import _assert_grads_close, _filled_batch
    pol = _train_policy(mode)
    b = _filled_batch(1, N, N, pol)
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
    # every gradient is WRITTEN by the step; the alignment padding between the tensors of the flat buffer belongs to nobody
    covered = torch.zeros(pol._flat_grad.numel(), dtype=torch.bool, device="cuda")
    for _, off, n in pol._flat_layout():
        covered[off:off + n] = True
    assert int((~covered).sum()) > 0
    idx = torch.arange(N, device="cuda")
    assert pol._train_handle(N) is not None, "the hand-written update step was not selected"
    runs = []
    for _ in range(2):
        pol._flat_grad.fill_(_SENT)
        log = _Guarded((6,))
        log.t.zero_()
        assert pol._fwd_bwd(b, idx, None, log.t) == "chain"
        torch.cuda.synchronize()
        log.check(f"train_step {mode} N={N} loss terms")
        assert bool((pol._flat_grad[~covered] == _SENT).all()), "a gradient launch wrote into the padding of the flat buffer"
        assert not bool((pol._flat_grad[covered] == _SENT).any()), "an element of a gradient was never stored"
        runs.append((pol._flat_grad.clone(), log.t.cpu().tolist()))
    # the loss terms are sums by floating-point atomics over the loss kernel's workgroups (csrc/ppo.hip, not a dense3 launch):
    # their last bit may depend on the order, so the bit-for-bit claim is made for what the dense3 / gru3 launches write
    assert torch.equal(runs[0][0], runs[1][0])
    log = runs[0][1]
    for i, k in enumerate(("loss", "loss/clip", "loss/vf", "loss/ent", "loss/kld", "approx_kl")):
        assert abs(log[i] - ref_terms[k]) <= 2e-4 * max(1.0, abs(ref_terms[k])), (k, log[i], ref_terms[k])
    for n_, p_ in pol.named_parameters():
        if n_.startswith("_actor_critic."):
            continue
        _assert_grads_close(n_, p_.grad, ref[n_])
