"""The fp32 yardstick of the rollout-side networks (shared by test_fp32_yardstick_cpu.py and test_fp32_equivalence_gpu.py).

egx_policy_forward at precision 0, egx_sample_prior and egx_vposer_encode carry every fp32 operand of a matrix product as three
bf16 planes (csrc/d3.h), which is claimed to be fp32-equivalent.  The claim is held to what fp32 itself costs on the same
weights and inputs: the oracle (oracle/nets.py) is evaluated in float64 and in float32, and per output group

    bound = R * max|oracle32 - oracle64| + 2^-23 * max|oracle64|          R = 3 (test_trainer_gpu.py: _P3_MODES["f32"])

(the second term: one ulp of the fp32 store of the result).  So that the bound can be shown to tell three planes from two, the
oracle can also be run with both operands of every product truncated to the first k bf16 planes (`truncated_products`).

No GPU needed to import; nothing here is a pytest fixture or setting.
"""
import contextlib
import functools
import os

import torch

from oracle import nets
from oracle.rot import tgm_angle_axis_to_rotation_matrix as aa2R
from tests.helpers import load_golden, rebuild_state_dict

R = 3.0
ULP = 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle in a chosen dtype, and with truncated operands
# ---------------------------------------------------------------------------------------------------------------------------
def _cast(v, dtype):
    if isinstance(v, torch.Tensor):
        return v.to(dtype) if v.is_floating_point() else v
    if isinstance(v, dict):
        return {k: _cast(x, dtype) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return type(v)(_cast(x, dtype) for x in v)
    return v


def oracle_eval(fn, sd, inputs, dtype):
    """fn(sd, *inputs) with every floating-point tensor of sd and inputs in `dtype` (the functions of oracle/nets.py compute in
    the dtype of what they are given)."""
    with torch.no_grad():
        return fn(_cast(sd, dtype), *_cast(tuple(inputs), dtype))


def planes(x, k):
    """x (fp32) rounded to the sum of its first k bf16 planes: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)
    (round to nearest even; the residuals are exact in fp32), returned in float64."""
    assert x.dtype == torch.float32
    r, s = x, torch.zeros_like(x, dtype=torch.float64)
    for _ in range(k):
        p = r.to(torch.bfloat16).to(torch.float32)
        s, r = s + p.double(), r - p
    return s


def _product(x, w, k):
    """x @ w^T with both operands cut to k planes, formed in float64 and rounded to fp32."""
    return (planes(x, k) @ planes(w, k).t()).to(torch.float32)


@contextlib.contextmanager
def truncated_products(k, only=None):
    """While active, nets.linear and nets.gru_cell (called with fp32 tensors) cut both operands of every product to k bf16
    planes, form the product in float64, round it to fp32 and add the fp32 bias: the arithmetic of `prec 0` (k = 3) and
    `prec 2` (k = 2) without their accumulation order.  only: a predicate on the layer (linear: its state-dict prefix; GRU
    cell: the tuple of weight shapes) choosing the layers that are cut - the others keep plain fp32 - to localise an error."""
    lin0, gru0 = nets.linear, nets.gru_cell

    def linear(x, sd, prefix):
        if only is not None and not only(prefix):
            return lin0(x, sd, prefix)
        return _product(x, sd[prefix + ".weight"], k) + sd[prefix + ".bias"]

    def gru_cell(x, h, w_ih, w_hh, b_ih, b_hh):
        if only is not None and not only((tuple(w_ih.shape), tuple(w_hh.shape))):
            return gru0(x, h, w_ih, w_hh, b_ih, b_hh)
        H = h.shape[-1]
        gi, gh = _product(x, w_ih, k) + b_ih, _product(h, w_hh, k) + b_hh
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        return (1 - z) * n + z * h

    nets.linear, nets.gru_cell = linear, gru_cell
    try:
        yield
    finally:
        nets.linear, nets.gru_cell = lin0, gru0


# ---------------------------------------------------------------------------------------------------------------------------
# output groups
# ---------------------------------------------------------------------------------------------------------------------------
def _policy_fn(sd, obs):
    hx = nets.policy_base(sd, obs)
    mu, logvar = nets.policy_actor(sd, hx)
    return {"mu": mu, "logvar": logvar, "value": nets.policy_critic(sd, hx).reshape(-1)}


def prior_groups(Y, Yb):
    """Y[18,A,201], Yb[18,A,93] (any float dtype, any device) -> the groups in float64 on the CPU; the rotations as matrices
    (axis-angle is discontinuous at pi)."""
    Y, Yb = Y.detach().cpu().double(), Yb.detach().cpu().double()
    return {"Y": Y, "transl": Yb[..., :3], "rot": aa2R(Yb[..., 3:69].reshape(-1, 3)), "hands": Yb[..., 69:]}


def _prior_fn(sd, X, betas, z):
    return prior_groups(*nets.sample_prior(sd, X, betas, z))


def _vposer_fn(sd, x):
    return {"mean": nets.vposer_encode(sd, x)}


def _f64(out):
    return {k: v.detach().cpu().double() for k, v in out.items()}


class Case:
    """One network on one set of weights and inputs: the oracle in float64 and float32, the bound per group."""

    def __init__(self, name, fn, sd, inputs):
        self.name, self.fn, self.sd, self.inputs = name, fn, sd, inputs
        self.o64 = _f64(oracle_eval(fn, sd, inputs, torch.float64))
        self.o32 = _f64(oracle_eval(fn, sd, inputs, torch.float32))
        self.groups = tuple(self.o64)
        self.scale = {g: float(self.o64[g].abs().max()) for g in self.groups}
        self.err32 = {g: float((self.o32[g] - self.o64[g]).abs().max()) for g in self.groups}
        assert all(self.err32[g] > 0 and self.scale[g] > 0 for g in self.groups)

    def bound(self, group, r=R):
        return r * self.err32[group] + ULP * self.scale[group]

    def error(self, out, rows=None):
        """max|out - oracle64| per group of `out`; rows: out holds these rows (agents / observations) of the case only."""
        res = {}
        for g, v in _f64(out).items():
            ref = self.o64[g] if rows is None else rows(g, self.o64[g])
            assert v.shape == ref.shape, (g, v.shape, ref.shape)
            res[g] = float((v - ref).abs().max())
        return res

    def emulated(self, k, only=None):
        """The fp32 oracle with the operands of its products cut to k planes."""
        with truncated_products(k, only):
            return _f64(oracle_eval(self.fn, self.sd, self.inputs, torch.float32))


# Weights and inputs: those of test_dense3_epilogue_gpu.py (policy_ref.npz, seed 1, the first 33 of 64 observations; cvae_ref.npz
# + regressor_ref.npz, seed 7, the first 33 of 64 agents) and of test_vposer_encoder_matches_oracle (seeded_fill 105, n = 100).
POLICY_N, PRIOR_A, VPOSER_N = 33, 33, 100


def policy_state_dict():
    g = load_golden("policy_ref.npz")
    return rebuild_state_dict(g, g["fill_seeds"], ["shared_net.", "actor.", "critic."], gains=[1.0, 1.4, 1.4])


def prior_state_dict():
    g1, g2 = load_golden("cvae_ref.npz"), load_golden("regressor_ref.npz")
    sd = {"predictor." + k: v for k, v in rebuild_state_dict(g1, [g1["fill_seed"]], [""]).items()}
    sd.update({"regressor." + k: v for k, v in rebuild_state_dict(g2, [g2["fill_seed"]], [""], gains=[float(g2["fill_gain"])]).items()})
    return sd


def vposer_state_dict():
    from egogen_amd.models import VPoserEncoder
    from egogen_amd.synth import seeded_fill
    vals = seeded_fill({k: tuple(v.shape) for k, v in VPoserEncoder().state_dict().items()}, 105)
    vals = {k: torch.from_numpy(v) for k, v in vals.items()}
    vals["bodyprior_enc_bn1.num_batches_tracked"] = torch.tensor(0)
    vals["bodyprior_enc_bn2.num_batches_tracked"] = torch.tensor(0)
    return vals


@functools.lru_cache(maxsize=None)
def policy_case():
    gen = torch.Generator().manual_seed(1)
    n = 64
    obs = {"state": torch.randn(n, 2, 402, generator=gen) * 0.3, "egosensing": torch.rand(n, 2, 32, generator=gen) * 2 - 1,
           "dist": torch.rand(n, generator=gen), "time": torch.rand(n, generator=gen)}
    return Case("policy", _policy_fn, policy_state_dict(), ({k: v[:POLICY_N].contiguous() for k, v in obs.items()},))


@functools.lru_cache(maxsize=None)
def prior_case():
    gen = torch.Generator().manual_seed(7)
    A = 64
    X = torch.randn(2, A, 201, generator=gen) * 0.3
    z = torch.randn(A, 128, generator=gen)
    betas = torch.randn(A, 10, generator=gen)
    a = PRIOR_A
    return Case("prior", _prior_fn, prior_state_dict(), (X[:, :a].contiguous(), betas[None, :a].repeat(18, 1, 1), z[:a].contiguous()))


@functools.lru_cache(maxsize=None)
def vposer_case():
    x = torch.randn(VPOSER_N, 63, generator=torch.Generator().manual_seed(1)) * 0.3
    return Case("vposer", _vposer_fn, vposer_state_dict(), (x,))


# ---------------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------------
def table(case, title, columns):
    """columns: {heading: {group: max|x - oracle64|}} -> lines of text, every error next to its ratio to the fp32 oracle's."""
    lines = [f"# {title}", "# group            max|f64|   |f32-f64|      bound" + "".join(f"  {h:>22s}" for h in columns)]
    for g in case.groups:
        row = f"{case.name + ' ' + g:16s} {case.scale[g]:10.3e} {case.err32[g]:11.3e} {case.bound(g):10.3e}"
        for col in columns.values():
            row += f"  {col[g]:10.3e} ({col[g] / case.err32[g]:7.2f} x)" if g in col else " " * 24
        lines.append(row)
    return lines


def emit(lines, env="EGX_F32_TABLE"):
    """Print the table; append it to the file that the environment variable names, if it names one."""
    print("\n".join(lines))
    out = os.environ.get(env)
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
